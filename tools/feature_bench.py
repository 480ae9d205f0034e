#!/usr/bin/env python3
"""The DNN front end of a training batch at 8 kHz: FeatureExtractor.extract_frame_features + add_context ([B, T, 594] from
[B, L]), and MeddisHairCell.process_to_frames on GammatoneFilterbank.filter's [B, 64, L], at B 64 x 4 s and B 256 x 4 s.

Synchronised wall time of each whole call (host clock around work that ends in a device synchronise; median and spread of
`rounds` calls after a warm-up of every shape), then - in a pass of its own - device events around every launch (ops.profiler)
next to the roofline its wrapper states: the larger of flops over the peak rate (157.3 TFLOP/s for the fp32 matrix instruction of
the framed GEMM and the FIR bank, 78.6 TFLOP/s vector fp64 for the hair cell, 157.3 TFLOP/s vector fp32 otherwise) and bytes over
8 TB/s.  The hair cell and the RASTA kernel are chains (latency-bound): their floors are far below any time they can reach, and
are printed for completeness.

    python tools/feature_bench.py [--B 64 256] [--seconds 4] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.signal_processing import FeatureExtractor, MeddisHairCell  # noqa: E402

HBM_BYTES_S = 8.0e12
PEAK = {"framed_gemm_f32": 157.3e12, "gammatone_tf": 157.3e12, "gammatone_fir": 157.3e12, "cepstral": 157.3e12, "rasta": 78.6e12,
        "feature_context": 157.3e12, "haircell_frames": 78.6e12}


def timed(fn, rounds):
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def launches(fn):
    """per family: launches, device-event ms, the wrapper's flops and bytes, and the roofline floor they give"""
    ops.profiler.enable(set(PEAK))
    fn()
    rows = {}
    for name, d in ops.profiler.summary().items():
        floor = max(d["flops"] / PEAK[name], d["bytes"] / HBM_BYTES_S) * 1e3
        rows[name] = {"n": d["n"], "ms": round(d["ms_total"], 4), "gflop": round(d["flops"] / 1e9, 3), "mbyte": round(d["bytes"] / 1e6, 3),
                      "floor_ms": round(floor, 4), "bound": "flops" if d["flops"] / PEAK[name] > d["bytes"] / HBM_BYTES_S else "bytes"}
    ops.profiler.disable()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_bench: needs the GPU (a CPU timing says nothing about it)")
    fe, hc = FeatureExtractor(), MeddisHairCell()
    L = int(a.seconds * fe.fs)
    gen = torch.Generator(device="cuda").manual_seed(23)
    res = {"L": L, "fs": fe.fs, "rounds": a.rounds, "shapes": {}}
    for B in a.B:
        wave = 0.1 * torch.randn(B, L, device="cuda", generator=gen)
        front = lambda: fe.add_context(fe.extract_frame_features(wave))
        y = fe.gfb.filter(wave)                                  # the hair cell's input: [B, 64, L] fp32
        cell = lambda: hc.process_to_frames(y)
        for _ in range(2):                                        # warm-up of both shapes
            f, c = front(), cell()
        torch.cuda.synchronize()
        shape = {"features": list(f.shape), "haircell_frames": list(c.shape)}
        del f, c
        shape["front_end_wall"] = timed(front, a.rounds)
        shape["haircell_wall"] = timed(cell, a.rounds)
        shape["front_end_launches"] = launches(front)
        shape["haircell_launches"] = launches(cell)
        res["shapes"]["B%d" % B] = shape
        del wave, y
    print(json.dumps(res))


if __name__ == "__main__":
    main()
