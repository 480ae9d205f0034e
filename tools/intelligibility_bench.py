#!/usr/bin/env python3
"""CSII and NCM of a test batch on the device: evaluation.compute_csii and evaluation.compute_ncm on B 64 x 4 s at 8 kHz
(64 x 32 000 samples; NCM: 64 gammatone channels x 400 taps, then the O(L^2) Hilbert transform on the fp32 matrix cores).
Synchronised wall time of each call (host clock around work that ends in a device synchronise; median and spread of `rounds`
calls after a warm-up), then - in a pass of its own - device events around every launch (ops.profiler).  Beside the Hilbert
kernel's time its floor: 2 x 128 columns x L x (L / 2 for an even L, else L) FLOP per utterance at 157.3 TFLOP/s.  For comparison the reference's procedure
on the host for ONE utterance, in float64: scipy's fftconvolve and FFT-based hilbert per channel, numpy's rfft per frame.

    python tools/intelligibility_bench.py [--B 64] [--seconds 4] [--rounds 7] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import evaluation, ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.evaluation import csii, ncm  # noqa: E402

MFMA_F32_FLOPS = 157.3e12
FAMILIES = {"hilbert_env", "intelligibility", "gammatone_fir", "framed_gemm_f32_varlen"}


def host_ncm(gfb, c, e):
    from scipy.signal import fftconvolve, hilbert
    L = len(c)
    env = [np.abs(hilbert(np.stack([fftconvolve(s, h, mode="full")[:L] for h in gfb.impulse_responses]), axis=-1)) for s in (c, e)]
    a, b = (v - v.mean(axis=1, keepdims=True) for v in env)
    den = np.sqrt((a * a).mean(1) * (b * b).mean(1))
    ncc = np.where(den < 1e-10, 0.0, np.clip((a * b).mean(1) / np.maximum(den, 1e-300), -1, 1))
    return float(np.clip(np.sum(ncm.channel_weights(gfb.center_freqs) * np.maximum(ncc, 0)), 0, 1))


def host_csii(c, e, fs):
    frame, hop = csii.csii_framing(fs)
    w = np.hamming(frame)
    T = (len(c) - frame) // hop + 1
    X = np.stack([np.fft.rfft(c[t * hop:t * hop + frame] * w, n=256) for t in range(T)])
    Y = np.stack([np.fft.rfft(e[t * hop:t * hop + frame] * w, n=256) for t in range(T)])
    pxx, pyy, pxy = (np.abs(X) ** 2).mean(0), (np.abs(Y) ** 2).mean(0), (X * np.conj(Y)).mean(0)
    return float(np.clip(np.sum(csii.sii_weights(fs) * np.clip(np.abs(pxy) ** 2 / (pxx * pyy + 1e-10), 0, 1)), 0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intelligibility_bench: needs the GPU (a CPU timing says nothing about it)")
    fs = 8000
    gfb = ncm.default_bank(fs)
    L = int(a.seconds * fs)
    gen = torch.Generator(device="cuda").manual_seed(23)
    t = torch.arange(L, device="cuda") / fs
    clean = 0.5 * (1 + 0.5 * torch.sin(2 * np.pi * 7 * t)) * torch.sin(2 * np.pi * 440 * t) + 0.05 * torch.randn(a.B, L, device="cuda",
                                                                                                            generator=gen)
    enh = 0.8 * clean + 0.15 * torch.randn(a.B, L, device="cuda", generator=gen)
    calls = {"ncm": lambda: evaluation.compute_ncm(clean, enh, fs), "csii": lambda: evaluation.compute_csii(clean, enh, fs)}
    res = {"B": a.B, "L": L, "fs": fs, "C": gfb.num_channels}
    scores = {}
    for name, fn in calls.items():
        for _ in range(2):
            scores[name] = fn()
        torch.cuda.synchronize()
        wall = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            del out
        ops.profiler.enable(FAMILIES)
        fn()
        split = {k: round(v["ms_total"], 4) for k, v in ops.profiler.summary().items()}
        ops.profiler.disable()
        res[name] = {"ms_median": round(statistics.median(wall), 3), "ms_min": round(min(wall), 3), "ms_max": round(max(wall), 3),
                     "device_event_split_ms": split, "mean_score": round(float(scores[name].mean()), 6)}
    flops = 2.0 * 128 * float(L) * int(ops.hilbert_conv_len(L)) * a.B     # an even L: two convolutions of L / 2 samples
    hil = res["ncm"]["device_event_split_ms"].get("hilbert_env", 0.0)
    res["hilbert_flop"] = flops
    res["hilbert_floor_mfma_f32_ms"] = round(flops / MFMA_F32_FLOPS * 1e3, 3)
    res["hilbert_share_of_ncm_wall"] = round(hil / res["ncm"]["ms_median"], 3)
    res["hilbert_fraction_of_fp32_matrix_peak"] = round(flops / (hil * 1e-3) / MFMA_F32_FLOPS, 3) if hil else None
    if not a.no_host:
        c, e = clean[0].cpu().numpy().astype(np.float64), enh[0].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        hn = host_ncm(gfb, c, e)
        res["host_ncm_one_utterance_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        hc = host_csii(c, e, fs)
        res["host_csii_one_utterance_s"] = round(time.perf_counter() - t0, 4)
        res["host_minus_device_utterance0"] = {"ncm": hn - float(scores["ncm"][0]), "csii": hc - float(scores["csii"][0])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
