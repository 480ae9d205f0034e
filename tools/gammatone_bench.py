#!/usr/bin/env python3
"""The gammatone T-F analysis of a training batch: GammatoneFilterbank.get_tf_magnitudes over the clean, noise and noisy
waveforms of B 256 x 4 s at 8 kHz in ONE call (768 x 32 000 samples, 64 channels x 400 taps, frames 160 / 80, N 256).
  fused     sfm_gammatone_tf + sfm_gammatone_tf_finish: the filtered signal never leaves the chip;
  unfused   sfm_gammatone_fir ([3B, 64, L] fp32 in HBM) + sfm_gammatone_moments + sfm_gammatone_tf_finish;
  host      the reference's procedure in numpy for ONE utterance: an fftconvolve per channel, an rfft per (channel, frame).
Synchronised wall time of the whole call (host clock around work that ends in a device synchronise; median and spread of
`rounds` calls after a warm-up, the two routes alternating), then - in a pass of its own - device events around every launch
(ops.profiler).  Beside the times the floors: the fp32 MFMA time of 2 * 64 * K FLOP per sample at 157.3 TFLOP/s and the HBM
time of the route's bytes per sample (fused 4 read + 16 written, unfused about 516) at 8 TB/s.

    python tools/gammatone_bench.py [--B 256] [--seconds 4] [--rounds 7] [--no-host]
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

from sincformer_metacog_speech_enhancement_amd import config, ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.signal_processing import GammatoneFilterbank  # noqa: E402

MFMA_F32_FLOPS, HBM_BYTES_S = 157.3e12, 8.0e12
FAMILIES = {"gammatone_tf", "gammatone_fir", "gammatone_moments", "gammatone_tf_finish"}


def host_tf(gfb, x, frame, hop, N):
    """the reference's procedure: per-channel linear convolution cut to L, frames without a window, one rfft per unit"""
    from scipy.signal import fftconvolve
    L = len(x)
    y = np.stack([fftconvolve(x, h, mode="full")[:L] for h in gfb.impulse_responses])
    T = (L - frame) // hop + 1
    mag, ph = np.zeros((len(y), T)), np.zeros((len(y), T))
    bins = gfb.cf_bins(N)
    for c in range(len(y)):
        for n in range(T):
            S = np.fft.rfft(y[c, n * hop:n * hop + frame], n=N)
            mag[c, n] = np.sum(np.abs(S) ** 2)
            ph[c, n] = np.angle(S[bins[c]])
    return mag, ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gammatone_bench: needs the GPU (a CPU timing says nothing about it)")
    gfb = GammatoneFilterbank()
    L = int(a.seconds * gfb.sample_rate)
    gen = torch.Generator(device="cuda").manual_seed(19)
    clean = 0.1 * torch.randn(a.B, L, device="cuda", generator=gen)
    noise = 0.05 * torch.randn(a.B, L, device="cuda", generator=gen)
    batch = torch.cat([clean, noise, clean + noise])
    frame, hop, N = config.FRAME_SIZE, config.HOP_SIZE, config.FFT_SIZE
    K = len(gfb.impulse_responses[0])

    def run(fused):
        ops.set_gammatone_fused(fused)
        try:
            return gfb.get_tf_magnitudes(batch)
        finally:
            ops.set_gammatone_fused(True)

    for _ in range(2):
        f, u = run(True), run(False)
    torch.cuda.synchronize()
    agree = float((f[0] - u[0]).abs().max() / u[0].abs().max())
    del f, u
    wall = {True: [], False: []}
    for _ in range(a.rounds):
        for fused in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(fused)
            torch.cuda.synchronize()
            wall[fused].append((time.perf_counter() - t0) * 1e3)
            del out
    split = {}
    for fused in (True, False):
        ops.profiler.enable(FAMILIES)
        run(fused)
        split["fused" if fused else "unfused"] = {k: round(v["ms_total"], 4) for k, v in ops.profiler.summary().items()}
        ops.profiler.disable()
    samples = float(batch.numel())
    res = {"signals": batch.shape[0], "L": L, "C": gfb.num_channels, "taps": K, "frame": frame, "hop": hop, "fft": N,
           "fused_ms_median": round(statistics.median(wall[True]), 3), "fused_ms_min": round(min(wall[True]), 3),
           "fused_ms_max": round(max(wall[True]), 3),
           "unfused_ms_median": round(statistics.median(wall[False]), 3), "unfused_ms_min": round(min(wall[False]), 3),
           "unfused_ms_max": round(max(wall[False]), 3),
           "device_event_split_ms": split, "routes_max_rel_diff_mag": agree,
           "floor_mfma_f32_ms": round(2.0 * 64 * K * samples / MFMA_F32_FLOPS * 1e3, 3),
           "floor_hbm_fused_ms": round(20.0 * samples / HBM_BYTES_S * 1e3, 3),
           "floor_hbm_unfused_ms": round(516.0 * samples / HBM_BYTES_S * 1e3, 3)}
    if not a.no_host:
        x = clean[0].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        host_tf(gfb, x, frame, hop, N)
        res["host_numpy_one_utterance_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
