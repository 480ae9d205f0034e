#!/usr/bin/env python3
"""curriculum_batch at the c3se training shape (B 256 x 64 000 samples, mask 'pcirm'): the whole call, its launches one by one
(sfm_mix_scale, sfm_mix_apply with the noise rows, sfm_curriculum_mask) and what a training step pays for its spectra without
it: two functional.stft calls at the same shape (the STFT path is the one curriculum_batch itself calls).  All variants run in
one process in alternating rounds (device events around `iters` back-to-back calls after a warm-up of every shape); the median
round is reported with the spread, next to the bytes each launch has to move (each operand read once, each result written
once) and the share of the 8.0 TB/s HBM peak they imply.

    python tools/curriculum_batch_bench.py [--B 256] [--L 64000] [--mask pcirm] [--iters 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import config, functional as Fn, ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp  # noqa: E402

HBM_PEAK_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--L", type=int, default=64000)
    ap.add_argument("--mask", default="pcirm", choices=["irm", "pcirm", "opt_pcirm", "none"])
    ap.add_argument("--noises", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curriculum_batch_bench: needs the GPU (a CPU timing says nothing about it)")
    B, L = a.B, a.L
    kind = None if a.mask == "none" else a.mask
    g = torch.Generator(device="cuda").manual_seed(0)
    clean = 0.1 * torch.randn(B, L, device="cuda", generator=g)
    noises = [0.3 * torch.randn(24000 + 9000 * i, device="cuda", generator=g) for i in range(a.noises)]    # 3 s .. 10.9 s at 8 kHz
    snr_levels = [-5, 0, 5, 10]
    bank = cp.noise_bank(noises)
    ids, snr = cp.mix_assignment(B, bank.count, snr_levels)
    _, ids, snr, _ = cp._mix_args("bench", clean, bank, ids, snr, None)
    fft, hop, win = config.FFT_SIZE, config.HOP_SIZE, config.FRAME_SIZE
    T, F = 1 + L // hop, fft // 2 + 1
    scale = ops.mix_scale(clean, bank.buffer, bank.offsets, ids, snr)
    noisy, rows = ops.mix_apply(clean, bank.buffer, bank.offsets, ids, scale, want_rows=True)
    cr, ci = Fn.stft(clean, fft, hop, win)
    nr, ni = Fn.stft(rows, fft, hop, win)
    n = B * T * F
    table, M = (None, 0)
    if kind == "opt_pcirm":
        from sincformer_metacog_speech_enhancement_amd.masks.opt_pcirm import compute_snr_boundaries, quantizer_table
        table, M = quantizer_table(compute_snr_boundaries()[0], None, "cuda")

    def two_stfts():
        Fn.stft(noisy, fft, hop, win)
        Fn.stft(clean, fft, hop, win)

    variants = {
        "curriculum_batch": (lambda: cp.curriculum_batch(clean, bank, snr_levels, kind), None),
        "two_stft_calls": (two_stfts, None),
        "mix_scale": (lambda: ops.mix_scale(clean, bank.buffer, bank.offsets, ids, snr), 8.0 * B * L),
        "mix_apply_rows": (lambda: ops.mix_apply(clean, bank.buffer, bank.offsets, ids, scale, want_rows=True), 16.0 * B * L),
        "curriculum_mask": (lambda: ops.curriculum_mask(cr, ci, nr, ni, scale, kind, table=table, M=M), (28.0 if kind else 24.0) * n),
    }
    # linearity on these inputs: the kernel's spectrum of the mix against the STFT of the mixed waveform
    yr, yi, _ = ops.curriculum_mask(cr, ci, nr, ni, scale, kind, table=table, M=M)
    sr, si = Fn.stft(noisy, fft, hop, win)
    peak = float(torch.maximum(sr.abs().max(), si.abs().max()))
    check = {"spectrum_by_linearity_max_abs_err_over_peak": float(torch.maximum((yr - sr).abs().max(), (yi - si).abs().max())) / peak}
    for fn, _ in variants.values():                         # warm-up: every shape, every code object, the clock ramp
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.iters)
    out = {"B": B, "L": L, "T": T, "F": F, "mask": a.mask, "iters": a.iters, "rounds": a.rounds, "check": check, "variants": {}}
    for k, (_, nbytes) in variants.items():
        ms = statistics.median(times[k])
        row = {"ms_median": round(ms, 5), "ms_min": round(min(times[k]), 5), "ms_max": round(max(times[k]), 5)}
        if nbytes is not None:
            row["MB_moved"] = round(nbytes / 1e6, 2)
            row["TBps"] = round(nbytes / ms / 1e9, 3)
            row["share_of_hbm_peak"] = round(nbytes / ms / 1e9 / HBM_PEAK_TBPS, 3)
        out["variants"][k] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
