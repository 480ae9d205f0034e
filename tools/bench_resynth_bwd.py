#!/usr/bin/env python3
"""The resynthesis' adjoint in the mask (csrc/resynth.hip, sfm_mask_resynth_bwd) at B 64 x 4 s and B 256 x 4 s, 8 kHz, the default
framing (frame 160, hop 80, n_fft 256, 64 channels), T_mask = T.

  backward   one ops.mask_resynth_bwd launch
  forward    one ops.mask_resynth launch at the same shape, in the same process
  torch      the same gradient from torch autograd through a composition of torch ops on the kernel's own operands: unfold,
             matmul with Wf, the gain gathered from the mask by the interpolation table, matmul with Wi, fold, times 1 / wsum.
             torch_backward times torch.autograd.grad on a kept graph (the backward alone), torch_both the forward with it.

Every launch is timed on its own with device events; the arms alternate launch by launch after a warm-up of each; per arm the
median over `launches` (at least 200) and the minimum and maximum, in microseconds.  The two ratios the issue asks for:
backward / forward and torch_backward / backward.  For the backward launch also the bytes and flops its wrapper states over the
median time and its share of the larger of the two hardware bounds (HBM 8 TB/s, fp32 matrix 157.3 TFLOP/s), and the largest
difference between the kernel's gradient and torch's relative to the largest element.  One JSON line per batch size.

    python tools/bench_resynth_bwd.py [--batches 64 256] [--seconds 4] [--launches 200]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import config, ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.signal_processing.gammatone import erb_space  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12


def alternate(arms, launches, warmup=5):
    """arms: {name: fn} -> {name: [ms of each launch]}"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(launches):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def row(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2)}


def one_batch(B, seconds, launches):
    fs, frame, hop, n_fft, C = config.SAMPLE_RATE, config.FRAME_SIZE, config.HOP_SIZE, config.FFT_SIZE, config.NUM_CHANNELS
    L = int(seconds * fs)
    T = (L - frame) // hop + 1
    cf = np.asarray(erb_space(config.FREQ_LOW, config.FREQ_HIGH, C), dtype=np.float64)
    gen = torch.Generator(device="cuda").manual_seed(31)
    noisy = torch.randn(B, L, device="cuda", generator=gen) * 0.1
    mask = torch.rand(B, T, C, device="cuda", generator=gen)
    dout = torch.randn(B, L, device="cuda", generator=gen)
    kw = dict(frame=frame, hop=hop, n_fft=n_fft, fs=fs, cf=cf)
    out = torch.empty(B, L, device="cuda")
    dmask = torch.empty(B, T, C, device="cuda")

    Wf, Wi, tab_idx, tab_wt, inv_wsum = ops.resynth_operands(frame, hop, n_fft, fs, cf, noisy.device)
    lo = tab_idx.long()
    scale = torch.cat([inv_wsum[0]] + [inv_wsum[1]] * (T - 1) + [inv_wsum[2]])
    covered = (T + 1) * hop

    def torch_forward(m):
        X = noisy.unfold(1, frame, hop) @ Wf[:frame]
        g = torch.lerp(m[:, :, lo], m[:, :, lo + 1], tab_wt)
        y = ((X * g) @ Wi[:, :frame]).transpose(1, 2)
        ola = torch.nn.functional.fold(y, (1, covered), (1, frame), stride=(1, hop)).reshape(B, covered)
        return ola * scale

    m_graph = mask.clone().requires_grad_()
    kept = torch_forward(m_graph)
    d_cov = dout[:, :covered].contiguous()

    def backward():
        ops.mask_resynth_bwd(noisy, dout, T_mask=T, out=dmask, **kw)

    def forward():
        ops.mask_resynth(noisy, mask, out=out, **kw)

    def torch_backward():
        return torch.autograd.grad(kept, m_graph, d_cov, retain_graph=True)[0]

    def torch_both():
        m = mask.detach().requires_grad_()
        return torch.autograd.grad(torch_forward(m), m, d_cov)[0]

    t = alternate({"backward": backward, "forward": forward, "torch_backward": torch_backward, "torch_both": torch_both}, launches)
    torch.cuda.synchronize()
    ops.profiler.enable({"resynth_bwd"})
    backward()
    stated = ops.profiler.summary()["resynth_bwd"]
    ops.profiler.disable()
    res = {"batch": B, "samples": L, "frames": T, "launches": launches}
    res.update({name: row(ms) for name, ms in t.items()})
    med = statistics.median(t["backward"]) * 1e-3
    floor = max(stated["bytes"] / PEAK_HBM, stated["flops"] / PEAK_F32_MATRIX)
    res["backward"].update({"stated_mbyte": round(stated["bytes"] / 1e6, 2), "stated_gflop": round(stated["flops"] / 1e9, 2),
                            "tbyte_per_s": round(stated["bytes"] / med / 1e12, 3), "tflop_per_s": round(stated["flops"] / med / 1e12, 1),
                            "bound": "fp32 matrix" if stated["flops"] / PEAK_F32_MATRIX > stated["bytes"] / PEAK_HBM else "HBM",
                            "share_of_bound": round(floor / med, 3)})
    res["backward_over_forward"] = round(statistics.median(t["backward"]) / statistics.median(t["forward"]), 3)
    res["torch_backward_over_backward"] = round(statistics.median(t["torch_backward"]) / statistics.median(t["backward"]), 3)
    res["torch_both_over_backward"] = round(statistics.median(t["torch_both"]) / statistics.median(t["backward"]), 3)
    ref = torch_backward()
    res["max_difference_over_max"] = float((dmask - ref).abs().max() / ref.abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if a.launches < 200:
        raise SystemExit("bench_resynth_bwd: the median is taken over at least 200 launches")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resynth_bwd: needs the GPU (a CPU timing says nothing about it)")
    for B in a.batches:
        print(json.dumps(one_batch(B, a.seconds, a.launches)), flush=True)


if __name__ == "__main__":
    main()
