#!/usr/bin/env python3
"""Mask to waveform (csrc/resynth.hip) at B 256 x 4 s, 8 kHz, the default framing (frame 160, hop 80, n_fft 256, 64 channels).

  fused      one ops.mask_resynth launch
  composed   the same result from the kernels the project had before it: ops.framed_gemm (sfm_framed_gemm_f32) with the windowed DFT
             operand -> [B, T, 258] spectrum, a torch elementwise gain from the same interpolation table, ops.framed_gemm with the
             windowed inverse operand -> [B, T + 1, 160] frames (row 0 of every utterance a zero frame: sfm_istft_ola trims half a
             window, as torch.istft does, and the zero frame puts that half back), ops.istft_ola, and the first hop's window sum
             corrected for the zero frame

Device events around windows of `launches` back-to-back runs, the arms alternating window by window after a warm-up of both; per arm
the median over `windows` and its spread (max - min) in microseconds per run; for the fused launch the bytes and flops its wrapper
states over the median time, and its share of the larger of the two hardware bounds (HBM 8 TB/s, fp32 matrix 157.3 TFLOP/s); the
largest difference between the two results.

    python tools/bench_resynth.py [--batch 256] [--seconds 4] [--windows 9] [--launches 20]
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


def windows(arms, n_windows, launches):
    """arms: {name: fn}.  -> {name: [ms per run of each window]}, the arms alternating"""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(n_windows):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / launches)
    return out


def row(ms):
    med = statistics.median(ms)
    return {"median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
            "spread_us": round((max(ms) - min(ms)) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resynth: needs the GPU (a CPU timing says nothing about it)")
    fs, frame, hop, n_fft, C = config.SAMPLE_RATE, config.FRAME_SIZE, config.HOP_SIZE, config.FFT_SIZE, config.NUM_CHANNELS
    F = n_fft // 2 + 1
    B, L = a.batch, int(a.seconds * fs)
    T = (L - frame) // hop + 1
    cf = np.asarray(erb_space(config.FREQ_LOW, config.FREQ_HIGH, C), dtype=np.float64)
    gen = torch.Generator(device="cuda").manual_seed(31)
    noisy = torch.randn(B, L, device="cuda", generator=gen) * 0.1
    mask = torch.rand(B, T, C, device="cuda", generator=gen)
    kw = dict(frame=frame, hop=hop, n_fft=n_fft, fs=fs, cf=cf)
    out_f = torch.empty(B, L, device="cuda")

    # the composition's operands: the full [frame, 2F] / [2F, frame] matrices in framed_gemm's padding, the table per bin
    Wf64, Wi64 = ops.resynth_matrices_host(frame, n_fft)
    full_f = np.zeros((frame, 2 * F))
    full_f[:, :F], full_f[:, F + 1:2 * F - 1] = Wf64[:, :F], Wf64[:, F:]
    full_i = np.zeros((2 * F, frame))
    full_i[:F], full_i[F + 1:2 * F - 1] = Wi64[:F], Wi64[F:]
    Wf = ops.pack_f32_matrix(torch.from_numpy(full_f.astype(np.float32)).cuda())
    Wi = ops.pack_f32_matrix(torch.from_numpy(full_i.astype(np.float32)).cuda())
    idx64, wt64 = ops.resynth_interp_table(fs, n_fft, cf)
    idx, wt = torch.from_numpy(idx64).cuda(), torch.from_numpy(wt64.astype(np.float32)).cuda()
    w2 = np.hanning(frame) ** 2
    win2 = torch.from_numpy(w2.astype(np.float32)).cuda()
    first, both = w2[:hop].copy(), w2[:hop] + w2[hop:]
    first[first < 1e-8] = 1.0
    corr = torch.from_numpy((both / first).astype(np.float32)).cuda()
    spec = torch.empty(B, T, 2 * F, device="cuda")
    frames = torch.zeros(B, T + 1, frame, device="cuda")
    out_c = torch.empty(B, L, device="cuda")

    def fused():
        ops.mask_resynth(noisy, mask, out=out_f, **kw)

    def composed():
        ops.framed_gemm(noisy, Wf, spec, B=B, M=T, Ls=L, sig_batch_stride=L, hop=hop, padl=0, K=frame, N=2 * F,
                        o_batch_stride=T * 2 * F, ldm=2 * F, ldn=1)
        g = torch.lerp(mask[:, :, idx], mask[:, :, idx + 1], wt)
        spec.view(B, T, 2, F).mul_(g.unsqueeze(2))
        ops.framed_gemm(spec, Wi, frames[:, 1:], B=B, M=T, Ls=T * 2 * F, sig_batch_stride=T * 2 * F, hop=2 * F, padl=0, K=2 * F,
                        N=frame, o_batch_stride=(T + 1) * frame, ldm=frame, ldn=1)
        ops.istft_ola(frames, win2, out_c, B, T + 1, L, frame, hop, frame, frame)
        out_c[:, :hop].mul_(corr)

    t = windows({"fused": fused, "composed": composed}, a.windows, a.launches)
    torch.cuda.synchronize()
    ops.profiler.enable({"resynth"})
    fused()
    stated = ops.profiler.summary()["resynth"]
    ops.profiler.disable()
    res = {"batch": B, "samples": L, "frames": T, "windows": a.windows, "launches_per_window": a.launches,
           "fused": row(t["fused"]), "composed": row(t["composed"])}
    med = statistics.median(t["fused"]) * 1e-3
    floor = max(stated["bytes"] / PEAK_HBM, stated["flops"] / PEAK_F32_MATRIX)
    res["fused"].update({"stated_mbyte": round(stated["bytes"] / 1e6, 2), "stated_gflop": round(stated["flops"] / 1e9, 2),
                         "tbyte_per_s": round(stated["bytes"] / med / 1e12, 3), "tflop_per_s": round(stated["flops"] / med / 1e12, 1),
                         "bound": "fp32 matrix" if stated["flops"] / PEAK_F32_MATRIX > stated["bytes"] / PEAK_HBM else "HBM",
                         "share_of_bound": round(floor / med, 3)})
    res["composed"]["moved_mbyte"] = round(4.0 * (2 * B * L + B * T * C + 4 * B * T * 2 * F + 2 * B * T * frame) / 1e6, 2)
    res["speedup"] = round(statistics.median(t["composed"]) / statistics.median(t["fused"]), 3)
    res["max_abs_difference"] = float((out_f - out_c).abs().max())
    res["max_abs_difference_interior"] = float((out_f[:, hop:T * hop] - out_c[:, hop:T * hop]).abs().max())
    res["max_abs_interior"] = float(out_f[:, hop:T * hop].abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
