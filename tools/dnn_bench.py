#!/usr/bin/env python3
"""SpeechEnhancementDNN's layer kernel (csrc/dnn.hip) at a training batch of 100 x DNN_BATCH_SIZE = 25 600 rows, fp16.

  hidden     one hidden layer (K = N = 1024, ReLU, 16-bit rows out) through ops.dnn_layer, against ops.linear16 (sfm_gemm16, no
             activation: the kernel a hidden layer would otherwise run on) on the same operands in the same process
  first      the first layer in context mode (raw [64, 400, 54] -> [25 600, 1024]) against ops.feature_context + the same layer on
             the fp32 rows it wrote (rows32)

Device events around windows of `launches` back-to-back launches, the arms alternating window by window after a warm-up of every
arm; per arm the median over `windows` and its spread (max - min) in microseconds per launch, the share of the 2.5 PFLOP/s dense
fp16 matrix peak (the flops the algorithm needs: 2 M N K), and for `first` the bytes each arm's wrappers state.

    python tools/dnn_bench.py [--rows 25600] [--windows 9] [--launches 40]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import ops  # noqa: E402

PEAK_F16 = 2.5e15


def windows(arms, n_windows, launches):
    """arms: {name: fn}.  -> {name: [ms per launch of each window]}, the arms alternating"""
    for fn in arms.values():
        for _ in range(5):
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


def row(ms, flops):
    med = statistics.median(ms)
    return {"median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
            "spread_us": round((max(ms) - min(ms)) * 1e3, 2), "tflops": round(flops / med / 1e9, 1),
            "share_of_f16_peak": round(flops / (med * 1e-3) / PEAK_F16, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=25600)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dnn_bench: needs the GPU (a CPU timing says nothing about it)")
    ops.set_compute_dtype(torch.float16)
    gen = torch.Generator(device="cuda").manual_seed(29)
    M, H = a.rows, 1024
    res = {"rows": M, "windows": a.windows, "launches_per_window": a.launches, "dtype": "f16"}

    w = torch.randn(H, H, device="cuda", generator=gen) * (2.0 / H) ** 0.5
    b = torch.randn(H, device="cuda", generator=gen) * 0.05
    pw = ops.pack_linear(w, b)
    x16 = torch.randn(M, H, device="cuda", generator=gen).clamp_(min=0).half()
    o_new, o_old = torch.empty(M, H, device="cuda", dtype=torch.float16), torch.empty(M, H, device="cuda", dtype=torch.float16)
    arms = {"dnn_layer": lambda: ops.dnn_layer(x16, pw, act="relu", out=o_new),
            "linear16": lambda: ops.linear16(x16, pw, out=o_old)}
    t = windows(arms, a.windows, a.launches)
    torch.cuda.synchronize()
    diff = float((o_new.float() - o_old.float().clamp(min=0)).abs().max())
    flops = 2.0 * M * H * H
    res["hidden"] = {name: row(ms, flops) for name, ms in t.items()}
    res["hidden"]["max_abs_difference_to_relu_of_linear16"] = diff

    B, T, D, ctx = M // 400, 400, 54, 5
    K = D * (2 * ctx + 1)
    raw = (torch.randn(B, T, D, device="cuda", generator=gen) * 1.5).clamp_(-10, 10)
    mean = torch.randn(K, device="cuda", generator=gen) * 0.3
    std = 0.5 + 1.5 * torch.rand(K, device="cuda", generator=gen)
    w0 = torch.randn(H, K, device="cuda", generator=gen) * (2.0 / K) ** 0.5
    pw0 = ops.pack_linear(w0, b, k_pad_to=ops.round_up(K, 8))
    o_ctx, o_mat = torch.empty(B * T, H, device="cuda", dtype=torch.float16), torch.empty(B * T, H, device="cuda", dtype=torch.float16)

    def materialised():
        rows = ops.feature_context(raw, ctx, L=T, frame=1, hop=1, mean=mean, std=std, clip=10.0)
        ops.dnn_layer(rows.reshape(B * T, K), pw0, act="relu", out=o_mat)

    arms = {"context": lambda: ops.dnn_layer(raw, pw0, act="relu", out=o_ctx, context=ctx, mean=mean, std=std),
            "add_context_rows32": materialised}
    t = windows(arms, a.windows, a.launches)
    torch.cuda.synchronize()
    flops0 = 2.0 * B * T * H * K
    res["first"] = {name: row(ms, flops0) for name, ms in t.items()}
    res["first"]["rows"] = B * T
    res["first"]["max_abs_difference"] = float((o_ctx.float() - o_mat.float()).abs().max())
    ops.profiler.enable({"dnn_layer", "feature_context"})
    arms["context"]()
    n_ctx = {k: v["bytes"] for k, v in ops.profiler.summary().items()}
    ops.profiler.enable({"dnn_layer", "feature_context"})
    materialised()
    n_mat = {k: v["bytes"] for k, v in ops.profiler.summary().items()}
    ops.profiler.disable()
    res["first"]["stated_mbyte"] = {"context": round(sum(n_ctx.values()) / 1e6, 2), "add_context_rows32": round(sum(n_mat.values()) / 1e6, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
