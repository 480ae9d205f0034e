#!/usr/bin/env python3
"""RBM pre-training (csrc/rbm.hip, models/rbm.py): one CD-1 step at batch 256 in counter mode, layer 1 (50 000 x 594 -> 1024) and
layer 2 (1024 -> 1024), and the whole three-layer pre-training of the default recipe (10 epochs, 1 960 steps per layer).

  hip      RBM._step: up + sample, down, up, update - four launches, the batch rows gathered through the index
  torch    the same step composed from torch fp32 operations on the same GPU (index_select, three addmm + sigmoid, a rand_like
           comparison, two matmuls for the associations, the means): the yardstick, which lives in this tool only

Device events around windows of `steps` back-to-back steps, the two arms alternating window by window after a warm-up of both; per
arm the median over `windows` (at least 20) and its spread in microseconds per step, the step's 1.56 Gflop (layer 1) over the median
as a share of the fp32 matrix rate (157.3 TFLOP/s); per launch the HIP-event time of ops.profiler.  The whole pre-training is
host wall-clock time around pretrain_dnn_with_rbm including its one readback per layer.

    python tools/rbm_bench.py [--windows 21] [--steps 50] [--pretrain-reps 20]
    python tools/rbm_bench.py --trace-steps 200        # only HIP steps of layer 1, then of layer 2: for a kernel trace of its own
    python tools/rbm_bench.py --reference <root>       # 20 CD-1 steps of the reference's numpy RBM on this host's CPU (no GPU)
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

PEAK_F32_MATRIX = 157.3e12
ROWS, BATCH = 50000, 256
LAYERS = {"layer1": (594, 1024), "layer2": (1024, 1024)}


def reference_cpu(root):
    sys.path.insert(0, root)
    sys.dont_write_bytecode = True
    from models.rbm import RBM
    np.random.seed(0)
    rbm = RBM(594, 1024)
    batch = np.random.random((BATCH, 594))
    rbm.contrastive_divergence(batch)
    t0 = time.perf_counter()
    for _ in range(20):
        rbm.contrastive_divergence(batch)
    dt = time.perf_counter() - t0
    print(json.dumps({"reference_cpu_20_steps_s": round(dt, 3), "extrapolated_layer1_s": round(dt / 20 * 1960, 1),
                      "threads": torch.get_num_threads()}))


def step_flops(V, H, B=BATCH):
    return 2.0 * B * V * H * 3 + 2.0 * (2 * B) * V * H


def windows(arms, n_windows, steps):
    for fn in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(n_windows):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / steps)
    return out


def row(ms):
    med = statistics.median(ms)
    return {"median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
            "spread_us": round((max(ms) - min(ms)) * 1e3, 2)}


def arms_for(V, H, gen):
    from sincformer_metacog_speech_enhancement_amd import models, ops
    data = torch.rand(ROWS, V, device="cuda", generator=gen)
    rows = torch.randperm(ROWS, device="cuda", generator=gen)[:BATCH].to(torch.int32)
    rows64 = rows.long()
    np.random.seed(1)
    rbm = models.RBM(V, H, seed=1)
    rbm.train(data[:BATCH], epochs=1, batch_size=BATCH, verbose=False)                 # moves the state to the device
    bufs = rbm._buffers(BATCH, data.device)
    partial = torch.zeros(ops.rbm_error_tiles(V), device="cuda", dtype=torch.float64)
    W, vb, hb = rbm.get_weights()
    lr = rbm.lr
    err = torch.zeros((), device="cuda")

    def hip():
        rbm._step(data, rows, BATCH, bufs, partial, None)

    def composed():
        v = data.index_select(0, rows64)
        ph = torch.sigmoid(torch.addmm(hb, v, W))
        hs = (ph > torch.rand_like(ph)).float()
        nv = torch.sigmoid(torch.addmm(vb, hs, W.t()))
        nh = torch.sigmoid(torch.addmm(hb, nv, W))
        W.add_(v.t() @ ph - nv.t() @ nh, alpha=lr / BATCH)
        d = v - nv
        vb.add_(d.mean(0), alpha=lr)
        hb.add_((ph - nh).mean(0), alpha=lr)
        err.copy_((d * d).mean())

    return hip, composed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--pretrain-reps", type=int, default=20)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    if a.reference:
        return reference_cpu(a.reference)
    if not torch.cuda.is_available():
        raise SystemExit("rbm_bench: needs the GPU (a CPU timing says nothing about it)")
    from sincformer_metacog_speech_enhancement_amd import models, ops
    gen = torch.Generator(device="cuda").manual_seed(24)
    if a.trace_steps:
        for V, H in LAYERS.values():
            hip, _ = arms_for(V, H, gen)
            for _ in range(a.trace_steps):
                hip()
            torch.cuda.synchronize()
        return
    res = {"rows": ROWS, "batch": BATCH, "windows": a.windows, "steps_per_window": a.steps}
    for name, (V, H) in LAYERS.items():
        hip, composed = arms_for(V, H, gen)
        t = windows({"hip": hip, "torch": composed}, a.windows, a.steps)
        r = {"hip": row(t["hip"]), "torch": row(t["torch"])}
        med = statistics.median(t["hip"]) * 1e-3
        r["hip"]["step_gflop"] = round(step_flops(V, H) / 1e9, 3)
        r["hip"]["share_of_fp32_matrix_rate"] = round(step_flops(V, H) / med / PEAK_F32_MATRIX, 4)
        r["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
        ops.profiler.enable({"rbm_prob", "rbm_update"}, tags=True)
        for _ in range(20):
            hip()
        launches = ops.profiler.summary()
        ops.profiler.disable()
        r["hip"]["launch_us_by_events"] = {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(launches.items()) if "[" in k}
        res[name] = r
    data = torch.rand(ROWS, 594, device="cuda", generator=gen)
    times = []
    for rep in range(a.pretrain_reps + 1):
        np.random.seed(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        models.pretrain_dnn_with_rbm(data, [594, 1024, 1024, 1024], verbose=False, seed=rep)
        torch.cuda.synchronize()
        if rep:                                                                      # the first one warms up
            times.append((time.perf_counter() - t0) * 1e3)
    res["pretrain_3_layers_ms"] = {"median": round(statistics.median(times), 1), "min": round(min(times), 1), "max": round(max(times), 1),
                                   "reps": len(times), "steps": 3 * 1960}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
