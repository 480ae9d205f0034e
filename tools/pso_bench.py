#!/usr/bin/env python3
"""One PSO search of OPT-PCIRM's middle step at the reference's defaults (30 particles x 100 iterations) over a batch of
utterances: masks.compute_opt_pcirm with use_pso=True at B 64 x 4 s, fs 8000, C 64.  Synchronised wall time of the whole call
(host clock around work that ends in a device synchronise; median and spread of `rounds` calls after a warm-up), then - in a pass
of its own, device events around every launch (ops.profiler) - the per-family split.  Beside it the float64 restatement of
tests/pso_cases.py (the reference's own loop structure, numpy) on the CPU for ONE utterance of the same shape, same draws.

    python tools/pso_bench.py [--B 64] [--seconds 4] [--particles 30] [--iters 100] [--rounds 5] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pso_cases as pc  # noqa: E402
from sincformer_metacog_speech_enhancement_amd import masks, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--particles", type=int, default=30)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pso_bench: needs the GPU (a CPU timing says nothing about it)")
    fs, C = 8000, 64
    L = int(a.seconds * fs)
    T = -(-L // pc.MASK_HOP)
    B, N, K = a.B, a.particles, a.iters
    cases = []
    for b in range(B):                                       # the burst-noise construction of the tests, one seed per utterance
        pc.INPUTS["bench%d" % b] = (100 + b, C, L, T, fs)
        cases.append(pc.burst_case("bench%d" % b))
    pcirm = torch.from_numpy(np.stack([c["pcirm"] for c in cases])).cuda()
    noisy = torch.from_numpy(np.stack([c["noisy"] for c in cases])).cuda()
    clean = torch.from_numpy(np.stack([c["clean"] for c in cases])).cuda()
    draws = np.stack([pc.draws_after_seed(500 + b, N, K) for b in range(B)])
    cfg = {"num_particles": N, "max_iter": K, "draws": torch.from_numpy(draws).cuda(), "history": True}

    def run():
        return masks.compute_opt_pcirm(pcirm, noisy, clean, fs=fs, pso_config=cfg)

    for _ in range(2):
        out = run()
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    recs = out[3]
    ops.profiler.enable({"pso_prepare", "pso_fitness", "pso_step", "mask_quantize", "framed_gemm_f32_varlen"})
    run()
    split = {k: {"launches": v["n"], "ms_total": round(v["ms_total"], 4)} for k, v in ops.profiler.summary().items()}
    ops.profiler.disable()
    frames = (L - int(0.0256 * fs)) // (int(0.0256 * fs) // 2) + 1
    res = {"B": B, "L": L, "C": C, "T": T, "particles": N, "max_iter": K, "stoi_frames_per_utterance": frames,
           "search_ms_median": round(statistics.median(wall), 3), "search_ms_min": round(min(wall), 3),
           "search_ms_max": round(max(wall), 3), "utterances_per_s": round(B / statistics.median(wall) * 1e3, 1),
           "iterations_run": [r["iterations_run"] for r in recs][:8], "stopped_early": sum(r["stopped"] for r in recs),
           "middle_first8": [round(r["best_position"], 6) for r in recs][:8], "device_event_split": split}
    if not a.no_cpu:
        steps = pc.snr_boundaries(3)
        c = cases[0]
        t0 = time.perf_counter()
        rep = pc.pso(lambda x, it: np.array([pc.fitness(c["pcirm"], c["noisy"], c["clean"], float(v), fs, steps) for v in x]),
                     draws[0], N, K)
        res["cpu_restatement_one_utterance_s"] = round(time.perf_counter() - t0, 3)
        res["cpu_restatement_iterations_run"] = rep["iterations_run"]
        res["cpu_vs_device_middle_abs_diff"] = abs(rep["best_position"] - recs[0]["best_position"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
