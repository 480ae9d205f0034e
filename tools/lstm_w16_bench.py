#!/usr/bin/env python3
"""bilstm_layer inference: fp32 recurrence against the fp16-operand form (sfm_bilstm_layer_ex), interleaved, at the shapes of the
bench workloads: B 64 x T 801 (configs[1]), B 256 x T 512 (c3p), B 32 x T 6001 (c5).

Per layer and shape: median and range over `--windows` windows of `--launches` back-to-back launches, device events around each
window.  To time another build, run the tool once more with SFM_LIB_PATH naming that build's library (lib.py); each line names
the library it measured.  `--w16-only` skips the fp32 recurrence (a counter-collection run wants one kernel)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sincformer_metacog_speech_enhancement_amd import lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64x801,256x512,32x6001,128x801", help="comma-separated BxT")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--w16-only", action="store_true")
args = ap.parse_args()

H = 128
g = torch.Generator(device="cuda").manual_seed(0)
for B, T in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
    xg = torch.randn(B, T, 2, 4 * H, device="cuda", generator=g)
    whh = torch.randn(2, 4 * H, H, device="cuda", generator=g) / H ** 0.5
    res = {}
    outs = {}
    forms = (True,) if args.w16_only else (False, True)
    for rnd in range(args.windows):
        for w16 in forms:
            run = lambda: ops.bilstm_layer(xg, whh, B, T, H, w16=w16)
            outs[w16] = run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                run()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(w16, []).append(e0.elapsed_time(e1) / args.launches)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    line = {"B": B, "T": T, "lib": lib.LIB_PATH, "windows": args.windows, "launches": args.launches,
            "fp16_ms": med[True], "fp16_ms_min": min(res[True]), "fp16_ms_max": max(res[True]),
            "us_per_step_fp16": 1e3 * med[True] / T}
    if not args.w16_only:
        d = (outs[True] - outs[False]).abs()
        line.update({"fp32_ms": med[False], "fp32_ms_min": min(res[False]), "fp32_ms_max": max(res[False]),
                     "us_per_step_fp32": 1e3 * med[False] / T,
                     "max_abs_diff": float(d.max()), "rms_diff": float(d.pow(2).mean().sqrt())})
    print(json.dumps(line))
