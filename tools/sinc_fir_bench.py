#!/usr/bin/env python3
"""sinc_fir16 micro-benchmark (one pass, fp16 operands, 16-bit result) at the bench workload's shape and at B 64 x 4 s.

Times ops.sinc_fir16 (filter prep + FIR kernel + the zero fill of the partials) with HIP events over --launches launches, in
--rounds rounds that alternate the resident-tap kernel and the streaming one inside ONE process.  --default-only times only
what passes = 1 selects: the form to use with another build's library (SFM_LIB_PATH) that has no streaming selector."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sincformer_metacog_speech_enhancement_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--default-only", action="store_true")
args = ap.parse_args()

ops.set_compute_dtype("f16")
K, C = 251, 64
g = torch.Generator(device="cuda").manual_seed(0)
filt = torch.randn(C, K, device="cuda", generator=g)
filt = (filt / filt.abs().sum(dim=1, keepdim=True)).contiguous()
res = {"lib": os.environ.get("SFM_LIB_PATH", "tree"), "launches": args.launches}
for B, L in ((256, 40880), (64, 64000)):
    x = (torch.rand(B, L, device="cuda", generator=g) - 0.5) * 0.6
    out = torch.empty(B, L, C, device="cuda", dtype=torch.float16)

    def timed(resident):
        if not args.default_only:
            ops.set_sinc_fir_resident(resident)
        run = lambda: ops.sinc_fir16(x, filt, out, B, L, C, K, passes=1)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            run()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.launches * 1e3, 1)

    row = {"default_us": []} if args.default_only else {"resident_us": [], "streaming_us": []}
    for _ in range(args.rounds):
        if args.default_only:
            row["default_us"].append(timed(True))
        else:
            row["resident_us"].append(timed(True))
            row["streaming_us"].append(timed(False))
    row["out_GB"] = round(B * L * C * 2 / 1e9, 3)
    res["B%d_L%d" % (B, L)] = row
if not args.default_only:
    ops.set_sinc_fir_resident(True)
print(json.dumps(res))
