#!/usr/bin/env python3
"""One ConformerBlock (D 256, 4 heads, FF 1024, kernel 31, dropout 0.1), forward plus backward in train() mode, on packed rows
against the dense node, two questions in one process each:

  --mode ragged   64 utterances drawn uniformly from 1-4 s (T 201 .. 801): ConformerBlock.forward_packed on the sum_T real rows
                  against forward() on the same utterances zero-padded to [64, 801, D] (a time reference: its BatchNorm
                  statistics and attention rows see the padding).  Also prints sum_T / (B Tmax), the ratio padding alone explains.
  --mode equal    B 64 x T 512: forward_packed on [512] * 64 against forward() on [64, 512, D] - the item-table path against
                  the dense launches on the same work.
  --mode dense    the dense step at B 64 x T 512 alone: with --package-root it times another checkout's package (the parent
                  commit's).  Two packages of one name cannot live in one process, so this arm runs in a process of its own and
                  cannot alternate with the others window by window: alternate the PROCESSES, and read its figure against the
                  spread between processes of the same code, not against the spread between windows.

The arms of a process alternate window by window after a warm-up of --warmup steps of each, twice over; a window is --iters steps
(0.4 s at 2 ms a step) between two device synchronisations (host clock).  Per arm the median window, the fastest and the slowest,
as milliseconds per step; one JSON line, labelled with --label.

    python tools/packed_train_bench.py --mode ragged [--windows 7 --iters 200 --warmup 60]
    python tools/packed_train_bench.py --mode dense --package-root /path/to/other/checkout --label parent
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["ragged", "equal", "dense"], default="ragged")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=60)
ap.add_argument("--label", default="tree", help="what the JSON line calls the package it timed")
ap.add_argument("--seed", type=int, default=34)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.package_root))
import numpy as np  # noqa: E402
import torch  # noqa: E402

D, H, FF, KS, P = 256, 4, 1024, 31, 0.1


def window(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    if not torch.cuda.is_available():
        raise SystemExit("packed_train_bench: needs the GPU (a CPU timing says nothing about it)")
    from sincformer_metacog_speech_enhancement_amd import ops
    from sincformer_metacog_speech_enhancement_amd.models.conformer import ConformerBlock
    ops.set_compute_dtype(torch.float16)
    torch.manual_seed(ARGS.seed)
    block = ConformerBlock(D, H, FF, KS, P).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(ARGS.seed)
    if ARGS.mode == "ragged":
        lengths = np.random.default_rng(ARGS.seed).integers(201, 802, size=64).tolist()
    else:
        lengths = [512] * 64
    B, Tmax, sum_T = len(lengths), max(lengths), sum(lengths)
    xp = torch.randn(sum_T, D, device="cuda", generator=gen)
    gp = torch.randn(sum_T, D, device="cuda", generator=gen)
    xd = torch.zeros(B, Tmax, D, device="cuda")
    gd = torch.zeros(B, Tmax, D, device="cuda")
    o = 0
    for b, T in enumerate(lengths):
        xd[b, :T], gd[b, :T] = xp[o:o + T], gp[o:o + T]
        o += T

    def run(x, g, fwd):
        x = x.detach().requires_grad_(True)
        for p_ in block.parameters():
            p_.grad = None
        fwd(x).backward(g)

    arms = {"dense": lambda: run(xd, gd, block)}
    if ARGS.mode != "dense":
        from sincformer_metacog_speech_enhancement_amd import functional as Fn
        seg = Fn.packed_frames(lengths)
        arms["packed"] = lambda: run(xp, gp, lambda x: block.forward_packed(x, seg))
    for _ in range(2):                                              # warm-up: code objects, grants, the tables' upload, the
        for step in arms.values():                                  # allocator's pool at both arms' sizes, the clocks
            window(step, ARGS.warmup)
    times = {k: [] for k in arms}
    for _ in range(ARGS.windows):
        for k, step in arms.items():
            times[k].append(window(step, ARGS.iters))
    out = {"mode": ARGS.mode, "package": ARGS.label, "B": B, "Tmax": Tmax, "sum_T": sum_T,
           "rows_ratio": sum_T / float(B * Tmax), "sum_T2_ratio": sum(t * t for t in lengths) / float(B * Tmax * Tmax),
           "iters": ARGS.iters, "windows": ARGS.windows,
           "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(t, 4) for t in v]}
                           for k, v in times.items()}}
    if "packed" in times:
        out["packed_over_dense"] = out["ms_per_step"]["packed"]["median"] / out["ms_per_step"]["dense"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
