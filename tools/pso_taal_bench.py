"""The OPT-PCIRM search on the STOI / ESTOI of Taal et al. over 64 utterances of 4 s at 8 kHz with 30 particles, for a kernel trace
in a run of its own, beside what the measure alone offers for the same job: compute_stoi_taal on the materialised [B x N, L] batch
of ya + x yb.

    rocprofv3 --kernel-trace -d DIR -o pso_taal --output-format csv -- python tools/pso_taal_bench.py [--rounds 200] [--passes 8]
    python tools/pso_taal_bench.py --summary DIR

The first form runs one search per measure whose swarms stand still at uniform positions (zero velocities and draws: no swarm
converges and stops, so each of the --rounds rounds costs the same two launches), then --passes scorings of the materialised batch per
measure.  The second reads DIR/**/*kernel_trace.csv and prints, per kernel and grid, the launches, the median duration of a launch
and the total: the once-per-search preparation has the grids of 64 utterances, the materialised scoring those of 1920."""
import csv
import glob
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FS, B, C, SECONDS, N = 8000, 64, 64, 4.0, 30


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def run(rounds, passes):
    import torch
    import pso_cases as pc
    from sincformer_metacog_speech_enhancement_amd import config, masks, ops
    from sincformer_metacog_speech_enhancement_amd import functional as Fn
    from sincformer_metacog_speech_enhancement_amd.evaluation.stoi_taal import compute_stoi_taal, compute_stoi_taal_packed
    from sincformer_metacog_speech_enhancement_amd.masks.opt_pcirm import compute_snr_boundaries, quantizer_table
    if not torch.cuda.is_available():
        raise SystemExit("pso_taal_bench: needs the GPU (a CPU timing says nothing about it)")
    L = int(SECONDS * FS)
    T = -(-L // pc.MASK_HOP)
    cases = []
    for b in range(B):                                       # the burst-noise construction of the tests, one seed per utterance
        pc.INPUTS["bench%d" % b] = (100 + b, C, L, T, FS)
        cases.append(pc.burst_case("bench%d" % b))
    pcirm = torch.from_numpy(np.stack([c["pcirm"] for c in cases])).cuda()
    noisy = torch.from_numpy(np.stack([c["noisy"] for c in cases])).cuda()
    clean = torch.from_numpy(np.stack([c["clean"] for c in cases])).cuda()
    xs = np.random.RandomState(7).uniform(0, 1, (B, N))
    K = rounds - 1
    draws = torch.from_numpy(np.concatenate([xs, np.zeros((B, N)), np.zeros((B, 2 * N * K))], axis=1)).cuda()
    for m in ("stoi_taal", "estoi"):
        cfg = {"num_particles": N, "max_iter": K, "draws": draws, "history": True, "fitness": m}
        for _ in range(2):                                   # the second search is the one to read: every shape is warm
            recs = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=FS, pso_config=cfg)[3]
        torch.cuda.synchronize()
        ran = [r["iterations_run"] for r in recs]
        print("%s: %d rounds in every swarm: %s | mean fitness of round 0: %.6f" % (
            m, rounds, min(ran) == max(ran) == K, float(np.mean([r["fitness"][0].mean() for r in recs]))))
    # what the measure alone offers: every particle's signal materialised and scored
    steps, _ = compute_snr_boundaries()
    table, M = quantizer_table(steps, None, "cuda")
    lengths = np.full(B, L, dtype=np.int64)
    seg = Fn.PackedSegments(1 + lengths // config.HOP_SIZE, lengths)
    samp_off = seg.tables("cuda")["samp_off"]
    a, b = ops.pso_frame_coef(pcirm, table, M)
    ya, yb, cp, _ = ops.pso_split(noisy, clean, (samp_off[1:] - samp_off[:-1]).contiguous(), samp_off, a, b, seg.sum_L,
                                  config.FRAME_SIZE, config.HOP_SIZE)
    x32 = torch.from_numpy(xs.astype(np.float32)).cuda()
    enh = (ya.view(B, 1, L) + x32.view(B, N, 1) * yb.view(B, 1, L)).reshape(B * N, L).contiguous()
    ref = cp.view(B, 1, L).expand(B, N, L).reshape(B * N, L).contiguous()
    state = {}
    compute_stoi_taal_packed(cp, ya, seg, fs=FS, clean_state=state)
    kept = state[("stoi_taal", FS)]["kept"].cpu().numpy()
    print("kept frames per utterance: mean %.1f, min %d, max %d of %d; segments mean %.1f" % (
        kept.mean(), kept.min(), kept.max(), (L * 5 // 4 - 256) // 128 + 1, np.maximum(kept - 30, 0).mean()))
    for ext in (False, True):
        for _ in range(passes):
            out = compute_stoi_taal(ref, enh, FS, extended=ext)
        torch.cuda.synchronize()
        got = np.array([r["fitness"][0] for r in recs]) if ext else None
        print("materialised [%d, %d] batch, %s: %d passes, mean %.6f%s" % (
            B * N, L, "estoi" if ext else "stoi", passes, float(out.mean()),
            "" if got is None else " | largest distance from the search's fitness %.3g" % float(np.abs(out.cpu().numpy().reshape(B, N) - got).max())))


def summary(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % root)
    per = {}
    for r in csv.DictReader(open(files[0])):
        key = "%s [grid %s x %s]" % (r["Kernel_Name"], r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?"))
        per.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print("per kernel and grid: launches, median us of a launch, total ms")
    for name, d in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        if not any(k in name for k in ("stoi_", "pso_")):
            continue
        print("%-110s %6d x %10.1f us = %9.3f ms" % (name[:110], len(d), statistics.median(d) / 1e3, sum(d) / 1e6))


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
    else:
        run(arg("--rounds", 200), arg("--passes", 8))
