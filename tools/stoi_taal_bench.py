"""One packed pass of STOI (Taal et al.) and ESTOI over 64 utterances of 4 s at 16 kHz, beside the simplified "stoi" of the same
compute_metrics_packed call, for a kernel trace in a run of its own:

    rocprofv3 --kernel-trace -d DIR -o stoi --output-format csv -- python tools/stoi_taal_bench.py [--passes 60]
    python tools/stoi_taal_bench.py --summary DIR

The first form packs the set once and runs the call --passes times (the clean side is computed in every pass: no clean_spectra
dict).  The second reads DIR/**/*kernel_trace.csv and prints, per kernel, the launches per pass and the median duration of a
launch; the first 5 passes' launches are dropped as warm-up."""
import csv
import glob
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
METRICS = ("stoi", "stoi_taal", "estoi")
WARMUP = 5


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def run(passes):
    import torch
    from sincformer_metacog_speech_enhancement_amd import config, functional as Fn
    from sincformer_metacog_speech_enhancement_amd.evaluation import compute_metrics_packed
    fs, B, L = 16000, 64, 64000
    rng = np.random.default_rng(0)
    t = np.arange(L) / fs
    clean = (0.5 * (1 + 0.5 * np.sin(2 * np.pi * 7 * t)) * np.sin(2 * np.pi * 440 * t))[None, :] + 0.05 * rng.standard_normal((B, L))
    clean[:, 20000:30000] *= 1e-4                              # a pause: frames are dropped, as in speech
    enh = 0.8 * clean + 0.15 * rng.standard_normal((B, L))
    lengths = np.full(B, L, dtype=np.int64)
    seg = Fn.PackedSegments(1 + lengths // config.HOP_SIZE, lengths)
    c = torch.from_numpy(clean.astype(np.float32).reshape(-1)).cuda()
    e = torch.from_numpy(enh.astype(np.float32).reshape(-1)).cuda()
    for _ in range(passes):
        out = compute_metrics_packed(c, e, seg, fs=fs, metrics=METRICS)
    torch.cuda.synchronize()
    print("passes %d | " % passes + " | ".join("%s mean %.6f" % (m, float(out[m].mean())) for m in METRICS))


def summary(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % root)
    per = {}
    for r in csv.DictReader(open(files[0])):
        # (the packed framed GEMM serves the resampler and the simplified measure's DFT: told apart by their grids)
        per.setdefault("%s [grid %s x %s]" % (r["Kernel_Name"], r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?")), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    passes = max(len(v) for k, v in per.items() if "stoi_keep_kernel" in k)
    print("%d passes in the trace; per kernel: launches per pass, median us of a launch (first %d passes dropped)" % (passes, WARMUP))
    total = 0.0
    for name, rows in sorted(per.items(), key=lambda kv: -sum(d for _, d in kv[1])):
        if len(rows) % passes:
            continue                                           # set-up work outside the passes
        n = len(rows) // passes
        d = [d for _, d in sorted(rows)[WARMUP * n:]]
        med = statistics.median(d) / 1e3
        total += med * n
        print("%3d x %9.1f us  %s" % (n, med, name[:160]))
    print("sum over the kernels of a pass (launches x median): %.1f us" % total)


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(arg("--summary", ""))
    else:
        run(arg("--passes", 60))
