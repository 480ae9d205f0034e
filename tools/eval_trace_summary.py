"""Share of the metric side in a kernel trace of tools/eval_bench.py --trace-only (arm b):

    rocprofv3 --kernel-trace --stats -d DIR -o evalb --output-format csv -- python tools/eval_bench.py --trace-only
    python tools/eval_trace_summary.py DIR [--save profiles/rNN]

Reads DIR/**/*kernel_stats.csv (time per kernel) and DIR/**/*kernel_trace.csv (one row per launch).  The packed framed GEMM
serves both the model's STFT and the metric DFTs under one kernel name; its launches are told apart by their grid: the STFT
writes 2 x 129 columns (5 column tiles of 64: grid x = 5 x 256 threads), the STOI DFT at 8 kHz 2 x 103 columns (4 tiles) - so
the split is made per launch on grid x.  That holds for arm (b), which --trace-only runs: the PESQ DFT at 8 kHz is as wide
as the STFT, so a trace of arm (b') could not be split this way.  --save copies the per-kernel table and the per-launch rows of that kernel as eval_kernels.csv and
eval_framed_gemm_launches.csv."""
import csv
import glob
import os
import sys

METRIC_KERNELS = ("ssnr_frames_varlen_kernel", "spec_frames_kernel", "wave_moments_varlen_kernel")
FRAMED = "framed_gemm_kernel<F16, true>"


def find(root, suffix):
    files = sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True))
    if not files:
        raise SystemExit("no *%s under %s" % (suffix, root))
    return files[0]


def main():
    root = sys.argv[1]
    save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
    stats = list(csv.DictReader(open(find(root, "kernel_stats.csv"))))
    trace = list(csv.DictReader(open(find(root, "kernel_trace.csv"))))
    tot = sum(float(r["TotalDurationNs"]) for r in stats)
    print("kernel trace of arm (b): %d kernels, %.2f ms of kernel time" % (len(stats), tot / 1e6))
    red = sum(float(r["TotalDurationNs"]) for r in stats if any(m in r["Name"] for m in METRIC_KERNELS))
    print("metric reduction kernels (%s): %.2f ms = %.1f %%" % (", ".join(METRIC_KERNELS), red / 1e6, 100 * red / tot))
    launches = sorted((r for r in trace if FRAMED in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            for r in launches]
    stft_grid = max(g for _, g, _, _ in rows)                     # the widest result: 258 columns
    stft = [r for r in rows if r[1] == stft_grid]
    dft = [r for r in rows if r[1] != stft_grid]
    t_stft, t_dft = sum(r[3] for r in stft), sum(r[3] for r in dft)
    print("packed framed GEMM: %d STFT launches (grid x %d) %.2f ms; %d metric DFT launches %.2f ms = %.1f %%" % (
        len(stft), stft_grid, t_stft / 1e6, len(dft), t_dft / 1e6, 100 * t_dft / tot))
    print("metric side in all (DFTs + reductions): %.2f ms = %.1f %% of the kernel time" % ((red + t_dft) / 1e6, 100 * (red + t_dft) / tot))
    for r in sorted(stats, key=lambda r: -float(r["TotalDurationNs"]))[:16]:
        print("%6.2f %%  %8.3f ms  %6s calls  %s" % (100 * float(r["TotalDurationNs"]) / tot, float(r["TotalDurationNs"]) / 1e6, r["Calls"],
                                                   r["Name"][:110]))
    if save:
        os.makedirs(save, exist_ok=True)
        with open(os.path.join(save, "eval_kernels.csv"), "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=list(stats[0].keys()))
            w.writeheader()
            w.writerows(stats)
        with open(os.path.join(save, "eval_framed_gemm_launches.csv"), "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["kernel", "grid_x", "grid_y", "duration_ns"])
            w.writerows(rows)


if __name__ == "__main__":
    main()
