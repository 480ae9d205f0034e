"""Forward + backward of training.TaalSTOILoss (STOI of Taal et al. / ESTOI as an objective) over B utterances of 4 s at 16 kHz,
for a kernel trace in a run of its own - the protocol of tools/stoi_taal_bench.py:

    rocprofv3 --kernel-trace -d DIR -o loss --output-format csv -- python tools/stoi_loss_bench.py --batch 64 --measure estoi
    python tools/stoi_loss_bench.py --summary DIR
    python tools/stoi_loss_bench.py --events [--batch 64]

The first form runs --passes steps (loss, backward) on one batch; the second reads DIR/**/*kernel_trace.csv and prints, per
kernel, the launches per pass and the median duration of a launch, the first 5 passes dropped as warm-up.  --events times, with
device events in one process, a step of each measure and - as context - the same objective composed from torch fp32 operations
(conv1d resampler, unfold, index ops, rfft, band matrix, unfold again).  That arm is no reference (its sums are fp32) and no
kernel-for-kernel comparison: the kept list makes the utterances ragged, so it loops over them and calls torch.nonzero for each,
a device synchronisation per utterance, and its time is mostly host overhead."""
import csv
import glob
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP = 5
FS, L = 16000, 64000


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def signals(B):
    import torch
    rng = np.random.default_rng(0)
    t = np.arange(L) / FS
    clean = (0.5 * (1 + 0.5 * np.sin(2 * np.pi * 7 * t)) * np.sin(2 * np.pi * 440 * t))[None, :] + 0.05 * rng.standard_normal((B, L))
    clean[:, 20000:30000] *= 1e-4                              # a pause: frames are dropped, as in speech
    enh = 0.8 * clean + 0.15 * rng.standard_normal((B, L))
    return torch.from_numpy(clean.astype(np.float32)).cuda(), torch.from_numpy(enh.astype(np.float32)).cuda()


def run(passes, B, measure):
    import torch
    from sincformer_metacog_speech_enhancement_amd.training import TaalSTOILoss
    c, e = signals(B)
    e.requires_grad_(True)
    loss_fn = TaalSTOILoss(FS, extended=measure == "estoi")
    for _ in range(passes):
        e.grad = None
        loss = loss_fn(e, c)
        loss.backward()
    torch.cuda.synchronize()
    print("B %d %s | passes %d | loss %.6f | |grad| %.6e" % (B, measure, passes, float(loss), float(e.grad.double().norm())))


def torch_objective(e, c, extended):
    """the objective from torch fp32 operations; the kept list from the clean side, as the measure has it"""
    import torch
    import torch.nn.functional as F
    from sincformer_metacog_speech_enhancement_amd.evaluation import stoi_taal as st
    dev = e.device
    up, down = st.rate_ratio(FS)
    h = torch.from_numpy(st.resample_taps(up, down).astype(np.float32)).to(dev)
    half = (h.numel() - 1) // 2
    w = torch.from_numpy(st.window().astype(np.float32)).to(dev)
    edges = st.band_edges()
    bm = torch.zeros(257, 15, device=dev)
    for j in range(15):
        bm[edges[j]:edges[j + 1], j] = 1.0

    def to10k(x):
        z = torch.zeros(x.shape[0], x.shape[1] * up, device=dev)
        z[:, ::up] = x
        full = F.conv1d(z[:, None], h.flip(0)[None, None], padding=h.numel() - 1)[:, 0]
        n = -(-x.shape[1] * up // down)
        return full[:, half:half + n * down:down]
    x, y = to10k(c), to10k(e)
    xf, yf = x.unfold(1, 256, 128) * w, y.unfold(1, 256, 128) * w
    en = 20.0 * torch.log10(xf.norm(dim=2) + 1e-12)
    total = 0.0
    for u in range(e.shape[0]):                               # ragged after the keep decision
        idx = torch.nonzero(en[u] > en[u].max() - 40.0)[:, 0]
        K = idx.numel()

        def bands(fr):
            s = torch.zeros((K + 1) * 128, device=dev)
            s = s.index_add(0, (idx.new_tensor(range(K))[:, None] * 128 + torch.arange(256, device=dev)[None]).reshape(-1),
                            fr[idx].reshape(-1))
            sp = torch.fft.rfft(s.unfold(0, 256, 128)[:K - 1] * w, 512)
            return torch.sqrt((sp.real ** 2 + sp.imag ** 2) @ bm).t()                    # [15, K - 1]
        xt, yt = bands(xf[u]), bands(yf[u])
        xg, yg = xt.unfold(1, 30, 1).permute(1, 0, 2), yt.unfold(1, 30, 1).permute(1, 0, 2)
        if extended:
            def rc(a):
                a = a - a.mean(2, keepdim=True)
                a = a / (a.norm(dim=2, keepdim=True) + 1e-12)
                a = a - a.mean(1, keepdim=True)
                return a / (a.norm(dim=1, keepdim=True) + 1e-12)
            total = total + (rc(xg) * rc(yg)).sum() / 30.0 / xg.shape[0]
        else:
            a = xg.norm(dim=2, keepdim=True) / (yg.norm(dim=2, keepdim=True) + 1e-12)
            yp = torch.minimum(yg * a, xg * (1.0 + 10.0 ** 0.75))
            yp, xz = yp - yp.mean(2, keepdim=True), xg - xg.mean(2, keepdim=True)
            total = total + (yp / (yp.norm(dim=2, keepdim=True) + 1e-12) * xz / (xz.norm(dim=2, keepdim=True) + 1e-12)).sum() \
                / (xg.shape[0] * 15)
    return -total / e.shape[0]


def events(B, steps):
    import torch
    from sincformer_metacog_speech_enhancement_amd.training import TaalSTOILoss
    c, e = signals(B)
    e.requires_grad_(True)

    def timed(step):
        ms = []
        for i in range(steps + WARMUP):
            e.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            val = step()
            t1.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), float(val)
    for measure in ("stoi", "estoi"):
        loss_fn = TaalSTOILoss(FS, extended=measure == "estoi")

        def hip_step():
            loss = loss_fn(e, c)
            loss.backward()
            return loss.detach()

        def torch_step():
            loss = torch_objective(e, c, measure == "estoi")
            loss.backward()
            return loss.detach()
        a, va = timed(hip_step)
        b, vb = timed(torch_step)
        print("B %d %s | forward + backward, median of %d | HIP %.3f ms (loss %.6f) | torch fp32 composition %.3f ms (loss %.6f)"
              % (B, measure, steps, a, va, b, vb))


def summary(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % root)
    per = {}
    for r in csv.DictReader(open(files[0])):
        per.setdefault("%s [grid %s x %s]" % (r["Kernel_Name"], r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?")), []).append(
            (int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    passes = max(len(v) for k, v in per.items() if "stoi_keep_kernel" in k)
    print("%d passes in the trace; per kernel: launches per pass, median us of a launch (first %d passes dropped)" % (passes, WARMUP))
    total = 0.0
    for name, rows in sorted(per.items(), key=lambda kv: -sum(d for _, d in kv[1])):
        if len(rows) % passes:
            continue                                           # set-up work outside the passes
        n = len(rows) // passes
        med = statistics.median([d for _, d in sorted(rows)[WARMUP * n:]]) / 1e3
        total += med * n
        print("%3d x %9.1f us  %s" % (n, med, name[:150]))
    print("sum over the kernels of a pass (launches x median): %.1f us" % total)


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(arg("--summary", ""))
    elif "--events" in sys.argv:
        events(arg("--batch", 64), arg("--steps", 20))
    else:
        run(arg("--passes", 40), arg("--batch", 64), arg("--measure", "stoi"))
