"""Evaluate-loop throughput: a seeded list of 800 utterances of 1-6 s at 8 kHz (the reference's `evaluate` walks 50 utterances
x 4 noises x 4 SNRs) through the default SpeechEnhancer at the default precision, four ways, in one process, alternating:

  (a)  ConformerPipeline.enhance_signal per signal - plain launches
  (a') the same with use_graph = True (one hipGraph per signal length; a seeded 100-signal subset, since every new length is
       a capture): the first walk over the list, captures included, and a walk that only replays, separately
  (b)  zero-padded rectangular batches under the same frame budget (B x Tmax <= --max-frames).  WRONG ANSWERS for every
       utterance shorter than its batch's longest (tests/test_ragged_host.py): a time reference only
  (c)  ConformerPipeline.enhance_batch(max_frames = --max-frames): packed passes

Every shape is warmed first; an arm's figure is walks over the list repeated until >= --seconds of work, timed on the host
around a device synchronise, host-to-device and device-to-host copies included (all four return numpy arrays).  Three
repeats give the spread.  Also: TFLOP/s of the variable-length attention kernel over its useful FLOPs (4 x hd x H x sum T_i^2)
from device events around its launches in one pass of (c), next to the dense dispatcher's kernel at B 256 x T 512.

    python tools/ragged_bench.py [--n 800] [--max-frames 65536] [--seconds 2] [--trace-only]

--trace-only runs (c) alone a few times, for `rocprofv3 --kernel-trace --stats -- python tools/ragged_bench.py --trace-only`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sincformer_metacog_speech_enhancement_amd import functional as Fn, ops, synthetic as syn      # noqa: E402
from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp             # noqa: E402

FS, HOP = 8000, 80


def make_signals(n, seed):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1 * FS, 6 * FS + 1, n)
    noisy, _ = syn.synth_wave(8, int(lengths.max()), seed + 1)
    return [np.ascontiguousarray(noisy[i % 8, :L]) for i, L in enumerate(lengths)]


def make_pipe(seed):
    pipe = cp.ConformerPipeline()
    model = cp.SpeechEnhancer(n_freq=129)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed).items()}, strict=True)
    pipe.model = model.cuda().eval()
    return pipe


def padded_batches(sigs, budget):
    """greedy, in the given order: B x Tmax <= budget"""
    out, cur, tmax = [], [], 0
    for s in sigs:
        t = 1 + s.size // HOP
        if cur and (len(cur) + 1) * max(tmax, t) > budget:
            out.append(cur)
            cur, tmax = [], 0
        cur.append(s)
        tmax = max(tmax, t)
    if cur:
        out.append(cur)
    return out


@torch.no_grad()
def walk_padded(pipe, batches):
    res = []
    for b in batches:
        Lmax = max(s.size for s in b)
        x = np.zeros((len(b), Lmax), dtype=np.float32)
        for i, s in enumerate(b):
            x[i, :s.size] = s
        y = pipe._enhance_device(torch.from_numpy(x).to(pipe.device)).cpu().numpy()
        res.extend(y[i, :s.size] for i, s in enumerate(b))
    return res


def timed(fn, seconds):
    """(walks, wall seconds) of fn() repeated until >= seconds"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n, dt


def attention_rates(pipe, sigs, budget):
    """TFLOP/s from device events around the launches (ops.profiler)"""
    ops.profiler.enable({"attention_fwd_varlen", "attention_fwd"})
    try:
        pipe.enhance_batch(sigs, max_frames=budget)
        v = ops.profiler.launches("attention_fwd_varlen")
        ops.profiler.records = []
        B, T, H, hd = 256, 512, 4, 64
        with ops.stage("attn"):
            qkv = torch.randn(B * T, 3 * H * hd, device="cuda").to(ops.compute_dtype())
            for _ in range(6):
                ops.attention(qkv, B, T, H, hd)
        d = ops.profiler.launches("attention_fwd")[1:]
    finally:
        ops.profiler.disable()
        ops.profiler.records = []
    rate = lambda recs: sum(r[1] for r in recs) / (sum(r[0] for r in recs) * 1e-3) / 1e12
    return {"varlen_useful_tflops": rate(v), "varlen_launches": len(v), "varlen_ms_total": sum(r[0] for r in v),
            "dense_B256_T512_tflops": rate(d), "dense_kernel": ops.attention_kernel_name(B, T, H)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=800)
    ap.add_argument("--graph-n", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=65536)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench: needs the GPU (no CPU timing)")
    ops.reset_precision()
    sigs = make_signals(a.n, a.seed)
    frames = sum(1 + s.size // HOP for s in sigs)
    pipe = make_pipe(a.seed + 2)
    if a.trace_only:
        for _ in range(3):
            pipe.enhance_batch(sigs, max_frames=a.max_frames)
        torch.cuda.synchronize()
        return
    sub = [sigs[i] for i in np.random.RandomState(a.seed + 3).permutation(a.n)[:a.graph_n]]
    sub_frames = sum(1 + s.size // HOP for s in sub)
    batches = padded_batches(sigs, a.max_frames)
    padded_frames = sum(len(b) * max(1 + s.size // HOP for s in b) for b in batches)
    passes = Fn.packed_segments([s.size for s in sigs], max_frames=a.max_frames)
    print("# %d utterances, %d useful frames (T %d..%d); frame budget %d: %d packed passes, %d padded batches of %d frames "
          "(useful share %.2f); graphed subset %d utterances, %d frames" % (
              a.n, frames, min(1 + s.size // HOP for s in sigs), max(1 + s.size // HOP for s in sigs), a.max_frames, len(passes),
              len(batches), padded_frames, frames / padded_frames, len(sub), sub_frames))

    gpipe = make_pipe(a.seed + 2)
    gpipe.use_graph = True
    arms = {
        "a  enhance_signal, plain": (lambda: [pipe.enhance_signal(s) for s in sigs], a.n, frames),
        "a' enhance_signal, hipGraph replay": (lambda: [gpipe.enhance_signal(s) for s in sub], len(sub), sub_frames),
        "b  zero-padded batches (wrong answers)": (lambda: walk_padded(pipe, batches), a.n, frames),
        "c  enhance_batch (packed)": (lambda: pipe.enhance_batch(sigs, max_frames=a.max_frames), a.n, frames),
    }
    # warm every shape: one untimed walk per arm; for the graphed arm that walk is the one with the captures, timed on its own
    first = {}
    for name, (fn, n, fr) in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        first[name] = time.perf_counter() - t0
    n_sub = len(sub)
    print("a' first walk, %d captures included: %.2f s = %.1f utterances/s, %.0f useful frames/s" % (
        n_sub, first["a' enhance_signal, hipGraph replay"], n_sub / first["a' enhance_signal, hipGraph replay"],
        sub_frames / first["a' enhance_signal, hipGraph replay"]))
    rates = {k: [] for k in arms}
    for rep in range(a.repeats):
        for name, (fn, n, fr) in arms.items():
            walks, dt = timed(fn, a.seconds)
            rates[name].append((walks * n / dt, walks * fr / dt))
    out = {}
    print("%-42s %34s %40s" % ("arm", "utterances/s  (min / median / max)", "useful frames/s  (min / median / max)"))
    for name, r in rates.items():
        u, f = sorted(x[0] for x in r), sorted(x[1] for x in r)
        med = len(u) // 2
        print("%-42s %10.1f / %10.1f / %10.1f   %12.0f / %12.0f / %12.0f" % (name, u[0], u[med], u[-1], f[0], f[med], f[-1]))
        out[name] = {"utt_per_s": u, "frames_per_s": f}
    c, pl, gr = out["c  enhance_batch (packed)"], out["a  enhance_signal, plain"], out["a' enhance_signal, hipGraph replay"]
    print("packed / plain: %.1fx (worst packed repeat over best plain repeat %.1fx); packed / graph replay: %.1fx (worst over "
          "best %.1fx); packed / padded per useful frame: %.2fx" % (
              c["utt_per_s"][1] / pl["utt_per_s"][1], c["utt_per_s"][0] / pl["utt_per_s"][-1], c["utt_per_s"][1] / gr["utt_per_s"][1],
              c["utt_per_s"][0] / gr["utt_per_s"][-1],
              c["frames_per_s"][1] / out["b  zero-padded batches (wrong answers)"]["frames_per_s"][1]))
    att = attention_rates(pipe, sigs, a.max_frames)
    print("attention, device events: variable-length kernel %.1f TFLOP/s over the useful FLOPs (%d launches, %.2f ms in all); "
          "dense %s at B 256 x T 512: %.1f TFLOP/s" % (att["varlen_useful_tflops"], att["varlen_launches"], att["varlen_ms_total"],
                                                      att["dense_kernel"], att["dense_B256_T512_tflops"]))
    out["attention"] = att
    print(json.dumps(out))


if __name__ == "__main__":
    main()
