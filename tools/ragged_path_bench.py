"""Throughput of the EnhancementPath on a test set of different lengths: a seeded list of 800 utterances of 1-4 s at 16 kHz
through the default composition (PerceptionAgent -> CPEA -> STFT -> MaskSynthesisAgent -> iSTFT) at the default precision, three
ways, in one process, alternating:

  (a)  one dense `path(w[None])` call per utterance - plain launches (the only correct route without the ragged pass)
  (a') the same loop under graph.GraphedForward (one hipGraph per length; a seeded --graph-n subset, since every new length is a
       capture): the first walk, captures included, and walks that only replay, separately
  (c)  EnhancementPath.enhance_batch in passes of at most --max-samples PADDED samples (utterances of a pass x its longest), cut
       greedily in the list's order: one pinned upload, one ragged pass, one download per pass

Every shape is warmed first; an arm's figure is walks over the list repeated until >= --seconds of work, timed on the host
around a device synchronise, host-to-device and device-to-host copies included (all arms return numpy arrays).  --repeats
repeats give the spread.

    python tools/ragged_path_bench.py [--n 800] [--max-samples 4000000] [--seconds 2] [--trace-only]

--trace-only runs (c) alone a few times, for `rocprofv3 --kernel-trace --stats -- python tools/ragged_path_bench.py --trace-only`.
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

from sincformer_metacog_speech_enhancement_amd import graph, ops, synthetic as syn                   # noqa: E402
from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp             # noqa: E402

FS, HOP = 16000, 80


def make_signals(n, seed):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1 * FS, 4 * FS + 1, n)
    noisy, _ = syn.synth_wave(8, int(lengths.max()), seed + 1)
    return [np.ascontiguousarray(noisy[i % 8, :L]) for i, L in enumerate(lengths)]


def make_path(seed):
    """the default composition with bench.py's synthetic weights (the sinc layer keeps its own cut-offs and window)"""
    path = cp.EnhancementPath(sample_rate=FS)
    sd = path.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    keep = {k: v.numpy() for k, v in sd.items() if k.split(".")[-1] in ("low_hz_", "band_hz_", "window", "n_")}
    new = syn.synth_state_dict(shapes, seed, keep=keep, sinc_scale=2000.0)
    path.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=True)
    return path.cuda().eval()


def passes_of(sigs, budget):
    """greedy, in the given order: utterances x longest <= budget padded samples"""
    out, cur, lmax = [], [], 0
    for s in sigs:
        if cur and (len(cur) + 1) * max(lmax, s.size) > budget:
            out.append(cur)
            cur, lmax = [], 0
        cur.append(s)
        lmax = max(lmax, s.size)
    if cur:
        out.append(cur)
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=800)
    ap.add_argument("--graph-n", type=int, default=100)
    ap.add_argument("--max-samples", type=int, default=4000000)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2032)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_path_bench: needs the GPU (no CPU timing)")
    ops.reset_precision()
    sigs = make_signals(a.n, a.seed)
    path = make_path(a.seed + 2)
    passes = passes_of(sigs, a.max_samples)
    samples = sum(s.size for s in sigs)
    padded = sum(len(p) * max(s.size for s in p) for p in passes)

    @torch.no_grad()
    def ragged():
        out = []
        for p in passes:
            out.extend(path.enhance_batch(p))
        return out

    if a.trace_only:
        for _ in range(3):
            ragged()
        torch.cuda.synchronize()
        return

    @torch.no_grad()
    def dense_one(s):
        return path(torch.from_numpy(s[None]).cuda(), want=("wave",))["enhanced"].cpu().numpy()[0]

    graphed = graph.GraphedForward(lambda w: path(w, want=("wave",))["enhanced"])

    @torch.no_grad()
    def graph_one(s):
        return graphed(torch.from_numpy(s[None]).cuda()).cpu().numpy()[0]

    sub = [sigs[i] for i in np.random.RandomState(a.seed + 3).permutation(a.n)[:a.graph_n]]
    print("# %d utterances, %d samples (%.1f s of audio, L %d..%d); budget %d padded samples: %d ragged passes of %d padded "
          "samples (useful share %.2f); graphed subset %d utterances" % (
              a.n, samples, samples / FS, min(s.size for s in sigs), max(s.size for s in sigs), a.max_samples, len(passes), padded,
              samples / padded, len(sub)))
    arms = {
        "a  path(w[None]) per utterance, plain": (lambda: [dense_one(s) for s in sigs], a.n),
        "a' path(w[None]) per utterance, hipGraph replay": (lambda: [graph_one(s) for s in sub], len(sub)),
        "c  enhance_batch (ragged passes)": (ragged, a.n),
    }
    first = {}
    for name, (fn, n) in arms.items():                    # warm every shape; for the graphed arm this walk holds the captures
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        first[name] = time.perf_counter() - t0
        assert len(res) == n and all(np.isfinite(r).all() for r in res[:4])
    g = "a' path(w[None]) per utterance, hipGraph replay"
    print("a' first walk, %d captures included: %.2f s = %.1f utterances/s" % (len(sub), first[g], len(sub) / first[g]))
    rates = {k: [] for k in arms}
    for rep in range(a.repeats):
        for name, (fn, n) in arms.items():
            walks, dt = timed(fn, a.seconds)
            rates[name].append(walks * n / dt)
    out = {"n": a.n, "samples": samples, "padded_samples": padded, "passes": len(passes), "max_samples": a.max_samples,
           "first_walk_s": first}
    print("%-50s %s" % ("arm", "utterances/s  (min / median / max)"))
    for name, r in rates.items():
        u = sorted(r)
        print("%-50s %10.1f / %10.1f / %10.1f" % (name, u[0], u[len(u) // 2], u[-1]))
        out[name] = {"utt_per_s": u}
    c, pl, gr = (out[k]["utt_per_s"] for k in ("c  enhance_batch (ragged passes)", "a  path(w[None]) per utterance, plain", g))
    med = len(c) // 2
    print("ragged / plain loop: %.1fx at the medians (plain loop's min-max spread %.1f utterances/s, ragged median above the loop's "
          "by %.1f); ragged / graph replay: %.1fx" % (c[med] / pl[med], pl[-1] - pl[0], c[med] - pl[med], c[med] / gr[med]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
