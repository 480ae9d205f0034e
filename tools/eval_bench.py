"""Evaluate-loop throughput, enhancement AND scoring: the 800-utterance list of tools/ragged_bench.py (1-6 s at 8 kHz) with a
clean partner per utterance, through the default SpeechEnhancer at the default precision, three ways, in one process,
alternating:

  (a)  what the build offered before the packed evaluation: ConformerPipeline.enhance_batch, then compute_ssnr +
       compute_stoi per utterance on the returned arrays, for the noisy and for the enhanced signal (4 metric calls, each
       with its own upload and its own read-back, per utterance)
  (b)  ConformerPipeline.evaluate_batch with the same two measures (like for like)
  (b') evaluate_batch with all three measures (SSNR, STOI, the PESQ fallback)

Every arm is warmed with one untimed walk; an arm's figure is walks over the list repeated until >= --seconds of work, timed
on the host around a device synchronise, every copy included (all arms end with the scores on the host).  Three repeats
give the spread.

    python tools/eval_bench.py [--n 800] [--max-frames 65536] [--seconds 2] [--trace-only]

--trace-only runs (b) alone a few times, for `rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --trace-only`.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sincformer_metacog_speech_enhancement_amd import ops, synthetic as syn                               # noqa: E402
from sincformer_metacog_speech_enhancement_amd.evaluation import compute_ssnr, compute_stoi               # noqa: E402
from ragged_bench import FS, HOP, make_pipe, timed                                                        # noqa: E402


def make_pairs(n, seed):
    """ragged_bench.make_signals with the clean partner of every noisy signal"""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1 * FS, 6 * FS + 1, n)
    noisy, clean = syn.synth_wave(8, int(lengths.max()), seed + 1)
    return ([np.ascontiguousarray(clean[i % 8, :L]) for i, L in enumerate(lengths)],
            [np.ascontiguousarray(noisy[i % 8, :L]) for i, L in enumerate(lengths)])


def walk_per_utterance(pipe, clean, noisy, max_frames):
    enh = pipe.enhance_batch(noisy, max_frames=max_frames)
    out = {"noisy": {"ssnr": [], "stoi": []}, "enhanced": {"ssnr": [], "stoi": []}}
    for c, x, y in zip(clean, noisy, enh):
        for side, s in (("noisy", x), ("enhanced", y)):
            out[side]["ssnr"].append(compute_ssnr(c, s, FS))
            out[side]["stoi"].append(compute_stoi(c, s, FS))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=800)
    ap.add_argument("--max-frames", type=int, default=65536)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs the GPU (no CPU timing)")
    ops.reset_precision()
    clean, noisy = make_pairs(a.n, a.seed)
    frames = sum(1 + s.size // HOP for s in noisy)
    pipe = make_pipe(a.seed + 2)
    two = ("ssnr", "stoi")
    if a.trace_only:
        for _ in range(3):
            pipe.evaluate_batch(clean, noisy, fs=FS, max_frames=a.max_frames, metrics=two)
        torch.cuda.synchronize()
        return
    print("# %d utterances, %d model frames, %.1f s of audio; frame budget %d" % (a.n, frames, sum(s.size for s in noisy) / FS,
                                                                                 a.max_frames))
    arms = {
        "a  enhance_batch + per-utterance ssnr, stoi": lambda: walk_per_utterance(pipe, clean, noisy, a.max_frames),
        "b  evaluate_batch (ssnr, stoi)": lambda: pipe.evaluate_batch(clean, noisy, fs=FS, max_frames=a.max_frames, metrics=two),
        "b' evaluate_batch (ssnr, stoi, pesq)": lambda: pipe.evaluate_batch(clean, noisy, fs=FS, max_frames=a.max_frames),
    }
    first = {name: fn() for name, fn in arms.items()}                      # warm-up walk of every arm; its scores are compared
    ra, rb = first["a  enhance_batch + per-utterance ssnr, stoi"], first["b  evaluate_batch (ssnr, stoi)"]
    for side in ("noisy", "enhanced"):
        for m in two:
            print("# arms a and b agree: %s %s max |difference| %.2e" % (side, m, float(np.abs(np.asarray(ra[side][m]) - rb[side][m]).max())))
    rates = {k: [] for k in arms}
    for rep in range(a.repeats):
        for name, fn in arms.items():
            walks, dt = timed(fn, a.seconds)
            rates[name].append(walks * a.n / dt)
    out = {}
    print("%-46s %40s" % ("arm", "utterances/s  (min / median / max)"))
    for name, r in rates.items():
        u = sorted(r)
        print("%-46s %12.1f / %12.1f / %12.1f" % (name, u[0], u[len(u) // 2], u[-1]))
        out[name] = u
    med = lambda k: out[k][len(out[k]) // 2]
    print("b / a: %.1fx (worst b over best a %.1fx); b' / b: %.2fx" % (
        med("b  evaluate_batch (ssnr, stoi)") / med("a  enhance_batch + per-utterance ssnr, stoi"),
        out["b  evaluate_batch (ssnr, stoi)"][0] / out["a  enhance_batch + per-utterance ssnr, stoi"][-1],
        med("b' evaluate_batch (ssnr, stoi, pesq)") / med("b  evaluate_batch (ssnr, stoi)")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
