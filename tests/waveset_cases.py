"""The cases and the float64 restatement behind tests/golden/g26_waveset.npz, shared by its generator and by
tests/test_waveset_host.py / tests/test_waveset_gpu.py.

WaveformDataset (training/conformer_pipeline.py:153-189 of the reference) restated: entry i of the file list - skipped entries
counted - is mixed over its WHOLE length with noise i % n_noise (tiled from sample 0, or cut) at snr_levels[i % len(snr_levels)],
P = mean + 1e-10 on both sides, and only then cut to max_len; __getitem__ zero-pads to max_len.  Evaluated in float64 it is the
tests' reference; evaluated in float32 it gives e32, the error that an fp32 evaluation of the same formula carries (the reference
takes its means in float32), and every bound here is 16 x e32.  The schedule and the two loaders' batch counts are restated too.
"""
import math

import numpy as np

FS, MAX_LEN, MIN_LEN = 8000, 2000, 640
# samples of each entry of the file list, in order; None: a file whose load raises
ENTRY_LENGTHS = (639, 640, 641, 1999, None, 2000, 2001, 5000, 300, 2000)
KEPT = (1, 2, 3, 5, 6, 7, 9)
NOISE_LENGTHS = (300, 2000, 7000)                           # tiled, equal to max_len, cut
LONG = 7                                                    # the non-stationary entry: scale over 5000 samples != over 2000
TOTALS = (1, 3, 4, 5, 9, 10, 12, 25, 50)                    # epoch counts whose schedule multipliers are recorded (3: the GPU run)
K = 16.0

MUTANTS = ("assignment by kept index instead of list position", "scale taken after the cut", "noise phase restarted at the cut")


def make_inputs():
    """(entries: list of float32 arrays or None, noises: list of float32 arrays), seeded"""
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    entries = []
    for i, n in enumerate(ENTRY_LENGTHS):
        if n is None:
            entries.append(None)
            continue
        x = syn.synth_array("waveset_clean%d" % i, (n,), 260 + i, 0.1)
        if i == LONG:
            x[MAX_LEN:] *= np.float32(0.05)                 # a twentieth of the amplitude behind the cut
        entries.append(x)
    noises = [syn.synth_array("waveset_noise%d" % k, (n,), 280 + k, 0.3) for k, n in enumerate(NOISE_LENGTHS)]
    return entries, noises


def tiled(noise, n, restart=None):
    """noise[j mod Ln] for j < n; restart: the phase starts again at every multiple of `restart` (a mutant)"""
    j = np.arange(n)
    if restart is not None:
        j = j % restart
    return noise[j % len(noise)]


def mix_scale(clean, noise, snr_db, dtype=np.float64, mutant=None, max_len=MAX_LEN):
    """_add_noise_at_snr's scale (:144-149) in `dtype`"""
    c, z = clean.astype(dtype), noise.astype(dtype)
    if mutant == MUTANTS[1]:
        c = c[:max_len]
    t = tiled(z, len(c), max_len if mutant == MUTANTS[2] else None)
    pc = np.mean(c ** 2, dtype=dtype) + dtype(1e-10)
    pn = np.mean(t ** 2, dtype=dtype) + dtype(1e-10)
    return np.sqrt(pc / (pn * dtype(10.0) ** dtype(snr_db / 10.0)))


def dataset(entries, noises, snr_levels, max_len=MAX_LEN, dtype=np.float64, mutant=None):
    """-> (kept positions, scales, noise ids, pairs [(noisy [max_len], clean [max_len])]) in `dtype`"""
    kept, scales, ids, pairs = [], [], [], []
    for i, c in enumerate(entries):
        if c is None or len(c) < MIN_LEN:
            continue
        a = len(kept) if mutant == MUTANTS[0] else i
        nid, snr = a % len(noises), snr_levels[a % len(snr_levels)]
        s = mix_scale(c, noises[nid], snr, dtype, mutant, max_len)
        n = min(len(c), max_len)
        noisy, clean = np.zeros(max_len, dtype), np.zeros(max_len, dtype)
        clean[:n] = c[:n].astype(dtype)
        noisy[:n] = clean[:n] + s * tiled(noises[nid].astype(dtype), n)
        kept.append(i)
        scales.append(s)
        ids.append(nid)
        pairs.append((noisy, clean))
    return kept, np.asarray(scales, dtype=dtype), ids, pairs


def e32_rows(entries, noises, snr_levels, max_len=MAX_LEN):
    """per kept utterance: max |float32 restatement - float64 restatement| of the noisy row; and the float64 data set"""
    d64 = dataset(entries, noises, snr_levels, max_len, np.float64)
    d32 = dataset(entries, noises, snr_levels, max_len, np.float32)
    return [float(np.abs(a[0].astype(np.float64) - b[0]).max()) for a, b in zip(d32[3], d64[3])], d64


def pairs_within(got, want, e32, lengths, k=K):
    """the assertion of the fixture and GPU rows: every noisy row within k x e32 of `want`'s (max |d|), every clean row and all
    padding (from lengths[u] on) exact.  got / want: lists of (noisy, clean); -> (ok, worst noisy |d| / (k e32))"""
    if not len(got) == len(want) == len(e32) == len(lengths):
        return False, float("inf")
    worst, ok = 0.0, True
    for (gn, gc), (wn, wc), e, n in zip(got, want, e32, lengths):
        gn, gc, wn, wc = (np.asarray(t, dtype=np.float64) for t in (gn, gc, wn, wc))
        if gn.shape != wn.shape or gc.shape != wc.shape:
            return False, float("inf")
        ok = ok and np.array_equal(gc, wc) and not gn[n:].any() and not gc[n:].any()
        worst = max(worst, float(np.abs(gn - wn).max()) / (k * e))
    return ok and worst <= 1.0, worst


def kept_lengths(entries, max_len=MAX_LEN):
    return [min(len(c), max_len) for c in entries if c is not None and len(c) >= MIN_LEN]


# ---- the schedule (:432-439) and the loaders (:445-451) ------------------------------------------------------------------------
def multipliers(total, mutant=None):
    warmup = max(1, min(5, total // 5))
    out = []
    for e in range(total):
        if e < warmup:
            out.append((e if mutant == "warm-up off by one" else e + 1) / warmup)
        else:
            out.append(max(0.01, 0.5 * (1 + math.cos(math.pi * (e - warmup) / max(1, total - warmup)))))
    return out


def batch_counts(n_train, n_test, batch, mutant=None):
    """(training batches: the last partial one dropped, validation batches: kept)"""
    val = n_test // batch if mutant == "drop_last applied to validation" else -(-n_test // batch)
    return n_train // batch, val
