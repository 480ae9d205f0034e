"""Shared cases of the mask-to-waveform tests (tests/test_resynth_*.py, tests/golden/make_golden_resynth.py): a restatement in
numpy of steps 2-4 of enhance_signal (the Hann STFT of the noisy signal, np.interp of the mask's channels onto the STFT bins, the
masked irfft, overlap-add, division by the window sum), the same evaluation with float32 operands, the seeded inputs and the
mutants.  Test-side only; nothing here reads a kernel's output.

  restate64: float64 throughout, np.fft and np.interp themselves: the reference of the GPU rows (tests/test_resynth_host.py holds it
    to the reference's own output, tests/golden/g23_resynth.npz).
  restate32: the same result as two matrix products with float32 operands (the windowed DFT [frame, 2F] and the windowed, cropped
    inverse [2F, frame], built in float64 and cast), float32 signal, float32 table weights, float32 products and sums, float32
    1 / wsum: the row's e32 = its distance from restate64 relative to the row's largest float64 value, as tests/intelligibility_cases.py
    defines it.

Bounds.  A GPU row passes within K = 16 x e32.  Every case has two rows, each with its own e32 and its own maximum: the interior
samples (two frames cover them) and the single-coverage hops (the first `hop` and the last `hop` covered samples).  They are apart
because np.hanning(160)[1] ** 2 is 1.5e-7: the reference divides sample 1 by it, a gain of 2.6e3, and with one row that sample
would set the scale of the whole utterance.

The guard.  wsum < 1e-8 counts as 1.  check_wsum asserts for every framing used here that a window sum is exactly 0 (w[0], w[-1])
or at least 1e-7, a decade above the guard, so that float32 decides the guard as float64 does.  (1e-6 cannot be asked: that same
np.hanning(160)[1] ** 2 = 1.5e-7 is a window sum of every default case.)

Signals: noisy = the AM tone plus noise of intelligibility_cases.pair(L, seed, fs)[0]; mask = seeded uniform [0, 1] with about 5 %
exact zeros and 5 % exact ones."""
import numpy as np

import intelligibility_cases as ic
from sincformer_metacog_speech_enhancement_amd import config
from sincformer_metacog_speech_enhancement_amd.signal_processing.gammatone import erb_space

K = ic.K
fig = ic.fig

# name -> (frame, hop, n_fft, fs, channels)
FRAMINGS = {"default": (160, 80, 256, 8000, 64), "fs16k": (160, 80, 256, 16000, 64), "f128": (128, 64, 128, 8000, 20)}
GOLDEN_LENGTHS = (159, 160, 239, 240, 241, 1237)
GOLDEN_SHORT = (1237, -2)             # (L, rows of the mask relative to the STFT's frames): the stub returns two rows fewer
MUTANTS = ("periodic Hann", "irfft not cropped", "no synthesis window", "interior wsum on the first hop", "left / right = 0",
           "min(T_b, T_mask) ignored")

_cache = {}


def center_freqs(framing):
    C = FRAMINGS[framing][4]
    return np.asarray(erb_space(config.FREQ_LOW, config.FREQ_HIGH, C), dtype=np.float64)


def frames_of(L, frame, hop):
    return (L - frame) // hop + 1 if L >= frame else 0


def case(framing, L, seed, dT=0):
    """(noisy float32 [L], mask float32 [T_mask, C]) with T_mask = max(T + dT, 1).  Cached and shared: do not modify."""
    key = ("case", framing, L, seed, dT)
    if key not in _cache:
        frame, hop, _, fs, C = FRAMINGS[framing]
        T_mask = max(frames_of(L, frame, hop) + dT, 1)
        rng = np.random.RandomState(seed + 7919)
        m = rng.uniform(0.0, 1.0, size=(T_mask, C))
        u = rng.uniform(0.0, 1.0, size=(T_mask, C))
        m[u < 0.05] = 0.0
        m[u > 0.95] = 1.0
        _cache[key] = (ic.pair(L, seed, fs)[0], m.astype(np.float32))
    return _cache[key]


def cases(R):
    """(name, framing, L, seed, dT) of the GPU rows; R = the kernel's tile, in frames: the lengths put the last frame one hop before,
    at and one hop after a workgroup boundary, and one utterance spans three tiles"""
    frame, hop = FRAMINGS["default"][:2]
    edge = hop * (R - 1) + frame
    Ls = GOLDEN_LENGTHS + (edge - hop, edge, edge + hop, hop * (2 * (R - 1) + 5) + frame + 13)
    out = [("d%d" % L, "default", L, 800 + i, 0) for i, L in enumerate(Ls)]
    out += [("d1237_tm-2", "default", 1237, 820, -2), ("d1237_tm+1", "default", 1237, 821, 1),
            ("k1237", "fs16k", 1237, 822, 0), ("f128_1000", "f128", 1000, 823, 0)]
    return out


def check_wsum(framing):
    frame, hop = FRAMINGS[framing][:2]
    w2 = np.hanning(frame) ** 2
    ws = np.concatenate([w2[:hop], w2[:hop] + w2[hop:], w2[hop:]])
    small = ws < 1e-7
    assert np.all(ws[small] == 0.0) and small.sum() == 2 and w2[0] == 0.0 and w2[-1] == 0.0, (framing, ws[small])


def rows(L, N, frame, hop):
    """(interior, single, tail) index arrays of an utterance of L samples with N live frames"""
    s = np.arange(L)
    if N == 0:
        return s[:0], s[:0], s
    return s[hop:N * hop], np.concatenate([s[:hop], s[N * hop:(N + 1) * hop]]), s[(N + 1) * hop:]


# ---- float64: the definition itself ----
def restate64(noisy, mask, framing, mutant=None):
    """-> float64 [L], the value enhance_signal has before its cast to float32"""
    frame, hop, n_fft, fs, C = FRAMINGS[framing]
    cf = center_freqs(framing)
    x = np.asarray(noisy, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    L = x.shape[0]
    F = n_fft // 2 + 1
    w = np.hanning(frame)
    if mutant == "periodic Hann":
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(frame) / frame)
    T = frames_of(L, frame, hop)
    N = min(T, m.shape[0])
    freqs = np.arange(F) * (fs / 2.0) / (F - 1)
    enh = np.zeros(L + n_fft)
    wsum = np.zeros(L + n_fft)
    for n in range(T if mutant == "min(T_b, T_mask) ignored" else N):
        X = np.fft.rfft(x[n * hop:n * hop + frame] * w, n_fft)
        if n < N:
            if mutant == "left / right = 0":
                g = np.interp(freqs, cf, m[n], left=0.0, right=0.0)
            else:
                g = np.interp(freqs, cf, m[n], left=m[n, 0], right=m[n, C - 1])
        else:
            g = np.ones(F)
        y = np.fft.irfft(X * g, n_fft)
        sw = np.ones(frame) if mutant == "no synthesis window" else w
        enh[n * hop:n * hop + frame] += y[:frame] * sw
        if mutant == "irfft not cropped":
            enh[n * hop + frame:n * hop + n_fft] += y[frame:]
        wsum[n * hop:n * hop + frame] += w ** 2
    if mutant == "interior wsum on the first hop":
        wsum[:hop] = wsum[hop:2 * hop] if N > 1 else wsum[:hop]
    wsum[wsum < 1e-8] = 1.0
    return (enh / wsum)[:L]


# ---- float32 operands, float32 products ----
def operands64(frame, n_fft, w):
    """float64 (A [frame, 2F], S [2F, frame]): x @ A = [Re | Im] of rfft(x w, n_fft); [Re | Im] @ S = irfft(., n_fft)[:frame] w;
    phases (n k) mod n_fft"""
    F = n_fft // 2 + 1
    ph = 2.0 * np.pi * ((np.arange(frame)[:, None] * np.arange(F)[None, :]) % n_fft) / n_fft
    A = np.concatenate([w[:, None] * np.cos(ph), -w[:, None] * np.sin(ph)], axis=1)
    c = np.full(F, 2.0)
    c[0] = 1.0
    c[-1] = 1.0
    S = np.concatenate([c[:, None] * np.cos(ph.T), -c[:, None] * np.sin(ph.T)], axis=0) / n_fft * w[None, :]
    return A, S


def interp_table(framing):
    """(lower channel index [F], weight float64 [F]) of np.interp's rule, from cf and the bin frequencies"""
    _, _, n_fft, fs, C = FRAMINGS[framing]
    cf = center_freqs(framing)
    F = n_fft // 2 + 1
    freqs = np.arange(F) * (fs / 2.0) / (F - 1)
    lo = np.clip(np.searchsorted(cf, freqs, side="right") - 1, 0, C - 2)
    return lo, np.clip((freqs - cf[lo]) / (cf[lo + 1] - cf[lo]), 0.0, 1.0)


def restate32(noisy, mask, framing):
    """-> float32 [L]: restate64's result evaluated with float32 operands and float32 matrix products"""
    frame, hop, n_fft, fs, C = FRAMINGS[framing]
    f32 = np.float32
    x = np.asarray(noisy, dtype=f32)
    m = np.asarray(mask, dtype=f32)
    L = x.shape[0]
    N = min(frames_of(L, frame, hop), m.shape[0])
    out = np.zeros(L, dtype=f32)
    if N == 0:
        return out
    w = np.hanning(frame)
    A, S = (a.astype(f32) for a in operands64(frame, n_fft, w))
    lo, wt = interp_table(framing)
    wt = wt.astype(f32)
    fr = np.stack([x[n * hop:n * hop + frame] for n in range(N)])
    X = fr @ A
    g = (f32(1.0) - wt) * m[:N][:, lo] + wt * m[:N][:, lo + 1]
    y = (X * np.concatenate([g, g], axis=1)) @ S
    assert X.dtype == f32 and g.dtype == f32 and y.dtype == f32
    enh = np.zeros((N + 1) * hop, dtype=f32)
    for n in range(N):
        enh[n * hop:n * hop + frame] += y[n]
    w2 = w ** 2
    ws = np.concatenate([w2[:hop]] + [w2[:hop] + w2[hop:]] * (N - 1) + [w2[hop:]])
    ws[ws < 1e-8] = 1.0
    out[:(N + 1) * hop] = enh * (1.0 / ws).astype(f32)
    return out


def refs(framing, L, seed, dT=0):
    """(noisy, mask, out64, out32) of a case.  Cached and shared: do not modify."""
    key = ("refs", framing, L, seed, dT)
    if key not in _cache:
        check_wsum(framing)
        noisy, mask = case(framing, L, seed, dT)
        _cache[key] = (noisy, mask, restate64(noisy, mask, framing), restate32(noisy, mask, framing))
    return _cache[key]


def row_figures(got, out64, out32, framing, n_mask_rows):
    """[(row name, observed, e32)] of the interior and the single-coverage row (a row without samples is left out), after asserting
    that the uncovered tail of `got` is exactly 0"""
    frame, hop = FRAMINGS[framing][:2]
    L = out64.shape[0]
    N = min(frames_of(L, frame, hop), n_mask_rows)
    interior, single, tail = rows(L, N, frame, hop)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == out64.shape and np.all(got[tail] == 0.0) and np.all(out64[tail] == 0.0)
    return [(name, fig(got[sel], out64[sel]), fig(out32[sel], out64[sel])) for name, sel in (("interior", interior), ("single", single))
            if sel.size]


def check(name, got, out64, out32, framing, n_mask_rows):
    """print and assert both rows of a case: observed <= K x e32"""
    for row, o, e32 in row_figures(got, out64, out32, framing, n_mask_rows):
        print("ROW | %s %s | e32 %.2e | bound %.2e | observed %.2e" % (name, row, e32, K * e32, o))
        assert np.isfinite(o) and o <= K * e32, (name, row, o, K * e32)
