"""Shared cases of the STOI (Taal et al.) / ESTOI tests (tests/test_stoi_taal_*.py): a restatement of the measure in numpy that
holds its OPERANDS in a chosen dtype and sums in float64, the seeded signals, the case table and the mutants.  Test-side only;
nothing here comes from the package but the launch-free constants it is compared with in the host test.

  float64 operands: the reference of the GPU rows.
  float32 operands (resampling taps, window, DFT matrix, signals, and float32 results where a kernel stores one: the resampled
  samples and the band rows), every sum in float64: the case's e32 = |that value - the float64 value|.

Bounds.  A GPU value passes within K = 16 x e32 of the float64 value, an absolute figure per case and measure; e32 never comes
from a kernel.  The outcomes that involve no arithmetic (1e-5 for fewer than 30 spectral frames, 0.0 for a clean signal of exact
zeros) have e32 = 0 and must be exact.

The keep decision is discontinuous, so the generator asserts that every frame of every case lies at least 1 dB from the 40 dB
threshold in the float64 evaluation, that the clip branch runs in cases 4 and 7, and that the gap cases drop frames.

Signals: clean = 0.5 (1 + 0.5 sin 2 pi 7 t)(sin 2 pi 440 t + 0.5 sin 2 pi 1250 t + 0.3 sin 2 pi 2900 t) + 0.05 N(0, 1); enhanced =
0.8 clean + g N(0, 1), g = 0.15; float32.  A gap multiplies the clean signal by 1e-4 over a sample range before the enhanced signal
is made; a burst adds 2 N(0, 1) to the enhanced signal over a range."""
import math

import numpy as np

K = 16.0
FS, NF, HOP, NFFT, NB, SEG, DYN = 10000, 256, 128, 512, 15, 30, 40.0
EPS = np.finfo(np.float64).eps
SEED = 7
MEASURES = (False, True)                                     # extended

# (number, fs, L, gap, burst, zero_clean)
CASES = (
    (1, 10000, 4095, None, None, False),
    (2, 10000, 4223, None, None, False),
    (3, 10000, 4224, None, None, False),
    (4, 10000, 6000, (2000, 3000), (4000, 4400), False),
    (5, 16000, 6000, None, None, False),
    (6, 16000, 6759, None, None, False),
    (7, 16000, 9600, (3000, 5000), (7000, 7700), False),
    (8, 16000, 9601, (3001, 4990), (7000, 7700), False),
    (9, 16000, 16000, (4000, 7000), None, False),
    (10, 8000, 5000, None, None, False),
    (11, 16000, 200, None, None, False),
    (12, 16000, 9600, None, None, True),
)
# what the issue's table states for the float64 evaluation: {case: (frames, kept, segments)}; None = not stated
EXPECTED = {1: (None, 30, 0), 2: (None, 31, 1), 3: (None, 32, 2), 4: (45, 39, 9), 5: (28, None, 0), 6: (None, 32, 2),
            7: (45, 37, 7), 9: (77, 64, 34), 10: (47, None, 17), 11: (0, 0, 0)}
TOO_SHORT = (1, 5, 11)
# beside the table: (fs, L) of utterances with exactly ONE frame at 10 kHz (256 .. 383 samples there), hence no spectral frame and no
# tile of the bands kernel - alone and in a pack of their own nothing but the keep kernel and the segment kernel has work - and one
# with two frames (one spectral frame).  All score 1e-5.
ONE_FRAME = ((10000, 256), (10000, 383), (16000, 410), (16000, 612), (8000, 205), (8000, 300))
TWO_FRAMES = ((10000, 384), (16000, 613))
MUTANTS = ("hanning(256)", "no silent-frame removal", "no clipping", "last frame taken", "band edges off by one bin")

_cache = {}


def pair(L, fs, gap=None, burst=None, gain=0.15, seed=SEED, zero_clean=False):
    """(clean, enhanced) float32 [L] from the seed alone.  Cached and shared: do not modify."""
    key = (L, fs, gap, burst, gain, seed, zero_clean)
    if key not in _cache:
        r = np.random.default_rng(seed)
        t = np.arange(L) / fs
        c = 0.5 * (1 + 0.5 * np.sin(2 * np.pi * 7 * t)) * (np.sin(2 * np.pi * 440 * t) + 0.5 * np.sin(2 * np.pi * 1250 * t) +
                                                           0.3 * np.sin(2 * np.pi * 2900 * t)) + 0.05 * r.standard_normal(L)
        if gap:
            c[gap[0]:gap[1]] *= 1e-4
        e = 0.8 * c + gain * r.standard_normal(L)
        if burst:
            e[burst[0]:burst[1]] += 2.0 * r.standard_normal(burst[1] - burst[0])
        if zero_clean:
            c = np.zeros(L)
        _cache[key] = (c.astype(np.float32), e.astype(np.float32))
    return _cache[key]


def case_pair(case):
    _, fs, L, gap, burst, zero = case
    return pair(L, fs, gap, burst, zero_clean=zero)


# ---- the restatement ----
def _as(a, dtype):
    """a held in `dtype`, as float64 for the sums"""
    return np.asarray(a).astype(dtype).astype(np.float64)


def taps(up, down):
    """the default filter of scipy.signal.resample_poly(x, up, down), times up"""
    half = 10 * max(up, down)
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(m / max(up, down)) / max(up, down) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def resample(x, fs, dtype=np.float64):
    """x -> 10 kHz: zero stuffing, the filter, every down-th sample from the filter's centre on; ceil(L up / down) samples"""
    if fs == FS:
        return _as(x, dtype)
    g = math.gcd(FS, fs)
    up, down = FS // g, fs // g
    h = _as(taps(up, down), dtype)
    x = _as(x, dtype)
    z = np.zeros(x.size * up)
    z[::up] = x
    full = np.convolve(z, h)
    n = -(-x.size * up // down)
    half = (h.size - 1) // 2
    idx = half + np.arange(n) * down
    y = np.where(idx < full.size, full[np.minimum(idx, full.size - 1)], 0.0)
    return _as(y, dtype)


def band_table(shift=0):
    """[(lo, hi)] x 15 by the rule: centres 150 * 2^(j/3), edges the geometric means of neighbouring centres snapped to the nearest
    bin of linspace(0, 10000, 513)[:257]"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    out = []
    for j in range(NB):
        cf = 150.0 * 2.0 ** (j / 3.0)
        lo, hi = math.sqrt(cf * 150.0 * 2.0 ** ((j - 1) / 3.0)), math.sqrt(cf * 150.0 * 2.0 ** ((j + 1) / 3.0))
        out.append((int(np.argmin((f - lo) ** 2)) + shift, int(np.argmin((f - hi) ** 2)) + shift))
    return out


def stoi64(clean, enhanced, fs, extended=False, dtype=np.float64, mutant=None, info=None):
    """the measure of the issue, steps 0-5, operands in `dtype`, sums in float64.  info: a dict that receives frames, kept,
    segments, margin (dB, the smallest distance of a frame from the threshold) and clipped (share of clipped elements, STOI)."""
    n = min(len(clean), len(enhanced))
    x, y = resample(clean[:n], fs, dtype), resample(enhanced[:n], fs, dtype)
    w = _as(np.hanning(NF) if mutant == "hanning(256)" else np.hanning(NF + 2)[1:-1], dtype)
    starts = list(range(0, x.size - NF + 1, HOP))
    if info is not None:
        info.update(frames=len(starts), kept=0, segments=0, margin=float("inf"), clipped=0.0)
    if not starts:
        return 1e-5
    xf = np.array([w * x[i:i + NF] for i in starts])
    yf = np.array([w * y[i:i + NF] for i in starts])
    e = 20.0 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    mask = (np.max(e) - DYN - e) < 0
    if mutant == "no silent-frame removal":
        mask[:] = True
    xf, yf = xf[mask], yf[mask]
    xs, ys = np.zeros((len(xf) - 1) * HOP + NF), np.zeros((len(xf) - 1) * HOP + NF)
    for i in range(len(xf)):
        xs[i * HOP:i * HOP + NF] += xf[i]
        ys[i * HOP:i * HOP + NF] += yf[i]
    if info is not None:
        info.update(kept=int(mask.sum()), margin=float(np.min(np.abs(np.max(e) - DYN - e))))
    stop = xs.size - NF + (1 if mutant == "last frame taken" else 0)
    ang = 2.0 * np.pi * ((np.arange(NF)[:, None] * np.arange(NFFT // 2 + 1)[None, :]) % NFFT) / NFFT
    C, S = _as(np.cos(ang), dtype), _as(-np.sin(ang), dtype)
    bands = []
    for s in (xs, ys):
        fr = np.array([w * s[i:i + NF] for i in range(0, stop, HOP)]).reshape(-1, NF)
        p = (fr @ C) ** 2 + (fr @ S) ** 2
        tab = band_table(1 if mutant == "band edges off by one bin" else 0)
        bands.append(_as(np.sqrt(np.stack([p[:, lo:hi].sum(1) for lo, hi in tab])), dtype))     # [15, frames]
    xt, yt = bands
    M = xt.shape[1]
    if M < SEG:
        return 1e-5
    xg = np.array([xt[:, m - SEG:m] for m in range(SEG, M + 1)])
    yg = np.array([yt[:, m - SEG:m] for m in range(SEG, M + 1)])
    if info is not None:
        info.update(segments=xg.shape[0])
    if extended:
        def rc(a):
            a = a - a.mean(2, keepdims=True)
            a = a / (np.linalg.norm(a, axis=2, keepdims=True) + EPS)
            a = a - a.mean(1, keepdims=True)
            return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
        return float(np.sum(rc(xg) * rc(yg) / SEG) / xg.shape[0])
    alpha = np.linalg.norm(xg, axis=2, keepdims=True) / (np.linalg.norm(yg, axis=2, keepdims=True) + EPS)
    yn = yg * alpha
    lim = xg * (1.0 + 10.0 ** (15.0 / 20.0))
    if info is not None:
        info.update(clipped=float(np.mean(yn > lim)))
    yp = yn if mutant == "no clipping" else np.minimum(yn, lim)
    yp = yp - yp.mean(2, keepdims=True)
    xz = xg - xg.mean(2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xz = xz / (np.linalg.norm(xz, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xz) / (xg.shape[0] * xg.shape[1]))


def evaluated():
    """{(number, extended): dict(ref, e32, bound, info)} of every case, computed once and shared (do not modify); asserts the
    generator's conditions"""
    if "rows" not in _cache:
        rows = {}
        for case in CASES:
            num, fs = case[0], case[1]
            c, e = case_pair(case)
            for ext in MEASURES:
                info = {}
                ref = stoi64(c, e, fs, ext, np.float64, info=info)
                e32 = abs(stoi64(c, e, fs, ext, np.float32) - ref)
                assert np.isfinite(ref) and info["margin"] >= 1.0, (num, ref, info)
                rows[(num, ext)] = {"ref": ref, "e32": e32, "bound": K * e32, "info": info}
            inf = rows[(num, False)]["info"]
            if num in (4, 7):
                assert inf["clipped"] > 0.0, (num, inf)
            if case[3] is not None:
                assert inf["kept"] < inf["frames"], (num, inf)
        _cache["rows"] = rows
    return _cache["rows"]


def check(name, got, row):
    """print and assert a GPU value against its case: |got - float64| <= K x e32"""
    o = abs(float(got) - row["ref"])
    print("ROW | %s | float64 %.9f | e32 %.2e | bound %.2e | observed %.2e" % (name, row["ref"], row["e32"], row["bound"], o))
    assert np.isfinite(o) and o <= row["bound"], (name, float(got), row["ref"], o, row["bound"])
