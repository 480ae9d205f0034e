"""Shared cases of the CSII / NCM tests (tests/test_intelligibility_*.py, tests/golden/make_golden_intelligibility.py):
restatements of evaluation/csii.py and evaluation/ncm.py in numpy that compute in the dtype of their OPERANDS and reduce in
float64, the seeded signals and the mutants.  Test-side only.

  float64 operands: the reference of the GPU rows (tests/test_intelligibility_host.py holds it to the reference's own values);
  float32 operands (DFT matrix, gammatone taps, Hilbert table, signal) and float32 results where a kernel stores one (the
  spectra, the filtered planes, the transform), every sum in float64: the row's e32 = its distance from the float64 evaluation.

Bounds.  A GPU row passes when its largest error, relative to the row's largest float64 value, is within K = 16 x e32.
e32 of a plane (envelope, msc, ncc) is that same figure of the float32-operand evaluation.  The two scores are convex
combinations of their planes (the SII weights and the channel weights are non-negative and sum to at most 1, max(., 0) and the
clips are 1-Lipschitz), so a score's error is at most its plane's largest error: the score is held to K x (the plane's e32 x
the plane's largest value), an absolute figure.  e32 never comes from a kernel's output.

Signals (pair(L, seed, fs)): clean = an amplitude-modulated 440 Hz tone 0.5 (1 + 0.5 sin 2 pi 7 t) sin plus 0.05 N(0, 1);
enhanced = 0.8 clean + 0.15 N(0, 1); float32.  The levels keep every case away from the two guards of the reference (msc's
1e-10 beside Pxx Pyy, ncc's denom < 1e-10), where no fp32 bound means anything: the generator asserts that each Pxx Pyy and each
sqrt(var var) is exactly 0 or above 1e-6."""
import numpy as np

from sincformer_metacog_speech_enhancement_amd.evaluation import csii as pcsii, ncm as pncm
from sincformer_metacog_speech_enhancement_amd.signal_processing import gammatone as gt

K = 16.0
N_FFT = 256
BANKS = {"default": {}, "fs16k": {"sample_rate": 16000}, "ch20": {"num_channels": 20}}

# 256 = the output tile, 64 = the k-step of a convolution: one below, at, one above, for an odd length (L samples, no "at") and
# for an even one (two convolutions of L / 2 samples)
HILBERT_L = (64, 65, 255, 256, 257, 1000, 1001, 63, 127, 128, 129, 126, 130, 510, 512, 514)
HILBERT_ROWS = 3


def _csii_lengths(fs):
    frame = int(0.016 * fs)
    hop = frame // 2
    return (frame - 1, frame, frame + hop - 1, frame + hop, 1237, 4000)


# (name, fs, L, seed)
CSII_CASES = tuple(("c%d_%d" % (fs // 1000, L), fs, L, 500 + i) for fs in (8000, 16000) for i, L in enumerate(_csii_lengths(fs))) + \
    (("c22_1400", 22050, 1400, 520),)      # 6 frames of 352 samples; 7 if the cropped 256 were counted
CSII_GOLDEN_LENGTHS = {fs: _csii_lengths(fs) + (2 * int(0.016 * fs), 2 * int(0.016 * fs) + 1) for fs in (8000, 16000)}
# (name, bank, fs, L, seed)
NCM_CASES = (("n63", "default", 8000, 63, 601), ("n64", "default", 8000, 64, 602), ("n65", "default", 8000, 65, 603),
             ("n1237", "default", 8000, 1237, 604), ("n2000", "default", 8000, 2000, 605), ("k2403", "fs16k", 16000, 2403, 606),
             ("c401", "ch20", 8000, 401, 607))
RAGGED = (2000, 64, 1237, 63, 401)
RAGGED_SEED = 700

HILBERT_MUTANTS = ("linear convolution", "even-L table at odd L", "Nyquist bin doubled")
NCM_MUTANTS = ("means not removed",)
CSII_MUTANTS = ("rectangular window", "n_fft = frame at 8 kHz", "|Pxy| not squared", "frames counted with the cropped frame")

_cache = {}


def bank(name):
    """the package's GammatoneFilterbank of BANKS[name] (host design only; shared: do not modify)"""
    if ("bank", name) not in _cache:
        _cache[("bank", name)] = gt.GammatoneFilterbank(**BANKS[name])
    return _cache[("bank", name)]


def pair(L, seed, fs=8000):
    """(clean, enhanced) float32 [L], from the seed alone.  Cached and shared: do not modify."""
    key = ("pair", L, seed, fs)
    if key not in _cache:
        rng = np.random.RandomState(seed)
        t = np.arange(L) / float(fs)
        c = 0.5 * (1.0 + 0.5 * np.sin(2 * np.pi * 7.0 * t)) * np.sin(2 * np.pi * 440.0 * t) + 0.05 * rng.standard_normal(L)
        e = 0.8 * c + 0.15 * rng.standard_normal(L)
        _cache[key] = (c.astype(np.float32), e.astype(np.float32))
    return _cache[key]


def hilbert_rows(L):
    """float32 [HILBERT_ROWS, L]: a clean signal, its enhanced version and noise"""
    c, e = pair(L, 400 + L)
    return np.stack([c, e, (0.1 * np.random.RandomState(900 + L).standard_normal(L)).astype(np.float32)])


# ---- figures ----
def fig(got, ref64):
    """largest |got - ref| over the row's largest |ref|"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    return float(np.abs(got - ref64).max()) / max(float(np.abs(ref64).max()), 1e-300)


def check(name, got, ref64, ref32):
    """print and assert a plane row: fig(got) <= K x e32"""
    e32, o = fig(ref32, ref64), fig(got, ref64)
    print("ROW | %s | e32 %.2e | bound %.2e | observed %.2e" % (name, e32, K * e32, o))
    assert np.isfinite(o) and o <= K * e32, (name, o, K * e32)


def check_score(name, got, ref64, plane64, plane32):
    """print and assert a score against the absolute bound K x e32(plane) x max|plane| (module docstring)"""
    bound = K * fig(plane32, plane64) * float(np.abs(plane64).max())
    o = abs(float(got) - float(ref64))
    print("ROW | %s | float64 %.6f | bound %.2e | observed %.2e" % (name, float(ref64), bound, o))
    assert np.isfinite(o) and o <= bound, (name, o, bound)


# ---- Hilbert transform and envelope ----
def hilbert_h(L, mutant=None):
    """float64 [L]: the circular kernel of scipy.signal.hilbert(.).imag"""
    H = np.zeros(L)
    even = L % 2 == 0 or mutant == "even-L table at odd L"
    if even:
        H[0] = H[L // 2] = 1.0
        H[1:L // 2] = 2.0
    else:
        H[0] = 1.0
        H[1:(L + 1) // 2] = 2.0
    return np.fft.ifft(H).imag


def hilbert64(x, dtype=np.float64, mutant=None):
    """x [.., L] -> (y, env): y = h (*) x circularly with h and x held in `dtype`, summed in float64 and held in `dtype` (the matrix
    cores' result is a float32 word); env = sqrt(x^2 + y^2) in float64"""
    x = np.asarray(x)
    L = x.shape[-1]
    h = hilbert_h(L, mutant).astype(dtype).astype(np.float64)
    xd = x.astype(dtype).astype(np.float64)
    idx = (np.arange(L)[:, None] - np.arange(L)[None, :])
    M = h[idx % L]
    if mutant == "linear convolution":
        M = np.where(idx >= 0, M, 0.0)
    y = (xd @ M.T).astype(dtype).astype(np.float64)
    re = xd
    if mutant == "Nyquist bin doubled" and L % 2 == 0:       # H[L / 2] = 2 leaves the imaginary part alone and adds the Nyquist
        sign = 1.0 - 2.0 * (np.arange(L) % 2)                # component once more to the REAL part of the analytic signal
        re = xd + sign * (xd @ sign)[..., None] / L
    return y, np.sqrt(re * re + y * y)


# ---- NCM ----
def fir64(x, taps, dtype):
    """x [L], taps [C, K] -> [C, L] causal FIR with operands held in `dtype`, summed in float64; float32: the result is then
    rounded to float32, as the filter kernel stores it"""
    xd = x.astype(dtype).astype(np.float64)
    td = taps.astype(dtype).astype(np.float64)
    y = np.stack([np.convolve(xd, td[c])[:x.shape[0]] for c in range(td.shape[0])])
    return y.astype(dtype).astype(np.float64)


def ncm64(clean, enhanced, b, dtype=np.float64, mutant=None):
    """-> (score, ncc [C]) of evaluation/ncm.py with the bank `b`, operands in `dtype`"""
    n = min(len(clean), len(enhanced))
    C = b.num_channels
    if n < 64:
        return 0.0, np.zeros(C)
    taps = np.stack(b.impulse_responses)
    ncc = np.zeros(C)
    envs = [hilbert64(fir64(np.asarray(s[:n]), taps, dtype), dtype)[1] for s in (clean, enhanced)]
    for c in range(C):
        ec, ee = envs[0][c], envs[1][c]
        if mutant != "means not removed":
            ec, ee = ec - ec.mean(), ee - ee.mean()
        den = np.sqrt(np.mean(ec * ec) * np.mean(ee * ee))
        ncc[c] = 0.0 if den < 1e-10 else np.clip(np.mean(ec * ee) / den, -1, 1)
    w = pncm.channel_weights(b.center_freqs)
    return float(np.clip(np.sum(w * np.maximum(ncc, 0)), 0.0, 1.0)), ncc


def ncm_denominators(clean, enhanced, b):
    """sqrt(var var) per channel in float64 (the generator asserts each is 0 or above 1e-6)"""
    taps = np.stack(b.impulse_responses)
    n = min(len(clean), len(enhanced))
    envs = [hilbert64(fir64(np.asarray(s[:n]), taps, np.float64))[1] for s in (clean, enhanced)]
    return np.sqrt(envs[0].var(axis=1) * envs[1].var(axis=1))


# ---- CSII ----
def msc64(clean, enhanced, fs, dtype=np.float64, mutant=None, want_den=False):
    """-> msc [129] (None when the signals hold no frame): the coherence of evaluation/csii.py over all frames, DFT matrix and
    signal held in `dtype`, products summed in float64, spectra rounded to `dtype` as the DFT kernel stores them"""
    n = min(len(clean), len(enhanced))
    frame = int(0.016 * fs)
    hop = frame // 2
    n_fft = frame if (mutant == "n_fft = frame at 8 kHz" and fs == 8000) else N_FFT
    Kf = min(frame, n_fft)
    count_frame = Kf if mutant == "frames counted with the cropped frame" else frame
    if n < count_frame:
        return None
    T = (n - count_frame) // hop + 1
    w = np.ones(frame) if mutant == "rectangular window" else np.hamming(frame)
    F = n_fft // 2 + 1
    ang = 2.0 * np.pi * ((np.arange(Kf)[:, None] * np.arange(F)[None, :]) % n_fft) / n_fft
    Mre = (w[:Kf, None] * np.cos(ang)).astype(dtype).astype(np.float64)
    Mim = (-w[:Kf, None] * np.sin(ang)).astype(dtype).astype(np.float64)
    spec = []
    for s in (clean, enhanced):
        xd = np.asarray(s[:n]).astype(dtype).astype(np.float64)
        fr = np.stack([xd[t * hop:t * hop + Kf] for t in range(T)])
        spec.append(((fr @ Mre).astype(dtype).astype(np.float64), (fr @ Mim).astype(dtype).astype(np.float64)))
    (a0, a1), (b0, b1) = spec
    pxx = (a0 * a0 + a1 * a1).sum(0) / T
    pyy = (b0 * b0 + b1 * b1).sum(0) / T
    pr = (a0 * b0 + a1 * b1).sum(0) / T
    pi = (a1 * b0 - a0 * b1).sum(0) / T
    mag2 = pr * pr + pi * pi
    if mutant == "|Pxy| not squared":
        mag2 = np.sqrt(mag2)
    msc = np.clip(mag2 / (pxx * pyy + 1e-10), 0, 1)
    if F != N_FFT // 2 + 1:                                  # (a mutant's other bin count: compared over the common bins' weights)
        msc = np.interp(np.arange(N_FFT // 2 + 1) * fs / N_FFT, np.arange(F) * fs / n_fft, msc)
    return (msc, pxx * pyy) if want_den else msc


def csii64(clean, enhanced, fs, dtype=np.float64, mutant=None):
    """-> (score, msc [129]) of evaluation/csii.py (any num_levels >= 1)"""
    msc = msc64(clean, enhanced, fs, dtype, mutant)
    if msc is None:
        return 0.0, np.zeros(N_FFT // 2 + 1)
    return float(np.clip(np.sum(pcsii.sii_weights(fs) * msc), 0, 1)), msc
