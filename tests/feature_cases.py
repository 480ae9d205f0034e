"""Shared cases of the front-end tests (tests/test_features_*.py, tests/golden/make_golden_features.py): a restatement of
signal_processing/features.py in torch that computes in the dtype of its arguments (float64: the reference of the GPU rows;
float32: the row's e32), the seeded signals and the mutants.  Test-side only.  The windows and matrices come from the package's
host functions, which tests/test_features_host.py pins to the reference's own values.

Signals are gammatone_cases.signal: a signal of at least 1000 samples carries 600 exact zeros, so whole frames (their 160 samples
and the sample before them) are silent.  The RASTA filter is the direct form II transposed of lfilter, as scipy runs it."""
import numpy as np
import torch

import gammatone_cases as gc
from sincformer_metacog_speech_enhancement_amd import config
from sincformer_metacog_speech_enhancement_amd.signal_processing import features as ft

K = 16.0                                                     # the rows' factor over e32 (helpers.check_row)
FRAME, HOP, CTX = 160, 80, 5
BLOCKS = {"ams": slice(0, 15), "rasta": slice(15, 28), "mfcc": slice(28, 41), "gfcc": slice(41, 54)}
# (case name, fs, L, signal kind, seed)
SINGLE = (
    ("p100", 8000, 100, "noise", 401),                       # padded to one frame
    ("s160", 8000, 160, "tone", 402),                        # one frame; its context is 11 copies
    ("s239", 8000, 239, "noise", 403),                       # the frame-count boundary
    ("s240", 8000, 240, "tone", 404),
    ("s401", 8000, 401, "noise", 405),                       # around the tap count
    ("s1041", 8000, 1041, "tone", 406),
    ("s1153", 8000, 1153, "tone", 407),                      # a fourth workgroup of the FIR kernel
    ("s2403", 8000, 2403, "noise", 408),                     # 29 frames
    ("k2403", 16000, 2403, "tone", 409),                     # the second sample rate
)
CASES = {c[0]: c for c in SINGLE}
RAGGED = ("s2403", "s160", "s1041")                          # the padded batch: these cases as rows, with lengths
GOLDEN_CONTEXT = ("s160", "s401")
AMS_CASES = ("s1041", "s1153", "s2403", "k2403")             # stand-alone extract_ams: one to three segments (131+ decimated samples)
MUTANTS = ("pre-emphasis dropped at a frame's sample 0", "GFCC window at [80 n, 80 n + 80)", "RASTA state carried across utterances",
           "mean over T instead of T_b", "context wraps instead of clamping", "DCT without the k = 0 scaling")

_cache = {}


def case_signal(name):
    """float32 [L] of a case, from its seed alone.  Cached and shared: do not modify."""
    if ("sig", name) not in _cache:
        _, _, L, kind, seed = CASES[name]
        _cache[("sig", name)] = gc.signal(L, seed, kind)
    return _cache[("sig", name)]


def bank(fs):
    if ("bank", fs) not in _cache:
        _cache[("bank", fs)] = ft.GammatoneFilterbank(sample_rate=fs)
    return _cache[("bank", fs)]


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def padded_signal(x):
    return torch.nn.functional.pad(x, (0, FRAME - x.numel())) if x.numel() < FRAME else x


def dct(v, num_coeffs, mutant=None):
    """v [.., M] -> [.., num_coeffs]: the orthonormal DCT-II"""
    rows = ft.dct_rows(num_coeffs, v.shape[-1])
    if mutant == "DCT without the k = 0 scaling":
        rows[0] *= np.sqrt(2.0)
    return v @ _t(rows, v.dtype).T


def power_frames(x, n_fft):
    """x [L] -> |rfft(hamming * frame, n_fft)|^2 [T, n_fft // 2 + 1]"""
    f = x.unfold(0, FRAME, HOP) * _t(ft.hamming(FRAME), x.dtype)
    return torch.fft.rfft(f, n=n_fft, dim=-1).abs() ** 2


def mfcc_rows(x, fs, mutant=None, raw_len=None):
    """raw_len: the pre-emphasis is taken on the first raw_len samples and padded afterwards (stand-alone extract_mfcc)"""
    pre = torch.cat([x[:1], x[1:] - 0.97 * x[:-1]])
    if raw_len is not None:
        pre[raw_len:] = 0
    f = pre.unfold(0, FRAME, HOP).clone()
    if mutant == "pre-emphasis dropped at a frame's sample 0":
        f[:, 0] = x.unfold(0, FRAME, HOP)[:, 0]
    f = f * _t(ft.hamming(FRAME), x.dtype)
    power = torch.fft.rfft(f, n=config.MFCC_FFT_SIZE, dim=-1).abs() ** 2
    mel = power @ _t(ft.mel_filterbank(config.MFCC_NUM_FILTERS, config.MFCC_FFT_SIZE, fs), x.dtype).T
    return dct(torch.log(mel + 1e-10), config.MFCC_NUM_COEFF, mutant)


def log_bark(x, fs):
    return torch.log(power_frames(x, config.FFT_SIZE) @ _t(ft.bark_filterbank(fs)[0], x.dtype).T + 1e-10)     # [T, 21]


def rasta_filter(lb, state=None):
    """lb [T, M] -> (lfilter([.2, .1, 0, -.1, -.2], [1, -.98]) along T, final state): direct form II transposed"""
    z = [torch.zeros_like(lb[0]) for _ in range(4)] if state is None else list(state)
    out = torch.empty_like(lb)
    for n in range(lb.shape[0]):
        x = lb[n]
        y = 0.2 * x + z[0]
        z = [0.1 * x + z[1] + 0.98 * y, 0.0 * x + z[2], -0.1 * x + z[3], -0.2 * x]
        out[n] = y
    return out, z


def rasta_vector(x, fs, mutant=None, state=None, mean_over=None):
    lb = log_bark(x, fs)
    y, _ = rasta_filter(lb, state)
    loud = (torch.exp(y) * _t(ft.bark_filterbank(fs)[1], x.dtype)) ** (1.0 / 3.0)
    mean = loud.sum(0) / (mean_over or loud.shape[0])
    return dct(mean, config.RASTA_NUM_COEFF, mutant)


def gfcc_rows(x, fs, mutant=None, standalone=False):
    b = bank(fs)
    y = gc.fir(x, gc.taps_of(b, x.dtype))                                     # [C, L]
    w = fs // config.GFCC_DECIMATE_RATE
    if standalone:
        e = (y[:, :x.numel() // w * w].reshape(y.shape[0], -1, w) ** 2).mean(-1).T
    else:
        T = (x.numel() - FRAME) // HOP + 1
        start = [n * HOP for n in range(T)] if mutant == "GFCC window at [80 n, 80 n + 80)" else \
                [n * HOP + FRAME // 2 - w // 2 for n in range(T)]
        e = torch.stack([(y[:, s:s + w] ** 2).mean(-1) for s in start])       # [T, C]
    return dct(torch.sign(e) * e.abs() ** (1.0 / 3.0), config.GFCC_NUM_COEFF, mutant)


def frame_features(name, dtype, mutant=None, state_from=None, mean_over=None):
    """extract_frame_features of a case in `dtype` -> [T, 54].  Cached per (case, dtype, mutant, ..): do not modify.
    state_from: the case whose RASTA state is carried into this one (mutant); mean_over: the divisor of the RASTA mean (mutant)."""
    key = ("ff", name, dtype, mutant, state_from, mean_over)
    if key not in _cache:
        fs = CASES[name][1]
        x = padded_signal(case_signal(name).to(dtype))
        T = (x.numel() - FRAME) // HOP + 1
        state = None
        if state_from is not None:
            state = rasta_filter(log_bark(padded_signal(case_signal(state_from).to(dtype)), fs))[1]
        out = torch.zeros(T, 54, dtype=dtype)
        out[:, BLOCKS["rasta"]] = rasta_vector(x, fs, mutant, state, mean_over)[None, :]
        out[:, BLOCKS["mfcc"]] = mfcc_rows(x, fs, mutant)
        out[:, BLOCKS["gfcc"]] = gfcc_rows(x, fs, mutant)
        _cache[key] = out
    return _cache[key]


def standalone(name, dtype):
    """dict(mfcc, gfcc, rasta [13], ams [15]) of the stand-alone extractors on a case signal in `dtype`.  Cached: do not modify."""
    key = ("alone", name, dtype)
    if key not in _cache:
        fs = CASES[name][1]
        raw = case_signal(name).to(dtype)
        x = padded_signal(raw)
        _cache[key] = {"mfcc": mfcc_rows(x, fs, raw_len=raw.numel()).mean(0), "rasta": rasta_vector(x, fs), "ams": ams(raw, fs),
                       "gfcc": gfcc_rows(raw, fs, standalone=True).mean(0) if raw.numel() >= fs // config.GFCC_DECIMATE_RATE
                       else torch.zeros(config.GFCC_NUM_COEFF, dtype=dtype)}
    return _cache[key]


def ams(x, fs):
    """stand-alone extract_ams: |x|[::8], segments of 128 at hop 64, Hamming, 256-point magnitude, 15 triangles, / num_segs"""
    d = x.abs()[::8]
    seg, hop = config.AMS_SEGMENTS, config.AMS_SEGMENTS - config.AMS_OVERLAP
    if d.numel() < seg:
        return torch.zeros(config.AMS_NUM_BANDS, dtype=x.dtype)
    f = d.unfold(0, seg, hop) * _t(ft.hamming(seg), x.dtype)
    mag = torch.fft.rfft(f, n=config.AMS_FFT_SIZE, dim=-1).abs()
    return (mag @ _t(ft.ams_filterbank(fs), x.dtype).T).sum(0) / max(1, (d.numel() - seg) // hop + 1)


def context(feat, Tb=None, mean=None, std=None, mutant=None):
    """feat [T, D] -> [T, 11 D]: rows clamp(n - 5 .. n + 5, 0, Tb - 1) side by side (0 from Tb on), then - with statistics -
    nan / inf -> 0, (f - mean) / std, clip to +-10, in feat's dtype"""
    T, D = feat.shape
    Tb = T if Tb is None else Tb
    n = torch.arange(T)[:, None] + torch.arange(-CTX, CTX + 1)[None, :]
    idx = n % Tb if mutant == "context wraps instead of clamping" else n.clamp(0, Tb - 1)
    out = feat[idx].reshape(T, -1)
    if mean is not None:
        out = torch.nan_to_num(out, nan=0.0, posinf=0.0, neginf=0.0)
        out = ((out - mean.to(feat.dtype)) / std.to(feat.dtype)).clamp(-10.0, 10.0)
    out = out.clone()
    out[Tb:] = 0
    return out


def statistics(seed=77):
    """(mean, std) float32 [594]: seeded stand-ins for the Dataset's statistics, std in [0.5, 2]; some rows clip at +-10"""
    rng = np.random.RandomState(seed)
    mean = rng.standard_normal(594).astype(np.float32)
    std = (0.5 + 1.5 * rng.random_sample(594)).astype(np.float32)
    std[BLOCKS["mfcc"]] = 0.05                                # the MFCC block of the first context frame leaves +-10
    return torch.from_numpy(mean), torch.from_numpy(std)


def silent_frames(name):
    """[first, last) of the frames whose 160 samples and the sample before them lie inside the exact zeros (MFCC's view)"""
    L = CASES[name][2]
    a, z = gc.zero_stretch(L)
    first = -(-(a + 1) // HOP)
    last = min((a + z - FRAME) // HOP + 1, (max(L, FRAME) - FRAME) // HOP + 1)
    return first, max(first, last)


def silent_mfcc_row():
    """the MFCC row of a wholly silent frame: the DCT of 64 copies of log(1e-10)"""
    return dct(torch.full((config.MFCC_NUM_FILTERS,), float(np.log(1e-10)), dtype=torch.float64), config.MFCC_NUM_COEFF)
