"""Shared cases of the gammatone tests (tests/test_gammatone_*.py, tests/golden/make_golden_gammatone.py): a restatement of
signal_processing/gammatone.py's T-F analysis in torch, computing in the dtype of its arguments (float64: the reference of the
GPU rows; float32: the row's e32), in two forms -

  direct     causal FIR (conv1d), frames, rfft: what the reference does;
  five-sum   {sum f^2, sum f, sum (-1)^t f, sum f cos, sum f sin} per frame, or per hop-block and then combined by one rotation:
             what the kernels do;

the seeded signals and the mutants.  Test-side only.  The filter design comes from the package's host functions, which
tests/test_gammatone_host.py pins to the reference bit for bit.

Signals (signal(L, seed, kind)): 'tone' = an amplitude-modulated 440 Hz tone 0.1 (1 + 0.5 sin) sin plus 0.01 N(0, 1), 'noise' =
0.1 N(0, 1); float32.  A signal of at least 1000 samples carries 600 exact zeros in the middle: the 399 samples of history of
the default bank's 400 taps, one frame of 160 and 41 to spare, so the stretch starts 399 samples before a multiple of the hop
(the first one at or behind the centred position) and exactly one default frame lies wholly behind the taps' reach: its planes
must be exactly 0.  A shorter signal has no room for that and carries L // 3 zeros, which silence no frame.

Units below the tap operand's range: the kernels' tap operand is fp32, which holds nothing below 2^-149 and loses bits below
2^-126, while the float64 design keeps taps down to 1e-64.  In the decay behind the stretch's start a few units are built from
such taps alone; their float64 values (down to 1e-60 of the plane's largest) cannot be had from any fp32 operand.  A unit whose
frame norm sqrt(w sum f^2) is at most 2^-100 of the plane's largest is therefore `dead` (live_units): it stays in every row that
is measured against the plane's largest value and leaves the rows that are measured against the unit's own norm."""
import math

import numpy as np
import torch

from sincformer_metacog_speech_enhancement_amd.signal_processing import gammatone as gt

K = 16.0                                                    # the rows' factor over e32 (helpers.check_row)
FRAME, HOP, FFT = 160, 80, 256

# filterbank configurations: name -> GammatoneFilterbank arguments
BANKS = {"default": {}, "fs16k": {"sample_rate": 16000}, "ch20": {"num_channels": 20}}
# (case name, bank, L or the lengths of a padded batch, signal kind, seed, framing (frame, hop, fft))
SINGLE = (
    ("d160", "default", 160, "noise", 301, (FRAME, HOP, FFT)),           # one frame, shorter than the taps
    ("d239", "default", 239, "tone", 302, (FRAME, HOP, FFT)),            # a trailing partial block that belongs to no frame
    ("d240", "default", 240, "noise", 303, (FRAME, HOP, FFT)),
    ("d400", "default", 400, "tone", 304, (FRAME, HOP, FFT)),            # around the tap count
    ("d401", "default", 401, "noise", 305, (FRAME, HOP, FFT)),
    ("d559", "default", 559, "tone", 306, (FRAME, HOP, FFT)),
    ("d1153", "default", 1153, "tone", 307, (FRAME, HOP, FFT)),          # 3 x 384 + 1: a fourth workgroup of either kernel
    ("d2403", "default", 2403, "noise", 308, (FRAME, HOP, FFT)),
    ("d1041", "default", 1041, "tone", 309, (FRAME, HOP, FFT)),
    ("k1153", "fs16k", 1153, "noise", 310, (FRAME, HOP, FFT)),           # 800 taps, other cf bins
    ("k2403", "fs16k", 2403, "tone", 311, (FRAME, HOP, FFT)),
    ("c239", "ch20", 239, "noise", 312, (FRAME, HOP, FFT)),              # 20 channels: padded operand columns
    ("c1153", "ch20", 1153, "tone", 313, (FRAME, HOP, FFT)),
    ("g401", "default", 401, "tone", 314, (200, 64, FFT)),               # a general framing: filter + moments
    ("g2403", "default", 2403, "noise", 315, (200, 64, FFT)),
    ("f559", "default", 559, "noise", 316, (FRAME, HOP, 128)),           # fft_size < frame_size: the crop
    ("f2403", "default", 2403, "tone", 317, (FRAME, HOP, 128)),
)
CASES = {c[0]: c for c in SINGLE}
RAGGED = ("d2403", "d160", "d1041")                          # the padded batch: these cases as rows, with lengths
GOLDEN_CASES = ("d160", "d239", "d240", "d400", "d401", "d559", "d1153", "d2403", "d1041", "k2403", "c1153", "g401", "f559")
GOLDEN_FILTER = ("d559", (0, 21, 42, 63))
MUTANTS = ("norot", "noparity", "hist128", "cfbin+1", "parityflip", "lastpartial")

_cache = {}


def bank(name):
    """the package's GammatoneFilterbank of BANKS[name] (host design only; shared: do not modify)"""
    if ("bank", name) not in _cache:
        _cache[("bank", name)] = gt.GammatoneFilterbank(**BANKS[name])
    return _cache[("bank", name)]


def zero_stretch(L):
    """(start, length) of the exact zeros of a signal of L samples"""
    if L < 1000:
        return (L - L // 3) // 2, L // 3
    return -(-((L - 600) // 2 + 399) // HOP) * HOP - 399, 600


def signal(L, seed, kind):
    rng = np.random.RandomState(seed)
    n = rng.standard_normal(L)
    if kind == "tone":
        t = np.arange(L) / 8000.0
        x = 0.1 * (1.0 + 0.5 * np.sin(2 * np.pi * 7.0 * t)) * np.sin(2 * np.pi * 440.0 * t) + 0.01 * n
    else:
        x = 0.1 * n
    a, z = zero_stretch(L)
    x[a:a + z] = 0.0
    return torch.from_numpy(x.astype(np.float32))


def case_signal(name):
    """float32 [L] of a case, from its seed alone.  Cached and shared: do not modify."""
    if ("sig", name) not in _cache:
        _, _, L, kind, seed, _ = CASES[name]
        _cache[("sig", name)] = signal(L, seed, kind)
    return _cache[("sig", name)]


def silent_frames(name):
    """[first, last) of the frames whose samples AND whose taps' history are all inside the zero stretch (empty when none)"""
    _, bname, L, _, _, (frame, hop, _) = CASES[name]
    a, z = zero_stretch(L)
    taps = len(bank(bname).impulse_responses[0])
    first = -(-(a + taps - 1) // hop)                       # first n with n hop - (taps - 1) >= a
    T = (L - frame) // hop + 1
    last = min((a + z - frame) // hop + 1, T)               # last n with n hop + frame <= a + z, exclusive
    return (first, max(first, last))


# ---- the restatement, in the dtype of x ----
def taps_of(b, dtype, cut=None):
    h = torch.from_numpy(np.stack(b.impulse_responses)).to(dtype)           # [C, taps]
    if cut is not None:
        h = h[:, :cut]
    return h


def fir(x, h):
    """x [L], h [C, taps] -> [C, L]: (x * h_c)[:L]"""
    taps = h.shape[1]
    xp = torch.nn.functional.pad(x, (taps - 1, 0))[None, None]
    return torch.nn.functional.conv1d(xp, h.flip(-1)[:, None])[0]


def frames_of(y, frame, hop):
    return y.unfold(-1, frame, hop)                                           # [C, T, frame]


def direct(y, frame, hop, N, bins):
    """-> dict(mag, re, im, phase [C, T], norm): through the rfft, as the reference"""
    f = frames_of(y, frame, hop)
    S = torch.fft.rfft(f, n=N, dim=-1)
    idx = torch.as_tensor(bins).view(-1, 1, 1).expand(-1, f.shape[1], 1)
    s = torch.gather(S, 2, idx)[..., 0]
    w = min(frame, N)
    return {"mag": (S.abs() ** 2).sum(-1), "re": s.real, "im": s.imag, "phase": torch.angle(s),
            "norm": torch.sqrt(w * (f[..., :w] ** 2).sum(-1))}


def twiddles(n_t, N, bins, dtype):
    """cos, sin [C, n_t] of 2 pi ((k t) mod N) / N, evaluated in float64 and rounded to dtype"""
    k = torch.as_tensor(bins, dtype=torch.int64).view(-1, 1)
    idx = (k * torch.arange(n_t, dtype=torch.int64)) % N
    ang = 2.0 * math.pi * idx.double() / N
    sin = torch.sin(ang)
    sin[(idx == 0) | (2 * idx == N)] = 0.0
    return torch.cos(ang).to(dtype), sin.to(dtype)


def five_sums(f, N, bins, parity=True):
    """f [C, R, n_t] (frames or blocks, local t) -> [C, R, 5] = {sum f^2, sum f, sum (-1)^t f, sum f cos, sum f sin}"""
    n_t = f.shape[-1]
    cs, sn = twiddles(n_t, N, bins, f.dtype)
    sign = torch.ones(n_t, dtype=f.dtype)
    sign[1::2] = -1.0
    sp = (f * sign).sum(-1) if parity else torch.zeros_like(f[..., 0])
    return torch.stack([(f * f).sum(-1), f.sum(-1), sp, (f * cs[:, None, :]).sum(-1), (f * sn[:, None, :]).sum(-1)], dim=-1)


def combine_blocks(p, hop, N, bins, mutant=None):
    """block sums p [C, nblocks, 5] -> frame sums [C, nblocks - 1, 5]: frame n = block n + exp(-2 pi i k hop / N) block n + 1"""
    k = torch.as_tensor(bins, dtype=torch.int64)
    ang = 2.0 * math.pi * ((k * hop) % N).double() / N
    rc, rs = torch.cos(ang).to(p.dtype)[:, None], torch.sin(ang).to(p.dtype)[:, None]
    if mutant == "norot":
        rc, rs = torch.ones_like(rc), torch.zeros_like(rs)
    a, b = p[:, :-1], p[:, 1:]
    sp = a[..., 2] + (-b[..., 2] if mutant == "parityflip" else b[..., 2])
    return torch.stack([a[..., 0] + b[..., 0], a[..., 1] + b[..., 1], sp,
                        a[..., 3] + rc * b[..., 3] - rs * b[..., 4], a[..., 4] + rc * b[..., 4] + rs * b[..., 3]], dim=-1)


def finish(s, N):
    """frame sums [C, T, 5] -> dict(mag, re, im, phase)"""
    re, im = s[..., 3], -s[..., 4]
    return {"mag": 0.5 * (N * s[..., 0] + s[..., 1] ** 2 + s[..., 2] ** 2), "re": re, "im": im, "phase": torch.atan2(im, re)}


def block_sums(y, hop, N, bins):
    nb = y.shape[-1] // hop
    return five_sums(y[:, :nb * hop].reshape(y.shape[0], nb, hop), N, bins)


def analysis(name, dtype, mutant=None):
    """a case evaluated in `dtype` -> dict(y [C, L]; direct: mag / re / im / phase / norm [C, T]; sums: the five-sum form's mag /
    re / im / phase; blocks [C, nblocks, 5] where the framing is the fused one).  Cached per (case, dtype, mutant): do not modify.
    mutant 'lastpartial' appends the frame that the trailing partial block (zero-padded) would give."""
    key = ("ana", name, dtype, mutant)
    if key in _cache:
        return _cache[key]
    _, bname, L, _, _, (frame, hop, N) = CASES[name]
    b = bank(bname)
    bins = b.cf_bins(N)
    if mutant == "cfbin+1":
        bins = [min(k + 1, N // 2) for k in bins]
    x = case_signal(name).to(dtype)
    y = fir(x, taps_of(b, dtype, 128 if mutant == "hist128" else None))
    out = {"y": y}
    out.update(direct(y, frame, hop, N, bins))
    w = min(frame, N)
    fused = hop * 2 == frame and hop % 2 == 0 and N >= frame
    if fused:
        yb = y
        if mutant == "lastpartial" and L % hop:
            yb = torch.nn.functional.pad(y, (0, hop - L % hop))
        out["blocks"] = block_sums(yb, hop, N, bins)
        s = combine_blocks(out["blocks"], hop, N, bins, mutant)
        if mutant == "noparity":
            s[..., 2] = 0.0
    else:
        s = five_sums(frames_of(y, frame, hop)[..., :w], N, bins, parity=mutant != "noparity")
    out["sums"] = finish(s, N)
    _cache[key] = out
    return out


def padded(plane, T):
    """[C, t] -> [C, T] with zeros behind: an utterance's plane as a row of a padded batch"""
    return torch.nn.functional.pad(plane, (0, T - plane.shape[-1]))


# ---- the rows' bounds ----
def live_units(norm64):
    """bool [C, T]: the frame norm is above 2^-100 of the plane's largest (see the module docstring)"""
    n = norm64.double()
    return n > n.max() * 2.0 ** -100


def normalised(plane, norm64):
    """a bin plane over the Cauchy-Schwarz norm sqrt(w sum f^2) of its frame (float64); 0 at silent and dead units"""
    n = norm64.double()
    return torch.where(live_units(n), plane.double() / n.clamp_min(1e-300), torch.zeros_like(n))


def bin_error_bound(name):
    """e of the bin row, in units of the frame norm: K x the larger of the float32 five-sum form's errors in re and im"""
    a64, a32 = analysis(name, torch.float64), analysis(name, torch.float32)
    n = a64["norm"]
    return K * max(float((normalised(a32["sums"][q], n) - normalised(a64[q], n)).abs().max()) for q in ("re", "im"))


def phase_bound(name):
    """(bound [C, T] rad, keep [C, T] bool, skipped): 2 e / (|S64[cf_bin]| / norm) at the live units; keep = live and the bound
    is at most 0.1 rad; skipped = the live units that are not kept"""
    a64 = analysis(name, torch.float64)
    live = live_units(a64["norm"])
    size = normalised(torch.sqrt(a64["re"] ** 2 + a64["im"] ** 2), a64["norm"])
    bound = torch.where(live, 2.0 * bin_error_bound(name) / size.clamp_min(1e-300), torch.zeros_like(size))
    keep = live & (bound <= 0.1)
    return bound, keep, int((live & ~keep).sum())


def angular_distance(a, b):
    d = (a.double() - b.double()).abs() % (2.0 * math.pi)
    return torch.minimum(d, 2.0 * math.pi - d)
