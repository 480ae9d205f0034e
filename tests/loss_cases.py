"""Shared cases of the curriculum-objective tests (tests/test_losses_*.py, tests/golden/make_golden_losses.py): a restatement
of PerceptualSTOILoss and MSEMaskLoss in torch that computes in the dtype of its inputs (float64: the reference of the GPU
rows; float32: the row's e32) and takes the band matrix as an argument, plausible wrong forms of it for the CPU mutant
checks, and the seeded cases.  Test-side only.

A case is built from its seed alone: magnitudes [B, F, T] of a clean and an enhanced spectrogram and two phase arrays, so
that the channels-last pair form (real, imag [B, T, F]) has the same magnitudes up to rounding.  `loud` segments carry an
enhanced side ~12 x the clean one in envelope energy (beyond the 15 dB clip, ratio ~0.47), `flat` segments a clean side that
is constant in time (its energy is the sqrt(1e-8) floor, so the clip is certain), `quiet` segments a clean side 3e-4 x
the usual one: its envelope energy is of the order of the 1e-8 under the roots, and only there does the clip change the value
(a correlation does not see the scale of its arguments: without the 1e-8s the clip would cancel)."""
import numpy as np
import torch

FRAME_LEN, BETA_DB = 30, 15.0
CENTRES = (150, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150)
TIE_MARGIN = 0.05                       # min |ratio - 1| every case keeps: torch.min has no gradient at a tie
MUTANTS = ("no clip", "clip without the 1e-8s", "mean over the wrong axis", "tail frames included")


def band_matrix(sample_rate, n_freq=129, centres=CENTRES):
    """normalised indicator rows of the 1/3-octave bands over n_freq bins from 0 to sample_rate / 2, float32"""
    freqs = np.linspace(0, sample_rate / 2, n_freq)
    w = np.zeros((len(centres), n_freq), dtype=np.float32)
    for i, cf in enumerate(centres):
        w[i, (freqs >= cf / 2 ** (1 / 6)) & (freqs <= cf * 2 ** (1 / 6))] = 1.0
    s = w.sum(axis=1, keepdims=True)
    s[s == 0] = 1.0
    return w / s


def overlap_matrix(n_freq=257, nb=14):
    """a replaced matrix: nb bands of 20 bins, each sharing its last two bins with the next band; unequal weights in a row"""
    w = np.zeros((nb, n_freq), dtype=np.float32)
    for i in range(nb):
        lo = 3 + 18 * i
        w[i, lo:lo + 20] = np.linspace(1.0, 2.0, 20, dtype=np.float32)
    return w / w.sum(axis=1, keepdims=True)


# name -> (B, T, F, band matrix, seed, loud (b, s), flat (b, s), zero, quiet (b, s))
CASES = {
    "c1_one_segment": (1, 30, 129, 8000, 151, (), (), False),
    "c2_tail_loud_flat": (2, 61, 129, 8000, 152, ((0, 1),), ((1, 1),), False),
    "c3_five_tail_frames": (3, 95, 129, 8000, 153, ((0, 2),), (), False, ((2, 0),)),
    "c4_empty_band_16k": (1, 30, 129, 16000, 154, (), (), False),
    "c5_overlapping_bands": (2, 60, 257, "overlap", 155, ((1, 0),), (), False),
    "c6_all_zero": (2, 61, 129, 8000, 152, (), (), True),
    "c7_many_partials": (64, 120, 129, 8000, 157, tuple((b, s) for b in range(64) for s in range(4) if (b + s) % 3 == 0), (),
                        False),
}
FIXTURE_CASES = ("c1_one_segment", "c2_tail_loud_flat", "c3_five_tail_frames", "c4_empty_band_16k", "c6_all_zero", "c7_many_partials")
# the fixture keeps the whole gradient, except for c7 (4 MB): there the last utterance's
FIXTURE_GRAD_ROWS = {"c7_many_partials": slice(63, 64)}
# expected (clipped pairs, all pairs) of each case: asserted by the CPU test from the restatement
CLIPPED = {"c1_one_segment": (0, 14), "c2_tail_loud_flat": (28, 56), "c3_five_tail_frames": (28, 126), "c4_empty_band_16k": (0, 14),
           "c5_overlapping_bands": (14, 56), "c6_all_zero": (0, 56), "c7_many_partials": (14 * 86, 14 * 256)}

_cache = {}


def weights(name):
    m = CASES[name][3]
    return torch.from_numpy(overlap_matrix() if m == "overlap" else band_matrix(m, CASES[name][2]))


def case(name):
    """dict(enh, clean: float32 magnitudes [B, F, T]; ph_e, ph_c: float32 phases [B, F, T]; w: band matrix).  Cached and shared:
    do not modify."""
    if name in _cache:
        return _cache[name]
    B, T, F, _, seed, loud, flat, zero = CASES[name][:8]
    quiet = CASES[name][8] if len(CASES[name]) > 8 else ()
    rng = np.random.RandomState(seed)
    clean = rng.uniform(0.05, 1.0, (B, F, T))
    enh = clean * rng.uniform(0.6, 1.1, (B, F, T)) + rng.uniform(0.0, 0.2, (B, F, T))
    wild = rng.uniform(0.05, 1.0, (B, F, T))
    ph_e, ph_c = rng.uniform(-np.pi, np.pi, (B, F, T)), rng.uniform(-np.pi, np.pi, (B, F, T))
    for b, s in loud:
        seg = slice(s * FRAME_LEN, (s + 1) * FRAME_LEN)
        enh[b, :, seg] = 12.0 * wild[b, :, seg]
    for b, s in flat:
        seg = slice(s * FRAME_LEN, (s + 1) * FRAME_LEN)
        clean[b, :, seg] = clean[b, :, s * FRAME_LEN:s * FRAME_LEN + 1]
        ph_c[b, :, seg] = ph_c[b, :, s * FRAME_LEN:s * FRAME_LEN + 1]           # (real, imag) constant as well: flat to the bit
    for b, s in quiet:
        clean[b, :, s * FRAME_LEN:(s + 1) * FRAME_LEN] *= 3e-4
    if zero:
        clean[:], enh[:] = 0.0, 0.0
    c = {"enh": torch.from_numpy(enh.astype(np.float32)), "clean": torch.from_numpy(clean.astype(np.float32)),
         "ph_e": torch.from_numpy(ph_e.astype(np.float32)), "ph_c": torch.from_numpy(ph_c.astype(np.float32)),
         "w": weights(name)}
    _cache[name] = c
    return c


def pairs(c):
    """channels-last (real, imag) pairs [B, T, F] float32 whose magnitudes are the case's: er, ei, cr, ci"""
    out = []
    for m, p in ((c["enh"], c["ph_e"]), (c["clean"], c["ph_c"])):
        out += [(m * torch.cos(p)).transpose(1, 2).contiguous(), (m * torch.sin(p)).transpose(1, 2).contiguous()]
    return out


def magnitude(re, im):
    return torch.sqrt(re * re + im * im + 1e-8)


def pstoi(enh, clean, w, frame_len=FRAME_LEN, beta=BETA_DB, mutant=None, info=None):
    """enh, clean [B, F, T], w [NB, F], all of one dtype -> scalar loss in that dtype.  info (a dict): gets `ratio`, the clip
    ratio of every (batch, band, segment)."""
    eps = 0.0 if mutant == "clip without the 1e-8s" else 1e-8
    env_c, env_e = torch.matmul(w.unsqueeze(0), clean), torch.matmul(w.unsqueeze(0), enh)
    B, NB, T = env_c.shape
    S = max(1, T // frame_len)
    first = T - S * frame_len if mutant == "tail frames included" else 0
    seg_c = env_c[..., first:first + S * frame_len].reshape(B, NB, S, frame_len)
    seg_e = env_e[..., first:first + S * frame_len].reshape(B, NB, S, frame_len)
    axis = 1 if mutant == "mean over the wrong axis" else -1
    seg_c = seg_c - seg_c.mean(dim=axis, keepdim=True)
    seg_e = seg_e - seg_e.mean(dim=axis, keepdim=True)
    en_c = torch.sqrt(torch.sum(seg_c ** 2, dim=-1, keepdim=True) + eps)
    en_e = torch.sqrt(torch.sum(seg_e ** 2, dim=-1, keepdim=True) + eps)
    ratio = 10 ** (beta / 20.0) * en_c / (en_e + eps)
    if info is not None:
        info["ratio"] = ratio.detach().squeeze(-1)
    scale = torch.ones_like(ratio) if mutant == "no clip" else torch.min(torch.ones_like(ratio), ratio)
    clipped = seg_e * scale
    num = torch.sum(seg_c * clipped, dim=-1)
    den = torch.sqrt(torch.sum(seg_c ** 2, dim=-1) + eps) * torch.sqrt(torch.sum(clipped ** 2, dim=-1) + eps)
    return -(num / (den + eps)).mean()


def mse(p, t):
    return ((p - t) ** 2).mean()


def clip_report(name):
    """(clipped pairs, all pairs, min |ratio - 1|) of a case, from the float64 restatement"""
    c, info = case(name), {}
    pstoi(c["enh"].double(), c["clean"].double(), c["w"].double(), info=info)
    r = info["ratio"]
    return int((r < 1).sum()), r.numel(), float((r - 1).abs().min())


def reference(name, form, dtype, mutant=None):
    """(loss, gradient) of a case in `dtype` on the CPU.  form 0: gradient to the enhanced magnitudes [B, F, T]; form 1: the
    magnitudes are taken from the channels-last pairs and the gradient is (d real, d imag) stacked [2, B, T, F]."""
    key = (name, form, dtype, mutant)
    if key in _cache:
        return _cache[key]
    c = case(name)
    w = c["w"].to(dtype)
    if form == 0:
        e = c["enh"].to(dtype).clone().requires_grad_(True)
        loss = pstoi(e, c["clean"].to(dtype), w, mutant=mutant)
        loss.backward()
        out = (loss.detach(), e.grad)
    else:
        er, ei, cr, ci = (t.to(dtype).clone() for t in pairs(c))
        er.requires_grad_(True), ei.requires_grad_(True)
        loss = pstoi(magnitude(er, ei).transpose(1, 2), magnitude(cr, ci).transpose(1, 2), w, mutant=mutant)
        loss.backward()
        out = (loss.detach(), torch.stack([er.grad, ei.grad]))
    _cache[key] = out
    return out


def mse_case(shape, seed):
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.uniform(0.0, 1.0, shape).astype(np.float32)),
            torch.from_numpy(rng.uniform(0.0, 1.0, shape).astype(np.float32)))
