"""Shared cases of the curriculum-batch tests (tests/test_masks_*.py, tests/golden/make_golden_masks.py): a restatement of the
mask targets (IRM, correlation coefficients, PCIRM, the fixed-step quantiser), of the SNR mix and of the STFT around them in
torch, computing in the dtype of its inputs (float64: the reference of the GPU rows; float32: the row's e32), and the seeded
cases.  Test-side only.

Utterances (UTTERANCES): clean speech 0.1 N(0, 1) with 400 exact zeros in the middle (three all-zero STFT frames), noise
0.3 N(0, 1): a noise tiled with more than three wraps, a noise longer than the utterance, a length that is no multiple of
the hop, an SNR on either side of 0 dB.  Random planes (RANDOM): two shapes with an odd last dimension, so a flat range has a
scalar tail behind its 16-byte accesses; phases include exact +-pi, magnitudes exact zeros; the quantiser's input holds exactly
0, 1, the fp32 neighbours of step_values[1], a NaN and a negative value."""
import math

import numpy as np
import torch

FFT, HOP, WIN = 256, 80, 160
EPS = 1e-10
LOCAL_CRITERION_DB, NUM_STEPS = -15, 3
MIDDLE_VALUE = 0.05
# (L, noise length, SNR dB, seed)
UTTERANCES = ((1700, 450, 5.0, 171), (2403, 5000, -5.0, 172), (800, 800, 10.0, 173))
SILENT_FRAMES = ((10, 13), (14, 17), (4, 7))            # [first, last) all-zero frames of each clean utterance
RANDOM = {"r1": ((3, 21, 129), 174), "r2": ((2, 5, 257), 175)}
U32 = 2.0 ** -24
K = 16.0                                                # masks sit behind a sqrt and a division

_cache = {}


# ---- the formulas, in the dtype of their arguments ----
def irm(clean_mag, noise_mag, p=0.5, eps=EPS):
    cp, npow = clean_mag.abs() ** 2, noise_mag.abs() ** 2
    return ((cp / (cp + npow + eps)) ** p).clamp(0.0, 1.0)


def corr(noisy, clean, noise, eps=EPS):
    """the per-T-F-unit rule at every element -> (rho_s, rho_n)"""
    def rho(a, b):
        return ((a * b) / (torch.sqrt(a ** 2 + eps) * torch.sqrt(b ** 2 + eps))).abs().clamp(0.0, 1.0)
    return rho(noisy, clean), rho(noisy, noise)


def pcirm(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2, eps=EPS):
    s = rho_s * (clean_mag.abs() * torch.cos(phi1).abs()) ** 2
    n = rho_n * (noise_mag.abs() * torch.cos(phi2).abs()) ** 2
    return (s / (s + n + eps)).clamp(0.0, 1.0)


def snr_boundaries(lc_db=LOCAL_CRITERION_DB, num_steps=NUM_STEPS):
    lc = 10 ** (lc_db / 10.0)
    n_exp = -math.log2(lc / (lc + 1.0))
    return np.array([((m - 1) / num_steps) ** n_exp for m in range(1, num_steps + 1)], dtype=np.float64), n_exp


def quantize(x, steps, middle=None):
    """x: tensor; compared in float64 with the boundaries [0, s_2 .. s_M, 1]; the assigned values rounded to x's dtype"""
    v = x.detach().double().cpu().numpy()
    M = len(steps)
    values = np.array(steps, dtype=np.float64)
    if middle is not None and M >= 3:
        values[1] = middle
    bounds = np.concatenate([[0.0], np.asarray(steps, dtype=np.float64)[1:], [1.0]])
    out = np.zeros_like(v)
    with np.errstate(invalid="ignore"):
        for m in range(M):
            out[(v >= bounds[m]) & (v < bounds[m + 1])] = values[m]
        out[v >= bounds[-1]] = values[-1]
    return torch.from_numpy(out).to(x.dtype)


def spectral_masks(C, sN, Y, p=0.5):
    """complex spectra of the clean utterance, the scaled noise and the mix -> dict(irm, pcirm) through magnitudes and angles
    (a zero has angle 0)"""
    cm, nm, ym = C.abs(), sN.abs(), Y.abs()
    rho_s, rho_n = corr(ym, cm, nm)
    ay = torch.angle(Y)
    return {"irm": irm(cm, nm, p), "pcirm": pcirm(cm, nm, rho_s, rho_n, torch.angle(C) - ay, torch.angle(sN) - ay)}


def mix(clean, noise, snr_db, length=None):
    """1-D clean [L] and noise of one dtype -> (noisy [L], scale, the tiled / cut noise [L]); samples from `length` on are 0"""
    L = clean.numel()
    n = L if length is None else length
    reps = -(-n // noise.numel())
    tiled = torch.zeros_like(clean)
    tiled[:n] = noise.repeat(reps)[:n]
    pc = (clean[:n] ** 2).mean() + 1e-10
    pn = (tiled[:n] ** 2).mean() + 1e-10
    scale = torch.sqrt(pc / (pn * 10 ** (snr_db / 10.0)))
    noisy = torch.zeros_like(clean)
    noisy[:n] = clean[:n] + scale * tiled[:n]
    return noisy, scale, tiled


def stft(wave):
    """[B, L] -> complex [B, T, F], T = 1 + L // HOP (periodic Hann window of WIN samples, centred, reflect padding)"""
    w = torch.hann_window(WIN, dtype=wave.dtype)
    return torch.stft(wave, n_fft=FFT, hop_length=HOP, win_length=WIN, window=w, return_complex=True).transpose(1, 2)


# ---- the cases ----
def utterance(k):
    """(clean [L], noise [Ln]) float32 tensors of UTTERANCES[k], from its seed alone.  Cached and shared: do not modify."""
    key = ("utt", k)
    if key not in _cache:
        L, Ln, _, seed = UTTERANCES[k]
        rng = np.random.RandomState(seed)
        clean = (0.1 * rng.standard_normal(L)).astype(np.float32)
        a = (L - 400) // 2
        clean[a:a + 400] = 0.0
        noise = (0.3 * rng.standard_normal(Ln)).astype(np.float32)
        _cache[key] = (torch.from_numpy(clean), torch.from_numpy(noise))
    return _cache[key]


def utterance_reference(k, dtype):
    """UTTERANCES[k] alone (not padded) in `dtype`: dict(noisy [L], scale, C, sN, Y [T, F] complex, irm, pcirm [T, F])"""
    key = ("uref", k, dtype)
    if key not in _cache:
        clean, noise = (t.to(dtype) for t in utterance(k))
        noisy, scale, tiled = mix(clean, noise, UTTERANCES[k][2])
        C, sN, Y = (stft(x.unsqueeze(0))[0] for x in (clean, scale * tiled, noisy))
        out = {"noisy": noisy, "scale": scale, "C": C, "sN": sN, "Y": Y}
        out.update(spectral_masks(C, sN, Y))
        _cache[key] = out
    return _cache[key]


def padded_batch():
    """the three utterances as one zero-padded batch: clean [3, 2403] float32, the noise list, SNRs, lengths"""
    Lmax = max(u[0] for u in UTTERANCES)
    clean = torch.zeros(len(UTTERANCES), Lmax)
    for k, u in enumerate(UTTERANCES):
        clean[k, :u[0]] = utterance(k)[0]
    return clean, [utterance(k)[1] for k in range(len(UTTERANCES))], [u[2] for u in UTTERANCES], [u[0] for u in UTTERANCES]


def batch_reference(dtype, p=0.5):
    """the padded batch in `dtype`: dict(noisy [B, L], scale [B], C, Y [B, T, F] complex, irm, pcirm [B, T, F])"""
    key = ("bref", dtype, p)
    if key not in _cache:
        clean, noises, snrs, lengths = padded_batch()
        rows = [mix(clean[k].to(dtype), noises[k].to(dtype), snrs[k], lengths[k]) for k in range(clean.shape[0])]
        noisy = torch.stack([r[0] for r in rows])
        scale = torch.stack([r[1] for r in rows])
        scaled = torch.stack([r[1] * r[2] for r in rows])
        C, sN, Y = stft(clean.to(dtype)), stft(scaled), stft(noisy)
        out = {"noisy": noisy, "scale": scale, "C": C, "Y": Y}
        out.update(spectral_masks(C, sN, Y, p))
        _cache[key] = out
    return _cache[key]


def random_case(name):
    """float32 planes of RANDOM[name]: cm, nm, ym (magnitudes, a few exact zeros), py, pc, pn (phases in [-pi, pi], a few at
    exactly +-pi), rho_s, rho_n (the float32 restatement's, the inputs of the PCIRM row), q (the quantiser's input)"""
    key = ("rand", name)
    if key not in _cache:
        shape, seed = RANDOM[name]
        rng = np.random.RandomState(seed)
        c = {}
        for m in ("cm", "nm", "ym"):
            a = rng.uniform(0.0, 1.0, shape).astype(np.float32)
            a.reshape(-1)[rng.choice(a.size, 7, replace=False)] = 0.0
            c[m] = torch.from_numpy(a)
        for ph in ("py", "pc", "pn"):
            a = rng.uniform(-np.pi, np.pi, shape).astype(np.float32)
            flat = a.reshape(-1)
            flat[rng.choice(a.size, 6, replace=False)] = np.float32(np.pi)
            flat[rng.choice(a.size, 6, replace=False)] = -np.float32(np.pi)
            c[ph] = torch.from_numpy(a)
        c["rho_s"], c["rho_n"] = corr(c["ym"], c["cm"], c["nm"])
        q = (rng.uniform(0.0, 1.0, shape) ** 3).astype(np.float32)          # a third of the values below the upper boundary
        s1 = np.float32(snr_boundaries()[0][1])
        planted = [0.0, 1.0, s1, np.nextafter(s1, np.float32(0)), np.nextafter(s1, np.float32(1)), np.nan, -0.25,
                   np.float32(snr_boundaries()[0][2]), 1.5]
        q.reshape(-1)[rng.choice(q.size, len(planted), replace=False)] = np.array(planted, dtype=np.float32)
        c["q"] = torch.from_numpy(q)
        _cache[key] = c
    return _cache[key]


def random_reference(name, dtype):
    """dict(irm, irm_p (p = 0.3), rho_s, rho_n, pcirm) of a random case evaluated in `dtype` from its float32 planes"""
    key = ("rref", name, dtype)
    if key not in _cache:
        c = {k: v.to(dtype) for k, v in random_case(name).items()}
        rho_s, rho_n = corr(c["ym"], c["cm"], c["nm"])
        _cache[key] = {"irm": irm(c["cm"], c["nm"]), "irm_p": irm(c["cm"], c["nm"], p=0.3), "rho_s": rho_s, "rho_n": rho_n,
                       "pcirm": pcirm(c["cm"], c["nm"], c["rho_s"], c["rho_n"], c["pc"] - c["py"], c["pn"] - c["py"])}
    return _cache[key]


# ---- bounds ----
def abs_bound(ref32, ref64, peak=1.0):
    """(e32, bound): e32 = max |float32 evaluation - float64 one|; bound = max(16 e32, 16 x 2^-24 x peak)"""
    e32 = float((ref32.double() - ref64.double()).abs().max())
    return e32, max(K * e32, K * U32 * peak)


def check(name, got, ref64, ref32, peak=1.0):
    """print `ROW | name | e32 | bound | observed`, assert max |got - ref64| <= bound and return the bound"""
    e32, bound = abs_bound(ref32, ref64, peak)
    obs = float((torch.as_tensor(got).detach().cpu().double() - ref64.double()).abs().max())
    print("ROW | %s | e32 %.2e | bound %.2e | observed %.2e" % (name, e32, bound, obs))
    assert math.isfinite(obs) and obs <= bound, (name, obs, bound)
    return bound


def near_boundary(pcirm64, steps, margin):
    """bool mask: the float64 PCIRM lies within `margin` of one of the quantiser's inner boundaries s_2 .. s_M"""
    near = torch.zeros_like(pcirm64, dtype=torch.bool)
    for s in steps[1:]:
        near |= (pcirm64 - float(s)).abs() <= margin
    return near


def adjacent_values(pcirm64, steps, values):
    """for every element the two step values on either side of the inner boundary nearest to it: (lower, upper)"""
    inner = torch.tensor(steps[1:], dtype=torch.float64)
    m = (pcirm64.unsqueeze(-1) - inner).abs().argmin(dim=-1)              # nearest inner boundary = boundary m + 1
    v = torch.tensor(values, dtype=torch.float64)
    return v[m], v[m + 1]
