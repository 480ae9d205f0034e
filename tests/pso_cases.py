"""Shared cases of the PSO tests (tests/test_pso_*.py, tests/golden/make_golden_pso.py): a float64 restatement of the fitness of
masks/opt_pcirm.py:146-183 (quantise with the candidate middle value, average over the channels, overlap-add the gains, STOI
fallback), a float64 restatement of optimizer/pso.py with the loop over the particles written per iteration, and the seeded
inputs.  Test-side only, numpy only.

Inputs (burst_case): fs 8000 (one case 16000, one 44100); the clean signal is three harmonics of a voiced pitch under a
syllable gate; the noise has standard deviation 0.4 in a random half of the 80-sample mask hops and 0.02 elsewhere; the PCIRM of
a loud frame is uniform in [0.005, 0.125] - inside step 2 of the default quantiser, [0.00399, 0.1302) - and uniform in [0.2, 1]
elsewhere.  The middle value then scales exactly the loud frames and the fitness is not flat (it spans 3e-2 .. 2e-1).

TOL: the golden generator asserts that every decision the reference took on the trajectory cases (fit > pbest, the argmax, >
gbest) had a margin >= MARGIN = 1e-6.  Two values whose true gap is >= 1e-6 compare the same way while each is off by < 5e-7;
TOL = MARGIN / 8 = 1.25e-7 keeps a factor 4 beyond that, and bounds restatement-vs-golden and device-vs-restatement alike."""
import math

import numpy as np

MASK_FRAME, MASK_HOP = 160, 80
MARGIN = 1e-6
TOL = MARGIN / 8
LOCAL_CRITERION_DB = -15

# name: (seed, C, L, T, fs)
INPUTS = {
    "a": (1, 64, 4000, 50, 8000),
    "b": (3, 64, 2485, 32, 8000),            # T = ceil(L / 80): the last two mask frames are cut by the signal's end
    "c": (2, 64, 1100, 14, 8000),
    "d": (4, 5, 1100, 15, 8000),             # five channels; mask frame 14 starts at 1120, past the end
    "e": (6, 64, 4000, 50, 16000),           # STOI frames of 409 samples, 205 bins
    "f": (8, 64, 4000, 50, 44100),           # STOI frames of 1128 samples, 565 bins: the fitness kernel's widest form
    "short": (7, 64, 150, 2, 8000),          # no STOI frame
    "g": (9, 5, 4097, 52, 8000),             # one sample past the split's 4096-sample chunk: two partials per sum
}
# the searches run against the reference: name -> (input, N, max_iter, np.random seed)
TRAJECTORIES = {"t1": ("a", 8, 8, 1), "t2": ("b", 8, 8, 3), "t3": ("a", 12, 10, 5), "t4": ("c", 6, 8, 2)}
# the recurrences alone, fitness -(x - t)^2 (maximise) or +(x - t)^2 (minimise): name -> (t, maximize, w, c1, c2, max_iter, seed)
RECURRENCES = {"inner": (0.3, True, 0.7, 1.5, 1.5, 12, 11), "upper": (1.4, True, 0.7, 1.5, 1.5, 12, 12),
               "lower": (-0.2, False, 0.7, 1.5, 1.5, 12, 13), "early": (0.3, True, 0.2, 0.5, 0.5, 60, 14)}
REC_N, BOUNDS = 8, (0.0, 1.0)

_cache = {}


def snr_boundaries(num_steps=3, lc_db=LOCAL_CRITERION_DB):
    lc = 10 ** (lc_db / 10.0)
    n_exp = -math.log2(lc / (lc + 1.0))
    return np.array([((m - 1) / num_steps) ** n_exp for m in range(1, num_steps + 1)], dtype=np.float64)


def burst_case(name):
    """-> dict(pcirm float32 [C, T], noisy, clean float32 [L], fs); built once per process, never modified"""
    if name in _cache:
        return _cache[name]
    seed, C, L, T, fs = INPUTS[name]
    rng = np.random.RandomState(18000 + seed)
    t = np.arange(L) / 8000.0
    f0 = 110.0 + 60.0 * rng.rand()
    voiced = sum(a * np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) for k, a in ((1, 0.30), (2, 0.20), (3, 0.12)))
    gate = (np.sin(2 * np.pi * (3.0 + 2.0 * rng.rand()) * t + rng.uniform(0, 2 * np.pi)) > -0.3).astype(np.float64)
    clean = voiced * gate
    hops = -(-L // MASK_HOP)
    loud = np.zeros(max(hops, T), dtype=bool)
    loud[rng.permutation(hops)[:hops // 2]] = True
    sigma = np.where(np.repeat(loud[:hops], MASK_HOP)[:L], 0.4, 0.02)
    noise = sigma * rng.randn(L)
    pc = np.where(loud[None, :T], rng.uniform(0.005, 0.125, (C, T)), rng.uniform(0.2, 1.0, (C, T)))
    case = {"pcirm": pc.astype(np.float32), "noisy": (clean + noise).astype(np.float32), "clean": clean.astype(np.float32), "fs": fs}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[name] = case
    return case


# ---- the fitness -------------------------------------------------------------------------------------------------------------
def quantize(pcirm, steps, middle=None):
    """masks/opt_pcirm.py:54-98 on a float32 array: compared in float64, the assigned values rounded to float32"""
    v = np.asarray(pcirm, dtype=np.float64)
    M = len(steps)
    values = np.array(steps, dtype=np.float64)
    if middle is not None and M >= 3:
        values[1] = middle
    bounds = np.concatenate([[0.0], np.asarray(steps, dtype=np.float64)[1:], [1.0]])
    out = np.zeros(v.shape, dtype=np.float32)
    for m in range(M):
        out[(v >= bounds[m]) & (v < bounds[m + 1])] = values[m]
    out[v >= bounds[-1]] = values[-1]
    return out


def stoi_fallback(clean, enhanced, fs):
    """evaluation/stoi.py:53-99 in float64"""
    clean, enhanced = np.asarray(clean, dtype=np.float64), np.asarray(enhanced, dtype=np.float64)
    frame = int(0.0256 * fs)
    hop = frame // 2
    clean = clean / (np.sqrt(np.mean(clean ** 2)) + 1e-10)
    enhanced = enhanced / (np.sqrt(np.mean(enhanced ** 2)) + 1e-10)
    n = (len(clean) - frame) // hop + 1
    if n < 1:
        return 0.0
    idx = np.arange(n)[:, None] * hop + np.arange(frame)[None, :]
    w = np.hanning(frame)
    cs = np.abs(np.fft.rfft(clean[idx] * w, axis=1))
    es = np.abs(np.fft.rfft(enhanced[idx] * w, axis=1))
    energy = np.sqrt(np.sum(cs ** 2, axis=1) + 1e-10)
    en = es / (np.sqrt(np.sum(es ** 2, axis=1)) + 1e-10)[:, None] * energy[:, None]
    corr = np.sum(cs * en, axis=1) / (np.sqrt(np.sum(cs ** 2, axis=1) * np.sum(en ** 2, axis=1)) + 1e-10)
    return float(np.clip(np.mean(np.clip(corr, -1, 1)), 0, 1))


def fitness(pcirm, noisy, clean, x, fs, steps):
    """masks/opt_pcirm.py:146-183 in float64: only the mask values are float32, as the reference's mask array holds them"""
    mask = quantize(pcirm, steps, middle=x).astype(np.float64)
    L = min(len(noisy), len(clean))
    noisy = np.asarray(noisy[:L], dtype=np.float64)
    enhanced, weights = np.zeros(L), np.zeros(L)
    for n in range(mask.shape[1]):
        start = n * MASK_HOP
        end = min(start + MASK_FRAME, L)
        if end <= start:
            continue
        enhanced[start:end] += noisy[start:end] * np.mean(mask[:, n])
        weights[start:end] += 1
    return stoi_fallback(clean[:L], enhanced / np.maximum(weights, 1), fs)


def fitness_of(name, xs, num_steps=3):
    c = burst_case(name)
    steps = snr_boundaries(num_steps)
    return np.array([fitness(c["pcirm"], c["noisy"], c["clean"], float(x), c["fs"], steps) for x in xs])


def probe_positions(seed):
    """the 82 positions of the fitness test: 40 uniform in [0, 1], 40 in [0, 0.05], 0 and 1"""
    rng = np.random.RandomState(18100 + seed)
    return np.concatenate([rng.uniform(0, 1, 40), rng.uniform(0, 0.05, 40), [0.0, 1.0]])


# ---- the swarm ---------------------------------------------------------------------------------------------------------------
def draws_after_seed(seed, N, max_iter, bounds=BOUNDS):
    """what optimizer/pso.py draws after np.random.seed(seed), in its order (a private RandomState: the same MT19937 stream)"""
    rng = np.random.RandomState(seed)
    lb, ub = bounds
    v = (ub - lb) * 0.1
    return np.concatenate([rng.uniform(lb, ub, N), rng.uniform(-v, v, N), rng.random_sample((max_iter, N, 2)).reshape(-1)])


def pso(fitness_fn, draws, N, max_iter, w=0.7, c1=1.5, c2=1.5, bounds=BOUNDS, maximize=True):
    """optimizer/pso.py:81-181 in float64 with the inner loop vectorised over the particles (they do not see each other inside
    an iteration).  fitness_fn(positions [N], round) -> [N].  Returns a dict: the three history lists, 'positions' / 'fitness'
    [rounds, N], 'margins' [rounds] (the smallest gap any decision of the round had, ties of one position excluded),
    'iterations_run', 'best_position', 'best_fitness'."""
    lb, ub = bounds
    draws = np.asarray(draws, dtype=np.float64)
    pos, vel = draws[:N].copy(), draws[N:2 * N].copy()
    r = draws[2 * N:].reshape(max_iter, N, 2)
    better = (lambda a, b: a > b) if maximize else (lambda a, b: a < b)
    arg = np.argmax if maximize else np.argmin

    def top_margin(values, positions, best):
        other = positions != positions[best]
        return float(np.min(np.abs(values[other] - values[best]))) if other.any() else np.inf

    fit = np.asarray(fitness_fn(pos, 0), dtype=np.float64)
    pbp, pbf = pos.copy(), fit.copy()
    g = int(arg(fit))
    gp, gf = pos[g], fit[g]
    H = {"gbest_fitness": [gf], "gbest_position": [gp], "mean_fitness": [np.mean(fit)], "positions": [pos.copy()],
         "fitness": [fit.copy()], "margins": [top_margin(fit, pos, g)]}
    it = 0
    for it in range(1, max_iter + 1):
        cognitive = c1 * r[it - 1, :, 0] * (pbp - pos)
        social = c2 * r[it - 1, :, 1] * (gp - pos)
        vel = w * vel + cognitive + social
        max_v = (ub - lb) * 0.5
        vel = np.clip(vel, -max_v, max_v)
        pos = pos + vel
        low, high = pos < lb, pos > ub
        vel = np.where(low, np.abs(vel) * 0.5, np.where(high, -np.abs(vel) * 0.5, vel))
        pos = np.where(low, lb, np.where(high, ub, pos))
        fit = np.asarray(fitness_fn(pos, it), dtype=np.float64)
        moved = pos != pbp
        margin = float(np.min(np.abs(fit - pbf)[moved])) if moved.any() else np.inf
        up = better(fit, pbf)
        pbf, pbp = np.where(up, fit, pbf), np.where(up, pos, pbp)
        best = int(arg(pbf))
        margin = min(margin, top_margin(pbf, pbp, best))
        if pbp[best] != gp:
            margin = min(margin, abs(float(pbf[best] - gf)))
        if better(pbf[best], gf):
            gf, gp = pbf[best], pbp[best]
        for k, v in (("gbest_fitness", gf), ("gbest_position", gp), ("mean_fitness", np.mean(fit)), ("positions", pos.copy()),
                     ("fitness", fit.copy()), ("margins", margin)):
            H[k].append(v)
        if np.std(pos) < 1e-6:
            break
    H.update(iterations_run=it, best_position=float(gp), best_fitness=float(gf))
    for k in ("gbest_fitness", "gbest_position", "mean_fitness", "positions", "fitness", "margins"):
        H[k] = np.asarray(H[k], dtype=np.float64)
    return H


def quadratic(t, maximize):
    """the fitness of the recurrence cases, written as a product (bit-identical in numpy and in float64 torch ops)"""
    return (lambda x: -((x - t) * (x - t))) if maximize else (lambda x: (x - t) * (x - t))
