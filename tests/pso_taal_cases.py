"""Shared cases of the tests of the OPT-PCIRM search on the Taal measures (tests/test_pso_taal_*.py): the planes route restated in
numpy with OPERANDS in a chosen dtype and every sum in float64, the inputs, the searches and the mutants.  Test-side only, numpy
only; it rests on stoi_taal_cases (the measure) and pso_cases (inputs, quantiser, swarm).

The route.  The candidate x gives the enhanced signal ya + x yb (pso_cases.fitness: quantise with the middle value x, average over
the channels, overlap-add the gains).  The resampler, the kept-frame list (the CLEAN signal's), the overlap-add rebuild and the
windowed DFT are linear in it, so spectral frame m is A_m + x B_m and the energy of band j is
    E(x) = P + 2 x Q + x^2 R,   P = sum_k |A_k|^2,  Q = sum_k Re(A_k conj B_k),  R = sum_k |B_k|^2   over the band's bins;
the enhanced band rows are sqrt(max(E(x), 0)) and the segments are stoi_taal_cases.stoi64's.  x is float32(x) as a float64: the
mask array that carries the middle value is float32.

  float64 operands: the reference of the GPU rows.
  float32 operands (ya, yb, the clean signal, the taps, the window, the DFT matrix, the resampled samples, the clean band rows;
  the planes stay float64, as on the device): e32 = |that value - the float64 value|.
A GPU value passes within K = 16 x (the largest e32 over the positions it is probed at), per case and measure; the bound never
comes from a kernel.

Inputs: pso_cases.burst_case at sizes whose utterances keep 30 .. 110 frames (the inputs of pso_cases keep 24-26 and would score a
flat 1e-5).  evaluated() asserts the table below, that every frame lies at least 1 dB from the 40 dB threshold, that the STOI clip
branch runs wherever there is a segment and that the float64 fitness spans more than 1e-2 over the probes."""
import numpy as np

import pso_cases as pc
import stoi_taal_cases as stc

K = stc.K
MEASURES = (False, True)                                     # extended
# name: (seed, C, L, T, fs) as pso_cases.INPUTS, and what the float64 evaluation must show: (frames, kept, segments)
INPUTS = {
    "A": (1, 64, 8000, 100, 8000),           # 48 spectral frames = exactly three 16-row tiles
    "B": (3, 64, 6085, 77, 8000),            # odd length, partial last tile, the last mask frames cut by the signal's end
    "C": (4, 5, 12000, 150, 16000),          # 8 -> 5 resampling, five channels
    "D": (2, 64, 9000, 113, 10000),          # no resampler
    "E": (1, 64, 4733, 60, 8000),            # exactly one segment
    "F": (1, 64, 4622, 58, 8000),            # 29 spectral frames: 1e-5 exactly, every particle
    "G": (5, 64, 16000, 200, 8000),          # three stages of the 32-segment ring
}
EXPECTED = {"A": (77, 49, 19), "B": (58, 40, 10), "C": (57, 42, 12), "D": (69, 47, 17), "E": (45, 31, 1), "F": (44, 30, 0),
            "G": (155, 110, 80)}
SCORED = ("A", "B", "C", "D", "E", "G")
# the searches: name -> (input, N, max_iter, seed of pso_cases.draws_after_seed, extended).  A's ESTOI searches are left out on
# purpose: their smallest decision margins (3.3e-7, 6.6e-7) do not reach twice their bound (3.7e-7).
TRAJECTORIES = {"A8": ("A", 8, 8, 1, False), "B8": ("B", 8, 8, 3, False), "B8e": ("B", 8, 8, 3, True), "C6": ("C", 6, 8, 2, False),
                "C6e": ("C", 6, 8, 2, True), "A12": ("A", 12, 10, 5, False)}
MUTANTS = ("Q dropped", "Q with the imaginary product's sign flipped", "kept list from ya", "x^2 replaced by x")
for _k, _v in INPUTS.items():
    pc.INPUTS.setdefault("taal" + _k, _v)    # burst_case reads its sizes there

_cache = {}


def case(name):
    """pso_cases.burst_case(name): dict(pcirm float32 [C, T], noisy, clean float32 [L], fs); shared, never modified"""
    return pc.burst_case("taal" + name)


def f32(x):
    """the middle value as the float32 mask array holds it"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def split(name, num_steps=3):
    """(ya, yb) float64 [L]: pso_cases.fitness's enhanced signal for the middle value x is ya + float32(x) yb (num_steps < 3: the
    middle value is unused and yb = 0)"""
    key = ("split", name, num_steps)
    if key not in _cache:
        c = case(name)
        steps = pc.snr_boundaries(num_steps)
        q0 = pc.quantize(c["pcirm"], steps, middle=0.0).astype(np.float64)
        q1 = pc.quantize(c["pcirm"], steps, middle=1.0).astype(np.float64)
        a, b = np.mean(q0, axis=0), np.mean(q1 - q0, axis=0)
        L = min(len(c["noisy"]), len(c["clean"]))
        noisy = np.asarray(c["noisy"][:L], dtype=np.float64)
        ya, yb, weights = np.zeros(L), np.zeros(L), np.zeros(L)
        for n in range(a.size):
            start = n * pc.MASK_HOP
            end = min(start + pc.MASK_FRAME, L)
            if end <= start:
                continue
            ya[start:end] += noisy[start:end] * a[n]
            yb[start:end] += noisy[start:end] * b[n]
            weights[start:end] += 1
        w = np.maximum(weights, 1)
        _cache[key] = (ya / w, yb / w)
    return _cache[key]


def enhanced(name, x, num_steps=3):
    """float32 [L]: the enhanced signal of pso_cases.fitness for the middle value x, as that function forms it"""
    c = case(name)
    mask = pc.quantize(c["pcirm"], pc.snr_boundaries(num_steps), middle=x).astype(np.float64)
    L = min(len(c["noisy"]), len(c["clean"]))
    noisy = np.asarray(c["noisy"][:L], dtype=np.float64)
    e, weights = np.zeros(L), np.zeros(L)
    for n in range(mask.shape[1]):
        start = n * pc.MASK_HOP
        end = min(start + pc.MASK_FRAME, L)
        if end <= start:
            continue
        e[start:end] += noisy[start:end] * np.mean(mask[:, n])
        weights[start:end] += 1
    return (e / np.maximum(weights, 1)).astype(np.float32)


# ---- the planes route ----
def planes(clean, ya, yb, fs, dtype=np.float64, mutant=None, info=None):
    """steps 0-3 once per search -> (xt, P, Q, R): the clean band rows [15, M] held in `dtype` and the float64 planes [15, M] of the
    band energies of ya + x yb; None where there is no frame at all.  info receives frames, kept, margin (dB)."""
    _as = stc._as
    x, ra, rb = (stc.resample(s, fs, dtype) for s in (clean, ya, yb))
    w = _as(np.hanning(stc.NF + 2)[1:-1], dtype)
    starts = list(range(0, x.size - stc.NF + 1, stc.HOP))
    if info is not None:
        info.update(frames=len(starts), kept=0, margin=float("inf"))
    if not starts:
        return None
    framed = [np.array([w * s[i:i + stc.NF] for i in starts]) for s in (x, ra, rb)]
    decide = framed[1] if mutant == "kept list from ya" else framed[0]
    e = 20.0 * np.log10(np.linalg.norm(decide, axis=1) + stc.EPS)
    mask = (np.max(e) - stc.DYN - e) < 0
    if info is not None:
        info.update(kept=int(mask.sum()), margin=float(np.min(np.abs(np.max(e) - stc.DYN - e))))
    kept = int(mask.sum())
    rebuilt = []
    for f in framed:
        f = f[mask]
        s = np.zeros((kept - 1) * stc.HOP + stc.NF)
        for i in range(kept):
            s[i * stc.HOP:i * stc.HOP + stc.NF] += f[i]
        rebuilt.append(s)
    stop = rebuilt[0].size - stc.NF
    ang = 2.0 * np.pi * ((np.arange(stc.NF)[:, None] * np.arange(stc.NFFT // 2 + 1)[None, :]) % stc.NFFT) / stc.NFFT
    C, S = _as(np.cos(ang), dtype), _as(-np.sin(ang), dtype)
    fr = [np.array([w * s[i:i + stc.NF] for i in range(0, stop, stc.HOP)]).reshape(-1, stc.NF) for s in rebuilt]
    (cr, ci), (ar, ai), (br, bi) = ((f @ C, f @ S) for f in fr)
    tab = stc.band_table()

    def band(p):
        return np.stack([p[:, lo:hi].sum(1) for lo, hi in tab])
    xt = _as(np.sqrt(band(cr ** 2 + ci ** 2)), dtype)
    if mutant == "Q dropped":
        Q = np.zeros_like(xt)
    elif mutant == "Q with the imaginary product's sign flipped":
        Q = band(ar * br - ai * bi)
    else:
        Q = band(ar * br + ai * bi)
    return xt, band(ar ** 2 + ai ** 2), Q, band(br ** 2 + bi ** 2)


def segments(xt, yt, extended, info=None):
    """steps 4 and 5 of stoi_taal_cases.stoi64 on band rows [15, M] (float64 arithmetic)"""
    M, SEG, EPS = xt.shape[1], stc.SEG, stc.EPS
    if M < SEG:
        return 1e-5
    xg = np.array([xt[:, m - SEG:m] for m in range(SEG, M + 1)])
    yg = np.array([yt[:, m - SEG:m] for m in range(SEG, M + 1)])
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
        info["clipped"] = min(info.get("clipped", 1.0), float(np.mean(yn > lim)))
    yp = np.minimum(yn, lim)
    yp = yp - yp.mean(2, keepdims=True)
    xz = xg - xg.mean(2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xz = xz / (np.linalg.norm(xz, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xz) / (xg.shape[0] * xg.shape[1]))


def at(pl, x, extended, mutant=None, info=None):
    """the fitness at the middle value x from planes()'s result"""
    if pl is None:
        return 1e-5
    xt, P, Q, R = pl
    x = float(f32(x))
    E = P + 2.0 * x * Q + (x if mutant == "x^2 replaced by x" else x * x) * R
    return segments(xt, np.sqrt(np.maximum(E, 0.0)), extended, info)


def case_planes(name, dtype=np.float64, num_steps=3, mutant=None, info=None):
    """planes() of an input, computed once per (input, dtype, steps, mutant) and shared"""
    key = ("planes", name, np.dtype(dtype).name, num_steps, mutant)
    if key not in _cache:
        c = case(name)
        ya, yb = split(name, num_steps)
        inf = {}
        _cache[key] = (planes(c["clean"][:ya.size], ya, yb, c["fs"], dtype, mutant, inf), inf)
    if info is not None:
        info.update(_cache[key][1])
    return _cache[key][0]


def fitness_of(name, xs, extended, dtype=np.float64, num_steps=3, mutant=None, info=None):
    """[len(xs)] float64: the planes route at each x with operands in `dtype`"""
    pl = case_planes(name, dtype, num_steps, None if mutant == "x^2 replaced by x" else mutant, info)
    return np.array([at(pl, x, extended, mutant, info) for x in np.asarray(xs, dtype=np.float64).reshape(-1)])


def direct(name, x, extended, dtype=np.float64, num_steps=3, info=None):
    """stoi_taal_cases.stoi64(clean, ya + float32(x) yb): the measure itself on the float64 signals"""
    c = case(name)
    ya, yb = split(name, num_steps)
    return stc.stoi64(c["clean"][:ya.size], ya + float(f32(x)) * yb, c["fs"], extended, dtype, info=info)


def probes(name):
    return pc.probe_positions(INPUTS[name][0])


def bound_at(name, xs, extended, num_steps=3):
    """(ref float64 [n], e32 [n]): the float64 fitness at xs and the distance of the float32-operand evaluation from it"""
    ref = fitness_of(name, xs, extended, np.float64, num_steps)
    return ref, np.abs(fitness_of(name, xs, extended, np.float32, num_steps) - ref)


def evaluated():
    """{(name, extended): dict(xs, ref [82], e32, bound, info)} at the probe positions of every input, computed once and shared
    (do not modify); asserts the generator's conditions"""
    if "rows" not in _cache:
        rows = {}
        for name in INPUTS:
            xs = probes(name)
            for ext in MEASURES:
                info = {}
                ref = fitness_of(name, xs, ext, np.float64, info=info)
                e32 = float(np.abs(fitness_of(name, xs, ext, np.float32) - ref).max())
                info["segments"] = max(info["kept"] - 1 - stc.SEG + 1, 0)
                assert (info["frames"], info["kept"], info["segments"]) == EXPECTED[name], (name, info)
                assert np.isfinite(ref).all() and info["margin"] >= 1.0, (name, info)
                if info["segments"]:
                    assert ref.max() - ref.min() > 1e-2, (name, ext, ref.min(), ref.max())
                    assert ext or info["clipped"] > 0.0, (name, info)          # the clip branch runs at every probe
                else:
                    assert e32 == 0.0 and np.all(ref == 1e-5), (name, ext)
                rows[(name, ext)] = {"xs": xs, "ref": ref, "e32": e32, "bound": K * e32, "info": info}
        _cache["rows"] = rows
    return _cache["rows"]


def trajectory(name):
    """the float64 search `name`: pso_cases.pso fed the float64 fitness -> dict(draws, H, e32, bound, margin); asserts that every
    decision's margin is at least twice the bound over the positions the search visits"""
    key = ("trajectory", name)
    if key not in _cache:
        inp, N, Kmax, seed, ext = TRAJECTORIES[name]
        draws = pc.draws_after_seed(seed, N, Kmax)
        H = pc.pso(lambda x, it: fitness_of(inp, x, ext), draws, N, Kmax)
        visited = H["positions"].reshape(-1)
        e32 = float(np.abs(fitness_of(inp, visited, ext, np.float32) - H["fitness"].reshape(-1)).max())
        margin = float(H["margins"].min())
        assert margin >= 2.0 * K * e32, (name, margin, K * e32)
        _cache[key] = {"draws": draws, "H": H, "e32": e32, "bound": K * e32, "margin": margin}
    return _cache[key]


def check(name, got, ref, bound):
    """print and assert GPU values against their float64 values: max |got - ref| <= bound"""
    o = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
    print("ROW | %s | %.3g | %.3g" % (name, bound, o))
    assert np.isfinite(o) and o <= bound, (name, o, bound)
    return o
