"""Shared cases of the tests of the STOI / ESTOI gradient (tests/test_stoi_loss_*.py): tests/stoi_taal_cases.py::stoi64 restated in
torch float64 with autograd behind the ENHANCED signal.  Test-side only; nothing here comes from the package.

Everything of the clean side (its resampled signal, the kept list, its band rows) is a numpy constant.  Operands are held in a
chosen dtype by straight-through rounding, a + (round(a) - a).detach(), at the points where the device holds fp32: taps, window,
DFT matrix, signals, resampled samples, band rows; every sum is float64.  sqrt and the norms pass nothing back at zero (a plain
torch.sqrt gives NaN on a clean signal of zeros and on an enhanced signal with a silent stretch).  The resampler is a conv1d on the
zero-stuffed signal.

Bound.  Per case and measure e32g = the relative RMSE between the gradient of the float32-operand evaluation and the float64
one, computed here on the CPU; a device gradient passes within K = 16 x e32g relative RMSE of the float64 gradient, and must be
exactly 0 wherever the float64 gradient is exactly 0 (samples of dropped frames, samples only the last kept frame covers, the
tail behind the last frame).

The generator asserts, beside the 1 dB keep margin of stoi_taal_cases.evaluated(): every clip comparison |a y - c x| / (c x) of every
case with segments is at least 1e-4 (the clip decision is discontinuous), and cases 4, 7 and 8 clip.

Ascent.  ASCENT_STEP: ten steps e += ASCENT_STEP * d score / d e on case 4 raise the float64 score by at least 10 x the case's
forward e32 (asserted in the host test, where the rise is computed with this file's gradient)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import stoi_taal_cases as sc

K = sc.K
GRAD_CASES = (2, 3, 4, 6, 7, 8, 9, 10)
CONSTANT_CASES = (1, 5, 11)
CLIPPING = (4, 7, 8)
MIN_CLIP_MARGIN = 1e-4
# the silent stretch: case-4-sized pair without gap or burst, enhanced samples 2000 .. 3000 set to 0
SILENT = (6000, 10000, 2000, 3000)
# the long utterance: 16 kHz, 32000 samples, a gap - 155 frames, 127 kept, 126 band rows, 97 segments.  The segment backward gives a
# workgroup 32 band rows and walks the segments of a workgroup in stages of 32 through rings of 64 rows: here there are four row
# blocks (and a fifth that only writes zeros), the inner ones walk 61 segments in two stages, and rows from 64 on wrap the rings -
# the path of every utterance of a second or more, which the twelve cases of stoi_taal_cases (63 rows at the most) do not reach
LONG = (32000, 16000, (9000, 15000))
ASCENT_CASE, ASCENT_STEPS, ASCENT_STEP = 4, 10, 2.0
MUTANTS = ("through clipped", "alpha constant", "window once", "last frame taken", "kept from enhanced", "plain sqrt")

_cache = {}
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)


def case(num):
    return next(c for c in sc.CASES if c[0] == num)


def silent_pair():
    L, fs, a, b = SILENT
    c, e = sc.pair(L, fs)
    e = e.copy()
    e[a:b] = 0.0
    return c, e


def long_pair():
    L, fs, gap = LONG
    return sc.pair(L, fs, gap)


def forward_row(c, e, fs, ext):
    """the row stoi_taal_cases.check takes, for a pair beside its table: float64 value, e32, bound; asserts the 1 dB keep margin"""
    info = {}
    ref = sc.stoi64(c, e, fs, ext, np.float64, info=info)
    e32 = abs(sc.stoi64(c, e, fs, ext, np.float32) - ref)
    assert np.isfinite(ref) and info["margin"] >= 1.0 and info["kept"] < info["frames"], info
    return {"ref": ref, "e32": e32, "bound": K * e32, "info": info}


def _st(a, dtype):
    """a held in `dtype`: the rounded value, the gradient of the identity"""
    if dtype == np.float64:
        return a
    return a + (a.detach().float().double() - a.detach())


def _const(a, dtype):
    return torch.from_numpy(sc._as(a, dtype))


def sqrt0(s, plain=False):
    """sqrt that passes nothing back at 0"""
    if plain:
        return torch.sqrt(s)
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def norm0(v, dim):
    return sqrt0((v * v).sum(dim, keepdim=True))


def resample_t(y, fs, dtype):
    """stoi_taal_cases.resample with a graph: conv1d on the zero-stuffed signal"""
    y = _st(y, dtype)
    if fs == sc.FS:
        return y
    g = math.gcd(sc.FS, fs)
    up, down = sc.FS // g, fs // g
    h = _const(sc.taps(up, down), dtype)
    half = (h.numel() - 1) // 2
    z = torch.zeros(y.numel() * up, dtype=torch.float64)
    z = torch.index_add(z, 0, torch.arange(y.numel()) * up, y)
    full = F.conv1d(z[None, None], h.flip(0)[None, None], padding=h.numel() - 1)[0, 0]         # np.convolve(z, h)
    n = -(-y.numel() * up // down)
    idx = half + torch.arange(n) * down
    out = torch.where(idx < full.numel(), full[torch.clamp(idx, max=full.numel() - 1)], torch.zeros(n, dtype=torch.float64))
    return _st(out, dtype)


def score_t(clean, enh, fs, extended=False, dtype=np.float64, mutant=None, info=None):
    """stoi64(clean, enh, fs, extended, dtype) as a torch float64 scalar with a graph behind `enh` (a float64 tensor of the
    float32 samples).  info receives margin_clip: the smallest |a y - c x| / (c x) over the clip comparisons with c x > 0."""
    n = min(len(clean), enh.numel())
    x = sc.resample(clean[:n], fs, dtype)
    y = resample_t(enh[:n], fs, dtype)
    w_np = sc._as(np.hanning(sc.NF + 2)[1:-1], dtype)
    w = torch.from_numpy(w_np)
    const = torch.tensor(1e-5, dtype=torch.float64) + 0.0 * enh.sum()
    if x.size < sc.NF:
        return const
    yf = y.unfold(0, sc.NF, sc.HOP) * w
    if mutant == "kept from enhanced":
        e = 20.0 * np.log10(np.linalg.norm(yf.detach().numpy(), axis=1) + sc.EPS)
    else:
        xf_all = np.array([w_np * x[i:i + sc.NF] for i in range(0, x.size - sc.NF + 1, sc.HOP)])
        e = 20.0 * np.log10(np.linalg.norm(xf_all, axis=1) + sc.EPS)
    mask = (np.max(e) - sc.DYN - e) < 0
    xf = np.array([w_np * x[i:i + sc.NF] for i in range(0, x.size - sc.NF + 1, sc.HOP)])[mask]
    yk = yf[torch.from_numpy(np.nonzero(mask)[0])]
    nk = len(xf)
    xs, ys = np.zeros((nk - 1) * sc.HOP + sc.NF), torch.zeros((nk - 1) * sc.HOP + sc.NF, dtype=torch.float64)
    for i in range(nk):
        xs[i * sc.HOP:i * sc.HOP + sc.NF] += xf[i]
        ys = ys + F.pad(yk[i], (i * sc.HOP, ys.numel() - i * sc.HOP - sc.NF))
    nspec = nk - 1 + (1 if mutant == "last frame taken" else 0)
    if nspec < 1:
        return const
    ang = 2.0 * np.pi * ((np.arange(sc.NF)[:, None] * np.arange(sc.NFFT // 2 + 1)[None, :]) % sc.NFFT) / sc.NFFT
    C_np, S_np = sc._as(np.cos(ang), dtype), sc._as(-np.sin(ang), dtype)
    tab = sc.band_table()
    frx = np.array([w_np * xs[i:i + sc.NF] for i in range(0, nspec * sc.HOP, sc.HOP)]).reshape(-1, sc.NF)
    px = (frx @ C_np) ** 2 + (frx @ S_np) ** 2
    xt = sc._as(np.sqrt(np.stack([px[:, lo:hi].sum(1) for lo, hi in tab])), dtype)             # [15, frames]
    v = ys.unfold(0, sc.NF, sc.HOP)[:nspec]
    if mutant == "window once":
        v = v + (v * w - v).detach()                           # the value of w v, the gradient of v
    else:
        v = v * w
    py = (v @ torch.from_numpy(C_np)) ** 2 + (v @ torch.from_numpy(S_np)) ** 2
    yt = _st(torch.stack([sqrt0(py[:, lo:hi].sum(1), plain=mutant == "plain sqrt") for lo, hi in tab]), dtype)
    M = xt.shape[1]
    if M < sc.SEG:
        return const
    xg = torch.from_numpy(np.array([xt[:, m - sc.SEG:m] for m in range(sc.SEG, M + 1)]))      # [S, 15, 30]
    yg = yt.unfold(1, sc.SEG, 1).permute(1, 0, 2)
    if extended:
        def rc(a):
            a = a - a.mean(2, keepdim=True)
            a = a / (norm0(a, 2) + sc.EPS)
            a = a - a.mean(1, keepdim=True)
            return a / (norm0(a, 1) + sc.EPS)
        return (rc(xg) * rc(yg) / sc.SEG).sum() / xg.shape[0]
    alpha = norm0(xg, 2) / (norm0(yg, 2) + sc.EPS)
    if mutant == "alpha constant":
        alpha = alpha.detach()
    yn = yg * alpha
    lim = xg * CLIP
    clipped = yn > lim
    if info is not None:
        pos = lim > 0
        info["clipped"] = float(clipped.double().mean())
        info["margin_clip"] = float(((yn - lim).abs()[pos] / lim[pos]).min().detach()) if bool(pos.any()) else float("inf")
    if mutant == "through clipped":
        yp = torch.where(clipped, lim + (yn - yn.detach()), yn)
    else:
        yp = torch.where(clipped, lim, yn)
    yp = yp - yp.mean(2, keepdim=True)
    xz = xg - xg.mean(2, keepdim=True)
    yp = yp / (norm0(yp, 2) + sc.EPS)
    xz = xz / (norm0(xz, 2) + sc.EPS)
    return (yp * xz).sum() / (xg.shape[0] * xg.shape[1])


def value_and_grad(clean, enhanced, fs, extended=False, dtype=np.float64, mutant=None, info=None):
    """(score float, d score / d enhanced float64 [L]) of float32 signals"""
    e = torch.from_numpy(np.asarray(enhanced, dtype=np.float32).astype(np.float64)).requires_grad_(True)
    s = score_t(clean, e, fs, extended, dtype, mutant, info)
    g, = torch.autograd.grad(s, e)
    return float(s.detach()), g.numpy()


def rel_rmse(got, ref):
    d = np.linalg.norm(np.asarray(got, dtype=np.float64) - ref)
    n = np.linalg.norm(ref)
    return float(d / n) if n > 0 else float(d)


def _row(c, e, fs, ext):
    info = {}
    val, g64 = value_and_grad(c, e, fs, ext, np.float64, info=info)
    _, g32 = value_and_grad(c, e, fs, ext, np.float32)
    e32g = rel_rmse(g32, g64)
    assert np.isfinite(g64).all() and np.isfinite(g32).all()
    return {"value": val, "grad": g64, "e32g": e32g, "bound": K * e32g, "zeros": int((g64 == 0).sum()), "info": info}


def evaluated():
    """{(number | "silent" | "long", extended): dict(value, grad, e32g, bound, zeros, info)}, computed once and shared (do not modify);
    asserts the generator's conditions"""
    if "rows" not in _cache:
        sc.evaluated()                                        # the 1 dB keep margin of every case
        rows = {}
        for num in GRAD_CASES:
            cs = case(num)
            c, e = sc.case_pair(cs)
            for ext in sc.MEASURES:
                rows[(num, ext)] = _row(c, e, cs[1], ext)
            inf = rows[(num, False)]["info"]
            assert inf["margin_clip"] >= MIN_CLIP_MARGIN, (num, inf)
            if num in CLIPPING:
                assert inf["clipped"] > 0.0, (num, inf)
        c, e = silent_pair()
        for ext in sc.MEASURES:
            rows[("silent", ext)] = _row(c, e, SILENT[1], ext)
        assert rows[("silent", False)]["info"]["margin_clip"] >= MIN_CLIP_MARGIN
        c, e = long_pair()
        for ext in sc.MEASURES:
            rows[("long", ext)] = dict(_row(c, e, LONG[1], ext), forward=forward_row(c, e, LONG[1], ext))
        inf = rows[("long", False)]
        assert inf["info"]["margin_clip"] >= MIN_CLIP_MARGIN and inf["info"]["clipped"] > 0.0
        assert (inf["forward"]["info"]["frames"], inf["forward"]["info"]["kept"], inf["forward"]["info"]["segments"]) == (155, 127, 97)
        _cache["rows"] = rows
    return _cache["rows"]


def violates(got, row):
    """why `got` fails the GPU test's assertion against `row`, or None"""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return "not finite"
    zero = row["grad"] == 0
    if np.any(got[zero] != 0):
        return "%d non-zero elements where the float64 gradient is exactly 0" % int(np.count_nonzero(got[zero]))
    o = rel_rmse(got, row["grad"])
    return None if o <= row["bound"] else "relative RMSE %.3e beyond %.3e" % (o, row["bound"])


def check(name, got, row):
    """print and assert a device gradient against its case: relative RMSE <= K x e32g, exact zeros where the reference has them"""
    got = np.asarray(got, dtype=np.float64)
    o = rel_rmse(got, row["grad"]) if np.isfinite(got).all() else float("nan")
    print("ROW | %s | float64 |grad| %.6e | e32g %.2e | bound %.2e | observed %.2e | exact zeros %d"
          % (name, np.linalg.norm(row["grad"]), row["e32g"], row["bound"], o, row["zeros"]))
    why = violates(got, row)
    assert why is None, (name, why)
