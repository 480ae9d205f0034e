"""Shared cases of the tests of the resynthesis' adjoint in the mask (tests/test_resynth_grad_*.py): the cotangent of the mask under
tests/resynth_cases.py's restatement, in float64 with np.fft and the np.interp table, the same evaluation with float32 operands and
float32 matrix products, the seeded cotangent of the waveform and the mutants.  Test-side only; nothing here reads a kernel's output,
and resynth_cases is imported and left unchanged.

The forward (rc.restate64) is linear in the mask, so the cotangent needs the noisy signal and dout alone.  With N = min(T, T_mask),
frames n < N:
  X_n = rfft(frame_n w, n_fft);   v_n = dout[n hop : n hop + frame] / wsum * w, the window sum being the forward's (frame 0 alone
  over the first hop, frame N - 1 alone over hop N, two frames elsewhere; below 1e-8: 1);   V_n = rfft(v_n, n_fft);
  dg_n[k] = c_k / n_fft (Re X_n[k] Re V_n[k] + Im X_n[k] Im V_n[k]), c = 1, 2, .., 2, 1 (irfft's weights);
  dmask[n, lo[k]] += (1 - wt[k]) dg_n[k];   dmask[n, lo[k] + 1] += wt[k] dg_n[k]     (rc.interp_table).
Rows from N on are exactly 0, and so is every channel that is neither lo[k] nor lo[k] + 1 of any bin.  dout has no influence from
min(L, (N + 1) hop) on; the seeded dout holds NaN there.

  grad64: float64 throughout: the reference of the GPU rows (tests/test_resynth_grad_host.py pins it to rc.restate64 by the adjoint
    identity <dout, restate64(noisy, m)> == <grad64, m>, and restate64 is pinned to the reference's own output by g23_resynth.npz).
  grad32: the same as two matrix products with float32 operands (rc.operands64 cast), float32 signal and cotangent, float32 1 / wsum
    and table weights, float32 products and sums: a row's e32 = its distance from grad64 relative to the row's largest float64 value.

Bounds.  A GPU row passes within rc.K = 16 x e32.  Every case has two rows, each with its own e32 and its own maximum: the edge
frames (0 and N - 1) and the interior frames.  They are apart for the forward's reason: np.hanning(160)[1] ** 2 = 1.5e-7 is the window
sum of sample 1 of the first hop and of its mirror in the last covered hop, so those two frames see dout times 2.6e3 there, and with
one row they would set the scale for all."""
import numpy as np

import resynth_cases as rc

K = rc.K
MUTANTS = ("interior wsum on the first hop", "last covered hop as interior", "Im column dropped", "Im sign flipped",
           "wt share to idx", "min(T_b, T_mask) ignored", "frames >= N_b given a gradient")

_cache = {}


def live(L, N, hop):
    """samples of dout that have an influence: [0, live)"""
    return min(L, (N + 1) * hop)


def dout_of(L, seed, N, hop):
    """float32 [L]: standard normal, NaN from min(L, (N + 1) hop) on.  Cached and shared: do not modify."""
    key = ("dout", L, seed, N, hop)
    if key not in _cache:
        d = np.random.RandomState(seed + 104729).standard_normal(L).astype(np.float32)
        d[live(L, N, hop):] = np.nan
        _cache[key] = d
    return _cache[key]


def inv_wsum_rows(frame, hop, N, mutant=None):
    """float64 [N + 1, hop]: 1 / window sum of every covered hop"""
    w2 = np.hanning(frame) ** 2
    first, inner, last = w2[:hop].copy(), w2[:hop] + w2[hop:], w2[hop:].copy()
    if mutant == "interior wsum on the first hop":
        first = inner
    if mutant == "last covered hop as interior":
        last = inner
    ws = np.stack([first] + [inner] * (N - 1) + [last])
    ws[ws < 1e-8] = 1.0
    return 1.0 / ws


def grad64(noisy, dout, framing, T_mask, mutant=None):
    """-> float64 [T_mask, C], the cotangent of the mask"""
    frame, hop, n_fft, fs, C = rc.FRAMINGS[framing]
    x = np.asarray(noisy, dtype=np.float64)
    d = np.asarray(dout, dtype=np.float64)
    L = x.shape[0]
    F = n_fft // 2 + 1
    T = rc.frames_of(L, frame, hop)
    N = min(T, T_mask)
    out = np.zeros((T_mask, C))
    if N == 0:
        return out
    Nw = T if mutant == "min(T_b, T_mask) ignored" else N           # the frame count the window sum is taken for
    inv = inv_wsum_rows(frame, hop, Nw, mutant)
    rows = N
    if mutant == "frames >= N_b given a gradient":
        rows = T_mask
        x = np.concatenate([x, np.zeros((T_mask + 1) * hop)])
        d = np.concatenate([np.nan_to_num(d, nan=0.0), np.zeros((T_mask + 1) * hop)])
        inv = np.concatenate([inv, np.ones((T_mask + 2 - inv.shape[0], hop))])
    if mutant == "min(T_b, T_mask) ignored":
        d = np.nan_to_num(d, nan=0.0)
    w = np.hanning(frame)
    lo, wt = rc.interp_table(framing)
    c = np.full(F, 2.0)
    c[0] = c[-1] = 1.0
    for n in range(rows):
        X = np.fft.rfft(x[n * hop:n * hop + frame] * w, n_fft)
        v = d[n * hop:n * hop + frame] * inv[n:n + 2].reshape(-1) * w
        V = np.fft.rfft(v, n_fft)
        im = X.imag * V.imag
        if mutant == "Im column dropped":
            im = 0.0
        if mutant == "Im sign flipped":
            im = -im
        dg = c / n_fft * (X.real * V.real + im)
        np.add.at(out[n], lo, (1.0 - wt) * dg)
        np.add.at(out[n], lo if mutant == "wt share to idx" else lo + 1, wt * dg)
    return out


def grad32(noisy, dout, framing, T_mask):
    """-> float32 [T_mask, C]: grad64's result evaluated with float32 operands and float32 matrix products"""
    frame, hop, n_fft, fs, C = rc.FRAMINGS[framing]
    f32 = np.float32
    x = np.asarray(noisy, dtype=f32)
    L = x.shape[0]
    F = n_fft // 2 + 1
    N = min(rc.frames_of(L, frame, hop), T_mask)
    out = np.zeros((T_mask, C), dtype=f32)
    if N == 0:
        return out
    d = np.asarray(dout, dtype=f32)[:(N + 1) * hop]
    A, S = (a.astype(f32) for a in rc.operands64(frame, n_fft, np.hanning(frame)))
    lo, wt = rc.interp_table(framing)
    wt = wt.astype(f32)
    dy = (d * inv_wsum_rows(frame, hop, N).astype(f32).reshape(-1)).reshape(N + 1, hop)
    fr = np.stack([x[n * hop:n * hop + frame] for n in range(N)])
    dyf = np.concatenate([dy[:N], dy[1:]], axis=1)                  # [N, frame]
    X = fr @ A
    dZ = dyf @ np.ascontiguousarray(S.T)
    P = X * dZ
    dg = P[:, :F] + P[:, F:]
    assert X.dtype == f32 and dZ.dtype == f32 and dg.dtype == f32 and dy.dtype == f32
    acc = np.zeros((C, N), dtype=f32)
    np.add.at(acc, lo, ((f32(1.0) - wt) * dg).T)
    np.add.at(acc, lo + 1, (wt * dg).T)
    out[:N] = acc.T
    return out


def refs(framing, L, seed, dT=0):
    """(noisy, dout, T_mask, g64, g32) of a case of rc.cases.  Cached and shared: do not modify."""
    key = ("refs", framing, L, seed, dT)
    if key not in _cache:
        rc.check_wsum(framing)
        frame, hop = rc.FRAMINGS[framing][:2]
        noisy, mask = rc.case(framing, L, seed, dT)
        T_mask = mask.shape[0]
        N = min(rc.frames_of(L, frame, hop), T_mask)
        dout = dout_of(L, seed, N, hop)
        _cache[key] = (noisy, dout, T_mask, grad64(noisy, dout, framing, T_mask), grad32(noisy, dout, framing, T_mask))
    return _cache[key]


def frame_rows(N):
    """(edge, interior) frame index arrays of N live frames"""
    n = np.arange(N)
    edge = (n == 0) | (n == N - 1)
    return n[edge], n[~edge]


def row_figures(got, g64, g32, N):
    """[(row name, observed, e32)] of the edge frames and the interior frames (a row without frames is left out), after asserting
    that `got` is exactly 0 in the rows from N on and wherever g64 is exactly 0"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == g64.shape and not got[N:].any() and not g64[N:].any()
    assert not got[g64 == 0.0].any()
    edge, interior = frame_rows(N)
    return [(name, rc.fig(got[sel], g64[sel]), rc.fig(g32[sel], g64[sel])) for name, sel in (("edge", edge), ("interior", interior))
            if sel.size]


def check(name, got, g64, g32, N):
    """print and assert both rows of a case: observed <= K x e32"""
    for row, o, e32 in row_figures(got, g64, g32, N):
        print("ROW | %s %s | e32 %.2e | bound %.2e | observed %.2e" % (name, row, e32, K * e32, o))
        assert np.isfinite(o) and o <= K * e32, (name, row, o, K * e32)


def identity_gap(noisy, dout, mask, grad, framing):
    """|<dout, restate64(noisy, mask)> - <grad, mask>| over sum |dout out| + sum |grad mask| (float64; the NaN tail of dout, which
    meets zeros of the forward, counts as 0)"""
    out = rc.restate64(noisy, mask, framing)
    d = np.nan_to_num(np.asarray(dout, dtype=np.float64), nan=0.0)
    g, m = np.asarray(grad, dtype=np.float64), np.asarray(mask, dtype=np.float64)
    scale = np.abs(d * out).sum() + np.abs(g * m).sum()
    return abs(float((d * out).sum()) - float((g * m).sum())) / max(scale, 1e-300)
