"""Shared cases of the ragged front-end kernel tests (tests/test_ragged_kernels_host.py, tests/test_ragged_kernels_gpu.py): one
entry point at a time, synthetic operands, the length sets that take each branch of the `#if ..._VARLEN` blocks, a float64
reference of every operation written out here (the host file pins each to torch's own operator), and the comparison helpers
both files use.  Test-side only; nothing here launches a kernel.

The contract every ragged entry point promises (include/sincformer_hip.h, "The ragged front end"):
  1. what utterance b gets is, bit for bit, what the dense entry point writes for that utterance alone    -> check_rows / check_slots
  2. nothing beyond a length is read: inputs are NaN from each length on, valid outputs are finite         -> check_rows
  3. nothing beyond a length is written but the zeros the contract names: outputs start as NaN            -> check_rows(rest=...)
  4. the valid part meets the dense twin's bound against a float64 reference                               -> check_ref
  5. the batch reversed / laid out with a wider row stride gives every row the same bits                   -> check_same"""
import math

import numpy as np
import torch

from helpers import arr
from oracle import sfm_oracle as orc

FS = 16000
# relative size of one 16-bit rounding of an O(1) value (tests/test_kernels_gpu.py:17, tests/test_sinc_fir16_resident_gpu.py:19)
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NAN = float("nan")


# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------
def _t(x):
    return x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def check_rows(name, got, alone, rest, cols=None):
    """got [B, S, ...]: the ragged launch's result in a buffer that started as NaN; alone[b] [n_b, ...]: the dense launch on
    utterance b alone.  Rows below n_b are finite and equal alone[b] bit for bit; the rows from n_b on are untouched
    (rest="nan") or exact zeros (rest="zero").  cols: the contract covers the first `cols` of the last dimension only, and the
    columns behind them keep their NaN fill in EVERY row."""
    got = _t(got)
    if cols is not None:
        assert bool(torch.isnan(got[..., cols:]).all()), "%s: columns from %d on were written" % (name, cols)
        got = got[..., :cols]
    assert got.shape[0] == len(alone), (name, got.shape, len(alone))
    for b, want in enumerate(alone):
        want = _t(want)
        n = want.shape[0]
        assert n <= got.shape[1] and got[b, :n].shape == want.shape, (name, b, got.shape, want.shape)
        assert bool(torch.isfinite(got[b, :n].float()).all()), "%s, row %d: a valid element is not finite (read past a length)" % (name, b)
        assert torch.equal(got[b, :n], want), "%s, row %d (%d valid): differs from the dense launch on the row alone, max %.3e" % (
            name, b, n, float((got[b, :n].double() - want.double()).abs().max()))
        tail = got[b, n:]
        if rest == "nan":
            assert bool(torch.isnan(tail).all()), "%s, row %d: rows from %d on were written" % (name, b, n)
        else:
            assert rest == "zero"
            assert bool((tail == 0).all()), "%s, row %d: rows from %d on are not exact zeros" % (name, b, n)


def check_slots(name, part, alone, used=None):
    """part [B, P, ...]: GroupNorm partial slots of the ragged launch, zero-filled by the caller; alone[b] [P_b, ...]: those of
    the dense launch on utterance b alone.  The first P_b slots equal alone[b] bit for bit, the slots from P_b on are exact
    zeros.  used[b] (bool [P_b]): the slots utterance b's own length reaches - every other slot of the row is zero too."""
    part = _t(part)
    assert part.shape[0] == len(alone), (name, part.shape, len(alone))
    for b, want in enumerate(alone):
        want = _t(want)
        n = want.shape[0]
        assert n <= part.shape[1], (name, b, n, part.shape)
        assert bool(torch.isfinite(part[b]).all()), "%s, row %d: a partial slot is not finite" % (name, b)
        assert torch.equal(part[b, :n], want), "%s, row %d: partial slots differ from the dense launch on the row alone" % (name, b)
        assert bool((part[b, n:] == 0).all()), "%s, row %d: a partial slot past the last tile (%d) is not zero" % (name, b, n)
        if used is not None:
            u = _t(used[b]).bool()
            assert u.numel() == n and bool((part[b, :n][~u] == 0).all()), "%s, row %d: a slot of a tile past the length is not zero" % (name, b)


def check_same(name, base, other, lens):
    """company: the first lens[b] rows of utterance b are the same bits in both launches"""
    base, other = _t(base), _t(other)
    for b, n in enumerate(lens):
        assert torch.equal(base[b, :n], other[b, :n]), "%s: row %d depends on its company, max %.3e" % (
            name, b, float((base[b, :n].double() - other[b, :n].double()).abs().max()))


WORST = {}          # entry point -> (worst error / bound, error, bound, where): the table the GPU file prints


def check_ref(entry, name, got, ref, tol):
    """max |got - ref| <= tol against the float64 reference; keeps the worst ratio per entry point"""
    got, ref = _t(got).double(), _t(ref).double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e = float((got - ref).abs().max()) if ref.numel() else 0.0
    print("%-28s %-58s max|err| %.3e  bound %.3e" % (entry, name, e, tol))
    ratio = e / tol if math.isfinite(e) else float("inf")
    if entry not in WORST or ratio > WORST[entry][0]:
        WORST[entry] = (ratio, e, tol, name)
    assert math.isfinite(e) and e <= tol, "%s %s: max|err| %.3e > %.3e" % (entry, name, e, tol)
    return e


def worst_table():
    return ["WORST %-28s max|err| %.3e  bound %.3e  (%.2f of the bound)  at %s" % (k, v[1], v[2], v[0], v[3])
            for k, v in sorted(WORST.items())]


def q64(x, dt):
    """round to the 16-bit format `dt`, then float64"""
    return x.to(dt).double()


def nan_tail(x, lens):
    """a copy of x [B, S, ...] with NaN from row lens[b] on in utterance b"""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = NAN
    return x


def conv1d_rows(lin, k, s, p):
    """output rows of a conv over `lin` rows, from the shape torch's own conv1d gives on meta tensors"""
    x = torch.empty(1, 1, int(lin), device="meta")
    return int(torch.nn.functional.conv1d(x, torch.empty(1, 1, k, device="meta"), stride=s, padding=p).shape[-1])


# ---------------------------------------------------------------------------
# sinc_fir16_varlen
# ---------------------------------------------------------------------------
SINC_C = 64
SINC_A = dict(Lrow=2053, lengths=[1, 7, 255, 256, 257, 1023, 1024, 1025, 2048, 2053])      # below a wave-tile, a span, two spans
SINC_A_TAPS = (251, 31, 265)
# Lrow 33000 at B 5.  The launch rule of the one-pass kernel, restated (sinc_spans_per_wg below): a span is 1024 samples, so the
# buffer has ceil(33000 / 1024) = 33 spans; want = ceil((4 * 2 * 256) / (8 * 5)) = 52 segments, but a segment has at least 16
# spans: nseg = min(52, 33 // 16) = 2, so a workgroup walks ceil(33 / 2) = 17 spans and the second workgroup of a row starts at
# sample 17 * 1024 = 17408.  Row 1 ends there (its second workgroup leaves), row 2 hands it one sample, row 4 one sample at all.
SINC_B = dict(Lrow=33000, lengths=[33000, 17408, 17409, 17407, 1], K=251, boundary=17408)
SINC_B_WINDOW = 512
SINC_SPAN, SINC_WAVE_TILE = 1024, 256


def sinc_spans_per_wg(B, Lrow):
    """spans of 1024 samples a workgroup of the resident-tap kernel walks, restated from the launcher's rule"""
    spans = -(-Lrow // SINC_SPAN)
    want = -(-(4 * 2 * 256) // (8 * B))
    nseg = max(1, min(want, spans // 16))
    return -(-spans // nseg)


def sinc_tiles(L):
    """GroupNorm partial slots of a row of L samples: 8192-sample chunks of 32 wave-tiles x 8 shifts"""
    return -(-L // 8192) * 256


def sinc_slot(g, o):
    """slot of wave-tile g = sample // 256 and shift o (tests/test_sinc_fir16_resident_gpu.py:86-90)"""
    return (g // 8) * 64 + o * 8 + g % 8


def sinc_used(L):
    """bool [sinc_tiles(L)]: the slots the wave-tiles inside L own"""
    used = torch.zeros(sinc_tiles(L), dtype=torch.bool)
    for g in range(-(-L // SINC_WAVE_TILE)):
        for o in range(8):
            used[sinc_slot(g, o)] = True
    return used


_SINC = {}


def sinc_filters(K):
    """[64, K] fp32 taps: the bank of tests/test_sinc_fir16_resident_gpu.py"""
    if K not in _SINC:
        p = orc.sinc_init(SINC_C, K, FS)
        _SINC[K] = orc.sinc_filters(p["low_hz_"] * (FS / 8.0), p["band_hz_"] * (FS / 8.0), p["window"], p["n_"], FS).contiguous()
    return _SINC[K]


def sinc_wave(B, Lrow, seed=23):
    return arr("rk_firx", (B, Lrow), seed, 0.3)


def sinc_ref64(x, filt, dt, rows=None):
    """float64 FIR of ONE row x [L] (valid samples only; zero edges) with taps [C, K]: out[m, c] = sum_k h[c, k] x[m + k - K // 2]
    on the operands as the one-pass kernel rounds them - the waveform once to `dt`, the taps once to `dt` after the 2^12
    pre-scale that keeps fp16 taps out of the subnormals (sinc_fir16_prep_kernel).  rows: output samples to evaluate (all)."""
    K = filt.shape[1]
    xq = q64(x, dt) if dt is not None else x.double()
    hq = (q64(filt * 4096.0, dt) / 4096.0) if dt is not None else filt.double()
    xp = torch.nn.functional.pad(xq, (K // 2, K // 2))
    win = xp.unfold(0, K, 1)                                                    # [L, K]: window of output sample m
    if rows is not None:
        win = win[rows]
    return win @ hq.t()                                                         # [n, C]


def sinc_windows(L, boundary=None, w=SINC_B_WINDOW):
    """sorted output samples of a row of L on which the long case evaluates the reference: the first and last `w`, and +-w around
    the workgroup boundary"""
    idx = set(range(min(w, L))) | set(range(max(L - w, 0), L))
    if boundary is not None:
        idx |= set(range(max(boundary - w, 0), min(boundary + w, L)))
    return torch.tensor(sorted(idx), dtype=torch.long)


def sinc_tol(dt):
    return 4 * EPS[dt] * 0.1                                                    # tests/test_sinc_fir16_resident_gpu.py:81


# ---------------------------------------------------------------------------
# conv16p_varlen
# ---------------------------------------------------------------------------
# (cin, N, k, s, p, inputs, fused skip): the seven instantiations of the dense dispatcher, all of them used by the path
CONV_FORMS = [(64, 128, 7, 2, 3, 1, True), (128, 128, 7, 2, 3, 2, True), (128, 256, 7, 2, 3, 2, False), (128, 256, 1, 2, 0, 2, False),
              (128, 128, 3, 1, 1, 1, False), (256, 256, 3, 1, 1, 1, False), (256, 256, 5, 2, 2, 2, False)]
CONV_LOUTS = (1, 2, 127, 128, 129, 256, 257)        # below a tile, its edges, two tiles and their edges
CONV_MIN_BUFFER_LOUT = 385                          # a fourth 128-row tile column that no row reaches


def conv_form_id(f):
    return "cin%d-N%d-k%d-s%d-in%d%s" % (f[0], f[1], f[2], f[3], f[5], "-skip" if f[6] else "")


def conv_lengths(k, s, p, extra=0):
    """(lin per row, lout per row, buffer Lin, buffer Lout): the `lin` whose conv1d shape is each of CONV_LOUTS - lin 1 among
    them, and for a stride-2 form both the even and the odd lin that give 128 and 129 rows; the buffer is the shortest whose
    own Lout is CONV_MIN_BUFFER_LOUT (+ extra rows of stride for the company check).  Not sorted: short rows sit between long ones."""
    by_lout = {}
    lin = 1
    while True:
        lo = conv1d_rows(lin, k, s, p)
        by_lout.setdefault(lo, []).append(lin)
        if lo >= CONV_MIN_BUFFER_LOUT:
            break
        lin += 1
    Lin = lin + extra
    lins = []
    for lo in CONV_LOUTS:
        cand = by_lout[lo]
        lins += cand if (s == 2 and lo in (128, 129)) else cand[:1]
    assert lins[0] == 1
    order = [lins[i] for i in np.random.RandomState(7).permutation(len(lins))]
    return order, [conv1d_rows(l, k, s, p) for l in order], Lin, conv1d_rows(Lin, k, s, p)


def conv_operands(form, B, Lin):
    """fp32 operands of a form, as tests/test_kernels_gpu.py:292-299 draws them"""
    cin, N, k, s, p, nin, skip = form
    two = nin == 2
    d = dict(x1=arr("rk_px1", (B, Lin, cin), 20), x2=arr("rk_px2", (B, Lin, cin), 21) if two else None,
             sc1=arr("rk_ps1", (B, cin), 22) * 0.2 + 1.0, sh1=arr("rk_ph1", (B, cin), 23) * 0.3,
             sc2=arr("rk_ps2", (B, cin), 24) * 0.2 + 0.7 if two else None, sh2=arr("rk_ph2", (B, cin), 25) * 0.3 if two else None,
             w=arr("rk_pw", (N, cin, k), 26) / math.sqrt(cin * k), b=arr("rk_pb", (N,), 27),
             ws=arr("rk_pws", (N, cin, 1), 28) / math.sqrt(cin) if skip else None, bs=arr("rk_pbs", (N,), 29) if skip else None)
    return d


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def conv_taps64(xn, w, bias, s, p):
    """float64 Conv1d written out tap by tap: xn [lin, cin] channels-last, w [N, cin, k] -> [lout, N], zero padding p, stride s"""
    lin, k = xn.shape[0], w.shape[2]
    lout = (lin + 2 * p - k) // s + 1
    xp = torch.nn.functional.pad(xn, (0, 0, p, p))
    out = bias.double().repeat(lout, 1)
    for t in range(k):
        out = out + xp[t:t + (lout - 1) * s + 1:s] @ w[:, :, t].double().t()
    return out


def conv_ref64(d, b, lin, form, dt=torch.float16):
    """float64 reference of utterance b cut to lin rows, on the operands as conv16p rounds them (raw inputs, the normalised
    operand GELU(sc1 x1 + sh1 [+ sc2 x2 + sh2]), the weights: tests/test_kernels_gpu.py:300-304) -> main [lout, N], skip or None"""
    cin, N, k, s, p, nin, skip = form
    z = q64(d["x1"][b, :lin], dt) * d["sc1"][b].double() + d["sh1"][b].double()
    if nin == 2:
        z = z + q64(d["x2"][b, :lin], dt) * d["sc2"][b].double() + d["sh2"][b].double()
    xn = q64(gelu64(z), dt)
    main = conv_taps64(xn, q64(d["w"], dt), d["b"], s, p)
    sk = conv_taps64(xn, q64(d["ws"], dt), d["bs"], 2, 0) if skip else None
    return main, sk


def conv_tol(dt, out_dt, ref):
    """tests/test_kernels_gpu.py:318 (fp32 result) and :332 (16-bit result)"""
    tol = 8 * EPS[dt]
    return tol if out_dt == torch.float32 else tol + 2 * EPS[dt] * float(ref.abs().max())


def conv_slots(lout):
    return 2 * (-(-lout // 128))


def group_sums64(ref, G):
    """[rows, N] float64 -> (sum, sum of squares) per group of N / G columns over all rows: [G], [G]"""
    rg = ref.reshape(ref.shape[0], G, -1)
    return rg.sum(dim=(0, 2)), (rg ** 2).sum(dim=(0, 2))


def conv_sum_tol(lout):
    """tests/test_kernels_gpu.py:322,327: bounds of the summed partials (sum, sum of squares)"""
    return 2e-2 * lout ** 0.5, 5e-2 * lout ** 0.5


# ---------------------------------------------------------------------------
# gn_finalize_varlen / gn_apply_varlen
# ---------------------------------------------------------------------------
GN_SHAPES = [(8, 64), (16, 256), (32, 512)]
GN_SYNTH_ROWS = [700, 1, 8, 5, 9, 4200]             # rows per utterance; 8 rows per slot: 1 .. 525 slots (the fold's second pass of 512)
GN_SLOT_ROWS = 8
GN_EPS = 1e-5
U32 = 2.0 ** -24


def gn_affine(C, seed=13):
    return arr("rk_gnw", (C,), seed) * 0.1 + 1.0, arr("rk_gnb", (C,), seed + 1) * 0.1


def gn_synth_partials(G, C, rows_tab, Pmax=None, dtype=torch.float32):
    """synthetic partials [B, Pmax, G, 2] (sum, sum of squares of GN_SLOT_ROWS-row slots of per-group random data with a group offset),
    NaN in the slots from p_tab[b] on, and p_tab.  dtype float64: the same sums before the fp32 store, and the data [rows, C]"""
    B = len(rows_tab)
    p_tab = [-(-r // GN_SLOT_ROWS) for r in rows_tab]
    Pmax = Pmax or max(p_tab)
    part = torch.full((B, Pmax, G, 2), NAN, dtype=dtype)
    data = []
    for b, r in enumerate(rows_tab):
        g = torch.Generator().manual_seed(100 + b)
        x = (torch.randn(r, C, generator=g, dtype=torch.float64) * (0.5 + 0.1 * b) + torch.linspace(-1.0, 2.0, G).repeat_interleave(C // G))
        pad = p_tab[b] * GN_SLOT_ROWS - r
        xs = torch.nn.functional.pad(x, (0, 0, 0, pad)).reshape(p_tab[b], GN_SLOT_ROWS, G, C // G)
        part[b, :p_tab[b], :, 0] = xs.sum(dim=(1, 3)).to(dtype)
        part[b, :p_tab[b], :, 1] = (xs ** 2).sum(dim=(1, 3)).to(dtype)
        data.append(x)
    return part, p_tab, data


def gn_finalize64(part, rows, w, b, eps=GN_EPS):
    """float64 GroupNorm scale / shift of ONE utterance from its partial slots part [P, G, 2] over `rows` rows of C channels:
    mean and biased variance of the group, scale = w / sqrt(var + eps), shift = b - mean scale -> [C], [C], and the bound of an
    fp32 evaluation of these two expressions from exact sums, 4 x 2^-24 of the terms: scale = fl(w fl(rstd)) is two roundings;
    shift = fl(b - fl(fl(mean) scale)) carries the two of scale, one of the mean, one of the product (4 on |mean scale|) and
    one of the difference (on |b| + |mean scale|)"""
    G, C = part.shape[1], w.numel()
    cpg = C // G
    count = float(rows) * cpg
    s, q = part[..., 0].double().sum(0), part[..., 1].double().sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = w.double() * rstd.repeat_interleave(cpg)
    mean_c = mean.repeat_interleave(cpg)
    shift = b.double() - mean_c * scale
    return scale, shift, 4 * U32 * scale.abs(), 4 * U32 * (b.double().abs() + 2 * (mean_c * scale).abs())


def gn_apply_ref64(x, sc, sh, dt):
    """GELU(x sc + sh) of ONE utterance's valid rows x [n, C] (16-bit values), float64"""
    return gelu64(q64(x, dt) * sc.double() + sh.double())


def gn_apply_tol(dt, ref):
    """elementwise: the fp32 GroupNorm + GELU bound of tests/test_kernels_gpu.py:269 (5e-4) plus one rounding of the result to
    the 16-bit format (EPS |ref|)"""
    return 5e-4 + EPS[dt] * float(ref.abs().max())


# ---------------------------------------------------------------------------
# headpool_varlen
# ---------------------------------------------------------------------------
HP_N, HP_K, HP_GCOLS, HP_LDP = 512, 256, 16, 520
HP_PAIRS = [(9, 2), (100, 21), (300, 300), (640, 129), (2555, 512)]          # (Tin, Tout): one tile beside many; windows of 1 frame
HP_STRIDES = [(2555, 512), (2558, 514)]                                      # (TinS, ToutS): nothing to zero for the longest; two rows
HP_TILES = [(32, 1), (32, 1), (32, 10), (25, 6), (25, 21)]                   # (frames per tile, tiles) the rule gives for HP_PAIRS


def headpool_frames_per_tile(Tin, Tout):
    """the rule restated: the largest f <= 32 whose tiles of f pooled frames never span more than 128 input rows (0: refused)"""
    if Tin <= 0 or Tout <= 0 or Tin < Tout:
        return 0
    for f in range(32, 0, -1):
        if all(-(-(min(i0 + f, Tout) * Tin) // Tout) - (i0 * Tin) // Tout <= 128 for i0 in range(0, Tout, f)):
            return f
    return 0


def headpool_operands(B, TinS):
    return dict(x=arr("rk_hpx", (B, TinS, HP_K), 41), w=arr("rk_hpw", (HP_N, HP_K), 42) / 16.0, b=arr("rk_hpb", (HP_N,), 43))


def headpool_ref64(x, w, bias, Tout, dt):
    """x [Tin, 256] of ONE utterance -> raw heads [Tin, N] float64 on the rounded operands, and their adaptive average over
    [(i Tin) // Tout, ceil((i + 1) Tin / Tout)) for i < Tout (tests/test_kernels_gpu.py:179-180)"""
    Tin = x.shape[0]
    raw = q64(x, dt) @ q64(w, dt).t() + bias.double()
    pooled = torch.stack([raw[(i * Tin) // Tout: -((-(i + 1) * Tin) // Tout)].mean(0) for i in range(Tout)])
    return raw, pooled


# ---------------------------------------------------------------------------
# bilstm_layer_rows16_varlen
# ---------------------------------------------------------------------------
LSTM_H = 128
LSTM_TOL = 2e-3                                     # tests/test_bilstm_mfma_gpu.py:17
LSTM_PADCOLS = 24
# (ttab, row stride T): tail steps only (1, 2, 3: the four-step xg ring re-reads row Tj - 1) beside a chain of 130 in one
# workgroup, three workgroups; a workgroup whose Tw is 1, then one live chain with three idle columns; B 1; every chain full
LSTM_CASES = [([130, 1, 2, 3, 5, 129, 4, 7, 21], 130), ([1, 1, 1, 1, 130], 130), ([3], 7), ([130] * 5, 130)]


def lstm_operands(B, T):
    """xg [B, T, 2, 4H], whh [2, 4H, H] as tests/test_bilstm_mfma_gpu.py:30-32 draws them (rows of the first B x T)"""
    g = torch.Generator().manual_seed(20)
    xg = torch.randn(9, 130, 2, 4 * LSTM_H, generator=g)
    whh = torch.randn(2, 4 * LSTM_H, LSTM_H, generator=g) / LSTM_H ** 0.5
    return xg[:B, :T].contiguous(), whh


def lstm_chain64(xg, whh, reverse, round16=True, start=None, steps=None):
    """float64 LSTM recurrence of ONE chain, written out: xg [T, 4H] input projection (gate order i, f, g, o), whh [4H, H];
    h, c start at zero; forward walks rows 0 .. T - 1, reverse walks T - 1 .. 0; -> h [T, H].  round16: W_hh once and h before
    every product are rounded to fp16, as the kernel's recurrent operands are.  start / steps: a wrong walk, for the mutants."""
    T, H = xg.shape[0], xg.shape[1] // 4
    w = (whh.half() if round16 else whh).double()
    h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
    out = torch.zeros(T, H, dtype=torch.float64)
    order = list(range(T - 1, -1, -1) if reverse else range(T))
    if start is not None:
        order = list(range(start, -1, -1))
    if steps is not None:
        order = order[:steps]
    for t in order:
        hq = h.half().double() if round16 else h
        pre = xg[t].double() + w @ hq
        i, f, g, o = pre.split(H)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return out


def lstm_ref64(xg, whh, Tj, round16=True):
    """xg [T, 2, 4H] of ONE utterance cut to Tj steps -> [Tj, 2H] (forward | reverse)"""
    return torch.cat([lstm_chain64(xg[:Tj, 0], whh[0], False, round16), lstm_chain64(xg[:Tj, 1], whh[1], True, round16)], dim=1)


# ---------------------------------------------------------------------------
# rows_gather32
# ---------------------------------------------------------------------------
# (element type, rows_tab, src rows per utterance, src columns, dst columns, width)
GATHER_CASES = [(torch.float16, [21, 26, 26, 26, 41, 53, 21], 53, 24, 32, 20),         # the shape of tests/test_ragged_path_gpu.py
                (torch.float32, [4, 1, 9, 1, 6], 9, 7, 9, 5),                            # 4-byte words, an odd width, rows of 1
                (torch.float32, [3], 5, 7, 9, 5), (torch.float16, [1], 4, 24, 32, 20)]   # B 1


def gather_ref(src, rows_tab, width):
    """src [B, T, ld] -> the packed rows [sum rows_tab, width]"""
    return torch.cat([src[b, :n, :width] for b, n in enumerate(rows_tab)])
