"""Each ragged front-end entry point on the MI355X, alone and on synthetic operands, at the length edges its `#if ..._VARLEN`
block has (cases, references and helpers: tests/ragged_kernel_cases.py; the path as a whole: tests/test_ragged_path_gpu.py).
Every case runs the five checks of the cases file: bitwise against the dense wrapper on each row alone, NaN inputs from each
length on, NaN outputs / zero partials before the launch, the dense twin's bound against float64, and independence of the
batch order and of the row stride.  The last lines of the file's output are the worst error of every entry point beside its
bound.  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

import ragged_kernel_cases as rk
from helpers import arr

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16]
DT_ID = {F16: "fp16", BF16: "bf16", F32: "fp32"}
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    yield _ops
    print()
    for line in rk.worst_table():
        print(line)


@pytest.fixture(autouse=True)
def _reset(ops):
    yield
    ops.reset_precision()


def dev(t):
    return None if t is None else t.cuda().contiguous()


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def nans(*shape, dtype):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


# ---------------------------------------------------------------------------
# sinc_fir16_varlen
# ---------------------------------------------------------------------------
def _sinc_ragged(ops, x, lengths, filt, K, out_dt, passes, Lrow=None, order=None):
    """the ragged launch on rows `order` of x (NaN from each length on, row stride Lrow) -> out, partials in the given order"""
    B, L0 = x.shape
    Lrow = Lrow or L0
    order = list(order or range(B))
    xb = torch.full((B, Lrow), NAN)
    for i, b in enumerate(order):
        xb[i, :lengths[b]] = x[b, :lengths[b]]
    out = nans(B, Lrow, 64, dtype=out_dt)
    part, P = ops.sinc_fir16_varlen(dev(xb), i32(lengths[b] for b in order), filt, out, 64, K, sum(lengths), passes=passes)
    torch.cuda.synchronize()
    assert P == rk.sinc_tiles(Lrow) and tuple(part.shape) == (B, P, 8, 2)
    inv = [order.index(b) for b in range(B)]
    return out[inv], part[inv]


def _sinc_alone(ops, x, lengths, filt, K, out_dt, passes):
    outs, parts = [], []
    for b, L in enumerate(lengths):
        o = nans(1, L, 64, dtype=out_dt)
        p, P = ops.sinc_fir16(dev(x[b:b + 1, :L]), filt, o, 1, L, 64, K, passes=passes)
        assert P == rk.sinc_tiles(L)
        outs.append(o[0].cpu())
        parts.append(p[0].cpu())
    return outs, parts


def _sinc_case(ops, dt, out32, Lrow, lengths, K, boundary=None, wide=None):
    ops.set_compute_dtype(dt)
    out_dt = F32 if out32 else dt
    passes = 0 if (dt is F16 and not out32) else 1        # the path's own call where the auto rule picks one pass
    B = len(lengths)
    x, filt = rk.sinc_wave(B, Lrow), rk.sinc_filters(K)
    fd = dev(filt)
    out, part = _sinc_ragged(ops, x, lengths, fd, K, out_dt, passes)
    alone, alone_p = _sinc_alone(ops, x, lengths, fd, K, out_dt, passes)
    name = "L%d K%d %s->%s" % (Lrow, K, DT_ID[dt], DT_ID[out_dt])
    rk.check_rows("sinc_fir16_varlen out " + name, out, alone, "nan")
    rk.check_slots("sinc_fir16_varlen gn_partial " + name, part, alone_p, used=[rk.sinc_used(L) for L in lengths])
    part = part.cpu()
    for b, L in enumerate(lengths):                       # the slots inside the length carry the sums
        assert bool(part[b, :rk.sinc_tiles(L)][rk.sinc_used(L)][..., 1].sum() > 0), (name, b)
    oc = out.cpu()
    for b, L in enumerate(lengths):
        rows = None if boundary is None else rk.sinc_windows(L, boundary)
        ref = rk.sinc_ref64(x[b, :L], filt, dt, rows)
        rk.check_ref("sinc_fir16_varlen", "%s row %d (L %d)" % (name, b, L), oc[b, :L] if rows is None else oc[b, rows], ref, rk.sinc_tol(dt))
    rev, rev_p = _sinc_ragged(ops, x, lengths, fd, K, out_dt, passes, order=range(B - 1, -1, -1))
    rk.check_same("sinc_fir16_varlen reversed " + name, out, rev, lengths)
    assert torch.equal(part, rev_p.cpu())
    wide = wide or Lrow + 75
    wid, wid_p = _sinc_ragged(ops, x, lengths, fd, K, out_dt, passes, Lrow=wide)
    rk.check_rows("sinc_fir16_varlen wider row stride " + name, wid, alone, "nan")
    assert torch.equal(wid_p[:, :part.shape[1]].cpu(), part) and bool((wid_p[:, part.shape[1]:] == 0).all())
    return part


@pytest.mark.parametrize("out32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("K", rk.SINC_A_TAPS)
def test_sinc_fir16_varlen_rows_shorter_than_a_tile_a_span_and_two(ops, K, dt, out32):
    """case A: one workgroup per (row, shift); rows of 1 and 7 samples, the edges of a 256-sample wave-tile and of a
    1024-sample span, the full row"""
    _sinc_case(ops, dt, out32, rk.SINC_A["Lrow"], rk.SINC_A["lengths"], K)


@pytest.mark.parametrize("out32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_sinc_fir16_varlen_rows_that_end_at_the_second_workgroup(ops, dt, out32):
    """case B: two workgroups of 17 spans per (row, shift): the early return of the second one (rows 1, 3, 4), the clamp of its
    last span (row 2: one sample), and the boundary itself shown by the outcome: row 1 (17408 samples) has zeros in every slot
    of the tiles from 17408 on, row 2 (17409) has a sum in the slot of the tile at 17408"""
    c = rk.SINC_B
    B, bd = len(c["lengths"]), c["boundary"]
    assert rk.sinc_spans_per_wg(B, c["Lrow"]) * rk.SINC_SPAN == bd
    # the wider row stride moves the boundary (18 spans per workgroup): the result does not depend on the choice
    wide = 34817
    assert rk.sinc_spans_per_wg(B, wide) == 18
    part = _sinc_case(ops, dt, out32, c["Lrow"], c["lengths"], c["K"], boundary=bd, wide=wide)
    g, P = bd // rk.SINC_WAVE_TILE, part.shape[1]

    def slots_from(g0):                                   # bool [P]: the slots of the wave-tiles from g0 on
        m = torch.zeros(P, dtype=torch.bool)
        for gg in range(g0, P // 8):
            for o in range(8):
                m[rk.sinc_slot(gg, o)] = True
        return m
    assert bool((part[1][slots_from(g)] == 0).all()), "row 1 ends on the boundary: nothing from sample %d on" % bd
    assert float(part[2, rk.sinc_slot(g, 0), :, 1].sum()) > 0, "row 2 has one sample in the tile at %d" % bd
    assert bool((part[2][slots_from(g + 1)] == 0).all()) and bool((part[4][slots_from(1)] == 0).all())


# ---------------------------------------------------------------------------
# conv16p_varlen (+ gn_finalize_varlen on the partials it produced)
# ---------------------------------------------------------------------------
def _conv_ragged(ops, form, d16, pw, spw, lins, louts, Lin, out_dt, order=None):
    cin, N, k, s, p, nin, skip = form
    B = len(lins)
    order = list(order or range(B))
    Lout = rk.conv1d_rows(Lin, k, s, p)
    P = rk.conv_slots(Lout)

    def rows(t):                                            # [B, Lin, cin] in the launch's order, NaN from each length on
        if t is None:
            return None
        buf = torch.full((B, Lin, cin), NAN, dtype=F16)
        for i, b in enumerate(order):
            buf[i, :lins[b]] = t[b, :lins[b]]
        return dev(buf)
    pick = lambda t: None if t is None else dev(t[order])
    out, part = nans(B, Lout, N, dtype=out_dt), torch.zeros(B, P, 16, 2, device="cuda")
    out_s = nans(B, Lout, N, dtype=out_dt) if skip else None
    part_s = torch.zeros(B, P, 16, 2, device="cuda") if skip else None
    ops.conv16p_varlen(rows(d16["x1"]), pick(d16["sc1"]), pick(d16["sh1"]), pw, out, i32(lins[b] for b in order),
                       i32(louts[b] for b in order), B=B, Lin=Lin, stride=s, pad=p, n_out=sum(louts), x2=rows(d16["x2"]),
                       sc2=pick(d16["sc2"]), sh2=pick(d16["sh2"]), gn_partial=part, gn_group=N // 16, skip_pw=spw, out_s=out_s,
                       gn_partial_s=part_s)
    torch.cuda.synchronize()
    inv = [order.index(b) for b in range(B)]
    return [None if t is None else t[inv] for t in (out, part, out_s, part_s)]


def _conv_alone(ops, form, d16, pw, spw, lins, louts, out_dt):
    cin, N, k, s, p, nin, skip = form
    res = []
    for b, (lin, lout) in enumerate(zip(lins, louts)):
        cut = lambda t: None if t is None else dev(t[b:b + 1, :lin])
        one = lambda t: None if t is None else dev(t[b:b + 1])
        P = rk.conv_slots(lout)
        out, part = nans(1, lout, N, dtype=out_dt), torch.zeros(1, P, 16, 2, device="cuda")
        out_s = nans(1, lout, N, dtype=out_dt) if skip else None
        part_s = torch.zeros(1, P, 16, 2, device="cuda") if skip else None
        ops.conv16p(cut(d16["x1"]), one(d16["sc1"]), one(d16["sh1"]), pw, out, B=1, Lin=lin, stride=s, pad=p, x2=cut(d16["x2"]),
                    sc2=one(d16["sc2"]), sh2=one(d16["sh2"]), gn_partial=part, gn_group=N // 16, skip_pw=spw, out_s=out_s,
                    gn_partial_s=part_s)
        res.append([None if t is None else t[0].cpu() for t in (out, part, out_s, part_s)])
    return res


@pytest.mark.parametrize("out_dt", [F32, F16], ids=["out32", "out16"])
@pytest.mark.parametrize("form", rk.CONV_FORMS, ids=[rk.conv_form_id(f) for f in rk.CONV_FORMS])
def test_conv16p_varlen_rows_far_below_a_tile_beside_rows_of_several(ops, form, out_dt):
    """rows of 1, 2, 127 .. 129, 256 and 257 output rows in a buffer of 385: tiles that start past a row leave, and no
    workgroup of the fourth tile column writes; then gn_finalize_varlen on the partials this launch produced"""
    cin, N, k, s, p, nin, skip = form
    ops.set_compute_dtype(F16)
    lins, louts, Lin, Lout = rk.conv_lengths(k, s, p)
    assert Lout >= rk.CONV_MIN_BUFFER_LOUT and max(louts) <= 3 * 128 and min(lins) == 1
    B = len(lins)
    d = rk.conv_operands(form, B, Lin)
    d16 = dict(d, x1=d["x1"].half(), x2=None if d["x2"] is None else d["x2"].half())
    pw = ops.pack_linear(dev(d["w"]), dev(d["b"]))
    spw = ops.pack_linear(dev(d["ws"]), dev(d["bs"])) if skip else None
    got = _conv_ragged(ops, form, d16, pw, spw, lins, louts, Lin, out_dt)
    alone = _conv_alone(ops, form, d16, pw, spw, lins, louts, out_dt)
    name = "%s %s" % (rk.conv_form_id(form), DT_ID[out_dt])
    for j, what in ((0, "out"), (2, "out_s")):
        if got[j] is not None:
            rk.check_rows("conv16p_varlen %s %s" % (what, name), got[j], [a[j] for a in alone], "nan")
            rk.check_slots("conv16p_varlen gn_partial of %s %s" % (what, name), got[j + 1], [a[j + 1] for a in alone])
    for b, (lin, lout) in enumerate(zip(lins, louts)):
        ref, ref_s = rk.conv_ref64(d, b, lin, form)
        assert ref.shape[0] == lout
        ts, tq = rk.conv_sum_tol(lout)
        for j, r, what in ((0, ref, "out"), (2, ref_s, "skip")):
            if r is None:
                continue
            rk.check_ref("conv16p_varlen", "%s %s row %d (lout %d)" % (name, what, b, lout), got[j][b, :lout].cpu(), r,
                         rk.conv_tol(F16, out_dt, r))
            sums = got[j + 1][b].cpu().double().sum(0)                          # [16, 2]
            s0, s1 = rk.group_sums64(r, 16)
            assert float((sums[:, 0] - s0).abs().max()) < ts, (name, what, b, float((sums[:, 0] - s0).abs().max()), ts)
            if j == 0:                                                          # (the twin bounds the skip conv's sums only)
                assert float((sums[:, 1] - s1).abs().max()) < tq, (name, what, b, float((sums[:, 1] - s1).abs().max()), tq)
    rev = _conv_ragged(ops, form, d16, pw, spw, lins, louts, Lin, out_dt, order=range(B - 1, -1, -1))
    wide = _conv_ragged(ops, form, d16, pw, spw, lins, louts, Lin + 300, out_dt)     # the same rows inside longer buffers
    for j in (0, 2):
        if got[j] is not None:
            rk.check_same("conv16p_varlen reversed " + name, got[j], rev[j], louts)
            assert torch.equal(got[j + 1], rev[j + 1])
            rk.check_rows("conv16p_varlen wider row stride " + name, wide[j], [a[j] for a in alone], "nan")
            rk.check_slots("conv16p_varlen wider row stride, gn_partial " + name, wide[j + 1], [a[j + 1] for a in alone])
    # gn_finalize_varlen on these partials (G 16, C = N), NaN in the slots it must not read
    if out_dt is F32:
        _finalize_case(ops, "conv partials " + name, got[1].cpu(), louts, [rk.conv_slots(lo) for lo in louts], 16, N)


def test_conv16p_varlen_refuses_bf16_operands(ops):
    """fp16 only: with bf16 operands the launcher answers SFM_ERR_SHAPE and launches nothing"""
    form = rk.CONV_FORMS[4]
    cin, N, k, s, p, nin, skip = form
    ops.set_compute_dtype(BF16)
    lins, louts, Lin, Lout = rk.conv_lengths(k, s, p)
    B = len(lins)
    d = rk.conv_operands(form, B, Lin)
    pw = ops.pack_linear(dev(d["w"]), dev(d["b"]))
    out = nans(B, Lout, N, dtype=BF16)
    part = torch.zeros(B, rk.conv_slots(Lout), 16, 2, device="cuda")
    with pytest.raises(RuntimeError, match=r"unsupported shape \(-2\)"):
        ops.conv16p_varlen(dev(d["x1"].to(BF16)), dev(d["sc1"]), dev(d["sh1"]), pw, out, i32(lins), i32(louts), B=B, Lin=Lin,
                           stride=s, pad=p, n_out=sum(louts), gn_partial=part, gn_group=N // 16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((part == 0).all())


# ---------------------------------------------------------------------------
# gn_finalize_varlen / gn_apply_varlen
# ---------------------------------------------------------------------------
def _finalize_case(ops, name, part, rows_tab, p_tab, G, C):
    """part [B, Pmax, G, 2] (CPU, fp32): scale / shift of the ragged launch - with NaN in every slot from p_tab[b] on - bitwise
    against gn_finalize on each utterance alone, against the float64 formula, reversed and with a wider slot stride"""
    B, Pmax = part.shape[:2]
    w, bb = rk.gn_affine(C)
    wd, bd = dev(w), dev(bb)
    poisoned = rk.nan_tail(part, p_tab)

    def run(pt, order, Pm):
        sc, sh = ops.gn_finalize_varlen(dev(pt[order]), wd, bd, i32(rows_tab[b] for b in order), i32(p_tab[b] for b in order), B, Pm,
                                        G, C)
        inv = [order.index(b) for b in range(B)]
        return sc[inv].cpu(), sh[inv].cpu()
    sc, sh = run(poisoned, list(range(B)), Pmax)
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all()), name + ": a slot past p_tab was read"
    for b in range(B):
        one = dev(part[b:b + 1, :p_tab[b]])
        s1, h1 = ops.gn_finalize(one, wd, bd, 1, p_tab[b], G, C, rows_tab[b])
        assert torch.equal(sc[b], s1[0].cpu()) and torch.equal(sh[b], h1[0].cpu()), "%s, row %d: differs from gn_finalize alone" % (name, b)
        rs, rh, ts, th = rk.gn_finalize64(part[b, :p_tab[b]], rows_tab[b], w, bb)
        es, eh = (sc[b].double() - rs).abs(), (sh[b].double() - rh).abs()
        rk.check_ref("gn_finalize_varlen", "%s G%d C%d row %d (rows %d): scale err / bound" % (name, G, C, b, rows_tab[b]),
                     es / ts, torch.zeros_like(es), 1.0)
        rk.check_ref("gn_finalize_varlen", "%s G%d C%d row %d (rows %d): shift err / bound" % (name, G, C, b, rows_tab[b]),
                     eh / th, torch.zeros_like(eh), 1.0)
    sr, hr = run(poisoned, list(range(B - 1, -1, -1)), Pmax)
    assert torch.equal(sr, sc) and torch.equal(hr, sh), name + ": reversed"
    wider = torch.cat([poisoned, torch.full((B, 3, G, 2), NAN)], dim=1)
    sw, hw = run(wider, list(range(B)), Pmax + 3)
    assert torch.equal(sw, sc) and torch.equal(hw, sh), name + ": wider slot stride"
    return sc, sh


@pytest.mark.parametrize("G,C", rk.GN_SHAPES)
def test_gn_finalize_varlen_on_synthetic_partials(ops, G, C):
    """rows_tab with 1, one slot, a slot edge, and 525 slots (the fold's second pass of 512)"""
    part, p_tab, _ = rk.gn_synth_partials(G, C, rk.GN_SYNTH_ROWS)
    _finalize_case(ops, "synthetic", part, rk.GN_SYNTH_ROWS, p_tab, G, C)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_gn_finalize_varlen_on_sinc_partials(ops, dt):
    """(G 8, C 64) on what sinc_fir16_varlen wrote: case A (a row of one sample) and case B (1280 slots)"""
    ops.set_compute_dtype(dt)
    for c, K in ((rk.SINC_A, 251), (rk.SINC_B, rk.SINC_B["K"])):
        lengths = c["lengths"]
        x = rk.sinc_wave(len(lengths), c["Lrow"])
        _, part = _sinc_ragged(ops, x, lengths, dev(rk.sinc_filters(K)), K, dt, 1)
        _finalize_case(ops, "sinc partials Lrow %d %s" % (c["Lrow"], DT_ID[dt]), part.cpu(), lengths, [rk.sinc_tiles(L) for L in lengths], 8, 64)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("C", [64, 256])
def test_gn_apply_varlen_gelu_rows_then_zeros(ops, dt, C):
    ops.set_compute_dtype(dt)
    rows_tab, L = [300, 1, 256, 257, 5, 700], 700
    B = len(rows_tab)
    x = arr("rk_gax", (B, L, C), 31).to(dt)
    sc, sh = arr("rk_gas", (B, C), 32) * 0.2 + 1.0, arr("rk_gah", (B, C), 33) * 0.3

    def run(order, Lr):
        xb = torch.full((B, Lr, C), NAN, dtype=dt)
        for i, b in enumerate(order):
            xb[i, :rows_tab[b]] = x[b, :rows_tab[b]]
        out = nans(B, Lr, C, dtype=dt)
        ops.gn_apply_varlen(dev(xb), dev(sc[order]), dev(sh[order]), out, i32(rows_tab[b] for b in order), B, Lr, C, sum(rows_tab))
        return out[[order.index(b) for b in range(B)]].cpu()
    out = run(list(range(B)), L)
    alone = []
    for b, n in enumerate(rows_tab):
        o = nans(1, n, C, dtype=dt)
        ops.gn_apply(dev(x[b:b + 1, :n]), dev(sc[b:b + 1]), dev(sh[b:b + 1]), o, 1, n, C, act=1)
        alone.append(o[0].cpu())
    name = "C%d %s" % (C, DT_ID[dt])
    rk.check_rows("gn_apply_varlen " + name, out, alone, "zero")
    for b, n in enumerate(rows_tab):
        ref = rk.gn_apply_ref64(x[b, :n], sc[b], sh[b], dt)
        rk.check_ref("gn_apply_varlen", "%s row %d (rows %d)" % (name, b, n), out[b, :n], ref, rk.gn_apply_tol(dt, ref))
    rk.check_rows("gn_apply_varlen reversed " + name, run(list(range(B - 1, -1, -1)), L), alone, "zero")
    rk.check_rows("gn_apply_varlen wider row stride " + name, run(list(range(B)), L + 41), alone, "zero")


# ---------------------------------------------------------------------------
# headpool_varlen
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_headpool_varlen_one_tile_beside_twenty_one(ops, dt):
    """(Tin, Tout) of one tile beside rows of 6, 10 and 21 tiles: the zero fill of the pooled rows shared out over PS workgroups,
    the exit of the tiles past P_b; first with strides at which the longest row has nothing to zero, then with two more rows;
    then gn_finalize_varlen (G 32, C 512) on the partials"""
    ops.set_compute_dtype(dt)
    pairs = rk.HP_PAIRS
    B = len(pairs)
    keep = ops.switch("headpool")
    ops.set_headpool(True)                                                           # (whatever SFM_HEADPOOL says)
    try:
        tab = ops.headpool_tab([a for a, _ in pairs], [b for _, b in pairs])
    finally:
        ops.set_headpool(keep)
    assert tab is not None and [tuple(r) for r in tab[:, 2:].tolist()] == rk.HP_TILES
    PS = int(tab[:, 3].max())
    d = rk.headpool_operands(B, max(a for a, _ in pairs))
    pw = ops.pack_linear(dev(d["w"]), dev(d["b"]))
    N, ldp = rk.HP_N, rk.HP_LDP
    x16 = d["x"].to(dt)

    def run(order, TinS, ToutS):
        xb = torch.full((B, TinS, rk.HP_K), NAN, dtype=dt)
        for i, b in enumerate(order):
            xb[i, :pairs[b][0]] = x16[b, :pairs[b][0]]
        pooled, part = nans(B, ToutS, ldp, dtype=dt), torch.zeros(B, PS, N // 16, 2, device="cuda")
        ops.headpool_varlen(dev(xb), pw, pooled, part, torch.from_numpy(tab[order]).cuda().contiguous(), B, TinS, ToutS, PS,
                            sum(a for a, _ in pairs), sum(b for _, b in pairs))
        torch.cuda.synchronize()
        inv = [order.index(b) for b in range(B)]
        return pooled[inv].cpu(), part[inv].cpu()
    alone, alone_p = [], []
    for b, (Tin, Tout) in enumerate(pairs):
        po, pa = nans(1, Tout, ldp, dtype=dt), torch.zeros(1, int(tab[b, 3]), N // 16, 2, device="cuda")
        ops.headpool(dev(x16[b:b + 1, :Tin]), pw, po, pa, 1, Tin, Tout)
        assert bool(torch.isnan(po[..., N:]).all())
        alone.append(po[0, :, :N].cpu())
        alone_p.append(pa[0].cpu())
    base = None
    for TinS, ToutS in rk.HP_STRIDES:
        name = "%s strides %d / %d" % (DT_ID[dt], TinS, ToutS)
        pooled, part = run(list(range(B)), TinS, ToutS)
        rk.check_rows("headpool_varlen pooled " + name, pooled, alone, "zero", cols=N)
        rk.check_slots("headpool_varlen gn_partial " + name, part, alone_p)
        if base is None:
            base = (pooled, part)
            for b, (Tin, Tout) in enumerate(pairs):
                raw, ref = rk.headpool_ref64(x16[b, :Tin], d["w"], d["b"], Tout, dt)
                tag = "%s row %d (%d -> %d)" % (DT_ID[dt], b, Tin, Tout)
                rk.check_ref("headpool_varlen", tag + " pooled", pooled[b, :Tout, :N], ref, 3 * rk.EPS[dt] * float(ref.abs().max()))
                s0, s1 = rk.group_sums64(raw, N // 16)
                sums = part[b].double().sum(0)
                rg = raw.reshape(Tin, N // 16, 16)
                rk.check_ref("headpool_varlen", tag + " sum", sums[:, 0], s0, 2e-5 * float(rg.abs().sum((0, 2)).max()))
                rk.check_ref("headpool_varlen", tag + " sum of squares", sums[:, 1], s1, 2e-5 * float(s1.max()))
        rev, rev_p = run(list(range(B - 1, -1, -1)), TinS, ToutS)
        rk.check_rows("headpool_varlen reversed " + name, rev, alone, "zero", cols=N)
        assert torch.equal(rev_p, part) and torch.equal(part, base[1])
    _finalize_case(ops, "headpool partials " + DT_ID[dt], base[1], [a for a, _ in pairs], [int(t) for t in tab[:, 3]], 32, N)


# ---------------------------------------------------------------------------
# bilstm_layer_rows16_varlen
# ---------------------------------------------------------------------------
def _lstm_ragged(ops, xg, whh, ttab, T, dt, order=None, Tr=None):
    """-> [B, Tr, 2H + 24] (rows in the caller's order): NaN from each chain's length on in xg, a NaN destination with 24 more columns"""
    H, B = rk.LSTM_H, len(ttab)
    Tr = Tr or T
    order = list(order or range(B))
    xb = torch.full((B, Tr, 2, 4 * H), NAN)
    for i, b in enumerate(order):
        xb[i, :ttab[b]] = xg[b, :ttab[b]]
    buf = nans(B * Tr, 2 * H + rk.LSTM_PADCOLS, dtype=dt)
    got = ops.bilstm_layer_rows16_varlen(dev(xb), whh, i32(ttab[b] for b in order), B, Tr, H, sum(ttab), out16=buf[:, :2 * H])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and got.stride(0) == 2 * H + rk.LSTM_PADCOLS
    return buf.view(B, Tr, -1)[[order.index(b) for b in range(B)]].cpu()


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("ttab,T", rk.LSTM_CASES, ids=["tails-beside-130", "Tw1-then-one-live-chain", "B1", "all-full"])
def test_bilstm_layer_rows16_varlen_chains_of_tail_steps_only(ops, ttab, T, dt):
    ops.set_compute_dtype(dt)
    H, B = rk.LSTM_H, len(ttab)
    xg, whh = rk.lstm_operands(B, T)
    wd = dev(whh)
    out = _lstm_ragged(ops, xg, wd, ttab, T, dt)
    alone = [ops.bilstm_layer_rows16(dev(xg[b:b + 1, :Tj]), wd, 1, Tj, H).cpu() for b, Tj in enumerate(ttab)]
    name = "ttab %s T %d %s" % (ttab, T, DT_ID[dt])
    rk.check_rows("bilstm_layer_rows16_varlen " + name, out, alone, "zero", cols=2 * H)
    if all(Tj == T for Tj in ttab):                            # every chain full: the dense launch on the same batch
        dense = ops.bilstm_layer_rows16(dev(xg), wd, B, T, H).view(B, T, 2 * H).cpu()
        assert torch.equal(out[..., :2 * H], dense)
    for b, Tj in enumerate(ttab):
        ref = rk.lstm_ref64(xg[b], whh, Tj)
        for dname, sl in (("forward", slice(0, H)), ("reverse", slice(H, 2 * H))):
            rk.check_ref("bilstm_layer_rows16_varlen", "%s chain %d (%d steps) %s" % (DT_ID[dt], b, Tj, dname), out[b, :Tj, sl], ref[:, sl],
                         rk.LSTM_TOL)
        if Tj > 1:
            # the two directions are different functions of this input, and the reverse chain walked forwards is far outside
            assert float((ref[:, :H] - ref[:, H:]).abs().max()) > 50 * rk.LSTM_TOL
            fwd = rk.lstm_chain64(xg[b, :Tj, 1], whh[1], False)
            assert float((fwd - out[b, :Tj, H:2 * H].double()).abs().max()) > 50 * rk.LSTM_TOL
    rev = _lstm_ragged(ops, xg, wd, ttab, T, dt, order=range(B - 1, -1, -1))
    rk.check_rows("bilstm_layer_rows16_varlen reversed " + name, rev, alone, "zero", cols=2 * H)
    wide = _lstm_ragged(ops, xg, wd, ttab, T, dt, Tr=T + 3)
    rk.check_rows("bilstm_layer_rows16_varlen wider row stride " + name, wide, alone, "zero", cols=2 * H)


# ---------------------------------------------------------------------------
# rows_gather32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,rows_tab,T,scols,dcols,width", rk.GATHER_CASES, ids=["fp16-path-shape", "fp32-odd-width", "fp32-B1", "fp16-B1"])
def test_rows_gather32_two_and_four_byte_elements(ops, dt, rows_tab, T, scols, dcols, width):
    B, n = len(rows_tab), sum(rows_tab)
    off = [sum(rows_tab[:b]) for b in range(B)]
    src = arr("rk_gsrc", (B, T, scols), 5).to(dt)

    def run(order, Tr):
        sb = torch.full((B, Tr, scols), NAN, dtype=dt)
        for i, b in enumerate(order):
            sb[i, :rows_tab[b]] = src[b, :rows_tab[b]]
        dst = nans(n + 1, dcols, dtype=dt)
        ops.rows_gather32(dev(sb).view(B * Tr, scols), dst[:-1], i32(rows_tab[b] for b in order), i32(off[b] for b in order), B, Tr, width, n)
        torch.cuda.synchronize()
        return dst.cpu()
    want = rk.gather_ref(src, rows_tab, width)
    for what, dst in (("", run(list(range(B)), T)), (" reversed", run(list(range(B - 1, -1, -1)), T)), (" wider row stride", run(list(range(B)), T + 3))):
        assert torch.equal(dst[:-1, :width], want), "rows_gather32%s: the packed rows" % what
        assert bool(torch.isnan(dst[:, width:]).all()) and bool(torch.isnan(dst[-1]).all()), "rows_gather32%s: wrote outside its rows" % what
