"""The PerceptionAgent's GroupNorm and time-pooling training nodes (the kernels train.PerceptionFunction runs nine times a step,
forward and backward), each called directly and compared, element by element, with its float64 restatement in
tests/pa_nodes_cases.py (pinned to float64 torch autograd and shown to separate wrong kernels by tests/test_host_logic.py).

Bounds come from the reference alone (helpers.py: K_SUM / K_TRANS x e32, or the fp32 sum bound), plus - where a kernel evaluates
normal_cdf_poly - the allowance written out in pa_nodes_cases for EPS_POLY, the polynomial's largest error as
tests/test_normal_cdf_host.py measures it from the header's literals.  Every row prints its `ROW | ...` line; profiles/README.md
keeps the table."""

import pytest
import torch

import helpers as hp
import pa_nodes_cases as pc
from test_normal_cdf_host import EPS_POLY

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
NAN = float("nan")
SENTINEL = 7.0
GUARD = 3                                                   # rows (or table rows) of NaN / sentinel on each side of an operand


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    assert EPS_POLY == pc.eps_poly()                        # the bounds below name the figure the host sweep measured
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def train():
    from sincformer_metacog_speech_enhancement_amd import train as _train
    return _train


def dev(t):
    return None if t is None else t.cuda().contiguous()


def _id(row):
    return "-".join(str(v) for v in row) if isinstance(row, tuple) else str(row).replace("torch.", "")


def guarded(t, fill, dtype=None):
    """`t` [n, ...] on the device between GUARD leading and trailing slices of `fill`: (whole buffer, the view that holds t)"""
    t = t.cuda() if dtype is None else t.cuda().to(dtype)
    buf = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), fill, device="cuda", dtype=t.dtype)
    buf[GUARD:GUARD + t.shape[0]] = t
    return buf, buf[GUARD:GUARD + t.shape[0]]


def guards_hold(buf, fill=SENTINEL):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


# ---------------------------------------------------------------------------
# gn_finalize + ops.gn_stats
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dc", pc.GN_FIN_DC, ids=["zero-mean", "dc30"])
@pytest.mark.parametrize("CG", pc.GN_FIN_CG, ids=_id)
@pytest.mark.parametrize("P", pc.GN_FIN_P)
def test_gn_finalize_and_stats(ops, P, CG, dc):
    """fp32 partial slots built on the CPU -> scale / shift (gn_finalize) and mean / rstd (ops.gn_stats) against gn_finalize64 in
    float64 on the same fp32 partials, K_TRANS x e32 (behind the square root and the division); the two must describe the same
    statistics: scale = gamma rstd to one fp32 unit (2^-23 of the value), shift = beta - mean scale to one unit of its two terms.
    The distance to the two-pass statistics of x itself (what rounding the slots to fp32 costs) is printed, not asserted."""
    C, G = CG
    c = pc.gn_finalize_case(P, C, G, dc)
    B, L = c["B"], c["L"]
    part = dev(c["partial"])
    scale, shift = ops.gn_finalize(part, dev(c["gamma"]), dev(c["beta"]), B, P, G, C, L)
    mean, rstd = ops.gn_stats(part, L, C, G)
    got = [t.cpu() for t in (mean, rstd, scale, shift)]
    name = "P %d C %d G %d dc %g" % (P, C, G, dc)
    for i, what in enumerate(pc.GN_FIN_NAMES):
        hp.check_row("gn_finalize %s %s" % (what, name), got[i], c["ref64"][i], c["ref32"][i], hp.K_TRANS)
        f = hp.figs(got[i], c["exact"][i])
        print("FIGURE | gn_finalize %s %s | distance to the two-pass statistics of x %.2e %.2e" % (what, name, f[0], f[1]))
    cg = C // G
    ga, be = c["gamma"].double(), c["beta"].double()
    sc, sh = got[2].double(), got[3].double()
    want_sc = got[1].double().repeat_interleave(cg, dim=1) * ga
    ms = got[0].double().repeat_interleave(cg, dim=1) * sc
    u = 2.0 ** -23
    d_sc = float(((sc - want_sc).abs() / sc.abs()).max())
    d_sh = float(((sh - (be - ms)).abs() / (be.abs() + ms.abs())).max())
    print("ROW | gn_stats vs gn_finalize %s | all | unit 2^-23 | scale - gamma rstd: %.2f units | shift - (beta - mean scale): %.2f units"
          % (name, d_sc / u, d_sh / u))
    assert d_sc <= u and d_sh <= u


# ---------------------------------------------------------------------------
# gn_apply
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("row", pc.GN_APPLY_ROWS, ids=_id)
def test_gn_apply(ops, row, dt):
    """act(x1 sc1 + sh1 [+ x2 sc2 + sh2]) for act 0 / 1 / 2, one and two inputs, fp32 and 16-bit x, fp32 and 16-bit result.
    fp32 result: K_TRANS x e32.  16-bit result: one rounding + K_TRANS x e32, and for GELU the EPS_POLY |p| allowance inside the
    switch (pa_nodes_cases.gn_apply_extra).  NaN rows around x and around the scale / shift tables, sentinel rows around the
    result: the sentinels stay and no NaN arrives."""
    B, L, C = row
    ops.set_compute_dtype(dt)
    f64, f32 = torch.float64, torch.float32
    for two in (False, True):
        for x_dt in (None, dt):
            c = pc.gn_apply_case(row, two, x_dt)
            xs = [guarded(x.reshape(B * L, C), NAN, x_dt)[1] for x in c["xs"]]
            scs = [guarded(s, NAN)[1] for s in c["scs"]]
            shs = [guarded(h, NAN)[1] for h in c["shs"]]
            extra = pc.gn_apply_extra(c["p64"], c["p32"])
            for act in (0, 1, 2):
                r64, r32 = c["ev"](f64, act)[1], c["ev"](f32, act)[1]
                for out_dt in (f32, dt):
                    buf, out = guarded(torch.full((B * L, C), NAN), SENTINEL, out_dt)
                    if two:
                        ops.gn_apply(xs[0], scs[0], shs[0], out, B, L, C, act=act, x2=xs[1], sc2=scs[1], sh2=shs[1])
                    else:
                        ops.gn_apply(xs[0], scs[0], shs[0], out, B, L, C, act=act)
                    name = "gn_apply %s act %d %s x %s -> %s" % (_id(row), act, "two" if two else "one", _id(x_dt or f32), _id(out_dt))
                    assert guards_hold(buf), name
                    got = out.float().cpu().reshape(B, L, C)
                    assert not torch.isnan(got).any(), name
                    if out_dt == f32:
                        hp.check_row(name, got, r64, r32, hp.K_TRANS)
                    else:
                        pc.check_elem(name, got, r64, r32, hp.K_TRANS, extra if act == 1 else None, dt)


# ---------------------------------------------------------------------------
# gn_act_backward: gn_bwd_reduce, gn_bwd_coefs, gn_bwd_apply through the wrapper
# ---------------------------------------------------------------------------
def _gn_bwd(ops, c, row, io_dt):
    B, L, C, G, act, two = row
    cast = (lambda t: dev(t)) if io_dt is None else (lambda t: dev(t).to(io_dt))
    args = []
    for i in range(2 if two else 1):
        args += [cast(c["xs"][i]), dev(c["scs"][i]), dev(c["shs"][i]), dev(c["means"][i]), dev(c["rstds"][i]), dev(c["gam"][i])]
    res = ops.gn_act_backward(cast(c["dout"]), act, G, *args, dx_dtype=io_dt or torch.float32)
    dx1, dg1, db1 = res[:3]
    if two:
        assert torch.equal(res[5], db1)                     # one dbeta: that of the sum of the two normalised inputs
        return [dx1.clone(), res[3].clone(), dg1.clone(), res[4].clone(), db1.clone()]
    return [dx1.clone(), None, dg1.clone(), None, db1.clone()]


@pytest.mark.parametrize("deterministic", [True, False], ids=["ordered", "atomics"])
@pytest.mark.parametrize("io", [None] + DTYPES, ids=["fp32", "bfloat16", "float16"])
@pytest.mark.parametrize("row", pc.GN_BWD_ROWS, ids=_id)
def test_gn_act_backward(ops, row, io, deterministic):
    """dx, dgamma, dbeta against gn_bwd64 with the statistics of the float64 restatement rounded to fp32, in the storage formats
    of the path: fp32 x, dout, dx (the latent heads) or all three 16-bit.  Both arms of the reduce: the ordered fold of row-tile
    partials (two calls, equal bits) and the fp32 atomics, within the same bounds.  dx: K_TRANS x e32 (+ one rounding of a 16-bit
    dx); dgamma / dbeta: K_SUM x e32 or the (B L + 8) 2^-24 sum|terms| bound; act 1 adds the EPS_POLY allowance of
    pa_nodes_cases.gn_bwd_case on each."""
    B, L, C, G, act, two = row
    if io is not None:
        ops.set_compute_dtype(io)
    c = pc.gn_bwd_case(row, io)
    before = ops.is_deterministic()
    try:
        ops.set_deterministic(deterministic)
        got = _gn_bwd(ops, c, row, io)
        if deterministic:
            again = _gn_bwd(ops, c, row, io)
            for i, (u, v) in enumerate(zip(got, again)):
                assert (u is None and v is None) or torch.equal(u, v), ("ordered arm is not bit-reproducible", pc.GN_BWD_NAMES[i])
    finally:
        ops.set_deterministic(before)
    tag = "%s %s %s" % (_id(row), _id(io or torch.float32), "ordered" if deterministic else "atomics")
    for i, what in enumerate(pc.GN_BWD_NAMES):
        if got[i] is None:
            assert c["ref64"][i] is None
            continue
        name = "gn_act_backward %s %s" % (what, tag)
        g = got[i].float().cpu()
        assert g.shape == c["ref64"][i].shape
        if i < 2:
            if act == 0 and io is None:
                hp.check_row(name, g, c["ref64"][i], c["ref32"][i], hp.K_TRANS)
            elif act == 0:
                hp.check_row16(name, g, c["ref64"][i], c["ref32"][i], hp.K_TRANS, io)
            else:                                           # the same two forms with the EPS_POLY allowance of each element added
                pc.check_elem(name, g, c["ref64"][i], c["ref32"][i], hp.K_TRANS, c["extra"][i], io)
        else:
            pc.check_elem(name, g, c["ref64"][i], c["ref32"][i], hp.K_SUM, c["extra"][i], None, c["sums"][i])


# ---------------------------------------------------------------------------
# pooling over time and its adjoint
# ---------------------------------------------------------------------------
def _padded(t, fill, dtype=torch.float32):
    """[B, T, C] -> device [B, T, C + POOL_PAD] in `dtype` with `fill` in the padding columns"""
    B, T, C = t.shape
    buf = torch.full((B, T, C + pc.POOL_PAD), fill, device="cuda", dtype=dtype)
    buf[:, :, :C] = t.cuda().to(dtype)
    return buf


def _pool(ops, c, B, Tin, Tout, C, src_dt, dst_dt, affine, tag):
    """one call that writes dst16 and dst32 together; both checked, the sentinel columns behind them too"""
    ops.set_compute_dtype(dst_dt)
    src = _padded(c["srcs"][src_dt], NAN, src_dt)
    d16 = torch.full((B, Tout, C + pc.POOL_PAD), SENTINEL, device="cuda", dtype=dst_dt)
    d32 = torch.full((B, Tout, C + pc.POOL_PAD), SENTINEL, device="cuda")
    ld = C + pc.POOL_PAD
    ops.pool_time(src, d16, d32, B, Tin, Tout, C, ld, ld, dev(c["scale"]) if affine else None, dev(c["shift"]) if affine else None)
    name = "pool_time%s %s src %s" % (" affine" if affine else "", tag, _id(src_dt))
    r64, r32 = (c[("aff64", src_dt)], c[("aff32", src_dt)]) if affine else (c["plain64"], c["plain32"])
    for d in (d16, d32):
        assert bool((d[:, :, C:] == SENTINEL).all()), name
    hp.check_row(name + " dst32", d32[:, :, :C].cpu(), r64, r32, hp.K_SUM)
    hp.check_row16(name + " dst16 %s" % _id(dst_dt), d16[:, :, :C].float().cpu(), r64, r32, hp.K_SUM, dst_dt)
    return d32[:, :, :C].cpu()


def _pool_rows(ops, train, B, Tin, Tout, C):
    f32 = torch.float32
    c = pc.pool_case(B, Tin, Tout, C)
    tag = "B%d C%d %d->%d" % (B, C, Tin, Tout)
    for dt in DTYPES:
        _pool(ops, c, B, Tin, Tout, C, f32, dt, True, tag)              # sfm_pool_time_affine
        _pool(ops, c, B, Tin, Tout, C, dt, dt, True, tag)               # sfm_pool_time_affine16
    fwd = _pool(ops, c, B, Tin, Tout, C, f32, torch.bfloat16, False, tag)          # sfm_pool_time
    bwd = ops.pool_time_bwd(dev(c["y"]), B, Tin, Tout, C).cpu()
    hp.check_row("pool_time_bwd " + tag, bwd, c["adj64"], c["adj32"], hp.K_SUM)
    x, y = c["srcs"][f32].double(), c["y"].double()
    lhs, rhs = float((fwd.double() * y).sum()), float((x * bwd.double()).sum())
    bound = pc.adjoint_identity_bound(c)
    print("ROW | pool adjoint identity %s | all | <pool x, y> %.9e | <x, pool_bwd y> %.9e | bound %.2e | observed %.2e"
          % (tag, lhs, rhs, bound, abs(lhs - rhs)))
    assert abs(lhs - rhs) <= bound
    xg = dev(c["srcs"][f32]).requires_grad_(True)                        # the autograd node of the path: contiguous rows
    out = train.PoolTimeFunction.apply(xg, Tout)
    (out * dev(c["y"])).sum().backward()
    hp.check_row("PoolTimeFunction forward " + tag, out.detach().cpu(), c["plain64"], c["plain32"], hp.K_SUM)
    hp.check_row("PoolTimeFunction backward " + tag, xg.grad.cpu(), c["adj64"], c["adj32"], hp.K_SUM)
    if Tout == 1:                                                        # glue G2: the mean over the frames and its adjoint
        x64 = c["srcs"][f32].double()
        xg = dev(c["srcs"][f32]).requires_grad_(True)
        m = train.MeanTimeFunction.apply(xg)
        (m * dev(c["y"][:, 0])).sum().backward()
        hp.check_row("MeanTimeFunction forward " + tag, m.detach().cpu(), c["plain64"][:, 0], c["plain32"][:, 0], hp.K_SUM,
                     hp.time_sum_bound(x64, True))           # 64-row partials, then their sum: another order than the row walk
        hp.check_row("MeanTimeFunction backward " + tag, xg.grad.cpu(), c["adj64"], c["adj32"], hp.K_SUM)


@pytest.mark.parametrize("T", pc.POOL_T, ids=_id)
@pytest.mark.parametrize("C", pc.POOL_C)
def test_pool_time(ops, train, C, T):
    """pool_time, pool_time_affine, pool_time_affine16 (fp32, fp16, bf16 sources; dst16 and dst32 of one call), pool_time_bwd,
    train.PoolTimeFunction and - at one output frame - train.MeanTimeFunction against pool64 / pool_adjoint64 at K_SUM x e32;
    B 2 with a different affine for each utterance; NaN in the source's padding columns, sentinels behind the destination's;
    <pool x, y> = <x, pool_bwd y> within pa_nodes_cases.adjoint_identity_bound"""
    _pool_rows(ops, train, 2, T[0], T[1], C)


def test_pool_time_64bit_windows(ops, train):
    """Tin 65536 -> Tout 32769: Tin (Tout + 1) >= 2^31, the window bounds of pool_time_vec_kernel in 64-bit arithmetic"""
    _pool_rows(ops, train, 1, pc.POOL_BIG[0], pc.POOL_BIG[1], 64)
