"""Attention as every module runs it: the kernel the DEFAULT rule picks (attention variant 0), the log-sum-exp the pipelined
kernels hand to the backward, and the older training kernels at the lengths and tile edges they are used at.

Every case runs in fp16 and bf16 at head_dim 64; the reference is float64 on the CPU from the 16-bit-rounded operands
(helpers.attn_ref64).  Needs a real MI355X: `pytest -m gpu`."""
import math
import pytest
import torch

from helpers import arr, maxerr, rmse, keep_mask, attn_ref64, ATTN_KERNELS, ATTN_VARIANT_OF, ATTN_RULE_ROWS

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# relative tolerance of one 16-bit rounding of an O(1) value
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HD = 64
# log2-domain LSE against float64: the bounds test_attention_train_fwd_bwd (test_backward_gpu.py) holds the older kernel to
LSE_TOL = {torch.bfloat16: 6e-3, torch.float16: 1e-3}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _reset_variant(ops):
    yield
    ops.set_attention_variant(0)


def q16(x, dt):
    """round to the 16-bit format and back (CPU)"""
    return x.to(dt).float()


def report(name, got, ref, tol):
    e = maxerr(got, ref)
    r = rmse(got, ref)
    print("%-52s max|err| %.3e  rmse %.3e  tol %.1e  ref_rms %.3e" % (name, e, r, tol, float(ref.double().pow(2).mean().sqrt())))
    assert math.isfinite(e) and e <= tol, "%s: max err %.3e > %.1e" % (name, e, tol)


def _forced(ops, variant, qkv16, B, T, H, **kw):
    ops.set_attention_variant(variant)
    try:
        return ops.attention(qkv16, B, T, H, HD, **kw)
    finally:
        ops.set_attention_variant(0)


def _variant_named(ops, B, T, H):
    """the variant that forces the kernel ops.attention_kernel_name names for the default rule; an unknown name is a failure"""
    assert ops.switch("attention_variant") == 0
    name = ops.attention_kernel_name(B, T, H)
    assert name in ATTN_VARIANT_OF, "attention_kernel_name(%d, %d, %d) = %r is no kernel a variant can force" % (B, T, H, name)
    return name, ATTN_VARIANT_OF[name]


# ---------------------------------------------------------------------------
# A. the default rule, in inference
# ---------------------------------------------------------------------------
# Inputs: Q and K ~ N(0, 1.5^2) as in test_attention (scores of std 2.25: peaked rows), V ~ N(0, 0.4^2).  The parity bound
# 6 * EPS is absolute and sized for O(1) values.  These rows have up to 4 M outputs each, and with V at 1.5 the largest |O| is
# 5.2 (float64 reference): rounding a value in [4, 8) to bf16 alone costs up to 4 EPS, which leaves the bound no room for the
# arithmetic (P rounded to 16 bits before P V and the row sum).  With V at 0.4 every |O| is below 2 (1.66 at most; asserted),
# where the output rounding is at most 1 EPS; a float64 emulation of that arithmetic on these inputs (bf16, rows T 230, 256
# and 1024) is 1.02 EPS from the reference.
V_SCALE = 0.4
_RULE_INFO = {}           # (dt, row) -> what the identity check saw at that row (small: names and flags only)


def _rule_row(ops, dt, row):
    """run the row with the variant at 0 (twice) and with each of the variants 1, 4, 5 forced -> (default O, info)"""
    B, H, T, _ = row
    ops.set_compute_dtype(dt)
    qkv = arr("aq", (B * T, 3 * H * HD), 40 + T, 1.5)
    qkv[:, 2 * H * HD:] *= V_SCALE / 1.5
    q16d = qkv.cuda().to(dt).contiguous()
    name, named = _variant_named(ops, B, T, H)
    out = ops.attention(q16d, B, T, H, HD)
    again = ops.attention(q16d, B, T, H, HD)
    forced = {v: _forced(ops, v, q16d, B, T, H) for v in sorted({1, 4, 5} | {named})}
    info = dict(name=name, named=named, repeat=torch.equal(out, again), same_as_named=torch.equal(out, forced[named]),
                differs={v: not torch.equal(forced[v], forced[named]) for v in (1, 4, 5) if v != named},
                same_as={v: torch.equal(out, forced[v]) for v in (1, 4, 5)})
    _RULE_INFO[(dt, row)] = info
    return qkv, out, info


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("row", ATTN_RULE_ROWS, ids=["B%d-H%d-T%d-%s" % r for r in ATTN_RULE_ROWS])
def test_default_rule_launches_the_kernel_it_is_said_to(ops, dt, row):
    """ops.attention with the variant left at 0, on either side of every edge of the rule of attention_fwd_impl: the output
    matches float64, is bitwise the output of the variant that forces the kernel ops.attention_kernel_name names (so the name
    bench.py and the tools print is the kernel that ran), that name is the one worked out by hand from the C rule, and two
    runs give the same bits.  Whether the bits can tell the kernels apart at this row is printed;
    test_default_rule_identity_can_tell_the_kernels_apart asserts that they can where it matters."""
    B, H, T, kern = row
    qkv, out, info = _rule_row(ops, dt, row)
    print("RULE | %s B%d H%d T%d | named %s (variant %d) | default == named: %s | default == v1 / v4 / v5: %s | "
          "other kernels differ from the named one: %s" % (dt, B, H, T, info["name"], info["named"], info["same_as_named"],
                                                            [info["same_as"][v] for v in (1, 4, 5)], info["differs"]))
    ref = attn_ref64(q16(qkv, dt), B, T, H, HD)[0]
    assert float(ref.abs().max()) < 2.0          # the premise of the absolute bound (see V_SCALE)
    report("attention default %s B%d T%d H%d" % (dt, B, T, H), out.float().cpu(), ref, 6 * EPS[dt])
    assert info["name"] == ATTN_KERNELS[kern], "attention_kernel_name says %s, the rule of attention.hip gives %s" % (info["name"], kern)
    assert info["same_as_named"], "the default launch is not bitwise the forced %s" % info["name"]
    assert info["repeat"], "two default runs differ"


@pytest.mark.parametrize("dt", DTYPES)
def test_default_rule_identity_can_tell_the_kernels_apart(ops, dt):
    """the bitwise identity above proves something only at a row where another kernel gives other bits.  Each of the three
    kernels the rule chooses between (variants 1, 4, 5) must be named at a row where one of the other two differs from it; rows
    where none differs are printed and do not count."""
    told = {}
    for row in ATTN_RULE_ROWS:
        info = _RULE_INFO.get((dt, row)) or _rule_row(ops, dt, row)[2]
        apart = sorted(v for v, d in info["differs"].items() if d)
        print("APART | %s B%d H%d T%d | named variant %d | differs from variants %s%s" %
              ((dt,) + row[:3] + (info["named"], apart, "" if apart else "  (this row proves nothing)")))
        if apart and info["same_as_named"]:
            told.setdefault(info["named"], set()).update(apart)
    print("APART | %s | kernel -> kernels it was told apart from: %s" % (dt, {k: sorted(v) for k, v in told.items()}))
    assert set(told) >= {1, 4, 5}, "no row tells variant(s) %s apart from another kernel" % sorted({1, 4, 5} - set(told))


# ---------------------------------------------------------------------------
# B / C. training: O, LSE and the backward fed with them
# ---------------------------------------------------------------------------
def _ulp16(x, dt):
    """spacing of the 16-bit format at |x| (x float32 holding 16-bit values)"""
    _, e = torch.frexp(x.abs().double())
    ulp = torch.ldexp(torch.full_like(x, 2 * EPS[dt], dtype=torch.float64), e - 1)
    return ulp.clamp(min=2.0 ** -24 if dt is torch.float16 else 2.0 ** -133)


def _train_case(ops, dt, B, H, T, p, tag, force_equal=None):
    """forward + LSE + backward of (B, H, T) with dropout p against float64, with the bounds of test_attention_train_fwd_bwd.
    force_equal: a variant whose inference output (pre-scaled Q, same input) must be bitwise the training O"""
    ops.set_compute_dtype(dt)
    seed = 77
    D = H * HD
    qkv = arr("aq", (B * T, 3 * D), 40 + T, 1.0)
    qkv[:, :D] *= 0.35                       # q' ~ pre-scaled magnitude
    dO = arr("ado", (B * T, D), 41 + T, 0.5)
    keep = keep_mask(seed, B, H, T, p) if p > 0 else None
    ref_o, ref_lse, gref = attn_ref64(q16(qkv, dt), B, T, H, HD, prescaled=True, dO=q16(dO, dt), keep=keep)
    q16d = qkv.cuda().to(dt).contiguous()
    O, lse = ops.attention_train(q16d, B, T, H, HD, p_drop=p, seed=seed)
    name = "%s %s B%d H%d T%d p=%.2f" % (tag, str(dt).split(".")[-1], B, H, T, p)
    e_o, e_lse = maxerr(O.float().cpu(), ref_o), maxerr(lse.cpu(), ref_lse)
    print("TRAIN | %s | O max|err| %.3e (bound %.1e) | LSE max|err| %.3e rmse %.3e (bound %.1e)" %
          (name, e_o, 8 * EPS[dt], e_lse, rmse(lse.cpu(), ref_lse), LSE_TOL[dt]))
    same = None
    if force_equal is not None:
        same = torch.equal(O, _forced(ops, force_equal, q16d, B, T, H, prescaled=True))
    dqkv = ops.attention_bwd(q16d, O, dO.cuda().to(dt).contiguous(), lse, B, T, H, HD, p_drop=p, seed=seed).float().cpu()
    assert tuple(lse.shape) == (B, H, T)
    report(name + " O", O.float().cpu(), ref_o, 8 * EPS[dt])
    report(name + " lse", lse.cpu(), ref_lse, LSE_TOL[dt])
    if same is not None:
        assert same, "%s: the training entry point's O is not bitwise the inference O of variant %d" % (name, force_equal)
    scale = float(gref.abs().max())
    tol = 0.03 * scale + 8 * EPS[dt] * scale
    report(name + " dq", dqkv[:, :D], gref[:, :D], tol)
    report(name + " dk", dqkv[:, D:2 * D], gref[:, D:2 * D], tol)
    report(name + " dv", dqkv[:, 2 * D:], gref[:, 2 * D:], tol)
    assert rmse(dqkv, gref) < (0.02 if dt is torch.bfloat16 else 0.004) * float(gref.pow(2).mean().sqrt()) + 1e-6
    return dict(dqkv=dqkv, dO16=q16(dO, dt), gref=gref, tol=tol)


# (B, H, T, kernel): the pipelined rows (at least 128 items inside a window) and, at the same T below the item threshold,
# control rows that take the older kernel
TRAIN_PIPE_ROWS = [(32, 4, 231, "p4"), (32, 4, 256, "p4"), (32, 4, 400, "p8"), (32, 4, 512, "p8"), (16, 4, 799, "p8"),
                   (11, 4, 1025, "p8"), (2, 4, 256, "hd64"), (2, 4, 512, "hd64")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,T,kern", TRAIN_PIPE_ROWS, ids=["B%d-H%d-T%d-%s" % r for r in TRAIN_PIPE_ROWS])
def test_train_forward_lse_of_the_kernel_the_rule_picks(ops, dt, B, H, T, kern):
    """ops.attention_train without dropout where the rule sends it to the pipelined kernels (and control rows at the same T
    that stay on the older kernel): O and every entry of the log2-domain LSE [B, H, T] against float64; O bitwise equal to
    the inference entry point with the named kernel forced (both entry points launch the same kernel, and writing the LSE
    does not change O); ops.attention_bwd fed with this O and this LSE against float64 autograd for dq, dk, dv.

    LSE bounds: 6e-3 (bf16) / 1e-3 (fp16), the ones the older kernel is held to.  The pipelined kernels sum P after rounding
    it to 16 bits (the row sum is an MFMA over the packed P) and subtract the running maximum as two 16-bit terms."""
    name, named = _variant_named(ops, B, T, H)
    assert name == ATTN_KERNELS[kern], (name, kern)
    _train_case(ops, dt, B, H, T, 0.0, "train " + kern, force_equal=named)


# the older training kernels (few items, or dropout): a single key, below / on / above the 64-row tile and the 128-row
# workgroup, more than two workgroups per (batch, head), and the training length T 801 with and without dropout
TRAIN_EDGE_ROWS = [(3, 2, 1, 0.0), (2, 2, 63, 0.0), (2, 2, 64, 0.1), (2, 2, 65, 0.0), (1, 2, 127, 0.0), (1, 2, 128, 0.15),
                   (1, 1, 257, 0.0), (1, 2, 300, 0.1), (1, 4, 801, 0.0), (1, 4, 801, 0.15)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,T,p", TRAIN_EDGE_ROWS, ids=["B%d-H%d-T%d-p%g" % r for r in TRAIN_EDGE_ROWS])
def test_train_forward_backward_at_tile_edges_and_the_training_length(ops, dt, B, H, T, p):
    """attn_fwd_hd64_kernel (with the dropout replica helpers.keep_mask for p > 0), attn_bwd_dq and attn_bwd_dkv against
    float64.  T 1: a single key has probability 1, so dv is dO to one 16-bit rounding step and dq, dk are zero within the
    test's bound."""
    assert ops.attention_kernel_name(B, T, H) == ATTN_KERNELS["hd64"]
    c = _train_case(ops, dt, B, H, T, p, "train edge")
    if T == 1:
        D = H * HD
        dv, dO16 = c["dqkv"][:, 2 * D:], c["dO16"]
        step = float(((dv - dO16).abs().double() / _ulp16(dO16, dt)).max())
        print("T 1: max |dv - dO| = %.3f rounding steps; max |dq| %.3e max |dk| %.3e (bound %.3e)" %
              (step, float(c["dqkv"][:, :D].abs().max()), float(c["dqkv"][:, D:2 * D].abs().max()), c["tol"]))
        assert step <= 1.0, "dv is %.3f 16-bit rounding steps from dO" % step
        assert float(c["gref"][:, :2 * D].abs().max()) <= 1e-12
        assert float(c["dqkv"][:, :2 * D].abs().max()) <= c["tol"]
