"""sfm_conv16p's staging transform (GroupNorm affine + GELU in packed fp16), the row ranges it walks and the bias-started
accumulators, each against a float64 restatement.  Needs a real MI355X: `pytest -m gpu`."""
import math
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gelu_fp16_cases as gc

pytestmark = pytest.mark.gpu

EPS16 = 2.0 ** -11                       # relative tolerance of one fp16 rounding of an O(1) value (tests/test_kernels_gpu.py:17)
TOL = 8 * EPS16                          # the tolerance test_conv16p_normalises_its_input_while_staging uses (test_kernels_gpu.py:318)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def sweep():
    """every finite fp16 value once, as [496, 128] in a fixed shuffled order"""
    z = gc.finite_fp16()
    assert z.size == 496 * 128
    return z[np.random.default_rng(23).permutation(z.size)].reshape(496, 128)


def _check_gelu(name, got, z):
    """got: fp16 results of the transform for the fp16 inputs z (numpy, any shape)"""
    got, z = got.reshape(-1), z.reshape(-1)
    z64 = z.astype(np.float64)
    max_abs, max_ulp, z_abs, z_ulp = gc.errors(got, z)
    print("GELU_SWEEP %s: max |err| %.6e at z = %r; max err %.3f fp16 ulps of the exact result at z = %r" % (name, max_abs, z_abs,
                                                                                                              max_ulp, z_ulp))
    z_id, z_zero = gc.thresholds()
    print("GELU_SWEEP %s: identity from z = %r on, zero from z = %r down" % (name, z_id, z_zero))
    assert not np.isnan(got.astype(np.float64)).any()
    assert (got[z64 == 0] == 0).all()
    big = z64 >= z_id
    assert (got[big] == z[big]).all()
    assert (got[z64 <= z_zero] == 0).all()
    assert max_abs <= gc.PARENT_MAX_ABS and max_ulp <= gc.PARENT_MAX_ULP, (max_abs, max_ulp)


def test_gelu_every_finite_fp16(ops, sweep):
    """k 3 conv whose only non-zero weight is 1 at (centre tap, c = n), zero bias, unit scale, zero shift: out[l, c] is the
    transform of x1[l, c] bit for bit (one product with 1.0, the rest zeros: the MFMA sum is exact)"""
    ops.set_compute_dtype(torch.float16)
    w = torch.zeros(128, 128, 3)
    w[torch.arange(128), torch.arange(128), 1] = 1.0
    pw = ops.pack_linear(w.cuda(), torch.zeros(128).cuda())
    x1 = torch.from_numpy(sweep.copy()).reshape(1, 496, 128).cuda()
    out = torch.full((1, 496, 128), float("nan"), device="cuda", dtype=torch.float16)
    ops.conv16p(x1, torch.ones(1, 128).cuda(), torch.zeros(1, 128).cuda(), pw, out, B=1, Lin=496, stride=1, pad=1)
    _check_gelu("one input", out.cpu().numpy()[0], sweep)


def test_gelu_two_input_form(ops, sweep):
    """k 1 stride 2, two inputs: z = x1 + 0.5 x2 + (0.125 + 0.125) in fp32, rounded to fp16 once.  x2 is a multiple of 0.25 in
    [-2, 2], so the fp32 affine is exact wherever its fp16 rounding could tie.  The odd input rows hold NaN: the stride skips them"""
    ops.set_compute_dtype(torch.float16)
    w = torch.zeros(256, 128, 1)
    w[torch.arange(128), torch.arange(128), 0] = 1.0
    pw = ops.pack_linear(w.cuda(), torch.zeros(256).cuda())
    x2e = (np.random.default_rng(24).integers(-8, 9, size=sweep.shape) * 0.25).astype(np.float16)
    x1 = np.full((992, 128), np.nan, dtype=np.float16)
    x2 = np.full((992, 128), np.nan, dtype=np.float16)
    x1[0::2], x2[0::2] = sweep, x2e
    t0 = x2e.astype(np.float32) * np.float32(0.5) + (np.float32(0.125) + np.float32(0.125))
    z = (sweep.astype(np.float32) * np.float32(1.0) + t0).astype(np.float16)
    assert np.isfinite(z).all()
    out = torch.full((1, 496, 256), float("nan"), device="cuda", dtype=torch.float16)
    c = lambda v: torch.full((1, 128), v, device="cuda")
    ops.conv16p(torch.from_numpy(x1).reshape(1, 992, 128).cuda(), c(1.0), c(0.125), pw, out, B=1, Lin=992, stride=2, pad=0,
                x2=torch.from_numpy(x2).reshape(1, 992, 128).cuda(), sc2=c(0.5), sh2=c(0.125))
    got = out.cpu().numpy()[0]
    assert (got[:, 128:] == 0).all()
    _check_gelu("two inputs", got[:, :128], z)


# ---------------------------------------------------------------------------
def _conv_ref64(x1, sc1, sh1, x2, sc2, sh2, w, b, stride, pad):
    """float64 conv of the operand the kernel stages: z = fp32 affine rounded to fp16, exact GELU rounded to fp16, fp16 weights"""
    z = x1.half().float() * sc1[:, None, :] + sh1[:, None, :]
    if x2 is not None:
        z = z + x2.half().float() * sc2[:, None, :] + sh2[:, None, :]
    z16 = z.half()
    xn = torch.from_numpy(gc.gelu64(z16.numpy())).half().double().transpose(1, 2)
    return F.conv1d(xn, w.half().double(), b.double(), stride=stride, padding=pad).transpose(1, 2)


def _run(ops, x1, sc1, sh1, x2, sc2, sh2, w, b, ws, bs, stride, pad, G=16):
    B, Lin, cin = x1.shape
    cout, _, k = w.shape
    Lout = (Lin + 2 * pad - k) // stride + 1
    P = 2 * ((Lout + 127) // 128)
    d = lambda t: None if t is None else t.cuda().contiguous()
    h = lambda t: None if t is None else t.cuda().half().contiguous()
    pw = ops.pack_linear(d(w), d(b))
    spw = ops.pack_linear(d(ws), d(bs)) if ws is not None else None
    out = torch.full((B, Lout, cout), float("nan"), device="cuda")
    part = torch.zeros(B, P, G, 2, device="cuda")
    out_s = torch.full((B, Lout, cout), float("nan"), device="cuda") if ws is not None else None
    part_s = torch.zeros(B, P, G, 2, device="cuda") if ws is not None else None
    ops.conv16p(h(x1), d(sc1), d(sh1), pw, out, B=B, Lin=Lin, stride=stride, pad=pad, x2=h(x2), sc2=d(sc2), sh2=d(sh2),
                gn_partial=part, gn_group=cout // G, skip_pw=spw, out_s=out_s, gn_partial_s=part_s)
    return out, part, out_s, part_s


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)) * scale


@pytest.mark.parametrize("Lin", [1, 2, 127, 128, 129, 255, 257])
@pytest.mark.parametrize("k,pad,cout,two,skip", [(7, 3, 128, False, True), (5, 2, 256, True, False)])
def test_rows_transformed_and_rows_left_zero(ops, k, pad, cout, two, skip, Lin):
    """the transform walks exactly the input rows inside [0, Lin).  (a) random weights against the float64 restatement;
    (b) x = 0, shift 1e3, weights in {-1, 0, 1}: every staged value is exactly 1000 and every sum an integer below 2^24, so the
    fp32 result must EQUAL the float64 one; a padding row transformed by mistake would add GELU(1e3) = 1e3 times its weights"""
    ops.set_compute_dtype(torch.float16)
    B, cin = 2, 128
    x1 = _rand((B, Lin, cin), 30 + Lin)
    x2 = _rand((B, Lin, cin), 31 + Lin) if two else None
    sc1, sh1 = _rand((B, cin), 32, 0.2) + 1.0, _rand((B, cin), 33, 0.3)
    sc2, sh2 = (_rand((B, cin), 34, 0.2) + 0.7, _rand((B, cin), 35, 0.3)) if two else (None, None)
    w, b = _rand((cout, cin, k), 36, 1.0 / math.sqrt(cin * k)), _rand((cout,), 37)
    ws, bs = (_rand((cout, cin, 1), 38, 1.0 / math.sqrt(cin)), _rand((cout,), 39)) if skip else (None, None)
    out, _, out_s, _ = _run(ops, x1, sc1, sh1, x2, sc2, sh2, w, b, ws, bs, 2, pad)
    ref = _conv_ref64(x1, sc1, sh1, x2, sc2, sh2, w, b, 2, pad)
    err = float((out.cpu().double() - ref).abs().max())
    print("rows k%d Lin %d: max |err| %.3e (tol %.1e)" % (k, Lin, err, TOL))
    assert math.isfinite(err) and err <= TOL
    if skip:
        refs = _conv_ref64(x1, sc1, sh1, None, None, None, ws, bs, 2, 0)
        errs = float((out_s.cpu().double() - refs).abs().max())
        assert math.isfinite(errs) and errs <= TOL
    # (b)
    zero, one = torch.zeros(B, Lin, cin), torch.ones(B, cin)
    wi = torch.from_numpy(np.random.default_rng(40).integers(-1, 2, size=(cout, cin, k)).astype(np.float32))
    wsi = torch.from_numpy(np.random.default_rng(41).integers(-1, 2, size=(cout, cin, 1)).astype(np.float32)) if skip else None
    bi = torch.zeros(cout)
    sh = (one * 1e3, one * 0.0) if two else (one * 1e3, None)
    out, _, out_s, _ = _run(ops, zero, one, sh[0], zero if two else None, one if two else None, sh[1], wi, bi, wsi,
                            bi if skip else None, 2, pad)
    ref = _conv_ref64(zero, one, sh[0], zero if two else None, one if two else None, sh[1], wi, bi, 2, pad)
    assert torch.equal(out.cpu().double(), ref)
    if skip:
        assert torch.equal(out_s.cpu().double(), _conv_ref64(zero, one, sh[0], None, None, None, wsi, bi, 2, 0))


# every (k, stride, pad, N, inputs, skip) combination sfm_conv16p is built for
COMBOS = [(7, 2, 3, 128, False, True), (7, 2, 3, 128, True, True), (7, 2, 3, 256, True, False), (3, 1, 1, 128, False, False),
          (3, 1, 1, 256, False, False), (5, 2, 2, 256, True, False), (1, 2, 0, 256, True, False)]


@pytest.mark.parametrize("Lout", [1, 64, 65, 128, 129])
@pytest.mark.parametrize("k,s,pad,cout,two,skip", COMBOS)
def test_accumulators_started_from_the_bias(ops, k, s, pad, cout, two, skip, Lout):
    """bias ~ N(0, 1): raw outputs against the float64 restatement; the GroupNorm partial sums against the float64 sums of the
    fp32 outputs of the same launch (the bound of test_conv16p_statistics_and_determinism_at_scale, test_kernels_gpu.py:369-370);
    two launches bit for bit"""
    ops.set_compute_dtype(torch.float16)
    B, cin, G = 2, 128, 16
    Lin = (Lout - 1) * s + k - 2 * pad
    if Lin < 1:                                        # Lout 1 at k 3 stride 1 pad 1
        Lin = 1
    assert (Lin + 2 * pad - k) // s + 1 == Lout
    x1 = _rand((B, Lin, cin), 50 + Lout)
    x2 = _rand((B, Lin, cin), 51 + Lout) if two else None
    sc1, sh1 = _rand((B, cin), 52, 0.2) + 1.0, _rand((B, cin), 53, 0.3)
    sc2, sh2 = (_rand((B, cin), 54, 0.2) + 0.7, _rand((B, cin), 55, 0.3)) if two else (None, None)
    w, b = _rand((cout, cin, k), 56, 1.0 / math.sqrt(cin * k)), _rand((cout,), 57)
    ws, bs = (_rand((cout, cin, 1), 58, 1.0 / math.sqrt(cin)), _rand((cout,), 59)) if skip else (None, None)
    first = _run(ops, x1, sc1, sh1, x2, sc2, sh2, w, b, ws, bs, s, pad, G)
    second = _run(ops, x1, sc1, sh1, x2, sc2, sh2, w, b, ws, bs, s, pad, G)
    for t1, t2 in zip(first, second):
        assert (t1 is None and t2 is None) or torch.equal(t1, t2)
    refs = [_conv_ref64(x1, sc1, sh1, x2, sc2, sh2, w, b, s, pad)]
    if skip:
        refs.append(_conv_ref64(x1, sc1, sh1, x2, sc2, sh2, ws, bs, 2, 0))
    P = 2 * ((Lout + 127) // 128)
    for ref, out, part in zip(refs, first[0::2], first[1::2]):
        err = float((out.cpu().double() - ref).abs().max())
        print("bias start k%d s%d N%d in%d Lout %d: max |err| %.3e (tol %.1e)" % (k, s, cout, 2 if two else 1, Lout, err, TOL))
        assert math.isfinite(err) and err <= TOL
        rows = torch.cat([out.double(), torch.zeros(B, P * 64 - Lout, cout, device="cuda", dtype=torch.float64)], dim=1)
        rows = rows.reshape(B, P, 64, G, cout // G)
        want = torch.stack([rows.sum(dim=(2, 4)), (rows ** 2).sum(dim=(2, 4))], dim=-1)
        perr = float(((part.double() - want).abs() / (1.0 + want.abs())).max())
        assert perr < 1e-4, perr
