"""The H 128 inference recurrence on fp16 operands (sfm_bilstm_layer_ex with w16: bilstm_layer16_mfma_kernel, four chains of one
direction per workgroup, W_hh on the matrix pipe): accuracy against the fp32 recurrence at batch sizes around the four-chain
group and lengths around the four-step xg ring, independence of a chain from the chains it shares a workgroup with, and that
nothing outside the operands is read into the result or written; the 16-bit-rows form (sfm_bilstm_layer_rows16) against
convert_rows of the fp32 result, and - on the CPU, with a recording _call - that the fused forward takes it only at H 128 with
the fp16-operand switch on.  The kernel tests need a real MI355X: `pytest -m gpu`."""
import ctypes
import math

import pytest
import torch

gpu = pytest.mark.gpu

H = 128
BMAX, TMAX = 9, 130
TOL = 2e-3          # the bound of tests/test_kernels_gpu.py::test_bilstm_layer for the fp16-operand recurrence


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def data():
    """one seeded input projection [BMAX, TMAX, 2, 4H] and recurrent weights [2, 4H, H], the two directions' weights different"""
    g = torch.Generator().manual_seed(20)
    xg = torch.randn(BMAX, TMAX, 2, 4 * H, generator=g)
    whh = torch.randn(2, 4 * H, H, generator=g) / H ** 0.5
    return xg.cuda(), whh.cuda()


def _cut(xg, B, T):
    return xg[:B, :T].contiguous()


# B around the group of four chains (1, 3: idle columns; 4: none; 5, 9: a second / third workgroup with three idle columns);
# T around the four-step ring (1, 2, 3: tail steps only; 7: three tail steps; 21, 130: main loop and one / two tail steps)
CASES = [(B, T) for B in (1, 3, 4, 5, 9) for T in (1, 2, 21)] + [(5, 130), (5, 3), (2, 7)]


@gpu
@pytest.mark.parametrize("B,T", CASES)
def test_against_fp32_recurrence(ops, data, B, T):
    xg, whh = _cut(data[0], B, T), data[1]
    ref = ops.bilstm_layer(xg, whh, B, T, H, w16=False)
    out = ops.bilstm_layer(xg, whh, B, T, H, w16=True)
    assert out.shape == (B, T, 2 * H)
    for d, name in ((0, "forward"), (1, "reverse")):
        o, r = out[:, :, d * H:(d + 1) * H], ref[:, :, d * H:(d + 1) * H]
        e = float((o - r).abs().max())
        print("B %d T %d %s: max|err| %.3e (<= %.0e), ref rms %.3e" % (B, T, name, e, TOL, float(r.pow(2).mean().sqrt())))
        assert math.isfinite(e) and e <= TOL, "%s direction: %.3e > %.0e" % (name, e, TOL)
    # the two directions are different functions of this input: a kernel that ran one of them twice, or the reverse one forwards,
    # is far outside the bound
    assert float((ref[:, :, :H] - ref[:, :, H:]).abs().max()) > 50 * TOL
    if T > 1:
        xr = torch.stack([xg[:, :, 0], xg[:, :, 1].flip(1)], dim=2).contiguous()   # reverse chain fed its input backwards
        wrong = ops.bilstm_layer(xr, whh, B, T, H, w16=False)
        assert float((wrong[:, :, H:] - ref[:, :, H:]).abs().max()) > 50 * TOL
        assert not torch.equal(out, ref)                     # the fp16-operand kernel did run (at T 1 h is 0: no product to round)


@gpu
def test_chain_does_not_depend_on_its_company(ops, data):
    """every chain of a B 5 batch (column 0..3 of the first workgroup, column 0 of the second) bitwise equals the same utterance
    run alone and inside a B 9 batch in another order; a repeated call is bitwise the same"""
    T = 21
    xg9, whh = _cut(data[0], 9, T), data[1]
    out5 = ops.bilstm_layer(xg9[:5].contiguous(), whh, 5, T, H, w16=True)
    again = ops.bilstm_layer(xg9[:5].contiguous(), whh, 5, T, H, w16=True)
    assert torch.equal(out5, again)
    perm = [7, 2, 4, 8, 0, 3, 6, 1, 5]                       # utterance b of the B 5 batch sits at another column here
    out9 = ops.bilstm_layer(xg9[perm].contiguous(), whh, 9, T, H, w16=True)
    for b in range(5):
        alone = ops.bilstm_layer(xg9[b:b + 1].contiguous(), whh, 1, T, H, w16=True)
        assert torch.equal(out5[b], alone[0]), "utterance %d alone" % b
        assert torch.equal(out5[b], out9[perm.index(b)]), "utterance %d at position %d of 9" % (b, perm.index(b))
        assert perm.index(b) != b


@gpu
@pytest.mark.parametrize("B", [5, 1])
def test_reads_and_writes_only_its_operands(ops, data, B):
    """xg and the result are the middle B utterances of larger allocations: NaN around xg must not reach the result, and the
    sentinel around the result must stay"""
    from sincformer_metacog_speech_enhancement_amd import lib
    T, PAD = 21, 2
    whh = data[1]
    xbig = torch.full((PAD + B + PAD, T, 2, 4 * H), float("nan"), device="cuda")
    xbig[PAD:PAD + B] = data[0][:B, :T]
    SENT = -12345.0
    obig = torch.full((PAD + B + PAD, T, 2 * H), SENT, device="cuda")
    xv, ov = xbig[PAD:PAD + B], obig[PAD:PAD + B]
    assert xv.is_contiguous() and ov.is_contiguous()
    L = lib.load()
    rc = L.sfm_bilstm_layer_ex(ctypes.c_void_p(xv.data_ptr()), ctypes.c_void_p(whh.data_ptr()), ctypes.c_void_p(ov.data_ptr()),
                               B, T, H, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ov).all())
    assert bool((obig[:PAD] == SENT).all()) and bool((obig[PAD + B:] == SENT).all())
    assert torch.equal(ov, ops.bilstm_layer(_cut(data[0], B, T), whh, B, T, H, w16=True))


@gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("pad", [0, 24])
def test_rows16_is_convert_rows_of_the_fp32_result(ops, data, dt, pad):
    """the 16-bit rows, also into a destination with a wider row stride, bitwise equal convert_rows of the same kernel's fp32
    result; the columns behind the rows keep their sentinel"""
    B, T = 5, 21
    M = B * T
    ops.set_compute_dtype(dt)
    xg, whh = _cut(data[0], B, T), data[1]
    h32 = ops.bilstm_layer(xg, whh, B, T, H, w16=True)
    want = torch.empty(M, 2 * H, device="cuda", dtype=dt)
    ops.convert_rows(h32, want, M, 2 * H, 2 * H, 2 * H, 2 * H)
    buf = torch.full((M, 2 * H + pad), 7.0, device="cuda", dtype=dt)
    got = ops.bilstm_layer_rows16(xg, whh, B, T, H, out16=buf[:, :2 * H])
    assert got.dtype == dt and got.stride(0) == 2 * H + pad
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool((buf[:, 2 * H:] == 7.0).all())
    assert bool((want.float() - h32.view(M, 2 * H)).abs().max() > 0)      # a rounding did happen
    fresh = ops.bilstm_layer_rows16(xg, whh, B, T, H)                     # the wrapper's own destination
    assert fresh.shape == (M, 2 * H) and torch.equal(fresh.view(torch.int16), want.view(torch.int16))


# ---- routing of the fused forward, on the CPU: the wrappers run against a stub library and a recording _call ------------------
@pytest.fixture
def launches(monkeypatch):
    import ops_stub
    return ops_stub.install(monkeypatch, tags=False)


def _cpea_pack(ops_, Hh, D=64):
    F16 = torch.float16
    pw = lambda N, K: ops_.PackedWeight(torch.zeros(N, K, dtype=F16), torch.zeros(N), N, K, 1, K, False)
    return {"H": Hh, "oc": 8, "heads": pw(32, 2 * Hh),
            "layers": [{"wih": pw(8 * Hh, D), "whh": torch.zeros(2, 4 * Hh, Hh)},
                       {"wih": pw(8 * Hh, 2 * Hh), "whh": torch.zeros(2, 4 * Hh, Hh)}]}


@pytest.mark.parametrize("Hh,w16,rows16", [(128, True, True), (128, False, False), (64, True, False)])
def test_cpea_forward_takes_rows16_only_at_h128_with_the_switch_on(launches, Hh, w16, rows16):
    from sincformer_metacog_speech_enhancement_amd import functional as Fn, ops as ops_
    B, T, D = 2, 3, 64
    ops_.set_lstm_w16(w16)
    try:
        Fn._cpea_forward(torch.zeros(B * T, D, dtype=torch.float16), _cpea_pack(ops_, Hh, D), B, T, None)
    finally:
        ops_.set_lstm_w16(True)
    symbols = [r[0] for r in launches]
    lstm = [r for r in launches if r[1] == "bilstm_layer"]
    assert len(lstm) == 2
    if rows16:
        assert [r[0] for r in lstm] == ["sfm_bilstm_layer_rows16"] * 2 and "sfm_convert_rows" not in symbols
    else:
        assert [r[0] for r in lstm] == ["sfm_bilstm_layer_ex" if w16 else "sfm_bilstm_layer"] * 2
        assert symbols.count("sfm_convert_rows") == 2


def test_rows16_wrapper_states_its_cost(launches):
    from sincformer_metacog_speech_enhancement_amd import ops as ops_
    B, T = 2, 300
    ops_.bilstm_layer_rows16(torch.zeros(B, T, 2, 4 * H), torch.zeros(2, 4 * H, H), B, T, H)
    # the flops of bilstm_layer; xg read in fp32, the rows written in 16 bits: 600 * (1024 * 4 + 256 * 2)
    assert launches == [("sfm_bilstm_layer_rows16", "bilstm_layer", 157286400.0, 2764800)]
