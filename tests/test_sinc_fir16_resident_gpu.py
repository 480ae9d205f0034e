"""The one-pass sinc FIR with the taps resident in registers (sinc_fir16_resident_kernel) against the streaming one-pass kernel
it replaces (bit for bit: out and the whole gn_partial tensor) and against the fp32 conv of the oracle (the one-pass bound of
tests/test_kernels_gpu.py::test_sinc_fir16_split_mfma), with guard rows behind the output and the partial slots past L.

Lengths: one sample, less than a row group, the edges of a 256-sample wave-tile, of a 1024-sample span (the resident kernel's
staging unit), of a 2048-sample sub-tile and of the 8192-sample chunk of the streaming kernel, a length that ends inside a
span, and 33 000 samples: at B = 2 the first length whose spans are walked by two workgroups per (utterance, shift)."""
import math
import pytest
import torch

from helpers import arr, maxerr
from oracle import sfm_oracle as orc

pytestmark = pytest.mark.gpu

B = 2
FS = 16000
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LENGTHS = [1, 7, 255, 256, 257, 1024 + 3, 2048, 2048 + 5, 8192, 8193, 20011, 33000]
CASES = [(L, 251) for L in LENGTHS] + [(L, K) for K in (31, 265) for L in (257, 2048 + 5, 8193)]
GUARD = 4 * 64                      # sentinel elements behind the last utterance: four rows
SENTINEL = 123.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _reset(ops):
    yield
    ops.set_sinc_fir_resident(True)
    ops.reset_precision()


_REF = {}


def _reference(L, K):
    """(waveform [B, L], filters [64, K], fp32 conv [B, 64, L]) - computed once per (L, K), shared by the dtype / output cases"""
    if (L, K) not in _REF:
        p = orc.sinc_init(64, K, FS)
        filt = orc.sinc_filters(p["low_hz_"] * (FS / 8.0), p["band_hz_"] * (FS / 8.0), p["window"], p["n_"], FS).contiguous()
        x = arr("firx", (B, L), 23, 0.3)
        _REF[(L, K)] = (x, filt, orc.sinc_conv(x, filt))
    return _REF[(L, K)]


def _run(ops, x, filt, L, K, out_dt):
    buf = torch.full((B * L * 64 + GUARD,), SENTINEL, device="cuda", dtype=out_dt)
    out = buf[:B * L * 64].view(B, L, 64)
    part, P = ops.sinc_fir16(x, filt, out, B, L, 64, K, passes=1)
    torch.cuda.synchronize()
    return buf, out, part, P


@pytest.mark.parametrize("out32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("L,K", CASES, ids=["L%d-K%d" % c for c in CASES])
def test_resident_equals_streaming_and_meets_the_one_pass_bound(ops, L, K, dt, out32):
    ops.set_compute_dtype(dt)
    x, filt, ref = _reference(L, K)
    xd, fd = x.cuda(), filt.cuda()
    out_dt = torch.float32 if out32 else dt
    assert ops.switch("sinc_fir_resident") is True
    buf, out, part, P = _run(ops, xd, fd, L, K, out_dt)
    ops.set_sinc_fir_resident(False)
    sbuf, sout, spart, sP = _run(ops, xd, fd, L, K, out_dt)
    ops.set_sinc_fir_resident(True)

    # bitwise against the streaming kernel: the result and every GroupNorm partial
    assert P == sP and part.shape == spart.shape
    assert torch.equal(out, sout)
    assert torch.equal(part, spart)
    # the one-pass bound against the fp32 conv
    e = maxerr(out.float().cpu().transpose(1, 2), ref)
    tol = 4 * EPS[dt] * 0.1
    print("sinc fir16 resident L%d K%d %s out %s: max|err| %.3e tol %.1e" % (L, K, dt, out_dt, e, tol))
    assert math.isfinite(e) and e <= tol
    # guard rows behind the last utterance are intact (both kernels)
    assert bool((buf[B * L * 64:] == SENTINEL).all()) and bool((sbuf[B * L * 64:] == SENTINEL).all())
    # partial slots of wave-tiles past L are zero: tile g = sample / 256 of shift o has slot (g / 8) * 64 + o * 8 + g % 8
    used = torch.zeros(P, dtype=torch.bool)
    for g in range((L + 255) // 256):
        for o in range(8):
            used[(g // 8) * 64 + o * 8 + g % 8] = True
    assert P == used.numel() and bool((part[:, ~used.cuda()] == 0).all())
    assert bool(part[:, used.cuda(), :, 1].sum() > 0)          # ... and the slots of the tiles inside L carry the sums


def test_auto_choice_and_switch_route_the_one_pass_kernels(ops):
    """passes = 0 with fp16 operands and a 16-bit result is the one-pass product, with the switch on or off"""
    ops.set_compute_dtype(torch.float16)
    L, K = 2048 + 5, 251
    x, filt, _ = _reference(L, K)
    xd, fd = x.cuda(), filt.cuda()
    one = torch.empty(B, L, 64, device="cuda", dtype=torch.float16)
    ops.sinc_fir16(xd, fd, one, B, L, 64, K, passes=1)
    for flag in (True, False):
        ops.set_sinc_fir_resident(flag)
        auto = torch.empty_like(one)
        ops.sinc_fir16(xd, fd, auto, B, L, 64, K)
        assert torch.equal(auto, one), flag
        assert ops.variant_overrides() == ({} if flag else {"sinc_fir_resident": False})
