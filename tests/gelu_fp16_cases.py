"""The packed-fp16 GELU of conv16p's transform (csrc/conv16p.hip, gelu_lg_h2p): every finite fp16 input, the float64 erf GELU it
is measured against, the two error figures, and a numpy emulation of the kernel's sequence of fp16 roundings.  Shared by
tests/test_gelu_fp16_host.py (CPU) and tests/test_conv16p_transform_gpu.py.  Test-side only."""
import math
import numpy as np

# the coefficients of q(a) = c0 + c1 a + c2 a^2 + c3 a^3 + c4 a^4 in  e = 2^(-a q(a)),  as the fp16 bit patterns the kernel's
# literals round to (SFM_GELU_H_C0 .. C4 in csrc/conv16p.hip)
COEF_BITS = (0x40AB, 0xAD27, 0x3163, 0xA4B1, 0x128C)
COEF = tuple(float(np.array([b], dtype=np.uint16).view(np.float16)[0]) for b in COEF_BITS)

# Largest |error| and largest error in fp16 ulps of the exact result of the PARENT commit's transform (A&S 7.1.26 erf in packed
# fp16) over all finite fp16 z, measured on the MI355X by test_conv16p_transform_gpu.py::test_gelu_every_finite_fp16 run against
# the parent's library: profiles/r23/gelu_fp16_sweep.txt.  The new form has to stay at or below both, with no margin.
PARENT_MAX_ABS = 0.0019347484914766788
PARENT_MAX_ULP = 2042.673379380236


def finite_fp16():
    """all 63 488 finite fp16 values (float16 array, in bit-pattern order)"""
    z = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    return z[np.isfinite(z)]


_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def gelu64(z):
    """z Phi(z) in float64 by erfc (no cancellation on the negative side)"""
    z = np.asarray(z, dtype=np.float64)
    return 0.5 * z * _erfc(-z / math.sqrt(2.0))


def ulp16(x):
    """spacing of fp16 at |x| (float64): 2^(e - 10) for normal |x|, 2^-24 below 2^-14"""
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(ax)) - 10)


def errors(got, z):
    """(largest |error|, largest error in fp16 ulps of the exact result, z of each) of fp16 results `got` for fp16 inputs `z`"""
    exact = gelu64(z)
    err = np.abs(np.asarray(got, dtype=np.float64) - exact)
    rel = err / ulp16(exact)
    zz = np.asarray(z, dtype=np.float64)
    return float(err.max()), float(rel.max()), float(zz[int(err.argmax())]), float(zz[int(rel.argmax())])


def thresholds():
    """(z_id, z_zero): the smallest positive fp16 z from which on the float64 GELU rounds to z itself, and the negative fp16 z
    from which on downwards it rounds to zero"""
    z = finite_fp16()
    pos = np.sort(z[z > 0])                                                     # tiny ... 65504
    other = np.nonzero(gelu64(pos).astype(np.float16) != pos)[0]
    neg = np.sort(z[z < 0])[::-1]                                               # -tiny ... -65504
    nonzero = np.nonzero(gelu64(neg).astype(np.float16) != 0)[0]                # (the tiniest inputs round to zero as well)
    return float(pos[other[-1] + 1]), float(neg[nonzero[-1] + 1])


def _r16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def emulate(z, coef=COEF):
    """the kernel's ten packed operations in float64, each rounded to fp16 once (an fma is one operation); exp2 and the
    reciprocal are taken as exact to fp16 rounding"""
    z = np.asarray(z, dtype=np.float16).astype(np.float64)
    c0, c1, c2, c3, c4 = coef
    with np.errstate(all="ignore"):
        a = np.abs(z)                                  # v_and_b32
        q = _r16(a * c4 + c3)                          # v_pk_fma_f16 x 4
        q = _r16(q * a + c2)
        q = _r16(q * a + c1)
        q = _r16(q * a + c0)
        w = _r16(q * -a)                               # v_pk_mul_f16 (neg modifier)
        e = _r16(np.exp2(w))                           # v_exp_f16 x 2
        u = _r16(e + 1.0)                              # v_pk_add_f16
        t = _r16(1.0 / u)                              # v_rcp_f16 x 2
        m = _r16(a * e)                                # v_pk_mul_f16
        r = np.where(np.signbit(z), 0.0, z)            # v_pk_max_i16 on the bit patterns
        return (r - m * t).astype(np.float16)          # v_pk_fma_f16
