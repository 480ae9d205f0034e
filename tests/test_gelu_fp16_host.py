"""The packed-fp16 GELU of conv16p's transform, checked without a GPU: a numpy emulation of the kernel's fp16 operations over
every finite fp16 input against the float64 erf GELU.  This is where the coefficients are pinned."""
import os
import re
import numpy as np

import gelu_fp16_cases as gc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sincformer_metacog_speech_enhancement_amd", "csrc")


def test_coefficients_are_the_kernels():
    """the literals in csrc/conv16p.hip are exactly the fp16 values this file sweeps"""
    src = open(os.path.join(CSRC, "conv16p.hip")).read()
    for i, want in enumerate(gc.COEF):
        m = re.search(r"#define SFM_GELU_H_C%d \(?(-?[0-9.]+)f\)?" % i, src)
        assert m, i
        lit = float(m.group(1))
        assert float(np.float16(lit)) == lit == want, (i, lit, want)
    assert gc.COEF[4] > 0 and gc.COEF[0] > 0            # q grows without bound and starts positive: no clamp, no 0 x inf


def test_emulated_form_over_every_finite_fp16():
    z = gc.finite_fp16()
    assert z.size == 63488
    got = gc.emulate(z)
    z64 = z.astype(np.float64)
    max_abs, max_ulp, z_abs, z_ulp = gc.errors(got, z)
    print("emulated: max |err| %.6e at z = %r; max err %.3f ulps at z = %r" % (max_abs, z_abs, max_ulp, z_ulp))
    z_id, z_zero = gc.thresholds()
    print("identity from z = %r on, zero from z = %r down" % (z_id, z_zero))
    assert 3.0 < z_id < 4.5 and -6.5 < z_zero < -5.0
    assert not np.isnan(got.astype(np.float64)).any()
    assert (got[z64 == 0] == 0).all()
    assert (got[z64 >= z_id] == z[z64 >= z_id]).all()
    assert (got[z64 <= z_zero] == 0).all()
    # the parent's two figures plus one fp16 ulp for the hardware's exp2 and reciprocal (the emulation rounds them exactly)
    exact = gc.gelu64(z)
    err = np.abs(got.astype(np.float64) - exact)
    assert (err <= gc.PARENT_MAX_ABS + gc.ulp16(exact)).all()
    assert max_ulp <= gc.PARENT_MAX_ULP + 1.0
    # and what the fit itself reached (csrc/conv16p.hip quotes these)
    assert max_ulp < 11.9 and max_abs < 1.03e-3


def test_a_wrong_coefficient_shows():
    """one fp16 step on c0 or a sign error on c1 moves the sweep's figures: the sweep pins the coefficients it is given"""
    z = gc.finite_fp16()
    base = gc.errors(gc.emulate(z), z)
    c = list(gc.COEF)
    c[1] = -c[1]
    assert gc.errors(gc.emulate(z, tuple(c)), z)[1] > 4 * base[1]
    c = list(gc.COEF)
    c[0] = float(np.nextafter(np.float16(c[0]), np.float16(10)))
    assert gc.errors(gc.emulate(z, tuple(c)), z)[:2] != base[:2]
