"""normal_cdf_poly of csrc/sfm_common.h, checked without a GPU: the header's own seven literals, evaluated in float32 with one
rounding per fma, against the float64 erf form over every finite fp16 value and a float32 grid on [-8, 8].  The header states
|error| < 5.7e-5; the 16-bit GELU of gn_apply_rows_kernel and gelu_grad of the GroupNorm backward rest on that figure.
EPS_POLY, the measured maximum, is what the GPU rows of tests/test_pa_nodes_gpu.py allow for the polynomial."""
import numpy as np

import pa_nodes_cases as pc

HEADER_FIGURE = 5.7e-5
EPS_POLY = pc.eps_poly()                             # computed at import from the header's literals


def test_literals_are_the_headers():
    coef, clamp = pc.cdf_literals()
    assert len(coef) == 7 and clamp == 3.75 == pc.SWITCH
    assert all(float(np.float32(c)) == c for c in coef)
    assert abs(coef[-1] - 1.0 / np.sqrt(2.0 * np.pi)) < 3e-4          # the leading term of Phi(z) - 1/2 = z phi(0) + ...
    assert [c > 0 for c in coef] == [True, False, True, False, True, False, True]
    assert float(pc.cdf_poly(np.zeros(1))[0]) == 0.5


def test_polynomial_holds_the_headers_figure():
    fp16, grid = pc.cdf_sweep_points()
    assert fp16.size == 63488 and grid.size >= 10 ** 6 and grid[0] == -8.0 and grid[-1] == 8.0
    worst = 0.0
    for name, z in (("every finite fp16", fp16), ("%d-point float32 grid on [-8, 8]" % grid.size, grid)):
        e, at = pc.cdf_max_error(z)
        print("normal_cdf_poly over %s: max |err| %.4e at z = %.6f" % (name, e, at))
        assert e < HEADER_FIGURE, (name, e, at)
        worst = max(worst, e)
    assert worst == EPS_POLY
    # beyond the clamp the value is that at the clamp: still inside the figure against a CDF that goes on to 0 / 1
    big = np.array([-65504.0, -3.75, 3.75, 65504.0], dtype=np.float32)
    v = pc.cdf_poly(big)
    assert v[0] == v[1] and v[2] == v[3] and 0.0 <= v[0] < HEADER_FIGURE and 1.0 - HEADER_FIGURE < v[2] <= 1.0


def test_a_wrong_coefficient_shows():
    """a sign flip on any one coefficient at least quadruples the sweep's figure: the sweep pins the literals it is given"""
    coef, clamp = pc.cdf_literals()
    _, grid = pc.cdf_sweep_points(200001)
    base = pc.cdf_max_error(grid)[0]
    for i in range(7):
        c = list(coef)
        c[i] = -c[i]
        e = pc.cdf_max_error(grid, tuple(c), clamp)[0]
        print("coefficient %d negated: max |err| %.3e = %.1f x" % (i, e, e / base))
        assert e >= 4.0 * base, (i, e, base)
