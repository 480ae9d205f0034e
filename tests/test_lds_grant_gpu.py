"""The dynamic-LDS grant of a kernel whose LDS size depends on a run-time argument grows with it: small first, large second.

The grant is state of the process, so each case runs in a fresh child (this file run as a script): inside the pytest process
an earlier test may already have raised it.  References and bounds are those of test_ffn_fused / test_dwconv_folded.
Needs a real MI355X: `pytest -m gpu`."""
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_ffn_fused(dt):
    """M 130 (two row tiles, the second partial); FF 64 (147 712 B of LDS), then FF 1024 (151 552 B)"""
    M, D = 130, 256
    for FF in (64, 1024):
        x = arr("ffx", (M, D), 91, 1.5) + 0.2
        lw, lb = arr("fflw", (D,), 92) * 0.1 + 1.0, arr("fflb", (D,), 93) * 0.1
        w1, b1 = arr("ffw1", (FF, D), 94) / 16.0, arr("ffb1", (FF,), 95) * 0.1
        w2, b2 = arr("ffw2", (D, FF), 96) / math.sqrt(FF), arr("ffb2", (D,), 97) * 0.1
        out = ops.ffn_fused(dev(x), dev(lw), dev(lb), dev(w1).to(dt).contiguous(), dev(b1), dev(w2).to(dt).contiguous(), dev(b2))
        h = q16(orc.layer_norm(x, lw, lb), dt)
        u = q16(orc.swish(h @ q16(w1, dt).t() + b1), dt)
        ref = x + 0.5 * (u @ q16(w2, dt).t() + b2)
        r = rmse(out.cpu(), ref)
        print("ffn fused %s M%d FF%d  max|err| %.3e  rmse %.3e  bound %.1e" % (dt, M, FF, maxerr(out.cpu(), ref), r, EPS[dt]))
        assert math.isfinite(r) and r < EPS[dt]


def child_dwconv_folded(dt):
    """k 31 (fp16: the dot kernel, bf16: the multiply-add kernel), B 2, T 70 (two 64-frame tiles); C 64 (12 032 B), then C 512 (96 256 B)"""
    B, T, KS = 2, 70, 31
    for C in (64, 512):
        x = arr("dx", (B, T, C), 60)
        w, b = arr("dw", (C, 1, KS), 61) / math.sqrt(KS), arr("db", (C,), 62) * 0.1
        bw, bb = arr("dbw", (C,), 63) * 0.1 + 1, arr("dbb", (C,), 64) * 0.1
        rm, rv = arr("drm", (C,), 65) * 0.1, torch.rand(C, generator=torch.Generator().manual_seed(1)) + 0.5
        sc = bw / torch.sqrt(rv + 1e-5)
        sh = bb - rm * sc + b * sc
        out = ops.dwconv_folded(dev(x).to(dt).contiguous(), dev(w.reshape(C, KS).t().contiguous()), dev(sc), dev(sh), B, T, C)
        h = F.conv1d(q16(x, dt).transpose(1, 2), w, b, padding=(KS - 1) // 2, groups=C)
        ref = orc.swish(orc.batch_norm_eval(h, bw, bb, rm, rv)).transpose(1, 2)
        report("dwconv folded %s C%d k%d T%d" % (dt, C, KS, T), out.float().cpu(), ref, 8 * EPS[dt])


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("case", ["ffn_fused", "dwconv_folded"])
def test_grant_grows_with_the_launch(case, dt):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, dt], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, "%s %s: exit status %d\n%s\n%s" % (case, dt, r.returncode, r.stdout, r.stderr)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import torch.nn.functional as F
    from helpers import arr, maxerr, rmse
    from oracle import sfm_oracle as orc
    from sincformer_metacog_speech_enhancement_amd import ops
    from test_kernels_gpu import EPS, dev, q16, report
    dtype = getattr(torch, sys.argv[2])
    ops.set_compute_dtype(dtype)
    {"ffn_fused": child_ffn_fused, "dwconv_folded": child_dwconv_folded}[sys.argv[1]](dtype)
