"""Mask to waveform without a GPU: the float64 restatement of tests/resynth_cases.py against the reference's recorded output
(tests/golden/g23_resynth.npz), the host-built operands and tables of ops.mask_resynth against that restatement, the argument guards
of sfm_mask_resynth through the built library and of training.resynthesize, the launch cost the wrapper states, and a proof on the CPU
that the bound of tests/test_resynth_gpu.py - 16 x e32 per row - catches plausible wrong kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ops_stub
import resynth_cases as rc
from sincformer_metacog_speech_enhancement_amd import lib, ops, training

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SEED = 900


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "g23_resynth.npz"))


@pytest.fixture(scope="module")
def built():
    from sincformer_metacog_speech_enhancement_amd import build
    build.build(verbose=False)
    return lib.load()


# ---- the restatement against the reference's recorded results ----
def _same_as_float32(r64, g32):
    """the reference returns float32: the float64 restatement lies within half a float32 ulp of it (plus 1e-12 of the largest value)"""
    g = g32.astype(np.float64)
    tol = 0.5 * np.spacing(np.abs(g32)).astype(np.float64) + 1e-12 * max(float(np.abs(g).max()), 1e-30)
    return np.all(np.abs(r64 - g) <= tol)


@pytest.mark.parametrize("i,L", list(enumerate(rc.GOLDEN_LENGTHS)))
def test_restatement_matches_the_fixture(golden, i, L):
    noisy, mask = rc.case("default", L, GOLDEN_SEED + i)
    g = golden["out.%d" % L]
    assert g.dtype == np.float32 and g.shape == (L,)
    assert _same_as_float32(rc.restate64(noisy, mask, "default"), g)
    if L < 160:
        assert not g.any()                                       # hop <= L < frame: the reference itself gives zeros


def test_restatement_matches_the_fixture_with_fewer_mask_rows(golden):
    L, dT = rc.GOLDEN_SHORT
    noisy, mask = rc.case("default", L, GOLDEN_SEED + 20, dT)
    assert mask.shape[0] == rc.frames_of(L, 160, 80) - 2
    g = golden["out.short"]
    assert _same_as_float32(rc.restate64(noisy, mask, "default"), g)
    assert not g[(mask.shape[0] + 1) * 80:].any() and g[mask.shape[0] * 80:(mask.shape[0] + 1) * 80].any()


def test_fixture_inputs_are_the_package_s(golden):
    assert np.array_equal(golden["cf"], rc.center_freqs("default"))
    assert np.array_equal(golden["hann"], np.hanning(160))
    assert np.array_equal(golden["bin_freqs"], np.arange(129) * 4000.0 / 128)
    for f in rc.FRAMINGS:
        rc.check_wsum(f)


# ---- the host-built operands of the kernel ----
def test_interp_table_reproduces_np_interp(golden):
    idx, wt = ops.resynth_interp_table(8000, 256, golden["cf"])
    row = golden["interp.mask"]
    assert idx.min() >= 0 and idx.max() <= 62 and wt.min() >= 0.0 and wt.max() <= 1.0
    assert np.abs((1.0 - wt) * row[idx] + wt * row[idx + 1] - golden["interp.g"]).max() <= 1e-15
    rng = np.random.RandomState(3)
    for fs, n_fft, cf in ((16000, 256, golden["cf"]), (8000, 128, rc.center_freqs("f128")), (8000, 64, np.array([100.0, 700.0, 701.0, 5000.0]))):
        idx, wt = ops.resynth_interp_table(fs, n_fft, cf)
        m = rng.uniform(size=cf.size)
        x = np.arange(n_fft // 2 + 1) * (fs / 2.0) / (n_fft // 2)
        assert np.abs((1.0 - wt) * m[idx] + wt * m[idx + 1] - np.interp(x, cf, m, left=m[0], right=m[-1])).max() <= 1e-15
    idx, wt = ops.resynth_interp_table(16000, 256, golden["cf"])
    assert np.all(idx[129 // 2 + 1:] == 62) and np.all(wt[129 // 2 + 1:] == 1.0)      # bins above 4 kHz take the last channel
    with pytest.raises(ValueError):
        ops.resynth_interp_table(8000, 256, np.array([100.0, 100.0, 200.0]))


def _emulate(noisy, mask, framing):
    """the kernel's arithmetic in float64 on the operands ops.resynth_operands hands it (read back from their fp32 tensors)"""
    frame, hop, n_fft, fs, C = rc.FRAMINGS[framing]
    Wf, Wi, tab_idx, tab_wt, inv = (t.numpy().astype(np.float64) for t in ops.resynth_operands(frame, hop, n_fft, fs, rc.center_freqs(framing), "cpu"))
    NC, FR = ops.round_up(n_fft, ops.RESYNTH_COL_ALIGN), ops.round_up(frame, ops.RESYNTH_COL_ALIGN)
    assert Wf.shape == (FR, NC) and not Wf[frame:].any() and Wi.shape == (NC, FR) and tab_idx.shape == tab_wt.shape == (NC,) and inv.shape == (3, hop)
    assert not Wf[:, n_fft:].any() and not Wi[n_fft:].any() and not Wi[:, frame:].any()
    idx = tab_idx.astype(np.int64)
    assert idx.min() >= 0 and idx.max() <= C - 2
    L = noisy.shape[0]
    N = min(rc.frames_of(L, frame, hop), mask.shape[0])
    out = np.zeros(L)
    if N == 0:
        return out
    x, m = noisy.astype(np.float64), mask.astype(np.float64)
    fr = np.stack([x[n * hop:n * hop + frame] for n in range(N)])
    g = (1.0 - tab_wt) * m[:N][:, idx] + tab_wt * m[:N][:, idx + 1]
    y = ((fr @ Wf[:frame]) * g) @ Wi
    ola = np.zeros((N + 1) * hop)
    for n in range(N):
        ola[n * hop:n * hop + frame] += y[n, :frame]
    scale = np.concatenate([inv[0]] + [inv[1]] * (N - 1) + [inv[2]])
    out[:(N + 1) * hop] = ola * scale
    return out


@pytest.mark.parametrize("name,framing,L,seed,dT", rc.cases(ops.RESYNTH_TILE_FRAMES)[3:])
def test_host_operands_give_the_restatement(name, framing, L, seed, dT):
    """the operands differ from float64 by their cast to fp32 alone: both rows within 4 x e32 of the restatement"""
    noisy, mask, out64, out32 = rc.refs(framing, L, seed, dT)
    for row, o, e32 in rc.row_figures(_emulate(noisy, mask, framing), out64, out32, framing, mask.shape[0]):
        assert o <= 4 * e32, (name, row, o, e32)


# ---- argument guards ----
def test_entry_point_guards_without_a_gpu(built):
    one = ctypes.c_void_p(16)
    ptrs = [one] * 9

    def call(p=ptrs, B=2, L=1237, T=14, frame=160, hop=80, n_fft=256, C=64):
        return built.sfm_mask_resynth(*p, B, L, T, frame, hop, n_fft, C, None)
    for i in range(9):
        if i == 2:
            continue                                             # lengths may be NULL
        assert call(ptrs[:i] + [None] + ptrs[i + 1:]) == -1, i
    assert call(hop=64) == -2                                    # hop * 2 != frame
    assert call(frame=320, hop=160) == -2                        # frame > n_fft
    assert call(frame=128, hop=64, n_fft=255) == -2              # odd n_fft
    assert call(C=65) == -2
    assert call(C=1) == -2
    assert call(frame=512, hop=256, n_fft=512) == -2             # beyond SFM_RESYNTH_MAX_NFFT
    assert call(B=0) == -2 and call(L=0) == -2 and call(T=0) == -2
    assert lib.CONSTANTS["RESYNTH_MAX_NFFT"] == 256 and lib.CONSTANTS["RESYNTH_TILE_FRAMES"] == ops.RESYNTH_TILE_FRAMES


def test_python_guards_raise_value_error():
    noisy, mask = torch.zeros(2, 1237), torch.zeros(2, 14, 64)
    with pytest.raises(ValueError, match="device"):
        training.resynthesize(noisy, mask)                       # host tensors
    with pytest.raises(ValueError, match="2 waveforms, 3 masks"):
        training.resynthesize(noisy, torch.zeros(3, 14, 64))
    with pytest.raises(ValueError, match="63 channels"):
        training.resynthesize(noisy, torch.zeros(2, 14, 63))
    with pytest.raises(ValueError, match="both batched or both single"):
        training.resynthesize(noisy[0], mask)
    with pytest.raises(ValueError, match="fp32"):
        training.resynthesize(noisy.double(), mask)
    with pytest.raises(ValueError, match="ascending"):
        training.resynthesize(noisy, mask[:, :, :3], center_freqs=[100.0, 90.0, 300.0])
    with pytest.raises(ValueError, match="hop \\* 2 == frame"):
        training.resynthesize(noisy, mask, hop=64)
    with pytest.raises(ValueError, match="hop \\* 2 == frame"):
        training.resynthesize(noisy, mask, frame=512, hop=256, n_fft=512)
    assert "resynthesize" in training.__all__ and "dnn_enhance_signal" in training.__all__


# ---- the launch's stated cost (the stub-library pattern of tests/test_launch_costs_host.py) ----
@pytest.fixture
def launches(monkeypatch):
    """[(symbol, family, flops, bytes, tag)] of every launch the wrappers under test enqueue"""
    return ops_stub.install(monkeypatch)


def test_mask_resynth_cost(launches):
    cf = rc.center_freqs("default")
    kw = dict(frame=160, hop=80, n_fft=256, fs=8000, cf=cf)
    noisy, mask = torch.zeros(2, 1237), torch.zeros(2, 14, 64)
    out = ops.mask_resynth(noisy, mask, **kw)
    assert out.shape == (2, 1237) and out.dtype == torch.float32
    ops.mask_resynth(noisy, mask, torch.tensor([1237, 400], dtype=torch.int32), frames=18, **kw)
    # per frame 2 * 160 * 258 + 2 * 258 * 160 = 165120 flops; bytes: noisy 2474 + mask 1792 + Wf 40960 + Wi 40960 + tables 512 + 1 / wsum
    # 240 (+ lengths 2) + out 2474 words
    assert launches == [
        ("sfm_mask_resynth", "resynth", 4623360.0, 357648.0, "B2 L1237 T14 f160 n256 C64"),
        ("sfm_mask_resynth", "resynth", 2972160.0, 357656.0, "B2 L1237 T14 f160 n256 C64"),
    ]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.mask_resynth(noisy, mask, frame=160, hop=64, n_fft=256, fs=8000, cf=cf)


# ---- the bound bites ----
@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_mutants_miss_the_bound(mutant):
    missed = []
    for name, framing, L, seed, dT in rc.cases(ops.RESYNTH_TILE_FRAMES):
        if L > 2000:
            continue
        noisy, mask, out64, out32 = rc.refs(framing, L, seed, dT)
        got = rc.restate64(noisy, mask, framing, mutant)
        frame, hop = rc.FRAMINGS[framing][:2]
        N = min(rc.frames_of(L, frame, hop), mask.shape[0])
        for sel in rc.rows(L, N, frame, hop)[:2]:
            if sel.size and rc.fig(got[sel], out64[sel]) > rc.K * rc.fig(out32[sel], out64[sel]):
                missed.append(name)
    assert missed, mutant
