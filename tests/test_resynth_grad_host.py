"""The resynthesis' adjoint in the mask without a GPU: the float64 cotangent of tests/resynth_grad_cases.py against the forward's
restatement (the adjoint identity and unit masks: rc.restate64 is pinned to the reference's recorded output by g23_resynth.npz, and
these pin grad64 to it), a proof that plausible wrong adjoints break that identity by far more than the GPU rows' bound, the
channel-range table and the transposed operand that ops hands the kernel, the entry point's guards through the built library, the
launch cost the wrapper states and the refusal of a gradient to the noisy signal."""
import ctypes

import numpy as np
import pytest
import torch

import ops_stub
import resynth_cases as rc
import resynth_grad_cases as gc
from sincformer_metacog_speech_enhancement_amd import lib, ops, training

LENGTHS = (160, 241, 1237)
D_T = (0, -2, 1)


def _inputs(framing, L, dT, seed):
    """(noisy, dout, T_mask, N) - T_mask = T + dT, at least 1"""
    frame, hop = rc.FRAMINGS[framing][:2]
    noisy, mask = rc.case(framing, L, seed, dT)
    T_mask = mask.shape[0]
    N = min(rc.frames_of(L, frame, hop), T_mask)
    return noisy, gc.dout_of(L, seed, N, hop), T_mask, N


def _masks(T_mask, C, seed):
    rng = np.random.RandomState(seed)
    return [rng.uniform(0.0, 1.0, size=(T_mask, C)), rng.standard_normal((T_mask, C)), rng.uniform(-3.0, 3.0, size=(T_mask, C))]


@pytest.mark.parametrize("framing", ["default", "fs16k", "f128"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dT", D_T)
def test_adjoint_identity(framing, L, dT):
    """<dout, restate64(noisy, m)> == <grad64, m> within 1e-12 relative for three random masks; the NaN tail of dout counts as zeros
    on the left side only: grad64 itself never reads it"""
    noisy, dout, T_mask, N = _inputs(framing, L, dT, 1000 + L + dT)
    g = gc.grad64(noisy, dout, framing, T_mask)
    assert np.isfinite(g).all() and not g[N:].any() and g[:N].any()
    for m in _masks(T_mask, g.shape[1], L + dT):
        assert gc.identity_gap(noisy, dout, m, g, framing) <= 1e-12, (framing, L, dT)


@pytest.mark.parametrize("framing", ["default", "fs16k", "f128"])
def test_unit_masks(framing):
    """grad64[n, c] == <dout, restate64(noisy, e_{n, c})>: frame 0, frame N - 1, an interior frame, channel 0, channel C - 1, and a
    channel that brackets no bin (the default bank at 16 kHz has seven), whose gradient is exactly 0"""
    L = 1237
    noisy, dout, T_mask, N = _inputs(framing, L, 0, 1100)
    C = rc.FRAMINGS[framing][4]
    g = gc.grad64(noisy, dout, framing, T_mask)
    lo, _ = rc.interp_table(framing)
    touched = np.zeros(C, dtype=bool)
    touched[lo] = touched[lo + 1] = True
    dead = np.flatnonzero(~touched)
    assert not g[:, dead].any()
    if framing == "fs16k":
        F = 129
        assert dead.size >= 2 and dead.max() < C // 2           # bins 62.5 Hz apart: several low channels lie between two bins
        assert np.all(lo[F // 2 + 1:] == C - 2)                 # every bin above 4 kHz falls on the last channel
    else:
        assert dead.size == 0                                   # (at 8 kHz every channel of both banks brackets a bin)
    d = np.nan_to_num(dout.astype(np.float64), nan=0.0)
    scale = np.abs(g).max()
    chans = [0, C - 1, C // 2] + ([int(dead[0])] if dead.size else [])
    for n in (0, N - 1, N // 2):
        for c in chans:
            e = np.zeros((T_mask, C))
            e[n, c] = 1.0
            want = float((d * rc.restate64(noisy, e, framing)).sum())
            assert abs(g[n, c] - want) <= 1e-12 * scale, (n, c, g[n, c], want)
            if dead.size and c == dead[0]:
                assert g[n, c] == 0.0 and want == 0.0


@pytest.mark.parametrize("mutant", gc.MUTANTS)
def test_mutants_break_the_identity(mutant):
    """every mutant misses the identity by more than 100 x the GPU rows' bound (16 x e32 of the case's worse row) in some case"""
    worst = 0.0
    for framing in ("default", "fs16k", "f128"):
        for L in LENGTHS[1:]:
            for dT in D_T:
                noisy, dout, T_mask, N = _inputs(framing, L, dT, 1000 + L + dT)
                g64 = gc.grad64(noisy, dout, framing, T_mask)
                e32 = max(e for _, _, e in gc.row_figures(g64, g64, gc.grad32(noisy, dout, framing, T_mask), N))
                gm = gc.grad64(noisy, dout, framing, T_mask, mutant)
                m = _masks(T_mask, g64.shape[1], 7)[0]
                gap = gc.identity_gap(noisy, dout, m, gm, framing)
                assert gc.identity_gap(noisy, dout, m, g64, framing) <= 1e-12
                worst = max(worst, gap / (gc.K * e32)) if np.isfinite(gap) else np.inf
    assert worst > 100.0, (mutant, worst)


# ---- the operands ops adds for the adjoint ----
@pytest.mark.parametrize("framing", ["default", "fs16k", "f128"])
def test_channel_bins_are_the_inverse_of_the_interp_table(framing):
    frame, hop, n_fft, fs, C = rc.FRAMINGS[framing]
    F = n_fft // 2 + 1
    idx, _ = ops.resynth_interp_table(fs, n_fft, rc.center_freqs(framing))
    bins = ops.resynth_channel_bins(idx, C)
    assert bins.dtype == np.int32 and bins.shape == (C + 1,) and bins[0] == 0 and bins[C - 1] == F and bins[C] == F
    assert np.all(np.diff(bins) >= 0)                            # the ranges ascend and each ends where the next begins
    owner = np.full(F, -1)
    for c in range(C):
        assert np.all(owner[bins[c]:bins[c + 1]] == -1)          # every bin sits in exactly one lower range
        owner[bins[c]:bins[c + 1]] = c
    assert np.array_equal(owner, idx)
    seven = ops.resynth_operands(frame, hop, n_fft, fs, rc.center_freqs(framing), "cpu", bwd=True)
    five = ops.resynth_operands(frame, hop, n_fft, fs, rc.center_freqs(framing), "cpu")
    assert len(five) == 5 and len(seven) == 7 and all(a is b for a, b in zip(five, seven))
    Wi, WiT, dev_bins = seven[1], seven[5], seven[6]
    NC, FR = ops.round_up(n_fft, ops.RESYNTH_COL_ALIGN), ops.round_up(frame, ops.RESYNTH_COL_ALIGN)
    assert WiT.shape == (FR, NC) and WiT.is_contiguous() and WiT.dtype == torch.float32 and torch.equal(WiT, Wi.t())
    assert dev_bins.dtype == torch.int32 and np.array_equal(dev_bins.numpy(), bins)
    with pytest.raises(ValueError):
        ops.resynth_channel_bins(np.array([0, 2, 1]), 4)
    with pytest.raises(ValueError):
        ops.resynth_channel_bins(np.array([0, 1, 3]), 4)


def _emulate(noisy, dout, framing, T_mask):
    """the kernel's arithmetic in float64 on the operands ops.resynth_operands hands it (read back from their fp32 tensors)"""
    frame, hop, n_fft, fs, C = rc.FRAMINGS[framing]
    F = n_fft // 2 + 1
    Wf, _, _, tab_wt, inv, WiT, bins = (t.numpy().astype(np.float64) for t in
                                        ops.resynth_operands(frame, hop, n_fft, fs, rc.center_freqs(framing), "cpu", bwd=True))
    bins = bins.astype(np.int64)
    L = noisy.shape[0]
    N = min(rc.frames_of(L, frame, hop), T_mask)
    out = np.zeros((T_mask, C))
    if N == 0:
        return out
    x, d = noisy.astype(np.float64), dout.astype(np.float64)[:(N + 1) * hop]
    scale = np.concatenate([inv[0]] + [inv[1]] * (N - 1) + [inv[2]])
    dy = (d * scale).reshape(N + 1, hop)
    fr = np.stack([x[n * hop:n * hop + frame] for n in range(N)])
    P = (fr @ Wf[:frame]) * (np.concatenate([dy[:N], dy[1:]], axis=1) @ WiT[:frame])
    dg = P[:, :F].copy()
    dg[:, 1:F - 1] += P[:, F:n_fft]
    for c in range(C):
        if c > 0:
            k = slice(bins[c - 1], bins[c])
            out[:N, c] += dg[:, k] @ tab_wt[k]
        k = slice(bins[c], bins[c + 1])
        out[:N, c] += dg[:, k] @ (1.0 - tab_wt[k])
    return out


@pytest.mark.parametrize("name,framing,L,seed,dT", rc.cases(ops.RESYNTH_BWD_TILE_FRAMES)[3:])
def test_host_operands_give_the_cotangent(name, framing, L, seed, dT):
    """the operands differ from float64 by their cast to fp32 alone: both rows within 4 x e32 of grad64"""
    noisy, dout, T_mask, g64, g32 = gc.refs(framing, L, seed, dT)
    N = min(rc.frames_of(L, *rc.FRAMINGS[framing][:2]), T_mask)
    for row, o, e32 in gc.row_figures(_emulate(noisy, dout, framing, T_mask), g64, g32, N):
        assert o <= 4 * e32, (name, row, o, e32)


# ---- guards, cost, refusals ----
def test_entry_point_guards_without_a_gpu():
    from sincformer_metacog_speech_enhancement_amd import build
    build.build(verbose=False)
    built = lib.load()
    one = ctypes.c_void_p(16)
    ptrs = [one] * 9

    def call(p=ptrs, B=2, L=1237, T=14, frame=160, hop=80, n_fft=256, C=64):
        return built.sfm_mask_resynth_bwd(*p, B, L, T, frame, hop, n_fft, C, None)
    for i in range(9):
        if i == 2:
            continue                                             # lengths may be NULL
        assert call(ptrs[:i] + [None] + ptrs[i + 1:]) == -1, i
    assert call(hop=64) == -2                                    # hop * 2 != frame
    assert call(frame=320, hop=160) == -2                        # frame > n_fft
    assert call(frame=128, hop=64, n_fft=255) == -2              # odd n_fft
    assert call(C=65) == -2 and call(C=1) == -2
    assert call(frame=512, hop=256, n_fft=512) == -2             # beyond SFM_RESYNTH_MAX_NFFT
    assert call(B=0) == -2 and call(L=0) == -2 and call(T=0) == -2
    assert lib.CONSTANTS["RESYNTH_BWD_TILE_FRAMES"] == ops.RESYNTH_BWD_TILE_FRAMES == 64


def test_mask_resynth_bwd_cost(monkeypatch):
    rec = ops_stub.install(monkeypatch)
    cf = rc.center_freqs("default")
    kw = dict(frame=160, hop=80, n_fft=256, fs=8000, cf=cf, T_mask=14)
    noisy, dout = torch.zeros(2, 1237), torch.zeros(2, 1237)
    out = ops.mask_resynth_bwd(noisy, dout, **kw)
    assert out.shape == (2, 14, 64) and out.dtype == torch.float32
    ops.mask_resynth_bwd(noisy, dout, torch.tensor([1237, 400], dtype=torch.int32), frames=18, **kw)
    # per frame two products of 2 * 160 * 258 = 82560 flops; bytes: noisy 2474 + dout 2474 + Wf 40960 + WiT 40960 + tab_wt 256 +
    # 1 / wsum 240 + channel bins 65 (+ lengths 2) + dmask 1792 words
    assert rec == [
        ("sfm_mask_resynth_bwd", "resynth_bwd", 4623360.0, 356884.0, "B2 L1237 T14 f160 n256 C64"),
        ("sfm_mask_resynth_bwd", "resynth_bwd", 2972160.0, 356892.0, "B2 L1237 T14 f160 n256 C64"),
    ]
    for bad in (dict(hop=64), dict(T_mask=0)):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ops.mask_resynth_bwd(noisy, dout, **{**kw, **bad})
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.mask_resynth_bwd(noisy, dout[:, :1200], **kw)


def test_a_gradient_to_the_noisy_signal_is_refused_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(ops._lib, "load", no_library)
    noisy, mask = torch.zeros(2, 1237, requires_grad=True), torch.zeros(2, 14, 64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="noisy"):
        training.resynthesize(noisy, mask)
    with pytest.raises(NotImplementedError, match="noisy"):
        training.resynthesize(noisy[0], mask[0].detach())
    with torch.no_grad(), pytest.raises(ValueError, match="device"):         # without autograd nothing is asked of it: today's guards
        training.resynthesize(noisy, mask)
