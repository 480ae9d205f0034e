"""CSII and NCM without a GPU: the float64 restatements of tests/intelligibility_cases.py against the reference's recorded values
(tests/golden/g21_intelligibility.npz), the package's host-built operands (SII weights, channel weights, the Hilbert kernel h,
the Hamming DFT operand, tile tables, groups), the C ABI's guards, the launches' stated costs, and - for every mutant - that the
bound the GPU rows use tells it from the float64 value on at least one case."""
import ctypes
import os

import numpy as np
import pytest
import torch

import intelligibility_cases as ic
import ops_stub
from sincformer_metacog_speech_enhancement_amd import evaluation, lib, ops
from sincformer_metacog_speech_enhancement_amd.evaluation import csii, intelligibility, ncm

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_intelligibility.npz"))
F32, F64 = np.float32, np.float64

_memo = {}


def _csii(name, dtype):
    if (name, dtype) not in _memo:
        _, fs, L, seed = next(c for c in ic.CSII_CASES if c[0] == name)
        _memo[(name, dtype)] = ic.csii64(*ic.pair(L, seed, fs), fs, dtype)
    return _memo[(name, dtype)]


def _ncm(name, dtype):
    if (name, dtype) not in _memo:
        _, bname, fs, L, seed = next(c for c in ic.NCM_CASES if c[0] == name)
        _memo[(name, dtype)] = ic.ncm64(*ic.pair(L, seed, fs), ic.bank(bname), dtype)
    return _memo[(name, dtype)]


# ---- the restatements are the reference ----
@pytest.mark.parametrize("case", ic.CSII_CASES, ids=lambda c: c[0])
def test_csii_restatement_equals_the_reference(case):
    name, fs, L, seed = case
    score, msc = _csii(name, F64)
    assert abs(score - float(G["csii." + name])) <= 1e-12
    assert np.abs(msc - G["msc." + name]).max() <= 1e-12
    c = ic.pair(L, seed, fs)[0]
    assert abs(ic.csii64(c, c, fs)[0] - float(G["csii.ident." + name])) <= 1e-12
    if L < int(0.016 * fs):
        assert score == 0.0 and float(G["csii." + name]) == 0.0


@pytest.mark.parametrize("fs", [8000, 16000])
def test_csii_is_one_coherence_estimate_at_every_length(fs):
    for i, L in enumerate(ic.CSII_GOLDEN_LENGTHS[fs]):
        assert abs(ic.csii64(*ic.pair(L, 540 + i, fs), fs)[0] - G["csii.len.%d" % fs][i]) <= 1e-12, L


@pytest.mark.parametrize("case", ic.NCM_CASES, ids=lambda c: c[0])
def test_ncm_restatement_equals_the_reference(case):
    name, bname, fs, L, seed = case
    score, ncc = _ncm(name, F64)
    assert abs(score - float(G["ncm." + name])) <= 1e-12
    assert np.abs(ncc - G["ncc." + name]).max() <= 1e-12
    if L < 64:
        assert score == 0.0 and float(G["ncm." + name]) == 0.0


@pytest.mark.parametrize("L", [64, 65])
def test_hilbert_restatement_equals_scipy(L):
    y, _ = ic.hilbert64(ic.hilbert_rows(L).astype(F64))
    assert np.abs(y - G["hilbert.y%d" % L]).max() <= 1e-12


# ---- host-built operands ----
def test_weights_and_hilbert_kernel_equal_the_reference():
    for fs in (8000, 16000, 22050):
        assert np.abs(csii.sii_weights(fs) - G["sii.%d" % fs]).max() <= 1e-15
    for bname in ic.BANKS:
        w = ncm.channel_weights(ic.bank(bname).center_freqs)
        assert w.shape == G["chw." + bname].shape and np.abs(w - G["chw." + bname]).max() <= 1e-15
    for L in (64, 65):
        h = ops.hilbert_kernel_table(L)
        assert h.dtype == np.float64 and np.abs(h - G["hilbert.h%d" % L]).max() <= 1e-15
        assert np.array_equal(h, ic.hilbert_h(L))
    h = ops.hilbert_kernel_table(64)
    assert np.abs(h[0::2]).max() <= 1e-17 and np.abs(ops.hilbert_kernel_table(65)[2::2]).min() > 1e-4   # even lags: 0 for an even L only


@pytest.mark.parametrize("L", [2, 64, 65, 128, 1000])
def test_kernel_table_restates_the_convolution(L):
    """the table's index arithmetic, as csrc/intelligibility.hip reads it, against the circular convolution with h"""
    tab = ops.hilbert_table_host(L).astype(F64)
    assert tab.shape == (2 * L,)
    x = np.random.RandomState(L).standard_normal(L)
    h = ops.hilbert_kernel_table(L).astype(F32).astype(F64)
    want = np.asarray([sum(h[(n - m) % L] * x[m] for m in range(L)) for n in range(L)])
    got = np.zeros(L)
    if L % 2:
        for n in range(L):
            got[n] = sum(tab[n - m + L] * x[m] for m in range(L))
    else:
        Lc = L // 2
        for p in (0, 1):
            for i in range(Lc):
                got[2 * i + p] = sum(tab[p * L + i - j + Lc] * x[2 * j + 1 - p] for j in range(Lc))
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_dft_operand_is_the_hamming_rfft_256():
    for fs, K in ((8000, 128), (16000, 256), (22050, 256)):
        frame = int(0.016 * fs)
        M = csii.csii_operand_host(fs)
        assert M.shape == (K, 258) and M.dtype == np.float64
        x = np.random.RandomState(fs).standard_normal(frame)
        want = np.fft.rfft(x * np.hamming(frame), n=256)
        got = x[:K] @ M
        assert np.abs(got[:129] - want.real).max() <= 1e-12 and np.abs(got[129:] - want.imag).max() <= 1e-12
    assert csii.csii_framing(22050) == (352, 176) and csii.csii_framing() == (128, 64)


def test_tile_table_and_groups():
    # an odd length: ceil(L / 256) tiles; an even one: two problems of L / 2 samples, ceil(L / 512) tiles each
    tiles, off, work = ops.hilbert_tiles([2000, 64, 1237, 63, 401, 256, 257, 514], ncm.MIN_LEN)
    assert off.tolist() == [0, 8, 10, 15, 15, 17, 19, 21, 25] and tiles.dtype == np.int32 and tiles.shape == (25, 2)
    assert tiles[:10].tolist() == [[0, t] for t in range(8)] + [[1, 0], [1, 1]] and tiles[-4:].tolist() == [[7, t] for t in range(4)]
    assert work == 8 * 1000 + 2 * 32 + 5 * 1237 + 2 * 401 + 2 * 128 + 2 * 257 + 4 * 257
    lens = [2000, 64, 1237, 401]                                            # the ragged set without its 63-sample member
    assert ncm.plan_groups(lens, 64) == [(0, 4)]
    assert ncm.plan_groups(lens, 64, 1_300_000) == [(0, 1), (1, 3), (3, 4)]  # 512 bytes per padded sample: 1 024 000, 1 266 688, ..
    assert ncm.plan_groups(lens, 64, 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]  # above the budget: groups of one
    assert ncm.plan_groups([], 64) == []


def test_exports_and_signatures():
    import inspect
    assert list(inspect.signature(evaluation.compute_csii).parameters)[:4] == ["clean_signal", "enhanced_signal", "fs", "num_levels"]
    assert list(inspect.signature(evaluation.compute_ncm).parameters)[:4] == ["clean_signal", "enhanced_signal", "fs", "gfb"]
    assert inspect.signature(evaluation.compute_csii).parameters["num_levels"].default == 3
    assert list(inspect.signature(evaluation.compute_intelligibility_packed).parameters)[:6] == [
        "clean", "enhanced", "seg", "fs", "metrics", "gfb"]
    assert evaluation.hilbert_envelope is ncm.hilbert_envelope
    assert intelligibility.INTELLIGIBILITY_METRICS == ("csii", "ncm")
    with pytest.raises(ValueError, match="choose from"):
        evaluation.compute_intelligibility_packed([np.zeros(100)], [np.zeros(100)], metrics=("stoi",))
    with pytest.raises(ValueError, match="num_levels"):
        evaluation.compute_intelligibility_packed([np.zeros(100)], [np.zeros(100)], num_levels=0)
    with pytest.raises(ValueError, match="num_levels"):
        evaluation.compute_csii(np.zeros(100), np.zeros(100), num_levels=0)


# ---- the C ABI's guards, before any HIP call ----
def test_abi_guards_without_a_gpu():
    L = lib.load()
    one = ctypes.c_void_p(16)
    for name in ("sfm_csii_frames_varlen", "sfm_hilbert_env", "sfm_hilbert_env_moments", "sfm_ncm_finish"):
        assert lib.ABI[name][0] is ctypes.c_int
    assert L.sfm_csii_frames_varlen(one, one, one, None, one, one, one, None, 2, 10, 129, None) == -1
    assert L.sfm_csii_frames_varlen(one, one, one, one, one, one, None, None, 2, 10, 129, None) == -1
    assert L.sfm_csii_frames_varlen(one, one, one, one, one, one, one, None, 2, 10, 128, None) == -2     # plane width != 129
    assert L.sfm_csii_frames_varlen(one, one, one, one, one, one, one, None, 0, 10, 129, None) == -2
    assert L.sfm_hilbert_env(None, one, one, 3, 64, None) == -1
    assert L.sfm_hilbert_env(one, one, one, 3, 0, None) == -2                                             # L < 1
    assert L.sfm_hilbert_env(one, one, one, 0, 64, None) == -2
    assert L.sfm_hilbert_env_moments(one, one, one, one, None, one, 1, 64, 64, 1, None) == -1
    assert L.sfm_hilbert_env_moments(one, one, one, one, one, one, 1, 65, 64, 1, None) == -2              # C > 64: 2 C > 128 columns
    assert L.sfm_hilbert_env_moments(one, one, one, one, one, one, 1, 64, 0, 1, None) == -2               # L < 1
    assert L.sfm_hilbert_env_moments(one, one, one, one, one, one, 1, 64, 64, 0, None) == 0               # no tile: nothing launched
    assert L.sfm_ncm_finish(one, one, one, None, one, one, 1, 64, None) == -1
    assert L.sfm_ncm_finish(one, one, one, one, one, one, 1, 65, None) == -2


def test_launch_costs(monkeypatch):
    rec = ops_stub.install(monkeypatch)
    monkeypatch.setattr(ops, "hilbert_table", lambda L, dev: torch.zeros(2 * L))
    B, C, L = 2, 64, 1000
    planes = torch.zeros(4, 30, 129)
    s, m = ops.csii_frames_varlen(planes[0], planes[1], planes[2], planes[3], torch.zeros(B + 1, dtype=torch.int32),
                                  torch.zeros(129, dtype=torch.float64), B, True)
    assert s.shape == (B,) and m.shape == (B, 129) and s.dtype == m.dtype == torch.float64
    assert ops.hilbert_env(torch.zeros(3, L)).shape == (3, L)
    tiles, off, work = ops.hilbert_tiles([L, L])
    assert work == 8 * 500
    p = ops.hilbert_env_moments(torch.zeros(2, B, C, L), torch.zeros(2 * L), torch.zeros(B, dtype=torch.int32),
                                torch.zeros(B, dtype=torch.int32), torch.from_numpy(tiles), C, work)
    assert p.shape == (8, C, 5) and p.dtype == torch.float64
    ops.ncm_finish(p, torch.from_numpy(off), torch.zeros(B, dtype=torch.int32), torch.zeros(C, dtype=torch.float64), B, C)
    assert rec == [
        ("sfm_csii_frames_varlen", "intelligibility", 54180.0, 61920.0, None),
        ("sfm_hilbert_env", "hilbert_env", 3000000.0, 32000.0, "R3 L1000"),                # an even L: two convolutions of L / 2
        ("sfm_hilbert_env_moments", "hilbert_env", 262144000.0, 1044480.0, "B2 C64 L1000 tiles8"),
        ("sfm_ncm_finish", "intelligibility", 2560.0, 20480.0, None),
    ]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.hilbert_env_moments(torch.zeros(2, B, 65, L), torch.zeros(2 * L), torch.zeros(B, dtype=torch.int32),
                                torch.zeros(B, dtype=torch.int32), torch.from_numpy(tiles), 65)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.csii_frames_varlen(planes[0, :, :128].contiguous(), planes[1, :, :128].contiguous(), planes[2, :, :128].contiguous(),
                               planes[3, :, :128].contiguous(), torch.zeros(B + 1, dtype=torch.int32),
                               torch.zeros(129, dtype=torch.float64), B)


# ---- mutants: the GPU rows' bound tells each from the float64 value ----
def _separated(name, mutant, wrong, ref64, ref32):
    bound = ic.K * ic.fig(ref32, ref64)
    moved = ic.fig(wrong, ref64)
    print("MUTANT | %s | %s | moves the reference by %.3e, bound %.3e" % (name, mutant, moved, bound))
    return moved > bound


@pytest.mark.parametrize("mutant", ic.HILBERT_MUTANTS)
def test_hilbert_mutants_are_told_apart(mutant):
    hit = []
    for L in ic.HILBERT_L:
        x = ic.hilbert_rows(L)
        e64, e32 = ic.hilbert64(x, F64)[1], ic.hilbert64(x, F32)[1]
        if _separated("hilbert L%d" % L, mutant, ic.hilbert64(x, F64, mutant)[1], e64, e32):
            hit.append(L)
    assert hit, mutant
    if mutant == "even-L table at odd L":
        assert all(L % 2 for L in hit)
    if mutant == "Nyquist bin doubled":
        assert all(L % 2 == 0 for L in hit)


@pytest.mark.parametrize("mutant", ic.NCM_MUTANTS)
def test_ncm_mutants_are_told_apart(mutant):
    hit = []
    for name, bname, fs, L, seed in ic.NCM_CASES[1:4]:
        wrong = ic.ncm64(*ic.pair(L, seed, fs), ic.bank(bname), F64, mutant)[1]
        if _separated(name, mutant, wrong, _ncm(name, F64)[1], _ncm(name, F32)[1]):
            hit.append(name)
    assert hit, mutant


@pytest.mark.parametrize("mutant", ic.CSII_MUTANTS)
def test_csii_mutants_are_told_apart(mutant):
    hit = []
    for name, fs, L, seed in ic.CSII_CASES:
        if L < int(0.016 * fs):
            continue
        wrong = ic.csii64(*ic.pair(L, seed, fs), fs, F64, mutant)[1]
        if _separated(name, mutant, wrong, _csii(name, F64)[1], _csii(name, F32)[1]):
            hit.append(name)
    assert hit, mutant
    if mutant == "frames counted with the cropped frame":
        assert hit == ["c22_1400"]
    if mutant == "n_fft = frame at 8 kHz":
        assert all(n.startswith("c8_") for n in hit)
