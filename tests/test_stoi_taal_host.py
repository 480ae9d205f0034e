"""STOI of Taal et al. / ESTOI without a GPU: the host design of evaluation/stoi_taal.py against scipy and the issue's rule, the
restatement of tests/stoi_taal_cases.py against its own fixed points, the frame-table planning, the argument errors, the launch
costs of the four wrappers, and the proof that the bounds of tests/test_stoi_taal_gpu.py tell the measure from its mutants."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import signal

import ops_stub
import stoi_taal_cases as sc
from sincformer_metacog_speech_enhancement_amd import lib, ops
from sincformer_metacog_speech_enhancement_amd.evaluation import packed, stoi as pstoi, stoi_taal as st

BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]


# ---- the resampler ----
@pytest.mark.parametrize("up,down", [(5, 8), (5, 4)])
def test_taps_are_resample_polys_default_filter(up, down):
    ref = signal.firwin(2 * 10 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    for h in (st.resample_taps(up, down), sc.taps(up, down)):
        assert h.dtype == np.float64 and h.shape == ref.shape
        assert np.abs(h - ref).max() <= 1e-14 * np.abs(ref).max()


@pytest.mark.parametrize("num", [8, 10])
def test_restated_resampling_is_resample_poly(num):
    case = sc.CASES[num - 1]
    up, down = st.rate_ratio(case[1])
    for x in sc.case_pair(case):
        ref = signal.resample_poly(x.astype(np.float64), up, down)
        got = sc.resample(x, case[1])
        assert got.shape == ref.shape == (-(-x.size * up // down),)
        assert np.abs(got - ref).max() <= 1e-12


@pytest.mark.parametrize("fs,L", [(16000, 9601), (8000, 5000), (16000, 3)])
def test_polyphase_operand_is_the_same_filter(fs, L):
    """the [K, up] operand the framed GEMM multiplies by, applied as that launch applies it (row t = samples t down + k - padl,
    zeros beyond both ends), gives the restatement's resampled signal"""
    up, down = st.rate_ratio(fs)
    W, padl = st.resample_operand(up, down)
    x = np.random.default_rng(5).standard_normal(L)
    n = -(-L * up // down)
    rows = -(-n // up)
    xp = np.concatenate([np.zeros(padl), x, np.zeros(W.shape[0] + rows * down)])
    y = np.stack([xp[t * down:t * down + W.shape[0]] @ W for t in range(rows)]).reshape(-1)[:n]
    assert np.abs(y - sc.resample(x, fs)).max() <= 1e-12
    assert max(up, down) <= ops.STOI_MAX_RATE and st.resample_taps(up, down).size == 2 * ops.STOI_TAP_HALF * max(up, down) + 1


# ---- bands, window, constants ----
def test_band_table_is_the_rule():
    assert sc.band_table() == BANDS
    e = st.band_edges()
    assert list(zip(e[:-1], e[1:])) == BANDS
    assert (ops.STOI_FIRST_BIN, ops.STOI_LAST_BIN, ops.STOI_NBIN, ops.STOI_BANDS) == (7, 218, 212, 15)
    assert (ops.STOI_FS, ops.STOI_FRAME, ops.STOI_HOP, ops.STOI_NFFT, ops.STOI_SEG) == (10000, 256, 128, 512, 30)
    assert ops.STOI_DFT_COLS % 16 == 0 and ops.STOI_DFT_COLS >= 2 * ops.STOI_NBIN


def test_dft_operand_is_the_rfft_of_bins_7_to_218():
    D = st.dft_operand()
    z = np.random.default_rng(1).standard_normal(256)
    ref = np.fft.rfft(z, n=512)[7:219]
    got = z @ D
    assert D.shape == (256, ops.STOI_DFT_COLS) and not D[:, 424:].any()
    assert np.abs(got[:212] - ref.real).max() <= 1e-11 and np.abs(got[212:424] - ref.imag).max() <= 1e-11
    assert np.array_equal(st.window(), np.hanning(258)[1:-1])


# ---- the restatement's fixed points ----
def test_a_signal_against_itself_scores_one():
    c, _ = sc.pair(16000, 16000, seed=3)
    for ext in sc.MEASURES:
        assert abs(sc.stoi64(c, c, 16000, ext) - 1.0) <= 1e-12


def test_both_measures_fall_as_the_noise_rises():
    for ext in sc.MEASURES:
        v = [sc.stoi64(*sc.pair(16000, 16000, gain=g, seed=3), 16000, ext) for g in (0.05, 0.15, 0.5, 1.5)]
        assert all(a > b for a, b in zip(v, v[1:])), v


def test_case_table_is_what_the_issue_states():
    rows = sc.evaluated()                                     # (asserts the margins, the clip branch and the dropped frames)
    for num, (frames, kept, segments) in sc.EXPECTED.items():
        info = rows[(num, False)]["info"]
        assert frames in (None, info["frames"]) and kept in (None, info["kept"]) and segments == info["segments"], (num, info)
    for num in sc.TOO_SHORT:
        for ext in sc.MEASURES:
            assert rows[(num, ext)]["ref"] == 1e-5 and rows[(num, ext)]["e32"] == 0.0
    for ext in sc.MEASURES:
        assert rows[(12, ext)]["ref"] == 0.0 and rows[(12, ext)]["e32"] == 0.0
    assert 0.005 < rows[(4, False)]["info"]["clipped"] < 0.015 and 0.015 < rows[(7, False)]["info"]["clipped"] < 0.025
    assert min(r["info"]["margin"] for r in rows.values()) >= 17.0


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_the_bounds_tell_the_measure_from_its_mutants(mutant):
    """each mutant moves at least one case's value by more than that case's GPU bound"""
    rows = sc.evaluated()
    moved = []
    for case in sc.CASES:
        c, e = sc.case_pair(case)
        for ext in sc.MEASURES:
            r = rows[(case[0], ext)]
            d = abs(sc.stoi64(c, e, case[1], ext, mutant=mutant) - r["ref"])
            if d > r["bound"]:
                moved.append((case[0], ext, d, r["bound"]))
    assert moved, mutant


# ---- planning ----
def test_frame_tables_of_ragged_lengths():
    """an utterance shorter than one frame between two long ones owns no frame, no tile and no band row"""
    p = st.plan_tables([6000, 100, 9601], 16000)
    assert p["sig_len"].tolist() == [3750, 63, 6001] and (p["up"], p["down"]) == (5, 8)
    assert p["in_off"].tolist() == [0, 6000, 6100] and p["in_len"].tolist() == [6000, 100, 9601] and p["sig_off"].tolist() == [0, 3750, 3813]
    assert p["frames"].tolist() == [28, 0, 45] and p["frame_off"].tolist() == [0, 28, 28, 73]
    assert p["tiles"].tolist() == [[0, 0], [0, 1], [2, 0], [2, 1], [2, 2]] and p["spec_rows"] == 71 and p["segments"] == 15
    assert p["sum_frames"] == 73 and p["n_samples"] == 9814 and p["n_in"] == 15701
    q = st.plan_tables([255, 256, 383, 384, 4224], 10000)
    assert q["frames"].tolist() == [0, 1, 1, 2, 32] and q["sig_off"].tolist() == [0, 255, 511, 894, 1278]
    assert q["tiles"].tolist() == [[3, 0], [4, 0], [4, 1]] and q["spec_rows"] == 32 and q["in_off"].tolist() == q["sig_off"].tolist()
    r = st.plan_tables([300, 300], 10000, [0, 1000])           # rows of a zero-padded batch
    assert r["sig_off"].tolist() == [0, 1000] and r["in_off"].tolist() == [0, 1000]
    assert st.plan_tables([300, 300], 8000, [0, 1000])["in_off"].tolist() == [0, 1000]
    p8 = st.plan_tables([5000], 8000)
    assert p8["sig_len"].tolist() == [6250] and p8["frames"].tolist() == [47] and (p8["up"], p8["down"]) == (5, 4)
    for case in sc.CASES:                                      # the plan's frame counts are the restatement's
        info = sc.evaluated()[(case[0], False)]["info"]
        assert st.plan_tables([case[2]], case[1])["frames"].tolist() == [info["frames"]]
    with pytest.raises(ValueError):
        st.plan_tables([], 16000)


# ---- errors raised before anything is launched ----
def test_unsupported_rate_and_unknown_names():
    x = np.zeros(4000, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="22050"):
        st.compute_stoi_taal(x, x, fs=22050)
    with pytest.raises(NotImplementedError, match="22050"):
        st.compute_stoi_taal_packed([x], [x], fs=22050)
    with pytest.raises(NotImplementedError, match="22050"):
        pstoi.compute_stoi(x, x, fs=22050, method="taal")
    with pytest.raises(ValueError, match="pystoi"):
        pstoi.compute_stoi(x, x, fs=16000, method="pystoi")
    with pytest.raises(ValueError, match="stoi_extended"):
        packed.compute_metrics_packed([x], [x], metrics=("stoi", "stoi_extended"))
    assert packed._check_metrics(("stoi", "stoi_taal", "estoi")) == ("stoi", "stoi_taal", "estoi")
    assert packed.METRICS == ("stoi", "pesq", "ssnr")


# ---- launch costs: the recording _call of tests/test_launch_costs_host.py ----
@pytest.fixture
def launches(monkeypatch):
    return ops_stub.install(monkeypatch)


def test_stoi_launch_costs(launches):
    p = st.plan_tables([6000, 100, 9601], 16000)
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32))
    W, padl = st.resample_operand(p["up"], p["down"])
    sig = ops.stoi_resample(torch.zeros(p["n_in"]), torch.from_numpy(W.astype(np.float32)), i32(p["in_off"]), i32(p["in_len"]),
                            i32(p["sig_off"]), i32(p["sig_len"]), 3, p["n_samples"], int(p["sig_len"].max()), p["n_in"], 5, 8, padl)
    assert sig.shape == (9814,) and W.shape == (39, 5) and padl == 16
    win, dft = torch.zeros(256), torch.zeros(256, ops.STOI_DFT_COLS)
    so, sl, fo, tiles = i32(p["sig_off"]), i32(p["sig_len"]), i32(p["frame_off"]), i32(p["tiles"])
    src, kept, _ = ops.stoi_keep(sig, win, so, sl, fo, 3, p["sum_frames"], p["n_samples"])
    xb, yb = ops.stoi_bands((sig, sig), win, dft, so, fo, src, kept, tiles, p["sum_frames"], p["spec_rows"], p["n_samples"])
    ops.stoi_bands((sig,), win, dft, so, fo, src, kept, tiles, p["sum_frames"], p["spec_rows"], p["n_samples"])
    ops.stoi_segments(xb, yb, fo, kept, 3, False, p["spec_rows"], p["segments"])
    ops.stoi_segments(xb, yb, fo, kept, 3, True, p["spec_rows"], p["segments"])
    assert xb.shape == (73, 15) and src.shape == (73,) and kept.shape == (3,)
    assert launches == [
        ("sfm_stoi_resample", "stoi", 765492.0, 102888.0, "resample 5/8 B3 out9814"),
        ("sfm_stoi_keep", "stoi", 56064.0, 41204.0, "keep B3 frames73"),
        ("sfm_stoi_bands", "stoi", 30826496.0, 522564.0, "bands x2 rows71"),
        ("sfm_stoi_bands", "stoi", 15413248.0, 479048.0, "bands x1 rows71"),
        ("sfm_stoi_segments", "stoi", 81000.0, 8572.0, "stoi B3 rows71"),
        ("sfm_stoi_segments", "stoi", 81000.0, 8572.0, "estoi B3 rows71"),
    ]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.stoi_bands((sig,), win, torch.zeros(256, 424), so, fo, src, kept, tiles, p["sum_frames"], p["spec_rows"], p["n_samples"])


# ---- utterances with one frame: no spectral frame, no tile ----
def test_one_frame_utterances_score_1e_5_and_own_no_tile():
    for fs, L in sc.ONE_FRAME + sc.TWO_FRAMES:
        info = {}
        c, e = sc.pair(L, fs)
        for ext in sc.MEASURES:
            assert sc.stoi64(c, e, fs, ext, info=info) == 1e-5
        p = st.plan_tables([L], fs)
        assert p["frames"].tolist() == [info["frames"]] == [1 if (fs, L) in sc.ONE_FRAME else 2]
        assert p["tiles"].shape == ((0, 2) if (fs, L) in sc.ONE_FRAME else (1, 2)) and p["segments"] == 0
    p = st.plan_tables([L for fs, L in sc.ONE_FRAME if fs == 16000], 16000)
    assert p["sum_frames"] == 2 and p["spec_rows"] == 0 and p["tiles"].shape == (0, 2)


def test_bands_entry_point_takes_an_empty_tile_table_without_a_gpu():
    """no utterance with a spectral frame: n_tiles = 0 with a NULL table (an empty tensor has no address) is SFM_OK and launches
    nothing; a NULL table with tiles to do, and the other null pointers, are refused as everywhere"""
    L = lib.load()
    one = ctypes.c_void_p(16)
    assert L.sfm_stoi_bands(one, one, one, one, one, one, one, one, None, one, one, 0, 2, None) == 0
    assert L.sfm_stoi_bands(one, None, one, one, one, one, one, one, None, one, None, 0, 1, None) == 0
    assert L.sfm_stoi_bands(one, one, one, one, one, one, one, one, None, one, one, 1, 2, None) == -1
    assert L.sfm_stoi_bands(None, one, one, one, one, one, one, one, None, one, one, 0, 2, None) == -1
    assert L.sfm_stoi_bands(one, None, one, one, one, one, one, one, None, one, one, 0, 2, None) == -1
    assert L.sfm_stoi_bands(one, one, one, one, one, one, one, one, None, one, one, 0, 3, None) == -2
    assert torch.zeros(10, dtype=torch.int32)[5:5].view(-1, 2).data_ptr() == 0      # (why the table can be NULL)
