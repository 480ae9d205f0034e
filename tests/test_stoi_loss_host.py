"""The STOI / ESTOI gradient without a GPU: the float64 autograd restatement of tests/stoi_loss_cases.py against stoi64 and
central differences, the generator's conditions, the host design of the adjoint resampler, plan caching, the refusals, and the
mutants of the gradient against the GPU test's own assertion."""
import ctypes

import numpy as np
import pytest
import torch

import ops_stub
import stoi_loss_cases as lc
import stoi_taal_cases as sc
from sincformer_metacog_speech_enhancement_amd import lib, ops
from sincformer_metacog_speech_enhancement_amd.evaluation import stoi_taal as st


# ---- the restatement ----
def test_restatement_value_is_stoi64():
    for cs in sc.CASES:
        c, e = sc.case_pair(cs)
        for ext in sc.MEASURES:
            for dt in (np.float64, np.float32):
                e64 = torch.from_numpy(e.astype(np.float64))
                got = float(lc.score_t(c, e64, cs[1], ext, dt))
                assert abs(got - sc.stoi64(c, e, cs[1], ext, dt)) <= 1e-14, (cs[0], ext, dt)
    for fs, L in sc.ONE_FRAME + sc.TWO_FRAMES:
        c, e = sc.pair(L, fs)
        assert float(lc.score_t(c, torch.from_numpy(e.astype(np.float64)), fs)) == 1e-5


def test_restatement_gradient_is_the_central_difference():
    rows = lc.evaluated()
    for num in lc.GRAD_CASES:
        cs = lc.case(num)
        c, e = sc.case_pair(cs)
        d = np.random.default_rng(100 + num).standard_normal(e.size)
        d /= np.linalg.norm(d)
        h = 1e-6
        for ext in sc.MEASURES:
            up = sc.stoi64(c, e.astype(np.float64) + h * d, cs[1], ext)
            dn = sc.stoi64(c, e.astype(np.float64) - h * d, cs[1], ext)
            fd, an = (up - dn) / (2 * h), float(rows[(num, ext)]["grad"] @ d)
            print("ROW | case %d %s | directional %.9e | central difference %.9e | relative %.2e"
                  % (num, "estoi" if ext else "stoi", an, fd, abs(fd - an) / abs(an)))
            assert abs(fd - an) <= 1e-5 * abs(an), (num, ext, fd, an)


def test_generator_conditions_and_bounds():
    rows = lc.evaluated()
    margins = {num: rows[(num, False)]["info"]["margin_clip"] for num in lc.GRAD_CASES}
    assert min(margins.values()) >= lc.MIN_CLIP_MARGIN
    for num in lc.CLIPPING:
        assert rows[(num, False)]["info"]["clipped"] > 0.0
    for key, row in rows.items():
        assert 1e-8 < row["e32g"] < 1e-5 and row["zeros"] >= 128, (key, row["e32g"], row["zeros"])
        print("ROW | %s %s | e32g %.2e | bound %.2e | exact zeros %d" % (key[0], "estoi" if key[1] else "stoi", row["e32g"],
                                                                      row["bound"], row["zeros"]))


def test_ascent_step_raises_the_float64_score_by_ten_e32():
    """ASCENT_STEP is chosen here, on the CPU: ten steps along this file's float64 gradient raise the float64 score of case 4 by
    at least 10 x the case's forward e32"""
    cs = lc.case(lc.ASCENT_CASE)
    c, e = sc.case_pair(cs)
    for ext in sc.MEASURES:
        x, first = e.copy(), None
        for _ in range(lc.ASCENT_STEPS):
            v, g = lc.value_and_grad(c, x, cs[1], ext)
            first = v if first is None else first
            x = x + np.float32(lc.ASCENT_STEP) * g.astype(np.float32)
        rise = sc.stoi64(c, x, cs[1], ext) - first
        assert rise >= 10.0 * sc.evaluated()[(lc.ASCENT_CASE, ext)]["e32"] and rise > 1e-2, (ext, rise)


# ---- mutants of the gradient: each fails the GPU test's own assertion ----
MUTANT_CASES = {"through clipped": (4, False), "alpha constant": (7, False), "window once": (2, True), "last frame taken": (3, True),
                "kept from enhanced": (4, True), "plain sqrt": ("silent", False)}


def _pair_of(key):
    if key == "silent":
        return lc.silent_pair() + (lc.SILENT[1],)
    cs = lc.case(key)
    return sc.case_pair(cs) + (cs[1],)


def test_the_float32_operand_gradient_passes_and_every_mutant_fails():
    rows = lc.evaluated()
    assert set(MUTANT_CASES) == set(lc.MUTANTS)
    for mutant, (key, ext) in MUTANT_CASES.items():
        c, e, fs = _pair_of(key)
        _, good = lc.value_and_grad(c, e, fs, ext, np.float32)
        assert lc.violates(good, rows[(key, ext)]) is None, (mutant, key)
        _, bad = lc.value_and_grad(c, e, fs, ext, np.float32, mutant=mutant)
        why = lc.violates(bad, rows[(key, ext)])
        print("ROW | mutant %s | case %s %s | %s" % (mutant, key, "estoi" if ext else "stoi", why))
        assert why is not None, mutant


# ---- host design ----
@pytest.mark.parametrize("fs", [8000, 16000])
def test_adjoint_resampling_operand_is_the_transpose(fs):
    up, down = st.rate_ratio(fs)
    W, padl = st.resample_operand(up, down)
    Wt, padt = st.resample_adjoint_operand(up, down)
    assert Wt.shape[1] == down and Wt.shape[0] <= 2 * ops.STOI_TAP_HALF * ops.STOI_MAX_RATE + 1 and 0 <= padt < Wt.shape[0]
    for L in (61, 200):
        Lr = int(st.resampled_lengths([L], fs)[0])
        R, A = np.zeros((Lr, L)), np.zeros((L, Lr))
        for n in range(Lr):                                  # the forward as sfm_stoi_resample applies its operand
            t, p = divmod(n, up)
            for k in range(W.shape[0]):
                s = t * down + k - padl
                if 0 <= s < L:
                    R[n, s] += W[k, p]
        for n in range(L):                                   # the same kernel with up and down exchanged
            t, p = divmod(n, down)
            for k in range(Wt.shape[0]):
                s = t * up + k - padt
                if 0 <= s < Lr:
                    A[n, s] += Wt[k, p]
        assert np.array_equal(A, R.T) and np.array_equal(A.astype(np.float32), R.T.astype(np.float32))
        x = np.random.default_rng(L).standard_normal(L)
        assert np.allclose(R @ x, sc.resample(x, fs), rtol=0, atol=1e-12)
    assert set(np.unique(Wt[Wt != 0])) <= set(np.unique(st.resample_taps(up, down)))


def test_plan_caching_returns_the_same_objects(monkeypatch):
    uploads = []

    def upload(plan, dev):
        uploads.append(plan)
        return {"frame_off": object()}
    monkeypatch.setattr(st, "_upload", upload)
    monkeypatch.setattr(st, "_plans", {})
    a = st.batch_plan(16000, 3, 9601, [9601, 200, 6759], "cuda:0")
    b = st.batch_plan(16000, 3, 9601, np.array([9601, 200, 6759]), "cuda:0")
    c = st.batch_plan(16000, 3, 9601, (9601, 200, 6000), "cuda:0")
    d = st.batch_plan(16000, 3, 9601, None, "cuda:0")
    assert a[0] is b[0] and a[1] is b[1] and c[0] is not a[0] and d[0] is not a[0] and len(uploads) == 3
    assert a[0]["in_off"].tolist() == [0, 9601, 2 * 9601] and a[0]["in_len"].tolist() == [9601, 200, 6759]
    assert d[0]["in_len"].tolist() == [9601] * 3
    for bad in ([9601, 200], [9601, 200, 9602], [9601, -1, 5]):
        with pytest.raises(ValueError, match="lengths"):
            st.batch_plan(16000, 3, 9601, bad, "cuda:0")
    assert len(uploads) == 3


def test_refusals_without_a_gpu():
    from sincformer_metacog_speech_enhancement_amd import config, evaluation, training
    assert "TaalSTOILoss" in training.__all__ and evaluation.stoi_taal_scores is st.stoi_taal_scores
    for rate in (44100, 22050, 4000):
        with pytest.raises(NotImplementedError, match="sample rate"):
            training.TaalSTOILoss(sample_rate=rate)
    m = training.TaalSTOILoss()
    assert m.sample_rate == config.SAMPLE_RATE and m.extended is None and config.STOI_EXTENDED is False
    assert training.TaalSTOILoss(16000, extended=True).extended is True and not list(m.parameters())
    x = torch.zeros(2, 6000)
    with pytest.raises(RuntimeError, match="CPU"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.stoi_taal_scores(x, x, 16000)


# ---- the entry points ----
def test_backward_launch_costs(monkeypatch):
    rec = ops_stub.install(monkeypatch)
    p = st.plan_tables([6000, 100, 9601], 16000, np.arange(3) * 9601)
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32))
    so, sl, fo, tiles = i32(p["sig_off"]), i32(p["sig_len"]), i32(p["frame_off"]), i32(p["tiles"])
    tabs = {"sig_off": so, "sig_len": sl, "frame_off": fo, "tiles": tiles, "in_off": i32(p["in_off"]), "in_len": i32(p["in_len"])}
    a = {"re": torch.zeros(p["n_samples"]), "src": torch.zeros(73, dtype=torch.int32), "kept": torch.zeros(3, dtype=torch.int32),
         "xb": torch.zeros(73, 15), "yb": torch.zeros(73, 15)}
    monkeypatch.setattr(st, "_operands", {})
    out = st.gradient_flat(a, p, tabs, torch.zeros(3, dtype=torch.float64), True, 9601)
    assert out.shape == (3 * 9601,) and not out.any()       # (ragged rows: the buffer starts as zeros)
    assert [r[0] for r in rec] == ["sfm_stoi_segments_bwd", "sfm_stoi_bands_bwd", "sfm_stoi_fold_bwd", "sfm_stoi_resample"]
    assert [r[4] for r in rec] == ["estoi bwd B3 rows71", "bands bwd rows71", "fold bwd B3 out9814", "resample 8/5 B3 out28803"]
    assert rec[0][2] == 30.0 * 30 * 15 * p["segments"] and rec[1][2] == 2.0 * 71 * 256 * (424 + 432) and all(r[3] > 0 for r in rec)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.stoi_segments_bwd(a["xb"], a["yb"], fo, a["kept"], torch.zeros(3), 3, 45, False, 71, p["segments"])
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.stoi_segments_bwd(a["xb"], a["yb"], fo, a["kept"], torch.zeros(3, dtype=torch.float64), 3, 74, False, 71, p["segments"])
    assert ops.STOI_BWD_ROWS == 32
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.stoi_fold_bwd(torch.zeros(73, 256), torch.zeros(256), so, sl, fo, a["src"], a["kept"], 3, 10, 5, 6, 73)


def test_backward_entry_points_refuse_without_a_gpu():
    L = lib.load()
    one = ctypes.c_void_p(16)
    assert L.sfm_stoi_segments_bwd(one, one, one, one, one, None, 1, 40, 0, None) == -1
    assert L.sfm_stoi_segments_bwd(one, one, one, one, one, one, 0, 40, 0, None) == -2
    assert L.sfm_stoi_segments_bwd(one, one, one, one, one, one, 1, 40, 2, None) == -2
    assert L.sfm_stoi_segments_bwd(one, one, one, one, one, one, 1, -1, 0, None) == -2
    assert L.sfm_stoi_segments_bwd(one, one, one, one, one, one, 1, 0, 1, None) == 0                        # no row: no launch
    assert L.sfm_stoi_bands_bwd(one, one, one, one, one, one, one, one, None, one, one, 0, None) == 0       # no tile: no launch
    assert L.sfm_stoi_bands_bwd(one, one, one, one, one, one, one, one, None, one, one, 1, None) == -1
    assert L.sfm_stoi_bands_bwd(one, one, one, None, one, one, one, one, None, one, one, 0, None) == -1
    assert L.sfm_stoi_bands_bwd(one, one, one, one, one, one, one, one, one, one, one, -1, None) == -2
    assert L.sfm_stoi_fold_bwd(one, one, one, one, one, one, one, one, 1, 0, 0, None) == 0                  # no sample: no launch
    assert L.sfm_stoi_fold_bwd(one, one, one, one, one, one, one, None, 1, 0, 0, None) == -1
    assert L.sfm_stoi_fold_bwd(one, one, one, one, one, one, one, one, 1, 5, 6, None) == -2
    assert L.sfm_stoi_fold_bwd(one, one, one, one, one, one, one, one, 65536, 5, 0, None) == -2
