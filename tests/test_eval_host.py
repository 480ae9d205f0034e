"""Packed evaluation, the part that needs no GPU: the oracle and the restated PESQ fallback against the reference's values
(tests/golden/g14_eval.npz), the frame-offset tables of the three framings, the host part of evaluate_batch, the argument
guards of the new entry points, and - in the style of test_host_logic.py - proof that the bounds of tests/test_eval_gpu.py
separate plausible wrong packed kernels."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as ec
from helpers import gold, K_TRANS
from oracle import sfm_oracle as orc
from sincformer_metacog_speech_enhancement_amd import functional as Fn
from sincformer_metacog_speech_enhancement_amd.evaluation import packed as pk


@pytest.fixture(scope="module")
def case():
    c, x, e = ec.signals()
    return c, x, e, ec.scores64(c, e)


@pytest.fixture(scope="module")
def pesq_bound():
    e32 = ec.pesq_e32()
    print("PESQ e32 %.3e -> bound %.3e" % (e32, K_TRANS * e32))
    return K_TRANS * e32


# ---------------------------------------------------------------------------
# oracle / restatement against the reference's values
# ---------------------------------------------------------------------------
def test_oracle_and_restatement_reproduce_the_reference_values(case):
    c, x, e, s = case
    g = gold("g14_eval")
    assert g["lengths"].tolist() == ec.LENGTHS == [a.size for a in c]
    for m in ec.METRICS:
        d = np.abs(s[m] - g[m])
        print("%s max |oracle - reference| %.2e" % (m, d.max()))
        assert d.max() <= 1e-9, (m, d)
    ic, ie = ec.identical_pair()
    got = [orc.ssnr(ic, ie), orc.stoi_simplified(ic, ie, ec.FS), ec.pesq_simplified64(ic, ie, ec.FS)]
    assert np.abs(np.array(got) - g["identical"]).max() <= 1e-9 and np.abs(g["identical"] - [35.0, 1.0, 4.5]).max() < 1e-12


def test_the_set_holds_every_boundary(case):
    c, x, e, s = case
    n = {m: [ec.frame_count(L, *ec.FRAMINGS[m]) for L in ec.LENGTHS] for m in ec.METRICS}
    at = ec.LENGTHS.index
    assert (n["ssnr"][at(160)], n["ssnr"][at(159)]) == (1, 0) and (n["pesq"][at(512)], n["pesq"][at(511)]) == (1, 0)
    assert n["stoi"][at(400)] == 0 and n["ssnr"][at(400)] > 0 and [n[m][at(129)] for m in ec.METRICS] == [0, 0, 0]
    for m in ec.METRICS:                                    # leading / inner / trailing utterances without a frame in a pack
        assert n[m][-1] == 0 and 0 in n[m][1:-1]
        assert n[m][::-1][0] == 0 and n[m][0] > 0             # ... so the reversed set (a GPU case) starts with an empty one
    assert s["ssnr"][at(159)] == 0.0 and s["stoi"][at(400)] == 0.0 and s["pesq"][at(511)] == 1.0
    assert s["pesq"][3] < 1.2 and s["pesq"][6] > 4.0                    # the huge LSD of the zeroed stretch; exact-zero bins


def test_float32_dft_error_is_small_and_the_bound_follows_from_it(pesq_bound):
    assert 1e-8 < pesq_bound / K_TRANS < 1e-6 and pesq_bound < 2e-5


# ---------------------------------------------------------------------------
# frame-offset tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [ec.LENGTHS, ec.LENGTHS[::-1], [129], [159, 129, 2000, 130], [0, 5, 700]])
def test_metric_frame_counts_against_a_direct_count(lengths):
    for m, (frame, hop) in ec.FRAMINGS.items():
        n = Fn.metric_frame_counts(lengths, frame, hop)
        assert n.dtype == np.int64 and n.tolist() == [ec.frame_count(L, frame, hop) for L in lengths], m
    with pytest.raises(ValueError):
        Fn.metric_frame_counts(lengths, 0, 80)
    with pytest.raises(ValueError):
        Fn.metric_frame_counts(lengths, 160, 0)


def test_metric_framings_follow_the_sample_rate():
    assert pk.metric_framings(16000) == ec.FRAMINGS
    assert pk.metric_framings(8000) == {"ssnr": (160, 80), "stoi": (204, 102), "pesq": (256, 128)}
    assert pk.metric_framings() == pk.metric_framings(8000)


def test_metric_tables_layout_and_cache():
    (seg,) = Fn.packed_segments(ec.LENGTHS)
    fr = tuple(ec.FRAMINGS[m] for m in ec.METRICS)
    tabs = seg.metric_tables("cpu", fr)
    for m in ec.METRICS:
        t = tabs[ec.FRAMINGS[m]]
        want = [ec.frame_count(L, *ec.FRAMINGS[m]) for L in ec.LENGTHS]
        assert t["frame_off"].dtype == torch.int32 and t["frame_off"].tolist() == np.concatenate([[0], np.cumsum(want)]).tolist()
        assert t["counts"].tolist() == want and t["n"].tolist() == want and t["sum"] == sum(want)
        # no frame reaches past its utterance's last sample
        assert all(n == 0 or (n - 1) * ec.FRAMINGS[m][1] + ec.FRAMINGS[m][0] <= L for n, L in zip(want, ec.LENGTHS))
    again = seg.metric_tables("cpu", fr[:1])
    assert again[fr[0]]["frame_off"] is tabs[fr[0]]["frame_off"]                # cached next to tables()
    with pytest.raises(ValueError):
        Fn.PackedSegments([3, 4]).metric_tables("cpu", fr)


# ---------------------------------------------------------------------------
# the host part of evaluate_batch
# ---------------------------------------------------------------------------
def test_plan_trims_pairs_validates_and_builds_the_passes(case):
    c, x, e, _ = case
    longer = [np.concatenate([a, np.ones(7, np.float32)]) for a in x]
    cl, no, passes = pk.plan_evaluation(c, longer)
    assert [a.size for a in cl] == [a.size for a in no] == ec.LENGTHS and all(np.array_equal(a, b) for a, b in zip(no, x))
    assert len(passes) == 1 and passes[0].lengths.tolist() == ec.LENGTHS
    cl, no, _ = pk.plan_evaluation([torch.from_numpy(c[0]), c[1][:500]], [x[0][:300], torch.from_numpy(x[1])])
    assert [a.size for a in cl] == [a.size for a in no] == [300, 500] and cl[0].dtype == np.float32
    frames = [1 + L // 80 for L in ec.LENGTHS]
    three = pk.plan_evaluation(c, x, max_frames=sum(frames) // 2)[2]
    assert len(three) == 3 and [p.start for p in three] == [0, 9, 10] and three[-1].stop == 12
    assert pk.plan_evaluation([], []) == ([], [], [])
    with pytest.raises(ValueError, match=r"signal 1 .*L=128"):           # the error enhance_batch raises, after the trim
        pk.plan_evaluation([c[0], c[1]], [x[0], x[1][:128]])
    with pytest.raises(ValueError, match="pair up"):
        pk.plan_evaluation(c[:3], x[:2])
    with pytest.raises(ValueError, match="choose from"):
        pk._check_metrics(("stoi", "csii"))


# ---------------------------------------------------------------------------
# argument guards of the new entry points (validation happens before any HIP call)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib.load()


one = ctypes.c_void_p(16)


def _each_null(fn, nptr, tail):
    for i in range(nptr):
        ptrs = [one] * nptr
        ptrs[i] = None
        assert fn(*ptrs, *tail, None) == -1, i


def _each_bad(fn, nptr, tail, bad):
    for idx, val in bad:
        assert fn(*[one] * nptr, *[val if j == idx else v for j, v in enumerate(tail)], None) == -2, (idx, val)


def test_new_entry_points_refuse_null_pointers_and_bad_shapes_without_a_gpu(L):
    # sum_frames = 0 is the control: every check passes and nothing is launched
    ok = (3, 0, 160, 80, 35.0, -10.0)
    assert L.sfm_ssnr_frames_varlen(*[one] * 5, *ok, None) == 0
    _each_null(L.sfm_ssnr_frames_varlen, 5, ok)
    _each_bad(L.sfm_ssnr_frames_varlen, 5, ok, [(0, 0), (1, -1), (2, 0), (3, 0)])
    ok = (3, 0, 205)
    assert L.sfm_stoi_frames_varlen(*[one] * 8, *ok, None) == 0
    _each_null(L.sfm_stoi_frames_varlen, 8, ok)
    _each_bad(L.sfm_stoi_frames_varlen, 8, ok, [(0, 0), (1, -1), (2, 0)])
    assert L.sfm_lsd_frames_varlen(*[one] * 6, *ok, None) == 0
    _each_null(L.sfm_lsd_frames_varlen, 6, ok)
    _each_bad(L.sfm_lsd_frames_varlen, 6, ok, [(0, 0), (1, -1), (2, 0)])
    dense = (3, 10, 257)
    _each_null(L.sfm_lsd_frames, 5, dense)
    _each_bad(L.sfm_lsd_frames, 5, dense, [(0, 0), (1, 0), (2, 0)])
    mom = (3, 4000)
    _each_null(L.sfm_wave_moments_varlen, 4, mom)
    _each_bad(L.sfm_wave_moments_varlen, 4, mom, [(0, 0), (1, 0), (0, 2 ** 31 // 16)])     # 16 workgroups x B along grid x


def test_header_binding_and_library_agree_on_the_new_entry_points(L):
    import test_abi
    from sincformer_metacog_speech_enhancement_amd import lib
    decls = test_abi._header_decls()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for n in ("sfm_ssnr_frames_varlen", "sfm_stoi_frames_varlen", "sfm_lsd_frames", "sfm_lsd_frames_varlen", "sfm_wave_moments_varlen"):
        assert decls[n][1] == lib.SIGNATURES[n] and decls[n][0] is getattr(L, n).restype and hasattr(raw, n), n


# ---------------------------------------------------------------------------
# the GPU tests can fail: wrong packed computations move some utterance by >= 5 x the bound
# ---------------------------------------------------------------------------
def _moves(name, wrong, right, bounds):
    best = {m: float(np.max(np.abs(wrong[m] - right[m])) / bounds[m]) for m in wrong}
    print("MUTANT | %s | moves some utterance by %s x the bound" % (name, ", ".join("%s %.1e" % kv for kv in best.items())))
    return best


@pytest.mark.parametrize("mutant", ec.PACKED_MUTANTS)
def test_wrong_packed_framing_and_means_are_caught_by_every_measure(case, pesq_bound, mutant):
    c, x, e, right = case
    bounds = {"ssnr": ec.SSNR_BOUND, "stoi": ec.STOI_BOUND, "pesq": pesq_bound}
    best = _moves(mutant, ec.packed_mutant_scores(c, e, mutant), right, bounds)
    assert all(v >= 5.0 for v in best.values()), (mutant, best)


def test_the_mutant_generator_without_a_mutation_is_the_reference(case):
    """(a padded frame that does not exist changes nothing: on a set whose lengths all fit whole frames the mutant is the oracle)"""
    L = [160 + 80 * 7, 409 + 204 * 3, 512 + 256 * 2]
    c, x, e = ec.signals()
    for frame_metric, n in zip(("ssnr", "stoi", "pesq"), L):
        cc, ee = [c[9][:n]], [e[9][:n]]
        got = ec.packed_mutant_scores(cc, ee, "a last partial frame zero-padded and counted")[frame_metric]
        assert abs(got[0] - ec.scores64(cc, ee)[frame_metric][0]) < 1e-12, frame_metric
        same = ec.packed_mutant_scores(cc, ee, "the mean over max n_u")                    # one utterance: n_u is the maximum
        assert abs(same[frame_metric][0] - ec.scores64(cc, ee)[frame_metric][0]) < 1e-12


@pytest.mark.parametrize("mutant", ec.PESQ_MUTANTS)
def test_wrong_lsd_arithmetic_is_caught(case, pesq_bound, mutant):
    c, x, e, right = case
    wrong = np.array([ec.pesq_simplified64(a, b, ec.FS, mutant=mutant) for a, b in zip(c, e)])
    best = _moves(mutant, {"pesq": wrong}, right, {"pesq": pesq_bound})
    assert best["pesq"] >= 5.0, (mutant, best)


# ---------------------------------------------------------------------------
# the walk of the packed kernels: a wave that owns several consecutive frames flushes when the utterance changes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_values(case):
    """per distinct utterance: SSNR (clipped SNR, kept) per frame and the LSD per PESQ frame"""
    c, x, e, _ = case
    return [ec.ssnr_frame_values(a, b) for a, b in zip(c, e)], [ec.lsd_frames64(a, b, ec.FS) for a, b in zip(c, e)]


def _walked_scores(order, frame_values, mutant):
    sv, lv = frame_values
    ns = np.array([sv[i][0].size for i in order])
    nl = np.array([lv[i].size for i in order])
    waves = lambda total: 4 * min((total + 3) // 4, ec.MAX_WAVES // 4)
    ssum = ec.walk_sums(np.concatenate([sv[i][0] for i in order]), ns, waves(int(ns.sum())), mutant)
    scnt = ec.walk_sums(np.concatenate([sv[i][1].astype(np.float64) for i in order]), ns, waves(int(ns.sum())), mutant)
    lsum = ec.walk_sums(np.concatenate([lv[i] for i in order]), nl, waves(int(nl.sum())), mutant)
    return {"ssnr": np.where(scnt > 0, ssum / np.maximum(scnt, 1.0), 0.0),
            "pesq": np.where(nl > 0, np.clip(4.5 - 0.5 * lsum / np.maximum(nl, 1), -0.5, 4.5), 1.0)}


def test_the_long_pack_makes_every_wave_walk_several_utterances():
    for m, (frame, hop) in ec.FRAMINGS.items():
        small = [ec.frame_count(L, frame, hop) for L in ec.LENGTHS]
        n = [small[i] for i in ec.LONG_ORDER]
        per = ec.run_length(sum(n))
        assert ec.run_length(sum(small)) == 1 and per >= 5, (m, per)              # the 12-utterance set never walks
        assert n[0] == 0 and n[-1] == 0 and sum(1 for v in n if v == 0) >= 300     # empties at the head, inside, at the tail
        assert sum(1 for v in n if 0 < v < per) >= 300                             # utterances a run passes through entirely
    assert {m: ec.run_length(sum(ec.frame_count(ec.LENGTHS[i], *ec.FRAMINGS[m]) for i in ec.LONG_ORDER)) for m in ec.METRICS} == {
        "stoi": 7, "pesq": 5, "ssnr": 17}


def test_the_emulated_walk_gives_every_utterance_its_own_sums(case, frame_values):
    c, x, e, right = case
    for order in (list(range(12)), ec.LONG_ORDER):
        got = _walked_scores(order, frame_values, None)
        for m in ("ssnr", "pesq"):
            assert np.abs(got[m] - right[m][order]).max() <= ec.ACC_BOUND, m


@pytest.mark.parametrize("mutant", ec.WALK_MUTANTS)
def test_a_wrong_flush_is_caught_on_the_long_pack_and_only_there(case, frame_values, pesq_bound, mutant):
    c, x, e, right = case
    bounds = {"ssnr": ec.SSNR_BOUND, "pesq": pesq_bound}
    wrong = _walked_scores(ec.LONG_ORDER, frame_values, mutant)
    best = _moves(mutant, wrong, {m: right[m][ec.LONG_ORDER] for m in wrong}, bounds)
    assert all(v >= 5.0 for v in best.values()), (mutant, best)
    small = _walked_scores(list(range(12)), frame_values, mutant)                  # one frame per wave: the flush never runs
    assert all(np.abs(small[m] - right[m]).max() <= ec.ACC_BOUND for m in small)
