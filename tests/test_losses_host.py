"""CPU checks of the curriculum objectives: the restatement of tests/loss_cases.py against what the reference returned
(tests/golden/g15_losses.npz), the cases' clip counts and tie margins, wrong forms of the restatement, the band matrices, the
scheduler against g15_curriculum.json and the argument guards of the two entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import helpers as hp
import loss_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "g15_losses.npz"))


def _figures(name, fixture):
    """e32 and the fixture's distance from the float64 restatement, for the loss (absolute) and the gradient (figs)"""
    rows = lc.FIXTURE_GRAD_ROWS.get(name, slice(None))
    l64, g64 = lc.reference(name, 0, torch.float64)
    l32, g32 = lc.reference(name, 0, torch.float32)
    return (abs(float(l32) - float(l64)), hp.figs(g32[rows], g64[rows]), g64[rows],
            abs(float(fixture[name + ".loss"]) - float(l64)), hp.figs(torch.from_numpy(fixture[name + ".grad"]), g64[rows]))


@pytest.mark.parametrize("name", lc.FIXTURE_CASES)
def test_restatement_equals_the_reference(fixture, name):
    """float64 restatement against the reference's fp32 loss and gradient: within 4 x e32, e32 = float32 restatement against
    the float64 one (the reference in fp32 and the restatement in fp32 are two roundings of one formula)"""
    assert int(fixture[name + ".seed"]) == lc.CASES[name][4]
    e_loss, e_grad, _, d_loss, d_grad = _figures(name, fixture)
    print("ROW | %s | loss e32 %.2e fixture %.2e | grad e32 %.2e %.2e fixture %.2e %.2e" % ((name, e_loss, d_loss) + e_grad + d_grad))
    assert d_loss <= 4 * e_loss
    assert d_grad[0] <= 4 * e_grad[0] and d_grad[1] <= 4 * e_grad[1]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_cases_keep_their_clip_counts_and_tie_margin(name):
    """from the restatement alone: the clipped (band, segment) pairs are the ones the case was built to have, clipped and
    unclipped pairs both exist where any clips, and no pair is within 0.05 of the tie of min(1, ratio)"""
    clipped, pairs_, margin = lc.clip_report(name)
    print("ROW | %s | clipped %d of %d | min |ratio - 1| %.3f" % (name, clipped, pairs_, margin))
    assert (clipped, pairs_) == lc.CLIPPED[name]
    assert margin >= lc.TIE_MARGIN
    if clipped:
        assert 0 < clipped < pairs_


def test_case_shapes_are_the_documented_ones():
    shapes = {n: v[:3] for n, v in lc.CASES.items()}
    assert shapes == {"c1_one_segment": (1, 30, 129), "c2_tail_loud_flat": (2, 61, 129), "c3_five_tail_frames": (3, 95, 129),
                      "c4_empty_band_16k": (1, 30, 129), "c5_overlapping_bands": (2, 60, 257), "c6_all_zero": (2, 61, 129),
                      "c7_many_partials": (64, 120, 129)}
    w = lc.weights("c5_overlapping_bands")
    assert w.shape == (14, 257)
    assert all(int(((w[i] > 0) & (w[i + 1] > 0)).sum()) == 2 for i in range(13))          # neighbours share two bins
    assert int((lc.weights("c1_one_segment") > 0).sum(0).max()) == 1                      # the default rows never overlap
    c = lc.case("c6_all_zero")
    assert not c["enh"].any() and not c["clean"].any()


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_wrong_forms_miss_the_bound(fixture, mutant):
    """each plausible wrong form of the formula is farther than 4 x e32 from the reference's loss or gradient on at least
    one fixture case (a NaN counts as a miss)"""
    missed = []
    for name in lc.FIXTURE_CASES:
        rows = lc.FIXTURE_GRAD_ROWS.get(name, slice(None))
        e_loss, e_grad, g64, _, _ = _figures(name, fixture)
        lm, gm = lc.reference(name, 0, torch.float64, mutant=mutant)
        d_loss = abs(float(lm) - float(fixture[name + ".loss"]))
        d_grad = hp.figs(gm[rows], torch.from_numpy(fixture[name + ".grad"]))
        # the fixture itself is within 4 x e32 of the float64 form: a form farther than 8 x e32 from the fixture misses
        ok = d_loss <= 8 * e_loss and d_grad[0] <= 8 * e_grad[0] and d_grad[1] <= 8 * e_grad[1]
        if not ok:
            missed.append(name)
    print("ROW | mutant %s | misses on %s" % (mutant, missed))
    assert missed, mutant


def test_band_matrices_are_bit_equal(fixture):
    from sincformer_metacog_speech_enhancement_amd.training import PerceptualSTOILoss
    for sr in (8000, 16000):
        ref = fixture["band_weights_%d" % sr]
        for got in (PerceptualSTOILoss(sample_rate=sr).band_weights.numpy(), lc.band_matrix(sr)):
            assert got.dtype == np.float32 and got.shape == (14, 129)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    m = PerceptualSTOILoss()
    assert (m.num_bands, m.frame_len, m.beta) == (14, 30, 15.0)
    assert list(m.state_dict()) == ["band_weights"]
    assert [int(v) for v in (fixture["band_weights_8000"] > 0).sum(1)] == [1, 2, 1, 3, 3, 3, 5, 6, 7, 9, 12, 14, 18, 24]
    assert not fixture["band_weights_16000"][0].any()


def test_mse_restatement_equals_the_reference(fixture):
    p, t = lc.mse_case((2, 61, 129), int(fixture["mse.seed"]))
    p64 = p.double().requires_grad_(True)
    l64 = lc.mse(p64, t.double())
    l64.backward()
    p32 = p.clone().requires_grad_(True)
    l32 = lc.mse(p32, t)
    l32.backward()
    e_loss, e_grad = abs(float(l32) - float(l64)), hp.figs(p32.grad, p64.grad)
    d_loss, d_grad = abs(float(fixture["mse.loss"]) - float(l64)), hp.figs(torch.from_numpy(fixture["mse.grad"]), p64.grad)
    print("ROW | mse | loss e32 %.2e fixture %.2e | grad e32 %.2e %.2e fixture %.2e %.2e" % ((e_loss, d_loss) + e_grad + d_grad))
    assert d_loss <= max(4 * e_loss, 4 * 2.0 ** -24 * float(l64))
    assert d_grad[0] <= 4 * e_grad[0] and d_grad[1] <= 4 * e_grad[1]


def test_curriculum_scheduler_equals_the_reference():
    from sincformer_metacog_speech_enhancement_amd import config
    from sincformer_metacog_speech_enhancement_amd.training import CurriculumScheduler
    gold = json.load(open(os.path.join(GOLDEN, "g15_curriculum.json")))
    s = CurriculumScheduler()
    assert (config.CURRICULUM_STAGE1_EPOCHS, config.CURRICULUM_STAGE2_EPOCHS, config.CURRICULUM_STAGE3_EPOCHS) == (15, 20, 15)
    assert s.total_epochs == gold["total_epochs"] == 50
    assert len(gold["stages"]) == 50
    for e, want in enumerate(gold["stages"]):
        assert s.get_stage(e) == want, e
    assert [s.get_stage(e)["loss_type"] for e in (0, 15, 35)] == ["mse", "mse+perceptual", "perceptual+vq+adversarial"]


def test_print_schedule_names_every_stage(capsys):
    from sincformer_metacog_speech_enhancement_amd.training import CurriculumScheduler
    CurriculumScheduler().print_schedule()
    out = capsys.readouterr().out
    for text in ("Stage 1", "Stage 2", "Stage 3", "Epochs: 0 - 14", "Epochs: 15 - 34", "Epochs: 35 - 49"):
        assert text in out


def test_cpu_tensors_and_short_inputs_raise():
    from sincformer_metacog_speech_enhancement_amd.training import MSEMaskLoss, PerceptualSTOILoss
    x = torch.rand(1, 129, 30)
    with pytest.raises(RuntimeError, match="CPU"):
        PerceptualSTOILoss()(x, x)
    with pytest.raises(RuntimeError, match="CPU"):
        PerceptualSTOILoss().forward_cl(*([x.transpose(1, 2)] * 4))
    with pytest.raises(RuntimeError, match="CPU"):
        MSEMaskLoss()(x, x)


def test_argument_guards_without_a_gpu():
    """null pointers -> -1, unsupported shapes -> -2, both before any HIP call"""
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    L = lib.load()
    one = ctypes.c_void_p(16)

    def pstoi(e0=one, e1=None, c0=one, c1=None, w=one, loss=one, g0=None, g1=None, ws=one, B=2, T=61, F=129, NB=14, FL=30,
              layout=0):
        return L.sfm_pstoi_loss(e0, e1, c0, c1, w, loss, g0, g1, ws, B, T, F, NB, FL, 15.0, layout, None)
    for k in ("e0", "c0", "w", "loss", "ws"):
        assert pstoi(**{k: None}) == -1, k
    assert pstoi(layout=2) == -1
    assert pstoi(layout=1) == -1                                   # the pair form needs the imaginary parts
    assert pstoi(layout=1, e1=one, c1=one, g0=one) == -1           # ... and both gradients or neither
    assert pstoi(layout=0, g1=one) == -1
    for bad in (dict(T=29), dict(F=258), dict(NB=33), dict(B=0), dict(F=0), dict(NB=0), dict(FL=33), dict(FL=1),
                dict(T=31, FL=32)):
        assert pstoi(**bad) == -2, bad
        assert pstoi(layout=1, e1=one, c1=one, **bad) == -2, bad
    assert pstoi(B=2 ** 30, T=64, FL=2) == -2                      # B * S beyond the grid
    assert L.sfm_mse_loss(None, one, one, None, one, 8, None) == -1
    assert L.sfm_mse_loss(one, None, one, None, one, 8, None) == -1
    assert L.sfm_mse_loss(one, one, None, None, one, 8, None) == -1
    assert L.sfm_mse_loss(one, one, one, None, None, 8, None) == -1
    assert L.sfm_mse_loss(one, one, one, None, one, 0, None) == -2
