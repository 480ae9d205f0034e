"""CPU checks of the curriculum batches: the restatement of tests/mask_cases.py against what the reference returned
(tests/golden/g17_masks.npz), compute_snr_boundaries and the mix assignment against literals, the argument guards of the seven
entry points of csrc/masks.hip, the launch costs their wrappers state, and the share of the batch's PCIRM values that lie too
near a quantiser boundary for the quantised mask to be pinned (the condition of the GPU test of 'opt_pcirm')."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mask_cases as mc
import ops_stub

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASKS = ("irm", "pcirm")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "g17_masks.npz"))


@pytest.mark.parametrize("k", range(len(mc.UTTERANCES)))
def test_restatement_equals_the_reference_on_the_utterances(fixture, k):
    """float64 restatement against the reference's fp32 mix and masks of each utterance alone: within 16 x e32, e32 = the
    float32 restatement against the float64 one (the reference in fp32 and the restatement in fp32 are two roundings of one
    formula), never below 16 x 2^-24 of the row's largest value"""
    u = "u%d." % k
    clean, noise = mc.utterance(k)
    assert int(fixture[u + "seed"]) == mc.UTTERANCES[k][3]
    assert np.array_equal(fixture[u + "clean"], clean.numpy()) and np.array_equal(fixture[u + "noise"], noise.numpy())
    r64, r32 = mc.utterance_reference(k, torch.float64), mc.utterance_reference(k, torch.float32)
    peak = float(r64["noisy"].abs().max())
    mc.check(u + "noisy (fixture)", fixture[u + "noisy"], r64["noisy"], r32["noisy"], peak)
    mc.check(u + "scale (fixture)", fixture[u + "scale"], r64["scale"], r32["scale"], float(r64["scale"]))
    for m in MASKS:
        assert fixture[u + m].shape == (1 + mc.UTTERANCES[k][0] // mc.HOP, mc.FFT // 2 + 1)
        mc.check(u + m + " (fixture)", fixture[u + m], r64[m], r32[m])
    first, last = mc.SILENT_FRAMES[k]
    assert not r64["C"][first:last].abs().any() and bool(r64["C"][first - 1].abs().any()) and bool(r64["C"][last].abs().any())
    assert not fixture[u + "irm"][first:last].any()
    steps = fixture["steps"]
    for name, mid in (("opt", None), ("opt_mid", mc.MIDDLE_VALUE)):                # the quantiser on the reference's own PCIRM: exact
        assert np.array_equal(mc.quantize(torch.from_numpy(fixture[u + "pcirm"]), steps, mid).numpy(), fixture[u + name])


@pytest.mark.parametrize("name", list(mc.RANDOM))
def test_restatement_equals_the_reference_on_the_random_planes(fixture, name):
    assert int(fixture[name + ".seed"]) == mc.RANDOM[name][1]
    c = mc.random_case(name)
    assert tuple(c["cm"].shape) == mc.RANDOM[name][0] and c["cm"].shape[-1] % 2 == 1
    assert bool((c["pc"] == np.float32(np.pi)).any()) and bool((c["pc"] == -np.float32(np.pi)).any())
    r64, r32 = mc.random_reference(name, torch.float64), mc.random_reference(name, torch.float32)
    for m in ("irm", "irm_p", "rho_s", "rho_n", "pcirm"):
        mc.check("%s %s (fixture)" % (name, m), fixture[name + "." + m], r64[m], r32[m])
    steps = fixture["steps"]
    q = c["q"]
    s1 = np.float32(steps[1])
    for v in (0.0, 1.0, s1, np.nextafter(s1, np.float32(0)), np.nextafter(s1, np.float32(1))):
        assert bool((q == float(v)).any()), v
    assert bool(torch.isnan(q).any()) and bool((q < 0).any())
    for key, mid in (("opt", None), ("opt_mid", mc.MIDDLE_VALUE)):
        got = mc.quantize(q, steps, mid).numpy()
        assert np.array_equal(got, fixture[name + "." + key])
        values = np.array(steps, dtype=np.float64)
        if mid is not None:
            values[1] = mid
        assert set(np.unique(got)) == set(values.astype(np.float32))
        assert got[np.isnan(q.numpy())].max() == 0.0 and got[q.numpy() < 0].max() == 0.0
        assert (got[q.numpy() >= 1.0] == np.float32(values[-1])).all()


def test_snr_boundaries_equal_the_reference(fixture):
    from sincformer_metacog_speech_enhancement_amd import config, masks
    assert (config.LOCAL_CRITERION_DB, config.OPT_NUM_STEPS) == (-15, 3)
    for steps, exponent in (masks.compute_snr_boundaries(), mc.snr_boundaries()):
        assert steps.dtype == np.float64 and np.array_equal(steps, fixture["steps"])
        assert float(exponent) == float(fixture["exponent"])
    assert np.allclose(fixture["steps"], [0.0, 0.00399141, 0.1302108], rtol=0, atol=5e-9)
    assert abs(float(fixture["exponent"]) - 5.0278) < 5e-5
    steps5, _ = masks.compute_snr_boundaries(local_criterion_db=-10, num_steps=5)
    assert steps5.shape == (5,) and steps5[0] == 0.0 and bool(np.all(np.diff(steps5) > 0))
    with pytest.raises(NotImplementedError, match="PSO"):
        masks.compute_opt_pcirm(torch.zeros(2, 2))
    with pytest.raises(NotImplementedError, match="PSO"):
        masks.compute_opt_pcirm(torch.zeros(2, 2), use_pso=True)


def test_mix_assignment_is_the_data_sets_rule():
    """utterance i of the data set: noise i % 3, snr_levels[i % len]; literal tables for first_index 0 and 5"""
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import mix_assignment
    assert mix_assignment(7, 3, [-5, 0, 5, 10], 0) == ([0, 1, 2, 0, 1, 2, 0], [-5.0, 0.0, 5.0, 10.0, -5.0, 0.0, 5.0])
    assert mix_assignment(7, 3, [-5, 0, 5, 10], 5) == ([2, 0, 1, 2, 0, 1, 2], [0.0, 5.0, 10.0, -5.0, 0.0, 5.0, 10.0])
    assert mix_assignment(4, 2, [5, 10], 5) == ([1, 0, 1, 0], [10.0, 5.0, 10.0, 5.0])
    assert mix_assignment(3, 1, [0, 5, 10], 0) == ([0, 0, 0], [0.0, 5.0, 10.0])
    with pytest.raises(ValueError):
        mix_assignment(2, 3, [], 0)


def test_host_tensors_and_bad_arguments_raise():
    from sincformer_metacog_speech_enhancement_amd import masks
    from sincformer_metacog_speech_enhancement_amd.training import curriculum_batch, mix_at_snr, mix_batch
    x = torch.rand(2, 5, 129)
    for call in (lambda: masks.compute_irm(x, x), lambda: masks.compute_correlation_coefficients(x, x, x),
                 lambda: masks.compute_phase_differences(x, x, x), lambda: masks.compute_pcirm(x, x, x, x, x, x),
                 lambda: masks.compute_pcirm_from_signals(x, x, x, x, x, x, x, x),
                 lambda: masks.quantize_pcirm(x, mc.snr_boundaries()[0]),
                 lambda: masks.compute_opt_pcirm(x, use_pso=False),
                 lambda: mix_at_snr(torch.rand(2, 800), [torch.rand(100)], [0, 0], [5.0, 5.0]),
                 lambda: mix_batch(torch.rand(2, 800), [torch.rand(100)], [5, 10]),
                 lambda: curriculum_batch(torch.rand(2, 800), [torch.rand(100)], [5, 10], "irm")):
        with pytest.raises(RuntimeError, match="CPU"):
            call()
    with pytest.raises(ValueError):
        masks.compute_irm(x, x, p=0.0)
    with pytest.raises(ValueError, match="mask_type"):
        curriculum_batch(torch.rand(2, 800), [torch.rand(100)], [5, 10], "ibm")


def test_argument_guards_without_a_gpu():
    """null pointers and a non-positive exponent -> -1, sizes the kernels do not take -> -2, all before any HIP call"""
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    L = lib.load()
    one = ctypes.c_void_p(16)
    big = 2 ** 31

    def variants(fn, good, pointers):
        """every pointer argument nulled in turn -> -1"""
        for i in pointers:
            args = list(good)
            args[i] = None
            assert fn(*args) == -1, (fn.__name__, i)

    variants(L.sfm_mask_irm, (one, one, one, 8, 0.5, 1e-10, None), range(3))
    assert L.sfm_mask_irm(one, one, one, 8, 0.0, 1e-10, None) == -1
    assert L.sfm_mask_irm(one, one, one, 8, -1.0, 1e-10, None) == -1
    assert L.sfm_mask_irm(one, one, one, 0, 0.5, 1e-10, None) == -2
    assert L.sfm_mask_irm(one, one, one, big, 0.5, 1e-10, None) == -2
    variants(L.sfm_mask_corr, (one, one, one, one, one, 8, 1e-10, None), range(5))
    assert L.sfm_mask_corr(one, one, one, one, one, 0, 1e-10, None) == -2
    assert L.sfm_mask_corr(one, one, one, one, one, big, 1e-10, None) == -2
    variants(L.sfm_mask_pcirm, (one, one, one, one, one, one, one, 8, 1e-10, None), range(7))
    assert L.sfm_mask_pcirm(one, one, one, one, one, one, one, -3, 1e-10, None) == -2
    assert L.sfm_mask_pcirm(one, one, one, one, one, one, one, big, 1e-10, None) == -2
    variants(L.sfm_mask_quantize, (one, one, one, 8, 3, None), range(3))
    for M in (1, 0, 17):
        assert L.sfm_mask_quantize(one, one, one, 8, M, None) == -2
    assert L.sfm_mask_quantize(one, one, one, 0, 3, None) == -2
    assert L.sfm_mask_quantize(one, one, one, big, 3, None) == -2
    scale_ok = (one, one, one, one, one, None, one, one, 2, 800, 3, None)
    variants(L.sfm_mix_scale, scale_ok, (0, 1, 2, 3, 4, 6, 7))
    apply_ok = (one, one, one, one, None, one, one, None, 2, 800, 3, None)
    variants(L.sfm_mix_apply, apply_ok, (0, 1, 2, 3, 5, 6))
    for fn, ok in ((L.sfm_mix_scale, scale_ok), (L.sfm_mix_apply, apply_ok)):
        for B, Ln, n_noise in ((0, 800, 3), (2, 0, 3), (2, 800, 0), (-1, 800, 3), (65536, 8, 3), (40000, 60000, 3)):
            args = list(ok)
            args[8:11] = [B, Ln, n_noise]
            assert fn(*args) == -2, (fn.__name__, B, Ln, n_noise)

    def curr(cr=one, ci=one, nr=one, ni=one, scale=one, table=None, yr=one, yi=one, mask=one, B=2, T=11, F=129, kind=1, p=0.5,
             M=0):
        return L.sfm_curriculum_mask(cr, ci, nr, ni, scale, table, yr, yi, mask, B, T, F, kind, p, 1e-10, M, None)
    for k in ("cr", "ci", "nr", "ni", "scale", "yr", "yi", "mask"):
        assert curr(**{k: None}) == -1, k
    assert curr(kind=4) == -1 and curr(kind=-1) == -1
    assert curr(kind=3, M=3) == -1                                   # the quantised form needs its table
    assert curr(kind=1, p=0.0) == -1
    for bad in (dict(B=0), dict(T=0), dict(F=0), dict(B=70000, T=801, F=129), dict(B=2, T=70000, F=70000)):
        assert curr(**bad) == -2, bad
    for M in (1, 17):
        assert curr(kind=3, table=one, M=M) == -2


def test_launch_costs_of_the_new_wrappers(monkeypatch):
    """(symbol, family, flops, bytes, tag) of every launch, literals: each operand read once, each result written once"""
    from sincformer_metacog_speech_enhancement_amd import ops
    rec = ops_stub.install(monkeypatch)
    x = torch.zeros(2, 5, 129)                                       # n = 1290
    ops.mask_irm(x, x)
    ops.mask_corr(x, x, x)
    ops.mask_pcirm(x, x, x, x, x, x)
    ops.mask_quantize(x, torch.zeros(7, dtype=torch.float64), 3)
    clean = torch.zeros(2, 8000)
    bank, off = torch.zeros(300), torch.tensor([0, 100, 300], dtype=torch.int32)
    ids, snr = torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    scale = ops.mix_scale(clean, bank, off, ids, snr)
    ops.mix_apply(clean, bank, off, ids, scale)
    ops.mix_apply(clean, bank, off, ids, scale, want_rows=True)
    ops.curriculum_mask(x, x, x, x, scale, "pcirm")
    ops.curriculum_mask(x, x, x, x, scale, None)
    assert rec == [
        ("sfm_mask_irm", "mask_irm", 7740.0, 15480.0, None),
        ("sfm_mask_corr", "mask_corr", 18060.0, 25800.0, None),
        ("sfm_mask_pcirm", "mask_pcirm", 15480.0, 36120.0, None),
        ("sfm_mask_quantize", "mask_quantize", 0.0, 10320.0, None),
        ("sfm_mix_scale", "mix", 64000.0, 128000.0, "scale B2 L8000"),
        ("sfm_mix_apply", "mix", 32000.0, 192000.0, "apply B2 L8000 rows0"),
        ("sfm_mix_apply", "mix", 32000.0, 256000.0, "apply B2 L8000 rows1"),
        ("sfm_curriculum_mask", "curriculum_mask", 41280.0, 36120.0, "B2 T5 F129 kind2"),
        ("sfm_curriculum_mask", "curriculum_mask", 10320.0, 30960.0, "B2 T5 F129 kind0"),
    ]


def test_few_values_lie_near_a_quantiser_boundary():
    """The GPU test of 'opt_pcirm' pins the quantised mask wherever the float64 PCIRM of the padded batch is farther from every
    inner boundary than the PCIRM row's bound (16 x e32, at least 16 x 2^-24); the rest may fall on either side.  That rest
    must stay a small share or the test says little: at most 1 % of the mask, from the restatement alone."""
    r64, r32 = mc.batch_reference(torch.float64), mc.batch_reference(torch.float32)
    e32, bound = mc.abs_bound(r32["pcirm"], r64["pcirm"])
    steps = mc.snr_boundaries()[0]
    near = mc.near_boundary(r64["pcirm"], steps, bound)
    share = float(near.double().mean())
    print("ROW | pcirm near a boundary | e32 %.2e | margin %.2e | share %.4f %% (%d of %d)" % (e32, bound, 100 * share,
                                                                                               int(near.sum()), near.numel()))
    assert share <= 0.01
    lo, hi = mc.adjacent_values(r64["pcirm"], steps, steps)
    q = mc.quantize(r64["pcirm"], steps).double()
    assert bool(((q == lo) | (q == hi))[near].all())                  # (the two candidates hold the restatement's own value)
    assert len(torch.unique(q)) == 3
