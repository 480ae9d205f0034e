"""Curriculum batches on the device (csrc/masks.hip through masks/, training.mix_at_snr / mix_batch / curriculum_batch) against
the float64 restatement of tests/mask_cases.py and the reference's own results in tests/golden/g17_masks.npz.

Bounds come from the restatement alone, by the rule of tests/test_losses_gpu.py: e32 = the float32 evaluation of the
restatement on the CPU against the float64 one, on the same inputs; the device result within 16 x e32 in absolute error (masks
live in [0, 1] behind a sqrt and a division), never below 16 x 2^-24 of the row's largest value (1 for a mask, the largest
sample for a waveform or a spectrum).  Against the fixture, itself a float32 evaluation within that bound of the float64 one
(tests/test_masks_host.py), twice the bound.  The quantiser compares in double what numpy compares in double: exact.
Every row prints `ROW | name | e32 | bound | observed`; profiles/README.md keeps the table."""
import math
import os

import numpy as np
import pytest
import torch

import mask_cases as mc

pytestmark = pytest.mark.gpu
NAN = float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "g17_masks.npz"))


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd import functional, masks, ops, training
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline
    return {"masks": masks, "ops": ops, "training": training, "fn": functional, "pipe": conformer_pipeline}


@pytest.fixture(scope="module")
def batches(mods):
    """curriculum_batch of the padded fixture batch, once per mask type (shared: do not modify)"""
    clean, noises, snrs, lengths = mc.padded_batch()
    dev = [n.cuda() for n in noises]
    # utterance i gets noise i % 3 and snrs[i % 3]: the data set's rule hands each fixture utterance its own noise and SNR
    return {kind: mods["training"].curriculum_batch(clean.cuda(), dev, snrs, kind, lengths=lengths)
            for kind in ("irm", "pcirm", "opt_pcirm", None)}


def _dev(c, *names):
    return [c[n].cuda() for n in names]


@pytest.mark.parametrize("name", list(mc.RANDOM))
def test_drop_ins_on_the_random_planes(mods, fixture, name):
    m = mods["masks"]
    c = mc.random_case(name)
    r64, r32 = mc.random_reference(name, torch.float64), mc.random_reference(name, torch.float32)
    cm, nm, ym, py, pc, pn, rs, rn = _dev(c, "cm", "nm", "ym", "py", "pc", "pn", "rho_s", "rho_n")
    phi1, phi2 = m.compute_phase_differences(py, pc, pn)
    assert torch.equal(phi1.cpu(), c["pc"] - c["py"]) and torch.equal(phi2.cpu(), c["pn"] - c["py"])
    rho_s, rho_n = m.compute_correlation_coefficients(ym, cm, nm)
    got = {"irm": m.compute_irm(cm, nm), "irm_p": m.compute_irm(cm, nm, p=0.3), "rho_s": rho_s, "rho_n": rho_n,
           "pcirm": m.compute_pcirm(cm, nm, rs, rn, phi1, phi2)}
    for key, g in got.items():
        assert g.dtype == torch.float32 and g.shape == cm.shape and not g.requires_grad
        assert float(g.min()) >= 0.0 and float(g.max()) <= 1.0
        mc.check("%s %s" % (name, key), g, r64[key], r32[key])
        d = float((g.cpu().double() - torch.from_numpy(fixture[name + "." + key]).double()).abs().max())
        _, bound = mc.abs_bound(r32[key], r64[key])
        print("ROW | %s %s vs fixture | bound %.2e | observed %.2e" % (name, key, 2 * bound, d))
        assert d <= 2 * bound
    both = m.compute_pcirm_from_signals(ym, cm, nm, py, pc, pn, cm, nm)
    assert len(both) == 5 and torch.equal(both[1], rho_s) and torch.equal(both[2], rho_n)
    assert torch.equal(both[0], m.compute_pcirm(cm, nm, rho_s, rho_n, phi1, phi2))
    # exact zeros: a silent clean unit is masked out entirely, a silent noise unit with speech is kept entirely (to 1e-10 / c^2)
    z = (c["cm"] == 0) & (c["nm"] > 0)
    assert int(z.sum()) > 0 and bool((got["irm"].cpu()[z] == 0).all())
    # inputs that carry autograd history, and a non-contiguous view
    leaf = cm.clone().requires_grad_(True)
    assert not m.compute_irm(leaf * 1.0, nm).requires_grad
    t = cm.transpose(0, 2)
    assert not t.is_contiguous() and torch.equal(m.compute_irm(t, nm.transpose(0, 2)), got["irm"].transpose(0, 2))


@pytest.mark.parametrize("name", list(mc.RANDOM))
def test_quantiser_is_exactly_the_references(mods, fixture, name):
    m = mods["masks"]
    q = mc.random_case(name)["q"].cuda()
    steps = fixture["steps"]
    for key, mid in (("opt", None), ("opt_mid", mc.MIDDLE_VALUE)):
        out = torch.full_like(q, NAN)
        got = m.quantize_pcirm(q, steps, mid)
        assert got.dtype == torch.float32 and not bool(torch.isnan(got).any()) and out.shape == got.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), fixture[name + "." + key].view(np.uint32)), key
    opt, steps_out, middle = m.compute_opt_pcirm(q, use_pso=False)
    assert np.array_equal(steps_out, steps) and middle == steps[1]
    assert np.array_equal(opt.cpu().numpy(), fixture[name + ".opt"])
    # a misaligned contiguous view takes the scalar path: the same result
    flat = torch.empty(q.numel() + 1, device="cuda")
    flat[1:] = q.reshape(-1)
    assert flat[1:].data_ptr() % 16 != 0
    assert torch.equal(m.quantize_pcirm(flat[1:], steps), m.quantize_pcirm(q, steps).reshape(-1))
    five = mc.snr_boundaries(num_steps=5)[0]
    assert torch.equal(m.quantize_pcirm(q, five, 0.5).cpu(), mc.quantize(q.cpu(), five, 0.5))
    two = mc.snr_boundaries(num_steps=2)[0]
    assert torch.equal(m.quantize_pcirm(q, two, 0.5).cpu(), mc.quantize(q.cpu(), two, 0.5))     # M < 3: middle_value is ignored


@pytest.mark.parametrize("pad", [0, 1], ids=["L2403", "L2404"])
def test_mix(mods, fixture, pad):
    """scale and noisy against the restatement and the fixture; the padding is written as exact zeros; two runs are the same
    bits.  L = 2403 puts rows 1 and 2 off the 16-byte grid (scalar head and tail around the quads), L = 2404 keeps every row
    on it."""
    tr = mods["training"]
    clean, noises, snrs, lengths = mc.padded_batch()
    if pad:
        clean = torch.cat([clean, torch.zeros(clean.shape[0], pad)], dim=1)
    dev = [n.cuda() for n in noises]
    noisy, scale = tr.mix_at_snr(clean.cuda(), dev, [0, 1, 2], snrs, lengths=lengths)
    assert noisy.shape == clean.shape and scale.shape == (3,) and not noisy.requires_grad
    r64, r32 = mc.batch_reference(torch.float64), mc.batch_reference(torch.float32)
    L0 = r64["noisy"].shape[1]
    for k, (L, _, _, _) in enumerate(mc.UTTERANCES):
        peak = float(r64["noisy"][k].abs().max())
        bound = mc.check("mix noisy u%d L+%d" % (k, pad), noisy[k, :L0], r64["noisy"][k], r32["noisy"][k], peak)
        assert float((noisy[k, :L].cpu().double() - torch.from_numpy(fixture["u%d.noisy" % k]).double()).abs().max()) <= 2 * bound
        sb = mc.check("mix scale u%d L+%d" % (k, pad), scale[k], r64["scale"][k], r32["scale"][k], float(r64["scale"][k]))
        assert abs(float(scale[k]) - float(fixture["u%d.scale" % k])) <= 2 * sb
        assert bool((noisy[k, L:] == 0).all())
    again, scale2 = tr.mix_batch(clean.cuda(), dev, snrs, lengths=lengths)                   # the data set's rule gives the same rows
    assert torch.equal(again, noisy) and torch.equal(scale2, scale)
    # the kernel's own output buffers, pre-filled with NaN: every element written, the padding exactly 0
    ops, pipe = mods["ops"], mods["pipe"]
    bank = pipe.noise_bank(dev)
    assert bank is pipe.noise_bank(dev) and bank.offsets.tolist() == [0, 450, 5450, 6250]
    B, L = clean.shape
    out, rows = torch.full((B, L), NAN, device="cuda"), torch.full((B, L), NAN, device="cuda")
    ids = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    rc = ops._lib.load().sfm_mix_apply(ops._p(clean.cuda()), ops._p(bank.buffer), ops._p(bank.offsets), ops._p(ids), ops._p(lens),
                                       ops._p(scale), ops._p(out), ops._p(rows), B, L, 3, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out, noisy) and not bool(torch.isnan(rows).any())
    for k, (Lk, Ln, _, _) in enumerate(mc.UTTERANCES):
        tiled = noises[k].repeat(-(-Lk // Ln))[:Lk]
        assert torch.equal(rows[k, :Lk].cpu(), tiled) and bool((rows[k, Lk:] == 0).all())
    # the single-utterance form under the reference's name
    one = pipe._add_noise_at_snr(mc.utterance(0)[0].cuda(), dev[0], snrs[0])
    assert one.shape == (mc.UTTERANCES[0][0],)
    assert float((one.cpu().double() - torch.from_numpy(fixture["u0.noisy"]).double()).abs().max()) <= 2 * mc.abs_bound(
        r32["noisy"][0], r64["noisy"][0], float(r64["noisy"][0].abs().max()))[1]
    with pytest.raises(ValueError, match="noise_ids"):
        tr.mix_at_snr(clean.cuda(), dev, [0, 1, 3], snrs)
    with pytest.raises(ValueError, match="lengths"):
        tr.mix_at_snr(clean.cuda(), dev, [0, 1, 2], snrs, lengths=[1700, L + 1, 800])


def test_mix_of_more_than_one_chunk(mods):
    """L = 9001: three 4096-sample workgroups per utterance, the last one partial; a 7-sample noise wraps inside every quad"""
    tr = mods["training"]
    rng = np.random.RandomState(176)
    clean = torch.from_numpy((0.1 * rng.standard_normal((2, 9001))).astype(np.float32))
    noises = [torch.from_numpy((0.3 * rng.standard_normal(n)).astype(np.float32)) for n in (7, 4096)]
    lengths = [9001, 8193]
    clean[1, 8193:] = 0.0
    noisy, scale = tr.mix_batch(clean.cuda(), [n.cuda() for n in noises], [0.0, 10.0], first_index=2, lengths=lengths)
    for k in range(2):
        refs = [mc.mix(clean[k].to(dt), noises[k].to(dt), (0.0, 10.0)[k], lengths[k]) for dt in (torch.float64, torch.float32)]
        mc.check("mix noisy 3 chunks u%d" % k, noisy[k], refs[0][0], refs[1][0], float(refs[0][0].abs().max()))
        mc.check("mix scale 3 chunks u%d" % k, scale[k], refs[0][1], refs[1][1], float(refs[0][1]))
    noisy2, scale2 = tr.mix_batch(clean.cuda(), [n.cuda() for n in noises], [0.0, 10.0], first_index=2, lengths=lengths)
    assert torch.equal(noisy, noisy2) and torch.equal(scale, scale2)


@pytest.mark.parametrize("kind", ["irm", "pcirm"])
def test_curriculum_batch(mods, batches, kind):
    b = batches[kind]
    clean, noises, snrs, lengths = mc.padded_batch()
    r64, r32 = mc.batch_reference(torch.float64), mc.batch_reference(torch.float32)
    B, L = clean.shape
    T, F = 1 + L // mc.HOP, mc.FFT // 2 + 1
    assert b.noisy.shape == (B, L) and b.scale.shape == (B,)
    for t in (b.noisy_real, b.noisy_imag, b.clean_real, b.clean_imag, b.mask):
        assert t.shape == (B, T, F) and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad
    peak = float(r64["Y"].abs().max())
    mc.check("batch %s noisy_real" % kind, b.noisy_real, r64["Y"].real, r32["Y"].real, peak)
    mc.check("batch %s noisy_imag" % kind, b.noisy_imag, r64["Y"].imag, r32["Y"].imag, peak)
    cr, ci = mods["fn"].stft(clean.cuda(), mc.FFT, mc.HOP, mc.WIN)
    assert torch.equal(b.clean_real, cr) and torch.equal(b.clean_imag, ci)
    mc.check("batch %s mask" % kind, b.mask, r64[kind], r32[kind])
    noisy, scale = mods["training"].mix_batch(clean.cuda(), [n.cuda() for n in noises], snrs, lengths=lengths)
    assert torch.equal(b.noisy, noisy) and torch.equal(b.scale, scale)
    if kind == "irm":
        for k, (first, last) in enumerate(mc.SILENT_FRAMES):
            assert bool((b.mask[k, first:last] == 0).all()) and bool((b.mask[k, first - 1] != 0).any())
    # the frames past an utterance's samples hold nothing: spectra and mask exactly 0
    assert bool((b.noisy_real[2, 13:] == 0).all()) and bool((b.mask[2, 13:] == 0).all())
    assert float(b.mask.min()) >= 0.0 and float(b.mask.max()) <= 1.0


@pytest.mark.parametrize("kind", ["irm", "pcirm", "opt_pcirm", None])
def test_every_output_element_is_written(mods, batches, kind):
    """the fused kernel's own output buffers, pre-filled with NaN: none is left, and they hold what curriculum_batch returns"""
    ops, b = mods["ops"], batches[kind]
    clean, noises, _, lengths = mc.padded_batch()
    bank = mods["pipe"].noise_bank([n.cuda() for n in noises])
    ids = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    _, rows = ops.mix_apply(clean.cuda(), bank.buffer, bank.offsets, ids, b.scale, lens, want_rows=True)
    nr, ni = mods["fn"].stft(rows, mc.FFT, mc.HOP, mc.WIN)
    yr, yi, mask = (torch.full_like(nr, NAN) for _ in range(3))
    table, M = mods["masks"].opt_pcirm.quantizer_table(mc.snr_boundaries()[0], None, "cuda")
    B, T, F = nr.shape
    p = ops._p
    rc = ops._lib.load().sfm_curriculum_mask(p(b.clean_real), p(b.clean_imag), p(nr), p(ni), p(b.scale), p(table), p(yr), p(yi),
                                             p(mask) if kind else None, B, T, F, ops.MASK_KINDS[kind], 0.5, 1e-10, M, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(yr, b.noisy_real) and torch.equal(yi, b.noisy_imag) and not bool(torch.isnan(yr).any())
    if kind:
        assert torch.equal(mask, b.mask) and not bool(torch.isnan(mask).any())
    else:
        assert b.mask is None and bool(torch.isnan(mask).all())


def test_curriculum_batch_with_another_exponent(mods):
    clean, noises, snrs, lengths = mc.padded_batch()
    b = mods["training"].curriculum_batch(clean.cuda(), [n.cuda() for n in noises], snrs, "irm", lengths=lengths, p=0.3)
    mc.check("batch irm p 0.3 mask", b.mask, mc.batch_reference(torch.float64, 0.3)["irm"], mc.batch_reference(torch.float32, 0.3)["irm"])


@pytest.mark.parametrize("middle", [None, mc.MIDDLE_VALUE])
def test_quantised_batch(mods, batches, middle):
    """'opt_pcirm' equals the restatement's quantised mask wherever the float64 PCIRM is farther from every inner boundary than
    the PCIRM row's bound; the rest - at most 1 % of the mask - takes one of the two step values beside its boundary"""
    clean, noises, snrs, lengths = mc.padded_batch()
    b = batches["opt_pcirm"] if middle is None else mods["training"].curriculum_batch(
        clean.cuda(), [n.cuda() for n in noises], snrs, "opt_pcirm", lengths=lengths, middle_value=middle)
    r64, r32 = mc.batch_reference(torch.float64), mc.batch_reference(torch.float32)
    e32, bound = mc.abs_bound(r32["pcirm"], r64["pcirm"])
    steps = mc.snr_boundaries()[0]
    values = steps.copy()
    if middle is not None:
        values[1] = middle
    values32 = torch.from_numpy(values.astype(np.float32)).double()
    want = mc.quantize(r64["pcirm"], steps, middle).float().double()
    got = b.mask.cpu().double()
    near = mc.near_boundary(r64["pcirm"], steps, bound)
    share = float(near.double().mean())
    differ = int((got != want).sum())
    print("ROW | batch opt_pcirm middle %s | e32 %.2e | margin %.2e | near a boundary %.4f %% | differing %d of %d"
          % (middle, e32, bound, 100 * share, differ, got.numel()))
    assert share <= 0.01
    assert torch.equal(got[~near], want[~near])
    lo, hi = mc.adjacent_values(r64["pcirm"], steps, values32.tolist())
    assert bool(((got == lo) | (got == hi))[near].all())
    assert set(torch.unique(got).tolist()) == set(values32.tolist())
    assert torch.equal(b.noisy_real, batches["pcirm"].noisy_real)
    assert torch.equal(b.mask, mods["masks"].quantize_pcirm(batches["pcirm"].mask, steps, middle))      # the same PCIRM, quantised


def test_a_stage_one_step_runs_end_to_end(mods):
    """the README's stage-1 step: get_stage(epoch) -> curriculum_batch -> EnhancementPath in train() -> MSEMaskLoss on the
    magnitude of its complex mask, backpropagated; the target carries no gradient"""
    from sincformer_metacog_speech_enhancement_amd.training import CurriculumScheduler, MSEMaskLoss
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import EnhancementPath
    info = CurriculumScheduler().get_stage(0)
    assert info["loss_type"] == "mse" and info["use_soft_mask"]
    clean, noises, _, lengths = mc.padded_batch()
    batch = mods["training"].curriculum_batch(clean.cuda(), [n.cuda() for n in noises], info["snr_levels"], "irm", lengths=lengths)
    assert batch.mask.requires_grad is False
    pred = torch.rand_like(batch.mask).requires_grad_(True)          # any [B, T, F] prediction
    loss = MSEMaskLoss()(pred, batch.mask)
    loss.backward()
    assert math.isfinite(float(loss.detach())) and pred.grad is not None and bool((pred.grad != 0).any()) and batch.mask.grad is None
    torch.manual_seed(5)
    path = EnhancementPath(sample_rate=16000).cuda().train()
    out = path(batch.noisy, want=("mask", "spectrum"))
    pred = torch.sqrt(out["mask_real"] ** 2 + out["mask_imag"] ** 2 + 1e-8)
    assert pred.shape == batch.mask.shape and pred.requires_grad
    loss = MSEMaskLoss()(pred, batch.mask)
    assert math.isfinite(float(loss.detach()))
    loss.backward()
    grads = {k: p_.grad for k, p_ in path.named_parameters() if p_.grad is not None}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(k.startswith("msa.") and bool((g != 0).any()) for k, g in grads.items())
