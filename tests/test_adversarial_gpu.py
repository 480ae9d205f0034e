"""AdversarialLoss on the device against the float64 restatement of tests/adversarial_cases.py, run with the same call sequence
from the same seeded state (the spectral-norm vectors are far from converged after init, so the sequence is part of the result).

Bounds.  Loss: 4 x the largest relative error, over the cases, of the restatement's 16-bit emulation (W / sigma and every conv's
input rounded to the operand format) against its float64 form - computed on the CPU, never from the kernels; the factor covers
fp32 accumulation and its order on top of operand rounding.  Gradients (to `enhanced`, and every parameter's): relative RMSE
<= 3e-3 in fp16 and <= 2.6e-2 in bf16, the bounds tests/test_train_gpu.py holds the PerceptionAgent's conv stack to.
Spectral-norm vectors: 16 x the float32 restatement's own error against float64 (at least 16 x 2^-24: they are unit vectors).

The forward keeps every GEMM operand as a hi / lo pair of 16-bit words (three GEMMs per conv), so the kinks of LeakyReLU and of
the L1 feature term are decided as in fp32: with single 16-bit operands a few pre-activations per tensor take the other slope
and the gradient misses these bounds by 1e-2..1e-1 however exact the backward is (a float64 CPU emulation with only the operands
rounded shows the same).  With the exact forward and 16-bit operands in the backward alone that emulation gives at most 7.6e-4
(fp16) and 5.7e-3 (bf16) on these rows."""
import math

import pytest
import torch

import adversarial_cases as ac

pytestmark = pytest.mark.gpu

FMTS = {"f16": torch.float16, "bf16": torch.bfloat16}
GRAD_BOUND = {"f16": 3e-3, "bf16": 2.6e-2}
U32 = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module")
def mods():
    from sincformer_metacog_speech_enhancement_amd import ops, train
    from sincformer_metacog_speech_enhancement_amd.training import AdversarialLoss
    return {"ops": ops, "train": train, "adv": AdversarialLoss}


_refs, _emu = {}, {}


def ref(name, mode, dtype=torch.float64, **kw):
    """the restatement on a case from the seeded init: computed once, shared, never changed"""
    key = (name, mode, dtype) + tuple(sorted(kw.items()))
    if key not in _refs:
        c = ac.case(name)
        pair = (c["clean_re"], c["clean_im"], c["enh_re"], c["enh_im"]) if kw.pop("pair", False) else None
        _refs[key] = ac.run(ac.init_state(ac.CASES[name][0]), mode, c["clean"], c["enh"], dtype, pair=pair, **kw)
    return _refs[key]


def loss_bound(fmt, mode):
    if (fmt, mode) not in _emu:
        _emu[(fmt, mode)] = 4.0 * ac.emulation_error(FMTS[fmt], mode)
    return _emu[(fmt, mode)]


def module(mods, name, fmt, training=True):
    mods["ops"].set_compute_dtype(FMTS[fmt])
    torch.manual_seed(ac.INIT_SEED)
    m = mods["adv"](input_dim=ac.CASES[name][0]).cuda()
    return m.train() if training else m.eval()


def call(m, mode, clean, enh):
    return {"d": lambda: m.discriminator_loss(clean, enh), "g": lambda: m.generator_loss(enh),
            "fm": lambda: m.feature_matching_loss(clean, enh)}[mode]()


def call_cl(m, mode, cr, ci, er, ei):
    return {"d": lambda: m.discriminator_loss_cl(cr, ci, er, ei), "g": lambda: m.generator_loss_cl(er, ei),
            "fm": lambda: m.feature_matching_loss_cl(cr, ci, er, ei)}[mode]()


def run_gpu(mods, name, mode, fmt, grad_out=None, freeze=False, training=True, rows=slice(None)):
    m = module(mods, name, fmt, training)
    if freeze:
        for p in m.parameters():
            p.requires_grad_(False)
    c = ac.case(name)
    clean = c["clean"][rows].cuda().requires_grad_(True)
    enh = c["enh"][rows].cuda().requires_grad_(True)
    loss = call(m, mode, clean, enh)
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_out, device="cuda"))
    torch.cuda.synchronize()
    return m, loss.detach(), clean, enh


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


_gpu = {}


def gpu(mods, name, mode, fmt):
    """the device's plain step on a case: run once, shared by the parity tests, never changed"""
    if (name, mode, fmt) not in _gpu:
        _gpu[(name, mode, fmt)] = run_gpu(mods, name, mode, fmt)
    return _gpu[(name, mode, fmt)]


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("name", list(ac.CASES))
def test_loss_parity_and_gradient_routing(mods, name, mode, fmt):
    m, loss, clean, enh = gpu(mods, name, mode, fmt)
    e_loss = rel(loss, ref(name, mode)["loss"])
    print("ROW | %s %s %s | loss %.3e (bound %.3e)" % (name, mode, fmt, e_loss, loss_bound(fmt, mode)))
    assert e_loss <= loss_bound(fmt, mode)
    assert clean.grad is None
    assert (enh.grad is None) == (mode == "d")


def _gradient_parity(mods, name, mode, fmt, r, what):
    m, loss, clean, enh = gpu(mods, name, mode, fmt)
    worst = ("", 0.0)
    if mode != "d":
        worst = ("enhanced", ac.rel_rmse(enh.grad, r["grad"]))
        print("ROW | %s | %s %s %s | grad enhanced %.3e" % (what, name, mode, fmt, worst[1]))
    figs = {}
    for k, p in m.named_parameters():
        want = r["pgrads"][k]
        if want is None or not bool(want.any()):
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        assert p.grad is not None, k
        figs[k] = ac.rel_rmse(p.grad, want)
    kmax = max(figs, key=figs.get)
    print("ROW | %s | %s %s %s | worst parameter gradient %s %.3e" % (what, name, mode, fmt, kmax, figs[kmax]))
    assert worst[1] <= GRAD_BOUND[fmt]
    assert figs[kmax] <= GRAD_BOUND[fmt], (kmax, figs[kmax])


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("name", list(ac.CASES))
def test_gradient_parity_with_the_restatement(mods, name, mode, fmt):
    _gradient_parity(mods, name, mode, fmt, ref(name, mode), "float64")


def _state_errors(m, want64, want32):
    out = []
    sd = m.state_dict()
    for k in want64:
        if k.endswith(("weight_u", "weight_v")):
            e32 = float((want32[k].double() - want64[k]).abs().max())
            out.append((k, float((sd[k].double().cpu() - want64[k]).abs().max()), max(16 * e32, 16 * U32)))
    return out


@pytest.mark.parametrize("mode,calls", [("d", 2), ("g", 1)])
@pytest.mark.parametrize("name", ["a1_odd_f9_t37", "a3_default_t64"])
def test_spectral_norm_vectors_after_the_calls(mods, name, mode, calls):
    """discriminator_loss calls every discriminator twice (two iterations), generator_loss once"""
    m, _, _, _ = run_gpu(mods, name, mode, "f16")
    errs = _state_errors(m, ref(name, mode)["state"], ref(name, mode, torch.float32)["state"])
    assert len(errs) == 2 * 13                                      # 5 + 4 + 4 convs
    for k, obs, bound in errs:
        assert obs <= bound, (k, obs, bound)
    other = ref(name, "g" if mode == "d" else "d")["state"]          # and the other call count is far outside it
    k = "discriminators.0.layers.0.weight_u"
    assert float((m.state_dict()[k].double().cpu() - other[k]).abs().max()) > 1e-3
    assert m.discriminator.layers[0].weight_u.data_ptr() == m.discriminators[0].layers[0].weight_u.data_ptr()


def test_eval_leaves_the_vectors_alone(mods):
    """after two training calls (at the raw init sigma = u^T W v of random u, v is ~1e-3 of its converged value and W / sigma is
    beyond fp16: the reference's own eval() loss there is 3.6e14), eval() iterates nothing and uses the vectors as they stand"""
    name = "a3_default_t64"
    m = module(mods, name, "f16")
    c = ac.case(name)
    state = ac.cast_state(ac.init_state(129), torch.float64)
    with torch.no_grad():
        for _ in range(2):
            m.generator_loss(c["enh"].cuda())
            ac.loss(state, "g", None, c["enh"].double())
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    enh = c["enh"].cuda().requires_grad_(True)
    loss = m.generator_loss(enh)
    loss.backward()
    d = m.discriminator_loss(c["clean"].cuda(), enh)
    torch.cuda.synchronize()
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    r = ac.run(state, "g", None, c["enh"], training=False)
    assert rel(loss.detach(), r["loss"]) <= loss_bound("f16", "g")
    assert ac.rel_rmse(enh.grad, r["grad"]) <= GRAD_BOUND["f16"]
    assert rel(d.detach(), ac.run(state, "d", c["clean"], c["enh"], training=False)["loss"]) <= loss_bound("f16", "d")
    assert all(torch.equal(r["state"][k], state[k]) for k in state)             # the restatement's eval moved nothing either


@pytest.mark.parametrize("mode", ["g", "fm"])
def test_frozen_discriminators_give_the_same_input_gradient(mods, mode):
    name = "a1_odd_f9_t37"
    m, loss, clean, enh = run_gpu(mods, name, mode, "f16")
    mf, loss_f, clean_f, enh_f = run_gpu(mods, name, mode, "f16", freeze=True)
    assert all(p.grad is None for p in mf.parameters()) and clean_f.grad is None
    assert any(p.grad is not None for p in m.parameters())
    assert torch.equal(enh.grad, enh_f.grad) and torch.equal(loss, loss_f)


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("shape", [(2, 9, 37, 16), (1, 129, 5, 256)])
def test_every_element_of_the_input_gradient_is_written(mods, shape, pair):
    """the staging adjoint's own output buffers, pre-filled with NaN: none is left, and the values are the padded rows'"""
    ops = mods["ops"]
    B, F, T, Cp = shape
    g = torch.Generator().manual_seed(11)
    d = torch.randn(B, T, Cp, generator=g).cuda()
    re, im = torch.randn(B, T, F, generator=g).cuda(), torch.randn(B, T, F, generator=g).cuda()
    dx = torch.full((B, T, F) if pair else (B, F, T), NAN, device="cuda")
    dxi = torch.full((B, T, F), NAN, device="cuda") if pair else None
    p = ops._p
    rc = ops._lib.load().sfm_adv_stage_bwd(p(d), p(re) if pair else None, p(im) if pair else None, p(dx), p(dxi), None, 0.0, B, F, T, Cp, pair,
                                           ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    if pair:
        mag = torch.sqrt(re * re + im * im + 1e-8)
        assert torch.allclose(dx, d[:, :, :F] * re / mag, rtol=1e-5, atol=1e-7)
        assert torch.allclose(dxi, d[:, :, :F] * im / mag, rtol=1e-5, atol=1e-7)
    else:
        assert torch.equal(dx, d[:, :, :F].transpose(1, 2))


@pytest.mark.parametrize("n", [4 * 256 + 4, 2048 * 4 * 256 + 4])
def test_leaky_feature_term_partials(mods, n):
    """sfm_adv_leaky with z_real, called directly: one quad past one workgroup's share of a pass (256 threads x 4), and one quad
    past the share of the 2048 workgroups its grid is capped at.  loss += scale x sum |leaky(z) - leaky(z_real)|, the terms in
    fp32 (two products by the slope and a difference: three roundings of values no larger than |leaky(z)| + |leaky(z_real)|),
    the sum in float64 in a fixed order: within 4 x 2^-24 x scale x sum (|leaky(z)| + |leaky(z_real)|) of the float64 value,
    the factor this suite gives rows that only add and multiply; and the same bits from run to run."""
    ops = mods["ops"]
    ops.set_compute_dtype(torch.float16)
    g = torch.Generator().manual_seed(177)
    z, zr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    scale, start = 0.37, 1.5
    leaky = lambda t: torch.where(t > 0, t.double(), 0.2 * t.double())
    want = start + scale * float((leaky(z) - leaky(zr)).abs().sum())
    bound = 4 * U32 * scale * float((leaky(z).abs() + leaky(zr).abs()).sum())
    got = []
    for _ in range(2):
        loss = torch.full((1,), start, device="cuda", dtype=torch.float64)
        a16, _ = ops.adv_leaky(z.cuda(), zr.cuda(), loss, scale)
        got.append(float(loss))
    print("ROW | adv_leaky n %d | bound %.3e | observed %.3e" % (n, bound, abs(got[0] - want)))
    assert abs(got[0] - want) <= bound and got[0] == got[1]
    assert torch.equal(a16.cpu(), torch.where(z > 0, z, 0.2 * z).half())


@pytest.mark.parametrize("fmt", list(FMTS))
def test_head_weight_gradient_over_two_chunks(mods, fmt):
    """sfm_adv_head_bwd with the weight gradient, called directly at B T = 65: one row past the 64 rows of a chunk, so two
    partial rows [3 C + 1] are folded.  dw, db and da against float64 on the same 16-bit operands, within this file's gradient
    bound; an utterance boundary falls inside the first chunk (the taps must not cross it)."""
    ops = mods["ops"]
    ops.set_compute_dtype(FMTS[fmt])
    B, T, C = 5, 13, 8
    g = torch.Generator().manual_seed(178)
    a16 = torch.randn(B, T, C, generator=g).to(FMTS[fmt])
    w16 = (0.3 * torch.randn(3, C, generator=g)).to(FMTS[fmt])
    out = torch.randn(B, T, generator=g)
    gin, coef, target = torch.tensor([0.7]), 0.25, 1.0
    da, dwb = ops.adv_head_bwd(a16.cuda(), w16.reshape(-1).cuda(), out.cuda(), gin.cuda(), coef, 1.0, target, True)
    dout = (float(gin) * coef) * (out.double() - target)                                  # [B, T]
    ap = torch.nn.functional.pad(a16.double(), (0, 0, 1, 1))                                # [B, T + 2, C]
    dw = torch.stack([(dout.unsqueeze(-1) * ap[:, tap:tap + T]).sum((0, 1)) for tap in range(3)])
    dp = torch.nn.functional.pad(dout, (1, 1))
    da64 = sum(dp[:, 2 - tap:2 - tap + T].unsqueeze(-1) * w16.double()[tap] for tap in range(3))
    figs = {"dw": ac.rel_rmse(dwb[:3 * C].cpu().reshape(3, C), dw), "db": rel(dwb[3 * C], dout.sum())}
    S = 2.0 ** (6 - math.frexp(abs(float(gin)) * 1.0)[1])                                  # the pass's scale: |g cnorm| S in [32, 64)
    figs["da"] = ac.rel_rmse(da.cpu() / S, da64)
    print("ROW | adv_head_bwd B T 65 %s | %s (bound %.1e)" % (fmt, {k: "%.2e" % v for k, v in figs.items()}, GRAD_BOUND[fmt]))
    assert max(figs.values()) <= GRAD_BOUND[fmt], figs


def test_no_poison_reaches_the_gradients(mods):
    """the allocator's free blocks are filled with NaN before the step: whatever the step leaves unwritten would show"""
    name = "a1_odd_f9_t37"
    junk = [torch.full((n,), NAN, device="cuda") for n in (1 << 20, 1 << 18, 1 << 16, 1 << 14, 4096, 1024) for _ in range(4)]
    del junk
    m, loss, clean, enh = run_gpu(mods, name, "fm", "f16")
    assert math.isfinite(float(loss)) and bool(torch.isfinite(enh.grad).all()) and bool((enh.grad != 0).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("mode", ac.MODES)
def test_two_runs_are_bitwise_equal(mods, mode):
    name = "a3_default_t64"
    a = run_gpu(mods, name, mode, "f16")
    b = run_gpu(mods, name, mode, "f16")
    assert torch.equal(a[1], b[1])
    if mode != "d":
        assert torch.equal(a[3].grad, b[3].grad)
    for (k, p), q in zip(a[0].named_parameters(), b[0].parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for k, v in a[0].state_dict().items():
        assert torch.equal(v, b[0].state_dict()[k]), k


@pytest.mark.parametrize("mode", ["g", "fm"])
def test_an_incoming_gradient_of_4096_scales_the_gradient(mods, mode):
    name = "a3_default_t64"
    m, _, _, enh = run_gpu(mods, name, mode, "f16", grad_out=4096.0)
    m1, _, _, enh1 = gpu(mods, name, mode, "f16")
    assert ac.rel_rmse(enh.grad / 4096.0, enh1.grad) <= GRAD_BOUND["f16"]
    for (k, p), q in zip(m.named_parameters(), m1.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert ac.rel_rmse(p.grad / 4096.0, q.grad) <= GRAD_BOUND["f16"], k


@pytest.mark.parametrize("mode", ["g", "fm"])
def test_an_utterance_alone_gets_its_share_of_the_batch_gradient(mods, mode):
    name = "a2_shortest_t4"                                         # B 3: the mean's 1 / B
    _, _, _, enh = run_gpu(mods, name, mode, "f16")
    _, _, _, alone = run_gpu(mods, name, mode, "f16", rows=slice(0, 1))
    assert ac.rel_rmse(enh.grad[:1], alone.grad / 3.0) <= GRAD_BOUND["f16"]


@pytest.mark.parametrize("mode", ac.MODES)
def test_channels_last_pair_form(mods, mode):
    name = "a1_odd_f9_t37"
    c = ac.case(name)
    m = module(mods, name, "f16")
    cr, ci, er, ei = (c[k].cuda().requires_grad_(True) for k in ("clean_re", "clean_im", "enh_re", "enh_im"))
    loss = call_cl(m, mode, cr, ci, er, ei)
    loss.backward()
    m2 = module(mods, name, "f16")
    with torch.no_grad():
        mag_c, mag_e = ac.magnitudes(cr, ci).contiguous(), ac.magnitudes(er, ei).contiguous()
    loss2 = call(m2, mode, mag_c, mag_e)
    r = ref(name, mode, pair=True)
    assert rel(loss, loss2) <= loss_bound("f16", mode) and rel(loss, r["loss"]) <= loss_bound("f16", mode)
    assert cr.grad is None and ci.grad is None
    if mode == "d":
        assert er.grad is None and ei.grad is None
    else:
        assert ac.rel_rmse(er.grad, r["grad"][0]) <= GRAD_BOUND["f16"] and ac.rel_rmse(ei.grad, r["grad"][1]) <= GRAD_BOUND["f16"]


def test_non_contiguous_and_16_bit_inputs(mods):
    name = "a1_odd_f9_t37"
    c = ac.case(name)
    base = run_gpu(mods, name, "g", "f16")
    m = module(mods, name, "f16")
    enh = c["enh"].transpose(1, 2).contiguous().cuda().transpose(1, 2).requires_grad_(True)      # [B, F, T] view, strides swapped
    assert not enh.is_contiguous()
    loss = m.generator_loss(enh)
    loss.backward()
    assert torch.equal(loss, base[1]) and torch.equal(enh.grad, base[3].grad)
    m = module(mods, name, "f16")
    half = c["enh"].cuda().half().requires_grad_(True)
    loss = m.generator_loss(half)
    loss.backward()
    m2 = module(mods, name, "f16")
    same = half.detach().float().requires_grad_(True)
    loss2 = m2.generator_loss(same)
    loss2.backward()
    assert torch.equal(loss, loss2) and half.grad.dtype == torch.float16 and torch.equal(half.grad, same.grad.half())


def test_subdiscriminator_forward_returns_the_reference_layout(mods):
    name = "a1_odd_f9_t37"
    m = module(mods, name, "f16")
    c = ac.case(name)
    out, feats = m.discriminators[2](c["enh"].cuda())
    state = ac.cast_state(ac.init_state(9), torch.float64)
    with torch.no_grad():
        want, wfeats = ac.disc(state, 2, c["enh"].double(), True)
    assert out.shape == want.shape == (2, 1, 10) and [f.shape for f in feats] == [f.shape for f in wfeats]
    assert ac.rel_rmse(out, want) <= GRAD_BOUND["f16"]
    assert all(ac.rel_rmse(a, b) <= GRAD_BOUND["f16"] for a, b in zip(feats, wfeats))
    k = "discriminators.2.layers.0.weight_u"
    assert float((m.state_dict()[k].double().cpu() - state[k]).abs().max()) <= 16 * 16 * U32


def test_composition_with_the_enhancer_and_the_optimiser(mods):
    """a small SpeechEnhancer's output through generator_loss_cl + feature_matching_loss_cl reaches its parameters; three
    FlatAdamW steps on the discriminators lower discriminator_loss on the fixed batch (lr 1e-4: in the float64 restatement
    with torch.optim.AdamW the same steps take the loss 1.077 -> 0.811 -> 0.712 -> 0.667)"""
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    from sincformer_metacog_speech_enhancement_amd.optim import FlatAdamW
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import SpeechEnhancer
    name = "a3_default_t64"
    torch.manual_seed(5)
    model = SpeechEnhancer(n_freq=129, d_model=64, num_blocks=1, num_heads=2, d_ff=128, dropout=0.0)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, 99).items()})
    model.cuda().train()
    adv = module(mods, name, "f16")
    mods["ops"].reset_precision()                                   # the enhancer and the objective in the training default
    c = ac.case(name)
    cr, ci, nr, ni = (c[k].cuda() for k in ("clean_re", "clean_im", "enh_re", "enh_im"))
    er, ei, _ = model(nr, ni)
    for p in adv.parameters():
        p.requires_grad_(False)                                     # a generator step
    total = adv.generator_loss_cl(er, ei) + adv.feature_matching_loss_cl(cr, ci, er, ei)
    total.backward()
    assert math.isfinite(float(total))
    got = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(got) > 10 and all(bool(torch.isfinite(g).all()) for g in got) and sum(float(g.abs().sum()) for g in got) > 0
    assert all(p.grad is None for p in adv.parameters())
    for p in adv.parameters():
        p.requires_grad_(True)
    opt = FlatAdamW(adv.parameters(), lr=1e-4, betas=(0.9, 0.98), weight_decay=0.01, max_norm=5.0)
    er, ei = er.detach(), ei.detach()
    hist = []
    for _ in range(4):
        opt.zero_grad()
        loss = adv.discriminator_loss_cl(cr, ci, er, ei)
        hist.append(float(loss))
        loss.backward()
        opt.step(loss=loss)
    print("ROW | discriminator_loss over three steps | %s" % " ".join("%.4f" % v for v in hist))
    assert hist[3] < hist[0]
