"""Training the DNN from a frame set kept at 54 columns, on the device (csrc/features.hip sfm_context_moments, csrc/dnn.hip
sfm_dnn_layer_indexed and sfm_mse_gather_loss, csrc/optim.hip sfm_adam_l2_step, training/dnn_training.py) against the float64
restatements of tests/dnn_train_cases.py and the reference's captured values.  Needs a real MI355X: `pytest -m gpu`.

Bounds, none of them taken from the kernels:
  statistics     16 x e32, e32 = the reference's own float32 statistics against float64 (tests/test_dnn_train_host.py prints it).
  indexed rows   bit for bit: the staged rows against numpy's float32 arithmetic in the kernel's written order rounded once to 16
                 bits, the outputs against the context mode's on the frame's utterance alone.
  loss           16 x e32, e32 = nn.MSELoss in float32 on the CPU against float64, and no less than half a unit in the last place of
                 the float32 the loss is stored in.  dz: within 1 unit in the last place of the 16-bit rounding of float64.
  Adam           p, m, v within 16 x e32, e32 = torch.optim.Adam + clip_grad_norm_ in float32 on the CPU against float64; the norm
                 within 1e-6 relative.
  trajectory     device minus float64 (RMS and max) <= 4 x the same error of the operand-rounding emulation, as tests/test_dnn_gpu.py.
Each case prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import dnn_cases as dn
import dnn_train_cases as tc
import dropout_cases as dc

pytestmark = pytest.mark.gpu

FMTS = {"f16": torch.float16, "bf16": torch.bfloat16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_dnn_train.npz")


@pytest.fixture(scope="module")
def mods():
    from sincformer_metacog_speech_enhancement_amd import models, ops, optim, train, training
    return {"ops": ops, "models": models, "train": train, "training": training, "optim": optim}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def case():
    raws, masks = tc.frame_set()
    raw, mask = np.concatenate(raws), np.concatenate(masks)
    rows = tc.context_rows64(raw, tc.bounds())
    mean, std = tc.stats64(rows)
    return dict(raws=raws, masks=masks, raw=raw, mask=mask, rows=rows, mean=mean, std=std)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def frameset(mods, case, **stats):
    return mods["training"].FrameSet([dev(r) for r in case["raws"]], [dev(m) for m in case["masks"]], **stats)


def shuffled_index(M, seed):
    """repeats and -1 entries; the first entries cover the lone frame, the short utterances and both sides of row 128"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, tc.N_FRAMES, size=M)
    idx[: min(M, 6)] = np.array([0, 1, 3, 14, 156, 27])[: min(M, 6)]
    if M > 8:
        idx[rng.integers(6, M, size=max(1, M // 16))] = -1
        idx[7] = idx[6]
    return idx.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
def test_frameset_statistics(mods, golden, case):
    fs = frameset(mods, case)
    assert len(fs) == tc.N_FRAMES and fs.raw.shape == (tc.N_FRAMES, 54) and fs.mask.shape == (tc.N_FRAMES, 64)
    assert np.array_equal(fs.bounds.cpu().numpy(), tc.bounds()) and fs.bounds.dtype == torch.int32
    assert not hasattr(fs, "features") and fs.bytes_per_frame() == 4 * 54 + 4 * 64 + 8
    live = golden["ds.feat_std"] != 1.0
    em = float(np.abs(golden["ds.feat_mean"].astype(np.float64) - case["mean"]).max())
    es = float(np.abs(golden["ds.feat_std"].astype(np.float64) - case["std"])[live].max())
    dm = np.abs(fs.feat_mean.astype(np.float64) - case["mean"]).max()
    ds = np.abs(fs.feat_std.astype(np.float64) - case["std"])[live].max()
    print("statistics: mean |d| %.3e (e32 %.3e)  std |d| %.3e (e32 %.3e)" % (dm, em, ds, es))
    assert fs.feat_mean.dtype == np.float32 and fs.feat_std.dtype == np.float32 and fs.feat_mean.shape == (594,)
    assert dm <= 16 * em and ds <= 16 * es
    zero = np.arange(594) % 54 < 15
    assert (fs.feat_std[zero] == 1.0).all() and (fs.feat_mean[zero] == 0.0).all() and (fs.feat_std[~zero] != 1.0).all()
    again = frameset(mods, case)
    assert torch.equal(bits(fs.mean_dev), bits(again.mean_dev)) and torch.equal(bits(fs.std_dev), bits(again.std_dev))
    given = frameset(mods, case, feat_mean=golden["ds.feat_mean"], feat_std=golden["ds.feat_std"])
    assert given.feat_mean is golden["ds.feat_mean"] and np.array_equal(given.std_dev.cpu().numpy(), golden["ds.feat_std"])
    # the rows, for inspection: the Dataset's
    f, m = given.rows(np.arange(tc.N_FRAMES))
    assert np.abs(host(f) - golden["ds.features"]).max() < 2e-6 and np.array_equal(m.cpu().numpy(), golden["ds.masks"])
    f1, m1 = given[156]
    assert torch.equal(f1, f[156]) and torch.equal(m1, m[156]) and torch.equal(given[-1][0], f[156]) and torch.equal(given[-157][0], f[0])
    for bad in (157, -158):                                 # the sequence protocol: an iteration over the set ends
        with pytest.raises(IndexError):
            given[bad]
    # statistics handed over as device tensors (or anything but a numpy float32 vector) are copied to the host once
    from_dev = frameset(mods, case, feat_mean=fs.mean_dev, feat_std=fs.std_dev.double())
    for a, b in ((from_dev.feat_mean, fs.feat_mean), (from_dev.feat_std, fs.feat_std)):
        assert type(a) is np.ndarray and a.dtype == np.float32 and np.array_equal(a, b)
    # a padded batch with lengths packs to the same set
    T = max(tc.LENGTHS)
    praw, pmask = torch.zeros(5, T, 54, device="cuda"), torch.zeros(5, T, 64, device="cuda")
    for b, (r, k) in enumerate(zip(case["raws"], case["masks"])):
        praw[b, :len(r)], pmask[b, :len(k)] = dev(r), dev(k)
    padded = mods["training"].FrameSet.from_padded(praw, pmask, list(tc.LENGTHS))
    assert torch.equal(bits(padded.raw), bits(fs.raw)) and torch.equal(bits(padded.mean_dev), bits(fs.mean_dev))


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("N", [1024, 64])
def test_indexed_rows_against_the_context_mode(mods, golden, case, fmt, N):
    ops, dt = mods["ops"], FMTS[fmt]
    ops.set_compute_dtype(dt)
    fs = frameset(mods, case, feat_mean=golden["ds.feat_mean"], feat_std=golden["ds.feat_std"])
    (W,), (b,) = dn.params((594, N), 300 + N)
    pw = ops.pack_linear(dev(W), dev(b), k_pad_to=600)
    # the context mode on each utterance alone, and on no frames at all (a zero row)
    per_utt = [ops.dnn_layer(dev(r).reshape(1, -1, 54).contiguous(), pw, act="relu", context=5, mean=fs.mean_dev, std=fs.std_dev)
               for r in case["raws"]]
    mode2 = torch.cat(per_utt, dim=0)
    zero_row = ops.dnn_layer(dev(case["raws"][0]).reshape(1, -1, 54).contiguous(), pw, act="relu", context=5, mean=fs.mean_dev,
                             std=fs.std_dev, frames=torch.zeros(1, dtype=torch.int32, device="cuda"))
    # the staged rows in numpy's float32, in the kernel's written order: (x - mean) * (1 / std), clip, one rounding
    x = case["rows"].astype(np.float32)
    rs = np.float32(1.0) / golden["ds.feat_std"]
    staged = np.clip((x - golden["ds.feat_mean"]) * rs, np.float32(-10), np.float32(10))
    want16 = torch.zeros(tc.N_FRAMES + 1, 640, dtype=dt)
    want16[:tc.N_FRAMES, :594] = torch.from_numpy(staged).to(dt)
    alone = {}
    for M in (157, 1, 37, 127, 128, 129):
        idx = shuffled_index(M, 40 + M) if M != 157 else np.random.default_rng(7).permutation(157).astype(np.int32)
        out, a16 = ops.dnn_layer_indexed(fs.raw, fs.bounds, dev(idx, torch.int32), pw, context=5, act="relu", mean=fs.mean_dev,
                                         std=fs.std_dev, a16_out=torch.full((M, 640), float("nan"), device="cuda", dtype=dt))
        plain = ops.dnn_layer_indexed(fs.raw, fs.bounds, dev(idx, torch.int32), pw, context=5, act="relu", mean=fs.mean_dev, std=fs.std_dev)
        torch.cuda.synchronize()
        tag = "%s N%d M%d" % (fmt, N, M)
        src = torch.from_numpy(np.where(idx < 0, tc.N_FRAMES, idx).astype(np.int64))
        assert a16.shape == (M, 640) and (host(a16)[:, 594:] == 0).all(), tag
        assert torch.equal(bits(a16), bits(want16[src])), tag
        expect = torch.cat([mode2, zero_row], dim=0).cpu()[src]
        assert torch.equal(bits(out), bits(expect)), tag
        assert torch.equal(bits(plain), bits(out)), tag                               # with and without the staged rows written
        for m, f in enumerate(idx):
            if M == 157:
                alone[int(f)] = bits(out[m])
            elif f >= 0:
                assert torch.equal(bits(out[m]), alone[int(f)]), (tag, m)             # a row alone or inside any M
    print("indexed rows %s N%d: staged rows and outputs equal the context mode's bit for bit at M = 1 .. 157" % (fmt, N))


def loss_bound(y32, t32, exact):
    e32 = abs(float(torch.nn.MSELoss()(torch.from_numpy(y32), torch.from_numpy(t32))) - exact)
    return 16 * max(e32, 2.0 ** -25 * exact)


def ulp_distance(got, want):
    """16-bit patterns as ordered integers (sign-magnitude -> two's complement)"""
    def ordered(t):
        v = t.view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7fff), v)
    return (ordered(got) - ordered(want)).abs()


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_loss_kernel(mods, case, fmt):
    ops, dt = mods["ops"], FMTS[fmt]
    ops.set_compute_dtype(dt)
    mask = dev(case["mask"])
    special = np.array([16 + 11 + 3, 27 + 64, 15 + 2, 1, 156])                       # the frames of the five special mask values
    assert not np.isfinite(case["mask"][special[:3]]).all() and case["mask"][1, 0] > 1 and case["mask"][156, 63] < 0
    scale = mods["optim"].DynamicLossScale("cuda")
    rec = torch.zeros(4, device="cuda", dtype=torch.float64)
    ctl = torch.zeros(8, device="cuda", dtype=torch.float64)
    losses = []
    for k, M in enumerate((9, 37, 256, 37, 9)):
        rng = np.random.default_rng(60 + k)
        idx = rng.integers(0, tc.N_FRAMES, size=M).astype(np.int32)
        idx[:5] = special
        y = dn.sigmoid(rng.standard_normal((M, 64)) * 2.0).astype(np.float32)
        t = tc.targets64(case["mask"][idx])
        for S, ls in ((tc.INIT_SCALE, scale.state), (1.0, None)):
            exact, dz64 = tc.loss_dz64(y.astype(np.float64), t, S)
            r = rec if ls is not None else None
            loss, dz = ops.mse_gather_loss(dev(y), mask, dev(idx, torch.int32), loss_scale=ls, rec=r, ctl=ctl)
            torch.cuda.synchronize()
            d = abs(float(loss) - exact)
            bound = loss_bound(y, t.astype(np.float32), exact)
            dist = ulp_distance(dz.cpu()[:, :64], torch.from_numpy(dz64).to(dt))
            print("loss %s M%d S%g: |d| %.3e (bound %.3e)  dz max ulp distance %d" % (fmt, M, S, d, bound, int(dist.max())))
            assert d <= bound and int(dist.max()) <= 1 and dz.shape == (M, 64) and dz.dtype == dt
        losses.append(float(loss))
        none, no_dz = ops.mse_gather_loss(dev(y), mask, dev(idx, torch.int32), need_dz=False)
        assert no_dz is None and float(none) == float(loss)
    got = rec.cpu().numpy()
    assert got[1] == 5 and got[2] == 0 and abs(got[3] - losses[-1]) < 1e-7
    assert abs(got[0] / got[1] - tc.epoch_loss(losses)) < 1e-7 and float(ctl[2]) == 0.0        # the mean of the per-batch means
    # a nan in y: the flag is raised, the batch counts as non-finite and the finite sum is untouched
    y[3, 7] = np.nan
    before = rec.clone()
    ops.mse_gather_loss(dev(y), mask, dev(idx, torch.int32), loss_scale=scale.state, rec=rec, ctl=ctl)
    after = rec.cpu().numpy()
    assert float(ctl[2]) == 1.0 and after[0] == float(before[0]) and after[1] == 5 and after[2] == 1 and np.isnan(after[3])


def test_underflow_share_under_the_initial_scale(mods, golden, case):
    """fp16, the fixture's first batch: of the dz elements that are non-zero in float64, at most 1e-3 are written as 0 or as a
    subnormal under the initial scale (a condition; tests/test_dnn_train_host.py records what S = 1 gives)"""
    ops = mods["ops"]
    ops.set_compute_dtype(torch.float16)
    fs = frameset(mods, case, feat_mean=golden["ds.feat_mean"], feat_std=golden["ds.feat_std"])
    Ws, bs = tc.fixture_params()
    m = mods["models"].SpeechEnhancementDNN(594, 64, 64, 3)
    m.load_state_dict(dn.state_dict(Ws, bs))
    m = m.cuda().eval()
    idx = dev(tc.batches()[0], torch.int32)
    y = m.forward_indexed(fs, idx)
    scale = mods["optim"].DynamicLossScale("cuda")
    assert scale.get_scale() == tc.INIT_SCALE
    _, dz = ops.mse_gather_loss(y, fs.mask, idx, loss_scale=scale.state)
    _, dz64 = tc.loss_dz64(host(y), tc.targets64(case["mask"][:tc.BATCH]), 1.0)
    live = dz64 != 0
    share = float(np.mean(np.abs(host(dz))[live] < 2.0 ** -14))
    print("underflow: %d live elements, share written as 0 or subnormal under S = %g: %.2e" % (live.sum(), tc.INIT_SCALE, share))
    assert share <= 1e-3


@pytest.mark.parametrize("wd", tc.ADAM_DECAYS)
def test_flat_adam(mods, golden, wd):
    """5 steps on the gradients of the fixture's five batches at its initial parameters (dnn_train_cases.adam_case; norms on both
    sides of the clip), the third one skipped by the flag, at the reference's decay 1e-5 and at 0.1.  At 1e-5 the decay term is too
    small for these bounds to tell a norm taken with it from one taken without; at 0.1 they do, and the decoupled decay fails at
    both (tests/test_dnn_train_host.py evaluates this very assertion, dnn_train_cases.adam_within, on the mutants).
    The norms are compared with the float64 restatement's: these gradients are not those of the captured trajectory, and the
    restatement is pinned to the reference's captured norms (to 1e-5, the float32 reference's own accuracy) in the host test."""
    optim = mods["optim"]
    p0, grads = tc.adam_case(golden["ds.features"], golden["ds.masks"])
    like = tc.interleave(*tc.fixture_params())
    e32 = tc.adam_e32(p0, grads, wd)
    *want, norms = tc.adam_run64(p0, grads, wd)
    assert any(n > tc.MAX_NORM for n in norms) and any(n < tc.MAX_NORM for n in norms) and norms[0] > tc.MAX_NORM
    S = tc.INIT_SCALE
    runs, got_norms = [], []
    for _ in range(2):
        params = [torch.nn.Parameter(dev(a)) for a in like]
        opt = optim.FlatAdam(params, lr=tc.LR) if wd == tc.WD else optim.FlatAdam(params, lr=tc.LR, weight_decay=wd)
        assert (opt.betas, opt.eps, opt.weight_decay, opt.max_norm) == ((0.9, 0.999), 1e-8, wd, 5.0)
        scale = optim.DynamicLossScale("cuda")
        got_norms = []
        for k, g in enumerate(grads):
            opt.zero_grad()
            opt.sync.flat.copy_(dev(g) * S)                 # the gradients, by hand, under the scale
            if k == tc.ADAM_SKIP:
                before = [opt.flat_p.clone(), opt.m.clone(), opt.v.clone()]
                opt.ctl[2] = 1.0
            opt.step(scaler=scale)
            s = opt.stats()
            got_norms.append(s["grad_norm"])
            assert s["skipped"] == (k == tc.ADAM_SKIP), (k, s)
            if k == tc.ADAM_SKIP:
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, (opt.flat_p, opt.m, opt.v))) and s["step"] == 2
                assert scale.stats() == {"scale": S / 2, "clean_steps": 0, "skipped_inf": 0, "skipped_loss": 1}
                S = S / 2
        assert opt.stats()["step"] == 4 and all(pp.data_ptr() >= opt.flat_p.data_ptr() for pp in params)
        runs.append([opt.flat_p.clone(), opt.m.clone(), opt.v.clone()])
        S = tc.INIT_SCALE
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b))                                          # run to run
    got = [host(t) for t in runs[0]]
    for name, g, w, e in zip("pmv", got, want, e32):
        print("FlatAdam wd %g %s: max |d| %.3e (e32 %.3e)" % (wd, name, float(np.abs(g - w).max()), e))
    print("FlatAdam wd %g norms: max relative |d| %.2e" % (wd, max(abs(a / b - 1.0) for a, b in zip(got_norms, norms))))
    assert tc.adam_within(got, want, e32, got_norms, norms)


# ---------------------------------------------------------------------------------------------------------------------------
def small_pipeline(mods, golden, case, fmt, dropout=0.0):
    mods["ops"].set_compute_dtype(FMTS[fmt])
    stats = dict(feat_mean=golden["ds.feat_mean"], feat_std=golden["ds.feat_std"])
    train_set = frameset(mods, case, **stats)
    test_set = mods["training"].FrameSet([dev(r) for r in case["raws"][:3]], [dev(m) for m in case["masks"][:3]], **stats)
    pipe = mods["training"].TrainingPipeline("pcirm", use_rbm_pretrain=False)
    Ws, bs = tc.fixture_params()
    pipe.model = mods["models"].SpeechEnhancementDNN(594, 64, 64, 3)
    pipe.model.load_state_dict(dn.state_dict(Ws, bs))
    pipe.model = pipe.model.cuda()
    pipe.model.dropout_rate = dropout
    pipe.batch_size = tc.BATCH
    pipe.feature_dim, pipe.mask_dim = 594, 64
    return pipe, train_set, test_set, pipe._optimizer(tc.LR), mods["optim"].DynamicLossScale("cuda")


def within(tag, got, exact, emu):
    (r, m), (re, me) = dn.err(got, exact), dn.err(emu, exact)
    print("%s: rms %.3e (emulation %.3e, ratio %.2f)  max %.3e (emulation %.3e, ratio %.2f)" % (tag, r, re, r / re, m, me, m / me))
    assert np.isfinite(np.asarray(got)).all() and r <= 4.0 * re and m <= 4.0 * me, (tag, r, re, m, me)


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_trajectory(mods, golden, case, fmt):
    pipe, train_set, test_set, opt, scale = small_pipeline(mods, golden, case, fmt)
    order = np.arange(tc.N_FRAMES)
    torch.cuda.synchronize()
    got_loss, train_losses, val_losses = [], [], []
    for _ in range(2):
        train_losses.append(pipe._train_epoch(train_set, opt, scale, order=order))
        got_loss += [float(l) for l in pipe.batch_losses]
        val_losses.append(pipe._validate(test_set))
    assert opt.stats()["step"] == 10 and scale.stats()["skipped_inf"] == 0
    Ws, bs = tc.fixture_params()
    x, t = golden["ds.features"].astype(np.float64), golden["ds.masks"].astype(np.float64)
    x2, t2 = golden["ds2.features"].astype(np.float64), golden["ds2.masks"].astype(np.float64)
    exact = tc.train64(Ws, bs, x, t, tc.batches(), 2)
    emu = tc.train64(Ws, bs, x, t, tc.batches(), 2, fmt=FMTS[fmt], S=tc.INIT_SCALE)
    like = tc.interleave(Ws, bs)
    within("trajectory %s per-step loss" % fmt, got_loss, np.asarray(exact["loss"]), np.asarray(emu["loss"]))
    got_p = tc.unflat(host(opt.flat_p), like)
    for name, g, e, u in zip(["W0", "b0", "W1", "b1", "W2", "b2", "W3", "b3"], got_p, tc.unflat(exact["params"][-1], like),
                             tc.unflat(emu["params"][-1], like)):
        within("trajectory %s %s after 10 steps" % (fmt, name), g, e, u)
    val_emu = [tc.validate64(emu["params"][k], like, x2, t2, tc.batches(15), fmt=FMTS[fmt]) for k in (4, 9)]
    within("trajectory %s epoch training loss against the reference" % fmt, train_losses, golden["train_loss"], np.asarray(emu["epoch"]))
    within("trajectory %s validation loss against the reference" % fmt, val_losses, golden["val_loss"], np.asarray(val_emu))


def test_dropout_epoch(mods, golden, case):
    """dropout 0.2: the masks are the host replica's, and an epoch is repeatable bit for bit for one seed"""
    ends = []
    for _ in range(2):
        pipe, train_set, _, opt, scale = small_pipeline(mods, golden, case, "f16", dropout=dn.P_DROP)
        pipe.model.train()
        torch.manual_seed(31)
        idx = dev(tc.batches()[0], torch.int32)
        y = pipe.model.forward_indexed(train_set, idx)
        acts = y.grad_fn.saved[0]
        seeds = dn.layer_seeds(dc.drawn_seed(31), 3)
        for l in range(3):
            keep = dc.keep_bits(seeds[l], 0, tc.BATCH * 64, dn.P_DROP).reshape(tc.BATCH, 64)
            h = host(acts[l + 1])[:, :64]
            assert (h[~keep] == 0).all() and (h[keep] > 0).mean() > 0.2, l
        torch.manual_seed(32)
        loss = pipe._train_epoch(train_set, opt, scale, order=np.arange(tc.N_FRAMES))
        ends.append((opt.flat_p.clone(), loss))
    assert torch.equal(bits(ends[0][0]), bits(ends[1][0])) and ends[0][1] == ends[1][1] and np.isfinite(ends[0][1])


@pytest.mark.parametrize("rbm", [False, True])
def test_end_to_end(mods, tmp_path, monkeypatch, rbm):
    from sincformer_metacog_speech_enhancement_amd import config, synthetic
    mods["ops"].set_compute_dtype(torch.float16)
    monkeypatch.setattr(config, "RBM_EPOCHS", 1)
    noisy, clean = synthetic.synth_wave(6, 8000, 3)
    noisy, clean = dev(noisy), dev(clean)
    noise = noisy - clean
    FrameSet = mods["training"].FrameSet
    train_set = FrameSet.from_waveforms(clean[:4], noise[:4], noisy[:4], "irm")
    test_set = FrameSet.from_waveforms(clean[4:], noise[4:], noisy[4:], "irm", feat_mean=train_set.feat_mean, feat_std=train_set.feat_std)
    assert len(train_set) == 4 * 99 and train_set.raw.shape[1] == 54 and test_set.feat_mean is train_set.feat_mean
    pipe = mods["training"].TrainingPipeline("irm", use_rbm_pretrain=rbm, model_dir=str(tmp_path), rbm_seed=5)
    torch.manual_seed(1)
    pipe.train(train_set, test_set, epochs=3, verbose=False)
    hist = pipe.history
    print("end to end (rbm %d): train %s val %s" % (rbm, [round(h[0], 5) for h in hist], [round(h[1], 5) for h in hist]))
    assert len(hist) == 3 and all(np.isfinite(h[0]) and np.isfinite(h[1]) for h in hist)
    assert hist[-1][0] < hist[0][0]                                                   # the training loss falls
    assert os.path.exists(os.path.join(str(tmp_path), "best_irm.pt"))
    fresh = mods["training"].TrainingPipeline("irm", model_dir=str(tmp_path))
    fresh.load_model()
    assert fresh.feat_mean.dtype == np.float32 and fresh.feature_dim == 594 and fresh.mask_dim == 64
    out = fresh.enhance_signal(noisy[:2])
    assert out.shape == (2, 8000) and bool(torch.isfinite(out).all())
    if not rbm:
        # nothing synchronises inside an epoch: every launch of it is enqueued while synchronising calls raise
        opt, scale = pipe._optimizer(1e-3), mods["optim"].DynamicLossScale("cuda")
        pipe._train_epoch(train_set, opt, scale)            # warm: allocations, packs
        torch.cuda.synchronize()
        real = pipe._epoch_loss
        seen = {}

        def deferred(rec):
            seen["rec"] = rec
            return 0.0
        monkeypatch.setattr(pipe, "_epoch_loss", deferred)
        torch.cuda.set_sync_debug_mode("error")
        try:
            pipe._train_epoch(train_set, opt, scale)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert np.isfinite(real(seen["rec"]))
