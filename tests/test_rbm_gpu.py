"""The RBM pre-training on the MI355X (csrc/rbm.hip, models/rbm.py) against the reference's recorded runs (tests/golden/g24_rbm.npz) and
the float64 restatement of tests/rbm_cases.py.

Bounds are not fixed in advance: per tensor 16 x e32, e32 = the error of the restatement run in numpy float32 against float64 on the
same inputs (rbm_cases.bound); a probability that enters a decision is additionally held to an eighth of the fixture's smallest
margin |prob - u|.  tests/test_rbm_host.py shows on the CPU that these bounds catch the mutants of rbm_cases.MUTANTS."""
import os

import numpy as np
import pytest
import torch

import dropout_cases as dc
import rbm_cases as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = (rc.ROWS + rc.BATCH - 1) // rc.BATCH
LR32 = np.float32(rc.LR)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "g24_rbm.npz")))


@pytest.fixture(scope="module")
def pkg():
    from sincformer_metacog_speech_enhancement_amd import config, models, ops, training
    return {"config": config, "models": models, "ops": ops, "training": training}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().cpu().numpy()


def draws_of(golden, prefix):
    return {"perms": golden[prefix + ".perms"], "u": [golden["%s.u%d" % (prefix, s)] for s in range(rc.EPOCHS * STEPS)]}


def zero_state(W0):
    return rc.f32_state((W0, np.zeros(W0.shape[0]), np.zeros(W0.shape[1])))


def check(name, got, ref, bound):
    e = rc.err(got, ref)
    print("%-28s err %.3e bound %.3e" % (name, e, bound))
    assert e <= bound, (name, e, bound)


# ---- replay, on the fixture ----
def test_replay_first_step(golden, pkg):
    """one step's prob_h, the sample plane exactly the reference's, nv and nh"""
    np.random.seed(int(golden["seed"]))
    rbm = pkg["models"].RBM(rc.V, rc.H)
    x = golden["data"]
    rows = golden["k1.perms"][0][:rc.BATCH]
    st0 = zero_state(golden["k1.W0"])
    _, o64 = rc.step(st0, x[rows], 1, LR32, u=golden["k1.u0"])
    _, o32 = rc.step(st0, x[rows], 1, LR32, u=golden["k1.u0"], dt=np.float32)
    margin = float(golden["margin"])
    ph, hs = rbm.sample_hidden(dev(x[rows]), u=golden["k1.u0"][0])
    check("ph", host(ph), golden["k1.ph"], rc.bound(o32["ph"], o64["ph"], margin))
    assert np.array_equal(host(hs), golden["k1.hs"])
    nv, _ = rbm.sample_visible(hs)
    nh = rbm.transform(nv)
    check("nv", host(nv), golden["k1.nv"], rc.bound(o32["nv"], o64["nv"]))
    check("nh", host(nh), golden["k1.nh"], rc.bound(o32["nh"], o64["nh"]))


@pytest.mark.parametrize("k", rc.KS)
def test_replay_train(golden, pkg, k):
    """the whole train(): W, both biases and the per-epoch errors against the reference's"""
    np.random.seed(int(golden["seed"]))
    rbm = pkg["models"].RBM(rc.V, rc.H, learning_rate=rc.LR, k_steps=k, draws=draws_of(golden, "k%d" % k))
    errors = rbm.train(dev(golden["data"]), epochs=rc.EPOCHS, batch_size=rc.BATCH, verbose=False)
    st0 = zero_state(golden["k%d.W0" % k])
    r64 = rc.train(st0, golden["data"], rbm.draws, k, LR32, rc.BATCH)
    r32 = rc.train(st0, golden["data"], rbm.draws, k, LR32, rc.BATCH, dt=np.float32)
    W, vb, hb = rbm.get_weights()
    for i, (name, got) in enumerate((("W", W), ("v_bias", vb), ("h_bias", hb))):
        check("k%d %s" % (k, name), host(got), golden["k%d.%s" % (k, name)], rc.bound(r32[0][i], r64[0][i]))
    assert isinstance(errors, list) and len(errors) == rc.EPOCHS and all(isinstance(e, float) for e in errors)
    check("k%d errors" % k, errors, golden["k%d.errors" % k], rc.bound(r32[1], r64[1]))


def test_replay_stack(golden, pkg, monkeypatch):
    """pretrain_dnn_with_rbm(replay=True) consumes np.random in the reference's order: the three layers are the reference's"""
    monkeypatch.setattr(pkg["config"], "RBM_EPOCHS", rc.EPOCHS)
    monkeypatch.setattr(pkg["config"], "RBM_BATCH_SIZE", rc.BATCH)
    np.random.seed(int(golden["seed"]))
    weights = pkg["models"].pretrain_dnn_with_rbm(dev(golden["data"]), list(rc.STACK), verbose=False, replay=True)
    assert np.random.random() == float(golden["stack.next"])
    np.random.seed(int(golden["seed"]))
    states, draws = [], []
    for l in range(len(rc.STACK) - 1):
        states.append(zero_state(np.random.randn(rc.STACK[l], rc.STACK[l + 1]) * 0.01))
        draws.append(pkg["models"].rbm_draws(rc.ROWS, rc.STACK[l], rc.STACK[l + 1], rc.EPOCHS, rc.BATCH, 1))
        np.random.random((rc.ROWS, rc.STACK[l + 1]))
    s64 = rc.stack(states, golden["data"], draws, 1, LR32, rc.BATCH)
    s32 = rc.stack(states, golden["data"], draws, 1, LR32, rc.BATCH, dt=np.float32)
    assert len(weights) == 3
    for l, tup in enumerate(weights):
        assert all(t.is_cuda and t.dtype == torch.float32 for t in tup)
        for i, name in enumerate(("W", "v_bias", "h_bias")):
            check("layer %d %s" % (l, name), host(tup[i]), golden["stack.l%d.%s" % (l, name)], rc.bound(s32[l][i], s64[l][i]))


# ---- the probability pass alone ----
MS = (1, 31, 32, 33, 127, 128, 129)             # 32 = the tile edge of rbm.hip


@pytest.mark.parametrize("down", (False, True))
@pytest.mark.parametrize("shape", ((594, 1024), (1024, 594), (70, 48), (1, 1)))
def test_prob_pass(pkg, shape, down):
    """(K, N) = shape: against float64 at every M; a row's bits the same alone and inside any M; through a shuffled index bitwise
    the pre-gathered call; the sample plane exactly prob > u, also where u IS the probability; 0 and 1 at the extremes"""
    ops = pkg["ops"]
    K, N = shape
    V, H = (N, K) if down else (K, N)
    rng = np.random.default_rng(K * 7 + N + down)
    W = (rng.standard_normal((V, H)) * 0.05).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    A = rc.data(max(MS), K, K + N)
    z64 = A.astype(np.float64) @ (W.T if down else W).astype(np.float64) + bias
    p64 = rc.sigmoid(z64)
    p32 = rc.sigmoid(A @ (W.T if down else W) + bias).astype(np.float32)
    b = rc.bound(p32, p64)
    Wd, bd, Ad = dev(W), dev(bias), dev(A)
    full = host(ops.rbm_prob(Ad, Wd, bd, down=down))
    check("K%d N%d down%d" % (K, N, down), full, p64, b)
    for M in MS:
        part = host(ops.rbm_prob(Ad, Wd, bd, down=down, M=M))
        assert part.shape == (M, N) and np.array_equal(part, full[:M]), M
    perm = rng.permutation(max(MS))[:77].astype(np.int32)
    gathered = host(ops.rbm_prob(dev(A[perm]), Wd, bd, down=down))
    indexed = host(ops.rbm_prob(Ad, Wd, bd, down=down, rows=dev(perm, torch.int32)))
    assert np.array_equal(gathered, indexed) and np.array_equal(gathered, full[perm])
    u = rng.random((max(MS), N))
    pr, s = ops.rbm_prob(Ad, Wd, bd, down=down, u=dev(u, torch.float64))
    assert np.array_equal(host(pr), full) and np.array_equal(host(s), (full.astype(np.float64) > u).astype(np.float32))
    _, s = ops.rbm_prob(Ad, Wd, bd, down=down, u=dev(full, torch.float64))
    assert not host(s).any()                                             # prob > prob nowhere (>= would hold everywhere)
    for big, want in ((1e4, 1.0), (-1e4, 0.0), (float("inf"), 1.0), (float("-inf"), 0.0)):
        ext = host(ops.rbm_prob(Ad[:3], Wd, torch.full((N,), big, device="cuda"), down=down))
        assert np.array_equal(ext, np.full((3, N), want, dtype=np.float32)), big


# ---- one step at the first layer's shape ----
def test_big_step(pkg):
    """594 -> 1024, B = 203, replay: the sample plane is exactly prob_device > u and differs from float64's decision on at most
    1e-4 of the units; everything behind it against the restatement GIVEN the device's samples"""
    Vb, Hb, Bb = rc.BIG
    rng = np.random.default_rng(2401)
    st = rc.f32_state((rng.standard_normal((Vb, Hb)) * 0.01, rng.standard_normal(Vb) * 0.01, rng.standard_normal(Hb) * 0.01))
    v, u = rc.data(Bb, Vb, 2402), rng.random((1, Bb, Hb))
    rbm = pkg["models"].RBM(Vb, Hb)
    rbm.W, rbm.v_bias, rbm.h_bias = (dev(a) for a in st)
    vd = dev(v)
    bufs = rbm._buffers(Bb, vd.device)
    partial = torch.zeros(pkg["ops"].rbm_error_tiles(Vb), device="cuda", dtype=torch.float64)
    rbm._step(vd, None, Bb, bufs, partial, dev(u, torch.float64))
    ph, hs, nv, nh = (host(t) for t in bufs)
    assert np.array_equal(hs, (ph.astype(np.float64) > u[0]).astype(np.float32))
    _, d64 = rc.step(st, v, 1, LR32, u=u)
    flips = int((d64["hs"][0] != hs).sum())
    print("decisions that differ from float64's: %d of %d" % (flips, hs.size))
    assert flips <= 1e-4 * hs.size
    n64, o64 = rc.step(st, v, 1, LR32, samples=[hs])
    n32, o32 = rc.step(st, v, 1, LR32, samples=[hs], dt=np.float32)
    for name, got in (("ph", ph), ("nv", nv), ("nh", nh)):
        check("big " + name, got, o64[name], rc.bound(o32[name], o64[name]))
    for i, (name, got) in enumerate((("W", rbm.W), ("v_bias", rbm.v_bias), ("h_bias", rbm.h_bias))):
        check("big " + name, host(got), n64[i], rc.bound(n32[i], n64[i]))
    e = float(host(partial).sum()) / (Bb * Vb)
    check("big err", e, o64["err"], rc.bound(o32["err"], o64["err"]))


# ---- the update alone ----
@pytest.mark.parametrize("shape", ((70, 48, 37), (33, 65, 5), (1, 1, 1), (594, 1024, 203)))
def test_update_touches_every_element_once(pkg, shape):
    """v = ph = 1 and nv = nh = 0: every element of W moves by exactly one application of (lr / B) B and every bias by lr - not
    zero times, not twice; the products and sums of this case are exact, so the expected values are the kernel's own arithmetic.
    Then v = nv and ph = nh on sixteenths (every product and partial sum is exact in fp32, so the accumulation IS zero): the state
    stays bit for bit and the error partials are zero."""
    ops = pkg["ops"]
    V, H, B = shape
    rng = np.random.default_rng(V + H + B)
    W0 = (rng.standard_normal((V, H)) * 0.01).astype(np.float32)
    vb0, hb0 = (rng.standard_normal(V) * 0.01).astype(np.float32), (rng.standard_normal(H) * 0.01).astype(np.float32)
    tiles = ops.rbm_error_tiles(V)
    n_rows = B + 3
    rows = rng.permutation(n_rows)[:B].astype(np.int32)
    data = np.full((n_rows, V), 7.0, dtype=np.float32)                    # a row the index does not name must not be read
    data[rows] = 1.0
    W, vb, hb = dev(W0), dev(vb0), dev(hb0)
    part = torch.full((tiles,), -1.0, device="cuda", dtype=torch.float64)
    ops.rbm_update(dev(data), dev(np.ones((B, H), np.float32)), dev(np.zeros((B, V), np.float32)), dev(np.zeros((B, H), np.float32)),
                   W, vb, hb, part, rc.LR, rows=dev(rows, torch.int32))
    scale = np.float32(LR32 / np.float32(B))
    want_W = (W0.astype(np.float64) + float(scale) * B).astype(np.float32)           # fmaf(scale, B, W): one rounding
    assert np.array_equal(host(W), want_W) and not np.array_equal(want_W, W0)
    assert np.array_equal(host(vb), (vb0.astype(np.float64) + float(LR32) * B / B).astype(np.float32))
    assert np.array_equal(host(hb), (hb0.astype(np.float64) + float(LR32) * B / B).astype(np.float32))
    cols = np.minimum(32, V - 32 * np.arange(tiles))
    assert np.array_equal(host(part), (B * cols).astype(np.float64))
    # no difference, no change
    v16 = (rng.integers(0, 17, (n_rows, V)) / 16.0).astype(np.float32)
    h16 = (rng.integers(0, 17, (B, H)) / 16.0).astype(np.float32)
    W, vb, hb = dev(W0), dev(vb0), dev(hb0)
    ops.rbm_update(dev(v16), dev(h16), dev(v16[rows]), dev(h16), W, vb, hb, part, rc.LR, rows=dev(rows, torch.int32))
    assert np.array_equal(host(W), W0) and np.array_equal(host(vb), vb0) and np.array_equal(host(hb), hb0)
    assert not host(part).any()


# ---- counter mode ----
def test_counter_plane_is_the_host_replicas(golden, pkg):
    np.random.seed(1)
    rbm = pkg["models"].RBM(rc.V, rc.H, seed=77)
    x = dev(golden["data"])
    seeds = dc.Seeds(77)
    ph, hs = rbm.sample_hidden(x)
    assert np.array_equal(host(hs), rc.sample_counter(host(ph), seeds.next()))
    pv, vs = rbm.sample_visible(hs)
    assert np.array_equal(host(vs), rc.sample_counter(host(pv), seeds.next()))
    assert 0.3 < host(hs).mean() < 0.7


def counter_run(pkg, golden, seed, epochs=2, lr=None, batch=rc.BATCH):
    np.random.seed(5)
    torch.manual_seed(11)                                               # the permutation is torch.randperm on the device
    rbm = pkg["models"].RBM(rc.V, rc.H, learning_rate=lr, seed=seed)
    errors = rbm.train(dev(golden["data"]), epochs=epochs, batch_size=batch, verbose=False)
    return [host(t) for t in rbm.get_weights()], errors


def test_counter_runs_repeat_bitwise_and_seeds_differ(golden, pkg):
    a, ea = counter_run(pkg, golden, 3)
    b, eb = counter_run(pkg, golden, 3)
    c, ec = counter_run(pkg, golden, 4)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and ea == eb
    assert not np.array_equal(a[0], c[0]) and ea != ec


def test_counter_errors_do_not_rise(golden, pkg):
    """a 5-epoch run on the fixture data: no epoch's error is above the one before it.  The fixture's 101 rows are independent
    noise around 0.5, so all there is to learn are the columns' means, and the error falls by about 5e-4 in five epochs while the
    sampling moves an epoch's error by about 1e-4: at the default rate and batches of 37 the float64 restatement's error rises
    somewhere in most seeded runs (86 of 100), whatever the arithmetic.  The recipe here is the one at which the fall dominates:
    lr 0.05 with the 101 rows in one batch, where the restatement's error fell from the first epoch to the fifth in 200 of 200
    seeded runs (mean -4.6e-4, standard deviation 0.9e-4).  The seeds are fixed and the run repeats bit for bit (the test above),
    so the outcome is that of one known trajectory."""
    _, errors = counter_run(pkg, golden, 9, epochs=5, lr=0.05, batch=rc.ROWS)
    print("errors", errors)
    assert len(errors) == 5 and all(np.isfinite(errors))
    assert all(b <= a for a, b in zip(errors, errors[1:])), errors


# ---- rbm_pretrain end to end ----
def test_rbm_pretrain_end_to_end(golden, pkg, monkeypatch):
    monkeypatch.setattr(pkg["config"], "RBM_EPOCHS", 2)
    monkeypatch.setattr(pkg["config"], "RBM_BATCH_SIZE", rc.BATCH)
    np.random.seed(8)
    torch.manual_seed(8)
    dnn = pkg["models"].SpeechEnhancementDNN(rc.V, rc.H, 64, 3).cuda()
    out_w = dnn.network[9].weight.detach().clone()
    feats = dev(np.random.default_rng(3).standard_normal((2, 60, rc.V)).astype(np.float32))
    assert pkg["training"].rbm_pretrain(dnn, feats, max_samples=rc.ROWS, seed=21, verbose=False) is True
    # the same stack again, by hand
    np.random.seed(8)
    torch.manual_seed(8)
    x01 = pkg["models"].RBM.sigmoid(feats.reshape(-1, rc.V)[:rc.ROWS]).contiguous()
    stack = pkg["models"].pretrain_dnn_with_rbm(x01, [rc.V, rc.H, rc.H, rc.H], verbose=False, seed=21)
    for l, (W, _, hb) in enumerate(stack):
        lin = dnn.network[3 * l]
        assert torch.equal(lin.weight.detach(), W.T) and torch.equal(lin.bias.detach(), hb), l
        assert float(W.std()) > 1e-6
    assert torch.equal(dnn.network[9].weight.detach(), out_w)
