"""The RBM pre-training without a GPU: the float64 restatement of tests/rbm_cases.py against the reference's recorded runs
(tests/golden/g24_rbm.npz), models.rbm_draws against the recorded stream, the module's host side, the host replica of the counter
rule, the argument guards of the three entry points through the built library, the launch costs the wrappers state, and a proof on
the CPU that the bounds of tests/test_rbm_gpu.py - 16 x the error of the float32 restatement - catch plausible wrong kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dropout_cases as dc
import ops_stub
import rbm_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "g24_rbm.npz")))


@pytest.fixture(scope="module")
def pkg():
    from sincformer_metacog_speech_enhancement_amd import config, models, ops, training
    return {"config": config, "models": models, "ops": ops, "training": training}


STEPS = (rc.ROWS + rc.BATCH - 1) // rc.BATCH


def draws_of(golden, prefix, k=1):
    return {"perms": golden[prefix + ".perms"], "u": [golden["%s.u%d" % (prefix, s)] for s in range(rc.EPOCHS * STEPS)]}


def zero_state(W0):
    return (W0, np.zeros(W0.shape[0]), np.zeros(W0.shape[1]))


# ---- the restatement against the reference's recorded runs ----
@pytest.mark.parametrize("k", rc.KS)
def test_restatement_matches_the_fixture(golden, k):
    assert float(golden["margin"]) >= 1e-5
    x = golden["data"].astype(np.float64)
    state, errors, first = rc.train(zero_state(golden["k%d.W0" % k]), x, draws_of(golden, "k%d" % k), k, rc.LR, rc.BATCH)
    for name, got in zip(("W", "v_bias", "h_bias"), state):
        assert rc.err(got, golden["k%d.%s" % (k, name)]) < 1e-12, name
    assert rc.err(errors, golden["k%d.errors" % k]) < 1e-12
    assert np.array_equal(first["hs"][0], golden["k%d.hs" % k])
    for name in ("ph",) + (("nv", "nh") if k == 1 else ()):         # (at k = 2 `nv`, `nh` of a step are those of its LAST Gibbs iteration)
        assert rc.err(first[name], golden["k%d.%s" % (k, name)]) < 1e-12, name


def test_restatement_of_the_stack_matches_the_fixture(golden):
    np.random.seed(int(golden["seed"]))
    states, draws = [], []
    x = golden["data"].astype(np.float64)
    for l in range(len(rc.STACK) - 1):
        draws.append(draws_of(golden, "stack.l%d" % l))
    # the initial weights are the seeded constructor's: regenerate the stream in the reference's order
    from sincformer_metacog_speech_enhancement_amd.models import rbm_draws
    for l in range(len(rc.STACK) - 1):
        states.append(zero_state(np.random.randn(rc.STACK[l], rc.STACK[l + 1]) * 0.01))
        rbm_draws(rc.ROWS, rc.STACK[l], rc.STACK[l + 1], rc.EPOCHS, rc.BATCH, 1)
        np.random.random((rc.ROWS, rc.STACK[l + 1]))
    assert np.random.random() == float(golden["stack.next"])
    out = rc.stack(states, x, draws, 1, rc.LR, rc.BATCH)
    for l, st in enumerate(out):
        for name, got in zip(("W", "v_bias", "h_bias"), st):
            assert rc.err(got, golden["stack.l%d.%s" % (l, name)]) < 1e-12, (l, name)


# ---- rbm_draws ----
@pytest.mark.parametrize("k", rc.KS)
def test_rbm_draws_is_the_recorded_stream(golden, pkg, k):
    """bit for bit the permutations and the deciding uniforms, and the stream stands where the reference's stood after train():
    the dropped planes have the reference's sizes and positions"""
    np.random.seed(int(golden["seed"]))
    W0 = np.random.randn(rc.V, rc.H) * 0.01
    assert np.array_equal(W0, golden["k%d.W0" % k])
    d = pkg["models"].rbm_draws(rc.ROWS, rc.V, rc.H, rc.EPOCHS, rc.BATCH, k)
    assert np.random.random() == float(golden["k%d.next" % k])
    assert d["perms"].dtype == np.int64 and np.array_equal(d["perms"], golden["k%d.perms" % k])
    assert len(d["u"]) == rc.EPOCHS * STEPS
    for s, u in enumerate(d["u"]):
        assert u.shape == (k, (37, 37, 27)[s % STEPS], rc.H) and np.array_equal(u, golden["k%d.u%d" % (k, s)]), s


def test_rbm_draws_defaults_and_budget(pkg, monkeypatch):
    models = pkg["models"]
    np.random.seed(3)
    d = models.rbm_draws(300, 5, 4)
    assert d["perms"].shape == (10, 300) and len(d["u"]) == 20 and d["u"][1].shape == (1, 44, 4)          # 10 epochs, 256 + 44, k 1
    with pytest.raises(ValueError, match="small runs"):
        models.rbm_draws(50000, 594, 1024)
    with pytest.raises(ValueError):
        models.rbm_draws(0, 5, 4)


# ---- the module's host side ----
def test_constructor_is_seeded_like_the_reference(golden, pkg):
    np.random.seed(int(golden["seed"]))
    r = pkg["models"].RBM(rc.V, rc.H)
    assert r.W.dtype == torch.float32 and np.array_equal(r.W.numpy(), golden["k1.W0"].astype(np.float32))
    assert r.v_bias.shape == (rc.V,) and r.h_bias.shape == (rc.H,) and not r.v_bias.any() and not r.h_bias.any()
    assert (r.n_visible, r.n_hidden, r.lr, r.k) == (rc.V, rc.H, 0.01, 1)
    W, vb, hb = r.get_weights()
    assert W is not r.W and torch.equal(W, r.W) and vb is not r.v_bias and hb is not r.h_bias


def test_or_defaults_and_config(golden, pkg):
    cfg = pkg["config"]
    assert (cfg.RBM_LEARNING_RATE, cfg.RBM_EPOCHS, cfg.RBM_BATCH_SIZE, cfg.RBM_K_STEPS) == (0.01, 10, 256, 1)
    z = pkg["models"].RBM(3, 2, 0, 0)
    assert [z.lr, z.k] == [float(v) for v in golden["or_defaults"]] == [0.01, 1]
    r = pkg["models"].RBM(3, 2, 0.5, 3)
    assert (r.lr, r.k) == (0.5, 3)
    for bad in ((0, 4), (4, 0), (pkg["ops"].RBM_MAX_UNITS + 1, 4)):
        with pytest.raises(ValueError, match="the kernels take"):
            pkg["models"].RBM(*bad)
    with pytest.raises(ValueError, match="not both"):
        pkg["models"].RBM(3, 2, seed=1, draws={})


def test_sigmoid_static(pkg):
    RBM = pkg["models"].RBM
    x = np.array([-1e4, -3.0, 0.0, 3.0, 1e4])
    assert np.array_equal(RBM.sigmoid(x), 1.0 / (1.0 + np.exp(-np.clip(x, -500, 500))))
    t = RBM.sigmoid(torch.tensor(x, dtype=torch.float32))
    assert t.dtype == torch.float32 and t[0] == 0 and t[-1] == 1 and not torch.isnan(t).any()
    assert np.abs(t.double().numpy() - RBM.sigmoid(x)).max() < 1e-7


def test_a_host_tensor_is_refused(pkg):
    np.random.seed(0)
    r = pkg["models"].RBM(6, 4)
    for call in (lambda: r.sample_hidden(torch.zeros(3, 6)), lambda: r.sample_visible(torch.zeros(3, 4)),
                 lambda: r.contrastive_divergence(torch.zeros(3, 6)), lambda: r.train(torch.zeros(3, 6)),
                 lambda: r.transform(torch.zeros(3, 6)), lambda: pkg["models"].pretrain_dnn_with_rbm(torch.zeros(3, 6), [6, 4], verbose=False)):
        with pytest.raises(RuntimeError, match="CPU"):
            call()
    with pytest.raises(ValueError, match=r"\[rows, 6\]"):
        r.transform(torch.zeros(3, 5))
    dnn = pkg["models"].SpeechEnhancementDNN(6, 4, 2, 2)
    with pytest.raises(RuntimeError, match="CPU"):
        pkg["training"].rbm_pretrain(dnn, torch.zeros(3, 6), verbose=False)
    with pytest.raises(ValueError, match="features"):
        pkg["training"].rbm_pretrain(dnn, torch.zeros(3, 5), verbose=False)
    assert "rbm_pretrain" in pkg["training"].__all__


def test_load_rbm_weights_of_a_stack(golden, pkg):
    m = pkg["models"].SpeechEnhancementDNN(70, 48, 64, 3)
    before = m.network[9].weight.detach().clone()
    tuples = [tuple(torch.from_numpy(golden["stack.l%d.%s" % (l, n)].astype(np.float32)) for n in ("W", "v_bias", "h_bias")) for l in range(3)]
    m.load_rbm_weights(tuples)
    for l in range(3):
        assert torch.equal(m.network[3 * l].weight.detach(), tuples[l][0].T) and torch.equal(m.network[3 * l].bias.detach(), tuples[l][2])
    assert torch.equal(m.network[9].weight.detach(), before)


def test_degenerate_check_on_stub_tuples(pkg):
    from sincformer_metacog_speech_enhancement_amd.training import pipeline
    good = (np.random.default_rng(0).standard_normal((5, 4)) * 0.01, np.zeros(5), np.zeros(4))
    flat = (np.full((5, 4), 0.3), np.zeros(5), np.zeros(4))
    nan = (np.full((5, 4), np.nan), np.zeros(5), np.zeros(4))
    tiny = (good[0] * 1e-5, np.zeros(5), np.zeros(4))
    assert pipeline.rbm_weights_degenerate([good, good]) is None
    assert pipeline.rbm_weights_degenerate([good, flat]) == 1 and pipeline.rbm_weights_degenerate([nan, good]) == 0
    assert pipeline.rbm_weights_degenerate([good, good, tiny]) == 2
    as_t = lambda t: tuple(torch.from_numpy(np.asarray(a, dtype=np.float32)) for a in t)
    assert pipeline.rbm_weights_degenerate([as_t(good), as_t(good)]) is None and pipeline.rbm_weights_degenerate([as_t(good), as_t(nan)]) == 1
    assert pipeline.rbm_weights_degenerate([as_t(flat)]) == 0


# ---- the counter rule ----
def test_counter_rule_replica():
    """the word is the one the dropout replica compares: word >= threshold(p) is dropout_cases.keep_bits; the sample is its
    complement at p = prob; P(S = 1) = ceil(p 2^24) / 2^24"""
    M, N, seed = 13, 29, 0x9E3779B1
    for p in (0.2, 0.5, 0.937):
        s = rc.sample_counter(np.full((M, N), p, dtype=np.float32), seed)
        assert np.array_equal(s.reshape(-1) == 0.0, dc.keep_bits(seed, 0, M * N, p)), p
    assert rc.sample_counter(np.zeros((M, N), dtype=np.float32), seed).sum() == 0            # word < 0 never
    assert rc.sample_counter(np.ones((M, N), dtype=np.float32), seed).sum() == M * N          # word < 2^24 always
    rate = rc.sample_counter(np.full((200, 500), 0.3, dtype=np.float32), 7).mean()
    assert abs(rate - 0.3) < 0.01
    assert not np.array_equal(rc.sample_counter(np.full((M, N), 0.5, dtype=np.float32), 1), rc.sample_counter(np.full((M, N), 0.5, dtype=np.float32), 2))


# ---- argument guards through the built library ----
@pytest.fixture(scope="module")
def L():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def test_rbm_prob_guards_without_a_gpu(L):
    """a null pointer or a bad code gives -1 and a bad shape -2, before any HIP call: every call below is refused"""
    one = ctypes.c_void_p(16)

    def call(data=one, rows=None, W=one, bias=one, prob=one, sample=None, u=None, M=4, V=70, H=48, n_rows=4, lda=70, down=0, mode=0):
        return L.sfm_rbm_prob(data, rows, W, bias, prob, sample, u, M, V, H, n_rows, lda, down, mode, 0, None)
    assert call(data=None) == -1 and call(W=None) == -1 and call(bias=None) == -1 and call(prob=None) == -1
    assert call(down=2) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(sample=one) == -1 and call(mode=1, sample=one) == -1 and call(mode=1, u=one) == -1      # sample and u go with their mode
    assert call(mode=2, sample=one, u=one) == -1 and call(mode=2) == -1 and call(u=one) == -1
    assert call(M=0) == -2 and call(V=0) == -2 and call(H=0) == -2 and call(n_rows=0) == -2
    assert call(V=16385) == -2 and call(H=16385) == -2
    assert call(lda=69) == -2 and call(down=1, lda=47) == -2            # a row stride below the row
    assert call(M=5) == -2                                              # without an index the rows are the data's first M


def test_rbm_update_and_fold_guards_without_a_gpu(L):
    one = ctypes.c_void_p(16)

    def call(data=one, rows=None, ph=one, nv=one, nh=one, W=one, vb=one, hb=one, part=one, B=4, V=70, H=48, n_rows=4, ldv=70, lr=0.01):
        return L.sfm_rbm_update(data, rows, ph, nv, nh, W, vb, hb, part, B, V, H, n_rows, ldv, lr, None)
    for name in ("data", "ph", "nv", "nh", "W", "vb", "hb", "part"):
        assert call(**{name: None}) == -1, name
    assert call(lr=float("nan")) == -1
    assert call(B=0) == -2 and call(B=65537, rows=one) == -2 and call(V=0) == -2 and call(H=16385) == -2 and call(n_rows=0) == -2
    assert call(ldv=69) == -2 and call(B=5) == -2

    def fold(part=one, out=one, steps=3, tiles=3, n=101, batch=37, V=70):
        return L.sfm_rbm_fold_error(part, out, steps, tiles, n, batch, V, None)
    assert fold(part=None) == -1 and fold(out=None) == -1
    assert fold(steps=0) == -2 and fold(tiles=0) == -2 and fold(n=0) == -2 and fold(batch=0) == -2 and fold(V=0) == -2
    assert fold(tiles=2) == -2 and fold(steps=2) == -2 and fold(V=97) == -2                   # tiles = ceil(V / 32), steps = ceil(n / batch)


# ---- the launch costs the wrappers state ----
@pytest.fixture
def launches(monkeypatch):
    return ops_stub.install(monkeypatch)


def test_rbm_launch_costs(launches, pkg):
    ops = pkg["ops"]
    B, V, H, N = 256, 594, 1024, 1000
    data, W, vb, hb = torch.zeros(N, V), torch.zeros(V, H), torch.zeros(V), torch.zeros(H)
    rows = torch.zeros(B, dtype=torch.int32)
    ph, hs = ops.rbm_prob(data, W, hb, rows=rows, seed=5)
    assert ph.shape == hs.shape == (B, H)
    nv = ops.rbm_prob(hs, W, vb, down=True)
    assert nv.shape == (B, V)
    nh, _ = ops.rbm_prob(nv, W, hb, u=torch.zeros(B, H, dtype=torch.float64))
    part = torch.zeros(ops.rbm_error_tiles(V), dtype=torch.float64)
    assert part.numel() == 19
    ops.rbm_update(data, ph, nv, nh, W, vb, hb, part, 0.01, rows=rows)
    ops.rbm_fold_error(part, torch.zeros(1, dtype=torch.float64), 1, B, B, V)
    wb = 4 * V * H
    assert launches == [
        ("sfm_rbm_prob", "rbm_prob", 2.0 * B * H * V, 4 * B * V + wb + 4 * H + 4 * B * H + 4 * B + 4 * B * H, "M256 N1024 K594 up s2"),
        ("sfm_rbm_prob", "rbm_prob", 2.0 * B * V * H, 4 * B * H + wb + 4 * V + 4 * B * V, "M256 N594 K1024 down s0"),
        ("sfm_rbm_prob", "rbm_prob", 2.0 * B * H * V, 4 * B * V + wb + 4 * H + 4 * B * H + 4 * B * H + 8 * B * H, "M256 N1024 K594 up s1"),
        # the update reads v, ph, nv, nh once and reads and writes W and the biases once
        ("sfm_rbm_update", "rbm_update", 2.0 * 2 * B * V * H + 3.0 * B * V + 2.0 * B * H,
         4 * (2 * B * V + 2 * B * H) + 2 * wb + 8 * (V + H) + 8 * 19 + 4 * B, "B256 V594 H1024"),
        ("sfm_rbm_fold_error", "rbm_fold", 1.0 * (19 + 2), 8.0 * 19 + 8.0, None),
    ]


def test_rbm_wrappers_refuse_what_the_kernels_would(launches, pkg):
    ops = pkg["ops"]
    data, W, vb, hb = torch.zeros(10, 70), torch.zeros(70, 48), torch.zeros(70), torch.zeros(48)
    f64 = torch.float64
    for call in (lambda: ops.rbm_prob(torch.zeros(10, 71), W, hb), lambda: ops.rbm_prob(data, W, vb),
                 lambda: ops.rbm_prob(data, W, hb, down=True), lambda: ops.rbm_prob(data, W, hb, M=11),
                 lambda: ops.rbm_prob(data, W, hb, rows=torch.zeros(4, dtype=torch.int64)),
                 lambda: ops.rbm_prob(data, W, hb, u=torch.zeros(10, 48)), lambda: ops.rbm_prob(data, W, hb, u=torch.zeros(9, 48, dtype=f64)),
                 lambda: ops.rbm_prob(data, W, hb, u=torch.zeros(10, 48, dtype=f64), seed=1),
                 lambda: ops.rbm_prob(data.double(), W, hb), lambda: ops.rbm_prob(data, torch.zeros(70, 48, dtype=f64), hb),
                 lambda: ops.rbm_update(data, torch.zeros(10, 48), torch.zeros(10, 70), torch.zeros(9, 48), W, vb, hb, torch.zeros(3, dtype=f64), 0.01),
                 lambda: ops.rbm_update(data, torch.zeros(10, 48), torch.zeros(10, 70), torch.zeros(10, 48), W, vb, hb, torch.zeros(2, dtype=f64), 0.01),
                 lambda: ops.rbm_update(data, torch.zeros(10, 48), torch.zeros(10, 70), torch.zeros(10, 48), W, hb, vb, torch.zeros(3, dtype=f64), 0.01),
                 lambda: ops.rbm_fold_error(torch.zeros(3, 3, dtype=f64), torch.zeros(1, dtype=f64), 2, 101, 37, 70),
                 lambda: ops.rbm_fold_error(torch.zeros(3, 2, dtype=f64), torch.zeros(1, dtype=f64), 3, 101, 37, 70)):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            call()
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.rbm_prob(data, W, hb, sample=torch.zeros(10, 48))                       # a sample plane without a source of decisions
    assert launches == []


# ---- the GPU tests' bounds catch wrong kernels (all on the CPU) ----
@pytest.fixture(scope="module")
def fixture_runs(golden):
    """(float64 run, float32 run) of the fixture's k = 1 train(), from the state as the device holds it"""
    x = golden["data"]
    st0 = rc.f32_state(zero_state(golden["k1.W0"]))
    dr = draws_of(golden, "k1")
    r64 = rc.train(st0, x, dr, 1, np.float32(rc.LR), rc.BATCH, dt=np.float64)
    r32 = rc.train(st0, x, dr, 1, np.float32(rc.LR), rc.BATCH, dt=np.float32)
    return st0, dr, r64, r32


def test_float32_takes_every_decision_of_the_fixture_the_same_way(golden, fixture_runs):
    _, _, r64, r32 = fixture_runs
    assert np.array_equal(r64[2]["hs"][0], r32[2]["hs"][0]) and np.array_equal(r64[2]["hs"][0], golden["k1.hs"])
    e = rc.err(r32[2]["ph"], r64[2]["ph"])
    print("e32: ph %.2e W %.2e (max |W| %.2e)" % (e, rc.err(r32[0][0], r64[0][0]), np.abs(r64[0][0]).max()))
    assert 16.0 * e < float(golden["margin"]) / 8.0                # 16 x e32 is the tighter of the two bounds on a deciding probability


@pytest.mark.parametrize("mutant", [m for m in rc.MUTANTS if m != "ge"])
def test_train_bounds_catch_mutants(golden, fixture_runs, mutant):
    st0, dr, r64, r32 = fixture_runs
    rm = rc.train(st0, golden["data"], dr, 1, np.float32(rc.LR), rc.BATCH, dt=np.float64, mutant=mutant)
    tensors = {"W": 0, "v_bias": 1, "h_bias": 2}
    name = rc.MUTANT_TENSOR[mutant]
    if name == "errors":
        got, ref, b = rm[1], r64[1], rc.bound(r32[1], r64[1])
    else:
        i = tensors[name]
        got, ref, b = rm[0][i], r64[0][i], rc.bound(r32[0][i], r64[0][i])
    assert rc.err(got, ref) > b, (mutant, name, rc.err(got, ref), b)


def test_plane_check_catches_ge():
    """u = the probabilities themselves: prob > u holds nowhere, prob >= u everywhere"""
    p = rc.data(5, 7, 1)
    assert rc.decide(p, p.astype(np.float64)).sum() == 0 and rc.decide(p, p.astype(np.float64), mutant="ge").sum() == p.size


def test_float32_flips_stay_under_a_quarter_of_the_cap():
    """the GPU test caps the share of units decided differently from float64 at 1e-4 on one step at 594 -> 1024, B 203; the float32
    restatement alone must stay under a quarter of it on the same inputs"""
    Vb, Hb, Bb = rc.BIG
    rng = np.random.default_rng(2401)
    st = rc.f32_state((rng.standard_normal((Vb, Hb)) * 0.01, rng.standard_normal(Vb) * 0.01, rng.standard_normal(Hb) * 0.01))
    v, u = rc.data(Bb, Vb, 2402), rng.random((1, Bb, Hb))
    _, o64 = rc.step(st, v, 1, np.float32(rc.LR), u=u)
    _, o32 = rc.step(st, v, 1, np.float32(rc.LR), u=u, dt=np.float32)
    flips = int((o64["hs"][0] != o32["hs"][0]).sum())
    print("float32 flips %d of %d" % (flips, Bb * Hb))
    assert flips / float(Bb * Hb) < 0.25e-4
