"""Training the DNN from a frame set, the CPU side: the float64 restatements of tests/dnn_train_cases.py against the reference's
captured values (tests/golden/g25_dnn_train.npz) and against torch on the CPU, the argument guards of the new entry points through
the built library, the launch costs their wrappers state, and mutants that the GPU tests' bounds must catch.

Bounds: the statistics' e32 is the reference's own float32 result against float64 (the GPU test allows 16 x that); losses within
2e-6 and gradient norms / parameters within 1e-5 relative of the reference's float32 step, as tests/test_dnn_host.py holds them."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dnn_cases as dn
import dnn_train_cases as tc
import ops_stub

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_dnn_train.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def case():
    raws, masks = tc.frame_set()
    raw, mask = np.concatenate(raws), np.concatenate(masks)
    rows = tc.context_rows64(raw, tc.bounds())
    mean, std = tc.stats64(rows)
    return dict(raw=raw, mask=mask, rows=rows, mean=mean, std=std)


@pytest.fixture(scope="module")
def built():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib


def e32(golden, case):
    """(mean, std): max |reference float32 - float64 restatement|"""
    m, s = tc.stats_rule(case["mean"], case["std"])
    live = golden["ds.feat_std"] != 1.0
    return (float(np.abs(golden["ds.feat_mean"].astype(np.float64) - case["mean"]).max()),
            float(np.abs(golden["ds.feat_std"].astype(np.float64) - case["std"])[live].max()))


# ---- the Dataset ------------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_seeded_frame_set(golden, case):
    assert tuple(golden["lengths"]) == tc.LENGTHS and case["raw"].shape == (tc.N_FRAMES, 54)
    assert (case["raw"][:, :15] == 0).all()
    assert np.isnan(case["raw"]).sum() == 1 and np.isposinf(case["raw"]).sum() == 1 and np.isneginf(case["raw"]).sum() == 1
    m = case["mask"]
    assert np.isnan(m).sum() == 1 and np.isposinf(m).sum() == 1 and np.isneginf(m).sum() == 1
    assert (m[np.isfinite(m)] > 1).sum() == 1 and (m[np.isfinite(m)] < 0).sum() == 1
    assert golden["ds.features"].shape == (tc.N_FRAMES, 594) and golden["ds2.features"].shape == (15, 594)


def test_statistics_against_the_reference(golden, case):
    em, es = e32(golden, case)
    print("e32: mean %.3e std %.3e" % (em, es))
    assert 0 < em < 1e-5 and 0 < es < 1e-5                  # the reference's float32 sums over 157 rows; c0's mean is about 40
    mean, std = tc.stats_rule(case["mean"], case["std"])
    assert (std[:15] == 1.0).all() and (mean[:15] == 0.0).all() and (golden["ds.feat_std"][:15] == 1.0).all()
    assert (np.arange(594) % 54 < 15)[golden["ds.feat_std"] == 1.0].all()
    x = tc.normalise64(case["rows"], golden["ds.feat_mean"], golden["ds.feat_std"])
    assert np.abs(x - golden["ds.features"]).max() < 2e-6
    assert np.array_equal(tc.targets64(case["mask"]).astype(np.float32), golden["ds.masks"])
    assert np.array_equal(golden["ds2.feat_mean"], golden["ds.feat_mean"]) and np.array_equal(golden["ds2.feat_std"], golden["ds.feat_std"])
    rows2 = tc.context_rows64(case["raw"][:15], tc.bounds(tc.LENGTHS[:3]))
    assert np.abs(tc.normalise64(rows2, golden["ds.feat_mean"], golden["ds.feat_std"]) - golden["ds2.features"]).max() < 2e-6


@pytest.mark.parametrize("mutant", tc.CLAMP_MUTANTS)
def test_clamp_mutants_break_the_statistics_bound_and_the_rows(golden, case, mutant):
    em, es = e32(golden, case)
    rows = tc.context_rows64(case["raw"], tc.bounds(), mutant=mutant)
    mean, std = tc.stats64(rows)
    assert np.abs(mean - case["mean"]).max() > 16 * em and np.abs(std - case["std"]).max() > 16 * es
    # the staged rows are compared bit for bit on the GPU: the mutant differs in fp16 already
    a = dn.rnd(tc.normalise64(rows, golden["ds.feat_mean"], golden["ds.feat_std"]), torch.float16)
    b = dn.rnd(tc.normalise64(case["rows"], golden["ds.feat_mean"], golden["ds.feat_std"]), torch.float16)
    assert (a != b).any()


# ---- the trajectory -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trajectory(golden):
    Ws, bs = tc.fixture_params()
    x = golden["ds.features"].astype(np.float64)
    t = golden["ds.masks"].astype(np.float64)
    return tc.train64(Ws, bs, x, t, tc.batches(), 2), tc.interleave(Ws, bs)


def snapshot(golden, k, like):
    keys = ["network.%d.%s" % (3 * l, n) for l in range(4) for n in ("weight", "bias")]
    return [golden["step%d.%s" % (k, key)].astype(np.float64) for key in keys]


def pick(params_flat, like):
    cur = tc.unflat(params_flat, like)
    cur[0] = cur[0][:, dn.GRAD_COLS]
    return cur


def test_trajectory_against_the_reference(golden, trajectory):
    r, like = trajectory
    assert np.abs(np.asarray(r["loss"]) - golden["loss"]).max() < 2e-6
    assert np.abs(np.asarray(r["norm"]) / golden["norm"] - 1.0).max() < 1e-5
    assert (golden["norm"] > tc.MAX_NORM).any() and (golden["norm"] < tc.MAX_NORM).any()
    assert (np.abs(golden["norm"] / tc.MAX_NORM - 1.0) > 0.01).all()
    for k in golden["snapshots"]:
        for got, want in zip(pick(r["params"][k - 1], like), snapshot(golden, k, like)):
            assert dn.rel(got, want) < 1e-5, k
    assert np.abs(np.asarray(r["epoch"]) - golden["train_loss"]).max() < 2e-6
    x2, t2 = golden["ds2.features"].astype(np.float64), golden["ds2.masks"].astype(np.float64)
    for e, k in enumerate((5, 10)):
        assert abs(tc.validate64(r["params"][k - 1], like, x2, t2, tc.batches(15)) - golden["val_loss"][e]) < 2e-6


def test_per_element_average_is_caught(golden, trajectory):
    """the ragged last batch weighs as much as a full one: the per-element mean is further from the reference than the bound"""
    r, _ = trajectory
    sizes = [len(b) for b in tc.batches()]
    wrong = tc.epoch_loss(r["loss"][:5], sizes, mutant="per_element_mean")
    assert abs(wrong - golden["train_loss"][0]) > 100 * 2e-6
    assert abs(tc.epoch_loss(r["loss"][:5], sizes) - golden["train_loss"][0]) < 2e-6


@pytest.fixture(scope="module")
def adam_case(golden):
    return tc.adam_case(golden["ds.features"], golden["ds.masks"])


def test_adam_mutants_fail_the_assertion_of_the_gpu_test(adam_case):
    """The configuration and the assertion of tests/test_dnn_train_gpu.py::test_flat_adam, evaluated on the CPU: five steps on the
    fixture's gradients, the third skipped, p / m / v within 16 x e32 and every norm within 1e-6, at each decay the GPU test runs.
    The float64 rule passes it at both decays.  The decoupled decay fails it at both.  The decay term in the norm moves every
    figure by less than a fiftieth of its bound at the reference's 1e-5 - that decay cannot tell the two norms apart, which is
    why the GPU test also runs 0.1 - and fails it at 0.1, where the clipped steps' norms differ in the first digits."""
    p0, grads = adam_case
    caught = {}
    for wd in tc.ADAM_DECAYS:
        e32 = tc.adam_e32(p0, grads, wd)
        *want, norms = tc.adam_run64(p0, grads, wd)
        assert any(n > tc.MAX_NORM for n in norms) and any(n < tc.MAX_NORM for n in norms)
        assert norms[0] > tc.MAX_NORM and norms[tc.ADAM_SKIP + 2] > tc.MAX_NORM          # applied steps on the clipped side
        assert tc.adam_within(want, want, e32, norms, norms)
        for mutant in tc.ADAM_MUTANTS:
            *got, bad_norms = tc.adam_run64(p0, grads, wd, mutant=mutant)
            caught[(mutant, wd)] = not tc.adam_within(got, want, e32, bad_norms, norms)
            print("Adam mutant %s at wd %g: p %.2e (bound %.2e)  m %.2e (%.2e)  v %.2e (%.2e)  norm %.2e (%.0e)  caught %s"
                  % ((mutant, wd) + tuple(x for g, w, e in zip(got, want, e32) for x in (float(np.abs(g - w).max()), 16 * e))
                     + (max(abs(a / b - 1.0) for a, b in zip(bad_norms, norms)), tc.ADAM_NORM_RTOL, caught[(mutant, wd)])))
    assert caught[("decoupled_decay", tc.WD)] and caught[("decoupled_decay", 0.1)] and caught[("norm_with_decay", 0.1)]
    assert not caught[("norm_with_decay", tc.WD)]                                          # (what the second decay is there for)


def test_adam_l2_against_torch_float64():
    """5 steps, one of them forced to skip, against torch.optim.Adam + clip_grad_norm_ in float64"""
    rng = np.random.default_rng(5)
    n = 300
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * s for s in (0.1, 1.0, 0.05, 2.0, 0.2)]       # norms on both sides of the clip
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=tc.LR, weight_decay=tc.WD)
    p, m, v, step = p0.copy(), np.zeros(n), np.zeros(n), 0
    clipped = []
    for k, g in enumerate(grads):
        skip = k == 2
        p, m, v, step, norm, skipped = tc.adam_l2_step64(p, g, m, v, step, skip=skip)
        assert skipped == skip
        if not skip:
            q.grad = torch.from_numpy(g.copy())
            total = torch.nn.utils.clip_grad_norm_([q], tc.MAX_NORM)
            assert abs(float(total) - norm) <= 1e-12 * norm
            clipped.append(norm > tc.MAX_NORM)
            opt.step()
        assert np.abs(q.detach().numpy() - p).max() < 1e-13
    assert step == 4 and any(clipped) and not all(clipped)


def test_plateau_rule_against_torch():
    from sincformer_metacog_speech_enhancement_amd.training.dnn_training import PlateauRule
    losses = [1.0, 0.9] + [0.95] * 7 + [0.8] + [0.85] * 6 + [0.85] * 80          # two reductions, then down to the floor
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([q], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='min', factor=0.5, patience=5, min_lr=1e-6)
    rule = PlateauRule(1e-3, factor=0.5, patience=5, min_lr=1e-6)
    want = []
    for l in losses:
        sch.step(l)
        want.append(opt.param_groups[0]["lr"])
    got = [rule.step(l) for l in losses]
    assert got == want == tc.plateau(losses, 1e-3)
    assert want[6] == 1e-3 and want[7] == 5e-4 and want[14] == 5e-4 and want[15] == 2.5e-4 and want[-1] == 1e-6 and len(set(want)) >= 4


# ---- the loss scale ----------------------------------------------------------------------------------------------------------------
def test_underflow_share_of_the_first_batch(golden):
    """what the loss scale buys, by the CPU emulation: at S = 1 most of the fp16 cotangent is subnormal or 0, at the initial scale
    the share is within the GPU test's 1e-3 cap"""
    Ws, bs = tc.fixture_params()
    idx = tc.batches()[0]
    y = dn.forward64(Ws, bs, golden["ds.features"][idx].astype(np.float64), fmt=torch.float16)[0]
    _, dz = tc.loss_dz64(y, golden["ds.masks"][idx].astype(np.float64))
    s1, s_init = tc.subnormal_share(dz, 1.0), tc.subnormal_share(dz, tc.INIT_SCALE)
    print("fp16 cotangent of the first batch: 0 or subnormal share %.4f at S = 1, %.2e at S = %g" % (s1, s_init, tc.INIT_SCALE))
    assert s_init <= 1e-3 and s1 > 0.25


# ---- the entry points' guards and the wrappers' costs ----------------------------------------------------------------------------
def test_argument_guards_without_a_gpu(built):
    L = built.load()
    one = ctypes.c_void_p(16)

    def layer(raw=one, bounds=one, index=one, mean=one, std=one, M=4, K=594, D=54, ctx=5, n_frames=10, dtype=1):
        return L.sfm_dnn_layer_indexed(raw, bounds, index, mean, std, one, one, one, None, M, 64, K, n_frames, D, ctx, 640, 64, 64, 0, 0, 1,
                                       0.0, 0, dtype, None)
    assert layer(dtype=7) == -1                              # control: every shape check passed, the format is refused last
    assert layer(index=None) == -1 and layer(bounds=None) == -1 and layer(raw=None) == -1
    assert layer(std=None) == -1 and layer(mean=None) == -1                       # statistics given in half
    assert layer(D=53, K=583) == -2 and layer(K=592) == -2 and layer(M=0) == -2 and layer(n_frames=0) == -2 and layer(ctx=65) == -2
    assert layer(D=6, K=66) == -2
    # the existing entry point still has three modes: the indexed one is not reachable through it
    assert L.sfm_dnn_layer(one, None, None, None, one, one, one, 3, 4, 64, 594, 0, 1, 54, 5, 640, 64, 64, 0, 1, 0.0, 0, 1, None) == -1

    def moments(raw=one, bounds=one, N=5, D=54, ctx=5):
        return L.sfm_context_moments(raw, bounds, one, one, one, N, D, ctx, None)
    assert moments(raw=None) == -1 and moments(bounds=None) == -1 and moments(bounds=ctypes.c_void_p(12)) == -1
    assert moments(N=0) == -2 and moments(D=0) == -2 and moments(ctx=-1) == -2

    def loss(y=one, index=one, M=4, C=64, ldz=64, dtype=7, n_frames=5, out=one):
        return L.sfm_mse_gather_loss(y, one, index, None, None, ldz, out, None, None, one, M, C, n_frames, dtype, None)
    assert loss() == -1                                      # control: refused for the format only
    assert loss(index=None) == -1 and loss(y=None) == -1 and loss(out=None) == -1
    assert loss(M=0, dtype=1) == -2 and loss(ldz=60, dtype=1) == -2 and loss(ldz=32, dtype=1) == -2 and loss(n_frames=0, dtype=1) == -2

    def adam(p=one, n=8, spans=None, touched=None, growth=2.0, eps=1e-8, omb=0.1):
        return L.sfm_adam_l2_step(p, one, one, one, n, one, 1e-3, omb, 0.001, eps, 1e-5, 1.0, 5.0, spans, touched, 0, None, growth, 0.5,
                                  2000, None)
    assert adam(p=None) == -1 and adam(n=0) == -2 and adam(spans=one) == -1 and adam(growth=0.5) == -1 and adam(eps=0.0) == -1
    assert adam(n=0, omb=0.0) == -1 and adam(n=0, omb=1.5) == -1                   # 1 - beta outside (0, 1]


def test_launch_costs(monkeypatch):
    from sincformer_metacog_speech_enhancement_amd import ops
    rec = ops_stub.install(monkeypatch)
    ops.set_compute_dtype(torch.float16)
    N, D, M = 1000, 54, 256
    raw, bounds = torch.zeros(N, D), torch.zeros(N, 2, dtype=torch.int32)
    index = torch.zeros(M, dtype=torch.int32)
    stat = torch.ones(594)
    pw = ops.PackedWeight(torch.zeros(1024, 640, dtype=torch.float16), torch.zeros(1024), 1024, 594, 1, 594, False)
    ops.context_moments(raw, bounds, 5)
    ops.dnn_layer_indexed(raw, bounds, index, pw, context=5, act="relu", mean=stat, std=stat)
    ops.dnn_layer_indexed(raw, bounds, index, pw, context=5, act="relu", mean=stat, std=stat, a16_out=True)
    ops.mse_gather_loss(torch.zeros(M, 64), torch.zeros(N, 64), index)
    ops.mse_gather_loss(torch.zeros(M, 64), torch.zeros(N, 64), index, need_dz=False)
    w = 2.0 * 1024 * 640 + 4.0 * 1024 + 2.0 * M * 1024
    a = 4.0 * M * 594 + 12.0 * M + 8.0 * 594
    assert rec == [
        ("sfm_context_moments", "context_moments", 5.0 * N * 594, 2.0 * (4.0 * N * D + 8.0 * N) + 8.0 * 594, "N1000 D54 ctx5"),
        ("sfm_dnn_layer_indexed", "dnn_layer", 2.0 * M * 1024 * 594, a + w, "M256 N1024 K594 a3 act1 o2"),
        ("sfm_dnn_layer_indexed", "dnn_layer", 2.0 * M * 1024 * 594, a + 2.0 * M * 640 + w, "M256 N1024 K594 a3 act1 o2"),
        ("sfm_mse_gather_loss", "mse_loss", 8.0 * M * 64, 8.0 * M * 64 + 4.0 * M + 2.0 * M * 64, "M256 C64 dz1"),
        ("sfm_mse_gather_loss", "mse_loss", 3.0 * M * 64, 8.0 * M * 64 + 4.0 * M, "M256 C64 dz0"),
    ]


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_and_dtypes(tmp_path, golden):
    """the dictionary the reference's load_model reads: its keys, numpy float32 statistics, a state dict its module accepts"""
    from sincformer_metacog_speech_enhancement_amd import models
    from sincformer_metacog_speech_enhancement_amd.training.dnn_training import TrainingPipeline
    pipe = object.__new__(TrainingPipeline)                  # the constructor needs the device; the checkpoint code does not
    pipe.mask_type, pipe.model_dir, pipe.device = "pcirm", str(tmp_path), torch.device("cpu")
    pipe.model = models.SpeechEnhancementDNN()
    pipe.feature_dim, pipe.mask_dim = 594, 64
    pipe.feat_mean, pipe.feat_std = golden["ds.feat_mean"].astype(np.float64), torch.from_numpy(golden["ds.feat_std"])
    best, final = pipe._save_best(), pipe.save_model()
    assert os.path.basename(best) == "best_pcirm.pt" and os.path.basename(final) == "dnn_pcirm_final.pt"
    keys = ["model_state", "mask_type", "feature_dim", "mask_dim", "feat_mean", "feat_std"]
    ck = torch.load(best, map_location="cpu", weights_only=False)
    assert list(ck) == keys and list(torch.load(final, map_location="cpu", weights_only=False)) == keys + ["device"]
    for k in ("feat_mean", "feat_std"):
        assert type(ck[k]) is np.ndarray and ck[k].dtype == np.float32 and ck[k].shape == (594,)
    assert np.array_equal(ck["feat_std"], golden["ds.feat_std"]) and ck["mask_type"] == "pcirm" and ck["feature_dim"] == 594
    # the reference's module: [Linear, ReLU, Dropout] x 3, Linear, Sigmoid under `network` - built here from torch alone
    from torch import nn
    layers = [nn.Linear(594, 1024), nn.ReLU(), nn.Dropout(0.2)]
    for _ in range(2):
        layers += [nn.Linear(1024, 1024), nn.ReLU(), nn.Dropout(0.2)]
    layers += [nn.Linear(1024, 64), nn.Sigmoid()]
    ref = nn.Module()
    ref.network = nn.Sequential(*layers)
    ref.load_state_dict(ck["model_state"])
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in ck["model_state"].values())
