"""CPU checks of AdversarialLoss: the float64 restatement of tests/adversarial_cases.py against what the reference returned
(tests/golden/g16_adversarial.npz: losses, gradients, spectral-norm vectors after the calls), the mirror's keys / shapes / alias
/ seeded init against g16_adversarial_state.json, a strict load of a state with the reference's keys, the argument guards
(no library needed) and the launch costs the new ops wrappers state.

Bounds, by the rule of tests/test_losses_gpu.py: e32 = the float32 evaluation of the restatement against the float64 one; the
fixture (the reference's own fp32 evaluation) lies within max(16 x e32, 16 x 2^-24 x the quantity's scale) of the float64 form."""
import json
import os

import numpy as np
import pytest
import torch

import adversarial_cases as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24
K = 16.0


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "g16_adversarial.npz"))


@pytest.fixture(scope="module")
def state_fixture():
    with open(os.path.join(GOLDEN, "g16_adversarial_state.json")) as f:
        return json.load(f)


_runs = {}


def _run(name, mode, dtype):
    """the restatement on a case, computed once per (case, objective, dtype) and shared"""
    key = (name, mode, dtype)
    if key not in _runs:
        c = ac.case(name)
        _runs[key] = ac.run(ac.init_state(ac.CASES[name][0]), mode, c["clean"], c["enh"], dtype)
    return _runs[key]


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("name", list(ac.CASES))
def test_restatement_equals_the_reference(fixture, name, mode):
    assert int(fixture[name + ".seed"]) == ac.CASES[name][3]
    r64, r32 = _run(name, mode, torch.float64), _run(name, mode, torch.float32)
    pre = "%s.%s." % (name, mode)
    l64 = float(r64["loss"])
    e32 = abs(float(r32["loss"]) - l64)
    obs = abs(float(fixture[pre + "loss"]) - l64)
    print("ROW | %s %s loss | e32 %.2e | observed %.2e" % (name, mode, e32, obs))
    assert obs <= max(K * e32, K * U32 * abs(l64))
    if mode == "d":
        assert r64["grad"] is None or not r64["grad"].any()          # enhanced is detached
    else:
        e32 = ac.rel_rmse(r32["grad"], r64["grad"])
        obs = ac.rel_rmse(torch.from_numpy(fixture[pre + "grad"]), r64["grad"])
        print("ROW | %s %s grad | e32 %.2e | observed %.2e" % (name, mode, e32, obs))
        assert obs <= max(K * e32, K * U32)
    names = [str(n) for n in fixture[name + ".param_names"]]
    assert names == ac.param_keys(r64["state"])
    for k, want in zip(names, fixture[pre + "pgrad_sums"]):
        g64, g32 = r64["pgrads"][k], r32["pgrads"][k]
        if np.isnan(want):
            assert g64 is None or not g64.any(), k               # the heads under feature matching
            continue
        e32 = abs(float(g32.double().sum()) - float(g64.sum()))
        assert abs(float(want) - float(g64.sum())) <= max(K * e32, K * U32 * float(g64.abs().sum())), k
    for i in range(3):
        for k in ("weight_u", "weight_v"):
            key = "discriminators.%d.layers.0.%s" % (i, k)
            v64, v32 = r64["state"][key], r32["state"][key]
            e32 = float((v32.double() - v64).abs().max())
            obs = float((torch.from_numpy(fixture["%su%d.%s" % (pre, i, k)]).double() - v64).abs().max())
            assert obs <= max(K * e32, K * U32), key


def test_a_mistaken_call_count_misses_the_bound(fixture):
    """the spectral-norm vectors are far from converged after init: a restatement that does not iterate on the second (fake)
    call of discriminator_loss is far outside the bound the right one keeps"""
    name = "a3_default_t64"
    c = ac.case(name)
    state = ac.cast_state(ac.init_state(129), torch.float64)
    with torch.no_grad():
        wrong = 0.0
        real, fake = c["clean"].double(), c["enh"].double()
        for i in range(3):
            ro, _ = ac.disc(state, i, real, True)
            fo, _ = ac.disc(state, i, fake, False)
            wrong = wrong + (ro - 1).pow(2).mean() + fo.pow(2).mean()
            real, fake = ac._pool(real), ac._pool(fake)
        wrong = float(wrong) / 3
    want = float(fixture[name + ".d.loss"])
    assert abs(wrong - want) > 1e-4 * abs(want)


def test_case_shapes_are_the_documented_ones():
    assert {n: v[:3] for n, v in ac.CASES.items()} == {"a1_odd_f9_t37": (9, 2, 37), "a2_shortest_t4": (129, 3, 4),
                                                       "a3_default_t64": (129, 2, 64), "a4_wide_f257_t16": (257, 1, 16)}
    c = ac.case("a3_default_t64")
    assert c["enh"].shape == (2, 129, 64) and c["enh_re"].shape == (2, 64, 129)
    assert ac.rel_rmse(ac.magnitudes(c["enh_re"], c["enh_im"]), c["enh"]) < 1e-6


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def _mirror(input_dim=None):
    from sincformer_metacog_speech_enhancement_amd.training import AdversarialLoss
    torch.manual_seed(ac.INIT_SEED)
    return AdversarialLoss(input_dim=input_dim)


@pytest.mark.parametrize("dim", [9, 129, 257])
def test_mirror_state_equals_the_reference(state_fixture, dim):
    m = _mirror(dim)
    want = state_fixture[str(dim)]
    sd = m.state_dict()
    assert list(sd) == list(want["keys"]) and len(sd) == 72
    assert len(list(m.parameters())) == want["parameters"] == 26
    assert sum(p.numel() for p in m.parameters()) == want["elements"]
    for k, w in want["keys"].items():
        got = ac.summary(sd[k])
        assert got["shape"] == w["shape"], k
        assert got["first"] == w["first"] and got["sum"] == w["sum"], k           # the same draws, bit for bit
    assert m.discriminator is m.discriminators[0]
    mine = ac.init_state(dim)                                                       # the restatement draws the same init
    assert all(torch.equal(mine[k], sd[k]) for k in mine) and list(mine) == [k for k in sd if k.startswith("discriminators.")]


def test_default_width_and_element_count(state_fixture):
    m = _mirror()
    assert m.n_freq == 129 and sum(p.numel() for p in m.parameters()) == 1223683


def test_strict_load_of_a_state_with_the_reference_keys(state_fixture):
    m = _mirror(129)
    state = {k: torch.full(v["shape"], 0.25) for k, v in state_fixture["129"]["keys"].items()}
    m.load_state_dict(state, strict=True)
    assert float(m.discriminators[2].layers[6].weight_orig.detach().sum()) == 0.25 * 128 * 3
    assert m.discriminator.layers[0].weight_u.data_ptr() == m.discriminators[0].layers[0].weight_u.data_ptr()
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in state.items() if not k.endswith("layers.0.weight_u")}, strict=True)


def test_guards_raise_without_the_library(monkeypatch):
    from sincformer_metacog_speech_enhancement_amd import lib, ops
    from sincformer_metacog_speech_enhancement_amd.training import AdversarialLoss, SubDiscriminator

    def no_library():
        raise AssertionError("a guard let a call through to the library")
    monkeypatch.setattr(lib, "load", no_library)
    m = _mirror(129)
    x = torch.rand(2, 129, 8)
    for call in (lambda: m.generator_loss(x), lambda: m.discriminator_loss(x, x), lambda: m.feature_matching_loss(x, x),
                 lambda: m.generator_loss_cl(x.transpose(1, 2), x.transpose(1, 2)), lambda: m.discriminator(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # shapes: the device check comes first, so it is switched off here to reach the others on CPU tensors
    monkeypatch.setattr(AdversarialLoss, "_require_device", lambda self, *t: None)
    monkeypatch.setattr(SubDiscriminator, "_require_device", lambda self, *t: None)
    with pytest.raises(ValueError, match="rank-3"):
        m.generator_loss(torch.rand(129, 8))
    with pytest.raises(ValueError, match="frequency bins"):
        m.generator_loss(torch.rand(2, 128, 8))
    with pytest.raises(ValueError, match="frequency bins"):
        m.generator_loss_cl(torch.rand(2, 129, 8), torch.rand(2, 129, 8))           # [B, T, F] is expected there
    with pytest.raises(ValueError, match="shapes differ"):
        m.discriminator_loss(torch.rand(2, 129, 8), torch.rand(2, 129, 9))
    with pytest.raises(ValueError, match="shapes differ"):
        m.feature_matching_loss_cl(x.transpose(1, 2), x.transpose(1, 2), x.transpose(1, 2), torch.rand(2, 7, 129))
    with pytest.raises(ValueError, match="4 frames"):
        m.generator_loss(torch.rand(2, 129, 3))
    with pytest.raises(ValueError, match="4 frames"):
        m.discriminator(torch.rand(2, 129, 3))
    wide = AdversarialLoss(input_dim=513)
    with pytest.raises(NotImplementedError, match="at most 512"):
        wide.generator_loss(torch.rand(1, 513, 8))
    assert ops.ADV_MAX_WIDTH == 512


def test_layer_plan():
    """what the kernels are told about SubDiscriminator(129, [64, 128, 256, 512]): Cin padded to a power of two, packed sizes"""
    from sincformer_metacog_speech_enhancement_amd import ops
    plan, n16, n32 = ops.adv_plan(129, [64, 128, 256, 512])
    assert [(p["N"], p["Cin"], p["Cp"], p["ksize"], p["stride"], p["Npad"], p["Kpad"]) for p in plan] == [
        (64, 129, 256, 5, 2, 64, 1280), (128, 64, 64, 5, 2, 128, 320), (256, 128, 128, 5, 2, 256, 640),
        (512, 256, 256, 5, 1, 512, 1280), (1, 512, 512, 3, 1, 1, 1536)]
    assert all(p["off16"] % 8 == 0 for p in plan) and n16 == 943616 and n32 == 7320
    assert [p["Cp"] for p in ops.adv_plan(257, [32])[0]] == [512, 32] and ops.adv_plan(9, [32])[0][0]["Cp"] == 16


# ---- launch costs: stub library, recorded _call, literal expectations (tests/test_launch_costs_host.py) ------------------------
@pytest.fixture
def launches(monkeypatch):
    import ops_stub
    from sincformer_metacog_speech_enhancement_amd import ops
    rec = ops_stub.install(monkeypatch, tags=False)
    monkeypatch.setattr(ops, "_ws", lambda n, device, dtype=torch.float32: torch.zeros(1, dtype=dtype))
    return rec


def test_adversarial_launch_costs(launches):
    from sincformer_metacog_speech_enhancement_amd import ops
    ops.set_compute_dtype(torch.float16)
    F16 = torch.float16
    B, F, T, Cp, C = 2, 129, 64, 256, 128
    plan, n16, n32 = ops.adv_plan(9, [32, 64])               # weights: 32*9*5 + 64*32*5 + 64*3 = 11872 elements
    table = torch.zeros(len(plan), 16, dtype=torch.int64)
    ops.adv_sn_fwd(table, plan, n16, n32, True)
    ops.adv_sn_fwd(table, plan, n16, n32, False)
    w = torch.zeros(64, 32, 5)
    ops.adv_sn_bwd(torch.zeros(64, 5, 32), w, torch.zeros(64), torch.zeros(160), torch.zeros(1), torch.zeros(64, 32, 5), 32, False)
    ops.adv_sn_bwd(torch.zeros(64, 5, 32), w, torch.zeros(64), torch.zeros(160), torch.zeros(1), torch.zeros(64, 32, 5), 32, True)
    ops.adv_stage(torch.zeros(B, F, T), None, Cp, True)
    ops.adv_stage(torch.zeros(B, T, F), torch.zeros(B, T, F), Cp, False)
    ops.adv_stage_bwd(torch.zeros(B, T, Cp), None, None, B, F, T)
    ops.adv_stage_bwd(torch.zeros(B, T, Cp), torch.zeros(B, T, F), torch.zeros(B, T, F), B, F, T)
    z = torch.zeros(B, 32, 64)
    ops.adv_leaky(z)
    ops.adv_leaky(z, z_real=z, loss=torch.zeros(1, dtype=torch.float64), scale=0.5)
    ops.adv_leaky_bwd(z, z, None, torch.ones(1), 0.0, 0.1)
    ops.adv_leaky_bwd(z, z, z, torch.ones(1), 0.5, 0.5)
    ops.adv_pool(torch.zeros(B, T, F), Cp, True)
    ops.adv_pool_bwd(torch.zeros(B, T // 2, Cp), torch.zeros(B, T, Cp))
    a16 = torch.zeros(B, 8, C, dtype=F16)
    ops.adv_head(a16, a16, torch.zeros(3 * C, dtype=F16), torch.zeros(3 * C, dtype=F16), torch.zeros(1),
                 torch.zeros(1, dtype=torch.float64), 1.0, 0.1)
    ops.adv_head_bwd(a16, torch.zeros(3 * C, dtype=F16), torch.zeros(B, 8), torch.ones(1), 0.1, 0.1, 1.0, False)
    ops.adv_head_bwd(a16, torch.zeros(3 * C, dtype=F16), torch.zeros(B, 8), torch.ones(1), 0.1, 0.1, 1.0, True)
    n = B * F * T                                              # 16512
    assert launches == [
        ("sfm_adv_sn_fwd", "adv_sn", 71232.0, 189952.0 + 4.0 * n16),           # W / sigma leaves as hi and lo words
        ("sfm_adv_sn_fwd", "adv_sn", 47488.0, 142464.0 + 4.0 * n16),
        ("sfm_adv_sn_bwd", "adv_sn", 61440.0, 204800.0),
        ("sfm_adv_sn_bwd", "adv_sn", 61440.0, 245760.0),
        ("sfm_adv_stage", "adv_stage", 0.0, 4.0 * n + 4.0 * B * T * Cp + 4.0 * n),
        ("sfm_adv_stage", "adv_stage", 4.0 * n, 8.0 * n + 4.0 * B * T * Cp),
        ("sfm_adv_stage_bwd", "adv_stage", 0.0, 8.0 * n),
        ("sfm_adv_stage_bwd", "adv_stage", 6.0 * n, 20.0 * n),
        ("sfm_adv_leaky", "adv_leaky", 4096.0, 32768.0),
        ("sfm_adv_leaky", "adv_leaky", 16384.0, 49152.0),
        ("sfm_adv_leaky_bwd", "adv_leaky", 12288.0, 40960.0),
        ("sfm_adv_leaky_bwd", "adv_leaky", 20480.0, 57344.0),
        ("sfm_adv_pool", "adv_pool", 33024.0, 66048.0 + 65536.0 + 33024.0),
        ("sfm_adv_pool_bwd", "adv_pool", 98304.0, 262144.0 + 65536.0),
        ("sfm_adv_head", "adv_head", 12288.0, 8192.0 + 1536.0 + 64.0),
        ("sfm_adv_head_bwd", "adv_head", 12288.0, 8192.0 + 64.0 + 768.0),
        ("sfm_adv_head_bwd", "adv_head", 24576.0, 12288.0 + 64.0 + 768.0),
    ]
