"""CPU checks of the PSO search (optimizer/pso.py, masks.compute_opt_pcirm with use_pso=True): the restatements of
tests/pso_cases.py against what the reference did (tests/golden/g18_pso.npz), the draw order, the argument guards of the five
entry points of csrc/pso.hip and of the Python layer, and the launch costs the wrappers state."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ops_stub
import pso_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g18_pso.npz"))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


@pytest.mark.parametrize("name", list(pc.TRAJECTORIES))
def test_restated_fitness_equals_every_call_of_the_reference(golden, name):
    calls = golden[name + ".calls"]
    got = pc.fitness_of(pc.TRAJECTORIES[name][0], calls[:, 0])
    err = float(np.abs(got - calls[:, 1]).max())
    print("ROW | %s restated fitness vs the reference, %d calls | bound %.3g | observed %.3g" % (name, len(calls), pc.TOL, err))
    assert err <= pc.TOL
    assert float(golden[name + ".margins"].min()) >= pc.MARGIN          # the condition the tolerance rests on
    assert calls[:, 1].max() - calls[:, 1].min() > 1e-2                 # not a flat landscape


@pytest.mark.parametrize("name", list(pc.TRAJECTORIES))
def test_restated_swarm_reproduces_the_reference_history_bitwise(golden, name):
    _, N, K, seed = pc.TRAJECTORIES[name]
    calls = golden[name + ".calls"]
    rounds = calls[:, 1].reshape(-1, N)
    rep = pc.pso(lambda x, it: rounds[it], golden[name + ".draws"], N, K)
    assert same_bits(rep["positions"].reshape(-1), calls[:, 0])         # the reference asked for exactly these positions
    for k in ("gbest_fitness", "gbest_position", "mean_fitness"):
        assert same_bits(rep[k], golden[name + "." + k]), k
    assert same_bits(rep["best_position"], golden[name + ".middle"])


@pytest.mark.parametrize("name", list(pc.RECURRENCES))
def test_restated_swarm_on_the_quadratics(golden, name):
    t, maximize, w, c1, c2, K, seed = pc.RECURRENCES[name]
    f = pc.quadratic(t, maximize)
    rep = pc.pso(lambda x, it: f(x), golden[name + ".draws"], pc.REC_N, K, w, c1, c2, pc.BOUNDS, maximize)
    for k in ("gbest_fitness", "gbest_position", "mean_fitness", "positions", "fitness"):
        assert same_bits(rep[k], golden[name + "." + k]), k
    assert rep["iterations_run"] == int(golden[name + ".iterations_run"]) and same_bits(rep["best_position"], golden[name + ".best"])
    assert (rep["iterations_run"] < K) == (name == "early")


def test_pso_draws_follow_the_reference_order(golden):
    from sincformer_metacog_speech_enhancement_amd.optimizer import pso_draws
    for name, (_, N, K, seed) in pc.TRAJECTORIES.items():
        np.random.seed(seed)
        assert same_bits(pso_draws(N, K, pc.BOUNDS), golden[name + ".draws"]), name
    for name, (t, maximize, w, c1, c2, K, seed) in pc.RECURRENCES.items():
        np.random.seed(seed)
        assert same_bits(pso_draws(pc.REC_N, K, pc.BOUNDS), golden[name + ".draws"]), name
    np.random.seed(5)
    d = pso_draws(4, 3, (-2.0, 6.0))
    assert d.shape == (2 * 4 + 2 * 4 * 3,) and -2.0 <= d[:4].min() and d[:4].max() < 6.0 and np.abs(d[4:8]).max() <= 0.8
    np.random.seed(5)
    assert same_bits(pso_draws(), pc.draws_after_seed(5, 30, 100))      # the defaults of config.py


def test_config_defaults_are_the_reference_ones():
    from sincformer_metacog_speech_enhancement_amd import config
    assert (config.PSO_NUM_PARTICLES, config.PSO_MAX_ITER, config.PSO_W, config.PSO_C1, config.PSO_C2, config.PSO_BOUNDS) == \
        (30, 100, 0.7, 1.5, 1.5, (0.0, 1.0))


def test_optimizer_imports_without_a_device():
    code = ("import os; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['CUDA_VISIBLE_DEVICES'] = ''\n"
            "from sincformer_metacog_speech_enhancement_amd.optimizer import ParticleSwarmOptimizer, pso_draws\n"
            "p = ParticleSwarmOptimizer(lambda x: x)\n"
            "assert (p.N, p.max_iter, p.w, p.c1, p.c2, p.lb, p.ub, p.maximize) == (30, 100, 0.7, 1.5, 1.5, 0.0, 1.0, True)\n"
            "assert sorted(p.get_convergence_history()) == ['gbest_fitness', 'gbest_position', 'mean_fitness']\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_argument_errors_of_the_python_layer():
    from sincformer_metacog_speech_enhancement_amd import masks
    from sincformer_metacog_speech_enhancement_amd.optimizer import ParticleSwarmOptimizer, SwarmState, pso_draws
    for kw in ({"num_particles": 257}, {"num_particles": -1}, {"max_iter": -3}, {"bounds": (1.0, 1.0)}, {"bounds": (2.0, 1.0)}):
        with pytest.raises(ValueError, match="PSO"):
            ParticleSwarmOptimizer(lambda x: x, **kw)
        with pytest.raises(ValueError, match="PSO"):
            pso_draws(kw.get("num_particles"), kw.get("max_iter"), kw.get("bounds"))
    with pytest.raises(ValueError, match="draws"):
        SwarmState(np.zeros((1, 7)), 4, 3, 0.7, 1.5, 1.5, (0.0, 1.0), device="cpu")
    s = SwarmState(np.arange(32.0), 4, 3, 0.7, 1.5, 1.5, (0.0, 1.0), device="cpu")
    assert s.B == 1 and s.pos.tolist() == [[0.0, 1.0, 2.0, 3.0]] and s.vel.tolist() == [[4.0, 5.0, 6.0, 7.0]]
    assert s.hist.shape == (1, 4, 11) and s.params.tolist() == [0.7, 1.5, 1.5, 0.0, 1.0]
    x, sig = torch.zeros(2, 2), np.zeros(400, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="PSO"):               # nothing to score
        masks.compute_opt_pcirm(x)
    with pytest.raises(NotImplementedError, match="PSO"):
        masks.compute_opt_pcirm(x, noisy_signal=sig)
    with pytest.raises(ValueError, match="PSO"):
        masks.compute_opt_pcirm(x, sig, sig, pso_config={"num_particles": 300})
    with pytest.raises(ValueError, match="PSO"):
        masks.compute_opt_pcirm(x, sig, sig, pso_config={"bounds": (0.5, 0.5)})
    with pytest.raises(ValueError, match="pso_config"):
        masks.compute_opt_pcirm(x, sig, sig, pso_config={"particles": 3})
    with pytest.raises(ValueError, match="steps"):
        masks.compute_opt_pcirm(x, sig, sig, num_steps=17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a host tensor is refused, not computed on the host
        masks.compute_opt_pcirm(x, sig, sig)


@pytest.fixture(scope="module")
def L():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def test_entry_points_refuse_bad_arguments_before_any_launch(L):
    one = ctypes.c_void_p(16)
    assert L.sfm_pso_frame_coef(None, one, one, one, 1, 4, 4, 3, None) == -1
    for B, C, T, M in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3), (1, 4, 4, 1), (1, 4, 4, 17), (65536, 4, 4, 3), (4, 32768, 32768, 3)):
        assert L.sfm_pso_frame_coef(one, one, one, one, B, C, T, M, None) == -2, (B, C, T, M)
    split = lambda *tail: L.sfm_pso_split(one, one, one, one, one, one, one, one, one, one, one, *tail, None)
    assert L.sfm_pso_split(one, one, one, one, one, one, one, one, one, None, one, 1, 100, 2, 160, 80, None) == -1
    for tail in ((0, 100, 2, 160, 80), (1, 0, 2, 160, 80), (1, 100, 0, 160, 80), (1, 100, 2, 160, 0), (1, 100, 2, 80, 160),
                 (65536, 100, 2, 160, 80), (40000, 65536, 2, 160, 80)):
        assert split(*tail) == -2, tail
    fit = lambda *tail: L.sfm_pso_fitness(*([one] * 12), *tail, None)
    assert L.sfm_pso_fitness(*([one] * 11), None, 1, 8, 103, 1, None) == -1
    for tail in ((0, 8, 103, 1), (1, 0, 103, 1), (1, 257, 103, 1), (1, 8, 0, 1), (1, 8, 1025, 1), (1, 8, 103, 0)):
        assert fit(*tail) == -2, tail

    def step(partial, fitness, *tail):
        return L.sfm_pso_step(partial, fitness, one, *([one] * 10), *tail, None)
    assert step(one, one, 1, 8, 1, 0, 4, 1) == -1                       # exactly one source of the fitness
    assert step(None, None, 1, 8, 1, 0, 4, 1) == -1
    assert L.sfm_pso_step(one, None, None, *([one] * 10), 1, 8, 1, 0, 4, 1, None) == -1
    for tail in ((0, 8, 1, 0, 4, 1), (1, 0, 1, 0, 4, 1), (1, 257, 1, 0, 4, 1), (1, 8, 1, 0, 0, 1), (1, 8, 1, 5, 4, 1),
                 (1, 8, 1, -1, 4, 1), (1, 8, 0, 0, 4, 1)):
        assert step(one, None, *tail) == -2, tail
    assert step(None, one, 1, 8, 0, 0, 0, 1) == -2
    assert L.sfm_pso_quantize(one, one, None, one, 1, 16, 3, None) == -1
    for B, CT, M in ((0, 16, 3), (1, 0, 3), (1, 16, 1), (1, 16, 17), (3, 2 ** 30, 3)):
        assert L.sfm_pso_quantize(one, one, one, one, B, CT, M, None) == -2, (B, CT, M)


def test_wrappers_state_their_launch_costs(monkeypatch):
    from sincformer_metacog_speech_enhancement_amd import ops
    from sincformer_metacog_speech_enhancement_amd.optimizer import SwarmState
    rec = ops_stub.install(monkeypatch)
    B, C, T, Lmax, N, K, F, NF = 2, 64, 50, 4000, 8, 3, 103, 38
    table = torch.zeros(7, dtype=torch.float64)
    a, b = ops.pso_frame_coef(torch.zeros(B, C, T), table, 3)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    ya, yb, cp, S = ops.pso_split(torch.zeros(B, Lmax), torch.zeros(B, Lmax), i32(B), i32(B + 1), a, b, B * Lmax, 160, 80)
    state = SwarmState(np.zeros((B, 2 * N + 2 * N * K)), N, K, 0.7, 1.5, 1.5, (0.0, 1.0), device="cpu")
    partial = torch.zeros(B, 5, N, dtype=torch.float64)
    spectra = tuple(torch.zeros(B * NF, F) for _ in range(6))
    ops.pso_fitness(spectra, i32(B + 1), i32(B), S, state.pos, state.stopped, partial, B * NF)
    ops.pso_step(state, 0, partial=partial, frame_off=i32(B + 1))
    ops.pso_step(state, 1, fitness=torch.zeros(B, N, dtype=torch.float64))
    ops.pso_quantize(torch.zeros(B, C, T), table, torch.zeros(B, dtype=torch.float64), 3)
    assert rec == [
        ("sfm_pso_frame_coef", "pso_prepare", 0.0, 4.0 * B * C * T + 16.0 * B * T, "coef B2 C64 T50"),
        ("sfm_pso_split", "pso_prepare", 8.0 * B * Lmax, 20.0 * B * Lmax + 16.0 * B * T, "split B2 L4000"),
        ("sfm_pso_fitness", "pso_fitness", 16.0 * B * NF * F * N, 24.0 * B * NF * F + 8.0 * B * 5 * N, "B2 N8 F103"),
        ("sfm_pso_step", "pso_step", 12.0 * B * N, 8.0 * B * N * 15, "B2 N8"),
        ("sfm_pso_step", "pso_step", 12.0 * B * N, 8.0 * B * N * 10, "B2 N8"),
        ("sfm_pso_quantize", "mask_quantize", 0.0, 8.0 * B * C * T, None),
    ]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.pso_step(state, 0)                                          # neither partials nor fitness
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.pso_fitness(spectra, i32(B + 1), i32(B), S, state.pos.float(), state.stopped, partial, B * NF)
