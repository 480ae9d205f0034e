"""The PSO search of OPT-PCIRM's middle step on the MI355X (csrc/pso.hip through optimizer.ParticleSwarmOptimizer and
masks.compute_opt_pcirm) against the float64 restatements of tests/pso_cases.py and what the reference itself did
(tests/golden/g18_pso.npz).

  1. fitness: 82 positions per case within pso_cases.TOL = 1.25e-7 of the restatement (the bound is derived there: the smallest
     margin of any decision of the reference's searches, asserted >= 1e-6 by the generator, divided by 8); an utterance gets
     the same bits alone and in a padded batch, and from run to run.
  2. recurrences: on a quadratic written as a product in float64 torch ops the whole history is the reference's, bit for bit.
  3. search: with the reference's draws the swarm takes the reference's decisions: gbest positions and the returned middle
     value to 1e-12, gbest fitness within TOL, the mask bitwise quantize_pcirm(pcirm, steps, middle); a host float64 replica fed
     the device's own fitness values reproduces the device's positions bit for bit.
  4. edges: no STOI frame, M = 2, M = 5, a ragged batch with explicit draws against three single calls.
Every fitness row prints `ROW | name | bound | observed`; profiles/README.md keeps the table."""
import os

import numpy as np
import pytest
import torch

import pso_cases as pc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_restated = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g18_pso.npz"))


@pytest.fixture(scope="module")
def masks():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd import masks
    return masks


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def restated(name, xs, num_steps=3):
    """the float64 fitness of case `name` at xs, computed once per (case, positions) and shared"""
    key = (name, num_steps, np.asarray(xs, dtype=np.float64).tobytes())
    if key not in _restated:
        _restated[key] = pc.fitness_of(name, xs, num_steps)
    return _restated[key]


def still_draws(xs, max_iter=1):
    """draws of a swarm that stands still at xs: zero velocities, r1 = r2 = 0"""
    xs = np.asarray(xs, dtype=np.float64)
    return np.concatenate([xs, np.zeros(xs.size), np.zeros(2 * xs.size * max_iter)])


def search(masks, name, cfg, num_steps=None):
    c = pc.burst_case(name)
    cfg = dict(cfg, history=True)
    return masks.compute_opt_pcirm(torch.tensor(c["pcirm"]).cuda(), c["noisy"].copy(), c["clean"].copy(), fs=c["fs"], num_steps=num_steps,
                                   pso_config=cfg)


def padded(names):
    cs = [pc.burst_case(n) for n in names]
    L = [c["noisy"].size for c in cs]
    C, T = cs[0]["pcirm"].shape[0], max(c["pcirm"].shape[1] for c in cs)
    pcirm, noisy, clean = np.zeros((len(cs), C, T), np.float32), np.zeros((len(cs), max(L)), np.float32), np.zeros((len(cs), max(L)), np.float32)
    for i, c in enumerate(cs):
        pcirm[i, :, :c["pcirm"].shape[1]] = c["pcirm"]
        noisy[i, :L[i]], clean[i, :L[i]] = c["noisy"], c["clean"]
    return torch.from_numpy(pcirm).cuda(), torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda(), L


# ---- 1. fitness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d", "e", "f", "g"])
def test_fitness_against_the_restatement(masks, name):
    xs = pc.probe_positions(pc.INPUTS[name][0])
    cfg = {"num_particles": xs.size, "max_iter": 1, "draws": still_draws(xs)}
    _, _, _, rec = search(masks, name, cfg)
    got, ref = rec["fitness"][0], restated(name, xs)
    assert same_bits(rec["positions"][0], xs)
    err = float(np.abs(got - ref).max())
    print("ROW | fitness %s C%d L%d fs%d, 82 positions | %.3g | %.3g" % ((name,) + pc.INPUTS[name][1:3] + (pc.INPUTS[name][4], pc.TOL, err)))
    assert ref.max() - ref.min() > 1e-2
    assert err <= pc.TOL, (err, int(np.abs(got - ref).argmax()))
    again = search(masks, name, cfg)[3]
    assert same_bits(again["fitness"], rec["fitness"]) and same_bits(again["mean_fitness"], rec["mean_fitness"])    # run to run


def test_fitness_of_an_utterance_is_the_same_bits_alone_and_in_a_padded_batch(masks):
    names = ["a", "b", "c"]
    xs = pc.probe_positions(9)
    pcirm, noisy, clean, L = padded(names)
    cfg = {"num_particles": xs.size, "max_iter": 1, "draws": np.stack([still_draws(xs)] * 3), "lengths": L, "history": True}
    _, _, middle, recs = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config=cfg)
    assert middle.shape == (3,) and middle.dtype == torch.float64 and middle.is_cuda
    for i, n in enumerate(names):
        _, _, mid, rec = search(masks, n, {"num_particles": xs.size, "max_iter": 1, "draws": still_draws(xs)})
        assert same_bits(recs[i]["fitness"], rec["fitness"]), n
        assert same_bits(float(middle[i]), mid), n
        err = float(np.abs(rec["fitness"][0] - restated(n, xs)).max())
        print("ROW | fitness %s in a padded batch of 3 | %.3g | %.3g" % (n, pc.TOL, err))
        assert err <= pc.TOL


# ---- 2. recurrences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.RECURRENCES))
def test_recurrences_are_the_reference_ones_bit_for_bit(golden, name):
    from sincformer_metacog_speech_enhancement_amd.optimizer import ParticleSwarmOptimizer
    t, maximize, w, c1, c2, K, seed = pc.RECURRENCES[name]
    seen = []

    def f(x):
        assert x.is_cuda and x.dtype == torch.float64 and x.shape == (pc.REC_N,)
        seen.append(1)
        return -((x - t) * (x - t)) if maximize else (x - t) * (x - t)
    pso = ParticleSwarmOptimizer(f, num_particles=pc.REC_N, max_iter=K, w=w, c1=c1, c2=c2, bounds=pc.BOUNDS, maximize=maximize,
                                 draws=golden[name + ".draws"])
    best, best_fit = pso.optimize()
    h = pso.get_convergence_history()
    n = int(golden[name + ".iterations_run"])
    assert pso.iterations_run == n and len(seen) == K + 1 and (n < K) == (name == "early")
    for k in ("gbest_fitness", "gbest_position", "mean_fitness", "positions", "fitness"):
        assert same_bits(h[k], golden[name + "." + k]), k
    assert same_bits(best, golden[name + ".best"]) and same_bits(best_fit, golden[name + ".gbest_fitness"][-1])


def test_the_optimizer_draws_from_the_global_stream_when_no_draws_are_given(golden):
    from sincformer_metacog_speech_enhancement_amd.optimizer import ParticleSwarmOptimizer
    t, maximize, w, c1, c2, K, seed = pc.RECURRENCES["inner"]
    np.random.seed(seed)
    pso = ParticleSwarmOptimizer(lambda x: -((x - t) * (x - t)), num_particles=pc.REC_N, max_iter=K)
    best, _ = pso.optimize()
    assert same_bits(best, golden["inner.best"]) and same_bits(pso.history["mean_fitness"], golden["inner.mean_fitness"])


# ---- 3. the search against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.TRAJECTORIES))
def test_search_takes_the_decisions_of_the_reference(masks, golden, name):
    inp, N, K, seed = pc.TRAJECTORIES[name]
    c = pc.burst_case(inp)
    draws = golden[name + ".draws"]
    mask, steps, middle, rec = search(masks, inp, {"num_particles": N, "max_iter": K, "draws": draws})
    assert isinstance(middle, float) and not mask.requires_grad and mask.shape == c["pcirm"].shape and mask.dtype == torch.float32
    calls = golden[name + ".calls"]
    rounds = len(calls) // N
    assert rec["iterations_run"] == rounds - 1 and rec["positions"].shape == (rounds, N)
    ferr = float(np.abs(rec["fitness"].reshape(-1) - calls[:, 1]).max())
    gerr = float(np.abs(np.asarray(rec["gbest_fitness"]) - golden[name + ".gbest_fitness"]).max())
    perr = float(np.abs(np.asarray(rec["gbest_position"]) - golden[name + ".gbest_position"]).max())
    print("ROW | search %s: per-particle fitness vs the reference's %d calls | %.3g | %.3g" % (name, len(calls), pc.TOL, ferr))
    print("ROW | search %s: gbest fitness | %.3g | %.3g" % (name, pc.TOL, gerr))
    print("ROW | search %s: gbest position | 1e-12 | %.3g" % (name, perr))
    assert perr <= 1e-12 and abs(middle - float(golden[name + ".middle"])) <= 1e-12
    assert np.abs(rec["positions"].reshape(-1) - calls[:, 0]).max() <= 1e-12
    assert gerr <= pc.TOL and ferr <= pc.TOL
    assert float(np.abs(np.asarray(rec["mean_fitness"]) - golden[name + ".mean_fitness"]).max()) <= pc.TOL
    assert same_bits(steps, pc.snr_boundaries(3))
    assert torch.equal(mask, masks.quantize_pcirm(torch.tensor(c["pcirm"]).cuda(), steps, middle))
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(c["pcirm"], steps, middle))
    # a host float64 replica fed the device's own fitness values reproduces the device's swarm bit for bit
    rep = pc.pso(lambda x, it: rec["fitness"][it], draws, N, K)
    assert rep["iterations_run"] == rec["iterations_run"]
    for k in ("positions", "gbest_position", "gbest_fitness", "mean_fitness"):
        assert same_bits(rep[k], rec[k]), k
    assert same_bits(rep["best_position"], middle)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------
def test_a_signal_without_a_stoi_frame_scores_zero(masks):
    draws = pc.draws_after_seed(31, 6, 4)
    mask, steps, middle, rec = search(masks, "short", {"num_particles": 6, "max_iter": 4, "draws": draws})
    assert not rec["fitness"].any() and not np.asarray(rec["gbest_fitness"]).any() and rec["fitness"].shape == (5, 6)
    assert same_bits(middle, draws[0])                                    # nothing beats particle 0's first position
    rep = pc.pso(lambda x, it: np.zeros(6), draws, 6, 4)
    assert same_bits(rep["positions"], rec["positions"])
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(pc.burst_case("short")["pcirm"], steps, middle))


def test_two_steps_leave_the_middle_value_unused(masks):
    draws = pc.draws_after_seed(32, 6, 4)
    mask, steps, middle, rec = search(masks, "c", {"num_particles": 6, "max_iter": 4, "draws": draws}, num_steps=2)
    assert len(steps) == 2 and same_bits(steps, pc.snr_boundaries(2))
    assert np.unique(rec["fitness"].view(np.int64)).size == 1             # constant, to the bit
    err = abs(float(rec["fitness"][0, 0]) - float(restated("c", [0.5], 2)[0]))
    print("ROW | fitness c with M = 2 | %.3g | %.3g" % (pc.TOL, err))
    assert err <= pc.TOL and same_bits(middle, draws[0])
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(pc.burst_case("c")["pcirm"], steps, middle))


def test_five_steps(masks):
    draws = pc.draws_after_seed(33, 6, 4)
    mask, steps, middle, rec = search(masks, "c", {"num_particles": 6, "max_iter": 4, "draws": draws}, num_steps=5)
    ref = restated("c", rec["positions"].reshape(-1), 5)
    err = float(np.abs(rec["fitness"].reshape(-1) - ref).max())
    print("ROW | fitness c with M = 5, %d positions | %.3g | %.3g" % (ref.size, pc.TOL, err))
    assert err <= pc.TOL and ref.max() - ref.min() > 1e-4                 # the middle value is in use
    rep = pc.pso(lambda x, it: rec["fitness"][it], draws, 6, 4)
    assert same_bits(rep["positions"], rec["positions"]) and same_bits(rep["best_position"], middle)
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(pc.burst_case("c")["pcirm"], steps, middle))


def test_a_ragged_batch_is_three_single_calls_bit_for_bit(masks):
    names = ["a", "b", "c"]
    N, K = 6, 5
    draws = np.stack([pc.draws_after_seed(41 + i, N, K) for i in range(3)])
    pcirm, noisy, clean, L = padded(names)
    mask, steps, middle, recs = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config={
        "num_particles": N, "max_iter": K, "draws": draws, "lengths": torch.tensor(L), "history": True})
    middle = middle.cpu().numpy()
    for i, n in enumerate(names):
        m1, _, mid, rec = search(masks, n, {"num_particles": N, "max_iter": K, "draws": draws[i]})
        assert same_bits(middle[i], mid) and recs[i]["iterations_run"] == rec["iterations_run"], n
        for k in ("positions", "fitness", "gbest_position", "gbest_fitness", "mean_fitness"):
            assert same_bits(recs[i][k], rec[k]), (n, k)
        T = m1.shape[1]
        assert torch.equal(mask[i, :, :T], m1) and not mask[i, :, T:].any()
    # the default draws come from np.random's global stream, one pso_draws per utterance in batch order
    np.random.seed(77)
    _, _, mid2 = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config={"num_particles": N, "max_iter": K, "lengths": L})
    np.random.seed(77)
    from sincformer_metacog_speech_enhancement_amd.optimizer import pso_draws
    d = np.stack([pso_draws(N, K) for _ in range(3)])
    _, _, mid3 = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config={"num_particles": N, "max_iter": K, "lengths": L,
                                                                                   "draws": d})
    assert torch.equal(mid2, mid3)
