"""The OPT-PCIRM search on the STOI / ESTOI of Taal et al. on the MI355X (masks.compute_opt_pcirm with pso_config["fitness"];
csrc/stoi.hip: sfm_stoi_bands_pair, sfm_pso_fitness_taal) against the float64 planes route of tests/pso_taal_cases.py.

  1. fitness: the 82 probe positions of every input, both measures, within 16 x e32 (the float32-operand evaluation's own error,
     derived in pso_taal_cases, never from a kernel); the 29-frame input scores 1e-5 exactly; the same bits from run to run.
  2. the fitness is the measure: against evaluation.compute_stoi_taal of the materialised float32 enhanced signal.
  3. an utterance gets the same bits alone, in a padded batch and in a ragged search.
  4. search: the swarm takes the decisions of the float64 search (every one of which has twice the bound as margin).
  5. interface: the default and "fallback" are one path, the guards, M = 2 and M = 5.
Every row prints `ROW | name | bound | observed`; profiles/README.md keeps the table."""
import numpy as np
import pytest
import torch

import pso_cases as pc
import pso_taal_cases as tc
import stoi_taal_cases as stc

pytestmark = pytest.mark.gpu
KEY = {False: "stoi_taal", True: "estoi"}


@pytest.fixture(scope="module")
def masks():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd import masks
    return masks


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def still_draws(xs, max_iter=1):
    """draws of a swarm that stands still at xs: zero velocities, r1 = r2 = 0"""
    xs = np.asarray(xs, dtype=np.float64)
    return np.concatenate([xs, np.zeros(xs.size), np.zeros(2 * xs.size * max_iter)])


def search(masks, c, cfg, ext, num_steps=None):
    cfg = dict(cfg, history=True, fitness=KEY[ext])
    return masks.compute_opt_pcirm(torch.tensor(c["pcirm"]).cuda(), c["noisy"].copy(), c["clean"].copy(), fs=c["fs"], num_steps=num_steps,
                                   pso_config=cfg)


def still(masks, name, xs, ext, num_steps=None):
    """the device's fitness of input `name` at xs: one round of a swarm that stands there"""
    rec = search(masks, tc.case(name), {"num_particles": len(xs), "max_iter": 1, "draws": still_draws(xs)}, ext, num_steps)[3]
    assert same_bits(rec["positions"][0], xs)
    return rec


def padded(names):
    cs = [tc.case(n) for n in names]
    L = [c["noisy"].size for c in cs]
    C, T = cs[0]["pcirm"].shape[0], max(c["pcirm"].shape[1] for c in cs)
    pcirm, noisy, clean = np.zeros((len(cs), C, T), np.float32), np.zeros((len(cs), max(L)), np.float32), np.zeros((len(cs), max(L)), np.float32)
    for i, c in enumerate(cs):
        pcirm[i, :, :c["pcirm"].shape[1]] = c["pcirm"]
        noisy[i, :L[i]], clean[i, :L[i]] = c["noisy"], c["clean"]
    return torch.from_numpy(pcirm).cuda(), torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda(), L


# ---- 1. fitness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", tc.MEASURES)
@pytest.mark.parametrize("name", tc.SCORED)
def test_fitness_against_the_restatement(masks, name, ext):
    row = tc.evaluated()[(name, ext)]
    rec = still(masks, name, row["xs"], ext)
    tc.check("fitness %s %s C%d L%d fs%d, 82 positions" % ((KEY[ext], name) + tc.INPUTS[name][1:3] + (tc.INPUTS[name][4],)),
             rec["fitness"][0], row["ref"], row["bound"])
    again = still(masks, name, row["xs"], ext)
    assert same_bits(again["fitness"], rec["fitness"]) and same_bits(again["mean_fitness"], rec["mean_fitness"])    # run to run


@pytest.mark.parametrize("ext", tc.MEASURES)
def test_below_thirty_spectral_frames_every_particle_scores_the_constant(masks, ext):
    row = tc.evaluated()[("F", ext)]
    rec = still(masks, "F", row["xs"], ext)
    print("ROW | fitness %s F: 29 spectral frames, 82 positions | 0 | %.3g" % (KEY[ext], float(np.abs(rec["fitness"] - 1e-5).max())))
    assert np.all(rec["fitness"] == 1e-5) and np.all(row["ref"] == 1e-5) and rec["fitness"].shape == (2, 82)
    draws = pc.draws_after_seed(31, 6, 4)
    mask, steps, middle, rec = search(masks, tc.case("F"), {"num_particles": 6, "max_iter": 4, "draws": draws}, ext)
    assert np.all(rec["fitness"] == 1e-5) and same_bits(middle, draws[0])       # nothing beats particle 0's first position
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(tc.case("F")["pcirm"], steps, middle))


# ---- 2. the fitness is the measure ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", tc.MEASURES)
@pytest.mark.parametrize("name", ["A", "C"])
def test_fitness_is_the_measure_of_the_materialised_signal(masks, name, ext):
    from sincformer_metacog_speech_enhancement_amd.evaluation.stoi_taal import compute_stoi_taal
    c = tc.case(name)
    xs = np.array([0.0, 0.013, 0.3, 1.0])
    got = still(masks, name, xs, ext)["fitness"][0]
    for x, g in zip(xs, got):
        e = tc.enhanced(name, float(x))
        own = abs(stc.stoi64(c["clean"], e, c["fs"], ext, np.float32) - stc.stoi64(c["clean"], e, c["fs"], ext, np.float64))
        bound = tc.evaluated()[(name, ext)]["bound"] + stc.K * own
        measure = compute_stoi_taal(c["clean"].copy(), e, c["fs"], extended=ext)
        tc.check("fitness %s %s at x = %g vs compute_stoi_taal(clean, float32(ya + x yb))" % (KEY[ext], name, x), g, measure, bound)


# ---- 3. alone, padded, ragged ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", tc.MEASURES)
def test_an_utterance_has_the_same_bits_alone_padded_and_ragged(masks, ext):
    names = ["A", "B", "E"]
    xs = pc.probe_positions(9)
    pcirm, noisy, clean, L = padded(names)
    N, K = 6, 5
    moving = np.stack([pc.draws_after_seed(41 + i, N, K) for i in range(3)])
    cfg = {"num_particles": xs.size, "max_iter": 1, "draws": np.stack([still_draws(xs)] * 3), "lengths": L, "history": True, "fitness": KEY[ext]}
    _, _, middle, recs = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config=cfg)
    mask, _, middle2, recs2 = masks.compute_opt_pcirm(pcirm, noisy, clean, fs=8000, pso_config={
        "num_particles": N, "max_iter": K, "draws": moving, "lengths": torch.tensor(L), "history": True, "fitness": KEY[ext]})
    assert middle.shape == (3,) and middle.dtype == torch.float64 and middle.is_cuda
    for i, n in enumerate(names):
        rec = still(masks, n, xs, ext)
        assert same_bits(recs[i]["fitness"], rec["fitness"]), n
        assert same_bits(float(middle[i]), rec["best_position"]), n
        ref, e32 = tc.bound_at(n, xs, ext)
        tc.check("fitness %s %s in a padded batch of 3" % (KEY[ext], n), recs[i]["fitness"][0], ref, tc.K * float(e32.max()))
        m1, _, mid, rec = search(masks, tc.case(n), {"num_particles": N, "max_iter": K, "draws": moving[i]}, ext)
        assert same_bits(float(middle2[i]), mid) and recs2[i]["iterations_run"] == rec["iterations_run"], n
        for k in ("positions", "fitness", "gbest_position", "gbest_fitness", "mean_fitness"):
            assert same_bits(recs2[i][k], rec[k]), (n, k)
        T = m1.shape[1]
        assert torch.equal(mask[i, :, :T], m1) and not mask[i, :, T:].any()


# ---- 4. search -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.TRAJECTORIES))
def test_search_takes_the_decisions_of_the_float64_search(masks, name):
    inp, N, K, seed, ext = tc.TRAJECTORIES[name]
    t = tc.trajectory(name)
    H, c = t["H"], tc.case(inp)
    mask, steps, middle, rec = search(masks, c, {"num_particles": N, "max_iter": K, "draws": t["draws"]}, ext)
    assert isinstance(middle, float) and mask.shape == c["pcirm"].shape and mask.dtype == torch.float32
    assert rec["iterations_run"] == H["iterations_run"] and rec["positions"].shape == H["positions"].shape
    perr = float(np.abs(np.asarray(rec["gbest_position"]) - H["gbest_position"]).max())
    print("ROW | search %s: gbest position | 1e-12 | %.3g" % (name, perr))
    assert perr <= 1e-12 and abs(middle - H["best_position"]) <= 1e-12
    assert np.abs(rec["positions"] - H["positions"]).max() <= 1e-12
    tc.check("search %s: gbest fitness" % name, rec["gbest_fitness"], H["gbest_fitness"], t["bound"])
    tc.check("search %s: per-particle fitness, %d evaluations" % (name, H["fitness"].size), rec["fitness"], H["fitness"], t["bound"])
    assert same_bits(steps, pc.snr_boundaries(3))
    assert torch.equal(mask, masks.quantize_pcirm(torch.tensor(c["pcirm"]).cuda(), steps, middle))
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(c["pcirm"], steps, middle))
    # a host float64 replica fed the device's own fitness values reproduces the device's swarm bit for bit
    rep = pc.pso(lambda x, it: rec["fitness"][it], t["draws"], N, K)
    for k in ("positions", "gbest_position", "gbest_fitness", "mean_fitness"):
        assert same_bits(rep[k], rec[k]), k
    assert same_bits(rep["best_position"], middle)


# ---- 5. interface --------------------------------------------------------------------------------------------------------------
def test_the_default_is_the_fallback_path_bit_for_bit(masks):
    c = pc.burst_case("a")
    cfg = {"num_particles": 8, "max_iter": 8, "draws": pc.draws_after_seed(1, 8, 8), "history": True}
    args = (torch.tensor(c["pcirm"]).cuda(), c["noisy"].copy(), c["clean"].copy())
    m0, s0, mid0, r0 = masks.compute_opt_pcirm(*args, fs=c["fs"], pso_config=cfg)
    m1, s1, mid1, r1 = masks.compute_opt_pcirm(*args, fs=c["fs"], pso_config=dict(cfg, fitness="fallback"))
    assert torch.equal(m0, m1) and same_bits(s0, s1) and same_bits(mid0, mid1)
    for k in ("positions", "fitness", "gbest_position", "gbest_fitness", "mean_fitness"):
        assert same_bits(r0[k], r1[k]), k
    err = float(np.abs(r1["fitness"].reshape(-1) - pc.fitness_of("a", r1["positions"].reshape(-1))).max())
    print("ROW | fitness: \"fallback\" on pso_cases a, %d evaluations | %.3g | %.3g" % (r1["fitness"].size, pc.TOL, err))
    assert err <= pc.TOL


def test_guards_raise_without_a_launch(masks, monkeypatch):
    from sincformer_metacog_speech_enhancement_amd import ops
    c = tc.case("E")
    args = (torch.tensor(c["pcirm"]).cuda(), c["noisy"].copy(), c["clean"].copy())

    def launched(*a, **k):
        raise AssertionError("a launch before the guard")
    monkeypatch.setattr(ops, "_call", launched)
    with pytest.raises(ValueError, match="fitness"):
        masks.compute_opt_pcirm(*args, fs=8000, pso_config={"fitness": "pesq"})
    for ext in tc.MEASURES:
        with pytest.raises(NotImplementedError, match="44100"):
            masks.compute_opt_pcirm(*args, fs=44100, pso_config={"fitness": KEY[ext]})
    with pytest.raises(AssertionError, match="a launch before the guard"):          # (the patch is in place: a valid call launches)
        masks.compute_opt_pcirm(*args, fs=8000, pso_config={"fitness": "estoi"})


@pytest.mark.parametrize("ext", tc.MEASURES)
def test_two_steps_leave_the_middle_value_unused(masks, ext):
    draws = pc.draws_after_seed(32, 6, 4)
    mask, steps, middle, rec = search(masks, tc.case("A"), {"num_particles": 6, "max_iter": 4, "draws": draws}, ext, num_steps=2)
    assert len(steps) == 2 and same_bits(steps, pc.snr_boundaries(2))
    assert np.unique(rec["fitness"].view(np.int64)).size == 1             # constant, to the bit
    ref, e32 = tc.bound_at("A", [0.5], ext, 2)
    tc.check("fitness %s A with M = 2" % KEY[ext], rec["fitness"][0, :1], ref, tc.K * float(e32.max()))
    assert same_bits(middle, draws[0])
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(tc.case("A")["pcirm"], steps, middle))


@pytest.mark.parametrize("ext", tc.MEASURES)
def test_five_steps(masks, ext):
    draws = pc.draws_after_seed(33, 6, 4)
    mask, steps, middle, rec = search(masks, tc.case("A"), {"num_particles": 6, "max_iter": 4, "draws": draws}, ext, num_steps=5)
    ref, e32 = tc.bound_at("A", rec["positions"].reshape(-1), ext, 5)
    tc.check("fitness %s A with M = 5, %d positions" % (KEY[ext], ref.size), rec["fitness"].reshape(-1), ref, tc.K * float(e32.max()))
    assert ref.max() - ref.min() > 1e-4                                   # the middle value is in use
    rep = pc.pso(lambda x, it: rec["fitness"][it], draws, 6, 4)
    assert same_bits(rep["positions"], rec["positions"]) and same_bits(rep["best_position"], middle)
    assert np.array_equal(mask.cpu().numpy(), pc.quantize(tc.case("A")["pcirm"], steps, middle))
