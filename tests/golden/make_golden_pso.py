"""Generator of tests/golden/g18_pso.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), like the
other generators, on the CPU: imports the reference's masks/opt_pcirm.py and optimizer/pso.py - never shipped, never copied -
and stores what they do on the seeded cases of tests/pso_cases.py.

  <t>.draws                 what optimizer/pso.py drew after np.random.seed(seed), in its order (checked: the restated swarm fed
                            these draws and the recorded fitness values reproduces the reference's history bit for bit)
  <t>.calls                 [n, 2]: every call (x, value) of the reference's fitness function, in call order
  <t>.gbest_fitness / .gbest_position / .mean_fitness
                            the reference's history lists
  <t>.middle                the optimized_middle compute_opt_pcirm returned
  <t>.margins               the smallest margin of the decisions of each round (pso_cases.pso)
  <r>.draws / .gbest_fitness / .gbest_position / .mean_fitness / .positions / .fitness / .best / .iterations_run
                            the recurrence cases: ParticleSwarmOptimizer alone on a quadratic

CONDITION, asserted here: every margin of the trajectory cases is >= pso_cases.MARGIN (a case that fails needs another seed).

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pso.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_pso: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import pso_cases as pc  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def main():
    import masks.opt_pcirm as ref_opt
    from optimizer.pso import ParticleSwarmOptimizer
    out = {}
    made = []

    class Recording(ParticleSwarmOptimizer):
        def __init__(self, fitness_fn, **kw):
            self.calls = []

            def logged(x):
                v = fitness_fn(x)
                self.calls.append((float(x), float(v)))
                return v
            super().__init__(logged, **kw)
            made.append(self)

    ref_opt.ParticleSwarmOptimizer = Recording
    for name, (inp, N, K, seed) in pc.TRAJECTORIES.items():
        c = pc.burst_case(inp)
        np.random.seed(seed)
        mask, steps, middle = ref_opt.compute_opt_pcirm(c["pcirm"], c["noisy"], c["clean"], fs=c["fs"],
                                                        pso_config={"num_particles": N, "max_iter": K})
        pso = made.pop()
        calls = np.asarray(pso.calls, dtype=np.float64)
        draws = pc.draws_after_seed(seed, N, K)
        rounds = calls[:, 1].reshape(-1, N)
        rep = pc.pso(lambda x, it: rounds[it], draws, N, K)
        hist = pso.get_convergence_history()
        assert same_bits(rep["positions"].reshape(-1), calls[:, 0]), name
        for k in ("gbest_fitness", "gbest_position", "mean_fitness"):
            assert same_bits(rep[k], hist[k]), (name, k)
        assert same_bits(rep["best_position"], middle) and np.array_equal(mask, pc.quantize(c["pcirm"], steps, middle))
        assert same_bits(steps, pc.snr_boundaries(3))
        restated = pc.fitness_of(inp, calls[:, 0])
        print("%s: %d calls, %d iterations, middle %.6f, fitness %.4f..%.4f, smallest margin %.2e, restatement off by %.2e" % (
            name, len(calls), rep["iterations_run"], middle, calls[:, 1].min(), calls[:, 1].max(), rep["margins"].min(),
            np.abs(restated - calls[:, 1]).max()))
        assert rep["margins"].min() >= pc.MARGIN, "%s: a decision with margin %.2e: take another seed" % (name, rep["margins"].min())
        out.update({name + ".draws": draws, name + ".calls": calls, name + ".middle": np.float64(middle),
                    name + ".margins": rep["margins"]})
        out.update({name + "." + k: np.asarray(hist[k], dtype=np.float64) for k in ("gbest_fitness", "gbest_position", "mean_fitness")})
    for name, (t, maximize, w, c1, c2, K, seed) in pc.RECURRENCES.items():
        f = pc.quadratic(t, maximize)
        np.random.seed(seed)
        pso = ParticleSwarmOptimizer(f, num_particles=pc.REC_N, max_iter=K, w=w, c1=c1, c2=c2, bounds=pc.BOUNDS, maximize=maximize)
        best, best_fit = pso.optimize()
        draws = pc.draws_after_seed(seed, pc.REC_N, K)
        rep = pc.pso(lambda x, it: f(x), draws, pc.REC_N, K, w, c1, c2, pc.BOUNDS, maximize)
        hist = pso.get_convergence_history()
        for k in ("gbest_fitness", "gbest_position", "mean_fitness"):
            assert same_bits(rep[k], hist[k]), (name, k)
        assert same_bits(rep["best_position"], best) and same_bits(rep["best_fitness"], best_fit)
        pos = rep["positions"]
        print("%s: %d iterations of %d, best %.6f, positions at lb %d / at ub %d" % (
            name, rep["iterations_run"], K, best, int((pos == pc.BOUNDS[0]).sum()), int((pos == pc.BOUNDS[1]).sum())))
        out.update({name + ".draws": draws, name + ".best": np.float64(best), name + ".iterations_run": np.int64(rep["iterations_run"]),
                    name + ".positions": pos, name + ".fitness": rep["fitness"]})
        out.update({name + "." + k: np.asarray(hist[k], dtype=np.float64) for k in ("gbest_fitness", "gbest_position", "mean_fitness")})
    assert out["upper.positions"].max() == pc.BOUNDS[1] and out["lower.positions"].min() == pc.BOUNDS[0]
    assert out["early.iterations_run"] < pc.RECURRENCES["early"][5]
    path = os.path.join(HERE, "g18_pso.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
