"""Mirror of optimizer/pso.py: the particle swarm of Eq. 12-13 for one scalar x in [lb, ub], its recurrences on the device
(csrc/pso.hip, sfm_pso_step) in float64, bit for bit as the reference's numpy loop computes them.

Within one iteration the reference's particles do not see each other: gbest changes only after the inner loop.  An iteration is
therefore N independent updates and one fold, and the random numbers r1, r2, drawn particle by particle there, can be drawn
beforehand in the same order (pso_draws).  Two stated differences:
  * `fitness_fn` receives ALL N positions as a float64 device tensor [N] and returns N values, once per iteration (a scalar
    Python callback per particle would serialise the device);
  * early stopping is decided on the device, so the host never learns inside the loop that a swarm has stopped: pso_draws always
    consumes 2 N + 2 N max_iter numbers of np.random's global stream, where the reference consumes fewer when it stops early.
    Up to the point of stopping the numbers are the same ones."""
import numpy as np
import torch

from .. import config


def pso_draws(num_particles=None, max_iter=None, bounds=None):
    """float64 [2 N + 2 N max_iter] from np.random's GLOBAL state in the order optimizer/pso.py consumes it: uniform(lb, ub, N)
    (:86), uniform(-0.1 (ub - lb), 0.1 (ub - lb), N) (:89-90), then random() twice per particle and iteration (:116-117).
    np.random.seed(s) before the call gives the reference's stream after the same seed."""
    N = num_particles or config.PSO_NUM_PARTICLES
    K = max_iter or config.PSO_MAX_ITER
    lb, ub = bounds or config.PSO_BOUNDS
    check_swarm(N, K, (lb, ub))
    positions = np.random.uniform(lb, ub, N)
    v_range = (ub - lb) * 0.1
    velocities = np.random.uniform(-v_range, v_range, N)
    r = np.random.random((K, N, 2))
    return np.concatenate([positions, velocities, r.reshape(-1)])


def check_swarm(N, max_iter, bounds):
    """the limits of sfm_pso_step, raised on the host before anything is launched"""
    from .. import ops
    if int(N) != N or not 1 <= N <= ops.PSO_MAX_PARTICLES:
        raise ValueError("PSO: %r particles; the kernel takes 1..%d" % (N, ops.PSO_MAX_PARTICLES))
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("PSO: max_iter %r; at least one iteration is needed" % (max_iter,))
    lb, ub = bounds
    if not (np.isfinite(lb) and np.isfinite(ub) and lb < ub):
        raise ValueError("PSO: bounds %r; lb < ub is needed" % (bounds,))


class SwarmState:
    """B swarms of N particles on the device: what sfm_pso_step reads and writes.  draws: float64 [B, 2 N + 2 N max_iter] (host
    or device)."""

    def __init__(self, draws, num_particles, max_iter, w, c1, c2, bounds, maximize=True, device="cuda"):
        check_swarm(num_particles, max_iter, bounds)
        N, K = int(num_particles), int(max_iter)
        d = torch.as_tensor(draws, dtype=torch.float64)
        if d.dim() == 1:
            d = d.unsqueeze(0)
        if d.dim() != 2 or d.shape[1] != 2 * N + 2 * N * K:
            raise ValueError("PSO: draws %s; [B, 2 N + 2 N max_iter] = [B, %d] is needed" % (tuple(d.shape), 2 * N + 2 * N * K))
        self.B, self.N, self.max_iter, self.maximize = int(d.shape[0]), N, K, bool(maximize)
        host = np.asarray([w, c1, c2, bounds[0], bounds[1]], dtype=np.float64)
        self.draws = d.to(device).contiguous()
        dev = self.draws.device
        self.params = torch.from_numpy(host).to(dev)
        self.pos = self.draws[:, :N].contiguous()
        self.vel = self.draws[:, N:2 * N].contiguous()
        self.pbest_pos = torch.empty_like(self.pos)
        self.pbest_fit = torch.empty_like(self.pos)
        self.gbest = torch.zeros(self.B, 2, device=dev, dtype=torch.float64)
        self.hist = torch.zeros(self.B, K + 1, 3 + 2 * N, device=dev, dtype=torch.float64)
        self.iters = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.stopped = torch.zeros(self.B, device=dev, dtype=torch.int32)

    def fetch(self):
        """ONE copy to the host -> per swarm a dict: the reference's three history lists, cut where the swarm stopped, the
        per-particle 'positions' / 'fitness' [rounds, N], 'iterations_run', 'stopped', 'best_position', 'best_fitness'"""
        B, N, K = self.B, self.N, self.max_iter
        flat = torch.cat([self.hist.reshape(-1), self.gbest.reshape(-1), self.iters.double(), self.stopped.double()]).cpu().numpy()
        n = B * (K + 1) * (3 + 2 * N)
        hist, gbest = flat[:n].reshape(B, K + 1, 3 + 2 * N), flat[n:n + 2 * B].reshape(B, 2)
        iters, stopped = flat[n + 2 * B:n + 3 * B].astype(np.int64), flat[n + 3 * B:].astype(np.int64)
        out = []
        for b in range(B):
            h = hist[b, :iters[b] + 1]
            out.append({"gbest_fitness": h[:, 0].tolist(), "gbest_position": h[:, 1].tolist(), "mean_fitness": h[:, 2].tolist(),
                        "positions": h[:, 3:3 + N].copy(), "fitness": h[:, 3 + N:].copy(), "iterations_run": int(iters[b]),
                        "stopped": bool(stopped[b]), "best_position": float(gbest[b, 0]), "best_fitness": float(gbest[b, 1])})
        return out


class ParticleSwarmOptimizer:
    """optimizer/pso.py:26-189 with the reference's constructor, defaults and history keys.

        pso = ParticleSwarmOptimizer(lambda x: -(x - 0.3) * (x - 0.3))      # x: float64 device tensor [N]
        best_value, best_fitness = pso.optimize()

    draws: float64 [2 N + 2 N max_iter] instead of a call of pso_draws (which consumes np.random's global stream)."""

    def __init__(self, fitness_fn, num_particles=None, max_iter=None, w=None, c1=None, c2=None, bounds=None, maximize=True,
                 verbose=False, draws=None):
        self.fitness_fn = fitness_fn
        self.N = num_particles or config.PSO_NUM_PARTICLES
        self.max_iter = max_iter or config.PSO_MAX_ITER
        self.w = w if w is not None else config.PSO_W
        self.c1 = c1 if c1 is not None else config.PSO_C1
        self.c2 = c2 if c2 is not None else config.PSO_C2
        self.lb, self.ub = bounds or config.PSO_BOUNDS
        self.maximize = maximize
        self.verbose = verbose
        self.draws = draws
        check_swarm(self.N, self.max_iter, (self.lb, self.ub))
        self.iterations_run = 0
        self.history = {"gbest_fitness": [], "gbest_position": [], "mean_fitness": []}

    def optimize(self):
        """-> (best_position, best_fitness) as Python floats.  max_iter + 1 rounds of fitness_fn + one launch, then one copy."""
        from .. import ops
        if not torch.cuda.is_available():
            raise RuntimeError("ParticleSwarmOptimizer: the swarm runs on an MI355X (no CPU fallback)")
        draws = pso_draws(self.N, self.max_iter, (self.lb, self.ub)) if self.draws is None else self.draws
        state = SwarmState(draws, self.N, self.max_iter, self.w, self.c1, self.c2, (self.lb, self.ub), self.maximize)
        if state.B != 1:
            raise ValueError("ParticleSwarmOptimizer: one swarm; draws describe %d" % state.B)
        for it in range(self.max_iter + 1):
            fit = torch.as_tensor(self.fitness_fn(state.pos[0]), dtype=torch.float64, device=state.pos.device)
            if fit.numel() != self.N:
                raise ValueError("fitness_fn returned %d values for %d positions" % (fit.numel(), self.N))
            ops.pso_step(state, it, fitness=fit.detach().reshape(1, self.N).contiguous())
        rec = state.fetch()[0]
        for k in ("gbest_fitness", "gbest_position", "mean_fitness", "positions", "fitness"):
            self.history[k] = rec[k]
        self.iterations_run = rec["iterations_run"]
        if self.verbose:
            for i in range(10, self.iterations_run + 1, 10):
                print(f"  PSO iter {i}/{self.max_iter}: gbest={rec['gbest_position'][i]:.4f}, fitness={rec['gbest_fitness'][i]:.4f}")
            if rec["stopped"]:
                print(f"  PSO converged at iteration {self.iterations_run}")
        return rec["best_position"], rec["best_fitness"]

    def get_convergence_history(self):
        """the optimisation history: 'gbest_fitness', 'gbest_position', 'mean_fitness' lists (one entry per round, as the
        reference), and the per-particle 'positions' / 'fitness' arrays"""
        return self.history
