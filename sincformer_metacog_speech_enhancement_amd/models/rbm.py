"""Mirror of models/rbm.py (RBM :21-187, pretrain_dnn_with_rbm :190-223): the layer-wise CD-k pre-training of the DNN on
csrc/rbm.hip.  W [n_visible, n_hidden], v_bias and h_bias are fp32 tensors; one CD-k step is 2 + 2 k launches (up + sample, then
k x (down, up [+ sample]), then the update), the batch gather data[indices[start:end]] happens inside the launches that stage the
rows, and train() returns to the host once, at its end.

What the reference's step really uses of its 2 k + 1 draws: only HIDDEN samples ever feed anything.  neg_v_sample is never used
(the down pass's probabilities go up again) and the last h_sample of the Gibbs loop is never used, so only the first k hidden
draws decide anything.  Two sources of those decisions:
  counter (default, seed=)  S = 1 iff word(seed, m N + n) < ceil(prob 2^24), the 24-bit word of the dropout keep function
                            (include/sincformer_hip.h, sfm_rbm_prob), a fresh seed per draw site from one sequence (train._Seeds);
                            the unused draws are never generated; the epoch's permutation is torch.randperm on the device.
  replay (draws=)           S = prob > u with the float64 uniforms and the permutations np.random gives the reference
                            (rbm_draws consumes the stream exactly as the reference's train() does and drops the unused draws).
                            k B n_hidden doubles per step: for tests and small runs, refused beyond REPLAY_MAX_BYTES.
There is no CPU fallback: a host tensor is refused."""
import numpy as np
import torch

from .. import config

REPLAY_MAX_BYTES = 256 * 1024 * 1024     # of float64 uniforms one replayed train() may hold


def _steps(num_samples, batch_size):
    return (num_samples + batch_size - 1) // batch_size


def rbm_draws(num_samples, n_visible, n_hidden, epochs=None, batch_size=None, k_steps=None):
    """consumes np.random's GLOBAL stream exactly as RBM.train (:126-165) does after the constructor: per epoch one
    permutation(num_samples), per batch random((B, n_hidden)), then k x (random((B, n_visible)), random((B, n_hidden))).
    -> {"perms": int64 [epochs, num_samples], "u": [epochs * steps] float64 arrays [k, B, n_hidden]}: the uniforms that enter a
    decision (the first hidden draw and the hidden draws of all Gibbs iterations but the last); the others are drawn and dropped."""
    epochs = epochs or config.RBM_EPOCHS
    batch_size = batch_size or config.RBM_BATCH_SIZE
    k = k_steps or config.RBM_K_STEPS
    if min(num_samples, n_visible, n_hidden, epochs, batch_size, k) < 1:
        raise ValueError("rbm_draws: every size must be at least 1")
    total = 8 * epochs * num_samples * k * n_hidden
    if total > REPLAY_MAX_BYTES:
        raise ValueError("rbm_draws: %d bytes of uniforms; replay is for tests and small runs (at most %d)" % (total, REPLAY_MAX_BYTES))
    perms, us = [], []
    for _ in range(epochs):
        perms.append(np.random.permutation(num_samples))
        for start in range(0, num_samples, batch_size):
            B = min(start + batch_size, num_samples) - start
            u = np.empty((k, B, n_hidden), dtype=np.float64)
            u[0] = np.random.random((B, n_hidden))
            for g in range(k):
                np.random.random((B, n_visible))               # neg_v_sample: never used
                h = np.random.random((B, n_hidden))            # the last one: never used
                if g + 1 < k:
                    u[g + 1] = h
            us.append(u)
    return {"perms": np.stack(perms).astype(np.int64), "u": us}


class RBM:
    """models/rbm.py:21-187 under the reference's names and argument order.

        rbm = RBM(594, 1024)                    # draws W from np.random, as there
        errors = rbm.train(features)            # fp32 device tensor [N, 594]
        W, v_bias, h_bias = rbm.get_weights()

    seed: base of the counter mode's seed sequence (None: drawn from torch's host generator at the first draw).
    draws: what rbm_draws returned: train() replays it."""

    def __init__(self, n_visible, n_hidden, learning_rate=None, k_steps=None, *, seed=None, draws=None):
        from .. import ops
        if seed is not None and draws is not None:
            raise ValueError("RBM: seed (counter mode) or draws (replay mode), not both")
        for name, n in (("n_visible", n_visible), ("n_hidden", n_hidden)):
            if int(n) != n or not 1 <= n <= ops.RBM_MAX_UNITS:
                raise ValueError("RBM: %s %r; the kernels take 1..%d" % (name, n, ops.RBM_MAX_UNITS))
        self.n_visible = int(n_visible)
        self.n_hidden = int(n_hidden)
        self.lr = learning_rate or config.RBM_LEARNING_RATE
        self.k = k_steps or config.RBM_K_STEPS
        self.W = torch.from_numpy((np.random.randn(self.n_visible, self.n_hidden) * 0.01).astype(np.float32))
        self.v_bias = torch.zeros(self.n_visible, dtype=torch.float32)
        self.h_bias = torch.zeros(self.n_hidden, dtype=torch.float32)
        self.seed = seed
        self.draws = draws
        self._seeds = None

    # ---- plumbing ----
    def _on(self, t, width, what):
        """the state follows the first device tensor; a host tensor is refused like everywhere else"""
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
            raise ValueError("RBM.%s: an fp32 tensor [rows, %d] is needed; got %s" % (what, width, tuple(t.shape) if torch.is_tensor(t) else type(t)))
        if not t.is_cuda:
            raise RuntimeError("RBM.%s: the RBM only runs on an MI355X device tensor; got a CPU tensor (there is no CPU fallback)" % what)
        if self.W.device != t.device:
            self.W, self.v_bias, self.h_bias = (x.to(t.device) for x in (self.W, self.v_bias, self.h_bias))
        return t if t.stride(1) == 1 and t.stride(0) >= width else t.contiguous()

    def _next_seed(self):
        if self._seeds is None:
            from ..train import _Seeds
            base = self.seed if self.seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            self._seeds = _Seeds(base)
        return self._seeds.next()

    def _source(self, u, rows, width, device):
        """keyword arguments of ops.rbm_prob for one draw site"""
        if u is None:
            return {"seed": self._next_seed()}
        u = torch.as_tensor(u, dtype=torch.float64).to(device).contiguous()
        if u.numel() != rows * width:
            raise ValueError("RBM: %d uniforms for a plane of %d x %d" % (u.numel(), rows, width))
        return {"u": u}

    # ---- the reference's methods ----
    @staticmethod
    def sigmoid(x):
        """1 / (1 + exp(-clip(x, -500, 500))): of a tensor on its device, of anything else in numpy"""
        if torch.is_tensor(x):
            return 1.0 / (1.0 + torch.exp(-x.clamp(-500, 500)))
        return 1.0 / (1.0 + np.exp(-np.clip(x, -500, 500)))

    def sample_hidden(self, v, u=None):
        """-> (prob_h, sample_h) [rows, n_hidden]; u: float64 uniforms [rows, n_hidden] to decide with (default: counter mode)"""
        from .. import ops
        v = self._on(v, self.n_visible, "sample_hidden")
        return ops.rbm_prob(v, self.W, self.h_bias, **self._source(u, v.shape[0], self.n_hidden, v.device))

    def sample_visible(self, h, u=None):
        """-> (prob_v, sample_v) [rows, n_visible]; the sample exists for this method alone: no step uses it"""
        from .. import ops
        h = self._on(h, self.n_hidden, "sample_visible")
        return ops.rbm_prob(h, self.W, self.v_bias, down=True, **self._source(u, h.shape[0], self.n_visible, h.device))

    def _step(self, data, rows, B, bufs, partial, u):
        """one CD-k step on the rows `rows` of data (None: its first B rows): 2 + 2 k launches.  u: float64 device [k, B, n_hidden]
        or None (counter)"""
        from .. import ops
        ph, hs, nv, nh = (t[:B] for t in bufs)
        src = {"u": u[0]} if u is not None else {"seed": self._next_seed()}
        ops.rbm_prob(data, self.W, self.h_bias, rows=rows, M=B, prob=ph, sample=hs, **src)
        for g in range(self.k):
            ops.rbm_prob(hs, self.W, self.v_bias, down=True, prob=nv)
            if g + 1 < self.k:
                src = {"u": u[g + 1]} if u is not None else {"seed": self._next_seed()}
                ops.rbm_prob(nv, self.W, self.h_bias, prob=nh, sample=hs, **src)
            else:
                ops.rbm_prob(nv, self.W, self.h_bias, prob=nh)
        ops.rbm_update(data, ph, nv, nh, self.W, self.v_bias, self.h_bias, partial, self.lr, rows=rows, B=B)

    def _buffers(self, B, device):
        return tuple(torch.empty(B, n, device=device, dtype=torch.float32) for n in (self.n_hidden, self.n_hidden, self.n_visible, self.n_hidden))

    def contrastive_divergence(self, v_data, u=None):
        """one CD-k step on the batch v_data -> its reconstruction error (a float: one readback).  u: float64 [k, B, n_hidden], the
        uniforms of the k hidden draws that decide (default: counter mode)"""
        from .. import ops
        v = self._on(v_data, self.n_visible, "contrastive_divergence")
        B = v.shape[0]
        if B > ops.RBM_MAX_BATCH:
            raise ValueError("RBM.contrastive_divergence: %d rows; a step takes at most %d" % (B, ops.RBM_MAX_BATCH))
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float64).to(v.device).contiguous()
            if tuple(u.shape) != (self.k, B, self.n_hidden):
                raise ValueError("RBM.contrastive_divergence: uniforms %s; [%d, %d, %d] are needed" % (tuple(u.shape), self.k, B, self.n_hidden))
        partial = torch.empty(ops.rbm_error_tiles(self.n_visible), device=v.device, dtype=torch.float64)
        out = torch.empty(1, device=v.device, dtype=torch.float64)
        self._step(v, None, B, self._buffers(B, v.device), partial, u)
        ops.rbm_fold_error(partial, out, 1, B, B, self.n_visible)
        return float(out.item())

    def train(self, data, epochs=None, batch_size=None, verbose=True):
        """-> the list of per-epoch reconstruction errors.  Nothing returns to the host before the last step is enqueued; the
        verbose lines are the reference's, printed from the one readback."""
        from .. import ops
        epochs = epochs or config.RBM_EPOCHS
        batch_size = batch_size or config.RBM_BATCH_SIZE
        data = self._on(data, self.n_visible, "train")
        num_samples = data.shape[0]
        if batch_size > ops.RBM_MAX_BATCH or num_samples >= 2 ** 31:
            raise ValueError("RBM.train: batch_size %d (at most %d), %d rows (below 2^31)" % (batch_size, ops.RBM_MAX_BATCH, num_samples))
        dev = data.device
        steps = _steps(num_samples, batch_size)
        tiles = ops.rbm_error_tiles(self.n_visible)
        perms = u_all = None
        if self.draws is not None:
            perms = np.asarray(self.draws["perms"])
            us = self.draws["u"]
            shapes = [(self.k, min(batch_size, num_samples - s * batch_size), self.n_hidden) for s in range(steps)] * epochs
            if perms.shape != (epochs, num_samples) or [tuple(np.shape(a)) for a in us] != shapes:
                raise ValueError("RBM.train: the draws are not those of rbm_draws(%d, %d, %d, %d, %d, %d)"
                                 % (num_samples, self.n_visible, self.n_hidden, epochs, batch_size, self.k))
            if 8 * sum(int(np.size(a)) for a in us) > REPLAY_MAX_BYTES:
                raise ValueError("RBM.train: replay is for tests and small runs (at most %d bytes of uniforms)" % REPLAY_MAX_BYTES)
            perms = torch.from_numpy(perms.astype(np.int32)).to(dev)
            u_all = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in us]
        bufs = self._buffers(min(batch_size, num_samples), dev)
        partial = torch.empty(steps, tiles, device=dev, dtype=torch.float64)
        out = torch.empty(epochs, device=dev, dtype=torch.float64)
        for epoch in range(epochs):
            indices = perms[epoch] if perms is not None else torch.randperm(num_samples, device=dev, dtype=torch.int32)
            for s in range(steps):
                start = s * batch_size
                B = min(start + batch_size, num_samples) - start
                self._step(data, indices[start:start + B], B, bufs, partial[s], None if u_all is None else u_all[epoch * steps + s])
            ops.rbm_fold_error(partial, out[epoch:epoch + 1], steps, num_samples, batch_size, self.n_visible)
        errors = out.cpu().tolist()
        if verbose:
            for epoch, avg_error in enumerate(errors):
                print(f"  RBM Epoch {epoch+1}/{epochs}: "
                      f"Reconstruction Error = {avg_error:.6f}")
        return errors

    def transform(self, data):
        """the hidden probabilities of every row: one up pass, no sampling (the reference draws and drops a plane here)"""
        from .. import ops
        data = self._on(data, self.n_visible, "transform")
        return ops.rbm_prob(data, self.W, self.h_bias)

    def get_weights(self):
        return self.W.clone(), self.v_bias.clone(), self.h_bias.clone()


def pretrain_dnn_with_rbm(data, layer_sizes, verbose=True, seed=None, replay=False):
    """models/rbm.py:190-223: one RBM per hidden layer, each trained on the previous one's hidden probabilities -> the list of
    (W, v_bias, h_bias) device tensors SpeechEnhancementDNN.load_rbm_weights accepts.  data: fp32 device tensor [N, layer_sizes[0]].
    seed: base of the counter mode's seeds, one sequence over the stack.  replay=True: np.random's global stream is consumed in the
    reference's order - constructor, rbm_draws, and the plane that its transform() draws and drops - and train() replays it."""
    if seed is not None and replay:
        raise ValueError("pretrain_dnn_with_rbm: seed (counter mode) or replay, not both")
    seeds = None
    if seed is not None:
        from ..train import _Seeds
        seeds = _Seeds(seed)
    rbm_weights = []
    current_data = data
    for i in range(len(layer_sizes) - 1):
        n_visible = layer_sizes[i]
        n_hidden = layer_sizes[i + 1]
        if verbose:
            print(f"\n--- RBM Layer {i+1}: {n_visible} → {n_hidden} ---")
        rbm = RBM(n_visible, n_hidden, seed=None if seeds is None else seeds.next())
        if replay:
            rbm.draws = rbm_draws(current_data.shape[0], n_visible, n_hidden)
        rbm.train(current_data, verbose=verbose)
        rbm_weights.append(rbm.get_weights())
        current_data = rbm.transform(current_data)
        if replay:
            np.random.random((current_data.shape[0], n_hidden))
    return rbm_weights
