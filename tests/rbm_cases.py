"""The RBM pre-training (models/rbm.py of the reference) restated in numpy (tests/test_rbm_host.py on the CPU, tests/test_rbm_gpu.py
on the GPU).  No GPU import.

  restatement    step / train / stack take every draw as an ARGUMENT (the uniforms that decide and the permutations; what
                 models.rbm_draws returns), in any dtype: float64 equals the reference (tests/golden/g24_rbm.npz), float32 is the
                 measure e32 of what fp32 arithmetic costs on the same inputs.  A step can also be given the hidden samples
                 themselves (the device's own), so that a unit decided the other way is no error of the tensors behind it.
  bounds         per tensor 16 x e32 = 16 x max |float32 run - float64 run|; for a probability that enters a decision additionally
                 at most an eighth of the fixture's smallest margin |prob - u|
  counter rule   sample_counter: the host replica of the device's seeded decision, from dropout_cases.sfm_hash:
                 S[m, n] = 1 iff word(seed, m N + n) < ceil(float32(prob) 2^24), word = the 24-bit number the dropout keep function
                 compares with its threshold
  mutants        plausible wrong kernels; test_rbm_host.py shows that each misses the bounds on a named tensor
"""
import math

import numpy as np

import dropout_cases as dc

V, H, ROWS, BATCH, EPOCHS, LR = 70, 48, 101, 37, 2, 0.01
STACK = (70, 48, 48, 48)
KS = (1, 2)
BIG = (594, 1024, 203)                      # one step at the first layer's shape: n_visible, n_hidden, B
MUTANTS = ("neg_from_samples", "div_batch_size", "vbias_from_sample", "ge", "down_transposed", "no_hbias_second_up", "err_sum")
# the tensor on which each mutant must miss its bound (train: the fixture's two epochs; plane: the sample plane with u = prob)
MUTANT_TENSOR = {"neg_from_samples": "W", "div_batch_size": "W", "vbias_from_sample": "v_bias", "ge": "plane", "down_transposed": "W",
                 "no_hbias_second_up": "h_bias", "err_sum": "errors"}


def data(rows, width, seed):
    """float32 values in (0, 1): squashed normals, as the pipeline hands them over"""
    rng = np.random.default_rng(seed)
    return (1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal((rows, width))))).astype(np.float32)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.clip(x, -500, 500)))


def decide(prob, u, mutant=None):
    """prob (any dtype) against float64 uniforms, compared in float64 as the device does"""
    p = prob.astype(np.float64)
    return (p >= u) if mutant == "ge" else (p > u)


def step(state, v, k, lr, u=None, samples=None, dt=np.float64, mutant=None, batch_size=None):
    """one CD-k step in dtype dt.  state = (W, v_bias, h_bias), updated copies are returned.  u float64 [k, B, n_hidden] or
    samples = the k hidden sample planes.  -> (new state, dict(ph, hs [k planes], nv, nh, err))"""
    W, vb, hb = (a.astype(dt) for a in state)
    v = v.astype(dt)
    lr = dt(lr)
    B = v.shape[0]

    def hidden(x, with_bias=True):
        return sigmoid(x @ W + (hb if with_bias else dt(0))).astype(dt)

    def visible(h):
        Wd = W.reshape(W.shape[1], W.shape[0]) if mutant == "down_transposed" else W.T
        return sigmoid(h @ Wd + vb).astype(dt)

    def plane(prob, g):
        return samples[g].astype(dt) if samples is not None else decide(prob, u[g], mutant).astype(dt)

    ph = hidden(v)
    hs = [plane(ph, 0)]
    h = hs[0]
    for g in range(k):
        nv = visible(h)
        nh = hidden(nv, with_bias=mutant != "no_hbias_second_up")
        if g + 1 < k:
            hs.append(plane(nh, g + 1))
            h = hs[-1]
    neg_h = (nh > 0.5).astype(dt) if mutant == "neg_from_samples" else nh
    div = dt(batch_size if (mutant == "div_batch_size" and batch_size) else B)
    W = (W + lr * (v.T @ ph - nv.T @ neg_h) / div).astype(dt)
    nv_b = (nv > 0.5).astype(dt) if mutant == "vbias_from_sample" else nv
    vb = (vb + lr * np.mean(v - nv_b, axis=0)).astype(dt)
    hb = (hb + lr * np.mean(ph - nh, axis=0)).astype(dt)
    d = (v - nv).astype(np.float64)
    err = float(np.sum(d * d)) if mutant == "err_sum" else float(np.mean(d * d))
    return (W, vb, hb), {"ph": ph, "hs": hs, "nv": nv, "nh": nh, "err": err}


def train(state, x, draws, k, lr, batch_size, dt=np.float64, mutant=None):
    """RBM.train with the draws of models.rbm_draws -> (state, [per-epoch errors], first step's dict)"""
    perms, us = draws["perms"], draws["u"]
    n = x.shape[0]
    errors, first, s = [], None, 0
    for epoch in range(perms.shape[0]):
        tot, nb = 0.0, 0
        for start in range(0, n, batch_size):
            rows = perms[epoch][start:min(start + batch_size, n)]
            state, out = step(state, x[rows], k, lr, u=us[s], dt=dt, mutant=mutant, batch_size=batch_size)
            first = first or out
            tot += out["err"]
            nb += 1
            s += 1
        errors.append(tot / nb)
    return state, errors, first


def stack(states, x, draws, k, lr, batch_size, dt=np.float64):
    """pretrain_dnn_with_rbm: states / draws per layer -> [(W, v_bias, h_bias)]"""
    out, cur = [], x
    for st, dr in zip(states, draws):
        st, _, _ = train(st, cur, dr, k, lr, batch_size, dt=dt)
        out.append(st)
        cur = sigmoid(cur.astype(dt) @ st[0] + st[2]).astype(dt)
    return out


def f32_state(state):
    """the state as the device holds it: float32 values"""
    return tuple(np.asarray(a, dtype=np.float32) for a in state)


def err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def bound(a32, a64, margin=None):
    """16 x e32, and for a probability that enters a decision at most margin / 8"""
    b = 16.0 * err(a32, a64)
    return min(b, margin / 8.0) if margin is not None else b


def sample_counter(prob32, seed):
    """the device's counter rule on float32 probabilities [M, N] -> float32 0 / 1"""
    p = np.asarray(prob32, dtype=np.float32)
    M, N = p.shape
    idx = np.arange(M * N, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    gh = dc.sfm_hash(seed, idx >> np.uint64(3))
    x = (gh + (((idx & np.uint64(7)) * np.uint64(0x9E3779B1)) & m32)) & m32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & m32
    x ^= x >> np.uint64(16)
    word = (x >> np.uint64(8)).astype(np.int64).reshape(M, N)
    thr = np.ceil(p.astype(np.float64) * 16777216.0).astype(np.int64)        # float32(p) 2^24 is exact in float32 and in float64
    return (word < thr).astype(np.float32)


def keep_threshold(p):
    return int(math.ceil(float(np.float32(p)) * 16777216.0))
