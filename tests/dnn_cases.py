"""SpeechEnhancementDNN restated in float64 (tests/test_dnn_host.py on the CPU, tests/test_dnn_gpu.py on the GPU).  No GPU import.

  cases          seeded: Kaiming-normal weights N(0, 2 / fan_in), biases 0.05 N(0, 1), inputs clip(1.5 N(0, 1), +-10); parameters
                 and inputs are float32 values (what the device is handed), the restatement computes on them in float64
  forward64      [Linear, ReLU, keep] x L, Linear, sigmoid; keep = the factors of tests/dropout_cases.py's host replica of
                 sfm_keep_scale at element m N + n, one seed per hidden layer from train._Seeds (dropout_cases.Seeds)
  emulation      fmt = torch.float16 / torch.bfloat16: the same float64 arithmetic with the weights and each layer's input rounded to
                 fmt and the hidden outputs rounded to fmt (they are the next layer's 16-bit operand); backward: the cotangent of each
                 pre-activation, the saved operands and the weights rounded, the data gradient between hidden layers rounded
  backward64     from given active-and-kept masks (the device's own: h > 0), so that a unit whose sign the 16-bit forward decided
                 the other way is no gradient error
  context64      FeatureExtractor.add_context restated: the clamped gather, nan / inf -> 0, (f - mean) / std, clip to +-10
  mutants        plausible wrong kernels; test_dnn_host.py shows that the GPU tests' bounds catch each of them
"""
import numpy as np
import torch

import dropout_cases as dc

CTX = 5
RAW_DIM = 54
SMALL = (594, 64, 64, 64, 64)                  # the fixture's model: input 594, hidden 64 x 3, output 64
DEFAULT = (594, 1024, 1024, 1024, 64)
SMALL_ROWS = 37
GOLDEN_SEED = 22
GRAD_COLS = np.r_[0:594:7, 584:594]         # the columns of network.0.weight's gradient that the fixture stores
P_DROP = 0.2

FWD_MUTANTS = ("no_bias", "k_tail_zero", "no_drop_scale")
CTX_MUTANTS = ("clamp_lo", "clamp_hi", "clip_first")
BWD_MUTANTS = ("sigmoid_no_1my", "no_drop_scale")


def params(dims, seed):
    """([W_l float32 [dims[l + 1], dims[l]]], [b_l float32])"""
    rng = np.random.default_rng(seed)
    Ws = [(rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.05).astype(np.float32) for i in range(len(dims) - 1)]
    return Ws, bs


def inputs(M, K, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((M, K)) * 1.5, -10.0, 10.0).astype(np.float32)


def targets(M, N, seed):
    return np.random.default_rng(seed).random((M, N)).astype(np.float32)


def raw_frames(B, T, seed, D=RAW_DIM):
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((B, T, D)) * 1.5, -10.0, 10.0).astype(np.float32)


CTX_FRAMES = (23, 7, 1)                        # T_b of the context case: a full utterance, a short one, a single frame


def context_case():
    """raw [3, 23, 54] with a nan and an inf cell and a few large ones (the clip acts only behind the normalisation), mean, std"""
    raw = raw_frames(3, 23, 31)
    raw[0, 3, 7], raw[1, 2, 50] = np.nan, np.inf
    raw[0, 10, :4], raw[2, 0, 5] = 9.0, -9.5
    mean, std = stats(594, 32)
    return raw, mean, std


def stats(K, seed):
    """feat_mean, feat_std float32 [K]; std in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(K) * 0.3).astype(np.float32), (0.5 + 1.5 * rng.random(K)).astype(np.float32)


def rbm_tuples(dims, seed):
    """(W [visible, hidden], visible_bias, hidden_bias) float64 per Linear of the model, the output layer's included"""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((dims[i], dims[i + 1])) * 0.1, rng.standard_normal(dims[i]) * 0.1,
             rng.standard_normal(dims[i + 1]) * 0.1) for i in range(len(dims) - 1)]


def state_dict(Ws, bs):
    sd = {}
    for l, (w, b) in enumerate(zip(Ws, bs)):
        sd["network.%d.weight" % (3 * l)] = torch.from_numpy(w.copy())
        sd["network.%d.bias" % (3 * l)] = torch.from_numpy(b.copy())
    return sd


def rnd(a, fmt):
    """a (float64) rounded to fmt, as float64; fmt None: unchanged"""
    if fmt is None:
        return np.asarray(a, dtype=np.float64)
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(torch.float32).to(fmt).double().numpy()


def layer_seeds(base, n):
    s = dc.Seeds(base)
    return [s.next() for _ in range(n)]


def keep_masks(base, M, widths, p):
    """float64 [M, N_l] per hidden layer: 1 / (1 - p) where element m N_l + n is kept, 0 where dropped (None when p = 0)"""
    if p <= 0:
        return None
    return [dc.keep_elems(s, 0, M * N, p).reshape(M, N) for s, N in zip(layer_seeds(base, len(widths)), widths)]


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward64(Ws, bs, x, keeps=None, fmt=None, mutant=None):
    """-> (y [M, out], zs: the pre-activations, hs: the layer inputs [x, h_1, ..., h_L] as the next layer reads them)"""
    h = rnd(x, fmt)
    hs, zs = [h], []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W = rnd(W, fmt)
        if mutant == "k_tail_zero" and l == 0:
            W = W.copy()
            W[:, 592:] = 0.0
        z = h @ W.T + (0.0 if mutant == "no_bias" else b.astype(np.float64))
        zs.append(z)
        if l == len(Ws) - 1:
            return sigmoid(z), zs, hs
        h = np.maximum(z, 0.0)
        if keeps is not None:
            h = h * ((keeps[l] > 0) if mutant == "no_drop_scale" else keeps[l])
        h = rnd(h, fmt)
        hs.append(h)


def backward64(Ws, hs, y, dy, p=0.0, fmt=None, mutant=None):
    """hs: the layer inputs (hs[l + 1] > 0 is the active-and-kept mask of hidden layer l) -> (dx, [dW_l], [db_l])"""
    dz = dy * y * (1.0 if mutant == "sigmoid_no_1my" else (1.0 - y))
    dWs, dbs = [None] * len(Ws), [None] * len(Ws)
    scale = 1.0 if mutant == "no_drop_scale" else 1.0 / (1.0 - p)
    for l in range(len(Ws) - 1, -1, -1):
        dz = rnd(dz, fmt)
        dWs[l] = dz.T @ rnd(hs[l], fmt)
        dbs[l] = dz.sum(0)
        dx = dz @ rnd(Ws[l], fmt)
        if l > 0:
            dz = rnd(dx, fmt) * np.where(hs[l] > 0, scale, 0.0)
    return dx, dWs, dbs


def mse_grad(y, target):
    """d mean((y - t)^2) / dy"""
    return 2.0 * (y - target.astype(np.float64)) / y.size


def context64(raw, frames, ctx=CTX, mean=None, std=None, mutant=None):
    """raw [B, T, D] -> float64 [B, T, D (2 ctx + 1)]; frames: T_b per utterance (None: T); rows from T_b on are 0"""
    B, T, D = raw.shape
    out = np.zeros((B, T, D * (2 * ctx + 1)))
    lo = 1 if mutant == "clamp_lo" else 0
    for b in range(B):
        tb = T if frames is None else int(frames[b])
        hi = tb - 1 - (1 if mutant == "clamp_hi" else 0)
        for n in range(tb):
            idx = np.clip(np.arange(n - ctx, n + ctx + 1), lo, max(hi, lo))
            idx = np.minimum(idx, tb - 1)
            f = raw[b, idx].astype(np.float64).reshape(-1)
            if mean is not None:
                f = np.where(np.isfinite(f), f, 0.0)
                if mutant == "clip_first":
                    f = (np.clip(f, -10.0, 10.0) - mean) / std
                else:
                    f = np.clip((f - mean) / std, -10.0, 10.0)
            out[b, n] = f
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def err(got, exact):
    """(RMS, max) of got - exact"""
    d = np.asarray(got, dtype=np.float64) - exact
    return rms(d), float(np.abs(d).max())


def rel(got, ref):
    return rms(np.asarray(got, dtype=np.float64) - ref) / max(rms(ref), 1e-300)


def flip_share(h_got, z_exact, keeps=None):
    """share of hidden units whose sign (got > 0) differs from float64's `z > 0 and kept`"""
    want = z_exact > 0
    if keeps is not None:
        want = want & (keeps > 0)
    return float(np.mean((np.asarray(h_got) > 0) != want))


_cache = {}


def model_case(name, dims, M, seed):
    """the seeded case `name`: parameters, inputs, the exact forward and (per format) the emulation, computed once and shared"""
    if name not in _cache:
        Ws, bs = params(dims, seed)
        x = inputs(M, dims[0], seed + 1)
        y, zs, hs = forward64(Ws, bs, x)
        _cache[name] = dict(Ws=Ws, bs=bs, x=x, y=y, zs=zs, hs=hs, emu={})
    return _cache[name]


def emulation(case, fmt):
    if fmt not in case["emu"]:
        case["emu"][fmt] = forward64(case["Ws"], case["bs"], case["x"], fmt=fmt)
    return case["emu"][fmt]


def default_case():
    return model_case("default", DEFAULT, 203, 7)


def small_case():
    return model_case("small", SMALL, SMALL_ROWS, GOLDEN_SEED)
