"""Training the DNN from a frame set, restated in float64 (tests/test_dnn_train_host.py on the CPU, tests/test_dnn_train_gpu.py on
the GPU).  No GPU import.  Imports tests/dnn_cases.py and changes nothing there.

  frame_set        the fixture's five utterances of 1, 3, 11, 12 and 130 frames: 54-column float32 rows whose 15 leading columns are
                   exactly 0 (the AMS block), one nan, +inf and -inf among them; 64-column masks with a nan, +inf, -inf, a value
                   above 1 and one below 0
  bounds           int32 [N, 2]: first and one-past-last packed row of each frame's utterance
  context_rows64   the [N, 594] context rows from the packed rows and the bounds, nan / inf -> 0 (the Dataset's nan_to_num)
  stats64          mean and population std over all frames in float64; stats_rule: rounded to float32, std < 1e-6 -> 1
  normalise64      clip((f - mean) / std, +-10)
  targets64        nan -> 0, +inf -> 1, -inf -> 0, clip to [0, 1]
  loss_dz64        mean (y - t)^2 and S 2 (y - t) / (M C) y (1 - y)
  adam_l2_step64   unscale, norm of the gradient without the decay, clip_grad_norm_, g + wd p, torch's Adam formulas; skip
  plateau          ReduceLROnPlateau(mode min, relative threshold 1e-4) on the host
  train64          the training loop on batches of row indices: dnn_cases.forward64 / backward64 (fmt: the operand-rounding emulation,
                   with the cotangent rounded under the loss scale S), loss_dz64, adam_l2_step64
  mutants          plausible wrong implementations; test_dnn_train_host.py shows that the GPU tests' bounds catch each
"""
import numpy as np
import torch

import dnn_cases as dn

LENGTHS = (1, 3, 11, 12, 130)
N_FRAMES = sum(LENGTHS)
BATCH = 37
SEED = 25
LR, WD, MAX_NORM, BETAS, EPS = 1e-3, 1e-5, 5.0, (0.9, 0.999), 1e-8
INIT_SCALE = 65536.0
W_SCALE = 5.5                                   # the fixture's hidden weights are dnn_cases' times this: some steps clip, some do not

CLAMP_MUTANTS = ("clamp_batch", "hi_off_by_one")
ADAM_MUTANTS = ("norm_with_decay", "decoupled_decay")
LOSS_MUTANTS = ("per_element_mean",)


def frame_set(seed=SEED):
    """([raw_u float32 [T_u, 54]], [mask_u float32 [T_u, 64]])"""
    rng = np.random.default_rng(seed)
    raws, masks = [], []
    for T in LENGTHS:
        r = (rng.standard_normal((T, dn.RAW_DIM)) * 1.5).astype(np.float32)
        r[:, 39:] += 40.0 * (np.arange(dn.RAW_DIM - 39) == 0)          # one column with a mean far above its spread (MFCC c0)
        r[:, :15] = 0.0
        raws.append(r)
        masks.append(rng.random((T, 64)).astype(np.float32))
    raws[4][7, 20], raws[4][100, 33], raws[2][0, 50] = np.nan, np.inf, -np.inf
    masks[4][3, 5], masks[4][64, 9], masks[3][2, 1], masks[1][0, 0], masks[4][129, 63] = np.nan, np.inf, -np.inf, 1.75, -0.5
    return raws, masks


def bounds(lengths=LENGTHS):
    ends = np.cumsum(lengths)
    starts = ends - np.asarray(lengths)
    return np.stack([np.repeat(starts, lengths), np.repeat(ends, lengths)], axis=1).astype(np.int32)


def context_rows64(raw, bnd, ctx=dn.CTX, mutant=None):
    """raw [N, D] packed -> float64 [N, D (2 ctx + 1)], nan / inf read as 0"""
    N, D = raw.shape
    clean = np.where(np.isfinite(raw), raw, 0.0).astype(np.float64)
    out = np.zeros((N, D * (2 * ctx + 1)))
    for n in range(N):
        lo, hi = int(bnd[n, 0]), int(bnd[n, 1])
        if mutant == "clamp_batch":
            lo, hi = 0, N
        if mutant == "hi_off_by_one":
            hi = min(hi + 1, N)
        idx = np.clip(np.arange(n - ctx, n + ctx + 1), lo, hi - 1)
        out[n] = clean[idx].reshape(-1)
    return out


def stats64(rows):
    return rows.mean(axis=0), rows.std(axis=0)


def stats_rule(mean, std):
    """what is stored: float32, std < 1e-6 -> 1"""
    m, s = mean.astype(np.float32), std.astype(np.float32)
    s[s < 1e-6] = 1.0
    return m, s


def normalise64(rows, mean, std):
    return np.clip((rows - mean.astype(np.float64)) / std.astype(np.float64), -10.0, 10.0)


def targets64(mask):
    return np.clip(np.nan_to_num(mask.astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)


def loss_dz64(y, t, S=1.0):
    d = y - t
    return float(np.mean(d * d)), S * 2.0 * d / d.size * y * (1.0 - y)


def epoch_loss(batch_losses, sizes=None, mutant=None):
    """the reference averages the per-batch means: the ragged last batch weighs as much as a full one"""
    ok = [(l, n) for l, n in zip(batch_losses, sizes or [1] * len(batch_losses)) if np.isfinite(l)]
    if mutant == "per_element_mean":
        return sum(l * n for l, n in ok) / max(sum(n for _, n in ok), 1)
    return sum(l for l, _ in ok) / max(len(ok), 1)


def adam_l2_step64(p, g, m, v, step, lr=LR, wd=WD, max_norm=MAX_NORM, betas=BETAS, eps=EPS, S=1.0, skip=False, mutant=None):
    """flat float64 arrays; g = S times the gradient -> (p, m, v, step, norm, skipped)"""
    g = g / S
    norm = float(np.sqrt(np.sum(g * g)))
    if mutant == "norm_with_decay":
        norm = float(np.sqrt(np.sum((g + wd * p) ** 2)))
    if skip or not np.isfinite(norm):
        return p, m, v, step, norm, True
    if norm > max_norm:
        g = g * (max_norm / (norm + 1e-6))
    step += 1
    if mutant == "decoupled_decay":
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = betas[0] * m + (1.0 - betas[0]) * g
    v = betas[1] * v + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v, step, norm, False


def plateau(losses, lr, factor=0.5, patience=5, min_lr=1e-6, threshold=1e-4, eps=1e-8):
    """-> the rate after each epoch's scheduler.step(loss)"""
    best, bad, out = float("inf"), 0, []
    for l in losses:
        if l < best * (1.0 - threshold):
            best, bad = l, 0
        else:
            bad += 1
        if bad > patience:
            new = max(lr * factor, min_lr)
            if lr - new > eps:
                lr = new
            bad = 0
        out.append(lr)
    return out


def flat(arrs):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in arrs])


def unflat(vec, like):
    out, off = [], 0
    for a in like:
        out.append(vec[off:off + a.size].reshape(a.shape))
        off += a.size
    return out


def interleave(Ws, bs):
    """parameter order of the module: W0, b0, W1, b1, ..."""
    return [t for pair in zip(Ws, bs) for t in pair]


def batches(n=N_FRAMES, size=BATCH):
    return [np.arange(s, min(s + size, n)) for s in range(0, n, size)]


def backward_from_dz64(Ws, hs, dz, fmt=None):
    """dnn_cases.backward64 from the output layer's pre-activation cotangent on, without dropout -> ([dW_l], [db_l])"""
    dWs, dbs = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        dz = dn.rnd(dz, fmt)
        dWs[l] = dz.T @ dn.rnd(hs[l], fmt)
        dbs[l] = dz.sum(0)
        if l > 0:
            dz = dn.rnd(dz @ dn.rnd(Ws[l], fmt), fmt) * (hs[l] > 0)
    return dWs, dbs


def train64(Ws, bs, rows, targets, index_batches, epochs, fmt=None, S=1.0, max_steps=None):
    """-> dict(losses per step, norms per step, params after each step (flat, module order), epoch training losses)
    fmt: the operand-rounding emulation; the output cotangent is rounded to fmt under the scale S, as the device writes it"""
    Ws = [w.astype(np.float64) for w in Ws]
    bs = [b.astype(np.float64) for b in bs]
    p = flat(interleave(Ws, bs))
    like = interleave(Ws, bs)
    m, v, step = np.zeros_like(p), np.zeros_like(p), 0
    out = dict(loss=[], norm=[], params=[], epoch=[])
    for _ in range(epochs):
        per_batch = []
        for idx in index_batches:
            cur = unflat(p, like)
            W_, b_ = cur[0::2], cur[1::2]
            y, _, hs = dn.forward64(W_, b_, rows[idx], fmt=fmt)
            loss, dz = loss_dz64(y, targets[idx], S)
            dWs, dbs = backward_from_dz64(W_, hs, dz, fmt=fmt)
            p, m, v, step, norm, _ = adam_l2_step64(p, flat(interleave(dWs, dbs)), m, v, step, S=S)
            out["loss"].append(loss)
            out["norm"].append(norm)
            out["params"].append(p.copy())
            per_batch.append(loss)
            if max_steps is not None and len(out["loss"]) >= max_steps:
                return out
        out["epoch"].append(epoch_loss(per_batch))
    return out


def validate64(params_flat, like, rows, targets, index_batches, fmt=None):
    cur = unflat(params_flat, like)
    losses = [loss_dz64(dn.forward64(cur[0::2], cur[1::2], rows[idx], fmt=fmt)[0], targets[idx])[0] for idx in index_batches]
    return epoch_loss(losses)


def fixture_params():
    """the fixture's initial model: dnn_cases' seeded small model, its weights scaled so that the first steps' gradient norms lie
    on both sides of the clip"""
    Ws, bs = dn.params(dn.SMALL, dn.GOLDEN_SEED)
    scales = (W_SCALE, W_SCALE, W_SCALE, W_SCALE ** -3)                    # the outputs keep their size, the gradients grow
    return [(w * k).astype(np.float32) for w, k in zip(Ws, scales)], bs


# ---- the FlatAdam case of tests/test_dnn_train_gpu.py, shared with the mutant test on the CPU --------------------------------------
ADAM_DECAYS = (WD, 0.1)        # the reference's decay, and one at which the decay term is visible in the norm and in five steps
ADAM_SKIP = 2                  # the third of the five steps is skipped by the flag
ADAM_NORM_RTOL = 1e-6


def adam_case(features, masks):
    """(p0 float32 flat, [g_k float32 flat]): the fixture's initial parameters and the gradients of its five batches there.  At the
    initial parameters every batch's norm is above the clip: every other gradient is halved, to lie below it."""
    Ws, bs = fixture_params()
    x, t = features.astype(np.float64), masks.astype(np.float64)
    grads = []
    for idx in batches():
        y, _, hs = dn.forward64(Ws, bs, x[idx])
        dWs, dbs = backward_from_dz64([w.astype(np.float64) for w in Ws], hs, loss_dz64(y, t[idx])[1])
        grads.append((flat(interleave(dWs, dbs)) * (0.5 if len(grads) % 2 else 1.0)).astype(np.float32))
    return flat(interleave(Ws, bs)).astype(np.float32), grads


def adam_run64(p0, grads, wd, mutant=None):
    """the five steps in float64 -> (p, m, v, [norm per step])"""
    p, m, v, step, norms = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size), 0, []
    for k, g in enumerate(grads):
        p, m, v, step, norm, _ = adam_l2_step64(p, g.astype(np.float64), m, v, step, wd=wd, skip=k == ADAM_SKIP, mutant=mutant)
        norms.append(norm)
    return p, m, v, norms


def adam_e32(p0, grads, wd):
    """max |torch.optim.Adam + clip_grad_norm_ in float32 on the CPU - float64| for (p, m, v) over the same five steps"""
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref = torch.optim.Adam([q], lr=LR, weight_decay=wd)
    for k, g in enumerate(grads):
        if k != ADAM_SKIP:
            q.grad = torch.from_numpy(g.copy())
            torch.nn.utils.clip_grad_norm_([q], MAX_NORM)
            ref.step()
    p, m, v, _ = adam_run64(p0, grads, wd)
    st = ref.state[q]
    return [float(np.abs(a.detach().double().numpy() - b).max()) for a, b in ((q, p), (st["exp_avg"], m), (st["exp_avg_sq"], v))]


def adam_within(got, want, e32, norms_got, norms_want):
    """the GPU test's assertion: p, m, v within 16 x e32 and every step's norm within ADAM_NORM_RTOL relative"""
    ok = all(float(np.abs(g - w).max()) <= 16 * e for g, w, e in zip(got, want, e32))
    return ok and all(abs(a / b - 1.0) < ADAM_NORM_RTOL for a, b in zip(norms_got, norms_want))


def subnormal_share(dz64, S, fmt=torch.float16):
    """share of the elements with a non-zero float64 cotangent that fmt holds as 0 or as a subnormal under the scale S"""
    live = dz64 != 0
    r = np.abs(dn.rnd(dz64 * S, fmt))
    tiny = 2.0 ** -14 if fmt is torch.float16 else 2.0 ** -126
    return float(np.mean(r[live] < tiny))
