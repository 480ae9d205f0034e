"""Training on packed rows: the cases and float64 references of tests/test_packed_train_host.py (CPU) and
tests/test_packed_train_gpu.py (GPU).  No GPU import here.

A pack holds utterances of T_u frames back to back; utterance u = rows [off[u], off[u + 1]).  Everything row-wise in a Conformer
block is the dense restatement on [1, sum_T, D]; what sees the utterances is restated here per utterance from the pieces of
helpers.py and dropout_cases.py:

  attention      helpers.attn_ref64 on each utterance alone; the dropout factor on its probabilities from the replica of the
                 PACKED row rule (packed_keep): hash row H * off[u] + h * T_u + q, utterance-local key index
  depthwise      helpers.dwconv64 / helpers.dwconv_wgrad64 on each utterance alone ([1, T_u, C]), gradients summed over utterances
  BatchNorm      batch statistics over the concatenated valid rows (helpers.bn_stats64 restates them; packed_conv64 forms them
                 inside autograd so that the gradient flows through them)
  block / model  packed_block64 / packed_enhancer64 from dropout_cases.ffn64 / mhsa64 and packed_conv64

References are computed once per case (functools-style cache), shared by the tests and never modified.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dropout_cases as dc
import helpers as hp
from oracle import sfm_oracle as orc

# ---- length sets: the smallest at which each kernel can go wrong -----------------------------------------------------------------
# attention: one row; the edges of a wave's 32 rows; the 64-key tile edges; one and two 128-row tiles, three with a one-row tail
ATTN_RAGGED = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
ATTN_SETS = {"ragged": ATTN_RAGGED, "reversed": ATTN_RAGGED[::-1], "equal": [130, 130, 130]}
# depthwise conv and its weight gradient: utterances shorter than the pad (15 / 3), than the kernel and than a 64-frame tile
CONV_LENGTHS = [1, 3, 14, 15, 16, 30, 31, 32, 63, 64, 65, 200]
# (KS, C): the LDS kernel of the Conformer's conv, the register-window kernel at KS 7 and at KS 31 (C no multiple of 256)
WGRAD_ROWS = [(31, 256), (7, 256), (31, 64)]
H, HD = 4, 64
D = H * HD
FF = 1024
DTYPES = [torch.float16, torch.bfloat16]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# the dense attention kernels' bounds (tests/test_backward_gpu.py::test_attention_train_fwd_bwd, test_attention_rule_gpu.py):
# O 8 roundings of an O(1) value; log2-domain LSE; each of dq / dk / dv 0.03 max|g| + 8 eps max|g|; RMSE of dqkv
LSE_TOL = {torch.bfloat16: 6e-3, torch.float16: 1e-3}
DQKV_RMS = {torch.bfloat16: 0.02, torch.float16: 0.004}
# relative RMSE of the block's output, dx, parameter gradients and running statistics against float64 (the issue's figures)
BLOCK_TOL = {torch.float16: 3e-3, torch.bfloat16: 2.5e-2}
MASK_TOL = 1e-3                                # forward_packed_train against forward_packed (the existing mask bound)

_cache = {}


def cached(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    wrapped.__name__ = fn.__name__
    return wrapped


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


def rows_of(lengths, u):
    off = offsets(lengths)
    return slice(int(off[u]), int(off[u + 1]))


# ---- the dropout replica under the packed row rule ------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def keep_of_rows(seed, rows, T, p):
    """float32 [len(rows), T]: the keep factor of probability row `rows[i]` (the hashed index) at keys 0 .. T - 1: the full hash
    of the row (dropout_cases.sfm_hash), then one multiply-add and one xorshift-multiply round per key (helpers.keep_mask)"""
    x = dc.sfm_hash(seed, np.asarray(rows, dtype=np.uint64))
    key = np.arange(T, dtype=np.uint64)
    y = (x[:, None] + ((key * np.uint64(0x9E3779B1)) & _M32)[None, :]) & _M32
    y ^= y >> np.uint64(15); y = (y * np.uint64(0x846CA68B)) & _M32
    y ^= y >> np.uint64(16)
    keep = ((y >> np.uint64(8)) >= np.uint64(dc.keep_threshold(p))).astype(np.float32) / (1.0 - p)
    return torch.from_numpy(keep)


def packed_keep(seed, lengths, nheads, p, rule="packed"):
    """per utterance [1, H, T_u, T_u]: the keep factors of the pack.  rule "packed": hash row H * off[u] + h * T_u + q (the
    kernels'); "dense" (a wrong variant): (u * H + h) * T_u + q, the dense launch's index with the utterance as its batch entry"""
    off = offsets(lengths)
    out = []
    for u, T in enumerate(lengths):
        h, q = np.meshgrid(np.arange(nheads, dtype=np.int64), np.arange(T, dtype=np.int64), indexing="ij")
        rows = (nheads * off[u] + h * T + q) if rule == "packed" else ((u * nheads + h) * T + q)
        out.append(keep_of_rows(seed, rows.reshape(-1), T, p).reshape(1, nheads, T, T))
    return out


# ---- attention ------------------------------------------------------------------------------------------------------------------
SEED = 77


def q16(x, dt):
    return x.to(dt).float()


@cached
def attn_inputs(name, dt):
    """(qkv [sum_T, 3 D], dO [sum_T, D]) rounded to dt, as floats: q at the pre-scaled magnitude of the dense tests"""
    n = int(sum(ATTN_SETS[name]))
    qkv = hp.arr("pt_q", (n, 3 * D), 40 + n, 1.0)
    qkv[:, :D] *= 0.35
    dO = hp.arr("pt_do", (n, D), 41 + n, 0.5)
    return q16(qkv, dt), q16(dO, dt)


@cached
def attn_case(name, dt, p, mutant=None):
    """per utterance (O [T_u, D], LSE [H, T_u], dqkv [T_u, 3 D]) in float64.  mutant "dense index": the dropout mask under the
    dense row index; "neighbour keys": every utterance but the last also attends to the next utterance's rows (O and LSE only)"""
    lengths = ATTN_SETS[name]
    qkv, dO = attn_inputs(name, dt)
    keep = packed_keep(SEED, lengths, H, p, "dense" if mutant == "dense index" else "packed") if p > 0 else None
    out = []
    for u, T in enumerate(lengths):
        r = rows_of(lengths, u)
        if mutant == "neighbour keys" and u + 1 < len(lengths):
            r2 = slice(r.start, rows_of(lengths, u + 1).stop)
            n2 = r2.stop - r2.start
            o, lse, _ = hp.attn_ref64(qkv[r2], 1, n2, H, HD, prescaled=True)
            out.append((o[:T], lse[0, :, :T], None))
            continue
        o, lse, g = hp.attn_ref64(qkv[r], 1, T, H, HD, prescaled=True, dO=dO[r], keep=None if keep is None else keep[u])
        out.append((o, lse[0], g))
    return out


def attn_tols(dt, gref):
    """(O, LSE, each of dq / dk / dv, RMSE of dqkv) for a gradient reference gref: the dense tests' bounds"""
    scale = float(gref.abs().max())
    return 8 * EPS[dt], LSE_TOL[dt], 0.03 * scale + 8 * EPS[dt] * scale, DQKV_RMS[dt] * float(gref.pow(2).mean().sqrt()) + 1e-6


def separates_abs(name, mutant, moved, bound):
    """helpers.separates for an absolute bound: the wrong form moves the reference by >= 5 x the bound"""
    print("MUTANT | %s | %s | moves the reference by %.1f x the bound" % (name, mutant, moved / bound))
    assert moved >= 5.0 * bound, (name, mutant, moved, bound)


# ---- depthwise weight gradient --------------------------------------------------------------------------------------------------
def _wgrad_sum(x, dy, lengths, KS, dtype, mutant=None):
    """sum over utterances of helpers.dwconv_wgrad64 on each alone; mutant "window crosses": the pack as ONE utterance"""
    if mutant == "window crosses":
        return hp.dwconv_wgrad64(x.to(dtype)[None], dy.to(dtype)[None], KS)
    dw = db = 0
    for u in range(len(lengths)):
        r = rows_of(lengths, u)
        a, b = hp.dwconv_wgrad64(x[r].to(dtype)[None], dy[r].to(dtype)[None], KS)
        dw, db = dw + a, db + b
    return dw, db


def wgrad_inputs(lengths, C, dt, tag=0):
    """x rounded to the 16-bit format, dy fp32, both with the offset of helpers.dwgrad_case (the sums do not cancel)"""
    n = int(sum(lengths))
    x = (hp.arr("pw_x", (n, C), n + C + tag) + 2.0).to(dt).float()
    dy = hp.arr("pw_g", (n, C), n + C + 1 + tag) + 2.0
    return x, dy


def wgrad_ref(x, dy, lengths, KS, mutant=None):
    """dict(ref64, ref32, dw_bound, db_bound) as helpers.dwgrad_case builds them, over the pack"""
    lengths = list(lengths)
    n = int(sum(lengths)) + 2
    mag = _wgrad_sum(x.double().abs(), dy.double().abs(), lengths, KS, torch.float64)
    return dict(ref64=_wgrad_sum(x, dy, lengths, KS, torch.float64, mutant), ref32=_wgrad_sum(x, dy, lengths, KS, torch.float32),
                dw_bound=hp.sum_terms_bound(n, mag[0]), db_bound=hp.sum_terms_bound(n, mag[1]))


@cached
def wgrad_case(KS, C, dt):
    x, dy = wgrad_inputs(CONV_LENGTHS, C, dt)
    c = wgrad_ref(x, dy, CONV_LENGTHS, KS)
    c.update(x=x, dy=dy, wrong64=_wgrad_sum(x, dy, CONV_LENGTHS, KS, torch.float64, "window crosses"))
    return c


def dwconv_packed64(x, w, bias, lengths, mutant=None):
    """helpers.dwconv64 on each utterance alone -> [sum_T, C]; mutant "window crosses": on the pack as one utterance"""
    if mutant == "window crosses":
        return hp.dwconv64(x[None], w, bias)[0]
    return torch.cat([hp.dwconv64(x[rows_of(lengths, u)][None], w, bias)[0] for u in range(len(lengths))])


# ---- ConformerBlock on packed rows, float64 --------------------------------------------------------------------------------------
def packed_conv64(x, sd, lengths, bn_eval=False, branch=None, stats=None, eps=1e-5):
    """dropout_cases.conv64 on packed rows x [sum_T, D]: the depthwise conv per utterance, BatchNorm over the sum_T valid rows
    (bn_eval: on the running statistics).  stats: receives mean, biased variance and n, as conv64's"""
    Dm = x.shape[1]
    h = orc.layer_norm(x, sd["layer_norm.weight"], sd["layer_norm.bias"])
    h = orc.linear(h, sd["pointwise1.weight"].reshape(2 * Dm, Dm), sd["pointwise1.bias"])
    a, g = h.split(Dm, dim=1)
    glu = a * torch.sigmoid(g)
    ksz = sd["depthwise.weight"].shape[-1]
    parts = []
    for u in range(len(lengths)):
        xu = glu[rows_of(lengths, u)].t()[None]
        parts.append(F.conv1d(xu, sd["depthwise.weight"], sd["depthwise.bias"], padding=(ksz - 1) // 2, groups=Dm)[0].t())
    y = torch.cat(parts)
    if bn_eval:
        mean, var = sd["batch_norm.running_mean"].to(y.dtype), sd["batch_norm.running_var"].to(y.dtype)
    else:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        if stats is not None:
            stats.update(mean=mean.detach(), var=var.detach(), n=y.shape[0])
    t = (y - mean) * torch.rsqrt(var + eps) * sd["batch_norm.weight"] + sd["batch_norm.bias"]
    h = orc.linear(orc.swish(t), sd["pointwise2.weight"].reshape(Dm, Dm), sd["pointwise2.bias"])
    if branch is not None:
        h = h * branch
    return x + h


def packed_mhsa64(x, sd, lengths, nheads, prob=None, branch=None, mutant=None):
    """dropout_cases.mhsa64 with every utterance attending to its own rows; prob: packed_keep's list; branch [sum_T, D]"""
    outs = []
    for u in range(len(lengths)):
        r = rows_of(lengths, u)
        outs.append(dc.mhsa64(x[r][None], sd, nheads, None if prob is None else prob[u].double(),
                              None if branch is None else branch[r][None])[0])
    return torch.cat(outs)


def packed_masks(base, lengths, Dm, nheads, ff, p):
    """dropout_cases.block_masks for a pack: the row-wise masks are the dense ones of ONE utterance of sum_T rows (counter
    m * N + n over the packed rows), the attention mask follows the packed row rule"""
    n = int(sum(lengths))
    s = dc.named_seeds(base)
    masks = {}
    for name, seed in s.items():
        if name == "attn_prob":
            masks[name] = packed_keep(seed, lengths, nheads, p)
        else:
            masks[name] = dc.keep_rows(seed, 1, n, ff if name.endswith("hidden") else Dm, p)[0]
    return masks


def packed_block64(x, sd, lengths, nheads, bn_eval=False, masks=None, stats=None):
    """ConformerBlock on packed rows x [sum_T, D] in the dtype of its inputs (dropout_cases.block64 is this on one utterance)"""
    g = (masks or {}).get
    one = lambda m: None if m is None else m[None]
    x = dc.ffn64(x[None], orc.sub(sd, "ff1"), one(g("ff1_hidden")), one(g("ff1_branch")))[0]
    x = packed_mhsa64(x, orc.sub(sd, "mhsa"), lengths, nheads, g("attn_prob"), g("attn_branch"))
    x = packed_conv64(x, orc.sub(sd, "conv"), lengths, bn_eval, g("conv_branch"), stats)
    x = dc.ffn64(x[None], orc.sub(sd, "ff2"), one(g("ff2_hidden")), one(g("ff2_branch")))[0]
    return orc.layer_norm(x, sd["final_norm.weight"], sd["final_norm.bias"])


@cached
def block_inputs(name):
    """(float32 state dict with moved running statistics, x [sum_T, D], dy [sum_T, D])"""
    n = int(sum(ATTN_SETS[name]))
    sd = hp.width_block_state(D, H, FF, 31, seed=7)
    sd["conv.batch_norm.running_mean"] = hp.arr("pb_rm", (D,), 3) * 0.2
    sd["conv.batch_norm.running_var"] = hp.arr("pb_rv", (D,), 4).abs() * 0.5 + 0.5
    x = hp.width_input(1, n, D, seed=8)[0].contiguous()
    dy = hp.arr("pb_dy", (n, D), 9 + n)
    return sd, x, dy


@cached
def block_case(name, bn_eval):
    """float64 packed block at p = 0 -> dict(out, dx, grads, stats, running)"""
    lengths = ATTN_SETS[name]
    sd, x, dy = block_inputs(name)
    ref = dc.leaves64(sd)
    xr = x.double().clone().requires_grad_(True)
    stats = {}
    y = packed_block64(xr, ref, lengths, H, bn_eval, None, stats)
    y.backward(dy.double())
    grads = {k: v.grad for k, v in ref.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    running = None if bn_eval else dc.running_stats_after(sd, stats)
    return dict(out=y.detach(), dx=xr.grad, grads=grads, stats=stats, running=running)


# ---- SpeechEnhancer on packed rows ----------------------------------------------------------------------------------------------
MODEL_ROW = dict(n_freq=129, d_model=128, num_blocks=2, num_heads=2, d_ff=256, kernel_size=31, p=0.1)
MODEL_LENGTHS = [21, 53, 34, 47, 29]


def model_state():
    return dc.model_state(MODEL_ROW)


CLEAN_GAINS = (0.005, 1.5)


@cached
def model_inputs():
    """(noisy real, noisy imag, clean real, clean imag), each [sum_T, F].  The L1 magnitude term's derivative is the SIGN of
    |enh| - |clean|: an element whose difference lies within the forward's 16-bit error of zero flips it and moves the gradient by
    2 / N whatever the kernels compute (in float64, noise of 3e-4 of the output's RMS on a random clean spectrum moves the
    gradients of this model by 0.7 - 1.5e-2, five times the bound; on this one by 2e-4).  So that the check measures the kernels
    and not that kink, the clean magnitudes are |noisy| x CLEAN_GAINS in a checkerboard over (frame, bin): |enh| = mask |noisy|
    with the mask inside (0.018, 0.981) on this model, so the sign is + on one colour and - on the other, away from zero."""
    n = int(sum(MODEL_LENGTHS))
    shp = (n, MODEL_ROW["n_freq"])
    nr, ni = hp.arr("pm_nr", shp, 41, 0.5), hp.arr("pm_ni", shp, 42, 0.5)
    colour = (torch.arange(shp[0])[:, None] + torch.arange(shp[1])[None, :]) % 2
    gain = torch.where(colour == 0, CLEAN_GAINS[0], CLEAN_GAINS[1])
    return nr, ni, (torch.sqrt(nr * nr + ni * ni) * gain).float(), torch.zeros(shp)


def packed_enhancer64(sd, nr, ni, lengths, nheads, bn_eval=False):
    """dropout_cases.enhancer64 with the blocks on packed rows, p = 0 -> (enh_real, enh_imag, mask_mag)"""
    x = torch.cat([nr, ni], dim=-1)
    x = orc.layer_norm(x, sd["input_norm.weight"], sd["input_norm.bias"])
    x = orc.linear(x, sd["input_proj.weight"], sd["input_proj.bias"])
    for i in range(orc._num_blocks(sd)):
        x = packed_block64(x, orc.sub(sd, "blocks.%d" % i), lengths, nheads, bn_eval)
    x = orc.layer_norm(x, sd["output_norm.weight"], sd["output_norm.bias"])
    mmag = torch.sigmoid(orc.linear(x, sd["mag_head.weight"], sd["mag_head.bias"]))
    mph = torch.tanh(orc.linear(x, sd["phase_head.weight"], sd["phase_head.bias"])) * (math.pi / 6)
    mr, mi = mmag * torch.cos(mph), mmag * torch.sin(mph)
    return mr * nr - mi * ni, mr * ni + mi * nr, mmag


def l1_magnitude64(er, ei, cr, ci):
    """the reference's L1 magnitude term (training/conformer_pipeline.py:562-564)"""
    return (torch.sqrt(er * er + ei * ei + 1e-8) - torch.sqrt(cr * cr + ci * ci + 1e-8)).abs().mean()


@cached
def model_case(bn_eval):
    """float64 packed enhancer, one step on the L1 magnitude term, p = 0 -> dict(out (er, ei, mm), loss, grads)"""
    sd = model_state()
    nr, ni, cr, ci = [t.double() for t in model_inputs()]
    ref = dc.leaves64(sd)
    er, ei, mm = packed_enhancer64(ref, nr, ni, MODEL_LENGTHS, MODEL_ROW["num_heads"], bn_eval)
    assert CLEAN_GAINS[0] < 0.5 * float(mm.detach().min()) and float(mm.detach().max()) < 0.75 * CLEAN_GAINS[1]     # (the sign is away from its kink)
    loss = l1_magnitude64(er, ei, cr, ci)
    loss.backward()
    grads = {k: v.grad for k, v in ref.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    return dict(out=(er.detach(), ei.detach(), mm.detach()), loss=float(loss.detach()), grads=grads)
