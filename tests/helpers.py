"""Shared test helpers: synthetic state_dicts shaped like the reference's
modules (tests/golden/state_shapes.json, captured from the reference) and
golden loaders.  Test-side only."""
import json
import math
import os
import numpy as np
import torch
import torch.nn.functional as _F

from sincformer_metacog_speech_enhancement_amd import synthetic as syn
from oracle import sfm_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "state_shapes.json")) as _fh:
    STATE_TABLES = json.load(_fh)


def gold(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def synth_sd(table, seed, fs=16000, sinc_scale=None, as_torch=True):
    """State dict for reference module `table` filled by synthetic.synth_state_dict."""
    shapes = {k: tuple(v[0]) for k, v in STATE_TABLES[table]["state"].items()}
    keep = None
    sinc_keys = [k for k in shapes if k.split(".")[-1] in ("low_hz_", "band_hz_", "window", "n_")]
    if sinc_keys:
        init = orc.sinc_init(64, 251, fs)
        keep = {k: init[k.split(".")[-1]].numpy() for k in sinc_keys}
    sd = syn.synth_state_dict(shapes, seed, keep=keep, sinc_scale=sinc_scale)
    if as_torch:
        return {k: torch.from_numpy(v) for k, v in sd.items()}
    return sd


def arr(key, shape, seed, scale=1.0):
    return torch.from_numpy(syn.synth_array(key, shape, seed, scale))


def maxerr(a, b):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max())


def rmse(a, b):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float(((a - b) ** 2).mean().sqrt())


# ---------------------------------------------------------------------------
# Attention: the default kernel-selection rule (tests/test_attention_rule_gpu.py on the GPU, tests/test_host_logic.py for
# ops.attention_kernel_name without one).  (B, H, T, kernel) rows at head_dim 64, worked out by hand from the integer rule of
# attention_fwd_impl (csrc/attention.hip): nq = ceil(T / 512); enough = B * H * nq >= 128; the 8-wave pipelined kernel when
# enough and (T >= 1024 or 100 T >= 78 * 512 nq): T 400..512 (39936 <= 100 T), T 799..1023 (79872 <= 100 T); else the 4-wave
# one when enough and T <= 256 and 100 T >= 23040: T 231..256; the 32-rows-per-wave kernel otherwise.  Each row stands on one
# side of one edge of that rule (a T window's end, or 127 / 128 and 88 / 132 items).
# ---------------------------------------------------------------------------
ATTN_KERNELS = {"hd64": "attn_fwd_hd64_kernel", "ring": "attn_fwd_hd64r_kernel", "p8": "attn_fwd_hd64p8_kernel",
                "p4": "attn_fwd_hd64p4_kernel", "q4": "attn_fwd_hd64q4_kernel"}
ATTN_FORCED = {1: "hd64", 2: "ring", 3: "ring", 4: "p8", 5: "p4", 6: "q4"}          # ops.set_attention_variant(v) -> kernel
ATTN_VARIANT_OF = {ATTN_KERNELS[k]: v for v, k in ATTN_FORCED.items() if v != 2}     # kernel name -> the variant that forces it
ATTN_RULE_ROWS = [(32, 4, 230, "hd64"), (32, 4, 231, "p4"), (32, 4, 256, "p4"), (32, 4, 257, "hd64"), (32, 4, 399, "hd64"),
                  (32, 4, 400, "p8"), (32, 4, 512, "p8"), (16, 4, 513, "hd64"), (16, 4, 798, "hd64"), (16, 4, 799, "p8"),
                  (11, 4, 1024, "hd64"), (16, 4, 1024, "p8"), (11, 4, 1025, "p8"), (127, 1, 256, "hd64"), (128, 1, 256, "p4")]


def attn_ref64(qkv, B, T, H, hd, prescaled=False, dO=None, keep=None):
    """float64 attention of qkv [B*T, 3*H*hd] (q | k | v), one utterance at a time (a [H, T, T] score block at most is alive).
    prescaled: q carries log2(e) / sqrt(hd), P = softmax(ln2 * q.k); otherwise P = softmax(q.k / sqrt(hd)).  keep [B, H, T, T]:
    the dropout factor on P.  -> O [B*T, H*hd], log2-domain log-sum-exp of the scaled scores [B, H, T], and - with a cotangent
    dO [B*T, H*hd] - the float64 autograd gradient w.r.t. qkv (else None)"""
    D = H * hd
    x = qkv.double().reshape(B, T, 3 * D)
    scale = math.log(2.0) if prescaled else 1.0 / math.sqrt(hd)
    outs, lses, grads = [], [], []
    for b in range(B):
        xb = x[b].clone().requires_grad_(dO is not None)
        q, k, v = [t.reshape(T, H, hd).transpose(0, 1) for t in xb.split(D, dim=-1)]
        s = (q @ k.transpose(-1, -2)) * scale
        p = torch.softmax(s, dim=-1)
        lses.append((torch.logsumexp(s, dim=-1) / math.log(2.0)).detach())
        if keep is not None:
            p = p * keep[b].double()
        o = (p @ v).transpose(0, 1).reshape(T, D)
        if dO is not None:
            o.backward(dO.double().reshape(B, T, D)[b])
            grads.append(xb.grad)
        outs.append(o.detach())
    return torch.cat(outs), torch.stack(lses), (torch.cat(grads) if dO is not None else None)


def keep_mask(seed, B, H, T, p):
    """numpy replica of the counter-based keep function (attention.hip / attention_bwd.hip): full hash of the probability row
    (b, h, q), then one multiply-add + xorshift-multiply round per key"""
    M32 = np.uint64(0xFFFFFFFF)
    row = np.arange(B * H * T, dtype=np.uint64)
    x = ((row & M32) * np.uint64(0x9E3779B1)) & M32
    x ^= ((row >> np.uint64(32)) * np.uint64(0x85EBCA77)) & M32
    x ^= np.uint64(seed)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    key = np.arange(T, dtype=np.uint64)
    y = (x[:, None] + ((key * np.uint64(0x9E3779B1)) & M32)[None, :]) & M32
    y ^= y >> np.uint64(15); y = (y * np.uint64(0x846CA68B)) & M32
    y ^= y >> np.uint64(16)
    thr = np.uint64(math.ceil(float(np.float32(p)) * 16777216.0))
    keep = ((y >> np.uint64(8)) >= thr).astype(np.float32) / (1.0 - p)
    return torch.from_numpy(keep.reshape(B, H, T, T))


def metric_cases():
    """(name, fs, clean, enhanced) pairs shared by the generator and the tests: plain noisy pairs at both sample rates,
    a silent stretch (skipped frames), identical signals (upper bound), ragged length, shorter-than-a-frame."""
    cases = []
    for i, (fs, L) in enumerate(((8000, 8000), (16000, 12345), (8000, 3001))):
        noisy, clean = syn.synth_wave(1, L, 120 + i)
        cases.append(("pair%d" % i, fs, clean[0], (0.7 * noisy[0] + 0.3 * clean[0]).astype(np.float32)))
    noisy, clean = syn.synth_wave(1, 6000, 125)
    c = clean[0].copy()
    c[2000:3500] = 0.0
    cases.append(("silence", 8000, c, noisy[0]))
    cases.append(("identical", 8000, clean[0], clean[0].copy()))
    cases.append(("short", 8000, clean[0][:100], noisy[0][:100]))
    return cases


def central_difference_along_gradient(params, objective, eps):
    """objective() -> scalar tensor with grad; returns (|g|, central-difference slope of the objective along g / |g|)"""
    total = objective()
    total.backward()
    params = [p_ for p_ in params if p_.grad is not None]
    gnorm = float(torch.sqrt(sum((p_.grad.double() ** 2).sum() for p_ in params)))
    assert math.isfinite(gnorm) and gnorm > 0
    base = [p_.detach().clone() for p_ in params]
    vals = []
    for sign in (1.0, -1.0):
        with torch.no_grad():
            for p_, b0 in zip(params, base):
                p_.copy_(b0 + sign * eps * p_.grad / gnorm)
        vals.append(float(objective().detach()))
    with torch.no_grad():
        for p_, b0 in zip(params, base):
            p_.copy_(b0)
    return float(total.detach()), gnorm, (vals[0] - vals[1]) / (2 * eps)


# ---------------------------------------------------------------------------
# Conformer widths pinned against the oracle (tests/test_widths_gpu.py).  One row per route it is there to exercise;
# tests/test_host_logic.py checks on CPU that the bounds below separate plausible wrong answers at every row.
# train_KS / train_BT: the training-mode check's kernel size and batch x frames (sfm_dwconv_wgrad takes k 7 / 31; w512 trains
# on fewer frames; w256h8 keeps M >= 4096 so the training forward's lin256 routing is covered).
# ---------------------------------------------------------------------------
WIDTH_ROWS = [
    dict(id="w128", D=128, H=2, FF=512, KS=31, BT=(2, 200), train_KS=31, train_BT=(2, 200),
         route="MFMA attention at D 128; un-fused FFN; folded dwconv C 128"),
    dict(id="w192", D=192, H=4, FF=768, KS=15, BT=(2, 150), train_KS=7, train_BT=(2, 150),
         route="generic attention hd 48; LayerNorm D 192; dwconv_bn_swish C 192 k 15"),
    dict(id="w256h8", D=256, H=8, FF=1024, KS=31, BT=(2, 2100), train_KS=31, train_BT=(2, 2100),
         route="ln+lin256, lin256 and ffn_fused_ln with generic attention (hd 32) at T 2100"),
    dict(id="w256h2", D=256, H=2, FF=1000, KS=31, BT=(3, 100), train_KS=31, train_BT=(3, 100),
         route="generic attention hd 128; FF % 64 != 0: un-fused FFN at D 256"),
    dict(id="w384", D=384, H=6, FF=1536, KS=31, BT=(2, 300), train_KS=31, train_BT=(2, 300),
         route="ln_linear16 un-fused fallback at D 384; MFMA attention H 6; LayerNorm D 384; dwconv_bn_swish C 384"),
    dict(id="w512", D=512, H=8, FF=2048, KS=31, BT=(16, 512), train_KS=31, train_BT=(2, 256),
         route="LayerNorm D 512; folded dwconv C 512; pipelined attention kernel at H 8 (B*H*ceil(T/512) = 128)"),
    dict(id="w512h4", D=512, H=4, FF=2048, KS=7, BT=(2, 64), train_KS=7, train_BT=(2, 64),
         route="generic attention hd 128 at D 512; folded dwconv k 7"),
]
# eval: relative RMSE of each module's output vs the float64 oracle.  fp16 as test_conformer_block_full_vs_golden; mixed / bf16
# tighter than its 1.5e-2: measured on the MI355X at most 1.9e-3 (mixed) / 3.7e-3 (bf16) over every row and part (fp16 4.7e-4)
WIDTH_EVAL_TOL = {"fp16": 2e-3, "mixed": 1e-2, "bf16": 1e-2}
WIDTH_QSCALE = 3.0          # Q rows of in_proj scaled up: peaked softmax rows, so the attention branch is far from a time average


def width_block_state(D, H, FF, KS, seed=7):
    """float32 state dict of ConformerBlock(D, H, FF, KS) filled by synthetic.synth_state_dict from the module's own shapes"""
    from sincformer_metacog_speech_enhancement_amd.models.conformer import ConformerBlock
    shapes = {k: tuple(v.shape) for k, v in ConformerBlock(D, H, FF, KS, 0.0).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed).items()}
    sd["mhsa.attention.in_proj_weight"][:D] *= WIDTH_QSCALE
    return sd


def width_input(B, T, D, seed=8):
    """[B, T, D] float32 with per-channel scales 0.7 .. 1.5 and offsets -0.3 .. 0.3 (so row statistics over a subset of the
    columns differ from those over all of them)"""
    z = torch.from_numpy(syn.synth_array("width_x", (B, T, D), seed))
    return (z * torch.linspace(0.7, 1.5, D) + torch.linspace(-0.3, 0.3, D)).float().contiguous()


def rel_rmse(got, ref):
    ref = torch.as_tensor(np.asarray(ref)).double()
    return rmse(got, ref) / max(float(ref.pow(2).mean().sqrt()), 1e-30)


# ---------------------------------------------------------------------------
# float64 restatements of the fp32 nodes of the training path (tests/test_train_nodes_gpu.py).  Each computes in the dtype of
# its inputs: evaluated in float64 it is the reference, evaluated in float32 on the same inputs it gives the row's `e32`, the
# error any fp32 evaluation of the formula carries, from which the row's bound is derived (4 x e32 for sums and products,
# 16 x e32 behind the hardware's exp / rcp / sin / cos / log / sqrt; never from a kernel's output).
# tests/test_host_logic.py pins every restatement to the oracle and checks that the bounds separate plausible wrong kernels.
# ---------------------------------------------------------------------------
K_SUM, K_TRANS = 4.0, 16.0
U32 = 2.0 ** -24


def lstm_dir64(xg, whh, reverse):
    """recurrence of orc._lstm_dir on a given input projection xg [B, T, 4H] (gate order i, f, g, o), whh [4H, H]
    -> out [B, T, H], saved state [B, T, 5, H] = activated i, f, g, o and the cell state c of every step"""
    B, T, G = xg.shape
    H = G // 4
    h, c = xg.new_zeros(B, H), xg.new_zeros(B, H)
    outs, saves = [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = xg[:, t] + h @ whh.t()
        i, f, gg, o = g.split(H, dim=-1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        outs[t], saves[t] = h, torch.stack([i, f, gg, o, c], dim=1)
    return torch.stack(outs, dim=1), torch.stack(saves, dim=1)


def bilstm64(xg, whh):
    """xg [B, T, 2, 4H], whh [2, 4H, H] -> out [B, T, 2H], saved state [B, T, 2, 5, H] (the kernel's layout)"""
    of, sf = lstm_dir64(xg[:, :, 0], whh[0], False)
    orv, sr = lstm_dir64(xg[:, :, 1], whh[1], True)
    return torch.cat([of, orv], dim=-1), torch.stack([sf, sr], dim=2)


def bptt64(save, whh, dout, reverse, mutant=None):
    """gradient w.r.t. xg [B, T, 4H] of one direction from its saved state [B, T, 5, H] and dout [B, T, H]: the hand-written
    adjoint of lstm_dir64 (equal to its autograd; test_host_logic).  mutant: a plausible wrong form of the walk."""
    B, T, _, H = save.shape
    chain = list(range(T - 1, -1, -1) if reverse else range(T))
    if mutant == "reverse chain walked in forward order":
        chain = list(range(T))
    dxg = save.new_zeros(B, T, 4 * H)
    dh_rec, dc_next = save.new_zeros(B, H), save.new_zeros(B, H)
    for s in range(T - 1, -1, -1):
        t = chain[s]
        i, f, g, o, c = save[:, t].unbind(dim=1)
        cp = save[:, chain[s - 1], 4] if s > 0 else torch.zeros_like(c)
        dh = dout[:, t] + dh_rec
        if mutant == "recurrent term dropped at the chain's first step" and s == 0:
            dh = dout[:, t]
        tc = torch.tanh(c)
        dc = dh * o * (1 - tc * tc) + dc_next
        da = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=-1)
        dxg[:, t] = da
        dc_next = dc * f
        if mutant == "f[t] in place of f[t+1] in the cell-gradient carry" and s > 0:
            dc_next = dc * save[:, chain[s - 1], 1]
        dh_rec = da @ whh
    return dxg


BPTT_MUTANTS = ("f[t] in place of f[t+1] in the cell-gradient carry", "recurrent term dropped at the chain's first step",
                "reverse chain walked in forward order")


def frame64(wave, n_fft, hop, win):
    """reflect-pad by n_fft/2, cut `win` samples at offset (n_fft - win)/2 every `hop`: [B, L] -> [B, 1 + L // hop, win]"""
    B, L = wave.shape
    pad, woff = n_fft // 2, (n_fft - win) // 2
    xp = _F.pad(wave.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    idx = torch.arange(1 + L // hop).unsqueeze(1) * hop + woff + torch.arange(win).unsqueeze(0)
    return xp[:, idx]


def frame_adjoint(frames, L, n_fft, hop, win):
    """torch autograd of frame64 on the cotangent `frames` [B, T, win] -> [B, L], in the dtype of `frames`"""
    x = torch.zeros(frames.shape[0], L, dtype=frames.dtype, requires_grad=True)
    (frame64(x, n_fft, hop, win) * frames).sum().backward()
    return x.grad


OLA_MUTANTS = ("left reflected image dropped", "right image mirrored about L", "s == n_fft/2 left out of the left image",
               "window offset ignored", "post applied before the accumulate")


def adjoint_ola64(frames, L, n_fft, hop, win, mutant=None):
    """the same adjoint in closed form (overlap-add in the padded signal, then the two reflected images folded in)"""
    B, T, _ = frames.shape
    pad, woff = n_fft // 2, (n_fft - win) // 2
    if mutant == "window offset ignored":
        woff = 0
    ola = frames.new_zeros(B, L + 2 * pad + 2)
    pos = (torch.arange(T).unsqueeze(1) * hop + woff + torch.arange(win).unsqueeze(0)).reshape(-1)
    ola.index_add_(1, pos, frames.reshape(B, -1))
    s = torch.arange(L)
    out = ola[:, pad + s].clone()
    left = (s >= 1) & (s <= pad)
    if mutant == "s == n_fft/2 left out of the left image":
        left = (s >= 1) & (s < pad)
    if mutant != "left reflected image dropped":
        out[:, left] += ola[:, pad - s[left]]
    if mutant == "right image mirrored about L":
        right = (s >= L - pad + 1) & (s <= L - 1)
        out[:, right] += ola[:, pad + 2 * L - s[right]]
    else:
        right = (s >= L - 1 - pad) & (s <= L - 2)
        out[:, right] += ola[:, pad + 2 * (L - 1) - s[right]]
    return out


def ola_finish(adj, prev, post, mutant=None):
    """what sfm_stft_adjoint_ola leaves in dwave: (prev + adjoint) * post"""
    if mutant == "post applied before the accumulate" and post is not None and prev is not None:
        return prev + adj * post
    v = adj if prev is None else prev + adj
    return v if post is None else v * post


def sisnr64(est, tgt, mutant=None):
    """orc.si_snr_loss in the dtype of its inputs"""
    if mutant != "no mean removal":
        tgt = tgt - tgt.mean(dim=-1, keepdim=True)
        est = est - est.mean(dim=-1, keepdim=True)
    dot = (est * tgt).sum(dim=-1, keepdim=True)
    s_energy = (tgt ** 2).sum(dim=-1, keepdim=True) + 1e-8
    s_target = dot * tgt / s_energy
    e_noise = est - s_target
    si = 10 * torch.log10((s_target ** 2).sum(dim=-1) / ((e_noise ** 2).sum(dim=-1) + 1e-8) + 1e-8)
    return -si.sum() if mutant == "1/B missing" else -si.mean()


SISNR_MUTANTS = ("no mean removal", "1/B missing")
SPEC_MUTANTS = {0: ("element count off by one row", "1e-8 inside the square root", "sign term non-zero at P = T"),
                1: ("element count off by one row", "sign term non-zero at P = T")}


def spec_terms64(pr, pi, tr, ti, mode, mutant=None):
    """mode 0: spectral convergence + mean |log-magnitude difference| of one resolution, as orc.mr_stft_loss writes them;
    mode 1: the L1 magnitude term of orc.spectrum_objective.  The magnitude is torch.abs of the complex bin: the same value as
    the oracle's sqrt(re^2 + im^2), with the reference's zero gradient at a bin that is exactly 0 + 0j."""
    n = pr.numel()
    if mutant == "element count off by one row":
        n = n + pr.shape[-1]
    if mode == 0:
        pm, tm = torch.abs(torch.complex(pr, pi)), torch.abs(torch.complex(tr, ti))
        sc = torch.linalg.norm((tm - pm).reshape(-1)) / (torch.linalg.norm(tm.reshape(-1)) + 1e-8)
        if mutant == "1e-8 inside the square root":
            d = torch.log(torch.sqrt(pr ** 2 + pi ** 2 + 1e-8)) - torch.log(torch.sqrt(tr ** 2 + ti ** 2 + 1e-8))
        else:
            d = torch.log(pm + 1e-8) - torch.log(tm + 1e-8)
    else:
        sc = 0.0
        d = torch.sqrt(pr ** 2 + pi ** 2 + 1e-8) - torch.sqrt(tr ** 2 + ti ** 2 + 1e-8)
    if mutant == "sign term non-zero at P = T":                  # sign(0) = +1: the slope of d where d is exactly zero
        return sc + (d.abs().sum() + torch.where(d.detach() == 0, d, torch.zeros_like(d)).sum()) / n
    return sc + d.abs().sum() / n


def finalize64(Sw, Sm, Sr, nr, B, L, n_mag, R, dtype=torch.float64):
    """[total, neg SI-SNR, L1 magnitude, MR-STFT] from the reductions of the objective (wave moments [B, 5], magnitude sums [4],
    per-resolution sums [R, 4] with element counts nr [R]): si_snr_loss / mr_stft_loss / spectrum_objective in terms of sums"""
    Sw, Sm, Sr = Sw.to(dtype), Sm.to(dtype), Sr.to(dtype)
    me, mt = Sw[:, 0] / L, Sw[:, 1] / L
    Et, Ee, dot = Sw[:, 3] - L * mt * mt, Sw[:, 2] - L * me * me, Sw[:, 4] - L * me * mt
    k = dot / (Et + 1e-8)
    star, noise = k * k * Et, Ee - 2.0 * k * dot + k * k * Et
    neg = -(10.0 * torch.log10(star / (noise + 1e-8) + 1e-8)).sum() / B
    l1 = Sm[3] / n_mag
    mr = torch.zeros((), dtype=dtype)
    for r in range(R):
        mr = mr + torch.sqrt(Sr[r, 0]) / (torch.sqrt(Sr[r, 1]) + 1e-8) + Sr[r, 2] / float(nr[r])
    mr = mr / max(R, 1)
    return torch.stack([neg + 0.5 * l1 + mr, neg, l1, mr])


POLAR_MUTANTS = ("bias row of the neighbouring utterance", "one factor phase_scale missing", "conjugate sign wrong")


def polar64(lm, lp, bias, nr, ni, phase_scale, mutant=None):
    """bounded polar mask (agents/msa.py:166-172 as orc.msa_forward writes it) and its product with the noisy spectrum
    (orc.apply_mask): lm, lp [B, T, F] logits, bias [B, F] or None, nr / ni [B, T, F] or None (the mask itself)"""
    if bias is not None:
        if mutant == "bias row of the neighbouring utterance":
            bias = torch.roll(bias, 1, dims=0)
        lm = lm + bias.unsqueeze(1)
    mg = torch.sigmoid(lm)
    th = torch.tanh(lp)
    ph = th * phase_scale
    if mutant == "one factor phase_scale missing":              # same value, slope without the factor
        ph = ph.detach() + (th - th.detach())
    mr, mi = mg * torch.cos(ph), mg * torch.sin(ph)
    if nr is None:
        return mr, mi
    if mutant == "conjugate sign wrong":                         # gradient = g x noisy instead of g x conj(noisy)
        ni = -ni
    return mr * nr - mi * ni, mr * ni + mi * nr


def istft64(real, imag, length, n_fft, hop, win, absolute=False):
    """orc.istft in the dtype of its inputs (twiddles formed in float64, then cast).  absolute: with |coefficients|, so that
    non-negative inputs give the sum of |terms| of every output sample"""
    B, T, Fq = real.shape
    dt = real.dtype
    w = orc._padded_window(n_fft, win)
    n = torch.arange(n_fft, dtype=torch.float64).unsqueeze(0)
    f = torch.arange(Fq, dtype=torch.float64).unsqueeze(1)
    ang = 2.0 * math.pi * ((f * n) % n_fft) / n_fft
    coef = torch.full((Fq, 1), 2.0, dtype=torch.float64)
    coef[0, 0] = 1.0
    coef[Fq - 1, 0] = 1.0
    br = coef * torch.cos(ang) / n_fft * w.unsqueeze(0)
    bi = -coef * torch.sin(ang) / n_fft * w.unsqueeze(0)
    bi[0, :] = 0.0
    bi[Fq - 1, :] = 0.0
    if absolute:
        br, bi = br.abs(), bi.abs()
    frames = real @ br.to(dt) + imag @ bi.to(dt)
    full = n_fft + hop * (T - 1)
    env = torch.zeros(full, dtype=torch.float64)
    y = real.new_zeros(B, full)
    for t in range(T):
        y = y + _F.pad(frames[:, t], (t * hop, full - n_fft - t * hop))
        env[t * hop:t * hop + n_fft] += w * w
    start = n_fft // 2
    return y[:, start:start + length] / env[start:start + length].to(dt)


def dft64(frames, n_fft, win):
    """windowed one-sided DFT of frames [B, T, win] cut by frame64 -> real, imag [B, T, n_fft/2 + 1]"""
    woff = (n_fft - win) // 2
    n = (torch.arange(win, dtype=torch.float64) + woff).unsqueeze(1)
    f = torch.arange(n_fft // 2 + 1, dtype=torch.float64).unsqueeze(0)
    ang = 2.0 * math.pi * ((n * f) % n_fft) / n_fft
    w = orc.hann_periodic(win).unsqueeze(1)
    return frames @ (w * torch.cos(ang)).to(frames.dtype), frames @ (-w * torch.sin(ang)).to(frames.dtype)


def hprev_ref(h, B, T, H, dtype, mutant=None):
    """previous output of each chain: [B, T, 2H] fp32 -> [B*T, 2H] rounded by tensor.to(dtype); forward half h[t-1] (0 at
    t = 0), reverse half h[t+1] (0 at t = T-1)"""
    out = torch.zeros_like(h)
    if mutant == "no zero at an utterance boundary":
        flat = h.reshape(B * T, 2 * H)
        o = torch.zeros_like(flat)
        o[1:, :H] = flat[:-1, :H]
        o[:-1, H:] = flat[1:, H:]
        return o.to(dtype)
    out[:, 1:, :H] = h[:, :-1, :H]
    if mutant == "reverse half shifted like the forward half":
        out[:, 1:, H:] = h[:, :-1, H:]
    else:
        out[:, :-1, H:] = h[:, 1:, H:]
    return out.reshape(B * T, 2 * H).to(dtype)


def time_reduce(x, mean, mutant=None):
    """sum / mean over the frames of x [B, T, C] in its dtype"""
    T = x.shape[1]
    if mutant == "last partial chunk of 64 dropped":
        x = x[:, :T - T % 64]
    s = x.sum(dim=1)
    if not mean:
        return s
    return s / ((T + 63) // 64 * 64 if mutant == "division by the padded length" else T)


# (B, T, H): T 1 and 2, B >= 3 (a shift across an utterance boundary shows), 3 x 21846 rows > 65536
HPREV_ROWS = [(3, 1, 32), (3, 2, 64), (4, 5, 128), (3, 7, 32), (5, 2, 128), (3, 21846, 128)]
HPREV_MUTANTS = ("reverse half shifted like the forward half", "no zero at an utterance boundary")


def hprev_case(row):
    B, T, H = row
    return arr("hp_h", (B, T, 2 * H), T + H) * 0.5


TIME_MUTANTS = ("last partial chunk of 64 dropped", "division by the padded length")


# ---- figures and bounds ----
def figs(got, ref):
    """(relative RMSE, max |err| / max |ref|) over ALL elements"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    d = got - ref
    return (float(d.pow(2).mean().sqrt()) / max(float(ref.pow(2).mean().sqrt()), 1e-300),
            float(d.abs().max()) / max(float(ref.abs().max()), 1e-300))


def row_bound(ref64, ref32, k, sum_bound=None):
    """(e32, bound), each as (relative RMSE, max/max): bound = k x e32, or - where it is larger - the figures of `sum_bound`,
    the elementwise n 2^-24 sum|terms| forward bound of an fp32 sum in any order, formed from the reference's own terms"""
    e32 = figs(ref32, ref64)
    b = [k * e32[0], k * e32[1]]
    if sum_bound is not None:
        r = ref64.detach().double()
        b[0] = max(b[0], float(sum_bound.double().pow(2).mean().sqrt()) / max(float(r.pow(2).mean().sqrt()), 1e-300))
        b[1] = max(b[1], float(sum_bound.double().abs().max()) / max(float(r.abs().max()), 1e-300))
    return e32, tuple(b)


def check_row(name, got, ref64, ref32, k, sum_bound=None, slices=None, unit="e32"):
    """print e32 / bound / observed of a row (and of each named slice of it) and assert observed <= bound on every one
    (unit: what `ref32` is when it is not the float32 evaluation, e.g. the reference under the forward's allowed error)"""
    parts = {"all": lambda t: t}
    parts.update(slices or {})
    bad = []
    for pname, cut in parts.items():
        r64 = cut(ref64)
        if r64.numel() == 0:
            continue
        e32, b = row_bound(r64, cut(ref32), k, None if sum_bound is None else cut(sum_bound))
        o = figs(cut(torch.as_tensor(got).detach().cpu()), r64)
        print("ROW | %s | %s | %s %.2e %.2e | bound %.2e %.2e | observed %.2e %.2e" % (name, pname, unit, e32[0], e32[1], b[0], b[1],
                                                                                         o[0], o[1]))
        if not (math.isfinite(o[0]) and o[0] <= b[0] and o[1] <= b[1]):
            bad.append((pname, o, b))
    assert not bad, (name, bad)


def separates(name, mutant, wrong64, ref64, ref32, k, sum_bound=None, slices=None):
    """a wrong form must move the reference by >= 5 x the bound on at least one slice the GPU row checks"""
    parts = {"all": lambda t: t}
    parts.update(slices or {})
    best = 0.0
    for pname, cut in parts.items():
        r64 = cut(ref64)
        if r64.numel() == 0:
            continue
        _, b = row_bound(r64, cut(ref32), k, None if sum_bound is None else cut(sum_bound))
        m = figs(cut(wrong64), r64)
        best = max(best, min(m[0] / max(b[0], 1e-300), m[1] / max(b[1], 1e-300)))
    print("MUTANT | %s | %s | moves the reference by %.1f x the bound" % (name, mutant, best))
    assert best >= 5.0, (name, mutant, best)


# ---- the rows: inputs (fp32 values), the float64 reference and the float32 evaluation of the same restatement ----
def _grad(fn, *xs):
    xs = [x.clone().requires_grad_(True) for x in xs]
    fn(*xs).backward()
    return [x.grad for x in xs]


def ola_rows():
    """(B, L, n_fft, hop, win, accumulate, post): the four resolutions of the path x ordinary, ragged, short (L < n_fft) and
    minimal (L = n_fft/2 + 1) lengths; accumulate / post / B cycle so that each value meets each resolution"""
    rows, i = [], 0
    for nf, hp, wn, Ls in ((256, 80, 160, (1600, 1637, 479, 4321, 129)), (256, 64, 256, (1600, 1637, 479, 4321, 129)),
                           (512, 128, 512, (1600, 1637, 479, 4321, 257)), (1024, 256, 1024, (1600, 1637, 4321, 600, 513))):
        for L in Ls:
            rows.append((3 if i % 3 else 1, L, nf, hp, wn, i % 2 == 0, (i // 2) % 2 == 0))
            i += 1
        i += 1
    return rows


def ola_case(row):
    B, L, nf, hp, wn, acc, post = row
    T = 1 + L // hp
    frames = arr("ola_f", (B, T, wn), L + nf)
    prev = arr("ola_p", (B, L), L + 1) if acc else None
    pst = (arr("ola_q", (L,), L + 2).abs() + 0.5) if post else None
    up = lambda t, dt: None if t is None else t.to(dt)
    ev = lambda dt, mutant=None: ola_finish(adjoint_ola64(frames.to(dt), L, nf, hp, wn, mutant), up(prev, dt), up(pst, dt), mutant)
    ref64 = ola_finish(frame_adjoint(frames.double(), L, nf, hp, wn), up(prev, torch.float64), up(pst, torch.float64))
    ref32 = ola_finish(frame_adjoint(frames, L, nf, hp, wn), prev, pst)
    nterm = 3 * (-(-wn // hp)) + 2
    mag = ola_finish(frame_adjoint(frames.double().abs(), L, nf, hp, wn), None if prev is None else prev.double().abs(),
                     up(pst, torch.float64))
    pad = nf // 2
    sl = {"first n_fft/2": lambda t: t[..., :pad], "last n_fft/2": lambda t: t[..., max(L - pad, pad):],
          "interior": lambda t: t[..., pad:max(L - pad, pad)]}
    return dict(frames=frames, prev=prev, post=pst, T=T, ref64=ref64, ref32=ref32, sum_bound=nterm * U32 * mag, slices=sl, ev=ev)


SISNR_ROWS = [(3, 4321, 0.37), (1, 4321, 1.0), (3, 70001, 1.0), (1, 70001, 2.5)]          # (B, L, scale); 70001 > 256 x 256


def sisnr_case(row):
    B, L, scale = row
    off = torch.arange(B, dtype=torch.float32).unsqueeze(1)
    tgt = arr("si_t", (B, L), L) * 0.1 + 0.05 + 0.01 * off                    # DC offsets, different on estimate and target
    est = (0.8 * tgt + arr("si_e", (B, L), L + 1) * 0.05 - 0.08 - 0.02 * off).float()
    ev = lambda dt, mutant=None: _grad(lambda e: scale * sisnr64(e, tgt.to(dt), mutant), est.to(dt))[0]
    return dict(est=est, tgt=tgt, ref64=ev(torch.float64), ref32=ev(torch.float32), ev=ev)


# (M, F, mode, padded rows (ld = round_up(2F, 8)) or two [M, F] planes, accumulate, scale); 32600 x 129 > 16384 x 256
SPEC_ROWS = [(300, 129, 0, True, False, 1.0 / 3.0), (300, 129, 0, False, True, 1.0), (300, 129, 1, False, True, 0.5),
             (300, 129, 1, True, False, 1.0), (100, 257, 0, True, True, 1.7), (32600, 129, 0, True, False, 1.0 / 3.0),
             (32600, 129, 1, False, True, 0.5)]


def spec_case(row):
    """P from T by a magnitude ratio in [0.5, 0.9] or [1.1, 1.7] and a small phase turn (the sign terms are unambiguous); ~5 % of
    the bins scaled by 1e-4 (the 1e-8 terms matter there); row 0: P = 0 + 0j, row 1: P = T exactly"""
    M, F, mode, padded, acc, scale = row
    z = [arr("sp%d" % i, (M, F), 11 + i + M).double() for i in range(5)]
    small = z[4].abs() > 1.96
    t = torch.complex(z[0], z[1]) * torch.where(small, 1e-4, 1.0)
    u = z[2].abs().clamp(max=2.0)
    ratio = torch.where(z[2] > 0, 1.1 + 0.3 * u, 0.9 - 0.2 * u)
    p = t * ratio * torch.exp(1j * 0.1 * z[3])
    p[0] = 0
    p[1] = t[1]
    tr, ti, pr, pi = t.real.float(), t.imag.float(), p.real.float(), p.imag.float()
    pr[1], pi[1] = tr[1], ti[1]
    prev = None

    def ev(dt, mutant=None):
        g = _grad(lambda a, b: scale * spec_terms64(a, b, tr.to(dt), ti.to(dt), mode, mutant), pr.to(dt), pi.to(dt))
        if prev is not None:
            g = [prev[i].to(dt) + g[i] for i in range(2)]
        return torch.stack(g)                                            # [2, M, F]: d / d real, d / d imag
    if acc:                                                          # what is already in the buffers: of the gradient's own size
        rms = float(ev(torch.float64).pow(2).mean().sqrt())
        prev = [(arr("sp_prev%d" % i, (M, F), 17 + i) * rms).float() for i in range(2)]
    ordinary = ~small
    ordinary[:2] = False
    sl = {"ordinary bins": lambda t_: t_[..., ordinary]}
    return dict(pr=pr, pi=pi, tr=tr, ti=ti, prev=prev, ref64=ev(torch.float64), ref32=ev(torch.float32), ev=ev, slices=sl)


# (B, T, F, noisy spectrum, bias, layout of the logits): merged [M, 2F], split planes, merged rows with ld_logits > 2F
POLAR_ROWS = [(3, 50, 129, True, False, "merged"), (3, 50, 129, False, True, "strided"), (4, 37, 129, True, True, "split"),
              (3, 41, 257, False, False, "split"), (3, 10867, 129, True, True, "merged")]    # 3 x 10867 x 129 > 16384 x 256
PHASE_SCALE = 3.14159 / 8.0


def polar_case(row):
    B, T, F, noisy, bias, layout = row
    lm = (arr("po_m", (B, T, F), 3 + T) * 4.0).clamp(-12.0, 12.0)             # saturated sigmoid / tanh at the ends
    lp = (arr("po_p", (B, T, F), 4 + T) * 4.0).clamp(-12.0, 12.0)
    lm[0, 0, :4] = torch.tensor([12.0, -12.0, 12.0, -12.0])
    lp[0, 0, :4] = torch.tensor([12.0, 12.0, -12.0, -12.0])
    bs = (arr("po_b", (B, F), 5 + T) + torch.arange(B, dtype=torch.float32).unsqueeze(1) - 1.0) if bias else None
    nr, ni = (arr("po_r", (B, T, F), 6 + T), arr("po_i", (B, T, F), 7 + T)) if noisy else (None, None)
    gr, gi = arr("po_gr", (B, T, F), 8 + T), arr("po_gi", (B, T, F), 9 + T)
    up = lambda t, dt: None if t is None else t.to(dt)

    def ev(dt, mutant=None, forward=False):
        xs = [lm.to(dt).clone().requires_grad_(True), lp.to(dt).clone().requires_grad_(True)]
        b = None if bs is None else bs.to(dt).clone().requires_grad_(True)
        er, ei = polar64(xs[0], xs[1], b, up(nr, dt), up(ni, dt), PHASE_SCALE, mutant)
        if forward:
            return torch.stack([er.detach(), ei.detach()])
        ((er * gr.to(dt)).sum() + (ei * gi.to(dt)).sum()).backward()
        return torch.stack([xs[0].grad, xs[1].grad]), (None if b is None else b.grad)
    g64, db64 = ev(torch.float64)
    g32, db32 = ev(torch.float32)
    return dict(lm=lm, lp=lp, bias=bs, nr=nr, ni=ni, gr=gr, gi=gi, ref64=g64, ref32=g32, db64=db64, db32=db32, ev=ev,
                fwd64=ev(torch.float64, forward=True), fwd32=ev(torch.float32, forward=True))


TIME_ROWS = [(3, T, C, C + pad) for T in (1, 63, 64, 65, 801) for C, pad in ((129, 7), (256, 8), (260, 4))]


def time_case(row):
    B, T, C, ld = row
    return arr("tm_x", (B, T, ld), T + C) + 0.3


def time_sum_bound(x64, mean):
    T = x64.shape[1]
    return (T + 1) * U32 * x64.abs().sum(dim=1) / (T if mean else 1)


BPTT_ROWS = [(2, 801, 128), (300, 9, 128), (1, 1, 128), (3, 40, 64), (2, 17, 32)]
_bptt_cache = {}


def bptt_case(row):
    """inputs, float64 forward (saved state) and the float64 / float32 autograd gradient w.r.t. the input projection"""
    if row in _bptt_cache:
        return _bptt_cache[row]
    B, T, H = row
    xg = arr("bp_x", (B, T, 2, 4 * H), T + H)
    whh = arr("bp_w", (2, 4 * H, H), T + H + 1) / H ** 0.5
    dout = arr("bp_d", (B, T, 2 * H), T + H + 2)

    def ev(dt):
        x = xg.to(dt).clone().requires_grad_(True)
        out, save = bilstm64(x, whh.to(dt))
        (out * dout.to(dt)).sum().backward()
        return x.grad, save.detach(), out.detach()
    g64, save64, out64 = ev(torch.float64)
    g32 = ev(torch.float32)[0]
    first = lambda t: torch.stack([t[:, 0, 0], t[:, T - 1, 1]])          # first step of each chain (forward t = 0, reverse t = T-1)
    last = lambda t: torch.stack([t[:, T - 1, 0], t[:, 0, 1]])
    sl = {"forward direction": lambda t: t[:, :, 0], "reverse direction": lambda t: t[:, :, 1], "first step of each chain": first,
          "last step of each chain": last}
    c = dict(xg=xg, whh=whh, dout=dout, ref64=g64, ref32=g32, save64=save64, out64=out64, slices=sl)
    _bptt_cache[row] = c
    return c


def bptt_from_save(save, whh, dout, mutant=None):
    """[B, T, 2, 4H] gradient of both directions from a saved state [B, T, 2, 5, H] (float64)"""
    H = whh.shape[-1]
    return torch.stack([bptt64(save[:, :, d], whh[d], dout[..., d * H:(d + 1) * H], bool(d), mutant) for d in range(2)], dim=2)


def bptt_forward_error_bound(case, amplitude, seed=0):
    """arm B (the kernel's own forward feeds its BPTT): how far the float64 gradient moves when the float64 saved state is
    perturbed by uniform noise of the amplitude the suite allows the forward; the bound is twice that, per slice"""
    g = torch.Generator().manual_seed(seed)
    s = case["save64"]
    noisy = s + (torch.rand(s.shape, generator=g, dtype=torch.float64) * 2 - 1) * amplitude
    return bptt_from_save(noisy, case["whh"].double(), case["dout"].double())


# ---------------------------------------------------------------------------
# ConvolutionModule: BatchNorm and depthwise nodes of train._conv_fwd / _conv_bwd
# ---------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BN_STATS_MUTANTS = ("variance from one-pass fp32 sums of y and y^2 in 128-row blocks",)
BN_FINALIZE_MUTANTS = ("biased variance in the running update", "momentum applied to the old value")
BN_BWD_MUTANTS = ("eval mode keeps the batch-statistics correction", "the S1/M xhat correction dropped", "dgamma and dbeta swapped")
DWCONV_MUTANTS = ("x of the neighbouring utterance read across a batch boundary", "taps mirrored")
DWGRAD_MUTANTS = DWCONV_MUTANTS + ("halo frames outside a span taken as zero",
                                   "last chunk of partials dropped at the second reduce level")


def seq_sum(t):
    """sum over dim 0 accumulated row by row in the dtype of t (numpy's cumsum; torch's CPU cumsum and sum accumulate float32 in
    a wider type or pairwise, and give an e32 near 3e-8 that no fp32 reduction over thousands of rows can meet)"""
    a = t.detach().numpy()
    return torch.from_numpy(np.cumsum(a, axis=0, dtype=a.dtype)[-1].copy())


def bn_stats64(y, mutant=None):
    """mean and biased variance of y [M, C] over its rows as nn.BatchNorm1d forms them: two passes, mean first, then the mean of
    (y - mean)^2; each pass a sequential row-order accumulation in the dtype of y"""
    M = y.shape[0]
    if mutant == BN_STATS_MUTANTS[0]:                            # fp32 whatever the input: this IS the rounding
        a = y.float().numpy()
        pad = (-M) % 128
        a = np.concatenate([a, np.zeros((pad, a.shape[1]), np.float32)]).reshape(-1, 128, a.shape[1])
        s0 = np.cumsum(np.cumsum(a, axis=1, dtype=np.float32)[:, -1], axis=0, dtype=np.float32)[-1]
        s1 = np.cumsum(np.cumsum(a * a, axis=1, dtype=np.float32)[:, -1], axis=0, dtype=np.float32)[-1]
        mu = s0 / np.float32(M)
        var = np.maximum(s1 / np.float32(M) - mu * mu, np.float32(0))
        return torch.from_numpy(mu).to(y.dtype), torch.from_numpy(var).to(y.dtype)
    mean = seq_sum(y) / M
    d = y - mean
    return mean, seq_sum(d * d) / M


def bn_finalize64(y, gamma, beta, run_mean, run_var, eps, momentum, eval_mode, mutant=None, stats=None):
    """-> mean, rstd, sc = gamma rstd, sh = beta - mean sc, running mean, running variance (nn.BatchNorm1d: the running
    variance takes the unbiased batch variance M / (M - 1)); eval mode: mean / var are the running statistics, nothing moves"""
    M = y.shape[0]
    if eval_mode:
        mean, var, rm, rv = run_mean, run_var, run_mean, run_var
    else:
        mean, var = stats if stats is not None else bn_stats64(y)
        unb = var if mutant == BN_FINALIZE_MUTANTS[0] else var * (M / (M - 1.0))
        if mutant == BN_FINALIZE_MUTANTS[1]:
            rm, rv = momentum * run_mean + (1 - momentum) * mean, momentum * run_var + (1 - momentum) * unb
        else:
            rm, rv = (1 - momentum) * run_mean + momentum * mean, (1 - momentum) * run_var + momentum * unb
    rstd = torch.rsqrt(var + eps)
    sc = gamma * rstd
    return mean, rstd, sc, beta - mean * sc, rm, rv


def bn_swish64(y, mean, rstd, gamma, beta):
    """Swish(BatchNorm(y)) from given statistics"""
    t = (y - mean) * rstd * gamma + beta
    return t * torch.sigmoid(t)


def bn_swish_bwd64(g, y, mean, rstd, gamma, beta, eval_mode, mutant=None):
    """-> dy, dgamma, dbeta for the cotangent g of bn_swish64; training: mean / rstd are the batch statistics of y, so dy
    carries their gradient (equal to autograd of the forward; test_host_logic)"""
    M = y.shape[0]
    xh = (y - mean) * rstd
    t = xh * gamma + beta
    sg = torch.sigmoid(t)
    dt = g * sg * (1 + t * (1 - sg))
    dbeta, dgamma = seq_sum(dt), seq_sum(dt * xh)
    if eval_mode and mutant != BN_BWD_MUTANTS[0]:
        dy = gamma * rstd * dt
    elif mutant == BN_BWD_MUTANTS[1]:
        dy = gamma * rstd * (dt - dbeta / M)
    else:
        dy = gamma * rstd * (dt - dbeta / M - xh * (dgamma / M))
    return (dy, dbeta, dgamma) if mutant == BN_BWD_MUTANTS[2] else (dy, dgamma, dbeta)


def _dw_pad(x, KS, mutant=None):
    B, T, C = x.shape
    pad = (KS - 1) // 2
    if mutant == DWCONV_MUTANTS[0]:                               # one long utterance: the edges see the neighbours
        flat = _F.pad(x.reshape(1, B * T, C), (0, 0, pad, pad))[0]
        return torch.stack([flat[b * T:b * T + T + 2 * pad] for b in range(B)])
    return _F.pad(x, (0, 0, pad, pad))


def dwconv64(x, w, bias, mutant=None):
    """depthwise conv over time, channels last: x [B, T, C], w [C, KS], bias [C] -> [B, T, C], zero edges per utterance"""
    B, T, C = x.shape
    KS = w.shape[1]
    xp = _dw_pad(x, KS, mutant)
    if mutant == DWCONV_MUTANTS[1]:
        w = torch.flip(w, dims=[1])
    out = xp.new_zeros(B, T, C) + bias
    for k in range(KS):
        out = out + xp[:, k:k + T] * w[:, k]
    return out


def dwgrad_spans(B, T, nparts):
    """the (utterance, first frame, end frame) of each partial, in the kernel's order"""
    ny = nparts // B
    span = -(-T // ny)
    return [(b, s * span, min(T, (s + 1) * span)) for b in range(B) for s in range(ny)]


def dwconv_wgrad64(x, dy, KS, mutant=None, nparts=None):
    """dw [C, KS], db [C] of dwconv64 for the cotangent dy; with mutant (and the row's partial count) a wrong form of the
    kernel's span / partial structure"""
    B, T, C = x.shape
    pad = (KS - 1) // 2
    xp = _dw_pad(x, KS, mutant if mutant == DWCONV_MUTANTS[0] else None)
    parts = [(0, 0, T)] if mutant not in DWGRAD_MUTANTS[2:] else dwgrad_spans(B, T, nparts)
    if mutant == DWGRAD_MUTANTS[3]:
        n1 = -(-len(parts) // 32)
        parts = parts[:32 * (n1 - 1)]
    dw, db = x.new_zeros(C, KS), x.new_zeros(C)
    for b, t0, t1 in parts:
        sel = slice(None) if mutant not in DWGRAD_MUTANTS[2:] else slice(b, b + 1)
        g, xs = dy[sel, t0:t1], xp[sel]
        if mutant == DWGRAD_MUTANTS[2]:
            xs = xs.clone()
            xs[:, :t0 + pad] = 0
            xs[:, t1 + pad:] = 0
        db = db + g.sum(dim=(0, 1))
        dw = dw + torch.stack([(g * xs[:, t0 + k:t1 + k]).sum(dim=(0, 1)) for k in range(KS)], dim=1)
    return (torch.flip(dw, dims=[1]) if mutant == DWCONV_MUTANTS[1] else dw), db


# (M, C, mean / std): 2 = the smallest batch nn.BatchNorm1d trains on; 129 = one row past a 128-row block of the vector route
# (C 256: 4 row lanes, C 64: 16, C 512: 2); C 192 / 384 take the scalar route (256-row blocks); 4101 rows = 33 partials, 20011 = 79
COLSTAT_ROWS = [(2, 256, 0), (129, 256, 0), (129, 256, 8), (129, 256, 64), (257, 192, 0), (257, 192, 8), (257, 192, 64),
                (300, 64, 1), (4101, 512, 1), (4101, 512, 64), (20011, 384, 8)]
BNBWD_ROWS = [r for r in COLSTAT_ROWS if r[2] in (0, 8)]
BNBWD_16BIT_ROWS = [(129, 256, 8), (257, 192, 8)]                 # one vector row, one scalar row
_case_cache = {}


def _cached(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _case_cache:
            _case_cache[k] = fn(*key)
        return _case_cache[k]
    return wrapped


def sum_terms_bound(n_ops, terms_abs_sum):
    """n 2^-24 sum|terms|: forward bound of an fp32 sum of n_ops roundings per term chain, in any order"""
    return n_ops * U32 * terms_abs_sum


@_cached
def colstat_case(row):
    """y = std randn + (mean / std) std with a per-channel std in [0.5, 2] and a per-channel sign of the offset; float64 and
    float32 evaluations of bn_stats64 / bn_finalize64 (training and eval) and the any-order sum bounds of the mean and of the
    raw moments from their own terms.  The variance and the running variance have none: their terms (y - mean)^2 are all
    non-negative, so n 2^-24 sum|terms| is n 2^-24 of the value itself - 1.2e-3 at M 20 011, wide enough to admit the
    cancellation of sum y^2 / M - mean^2 that the rows are there to catch.  They are held to K_SUM x e32 of the two-pass
    formula alone."""
    M, C, ratio = row
    f64, f32 = torch.float64, torch.float32
    std = 0.5 + 1.5 * (arr("cs_s", (C,), M + C).abs().clamp(max=3.0) / 3.0)
    sign = torch.where(arr("cs_g", (C,), M + C + 1) >= 0, 1.0, -1.0)
    y = (arr("cs_y", (M, C), M + C + 2) * std + sign * ratio * std).float()
    gamma, beta = arr("cs_ga", (C,), M + 3) * 0.1 + 1, arr("cs_be", (C,), M + 4) * 0.1
    rm0, rv0 = arr("cs_rm", (C,), M + 5) * 0.5, arr("cs_rv", (C,), M + 6).abs() + 0.5
    y64 = y.double()
    m64, v64 = bn_stats64(y64)
    m32, v32 = bn_stats64(y)
    n = M + 3                                                    # M - 1 additions, the subtraction, the product, the division
    bm = sum_terms_bound(n, y64.abs().sum(0)) / M
    braw = torch.stack([sum_terms_bound(n, y64.abs().sum(0)), sum_terms_bound(n, (y64 * y64).sum(0))], dim=1)

    def fin(dt, eval_mode, mutant=None, stats=None):
        return bn_finalize64(y.to(dt), gamma.to(dt), beta.to(dt), rm0.to(dt), rv0.to(dt), BN_EPS, BN_MOMENTUM, eval_mode, mutant, stats)
    c = dict(y=y, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, mean64=m64, var64=v64, mean32=m32, var32=v32, mean_bound=bm,
             raw64=torch.stack([y64.sum(0), (y64 * y64).sum(0)], dim=1),
             raw32=torch.stack([seq_sum(y), seq_sum(y * y)], dim=1), raw_bound=braw, fin=fin,
             fin64=fin(f64, False, stats=(m64, v64)), fin32=fin(f32, False, stats=(m32, v32)),
             fin64_eval=fin(f64, True), fin32_eval=fin(f32, True),
             run_mean_bound=BN_MOMENTUM * bm)                   # the running mean moves by momentum x the batch mean
    return c


FIN_NAMES = ("mean", "rstd", "sc", "sh", "running mean", "running var")


@_cached
def bnbwd_case(row, eval_mode, g_dtype=None):
    """cotangent g (rounded to g_dtype first, when given: both sides see the same 16-bit values), statistics as the forward
    hands them over (fp32 roundings of the float64 batch statistics, or the running ones), dy / dgamma / dbeta in float64 and
    float32 and the sum bounds of dgamma / dbeta from the reference's own terms"""
    M, C, _ = row
    c = colstat_case(row)
    g = arr("bb_g", (M, C), M + C + 9)
    if g_dtype is not None:
        g = g.to(g_dtype).float()
    fin = c["fin64_eval"] if eval_mode else c["fin64"]
    mean, rstd = fin[0].float(), fin[1].float()
    ev = lambda dt, mutant=None, em=eval_mode: bn_swish_bwd64(g.to(dt), c["y"].to(dt), mean.to(dt), rstd.to(dt), c["gamma"].to(dt),
                                                               c["beta"].to(dt), em, mutant)
    y64 = c["y"].double()
    xh = (y64 - mean.double()) * rstd.double()
    t = xh * c["gamma"].double() + c["beta"].double()
    sg = torch.sigmoid(t)
    dt_ = (g.double() * sg * (1 + t * (1 - sg))).abs()
    n = M + 8                                                    # M - 1 additions behind ~8 roundings of each term
    return dict(g=g, mean=mean, rstd=rstd, ref64=ev(torch.float64), ref32=ev(torch.float32), ev=ev,
                dbeta_bound=sum_terms_bound(n, dt_.sum(0)), dgamma_bound=sum_terms_bound(n, (dt_ * xh.abs()).sum(0)))


# (B, T, C, KS) -> reduce levels of the partial sums (32 partials per level): LDS kernel at the old shape; T 1; T < k; 52
# partials (two levels, a second chunk of 20); generic <31> kernel with a half-empty second channel block and 39 partials
# (a remainder of 7 = 4 + 3); 1040 partials (three levels); C even but no multiple of 4; 4 active threads
DWGRAD_ROWS = [(3, 50, 256, 31), (1, 1, 256, 31), (2, 7, 512, 31), (2, 801, 256, 31), (3, 400, 384, 31), (40, 832, 64, 7),
               (3, 33, 130, 7), (2, 20, 8, 7)]
DWGRAD_PARTS = {(3, 50, 256, 31): (6, 1), (1, 1, 256, 31): (1, 1), (2, 7, 512, 31): (2, 1), (2, 801, 256, 31): (52, 2),
                (3, 400, 384, 31): (39, 2), (40, 832, 64, 7): (1040, 3), (3, 33, 130, 7): (6, 1), (2, 20, 8, 7): (2, 1)}


def dwgrad_parts(row):
    """(partials, reduce levels) of a row from the library's own scratch size (a host function: no GPU needed)"""
    from sincformer_metacog_speech_enhancement_amd import lib
    B, T, C, KS = row
    n = int(lib.load().sfm_dwconv_wgrad_scratch_floats(B, T, C, KS)) // ((KS + 1) * C)
    levels, m = 1, n
    while m > 32:
        m, levels = -(-m // 32), levels + 1
    return n, levels


@_cached
def dwgrad_case(row, dt16):
    """x rounded to the 16-bit format before both sides see it, dy fp32.  Both carry an offset (x + 2, dy + 2): the sums over
    B x T frames then do not cancel, and the any-order sum bound (n 2^-24 sum|terms|, ~ n 2^-24 of the value instead of
    n^1/2 times more) still sees a dropped chunk of partials at 33 282 frames"""
    B, T, C, KS = row
    x = (arr("dg_x", (B, T, C), T + C) + 2.0).to(dt16).float()
    dy = arr("dg_g", (B, T, C), T + C + 1) + 2.0
    ev = lambda dt, mutant=None, nparts=None: dwconv_wgrad64(x.to(dt), dy.to(dt), KS, mutant, nparts)
    xa, ga = x.double().abs(), dy.double().abs()
    mag = dwconv_wgrad64(xa, ga, KS)
    n = B * T + 2
    return dict(x=x, dy=dy, ref64=ev(torch.float64), ref32=ev(torch.float32), ev=ev,
                dw_bound=sum_terms_bound(n, mag[0]), db_bound=sum_terms_bound(n, mag[1]))


DWFOLD_ROWS = [(2, 200, 256, 31), (3, 7, 64, 7), (1, 1, 256, 31), (2, 801, 384, 31)]


@_cached
def dwfold_case(row, dt16):
    """forward: conv + bias with the forward taps; backward: the input gradient of dwconv64 (torch autograd) for a cotangent
    rounded to the 16-bit format, which the kernel forms with the flipped taps and a zero bias"""
    B, T, C, KS = row
    x = arr("df_x", (B, T, C), T + C).to(dt16).float()
    w = arr("df_w", (C, KS), T + C + 1) / math.sqrt(KS)
    bias = arr("df_b", (C,), T + C + 2) * 0.1
    gy = arr("df_g", (B, T, C), T + C + 3).to(dt16).float()
    fwd = lambda dt, mutant=None: dwconv64(x.to(dt), w.to(dt), bias.to(dt), mutant)
    bwd = lambda dt, mutant=None: _grad(lambda xx: (dwconv64(xx, w.to(dt), bias.to(dt), mutant) * gy.to(dt)).sum(), x.to(dt))[0]
    n = KS + 2
    wa = w.double().abs()
    bf = sum_terms_bound(n, dwconv64(x.double().abs(), wa, bias.double().abs()))
    bb = sum_terms_bound(n, dwconv64(gy.double().abs(), torch.flip(wa, dims=[1]), torch.zeros(C, dtype=torch.float64)))
    return dict(x=x, w=w, bias=bias, gy=gy, fwd=fwd, bwd=bwd, fwd64=fwd(torch.float64), fwd32=fwd(torch.float32),
                bwd64=bwd(torch.float64), bwd32=bwd(torch.float32), fwd_bound=bf, bwd_bound=bb)


def check_row16(name, got, ref64, ref32, k, dt16):
    """a 16-bit output against the float64 reference, element by element: one rounding to nearest in the format - the unit
    roundoff, 2^-8 of the element for bf16 (8 significant bits) and 2^-11 for fp16 (11), which tensor.to() itself reaches; half
    of that is below what a correctly rounded result can meet - plus k x e32 (the max figure of the float32 evaluation, x
    max|ref|)"""
    rnd = 2.0 ** -8 if dt16 == torch.bfloat16 else 2.0 ** -11
    r = ref64.detach().double()
    e32 = figs(ref32, r)
    allow = rnd * r.abs() + k * e32[1] * float(r.abs().max())
    err = (torch.as_tensor(got).detach().cpu().double() - r).abs()
    worst = float((err / allow).max())
    print("ROW | %s | all | e32 %.2e %.2e | bound 1 rounding (%.2e of the element) + %g e32 | observed %.2f of the bound, max err %.2e"
          % (name, e32[0], e32[1], rnd, k, worst, float(err.max())))
    assert math.isfinite(worst) and worst <= 1.0, (name, worst)
