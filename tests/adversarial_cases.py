"""Shared cases of the AdversarialLoss tests (tests/test_adversarial_*.py, tests/golden/make_golden_adversarial.py): the seeded
inputs, a restatement of SubDiscriminator / AdversarialLoss from torch's own CPU ops (F.conv1d, F.avg_pool1d, an explicit power
iteration, autograd for the gradients) that computes in the dtype of the state it is given (float64: the reference of the GPU
rows; float32: that evaluation's own error), and a 16-bit emulation of it (W / sigma and every conv's input rounded to the
operand format, everything else as before) whose distance from the float64 form sets the GPU loss tolerance, and whose
gradient is the float64 gradient AT the rounded operands: LeakyReLU and the L1 of the feature term have kinks, so a
pre-activation (or feature difference) within operand rounding of zero takes the other slope there.  Test-side only.

A `state` is a dict with the keys of the module's state_dict (discriminators.{i}.layers.{j}.{bias, weight_orig, weight_u,
weight_v}); a call of a discriminator in training mode advances weight_u / weight_v IN the dict, as the module's buffers move."""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = ((64, 128, 256, 512), (64, 128, 256), (32, 64, 128))
INIT_SEED = 170
EPS = 1e-12
# name -> (input_dim, B, T, seed)
CASES = {
    "a1_odd_f9_t37": (9, 2, 37, 171),           # 37 -> 19 -> 10 -> 5 through the strides, 37 -> 18 -> 9 through the pools; F % 8 != 0
    "a2_shortest_t4": (129, 3, 4, 172),         # 4 -> 2 -> 1: the last scale is one frame, every window mostly padding
    "a3_default_t64": (129, 2, 64, 173),
    "a4_wide_f257_t16": (257, 1, 16, 174),      # the 16 kHz width (padded to 512 on the device)
}
MODES = ("d", "g", "fm")

_cache = {}


def case(name):
    """clean / enh: fp32 magnitudes [B, F, T] (positive, spectrum-like: louder at low bins); *_re / *_im: channels-last
    [B, T, F] spectra with those magnitudes up to rounding and the 1e-8 under the root"""
    if name not in _cache:
        n_freq, B, T, seed = CASES[name]
        g = torch.Generator().manual_seed(seed)
        tilt = torch.linspace(1.5, 0.3, n_freq).view(1, n_freq, 1)
        clean = (torch.randn(B, n_freq, T, generator=g).abs() + 0.05) * tilt
        enh = (clean * (1.0 + 0.3 * torch.randn(B, n_freq, T, generator=g)).abs() + 0.02 * torch.rand(B, n_freq, T, generator=g))
        out = {"clean": clean.contiguous(), "enh": enh.contiguous()}
        for k in ("clean", "enh"):
            ph = 6.2831853 * torch.rand(B, T, n_freq, generator=g)
            m = out[k].transpose(1, 2)
            out[k + "_re"], out[k + "_im"] = (m * torch.cos(ph)).contiguous(), (m * torch.sin(ph)).contiguous()
        _cache[name] = out
    return _cache[name]


def conv_keys(i):
    """state keys' prefixes of discriminator i's convs, the head last"""
    return ["discriminators.%d.layers.%d." % (i, 2 * l) for l in range(len(CHANNELS[i]) + 1)]


def init_state(input_dim, seed=INIT_SEED):
    """the seeded default init, drawn as a module built in the documented order draws it: per discriminator, per conv, a
    Conv1d and at once its legacy spectral_norm (which draws weight_u, weight_v)"""
    torch.manual_seed(seed)
    state = {}
    for i, chans in enumerate(CHANNELS):
        cin = input_dim
        for l, c in enumerate(list(chans) + [1]):
            head = l == len(chans)
            m = torch.nn.utils.spectral_norm(torch.nn.Conv1d(cin, c, 3 if head else 5, padding=1 if head else 2))
            for k in ("bias", "weight_orig", "weight_u", "weight_v"):
                state[conv_keys(i)[l] + k] = getattr(m, k).detach().clone()
            cin = c
    return state


def cast_state(state, dtype):
    return {k: v.detach().to("cpu", dtype).clone() for k, v in state.items() if k.startswith("discriminators.")}


def param_keys(state):
    return [k for k in state if k.endswith(("bias", "weight_orig"))]


class _RoundSTE(torch.autograd.Function):
    """round to `fmt` and back; the gradient passes unchanged (the device rounds operands, not the chain rule's factors)"""

    @staticmethod
    def forward(ctx, t, fmt):
        return t.to(fmt).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def _round(t, fmt):
    return t if fmt is None else _RoundSTE.apply(t, fmt)


def spectral_weight(state, pre, training):
    """W / sigma of the conv at `pre`; in training mode first one power iteration, written into the state without gradient"""
    w = state[pre + "weight_orig"]
    mat = w.reshape(w.shape[0], -1)
    if training:
        with torch.no_grad():
            v = F.normalize(torch.mv(mat.t(), state[pre + "weight_u"]), dim=0, eps=EPS)
            u = F.normalize(torch.mv(mat, v), dim=0, eps=EPS)
            state[pre + "weight_u"], state[pre + "weight_v"] = u, v
    u, v = state[pre + "weight_u"].detach(), state[pre + "weight_v"].detach()
    return w / torch.dot(u, torch.mv(mat, v))


def disc(state, i, x, training, fmt=None):
    """one call of discriminator i on x [B, F, T] -> (out [B, 1, T'], [post-LeakyReLU features])"""
    pres = conv_keys(i)
    feats = []
    for l, pre in enumerate(pres[:-1]):
        w = _round(spectral_weight(state, pre, training), fmt)
        x = F.leaky_relu(F.conv1d(_round(x, fmt), w, state[pre + "bias"], stride=2 if l < len(pres) - 2 else 1, padding=2), 0.2)
        feats.append(x)
    w = _round(spectral_weight(state, pres[-1], training), fmt)
    return F.conv1d(_round(x, fmt), w, state[pres[-1] + "bias"], padding=1), feats


def _pool(x):
    return F.avg_pool1d(x, 4, 2, 1)


def loss(state, mode, clean, enh, training=True, fmt=None):
    """the objective `mode` of MODES with the reference's call sequence: per scale real first, then fake"""
    total = 0.0
    real, fake = clean, (enh.detach() if mode == "d" else enh)
    for i in range(len(CHANNELS)):
        if mode == "d":
            ro, _ = disc(state, i, real, training, fmt)
            fo, _ = disc(state, i, fake, training, fmt)
            total = total + F.mse_loss(ro, torch.ones_like(ro)) + F.mse_loss(fo, torch.zeros_like(fo))
        elif mode == "g":
            fo, _ = disc(state, i, fake, training, fmt)
            total = total + F.mse_loss(fo, torch.ones_like(fo))
        else:
            _, rf = disc(state, i, real, training, fmt)
            _, ff = disc(state, i, fake, training, fmt)
            for a, b in zip(rf, ff):
                total = total + F.l1_loss(b, a.detach())
        if i < len(CHANNELS) - 1:
            real = None if real is None else _pool(real)
            fake = _pool(fake)
    return total / len(CHANNELS)


def magnitudes(re, im):
    """[B, T, F] pair -> [B, F, T] magnitudes, the convention of the *_cl forms"""
    return torch.sqrt(re * re + im * im + 1e-8).transpose(1, 2)


def run(state0, mode, clean, enh, dtype=torch.float64, training=True, fmt=None, grad_out=1.0, pair=None):
    """evaluate in `dtype` from a copy of state0 -> dict(loss, grad (to enh, or (d re, d im) with pair = (clean_re, clean_im,
    enh_re, enh_im)), pgrads {key: gradient}, state (after the calls)).  mode "g" ignores clean."""
    state = cast_state(state0, dtype)
    for k in param_keys(state):
        state[k].requires_grad_(True)
    if pair is not None:
        cr, ci, er, ei = [t.detach().to(dtype) for t in pair]
        leaves = [er.requires_grad_(True), ei.requires_grad_(True)]
        c, e = magnitudes(cr, ci), magnitudes(er, ei)
    else:
        c = None if clean is None else clean.detach().to(dtype)
        e = enh.detach().to(dtype).requires_grad_(True)
        leaves = [e]
    val = loss(state, mode, c, e, training, fmt)
    (val * grad_out).backward()
    out = {"loss": val.detach(), "pgrads": {k: state[k].grad for k in param_keys(state)},
           "state": {k: v.detach() for k, v in state.items()}}
    out["grad"] = leaves[0].grad if pair is None else (leaves[0].grad, leaves[1].grad)
    return out


def emulation_error(fmt, mode, names=tuple(CASES)):
    """largest relative error, over the cases, of the 16-bit emulation's loss against the float64 restatement (training mode,
    seeded init): what rounding the operands alone costs.  Computed on the CPU from the restatement, never from the kernels."""
    worst = 0.0
    for name in names:
        c = case(name)
        s0 = init_state(CASES[name][0])
        with torch.no_grad():
            ref = float(loss(cast_state(s0, torch.float64), mode, c["clean"].double(), c["enh"].double()))
            emu = float(loss(cast_state(s0, torch.float64), mode, c["clean"].double(), c["enh"].double(), fmt=fmt))
        worst = max(worst, abs(emu - ref) / abs(ref))
    return worst


def rel_rmse(a, b):
    """||a - b|| / ||b|| in float64"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def summary(t):
    """what the state fixture keeps of a tensor: its float64 sum and first 8 values"""
    f = t.detach().double().reshape(-1)
    return {"shape": list(t.shape), "sum": float(f.sum()), "first": [float(v) for v in f[:8]]}


def to_numpy(t):
    return np.asarray(t.detach().cpu().numpy())
