"""Thin Python wrappers over the C ABI (one function per entry point) plus the
host-side weight packing the kernels expect.  Tensors must live on the HIP
device; there is no CPU fallback (lib.load() raises if the .so is missing).

A wrapper checks what its launcher cannot see behind a pointer - each tensor operand's dtype, contiguity and shape or element
count, all with the one predicate _is - and refuses through _refuse with the header's SFM_ERR_SHAPE, the launcher's own answer,
before any shape is unpacked or anything is enqueued.  The scalar ranges of a contract (2 <= M <= QUANT_MAX_STEPS, 0 < hop <=
frame, ...) are tested inline beside the operands they size; only sfm_gammatone_tf's own fit of K and hop is left to its launcher.
The Conformer hot path (gemm16 ... istft_ola, the training GEMMs, the LSTM) checks nothing."""
import ctypes
import math
import re as _re
import numpy as np
import torch

from . import lib as _lib

_K = _lib.CONSTANTS                 # every number shared with the kernels is read from include/sincformer_hip.h (SFM_<NAME>)
EPI_NONE, EPI_SWISH, EPI_GELU, EPI_RESID, EPI_GLU, EPI_SIGMOID, EPI_TANH_SCALE, EPI_SIGMA, EPI_CPEA = (
    _K["EPI_" + _n] for _n in ("NONE", "SWISH", "GELU", "RESID", "GLU", "SIGMOID", "TANH_SCALE", "SIGMA", "CPEA"))

_DT_ID = {torch.bfloat16: _K["DT_BF16"], torch.float16: _K["DT_F16"]}
import os as _os
TRAIN_DTYPE = torch.float16         # base (training) operand format: the reference's own AMP recipe, see reset_precision
_state = {"dtype": TRAIN_DTYPE}

# Every kernel-selection switch of the package: name -> [environment variable or None, default, current value].  The environment
# is read here, once, at import; the set_* functions below write the current value.  bench.py times nothing while
# variant_overrides() reports an entry away from its default.  The precision policy is no switch
# (bench.py sets it itself), nor is SFM_LIB_PATH (lib.py: the documented way to time another build).
_SWITCHES = {
    "gemm_variant": ["SFM_GEMM_VARIANT", 0, 0],             # set_gemm_variant
    "attention_variant": [None, 0, 0],                      # set_attention_variant
    "lin256": ["SFM_LIN256", True, True],                   # set_lin256
    "headpool": ["SFM_HEADPOOL", True, True],               # set_headpool
    "lstm_w16": ["SFM_LSTM_W16", True, True],               # set_lstm_w16
    "deterministic": ["SFM_DETERMINISTIC", True, True],     # set_deterministic
    "wgrad_stream": ["SFM_WGRAD_STREAM", True, True],       # wgrad_side_stream: weight-gradient GEMMs on a second stream
    "fuse_ffn_swish": ["SFM_FUSE_FFN_SWISH", True, True],   # train.py: Swish (+ hidden dropout) of the FFN in its GEMMs' epilogues
    "fuse_next_drop": ["SFM_FUSE_NEXT_DROP", True, True],   # train.py: the LayerNorm backward also writes the next node's operand
    "steal_grads": ["SFM_STEAL_GRADS", False, False],       # optim.FlatAdamW's default for steal_grads=None
    # read by the library itself (csrc/lstm.hip), never by the package: listed so that it is reported
    "lstm_bwd_lpu": ["SFM_LSTM_BWD_LPU", 4, 4],
    "gammatone_fused": [None, True, True],                  # set_gammatone_fused: hop-block sums inside the FIR kernel
    "sinc_fir_resident": [None, True, True],                # set_sinc_fir_resident: one-pass sinc FIR with the taps in registers
}
for _sw in _SWITCHES.values():
    if _sw[0] is not None and _sw[0] in _os.environ:
        _sw[2] = (_os.environ[_sw[0]] != "0") if isinstance(_sw[1], bool) else int(_os.environ[_sw[0]])


def switch(name):
    return _SWITCHES[name][2]


def variant_overrides():
    """the switches that are NOT at their default, by name: bench.py refuses to time anything while one is active"""
    return {name: cur for name, (_, default, cur) in _SWITCHES.items() if cur != default}


def set_gemm_variant(v):
    """0 auto, 2 = 128-row tiles, 6 = persistent, 9 = 256-row wide tiles, 10 = 512 x 128 tiles (A/B testing)."""
    _SWITCHES["gemm_variant"][2] = int(v)


_DT_NAMES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16,
             "float16": torch.float16}
# Inference stages of the path whose 16-bit operand format can be chosen separately (the boundaries between them are
# fp32 tensors, so no stage reads another stage's 16-bit data in the wrong format):
#   pa    PerceptionAgent convs (inputs are GroupNorm + GELU outputs, the sinc FIR output is bounded by the waveform)
#   front CPEA, the fused 1026-column operand, fusion MLP, input projections
#   block the Linear / Conv1d GEMMs of the Conformer blocks (operands are LayerNorm outputs or bounded activations)
#   attn  the Q | K | V buffer and the attention core (QK^T, softmax, PV), head_dim 64 kernels
#   tail  output projection and the mask heads
STAGES = ("pa", "front", "block", "attn", "tail")
POLICIES = {
    "bf16": {s: torch.bfloat16 for s in STAGES},
    "fp16": {s: torch.float16 for s in STAGES},
    # default of inference: measured per-stage error budget in profiles/r02/precision_probe.json
    # (bf16 everywhere misses the 1e-3 mask bound: 1.3-1.6e-3; a bf16 PerceptionAgent alone costs 6.5e-4 of it; with the
    # attention core in bf16 and fp16 elsewhere the whole path is at 3e-4)
    "mixed": {"pa": torch.float16, "front": torch.float16, "block": torch.float16, "attn": torch.bfloat16,
              "tail": torch.float16},
}
_state["policy"] = dict(POLICIES["mixed"])          # inference default; training uses the base dtype (fp16 + loss scale)
_state["policy_name"] = "mixed"


def reset_precision():
    """the defaults: inference stages per POLICIES["mixed"]; base (training) format fp16 - what the reference trains in
    (fp16 autocast + torch.amp.GradScaler, training/conformer_pipeline.py:442, 504, 512-517), used with optim.DynamicLossScale.
    A uniform bf16 step stays available (set_compute_dtype) as a diagnostic: its 8-bit mantissas make this objective's
    gradient a quarter noise (training error budget)."""
    _state["dtype"] = TRAIN_DTYPE
    _state["policy"] = dict(POLICIES["mixed"])
    _state["policy_name"] = "mixed"


def _as_dtype(dt):
    if isinstance(dt, str):
        dt = _DT_NAMES[dt]
    if dt not in _DT_ID:
        raise ValueError("compute dtype must be bfloat16 or float16")
    return dt


def set_compute_dtype(dt):
    """16-bit MFMA operand/activation format for EVERYTHING (training and every inference stage):
    torch.bfloat16 or torch.float16.  See set_precision_policy for the per-stage recipe of inference."""
    dt = _as_dtype(dt)
    _state["dtype"] = dt
    _state["policy"] = {s: dt for s in STAGES}
    _state["policy_name"] = "bf16" if dt is torch.bfloat16 else "fp16"


def set_precision_policy(policy):
    """Operand format per inference stage: a name of POLICIES ("bf16", "fp16", "mixed") or a dict stage -> dtype
    (keys of STAGES; "block3" / "attn3" override one Conformer block).  Training keeps the base dtype."""
    if isinstance(policy, str):
        name, pol = policy, dict(POLICIES[policy])
    else:
        pol = dict(POLICIES["bf16"])
        pol.update({k: _as_dtype(v) for k, v in policy.items()})
        name = "custom:" + ",".join("%s=%s" % (k, "bf16" if v is torch.bfloat16 else "fp16") for k, v in sorted(pol.items()))
    _state["policy"] = pol
    _state["policy_name"] = name


def policy_name():
    return _state["policy_name"]


_state["weights_gen"] = 0


def bump_weights_generation():
    """Called by optimisers that update parameters through storage the parameter's own version counter does not see
    (optim.FlatAdamW steps a flat buffer the parameters are views of): invalidates every packed-weight cache."""
    _state["weights_gen"] += 1


def policy_key():
    """hashable signature of (base dtype, per-stage formats, weights generation): part of every packed-weight cache key"""
    return (_state["dtype"], _state["weights_gen"]) + tuple(sorted((k, str(v)) for k, v in _state["policy"].items()))


def stage_dtype(name, index=None):
    pol = _state["policy"]
    if index is not None and (name + str(index)) in pol:
        return pol[name + str(index)]
    return pol[name]


class stage:
    """with ops.stage("block", 3): ... — kernels and packs inside use that stage's operand format"""

    def __init__(self, name, index=None):
        self.dt = stage_dtype(name, index)

    def __enter__(self):
        self.prev = _state["dtype"]
        _state["dtype"] = self.dt
        return self

    def __exit__(self, *exc):
        _state["dtype"] = self.prev
        return False


def compute_dtype():
    return _state["dtype"]


def dtype_name():
    return "bf16" if _state["dtype"] is torch.bfloat16 else "f16"


def _dt():
    return _DT_ID[_state["dtype"]]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("sincformer HIP ops need device tensors (no CPU fallback); got a CPU tensor")


_F32, _F64, _I32 = torch.float32, torch.float64, torch.int32


def _is(t, dtype, size=None, least=None, rows=None, opt=False, contig=True, ndim=None):
    """the one operand predicate: t is a tensor of `dtype` (None: any), contiguous (contig="last": only its last stride must be 1,
    a row matrix; contig=False: not asked), of `size`: an int = that many elements in any shape, a tuple = that shape, where a
    None entry is a dimension of any size that the caller binds afterwards (ndim=k: k such dimensions).  least: at least that
    many elements; rows: at least that many in the first dimension; opt=True: None passes (an optional operand).  A bool; never
    raises on a tensor or None.  It runs before every launch of a checking wrapper: the plain cases come first and cost a call."""
    if t is None:
        return opt
    if t.dtype is not dtype and dtype is not None:          # (torch's dtypes are singletons)
        return False
    if contig is True:
        if not t.is_contiguous():
            return False
    elif contig and (t.dim() == 0 or t.stride(-1) != 1):
        return False
    if size is not None:
        if size.__class__ is not tuple:
            if t.numel() != size:
                return False
        else:
            shape = t.shape
            if shape != size:                               # (an exact shape passes here; the loop is for the None entries)
                if len(shape) != len(size):
                    return False
                for want, have in zip(size, shape):
                    if want is not None and want != have:
                        return False
    if ndim is not None and t.dim() != ndim:
        return False
    if least is not None and t.numel() < least:
        return False
    return rows is None or (t.dim() > 0 and t.shape[0] >= rows)


def _each(dtype, n, *ts):
    """_is(t, dtype, n) of every t in one call: contiguous tensors of `dtype` with n elements each (n None: of any size)"""
    for t in ts:
        if t is None or t.dtype is not dtype or not t.is_contiguous() or (n is not None and t.numel() != n):
            return False
    return True


def _lengths_ok(lengths, B):
    """the per-utterance `lengths` operand (and `frames` of dnn_layer): None, or int32 [B] contiguous"""
    return lengths is None or _is(lengths, _I32, B)


def _refuse(name):
    """the one refusal of a wrapper's contract: RuntimeError("<name> failed: unsupported shape (-2)"), the launcher's own answer"""
    _lib.check(_K["ERR_SHAPE"], name)


def round_up(x, m):
    return (x + m - 1) // m * m


class KernelProfiler:
    """Optional HIP-event timing of individual launches (bench.py / profiling only).
    Events are recorded on the current torch stream, i.e. the stream the kernels are
    enqueued on.  enable(None) instruments every family, enable({"attention"}) one."""

    def __init__(self):
        self.families = set()
        self.all = False
        self.records = []
        self.tags = False

    def enable(self, families=None, tags=False):
        self.tags = tags
        self.all = families is None
        self.families = set(families or ())
        self.records = []

    def disable(self):
        self.all = False
        self.families = set()

    def active(self, name):
        return self.all or name in self.families

    def summary(self):
        """{family: dict(n, ms_total, ms_avg, flops, bytes)} — synchronises."""
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, fl, by in self.records:
            d = out.setdefault(name, {"n": 0, "ms_total": 0.0, "flops": 0.0, "bytes": 0.0})
            d["n"] += 1
            d["ms_total"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        for d in out.values():
            d["ms_avg"] = d["ms_total"] / max(d["n"], 1)
        return out


    def launches(self, name):
        """[(ms, flops, bytes)] of every recorded launch of family `name`, in launch order — synchronises."""
        torch.cuda.synchronize()
        return [(e0.elapsed_time(e1), fl, by) for n, e0, e1, fl, by in self.records if n == name]


profiler = KernelProfiler()

# ---------------------------------------------------------------------------
# ordered reductions: scratch for the per-workgroup partials
# ---------------------------------------------------------------------------
# Every split reduction of the training step (weight-gradient M-splits, bias column sums, LayerNorm / GroupNorm dgamma / dbeta,
# BatchNorm statistics, the objective's moments, ||g||^2) writes its per-workgroup partials into a workspace and folds them in a
# fixed order (csrc/reduce.hip) instead of issuing atomics: a step is then bit-reproducible, like the reference's CPU step.
# SFM_DETERMINISTIC=0 / set_deterministic(False) passes NULL workspaces = the fp32-atomics form (A/B of the cost).
_WS_BUFS = {}


def set_deterministic(flag):
    _SWITCHES["deterministic"][2] = bool(flag)


def is_deterministic():
    return switch("deterministic")


def _ws(n, device, dtype=torch.float32):
    """scratch of >= n elements for the kernel about to be enqueued on the CURRENT stream (one grow-only buffer per device,
    stream and dtype: launches of one stream run in order, so the fold of one launch has read the partials before the next
    launch overwrites them; a replaced buffer goes back to the caching allocator, which hands memory freed on a stream only
    to later work of that stream).  None when the atomics form is selected."""
    if not switch("deterministic"):
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, dtype)
    t = _WS_BUFS.get(key)
    if t is None or t.numel() < n:
        t = _WS_BUFS[key] = torch.empty(max(int(n), 1 << 18), device=device, dtype=dtype)
    return t


def _call(name, fn, args, flops=0.0, nbytes=0.0, tag=None):
    """enqueue one entry point; flops / nbytes = the launch's algorithmic cost, stated by the wrapper (each operand read once,
    each result written once: DESIGN.md section 4), tag = its shape for the profiler's per-shape records"""
    if len(args) != len(fn.argtypes):                   # ctypes itself lets surplus arguments of a cdecl function through
        raise TypeError("%s takes %d arguments (include/sincformer_hip.h), %d given" % (fn.__name__, len(fn.argtypes), len(args)))
    try:
        if profiler.active(name):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            profiler.records.append((name, e0, e1, float(flops), float(nbytes)))
            if tag is not None and profiler.tags:
                profiler.records.append(("%s[%s]" % (name, tag), e0, e1, float(flops), float(nbytes)))
        else:
            rc = fn(*args)
    except ctypes.ArgumentError as e:                   # "argument 7: ... wrong type": say which parameter of the header that is
        m = _re.match(r"argument (\d+):", str(e))
        names = _lib.ABI[fn.__name__][2]
        if m is None or not 1 <= int(m.group(1)) <= len(names):
            raise
        raise ctypes.ArgumentError("%s, parameter `%s`: %s" % (fn.__name__, names[int(m.group(1)) - 1], e)) from None
    _lib.check(rc, name)


# ---------------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------------
class PackedWeight:
    """W [Npad, Kpad] 16-bit (+ fp32 bias [Npad]) for sfm_gemm16."""
    __slots__ = ("w", "bias", "N", "K", "Npad", "Kpad", "ksize", "cin", "glu")

    def __init__(self, w, bias, N, K, ksize, cin, glu=False):
        self.w, self.bias, self.N, self.K = w, bias, N, K
        self.Npad, self.Kpad = w.shape
        self.ksize, self.cin, self.glu = ksize, cin, glu


_ZERO_BIAS = {}


def _zero_bias(n, device):
    """read-only fp32 zeros [n], cached per device"""
    key = (int(n), str(device))
    t = _ZERO_BIAS.get(key)
    if t is None:
        t = _ZERO_BIAS[key] = torch.zeros(n, device=device, dtype=torch.float32)
    return t


def pack_linear(weight, bias=None, glu=False, k_pad_to=None, dtype=None):
    """weight [N, K] (nn.Linear) or [N, Cin, k] (nn.Conv1d; repacked to tap-major K).
    glu=True interleaves the two halves in 32-row groups for the GLU epilogue."""
    dtype = dtype or _state["dtype"]
    w = weight.detach().float()
    ksize, cin = 1, w.shape[1]
    if w.dim() == 3:
        ksize = w.shape[2]
        w = w.permute(0, 2, 1).reshape(w.shape[0], -1)       # [N, k*Cin], tap-major
    N, K = w.shape
    Kpad = round_up(k_pad_to or K, 64)
    if glu or (N > 64 and round_up(N, 128) - N < 64):
        Npad = round_up(N, 128)          # 128-column tiles
    else:
        Npad = round_up(N, 64)           # 64-column tiles (kernel picks BN from Npad % 128)
    if not glu and N == Npad and K == Kpad:
        # already tile-aligned (every Linear / Conv1d of the path but the heads): one convert launch, the bias is used in
        # place (the training step packs ~150 weights per step; zero-fill + slice-copy per operand was ~800 tiny launches)
        W = w.to(dtype).contiguous()
        Bp = bias.detach().float().contiguous() if bias is not None else _zero_bias(Npad, w.device)
    else:
        b = bias.detach().float() if bias is not None else _zero_bias(N, w.device)
        if glu:
            C = N // 2
            idx = torch.arange(N, device=w.device)
            blk, t = idx // 64, idx % 64
            src = torch.where(t < 32, blk * 32 + t, C + blk * 32 + (t - 32))
            w, b = w[src], b[src]
        W = torch.zeros(Npad, Kpad, device=w.device, dtype=dtype)
        W[:N, :K] = w.to(dtype)
        Bp = torch.zeros(Npad, device=w.device, dtype=torch.float32)
        Bp[:N] = b
    if ksize == 1:
        cin = Kpad if k_pad_to else K    # operand rows must be zero padded up to cin
        if cin % 8 != 0:
            raise ValueError("K=%d is not a multiple of 8: pass k_pad_to and zero-pad the operand" % K)
    return PackedWeight(W.contiguous(), Bp, (N // 2) if glu else N, K, ksize, cin, glu)


def gemm16_cost(pw, B, Lout, Lin, stride, epi, osz, has_resid):
    """(flops, bytes, tag) of one sfm_gemm16 launch with osz-byte results.  A GLU pack multiplies its Npad columns; the bytes count
    pw.N result columns for every pack."""
    rows, ncols = B * Lout, pw.Npad if pw.glu else pw.N
    nbytes = B * Lin * pw.cin * 2 + pw.Npad * pw.Kpad * 2 + rows * pw.N * osz + (rows * pw.N * 4 if has_resid else 0)
    return 2.0 * rows * ncols * pw.K, nbytes, "M%d N%d K%d k%d s%d epi%d o%d" % (rows, ncols, pw.K, pw.ksize, stride, epi, osz)


def gemm16(A, pw, out, *, B, Lout, Lin, a_batch_stride, ldo, o_batch_stride, lda=None, stride=1, pad=0,
           epi=EPI_NONE, resid=None, ldr=0, r_batch_stride=0, alpha=1.0, gn_partial=None, gn_group=0, nsplit=0,
           p_drop=0.0, seed=0):
    """A: [B, Lin, cin] 16-bit with position stride lda (default cin) -> out rows (b, l)."""
    _need_dev(A, out)
    L = _lib.load()
    cin = pw.cin
    lda = cin if lda is None else lda
    # out_f32: 0 = 16-bit in the operands' format, 1 = fp32, 2 = the OTHER 16-bit format (a stage boundary of the precision
    # policy, e.g. the Q | K | V buffer of a bf16 attention core behind fp16 projections): one rounding of the fp32 accumulators
    out_f32 = 1 if out.dtype == torch.float32 else (0 if out.dtype == _state["dtype"] else 2)
    if A.dtype != _state["dtype"] or pw.w.dtype != _state["dtype"]:
        raise RuntimeError("gemm16: operand formats %s / %s do not match the stage's %s (precision policy)" %
                           (A.dtype, pw.w.dtype, _state["dtype"]))
    cost = gemm16_cost(pw, B, Lout, Lin, stride, epi, 4 if out_f32 == 1 else 2, resid is not None)
    if p_drop > 0.0:                                   # training forward: residual-branch dropout in the epilogue
        _call("gemm16", L.sfm_gemm16_train, (_p(A), _p(pw.w), _p(pw.bias), _p(out), _p(resid), _p(gn_partial), B, Lout, Lin, cin,
                                             lda, pw.ksize, stride, pad, a_batch_stride, pw.Kpad, pw.N, pw.Npad, ldo,
                                             o_batch_stride, ldr, r_batch_stride, float(alpha), epi, out_f32, gn_group, nsplit,
                                             _dt(), switch("gemm_variant"), float(p_drop), int(seed) & 0xffffffff, _stream()), *cost)
        return out
    _call("gemm16", L.sfm_gemm16_ex, (_p(A), _p(pw.w), _p(pw.bias), _p(out), _p(resid), _p(gn_partial), B, Lout, Lin, cin, lda,
                      pw.ksize, stride, pad, a_batch_stride, pw.Kpad, pw.N, pw.Npad, ldo, o_batch_stride, ldr, r_batch_stride,
                      float(alpha), epi, out_f32, gn_group, nsplit, _dt(), switch("gemm_variant"), _stream()), *cost)
    return out


def conv16p_supported(cin, n, ksize, stride, pad, two_inputs, skip):
    """layer shapes sfm_conv16p is built for (the PerceptionAgent's: include/sincformer_hip.h)"""
    if cin % 64:
        return False
    key = (ksize, stride, pad, n)
    if skip:
        return key == (7, 2, 3, 128)
    return (key == (7, 2, 3, 256) and two_inputs) or (key in ((3, 1, 1, 128), (3, 1, 1, 256)) and not two_inputs) or \
        (key in ((5, 2, 2, 256), (1, 2, 0, 256)) and two_inputs)


def conv16p(x1, sc1, sh1, pw, out, *, B, Lin, stride, pad, x2=None, sc2=None, sh2=None, gn_partial=None, gn_group=0,
            skip_pw=None, out_s=None, gn_partial_s=None):
    """out = Conv1d(GELU(sc1 * x1 + sh1 [+ sc2 * x2 + sh2]); pw) on channels-last raw conv outputs x1 / x2 [B, Lin, Cin] with
    per-(batch, channel) GroupNorm scale / shift [B, Cin]: the normalised activation is produced while the operand is staged
    and never written to HBM.  skip_pw / out_s / gn_partial_s: the residual block's 1x1 stride-2 skip conv on the same input."""
    _need_dev(x1, out)
    L = _lib.load()
    cin, N, ks = pw.cin, pw.N, pw.ksize
    dt = _state["dtype"]
    if x1.dtype != dt or pw.w.dtype != dt or (x2 is not None and x2.dtype != dt):
        raise RuntimeError("conv16p: operand formats do not match the stage's %s (precision policy)" % dt)
    if pw.Npad != N or pw.Kpad != ks * cin or (skip_pw is not None and (skip_pw.Npad != N or skip_pw.Kpad != cin)):
        raise RuntimeError("conv16p: weights must be packed without padding")
    out_f32 = 1 if out.dtype == torch.float32 else (0 if out.dtype == dt else 2)
    Lout = (Lin + 2 * pad - ks) // stride + 1
    nin = 2 if x2 is not None else 1
    flops = 2.0 * B * Lout * N * (ks * cin + (cin if skip_pw is not None else 0))
    nbytes = B * Lin * cin * 2.0 * nin + B * Lout * N * out.element_size() * (2 if skip_pw is not None else 1) + N * ks * cin * 2.0
    _call("conv16p", L.sfm_conv16p, (_p(x1), _p(sc1), _p(sh1), _p(x2), _p(sc2), _p(sh2), _p(pw.w), _p(pw.bias), _p(out),
                                     _p(gn_partial), _p(skip_pw.w if skip_pw is not None else None),
                                     _p(skip_pw.bias if skip_pw is not None else None), _p(out_s), _p(gn_partial_s), B, Lin, cin, N,
                                     ks, stride, pad, out_f32, gn_group, _dt(), _stream()),
          flops, nbytes, tag="Lout%d Cin%d N%d k%d s%d in%d%s" % (B * Lout, cin, N, ks, stride, nin, " +skip" if skip_pw is not None else ""))
    return out


def set_lin256(flag):
    """K = 256 linears with a plain / GLU epilogue and a 16-bit result on the resident-operand kernel (csrc/lin256.hip; default on,
    SFM_LIN256=0 / False = sfm_gemm16 for every shape: the A/B)"""
    _SWITCHES["lin256"][2] = bool(flag)


def _lin256_weight_ok(pw, epi):
    """the half of the lin256 routing that the switches, the packed weight and the epilogue decide: shared by linear16
    (_lin256_ok) and ln_linear16, whose operand checks differ"""
    return (switch("lin256") and switch("gemm_variant") == 0 and epi in (EPI_NONE, EPI_GLU) and (epi == EPI_GLU) == bool(pw.glu) and
            pw.K == 256 and pw.Kpad == 256 and pw.ksize == 1 and pw.Npad % (128 if pw.glu else 64) == 0 and
            pw.Npad == (2 * pw.N if pw.glu else pw.N) and pw.Npad <= 2048 and pw.w.dtype == _state["dtype"])


def _lin256_ok(x16, pw, epi, out, resid, nsplit, p_drop):
    return (_lin256_weight_ok(pw, epi) and
            resid is None and nsplit == 0 and p_drop == 0.0 and
            (out.dtype in (torch.float16, torch.bfloat16) or (out.dtype == torch.float32 and not pw.glu and out.stride(0) % 4 == 0)) and
            x16.shape[0] >= 4096 and x16.stride(1) == 1 and out.stride(1) == 1 and x16.stride(0) % 8 == 0 and
            (out.stride(0) % 8 == 0 or out.dtype == torch.float32) and
            x16.dtype == _state["dtype"])


def lin256(x16, pw, out):
    """sfm_lin256 (csrc/lin256.hip): out = x16[:, :256] @ W^T + b, or its GLU when pw was packed with glu=True; out 16-bit (either
    format) or, plain epilogue only, fp32.  linear16 routes the shapes of the path here (see _lin256_ok)."""
    _need_dev(x16, out)
    L = _lib.load()
    M, ld = x16.shape[0], x16.stride(0)
    odt_id = 2 if out.dtype == torch.float32 else (1 if out.dtype == torch.float16 else 0)
    osz = 4.0 if out.dtype == torch.float32 else 2.0
    _call("gemm16", L.sfm_lin256, (_p(x16), _p(pw.w), _p(pw.bias), _p(out), M, pw.Npad, ld, out.stride(0), 1 if pw.glu else 0,
                                   _dt(), odt_id, _stream()),
          2.0 * M * pw.Npad * 256, M * 256 * 2.0 + pw.Npad * 512.0 + M * pw.N * osz,
          tag="M%d N%d K256 lin256%s o%d" % (M, pw.Npad, " glu" if pw.glu else "", int(osz)))
    return out


def set_headpool(flag):
    """latent heads + time pooling in one launch (sfm_headpool) in the fused path; False / SFM_HEADPOOL=0 = heads GEMM, then pool_time"""
    _SWITCHES["headpool"][2] = bool(flag)


def headpool_tiles(Tin, Tout):
    """(frames per tile, tiles per utterance) of sfm_headpool, or None when the pair is not supported / the fusion is switched off"""
    if not switch("headpool") or switch("gemm_variant") != 0:
        return None
    fpt = int(_lib.load().sfm_headpool_frames_per_tile(int(Tin), int(Tout)))
    return (fpt, (Tout + fpt - 1) // fpt) if fpt > 0 else None


def headpool(xd16, pw, pooled16, part, B, Tin, Tout, gcols=16):
    """xd16 [B, Tin, 256] -> pooled16 [B, Tout, N] = time-pooled RAW head outputs, part [B, P, N / gcols, 2] = GroupNorm partial sums of
    the full-rate outputs (see include/sincformer_hip.h)."""
    _need_dev(xd16, pooled16, part)
    L = _lib.load()
    if xd16.dtype != _state["dtype"] or pw.w.dtype != _state["dtype"] or pooled16.dtype != _state["dtype"]:
        raise RuntimeError("headpool: operands must be in the stage's format")
    _call("gemm16", L.sfm_headpool, (_p(xd16), _p(pw.w), _p(pw.bias), _p(pooled16), _p(part), B, Tin, Tout, pw.Npad, xd16.stride(1),
                                     pooled16.stride(1), gcols, _dt(), _stream()),
          2.0 * B * Tin * pw.Npad * 256, B * Tin * 512.0 + pw.Npad * 512.0 + B * Tout * pw.Npad * 2.0,
          tag="M%d N%d K256 headpool->T%d" % (B * Tin, pw.Npad, Tout))


def _ln_lin256_ok(x32, ln_w, pw, epi, out):
    return (_lin256_weight_ok(pw, epi) and out.dtype in (torch.float16, torch.bfloat16) and
            x32.shape[0] >= 4096 and x32.dtype == torch.float32 and x32.stride(1) == 1 and x32.stride(0) % 4 == 0 and
            x32.data_ptr() % 16 == 0 and ln_w.numel() == 256)


def ln_linear16(x32, ln_w, ln_b, pw, epi=EPI_NONE, out_dtype=None, eps=1e-5):
    """linear16(LayerNorm(x32[:, :D]), pw, epi) with a 16-bit result, D = ln_w.numel().  On the shapes sfm_lin256 takes (D = K = 256,
    plain or GLU epilogue, M >= 4096) the LayerNorm is the GEMM kernel's prologue (sfm_ln_lin256): one launch, the normalised 16-bit rows
    never reach HBM; otherwise sfm_layernorm + linear16.  The two routes give the same bits."""
    M = x32.shape[0]
    out = torch.empty(M, pw.N, device=x32.device, dtype=out_dtype or _state["dtype"])
    if _ln_lin256_ok(x32, ln_w, pw, epi, out):
        _need_dev(x32, out)
        L = _lib.load()
        lw, lb = ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous()
        _call("gemm16", L.sfm_ln_lin256, (_p(x32), x32.stride(0), _p(lw), _p(lb), float(eps), _p(pw.w), _p(pw.bias), _p(out), M, pw.Npad,
                                          out.stride(0), 1 if pw.glu else 0, _dt(), 1 if out.dtype == torch.float16 else 0, _stream()),
              2.0 * M * pw.Npad * 256, M * 256 * 4.0 + pw.Npad * 512.0 + M * pw.N * 2.0,
              tag="M%d N%d K256 ln+lin256%s" % (M, pw.Npad, " glu" if pw.glu else ""))
        return out
    h16 = torch.empty(M, ln_w.numel(), device=x32.device, dtype=_state["dtype"])
    layernorm(x32, ln_w, ln_b, out16=h16, eps=eps)
    return linear16(h16, pw, epi=epi, out=out)


def linear16(x16, pw, epi=EPI_NONE, out_dtype=None, resid=None, alpha=1.0, out=None, nsplit=0, p_drop=0.0, seed=0):
    """x16 [M, K(>=pw.K)] 16-bit contiguous rows -> [M, N]."""
    M, ld = x16.shape[0], x16.stride(0)
    if out is None:
        odt = out_dtype or (torch.float32 if epi == EPI_RESID else _state["dtype"])
        out = torch.empty(M, pw.N, device=x16.device, dtype=odt)
    if _lin256_ok(x16, pw, epi, out, resid, nsplit, p_drop):
        return lin256(x16, pw, out)
    gemm16(x16, pw, out, B=1, Lout=M, Lin=M, a_batch_stride=0, lda=ld, ldo=out.stride(0), o_batch_stride=0, epi=epi,
           resid=resid, ldr=(resid.stride(0) if resid is not None else 0), alpha=alpha, nsplit=nsplit, p_drop=p_drop,
           seed=seed)
    return out


def linear16_swish(x16, pw, p_drop=0.0, seed=0, aux=None):
    """FFN Linear with the Swish (+ hidden dropout) in the GEMM epilogue (training).
    aux is None: forward -> (d [M, N] 16-bit = drop * swish'(z), the derivative factor the backward needs, u = drop * swish(z));
    aux = saved d: backward -> g * d where g = x16 @ W^T (pw = the transposed pack, no bias)."""
    L = _lib.load()
    M, ld = x16.shape[0], x16.stride(0)
    dt = _state["dtype"]
    out = torch.empty(M, pw.N, device=x16.device, dtype=dt)
    out2 = torch.empty(M, pw.N, device=x16.device, dtype=dt) if aux is None else None
    _call("gemm16", L.sfm_gemm16_swish, (_p(x16), _p(pw.w), _p(pw.bias), _p(out), _p(aux), _p(out2), M, pw.cin, ld, pw.Kpad, pw.N,
                                         pw.Npad, pw.N, 0 if aux is None else 1, float(p_drop), int(seed) & 0xffffffff, _dt(),
                                         _stream()), 2.0 * M * pw.N * pw.K, M * (pw.cin + 2.0 * pw.N) * 2.0 + pw.Npad * pw.Kpad * 2.0,
          tag="M%d N%d K%d swish%s" % (M, pw.N, pw.K, "" if aux is None else "_bwd"))
    return (out2, out) if aux is None else out


def framed_gemm_cost(B, M, Ls, K, N, hop, osz):
    """(flops, bytes, tag) of one sfm_framed_gemm_f32 launch with osz-byte results: the signal is read once, not once per frame"""
    rows = B * M
    return 2.0 * rows * N * K, B * Ls * 4 + rows * N * osz, "M%d N%d K%d hop%d" % (rows, N, K, hop)


def framed_gemm(sig, Wt, out, *, B, M, Ls, sig_batch_stride, hop, padl, K, N, o_batch_stride, ldm, ldn, mode=0,
                bias=None, out2=None, nsplit=0, gn_partial=None, gn_group=0):
    _need_dev(sig, Wt, out)
    L = _lib.load()
    Kpad, Npad = Wt.shape
    out_f32 = 1 if out.dtype == torch.float32 else 0
    _call("framed_gemm_f32", L.sfm_framed_gemm_f32, (_p(sig), _p(Wt), _p(bias), _p(out), _p(out2), _p(gn_partial), B, M, Ls,
                               sig_batch_stride, hop, padl, K, Kpad, N, Npad, nsplit, o_batch_stride, ldm, ldn, mode,
                               out_f32, gn_group, _dt(), _stream()),
          *framed_gemm_cost(B, M, Ls, K, N, hop, 4 if out_f32 else 2))
    return out


def pack_split16_matrix(wt_kn):
    """[K, N] fp32 -> (hi, lo) bf16 pair, n-major [round256(N), round32(K)], operand of framed_gemm_split16."""
    K, N = wt_kn.shape
    w = torch.zeros(round_up(N, 256), round_up(K, 32), device=wt_kn.device, dtype=torch.float32)
    w[:N, :K] = wt_kn.t()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous(), K, N


def framed_gemm_split16(sig, W, out, *, B, M, Ls, sig_batch_stride, hop, padl, o_batch_stride, ldm, mode=0, out2=None, nsplit=0,
                        col2_off=0):
    """W = pack_split16_matrix(...)"""
    _need_dev(sig, out)
    L = _lib.load()
    hi, lo, K, N = W
    Npad, Kpad = hi.shape
    _call("framed_gemm_split16", L.sfm_framed_gemm_split16, (_p(sig), _p(hi), _p(lo), _p(out), _p(out2), B, M, Ls, sig_batch_stride,
                                                             hop, padl, K, Kpad, N, Npad, nsplit, col2_off, o_batch_stride, ldm,
                                                             mode, _stream()),
          2.0 * B * M * K * N, 4.0 * (B * M * hop + B * M * N))
    return out


def pack_f32_matrix(wt_kn):
    """[K, N] fp32 -> zero padded [round32(K), round64(N)] operand of framed_gemm."""
    K, N = wt_kn.shape
    W = torch.zeros(round_up(K, 32), round_up(N, 64), device=wt_kn.device, dtype=torch.float32)
    W[:K, :N] = wt_kn
    return W


ATTN_QSCALE_LOG2E = 1.4426950408889634


def attention_kernel_name(B, T, H, variant=None):
    """name of the forward kernel sfm_attention_fwd_ex / sfm_attention_fwd_train (no dropout) pick for head_dim 64: the rule of
    attention_fwd_impl in csrc/attention.hip, restated (tests/test_attention_rule_gpu.py holds the two together bit by bit)"""
    v = switch("attention_variant") if variant is None else variant
    nqt5 = (T + 511) // 512
    enough = B * H * nqt5 >= 128
    if v == 0:
        if enough and (T >= 1024 or 100 * T >= 78 * 512 * nqt5):
            v = 4
        elif enough and T <= 256 and 100 * T >= 90 * 256:
            v = 5
        else:
            v = 1                                   # short launches and every T outside the windows, T >= 1024 included
    return {1: "attn_fwd_hd64_kernel", 2: "attn_fwd_hd64r_kernel", 3: "attn_fwd_hd64r_kernel", 4: "attn_fwd_hd64p8_kernel",
            5: "attn_fwd_hd64p4_kernel", 6: "attn_fwd_hd64q4_kernel"}[v]


def set_attention_variant(v):
    """0: chosen by shape (default), 1: 32 query rows per wave, 3: persistent ring kernel (2 is accepted as 3), 4 / 5:
    pipelined persistent kernel with one 8-wave / two 4-wave workgroups per CU and 64 query rows per wave, 6: the same with
    four waves of 128 rows (A/B measurements).  Host-side state only: the value is passed to sfm_attention_fwd_ex with every
    call (the library keeps no selection state)."""
    v = int(v)
    if not 0 <= v <= 6:
        raise ValueError("attention variant %d" % v)
    _SWITCHES["attention_variant"][2] = v


def attention(qkv16, B, T, H, hd, out=None, prescaled=False, out_dtype=None):
    """qkv16 [B*T, 3*H*hd] (q | k | v) -> [B*T, H*hd].  prescaled: q already multiplied by
    log2(e)/sqrt(hd) (functional.pack_mhsa folds it into W_q, b_q before the 16-bit rounding)."""
    _need_dev(qkv16)
    L = _lib.load()
    D = H * hd
    ld = qkv16.stride(0)
    if qkv16.dtype != _state["dtype"]:
        raise RuntimeError("attention: Q | K | V are %s, the stage's format is %s" % (qkv16.dtype, _state["dtype"]))
    if out is None:
        out = torch.empty(B * T, D, device=qkv16.device, dtype=out_dtype or qkv16.dtype)
    _call("attention_fwd", L.sfm_attention_fwd_ex, (_p(qkv16), _p(out), B, T, H, hd, ld, out.stride(0), D, 2 * D, T * ld,
                                                    T * out.stride(0), (-1.0 if prescaled else 1.0 / math.sqrt(hd)), _dt(),
                                                    _DT_ID[out.dtype], switch("attention_variant"), _stream()),
          4.0 * B * H * T * T * hd, 4.0 * B * T * H * hd * 2)
    return out


LAYERNORM_MAX_D = _K["LAYERNORM_MAX_D"]      # the widest row sfm_layernorm / sfm_layernorm_bwd_* normalise (so the widest d_model)


def layernorm_bytes(M, D, has_out16, has_out32):
    """fp32 rows in, a 16-bit and / or an fp32 copy of the normalised rows out"""
    return M * D * (4 + (2 if has_out16 else 0) + (4 if has_out32 else 0))


def layernorm(x32, w, b, out16=None, out32=None, act=0, eps=1e-5):
    """rows of x32 [M, >=D] are normalised over their first D = w.numel() columns."""
    _need_dev(x32)
    L = _lib.load()
    M, D = x32.shape[0], w.numel()
    if D > LAYERNORM_MAX_D:
        raise RuntimeError("layernorm: width %d is not supported (the LayerNorm kernels take D <= %d)" % (D, LAYERNORM_MAX_D))
    _call("layernorm", L.sfm_layernorm, (_p(x32), _p(w), _p(b), _p(out16), _p(out32), M, D, x32.stride(0),
                         out16.stride(0) if out16 is not None else 0, out32.stride(0) if out32 is not None else 0,
                         eps, act, _dt(), _stream()),
          8.0 * M * D, layernorm_bytes(M, D, out16 is not None, out32 is not None))


def gn_finalize(partial, w, b, Bn, P, G, C, rows, eps=1e-5):
    L = _lib.load()
    scale = torch.empty(Bn, C, device=w.device, dtype=torch.float32)
    shift = torch.empty(Bn, C, device=w.device, dtype=torch.float32)
    _call("gn_finalize", L.sfm_gn_finalize, (_p(partial), _p(w), _p(b), _p(scale), _p(shift), Bn, P, G, C, rows, eps, _stream()))
    return scale, shift


def gn_apply_bytes(n, in_f32, out_f32, two_inputs):
    """n elements of one or two inputs in, n out, each fp32 or 16-bit"""
    return n * ((4 if in_f32 else 2) * (2 if two_inputs else 1) + (4 if out_f32 else 2))


def gn_apply(x1, sc1, sh1, out, Bn, rows, C, act=0, x2=None, sc2=None, sh2=None):
    L = _lib.load()
    in_f32 = 1 if x1.dtype == torch.float32 else 0
    out_f32 = 1 if out.dtype == torch.float32 else 0
    _call("gn_apply", L.sfm_gn_apply, (_p(x1), _p(sc1), _p(sh1), _p(x2), _p(sc2), _p(sh2), _p(out), Bn, rows, C, in_f32, out_f32, act,
                        _dt(), _stream()),
          10.0 * Bn * rows * C, gn_apply_bytes(Bn * rows * C, in_f32, out_f32, x2 is not None))
    return out


def dwconv_bn_swish(x16, wdw, bdw, bnw, bnb, bnm, bnv, B, T, C, out=None, eps=1e-5):
    L = _lib.load()
    KS = wdw.shape[-1]
    if out is None:
        out = torch.empty_like(x16)
    _call("dwconv_bn_swish", L.sfm_dwconv_bn_swish, (_p(x16), _p(wdw), _p(bdw), _p(bnw), _p(bnb), _p(bnm), _p(bnv), _p(out), B, T, C, KS,
                               eps, _dt(), _stream()),
          2.0 * B * T * C * KS, B * T * C * 4)
    return out


def dwconv_folded(x16, wT, sc, sh, B, T, C, out=None, act=1):
    """depthwise conv + folded BatchNorm(eval) (+ Swish when act) with register-resident taps (KS 7 / 31);
    `out` may be 16-bit (default) or fp32."""
    L = _lib.load()
    KS = wT.shape[0]
    if out is None:
        out = torch.empty_like(x16)
    _call("dwconv_bn_swish", L.sfm_dwconv_folded, (_p(x16), _p(wT), _p(sc), _p(sh), _p(out), B, T, C, KS, int(act),
                                                   1 if out.dtype == torch.float32 else 0, _dt(), _stream()),
          2.0 * B * T * C * KS, B * T * C * 4.0)
    return out


def convert_rows(src32, dst16, M, C, Cz, ld_src, ld_dst):
    L = _lib.load()
    _call("convert_rows", L.sfm_convert_rows, (_p(src32), _p(dst16), M, C, Cz, ld_src, ld_dst, _dt(), _stream()),
          tag="M%d C%d" % (M, C))


def transpose(src, dst, B, R, C, src_batch, src_row, dst_batch, dst_row):
    L = _lib.load()
    _call("transpose", L.sfm_transpose, (_p(src), _p(dst), B, R, C, src_batch, src_row, dst_batch, dst_row,
                         1 if src.dtype == torch.float32 else 0, 1 if dst.dtype == torch.float32 else 0, _dt(),
                         _stream()))


def mean_time(src32, B, T, C, ld_src):
    """mean over time of fp32 [B, T, ld_src] cols [0, C) -> [B, C] (glue G2)"""
    L = _lib.load()
    out = torch.empty(B, C, device=src32.device, dtype=torch.float32)
    scratch = torch.empty(int(L.sfm_mean_time_scratch_floats(B, T, C)), device=src32.device, dtype=torch.float32)
    _call("pool_time", L.sfm_mean_time, (_p(src32), _p(out), _p(scratch), B, T, C, ld_src, _stream()), 0.0, 4.0 * B * T * C)
    return out


def pool_time_bwd(dout32, B, Tin, Tout, C):
    """adjoint of pool_time: dout fp32 [B, Tout, C] -> dsrc fp32 [B, Tin, C]"""
    L = _lib.load()
    dout32 = dout32.contiguous()
    dsrc = torch.empty(B, Tin, C, device=dout32.device, dtype=torch.float32)
    _call("pool_time_bwd", L.sfm_pool_time_bwd, (_p(dout32), _p(dsrc), B, Tin, Tout, C, C, C, _stream()), 0.0,
          4.0 * B * (Tin + Tout) * C)
    return dsrc


def pool_time_bytes(B, Tin, Tout, C, src_bytes):
    """Tin rows of src_bytes-wide elements in, Tout rows out, counted as fp32"""
    return B * (Tin * src_bytes + Tout * 4) * C


def pool_time(src32, dst16, dst32, B, Tin, Tout, C, ld_src, ld_dst, scale=None, shift=None):
    """adaptive average pooling over time; scale / shift [B, C]: out = scale * avg + shift (pooled GroupNorm output).
    src32: fp32, or 16-bit in the current operand format (the fused path's raw latent heads)."""
    L = _lib.load()
    src_bytes = src32.element_size()
    if src_bytes == 4:
        args = (_p(src32), _p(scale), _p(shift), _p(dst16), _p(dst32), B, Tin, Tout, C, ld_src, ld_dst, _dt(), _stream())
        fn = L.sfm_pool_time_affine
    else:
        args = (_p(src32), _DT_ID[src32.dtype], _p(scale), _p(shift), _p(dst16), _p(dst32), B, Tin, Tout, C, ld_src, ld_dst,
                _dt(), _stream())
        fn = L.sfm_pool_time_affine16
    _call("pool_time", fn, args, 0.0, pool_time_bytes(B, Tin, Tout, C, src_bytes))


def stft_lognorm_pack(re, im, dst16, M, F, zpad, ld_dst):
    L = _lib.load()
    _call("stft_lognorm_pack", L.sfm_stft_lognorm_pack, (_p(re), _p(im), _p(dst16), M, F, zpad, ld_dst, _dt(), _stream()),
          0.0, M * F * (8 + 4))


def polar_mask(lm, lp, B, rows, F, phase_scale, ld_logits, mag_bias=None, nr=None, ni=None, mr=None, mi=None, er=None,
               ei=None, mmag=None, ld_enh=0):
    L = _lib.load()
    _call("polar_mask", L.sfm_polar_mask, (_p(lm), _p(lp), _p(mag_bias), _p(nr), _p(ni), _p(mr), _p(mi), _p(er), _p(ei), _p(mmag), B,
                          rows, F, float(phase_scale), ld_logits, ld_enh, _stream()),
          20.0 * B * rows * F, B * rows * F * 4 * 8)


def complex_mul(sr, si, mr, mi):
    L = _lib.load()
    er, ei = torch.empty_like(sr), torch.empty_like(sr)
    _call("complex_mul", L.sfm_complex_mul, (_p(sr), _p(si), _p(mr), _p(mi), _p(er), _p(ei), sr.numel(), _stream()))
    return er, ei


def istft_ola(frames, win2, out, B, T, Ln, n_fft, hop, win, ld_frames):
    L = _lib.load()
    _call("istft_ola", L.sfm_istft_ola, (_p(frames), _p(win2), _p(out), B, T, Ln, n_fft, hop, win, ld_frames, _stream()),
          0.0, B * Ln * 12)


# ---------------------------------------------------------------------------
# packed (variable-length) batches: B utterances back to back, no padding.  Rows of utterance u = [frame_off[u], frame_off[u + 1])
# of every [sum_T, ...] matrix, its samples = [samp_off[u], samp_off[u + 1]) of the packed waveform; the offsets are int32 device
# tensors (functional.PackedSegments uploads them with the two work tables below in one copy).
# ---------------------------------------------------------------------------
ATTN_QTILE = _K["ATTN_QTILE"]       # query rows of a workgroup of attn_fwd_hd64_kernel
DWCONV_TILE = _K["DWCONV_TILE"]     # frames of a workgroup of the register-resident depthwise kernels
_XCDS, _XCD_RUN = _K["XCDS"], _K["XCD_RUN"]


def attention_items(frame_counts, H):
    """work table of sfm_attention_fwd_varlen at head_dim 64: int32 [n, 4] = (utterance, head, query tile, 0), one row per
    workgroup, only the tiles that exist.  Logical order: longest key range first (the long items start first, the short ones
    fill the tail), the tiles of one (utterance, head) adjacent.  Workgroups are dealt round-robin over the 8 XCDs, so within
    every run of 64 the table is dealt the way the dense kernel maps its block ids: XCD x takes 8 consecutive logical items,
    and the tiles that share one (utterance, head)'s K / V share an L2."""
    T = np.asarray(frame_counts, dtype=np.int64)
    order = np.argsort(-T, kind="stable")
    nt = (T[order] + ATTN_QTILE - 1) // ATTN_QTILE                   # tiles per (utterance, head), in logical order
    per = np.repeat(nt, H)                                           # ... per (utterance, head) pair
    n = int(per.sum())
    utt = np.repeat(np.repeat(order, H), per)
    head = np.repeat(np.tile(np.arange(H), len(T)), per)
    first = np.repeat(np.cumsum(per) - per, per)
    tile = np.arange(n) - first
    logical = np.stack([utt, head, tile, np.zeros(n, dtype=np.int64)], axis=1)
    run = _XCDS * _XCD_RUN
    pos = np.arange(n)
    base = pos // run * run
    total = np.minimum(run, n - base)                                # items of the position's run (the last one may be short)
    p = pos - base
    q, r, xcd, slot = total // _XCDS, total % _XCDS, p % _XCDS, p // _XCDS
    src = base + np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + slot
    return np.ascontiguousarray(logical[src], dtype=np.int32)


def dwconv_tiles(frame_counts):
    """work table of sfm_dwconv_folded_varlen: int32 [n, 2] = (utterance, 64-frame tile of that utterance)"""
    T = np.asarray(frame_counts, dtype=np.int64)
    nt = (T + DWCONV_TILE - 1) // DWCONV_TILE
    n = int(nt.sum())
    utt = np.repeat(np.arange(len(T)), nt)
    tile = np.arange(n) - np.repeat(np.cumsum(nt) - nt, nt)
    return np.ascontiguousarray(np.stack([utt, tile], axis=1), dtype=np.int32)


def framed_gemm_varlen(sig, Wt, out, samp_off, frame_off, *, B, sum_T, hop, padl, K, N, ldm, ldn=1, mode=0, out2=None, nsplit=0):
    """framed_gemm on packed signals sig [sum_L] -> packed rows out [sum_T, ldm]"""
    _need_dev(sig, Wt, out, samp_off, frame_off)
    L = _lib.load()
    Kpad, Npad = Wt.shape
    _call("framed_gemm_f32_varlen", L.sfm_framed_gemm_f32_varlen,
          (_p(sig), _p(Wt), _p(out), _p(out2), _p(samp_off), _p(frame_off), B, sum_T, hop, padl, K, Kpad, N, Npad, nsplit, ldm, ldn,
           mode, 1 if out.dtype == torch.float32 else 0, _dt(), _stream()),
          2.0 * sum_T * N * K, 4.0 * (sig.numel() + sum_T * N))
    return out


def framed_gemm_split16_varlen(sig, W, out, samp_off, frame_off, *, B, sum_T, hop, padl, ldm, mode=0, out2=None, nsplit=0,
                               col2_off=0):
    """framed_gemm_split16 on packed signals; W = pack_split16_matrix(...)"""
    _need_dev(sig, out, samp_off, frame_off)
    L = _lib.load()
    hi, lo, K, N = W
    Npad, Kpad = hi.shape
    _call("framed_gemm_split16_varlen", L.sfm_framed_gemm_split16_varlen,
          (_p(sig), _p(hi), _p(lo), _p(out), _p(out2), _p(samp_off), _p(frame_off), B, sum_T, hop, padl, K, Kpad, N, Npad, nsplit,
           col2_off, ldm, mode, _stream()),
          2.0 * sum_T * K * N, 4.0 * (sig.numel() + sum_T * N))
    return out


def attention_varlen(qkv16, frame_off, items, B, max_T, sum_T, H, hd, out=None, prescaled=False, out_dtype=None, sum_T2=None):
    """attention() on packed rows: qkv16 [sum_T, 3*H*hd] (q | k | v) -> [sum_T, H*hd], every utterance over its own rows.
    items: device copy of attention_items(frame_counts, H) (head_dim 64; None otherwise).  sum_T2 = sum of T_i^2, for the
    profiler's FLOP count only."""
    _need_dev(qkv16, frame_off, items)
    L = _lib.load()
    D = H * hd
    ld = qkv16.stride(0)
    if qkv16.dtype != _state["dtype"]:
        raise RuntimeError("attention: Q | K | V are %s, the stage's format is %s" % (qkv16.dtype, _state["dtype"]))
    if out is None:
        out = torch.empty(sum_T, D, device=qkv16.device, dtype=out_dtype or qkv16.dtype)
    n_items = 0 if items is None else items.shape[0]
    _call("attention_fwd_varlen", L.sfm_attention_fwd_varlen,
          (_p(qkv16), _p(out), _p(frame_off), _p(items), n_items, B, max_T, sum_T, H, hd, ld, out.stride(0), D, 2 * D,
           (-1.0 if prescaled else 1.0 / math.sqrt(hd)), _dt(), _DT_ID[out.dtype], _stream()),
          4.0 * H * hd * float(sum_T2 if sum_T2 is not None else 0), 4.0 * sum_T * D * 2)
    return out


def dwconv_folded_varlen(x16, wT, sc, sh, frame_off, tiles, B, max_T, sum_T, C, out=None, act=1):
    """dwconv_folded() on packed rows [sum_T, C]: zero edge at each utterance's own first and last frame.
    tiles: device copy of dwconv_tiles(frame_counts)."""
    _need_dev(x16, frame_off, tiles)
    L = _lib.load()
    KS = wT.shape[0]
    if out is None:
        out = torch.empty_like(x16)
    _call("dwconv_varlen", L.sfm_dwconv_folded_varlen,
          (_p(x16), _p(wT), _p(sc), _p(sh), _p(out), _p(frame_off), _p(tiles), 0 if tiles is None else tiles.shape[0], B, max_T,
           sum_T, C, KS, int(act), 1 if out.dtype == torch.float32 else 0, _dt(), _stream()),
          2.0 * sum_T * C * KS, sum_T * C * 4.0)
    return out


# ---- training on packed rows: the three launches of a Conformer block's training step that see (B, T) -------------------------
WGRAD_PARTIALS, WGRAD_MIN_SPAN = 2048, 32      # sfm_dwconv_wgrad's own aim: ~2048 partials, no span under 32 frames


def dwconv_wgrad_spans(frame_counts):
    """work table of sfm_dwconv_wgrad_varlen: int32 [n, 3] = (utterance, first frame, frame count), in utterance order.  Every
    frame of every utterance lies in exactly one span and no span crosses an utterance.  Spans are cut for about WGRAD_PARTIALS
    partials over the pack and at least WGRAD_MIN_SPAN frames each (an utterance's frames split evenly over its spans), which
    on equal lengths is the dense launcher's own cut; n <= WGRAD_PARTIALS + B."""
    T = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    if T.size == 0 or int(T.min()) < 1:
        raise ValueError("dwconv_wgrad_spans: at least one utterance and one frame per utterance")
    span = max(WGRAD_MIN_SPAN, -(-int(T.sum()) // WGRAD_PARTIALS))
    per = -(-T // (-(-T // span)))                                   # frames per span of each utterance: an even split
    n = -(-T // per)
    utt = np.repeat(np.arange(T.size), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    first = k * per[utt]
    count = np.minimum(per[utt], T[utt] - first)
    return np.ascontiguousarray(np.stack([utt, first, count], axis=1), dtype=np.int32)


def _packed_attention_ok(qkv16, frame_off, items, B, max_T, sum_T, H, hd):
    """the operands the packed training attention launches share: 16-bit rows [sum_T, >= 3 H hd] in the stage's format, the
    offsets and the head_dim-64 item table"""
    return (hd == 64 and H > 0 and 0 < B and 0 < max_T <= sum_T and
            _is(qkv16, _state["dtype"], (sum_T, None), contig="last") and qkv16.shape[1] >= 3 * H * hd and
            _is(frame_off, _I32, B + 1) and _is(items, _I32, (None, 4)))


def attention_train_varlen(qkv16, frame_off, items, B, max_T, sum_T, H, hd, p_drop=0.0, seed=0, sum_T2=None, lse=None):
    """attention_train() on packed rows (q pre-scaled, head_dim 64): qkv16 [sum_T, 3 H hd] -> O [sum_T, H hd] 16-bit and LSE
    [H, sum_T] fp32 (log2 domain; `lse`: a buffer of at least that many elements to write it into).  items: device copy of
    attention_items(frame_counts, H).  Dropout hashes row H * frame_off[u] + h * T_u + q: an equal-length pack is the dense
    launch bit for bit.  sum_T2 = sum of T_u^2, for the stated cost."""
    _need_dev(qkv16, frame_off, items, lse)
    L = _lib.load()
    D = H * hd
    _ragged_check("attention_train_varlen", _packed_attention_ok(qkv16, frame_off, items, B, max_T, sum_T, H, hd) and
                  0.0 <= p_drop < 1.0 and _is(lse, _F32, least=H * sum_T, opt=True))
    out = torch.empty(sum_T, D, device=qkv16.device, dtype=qkv16.dtype)
    lse = torch.empty(H, sum_T, device=qkv16.device, dtype=torch.float32) if lse is None else lse
    _call("attention_fwd_varlen", L.sfm_attention_fwd_train_varlen,
          (_p(qkv16), _p(out), _p(lse), _p(frame_off), _p(items), items.shape[0], B, max_T, sum_T, H, hd, qkv16.stride(0),
           out.stride(0), D, 2 * D, -1.0, float(p_drop), int(seed) & 0xffffffff, _dt(), _stream()),
          4.0 * H * hd * float(sum_T2 if sum_T2 is not None else 0), 4.0 * sum_T * D * 2)
    return out, lse


def attention_bwd_varlen(qkv16, O16, dO16, lse, frame_off, items, B, max_T, sum_T, H, hd, p_drop=0.0, seed=0, sum_T2=None,
                         delta=None):
    """attention_bwd() on packed rows (head_dim 64): -> dqkv like qkv16.  lse [H, sum_T] from attention_train_varlen, same
    p_drop and seed; delta: the [H, sum_T] fp32 workspace (a buffer of at least that many elements), fresh when None."""
    _need_dev(qkv16, O16, dO16, lse, frame_off, items, delta)
    L = _lib.load()
    D = H * hd
    dt = _state["dtype"]
    _ragged_check("attention_bwd_varlen", _packed_attention_ok(qkv16, frame_off, items, B, max_T, sum_T, H, hd) and
                  0.0 <= p_drop < 1.0 and _is(O16, dt, (sum_T, None), contig="last") and O16.shape[1] >= D and
                  _is(dO16, dt, (sum_T, None), contig="last") and dO16.shape[1] >= D and O16.stride(0) == dO16.stride(0) and
                  _is(lse, _F32, least=H * sum_T) and _is(delta, _F32, least=H * sum_T, opt=True))
    dqkv = torch.empty_like(qkv16)
    delta = torch.empty(H, sum_T, device=qkv16.device, dtype=torch.float32) if delta is None else delta
    _call("attention_bwd_varlen", L.sfm_attention_bwd_varlen,
          (_p(qkv16), _p(O16), _p(dO16), _p(lse), _p(delta), _p(dqkv), _p(frame_off), _p(items), items.shape[0], B, max_T, sum_T,
           H, hd, qkv16.stride(0), O16.stride(0), D, 2 * D, float(p_drop), int(seed) & 0xffffffff, _dt(), _stream()),
          10.0 * H * hd * float(sum_T2 if sum_T2 is not None else 0), 8.0 * sum_T * D * 2)
    return dqkv


def dwconv_wgrad_varlen(x16, dy32, frame_off, spans, B, sum_T, C, KS, dw=None, db=None):
    """dwconv_wgrad() on packed rows x16 / dy32 [sum_T, C]: -> dw [C, KS], db [C] (accumulated into dw / db when given), each
    utterance's window zero outside its own frames.  spans: device copy of dwconv_wgrad_spans(frame_counts)."""
    _need_dev(x16, dy32, frame_off, spans, dw, db)
    L = _lib.load()
    _ragged_check("dwconv_wgrad_varlen", KS in (7, 31) and C > 0 and C % 2 == 0 and 0 < B <= sum_T and
                  _is(x16, _state["dtype"], (sum_T, C)) and _is(dy32, _F32, (sum_T, C)) and _is(frame_off, _I32, B + 1) and
                  _is(spans, _I32, (None, 3)) and B <= spans.shape[0] <= min(sum_T, 65535) and
                  _is(dw, _F32, (C, KS), opt=True) and _is(db, _F32, (C,), opt=True))
    n = spans.shape[0]
    dw = torch.zeros(C, KS, device=x16.device, dtype=torch.float32) if dw is None else dw
    db = torch.zeros(C, device=x16.device, dtype=torch.float32) if db is None else db
    floats = int(L.sfm_dwconv_wgrad_varlen_scratch_floats(n, C, KS))       # (a negative count is the launcher's status)
    _lib.check(min(floats, 0), "dwconv_wgrad_varlen")
    scratch = torch.empty(floats, device=x16.device, dtype=torch.float32)
    _call("dwconv_wgrad_varlen", L.sfm_dwconv_wgrad_varlen,
          (_p(x16), _p(dy32), _p(dw), _p(db), _p(scratch), _p(frame_off), _p(spans), n, B, sum_T, C, KS, _dt(), _stream()),
          2.0 * sum_T * C * (KS + 1), sum_T * C * 6.0 + n * (KS + 1) * C * 8.0)
    return dw, db


def istft_ola_varlen(frames, win2, out, frame_off, samp_off, B, n_fft, hop, win, ld_frames):
    """istft_ola() on packed frames [sum_T, ld_frames] -> packed samples out [sum_L]"""
    _need_dev(frames, out, frame_off, samp_off)
    L = _lib.load()
    _call("istft_ola_varlen", L.sfm_istft_ola_varlen,
          (_p(frames), _p(win2), _p(out), _p(frame_off), _p(samp_off), B, out.numel(), n_fft, hop, win, ld_frames, _stream()),
          0.0, out.numel() * 12.0)
    return out


# ---------------------------------------------------------------------------
# The ragged front end: the dense front-end kernels with a length per row.  Buffers have the dense layout of
# the LONGEST row; the tables are int32 device tensors that functional.ragged_plan builds once per lengths tuple.  Costs are
# stated over the valid rows (`n_*` = their sums over the batch, host integers of the plan), as the dense wrappers state theirs.
# ---------------------------------------------------------------------------
def _ragged_check(name, ok):
    """the ragged wrappers' refusal: the one predicate's verdict `ok`, answered like every checking wrapper (_refuse)"""
    if not ok:
        _refuse(name)


def sinc_fir16_varlen(wave, lengths, filt, out, C, K, n_valid, passes=0):
    """sinc_fir16 (one pass, resident taps) on wave [B, Lrow] with lengths[b] valid samples per row -> out [B, Lrow, C] rows below
    lengths[b], and the zero-filled GroupNorm partials [B, P, 8, 2] whose slots past a row's last tile stay zero."""
    _need_dev(wave, lengths, filt, out)
    Lb = _lib.load()
    _ragged_check("sinc_fir16_varlen", _is(wave, _F32, ndim=2, least=1) and wave.shape[0] <= 65535 and
                  _lengths_ok(lengths, wave.shape[0]) and lengths is not None and _is(filt, _F32, (C, K)) and
                  _is(out, None, (wave.shape[0], wave.shape[1], C)) and out.dtype in (_state["dtype"], _F32))
    B, Lrow = wave.shape
    wsh = torch.empty(_K["SINC_FIR16_WS_WORDS"], device=wave.device, dtype=torch.int16)
    P = Lb.sfm_sinc_fir16_tiles(Lrow)
    part = torch.zeros(B, P, 8, 2, device=wave.device, dtype=torch.float32)
    out_f32 = 1 if out.dtype == torch.float32 else 0
    _call("sinc_fir16", Lb.sfm_sinc_fir16_varlen, (_p(wave), _p(lengths), _p(filt), _p(wsh), _p(out), _p(part), B, Lrow, C, K, out_f32,
                                                   _dt(), int(passes), _stream()),
          2.0 * n_valid * C * K, n_valid * 4 + n_valid * C * (4 if out_f32 else 2))
    return part, P


def conv16p_varlen(x1, sc1, sh1, pw, out, lin_tab, lout_tab, *, B, Lin, stride, pad, n_out, x2=None, sc2=None, sh2=None,
                   gn_partial=None, gn_group=0, skip_pw=None, out_s=None, gn_partial_s=None):
    """conv16p with lin_tab[b] input rows and lout_tab[b] output rows per utterance inside buffers of row counts Lin / Lout;
    gn_partial (_s) zero-filled by the caller.  n_out: the sum of lout_tab (host), for the cost."""
    _need_dev(x1, out, lin_tab, lout_tab)
    L = _lib.load()
    cin, N, ks = pw.cin, pw.N, pw.ksize
    dt = _state["dtype"]
    Lout = (Lin + 2 * pad - ks) // stride + 1
    _ragged_check("conv16p_varlen", _is(x1, dt, (B, Lin, cin)) and _is(x2, dt, (B, Lin, cin), opt=True) and pw.w.dtype is dt and
                  _each(_F32, B * cin, sc1, sh1) and (x2 is None or _each(_F32, B * cin, sc2, sh2)) and
                  _lengths_ok(lin_tab, B) and _lengths_ok(lout_tab, B) and lin_tab is not None and lout_tab is not None and
                  _is(out, None, (B, Lout, N)) and _is(out_s, out.dtype, (B, Lout, N), opt=True) and
                  pw.Npad == N and pw.Kpad == ks * cin and (skip_pw is None or (skip_pw.Npad == N and skip_pw.Kpad == cin)))
    out_f32 = 1 if out.dtype == torch.float32 else (0 if out.dtype == dt else 2)
    nin = 2 if x2 is not None else 1
    n_in = n_out * stride
    flops = 2.0 * n_out * N * (ks * cin + (cin if skip_pw is not None else 0))
    nbytes = n_in * cin * 2.0 * nin + n_out * N * out.element_size() * (2 if skip_pw is not None else 1) + N * ks * cin * 2.0
    _call("conv16p", L.sfm_conv16p_varlen,
          (_p(x1), _p(sc1), _p(sh1), _p(x2), _p(sc2), _p(sh2), _p(pw.w), _p(pw.bias), _p(out), _p(gn_partial),
           _p(skip_pw.w if skip_pw is not None else None), _p(skip_pw.bias if skip_pw is not None else None), _p(out_s),
           _p(gn_partial_s), _p(lin_tab), _p(lout_tab), B, Lin, cin, N, ks, stride, pad, out_f32, gn_group, _dt(), _stream()),
          flops, nbytes, tag="Lout%d Cin%d N%d k%d s%d in%d%s varlen" % (n_out, cin, N, ks, stride, nin,
                                                                       " +skip" if skip_pw is not None else ""))
    return out


def gn_finalize_varlen(partial, w, b, rows_tab, p_tab, Bn, Pmax, G, C, eps=1e-5):
    """gn_finalize with rows_tab[b] rows and p_tab[b] partial slots per utterance (partial [Bn, Pmax, G, 2]) -> scale, shift [Bn, C]"""
    _need_dev(partial, w, b, rows_tab, p_tab)
    L = _lib.load()
    _ragged_check("gn_finalize_varlen", _is(partial, _F32, Bn * Pmax * G * 2) and _each(_F32, C, w, b) and G > 0 and C % G == 0 and
                  _lengths_ok(rows_tab, Bn) and _lengths_ok(p_tab, Bn) and rows_tab is not None and p_tab is not None)
    scale = torch.empty(Bn, C, device=w.device, dtype=torch.float32)
    shift = torch.empty(Bn, C, device=w.device, dtype=torch.float32)
    _call("gn_finalize", L.sfm_gn_finalize_varlen, (_p(partial), _p(w), _p(b), _p(scale), _p(shift), _p(rows_tab), _p(p_tab), Bn, Pmax,
                                                    G, C, eps, _stream()), 0.0, 8.0 * Bn * C)
    return scale, shift


def gn_apply_varlen(x1, sc1, sh1, out, rows_tab, Bn, rows, C, n_valid):
    """gn_apply(act=1) on 16-bit rows x1 [Bn, rows, C] -> out of the same shape and format: the rows below rows_tab[b] as gn_apply,
    zeros from there on (never read)"""
    _need_dev(x1, out, rows_tab)
    L = _lib.load()
    dt = _state["dtype"]
    _ragged_check("gn_apply_varlen", _is(x1, dt, (Bn, rows, C)) and _is(out, dt, (Bn, rows, C)) and _each(_F32, Bn * C, sc1, sh1) and
                  _lengths_ok(rows_tab, Bn) and rows_tab is not None and 64 <= C <= 2048 and C & (C - 1) == 0)
    _call("gn_apply", L.sfm_gn_apply_varlen, (_p(x1), _p(sc1), _p(sh1), _p(out), _p(rows_tab), Bn, rows, C, _dt(), _stream()),
          10.0 * n_valid * C, n_valid * C * 2 + Bn * rows * C * 2)
    return out


def headpool_tab(Tin, Tout):
    """host table of sfm_headpool_varlen: int32 [B, 4] = (Tin_b, Tout_b, frames per tile, tiles), by sfm_headpool_frames_per_tile;
    None when a pair is not supported or the fusion is switched off"""
    rows = []
    for ti, to in zip(Tin, Tout):
        t = headpool_tiles(int(ti), int(to))
        if t is None:
            return None
        rows.append((int(ti), int(to), t[0], t[1]))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def headpool_varlen(xd16, pw, pooled16, part, tab, B, TinS, ToutS, PS, n_in, n_out, gcols=16):
    """headpool with tab[b] = (Tin_b, Tout_b, frames per tile, tiles): xd16 [B, TinS, 256] -> pooled16 [B, ToutS, N] (zeros from
    Tout_b on), part [B, PS, N / gcols, 2] zero-filled by the caller.  n_in / n_out: the sums of Tin_b / Tout_b, for the cost."""
    _need_dev(xd16, pooled16, part, tab)
    L = _lib.load()
    dt = _state["dtype"]
    _ragged_check("headpool_varlen", _is(xd16, dt, (B, TinS, None)) and _is(pooled16, dt, (B, ToutS, None)) and pw.w.dtype is dt and
                  pooled16.shape[2] >= pw.Npad and _is(part, _F32, B * PS * (pw.Npad // gcols) * 2) and _is(tab, _I32, (B, 4)))
    _call("gemm16", L.sfm_headpool_varlen, (_p(xd16), _p(pw.w), _p(pw.bias), _p(pooled16), _p(part), _p(tab), B, TinS, ToutS, PS, pw.Npad,
                                            xd16.stride(1), pooled16.stride(1), gcols, _dt(), _stream()),
          2.0 * n_in * pw.Npad * 256, n_in * 512.0 + pw.Npad * 512.0 + B * ToutS * pw.Npad * 2.0,
          tag="M%d N%d K256 headpool->T%d varlen" % (n_in, pw.Npad, n_out))


def bilstm_layer_rows16_varlen(xg, whh, ttab, B, T, H, n_steps, out16=None):
    """bilstm_layer_rows16 with ttab[b] steps per chain inside rows of stride T; the rows from ttab[b] on are written as zeros.
    H 128 on fp16 recurrent operands only (the caller refuses the rest).  n_steps: the sum of ttab, for the cost."""
    _need_dev(xg, whh, ttab, out16)
    L = _lib.load()
    _ragged_check("bilstm_layer_rows16_varlen", H == 128 and _is(xg, _F32, B * T * 8 * H) and _is(whh, _F32, (2, 4 * H, H)) and
                  _lengths_ok(ttab, B) and ttab is not None and
                  _is(out16, _state["dtype"], (B * T, None), opt=True, contig="last"))
    if out16 is None:
        out16 = torch.empty(B * T, 2 * H, device=xg.device, dtype=compute_dtype())
    flops, nbytes = 2.0 * n_steps * 2 * 4 * H * H, n_steps * 8 * H * 4 + B * T * 2 * H * 2
    _call("bilstm_layer", L.sfm_bilstm_layer_rows16_varlen, (_p(xg), _p(whh), _p(out16), out16.stride(0), _p(ttab), B, T, H, 1, _dt(),
                                                             _stream()), flops, nbytes)
    return out16


def rows_gather32(src, dst, rows_tab, dst_off, B, src_rows, width, n_rows):
    """the hand-over from the padded to the packed layout: the first `width` elements of row r < rows_tab[b] of src [B * src_rows, ld]
    -> row dst_off[b] + r of dst [n_rows, ld'].  src and dst hold the same element type (4 bytes, or 2 with an even width)."""
    _need_dev(src, dst, rows_tab, dst_off)
    L = _lib.load()
    per = 4 // src.element_size() if src is not None and src.element_size() in (2, 4) else 0
    ok = (per > 0 and _is(src, dst.dtype if dst is not None else None, contig="last", ndim=2, rows=B * src_rows) and
          _is(dst, src.dtype, (n_rows, None), contig="last") and width % per == 0 and src.stride(0) % per == 0 and
          dst.stride(0) % per == 0 and 0 < width <= min(src.shape[1], dst.shape[1]) and
          _lengths_ok(rows_tab, B) and rows_tab is not None and _is(dst_off, _I32, least=B))
    _ragged_check("rows_gather32", ok)
    _call("rows_gather", L.sfm_rows_gather32, (_p(src), _p(dst), _p(rows_tab), _p(dst_off), B, src_rows, width // per,
                                               src.stride(0) // per, dst.stride(0) // per, _stream()),
          0.0, 2.0 * n_rows * width * src.element_size())
    return dst


def pack_spec(re, im, dst, M, F, ld, ld_src):
    L = _lib.load()
    _call("pack_spec", L.sfm_pack_spec, (_p(re), _p(im), _p(dst), M, F, ld, ld_src, _stream()))


def sinc_filters(low_hz, band_hz, window, n_, C, K, sample_rate, min_low_hz, min_band_hz, want_filt=True):
    L = _lib.load()
    dev = low_hz.device
    Npad = round_up(C, 64)
    Wt = torch.zeros(round_up(K, 32), Npad, device=dev, dtype=torch.float32)
    filt = torch.empty(C, K, device=dev, dtype=torch.float32) if want_filt else None
    _call("sinc_filters", L.sfm_sinc_filters, (_p(low_hz), _p(band_hz), _p(window), _p(n_), _p(filt), _p(Wt), C, K, Npad,
                            float(sample_rate), float(min_low_hz), float(min_band_hz), _stream()))
    return filt, Wt


def ffn_fused(x32, lnw, lnb, w1_16, b1, w2_16, b2, alpha=0.5, eps=1e-5, out=None):
    """FeedForwardModule in one launch: x32 [M, 256] fp32 -> [M, 256] fp32."""
    _need_dev(x32)
    Lb = _lib.load()
    M, D = x32.shape
    FF = w1_16.shape[0]
    if out is None:
        out = torch.empty_like(x32)
    _call("ffn_fused", Lb.sfm_ffn_fused, (_p(x32), _p(lnw), _p(lnb), _p(w1_16), _p(b1), _p(w2_16), _p(b2), _p(out), M, D, FF,
                                          float(alpha), float(eps), _dt(), _stream()), 4.0 * M * D * FF, M * D * 8.0)
    return out


def ffn_fused_ln(x32, lnw, lnb, w1_16, b1, w2_16, b2, ln2w, ln2b, ln_f32, want_y=True, alpha=0.5, eps=1e-5):
    """ffn_fused + the LayerNorm that follows the module (ln2w / ln2b) applied in the epilogue.
    Returns (y fp32 or None, LN(y) as fp32 or 16-bit)."""
    _need_dev(x32)
    Lb = _lib.load()
    M, D = x32.shape
    FF = w1_16.shape[0]
    y = torch.empty_like(x32) if want_y else None
    ln = torch.empty(M, D, device=x32.device, dtype=torch.float32 if ln_f32 else _state["dtype"])
    _call("ffn_fused", Lb.sfm_ffn_fused_ln, (_p(x32), _p(lnw), _p(lnb), _p(w1_16), _p(b1), _p(w2_16), _p(b2), _p(y), M, D, FF,
                                             float(alpha), float(eps), _p(ln2w), _p(ln2b), _p(ln), 1 if ln_f32 else 0, _dt(),
                                             _stream()), 4.0 * M * D * FF, M * D * (8.0 if want_y else 4.0) + M * D * (4.0 if ln_f32 else 2.0))
    return y, ln


def set_sinc_fir_resident(flag):
    """True (default): the one-pass sinc FIR keeps a shift's taps in registers (sinc_fir16_resident_kernel).  False: the
    streaming one-pass kernel with the taps in LDS computes it - the same out and gn_partial bit for bit (A/B, reference)."""
    _SWITCHES["sinc_fir_resident"][2] = bool(flag)


def sinc_fir16(wave, filt, out, B, L, C, K, want_stats=True, passes=0):
    """SincConv1d FIR on 16-bit operands -> out [B, L, C] channels-last (+ GroupNorm partials).  passes: 3 = split operands
    (fp32-class accuracy), 1 = operands rounded once, 0 = auto (1 for fp16 operands with a 16-bit result, else 3)."""
    Lb = _lib.load()
    dev = wave.device
    wsh = torch.empty(_K["SINC_FIR16_WS_WORDS"], device=dev, dtype=torch.int16)
    P = Lb.sfm_sinc_fir16_tiles(L)
    part = torch.zeros(B, P, 8, 2, device=dev, dtype=torch.float32) if want_stats else None
    out_f32 = 1 if out.dtype == torch.float32 else 0
    if not switch("sinc_fir_resident") and (passes == 1 or (passes == 0 and _dt() == _K["DT_F16"] and not out_f32)):
        passes = _K["SINC_FIR16_STREAM1"]               # wherever one pass is asked for or chosen (the launcher's own auto rule)
    flops, nbytes = 2.0 * B * L * C * K, B * L * 4 + B * L * C * (4 if out_f32 else 2)
    _call("sinc_fir16", Lb.sfm_sinc_fir16_ex, (_p(wave), _p(filt), _p(wsh), _p(out), _p(part), B, L, C, K, out_f32, _dt(), int(passes),
                                               _stream()), flops, nbytes)
    return part, P


def wave_moments(est, tgt):
    L = _lib.load()
    B, Ln = est.shape
    S = torch.zeros(B, 5, device=est.device, dtype=torch.float64)
    _call("loss_reduce", L.sfm_wave_moments, (_p(est), _p(tgt), _p(S), B, Ln,
                                              _p(_ws(L.sfm_wave_moments_ws_doubles(B, Ln), est.device, torch.float64)), _stream()),
          0.0, 8.0 * B * Ln)
    return S


def wave_moments_varlen(est, tgt, samp_off, B, max_L):
    """wave_moments of packed signals est, tgt [sum_L] -> S [B, 5] fp64 (the fp64-atomics form)"""
    _need_dev(est, tgt, samp_off)
    L = _lib.load()
    S = torch.zeros(B, 5, device=est.device, dtype=torch.float64)
    _call("loss_reduce", L.sfm_wave_moments_varlen, (_p(est), _p(tgt), _p(S), _p(samp_off), B, int(max_L), _stream()), 0.0,
          8.0 * est.numel())
    return S


def ssnr_frames_varlen(clean, enh, samp_off, frame_off, B, sum_frames, frame, hop, upper=35.0, lower=-10.0):
    """packed clean / enh [sum_L] -> acc [B, 2] fp64 = {sum of the clipped SNRs of the non-silent frames, their count}"""
    _need_dev(clean, enh, samp_off, frame_off)
    L = _lib.load()
    acc = torch.zeros(B, 2, device=clean.device, dtype=torch.float64)
    _call("metrics", L.sfm_ssnr_frames_varlen, (_p(clean), _p(enh), _p(acc), _p(samp_off), _p(frame_off), B, int(sum_frames),
                                                int(frame), int(hop), float(upper), float(lower), _stream()), 0.0,
          8.0 * clean.numel() * frame / hop)
    return acc


def stoi_frames_varlen(cr, ci, er, ei, sc, se, frame_off, B):
    """packed spectra rows [sum_frames, F], sc / se [B] fp64 -> acc [B] fp64 = sum of the clipped frame correlations"""
    _need_dev(cr, ci, er, ei, sc, se, frame_off)
    L = _lib.load()
    n, F = cr.shape
    acc = torch.zeros(B, device=cr.device, dtype=torch.float64)
    _call("metrics", L.sfm_stoi_frames_varlen, (_p(cr), _p(ci), _p(er), _p(ei), _p(sc), _p(se), _p(acc), _p(frame_off), B, n, F,
                                                _stream()), 0.0, 16.0 * n * F)
    return acc


def lsd_frames(cr, ci, er, ei):
    """spectra [B, nframes, F] -> acc [B] fp64 = sum over the frames of the log-spectral distortion"""
    _need_dev(cr, ci, er, ei)
    L = _lib.load()
    B, n, F = cr.shape
    acc = torch.zeros(B, device=cr.device, dtype=torch.float64)
    _call("metrics", L.sfm_lsd_frames, (_p(cr), _p(ci), _p(er), _p(ei), _p(acc), B, n, F, _stream()), 0.0, 16.0 * B * n * F)
    return acc


def lsd_frames_varlen(cr, ci, er, ei, frame_off, B):
    """packed spectra rows [sum_frames, F] -> acc [B] fp64"""
    _need_dev(cr, ci, er, ei, frame_off)
    L = _lib.load()
    n, F = cr.shape
    acc = torch.zeros(B, device=cr.device, dtype=torch.float64)
    _call("metrics", L.sfm_lsd_frames_varlen, (_p(cr), _p(ci), _p(er), _p(ei), _p(acc), _p(frame_off), B, n, F, _stream()), 0.0,
          16.0 * n * F)
    return acc


def _ws64(n, device):
    """float64 scratch of >= n elements for an entry point that has no atomics form (the ordered fold is its only path)"""
    t = _ws(n, device, torch.float64)
    return t if t is not None else torch.empty(int(n), device=device, dtype=torch.float64)


PSTOI_MAX_BANDS, PSTOI_MAX_BINS = _K["PSTOI_MAX_BANDS"], _K["PSTOI_MAX_BINS"]             # sfm_pstoi_loss: NB, F
PSTOI_MIN_FRAME_LEN, PSTOI_MAX_FRAME_LEN = _K["PSTOI_MIN_FRAME_LEN"], _K["PSTOI_MAX_FRAME_LEN"]


def pstoi_loss(enh, clean, band_w, need_grad=False, frame_len=30, beta=15.0):
    """PerceptualSTOILoss (training/losses.py:89-143) in one launch.  enh / clean: fp32 contiguous magnitudes [B, F, T], or
    (real, imag) pairs of channels-last [B, T, F] tensors; band_w [NB, F].  -> (loss [1] fp32, gradient to enh or None: one
    tensor or a (real, imag) pair, every element written)."""
    pair = isinstance(enh, (tuple, list))
    e0, e1 = enh if pair else (enh, None)
    c0, c1 = clean if pair else (clean, None)
    _need_dev(e0, e1, c0, c1, band_w)
    L = _lib.load()
    FL = int(frame_len)
    if not (_is(e0, None, ndim=3, contig=False) and
            _is(c0, None, tuple(e0.shape), contig=False) and
            _is(band_w, None, (None, e0.shape[2 if pair else 1]), contig=False) and
            band_w.shape[0] <= PSTOI_MAX_BANDS and band_w.shape[1] <= PSTOI_MAX_BINS and
            PSTOI_MIN_FRAME_LEN <= FL <= PSTOI_MAX_FRAME_LEN and e0.shape[1 if pair else 2] >= FL):
        _refuse("pstoi_loss")
    B, T, F = e0.shape if pair else (e0.shape[0], e0.shape[2], e0.shape[1])
    NB = band_w.shape[0]
    loss = torch.empty(1, device=e0.device, dtype=torch.float32)
    g0 = torch.empty_like(e0) if need_grad else None
    g1 = torch.empty_like(e0) if need_grad and pair else None
    S = T // FL
    n = e0.numel()
    _call("pstoi_loss", L.sfm_pstoi_loss, (_p(e0), _p(e1), _p(c0), _p(c1), _p(band_w), _p(loss), _p(g0), _p(g1),
                                           _p(_ws64(L.sfm_pstoi_loss_ws_doubles(B, T, FL), e0.device)), B, T, F, NB, FL, float(beta),
                                           1 if pair else 0, _stream()),
          (6.0 if need_grad else 4.0) * NB * F * B * S * FL,
          pstoi_bytes(B, T, F, FL, pair, need_grad))
    return loss, ((g0, g1) if pair else g0) if need_grad else None


def pstoi_bytes(B, T, F, frame_len, pair, need_grad):
    """bytes one sfm_pstoi_loss launch has to move: each used input element read once (the pair form reads re, im of the
    enhanced side again for the gradient), each gradient element written once"""
    used, every = 4.0 * B * (T // frame_len) * frame_len * F, 4.0 * B * T * F
    if pair:
        return 4 * used + ((2 * used + 2 * every) if need_grad else 0.0)
    return 2 * used + (every if need_grad else 0.0)


def mse_loss(pred, target, need_grad=False):
    """nn.MSELoss() of two fp32 contiguous tensors of one shape -> (loss [1] fp32, 2 (pred - target) / n or None)"""
    _need_dev(pred, target)
    L = _lib.load()
    if not (_is(pred, None, least=1, contig=False) and _is(target, None, tuple(pred.shape), contig=False)):
        _refuse("mse_loss")
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    grad = torch.empty_like(pred) if need_grad else None
    n = pred.numel()
    _call("mse_loss", L.sfm_mse_loss, (_p(pred), _p(target), _p(loss), _p(grad), _p(_ws64(L.sfm_mse_loss_ws_doubles(n), pred.device)),
                                       n, _stream()),
          3.0 * n, (12.0 if need_grad else 8.0) * n)
    return loss, grad


# ---------------------------------------------------------------------------
# curriculum batches: mask targets and the SNR mix (csrc/masks.hip)
# ---------------------------------------------------------------------------
MIX_CHUNK = _K["MIX_CHUNK"]                    # samples per workgroup of sfm_mix_scale / sfm_mix_apply
QUANT_MAX_STEPS = _K["QUANT_MAX_STEPS"]        # sfm_mask_quantize
MASK_KINDS = {None: _K["MASK_NONE"], "irm": _K["MASK_IRM"], "pcirm": _K["MASK_PCIRM"], "opt_pcirm": _K["MASK_OPT_PCIRM"]}


def _planes_ok(first, *others):
    """non-empty fp32 contiguous tensors of one shape"""
    return _is(first, _F32, least=1) and all(_is(t, _F32, tuple(first.shape)) for t in others)


def mask_irm(clean_mag, noise_mag, p=0.5, eps=1e-10):
    """masks/irm.py:17-39 on two fp32 contiguous tensors of one shape -> fp32 tensor of that shape"""
    _need_dev(clean_mag, noise_mag)
    L = _lib.load()
    if not _planes_ok(clean_mag, noise_mag):
        _refuse("mask_irm")
    n = clean_mag.numel()
    out = torch.empty_like(clean_mag)
    _call("mask_irm", L.sfm_mask_irm, (_p(clean_mag), _p(noise_mag), _p(out), n, float(p), float(eps), _stream()),
          6.0 * n, 12.0 * n)
    return out


def mask_corr(noisy, clean, noise, eps=1e-10):
    """masks/pcirm.py:49-57, 70-72 per element -> (rho_s, rho_n)"""
    _need_dev(noisy, clean, noise)
    L = _lib.load()
    if not _planes_ok(noisy, clean, noise):
        _refuse("mask_corr")
    n = noisy.numel()
    rho_s, rho_n = torch.empty_like(noisy), torch.empty_like(noisy)
    _call("mask_corr", L.sfm_mask_corr, (_p(noisy), _p(clean), _p(noise), _p(rho_s), _p(rho_n), n, float(eps), _stream()),
          14.0 * n, 20.0 * n)
    return rho_s, rho_n


def mask_pcirm(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2, eps=1e-10):
    """masks/pcirm.py:122-131 per element"""
    _need_dev(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2)
    L = _lib.load()
    if not _planes_ok(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2):
        _refuse("mask_pcirm")
    n = clean_mag.numel()
    out = torch.empty_like(clean_mag)
    _call("mask_pcirm", L.sfm_mask_pcirm, (_p(clean_mag), _p(noise_mag), _p(rho_s), _p(rho_n), _p(phi1), _p(phi2), _p(out), n,
                                           float(eps), _stream()), 12.0 * n, 28.0 * n)
    return out


def mask_quantize(pcirm, table, M):
    """masks/opt_pcirm.py:79-101; table: float64 device tensor, M + 1 boundaries then M values (masks.opt_pcirm.quantizer_table)"""
    _need_dev(pcirm, table)
    L = _lib.load()
    if not (_planes_ok(pcirm) and
            _is(table, _F64, 2 * M + 1, contig=False) and 2 <= M <= QUANT_MAX_STEPS):
        _refuse("mask_quantize")
    n = pcirm.numel()
    out = torch.empty_like(pcirm)
    _call("mask_quantize", L.sfm_mask_quantize, (_p(pcirm), _p(table), _p(out), n, int(M), _stream()), 0.0, 8.0 * n)
    return out


def mix_scale(clean, bank, bank_off, noise_ids, snr_db, lengths=None):
    """clean [B, L] fp32 contiguous; bank fp32, bank_off int32 [n_noise + 1]; noise_ids int32 [B]; snr_db fp32 [B]; lengths int32
    [B] or None -> scale [B] fp32 (two launches: fp64 chunk sums, then the ordered fold)"""
    _need_dev(clean, bank, bank_off, noise_ids, snr_db, lengths)
    L = _lib.load()
    if not (_is(clean, _F32, ndim=2, contig=False) and
            _is(bank, _F32, contig=False) and
            _is(bank_off, _I32, least=2, contig=False) and
            _is(noise_ids, _I32, clean.shape[0], contig=False) and
            _is(snr_db, _F32, clean.shape[0], contig=False) and
            _is(lengths, _I32, clean.shape[0], opt=True, contig=False)):
        _refuse("mix_scale")
    B, Ln = clean.shape
    n_noise = bank_off.numel() - 1
    scale = torch.empty(B, device=clean.device, dtype=torch.float32)
    ws = _ws64(L.sfm_mix_scale_ws_doubles(B, Ln), clean.device)
    _call("mix", L.sfm_mix_scale, (_p(clean), _p(bank), _p(bank_off), _p(noise_ids), _p(snr_db), _p(lengths), _p(ws), _p(scale), B,
                                   Ln, n_noise, _stream()), 4.0 * B * Ln, 8.0 * B * Ln, "scale B%d L%d" % (B, Ln))
    return scale


def mix_apply(clean, bank, bank_off, noise_ids, scale, lengths=None, want_rows=False):
    """-> (noisy [B, L], the unscaled noise rows [B, L] or None); every element written"""
    _need_dev(clean, bank, bank_off, noise_ids, scale, lengths)
    L = _lib.load()
    if not (_is(clean, _F32, ndim=2, contig=False) and
            _is(bank, _F32, contig=False) and
            _is(bank_off, _I32, least=2, contig=False) and
            _is(noise_ids, _I32, clean.shape[0], contig=False) and
            _is(scale, _F32, clean.shape[0], contig=False) and
            _is(lengths, _I32, clean.shape[0], opt=True, contig=False)):
        _refuse("mix_apply")
    B, Ln = clean.shape
    noisy = torch.empty_like(clean)
    rows = torch.empty_like(clean) if want_rows else None
    _call("mix", L.sfm_mix_apply, (_p(clean), _p(bank), _p(bank_off), _p(noise_ids), _p(lengths), _p(scale), _p(noisy), _p(rows), B,
                                   Ln, bank_off.numel() - 1, _stream()), 2.0 * B * Ln, (16.0 if want_rows else 12.0) * B * Ln,
          "apply B%d L%d rows%d" % (B, Ln, 1 if want_rows else 0))
    return noisy, rows


def mix_scale_varlen(packed, utt_off, bank, bank_off, noise_ids, snr_db, max_len):
    """mix_scale on packed utterances: packed fp32 [total], utterance u = packed[utt_off[u] : utt_off[u + 1]] (int32 [U + 1]);
    noise_ids int32 [U], snr_db fp32 [U]; max_len = the longest utterance (a host int) -> scale [U] fp32.  Two launches per 65535
    utterances: fp64 chunk sums, then the ordered fold."""
    _need_dev(packed, utt_off, bank, bank_off, noise_ids, snr_db)
    L = _lib.load()
    if not (_is(packed, _F32, ndim=1, least=1) and packed.numel() < 2 ** 31 and
            _is(utt_off, _I32, ndim=1, least=2) and
            _is(bank, _F32, contig=False) and
            _is(bank_off, _I32, least=2, contig=False) and
            _is(noise_ids, _I32, utt_off.numel() - 1) and
            _is(snr_db, _F32, utt_off.numel() - 1)):
        _refuse("mix_scale_varlen")
    U = utt_off.numel() - 1
    total, n_noise, max_len = packed.numel(), bank_off.numel() - 1, int(max_len)
    scale = torch.empty(U, device=packed.device, dtype=torch.float32)
    for a in range(0, U, 65535):                    # (the utterances are the grid's y dimension)
        n = min(65535, U - a)
        need = L.sfm_mix_scale_varlen_ws_doubles(n, max_len)
        if need < 0:
            _lib.check(need, "mix_scale_varlen")
        ws = _ws64(need, packed.device)
        _call("mix", L.sfm_mix_scale_varlen, (_p(packed), _p(utt_off[a:]), _p(bank), _p(bank_off), _p(noise_ids[a:]), _p(snr_db[a:]),
                                              _p(ws), _p(scale[a:]), n, max_len, total, n_noise, _stream()),
              4.0 * total, 8.0 * total, "scale_varlen U%d L%d" % (n, max_len))
    return scale


def wave_batch(packed, utt_off, bank, bank_off, noise_ids, scale, index, L_out, out=None):
    """index int32 [B] into a packed set -> out fp32 [2, B, L_out]: out[0] the mixes packed[u] + scale[u] * noise (tiled / cut), out[1]
    the clean rows, both zero-padded; an index outside 0 .. U - 1 (-1) gives zero rows.  One launch, every element written."""
    _need_dev(packed, utt_off, bank, bank_off, noise_ids, scale, index, out)
    L = _lib.load()
    L_out = int(L_out)
    if not (_is(packed, _F32, ndim=1, least=1) and packed.numel() < 2 ** 31 and
            _is(utt_off, _I32, ndim=1, least=2) and
            _is(bank, _F32, contig=False) and
            _is(bank_off, _I32, least=2, contig=False) and
            _is(noise_ids, _I32, utt_off.numel() - 1) and
            _is(scale, _F32, utt_off.numel() - 1) and
            _is(index, _I32, ndim=1, least=1) and
            _is(out, _F32, (2, index.numel(), L_out), opt=True)):
        _refuse("wave_batch")
    U, B = utt_off.numel() - 1, index.numel()
    if out is None:
        out = torch.empty(2, B, L_out, device=packed.device, dtype=torch.float32)
    _call("mix", L.sfm_wave_batch, (_p(packed), _p(utt_off), _p(bank), _p(bank_off), _p(noise_ids), _p(scale), _p(index), _p(out), B,
                                    L_out, U, packed.numel(), bank_off.numel() - 1, _stream()),
          2.0 * B * L_out, 16.0 * B * L_out, "wave_batch B%d L%d" % (B, L_out))
    return out


def curriculum_mask(cr, ci, nr, ni, scale, kind=None, p=0.5, eps=1e-10, table=None, M=0):
    """spectra [B, T, F] of the clean utterances and of the noise rows, scale [B] -> (yr, yi, mask or None): the spectrum of
    the mix and the mask target `kind` (MASK_KINDS), one launch"""
    _need_dev(cr, ci, nr, ni, scale, table)
    L = _lib.load()
    k = MASK_KINDS[kind]
    if not (_is(cr, _F32, ndim=3) and _planes_ok(cr, ci, nr, ni) and
            _is(scale, _F32, cr.shape[0], contig=False) and
            (k != MASK_KINDS["opt_pcirm"] or _is(table, None, 2 * M + 1, contig=False))):
        _refuse("curriculum_mask")
    B, T, F = cr.shape
    yr, yi = torch.empty_like(cr), torch.empty_like(cr)
    mask = torch.empty_like(cr) if k else None
    n = B * T * F
    _call("curriculum_mask", L.sfm_curriculum_mask, (_p(cr), _p(ci), _p(nr), _p(ni), _p(scale), _p(table), _p(yr), _p(yi), _p(mask),
                                                     B, T, F, k, float(p), float(eps), int(M), _stream()),
          (8.0, 16.0, 32.0, 32.0)[k] * n, (28.0 if k else 24.0) * n, "B%d T%d F%d kind%d" % (B, T, F, k))
    return yr, yi, mask


# ---------------------------------------------------------------------------
# the PSO search of OPT-PCIRM's middle step (csrc/pso.hip)
# ---------------------------------------------------------------------------
PSO_CHUNK = _K["PSO_CHUNK"]                    # samples per workgroup of sfm_pso_split
PSO_FRAMES = _K["PSO_FRAMES"]                  # STOI frames per workgroup of sfm_pso_fitness
PSO_MAX_PARTICLES = _K["PSO_MAX_PARTICLES"]
PSO_MAX_BINS = _K["PSO_MAX_BINS"]


def pso_frame_coef(pcirm, table, M):
    """pcirm [B, C, T] fp32 contiguous, table of masks.opt_pcirm.quantizer_table -> (a, b) [B, T] fp64: the channel mean of mask
    frame n quantised with the middle value x is a[n] + x b[n]"""
    _need_dev(pcirm, table)
    L = _lib.load()
    if not (_is(pcirm, _F32, ndim=3, least=1) and
            2 <= M <= QUANT_MAX_STEPS and _is(table, _F64, 2 * M + 1)):
        _refuse("pso_frame_coef")
    B, C, T = pcirm.shape
    a = torch.empty(B, T, device=pcirm.device, dtype=torch.float64)
    b = torch.empty(B, T, device=pcirm.device, dtype=torch.float64)
    _call("pso_prepare", L.sfm_pso_frame_coef, (_p(pcirm), _p(table), _p(a), _p(b), B, C, T, int(M), _stream()), 0.0,
          4.0 * B * C * T + 16.0 * B * T, "coef B%d C%d T%d" % (B, C, T))
    return a, b


def pso_split(noisy, clean, lengths, samp_off, a, b, sum_L, frame, hop):
    """noisy, clean [B, Lmax] fp32; lengths int32 [B]; samp_off int32 [B + 1]; a, b [B, T] -> (ya, yb, clean) packed [sum_L] fp32
    and S [B, 4] fp64 = {sum ya^2, sum ya yb, sum yb^2, sum clean^2} (two launches: chunk sums, then the ordered fold)"""
    _need_dev(noisy, clean, lengths, samp_off, a, b)
    L = _lib.load()
    if not (_is(noisy, _F32, ndim=2) and noisy.shape[1] > 0 and
            _is(clean, _F32, noisy.numel()) and
            _is(lengths, _I32, noisy.shape[0]) and
            _is(samp_off, _I32, noisy.shape[0] + 1) and
            _is(a, _F64) and a.dim() >= 1 and a.numel() == noisy.shape[0] * a.shape[-1] and
            _is(b, _F64, a.numel()) and 0 < hop <= frame):
        _refuse("pso_split")
    (B, Lmax), T = noisy.shape, a.shape[-1]
    dev = noisy.device
    ya, yb, cp = (torch.empty(max(int(sum_L), 1), device=dev, dtype=torch.float32) for _ in range(3))
    S = torch.empty(B, 4, device=dev, dtype=torch.float64)
    ws = _ws64(L.sfm_pso_split_ws_doubles(B, Lmax), dev)
    _call("pso_prepare", L.sfm_pso_split, (_p(noisy), _p(clean), _p(lengths), _p(samp_off), _p(a), _p(b), _p(ya), _p(yb), _p(cp),
                                           _p(ws), _p(S), B, Lmax, T, int(frame), int(hop), _stream()),
          8.0 * sum_L, 20.0 * sum_L + 16.0 * B * T, "split B%d L%d" % (B, Lmax))
    return ya, yb, cp, S


def pso_fitness(spectra, frame_off, lengths, S, pos, stopped, partial, sum_frames):
    """spectra: (cr, ci, ar, ai, br, bi) packed rows [sum_frames, F] fp32; pos [B, N] fp64; partial [B, NC, N] fp64 receives one
    sum of clipped frame correlations per (utterance, chunk of PSO_FRAMES frames, particle).  Each spectrum is read once."""
    _need_dev(frame_off, lengths, S, pos, stopped, partial, *spectra)
    L = _lib.load()
    if not (len(spectra) == 6 and _is(spectra[0], _F32) and spectra[0].dim() >= 1 and
            all(_is(s, _F32, spectra[0].numel()) for s in spectra[1:]) and
            0 < spectra[0].shape[-1] <= PSO_MAX_BINS and spectra[0].numel() >= sum_frames * spectra[0].shape[-1] and
            _is(pos, _F64, ndim=2) and 1 <= pos.shape[1] <= PSO_MAX_PARTICLES and
            _is(frame_off, _I32, pos.shape[0] + 1) and
            _is(lengths, _I32, pos.shape[0]) and
            _is(S, _F64, 4 * pos.shape[0]) and
            _is(stopped, _I32, pos.shape[0]) and
            _is(partial, _F64) and partial.dim() >= 2 and partial.shape[1] >= 1 and
            partial.numel() == pos.numel() * partial.shape[1]):
        _refuse("pso_fitness")
    (B, N), F, NC = pos.shape, spectra[0].shape[-1], partial.shape[1]
    _call("pso_fitness", L.sfm_pso_fitness, tuple(_p(s) for s in spectra) + (_p(frame_off), _p(lengths), _p(S), _p(pos),
                                                                              _p(stopped), _p(partial), B, N, F, NC, _stream()),
          16.0 * sum_frames * F * N, 24.0 * sum_frames * F + 8.0 * B * NC * N, "B%d N%d F%d" % (B, N, F))
    return partial


def pso_step(state, it, partial=None, fitness=None, frame_off=None):
    """round `it` of every swarm of `state` (optimizer.pso.SwarmState) that has not stopped: the fitness from the partials of
    pso_fitness or handed in as [B, N] fp64, then optimizer/pso.py:92-110 (it = 0) or :114-179"""
    s = state
    _need_dev(partial, fitness, frame_off, s.draws, s.params, s.pos, s.vel, s.pbest_pos, s.pbest_fit, s.gbest, s.hist, s.iters,
              s.stopped)
    L = _lib.load()
    B, N, K = s.B, s.N, s.max_iter
    if not (1 <= N <= PSO_MAX_PARTICLES and K >= 1 and 0 <= it <= K and (partial is None) != (fitness is None) and
            _is(s.draws, _F64, B * (2 * N + 2 * N * K)) and
            _is(s.params, _F64, 5) and
            _each(_F64, B * N, s.pos, s.vel, s.pbest_pos, s.pbest_fit) and
            _is(s.gbest, _F64, 2 * B) and
            _is(s.hist, _F64, B * (K + 1) * (3 + 2 * N)) and
            _each(_I32, B, s.iters, s.stopped) and
            (partial is None or (_is(frame_off, _I32, B + 1) and _is(partial, _F64) and partial.dim() >= 2 and
                                 partial.numel() == B * partial.shape[1] * N)) and
            _is(fitness, _F64, B * N, opt=True)):
        _refuse("pso_step")
    NC = 0 if partial is None else partial.shape[1]
    _call("pso_step", L.sfm_pso_step, (_p(partial), _p(fitness), _p(frame_off), _p(s.draws), _p(s.params), _p(s.pos), _p(s.vel),
                                       _p(s.pbest_pos), _p(s.pbest_fit), _p(s.gbest), _p(s.hist), _p(s.iters), _p(s.stopped), B, N,
                                       NC, int(it), K, 1 if s.maximize else 0, _stream()),
          12.0 * B * N, 8.0 * B * N * (NC + 10), "B%d N%d" % (B, N))


def pso_quantize(pcirm, table, middle, M):
    """quantize_pcirm over [B, ...] fp32 with middle[b] (fp64 [B]) as the value of step 2 of utterance b (M >= 3)"""
    _need_dev(pcirm, table, middle)
    L = _lib.load()
    if not (_planes_ok(pcirm) and pcirm.dim() >= 1 and
            2 <= M <= QUANT_MAX_STEPS and _is(table, _F64, 2 * M + 1) and
            _is(middle, _F64, pcirm.shape[0])):
        _refuse("pso_quantize")
    B, n = pcirm.shape[0], pcirm.numel()
    out = torch.empty_like(pcirm)
    _call("mask_quantize", L.sfm_pso_quantize, (_p(pcirm), _p(table), _p(middle), _p(out), B, n // B, int(M), _stream()), 0.0,
          8.0 * n)
    return out


# ---------------------------------------------------------------------------
# gammatone T-F analysis (csrc/gammatone.hip; signal_processing/gammatone.py)
# ---------------------------------------------------------------------------
GT_COLS = _K["GT_COLS"]                        # channel columns of the tap and twiddle operands (C <= 64, zero beyond C)
GT_ROWS = _K["GT_ROWS"]                        # samples per workgroup of sfm_gammatone_fir / sfm_gammatone_tf
GT_MAX_TAPS = _K["GT_MAX_TAPS"]
GT_LDS_MAX = _K["GT_LDS_MAX"]


def set_gammatone_fused(flag):
    """get_tf_magnitudes on hop-blocks inside the FIR kernel (sfm_gammatone_tf) where the framing allows it; False = the FIR
    bank's [B, C, L] result in HBM, then the moments pass over it (A/B testing)"""
    _SWITCHES["gammatone_fused"][2] = bool(flag)


def gammatone_tf_fits(K, hop):
    """sfm_gammatone_tf takes K taps (a multiple of 8) and this hop: one hop-block fits the workgroup's rows and its LDS image fits
    (the library's own predicate; no device work)"""
    return bool(_lib.load().sfm_gammatone_tf_fits(int(K), int(hop)))


def gammatone_fir(sig, taps, C, lengths=None):
    """sig [B, L], taps [K, 64] -> [B, C, L] = the causal FIR bank (0 from lengths[b] on)"""
    _need_dev(sig, taps, lengths)
    L_ = _lib.load()
    if not (_is(sig, _F32, ndim=2, least=1) and sig.shape[0] <= 65535 and
            _is(taps, _F32, (None, GT_COLS)) and 8 <= taps.shape[0] <= GT_MAX_TAPS and taps.shape[0] % 8 == 0 and
            1 <= C <= GT_COLS and _lengths_ok(lengths, sig.shape[0])):
        _refuse("gammatone_fir")
    (B, L), K = sig.shape, taps.shape[0]
    out = torch.empty(B, C, L, device=sig.device, dtype=torch.float32)
    _call("gammatone_fir", L_.sfm_gammatone_fir, (_p(sig), _p(taps), _p(lengths), _p(out), B, L, C, K, _stream()),
          2.0 * B * L * C * K, 4.0 * B * L + 4.0 * K * GT_COLS + 4.0 * B * C * L, "B%d L%d C%d K%d" % (B, L, C, K))
    return out


def gammatone_tf(sig, taps, tw, C, hop, lengths=None):
    """sig [B, L], taps [K, 64], tw [2, hop, 64] -> partial [B, L // hop, C, 5]: the five sums of every whole hop-block of the
    filtered signal, which is never stored"""
    _need_dev(sig, taps, tw, lengths)
    L_ = _lib.load()
    # (K and hop themselves - sfm_gammatone_tf_fits - are the launcher's to refuse: it sees them)
    if not (_is(sig, _F32, ndim=2, least=1) and sig.shape[0] <= 65535 and
            _is(taps, _F32, (None, GT_COLS)) and 8 <= taps.shape[0] <= GT_MAX_TAPS and taps.shape[0] % 8 == 0 and
            _is(tw, _F32, (2, hop, GT_COLS)) and
            1 <= C <= GT_COLS and 0 < hop <= sig.shape[1] and _lengths_ok(lengths, sig.shape[0])):
        _refuse("gammatone_tf")
    (B, L), K = sig.shape, taps.shape[0]
    nblocks = L // hop
    partial = torch.empty(B, nblocks, C, 5, device=sig.device, dtype=torch.float32)
    n = float(B) * nblocks * hop
    _call("gammatone_tf", L_.sfm_gammatone_tf, (_p(sig), _p(taps), _p(tw), _p(lengths), _p(partial), B, L, C, K, hop, nblocks,
                                                _stream()),
          n * C * (2.0 * K + 10.0), 4.0 * B * L + 4.0 * K * GT_COLS + 8.0 * hop * GT_COLS + 20.0 * B * nblocks * C,
          "B%d L%d C%d K%d hop%d" % (B, L, C, K, hop))
    return partial


def gammatone_moments(y, tw, T, w, frame, hop, lengths=None):
    """y [B, C, L] (gammatone_fir's), tw [2, w, 64] -> partial [B, T, C, 5]: the five sums of the first w samples of each frame"""
    _need_dev(y, tw, lengths)
    L_ = _lib.load()
    if not (_is(y, _F32, ndim=3, least=1) and y.shape[0] <= 65535 and y.shape[1] <= GT_COLS and
            _is(tw, _F32, (2, w, GT_COLS)) and
            T >= 1 and 1 <= w <= frame and hop >= 1 and (T - 1) * hop + frame <= y.shape[2] and
            _lengths_ok(lengths, y.shape[0])):
        _refuse("gammatone_moments")
    B, C, L = y.shape
    partial = torch.empty(B, T, C, 5, device=y.device, dtype=torch.float32)
    _call("gammatone_moments", L_.sfm_gammatone_moments, (_p(y), _p(tw), _p(lengths), _p(partial), B, L, C, T, w, frame, hop,
                                                          _stream()),
          10.0 * B * C * T * w, 4.0 * B * C * L + 8.0 * w * GT_COLS + 20.0 * B * T * C,
          "B%d L%d C%d T%d w%d hop%d" % (B, L, C, T, w, hop))
    return partial


def gammatone_tf_finish(partial, rot, T, L, frame, hop, N, two, lengths=None, want_bins=False):
    """partial [B, P, C, 5] -> (mag, phase[, re, im]) [B, C, T]; two: frame n = rows n, n + 1 (rot [2, 64] turns the second)"""
    _need_dev(partial, rot, lengths)
    L_ = _lib.load()
    if not (_is(partial, _F32, (None, None, None, 5)) and partial.shape[0] <= 65535 and partial.shape[2] <= GT_COLS and
            T >= 1 and partial.shape[1] >= T + (1 if two else 0) and
            (not two or _is(rot, _F32, (2, GT_COLS))) and
            N >= 2 and N % 2 == 0 and frame >= 1 and hop >= 1 and L >= frame and T <= (L - frame) // hop + 1 and
            _lengths_ok(lengths, partial.shape[0])):
        _refuse("gammatone_tf_finish")
    B, P, C, _ = partial.shape
    outs = [torch.empty(B, C, T, device=partial.device, dtype=torch.float32) for _ in range(4 if want_bins else 2)]
    re, im = (outs[2], outs[3]) if want_bins else (None, None)
    n = float(B) * C * T
    _call("gammatone_tf_finish", L_.sfm_gammatone_tf_finish, (_p(partial), _p(rot), _p(lengths), _p(outs[0]), _p(outs[1]), _p(re),
                                                              _p(im), B, C, T, P, int(bool(two)), L, frame, hop, N, _stream()),
          20.0 * n, 20.0 * B * C * (T + (1 if two else 0)) + 4.0 * n * len(outs), "B%d C%d T%d two%d" % (B, C, T, int(bool(two))))
    return tuple(outs)


# ---------------------------------------------------------------------------
# the DNN front end (csrc/features.hip; signal_processing/features.py)
# ---------------------------------------------------------------------------
FE_MAX_FILTERS, FE_MAX_BINS, FE_MAX_COEFFS = _K["FE_MAX_FILTERS"], _K["FE_MAX_BINS"], _K["FE_MAX_COEFFS"]
CEP_POWER, CEP_MAGNITUDE, CEP_BLOCKS = _K["CEP_POWER"], _K["CEP_MAGNITUDE"], _K["CEP_BLOCKS"]      # sfm_cepstral's in_mode
CEP_NONE, CEP_LOG, CEP_CBRT = _K["CEP_NONE"], _K["CEP_LOG"], _K["CEP_CBRT"]                        # its compress


def cepstral(src, fb, dct, out, col_off, *, B, T, L, frame, hop, in_mode, F, compress, im_off=0, bmul=1, badd=0, window=1.0,
             lengths=None):
    """rows of src -> out[.., col_off : col_off + (NC or M)]: [power / magnitude / block energy -> fb [M, F] (None: M = F) -> compress
    -> dct [NC, M] (None: NC = 0)].  src [B, T, ld_in] spectrum rows with re at [0, F) and im at [im_off, im_off + F)
    (CEP_POWER, CEP_MAGNITUDE) or gammatone_tf's partial [B, P, F, 5] (CEP_BLOCKS: blocks bmul n + badd and the next, over `window`
    samples).  out [B, T, ld_out] fp32; rows from T_b on are not written."""
    _need_dev(src, fb, dct, out, lengths)
    L_ = _lib.load()
    blocks = in_mode == CEP_BLOCKS                          # otherwise the rows may be a column slice of a wider row matrix
    if not (_is(src, _F32, (B, None, F, 5) if blocks else (B, T, None), contig=True if blocks else "last") and
            _is(fb, _F32, (None, F), opt=True) and
            _is(dct, _F32, (None, F if fb is None else fb.shape[0]), opt=True) and
            _is(out, _F32, (B, T, None)) and
            B >= 1 and T >= 1 and B * T < 2 ** 31 and 1 <= F <= FE_MAX_BINS and
            frame >= 1 and hop >= 1 and L >= frame and T <= (L - frame) // hop + 1 and
            _lengths_ok(lengths, B)):
        _refuse("cepstral")
    M = F if fb is None else fb.shape[0]
    NC = 0 if dct is None else dct.shape[0]
    ok = 1 <= M <= FE_MAX_FILTERS and NC <= FE_MAX_COEFFS and 0 <= col_off and col_off + (NC or M) <= out.shape[2]
    if blocks:
        ok = ok and F <= 64 and bmul >= 1 and badd >= 0 and window > 0 and bmul * (T - 1) + badd + 1 < src.shape[1]
        ld_in, P = 0, src.shape[1]
    else:
        ok = ok and in_mode in (CEP_POWER, CEP_MAGNITUDE) and src.stride(0) == T * src.stride(1) and src.stride(1) >= src.shape[2]
        ok = ok and F <= im_off and im_off + F <= src.shape[2]
        ld_in, P = src.stride(1), 0
    if not ok:
        _refuse("cepstral")
    rows = float(B) * T
    _call("cepstral", L_.sfm_cepstral, (_p(src), _p(fb), _p(dct), _p(lengths), _p(out), B, T, L, frame, hop, in_mode, ld_in, im_off, F,
                                        M, NC, compress, P, bmul, badd, float(window), out.shape[2], col_off, _stream()),
          rows * (3.0 * F + (2.0 * M * F if fb is not None else 0.0) + M + 2.0 * NC * M),
          rows * (8.0 * F + 4.0 * (NC or M)) + (4.0 * M * F if fb is not None else 0.0) + 4.0 * NC * M,
          "B%d T%d F%d M%d NC%d in%d c%d" % (B, T, F, M, NC, in_mode, compress))
    return out


def rasta(logb, eql, dct, out, col_off, *, L, frame, hop, lengths=None):
    """logb [B, T, M] fp32 (log bark energies), eql [M] and dct [NC, M] fp64 -> out[b, n < T_b, col_off : col_off + NC] = the
    utterance's RASTA-PLP vector on every live row.  The recurrence, the mean and the DCT run in fp64 in frame order."""
    _need_dev(logb, eql, dct, out, lengths)
    L_ = _lib.load()
    if not (_is(logb, _F32, ndim=3) and 1 <= logb.shape[2] <= FE_MAX_FILTERS and
            _is(eql, _F64, (logb.shape[2],)) and
            _is(dct, _F64, (None, logb.shape[2])) and 1 <= dct.shape[0] <= FE_MAX_COEFFS and
            _is(out, _F32, (logb.shape[0], logb.shape[1], None)) and 0 <= col_off and col_off + dct.shape[0] <= out.shape[2] and
            frame >= 1 and hop >= 1 and L >= frame and 1 <= logb.shape[1] <= (L - frame) // hop + 1 and
            _lengths_ok(lengths, logb.shape[0])):
        _refuse("rasta")
    (B, T, M), NC = logb.shape, dct.shape[0]
    _call("rasta", L_.sfm_rasta, (_p(logb), _p(eql), _p(dct), _p(lengths), _p(out), B, T, L, frame, hop, M, NC, out.shape[2], col_off,
                                  _stream()),
          12.0 * B * T * M + 2.0 * B * NC * M, 4.0 * B * T * M + 4.0 * B * T * NC + 8.0 * M + 8.0 * NC * M, "B%d T%d M%d NC%d" % (B, T, M, NC))
    return out


def feature_context(feat, ctx, *, L, frame, hop, mean=None, std=None, clip=10.0, lengths=None):
    """feat [B, T, D] -> [B, T, (2 ctx + 1) D]: rows clamp(n - ctx .. n + ctx, 0, T_b - 1) side by side, 0 from T_b on; with mean and
    std [(2 ctx + 1) D] the same launch applies nan / inf -> 0, (f - mean) / std and the clip to +-clip"""
    _need_dev(feat, mean, std, lengths)
    L_ = _lib.load()
    if not (_is(feat, _F32, ndim=3, least=1) and feat.shape[2] % 2 == 0 and feat.shape[0] * feat.shape[1] < 2 ** 31 and
            0 <= ctx <= 64 and clip > 0 and (mean is None) == (std is None) and
            _is(mean, _F32, ((2 * ctx + 1) * feat.shape[2],), opt=True) and
            _is(std, _F32, ((2 * ctx + 1) * feat.shape[2],), opt=True) and
            frame >= 1 and hop >= 1 and L >= frame and feat.shape[1] <= (L - frame) // hop + 1 and
            _lengths_ok(lengths, feat.shape[0])):
        _refuse("feature_context")
    B, T, D = feat.shape
    W = (2 * ctx + 1) * D
    out = torch.empty(B, T, W, device=feat.device, dtype=torch.float32)
    n = float(B) * T
    _call("feature_context", L_.sfm_feature_context, (_p(feat), _p(mean), _p(std), _p(lengths), _p(out), B, T, L, frame, hop, D, ctx,
                                                      float(clip), _stream()),
          0.0 if mean is None else 3.0 * n * W, 4.0 * n * (D + W) + (0.0 if mean is None else 8.0 * W),
          "B%d T%d D%d ctx%d norm%d" % (B, T, D, ctx, int(mean is not None)))
    return out


def rows_mean(src, col_off, N, *, L, frame, hop, den=0, lengths=None):
    """src [B, T, ld] -> [B, N]: the mean over an utterance's T_b rows of columns col_off .. col_off + N (den > 0: the sum over den)"""
    _need_dev(src, lengths)
    L_ = _lib.load()
    if not (_is(src, _F32, ndim=3, least=1) and
            N >= 1 and 0 <= col_off and col_off + N <= src.shape[2] and den >= 0 and
            frame >= 1 and hop >= 1 and L >= frame and src.shape[1] <= (L - frame) // hop + 1 and
            _lengths_ok(lengths, src.shape[0])):
        _refuse("rows_mean")
    B, T, ld = src.shape
    out = torch.empty(B, N, device=src.device, dtype=torch.float32)
    _call("rows_mean", L_.sfm_rows_mean, (_p(src), _p(lengths), _p(out), B, T, L, frame, hop, ld, col_off, N, int(den), _stream()),
          1.0 * B * T * N, 4.0 * B * T * N + 4.0 * B * N, "B%d T%d N%d" % (B, T, N))
    return out


# ---------------------------------------------------------------------------
# Meddis hair cell (csrc/haircell.hip; signal_processing/haircell.py)
# ---------------------------------------------------------------------------
HC_PARAMS = _K["HC_PARAMS"]         # par = {A, B, y, l, r, x, h, M, dt, q0, c0, w0}, fp64
HC_STEP_FLOPS = 24.0                # fp64 operations of one Euler step: 3 for k, 6 + 6 + 5 for q, c, w with their clamps, 1 for h c,
                                    # 3 for the two frame sums (counted in both forms: the algorithm, not the variant)


def haircell(x, par):
    """x [N, L] fp32, par [12] fp64 -> [N, L] fp64: the firing rate h c[t] of each row's chain"""
    _need_dev(x, par)
    L_ = _lib.load()
    if not (_is(x, _F32, ndim=2, least=1) and x.shape[0] < 2 ** 31 and
            _is(par, _F64, (HC_PARAMS,))):
        _refuse("haircell")
    N, L = x.shape
    out = torch.empty(N, L, device=x.device, dtype=torch.float64)
    _call("haircell", L_.sfm_haircell, (_p(x), _p(par), _p(out), N, L, _stream()),
          HC_STEP_FLOPS * N * L, 12.0 * N * L + 8.0 * HC_PARAMS, "N%d L%d" % (N, L))
    return out


def haircell_frames(x, par, frame, hop, lengths=None):
    """x [B, C, L] fp32 -> [B, C, T] fp64: the mean firing rate of each frame of `frame` samples at `hop` (frame <= 2 hop); with
    lengths (int32 [B]) a chain stops at its utterance's end and frames from T_b on are 0.  The rate signal is not stored."""
    _need_dev(x, par, lengths)
    L_ = _lib.load()
    if not (_is(x, _F32, ndim=3, least=1) and x.shape[0] * x.shape[1] < 2 ** 31 and
            _is(par, _F64, (HC_PARAMS,)) and
            1 <= hop and 1 <= frame <= 2 * hop and x.shape[2] >= frame and
            _lengths_ok(lengths, x.shape[0])):
        _refuse("haircell_frames")
    B, C, L = x.shape
    T = (L - frame) // hop + 1
    out = torch.empty(B, C, T, device=x.device, dtype=torch.float64)
    _call("haircell_frames", L_.sfm_haircell_frames, (_p(x), _p(par), _p(lengths), _p(out), B * C, C, L, frame, hop, T, _stream()),
          HC_STEP_FLOPS * B * C * L, 4.0 * B * C * L + 8.0 * B * C * T + 8.0 * HC_PARAMS, "B%d C%d L%d f%d h%d" % (B, C, L, frame, hop))
    return out


def spec_sums(pr, pi, tr, ti, out=None):
    L = _lib.load()
    S = torch.zeros(4, device=pr.device, dtype=torch.float64) if out is None else out
    _call("loss_reduce", L.sfm_spec_sums, (_p(pr), _p(pi), _p(tr), _p(ti), _p(S), pr.numel(),
                                           _p(_ws(L.sfm_spec_sums_ws_doubles(pr.numel()), pr.device, torch.float64)), _stream()),
          0.0, 16.0 * pr.numel())
    return S


def enhancer_loss_finalize(Sw, Sm, Sr, nr, B, Ln, n_mag, R=None):
    """-> [total, neg SI-SNR, L1 magnitude, MR-STFT]; R: resolutions in Sr / nr (default: all rows; 0 = none)"""
    L = _lib.load()
    out = torch.empty(4, device=Sw.device, dtype=torch.float32)
    _call("loss_reduce", L.sfm_enhancer_loss_finalize, (_p(Sw), _p(Sm), _p(Sr), _p(nr), B, Ln, n_mag,
                                                        Sr.shape[0] if R is None else int(R), _p(out), _stream()))
    return out


def sisnr_bwd(est, tgt, Sw, dwave, scale=1.0):
    L = _lib.load()
    B, Ln = est.shape
    _call("loss_bwd", L.sfm_sisnr_bwd, (_p(est), _p(tgt), _p(Sw), _p(dwave), B, Ln, float(scale), _stream()), 0.0, 12.0 * B * Ln)


def spec_loss_bwd(pr, pi, tr, ti, S, dr, di, F, ld, mode, accumulate=False, scale=1.0):
    L = _lib.load()
    _call("loss_bwd", L.sfm_spec_loss_bwd, (_p(pr), _p(pi), _p(tr), _p(ti), _p(S), _p(dr), _p(di), pr.numel(), F, ld, mode,
                                            1 if accumulate else 0, float(scale), _stream()), 0.0, 24.0 * pr.numel())


def stft_adjoint_ola(frames, dwave, B, T, Ln, n_fft, hop, win, accumulate=True, post=None):
    L = _lib.load()
    _call("loss_bwd", L.sfm_stft_adjoint_ola, (_p(frames), _p(dwave), _p(post), B, T, Ln, n_fft, hop, win,
                                               1 if accumulate else 0, _stream()), 0.0, 4.0 * (B * T * win + 2 * B * Ln))


def polar_mask_bwd(lm, lp, nr, ni, der, dei, dlog, M, F, phase_scale, ld_logits, mag_bias=None, rows_per_batch=None):
    L = _lib.load()
    _call("loss_bwd", L.sfm_polar_mask_bwd, (_p(lm), _p(lp), _p(mag_bias), _p(nr), _p(ni), _p(der), _p(dei), _p(dlog), M,
                                             rows_per_batch or M, F, float(phase_scale), ld_logits, dlog.stride(0), _stream()),
          0.0, 32.0 * M * F)


def sum_time(src32, B, T, C, ld_src):
    L = _lib.load()
    out = torch.empty(B, C, device=src32.device, dtype=torch.float32)
    scratch = torch.empty(int(L.sfm_mean_time_scratch_floats(B, T, C)), device=src32.device, dtype=torch.float32)
    _call("pool_time", L.sfm_sum_time, (_p(src32), _p(out), _p(scratch), B, T, C, ld_src, _stream()), 0.0, 4.0 * B * T * C)
    return out


def _tn_ws(L_, M, N, K, device):
    """(workspace, its size in floats) of the ordered M-split fold of the TN GEMMs, or (None, 0) in the atomics form"""
    if not switch("deterministic"):
        return None, 0
    n = int(L_.sfm_tn_ws_floats(M, N, K))
    return _ws(n, device), n


def sinc_wgrad(wave, dy, C, K, exact=False):
    """dfilt [C, K] = sum_{b,l} dy[b, l, c] * wave[b, l + k - K//2]   (dy [B, L, C] 16-bit or fp32).
    A 16-bit dy with the reference's 251 taps runs on the matrix cores (waveform rounded to the compute dtype, like the
    activations of every other weight gradient on the path); exact=True or an fp32 dy keeps the fp32 vector kernel."""
    L_ = _lib.load()
    B, L = wave.shape
    if not exact and K == 251 and dy.dtype == _state["dtype"] and C % 8 == 0:
        Lc = int(L_.sfm_sinc_shift_len(L))
        xs = torch.empty(B, 8, Lc, device=wave.device, dtype=dy.dtype)
        _call("sinc_shift_pack", L_.sfm_sinc_shift_pack, (_p(wave), _p(xs), B, L, _dt(), _stream()), 0.0, B * (4.0 * L + 16.0 * Lc))
        dW = torch.zeros(C, 256, device=wave.device, dtype=torch.float32)
        ws, wsn = _tn_ws(L_, B * L, C, 256, wave.device)
        _call("sinc_wgrad16", L_.sfm_sinc_wgrad16, (_p(dy), _p(xs), _p(dW), B, L, C, _dt(), _p(ws), wsn, _stream()),
              2.0 * B * L * C * 256, B * L * (2.0 * C + 16.0))
        return dW[:, :K].contiguous()
    dfilt = torch.zeros(C, K, device=wave.device, dtype=torch.float32)
    scratch = torch.empty(int(L_.sfm_sinc_wgrad_scratch_floats(B, L, C, K)), device=wave.device, dtype=torch.float32)
    _call("sinc_wgrad", L_.sfm_sinc_wgrad, (_p(wave), _p(dy), 1 if dy.dtype == torch.float32 else 0, _p(dfilt), _p(scratch), B, L, C,
                                            K, _dt(), _stream()), 2.0 * B * L * C * K, B * L * (4.0 + C * dy.element_size()))
    return dfilt


def gn_stats(partial, rows, C, G):
    """group mean / rstd [B, G] from the per-64-row partial sums a producing GEMM wrote ([B, P, G, 2] = sum, sum of squares)"""
    s = partial.double().sum(dim=1)
    n = float(rows * (C // G))
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp_min(0.0)
    return mean.float(), torch.rsqrt(var + 1e-5).float()


def gn_act_backward(dout, act, G, x1, sc1, sh1, mean1, rstd1, gamma1, x2=None, sc2=None, sh2=None, mean2=None, rstd2=None,
                    gamma2=None, dx_dtype=None):
    """backward of out = act(GN(x1) [+ GN(x2)]) on channels-last [B, L, C] tensors (PerceptionAgent nodes).
    sc / sh [B, C]: the forward's scale and shift; mean / rstd [B, G]; gamma [C].
    Returns dx1, dgamma1, dbeta1 (and dx2, dgamma2, dbeta2 when two inputs)."""
    L_ = _lib.load()
    B, L, C = x1.shape
    dx_dtype = dx_dtype or _state["dtype"]
    two = x2 is not None
    dev = x1.device
    f32 = lambda t: 1 if t.dtype == torch.float32 else 0
    c32 = lambda t: None if t is None else t.float().contiguous()
    dout = dout.contiguous()
    sc1, sh1, mean1, rstd1, gamma1 = c32(sc1), c32(sh1), c32(mean1), c32(rstd1), c32(gamma1)
    sc2, sh2, mean2, rstd2, gamma2 = c32(sc2), c32(sh2), c32(mean2), c32(rstd2), c32(gamma2)
    work = torch.zeros(3 * B * C + 3 * C, device=dev, dtype=torch.float32)       # S [B][3][C] | dparam [3][C]
    S, dparam = work[:3 * B * C], work[3 * B * C:].view(3, C)
    nbytes = float(B * L * C) * ((4 if f32(dout) else 2) + (1 + two) * (4 if f32(x1) else 2))
    ws = _ws(int(L_.sfm_gn_bwd_reduce_ws_floats(B, L, C)), dev) if switch("deterministic") else None
    _call("gn_bwd_reduce", L_.sfm_gn_bwd_reduce, (_p(dout), f32(dout), _p(x1), f32(x1), _p(sc1), _p(sh1), _p(mean1), _p(rstd1), _p(x2),
                                           f32(x2) if two else 0, _p(sc2), _p(sh2), _p(mean2), _p(rstd2), _p(S), B, L, C, G,
                                           int(act), _dt(), _p(ws), _stream()), 0.0, nbytes)
    coef = torch.empty(2, 3, B, C, device=dev, dtype=torch.float32)
    _call("gn_bwd_coefs", L_.sfm_gn_bwd_coefs, (_p(S), _p(gamma1), _p(rstd1), _p(gamma2), _p(rstd2), _p(coef[0]),
                                                _p(coef[1]) if two else None, _p(dparam), B, L, C, G, _stream()), 0.0,
          4.0 * 9 * B * C)
    dx1 = torch.empty(B, L, C, device=dev, dtype=dx_dtype)
    dx2 = torch.empty(B, L, C, device=dev, dtype=dx_dtype) if two else None
    _call("gn_bwd_apply", L_.sfm_gn_bwd_apply, (_p(dout), f32(dout), _p(x1), f32(x1), _p(sc1), _p(sh1), _p(mean1), _p(rstd1), _p(coef[0]),
                                          _p(dx1), f32(dx1), _p(x2), f32(x2) if two else 0, _p(sc2), _p(sh2), _p(mean2), _p(rstd2),
                                          _p(coef[1]) if two else None, _p(dx2), f32(dx2) if two else 0, B, L, C, G, int(act),
                                          _dt(), _stream()), 0.0, nbytes + float(B * L * C) * (1 + two) * (4 if f32(dx1) else 2))
    if two:
        return dx1, dparam[1], dparam[0], dx2, dparam[2], dparam[0]
    return dx1, dparam[1], dparam[0]


# ---------------------------------------------------------------------------
# training path (ConformerBlock backward)
# ---------------------------------------------------------------------------
_WGRAD = {"stream": None, "keep": []}


class wgrad_side_stream:
    """inside this context the weight-gradient GEMMs are enqueued on a second HIP stream: they are off the critical path of
    the backward pass (nothing but the optimiser reads dW), so they fill the CUs the input-gradient chain leaves idle; on
    exit the current stream waits for them."""

    def __init__(self, enabled=True):
        self.enabled = enabled and switch("wgrad_stream")

    def __enter__(self):
        if self.enabled:
            if "side" not in _WGRAD:
                _WGRAD["side"] = torch.cuda.Stream()
            _WGRAD["stream"] = _WGRAD["side"]
        return self

    def __exit__(self, *exc):
        if self.enabled:
            torch.cuda.current_stream().wait_stream(_WGRAD["side"])
            _WGRAD["stream"] = None
            # operands of the side-stream GEMMs were kept alive until the join is enqueued: whoever reuses their memory on the
            # main stream now runs after it.  (tensor.record_stream() instead defers the reuse to an event query; with the host
            # several steps ahead of the GPU the allocator then grows by hipMalloc: sporadic 1 s stalls in bench.py)
            _WGRAD["keep"].clear()
        return False


class after_wgrad:
    """host ops that post-process a weight gradient (e.g. rescaling rows) must run where the GEMM that produces it runs:
    on the side stream when wgrad_side_stream is active (the listed temporaries are kept alive for it), else in place."""

    def __init__(self, *temporaries):
        self.ws = _WGRAD["stream"]
        self.tmp = temporaries
        self.ctx = None

    def __enter__(self):
        if self.ws is not None:
            self.ctx = torch.cuda.stream(self.ws)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ws is not None:
            self.ctx.__exit__(*exc)
            _WGRAD["keep"].extend(self.tmp)
        return False


def gemm16_tn(G16, X16, dW, db=None):
    """dW[n,k] += sum_m G16[m,n] * X16[m,k]   (dW fp32, accumulated); db[n] += sum_m G16[m,n] when given."""
    ws = _WGRAD["stream"]
    if ws is not None and torch.cuda.current_stream() != ws:
        ws.wait_stream(torch.cuda.current_stream())          # operands (and the zero-filled dW) are ready
        with torch.cuda.stream(ws):
            gemm16_tn(G16, X16, dW, db)
        _WGRAD["keep"].extend((G16, X16))                      # alive until the join (see wgrad_side_stream.__exit__)
        return
    L = _lib.load()
    M, N = G16.shape
    K = X16.shape[1]
    ws, wsn = _tn_ws(L, M, N, K, G16.device)
    _call("gemm16_tn", L.sfm_gemm16_tn, (_p(G16), _p(X16), _p(dW), _p(db), M, N, K, G16.stride(0), X16.stride(0), dW.stride(0),
                                         _dt(), _p(ws), wsn, _stream()), 2.0 * M * N * K, M * (N + K) * 2.0,
          tag="M%d N%d K%d" % (M, N, K))


def conv_wgrad16(dy16, x16, B, Lout, Lin, Cin, N, ksize, stride, pad, tap_major=False):
    """Conv1d weight / bias gradient from dY [B*Lout, N] and the channels-last input x [B, Lin, Cin] (both 16-bit):
    returns dW in torch's Conv1d layout [N, Cin, ksize] and db [N] (fp32).  tap_major: dW as the GEMM leaves it,
    [N, ksize, Cin] (no permuting copy; adv_sn_bwd reads that layout)."""
    ws = _WGRAD["stream"]
    if ws is not None and torch.cuda.current_stream() != ws:   # off the critical path: see wgrad_side_stream
        ws.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ws):
            out = conv_wgrad16(dy16, x16, B, Lout, Lin, Cin, N, ksize, stride, pad, tap_major)
        _WGRAD["keep"].extend((dy16, x16))
        return out
    L = _lib.load()
    buf = torch.zeros(N * ksize * Cin + N, device=x16.device, dtype=torch.float32)       # dW | db: one fill
    dW, db = buf[:N * ksize * Cin].view(N, ksize * Cin), buf[N * ksize * Cin:]
    ws, wsn = _tn_ws(L, B * Lout, N, ksize * Cin, x16.device)
    _call("gemm16_tn", L.sfm_conv_wgrad16, (_p(dy16), _p(x16), _p(dW), _p(db), B, Lout, Lin, Cin, N, ksize, stride, pad,
                                            Lin * Cin, dy16.stride(0), dW.stride(0), _dt(), _p(ws), wsn, _stream()),
          2.0 * B * Lout * N * ksize * Cin, (B * Lout * N + B * Lin * Cin) * 2.0,
          tag="conv M%d N%d K%d s%d" % (B * Lout, N, ksize * Cin, stride))
    if tap_major:
        return dW.reshape(N, ksize, Cin), db
    return dW.reshape(N, ksize, Cin).permute(0, 2, 1).contiguous(), db


def conv_dgrad16(dy16, weight, B, Lout, Lin, stride, pad, accumulate_into=None, out_dtype=torch.float32, add_even=None):
    """input gradient of Conv1d(weight [N, Cin, k], stride 1 or 2, zero padding) on channels-last tensors:
    dy16 [B, Lout, N] 16-bit -> dx [B, Lin, Cin] in `out_dtype` (fp32 or the 16-bit compute type).  Stride 1 is the
    correlation with the flipped, transposed kernel; stride 2 is that per output parity (two implicit GEMMs writing the
    even / odd rows).  Every row is written exactly once, so there is no zero-fill and no read-modify-write:
      add_even [B, ceil(Lin / stride), Cin] fp32: added to the rows of parity 0 in the GEMM's epilogue - the input gradient of a
                 parallel k = 1 convolution with the same stride (the residual blocks' skip path, agents/perception.py:121-129);
      accumulate_into (fp32 [B, Lin, Cin]): the older read-modify-write form, kept for a parity that has no tap."""
    N, Cin, k = weight.shape
    w = weight.detach().float()
    plan = []
    for r in range(stride):
        t0 = (r + pad) % stride
        taps = list(range(t0, k, stride))
        nq = (Lin - r + stride - 1) // stride
        plan.append((r, t0, taps, nq))
    covered = all(taps and nq > 0 for _, _, taps, nq in plan)
    if accumulate_into is not None:
        dx = accumulate_into
    elif covered:
        dx = torch.empty(B, Lin, Cin, device=dy16.device, dtype=out_dtype)
    else:
        dx = torch.zeros(B, Lin, Cin, device=dy16.device, dtype=out_dtype)
    for r, t0, taps, nq in plan:
        if not taps or nq <= 0:
            continue
        J = len(taps)
        c0 = (r + pad - t0) // stride
        # out[q] = sum_j' in[q - pad2 + j'] Wf[j'],  Wf[j'] = W[:, :, taps[J-1-j']]^T,  pad2 = J - 1 - c0
        wf = torch.stack([w[:, :, taps[J - 1 - j]] for j in range(J)], dim=2).permute(1, 0, 2).contiguous()   # [Cin, N, J]
        pw = pack_linear(wf)
        view = dx.reshape(B, Lin * Cin)[:, r * Cin:]
        kw = dict(B=B, Lout=nq, Lin=Lout, a_batch_stride=Lout * N, ldo=stride * Cin, o_batch_stride=Lin * Cin, stride=1,
                  pad=J - 1 - c0)
        if accumulate_into is not None:
            gemm16(dy16, pw, view, epi=EPI_RESID, resid=view, ldr=stride * Cin, r_batch_stride=Lin * Cin, alpha=1.0, **kw)
        elif add_even is not None and r == 0:
            assert add_even.dtype == torch.float32 and add_even.shape[1] == nq
            gemm16(dy16, pw, view, epi=EPI_RESID, resid=add_even, ldr=Cin, r_batch_stride=nq * Cin, alpha=1.0, **kw)
        else:
            gemm16(dy16, pw, view, **kw)
    return dx


def colsum(G, out):
    L = _lib.load()
    M, N = G.shape
    ws = _ws(int(L.sfm_colsum_ws_floats(M, N)), G.device) if switch("deterministic") else None
    _call("colsum", L.sfm_colsum, (_p(G), _p(out), M, N, G.stride(0), 1 if G.dtype == torch.float32 else 0, _dt(), _p(ws), _stream()))


def layernorm_bwd(x32, gamma, dy, dres32, dgamma, dbeta, eps=1e-5, next_drop=None):
    """dy: fp32, or the 16-bit result of the GEMM that produced it (its own row stride); dres / dx fp32 [M, D].
    next_drop = (alpha, p, seed): also returns alpha * dropout(dx; p, seed) [M, D] in the 16-bit compute format, the operand the
    next backward node of the residual chain starts from (same counters as ew_train(EW_SCALE_DROP)) -> (dx, next16)."""
    L = _lib.load()
    M, D = dy.shape
    if D > LAYERNORM_MAX_D:
        raise RuntimeError("layernorm_bwd: width %d is not supported (the LayerNorm kernels take D <= %d)" % (D, LAYERNORM_MAX_D))
    dx = torch.empty(M, D, device=dy.device, dtype=torch.float32)
    ws = _ws(int(L.sfm_layernorm_bwd_ws_floats(M, D)), dy.device) if switch("deterministic") else None
    dy16 = 0 if dy.dtype == torch.float32 else 1
    if dy16 and dy.dtype != _state["dtype"]:
        raise RuntimeError("layernorm_bwd: a 16-bit dy must be in the compute format")
    if next_drop is not None:
        alpha, p, seed = next_drop
        nxt = torch.empty(M, D, device=dy.device, dtype=_state["dtype"])
        _call("layernorm_bwd", L.sfm_layernorm_bwd_next, (_p(x32), _p(gamma), _p(dy), dy16, _p(dres32), _p(dx), _p(dgamma), _p(dbeta), M, D,
                                                          x32.stride(0), dy.stride(0), D, eps, _dt(), _p(nxt), float(alpha), float(p),
                                                          int(seed) & 0xffffffff, _p(ws), _stream()))
        return dx, nxt
    _call("layernorm_bwd", L.sfm_layernorm_bwd_ex, (_p(x32), _p(gamma), _p(dy), dy16, _p(dres32), _p(dx), _p(dgamma), _p(dbeta), M, D,
                                                    x32.stride(0), dy.stride(0), D, eps, _dt(), _p(ws), _stream()))
    return dx


EW_SWISH_FWD, EW_SWISH_BWD, EW_GLU_FWD, EW_GLU_BWD, EW_SCALE_DROP, EW_GELU_FWD, EW_GELU_BWD, EW_CPEA_BWD = range(8)


def ew_train(mode, out, z=None, g=None, N=None, alpha=1.0, p=0.0, seed=0):
    L = _lib.load()
    M = out.shape[0]
    N = N if N is not None else (out.shape[1] // 2 if mode == EW_GLU_BWD else out.shape[1])
    _call("ew_train", L.sfm_ew_train, (_p(z), _p(g), _p(out), M, N, mode, 1 if (g is not None and g.dtype == torch.float32) else 0,
                                       1 if out.dtype == torch.float32 else 0, float(alpha), float(p), int(seed) & 0xffffffff,
                                       _dt(), _stream()))
    return out


def col_stats(y32, aux=None, mean=None, rstd=None):
    """-> S [C, 2] = {sum y, sum y^2}, or with aux {sum y, sum y * xhat(aux)}.  The training step does not call this: its
    statistics come from col_stats_shifted; the raw moments stay as a public entry point (sfm_col_stats), exercised by the tests"""
    L = _lib.load()
    M, C = y32.shape
    S = torch.zeros(C, 2, device=y32.device, dtype=torch.float32)
    ws = _ws(int(L.sfm_col_stats_ws_floats(M, C)), y32.device) if switch("deterministic") else None
    _call("col_stats", L.sfm_col_stats, (_p(y32), _p(aux), _p(mean), _p(rstd), _p(S), M, C, _p(ws), _stream()))
    return S


def col_stats_shifted(y32):
    """the sums of the BatchNorm statistics: -> S [C, 2] = {sum (y - K), sum (y - K)^2} and the shift K [C] (the mean of up to 128
    rows spread over the M: a fraction of a standard deviation from the mean, so S1 / M - (S0 / M)^2 does not cancel)"""
    L = _lib.load()
    M, C = y32.shape
    K = torch.empty(C, device=y32.device, dtype=torch.float32)
    S = torch.zeros(C, 2, device=y32.device, dtype=torch.float32)
    ws = _ws(int(L.sfm_col_stats_ws_floats(M, C)), y32.device) if switch("deterministic") else None
    _call("col_stats", L.sfm_col_pilot, (_p(y32), _p(K), M, C, _stream()))
    _call("col_stats", L.sfm_col_stats_shifted, (_p(y32), _p(K), _p(S), M, C, _p(ws), _stream()))
    return S, K


def add_cols(a, b, M, C, Cb):
    """out [M, C] fp32 = a[:, :C] + pad(b[:, :Cb]); a / b may be row-strided views"""
    L = _lib.load()
    out = torch.empty(M, C, device=a.device, dtype=torch.float32)
    _call("ew_train", L.sfm_add_cols, (_p(a), _p(b), _p(out), M, C, Cb, a.stride(0), b.stride(0), C, _stream()))
    return out


def lstm_hprev16(h32, B, T, H):
    L = _lib.load()
    out = torch.empty(B * T, 2 * H, device=h32.device, dtype=_state["dtype"])
    _call("convert_rows", L.sfm_lstm_hprev16, (_p(h32), _p(out), B, T, H, _dt(), _stream()))
    return out


def bn_finalize(S, K, gamma, beta, run_mean, run_var, M, eps, momentum, eval_mode=False):
    """S, K: the shifted sums and the shift of col_stats_shifted (None in eval mode) -> mean, rstd, sc [1, C], sh [1, C]; the
    fp32 running statistics are updated in place (training)"""
    L = _lib.load()
    C = gamma.numel()
    buf = torch.empty(4, C, device=gamma.device, dtype=torch.float32)
    _call("col_stats", L.sfm_bn_finalize, (_p(S), _p(K), _p(gamma), _p(beta), _p(run_mean), _p(run_var), _p(buf[0]), _p(buf[1]),
                                           _p(buf[2]), _p(buf[3]), C, M, float(eps), float(momentum), 1 if eval_mode else 0,
                                           _stream()))
    return buf[0], buf[1], buf[2:3], buf[3:4]


def bn_swish_bwd(g, y32, mean, rstd, gamma, beta, eval_mode=False):
    """backward through Swish(BatchNorm(y)): returns dy [M,C] fp32, dgamma, dbeta.  eval_mode: mean / rstd are the
    running statistics (constants), so dy carries no batch-statistics correction."""
    L = _lib.load()
    M, C = y32.shape
    S = torch.zeros(C, 2, device=y32.device, dtype=torch.float32)
    dy = torch.empty_like(y32)
    gf = 1 if g.dtype == torch.float32 else 0
    ws = _ws(int(L.sfm_col_stats_ws_floats(M, C)), y32.device) if switch("deterministic") else None
    for ps in (0, 1):
        Sx = torch.zeros_like(S) if (eval_mode and ps == 1) else S
        _call("bn_swish_bwd", L.sfm_bn_swish_bwd, (_p(g), _p(y32), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(Sx), _p(dy), M, C, gf,
                                                   ps, _dt(), _p(ws), _stream()))
    return dy, S[:, 1].contiguous(), S[:, 0].contiguous()


def dwconv_wgrad(x16, dy32, B, T, C, KS, dw=None, db=None):
    """-> dw [C, KS], db [C]; accumulated into dw / db when given (fp32), else into fresh zeros"""
    L = _lib.load()
    dw = torch.zeros(C, KS, device=x16.device, dtype=torch.float32) if dw is None else dw
    db = torch.zeros(C, device=x16.device, dtype=torch.float32) if db is None else db
    scratch = torch.empty(int(L.sfm_dwconv_wgrad_scratch_floats(B, T, C, KS)), device=x16.device, dtype=torch.float32)
    _call("dwconv_wgrad", L.sfm_dwconv_wgrad, (_p(x16), _p(dy32), _p(dw), _p(db), _p(scratch), B, T, C, KS, _dt(), _stream()))
    return dw, db


def attention_train(qkv16, B, T, H, hd, p_drop=0.0, seed=0):
    """training forward (q pre-scaled): returns O [B*T, D] 16-bit and LSE [B,H,T] fp32 (log2 domain)."""
    L = _lib.load()
    D = H * hd
    ld = qkv16.stride(0)
    out = torch.empty(B * T, D, device=qkv16.device, dtype=qkv16.dtype)
    lse = torch.empty(B, H, T, device=qkv16.device, dtype=torch.float32)
    _call("attention_fwd", L.sfm_attention_fwd_train, (_p(qkv16), _p(out), _p(lse), B, T, H, hd, ld, out.stride(0), D, 2 * D,
                                                       T * ld, T * out.stride(0), -1.0, float(p_drop), int(seed) & 0xffffffff,
                                                       _dt(), _stream()), 4.0 * B * H * T * T * hd, 4.0 * B * T * D * 2)
    return out, lse


def attention_bwd(qkv16, O16, dO16, lse, B, T, H, hd, p_drop=0.0, seed=0):
    L = _lib.load()
    D = H * hd
    dqkv = torch.empty_like(qkv16)
    if hd != 64:                                   # small-shape path (e.g. the reference's test config: 4 heads x 16)
        scratch = torch.zeros(B * T, 2 * D, device=qkv16.device, dtype=torch.float32)
        _call("attention_bwd", L.sfm_attention_bwd_generic, (_p(qkv16), _p(O16), _p(dO16), _p(lse), _p(scratch), _p(dqkv), B, T, H,
                                                             hd, qkv16.stride(0), O16.stride(0), D, 2 * D, float(p_drop),
                                                             int(seed) & 0xffffffff, _dt(), _stream()),
              10.0 * B * H * T * T * hd, 8.0 * B * T * D * 2)
        return dqkv
    delta = torch.empty(B, H, T, device=qkv16.device, dtype=torch.float32)
    _call("attention_bwd", L.sfm_attention_bwd, (_p(qkv16), _p(O16), _p(dO16), _p(lse), _p(delta), _p(dqkv), B, T, H, hd,
                                                 qkv16.stride(0), O16.stride(0), D, 2 * D, float(p_drop), int(seed) & 0xffffffff,
                                                 _dt(), _stream()), 10.0 * B * H * T * T * hd, 8.0 * B * T * D * 2)
    return dqkv


def set_lstm_w16(flag):
    """inference BiLSTM recurrence on fp16 operands (sfm_bilstm_layer_ex, default on; SFM_LSTM_W16=0 / False = fp32 W_hh and h)"""
    _SWITCHES["lstm_w16"][2] = bool(flag)


def lstm_w16():
    return switch("lstm_w16")


def bilstm_layer(xg, whh, B, T, H, w16=False):
    """one BiLSTM layer's recurrence (inference).  w16: recurrent product on fp16 operands (the fused path passes lstm_w16())"""
    L = _lib.load()
    out = torch.empty(B, T, 2 * H, device=xg.device, dtype=torch.float32)
    flops, nbytes = 2.0 * B * T * 2 * 4 * H * H, B * T * (8 * H + 2 * H) * 4
    if w16:
        _call("bilstm_layer", L.sfm_bilstm_layer_ex, (_p(xg), _p(whh), _p(out), B, T, H, 1, _stream()), flops, nbytes)
    else:
        _call("bilstm_layer", L.sfm_bilstm_layer, (_p(xg), _p(whh), _p(out), B, T, H, _dt(), _stream()), flops, nbytes)
    return out


def bilstm_layer_rows16(xg, whh, B, T, H, out16=None):
    """bilstm_layer(..., w16=True) at H 128 with the result as 16-bit rows [B * T, 2H] in the stage's format (`out16` may be a view
    with a wider row stride): bit for bit convert_rows of the fp32 result, which is never written"""
    L = _lib.load()
    if out16 is None:
        out16 = torch.empty(B * T, 2 * H, device=xg.device, dtype=compute_dtype())
    flops, nbytes = 2.0 * B * T * 2 * 4 * H * H, B * T * (8 * H * 4 + 2 * H * 2)
    _call("bilstm_layer", L.sfm_bilstm_layer_rows16, (_p(xg), _p(whh), _p(out16), out16.stride(0), B, T, H, 1, _dt(), _stream()),
          flops, nbytes)
    return out16


def bilstm_layer_train(xg, whh, B, T, H, w16=None):
    """forward of one BiLSTM layer that also saves the activated gates / cell states [B, T, 2, 5, H] for the BPTT.
    w16 (default: lstm_w16() when the training format is fp16): the recurrent product on fp16 operands, as under the reference's
    fp16 autocast; the saved state and the backward stay fp32"""
    L = _lib.load()
    out = torch.empty(B, T, 2 * H, device=xg.device, dtype=torch.float32)
    save = torch.empty(B, T, 2, 5, H, device=xg.device, dtype=torch.float32)
    if w16 is None:
        w16 = switch("lstm_w16") and _state["dtype"] == torch.float16
    if w16:
        _call("bilstm_layer", L.sfm_bilstm_layer_train_ex, (_p(xg), _p(whh), _p(out), _p(save), B, T, H, 1, _stream()))
    else:
        _call("bilstm_layer", L.sfm_bilstm_layer_train, (_p(xg), _p(whh), _p(out), _p(save), B, T, H, _dt(), _stream()))
    return out, save


def bilstm_layer_bwd(save, whh, dout, B, T, H):
    """dout [B, T, 2H] fp32 -> gradient w.r.t. the input projection xg [B, T, 2, 4H] fp32"""
    L = _lib.load()
    dxg = torch.empty(B, T, 2, 4 * H, device=dout.device, dtype=torch.float32)
    _call("bilstm_bwd", L.sfm_bilstm_layer_bwd, (_p(save), _p(whh), _p(dout), _p(dxg), B, T, H, _stream()))
    return dxg


def stft_lognorm_bwd(re, im, g, M, F):
    L = _lib.load()
    dre, dim_ = torch.empty_like(re), torch.empty_like(im)
    _call("stft_lognorm_bwd", L.sfm_stft_lognorm_bwd, (_p(re), _p(im), _p(g), _p(dre), _p(dim_), M, F, g.stride(0), _stream()))
    return dre, dim_


def memory_bwd(emb, params, d_out, d_gate, key_dim, value_dim, slots, temperature, want_d_emb=True):
    """-> (d_emb [B, key_dim] or None, dparams: blob laid out like `params`)"""
    L = _lib.load()
    Bn = emb.shape[0]
    d_emb = torch.empty(Bn, key_dim, device=emb.device, dtype=torch.float32) if want_d_emb else None
    dparams = torch.zeros_like(params)
    ws = None
    if switch("deterministic"):
        npar = int(L.sfm_memory_param_floats(key_dim, value_dim, slots))
        if npar != params.numel():
            raise RuntimeError("memory_bwd: the parameter blob has %d floats, the kernel's layout %d" % (params.numel(), npar))
        ws = _ws(L.sfm_memory_bwd_ws_floats(Bn, key_dim, value_dim, slots), emb.device)
    _call("memory_bwd", L.sfm_memory_bwd, (_p(emb), _p(params), _p(d_out), _p(d_gate), _p(d_emb), _p(dparams), Bn, key_dim, value_dim,
                                           slots, float(temperature), _p(ws), _stream()))
    return d_emb, dparams


def memory_fwd(emb, params, key_dim, value_dim, slots, temperature):
    L = _lib.load()
    Bn = emb.shape[0]
    dev = emb.device
    bias = torch.empty(Bn, value_dim, device=dev, dtype=torch.float32)
    gate = torch.empty(Bn, 1, device=dev, dtype=torch.float32)
    top = torch.empty(Bn, device=dev, dtype=torch.int32)
    sim = torch.empty(Bn, device=dev, dtype=torch.float32)
    _call("memory_fwd", L.sfm_memory_fwd, (_p(emb), _p(params), _p(bias), _p(gate), _p(top), _p(sim), Bn, key_dim, value_dim, slots,
                          float(temperature), _stream()))
    return bias, gate, top, sim


# ---------------------------------------------------------------------------
# constant operands for STFT / iSTFT as fp32 matrix products (host, float64 twiddles)
# ---------------------------------------------------------------------------
def _hann(n):
    k = np.arange(n, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)


def stft_matrix(n_fft, win, device):
    """[win, 2F] : columns [0,F) real part, [F,2F) imag part, restricted to the
    window support (torch.stft zero-pads the window to n_fft centred)."""
    F = n_fft // 2 + 1
    woff = (n_fft - win) // 2
    w = _hann(win)
    n = (np.arange(win, dtype=np.float64) + woff)[:, None]
    f = np.arange(F, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * ((n * f) % n_fft) / n_fft
    M = np.concatenate([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)], axis=1)
    return pack_f32_matrix(torch.from_numpy(M.astype(np.float32)).to(device))


def istft_matrix(n_fft, win, device):
    """[2F(+pad), win]: irfft restricted to the window support, times the window."""
    F = n_fft // 2 + 1
    woff = (n_fft - win) // 2
    w = _hann(win)
    n = (np.arange(win, dtype=np.float64) + woff)[None, :]
    f = np.arange(F, dtype=np.float64)[:, None]
    ang = 2.0 * np.pi * ((f * n) % n_fft) / n_fft
    coef = np.full((F, 1), 2.0)
    coef[0, 0] = 1.0
    if n_fft % 2 == 0:
        coef[F - 1, 0] = 1.0
    br = coef * np.cos(ang) / n_fft * w[None, :]
    bi = -coef * np.sin(ang) / n_fft * w[None, :]
    bi[0, :] = 0.0
    if n_fft % 2 == 0:
        bi[F - 1, :] = 0.0
    M = np.concatenate([br, bi], axis=0)
    win2 = torch.from_numpy((w * w).astype(np.float32)).to(device)
    return pack_f32_matrix(torch.from_numpy(M.astype(np.float32)).to(device)), win2


# ---------------------------------------------------------------------------
# MetacognitiveArbitrationAgent / VectorQuantizer kernels (routing.hip)
# ---------------------------------------------------------------------------
def maa_update_stats(sigma, stats, num_updates, momentum=0.1):
    """train()-mode EMA of agents/maa.py:126-135, in place on the device tensors stats [2] fp32 and num_updates int64 []"""
    L = _lib.load()
    acc = torch.zeros(2, device=sigma.device, dtype=torch.float64)
    _call("maa", L.sfm_maa_update_stats, (_p(sigma), sigma.numel(), _p(acc), _p(stats), _p(num_updates), float(momentum), _stream()),
          0.0, 4.0 * sigma.numel())


def maa_forward(sigma, stats, params):
    L = _lib.load()
    n = sigma.numel()
    dev = sigma.device
    logits = torch.empty(n, 4, device=dev, dtype=torch.float32)
    probs = torch.empty(n, 4, device=dev, dtype=torch.float32)
    dec = torch.empty(n, device=dev, dtype=torch.int64)
    conf = torch.empty(n, device=dev, dtype=torch.float32)
    _call("maa", L.sfm_maa_forward, (_p(sigma), _p(stats), _p(params), _p(logits), _p(probs), _p(dec), _p(conf), n, _stream()),
          2.0 * n * (64 + 64 * 64 + 4 * 64), n * 52.0)
    return logits, probs, dec, conf


def maa_backward(sigma, stats, params, g_logits, g_probs, g_conf):
    """-> dsigma [N] fp32, dparams fp32 [4548] in the layout of `params` (weight gradients as three TN GEMMs)"""
    L = _lib.load()
    n = sigma.numel()
    dev, dt = sigma.device, _state["dtype"]
    dsig = torch.empty(n, device=dev, dtype=torch.float32)
    H = torch.empty(4, n, 64, device=dev, dtype=dt)                     # H1, H2, dZ1, dZ2
    S = torch.empty(2, n, 8, device=dev, dtype=dt)                      # GL, XN
    _call("maa", L.sfm_maa_backward, (_p(sigma), _p(stats), _p(params), _p(g_logits), _p(g_probs), _p(g_conf), _p(dsig), _p(H[0]),
                                      _p(H[1]), _p(H[2]), _p(H[3]), _p(S[0]), _p(S[1]), n, _dt(), _stream()),
          4.0 * n * (64 * 64 * 2 + 8 * 64), n * (16.0 + 4 * 128 + 32))
    buf = torch.zeros(64 * 8 + 64 + 64 * 64 + 64 + 8 * 64 + 8, device=dev, dtype=torch.float32)
    o = 0
    dW1 = buf[o:o + 512].view(64, 8); o += 512
    db1 = buf[o:o + 64]; o += 64
    dW2 = buf[o:o + 4096].view(64, 64); o += 4096
    db2 = buf[o:o + 64]; o += 64
    dW3 = buf[o:o + 512].view(8, 64); o += 512
    db3 = buf[o:o + 8]
    gemm16_tn(H[2], S[1], dW1, db1)                                      # dZ1^T x [norm | 0...]: column 0 is dW1
    gemm16_tn(H[3], H[0], dW2, db2)
    gemm16_tn(S[0], H[1], dW3, db3)
    dparams = torch.cat([dW1[:, 0], db1, dW2.reshape(-1), db2, dW3[:4].reshape(-1), db3[:4]])
    return dsig, dparams


def vq_forward(x, centroids):
    """-> quantized fp32 (shape of x), indices int64, sum of squared distances (device double [1])"""
    L = _lib.load()
    x = x.contiguous()
    q = torch.empty_like(x)
    idx = torch.empty(x.shape, device=x.device, dtype=torch.int64)
    acc = torch.zeros(1, device=x.device, dtype=torch.float64)
    _call("vq", L.sfm_vq_forward, (_p(x), _p(centroids), centroids.numel(), _p(q), _p(idx), _p(acc), x.numel(), _stream()),
          0.0, 16.0 * x.numel())
    return q, idx, acc


def vq_backward(x, idx, centroids, g_q, g_loss, beta):
    L = _lib.load()
    dx = torch.empty_like(x)
    dcent = torch.zeros(centroids.numel(), device=x.device, dtype=torch.float32)
    _call("vq", L.sfm_vq_backward, (_p(x), _p(idx), _p(centroids), centroids.numel(), _p(g_q), _p(g_loss), float(beta), _p(dx),
                                     _p(dcent), x.numel(), _stream()), 0.0, 20.0 * x.numel())
    return dx, dcent


# ---------------------------------------------------------------------------
# AdversarialLoss (training/losses.py:150-289): csrc/adversarial.hip around gemm16 / conv_wgrad16 / conv_dgrad16
# ---------------------------------------------------------------------------
ADV_MAX_WIDTH = _K["ADV_MAX_WIDTH"]     # first-layer Cin after zero padding (257 bins -> 512)


def adv_plan(n_freq, channels):
    """the convs of SubDiscriminator(n_freq, channels) as the kernels see them: one dict per conv (the C -> 1 head last) with
    N, Cin, ksize, stride, pad, Cp (Cin zero-padded: a power of two >= 8 for sfm_gemm16's taps), Npad / Kpad of the packed
    weight, and its offsets in the call's two buffers (off16: W / sigma, 16-bit elements; off32: bias | u | v | W v | sigma)"""
    plan, cin, off16, off32 = [], int(n_freq), 0, 0
    specs = [(c, 5, 2 if i < len(channels) - 1 else 1, 2) for i, c in enumerate(channels)] + [(1, 3, 1, 1)]
    for n, k, stride, pad in specs:
        cp = 8
        while cp < cin:
            cp *= 2
        head = n == 1
        npad = 1 if head else (round_up(n, 128) if n > 64 and round_up(n, 128) - n < 64 else round_up(n, 64))
        kpad = k * cp if head else round_up(k * cp, 64)
        plan.append(dict(N=n, Cin=cin, ksize=k, stride=stride, pad=pad, Cp=cp, Npad=npad, Kpad=kpad, off16=off16, off32=off32))
        off16 += round_up(npad * kpad, 8)
        off32 += round_up(npad + 2 * n + cin * k + 1, 4)
        cin = n
    return plan, off16, off32


def adv_sn_table(plan, convs, device):
    """the device table sfm_adv_sn_fwd walks: 16 int64 words per conv (pointers of weight_orig, bias, weight_u, weight_v, then
    the plan's sizes and offsets)"""
    rows = []
    for L_, m in zip(plan, convs):
        rows.append([m.weight_orig.data_ptr(), m.bias.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr(), L_["N"], L_["Cin"],
                     L_["ksize"], L_["Cp"], L_["Npad"], L_["Kpad"], L_["off16"], L_["off32"], 0, 0, 0, 0])
    return torch.tensor(rows, dtype=torch.int64).to(device)


ADV_LO_SCALE = _K["ADV_LO_SCALE"]   # adversarial.hip: a forward operand is hi + lo / 2048


def adv_sn_views(L_, packed, saved, packed_lo=None):
    """(PackedWeight or the head's [3 C] row, bias, u, v, sigma) of one conv inside the buffers sfm_adv_sn_fwd filled; with
    packed_lo the same view of the lo words (zero bias: the correction GEMMs add to a result that has its bias)"""
    if packed_lo is not None:
        w = packed_lo[L_["off16"]:L_["off16"] + L_["Npad"] * L_["Kpad"]].view(L_["Npad"], L_["Kpad"])
        if L_["N"] == 1:
            return w
        return PackedWeight(w, _zero_bias(L_["Npad"], w.device), L_["N"], L_["ksize"] * L_["Cp"], L_["ksize"], L_["Cp"])
    n, k, cin = L_["N"], L_["ksize"], L_["Cin"]
    w = packed[L_["off16"]:L_["off16"] + L_["Npad"] * L_["Kpad"]].view(L_["Npad"], L_["Kpad"])
    o = L_["off32"]
    bias = saved[o:o + L_["Npad"]]
    u = saved[o + L_["Npad"]:o + L_["Npad"] + n]
    v = saved[o + L_["Npad"] + n:o + L_["Npad"] + n + cin * k]
    sigma = saved[o + L_["Npad"] + 2 * n + cin * k:o + L_["Npad"] + 2 * n + cin * k + 1]
    pw = w if n == 1 else PackedWeight(w, bias, n, k * L_["Cp"], k, L_["Cp"])
    return pw, bias, u, v, sigma


def adv_sn_fwd(table, plan, n16, n32, training, eps=1e-12):
    """spectral norm of every conv of one discriminator in ONE launch (a workgroup per conv): power iteration when `training`
    (weight_u / weight_v updated in place), sigma, W / sigma packed for gemm16 as hi / lo words
    -> (packed 16-bit [n16], packed_lo [n16], saved fp32 [n32])"""
    _need_dev(table)
    L = _lib.load()
    packed = torch.empty(n16, device=table.device, dtype=_state["dtype"])
    packed_lo = torch.empty(n16, device=table.device, dtype=_state["dtype"])
    saved = torch.empty(n32, device=table.device, dtype=torch.float32)
    nk = sum(p["N"] * p["Cin"] * p["ksize"] for p in plan)
    _call("adv_sn", L.sfm_adv_sn_fwd, (_p(table), len(plan), _p(packed), _p(packed_lo), _p(saved), 1 if training else 0,
                                       float(eps), _dt(), _stream()),
          (6.0 if training else 4.0) * nk, ((3 if training else 2) * 4.0 + 4.0) * nk + 4.0 * n16)
    return packed, packed_lo, saved


def adv_sn_bwd(G, weight_orig, u, v, sigma, dW, Cp, accumulate, db_in=None, db=None, g=None, cnorm=0.0):
    """dW [N, Cin, k] (= or +=) (G - <G, W / sigma> u v^T) / sigma / S, G [N, k, Cp] tap-major; db (= or +=) db_in / S.
    S = the power of two the pass's 16-bit tensors carry, derived from (g, cnorm) as in every backward kernel (g None: 1)"""
    _need_dev(G, weight_orig, dW, db_in, db, g)
    L = _lib.load()
    N, Cin, k = weight_orig.shape
    nk = N * Cin * k
    _call("adv_sn", L.sfm_adv_sn_bwd, (_p(G), _p(weight_orig), _p(u), _p(v), _p(sigma), _p(dW), _p(db_in), _p(db), _p(g),
                                       float(cnorm), N, Cin, k, Cp, 1 if accumulate else 0, _stream()), 6.0 * nk, (24.0 if accumulate else 20.0) * nk)
    return dW


def adv_stage(x, im, Cp, want32):
    """magnitudes [B, F, T] fp32 (im None), or (real, imag) [B, T, F] -> ((x16, x16lo) [B, T, Cp] zero-padded hi / lo words,
    x32 [B, T, F] or None)"""
    _need_dev(x, im)
    L = _lib.load()
    pair = im is not None
    if pair:
        B, T, F = x.shape
    else:
        B, F, T = x.shape
    x16 = torch.empty(B, T, Cp, device=x.device, dtype=_state["dtype"])
    lo = torch.empty_like(x16)
    x32 = torch.empty(B, T, F, device=x.device, dtype=torch.float32) if want32 else None
    n = B * T * F
    _call("adv_stage", L.sfm_adv_stage, (_p(x), _p(im), _p(x16), _p(lo), _p(x32), B, F, T, Cp, 1 if pair else 0, _dt(), _stream()),
          4.0 * n if pair else 0.0, (8.0 if pair else 4.0) * n + 4.0 * B * T * Cp + (4.0 * n if want32 else 0.0))
    return (x16, lo), x32


def adv_stage_bwd(d, re, im, B, F, T, g=None, cnorm=0.0):
    """adjoint of adv_stage: d [B, T, Cp] fp32 (carrying the pass's scale) -> d x [B, F, T], or (d re, d im) [B, T, F]; every
    element written"""
    _need_dev(d, re, im, g)
    L = _lib.load()
    pair = re is not None
    Cp = d.shape[-1]
    if pair:
        dx, dxi = torch.empty_like(re), torch.empty_like(im)
    else:
        dx, dxi = torch.empty(B, F, T, device=d.device, dtype=torch.float32), None
    n = B * T * F
    _call("adv_stage", L.sfm_adv_stage_bwd, (_p(d), _p(re), _p(im), _p(dx), _p(dxi), _p(g), float(cnorm), B, F, T, Cp,
                                             1 if pair else 0, _stream()),
          6.0 * n if pair else 0.0, (20.0 if pair else 8.0) * n)
    return dx, dxi


def adv_leaky(z, z_real=None, loss=None, scale=0.0):
    """(a16, a16lo) = LeakyReLU(0.2)(z) as hi / lo words; with z_real also loss[0] += scale * sum |leaky(z) - leaky(z_real)|,
    summed in order"""
    _need_dev(z, z_real, loss)
    L = _lib.load()
    n = z.numel()
    a16 = torch.empty(z.shape, device=z.device, dtype=_state["dtype"])
    lo = torch.empty_like(a16)
    ws = _ws64(L.sfm_adv_leaky_ws_doubles(n), z.device) if z_real is not None else None
    _call("adv_leaky", L.sfm_adv_leaky, (_p(z), _p(z_real), _p(a16), _p(lo), _p(ws), _p(loss), float(scale), n, _dt(), _stream()),
          (4.0 if z_real is not None else 1.0) * n, (12.0 if z_real is not None else 8.0) * n)
    return a16, lo


def adv_leaky_bwd(incoming, z, z_real, g, w_fm, cnorm):
    """dz16 = (incoming + S * w_fm * g * sign(leaky(z) - leaky(z_real))) * leaky'(z): the 16-bit dY of the gradient GEMMs"""
    _need_dev(incoming, z, z_real, g)
    L = _lib.load()
    n = z.numel()
    dz16 = torch.empty(z.shape, device=z.device, dtype=_state["dtype"])
    terms = (incoming is not None) + (z_real is not None)
    _call("adv_leaky", L.sfm_adv_leaky_bwd, (_p(incoming), _p(z), _p(z_real), _p(g), float(w_fm), float(cnorm), _p(dz16), n, _dt(),
                                             _stream()),
          (1.0 + 2.0 * terms) * n, (6.0 + 4.0 * terms) * n)
    return dz16


def adv_pool(in32, Cp, want32):
    """AvgPool1d(4, 2, 1) on channels-last rows: in32 [B, Tin, F] -> ((out16, out16lo) [B, Tin // 2, Cp] zero-padded hi / lo
    words, out32 or None)"""
    _need_dev(in32)
    L = _lib.load()
    B, Tin, F = in32.shape
    Tout = Tin // 2
    out16 = torch.empty(B, Tout, Cp, device=in32.device, dtype=_state["dtype"])
    lo = torch.empty_like(out16)
    out32 = torch.empty(B, Tout, F, device=in32.device, dtype=torch.float32) if want32 else None
    _call("adv_pool", L.sfm_adv_pool, (_p(in32), _p(out32), _p(out16), _p(lo), B, Tin, F, Cp, _dt(), _stream()),
          4.0 * B * Tout * F, 4.0 * B * Tin * F + 4.0 * B * Tout * Cp + (4.0 * B * Tout * F if want32 else 0.0))
    return (out16, lo), out32


def adv_pool_bwd(dnext, dx):
    """dx [B, Tin, Cp] += adjoint of AvgPool1d(4, 2, 1) applied to dnext [B, Tin // 2, Cp]"""
    _need_dev(dnext, dx)
    L = _lib.load()
    B, Tin, Cp = dx.shape
    _call("adv_pool", L.sfm_adv_pool_bwd, (_p(dnext), _p(dx), B, Tin, Cp, _stream()),
          3.0 * B * Tin * Cp, 8.0 * B * Tin * Cp + 4.0 * B * (Tin // 2) * Cp)
    return dx


def adv_head(a16, a16lo, w16, w16lo, bias, loss, target, scale):
    """Conv1d(C, 1, 3, pad 1) of a [B, T, C] (hi / lo words, as the weight) as a dot product per row -> out [B, T] fp32;
    loss[0] += scale * sum (out - target)^2"""
    _need_dev(a16, a16lo, w16, w16lo, bias, loss)
    L = _lib.load()
    B, T, C = a16.shape
    out = torch.empty(B, T, device=a16.device, dtype=torch.float32)
    ws = _ws64(L.sfm_adv_head_ws_doubles(B, T), a16.device)
    _call("adv_head", L.sfm_adv_head, (_p(a16), _p(a16lo), _p(w16), _p(w16lo), _p(bias), _p(out), _p(ws), _p(loss), float(target),
                                       float(scale), B, T, C, _dt(), _stream()),
          6.0 * B * T * C, 4.0 * B * T * C + 12.0 * C + 4.0 * B * T)
    return out


def adv_head_bwd(a16, w16, out, g, coef, cnorm, target, want_dw):
    """dout = g * coef * (out - target) -> (da [B, T, C] fp32 carrying the pass's scale, dwb = dw [3, C] tap-major | db or None)"""
    _need_dev(a16, w16, out, g)
    L = _lib.load()
    B, T, C = a16.shape
    da = torch.empty(B, T, C, device=a16.device, dtype=torch.float32)
    dwb = torch.empty(3 * C + 1, device=a16.device, dtype=torch.float32) if want_dw else None
    ws = None
    if want_dw:
        n = L.sfm_adv_head_bwd_ws_floats(B, T, C)
        ws = _ws(n, a16.device)
        ws = ws if ws is not None else torch.empty(n, device=a16.device, dtype=torch.float32)
    _call("adv_head", L.sfm_adv_head_bwd, (_p(a16), _p(w16), _p(out), _p(g), float(coef), float(cnorm), float(target), _p(da), _p(dwb),
                                           _p(ws),
                                           B, T, C, _dt(), _stream()),
          (12.0 if want_dw else 6.0) * B * T * C, (4.0 + (2.0 if want_dw else 0.0)) * B * T * C + 4.0 * B * T + 6.0 * C)
    return da, dwb


# ---------------------------------------------------------------------------
# CSII and NCM (csrc/intelligibility.hip; evaluation/csii.py, evaluation/ncm.py)
# ---------------------------------------------------------------------------
CSII_BINS = _K["CSII_BINS"]         # rfft(., 256) bins of the coherence
HE_ROWS = _K["HE_ROWS"]             # output samples per workgroup of the Hilbert kernel (its output tile)
HE_KSTEP = _K["HE_KSTEP"]           # input samples per staged k-step (one accumulation segment)
_HILBERT_TAB = {}                   # L -> fp32 [2 L], host (at most HILBERT_TAB_CACHE lengths)
HILBERT_TAB_CACHE = 1024


def hilbert_kernel_table(L):
    """float64 [L]: h with scipy.signal.hilbert(x).imag[n] = sum_m h[(n - m) mod L] x[m]: imag(ifft(H)), H = 1 at bin 0 (and at
    the Nyquist bin of an even L), 2 on the bins below L / 2, 0 above.  Host."""
    L = int(L)
    if L < 1:
        raise ValueError("hilbert_kernel_table: L %d" % L)
    H = np.zeros(L)
    if L % 2 == 0:
        H[0] = H[L // 2] = 1.0
        H[1:L // 2] = 2.0
    else:
        H[0] = 1.0
        H[1:(L + 1) // 2] = 2.0
    return np.fft.ifft(H).imag


def hilbert_table_host(L):
    """fp32 [2 L], the kernels' table.  Odd L: h twice back to back, so that h[(n - m) mod L] = table[n - m + L].  Even L: every
    even lag of h is exactly 0, so the outputs 2 i + p are a circular convolution of length L / 2 of the inputs 2 j + 1 - p with
    g_p[d] = h[(2 d + 2 p - 1) mod L]: g_0 twice, then g_1 twice.  Cached on the host by length (shared: do not modify)."""
    L = int(L)
    t = _HILBERT_TAB.get(L)
    if t is None:
        h = hilbert_kernel_table(L).astype(np.float32)
        if L % 2:
            t = np.concatenate([h, h])
        else:
            d = np.arange(L // 2)
            g0, g1 = h[(2 * d - 1) % L], h[(2 * d + 1) % L]
            t = np.concatenate([g0, g0, g1, g1])
        if len(_HILBERT_TAB) >= HILBERT_TAB_CACHE:
            _HILBERT_TAB.clear()
        _HILBERT_TAB[L] = t
    return t


def hilbert_table(lengths, device):
    """the tables of `lengths` (an int or a sequence of ints) back to back, one upload: fp32 [2 sum L] on the device"""
    lengths = [lengths] if np.isscalar(lengths) else list(lengths)
    return torch.from_numpy(np.concatenate([hilbert_table_host(L) for L in lengths])).to(device)


def hilbert_conv_len(L):
    """samples of one circular convolution of a signal of L samples: L, or L / 2 (twice) for an even L"""
    L = np.asarray(L, dtype=np.int64)
    return np.where(L % 2 == 0, L // 2, L)


def hilbert_tiles(lengths, min_len=1):
    """host tables of sfm_hilbert_env_moments for utterances of `lengths` samples: (tiles int32 [n, 2] = (utterance, tile),
    tile_off int32 [B + 1], sum over the tiles of their convolution's length); an odd length owns ceil(L / 256) tiles, an even one
    2 ceil(L / 512) (the two half-size problems one after the other), an utterance shorter than min_len none"""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    Lc = hilbert_conv_len(L)
    nt = np.where(L >= min_len, np.where(L % 2 == 0, 2, 1) * -(-Lc // HE_ROWS), 0)
    off = np.concatenate([[0], np.cumsum(nt)])
    utt = np.repeat(np.arange(L.size), nt)
    tile = np.arange(int(off[-1])) - np.repeat(off[:-1], nt)
    return np.ascontiguousarray(np.stack([utt, tile], axis=1), dtype=np.int32), off.astype(np.int32), int((nt * Lc).sum())


def csii_frames_varlen(cr, ci, er, ei, frame_off, weights, B, want_msc=False):
    """packed spectra rows [sum_frames, 129] of the clean and the enhanced pack, weights [129] fp64 -> score [B] fp64 (and the
    msc plane [B, 129] fp64)"""
    _need_dev(cr, ci, er, ei, frame_off, weights)
    L = _lib.load()
    if not (_is(cr, _F32, (None, CSII_BINS)) and all(_is(t, _F32, tuple(cr.shape)) for t in (ci, er, ei)) and
            _is(frame_off, None, B + 1, contig=False) and
            _is(weights, _F64, CSII_BINS, contig=False)):
        _refuse("csii_frames_varlen")
    n, F = cr.shape
    score = torch.empty(B, device=cr.device, dtype=torch.float64)
    msc = torch.empty(B, F, device=cr.device, dtype=torch.float64) if want_msc else None
    _call("intelligibility", L.sfm_csii_frames_varlen, (_p(cr), _p(ci), _p(er), _p(ei), _p(frame_off), _p(weights), _p(score), _p(msc),
                                                        B, n, F, _stream()), 14.0 * n * F, 16.0 * n * F)
    return (score, msc) if want_msc else score


def hilbert_env(x):
    """x [R, L] fp32 -> [R, L] fp32 = |scipy.signal.hilbert(x)| along the last axis"""
    _need_dev(x)
    L_ = _lib.load()
    if not _is(x, _F32, ndim=2, least=1):
        _refuse("hilbert_env")
    R, L = x.shape
    env = torch.empty_like(x)
    _call("hilbert_env", L_.sfm_hilbert_env, (_p(x), _p(hilbert_table(L, x.device)), _p(env), R, L, _stream()),
          2.0 * R * L * int(hilbert_conv_len(L)), 8.0 * R * L + 8.0 * L, "R%d L%d" % (R, L))
    return env


def hilbert_env_moments(X, tables, tab_off, lengths, tiles, C, tile_samples=0):
    """X [2, B, C, L] fp32 (clean, enhanced gammatone planes), tables / tab_off / lengths / tiles as sfm_hilbert_env_moments
    takes them -> partial [n_tiles, C, 5] fp64.  tile_samples: hilbert_tiles' third result (the launch's stated cost only)."""
    _need_dev(X, tables, tab_off, lengths, tiles)
    L_ = _lib.load()
    if not (_is(X, _F32, (2, None, C, None), least=1) and C <= GT_COLS and
            _is(tab_off, None, X.shape[1], contig=False) and
            _is(lengths, None, X.shape[1], contig=False) and
            _is(tiles, None, (None, 2), contig=False)):
        _refuse("hilbert_env_moments")
    _, B, _, L = X.shape
    n = tiles.shape[0]
    partial = torch.empty(max(n, 1), C, 5, device=X.device, dtype=torch.float64)
    _call("hilbert_env", L_.sfm_hilbert_env_moments, (_p(X), _p(tables), _p(tab_off), _p(lengths), _p(tiles), _p(partial), B, C, L, n,
                                                      _stream()),
          4.0 * C * HE_ROWS * tile_samples, 8.0 * B * C * L + 40.0 * n * C, "B%d C%d L%d tiles%d" % (B, C, L, n))
    return partial


def ncm_finish(partial, tile_off, lengths, weights, B, C):
    """partial [n_tiles, C, 5] fp64 -> (score [B], ncc [B, C]) fp64"""
    _need_dev(partial, tile_off, lengths, weights)
    L_ = _lib.load()
    if not (partial is not None and partial.dim() >= 1 and  # (its rows are the stated cost; nothing else is asked of it)
            _is(tile_off, None, B + 1, contig=False) and
            _is(lengths, None, B, contig=False) and
            _is(weights, _F64, C, contig=False)):
        _refuse("ncm_finish")
    ncc = torch.empty(B, C, device=partial.device, dtype=torch.float64)
    score = torch.empty(B, device=partial.device, dtype=torch.float64)
    _call("intelligibility", L_.sfm_ncm_finish, (_p(partial), _p(tile_off), _p(lengths), _p(weights), _p(ncc), _p(score), B, C,
                                                 _stream()), 5.0 * partial.shape[0] * C, 40.0 * partial.shape[0] * C)
    return score, ncc


# ---------------------------------------------------------------------------
# SpeechEnhancementDNN (csrc/dnn.hip)
# ---------------------------------------------------------------------------
DNN_ROW_TILE = _K["DNN_ROW_TILE"]   # rows of a workgroup of dnn_layer_kernel
DNN_ACT = {None: _K["DNN_ACT_NONE"], "relu": _K["DNN_ACT_RELU"], "sigmoid": _K["DNN_ACT_SIGMOID"]}
DNN_CONTEXT_MAX_K = _K["DNN_CONTEXT_MAX_K"]    # context rows with statistics: mean and std sit in LDS beside the tiles


def dnn_layer(a, pw, *, act=None, out=None, out_dtype=None, p_drop=0.0, seed=0, context=None, frames=None, mean=None, std=None):
    """out [M, pw.N] = act(A pw.w^T + pw.bias), one sfm_dnn_layer launch.  A is `a`, by its dtype and `context`:
      a 16-bit [M, >= round_up(pw.K, 8)], zero padded (rows16: a previous launch's result);
      a fp32 [M, pw.K] with any row stride (rows32: converted while staged);
      context=ctx: a = raw fp32 [B, T, D] contiguous (D even, >= 8), M = B T, pw.K = D (2 ctx + 1): the context rows of FeatureExtractor.add_context
        (frames int32 [B] = T_b or None; mean / std fp32 [pw.K] or None) are gathered, normalised and clipped while staged.
    act None / "relu" / "sigmoid"; p_drop > 0 (relu only): dropout with keep(seed, m N + n) after the ReLU.
    out (or out_dtype): 16-bit rows in the compute format [M, >= N], columns from N on written as zeros, or fp32 [M, N]."""
    _need_dev(a, out, frames, mean, std)
    L = _lib.load()
    dt = _state["dtype"]
    if pw.w.dtype != dt or pw.ksize != 1 or pw.glu:
        raise RuntimeError("dnn_layer: a plain Linear pack in the compute format %s is needed (got %s)" % (dt, pw.w.dtype))
    T = D = ctx = 0
    if context is not None:
        if not (_is(a, _F32, ndim=3, least=1) and 0 <= context <= 64 and
                a.shape[2] >= 8 and a.shape[2] % 2 == 0 and a.shape[2] * (2 * context + 1) == pw.K and
                _lengths_ok(frames, a.shape[0]) and
                (mean is None) == (std is None) and (mean is None or pw.K <= DNN_CONTEXT_MAX_K) and
                _is(mean, _F32, pw.K, opt=True) and _is(std, _F32, pw.K, opt=True)):
            _refuse("dnn_layer")
        mode, ctx, (B, T, D) = 2, int(context), a.shape
        M, lda, abytes = B * T, 0, 4.0 * a.numel() + (8.0 * pw.K if mean is not None else 0.0) + (4.0 * B if frames is not None else 0.0)
    else:
        K8 = round_up(pw.K, 8)
        if not (frames is None and mean is None and std is None and
                (_is(a, _F32, (None, pw.K), least=1, contig="last") or
                 (_is(a, dt, ndim=2, least=1, contig="last") and a.shape[1] >= K8 and a.stride(0) % 8 == 0))):
            _refuse("dnn_layer")
        M, lda = a.shape[0], a.stride(0)
        mode, abytes = (1, 4.0 * M * pw.K) if a.dtype == torch.float32 else (0, 2.0 * M * K8)
    if out is None:
        odt = out_dtype or dt
        out = torch.empty(M, pw.N if odt == torch.float32 else round_up(pw.N, 8), device=a.device, dtype=odt)
    if not ((_is(out, _F32, (M, pw.N), contig="last") or (_is(out, dt, (M, None), contig="last") and out.shape[1] >= pw.N)) and
            act in DNN_ACT):
        _refuse("dnn_layer")
    out_f32 = 1 if out.dtype == torch.float32 else 0
    # 16-bit rows: the columns N .. ldo are the next layer's K padding, written as zeros
    ldo = out.stride(0)
    osz = 4 if out_f32 else 2
    _call("dnn_layer", L.sfm_dnn_layer, (_p(a), _p(frames), _p(mean), _p(std), _p(pw.w), _p(pw.bias), _p(out), mode, M, pw.N, pw.K, lda,
                                         T, D, ctx, pw.Kpad, pw.Npad, ldo, out_f32, DNN_ACT[act], float(p_drop), int(seed) & 0xffffffff,
                                         _dt(), _stream()),
          2.0 * M * pw.N * pw.K, abytes + 2.0 * pw.Npad * pw.Kpad + 4.0 * pw.N + float(osz) * M * (pw.N if out_f32 else out.shape[1]),
          "M%d N%d K%d a%d act%d o%d%s" % (M, pw.N, pw.K, mode, DNN_ACT[act], osz, " drop" if p_drop > 0 else ""))
    return out


def dnn_act_bwd(dy, saved, act, N, p_drop=0.0, out=None):
    """dz [M, round_up(N, 64)] in the compute format = dy[:, :N] * act'(.), the columns from N on zeros: the cotangent of a
    layer's pre-activation as gemm16_tn and the data-gradient GEMM read it.  dy fp32 or 16-bit rows [M, >= N].
    act "relu": saved = the layer's 16-bit output h (positive exactly where the unit was active and kept),
    dz = dy (h > 0 ? 1 / (1 - p_drop) : 0); "sigmoid": saved = the fp32 output y, dz = dy y (1 - y); None: dz = dy."""
    _need_dev(dy, saved, out)
    L = _lib.load()
    dt = _state["dtype"]
    if not (_is(dy, None, ndim=2, rows=1, contig="last") and dy.dtype in (torch.float32, dt) and dy.shape[1] >= N and
            act in DNN_ACT and
            (act is None or (_is(saved, dt if act == "relu" else _F32, (dy.shape[0], None), contig="last") and saved.shape[1] >= N)) and
            (out is None or (_is(out, dt, (dy.shape[0], None)) and out.shape[1] >= N and out.shape[1] % 8 == 0))):
        _refuse("dnn_act_bwd")
    M = dy.shape[0]
    if out is None:
        out = torch.empty(M, round_up(N, 64), device=dy.device, dtype=dt)
    ssz = 0 if act is None else saved.element_size()
    _call("dnn_act_bwd", L.sfm_dnn_act_bwd, (_p(dy), 1 if dy.dtype == torch.float32 else 0, dy.stride(0), _p(saved),
                                             0 if saved is None else saved.stride(0), _p(out), out.shape[1], M, N, DNN_ACT[act],
                                             float(p_drop), _dt(), _stream()),
          2.0 * M * N, float(M) * N * (dy.element_size() + ssz) + 2.0 * M * out.shape[1], "M%d N%d act%d" % (M, N, DNN_ACT[act]))
    return out


# ---------------------------------------------------------------------------
# Training the DNN from a frame set kept at D columns (csrc/features.hip, dnn.hip, optim.hip; training/dnn_training.py)
# ---------------------------------------------------------------------------
MSE_GATHER_MAX_BLOCKS = _K["MSE_GATHER_MAX_BLOCKS"]     # sfm_mse_gather_loss: its scratch in doubles
MOMENTS_CHUNK_ROWS = _K["MOMENTS_CHUNK_ROWS"]           # sfm_context_moments: rows of a chunk at least
MOMENTS_MAX_CHUNKS = _K["MOMENTS_MAX_CHUNKS"]           # chunks at most: its scratch is (MOMENTS_MAX_CHUNKS + 1) K doubles


def context_moments(raw, bounds, ctx):
    """-> (mean, std) fp32 [D (2 ctx + 1)] of the context rows of the packed frames raw [N, D] fp32 (bounds int32 [N, 2]: each
    frame's utterance as first and one-past-last packed row), nan / inf read as 0, two fp64 passes, std < 1e-6 -> 1: the
    statistics of the reference's Dataset without its [N, K] rows.  Four launches, once per frame set."""
    _need_dev(raw, bounds)
    L = _lib.load()
    if not (_is(raw, _F32, ndim=2, least=1) and raw.shape[0] < 2 ** 31 and
            _is(bounds, _I32, (raw.shape[0], 2)) and
            0 <= int(ctx) <= 64):
        _refuse("context_moments")
    N, D = raw.shape
    K = D * (2 * int(ctx) + 1)
    mean = torch.empty(K, device=raw.device, dtype=torch.float32)
    std = torch.empty(K, device=raw.device, dtype=torch.float32)
    ws = _ws64((MOMENTS_MAX_CHUNKS + 1) * K, raw.device)
    _call("context_moments", L.sfm_context_moments, (_p(raw), _p(bounds), _p(mean), _p(std), _p(ws), N, D, int(ctx), _stream()),
          5.0 * N * K, 2.0 * (4.0 * N * D + 8.0 * N) + 8.0 * K, "N%d D%d ctx%d" % (N, D, ctx))
    return mean, std


def dnn_layer_indexed(raw, bounds, index, pw, *, context, act=None, out=None, out_dtype=None, p_drop=0.0, seed=0, mean=None, std=None,
                      a16_out=None):
    """out [M, pw.N] = act(A pw.w^T + pw.bias), one sfm_dnn_layer_indexed launch: row m of A is the context row (FeatureExtractor.
    add_context: clamped to the utterance, normalised with mean / std [pw.K] when given, clipped to +-10) of packed frame index[m]
    of raw [N, D] (bounds int32 [N, 2]; index int32 [M], < 0: a zero row, repeats allowed).  a16_out [M, round_up(pw.K, 64)] in the
    compute format (True: allocated): the staged operand rows, zero padded - returned beside out when asked for."""
    _need_dev(raw, bounds, index, out, mean, std, a16_out if torch.is_tensor(a16_out) else None)
    L = _lib.load()
    dt = _state["dtype"]
    if pw.w.dtype != dt or pw.ksize != 1 or pw.glu:
        raise RuntimeError("dnn_layer_indexed: a plain Linear pack in the compute format %s is needed (got %s)" % (dt, pw.w.dtype))
    if not _is(raw, _F32, ndim=2, least=1):
        _refuse("dnn_layer_indexed")
    (N, D), ctx = raw.shape, int(context)
    if not (N < 2 ** 31 and D >= 8 and D % 2 == 0 and 0 <= ctx <= 64 and D * (2 * ctx + 1) == pw.K and
            _is(bounds, _I32, (N, 2)) and
            _is(index, _I32, ndim=1, least=1) and
            (mean is None) == (std is None) and (mean is None or pw.K <= DNN_CONTEXT_MAX_K) and
            _is(mean, _F32, pw.K, opt=True) and _is(std, _F32, pw.K, opt=True)):
        _refuse("dnn_layer_indexed")
    M = index.numel()
    K64 = round_up(pw.K, 64)
    want_a16 = a16_out is not None and a16_out is not False
    odt = out_dtype or dt
    if not ((not want_a16 or a16_out is True or _is(a16_out, dt, (M, K64))) and
            (odt in (torch.float32, dt) if out is None else
             _is(out, _F32, (M, pw.N), contig="last") or (_is(out, dt, (M, None), contig="last") and out.shape[1] >= pw.N)) and
            act in DNN_ACT):
        _refuse("dnn_layer_indexed")
    if a16_out is True:
        a16_out = torch.empty(M, K64, device=raw.device, dtype=dt)
    if out is None:
        out = torch.empty(M, pw.N if odt == torch.float32 else round_up(pw.N, 8), device=raw.device, dtype=odt)
    out_f32 = 1 if out.dtype == torch.float32 else 0
    osz = 4 if out_f32 else 2
    # each gathered raw row read once per context column block (2 ctx + 1 times D floats per operand row), index and bounds once
    abytes = 4.0 * M * pw.K + 12.0 * M + (8.0 * pw.K if mean is not None else 0.0) + (2.0 * M * K64 if want_a16 else 0.0)
    _call("dnn_layer", L.sfm_dnn_layer_indexed,
          (_p(raw), _p(bounds), _p(index), _p(mean), _p(std), _p(pw.w), _p(pw.bias), _p(out), _p(a16_out) if want_a16 else None, M, pw.N,
           pw.K, N, D, ctx, pw.Kpad, pw.Npad, out.stride(0), K64 if want_a16 else 0, out_f32, DNN_ACT[act], float(p_drop),
           int(seed) & 0xffffffff, _dt(), _stream()),
          2.0 * M * pw.N * pw.K, abytes + 2.0 * pw.Npad * pw.Kpad + 4.0 * pw.N + float(osz) * M * (pw.N if out_f32 else out.shape[1]),
          "M%d N%d K%d a3 act%d o%d%s" % (M, pw.N, pw.K, DNN_ACT[act], osz, " drop" if p_drop > 0 else ""))
    return (out, a16_out) if want_a16 else out


def mse_gather_loss(y, mask, index, *, loss_scale=None, need_dz=True, rec=None, ctl=None, loss=None, dz=None):
    """nn.MSELoss()(y, clip(nan_to_num(mask[index]), 0, 1)) of y fp32 [M, C] against the rows index (int32 [M]) of mask fp32 [N, C]
    -> (loss fp32 [1], dz or None), two launches.  dz [M, round_up(C, 64)] in the compute format = S 2 (y - t) / (M C) y (1 - y),
    zero padded: the output layer's pre-activation cotangent as the gradient GEMMs read it, S = loss_scale[0] on the device
    (optim.DynamicLossScale.state; None: 1).  rec: 4 doubles {sum of finite losses, finite batches, non-finite batches, last loss},
    updated in place; ctl: an optimiser's control block, ctl[2] is raised when the loss is not finite."""
    _need_dev(y, mask, index, loss_scale, rec, ctl, loss, dz)
    L = _lib.load()
    dt = _state["dtype"]
    if not need_dz:
        dz = None
    if not _is(y, _F32, ndim=2, least=1):
        _refuse("mse_gather_loss")
    M, C = y.shape
    Cz = round_up(C, 64)
    if not (_is(mask, _F32, ndim=2, least=1) and mask.shape[1] == C and
            _is(index, _I32, (M,)) and
            (loss_scale is None or _is(loss_scale, _F32, least=1, contig=False)) and
            (rec is None or _is(rec, _F64, 4)) and
            (ctl is None or _is(ctl, _F64, least=8)) and
            (dz is None or _is(dz, dt, (M, Cz)))):
        _refuse("mse_gather_loss")
    if need_dz and dz is None:
        dz = torch.empty(M, Cz, device=y.device, dtype=dt)
    if loss is None:
        loss = torch.empty(1, device=y.device, dtype=torch.float32)
    ws = _ws64(MSE_GATHER_MAX_BLOCKS, y.device)
    _call("mse_loss", L.sfm_mse_gather_loss, (_p(y), _p(mask), _p(index), _p(loss_scale), _p(dz), Cz, _p(loss), _p(rec), _p(ctl), _p(ws),
                                              M, C, mask.shape[0], _dt(), _stream()),
          (8.0 if need_dz else 3.0) * M * C, 8.0 * M * C + 4.0 * M + (2.0 * M * Cz if need_dz else 0.0), "M%d C%d dz%d" % (M, C, int(need_dz)))
    return loss, dz


# ---------------------------------------------------------------------------
# Mask to waveform (csrc/resynth.hip; steps 2-4 of enhance_signal, training/pipeline.py:877-934)
# ---------------------------------------------------------------------------
RESYNTH_TILE_FRAMES = _K["RESYNTH_TILE_FRAMES"]    # frames a workgroup computes; it owns one output hop fewer
RESYNTH_BWD_TILE_FRAMES = _K["RESYNTH_BWD_TILE_FRAMES"]    # frames (rows of dmask) a workgroup of the mask adjoint computes
RESYNTH_MAX_NFFT = _K["RESYNTH_MAX_NFFT"]          # the largest n_fft / frame the kernel's LDS layout holds
RESYNTH_MAX_FRAME = _K["RESYNTH_MAX_FRAME"]
RESYNTH_MAX_CHANNELS = _K["RESYNTH_MAX_CHANNELS"]
RESYNTH_COL_ALIGN = _K["RESYNTH_COL_ALIGN"]
_RESYNTH_OPS = {}                                  # (frame, hop, n_fft, fs, cf, device) -> device operands
RESYNTH_OPS_CACHE = 16


def resynth_supported(frame, hop, n_fft, C):
    """the shapes sfm_mask_resynth takes (everything else is SFM_ERR_SHAPE there)"""
    return hop > 0 and hop * 2 == frame and frame <= n_fft and n_fft % 2 == 0 and n_fft <= RESYNTH_MAX_NFFT and \
        frame <= RESYNTH_MAX_FRAME and 2 <= C <= RESYNTH_MAX_CHANNELS


def resynth_matrices_host(frame, n_fft):
    """float64 (Wf [frame, n_fft], Wi [n_fft, frame]) with w = np.hanning(frame), phases (n k) mod n_fft as in stft_matrix:
    x[frame] @ Wf = the n_fft real numbers of rfft(x w, n_fft) - Re X[0 .. F - 1], then Im X[1 .. F - 2] (the imaginary parts of
    DC and Nyquist are identically zero and have no column); that row @ Wi = irfft(X, n_fft)[:frame] w."""
    F = n_fft // 2 + 1
    w = np.hanning(frame)
    n = np.arange(frame, dtype=np.int64)
    k = np.arange(F, dtype=np.int64)
    ang = 2.0 * np.pi * ((n[:, None] * k[None, :]) % n_fft) / n_fft
    Wf = np.concatenate([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang[:, 1:F - 1])], axis=1)
    coef = np.full(F, 2.0)
    coef[0] = coef[F - 1] = 1.0
    Wi = np.concatenate([(coef[:, None] * np.cos(ang.T)) / n_fft * w[None, :],
                         (-coef[1:F - 1, None] * np.sin(ang.T[1:F - 1])) / n_fft * w[None, :]], axis=0)
    return Wf, Wi


def resynth_interp_table(fs, n_fft, cf):
    """np.interp(k (fs / 2) / (F - 1), cf, m, left=m[0], right=m[-1]) as a table per bin k: (idx int64 [F], wt float64 [F]) with the
    value (1 - wt) m[idx] + wt m[idx + 1], 0 <= idx <= len(cf) - 2: idx = the interval of cf the bin frequency falls into, wt its
    position in it, clipped to [0, 1] (so a bin below cf[0] takes m[0] and one above cf[-1] takes m[-1]).  cf ascending, float64."""
    cf = np.asarray(cf, dtype=np.float64).reshape(-1)
    if cf.size < 2 or not np.all(np.diff(cf) > 0):
        raise ValueError("resynth_interp_table: the centre frequencies must be at least 2 and strictly ascending")
    F = n_fft // 2 + 1
    x = np.arange(F, dtype=np.float64) * (float(fs) / 2.0) / (F - 1)
    idx = np.clip(np.searchsorted(cf, x, side="right") - 1, 0, cf.size - 2)
    wt = np.clip((x - cf[idx]) / (cf[idx + 1] - cf[idx]), 0.0, 1.0)
    return idx.astype(np.int64), wt


def resynth_inv_wsum_host(frame, hop):
    """float64 [3, hop]: 1 / (sum of np.hanning(frame) ** 2 over the frames that cover a sample) for the utterance's first hop (frame
    0 alone), an interior hop (two frames) and the last covered hop (the last frame alone); a sum below 1e-8 counts as 1"""
    w2 = np.hanning(frame) ** 2
    ws = np.stack([w2[:hop], w2[:hop] + w2[hop:], w2[hop:]])
    ws[ws < 1e-8] = 1.0
    return 1.0 / ws


def resynth_channel_bins(idx, C):
    """the inverse of resynth_interp_table's idx (ascending in the bin k): int32 [C + 1] with the bins of lower channel c being
    bins[c] .. bins[c + 1] - 1, so bins[0] = 0 and bins[C - 1] = bins[C] = F (no bin has the last channel as its lower one)"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size == 0 or np.any(np.diff(idx) < 0) or idx[0] < 0 or idx[-1] > C - 2:
        raise ValueError("resynth_channel_bins: the lower channels must ascend within 0 .. C - 2")
    return np.searchsorted(idx, np.arange(C + 1), side="left").astype(np.int32)


def resynth_operands(frame, hop, n_fft, fs, cf, device, bwd=False):
    """the device operands of sfm_mask_resynth (Wf, Wi, tab_idx, tab_wt, inv_wsum), built in float64 and cast to fp32, cached by
    (frame, hop, n_fft, fs, cf) per device (shared: do not modify).  bwd: followed by the two that sfm_mask_resynth_bwd adds, WiT
    [FR, NC] (Wi transposed) and chan_bins int32 [C + 1] (resynth_channel_bins), built and cached with the five."""
    cf = np.ascontiguousarray(cf, dtype=np.float64).reshape(-1)
    key = (int(frame), int(hop), int(n_fft), float(fs), cf.tobytes(), str(device))
    ops_ = _RESYNTH_OPS.get(key)
    if ops_ is None:
        F = n_fft // 2 + 1
        NC, FR = round_up(n_fft, RESYNTH_COL_ALIGN), round_up(frame, RESYNTH_COL_ALIGN)
        Wf64, Wi64 = resynth_matrices_host(frame, n_fft)
        Wf = np.zeros((FR, NC), dtype=np.float32)
        Wf[:frame, :n_fft] = Wf64
        Wi = np.zeros((NC, FR), dtype=np.float32)
        Wi[:n_fft, :frame] = Wi64
        idx, wt = resynth_interp_table(fs, n_fft, cf)
        col_bin = np.concatenate([np.arange(F), np.arange(1, F - 1)])           # the bin of every operand column
        tab_idx = np.zeros(NC, dtype=np.int32)
        tab_wt = np.zeros(NC, dtype=np.float32)
        tab_idx[:n_fft], tab_wt[:n_fft] = idx[col_bin], wt[col_bin]
        host = (Wf, Wi, tab_idx, tab_wt, resynth_inv_wsum_host(frame, hop).astype(np.float32), Wi.T, resynth_channel_bins(idx, cf.size))
        ops_ = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in host)
        if len(_RESYNTH_OPS) >= RESYNTH_OPS_CACHE:
            _RESYNTH_OPS.clear()
        _RESYNTH_OPS[key] = ops_
    return ops_ if bwd else ops_[:5]


def mask_resynth(noisy, mask, lengths=None, *, frame, hop, n_fft, fs, cf, out=None, frames=None):
    """noisy [B, L] fp32, mask [B, T_mask, C] fp32, lengths int32 [B] on the device or None (= L) -> out [B, L] fp32: one
    sfm_mask_resynth launch.  cf: the C ascending centre frequencies of the mask's channels (host).  frames: the number of frames
    the launch computes, sum_b min(T_b, T_mask), for its stated cost (None: every utterance is L samples long)."""
    _need_dev(noisy, mask, lengths, out)
    L_ = _lib.load()
    if not (_is(noisy, _F32, ndim=2, least=1) and
            _is(mask, _F32, (noisy.shape[0], None, len(cf)), least=1) and resynth_supported(frame, hop, n_fft, len(cf)) and
            _lengths_ok(lengths, noisy.shape[0]) and
            _is(out, _F32, tuple(noisy.shape), opt=True)):
        _refuse("mask_resynth")
    B, L = noisy.shape
    T_mask, C = mask.shape[1], mask.shape[2]
    if out is None:
        out = torch.empty(B, L, device=noisy.device, dtype=torch.float32)
    Wf, Wi, tab_idx, tab_wt, inv_wsum = resynth_operands(frame, hop, n_fft, fs, cf, noisy.device)
    if frames is None:
        frames = B * min((L - frame) // hop + 1 if L >= frame else 0, T_mask)
    two_f = n_fft + 2
    nbytes = 4.0 * (noisy.numel() + mask.numel() + Wf.numel() + Wi.numel() + tab_idx.numel() + tab_wt.numel() + inv_wsum.numel() +
                    (0 if lengths is None else B) + out.numel())
    _call("resynth", L_.sfm_mask_resynth, (_p(noisy), _p(mask), _p(lengths), _p(Wf), _p(Wi), _p(tab_idx), _p(tab_wt), _p(inv_wsum),
                                           _p(out), B, L, T_mask, frame, hop, n_fft, C, _stream()),
          (2.0 * frame * two_f + 2.0 * two_f * frame) * frames, nbytes, "B%d L%d T%d f%d n%d C%d" % (B, L, T_mask, frame, n_fft, C))
    return out


def mask_resynth_bwd(noisy, dout, lengths=None, *, frame, hop, n_fft, fs, cf, T_mask, out=None, frames=None):
    """noisy [B, L] fp32, dout [B, L] fp32 (the cotangent of mask_resynth's result), lengths as there -> dmask [B, T_mask, C] fp32,
    the cotangent of the mask, every element written: one sfm_mask_resynth_bwd launch.  The forward is linear in the mask, so the
    mask is no argument; the gradient to `noisy` is not offered.  frames: as mask_resynth, for the stated cost."""
    _need_dev(noisy, dout, lengths, out)
    L_ = _lib.load()
    C = len(cf)
    T_mask = int(T_mask)
    if not (_is(noisy, _F32, ndim=2, least=1) and
            _is(dout, _F32, tuple(noisy.shape)) and
            _lengths_ok(lengths, noisy.shape[0]) and
            T_mask > 0 and resynth_supported(frame, hop, n_fft, C) and
            _is(out, _F32, (noisy.shape[0], T_mask, C), opt=True)):
        _refuse("mask_resynth_bwd")
    B, L = noisy.shape
    if out is None:
        out = torch.empty(B, T_mask, C, device=noisy.device, dtype=torch.float32)
    Wf, _, _, tab_wt, inv_wsum, WiT, chan_bins = resynth_operands(frame, hop, n_fft, fs, cf, noisy.device, bwd=True)
    if frames is None:
        frames = B * min((L - frame) // hop + 1 if L >= frame else 0, T_mask)
    two_f = n_fft + 2
    nbytes = 4.0 * (noisy.numel() + dout.numel() + Wf.numel() + WiT.numel() + tab_wt.numel() + inv_wsum.numel() + chan_bins.numel() +
                    (0 if lengths is None else B) + out.numel())
    _call("resynth_bwd", L_.sfm_mask_resynth_bwd, (_p(noisy), _p(dout), _p(lengths), _p(Wf), _p(WiT), _p(tab_wt), _p(inv_wsum),
                                                   _p(chan_bins), _p(out), B, L, T_mask, frame, hop, n_fft, C, _stream()),
          2.0 * (2.0 * frame * two_f) * frames, nbytes, "B%d L%d T%d f%d n%d C%d" % (B, L, T_mask, frame, n_fft, C))
    return out


# ---------------------------------------------------------------------------
# RBM pre-training (csrc/rbm.hip; models/rbm.py of the reference)
# ---------------------------------------------------------------------------
RBM_TILE = _K["RBM_TILE"]                    # a workgroup's 32 x 32 output tile; ceil(n_visible / RBM_TILE) fp64 error partials per step
RBM_MAX_UNITS = _K["RBM_MAX_UNITS"]
RBM_MAX_BATCH = _K["RBM_MAX_BATCH"]
RBM_SAMPLE = {None: _K["RBM_SAMPLE_NONE"], "replay": _K["RBM_SAMPLE_REPLAY"], "counter": _K["RBM_SAMPLE_COUNTER"]}


def rbm_error_tiles(n_visible):
    """fp64 partials sfm_rbm_update writes per step"""
    return (int(n_visible) + RBM_TILE - 1) // RBM_TILE


def rbm_prob(data, W, bias, *, down=False, rows=None, M=None, prob=None, sample=None, u=None, seed=None):
    """prob [M, N] = sigmoid(A op(W) + bias), one sfm_rbm_prob launch.  W fp32 [n_visible, n_hidden] contiguous; down=False: A rows
    of n_visible values, op(W) = W, bias = h_bias [n_hidden]; down=True: rows of n_hidden values, op(W) = W^T, bias = v_bias.
    Row m of A = data[rows[m]] (rows int32 [M] on the device) or data[m] for m < M (default: every row of data).
    u fp64 [M, N]: also the sample plane (prob > u) as fp32 0 / 1 (replay); seed: the sample plane of the counter rule of
    include/sincformer_hip.h; neither: probabilities only.  -> prob, or (prob, sample)."""
    _need_dev(data, W, bias, rows, prob, sample, u)
    L = _lib.load()
    if not (_is(W, _F32, ndim=2) and 1 <= W.shape[0] <= RBM_MAX_UNITS and 1 <= W.shape[1] <= RBM_MAX_UNITS):
        _refuse("rbm_prob")
    V, H = W.shape
    K, N = (H, V) if down else (V, H)
    if M is None:
        M = rows.numel() if rows is not None else (data.shape[0] if _is(data, None, ndim=2, contig=False) else 0)
    M = int(M)
    if not (M >= 1 and
            _is(data, _F32, (None, K), rows=1 if rows is not None else M, contig="last") and data.stride(0) >= K and
            _is(rows, _I32, (M,), opt=True) and
            _is(bias, _F32, N) and
            not (u is not None and seed is not None) and _is(u, _F64, M * N, opt=True)):
        _refuse("rbm_prob")
    mode = "replay" if u is not None else ("counter" if seed is not None else None)
    if prob is None:
        prob = torch.empty(M, N, device=data.device, dtype=torch.float32)
    if mode is not None and sample is None:
        sample = torch.empty(M, N, device=data.device, dtype=torch.float32)
    if not (_is(prob, _F32, M * N) and (mode is None or _is(sample, _F32, M * N))):
        _refuse("rbm_prob")
    if mode is None and sample is not None:                 # a sample plane without a source of randomness: the header's ERR_ARG
        _lib.check(_K["ERR_ARG"], "rbm_prob")
    nbytes = 4.0 * (M * K + V * H + N + M * N) + (4.0 * M if rows is not None else 0.0) + \
        (4.0 * M * N if mode is not None else 0.0) + (8.0 * M * N if mode == "replay" else 0.0)
    _call("rbm_prob", L.sfm_rbm_prob, (_p(data), _p(rows), _p(W), _p(bias), _p(prob), _p(sample) if mode is not None else None, _p(u),
                                       M, V, H, data.shape[0], data.stride(0), 1 if down else 0, RBM_SAMPLE[mode],
                                       (int(seed) & 0xffffffff) if seed is not None else 0, _stream()),
          2.0 * M * N * K, nbytes, "M%d N%d K%d %s s%d" % (M, N, K, "down" if down else "up", RBM_SAMPLE[mode]))
    return prob if mode is None else (prob, sample)


def rbm_update(data, ph, nv, nh, W, v_bias, h_bias, err_partial, lr, *, rows=None, B=None):
    """W += (lr / B) (v^T ph - nv^T nh), v_bias += lr mean(v - nv), h_bias += lr mean(ph - nh) in place, and err_partial
    [rbm_error_tiles(n_visible)] fp64 = the partial sums of (v - nv)^2: one sfm_rbm_update launch.  v[b] = data[rows[b]] (rows int32
    [B]) or data[b]; ph, nh [B, n_hidden], nv [B, n_visible] fp32 contiguous (their first B rows when they hold more)."""
    _need_dev(data, ph, nv, nh, W, v_bias, h_bias, err_partial, rows)
    L = _lib.load()
    if not (_is(W, _F32, ndim=2) and 1 <= W.shape[0] <= RBM_MAX_UNITS and 1 <= W.shape[1] <= RBM_MAX_UNITS):
        _refuse("rbm_update")
    V, H = W.shape
    if B is None:
        B = rows.numel() if rows is not None else (data.shape[0] if _is(data, None, ndim=2, contig=False) else 0)
    B = int(B)
    if not (1 <= B <= RBM_MAX_BATCH and
            _is(data, _F32, (None, V), rows=1 if rows is not None else B, contig="last") and data.stride(0) >= V and
            _is(rows, _I32, (B,), opt=True) and
            _is(ph, _F32, (None, H), rows=B) and
            _is(nv, _F32, (None, V), rows=B) and
            _is(nh, _F32, (None, H), rows=B) and
            _is(v_bias, _F32, V) and
            _is(h_bias, _F32, H) and
            _is(err_partial, _F64, least=rbm_error_tiles(V))):
        _refuse("rbm_update")
    nbytes = 4.0 * (2 * B * V + 2 * B * H) + 8.0 * (V * H + V + H) + 8.0 * rbm_error_tiles(V) + (4.0 * B if rows is not None else 0.0)
    _call("rbm_update", L.sfm_rbm_update, (_p(data), _p(rows), _p(ph), _p(nv), _p(nh), _p(W), _p(v_bias), _p(h_bias), _p(err_partial),
                                           B, V, H, data.shape[0], data.stride(0), float(lr), _stream()),
          2.0 * (2 * B) * V * H + 3.0 * B * V + 2.0 * B * H, nbytes, "B%d V%d H%d" % (B, V, H))


def rbm_fold_error(partial, out, n_steps, num_samples, batch_size, n_visible):
    """out[0] (fp64) = the mean over an epoch's n_steps batches of each batch's mean squared reconstruction error, from the
    partials [n_steps, rbm_error_tiles(n_visible)] that rbm_update wrote: one small launch, fixed order"""
    _need_dev(partial, out)
    L = _lib.load()
    tiles = rbm_error_tiles(n_visible)
    if not (_is(partial, _F64, least=n_steps * tiles) and
            _is(out, _F64, least=1, contig=False) and
            n_steps == (num_samples + batch_size - 1) // max(batch_size, 1)):
        _refuse("rbm_fold_error")
    _call("rbm_fold", L.sfm_rbm_fold_error, (_p(partial), _p(out), int(n_steps), tiles, int(num_samples), int(batch_size), int(n_visible),
                                             _stream()), float(n_steps) * (tiles + 2), 8.0 * n_steps * tiles + 8.0)


# ---------------------------------------------------------------------------
# STOI of Taal et al. and ESTOI (csrc/stoi.hip; evaluation/stoi_taal.py plans the tables)
# ---------------------------------------------------------------------------
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT = _K["STOI_FS"], _K["STOI_FRAME"], _K["STOI_HOP"], _K["STOI_NFFT"]
STOI_BANDS, STOI_SEG, STOI_FIRST_BIN, STOI_LAST_BIN = _K["STOI_BANDS"], _K["STOI_SEG"], _K["STOI_FIRST_BIN"], _K["STOI_LAST_BIN"]
STOI_DFT_COLS, STOI_ROW_TILE, STOI_SEG_TILE = _K["STOI_DFT_COLS"], _K["STOI_ROW_TILE"], _K["STOI_SEG_TILE"]
STOI_TAP_HALF, STOI_MAX_RATE, STOI_BWD_ROWS = _K["STOI_TAP_HALF"], _K["STOI_MAX_RATE"], _K["STOI_BWD_ROWS"]
STOI_NBIN = STOI_LAST_BIN - STOI_FIRST_BIN + 1


def stoi_resample(sig, taps, in_off, in_len, out_off, out_len, B, n_out, max_out_len, n_in, up, down, padl, out=None):
    """polyphase FIR to 10 kHz: sig fp32 (flat), utterance u = sig[in_off[u] : in_off[u] + in_len[u]] -> out fp32 [n_out], utterance u at
    out_off[u], out_len[u] samples; taps fp32 [K, up] (evaluation.stoi_taal.resample_operand).  fp32 operands, fp64 sums.  n_out,
    max_out_len, n_in: host sums / maximum (sizes and the cost).  out: a buffer of the caller's (the adjoint's zero-padded rows)."""
    _need_dev(sig, taps, in_off, in_len, out_off, out_len, out)
    L = _lib.load()
    if not (_is(sig, _F32) and
            _is(taps, _F32, (None, up)) and
            _is(in_off, _I32, B) and _is(in_len, _I32, B) and _is(out_off, _I32, B) and _is(out_len, _I32, B) and
            _is(out, _F32, least=n_out, opt=True)):
        _refuse("stoi_resample")
    K = taps.shape[0]
    if out is None:
        out = torch.empty(max(n_out, 1), device=sig.device, dtype=torch.float32)
    _call("stoi", L.sfm_stoi_resample, (_p(sig), _p(taps), _p(in_off), _p(in_len), _p(out_off), _p(out_len), _p(out), B, int(max_out_len),
                                        int(up), int(down), K, int(padl), _stream()),
          2.0 * K * n_out, 4.0 * (n_in + n_out) + 4.0 * K * up + 16.0 * B, "resample %d/%d B%d out%d" % (up, down, B, n_out))
    return out


def stoi_keep(sig, win, sig_off, sig_len, frame_off, B, sum_frames, n_samples):
    """silent-frame decision of the clean signals at 10 kHz: sig fp32 (flat), utterance u = sig[sig_off[u] : sig_off[u] + sig_len[u]],
    its frames = rows [frame_off[u], frame_off[u + 1]) -> (src int32 [sum_frames] the kept source frames of each utterance in
    order, kept int32 [B] their counts, energy fp64 [sum_frames] in dB).  sum_frames, n_samples: host sums (sizes and the cost)."""
    _need_dev(sig, win, sig_off, sig_len, frame_off)
    L = _lib.load()
    if not (_is(sig, _F32) and
            _is(win, _F32, STOI_FRAME, contig=False) and
            _is(sig_off, _I32, B) and _is(sig_len, _I32, B) and
            _is(frame_off, _I32, B + 1)):
        _refuse("stoi_keep")
    energy = torch.empty(max(sum_frames, 1), device=sig.device, dtype=torch.float64)
    src = torch.empty(max(sum_frames, 1), device=sig.device, dtype=torch.int32)
    kept = torch.empty(B, device=sig.device, dtype=torch.int32)
    _call("stoi", L.sfm_stoi_keep, (_p(sig), _p(win), _p(sig_off), _p(sig_len), _p(frame_off), _p(energy), _p(src), _p(kept), B,
                                    _stream()),
          3.0 * STOI_FRAME * sum_frames, 4.0 * n_samples + 12.0 * sum_frames + 16.0 * B + 4.0 * STOI_FRAME, "keep B%d frames%d" % (B, sum_frames))
    return src, kept, energy


def stoi_bands(sigs, win, dft, sig_off, frame_off, src, kept, tiles, sum_frames, spec_rows, n_samples):
    """one-third-octave band rows of one or two signals that share a kept list: sigs = (sig,) or (sig0, sig1) -> a tuple of fp32
    [sum_frames, 15] (rows beyond an utterance's K - 1 are not written).  tiles int32 [n, 2] on the device; spec_rows: the most
    spectral frames there can be (all frames kept), n_samples: samples of ONE signal (the cost)."""
    _need_dev(win, dft, sig_off, frame_off, src, kept, tiles, *sigs)
    L = _lib.load()
    nsig = len(sigs)
    if not (nsig in (1, 2) and _each(_F32, None, *sigs) and
            _is(win, None, STOI_FRAME, contig=False) and
            _is(dft, _F32, (STOI_FRAME, STOI_DFT_COLS)) and
            _each(_I32, None, sig_off, frame_off, kept) and
            _is(src, _I32, least=sum_frames) and
            _is(tiles, _I32, ndim=2) and tiles.shape[1] == 2):
        _refuse("stoi_bands")
    outs = tuple(torch.empty(max(sum_frames, 1), STOI_BANDS, device=sigs[0].device, dtype=torch.float32) for _ in sigs)
    n_tiles = tiles.shape[0]
    _call("stoi", L.sfm_stoi_bands, (_p(sigs[0]), _p(sigs[1]) if nsig == 2 else None, _p(win), _p(dft), _p(sig_off), _p(frame_off),
                                     _p(src), _p(kept), _p(tiles), _p(outs[0]), _p(outs[1]) if nsig == 2 else None, n_tiles, nsig,
                                     _stream()),
          nsig * 2.0 * spec_rows * STOI_FRAME * 2 * STOI_NBIN,
          nsig * (4.0 * n_samples + 4.0 * STOI_BANDS * spec_rows) + 4.0 * STOI_FRAME * (2 * STOI_NBIN + 1) + 4.0 * sum_frames + 8.0 * n_tiles,
          "bands x%d rows%d" % (nsig, spec_rows))
    return outs


def stoi_segments(xb, yb, frame_off, kept, B, extended, spec_rows, segments):
    """band rows of the clean and the enhanced signals -> score fp64 [B]: STOI, or ESTOI when extended; 1e-5 below 30 spectral
    frames.  spec_rows as stoi_bands, segments: the most segments there can be (the cost: every row read once, 12 flops per
    element of a 15 x 30 segment)."""
    _need_dev(xb, yb, frame_off, kept)
    L = _lib.load()
    if not (_is(xb, _F32, (None, STOI_BANDS)) and
            _is(yb, _F32, tuple(xb.shape)) and
            _is(frame_off, _I32, B + 1) and
            _is(kept, _I32, B)):
        _refuse("stoi_segments")
    score = torch.empty(B, device=xb.device, dtype=torch.float64)
    _call("stoi", L.sfm_stoi_segments, (_p(xb), _p(yb), _p(frame_off), _p(kept), _p(score), B, 1 if extended else 0, _stream()),
          12.0 * STOI_SEG * STOI_BANDS * segments, 8.0 * STOI_BANDS * spec_rows + 8.0 * B + 4.0 * (2 * B + 1),
          "%s B%d rows%d" % ("estoi" if extended else "stoi", B, spec_rows))
    return score


STOI_PLANES = _K["STOI_PLANES"]                # P | Q | R of sfm_stoi_bands_pair


def stoi_bands_pair(ya, yb, win, dft, sig_off, frame_off, src, kept, tiles, sum_frames, spec_rows, n_samples):
    """the band energies of ya + x yb as a quadratic in x: ya, yb fp32 (flat, at 10 kHz, laid out as stoi_bands' signals) that share
    the clean signal's kept list -> planes fp64 [sum_frames, 3, 15], row m = P | Q | R with E(x) = P + 2 x Q + x^2 R (rows beyond an
    utterance's K - 1 are not written).  One DFT operand read serves both signals; spec_rows, n_samples as stoi_bands (the cost)."""
    _need_dev(ya, yb, win, dft, sig_off, frame_off, src, kept, tiles)
    L = _lib.load()
    if not (_is(ya, _F32, ndim=1) and
            _is(yb, _F32, (ya.numel(),)) and
            _is(win, _F32, STOI_FRAME, contig=False) and
            _is(dft, _F32, (STOI_FRAME, STOI_DFT_COLS)) and
            _each(_I32, None, sig_off, frame_off, kept) and
            _is(src, _I32, least=sum_frames) and
            _is(tiles, _I32, ndim=2) and tiles.shape[1] == 2):
        _refuse("stoi_bands_pair")
    planes = torch.empty(max(sum_frames, 1), STOI_PLANES, STOI_BANDS, device=ya.device, dtype=torch.float64)
    n_tiles = tiles.shape[0]
    _call("stoi", L.sfm_stoi_bands_pair, (_p(ya), _p(yb), _p(win), _p(dft), _p(sig_off), _p(frame_off), _p(src), _p(kept), _p(tiles),
                                          _p(planes), n_tiles, _stream()),
          2 * 2.0 * spec_rows * STOI_FRAME * 2 * STOI_NBIN + 3.0 * spec_rows * 2 * STOI_NBIN,
          2 * 4.0 * n_samples + 8.0 * STOI_PLANES * STOI_BANDS * spec_rows + 4.0 * STOI_FRAME * (2 * STOI_NBIN + 1) + 4.0 * sum_frames +
          8.0 * n_tiles, "bands pair rows%d" % spec_rows)
    return planes


def pso_fitness_taal(xb, planes, frame_off, kept, pos, stopped, fitness, extended, spec_rows, segments):
    """the Taal measure of every particle of every swarm that has not stopped: xb fp32 [sum_frames, 15] the clean band rows
    (stoi_bands), planes fp64 [sum_frames, 3, 15] (stoi_bands_pair), pos [B, N] fp64, stopped int32 [B] -> fitness [B, N] fp64
    (written in place, returned): STOI, or ESTOI when extended; 1e-5 below 30 spectral frames.  The cost: per particle the
    quadratic and a square root per row element (6 flops) and stoi_segments' 12 flops per element of a 15 x 30 segment; the rows
    are counted once (every particle of an utterance reads the same ones)."""
    _need_dev(xb, planes, frame_off, kept, pos, stopped, fitness)
    L = _lib.load()
    if not (_is(xb, _F32, (None, STOI_BANDS), rows=1) and
            _is(planes, _F64, (xb.shape[0], STOI_PLANES, STOI_BANDS)) and
            _is(pos, _F64, ndim=2, rows=1) and 1 <= pos.shape[1] <= PSO_MAX_PARTICLES and
            _is(frame_off, _I32, pos.shape[0] + 1) and
            _is(kept, _I32, pos.shape[0]) and
            _is(stopped, _I32, pos.shape[0]) and
            _is(fitness, _F64, tuple(pos.shape))):
        _refuse("pso_fitness_taal")
    B, N = pos.shape
    _call("pso_fitness", L.sfm_pso_fitness_taal, (_p(xb), _p(planes), _p(frame_off), _p(kept), _p(pos), _p(stopped), _p(fitness), B, N,
                                                  1 if extended else 0, _stream()),
          N * (12.0 * STOI_SEG * STOI_BANDS * segments + 6.0 * STOI_BANDS * spec_rows),
          (4.0 + 8.0 * STOI_PLANES) * STOI_BANDS * spec_rows + 16.0 * B * N + 4.0 * (3 * B + 1),
          "%s B%d N%d rows%d" % ("estoi" if extended else "stoi", B, N, spec_rows))
    return fitness


def stoi_segments_bwd(xb, yb, frame_off, kept, gscore, B, max_rows, extended, spec_rows, segments):
    """the cotangent of the enhanced band rows: gscore fp64 [B] (the cotangent of stoi_segments' score) -> dyb fp32 like yb, EVERY
    row written (zeros from K - 1 on and below 30 spectral frames).  max_rows: the most frames of one utterance (the grid: one
    workgroup per STOI_BWD_ROWS rows).  The cost: the forward's terms again and their derivatives, 30 flops per element of a
    15 x 30 segment, each segment once (a workgroup recomputes the up to 29 that reach into its rows); both row sets read once,
    one written."""
    _need_dev(xb, yb, frame_off, kept, gscore)
    L = _lib.load()
    if not (_is(xb, _F32, (None, STOI_BANDS)) and 0 <= max_rows <= xb.shape[0] and
            _is(yb, _F32, tuple(xb.shape)) and
            _is(frame_off, _I32, B + 1) and
            _is(kept, _I32, B) and
            _is(gscore, _F64, B)):
        _refuse("stoi_segments_bwd")
    dyb = torch.empty_like(yb)
    _call("stoi", L.sfm_stoi_segments_bwd, (_p(xb), _p(yb), _p(frame_off), _p(kept), _p(gscore), _p(dyb), B, int(max_rows),
                                            1 if extended else 0, _stream()),
          30.0 * STOI_SEG * STOI_BANDS * segments, 12.0 * STOI_BANDS * spec_rows + 8.0 * B + 4.0 * (2 * B + 1),
          "%s bwd B%d rows%d" % ("estoi" if extended else "stoi", B, spec_rows))
    return dyb


def stoi_bands_bwd(sig, win, dft, dft_t, sig_off, frame_off, src, kept, tiles, dyb, sum_frames, spec_rows, n_samples):
    """dyb (stoi_segments_bwd) -> dframes fp32 [sum_frames, 256]: row frame_off[u] + m = the cotangent of the rebuilt enhanced
    signal's samples [128 m, 128 m + 256) through spectral frame m.  sig: the resampled enhanced signal; dft_t [432, 256] the
    transpose of dft.  Only the rows stoi_fold_bwd reads are written.  The cost: the forward's product and the adjoint one."""
    _need_dev(sig, win, dft, dft_t, sig_off, frame_off, src, kept, tiles, dyb)
    L = _lib.load()
    if not (_is(sig, _F32) and
            _is(win, _F32, STOI_FRAME, contig=False) and
            _is(dft, _F32, (STOI_FRAME, STOI_DFT_COLS)) and
            _is(dft_t, _F32, (STOI_DFT_COLS, STOI_FRAME)) and
            _each(_I32, None, sig_off, frame_off, kept) and
            _is(src, _I32, least=sum_frames) and
            _is(tiles, _I32, ndim=2) and tiles.shape[1] == 2 and
            _is(dyb, _F32, (None, STOI_BANDS), rows=sum_frames)):
        _refuse("stoi_bands_bwd")
    dframes = torch.empty(max(sum_frames, 1), STOI_FRAME, device=sig.device, dtype=torch.float32)
    n_tiles = tiles.shape[0]
    _call("stoi", L.sfm_stoi_bands_bwd, (_p(sig), _p(win), _p(dft), _p(dft_t), _p(sig_off), _p(frame_off), _p(src), _p(kept), _p(tiles),
                                         _p(dyb), _p(dframes), n_tiles, _stream()),
          2.0 * spec_rows * STOI_FRAME * (2 * STOI_NBIN + STOI_DFT_COLS),
          4.0 * n_samples + 4.0 * (STOI_BANDS + STOI_FRAME) * spec_rows + 4.0 * STOI_FRAME * (2 * STOI_NBIN + STOI_DFT_COLS + 1) +
          4.0 * sum_frames + 8.0 * n_tiles, "bands bwd rows%d" % spec_rows)
    return dframes


def stoi_fold_bwd(dframes, win, sig_off, sig_len, frame_off, src, kept, B, n_out, max_len, pad_to, sum_frames):
    """the overlap-add adjoint: dframes (stoi_bands_bwd) -> dsig fp32 [n_out], utterance u's 10 kHz samples at sig_off[u], every
    one written once (and zeros up to pad_to behind sig_len[u]: the rows of a zero-padded 10 kHz batch).  max_len: the largest
    of sig_len and pad_to (host figures)."""
    _need_dev(dframes, win, sig_off, sig_len, frame_off, src, kept)
    L = _lib.load()
    if not (_is(dframes, _F32, (None, STOI_FRAME), rows=sum_frames) and
            _is(win, _F32, STOI_FRAME, contig=False) and
            _is(sig_off, _I32, B) and _is(sig_len, _I32, B) and
            _is(frame_off, _I32, B + 1) and
            _is(src, _I32, least=sum_frames) and
            _is(kept, _I32, B) and
            0 <= pad_to <= max_len):
        _refuse("stoi_fold_bwd")
    dsig = torch.empty(max(n_out, 1), device=dframes.device, dtype=torch.float32)
    _call("stoi", L.sfm_stoi_fold_bwd, (_p(dframes), _p(win), _p(sig_off), _p(sig_len), _p(frame_off), _p(src), _p(kept), _p(dsig), B,
                                        int(max_len), int(pad_to), _stream()),
          8.0 * n_out, 4.0 * n_out + 4.0 * STOI_FRAME * sum_frames + 4.0 * sum_frames + 20.0 * B + 4.0 * STOI_FRAME,
          "fold bwd B%d out%d" % (B, n_out))
    return dsig
