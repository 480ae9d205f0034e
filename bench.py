#!/usr/bin/env python3
"""Benchmark of the hot path on MI355X (contract: see the round prompt / DESIGN.md section 7).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3p|c2|c1|c5|c3se|c2t|c3t] [--dtype mixed|bf16|f16]
                    [--streams S] [--full] [--dump-outputs DIR]

A step = one forward pass of the north-star path (PerceptionAgent -> pool -> CPEA -> STFT -> MaskSynthesisAgent ->
apply_mask -> iSTFT) over one batch of synthetic 16 kHz utterances that is already resident in HBM.  Default workload = the
shape BASELINE.json's metric is quoted on ("512-frame utts", target shape "batch 256 x 512-frame utterances"): c3p = batch
256 x 512 STFT frames (L = 40 880), forward, 16-bit MFMA operands (default policy "mixed": fp16 GEMM operands, bf16
attention core) with fp32 accumulation.  value = STFT frames/s over all ranks (utterances shard over ranks: no data-path
collective).

A plain run does only what that figure needs: set-up, warm-up (with the calibration of the passes in flight), the K timed steps,
the outputs of the last step if --dump-outputs DIR is given, the result line.  --dump-outputs writes what the last timed step
returned (forward: every array of the path's output dict; training: the loss and the trained flat fp32 parameters) as
DIR/<name>.npy in float32 (float64 for float64 and integer results), at most 64 MB in all: an array larger than its share is
replaced by a fixed seeded sample of its flattened elements.  Inputs and weights are seeded, so two builds run with the same
arguments can be compared output for output.

Everything else is measured only with --full: the instrumented pass (`breakdown_ms_per_step`, the dominant family and its
`roofline`, event-timed per launch inside the timed region), three sequential passes (`single_pass_ms_per_step`,
`roofline.exclusive_*`), the `attention` figure inside the pass, and for the default N = 1 line the sub-records measured after
the timed region:
  `configs1`  BASELINE configs[1] (B 64 x 4 s, T 801) through the same path: ms per step, frames/s, dominant kernel + roofline,
              the attention kernel inside that pass
  `train`     BASELINE configs[2] on the north-star composition (c3t: B 256 x 4 s, forward + objective + backward through
              every module + clip + AdamW, fp16 operands under the device-side dynamic loss scale): ms per step, frames/s,
              dominant family + roofline, final loss, skipped steps (0 in the timed steps)
  `headline`  the attention kernel ALONE at B 256 x T 512 x 4 heads x 64, bf16 (north_star's >= 30 % of bf16 MFMA peak)
  `sustained`, `mask_rmse`, `cpu_baseline` (the oracle on the host cores, bounded sample, N = 1 only).
With --gpus N > 1 the default --full line carries `dp_train` instead of `train`; the training workloads' --full lines carry the
roofline, the per-family breakdown and `cpu_baseline`.

Launching: `python bench.py --gpus N` with no torchrun environment starts the N ranks itself (child processes, before this
process touches the GPU); under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` the ranks are the
launcher's.  A --gpus that disagrees with WORLD_SIZE is an error.

`roofline`: the dominant kernel family, HIP-event timed per launch inside the timed region.  The roof is chosen PER LAUNCH
from its arithmetic intensity (algorithmic FLOPs / algorithmic bytes against the ridge of the pipe it runs on): a K = 256
linear of the GEMM family is HBM-bound, a K = 1024 one MFMA-bound; the family's `bound` is the class that takes most of its
time and achieved / peak / frac are over the launches of that class (`roofline_time_frac` covers all of them).
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (batch per GPU, samples, description)
    "c1": (1, 16000, "B1 x 1 s (L16000, T201) forward"),
    "c2": (64, 64000, "B64 x 4 s (L64000, T801) SincNet+Conformer forward (BASELINE configs[1])"),
    "c3p": (256, 40880, "B256 x 512-frame utterances (L40880, T512) forward"),
    "c3se": (256, 64000, "B256 x 4 s (L64000, T801) SpeechEnhancer training step: STFT, forward, SI-SNR + L1 + multi-res "
                         "STFT objective, backward, gradient all-reduce, clip, AdamW (BASELINE configs[2]/[3])"),
    "c2t": (64, 64000, "B64 x 4 s (L64000, T801) SincNet+Conformer path (PerceptionAgent, CPEA, MaskSynthesisAgent) training "
                       "step: forward, SI-SNR + L1 + multi-res STFT objective, backward through every module, all-reduce, "
                       "clip, AdamW"),
    "c3t": (256, 64000, "B256 x 4 s (L64000, T801) SincNet+Conformer path (PerceptionAgent, CPEA, MaskSynthesisAgent) training "
                        "step: forward, SI-SNR + L1 + multi-res STFT objective, backward through every module, all-reduce, "
                        "clip, AdamW (BASELINE configs[2]/[3] on the north-star composition)"),
    "c5": (32, 480000, "B32 x 30 s (L480000, T6001) forward with episodic memory (BASELINE configs[4], fwd)"),
}
TRAIN_WORKLOADS = ("c3se", "c2t", "c3t")
PEAKS = {"mfma16": 2500.0, "mfma32": 157.3, "valu32": 157.3, "hbm": 8000.0}   # TFLOP/s x3, GB/s (MI355X_MICROARCH.md)
# the pipe a family's FLOPs run on (everything else: fp32 vector ALU); WHICH roof binds a launch - that pipe or HBM - is
# decided per launch from its arithmetic intensity (roofline_of), not per family
FAMILY_PIPE = {"gemm16": "mfma16", "attention_fwd": "mfma16", "framed_gemm_f32": "mfma32", "gemm16_tn": "mfma16",
               "attention_bwd": "mfma16", "conv16": "mfma16", "conv16p": "mfma16", "ffn_fused": "mfma16", "sinc_fir16": "mfma16",
               "framed_gemm_split16": "mfma16", "conv_dgrad16": "mfma16", "conv_wgrad16": "mfma16"}
METRIC = "audio frames/sec/GPU (16 kHz, 512-frame utts) + mask RMSE vs CPU ref"
DTYPE_DESC = {
    "mixed": "fp16 MFMA operands (PerceptionAgent, fusion, Conformer GEMMs, heads) + bf16 attention core, fp32 accumulate "
             "(ops.POLICIES['mixed'])",
    "bf16": "bf16", "f16": "fp16",
    "amp16": "fp16 MFMA operands, fp32 accumulate, dynamic loss scale on the device (optim.DynamicLossScale = the reference's "
             "fp16 autocast + GradScaler recipe, training/conformer_pipeline.py:442,504,512-517)",
}


def set_precision(dtype):
    from sincformer_metacog_speech_enhancement_amd import ops
    if dtype == "mixed":
        ops.reset_precision()
    else:
        ops.set_compute_dtype(dtype)


def build_path(dtype, seed=1234, use_memory=False):
    import torch
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import EnhancementPath
    set_precision(dtype)
    path = EnhancementPath(sample_rate=16000, use_memory=use_memory)
    sd = path.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    keep = {k: v.numpy() for k, v in sd.items() if k.split(".")[-1] in ("low_hz_", "band_hz_", "window", "n_")}
    new = syn.synth_state_dict(shapes, seed, keep=keep, sinc_scale=2000.0)
    path.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
    return path, new


def host_cores():
    """threads this process may really use: affinity mask, cgroup cpu quota, capped at the
    16-core share a 1-GPU box gets (oversubscribing a quota makes the CPU leg crawl)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per) + 0.5)))
    except Exception:
        pass
    return max(1, min(n, 16))


def cpu_baseline(weights, L, wave_np, gpu_masks=None, batch=None, iters=4, use_memory=False):
    """Oracle (CPU restatement, kind 'port') timed on the host cores on a bounded sample (about 10-25 s of CPU work):
    the first `batch` utterances of the bench batch `wave_np` (numpy [B, L]).  gpu_masks: (mask_real, mask_imag) the HIP path produced for utterance 0 of the same synthetic batch -> the oracle's
    output for that utterance doubles as the parity check of the line (`mask_rmse`)."""
    batch = batch or max(1, min(8, 512000 // L))
    import torch
    from oracle import sfm_oracle as orc
    cores = host_cores()
    torch.set_num_threads(cores)

    def subd(prefix):
        p = prefix + "."
        return {k[len(p):]: torch.from_numpy(v) for k, v in weights.items() if k.startswith(p)}
    sds = {"pa": subd("perception"), "cpea": subd("cpea"), "msa": subd("msa")}
    if use_memory:
        sds["memory"] = subd("memory")
    batch = min(batch, wave_np.shape[0])
    noisy = wave_np[:batch]
    ref = orc.enhance_path(sds, noisy, 16000, use_memory=use_memory)           # warm-up (and the parity reference)
    rm = None
    if gpu_masks is not None:
        got = torch.cat([gpu_masks[0], gpu_masks[1]], -1).double()
        want = torch.cat([ref["mask_real"][:1], ref["mask_imag"][:1]], -1).double()
        rm = float(((got - want) ** 2).mean().sqrt())
    t0 = time.perf_counter()
    for _ in range(iters):
        orc.enhance_path(sds, noisy, 16000, use_memory=use_memory)
    dt = (time.perf_counter() - t0) / iters
    T = 1 + L // 80
    base = {"value": batch * T / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "oracle enhance_path, batch %d x L%d, %d iterations after 1 warm-up, fp32, torch %d threads"
                      % (batch, L, iters, cores)}
    return base, rm


def cpu_baseline_train(sd, L, iters=8, batch=8):
    """oracle forward + backward (torch autograd on the host cores) of the same training step, small batch."""
    import torch
    from oracle import sfm_oracle as orc
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    cores = host_cores()
    torch.set_num_threads(cores)
    noisy, clean = syn.synth_wave(batch, L, 77)
    noisy, clean = torch.from_numpy(noisy), torch.from_numpy(clean)
    ref = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
           for k, v in sd.items()}
    t0 = time.perf_counter()
    for i in range(iters):
        print("[bench] cpu baseline (training) iter %d/%d" % (i + 1, iters), file=sys.stderr, flush=True)
        total, _, _ = orc.enhancer_loss(ref, noisy, clean, 4, bn_train=True)
        total.backward()
    dt = (time.perf_counter() - t0) / iters
    T = 1 + L // 80
    return {"value": batch * T / dt, "unit": "STFT frames/s", "cores": cores, "kind": "port",
            "sample": "oracle (torch fp32 autograd restatement) forward+backward of the same step, batch %d x %d samples, %d "
                      "iterations, %.1f s each; no optimiser step" % (batch, L, iters, dt)}


def cpu_baseline_path_train(weights, L, iters=3, batch=4):
    """oracle forward + backward of the whole-path training step (torch autograd on the host cores), small batch."""
    import torch
    from oracle import sfm_oracle as orc
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    cores = host_cores()
    torch.set_num_threads(cores)
    noisy, clean = syn.synth_wave(batch, L, 77)
    noisy, clean = torch.from_numpy(noisy), torch.from_numpy(clean)

    def subd(prefix):
        p = prefix + "."
        out = {}
        for k, v in weights.items():
            if k.startswith(p):
                v = torch.from_numpy(v) if not torch.is_tensor(v) else v
                leaf = v.dtype.is_floating_point and "running" not in k and k.split(".")[-1] not in ("window", "n_")
                out[k[len(p):]] = v.clone().requires_grad_(True) if leaf else v.clone()
        return out
    sds = {"pa": subd("perception"), "cpea": subd("cpea"), "msa": subd("msa")}
    t0 = time.perf_counter()
    for i in range(iters):
        print("[bench] cpu baseline (path training) iter %d/%d" % (i + 1, iters), file=sys.stderr, flush=True)
        total, _, _ = orc.path_loss(sds, noisy, clean, 16000, bn_train=True)
        total.backward()
    dt = (time.perf_counter() - t0) / iters
    T = 1 + L // 80
    return {"value": batch * T / dt, "unit": "STFT frames/s", "cores": cores, "kind": "port",
            "sample": "oracle (torch fp32 autograd restatement) forward+backward of the same step, batch %d x %d samples, %d "
                      "iterations, %.1f s each; no optimiser step" % (batch, L, iters, dt)}


# ---------------------------------------------------------------------------------------------------------------
# --dump-outputs: what the last timed step returned
# ---------------------------------------------------------------------------------------------------------------
DUMP_BUDGET = 60 << 20                  # bytes of .npy payload in all (under 64 MB with the headers)


def collect_outputs(named, budget=DUMP_BUDGET):
    """{name: tensor} -> {name: numpy array}: floating results in float32 (float64 stays float64), integer / bool results in
    float64.  Arrays are taken smallest first; one that fits in its even share of what is left of the budget is kept whole with
    its shape, a larger one becomes a 1-D sample of its flattened elements at sorted indices drawn from a generator seeded by
    its name (the same positions in every run and every build for the same shapes).  Reads device tensors: call it after the
    device has finished the step."""
    import zlib
    import numpy as np
    import torch
    items = sorted(((k, v.detach()) for k, v in named.items() if torch.is_tensor(v)), key=lambda kv: (kv[1].numel(), kv[0]))
    out, left = {}, budget
    for i, (k, v) in enumerate(items):
        dt = torch.float32 if v.is_floating_point() and v.dtype != torch.float64 else torch.float64
        share = left // (len(items) - i) // (4 if dt == torch.float32 else 8)
        if v.numel() <= share:
            a = v.to(dt).cpu().numpy()
        else:
            idx = np.unique(np.random.default_rng(zlib.crc32(k.encode())).integers(0, v.numel(), share))
            a = v.reshape(-1)[torch.from_numpy(idx).to(v.device)].to(dt).cpu().numpy()
        out[k] = a
        left -= a.nbytes
    return out


def write_outputs(dirname, arrays):
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    print("[bench] outputs of the last timed step -> %s: %s" % (dirname, ", ".join("%s %s %s" % (k, a.dtype, a.shape)
                                                                              for k, a in sorted(arrays.items()))),
          file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------------------------------------------
# launching
# ---------------------------------------------------------------------------------------------------------------
def spawn_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start N ranks as child processes (this process has not touched the
    GPU and never will), pass rank 0's line through, exit with the worst return code."""
    n = args.gpus
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "SFM_BENCH_CHILD": "1"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=(None if r == 0 else subprocess.DEVNULL)))
    rc = 0
    for p_ in procs:
        rc = max(rc, abs(p_.wait()))
    return rc


def init_ranks(args):
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    torch.cuda.set_device(0 if os.environ.get("SFM_SINGLE_DEVICE") else local_rank)   # rehearsal of N ranks on a 1-GPU box
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("SFM_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    return rank, world


def roofline_of(family, launches, traffic_src=None):
    """launches: [(ms, algorithmic flops, algorithmic bytes)] of one kernel family, HIP-event timed.  The roof is chosen per
    LAUNCH: t_mfma = flops / peak of the pipe the family's arithmetic runs on, t_hbm = bytes / 8 TB/s, the larger one binds
    (= arithmetic intensity against the ridge).  `bound` = the class whose launches take most of the family's time;
    achieved / peak / frac / launches / avg_ms are over the launches of THAT class; `roofline_time_frac` = sum of the per-launch
    roofline times over the sum of the measured times, all launches."""
    pipe = FAMILY_PIPE.get(family, "valu32")
    cls = {"hbm": [], "mfma": []}
    t_roof = 0.0
    for ms, fl, by in launches:
        tf, tb = fl / (PEAKS[pipe] * 1e12), by / (PEAKS["hbm"] * 1e9)
        k = "mfma" if (pipe != "valu32" and tf > tb) else "hbm"
        cls[k].append((ms, fl, by))
        t_roof += max(tf, tb) if pipe != "valu32" else tb
    total_ms = sum(l[0] for l in launches)
    bound = max(cls, key=lambda k: sum(l[0] for l in cls[k]))
    sel = cls[bound]
    secs = sum(l[0] for l in sel) * 1e-3
    if bound == "hbm":
        ach, peak, unit = sum(l[2] for l in sel) / secs / 1e9, PEAKS["hbm"], "GB/s"
    else:
        ach, peak, unit = sum(l[1] for l in sel) / secs / 1e12, PEAKS[pipe], "TFLOP/s"
    n = len(sel)
    r = {"bound": bound, "kernel": family, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak, "traffic": None,
         "algorithmic_bytes_per_launch": sum(l[2] for l in sel) / n, "algorithmic_flops_per_launch": sum(l[1] for l in sel) / n,
         "launches": n, "avg_ms": secs * 1e3 / n,
         "roof_choice": "per launch: max(flops / %s peak, bytes / HBM peak)" % pipe,
         "roofline_time_frac": t_roof * 1e3 / total_ms if total_ms > 0 else None, "family_launches": len(launches),
         "family_ms": total_ms}
    other = "mfma" if bound == "hbm" else "hbm"
    if cls[other]:
        o = cls[other]
        osec = sum(l[0] for l in o) * 1e-3
        if other == "hbm":
            oa, op, ou = sum(l[2] for l in o) / osec / 1e9, PEAKS["hbm"], "GB/s"
        else:
            oa, op, ou = sum(l[1] for l in o) / osec / 1e12, PEAKS[pipe], "TFLOP/s"
        r["other_bound"] = {"bound": other, "launches": len(o), "ms": osec * 1e3, "achieved": oa, "peak": op, "unit": ou, "frac": oa / op}
    if traffic_src and os.path.exists(os.path.join(ROOT, traffic_src)):
        t = json.load(open(os.path.join(ROOT, traffic_src))).get(family, {}).get("hbm_bytes_per_launch")
        if t is not None:
            r.update({"traffic": t, "traffic_unit": "HBM bytes/launch",
                      "traffic_source": "NOT measured in this run: read from %s = committed rocprofv3 --pmc FETCH_SIZE / "
                                        "WRITE_SIZE passes of this command (FETCH_SIZE doubled per the gfx950 note)" % traffic_src})
    return r


def refuse_variant_overrides():
    """the kernel-selection knobs (ops.set_gemm_variant / set_attention_variant / SFM_GEMM_VARIANT) are A/B test tools: nothing
    is timed while one is away from its default"""
    from sincformer_metacog_speech_enhancement_amd import ops
    ov = ops.variant_overrides()
    if ov:
        raise SystemExit("bench.py: kernel variant override active %r - refusing to time anything" % (ov,))


def traffic_file(workload):
    rounds = sorted((d for d in os.listdir(os.path.join(ROOT, "profiles")) if d.startswith("r") and d[1:].isdigit()), reverse=True)
    for d in ["profiles/" + r for r in rounds] + ["profiles"]:                   # the newest round that measured this workload
        p = "%s/pmc_traffic_%s.json" % (d, workload)
        if os.path.exists(os.path.join(ROOT, p)):
            return p
    return None


# ---------------------------------------------------------------------------------------------------------------
# training workloads
# ---------------------------------------------------------------------------------------------------------------
def train_dtype(args):
    """operand recipe of the training workloads: the default ("mixed") is the reference's AMP recipe - fp16 operands (ops'
    default training format) under the device-side dynamic loss scale; --dtype bf16 / f16 force one format WITHOUT a loss scale
    (diagnostics)."""
    return "amp16" if args.dtype == "mixed" else args.dtype


def build_train_step(workload, dtype, rank, batch=0):
    """model + flat optimiser (+ gradient synchroniser over the default process group) + synthetic shard of one training
    workload; returns (step, opt, scaler, sd, B, L, T, desc, whole_path)."""
    import torch
    from sincformer_metacog_speech_enhancement_amd import ops, synthetic as syn
    from sincformer_metacog_speech_enhancement_amd.optim import FlatAdamW, DynamicLossScale
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import SpeechEnhancer, batch_stft, compute_loss
    if dtype == "amp16":
        ops.reset_precision()                                       # base (training) format fp16
        scaler = DynamicLossScale("cuda")                           # GradScaler defaults: S = 65536, x0.5 / x2 every 2000
    else:
        ops.set_compute_dtype(dtype)
        scaler = None
    B, L, desc = WORKLOADS[workload]
    if batch:
        B = batch
    T = 1 + L // 80
    whole_path = workload in ("c2t", "c3t")
    if whole_path:
        from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import compute_path_loss
        model, sd = build_path("mixed" if dtype == "amp16" else dtype, seed=4321)
    else:
        model = SpeechEnhancer(n_freq=129, d_model=256, num_blocks=4, num_heads=4, d_ff=1024, kernel_size=31, dropout=0.15)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, 4321).items()}
        model.load_state_dict(sd)                                   # same weights on every rank
    model.cuda().train()
    # the objective's graph does not reach the uncertainty head (sigma feeds no loss on the path): like torch.optim.AdamW,
    # which skips parameters whose grad is None, the flat optimiser is built from the parameters that are trained
    params = [p_ for n_, p_ in model.named_parameters() if "uncertainty_head" not in n_]
    opt = FlatAdamW(params, lr=5e-4, betas=(0.9, 0.98), weight_decay=0.01, max_norm=5.0)
    noisy, clean = syn.synth_wave(B, L, 1234 + rank)                # each rank trains on its own utterance shard
    noisy, clean = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    torch.manual_seed(1000 + rank)                                  # dropout seeds

    def step():
        # training/conformer_pipeline.py:496-532 in its call order; no host synchronisation anywhere in it
        opt.zero_grad()
        if whole_path:
            total, _ = compute_path_loss(model, noisy, clean)
        else:
            nr, ni = batch_stft(noisy, 256, 80, 160)
            cr, ci = batch_stft(clean, 256, 80, 160)
            total, _ = compute_loss(model, nr, ni, clean, cr, ci)
        if scaler is not None:
            scaler.scale(total).backward()
            scaler.unscale_(opt)
            scaler.step(opt, loss=total)
            scaler.update()
        else:
            total.backward()
            opt.step(loss=total)
        return total

    return step, opt, scaler, sd, B, L, T, desc, whole_path


def settle_loss_scale(step, opt, scaler, min_steps, barrier=None):
    """warm-up of a training workload: at least `min_steps` steps, and on until the dynamic loss scale has settled (the last two
    steps were applied, not skipped: GradScaler starts at 65536 and halves on every overflow), so that every step of the timed
    region is a full step.  The decision is taken from rank-consistent state (the skip flag is computed from the all-reduced
    gradients).  Returns the number of warm-up steps run."""
    n, clean = 0, 0
    while n < min_steps or (scaler is not None and clean < 2):
        step()
        n += 1
        if scaler is not None:
            clean = 0 if opt.stats()["skipped"] else clean + 1
        if n >= min_steps + 40:
            raise SystemExit("bench.py: the loss scale did not settle within %d steps: %r" % (n, scaler.stats()))
    return n


def train_leg(args, workload, rank, world, steps, warmup, batch=0, profile=True, keep_outputs=False):
    """warm-up (incl. settling the loss scale), one instrumented step alone on the device (per-family breakdown; profile only),
    then `steps` timed steps between barriers (profile: with the dominant family event-timed per launch).  keep_outputs: the
    record's `outputs` = collect_outputs of the last timed step's loss and the trained flat fp32 parameters.  Every rank calls
    it; returns a dict."""
    import torch
    import torch.distributed as dist
    from sincformer_metacog_speech_enhancement_amd import ops
    dtype = train_dtype(args)
    step, opt, scaler, sd, B, L, T, desc, whole_path = build_train_step(workload, dtype, rank, batch=batch)
    opt.sync.time_exposed = world > 1

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if rank == 0:
        print("[bench] %s, dtype %s, world %d, batch/GPU %d" % (desc, dtype, world, B), file=sys.stderr, flush=True)
    n_warm = settle_loss_scale(step, opt, scaler, max(warmup, 1))
    breakdown, dominant, launches = {}, None, []
    if profile:
        torch.cuda.synchronize()                                    # the instrumented step runs alone on the device
        ops.profiler.enable(None)
        step()
        breakdown = ops.profiler.summary()
        ops.profiler.disable()
        dominant = max(breakdown, key=lambda k: breakdown[k]["ms_total"])
        ops.profiler.enable({dominant})
    if world > 1:
        opt.sync.exposed_ms()                                       # (drops the warm-up events; host sync)
    refuse_variant_overrides()
    skipped0 = scaler.stats() if scaler is not None else None
    step0 = opt.stats()["step"]
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if profile:
        launches = ops.profiler.launches(dominant)
        ops.profiler.disable()
    outputs = collect_outputs({"loss": loss.detach().reshape(1), "params": opt.flat_p}) if keep_outputs else None
    tmax = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax.item())
    st = opt.stats()
    rec = {"workload": desc, "batch_per_gpu": B, "samples": L, "frames_per_utt": T, "steps": steps, "warmup": n_warm,
           "elapsed": elapsed, "ms_per_step": elapsed / steps * 1e3, "frames_per_s": world * B * T * steps / elapsed,
           "dtype": DTYPE_DESC[dtype], "final_loss": float(loss.detach()), "optimizer_state": st,
           "applied_steps_in_timed_region": st["step"] - step0, "whole_path": whole_path, "sd": sd,
           "allreduce_bytes_per_step": opt.sync.bytes_per_step() if world > 1 else 0,
           "allreduce_buckets": len(opt.sync.buckets), "overlap": bool(opt.sync.overlap),
           "exposed_allreduce_ms_per_step": opt.sync.exposed_ms() if world > 1 else None,
           "breakdown": breakdown, "dominant": dominant, "launches": launches, "outputs": outputs}
    if scaler is not None:
        s1 = scaler.stats()
        rec["loss_scale"] = {"scale": s1["scale"], "init_scale": 65536.0,
                             "skipped_in_timed_region": (s1["skipped_inf"] - skipped0["skipped_inf"]) +
                                                        (s1["skipped_loss"] - skipped0["skipped_loss"]),
                             "skipped_in_warmup": skipped0["skipped_inf"] + skipped0["skipped_loss"],
                             "rule": "x0.5 after a step with Inf / NaN gradients (step skipped), x2 after 2000 clean steps; on the device"}
        if rec["loss_scale"]["skipped_in_timed_region"] != 0 or rec["applied_steps_in_timed_region"] != steps:
            raise SystemExit("bench.py: %d of the %d timed training steps were skipped - not a valid measurement: %r" %
                             (steps - rec["applied_steps_in_timed_region"], steps, rec["loss_scale"]))
    ops.reset_precision()
    return rec


def dp_train_record(args, rank, world):
    """N > 1, default workload: the data-parallel TRAINING step beside the forward shard, in the same line - the c3se step
    (training/conformer_pipeline.py:496-532: forward, objective, backward, bucketed all-reduce of the flat fp32 gradient over
    RCCL overlapped with backward, global-norm clip, AdamW under the dynamic loss scale), weak scaling.  Every rank calls this;
    rank 0 returns the record."""
    import torch.distributed as dist
    r = train_leg(args, "c3se", rank, world, args.dp_steps, args.dp_warmup, batch=args.dp_batch, profile=False)
    if rank != 0:
        return None
    rec = {k: r[k] for k in ("workload", "batch_per_gpu", "steps", "warmup", "ms_per_step", "frames_per_s", "dtype",
                             "allreduce_bytes_per_step", "allreduce_buckets", "exposed_allreduce_ms_per_step", "overlap",
                             "final_loss", "optimizer_state", "applied_steps_in_timed_region")}
    if "loss_scale" in r:
        rec["loss_scale"] = r["loss_scale"]
    rec.update({"scaling": "weak", "rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(),
                "note": "time = max over ranks between barriers; exposed = HIP events around the wait for the bucketed "
                        "all-reduce on the compute stream (the part of the exchange that did not overlap backward)"})
    return rec


def train_subrecord(r, workload):
    """the `train` object of the default N = 1 line (and the body of a --workload c3t / c3se / c2t line) from a train_leg record"""
    roof = roofline_of(r["dominant"], r["launches"], traffic_file(workload))
    rec = {k: r[k] for k in ("workload", "batch_per_gpu", "steps", "warmup", "ms_per_step", "frames_per_s", "dtype", "final_loss",
                             "optimizer_state", "applied_steps_in_timed_region")}
    if "loss_scale" in r:
        rec["loss_scale"] = r["loss_scale"]
    rec["roofline"] = roof
    rec["breakdown_ms_per_step"] = {k: round(v["ms_total"], 4) for k, v in
                                    sorted(r["breakdown"].items(), key=lambda kv: -kv[1]["ms_total"])}
    rec["breakdown_note"] = ("one instrumented step alone on the device (HIP events per launch); weight gradients run on a side "
                             "stream, so the per-family times overlap and can sum to more than the step")
    return rec


def main_train(args):
    """--workload c3se / c2t / c3t: one training step of training/conformer_pipeline.py per bench step (c3se: the reference's
    SpeechEnhancer; c2t / c3t: the north-star SincNet + Conformer composition at B 64 / B 256)."""
    import torch.distributed as dist
    rank, world = init_ranks(args)
    r = train_leg(args, args.workload, rank, world, args.steps, args.warmup, batch=args.batch, profile=args.full,
                  keep_outputs=bool(args.dump_outputs) and rank == 0)
    if rank == 0:
        line = {
            "metric": METRIC,
            "value": r["frames_per_s"], "unit": "STFT frames/s trained (whole job)", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "warmup_run": r["warmup"], "ms_per_step": r["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": r["dtype"], "data": "synthetic",
            "config": {"workload": r["workload"], "batch_per_gpu": r["batch_per_gpu"], "samples": r["samples"],
                       "frames_per_utt": r["frames_per_utt"],
                       "sharding": "utterances over ranks; one bucketed all-reduce (RCCL) of the flat fp32 gradient per step, "
                                   "overlapped with backward", "optimizer": "AdamW lr 5e-4 betas (0.9, 0.98) wd 0.01, clip 5.0",
                       "dropout": "module defaults (0.1 / 0.15)" if r["whole_path"] else 0.15},
            "frames_per_s_per_gpu": r["frames_per_s"] / world,
            "final_loss": r["final_loss"], "optimizer_state": r["optimizer_state"],
            "applied_steps_in_timed_region": r["applied_steps_in_timed_region"],
            "allreduce_bytes_per_step": r["allreduce_bytes_per_step"],
            "exposed_allreduce_ms_per_step": r["exposed_allreduce_ms_per_step"],
            "rccl_ranks": world,
        }
        if args.full:
            sub = train_subrecord(r, args.workload)
            line["roofline"] = sub["roofline"]
            line["breakdown_ms_per_step"] = sub["breakdown_ms_per_step"]
        if "loss_scale" in r:
            line["loss_scale"] = r["loss_scale"]
        print("[bench] gpu leg done: %.1f ms/step, %.3e frames/s%s" % (line["ms_per_step"], line["value"],
              "; dominant kernel %s" % r["dominant"] if r["dominant"] else ""), file=sys.stderr, flush=True)
        if r["outputs"] is not None:
            write_outputs(args.dump_outputs, r["outputs"])
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline_path_train(r["sd"], r["samples"]) if r["whole_path"] else \
                cpu_baseline_train(r["sd"], r["samples"])
        if args.breakdown:
            with open(args.breakdown, "w") as fh:
                json.dump(r["breakdown"], fh, indent=1)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------
# the headline shape of BASELINE's metric, measured after the timed region (rank 0)
# ---------------------------------------------------------------------------------------------------------------
def headline_attention():
    """the attention kernel ALONE at B 256 x T 512 x 4 heads x 64 in the attention stage's format (bf16: the north-star's >= 30 %
    of bf16 MFMA peak target), each launch timed by HIP events with nothing else on the device."""
    import torch
    from sincformer_metacog_speech_enhancement_amd import ops
    B, L, desc = WORKLOADS["c3p"]
    T = 1 + L // 80
    out = {}
    H, hd = 4, 64
    with ops.stage("attn"):
        adt = ops.compute_dtype()
        g = torch.Generator(device="cuda").manual_seed(1)
        qkv = torch.randn(B * T, 3 * H * hd, device="cuda", generator=g)
        # the call the path makes: functional.pack_mhsa folds log2(e) / sqrt(hd) into W_q, the kernel gets q pre-scaled
        # (prescaled=True; with the scale passed instead it rescales the Q fragments of every item: ~2 % at this shape)
        qkv[:, :H * hd] *= 1.4426950408889634 / math.sqrt(hd)
        qkv = qkv.to(adt)
        o = torch.empty(B * T, H * hd, device="cuda", dtype=adt)
        attn = lambda: ops.attention(qkv, B, T, H, hd, out=o, prescaled=True)
        for _ in range(3):
            attn()
        torch.cuda.synchronize()
        # pass 1: 20 launches back to back between ONE pair of HIP events -> the average launch duration of that 2 ms window; FIVE
        # such windows, and the figure is their MEDIAN: the chip's clock moves by +-7 % within seconds under this kernel (94.9 ..
        # 110.8 us for consecutive windows in one process, profiles/README.md round 3), a single window is a draw from that
        wins = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(20):
                attn()
            e1.record()
            torch.cuda.synchronize()
            wins.append(e0.elapsed_time(e1) / 20.0)
        avg = sorted(wins)[2]
        # pass 2: an event after every launch -> the spread (each interval then also holds the event's own packet)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        ev[0].record()
        for i in range(20):
            attn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        # pass 3: the same launch kept up for >= 2 s (power / thermal steady state: under this kernel the part sits at its socket
        # power limit and the shader clock settles below the boost the short windows above still see: profiles/r04/power_probe.txt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_sus, t_host = 0, time.time()
        e0.record()
        while time.time() - t_host < 2.0:
            for i in range(200):
                attn()
            n_sus += 200
            torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
        sus = e0.elapsed_time(e1) / n_sus
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(20))
    med = 0.5 * (ms[9] + ms[10])
    fl = 4.0 * B * H * T * T * hd
    out["attention"] = {"shape": "B256 x T512 x 4 heads x 64", "operands": "bf16" if adt is torch.bfloat16 else "fp16",
                        "avg_ms": sus, "tflops": fl / sus / 1e9, "frac_bf16_mfma_peak": fl / sus / 1e9 / PEAKS["mfma16"],
                        "sustained_launches": n_sus, "measure": "steady state: the launch repeated back to back for >= 2 s",
                        "window_avg_ms": [round(w, 5) for w in wins], "window_median_ms": avg,
                        "frac_windows_median": fl / avg / 1e9 / PEAKS["mfma16"], "median_ms": med, "min_ms": ms[0],
                        "frac_at_median": fl / med / 1e9 / PEAKS["mfma16"], "frac_at_min": fl / ms[0] / 1e9 / PEAKS["mfma16"],
                        "kernel": ops.attention_kernel_name(256, 512, 4),
                        "note": "kernel alone on the device, random (gaussian) Q K V, q pre-scaled by log2(e)/sqrt(hd) as the path's W_q pack does (prescaled call).  avg_ms / tflops / "
                                "frac_bf16_mfma_peak: the launch repeated back to back for >= 2 s between one pair of HIP events (launch gaps "
                                "included; the queue is kept 200 launches deep) - the steady state: the part runs this kernel at its socket "
                                "power limit, ~2.14-2.26 GHz (profiles/r04/power_probe.txt).  window_*: five windows of 20 launches, each started "
                                "from an idle device (the shader clock is still ramping: rounds 1-3 quoted their median, "
                                "frac_windows_median); median_ms / min_ms: a further 20 launches with an event after each"}
    return out


# ---------------------------------------------------------------------------------------------------------------
# forward workloads
# ---------------------------------------------------------------------------------------------------------------
def forward_leg(args, workload, rank, world, steps, warmup, streams_req, batch=0, sustained=True, graph=False, tags=False,
                profile=True, keep_outputs=False):
    """one forward workload: calibration of the passes in flight, warm-up, one instrumented pass alone on the device (profile),
    `steps` timed steps between barriers (profile: with the dominant family event-timed per launch), three strictly sequential
    passes (profile: exclusive launch durations, single-pass step), optionally the >= 2 s sustained loop.  keep_outputs: the
    record's `outputs` = collect_outputs of what the last timed step returned.  Every rank calls it; returns a dict."""
    import torch
    import torch.distributed as dist
    from sincformer_metacog_speech_enhancement_amd import ops, synthetic as syn
    B, L, desc = WORKLOADS[workload]
    if batch:
        B = batch
    T = 1 + L // 80
    use_memory = workload == "c5"
    path, weights = build_path(args.dtype, use_memory=use_memory)
    path = path.cuda().eval()
    noisy, _ = syn.synth_wave(B, L, 1234 + rank)          # each rank enhances its own utterance shard
    wave = torch.from_numpy(noisy).cuda()
    n_streams = streams_req

    if graph:
        from sincformer_metacog_speech_enhancement_amd.graph import GraphedForward
        # one captured graph (with its own static buffers) per pass in flight: a graph is never replayed concurrently with itself
        graphs = [GraphedForward(lambda w: path(w)) for _ in range(max(n_streams, 1))]
        for g_ in graphs:
            g_(wave)                                      # capture outside the timed region
        graphed = graphs[0]

    auto_streams = n_streams == 0
    if auto_streams:
        n_streams = 2
    # the current (default) stream + S-1 new ones: as few HIP streams as possible, so that they never have to share one of
    # the process's hardware queues (5 streams on 4 queues ran SLOWER than a single stream: 12.9 vs 11.0 ms)
    box = {"streams": ([torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]) if n_streams > 1 else None,
           "counter": 0}

    def step():
        streams = box["streams"]
        if streams is not None:
            st = streams[box["counter"] % len(streams)]
            box["counter"] += 1
            with torch.cuda.stream(st):
                return graphs[(box["counter"] - 1) % len(streams)](wave) if graph else path(wave)
        return graphed(wave) if graph else path(wave)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if rank == 0:
        print("[bench] %s, dtype %s, world %d" % (desc, args.dtype, world), file=sys.stderr, flush=True)
    with torch.no_grad():
        calib = None
        if auto_streams and not graph:
            # calibration (untimed, part of the warm-up): 6 passes each with 1, 2 and 3 passes in flight; the fastest wins
            # (more streams than the process has hardware queues run SLOWER than one: never assume, measure)
            def timed(n):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(n):
                    step()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / n
            pool = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
            res = {}
            for cand in (3, 2, 1):
                box["streams"] = pool[:cand] if cand > 1 else None
                for _ in range(cand):
                    step()
                res[cand] = timed(6)
            best = min(res, key=lambda c: res[c] * (1.0 + 0.01 * c))          # prefer fewer passes in flight on a tie
            n_streams = best
            box["streams"] = pool[:best] if best > 1 else None
            calib = {str(c): res[c] * 1e3 for c in (1, 2, 3)}
            if rank == 0:
                print("[bench] calibration (ms/pass): %s -> --streams %d" %
                      (", ".join("%d in flight %.2f" % (c, res[c] * 1e3) for c in (1, 2, 3)), best), file=sys.stderr, flush=True)
        # warm-up; then ONE instrumented pass, alone on the device (everything enqueued before it has finished), to find the
        # dominant kernel family and the exclusive per-family times
        for i in range(max(warmup, 1)):
            step()
        torch.cuda.synchronize()
        breakdown, launches_one, dominant, launches, gpu_masks = {}, {}, None, None, None
        if profile:
            ops.profiler.enable(None, tags=tags)
            out_one = path(wave)                          # eager, so the per-launch events exist even with --graph
            breakdown = ops.profiler.summary()
            launches_one = {k: ops.profiler.launches(k) for k in breakdown if "[" not in k}
            ops.profiler.disable()
            gpu_masks = (out_one["mask_real"][:1].cpu(), out_one["mask_imag"][:1].cpu()) if rank == 0 else None
            del out_one
            dominant = max((k for k in breakdown if "[" not in k), key=lambda k: breakdown[k]["ms_total"])
        refuse_variant_overrides()
        if profile and not graph:
            ops.profiler.enable({dominant})
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            if keep_outputs and i == steps - 1:
                last = step()
            else:
                step()
        barrier()
        elapsed = time.perf_counter() - t0
        if profile:
            launches = launches_one[dominant] if graph else ops.profiler.launches(dominant)
            ops.profiler.disable()
        outputs = None
        if keep_outputs:                                  # before anything else runs: a graph replay reuses its output buffers
            outputs = collect_outputs(last)
            del last
        # with several passes in flight the live per-launch durations include the time a kernel shares the chip with the
        # other stream's kernels; strictly sequential passes AFTER the timed region give the exclusive durations and the
        # single-pass step time
        launches_excl, single_ms = None, None
        if profile and not graph:
            torch.cuda.synchronize()
            ops.profiler.enable({dominant})
            t1 = time.perf_counter()
            for _ in range(3):
                path(wave)
            torch.cuda.synchronize()
            single_ms = (time.perf_counter() - t1) / 3 * 1e3
            launches_excl = ops.profiler.launches(dominant)
            ops.profiler.disable()
        # sustained figure: the same step() loop for >= 2 s of wall time and >= 250 steps (the timed region above is K steps
        # as the contract says - a burst of a fraction of a second at the default K), dominant family timed live
        sus = None
        if sustained:
            if profile and not graph:
                ops.profiler.enable({dominant})
            barrier()
            t2 = time.perf_counter()
            n_s = 0
            while True:
                for _ in range(50):
                    step()
                n_s += 50
                torch.cuda.synchronize()
                # every rank runs the same number of steps: rank 0's clock decides
                go = torch.tensor([1.0 if (time.perf_counter() - t2 < 2.0 or n_s < 250) else 0.0], device="cuda")
                if world > 1:
                    dist.broadcast(go, 0)
                if float(go.item()) == 0.0:
                    break
            barrier()
            dt_s = time.perf_counter() - t2
            sus = {"steps": n_s, "seconds": dt_s, "ms_per_step": dt_s / n_s * 1e3, "frames_per_s": world * B * T * n_s / dt_s}
            if profile and not graph:
                ds = ops.profiler.summary()[dominant]
                sus.update({"dominant_kernel": dominant, "dominant_avg_ms": ds["ms_avg"], "dominant_launches": ds["n"]})
                ops.profiler.disable()
    tmax = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax.item())
    del path, wave
    torch.cuda.empty_cache()
    return {"workload": workload, "desc": desc, "B": B, "L": L, "T": T, "elapsed": elapsed, "steps": steps, "streams": n_streams,
            "calib": calib, "breakdown": breakdown, "launches_one": launches_one, "dominant": dominant, "launches": launches,
            "launches_excl": launches_excl, "single_ms": single_ms, "sustained": sus, "gpu_masks": gpu_masks, "weights": weights,
            "noisy": noisy, "use_memory": use_memory, "policy": ops.policy_name(), "outputs": outputs}


def forward_roofline(r, passes_in_flight):
    roof = roofline_of(r["dominant"], r["launches"], traffic_file(r["workload"]))
    if r["launches_excl"]:
        ex = roofline_of(r["dominant"], r["launches_excl"])
        roof.update({"passes_in_flight": passes_in_flight, "exclusive_achieved": ex["achieved"], "exclusive_frac": ex["frac"],
                     "exclusive_avg_ms": ex["avg_ms"], "exclusive_bound": ex["bound"],
                     "note": "achieved / avg_ms are live in the timed region, where %d pass(es) share the chip; "
                             "exclusive_* are the same launches in 3 strictly sequential passes right after "
                             "it" % passes_in_flight})
    return roof


def attention_in_pass(r):
    att = r["breakdown"].get("attention_fwd")
    if not att:
        return None
    tf = att["flops"] / att["n"] / (att["ms_avg"] * 1e-3) / 1e12
    return {"tflops": tf, "frac_bf16_mfma_peak": tf / PEAKS["mfma16"], "avg_ms": att["ms_avg"],
            "shape": "B%d x T%d x 4 heads x 64 (this workload), instrumented pass alone on the device" % (r["B"], r["T"])}


def breakdown_of(r):
    return {k: round(v["ms_total"], 4) for k, v in sorted(r["breakdown"].items(), key=lambda kv: -kv[1]["ms_total"]) if "[" not in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline figure: the instrumented pass (breakdown, roofline), sequential "
                         "passes, the sustained loop, the sub-records of the default line and the CPU baseline with mask_rmse "
                         "(the --no-* / --train-* / --configs1-* / --dp-* options shape these)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32 / float64, at most "
                         "64 MB in all: larger arrays as a fixed seeded sample of their elements)")
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: c3p = the shape BASELINE's metric names (B 256 x 512-frame utterances); with --full the "
                         "default line also carries `configs1` (BASELINE configs[1], B 64 x 4 s) and `train` (configs[2] on the "
                         "north-star composition) at N = 1, and with --gpus N > 1 a `dp_train` sub-record: the c3se training step "
                         "with the RCCL gradient all-reduce (BASELINE configs[3])")
    ap.add_argument("--dp-batch", type=int, default=0, help="per-GPU batch of the dp_train sub-record (default: the workload's 256)")
    ap.add_argument("--dp-steps", type=int, default=5)
    ap.add_argument("--dp-warmup", type=int, default=2)
    ap.add_argument("--no-dp-train", action="store_true", help="N > 1, default workload: skip the dp_train sub-record")
    ap.add_argument("--train-steps", type=int, default=5, help="timed steps of the `train` sub-record (default line, N = 1)")
    ap.add_argument("--train-warmup", type=int, default=3)
    ap.add_argument("--train-batch", type=int, default=0, help="per-GPU batch of the `train` sub-record (default: c3t's 256)")
    ap.add_argument("--no-train", action="store_true", help="default line, N = 1: skip the `train` sub-record")
    ap.add_argument("--no-configs1", action="store_true", help="default line: skip the `configs1` sub-record")
    ap.add_argument("--configs1-batch", type=int, default=0, help="per-GPU batch of the `configs1` sub-record (default 64)")
    ap.add_argument("--no-sustained", action="store_true", help="skip the >= 2 s sustained loop after the timed region")
    ap.add_argument("--dtype", default="mixed", choices=["mixed", "bf16", "f16"],
                    help="16-bit operand formats: mixed = the default per-stage policy (ops.POLICIES['mixed']; training: fp16 + "
                         "dynamic loss scale)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-headline", action="store_true", help="skip the attention-kernel-alone measurement at B256 x T512")
    ap.add_argument("--breakdown", default=None, help="write the per-kernel-family breakdown JSON here (needs --full)")
    ap.add_argument("--batch", type=int, default=0, help="override the per-GPU batch of the workload")
    ap.add_argument("--graph", action="store_true", help="replay the forward as one hipGraph (launch-bound small batches)")
    ap.add_argument("--streams", type=int, default=0, help="forward passes in flight: consecutive steps alternate over this many "
                    "HIP streams (each step is still one whole pass over its own buffers; 1 = strictly one pass at a time; "
                    "0 = auto: a short calibration during warm-up picks the fastest of 1, 2 and 3 on this machine)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if args.breakdown and not args.full:
        raise SystemExit("bench.py: --breakdown comes from the instrumented pass of --full")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))                          # before anything in this process touches the GPU
    default_line = args.workload is None
    if default_line:
        args.workload = "c3p"
    if args.workload in TRAIN_WORKLOADS:
        return main_train(args)

    import torch
    import torch.distributed as dist
    rank, world = init_ranks(args)
    full = args.full
    dp_sub = full and default_line and world > 1 and not args.no_dp_train
    train_sub = full and default_line and world == 1 and not args.no_train
    c1_sub = full and default_line and not args.no_configs1

    r = forward_leg(args, args.workload, rank, world, args.steps, args.warmup, args.streams, batch=args.batch,
                    sustained=full and not args.no_sustained, graph=args.graph, tags=bool(args.breakdown), profile=full,
                    keep_outputs=bool(args.dump_outputs) and rank == 0)
    if rank == 0 and r["outputs"] is not None:
        write_outputs(args.dump_outputs, r["outputs"])
        r["outputs"] = None
    # the attention kernel alone comes right after the primary workload: it is specified like the timed region - the kernel on
    # a chip that has just run the K steps - and the other ranks simply wait at the next barrier
    headline = None
    if full and rank == 0 and not args.no_headline and default_line:
        headline = headline_attention()
    c1 = None
    if c1_sub:
        c1 = forward_leg(args, "c2", rank, world, 10, 3, args.streams, batch=args.configs1_batch, sustained=False)
    tr = None
    if train_sub:
        tr = train_leg(args, "c3t", rank, world, args.train_steps, args.train_warmup, batch=args.train_batch)
    dp_rec = dp_train_record(args, rank, world) if dp_sub else None

    frames = world * r["B"] * r["T"] * r["steps"]
    if rank == 0:
        elapsed = r["elapsed"]
        line = {
            "metric": METRIC,
            "value": frames / elapsed, "unit": "STFT frames/s (whole job)", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_DESC[args.dtype], "data": "synthetic",
            "config": {"workload": r["desc"], "batch_per_gpu": r["B"], "samples": r["L"], "frames_per_utt": r["T"],
                       "sharding": "utterances over ranks, no data-path collective",
                       "launch": "one hipGraph replay per step" if args.graph else "eager launches",
                       "streams": r["streams"], "precision_policy": r["policy"]},
            "frames_per_s_per_gpu": frames / elapsed / world,
        }
        if full:
            line["roofline"] = forward_roofline(r, r["streams"])
        if default_line:
            line["config"]["why_this_workload"] = ("the shape BASELINE.json's metric and north_star target are quoted on (batch 256 x "
                                                   "512-frame utterances); BASELINE configs[1] (B 64 x 4 s) is the `configs1` sub-record, "
                                                   "configs[2] the `train` sub-record (both with --full)")
        if r["calib"]:
            line["config"]["calibration_ms_per_pass"] = r["calib"]
        if r["single_ms"] is not None:
            line["single_pass_ms_per_step"] = r["single_ms"]
        att = attention_in_pass(r)
        if att:
            line["attention"] = att
        if full:
            line["breakdown_ms_per_step"] = breakdown_of(r)
            line["breakdown_note"] = "one instrumented pass alone on the device (HIP events per launch); sums to the single-pass step"
        if r["sustained"]:
            sus = r["sustained"]
            sus["vs_timed_region"] = sus["ms_per_step"] / line["ms_per_step"]
            sus["note"] = ("`value` / `ms_per_step` are the K timed steps of the contract; this is the same loop kept up "
                           "for >= 2 s and >= 250 steps (clock and thermal steady state)")
            line["sustained"] = sus
        if headline:
            line["headline"] = headline
        if c1:
            fr1 = world * c1["B"] * c1["T"] * c1["steps"]
            line["configs1"] = {"workload": c1["desc"], "batch_per_gpu": c1["B"], "steps": c1["steps"], "warmup": 3,
                                "ms_per_step": c1["elapsed"] / c1["steps"] * 1e3, "frames_per_s": fr1 / c1["elapsed"],
                                "streams": c1["streams"], "single_pass_ms_per_step": c1["single_ms"],
                                "roofline": forward_roofline(c1, c1["streams"]), "attention": attention_in_pass(c1),
                                "breakdown_ms_per_step": breakdown_of(c1)}
            if c1["calib"]:
                line["configs1"]["calibration_ms_per_pass"] = c1["calib"]
        if tr:
            line["train"] = train_subrecord(tr, "c3t")
        if dp_rec:
            line["dp_train"] = dp_rec
        print("[bench] gpu leg done: %.1f ms/step, %.3e frames/s%s" % (line["ms_per_step"], line["value"],
              "; dominant kernel %s" % r["dominant"] if r["dominant"] else ""), file=sys.stderr, flush=True)
        if full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], rm = cpu_baseline(r["weights"], r["L"], r["noisy"], gpu_masks=r["gpu_masks"],
                                                    use_memory=r["use_memory"])
            line["mask_rmse"] = {"value": rm, "bound": 1e-3, "what": "RMSE of (mask_real | mask_imag) of utterance 0 of the bench "
                                 "batch, HIP path (this dtype) vs the CPU oracle (fp32), outside the timed region"}
        if args.breakdown:
            with open(args.breakdown, "w") as fh:
                json.dump({"breakdown": r["breakdown"],
                           "launches": {k: v for k, v in r["launches_one"].items()}}, fh, indent=1)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
