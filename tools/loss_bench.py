#!/usr/bin/env python3
"""PerceptualSTOILoss micro-benchmark at the training shape (B 256 x T 501 x F 129, 14 bands): sfm_pstoi_loss in both input
forms ([B, F, T] magnitudes; channels-last (real, imag) pairs), each with and without the gradient, and the same formula
composed of torch ops on the device (forward; forward + autograd backward), all in one process.  The variants are timed in
alternating rounds (device events around `iters` back-to-back calls after a warm-up of every shape); the median round is
reported with the spread, next to the bytes each launch has to move (ops.pstoi_bytes: every used input element once, every
gradient element once) and the bytes per second they imply.  The kernel's and the composition's losses are compared first.

    python tools/loss_bench.py [--B 256] [--T 501] [--iters 100] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sincformer_metacog_speech_enhancement_amd import ops  # noqa: E402
from sincformer_metacog_speech_enhancement_amd.training import PerceptualSTOILoss  # noqa: E402


def composed(enh, clean, w, frame_len=30, beta=15.0):
    """the reference's formula in torch ops, [B, F, T] magnitudes"""
    ec, ee = torch.matmul(w.unsqueeze(0), clean), torch.matmul(w.unsqueeze(0), enh)
    B, NB, T = ec.shape
    S = max(1, T // frame_len)
    sc = ec[..., :S * frame_len].reshape(B, NB, S, frame_len)
    se = ee[..., :S * frame_len].reshape(B, NB, S, frame_len)
    sc = sc - sc.mean(dim=-1, keepdim=True)
    se = se - se.mean(dim=-1, keepdim=True)
    nc = torch.sqrt(torch.sum(sc ** 2, dim=-1, keepdim=True) + 1e-8)
    ne = torch.sqrt(torch.sum(se ** 2, dim=-1, keepdim=True) + 1e-8)
    ratio = 10 ** (beta / 20.0) * nc / (ne + 1e-8)
    cl = se * torch.min(torch.ones_like(ratio), ratio)
    num = torch.sum(sc * cl, dim=-1)
    den = torch.sqrt(torch.sum(sc ** 2, dim=-1) + 1e-8) * torch.sqrt(torch.sum(cl ** 2, dim=-1) + 1e-8)
    return -(num / (den + 1e-8)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=501)
    ap.add_argument("--F", type=int, default=129)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: needs the GPU (a CPU timing says nothing about it)")
    B, T, F = a.B, a.T, a.F
    g = torch.Generator(device="cuda").manual_seed(0)
    U = lambda *s: torch.rand(*s, device="cuda", generator=g)
    w = PerceptualSTOILoss().band_weights.cuda()
    er, ei, cr, ci = (U(B, T, F) - 0.5 for _ in range(4))
    me = torch.sqrt(er * er + ei * ei + 1e-8).transpose(1, 2).contiguous()
    mc = torch.sqrt(cr * cr + ci * ci + 1e-8).transpose(1, 2).contiguous()
    me_g = me.clone().requires_grad_(True)
    er_g, ei_g = er.clone().requires_grad_(True), ei.clone().requires_grad_(True)

    def torch_fwd_bwd():
        me_g.grad = None
        composed(me_g, mc, w).backward()

    def torch_cl_fwd_bwd():
        er_g.grad = ei_g.grad = None
        composed(torch.sqrt(er_g * er_g + ei_g * ei_g + 1e-8).transpose(1, 2),
                 torch.sqrt(cr * cr + ci * ci + 1e-8).transpose(1, 2), w).backward()

    variants = {
        "hip_bft_fwd": (lambda: ops.pstoi_loss(me, mc, w), ops.pstoi_bytes(B, T, F, 30, False, False), a.iters),
        "hip_bft_fwd_grad": (lambda: ops.pstoi_loss(me, mc, w, need_grad=True), ops.pstoi_bytes(B, T, F, 30, False, True), a.iters),
        "hip_cl_fwd": (lambda: ops.pstoi_loss((er, ei), (cr, ci), w), ops.pstoi_bytes(B, T, F, 30, True, False), a.iters),
        "hip_cl_fwd_grad": (lambda: ops.pstoi_loss((er, ei), (cr, ci), w, need_grad=True), ops.pstoi_bytes(B, T, F, 30, True, True),
                            a.iters),
        "torch_bft_fwd": (lambda: composed(me, mc, w), None, max(a.iters // 5, 4)),
        "torch_bft_fwd_bwd": (torch_fwd_bwd, None, max(a.iters // 5, 4)),
        "torch_cl_fwd_bwd": (torch_cl_fwd_bwd, None, max(a.iters // 10, 4)),
    }
    # the kernel against the composition on these inputs (fp32 on both sides)
    l_hip, g_hip = ops.pstoi_loss(me, mc, w, need_grad=True)
    l_cl, _ = ops.pstoi_loss((er, ei), (cr, ci), w, need_grad=True)
    torch_fwd_bwd()
    check = {"loss_hip_bft": float(l_hip), "loss_hip_cl": float(l_cl), "loss_torch": float(composed(me, mc, w)),
             "grad_rel_rmse_vs_torch": float((g_hip - me_g.grad).double().pow(2).mean().sqrt() /
                                             me_g.grad.double().pow(2).mean().sqrt())}
    for fn, _, _ in variants.values():                      # warm-up: every shape, every code object
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, _, iters) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    out = {"B": B, "T": T, "F": F, "iters": a.iters, "rounds": a.rounds, "check": check, "variants": {}}
    for k, (_, nbytes, _) in variants.items():
        ms = statistics.median(times[k])
        row = {"ms_median": round(ms, 5), "ms_min": round(min(times[k]), 5), "ms_max": round(max(times[k]), 5)}
        if nbytes is not None:
            row["MB_moved"] = round(nbytes / 1e6, 2)
            row["TBps"] = round(nbytes / ms / 1e9, 3)
        out["variants"][k] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
