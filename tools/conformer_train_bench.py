#!/usr/bin/env python3
"""One epoch of ConformerPipeline._train_epoch over 512 utterances of 4 s (8 kHz), at batch 8 and at batch 256, fed two ways
in one process:

  resident   train()'s form: WaveformSet.batches(batch, shuffle=True, drop_last=True) - a device permutation, one
             sfm_wave_batch launch per step, no host data
  host       what the library offered before: the same epoch body iterating over (noisy, clean) pairs of pageable host tensors,
             as a DataLoader hands them over (one host-to-device copy of each per step; the mixes were made ahead of time)

Wall time of whole epochs (each ends with _train_epoch's own readback), the arms alternating epoch by epoch after a warm-up epoch of
each; per arm the median and the spread.  Also the launch of one sfm_wave_batch alone (device events), and the device bytes held.

    python tools/conformer_train_bench.py [--utterances 512] [--epochs 5] [--batches 8,256]
    python tools/conformer_train_bench.py --trace-epochs 2 --batches 8     # resident epochs only, for a kernel trace of its own:
                                                                           # wall time per step against the trace's kernel time
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FS, SECONDS = 8000, 4


def make_set(n_utt, gen):
    from sincformer_metacog_speech_enhancement_amd import training
    L = FS * SECONDS
    clean = torch.randn(n_utt, L, device="cuda", generator=gen) * 0.1
    lengths = [L - (37 * i) % 4000 for i in range(n_utt)]                   # ragged: 3.5 .. 4 s
    noises = [torch.randn(n, device="cuda", generator=gen) * 0.3 for n in (FS * 30, FS * 7, 12345)]
    return training.WaveformSet.from_padded(clean, lengths, noises, [-5, 0, 5, 10], FS)


def epoch_wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batches", default="8,256")
    ap.add_argument("--trace-epochs", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conformer_train_bench: needs the GPU (a CPU timing says nothing about it)")
    from sincformer_metacog_speech_enhancement_amd import ops
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp
    gen = torch.Generator(device="cuda").manual_seed(26)
    ws = make_set(a.utterances, gen)
    torch.manual_seed(0)
    pipe = cp.ConformerPipeline(fs=FS)
    pipe.model = pipe._new_model().to(pipe.device)
    mr = cp.MultiResolutionSTFTLoss()
    optimizer, scaler = pipe.make_optimizer()
    res = {"utterances": len(ws), "samples": ws.max_len, "format": ops.dtype_name(),
           "device_bytes": {"set": 4 * ws.clean.numel(), "stored_pairs": 8 * len(ws) * ws.max_len}}
    for batch in [int(b) for b in a.batches.split(",")]:
        steps = len(ws) // batch
        resident = lambda: pipe._train_epoch(ws.batches(batch, shuffle=True, drop_last=True), optimizer, mr, scaler)
        if a.trace_epochs:
            resident()
            t = [epoch_wall(resident) for _ in range(a.trace_epochs)]
            print(json.dumps({"batch": batch, "steps": steps, "epoch_s": t, "step_ms_wall": [round(x / steps * 1e3, 3) for x in t]}))
            continue
        order = torch.arange(steps * batch, device="cuda", dtype=torch.int32)
        pairs = [tuple(t.cpu() for t in ws.batch(order[s * batch:(s + 1) * batch])) for s in range(steps)]
        host = lambda: pipe._train_epoch(pairs, optimizer, mr, scaler)
        arms = {"resident": resident, "host": host}
        for fn in arms.values():
            fn()
        t = {k: [] for k in arms}
        for _ in range(a.epochs):
            for k, fn in arms.items():
                t[k].append(epoch_wall(fn))
        row = {k: {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4),
                   "step_ms": round(statistics.median(v) / steps * 1e3, 3)} for k, v in t.items()}
        row["steps"] = steps
        row["host_over_resident"] = round(statistics.median(t["host"]) / statistics.median(t["resident"]), 3)
        index = torch.randperm(len(ws), device="cuda", dtype=torch.int32)[:batch]
        out = torch.empty(2, batch, ws.max_len, device="cuda")
        call = lambda: ops.wave_batch(ws.clean, ws.offsets, ws.bank.buffer, ws.bank.offsets, ws.noise_ids, ws.scale, index, ws.max_len, out=out)
        for _ in range(20):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) / 200 * 1e3
        row["wave_batch_us"] = round(us, 2)
        row["wave_batch_GBps"] = round(16.0 * batch * ws.max_len / (us * 1e-6) / 1e9, 1)       # 4 read + 4 noise + 8 written a sample
        res["batch%d" % batch] = row
    if not a.trace_epochs:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
