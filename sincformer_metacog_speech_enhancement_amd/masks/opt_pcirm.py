"""Mirror of masks/opt_pcirm.py on device tensors: the OPT-PCIRM quantiser (csrc/masks.hip, sfm_mask_quantize) and the search of
its middle step by a particle swarm (csrc/pso.hip, optimizer/pso.py) that maximises the STOI fallback or - pso_config["fitness"] -
the STOI / ESTOI of Taal et al. (csrc/stoi.hip, evaluation/stoi_taal.py).

The search never rebuilds a signal.  quantize_pcirm puts the candidate x into exactly the units of step 2, so the channel mean
of mask frame n is a[n] + x b[n], the overlap-add of the reference's fitness (:160-179) is a per-sample gain ga + x gb, the
enhanced signal is ya + x yb and - the DFT being linear - every STOI frame has the spectrum A + x B.  One search therefore costs
three framed DFT passes (clean, ya, yb) and four moments, once; after that a round reads |C|, A, B once for all N particles.
On the Taal measures the resampler, the kept-frame list (the clean signal's), the overlap-add and the windowed DFT are linear in
the enhanced signal as well, so the energy of band j of spectral frame m is the quadratic P + 2 x Q + x^2 R: one search costs the
clean band rows and the three fp64 planes P | Q | R (ops.stoi_bands_pair), once; a round evaluates sqrt(E(x)) per band and frame
and the 15 x 30 segment terms per particle (ops.pso_fitness_taal) - no DFT, no resampling, no signal.
A batch runs one swarm per utterance side by side; each utterance gets the bits it gets alone."""
import numpy as np
import torch

from .. import config, ops
from ._device import planes

_tables = {}


def compute_snr_boundaries(local_criterion_db=None, num_steps=None):
    """masks/opt_pcirm.py:24-52 -> (step_values float64 [M], exponent): n = -log2(lc / (lc + 1)), s_m = ((m - 1) / M)^n.
    Host arithmetic in float64."""
    lc_db = local_criterion_db if local_criterion_db is not None else config.LOCAL_CRITERION_DB
    M = num_steps or config.OPT_NUM_STEPS
    lc = 10 ** (lc_db / 10.0)
    n_exp = -np.log2(lc / (lc + 1.0))
    steps = np.zeros(M)
    for m in range(1, M + 1):
        steps[m - 1] = ((m - 1) / M) ** n_exp
    return steps, n_exp


def quantizer_table(step_values, middle_value=None, device="cuda"):
    """(table, M) of sfm_mask_quantize: boundaries [0, s_2 .. s_M, 1] from the UNMODIFIED step values, then the assigned values
    (`middle_value` replaces that of step 2 only, and only when M >= 3), float64 on the device.  Uploaded once per content."""
    steps = np.asarray(step_values, dtype=np.float64).reshape(-1)
    M = steps.size
    if not 2 <= M <= ops.QUANT_MAX_STEPS:
        raise ValueError("quantize_pcirm: %d steps; the kernel takes 2..%d" % (M, ops.QUANT_MAX_STEPS))
    values = steps.copy()
    if middle_value is not None and M >= 3:
        values[1] = middle_value
    bounds = np.concatenate([[0.0], steps[1:], [1.0]])
    host = np.concatenate([bounds, values])
    key = (host.tobytes(), str(torch.device(device)))
    t = _tables.get(key)
    if t is None:
        if len(_tables) > 64:
            _tables.clear()
        t = _tables[key] = torch.from_numpy(host).to(device)
    return t, M


def quantize_pcirm(pcirm, step_values, middle_value=None):
    """masks/opt_pcirm.py:55-103.  Step m is assigned where boundary[m] <= x < boundary[m + 1]; x >= 1 takes the last value; a
    NaN or a negative input stays 0.  The fp32 mask values are compared with the float64 boundaries in double, as numpy
    compares them, and the assigned values are the float64 step values rounded to fp32: the result is the reference's."""
    x, = planes("quantize_pcirm", pcirm)
    table, M = quantizer_table(step_values, middle_value, x.device)
    return ops.mask_quantize(x, table, M)


PSO_KEYS = ("num_particles", "max_iter", "w", "c1", "c2", "bounds", "lengths", "draws", "history", "fitness")
FITNESS = ("fallback", "stoi_taal", "estoi")        # the measure the swarm climbs: the names of compute_metrics_packed


def _taal_fitness(seg, fs, cp, ya, yb, extended, dev):
    """what one search on a Taal measure computes once -> fitness(state, out): the clean band rows and the planes P | Q | R of
    ya + x yb, from the packed signals of ops.pso_split.  None where no utterance reaches one frame at 10 kHz (every score is the
    measure's 1e-5)."""
    from ..evaluation import stoi_taal as st
    plan, tabs = st._packed_plan(seg, fs, dev)
    if plan["sum_frames"] == 0:
        return None
    op = st._device_operands(dev, fs)
    rc, ra, rb = (st._resample(s, plan, tabs, op) for s in (cp, ya, yb))
    src, kept, _ = ops.stoi_keep(rc, op["win"], tabs["sig_off"], tabs["sig_len"], tabs["frame_off"], plan["B"], plan["sum_frames"],
                                 plan["n_samples"])
    args = (op["win"], op["dft"], tabs["sig_off"], tabs["frame_off"], src, kept, tabs["tiles"], plan["sum_frames"], plan["spec_rows"],
            plan["n_samples"])
    xb, = ops.stoi_bands((rc,), *args)
    planes = ops.stoi_bands_pair(ra, rb, *args)
    return lambda state, out: ops.pso_fitness_taal(xb, planes, tabs["frame_off"], kept, state.pos, state.stopped, out, extended,
                                                   plan["spec_rows"], plan["segments"])


def compute_opt_pcirm(pcirm, noisy_signal=None, clean_signal=None, fs=None, num_steps=None, use_pso=True, pso_config=None):
    """masks/opt_pcirm.py:101-202 -> (opt_mask, step_values, optimized_middle).

    pcirm: fp32 device tensor (C, T) or [B, C, T]; the signals: 1-D or [B, L], device tensors or numpy arrays, trimmed to their
    common length (evaluation/stoi.py:42-44).  use_pso=False: the fixed steps, the signals are not read.  use_pso=True: the
    middle step that the swarm finds, a Python float for one utterance and a float64 device tensor [B] for a batch; without both
    signals there is nothing to score and the call raises NotImplementedError.  pso_config: the reference's six keys
    ('num_particles', 'max_iter', 'w', 'c1', 'c2', 'bounds') and
      'lengths'  [B] samples of each utterance of a padded batch (default: the common length);
      'draws'    float64 [B, 2 N + 2 N max_iter] (default: optimizer.pso.pso_draws per utterance, in batch order);
      'history'  True: a fourth result, the per-round record of each swarm (SwarmState.fetch: a dict, or a list of B);
      'fitness'  what the swarm maximises: "fallback" (default) the reference's _stoi_simplified, "stoi_taal" / "estoi" the STOI /
                 ESTOI of Taal et al. as evaluation.compute_stoi_taal scores ya + x yb (fs out of stoi_taal.RATES, else
                 NotImplementedError before anything is launched; below 30 spectral frames every particle scores 1e-5).
    The mask frames are config.FRAME_SIZE / HOP_SIZE samples whatever fs (as there); fs sets the STOI frame (fallback) or selects
    the resampler (Taal).  max_iter + 1 rounds of two launches on the current stream, no host synchronisation between them."""
    steps, _ = compute_snr_boundaries(num_steps=num_steps)
    if not use_pso:
        return quantize_pcirm(pcirm, steps), steps, (steps[1] if len(steps) > 1 else None)
    if noisy_signal is None or clean_signal is None:
        raise NotImplementedError("compute_opt_pcirm: the PSO search of the middle step scores candidates by the STOI of "
                                  "noisy_signal against clean_signal; pass both, or use_pso=False for the fixed steps")
    from ..evaluation._common import to_device_batch
    from ..evaluation.packed import _spectra
    from ..evaluation.stoi import _dft_operand
    from ..optimizer.pso import SwarmState, check_swarm, pso_draws
    from .. import functional as Fn
    cfg = {"num_particles": config.PSO_NUM_PARTICLES, "max_iter": config.PSO_MAX_ITER, "w": config.PSO_W, "c1": config.PSO_C1,
           "c2": config.PSO_C2, "bounds": config.PSO_BOUNDS, "lengths": None, "draws": None, "history": False, "fitness": "fallback"}
    unknown = [k for k in (pso_config or {}) if k not in PSO_KEYS]
    if unknown:
        raise ValueError("compute_opt_pcirm: pso_config keys %r; known: %r" % (unknown, PSO_KEYS))
    cfg.update(pso_config or {})
    if cfg["fitness"] not in FITNESS:
        raise ValueError("compute_opt_pcirm: fitness %r; known: %r" % (cfg["fitness"], FITNESS))
    taal = cfg["fitness"] != "fallback"
    if taal:
        from ..evaluation.stoi_taal import check_rate
        fs = check_rate(fs)
    N, K, bounds = cfg["num_particles"], cfg["max_iter"], tuple(cfg["bounds"])
    check_swarm(N, K, bounds)
    M = len(steps)
    if not 2 <= M <= ops.QUANT_MAX_STEPS:
        raise ValueError("compute_opt_pcirm: %d steps; the kernels take 2..%d" % (M, ops.QUANT_MAX_STEPS))
    fs = fs or config.SAMPLE_RATE
    frame = int(0.0256 * fs)
    if frame < 2 or frame // 2 + 1 > ops.PSO_MAX_BINS:
        raise ValueError("compute_opt_pcirm: fs %r gives STOI frames of %d samples; 2..%d are taken" % (
            fs, frame, 2 * ops.PSO_MAX_BINS - 1))
    x, = planes("compute_opt_pcirm", pcirm)
    if x.dim() not in (2, 3):
        raise ValueError("compute_opt_pcirm: pcirm %s; (C, T) or [B, C, T] is needed" % (tuple(x.shape),))
    (noisy, clean), one_d = to_device_batch(noisy_signal, clean_signal)
    xb = x.unsqueeze(0) if x.dim() == 2 else x
    B, C, T = xb.shape
    if noisy.shape[0] != B or clean.shape[0] != B or one_d != (x.dim() == 2):
        raise ValueError("compute_opt_pcirm: pcirm %s with signals %s / %s" % (tuple(x.shape), tuple(noisy.shape), tuple(clean.shape)))
    Lmax = noisy.shape[1]
    L = np.full(B, Lmax, dtype=np.int64) if cfg["lengths"] is None else np.asarray(
        cfg["lengths"].cpu() if torch.is_tensor(cfg["lengths"]) else cfg["lengths"], dtype=np.int64).reshape(-1)
    if L.size != B or Lmax < 1 or int(L.min()) < 1 or int(L.max()) > Lmax:
        raise ValueError("compute_opt_pcirm: lengths %r for %d signals of %d samples" % (L.tolist(), B, Lmax))
    draws = cfg["draws"]
    if draws is None:
        draws = np.stack([pso_draws(N, K, bounds) for _ in range(B)])
    dev = x.device
    state = SwarmState(draws, N, K, cfg["w"], cfg["c1"], cfg["c2"], bounds, True, dev)
    if state.B != B:
        raise ValueError("compute_opt_pcirm: draws for %d swarms, %d utterances" % (state.B, B))

    seg = Fn.PackedSegments(1 + L // config.HOP_SIZE, L)
    hop = frame // 2
    tab = seg.metric_tables(dev, ((frame, hop),))[(frame, hop)]
    samp_off = seg.tables(dev)["samp_off"]
    lengths = (samp_off[1:] - samp_off[:-1]).contiguous()
    table, _ = quantizer_table(steps, None, dev)
    a, b = ops.pso_frame_coef(xb, table, M)
    ya, yb, cp, S = ops.pso_split(noisy, clean, lengths, samp_off, a, b, seg.sum_L, config.FRAME_SIZE, config.HOP_SIZE)
    if taal:
        fit_fn = _taal_fitness(seg, fs, cp, ya, yb, cfg["fitness"] == "estoi", dev)
        fit = torch.full((B, N), 1e-5, device=dev, dtype=torch.float64)
        for it in range(K + 1):
            if fit_fn is not None:
                fit_fn(state, fit)
            ops.pso_step(state, it, fitness=fit)
        return _result(x, xb, table, M, state, steps, one_d, cfg["history"])
    NC = max(1, -(-int(tab["n"].max()) // ops.PSO_FRAMES))
    partial = torch.empty(B, NC, N, device=dev, dtype=torch.float64)
    spectra = None
    if tab["sum"]:                                            # (no utterance reaches one STOI frame: every fitness is 0.0)
        W = _dft_operand(frame, dev)
        spectra = sum((_spectra(w, W, samp_off, tab, B, frame, hop) for w in (cp, ya, yb)), ())
    for it in range(K + 1):
        if spectra is not None:
            ops.pso_fitness(spectra, tab["frame_off"], lengths, S, state.pos, state.stopped, partial, tab["sum"])
        ops.pso_step(state, it, partial=partial, frame_off=tab["frame_off"])
    return _result(x, xb, table, M, state, steps, one_d, cfg["history"])


def _result(x, xb, table, M, state, steps, one_d, history):
    """the swarm's best middle value -> what compute_opt_pcirm returns"""
    middle = state.gbest[:, 0].contiguous()
    mask = ops.pso_quantize(xb, table, middle, M).view(x.shape)
    record = state.fetch() if (one_d or history) else None
    out = (mask, steps, record[0]["best_position"] if one_d else middle)
    if history:
        out += (record[0] if one_d else record,)
    return out
