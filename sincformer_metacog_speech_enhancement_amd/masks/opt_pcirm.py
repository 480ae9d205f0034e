"""Mirror of masks/opt_pcirm.py: the fixed-step OPT-PCIRM quantiser on device tensors (csrc/masks.hip, sfm_mask_quantize).
The PSO search of the middle step (optimizer/pso.py) is out of scope."""
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


def compute_opt_pcirm(pcirm, noisy_signal=None, clean_signal=None, fs=None, num_steps=None, use_pso=True, pso_config=None):
    """masks/opt_pcirm.py:106-200 with use_pso=False only -> (opt_mask, step_values, step_values[1]).  The signals and `fs` feed
    the PSO's STOI fitness alone and are not read."""
    if use_pso:
        raise NotImplementedError("compute_opt_pcirm (HIP build): the PSO search of the middle step (optimizer/pso.py, "
                                  "ParticleSwarmOptimizer) is out of scope; pass use_pso=False for the fixed steps")
    steps, _ = compute_snr_boundaries(num_steps=num_steps)
    return quantize_pcirm(pcirm, steps), steps, (steps[1] if len(steps) > 1 else None)
