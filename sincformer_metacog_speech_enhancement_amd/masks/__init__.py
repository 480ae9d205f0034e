from .irm import compute_irm
from .opt_pcirm import compute_opt_pcirm, compute_snr_boundaries, quantize_pcirm
from .pcirm import (compute_correlation_coefficients, compute_pcirm, compute_pcirm_from_signals,
                    compute_phase_differences)

__all__ = ["compute_correlation_coefficients", "compute_irm", "compute_opt_pcirm", "compute_pcirm",
           "compute_pcirm_from_signals", "compute_phase_differences", "compute_snr_boundaries", "quantize_pcirm"]
