"""Batched, on-device counterparts of the reference's evaluation/ssnr.py, evaluation/csii.py and evaluation/ncm.py and of the
fallbacks of evaluation/stoi.py and evaluation/pesq_eval.py, and all of them over a ragged set in packed passes; and STOI of
Taal et al. with its extended form, the pystoi branch of evaluation/stoi.py (stoi_taal.py)."""
from .ssnr import compute_ssnr, compute_ssnr_improvement  # noqa: F401
from .stoi import compute_stoi  # noqa: F401
from .stoi_taal import compute_stoi_taal, compute_stoi_taal_packed, stoi_taal_scores  # noqa: F401
from .pesq_eval import compute_pesq  # noqa: F401
from .csii import compute_csii  # noqa: F401
from .ncm import compute_ncm, hilbert_envelope  # noqa: F401
from .packed import compute_metrics_packed  # noqa: F401
from .intelligibility import compute_intelligibility_packed  # noqa: F401
