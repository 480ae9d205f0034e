"""The operand contract of every ops wrapper that checks before it launches, as one table: a valid call on tiny CPU tensors
(through the stub harness of tests/ops_stub.py) and single-defect variants of it.  The valid call reaches _call as often as
the wrapper launches; every defect is refused with the header's "unsupported shape" before any launch (rbm_prob's sample plane
without a source of randomness: "bad argument").

Per operand the defects are letters: d another dtype, c a non-contiguous view of the same shape, f one row (1-D: one element)
fewer, - one rank fewer, + one rank more, n None.  Only what a wrapper's contract refuses is listed: an operand whose contract
is an element count has no rank defects, one that need not be contiguous has no c.  Scalar bounds and the defects that need
more than one operand's change are spelled out beside them."""
import copy
import types

import pytest
import torch

import ops_stub
import resynth_cases as rc
from sincformer_metacog_speech_enhancement_amd import ops

F16, BF16, F32, F64, I32 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32
_OTHER = {F32: F64, F64: F32, I32: torch.int64, F16: BF16}


def f32(*shape):
    return torch.zeros(*shape, dtype=F32)


def f64(*shape):
    return torch.zeros(*shape, dtype=F64)


def i32(*shape):
    return torch.zeros(*shape, dtype=I32)


def f16(*shape):
    return torch.zeros(*shape, dtype=F16)


DEFECT = {
    "d": lambda t: t.to(_OTHER[t.dtype]),
    "c": lambda t: torch.stack([t, t], -1)[..., 0],
    "f": lambda t: t[:-1].contiguous(),
    "-": lambda t: t.reshape(-1) if t.dim() > 1 else t[0],
    "+": lambda t: t.unsqueeze(0),
    "n": lambda t: None,
}
NAMES = {"d": "dtype", "c": "noncontiguous", "f": "one_fewer", "-": "rank_less", "+": "rank_more", "n": "none"}


def pack(N, K):
    return ops.PackedWeight(f16(64, 64), f32(64), N, K, 1, K, False)


def swarm(K=2):
    B, N = 2, 3
    return types.SimpleNamespace(B=B, N=N, max_iter=K, maximize=True, draws=f64(B, 2 * N + 2 * N * K), params=f64(5), pos=f64(B, N),
                                 vel=f64(B, N), pbest_pos=f64(B, N), pbest_fit=f64(B, N), gbest=f64(B, 2),
                                 hist=f64(B, K + 1, 3 + 2 * N), iters=i32(B), stopped=i32(B))


X = f32(2, 3, 4)
TABLE = f64(7)
BANK = dict(bank=f32(20), bank_off=i32(3))
SIG, TAPS = f32(2, 40), f32(8, 64)
FRAMING = dict(L=48, frame=16, hop=8)
PAR = f64(12)
PLANE = f32(5, 129)
CF = rc.center_freqs("default")
RESYNTH = dict(frame=160, hop=80, n_fft=256, fs=8000, cf=CF)
WIN, DFT = f32(256), f32(256, 432)
STOI_TABLES = dict(sig_off=i32(2), frame_off=i32(3), src=i32(4), kept=i32(2), tiles=i32(1, 2))
STOI_TAIL = dict(sum_frames=4, spec_rows=4, n_samples=600)
XB = f32(4, 15)
SEG = dict(frame_off=i32(3), kept=i32(2), B=2, extended=False, spec_rows=4, segments=1)
QMAX = ops.QUANT_MAX_STEPS

# (id, wrapper, launches, the valid call, {operand: defect letters}, [(label, {argument: value})])
TABLE_OF_CONTRACTS = [
    ("pstoi_loss", "pstoi_loss", 1, dict(enh=f32(2, 4, 32), clean=f32(2, 4, 32), band_w=f32(3, 4), frame_len=30),
     {"enh": "-+n", "clean": "f-+n", "band_w": "-+n"},
     [("bins", dict(band_w=f32(3, 5))), ("bands", dict(band_w=f32(ops.PSTOI_MAX_BANDS + 1, 4))),
      ("frame_len_low", dict(frame_len=ops.PSTOI_MIN_FRAME_LEN - 1)), ("frame_len_high", dict(frame_len=ops.PSTOI_MAX_FRAME_LEN + 1)),
      ("frames_short", dict(frame_len=33))]),
    ("mse_loss", "mse_loss", 1, dict(pred=f32(2, 3), target=f32(2, 3)), {"pred": "n", "target": "f-+n"},
     [("empty", dict(pred=f32(0, 3), target=f32(0, 3)))]),
    ("mask_irm", "mask_irm", 1, dict(clean_mag=X, noise_mag=X), {"clean_mag": "dcn", "noise_mag": "dcf-+n"}, []),
    ("mask_corr", "mask_corr", 1, dict(noisy=X, clean=X, noise=X), {"noisy": "dcn", "clean": "dcf-+n", "noise": "dcf-+n"}, []),
    ("mask_pcirm", "mask_pcirm", 1, dict(clean_mag=X, noise_mag=X, rho_s=X, rho_n=X, phi1=X, phi2=X),
     {"clean_mag": "dcn", "noise_mag": "dcf-+n", "rho_s": "dcf-+n", "rho_n": "dcf-+n", "phi1": "dcf-+n", "phi2": "dcf-+n"}, []),
    ("mask_quantize", "mask_quantize", 1, dict(pcirm=X, table=TABLE, M=3), {"pcirm": "dcn", "table": "dfn"},
     [("table_fp32", dict(table=f32(7))), ("M_low", dict(M=1, table=f64(3))), ("M_high", dict(M=QMAX + 1, table=f64(2 * QMAX + 3))),
      ("empty", dict(pcirm=f32(0, 3)))]),
    ("mix_scale", "mix_scale", 1, dict(clean=f32(2, 8), noise_ids=i32(2), snr_db=f32(2), lengths=i32(2), **BANK),
     {"clean": "d-+n", "bank": "dn", "bank_off": "dn", "noise_ids": "dfn", "snr_db": "dfn", "lengths": "df"},
     [("bank_off_short", dict(bank_off=i32(1)))]),
    ("mix_apply", "mix_apply", 1, dict(clean=f32(2, 8), noise_ids=i32(2), scale=f32(2), lengths=i32(2), want_rows=True, **BANK),
     {"clean": "d-+n", "bank": "dn", "bank_off": "dn", "noise_ids": "dfn", "scale": "dfn", "lengths": "df"},
     [("bank_off_short", dict(bank_off=i32(1)))]),
    ("mix_scale_varlen", "mix_scale_varlen", 1, dict(packed=f32(16), utt_off=i32(3), noise_ids=i32(2), snr_db=f32(2), max_len=8, **BANK),
     {"packed": "dc-+n", "utt_off": "dcf+n", "bank": "dn", "bank_off": "dn", "noise_ids": "dcfn", "snr_db": "dcfn"},
     [("packed_empty", dict(packed=f32(0))), ("utt_off_short", dict(utt_off=i32(1))), ("bank_off_short", dict(bank_off=i32(1)))]),
    ("wave_batch", "wave_batch", 1,
     dict(packed=f32(16), utt_off=i32(3), noise_ids=i32(2), scale=f32(2), index=i32(2), L_out=8, out=f32(2, 2, 8), **BANK),
     {"packed": "dc-+n", "utt_off": "dcf+n", "bank": "dn", "bank_off": "dn", "noise_ids": "dcfn", "scale": "dcfn", "index": "dcf-+n",
      "out": "dcf-+"},
     [("index_empty", dict(index=i32(0), out=f32(2, 0, 8)))]),
    ("curriculum_mask", "curriculum_mask", 1, dict(cr=X, ci=X, nr=X, ni=X, scale=f32(2), kind="opt_pcirm", table=TABLE, M=3),
     {"cr": "dc-+n", "ci": "dcf-+n", "nr": "dcf-+n", "ni": "dcf-+n", "scale": "dfn", "table": "fn"},
     [("cr_2d", dict(cr=f32(2, 12))), ("all_2d", dict(cr=f32(2, 12), ci=f32(2, 12), nr=f32(2, 12), ni=f32(2, 12)))]),
    ("pso_frame_coef", "pso_frame_coef", 1, dict(pcirm=X, table=TABLE, M=3), {"pcirm": "dc-+n", "table": "dcfn"},
     [("M_low", dict(M=1, table=f64(3))), ("M_high", dict(M=QMAX + 1, table=f64(2 * QMAX + 3))), ("empty", dict(pcirm=f32(2, 0, 4)))]),
    ("pso_split", "pso_split", 1,
     dict(noisy=f32(2, 8), clean=f32(2, 8), lengths=i32(2), samp_off=i32(3), a=f64(2, 3), b=f64(2, 3), sum_L=16, frame=4, hop=2),
     {"noisy": "dc-+n", "clean": "dcfn", "lengths": "dcfn", "samp_off": "dcfn", "a": "dcfn", "b": "dcfn"},
     [("noisy_1d", dict(noisy=f32(16))), ("hop_low", dict(hop=0)), ("hop_high", dict(hop=5)),
      ("no_samples", dict(noisy=f32(2, 0), clean=f32(2, 0)))]),
    ("pso_fitness", "pso_fitness", 1,
     dict(spectra=tuple(f32(6, 5) for _ in range(6)), frame_off=i32(3), lengths=i32(2), S=f64(2, 4), pos=f64(2, 3), stopped=i32(2),
          partial=f64(2, 2, 3), sum_frames=6),
     {"frame_off": "dcfn", "lengths": "dcfn", "S": "dcfn", "pos": "dc-+n", "stopped": "dcfn", "partial": "dcfn"},
     [("pos_1d", dict(pos=f64(6))), ("partial_2d", dict(partial=f64(2, 3))), ("partial_1d", dict(partial=f64(12))),
      ("five_spectra", dict(spectra=tuple(f32(6, 5) for _ in range(5)))),
      ("spectrum_dtype", dict(spectra=tuple(f32(6, 5) for _ in range(5)) + (f64(6, 5),))),
      ("spectrum_noncontiguous", dict(spectra=(DEFECT["c"](f32(6, 5)),) + tuple(f32(6, 5) for _ in range(5)))),
      ("spectrum_one_fewer", dict(spectra=tuple(f32(6, 5) for _ in range(5)) + (f32(5, 5),))),
      ("spectrum_0d", dict(spectra=tuple(f32(()) for _ in range(6)), sum_frames=0)),
      ("sum_frames_high", dict(sum_frames=7)),
      ("bins_high", dict(spectra=tuple(f32(6, ops.PSO_MAX_BINS + 1) for _ in range(6)))),
      ("particles_high", dict(pos=f64(2, ops.PSO_MAX_PARTICLES + 1), partial=f64(2, 2, ops.PSO_MAX_PARTICLES + 1))),
      ("particles_low", dict(pos=f64(2, 0), partial=f64(2, 2, 0))), ("bins_low", dict(spectra=tuple(f32(6, 0) for _ in range(6))))]),
    ("pso_step_fitness", "pso_step", 1, dict(state=swarm(), it=1, fitness=f64(2, 3)),
     {"state.draws": "dcfn", "state.params": "dcfn", "state.pos": "dcfn", "state.vel": "dcfn", "state.pbest_pos": "dcfn",
      "state.pbest_fit": "dcfn", "state.gbest": "dcfn", "state.hist": "dcfn", "state.iters": "dcfn", "state.stopped": "dcfn",
      "fitness": "dcf"},
     [("it_low", dict(it=-1)), ("it_high", dict(it=3)), ("neither", dict(fitness=None)),
      ("both", dict(partial=f64(2, 2, 3), frame_off=i32(3))),
      ("rounds_low", dict(state=swarm(K=0), it=0))]),
    ("pso_step_partial", "pso_step", 1, dict(state=swarm(), it=0, partial=f64(2, 2, 3), frame_off=i32(3)),
     {"partial": "dcf", "frame_off": "dcfn"}, [("partial_1d", dict(partial=f64(12)))]),
    ("pso_quantize", "pso_quantize", 1, dict(pcirm=X, table=TABLE, middle=f64(2), M=3),
     {"pcirm": "dcn", "table": "dcfn", "middle": "dcfn"},
     [("M_low", dict(M=1, table=f64(3))), ("M_high", dict(M=QMAX + 1, table=f64(2 * QMAX + 3))), ("pcirm_0d", dict(pcirm=f32(())))]),
    ("gammatone_fir", "gammatone_fir", 1, dict(sig=SIG, taps=TAPS, C=4, lengths=i32(2)),
     {"sig": "dc-+n", "taps": "dcf-+n", "lengths": "dcf"},
     [("C_low", dict(C=0)), ("C_high", dict(C=ops.GT_COLS + 1)), ("taps_low", dict(taps=f32(0, 64))),
      ("taps_high", dict(taps=f32(ops.GT_MAX_TAPS + 8, 64))), ("taps_columns", dict(taps=f32(8, 63))),
      ("taps_not_in_eights", dict(taps=f32(12, 64))), ("utterances_high", dict(sig=f32(65536, 1), lengths=i32(65536)))]),
    ("gammatone_tf", "gammatone_tf", 1, dict(sig=SIG, taps=TAPS, tw=f32(2, 8, 64), C=4, hop=8, lengths=i32(2)),
     {"sig": "dc-+n", "taps": "dcf-+n", "tw": "dcf-+n", "lengths": "dcf"},
     [("C_low", dict(C=0)), ("C_high", dict(C=ops.GT_COLS + 1)), ("hop_low", dict(hop=0, tw=f32(2, 0, 64))),
      ("hop_high", dict(hop=41, tw=f32(2, 41, 64))),
      ("taps_low", dict(taps=f32(0, 64))), ("taps_high", dict(taps=f32(ops.GT_MAX_TAPS + 8, 64))), ("taps_not_in_eights", dict(taps=f32(12, 64))),
      ("utterances_high", dict(sig=f32(65536, 8), lengths=i32(65536)))]),
    ("gammatone_moments", "gammatone_moments", 1,
     dict(y=f32(2, 4, 40), tw=f32(2, 8, 64), T=3, w=8, frame=16, hop=8, lengths=i32(2)),
     {"y": "dc-+n", "tw": "dcf-+n", "lengths": "dcf"},
     [("T_low", dict(T=0)), ("T_high", dict(T=5)), ("w_low", dict(w=0, tw=f32(2, 0, 64))), ("w_high", dict(w=17, tw=f32(2, 17, 64))),
      ("hop_low", dict(hop=0)), ("channels_high", dict(y=f32(2, ops.GT_COLS + 1, 40))),
      ("frame_low", dict(frame=7)), ("utterances_high", dict(y=f32(65536, 1, 40), lengths=i32(65536)))]),
    ("gammatone_tf_finish", "gammatone_tf_finish", 1,
     dict(partial=f32(2, 5, 4, 5), rot=f32(2, 64), T=4, L=48, frame=16, hop=8, N=16, two=True, lengths=i32(2)),
     {"partial": "dcf-+n", "rot": "dcf-+n", "lengths": "dcf"},
     [("T_low", dict(T=0)), ("T_high", dict(T=5)), ("N_low", dict(N=0)), ("N_odd", dict(N=3)), ("frame_low", dict(frame=0)),
      ("hop_low", dict(hop=0)), ("L_low", dict(L=15)), ("sums", dict(partial=f32(2, 5, 4, 4))),
      ("channels_high", dict(partial=f32(2, 5, ops.GT_COLS + 1, 5))), ("utterances_high", dict(partial=f32(65536, 5, 1, 5), lengths=i32(65536))),
      ("frames_high", dict(T=6, partial=f32(2, 7, 4, 5)))]),
    ("cepstral_spectrum", "cepstral", 1,
     dict(src=f32(2, 3, 16), fb=f32(3, 4), dct=f32(2, 3), out=f32(2, 3, 6), col_off=1, B=2, T=3, in_mode=ops.CEP_POWER, F=4,
          compress=ops.CEP_LOG, im_off=8, lengths=i32(2), **FRAMING),
     {"src": "df-+n", "fb": "dcf-+", "dct": "dc-+", "out": "dcf-+n", "lengths": "dcf"},
     [("src_last_stride", dict(src=f32(2, 3, 32)[:, :, ::2])), ("col_off_low", dict(col_off=-1)), ("col_off_high", dict(col_off=5)),
      ("frame_low", dict(frame=0)), ("hop_low", dict(hop=0)), ("L_low", dict(L=15)), ("in_mode", dict(in_mode=99)),
      ("im_off_low", dict(im_off=3)), ("im_off_high", dict(im_off=13)), ("F_low", dict(F=0, fb=f32(3, 0))),
      ("F_high", dict(F=ops.FE_MAX_BINS + 1, im_off=ops.FE_MAX_BINS + 1, src=f32(2, 3, 2 * ops.FE_MAX_BINS + 2), fb=f32(3, ops.FE_MAX_BINS + 1))),
      ("filters_high", dict(fb=f32(ops.FE_MAX_FILTERS + 1, 4), dct=f32(2, ops.FE_MAX_FILTERS + 1))),
      ("coefficients_high", dict(dct=f32(ops.FE_MAX_COEFFS + 1, 3), out=f32(2, 3, ops.FE_MAX_COEFFS + 2))),
      ("T_high", dict(T=6, src=f32(2, 6, 16), out=f32(2, 6, 6))), ("T_low", dict(T=0, src=f32(2, 0, 16), out=f32(2, 0, 6))),
      ("B_low", dict(B=0, src=f32(0, 3, 16), out=f32(0, 3, 6), lengths=i32(0)))]),
    ("cepstral_blocks", "cepstral", 1,
     dict(src=f32(2, 8, 4, 5), fb=None, dct=f32(2, 4), out=f32(2, 3, 6), col_off=1, B=2, T=3, in_mode=ops.CEP_BLOCKS, F=4,
          compress=ops.CEP_CBRT, bmul=2, badd=1, window=8.0, **FRAMING),
     {"src": "dcf-+n"},
     [("bmul_low", dict(bmul=0)), ("badd_low", dict(badd=-1)), ("badd_high", dict(badd=3)), ("window_low", dict(window=0.0)),
      ("channels_high", dict(F=65, src=f32(2, 8, 65, 5), fb=f32(4, 65), dct=f32(2, 4)))]),
    ("rasta", "rasta", 1, dict(logb=f32(2, 3, 5), eql=f64(5), dct=f64(2, 5), out=f32(2, 3, 6), col_off=1, lengths=i32(2), **FRAMING),
     {"logb": "dc-+n", "eql": "dcf-+n", "dct": "dc-+n", "out": "dcf-+n", "lengths": "dcf"},
     [("col_off_low", dict(col_off=-1)), ("col_off_high", dict(col_off=5)), ("frame_low", dict(frame=0)), ("hop_low", dict(hop=0)),
      ("L_low", dict(L=15)), ("dct_columns", dict(dct=f64(2, 4))), ("no_coefficients", dict(dct=f64(0, 5))),
      ("filters_high", dict(logb=f32(2, 3, ops.FE_MAX_FILTERS + 1), eql=f64(ops.FE_MAX_FILTERS + 1), dct=f64(2, ops.FE_MAX_FILTERS + 1))),
      ("coefficients_high", dict(dct=f64(ops.FE_MAX_COEFFS + 1, 5), out=f32(2, 3, ops.FE_MAX_COEFFS + 2))), ("T_high", dict(logb=f32(2, 6, 5), out=f32(2, 6, 6))),
      ("T_low", dict(logb=f32(2, 0, 5), out=f32(2, 0, 6)))]),
    ("feature_context", "feature_context", 1,
     dict(feat=X, ctx=1, mean=f32(12), std=f32(12), clip=10.0, lengths=i32(2), **FRAMING),
     {"feat": "dc-+n", "mean": "dcf+n", "std": "dcf+n", "lengths": "dcf"},
     [("ctx_low", dict(ctx=-1)), ("ctx_high", dict(ctx=65, mean=f32(524), std=f32(524))), ("clip_low", dict(clip=0.0)),
      ("odd_columns", dict(feat=f32(2, 3, 5), mean=f32(15), std=f32(15))), ("frame_low", dict(frame=0)), ("L_low", dict(L=15)),
      ("hop_low", dict(hop=0)), ("T_high", dict(feat=f32(2, 6, 4)))]),
    ("rows_mean", "rows_mean", 1, dict(src=f32(2, 3, 6), col_off=1, N=2, den=0, lengths=i32(2), **FRAMING),
     {"src": "dc-+n", "lengths": "dcf"},
     [("N_low", dict(N=0)), ("col_off_low", dict(col_off=-1)), ("col_off_high", dict(col_off=5)), ("den_low", dict(den=-1)),
      ("hop_low", dict(hop=0)),
      ("frame_low", dict(frame=0)), ("L_low", dict(L=15)), ("T_high", dict(src=f32(2, 6, 6)))]),
    ("haircell", "haircell", 1, dict(x=f32(3, 8), par=PAR), {"x": "dc-+n", "par": "dcf-+n"}, [("empty", dict(x=f32(0, 8)))]),
    ("haircell_frames", "haircell_frames", 1, dict(x=f32(2, 3, 40), par=PAR, frame=16, hop=8, lengths=i32(2)),
     {"x": "dc-+n", "par": "dcf-+n", "lengths": "dcf"},
     [("frame_low", dict(frame=0)), ("frame_high", dict(frame=17)), ("hop_low", dict(hop=0)), ("short", dict(x=f32(2, 3, 15)))]),
    ("csii_frames_varlen", "csii_frames_varlen", 1,
     dict(cr=PLANE, ci=PLANE, er=PLANE, ei=PLANE, frame_off=i32(3), weights=f64(129), B=2, want_msc=True),
     {"cr": "dc-+n", "ci": "dcf-+n", "er": "dcf-+n", "ei": "dcf-+n", "frame_off": "fn", "weights": "dfn"},
     [("bins", dict(cr=f32(5, 128), ci=f32(5, 128), er=f32(5, 128), ei=f32(5, 128)))]),
    ("hilbert_env", "hilbert_env", 1, dict(x=f32(2, 8)), {"x": "dc-+n"}, [("empty", dict(x=f32(0, 8)))]),
    ("hilbert_env_moments", "hilbert_env_moments", 1,
     dict(X=f32(2, 2, 3, 8), tables=f32(32), tab_off=i32(2), lengths=i32(2), tiles=i32(2, 2), C=3),
     {"X": "dc-+n", "tab_off": "fn", "lengths": "fn", "tiles": "-+n"},
     [("tiles_columns", dict(tiles=i32(2, 3))), ("C", dict(C=2)), ("one_plane", dict(X=f32(1, 2, 3, 8)))]),
    ("ncm_finish", "ncm_finish", 1, dict(partial=f64(2, 3, 5), tile_off=i32(3), lengths=i32(2), weights=f64(3), B=2, C=3),
     {"partial": "n", "tile_off": "fn", "lengths": "fn", "weights": "dfn"}, []),
    ("dnn_layer_rows16", "dnn_layer", 1, dict(a=f16(3, 24), pw=pack(4, 24), act="relu", out=f16(3, 8)),
     {"a": "d-+n", "out": "df-+"},
     [("a_last_stride", dict(a=f16(3, 48)[:, ::2])), ("a_columns", dict(a=f16(3, 16))), ("a_row_stride", dict(a=f16(3, 28)[:, :24])),
      ("a_empty", dict(a=f16(0, 24), out=f16(0, 8))), ("out_columns", dict(out=f16(3, 3))), ("out_fp32_columns", dict(out=f32(3, 5))),
      ("out_last_stride", dict(out=f16(3, 16)[:, ::2])), ("act", dict(act="tanh")), ("frames", dict(frames=i32(3))),
      ("mean", dict(mean=f32(24), std=f32(24)))]),
    ("dnn_layer_rows32", "dnn_layer", 1, dict(a=f32(3, 24), pw=pack(4, 24), out_dtype=F32), {"a": "d-+n"},
     [("a_columns_low", dict(a=f32(3, 23))), ("a_columns_high", dict(a=f32(3, 25)))]),
    ("dnn_layer_context", "dnn_layer", 1,
     dict(a=f32(2, 3, 8), pw=pack(4, 24), context=1, frames=i32(2), mean=f32(24), std=f32(24)),
     {"a": "dc-+n", "frames": "dcf", "mean": "dcfn", "std": "dcfn"},
     [("a_odd_columns", dict(a=f32(2, 3, 9), pw=pack(4, 27), mean=f32(27), std=f32(27))),
      ("a_few_columns", dict(a=f32(2, 3, 6), pw=pack(4, 18), mean=f32(18), std=f32(18))),
      ("context_low", dict(context=-1)), ("context_high", dict(context=65, pw=pack(4, 8 * 131), mean=None, std=None)),
      ("K", dict(pw=pack(4, 16), mean=f32(16), std=f32(16))),
      ("statistics_K_high", dict(a=f32(2, 3, 32), context=64, pw=pack(4, 4128), mean=f32(4128), std=f32(4128)))]),
    ("dnn_act_bwd", "dnn_act_bwd", 1, dict(dy=f32(3, 4), saved=f16(3, 4), act="relu", N=4, out=f16(3, 64)),
     {"dy": "d-+n", "saved": "df-+n", "out": "dcf-+"},
     [("dy_1d", dict(dy=f32(12))), ("dy_last_stride", dict(dy=f32(3, 8)[:, ::2])), ("N_high", dict(N=5)), ("act", dict(act="tanh")),
      ("saved_sigmoid_dtype", dict(act="sigmoid")), ("out_columns", dict(out=f16(3, 12))), ("dy_empty", dict(dy=f32(0, 4), saved=f16(0, 4), out=f16(0, 64)))]),
    ("context_moments", "context_moments", 1, dict(raw=f32(5, 8), bounds=i32(5, 2), ctx=1), {"raw": "dc-+n", "bounds": "dcf-+n"},
     [("ctx_low", dict(ctx=-1)), ("ctx_high", dict(ctx=65))]),
    ("dnn_layer_indexed", "dnn_layer_indexed", 1,
     dict(raw=f32(5, 8), bounds=i32(5, 2), index=i32(3), pw=pack(4, 24), context=1, mean=f32(24), std=f32(24), a16_out=f16(3, 64),
          out=f16(3, 8)),
     {"raw": "dc-+n", "bounds": "dcf-+n", "index": "dc-+n", "mean": "dcfn", "std": "dcfn", "a16_out": "dcf-+", "out": "df-+"},
     [("index_empty", dict(index=i32(0), a16_out=f16(0, 64), out=f16(0, 8))), ("context_low", dict(context=-1)),
      ("raw_odd_columns", dict(raw=f32(5, 9), pw=pack(4, 27), mean=f32(27), std=f32(27))), ("act", dict(act="tanh")),
      ("out_columns", dict(out=f16(3, 3))),
      ("context_high", dict(context=65, pw=pack(4, 8 * 131), mean=None, std=None, a16_out=None)),
      ("raw_few_columns", dict(raw=f32(5, 6), pw=pack(4, 18), mean=f32(18), std=f32(18))),
      ("statistics_K_high", dict(raw=f32(5, 32), context=64, pw=pack(4, 4128), mean=f32(4128), std=f32(4128), a16_out=None)),
      ("out_dtype", dict(out=None, out_dtype=F64))]),
    ("mse_gather_loss", "mse_gather_loss", 1,
     dict(y=f32(3, 4), mask=f32(5, 4), index=i32(3), loss_scale=f32(1), rec=f64(4), ctl=f64(8), dz=f16(3, 64)),
     {"y": "dc-+n", "mask": "dc-+n", "index": "dcf-+n", "loss_scale": "d", "rec": "dcf", "ctl": "dcf", "dz": "dcf-+"},
     [("mask_columns", dict(mask=f32(5, 3))), ("mask_empty", dict(mask=f32(0, 4))), ("loss_scale_empty", dict(loss_scale=f32(0)))]),
    ("mask_resynth", "mask_resynth", 1, dict(noisy=f32(2, 400), mask=f32(2, 3, 64), lengths=i32(2), out=f32(2, 400), **RESYNTH),
     {"noisy": "dc-+n", "mask": "dcf-+n", "lengths": "dcf", "out": "dcf-+"}, [("channels", dict(mask=f32(2, 3, 63))),
      ("framing", dict(hop=81))]),
    ("mask_resynth_bwd", "mask_resynth_bwd", 1,
     dict(noisy=f32(2, 400), dout=f32(2, 400), lengths=i32(2), T_mask=3, out=f32(2, 3, 64), **RESYNTH),
     {"noisy": "dc-+n", "dout": "dcf-+n", "lengths": "dcf", "out": "dcf-+"}, [("T_mask_low", dict(T_mask=0, out=None)),
      ("framing", dict(hop=81))]),
    ("rbm_prob_rows", "rbm_prob", 1, dict(data=f32(5, 4), W=f32(4, 3), bias=f32(3), rows=i32(2), u=f64(2, 3), prob=f32(2, 3)),
     {"data": "d-+n", "W": "dc-+n", "bias": "dcfn", "rows": "dc+", "u": "dcf", "prob": "dcf"},
     [("data_columns", dict(data=f32(5, 3))), ("data_last_stride", dict(data=f32(5, 8)[:, ::2])), ("two_sources", dict(seed=1)),
      ("units_high", dict(W=f32(4, ops.RBM_MAX_UNITS + 1), bias=f32(ops.RBM_MAX_UNITS + 1), u=None, prob=None)),
      ("sample_size", dict(sample=f32(2, 2))),
      ("units_low", dict(W=f32(0, 3), data=f32(5, 0))), ("hidden_low", dict(W=f32(4, 0), bias=f32(0), u=f64(2, 0), prob=f32(2, 0))),
      ("data_row_stride", dict(data=f32(4).expand(5, 4)))]),
    ("rbm_prob_first_rows", "rbm_prob", 1, dict(data=f32(5, 3), W=f32(4, 3), bias=f32(4), down=True, M=5),
     {}, [("M_high", dict(M=6)), ("M_low", dict(M=0)), ("data_empty", dict(data=f32(0, 3), M=None))]),
    ("rbm_update", "rbm_update", 1,
     dict(data=f32(5, 4), ph=f32(2, 3), nv=f32(2, 4), nh=f32(2, 3), W=f32(4, 3), v_bias=f32(4), h_bias=f32(3), err_partial=f64(1),
          lr=0.1, rows=i32(2)),
     {"data": "d-+n", "ph": "dcf-+n", "nv": "dcf-+n", "nh": "dcf-+n", "W": "dc-+n", "v_bias": "dcfn", "h_bias": "dcfn",
      "err_partial": "dfn", "rows": "dc+"},
     [("batch_high", dict(B=ops.RBM_MAX_BATCH + 1, rows=None)), ("batch_low", dict(B=0, rows=None)),
      ("units_low", dict(W=f32(0, 3), data=f32(5, 0), nv=f32(2, 0), v_bias=f32(0))),
      ("units_high", dict(W=f32(4, ops.RBM_MAX_UNITS + 1), ph=f32(2, ops.RBM_MAX_UNITS + 1), nh=f32(2, ops.RBM_MAX_UNITS + 1),
                          h_bias=f32(ops.RBM_MAX_UNITS + 1))),
      ("data_row_stride", dict(data=f32(4).expand(5, 4)))]),
    ("rbm_fold_error", "rbm_fold_error", 1, dict(partial=f64(2, 1), out=f64(1), n_steps=2, num_samples=4, batch_size=2, n_visible=4),
     {"partial": "dcfn", "out": "dfn"}, [("n_steps", dict(n_steps=1))]),
    ("stoi_resample", "stoi_resample", 1,
     dict(sig=f32(20), taps=f32(3, 5), in_off=i32(2), in_len=i32(2), out_off=i32(2), out_len=i32(2), B=2, n_out=10, max_out_len=5,
          n_in=20, up=5, down=8, padl=1, out=f32(10)),
     {"sig": "dcn", "taps": "dc-+n", "in_off": "dcfn", "in_len": "dcfn", "out_off": "dcfn", "out_len": "dcfn", "out": "dcf"},
     [("taps_columns", dict(taps=f32(3, 4)))]),
    ("stoi_keep", "stoi_keep", 1,
     dict(sig=f32(600), win=WIN, sig_off=i32(2), sig_len=i32(2), frame_off=i32(3), B=2, sum_frames=4, n_samples=600),
     {"sig": "dcn", "win": "dfn", "sig_off": "dcfn", "sig_len": "dcfn", "frame_off": "dcfn"}, []),
    ("stoi_bands", "stoi_bands", 1, dict(sigs=(f32(600), f32(600)), win=WIN, dft=DFT, **STOI_TABLES, **STOI_TAIL),
     {"win": "fn", "dft": "dcf-+n", "sig_off": "dcn", "frame_off": "dcn", "src": "dcfn", "kept": "dcn", "tiles": "dc-+n"},
     [("tiles_columns", dict(tiles=i32(1, 3))), ("no_signal", dict(sigs=())), ("three_signals", dict(sigs=(f32(600),) * 3)),
      ("signal_dtype", dict(sigs=(f32(600), f64(600)))), ("signal_noncontiguous", dict(sigs=(DEFECT["c"](f32(600)),))),
      ("signal_none", dict(sigs=(None,)))]),
    ("stoi_segments", "stoi_segments", 1, dict(xb=XB, yb=XB, **SEG),
     {"xb": "dc-+n", "yb": "dcf-+n", "frame_off": "dcfn", "kept": "dcfn"}, [("bands", dict(xb=f32(4, 14), yb=f32(4, 14)))]),
    ("stoi_bands_pair", "stoi_bands_pair", 1, dict(ya=f32(600), yb=f32(600), win=WIN, dft=DFT, **STOI_TABLES, **STOI_TAIL),
     {"ya": "dc-+n", "yb": "dcf-+n", "win": "dfn", "dft": "dcf-+n", "sig_off": "dcn", "frame_off": "dcn", "src": "dcfn", "kept": "dcn",
      "tiles": "dc-+n"},
     [("tiles_columns", dict(tiles=i32(1, 3)))]),
    ("pso_fitness_taal", "pso_fitness_taal", 1,
     dict(xb=XB, planes=f64(4, 3, 15), frame_off=i32(3), kept=i32(2), pos=f64(2, 3), stopped=i32(2), fitness=f64(2, 3), extended=False,
          spec_rows=4, segments=1),
     {"xb": "dc-+n", "planes": "dcf-+n", "frame_off": "dcfn", "kept": "dcfn", "pos": "dc-+n", "stopped": "dcfn", "fitness": "dcf-+n"},
     [("particles_high", dict(pos=f64(2, ops.PSO_MAX_PARTICLES + 1), fitness=f64(2, ops.PSO_MAX_PARTICLES + 1))),
      ("no_rows", dict(xb=f32(0, 15), planes=f64(0, 3, 15)))]),
    ("stoi_segments_bwd", "stoi_segments_bwd", 1,
     dict(xb=XB, yb=XB, frame_off=i32(3), kept=i32(2), gscore=f64(2), B=2, max_rows=4, extended=True, spec_rows=4, segments=1),
     {"xb": "dc-+n", "yb": "dcf-+n", "frame_off": "dcfn", "kept": "dcfn", "gscore": "dcfn"},
     [("max_rows_low", dict(max_rows=-1)), ("max_rows_high", dict(max_rows=5))]),
    ("stoi_bands_bwd", "stoi_bands_bwd", 1,
     dict(sig=f32(600), win=WIN, dft=DFT, dft_t=f32(432, 256), dyb=XB, **STOI_TABLES, **STOI_TAIL),
     {"sig": "dcn", "win": "dfn", "dft": "dcf-+n", "dft_t": "dcf-+n", "sig_off": "dcn", "frame_off": "dcn", "src": "dcfn", "kept": "dcn",
      "tiles": "dc-+n", "dyb": "dcf-+n"},
     [("tiles_columns", dict(tiles=i32(1, 3)))]),
    ("stoi_fold_bwd", "stoi_fold_bwd", 1,
     dict(dframes=f32(4, 256), win=WIN, sig_off=i32(2), sig_len=i32(2), frame_off=i32(3), src=i32(4), kept=i32(2), B=2, n_out=600,
          max_len=300, pad_to=0, sum_frames=4),
     {"dframes": "dcf-+n", "win": "dfn", "sig_off": "dcfn", "sig_len": "dcfn", "frame_off": "dcfn", "src": "dcfn", "kept": "dcfn"},
     [("pad_to_low", dict(pad_to=-1)), ("pad_to_high", dict(pad_to=301))]),
]

CASES = {c[0]: c for c in TABLE_OF_CONTRACTS}
DEFECTS = [(c[0], "%s_%s" % (k, NAMES[d])) for c in TABLE_OF_CONTRACTS for k, ds in c[4].items() for d in ds] + \
          [(c[0], label) for c in TABLE_OF_CONTRACTS for label, _ in c[5]]


def with_arguments(call, changes):
    """a copy of `call` with `changes`; "state.pos" changes an attribute of a copy of call["state"]"""
    call = dict(call)
    for key, value in changes.items():
        if "." in key:
            obj, attr = key.split(".")
            call[obj] = copy.copy(call[obj])
            setattr(call[obj], attr, value)
        else:
            call[key] = value
    return call


def changes_of(case, label):
    for key, letters in case[4].items():
        for d in letters:
            if label == "%s_%s" % (key, NAMES[d]):
                t = case[3]
                for part in key.split("."):
                    t = t[part] if isinstance(t, dict) else getattr(t, part)
                return {key: DEFECT[d](t)}
    return dict(case[5])[label]


@pytest.fixture
def launches(monkeypatch):
    ops.set_compute_dtype(F16)
    return ops_stub.install(monkeypatch)


@pytest.mark.parametrize("name", list(CASES))
def test_the_valid_call_launches(launches, name):
    _, wrapper, n, call, _, _ = CASES[name]
    getattr(ops, wrapper)(**call)
    assert len(launches) == n, launches


@pytest.mark.parametrize("name,label", DEFECTS, ids=["%s-%s" % d for d in DEFECTS])
def test_a_defect_is_refused_before_any_launch(launches, name, label):
    case = CASES[name]
    call = with_arguments(case[3], changes_of(case, label))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        getattr(ops, case[1])(**call)
    assert launches == []


def test_a_sample_plane_without_a_source_is_a_bad_argument(launches):
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.rbm_prob(f32(5, 4), f32(4, 3), f32(3), sample=f32(5, 3))
    assert launches == []


def test_the_table_names_every_checking_wrapper():
    """a wrapper that refuses (calls _refuse) has a row here: a new contract comes with its row"""
    import inspect
    import re
    src = inspect.getsource(ops)
    refusing = set(re.findall(r'_refuse\("(\w+)"\)', src))
    assert refusing == {c[1] for c in TABLE_OF_CONTRACTS}
