"""Shared cases of the ragged EnhancementPath tests (tests/test_ragged_path_host.py, tests/test_ragged_path_gpu.py and
tools/ragged_path_bench.py): the length set, its signals and weights, the length chain restated from torch's own conv1d / stft
shapes, two wrong chains, and the assertions that tell them apart.  Test-side only."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import synth_sd
from sincformer_metacog_speech_enhancement_amd import synthetic as syn

FS = 16000
N_FFT, HOP, WIN = 256, 80, 160
# 2048 puts every conv layer's output on a tile edge (1024, 512, 256, 128 rows), 2047 and 2049 sit on either side; seven rows
# leave the second BiLSTM workgroup with three chains of different lengths; not sorted.  21 .. 53 STFT frames.
LENGTHS = [1600, 2047, 2048, 2049, 3200, 4177, 1601]
CHAIN_RANGE = range(129, 4301)              # every L of the host check
# (kernel, stride, padding) of the convs that shorten the rows (agents/perception.py:160-171), written out here: the reference
# of the chain is torch's conv1d on these, not the package's constant
CONVS = ((7, 2, 3), (7, 2, 3), (7, 2, 3), (5, 2, 2))


def states():
    """seeded weights of the three agents (the fixtures of tests/test_fullsize_properties_gpu.py)"""
    return {"pa": synth_sd("PerceptionAgent", 291, sinc_scale=2000.0), "cpea": synth_sd("CorrelationPhaseEstimationAgent", 292),
            "msa": synth_sd("MaskSynthesisAgent", 293)}


def waves(lengths=LENGTHS, seed=82):
    """one noisy signal per length: rows of synthetic.synth_wave cut to the lengths"""
    noisy, _ = syn.synth_wave(len(lengths), max(lengths), seed)
    return [np.ascontiguousarray(noisy[i, :n]) for i, n in enumerate(lengths)]


def padded(sigs, Lrow=None, fill=float("nan")):
    """[B, Lrow] float32 with row b = sigs[b] followed by `fill` (NaN: a sample read beyond a length poisons the result)"""
    Lrow = Lrow or max(s.size for s in sigs)
    out = np.full((len(sigs), Lrow), fill, dtype=np.float32)
    for b, s in enumerate(sigs):
        out[b, :s.size] = s
    return out


def conv_shape_chain(L):
    """[L, L1, L2, L3, Tpa] of one utterance from the shapes torch.nn.functional.conv1d gives (meta tensors: shapes only)"""
    x = torch.empty(1, 1, int(L), device="meta")
    rows = [int(L)]
    for k, s, p in CONVS:
        x = F.conv1d(x, torch.empty(1, 1, k, device="meta"), stride=s, padding=p)
        rows.append(int(x.shape[-1]))
    return rows


def stft_frames(L):
    """frames of the centred STFT (hop 80) of L samples, from torch.stft's own shape"""
    spec = torch.stft(torch.zeros(int(L)), N_FFT, HOP, WIN, window=torch.ones(WIN), center=True, pad_mode="reflect",
                      return_complex=True)
    return int(spec.shape[-1])


def check_chain(chain_fn, lengths=CHAIN_RANGE, batch=None):
    """the host file's assertions on a length chain `chain_fn(lengths) -> {"rows": [4 arrays], "Tpa", "T"}`: per utterance it equals
    conv1d's shapes, whatever other utterances share the call (`batch`: extra lengths appended to every call)."""
    extra = list(batch or [])
    Ls = list(lengths)
    got = chain_fn(Ls + extra)
    for i, L in enumerate(Ls):
        want = conv_shape_chain(L)
        have = [int(r[i]) for r in got["rows"]] + [int(got["Tpa"][i])]
        assert have == want, "L %d: chain %s, conv1d shapes %s" % (L, have, want)
        assert int(got["T"][i]) == 1 + L // HOP, "L %d: %d frames" % (L, int(got["T"][i]))


def mutant_off_by_one(chain_fn):
    """a chain that takes L // 2 at the second stride-2 layer: one row short whenever that layer's input row count is odd"""
    def fn(lengths):
        ch = chain_fn(lengths)
        rows = [np.array(r) for r in ch["rows"]]
        rows[2] = rows[1] // 2
        rows[3] = (rows[2] + 2 * 3 - 7) // 2 + 1
        return {"rows": rows, "Tpa": (rows[3] + 2 * 2 - 5) // 2 + 1, "T": ch["T"]}
    return fn


def mutant_tpa_from_lmax(chain_fn):
    """a chain whose Tpa is that of the LONGEST utterance of the call for every row (the padded batch's row count)"""
    def fn(lengths):
        ch = chain_fn(lengths)
        return {"rows": ch["rows"], "Tpa": np.full_like(np.asarray(ch["Tpa"]), int(np.max(ch["Tpa"]))), "T": ch["T"]}
    return fn
