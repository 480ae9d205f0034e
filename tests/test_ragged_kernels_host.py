"""CPU side of the ragged front-end kernel tests (tests/ragged_kernel_cases.py, tests/test_ragged_kernels_gpu.py):
  1. every float64 reference of the cases file against torch's own operator in float64, at the edge lengths of the GPU cases,
     so that a wrong reference cannot pass a wrong kernel;
  2. mutants of a kernel's result, built from the references: the shared comparison helpers must reject each one (and accept
     the result they were built from);
  3. the length tables: conv rows from conv1d's shapes, the sinc slot masks, the workgroup boundary 17408 from the restated
     launch rule, the headpool (Tin, Tout) pairs under the restated frames-per-tile rule.
No kernel runs here, and no wrong kernel exists anywhere: the mutants are arrays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ragged_kernel_cases as rk
from helpers import arr

F16, BF16 = torch.float16, torch.bfloat16


def close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    e = float((a - b).abs().max()) if a.numel() else 0.0
    assert e <= tol * max(1.0, float(b.abs().max()) if b.numel() else 1.0), e


# ---------------------------------------------------------------------------
# 1. the references against torch in float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", rk.SINC_A_TAPS)
def test_sinc_reference_is_a_direct_convolution(K):
    filt = rk.sinc_filters(K)
    x = rk.sinc_wave(1, 2053)[0]
    for L in rk.SINC_A["lengths"]:
        got = rk.sinc_ref64(x[:L], filt, None)
        want = F.conv1d(x[:L].double().view(1, 1, L), filt.double().unsqueeze(1), padding=K // 2)[0].t()
        close(got, want)
        direct = np.stack([np.correlate(np.pad(x[:L].double().numpy(), K // 2), filt[c].double().numpy(), "valid") for c in (0, 63)], 1)
        close(got[:, [0, 63]], torch.from_numpy(direct))
    # the operand roundings: the waveform once, the taps once after the 2^12 pre-scale (fp16 taps of 1e-6 would be subnormal)
    for dt in (F16, BF16):
        got = rk.sinc_ref64(x[:300], filt, dt)
        want = F.conv1d(x[:300].to(dt).double().view(1, 1, 300), ((filt * 4096).to(dt).double() / 4096).unsqueeze(1), padding=K // 2)[0].t()
        close(got, want)
        assert float((got - rk.sinc_ref64(x[:300], filt, None)).abs().max()) > 0


def test_sinc_reference_on_windows_is_the_full_reference_cut():
    c = rk.SINC_B
    filt = rk.sinc_filters(c["K"])
    x = rk.sinc_wave(1, 20000)[0]
    for L in (17409, 1, 700):
        rows = rk.sinc_windows(L, c["boundary"])
        close(rk.sinc_ref64(x[:L], filt, F16, rows), rk.sinc_ref64(x[:L], filt, F16)[rows], 0.0)
    rows = rk.sinc_windows(33000, c["boundary"])
    assert rows.numel() == 4 * rk.SINC_B_WINDOW and {0, 511, 16896, 17407, 17408, 17919, 32488, 32999} <= set(rows.tolist())
    assert rk.sinc_windows(17407, c["boundary"])[-1] == 17406 and rk.sinc_windows(1, c["boundary"]).tolist() == [0]


@pytest.mark.parametrize("form", rk.CONV_FORMS, ids=[rk.conv_form_id(f) for f in rk.CONV_FORMS])
def test_conv_reference_is_conv1d_of_the_normalised_operand(form):
    cin, N, k, s, p, nin, skip = form
    lins, louts, Lin, Lout = rk.conv_lengths(k, s, p)
    d = rk.conv_operands(form, len(lins), Lin)
    for b, lin in enumerate(lins):
        z = d["x1"][b, :lin].half().double() * d["sc1"][b].double() + d["sh1"][b].double()
        if nin == 2:
            z = z + d["x2"][b, :lin].half().double() * d["sc2"][b].double() + d["sh2"][b].double()
        xn = F.gelu(z).half().double().t().unsqueeze(0)                          # [1, cin, lin]
        want = F.conv1d(xn, d["w"].half().double(), d["b"].double(), stride=s, padding=p)[0].t()
        got, got_s = rk.conv_ref64(d, b, lin, form)
        assert got.shape[0] == louts[b]
        close(got, want)
        if skip:
            close(got_s, F.conv1d(xn, d["ws"].half().double(), d["bs"].double(), stride=2)[0].t())
        else:
            assert got_s is None


@pytest.mark.parametrize("G,C", rk.GN_SHAPES)
def test_groupnorm_reference_is_group_norm(G, C):
    rows_tab = rk.GN_SYNTH_ROWS
    part, p_tab, data = rk.gn_synth_partials(G, C, rows_tab, dtype=torch.float64)
    w, b = rk.gn_affine(C)
    for i, r in enumerate(rows_tab):
        assert bool(torch.isnan(part[i, p_tab[i]:]).all()) and bool(torch.isfinite(part[i, :p_tab[i]]).all())
        sc, sh, ts, th = rk.gn_finalize64(part[i, :p_tab[i]], r, w, b)
        want = F.group_norm(data[i].t().unsqueeze(0), G, w.double(), b.double(), eps=rk.GN_EPS)[0].t()
        close(data[i] * sc + sh, want, 1e-9)
        assert bool((ts > 0).all()) and bool((th > 0).all())
    assert max(p_tab) > 512 and 1 in rows_tab and 1 in p_tab
    # GELU rows of gn_apply
    x = arr("rk_gax", (7, C), 31)
    sc, sh = arr("rk_gas", (C,), 32) * 0.2 + 1.0, arr("rk_gah", (C,), 33) * 0.3
    close(rk.gn_apply_ref64(x.half(), sc, sh, F16), F.gelu(x.half().double() * sc.double() + sh.double()))


def test_headpool_reference_is_adaptive_avg_pool1d():
    d = rk.headpool_operands(1, 700)
    for Tin, Tout in rk.HP_PAIRS[:4] + [(700, 141)]:
        raw, pooled = rk.headpool_ref64(d["x"][0, :Tin].half(), d["w"], d["b"], Tout, F16)
        want_raw = d["x"][0, :Tin].half().double() @ d["w"].half().double().t() + d["b"].double()
        close(raw, want_raw)
        close(pooled, F.adaptive_avg_pool1d(want_raw.t().unsqueeze(0), Tout)[0].t())
    s0, s1 = rk.group_sums64(raw, 32)
    close(s0, raw.reshape(-1, 32, 16).sum((0, 2)))
    close(s1, (raw ** 2).reshape(-1, 32, 16).sum((0, 2)))


def test_lstm_reference_is_nn_lstm():
    H = rk.LSTM_H
    xg, whh = rk.lstm_operands(2, 21)
    lstm = torch.nn.LSTM(4 * H, H, batch_first=True, bidirectional=True).double()
    eye = torch.eye(4 * H, dtype=torch.float64)                # the input projection is the identity: xg is the projected input
    with torch.no_grad():
        for sfx, d in (("", 0), ("_reverse", 1)):
            getattr(lstm, "weight_ih_l0" + sfx).copy_(eye)
            getattr(lstm, "weight_hh_l0" + sfx).copy_(whh[d].double())
            getattr(lstm, "bias_ih_l0" + sfx).zero_()
            getattr(lstm, "bias_hh_l0" + sfx).zero_()
        for Tj in (1, 2, 3, 5, 21):
            wf = lstm(xg[:1, :Tj, 0].double())[0][0, :, :H]
            wr = lstm(xg[:1, :Tj, 1].double())[0][0, :, H:]
            got = rk.lstm_ref64(xg[0], whh, Tj, round16=False)
            close(got[:, :H], wf, 1e-12)
            close(got[:, H:], wr, 1e-12)
    # a walk cut short is the walk of the shorter chain (forward) / leaves the rows it never reached at zero
    cut = rk.lstm_chain64(xg[0, :, 0], whh[0], False, steps=3)
    assert torch.equal(cut[:3], rk.lstm_chain64(xg[0, :3, 0], whh[0], False)) and bool((cut[3:] == 0).all())
    # the fp16 recurrent operands move it by less than the bound the kernel is held to, and by more than nothing
    e = float((rk.lstm_ref64(xg[0], whh, 21) - rk.lstm_ref64(xg[0], whh, 21, round16=False)).abs().max())
    assert 0 < e < rk.LSTM_TOL


def test_gather_reference():
    src = arr("rk_gsrc", (3, 4, 7), 5)
    got = rk.gather_ref(src, [2, 1, 4], 5)
    assert got.shape == (7, 5) and torch.equal(got[2], src[1, 0, :5]) and torch.equal(got[3:], src[2, :, :5])


# ---------------------------------------------------------------------------
# 2. mutants of a kernel's result
# ---------------------------------------------------------------------------
def _perfect(alone, S, rest, extra_cols=0):
    """the result a correct ragged launch leaves in a NaN buffer [B, S, cols + extra_cols]"""
    cols = alone[0].shape[1]
    out = np.full((len(alone), S, cols + extra_cols), np.nan, dtype=np.float32)
    for b, a in enumerate(alone):
        out[b, :a.shape[0], :cols] = a
        if rest == "zero":
            out[b, a.shape[0]:, :cols] = 0.0
    return out


@pytest.fixture(scope="module")
def sinc_result():
    """case A at K 31 from the reference: rows alone, the buffer, the partial slots"""
    lengths, Lrow = rk.SINC_A["lengths"], rk.SINC_A["Lrow"]
    filt, x = rk.sinc_filters(31), rk.sinc_wave(len(lengths), Lrow)
    alone = [rk.sinc_ref64(x[b, :L], filt, F16).float().numpy() for b, L in enumerate(lengths)]
    parts = []
    for b, L in enumerate(lengths):
        p = np.zeros((rk.sinc_tiles(L), 8, 2), np.float32)
        p[rk.sinc_used(L).numpy()] = 1.0 + b
        parts.append(p)
    part = np.zeros((len(lengths), rk.sinc_tiles(Lrow), 8, 2), np.float32)
    for b, p in enumerate(parts):
        part[b, :p.shape[0]] = p
    return dict(lengths=lengths, alone=alone, out=_perfect(alone, Lrow, "nan"), parts=parts, part=part, x=x, filt=filt)


def test_helpers_accept_the_correct_result(sinc_result):
    r = sinc_result
    rk.check_rows("ok", r["out"], r["alone"], "nan")
    rk.check_slots("ok", r["part"], r["parts"], used=[rk.sinc_used(L) for L in r["lengths"]])
    rk.check_same("ok", r["out"], r["out"][:, :, :], r["lengths"])
    rk.check_rows("ok", _perfect(r["alone"], 2053, "zero", extra_cols=3), r["alone"], "zero", cols=64)


def test_mutant_one_row_stored_past_a_length(sinc_result):
    r = sinc_result
    for b in (0, 3, 8):                                       # lengths 1, 256, 2048
        bad = r["out"].copy()
        bad[b, r["lengths"][b]] = 0.25
        with pytest.raises(AssertionError, match="were written"):
            rk.check_rows("mutant", bad, r["alone"], "nan")
    bad = _perfect(r["alone"], 2053, "zero")
    bad[4, 257, 5] = 1e-3                                     # a zero row that is not zero
    with pytest.raises(AssertionError, match="not exact zeros"):
        rk.check_rows("mutant", bad, r["alone"], "zero")
    bad = _perfect(r["alone"], 2053, "zero", extra_cols=3)
    bad[2, 0, 65] = 0.0                                       # a column behind the row
    with pytest.raises(AssertionError, match="columns from 64 on"):
        rk.check_rows("mutant", bad, r["alone"], "zero", cols=64)


def test_mutant_one_sample_read_past_a_length(sinc_result):
    """the FIR of a NaN-padded row that stages one sample beyond its length: the NaN reaches the last K // 2 outputs"""
    r = sinc_result
    b, L = 4, r["lengths"][4]
    xb = torch.cat([r["x"][b, :L], torch.tensor([float("nan")])])
    leaked = rk.sinc_ref64(xb, r["filt"], F16)[:L].float().numpy()
    assert np.isnan(leaked[L - 15:]).all() and np.isfinite(leaked[:L - 15]).all()
    bad = r["out"].copy()
    bad[b, :L] = leaked
    with pytest.raises(AssertionError, match="not finite"):
        rk.check_rows("mutant", bad, r["alone"], "nan")
    with pytest.raises(AssertionError):
        rk.check_ref("host-mutant", "NaN carried in", leaked, r["alone"][b], rk.sinc_tol(F16))
    del rk.WORST["host-mutant"]


def test_mutant_partial_slot_of_a_tile_past_the_length(sinc_result):
    r = sinc_result
    bad = r["part"].copy()
    bad[1, rk.sinc_slot(1, 3), 2, 1] = 1e-6                   # row of 7 samples: tile 1 of shift 3, inside the row's own P_b
    with pytest.raises(AssertionError, match="differ from the dense launch"):
        rk.check_slots("mutant", bad, r["parts"], used=[rk.sinc_used(L) for L in r["lengths"]])
    parts = [p.copy() for p in r["parts"]]                    # ... and when the dense launch on the row alone leaves it too
    parts[1][rk.sinc_slot(1, 3), 2, 1] = 1e-6
    with pytest.raises(AssertionError, match="tile past the length"):
        rk.check_slots("mutant", bad, parts, used=[rk.sinc_used(L) for L in r["lengths"]])
    lout = [127, 1, 257]
    parts = [np.ones((rk.conv_slots(l), 16, 2), np.float32) for l in lout]
    part = np.zeros((3, rk.conv_slots(385), 16, 2), np.float32)
    for b, p in enumerate(parts):
        part[b, :p.shape[0]] = p
    rk.check_slots("ok", part, parts)
    part[1, 2, 0, 0] = -3.0                                   # slot 2 = rows 128 .. 191 of a row with one output row
    with pytest.raises(AssertionError, match="past the last tile"):
        rk.check_slots("mutant", part, parts)


@pytest.fixture(scope="module")
def lstm_result():
    ttab, T = [5, 1, 3, 21], 21
    xg, whh = rk.lstm_operands(len(ttab), T)
    alone = [rk.lstm_ref64(xg[b], whh, Tj).float().numpy() for b, Tj in enumerate(ttab)]
    return dict(ttab=ttab, T=T, xg=xg, whh=whh, alone=alone, out=_perfect(alone, T, "zero", extra_cols=rk.LSTM_PADCOLS))


def test_mutant_longest_step_count_for_every_chain(lstm_result):
    """every chain walked T steps: the forward rows below Tj are right, the rows from Tj on are not zero, the reverse chain
    starts in the padding"""
    r = lstm_result
    H, T = rk.LSTM_H, r["T"]
    rk.check_rows("ok", r["out"], r["alone"], "zero", cols=2 * H)
    bad = r["out"].copy()
    for b in range(len(r["ttab"])):
        bad[b, :, :2 * H] = rk.lstm_ref64(r["xg"][b], r["whh"], T).float().numpy()
    with pytest.raises(AssertionError):
        rk.check_rows("mutant", bad, r["alone"], "zero", cols=2 * H)
    fwd_only = r["out"].copy()                                # even with the reverse half repaired, the zeros are missing
    for b in range(len(r["ttab"])):
        fwd_only[b, :, :H] = bad[b, :, :H]
    with pytest.raises(AssertionError, match="not exact zeros"):
        rk.check_rows("mutant", fwd_only, r["alone"], "zero", cols=2 * H)


def test_mutant_reverse_chain_started_at_the_last_row_of_the_buffer(lstm_result):
    """reverse chain from T - 1 instead of Tj - 1 (over finite padding, so that only the values tell): outside the bound on
    every chain shorter than T, and not the dense bits"""
    r = lstm_result
    H, T = rk.LSTM_H, r["T"]
    for b, Tj in enumerate(r["ttab"]):
        wrong = rk.lstm_chain64(r["xg"][b, :, 1], r["whh"][1], True, start=T - 1)[:Tj]
        ref = rk.lstm_ref64(r["xg"][b], r["whh"], Tj)[:, H:]
        if Tj == T:
            assert torch.equal(wrong, ref)
            continue
        assert float((wrong - ref).abs().max()) > 50 * rk.LSTM_TOL
        with pytest.raises(AssertionError):
            rk.check_ref("host-mutant", "reverse from T - 1", wrong, ref, rk.LSTM_TOL)
        bad = r["out"].copy()
        bad[b, :Tj, H:2 * H] = wrong.float().numpy()
        with pytest.raises(AssertionError, match="differs from the dense launch"):
            rk.check_rows("mutant", bad, r["alone"], "zero", cols=2 * H)
    del rk.WORST["host-mutant"]


def test_mutant_pooled_zero_fill_missing_for_one_workgroup():
    """the rows Tout_b + jz, Tout_b + jz + PS, ... of one workgroup jz keep their NaN"""
    pairs, (TinS, ToutS) = rk.HP_PAIRS, rk.HP_STRIDES[1]
    PS = max(t for _, t in rk.HP_TILES)
    g = torch.Generator().manual_seed(3)
    alone = [torch.randn(Tout, 8, generator=g).numpy() for _, Tout in pairs]
    good = _perfect(alone, ToutS, "zero", extra_cols=2)
    rk.check_rows("ok", good, alone, "zero", cols=8)
    for b, jz in ((0, 0), (1, 20), (3, 7), (4, 1)):           # the longest row too: two rows to zero at these strides
        Tout = pairs[b][1]
        share = list(range(Tout + jz, ToutS, PS))
        if not share:
            continue
        bad = good.copy()
        bad[b, share, :8] = np.nan
        with pytest.raises(AssertionError, match="not exact zeros"):
            rk.check_rows("mutant", bad, alone, "zero", cols=8)
    assert list(range(512 + 1, ToutS, PS)) == [513]           # (the (4, 1) mutant above exists)


def test_company_helper_rejects_a_row_that_moved():
    a = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    b = a.copy()
    b[1, 3] += 1                                              # beyond lens[1] = 3: not compared
    rk.check_same("ok", a, b, [4, 3])
    b[1, 2, 0] += 1e-6 * 64
    with pytest.raises(AssertionError, match="depends on its company"):
        rk.check_same("mutant", a, b, [4, 3])


# ---------------------------------------------------------------------------
# 3. the length tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", rk.CONV_FORMS, ids=[rk.conv_form_id(f) for f in rk.CONV_FORMS])
def test_conv_lengths_take_every_tile_edge(form):
    cin, N, k, s, p, nin, skip = form
    lins, louts, Lin, Lout = rk.conv_lengths(k, s, p)
    assert sorted(set(louts)) == sorted(rk.CONV_LOUTS) and 1 in lins and Lout == rk.CONV_MIN_BUFFER_LOUT
    for lin, lout in zip(lins, louts):
        x = torch.zeros(1, cin, lin, device="meta")
        assert F.conv1d(x, torch.zeros(N, cin, k, device="meta"), stride=s, padding=p).shape[-1] == lout
    if s == 2:
        for lo in (128, 129):
            both = [l for l, o in zip(lins, louts) if o == lo]
            assert len(both) == 2 and {l % 2 for l in both} == {0, 1}
    assert lins != sorted(lins)                               # short rows between long ones
    nMt = -(-Lout // 128)
    assert nMt == 4 and all(-(-lo // 128) < nMt for lo in louts)       # a fourth tile column that no row reaches
    assert [rk.conv_slots(lo) for lo in (1, 128, 129, 257)] == [2, 2, 4, 6]
    wl = rk.conv_lengths(k, s, p, extra=300)
    assert wl[:2] == (lins, louts) and wl[2] == Lin + 300


def test_sinc_slot_masks_and_the_workgroup_boundary():
    assert [rk.sinc_tiles(L) for L in (1, 8192, 8193, 33000, 34817)] == [256, 256, 512, 1280, 1280]
    for L in rk.SINC_A["lengths"] + rk.SINC_B["lengths"]:
        used = rk.sinc_used(L)
        tiles = -(-L // 256)
        assert used.numel() == rk.sinc_tiles(L) and int(used.sum()) == 8 * tiles
        ref = torch.zeros_like(used)
        for g in range(tiles):                                # tests/test_sinc_fir16_resident_gpu.py:87-90
            for o in range(8):
                ref[(g // 8) * 64 + o * 8 + g % 8] = True
        assert torch.equal(used, ref)
    slots = {rk.sinc_slot(g, o) for g in range(32) for o in range(8)}
    assert slots == set(range(256))                           # a chunk's slots: each once
    # the launch rule: B 5 x 33000 samples -> two workgroups of 17 spans; one workgroup per row in case A
    c = rk.SINC_B
    assert rk.sinc_spans_per_wg(len(c["lengths"]), c["Lrow"]) == 17 and 17 * rk.SINC_SPAN == c["boundary"] == 17408
    assert c["lengths"][1:4] == [c["boundary"], c["boundary"] + 1, c["boundary"] - 1]
    assert rk.sinc_spans_per_wg(len(rk.SINC_A["lengths"]), rk.SINC_A["Lrow"]) == 3 == -(-rk.SINC_A["Lrow"] // rk.SINC_SPAN)
    assert rk.sinc_spans_per_wg(5, 34817) == 18 and rk.sinc_spans_per_wg(5, 31744) == 31 and rk.sinc_spans_per_wg(5, 31745) == 16
    assert rk.sinc_spans_per_wg(256, 65536) == 64 and rk.sinc_spans_per_wg(128, 65536) == 32       # want = 1: the whole row; want = 2


def test_headpool_pairs_and_tile_counts():
    for (Tin, Tout), (fpt, tiles) in zip(rk.HP_PAIRS, rk.HP_TILES):
        f = rk.headpool_frames_per_tile(Tin, Tout)
        assert f == fpt and -(-Tout // f) == tiles
        for i0 in range(0, Tout, f):                          # a tile never spans more than 128 input rows; f + 1 frames would
            assert -(-(min(i0 + f, Tout) * Tin) // Tout) - (i0 * Tin) // Tout <= 128
    assert rk.headpool_frames_per_tile(5, 9) == 0 and rk.headpool_frames_per_tile(0, 0) == 0
    assert rk.headpool_frames_per_tile(129 * 40, 1) == 0      # one window of more than 128 rows
    TinS, ToutS = rk.HP_STRIDES[0]
    assert (TinS, ToutS) == rk.HP_PAIRS[-1] == max(rk.HP_PAIRS)
    assert all(a <= rk.HP_STRIDES[1][0] and b <= rk.HP_STRIDES[1][1] for a, b in rk.HP_PAIRS)


def test_lstm_and_gather_tables():
    (t0, T0), (t1, T1), (t2, T2), (t3, T3) = rk.LSTM_CASES
    assert len(t0) == 9 and {1, 2, 3, 130} <= set(t0[:4]) and max(t0) == T0          # first workgroup: tails beside 130; three workgroups
    assert t1[:4] == [1, 1, 1, 1] and t1[4] == T1 and len(t1) == 5
    assert t2 == [3] and T2 == 7 and t3 == [130] * 5
    for dt, rows_tab, T, scols, dcols, width in rk.GATHER_CASES:
        assert max(rows_tab) <= T and width <= min(scols, dcols) and (dt is torch.float32 or width % 2 == 0)
    assert rk.GATHER_CASES[1][0] is torch.float32 and 1 in rk.GATHER_CASES[1][1] and rk.GATHER_CASES[1][5] % 2 == 1
