"""training.WaveformSet, its two kernels and ConformerPipeline.train on the MI355X.

  fixture set       file_index and noise_ids exact; scale within 2^-22 relative of the float64 restatement (a double rounded once to
                    fp32); every __getitem__ pair within 16 x e32 of what the reference's WaveformDataset gave
                    (tests/golden/g26_waveset.npz), e32 = the float32 restatement against the float64 one; clean rows and padding exact
  mix_scale_varlen  1, 4095, 4096, 4097 and 12289 samples at every packed alignment mod 4, noises of 1, 3 and 5000 samples: the same
                    bound, and the same bits from run to run
  wave_batch        plane 0 bitwise ops.mix_apply on the padded rows with the set's scale, plane 1 bitwise the stored samples, into a
                    NaN-filled buffer; rows of 2001 and 2002 samples are not 16-byte aligned; repeats and -1 in the index
  train             bitwise a replay by hand of the unchanged _train_epoch / _validate at the fixture's rates; best_conformer.pt holds
                    the best epoch; the same bits twice; a NaN-poisoned batch is left out and steps nothing; N < batch trains nothing
"""
import numpy as np
import pytest
import torch

import helpers as hp
import waveset_cases as wc

pytestmark = pytest.mark.gpu

SEED, BATCH, EPOCHS = 1234, 4, 3


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "the GPU suite needs the MI355X"
    import sincformer_metacog_speech_enhancement_amd as p
    from sincformer_metacog_speech_enhancement_amd import ops, training
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp
    return dict(ops=ops, training=training, cp=cp)


@pytest.fixture(scope="module")
def gold():
    g = hp.gold("g26_waveset")
    entries = [g.get("entry%d" % i) for i in range(len(g["lengths"]))]
    noises = [g["noise%d" % k] for k in range(len(wc.NOISE_LENGTHS))]
    snr = [float(s) for s in g["snr_levels"]]
    e32, d64 = wc.e32_rows(entries, noises, snr)
    return dict(g=g, entries=entries, noises=noises, snr=snr, e32=e32, d64=d64, pairs=list(zip(g["noisy"], g["clean"])),
                lengths=wc.kept_lengths(entries))


def _dev(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def _make_set(pkg, gold, max_len=wc.MAX_LEN, entries=None):
    return pkg["training"].WaveformSet(gold["entries"] if entries is None else entries, _dev(gold["noises"]), gold["snr"], wc.FS,
                                       max_len=max_len)


@pytest.fixture(scope="module")
def fixture_set(pkg, gold):
    return _make_set(pkg, gold)


# ---- the fixture set ------------------------------------------------------------------------------------------------------------
def test_fixture_set_against_the_reference(pkg, gold, fixture_set):
    ws = fixture_set
    kept, scales, ids, _ = gold["d64"]
    assert ws.file_index == kept == gold["g"]["kept"].tolist() and len(ws) == len(kept)
    assert ws.noise_ids.dtype == torch.int32 and ws.noise_ids.tolist() == ids
    assert ws.offsets.dtype == torch.int32 and ws.offsets.tolist() == np.concatenate([[0], np.cumsum(gold["lengths"])]).tolist()
    assert ws.clean.dtype == torch.float32 and ws.clean.numel() == sum(gold["lengths"])      # 4 bytes a sample: no stored mix
    rel = np.abs(ws.scale.cpu().numpy().astype(np.float64) / scales - 1.0)
    print("scale: max relative |d| %.3e (bound 2^-22 = %.3e)" % (rel.max(), 2.0 ** -22))
    assert ws.scale.dtype == torch.float32 and rel.max() <= 2.0 ** -22
    got = [tuple(t.cpu().numpy() for t in ws[i]) for i in range(len(ws))]
    assert all(n.shape == c.shape == (wc.MAX_LEN,) for n, c in got)
    ok, worst = wc.pairs_within(got, gold["pairs"], gold["e32"], gold["lengths"])
    print("__getitem__ against the fixture: worst |d| = %.3f x (16 e32)" % worst)
    assert ok, worst
    with pytest.raises(IndexError):
        ws[len(ws)]


def test_from_padded_and_device_entries_give_the_same_set(pkg, gold, fixture_set):
    longest = max(len(e) for e in gold["entries"] if e is not None)
    padded = np.zeros((len(gold["entries"]), longest), np.float32)
    lengths = []
    for i, e in enumerate(gold["entries"]):
        lengths.append(0 if e is None else len(e))
        if e is not None:
            padded[i, :len(e)] = e
    ws = pkg["training"].WaveformSet.from_padded(torch.from_numpy(padded).cuda(), lengths, _dev(gold["noises"]), gold["snr"], wc.FS,
                                                 max_len=wc.MAX_LEN)
    mixed = [None if e is None else (torch.from_numpy(e).cuda() if i % 2 else e) for i, e in enumerate(gold["entries"])]
    ws2 = _make_set(pkg, gold, entries=mixed)
    for other in (ws, ws2):
        assert other.file_index == fixture_set.file_index
        for name in ("clean", "offsets", "noise_ids", "scale"):
            assert torch.equal(getattr(other, name), getattr(fixture_set, name)), name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fixture_set.batch(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fixture_set.batches(4, order=[0, 1, 2])
    with pytest.raises(ValueError):
        _make_set(pkg, gold, entries=[gold["entries"][0], None])                   # nothing of 640 samples


# ---- sfm_mix_scale_varlen ---------------------------------------------------------------------------------------------------------
def test_mix_scale_varlen_at_every_alignment(pkg):
    ops = pkg["ops"]
    rng = np.random.default_rng(5)
    lens, starts = [], {}
    cur = 0
    for a in range(4):                                      # every length at every alignment mod 4: a filler utterance in front
        for n in (1, 4095, 4096, 4097, 12289):
            fill = (a - cur) % 4 or 4
            lens.append(fill)
            cur += fill
            starts[(n, a)] = len(lens)
            assert cur % 4 == a
            lens.append(n)
            cur += n
    U = len(lens)
    packed = (rng.standard_normal(cur) * 0.1).astype(np.float32)
    noises = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in (1, 3, 5000)]
    off = np.concatenate([[0], np.cumsum(lens)])
    ids = np.arange(U) % 3
    ids[1::2] = (np.arange(U // 2) % 5 + np.arange(U // 2) // 5) % 3        # (length + alignment) % 3: each length meets every noise
    snr = np.asarray([-5.0, 0.0, 5.0, 10.0])[np.arange(U) % 4]
    bank = pkg["training"].NoiseBank(_dev(noises))
    args = (torch.from_numpy(packed).cuda(), torch.from_numpy(off.astype(np.int32)).cuda(), bank.buffer, bank.offsets,
            torch.from_numpy(ids.astype(np.int32)).cuda(), torch.from_numpy(snr.astype(np.float32)).cuda(), max(lens))
    first = ops.mix_scale_varlen(*args)
    again = ops.mix_scale_varlen(*args)
    want = np.asarray([wc.mix_scale(packed[off[u]:off[u + 1]], noises[ids[u]], snr[u], max_len=None) for u in range(U)])
    rel = np.abs(first.cpu().numpy().astype(np.float64) / want - 1.0)
    print("mix_scale_varlen: %d utterances, max relative |d| %.3e (bound %.3e)" % (U, rel.max(), 2.0 ** -22))
    assert {ids[u] for u in starts.values()} == {0, 1, 2}
    assert rel.max() <= 2.0 ** -22, [(lens[u], off[u] % 4, rel[u]) for u in np.argsort(rel)[-3:]]
    assert torch.equal(first, again)


# ---- sfm_wave_batch ---------------------------------------------------------------------------------------------------------------
INDEX = {1: [5], 3: [5, -1, 5], 8: [3, 0, -1, 6, 5, 5, 2, 4]}      # (5: the 5000-sample utterance, cut to L)


@pytest.mark.parametrize("B,L", [(1, 2000), (3, 2000), (8, 2000), (3, 2001), (8, 2002)])
def test_wave_batch_is_mix_apply_on_the_padded_rows(pkg, gold, B, L):
    ops = pkg["ops"]
    ws = _make_set(pkg, gold, max_len=L)
    index = torch.tensor(INDEX[B], dtype=torch.int32).cuda()
    out = torch.full((2, B, L), float("nan"), device="cuda")
    res = ops.wave_batch(ws.clean, ws.offsets, ws.bank.buffer, ws.bank.offsets, ws.noise_ids, ws.scale, index, L, out=out)
    assert res is out and not bool(torch.isnan(out).any())               # every element written
    noisy, clean = ws.batch(index)
    assert torch.equal(noisy, out[0]) and torch.equal(clean, out[1])
    off, stored = ws.offsets.tolist(), ws.clean.cpu().numpy()
    valid = [u for u in INDEX[B] if u >= 0]
    padded = np.zeros((len(valid), L), np.float32)
    for r, u in enumerate(valid):
        padded[r, :off[u + 1] - off[u]] = stored[off[u]:off[u + 1]]
    sel = torch.tensor(valid, dtype=torch.long).cuda()
    lens = (ws.offsets[1:] - ws.offsets[:-1])[sel].contiguous()
    assert int(lens.max()) <= L and (L == 2000 or int(lens.max()) == L)
    want, _ = ops.mix_apply(torch.from_numpy(padded).cuda(), ws.bank.buffer, ws.bank.offsets, ws.noise_ids[sel].contiguous(),
                            ws.scale[sel].contiguous(), lens)
    rows = [r for r, u in enumerate(INDEX[B]) if u >= 0]
    assert torch.equal(out[0][rows], want)                                # the bits of mix_apply
    assert np.array_equal(out[1][rows].cpu().numpy(), padded)             # the stored samples, zero-padded
    empty = [r for r, u in enumerate(INDEX[B]) if u < 0]
    assert not bool(out[:, empty].any())
    assert bool((out[0][rows] != out[1][rows]).any())


def test_an_index_outside_the_set_gives_zero_rows(pkg, fixture_set):
    index = torch.tensor([len(fixture_set), 0, -7, 2 ** 31 - 1], dtype=torch.int32).cuda()
    noisy, clean = fixture_set.batch(index)
    assert not bool(noisy[[0, 2, 3]].any()) and not bool(clean[[0, 2, 3]].any()) and bool(clean[1].any())


def test_batches_cover_the_set_without_a_synchronisation(pkg, fixture_set):
    ws = fixture_set
    N = len(ws)
    assert N == 7
    rows = torch.stack([ws[i][1] for i in range(N)])
    order = torch.tensor([4, 2, 6, 0, 5, 1, 3], dtype=torch.int32).cuda()
    one = torch.tensor([1, -1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        shuffled = list(ws.batches(3, shuffle=True))
        dropped = list(ws.batches(BATCH, shuffle=True, drop_last=True))
        kept = list(ws.batches(BATCH))
        ordered = list(ws.batches(BATCH, order=order, drop_last=True))
        single = ws.batch(one)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [tuple(n.shape) for n, _ in shuffled] == [(3, wc.MAX_LEN), (3, wc.MAX_LEN), (1, wc.MAX_LEN)]
    seen = torch.cat([c for _, c in shuffled])
    match = (seen[:, None, :] == rows[None, :, :]).all(dim=-1)             # [N seen, N stored]
    assert match.sum(dim=0).tolist() == [1] * N and match.sum(dim=1).tolist() == [1] * N       # each utterance once
    assert len(dropped) == 1 and dropped[0][0].shape == (BATCH, wc.MAX_LEN)
    assert [c.shape[0] for _, c in kept] == [4, 3] and torch.equal(torch.cat([c for _, c in kept]), rows)
    assert len(ordered) == 1 and torch.equal(ordered[0][1], rows[order[:BATCH].long()])
    assert torch.equal(single[1][0], rows[1]) and not bool(single[0][1].any())


# ---- train() ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_sets(pkg, gold, fixture_set):
    test_set = _make_set(pkg, gold, entries=[gold["entries"][i] for i in (9, 3, 6)])
    order = [torch.tensor(o, dtype=torch.int32).cuda() for o in ([4, 2, 6, 0, 5, 1, 3], [1, 3, 5, 6, 0, 2, 4], [6, 5, 4, 3, 2, 1, 0])]
    return fixture_set, test_set, order


def _params(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def trained(pkg, train_sets, tmp_path_factory):
    train_set, test_set, order = train_sets
    assert len(train_set) == 7 and len(test_set) == 3
    runs = []
    for name in ("a", "b"):
        d = tmp_path_factory.mktemp("conformer_" + name)
        pipe = pkg["cp"].ConformerPipeline(model_dir=str(d))
        pipe.train(train_set, test_set, epochs=EPOCHS, seed=SEED, order=order, batch_size=BATCH, verbose=(name == "a"))
        runs.append((pipe, d))
    return runs


def test_train_is_the_replay_of_its_epoch_bodies(pkg, gold, train_sets, trained, tmp_path):
    cp = pkg["cp"]
    train_set, test_set, order = train_sets
    pipe, model_dir = trained[0]
    rates = [5e-4 * float(m) for m in gold["g"]["mult%d" % EPOCHS]]
    torch.manual_seed(SEED)
    hand = cp.ConformerPipeline(model_dir=str(tmp_path))
    hand.model = cp.SpeechEnhancer(n_freq=129, d_model=256, num_blocks=4, num_heads=4, d_ff=1024, kernel_size=31, dropout=0.15).cuda()
    mr = cp.MultiResolutionSTFTLoss()
    optimizer, scaler = hand.make_optimizer()
    val_index = torch.arange(len(test_set), dtype=torch.int32).cuda()
    history, best, best_params = [], float("inf"), None
    for e in range(EPOCHS):
        optimizer.lr = rates[e]
        tl, ts = hand._train_epoch([train_set.batch(order[e][:BATCH])], optimizer, mr, scaler)
        vl, vs = hand._validate([test_set.batch(val_index)], mr)
        history.append((tl, ts, vl, vs, rates[e]))
        if vl < best:
            best, best_params = vl, _params(hand.model)
    print("history:", pipe.history)
    assert pipe.history == history
    assert all(np.isfinite(h).all() for h in history) and history[0][0] != history[1][0]
    got, want = _params(pipe.model), _params(hand.model)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    assert pipe.optimizer.stats() == optimizer.stats() and pipe.scaler.stats() == scaler.stats()
    print("optimiser:", optimizer.stats(), "loss scale:", scaler.stats())
    assert optimizer.stats()["step"] >= 1
    loaded = cp.ConformerPipeline(model_dir=str(model_dir))
    loaded.load_model()                                                    # best_conformer.pt of the run's own directory
    sd = loaded.model.state_dict()
    assert all(torch.equal(sd[k], best_params[k]) for k in best_params)
    assert sorted(p.name for p in model_dir.iterdir()) == ["best_conformer.pt"]


def test_train_twice_gives_the_same_bits(trained):
    (a, _), (b, _) = trained
    assert a.history == b.history and len(a.history) == EPOCHS
    pa, pb = _params(a.model), _params(b.model)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)


def test_a_poisoned_batch_is_left_out_and_steps_nothing(pkg, gold, tmp_path):
    cp = pkg["cp"]
    clean8 = [gold["entries"][i] for i in wc.KEPT] + [gold["entries"][1][::-1].copy()]
    good = pkg["training"].WaveformSet(clean8, _dev(gold["noises"]), gold["snr"], wc.FS, max_len=wc.MAX_LEN)
    bad = [c.copy() for c in clean8]
    bad[6][100] = np.nan
    poisoned = pkg["training"].WaveformSet(bad, _dev(gold["noises"]), gold["snr"], wc.FS, max_len=wc.MAX_LEN)
    test_set = _make_set(pkg, gold, entries=[gold["entries"][i] for i in (9, 3, 6)])
    order = torch.arange(8, dtype=torch.int32).cuda()                      # the poisoned utterance is in the second batch
    assert bool(torch.isnan(poisoned.batch(order[4:])[0]).any()) and not bool(torch.isnan(poisoned.batch(order[:4])[0]).any())
    pipe = cp.ConformerPipeline(model_dir=str(tmp_path / "p"))
    pipe.train(poisoned, test_set, epochs=1, seed=SEED, order=order, batch_size=BATCH, verbose=False)
    torch.manual_seed(SEED)
    hand = cp.ConformerPipeline(model_dir=str(tmp_path / "h"))
    hand.model = hand._new_model().cuda()
    optimizer, scaler = hand.make_optimizer()
    optimizer.lr = 5e-4 * float(gold["g"]["mult1"][0])
    tl, ts = hand._train_epoch([good.batch(order[:4])], optimizer, cp.MultiResolutionSTFTLoss(), scaler)      # the first batch alone
    assert pipe.history[0][:2] == (tl, ts) and np.isfinite(tl)
    skips = lambda s: s.stats()["skipped_loss"] + s.stats()["skipped_inf"]
    assert pipe.optimizer.stats()["step"] == optimizer.stats()["step"] and skips(pipe.scaler) == skips(scaler) + 1
    # the weights are those of the first batch's step alone (BatchNorm's running statistics did see the poisoned forward, as
    # the reference's do)
    pa, pb = _params(pipe.model), _params(hand.model)
    assert all(torch.equal(pa[k], pb[k]) for k in pa if "num_batches_tracked" not in k and "running_" not in k)


def test_a_set_smaller_than_the_batch_trains_nothing_and_validates(pkg, gold, tmp_path):
    cp = pkg["cp"]
    small = _make_set(pkg, gold, entries=[gold["entries"][i] for i in (9, 3, 6)])
    pipe = cp.ConformerPipeline(model_dir=str(tmp_path))
    torch.manual_seed(SEED)
    w0 = _params(cp.ConformerPipeline(model_dir=str(tmp_path))._new_model())
    pipe.train(small, small, epochs=1, seed=SEED, batch_size=BATCH, verbose=False)
    tl, ts, vl, vs, lr = pipe.history[0]
    assert tl == 0.0 and ts == 0.0 and np.isfinite(vl) and vl != 0.0 and lr == 5e-4
    assert pipe.optimizer.stats()["step"] == 0
    w1 = _params(pipe.model)
    assert all(torch.equal(w0[k].cuda(), w1[k]) for k in w0)
    assert (tmp_path / "best_conformer.pt").exists()
