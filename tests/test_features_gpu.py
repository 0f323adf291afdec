"""The features builder on the GPU: ``bm_segment_features`` (csrc/features.hip) against the live reference's windows
(tests/golden/features_builder.npz) and, beyond them, against the numpy restatement of the same rules
(tests/features_cases.py, itself held to the fixture by test_features_cpu.py).  Every output is a copy of a table value, an
array entry or a default, so every comparison is bit equality.

Random case: three recordings at 120 Hz with 40, 0 and 9 words (120, 0 and 27 phonemes) and 6, 3 and 0 sounds; the builder
has 70 channels -- WordLength 1, Mel 30 (resampled), WordVector 20, Phoneme 1 (categorical), Embedding 18 (chunk) -- so the
16-channel slabs of the kernel are ragged: features start and end inside slabs, the last slab has 6 channels.
"""
import numpy as np
import pytest
import torch

import features_cases as FC
from test_segments_gpu import Carver, bits

pytestmark = pytest.mark.gpu

SR = 120.
N_SAMPLES = 2400
DIMS = (20, 30, 18)
SPECS = FC.RANDOM_SPECS(*DIMS)
COUNTS = ((40, 6), (0, 3), (9, 0))          # (words, sounds) per recording


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def random_case():
    """(builder, host event tables, DeviceEvents) of the three recordings, made once."""
    from brainmagick_amd.features import DeviceEvents
    builder = FC.make_builder(SPECS, SR, event_mask=True)
    host = [FC.random_events(11 + i, SR, N_SAMPLES, w, s, DIMS) for i, (w, s) in enumerate(COUNTS)]
    return builder, host, [DeviceEvents(builder, ev) for ev in host]


def event_table(H, builder, device_events):
    return H.EventTable(builder.plan(), len(builder.kinds), builder.mask_kind,
                        [(ev.kind_tables, ev.sources) for ev in device_events], "cuda")


def windows(rec, first_samples, T, sr):
    times = [FC.window_times(s, T, sr) for s in first_samples]
    return (torch.tensor(rec, dtype=torch.int32, device="cuda"),
            torch.tensor([t[0] for t in times], dtype=torch.float64, device="cuda"),
            torch.tensor([t[1] for t in times], dtype=torch.float64, device="cuda"))


def truth(specs, event_mask, host, rec, first_samples, T, sr):
    data, mask = zip(*[FC.build_window(specs, event_mask, host[r], *FC.window_times(s, T, sr), sr, T)
                       for r, s in zip(rec, first_samples)])
    return torch.from_numpy(np.stack(data)), torch.from_numpy(np.stack(mask))


def flag_word():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("case", FC.fixture_cases(), ids=[c["name"] for c in FC.fixture_cases()])
def test_kernel_equals_the_reference(H, case):
    from brainmagick_amd.features import DeviceEvents
    sr = case["sample_rate"]
    builder = FC.make_builder(case["specs"], sr, case["event_mask"])
    table = event_table(H, builder, [DeviceEvents(builder, case["events"])])
    flag = flag_word()
    for T in (13, 87):
        ws = [w for w in case["windows"] if w["T"] == T]
        rec, wstart, wdur = windows([0] * len(ws), [w["first"] for w in ws], T, sr)
        feats, mask = H.segment_features(table, rec, wstart, wdur, 0, len(ws), T, sr, flag)
        assert feats.shape == (len(ws), case["dimension"], T) and mask.shape == (len(ws), 1, T) and mask.dtype == torch.bool
        want = torch.from_numpy(np.stack([w["data"] for w in ws]))
        want_mask = torch.from_numpy(np.stack([w["mask"] for w in ws]))
        wrong = (bits(feats) != bits(want)).flatten(1).any(1).nonzero().flatten().tolist()
        assert not wrong, (case["name"], T, [ws[i]["first"] for i in wrong[:5]])
        assert torch.equal(mask.cpu(), want_mask)
        assert bool((mask.view(torch.uint8) <= 1).all())
    assert int(flag.item()) == 0


REC7 = [0, 2, 1, 0, 0, 2, 1]


def _firsts(T):
    return [0, N_SAMPLES - T, 777, 1203, N_SAMPLES - T, 5, 1500]


@pytest.mark.parametrize("T", [87, 13])
def test_random_tables_equal_the_restatement_twice(H, random_case, T):
    builder, host, dev = random_case
    assert builder.dimension == 70 and builder.output_dimension == 109
    table = event_table(H, builder, dev)
    flag = flag_word()
    firsts = _firsts(T)
    rec, wstart, wdur = windows(REC7, firsts, T, SR)
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 7, T, SR, flag)
    want, want_mask = truth(SPECS, True, host, REC7, firsts, T, SR)
    assert torch.equal(bits(feats), bits(want)) and torch.equal(mask.cpu(), want_mask)
    assert want_mask.any() and not want_mask.all() and not want_mask[2].any()        # recording 1 has no word
    assert bool((want[:, 1:31] != -5.0).any()) and bool((want[:, 52:] != 0).any())   # mel and embedding were painted
    again, mask_again = H.segment_features(table, rec, wstart, wdur, 0, 7, T, SR, flag)
    assert torch.equal(bits(again), bits(feats)) and torch.equal(mask_again, mask)
    assert int(flag.item()) == 0


def test_a_batch_at_an_offset_equals_its_segments_alone(H, random_case):
    builder, host, dev = random_case
    table = event_table(H, builder, dev)
    flag = flag_word()
    T = 87
    firsts = _firsts(T)
    rec, wstart, wdur = windows([9, -4] + REC7 + [5], [10 ** 6, 3] + firsts + [0], T, SR)
    feats, mask = H.segment_features(table, rec, wstart, wdur, 2, 7, T, SR, flag)
    want, want_mask = truth(SPECS, True, host, REC7, firsts, T, SR)
    assert torch.equal(bits(feats), bits(want)) and torch.equal(mask.cpu(), want_mask)
    for b in range(7):
        one, one_mask = H.segment_features(table, rec, wstart, wdur, 2 + b, 1, T, SR, flag)
        assert torch.equal(bits(one[0]), bits(feats[b])) and torch.equal(one_mask[0], mask[b]), b
    assert int(flag.item()) == 0


def test_non_finite_values_pass_through(H):
    from brainmagick_amd.features import DeviceEvents
    nan, inf = float("nan"), float("inf")
    specs = [FC.feature("Vec", "constant", "word", 3), FC.feature("Mel", "resampled", "sound", 2),
             FC.feature("Emb", "chunk", "sound", 2)]
    builder = FC.make_builder(specs, SR)
    mel = np.arange(2 * 240, dtype=np.float32).reshape(2, 240)
    emb = np.arange(2 * 96, dtype=np.float32).reshape(2, 96)
    mel[0, 100:140], mel[1, 7] = nan, -inf
    emb[1, 40:60], emb[0, 3] = inf, nan
    payload = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)
    mel_t = torch.from_numpy(mel)
    mel_t[1, 120] = payload[0]
    host = dict(word=dict(start=[0.1, 0.5], duration=[0.3, 0.4], Vec=[[nan, 1., -inf], [inf, -0., 2.]]),
                sound=dict(start=[0.], duration=[2.], Mel=[mel_t.numpy()], Emb=[emb]))
    table = event_table(H, builder, [DeviceEvents(builder, host)])
    firsts = [0, 60, 110]
    rec, wstart, wdur = windows([0] * 3, firsts, 87, SR)
    flag = flag_word()
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 3, 87, SR, flag)
    want, _ = truth(specs, False, [host], [0] * 3, firsts, 87, SR)
    assert torch.equal(bits(feats), bits(want)) and bool(mask.all())
    got = feats.cpu()
    assert torch.isnan(got).sum() > 40 and torch.isinf(got).sum() > 20
    assert (bits(feats) == 0x7FC12345).any() and (bits(feats[:, 1]) == -2 ** 31).any()      # a payload and -0.0


def _carved_events(carver, builder, dev):
    """The device tensors of a DeviceEvents moved into poisoned buffers: value rows and arrays 4- but not 16-byte
    aligned, the float64 tables 8- but not 16-byte aligned."""
    def place64(t):                                         # through int32 words: the carver poisons those with 0xFF
        return carver.place(t.contiguous().view(torch.int32), 2).view(torch.float64)
    kinds = [None if k is None else tuple(place64(t) for t in k) for k in dev.kind_tables]
    sources = []
    for i, s in enumerate(dev.sources):
        if s is None:
            sources.append(None)
        elif isinstance(s, torch.Tensor):
            sources.append(carver.place(s, 1 + i % 3))
        else:
            sources.append(([carver.place(a, 1 + (i + e) % 3) for e, a in enumerate(s[0])], s[1]))
    return kinds, sources


@pytest.mark.parametrize("T", [87, 13])
def test_guard_bands_and_misaligned_tables(H, random_case, T):
    """Event tables, value rows, arrays, index arrays and both outputs inside poisoned bands; outputs at every 4-byte
    alignment, NaN-filled (0xFF for the mask) beforehand: nothing outside is written, everything inside is."""
    builder, host, dev = random_case
    carver = Carver()
    carved = [_carved_events(carver, builder, ev) for ev in dev]
    for kinds, sources in carved:
        for s in sources:
            for t in ([s] if isinstance(s, torch.Tensor) else [] if s is None else s[0]):
                assert t.data_ptr() % 16 != 0 and t.data_ptr() % 4 == 0
    table = H.EventTable(builder.plan(), len(builder.kinds), builder.mask_kind, carved, "cuda")
    firsts = _firsts(T)
    rec, wstart, wdur = windows([7] + REC7 + [-1], [0] + firsts + [0], T, SR)
    rec = carver.place(rec, 1)
    wstart, wdur = (carver.place(t.view(torch.int32), 2).view(torch.float64) for t in (wstart, wdur))
    want, want_mask = truth(SPECS, True, host, REC7, firsts, T, SR)
    flag = carver.empty((1,), torch.int32, 1)
    flag.zero_()
    for shift in (1, 2, 3, 0):
        dest = carver.empty((7, 70, T), torch.float32, shift)
        dest_mask = carver.empty((7, 1, T), torch.bool, shift + 1)
        feats, mask = H.segment_features(table, rec, wstart, wdur, 1, 7, T, SR, flag, dest=dest, dest_mask=dest_mask)
        assert feats.data_ptr() == dest.data_ptr() and mask.data_ptr() == dest_mask.data_ptr()
        carver.check()
        assert not torch.isnan(feats).any() and bool((mask.view(torch.uint8) <= 1).all())       # no element was left out
        assert torch.equal(bits(feats), bits(want)) and torch.equal(mask.cpu(), want_mask), shift
    assert int(flag.item()) == 0


@pytest.mark.parametrize("event_mask", [True, False])
def test_range_flag_and_defaults(H, random_case, event_mask):
    from brainmagick_amd.features import DeviceEvents
    _, host, _ = random_case
    builder = FC.make_builder(SPECS, SR, event_mask=event_mask)
    table = event_table(H, builder, [DeviceEvents(builder, ev) for ev in host])
    T = 87
    firsts = _firsts(T)
    flag = flag_word()
    rec, wstart, wdur = windows(REC7, firsts, T, SR)
    H.segment_features(table, rec, wstart, wdur, 0, 7, T, SR, flag)
    assert int(flag.item()) == 0                                       # valid segments leave the flag down
    bad_rec = list(REC7)
    bad_rec[0], bad_rec[3], bad_rec[6] = 3, -1, 2 ** 31 - 1
    rec, wstart, wdur = windows(bad_rec, firsts, T, SR)
    carver = Carver()
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 7, T, SR, flag,
                                     dest=carver.empty((7, 70, T), torch.float32, 1),
                                     dest_mask=carver.empty((7, 1, T), torch.bool, 1))
    carver.check()
    assert int(flag.item()) == 1
    want, want_mask = truth(SPECS, event_mask, host, REC7, firsts, T, SR)
    defaults = torch.zeros(70, T)
    defaults[1:31] = -5.0
    for b in range(7):
        if b in (0, 3, 6):
            assert torch.equal(bits(feats[b]), bits(defaults)) and bool((mask[b] != event_mask).all()), b
        else:
            assert torch.equal(bits(feats[b]), bits(want[b])) and torch.equal(mask[b].cpu(), want_mask[b]), b


def _segments(random_case, specs=None, event_mask=True, n_meg=(5, 8, 3)):
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    _, host, _ = random_case
    specs = SPECS if specs is None else specs
    builder = FC.make_builder(specs, SR, event_mask=event_mask)
    g = torch.Generator().manual_seed(4)
    recs = []
    for i, c in enumerate(n_meg):
        names = {"start", "duration"} | {s["name"] for s in specs}
        ev = {k: {n: v for n, v in t.items() if n in names} for k, t in host[i].items() if k in builder.kinds}
        recs.append(DeviceRecording(torch.randn(c, N_SAMPLES, generator=g).cuda(), events=DeviceEvents(builder, ev),
                                    recording=Recording(10 + i, torch.rand(c, 2, generator=g)), subject_index=2 - i))
    return DeviceSegments(recs, SR, tmin=-0.1, tmax=0.6166, condition=0.9, meg_dimension=8), builder, host


def test_one_loader_epoch(H, random_case, monkeypatch):
    from brainmagick_amd import dataset as D
    seg, builder, host = _segments(random_case)
    assert seg.T == 87 and seg.n_features == 70 and len(seg) > 20
    launches, real = [], H.segment_features

    def spy(table, rec, wstart, wdur, first, count, *args, **kw):
        launches.append((rec.data_ptr(), wstart.data_ptr(), first, count))
        return real(table, rec, wstart, wdur, first, count, *args, **kw)
    monkeypatch.setattr(H, "segment_features", spy)
    loader = D.DeviceSegmentLoader(seg, 8, shuffle=True, generator=torch.Generator().manual_seed(3))
    batches = list(loader)
    monkeypatch.setattr(H, "segment_features", real)
    ep = loader.epoch_arrays
    assert len(launches) == len(batches) == len(loader)                 # ONE features launch per batch
    assert {(r, w) for r, w, _, _ in launches} == {(ep["rec"].data_ptr(), ep["wstart"].data_ptr())}
    for k, batch in enumerate(batches):
        idx = loader.order[8 * k:8 * k + 8]
        want, want_mask = truth(SPECS, True, host, seg.rec[idx].tolist(), seg.start[idx].tolist(), seg.T, SR)
        assert batch.features.shape == (len(idx), 70, 87) and batch.meg.shape == (len(idx), 8, 87)
        assert torch.equal(bits(batch.features), bits(want)) and torch.equal(batch.features_mask.cpu(), want_mask)
        assert batch.recording_index.tolist() == [10 + int(seg.rec[i]) for i in idx]
    sub = seg.only(2)
    one = sub.batch([0, 1])
    want, _ = truth(SPECS, True, host, [2, 2], sub.start[:2].tolist(), seg.T, SR)
    assert torch.equal(bits(one.features), bits(want))


def test_train_step_equals_the_step_on_a_host_built_batch(random_case):
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.synthetic import SegmentBatch
    specs = [FC.feature("Mel", "resampled", "sound", DIMS[1], default_value=-5.0), FC.feature("Embedding", "chunk", "sound", DIMS[2])]
    seg, builder, host = _segments(random_case, specs, event_mask=False, n_meg=(5, 8))      # ClipLoss takes an all-true mask
    idx = [int(i) for i in np.linspace(0, len(seg) - 1, 6).astype(int)]
    batch = seg.batch(idx)
    want, want_mask = truth(specs, False, host, seg.rec[idx].tolist(), seg.start[idx].tolist(), seg.T, SR)
    assert torch.equal(bits(batch.features), bits(want)) and bool(batch.features_mask.all()) and bool(want_mask.all())
    moved = batch.to("cpu")
    host_batch = SegmentBatch(moved.meg, want, want_mask, moved.subject_index, moved.recording_index, moved._recordings)
    cfg = dict(depth=4, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2, glu_context=1,
               complex_out=True, merger=True, merger_pos_dim=128, merger_channels=24, merger_dropout=0.0,
               initial_linear=24, subject_layers=True, subject_dim=0)

    def solver():
        torch.manual_seed(0)
        return Solver(SimpleConv(in_channels={"meg": 8}, out_channels=builder.dimension, hidden={"meg": 8}, n_subjects=3,
                                 **cfg), ClipLoss())
    loss_a = solver().train_step(batch)
    loss_b = solver().train_step(host_batch)
    assert bool(torch.isfinite(loss_a)) and torch.equal(bits(loss_a.reshape(1).float()), bits(loss_b.reshape(1).float()))


def test_feature_decoding_step_on_a_categorical_feature_built_by_the_kernel(random_case):
    from brainmagick_amd.losses import FeatureDecodingLoss
    specs = [FC.feature("Phoneme", "constant", "phoneme", cardinality=40), FC.feature("WordLength", "constant", "word")]
    seg, builder, host = _segments(random_case, specs, event_mask=True, n_meg=(5,))
    idx = list(range(0, len(seg), 2))[:8]
    batch = seg.batch(idx)
    want, want_mask = truth(specs, True, host, [0] * len(idx), seg.start[idx].tolist(), seg.T, SR)
    assert torch.equal(bits(batch.features), bits(want)) and torch.equal(batch.features_mask.cpu(), want_mask)
    assert want_mask.any() and len(want[:, 0][want_mask[:, 0]].unique()) > 3                 # several classes selected
    est = torch.randn(len(idx), builder.output_dimension, seg.T, generator=torch.Generator().manual_seed(6))
    loss_mod = FeatureDecodingLoss(builder, None)
    loss_mod.no_mask_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    e = est.cuda().requires_grad_(True)
    loss = loss_mod(e, batch.features, batch.features_mask)
    loss.backward()
    sel = want_mask[:, 0]                                                                      # [B, T]
    logits = est[:, :40].permute(0, 2, 1)[sel].double()
    ce = torch.nn.functional.cross_entropy(logits, want[:, 0][sel].long())
    mse = ((est[:, 40].double() - want[:, 1].double())[sel] ** 2).mean()
    # fp32 terms against fp64 ones: a few dozen roundings of 2^-24 per term, the means keep the relative error
    assert abs(float(loss.detach()) - float(ce + mse)) <= 1e-5 * float(ce + mse)
    assert int(loss_mod.no_mask_flag.item()) == 0 and bool(torch.isfinite(e.grad).all())
    assert bool((e.grad.cpu()[~sel[:, None].expand_as(est)] == 0).all())


@pytest.mark.parametrize("T", [87, 13])
def test_more_candidates_than_a_chunk_and_a_table_of_three_search_rounds(H, T):
    """5 000 words (64^2 < 5 000: the wavefront-wide searches take three rounds) behind one word that lasts the whole
    recording: the running maximum holds the lower bound at 0, so a window at sample s has every word that starts before
    its end as a candidate -- 1, about 260 (two chunks of 256 candidates, the second nearly empty), about 2 500 and all
    5 000 (twenty chunks).  The long word paints every sample and later words overwrite it, across chunks."""
    from brainmagick_amd.features import DeviceEvents
    rng = np.random.default_rng(9)
    n = 5000
    total = N_SAMPLES / SR
    start = np.concatenate([[0.0], np.sort(rng.uniform(0.01, total, n - 1))])
    dur = np.concatenate([[total + 1.0], rng.uniform(0.0, 0.05, n - 1)])
    host = dict(word=dict(start=start, duration=dur, WordLength=rng.integers(1, 12, n).astype(np.float64),
                          WordVector=rng.standard_normal((n, 5))))
    specs = [FC.feature("WordVector", "constant", "word", 5), FC.feature("WordLength", "constant", "word")]
    builder = FC.make_builder(specs, SR, event_mask=True)
    table = event_table(H, builder, [DeviceEvents(builder, host)])
    at_260 = int(start[260] * SR) - T + 1                  # the window's end lies just behind the start of word 260
    firsts = [0, max(at_260, 0), N_SAMPLES // 2, N_SAMPLES - T]
    counts = [int(np.searchsorted(start, (s + T) / SR)) for s in firsts]
    assert counts[0] < 256 < counts[1] < 512 and 2000 < counts[2] < 3000 and counts[3] == n, counts
    rec, wstart, wdur = windows([0] * 4, firsts, T, SR)
    flag = flag_word()
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 4, T, SR, flag)
    want, want_mask = truth(specs, True, [host], [0] * 4, firsts, T, SR)
    assert torch.equal(bits(feats), bits(want)) and torch.equal(mask.cpu(), want_mask) and bool(want_mask.all())
    long_row = torch.from_numpy(host["word"]["WordVector"][0].astype(np.float32))
    painted_by_long = (want[:, :5] == long_row[None, :, None]).all(1)
    assert painted_by_long.any() and not painted_by_long.all()          # both the long word and later ones show
    assert int(flag.item()) == 0
