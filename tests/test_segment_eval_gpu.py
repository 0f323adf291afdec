"""The segment-level evaluation on the GPU (scripts/run_eval_probs.py:27-180, 237-382): ``bm_segment_eval_labels`` and
``bm_first_occurrence`` (csrc/segment_eval.hip) against the numpy restatement of their rules (tests/segment_eval_cases.py,
itself held to the live reference by test_segment_eval_cpu.py) -- labels are copies of table values, so every comparison
is equality; the batches, masks, vocabularies and hit counts of the runs the reference's own functions made
(tests/golden/segment_eval.npz); and ``retrieval.segment_eval_epoch`` end to end over resident segments against plain
``_process_batch`` calls and a torch / numpy restatement of the collection."""
import numpy as np
import pytest
import torch

import features_cases as FC
import segment_eval_cases as SC
from helpers import Golden

pytestmark = pytest.mark.gpu

T = 13
SR = 120.
SENTINEL = -(2 ** 40) - 7
WORD_HASH = FC.feature("WordHash", "constant", "word", cardinality=51)


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def golden():
    return Golden("segment_eval")


def flag_word(value=0):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def masks_of(B):
    """None, all true, all false, alternating, a single kept row at each end."""
    every = np.ones(B, dtype=bool)
    first, last = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    first[0], last[-1] = True, True
    return [None, every, ~every, np.arange(B) % 2 == 0, first, last]


def features_of(hash_rows, channel=1, F=3):
    """[B, F, T] with the word hashes on ``channel`` and NaN everywhere else: a read of another channel shows."""
    x = torch.full((hash_rows.shape[0], F, hash_rows.shape[1]), float("nan"))
    x[:, channel] = torch.from_numpy(hash_rows)
    return x.cuda()


class Tables:
    """Word tables of some recordings on the device: the ``EventTable`` of a builder that holds only WordHash, the
    ``WordInfoTable`` over the dense ids, and the host tables ``(start, duration, info [n, 3])`` of the restatement.
    ``host``: per recording None (no word event) or ``(start, duration, word info [n, 2])``."""

    def __init__(self, H, host):
        from brainmagick_amd.features import DeviceEvents
        self.builder = FC.make_builder([WORD_HASH], SR)
        self.events = []
        for t in host:
            table = {} if t is None else dict(word=dict(start=t[0], duration=t[1], WordHash=np.ones(len(t[0])),
                                                        word_index=t[2][:, 0], sequence_id=t[2][:, 1]))
            self.events.append(DeviceEvents(self.builder, table))
        self.table = H.EventTable(self.builder.plan(), len(self.builder.kinds), self.builder.mask_kind,
                                  [(e.kind_tables, e.sources) for e in self.events], "cuda")
        rows, self.n_ids = SC.dense_ids([None if t is None else t[2] for t in host])
        rows = [np.zeros((0, 3), dtype=np.int64) if r is None else r for r in rows]
        self.infos = H.WordInfoTable(rows, self.n_ids, "cuda")
        self.host = [None if t is None else (t[0], t[1], rows[r]) for r, t in enumerate(host)]
        self.word_kind = self.builder.kinds.index("word")


def epoch_arrays(rec, wstart, subject, recording, front=0):
    """The epoch's arrays on the device with ``front`` foreign segments in front of the batch."""
    pad = lambda a, fill: np.concatenate([np.full(front, fill, dtype=a.dtype), a])      # noqa: E731
    return dict(rec=torch.from_numpy(pad(np.asarray(rec, dtype=np.int32), 99)).cuda(),
                wstart=torch.from_numpy(pad(np.asarray(wstart, dtype=np.float64), -1.0)).cuda(),
                subject_index=torch.from_numpy(pad(np.asarray(subject, dtype=np.int64), -5)).cuda(),
                recording_index=torch.from_numpy(pad(np.asarray(recording, dtype=np.int64), -6)).cuda())


def run_labels(H, x, channel, t0, mask, arrays, first, tables, n0=0, room=None, flag=None, count=None):
    """(rows written [kept, 7], flag bits): ``dest`` holds ``n0`` sentinel rows, room for every row and 5 more sentinel
    rows; all sentinels are checked."""
    B = x.shape[0]
    kept = B if mask is None else int(np.sum(mask))
    room = B if room is None else room
    dest = torch.full((n0 + room + 5, 7), SENTINEL, dtype=torch.int64, device="cuda")
    flag = flag_word() if flag is None else flag
    m = None if mask is None else torch.from_numpy(np.asarray(mask)).cuda()
    H.segment_eval_labels(x, channel, t0, m, arrays, first, tables.table, tables.word_kind, tables.infos, SR,
                          dest[:n0 + room], n0, flag, count=count)
    out = dest.cpu()
    assert bool((out[:n0] == SENTINEL).all()), "a row in front of n0 was written"
    assert bool((out[n0 + min(kept, room):] == SENTINEL).all()), "a row behind the kept rows was written"
    return out[n0:n0 + min(kept, room)].numpy(), int(flag.item())


def ragged_tables(seed=0, n_samples=6000):
    """Three recordings: 130 words (the first one lasts the whole recording, so every window's candidates start at 0 and
    are walked in several chunks of 64; some overlap, some have no duration, some start on a half sample), 7 words, none."""
    rng = np.random.default_rng(seed)
    host = []
    for n in (130, 7, 0):
        if n == 0:
            host.append(None)
            continue
        start = np.sort(rng.uniform(0, n_samples / SR, n))
        half = rng.random(n) < 0.3
        start[half] = (np.floor(start[half] * SR) + 0.5) / SR
        whole = rng.random(n) < 0.3
        start[whole] = np.floor(start[whole] * SR) / SR
        start = np.sort(start)
        dur = rng.uniform(0.5 / SR, 9 / SR, n)
        dur[rng.random(n) < 0.1] = 0.0
        dur[rng.random(n) < 0.2] = 3 / SR
        if n > 100:
            start[0], dur[0] = 0.0, n_samples / SR
        info = np.stack([rng.integers(0, 6, n), rng.integers(1, 4, n)], axis=1).astype(np.int64)
        host.append((start, dur, info))
    return host


def rows_near_words(rng, host, B, t0, n_samples=6000):
    """``B`` windows: a recording each, and a first sample that puts a word of the recording within two samples of t0."""
    rec = rng.integers(0, len(host), B)
    first = np.zeros(B, dtype=np.int64)
    for b in range(B):
        t = host[rec[b]]
        if t is None:
            first[b] = rng.integers(0, n_samples)
        else:
            first[b] = int(np.floor(t[0][rng.integers(0, len(t[0]))] * SR)) - t0 + rng.integers(-2, 3)
    return rec.astype(np.int32), first / SR


@pytest.fixture(scope="module")
def ragged(H):
    return Tables(H, ragged_tables())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 600])
def test_labels_equal_the_rule(H, ragged, B):
    """Every check_at_time the guards distinguish (11: ``+ 1`` is the window's last sample) under every mask, the batch
    at an offset into the epoch's arrays."""
    rng = np.random.default_rng(B)
    covered = 0
    for t0 in (0, 1, 2, 6, T - 2):
        hashes = SC.hash_rows(rng, B, T, t0, all_zero=(B // 2,))
        x = features_of(hashes)
        rec, wstart = rows_near_words(rng, ragged.host, B, t0)
        subject, recording = rng.integers(0, 50, B), rng.integers(0, 50, B)
        arrays = epoch_arrays(rec, wstart, subject, recording, front=5)
        want, bits = SC.labels(hashes, t0, None, rec, wstart, subject, recording, ragged.host, SR)
        assert bits == 0
        covered += int((want[:, 6] >= 0).sum())
        for mask in masks_of(B):
            kept = np.arange(B) if mask is None else np.flatnonzero(mask)
            got, flag = run_labels(H, x, 1, t0, mask, arrays, 5, ragged, n0=3 if B % 2 else 0)
            assert np.array_equal(got, want[kept]) and flag == 0, (t0, None if mask is None else mask[:8])
    if B >= 63:
        assert covered > B                                                  # more than a fifth of the rows find a word


def test_labels_of_the_fixture_batches_and_its_ranking(H, golden):
    """The batches the reference's ``_load_test_data`` ran: every label column, the first-occurrence mask, the
    vocabulary and -- under the fp64 margin the maker asserted -- the hit counts of top-1, 5 and 10."""
    from brainmagick_amd import retrieval
    from brainmagick_amd.losses import ClipLoss
    meta = golden.meta
    clip = ClipLoss().cuda()
    for name, c in meta["cases"].items():
        case = SC.fixture_case(golden.raw, meta, name)
        tables = Tables(H, case["tables"])
        t0, n = c["check_at_time"], c["n_kept"]
        arrays = epoch_arrays(*(np.concatenate([b[k] for b in case["batches"]])
                                for k in ("rec", "wstart", "subject", "recording")))
        dest = torch.full((n + 2, 7), SENTINEL, dtype=torch.int64, device="cuda")
        flag, at, first = flag_word(), 0, 0
        for b in case["batches"]:
            m = int(b["keep"].sum())
            if m:                                                           # a fully rejected batch launches nothing
                H.segment_eval_labels(torch.from_numpy(b["features"].copy()).cuda(), 2, t0,
                                      torch.from_numpy(b["keep"]).cuda(), arrays, first, tables.table, tables.word_kind,
                                      tables.infos, meta["sample_rate"], dest[:n], at, flag, count=m)
            at, first = at + m, first + len(b["keep"])
        assert at == n and int(flag.item()) == 0 and bool((dest[n:] == SENTINEL).all())
        got = dest[:n].cpu().numpy()
        for column, key in ((0, "word_hashes"), (1, "word_indices"), (2, "seq_indices"), (4, "subject_id"),
                            (5, "recording_id")):
            assert np.array_equal(got[:, column], golden.raw[f"{name}/{key}"]), (name, key)
        assert np.array_equal(SC.groups(got[:, 3]), golden.raw[f"{name}/segment_groups"]), name
        assert np.array_equal(got[:, 3] == 0, golden.raw[f"{name}/word_indices"] == -1)
        segment_id = dest[:n, 3].contiguous()
        mask, first_row = H.first_occurrence(segment_id, tables.n_ids, flag)
        assert int(flag.item()) == 0
        assert np.array_equal(mask.cpu().numpy(), golden.raw[f"{name}/first_mask"]), name
        vocab = segment_id[mask]
        assert np.array_equal(SC.groups(np.concatenate([got[:, 3], vocab.cpu().numpy()]))[n:],
                              golden.raw[f"{name}/vocab_groups"]), name
        preds = torch.from_numpy(golden.raw[f"{name}/estimate"]).cuda()
        trues = torch.from_numpy(golden.raw[f"{name}/output"]).cuda()[mask]
        probs = retrieval.builds_probs(clip, preds, trues, batch_size=16)
        for k in meta["topks"]:
            acc = retrieval.get_accuracy_from_probs(probs, segment_id, vocab, topk=k)
            print(name, k, acc * n, c["hits"][str(k)])
            assert int(round(acc * n)) == c["hits"][str(k)] and abs(acc * n - round(acc * n)) < 1e-3, (name, k)


def small_batch(tables, B=9, t0=6, seed=3):
    rng = np.random.default_rng(seed)
    host = tables.host
    hashes = SC.hash_rows(rng, B, T, t0)
    rec, wstart = rows_near_words(rng, host, B, t0)
    subject, recording = rng.integers(0, 50, B), rng.integers(0, 50, B)
    return host, hashes, rec, wstart, subject, recording


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 0.5, -3.5, 2.0 ** 63, 3e38])
def test_a_word_hash_that_is_no_label_raises_bit_1(H, ragged, bad):
    host, hashes, rec, wstart, subject, recording = small_batch(ragged)
    hashes[4, 6] = bad
    want, bits = SC.labels(hashes, 6, None, rec, wstart, subject, recording, host, SR)
    assert bits == SC.VALUE_BIT
    got, flag = run_labels(H, features_of(hashes), 1, 6, None, epoch_arrays(rec, wstart, subject, recording), 0, ragged)
    assert np.array_equal(got, want) and flag == SC.VALUE_BIT == H.SEGMENT_EVAL_VALUE_BIT      # the other rows are right


def test_large_word_hashes_are_exact_and_zero_is_legal(H, ragged):
    host, hashes, rec, wstart, subject, recording = small_batch(ragged)
    big = float(np.nextafter(np.float32(2.0 ** 63), np.float32(0)))
    hashes[0, 6], hashes[1, 6], hashes[2, 6], hashes[3, 6] = 2.0 ** 24 + 2, big, -big, -1.0
    hashes[5, 5:8] = 0.0
    got, flag = run_labels(H, features_of(hashes), 1, 6, None, epoch_arrays(rec, wstart, subject, recording), 0, ragged)
    assert got[:4, 0].tolist() == [2 ** 24 + 2, int(big), -int(big), -1] and got[5, 0] == 0 and flag == 0
    assert np.array_equal(got, SC.labels(hashes, 6, None, rec, wstart, subject, recording, host, SR)[0])


def test_dest_bound_is_the_kernels_own(H, ragged):
    """A caller that announces fewer kept rows than the mask keeps: the kernel stops at the end of ``dest``, says so,
    and adds its bits to the ones the word holds."""
    host, hashes, rec, wstart, subject, recording = small_batch(ragged, B=70)
    want, _ = SC.labels(hashes, 6, None, rec, wstart, subject, recording, host, SR)
    got, flag = run_labels(H, features_of(hashes), 1, 6, None, epoch_arrays(rec, wstart, subject, recording), 0, ragged,
                           n0=2, room=66, count=0, flag=flag_word(16))
    assert np.array_equal(got, want[:66]) and flag == 16 | SC.DEST_BIT and SC.DEST_BIT == H.SEGMENT_EVAL_DEST_BIT


def test_recording_out_of_range_gets_the_no_word_values(H, ragged):
    host, hashes, rec, wstart, subject, recording = small_batch(ragged, B=70)
    rec = rec.copy()
    rec[[0, 33, 69]] = [3, -1, 2 ** 30]
    want, bits = SC.labels(hashes, 6, None, rec, wstart, subject, recording, host, SR)
    assert bits == SC.RANGE_BIT and want[[0, 33, 69], 1:4].tolist() == [[-1, -1, 0]] * 3
    got, flag = run_labels(H, features_of(hashes), 1, 6, None, epoch_arrays(rec, wstart, subject, recording), 0, ragged)
    assert np.array_equal(got, want) and flag == SC.RANGE_BIT == H.SEGMENT_EVAL_RANGE_BIT
    keep = np.ones(70, dtype=bool)
    keep[[0, 33, 69]] = False                                               # rejected rows are not looked at
    got, flag = run_labels(H, features_of(hashes), 1, 6, keep, epoch_arrays(rec, wstart, subject, recording), 0, ragged)
    assert np.array_equal(got, want[keep]) and flag == 0


def test_misaligned_source_inside_guard_bands_twice(H, ragged):
    """The features one float past a 16-byte boundary, NaN in front of them and behind them; two runs, the same bits."""
    rng = np.random.default_rng(9)
    B, F, guard = 65, 3, 64
    for t0 in (0, T - 2):
        hashes = SC.hash_rows(rng, B, T, t0)
        rec, wstart = rows_near_words(rng, ragged.host, B, t0)
        subject, recording = rng.integers(0, 50, B), rng.integers(0, 50, B)
        arrays = epoch_arrays(rec, wstart, subject, recording)
        buf = torch.full((guard + 1 + B * F * T + guard,), float("nan"), device="cuda")
        assert buf.data_ptr() % 16 == 0
        x = buf[guard + 1:guard + 1 + B * F * T].view(B, F, T)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        x.zero_()
        x[:, 0] = torch.from_numpy(hashes).cuda()                     # channel 0 at t0 = 0: t0 - 1 is the guard band
        x[:, 2] = torch.from_numpy(hashes).cuda()                     # channel F - 1 at t0 = T - 2: t0 + 2 is
        mask = np.arange(B) % 3 != 1
        want = SC.labels(hashes, t0, mask, rec, wstart, subject, recording, ragged.host, SR)[0]
        for channel in (0, 2):
            a, fa = run_labels(H, x, channel, t0, mask, arrays, 0, ragged, n0=1)
            b, fb = run_labels(H, x, channel, t0, mask, arrays, 0, ragged, n0=1)
            assert np.array_equal(a, want) and fa == 0
            assert np.array_equal(a, b) and fa == fb


# ---------------------------------------------------------------------------------------------------------------------
# bm_first_occurrence
# ---------------------------------------------------------------------------------------------------------------------
def unique_first(ids):
    _, index, inverse = np.unique(ids, return_index=True, return_inverse=True)
    first_row = index[np.asarray(inverse).reshape(-1)]
    return first_row == np.arange(len(ids)), first_row.astype(np.int32)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 70_001])
def test_first_occurrence_equals_unique(H, N):
    rng = np.random.default_rng(N)
    n_ids = max(2, N // 3)
    cases = dict(random=rng.integers(0, n_ids, N), equal=np.full(N, n_ids - 1), zero=np.zeros(N, dtype=np.int64),
                 ends=rng.choice([0, n_ids - 1], N))
    for name, ids in cases.items():
        ids = ids.astype(np.int64)
        mask, first_row = H.first_occurrence(torch.from_numpy(ids).cuda(), n_ids)
        again = H.first_occurrence(torch.from_numpy(ids).cuda(), n_ids)
        want_mask, want_first = unique_first(ids)
        assert mask.dtype == torch.bool and first_row.dtype == torch.int32
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(first_row.cpu().numpy(), want_first), name
        assert torch.equal(mask, again[0]) and torch.equal(first_row, again[1]), name
        rule = SC.first_occurrence(ids, n_ids)
        assert np.array_equal(rule[0], want_mask) and np.array_equal(rule[1], want_first)
    ids = rng.permutation(N).astype(np.int64)                               # all distinct
    mask, first_row = H.first_occurrence(torch.from_numpy(ids).cuda(), N)
    assert bool(mask.all()) and np.array_equal(first_row.cpu().numpy(), np.arange(N))


def test_first_occurrence_out_of_range_leaves_the_other_rows_right(H):
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 40, 300).astype(np.int64)
    ids[[0, 77, 299]] = [40, -1, 2 ** 40]
    flag = flag_word(1)
    mask, first_row = H.first_occurrence(torch.from_numpy(ids).cuda(), 40, flag)
    want_mask, want_first, bits = SC.first_occurrence(ids, 40)
    assert bits == SC.ID_RANGE_BIT == H.FIRST_OCCURRENCE_RANGE_BIT and int(flag.item()) == 1 | bits
    assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(first_row.cpu().numpy(), want_first)
    assert not want_mask[[0, 77, 299]].any() and want_first[[0, 77, 299]].tolist() == [-1, -1, -1]
    empty = H.first_occurrence(torch.zeros(0, dtype=torch.int64, device="cuda"), 4)
    assert empty[0].numel() == 0 and empty[1].numel() == 0


# ---------------------------------------------------------------------------------------------------------------------
# The collection loop over the batches the reference ran (tests/golden/segment_eval.npz)
# ---------------------------------------------------------------------------------------------------------------------
class CannedEpoch:
    """The stand-ins of the fixture's maker on the device, for ``collect_segment_eval``: the solver (``_process_batch``
    returns the recorded estimate and output of the kept rows), and the loader with the segments it belongs to (the
    fixture's batches in order, the epoch's arrays and the word tables)."""
    feature_model = None
    _gather = None

    def __init__(self, H, meta, case):
        from brainmagick_amd.losses import ClipLoss
        from brainmagick_amd.synthetic import SegmentBatch
        self.loss = ClipLoss().cuda()
        words = Tables(H, case["tables"])
        self.builder, self.sample_rate, self.device = words.builder, meta["sample_rate"], torch.device("cuda", 0)
        self.tables = lambda: (None, words.table)
        self.infos = words.infos
        self.segments, self.batch_size = self, meta["batch_size"]
        self.epoch_arrays = epoch_arrays(*(np.concatenate([b[k] for b in case["batches"]])
                                           for k in ("rec", "wstart", "subject", "recording")))
        self.by_id, self.batches = {}, []
        for b in case["batches"]:
            B = len(b["keep"])
            batch = SegmentBatch(torch.zeros(B, 1, T, device="cuda"), torch.from_numpy(b["features"].copy()).cuda(),
                                 torch.ones(B, 1, T, dtype=torch.bool, device="cuda"),
                                 torch.zeros(B, dtype=torch.int64, device="cuda"),
                                 torch.zeros(B, dtype=torch.int64, device="cuda"))
            self.by_id[id(batch.meg)] = b
            self.batches.append(batch)

    def __iter__(self):
        return iter(self.batches)

    def _all_models(self):
        return []

    def check_pending_flags(self):
        pass

    def _process_batch(self, batch):
        b = self.by_id[id(batch.meg)]
        keep = torch.from_numpy(b["keep"]).cuda()
        if b["estimate"] is None:
            return None, None, None, keep
        return (torch.from_numpy(b["estimate"]).cuda(), torch.from_numpy(b["output"]).cuda(), batch.features_mask[keep],
                keep)


def test_bits_left_by_an_aborted_evaluation_do_not_reach_the_next(H, golden):
    """The flag word is the module's: an evaluation that ended in an exception never read it; the next collection
    starts clean, and its labels are the ones the reference's ``_load_test_data`` collected."""
    from brainmagick_amd import retrieval
    meta, name = golden.meta, "t0_6"
    c = meta["cases"][name]
    epoch = CannedEpoch(H, meta, SC.fixture_case(golden.raw, meta, name))
    specs = [FC.feature(f, "constant", "word", cardinality=meta["cardinality"][f]) for f in meta["features"]]
    retrieval.segment_eval_flag("cuda").fill_(15)
    preds, trues, labels = retrieval.collect_segment_eval(epoch, epoch, sum(c["batches"]),
                                                          FC.make_builder(specs, meta["sample_rate"]), c["names"],
                                                          c["check_at_time"], epoch.infos)
    assert int(retrieval.segment_eval_flag("cuda").item()) == 0
    got = labels.cpu().numpy()
    assert got.shape == (c["n_kept"], 7) and labels.dtype == torch.int64
    for column, key in ((0, "word_hashes"), (1, "word_indices"), (2, "seq_indices"), (4, "subject_id"), (5, "recording_id")):
        assert np.array_equal(got[:, column], golden.raw[f"{name}/{key}"]), key
    assert np.array_equal(SC.groups(got[:, 3]), golden.raw[f"{name}/segment_groups"])
    assert np.array_equal(preds.cpu().numpy(), golden.raw[f"{name}/estimate"])
    assert np.array_equal(trues.cpu().numpy(), golden.raw[f"{name}/output"])


# ---------------------------------------------------------------------------------------------------------------------
# End to end over resident segments
# ---------------------------------------------------------------------------------------------------------------------
N_SAMPLES = 1300
LIMIT = 6.0
TOPKS = (1, 5, 10)
CFG = dict(depth=4, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2, glu_context=1,
           complex_out=True, merger=True, merger_pos_dim=128, merger_channels=24, merger_dropout=0.0, initial_linear=24,
           subject_layers=True, subject_dim=0)
MEL = FC.feature("Mel", "resampled", "sound", 8, default_value=-5.0)


def make_segments(spikes=(), columns=True):
    """Two recordings of 6 and 5 MEG channels that hear the same sentences in their first half (a word every 42 samples,
    durations of 1, 2, 5 and 20 samples: the first two end before check_at_time -- no word there) and one mel-like array
    over the whole recording; windows of 37 samples around the word onsets."""
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    builder = FC.make_builder([MEL, WORD_HASH], SR, event_mask=False)
    g = torch.Generator().manual_seed(21)
    rng = np.random.default_rng(21)
    onset = np.arange(20, N_SAMPLES - 40, 42)
    n = len(onset)
    recs, host = [], []
    for i, c in enumerate((6, 5)):
        mel = rng.standard_normal((8, N_SAMPLES)).astype(np.float32)       # its own: no two candidates are equal
        word = dict(start=onset / SR, duration=np.array([1, 2, 5, 20])[np.arange(n) % 4] / SR,
                    WordHash=rng.integers(1, 9, n).astype(np.float64))
        info = np.stack([np.arange(n) % 7, 1 + np.arange(n) // 7 + (100 if i == 1 else 0) * (np.arange(n) >= n // 2)], axis=1)
        if columns:
            word.update(word_index=info[:, 0], sequence_id=info[:, 1])
        events = dict(sound=dict(start=np.array([0.0]), duration=np.array([N_SAMPLES / SR]), Mel=[mel]), word=word)
        meg = torch.randn(c, N_SAMPLES, generator=g).clamp(-3, 3)
        for r, s in spikes:
            if r == i:
                meg[0, s] = 50.0
        recs.append(DeviceRecording(meg.cuda(), events=DeviceEvents(builder, events),
                                    recording=Recording(i, torch.rand(c, 2, generator=g), "study%d" % i), subject_index=i + 3))
        host.append((word["start"], word["duration"], info.astype(np.int64)))
    seg = DeviceSegments(recs, SR, tmin=-0.1, tmax=0.2, condition=onset / SR, meg_dimension=6)
    return seg, builder, host


MODEL_SEED = 0                  # a seed for which the fp64 margin of every verdict holds (asserted by the test)


def make_solver(loss=None, seed=MODEL_SEED):
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    from brainmagick_amd.solver import Solver
    torch.manual_seed(seed)
    model = SimpleConv(in_channels={"meg": 6}, out_channels=8, hidden={"meg": 8}, n_subjects=5, **CFG)
    scaler = DeviceBatchScaler(torch.zeros(2, 6), torch.ones(2, 6))
    return Solver(model, loss if loss is not None else ClipLoss(), scale_reject=ScaleReject(scaler, limit=LIMIT, clip=False))


@pytest.fixture(scope="module")
def epoch():
    return collect_truth()


def collect_truth(seed=MODEL_SEED):
    """The segments (some rows and the whole third batch of the epoch rejected), and the truth collected once by plain
    ``_process_batch`` calls, the reference's torch.where chain and the restated label rule."""
    from brainmagick_amd.dataset import DeviceSegmentLoader
    plain, _, _ = make_segments()
    order = list(range(len(plain)))                                         # shuffle=False: the dataset's order
    rejected = sorted(set(order[14:21]) | {order[0], order[6], order[30], order[-1]})
    spikes = [(int(plain.rec[i]), int(plain.start[i]) + 20) for i in rejected]      # behind the baseline window
    seg, builder, host = make_segments(spikes)
    assert seg.T == 37 and len(seg) == len(plain) and len(seg) % 7 != 0 and len(seg) > 50
    solver = make_solver(seed=seed)
    for m in solver._all_models():
        m.train(False)
    t0 = SC.check_at_time(seg.tmin, SR)
    assert t0 == 14
    rows, n_ids = SC.dense_ids([h[2] for h in host])
    tables = [(h[0], h[1], rows[r]) for r, h in enumerate(host)]
    estimates, outputs, labels, none_batches = [], [], [], 0
    loader = DeviceSegmentLoader(seg, 7)
    for k, batch in enumerate(loader):
        word_hash = batch.features[:, builder.get_slice("WordHash")][:, 0]
        features = batch.features[:, builder.get_slice("Mel")].contiguous()
        with torch.no_grad():
            estimate, output, _, reject_mask = solver._process_batch(batch.replace(features=features))
        idx = order[7 * k:7 * k + 7]
        if estimate is None:
            assert all(i in rejected for i in idx)
            none_batches += 1
            continue
        keep = np.array([i not in rejected for i in idx])
        assert reject_mask.cpu().tolist() == keep.tolist()
        wh = word_hash[reject_mask][:, t0]                                  # scripts/run_eval_probs.py:116-130
        wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 - 1], wh)
        wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 + 1], wh)
        lab, bits = SC.labels(word_hash.cpu().numpy(), t0, keep, seg.rec[idx], seg.wstart[idx],
                              [3 + seg.rec[i] for i in idx], seg.rec[idx], tables, SR)
        assert bits == 0 and np.array_equal(lab[:, 0], wh.cpu().long().numpy())
        estimates.append(estimate.cpu()), outputs.append(output.cpu()), labels.append(lab)
    assert none_batches == 1
    labels = np.concatenate(labels)
    assert (labels[:, 0] == 0).any() and (labels[:, 3] == 0).any() and (labels[:, 3] > 0).sum() > 20
    return dict(seg=seg, builder=builder, rejected=rejected, estimates=torch.cat(estimates), outputs=torch.cat(outputs),
                labels=labels, n_ids=n_ids)


def run_eval(epoch, monkeypatch=None, solver=None, **kw):
    from brainmagick_amd import retrieval
    solver = make_solver() if solver is None else solver
    seen = {}
    real = retrieval.collect_segment_eval

    def no_cpu(self, *a, **k):
        raise AssertionError("Tensor.cpu() during the collection")

    def collect(*args, **kwargs):
        if monkeypatch is None:
            out = real(*args, **kwargs)
        else:
            with monkeypatch.context() as patch:            # no host tensor is created during the collection
                patch.setattr(torch.Tensor, "cpu", no_cpu)
                out = real(*args, **kwargs)
        seen.update(preds=out[0].clone(), outputs=out[1].clone(), labels=out[2].clone())
        return out
    retrieval.collect_segment_eval = collect
    try:
        got = retrieval.segment_eval_epoch(solver, kw.pop("segments", epoch["seg"]), epoch["builder"], ["Mel"],
                                           batch_size=7, **kw)
    finally:
        retrieval.collect_segment_eval = real
    return got, seen


def test_segment_eval_epoch_end_to_end(epoch, monkeypatch):
    from brainmagick_amd import retrieval
    from brainmagick_amd.losses import ClipLoss
    labels = epoch["labels"]
    n = len(labels)
    assert n == len(epoch["seg"]) - len(epoch["rejected"])
    got, seen = run_eval(epoch, monkeypatch, topks=TOPKS, probs_batch_size=16, n_negatives=30)
    # rows and their order: the boolean-index order of every batch, batches in the loader's order
    assert torch.equal(seen["preds"].cpu(), epoch["estimates"]) and torch.equal(seen["outputs"].cpu(), epoch["outputs"])
    assert np.array_equal(seen["labels"].cpu().numpy(), labels)
    assert list(got["metadata"]) == list(retrieval.METADATA_KEYS)
    for column, key in enumerate(retrieval.METADATA_KEYS):
        assert got["metadata"][key].dtype == torch.int64 and got["metadata"][key].is_cuda
        assert np.array_equal(got["metadata"][key].cpu().numpy(), labels[:, column]), key
    mask, _, bits = SC.first_occurrence(labels[:, 3], epoch["n_ids"])
    assert bits == 0 and 3 < mask.sum() < n
    assert np.array_equal(got["vocab_segment"].cpu().numpy(), labels[mask, 3])
    assert got["negative_stats"] == {
        "n_test_samples": n, "n_test_vocab": len(np.unique(labels[:, 0])), "n_test_segments": len(np.unique(labels[:, 3])),
        "n_neg_samples": 30, "n_neg_segments": len(np.unique(labels[:30, 3]))}
    # the ranking: fp64 margins first, then equal hit counts
    trues = epoch["outputs"][torch.from_numpy(mask)]
    hits64 = SC.assert_margins(epoch["estimates"].numpy(), trues.numpy(), labels[:, 3], labels[mask, 3], TOPKS, "end to end")
    print("end to end", got["acc"], {k: v / n for k, v in hits64.items()})
    assert set(got["acc"]) == set(TOPKS)
    for k in TOPKS:
        assert int(round(got["acc"][k] * n)) == hits64[k] and got["acc"][k] == pytest.approx(hits64[k] / n, abs=1e-9)
    assert hits64[1] <= hits64[5] <= hits64[10] and 0 < hits64[10]
    # segment_topk_accuracy over the de-duplicated arrays: the first occurrences' own predictions
    dedup = retrieval.segment_topk_accuracy(ClipLoss().cuda(), epoch["estimates"][torch.from_numpy(mask)], trues,
                                            torch.from_numpy(labels[mask, 3]), topks=TOPKS, batch_size=16)
    margins = {k: SC.ranking_margins(epoch["estimates"].numpy()[mask], trues.numpy(), labels[mask, 3], labels[mask, 3], k)
               for k in TOPKS}
    for k in TOPKS:
        assert dedup[f"top{k}"] == pytest.approx(sum(h for h, _ in margins[k]) / int(mask.sum()), abs=1e-6)
    # blocked against the materialised matrix
    full, _ = run_eval(epoch, topks=TOPKS, probs_batch_size=16, return_probs=True)
    assert tuple(full["probs_segment"].shape) == (n, int(mask.sum())) and "probs_segment" not in got
    for k in TOPKS:
        assert int(round(full["acc"][k] * n)) == hits64[k]
    assert torch.equal(full["vocab_segment"], got["vocab_segment"])
    whole, _ = run_eval(epoch, topks=TOPKS, probs_batch_size=1000)
    assert whole["acc"] == got["acc"]


def test_n_recordings_and_study(epoch):
    """``n_recordings=1`` is the run over ``segments.only(0)``; ``test_study`` picks the other recording."""
    one, seen_one = run_eval(epoch, n_recordings=1, topks=(1, 5))
    only, seen_only = run_eval(epoch, segments=epoch["seg"].only(0), topks=(1, 5))
    assert one["acc"] == only["acc"] and one["negative_stats"] == only["negative_stats"]
    assert torch.equal(seen_one["preds"], seen_only["preds"]) and torch.equal(seen_one["labels"], seen_only["labels"])
    labels = epoch["labels"]
    n0 = int((labels[:, 5] == 0).sum())
    assert len(seen_one["labels"]) == n0 and 0 < n0 < len(labels)
    assert np.array_equal(seen_one["labels"][:, [0, 1, 2, 4, 5, 6]].cpu().numpy(), labels[labels[:, 5] == 0][:, [0, 1, 2, 4, 5, 6]])
    _, seen_study = run_eval(epoch, test_study="study1", topks=(1,))
    assert len(seen_study["labels"]) == len(labels) - n0 and bool((seen_study["labels"][:, 5] == 1).all())


def test_a_regression_solver_ranks_with_its_own_clip_loss(epoch):
    """scripts/run_eval_probs.py:318-322: a solver whose loss is not a ClipLoss builds one from ``clip=``."""
    from brainmagick_amd.losses import L2Loss
    got, seen = run_eval(epoch, solver=make_solver(L2Loss()), topks=(1, 5), clip={})
    want, seen_clip = run_eval(epoch, topks=(1, 5))
    assert torch.equal(seen["preds"], seen_clip["preds"]) and got["acc"] == want["acc"]


def test_segments_without_word_information_are_refused(epoch):
    seg, builder, _ = make_segments(columns=False)
    from brainmagick_amd import retrieval
    with pytest.raises(ValueError, match="word_index / sequence_id"):
        retrieval.segment_eval_epoch(make_solver(), seg, builder, ["Mel"], batch_size=7)


def test_not_built_host_spill_names_the_bytes(epoch, monkeypatch):
    """The labels are part of what has to fit: 7 int64 per row, next to the two fp32 arrays."""
    from brainmagick_amd import retrieval
    monkeypatch.setattr(retrieval, "_free_bytes", lambda device: 1000)
    n = len(epoch["seg"])
    need = n * 4 * (8 * 37 + 8 * 37) + n * 8 * 7
    with pytest.raises(NotImplementedError, match=f"Not built.*{need} bytes.*1000 bytes"):
        run_eval(epoch)


def test_solver_segment_eval_is_pure_dispatch(epoch, monkeypatch):
    from brainmagick_amd import retrieval
    calls = []
    monkeypatch.setattr(retrieval, "segment_eval_epoch", lambda solver, segments, **kw: calls.append((solver, segments, kw))
                        or {"acc": {1: 0.25}})
    solver = make_solver()
    kw = dict(test_features=epoch["builder"], used_names=["Mel"], batch_size=7, topks=(1,))
    assert solver.segment_eval(epoch["seg"], **kw) == {"acc": {1: 0.25}}
    assert calls == [(solver, epoch["seg"], kw)]
