"""The GPU-resident segment dataset: ``bm_segment_gather`` (csrc/segments.hip) against an fp64 restatement of what the
reference's loader computes (``mne.Epochs`` holds float64, subtracts the baseline mean, the reference rounds with
``.float()``; bm/dataset.py:172-175, 349-364) -- a restatement, not mne -- and ``DeviceSegments`` / ``DeviceSegmentLoader``
into the scaler fit and the Solver.

Base case: three recordings of 5, 8 and 3 channels and 97, 64 and 130 samples at 20 Hz, a per-channel offset of 1e3 times
the spread (the baseline mean matters), padded to ``meg_dimension`` 8, 3 feature rows, 1 mask row.

The MEG bound, per element:  |ours - truth| <= 2^-24 |truth| + 2^-40 max|row| + 2^-149  -- half an ulp of the final
rounding, plus the reordering error of an fp64 mean of at most T terms ((T - 1) 2^-53 max|row| < 2^-40 max|row| for
T <= 4096, the kernel's limit).  Derived, not measured.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHANNELS, LENGTHS, MEG_DIM, SR = (5, 8, 3), (97, 64, 130), 8, 20.
GUARD = 256                         # poisoned elements on either side of a carved tensor
# (tmin, tmax, baseline in seconds) -> (T, baseline window): the forms of tests/test_segments_cpu.py at 20 Hz
FORMS = {
    "T13_none_0": ((-0.2, 0.4, (None, 0)), 13, (0, 4)),
    "T12_inner": ((-0.2, 0.35, (-0.1, 0.1)), 12, (2, 6)),
    "T13_off": ((-0.2, 0.4, None), 13, None),
    "T12_off": ((-0.2, 0.35, None), 12, None),
    "T12_none_0": ((-0.2, 0.35, (None, 0)), 12, (0, 4)),
    "T13_whole": ((-0.2, 0.4, (None, None)), 13, (0, 12)),
}


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def make_arrays(n_features=3, seed=20, mask_density=0.7):
    """The base case on the CPU: per recording (meg [C_r, N], features [F, N], mask [1, N] bool)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c, n in zip(CHANNELS, LENGTHS):
        meg = torch.randn(c, n, generator=g) + 1e3 * torch.randn(c, 1, generator=g)
        out.append((meg, torch.randn(n_features, n, generator=g), torch.rand(1, n, generator=g) < mask_density))
    return out


@pytest.fixture(scope="module")
def arrays():
    return make_arrays()


def event_times(tmin, T):
    """Event times (one array for every recording; each keeps what fits) whose windows start at raw sample 0 and end at
    the last sample of every recording (and one sample too far: the selection drops those), and a few in between."""
    starts = sorted({0, 7, 18, 30, 51} | {n - T for n in LENGTHS} | {n - T + 1 for n in LENGTHS})
    return [(s - int(np.round(tmin * SR))) / SR for s in starts]


def make_segments(arrays, form):
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    (tmin, tmax, baseline), T, window = FORMS[form]
    lg = torch.Generator().manual_seed(5)
    recs = []
    for i, (meg, feats, mask) in enumerate(arrays):
        recs.append(DeviceRecording(meg.cuda(), feats.cuda(), mask.cuda(),
                                    recording=Recording(10 + i, torch.rand(len(meg), 2, generator=lg)), subject_index=2 - i))
    seg = DeviceSegments(recs, SR, tmin=tmin, tmax=tmax, baseline=baseline, condition=event_times(tmin, T),
                         meg_dimension=MEG_DIM)
    assert (seg.T, seg.baseline) == (T, window)
    return seg


def truth(arrays, rec, start, T, window):
    """(meg fp64 [B, 8, T] before the final rounding, max|row| [B, 8, 1], features, mask) by slicing."""
    meg, rowmax, feats, masks = [], [], [], []
    for r, s in zip(rec, start):
        x = arrays[r][0][:, s:s + T].double()
        if window is not None:
            x = x - x[..., window[0]:window[1] + 1].mean(-1, keepdim=True)
        pad = MEG_DIM - x.shape[0]
        meg.append(torch.nn.functional.pad(x, (0, 0, 0, pad)))
        rowmax.append(torch.nn.functional.pad(arrays[r][0][:, s:s + T].double().abs().amax(-1, keepdim=True), (0, 0, 0, pad)))
        feats.append(arrays[r][1][:, s:s + T])
        masks.append(arrays[r][2][:, s:s + T])
    return torch.stack(meg), torch.stack(rowmax), torch.stack(feats), torch.stack(masks)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8)


def assert_meg(got, want64, rowmax, what=""):
    got = got.detach().cpu().double()
    bound = 2.0 ** -24 * want64.abs() + 2.0 ** -40 * rowmax + 2.0 ** -149
    err = (got - want64).abs()
    worst = float((err / bound).max())
    print(what, "worst error / bound:", worst)
    assert bool((err <= bound).all()), (what, worst)


def pick_indices(seg):
    """7 segments: for every recording the window at raw sample 0 and the one that ends at its last sample (the
    64-sample recording is listed once more: a repeated segment), in an order that mixes the recordings."""
    idx = []
    for r, n in enumerate(LENGTHS):
        for s in (0, n - seg.T):
            hit = np.nonzero((seg.rec == r) & (seg.start == s))[0]
            assert len(hit) == 1, (r, s, seg.start[seg.rec == r])
            idx.append(int(hit[0]))
    idx = [idx[4], idx[0], idx[3], idx[1], idx[5], idx[2], idx[3]]
    assert len(idx) == 7 and len(set(idx)) == 6
    return idx


@pytest.mark.parametrize("form", list(FORMS))
def test_values(arrays, form):
    seg = make_segments(arrays, form)
    assert all(((seg.rec == r) & (seg.start == n - seg.T + 1)).sum() == 0 for r, n in enumerate(LENGTHS))   # one too far: dropped
    idx = pick_indices(seg)
    batch = seg.batch(idx)
    rec, start = seg.rec[idx].tolist(), seg.start[idx].tolist()
    want64, rowmax, feats, masks = truth(arrays, rec, start, seg.T, seg.baseline)
    assert batch.meg.shape == (7, MEG_DIM, seg.T) and batch.meg.dtype == torch.float32
    assert batch.features.shape == (7, 3, seg.T) and batch.features_mask.shape == (7, 1, seg.T)
    assert batch.features_mask.dtype == torch.bool
    if seg.baseline is None:
        assert torch.equal(bits(batch.meg), bits(want64.float()))                  # the slices, bit for bit
    else:
        assert_meg(batch.meg, want64, rowmax, form)
        assert float(want64.abs().max()) < 50 and float(rowmax.max()) > 500        # the mean mattered
    for b, r in enumerate(rec):                                                    # padded channels: +0.0
        assert not bits(batch.meg[b, CHANNELS[r]:]).any()
    assert torch.equal(bits(batch.features), bits(feats))
    assert torch.equal(batch.features_mask.cpu(), masks)
    assert batch.subject_index.dtype == batch.recording_index.dtype == torch.int64 and batch.subject_index.is_cuda
    assert batch.recording_index.tolist() == [10 + r for r in rec]
    assert batch.subject_index.tolist() == [2 - r for r in rec]
    assert [r.recording_index for r in batch._recordings] == [10 + r for r in rec]


@pytest.mark.parametrize("form", ["T13_none_0", "T12_inner"])
def test_determinism(H, arrays, form):
    seg = make_segments(arrays, form)
    idx = pick_indices(seg)
    first = seg.batch(idx)
    again = seg.batch(idx)
    assert torch.equal(bits(first.meg), bits(again.meg))
    for b, i in enumerate(idx):                            # alone: another place in the span (other grids: test_many_workgroups)
        alone = seg.batch([i])
        assert torch.equal(bits(alone.meg[0]), bits(first.meg[b])), b
        assert torch.equal(bits(alone.features[0]), bits(first.features[b])), b
    try:
        for mode in ("f16x2", "f32x3", "f32"):
            H.set_compute_dtype(mode)
            assert torch.equal(bits(seg.batch(idx).meg), bits(first.meg)), mode
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def test_non_finite(arrays):
    nan, inf = float("nan"), float("inf")
    poisoned = [tuple(t.clone() for t in rec) for rec in arrays]
    poisoned[0][0][1, 2] = nan           # recording 0, window at 0: inside the baseline window 0..4
    poisoned[0][0][3, 9] = nan           # outside it
    poisoned[0][0][4, 11] = inf
    poisoned[1][0][6, 63] = -inf         # recording 1, window at 51 (T = 13): its last sample, outside the baseline
    seg = make_segments(poisoned, "T13_none_0")
    idx = pick_indices(seg)
    batch = seg.batch(idx)
    rec, start = seg.rec[idx].tolist(), seg.start[idx].tolist()
    meg = batch.meg.cpu()
    clean64, rowmax, _, _ = truth(arrays, rec, start, seg.T, seg.baseline)
    expect_nan = torch.zeros_like(meg, dtype=torch.bool)
    expect_inf = torch.zeros_like(meg)
    for b, (r, s) in enumerate(zip(rec, start)):
        if (r, s) == (0, 0):
            expect_nan[b, 1, :] = True
            expect_nan[b, 3, 9] = True
            expect_inf[b, 4, 11] = inf
        if (r, s) == (1, 51):
            expect_inf[b, 6, 12] = -inf
    assert expect_nan.sum() == 14 and (expect_inf != 0).sum() == 3              # (1, 51) is the repeated segment
    assert torch.equal(torch.isnan(meg), expect_nan)
    assert torch.equal(torch.where(torch.isinf(meg), meg, torch.zeros_like(meg)), expect_inf)
    finite = ~expect_nan & (expect_inf == 0)
    assert_meg(torch.where(finite, meg, torch.zeros_like(meg)), torch.where(finite, clean64, torch.zeros_like(clean64)),
               rowmax, "finite rest")
    # without a baseline the bits pass through: -0.0 and a NaN's payload included
    poisoned[2][0][0, 5] = -0.0
    poisoned[2][0][1, 6] = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)[0]
    seg = make_segments(poisoned, "T13_off")
    idx = pick_indices(seg)
    got = seg.batch(idx).meg
    b = seg.rec[idx].tolist().index(2)
    assert seg.start[idx][b] == 0 and int(bits(got)[b, 0, 5]) == -2 ** 31
    assert torch.equal(bits(got), bits(torch.stack([torch.nn.functional.pad(poisoned[r][0][:, s:s + 13], (0, 0, 0, MEG_DIM - CHANNELS[r]))
                                                     for r, s in zip(seg.rec[idx].tolist(), seg.start[idx].tolist())])))


class Carver:
    """Tensors carved out of larger poisoned buffers (NaN for fp32, 0xFF bytes otherwise) at an offset of ``shift``
    elements past a 16-byte boundary: 4-byte aligned fp32 rows that are not 16-byte aligned."""

    def __init__(self):
        self.blocks = []

    def empty(self, shape, dtype, shift):
        n = int(np.prod(shape))
        if dtype == torch.float32:
            raw = torch.full((GUARD + shift + n + GUARD,), float("nan"), device="cuda")
        else:
            raw = torch.full((GUARD + shift + n + GUARD,), -1, device="cuda", dtype=torch.int8).view(torch.uint8) \
                if dtype in (torch.bool, torch.uint8) else torch.full((GUARD + shift + n + GUARD,), -1, device="cuda", dtype=dtype)
        assert raw.data_ptr() % 16 == 0
        body = raw[GUARD + shift:GUARD + shift + n]
        self.blocks.append((raw, GUARD + shift, n))
        return (body.view(torch.bool) if dtype == torch.bool else body).view(shape)

    def place(self, t, shift=1):
        dst = self.empty(tuple(t.shape), t.dtype, shift)
        dst.copy_(t)
        return dst

    def check(self):
        torch.cuda.synchronize()
        for raw, lo, n in self.blocks:
            for band in (raw[:lo], raw[lo + n:]):
                ok = torch.isnan(band).all() if raw.dtype == torch.float32 else (band.view(torch.uint8) == 0xFF).all()
                assert bool(ok), "a store landed in a guard band"


@pytest.mark.parametrize("form", ["T13_none_0", "T12_inner", "T12_off"])
def test_guard_bands(H, arrays, form):
    """Sources, index arrays and outputs inside poisoned bands, every fp32 tensor 4- but not 16-byte aligned; windows
    at the first and the last sample of every recording, hence of its first and last row."""
    (_, _, _), T, window = FORMS[form]
    carver = Carver()
    meg_t = H.SegmentTable([carver.place(a[0], 1 + i) for i, a in enumerate(arrays)])
    feat_t = H.SegmentTable([carver.place(a[1], 3 - i) for i, a in enumerate(arrays)])
    mask_t = H.SegmentTable([carver.place(a[2], 1) for a in arrays])
    for t in meg_t.arrays + feat_t.arrays:
        assert t.data_ptr() % 16 != 0 and t.data_ptr() % 4 == 0
    rec = [0, 2, 1, 1, 0, 2, 1, 0, 2]
    start = [0, 130 - T, 0, 64 - T, 97 - T, 0, 64 - T, 33, 70]
    first, B = 2, len(rec)                                  # the batch is an offset into longer arrays
    rec_d = carver.place(torch.tensor([7, -3] + rec + [9], dtype=torch.int32), 1)
    start_d = carver.place(torch.tensor([10 ** 6, -5] + start + [10 ** 6], dtype=torch.int32), 3)
    flag = carver.empty((1,), torch.int32, 1)
    flag.zero_()
    meg = H.segment_gather(meg_t, rec_d, start_d, first, B, MEG_DIM, T, flag, baseline=window,
                           dest=carver.empty((B, MEG_DIM, T), torch.float32, 1))
    feats = H.segment_gather(feat_t, rec_d, start_d, first, B, 3, T, flag, dest=carver.empty((B, 3, T), torch.float32, 3))
    mask = H.segment_gather(mask_t, rec_d, start_d, first, B, 1, T, flag, dest=carver.empty((B, 1, T), torch.bool, 1))
    carver.check()
    assert int(flag.item()) == 0
    want64, rowmax, wf, wm = truth(arrays, rec, start, T, window)
    assert not torch.isnan(meg).any() and not torch.isnan(feats).any()          # no element was left out
    assert bool((mask.view(torch.uint8) <= 1).all())
    if window is None:
        assert torch.equal(bits(meg), bits(want64.float()))
    else:
        assert_meg(meg, want64, rowmax, form)
    assert torch.equal(bits(feats), bits(wf)) and torch.equal(mask.cpu(), wm)


@pytest.mark.parametrize("form", ["T13_none_0", "T12_off"])
def test_range_check(H, arrays, form):
    """rec = R, rec = -1, start = -1 and start = N_r - T + 1 among valid segments: zeros, the flag, nothing else.  (The
    kernel checks before it forms an address: sg_row_source in csrc/segments.hip.)"""
    (_, _, _), T, window = FORMS[form]
    carver = Carver()
    meg_t = H.SegmentTable([carver.place(a[0], 1) for a in arrays])
    mask_t = H.SegmentTable([carver.place(a[2], 1) for a in arrays])
    rec = [0, 3, 1, -1, 2, 1, 0, 2]
    start = [5, 0, 51 if T == 13 else 52, 0, -1, 64 - T + 1, 97 - T, 130 - T]
    bad = [1, 3, 4, 5]
    rec_d = carver.place(torch.tensor(rec, dtype=torch.int32), 1)
    start_d = carver.place(torch.tensor(start, dtype=torch.int32), 1)
    flag = carver.empty((1,), torch.int32, 1)
    flag.zero_()
    valid = [b for b in range(len(rec)) if b not in bad]
    # valid segments alone leave the flag down
    ok_rec = carver.place(torch.tensor([rec[b] for b in valid], dtype=torch.int32), 1)
    ok_start = carver.place(torch.tensor([start[b] for b in valid], dtype=torch.int32), 1)
    H.segment_gather(meg_t, ok_rec, ok_start, 0, len(valid), MEG_DIM, T, flag, baseline=window)
    assert int(flag.item()) == 0
    meg = H.segment_gather(meg_t, rec_d, start_d, 0, len(rec), MEG_DIM, T, flag, baseline=window,
                           dest=carver.empty((len(rec), MEG_DIM, T), torch.float32, 1))
    assert int(flag.item()) == 1
    flag.zero_()
    mask = H.segment_gather(mask_t, rec_d, start_d, 0, len(rec), 1, T, flag, dest=carver.empty((len(rec), 1, T), torch.bool, 3))
    assert int(flag.item()) == 1
    carver.check()
    assert not bits(meg[bad]).any() and not mask[bad].view(torch.uint8).any()   # +0.0 / False, bit for bit
    want64, rowmax, _, wm = truth(arrays, [rec[b] for b in valid], [start[b] for b in valid], T, window)
    if window is None:
        assert torch.equal(bits(meg[valid]), bits(want64.float()))
    else:
        assert_meg(meg[valid], want64, rowmax, form)
    assert torch.equal(mask[valid].cpu(), wm)


# Several workgroups.  At T = 13 a workgroup of the fp32 kernel owns 256 rows, more than any launch above has.  At T = 87
# (tmin -0.2, tmax 4.1 at 20 Hz) it owns RB = 4096 // 87 = 47 rows = 4089 elements: 20 segments x 8 channels are four
# workgroups, the last one of 19 rows; 4089 % 4 = 1, so every workgroup shifts its LDS image differently and their spans
# meet in the middle of 16-byte groups (4-byte head and tail stores); 4089 > 2048 samples, so the staging loop and the
# store loop both go round more than once; the mask launch has 1 740 bytes, seven workgroups of the byte kernel.
WIDE_T = 87
WIDE_REC = [0, 2, 2, 0, 2, 0, 2, 2, 0, 2, 2, 0, 2, 0, 2, 2, 0, 2, 2, 0]
WIDE_START = [0, 43, 0, 10, 17, 3, 43, 29, 10, 1, 38, 7, 2, 0, 41, 11, 5, 30, 43, 9]


@pytest.mark.parametrize("window", [(0, 4), (2, 86), None], ids=["none_0", "inner", "off"])
def test_many_workgroups(H, arrays, window):
    from brainmagick_amd.dataset import window_samples
    T = WIDE_T
    assert window_samples(SR, -0.2, 4.1, (None, 0)) == (T, (0, 4))
    RB = 4096 // T
    B = len(WIDE_REC)
    assert (RB * T) % 4 == 1 and RB * T > 2048 and -(-B * MEG_DIM // RB) == 4 and (B * MEG_DIM) % RB == 19
    assert -(-B * 3 // RB) == 2 and B * T > 256 * 6
    assert {(0, 0), (0, LENGTHS[0] - T), (2, 0), (2, LENGTHS[2] - T)} <= set(zip(WIDE_REC, WIDE_START))
    carver = Carver()
    meg_t = H.SegmentTable([carver.place(a[0], 1 + i) for i, a in enumerate(arrays)])
    feat_t = H.SegmentTable([carver.place(a[1], 3 - i) for i, a in enumerate(arrays)])
    mask_t = H.SegmentTable([carver.place(a[2], 1) for a in arrays])
    rec_d = carver.place(torch.tensor([5] + WIDE_REC, dtype=torch.int32), 1)
    start_d = carver.place(torch.tensor([-9] + WIDE_START, dtype=torch.int32), 3)
    flag = carver.empty((1,), torch.int32, 1)
    flag.zero_()
    want64, rowmax, wf, wm = truth(arrays, WIDE_REC, WIDE_START, T, window)

    def check(meg, feats, mask, rows, what):
        assert not torch.isnan(meg).any() and not torch.isnan(feats).any()      # no element was left out
        assert bool((mask.view(torch.uint8) <= 1).all())
        if window is None:
            assert torch.equal(bits(meg), bits(want64[rows].float()))
        else:
            assert_meg(meg, want64[rows], rowmax[rows], what)
        for b, r in zip(range(len(rows)), [WIDE_REC[i] for i in rows]):
            assert not bits(meg[b, CHANNELS[r]:]).any()
        assert torch.equal(bits(feats), bits(wf[rows])) and torch.equal(mask.cpu(), wm[rows])

    for shift in (1, 2, 3, 0):                             # every alignment of the output, 16-byte aligned included
        meg = H.segment_gather(meg_t, rec_d, start_d, 1, B, MEG_DIM, T, flag, baseline=window,
                               dest=carver.empty((B, MEG_DIM, T), torch.float32, shift))
        feats = H.segment_gather(feat_t, rec_d, start_d, 1, B, 3, T, flag,
                                 dest=carver.empty((B, 3, T), torch.float32, (shift + 2) % 4))
        mask = H.segment_gather(mask_t, rec_d, start_d, 1, B, 1, T, flag, dest=carver.empty((B, 1, T), torch.bool, shift))
        carver.check()
        assert int(flag.item()) == 0
        check(meg, feats, mask, list(range(B)), f"shift {shift}")
        if shift == 1:
            first = meg, feats, mask
        else:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, (meg, feats, mask)))
    # each segment alone (one workgroup, rows 0 .. 7 of its own span) has the bits it has among the others
    for b in range(B):
        alone = H.segment_gather(meg_t, rec_d, start_d, 1 + b, 1, MEG_DIM, T, flag, baseline=window)
        assert torch.equal(bits(alone[0]), bits(first[0][b])), b
    # the range check at this shape: bad segments in the first, an inner and the last workgroup
    rec, start = list(WIDE_REC), list(WIDE_START)
    bad = {0: (3, 0), 6: (2, LENGTHS[2] - T + 1), 7: (1, 0), 12: (-1, 5), 19: (0, -1)}     # recording 1 is shorter than T
    for b, (r, s0) in bad.items():
        rec[b], start[b] = r, s0
    rec_b = carver.place(torch.tensor(rec, dtype=torch.int32), 3)
    start_b = carver.place(torch.tensor(start, dtype=torch.int32), 1)
    meg = H.segment_gather(meg_t, rec_b, start_b, 0, B, MEG_DIM, T, flag, baseline=window,
                           dest=carver.empty((B, MEG_DIM, T), torch.float32, 3))
    assert int(flag.item()) == 1
    flag.zero_()
    feats = H.segment_gather(feat_t, rec_b, start_b, 0, B, 3, T, flag, dest=carver.empty((B, 3, T), torch.float32, 1))
    assert int(flag.item()) == 1
    flag.zero_()
    mask = H.segment_gather(mask_t, rec_b, start_b, 0, B, 1, T, flag, dest=carver.empty((B, 1, T), torch.bool, 1))
    assert int(flag.item()) == 1
    carver.check()
    good = [b for b in range(B) if b not in bad]
    assert not bits(meg[list(bad)]).any() and not bits(feats[list(bad)]).any() and not mask[list(bad)].view(torch.uint8).any()
    check(meg[good], feats[good], mask[good], good, "among bad segments")


def test_loader_raises_index_error_at_the_end_of_the_epoch(arrays):
    from brainmagick_amd import dataset as D
    seg = make_segments(arrays, "T13_none_0")
    seg.start = seg.start.copy()
    seg.start[3] = 10 ** 6                                  # behind the host's validation
    loader = D.DeviceSegmentLoader(seg, 4)
    seen = 0
    with pytest.raises(IndexError):
        for batch in loader:
            seen += 1
            if seen == 1:
                assert not bits(batch.meg[3]).any()
    assert seen == len(loader)                              # every batch was delivered; the check came last
    assert int(D.range_error_flag(seg.device).item()) == 0  # and cleared the flag


def test_loader_epoch(H, arrays, monkeypatch):
    from torch.utils.data import RandomSampler
    from brainmagick_amd import dataset as D
    seg = make_segments(arrays, "T13_none_0")
    n = len(seg)
    assert n > 8 and n % 4 != 0                             # a ragged last batch
    order = list(RandomSampler(range(n), generator=torch.Generator().manual_seed(3)))
    loader = D.DeviceSegmentLoader(seg, 4, shuffle=True, generator=torch.Generator().manual_seed(3))
    received, real = [], H.segment_gather

    def spy(table, rec, start, first, count, *args, **kw):
        received.append((rec.data_ptr(), start.data_ptr(), first, count))
        return real(table, rec, start, first, count, *args, **kw)
    monkeypatch.setattr(H, "segment_gather", spy)
    batches = list(loader)
    monkeypatch.setattr(H, "segment_gather", real)
    assert loader.order == order and len(batches) == len(loader) == -(-n // 4)
    # the index arrays of the epoch went up once: every launch of the epoch received those very arrays and an offset
    ep = loader.epoch_arrays
    assert len(received) == 3 * len(batches)
    assert {(r, s) for r, s, _, _ in received} == {(ep["rec"].data_ptr(), ep["start"].data_ptr())}
    assert [f for _, _, f, _ in received[::3]] == list(range(0, n, 4))
    assert ep["rec"].tolist() == seg.rec[order].tolist() and ep["start"].tolist() == seg.start[order].tolist()
    for k, batch in enumerate(batches):
        idx = order[4 * k:4 * k + 4]
        want = seg.batch(idx)
        assert len(batch) == len(idx)
        assert torch.equal(bits(batch.meg), bits(want.meg)) and torch.equal(bits(batch.features), bits(want.features))
        assert torch.equal(batch.features_mask, want.features_mask)
        assert torch.equal(batch.recording_index, want.recording_index)
        assert torch.equal(batch.subject_index, want.subject_index)
        assert batch.recording_index.tolist() == [10 + int(seg.rec[i]) for i in idx]
        pos = batch.positions()
        assert pos.shape == (len(idx), MEG_DIM, 2)
        for b, i in enumerate(idx):
            layout = seg.recordings[int(seg.rec[i])].recording.layout
            assert torch.equal(pos[b, :len(layout)], layout) and bool((pos[b, len(layout):] == -0.1).all())


def test_into_the_scaler_fit_and_the_solver():
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    from brainmagick_amd.solver import Solver
    seg = make_segments(make_arrays(n_features=4, mask_density=2.), "T13_none_0")     # ClipLoss takes an all-true mask
    ours = [list(loader) for loader in seg.per_recording_loaders(4, generator=torch.Generator().manual_seed(1))]
    assert len(ours) == 3 and all(len({int(i) for b in batches for i in b.recording_index}) == 1 for batches in ours)
    moved = [[b.to("cpu").to("cuda") for b in batches] for batches in ours]
    fitted = DeviceBatchScaler.fit(ours, None)
    expect = DeviceBatchScaler.fit(moved, None)
    assert torch.equal(fitted.meg_center, expect.meg_center) and torch.equal(fitted.meg_scale, expect.meg_scale)
    assert fitted.meg_center.shape == (13, MEG_DIM) and float(fitted.meg_center[10:, :3].abs().min()) > 0

    cfg = dict(depth=4, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2, glu_context=1,
               complex_out=True, merger=True, merger_pos_dim=128, merger_channels=24, merger_dropout=0.0,
               initial_linear=24, subject_layers=True, subject_dim=0)

    def solver():
        torch.manual_seed(0)
        model = SimpleConv(in_channels={"meg": MEG_DIM}, out_channels=4, hidden={"meg": 8}, n_subjects=3, **cfg)
        return Solver(model, ClipLoss(), scale_reject=ScaleReject(fitted, clip=True))

    from brainmagick_amd.dataset import DeviceSegmentLoader
    batch = next(iter(DeviceSegmentLoader(seg, 6, shuffle=True, generator=torch.Generator().manual_seed(2))))
    host = batch.to("cpu")
    a, b = solver(), solver()
    assert a.stage(batch) is batch
    assert b.stage(host) is not host
    loss_a = a.train_step(batch)
    loss_b = b.train_step(host)
    assert bool(torch.isfinite(loss_a)) and torch.equal(bits(loss_a.reshape(1).float()), bits(loss_b.reshape(1).float()))
