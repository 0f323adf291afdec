"""The MEG preprocessing on the GPU: ``bm_fir_rows`` (csrc/fir.hip) through ``hip_ops.fir_rows`` / ``highpass_filter``,
``hip_ops.resample_rows``, ``dataset.preprocess_meg`` and ``DeviceRecording.from_raw``.

Inputs come from seeded generators with a DC offset of 100 x the spread (why one high-passes).  The truth of the FIR is
the direct sum in fp64 with the same fp32 taps (an fp64 product of the unfolded padded rows with the taps, on the device).
An output may be off by
    gamma(ntaps + 2) S[t]       with  S = (|taps| conv |x|)[t],  gamma(n) = n u / (1 - n u),  u = 2^-24,
the bound of a sum of ``ntaps`` fp32 products in any order (Higham, Accuracy and Stability, section 3.1: gamma(n) for n
terms; the two extra roundings leave room for the second-order terms), plus ``u |truth[t]|`` with ``subtract`` (the one
rounding of ``x - s``).  The project's usual ``(ntaps + 3) u`` is below ``gamma(ntaps)`` from about 9000 taps on.  The
bound is derived, not measured.  Every figure is printed before it is asserted (``pytest -s``).

Measured on an MI355X: the largest error is 0.17 of the bound (17 taps; 0.11 at 3, 0.073 at 67, 0.015 at one chunk of
taps, 0.0066 at 9601 taps); ``resample_rows`` 0.024 (10/1) and 0.026 (25/3) of the resampler's bound; ``preprocess_meg``
on the fixture's cases at most 0.023 of twice the stage bounds.
"""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import audio_cases as AC
import preprocess_cases as PC
from test_segments_gpu import bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def gamma(n: int) -> float:
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def make_rows(rows: int, T: int, seed: int) -> torch.Tensor:
    """[rows, T] fp32 on the CPU: unit-spread noise around a DC offset of +-100 and more, another one per row."""
    g = torch.Generator().manual_seed(seed)
    dc = 100.0 * (1.0 + torch.arange(rows, dtype=torch.float32))[:, None] * (1 - 2 * (torch.arange(rows) % 2))[:, None]
    return dc + torch.randn(rows, T, generator=g)


def make_taps(ntaps: int, seed: int = 9) -> torch.Tensor:
    """``ntaps`` fp32 taps of both signs with a sum of 1 (a filter with a DC gain, like the windowed sinc)."""
    g = torch.Generator().manual_seed(seed + ntaps)
    taps = torch.randn(ntaps, generator=g) + 0.5
    return (taps / taps.sum()).float()


def direct64(x: torch.Tensor, taps: torch.Tensor):
    """``(s, S)`` fp64 on the device: the direct sum over the replicate-padded rows of the device tensor ``x`` [rows, T]
    and ``(|taps| conv |x|)``; the windows are multiplied 256 MiB at a time."""
    ntaps = taps.numel()
    half = (ntaps - 1) // 2
    xp = F.pad(x.double()[:, None], (half, half), mode="replicate")[:, 0]
    win = xp.unfold(1, ntaps, 1)                                # [rows, T, ntaps], a view
    t64 = taps.double()
    step = max(1, (1 << 25) // (ntaps * x.shape[0]))
    s, S = [], []
    for a in range(0, x.shape[1], step):
        w = win[:, a:a + step].contiguous()
        s.append(w @ t64)
        S.append(w.abs() @ t64.abs())
    return torch.cat(s, 1), torch.cat(S, 1)


def check(what, got, x, s, S, ntaps, subtract):
    truth = x.double() - s if subtract else s
    bound = gamma(ntaps + 2) * S + (U * truth.abs() if subtract else 0.0)
    assert got.dtype == torch.float32 and got.shape == truth.shape and got.is_contiguous(), what
    err = (got.double() - truth).abs()
    ratio = float((err / bound).max())
    print(f"fir {what}: largest error / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


def view5(x: torch.Tensor) -> torch.Tensor:
    """``x`` [rows, T] on the device as the view ``base[..., 5:]`` of a NaN-filled ``[rows, T + 5]``."""
    base = torch.full((x.shape[0], x.shape[1] + 5), float("nan"), device="cuda")
    base[:, 5:] = x
    return base[:, 5:]


def launches(H, fn):
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        H.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def tap_counts(H):
    ch = H.fir_chunk()                                          # j = tap + column runs over ntaps + 15 values
    return [1, 3, 17, 67, ch - 17, ch - 15, ch - 13]            # ... one chunk less a tap pair, exactly, and one more


def lengths(H):
    nt = H.fir_tile()
    return [1, 2, 15, 16, 17, nt - 1, nt, nt + 1, 3 * nt + 37]


@pytest.mark.parametrize("which", range(7), ids=["1", "3", "17", "67", "chunk_less", "chunk", "chunk_more"])
def test_values_against_the_fp64_direct_sum(H, which):
    """Every length around the tile for one number of taps; 3 rows through the view ``[..., 5:]``, both ``subtract``."""
    ntaps = tap_counts(H)[which]
    assert ntaps % 2 == 1
    taps = make_taps(ntaps).cuda()
    worst = 0.0
    for T in lengths(H):
        x = view5(make_rows(3, T, 1000 + T).cuda())
        assert T == 1 or not x.is_contiguous()
        s, S = direct64(x, taps)
        for subtract in (False, True):
            got, names = launches(H, lambda: H.fir_rows(x, taps, subtract=subtract))
            assert names == ["fir_rows"]
            worst = max(worst, check(f"ntaps={ntaps} T={T} subtract={subtract}", got, x, s, S, ntaps, subtract))
            assert torch.equal(bits(got), bits(H.fir_rows(x.contiguous(), taps, subtract=subtract)))   # ... and in place
    print(f"fir ntaps={ntaps}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("T", ["3000", "tile_plus_1"])
def test_a_tenth_of_a_hertz_at_120(H, T):
    """half = 4800: five chunks of taps; at T = 3000 the padding dominates every window."""
    T = 3000 if T == "3000" else H.fir_tile() + 1
    cutoff = 0.1 / 120
    taps, half = H.lowpass_taps(cutoff, 8, "cuda")
    assert half == 4800
    x = view5(make_rows(3, T, 77).cuda())
    s, S = direct64(x, taps)
    low = H.fir_rows(x, taps)
    check(f"half=4800 T={T} lowpass", low, x, s, S, 2 * half + 1, False)
    high = H.highpass_filter(x, cutoff)
    check(f"half=4800 T={T} highpass", high, x, s, S, 2 * half + 1, True)
    assert torch.equal(bits(high), bits(x - low))               # the subtraction is one rounding of the same sum
    assert float(high.abs().max()) < 10.0                       # the offsets of 100 and more are gone


@pytest.mark.parametrize("cutoff,half", [(0.25, 16), (0.0625, 64), (0.5 / 120, 960)], ids=["h16", "h64", "h960"])
def test_equal_to_bm_lowpass_where_both_apply(H, cutoff, half):
    nt = H.fir_tile()
    taps, h = H.lowpass_taps(cutoff, 8, "cuda")
    assert h == half
    for T in (1, 17, nt - 1, nt + 1, 8192 - 2 * half):
        assert T + 2 * half <= 8192
        x = view5(make_rows(3, T, 500 + T).cuda())
        want = H.lowpass_filter(x, cutoff, publish_amax=False)
        got = H.fir_rows(x, taps)
        assert torch.equal(got, want), (T, float((got - want).abs().max()))
        assert torch.equal(bits(H.highpass_filter(x, cutoff)), bits(x - want)), T


def test_bits_do_not_depend_on_the_grid_or_the_tile(H):
    nt = H.fir_tile()
    T = 3 * nt + 37
    x = make_rows(3, T, 31).cuda()
    for taps in (make_taps(67).cuda(), H.lowpass_taps(0.1 / 120, 8, "cuda")[0]):
        half = (taps.numel() - 1) // 2
        for subtract in (False, True):
            y = H.fir_rows(x, taps, subtract=subtract)
            assert torch.equal(bits(y), bits(H.fir_rows(x, taps, subtract=subtract)))            # two runs
            alone = H.fir_rows(x[1:2], taps, subtract=subtract)
            assert torch.equal(bits(alone[0]), bits(y[1]))                                      # a row alone
            moved = H.fir_rows(x[:, 5:], taps, subtract=subtract)                               # the tiles move against the data
            inner = slice(half, T - 5 - half)                   # windows that touch neither end
            assert inner.stop - inner.start > 2000
            assert torch.equal(bits(moved[:, inner]), bits(y[:, inner.start + 5:inner.stop + 5])), (half, subtract)


@pytest.mark.parametrize("ntaps", [67, 1921])
def test_a_nan_stays_within_half_plus_15(H, ntaps):
    nt = H.fir_tile()
    T, half = 3 * nt + 37, (ntaps - 1) // 2
    at = nt + nt // 2 + 7                                       # a middle tile
    taps = make_taps(ntaps).cuda()
    x = make_rows(3, T, 41).cuda()
    bad = x.clone()
    bad[1, at] = float("nan")
    t = torch.arange(T)
    near, far = (t - at).abs() <= half, (t - at).abs() > half + 15
    for subtract in (False, True):
        clean = H.fir_rows(x, taps, subtract=subtract).cpu()
        got = H.fir_rows(bad, taps, subtract=subtract).cpu()
        assert not bool(torch.isfinite(got[1, near]).any())
        assert torch.equal(bits(got[1, far]), bits(clean[1, far]))
        assert torch.equal(bits(got[0]), bits(clean[0])) and torch.equal(bits(got[2]), bits(clean[2]))
        assert bool(torch.isfinite(clean).all())


def test_misaligned_rows_and_a_guarded_output(H):
    """The input one float past a 16-byte boundary with NaN around every row; the output in guarded, NaN-poisoned memory."""
    from test_guard_bands_gpu import Arena
    nt = H.fir_tile()
    for T, ntaps in ((nt + 1, 67), (333, 1921)):
        taps = make_taps(ntaps).cuda()
        x = make_rows(3, T, 51).cuda()
        stride = T + 3
        buf = torch.full((3 * stride + 8,), float("nan"), device="cuda")
        off = 1 + (-(buf.data_ptr() // 4)) % 4
        view = buf[off:off + 3 * stride].view(3, stride)[:, :T]
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 and H._uniform_rows(view) == stride
        for subtract in (False, True):
            want = H.fir_rows(x, taps, subtract=subtract)
            arena = Arena()
            with arena.active():
                got = H.fir_rows(view, taps, subtract=subtract)
            arena.check("fir_rows")
            assert bool(torch.isfinite(got).all())              # every element of the poisoned allocation was written
            assert torch.equal(bits(got), bits(want))


def test_errors_are_returned_not_launched(H):
    from brainmagick_amd import _lib
    L = _lib.lib()
    x = torch.zeros(3, 64, device="cuda")
    y = torch.full((3, 64), 7.0, device="cuda")
    taps = torch.zeros(5, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off                                                   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    cases = [
        ((p(x), 64, p(y), 3, 0, p(taps), 5, 0), "1 <= T < 2\\^31"),
        ((p(x), 2 ** 31, p(y), 3, 2 ** 31, p(taps), 5, 0), "1 <= T < 2\\^31"),
        ((p(x), 64, p(y), 65536, 64, p(taps), 5, 0), "limit is 65535"),
        ((p(x), 64, p(y), 3, 64, p(taps), 4, 0), "odd"),
        ((p(x), 64, p(y), 3, 64, p(taps), 2 * (H.FIR_MAX_HALF + 1) + 1, 0), f"limit is {H.FIR_MAX_HALF}"),
        ((p(x), 63, p(y), 3, 64, p(taps), 5, 0), "row_stride"),
        ((0, 64, p(y), 3, 64, p(taps), 5, 0), "null"),
        ((p(x, 2), 64, p(y), 3, 64, p(taps), 5, 0), "aligned"),
    ]
    import re
    for args, pattern in cases:
        code = L.bm_fir_rows(*args, stream)
        assert code != 0, pattern
        assert re.search(pattern, L.bm_last_error().decode()), (pattern, L.bm_last_error())
    assert L.bm_fir_rows(p(x), 64, p(y), 0, 64, p(taps), 5, 0, stream) == 0                   # no rows: nothing to do
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert int(L.bm_fir_max_half()) == H.FIR_MAX_HALF >= 16384
    with pytest.raises(ValueError, match="odd"):
        H.fir_rows(x, torch.zeros(4, device="cuda"))
    with pytest.raises(NotImplementedError):
        H.highpass_filter(x, 0.1, stride=2)
    with pytest.raises(NotImplementedError):
        H.highpass_filter(x, 0.1, pad=False)
    assert H.fir_rows(x[:0], taps).shape == (0, 64)
    assert torch.equal(bits(H.highpass_filter(x + 1, 0.1, fft=True)), bits(H.highpass_filter(x + 1, 0.1)))


# ---- resample_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("old,new", [(10, 1), (25, 3)], ids=["10_1", "25_3"])
def test_resample_rows_is_resample_frac_over_the_rows(H, old, new):
    L = 6000
    x = make_rows(3, L, 61)
    dev = view5(x.cuda())
    got, names = launches(H, lambda: H.resample_rows(dev, old * 40, new * 40))
    assert names == ["resample_frac"]                                                         # one launch for all rows
    r = AC.ResampleFrac(old, new)
    truth, bound = r(x.double()), (r.taps.shape[1] + 3) * U * r.magnitude(x)
    assert got.shape == truth.shape == (3, new * L // old) and got.is_contiguous() and got.dtype == torch.float32
    err = (got.cpu().double() - truth).abs()
    print(f"resample_rows {old}/{new}: largest error / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    listed = H.resample_frac([row.contiguous() for row in dev], old, new)
    assert torch.equal(bits(got), bits(torch.stack(listed)))
    same = H.resample_rows(dev, 120, 120)
    assert same is dev


# ---- preprocess_meg and DeviceRecording.from_raw ---------------------------------------------------------------------------
def test_preprocess_meg_on_the_fixture_s_cases(H):
    """Within twice the stage bounds: the resampler's ``(ntaps + 3) u (|taps| conv |x|)`` and, with a highpass, the
    FIR's ``gamma(ntaps + 2) S + u |truth|`` over the resampled rows, element by element."""
    from brainmagick_amd.dataset import preprocess_meg
    fx = PC.fixture()
    raw = torch.from_numpy(fx["raw"])
    for name, case in fx["meta"]["cases"].items():
        got, names = launches(H, lambda: preprocess_meg(raw.cuda(), case["sfreq"], case["sample_rate"], case["highpass"]))
        want64 = torch.from_numpy(fx[f"{name}/out64"])
        bound = PC.stage_bounds(raw, case)
        resampled = int(np.round(case["sfreq"])) != case["sample_rate"]
        assert names == ["resample_frac"] * resampled + ["fir_rows"] * bool(case["highpass"])   # one launch per stage
        assert got.shape == want64.shape and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
        err = (got.cpu().double() - want64).abs()
        ratio = float((err / (2 * bound)).max())
        ref32 = float(((torch.from_numpy(fx[f"{name}/out32"]).double() - want64).abs() / (2 * bound)).max())
        print(f"preprocess {name}: largest error / (2 x stage bounds) = {ratio:.4f} (the fp32 reference chain: {ref32:.4f})")
        assert bool((err <= 2 * bound).all()), (name, ratio)


def test_preprocess_meg_launch_counts_and_shortcut(H):
    from brainmagick_amd.dataset import preprocess_meg
    x = make_rows(3, 6000, 71).cuda()
    same, names = launches(H, lambda: preprocess_meg(x, 120.0, 120))
    assert same is x and names == []                                                          # the reference's (0, 0.0) key
    same, names = launches(H, lambda: preprocess_meg(x, 120.2, 120.0, 0.0))
    assert same is x and names == []
    _, names = launches(H, lambda: preprocess_meg(x, 1200.0, 120))
    assert names == ["resample_frac"]
    _, names = launches(H, lambda: preprocess_meg(x, 120.0, 120, 2.0))
    assert names == ["fir_rows"]
    both, names = launches(H, lambda: preprocess_meg(x, 1200.0, 120, 2.0))
    assert names == ["resample_frac", "fir_rows"]
    step = H.highpass_filter(H.resample_rows(x, 1200, 120), 2.0 / 120)
    assert torch.equal(bits(both), bits(step))
    from_host = preprocess_meg(x.cpu().double().numpy(), 1200.0, 120, 2.0)                    # what mne hands out
    assert torch.equal(bits(from_host), bits(both))
    for bad, match in (((x, 1000.0, 120.5), "only integer sampling rates"), ((x, 1000.0, 1200), "should be below 1000Hz"),
                       ((x, 1000.0, 120, 70.0), "above 0.5"), ((x, 1000.0, 120, -1.0), "larger than zero")):
        with pytest.raises(ValueError, match=match):
            preprocess_meg(*bad)


def test_from_raw_through_the_segment_loader(H):
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments, preprocess_meg
    from brainmagick_amd.synthetic import Recording
    g = torch.Generator().manual_seed(81)
    raws = [make_rows(c, 12_000, 90 + c).cuda() for c in (5, 8)]
    kw = [dict(recording=Recording(3 + i, torch.rand(r.shape[0], 2, generator=g)), subject_index=i)
          for i, r in enumerate(raws)]
    made = [DeviceRecording.from_raw(r, 1200.0, 120, 0.5, **k) for r, k in zip(raws, kw)]
    plain = [DeviceRecording(preprocess_meg(r, 1200.0, 120, 0.5), **k) for r, k in zip(raws, kw)]
    assert all(m.meg.shape == (r.shape[0], 1200) and m.meg.is_contiguous() for m, r in zip(made, raws))
    batches = []
    for recs in (made, plain):
        seg = DeviceSegments(recs, 120.0, tmin=-0.5, tmax=2.0, condition=1.5, meg_dimension=8)
        assert len(seg) > 4
        batches.append(seg.batch(list(range(len(seg)))))
    a, b = batches
    assert a.meg.shape[0] == len(seg) and bool(torch.isfinite(a.meg).all())
    assert torch.equal(bits(a.meg), bits(b.meg)) and torch.equal(a.recording_index, b.recording_index)
    assert float(a.meg.abs().max()) < 50.0                      # baseline-corrected windows of a high-passed recording
