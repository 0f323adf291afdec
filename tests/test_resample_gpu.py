"""The resampler on the GPU: ``bm_resample_frac`` (csrc/resample.hip) through ``hip_ops.resample_frac`` and
``DeviceMelSpectrum.compute(resample=True)``.

The truth of an output is the fp64 restatement on the CPU (tests/audio_cases.py: ``ResampleFrac`` on the waveform in
fp64, with the same fp32 taps); an output may be off by ``(ntaps + 3) 2^-24 (|taps| conv |x|)[n]``, the bound of a sum
of ``ntaps`` fp32 products in whatever order they are added (tests/test_lowpass_gpu.py).  The mel spectrogram behind the
resampler follows the rule of tests/test_mel_gpu.py: at most ``TOL_FACTOR`` = 4 times the deviation of the same chain in
fp32 torch ops from the fp64 chain.  Every figure is printed before it is asserted (``pytest -s``).

The three-tile case of the two 441-sample ratios needs 21 368 samples (a tile of the MFMA variant is 16 frames of 441
samples); every other waveform is shorter than 20 000.

Measured on an MI355X: the largest error is 0.018 of the bound at 441/160, 0.014 at 441/320 (MFMA), 0.059 at 3/1, 0.098 at
1/2 and 0.089 at 3/2 (fmaf chains); the mel spectrogram behind the resampler is at most 1.56 times as far from the fp64
chain as the fp32 torch chain (``n_fft`` 512; 1.40 at 100), the fixture's wiring cases 0.82 and 0.98.
"""
import math

import numpy as np
import pytest
import torch

import audio_cases as AC
import features_cases as FC
import mel_cases as MC
from test_segments_gpu import bits

pytestmark = pytest.mark.gpu

RATIOS = [(441, 160), (441, 320), (3, 1), (1, 2), (3, 2)]
IDS = [f"{o}_{n}" for o, n in RATIOS]
MEL_DEFAULTS = dict(norm_audio=True, use_log_scale=True, normalized=True, log_scale_eps=1e-5)


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def make_wave(L: int, seed: int, sr: int = 44_100) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L) / sr
    return (0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.2 * torch.randn(L, generator=g) + 0.05).float()


def lengths_of(H, old, new):
    _, _, _, width = H.resample_taps(old, new)
    tile = H.resample_frames_tile(old, new)
    one = tile * old - 1                                        # L // old + 1 = tile frames: exactly one tile
    return [1, 2, width - 1, old, old + 1, one - 1, one, one + 1, 3 * tile * old + 200]


_refs = {}


def reference(key, x, old, new):
    """(truth fp64, bound) of a waveform, computed once."""
    if key not in _refs:
        r = AC.ResampleFrac(old, new)
        ntaps = r.taps.shape[1]
        _refs[key] = (r(x.double()), (ntaps + 3) * 2.0 ** -24 * r.magnitude(x))
    return _refs[key]


def check(what, got, truth, bound):
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == truth.shape, (what, got.shape, truth.shape)
    if got.numel() == 0:
        return 0.0
    err = (got.double() - truth).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"resample {what}: largest error / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


@pytest.mark.parametrize("old,new", RATIOS, ids=IDS)
def test_values_against_the_fp64_restatement(H, old, new):
    lengths = lengths_of(H, old, new)
    assert max(lengths) < 20_000 or (old == 441 and sorted(lengths)[-2] < 20_000 and max(lengths) == 21_368)
    waves = [make_wave(L, 100 + i) for i, L in enumerate(lengths)]
    dev = [w.cuda() for w in waves]
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        outs = H.resample_frac(dev, old, new)
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["resample_frac"]                       # one launch for all of them
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1                  # carved from one allocation
    again = H.resample_frac(dev, old, new)
    worst = 0.0
    for i, (L, x) in enumerate(zip(lengths, waves)):
        assert outs[i].shape == (new * L // old,) and outs[i].is_contiguous()
        truth, bound = reference((old, new, i), x, old, new)
        worst = max(worst, check(f"{old}/{new} L={L}", outs[i], truth, bound))
        alone, = H.resample_frac([dev[i]], old, new)
        assert torch.equal(bits(outs[i]), bits(alone)), (L, "alone")
        assert torch.equal(bits(outs[i]), bits(again[i])), (L, "second run")
    print(f"resample {old}/{new}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("old,new", [(441, 160), (3, 1)], ids=["441_160", "3_1"])
def test_reduced_ratio_and_identity(H, old, new):
    x = make_wave(5000, 7).cuda()
    a, = H.resample_frac([x], old * 100, new * 100)
    b, = H.resample_frac([x], old, new)
    assert torch.equal(bits(a), bits(b))
    same, = H.resample_frac([x], 16_000, 16_000)
    assert same is x                                                                 # as julius: the input itself


@pytest.mark.parametrize("old,new", [(441, 160), (3, 2)], ids=["441_160", "3_2"])
def test_normalised_on_the_way_in(H, old, new):
    lengths = [old + 1, 5000, 9000]
    waves = [make_wave(L, 200 + i) * (1.0 + i) + 0.3 * i for i, L in enumerate(lengths)]
    dev = [w.cuda() for w in waves]
    mom = H.wave_moments(dev)
    outs = H.resample_frac(dev, old, new, moments=mom)
    mom_host = mom.cpu()
    for i, x in enumerate(waves):
        xn = ((x.double() - mom_host[i, 0]) * mom_host[i, 1]).float()                # fp64, rounded once
        assert float((xn - MC.normalise64(x)).abs().max()) <= 2 * float(np.spacing(np.float32(xn.abs().max())))
        truth, bound = reference((old, new, "norm", i), xn, old, new)
        check(f"{old}/{new} normalised L={lengths[i]}", outs[i], truth, bound)
        plain, = H.resample_frac([xn.cuda()], old, new)
        assert torch.equal(bits(outs[i]), bits(plain)), i                            # the same bits as resampling the rounded input
        alone, = H.resample_frac([dev[i]], old, new, moments=mom[i:i + 1].contiguous())
        assert torch.equal(bits(outs[i]), bits(alone)), i


@pytest.mark.parametrize("old,new", RATIOS, ids=IDS)
def test_a_nan_sample_stays_in_its_windows(H, old, new):
    _, _, _, width = H.resample_taps(old, new)
    ntaps = 2 * width + old
    L = 40 * old + 3 * width + 77
    at = L // 2 + 3
    x = make_wave(L, 300)
    bad = x.clone()
    bad[at] = float("nan")
    clean, = H.resample_frac([x.cuda()], old, new)
    got, = H.resample_frac([bad.cuda()], old, new)
    n = torch.arange(new * L // old)
    first = (n // new) * old - width                            # the window of output n: source samples [first, first + ntaps)
    covers = (first <= at) & (at < first + ntaps)
    assert 0 < int(covers.sum()) < n.numel() and int(covers.sum()) % new == 0
    got, clean = got.cpu(), clean.cpu()
    assert bool(torch.isnan(got[covers]).all())
    assert torch.equal(bits(got[~covers]), bits(clean[~covers]))


def shifted_copy(x: torch.Tensor) -> torch.Tensor:
    """``x`` on the device, one float past a 16-byte boundary, NaN on both sides."""
    buf = torch.full((x.numel() + 8,), float("nan"), device="cuda")
    off = 1 + (-(buf.data_ptr() // 4)) % 4
    view = buf[off:off + x.numel()]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("old,new", [(441, 160), (3, 1), (1, 2)], ids=["441_160", "3_1", "1_2"])
def test_misaligned_waveforms_and_guarded_outputs(H, old, new):
    from test_guard_bands_gpu import Arena
    lengths = [2, old + 1, 5003, lengths_of(H, old, new)[7]]
    waves = [make_wave(L, 400 + i) for i, L in enumerate(lengths)]
    want = H.resample_frac([w.cuda() for w in waves], old, new)
    shifted = [shifted_copy(w) for w in waves]
    H.resample_taps(old, new, device="cuda")                                          # the cached table: not the arena's
    arena = Arena()
    with arena.active():
        got = H.resample_frac(shifted, old, new)
    arena.check("resample_frac")
    for g, w in zip(got, want):
        assert not bool(torch.isnan(g).any())                   # every element of the poisoned allocation was written
        assert torch.equal(bits(g), bits(w))


# ---- DeviceMelSpectrum.compute(resample=True) --------------------------------------------------------------------------
def launches(H, fn):
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        H.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def test_launch_counts_and_the_bits_of_a_sound_at_in_sampling(H):
    from brainmagick_amd.audio import DeviceMelSpectrum
    mel = DeviceMelSpectrum(120.0)
    a441, b441 = make_wave(11_025, 1).cuda(), torch.stack([make_wave(9000, 2), make_wave(9000, 3)]).cuda()
    c8, d16 = make_wave(3000, 4, 8_000).cuda(), make_wave(4000, 5, 16_000).cuda()
    one, names = launches(H, lambda: mel.compute([a441, b441], 44_100, resample=True))
    assert names == ["wave_moments", "resample_frac", "mel_spectrogram"]              # one ratio
    assert [tuple(o.shape) for o in one] == [(40, 1 + 4000 // 128), (40, 1 + (16_000 * 9000 // 44_100) // 128)]
    two, names = launches(H, lambda: mel.compute([a441, c8, b441], [44_100, 8_000, 44_100], resample=True))
    assert names == ["wave_moments", "resample_frac", "resample_frac", "mel_spectrogram"]     # two ratios
    mix, names = launches(H, lambda: mel.compute([d16, a441, c8], [16_000, 44_100, 8_000], resample=True))
    assert names == ["wave_moments", "resample_frac", "resample_frac", "mel_spectrogram"]     # ... and a 16 kHz sound
    plain, names = launches(H, lambda: mel.compute([d16], 16_000))
    assert names == ["wave_moments", "mel_spectrogram"]
    same, names = launches(H, lambda: mel.compute([d16], 16_000, resample=True))
    assert names == ["wave_moments", "mel_spectrogram"]
    assert torch.equal(bits(mix[0]), bits(plain[0])) and torch.equal(bits(same[0]), bits(plain[0]))
    assert torch.equal(bits(one[0]), bits(two[0])) and torch.equal(bits(one[0]), bits(mix[1]))
    assert torch.equal(bits(one[1]), bits(two[2])) and torch.equal(bits(two[1]), bits(mix[2]))
    raw = DeviceMelSpectrum(120.0, norm_audio=False)
    _, names = launches(H, lambda: raw.compute([d16, a441, c8], [16_000, 44_100, 8_000], resample=True))
    assert names == ["resample_frac", "resample_frac", "mel_spectrogram"]
    with pytest.raises(ValueError, match="resample=True"):
        mel.compute([a441], 44_100)


def mel_truth(mono, sr, n_fft, n_mels, sw):
    """(truth fp64, the deviation of the same chain in fp32 torch ops from it): normalise from fp64 statistics rounded
    once (tests/test_mel_gpu.py), resample, transform, log."""
    x = MC.normalise64(mono) if sw["norm_audio"] else mono
    r = AC.ResampleFrac(sr, 16_000)
    truth = MC.finish(MC.stft_mel(r(x.double()), n_fft, n_mels, 16_000, sw["normalized"]), sw["use_log_scale"],
                      sw["log_scale_eps"])
    ref32 = MC.finish(MC.stft_mel(r(x), n_fft, n_mels, 16_000, sw["normalized"]), sw["use_log_scale"], sw["log_scale_eps"])
    return truth, MC.deviation(ref32, truth, sw["use_log_scale"])


@pytest.mark.parametrize("n_fft,n_mels", [(100, 8), (512, 40)], ids=["n_fft_100", "n_fft_512"])
def test_mel_behind_the_resampler_against_the_fp64_chain(H, n_fft, n_mels):
    from brainmagick_amd.audio import DeviceMelSpectrum
    sounds = [(make_wave(11_025, 11), 44_100), (make_wave(2000, 12, 8_000), 8_000), (make_wave(7000, 13), 44_100)]
    worst = 0.0
    for switch in (dict(), dict(norm_audio=False)):
        sw = dict(MEL_DEFAULTS, **switch)
        mel = DeviceMelSpectrum(120.0, n_mels=n_mels, n_fft=n_fft, **switch)
        got = mel.compute([w.cuda() for w, _ in sounds], [sr for _, sr in sounds], resample=True)
        for (mono, sr), g in zip(sounds, got):
            truth, ref_dev = mel_truth(mono, sr, n_fft, n_mels, sw)
            assert g.shape == truth.shape == (n_mels, 1 + (16_000 * mono.numel() // sr) // (n_fft // 4))
            dev = MC.deviation(g.cpu(), truth, True)
            print(f"mel behind the resampler n_fft={n_fft} {sr} Hz {switch}: deviation {dev:.3e}, reference side "
                  f"{ref_dev:.3e}, ratio {dev / ref_dev:.2f}")
            worst = max(worst, dev / ref_dev)
            assert dev <= MC.TOL_FACTOR * ref_dev, (sr, switch, dev, ref_dev)
    print(f"mel behind the resampler n_fft={n_fft}: worst ratio {worst:.2f}")


def test_the_fixture_s_wiring_cases(H):
    """The live reference's ``_compute`` on a stereo 44.1 kHz waveform (fp64 record = truth, fp32 record = the reference
    side): channel mean, normalisation, resampling, transform and logarithm in the reference's order."""
    from brainmagick_amd.audio import DeviceMelSpectrum
    fx = AC.fixture()
    stereo = torch.from_numpy(fx["wiring/wave"]).cuda()
    for case in fx["meta"]["wiring"]:
        if case["kind"] != "mel":
            continue
        mel = DeviceMelSpectrum(120.0, n_mels=case["n_mels"], n_fft=case["n_fft"])
        got, = mel.compute([stereo], case["sr"], resample=True)
        truth, out32 = torch.from_numpy(fx[f"wiring/{case['name']}/out64"]), torch.from_numpy(fx[f"wiring/{case['name']}/out32"])
        assert got.shape == truth.shape
        dev, ref_dev = MC.deviation(got.cpu(), truth, True), MC.deviation(out32, truth, True)
        print(f"wiring {case['name']}: deviation {dev:.3e}, reference side {ref_dev:.3e}, ratio {dev / ref_dev:.2f}")
        assert dev <= MC.TOL_FACTOR * ref_dev


def test_two_resampled_sounds_through_the_features_builder(H):
    from brainmagick_amd.audio import DeviceMelSpectrum
    from brainmagick_amd.features import DeviceEvents, DeviceFeaturesBuilder
    sr, T = 120.0, 87
    mel = DeviceMelSpectrum(sr)
    stereo = torch.stack([make_wave(22_050, 60), make_wave(22_050, 61)]).cuda()          # 0.5 s
    arrays = mel.compute([stereo, make_wave(17_640, 62).cuda()], [44_100, 44_100], resample=True)   # 0.4 s
    assert [tuple(a.shape) for a in arrays] == [(40, 63), (40, 51)]
    builder = DeviceFeaturesBuilder([mel.feature()], sr)
    host = dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], MelSpectrum=[a.cpu().numpy() for a in arrays]))
    events = DeviceEvents(builder, dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], MelSpectrum=arrays)))
    assert events.sources[0][0][0].data_ptr() == arrays[0].data_ptr()                    # read in place
    table = H.EventTable(builder.plan(), len(builder.kinds), builder.mask_kind, [(events.kind_tables, events.sources)], "cuda")
    times = [FC.window_times(s, T, sr) for s in (0, 60)]
    rec = torch.zeros(2, dtype=torch.int32, device="cuda")
    wstart = torch.tensor([t[0] for t in times], dtype=torch.float64, device="cuda")
    wdur = torch.tensor([t[1] for t in times], dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    feats, _ = H.segment_features(table, rec, wstart, wdur, 0, 2, T, sr, flag)
    specs = [FC.feature("MelSpectrum", "resampled", "sound", 40, default_value=mel.default_value)]
    want = np.stack([FC.build_window(specs, False, host, *t, sr, T)[0] for t in times])
    assert torch.equal(bits(feats), bits(torch.from_numpy(want))) and int(flag.item()) == 0
    assert bool((feats[0, :, 75:] == np.float32(mel.default_value)).all()) and bool((feats[0, :, 20:60] != np.float32(-5.0)).any())
