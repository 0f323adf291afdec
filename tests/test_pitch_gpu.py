"""The Pitch feature on the GPU: ``bm_yin_pitch`` (csrc/pitch.hip) through ``hip_ops.yin_pitch`` and
``audio.DevicePitch``, against the fixture of the live reference (tests/golden/make_audio_rates_golden.py) and the
direct-form restatement of tests/audio_cases.py.  The fixture's maker asserts that no comparison of any of its frames is
closer than 1e-9 (the kernel's fp64 sums differ from the reference's FFT form near 1e-13), so the pitches are compared
for equality."""
import numpy as np
import pytest
import torch

import audio_cases as AC
import features_cases as FC
from test_segments_gpu import bits

pytestmark = pytest.mark.gpu

FX = AC.fixture()
PITCH_CASES = [(c["params"], c["signal"]) for c in FX["meta"]["pitch"]]


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def signal(name: str) -> torch.Tensor:
    return torch.from_numpy(FX[f"signal/{name}"])


@pytest.mark.parametrize("params", sorted(AC.PITCH_PARAMS))
def test_the_fixture_s_pitches_exactly(H, params):
    kw = AC.yin_kwargs(AC.PITCH_PARAMS[params])
    names = [s for p, s in PITCH_CASES if p == params]
    assert len(names) == (5 if params == "default" else 2)
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        outs = H.yin_pitch([signal(n).cuda() for n in names], 16_000, **kw)
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["yin_pitch"]                            # one launch for all of them
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1                  # carved from one allocation
    for name, out in zip(names, outs):
        want = FX[f"pitch/{params}/{name}"]
        assert out.dtype == torch.float32 and tuple(out.shape) == (1, len(want)), name
        got = out.cpu().numpy()[0]
        print(f"pitch {params}/{name}: {len(want)} frames, {int((want > 0).sum())} voiced, {int((got != want).sum())} differ")
        assert np.array_equal(got, want), name
        alone, = H.yin_pitch([signal(name).cuda()], 16_000, **kw)
        assert torch.equal(bits(out), bits(alone)), name                             # among others and alone


def test_frame_counts_at_the_boundary_lengths(H):
    outs = H.yin_pitch([signal(n).cuda() for n in ("len_w1", "len_ws", "len_ws1")])
    assert [tuple(o.shape) for o in outs] == [(1, 1), (1, 1), (1, 2)]
    with pytest.raises(ValueError, match="L > w_len"):
        H.yin_pitch([signal("voiced")[:256].cuda()])


def test_silent_and_non_finite_frames_give_zero(H):
    x = signal("voiced")[:4000].clone()
    clean, = H.yin_pitch([x.cuda()])
    starts = torch.arange(clean.shape[1]) * 64
    assert bool((clean.cpu()[0] > 0).float().mean() > 0.9)
    silent = x.clone()
    silent[1000:2000] = 0.0
    got, = H.yin_pitch([silent.cuda()])
    inside = (starts >= 1000) & (starts + 256 <= 2000)
    assert int(inside.sum()) == 12 and bool((got.cpu()[0][inside] == 0).all())
    assert bool((H.yin_pitch([torch.zeros(1000).cuda()])[0] == 0).all())
    for value in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 1777, 3999 - ((4000 - 256 - 1) % 64) - 1):                   # the first sample, the middle, the last frame
            bad = x.clone()
            bad[at] = value
            got, = H.yin_pitch([bad.cuda()])
            holds = (starts <= at) & (at < starts + 256)
            assert int(holds.sum()) >= 1
            assert bool((got.cpu()[0][holds] == 0).all()), (value, at)               # exactly the frames that contain it
            assert torch.equal(bits(got.cpu()[0, ~holds]), bits(clean.cpu()[0, ~holds])), (value, at)


def test_misaligned_waveforms_and_guarded_outputs(H):
    from test_guard_bands_gpu import Arena
    from test_resample_gpu import shifted_copy
    waves = [signal("len_w1"), signal("len_ws1"), signal("voiced")[:4001], signal("mixed")[3000:8000]]
    want = H.yin_pitch([w.cuda() for w in waves])
    shifted = [shifted_copy(w) for w in waves]
    arena = Arena()
    with arena.active():
        got = H.yin_pitch(shifted)
    arena.check("yin_pitch")
    for g, w in zip(got, want):
        assert not bool(torch.isnan(g).any())                   # every element of the poisoned allocation was written
        assert torch.equal(bits(g), bits(w))


def test_a_resampled_sound_through_the_builder_and_a_train_step(H):
    from brainmagick_amd import synthetic
    from brainmagick_amd.audio import DevicePitch
    from brainmagick_amd.features import DeviceEvents, DeviceFeaturesBuilder
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    sr, T = 120.0, 87
    pitch = DevicePitch(sr)
    stereo = AC.stereo_441(22_050, 5).cuda()                                         # 0.5 s at 44.1 kHz
    second = AC.stereo_441(17_640, 6)[0].contiguous().cuda()                         # 0.4 s, mono
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        arrays = pitch.compute([stereo, second], 44_100, resample=True)
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["resample_frac", "yin_pitch"]
    assert [tuple(a.shape) for a in arrays] == [(1, 121), (1, 96)]                   # len(range(0, 8000 - 256, 64)), ... 6400
    # the restatement applied to the kernel's own resampled waveforms
    at16 = H.resample_frac([torch.mean(stereo, dim=0), second], 44_100, 16_000)
    for a, w in zip(arrays, at16):
        want, margin = AC.yin_direct(w.cpu().numpy(), 16_000, **AC.yin_kwargs(AC.PITCH_PARAMS["default"]))
        assert margin >= 1e-9, margin                           # else equality would not be a legitimate test of this input
        assert np.array_equal(a.cpu().numpy()[0], want) and bool((want > 0).mean() > 0.8)
    with pytest.raises(ValueError, match="resample=True"):
        pitch.compute([stereo], 44_100)
    same, = pitch.compute([at16[1]], 16_000)
    assert torch.equal(bits(same), bits(arrays[1]))

    builder = DeviceFeaturesBuilder([pitch.feature()], sr)
    host = dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], Pitch=[a.cpu().numpy() for a in arrays]))
    events = DeviceEvents(builder, dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], Pitch=arrays)))
    assert events.sources[0][0][0].data_ptr() == arrays[0].data_ptr()                # read in place
    table = H.EventTable(builder.plan(), len(builder.kinds), builder.mask_kind, [(events.kind_tables, events.sources)], "cuda")
    times = [FC.window_times(s, T, sr) for s in (0, 60)]
    rec = torch.zeros(2, dtype=torch.int32, device="cuda")
    wstart = torch.tensor([t[0] for t in times], dtype=torch.float64, device="cuda")
    wdur = torch.tensor([t[1] for t in times], dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 2, T, sr, flag)
    specs = [FC.feature("Pitch", "resampled", "sound", 1, default_value=0.0)]
    want = np.stack([FC.build_window(specs, False, host, *t, sr, T)[0] for t in times])
    assert torch.equal(bits(feats), bits(torch.from_numpy(want))) and int(flag.item()) == 0
    assert bool((feats[0, :, 75:] == 0).all()) and bool((feats[0, :, 20:60] > 100).any())

    batch = synthetic.make_batch(2, 8, T, 1, 2, seed=7)
    batch.features, batch.features_mask = feats, mask
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": 8}, out_channels=1, hidden={"meg": 16}, n_subjects=2, depth=2, kernel_size=3,
                       merger=False, subject_layers=False, subject_dim=0)
    loss = Solver(model, loss=L2Loss()).train_step(batch.to("cuda"))
    assert bool(torch.isfinite(loss))
