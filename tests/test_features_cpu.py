"""The features builder without a GPU: the numpy restatement of its index rules (tests/features_cases.py) against the live
reference's windows (tests/golden/features_builder.npz, made by tests/golden/make_features_golden.py from
bm/features/base.py:68-122), torch's nearest rule, the host's validation, the builder's slices, the C-ABI and the ISA
audit of features.hip."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import features_cases as FC

ROOT = Path(__file__).resolve().parent.parent
CASES = FC.fixture_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference(case):
    sr = case["sample_rate"]
    for w in case["windows"]:
        ws, wdur = FC.window_times(w["first"], w["T"], sr)
        data, mask = FC.build_window(case["specs"], case["event_mask"], case["events"], ws, wdur, sr, w["T"])
        assert np.array_equal(_bits(data), _bits(w["data"])), (case["name"], w["first"], w["T"])
        assert mask.dtype == w["mask"].dtype and np.array_equal(mask, w["mask"]), (case["name"], w["first"], w["T"])


def test_the_fixture_has_the_cases_it_is_meant_to_have():
    names = {c["name"] for c in CASES}
    for sr in (120, 50):
        assert {f"{k}_sr{sr}" for k in ("words", "vector", "mel", "wav2vec", "mixed")} <= names
    by_name = {c["name"]: c for c in CASES}
    for c in CASES:
        assert {w["T"] for w in c["windows"]} == {13, 87}
    words = by_name["words_sr120"]
    assert words["event_mask"] and any(s["cardinality"] for s in words["specs"])
    assert any(not w["mask"].any() for w in words["windows"]) and any(w["mask"].all() for w in words["windows"])
    assert any(s["dimension"] == 3 for s in by_name["vector_sr50"]["specs"])
    assert all(w["mask"].all() for w in by_name["vector_sr50"]["windows"])               # no event mask: all true
    mel = by_name["mel_sr120"]
    lengths = []
    for es, ed, a in zip(mel["events"]["sound"]["start"], mel["events"]["sound"]["duration"],
                         mel["events"]["sound"]["MelSpectrum"]):
        n_e = int(round(((es + ed) - es) * 120.0))
        lengths.append(np.sign(a.shape[1] - n_e))
    assert set(lengths) == {-1, 0, 1}
    assert any((w["data"] == -5.0).all() for w in mel["windows"])                        # default: log10(1e-5)
    sound = by_name["wav2vec_sr120"]["events"]["sound"]
    assert sound["duration"].max() > 120 and sound["duration"].min() < 0.5
    assert len({s["event_kind"] for s in by_name["mixed_sr50"]["specs"]}) == 2


def test_fp32_nearest_rule_is_torch_interpolate_for_every_size_pair_up_to_300():
    """Source column min(floorf(k * (L / n)), L - 1) in fp32 == F.interpolate(mode='nearest'), every column."""
    sizes = np.arange(1, 301)
    for L in sizes:
        src = torch.arange(int(L), dtype=torch.float32)[None, None]
        for n in sizes:
            k = np.arange(n)
            rule = k if L == n else np.minimum(np.floor(k.astype(np.float32) * (np.float32(L) / np.float32(n))).astype(np.int64),
                                               L - 1)
            want = torch.nn.functional.interpolate(src, int(n))[0, 0].long().numpy()
            assert np.array_equal(rule, want), (L, n)
    # the scalar form used by the restatement is the same expression
    for L, n in ((1000, 960), (7, 300), (300, 7), (299, 300)):
        assert [FC.nearest_source(k, L, n) for k in range(n)] == \
            torch.nn.functional.interpolate(torch.arange(L, dtype=torch.float32)[None, None], n)[0, 0].long().tolist()


def _words(start, duration, **values):
    return dict(word=dict(start=start, duration=duration, **values))


def test_host_validation_names_the_first_offending_event():
    from brainmagick_amd.features import DeviceEvents
    b = FC.make_builder([FC.feature("WordLength", "constant", "word")], 120.)
    DeviceEvents(b, _words([0.1, 0.1, 0.5], [0.2, 0., 0.1], WordLength=[1, 2, 3]), device="cpu")
    with pytest.raises(ValueError, match="word event 2"):
        DeviceEvents(b, _words([0.1, 0.6, 0.5, 0.4], [0.2, 0., 0.1, 0.1], WordLength=[1, 2, 3, 4]), device="cpu")
    with pytest.raises(ValueError, match="word event 1: duration"):
        DeviceEvents(b, _words([0.1, 0.6], [0.2, -0.1], WordLength=[1, 2]), device="cpu")
    with pytest.raises(ValueError, match="no values"):
        DeviceEvents(b, _words([0.1], [0.2]), device="cpu")
    other = DeviceEvents(b, dict(sound=dict(start=[0.], duration=[-1.])), device="cpu")     # a kind no feature uses
    assert other.n_events == {"word": 0} and other.kind_tables == [None]
    with pytest.raises(ValueError, match="shape"):
        DeviceEvents(b, _words([0.1, 0.6], [0.2, 0.1], WordLength=[[1, 2], [3, 4]]), device="cpu")
    mel = FC.make_builder([FC.feature("Mel", "resampled", "sound", 2)], 120.)
    ok = np.zeros((2, 5), dtype=np.float32)
    DeviceEvents(mel, dict(sound=dict(start=[0., 1.], duration=[1., 0.005], Mel=[ok, ok])), device="cpu")     # 0.6 -> 1
    with pytest.raises(ValueError, match="sound event 1"):
        DeviceEvents(mel, dict(sound=dict(start=[0., 1.], duration=[1., 0.004], Mel=[ok, ok])), device="cpu")  # 0.48 -> 0
    with pytest.raises(ValueError, match="sound event 0: an array of shape"):
        DeviceEvents(mel, dict(sound=dict(start=[0.], duration=[1.], Mel=[np.zeros((3, 5), dtype=np.float32)])),
                     device="cpu")
    emb = FC.make_builder([FC.feature("Emb", "chunk", "sound", 2)], 120.)
    a = lambda L: np.zeros((2, L), dtype=np.float32)                                                      # noqa: E731
    DeviceEvents(emb, dict(sound=dict(start=[0., 3.], duration=[2., 0.4], Emb=[a(99), a(3)])), device="cpu")
    for L in (84, 104):                                                 # 42 and 52 per second: the bounds are open
        with pytest.raises(ValueError, match="sound event 1"):
            DeviceEvents(emb, dict(sound=dict(start=[0., 3.], duration=[2., 2.], Emb=[a(99), a(L)])), device="cpu")


def test_feature_descriptions_refuse_what_the_reference_refuses():
    from brainmagick_amd.features import DeviceFeaturesBuilder, EventFeature
    with pytest.raises(ValueError):
        EventFeature("x", "pulse", "word")
    with pytest.raises(ValueError):
        EventFeature("x", "constant", "")
    with pytest.raises(ValueError):
        EventFeature("x", "constant", "word", dimension=2, cardinality=4)
    f = EventFeature("x", "constant", "word", cardinality=4)
    assert f.categorical and not f.normalizable and f.output_dimension == 4 and f.dimension == 1
    g = EventFeature("y", "chunk", "sound", 8, normalizable=False)
    assert not g.categorical and not g.normalizable and g.output_dimension == 8
    assert EventFeature("z", "resampled", "sound", 8).normalizable
    with pytest.raises(ValueError):
        DeviceFeaturesBuilder([f, f], 120.)
    many = [EventFeature(f"f{i}", "constant", "word") for i in range(33)]
    assert DeviceFeaturesBuilder(many[:32], 120.).dimension == 32
    with pytest.raises(ValueError, match="32"):                            # the kernel's plan: refused when it is built
        DeviceFeaturesBuilder(many, 120.)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_builder_slices_are_the_references(case):
    b = FC.make_builder(case["specs"], case["sample_rate"], case["event_mask"])
    assert b.dimension == case["dimension"] and b.output_dimension == case["output_dimension"]
    for name, (s0, s1, o0, o1) in case["slices"].items():
        assert b.get_slice(name) == slice(s0, s1) and b.get_slice(name, model_output=True) == slice(o0, o1)
    with pytest.raises(KeyError):
        b.get_slice("missing")
    assert list(b) == [s["name"] for s in case["specs"]]
    kinds = {s["event_kind"] for s in case["specs"]} | ({"word"} if case["event_mask"] else set())
    assert set(b.kinds) == kinds and (b.mask_kind == b.kinds.index("word") if case["event_mask"] else b.mask_kind == -1)
    plan = b.plan()
    assert [p[2] for p in plan] == [case["slices"][s["name"]][0] for s in case["specs"]]
    assert sum(p[3] for p in plan) == case["dimension"]


def test_the_mask_needs_the_word_table_without_a_word_feature():
    b = FC.make_builder([FC.feature("Mel", "resampled", "sound", 2)], 120., event_mask=True)
    assert b.kinds == ["sound", "word"] and b.mask_kind == 1 and b.dimension == 2


def test_builder_drives_the_decoding_loss_and_the_metrics():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd import metrics as M
    from brainmagick_amd.losses import FeatureDecodingLoss
    b = FC.make_builder([FC.feature("Mel", "resampled", "sound", 3, default_value=-5.), FC.feature("Phoneme", "constant", "phoneme", cardinality=40),
                         FC.feature("WordLength", "constant", "word")], 120., event_mask=True)
    table, weights = FeatureDecodingLoss(b, None)._plan()
    assert table == ((H.FEATURE_CONTINUOUS, 0, 3, 0, -1), (H.FEATURE_CATEGORICAL, 3, 40, 3, -1),
                     (H.FEATURE_CONTINUOUS, 43, 1, 4, -1)) and weights is None
    got = [c() for c in M.metric_constructors(b)]
    assert [type(m) for m in got] == [M.L2Reg, M.OnlineCorrelation, M.ClassificationAcc, M.L2Reg, M.OnlineCorrelation]
    assert [m.name for m in got] == ["l2_Mel", "corr_Mel", "acc_Phoneme", "l2_WordLength", "corr_WordLength"]


def test_segment_features_is_declared_defined_and_exported():
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    names = ("bm_segment_features", "bm_features_table_entry_bytes", "bm_features_kind_fill", "bm_features_source_fill",
             "bm_features_array_fill")
    L = _lib.lib()
    for name in names:
        assert name in protos and hasattr(L, name), name
    _, _, argnames = protos["bm_segment_features"]
    assert argnames[:2] == ["feat_table", "feat_default"] and argnames[-4:] == ["dst", "mask", "flag", "stream"]
    text = (ROOT / "brainmagick_amd" / "csrc" / "features.hip").read_text()
    for name in names:
        assert re.search(r'extern\s+"C"\s+(int|long)\s+' + name + r"\s*\(", text), name
    assert "bm_segment_features" not in (ROOT / "brainmagick_amd" / "csrc" / "segments.hip").read_text()
    header = (ROOT / "include" / "bm_hip.h").read_text()
    section = header[header.index("features.hip"):header.index("bm_segment_features(")]
    assert re.search(r"bm/features/base\.py:\d+", section) and re.search(r"bm/features/audio\.py:\d+", section)
    assert [L.bm_features_table_entry_bytes(i) > 0 for i in range(4)] == [True, True, True, False]
    assert L.bm_version() >= 113


def _call(L, table=(0, 0, 0, 2), default=(0.,), NF=1, NK=1, mask_kind=-1, R=1, n_index=4, first=0, B=0, F=2, T=13, sr=120.):
    import ctypes
    t = (ctypes.c_int * max(len(table), 1))(*table)
    d = (ctypes.c_float * max(len(default), 1))(*default)
    return L.bm_segment_features(ctypes.addressof(t), ctypes.addressof(d), NF, NK, mask_kind, None, None, R, None, None, None,
                                 n_index, first, B, F, T, sr, None, None, None, None)


def test_argument_refusals_need_no_device():
    import ctypes
    from brainmagick_amd import _lib
    L = _lib.lib()
    assert _call(L) == 0                                                   # B = 0: no launch
    assert _call(L, table=(0, 0, 0, 2, 0, 2, 2, 3), default=(0., 1.), NF=2, F=5) == 0
    assert _call(L, B=3) != 0 and b"null pointer" in L.bm_last_error()
    assert _call(L, first=2, B=3) != 0                                     # 2 + 3 > 4
    assert _call(L, F=3) != 0                                              # the features have 2 channels
    assert _call(L, table=(0, 0, 1, 2)) != 0                               # a gap before the first channel
    assert _call(L, table=(1, 0, 0, 2)) != 0                               # kind 1 of 1
    assert _call(L, table=(0, 3, 0, 2)) != 0                               # no such rule
    assert _call(L, table=(0, 0, 0, 0), F=0) != 0                          # a feature without channels
    assert _call(L, mask_kind=1) != 0 and _call(L, mask_kind=-2) != 0
    assert _call(L, sr=0.) != 0 and _call(L, sr=float("nan")) != 0
    assert _call(L, T=0) != 0
    assert _call(L, T=4097) == 1003 and b"4096" in L.bm_last_error()       # BM_ERR_UNSUPPORTED
    assert _call(L, table=(0, 0, 0, 1) * 33, default=(0.,) * 33, NF=33, F=33) == 1003
    entry = (ctypes.c_char * 64)()
    assert L.bm_features_kind_fill(entry, None, None, None, 0) == 0
    assert L.bm_features_kind_fill(entry, None, None, None, 3) != 0
    assert L.bm_features_kind_fill(None, None, None, None, 0) != 0
    assert L.bm_features_array_fill(entry, ctypes.c_void_p(64), 0, 1.) != 0          # L < 1
    assert L.bm_features_array_fill(entry, ctypes.c_void_p(64), 1 << 31, 1.) != 0     # L >= 2^31
    assert L.bm_features_array_fill(entry, ctypes.c_void_p(66), 5, 1.) != 0          # not 4-byte aligned
    assert L.bm_features_array_fill(entry, ctypes.c_void_p(64), 5, 1.) == 0
    assert L.bm_features_source_fill(entry, ctypes.c_void_p(66)) != 0


def test_features_kernel_is_free_of_spills_and_scratch(tmp_path):
    """ISA audit: every kernel of features.hip, compiled for gfx950, spills no register and has no private segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "features.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    "-o", str(out), str(csrc / "features.hip")], check=True, capture_output=True)
    text = out.read_text()
    names = [l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "_kernel" in l]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(set(names)) == 1 and len(spills) == 2 and len(scratch) == 1, names
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (names, spills, scratch)


def _recordings(kinds):
    """Two CPU-resident recordings; ``kinds[i]``: "events" or "arrays"."""
    from brainmagick_amd.dataset import DeviceRecording
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    b = FC.make_builder([FC.feature("WordLength", "constant", "word")], 20.)
    out = []
    for i, kind in enumerate(kinds):
        kw = dict(recording=Recording(i, torch.rand(2, 2)), subject_index=i, device="cpu")
        if kind == "events":
            ev = DeviceEvents(b, _words([0.1 * (i + 1), 2.], [0.2, 0.4], WordLength=[3, 4]), device="cpu")
            out.append(DeviceRecording(torch.zeros(2, 113), events=ev, **kw))
        else:
            out.append(DeviceRecording(torch.zeros(2, 113), torch.zeros(1, 113), **kw))
    return out, b


def test_device_segments_take_events_or_arrays_not_a_mix():
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    recs, b = _recordings(["events", "arrays"])
    with pytest.raises(ValueError, match="events"):
        DeviceSegments(recs, 20., tmin=-0.2, tmax=0.4, condition=0.5)
    recs, b = _recordings(["events", "events"])
    seg = DeviceSegments(recs, 20., tmin=-0.2, tmax=0.4, condition=0.5)
    assert seg.n_features == b.dimension == 1 and seg.n_mask == 1 and len(seg.wstart) == len(seg) == len(seg.wdur)
    assert np.array_equal(seg.wstart, seg.start / 20.) and (np.round(seg.wdur * 20.) == seg.T).all()
    sub = seg.only(1)
    assert np.array_equal(sub.wstart, sub.start / 20.) and len(sub.wdur) == len(sub)
    with pytest.raises(ValueError, match="sample"):                        # the builder's rate is the segments'
        DeviceSegments(recs, 40., tmin=-0.2, tmax=0.4, condition=0.5)
    other = FC.make_builder([FC.feature("WordLength", "constant", "word")], 20.)
    recs[1] = DeviceRecording(torch.zeros(2, 113), recording=Recording(1, torch.rand(2, 2)), subject_index=1, device="cpu",
                              events=DeviceEvents(other, {}, device="cpu"))
    with pytest.raises(ValueError, match="different"):
        DeviceSegments(recs, 20., tmin=-0.2, tmax=0.4, condition=0.5)
    with pytest.raises(ValueError, match="not both"):
        DeviceRecording(torch.zeros(2, 113), torch.zeros(1, 113), recording=Recording(0, torch.rand(2, 2)), subject_index=0,
                        device="cpu", events=DeviceEvents(b, {}, device="cpu"))


def test_there_is_no_cpu_fallback():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.dataset import DeviceSegments
    recs, b = _recordings(["events", "events"])
    seg = DeviceSegments(recs, 20., tmin=-0.2, tmax=0.4, condition=0.5)
    with pytest.raises(RuntimeError):
        seg.batch([0, 1])
    with pytest.raises(RuntimeError):
        H.EventTable(b.plan(), len(b.kinds), b.mask_kind, [(r.events.kind_tables, r.events.sources) for r in recs], "cpu")
