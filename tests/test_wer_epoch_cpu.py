"""CPU-only checks of the ClipLoss test epoch (bm/wer.py:21-80): the word-label rule restated in tests/wer_cases.py,
``extract_features`` / ``get_slice`` / ``check_at_time`` and the choice of recordings against the fixture the live
reference wrote (tests/golden/wer_epoch.npz), every ``ValueError`` of ``word_hash_pick``, what is not built, the new
symbol in header and library, and the ISA audit of wer.hip."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import features_cases as FC
import wer_cases as WC
from helpers import Golden

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def golden():
    return Golden("wer_epoch")


def make_builder(meta):
    specs = [FC.feature(name, "constant", "word", cardinality=meta["cardinality"][name]) for name in meta["features"]]
    return FC.make_builder(specs, meta["sample_rate"])


def test_fixture_holds_the_numpy_pick_rule(golden):
    """The labels the reference's torch.where chain produced (bm/wer.py:58-66) are what the numpy restatement gives:
    check_at_time 0, 1, 2, 6 and 10, rejected rows, a fully rejected batch; the reference's assert fires exactly where
    the restatement raises the all-zero bit."""
    meta = golden.meta
    seen = set()
    for name, case in meta["cases"].items():
        t0 = case["check_at_time"]
        labels, bits, decided = [], 0, set()
        for b in WC.fixture_batches(golden.raw, meta, name):
            got, bb = WC.pick(b["features"][:, 2], t0, b["keep"])
            labels.append(got)
            bits |= bb
            decided.update(WC.decisive(b["features"][r, 2], t0) for r in np.flatnonzero(b["keep"]))
        assert bool(bits & WC.ALL_ZERO_BIT) == case["assert_fired"], name
        assert not bits & ~WC.ALL_ZERO_BIT, name
        if case["assert_fired"]:
            continue
        assert np.array_equal(np.concatenate(labels), golden.raw[f"{name}/word_hashes"]), name
        assert decided == {k for k, t in enumerate(WC.positions(t0)) if t is not None}, name
        assert int(np.abs(golden.raw[f"{name}/word_hashes"]).max()) <= 2 ** 24
        seen.add(t0)
    assert seen == {0, 1, 2, 6, 10}
    assert any(c["assert_fired"] for c in meta["cases"].values())


def test_pick_rule_flags_and_guards():
    """The restatement itself: the two guards (a missing one would read the row's last samples), -0.0 is zero, a NaN is
    taken, and the three ways a value is no label."""
    row = np.zeros((1, 13), dtype=np.float32)
    row[0, 12], row[0, 11], row[0, 2] = 7, 8, 9
    assert WC.pick(row, 0)[0].tolist() == [9] and WC.decisive(row[0], 0) == 4
    row[0, 1] = -0.0
    assert WC.pick(row, 0)[0].tolist() == [9]
    assert WC.pick(row, 1)[0].tolist() == [9] and WC.pick(row, 1)[1] == 0
    for bad, label in ((np.nan, 0), (np.inf, 0), (2.0 ** 63, 0), (0.5, 0), (-3.5, -3)):
        row[0, 5] = bad
        got, bits = WC.pick(row, 5)
        assert got.tolist() == [label] and bits == WC.VALUE_BIT, bad
    row[0, 5] = -(2.0 ** 62)
    assert WC.pick(row, 5)[0].tolist() == [-2 ** 62] and WC.pick(row, 5)[1] == 0
    got, bits = WC.pick(np.zeros((2, 13), dtype=np.float32), 6, [False, True])
    assert got.tolist() == [0] and bits == WC.ALL_ZERO_BIT


def test_check_at_time_against_fixture(golden):
    from brainmagick_amd import retrieval
    for name, case in golden.meta["cases"].items():
        tmin = case["test_tmin"] if case["test_tmin"] is not None else case["tmin"]          # bm/wer.py:43-45
        assert retrieval.check_at_time(tmin, golden.meta["sample_rate"]) == case["check_at_time"], name
        assert WC.check_at_time(tmin, golden.meta["sample_rate"]) == case["check_at_time"], name


def test_get_slice_and_extract_features_against_fixture(golden):
    """``get_slice`` gives the reference builder's channels; ``extract_features`` gives, bit for bit, the tensor the
    reference's ``extract_features`` handed its ``_process_batch`` -- names in the builder's order (one leading run: a
    contiguous copy of the view) and swapped (one cat)."""
    meta = golden.meta
    builder = make_builder(meta)
    assert builder.dimension == meta["dimension"]
    for name, (start, stop) in meta["slices"].items():
        assert builder.get_slice(name) == slice(start, stop)
    orders = set()
    for name, case in meta["cases"].items():
        if case["assert_fired"]:
            continue
        orders.add(tuple(case["names"]))
        for b in WC.fixture_batches(golden.raw, meta, name):
            full = torch.from_numpy(b["features"].copy())
            got = builder.extract_features(full, case["names"])
            assert got.is_contiguous() and got.shape == (len(full), 2, meta["T"])
            assert got.data_ptr() != full.data_ptr() or got.shape == full.shape
            if b["output"] is not None:
                assert torch.equal(got[torch.from_numpy(b["keep"])], torch.from_numpy(b["output"])), name
    assert len(orders) == 2
    full = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    assert torch.equal(builder.extract_features(full, ["WordLength", "WordFrequency", "WordHash"]), full)
    assert torch.equal(builder.extract_features(full, ["WordHash", "WordLength"]), full[:, [2, 0]])
    assert torch.equal(builder.extract_features(full, ["WordFrequency"]), full[:, 1:2])
    with pytest.raises(AssertionError):
        builder.extract_features(full[:, :2], ["WordLength"])                    # "Input should contain all features"
    with pytest.raises(AssertionError):
        builder.extract_features(full, ["WordLength", "Phoneme"])
    with pytest.raises(KeyError):
        builder.get_slice("Phoneme")


def _cpu_segments(studies):
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    recordings = [DeviceRecording(torch.zeros(2, 40 if i != 1 else 400), recording=Recording(i, torch.zeros(2, 2), study),
                                  subject_index=i, device="cpu") for i, study in enumerate(studies)]
    return DeviceSegments(recordings, 10., tmin=-0.2, tmax=0.5, baseline=None, condition=1.0)


def test_wer_recordings_and_study_against_fixture(golden):
    """bm/wer.py:28-35: the study filter, then the first ``wer_recordings``; the order stays the dataset's."""
    from brainmagick_amd import retrieval
    meta = golden.meta
    segments = _cpu_segments(meta["studies"])
    assert all((segments.rec == i).any() for i in range(len(meta["studies"])))
    for name, case in meta["cases"].items():
        if case["assert_fired"]:
            continue
        sub = retrieval.wer_segments(segments, case["wer_recordings"], case["wer_study"])
        assert sorted(set(sub.rec.tolist())) == case["datasets"], name
        keep = np.isin(segments.rec, case["datasets"])
        assert np.array_equal(sub.rec, segments.rec[keep]) and np.array_equal(sub.start, segments.start[keep])
    assert any(c.get("datasets") not in (None, [0, 1, 2, 3]) for c in meta["cases"].values())
    # "the first N recordings that have segments": a recording too short for a window does not count
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    recs = [DeviceRecording(torch.zeros(2, n), recording=Recording(i, torch.zeros(2, 2)), subject_index=0, device="cpu")
            for i, n in enumerate((5, 40, 40))]
    short_first = DeviceSegments(recs, 10., tmin=-0.2, tmax=0.5, baseline=None, condition=1.0)
    assert not (short_first.rec == 0).any()
    assert set(retrieval.wer_segments(short_first, 1).rec.tolist()) == {1}
    only = segments.only(2)
    assert np.array_equal(only.rec, segments.subset([2]).rec) and np.array_equal(only.start, segments.subset([2]).start)


def test_every_value_error_before_any_launch():
    """Raised from the shapes alone -- on CPU tensors, in front of the "no CPU fallback" error."""
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd._lib import BmHipError
    x = torch.zeros(4, 3, 13)
    dest = torch.zeros(10, dtype=torch.int64)
    flag = torch.zeros(1, dtype=torch.int32)
    bad = [dict(check_at_time=-1), dict(check_at_time=11), dict(check_at_time=13), dict(c=-1), dict(c=3),
           dict(n0=-1), dict(n0=7), dict(n0=8, count=3), dict(count=5), dict(count=-1)]
    for kw in bad:
        args = dict(c=2, check_at_time=6, n0=0, count=None)
        args.update(kw)
        with pytest.raises(ValueError, match="word_hash_pick"):
            H.word_hash_pick(x, args["c"], args["check_at_time"], None, dest, args["n0"], flag, count=args["count"])
    with pytest.raises(ValueError, match="B, F_all, T"):
        H.word_hash_pick(x[0], 2, 6, None, dest, 0, flag)
    for ok in (dict(n0=6), dict(n0=8, count=2), dict(check_at_time=0), dict(check_at_time=10)):
        args = dict(c=2, check_at_time=6, n0=0, count=None)
        args.update(ok)
        H.word_hash_pick_check(x.shape, args["c"], args["check_at_time"], dest.numel(), args["n0"], args["count"])
        with pytest.raises(BmHipError, match="no CPU"):                          # valid arguments: only the GPU is missing
            H.word_hash_pick(x, args["c"], args["check_at_time"], None, dest, args["n0"], flag, count=args["count"])


def test_not_built_more_than_one_rank(monkeypatch):
    from brainmagick_amd import distrib, retrieval
    monkeypatch.setattr(distrib, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="Not built.*more than one rank"):
        retrieval.wer_epoch(None, None, None, [], batch_size=4)


def test_wer_epoch_refuses_a_window_without_room_before_anything_runs(golden):
    """check_at_time + 2 past the window: ``ValueError`` before the loader is built or the models are touched."""
    from brainmagick_amd import retrieval
    from brainmagick_amd.losses import ClipLoss
    import types
    builder = make_builder(golden.meta)
    segments = _cpu_segments(golden.meta["studies"])
    segments.n_features = builder.dimension
    solver = types.SimpleNamespace(loss=ClipLoss())
    assert segments.T == 8
    for tmin in (-0.4, 0.3):                                 # int(0.4 * 10) + 2 = 6: 6 + 2 >= 8;  int(-3.0) + 2 = -1
        with pytest.raises(ValueError, match="check_at_time"):
            retrieval.wer_epoch(solver, segments, builder, ["WordLength"], batch_size=4, tmin=tmin)
    with pytest.raises(ValueError, match="feature channels"):
        segments.n_features = 7
        retrieval.wer_epoch(solver, segments, builder, ["WordLength"], batch_size=4)


def test_header_and_library_carry_the_new_symbol():
    import ctypes
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    assert "bm_word_hash_pick" in protos
    restype, argtypes, argnames = protos["bm_word_hash_pick"]
    assert restype is ctypes.c_int
    assert argnames == ["x", "B", "F", "T", "c", "t0", "mask", "dest", "dest_len", "n0", "flag", "stream"]
    assert argtypes[8] is ctypes.c_long and argtypes[9] is ctypes.c_long and argtypes[0] is ctypes.c_void_p
    assert hasattr(_lib.lib(), "bm_word_hash_pick")
    # argument errors come back as codes before anything is launched (no GPU is touched)
    handle = _lib.lib()
    assert handle.bm_word_hash_pick(None, 4, 3, 13, 2, 11, None, None, 10, 0, None, None) == 1001
    assert handle.bm_word_hash_pick(None, 4, 3, 13, 3, 6, None, None, 10, 0, None, None) == 1001
    assert handle.bm_word_hash_pick(None, 4, 3, 13, 2, 6, None, None, 10, 11, None, None) == 1001
    assert handle.bm_word_hash_pick(None, 0, 3, 13, 2, 6, None, None, 10, 0, None, None) == 0


def test_wer_kernel_is_free_of_spills_and_scratch(tmp_path):
    """ISA audit: the kernel of wer.hip, compiled for gfx950, spills no register and has no private segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "wer.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    str(csrc / "wer.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    names = [l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "kernel" in l]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(set(names)) == 1 and len(spills) == 2 and len(scratch) == 1, names
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (names, spills, scratch)
