"""CPU-only checks of the segment-level evaluation (scripts/run_eval_probs.py:27-180): the label rule and the
first-occurrence rule restated in tests/segment_eval_cases.py against the fixture the live reference wrote
(tests/golden/segment_eval.npz), every ``ValueError``, the ``DeviceEvents`` columns, the dense segment ids, the new symbols
in header and library, and the ISA audit of segment_eval.hip."""
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import features_cases as FC
import segment_eval_cases as SC
from helpers import Golden

ROOT = Path(__file__).resolve().parent.parent
T = 13


@pytest.fixture(scope="module")
def golden():
    return Golden("segment_eval")


def restated(golden, name):
    """The restatement over the fixture's batches: (labels [n, 7], n_ids, case)."""
    meta = golden.meta
    case = SC.fixture_case(golden.raw, meta, name)
    rows, n_ids = SC.dense_ids([None if t is None else t[2] for t in case["tables"]])
    tables = [None if t is None else (t[0], t[1], rows[r]) for r, t in enumerate(case["tables"])]
    out = []
    for b in case["batches"]:
        lab, bits = SC.labels(b["features"][:, 2], case["meta"]["check_at_time"], b["keep"], b["rec"], b["wstart"],
                              b["subject"], b["recording"], tables, meta["sample_rate"])
        assert bits == 0
        out.append(lab)
    return np.concatenate(out), n_ids, case


def test_fixture_holds_the_numpy_label_rule(golden):
    """Word hash, word index, sentence, subject and recording of the reference's run are the restatement's; its segment
    hashes have the equality structure of the dense ids, with every "no word" row in segment 0; each of the three hash
    positions and an all-zero row decide; the first occurrences are the reference's ``seen`` loop."""
    meta = golden.meta
    seen = set()
    for name, c in meta["cases"].items():
        got, n_ids, case = restated(golden, name)
        t0 = c["check_at_time"]
        assert len(got) == c["n_kept"]
        for column, key in ((0, "word_hashes"), (1, "word_indices"), (2, "seq_indices"), (4, "subject_id"),
                            (5, "recording_id")):
            assert np.array_equal(got[:, column], golden.raw[f"{name}/{key}"]), (name, key)
        assert np.array_equal(SC.groups(got[:, 3]), golden.raw[f"{name}/segment_groups"]), name
        no_word = golden.raw[f"{name}/word_indices"] == -1
        assert np.array_equal(got[:, 3] == 0, no_word) and np.array_equal(got[:, 6] == -1, no_word)
        assert np.array_equal(golden.raw[f"{name}/seq_indices"] == -1, no_word) and no_word.any() and not no_word.all()
        assert got[:, 3].max() < n_ids and got[~no_word, 3].min() >= 1
        decided = {SC.decisive(b["features"][r, 2], t0) for b in case["batches"] for r in np.flatnonzero(b["keep"])}
        assert decided == {-1} | {k for k, t in enumerate(SC.positions(t0)) if t is not None}, name
        assert (got[:, 0] == 0).any()                                        # an all-zero row is legal here
        mask, first_row, bits = SC.first_occurrence(got[:, 3], n_ids)
        assert bits == 0 and np.array_equal(mask, golden.raw[f"{name}/first_mask"]), name
        assert np.array_equal(golden.raw[f"{name}/segment_groups"][mask], golden.raw[f"{name}/vocab_groups"])
        assert np.array_equal(got[first_row, 3], got[:, 3]) and (~mask).sum() >= 3
        assert sum(not b["keep"].any() for b in case["batches"]) == 1        # one fully rejected batch
        assert sorted(set(np.concatenate([b["rec"] for b in case["batches"]]).tolist())) == c["datasets"]
        seen.add(t0)
    assert seen == {0, 1, 2, 6, T - 2}
    assert any(c["datasets"] != [0, 1, 2, 3] for c in meta["cases"].values())


def test_fixture_hit_counts_are_the_fp64_ranking(golden):
    """The maker's condition, re-asserted from the stored arrays: every top-k verdict is MARGIN away from the other."""
    for name, c in golden.meta["cases"].items():
        mask = golden.raw[f"{name}/first_mask"]
        hits = SC.assert_margins(golden.raw[f"{name}/estimate"], golden.raw[f"{name}/output"][mask],
                                 golden.raw[f"{name}/segment_groups"], golden.raw[f"{name}/vocab_groups"],
                                 golden.meta["topks"], name)
        assert {str(k): v for k, v in hits.items()} == c["hits"], name


def test_int_truncation_differs_from_round_at_half_samples():
    """The coverage rule is ``int()``: an onset at t0 + 0.5 covers t0, an offset at t0 + 0.5 does not; ``round`` (the
    features builder's rule) gives the opposite at an even / odd t0.  The last covering event wins, not the last event."""
    sr, s = 120.0, 45
    ws = s / sr
    for t0 in (2, 6):
        on = (s + t0 + 0.5) / sr
        assert SC.covers(on, 2 / sr, ws, sr, t0, T)
        assert not SC.covers((s + t0 - 2) / sr, (s + t0 + 0.5) / sr - (s + t0 - 2) / sr, ws, sr, t0, T)
    assert int(sr * ((s + 3.5) / sr - ws)) == 3 and round(3.5) == 4
    start = np.array([s - 3, s + 1, s + 4]) / sr
    dur = np.array([10, 1, 2]) / sr
    assert SC.word_event(start, dur, ws, sr, 2, T) == 0            # events 1 and 2 are later and do not cover column 2
    assert SC.word_event(start, dur, ws, sr, 1, T) == 1 and SC.word_event(start, dur, ws, sr, 4, T) == 2
    assert SC.word_event(start, dur, ws, sr, 7, T) == -1
    assert not SC.covers((s - 9) / sr, 5 / sr, ws, sr, 0, T)       # trunc(b) < 0: an empty span, not a wrapped slice


def test_first_occurrence_and_dense_ids_restated():
    from brainmagick_amd import retrieval
    mask, first, bits = SC.first_occurrence([3, 0, 3, 1, 0, 4], 5)
    assert mask.tolist() == [True, True, False, True, False, True] and first.tolist() == [0, 1, 0, 3, 1, 5] and bits == 0
    mask, first, bits = SC.first_occurrence([3, 9, 3, -1], 5)
    assert mask.tolist() == [True, False, False, False] and first.tolist() == [0, -1, 0, -1] and bits == SC.ID_RANGE_BIT
    info = [np.array([[0, 5], [1, 5], [0, 7]]), None, np.array([[1, 5], [2, 5], [0, 0]])]
    rows, n_ids = retrieval.dense_segment_ids(info)
    want, want_n = SC.dense_ids(info)
    assert n_ids == want_n == 6 and rows[1] is None and want[1] is None
    for a, b in zip(rows, want):
        if a is not None:
            assert a.dtype == np.int64 and a.shape[1] == 3 and np.array_equal(a, b)
    assert rows[0][1, 2] == rows[2][0, 2]                           # the same (sentence, word) in two recordings
    ids = np.concatenate([rows[0][:, 2], rows[2][:, 2]])
    assert ids.min() == 1 and sorted(set(ids.tolist())) == [1, 2, 3, 4, 5]          # 0 is kept for "no word"
    assert retrieval.dense_segment_ids([None, None]) == ([None, None], 1)


def word_events(n=3, **columns):
    return dict(word=dict(start=np.arange(n) / 10, duration=np.full(n, 0.05), WordHash=np.arange(1., n + 1), **columns))


def test_device_events_word_columns():
    from brainmagick_amd.features import DeviceEvents
    builder = FC.make_builder([FC.feature("WordHash", "constant", "word", cardinality=51)], 120.)
    plain = DeviceEvents(builder, word_events(), device="cpu")
    assert plain.word_info is None and plain.word_info_host is None
    both = DeviceEvents(builder, word_events(word_index=[0, 1, 2], sequence_id=np.array([7, 7, 2 ** 40])), device="cpu")
    assert both.word_info.dtype == torch.int64 and both.word_info.tolist() == [[0, 7], [1, 7], [2, 2 ** 40]]
    assert np.array_equal(both.word_info_host, both.word_info.numpy())
    assert both.resident_bytes() == plain.resident_bytes() + 3 * 2 * 8
    for t_a, t_b in zip(plain.kind_tables[0], both.kind_tables[0]):
        assert torch.equal(t_a, t_b)
    assert torch.equal(plain.sources[0], both.sources[0])
    for bad, match in ((dict(word_index=[0, 1, 2]), "sequence_id"), (dict(sequence_id=[0, 1, 2]), "word_index"),
                       (dict(word_index=[0, 1], sequence_id=[0, 1, 2]), "word_index"),
                       (dict(word_index=[0, 1, 2], sequence_id=[0, 1, 2, 3]), "sequence_id"),
                       (dict(word_index=[0, -1, 2], sequence_id=[0, 1, 2]), "word_index"),
                       (dict(word_index=[0, 1, 2], sequence_id=[0, 1, -5]), "sequence_id"),
                       (dict(word_index=[0, 1.5, 2], sequence_id=[0, 1, 2]), "word_index")):
        with pytest.raises(ValueError, match=match):
            DeviceEvents(builder, word_events(**bad), device="cpu")


def test_every_value_error_before_any_launch():
    """Raised from the shapes alone -- on CPU tensors, in front of the "no CPU fallback" error."""
    from brainmagick_amd import hip_ops as H
    x = torch.zeros(4, 3, T)
    dest = torch.zeros(10, 7, dtype=torch.int64)
    flag = torch.zeros(1, dtype=torch.int32)
    arrays = dict(rec=torch.zeros(4, dtype=torch.int32), wstart=torch.zeros(4, dtype=torch.float64),
                  subject_index=torch.zeros(4, dtype=torch.int64), recording_index=torch.zeros(4, dtype=torch.int64))

    class Table:
        n_kinds, device, kinds, table = 1, torch.device("cpu"), None, None

        def __len__(self):
            return 1
    events = Table()

    def call(c=2, check_at_time=6, n0=0, count=None, features=x, dest=dest, events=events, infos=events):
        H.segment_eval_labels(features, c, check_at_time, None, arrays, 0, events, 0, infos, 120., dest, n0, flag,
                              count=count)
    for kw in (dict(check_at_time=-1), dict(check_at_time=12), dict(check_at_time=13), dict(c=-1), dict(c=3),
               dict(n0=-1), dict(n0=7), dict(n0=8, count=3), dict(count=5), dict(count=-1),
               dict(dest=torch.zeros(10, dtype=torch.int64)), dict(dest=torch.zeros(10, 6, dtype=torch.int64)),
               dict(dest=torch.zeros(3, 7, dtype=torch.int64)), dict(features=x[0]), dict(events=None), dict(infos=None)):
        with pytest.raises(ValueError, match="segment_eval_labels"):
            call(**kw)
    H.segment_eval_labels_check(x.shape, 2, 11, dest.shape, 6)               # T - 2 is the last legal check_at_time
    H.segment_eval_labels_check(x.shape, 2, 0, dest.shape, 8, 2)
    with pytest.raises(ValueError, match="first_occurrence"):
        H.first_occurrence(torch.zeros(2, 2, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="n_ids"):
        H.first_occurrence(torch.zeros(2, dtype=torch.int64), -1)


def cpu_segments(builder, columns=True, studies=("alpha", "beta")):
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    extra = dict(word_index=[0, 1, 2], sequence_id=[4, 4, 4]) if columns else {}
    recs = [DeviceRecording(torch.zeros(2, 400), events=DeviceEvents(builder, word_events(**extra), device="cpu"),
                            recording=Recording(i, torch.zeros(2, 2), study), subject_index=i, device="cpu")
            for i, study in enumerate(studies)]
    return DeviceSegments(recs, 120., tmin=-0.05, tmax=0.05, baseline=None, condition=1.0)


def test_segment_eval_epoch_refuses_before_anything_runs(monkeypatch):
    from brainmagick_amd import distrib, retrieval
    from brainmagick_amd.losses import ClipLoss
    solver = types.SimpleNamespace(loss=ClipLoss())
    with_hash = FC.make_builder([FC.feature("WordLength", "constant", "word"),
                                 FC.feature("WordHash", "constant", "word", cardinality=51)], 120.)
    without = FC.make_builder([FC.feature("WordLength", "constant", "word")], 120.)
    with pytest.raises(ValueError, match="no WordHash.*not built"):
        retrieval.segment_eval_epoch(solver, None, without, ["WordLength"], batch_size=4)
    arrays = types.SimpleNamespace(builder=None, n_features=2)
    with pytest.raises(ValueError, match="no events"):
        retrieval.segment_eval_epoch(solver, arrays, with_hash, ["WordLength"], batch_size=4)
    builder = FC.make_builder([FC.feature("WordHash", "constant", "word", cardinality=51)], 120.)
    with pytest.raises(ValueError, match="word_index / sequence_id"):
        retrieval.segment_eval_epoch(solver, cpu_segments(builder, columns=False), builder, [], batch_size=4)
    segments = cpu_segments(builder)
    assert segments.T == 13
    for tmin in (-0.09, 0.03):                               # int(10.8) + 2 = 12: 12 + 1 >= 13;  int(-3.6) + 2 = -1
        with pytest.raises(ValueError, match="check_at_time"):
            retrieval.segment_eval_epoch(solver, segments, builder, [], batch_size=4, tmin=tmin)
    with pytest.raises(ValueError, match="feature channels"):
        retrieval.segment_eval_epoch(solver, segments, with_hash, ["WordLength"], batch_size=4)
    monkeypatch.setattr(distrib, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="Not built.*more than one rank"):
        retrieval.segment_eval_epoch(None, None, None, [], batch_size=4)


def test_docstrings_say_what_is_not_built():
    from brainmagick_amd import dataset, features, retrieval
    doc = retrieval.segment_eval_epoch.__doc__
    for word in ("word_strings", "word_segment_strings", "files on disk", "Evaluator", "EvalJob", "submitit", "2^24",
                 "fallback"):
        assert word in doc, word
    assert "_event_lists" not in dataset.__doc__
    assert "_event_lists" not in features.__doc__.split("Not built")[1]


def test_header_and_library_carry_the_new_symbols():
    import ctypes
    from brainmagick_amd import _lib, hip_ops, retrieval, solver
    protos = _lib.parse_header()
    restype, argtypes, argnames = protos["bm_segment_eval_labels"]
    assert restype is ctypes.c_int
    assert argnames == ["x", "B", "F", "T", "c", "t0", "mask", "rec", "wstart", "subject_index", "recording_index",
                        "n_index", "first", "kinds", "NK", "word_kind", "infos", "R", "sr", "dest", "dest_rows", "n0",
                        "flag", "stream"]
    assert argtypes[18] is ctypes.c_double and argtypes[20] is ctypes.c_long and argtypes[21] is ctypes.c_long
    assert protos["bm_first_occurrence"][2] == ["ids", "N", "n_ids", "first", "mask", "first_row", "flag", "stream"]
    assert protos["bm_segment_eval_info_entry_bytes"][0] is ctypes.c_long
    handle = _lib.lib()
    for name in ("bm_segment_eval_labels", "bm_first_occurrence", "bm_segment_eval_info_fill",
                 "bm_segment_eval_info_entry_bytes"):
        assert hasattr(handle, name), name
    assert handle.bm_segment_eval_info_entry_bytes() == 16
    # argument errors come back as codes before anything is launched (no GPU is touched)
    tail = (None, None, None, None, 4, 0, None, 1, 0, None, 1, 120.0, None, 10, 0, None, None)
    assert handle.bm_segment_eval_labels(None, 4, 3, 13, 2, 12, None, *tail) == 1001
    assert handle.bm_segment_eval_labels(None, 4, 3, 13, 3, 6, None, *tail) == 1001
    assert handle.bm_segment_eval_labels(None, 4, 3, 13, 2, 6, None, None, None, None, None, 4, 0, None, 1, 0, None, 1,
                                         120.0, None, 10, 11, None, None) == 1001
    assert handle.bm_segment_eval_labels(None, 0, 3, 13, 2, 6, None, None, None, None, None, 0, 0, None, 1, 0, None, 1,
                                         120.0, None, 10, 0, None, None) == 0
    assert handle.bm_first_occurrence(None, 2 ** 31, 4, None, None, None, None, None) == 1001
    assert handle.bm_first_occurrence(None, 0, 4, None, None, None, None, None) == 0
    for fn in (hip_ops.segment_eval_labels, hip_ops.first_occurrence, hip_ops.WordInfoTable,
               retrieval.segment_eval_epoch, retrieval.collect_segment_eval, solver.Solver.segment_eval):
        assert callable(fn)
    assert hip_ops.SEGMENT_EVAL_COLUMNS == SC.COLUMNS and len(retrieval.METADATA_KEYS) == len(SC.COLUMNS)
    assert (hip_ops.SEGMENT_EVAL_VALUE_BIT, hip_ops.SEGMENT_EVAL_DEST_BIT, hip_ops.SEGMENT_EVAL_RANGE_BIT,
            hip_ops.FIRST_OCCURRENCE_RANGE_BIT) == (SC.VALUE_BIT, SC.DEST_BIT, SC.RANGE_BIT, SC.ID_RANGE_BIT)


def test_segment_eval_kernels_are_free_of_spills_and_scratch(tmp_path):
    """ISA audit: the three kernels of segment_eval.hip, compiled for gfx950, spill no register and have no private
    segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "segment_eval.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    str(csrc / "segment_eval.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    names = [l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "kernel" in l]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(set(names)) == 3 and len(spills) == 6 and len(scratch) == 3, names
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (names, spills, scratch)
