"""The segment dataset without a GPU: the window selection against the live reference's (tests/golden/segments.json,
made by tests/golden/make_segments_golden.py from bm/dataset.py:113-157), the window / baseline arithmetic restated from
mne's documentation, the loader's order against torch's own samplers, the C-ABI and the ISA audit of segments.hip."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
SELECTION_KEYS = ("n_samples", "sample_rate", "tmin", "tmax", "condition", "blocks", "ignore_start_in_block",
                  "ignore_end_in_block")
CASES = json.loads((GOLDEN / "segments.json").read_text())["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_selection_equals_the_reference(case):
    from brainmagick_amd.dataset import event_samples, segment_starts
    kw = {k: case[k] for k in SELECTION_KEYS}
    expected = np.asarray(case["samples"] or [], dtype=np.int64)       # null: the reference logged "Empty dataset"
    got = event_samples(**kw)
    assert got.dtype == np.int64 and got.tolist() == expected.tolist()
    # repeated event samples are dropped, keeping the first (mne's event_repeated='drop'), the order stays;
    # the window starts round(tmin * sample_rate) after the event
    seen, kept = set(), []
    for s in expected.tolist():
        if s not in seen:
            seen.add(s)
            kept.append(s + int(np.round(case["tmin"] * case["sample_rate"])))
    assert segment_starts(**kw).tolist() == kept


def test_the_fixture_has_the_cases_it_is_meant_to_have():
    by_name = {c["name"]: c for c in CASES}
    assert by_name["too_short"]["samples"] is None and by_name["too_short_events"]["samples"] is None
    dup = by_name["unsorted_duplicated"]["samples"]
    assert len(set(dup)) < len(dup) and dup != sorted(dup)
    for sr in (120, 50):        # half-way indices round to even: 20.5 -> 20, 21.5 -> 22
        assert by_name[f"half_way_sr{sr}"]["samples"][:4] == [20, 22, 22, 24]
    sizes = {n: len(c["samples"]) for n, c in by_name.items() if n.startswith("blocks_two")}
    assert len(set(sizes.values())) == 4, sizes                       # each ignore_* switch changes the selection


def test_empty_blocks_are_refused_and_a_condition_must_be_a_stride_or_times():
    from brainmagick_amd.dataset import segment_starts
    with pytest.raises(ValueError):
        segment_starts(1000, 120., -0.5, 2.5, 3.0, blocks=[])
    with pytest.raises(TypeError):
        segment_starts(1000, 120., -0.5, 2.5, "word")


@pytest.mark.parametrize("sr,tmin,tmax,baseline,T,window", [
    (120., -0.5, 2.5, (None, 0), 361, (0, 60)),
    (20., -0.2, 0.4, (None, 0), 13, (0, 4)),
    (20., -0.2, 0.35, (-0.1, 0.1), 12, (2, 6)),
    (20., -0.2, 0.4, None, 13, None),
])
def test_window_and_baseline_samples(sr, tmin, tmax, baseline, T, window):
    from brainmagick_amd.dataset import window_samples
    assert window_samples(sr, tmin, tmax, baseline) == (T, window)


def test_a_baseline_outside_the_window_is_refused():
    from brainmagick_amd.dataset import window_samples
    with pytest.raises(ValueError):
        window_samples(20., 0.1, 0.4, (None, 0))
    with pytest.raises(ValueError):
        window_samples(20., -0.2, 0.4, (-0.1, 0.5))


def _segments(n=23):
    """A DeviceSegments of exactly ``n`` segments over two CPU-resident recordings (no GPU: never gathered)."""
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    n0 = n // 2
    lens = [n0, n - n0]
    recs = [DeviceRecording(torch.zeros(2 + i, 10 * k + 13), recording=Recording(i, torch.rand(2 + i, 2)), subject_index=i,
                            device="cpu") for i, k in enumerate(lens)]
    seg = DeviceSegments(recs, 20., tmin=-0.2, tmax=0.4, condition=0.5)
    assert len(seg) == n, (len(seg), n)
    return seg


def test_loader_order_is_the_random_samplers():
    from torch.utils.data import RandomSampler
    from brainmagick_amd.dataset import DeviceSegmentLoader
    seg = _segments(23)
    loader = DeviceSegmentLoader(seg, 5, shuffle=True, generator=torch.Generator().manual_seed(7))
    sampler = RandomSampler(range(23), generator=torch.Generator().manual_seed(7))
    assert len(loader) == 5
    for _ in range(2):                                     # the generator advances from epoch to epoch on both sides
        assert loader.indices() == list(sampler)
    plain = DeviceSegmentLoader(seg, 5)
    assert plain.indices() == list(range(23))


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_order_is_the_distributed_samplers(drop_last, shuffle):
    from torch.utils.data import DataLoader, DistributedSampler
    from brainmagick_amd.dataset import DeviceSegmentLoader
    seg = _segments(23)
    seen = []
    for rank in range(3):
        loader = DeviceSegmentLoader(seg, 5, shuffle=shuffle, seed=11, rank=rank, world=3, drop_last=drop_last)
        sampler = DistributedSampler(range(23), num_replicas=3, rank=rank, shuffle=shuffle, seed=11,
                                     drop_last=drop_last)
        assert len(loader) == len(DataLoader(range(23), batch_size=5, sampler=sampler))
        for epoch in (0, 1):
            loader.set_epoch(epoch)
            sampler.set_epoch(epoch)
            order = loader.indices()
            assert order == list(sampler) and len(order) == (7 if drop_last else 8)
            seen.append(order)
    if shuffle:
        assert seen[0] != seen[1]                          # set_epoch reshuffles


def test_meg_dimension_below_a_recording_is_an_assertion():
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    rec = DeviceRecording(torch.zeros(5, 100), recording=Recording(0, torch.rand(5, 2)), subject_index=0, device="cpu")
    with pytest.raises(AssertionError):
        DeviceSegments([rec], 20., tmin=-0.2, tmax=0.4, condition=0.5, meg_dimension=4)


def test_a_window_one_sample_past_the_end_is_dropped_as_mne_drops_it():
    """The reference's edge mask compares times: 11.5 -> 12 and 7.5 -> 8 both round upward and the window 12 .. 20 of a
    20-sample recording stays selected.  mne drops such an epoch as too short; DeviceSegments drops the window."""
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments, event_samples, window_samples
    from brainmagick_amd.synthetic import Recording
    times = [0.575, 0.2]
    assert window_samples(20., 0., 0.375, None) == (9, None)
    assert event_samples(20, 20., 0., 0.375, times).tolist() == [12, 4]
    rec = DeviceRecording(torch.zeros(2, 20), recording=Recording(0, torch.rand(2, 2)), subject_index=0, device="cpu")
    seg = DeviceSegments([rec], 20., tmin=0., tmax=0.375, baseline=None, condition=times)
    assert seg.start.tolist() == [4] and seg.rec.tolist() == [0]


def test_there_is_no_cpu_fallback():
    seg = _segments(23)                                    # recordings in host memory
    with pytest.raises(RuntimeError):
        seg.batch([0, 1])


def test_segment_gather_is_declared_defined_and_exported():
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    for name in ("bm_segment_gather", "bm_segment_table_fill", "bm_segment_table_entry_bytes"):
        assert name in protos, name
        assert hasattr(_lib.lib(), name), name
    _, argtypes, argnames = protos["bm_segment_gather"]
    assert argnames[:4] == ["table", "R", "rec", "start"] and argnames[-3:] == ["dst", "flag", "stream"]
    assert "out" not in argnames and "inplace" not in argnames
    text = (ROOT / "brainmagick_amd" / "csrc" / "segments.hip").read_text()
    assert re.search(r'extern\s+"C"\s+int\s+bm_segment_gather\s*\(', text)
    header = (ROOT / "include" / "bm_hip.h").read_text()
    assert re.search(r"bm/dataset\.py:\d+", header[header.index("segments.hip"):header.index("bm_segment_gather(")])
    L = _lib.lib()
    # argument checks that need no device: no launch for an empty batch, refusals with a message
    assert L.bm_segment_gather(None, 0, None, None, 0, 0, 0, 4, 13, -1, -1, 4, None, None, None) == 0
    assert L.bm_segment_gather(None, 1, None, None, 4, 2, 3, 4, 13, -1, -1, 4, None, None, None) != 0      # 2 + 3 > 4
    assert L.bm_segment_gather(None, 1, None, None, 4, 0, 3, 4, 13, 0, 13, 4, None, None, None) != 0       # baseline end = T
    assert L.bm_segment_gather(None, 1, None, None, 4, 0, 3, 4, 13, 0, 4, 1, None, None, None) != 0        # bytes: no baseline
    assert L.bm_segment_gather(None, 1, None, None, 4, 0, 3, 4, 13, -1, -1, 2, None, None, None) != 0      # element size
    assert L.bm_segment_gather(None, 1, None, None, 4, 0, 3, 4, 13, -1, -1, 4, None, None, None) != 0      # null pointers


def test_segment_kernels_are_free_of_spills_and_scratch(tmp_path):
    """ISA audit: every kernel of segments.hip, compiled for gfx950, spills no register and has no private segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "segments.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    "-o", str(out), str(csrc / "segments.hip")], check=True, capture_output=True)
    text = out.read_text()
    names = [l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "_kernel" in l]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(set(names)) == 3 and len(spills) == 3 and len(scratch) == 3, names
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (names, spills, scratch)
