"""CPU-only checks of scaler fitting (brainmagick_amd/norm.py, csrc/scaler_fit.hip): which batches a fit uses, against
the batches the live reference used (tests/golden/scaler_fit.npz); the reference's asserts; the state_dict round trip;
no CPU fallback; and the new translation unit compiles for gfx950 without spills or scratch."""
import dataclasses
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from helpers import Golden

ROOT = Path(__file__).resolve().parent.parent
CASES = ["default", "per_channel", "budget"]


@dataclasses.dataclass
class FitBatch:
    meg: torch.Tensor
    features: torch.Tensor
    features_mask: torch.Tensor
    recording_index: torch.Tensor

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def fixture_loaders(g: Golden, device="cpu"):
    """The fixture's loaders: one list of batches per recording."""
    d = g.meta["dims"]
    index = g.t("in/recording_index")
    return [[FitBatch(g.t(f"in/{li}/{bi}/meg").to(device), g.t(f"in/{li}/{bi}/features").to(device),
                      g.t(f"in/{li}/{bi}/mask").to(device),
                      torch.full((d["B"],), int(index[li]), dtype=torch.long, device=device))
             for bi in range(d["batches"])] for li in range(d["recordings"])]


@pytest.mark.parametrize("case", CASES)
def test_fit_uses_the_batches_the_reference_used(case):
    """bm/norm.py:175-217: whole batches per loader until n_samples_per_recording segments were seen (the fourth batch
    stays unread); with n_samples_features, shuffled by random.Random(1234) and cut at the batch that reaches it."""
    from brainmagick_amd.norm import select_fit_batches
    g = Golden("scaler_fit")
    want = g.meta["cases"][case]
    loaders = fixture_loaders(g)
    meg, features, batches = select_fit_batches(loaders, g.meta["dims"]["n_samples_per_recording"],
                                                want["kwargs"].get("n_samples_features"))
    assert {str(k): [list(x) for x in v] for k, v in meg.items()} == want["meg"]
    assert [list(x) for x in features] == want["features"]
    assert all(batches[k] is loaders[k[0]][k[1]] for k in batches)
    assert len(want["features"]) == (5 if case == "budget" else 9)            # the fixture is what the issue describes
    assert all(bi < 3 for v in want["meg"].values() for _, bi in v)


def test_fit_keeps_the_reference_asserts():
    from brainmagick_amd.norm import select_fit_batches
    g = Golden("scaler_fit")
    loaders = fixture_loaders(g)
    mixed = loaders[0][1]
    loaders[0][1] = mixed.replace(recording_index=torch.tensor([2, 2, 0, 2]))
    with pytest.raises(AssertionError):
        select_fit_batches(loaders, 10)                    # two recordings in one loader
    loaders = fixture_loaders(g)
    with pytest.raises(AssertionError, match="fitted twice"):
        select_fit_batches(loaders + [loaders[1]], 10)     # a recording that already has its scaler


def test_state_dict_round_trip():
    from brainmagick_amd.norm import DeviceBatchScaler
    gen = torch.Generator().manual_seed(3)
    a = DeviceBatchScaler(torch.randn(3, 6, generator=gen), torch.rand(3, 6, generator=gen) + 0.5,
                          torch.randn(6, generator=gen), torch.rand(6, generator=gen) + 0.5, device="cpu")
    a.feature_slices = {"emb": (0, 4), "cat": (4, 5), "aux": (5, 6)}
    a.feature_kinds = {"emb": "standard", "cat": "category", "aux": "noop"}
    a.categories_count = {"cat": torch.tensor([4., 0., 7., 1., 2.])}
    sd = a.state_dict()
    assert all(not v.is_cuda for v in sd.values() if isinstance(v, torch.Tensor))
    assert sd["feature_names"] == ["emb", "cat", "aux"]
    b = DeviceBatchScaler(torch.zeros(1, 1), torch.ones(1, 1), device="cpu").load_state_dict(sd)
    for name in ("meg_center", "meg_scale", "feature_center", "feature_scale"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.feature_slices == a.feature_slices and list(b.feature_slices) == ["emb", "cat", "aux"]
    assert b.feature_kinds == a.feature_kinds
    assert torch.equal(b.categories_count["cat"], a.categories_count["cat"])
    assert torch.equal(b.get_categorical_feature_weights("cat"), a.get_categorical_feature_weights("cat"))
    sd["meg_center"].zero_()                               # the state is a copy
    assert not torch.equal(a.meg_center, sd["meg_center"])
    # MEG only (no feature tables) survives too
    c = DeviceBatchScaler(torch.zeros(2, 3), torch.ones(2, 3), device="cpu")
    e = DeviceBatchScaler(torch.zeros(1, 1), torch.ones(1, 1), torch.zeros(1), torch.ones(1), device="cpu")
    e.load_state_dict(c.state_dict())
    assert e.feature_center is None and e.meg_scale.shape == (2, 3) and e.feature_slices == {}


def test_fit_and_inverse_transform_refuse_cpu_batches():
    from brainmagick_amd.norm import DeviceBatchScaler
    g = Golden("scaler_fit")
    with pytest.raises(RuntimeError):
        DeviceBatchScaler.fit(fixture_loaders(g), n_samples_per_recording=10)
    scaler = DeviceBatchScaler(torch.zeros(3, 6), torch.ones(3, 6), device="cpu")
    with pytest.raises(RuntimeError):
        scaler.inverse_transform(fixture_loaders(g)[0][0])
    with pytest.raises(RuntimeError):
        scaler.transform(fixture_loaders(g)[0][0])


def test_category_cardinality_cap_is_named():
    from brainmagick_amd import hip_ops as H
    with pytest.raises(ValueError, match="16384"):
        H.category_counts(torch.zeros(1, 1, 4), None, 0, H.MAX_CATEGORY_CARDINALITY + 1)


def test_scaler_fit_kernels_are_free_of_spills_and_scratch(tmp_path):
    """Every kernel of scaler_fit.hip, compiled for gfx950: no spilled register and no private segment (the histogram
    and prefix arrays must stay in LDS / registers)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "scaler_fit.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    "-o", str(out), str(csrc / "scaler_fit.hip")], check=True, capture_output=True)
    text = out.read_text()
    names = [l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "_kernel" in l]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(set(names)) == 11 and len(spills) == 11 and len(scratch) == 11, names
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (names, spills, scratch)
