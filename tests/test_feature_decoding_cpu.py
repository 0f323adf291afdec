"""CPU checks of FeatureDecodingLoss / ClassificationAcc: the loss factory, the shape rules, no CPU fallback, the Solver's
construction guards, the decode branch of the metric constructors, the kernels' register audit, and the reproducibility
of tests/golden/feature_decoding.npz from the reference."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "golden"))

from make_feature_decoding_golden import CASES, Builder, Weights  # noqa: E402


def test_create_loss_builds_the_loss_from_the_features_builder():
    from brainmagick_amd.losses import FeatureDecodingLoss, create_loss
    builder = Builder(CASES["mixed"])
    loss = create_loss("regression_classification", used_features=builder, scaler=None)
    assert type(loss) is FeatureDecodingLoss and loss.used_features is builder and loss.scaler is None
    scaler = Weights({})
    assert create_loss("regression_classification", used_features=builder, scaler=scaler).scaler is scaler
    with pytest.raises(NotImplementedError, match="FeatureDecodingLoss"):
        create_loss("regression_classification")


def test_plan_follows_the_slices_and_fetches_the_weights_once():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import FeatureDecodingLoss
    builder = Builder(CASES["mixed"])
    calls = []

    class Scaler:
        def get_categorical_feature_weights(self, name):
            calls.append(name)
            return torch.full((builder[name].cardinality,), 0.5)

    loss = FeatureDecodingLoss(builder, Scaler())
    table, weights = loss._plan()
    assert table == ((H.FEATURE_CONTINUOUS, 0, 3, 0, -1), (H.FEATURE_CATEGORICAL, 3, 64, 3, 0),
                     (H.FEATURE_CONTINUOUS, 67, 2, 4, -1), (H.FEATURE_CATEGORICAL, 69, 3, 6, 64))
    assert weights.shape == (67,) and loss._plan()[0] is table and calls == ["ph", "seg"]
    assert FeatureDecodingLoss(builder, None)._plan()[1] is None

    class Wide(Builder):                      # a categorical feature that takes two target channels
        def get_slice(self, name, model_output=False):
            sl = super().get_slice(name, model_output)
            return sl if model_output else slice(sl.start, sl.start + 2)

    with pytest.raises(AssertionError, match="Supporting only single categorical cross entropy for now."):
        FeatureDecodingLoss(Wide(CASES["cat_only"]), None)._plan()


def test_dimension_assert_and_mask_shape():
    from brainmagick_amd.losses import FeatureDecodingLoss
    builder = Builder(CASES["mixed"])
    loss = FeatureDecodingLoss(builder, None)
    est, out = torch.randn(2, builder.output_dimension, 8), torch.zeros(2, builder.dimension, 8)
    with pytest.raises(AssertionError, match="Invalid features dim received"):
        loss(est[:, :-1], out)
    with pytest.raises(AssertionError, match="Invalid features dim received"):
        loss(est, est)
    for shape in ((2, builder.output_dimension, 8), (2, 8), (1, 1, 8), (2, 1, 7)):
        with pytest.raises(ValueError, match=r"\[B, 1, T\]"):
            loss(est, out, torch.ones(shape, dtype=torch.bool))
    with pytest.raises(TypeError):
        loss(est, out, torch.ones(2, 1, 8))
    with pytest.raises(NotImplementedError):
        loss(est, out.clone().requires_grad_(True))


def test_no_cpu_fallback():
    from brainmagick_amd import metrics as M
    from brainmagick_amd.losses import FeatureDecodingLoss
    builder = Builder(CASES["cat_first"])
    est, out = torch.randn(2, builder.output_dimension, 8), torch.zeros(2, builder.dimension, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FeatureDecodingLoss(builder, None)(est, out, torch.ones(2, 1, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FeatureDecodingLoss(builder, None)(est, out)
    acc = M.ClassificationAcc(slice(0, 2), slice(0, 1), name="acc_seg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.update(est, out, torch.ones(2, 1, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.update_all([acc, M.L2Reg(slice(2, 6), slice(1, 5))], est, out, None)


@pytest.mark.parametrize("kw", [dict(n_negatives=4), dict(negatives="node"),
                                dict(feature_model=torch.nn.Conv1d(4, 4, 1))])
def test_solver_refuses_what_the_loss_cannot_use(kw):
    from brainmagick_amd.losses import FeatureDecodingLoss
    from brainmagick_amd.solver import Solver
    with pytest.raises(ValueError, match="FeatureDecodingLoss"):
        Solver(torch.nn.Conv1d(4, 4, 1), loss=FeatureDecodingLoss(Builder(CASES["mixed"]), None), **kw)


def test_metric_constructors_follow_the_reference():
    """bm/solver.py:410-432 for the `mixed` builder: classes, names, slices (the L2 metric takes the feature slice
    first) and order."""
    from brainmagick_amd import metrics as M
    got = [c() for c in M.metric_constructors(Builder(CASES["mixed"]))]
    want = [(M.L2Reg, "l2_emb", slice(0, 3), slice(0, 3)), (M.OnlineCorrelation, "corr_emb", slice(0, 3), slice(0, 3)),
            (M.ClassificationAcc, "acc_ph", slice(3, 67), slice(3, 4)),
            (M.L2Reg, "l2_aux", slice(4, 6), slice(67, 69)), (M.OnlineCorrelation, "corr_aux", slice(67, 69), slice(4, 6)),
            (M.ClassificationAcc, "acc_seg", slice(69, 72), slice(6, 7))]
    assert [(type(m), m.name, m.left_slice, m.right_slice) for m in got] == want
    # the regression-only entry point is unchanged
    l2, corr = [c() for c in M.regression_metric_constructors("mel")]
    assert (l2.name, corr.name) == ("l2_mel", "corr_mel")


def test_classification_acc_reduce_and_empty_get():
    from brainmagick_amd import metrics as M
    assert M.ClassificationAcc.reduce([torch.tensor([[0.5, 1.0]]), torch.tensor([[0.0, 0.5]])]) == pytest.approx(0.5)
    assert M.ClassificationAcc(slice(0, 3), slice(0, 1)).get().tolist() == [0.0]       # nothing counted
    with pytest.raises(NotImplementedError):
        M.ClassificationAcc(slice(0, 3), slice(0, 1), dim=1)


def test_new_kernels_are_free_of_spilled_vector_registers_and_scratch(tmp_path):
    """regress.hip compiled for gfx950: no kernel of it -- the feature-decoding forward with its per-feature loop and
    by-value feature table included -- spills a vector register or has a private segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    out = tmp_path / "regress.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                    "-o", str(out), str(csrc / "regress.hip")], check=True, capture_output=True)
    text = out.read_text()
    names = {l.split(":")[1].strip() for l in text.splitlines() if l.strip().startswith(".name:") and "_kernel" in l}
    assert {n for n in names if "feature_decoding" in n or "class_acc" in n} and len(names) == 8, names
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 8 and len(scratch) == 8
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)


def test_feature_decoding_golden_is_reproduced_by_its_generator(tmp_path):
    from _ref_import import REF
    if not REF.exists():
        pytest.skip("the reference sources are not available here")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "make_feature_decoding_golden.py"),
                        str(tmp_path)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(tmp_path / "feature_decoding.npz")
    old = np.load(ROOT / "tests" / "golden" / "feature_decoding.npz")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k == "meta":
            continue
        assert np.array_equal(new[k], old[k]), k
