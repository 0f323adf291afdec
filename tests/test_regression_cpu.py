"""CPU checks of the regression objective: the loss factory, the Solver's construction guards, no CPU fallback, the
multi-rank merge of the test metrics, and the reproducibility of tests/golden/regression.npz from the reference."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_create_loss_mirrors_the_reference_factory():
    from brainmagick_amd.losses import ClipLoss, L1Loss, L2Loss, create_loss
    assert type(create_loss("l1")) is L1Loss
    assert type(create_loss("mse")) is L2Loss
    clip = create_loss("clip", save_best=True, sync_grad=False, center=True)
    assert isinstance(clip, ClipLoss) and clip.center
    with pytest.raises(NotImplementedError, match="FeatureDecodingLoss"):
        create_loss("regression_classification")
    with pytest.raises(ValueError, match="Unsupported loss"):
        create_loss("huber")


@pytest.mark.parametrize("kw", [dict(n_negatives=4), dict(negatives="node")])
def test_solver_refuses_what_regression_cannot_use(kw):
    from brainmagick_amd.losses import L1Loss, L2Loss
    from brainmagick_amd.solver import Solver
    for loss in (L1Loss(), L2Loss()):
        with pytest.raises(ValueError):
            Solver(torch.nn.Conv1d(4, 4, 1), loss=loss, **kw)


def test_regression_has_no_cpu_fallback():
    from brainmagick_amd.losses import L1Loss, L2Loss
    from brainmagick_amd import metrics as M
    est, out = torch.randn(2, 3, 8), torch.randn(2, 3, 8)
    with pytest.raises(RuntimeError):
        L1Loss()(est, out, torch.ones(2, 1, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        L2Loss()(est, out)
    with pytest.raises(RuntimeError):
        M.OnlineCorrelation(slice(None), slice(None)).update(est, out, torch.ones(2, 1, 8, dtype=torch.bool))


def test_metric_constructors_follow_the_reference():
    from brainmagick_amd import metrics as M
    l2, corr = [c() for c in M.regression_metric_constructors("mel", slice(0, 3), slice(3, 6))]
    assert isinstance(l2, M.L2Reg) and l2.name == "l2_mel" and l2.left_slice == slice(0, 3)
    assert isinstance(corr, M.OnlineCorrelation) and corr.name == "corr_mel" and corr.left_slice == slice(3, 6)
    assert M.L2Reg(slice(None), slice(None)).get().tolist() == [0.0]           # nothing accumulated
    assert M.L2Reg.reduce([torch.tensor([4.0]), torch.tensor([12.0])]) == pytest.approx(np.sqrt(8.0))
    assert M.OnlineCorrelation.reduce([torch.tensor([0.5]), torch.tensor([0.25])]) == pytest.approx(0.375)


def test_multi_rank_merge_puts_every_recording_back_in_place():
    from brainmagick_amd.metrics import merge_rank_results
    n, world = 7, 3
    per_rank = [{"corr": [torch.full((2,), float(i)) for i in range(n)[r::world]],
                 "l2": [torch.tensor([10.0 + i]) for i in range(n)[r::world]]} for r in range(world)]
    merged = merge_rank_results(per_rank, n)
    assert [float(t[0]) for t in merged["corr"]] == list(range(n))
    assert [float(t) for t in merged["l2"]] == [10.0 + i for i in range(n)]
    assert merge_rank_results([{"l2": [torch.tensor([1.0])]}], 1)["l2"][0].item() == 1.0
    with pytest.raises(ValueError):
        merge_rank_results([{"l2": []}, {"l2": []}], 3)


def test_exchange_over_ranks_with_an_idle_rank_and_a_zero_count_result():
    """World 3, two recordings (rank 2 evaluates none), and rank 1's L2 result is the [1]-shaped zero of a metric that
    never saw a sample: every rank ends up with every result, in recording order (loopback communicator, in process)."""
    from loopback import run_replicas
    from brainmagick_amd.metrics import _exchange
    mine = {0: {"l2": [torch.arange(6.).view(2, 3)], "corr": [torch.full((2, 3), 0.5)]},
            1: {"l2": [torch.tensor([0.])], "corr": [torch.full((2, 3), -0.25)]},
            2: {"l2": [], "corr": []}}
    res = run_replicas(3, lambda r: _exchange(mine[r], 2))
    for merged in res:
        assert torch.equal(merged["l2"][0], torch.arange(6.).view(2, 3))
        assert torch.equal(merged["l2"][1], torch.tensor([0.]))
        assert torch.equal(merged["corr"][0], torch.full((2, 3), 0.5))
        assert torch.equal(merged["corr"][1], torch.full((2, 3), -0.25))


def test_regression_golden_is_reproduced_by_its_generator(tmp_path):
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    from _ref_import import REF
    if not REF.exists():
        pytest.skip("the reference sources are not available here")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "make_regression_golden.py"), str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(tmp_path / "regression.npz")
    old = np.load(ROOT / "tests" / "golden" / "regression.npz")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k == "meta":
            continue
        assert np.array_equal(new[k], old[k]), k
