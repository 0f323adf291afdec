"""The control flow of ``brainmagick_amd.train_loop`` without a GPU: every run the reference's own ``train`` /
``_run_one_epoch`` recorded against stubs (tests/golden/train_loop.json, made by tests/golden/make_train_loop_golden.py
from bm/solver.py:189-228, 325-401) is repeated through ``train_loop.fit`` with a stub solver whose steps return the same
canned losses as CPU tensors -- losses are multiples of 1/8, so every comparison is equality -- and the loop's own
promises: the look-ahead, the one read-back of the loss record, ``num_prints``, the checkpoint's write protocol,
``restore`` and the weighting of ``average_metrics``."""
import json
import logging
import os
from pathlib import Path

import pytest
import torch

from helpers import GOLDEN

FIXTURE = json.loads((GOLDEN / "train_loop.json").read_text())
CASES = FIXTURE["cases"]


def epoch_losses(per_epoch, epoch):
    return per_epoch[min(epoch, len(per_epoch)) - 1]


class Tagged(torch.nn.Module):
    """A model whose whole state is the epoch that trained it last."""

    def __init__(self):
        super().__init__()
        self.register_buffer("tag", torch.zeros(()))


class Loader:
    def __init__(self, solver, phase, per_epoch):
        self.solver, self.phase, self.per_epoch, self.epochs_set = solver, phase, per_epoch, []

    def set_epoch(self, epoch):
        self.epochs_set.append([self.phase, epoch])

    def __len__(self):
        return len(epoch_losses(self.per_epoch, self.solver.epoch))

    def __iter__(self):
        epoch = self.solver.epoch
        for i in range(len(self)):
            yield (self.phase, epoch, i)


class StubSolver:
    """What ``train_loop`` touches on a Solver.  ``train_step`` keeps the real one's rule for a fully rejected batch
    (it re-runs ``_last_batch`` or raises); ``_eval_loss`` answers None for one."""

    def __init__(self, losses, resume=None):
        self.losses = losses                                   # {"train": per epoch, "valid": per epoch}
        self.device = torch.device("cpu")
        self.model, self.feature_model, self.loss = Tagged(), None, torch.nn.Linear(1, 1)
        self.scale_reject = None
        self.history, self.best_loss, self.best_epoch, self.best_state, self.last_test_epoch = [], float("inf"), 0, None, 0
        self.best_on = "device"
        self._last_batch = self._prefetched = self._gather = None
        self._staged = {}
        self.processed, self.events, self.modes, self.steps, self.state_dict_calls = [], [], [], [], 0
        if resume:
            self.history = [dict(h) for h in resume["history"]]
            self.best_epoch, self.best_loss = resume["best_epoch"], resume["best_loss"]
            self.last_test_epoch = resume["last_test_epoch"]
            self.best_state = {"model": {"tag": torch.tensor(float(resume["best_epoch"]))}}
            self.model.tag.fill_(len(self.history))

    @property
    def epoch(self):
        return len(self.history) + 1

    def _value(self, batch, training):
        phase, epoch, i = batch
        self.processed.append([phase, epoch, i])
        self.events.append((epoch, phase))
        self.modes.append((epoch, phase, self.model.training, self.loss.training))
        return epoch_losses(self.losses[phase], epoch)[i]

    def train_step(self, batch, next_batch=None):
        self.steps.append((batch, next_batch))
        self.model.train(True), self.loss.train(True)
        value = self._value(batch, True)
        if value is None:
            if self._last_batch is None:
                raise RuntimeError("Empty batch and last batch is none")
            value = self._value(self._last_batch, True)
        else:
            self._last_batch = batch
        self.model.tag.fill_(self.epoch)
        return torch.tensor(value, dtype=torch.float32)

    def _eval_loss(self, batch):
        assert not torch.is_grad_enabled()
        self.model.train(False), self.loss.train(False)
        value = self._value(batch, False)
        return None if value is None else torch.tensor(value, dtype=torch.float32)

    def state_dict(self):
        self.state_dict_calls += 1
        return {"model": self.model.state_dict(), "optimizer": {"step": 3}}

    def load_state_dict(self, state):
        self.model.load_state_dict(state["model"])
        self.loaded_optimizer = state["optimizer"]


def collapse(events):
    out = []
    for e in events:
        if not out or out[-1] != e:
            out.append(e)
    return [list(e) for e in out]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_repeats_the_reference_run(monkeypatch, name):
    from brainmagick_amd import distrib, train_loop
    spec, want = CASES[name]["settings"], CASES[name]["result"]
    solver = StubSolver({"train": spec["train"], "valid": spec["valid"]}, spec["resume"])
    loaders = {p: Loader(solver, p, spec[p]) for p in ("train", "valid")}
    averaged, test_saw = [], []
    monkeypatch.setattr(distrib, "is_distributed", lambda: spec["distributed"])
    monkeypatch.setattr(distrib, "average_metrics",
                        lambda metrics, count=1.: averaged.append([dict(metrics), count]) or dict(metrics))

    def test():
        assert not torch.is_grad_enabled()
        test_saw.append([solver.epoch, int(solver.model.tag)])
        solver.events.append((solver.epoch, "test"))
        return {"wer": 0.5}
    raised = None
    try:
        history = train_loop.fit(solver, loaders["train"], loaders["valid"], epochs=spec["epochs"], test=test,
                                 eval_every=spec["eval_every"], early_stop_patience=spec["early_stop_patience"],
                                 max_batches=spec["max_batches"])
        assert history is solver.history
    except RuntimeError as exc:
        raised = f"{type(exc).__name__}: {exc}"
    assert raised == want["raised"]
    assert collapse(solver.events) == want["stages"]
    assert solver.history == want["history"]
    assert solver.best_epoch == want["best_epoch"] and solver.best_loss == float(want["best_loss"])
    assert solver.last_test_epoch == want["last_test_epoch"]
    assert test_saw == want["test_saw"]                                # the state swapped in for the test stage
    assert int(solver.model.tag) == want["live_state_epoch"]           # and the live one is back
    if want["best_state_epoch"] is None:
        assert solver.best_state is None
    else:
        assert int(solver.best_state["model"]["tag"]) == want["best_state_epoch"]
        assert solver.best_state["model"]["tag"] is not solver.model.tag
    assert solver.processed == want["processed"]
    assert averaged == want["averaged"]
    assert loaders["train"].epochs_set == want["set_epoch"] and loaders["valid"].epochs_set == []
    # the reference sets the mode once per stage; here every step of the stage ran in it
    stage_modes = {}
    for module, mode in want["modes"]:
        stage_modes.setdefault(module, []).append(mode)
    assert stage_modes.get("all_models", []) == stage_modes.get("loss", [])
    stages = [s for s in want["stages"] if s[1] != "test"]
    assert len(stages) == len(stage_modes.get("all_models", []))
    for (epoch, phase), mode in zip(stages, stage_modes.get("all_models", [])):
        seen = {(m, l) for e, p, m, l in solver.modes if (e, p) == (epoch, phase)}
        assert seen <= {(mode, mode)} and mode == (phase == "train")
    assert solver._prefetched is None


def test_the_fixture_holds_the_cases_the_loop_is_made_of():
    """A fixture that lost a case fails here, not vacuously."""
    r = {k: v["result"] for k, v in CASES.items()}
    assert len(r["patience_hit"]["history"]) == 5 and r["patience_hit"]["test_saw"] == [[2, 2]]
    assert len(r["patience_not_hit"]["history"]) == 7
    assert r["ties_are_no_improvement"]["best_epoch"] == 1 and len(r["ties_are_no_improvement"]["history"]) == 3
    assert r["eval_every_3_final_newer"]["test_saw"] == [[3, 2], [5, 4]]
    assert r["eval_every_3_final_not_newer"]["test_saw"] == [[3, 3]]
    assert r["rejected_middle"]["history"][0]["train"]["loss"] == 2.25
    assert r["rejected_first_valid"]["raised"] == r["rejected_first_train_epoch_2"]["raised"] == \
        "RuntimeError: Empty batch and last batch is none"
    assert r["distributed"]["set_epoch"] == [["train", 0], ["train", 1], ["train", 2]]
    assert r["distributed_max_batches"]["averaged"][0][1] == 3
    assert [s[0] for s in r["resumed_at_epoch_3"]["stages"]][0] == 3 and r["resumed_past_the_end"]["stages"] == []
    for v in CASES.values():
        for per_epoch in (v["settings"]["train"], v["settings"]["valid"]):
            assert all(x is None or x * 8 == int(x * 8) for losses in per_epoch for x in losses)


@pytest.mark.parametrize("max_batches,n_steps", [(None, 5), (0, 5), (2, 2), (5, 5), (9, 5)])
def test_look_ahead(max_batches, n_steps):
    """``next_batch`` of step i is batch i + 1; None at the end of the loader, and at ``max_batches``."""
    from brainmagick_amd import train_loop
    solver = StubSolver({"train": [[1.0, 2.0, 3.0, 4.0, 0.5]], "valid": [[1.0]]})
    solver._last_batch = ("train", 0, 9)                         # an earlier epoch's: not this epoch's last good batch
    solver._prefetched = None
    got = train_loop.run_epoch(solver, Loader(solver, "train", solver.losses["train"]), True, max_batches=max_batches)
    batches = [("train", 1, i) for i in range(5)]
    assert [b for b, _ in solver.steps] == batches[:n_steps]
    assert [n for _, n in solver.steps] == batches[1:n_steps] + [None]
    assert got == {"loss": sum([1.0, 2.0, 3.0, 4.0, 0.5][:n_steps]) / n_steps}
    assert solver._prefetched is None and solver.history == [] and solver.best_state is None


def test_an_exception_of_a_step_leaves_no_prefetch_and_no_bookkeeping():
    from brainmagick_amd import train_loop

    class Gather:
        cancelled = 0

        def cancel(self):
            self.cancelled += 1
    solver = StubSolver({"train": [[1.0, 2.0, 3.0, 4.0]], "valid": [[1.0]]})
    solver._gather = Gather()
    real = solver.train_step

    def train_step(batch, next_batch=None):
        if batch[2] == 2:
            solver._prefetched = (next_batch, None, next_batch)          # what train_step had prepared when it asserted
            solver._staged[id(next_batch)] = (next_batch, next_batch)
            raise AssertionError("non-finite values in the MEG or feature tensors")
        return real(batch, next_batch)
    solver.train_step = train_step
    with pytest.raises(AssertionError, match="non-finite"):
        train_loop.fit(solver, Loader(solver, "train", solver.losses["train"]), Loader(solver, "valid", [[1.0]]), epochs=2)
    assert solver._prefetched is None and solver._gather.cancelled == 1 and not solver._staged
    assert solver.history == [] and solver.best_state is None and solver.best_epoch == 0
    assert solver.best_loss == float("inf") and solver.epoch == 1


def test_the_record_is_read_once_after_the_last_step(monkeypatch):
    """No ``.item()`` / ``float()`` / ``.cpu()`` / ``.tolist()`` of a tensor outside ``read_losses``, which runs once per
    epoch, after the last step."""
    from brainmagick_amd import train_loop
    solver = StubSolver({"train": [[1.0, 2.0, None, 4.0]], "valid": [[3.0, None, 1.0, 1.0]]})
    reads, outside, inside = [], [], []
    real_read = train_loop.read_losses

    def read_losses(record, count):
        reads.append((len(solver.processed), count))
        inside.append(True)
        try:
            return real_read(record, count)
        finally:
            inside.pop()
    monkeypatch.setattr(train_loop, "read_losses", read_losses)
    for name in ("item", "cpu", "tolist", "__float__"):
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **k):
            if not inside:
                outside.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    train = train_loop.run_epoch(solver, Loader(solver, "train", solver.losses["train"]), True)
    valid = train_loop.run_epoch(solver, Loader(solver, "valid", solver.losses["valid"]), False)
    monkeypatch.undo()
    assert train == {"loss": 2.25} and valid == {"loss": 2.0}
    assert reads == [(5, 4), (10, 4)]                             # 4 steps + 1 re-run each: behind the last one
    assert outside == []


def test_num_prints_reads_at_evenly_spaced_steps(monkeypatch, caplog):
    from brainmagick_amd import train_loop
    losses = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    solver = StubSolver({"train": [losses], "valid": [losses]})
    reads = []
    real_read = train_loop.read_losses
    monkeypatch.setattr(train_loop, "read_losses", lambda record, count: reads.append(count) or real_read(record, count))
    with caplog.at_level(logging.INFO, logger="brainmagick_amd.train_loop"):
        got = train_loop.run_epoch(solver, Loader(solver, "train", [losses]), True, num_prints=3)
    assert got == {"loss": 4.5} and reads == [2, 4, 6, 8]
    lines = [r.getMessage() for r in caplog.records if "loss" in r.getMessage()]
    assert lines == ["train | 2/8 | loss 1.5000", "train | 4/8 | loss 2.5000", "train | 6/8 | loss 3.5000"]
    reads.clear()
    train_loop.run_epoch(solver, Loader(solver, "valid", [losses]), False, num_prints=2, max_batches=4)
    assert reads == [2, 4]                                        # 2 of 4 (the second print would be the last step: the result)
    reads.clear()
    train_loop.run_epoch(solver, Loader(solver, "valid", [losses]), False)
    assert reads == [8]


def test_best_state_is_a_clone_on_the_chosen_device():
    from brainmagick_amd import train_loop
    solver = StubSolver({"train": [[1.0]], "valid": [[2.0], [1.0], [1.0]]})
    solver.model.tag.fill_(7)
    train_loop.run_epoch(solver, Loader(solver, "valid", solver.losses["valid"]), False)
    best = solver.best_state["model"]["tag"]
    solver.model.tag.fill_(9)
    assert float(best) == 7 and solver.best_loss == 2.0 and solver.best_epoch == 1
    solver.best_on = "cpu"
    solver.history.append({})
    train_loop.run_epoch(solver, Loader(solver, "valid", solver.losses["valid"]), False)
    assert float(solver.best_state["model"]["tag"]) == 9 and solver.best_state["model"]["tag"].device.type == "cpu"
    assert solver.best_epoch == 2 and solver.best_state["model"]["tag"] is not solver.model.tag
    solver.history.append({})
    solver.model.tag.fill_(11)
    train_loop.run_epoch(solver, Loader(solver, "valid", solver.losses["valid"]), False)      # a tie: not below
    assert float(solver.best_state["model"]["tag"]) == 9 and solver.best_epoch == 2
    solver.best_on = "host"
    solver.best_loss = 5.0
    with pytest.raises(ValueError, match="best_on"):
        train_loop.run_epoch(solver, Loader(solver, "valid", solver.losses["valid"]), False)


def test_swap_state_announces_both_loads(monkeypatch):
    from brainmagick_amd import hip_ops, train_loop
    solver = StubSolver({"train": [[1.0]], "valid": [[1.0]]})
    solver.model.tag.fill_(4)
    calls = []
    monkeypatch.setattr(hip_ops, "weights_changed", lambda: calls.append(float(solver.model.tag)))
    with pytest.raises(KeyError):
        with train_loop.swap_state(solver, {"model": {"tag": torch.tensor(2.0)}}):
            assert float(solver.model.tag) == 2 and calls == [2.0]
            raise KeyError("the test stage failed")
    assert float(solver.model.tag) == 4 and calls == [2.0, 4.0]         # put back on the way out of an exception too
    solver.best_state = {"model": {"tag": torch.tensor(3.0)}}
    train_loop.load_best(solver)
    assert float(solver.model.tag) == 3 and calls == [2.0, 4.0, 3.0]


class Scaler:
    def __init__(self, value):
        self.value = value

    def state_dict(self):
        return {"meg_center": torch.tensor([self.value])}

    def load_state_dict(self, state):
        self.value = float(state["meg_center"][0])


@pytest.mark.parametrize("rank", [0, 1])
def test_checkpoint_write_protocol(monkeypatch, tmp_path, rank):
    """Every rank calls ``state_dict()``; rank 0 writes a temporary file in the same directory and renames it; every
    rank meets at the barrier afterwards."""
    import types
    from brainmagick_amd import distrib, train_loop
    solver = StubSolver({"train": [[1.0, 2.0]], "valid": [[2.0, 1.0], [1.0, 1.0]]})
    solver.scale_reject = types.SimpleNamespace(scaler=Scaler(2.5), rejection_rate=0.25)
    path = tmp_path / "checkpoint.th"
    log = []
    real_replace, real_state_dict = os.replace, solver.state_dict
    monkeypatch.setattr(distrib, "rank", lambda: rank)
    monkeypatch.setattr(distrib, "world_size", lambda: 2)
    monkeypatch.setattr(distrib, "barrier", lambda: log.append(("barrier", path.exists())))
    monkeypatch.setattr(train_loop.os, "replace", lambda src, dst: log.append(("replace", Path(src), Path(dst),
                                                                                Path(src).exists(), Path(dst).exists()))
                        or real_replace(src, dst))
    solver.state_dict = lambda: log.append(("state_dict",)) or real_state_dict()
    train_loop.fit(solver, Loader(solver, "train", solver.losses["train"]), Loader(solver, "valid", solver.losses["valid"]),
                   epochs=2, checkpoint=path)
    if rank == 0:
        first = log[:3]
        assert [e[0] for e in log] == ["state_dict", "replace", "barrier"] * 2
        _, src, dst, src_exists, dst_existed = first[1]
        assert dst == path and src != path and src.parent == path.parent and src_exists and not dst_existed
        assert first[2] == ("barrier", True)
        assert sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint.th"]           # no temporary file left
        state = torch.load(path, map_location="cpu")
        assert set(state) == {"solver", "best_state", "best_loss", "best_epoch", "last_test_epoch", "history", "loss",
                              "scaler"}
        assert state["history"] == solver.history and len(state["history"]) == 2
        assert state["best_epoch"] == 2 and state["best_loss"] == 1.0 and state["last_test_epoch"] == 0
        assert float(state["best_state"]["model"]["tag"]) == 2 and state["solver"]["optimizer"] == {"step": 3}
        assert set(state["loss"]) == {"weight", "bias"} and float(state["scaler"]["meg_center"][0]) == 2.5
    else:
        assert [e[0] for e in log] == ["state_dict", "barrier"] * 2 and not path.exists()
        assert list(tmp_path.iterdir()) == []


def test_restore_in_its_three_outcomes(monkeypatch, tmp_path):
    import types
    from brainmagick_amd import hip_ops, train_loop
    losses = {"train": [[1.0, 2.0]], "valid": [[1.0], [2.0]]}
    first = StubSolver(losses)
    first.scale_reject = types.SimpleNamespace(scaler=Scaler(2.5), rejection_rate=0.)
    with torch.no_grad():
        first.loss.weight.fill_(0.375)
    path = tmp_path / "run" / "checkpoint.th"
    path.parent.mkdir()
    train_loop.fit(first, Loader(first, "train", losses["train"]), Loader(first, "valid", losses["valid"]), epochs=2,
                   checkpoint=path)
    assert first.best_epoch == 1 and float(first.model.tag) == 2
    changed = []
    monkeypatch.setattr(hip_ops, "weights_changed", lambda: changed.append(1))

    # 1. the checkpoint exists: everything comes back (continue_from is not looked at)
    second = StubSolver(losses)
    second.scale_reject = types.SimpleNamespace(scaler=Scaler(0.), rejection_rate=0.)
    assert train_loop.restore(second, path, continue_from=tmp_path / "nowhere.th") is True
    assert float(second.model.tag) == 2 and second.loaded_optimizer == {"step": 3} and changed
    assert second.history == first.history and second.epoch == 3
    assert (second.best_epoch, second.best_loss, second.last_test_epoch) == (1, 1.0, 0)
    assert float(second.best_state["model"]["tag"]) == 1
    assert float(second.loss.weight.detach()) == 0.375 and second.scale_reject.scaler.value == 2.5
    # ... and a fit to the same horizon has nothing left to do; one more epoch continues at epoch 3
    assert train_loop.fit(second, Loader(second, "train", losses["train"]), Loader(second, "valid", losses["valid"]),
                          epochs=2) == first.history
    assert second.processed == []
    train_loop.fit(second, Loader(second, "train", losses["train"]), Loader(second, "valid", losses["valid"]), epochs=3)
    assert [e for e, _ in collapse(second.events)] == [3, 3] and len(second.history) == 3

    # 2. no checkpoint, continue_from: the models only, from best_state or from the model state; no history
    for best, tag in ((True, 1), (False, 2)):
        third = StubSolver(losses)
        del changed[:]
        assert train_loop.restore(third, tmp_path / "other" / "checkpoint.th", continue_from=path,
                                  continue_best=best) is False
        assert float(third.model.tag) == tag and changed == [1]
        assert third.history == [] and third.best_state is None and third.best_epoch == 0 and third.epoch == 1
        assert not hasattr(third, "loaded_optimizer")
    with pytest.raises(AssertionError, match="Could not find checkpoint"):
        train_loop.restore(StubSolver(losses), tmp_path / "other.th", continue_from=tmp_path / "nowhere.th")

    # 3. neither: nothing happens
    fourth = StubSolver(losses)
    del changed[:]
    assert train_loop.restore(fourth, tmp_path / "other.th") is False
    assert float(fourth.model.tag) == 0 and fourth.history == [] and changed == []


def test_average_metrics_is_weighted_by_the_step_count(monkeypatch):
    """Two ranks: this one took 2 steps (mean 1.5), the other 4 (mean 3.0): (3 + 12) / 6."""
    from brainmagick_amd import distrib, train_loop

    class Comm:
        world, rank, kind = 2, 0, "test"

        def scalar_device(self):
            return "cpu"

        def all_reduce(self, t, op="sum"):
            assert t.tolist() == [3.0, 2.0]                       # [loss * steps, steps]
            t += torch.tensor([12.0, 4.0])
    monkeypatch.setattr(distrib, "_comm", Comm())
    solver = StubSolver({"train": [[1.0, 2.0, 8.0, 8.0]], "valid": [[1.0]]})
    loader = Loader(solver, "train", solver.losses["train"])
    assert train_loop.run_epoch(solver, loader, True, max_batches=2) == {"loss": 2.5}
    assert loader.epochs_set == [["train", 0]]


def test_solver_methods_are_dispatch(monkeypatch):
    """``Solver.run_epoch`` / ``fit`` / ``restore`` / ``load_best`` hand their arguments to ``train_loop``."""
    from brainmagick_amd import train_loop
    from brainmagick_amd.solver import Solver
    calls = []
    for name in ("run_epoch", "fit", "restore", "load_best"):
        monkeypatch.setattr(train_loop, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or _n)
    solver = object.__new__(Solver)
    assert Solver.run_epoch(solver, "L", True, max_batches=3) == "run_epoch"
    assert Solver.fit(solver, "A", "B", epochs=4, eval_every=2) == "fit"
    assert Solver.restore(solver, "C", continue_from="D", continue_best=False) == "restore"
    Solver.load_best(solver)
    assert calls[0] == ("run_epoch", (solver, "L", True), dict(max_batches=3, num_prints=0))
    assert calls[1] == ("fit", (solver, "A", "B"), dict(epochs=4, test=None, eval_every=2, early_stop_patience=None,
                                                        max_batches=None, checkpoint=None, num_prints=0))
    assert calls[2] == ("restore", (solver, "C"), dict(continue_from="D", continue_best=False))
    assert calls[3] == ("load_best", (solver,), {})
    solver.history = [{}, {}]
    assert solver.epoch == 3


def test_signatures_match():
    import inspect
    from brainmagick_amd import train_loop
    from brainmagick_amd.solver import Solver
    for name in ("run_epoch", "fit", "restore", "load_best"):
        ours = inspect.signature(getattr(Solver, name)).parameters
        theirs = inspect.signature(getattr(train_loop, name)).parameters
        assert list(ours)[1:] == list(theirs)[1:], name
        for key in list(ours)[1:]:
            assert ours[key].default == theirs[key].default and ours[key].kind == theirs[key].kind, (name, key)
