"""Recorded runs of the reference's training loop, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_train_loop_golden.py [output directory]
Writes ``train_loop.json`` (default: next to this file).

The reference ``Solver`` cannot be imported (flashy, dora), so ``Solver.train`` (bm/solver.py:189-228) and
``Solver._run_one_epoch`` (bm/solver.py:325-401) are taken from ``bm/solver.py`` by AST and run, unmodified, against
stubs (make_encode_golden.py's method):

  * a ``flashy`` namespace: ``averager`` and ``distrib.{is_distributed, average_metrics, sync_model}``.  flashy is not
    installed: ``averager(beta=1)`` and ``BaseSolver.epoch`` / ``run_stage`` / ``commit`` (below, ``StubSolver``) are
    restated from its published source, which cannot be checked here;
  * a ``self`` with canned loaders, ``_process_batch`` (the "estimate" is the batch's canned loss, None for a batch whose
    segments were all rejected), ``loss`` (returns the estimate), ``optimizer``, ``all_models``, ``run_stage``,
    ``commit``, ``log_progress`` and ``_test_one_epoch``;
  * ``copy_state`` / ``swap_state`` that record.  The "state" of the models is ``{"epoch": the epoch that made it}``.

``CASES``: settings and canned losses (multiples of 1/8: every mean is exact).  ``train`` / ``valid``: per epoch, the
losses of the loader's batches; the last list serves every later epoch.  The fixture holds, per case, these settings
and what the run recorded: the stage calls in order, ``history``, ``best_epoch``, ``best_loss``, ``last_test_epoch``,
the state every test stage saw, the ``train(mode)`` calls, the batches ``_process_batch`` was handed (re-runs of the
last good batch included), the ``set_epoch`` and ``average_metrics`` arguments under the distributed stub, the totals
handed to ``log_progress``, and the exception that ended the run, if one did.
"""
import ast
import contextlib
import json
import logging
import sys
import types
from collections import defaultdict
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

R = None      # a batch whose segments are all rejected
FOUR = [[1.0, 2.0, 3.0, 4.0]]


def _valid_means(*means):
    """Two batches per epoch around each mean (mean -/+ 0.5)."""
    return [[m - 0.5, m + 0.5] for m in means]


_BASE = dict(epochs=3, early_stop_patience=None, eval_every=1, max_batches=None, train=FOUR,
             valid=_valid_means(3.0, 2.0, 1.0), distributed=False, resume=None)
CASES = {
    # the issue's trial (its 2.6 / 2.7 moved to multiples of 1/8): stops after epoch 5, best 2, tested at epoch 2 only
    "patience_hit": dict(_BASE, epochs=7, early_stop_patience=3, eval_every=2,
                         valid=_valid_means(3.0, 2.0, 2.5, 2.625, 2.75, 1.0, 9.0)),
    "patience_not_hit": dict(_BASE, epochs=7, early_stop_patience=4, eval_every=2,
                             valid=_valid_means(3.0, 2.0, 2.5, 2.625, 2.75, 1.0, 9.0)),
    "patience_zero_is_off": dict(_BASE, epochs=4, early_stop_patience=0, valid=_valid_means(1.0, 2.0, 3.0, 4.0)),
    "eval_every_1": dict(_BASE, epochs=5, eval_every=1, valid=_valid_means(3.0, 2.0, 1.0, 4.0, 5.0)),
    "eval_every_2_final_not_newer": dict(_BASE, epochs=5, eval_every=2, valid=_valid_means(3.0, 2.0, 1.0, 4.0, 5.0)),
    "eval_every_3_final_newer": dict(_BASE, epochs=5, eval_every=3, valid=_valid_means(3.0, 2.0, 2.5, 1.0, 5.0)),
    "eval_every_3_final_not_newer": dict(_BASE, epochs=5, eval_every=3, valid=_valid_means(3.0, 2.0, 1.0, 4.0, 5.0)),
    "never_improves_after_1": dict(_BASE, epochs=4, valid=_valid_means(1.0, 2.0, 3.0, 4.0)),
    "ties_are_no_improvement": dict(_BASE, epochs=5, early_stop_patience=2, valid=_valid_means(2.0, 2.0, 2.0, 2.0, 2.0)),
    "max_batches_below": dict(_BASE, epochs=2, max_batches=2, valid=[[1.0, 2.0, 3.0, 4.0], [0.5, 1.0, 8.0, 8.0]]),
    "max_batches_equal": dict(_BASE, epochs=2, max_batches=4, valid=[[1.0, 2.0, 3.0, 4.0], [0.5, 1.0, 8.0, 8.0]]),
    "max_batches_above": dict(_BASE, epochs=2, max_batches=6, valid=[[1.0, 2.0, 3.0, 4.0], [0.5, 1.0, 8.0, 8.0]]),
    "rejected_middle": dict(_BASE, epochs=2, train=[[1.0, 2.0, R, 4.0]], valid=[[3.0, R, 1.0, 1.0], [2.0, R, R, 0.5]]),
    "rejected_last": dict(_BASE, epochs=2, train=[[1.0, 2.0, 4.0, R]], valid=[[3.0, 1.0, 2.0, R]]),
    "rejected_at_max_batches": dict(_BASE, epochs=2, max_batches=4, train=[[1.0, 2.0, 3.0, R, 4.0]],
                                    valid=[[3.0, 1.0, 2.0, R, 8.0]]),
    "rejected_first_train": dict(_BASE, epochs=2, train=[[R, 2.0, 3.0, 4.0]]),
    "rejected_first_valid": dict(_BASE, epochs=2, valid=[[R, 2.0]]),
    # the last good batch is an epoch's own: epoch 1 ends on a good batch, epoch 2 starts on a rejected one
    "rejected_first_train_epoch_2": dict(_BASE, epochs=3, train=[[1.0, 2.0], [R, 2.0]]),
    "rejected_first_valid_epoch_2": dict(_BASE, epochs=3, valid=[[1.0, 2.0], [R, 2.0]]),
    "distributed": dict(_BASE, epochs=3, distributed=True, valid=_valid_means(3.0, 2.0, 2.5)),
    "distributed_max_batches": dict(_BASE, epochs=2, distributed=True, max_batches=3, valid=[[1.0, 2.0, 3.0, 4.0]]),
    "resumed_at_epoch_3": dict(_BASE, epochs=5, eval_every=2, early_stop_patience=3,
                               valid=_valid_means(9.0, 9.0, 2.5, 1.5, 3.0),
                               resume=dict(history=[{"train": {"loss": 2.5}, "valid": {"loss": 3.0}},
                                                    {"train": {"loss": 2.5}, "valid": {"loss": 2.0},
                                                     "test": {"wer": 0.5}}],
                                           best_epoch=2, best_loss=2.0, last_test_epoch=2)),
    "resumed_past_the_end": dict(_BASE, epochs=2,
                                 resume=dict(history=[{"train": {"loss": 2.5}, "valid": {"loss": 3.0}},
                                                      {"train": {"loss": 2.5}, "valid": {"loss": 2.0}}],
                                             best_epoch=2, best_loss=2.0, last_test_epoch=0)),
}


def epoch_losses(per_epoch, epoch: int):
    """The canned losses of ``epoch`` (1-based): the last list serves every later epoch."""
    return per_epoch[min(epoch, len(per_epoch)) - 1]


class _Cfg(dict):
    """The attribute / item / ``in`` access of the reference's configuration objects."""
    __getattr__ = dict.__getitem__


def reference_methods(scope: dict):
    """``Solver.train`` and ``Solver._run_one_epoch`` of bm/solver.py as plain functions of ``self``."""
    from _ref_import import REF
    path = REF / "bm" / "solver.py"
    tree = ast.parse(path.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Solver")
    out = []
    for name in ("train", "_run_one_epoch"):
        fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
        fn.decorator_list = []
        fn.returns = None
        for arg in fn.args.args:
            arg.annotation = None
        exec(compile(ast.Module(body=[fn], type_ignores=[]), str(path), "exec"), scope)
        out.append(scope[name])
    return out


def averager(beta: float = 1):
    """flashy.averager, restated from its published source (flashy/utils.py): exponential moving average with
    ``beta`` = 1, i.e. the plain mean of ``float(value)`` in the order of the updates."""
    fix: dict = defaultdict(float)
    total: dict = defaultdict(float)

    def _update(metrics, weight: float = 1):
        nonlocal total, fix
        for key, value in metrics.items():
            total[key] = total[key] * beta + weight * float(value)
            fix[key] = fix[key] * beta + weight
        return {key: tot / fix[key] for key, tot in total.items()}
    return _update


class _Recorder:
    def __init__(self):
        self.stages, self.modes, self.processed, self.set_epoch, self.averaged = [], [], [], [], []
        self.test_saw, self.totals, self.copied, self.commits = [], [], [], 0


class _Loader:
    def __init__(self, solver, phase: str, per_epoch, rec: _Recorder):
        self.solver, self.phase, self.per_epoch, self.rec = solver, phase, per_epoch, rec
        self.sampler = types.SimpleNamespace(set_epoch=lambda e: rec.set_epoch.append([phase, e]))

    def __len__(self):
        return len(epoch_losses(self.per_epoch, self.solver.epoch))

    def __iter__(self):
        epoch = self.solver.epoch
        for i in range(len(epoch_losses(self.per_epoch, epoch))):
            yield (self.phase, epoch, i)


class _LogProgress:
    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        return iter(self.loader)

    def update(self, **metrics):
        pass


class _Modules:
    """``all_models`` / ``loss``: ``train(mode)`` records; the state is the epoch that made it."""

    def __init__(self, solver, name: str, rec: _Recorder):
        self.solver, self.name, self.rec = solver, name, rec

    def train(self, mode=True):
        self.rec.modes.append([self.name, bool(mode)])

    def state_dict(self):
        return dict(self.solver.live_state)

    def __call__(self, estimate, output, features_mask):
        return estimate


class StubSolver:
    """What ``train`` and ``_run_one_epoch`` touch on ``self``.  ``epoch``, ``run_stage`` and ``commit`` restate
    flashy.BaseSolver (flashy/solver.py): the epoch is ``len(history) + 1``, a stage's metrics wait in a pending dict,
    ``commit`` appends that dict to the history (and would save the checkpoint)."""

    def __init__(self, spec: dict, rec: _Recorder):
        self.rec, self.spec = rec, spec
        self.args = _Cfg(optim=_Cfg(epochs=spec["epochs"], max_batches=spec["max_batches"], negatives=None, svd=0.,
                                    loss="clip"),
                         early_stop_patience=spec["early_stop_patience"], eval_every=spec["eval_every"], num_prints=0)
        self.history, self._pending, self.current_stage = [], {}, None
        self.best_state, self.best_loss, self.best_epoch, self.last_test_epoch = None, float("inf"), 0, 0
        self.live_state = {"epoch": 0}
        if spec["resume"]:
            r = spec["resume"]
            self.history = [dict(h) for h in r["history"]]
            self.best_epoch, self.best_loss, self.last_test_epoch = r["best_epoch"], r["best_loss"], r["last_test_epoch"]
            self.best_state = {"epoch": r["best_epoch"]}
            self.live_state = {"epoch": len(self.history)}
        self.all_models = _Modules(self, "all_models", rec)
        self.loss = _Modules(self, "loss", rec)
        self.model = types.SimpleNamespace(modules=lambda: [])
        self.optimizer = types.SimpleNamespace(zero_grad=lambda: None, step=self._optimizer_step)
        self.loaders = {"train": _Loader(self, "train", spec["train"], rec),
                        "valid": _Loader(self, "valid", spec["valid"], rec)}
        self.scale_reject = None
        self.negative_pool = {"train": torch.zeros(0), "valid": torch.zeros(0)}
        self.result_logger = types.SimpleNamespace(_log_summary=lambda *a, **k: None)

    @property
    def epoch(self):
        return len(self.history) + 1

    def _optimizer_step(self):
        self.live_state = {"epoch": self.epoch}         # training made a new state

    def get_formatter(self, stage_name):
        return None

    def log_progress(self, stage, loader, updates=0, total=None):
        self.rec.totals.append([stage, self.epoch, total])
        return _LogProgress(loader)

    def run_stage(self, name, method, *args, **kwargs):
        self.rec.stages.append([self.epoch, name])
        self.current_stage = name
        metrics = method(*args, **kwargs)
        self._pending[name] = metrics
        self.current_stage = None
        return metrics

    def commit(self):
        self.history.append(self._pending)
        self._pending = {}
        self.rec.commits += 1

    def _process_batch(self, batch, training=False):
        phase, epoch, i = batch
        self.rec.processed.append([phase, epoch, i])
        value = epoch_losses(self.spec[phase], epoch)[i]
        if value is None:
            return None, None, None, None
        estimate = torch.tensor(value, dtype=torch.float32, requires_grad=bool(training))
        return estimate, torch.zeros(1), torch.ones(1, dtype=torch.bool), torch.ones(1, dtype=torch.bool)

    def _test_one_epoch(self):
        self.rec.test_saw.append([self.epoch, self.live_state["epoch"]])
        return {"wer": 0.5}


def run_case(spec: dict) -> dict:
    rec = _Recorder()
    solver = StubSolver(spec, rec)

    def copy_state(state):
        rec.copied.append([solver.epoch, state["epoch"]])
        return dict(state)

    @contextlib.contextmanager
    def swap_state(models, state):
        old = copy_state(models.state_dict())
        rec.copied.pop()
        solver.live_state = dict(state)
        try:
            yield
        finally:
            solver.live_state = old

    def average_metrics(metrics, count=1.):
        rec.averaged.append([{k: float(v) for k, v in metrics.items()}, count])
        return dict(metrics)
    flashy = types.SimpleNamespace(
        averager=averager,
        distrib=types.SimpleNamespace(is_distributed=lambda: spec["distributed"], average_metrics=average_metrics,
                                      sync_model=lambda models: None))
    scope = {"torch": torch, "flashy": flashy, "logger": logging.getLogger("bm_ref_solver"), "bold": lambda s: s,
             "copy_state": copy_state, "swap_state": swap_state, "svd_penalty": None}
    train, run_one_epoch = reference_methods(scope)
    solver._run_one_epoch = types.MethodType(run_one_epoch, solver)
    raised = None
    try:
        train(solver)
    except RuntimeError as exc:
        raised = f"{type(exc).__name__}: {exc}"
    return dict(stages=rec.stages, modes=rec.modes, processed=rec.processed, set_epoch=rec.set_epoch,
                averaged=rec.averaged, test_saw=rec.test_saw, totals=rec.totals, best_copied=rec.copied,
                commits=rec.commits, history=solver.history, best_epoch=solver.best_epoch,
                best_loss="inf" if solver.best_loss == float("inf") else solver.best_loss,
                best_state_epoch=None if solver.best_state is None else solver.best_state["epoch"],
                live_state_epoch=solver.live_state["epoch"], last_test_epoch=solver.last_test_epoch, raised=raised)


def build() -> dict:
    import warnings
    logging.getLogger("bm_ref_solver").setLevel(logging.ERROR)
    # the reference hands its averager the loss with its graph attached (bm/solver.py:389)
    warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad=True to a scalar")
    cases = {name: dict(settings=spec, result=run_case(spec)) for name, spec in CASES.items()}
    # the issue's trial, as a check of the stubs: stops after epoch 5, best epoch 2, the test ran at epoch 2 only
    r = cases["patience_hit"]["result"]
    assert len(r["history"]) == 5 and r["best_epoch"] == 2 and r["test_saw"] == [[2, 2]] and r["last_test_epoch"] == 2, r
    r = cases["rejected_middle"]["result"]
    assert r["history"][0]["train"]["loss"] == 2.25, r                 # 1, 2, rejected (2 again), 4
    assert cases["rejected_first_train"]["result"]["raised"] == "RuntimeError: Empty batch and last batch is none"
    return dict(meta=dict(torch=torch.__version__, reference="bm/solver.py:189-228, 325-401"), cases=cases)


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    (dest / "train_loop.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"train_loop: {len(out['cases'])} cases -> {dest / 'train_loop.json'} "
          f"({(dest / 'train_loop.json').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
