"""The epoch and the training loop around ``Solver.train_step`` / ``eval_step``: ``run_epoch`` mirrors
``_run_one_epoch`` (bm/solver.py:325-401), ``fit`` mirrors ``train`` (bm/solver.py:189-228) and what it uses of
``flashy.BaseSolver`` (``epoch``, ``run_stage``, ``commit``), ``restore`` mirrors bm/solver.py:104-118.  The ``Solver``
methods of the same names are pure dispatch onto this module.

No kernel lives here: an epoch's device work is the existing step.  What the loop owes the GPU is to add nothing to it:

  * the losses of an epoch stay on the device, in one resident fp32 array (``LossRecord``); the written part is read
    back ONCE, after the last step (``read_losses``; additionally at ``num_prints`` evenly spaced steps for a log
    line).  The epoch's loss is the sequential fp64 sum in step order over the count: what ``flashy.averager()``
    computes from ``float(loss)`` per step;
  * a training step gets the batch behind it (``train_step(batch, next_batch)``), and the last step of an epoch --
    also one forced by ``max_batches`` -- gets ``None``: nothing is prefetched that nobody consumes;
  * a state that is swapped in (``swap_state``, ``restore``, ``load_best``) is followed by ``hip_ops.weights_changed()``:
    the packed f16x2 weight planes and the cached weight maxima belong to the weights that were swapped out.

Everything here works on CPU tensors too (a solver whose steps return CPU losses): the control flow is tested without
a GPU.

Not built: tensorboard / wandb, Dora XPs and signatures, hydra configuration, the replay of past metrics to a result
logger, restoring RNG states (the reference does not restore them either), and deferring the validation batches' flag
reads the way ``train_step`` defers its own."""
import contextlib
import logging
import os
import typing as tp
from pathlib import Path

import torch

from . import distrib
from . import hip_ops as H

logger = logging.getLogger(__name__)

_END = object()


# -- the loss record --------------------------------------------------------------------------------------------
class LossRecord:
    """One fp32 slot per step of an epoch, on the device of the first loss it is handed."""

    def __init__(self, size: int):
        self.size = max(int(size), 1)
        self.values: tp.Optional[torch.Tensor] = None
        self.count = 0

    def put(self, idx: int, loss: torch.Tensor) -> None:
        """Device-to-device copy of a step's loss into slot ``idx``: no host read."""
        loss = loss.detach()
        if self.values is None:
            self.values = torch.zeros(self.size, dtype=torch.float32, device=loss.device)
        if idx >= self.size:                    # a loader that yields more batches than its len() announced
            self.size = max(2 * self.size, idx + 1)
            grown = torch.zeros(self.size, dtype=torch.float32, device=self.values.device)
            grown[:len(self.values)].copy_(self.values)
            self.values = grown
        self.values[idx:idx + 1].copy_(loss.reshape(1))
        self.count = max(self.count, idx + 1)


def read_losses(record: LossRecord, count: int) -> tp.List[float]:
    """THE host read of an epoch's losses: the first ``count`` slots, one copy."""
    return record.values[:count].cpu().tolist()


def sequential_mean(values: tp.Sequence[float]) -> float:
    """``flashy.averager()`` (beta = 1) over ``float(loss)`` per step: the fp64 sum in step order over the count."""
    total = 0.0
    for v in values:
        total += float(v)
    return total / len(values)


def _log_every(total: int, num_prints: int) -> int:
    return max(1, total // num_prints) if num_prints > 0 else 0


# -- model state ------------------------------------------------------------------------------------------------
def model_state(solver) -> tp.Dict[str, tp.Dict[str, torch.Tensor]]:
    """The state of ``[model, feature_model]`` (bm/solver.py:38 ``all_models``): references to the live tensors."""
    state = {"model": solver.model.state_dict()}
    if solver.feature_model is not None:
        state["feature_model"] = solver.feature_model.state_dict()
    return state


def copy_state(state, device: tp.Optional[str] = None):
    """bm/utils.py:96-97 with the copy's home a choice: a clone of every tensor where it lives (``device`` None), or
    on ``device``.  Never a reference to a live tensor."""
    def clone(v):
        if not isinstance(v, torch.Tensor):
            return v
        v = v.detach()
        return v.clone() if device is None or v.device == torch.device(device) else v.to(device, copy=True)
    return {name: {k: clone(v) for k, v in part.items()} for name, part in state.items()}


def load_model_state(solver, state) -> None:
    """``all_models.load_state_dict(state)``, then ``weights_changed()``: the packed weight planes and the amax cache
    belong to the weights that were overwritten."""
    solver.model.load_state_dict(state["model"])
    if solver.feature_model is not None and state.get("feature_model") is not None:
        solver.feature_model.load_state_dict(state["feature_model"])
    H.weights_changed()


@contextlib.contextmanager
def swap_state(solver, state):
    """bm/utils.py:100-115 for the solver's models: clone the live state, load ``state``, yield, load the clone back."""
    old = copy_state(model_state(solver))
    load_model_state(solver, state)
    try:
        yield
    finally:
        load_model_state(solver, old)


def _best_device(solver) -> tp.Optional[str]:
    best_on = getattr(solver, "best_on", "device")
    if best_on not in ("device", "cpu"):
        raise ValueError(f"best_on = {best_on!r}: 'device' or 'cpu'")
    return None if best_on == "device" else "cpu"


# -- bm/solver.py:325-401 ---------------------------------------------------------------------------------------
def _set_epoch(loader, epoch: int) -> None:
    target = loader if hasattr(loader, "set_epoch") else getattr(loader, "sampler", None)
    if target is not None and hasattr(target, "set_epoch"):
        target.set_epoch(epoch)


def _drop_prefetch(solver) -> None:
    """A batch that was handed over as ``next_batch`` and will not be consumed (an assert ended the epoch)."""
    if getattr(solver, "_prefetched", None) is not None:
        if getattr(solver, "_gather", None) is not None:
            solver._gather.cancel()
        solver._prefetched = None
    staged = getattr(solver, "_staged", None)
    if staged:
        staged.clear()


class _Progress:
    """The log lines of ``num_prints``: the record is read at evenly spaced steps, never with ``num_prints`` 0."""

    def __init__(self, stage: str, total: int, num_prints: int):
        self.stage, self.total, self.left = stage, total, num_prints
        self.every = _log_every(total, num_prints)

    def step(self, record: LossRecord, done: int) -> None:
        if self.left > 0 and done % self.every == 0 and done < self.total:
            self.left -= 1
            logger.info("%s | %d/%d | loss %.4f", self.stage, done, self.total,
                        sequential_mean(read_losses(record, done)))


def _train_steps(solver, loader, record: LossRecord, max_batches, progress: _Progress) -> int:
    solver._last_batch = None                   # bm/solver.py:341: the last good batch is the epoch's own
    it = iter(loader)
    idx = 0
    try:
        batch = next(it, _END)
        while batch is not _END:
            last = bool(max_batches) and idx + 1 == max_batches
            following = _END if last else next(it, _END)
            loss = solver.train_step(batch, None if following is _END else following)
            record.put(idx, loss)
            idx += 1
            progress.step(record, idx)
            batch = following
    finally:
        _drop_prefetch(solver)
        close = getattr(it, "close", None)
        if close is not None:
            close()
    return idx


def _valid_steps(solver, loader, record: LossRecord, max_batches, progress: _Progress) -> int:
    last_batch = None
    idx = 0
    for batch in loader:
        loss = solver._eval_loss(batch)
        if loss is None:                        # bm/solver.py:345-352: the batch held only rejected segments
            if last_batch is None:
                raise RuntimeError("Empty batch and last batch is none")
            loss = solver._eval_loss(last_batch)
        else:
            last_batch = batch
        record.put(idx, loss)
        idx += 1
        progress.step(record, idx)
        if idx == max_batches:
            break
    return idx


def run_epoch(solver, loader, training: bool, *, max_batches: tp.Optional[int] = None,
              num_prints: int = 0) -> tp.Dict[str, float]:
    """One pass over ``loader``: ``{"loss": mean of the steps' losses}``, averaged over the ranks by step count.  A
    validation epoch whose loss is below ``best_loss`` records ``best_loss``, ``best_epoch`` and a clone of the
    models' state.  An exception of a step propagates; nothing of the solver's bookkeeping has been touched by then."""
    if training and distrib.is_distributed():
        _set_epoch(loader, solver.epoch - 1)    # bm/solver.py:331-334
    total = len(loader)
    if max_batches:
        total = min(total, max_batches)
    record = LossRecord(total)
    progress = _Progress("train" if training else "valid", total, num_prints)
    if training:
        n_steps = _train_steps(solver, loader, record, max_batches, progress)
    else:
        with torch.no_grad():
            n_steps = _valid_steps(solver, loader, record, max_batches, progress)
    if n_steps == 0:
        raise ValueError("run_epoch: the loader yielded no batch")
    metrics = {"loss": sequential_mean(read_losses(record, n_steps))}
    metrics = distrib.average_metrics(metrics, n_steps)
    if not training and metrics["loss"] < solver.best_loss:
        solver.best_loss = metrics["loss"]
        solver.best_epoch = solver.epoch
        logger.info("New best valid loss %.4f", solver.best_loss)
        solver.best_state = copy_state(model_state(solver), _best_device(solver))
    return metrics


# -- bm/solver.py:189-228 ---------------------------------------------------------------------------------------
def save_checkpoint(solver, checkpoint) -> None:
    """``flashy.BaseSolver.commit``'s checkpoint.  EVERY rank calls ``state_dict()`` (it gathers the sharded Adam
    moments); rank 0 writes to a temporary file next to ``checkpoint`` and renames it; then every rank meets."""
    state = solver.state_dict()
    if distrib.rank() == 0:
        payload = {"solver": state, "best_state": solver.best_state, "best_loss": solver.best_loss,
                   "best_epoch": solver.best_epoch, "last_test_epoch": solver.last_test_epoch,
                   "history": solver.history, "loss": solver.loss.state_dict()}
        scaler = getattr(getattr(solver, "scale_reject", None), "scaler", None)
        if scaler is not None and hasattr(scaler, "state_dict"):
            payload["scaler"] = scaler.state_dict()
        path = Path(checkpoint)
        tmp = path.with_name(path.name + f".tmp.{os.getpid()}")
        try:
            torch.save(payload, tmp)
            os.replace(tmp, path)
        finally:
            if tmp.exists():
                tmp.unlink()
    distrib.barrier()


def _to_home(solver, state):
    return None if state is None else copy_state(state, _best_device(solver) or solver.device)


def restore(solver, checkpoint, *, continue_from=None, continue_best: bool = True) -> bool:
    """bm/solver.py:104-118.  ``checkpoint`` exists: everything is loaded, True.  Otherwise, with ``continue_from`` (a
    path), only the models are loaded -- from its ``best_state`` when ``continue_best``, else from its model state --
    the history stays empty, False."""
    if checkpoint is not None and Path(checkpoint).exists():
        state = torch.load(Path(checkpoint), map_location="cpu")
        solver.load_state_dict(state["solver"])
        solver.loss.load_state_dict(state["loss"])
        H.weights_changed()
        scaler = getattr(getattr(solver, "scale_reject", None), "scaler", None)
        if scaler is not None and "scaler" in state:
            scaler.load_state_dict(state["scaler"])
        solver.best_state = _to_home(solver, state["best_state"])
        solver.best_loss = state["best_loss"]
        solver.best_epoch = state["best_epoch"]
        solver.last_test_epoch = state["last_test_epoch"]
        solver.history = list(state["history"])
        return True
    if continue_from:
        path = Path(continue_from)
        assert path.exists(), "Could not find checkpoint " + str(path)
        state = torch.load(path, map_location="cpu")
        if continue_best:
            load_model_state(solver, state["best_state"])
        else:
            load_model_state(solver, {k: state["solver"].get(k) for k in ("model", "feature_model")})
    return False


def load_best(solver) -> None:
    """bm/solver.py:63-64: the best state into the models."""
    if solver.best_state is None:
        raise RuntimeError("load_best: no validation epoch has recorded a best state")
    load_model_state(solver, solver.best_state)


def fit(solver, train_loader, valid_loader, *, epochs: int, test: tp.Optional[tp.Callable[[], dict]] = None,
        eval_every: int = 1, early_stop_patience: tp.Optional[int] = None, max_batches: tp.Optional[int] = None,
        checkpoint=None, num_prints: int = 0) -> tp.List[dict]:
    """Epochs ``solver.epoch .. epochs``: the stages ``train`` and ``valid``, the ``test`` stage on the best state when
    it is due, then the commit (the epoch's ``{stage: metrics}`` joins ``history``; the checkpoint is written)."""
    for epoch in range(solver.epoch, epochs + 1):
        stages: tp.Dict[str, dict] = {}
        stages["train"] = run_epoch(solver, train_loader, True, max_batches=max_batches, num_prints=num_prints)
        with torch.no_grad():
            stages["valid"] = run_epoch(solver, valid_loader, False, max_batches=max_batches, num_prints=num_prints)
        for name in ("train", "valid"):
            logger.info("%s | epoch %d | loss %.4f", name, epoch, stages[name]["loss"])

        will_stop = epoch == epochs
        if early_stop_patience:
            if solver.epoch >= solver.best_epoch + early_stop_patience:
                logger.warning("Model valid_loss did not improve for %d epochs. Stopping the training.",
                               early_stop_patience)
                will_stop = True

        if test is not None and (epoch % eval_every == 0 or will_stop):
            if solver.best_epoch > solver.last_test_epoch:
                assert solver.best_state is not None
                with swap_state(solver, solver.best_state):
                    with torch.no_grad():
                        stages["test"] = test()
                solver.last_test_epoch = epoch
        if getattr(solver, "scale_reject", None) is not None:
            logger.info("Scale Reject | Ratio %.3f%%", 100 * solver.scale_reject.rejection_rate)
        solver.history.append(stages)
        if checkpoint is not None:
            save_checkpoint(solver, checkpoint)
        if will_stop:
            break
    return solver.history


__all__ = ["LossRecord", "read_losses", "sequential_mean", "model_state", "copy_state", "load_model_state", "swap_state",
           "run_epoch", "save_checkpoint", "restore", "load_best", "fit"]
