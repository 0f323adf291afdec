"""Test metrics of a decoding model: mirror of ``bm/metrics.py`` (``OnlineCorrelation``, ``L1Reg``, ``L2Reg``,
``ClassificationAcc``) and of ``bm/play.py:get_test_metrics`` / the decode branch of
``bm/solver.py:get_metric_constructors``.

Same API as the reference (``get_constructor``, ``update(left, right, mask)``, ``get()``, ``reduce(stats)``, the
slices and the names).  ``update`` is ONE pass of the HIP kernel ``bm_regress_metric_update`` over the batch: the
per-(f, t) fp64 sums over the batch dimension (the reference's ``dim=0``), accumulated on the device; ``get()`` finishes
with the reference's fp64 torch ops on those [F, T] accumulators.  The inputs are fp32 (what the model and the features
are): the reference casts them to double (bm/play.py:149-151), which is exact, and every product the kernel forms is
the one the reference forms in double -- only the order of the sums over the batch differs.
"""
import typing as tp
from functools import partial

import torch

from . import distrib
from . import hip_ops as H

_DOT, _LEFT, _RIGHT, _LEFT2, _RIGHT2, _COUNT, _L2, _L1 = range(H.METRIC_PLANES)


class TestMetric:
    """bm/metrics.py:16-34."""
    __test__ = False        # (not a pytest class)

    def __init__(self, left_slice: slice, right_slice: slice, name: str = "metric"):
        self.name = name
        self.left_slice = left_slice
        self.right_slice = right_slice

    @classmethod
    def get_constructor(cls, *args: tp.Any, **kwargs: tp.Any) -> tp.Callable[..., "TestMetric"]:
        return partial(cls, *args, **kwargs)

    def update(self, left: torch.Tensor, right: torch.Tensor, mask: torch.Tensor) -> "TestMetric":
        raise NotImplementedError()

    def get(self) -> torch.Tensor:
        raise NotImplementedError()

    @classmethod
    def reduce(cls, stats: tp.List[torch.Tensor]) -> float:
        return torch.stack(stats).mean().item()


class _ColumnSums(TestMetric):
    """The accumulators of every metric here: [8, F, T - t0] fp64 per-(f, t) sums over the batch (see hip_ops
    METRIC_PLANES), filled by the HIP kernel.  Metrics updated together by ``update_all`` with the same slices share one
    accumulator (one kernel pass); a metric of such a group that is then updated on its own first takes a private copy,
    so that nothing is counted twice."""

    def __init__(self, left_slice: slice, right_slice: slice, name: str, dim: int = 0):
        super().__init__(left_slice, right_slice, name)
        if dim != 0:
            raise NotImplementedError("brainmagick_amd metrics accumulate over the batch dimension (dim=0) only")
        self.dim = dim
        self._acc: tp.Optional[torch.Tensor] = None
        self._peers: tp.List["_ColumnSums"] = [self]       # the metrics that share self._acc (update_all)

    def _unshare(self) -> None:
        if len(self._peers) > 1:
            self._peers.remove(self)
            self._peers = [self]
            self._acc = self._acc.clone()

    def _sliced(self, left, right):
        return left[:, self.left_slice], right[:, self.right_slice]

    def update(self, left: torch.Tensor, right: torch.Tensor, mask: tp.Optional[torch.Tensor],
               t0: int = 0) -> "_ColumnSums":
        """``left`` / ``right``: fp32 [B, C, T] on the GPU; ``mask``: bool [B, 1, T] or [B, F, T] (None: all true).
        ``t0`` (extension): only the samples t >= t0 count -- ``x[..., t0:]`` without a copy."""
        update_all([self], left, right, mask, t0)
        return self

    def _planes(self) -> torch.Tensor:
        if self._acc is None:
            raise RuntimeError(f"metric {self.name!r}: get() before any update()")
        return self._acc


def _common_window(tensors: tp.Sequence[torch.Tensor]):
    """(base tensors, a) when every tensor is the same time window ``x[..., a:]`` (a > 0) of a contiguous 3-d tensor
    ``x`` -- what ``Solver._process_batch`` returns for the encode task -- else None."""
    bases, start = [], None
    for t in tensors:
        base = t._base
        if base is None or t.dim() != 3 or base.dim() != 3 or not base.is_contiguous() or \
                base.shape[:2] != t.shape[:2] or t.stride() != base.stride():
            return None
        a = t.storage_offset() - base.storage_offset()
        if a <= 0 or a + t.shape[2] != base.shape[2] or (start is not None and a != start):
            return None
        start = a
        bases.append(base)
    return bases, start


def update_all(metrics: tp.Sequence[TestMetric], left: torch.Tensor, right: torch.Tensor,
               mask: tp.Optional[torch.Tensor], t0: int = 0) -> None:
    """``metric.update(left, right, mask)`` for every metric, with ONE kernel pass per distinct pair of slices: metrics
    with the same slices that are always updated together share their accumulator (an L2Reg and an OnlineCorrelation of
    one feature).  A ``ClassificationAcc`` in the list takes its own pass.  Operands that are all the same window
    ``x[..., a:]`` of contiguous tensors are read in place: the kernels walk the base tensors from ``t0 + a``; any other
    non-contiguous layout is copied once by the kernel wrappers."""
    for t, what in ((left, "left"), (right, "right")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"brainmagick_amd metrics run on the MI355X HIP path only (no CPU fallback): {what} is "
                               f"on {t.device if isinstance(t, torch.Tensor) else type(t)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: expected float32 (the kernel accumulates in float64), got {t.dtype}")
    if mask is not None and mask.dtype != torch.bool:
        raise TypeError(f"mask must be a bool tensor, got {mask.dtype}")
    window = _common_window([left, right] + ([mask] if mask is not None else []))
    if window is not None:
        (left, right, *rest), start = window
        mask = rest[0] if rest else None
        t0 += start
    groups: tp.Dict[tp.Any, tp.List[_ColumnSums]] = {}
    for m in metrics:
        if isinstance(m, ClassificationAcc):
            m._count_batch(left, right, mask, t0)
            continue
        key = (m.left_slice.start, m.left_slice.stop, m.left_slice.step,
               m.right_slice.start, m.right_slice.stop, m.right_slice.step)
        groups.setdefault(key, []).append(m)
    for group in groups.values():
        l, r = group[0]._sliced(left, right)
        ids = {id(m) for m in group}

        def zeros():
            return torch.zeros(H.METRIC_PLANES, l.shape[1], l.shape[2] - t0, device=l.device, dtype=torch.float64)
        if all(m._acc is None for m in group):
            acc, peers = zeros(), list(group)
            for m in group:
                m._acc, m._peers = acc, peers
            H.regress_metric_update(l, r, mask, acc, t0)
        elif all(m._peers is group[0]._peers for m in group) and {id(m) for m in group[0]._peers} == ids:
            H.regress_metric_update(l, r, mask, group[0]._acc, t0)
        else:
            for m in group:          # groups that were updated differently before: every metric on its own
                m._unshare()
                if m._acc is None:
                    m._acc = zeros()
                H.regress_metric_update(l, r, mask, m._acc, t0)


class OnlineCorrelation(_ColumnSums):
    """bm/metrics.py:37-114 (real-valued): the correlation over the batch dimension, per (channel, time)."""

    def __init__(self, left_slice: slice, right_slice: slice, name: str = "correlation", dim: int = 0,
                 tol: float = 1e-8):
        super().__init__(left_slice, right_slice, name, dim)
        assert tol >= 0
        self.tol = tol

    def get(self) -> torch.Tensor:
        acc = self._planes()
        count = acc[_COUNT]

        def _norm_centered(sum_, sum_squared):
            norm_squared = sum_squared - sum_.abs().pow(2) / count
            if norm_squared.min() < -self.tol:
                raise ValueError(
                    f"Numerical instabilities when computing the correlation. "
                    f"Expected {sum_squared} - {sum_}**2 / {count} to be positive "
                    f"but got {norm_squared.min()}")
            return norm_squared.clamp_(0, float('inf')).sqrt_()

        norm_left = _norm_centered(acc[_LEFT], acc[_LEFT2])
        norm_right = _norm_centered(acc[_RIGHT], acc[_RIGHT2])
        dot = acc[_DOT] - acc[_LEFT] * acc[_RIGHT] / count
        correlation = dot / (norm_left * norm_right).clamp(self.tol, float('inf'))
        assert not torch.isnan(correlation).any(), "Tensor contain nans. Perhaps division by " \
                                                   f"zero cause that? {correlation}"
        return correlation


class AccumulativeMetric(_ColumnSums):
    """bm/metrics.py:117-149: sum over the batch of a per-element term, divided by the mask count."""
    _plane = -1

    def __init__(self, left_slice: slice, right_slice: slice, name: str = "N/A", dim: int = 0):
        super().__init__(left_slice, right_slice, name, dim)

    def get(self) -> torch.Tensor:
        if self._acc is None:
            return torch.Tensor([0.])
        count = self._acc[_COUNT]
        if count.sum() == 0:
            return torch.Tensor([0.])
        ret = self._acc[self._plane] / count
        assert not torch.isnan(ret).any(), "Tensor contain nans. Perhaps division by " \
                                           f"zero cause that? {ret}"
        return ret


class L1Reg(AccumulativeMetric):
    """bm/metrics.py:152-154: sum |(l - r) m|."""
    _plane = _L1


class L2Reg(AccumulativeMetric):
    """bm/metrics.py:157-163: sum ((l - r) m)^2; reduce = sqrt of the mean."""
    _plane = _L2

    @classmethod
    def reduce(cls, stats: tp.List[torch.Tensor]) -> float:
        return torch.stack(stats).mean().sqrt().item()


class ClassificationAcc(TestMetric):
    """bm/metrics.py:173-180: the share of selected positions whose arg-max over the class logits ``left[:, left_slice]``
    equals the class in ``right[:, right_slice]`` (one channel), per time sample over the batch.  ``update`` is one pass
    of the HIP kernel ``bm_class_acc_update`` into int64 [2, T - t0] counts (hits, selected) on the device."""

    def __init__(self, left_slice: slice, right_slice: slice, name: str = "N/A", dim: int = 0):
        super().__init__(left_slice, right_slice, name)
        if dim != 0:
            raise NotImplementedError("brainmagick_amd metrics accumulate over the batch dimension (dim=0) only")
        self.dim = dim
        self._acc: tp.Optional[torch.Tensor] = None

    def _count_batch(self, left, right, mask, t0):
        for t, what in ((left, "left"), (right, "right")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"brainmagick_amd metrics run on the MI355X HIP path only (no CPU fallback): {what} "
                                   f"is on {t.device if isinstance(t, torch.Tensor) else type(t)}")
        logits, target = left[:, self.left_slice], right[:, self.right_slice]
        if self._acc is None:
            self._acc = torch.zeros(2, logits.shape[2] - t0, device=logits.device, dtype=torch.int64)
        H.class_acc_update(logits, target, mask, self._acc, t0)

    def update(self, left: torch.Tensor, right: torch.Tensor, mask: tp.Optional[torch.Tensor],
               t0: int = 0) -> "ClassificationAcc":
        """``left``: fp32 [B, C, T] logits, ``right``: fp32 [B, C', T] with the class as a float, on the GPU; ``mask``:
        bool [B, 1, T] (None: all true).  ``t0`` (extension): only the samples t >= t0 count."""
        self._count_batch(left, right, mask, t0)
        return self

    def get(self) -> torch.Tensor:
        """AccumulativeMetric.get (bm/metrics.py:147-153): fp64 [1, T'] hits / count, or tensor([0.]) when nothing was
        counted."""
        if self._acc is None or self._acc[1].sum() == 0:
            return torch.Tensor([0.])
        ret = (self._acc[0].double() / self._acc[1].double())[None]
        assert not torch.isnan(ret).any(), "Tensor contain nans. Perhaps division by " \
                                           f"zero cause that? {ret}"
        return ret


def metric_constructors(used_features) -> tp.List[tp.Callable[..., TestMetric]]:
    """bm/solver.py:410-432, the decode task: per feature of ``used_features`` (the features builder, duck-typed as for
    ``losses.FeatureDecodingLoss``) ``ClassificationAcc("acc_<name>")`` if it is categorical, else ``L2Reg("l2_<name>")``
    and ``OnlineCorrelation("corr_<name>")``, with the reference's argument order (the L2 metric takes the feature slice
    first)."""
    ctors: tp.List[tp.Callable[..., TestMetric]] = []
    for feature in used_features.values():
        name = feature.name
        feature_slice = used_features.get_slice(name)
        model_out_slice = used_features.get_slice(name, model_output=True)
        if feature.categorical:
            ctors.append(ClassificationAcc.get_constructor(model_out_slice, feature_slice, name=f"acc_{name}"))
        else:
            ctors += regression_metric_constructors(name, feature_slice, model_out_slice)
    return ctors


def regression_metric_constructors(feature_name: str, feature_slice: slice = slice(None),
                                   model_out_slice: slice = slice(None)) -> tp.List[tp.Callable[..., TestMetric]]:
    """bm/solver.py:409-432, non-categorical feature: [L2Reg("l2_<name>"), OnlineCorrelation("corr_<name>")] with the
    reference's argument order (the L2 metric takes the feature slice first)."""
    return [L2Reg.get_constructor(feature_slice, model_out_slice, name=f"l2_{feature_name}"),
            OnlineCorrelation.get_constructor(model_out_slice, feature_slice, name=f"corr_{feature_name}")]


def encode_metric_constructors() -> tp.List[tp.Callable[..., TestMetric]]:
    """bm/solver.py:408-409, the encode task: the correlation of the predicted with the recorded MEG."""
    return [OnlineCorrelation.get_constructor(slice(None), slice(None), "corr_meg")]


def encode_trim_offset(sample_rate: float, tmin: float, meg_init: float) -> int:
    """bm/solver.py:436-439: the samples the encode task's test metrics leave out IN FRONT of those the Solver already
    removed (``_process_batch`` returns the samples after ``meg_init``): up to the stimulus onset at ``-tmin``."""
    time_offset = -tmin
    time_offset -= meg_init
    return int(sample_rate * time_offset)


def merge_rank_results(per_rank: tp.Sequence[tp.Dict[str, tp.List[torch.Tensor]]],
                       n_recordings: int) -> tp.Dict[str, tp.List[torch.Tensor]]:
    """bm/play.py:158-166 without the communication: rank r evaluated recordings r, r + world, ...; returns, per
    metric, the results in recording order."""
    world = len(per_rank)
    names = list(per_rank[0]) if per_rank else []
    out: tp.Dict[str, tp.List[tp.Optional[torch.Tensor]]] = {name: [None] * n_recordings for name in names}
    for r, results in enumerate(per_rank):
        for name in names:
            mine = list(range(n_recordings))[r::world]
            if len(results[name]) != len(mine):
                raise ValueError(f"rank {r} returned {len(results[name])} results of {name!r} for {len(mine)} "
                                 "recordings")
            for index, value in zip(mine, results[name]):
                out[name][index] = value
    for name, results in out.items():
        assert all(x is not None for x in results), name
    return out   # type: ignore[return-value]


def _exchange(results: tp.Dict[str, tp.List[torch.Tensor]], n_recordings: int):
    """Every rank's per-recording results on every rank (one fp32 all-reduce of a zero-padded table)."""
    world, rank = distrib.world_size(), distrib.rank()
    names = list(results)
    # the widest result of ANY rank decides the slot width (a rank may hold no recording, or only zero-count results)
    widest = torch.tensor([float(max([t.numel() for v in results.values() for t in v] + [1]))],
                          device=distrib.comm().scalar_device())
    distrib.comm().all_reduce(widest, op="max")
    per_slot = int(widest.item())
    width = 3 + per_slot                               # ndim, two dims, values
    slots = -(-n_recordings // world)
    table = torch.zeros(world, len(names), slots, width, dtype=torch.float32)
    for i, name in enumerate(names):
        for j, t in enumerate(results[name]):
            t = t.float().reshape(t.shape if t.dim() else (1,))
            table[rank, i, j, 0] = t.dim()
            table[rank, i, j, 1:1 + t.dim()] = torch.tensor(t.shape, dtype=torch.float32)
            table[rank, i, j, 3:3 + t.numel()] = t.flatten()
    flat = table.to(distrib.comm().scalar_device())
    distrib.comm().all_reduce(flat)
    table = flat.cpu()
    per_rank = []
    for r in range(world):
        mine = len(range(n_recordings)[r::world])
        entry = {}
        for i, name in enumerate(names):
            vals = []
            for j in range(mine):
                row = table[r, i, j]
                ndim = int(row[0])
                shape = [int(x) for x in row[1:1 + ndim]]
                n = 1
                for s in shape:
                    n *= s
                vals.append(row[3:3 + n].reshape(shape).clone())
            entry[name] = vals
        per_rank.append(entry)
    return merge_rank_results(per_rank, n_recordings)


def regression_test_metrics(solver, recordings: tp.Sequence[tp.Iterable], trim_offset: int = 0,
                            metrics: tp.Optional[tp.List[tp.Callable[..., TestMetric]]] = None, reduce: bool = True):
    """bm/play.py:88-175 for a regression model: ``recordings`` holds one iterable of ``SegmentBatch`` per recording;
    every batch runs through ``solver._process_batch`` under ``no_grad``, the first ``trim_offset`` samples are left
    out, and each recording gets its own set of metrics.  The mask is the batch's ``features_mask`` when the Solver has
    ``mask_loss``, otherwise all true (the reference's ``_process_batch`` hands ``torch.ones_like(features_mask)`` on
    unless ``task.mask_loss``, bm/solver.py:251-253).  Returns {name: reduced value} (``reduce``) or {name: stacked
    per-recording results}.  ``metrics`` defaults to ``regression_metric_constructors("feature")``.  With several ranks,
    rank r evaluates recordings r, r + world, ... (the reference shuffles the order first) and the results are
    exchanged."""
    if metrics is None:
        metrics = regression_metric_constructors("feature")
    world, rank = distrib.world_size(), distrib.rank()
    test_metrics: tp.Dict[str, tp.List[torch.Tensor]] = {ctor().name: [] for ctor in metrics}
    for model in solver._all_models():
        model.train(False)
    for recording in list(recordings)[rank::world]:
        current = [ctor() for ctor in metrics]
        for batch in recording:
            with torch.no_grad():
                estimate, gt, features_mask, _ = solver._process_batch(batch)
            if estimate is None:
                continue
            update_all(current, estimate, gt, features_mask if solver.mask_loss else None, trim_offset)
        for metric in current:
            test_metrics[metric.name].append(metric.get().cpu().float())
    solver.check_pending_flags()
    n = len(recordings)
    if world > 1:
        all_results = _exchange(test_metrics, n)
    else:
        all_results = merge_rank_results([test_metrics], n)
    out = {}
    for ctor in metrics:
        metric = ctor()
        if reduce:
            out[metric.name] = metric.reduce(all_results[metric.name])
        else:
            out[metric.name] = torch.stack(all_results[metric.name])
    return out
