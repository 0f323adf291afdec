"""Host-side mirror of ``bm/norm.py``: ``BatchScaler.transform`` + ``ScaleReject`` -- the step immediately in front of
the model in ``Solver._process_batch`` (bm/solver.py:245-246), fused into one HIP streaming kernel per tensor -- and
the fit that has to come before it.

``DeviceBatchScaler.fit`` fits the scalers on the GPU (``BatchScaler.__init__`` + ``fit``, bm/norm.py:152-237): the
robust MEG scalers from three exact order statistics per channel (one radix-select call per recording, one read-back
of a [C, 3] tensor where the reference sorts every channel and calls ``.item()`` three times), the feature scalers
from masked fp64 moments, the category counts from an LDS histogram.  ``DeviceBatchScaler.from_reference`` still
converts a fitted reference ``BatchScaler`` (its ``center_`` / ``scale_`` tensors) into device tables.
"""
import dataclasses
import random
import typing as tp

import torch

from . import hip_ops as H


QUANTILES = (0.25, 0.5, 0.75)      # RobustScaler's lowq, median, highq (bm/norm.py:52, 70)


def select_fit_batches(loaders, n_samples_per_recording: int = 200, n_samples_features: tp.Optional[int] = None):
    """Which batches ``BatchScaler.fit`` uses (bm/norm.py:175-217), as ``(meg, features, batches)``:

    - ``meg``: {recording index: [(loader, batch), ...]} -- per loader, whole batches until ``n_samples_per_recording``
      segments have been seen;
    - ``features``: [(loader, batch), ...] -- the same batches in the order taken or, with ``n_samples_features``,
      shuffled by ``random.Random(1234)`` and cut behind the batch that reaches that budget;
    - ``batches``: {(loader, batch): the batch object}.

    Only ``len(batch.meg)`` and ``batch.recording_index`` are read.  All segments of a loader share one recording
    index (the reference's assert), and no recording is fitted twice: the reference holds one loader per recording
    and asserts that a recording has no scaler yet, so a second loader of a recording is refused here."""
    meg: tp.Dict[int, tp.List[tp.Tuple[int, int]]] = {}
    taken: tp.List[tp.Tuple[int, int]] = []
    batches = {}
    for li, loader in enumerate(loaders):
        remaining = n_samples_per_recording
        first = None
        for bi, batch in enumerate(loader):
            remaining -= len(batch.meg)
            recording_index = int(batch.recording_index[0].item())
            assert bool((batch.recording_index == recording_index).all())
            if first is None:
                assert recording_index not in meg, f"recording {recording_index} is fitted twice"
                first = recording_index
            meg.setdefault(recording_index, []).append((li, bi))
            taken.append((li, bi))
            batches[(li, bi)] = batch
            if remaining <= 0:
                break
    features = taken
    if n_samples_features is not None:
        rand_indexes = list(range(len(taken)))
        random.Random(1234).shuffle(rand_indexes)
        features = [taken[idx] for idx in rand_indexes]
        remaining = n_samples_features
        for idx, key in enumerate(features):
            remaining -= len(batches[key].features)
            if remaining <= 0:
                features = features[:idx + 1]
                break
    return meg, features, batches


def _require_device_batch(batch):
    for name in ("meg", "features", "features_mask", "recording_index"):
        t = getattr(batch, name)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise H.BmHipError(f"DeviceBatchScaler: batch.{name} must be a GPU tensor; fitting and scaling have no "
                               "CPU fallback")


class DeviceBatchScaler:
    """Per-recording robust-scaler tables [R, C] for the MEG and (centre, scale) vectors [F] for
    the features, resident on the GPU."""

    def __init__(self, meg_center: torch.Tensor, meg_scale: torch.Tensor,
                 feature_center: tp.Optional[torch.Tensor] = None,
                 feature_scale: tp.Optional[torch.Tensor] = None, device="cuda"):
        self.meg_center = meg_center.to(device, torch.float32).contiguous()
        self.meg_scale = meg_scale.to(device, torch.float32).contiguous()
        self.feature_center = None if feature_center is None else \
            feature_center.to(device, torch.float32).contiguous()
        self.feature_scale = None if feature_scale is None else \
            feature_scale.to(device, torch.float32).contiguous()

    @classmethod
    def from_reference(cls, batch_scaler, n_channels: int, device="cuda"):
        """``batch_scaler``: a fitted reference ``bm.norm.BatchScaler`` (bm/norm.py:145-237)."""
        n_rec = max(batch_scaler.meg_scalers) + 1
        center = torch.zeros(n_rec, n_channels)
        scale = torch.ones(n_rec, n_channels)
        for idx, sc in batch_scaler.meg_scalers.items():
            center[idx, :len(sc.center_)] = sc.center_
            scale[idx, :len(sc.scale_)] = sc.scale_
        fdim = batch_scaler.features_builder.dimension
        fcenter, fscale = torch.zeros(fdim), torch.ones(fdim)
        for name, fs in batch_scaler.feature_scalers.items():
            if hasattr(fs, "center_"):
                sl = batch_scaler.features_builder.get_slice(name)
                fcenter[sl] = fs.center_
                fscale[sl] = fs.scale_
        return cls(center, scale, fcenter, fscale, device)

    def transform(self, batch):
        """BatchScaler.transform (bm/norm.py:239-275) on a device batch; returns a new batch."""
        meg, _ = H.center_scale(batch.meg.contiguous(), self.meg_center, self.meg_scale,
                                group=batch.recording_index.contiguous())
        features = batch.features
        if self.feature_center is not None:
            features, _ = H.center_scale(features.contiguous(), self.feature_center[None],
                                         self.feature_scale[None])
        return dataclasses.replace(batch, meg=meg, features=features)

    # What `fit` (or `load_state_dict`) knows beyond the tables; never mutated in place.
    feature_slices: tp.Mapping[str, tp.Tuple[int, int]] = {}      # name -> [f0, f1) of every feature
    feature_kinds: tp.Mapping[str, str] = {}                      # name -> "standard" | "category" | "noop"
    categories_count: tp.Mapping[str, torch.Tensor] = {}          # name -> fp32 counts [cardinality], on the host

    @classmethod
    def fit(cls, loaders, features_builder=None, n_samples_per_recording=200, per_channel=False,
            n_samples_features=None, device="cuda"):
        """``BatchScaler(features_builder, ...).fit(loaders)`` (bm/norm.py:152-237) on the GPU.  ``loaders``: one
        iterable of device batches per recording; ``features_builder`` (``None``: MEG only): ``.items()``,
        ``.get_slice(name)``, ``.dimension``; every feature ``.normalizable``, ``.categorical``, ``.cardinality``."""
        meg_keys, feature_keys, batches = select_fit_batches(_checked_loaders(loaders), n_samples_per_recording,
                                                             n_samples_features)
        # MEG: one select per recording, all enqueued before the first read-back
        selected = {}
        for recording_index, keys in meg_keys.items():
            meg = torch.cat([batches[k].meg for k in keys]).to(device, torch.float32).contiguous()
            n = meg.shape[0] * meg.shape[2]
            selected[recording_index] = H.quantile_select(meg, [int(q * n) for q in QUANTILES])
        n_channels = max(q.shape[0] for q in selected.values())
        center = torch.zeros(max(selected) + 1, n_channels)
        scale = torch.ones(max(selected) + 1, n_channels)
        for recording_index, quantiles in selected.items():
            low, med, high = quantiles.cpu().unbind(1)                  # ONE read-back per recording
            width = (high.double() - low.double()).float()              # python floats in the reference: a double difference
            width[width == 0] = 1                                       # padded channels (bm/norm.py:74-77)
            center[recording_index, :len(med)] = med
            scale[recording_index, :len(width)] = width
        if features_builder is None:
            return cls(center, scale, None, None, device)
        # features
        features = torch.cat([batches[k].features for k in feature_keys]).to(device, torch.float32).contiguous()
        mask = torch.cat([batches[k].features_mask for k in feature_keys]).to(device, torch.bool).contiguous()
        if features.shape[1] != features_builder.dimension:
            raise ValueError(f"Invalid channel dim {features.shape[1]} for features, "
                             f"expected {features_builder.dimension}")
        fcenter, fscale = torch.zeros(features_builder.dimension), torch.ones(features_builder.dimension)
        slices, kinds, pending = {}, {}, []
        for name, feature in features_builder.items():
            sl = features_builder.get_slice(name)
            f0, f1, _ = sl.indices(features.shape[1])
            slices[name] = (f0, f1)
            if feature.normalizable:
                kinds[name] = "standard"
                pending.append((name,) + H.masked_moments(features, mask, f0, f1, per_channel)[1:])
            elif feature.categorical:
                kinds[name] = "category"
                assert f1 - f0 == 1, f"categorical feature {name} must be one channel wide"
                pending.append((name,) + H.category_counts(features, mask, f0, feature.cardinality))
            else:
                kinds[name] = "noop"
        counts = {}
        for name, first, second in pending:                              # read back after everything is enqueued
            f0, f1 = slices[name]
            if kinds[name] == "standard":
                mean, std = first.cpu(), second.cpu()
                assert (std > 0).all(), \
                    f"Annotation embedding {name} could not be normalized as the " \
                    "values were all the same. Are there relevant event annotations" \
                    " to be embedded?"
                fcenter[f0:f1] = mean
                fscale[f0:f1] = std
            else:
                flags = int(second.cpu().item())
                assert flags == 0, f"categorical feature {name}: values must be the integers 0 .. cardinality - 1 " \
                    f"with minimum 0 (not an integer: {bool(flags & H.CATEGORY_NOT_INTEGER)}, max too large: " \
                    f"{bool(flags & H.CATEGORY_MAX)}, min != 0: {bool(flags & H.CATEGORY_MIN)})"
                counts[name] = first.cpu()
        scaler = cls(center, scale, fcenter, fscale, device)
        scaler.feature_slices, scaler.feature_kinds, scaler.categories_count = slices, kinds, counts
        return scaler

    def inverse_transform(self, batch):
        """BatchScaler.inverse_transform (bm/norm.py:280-281) on a device batch; returns a new batch."""
        _require_device_batch(batch)
        meg = H.center_scale_inverse(batch.meg.contiguous(), self.meg_center, self.meg_scale,
                                     group=batch.recording_index.contiguous())
        features = batch.features
        if self.feature_center is not None:
            features = H.center_scale_inverse(features.contiguous(), self.feature_center[None],
                                              self.feature_scale[None])
        return dataclasses.replace(batch, meg=meg, features=features)

    def inverse_transform_feature(self, feature_name, feature_data):
        """Inverse transform of one feature [B, F_name, T] (bm/norm.py:283-289)."""
        f0, f1 = self.feature_slices[feature_name]
        if self.feature_kinds[feature_name] != "standard":
            return feature_data
        if not feature_data.is_cuda:
            raise H.BmHipError("inverse_transform_feature: expected a GPU tensor; there is no CPU fallback")
        return H.center_scale_inverse(feature_data.contiguous(), self.feature_center[None, f0:f1].contiguous(),
                                      self.feature_scale[None, f0:f1].contiguous())

    def get_categorical_feature_weights(self, feature_name) -> torch.Tensor:
        """Weights inversely proportional to the square root of every category's frequency, E[weights] = 1
        (bm/norm.py:291-308): the reference's expression on the host, on the fp32 count vector."""
        assert self.feature_kinds[feature_name] == "category"
        count = self.categories_count[feature_name]
        probs = count / count.sum()
        weights = 1 / torch.sqrt(probs)
        weights[probs == 0] = 0.
        weights /= torch.sqrt(probs).sum()
        return weights

    def state_dict(self):
        """Tables, counts and names as CPU tensors / plain containers (what the reference's scaler cache holds)."""
        def host(t):
            return None if t is None else t.detach().cpu().clone()
        return {"meg_center": host(self.meg_center), "meg_scale": host(self.meg_scale),
                "feature_center": host(self.feature_center), "feature_scale": host(self.feature_scale),
                "feature_names": list(self.feature_slices),
                "feature_slices": {k: tuple(v) for k, v in self.feature_slices.items()},
                "feature_kinds": dict(self.feature_kinds),
                "categories_count": {k: host(v) for k, v in self.categories_count.items()}}

    def load_state_dict(self, state):
        device = self.meg_center.device

        def dev(t):
            return None if t is None else t.to(device, torch.float32).contiguous()
        self.meg_center, self.meg_scale = dev(state["meg_center"]), dev(state["meg_scale"])
        self.feature_center, self.feature_scale = dev(state["feature_center"]), dev(state["feature_scale"])
        self.feature_slices = {k: tuple(state["feature_slices"][k]) for k in state["feature_names"]}
        self.feature_kinds = dict(state["feature_kinds"])
        self.categories_count = {k: v.detach().cpu().clone() for k, v in state["categories_count"].items()}
        return self


def _checked_loaders(loaders):
    """The loaders' batches, each refused unless it lives on the GPU."""
    def checked(loader):
        for batch in loader:
            _require_device_batch(batch)
            yield batch
    return [checked(loader) for loader in loaders]


def _subset(batch, keep: torch.Tensor):
    """``batch[keep]`` with the reference's semantics (bm/dataset.py:242-257): tensor fields are
    indexed, list fields (``_recordings``, ``_event_lists``) keep the selected items, empty lists stay
    empty.  Uses the batch's own ``__getitem__`` when it has one (the reference's SegmentBatch)."""
    if hasattr(type(batch), "__getitem__"):
        return batch[keep]
    idx = keep.nonzero().flatten()
    picked = idx.tolist()
    kw = {}
    for field in dataclasses.fields(batch):
        data = getattr(batch, field.name)
        if isinstance(data, list):
            kw[field.name] = [data[i] for i in picked] if data else []
        elif isinstance(data, torch.Tensor):
            kw[field.name] = data[idx]
        else:
            kw[field.name] = data
    return dataclasses.replace(batch, **kw)


class ScaleReject:
    """bm/norm.py:311-345.  Rescales MEG and features; rejects items whose scaled MEG still exceeds
    ``limit`` (or, with ``clip``, clamps instead).  With ``clip=True`` (conf/config.yaml:131) no
    amplitude rejection can occur, so the step runs without any host synchronisation; otherwise
    one small read-back of the per-segment maxima decides the (rare) compaction."""

    def __init__(self, scaler: DeviceBatchScaler, limit=16, exclude_empty_features=False, clip=False):
        self.scaler = scaler
        self.limit = limit
        self.clip = clip
        self.exclude_empty_features = exclude_empty_features
        self._rejection_count = 0
        self._count = 0

    def __call__(self, batch) -> tp.Tuple[tp.Any, torch.Tensor]:
        sc = self.scaler
        meg, maxabs = H.center_scale(batch.meg.contiguous(), sc.meg_center, sc.meg_scale,
                                     group=batch.recording_index.contiguous(), clip=self.clip,
                                     limit=float(self.limit), want_maxabs=not self.clip)
        features = batch.features
        if sc.feature_center is not None:
            features, _ = H.center_scale(features.contiguous(), sc.feature_center[None],
                                         sc.feature_scale[None])
        self._count += len(meg)
        keep = torch.ones(len(meg), dtype=torch.bool, device=meg.device)
        if maxabs is not None:
            keep &= ~(maxabs > self.limit)
        if self.exclude_empty_features:
            keep &= batch.features_mask.view(len(meg), -1).sum(-1) != 0
        batch = dataclasses.replace(batch, meg=meg, features=features)
        if maxabs is None and not self.exclude_empty_features:
            return batch, keep                       # nothing can be rejected: no sync
        n_reject = int((~keep).sum().item())
        self._rejection_count += n_reject
        if n_reject == 0:
            return batch, keep
        return _subset(batch, keep), keep

    @property
    def rejection_rate(self):
        return self._rejection_count / max(self._count, 1)
