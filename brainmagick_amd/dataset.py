"""Segments out of recordings that stay resident on the GPU: the data loader of bm/dataset.py without the per-item loop.

The reference cuts one window per ``SegmentDataset.__getitem__`` on the CPU (``mne.Epochs``: float64 baseline
correction, ``.float()``), stacks the items in ``SegmentBatch.collate_fn`` and copies the batch to the card.  A
preprocessed recording is small (273 channels x 1 h at 120 Hz: 470 MB in fp32), so here the recordings live on the device
and a batch is ONE gather launch per tensor (``hip_ops.segment_gather``, csrc/segments.hip) over the ``(recording, first
sample)`` arrays of the epoch, which are uploaded once per epoch.

- ``event_samples`` / ``segment_starts``: the window selection of ``_DatasetFactory.apply`` (bm/dataset.py:113-158), pure
  numpy.  Held to the live reference by tests/golden/segments.json.
- ``window_samples``: the window length and the baseline window of ``mne.Epochs(tmin, tmax, baseline)``, restated from
  mne's documentation (mne itself cannot be run against this).
- ``DeviceRecording``, ``DeviceSegments``, ``DeviceSegmentLoader``: the dataset and its loader; torch's own samplers
  decide the order, the loader only replaces what they index.
- ``preprocess_meg`` / ``DeviceRecording.from_raw``: the resampling and the ``highpass`` of ``preprocess_mne``
  (bm/studies/api.py:334-363) over the raw recording, one launch each (csrc/resample.hip, csrc/fir.hip).

The features of a batch come either from full-length arrays (two more gathers) or from the recording's events
(``DeviceRecording(meg, events=features.DeviceEvents(...))``): then ONE ``hip_ops.segment_features`` launch builds the
features and the mask of the batch by the reference's per-window rules (features.py, csrc/features.hip).

Not built: WordPulse / PhonemePulse (``post_process``), Wav2VecChunk, computing the
wav2vec2 states / embeddings themselves (the mel spectrogram and the pitch: ``audio.py``), ``autoreject``,
``split_wav_as_block``, ``decim != 1``, channel picking, reading ``.fif`` files, ``mne.Info`` and layouts.  There is no CPU
fallback.
"""
import copy
import typing as tp

import numpy as np
import torch

from . import hip_ops as H
from ._lib import BmHipError
from .synthetic import SegmentBatch

Blocks = tp.Optional[tp.Sequence[tp.Tuple[float, float]]]


def _to_ind(seconds, sample_rate: float):
    """``Frequency.to_ind`` (bm/utils.py:39-45): ``np.round(seconds * sample_rate).astype(int)``, half to even."""
    if isinstance(seconds, np.ndarray):
        return np.round(seconds * sample_rate).astype(int)
    return int(round(seconds * sample_rate))


def event_samples(n_samples: int, sample_rate: float, tmin: float, tmax: float, condition, blocks: Blocks = None,
                  ignore_start_in_block: bool = False, ignore_end_in_block: bool = False) -> np.ndarray:
    """``samples`` of ``_DatasetFactory.apply`` (bm/dataset.py:113-158): the event sample of every window the reference
    keeps, in the order of the events, repeated samples included.  ``condition``: a float (an event every ``condition``
    seconds) or an array of event times in seconds.  The recording's time axis is ``np.arange(n_samples) /
    sample_rate``.  Empty where the reference logs "Empty dataset"."""
    if blocks is not None and not len(blocks):
        raise ValueError("No blocks provided.")
    sample_rate = float(sample_rate)
    last_time = (n_samples - 1) / sample_rate if n_samples > 0 else -1.0
    if isinstance(condition, float):
        times = np.arange(0, last_time, condition)
    elif isinstance(condition, (np.ndarray, list, tuple)):
        times = np.asarray(condition, dtype=np.float64)
    else:
        raise TypeError("Condition should be a float corresponding to a duration in seconds, or an array of event "
                        f"times, got:\n{condition} (type: {type(condition)})")
    delta = 0.5 / sample_rate
    mask = np.logical_and(times + tmin >= 0, times + tmax < last_time + delta)
    if blocks is not None:
        # only the extracts that are fully contained in at least one of the given blocks
        in_any_split = np.zeros(len(times), dtype=bool)
        for start, stop in blocks:
            in_split = times >= start if ignore_start_in_block else times + tmin >= start
            margin = delta if ignore_end_in_block else tmax - delta
            in_split = in_split & (times + margin < stop)
            in_any_split |= in_split
        mask &= in_any_split
    if not mask.any():
        return np.zeros(0, dtype=np.int64)
    return _to_ind(times[mask], sample_rate).astype(np.int64)


def segment_starts(n_samples: int, sample_rate: float, tmin: float, tmax: float, condition, blocks: Blocks = None,
                   ignore_start_in_block: bool = False, ignore_end_in_block: bool = False) -> np.ndarray:
    """The first raw sample of every window: ``event_samples`` with repeated event samples dropped, keeping the first
    (mne's ``event_repeated='drop'``, as documented by mne), plus ``round(tmin * sample_rate)``."""
    samples = event_samples(n_samples, sample_rate, tmin, tmax, condition, blocks, ignore_start_in_block,
                            ignore_end_in_block)
    _, first = np.unique(samples, return_index=True)
    return samples[np.sort(first)] + _to_ind(tmin, float(sample_rate))


def window_samples(sample_rate: float, tmin: float, tmax: float, baseline=(None, 0)):
    """``(T, baseline window)`` of ``mne.Epochs(tmin=, tmax=, baseline=)``: the window is the raw samples
    ``start ... start + T - 1`` with ``T = round(tmax sr) - round(tmin sr) + 1`` (inclusive at both ends);
    ``baseline=None``: no correction (``None``), else ``(a, b)`` in seconds, inclusive, ``None`` standing for
    ``tmin`` / ``tmax``: window samples ``round(a sr) - round(tmin sr) ... round(b sr) - round(tmin sr)``."""
    sample_rate = float(sample_rate)
    if not tmin < tmax:
        raise ValueError(f"tmin = {tmin} is not below tmax = {tmax}")
    first = _to_ind(tmin, sample_rate)
    T = _to_ind(tmax, sample_rate) - first + 1
    if baseline is None:
        return T, None
    a, b = baseline
    b0 = _to_ind(tmin if a is None else a, sample_rate) - first
    b1 = _to_ind(tmax if b is None else b, sample_rate) - first
    if b0 < 0 or b1 >= T or b0 > b1:
        raise ValueError(f"baseline {baseline} is outside the window [{tmin}, {tmax}] (samples {b0}..{b1} of {T})")
    return T, (b0, b1)


# One flag word per device, owned by this module (NOT the Solver's index_error_flag): raised by the gather kernel when a
# segment is out of range, read once per epoch by the loader.
range_error_flag = H.DeviceFlag()


def raise_if_range_error(device) -> None:
    """Synchronising check of the flag, which it clears."""
    if range_error_flag.take(device):
        raise IndexError("a segment's recording or first sample is out of range (such segments were gathered as zeros)")


def preprocess_meg(raw, sfreq: float, sample_rate, highpass: float = 0.) -> torch.Tensor:
    """``preprocess_mne(raw, sample_rate, highpass).get_data()`` (bm/studies/api.py:334-363) under the rate rules of
    ``Recording.preprocessed`` (bm/studies/api.py:208-216), on the device: ``raw`` [C, L] (the raw recording's
    ``get_data()`` at ``sfreq`` Hz; a tensor or an array, moved to the GPU as fp32) -> [C, floor(new L / old)] fp32.
    ``old_sr = int(np.round(sfreq))``; julius' ``ResampleFrac(old_sr, sample_rate)`` over the channels (ONE launch,
    ``hip_ops.resample_rows``), then, with ``highpass``, ``data -= lowpass_filter(data, highpass / sample_rate)`` (ONE
    launch, ``hip_ops.highpass_filter``; ``zeros = 8``, a Python float division as in the reference: ``int()`` of it
    decides the filter's length).  ``sample_rate == old_sr`` without ``highpass`` hands the tensor through untouched
    and launches nothing (the reference's ``(0, 0.0)`` key: the raw recording itself).  julius is restated, see
    ``hip_ops.resample_taps`` / ``lowpass_taps``; reading the file, ``mne.Info`` and layouts are not built."""
    if sample_rate != int(sample_rate):
        raise ValueError("For simplicity's sake, only integer sampling rates in Hz are allowed")
    sample_rate = int(sample_rate)
    old_sr = int(np.round(sfreq))
    if sample_rate > old_sr:
        raise ValueError(f"The sample rate should be below {old_sr}Hz, got {sample_rate}")
    if highpass:
        H._check_cutoff(highpass / sample_rate)                    # julius' errors, before anything is uploaded
    data = torch.as_tensor(raw)
    if data.dim() != 2:
        raise ValueError(f"expected [channels, samples], got {tuple(data.shape)}")
    if not (data.is_cuda and data.dtype == torch.float32):
        if not torch.cuda.is_available():
            raise BmHipError("preprocess_meg: no GPU; the brainmagick_amd hot path has no CPU fallback")
        data = data.to(device="cuda", dtype=torch.float32)
    data = H.resample_rows(data, old_sr, sample_rate)
    if highpass:
        data = H.highpass_filter(data, highpass / sample_rate)
    return data


class DeviceRecording:
    """One preprocessed recording on the device. ``meg``: [C_r, N] fp32, ``features``: [F, N] fp32, ``features_mask``:
    [M, N] bool; a tensor that is already there is adopted without a copy.  ``events`` (``features.DeviceEvents``)
    instead of ``features`` / ``features_mask``: the features and the mask of a batch are built from the events by
    ``hip_ops.segment_features``.  ``recording``: anything with ``recording_index`` and ``layout``
    (``synthetic.Recording``)."""

    def __init__(self, meg, features=None, features_mask=None, *, recording, subject_index: int, device=None,
                 events=None):
        self.recording = recording
        self.subject_index = int(subject_index)
        self.recording_index = int(recording.recording_index)
        if events is not None and (features is not None or features_mask is not None):
            raise ValueError("a recording carries either its events (the features are built per batch) or full-length "
                             "features / features_mask arrays, not both")
        if device is None:
            device = meg.device if isinstance(meg, torch.Tensor) and meg.is_cuda else \
                torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.meg = self._adopt(meg, torch.float32, device)
        self.events = events                                        # features.DeviceEvents, or None
        if events is not None and events.device.type != self.meg.device.type:
            raise ValueError(f"the events are on {events.device}, the MEG on {self.meg.device}")
        self.features = None if features is None else self._adopt(features, torch.float32, device)
        self.features_mask = None if features_mask is None else self._adopt(features_mask, torch.bool, device)
        for name in ("features", "features_mask"):
            t = getattr(self, name)
            if t is not None and t.shape[1] != self.n_samples:
                raise ValueError(f"{name} has {t.shape[1]} samples, the MEG has {self.n_samples}")

    @classmethod
    def from_raw(cls, raw, sfreq: float, sample_rate, highpass: float = 0., **kw) -> "DeviceRecording":
        """The recording from its RAW MEG ``[C, L]`` at ``sfreq`` Hz: ``preprocess_meg`` on the device, then the
        constructor with ``kw`` as it is (features and events are at ``sample_rate``)."""
        return cls(preprocess_meg(raw, sfreq, sample_rate, highpass), **kw)

    @staticmethod
    def _adopt(t, dtype, device) -> torch.Tensor:
        t = torch.as_tensor(t)
        if t.dim() != 2:
            raise ValueError(f"expected [channels, samples], got {tuple(t.shape)}")
        return t.to(device=device, dtype=dtype).contiguous()        # the same tensor when nothing has to change

    @property
    def n_samples(self) -> int:
        return self.meg.shape[1]

    @property
    def n_channels(self) -> int:
        return self.meg.shape[0]


def _blocks_of(blocks, i: int, n: int):
    """``blocks``: None, one list of (start, stop) for every recording, or {position of a recording: its list}."""
    if isinstance(blocks, dict):
        if set(blocks) != set(range(n)):
            raise ValueError(f"blocks for the recordings {sorted(blocks)}, there are {n}")
        return blocks[i]
    return blocks


class DeviceSegments:
    """The segments of ``recordings`` in ``ConcatDataset`` order (bm/dataset.py:541), selected like
    ``_DatasetFactory.apply`` and cut like ``mne.Epochs``.  ``rec[i]`` / ``start[i]`` (int32, host): the recording (its
    position in ``recordings``) and the first raw sample of segment ``i``.  A selected window that does not lie inside
    its recording (the reference's mask can keep one that ends one sample past the end) is dropped, as mne drops an
    epoch that is too short."""

    def __init__(self, recordings: tp.Sequence[DeviceRecording], sample_rate: float, tmin: float = -0.5,
                 tmax: float = 2.5, baseline=(None, 0), condition=3.0, blocks=None,
                 meg_dimension: tp.Optional[int] = None, ignore_start_in_block: bool = False,
                 ignore_end_in_block: bool = False):
        if not recordings:
            raise ValueError("no recording")
        self.recordings = list(recordings)
        self.sample_rate, self.tmin, self.tmax = float(sample_rate), tmin, tmax
        self.T, self.baseline = window_samples(sample_rate, tmin, tmax, baseline)
        if meg_dimension is None:
            meg_dimension = max(r.n_channels for r in self.recordings)
        for r in self.recordings:
            assert meg_dimension >= r.n_channels                               # bm/dataset.py:321
        self.meg_dimension = meg_dimension
        first = self.recordings[0]
        with_events = [r.events is not None for r in self.recordings]
        if any(with_events) and not all(with_events):
            raise ValueError("some recordings carry events and others full-length arrays: "
                             f"{['events' if e else 'arrays' for e in with_events]}")
        self.builder = first.events.builder if with_events[0] else None
        if self.builder is not None:
            if any(r.events.builder is not self.builder for r in self.recordings):
                raise ValueError("the recordings' events were made for different features builders")
            if self.builder.sample_rate != self.sample_rate:
                raise ValueError(f"the features builder samples at {self.builder.sample_rate} Hz, the segments at "
                                 f"{self.sample_rate} Hz")
        for name in ("features", "features_mask"):
            shapes = {None if getattr(r, name) is None else getattr(r, name).shape[0] for r in self.recordings}
            if len(shapes) != 1:
                raise ValueError(f"the recordings disagree on {name}: {sorted(map(str, shapes))} rows")
        if self.builder is not None:
            self.n_features, self.n_mask = self.builder.dimension, 1
        else:
            self.n_features = 0 if first.features is None else first.features.shape[0]
            self.n_mask = 0 if first.features_mask is None else first.features_mask.shape[0]
        rec, start = [], []
        for i, r in enumerate(self.recordings):
            s = segment_starts(r.n_samples, sample_rate, tmin, tmax, condition, _blocks_of(blocks, i, len(self.recordings)),
                               ignore_start_in_block, ignore_end_in_block)
            # Every window is validated here, so the kernel's range flag never fires in normal use.  The reference's edge
            # mask compares times, not samples: when the event and tmax both round upward (11.5 -> 12 and 7.5 -> 8) it
            # keeps a window whose last sample is one past the end.  mne drops such an epoch as too short; so does this.
            s = s[(s >= 0) & (s + self.T <= r.n_samples)]
            rec.append(np.full(len(s), i, dtype=np.int32))
            start.append(s.astype(np.int32))
        self.rec = np.concatenate(rec)
        self.start = np.concatenate(start)
        self.wstart = self.wdur = None
        if self.builder is not None:
            # The window in seconds, as _get_bounds_times hands it to FeaturesBuilder.__call__ (bm/dataset.py:323-344,
            # bm/features/base.py:77-90): Python's division here, no division on the device.
            s = self.start.astype(np.int64)
            self.wstart = s / self.sample_rate
            self.wdur = (s + self.T) / self.sample_rate - self.wstart
            n_times = np.round(self.wdur * self.sample_rate).astype(np.int64)
            if (n_times != self.T).any():
                i = int(np.flatnonzero(n_times != self.T)[0])
                raise ValueError(f"segment {i} (first sample {s[i]}): the reference would build {n_times[i]} feature "
                                 f"samples for a window of {self.T}")
        self._rec_index = np.array([r.recording_index for r in self.recordings], dtype=np.int64)
        self._subject_index = np.array([r.subject_index for r in self.recordings], dtype=np.int64)
        self._tables = None

    def __len__(self) -> int:
        return len(self.rec)

    @property
    def device(self) -> torch.device:
        return self.recordings[0].meg.device

    def tables(self):
        """(MEG, features, mask) device tables, built at the first batch."""
        if self._tables is None:
            if not self.device.type == "cuda":
                raise BmHipError("DeviceSegments: the recordings are not on a GPU; the segment gather is a HIP kernel "
                                 "and has no CPU fallback")
            if self.builder is not None:
                events = H.EventTable(self.builder.plan(), len(self.builder.kinds), self.builder.mask_kind,
                                      [(r.events.kind_tables, r.events.sources) for r in self.recordings], self.device)
                self._tables = (H.SegmentTable([r.meg for r in self.recordings]), events, None)
            else:
                self._tables = (H.SegmentTable([r.meg for r in self.recordings]),
                                H.SegmentTable([r.features for r in self.recordings]) if self.n_features else None,
                                H.SegmentTable([r.features_mask for r in self.recordings]) if self.n_mask else None)
        return self._tables

    def upload(self, indices) -> tp.Dict[str, torch.Tensor]:
        """The index arrays of ``indices`` (a whole epoch, or one batch) on the device: ONE upload each."""
        self.tables()
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < -len(self) or idx.max() >= len(self)):
            raise IndexError(f"segment index out of range for {len(self)} segments")
        rec = self.rec[idx]
        dev = self.device
        arrays = dict(rec=torch.from_numpy(rec).to(dev), start=torch.from_numpy(self.start[idx]).to(dev),
                      subject_index=torch.from_numpy(self._subject_index[rec]).to(dev),
                      recording_index=torch.from_numpy(self._rec_index[rec]).to(dev),
                      recordings=[self.recordings[int(r)].recording for r in rec])
        if self.builder is not None:
            arrays.update(wstart=torch.from_numpy(self.wstart[idx]).to(dev), wdur=torch.from_numpy(self.wdur[idx]).to(dev))
        return arrays

    def gather(self, arrays: tp.Dict[str, torch.Tensor], first: int, count: int) -> SegmentBatch:
        """Segments ``first ... first + count - 1`` of uploaded index arrays: at most three launches (two with events:
        the MEG gather and the features builder), no copy from the host, no synchronisation."""
        meg_t, feat_t, mask_t = self.tables()
        rec, start = arrays["rec"], arrays["start"]
        flag = range_error_flag(self.device)
        meg = H.segment_gather(meg_t, rec, start, first, count, self.meg_dimension, self.T, flag,
                               baseline=self.baseline)
        if self.builder is not None:                                   # ONE launch builds the features and the mask
            features, mask = H.segment_features(feat_t, rec, arrays["wstart"], arrays["wdur"], first, count, self.T,
                                                self.sample_rate, flag)
            return SegmentBatch(meg, features, mask, arrays["subject_index"][first:first + count],
                                arrays["recording_index"][first:first + count],
                                arrays["recordings"][first:first + count])
        if feat_t is not None:
            features = H.segment_gather(feat_t, rec, start, first, count, self.n_features, self.T, flag)
        else:
            features = torch.empty(count, 0, self.T, device=self.device)
        if mask_t is not None:
            mask = H.segment_gather(mask_t, rec, start, first, count, self.n_mask, self.T, flag)
        else:
            mask = torch.ones(count, 1, self.T, device=self.device, dtype=torch.bool)
        return SegmentBatch(meg, features, mask, arrays["subject_index"][first:first + count],
                            arrays["recording_index"][first:first + count],
                            arrays["recordings"][first:first + count])

    def batch(self, indices) -> SegmentBatch:
        arrays = self.upload(indices)
        return self.gather(arrays, 0, len(arrays["recordings"]))

    def only(self, recording: int) -> "DeviceSegments":
        """The segments of one recording (its position in ``recordings``) over the same resident recordings and the
        same device tables."""
        return self.subset([recording])

    def subset(self, recordings: tp.Iterable[int]) -> "DeviceSegments":
        """The segments of some recordings (their positions in ``recordings``), in this dataset's order, over the same
        resident recordings and the same device tables."""
        if self.device.type == "cuda":
            self.tables()                                   # built once here, shared by every copy
        sub = copy.copy(self)
        keep = np.isin(self.rec, np.asarray(list(recordings), dtype=np.int64))
        sub.rec, sub.start = self.rec[keep], self.start[keep]
        if self.builder is not None:
            sub.wstart, sub.wdur = self.wstart[keep], self.wdur[keep]
        return sub

    def per_recording_loaders(self, batch_size: int, generator=None) -> tp.List["DeviceSegmentLoader"]:
        """One shuffled loader of device batches per recording that has segments: what ``DeviceBatchScaler.fit`` takes
        (the ``loader_factory`` of bm/solver.py:132-141)."""
        return [DeviceSegmentLoader(self.only(i), batch_size, shuffle=True, generator=generator)
                for i in range(len(self.recordings)) if (self.rec == i).any()]


class DeviceSegmentLoader:
    """Iterates device batches of a ``DeviceSegments`` in the order of torch's samplers: ``RandomSampler(range(n),
    generator=generator)`` (``SequentialSampler`` without ``shuffle``) at ``world == 1``, else ``DistributedSampler(
    num_replicas=world, rank=rank, shuffle=, seed=, drop_last=)`` after ``set_epoch``, padding rule included.  The index
    arrays of an epoch are uploaded once when the iteration starts (``epoch_arrays``); a batch is an offset into them.
    The kernel's range flag is read once, after the last batch, and raises ``IndexError``."""

    def __init__(self, segments: DeviceSegments, batch_size: int, shuffle: bool = False, generator=None, seed: int = 0,
                 rank: int = 0, world: int = 1, drop_last: bool = False):
        from torch.utils.data import DistributedSampler, RandomSampler, SequentialSampler
        if batch_size < 1:
            raise ValueError(f"batch_size = {batch_size}")
        self.segments, self.batch_size = segments, batch_size
        index_space = range(len(segments))
        if world > 1:
            self.sampler = DistributedSampler(index_space, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                              drop_last=drop_last)
        elif shuffle:
            self.sampler = RandomSampler(index_space, generator=generator)
        else:
            self.sampler = SequentialSampler(index_space)
        self.epoch_arrays: tp.Optional[tp.Dict[str, torch.Tensor]] = None
        self.order: tp.List[int] = []

    def set_epoch(self, epoch: int) -> None:
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __len__(self) -> int:
        return -(-len(self.sampler) // self.batch_size)

    def indices(self) -> tp.List[int]:
        """Draws the order of one epoch from the sampler."""
        return [int(i) for i in self.sampler]

    def __iter__(self) -> tp.Iterator[SegmentBatch]:
        self.order = self.indices()
        self.epoch_arrays = arrays = self.segments.upload(self.order)
        for first in range(0, len(self.order), self.batch_size):
            yield self.segments.gather(arrays, first, min(self.batch_size, len(self.order) - first))
        raise_if_range_error(self.segments.device)
