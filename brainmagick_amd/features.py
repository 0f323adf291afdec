"""The events-to-features step of the data loader on the device: bm/features/base.py:23-178 (``FeaturesBuilder``) with the
events resident on the card and ONE launch per batch (``hip_ops.segment_features``, csrc/features.hip).

The reference builds the features of every segment on the CPU, event by event: ``FeaturesBuilder.__call__(start, stop)``
paints ``feature.get_on_overlap(event, overlap)`` into the window for every event that overlaps it.  For the two headline
targets the painted values depend on the window (the wav2vec embedding is cut for the overlap and only then interpolated
to the overlap's length; the mel spectrogram is resampled for the whole event and cut at a rounded offset), so they are
not a slice of one full-length array, and full-length arrays at the MEG rate would be 2.4 times the embedding's size at
its own 50 Hz.  Here the events, their value rows and their arrays (at their native rate) stay on the device and the
kernel applies the reference's index arithmetic per window.

Three rules, named for what they do, cover the reference's features:

- ``constant``: ``Feature.get`` returns a number or a 1-D tensor -- one value row per event (WordLength, WordIndex,
  WordFrequency, WordSegment, Modality, Phoneme, WordHash, WordEmbedding ...).  The caller supplies the values as float64
  (``wordfreq``, ``spacy`` and Python's salted ``hash`` stay with the caller); they are rounded once to fp32.
- ``resampled``: one array ``[D, L]`` per event; ``get`` = nearest ``F.interpolate`` to the event's own length, then the
  default ``get_on_overlap`` (MelSpectrum, Pitch; bm/features/audio.py:78-83, base.py:238-267).
- ``chunk``: one array ``[D, L]`` per event; ``_get_cached_tensor`` + ``get_on_overlap`` of bm/features/audio.py:211-274
  (Wav2VecTransformer, Wav2VecConvolution).

The batch's ``_event_lists`` have one reader in the reference, ``_get_extra_info`` of scripts/run_eval_probs.py:27-57 (the
word index and the sentence of the word at ``check_at_time``).  What it reads travels with the word events as two
optional integer columns, ``word_index`` and ``sequence_id`` (``DeviceEvents``), and ``hip_ops.segment_eval_labels`` looks
the word up in the resident tables (``retrieval.segment_eval_epoch``); no list of events is built per batch.

Not built: WordPulse and PhonemePulse (``post_process``), Wav2VecChunk, and computing the
wav2vec2 hidden states / the word embeddings themselves (the mel spectrogram's and the pitch's arrays come from
``audio.DeviceMelSpectrum.compute`` and ``audio.DevicePitch.compute``, resampled to 16 kHz on the device when asked).
There is no CPU fallback.
"""
import collections
import typing as tp

import numpy as np
import torch

RULES = ("constant", "resampled", "chunk")
WORD_KIND = "word"
WORD_INFO_COLUMNS = ("word_index", "sequence_id")              # optional integer columns of the word events


class EventFeature:
    """What ``FeatureDecodingLoss``, ``metrics.metric_constructors`` and ``DeviceBatchScaler.fit`` read of a reference
    ``Feature`` (bm/features/base.py:181-229), plus the ``rule`` that paints it."""

    def __init__(self, name: str, rule: str, event_kind: str, dimension: int = 1, cardinality: tp.Optional[int] = None,
                 default_value: float = 0., normalizable: tp.Optional[bool] = None):
        if rule not in RULES:
            raise ValueError(f"feature {name}: rule {rule!r} is not one of {RULES}")
        if not event_kind:
            raise ValueError(f"feature {name}: missing event_kind")
        if dimension < 1:
            raise ValueError(f"feature {name}: dimension {dimension}")
        if cardinality is not None and (dimension != 1 or rule != "constant"):    # base.py:220-222
            raise ValueError(f"feature {name}: a categorical feature is one constant channel")
        self.name, self.rule, self.event_kind = name, rule, event_kind
        self.dimension, self.cardinality, self.default_value = int(dimension), cardinality, float(default_value)
        self._normalizable = normalizable

    @property
    def output_dimension(self) -> int:
        return self.cardinality if self.categorical else self.dimension

    @property
    def categorical(self) -> bool:
        return self.cardinality is not None

    @property
    def normalizable(self) -> bool:
        return not self.categorical if self._normalizable is None else self._normalizable

    def __repr__(self) -> str:
        return f"{self.name}({self.rule}, {self.event_kind}, {self.dimension})"


class DeviceFeaturesBuilder(collections.OrderedDict):
    """name -> feature in channel order, with the reference's ``get_slice``, ``dimension`` and ``output_dimension``
    (bm/features/base.py:124-173).  ``event_mask``: the batch's mask is true exactly where a ``word`` event paints
    (WordSegment, base.py:109-114), else all true."""
    MASK_KIND = "word"
    MAX_FEATURES = 32                                          # FT_MAXF of csrc/features.hip

    def __init__(self, features: tp.Sequence[EventFeature], sample_rate: float, event_mask: bool = False):
        super().__init__()
        for feature in features:
            if feature.name in self:
                raise ValueError(f"feature {feature.name} given twice")
            self[feature.name] = feature
        self.sample_rate, self.event_mask = float(sample_rate), bool(event_mask)
        if not self.sample_rate > 0:
            raise ValueError(f"sample_rate = {sample_rate}")
        self.kinds: tp.List[str] = []                          # event kinds in the order of their first feature
        for feature in self.values():
            if feature.event_kind not in self.kinds:
                self.kinds.append(feature.event_kind)
        if self.event_mask and self.MASK_KIND not in self.kinds:
            self.kinds.append(self.MASK_KIND)                  # the word table is needed without any word feature
        if len(self) > self.MAX_FEATURES:
            raise ValueError(f"{len(self)} features; the kernel's plan holds {self.MAX_FEATURES}")
        # the builder is fixed from here on: (channels in the features, channels in the model's output) per feature
        self._slices: tp.Dict[str, tp.Tuple[slice, slice]] = {}
        at, at_out = 0, 0
        for feature in self.values():
            self._slices[feature.name] = (slice(at, at + feature.dimension), slice(at_out, at_out + feature.output_dimension))
            at, at_out = at + feature.dimension, at_out + feature.output_dimension
        self._widths = (at, at_out)

    def get_slice(self, name: str, model_output: bool = False) -> slice:
        """The channels of feature ``name`` in the features tensor, or -- ``model_output`` -- in the model's output, where
        a categorical feature takes one channel per class."""
        try:
            return self._slices[name][1 if model_output else 0]
        except KeyError:
            raise KeyError(f"no feature {name!r} among {list(self)}") from None

    def extract_features(self, features: torch.Tensor, feature_names: tp.Sequence[str]) -> torch.Tensor:
        """bm/features/base.py:145-160: the channels of ``feature_names``, in that order, out of a tensor ``[B,
        dimension, T]`` that holds all of the builder's features.  Names that are the builder's first features in the
        builder's order (the used features in front of the extra test features, bm/wer.py:49-50) are ONE leading run of
        channels: a view, made contiguous once; anything else is one ``torch.cat`` of the slices, as the reference
        writes it.  The result never shares memory with ``features`` unless it is all of it."""
        assert features.shape[1] == self.dimension, "Input should contain all features"
        feature_names = list(feature_names)
        assert all([name in self for name in feature_names])
        slices = [self.get_slice(name) for name in feature_names]
        at = 0
        for s in slices:
            if s.start != at:
                break
            at = s.stop
        else:
            if slices:
                return features[:, :at].contiguous()
        return torch.cat([features[:, s] for s in slices], dim=1)

    @property
    def dimension(self) -> int:
        return self._widths[0]

    @property
    def output_dimension(self) -> int:
        return self._widths[1]

    @property
    def mask_kind(self) -> int:
        return self.kinds.index(self.MASK_KIND) if self.event_mask else -1

    def plan(self) -> tp.List[tp.Tuple[int, str, int, int, float]]:
        """(kind slot, rule, first channel, channels, default) per feature: what ``hip_ops.EventTable`` takes."""
        return [(self.kinds.index(f.event_kind), f.rule, self.get_slice(f.name).start, f.dimension, f.default_value)
                for f in self.values()]


def _round(x: float) -> int:
    return int(round(x))


class DeviceEvents:
    """The events of one recording on the device.  ``events``: ``{kind: {"start": [n], "duration": [n], feature name:
    values}}`` for the builder's kinds, in the DataFrame's order, which is the painting order (a later event overwrites an
    earlier one); a kind that is left out has no event.  Values: ``[n]`` or ``[n, dimension]`` float64 for a constant
    feature, a sequence of ``n`` arrays ``[dimension, L_e]`` (fp32, already on the device or not) for the others.
    Everything is uploaded once; the arrays are read in place.  Per kind the running maximum of ``start + duration``
    travels with the events: with it two wavefront-wide searches bound a window's candidates, and the kernel tests
    every event between the bounds.

    The ``word`` kind takes two optional integer columns, ``"word_index"`` and ``"sequence_id"`` (each ``[n]``, both or
    none, non-negative): ``event.word_index`` and an integer the caller maps ``event.word_sequence`` to (Python's salted
    ``hash`` stays with the caller, as for ``WordHash``).  They stay resident as int64 (``word_info`` ``[n, 2]``) for the
    segment-level evaluation; without them nothing changes.  ``ValueError`` when one is missing, a length differs from
    ``n`` or a value is negative.

    ``ValueError`` names the first event whose ``start`` is below its predecessor's (or not finite), whose duration is
    negative, whose resampled length ``round(((start + duration) - start) * sample_rate)`` is below 1, or -- for a chunk
    feature with ``duration >= 0.5`` -- whose ``L / duration`` is outside (42, 52), the reference's assert
    (bm/features/audio.py:220-222)."""

    def __init__(self, builder: DeviceFeaturesBuilder, events: tp.Mapping[str, tp.Mapping[str, tp.Any]], device=None):
        self.builder = builder
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        sr = builder.sample_rate                               # events of other kinds are left out, as base.py:59 does
        self.n_events: tp.Dict[str, int] = {}
        self.kind_tables: tp.List[tp.Optional[tp.Tuple[torch.Tensor, ...]]] = []
        self.sources: tp.List[tp.Any] = [None] * len(builder)
        self.word_info: tp.Optional[torch.Tensor] = None       # [n, 2] int64 on the device: word_index, sequence_id
        self.word_info_host: tp.Optional[np.ndarray] = None    # the same on the host, for the dense segment ids
        for kind in builder.kinds:
            table = events.get(kind)
            n = 0 if table is None else len(table["start"])
            self.n_events[kind] = n
            if kind == WORD_KIND and table is not None:
                self._adopt_word_info(table, n)
            if n == 0:
                self.kind_tables.append(None)
                continue
            start = np.array(table["start"], dtype=np.float64).reshape(-1)
            dur = np.array(table["duration"], dtype=np.float64).reshape(-1)
            if len(dur) != n:
                raise ValueError(f"{kind}: {n} starts and {len(dur)} durations")
            for e in range(n):
                if not np.isfinite(start[e]) or (e and start[e] < start[e - 1]):
                    raise ValueError(f"{kind} event {e}: start {start[e]} after {start[e - 1] if e else None}; the starts "
                                     "of a kind must be finite and non-decreasing")
                if not dur[e] >= 0 or not np.isfinite(dur[e]):
                    raise ValueError(f"{kind} event {e}: duration {dur[e]}")
            stop = start + dur
            self.kind_tables.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                                          for a in (start, dur, np.maximum.accumulate(stop))))
            for f, feature in enumerate(builder.values()):
                if feature.event_kind != kind:
                    continue
                if feature.name not in table:
                    raise ValueError(f"{kind} events carry no values for the feature {feature.name}")
                values = table[feature.name]
                if feature.rule == "constant":
                    rows = np.asarray(values, dtype=np.float64).reshape(n, -1)
                    if rows.shape[1] != feature.dimension:
                        raise ValueError(f"{feature.name}: values of shape {np.shape(values)} for {n} events of "
                                         f"{feature.dimension} channels")
                    self.sources[f] = torch.from_numpy(rows.astype(np.float32)).to(self.device)
                    continue
                if len(values) != n:
                    raise ValueError(f"{feature.name}: {len(values)} arrays for {n} {kind} events")
                arrays, ers = [], []
                for e, a in enumerate(values):
                    a = torch.as_tensor(a)
                    if a.dim() == 1 and feature.dimension == 1:
                        a = a[None]
                    if a.dim() != 2 or a.shape[0] != feature.dimension or a.shape[1] < 1:
                        raise ValueError(f"{feature.name}, {kind} event {e}: an array of shape {tuple(a.shape)} for "
                                         f"{feature.dimension} channels")
                    L = a.shape[1]
                    if feature.rule == "resampled":
                        n_e = _round(((float(start[e]) + float(dur[e])) - float(start[e])) * sr)
                        if n_e < 1:
                            raise ValueError(f"{feature.name}, {kind} event {e}: a duration of {dur[e]} s is {n_e} samples "
                                             f"at {sr} Hz; a resampled event needs at least 1")
                        ers.append(0.)
                    else:
                        er = L / float(dur[e]) if dur[e] > 0 else 0.
                        if dur[e] >= 0.5 and not 42 < er < 52:
                            raise ValueError(f"{feature.name}, {kind} event {e}: {L} columns in {dur[e]} s are {er} per "
                                             "second, expected between 42 and 52")
                        ers.append(er)
                    arrays.append(a.to(device=self.device, dtype=torch.float32).contiguous())
                self.sources[f] = (arrays, ers)

    def _adopt_word_info(self, table: tp.Mapping[str, tp.Any], n: int) -> None:
        given = [c for c in WORD_INFO_COLUMNS if c in table]
        if not given:
            return
        if len(given) != len(WORD_INFO_COLUMNS):
            raise ValueError(f"{WORD_KIND} events carry {given[0]!r} without "
                             f"{[c for c in WORD_INFO_COLUMNS if c not in table][0]!r}: the word information is both or none")
        columns = []
        for c in WORD_INFO_COLUMNS:
            raw = np.asarray(table[c])
            if raw.ndim != 1 or len(raw) != n:
                raise ValueError(f"{c}: shape {raw.shape} for {n} {WORD_KIND} events")
            if raw.dtype.kind not in "iu" and not (raw.dtype.kind == "f" and np.array_equal(raw, np.trunc(raw))):
                raise ValueError(f"{c}: {raw.dtype} values that are not integers")
            if n and raw.min() < 0:
                raise ValueError(f"{c}: event {int(np.argmax(raw < 0))} is {raw[np.argmax(raw < 0)]}; the values are "
                                 "non-negative integers (-1 stands for \"no word\" in the evaluation's labels)")
            columns.append(raw.astype(np.int64))
        self.word_info_host = np.ascontiguousarray(np.stack(columns, axis=1)).reshape(n, 2)
        self.word_info = torch.from_numpy(self.word_info_host).to(self.device)

    def resident_bytes(self) -> int:
        total = sum(t.numel() * t.element_size() for k in self.kind_tables if k is not None for t in k)
        if self.word_info is not None:
            total += self.word_info.numel() * self.word_info.element_size()
        for s in self.sources:
            if isinstance(s, torch.Tensor):
                total += s.numel() * s.element_size()
            elif s is not None:
                total += sum(a.numel() * a.element_size() for a in s[0])
        return total
