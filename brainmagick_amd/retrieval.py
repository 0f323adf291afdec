"""Batched segment-retrieval evaluation on the HIP path -- the second half of the headline metric
("top-10 segment-retrieval accuracy").

Mirrors ``scripts/run_eval_probs.py``: ``builds_probs`` (:267-307, probability of every candidate
for every prediction, in batches) and ``_get_accuracy_from_probs`` (:237-264, a row is a hit when
its own label is among the labels of its top-k candidates).  Differences to the reference: the
candidate norms are computed once (not once per batch of predictions), probabilities stay on the
GPU, and top-k + label matching are one HIP kernel (``bm_topk_rows``) instead of
``topk`` + gather + compare.

``wer_epoch`` is the test epoch of a ClipLoss model, bm/wer.py:21-121 (``get_wer(solver)``): it collects the estimates,
the outputs and the word label of every kept segment of a ``dataset.DeviceSegments`` test set in resident device arrays
(bm/wer.py:24-69; the labels by ONE ``hip_ops.word_hash_pick`` launch per batch) and hands them to ``get_wer``
(bm/wer.py:71-121).  Not built: a process group of more than one rank, a host-memory spill of the two arrays, and the
soft WER, which the reference computes and never returns.

``segment_eval_epoch`` is the first half of the headline metric, ``_load_test_data`` + ``run_eval``
(scripts/run_eval_probs.py:60-180, 310-382): it collects predictions, outputs and seven labels per kept test segment in
resident arrays (ONE ``hip_ops.segment_eval_labels`` launch per batch: the word hash at ``check_at_time``, and the word
index, sentence and segment of the word event that covers it, read from the resident event tables), de-duplicates the
candidates with ``hip_ops.first_occurrence`` and ranks with ``builds_probs`` + ``get_accuracy_from_probs``.
"""
import typing as tp

import numpy as np
import torch

from . import distrib
from . import hip_ops as H
from .features import WORD_KIND
from .losses import ClipLoss


def builds_probs(clip: ClipLoss, preds: torch.Tensor, trues: torch.Tensor, dset_args=None,
                 batch_size: int = 1000, tmin=None, tmax=None) -> torch.Tensor:
    """[N, C, T] predictions x [N', C, T] candidates -> [N, N'] probabilities (on the GPU)."""
    trim_min = trim_max = None
    if tmin is not None:
        trim_min = int((tmin - dset_args.tmin) * dset_args.sample_rate)
    if tmax is not None:
        trim_max = int((tmax - dset_args.tmin) * dset_args.sample_rate)
    preds = preds[..., trim_min:trim_max]
    trues = trues[..., trim_min:trim_max]
    candidates = trues.cuda().contiguous()
    Bc = candidates.shape[0]
    K = candidates.numel() // Bc
    inv = H.clip_inv_norms(candidates)
    probs = torch.empty(len(preds), Bc, device=candidates.device, dtype=torch.float32)
    for lo in range(0, len(preds), batch_size):
        est = preds[lo:lo + batch_size].cuda().contiguous()
        part = H.gemm_nt_partials(est, candidates, 1, est.shape[0], Bc, K, (0, K), (0, K))
        _, p, _, _ = H.clip_ce(part, inv, want_probs=True)
        probs[lo:lo + batch_size] = p
    return probs


def get_accuracy_from_probs(probs: torch.Tensor, target_labels: torch.Tensor,
                            vocab_labels: torch.Tensor, topk: int = 10) -> float:
    """scripts/run_eval_probs.py:237-264.  probs [B, V]; target_labels [B]; vocab_labels [V]."""
    assert len(target_labels) == len(probs)
    assert len(vocab_labels) == probs.shape[1]
    return _topk_hits(probs, target_labels, vocab_labels, topk).float().mean().item()


def _topk_hits(probs: torch.Tensor, target_labels: torch.Tensor, vocab_labels: torch.Tensor, topk: int) -> torch.Tensor:
    """[B] int32: 1 where the row's own label is among the labels of its ``topk`` most probable columns."""
    _, _, hits = H.topk_rows(probs.contiguous(), topk,
                             vocab_labels.to(probs.device, torch.int64).contiguous(),
                             target_labels.to(probs.device, torch.int64).contiguous())
    return hits


def segment_topk_accuracy(clip: ClipLoss, preds: torch.Tensor, trues: torch.Tensor,
                          labels: tp.Optional[torch.Tensor] = None, topks=(1, 5, 10),
                          batch_size: int = 1000) -> tp.Dict[str, float]:
    """Top-k segment accuracy: segment i is retrieved when candidate i (or any candidate carrying
    the same label, e.g. the same audio segment hash) is among its k most probable candidates."""
    if labels is None:
        labels = torch.arange(len(trues))
    probs = builds_probs(clip, preds, trues, batch_size=batch_size)
    return {f"top{k}": get_accuracy_from_probs(probs, labels[:len(preds)], labels, k) for k in topks}


def get_wer(clip: ClipLoss, estimates: torch.Tensor, outputs: torch.Tensor, word_hashes: torch.Tensor,
            n_negatives: tp.Optional[int] = 10_000, topx: int = 10,
            generator: tp.Optional[torch.Generator] = None,
            batch_size: int = 1000, wer_random: bool = False) -> tp.Dict[str, float]:
    """Word-level top-k "word error rate" of bm/wer.py:67-121, batched on the GPU.

    Reference semantics, per test segment i: the negatives are a fixed random subset of the test
    outputs whose LAST entry is replaced by the segment's own target (wer.py:71-78,93-94); the
    probabilities over negatives are aggregated per word (wer.py:100-103); the segment is correct
    when its word is among the ``topx`` most probable negatives (``wer``) / vocabulary words
    (``wer_vocab``).  The reference re-scans all N candidates once per test segment (a Python loop
    of GEMVs); here: ONE MFMA GEMM for all scores, a row-wise dot product for the own-target column,
    a row softmax, a deterministic per-word segmented sum and two top-k passes.

    ``wer_random`` (`test.wer_random`, wer.py:95-96): every estimate is replaced by ``torch.randn_like`` of it, drawn on
    the device per block of ``batch_size`` estimates (the reference draws per estimate); the chance level."""
    n = len(outputs)
    if n_negatives:
        perm = torch.randperm(n, generator=generator)
        kept = perm[:n_negatives]
    else:
        kept = torch.arange(n)
    negatives = outputs[kept].cuda().contiguous()
    negative_hashes = word_hashes[kept].to(torch.int64)
    N = len(negatives)
    K = negatives.numel() // N
    dev = negatives.device
    # fixed columns 0..N-2 grouped by word; the own-target column N-1 is added per row
    fixed_hashes = negative_hashes[:N - 1]
    vocab, inverse = torch.unique(torch.cat([fixed_hashes, word_hashes.to(torch.int64)]),
                                  return_inverse=True)
    col_vocab = inverse[:N - 1]
    order = torch.argsort(col_vocab, stable=True).to(torch.int32)
    counts = torch.bincount(col_vocab, minlength=len(vocab))
    seg = torch.zeros(len(vocab) + 1, dtype=torch.int32)
    seg[1:] = torch.cumsum(counts, 0)
    own_vocab = inverse[N - 1:]                               # vocabulary index of every segment's word
    order_d, seg_d, vocab_d = order.to(dev), seg.to(dev), vocab.to(dev)
    inv = H.clip_inv_norms(negatives)
    correct = correct_vocab = 0.0
    for lo in range(0, len(estimates), batch_size):
        est = estimates[lo:lo + batch_size].cuda().contiguous()
        if wer_random:
            est = torch.randn_like(est)
        own = outputs[lo:lo + batch_size].cuda().contiguous()
        wh = word_hashes[lo:lo + batch_size].to(dev, torch.int64)
        m = est.shape[0]
        part = H.gemm_nt_partials(est, negatives, 1, m, N, K, (0, K), (0, K))
        scores, _, _, _ = H.clip_ce(part, inv)
        scores[:, N - 1] = H.rowwise_dot(est.view(m, K), own.view(m, K), H.clip_inv_norms(own))
        probas = H.row_softmax(scores)
        # candidate-level: labels of the columns, with the own word on the last column
        # (a per-row label for the last column: handle it by checking the two cases separately)
        sentinel = int(min(int(negative_hashes.min()), int(word_hashes.min()))) - 1
        col_labels = torch.cat([fixed_hashes.to(dev),
                                torch.full((1,), sentinel, dtype=torch.int64, device=dev)])
        idx, _, hits = H.topk_rows(probas, min(topx, N), col_labels, wh)
        own_in_top = (idx == N - 1).any(1)
        correct += float((hits.bool() | own_in_top).sum())
        # vocabulary-level
        pv = H.segment_sum_cols(probas, order_d, seg_d)
        ov = own_vocab[lo:lo + m].to(dev)
        pv[torch.arange(m, device=dev), ov] += probas[:, N - 1]
        _, _, hits_v = H.topk_rows(pv, min(topx, pv.shape[1]), vocab_d, wh)
        # vocabulary entries that have zero mass only exist for other rows' own words: harmless
        correct_vocab += float(hits_v.sum())
    total = len(estimates)
    return {"wer": 1 - correct / total, "wer_vocab": 1 - correct_vocab / total}


# One flag word per device for the word labels (hip_ops.WORD_HASH_*_BIT), owned by this module like the dataset's
# range flag -- NOT the Solver's flag word.  Read once per test epoch, after the last batch.
word_hash_flag = H.DeviceFlag()


def raise_if_word_hash_error(device) -> None:
    """Synchronising check of the flag, which it clears."""
    bits = word_hash_flag.take(device)
    if bits & H.WORD_HASH_ALL_ZERO_BIT:
        raise AssertionError("assert (wh != 0).all() (bm/wer.py:65): a kept segment has no word hash at check_at_time, "
                             "one or two samples around it")
    if bits & H.WORD_HASH_VALUE_BIT:
        raise AssertionError("a word hash (bm/wer.py:58-65) is not finite, not an integer or not below 2^63 in magnitude")
    if bits:
        raise AssertionError("more kept segments than rows in the label array (bm/wer.py:66)")


def check_at_time(tmin: float, sample_rate: float) -> int:
    """bm/wer.py:46, the reference's expression: the sample of the window at which the word's hash is read."""
    return int((-tmin) * sample_rate) + 2


def wer_segments(segments, wer_recordings: tp.Optional[int] = None, wer_study: tp.Optional[str] = None):
    """bm/wer.py:28-35 over a ``DeviceSegments``: the recordings that have segments (the reference's test datasets),
    those of the study ``wer_study`` (``recording.study_name()``), the first ``wer_recordings`` of them."""
    have = [i for i in range(len(segments.recordings)) if (segments.rec == i).any()]
    picked = have
    if wer_study is not None:
        picked = [i for i in picked if segments.recordings[i].recording.study_name() == wer_study]
    if wer_recordings is not None:
        picked = picked[:wer_recordings]
    return segments if picked == have else segments.subset(picked)


def _free_bytes(device) -> int:
    """What an allocation on ``device`` can still get: the driver's free memory plus what torch's allocator holds
    unused."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free) + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _collect(solver, loader: tp.Iterable, total: int, test_features, used_names: tp.Sequence[str], *, name: str,
             label_cols: tp.Tuple[int, ...], flag: "H.DeviceFlag", launch: tp.Callable[..., None], what: str, cite: str):
    """The collection loop of both test epochs: ``(estimates [n, ...], outputs [n, ...], labels [n, *label_cols]
    int64)`` of the kept segments of ``loader``'s device batches (at most ``total`` segments), views of resident device
    arrays that are allocated at the first kept batch's row shape.  Under ``no_grad`` and in eval mode, per batch:
    ``solver._process_batch`` on the batch with the extracted features; a fully rejected batch is skipped; estimate and
    output are copied in at the running row count ``n``, and ``launch(batch, k, reject_mask, labels, n, m)`` writes the
    labels of batch ``k``'s ``m`` kept rows from ``labels[n]`` on.  ``flag``'s word is cleared before the first launch
    (bits an epoch that ended in an exception left behind) and left to the caller to read.  ``name``: "wer" or
    "segment_eval", for the errors; ``what`` / ``cite``: the two texts that differ."""
    from .solver import Solver
    used_names = list(used_names)
    Solver._eval_mode(solver)                               # unbound: any solver that has ``_all_models`` and ``loss``
    estimates = outputs = labels = None
    n = 0
    with torch.no_grad():
        for k, batch in enumerate(loader):
            features = test_features.extract_features(batch.features, used_names)
            estimate, output, _, reject_mask = solver._process_batch(batch.replace(features=features))
            if getattr(solver, "_gather", None) is not None and solver.feature_model is None:
                solver._gather.wait()                       # whole-node negatives: nobody consumes the candidates here
            if estimate is None:
                continue
            device = estimate.device
            if estimates is None:
                need = total * 4 * (estimate[0].numel() + output[0].numel()) + total * 8 * int(np.prod(label_cols))
                free = _free_bytes(device)
                if need > free:
                    raise NotImplementedError(f"Not built: a host-memory spill for {what} of {total} segments take {need} "
                                              f"bytes on the device, {free} bytes are free")
                estimates = torch.empty((total,) + tuple(estimate.shape[1:]), device=device, dtype=torch.float32)
                outputs = torch.empty((total,) + tuple(output.shape[1:]), device=device, dtype=torch.float32)
                labels = torch.empty((total,) + label_cols, device=device, dtype=torch.int64)
                flag(device).zero_()
            m = estimate.shape[0]
            if n + m > total:
                raise ValueError(f"collect_{name}: the loader delivers more than the announced {total} segments")
            estimates[n:n + m].copy_(estimate)
            outputs[n:n + m].copy_(output)
            launch(batch, k, reject_mask.to(device), labels, n, m)
            n += m
    solver.check_pending_flags()
    if n == 0:
        raise RuntimeError(f"{name}_epoch: every test segment was rejected ({cite} would concatenate an empty list)")
    return estimates[:n], outputs[:n], labels[:n]


def collect_wer(solver, loader: tp.Iterable, total: int, test_features, used_names: tp.Sequence[str],
                check_at_time: int) -> tp.Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """bm/wer.py:24-25, 47-69, the collection loop: ``(estimates [n, ...], outputs [n, ...], word_hashes [n] int64)`` of
    the kept segments of ``loader``'s device batches (at most ``total`` segments), all three views of resident device
    arrays.  See ``wer_epoch``, which builds the loader."""
    channel = test_features.get_slice("WordHash").start

    def launch(batch, k, reject_mask, hashes, n, m):
        H.word_hash_pick(batch.features, channel, check_at_time, reject_mask, hashes, n, word_hash_flag(hashes.device),
                         count=m)
    out = _collect(solver, loader, total, test_features, used_names, name="wer", label_cols=(), flag=word_hash_flag,
                   launch=launch, what="the test epoch -- the estimates and outputs", cite="bm/wer.py:67")
    raise_if_word_hash_error(out[2].device)
    return out


def wer_from_loader(solver, loader: tp.Iterable, total: int, test_features, used_names: tp.Sequence[str],
                    check_at_time: int, *, wer_negatives: tp.Optional[int] = 10_000, wer_topx: int = 10,
                    wer_random: bool = False, negatives_generator: tp.Optional[torch.Generator] = None):
    """bm/wer.py:47-121 behind the loader: ``collect_wer``, then the ranking of ``get_wer``."""
    estimates, outputs, hashes = collect_wer(solver, loader, total, test_features, used_names, check_at_time)
    return get_wer(solver.loss, estimates, outputs, hashes, n_negatives=wer_negatives, topx=wer_topx,
                   generator=negatives_generator, wer_random=wer_random)


def _epoch_prologue(who: str, segments, test_features, used_names: tp.Sequence[str], n_recordings: tp.Optional[int],
                    study: tp.Optional[str], tmin: tp.Optional[float], batch_size: int,
                    shape_check: tp.Callable[[tp.Tuple[int, int, int], int, int, int], None], *,
                    own_checks: tp.Callable[[], None] = lambda: None,
                    segment_checks: tp.Callable[[tp.Any], None] = lambda segments: None, rank_note: str = "",
                    empty_note: str = ""):
    """What ``wer_epoch`` and ``segment_eval_epoch`` (``who``) check and derive before they build their loader, in the
    order in which they raise: one rank; ``own_checks()``; the builder describes the segments' channels and holds the
    used features; the picked recordings (``wer_segments``); ``segment_checks(picked segments)``; ``check_at_time`` from
    ``tmin`` (`dset.test.tmin`, by default the segments' own); the label launch's ``shape_check(batch shape, WordHash
    channel, check_at_time, total)``; a test set that is not empty.  Returns ``(used_names, segments, total,
    check_at_time)``."""
    if distrib.world_size() > 1:
        raise NotImplementedError(f"Not built: {who} in a process group of more than one rank{rank_note}")
    own_checks()
    if segments.n_features != test_features.dimension:
        raise ValueError(f"the segments carry {segments.n_features} feature channels, test_features describes "
                         f"{test_features.dimension}")
    used_names = list(used_names)
    assert all([name in test_features for name in used_names])          # bm/features/base.py:152
    channel = test_features.get_slice("WordHash").start
    segments = wer_segments(segments, n_recordings, study)
    total = len(segments)
    segment_checks(segments)
    if tmin is None:
        tmin = segments.tmin
    t0 = check_at_time(tmin, segments.sample_rate)
    shape_check((batch_size, test_features.dimension, segments.T), channel, t0, total)
    if total == 0:
        raise RuntimeError(f"{who}: no test segment{empty_note}")
    return used_names, segments, total, t0


def wer_epoch(solver, segments, test_features, used_names: tp.Sequence[str], *, batch_size: int,
              tmin: tp.Optional[float] = None, wer_negatives: tp.Optional[int] = 10_000, wer_topx: int = 10,
              wer_random: bool = False, wer_recordings: tp.Optional[int] = None, wer_study: tp.Optional[str] = None,
              generator: tp.Optional[torch.Generator] = None,
              negatives_generator: tp.Optional[torch.Generator] = None) -> tp.Dict[str, float]:
    """``get_wer(solver)`` of bm/wer.py:21-121 over a ``DeviceSegments`` test set: {"wer", "wer_vocab"}.

    ``segments``: word-conditioned windows whose features builder ``test_features`` holds the used features plus
    ``WordHash`` (`dset.features + extra_test_features`); ``used_names``: the features the model was trained on
    (``solver.used_features.keys()``), cut out per batch by ``test_features.extract_features``.  ``wer_recordings`` /
    ``wer_study`` / ``wer_negatives`` / ``wer_topx`` / ``wer_random``: `test.*` of the reference's configuration;
    ``tmin``: `dset.test.tmin`, by default the segments' own.  ``generator`` shuffles the loader (bm/wer.py:36-37),
    ``negatives_generator`` draws the ``randperm`` of the negatives (bm/wer.py:72).

    Per batch, under ``no_grad`` and in eval mode: ``solver._process_batch`` on the batch with the extracted features;
    a fully rejected batch is skipped; estimate and output are copied into two resident arrays (allocated for
    ``len(segments)`` rows at the first batch's row shape) at the running row count, and ONE ``hip_ops.word_hash_pick``
    launch writes the labels of the kept rows from the loader's own ``batch.features``.  Nothing is copied to the host:
    the host waits only where ``_process_batch`` does (its asserts, a ``ScaleReject`` that counts its rejections) and
    for the labels' flag word after the last batch -- ``AssertionError`` for the reference's ``assert (wh != 0).all()``.

    Deviation: the label is the int64 of the fp32 hash, the reference's ``.int()`` wraps it to 32 bits; they agree for
    hashes below 2^24 in magnitude (``WordHash(buckets=...)``).  Not built (``NotImplementedError``): more than one
    rank (the reference shards the loader and averages the metrics), test sets whose two arrays do not fit on the
    card (no host-memory spill); the soft WER is not computed."""
    def clip_loss():
        if not isinstance(solver.loss, ClipLoss):
            raise AssertionError(f"wer_epoch ranks with ClipLoss (bm/wer.py:87), the solver's loss is "
                                 f"{type(solver.loss).__name__}")
    used_names, segments, total, t0 = _epoch_prologue(
        "wer_epoch", segments, test_features, used_names, wer_recordings, wer_study, tmin, batch_size,
        lambda shape, channel, t0, total: H.word_hash_pick_check(shape, channel, t0, total, 0, 0), own_checks=clip_loss,
        rank_note=" (the reference shards the test loader over the ranks and averages the metrics, bm/wer.py:37, 121)",
        empty_note=" (bm/wer.py:67 would concatenate an empty list)")
    from .dataset import DeviceSegmentLoader
    loader = DeviceSegmentLoader(segments, batch_size, shuffle=True, generator=generator)
    return wer_from_loader(solver, loader, total, test_features, used_names, t0, wer_negatives=wer_negatives,
                           wer_topx=wer_topx, wer_random=wer_random, negatives_generator=negatives_generator)


# ---------------------------------------------------------------------------------------------------------------------
# The segment-level evaluation, scripts/run_eval_probs.py: _load_test_data (:60-180) + run_eval (:310-382)
# ---------------------------------------------------------------------------------------------------------------------
METADATA_KEYS = ("word_hashes", "word_indices", "seq_indices", "segment_hashes", "subject_id", "recording_id",
                 "word_event")                          # the columns of hip_ops.SEGMENT_EVAL_COLUMNS, in that order

# One flag word per device for the evaluation's labels and the first occurrences (hip_ops.SEGMENT_EVAL_*_BIT,
# FIRST_OCCURRENCE_RANGE_BIT), owned by this module.  Read once per evaluation, after the first-occurrence launches.
segment_eval_flag = H.DeviceFlag()


def raise_if_segment_eval_error(device) -> None:
    """Synchronising check of the flag, which it clears."""
    bits = segment_eval_flag.take(device)
    if bits & H.SEGMENT_EVAL_VALUE_BIT:
        raise AssertionError("a word hash (scripts/run_eval_probs.py:116-130) is not finite, not an integer or not below "
                             "2^63 in magnitude")
    if bits & H.SEGMENT_EVAL_RANGE_BIT:
        raise IndexError("a test segment's recording index is outside the word tables")
    if bits & H.FIRST_OCCURRENCE_RANGE_BIT:
        raise IndexError("a segment id is outside the dense ids of the evaluated set")
    if bits:
        raise AssertionError("more kept segments than rows in the label array (scripts/run_eval_probs.py:132)")


def dense_segment_ids(word_info: tp.Sequence[tp.Optional[np.ndarray]]):
    """``(rows, n_ids)``: per recording None or int64 ``[n_words, 3]`` = ``(word_index, sequence_id, segment_id)``, the
    segment id dense over the distinct ``(sequence_id, word_index)`` pairs of all the recordings given (``word_info``:
    their ``DeviceEvents.word_info_host`` ``[n_words, 2]``, None for a recording outside the evaluated set), in the
    pairs' sorted order and starting at 1 -- the equality structure of ``hash(f"{sid}_{wid}")``
    (scripts/run_eval_probs.py:137-139).  Id 0 is kept for "no word", the reference's ``hash("-1_-1")``; ``n_ids``
    counts it.  Pure numpy, once per evaluated set."""
    given = [w for w in word_info if w is not None]
    if not given:
        return [None] * len(word_info), 1
    pairs = np.concatenate([np.asarray(w, dtype=np.int64).reshape(-1, 2)[:, ::-1] for w in given])     # (sequence, word)
    distinct, inverse = np.unique(pairs, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    rows, at = [], 0
    for w in word_info:
        if w is None:
            rows.append(None)
            continue
        w = np.asarray(w, dtype=np.int64).reshape(-1, 2)
        rows.append(np.ascontiguousarray(np.concatenate([w, inverse[at:at + len(w), None] + 1], axis=1)))
        at += len(w)
    return rows, len(distinct) + 1


def collect_segment_eval(solver, loader, total: int, test_features, used_names: tp.Sequence[str], check_at_time: int,
                         infos: "H.WordInfoTable") -> tp.Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The loop of ``_load_test_data`` (scripts/run_eval_probs.py:95-158) over a ``DeviceSegmentLoader``: ``(preds [n,
    ...], trues [n, ...], labels [n, 7] int64)`` of the kept segments, views of resident device arrays; the structure of
    ``collect_wer``.  ``trues`` is every kept row's output: the de-duplication happens once, over the epoch."""
    segments = loader.segments
    channel = test_features.get_slice("WordHash").start
    word_kind = segments.builder.kinds.index(WORD_KIND)
    events = segments.tables()[1]

    def launch(batch, k, reject_mask, labels, n, m):
        H.segment_eval_labels(batch.features, channel, check_at_time, reject_mask, loader.epoch_arrays,
                              k * loader.batch_size, events, word_kind, infos, segments.sample_rate, labels, n,
                              segment_eval_flag(labels.device), count=m)
    return _collect(solver, loader, total, test_features, used_names, name="segment_eval",
                    label_cols=(len(METADATA_KEYS),), flag=segment_eval_flag, launch=launch,
                    what="the segment-level evaluation -- the predictions, outputs and labels",
                    cite="scripts/run_eval_probs.py:179")


def segment_eval_epoch(solver, segments, test_features, used_names: tp.Sequence[str], *, batch_size: int,
                       tmin: tp.Optional[float] = None, n_recordings: tp.Optional[int] = None,
                       test_study: tp.Optional[str] = None, topks: tp.Sequence[int] = (1, 5, 10),
                       probs_batch_size: int = 1000, n_negatives: int = 20_000, shuffle: bool = False,
                       generator: tp.Optional[torch.Generator] = None, return_probs: bool = False,
                       clip: tp.Optional[tp.Mapping[str, tp.Any]] = None) -> tp.Dict[str, tp.Any]:
    """The segment-level evaluation of scripts/run_eval_probs.py over a ``DeviceSegments`` test set: the collection of
    ``_load_test_data`` (:60-180), then ``run_eval`` (:310-382) -- the paper's top-k accuracy over unique audio
    segments.

    ``segments``: word-conditioned windows over recordings with events whose word events carry ``word_index`` and
    ``sequence_id`` (``features.DeviceEvents``) and whose builder ``test_features`` holds the used features plus
    ``WordHash``; ``used_names``: the features the model was trained on.  ``n_recordings`` / ``test_study``: as
    ``wer_segments`` picks recordings; ``tmin``: `dset.test.tmin`, by default the segments' own; ``shuffle`` /
    ``generator``: the loader's order (``Evaluator.shuffle_test_data``); ``topks``, ``probs_batch_size``,
    ``n_negatives``: `run_eval`'s.  A solver whose loss is not a ClipLoss ranks with ``ClipLoss(**clip)`` (:318-322).

    Once per evaluated set the host numbers the distinct ``(sequence_id, word_index)`` pairs (``dense_segment_ids``:
    numpy; 0 = no word) and uploads one ``[n_words, 3]`` array per recording.  Per batch, under ``no_grad`` and in eval
    mode: ``solver._process_batch`` on the batch with the extracted features; a fully rejected batch is skipped;
    prediction and output are copied into two resident arrays at the running row count and ONE
    ``hip_ops.segment_eval_labels`` launch writes the seven labels of the kept rows.  Nothing is copied to the host: the
    host waits only where ``_process_batch`` does, and once for the flag word.  Then ``hip_ops.first_occurrence`` over the
    segment ids gives ``trues = outputs[mask]`` and ``vocab_segment = segment_id[mask]`` (first occurrences in row order
    do not depend on the batching), and per ``k`` the accuracy is ``builds_probs`` + ``get_accuracy_from_probs`` with the
    segment ids as labels -- block by block over ``probs_batch_size`` predictions, so that the ``[N, V]`` matrix is
    never resident, unless ``return_probs`` asks for it.

    Returns ``{"acc": {k: accuracy}, "metadata": {key: int64 device tensor [N]} for METADATA_KEYS (the reference's
    names, plus "word_event": the index of the word in its recording's word table, -1 without one), "vocab_segment",
    "negative_stats": the five counts of :371-377, "probs_segment" (with return_probs)}``.

    Deviation: the reference squeezes ``hash(word_sequence)`` through an fp32 tensor before ``.long()``; the ids here
    are exact int64.  The two agree wherever the caller's ids are below 2^24.  Segment "hashes" are the dense ids, not
    Python hashes: only their equality structure is the reference's.

    Not built: the string columns (``word_strings``, ``word_segment_strings``, ``study``, ``*_uid``; ``word_event`` and
    ``recording_id`` let a caller look them up), the reference's fallback that hashes the word strings when the
    builder has no ``WordHash`` (``ValueError``), the files on disk, ``Evaluator`` / ``EvalJob`` / submitit, more than
    one rank and a host-memory spill (``NotImplementedError``)."""
    def has_words():
        if "WordHash" not in test_features:
            raise ValueError("segment_eval_epoch: the features builder has no WordHash; the reference's fallback that "
                             "hashes the word strings (scripts/run_eval_probs.py:110-113) is not built")
        if getattr(segments, "builder", None) is None:
            raise ValueError("segment_eval_epoch: the segments carry no events (full-length feature arrays hold no words)")

    def has_word_info(picked):
        for r in sorted(set(int(r) for r in picked.rec)):
            if picked.recordings[r].events.word_info_host is None:
                raise ValueError(f"segment_eval_epoch: the word events of recording {r} carry no word_index / "
                                 "sequence_id columns (features.DeviceEvents)")
    used_names, segments, total, t0 = _epoch_prologue(
        "segment_eval_epoch", segments, test_features, used_names, n_recordings, test_study, tmin, batch_size,
        lambda shape, channel, t0, total: H.segment_eval_labels_check(shape, channel, t0, (total, len(METADATA_KEYS)),
                                                                      0, 0),
        own_checks=has_words, segment_checks=has_word_info)
    evaluated = set(int(r) for r in segments.rec)
    clip_loss = solver.loss if isinstance(solver.loss, ClipLoss) else ClipLoss(**dict(clip or {})).to(segments.device)
    from .dataset import DeviceSegmentLoader
    rows, n_ids = dense_segment_ids([segments.recordings[r].events.word_info_host if r in evaluated else None
                                     for r in range(len(segments.recordings))])
    infos = H.WordInfoTable(rows, n_ids, segments.device)
    loader = DeviceSegmentLoader(segments, batch_size, shuffle=shuffle, generator=generator)
    preds, outputs, labels = collect_segment_eval(solver, loader, total, test_features, used_names, t0, infos)
    device = labels.device
    columns = labels.t().contiguous()
    metadata = dict(zip(METADATA_KEYS, columns))
    segment_id = metadata["segment_hashes"]
    mask, _ = H.first_occurrence(segment_id, n_ids, segment_eval_flag(device))
    raise_if_segment_eval_error(device)
    trues = outputs[mask]
    vocab_segment = segment_id[mask]
    n = len(preds)
    result: tp.Dict[str, tp.Any] = {}
    if return_probs:
        probs = builds_probs(clip_loss, preds, trues, batch_size=probs_batch_size)
        acc = {k: get_accuracy_from_probs(probs, segment_id, vocab_segment, topk=k) for k in topks}
        result["probs_segment"] = probs
    else:
        hits = {k: torch.zeros((), device=device, dtype=torch.int64) for k in topks}
        for lo in range(0, n, probs_batch_size):
            block = builds_probs(clip_loss, preds[lo:lo + probs_batch_size], trues, batch_size=probs_batch_size)
            for k in topks:
                hits[k] += _topk_hits(block, segment_id[lo:lo + probs_batch_size], vocab_segment, k).sum()
        acc = {k: int(hits[k]) / n for k in topks}
    word_hashes = metadata["word_hashes"]
    result.update(acc=acc, metadata=metadata, vocab_segment=vocab_segment, negative_stats={
        "n_test_samples": n,
        "n_test_vocab": len(torch.unique(word_hashes)),
        "n_test_segments": len(torch.unique(segment_id)),
        "n_neg_samples": len(word_hashes[:n_negatives]),
        "n_neg_segments": len(torch.unique(segment_id[:n_negatives])),
    })
    return result
