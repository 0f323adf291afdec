"""The label rule of csrc/segment_eval.hip and the first-occurrence rule restated in numpy / Python floats
(scripts/run_eval_probs.py:27-57, 105-158), held to the live reference by tests/golden/segment_eval.npz
(test_segment_eval_cpu.py) and used as the truth beyond the fixture; the fixture's reader; and the fp64 margin of a
segment-level ranking that the maker and the end-to-end test assert before they compare hit counts for equality."""
import numpy as np

COLUMNS = ("word_hash", "word_index", "sequence_id", "segment_id", "subject_index", "recording_index", "word_event")
VALUE_BIT, DEST_BIT, RANGE_BIT, ID_RANGE_BIT = 1, 2, 4, 8
# 100 x FWD_TOL of tests/test_kernels_gpu.py (5e-6, the relative tolerance its retrieval scores are held to)
MARGIN = 100 * 5e-6


def check_at_time(tmin: float, sample_rate: float) -> int:
    return int((-tmin) * sample_rate) + 2


def positions(t0: int):
    """The candidate samples in the reference's order: t0, t0 - 1 (only if t0 > 0), t0 + 1."""
    return [t0, t0 - 1 if t0 > 0 else None, t0 + 1]


def decisive(row: np.ndarray, t0: int) -> int:
    """Which of the three positions gives the row's word hash; -1: all candidates are zero (legal here)."""
    for k, t in enumerate(positions(t0)):
        if t is not None and not row[t] == 0:            # NaN != 0: a NaN is taken, as torch.where(wh == 0, ...) does
            return k
    return -1


def word_hash(row: np.ndarray, t0: int):
    """(label, flag bits) of one fp32 row."""
    k = decisive(row, t0)
    if k < 0:
        return 0, 0
    v = float(np.float32(row[positions(t0)[k]]))
    if not abs(v) < 2.0 ** 63:                           # NaN, +-inf, too large
        return 0, VALUE_BIT
    return int(v), (VALUE_BIT if v != np.trunc(v) else 0)


def covers(es: float, ed: float, ws: float, sr: float, t0: int, T: int) -> bool:
    """_get_extra_info's slice of one word event holds column t0 (Python floats: fp64, one rounding per operation)."""
    a = sr * (float(es) - float(ws))
    b = a + sr * float(ed)
    ta, tb = int(a), int(b)
    if tb < 0:                                           # an empty span here; no event of the window's selection has it
        return False
    return max(0, ta) <= t0 < min(T, tb)


def word_event(start, duration, ws: float, sr: float, t0: int, T: int) -> int:
    """The last event in table order that covers t0, -1 without one: every event is tested."""
    last = -1
    for e, (es, ed) in enumerate(zip(start, duration)):
        if covers(es, ed, ws, sr, t0, T):
            last = e
    return last


def dense_ids(word_info):
    """``(rows, n_ids)`` as ``retrieval.dense_segment_ids`` gives them, by a dictionary over the sorted pairs."""
    pairs = sorted({(int(s), int(w)) for info in word_info if info is not None for w, s in np.asarray(info).reshape(-1, 2)})
    ids = {p: i + 1 for i, p in enumerate(pairs)}
    rows = [None if info is None else
            np.array([[int(w), int(s), ids[(int(s), int(w))]] for w, s in np.asarray(info).reshape(-1, 2)],
                     dtype=np.int64).reshape(-1, 3) for info in word_info]
    return rows, len(pairs) + 1


def labels(hash_rows, t0: int, mask, rec, wstart, subject, recording, tables, sr: float):
    """``(rows [kept, 7] int64, flag bits)``: what ``bm_segment_eval_labels`` writes.  ``hash_rows`` [B, T] fp32;
    ``tables``: per recording None or ``(start, duration, info [n, 3])``."""
    hash_rows = np.asarray(hash_rows, dtype=np.float32)
    B, T = hash_rows.shape
    assert 0 <= t0 and t0 + 1 < T
    kept = np.arange(B) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool))
    out, bits = [], 0
    for b in kept:
        wh, bb = word_hash(hash_rows[b], t0)
        bits |= bb
        r = int(rec[b])
        event, info = -1, (-1, -1, 0)
        if not 0 <= r < len(tables):
            bits |= RANGE_BIT
        elif tables[r] is not None:
            start, duration, rows = tables[r]
            event = word_event(start, duration, float(wstart[b]), sr, t0, T)
            if event >= 0:
                info = tuple(int(v) for v in rows[event])
        out.append([wh, info[0], info[1], info[2], int(subject[b]), int(recording[b]), event])
    return np.asarray(out, dtype=np.int64).reshape(-1, len(COLUMNS)), bits


def first_occurrence(ids, n_ids: int):
    """``(mask, first_row, flag bits)`` by the reference's loop over a ``seen`` set (scripts/run_eval_probs.py:141-149);
    an id outside [0, n_ids) is masked out, its first row is -1."""
    seen, mask, bits = {}, [], 0
    for i, v in enumerate(np.asarray(ids).tolist()):
        if not 0 <= v < n_ids:
            bits |= ID_RANGE_BIT
            mask.append(False)
            continue
        mask.append(v not in seen)
        seen.setdefault(v, i)
    first_row = np.array([seen[v] if 0 <= v < n_ids else -1 for v in np.asarray(ids).tolist()], dtype=np.int32)
    return np.asarray(mask, dtype=bool), first_row.reshape(-1), bits


def groups(values) -> np.ndarray:
    """The equality structure of a label column: every value replaced by the rank of its first appearance."""
    seen = {}
    return np.array([seen.setdefault(v, len(seen)) for v in np.asarray(values).tolist()], dtype=np.int64)


def hash_rows(rng: np.random.Generator, B: int, T: int, t0: int, vocabulary: int = 12, all_zero=()):
    """[B, T] fp32 word-hash rows (integers 1 .. vocabulary, 0 = no word): row b's label comes from position
    ``b % (allowed positions)`` of the three, the positions in front of it are zero (every fourth row: -0.0), the ones
    behind it hold other words, and the sample a missing guard would wrap around to (T - 1) is never zero -- nor are
    t0 - 2 and t0 + 2, which the chain of bm/wer.py would read and this one must not.  ``all_zero``: rows whose
    three candidates are all zero."""
    x = rng.integers(0, vocabulary + 1, (B, T)).astype(np.float32)
    x[:, T - 1] = rng.integers(1, vocabulary + 1, B)
    for t in (t0 - 2, t0 + 2):
        if 0 <= t < T:
            x[:, t] = rng.integers(1, vocabulary + 1, B)
    allowed = [k for k, t in enumerate(positions(t0)) if t is not None]
    for b in range(B):
        want = allowed[b % len(allowed)]
        for k, t in enumerate(positions(t0)):
            if t is None:
                continue
            if k < want or b in all_zero:
                x[b, t] = -0.0 if b % 4 == 3 else 0.0
            else:
                x[b, t] = rng.integers(1, vocabulary + 1)
    return x


def ranking_margins(preds, trues, target_ids, vocab_ids, k: int):
    """fp64, per prediction: (hit, relative gap) of the top-``k`` verdict of scripts/run_eval_probs.py:237-264 over
    de-duplicated candidates.  Exactly one candidate carries the row's segment (``vocab_ids`` are distinct and hold
    every target); with ``p`` its probability and ``q`` the ``k``-th largest among the others the row is a hit when
    ``p > q``, and |p - q| / max(p, q) is the distance to the other verdict.  Fewer than ``k`` others: the gap is
    infinite."""
    est = np.asarray(preds, dtype=np.float64).reshape(len(preds), -1)
    cand = np.asarray(trues, dtype=np.float64).reshape(len(trues), -1)
    target_ids, vocab_ids = np.asarray(target_ids), np.asarray(vocab_ids)
    assert len(set(vocab_ids.tolist())) == len(vocab_ids)
    result = []
    for i in range(len(est)):
        scores = cand @ est[i] / (1e-8 + np.linalg.norm(cand, axis=1))             # bm/losses.py get_scores
        probas = np.exp(scores - scores.max())
        probas /= probas.sum()
        match = vocab_ids == target_ids[i]
        assert match.sum() == 1
        p = probas[match][0]
        others = np.sort(probas[~match])[::-1]
        if len(others) < k:
            result.append((True, np.inf))
            continue
        q = others[k - 1]
        result.append((bool(p > q), abs(p - q) / max(p, q)))
    return result


def assert_margins(preds, trues, target_ids, vocab_ids, topks, what: str = ""):
    """Every top-k verdict is ``MARGIN`` away, relatively, from the other one.  Returns {k: hits} in fp64."""
    hits = {}
    for k in topks:
        margins = ranking_margins(preds, trues, target_ids, vocab_ids, k)
        worst = min(gap for _, gap in margins)
        assert worst >= MARGIN, f"{what}: a top-{k} verdict hangs on a relative gap of {worst}, below {MARGIN}"
        hits[k] = sum(hit for hit, _ in margins)
    return hits


def fixture_case(raw, meta, name):
    """Case ``name`` of tests/golden/segment_eval.npz: ``batches`` (dicts of ``features`` [B, 3, T], ``keep`` [B],
    ``rec``, ``wstart``, ``subject``, ``recording`` [B] and ``estimate`` / ``output`` of the kept rows, None for the fully
    rejected batch), ``tables`` (per recording None or ``(start, duration, word info [n, 2])``) and the case's meta."""
    case = meta["cases"][name]
    arrays = {k: raw[f"{name}/{k}"] for k in ("features", "keep", "rec", "wstart", "subject", "recording", "estimate",
                                              "output")}
    batches, at, kept_at = [], 0, 0
    for B in case["batches"]:
        b = {k: arrays[k][at:at + B] for k in ("features", "keep", "rec", "wstart", "subject", "recording")}
        m = int(b["keep"].sum())
        b["estimate"] = arrays["estimate"][kept_at:kept_at + m] if m else None
        b["output"] = arrays["output"][kept_at:kept_at + m] if m else None
        batches.append(b)
        at, kept_at = at + B, kept_at + m
    tables = []
    for r in range(meta["n_recordings"]):
        if f"{name}/r{r}/start" not in raw:
            tables.append(None)
            continue
        tables.append((raw[f"{name}/r{r}/start"], raw[f"{name}/r{r}/duration"],
                       np.stack([raw[f"{name}/r{r}/word_index"], raw[f"{name}/r{r}/sequence_id"]], axis=1)))
    return dict(batches=batches, tables=tables, meta=case)
