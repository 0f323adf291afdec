"""The word-label rule of csrc/wer.hip restated in numpy (bm/wer.py:46, 58-66), held to the live reference by
tests/golden/wer_epoch.npz (test_wer_epoch_cpu.py) and used as the truth beyond the fixture; the canned batches of that
fixture (its maker and the tests rebuild nothing: the fixture stores them); and the fp64 margin of a word-level ranking
that the maker and the end-to-end test assert before they compare hit counts for equality."""
import numpy as np

ALL_ZERO_BIT, VALUE_BIT, DEST_BIT = 1, 2, 4
# 100 x FWD_TOL of tests/test_kernels_gpu.py (5e-6, the relative tolerance its retrieval scores are held to)
MARGIN = 100 * 5e-6


def check_at_time(tmin: float, sample_rate: float) -> int:
    return int((-tmin) * sample_rate) + 2


def positions(t0: int):
    """The candidate samples in the reference's order: t0, t0 - 1 (only if t0 > 0), t0 + 1, t0 - 2 (only if t0 > 1),
    t0 + 2; None where the guard leaves one out."""
    return [t0, t0 - 1 if t0 > 0 else None, t0 + 1, t0 - 2 if t0 > 1 else None, t0 + 2]


def decisive(row: np.ndarray, t0: int) -> int:
    """Which of the five positions (0 .. 4) gives the row's label; -1: all candidates are zero."""
    for k, t in enumerate(positions(t0)):
        if t is not None and not row[t] == 0:            # NaN != 0: a NaN is taken, as torch.where(wh == 0, ...) does
            return k
    return -1


def pick(word_hash: np.ndarray, t0: int, mask=None):
    """``(labels int64 [kept rows], flag bits)`` of ``word_hash`` [B, T] fp32: what ``bm_word_hash_pick`` writes."""
    word_hash = np.asarray(word_hash, dtype=np.float32)
    B, T = word_hash.shape
    assert 0 <= t0 and t0 + 2 < T
    rows = np.arange(B) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool))
    labels, bits = [], 0
    for b in rows:
        k = decisive(word_hash[b], t0)
        if k < 0:
            bits |= ALL_ZERO_BIT
            labels.append(0)
            continue
        v = float(word_hash[b, positions(t0)[k]])
        if not abs(v) < 2.0 ** 63:                       # NaN, +-inf, too large
            bits |= VALUE_BIT
            labels.append(0)
            continue
        if v != np.trunc(v):
            bits |= VALUE_BIT
        labels.append(int(v))
    return np.asarray(labels, dtype=np.int64), bits


def hash_rows(rng: np.random.Generator, B: int, T: int, t0: int, vocabulary: int = 12, all_zero=()):
    """[B, T] fp32 word-hash rows (integers 1 .. vocabulary, 0 = no word): row b's label comes from position
    ``b % (allowed positions)`` of the five, the positions in front of it are zero (every fourth row: -0.0), the ones
    behind it hold other words, and the samples a missing guard would wrap around to (T - 1, T - 2) are never zero.
    ``all_zero``: rows whose five candidates are all zero."""
    x = rng.integers(0, vocabulary + 1, (B, T)).astype(np.float32)
    x[:, T - 2:] = rng.integers(1, vocabulary + 1, (B, 2))
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


def ranking_margins(estimates, outputs, word_hashes, kept, topx: int):
    """fp64, per test segment: (hit, relative gap) at candidate level and at vocabulary level of bm/wer.py:91-112.

    A segment is a hit when a candidate (a word) that carries its label is among the ``topx`` most probable.  With
    ``p`` = the largest probability among the matching entries and ``q`` = the ``topx``-th largest among the others,
    that is ``p > q``; the gap |p - q| / max(p, q) is the distance to the other verdict.  Where the ``topx``-th and the
    ``(topx + 1)``-th probability decide the verdict (one of them matches, the entries above them do not), they ARE p
    and q; everywhere else |p - q| is larger than their difference would need to be.  Fewer than ``topx`` other
    entries: nothing can change the verdict, the gap is infinite.

    This REPLACES the literal "``topx``-th against ``(topx + 1)``-th probability" gap: that one cannot be asked for,
    because whenever ``kept`` contains segment i the own target in the last column duplicates a candidate and the two
    equal probabilities can sit at ranks ``topx`` and ``topx + 1`` (a gap of exactly 0 that decides nothing: both carry
    the same word).  Order statistics are 1-Lipschitz in the probabilities, so a perturbation below |p - q| cannot
    change ``p > q``, which is the verdict; where the literal pair does decide, it is this pair."""
    est = np.asarray(estimates, dtype=np.float64).reshape(len(estimates), -1)
    out = np.asarray(outputs, dtype=np.float64).reshape(len(outputs), -1)
    wh = np.asarray(word_hashes, dtype=np.int64)
    kept = np.asarray(kept, dtype=np.int64)
    negatives, labels = out[kept].copy(), wh[kept].copy()
    result = []
    for i in range(len(est)):
        negatives[-1], labels[-1] = out[i], wh[i]
        scores = negatives @ est[i] / (1e-8 + np.linalg.norm(negatives, axis=1))       # bm/losses.py get_scores
        probas = np.exp(scores - scores.max())
        probas /= probas.sum()
        vocab, inverse = np.unique(labels, return_inverse=True)
        probas_vocab = np.zeros(len(vocab))
        np.add.at(probas_vocab, inverse, probas)
        row = []
        for p_all, l_all in ((probas, labels), (probas_vocab, vocab)):
            match = l_all == wh[i]
            p = p_all[match].max()
            others = np.sort(p_all[~match])[::-1]
            if len(others) < topx:
                row.append((True, np.inf))
                continue
            q = others[topx - 1]
            row.append((bool(p > q), abs(p - q) / max(p, q)))
        result.append(row)
    return result


def assert_margins(estimates, outputs, word_hashes, kept, topx: int, what: str = ""):
    """Every verdict of the ranking is ``MARGIN`` away, relatively, from the other one: then an fp32 ranking whose
    probabilities are good to a hundredth of that counts the same hits.  Returns (wer, wer_vocab) in fp64."""
    margins = ranking_margins(estimates, outputs, word_hashes, kept, topx)
    worst = min(gap for row in margins for _, gap in row)
    assert worst >= MARGIN, f"{what}: a verdict of the ranking hangs on a relative gap of {worst}, below {MARGIN}"
    n = len(margins)
    return 1 - sum(row[0][0] for row in margins) / n, 1 - sum(row[1][0] for row in margins) / n


def fixture_batches(raw, meta, name):
    """The canned batches of case ``name`` of tests/golden/wer_epoch.npz: dicts of ``features`` [B, 3, T], ``keep`` [B]
    and -- unless the reference's assert fired -- the ``estimate`` / ``output`` the stand-in ``_process_batch`` returned
    for the kept rows (None for the fully rejected batch)."""
    sizes = meta["batches"]
    features, keep = raw[f"{name}/features"], raw[f"{name}/keep"]
    batches, at, kept_at = [], 0, 0
    for B in sizes:
        b = dict(features=features[at:at + B], keep=keep[at:at + B], estimate=None, output=None)
        m = int(b["keep"].sum())
        if m and f"{name}/estimate" in raw:
            b["estimate"] = raw[f"{name}/estimate"][kept_at:kept_at + m]
            b["output"] = raw[f"{name}/output"][kept_at:kept_at + m]
        batches.append(b)
        at, kept_at = at + B, kept_at + m
    return batches
