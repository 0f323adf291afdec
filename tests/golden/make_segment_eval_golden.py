"""Golden runs of the segment-level evaluation, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_segment_eval_golden.py [output directory]
Writes ``segment_eval.npz`` (default: next to this file).

``scripts/run_eval_probs.py`` cannot be imported (flashy, mne, pandas, omegaconf, bm.train), so the four functions
``_get_extra_info``, ``_load_test_data``, ``builds_probs`` and ``_get_accuracy_from_probs`` are taken from it by AST and
run, unmodified, against stubs (the pattern of make_wer_epoch_golden.py, whose stand-ins for the reference's ClipLoss and
FeaturesBuilder are reused):

  ``solver``         a namespace: ``args.dset`` (``tmin`` / ``test.tmin`` / ``sample_rate``), ``datasets.test.datasets``
                     (four stand-ins with ``recording.study_name()``, ``features`` and their canned windows),
                     ``make_loader`` (records the datasets it is handed and yields their windows in ConcatDataset order,
                     in batches of 7), ``_process_batch`` (the output IS the extracted features at the kept rows, the
                     estimate 0.35 x output + noise; the second batch of every case is fully rejected: ``None``)
  batches            ``features`` [B, 3, T] (WordLength, WordFrequency, WordHash), ``_event_lists``: per window the
                     window's own slice and then every word event the reference's selection admits (``_stop >= start``
                     and ``start < stop``, bm/features/base.py:80), in table order, plus a sound event it must skip
  ``hash``           bound in the executed namespace to a deterministic map into small integers (first come, first
                     numbered; far below 2^24), so nothing depends on PYTHONHASHSEED and the fp32 squeeze of
                     ``hash(word_sequence)`` loses nothing
  ``.cuda()`` / ``.cpu()``   copies (``Moved``); ``DataLoader`` / ``TensorDataset`` slice; ``flashy`` passes through

Word tables: per recording 20 windows, 40 samples apart, each with the events of one of ten scenarios laid around
``check_at_time``: an event containing t0, one before it, one after it, one that starts before the window and straddles
its start, two events covering t0 (the later one wins), a long event covering t0 followed by a later one that does not
(the earlier one wins: "last covering", not "last candidate"), an onset and an offset on an exact half sample (where
``int()`` and ``round`` differ), an event of no duration, and nothing at all.  Recordings 0 and 2 hear the same sentence
in their first ten windows and recording 1 repeats words of recording 0: duplicate segments across recordings and batches.

``CASES``: ``check_at_time`` 0, 1, 2, 6 and T - 2 = 11; ``n_recordings`` / ``test_study``; the word-hash channel from
tests/segment_eval_cases.py ``hash_rows`` (each of the three positions decides some row, asserted; one kept row of every
case is all zero, which is legal here).

Stored per case: the batches back to back (``features``, ``keep``, ``rec``, ``wstart``, ``subject``, ``recording``), the
``estimate`` / ``output`` of the kept rows, the word tables of the recordings (``sequence_id`` = the map's integer of the
sentence), and from the reference's run: ``word_hashes``, ``word_indices``, ``seq_indices``, ``subject_id``,
``recording_id``, the equality structure of ``segment_hashes`` (``segment_groups``: rank of first appearance; never a raw
hash), ``first_mask`` (verified against the reference's ``trues`` and ``trues_segment_hashes``), ``vocab_groups`` and
the hit counts of top-1, 5 and 10.

The maker asserts, in fp64, that every top-k verdict hangs on a relative gap of at least ``segment_eval_cases.MARGIN``
(100 x the relative tolerance of the retrieval scores in tests/test_kernels_gpu.py; the gap between the one candidate
that carries the row's segment and the k-th best other candidate), with no row left out, and that the numpy restatement
gives the reference's labels: under that condition the tests compare labels, masks, vocabularies and hit counts for
equality.  The seeds below meet it; a seed that does not fails the run.  This file holds none of the reference's text.
"""
import ast
import json
import sys
import types
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))
sys.path.insert(2, str(HERE.parent.parent))

import make_wer_epoch_golden as MW  # noqa: E402
import segment_eval_cases as SC  # noqa: E402

SAMPLE_RATE = 120.0
T = 13
STUDIES = ["alpha", "beta", "alpha", "alpha"]
WINDOWS = 20                                              # per recording
SPACING = 40                                              # samples between two windows' starts
BATCH = 7
TOPKS = (1, 5, 10)
NOISE = 2.0

CASES = {
    "t0_0": dict(tmin=2.5 / 120, test_tmin=None, names=["WordLength", "WordFrequency"], seed=31),
    "t0_1": dict(tmin=-1.0, test_tmin=1.5 / 120, names=["WordFrequency", "WordLength"], seed=32),
    "t0_2": dict(tmin=0.0, test_tmin=None, names=["WordLength", "WordFrequency"], seed=33),
    "t0_6": dict(tmin=-4.5 / 120, test_tmin=None, names=["WordLength", "WordFrequency"], seed=34,
                 test_study="alpha", n_recordings=2),
    "t0_11": dict(tmin=-9.5 / 120, test_tmin=None, names=["WordFrequency", "WordLength"], seed=35),
}


def scenario(kind: int, t0: int):
    """Word events of one window as (onset, offset) in samples relative to the window's start, in table order."""
    t = float(t0)
    return [
        [(t - 2.3, t + 3.1)],                             # contains t0
        [(t - 4.0, t - 0.5)],                             # before t0
        [(t + 1.2, t + 3.0)],                             # after t0
        [(-3.0, t + 1.5)],                                # starts before the window, straddles its start
        [(t - 3.0, t + 4.0), (t - 1.0, t + 2.0)],         # two cover t0: the later one wins
        [(t - 3.0, t + 4.0), (t + 1.0, t + 3.0)],         # the later one does not cover t0: the earlier one wins
        [(t + 0.5, t + 2.5)],                             # onset on a half sample: int() covers t0, round may not
        [(t - 2.0, t + 0.5)],                             # offset on a half sample: int() ends before t0
        [(t, t)],                                         # no duration
        [],                                               # no word at all
    ][kind]


def reference_functions():
    from _ref_import import REF
    path = REF / "scripts" / "run_eval_probs.py"
    tree = ast.parse(path.read_text())
    wanted = ("_get_extra_info", "_load_test_data", "builds_probs", "_get_accuracy_from_probs")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(f.name for f in fns) == sorted(wanted)
    code = compile(ast.Module(body=fns, type_ignores=[]), str(path), "exec")

    def bind(scope):
        exec(code, scope)
        return [scope[name] for name in wanted]
    return bind


class Moved(torch.Tensor):
    """A tensor whose ``.cuda()`` and ``.cpu()`` copy, as the reference's moves between host and GPU do."""

    def cuda(self, *args, **kwargs):
        return self.clone()

    def cpu(self, *args, **kwargs):
        return self.clone()


class HashMap:
    """``hash`` for the reference's functions: first come, first numbered."""

    def __init__(self):
        self.table = {}

    def __call__(self, value):
        assert isinstance(value, bytes)
        return self.table.setdefault(value, len(self.table) + 1)


def build_recordings(t0: int, rng, hashes: HashMap):
    """Per recording: the word table (start, duration, word_index, sequence, word) and the windows' first samples."""
    sentence_of = lambda r, j: ("sentence A" if j < 10 else "sentence C") if r == 2 else \
        "sentence A" if r == 0 else ("sentence A" if j % 3 == 0 else "sentence B") if r == 1 else "sentence D"   # noqa: E731
    recordings = []
    for r in range(len(STUDIES)):
        events, starts = [], []
        for j in range(WINDOWS):
            s = 5 + SPACING * j + r                           # first sample of the window
            starts.append(s)
            for i, (on, off) in enumerate(scenario((j + r) % 10, t0)):
                es = (s + on) / SAMPLE_RATE
                events.append(dict(start=es, duration=(s + off) / SAMPLE_RATE - es, word_index=2 * j + i,
                                   word_sequence=sentence_of(r, j), word=f"w{j}{i}"))
        assert all(a["start"] <= b["start"] for a, b in zip(events, events[1:]))
        for e in events:
            e["sequence_id"] = hashes(e["word_sequence"].encode())
        recordings.append(dict(events=events, starts=starts))
    return recordings


def run_case(name, bind, builder, clip_cls):
    from brainmagick_amd.synthetic import SegmentBatch
    spec = CASES[name]
    rng = np.random.default_rng(spec["seed"])
    tmin = spec["test_tmin"] if spec["test_tmin"] is not None else spec["tmin"]
    t0 = SC.check_at_time(tmin, SAMPLE_RATE)
    hashes = HashMap()
    recordings = build_recordings(t0, rng, hashes)
    tables = [(np.array([e["start"] for e in rec["events"]]), np.array([e["duration"] for e in rec["events"]]),
               np.array([[e["word_index"], e["sequence_id"]] for e in rec["events"]], dtype=np.int64))
              for rec in recordings]
    base = {}                                              # features of a segment: the same audio, the same features
    seen = dict(datasets=None, canned=[])
    by_id = {}

    def make_loader(dataset, shuffle=True, batch_size=None):
        assert shuffle is False and batch_size == BATCH
        seen["datasets"] = [d.index for d in dataset]
        rows = [(d.index, s) for d in dataset for s in recordings[d.index]["starts"]]
        batches = []
        for k, lo in enumerate(range(0, len(rows), BATCH)):
            chunk = rows[lo:lo + BATCH]
            B = len(chunk)
            rec = np.array([r for r, _ in chunk], dtype=np.int32)
            wstart = np.array([s / SAMPLE_RATE for _, s in chunk], dtype=np.float64)
            wdur = np.array([(s + T) / SAMPLE_RATE - s / SAMPLE_RATE for _, s in chunk])
            feats = np.zeros((B, 3, T), dtype=np.float32)
            zero_rows = (2,) if k == 2 else ()
            feats[:, 2] = SC.hash_rows(rng, B, T, t0, all_zero=zero_rows)
            event_lists = []
            for b, (r, s) in enumerate(chunk):
                start, dur, info = tables[r]
                e = SC.word_event(start, dur, wstart[b], SAMPLE_RATE, t0, T)
                key = (int(info[e, 1]), int(info[e, 0])) if e >= 0 else None
                if key not in base:
                    base[key] = rng.standard_normal((2, T)).astype(np.float32)
                feats[b, :2] = base[key]
                stop = wstart[b] + wdur[b]
                events = [types.SimpleNamespace(kind="slice", start=wstart[b], duration=wdur[b]),
                          types.SimpleNamespace(kind="sound", start=0.0, duration=100.0)]
                for ev in recordings[r]["events"]:
                    if ev["start"] + ev["duration"] >= wstart[b] and ev["start"] < stop:
                        events.append(types.SimpleNamespace(kind="word", **ev))
                event_lists.append(events)
            keep = np.ones(B, dtype=bool)
            if k == 0:
                keep[[0, B - 1]] = False
            elif k == 1:
                keep[:] = False                            # a fully rejected batch: _process_batch returns None
            elif k == 3:
                keep[3 % B] = False
            noise = NOISE * rng.standard_normal((int(keep.sum()), 2, T)).astype(np.float32)
            canned = dict(features=feats, keep=keep, noise=noise, rec=rec, wstart=wstart,
                          subject=np.array([10 + r for r, _ in chunk], dtype=np.int64),
                          recording=np.array([100 + r for r, _ in chunk], dtype=np.int64))
            people = [types.SimpleNamespace(study_name=lambda r=r: STUDIES[r], subject_uid=f"s{r}", recording_uid=f"r{r}")
                      for r, _ in chunk]
            batch = SegmentBatch(torch.zeros(B, 1, T), torch.from_numpy(feats.copy()), torch.ones(B, 1, T, dtype=torch.bool),
                                 torch.from_numpy(canned["subject"]), torch.from_numpy(canned["recording"]), people,
                                 event_lists)
            by_id[id(batch.meg)] = canned
            seen["canned"].append(canned)
            batches.append(batch)
        return batches

    def process_batch(batch):
        b = by_id[id(batch.meg)]
        keep = torch.from_numpy(b["keep"])
        if not b["keep"].any():
            return None, None, None, keep
        output = batch.features[keep].as_subclass(Moved)   # the extracted features, in the order asked for
        estimate = 0.35 * output + torch.from_numpy(b["noise"])
        b["estimate"], b["output"] = estimate.numpy().copy(), output.numpy().copy()
        return estimate, output, batch.features_mask[keep], keep

    datasets = [types.SimpleNamespace(index=i, features=builder, recording=types.SimpleNamespace(study_name=lambda s=s: s))
                for i, s in enumerate(STUDIES)]
    args = MW._Cfg(dset=MW._Cfg(tmin=spec["tmin"], sample_rate=SAMPLE_RATE, test=MW._Cfg(tmin=spec["test_tmin"])))
    solver = types.SimpleNamespace(args=args, datasets=types.SimpleNamespace(test=types.SimpleNamespace(datasets=datasets)),
                                   used_features=dict.fromkeys(spec["names"]), make_loader=make_loader,
                                   _process_batch=process_batch)
    quiet = types.SimpleNamespace(info=lambda *a, **k: None)
    progress = types.SimpleNamespace(LogProgressBar=lambda logger, iterable, **kw: iterable)

    def data_loader(dataset, batch_size):
        n = len(dataset[0])
        return [tuple(t[lo:lo + batch_size] for t in dataset) for lo in range(0, n, batch_size)]
    scope = dict(torch=torch, np=np, hash=hashes, flashy=types.SimpleNamespace(logging=progress), logger=quiet,
                 logging=quiet, defaultdict=defaultdict, ConcatDataset=lambda ds: list(ds), print=lambda *a, **k: None,
                 DataLoader=data_loader, TensorDataset=lambda *tensors: tensors)
    _, load_test_data, builds_probs, accuracy_from_probs = bind(scope)
    data = load_test_data(solver, batch_size=BATCH, n_recordings=spec.get("n_recordings"), shuffle=False,
                          test_study=spec.get("test_study"))
    canned = seen["canned"]
    assert not canned[1]["keep"].any() and "estimate" not in canned[1]
    n = int(sum(b["keep"].sum() for b in canned))
    assert all(len(data[k]) == n for k in ("preds", "segment_hashes", "word_hashes", "word_indices", "seq_indices",
                                           "subject_id", "recording_id", "word_strings", "word_segment_strings"))
    assert int(data["seq_indices"].abs().max()) < 2 ** 24 and int(data["word_hashes"].abs().max()) < 2 ** 24

    # the restatement gives the reference's labels; the dense ids have the equality structure of its segment hashes
    picked = seen["datasets"]
    rows, n_ids = SC.dense_ids([tables[r][2] if r in picked else None for r in range(len(STUDIES))])
    full = [None if rows[r] is None else (tables[r][0], tables[r][1], rows[r]) for r in range(len(STUDIES))]
    got, decided = [], set()
    for b in canned:
        lab, bits = SC.labels(b["features"][:, 2], t0, b["keep"], b["rec"], b["wstart"], b["subject"], b["recording"],
                              full, SAMPLE_RATE)
        assert bits == 0
        got.append(lab)
        decided.update(SC.decisive(b["features"][r, 2], t0) for r in np.flatnonzero(b["keep"]))
    got = np.concatenate(got)
    assert decided == {-1} | {k for k, t in enumerate(SC.positions(t0)) if t is not None}, (name, decided)
    for column, key in enumerate(("word_hashes", "word_indices", "seq_indices", None, "subject_id", "recording_id")):
        if key is not None:
            assert np.array_equal(got[:, column], data[key].numpy()), (name, key)
    segment_groups = SC.groups(data["segment_hashes"].numpy())
    assert np.array_equal(SC.groups(got[:, 3]), segment_groups), name
    no_word = data["word_indices"].numpy() == -1
    assert np.array_equal(got[:, 3] == 0, no_word) and np.array_equal(got[:, 6] == -1, no_word), name
    assert no_word.any() and (~no_word).sum() >= 8, (name, int((~no_word).sum()))
    words = data["word_strings"]
    for i in np.flatnonzero(~no_word):                     # word_event names the event the reference read the word from
        assert words[i] == recordings[int(got[i, 5]) - 100]["events"][int(got[i, 6])]["word"], (name, i)
    mask, first_row, bits = SC.first_occurrence(got[:, 3], n_ids)
    assert bits == 0 and (~mask).sum() >= 3, name
    outputs = np.concatenate([b["output"] for b in canned if "output" in b])
    estimates = np.concatenate([b["estimate"] for b in canned if "estimate" in b])
    assert np.array_equal(data["trues"].numpy(), outputs[mask]), name
    assert np.array_equal(data["trues_segment_hashes"].numpy(), data["segment_hashes"].numpy()[mask]), name
    assert np.array_equal(data["preds"].numpy(), estimates)
    vocab_groups = segment_groups[mask]
    assert len(vocab_groups) > max(TOPKS), (name, len(vocab_groups))
    rec_pairs = {r: set(map(tuple, got[got[:, 5] == 100 + r][:, 1:3].tolist())) - {(-1, -1)} for r in picked}
    assert any(rec_pairs[a] & rec_pairs[b] for a in picked for b in picked if a < b), "no segment shared by two recordings"

    # the ranking: the reference's own functions, and the fp64 margin of every verdict
    clip = clip_cls()
    probs = builds_probs(clip, data["preds"], data["trues"], None, batch_size=10)
    hits64 = SC.assert_margins(estimates, outputs[mask], segment_groups, vocab_groups, TOPKS, name)
    hits = {}
    for k in TOPKS:
        acc = accuracy_from_probs(probs, data["segment_hashes"], data["trues_segment_hashes"], topk=k)
        hits[k] = int(round(acc * n))
        assert abs(acc - hits64[k] / n) < 1e-6, (name, k, acc, hits64[k] / n)
    assert 0 < hits[1] < hits[10] < n, (name, hits)

    out = {f"{name}/{k}": np.concatenate([b[k] for b in canned])
           for k in ("features", "keep", "rec", "wstart", "subject", "recording")}
    out[f"{name}/estimate"], out[f"{name}/output"] = estimates, outputs
    for r in picked:
        out[f"{name}/r{r}/start"], out[f"{name}/r{r}/duration"] = tables[r][0], tables[r][1]
        out[f"{name}/r{r}/word_index"], out[f"{name}/r{r}/sequence_id"] = tables[r][2][:, 0], tables[r][2][:, 1]
    for key in ("word_hashes", "word_indices", "seq_indices", "subject_id", "recording_id"):
        out[f"{name}/{key}"] = data[key].numpy().astype(np.int64)
    out[f"{name}/segment_groups"], out[f"{name}/vocab_groups"] = segment_groups, vocab_groups
    out[f"{name}/first_mask"] = mask
    meta = dict(tmin=spec["tmin"], test_tmin=spec["test_tmin"], check_at_time=t0, names=spec["names"],
                n_recordings=spec.get("n_recordings"), test_study=spec.get("test_study"), datasets=picked,
                batches=[len(b["keep"]) for b in canned], n_kept=n, hits={str(k): hits[k] for k in TOPKS},
                n_vocab=int(len(vocab_groups)))
    return out, meta


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    torch.set_num_threads(1)
    torch.manual_seed(2036)
    bind, clip_cls, builder = reference_functions(), MW.reference_clip_loss(), MW.reference_builder()
    out, meta = {}, dict(source="scripts/run_eval_probs.py:27-180, 237-307", sample_rate=SAMPLE_RATE, T=T,
                         features=MW.FEATURES, params=MW.PARAMS, studies=STUDIES, n_recordings=len(STUDIES),
                         batch_size=BATCH, topks=list(TOPKS), margin=SC.MARGIN, cases={}, torch=torch.__version__)
    meta["cardinality"] = {f: builder[f].cardinality for f in MW.FEATURES}
    for name in CASES:
        arrays, case_meta = run_case(name, bind, builder, clip_cls)
        out.update(arrays)
        meta["cases"][name] = case_meta
    assert {c["check_at_time"] for c in meta["cases"].values()} == {0, 1, 2, 6, T - 2}
    assert any(c["datasets"] != [0, 1, 2, 3] for c in meta["cases"].values())
    out["meta"] = np.array(json.dumps(meta))
    path = dest / "segment_eval.npz"
    np.savez_compressed(path, **out)
    print(f"segment_eval: {len(meta['cases'])} cases, {path.stat().st_size} bytes -> {path}")
    print(json.dumps({k: {f: v.get(f) for f in ("check_at_time", "n_kept", "n_vocab", "hits", "datasets")}
                      for k, v in meta["cases"].items()}))


if __name__ == "__main__":
    main(sys.argv[1:])
