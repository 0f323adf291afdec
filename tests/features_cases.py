"""The per-window feature rules of csrc/features.hip restated in numpy / Python floats (bm/features/base.py:68-122,
238-267; bm/events.py:80-111; bm/features/audio.py:78-83, 211-274), held to the live reference by
tests/golden/features_builder.npz (test_features_cpu.py) and used as the truth beyond the fixture, plus the seeded random
event tables of the GPU tests.  Python's ``round`` and numpy's are half to even, as the reference's ``Frequency.to_ind``."""
import math

import numpy as np

F32 = np.float32


def nearest_source(k: int, L: int, n: int) -> int:
    """Source column of output column ``k`` when ``L`` columns are interpolated (nearest) to ``n``: torch's fp32 rule."""
    if L == n:
        return k
    return min(int(math.floor(F32(k) * (F32(L) / F32(n)))), L - 1)


def feature(name, rule, event_kind, dimension=1, cardinality=None, default_value=0.):
    return dict(name=name, rule=rule, event_kind=event_kind, dimension=dimension, cardinality=cardinality,
                default_value=default_value)


def make_builder(specs, sample_rate, event_mask=False):
    from brainmagick_amd.features import DeviceFeaturesBuilder, EventFeature
    return DeviceFeaturesBuilder([EventFeature(**s) for s in specs], sample_rate, event_mask=event_mask)


def overlap(ws, wstop, es, ed, sr):
    """(o0, o1, a, n) of an event against a window, or None when it is no candidate."""
    estop = es + ed
    if not (estop >= ws and es < wstop):
        return None
    o0 = max(ws, es)
    o1 = o0 + (min(wstop, estop) - o0)
    a = int(round(o0 * sr))
    return o0, o1, a, int(round(o1 * sr)) - a


def source_columns(rule, es, ed, o0, o1, n, L, sr):
    """The source column of every painted sample ``j < n`` of an array event of ``L`` columns."""
    if rule == "resampled":
        n_e = int(round(((es + ed) - es) * sr))
        first = min(max(0, -int(round((es - o0) * sr))), n_e - 1)
        return [nearest_source(min(first + j, n_e - 1), L, n_e) for j in range(n)]
    assert rule == "chunk"
    er = L / ed
    c0 = min(int(round((o0 - es) * er)), L - 1)
    c1 = min(max(c0 + 1, int(round((o1 - es) * er))), L)
    n_c = c1 - c0
    return [c0 + nearest_source(j, n_c, n) for j in range(n)]


def build_window(specs, event_mask, events, ws, wdur, sr, T):
    """``(data [F, T] fp32, mask [1, T] bool)`` of the window ``ws ... ws + wdur`` (seconds)."""
    ws, wdur, sr = float(ws), float(wdur), float(sr)
    F = sum(s["dimension"] for s in specs)
    data = np.zeros((F, T), dtype=np.float32)
    mask = np.zeros((1, T), dtype=bool) if event_mask else np.ones((1, T), dtype=bool)
    wstop = ws + wdur
    p0 = int(round(ws * sr))
    kinds = {s["event_kind"] for s in specs} | ({"word"} if event_mask else set())
    ch0 = 0
    slices = {}
    for s in specs:
        slices[s["name"]] = slice(ch0, ch0 + s["dimension"])
        data[slices[s["name"]]] = F32(s["default_value"])
        ch0 += s["dimension"]
    for kind in sorted(kinds):
        table = events.get(kind)
        if table is None:
            continue
        for e, (es, ed) in enumerate(zip(table["start"], table["duration"])):
            es, ed = float(es), float(ed)
            ov = overlap(ws, wstop, es, ed, sr)
            if ov is None or ov[3] < 1:
                continue
            o0, o1, a, n = ov
            w0 = a - p0
            assert 0 <= w0 and w0 + n <= T, (w0, n, T)
            for s in specs:
                if s["event_kind"] != kind:
                    continue
                if s["rule"] == "constant":
                    row = np.asarray(table[s["name"]], dtype=np.float64).reshape(len(table["start"]), -1)[e]
                    data[slices[s["name"]], w0:w0 + n] = row.astype(np.float32)[:, None]
                else:
                    src = np.asarray(table[s["name"]][e], dtype=np.float32).reshape(s["dimension"], -1)
                    cols = source_columns(s["rule"], es, ed, o0, o1, n, src.shape[1], sr)
                    data[slices[s["name"]], w0:w0 + n] = src[:, cols]
            if event_mask and kind == "word":
                mask[:, w0:w0 + n] = True
    return data, mask


_fixture = None


def fixture_cases():
    """tests/golden/features_builder.npz (made by tests/golden/make_features_golden.py from the live reference), read
    once: a list of cases ``{name, sample_rate, event_mask, specs, slices, dimension, output_dimension, events, windows:
    [{first, T, data, mask}]}``."""
    global _fixture
    if _fixture is None:
        import json
        from pathlib import Path
        z = np.load(Path(__file__).resolve().parent / "golden" / "features_builder.npz")
        cases = json.loads(str(z["meta"]))["cases"]
        for c in cases:
            name = c["name"]
            c["events"] = {}
            for kind, k in c["kinds"].items():
                ev = dict(start=z[f"{name}/{kind}/start"], duration=z[f"{name}/{kind}/duration"])
                for s in c["specs"]:
                    if s["event_kind"] != kind:
                        continue
                    if s["rule"] == "constant":
                        ev[s["name"]] = z[f"{name}/{kind}/{s['name']}"]
                    else:
                        ev[s["name"]] = [z[f"{name}/{kind}/{s['name']}/{e}"] for e in range(k["n"])]
                c["events"][kind] = ev
            seen = {}                                       # the windows of one length are stacked, in this order
            for w in c["windows"]:
                i = seen[w["T"]] = seen.get(w["T"], -1) + 1
                w["data"], w["mask"] = z[f"{name}/T{w['T']}/data"][i], z[f"{name}/T{w['T']}/mask"][i]
        _fixture = cases
    return _fixture


def window_times(first_sample: int, T: int, sr: float):
    """``(start, duration)`` in seconds of the window of ``T`` samples from ``first_sample`` (bm/dataset.py:323-344)."""
    start = first_sample / sr
    return start, (first_sample + T) / sr - start


def random_events(seed: int, sr: float, n_samples: int, n_words: int, n_sounds: int, dims):
    """A seeded event table over a recording of ``n_samples``: ``n_words`` word events (some overlapping, some of zero
    length, some on half samples), phonemes inside them, ``n_sounds`` sound events back to back with a mel-like array
    (``resampled``, near 2x the sample rate) and an embedding-like array (``chunk``, near 50 Hz).  ``dims``: channels of
    (word vector, mel, embedding)."""
    rng = np.random.default_rng(seed)
    total = n_samples / sr
    d_vec, d_mel, d_emb = dims
    events = {}
    if n_words:
        start = np.sort(rng.uniform(0, total, n_words))
        half = rng.random(n_words) < 0.3
        start[half] = (np.floor(start[half] * sr) + 0.5) / sr               # on a half sample
        start = np.sort(start)
        dur = rng.uniform(0.02, 0.6, n_words)
        dur[rng.random(n_words) < 0.1] = 0.0
        dur[rng.random(n_words) < 0.1] = 0.5 / sr
        events["word"] = dict(start=start, duration=dur, WordLength=rng.integers(1, 12, n_words).astype(np.float64),
                              WordVector=rng.standard_normal((n_words, d_vec)))
        ph_start = np.sort(rng.uniform(0, total, 3 * n_words))
        events["phoneme"] = dict(start=ph_start, duration=rng.uniform(0.01, 0.2, 3 * n_words),
                                 Phoneme=rng.integers(1, 40, 3 * n_words).astype(np.float64))
    if n_sounds:
        edges = np.sort(rng.uniform(0, total, n_sounds + 1))
        start, dur = edges[:-1], np.diff(edges) * rng.uniform(0.9, 1.05, n_sounds)   # gaps and overlaps
        dur = np.maximum(dur, 2.0 / sr)
        mel, emb = [], []
        for d in dur:
            n_e = int(round(d * sr))
            L = int(rng.choice([n_e, max(1, int(n_e * 2.08)), max(1, n_e // 2 + 1)]))
            mel.append(rng.standard_normal((d_mel, L)).astype(np.float32))
            L = max(1, int(round(d * rng.uniform(46, 50)))) if d >= 0.5 else max(1, int(d * 49))
            emb.append(rng.standard_normal((d_emb, L)).astype(np.float32))
        events["sound"] = dict(start=start, duration=dur, Mel=mel, Embedding=emb)
    return events


RANDOM_SPECS = lambda d_vec, d_mel, d_emb: [                                                    # noqa: E731
    feature("WordLength", "constant", "word"),
    feature("Mel", "resampled", "sound", d_mel, default_value=-5.0),
    feature("WordVector", "constant", "word", d_vec),
    feature("Phoneme", "constant", "phoneme", cardinality=40),
    feature("Embedding", "chunk", "sound", d_emb),
]
