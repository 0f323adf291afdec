"""Golden windows of the features builder, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_features_golden.py [output directory]
Writes ``features_builder.npz`` (default: next to this file): inputs and the ``(data, mask)`` that the live
``FeaturesBuilder.__call__`` (bm/features/base.py:68-122) returns for windows of 13 and 87 samples at 120 Hz and 50 Hz.

The reference runs under stubs of its own here (``_ref_import.py`` is not touched): ``bm`` and ``bm.features`` are
skeleton packages so that neither ``__init__`` runs; ``mne``, ``torchaudio`` (with ``transforms.MelSpectrogram``),
``julius``, ``wordfreq.zipf_frequency``, ``dora``, ``omegaconf``, ``transformers``, ``spacy``, ``Levenshtein`` and
``bm.lib.pitch_calc.yin`` are empty stand-ins; ``bm.cache`` is a pass-through; ``MelSpectrum._compute`` and
``_BaseWav2Vec._compute_hidden_states`` return the arrays of this file, looked up by the name of the event's (never
opened) ``MOCK_CACHE`` file.  ``bm.utils``, ``bm.events``, ``bm.features.base`` / ``basic`` / ``audio`` are the
reference's own files, unmodified.  Two feature classes are declared here on the reference's ``Feature`` /
``Wav2VecConvolution`` bases: a 3-channel word vector (``get`` returns a 1-D tensor) and a 2-channel
``Wav2VecConvolution`` (a subclass that only changes ``dimension``); MelSpectrum runs with ``n_mels=3``.  The channel
counts keep the fixture small -- the painting rules are the reference's.  This file holds none of the reference's text.

The inputs are chosen so that the reference raises nothing; any exception of the reference ends the run.  The coverage
the fixture is meant to have is asserted at the end (with the index rules of tests/features_cases.py).
"""
import hashlib
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference")

import features_cases as FC  # noqa: E402

ARRAYS = {}                 # file name of a sound event -> {"mel": [D, L] fp32, "emb": [D, L] fp32}


def load_reference():
    if not REF.exists():
        raise RuntimeError("/root/reference not available: the fixture can only be regenerated in the build container")

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    stub("mne")
    stub("julius")
    stub("spacy")
    stub("Levenshtein")
    stub("transformers")
    stub("torchaudio", transforms=types.SimpleNamespace(MelSpectrogram=lambda **kw: None), info=None)
    stub("wordfreq", zipf_frequency=lambda word, language: float(int(hashlib.md5(word.encode()).hexdigest(), 16) % 7919) / 1000.)
    stub("dora", to_absolute_path=lambda p: p, log=stub("dora.log", LogProgress=object))
    stub("omegaconf", OmegaConf=object, basecontainer=stub("omegaconf.basecontainer", BaseContainer=object))

    class PassThrough:
        def __init__(self, *args, **kwargs):
            pass

        def get(self, _computation, *args, **kwargs):
            return _computation(*args, **kwargs)

    bm = stub("bm")
    bm.__path__ = [str(REF / "bm")]                  # submodules are found, bm/__init__.py does not run
    stub("bm.cache", Cache=PassThrough, MemoryCache=PassThrough)
    stub("bm.lib.pitch_calc")
    stub("bm.lib.pitch_calc.yin", compute_yin=None)
    feats = stub("bm.features")
    feats.__path__ = [str(REF / "bm" / "features")]
    import importlib
    base = importlib.import_module("bm.features.base")
    basic = importlib.import_module("bm.features.basic")
    audio = importlib.import_module("bm.features.audio")
    utils = importlib.import_module("bm.utils")

    audio.MelSpectrum._compute = lambda self, filepath, start, stop: torch.from_numpy(ARRAYS[Path(filepath).name]["mel"])
    audio._BaseWav2Vec._compute_hidden_states = \
        lambda self, name, filepath, start, stop, layers=None: np.ascontiguousarray(ARRAYS[Path(filepath).name]["emb"].T)[None]

    class WordVector(base.Feature):
        event_kind = "word"
        dimension = 3

        def get(self, event):
            return torch.tensor(WORD_VECTORS[event.word], dtype=torch.float32)

    class Embedding(audio.Wav2VecConvolution):
        event_kind = "sound"
        dimension = 2

    return base, basic, audio, utils


WORDS = ["a", "the", "brain", "magick", "of", "window", "hertz", "segment", "feature", "x", "gather", "oracle"]
WORD_VECTORS = {w: [float(len(w)) + 0.1, -1.0 / (i + 3), 1e-3 * (i * i - 7)] for i, w in enumerate(WORDS)}


def word_table(sr, rng):
    """Words laid out in samples of ``sr``: before / after / straddling windows, half-sample times, zero-length and
    sub-sample events, overlapping events (the later wins), one event longer than a window, a long gap."""
    start, dur = [], []

    def add(s, d):
        start.append(s / sr)
        dur.append(d / sr)

    add(2.0, 5.0)
    add(4.5, 6.0)                    # half-sample start, overlaps the first
    add(6.5, 2.0)                    # inside the second: the later one wins
    add(13.5, 0.0)                   # zero length
    add(14.2, 0.2)                   # rounds to 0 samples
    add(15.5, 1.0)                   # half to even at both ends
    add(16.5, 1.0)
    add(20.0, 40.0)                  # contains a whole window of 13
    add(22.25, 3.5)                  # inside it
    add(61.0, 2.5)
    add(63.5, 2.5)
    # a gap without events: 66 ... 200
    add(200.0, 130.0)                # contains a whole window of 87
    add(210.5, 7.0)
    add(215.0, 7.0)
    for s in np.sort(rng.uniform(330, 520, 24)):
        add(float(s), float(rng.uniform(0.3, 9.0)))
    order = np.argsort(np.asarray(start), kind="stable")
    start, dur = np.asarray(start)[order], np.asarray(dur)[order]
    n = len(start)
    words = [WORDS[int(i)] for i in rng.integers(0, len(WORDS), n)]
    return dict(start=start, duration=dur, word=words, word_index=[int(i) for i in rng.integers(0, 9, n)],
                modality=["audio" if i % 3 else "visual" for i in range(n)])


def phoneme_table(sr, rng, n=60):
    start = np.sort(rng.uniform(0, 520, n)) / sr
    return dict(start=start, duration=rng.uniform(0.2, 6.0, n) / sr, phoneme_id=[int(i) for i in rng.integers(0, 30, n)])


def sound_table(sr, rng, d_mel, d_emb, tag, long_events):
    """Sound events in seconds: two back to back (of more than two minutes with ``long_events``; cut at both ends by the
    windows), a short one (< 0.5 s), one whose end lies half a sample inside a window (the chunk's c0 clamps to L - 1)
    and mel arrays whose length equals, exceeds and is below the event's own length."""
    a, b = (130.0, 125.0) if long_events else (3.0, 2.5)
    t = 1.0 + 0.25 / sr
    spec = [(t, a + 0.4 / sr, "above"), (t + a + 0.5, b, "equal"), (t + a + b + 1.0, 0.3, "below"),
            (round(t + a + b + 2.0) + 0.55 / sr, 6.0 + 1.0 / sr, "above"),      # ends 0.55 samples into a window
            (round(t + a + b + 9.0) + 0.0, 2.0 + 0.45 / sr, "below")]
    start = np.array([s for s, _, _ in spec])
    dur = np.array([d for _, d, _ in spec])
    files = []
    for e, (s, d, how) in enumerate(spec):
        n_e = int(round(((s + d) - s) * sr))
        L_mel = {"equal": n_e, "above": int(n_e * 1.04) + 3, "below": max(1, int(n_e * 0.96) - 2)}[how]
        L_emb = max(1, int(round(d * (43.0 if e == 3 else 47.0)))) if d >= 0.5 else 14
        name = f"{tag}_sound{e}.wav"
        emb = rng.standard_normal((d_emb, L_emb)).astype(np.float32)
        if L_emb > 1000:        # minutes of embedding: every column its own value (its index), which also compresses
            emb = (np.arange(L_emb, dtype=np.float32)[None] + 0.25 * np.arange(1, d_emb + 1, dtype=np.float32)[:, None])
        ARRAYS[name] = dict(mel=rng.standard_normal((d_mel, L_mel)).astype(np.float32), emb=emb)
        files.append(name)
    return dict(start=start, duration=dur, file=files)


def frame_of(tables):
    import pandas as pd
    rows = []
    for kind, t in tables.items():
        for e in range(len(t["start"])):
            row = dict(kind=kind, start=float(t["start"][e]), duration=float(t["duration"][e]), language="en",
                       modality="audio")
            if kind == "word":
                row.update(word=t["word"][e], word_index=t["word_index"][e], word_sequence="", modality=t["modality"][e])
            elif kind == "phoneme":
                row.update(phoneme_id=t["phoneme_id"][e])
            else:
                row.update(filepath=f"MOCK_CACHE/{t['file'][e]}", offset=0.0)
            rows.append(row)
    frame = pd.DataFrame(rows)
    return frame.sort_values("start", kind="stable", ignore_index=True)


def windows_of(tables, sr, T, limit):
    """First samples of the windows: a stride over the busy part, and windows around every event edge."""
    firsts = set(range(0, 120, 5 if T == 13 else 17))
    for t in tables.values():
        for s, d in zip(t["start"], t["duration"]):
            for edge in (s, s + d):
                k = int(round(edge * sr))
                firsts.update((k - T, k - T + 1, k - T // 2, k - 1, k, k + 1))
    firsts = sorted(f for f in firsts if 0 <= f)
    if len(firsts) > limit:                                     # thin evenly, keep the ends
        keep = np.unique(np.linspace(0, len(firsts) - 1, limit).astype(int))
        firsts = [firsts[i] for i in keep]
    return firsts


def run_case(ref, name, sr, features, params, event_mask, tables, specs, out, meta, limit=100):
    base, basic, audio, utils = ref
    rate = utils.Frequency(sr)
    builder = base.FeaturesBuilder(frame_of(tables), features, params, rate, event_mask=event_mask)
    assert [f.name for f in builder.values()] == [s["name"] for s in specs]
    for f, s in zip(builder.values(), specs):
        assert (f.dimension, f.cardinality, f.event_kind) == (s["dimension"], s["cardinality"], s["event_kind"]), s
        assert abs(float(f.default_value) - s["default_value"]) == 0.0, s
    case = dict(name=name, sample_rate=sr, event_mask=event_mask, specs=specs, dimension=builder.dimension,
                output_dimension=builder.output_dimension,
                slices={f: [builder.get_slice(f).start, builder.get_slice(f).stop, builder.get_slice(f, True).start,
                            builder.get_slice(f, True).stop] for f in features},
                kinds={}, windows=[])
    events = {}
    for kind, t in tables.items():
        n = len(t["start"])
        ev = dict(start=np.asarray(t["start"], dtype=np.float64), duration=np.asarray(t["duration"], dtype=np.float64))
        case["kinds"][kind] = dict(n=n, arrays=[s["name"] for s in specs if s["event_kind"] == kind and s["rule"] != "constant"])
        for s in specs:
            if s["event_kind"] != kind:
                continue
            feature = builder[s["name"]]
            if s["rule"] == "constant":                          # the reference's own Feature.get, event by event
                frame = frame_of({kind: t})
                vals = [feature.get(event) for event in frame.event.iter()]
                ev[s["name"]] = np.array([np.asarray(v, dtype=np.float64).reshape(-1) for v in vals], dtype=np.float64)
            else:
                ev[s["name"]] = [ARRAYS[f]["mel" if s["rule"] == "resampled" else "emb"] for f in t["file"]]
        events[kind] = ev
        out[f"{name}/{kind}/start"], out[f"{name}/{kind}/duration"] = ev["start"], ev["duration"]
        for s in specs:
            if s["event_kind"] != kind:
                continue
            if s["rule"] == "constant":
                out[f"{name}/{kind}/{s['name']}"] = ev[s["name"]]
            else:
                for e, a in enumerate(ev[s["name"]]):
                    out[f"{name}/{kind}/{s['name']}/{e}"] = a
    stats = dict(empty=0, contained=0, zero=0, later_wins=0, pad=0, clamp=0, cut_left=0, cut_right=0)
    stacked = {}
    for T in (13, 87):
        for first in windows_of(tables, sr, T, limit if T == 13 else limit // 4):
            start, stop = rate.to_sec(first), rate.to_sec(first + T)          # bm/dataset.py:323-333
            data, mask, _ = builder(start, stop)
            assert data.shape == (builder.dimension, T) and mask.shape == (1, T) and mask.dtype == torch.bool, data.shape
            case["windows"].append(dict(first=first, T=T))
            stacked.setdefault(T, ([], []))
            stacked[T][0].append(data.numpy()), stacked[T][1].append(mask.numpy())
            coverage(stats, specs, events, start, stop - start, sr, T)
    for T, (data, mask) in stacked.items():                     # the windows of one length, in the order of case["windows"]
        out[f"{name}/T{T}/data"], out[f"{name}/T{T}/mask"] = np.stack(data), np.stack(mask)
    meta["cases"].append(case)
    return stats


def coverage(stats, specs, events, ws, wdur, sr, T):
    wstop = ws + wdur
    painted_any = False
    for kind, ev in events.items():
        painted = np.zeros(T, dtype=int)
        for e, (es, ed) in enumerate(zip(ev["start"], ev["duration"])):
            ov = FC.overlap(ws, wstop, float(es), float(ed), sr)
            if ov is None:
                continue
            o0, o1, a, n = ov
            if n < 1:
                stats["zero"] += 1
                continue
            w0 = a - int(round(ws * sr))
            stats["later_wins"] += int(painted[w0:w0 + n].any())
            painted[w0:w0 + n] = 1
            stats["contained"] += int(n == T)
            stats["cut_left"] += int(es < ws and n < T)
            stats["cut_right"] += int(es + ed > wstop and n < T)
            for s in specs:
                if s["event_kind"] != kind or s["rule"] == "constant":
                    continue
                L = np.shape(ev[s["name"]][e])[-1]
                if s["rule"] == "resampled":
                    n_e = int(round(((es + ed) - es) * sr))
                    first = min(max(0, -int(round((es - o0) * sr))), n_e - 1)
                    assert first + n <= n_e + 1
                    stats["pad"] += int(first + n == n_e + 1)
                else:
                    stats["clamp"] += int(int(round((o0 - es) * (L / ed))) >= L)
        painted_any = painted_any or painted.any()
    stats["empty"] += int(not painted_any)


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    ref = load_reference()
    F = FC.feature
    out, meta, stats = {}, dict(source="bm/features/base.py:68-122", cases=[]), {}
    for sr in (120.0, 50.0):
        tag = f"sr{int(sr)}"
        rng = np.random.default_rng(int(sr))
        words, phonemes = word_table(sr, rng), phoneme_table(sr, rng)
        sounds = sound_table(sr, rng, 3, 2, tag, False)
        long_sounds = sound_table(sr, rng, 3, 2, tag + "_long", True)
        n_ph = len(ref[1].ph_dict) + 1 if hasattr(ref[1], "ph_dict") else None
        stats[f"words_{tag}"] = run_case(
            ref, f"words_{tag}", sr, ["WordLength", "WordFrequency", "Phoneme", "WordIndex"], {}, True,
            dict(word=words, phoneme=phonemes),
            [F("WordLength", "constant", "word"), F("WordFrequency", "constant", "word"),
             F("Phoneme", "constant", "phoneme", cardinality=n_ph), F("WordIndex", "constant", "word")], out, meta, limit=60)
        stats[f"vector_{tag}"] = run_case(
            ref, f"vector_{tag}", sr, ["WordVector", "Modality"], {}, False, dict(word=words),
            [F("WordVector", "constant", "word", 3), F("Modality", "constant", "word", cardinality=3)], out, meta, limit=30)
        stats[f"mel_{tag}"] = run_case(
            ref, f"mel_{tag}", sr, ["MelSpectrum"], dict(MelSpectrum=dict(n_mels=3)), False, dict(sound=sounds),
            [F("MelSpectrum", "resampled", "sound", 3, default_value=-5.0)], out, meta)
        stats[f"wav2vec_{tag}"] = run_case(
            ref, f"wav2vec_{tag}", sr, ["Embedding"], {}, False, dict(sound=long_sounds),
            [F("Embedding", "chunk", "sound", 2)], out, meta)
        stats[f"mixed_{tag}"] = run_case(
            ref, f"mixed_{tag}", sr, ["Embedding", "WordLength", "MelSpectrum"], dict(MelSpectrum=dict(n_mels=3)), True,
            dict(word=words, sound=sounds),
            [F("Embedding", "chunk", "sound", 2), F("WordLength", "constant", "word"),
             F("MelSpectrum", "resampled", "sound", 3, default_value=-5.0)], out, meta, limit=30)
    for tag in ("sr120", "sr50"):
        w, m, v = stats[f"words_{tag}"], stats[f"mel_{tag}"], stats[f"wav2vec_{tag}"]
        assert min(w["empty"], w["contained"], w["zero"], w["later_wins"], w["cut_left"], w["cut_right"]) > 0, (tag, w)
        assert m["pad"] > 0 and m["cut_left"] > 0 and m["cut_right"] > 0, (tag, m)
        assert v["clamp"] > 0 and v["cut_left"] > 0 and v["cut_right"] > 0 and v["contained"] > 0, (tag, v)
    out["meta"] = np.array(json.dumps(meta))
    path = dest / "features_builder.npz"
    np.savez_compressed(path, **out)
    n_windows = sum(len(c["windows"]) for c in meta["cases"])
    print(f"features_builder: {len(meta['cases'])} cases, {n_windows} windows, {path.stat().st_size} bytes -> {path}")
    print(json.dumps(stats, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
