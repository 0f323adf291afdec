"""The segment-level evaluation measured: ``hip_ops.segment_eval_labels``, ``hip_ops.first_occurrence`` (csrc/segment_eval.hip)
and ``retrieval.collect_segment_eval`` beside the reference's way of doing the same (scripts/run_eval_probs.py:27-158).
A stated baseline, not a target.

    python scripts/segment_eval_bench.py [--out profiles/segment_eval_vs_torch.txt] [--reps 5]

(a) The label launch at B = 256, T = 361, F_all = 121 with every fifth row rejected, beside the reference's way on the
    same batch: the Python loop of ``_get_extra_info`` over every word event of every segment that fills a [B, 2, T] host
    tensor (restated here without its two numpy string arrays, which only add to it), the column reads at check_at_time,
    and the ``torch.where`` chain of :116-130 on the device.  HIP events around 50 launches; a host clock around the
    reference's loop, which ends in a device synchronise.
(b) ``first_occurrence`` at N = 20 000 rows over 6 000 ids (two launches and the fill of the table; HIP events), beside
    the Python loop of :137-149: one string hash per row and a ``set`` (host clock; the ids come from a host list, as the
    reference has them after its ``.cpu()``).
(c) The collection over the 4 000 word windows of one recording (208 MEG channels, 120 mel channels + WordHash,
    paper-sized SimpleConv, batches of 256), beside the same loop with the reference's ``.cpu()`` of every prediction and
    output, its extra-info loop, its chain and its ``set`` -- and beside the loop that only runs ``_process_batch``.
    Host clock around the loop, which ends in a device synchronise.  The reference gets its ``_event_lists`` from the
    dataset's workers; here they are prepared outside the timed loop.

Everything is warmed up; the repetitions of the implementations alternate; medians are reported.  The measurement runs
in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

B, T, F_ALL, MEG, SR = 256, 361, 121, 208, 120.
WORDS = 4000
N_ROWS, N_IDS = 20_000, 6_000
CALLS = 50


def _median(v):
    return sorted(v)[len(v) // 2]


def _events(fn, calls):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _clock(fn, calls=1):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(impls, reps, timers, calls=1):
    import torch
    for fn in impls.values():
        fn()
        torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(timers[k](fn, calls) if timers[k] is _events else timers[k](fn))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), n=len(v)) for k, v in times.items()}


def extra_info(event_lists, wstart, n_times):
    """The loop of scripts/run_eval_probs.py:32-47 without its string arrays: [B, 2, T] on the host."""
    import torch
    data = torch.ones(len(event_lists), 2, n_times) * -1
    for k, events in enumerate(event_lists):
        start = wstart[k]
        for es, ed, word_index, sequence in events:
            a = SR * (es - start)
            b = a + SR * ed
            a, b = max(0, int(a)), min(n_times, int(b))
            data[k, 0, a:b] = word_index
            data[k, 1, a:b] = sequence
    return data


def reference_labels(features, channel, t0, reject_mask, event_lists, wstart):
    """:99-130: the extra-info loop, the reads at check_at_time and the chain (reach 1)."""
    import torch
    info = extra_info(event_lists, wstart, features.shape[-1])
    word_hash = features[:, channel:channel + 1][:, 0]
    keep = reject_mask.cpu()
    wh = word_hash[reject_mask][:, t0]
    wi = info[keep, 0][:, t0]
    si = info[keep, 1][:, t0]
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 - 1], wh)
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 + 1], wh)
    return wh, wi.long(), si.long()


def seen_loop(si, wi, seen):
    """:137-149: a string hash per row and a set."""
    hashes = [hash(f"{s}_{w}".encode()) for s, w in zip(si, wi)]
    mask = []
    for h in hashes:
        if h in seen:
            mask.append(False)
        else:
            seen.add(h)
            mask.append(True)
    return hashes, mask


def make_segments():
    import numpy as np
    import torch
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents, DeviceFeaturesBuilder, EventFeature
    from brainmagick_amd.synthetic import Recording
    builder = DeviceFeaturesBuilder([EventFeature("MelSpectrum", "resampled", "sound", 120, default_value=-5.0),
                                     EventFeature("WordHash", "constant", "word", cardinality=1001)], SR)
    rng = np.random.default_rng(7)
    g = torch.Generator().manual_seed(7)
    onset = 60 + 36 * np.arange(WORDS)                                      # a word every 0.3 s
    n = int(onset[-1]) + 320
    mel = torch.randn(120, n, generator=g)
    word = dict(start=onset / SR, duration=rng.integers(1, 30, WORDS) / SR,
                WordHash=rng.integers(1, 1001, WORDS).astype(np.float64),
                word_index=np.arange(WORDS) % 12, sequence_id=1 + (np.arange(WORDS) // 12) % 200)   # sentences repeat
    events = dict(sound=dict(start=np.array([0.0]), duration=np.array([n / SR]), MelSpectrum=[mel]), word=word)
    rec = DeviceRecording(torch.randn(MEG, n, generator=g).cuda(), events=DeviceEvents(builder, events),
                          recording=Recording(0, torch.rand(MEG, 2, generator=g)), subject_index=0)
    seg = DeviceSegments([rec], SR, tmin=-0.5, tmax=2.5, condition=onset / SR, meg_dimension=MEG)
    # what the reference's dataset hands over per window: the word events its selection admits (bm/features/base.py:80)
    stop = word["start"] + word["duration"]
    lists = []
    for ws, wd in zip(seg.wstart, seg.wdur):
        lo, hi = np.searchsorted(stop, ws, "left"), np.searchsorted(word["start"], ws + wd, "left")
        lists.append([(float(word["start"][e]), float(word["duration"][e]), int(word["word_index"][e]),
                       int(word["sequence_id"][e])) for e in range(lo, hi)])
    return seg, builder, lists


def measure(reps: int) -> dict:
    import numpy as np
    import torch
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd import retrieval
    from brainmagick_amd.dataset import DeviceSegmentLoader
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from oracle import bm_oracle as O
    out = dict(device=torch.cuda.get_device_name(0))
    res = {}
    seg, builder, lists = make_segments()
    t0 = retrieval.check_at_time(seg.tmin, SR)
    out.update(t0=t0, T=seg.T, n_collect=len(seg), events_per_window=sum(map(len, lists)) / len(lists))
    rows, n_ids = retrieval.dense_segment_ids([seg.recordings[0].events.word_info_host])
    infos = H.WordInfoTable(rows, n_ids, seg.device)
    events = seg.tables()[1]
    word_kind = builder.kinds.index("word")
    flag = retrieval.segment_eval_flag(seg.device)

    # (a) the label launch on the first batch of the epoch
    loader = DeviceSegmentLoader(seg, B)
    batch = next(iter(loader))
    arrays = loader.epoch_arrays
    x = batch.features
    keep = (torch.arange(B) % 5 != 0).cuda()
    n_keep = int(keep.sum())
    dest = torch.zeros(B, 7, dtype=torch.int64, device="cuda")
    wstart = seg.wstart[:B].tolist()

    def labels_ours():
        H.segment_eval_labels(x, 120, t0, keep, arrays, 0, events, word_kind, infos, SR, dest, 0, flag, count=n_keep)

    def labels_reference():
        res["ref"] = reference_labels(x, 120, t0, keep, lists[:B], wstart)
    out["labels"] = interleaved({"bm: segment_eval_labels (one launch)": labels_ours,
                                 "reference's way: extra-info loop on the host, reads, where chain": labels_reference},
                                reps, {"bm: segment_eval_labels (one launch)": _events,
                                       "reference's way: extra-info loop on the host, reads, where chain": _clock}, CALLS)
    got = dest[:n_keep].cpu()
    out["labels_equal"] = bool(torch.equal(got[:, 0], res["ref"][0].long().cpu()) and torch.equal(got[:, 1], res["ref"][1])
                               and torch.equal(got[:, 2], res["ref"][2]))
    out["n_keep"] = n_keep

    # (b) the first occurrences
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, N_IDS, (N_ROWS,), generator=g)
    ids_dev = ids.cuda()
    ids_host = ids.tolist()

    def first_ours():
        res["first"] = H.first_occurrence(ids_dev, N_IDS, flag)

    def first_reference():
        res["seen"] = seen_loop(ids_host, ids_host, set())
    out["first"] = interleaved({"bm: first_occurrence (fill + two launches)": first_ours,
                                "reference's way: a string hash per row and a set": first_reference}, reps,
                               {"bm: first_occurrence (fill + two launches)": _events,
                                "reference's way: a string hash per row and a set": _clock}, CALLS)
    out["first_equal"] = bool(res["first"][0].cpu().tolist() == res["seen"][1])

    # (c) the collection
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": MEG}, out_channels=120, hidden={"meg": 320}, n_subjects=1,
                       **dict(O.CLIP_CONV_CFG))
    solver = Solver(model, ClipLoss())
    for m in solver._all_models():
        m.train(False)
    names = ["MelSpectrum"]

    def collect_ours():
        preds, outputs, labels = retrieval.collect_segment_eval(solver, DeviceSegmentLoader(seg, B), len(seg), builder,
                                                                names, t0, infos)
        mask, _ = H.first_occurrence(labels[:, 3].contiguous(), n_ids, flag)
        retrieval.raise_if_segment_eval_error(seg.device)
        res["ours"] = (preds, outputs[mask], labels, mask)

    def collect_reference():
        preds, trues, cols, masks, seen = [], [], [], [], set()
        with torch.no_grad():
            for k, batch in enumerate(DeviceSegmentLoader(seg, B)):
                features = builder.extract_features(batch.features, names)
                estimate, output, _, reject_mask = solver._process_batch(batch.replace(features=features))
                lo = k * B
                wh, wi, si = reference_labels(batch.features, 120, t0, reject_mask, lists[lo:lo + len(batch)],
                                              seg.wstart[lo:lo + len(batch)].tolist())
                preds.append(estimate.cpu())
                _, mask = seen_loop(si.tolist(), wi.tolist(), seen)
                trues.append(output[mask].cpu())
                cols.append(torch.stack([wh.cpu().long(), wi, si], dim=1))
                masks.append(torch.tensor(mask))
        res["cpu"] = (torch.cat(preds), torch.cat(trues), torch.cat(cols), torch.cat(masks))

    def forward_only():
        with torch.no_grad():
            for batch in DeviceSegmentLoader(seg, B):
                features = builder.extract_features(batch.features, names)
                solver._process_batch(batch.replace(features=features))
    keys = ("bm: collect_segment_eval + first_occurrence (resident arrays)",
            "reference's way: .cpu() copies, extra-info loop, chain, set", "the loader and _process_batch alone")
    out["collect"] = interleaved(dict(zip(keys, (collect_ours, collect_reference, forward_only))), min(reps, 3),
                                 dict.fromkeys(keys, _clock))
    ours, cpu = res["ours"], res["cpu"]
    out["collect_equal"] = bool(torch.equal(ours[0].cpu(), cpu[0]) and torch.equal(ours[1].cpu(), cpu[1]) and
                                torch.equal(ours[2][:, :3].cpu(), cpu[2]) and torch.equal(ours[3].cpu(), cpu[3]))
    out["n_vocab"] = int(ours[3].sum())
    out["collect_bytes"] = int(cpu[0].numel() * 4 + cpu[1].numel() * 4)
    return out


def _row(label, v, width=70):
    return f"  {label:{width}s} {v['median_ms']:10.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]  n = {v['n']}"


def _versus(ours, base, what):
    return (f"  bm / {what}   x{ours / base:.3f}   "
            + (f"({what} takes {base / ours:.2f} times as long)" if ours <= base else f"(bm is SLOWER than {what})"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_eval_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps)))
        return
    cmd = ["timeout", "-k", "10", "500", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"segment_eval_bench: the measurement ended with status {proc.returncode}")
    r = json.loads(proc.stdout.strip().splitlines()[-1])
    l_ours, l_ref = (r["labels"][k]["median_ms"] for k in r["labels"])
    f_ours, f_ref = (r["first"][k]["median_ms"] for k in r["first"])
    c_ours, c_ref, c_fwd = (r["collect"][k]["median_ms"] for k in r["collect"])
    v_ours, _, v_fwd = r["collect"].values()
    fwd_spread = max(v_ours["max_ms"], v_fwd["max_ms"]) - min(v_ours["min_ms"], v_fwd["min_ms"])
    lines = [f"The segment-level evaluation's collection (scripts/run_eval_probs.py:27-158), {r['device']}: windows of "
             f"{r['T']} samples,", f"{MEG} MEG channels, {F_ALL} feature channels (120 mel + WordHash), batches of {B}, "
             f"check_at_time {r['t0']}, {r['events_per_window']:.1f} word events per window;",
             "SimpleConv of the paper's size (hidden 320), ClipLoss, no ScaleReject.  A baseline, not a target.",
             "Same device, implementations alternate, medians after warm-up [min .. max], milliseconds.", "",
             f"(a) The label launch, one batch ({r['n_keep']} of {B} rows kept); HIP events around {CALLS} launches, per "
             "launch; host clock and a synchronise", "    around the reference's loop:"]
    lines += [_row(name, v) for name, v in r["labels"].items()]
    lines += [_versus(l_ours, l_ref, "the reference's way"),
              f"  equal word hashes, word indices and sentences: {r['labels_equal']}.", "",
              f"(b) First occurrences of {N_ROWS} rows over {N_IDS} ids; HIP events around {CALLS} calls (the fill of the "
              "table and two launches), per call;", "    host clock around the Python loop:"]
    lines += [_row(name, v) for name, v in r["first"].items()]
    lines += [_versus(f_ours, f_ref, "the set loop"), f"  equal masks: {r['first_equal']}.", "",
              f"(c) The collection over {r['n_collect']} windows of one recording ({r['n_vocab']} distinct segments); host "
              "clock around the loop and a device synchronise:"]
    lines += [_row(name, v) for name, v in r["collect"].items()]
    lines += [_versus(c_ours, c_ref, "the reference's way"),
              f"  equal predictions, candidates, labels and masks: {r['collect_equal']}.  The reference's copies move "
              f"{r['collect_bytes'] / 1e6:.0f} MB to the host, each copy a synchronise, and its two Python loops run per "
              f"batch.  Here the median differs from the {c_fwd:.1f} ms of the loader and the forward passes alone by "
              f"{c_ours - c_fwd:+.1f} ms (" + ("inside" if abs(c_ours - c_fwd) <= fwd_spread else "outside")
              + f" the spread of the runs, {fwd_spread:.1f} ms): they bound it."]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
