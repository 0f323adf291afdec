"""The features builder measured: ONE ``bm_segment_features`` launch per batch beside the two ``bm_segment_gather``
launches over full-length arrays that it replaces, beside torch ops on the device, and inside the cfg2 training step.

    python scripts/features_builder_bench.py [--out profiles/features_builder_vs_gather.txt] [--reps 7]

Shape: two recordings of ``--samples`` samples at 120 Hz (default 200 000: 28 minutes each), sound events of 200 s back to
back, a word of 0.2 s every 0.31 s (the mask), a window every 3 s, tmin -0.5, tmax 2.5 (T = 361), batches of 256 in the
order of a seeded ``RandomSampler``.  Two builders: 120 mel channels (``resampled``, arrays at 125 Hz) and 1024 wav2vec
channels (``chunk``, arrays at 49.95 Hz), each with the word mask.

  ours     ``hip_ops.segment_features``: features [256, F, 361] and the mask in one launch.
  gathers  the parent's path for the same batch: ``hip_ops.segment_gather`` of [F, N] fp32 arrays at 120 Hz plus the
           gather of the [1, N] mask (random values: the time does not depend on them; the VALUES of this path differ
           from the reference's per-window rules, which is why the builder exists).
  torch    the same batch with torch ops on the device: a default fill, then per (recording, event) one advanced-indexing
           read of the event's array and one indexed assignment, and one for the mask; the index tensors are built
           outside the timed region from the rules of tests/features_cases.py.  Must equal ours bit for bit.
  step     the cfg2 training step (208 channels, F = 120, 27 subjects, batch 256, T = 361) with every batch built
           (MEG gather + features launch) inside the step, beside the same steps over batches built beforehand.

Everything is warmed up; a timed repetition is one epoch's whole batches bracketed by HIP events; the variants alternate;
medians of ``--reps`` are reported.  The measurement runs in ONE child process under a time limit; its exit status is
checked and a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SR, TMIN, TMAX, B = 120., -0.5, 2.5, 256
BUILDERS = {"mel": ("resampled", 120, 125.0, -5.0), "wav2vec": ("chunk", 1024, 49.95, 0.0)}
CFG2 = dict(C=208, F=120, S=27)


def _median(v):
    return sorted(v)[len(v) // 2]


def _stats(v):
    return dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v))


def _events(fn, n):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(n):
        fn(k)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def _host_events(name, n_samples, seed):
    """The event tables of one recording; the arrays are made on the device."""
    import numpy as np
    import torch
    rule, F, rate, _ = BUILDERS[name]
    total = n_samples / SR
    edges = np.arange(0.0, total, 200.0).tolist() + [total]
    start, dur = np.array(edges[:-1]), np.diff(edges)
    g = torch.Generator(device="cuda").manual_seed(seed)
    arrays = [torch.randn(F, max(1, int(d * rate)), device="cuda", generator=g) for d in dur]
    w_start = np.arange(0.05, total - 0.3, 0.31)
    return dict(sound=dict(start=start, duration=dur, **{name: arrays}),
                word=dict(start=w_start, duration=np.full(len(w_start), 0.2)))


def _dataset(name, n_samples, channels, seed, event_mask=True):
    import torch
    import features_cases as FC
    from brainmagick_amd import dataset as D
    from brainmagick_amd.features import DeviceEvents
    from brainmagick_amd.synthetic import Recording
    rule, F, _, default = BUILDERS[name]
    specs = [FC.feature(name, rule, "sound", F, default_value=default)]
    builder = FC.make_builder(specs, SR, event_mask=event_mask)
    g = torch.Generator(device="cuda").manual_seed(seed)
    lg = torch.Generator().manual_seed(seed + 1)
    recs, host = [], []
    for i, c in enumerate(channels):
        host.append(_host_events(name, n_samples, seed + 10 * i))
        meg = torch.randn(c, n_samples, device="cuda", generator=g)
        recs.append(D.DeviceRecording(meg, events=DeviceEvents(builder, host[-1]), recording=Recording(i, torch.rand(c, 2, generator=lg)),
                                      subject_index=i))
    return D.DeviceSegments(recs, SR, tmin=TMIN, tmax=TMAX, condition=3.0), specs, host


def _torch_plan(seg, specs, host, rec, start):
    """Index tensors of one batch for the torch variant: per (recording, sound event) the painted (segment, sample) pairs
    and their source columns; for the mask the painted pairs of the word events."""
    import numpy as np
    import torch
    import features_cases as FC
    T, rule, name = seg.T, specs[0]["rule"], specs[0]["name"]
    groups, mb, mt = {}, [], []
    for b, (r, s) in enumerate(zip(rec, start)):
        ws, wdur = FC.window_times(int(s), T, SR)
        p0 = int(round(ws * SR))
        owner = np.full(T, -1)
        sound = host[r]["sound"]
        for e, (es, ed) in enumerate(zip(sound["start"], sound["duration"])):
            ov = FC.overlap(ws, ws + wdur, float(es), float(ed), SR)
            if ov is not None and ov[3] >= 1:
                owner[ov[2] - p0:ov[2] - p0 + ov[3]] = e
        for e in np.unique(owner[owner >= 0]):
            es, ed = float(sound["start"][e]), float(sound["duration"][e])
            o0, o1, a, n = FC.overlap(ws, ws + wdur, es, ed, SR)
            cols = np.asarray(FC.source_columns(rule, es, ed, o0, o1, n, sound[name][e].shape[1], SR))
            t = np.arange(a - p0, a - p0 + n)
            keep = owner[t] == e
            gb, gt, gc = groups.setdefault((r, int(e)), ([], [], []))
            gb.append(np.full(keep.sum(), b)), gt.append(t[keep]), gc.append(cols[keep])
        word = host[r]["word"]
        lo = np.searchsorted(word["start"], ws - 1.0)
        for es, ed in zip(word["start"][lo:lo + 20], word["duration"][lo:lo + 20]):
            ov = FC.overlap(ws, ws + wdur, float(es), float(ed), SR)
            if ov is not None and ov[3] >= 1:
                mb.append(np.full(ov[3], b)), mt.append(np.arange(ov[2] - p0, ov[2] - p0 + ov[3]))
    dev = lambda parts: torch.from_numpy(np.concatenate(parts)).cuda()                      # noqa: E731
    return [(r, e, dev(gb), dev(gt), dev(gc)) for (r, e), (gb, gt, gc) in groups.items()], dev(mb), dev(mt)


def _torch_batch(seg, specs, host, plan):
    import torch
    groups, mb, mt = plan
    name = specs[0]["name"]
    feats = torch.full((B, seg.n_features, seg.T), specs[0]["default_value"], device="cuda")
    mask = torch.zeros(B, 1, seg.T, device="cuda", dtype=torch.bool)
    for r, e, gb, gt, gc in groups:
        feats[gb, :, gt] = host[r]["sound"][name][e][:, gc].t()
    mask[mb, 0, mt] = True
    return feats, mask


def _one_builder(name, n_samples, reps):
    import numpy as np
    import torch
    from brainmagick_amd import dataset as D
    from brainmagick_amd import hip_ops as H
    F = BUILDERS[name][1]
    seg, specs, host = _dataset(name, n_samples, (4, 4), 1)
    T = seg.T
    loader = D.DeviceSegmentLoader(seg, B, shuffle=True, generator=torch.Generator().manual_seed(0))
    order = loader.indices()
    nb = len(order) // B
    assert nb >= 4, "too few samples for an epoch of several batches"
    order = order[:nb * B]
    arrays = seg.upload(order)
    _, table, _ = seg.tables()
    flag = D.range_error_flag(seg.device)
    g = torch.Generator(device="cuda").manual_seed(5)
    full = [torch.randn(F, n_samples, device="cuda", generator=g) for _ in seg.recordings]
    full_mask = [torch.rand(1, n_samples, device="cuda", generator=g) < 0.6 for _ in seg.recordings]
    feat_t, mask_t = H.SegmentTable(full), H.SegmentTable(full_mask)
    ring = [None] * 3

    def keep(k, value):
        ring[k % 3] = value
    rec_h, start_h = seg.rec[order].reshape(nb, B), seg.start[order].reshape(nb, B)
    plans = [_torch_plan(seg, specs, host, rec_h[k].tolist(), start_h[k].tolist()) for k in range(nb)]
    impls = {
        "ours: features + mask (1 launch)": lambda k: keep(k, H.segment_features(table, arrays["rec"], arrays["wstart"],
                                                                                 arrays["wdur"], k * B, B, T, SR, flag)),
        "gathers: features + mask (2 launches)": lambda k: keep(k, (
            H.segment_gather(feat_t, arrays["rec"], arrays["start"], k * B, B, F, T, flag),
            H.segment_gather(mask_t, arrays["rec"], arrays["start"], k * B, B, 1, T, flag))),
        "torch ops: features + mask": lambda k: keep(k, _torch_batch(seg, specs, host, plans[k])),
    }
    same = True
    for k in range(nb):                                                  # agreement first (also the warm-up)
        ours = impls["ours: features + mask (1 launch)"](k) or ring[k % 3]
        tf, tm = _torch_batch(seg, specs, host, plans[k])
        same = same and torch.equal(ours[0].view(torch.int32), tf.view(torch.int32)) and torch.equal(ours[1], tm)
    for fn in impls.values():
        for k in range(nb):
            fn(k)
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for label, fn in impls.items():
            times[label].append(_events(fn, nb))
    assert int(flag.item()) == 0, "the range flag fired"
    events_bytes = sum(r.events.resident_bytes() for r in seg.recordings)
    arrays_bytes = sum(a.numel() * 4 for a in full) + sum(m.numel() for m in full_mask)
    out_bytes = B * F * T * 4 + B * T
    return dict(F=F, T=T, batches=nb, same=bool(same), times={k: _stats(v) for k, v in times.items()},
                resident_events=events_bytes, resident_arrays=arrays_bytes, out_bytes=out_bytes)


def _step(n_samples, reps):
    import torch
    from brainmagick_amd import dataset as D
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from oracle import bm_oracle as O
    c2 = CFG2
    seg, _, _ = _dataset("mel", n_samples, (c2["C"], c2["C"]), 2, event_mask=False)      # ClipLoss takes an all-true mask
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": c2["C"]}, out_channels=c2["F"], hidden={"meg": 320}, n_subjects=c2["S"],
                       **O.CLIP_CONV_CFG)
    solver = Solver(model, negatives="local")
    loader = D.DeviceSegmentLoader(seg, B, shuffle=True, generator=torch.Generator().manual_seed(1))
    order = loader.indices()
    nb = len(order) // B
    arrays = seg.upload(order[:nb * B])

    def built(k):
        return seg.gather(arrays, k * B, B)
    prebuilt = [built(k) for k in range(nb)]
    losses = [float(solver.train_step(prebuilt[k])) for k in range(3)]
    step = {"train_step over pre-built device batches": lambda k: solver.train_step(prebuilt[k]),
            "train_step, batch built (MEG gather + features launch) in the step": lambda k: solver.train_step(built(k))}
    times = {k: [] for k in step}
    for _ in range(reps):
        for label, fn in step.items():
            times[label].append(_events(fn, nb))
    solver.check_pending_flags()
    D.raise_if_range_error(seg.device)
    return dict(times={k: _stats(v) for k, v in times.items()}, batches=nb, losses=losses)


def measure(reps, n_samples):
    import torch
    from brainmagick_amd import hip_ops as H
    H.set_compute_dtype("f16x2")
    out = dict(device=torch.cuda.get_device_name(0), n_samples=n_samples)
    for name in BUILDERS:
        out[name] = _one_builder(name, n_samples, reps)
        torch.cuda.empty_cache()
    out["step"] = _step(n_samples, reps)
    return out


def _row(label, v, width=68):
    return f"  {label:{width}s} {v['median_ms']:9.4f}  [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "features_builder_vs_gather.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=200_000)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, args.samples)))
        return
    cmd = ["timeout", "-k", "10", "500", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps),
           "--samples", str(args.samples)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"features_builder_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    lines = [f"Features builder: 2 recordings of {res['n_samples']} samples at {SR:.0f} Hz on the {res['device']}, sound events "
             "of 200 s back to back,",
             f"a word every 0.31 s (the mask), windows of T = 361 every 3 s, batches of {B} in RandomSampler order.",
             "HIP events around one epoch's whole batches (the last three outputs are kept alive), variants alternating,",
             f"median of {args.reps} after warm-up [min .. max], milliseconds per batch.", ""]
    ok = True
    for name in BUILDERS:
        r = res[name]
        t = r["times"]
        ours, two = t["ours: features + mask (1 launch)"]["median_ms"], t["gathers: features + mask (2 launches)"]["median_ms"]
        tor = t["torch ops: features + mask"]["median_ms"]
        lines += [f"{name}: F = {r['F']} ({BUILDERS[name][0]}, arrays at {BUILDERS[name][2]} Hz), {r['batches']} batches, "
                  f"{r['out_bytes'] / 1e6:.1f} MB written per batch"]
        lines += [_row(k, v) for k, v in t.items()]
        lines += [f"  ours / the two gathers   x{ours / two:.3f}" + ("  (ours is SLOWER)" if ours > two else ""),
                  f"  ours / torch ops         x{ours / tor:.3f}" + ("  (ours is SLOWER)" if ours > tor else ""),
                  f"  ours writes {r['out_bytes'] / 1e9 / (ours / 1e3):.0f} GB/s",
                  f"  resident: events + arrays at their own rate {r['resident_events'] / 1e6:.1f} MB, full-length arrays at "
                  f"{SR:.0f} Hz {r['resident_arrays'] / 1e6:.1f} MB (x{r['resident_arrays'] / r['resident_events']:.2f})",
                  f"  ours and the torch ops bit-equal on every batch: {r['same']}", ""]
        ok = ok and r["same"]
    s = res["step"]["times"]
    pre = s["train_step over pre-built device batches"]
    inl = s["train_step, batch built (MEG gather + features launch) in the step"]
    lines += [f"cfg2 training step ({CFG2['C']} channels, F = {CFG2['F']} mel, {CFG2['S']} subjects, batch {B}, T = 361, f16x2), "
              f"HIP events around {res['step']['batches']} steps,",
              f"median of {args.reps} after 3 warm-up steps, alternating [min .. max], milliseconds per step:", ""]
    lines += [_row(k, v) for k, v in s.items()]
    lines += [f"  building the batch inside the step costs {1e3 * (inl['median_ms'] - pre['median_ms']):+.0f} us per step "
              f"(x{inl['median_ms'] / pre['median_ms']:.4f})",
              "  losses of the warm-up steps: " + ", ".join(f"{v:.5f}" for v in res["step"]["losses"])]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if not ok:
        raise SystemExit("features_builder_bench: the kernel and the torch ops disagree")


if __name__ == "__main__":
    main()
