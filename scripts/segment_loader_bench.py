"""The GPU-resident segment loader measured: ``bm_segment_gather`` beside torch ops on the device, beside the pinned
host -> device copy a perfect CPU loader would still cost, and inside the cfg2 training step.

    python scripts/segment_loader_bench.py [--out profiles/segment_loader_vs_torch.txt] [--reps 7]

Shape (the cfg5 mix): four recordings at 120 Hz -- two of 273 channels and two of 128, zero-padded to 273 -- of
``--samples`` samples each (default 200 000: 642 MB of MEG and 384 MB of features resident, beyond the 256 MiB Infinity
Cache), a window every 3 s, tmin -0.5, tmax 2.5 (T = 361), baseline (None, 0), F = 120, M = 1, batches of 256 in the
order of a seeded ``RandomSampler``.  An epoch's windows are disjoint, so every batch reads samples that no earlier batch
of the epoch read: the gather is timed from HBM.  The last three batches are kept alive, so the outputs rotate too.

  ours   ``DeviceSegments.gather``: three launches per batch; per tensor, the ``hip_ops.segment_gather`` call alone.
  (a)    the same batch with torch ops on the device, per recording: an index tensor (window starts + arange(T), built
         outside the timed region), advanced indexing, an fp64 ``mean`` of the baseline window, the subtraction in fp64,
         ``.float()``, ``F.pad`` to 273 channels and one indexed assignment into the batch's order.  Must equal ours within the
         bound of tests/test_segments_gpu.py.
  (b)    ``Solver.stage`` of the finished batch from pinned host memory (what the reference's loader ends with), to its
         completion on the copy stream.
  copy   a plain device-to-device ``copy_`` of 512 MB buffers (two pairs, alternating): the rate a memory-bound kernel can
         reach on this box.  "fraction" = (bytes read + bytes written of a variant, from the shapes) / time / that rate.
  step   the cfg2 training step (208 channels, F = 120, 27 subjects, batch 256, T = 361) with every batch gathered by
         the loader inside the step, beside the same steps over batches that were built before the clock started.

Everything is warmed up; a timed repetition is one epoch's eight batches bracketed by HIP events (host clock around a
synchronise for (b)); the variants alternate; medians of ``--reps`` are reported.  The measurement runs in ONE child process
under a time limit; its exit status is checked and a failure ends the run."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE = dict(channels=(273, 128, 273, 128), C=273, F=120, M=1, B=256, sample_rate=120., tmin=-0.5, tmax=2.5,
             baseline=(None, 0), condition=3.0, subjects=27)
CFG2 = dict(channels=(208, 208), C=208, F=120, B=256, S=27)


def _median(v):
    return sorted(v)[len(v) // 2]


def _stats(v):
    return dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v))


def _events(fn, n):
    """Milliseconds per call of ``fn(k)``, k = 0 .. n - 1, between two events on the current stream."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(n):
        fn(k)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def _dataset(channels, n_samples, F, gen_seed):
    import torch
    from brainmagick_amd import dataset as D
    from brainmagick_amd.synthetic import Recording
    d = SHAPE
    g = torch.Generator(device="cuda").manual_seed(gen_seed)
    lg = torch.Generator().manual_seed(gen_seed + 1)
    recs = []
    for i, c in enumerate(channels):
        meg = torch.randn(c, n_samples, device="cuda", generator=g) + 50. * torch.randn(c, 1, device="cuda", generator=g)
        feats = torch.randn(F, n_samples, device="cuda", generator=g)
        mask = torch.ones(1, n_samples, device="cuda", dtype=torch.bool)
        recs.append(D.DeviceRecording(meg, feats, mask, recording=Recording(i, torch.rand(c, 2, generator=lg)),
                                      subject_index=i % d["subjects"]))
    return D.DeviceSegments(recs, d["sample_rate"], tmin=d["tmin"], tmax=d["tmax"], baseline=d["baseline"],
                            condition=d["condition"], meg_dimension=max(channels))


def _torch_batch(seg, plan, B):
    """(a): the batch of ``plan`` = [(recording, window starts [n_r] (device), positions in the batch [n_r] (device))]."""
    import torch
    from torch.nn import functional as F
    T, (b0, b1) = seg.T, seg.baseline
    ar = plan["arange"]
    meg = torch.empty(B, seg.meg_dimension, T, device="cuda")
    feats = torch.empty(B, seg.n_features, T, device="cuda")
    mask = torch.empty(B, seg.n_mask, T, device="cuda", dtype=torch.bool)
    for r, starts, pos in plan["groups"]:
        rec = seg.recordings[r]
        idx = starts[:, None] + ar                                          # [n_r, T]
        w = rec.meg[:, idx].permute(1, 0, 2).double()                       # [n_r, C_r, T]
        w = (w - w[..., b0:b1 + 1].mean(-1, keepdim=True)).float()
        meg[pos] = F.pad(w, (0, 0, 0, seg.meg_dimension - w.shape[1]))
        feats[pos] = rec.features[:, idx].permute(1, 0, 2)
        mask[pos] = rec.features_mask[:, idx].permute(1, 0, 2)
    return meg, feats, mask


def measure(reps: int, n_samples: int) -> dict:
    import torch
    from brainmagick_amd import dataset as D
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.synthetic import SegmentBatch
    from oracle import bm_oracle as O
    d = SHAPE
    B = d["B"]
    H.set_compute_dtype("f16x2")
    seg = _dataset(d["channels"], n_samples, d["F"], 1)
    T = seg.T
    loader = D.DeviceSegmentLoader(seg, B, shuffle=True, generator=torch.Generator().manual_seed(0))
    order = loader.indices()
    nb = len(order) // B                                                    # whole batches of an epoch
    assert nb >= 4, "too few samples for an epoch of several batches"
    order = order[:nb * B]
    arrays = seg.upload(order)
    meg_t, feat_t, mask_t = seg.tables()
    flag = D.range_error_flag(seg.device)
    resident = sum(r.meg.numel() * 4 + r.features.numel() * 4 + r.features_mask.numel() for r in seg.recordings)
    out = dict(device=torch.cuda.get_device_name(0), T=T, batches=nb, segments=len(seg), resident_bytes=resident,
               n_samples=n_samples)

    # bytes from the shapes: what a batch reads (real channels only) and writes (padded)
    rec_h = seg.rec[order].reshape(nb, B)
    chan = torch.tensor([r.n_channels for r in seg.recordings])
    read_meg = float(chan[torch.from_numpy(rec_h).long()].sum()) / nb * T * 4
    nbytes = dict(meg=read_meg + B * d["C"] * T * 4, features=2 * B * d["F"] * T * 4, mask=2 * B * d["M"] * T)
    nbytes["batch"] = sum(nbytes.values())
    out["bytes"] = nbytes
    out["batch_out_bytes"] = B * (d["C"] + d["F"]) * T * 4 + B * d["M"] * T

    ring = [None] * 3

    def keep(k, value):
        ring[k % 3] = value

    plans = []
    ar = torch.arange(T, device="cuda")
    start_h = seg.start[order].reshape(nb, B)
    for k in range(nb):
        groups = []
        for r in range(len(seg.recordings)):
            pos = (rec_h[k] == r).nonzero()[0]
            groups.append((r, torch.from_numpy(start_h[k][pos]).cuda().long(), torch.from_numpy(pos).cuda()))
        plans.append(dict(arange=ar, groups=groups))

    impls = {
        "ours: batch (3 launches)": lambda k: keep(k, seg.gather(arrays, k * B, B)),
        "ours: meg": lambda k: keep(k, H.segment_gather(meg_t, arrays["rec"], arrays["start"], k * B, B, d["C"], T, flag,
                                                        baseline=seg.baseline)),
        "ours: features": lambda k: keep(k, H.segment_gather(feat_t, arrays["rec"], arrays["start"], k * B, B, d["F"], T,
                                                             flag)),
        "ours: mask": lambda k: keep(k, H.segment_gather(mask_t, arrays["rec"], arrays["start"], k * B, B, d["M"], T, flag)),
        "(a) torch ops: batch": lambda k: keep(k, _torch_batch(seg, plans[k], B)),
    }
    # agreement first (also the warm-up)
    ours = seg.gather(arrays, 0, B)
    tm, tf, tk = _torch_batch(seg, plans[0], B)
    rowmax = torch.stack([torch.nn.functional.pad(
        seg.recordings[int(r)].meg[:, int(s):int(s) + T].abs().amax(-1, keepdim=True), (0, 0, 0, d["C"] - int(chan[int(r)])))
        for r, s in zip(rec_h[0], start_h[0])]).double()
    bound = 2.0 ** -23 * tm.double().abs() + 2.0 ** -40 * rowmax + 2.0 ** -149      # both sides rounded once: an ulp
    out["same"] = bool(((ours.meg.double() - tm.double()).abs() <= bound).all()) and torch.equal(ours.features, tf) \
        and torch.equal(ours.features_mask, tk)
    out["meg_bit_equal_fraction"] = float((ours.meg.view(torch.int32) == tm.view(torch.int32)).double().mean())
    del ours, tm, tf, tk, rowmax, bound
    for fn in impls.values():
        for k in range(nb):
            fn(k)
    torch.cuda.synchronize()

    # the plain copy: two pairs of 512 MB buffers
    n_copy = 128 * 2 ** 20
    pairs = [(torch.empty(n_copy, device="cuda").normal_(), torch.empty(n_copy, device="cuda")) for _ in range(2)]
    impls["copy: 512 MB device to device"] = lambda k: pairs[k % 2][1].copy_(pairs[k % 2][0])
    for k in range(4):
        impls["copy: 512 MB device to device"](k)

    # (b) the pinned host -> device copy through Solver.stage
    torch.manual_seed(0)
    c2 = CFG2
    model = SimpleConv(in_channels={"meg": c2["C"]}, out_channels=c2["F"], hidden={"meg": 320}, n_subjects=c2["S"],
                       **O.CLIP_CONV_CFG)
    solver = Solver(model, negatives="local")
    hosts = [seg.gather(arrays, k * B, B).to("cpu").pin() for k in range(2)]

    def stage_all(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            keep(k, solver.stage(hosts[k % 2].replace()))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n
    stage_all(2)

    times = {k: [] for k in impls}
    times["(b) Solver.stage of the pinned batch"] = []
    for _ in range(reps):
        for name, fn in impls.items():
            times[name].append(_events(fn, nb))
        times["(b) Solver.stage of the pinned batch"].append(stage_all(nb))
    solver._staged.clear()
    raise_err = int(flag.item())
    assert raise_err == 0, "the range flag fired"
    out["times"] = {k: _stats(v) for k, v in times.items()}
    del pairs, hosts, ring[:], plans
    ring.extend([None] * 3)

    # the cfg2 step: loader batches gathered inside the step, beside batches built beforehand
    del seg, arrays, meg_t, feat_t, mask_t
    torch.cuda.empty_cache()
    seg2 = _dataset(c2["channels"], n_samples, c2["F"], 2)
    loader2 = D.DeviceSegmentLoader(seg2, B, shuffle=True, generator=torch.Generator().manual_seed(1))
    order2 = loader2.indices()
    nb2 = len(order2) // B
    arrays2 = seg2.upload(order2[:nb2 * B])
    prebuilt = [seg2.gather(arrays2, k * B, B) for k in range(nb2)]
    for b in prebuilt:
        b.meg.clamp_(-20, 20)
    losses = [float(solver.train_step(prebuilt[k])) for k in range(3)]            # warm-up

    def gathered(k):
        b = seg2.gather(arrays2, k * B, B)
        b.meg.clamp_(-20, 20)
        return b
    step = {"train_step over pre-built device batches": lambda k: solver.train_step(prebuilt[k]),
            "train_step, batch gathered by the loader in the step": lambda k: solver.train_step(gathered(k))}
    step_times = {k: [] for k in step}
    for _ in range(reps):
        for name, fn in step.items():
            step_times[name].append(_events(fn, nb2))
    solver.check_pending_flags()
    D.raise_if_range_error(seg2.device)
    out["step"] = {k: _stats(v) for k, v in step_times.items()}
    out["step_batches"] = nb2
    out["losses"] = losses
    return out


def _row(label, v, width=58):
    return f"  {label:{width}s} {v['median_ms']:9.4f}  [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_loader_vs_torch.txt"))
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
        raise SystemExit(f"segment_loader_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    d, t, nbytes = SHAPE, res["times"], res["bytes"]
    copy_ms = t["copy: 512 MB device to device"]["median_ms"]
    copy_rate = 2 * 4 * 128 * 2 ** 20 / 1e9 / (copy_ms / 1e3)                   # GB/s, read + write
    lines = [f"Segment loader: {len(d['channels'])} recordings of {d['channels']} channels x {res['n_samples']} samples "
             f"at {d['sample_rate']:.0f} Hz resident on the {res['device']}",
             f"({res['resident_bytes'] / 1e6:.0f} MB of MEG + features + mask: beyond the 256 MiB Infinity Cache), "
             f"{res['segments']} windows of T = {res['T']},",
             f"baseline {d['baseline']}, padded to {d['C']} channels, F = {d['F']}, M = {d['M']}, batches of {d['B']} in "
             f"RandomSampler order.",
             f"HIP events around one epoch's {res['batches']} batches (disjoint windows: every batch comes from HBM; the "
             "last three outputs are kept alive),",
             f"variants alternating, median of {args.reps} after warm-up [min .. max], milliseconds per batch.",
             f"Bytes per batch from the shapes (read + written): meg {nbytes['meg'] / 1e6:.1f} MB, features "
             f"{nbytes['features'] / 1e6:.1f} MB, mask {nbytes['mask'] / 1e6:.2f} MB.",
             f"Plain device copy on this box, same run: {copy_rate:.0f} GB/s (read + write).", ""]
    lines += [_row(k, v) for k, v in t.items()]
    ours, torch_ms = t["ours: batch (3 launches)"]["median_ms"], t["(a) torch ops: batch"]["median_ms"]
    stage_ms = t["(b) Solver.stage of the pinned batch"]["median_ms"]
    lines.append("")
    for key, label in (("batch", "ours: batch (3 launches)"), ("meg", "ours: meg"), ("features", "ours: features"),
                       ("mask", "ours: mask")):
        rate = nbytes[key] / 1e9 / (t[label]["median_ms"] / 1e3)
        lines.append(f"  {label:28s} {nbytes[key] / 1e6:8.2f} MB in {t[label]['median_ms']:.4f} ms = {rate:7.0f} GB/s = "
                     f"{rate / copy_rate:.2f} of the plain copy")
    lines += ["",
              f"  ours / (a) torch ops        x{ours / torch_ms:.3f}   "
              + (f"(the torch ops take {torch_ms / ours:.1f} times as long)" if ours <= torch_ms else "(ours is SLOWER)"),
              f"  ours / (b) pinned copy      x{ours / stage_ms:.3f}   "
              + (f"(the copy of the finished batch, {res['batch_out_bytes'] / 1e6:.0f} MB at "
                 f"{res['batch_out_bytes'] / 1e9 / (stage_ms / 1e3):.1f} GB/s, takes {stage_ms / ours:.1f} times as long)"
                 if ours <= stage_ms else "(ours is SLOWER)"),
              f"  ours and (a) agree within an ulp of the rounding + the reordering bound of the mean; features and mask "
              f"bit-equal: {res['same']}",
              f"  (MEG elements with the very same bits: {100 * res['meg_bit_equal_fraction']:.3f} %)"]
    s = res["step"]
    pre, inl = s["train_step over pre-built device batches"], s["train_step, batch gathered by the loader in the step"]
    lines += ["",
              f"cfg2 training step ({CFG2['C']} channels, F = {CFG2['F']}, {CFG2['S']} subjects, batch {CFG2['B']}, T = "
              f"{res['T']}, f16x2), HIP events around {res['step_batches']} steps,",
              f"median of {args.reps} after 3 warm-up steps, alternating [min .. max], milliseconds per step:", ""]
    lines += [_row(k, v) for k, v in s.items()]
    lines += [f"  the loader inside the step costs {1e3 * (inl['median_ms'] - pre['median_ms']):+.0f} us per step "
              f"(x{inl['median_ms'] / pre['median_ms']:.4f})",
              "  losses of the warm-up steps: " + ", ".join(f"{v:.5f}" for v in res["losses"])]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if not res["same"]:
        raise SystemExit("segment_loader_bench: the gather and the torch ops disagree")


if __name__ == "__main__":
    main()
