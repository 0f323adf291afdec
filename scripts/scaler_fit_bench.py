"""Fitting the robust MEG scaler of one recording: the radix select (csrc/scaler_fit.hip) beside the reference's algorithm
on the same device, interleaved.

    python scripts/scaler_fit_bench.py [--out profiles/scaler_fit_vs_torch.txt] [--reps 7]

Workload: one recording of 208 segments x 273 sensors x 360 samples (81.8 MB), seeded.  ``ours`` is the MEG part of
``DeviceBatchScaler.fit`` with its read-back (one [C, 3] tensor); ``select only`` is the ``bm_quantile_select`` call
without the read-back, for the achieved bytes/s against the bytes the algorithm has to read once.  The baseline is the
reference's ``RobustScaler(device="cuda").fit`` restated (bm/norm.py:58-80): the [N T, C] view of the same device
tensor, per column ``sort`` and three ``.item()``.  Every implementation is warmed up, the timed repetitions alternate,
each is bracketed by HIP events on the stream (both ends of ``ours`` and of the baseline are host-synchronous
anyway: they end in a read-back), and the median is reported.  Both must give the same tables.

The measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE = dict(N=208, C=273, T=360)
CPU_REFERENCE_SECONDS = 3.5          # the reference's RobustScaler().fit of this shape on a CPU container


def _median(v):
    return sorted(v)[len(v) // 2]


def measure(reps: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.norm import DeviceBatchScaler, QUANTILES
    from brainmagick_amd.synthetic import make_batch
    s = SHAPE
    batch = make_batch(s["N"], s["C"], s["T"], 4, 2, seed=3).to("cuda")
    batch = batch.replace(recording_index=torch.zeros_like(batch.recording_index))
    meg = batch.meg.contiguous()
    n = s["N"] * s["T"]
    ranks = [int(q * n) for q in QUANTILES]
    result = {}

    def ours():
        scaler = DeviceBatchScaler.fit([[batch]], None, n_samples_per_recording=s["N"])
        result["ours"] = (scaler.meg_center[0].cpu(), scaler.meg_scale[0].cpu())

    def select_only():
        H.quantile_select(meg, ranks)

    def torch_loop():
        X = meg.permute(0, 2, 1).reshape(-1, s["C"])
        center, scale = torch.empty(s["C"]), torch.empty(s["C"])
        for d in range(s["C"]):
            col, _ = X[:, d].sort()
            low, med, high = [col[int(q * len(col))].item() for q in QUANTILES]
            scale[d] = high - low
            center[d] = med
            if scale[d] == 0:
                scale[d] = 1
        result["torch"] = (center, scale)

    impls = {"ours (fit, with read-back)": ours, "select only (no read-back)": select_only,
             "torch sort loop (reference)": torch_loop}
    times = {k: [] for k in impls}
    for fn in impls.values():                       # warm-up: code objects, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):                           # interleaved
        for k, fn in impls.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times[k].append(start.elapsed_time(end))
    same = all(torch.equal(a, b) for a, b in zip(result["ours"], result["torch"]))
    return dict(times={k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()},
                same_tables=same, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scaler_fit_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps)))
        return
    cmd = ["timeout", "-k", "10", "420", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"scaler_fit_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    s = SHAPE
    nbytes = s["N"] * s["C"] * s["T"] * 4
    t = res["times"]
    ours, sel, base = (t[k]["median_ms"] for k in ("ours (fit, with read-back)", "select only (no read-back)",
                                                   "torch sort loop (reference)"))
    lines = [f"Robust MEG scaler of one recording, {s['N']} x {s['C']} x {s['T']} fp32 ({nbytes / 1e6:.1f} MB), {res['device']}:",
             "radix select (csrc/scaler_fit.hip) beside the reference's per-column sort + three .item() on the same device,",
             f"interleaved, HIP events, median of {args.reps} after warm-up [min .. max], milliseconds.", ""]
    for k, v in t.items():
        lines.append(f"  {k:30s} {v['median_ms']:9.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]")
    lines += ["",
              f"  ours / torch sort loop          x{ours / base:.4f}   (the loop takes {base / ours:.1f} times as long)"
              if ours <= base else
              f"  ours / torch sort loop          x{ours / base:.4f}   (the select is SLOWER than the torch loop)",
              f"  select only: {nbytes / 1e9 / (sel / 1e3):.1f} GB/s of the {nbytes / 1e6:.1f} MB algorithmic read "
              "(the column is walked once per digit, four times in all)",
              f"  same centre / scale tables from both: {res['same_tables']}",
              f"  for scale: the reference's RobustScaler().fit of this shape took {CPU_REFERENCE_SECONDS} s on a CPU "
              "container (not measured here)"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if not res["same_tables"]:
        raise SystemExit("scaler_fit_bench: the two implementations disagree")


if __name__ == "__main__":
    main()
