"""``task.lowpass`` measured: the one-launch filter beside the torch ops it replaces, and the encode training step with it.

    python scripts/lowpass_bench.py [--out profiles/lowpass_vs_torch.txt] [--reps 9] [--inner 200]

Shape: a batch of 256 segments x 273 sensors x 378 samples, read through the ``offset_meg_ms = 150`` view ``[..., 18:]``
(T = 360) at 120 Hz, compute mode f16x2; ``zeros = 5`` as the Solver calls it (bm/solver.py:279).

  (1) per cutoff -- 30 Hz (half 10, 21 taps) and 5 Hz (half 60, 121 taps) -- ``bm_lowpass`` (csrc/lowpass.hip) with and
      without the published maximum beside what a user would run without it on the same device: ``.contiguous()`` of
      the view, ``F.pad(mode="replicate")``, ``F.conv1d`` with the same taps, then the ``bm_amax`` scan the f16x2 first
      layer needs.  The two must agree within the summation bound of tests/test_lowpass_gpu.py, the maxima likewise.
  (2) the encode task's model input at limit 36: one ``keep = 36`` launch beside full-length ``lowpass`` + ``bm_meg_init``.
  (3) the full training step of ``Solver(task="encode")`` on README's ConvRNN (273 + 120 -> 273) with lowpass 0 and 30.

Everything is warmed up; a timed repetition is ``inner`` calls (``steps`` training steps) bracketed by HIP events on the
stream and followed by a synchronise; the repetitions of the implementations alternate; medians are reported.  The
measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE = dict(B=256, C=273, F=120, T_full=378, offset=18, S=30, sample_rate=120., meg_init=0.3,
             hidden=dict(meg=512, features=12), cutoffs_hz=(30., 5.), zeros=5)
HBM_MEASURED_TBS = 6.29          # float4 copy on the MI355X; 8.0 TB/s is the specification


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn, inner):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def _interleaved(impls, reps, inner):
    import torch
    for fn in impls.values():                       # warm-up: code objects, allocator, the conv's algorithm choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(_timed(fn, inner))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def measure(reps: int, inner: int, steps: int) -> dict:
    import torch
    from torch.nn import functional as F
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import L1Loss
    from brainmagick_amd.models import ConvRNN
    from brainmagick_amd.solver import Solver, encode_limit
    from brainmagick_amd.synthetic import SegmentBatch
    d = SHAPE
    H.set_compute_dtype("f16x2")
    gen = torch.Generator().manual_seed(11)
    base = torch.randn(d["B"], d["C"], d["T_full"], generator=gen).clamp_(-20, 20).cuda()
    view = base[..., d["offset"]:]
    T = view.shape[-1]
    limit = encode_limit(d["meg_init"], d["sample_rate"])
    out = dict(filters={}, device=torch.cuda.get_device_name(0), nbytes=view.numel() * 4, limit=limit, T=T)
    for hz in d["cutoffs_hz"]:
        cutoff = hz / d["sample_rate"]
        taps, half = H.lowpass_taps(cutoff, d["zeros"], view.device)
        result = {}

        def ours():
            result["ours"] = H.lowpass_filter(view, cutoff, zeros=d["zeros"])

        def ours_quiet():
            H.lowpass_filter(view, cutoff, zeros=d["zeros"], publish_amax=False)

        def torch_ops():
            x = view.contiguous()
            y = F.conv1d(F.pad(x.reshape(-1, 1, T), (half, half), mode="replicate"), taps[None, None]).reshape(x.shape)
            H.amax(y)
            result["torch"] = y

        def torch_alone():
            x = view.contiguous()
            F.conv1d(F.pad(x.reshape(-1, 1, T), (half, half), mode="replicate"), taps[None, None]).reshape(x.shape)

        impls = {"bm_lowpass, maximum published": ours, "bm_lowpass, no maximum": ours_quiet,
                 "torch: contiguous + pad + conv1d + bm_amax scan": torch_ops,
                 "torch: contiguous + pad + conv1d alone": torch_alone}
        times = _interleaved(impls, reps, inner)
        a, b = result["ours"], result["torch"]
        # both are fp32 sums of the same 2 half + 1 products: they differ by at most the two summation bounds
        mag = F.conv1d(F.pad(view.abs().reshape(-1, 1, T), (half, half), mode="replicate"),
                       taps.abs()[None, None]).reshape(a.shape)
        bound = 2 * (2 * half + 3) * 2.0 ** -24 * mag
        same = bool(((a - b).abs() <= bound).all()) and \
            abs(float(H.amax(a).max()) - float(H.amax(b).max())) <= float(bound.max())
        out["filters"][str(hz)] = dict(half=half, times=times, same=same)
        del result, a, b, mag, bound

    # (2) the encode task's model input
    cutoff = d["cutoffs_hz"][0] / d["sample_rate"]

    def one_launch():
        H.lowpass_filter(view, cutoff, zeros=d["zeros"], keep=limit)

    def two_launches():
        H.meg_init(H.lowpass_filter(view, cutoff, zeros=d["zeros"], publish_amax=False), limit)
    out["keep"] = _interleaved({f"bm_lowpass keep = {limit}": one_launch,
                                "bm_lowpass (full length) + bm_meg_init": two_launches}, reps, inner)

    # (3) the full encode training step, lowpass 0 and 30 Hz, alternating
    features = torch.randn(d["B"], d["F"], T, generator=gen).cuda()
    meg = view.contiguous()
    batch = SegmentBatch(meg, features, torch.ones(d["B"], 1, T, dtype=torch.bool, device="cuda"),
                         torch.randint(0, d["S"], (d["B"],), generator=gen).cuda(),
                         torch.zeros(d["B"], dtype=torch.int64, device="cuda"))
    solvers, losses = {}, {}
    for hz in (0., d["cutoffs_hz"][0]):
        torch.manual_seed(1)
        model = ConvRNN(in_channels={"meg": d["C"], "features": d["F"]}, out_channels=d["C"], hidden=dict(d["hidden"]),
                        n_subjects=d["S"])
        solvers[hz] = Solver(model, loss=L1Loss(), task="encode", meg_init=d["meg_init"], sample_rate=d["sample_rate"],
                             lowpass=hz)
        losses[str(hz)] = [float(solvers[hz].train_step(batch)) for _ in range(3)]           # warm-up
    torch.cuda.synchronize()
    step_times = {str(hz): [] for hz in solvers}
    for _ in range(reps):
        for hz, solver in solvers.items():
            step_times[str(hz)].append(_timed(lambda: solver.train_step(batch), steps))
    for hz, solver in solvers.items():
        solver.check_pending_flags()
        losses[str(hz)].append(float(solver.eval_step(batch)))
    out["step"] = {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in step_times.items()}
    out["losses"] = losses
    return out


def _row(label, v, width=52):
    return f"  {label:{width}s} {v['median_ms']:9.4f}  [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lowpass_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, args.inner, args.steps)))
        return
    cmd = ["timeout", "-k", "10", "500", sys.executable, str(Path(__file__).resolve()), "--child", "--reps",
           str(args.reps), "--inner", str(args.inner), "--steps", str(args.steps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"lowpass_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    d = SHAPE
    nbytes, T, limit = res["nbytes"], res["T"], res["limit"]
    moved = 2 * nbytes              # one read and one write of the tensor, from the shapes
    lines = [f"task.lowpass: batch [{d['B']}, {d['C']}, {d['T_full']}] fp32 read through the view [..., {d['offset']}:] "
             f"(T = {T}, {nbytes / 1e6:.0f} MB), zeros = {d['zeros']}, {d['sample_rate']:.0f} Hz, compute mode f16x2, "
             f"{res['device']}:",
             "bm_lowpass (csrc/lowpass.hip) beside the torch ops a user would run without it, same device, interleaved,",
             f"HIP events around {args.inner} calls, median of {args.reps} after warm-up [min .. max], milliseconds per call.",
             f"Bytes per launch from the shapes: one read and one write of the tensor = {moved / 1e6:.0f} MB."]
    ok = True
    for hz, f in res["filters"].items():
        t = f["times"]
        ours, quiet, base, alone = (t[k]["median_ms"] for k in t)
        rate = moved / 1e9 / (ours / 1e3)
        lines += ["", f"lowpass {float(hz):.0f} Hz: half {f['half']}, {2 * f['half'] + 1} taps"]
        lines += [_row(k, v) for k, v in t.items()]
        lines += [f"  bm_lowpass / (torch ops + bm_amax scan)   x{ours / base:.3f}   "
                  + (f"(the torch ops take {base / ours:.1f} times as long)" if ours <= base
                     else "(bm_lowpass is SLOWER)"),
                  f"  bm_lowpass, no maximum / (torch ops alone) x{quiet / alone:.3f}"
                  + ("" if quiet <= alone else "   (bm_lowpass is SLOWER)"),
                  f"  the published maximum costs {1e3 * (ours - quiet):.1f} us of the launch",
                  f"  {moved / 1e6:.0f} MB in {ours:.4f} ms = {rate:.0f} GB/s: {100 * rate / 1e3 / HBM_MEASURED_TBS:.0f} % of "
                  f"the {HBM_MEASURED_TBS} TB/s a float4 copy reaches from HBM.  The {moved / 1e6:.0f} MB of a call fit the "
                  "256 MiB Infinity Cache, so",
                  "  back-to-back calls may find their input there: the rate is a ceiling for HBM-resident data, and it "
                  + ("is below what HBM itself delivers: the kernel is bound by its LDS staging, not by memory."
                     if rate / 1e3 < HBM_MEASURED_TBS else "is in the Infinity Cache's range."),
                  f"  results within the two summation bounds of each other, maxima likewise: {f['same']}"]
        ok = ok and f["same"]
    k = res["keep"]
    one, two = (k[name]["median_ms"] for name in k)
    head = nbytes * min(T, limit + res["filters"][str(d["cutoffs_hz"][0])]["half"]) / T
    lines += ["", f"The encode task's model input (limit {limit} of {T} samples), lowpass {d['cutoffs_hz'][0]:.0f} Hz:"]
    lines += [_row(name, v) for name, v in k.items()]
    lines += [f"  one launch / two launches   x{one / two:.3f}" + ("" if one <= two else "   (the one launch is SLOWER)"),
              f"  the keep launch reads {head / 1e6:.0f} MB and writes {nbytes / 1e6:.0f} MB: "
              f"{(head + nbytes) / 1e9 / (one / 1e3):.0f} GB/s"]
    s = res["step"]
    off, on = s["0.0"], s[str(d["cutoffs_hz"][0])]
    lines += ["",
              f"Full training step of Solver(task=\"encode\"): ConvRNN {d['C']} sensors + {d['F']} feature channels -> "
              f"{d['C']}, hidden {d['hidden']['meg']} / {d['hidden']['features']}, L1 over t >= {limit}, Adam;",
              f"HIP events around {args.steps} steps, median of {args.reps} after 3 warm-up steps, alternating [min .. max]:",
              "",
              f"  train_step, lowpass = 0     {off['median_ms']:9.3f}  [{off['min_ms']:.3f} .. {off['max_ms']:.3f}] ms",
              f"  train_step, lowpass = {d['cutoffs_hz'][0]:.0f}    {on['median_ms']:9.3f}  [{on['min_ms']:.3f} .. "
              f"{on['max_ms']:.3f}] ms   ({1e3 * (on['median_ms'] - off['median_ms']):+.0f} us, "
              f"x{on['median_ms'] / off['median_ms']:.4f})",
              "  (lowpass_gt: the step filters at full length for the target, then bm_meg_init)",
              "  losses of the warm-up steps and after the timed ones: "
              + "; ".join(f"lowpass {float(hz):.0f}: " + ", ".join(f"{v:.5f}" for v in ls)
                          for hz, ls in res["losses"].items())]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if not ok:
        raise SystemExit("lowpass_bench: bm_lowpass and the torch ops disagree")


if __name__ == "__main__":
    main()
