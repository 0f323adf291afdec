"""The encode task's model input and training step, measured.

    python scripts/encode_bench.py [--out profiles/encode_vs_torch.txt] [--reps 9] [--inner 20]

Shape: the reference's ConvRNN configuration (bm/conf/model/convrnn.yaml: hidden meg 512 / features 12, task encode,
loss l1) at 273 sensors, 120 feature channels, B = 256, T = 360, sample rate 120, meg_init 0.3 (limit 36), compute mode
f16x2.

  (1) ``bm_meg_init`` (csrc/encode.hip: reads the head, writes x once, publishes max |x|) beside the torch composition it
      replaces on the same device: ``meg * mask`` (bm/solver.py:289-292) plus the ``bm_amax`` scan the f16x2 first layer
      would need.  Both are warmed up; a timed repetition is ``inner`` calls bracketed by HIP events on the stream and
      followed by a synchronise; the repetitions of the implementations alternate; the median is reported.  The two must
      agree element for element, and the maxima exactly.
  (2) the full training step of ``Solver(task="encode")`` (forward, L1 over the window, backward, Adam), timed the same way.

The measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE = dict(B=256, C=273, F=120, T=360, S=30, sample_rate=120., meg_init=0.3, hidden=dict(meg=512, features=12))


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


def measure(reps: int, inner: int, steps: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import L1Loss
    from brainmagick_amd.models import ConvRNN
    from brainmagick_amd.solver import Solver, encode_limit
    from brainmagick_amd.synthetic import SegmentBatch
    d = SHAPE
    H.set_compute_dtype("f16x2")
    limit = encode_limit(d["meg_init"], d["sample_rate"])
    gen = torch.Generator().manual_seed(11)
    meg = torch.randn(d["B"], d["C"], d["T"], generator=gen).clamp_(-20, 20).cuda()
    mask = torch.zeros(d["T"]).to(meg)
    mask[:limit] = 1
    result = {}

    def ours():
        result["ours"] = H.meg_init(meg, limit)

    def torch_ops():
        x = mask * meg
        H.amax(x)
        result["torch"] = x

    def torch_product_only():
        mask * meg

    impls = {"bm_meg_init": ours, "torch: mask * meg + bm_amax scan": torch_ops,
             "torch: mask * meg alone": torch_product_only}
    for fn in impls.values():                       # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):                           # interleaved
        for k, fn in impls.items():
            times[k].append(_timed(fn, inner))
    a, b = result["ours"], result["torch"]
    same = bool((a == b).all()) and float(H.amax(a).max()) == float(H.amax(b).max())

    # (2) the full encode training step
    torch.manual_seed(1)
    model = ConvRNN(in_channels={"meg": d["C"], "features": d["F"]}, out_channels=d["C"], hidden=dict(d["hidden"]),
                    n_subjects=d["S"])
    features = torch.randn(d["B"], d["F"], d["T"], generator=gen)
    batch = SegmentBatch(meg, features.cuda(), torch.ones(d["B"], 1, d["T"], dtype=torch.bool, device="cuda"),
                         torch.randint(0, d["S"], (d["B"],), generator=gen).cuda(),
                         torch.zeros(d["B"], dtype=torch.int64, device="cuda"))
    solver = Solver(model, loss=L1Loss(), task="encode", meg_init=d["meg_init"], sample_rate=d["sample_rate"])
    losses = [float(solver.train_step(batch)) for _ in range(3)]           # warm-up
    torch.cuda.synchronize()
    step_times = [_timed(lambda: solver.train_step(batch), steps) for _ in range(reps)]
    solver.check_pending_flags()
    losses.append(float(solver.eval_step(batch)))
    return dict(times={k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()},
                step=dict(median_ms=_median(step_times), min_ms=min(step_times), max_ms=max(step_times)),
                same=same, limit=limit, nbytes=meg.numel() * 4, losses=losses,
                parameters=sum(p.numel() for p in model.parameters()), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "encode_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, args.inner, args.steps)))
        return
    cmd = ["timeout", "-k", "10", "400", sys.executable, str(Path(__file__).resolve()), "--child", "--reps",
           str(args.reps), "--inner", str(args.inner), "--steps", str(args.steps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"encode_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    d, t = SHAPE, res["times"]
    ours, base, product = (t[k]["median_ms"] for k in t)
    nbytes, head = res["nbytes"], res["nbytes"] * res["limit"] / d["T"]
    lines = [f"The encode task's model input, meg [{d['B']}, {d['C']}, {d['T']}] fp32 ({nbytes / 1e6:.0f} MB), limit "
             f"{res['limit']} of {d['T']} samples, compute mode f16x2, {res['device']}:",
             "bm_meg_init (csrc/encode.hip) beside the torch composition it replaces on the same device, interleaved,",
             f"HIP events around {args.inner} calls, median of {args.reps} after warm-up [min .. max], milliseconds per call.",
             ""]
    for k, v in t.items():
        lines.append(f"  {k:36s} {v['median_ms']:9.4f}  [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]")
    lines += ["",
              f"  bm_meg_init / (mask * meg + bm_amax scan)   x{ours / base:.3f}   "
              + (f"(the torch composition takes {base / ours:.1f} times as long)" if ours <= base
                 else "(bm_meg_init is SLOWER)"),
              f"  bm_meg_init / (mask * meg alone)            x{ours / product:.3f}",
              f"  bm_meg_init moves {(nbytes + head) / 1e6:.0f} MB ({head / 1e6:.0f} MB read, {nbytes / 1e6:.0f} MB "
              f"written): {(nbytes + head) / 1e9 / (ours / 1e3):.0f} GB/s",
              f"  outputs equal element for element, maxima equal: {res['same']}",
              "",
              f"Full training step of Solver(task=\"encode\"): ConvRNN {d['C']} sensors + {d['F']} feature channels -> "
              f"{d['C']}, hidden {d['hidden']['meg']} / {d['hidden']['features']}, {res['parameters'] / 1e6:.1f} M "
              f"parameters, L1 over t >= {res['limit']}, Adam;",
              f"HIP events around {args.steps} steps, median of {args.reps} after 3 warm-up steps [min .. max]:",
              "",
              f"  train_step                           {res['step']['median_ms']:9.3f}  [{res['step']['min_ms']:.3f} .. "
              f"{res['step']['max_ms']:.3f}] ms",
              f"  bm_meg_init share of the step        {100 * ours / res['step']['median_ms']:9.3f} %",
              f"  losses of the warm-up steps and after the timed ones: "
              + ", ".join(f"{v:.5f}" for v in res["losses"])]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if not res["same"]:
        raise SystemExit("encode_bench: bm_meg_init and mask * meg disagree")


if __name__ == "__main__":
    main()
