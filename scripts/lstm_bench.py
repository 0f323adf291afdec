"""LSTM stack of ConvRNN on the HIP step kernels (csrc/lstm.hip) beside torch's LSTM, on one device, interleaved.

    python scripts/lstm_bench.py [--out profiles/lstm_vs_torch.txt] [--reps 7] [--skip-step]

Shapes: the reference's convrnn stack (In 576 -> H 512, B 256, T' 92) with 4 unidirectional layers, and the
decoder_convrnn stack (In 512, 2 bidirectional layers).  Three implementations per shape, forward and forward +
backward: ``BF.LSTMFn`` (this project), torch's composite ATen LSTM (vendor RNN library disabled: what ``DualPathRNN``
runs) and torch's default LSTM path.  Every shape is warmed up, the timed repetitions alternate between the
implementations, each is bracketed by HIP events on the stream, and the median is reported.  Last, one full ConvRNN
training step (273 sensors, hidden 512, B 256, T 360, 4 layers) with the per-family kernel time split from
``hip_ops.KernelTimer``.

Each part runs in a child process of its own under a time limit; a part that fails ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {
    "convrnn 4 layers unidirectional": dict(In=576, H=512, B=256, T=92, layers=4, bidirectional=False),
    "decoder_convrnn 2 layers bidirectional": dict(In=512, H=512, B=256, T=92, layers=2, bidirectional=True),
}


def _median(v):
    return sorted(v)[len(v) // 2]


def part_stack(name: str, reps: int) -> dict:
    import torch
    from brainmagick_amd import functional as BF
    s = SHAPES[name]
    torch.manual_seed(0)
    rnn = torch.nn.LSTM(s["In"], s["H"], s["layers"], bidirectional=s["bidirectional"]).cuda()
    params = [getattr(rnn, n) for n in rnn._flat_weights_names]
    dirs = 2 if s["bidirectional"] else 1
    x = torch.randn(s["B"], s["In"], s["T"], device="cuda")
    x_tbc = x.permute(2, 0, 1).contiguous()
    dy = torch.randn(s["B"], s["H"] * dirs, s["T"], device="cuda")
    dy_tbc = dy.permute(2, 0, 1).contiguous()

    def ours(backward):
        xg = x.detach().requires_grad_(backward)
        y, _, _ = BF.LSTMFn.apply(xg, s["H"], s["layers"], s["bidirectional"], 0., False, *params)
        if backward:
            y.backward(dy)

    def torch_lstm(backward, vendor):
        old = torch.backends.cudnn.enabled
        torch.backends.cudnn.enabled = vendor
        try:
            xg = x_tbc.detach().requires_grad_(backward)
            y, _ = rnn(xg)
            if backward:
                y.backward(dy_tbc)
        finally:
            torch.backends.cudnn.enabled = old

    impls = {"hip step kernels": ours, "torch composite": lambda b: torch_lstm(b, False),
             "torch default": lambda b: torch_lstm(b, True)}
    out = {}
    for backward in (False, True):
        times = {k: [] for k in impls}
        for k, fn in impls.items():                 # warm-up: code objects, algorithm choices, allocator
            for _ in range(2):
                rnn.zero_grad(set_to_none=True)
                fn(backward)
        torch.cuda.synchronize()
        for _ in range(reps):                       # interleaved
            for k, fn in impls.items():
                rnn.zero_grad(set_to_none=True)
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn(backward)
                end.record()
                end.synchronize()
                times[k].append(start.elapsed_time(end))
        out["forward + backward" if backward else "forward"] = \
            {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}
    return out


def part_step(reps: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd import synthetic
    from brainmagick_amd.models import ConvRNN
    from brainmagick_amd.solver import Solver
    torch.manual_seed(0)
    sb = synthetic.make_batch(256, 273, 360, 80, 30, seed=1)
    solver = Solver(ConvRNN(in_channels={"meg": 273}, out_channels=80, hidden={"meg": 512}, n_subjects=30, lstm=4))
    for _ in range(2):
        solver.train_step(sb)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        solver.train_step(sb)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        solver.train_step(sb)
        torch.cuda.synchronize()
    finally:
        H.set_kernel_timer(None)
    families = {}
    for label, _, start, end in timer.records:
        fam = label.split("<")[0]
        families[fam] = families.get(fam, 0.) + start.elapsed_time(end)
    return dict(step_median_ms=_median(times), step_min_ms=min(times), step_max_ms=max(times),
                timed_families_ms=dict(sorted(families.items(), key=lambda kv: -kv[1])))


def _child(args, limit):
    cmd = [sys.executable, str(Path(__file__).resolve())] + args
    proc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"lstm_bench: {' '.join(args)} ended with status {proc.returncode}; nothing more is started")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lstm_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--part", default=None)
    args = ap.parse_args()
    if args.part is not None:
        res = part_step(args.reps) if args.part == "step" else part_stack(args.part, args.reps)
        print(json.dumps(res))
        return
    lines = ["LSTM stack: HIP step kernels (csrc/lstm.hip) beside torch's LSTM, same device, interleaved, HIP events,",
             f"median of {args.reps} after warm-up [min .. max], milliseconds.  Ratio = ours / torch composite.", ""]
    for name, s in SHAPES.items():
        res = _child(["--part", name, "--reps", str(args.reps)], 420)
        lines.append(f"{name}: In {s['In']}, H {s['H']}, B {s['B']}, T' {s['T']}")
        for phase, by_impl in res.items():
            base = by_impl["torch composite"]["median_ms"]
            for impl, t in by_impl.items():
                ratio = f"   x{t['median_ms'] / base:.2f}" if impl == "hip step kernels" else ""
                lines.append(f"  {phase:18s} {impl:18s} {t['median_ms']:8.2f}  [{t['min_ms']:.2f} .. {t['max_ms']:.2f}]{ratio}")
        lines.append("")
    if not args.skip_step:
        res = _child(["--part", "step", "--reps", str(args.reps)], 420)
        lines.append("ConvRNN training step through Solver (273 sensors, hidden 512, B 256, T 360, 4 LSTM layers, ClipLoss):")
        lines.append(f"  step {res['step_median_ms']:.2f}  [{res['step_min_ms']:.2f} .. {res['step_max_ms']:.2f}]")
        lines.append("  kernel families under hip_ops.KernelTimer in one extra step (event pairs, launch gaps included):")
        for fam, ms in res["timed_families_ms"].items():
            lines.append(f"    {fam:32s} {ms:8.2f}")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
