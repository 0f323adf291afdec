"""FeatureDecodingLoss forward + backward: the fused kernels (csrc/regress.hip) beside the reference's algorithm written in
torch ops on the same device, interleaved.

    python scripts/feature_decoding_bench.py [--out profiles/feature_decoding_vs_torch.txt] [--reps 9]

Workload: B = 256, T = 360, features emb (300 continuous channels), ph (40 classes), hash (1025 classes), seg (3 classes)
with class weighting on, a [B, 1, T] mask about 60 % true, seeded; the model output has 1368 channels (504 MB).  ``ours``
is ``losses.FeatureDecodingLoss`` (one forward and one backward launch, no read-back); ``forward only`` is the same without
autograd.  The baseline is bm/losses.py:127-173 restated: per feature the boolean-mask gathers, the two transposes, the
``.long()`` cast, ``F.cross_entropy`` / ``F.mse_loss``, and the two synchronising asserts (``mask.any()``, the category
maximum).  Every implementation is warmed up, the timed repetitions alternate, each is bracketed by HIP events on the
stream and followed by a synchronise, and the median is reported.  Both must give the same loss (1e-6 relative) and the
same gradient (1e-5 of its largest element).

The measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests" / "golden"))

SHAPE = dict(B=256, T=360)
FEATURES = [("emb", 300, None), ("ph", 1, 40), ("hash", 1, 1025), ("seg", 1, 3)]


def _median(v):
    return sorted(v)[len(v) // 2]


def measure(reps: int) -> dict:
    import torch
    import torch.nn.functional as F
    from brainmagick_amd.losses import FeatureDecodingLoss
    from make_feature_decoding_golden import Builder, Weights, class_weights, targets
    B, T = SHAPE["B"], SHAPE["T"]
    gen = torch.Generator().manual_seed(7)
    builder = Builder(FEATURES)
    est = (3 * torch.randn(B, builder.output_dimension, T, generator=gen)).cuda()
    out = targets(builder, B, T, gen).cuda()
    mask = (torch.rand(B, 1, T, generator=gen) > 0.4).cuda()
    weights = class_weights(builder, gen)
    scaler = Weights(weights)
    dev_weights = {k: v.cuda() for k, v in weights.items()}
    loss_mod = FeatureDecodingLoss(builder, scaler)
    result = {}

    def ours():
        e = est.detach().requires_grad_(True)
        loss = loss_mod(e, out, mask)
        loss.backward()
        result["ours"] = (loss.detach(), e.grad)

    def forward_only():
        with torch.no_grad():
            loss_mod(est, out, mask)

    def torch_ops():
        e = est.detach().requires_grad_(True)
        assert mask.any()
        loss = 0
        for f in builder.values():
            sl, sl_out = builder.get_slice(f.name), builder.get_slice(f.name, model_output=True)
            fe, fo = e[:, sl_out], out[:, sl]
            fm = mask.expand_as(fe)
            if f.categorical:
                assert f.output_dimension > out[:, sl.start].max()
                fe, fo, fm = fe.transpose(1, 2), fo.transpose(1, 2), fm.transpose(1, 2)
                loss = loss + F.cross_entropy(fe[fm].reshape(-1, sl_out.stop - sl_out.start),
                                              fo.long()[mask.transpose(1, 2)], dev_weights[f.name])
            else:
                loss = loss + F.mse_loss(fe[fm], fo[fm])
        loss.backward()
        result["torch"] = (loss.detach(), e.grad)

    impls = {"ours (forward + backward)": ours, "ours (forward only)": forward_only,
             "torch ops (forward + backward)": torch_ops}
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
    (la, ga), (lb, gb) = result["ours"], result["torch"]
    loss_err = abs(float(la) - float(lb)) / abs(float(lb))
    grad_err = float((ga - gb).abs().max() / gb.abs().max())
    return dict(times={k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()},
                loss=float(la), loss_err=loss_err, grad_err=grad_err, nbytes=est.numel() * 4 + out.numel() * 4,
                grad_bytes=est.numel() * 4,
                channels=builder.output_dimension, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "feature_decoding_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps)))
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, str(Path(__file__).resolve()), "--child", "--reps",
           str(args.reps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"feature_decoding_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    t = res["times"]
    ours, fwd, base = (t[k]["median_ms"] for k in impls_order())
    read = res["nbytes"]
    lines = [f"FeatureDecodingLoss, B = {SHAPE['B']}, T = {SHAPE['T']}, features {FEATURES}, class weights on,",
             f"{res['channels']} model outputs ({read / 1e6:.0f} MB of logits and targets), {res['device']}:",
             "the fused kernels (csrc/regress.hip) beside the reference's algorithm in torch ops on the same device,",
             f"interleaved, HIP events, median of {args.reps} after warm-up [min .. max], milliseconds.", ""]
    for k, v in t.items():
        lines.append(f"  {k:32s} {v['median_ms']:9.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]")
    lines += ["",
              f"  ours / torch ops (forward + backward)   x{ours / base:.3f}   "
              + (f"(torch ops take {base / ours:.1f} times as long)" if ours <= base else "(the fused kernels are SLOWER)"),
              f"  forward only: {read / 1e9 / (fwd / 1e3):.0f} GB/s of the {read / 1e6:.0f} MB it has to read once; "
              f"forward + backward: {(2 * read + res['grad_bytes']) / 1e9 / (ours / 1e3):.0f} GB/s of two reads and the "
              f"{res['grad_bytes'] / 1e6:.0f} MB gradient written once",
              f"  loss {res['loss']:.6f}; against torch ops: loss {res['loss_err']:.1e} relative, gradient "
              f"{res['grad_err']:.1e} of its largest element"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    if res["loss_err"] > 1e-6 or res["grad_err"] > 1e-5:
        raise SystemExit("feature_decoding_bench: the two implementations disagree")


def impls_order():
    return ("ours (forward + backward)", "ours (forward only)", "torch ops (forward + backward)")


if __name__ == "__main__":
    main()
