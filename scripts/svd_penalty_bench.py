"""``optim.svd`` measured: the spectral kernels beside the reference's algorithm in torch ops, and the training step with it.

    python scripts/svd_penalty_bench.py [--out profiles/svd_penalty_vs_torch.txt] [--reps 7]

Model: the cfg2 SimpleConv of bench.py (208 sensors -> 120 mel bands, hidden 320, depth 10), compute mode f16x2.

  (1) value + gradient of the penalty over the model's penalised weights: ``SpectralPenaltyFn`` (csrc/spectral.hip: one
      plan, 6 + 2 forward and 7 backward launches for all matrices) beside what ``bm/svd.py`` runs, on the same device:
      per weight ``torch.svd_lowrank(p.view(p.shape[0], -1), 16, 2)[1][0] ** 2``, summed, and ``torch.autograd.grad``.
      The two draw different test matrices; both are compared with the exact sigma_1 ** 2 from ``torch.linalg.svdvals``.
  (2) the full training step of ``Solver`` at batch 256 with svd = 0 and svd = 0.1.

Everything is warmed up; a timed repetition is ``inner`` calls bracketed by HIP events on the stream and followed by a
synchronise; the repetitions of the implementations alternate; medians are reported."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


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
    for fn in impls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(_timed(fn, inner[k]))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def measure(reps: int) -> dict:
    import torch
    from bench import CLIP_CONV
    from brainmagick_amd import hip_ops as H, synthetic
    from brainmagick_amd.functional import SpectralPenaltyFn
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.svd import penalized_weights
    torch.cuda.set_device(0)
    c = synthetic.CONFIGS["cfg2"]

    def build():
        torch.manual_seed(2036)
        return SimpleConv(in_channels={"meg": c["C"]}, out_channels=c["F"], hidden={"meg": 320}, n_subjects=c["S"],
                          **CLIP_CONV)
    model = build().cuda()
    named = penalized_weights(model)
    ws = [p for _, p in named]
    sizes = [min(p.shape[0], p.numel() // p.shape[0]) for p in ws]
    R_all = torch.randn(sum(sizes), 16, device="cuda")
    out = dict(device=torch.cuda.get_device_name(0), compute_dtype=H.get_compute_dtype(),
               weights=[[k, list(p.shape)] for k, p in named])

    def ours():
        total = SpectralPenaltyFn.apply(R_all, 2, *ws)
        return total, torch.autograd.grad(total, ws)

    def torch_ops():
        total = sum(torch.svd_lowrank(p.view(p.shape[0], -1), 16, 2)[1][0].pow(2) for p in ws)
        return total, torch.autograd.grad(total, ws)
    exact = float(sum(torch.linalg.svdvals(p.detach().view(p.shape[0], -1).double())[0] ** 2 for p in ws))
    out["sum_of_exact_sigma1_squared"] = exact
    out["estimate_over_exact"] = dict(spectral=float(ours()[0]) / exact)
    impls = dict(spectral=ours)
    try:
        out["estimate_over_exact"]["torch_ops"] = float(torch_ops()[0]) / exact
        impls["torch_ops"] = torch_ops
    except Exception as exc:                        # the vendor solver behind torch.linalg.qr may be absent
        out["torch_ops_error"] = repr(exc)
    out["penalty_value_and_gradient"] = _interleaved(impls, reps, dict(spectral=20, torch_ops=2))
    plan = H.spectral_plan([p.detach() for p in ws], 16, 2)
    one = torch.ones(1, device="cuda")
    out["penalty_kernels_only"] = _interleaved(dict(forward=lambda: H.spectral_fwd(plan, R_all),
                                                    backward=lambda: H.spectral_bwd(plan, one)), reps,
                                               dict(forward=20, backward=20))

    batch = synthetic.make_config_batch("cfg2", seed=2036).to("cuda")
    solvers = {"svd=0": Solver(build()), "svd=0.1": Solver(build(), svd=0.1)}
    out["training_step"] = _interleaved({k: (lambda s=s: s.train_step(batch)) for k, s in solvers.items()}, reps,
                                        {k: 10 for k in solvers})
    for s in solvers.values():
        s.check_pending_flags()
    return out


def report(res: dict) -> str:
    lines = ["optim.svd: the spectral kernels beside torch.svd_lowrank + autograd (scripts/svd_penalty_bench.py)",
             f"device: {res['device']}, compute mode {res['compute_dtype']}; medians of alternating repetitions "
             "(min .. max), HIP events", "",
             f"penalised weights of the cfg2 SimpleConv ({len(res['weights'])}): "
             + ", ".join("x".join(map(str, s)) for _, s in res["weights"]), "",
             "sum of the estimates over the sum of the exact sigma_1 ** 2 (dim 16, niters 2): "
             + ", ".join(f"{k} {v:.4f}" for k, v in res["estimate_over_exact"].items()), ""]
    if "torch_ops_error" in res:
        lines += [f"torch ops on this device failed: {res['torch_ops_error']}", ""]
    for title, key in (("value + gradient of the penalty, all weights", "penalty_value_and_gradient"),
                       ("the launches alone (no autograd)", "penalty_kernels_only"),
                       ("training step, cfg2 at batch 256", "training_step")):
        lines.append(title + ":")
        for k, v in res[key].items():
            lines.append(f"  {k:12s} {v['median_ms']:9.3f} ms   ({v['min_ms']:.3f} .. {v['max_ms']:.3f})")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "svd_penalty_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    res = measure(args.reps)
    text = report(res)
    print(text)
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
