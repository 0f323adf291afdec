"""Golden vectors of the regression objective, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_regression_golden.py [output directory]
Writes ``regression.npz`` (default: next to this file) with three groups:

  (a) ``loss/<kind>/<mask form>/*``: bm/losses.py L1Loss / L2Loss values and the autograd gradients of both operands
      on a ragged shape, for the mask forms none (the reference gets an all-true mask), [B, 1, T] and [B, F, T], one
      segment masked out entirely;
  (b) ``train/<l2|l1>/*``: two training steps of the reference SimpleConv at tests/helpers.py's WIDE_DIMS / WIDE_CFG
      (the wide_kernels_train recipe: parameters and inputs rebuilt from the seed, digests, forward output, losses,
      gradient norms + 64 samples, 64 samples after Adam) -- L2Loss under a partial [B, 1, T] mask, L1Loss unmasked;
  (c) ``metrics/*``: OnlineCorrelation, L2Reg and L1Reg of bm/metrics.py over two recordings of three batches each,
      partial mask, trim_offset 5, in the statement order of bm/play.py:get_test_metrics: per-recording get(), reduce().
"""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))
sys.path.insert(2, str(HERE.parent.parent))

from _ref_import import REF, load_reference  # noqa: E402

LOSS_SHAPE = dict(B=5, F=7, T=37)
METRIC_SHAPE = dict(B=4, F=6, T=30, recordings=2, batches=3, trim=5)


def _ref_metrics():
    """bm/metrics.py by file spec (it imports only torch)."""
    if "bm_ref_metrics" not in sys.modules:
        spec = importlib.util.spec_from_file_location("bm_ref_metrics", REF / "bm" / "metrics.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["bm_ref_metrics"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["bm_ref_metrics"]


def partial_row_mask(B: int, T: int, gen: torch.Generator) -> torch.Tensor:
    """[B, 1, T] bool: every segment loses one random run of samples; segment 0 keeps at least half."""
    mask = torch.ones(B, 1, T, dtype=torch.bool)
    for b in range(B):
        n = int(torch.randint(1, T // 2, (1,), generator=gen))
        start = int(torch.randint(0, T - n, (1,), generator=gen))
        mask[b, 0, start:start + n] = False
    return mask


def loss_fixture(losses):
    d = LOSS_SHAPE
    B, F, T = d["B"], d["F"], d["T"]
    gen = torch.Generator().manual_seed(1234)
    est = torch.randn(B, F, T, generator=gen)
    out = torch.randn(B, F, T, generator=gen)
    out[0, 0, :4] = est[0, 0, :4]                      # exact ties: sign(0) = 0 in the L1 gradient
    row = partial_row_mask(B, T, gen)
    row[3] = False                                     # a segment that is masked out entirely
    full = torch.rand(B, F, T, generator=gen) > 0.4
    full[3] = False
    res = {"loss/est": est.numpy(), "loss/out": out.numpy(), "loss/mask_row": row.numpy(),
           "loss/mask_full": full.numpy()}
    for kind, cls in (("l1", losses.L1Loss), ("mse", losses.L2Loss)):
        for form, mask in (("none", torch.ones(B, 1, T, dtype=torch.bool)), ("row", row), ("full", full)):
            e = est.clone().requires_grad_(True)
            o = out.clone().requires_grad_(True)
            loss = cls()(e, o, mask)
            loss.backward()
            res[f"loss/{kind}/{form}/loss"] = np.array(loss.item(), dtype=np.float32)
            res[f"loss/{kind}/{form}/grad_est"] = e.grad.numpy().copy()
            res[f"loss/{kind}/{form}/grad_out"] = o.grad.numpy().copy()
    return res


def train_fixture(sc, common, losses):
    import helpers as Hh
    from make_golden import _Batch
    d = Hh.WIDE_DIMS
    res = {}
    for tag, cls, masked in (("l2", losses.L2Loss, True), ("l1", losses.L1Loss, False)):
        sb, features, ban_center, gen = Hh.wide_inputs()
        torch.manual_seed(d["seed"])
        model = sc.SimpleConv(in_channels={"meg": d["C"]}, out_channels=d["F"], hidden={"meg": d["hidden"]},
                              n_subjects=d["S"], **Hh.WIDE_CFG)
        Hh.randomize_batchnorm(model, gen)
        mask = partial_row_mask(d["B"], d["T"], torch.Generator().manual_seed(d["seed"] + 7)) if masked else \
            torch.ones(d["B"], 1, d["T"], dtype=torch.bool)
        loss_mod = cls()
        optim = torch.optim.Adam(model.parameters(), lr=3e-4, betas=(0.9, 0.999))
        model.train(True)
        batch = _Batch(sb)
        common.PositionGetter.get_positions = lambda self, b: b._positions.clone()
        real_rand = torch.rand

        def fake_rand(*a, **k):
            if a == (2,):
                return ban_center.clone()
            return real_rand(*a, **k)

        p = f"train/{tag}/"
        for k, v in model.state_dict().items():
            res[f"{p}sd0_digest/{k}"] = Hh.tensor_digest(v)
        res[f"{p}in_digest/meg"] = Hh.tensor_digest(sb.meg)
        res[f"{p}in_digest/features"] = Hh.tensor_digest(features)
        res[f"{p}in/mask"] = mask.numpy().copy()
        common.torch.rand = fake_rand
        try:
            seen = []
            for step in range(2):
                estimate = model({"meg": sb.meg.clone()}, batch)
                loss = loss_mod(estimate, features, mask)
                optim.zero_grad()
                loss.backward()
                if step == 0:
                    res[f"{p}out/estimate"] = estimate.detach().numpy().copy()
                    for k, prm in model.named_parameters():
                        g = prm.grad.detach().flatten()
                        res[f"{p}grad_norm/{k}"] = np.array(float(g.double().norm()))
                        res[f"{p}grad_max/{k}"] = np.array(float(g.abs().max()))
                        res[f"{p}grad_sample/{k}"] = g[Hh.sample_indices(g.numel())].numpy().copy()
                optim.step()
                seen.append(float(loss))
        finally:
            common.torch.rand = real_rand
        res[f"{p}out/losses"] = np.asarray(seen, dtype=np.float64)
        for k, prm in model.named_parameters():
            res[f"{p}sd1_sample/{k}"] = prm.detach().flatten()[Hh.sample_indices(prm.numel())].numpy().copy()
    return res


def metrics_fixture():
    M = _ref_metrics()
    d = METRIC_SHAPE
    B, F, T, trim = d["B"], d["F"], d["T"], d["trim"]
    gen = torch.Generator().manual_seed(77)
    res = {}
    ctors = [M.L2Reg.get_constructor(slice(None), slice(None), name="l2_feature"),
             M.OnlineCorrelation.get_constructor(slice(None), slice(None), name="corr_feature"),
             M.L1Reg.get_constructor(slice(None), slice(None), name="l1_feature")]
    results = {c().name: [] for c in ctors}
    for r in range(d["recordings"]):
        metrics = [c() for c in ctors]
        for i in range(d["batches"]):
            est = torch.randn(B, F, T, generator=gen)
            gt = 0.6 * est + 0.8 * torch.randn(B, F, T, generator=gen) + 0.1
            mask = partial_row_mask(B, T, gen)
            mask[0] = True                              # every (f, t) column keeps a sample
            res[f"metrics/in/{r}/{i}/est"] = est.numpy()
            res[f"metrics/in/{r}/{i}/gt"] = gt.numpy()
            res[f"metrics/in/{r}/{i}/mask"] = mask.numpy()
            e, g, m = est[..., trim:], gt[..., trim:], mask[..., trim:]
            for metric in metrics:
                metric.update(e.to(torch.double), g.to(torch.double), m)
        for metric in metrics:
            value = metric.get()
            res[f"metrics/get/{r}/{metric.name}"] = value.numpy().copy()
            results[metric.name].append(value.cpu().float())
    for c in ctors:
        metric = c()
        res[f"metrics/reduce/{metric.name}"] = np.array(metric.reduce(results[metric.name]), dtype=np.float64)
    return res


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    sc, common, losses = load_reference()
    out = {"meta": json.dumps(dict(loss_shape=LOSS_SHAPE, metric_shape=METRIC_SHAPE, torch=torch.__version__))}
    out.update(loss_fixture(losses))
    out.update(train_fixture(sc, common, losses))
    out.update(metrics_fixture())
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "regression.npz", **out)
    print(f"regression: {len(out)} arrays -> {dest / 'regression.npz'}")


if __name__ == "__main__":
    main(sys.argv[1:])
