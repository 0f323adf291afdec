"""Golden vectors of FeatureDecodingLoss and ClassificationAcc, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_feature_decoding_golden.py [output directory]
Writes ``feature_decoding.npz`` (default: next to this file).  The reference's ``bm/losses.py`` and ``bm/metrics.py`` are
loaded by file spec (both import only torch) and driven with the small features builder below (``Builder``: the surface
of ``bm.features.FeaturesBuilder`` that the loss and ``get_metric_constructors`` touch).  Three groups:

  (a) ``loss/<case>/...``: B = 5, T = 37, logits 3 randn, a [B, 1, T] mask about 60 % true.  Per case ``est``, ``out``,
      ``mask`` (``case_inputs``; the 190 000 logits of ``cat_only`` are not stored -- with their gradient they would not
      fit a committed file -- but rebuilt from the seed by both sides, ``est_digest`` proves that they did) and per variant ``<variant>/{loss, terms, grad}``: the loss, the per-feature terms (what the reference's
      ``F.mse_loss`` / ``F.cross_entropy`` calls returned, in feature order) and ``estimate.grad``.  Variants: ``plain``
      (no weights, partial mask); for ``mixed`` also ``weighted`` (class weights, one class of each feature with weight
      0: ``loss/mixed/weights/<name>``), ``plain_all`` and ``weighted_all`` (all-true mask);
  (b) ``train/*``: two Adam steps of the reference SimpleConv at tests/helpers.py's WIDE_DIMS / WIDE_CFG with
      ``out_channels`` = the model-output width of ``mixed`` and the weighted loss under a partial mask (parameters and MEG
      rebuilt from the seed, digests; targets, mask and weights stored);
  (c) ``metrics/*``: ClassificationAcc over two recordings of three batches, K = 7, partial mask, trim_offset 5, in the
      statement order of bm/play.py:get_test_metrics: per-recording get(), then reduce().
"""
import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))
sys.path.insert(2, str(HERE.parent.parent))

from _ref_import import REF, load_reference  # noqa: E402

LOSS_SHAPE = dict(B=5, T=37)
METRIC_SHAPE = dict(B=4, K=7, T=30, recordings=2, batches=3, trim=5)
# (name, dimension, cardinality): cardinality None = continuous
CASES = {"mixed": [("emb", 3, None), ("ph", 1, 64), ("aux", 2, None), ("seg", 1, 3)],
         "cat_first": [("seg", 1, 2), ("emb", 4, None)],
         "cat_only": [("hash", 1, 1025)],
         "reg_only": [("emb", 6, None)]}


class Feature:
    def __init__(self, name, dimension, cardinality):
        self.name, self.dimension, self.cardinality = name, dimension, cardinality

    @property
    def categorical(self):
        return self.cardinality is not None

    @property
    def output_dimension(self):
        return self.cardinality if self.categorical else self.dimension


class Builder(dict):
    """name -> Feature in order, with ``get_slice`` / ``dimension`` / ``output_dimension`` of
    bm.features.FeaturesBuilder (bm/features/base.py:124-143)."""

    def __init__(self, spec):
        super().__init__((name, Feature(name, dim, card)) for name, dim, card in spec)

    def get_slice(self, name, model_output=False):
        start = 0
        for key, feature in self.items():
            dim = feature.output_dimension if model_output else feature.dimension
            if key == name:
                return slice(start, start + dim)
            start += dim
        raise KeyError(f"Could not find feature {name}.")

    @property
    def dimension(self):
        return sum(f.dimension for f in self.values())

    @property
    def output_dimension(self):
        return sum(f.output_dimension for f in self.values())


class Weights:
    """The surface of BatchScaler that the loss touches."""

    def __init__(self, weights):
        self.weights = weights

    def get_categorical_feature_weights(self, name):
        return self.weights[name].clone()


def class_weights(builder, gen):
    """bm/norm.py:291-308 on random counts, class 1 (class 0 of a two-class feature) absent: weight 0."""
    out = {}
    for f in builder.values():
        if f.categorical:
            count = torch.randint(1, 50, (f.cardinality,), generator=gen).float()
            count[1 if f.cardinality > 2 else 0] = 0.
            probs = count / count.sum()
            w = 1 / torch.sqrt(probs)
            w[probs == 0] = 0.
            w /= torch.sqrt(probs).sum()
            out[f.name] = w
    return out


def targets(builder, B, T, gen):
    """[B, dimension, T]: randn on continuous channels, a class (as a float) on categorical ones."""
    out = torch.randn(B, builder.dimension, T, generator=gen)
    for f in builder.values():
        if f.categorical:
            sl = builder.get_slice(f.name)
            out[:, sl] = torch.randint(0, f.cardinality, (B, 1, T), generator=gen).float()
    return out


def _ref_metrics():
    if "bm_ref_metrics" not in sys.modules:
        spec = importlib.util.spec_from_file_location("bm_ref_metrics", REF / "bm" / "metrics.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["bm_ref_metrics"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["bm_ref_metrics"]


def run_reference(losses, builder, scaler, est, out, mask):
    """(loss, [term per feature], estimate.grad) of the reference class; the terms are what its F.mse_loss /
    F.cross_entropy calls returned."""
    real = losses.F
    seen = []

    def spy(fn):
        def call(*a, **k):
            value = fn(*a, **k)
            seen.append(float(value))
            return value
        return call
    losses.F = types.SimpleNamespace(mse_loss=spy(real.mse_loss), cross_entropy=spy(real.cross_entropy))
    try:
        e = est.clone().requires_grad_(True)
        loss = losses.FeatureDecodingLoss(builder, scaler)(e, out, mask)
        loss.backward()
    finally:
        losses.F = real
    assert len(seen) == len(builder)
    return loss, seen, e.grad


STORED_BY_SEED = ("cat_only",)       # cases whose logits are rebuilt from the seed instead of stored


def case_inputs(case):
    """(builder, est, out, mask, generator positioned behind them) of a loss case."""
    B, T = LOSS_SHAPE["B"], LOSS_SHAPE["T"]
    gen = torch.Generator().manual_seed(4242 + list(CASES).index(case))
    builder = Builder(CASES[case])
    est = 3 * torch.randn(B, builder.output_dimension, T, generator=gen)
    out = targets(builder, B, T, gen)
    mask = torch.rand(B, 1, T, generator=gen) > 0.4
    return builder, est, out, mask, gen


def loss_fixture(losses):
    import helpers as Hh
    res = {}
    for case in CASES:
        builder, est, out, mask, gen = case_inputs(case)
        p = f"loss/{case}/"
        res[p + "out"], res[p + "mask"] = out.numpy(), mask.numpy()
        res[p + "est_digest"] = Hh.tensor_digest(est)
        if case not in STORED_BY_SEED:
            res[p + "est"] = est.numpy()
        variants = [("plain", None, mask)]
        if case == "mixed":
            weights = class_weights(builder, gen)
            for name, w in weights.items():
                res[f"{p}weights/{name}"] = w.numpy().copy()
            everything = torch.ones_like(mask)
            variants += [("weighted", Weights(weights), mask), ("plain_all", None, everything),
                         ("weighted_all", Weights(weights), everything)]
        for variant, scaler, m in variants:
            loss, terms, grad = run_reference(losses, builder, scaler, est, out, m)
            res[f"{p}{variant}/loss"] = np.array(loss.item(), dtype=np.float32)
            res[f"{p}{variant}/terms"] = np.asarray(terms, dtype=np.float32)
            res[f"{p}{variant}/grad"] = grad.numpy().copy()
    return res


def train_fixture(sc, common, losses):
    import helpers as Hh
    from make_golden import _Batch
    from make_regression_golden import partial_row_mask
    d = Hh.WIDE_DIMS
    builder = Builder(CASES["mixed"])
    sb, _, ban_center, gen = Hh.wide_inputs()
    torch.manual_seed(d["seed"])
    model = sc.SimpleConv(in_channels={"meg": d["C"]}, out_channels=builder.output_dimension,
                          hidden={"meg": d["hidden"]}, n_subjects=d["S"], **Hh.WIDE_CFG)
    Hh.randomize_batchnorm(model, gen)
    tgen = torch.Generator().manual_seed(d["seed"] + 11)
    features = targets(builder, d["B"], d["T"], tgen)
    weights = class_weights(builder, tgen)
    mask = partial_row_mask(d["B"], d["T"], tgen)
    loss_mod = losses.FeatureDecodingLoss(builder, Weights(weights))
    optim = torch.optim.Adam(model.parameters(), lr=3e-4, betas=(0.9, 0.999))
    model.train(True)
    batch = _Batch(sb)
    common.PositionGetter.get_positions = lambda self, b: b._positions.clone()
    real_rand = torch.rand

    def fake_rand(*a, **k):
        if a == (2,):
            return ban_center.clone()
        return real_rand(*a, **k)

    p = "train/"
    res = {}
    for k, v in model.state_dict().items():
        res[f"{p}sd0_digest/{k}"] = Hh.tensor_digest(v)
    res[f"{p}in_digest/meg"] = Hh.tensor_digest(sb.meg)
    res[f"{p}in/features"] = features.numpy().copy()
    res[f"{p}in/mask"] = mask.numpy().copy()
    for name, w in weights.items():
        res[f"{p}in/weights/{name}"] = w.numpy().copy()
    common.torch.rand = fake_rand
    try:
        seen = []
        for step in range(2):
            estimate = model({"meg": sb.meg.clone()}, batch)
            loss = loss_mod(estimate, features, mask)
            optim.zero_grad()
            loss.backward()
            if step == 0:
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
    from make_regression_golden import partial_row_mask
    M = _ref_metrics()
    d = METRIC_SHAPE
    B, K, T, trim = d["B"], d["K"], d["T"], d["trim"]
    gen = torch.Generator().manual_seed(78)
    res = {}
    ctor = M.ClassificationAcc.get_constructor(slice(0, K), slice(0, 1), name="acc_ph")
    results = []
    for r in range(d["recordings"]):
        metric = ctor()
        for i in range(d["batches"]):
            gt = torch.randint(0, K, (B, 1, T), generator=gen).float()
            est = torch.randn(B, K, T, generator=gen)
            right = torch.rand(B, 1, T, generator=gen) < 0.5            # about half the positions are classified right
            est.scatter_add_(1, gt.long(), 3.0 * right.float())
            mask = partial_row_mask(B, T, gen)
            mask[0] = True                                          # every column keeps a sample
            res[f"metrics/in/{r}/{i}/est"] = est.numpy()
            res[f"metrics/in/{r}/{i}/gt"] = gt.numpy()
            res[f"metrics/in/{r}/{i}/mask"] = mask.numpy()
            metric.update(est[..., trim:].to(torch.double), gt[..., trim:].to(torch.double), mask[..., trim:])
        value = metric.get()
        res[f"metrics/get/{r}/acc_ph"] = value.numpy().copy()
        results.append(value.cpu().float())
    res["metrics/reduce/acc_ph"] = np.array(ctor().reduce(results), dtype=np.float64)
    return res


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    sc, common, losses = load_reference()
    out = {"meta": json.dumps(dict(loss_shape=LOSS_SHAPE, metric_shape=METRIC_SHAPE, torch=torch.__version__,
                                   cases={k: [list(f) for f in v] for k, v in CASES.items()}))}
    out.update(loss_fixture(losses))
    out.update(train_fixture(sc, common, losses))
    out.update(metrics_fixture())
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "feature_decoding.npz", **out)
    print(f"feature_decoding: {len(out)} arrays -> {dest / 'feature_decoding.npz'}")


if __name__ == "__main__":
    main(sys.argv[1:])
