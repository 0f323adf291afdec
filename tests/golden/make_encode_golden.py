"""Golden vectors of the encode task, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_encode_golden.py [output directory]
Writes ``encode.npz`` (default: next to this file).

The reference ``Solver`` cannot be imported (flashy, dora), so the body of ``Solver._process_batch`` is taken from
``bm/solver.py`` by AST and run, unmodified, against a stub ``self`` (``args.task``, ``args.dset.sample_rate``,
``lowpass: 0``; ``reference_process_batch``).  Around it the statements of ``_run_one_epoch`` (bm/solver.py:344-387):
the reference's L1Loss / L2Loss, ``torch.optim.Adam``; for the test metrics those of ``bm/play.py:140-154`` with the
reference's OnlineCorrelation.

``TRAIN_CASES`` (two Adam steps each, training mode; no dropout anywhere):

  ``convrnn_l1``                  ConvRNN {meg: 20, features: 7} -> 20, T = 100, sample_rate 100, meg_init 0.13
                                  (limit 13, no multiple of 4), L1
  ``convrnn_l1_offset_mask``      the same with offset_meg_ms = 50 and mask_loss under a mask with holes
  ``simpleconv_mse``              two-input SimpleConv, T = 96, sample_rate 120, meg_init 0.3 (limit 36), MSE
  ``simpleconv_mse_concatenate``  the same with ``concatenate``

Stored per case: ``<case>/sd/<key>`` and ``<case>/in/<name>`` digests (tests/helpers.py ``tensor_digest``) of the initial
state_dict and of the inputs -- both sides rebuild them from the seed (``build_model`` / ``make_batch``) -- the mask
in full, ``<case>/limit``, ``<case>/count`` (selected elements of the loss), ``<case>/losses`` [2], and, sampled as
make_convrnn_golden.py's ``put`` does, ``<case>/y`` (the step-0 estimate AFTER the reference's ``[..., limit:]``),
``<case>/grad/<key>`` (step 0) and ``<case>/sd1/<key>`` (after the two steps).

``metrics/*`` (``METRICS``): ``corr_meg`` over two recordings of three batches each through ``_process_batch`` of the
``simpleconv_mse`` model in eval mode, trimmed by ``trim_offset`` = bm/solver.py:436-439 at tmin = -0.5: the estimates
the reference's ``_process_batch`` returned (``metrics/est/<r>/<i>``, the inputs are rebuilt from the seed), the
per-recording ``get()`` and the ``reduce()`` value.

While it runs, the generator asserts that the models of ``brainmagick_amd.models`` built from the same seeds have the
reference's state_dicts, bit for bit.
"""
import ast
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

from make_convrnn_golden import put, randomize_batchnorm  # noqa: E402
from make_regression_golden import partial_row_mask  # noqa: E402

LR = 3e-4
_CONVRNN = dict(model="convrnn", inputs=dict(meg=20, features=7), hidden=dict(meg=24, features=8), B=6, S=4, T=100,
                sample_rate=100., meg_init=0.13, kw=dict(), loss="l1", offset_meg_ms=0., mask_loss=False)
_SIMPLECONV_CFG = dict(depth=4, kernel_size=3, dilation_growth=2, dilation_period=5, batch_norm=True, skip=True,
                       gelu=True, glu=2, glu_context=1, glu_glu=True, complex_out=True, merger=False, initial_linear=12,
                       initial_depth=1, subject_layers=True, subject_layers_dim="input", subject_dim=0)
_SIMPLECONV = dict(model="simpleconv", inputs=dict(meg=20, features=6), hidden=dict(meg=16, features=8), B=6, S=5, T=96,
                   sample_rate=120., meg_init=0.3, kw=_SIMPLECONV_CFG, loss="mse", offset_meg_ms=0., mask_loss=False)
TRAIN_CASES = {
    "convrnn_l1": _CONVRNN,
    "convrnn_l1_offset_mask": dict(_CONVRNN, offset_meg_ms=50., mask_loss=True),
    "simpleconv_mse": _SIMPLECONV,
    "simpleconv_mse_concatenate": dict(_SIMPLECONV, kw=dict(_SIMPLECONV_CFG, concatenate=True, complex_out=False,
                                                            linear_out=True)),
}
METRICS = dict(case="simpleconv_mse", B=4, recordings=2, batches=3, tmin=-0.5)


def case_seed(name: str) -> int:
    return 5150 + sum(map(ord, name))


def build_model(classes: dict, name: str) -> torch.nn.Module:
    """The case's model from its seed (CPU, fp32): ``classes`` = {"convrnn": ConvRNN, "simpleconv": SimpleConv} of the
    reference or of brainmagick_amd.models.  The output is the MEG: as many channels as the ``meg`` input."""
    spec = TRAIN_CASES[name]
    torch.manual_seed(case_seed(name))
    model = classes[spec["model"]](in_channels=dict(spec["inputs"]), out_channels=spec["inputs"]["meg"],
                                   hidden=dict(spec["hidden"]), n_subjects=spec["S"], **spec["kw"])
    randomize_batchnorm(model, torch.Generator().manual_seed(case_seed(name) + 1))
    return model


def make_batch(name: str, index: int = 0, B=None):
    """Batch ``index`` of the case (brainmagick_amd.synthetic.SegmentBatch, CPU): MEG, features, a mask with holes
    (every segment loses one run of samples) and subject indices from the seed."""
    from brainmagick_amd.synthetic import SegmentBatch
    spec = TRAIN_CASES[name]
    B = B or spec["B"]
    gen = torch.Generator().manual_seed(case_seed(name) + 2 + 10 * index)
    meg = torch.randn(B, spec["inputs"]["meg"], spec["T"], generator=gen)
    features = torch.randn(B, spec["inputs"]["features"], spec["T"], generator=gen)
    mask = partial_row_mask(B, spec["T"], gen)
    subjects = torch.randint(0, spec["S"], (B,), generator=gen)
    return SegmentBatch(meg, features, mask, subjects, torch.zeros(B, dtype=torch.int64))


class _Cfg(dict):
    """The attribute / item / ``in`` access of the reference's configuration objects."""
    __getattr__ = dict.__getitem__


def reference_process_batch():
    """``Solver._process_batch`` of bm/solver.py as a plain function of (self, batch, training)."""
    from _ref_import import REF
    path = REF / "bm" / "solver.py"
    tree = ast.parse(path.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Solver")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_process_batch")
    fn.decorator_list = []
    fn.returns = None
    for arg in fn.args.args:
        arg.annotation = None
    scope = {"torch": torch, "F": torch.nn.functional}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), str(path), "exec"), scope)
    return scope["_process_batch"]


def stub_solver(name: str, model):
    spec = TRAIN_CASES[name]
    task = _Cfg(type="encode", meg_init=spec["meg_init"], mask_loss=spec["mask_loss"], lowpass=0, lowpass_gt=False,
                lowpass_gt_test=False, offset_meg_ms=spec["offset_meg_ms"])
    args = _Cfg(task=task, dset=_Cfg(sample_rate=spec["sample_rate"]))
    return types.SimpleNamespace(args=args, device="cpu", scale_reject=None, model=model, feature_model=None)


def _reference_classes():
    from make_convrnn_golden import load_reference_convrnn
    from _ref_import import REF, load_reference
    convrnn, losses = load_reference_convrnn()
    simpleconv, _, _ = load_reference()
    if "bm_ref_metrics" not in sys.modules:
        spec = importlib.util.spec_from_file_location("bm_ref_metrics", REF / "bm" / "metrics.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["bm_ref_metrics"] = mod
        spec.loader.exec_module(mod)
    return dict(convrnn=convrnn.ConvRNN, simpleconv=simpleconv.SimpleConv), losses, sys.modules["bm_ref_metrics"]


def _assert_same_construction(name: str, ref_model):
    from brainmagick_amd.models import ConvRNN, SimpleConv
    ours = build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), name).state_dict()
    theirs = ref_model.state_dict()
    assert list(ours.keys()) == list(theirs.keys()), (name, list(ours.keys()), list(theirs.keys()))
    for k in theirs:
        assert ours[k].dtype == theirs[k].dtype and torch.equal(ours[k], theirs[k]), (name, k)


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    from helpers import tensor_digest
    classes, losses, ref_metrics = _reference_classes()
    process_batch = reference_process_batch()
    out = {}
    limits = {}
    for name, spec in TRAIN_CASES.items():
        model = build_model(classes, name)
        _assert_same_construction(name, model)
        model.train(True)
        batch = make_batch(name)
        for k, v in model.state_dict().items():
            out[f"{name}/sd/{k}"] = tensor_digest(v)
        out[f"{name}/in/meg"] = tensor_digest(batch.meg)
        out[f"{name}/in/features"] = tensor_digest(batch.features)
        out[f"{name}/mask"] = batch.features_mask.numpy().copy()
        out[f"{name}/subjects"] = batch.subject_index.numpy().copy()
        solver = stub_solver(name, model)
        loss_mod = losses.L1Loss() if spec["loss"] == "l1" else losses.L2Loss()
        optim = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
        seen = []
        for step in range(2):
            estimate, output, features_mask, _ = process_batch(solver, batch, True)
            assert features_mask.any()
            loss = loss_mod(estimate, output, features_mask)
            optim.zero_grad()
            loss.backward()
            if step == 0:
                limit = batch.meg.shape[-1] - int(spec["offset_meg_ms"] / 1000 * spec["sample_rate"]) - \
                    estimate.shape[-1]
                limits[name] = limit
                out[f"{name}/limit"] = np.array(limit, dtype=np.int64)
                out[f"{name}/count"] = np.array(int(features_mask.expand_as(estimate).sum()), dtype=np.int64)
                put(out, f"{name}/y", estimate)
                for k, p in model.named_parameters():
                    put(out, f"{name}/grad/{k}", p.grad)
            optim.step()
            seen.append(float(loss.detach()))
        out[f"{name}/losses"] = np.asarray(seen, dtype=np.float64)
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                put(out, f"{name}/sd1/{k}", v)
            else:
                out[f"{name}/sd1/{k}"] = v.numpy().copy()
    # test metrics: bm/play.py:133-154 around _process_batch, bm/solver.py:408-409 and 436-439
    d = METRICS
    name = d["case"]
    spec = TRAIN_CASES[name]
    model = build_model(classes, name)
    model.train(False)
    solver = stub_solver(name, model)
    time_offset = -d["tmin"]
    time_offset -= spec["meg_init"]
    trim_offset = int(spec["sample_rate"] * time_offset)
    out["metrics/trim_offset"] = np.array(trim_offset, dtype=np.int64)
    ctors = [ref_metrics.OnlineCorrelation.get_constructor(slice(None), slice(None), "corr_meg")]
    results = {c().name: [] for c in ctors}
    for r in range(d["recordings"]):
        metrics = [c() for c in ctors]
        for i in range(d["batches"]):
            batch = make_batch(name, 1 + r * d["batches"] + i, d["B"])
            out[f"metrics/in/{r}/{i}/meg"] = tensor_digest(batch.meg)
            with torch.no_grad():
                estimate, gt, features_mask, _ = process_batch(solver, batch)
            assert torch.equal(gt, batch.meg[..., limits[name]:]) and bool(features_mask.all())
            out[f"metrics/est/{r}/{i}"] = estimate.numpy().copy()
            estimate = estimate[..., trim_offset:]
            gt = gt[..., trim_offset:]
            features_mask = features_mask[..., trim_offset:]
            for metric in metrics:
                metric.update(estimate.to(torch.double), gt.to(torch.double), features_mask)
        for metric in metrics:
            value = metric.get()
            out[f"metrics/get/{r}/{metric.name}"] = value.numpy().copy()
            results[metric.name].append(value.cpu().float())
    for c in ctors:
        metric = c()
        out[f"metrics/reduce/{metric.name}"] = np.array(metric.reduce(results[metric.name]), dtype=np.float64)
    cases = {k: {f: v[f] for f in ("model", "inputs", "hidden", "B", "S", "T", "sample_rate", "meg_init", "loss",
                                   "offset_meg_ms", "mask_loss")} for k, v in TRAIN_CASES.items()}
    out["meta"] = json.dumps(dict(cases=cases, metrics=METRICS, lr=LR, torch=torch.__version__))
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "encode.npz", **out)
    print(f"encode: {len(out)} arrays -> {dest / 'encode.npz'} ({(dest / 'encode.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
