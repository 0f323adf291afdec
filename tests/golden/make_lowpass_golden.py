"""Golden vectors of ``task.lowpass``, from the REAL reference ``_process_batch`` (read-only /root/reference).

Run in the build container only:   python tests/golden/make_lowpass_golden.py [output directory]
Writes ``lowpass.npz`` (default: next to this file).

As in make_encode_golden.py the body of ``Solver._process_batch`` is taken from ``bm/solver.py`` by AST and run,
unmodified, against a stub ``self``.  ``julius`` cannot be imported here, so the name ``julius`` in that function's scope
is a namespace whose ``lowpass_filter(x, cutoff, zeros=8)`` RESTATES julius' published formula in fp32 (``restated_taps``
+ ``F.pad(mode="replicate")`` + ``F.conv1d``): the fixture pins the Solver's wiring -- the filter's place relative to
the offset slice, ``meg_gt``, ``meg_init`` and the ``training`` flag -- to the live reference, and the filter to the
restatement.  What the model is handed is recorded by a thin wrapper around the model.

``CASES`` (two Adam steps each, training mode), models / batches of make_encode_golden.py's cases (``base``):

  ``decode_mse``          SimpleConv {meg: 20} -> 6 of ``simpleconv_mse``'s size, MSE, offset_meg_ms 150 (18 samples),
                          lowpass 30 at 120 Hz (half 10)
  ``encode_l1_gt``        ``convrnn_l1``, lowpass 20 at 100 Hz (half 12), lowpass_gt: the target is filtered too
  ``encode_l1_raw_gt``    the same with lowpass_gt = False: the target is the unfiltered MEG
  ``encode_offset_mask``  ``convrnn_l1_offset_mask`` (offset_meg_ms 50, mask_loss), lowpass 20, lowpass_gt

``EVAL_CASES``: ``encode_l1_gt``'s untrained model through ``_process_batch(training=False)`` in eval mode, with
lowpass_gt_test False (unfiltered target) and True.

Stored per case: the digests of the initial state_dict and of the inputs, mask and subjects in full, ``<case>/limit``,
``<case>/losses`` [2] and, sampled as make_convrnn_golden.py's ``put`` does, ``<case>/y`` (step-0 estimate after the
reference's ``[..., limit:]``), ``<case>/meg`` (what the model was handed at step 0, full length), ``<case>/target``
(after ``[..., limit:]``), ``<case>/grad/<key>`` (step 0) and ``<case>/sd1/<key>`` (after the two steps); per eval case
``y``, ``meg`` and ``target``.
"""
import ast
import json
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))
sys.path.insert(2, str(HERE.parent.parent))

import make_encode_golden as E  # noqa: E402
from make_encode_golden import _Cfg, make_batch, put  # noqa: E402
from make_convrnn_golden import randomize_batchnorm  # noqa: E402

LR = E.LR
ZEROS = 5                   # bm/solver.py:279
CASES = {
    "decode_mse": dict(base="simpleconv_mse", task="decode", lowpass=30., lowpass_gt=True, lowpass_gt_test=False,
                       offset_meg_ms=150., mask_loss=False, loss="mse"),
    "encode_l1_gt": dict(base="convrnn_l1", task="encode", lowpass=20., lowpass_gt=True, lowpass_gt_test=False,
                         offset_meg_ms=0., mask_loss=False, loss="l1"),
    "encode_l1_raw_gt": dict(base="convrnn_l1", task="encode", lowpass=20., lowpass_gt=False, lowpass_gt_test=False,
                             offset_meg_ms=0., mask_loss=False, loss="l1"),
    "encode_offset_mask": dict(base="convrnn_l1_offset_mask", task="encode", lowpass=20., lowpass_gt=True,
                               lowpass_gt_test=False, offset_meg_ms=50., mask_loss=True, loss="l1"),
}
EVAL_CASES = {
    "eval_raw_gt": dict(case="encode_l1_gt", lowpass_gt_test=False),
    "eval_gt_test": dict(case="encode_l1_gt", lowpass_gt_test=True),
}


def base_spec(name: str) -> dict:
    return E.TRAIN_CASES[CASES[name]["base"]]


def restated_taps(cutoff: float, zeros: float = 8):
    """(taps, half) of julius' ``LowPassFilter(cutoff, zeros=zeros)``: its expressions, fp32, on the CPU."""
    half = int(zeros / cutoff / 2)
    time = torch.arange(-half, half + 1)
    win = torch.hann_window(2 * half + 1, periodic=False)
    arg = 2 * cutoff * math.pi * time
    sinc = torch.where(arg == 0, 1., torch.sin(arg) / arg)
    taps = 2 * cutoff * win * sinc
    taps /= taps.sum()
    return taps, half


def restated_lowpass_filter(x: torch.Tensor, cutoff: float, zeros: float = 8) -> torch.Tensor:
    """julius.lowpass_filter(x, cutoff, zeros=zeros) with stride 1 and pad=True, as the direct sum in x's dtype."""
    taps, half = restated_taps(cutoff, zeros)
    flat = x.reshape(-1, 1, x.shape[-1])
    out = F.conv1d(F.pad(flat, (half, half), mode="replicate"), taps.to(x.dtype)[None, None])
    return out.reshape(x.shape)


def reference_process_batch():
    """``Solver._process_batch`` of bm/solver.py as a plain function of (self, batch, training), ``julius`` being the
    restatement above."""
    from _ref_import import REF
    path = REF / "bm" / "solver.py"
    tree = ast.parse(path.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Solver")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_process_batch")
    fn.decorator_list = []
    fn.returns = None
    for arg in fn.args.args:
        arg.annotation = None
    scope = {"torch": torch, "F": F, "julius": types.SimpleNamespace(lowpass_filter=restated_lowpass_filter)}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), str(path), "exec"), scope)
    return scope["_process_batch"]


def build_model(classes: dict, name: str) -> torch.nn.Module:
    """The case's model from its seed (CPU, fp32): make_encode_golden.py's for the encode cases; for ``decode_mse`` the
    SimpleConv of ``simpleconv_mse``'s size with the MEG as its only input and the features' channels out."""
    base = CASES[name]["base"]
    if CASES[name]["task"] == "encode":
        return E.build_model(classes, base)
    spec = E.TRAIN_CASES[base]
    torch.manual_seed(E.case_seed(name))
    model = classes[spec["model"]](in_channels=dict(meg=spec["inputs"]["meg"]), out_channels=spec["inputs"]["features"],
                                   hidden=dict(meg=spec["hidden"]["meg"]), n_subjects=spec["S"], **spec["kw"])
    randomize_batchnorm(model, torch.Generator().manual_seed(E.case_seed(name) + 1))
    return model


class Recorder:
    """What the reference's ``self.model(inputs, batch)`` handed over, then the model's answer."""

    def __init__(self, model):
        self.model = model
        self.seen = []

    def __call__(self, inputs, batch):
        self.seen.append({k: v.detach().clone() for k, v in inputs.items()})
        return self.model(inputs, batch)


def stub_solver(name: str, model, **override):
    case = dict(CASES[name], **override)
    spec = base_spec(name)
    task = _Cfg(type=case["task"], meg_init=spec["meg_init"], mask_loss=case["mask_loss"], lowpass=case["lowpass"],
                lowpass_gt=case["lowpass_gt"], lowpass_gt_test=case["lowpass_gt_test"],
                offset_meg_ms=case["offset_meg_ms"])
    args = _Cfg(task=task, dset=_Cfg(sample_rate=spec["sample_rate"]))
    return types.SimpleNamespace(args=args, device="cpu", scale_reject=None, model=Recorder(model), feature_model=None)


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
    classes, losses, _ = E._reference_classes()
    process_batch = reference_process_batch()
    out = {}
    for name, case in CASES.items():
        spec = base_spec(name)
        model = build_model(classes, name)
        _assert_same_construction(name, model)
        model.train(True)
        batch = make_batch(case["base"])
        for k, v in model.state_dict().items():
            out[f"{name}/sd/{k}"] = tensor_digest(v)
        out[f"{name}/in/meg"] = tensor_digest(batch.meg)
        out[f"{name}/in/features"] = tensor_digest(batch.features)
        out[f"{name}/mask"] = batch.features_mask.numpy().copy()
        out[f"{name}/subjects"] = batch.subject_index.numpy().copy()
        solver = stub_solver(name, model)
        loss_mod = losses.L1Loss() if case["loss"] == "l1" else losses.L2Loss()
        optim = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
        seen = []
        for step in range(2):
            estimate, output, features_mask, _ = process_batch(solver, batch, True)
            assert features_mask.any()
            loss = loss_mod(estimate, output, features_mask)
            optim.zero_grad()
            loss.backward()
            if step == 0:
                limit = batch.meg.shape[-1] - int(case["offset_meg_ms"] / 1000 * spec["sample_rate"]) - \
                    estimate.shape[-1]
                out[f"{name}/limit"] = np.array(limit, dtype=np.int64)
                put(out, f"{name}/y", estimate)
                put(out, f"{name}/meg", solver.model.seen[0]["meg"])
                put(out, f"{name}/target", output)
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
    for name, ev in EVAL_CASES.items():
        case = ev["case"]
        model = build_model(classes, case)
        model.train(False)
        solver = stub_solver(case, model, lowpass_gt_test=ev["lowpass_gt_test"])
        with torch.no_grad():
            estimate, output, _, _ = process_batch(solver, make_batch(CASES[case]["base"]), False)
        put(out, f"{name}/y", estimate)
        put(out, f"{name}/meg", solver.model.seen[0]["meg"])
        put(out, f"{name}/target", output)
    cases = {k: dict(v, **{f: base_spec(k)[f] for f in ("model", "inputs", "hidden", "B", "S", "T", "sample_rate",
                                                         "meg_init")}) for k, v in CASES.items()}
    out["meta"] = json.dumps(dict(cases=cases, eval_cases=EVAL_CASES, zeros=ZEROS, lr=LR, torch=torch.__version__))
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "lowpass.npz", **out)
    print(f"lowpass: {len(out)} arrays -> {dest / 'lowpass.npz'} ({(dest / 'lowpass.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
