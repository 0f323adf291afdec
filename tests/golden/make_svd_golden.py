"""Golden vectors of ``optim.svd``, from the REAL reference ``bm/svd.py`` (read-only /root/reference).

Run in the build container only:   python tests/golden/make_svd_golden.py [output directory]
Writes ``svd_penalty.npz`` (default: next to this file).

``torch.svd_lowrank`` draws its Gaussian test matrix with ``torch.randn``; for the duration of a reference call that
function is wrapped, so the fixture holds the ``R`` of every penalised weight, and an fp64 run of the same reference code
is fed the same ``R``.

``CASES`` -- one layer each, the weight ``randn(shape) / sqrt(columns)`` from the case's seed (``make_weight``; proven
by a digest) or, for the two ``spectrum`` cases, ``U diag(base ** i) V^T`` (stored: it comes out of a QR):

  per case  ``<case>/R`` fp32, ``<case>/value32`` (the reference's fp32 estimate), ``<case>/value64`` and
            ``<case>/grad64`` (the reference in fp64 with the same R; fp32 storage for ``gauss_160x480``, which would not
            fit the size limit of a committed file otherwise), ``<case>/w_digest`` or ``<case>/w``;
  meta      ``dev`` = {case: [|value32 - value64| / value64, |grad32 - grad64| / |grad64|]}: the reference's own fp32
            distance from fp64, the yardstick of the GPU tests; ``dev_median`` = the medians over ``CASES``.

``VARIANTS``: ``lin_40x17`` with dim = 8 / niters = 1 and with niters = 0.  ``proba``: eight consecutive calls with
proba = 0.5 from a fresh ``penalty_rng``: which were applied, and the value of an applied call over the estimate.
``names``: what the reference penalises in the SimpleConv of make_lowpass_golden.py's ``decode_mse`` and the ConvRNN
of ``encode_l1_gt``.  ``train``: two Adam steps of that SimpleConv on the decode task with the MSE loss and svd = 0.1,
the loop body of bm/solver.py:373-387 composed here (flashy is absent): ``train/R/<step>/<i>``, ``train/losses``,
``train/grad/<key>`` (step 0) and ``train/sd<step + 1>/<key>``.
"""
import copy
import importlib.util
import json
import math
import random
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))
sys.path.insert(2, str(HERE.parent.parent))

SVD = 0.1
TRAIN_CASE, TRAIN_BATCH, RNN_CASE = "decode_mse", "simpleconv_mse", "encode_l1_gt"
CASES = {
    "lin_16x16": dict(layer=("linear", 16, 16)),                       # numel / 256 == 1: the smallest penalised weight
    "depthwise_300x1x1": dict(layer=("conv", 300, 300, 1, 300)),       # n' = 1
    "lin_273x16": dict(layer=("linear", 16, 273)),                     # min == q
    "lin_8x64": dict(layer=("linear", 64, 8)),                         # min < q, wide
    "lin_40x17": dict(layer=("linear", 17, 40)),                       # first size on the iterated branch
    "lin_17x300": dict(layer=("linear", 300, 17)),                     # wide on the iterated branch
    "conv_45x23x3": dict(layer=("conv", 23, 45, 3, 1)),                # 3-D view, ragged tiles
    "convtr_24x40x4": dict(layer=("convtr", 24, 40, 4, 1)),            # [in, out, k]
    "conv_groups_64x8x3": dict(layer=("conv", 32, 64, 3, 4)),          # [out, in / groups, k]
    "spectrum_0.5": dict(layer=("linear", 160, 96), spectrum=0.5),     # fp32 Gram matrices break here
    "spectrum_0.9": dict(layer=("linear", 160, 96), spectrum=0.9),     # gapped, converged
    "gauss_160x480": dict(layer=("linear", 480, 160), grad_fp32=True),  # one real layer's shape / 2, un-gapped
}
VARIANTS = {
    "lin_40x17/dim8_niters1": dict(case="lin_40x17", dim=8, niters=1),
    "lin_40x17/niters0": dict(case="lin_40x17", niters=0),
}
SKIPPED = ("linear", 17, 15)                                           # numel < 256: not penalised


def case_seed(name: str) -> int:
    return 7300 + sum(map(ord, name))


def make_layer(spec) -> torch.nn.Module:
    kind = spec[0]
    if kind == "linear":
        return torch.nn.Linear(spec[1], spec[2])
    cls = torch.nn.Conv1d if kind == "conv" else torch.nn.ConvTranspose1d
    return cls(spec[1], spec[2], spec[3], groups=spec[4])


def make_weight(name: str) -> torch.Tensor:
    """The case's weight (fp32, CPU) from its seed; the spectrum cases are read from the fixture instead."""
    shape = make_layer(CASES[name]["layer"]).weight.shape
    gen = torch.Generator().manual_seed(case_seed(name))
    cols = math.prod(shape[1:])
    base = CASES[name].get("spectrum")
    if base is None:
        return torch.randn(shape, generator=gen) / math.sqrt(cols)
    rows = shape[0]
    u = torch.linalg.qr(torch.randn(rows, rows, generator=gen, dtype=torch.float64))[0]
    v = torch.linalg.qr(torch.randn(cols, rows, generator=gen, dtype=torch.float64))[0]
    s = base ** torch.arange(rows, dtype=torch.float64)
    return ((u * s) @ v.t()).to(torch.float32).view(shape)


def case_model(name: str, weight: torch.Tensor) -> torch.nn.Module:
    layer = make_layer(CASES[name]["layer"])
    with torch.no_grad():
        layer.weight.copy_(weight)
    return torch.nn.Sequential(layer)


def load_reference_svd():
    from _ref_import import REF
    if "bm_ref_svd" not in sys.modules:
        spec = importlib.util.spec_from_file_location("bm_ref_svd", REF / "bm" / "svd.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["bm_ref_svd"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["bm_ref_svd"]


class RandnTap:
    """``torch.randn`` for the duration of the block: records what it returns, or -- with ``replay`` -- returns those
    tensors in the dtype asked for."""

    def __init__(self, replay=None):
        self.replay, self.seen = replay, []

    def __enter__(self):
        self.orig = torch.randn

        def randn(*size, **kw):
            if self.replay is None:
                out = self.orig(*size, **kw)
            else:
                out = self.replay[len(self.seen)].to(kw.get("dtype") or torch.float32)
                assert tuple(out.shape) == tuple(size), (out.shape, size)
            self.seen.append(out.detach().clone())
            return out
        torch.randn = randn
        return self

    def __exit__(self, *exc):
        torch.randn = self.orig
        return False


def reference_penalty(svd_mod, model, dtype=torch.float32, replay=None, **kw):
    """(value, [gradient per parameter of ``model`` or None], [R per penalised weight]) of the reference's
    ``svd_penalty(model, **kw)`` on a copy of ``model`` in ``dtype``."""
    model = copy.deepcopy(model).to(dtype)
    with RandnTap(replay) as tap:
        total = svd_mod.svd_penalty(model, **kw)
    params = list(model.parameters())
    if not isinstance(total, torch.Tensor):
        return total, [None] * len(params), tap.seen
    grads = torch.autograd.grad(total, params, allow_unused=True)
    return total.detach(), list(grads), tap.seen


def reference_names(svd_mod, model):
    """Names of the weights the reference hands to ``torch.svd_lowrank``, in its order."""
    by_ptr = {p.data_ptr(): k for k, p in model.named_parameters()}
    seen = []
    orig = torch.svd_lowrank

    def spy(p, *a, **kw):
        seen.append(by_ptr[p.data_ptr()])
        return orig(p, *a, **kw)
    torch.svd_lowrank = spy
    try:
        svd_mod.svd_penalty(model)
    finally:
        torch.svd_lowrank = orig
    return seen


def rel(a, b) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def build() -> dict:
    torch.set_num_threads(1)
    from helpers import tensor_digest
    import make_encode_golden as E
    import make_lowpass_golden as LPG
    svd_mod = load_reference_svd()
    out, dev = {}, {}

    def one(key, name, **kw):
        weight = make_weight(name)
        model = case_model(name, weight)
        torch.manual_seed(case_seed(key) + 1)                             # the draw of R
        v32, g32, R = reference_penalty(svd_mod, model, **kw)
        v64, g64, _ = reference_penalty(svd_mod, model, torch.float64, replay=R, **kw)
        assert len(R) == 1
        out[f"{key}/R"] = R[0].numpy().copy()
        out[f"{key}/value32"] = np.asarray(float(v32), dtype=np.float32)
        out[f"{key}/value64"] = np.asarray(float(v64), dtype=np.float64)
        keep = np.float32 if CASES[name].get("grad_fp32") else np.float64
        out[f"{key}/grad64"] = g64[0].numpy().astype(keep)
        dev[key] = [abs(float(v32) - float(v64)) / float(v64), rel(g32[0], g64[0])]
        return weight

    for name, case in CASES.items():
        weight = one(name, name)
        if case.get("spectrum") is None:
            out[f"{name}/w_digest"] = tensor_digest(weight)
        else:
            out[f"{name}/w"] = weight.numpy().copy()
    for key, var in VARIANTS.items():
        one(key, var["case"], **{k: v for k, v in var.items() if k != "case"})
    dev_median = [float(np.median([dev[k][i] for k in CASES])) for i in range(2)]

    # the skipped weight: the reference returns the float 0 and draws nothing
    skipped = torch.nn.Sequential(make_layer(SKIPPED))
    v, _, R = reference_penalty(svd_mod, skipped)
    assert v == 0 and not R

    # proba: the penalty_rng sequence is data
    svd_mod.penalty_rng = random.Random(1234)
    model = case_model("lin_16x16", make_weight("lin_16x16"))
    applied, ratio = [], []
    torch.manual_seed(case_seed("proba"))
    for _ in range(8):
        v, _, R = reference_penalty(svd_mod, model, proba=0.5)
        applied.append(bool(R))
        if R:
            state = svd_mod.penalty_rng.getstate()            # (the estimate itself: a call that draws too)
            full, _, _ = reference_penalty(svd_mod, model, replay=R)
            svd_mod.penalty_rng.setstate(state)
            ratio.append(float(v) / float(full))
        else:
            assert v == 0.
    svd_mod.penalty_rng = random.Random(1234)
    out["proba/applied"] = np.asarray(applied)
    out["proba/ratio"] = np.asarray(ratio, dtype=np.float64)

    # names, and two training steps of the SimpleConv
    classes, losses, _ = E._reference_classes()
    names = {}
    for tag, case in (("simpleconv", TRAIN_CASE), ("convrnn", RNN_CASE)):
        model = LPG.build_model(classes, case)
        LPG._assert_same_construction(case, model)
        names[tag] = reference_names(svd_mod, model)
    model = LPG.build_model(classes, TRAIN_CASE)
    model.train(True)
    batch = E.make_batch(TRAIN_BATCH)
    for k, v in model.state_dict().items():
        out[f"train/sd/{k}"] = tensor_digest(v)
    out["train/in/meg"] = tensor_digest(batch.meg)
    out["train/in/features"] = tensor_digest(batch.features)
    solver = LPG.stub_solver(TRAIN_CASE, model, lowpass=0., offset_meg_ms=0.)
    process_batch = LPG.reference_process_batch()
    loss_mod = losses.L2Loss()
    optim = torch.optim.Adam(model.parameters(), lr=E.LR, betas=(0.9, 0.999))
    seen = []
    torch.manual_seed(case_seed("train"))
    for step in range(2):
        estimate, output, features_mask, _ = process_batch(solver, batch, True)
        loss = loss_mod(estimate, output, features_mask)                  # bm/solver.py:373
        for mod in model.modules():                                       # bm/solver.py:375-378
            if hasattr(mod, "training_penalty"):
                loss += mod.training_penalty.to(loss.device)
        with RandnTap() as tap:
            loss += SVD * svd_mod.svd_penalty(solver.model.model)         # bm/solver.py:379-380
        assert len(tap.seen) == len(names["simpleconv"])
        for i, R in enumerate(tap.seen):
            out[f"train/R/{step}/{i}"] = R.numpy().copy()
        optim.zero_grad()
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                out[f"train/grad/{k}"] = p.grad.numpy().copy()
        optim.step()
        seen.append(float(loss.detach()))
        for k, v in model.state_dict().items():
            out[f"train/sd{step + 1}/{k}"] = v.numpy().copy()
    out["train/losses"] = np.asarray(seen, dtype=np.float64)
    out["meta"] = json.dumps(dict(cases={k: dict(v, layer=list(v["layer"])) for k, v in CASES.items()},
                                  variants=VARIANTS, dev=dev, dev_median=dev_median, names=names, svd=SVD, lr=E.LR,
                                  train_case=TRAIN_CASE, torch=torch.__version__))
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    path = dest / "svd_penalty.npz"
    np.savez_compressed(path, **out)
    print(f"svd_penalty: {len(out)} arrays -> {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
