"""Golden vectors of ConvRNN, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_convrnn_golden.py [output directory]
Writes ``convrnn.npz`` (default: next to this file).  Every case of ``CASES`` is a reference ``ConvRNN`` built from the
case's seed; stored per case:

  ``<case>/keys``          the state_dict keys in the reference's order, ``<case>/shapes`` their shapes (JSON)
  ``<case>/sd/<key>``      exact digest (tests/helpers.py ``tensor_digest``) of every state_dict tensor before the pass
                           (BatchNorm tensors randomised after construction), ``<case>/in/<name>`` of every input:
                           19 models and their inputs do not fit the size of a fixture, so both sides rebuild them from
                           the seed (``build_model`` / ``make_input``, as wide_kernels_train.npz does) and the digests
                           prove that they did
  ``<case>/table/<key>``   the relative-position tables of Attention in full: their smoothing is a running sum, whose
                           last bits depend on the host's vector width, so a rebuilt model takes them from here
                           (``load_stored_tables``) and matches them to round-off when it builds them itself
  ``<case>/subjects``      the subject indices
  ``<case>/y``             the output
  ``<case>/gin/<name>``    gradient of <y, cotangent> with respect to every input, ``<case>/grad/<key>`` to every
                           parameter (cotangent = ``cotangent(case, y.shape)``)
  ``<case>/after/<key>``   BatchNorm buffers after the pass (training-mode cases)
  ``<case>/valid_length``  [length, valid_length(length)] pairs

Result tensors (``y``, ``gin``, ``grad``, the after-step parameters) of more than ``SAMPLE`` elements are stored as
``<key>@norm`` (fp64 L2 norm), ``<key>@max`` and ``<key>@sample`` (the elements at ``sample_indices(numel)``: a fixed
random subset without repetition); smaller ones in full.  ``stored()`` reads either form back.

and for the two training cases (``TRAIN_CASES``: two Adam steps of the live reference model under the reference's
ClipLoss / L2Loss): ``<case>/features``, both losses, the step-0 gradients and the parameters after the two steps.

While it runs, the generator asserts for every case that ``brainmagick_amd.models.ConvRNN`` built from the same seed
has the reference's state_dict: same keys, same order, bit-equal values.

``CASES``, ``TRAIN_CASES``, ``build_model``, ``make_input``, ``make_subjects`` and ``cotangent`` are what
tests/test_convrnn_{cpu,gpu}.py import to rebuild the same models from ``brainmagick_amd.models.ConvRNN``.
"""
import importlib
import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
B = 6
S = 4            # subjects
F_OUT = 11       # output channels
LR = 3e-4

# name -> dict(inputs={name: channels}, hidden={name: width}, T=input length, train=bool, kw=ConvRNN keywords)
_MEG = dict(inputs=dict(meg=20), hidden=dict(meg=24), T=100, train=True)
CASES = {
    "defaults": dict(_MEG, kw=dict(lstm=4)),
    "bidirectional": dict(_MEG, kw=dict(lstm=2, bidirectional_lstm=True)),
    "flip": dict(_MEG, kw=dict(flip_lstm=True)),
    "no_lstm": dict(_MEG, kw=dict(lstm=0, embedding_location=["input"])),
    "embedding_input": dict(_MEG, kw=dict(embedding_location=["input"])),
    "embedding_both": dict(_MEG, kw=dict(embedding_location=["input", "lstm"], subject_dim=8, embedding_scale=2.0)),
    "no_subject": dict(_MEG, kw=dict(subject_dim=0)),
    "subject_layers_hidden": dict(_MEG, kw=dict(subject_layers=True, subject_layers_dim="hidden")),
    "linear_out": dict(_MEG, kw=dict(linear_out=True)),
    "complex_out": dict(_MEG, kw=dict(complex_out=True)),
    "growth": dict(_MEG, kw=dict(growth=1.5)),
    "bn_train": dict(_MEG, kw=dict(batch_norm=True)),
    "bn_eval": dict(_MEG, train=False, kw=dict(batch_norm=True)),
    "leaky": dict(_MEG, kw=dict(relu_leakiness=0.1)),
    "attention": dict(_MEG, kw=dict(attention=2, heads=2, batch_norm=True)),
    "two_inputs": dict(inputs=dict(meg=20, features=7), hidden=dict(meg=24, features=8), T=100, train=True,
                       kw=dict(bidirectional_lstm=True)),
    "two_inputs_concatenate": dict(inputs=dict(meg=20, features=7), hidden=dict(meg=24, features=8), T=100, train=True,
                                   kw=dict(concatenate=True)),
    "depth3": dict(inputs=dict(meg=20), hidden=dict(meg=32), T=101, train=True, kw=dict(depth=3, stride=2)),
    "long_attention": dict(inputs=dict(meg=12), hidden=dict(meg=16), T=121, train=True,
                           kw=dict(depth=1, attention=1, heads=4, lstm=1)),       # T' = 62 > radius 50: the band clamps
}
TRAIN_CASES = {
    "train_clip": dict(_MEG, kw=dict(lstm=2, bidirectional_lstm=True), loss="clip"),
    "train_l2": dict(_MEG, kw=dict(lstm=2, batch_norm=True), loss="l2"),
}
VALID_LENGTHS = [1, 2, 7, 100, 101, 102, 360, 361]
SAMPLE = 256


def sample_indices(numel: int) -> torch.Tensor:
    return torch.randperm(numel, generator=torch.Generator().manual_seed(77 + numel))[:SAMPLE]


def put(out: dict, key: str, t: torch.Tensor):
    """Store a result tensor: in full up to SAMPLE elements, else its norm, maximum and a fixed sample."""
    t = t.detach()
    if t.numel() <= SAMPLE:
        out[key] = t.numpy().copy()
        return
    flat = t.flatten()
    out[key + "@norm"] = np.array(float(flat.double().norm()))
    out[key + "@max"] = np.array(float(flat.abs().max()))
    out[key + "@sample"] = flat[sample_indices(flat.numel())].numpy().copy()


def stored(raw: dict, key: str):
    """(full tensor, None, None) or (sample, norm, max) of a tensor written by ``put``."""
    if key in raw:
        return torch.from_numpy(np.array(raw[key])), None, None
    return torch.from_numpy(np.array(raw[key + "@sample"])), float(raw[key + "@norm"]), float(raw[key + "@max"])


def spec_of(name: str) -> dict:
    return CASES[name] if name in CASES else TRAIN_CASES[name]


def case_seed(name: str) -> int:
    return 9090 + sum(map(ord, name))


def randomize_batchnorm(model, gen):
    """tests/helpers.py's recipe: non-trivial BatchNorm affine parameters / running statistics, in module order."""
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5, generator=gen)
                mod.bias.uniform_(-0.3, 0.3, generator=gen)
                mod.running_mean.uniform_(-0.2, 0.2, generator=gen)
                mod.running_var.uniform_(0.5, 1.5, generator=gen)


def build_model(convrnn_cls, name: str) -> torch.nn.Module:
    """The case's ``convrnn_cls`` model from its seed (CPU, fp32), in the case's train / eval mode."""
    spec = spec_of(name)
    torch.manual_seed(case_seed(name))
    model = convrnn_cls(in_channels=dict(spec["inputs"]), out_channels=F_OUT, hidden=dict(spec["hidden"]),
                        n_subjects=S, **spec["kw"])
    randomize_batchnorm(model, torch.Generator().manual_seed(case_seed(name) + 1))
    model.train(spec["train"])
    return model


def make_input(name: str) -> dict:
    spec = spec_of(name)
    gen = torch.Generator().manual_seed(case_seed(name) + 2)
    return {k: torch.randn(B, c, spec["T"], generator=gen) for k, c in spec["inputs"].items()}


def make_subjects(name: str) -> torch.Tensor:
    gen = torch.Generator().manual_seed(case_seed(name) + 4)
    return torch.randint(0, S, (B,), generator=gen)


def make_features(name: str) -> torch.Tensor:
    gen = torch.Generator().manual_seed(case_seed(name) + 5)
    return torch.randn(B, F_OUT, spec_of(name)["T"], generator=gen)


def cotangent(name: str, shape) -> torch.Tensor:
    gen = torch.Generator().manual_seed(case_seed(name) + 3)
    return torch.randn(*shape, generator=gen)


def load_reference_convrnn():
    """(bm.models.convrnn, reference losses) under tests/golden/_ref_import.py's stubs; ``bm/utils.py`` is loaded by
    file path as ``bm.utils`` (it needs numpy and the standard library only)."""
    sys.path.insert(0, str(HERE))
    from _ref_import import REF, load_reference
    _, _, losses = load_reference()
    if "bm.utils" not in sys.modules:
        spec = importlib.util.spec_from_file_location("bm.utils", REF / "bm" / "utils.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["bm.utils"] = mod
        spec.loader.exec_module(mod)
    return importlib.import_module("bm.models.convrnn"), losses


def _assert_same_construction(name: str, ref_model):
    sys.path.insert(0, str(HERE.parent.parent))
    from brainmagick_amd.models import ConvRNN
    ours = build_model(ConvRNN, name).state_dict()
    theirs = ref_model.state_dict()
    assert list(ours.keys()) == list(theirs.keys()), (name, list(ours.keys()), list(theirs.keys()))
    for k in theirs:
        assert ours[k].shape == theirs[k].shape and ours[k].dtype == theirs[k].dtype, (name, k)
        assert torch.equal(ours[k], theirs[k]), (name, k)


def is_table(key: str) -> bool:
    return key.startswith("attentions.") and key.endswith(".embedding.weight")


def load_stored_tables(model, raw: dict, name: str):
    """Put the fixture's Attention tables into a rebuilt model (everything else is bit-equal by construction)."""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if is_table(k):
                v.copy_(torch.from_numpy(np.array(raw[f"{name}/table/{k}"])))


def _store_state(out, name, model):
    sys.path.insert(0, str(HERE.parent))
    from helpers import tensor_digest
    sd = model.state_dict()
    out[f"{name}/keys"] = np.array(json.dumps(list(sd.keys())))
    out[f"{name}/shapes"] = np.array(json.dumps([list(v.shape) for v in sd.values()]))
    for k, v in sd.items():
        out[f"{name}/sd/{k}"] = tensor_digest(v)
        if is_table(k):
            out[f"{name}/table/{k}"] = v.numpy().copy()
    for k, v in make_input(name).items():
        out[f"{name}/in/{k}"] = tensor_digest(v)


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    convrnn, losses = load_reference_convrnn()
    sys.path.insert(0, str(HERE.parent))
    from helpers import tensor_digest
    out = {"meta": json.dumps(dict(cases=list(CASES), train_cases=list(TRAIN_CASES), B=B, S=S, F=F_OUT, lr=LR,
                                   torch=torch.__version__))}
    for name, spec in CASES.items():
        model = build_model(convrnn.ConvRNN, name)
        _assert_same_construction(name, model)
        _store_state(out, name, model)
        inputs = {k: v.requires_grad_(True) for k, v in make_input(name).items()}
        subjects = make_subjects(name)
        y = model(dict(inputs), types.SimpleNamespace(subject_index=subjects))
        assert y.shape == (B, F_OUT, spec["T"]), y.shape
        assert model.valid_length(spec["T"]) != spec["T"], name          # the crop and the padding do something
        (y * cotangent(name, y.shape)).sum().backward()
        out[f"{name}/subjects"] = subjects.numpy().copy()
        put(out, f"{name}/y", y)
        for k, v in inputs.items():
            put(out, f"{name}/gin/{k}", v.grad)
        for k, p in model.named_parameters():
            put(out, f"{name}/grad/{k}", p.grad)
        if spec["train"]:
            for k, v in model.named_buffers():
                out[f"{name}/after/{k}"] = v.numpy().copy()
        out[f"{name}/valid_length"] = np.array([[n, model.valid_length(n)] for n in VALID_LENGTHS], dtype=np.int64)
    for name, spec in TRAIN_CASES.items():
        model = build_model(convrnn.ConvRNN, name)
        _assert_same_construction(name, model)
        _store_state(out, name, model)
        meg = make_input(name)["meg"]
        subjects = make_subjects(name)
        features = make_features(name)
        mask = torch.ones(B, 1, spec["T"], dtype=torch.bool)
        loss_mod = losses.ClipLoss() if spec["loss"] == "clip" else losses.L2Loss()
        optim = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
        seen = []
        for step in range(2):
            estimate = model({"meg": meg.clone()}, types.SimpleNamespace(subject_index=subjects))
            loss = loss_mod(estimate, features, mask)
            optim.zero_grad()
            loss.backward()
            if step == 0:
                put(out, f"{name}/y", estimate)
                for k, p in model.named_parameters():
                    put(out, f"{name}/grad/{k}", p.grad)
            optim.step()
            seen.append(float(loss.detach()))
        out[f"{name}/subjects"] = subjects.numpy().copy()
        out[f"{name}/features"] = tensor_digest(features)
        out[f"{name}/losses"] = np.asarray(seen, dtype=np.float64)
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                put(out, f"{name}/sd1/{k}", v)
            else:
                out[f"{name}/sd1/{k}"] = v.numpy().copy()
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "convrnn.npz", **out)
    print(f"convrnn: {len(out)} arrays -> {dest / 'convrnn.npz'} ({(dest / 'convrnn.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
