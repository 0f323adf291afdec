"""Golden vectors of the strided / transposed ConvSequence layers, from the REAL reference code (read-only
/root/reference).

Run in the build container only:   python tests/golden/make_strided_golden.py [output directory]
Writes ``strided_conv.npz`` (default: next to this file).  Every case of ``CASES`` is a chain of reference
``ConvSequence`` modules (one, or an encoder -> decoder pair) built from the case's seed; stored per case:

  ``<case>/sd/<key>``     the state_dict before the pass (BatchNorm tensors randomised after construction)
  ``<case>/x``, ``/y``    input [B, C, T] and output
  ``<case>/gx``           gradient of <y, cotangent> with respect to the input, cotangent = ``cotangent(spec, y.shape)``
  ``<case>/grad/<key>``   the same for every parameter
  ``<case>/after/<key>``  BatchNorm buffers after the pass (training-mode cases)

``CASES``, ``build_model``, ``make_input`` and ``cotangent`` are what tests/test_strided_{cpu,gpu}.py import to rebuild
the same models from ``brainmagick_amd.models.common.ConvSequence``.
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
B = 3


def _valid_length(length: int, depth: int, stride: int) -> int:
    """ConvRNN.valid_length (bm/models/convrnn.py:209-223), restated: the length at which a kernel-4 stride-2 encoder
    followed by the mirrored decoder returns the input length."""
    import math
    for _ in range(depth):
        length = max(math.ceil(length / stride) + 1, 1)
    for _ in range(depth):
        length = (length - 1) * stride
    return int(length)


# name -> dict(stages=[(channels, ConvSequence kwargs), ...], T=input length, train=bool)
CASES = {
    "defaults": dict(stages=[((5, 9, 12, 7), {})], T=130, train=True),
    "defaults_decode": dict(stages=[((12, 9, 6, 3), dict(decode=True, activation_on_last=False))], T=50, train=True),
    "bn_train": dict(stages=[((5, 9, 12, 7), dict(batch_norm=True))], T=129, train=True),
    "bn_train_decode": dict(stages=[((12, 9, 6, 3), dict(batch_norm=True, decode=True, activation_on_last=False))],
                            T=51, train=True),
    "bn_eval": dict(stages=[((5, 9, 12, 7), dict(batch_norm=True))], T=129, train=False),
    "bn_eval_decode": dict(stages=[((12, 9, 6, 3), dict(batch_norm=True, decode=True, activation_on_last=False))],
                           T=51, train=False),
    "leaky": dict(stages=[((6, 10, 8), dict(leakiness=0.1))], T=101, train=True),
    "leaky_decode": dict(stages=[((8, 10, 6), dict(leakiness=0.1, decode=True))], T=50, train=True),
    "groups2": dict(stages=[((6, 12, 16, 8), dict(groups=2, batch_norm=True))], T=97, train=True),
    "groups2_decode": dict(stages=[((6, 12, 16, 8), dict(groups=2, decode=True))], T=50, train=True),
    "k5_s3_dilated": dict(stages=[((7, 11, 9), dict(kernel=5, stride=3, dilation_growth=2))], T=127, train=True),
    "k5_s3_dilated_decode": dict(stages=[((7, 11, 9), dict(kernel=5, stride=3, dilation_growth=2, decode=True))],
                                 T=50, train=True),
    "k4_s1": dict(stages=[((6, 10, 10, 7), dict(kernel=4, stride=1, skip=True))], T=51, train=True),
    "k3_s1_decode_skip": dict(stages=[((10, 10, 10), dict(kernel=3, stride=1, decode=True, skip=True, batch_norm=True))],
                              T=75, train=True),
    "k3_s1_decode_post_skip": dict(stages=[((8, 8, 8), dict(kernel=3, stride=1, decode=True, skip=True, post_skip=True,
                                                             scale=0.5))], T=60, train=True),
    "encoder_decoder": dict(stages=[((6, 10, 14), dict(kernel=4, stride=2, leakiness=0.)),
                                    ((14, 10, 6), dict(kernel=4, stride=2, leakiness=0., decode=True,
                                                       activation_on_last=False))],
                            T=_valid_length(100, 2, 2), train=True),
}


def case_seed(name: str) -> int:
    return 5150 + sum(map(ord, name))


def randomize_batchnorm(model, gen):
    """tests/helpers.py's recipe: non-trivial BatchNorm affine parameters / running statistics, in module order."""
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5, generator=gen)
                mod.bias.uniform_(-0.3, 0.3, generator=gen)
                mod.running_mean.uniform_(-0.2, 0.2, generator=gen)
                mod.running_var.uniform_(0.5, 1.5, generator=gen)


def build_model(conv_sequence_cls, name: str) -> torch.nn.Sequential:
    """The case's chain of ``conv_sequence_cls`` modules, from its seed (CPU, fp32)."""
    spec = CASES[name]
    torch.manual_seed(case_seed(name))
    model = torch.nn.Sequential(*[conv_sequence_cls(channels, **kwargs) for channels, kwargs in spec["stages"]])
    randomize_batchnorm(model, torch.Generator().manual_seed(case_seed(name) + 1))
    model.train(spec["train"])
    return model


def make_input(name: str) -> torch.Tensor:
    spec = CASES[name]
    gen = torch.Generator().manual_seed(case_seed(name) + 2)
    return torch.randn(B, spec["stages"][0][0][0], spec["T"], generator=gen)


def cotangent(name: str, shape) -> torch.Tensor:
    gen = torch.Generator().manual_seed(case_seed(name) + 3)
    return torch.randn(*shape, generator=gen)


def build() -> dict:
    sys.path.insert(0, str(HERE))
    from _ref_import import load_reference
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    _, common, _ = load_reference()
    out = {"meta": json.dumps(dict(cases=sorted(CASES), B=B, torch=torch.__version__))}
    for name, spec in CASES.items():
        model = build_model(common.ConvSequence, name)
        for k, v in model.state_dict().items():
            out[f"{name}/sd/{k}"] = v.numpy().copy()
        x = make_input(name).requires_grad_(True)
        y = model(x)
        assert y.shape[-1] >= 1
        if name == "encoder_decoder":
            assert y.shape == x.shape, (y.shape, x.shape)
        (y * cotangent(name, y.shape)).sum().backward()
        out[f"{name}/x"] = x.detach().numpy().copy()
        out[f"{name}/y"] = y.detach().numpy().copy()
        out[f"{name}/gx"] = x.grad.numpy().copy()
        for k, p in model.named_parameters():
            out[f"{name}/grad/{k}"] = p.grad.numpy().copy()
        if spec["train"]:
            for k, v in model.named_buffers():
                out[f"{name}/after/{k}"] = v.numpy().copy()
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "strided_conv.npz", **out)
    print(f"strided_conv: {len(out)} arrays -> {dest / 'strided_conv.npz'} "
          f"({(dest / 'strided_conv.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
