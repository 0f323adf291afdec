"""Mirror of ``bm/svd.py``: the penalty on the largest singular value of every conv / linear weight
(`optim.svd`, bm/solver.py:379-380), on the HIP low-rank estimate of ``csrc/spectral.hip``.

Differences to the reference:
  * the Gaussian test matrices of all penalised weights are ONE ``torch.randn`` draw per call (the reference draws one per
    weight inside ``torch.svd_lowrank``): the same distribution, another stream;
  * ``test_matrices`` replaces the draw (tests and fixtures pin the result with it), ``generator`` seeds it;
  * ``exact=True`` (a full SVD, "slow but useful at validation") and ``dim > 16`` are not built;
  * at a weight whose basis is rank deficient (a zero or duplicated column or row with ``min(rows, cols) <= 16``, rank
    below 16) the value is the reference's, and the gradient is the finite ``2 sigma_1 u_1 v_1^T`` where the reference's
    QR backward divides by a zero or rounding-noise pivot (its fp32 gradient is off by up to 0.5 in relative norm
    at rank 1 and by 1e9 .. 1e21 at an exactly singular basis);
  * at the all-zero weight value and gradient are exactly 0, where the reference returns 0 and a NaN gradient.
"""
import random
import typing as tp

import torch

# We need a shared RNG to make sure all the distributed workers skip the penalty together (bm/svd.py:12-14).
penalty_rng = random.Random(1234)


def penalized_weights(model: torch.nn.Module, min_size: float = 1.) -> tp.List[tp.Tuple[str, torch.nn.Parameter]]:
    """(module name + ".weight", parameter) of every weight the penalty covers, in the reference's order
    (bm/svd.py:33-39): conv and linear modules of ``model.named_modules()`` whose weight has at least ``min_size`` times
    2**8 elements.  Host only."""
    out = []
    for name, module in model.named_modules():
        if not isinstance(module, (torch.nn.modules.conv._ConvNd, torch.nn.Linear)):
            continue
        p = module.weight
        if p.numel() / 2**8 < min_size:
            continue
        out.append((f"{name}.weight" if name else "weight", p))
    return out


def _estimate_sum(weights: tp.Sequence[torch.Tensor], dim: int, niters: int, generator=None,
                  test_matrices: tp.Optional[tp.Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """Sum of the low-rank estimates of sigma_1 ** 2 of ``w.view(w.shape[0], -1)``, differentiable in the weights."""
    from .functional import SpectralPenaltyFn
    device = weights[0].device
    sizes = [min(w.shape[0], w.numel() // w.shape[0]) for w in weights]
    if test_matrices is None:
        R_all = torch.randn(sum(sizes), dim, device=device, generator=generator)
    else:
        if len(test_matrices) != len(weights):
            raise ValueError(f"svd_penalty: {len(test_matrices)} test matrices for {len(weights)} penalised weights")
        for i, (R, n) in enumerate(zip(test_matrices, sizes)):
            if tuple(R.shape) != (n, dim):
                raise ValueError(f"svd_penalty: test matrix {i} is {tuple(R.shape)}, weight {tuple(weights[i].shape)} "
                                 f"needs {(n, dim)}")
        R_all = torch.cat([R.to(device=device, dtype=torch.float32) for R in test_matrices]).contiguous()
    return SpectralPenaltyFn.apply(R_all, niters, *weights)


def svd_penalty(model: torch.nn.Module, min_size: float = 1., dim: int = 16, niters: int = 2, proba: float = 1,
                exact: bool = False, generator: tp.Optional[torch.Generator] = None,
                test_matrices: tp.Optional[tp.Sequence[torch.Tensor]] = None):
    """Penalty on the largest singular value of every layer (bm/svd.py:17-45).

    - model: model to penalize.
    - min_size: minimum size in kB of a layer to penalize.
    - dim: projection dimension of the low-rank SVD, 1..16.
    - niters: iterations of the algorithm ``torch.svd_lowrank`` uses, 0..8.
    - proba: probability to apply the penalty (drawn from ``penalty_rng``; the result is divided by it).
    - exact: not built.
    - generator: generator of the device for the test matrices.
    - test_matrices: one ``[min(rows, cols), dim]`` tensor per penalised weight, instead of the draw.
    """
    from . import hip_ops as H
    if exact:
        raise NotImplementedError("svd_penalty(exact=True), the full SVD of every weight, is not built: the penalty "
                                  "of the training loop never asks for it")
    H.spectral_check_limits(dim, niters)
    if penalty_rng.random() > proba:
        return 0.
    weights = [p for _, p in penalized_weights(model, min_size)]
    if not weights:
        return 0.
    return _estimate_sum(weights, dim, niters, generator, test_matrices) / proba
