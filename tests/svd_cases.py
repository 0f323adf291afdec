"""Inputs and fp64 truths of ``optim.svd`` beyond the fixture's twelve matrices, shared by tests/test_svd_penalty_cpu.py
(which proves them on the CPU) and tests/test_svd_conditioning_gpu.py (which holds the kernels to them).

Every weight and test matrix comes from a seeded ``torch.Generator``; every expectation is computed live in fp64.

``lowrank_ref`` restates ``torch.svd_lowrank``'s algorithm (torch/_lowrank.py) with the test matrix given -- Householder
QR, autograd through it.  ``analytic`` is ``sigma_1 ** 2`` and ``2 sigma_1 u_1 v_1^T`` from a full fp64 SVD: the
estimate never exceeds ``sigma_1 ** 2`` and equals it whenever range(Q) holds ``u_1``, so at an exactly low-rank or a
strongly gapped matrix it is the estimate's value AND gradient (a maximum over the subspace that is attained has the
gradient of the attained maximum) -- a truth that does not pass through a badly conditioned QR, whose backward divides by
the pivots of R.
"""
import functools
import json
import math
from pathlib import Path

import numpy as np
import torch

FIXTURE = Path(__file__).resolve().parent / "golden" / "svd_penalty.npz"

DIM, NITERS = 16, 2
GRAD_DEV_CAP = 10       # x the fixture's median gradient deviation: the most a case's own fp32 reference may be off


def _seed(name: str) -> int:
    return 9100 + sum(map(ord, name))


def gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(_seed(name))


def lowrank_ref(A: torch.Tensor, R: torch.Tensor, niters: int, want_grad: bool = True):
    """(value, d value / d A or None) of ``torch.svd_lowrank(A, R.shape[1], niters)[1][0] ** 2`` with R for its draw,
    in A's dtype."""
    A = A.detach().clone().requires_grad_(want_grad)
    M = A.t() if A.shape[0] < A.shape[1] else A
    R = R.to(A.dtype)
    with torch.set_grad_enabled(want_grad):
        Q = torch.linalg.qr(M @ R).Q
        for _ in range(niters):
            Q = torch.linalg.qr(M.t() @ Q).Q
            Q = torch.linalg.qr(M @ Q).Q
        value = torch.linalg.svdvals(Q.t() @ M)[0] ** 2
    grad = torch.autograd.grad(value, A)[0] if want_grad else None
    return value.detach(), grad


def analytic(A: torch.Tensor):
    """(sigma_1 ** 2, 2 sigma_1 u_1 v_1^T) of the matrix as stored, in fp64."""
    u, s, vh = torch.linalg.svd(A.double(), full_matrices=False)
    return s[0] ** 2, 2 * s[0] * torch.outer(u[:, 0], vh[0])


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def gauss(name: str, rows: int, cols: int) -> torch.Tensor:
    return torch.randn(rows, cols, generator=gen(name)) / math.sqrt(cols)


def spectrum(name: str, rows: int, cols: int, base: float) -> torch.Tensor:
    """``U diag(base ** i) V^T`` as tests/golden/make_svd_golden.py's spectrum cases build it, either orientation."""
    g, n = gen(name), min(rows, cols)
    u = torch.linalg.qr(torch.randn(rows, n, generator=g, dtype=torch.float64))[0]
    v = torch.linalg.qr(torch.randn(cols, n, generator=g, dtype=torch.float64))[0]
    s = base ** torch.arange(n, dtype=torch.float64)
    return ((u * s) @ v.t()).to(torch.float32)


def low_rank(name: str, rows: int, cols: int, rank: int) -> torch.Tensor:
    g = gen(name)
    return torch.randn(rows, rank, generator=g) @ torch.randn(rank, cols, generator=g) / 6


def draw_R(name: str, weight: torch.Tensor, dim: int = DIM) -> torch.Tensor:
    return torch.randn(min(weight.shape), dim, generator=gen(name + "/R"))


# A. shapes, against lowrank_ref in fp64:  name -> (weight builder, dim, niters)
SHAPES = {
    "gauss_150x70": (lambda n: gauss(n, 150, 70), DIM, NITERS),        # tall, 3 slabs, 2 chunks, all ragged
    "gauss_70x150": (lambda n: gauss(n, 70, 150), DIM, NITERS),        # wide
    "gauss_65x65": (lambda n: gauss(n, 65, 65), DIM, NITERS),          # square, one row past a slab
    "gauss_128x128": (lambda n: gauss(n, 128, 128), DIM, NITERS),      # square, whole slabs
    "gauss_640x320": (lambda n: gauss(n, 640, 320), DIM, NITERS),      # the head's 1x1
    "gauss_320x960": (lambda n: gauss(n, 320, 960), DIM, NITERS),      # a 3-tap conv
    "gauss_640x960": (lambda n: gauss(n, 640, 960), DIM, NITERS),      # a GLU conv
    "spectrum0.5_96x40/dim1": (lambda n: spectrum(n, 96, 40, 0.5), 1, NITERS),
    "spectrum_0.9/niters8": (None, DIM, 8),                            # the fixture's stored weight, a fresh R
    "gauss_12x300/dim8": (lambda n: gauss(n, 12, 300), 8, NITERS),     # nt < 16, q = dim
}

# B. rank and conditioning ladder, against `analytic`:  name -> weight builder (dim 16, niters 2)
LADDER = {}
for _rows, _cols in ((96, 40), (40, 200)):
    for _rank in (1, 3, 8, 15):
        LADDER[f"rank{_rank}_{_rows}x{_cols}"] = (lambda n, r=_rows, c=_cols, k=_rank: low_rank(n, r, c, k))
for _rows, _cols in ((160, 96), (96, 160)):
    for _base in (0.3, 0.2):
        LADDER[f"spectrum{_base}_{_rows}x{_cols}"] = (lambda n, r=_rows, c=_cols, b=_base: spectrum(n, r, c, b))


def _zero_col(name, rows, cols, col):
    w = gauss(name, rows, cols)
    w[:, col] = 0
    return w


def _zero_row(name, rows, cols, row):
    w = gauss(name, rows, cols)
    w[row] = 0
    return w


def _dup_col(name, rows, cols, dst, src):
    w = gauss(name, rows, cols)
    w[:, dst] = w[:, src]
    return w


# C. structurally singular Gram matrices, against `analytic`:  min(rows, cols) <= 16, so range(Q) is the whole row space
SINGULAR = {
    "64x16_zero_col9": lambda n: _zero_col(n, 64, 16, 9),
    "16x64_zero_row3": lambda n: _zero_row(n, 16, 64, 3),
    "70x12_zero_col0": lambda n: _zero_col(n, 70, 12, 0),
    "64x16_col9_is_col2": lambda n: _dup_col(n, 64, 16, 9, 2),
}
ZERO_SHAPE = (64, 48)


@functools.lru_cache(maxsize=None)
def fixture():
    raw = np.load(FIXTURE)
    return {k: raw[k] for k in raw.files}


def dev_median():
    """[value, gradient]: the medians of the reference's own fp32-vs-fp64 deviation over the fixture's cases."""
    return json.loads(str(fixture()["meta"]))["dev_median"]


def shape_case(name: str):
    """(weight, R, niters) of a case of ``SHAPES``."""
    build, dim, niters = SHAPES[name]
    w = torch.from_numpy(fixture()["spectrum_0.9/w"]).clone() if build is None else build(name)
    return w, draw_R(name, w, dim), niters


def ladder_case(name: str):
    """(weight, R, niters) of a case of ``LADDER`` or ``SINGULAR``."""
    w = (LADDER.get(name) or SINGULAR[name])(name)
    return w, draw_R(name, w), NITERS


@functools.lru_cache(maxsize=None)
def shape_truth(name: str):
    """(value64, grad64, [value, gradient] fp32-vs-fp64 deviation of ``lowrank_ref``) of a case of ``SHAPES``; computed
    once, never written to."""
    w, R, niters = shape_case(name)
    v64, g64 = lowrank_ref(w.double(), R, niters)
    v32, g32 = lowrank_ref(w, R, niters)
    return v64, g64, [abs(float(v32) - float(v64)) / float(v64), rel(g32, g64)]


@functools.lru_cache(maxsize=None)
def ladder_truth(name: str):
    """(sigma_1 ** 2, 2 sigma_1 u v^T, the reference's own fp32 [value, gradient] error against them) of a case of
    ``LADDER`` or ``SINGULAR``."""
    w, R, niters = ladder_case(name)
    value, grad = analytic(w)
    v32, g32 = lowrank_ref(w, R, niters)
    return value, grad, [abs(float(v32) - float(value)) / float(value), rel(g32, grad)]
