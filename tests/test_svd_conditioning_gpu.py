"""``optim.svd`` on the GPU beyond the fixture's twelve full-rank matrices (inputs and fp64 truths: tests/svd_cases.py, proven
on the CPU by tests/test_svd_penalty_cpu.py):

  A. shapes the fixture has none of -- several chunks in the tall orientation, squares, the production sizes, dim = 1,
     niters = 8, dim < nt < 16 -- against the reference's algorithm in fp64;
  B. rank 1..15 and spectra ``0.3^i`` / ``0.2^i``, where the Gram matrix the kernels factor by Cholesky is singular to
     working precision, against ``sigma_1 ** 2`` and ``2 sigma_1 u v^T``;
  C. exactly singular Gram matrices (a zero or duplicated column, a zero row) and the all-zero weight, same truth;
  D. the C-ABI's row stride (``ld > cols``), which ``hip_ops`` never passes;
  E. guard bands and NaN-poisoned workspaces around the spectral kernels.

Each test prints ``case: value error / tolerance; gradient error / tolerance``."""
import ctypes

import pytest
import torch

import svd_cases as SC
from test_guard_bands_gpu import Arena
from test_svd_penalty_gpu import FACTOR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(w, R, niters):
    """(value, gradient) through the autograd Function, on the CPU."""
    from brainmagick_amd.functional import SpectralPenaltyFn
    w = w.cuda().requires_grad_(True)
    value = SpectralPenaltyFn.apply(R.cuda(), niters, w)
    assert value.shape == () and value.dtype == torch.float32
    grad, = torch.autograd.grad(value, w)
    assert grad.shape == w.shape and grad.is_contiguous()
    return value.detach().cpu(), grad.cpu()


def _nan_weight_gives_nan(w, R, niters):
    from brainmagick_amd.functional import SpectralPenaltyFn
    w = w.clone()
    w.view(-1)[w.numel() // 2 + 1] = float("nan")
    return bool(torch.isnan(SpectralPenaltyFn.apply(R.cuda(), niters, w.cuda())))


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_shapes_against_the_reference_in_fp64(name):
    """The rule of tests/test_svd_penalty_gpu.py: FACTOR x the larger of the case's own and the fixture's median
    fp32-vs-fp64 deviation of the reference; the case's own is capped."""
    w, R, niters = SC.shape_case(name)
    want_v, want_g, dev = SC.shape_truth(name)
    assert dev[1] <= SC.GRAD_DEV_CAP * SC.dev_median()[1], (name, dev)
    value, grad = _run(w, R, niters)
    err_v = abs(float(value) - float(want_v)) / float(want_v)
    err_g = SC.rel(grad, want_g)
    tol_v, tol_g = (FACTOR * max(dev[i], SC.dev_median()[i]) for i in range(2))
    print(f"{name}: value {float(value):.8g} (fp64 {float(want_v):.8g}) error {err_v:.2e} / {tol_v:.2e}; "
          f"gradient error {err_g:.2e} / {tol_g:.2e}")
    assert bool(torch.isfinite(grad).all())
    assert err_v <= tol_v, (name, err_v, tol_v)
    assert err_g <= tol_g, (name, err_g, tol_g)


# ---- B, C ------------------------------------------------------------------------------------------------------------------
def _against_the_analytic_truth(name):
    """FACTOR x the fixture's MEDIAN deviation, for value and gradient: the truth is well conditioned, so the
    well-conditioned tolerance applies.  (The reference's own fp32 error here is printed, not used: it is 1e-3 to
    non-finite in the gradient and would hide anything.)"""
    w, R, niters = SC.ladder_case(name)
    want_v, want_g, ref32 = SC.ladder_truth(name)
    value, grad = _run(w, R, niters)
    err_v = abs(float(value) - float(want_v)) / float(want_v)
    err_g = SC.rel(grad, want_g)
    tol_v, tol_g = (FACTOR * d for d in SC.dev_median())
    print(f"{name}: value {float(value):.8g} (sigma_1^2 {float(want_v):.8g}) error {err_v:.2e} / {tol_v:.2e}; "
          f"gradient error {err_g:.2e} / {tol_g:.2e}; the reference in fp32: value {ref32[0]:.2e}, "
          f"gradient {ref32[1]:.2e}")
    assert bool(torch.isfinite(value)) and bool(torch.isfinite(grad).all()), name
    assert err_v <= tol_v, (name, err_v, tol_v)
    assert err_g <= tol_g, (name, err_g, tol_g)
    return w, R, niters


@pytest.mark.parametrize("name", list(SC.LADDER))
def test_rank_and_conditioning_ladder_against_the_analytic_truth(name):
    _against_the_analytic_truth(name)


@pytest.mark.parametrize("name", list(SC.SINGULAR))
def test_a_singular_gram_matrix_gives_the_exact_sigma_and_its_gradient(name):
    w, R, niters = _against_the_analytic_truth(name)
    assert _nan_weight_gives_nan(w, R, niters), name               # dropping a dead pivot hides no NaN


def test_the_all_zero_weight_gives_zero_and_a_zero_gradient():
    """The reference returns 0 and a NaN gradient (its QR backward divides by R's zero diagonal); here both are 0."""
    w = torch.zeros(SC.ZERO_SHAPE)
    R = SC.draw_R("zero", w)
    value, grad = _run(w, R, SC.NITERS)
    ref_v, ref_g = SC.lowrank_ref(w, R, SC.NITERS)
    print(f"zero_{w.shape[0]}x{w.shape[1]}: value {float(value)!r}, gradient max {float(grad.abs().max())!r}; "
          f"the reference in fp32: value {float(ref_v)!r}, finite gradient: {bool(torch.isfinite(ref_g).all())}")
    assert float(ref_v) == 0.0
    assert float(value) == 0.0 and bool((grad == 0).all())
    assert _nan_weight_gives_nan(w, R, SC.NITERS)


# ---- D ---------------------------------------------------------------------------------------------------------------------
STRIDED = [(45, 69), (150, 70)]
PAD = 5


def _table_with_row_stride(H, plan, bufs):
    """``plan``'s table again, through ``bm_spectral_table_fill`` directly, with every weight read from ``bufs[i]``
    ([rows, cols + PAD]) through the row stride cols + PAD.  The offsets advance as ``SpectralPlan`` advances them."""
    from brainmagick_amd._lib import lib
    L = lib()
    host = torch.zeros(plan.nmat, L.bm_spectral_table_entry_bytes(), dtype=torch.uint8)
    wsf = wsd = r_off = 0
    for i, buf in enumerate(bufs):
        rows, cols = plan.shapes[i]
        assert buf.shape == (rows, cols + PAD) and buf.is_contiguous()
        assert L.bm_spectral_table_fill(ctypes.c_void_p(host[i].data_ptr()), ctypes.c_void_p(buf.data_ptr()), rows, cols,
                                        cols + PAD, plan.dim, r_off, wsf, wsd, plan.grad_offsets[i]) == 0
        r_off += min(rows, cols)
        wsf += L.bm_spectral_ws_floats(rows, cols, plan.niters)
        wsd += L.bm_spectral_ws_doubles(rows, cols, plan.niters)
    assert wsf == plan.ws_floats.numel() and wsd == plan.ws_doubles.numel() and r_off == plan.r_rows
    return host.to(plan.device)


def test_a_row_stride_reads_the_weight_in_place(H):
    """``ld = cols + 5``, the padding floats NaN: values and gradients have the bits of the contiguous copy's, and the
    gradient stays dense (rows x cols, inside its guard bands, every element written)."""
    ws = [SC.gauss(f"strided_{r}x{c}", r, c).cuda() for r, c in STRIDED]
    R = torch.cat([SC.draw_R(f"strided_{r}x{c}", w) for (r, c), w in zip(STRIDED, ws)]).cuda()
    one = torch.ones(1, device="cuda")
    plan = H.SpectralPlan(ws, SC.DIM, SC.NITERS)
    _, want_values = H.spectral_fwd(plan, R)
    want_grads = H.spectral_bwd(plan, one)
    bufs = []
    for w in ws:
        buf = torch.full((w.shape[0], w.shape[1] + PAD), float("nan"), device="cuda")
        buf[:, :w.shape[1]] = w
        bufs.append(buf)
    strided = H.SpectralPlan(ws, SC.DIM, SC.NITERS)             # workspaces of its own
    strided.table = _table_with_row_stride(H, strided, bufs)
    arena = Arena()
    with arena.active():
        _, values = H.spectral_fwd(strided, R)
        grads = H.spectral_bwd(strided, one)
    arena.check("spectral, row stride")
    assert torch.equal(_bits(values), _bits(want_values)) and not bool(torch.isnan(values).any())
    for (r, c), g, want in zip(STRIDED, grads, want_grads):
        assert g.shape == (r, c) and g.is_contiguous()
        assert not bool(torch.isnan(g).any()), (r, c)
        assert torch.equal(_bits(g), _bits(want)), (r, c)
    assert all(bool(torch.isnan(buf[:, -PAD:]).all()) for buf in bufs)


# ---- E ---------------------------------------------------------------------------------------------------------------------
RAGGED = [(150, 70), (70, 150), (65, 65), (12, 300)]


def test_spectral_stores_stay_inside_their_buffers_and_read_nothing_stale(H):
    """Both workspaces, the values and the gradient buffer inside canary-bordered, NaN-poisoned allocations: no store
    leaves them, no NaN comes out ("the workspaces need no initialisation"), and the bits are those of a run in plain
    allocations."""
    ws = [SC.gauss(f"ragged_{r}x{c}", r, c).cuda() for r, c in RAGGED]
    R = torch.cat([SC.draw_R(f"ragged_{r}x{c}", w) for (r, c), w in zip(RAGGED, ws)]).cuda()
    one = torch.ones(1, device="cuda")

    def both():
        H._spectral_plans.clear()                               # fresh weights may reuse the addresses of a cached plan
        plan = H.spectral_plan(ws, SC.DIM, SC.NITERS)
        total, values = H.spectral_fwd(plan, R)
        return plan, total, values, H.spectral_bwd(plan, one)
    _, want_total, want_values, want_grads = both()
    arena = Arena()
    with arena.active():
        plan, total, values, grads = both()
    H._spectral_plans.clear()                                   # nothing keeps the arena's workspaces
    arena.check("spectral, four ragged matrices")
    sizes = sorted(nbytes for _, _, _, nbytes in arena.blocks)
    assert sizes == sorted([4 * plan.ws_floats.numel(), 8 * plan.ws_doubles.numel(), 4 * len(RAGGED), 4,
                            4 * plan.grad_numel]), sizes        # both workspaces are arena allocations
    for t in [total, values] + list(grads):
        assert not bool(torch.isnan(t).any())
    assert torch.equal(_bits(total), _bits(want_total)) and torch.equal(_bits(values), _bits(want_values))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, want_grads))
