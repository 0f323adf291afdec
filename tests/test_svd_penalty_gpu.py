"""``optim.svd`` on the GPU: the spectral kernels against the reference's fp64 value and autograd gradient with the
fixture's test matrices (tests/golden/svd_penalty.npz), held to a multiple of the reference's own fp32 distance from
fp64; table indexing, determinism, the compute modes, non-finite weights, the autograd glue; and the penalty through
``Solver(svd=...)`` against two training steps of the live reference."""
import copy
import json
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, adam_params_close, running_stat_close, tensor_digest

sys.path.insert(0, str(GOLDEN))
import make_svd_golden as G  # noqa: E402
import make_lowpass_golden as LPG  # noqa: E402
import make_encode_golden as E  # noqa: E402
from test_convrnn_gpu import LOSS_TOL, MODES  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4          # x max(the case's, the median) fp32-vs-fp64 deviation of the reference: another orthonormalisation
#                     and another summation order than torch's


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


@pytest.fixture(scope="module")
def z():
    raw = np.load(GOLDEN / "svd_penalty.npz")
    return {k: raw[k] for k in raw.files}


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _weight(z, name):
    if f"{name}/w" in z:
        return torch.from_numpy(z[f"{name}/w"]).cuda()
    w = G.make_weight(name)
    assert np.array_equal(tensor_digest(w), z[f"{name}/w_digest"]), name
    return w.cuda()


def _args(key):
    var = G.VARIANTS.get(key, {})
    return var.get("case", key), var.get("niters", 2)


def _one(z, key, gout=None):
    """(value, gradient) of one fixture case through the autograd Function."""
    from brainmagick_amd.functional import SpectralPenaltyFn
    name, niters = _args(key)
    w = _weight(z, name).requires_grad_(True)
    R = torch.from_numpy(z[f"{key}/R"]).cuda()
    value = SpectralPenaltyFn.apply(R, niters, w)
    assert value.shape == () and value.dtype == torch.float32
    grad, = torch.autograd.grad(value, w, grad_outputs=gout)
    assert grad.shape == w.shape and grad.is_contiguous()
    return value.detach(), grad


@pytest.mark.parametrize("key", list(G.CASES) + list(G.VARIANTS))
def test_value_and_gradient_against_the_reference_in_fp64(z, meta, key):
    value, grad = _one(z, key)
    want_v, want_g = float(z[f"{key}/value64"]), torch.from_numpy(z[f"{key}/grad64"]).double()
    err_v = abs(float(value) - want_v) / want_v
    err_g = float((grad.double().cpu() - want_g).norm() / want_g.norm())
    tol_v, tol_g = (FACTOR * max(meta["dev"][key][i], meta["dev_median"][i]) for i in range(2))
    print(f"{key}: value {float(value):.8g} (fp64 {want_v:.8g}) error {err_v:.2e} / {tol_v:.2e}; "
          f"gradient error {err_g:.2e} / {tol_g:.2e}")
    assert bool(torch.isfinite(grad).all())
    assert err_v <= tol_v, (key, err_v, tol_v)
    assert err_g <= tol_g, (key, err_g, tol_g)


def _together(H, z, poison=None):
    """All matrix cases as one plan: (total, values, gradients)."""
    ws = [_weight(z, name) for name in G.CASES]
    if poison is not None:
        ws[poison].view(-1)[7] = float("nan")
    R = torch.cat([torch.from_numpy(z[f"{name}/R"]) for name in G.CASES]).cuda()
    plan = H.spectral_plan(ws, 16, 2)
    total, values = H.spectral_fwd(plan, R)
    grads = H.spectral_bwd(plan, torch.ones(1, device="cuda"))
    torch.cuda.synchronize()
    return total, values, grads


def test_all_matrices_in_one_call_give_the_bits_of_one_at_a_time(H, z):
    total, values, grads = _together(H, z)
    assert len(grads) == len(G.CASES)
    for i, name in enumerate(G.CASES):
        value, grad = _one(z, name)
        assert torch.equal(_bits(values[i]), _bits(value)), name
        assert torch.equal(_bits(grads[i]), _bits(grad)), name
    assert abs(float(total) - float(values.double().sum())) <= 1e-6 * float(total)


def test_two_runs_and_the_three_modes_agree_bit_for_bit(H, z):
    try:
        runs = []
        for mode in MODES + MODES[:1]:
            H.set_compute_dtype(mode)
            runs.append(_together(H, z))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
    for total, values, grads in runs[1:]:
        assert torch.equal(_bits(total), _bits(runs[0][0])) and torch.equal(_bits(values), _bits(runs[0][1]))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, runs[0][2]))


def test_a_nan_weight_gives_a_nan_value_and_leaves_nothing_behind(H, z):
    clean = _together(H, z)
    poison = list(G.CASES).index("conv_45x23x3")
    total, values, grads = _together(H, z, poison=poison)             # returns: every loop is bounded
    assert bool(torch.isnan(total)) and bool(torch.isnan(values[poison]))
    others = [i for i in range(len(G.CASES)) if i != poison]
    assert torch.equal(_bits(values[others]), _bits(clean[1][others]))     # the matrices do not see each other
    again = _together(H, z)                                           # the same workspaces: they hold no state
    assert torch.equal(_bits(again[0]), _bits(clean[0])) and torch.equal(_bits(again[1]), _bits(clean[1]))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[2], clean[2]))


def test_the_incoming_gradient_scales_the_gradients(z):
    from brainmagick_amd.functional import SpectralPenaltyFn
    _, full = _one(z, "conv_45x23x3")
    tenth = torch.tensor(0.1, device="cuda")
    _, scaled = _one(z, "conv_45x23x3", gout=tenth)
    assert torch.equal(_bits(scaled), _bits(full * tenth))
    # several weights, one of them without a gradient; R gets none; a stale workspace is recomputed
    names = ["lin_40x17", "lin_8x64"]
    ws = [_weight(z, n).requires_grad_(n != "lin_8x64") for n in names]
    R = torch.cat([torch.from_numpy(z[f"{n}/R"]) for n in names]).cuda().requires_grad_(True)
    total = SpectralPenaltyFn.apply(R, 2, *ws)
    SpectralPenaltyFn.apply(R.detach(), 2, *[w.detach() * 2 for w in ws])           # other weights, other plan
    SpectralPenaltyFn.apply(R.detach(), 2, *[w.detach() for w in ws])               # the same plan: a later forward
    grads = torch.autograd.grad(total, [R, ws[0]], allow_unused=True)
    assert grads[0] is None
    assert torch.equal(_bits(grads[1]), _bits(_one(z, "lin_40x17")[1]))


# ---- through the Solver ------------------------------------------------------------------------------------------------------
def _rebuilt(z):
    from brainmagick_amd.models import ConvRNN, SimpleConv
    model = LPG.build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), G.TRAIN_CASE)
    for k, v in model.state_dict().items():
        assert np.array_equal(tensor_digest(v), z[f"train/sd/{k}"]), k
    batch = E.make_batch(G.TRAIN_BATCH)
    assert np.array_equal(tensor_digest(batch.meg), z["train/in/meg"])
    assert np.array_equal(tensor_digest(batch.features), z["train/in/features"])
    return model, batch


def _solver(model, **kw):
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    return Solver(model, loss=L2Loss(), lr=E.LR, sample_rate=LPG.base_spec(G.TRAIN_CASE)["sample_rate"], **kw)


def _matrices(z, meta, steps=2):
    n = len(meta["names"]["simpleconv"])
    return [[torch.from_numpy(z[f"train/R/{step}/{i}"]) for i in range(n)] for step in range(steps)]


@pytest.mark.parametrize("mode", MODES)
def test_two_training_steps_against_the_reference(H, z, meta, mode):
    """The fixture's loop (MSE + 0.1 x the reference's svd_penalty, Adam) through ``Solver(svd=0.1)`` with the recorded
    test matrices: the losses within LOSS_TOL and the parameters by ``adam_params_close`` / ``running_stat_close``, the
    rules of the two-step cases of tests/test_lowpass_gpu.py."""
    try:
        H.set_compute_dtype(mode)
        model, batch = _rebuilt(z)
        solver = _solver(model, svd=G.SVD)
        solver.svd_test_matrices = iter(_matrices(z, meta))
        gscale = max(float(np.linalg.norm(z[k])) for k in z if k.startswith("train/grad/"))
        for step in range(2):
            loss = solver.train_step(batch)
            ref = float(z["train/losses"][step])
            print(f"step {step}: loss {float(loss):.7f} (reference {ref:.7f})")
            assert abs(float(loss) - ref) <= LOSS_TOL, (step, float(loss), ref)
        solver.check_pending_flags()
        params = dict(model.named_parameters())
        for k, v in model.state_dict().items():
            ref = torch.from_numpy(z[f"train/sd2/{k}"])
            if not v.is_floating_point():
                assert int(v) == int(ref), k
            elif k in params:
                g_ref = torch.from_numpy(z[f"train/grad/{k}"])
                if float(g_ref.abs().max()) <= 1e-5 * gscale:
                    continue
                ok, detail = adam_params_close(v.cpu(), ref, 2, g_ref=g_ref, gscale=gscale, lr=E.LR)
                assert ok, (k, detail)
            else:
                assert running_stat_close(v.cpu(), ref, 2, lr=E.LR), k
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def test_the_penalty_gradient_adds_to_what_the_conv_kernels_wrote_into_the_bucket(z, meta):
    """p.grad after a step with svd = 0.1 is the svd = 0 gradient plus 0.1 x the penalty's, for weights whose
    gradient the convolution kernels write straight into the optimizer's bucket."""
    from brainmagick_amd.functional import SpectralPenaltyFn
    model, batch = _rebuilt(z)
    plain, pen = _solver(copy.deepcopy(model)), _solver(model, svd=G.SVD)
    names = meta["names"]["simpleconv"]
    mats = _matrices(z, meta, 1)
    ws = [dict(pen.model.named_parameters())[k] for k in names]
    total = SpectralPenaltyFn.apply(torch.cat(mats[0]).cuda(), 2, *ws)
    pgrads = [g.clone() for g in torch.autograd.grad(total, ws)]
    pen.svd_test_matrices = iter(mats)
    l0, l1 = plain.train_step(batch), pen.train_step(batch)
    assert abs(float(l1) - float(l0) - G.SVD * float(total)) <= 1e-6 * abs(float(l1))
    direct = 0
    for k, pg in zip(names, pgrads):
        a, b = dict(plain.model.named_parameters())[k], dict(pen.model.named_parameters())[k]
        assert b.grad.data_ptr() == getattr(b, "_bm_grad_dst")[0].data_ptr()          # the bucket view
        direct += int(getattr(b, "_bm_grad_dst")[1][0])
        want = a.grad.double() + G.SVD * pg.double()
        err = float((b.grad.double() - want).abs().max())
        assert err <= 2.0 ** -22 * float(want.abs().max()), (k, err)
        assert float((b.grad - a.grad).abs().max()) > 0, k                               # the sum is not vacuous
    assert direct > 0          # some of these gradients were written into the bucket by the kernels themselves


def test_svd_zero_is_the_path_of_a_solver_without_the_keyword(z, monkeypatch):
    from brainmagick_amd import svd
    model, batch = _rebuilt(z)
    plain, zero = _solver(copy.deepcopy(model)), _solver(model, svd=0.)

    def refuse(*a, **k):
        raise AssertionError("svd_penalty was called with svd = 0")
    monkeypatch.setattr(svd, "svd_penalty", refuse)
    state = svd.penalty_rng.getstate()
    for _ in range(2):
        a, b = plain.train_step(batch), zero.train_step(batch)
        assert torch.equal(_bits(a), _bits(b))
    for (k, v), w in zip(plain.model.state_dict().items(), zero.model.state_dict().values()):
        assert torch.equal(v, w), k
    assert svd.penalty_rng.getstate() == state


def test_a_failed_assert_draws_nothing_and_launches_nothing(z, monkeypatch):
    from brainmagick_amd import svd
    model, batch = _rebuilt(z)
    solver = _solver(model, svd=G.SVD)
    solver.train_step(batch)                    # draws its test matrices from the device generator
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gen, rng = torch.cuda.get_rng_state(), svd.penalty_rng.getstate()
    calls = []
    inner = svd.svd_penalty
    monkeypatch.setattr(svd, "svd_penalty", lambda *a, **k: calls.append(1) or inner(*a, **k))
    meg = batch.meg.clone()
    meg[1, 2, 50] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        solver.train_step(batch.replace(meg=meg))
    torch.cuda.synchronize()
    assert not calls and torch.equal(torch.cuda.get_rng_state(), gen) and svd.penalty_rng.getstate() == rng
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    loss = solver.train_step(batch)             # and training goes on
    assert calls == [1] and bool(torch.isfinite(loss)) and not torch.equal(torch.cuda.get_rng_state(), gen)
    solver.check_pending_flags()
