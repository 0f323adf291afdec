"""The encode task on the GPU: ``bm_meg_init`` against ``mask * meg`` (every path of the launcher, the three compute
modes, non-finite tails, determinism, guard bands), the reference fixture (tests/golden/encode.npz) through
``Solver(task="encode")``, the window mask of the loss, ``corr_meg`` through the view-resolving ``update_all``, the
untouched decode path and a failed assert in encode mode.  Tolerances are those of tests/test_convrnn_gpu.py and
tests/test_regression_gpu.py for the same quantities."""
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, adam_params_close, rel_l2, running_stat_close, tensor_digest

sys.path.insert(0, str(GOLDEN))
import make_encode_golden as G  # noqa: E402
from make_convrnn_golden import sample_indices, stored  # noqa: E402
from test_convrnn_gpu import LOSS_TOL, MODEL_FWD_TOL, MODEL_GRAD_TOL, MODES, _bias_in_front_of_batchnorm, \
    _compare, _grad_scale  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


@pytest.fixture(scope="module")
def z():
    raw = np.load(GOLDEN / "encode.npz")
    return {k: raw[k] for k in raw.files}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- bm_meg_init ---------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [
    (3, 5, 37, 7),        # T odd: the scalar instantiation
    (2, 4, 64, 16),       # 16-byte vectors, the boundary between two of them
    (2, 4, 64, 13),       # the boundary inside a vector
    (2, 3, 64, 0),        # nothing kept
    (2, 3, 64, 64),       # everything kept
    (2, 3, 64, 99),       # limit past the end: saturates
    (700, 9, 8, 3),       # more rows than the grid has workgroups, two vectors per row, a partly filled chunk
    (64, 64, 520, 52),    # more vectors than one pass of the largest grid takes: the grid-stride loop iterates
    (64, 64, 129, 13),    # the same in the scalar instantiation
]


def _reference(meg, limit):
    """bm/solver.py:289-292."""
    mask = torch.zeros(meg.shape[-1]).to(meg)
    mask[:max(limit, 0)] = 1
    return mask * meg


def _check_meg_init(H, meg, limit, mode):
    x = H.meg_init(meg, limit)
    ref = _reference(meg, limit)
    kept = min(max(limit, 0), meg.shape[-1])
    assert x.shape == meg.shape and x.is_contiguous() and x.data_ptr() != meg.data_ptr()
    assert bool((x == ref).all())                                                  # (-0.0 == +0.0)
    assert torch.equal(x[..., :kept].contiguous().view(torch.int32), meg[..., :kept].contiguous().view(torch.int32))
    assert not bool(x[..., kept:].contiguous().view(torch.int32).any())            # the tail is +0.0, bit for bit
    slot = H._noted(x, "_bm_amax")
    if mode == "f16x2":
        assert slot is not None and slot.shape == (H.AMAX_SHARDS,)
        want = float(meg[..., :kept].abs().max()) if kept else 0.
        assert float(slot.max()) == want
    else:
        assert slot is None
    return x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,T,limit", KERNEL_SHAPES)
def test_meg_init_is_mask_times_meg(H, mode, B, C, T, limit):
    H.set_compute_dtype(mode)
    try:
        scans = H.amax_scans
        meg = torch.randn(B, C, T, generator=_gen(B + C + T + limit)).cuda()
        x = _check_meg_init(H, meg, limit, mode)
        if mode == "f16x2":
            H.amax(x)
            assert H.amax_scans == scans          # the published maximum is found on the tensor: no scan
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("mode", MODES)
def test_meg_init_negative_limit_and_empty_batch(H, mode):
    H.set_compute_dtype(mode)
    try:
        _check_meg_init(H, torch.randn(2, 3, 16, generator=_gen(1)).cuda(), -4, mode)
        x = H.meg_init(torch.empty(0, 3, 16, device="cuda"), 5)
        assert x.shape == (0, 3, 16)
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("limit", [13, 16])
def test_meg_init_at_an_odd_element_offset(H, mode, limit):
    """T % 4 == 0 but the input starts 4 bytes past a 16-byte boundary: the launcher must take the scalar path."""
    H.set_compute_dtype(mode)
    try:
        B, C, T = 2, 4, 64
        buf = torch.randn(B * C * T + 1, generator=_gen(5)).cuda()
        meg = buf[1:].view(B, C, T)
        assert meg.is_contiguous() and meg.data_ptr() % 16 == 4
        _check_meg_init(H, meg, limit, mode)
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("B,C,T,limit", [(3, 5, 37, 7), (2, 4, 64, 13), (2, 4, 64, 16), (700, 9, 8, 3)])
def test_meg_init_drops_a_non_finite_tail(H, B, C, T, limit):
    """inf / NaN at t >= limit (in the vector that holds the boundary too): the output is finite and the published
    maximum is that of the head, exactly."""
    H.set_compute_dtype("f16x2")
    try:
        meg = torch.randn(B, C, T, generator=_gen(B + T)).cuda()
        meg[:, :, limit] = float("nan")
        meg[0, 0, limit + 1] = float("inf")
        meg[-1, -1, T - 1] = float("-inf")
        meg[B // 2, C // 2, limit + 2:] = float("nan")
        x = H.meg_init(meg, limit)
        assert bool(torch.isfinite(x).all())
        assert torch.equal(x[..., :limit], meg[..., :limit]) and not bool(x[..., limit:].any())
        assert float(H._noted(x, "_bm_amax").max()) == float(meg[..., :limit].abs().max())
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def test_meg_init_twice_is_bit_identical(H):
    H.set_compute_dtype("f16x2")
    try:
        meg = torch.randn(700, 9, 8, generator=_gen(3)).cuda()
        a, b = H.meg_init(meg, 3), H.meg_init(meg, 3)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(H._noted(a, "_bm_amax"), H._noted(b, "_bm_amax"))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("B,C,T,limit", [(3, 5, 37, 7), (2, 4, 64, 13), (700, 9, 8, 3)])
def test_meg_init_stays_inside_its_buffers(H, B, C, T, limit):
    """The output, the amax slots and the workspace inside canary-bordered, NaN-poisoned allocations
    (tests/test_guard_bands_gpu.py's arena)."""
    from test_guard_bands_gpu import Arena, _no_nan
    H.set_compute_dtype("f16x2")
    saved = dict(H._stream_workspaces), dict(H._amax_pool)
    H._stream_workspaces.clear()
    H._amax_pool.clear()
    try:
        meg = torch.randn(B, C, T, generator=_gen(T)).cuda()
        arena = Arena()
        with arena.active():
            x = H.meg_init(meg, limit)
            slot = H._noted(x, "_bm_amax")
        arena.check("meg_init")
        _no_nan(x, "meg_init")
        assert bool((x == _reference(meg, limit)).all())
        assert float(slot.max()) == float(meg[..., :limit].abs().max())
    finally:
        H._stream_workspaces.clear()
        H._amax_pool.clear()
        H._stream_workspaces.update(saved[0])
        H._amax_pool.update(saved[1])
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


# ---- the fixture through Solver(task="encode") ---------------------------------------------------------------------------
def _rebuilt(z, name):
    """The case's model and batch from the seed, proven identical to the reference's by the fixture's digests."""
    from brainmagick_amd.models import ConvRNN, SimpleConv
    model = G.build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), name)
    for k, v in model.state_dict().items():
        assert np.array_equal(tensor_digest(v), z[f"{name}/sd/{k}"]), (name, k)
    batch = G.make_batch(name)
    assert np.array_equal(tensor_digest(batch.meg), z[f"{name}/in/meg"])
    assert np.array_equal(tensor_digest(batch.features), z[f"{name}/in/features"])
    assert np.array_equal(batch.features_mask.numpy(), z[f"{name}/mask"])
    assert np.array_equal(batch.subject_index.numpy(), z[f"{name}/subjects"])
    return model, batch


def _encode_solver(name, model, **kw):
    from brainmagick_amd.losses import L1Loss, L2Loss
    from brainmagick_amd.solver import Solver
    spec = G.TRAIN_CASES[name]
    return Solver(model, loss=L1Loss() if spec["loss"] == "l1" else L2Loss(), lr=G.LR, task="encode",
                  meg_init=spec["meg_init"], sample_rate=spec["sample_rate"], offset_meg_ms=spec["offset_meg_ms"],
                  mask_loss=spec["mask_loss"], **kw)


@pytest.mark.parametrize("name", list(G.TRAIN_CASES))
def test_training_case_through_the_encode_solver(H, z, name):
    spec = G.TRAIN_CASES[name]
    model, batch = _rebuilt(z, name)
    solver = _encode_solver(name, model)
    limit = int(z[f"{name}/limit"])
    B, C = spec["B"], spec["inputs"]["meg"]
    T = spec["T"] - int(spec["offset_meg_ms"] / 1000 * spec["sample_rate"])
    seen = []

    def keep(module, args, output):          # (estimate, target, mask) at full length, as train_step hands them over
        args[0].retain_grad()
        seen.append(args)
    solver.loss.register_forward_hook(keep)
    ref_scale = _grad_scale(z, f"{name}/grad/")
    noise_keys = set()
    for step in range(2):
        loss = solver.train_step(batch)
        ref = float(z[f"{name}/losses"][step])
        print(f"{name} step {step}: loss {float(loss):.7f} (reference {ref:.7f})")
        assert abs(float(loss) - ref) <= LOSS_TOL, (step, float(loss), ref)
        if step == 0:
            estimate, target, window = seen[0]
            assert estimate.shape == target.shape == (B, C, T) and window.shape == (B, 1, T)
            assert window.dtype == torch.bool and not bool(window[..., :limit].any())
            _compare(z, f"{name}/y", estimate[..., limit:].contiguous(), MODEL_FWD_TOL, f"{name} estimate")
            # the window selects what the reference's slices select: its count, and no gradient in front of it
            count = int(z[f"{name}/count"])
            assert int(window.sum()) * C == count
            if not spec["mask_loss"]:
                assert count == B * C * (T - limit)
            _, counted = H.regress_loss_fwd(estimate.detach().contiguous(), target, window, spec["loss"])
            assert float(counted) == count
            d_est = estimate.grad
            assert d_est is not None and d_est.shape == estimate.shape
            assert not bool(d_est[..., :limit].contiguous().view(torch.int32).any())
            assert bool(d_est[..., limit:].any())
            for k, p in model.named_parameters():
                if _compare(z, f"{name}/grad/{k}", p.grad, MODEL_GRAD_TOL, f"{name} step-0 grad {k}", ref_scale):
                    noise_keys.add(k)
    solver.check_pending_flags()
    # only gradients that are round-off noise in the reference took the escape: conv biases in front of a BatchNorm
    if spec["model"] == "convrnn":
        assert all(_bias_in_front_of_batchnorm(model, k) for k in noise_keys), noise_keys
    else:
        assert all(k.endswith(".bias") for k in noise_keys), noise_keys
    params = dict(model.named_parameters())
    for k, v in model.state_dict().items():
        if k in noise_keys:
            continue
        if k in params:
            # Adam turns a round-off-noise gradient into a full +-lr update: not reproducible (helpers.is_noise_grad,
            # the rule of tests/test_regression_gpu.py)
            g_ref, _, g_max = stored(z, f"{name}/grad/{k}")
            if (float(g_ref.abs().max()) if g_max is None else g_max) <= 1e-5 * ref_scale:
                continue
        if not v.is_floating_point():
            assert int(v) == int(z[f"{name}/sd1/{k}"]), k
            continue
        ref, norm, _ = stored(z, f"{name}/sd1/{k}")
        got = v.detach().cpu()
        got = got.reshape(ref.shape) if norm is None else got.flatten()[sample_indices(got.numel())]
        if k in params:
            ok, detail = adam_params_close(got, ref, 2, lr=G.LR)
            assert ok, (name, k, detail)
        else:
            assert running_stat_close(got, ref, 2, lr=G.LR), (name, k, rel_l2(got, ref))


def test_encode_eval_step_and_public_process_batch(H, z):
    """``eval_step`` gives the training loss of the untouched model; the public ``_process_batch`` keeps the reference's
    contract: the tensors without their first ``limit`` samples, as views."""
    name = "convrnn_l1_offset_mask"
    spec = G.TRAIN_CASES[name]
    model, batch = _rebuilt(z, name)
    solver = _encode_solver(name, model)
    limit = int(z[f"{name}/limit"])
    loss = solver.eval_step(batch)
    assert abs(float(loss) - float(z[f"{name}/losses"][0])) <= LOSS_TOL          # (no dropout, no BatchNorm)
    with torch.no_grad():
        estimate, output, mask, reject = solver._process_batch(batch)
    T = spec["T"] - 5 - limit
    assert estimate.shape == output.shape == (spec["B"], 20, T) and mask.shape == (spec["B"], 1, T)
    assert estimate._base is not None and output._base is not None
    assert torch.equal(output.cpu(), batch.meg[..., 5:][..., limit:])
    assert torch.equal(mask.cpu(), batch.features_mask[..., :-5][..., limit:])
    _compare(z, f"{name}/y", estimate.contiguous(), MODEL_FWD_TOL, f"{name} public estimate")


def test_decode_process_batch_returns_the_forward_s_own_tensors(H, z):
    """The default task takes today's path: what ``_process_batch`` returns ARE the tensors the model and ``_prepare``
    made (no ``[..., 0:]`` view, which would lose the maxima cached on them)."""
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.models import ConvRNN
    from brainmagick_amd.solver import Solver
    torch.manual_seed(3)
    model = ConvRNN(in_channels={"meg": 20}, out_channels=7, hidden={"meg": 24}, n_subjects=4)
    batch = G.make_batch("convrnn_l1")
    solver = Solver(model, loss=L2Loss(), task="decode")
    assert solver.task == "decode"
    made, outputs = [], []
    inner = solver._forward

    def spy(*a, **k):
        made.append(inner(*a, **k))
        return made[-1]
    solver._forward = spy
    model.register_forward_hook(lambda m, a, out: outputs.append(out))
    with torch.no_grad():
        got = solver._process_batch(batch)
    assert len(made) == 1 and made[0][4] == 0 and len(got) == 4
    assert all(g is m for g, m in zip(got, made[0][:4]))
    assert got[0] is outputs[0] and got[0]._base is outputs[0]._base


def test_a_failed_assert_in_encode_mode_leaves_no_trace(H, z):
    """A non-finite feature value raises at the check point of ``train_step`` and leaves the parameters, the BatchNorm
    buffers and the last good batch as they were."""
    name = "simpleconv_mse"
    model, batch = _rebuilt(z, name)
    solver = _encode_solver(name, model)
    solver.train_step(batch)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert any("running_mean" in k for k in before)
    features = batch.features.clone()
    features[1, 2, 50] = float("nan")
    bad = batch.replace(features=features)
    with pytest.raises(AssertionError, match="non-finite"):
        solver.train_step(bad)
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert solver._last_batch is batch
    loss = solver.train_step(batch)              # and training goes on
    assert bool(torch.isfinite(loss))
    solver.check_pending_flags()


# ---- corr_meg -------------------------------------------------------------------------------------------------------------
def _metric_batches(z):
    d = G.METRICS
    for r in range(d["recordings"]):
        yield r, [G.make_batch(d["case"], 1 + r * d["batches"] + i, d["B"]) for i in range(d["batches"])]


def test_corr_meg_on_the_reference_s_estimates(H, z):
    """bm/play.py:140-154 on what the reference's ``_process_batch`` returned: the operands are the windows
    ``x[..., limit:]`` of full-length tensors (the head of the estimate poisoned with NaN: it is never read), trimmed by
    ``trim_offset``; per-recording results to 1e-10 (fp64), and bit-equal to the same call on contiguous copies."""
    from brainmagick_amd import metrics as M
    name = G.METRICS["case"]
    limit, trim = int(z[f"{name}/limit"]), int(z["metrics/trim_offset"])
    assert trim == M.encode_trim_offset(G.TRAIN_CASES[name]["sample_rate"], G.METRICS["tmin"],
                                        G.TRAIN_CASES[name]["meg_init"])
    results = []
    for r, batches in _metric_batches(z):
        by_view, by_copy = [c() for c in M.encode_metric_constructors()], [c() for c in M.encode_metric_constructors()]
        for i, batch in enumerate(batches):
            assert np.array_equal(tensor_digest(batch.meg), z[f"metrics/in/{r}/{i}/meg"])
            meg = batch.meg.cuda()
            full = torch.full_like(meg, float("nan"))
            full[..., limit:] = torch.from_numpy(z[f"metrics/est/{r}/{i}"]).cuda()
            mask = torch.ones(len(meg), 1, meg.shape[-1], dtype=torch.bool, device="cuda")
            for m in (None, mask):
                views = (full[..., limit:], meg[..., limit:]) + (() if m is None else (m[..., limit:],))
                assert M._common_window(list(views)) is not None
                assert M._common_window([views[0], meg]) is None and M._common_window([full[..., :-1], meg[..., :-1]]) is None
            M.update_all(by_view, full[..., limit:], meg[..., limit:], mask[..., limit:], trim)
            M.update_all(by_copy, full[..., limit:].contiguous(), meg[..., limit:].contiguous(),
                         mask[..., limit:].contiguous(), trim)
        assert torch.equal(by_view[0]._acc, by_copy[0]._acc)
        value = by_view[0].get().cpu()
        want = torch.from_numpy(z[f"metrics/get/{r}/corr_meg"])
        assert value.shape == want.shape and value.dtype == torch.float64
        assert (value - want).abs().max().item() <= 1e-10 * want.abs().max().item()
        results.append(value.float())
    want = float(z["metrics/reduce/corr_meg"])
    assert abs(by_view[0].reduce(results) - want) <= 1e-6 * abs(want)


def test_update_all_copies_any_other_layout_once(H):
    """Windows that differ, or only one windowed operand: the result is that of contiguous copies."""
    from brainmagick_amd import metrics as M
    g = _gen(11)
    a, b = torch.randn(3, 4, 20, generator=g).cuda(), torch.randn(3, 4, 24, generator=g).cuda()
    left, right = a[..., 4:], b[..., 8:]
    assert M._common_window([left, right]) is None
    got, want = M.OnlineCorrelation(slice(None), slice(None)), M.OnlineCorrelation(slice(None), slice(None))
    M.update_all([got], left, right, None, 2)
    M.update_all([want], left.contiguous(), right.contiguous(), None, 2)
    assert torch.equal(got._acc, want._acc)
    got2 = M.OnlineCorrelation(slice(1, 3), slice(1, 3))
    want2 = M.OnlineCorrelation(slice(1, 3), slice(1, 3))
    M.update_all([got2], a[..., 4:], b[..., 8:][..., :16].contiguous(), None, 0)
    M.update_all([want2], a[..., 4:].contiguous(), b[..., 8:][..., :16].contiguous(), None, 0)
    assert torch.equal(got2._acc, want2._acc)


def test_corr_meg_through_the_encode_solver(H, z):
    """``regression_test_metrics`` on ``Solver(task="encode")``: the estimates of the public ``_process_batch`` are the
    reference's (model tolerance), and the metrics are, bit for bit, those of the kernel on contiguous copies of them."""
    from brainmagick_amd import metrics as M
    name = G.METRICS["case"]
    trim = int(z["metrics/trim_offset"])
    model, _ = _rebuilt(z, name)
    solver = _encode_solver(name, model)
    recordings = [batches for _, batches in _metric_batches(z)]
    got = M.regression_test_metrics(solver, recordings, trim, metrics=M.encode_metric_constructors(), reduce=False)
    assert list(got) == ["corr_meg"] and got["corr_meg"].shape == (2,) + z["metrics/get/0/corr_meg"].shape
    for r, batches in enumerate(recordings):
        by_copy = M.encode_metric_constructors()[0]()
        for i, batch in enumerate(batches):
            with torch.no_grad():
                estimate, gt, _, _ = solver._process_batch(batch)
            assert rel_l2(estimate, torch.from_numpy(z[f"metrics/est/{r}/{i}"])) < MODEL_FWD_TOL
            print(f"recording {r} batch {i}: operands read in place: {M._common_window([estimate, gt]) is not None}")
            by_copy.update(estimate.contiguous(), gt.contiguous(), None, trim)
        assert torch.equal(got["corr_meg"][r], by_copy.get().cpu().float())
    reduced = M.regression_test_metrics(solver, recordings, trim, metrics=M.encode_metric_constructors())
    assert reduced["corr_meg"] == pytest.approx(float(got["corr_meg"].mean()), abs=1e-7)
