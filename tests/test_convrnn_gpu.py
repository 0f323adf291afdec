"""ConvRNN on the HIP path: ``functional.LSTMFn`` (csrc/lstm.hip) against ``torch.nn.LSTM`` in fp64 on the CPU, every
case of the reference fixture (tests/golden/convrnn.npz) through ``brainmagick_amd.models.ConvRNN`` in the three
compute modes, the two training cases through the unmodified ``Solver``, dropout, determinism, guard bands, launch
labels and one ConvRNN-sized step.

Tolerances are the project's: tests/test_kernels_gpu.py's for the exact-fp32 MFMA family (5e-6 forward, 2e-5 gradients,
rel-L2 against fp64) at kernel level, tests/test_model_gpu.py's (1e-5 forward, 1e-4 gradients, losses 1e-4) against the
reference fixture, with ``helpers.close``'s single escape for gradients that are round-off noise in the reference."""
import copy
import json
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NOISE, adam_params_close, rel_l2, running_stat_close, tensor_digest

sys.path.insert(0, str(GOLDEN))
import make_convrnn_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 5e-6, 2e-5               # LSTMFn against fp64
MODEL_FWD_TOL, MODEL_GRAD_TOL = 1e-5, 1e-4   # ConvRNN against the reference fixture
LOSS_TOL = 1e-4
MODES = ["f16x2", "f32x3", "f32"]


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)
    hip_ops.set_kernel_timer(None)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- LSTMFn against torch.nn.LSTM in fp64 ------------------------------------------------------------------------------
def _lstm_reference(rnn, x, dy, dh, dc, dtype):
    """(y [B, H * dirs, T], h_n, c_n, grads) of torch's own CPU LSTM in ``dtype`` for the loss <y, dy> + <h_n, dh> +
    <c_n, dc>; grads = [d input] + one per parameter in nn.LSTM's flat order."""
    ref = copy.deepcopy(rnn).to(dtype)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y, (h_n, c_n) = ref(xr.permute(2, 0, 1))
    y = y.permute(1, 2, 0)
    ((y * dy.to(dtype)).sum() + (h_n * dh.to(dtype)).sum() + (c_n * dc.to(dtype)).sum()).backward()
    grads = [xr.grad] + [getattr(ref, n).grad for n in ref._flat_weights_names]
    return y.detach(), h_n.detach(), c_n.detach(), grads


def _run_lstm_case(H, In, Hd, B, T, layers, bidirectional, seed, fwd_tol=FWD_TOL, grad_tol=GRAD_TOL):
    from brainmagick_amd import functional as BF
    torch.manual_seed(seed)
    rnn = torch.nn.LSTM(In, Hd, layers, bidirectional=bidirectional)
    dirs = 2 if bidirectional else 1
    g = _gen(seed + 1)
    x = torch.randn(B, In, T, generator=g)
    dy = torch.randn(B, Hd * dirs, T, generator=g)
    dh = torch.randn(layers * dirs, B, Hd, generator=g)
    dc = torch.randn(layers * dirs, B, Hd, generator=g)
    y64, h64, c64, g64 = _lstm_reference(rnn, x, dy, dh, dc, torch.float64)
    y32, h32, c32, g32 = _lstm_reference(rnn, x, dy, dh, dc, torch.float32)
    params = [getattr(rnn, n).detach().cuda().requires_grad_(True) for n in rnn._flat_weights_names]
    xg = x.detach().cuda().requires_grad_(True)
    y, h_n, c_n = BF.LSTMFn.apply(xg, Hd, layers, bidirectional, 0., False, *params)
    assert y.shape == y64.shape and h_n.shape == h64.shape and c_n.shape == c64.shape
    ((y * dy.cuda()).sum() + (h_n * dh.cuda()).sum() + (c_n * dc.cuda()).sum()).backward()
    torch.cuda.synchronize()
    tag = f"In={In} H={Hd} B={B} T={T} layers={layers} dirs={dirs} [{H.get_compute_dtype()}]"
    failures = []
    for what, got, ref, ref32, tol in [("y", y, y64, y32, fwd_tol), ("h_n", h_n, h64, h32, fwd_tol),
                                       ("c_n", c_n, c64, c32, fwd_tol)] + \
            [(f"grad {n}", t.grad, r, r32, grad_tol)
             for n, t, r, r32 in zip(["<input>"] + list(rnn._flat_weights_names), [xg] + params, g64, g32)]:
        assert got is not None, (tag, what)
        e = rel_l2(got, ref)
        print(f"LSTMFn {tag} {what}: {e:.2e}   (torch fp32 CPU LSTM against fp64: {rel_l2(ref32, ref):.2e})")
        if not e < tol:
            failures.append((what, e))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
@pytest.mark.parametrize("bidirectional", [False, True])
def test_lstm_fn_matches_fp64_off_tile(H, mode, layers, bidirectional):
    """In 37, H 45, B 5, T' 17: nothing is a multiple of a tile, a 32-row block or 4."""
    H.set_compute_dtype(mode)
    try:
        _run_lstm_case(H, 37, 45, 5, 17, layers, bidirectional, seed=100 + 10 * layers + int(bidirectional))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("In,Hd,B,T,layers,bidirectional", [
    (37, 45, 1, 17, 2, True),          # B = 1
    (37, 45, 5, 1, 2, True),           # T' = 1: no recurrent product at all
    (37, 45, 5, 1, 1, False),
    (20, 130, 70, 9, 2, True),         # several tiles in both directions, ragged edges, a partial reduction chunk
    (64, 64, 32, 5, 1, False),         # everything on the tile
])
def test_lstm_fn_matches_fp64_edge_shapes(H, In, Hd, B, T, layers, bidirectional):
    _run_lstm_case(H, In, Hd, B, T, layers, bidirectional, seed=In + Hd + B + T)


def test_lstm_fn_matches_fp64_paper_sized_stack(H):
    """In 576, H 512, B 256, T' 92, 4 layers: the stack of the reference's convrnn configuration."""
    _run_lstm_case(H, 576, 512, 256, 92, 4, False, seed=512)


# ---- the reference fixture through the model -------------------------------------------------------------------------
_fixture_cache = {}


def _fixture():
    if not _fixture_cache:
        z = np.load(GOLDEN / "convrnn.npz")
        _fixture_cache.update({k: z[k] for k in z.files})
    return _fixture_cache


def _rebuilt_model(name):
    """The case's model and inputs from the seed, proven identical to the reference's by the fixture's digests."""
    from brainmagick_amd.models import ConvRNN
    z = _fixture()
    model = G.build_model(ConvRNN, name)
    G.load_stored_tables(model, z, name)
    for k, v in model.state_dict().items():
        assert np.array_equal(tensor_digest(v), z[f"{name}/sd/{k}"]), (name, k)
    inputs = G.make_input(name)
    for k, v in inputs.items():
        assert np.array_equal(tensor_digest(v), z[f"{name}/in/{k}"]), (name, k)
    return model, inputs


class _Batch:
    def __init__(self, subjects):
        self.subject_index = subjects


def _compare(z, key, got, tol, what, ref_scale=None):
    """``got`` against the fixture entry ``key`` (full tensor, or norm + sample): rel-L2 <= tol, with helpers.close's
    escape for gradients that are round-off noise in the reference (``ref_scale`` given).  Returns True when the
    escape was taken."""
    ref, norm, mx = G.stored(z, key)
    got = got.detach().cpu()
    if norm is None:
        got_s, norm, mx = got.reshape(ref.shape), float(ref.double().norm()), float(ref.abs().max()) if ref.numel() else 0.
    else:
        got_s = got.flatten()[G.sample_indices(got.numel())]
    assert got_s.shape == ref.shape, (what, got.shape, ref.shape)
    e = rel_l2(got_s, ref)
    e_norm = abs(float(got.double().norm()) - norm) / norm if norm else float(got.double().norm())
    print(f"{what}: {e:.2e} (norm {e_norm:.2e})")
    if e <= tol and e_norm <= tol:
        return False
    noise = ref_scale is not None and mx <= 10 * NOISE * ref_scale
    assert noise and float((got_s.double() - ref.double()).abs().max()) <= NOISE * ref_scale, (what, e, e_norm)
    return True


def _bias_in_front_of_batchnorm(model, key):
    """True for the biases whose gradient is analytically zero: a conv whose next module is a BatchNorm1d, and in
    Attention the key bias (it adds <q_t, b> to every score of row t, which the softmax over s does not see) and the
    content bias (softmax rows sum to 1, so it reaches fc as a per-channel constant, which the BatchNorm removes)."""
    if not key.endswith(".bias"):
        return False
    path = key.rsplit(".", 1)[0]
    if path.startswith("attentions.") and path.endswith((".fc", ".key", ".content")):
        return True
    *seq_path, idx = path.split(".")
    seq = model.get_submodule(".".join(seq_path))
    if not isinstance(seq, torch.nn.Sequential):
        return False
    nxt = seq[int(idx) + 1] if int(idx) + 1 < len(seq) else None
    return isinstance(nxt, torch.nn.BatchNorm1d)


def _grad_scale(z, prefix):
    norms = []
    for k in z:
        if k.startswith(prefix):
            norms.append(float(z[k]) if k.endswith("@norm") else
                         (float(np.linalg.norm(z[k].astype(np.float64))) if "@" not in k else 0.))
    return max(norms)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(G.CASES))
def test_fixture_through_convrnn(H, name, mode):
    z = _fixture()
    H.set_compute_dtype(mode)
    try:
        model, inputs = _rebuilt_model(name)
        model = model.cuda()
        model.train(G.CASES[name]["train"])
        inputs = {k: v.cuda().requires_grad_(True) for k, v in inputs.items()}
        subjects = torch.from_numpy(z[f"{name}/subjects"]).cuda()
        y = model(dict(inputs), _Batch(subjects))
        assert y.shape == (G.B, G.F_OUT, G.CASES[name]["T"])
        _compare(z, f"{name}/y", y, MODEL_FWD_TOL, f"{name}[{mode}] forward")
        (y * G.cotangent(name, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        ref_scale = max(_grad_scale(z, f"{name}/grad/"), _grad_scale(z, f"{name}/gin/"))
        for k, v in inputs.items():
            _compare(z, f"{name}/gin/{k}", v.grad, MODEL_GRAD_TOL, f"{name}[{mode}] grad <input {k}>")
        escaped = []
        for k, p in model.named_parameters():
            assert p.grad is not None, k
            if _compare(z, f"{name}/grad/{k}", p.grad, MODEL_GRAD_TOL, f"{name}[{mode}] grad {k}", ref_scale):
                escaped.append(k)
        # nothing but the round-off-noise gradients (a conv bias directly in front of a BatchNorm) took the escape
        assert all(_bias_in_front_of_batchnorm(model, k) for k in escaped), escaped
        if G.CASES[name]["train"]:
            for k, v in model.named_buffers():
                v_ref = torch.from_numpy(z[f"{name}/after/{k}"])
                if k.endswith("num_batches_tracked"):
                    assert int(v) == int(v_ref), k
                else:
                    assert running_stat_close(v, v_ref, 1), (name, k, rel_l2(v, v_ref))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


# ---- the two training cases through the unmodified Solver --------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.TRAIN_CASES))
def test_training_case_through_solver(H, name):
    from brainmagick_amd.losses import ClipLoss, L2Loss
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.synthetic import SegmentBatch
    z = _fixture()
    spec = G.TRAIN_CASES[name]
    model, inputs = _rebuilt_model(name)
    features = G.make_features(name)
    assert np.array_equal(tensor_digest(features), z[f"{name}/features"])
    subjects = torch.from_numpy(z[f"{name}/subjects"])
    batch = SegmentBatch(inputs["meg"], features, torch.ones(G.B, 1, spec["T"], dtype=torch.bool), subjects,
                         torch.zeros(G.B, dtype=torch.int64))
    solver = Solver(model, loss=ClipLoss() if spec["loss"] == "clip" else L2Loss(), lr=G.LR)
    ref_scale = _grad_scale(z, f"{name}/grad/")
    noise_keys = set()
    for step in range(2):
        loss = solver.train_step(batch)
        ref = float(z[f"{name}/losses"][step])
        print(f"{name} step {step}: loss {float(loss):.7f} (reference {ref:.7f})")
        assert abs(float(loss) - ref) <= LOSS_TOL, (step, float(loss), ref)
        if step == 0:
            for k, p in model.named_parameters():
                if _compare(z, f"{name}/grad/{k}", p.grad, MODEL_GRAD_TOL, f"{name} step-0 grad {k}", ref_scale):
                    noise_keys.add(k)
    solver.check_pending_flags()
    assert all(_bias_in_front_of_batchnorm(model, k) for k in noise_keys), noise_keys
    # DESIGN §1's rule for parameters after Adam steps: <= 1 % deviating elements, deviation <= 2 * lr * steps
    for k, p in model.named_parameters():
        if k in noise_keys:
            continue
        ref, norm, _ = G.stored(z, f"{name}/sd1/{k}")
        got = p.detach().cpu()
        got = got.reshape(ref.shape) if norm is None else got.flatten()[G.sample_indices(got.numel())]
        ok, detail = adam_params_close(got, ref, 2, lr=G.LR)
        assert ok, (name, k, detail)


# ---- dropout, determinism -----------------------------------------------------------------------------------------------
def _small_model(**kw):
    from brainmagick_amd.models import ConvRNN
    torch.manual_seed(7)
    return ConvRNN(in_channels={"meg": 20}, out_channels=11, hidden={"meg": 24}, n_subjects=4, lstm=3, **kw).cuda()


def _small_batch():
    g = _gen(8)
    return torch.randn(6, 20, 100, generator=g).cuda(), _Batch(torch.randint(0, 4, (6,), generator=g).cuda())


def test_lstm_dropout_acts_in_training_mode_only(H):
    x, batch = _small_batch()
    plain, dropped = _small_model(lstm_dropout=0.), _small_model(lstm_dropout=0.5)
    for (ka, a), (kb, b) in zip(plain.state_dict().items(), dropped.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    plain.eval()
    dropped.eval()
    with torch.no_grad():
        assert torch.equal(plain({"meg": x}, batch), dropped({"meg": x}, batch))
    dropped.train()
    plain.train()
    xg = x.clone().requires_grad_(True)
    y = dropped({"meg": xg}, batch)
    y.square().sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xg.grad).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in dropped.parameters())
    with torch.no_grad():
        assert not torch.equal(y, plain({"meg": x}, batch))


@pytest.mark.parametrize("bidirectional", [False, True])
def test_training_step_is_deterministic(H, bidirectional):
    x, batch = _small_batch()

    def run():
        model = _small_model(bidirectional_lstm=bidirectional, batch_norm=True).train()
        xg = x.clone().requires_grad_(True)
        y = model({"meg": xg}, batch)
        y.square().sum().backward()
        torch.cuda.synchronize()
        return [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in model.parameters()] + \
            [b.clone() for b in model.buffers()]

    first, second = run(), run()
    assert len(first) == len(second)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---- guard bands --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hd,B,T,dirs", [(45, 5, 7, 2), (33, 37, 4, 1), (130, 70, 3, 2), (64, 32, 2, 1), (20, 3, 1, 2)])
def test_step_kernels_stay_inside_their_buffers(H, Hd, B, T, dirs):
    """y, the saved gates and cells, the gate gradients and the carried cell gradient are written inside
    canary-bordered, NaN-poisoned allocations (tests/test_guard_bands_gpu.py's arena), and are right."""
    from test_guard_bands_gpu import Arena, _no_nan
    g = _gen(Hd + B + T + dirs)
    whh = [(torch.randn(4 * Hd, Hd, generator=g) / Hd ** 0.5) for _ in range(dirs)]
    gx = [torch.randn(T, 4 * Hd, B, generator=g) for _ in range(dirs)]
    dy = torch.randn(T, Hd * dirs, B, generator=g)
    dcn = torch.randn(dirs, Hd, B, generator=g)
    whh_g, gx_g = [w.cuda() for w in whh], [t.cuda() for t in gx]
    dy_g, dcn_g = dy.cuda(), dcn.cuda()
    arena = Arena()
    with arena.active():
        y, gates, c = H.lstm_layer_fwd(whh_g, gx_g)
        dc = torch.empty_like(dcn_g)
        dc.copy_(dcn_g)
        dg = H.lstm_layer_bwd(whh_g, dy_g, gates, c, dc)
    what = f"lstm H={Hd} B={B} T={T} dirs={dirs}"
    arena.check(what)
    for t in (y, gates, c, dg, dc):
        _no_nan(t, what)
    # fp64 recurrence written out
    for d in range(dirs):
        w = whh[d].double().requires_grad_(True)
        pre = gx[d].double().requires_grad_(True)
        h = torch.zeros(Hd, B, dtype=torch.float64)
        cc = torch.zeros(Hd, B, dtype=torch.float64)
        hs = [None] * T
        order = range(T - 1, -1, -1) if d else range(T)
        for t in order:
            a = w @ h + pre[t]
            i, f, gg, o = a[:Hd].sigmoid(), a[Hd:2 * Hd].sigmoid(), a[2 * Hd:3 * Hd].tanh(), a[3 * Hd:].sigmoid()
            cc = f * cc + i * gg
            h = o * cc.tanh()
            hs[t] = h
        y64 = torch.stack(hs)
        ((y64 * dy[:, d * Hd:(d + 1) * Hd].double()).sum() + (cc * dcn[d].double()).sum()).backward()
        assert rel_l2(y[:, d * Hd:(d + 1) * Hd], y64) < FWD_TOL, what
        assert rel_l2(c[d, 0 if d else T - 1], cc) < FWD_TOL, what
        assert rel_l2(dg[d], pre.grad) < GRAD_TOL, (what, rel_l2(dg[d], pre.grad))


# ---- launch labels ------------------------------------------------------------------------------------------------------
def _labels(H, fn):
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        H.set_kernel_timer(None)
    return {name for name, *_ in timer.records}


def test_recurrence_runs_in_the_new_kernels_and_nowhere_else(H):
    from brainmagick_amd import synthetic
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    x, batch = _small_batch()
    model = _small_model(bidirectional_lstm=True).train()

    def convrnn_step():
        model({"meg": x.clone().requires_grad_(True)}, batch).square().sum().backward()
    labels = _labels(H, convrnn_step)
    assert {n.split("<")[0] for n in labels if n.startswith("lstm_")} == {"lstm_step_fwd_kernel", "lstm_step_bwd_kernel"}, labels

    sb = synthetic.make_batch(8, 24, 60, 12, 4, seed=3)
    for kw in (dict(), dict(dual_path=1, complex_out=True)):
        torch.manual_seed(0)
        solver = Solver(SimpleConv(in_channels={"meg": 24}, out_channels=12, hidden={"meg": 32}, n_subjects=4,
                                   depth=2, kernel_size=3, merger=False, subject_dim=0, **kw))
        labels = _labels(H, lambda: solver.train_step(sb))
        assert labels and not [n for n in labels if n.startswith("lstm_")], (kw, labels)


# ---- one ConvRNN-sized step ---------------------------------------------------------------------------------------------
def test_convrnn_sized_training_step(H):
    """hidden 512, B 256, T 360, 4 LSTM layers, 273 sensors: one forward + backward completes and is finite."""
    from brainmagick_amd.models import ConvRNN
    torch.manual_seed(1)
    model = ConvRNN(in_channels={"meg": 273}, out_channels=80, hidden={"meg": 512}, n_subjects=30, lstm=4).cuda().train()
    g = _gen(360)
    x = torch.randn(256, 273, 360, generator=g).cuda().requires_grad_(True)
    batch = _Batch(torch.randint(0, 30, (256,), generator=g).cuda())
    y = model({"meg": x}, batch)
    assert y.shape == (256, 80, 360)
    y.square().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
