"""Strided / transposed ConvSequence layers on the HIP path (csrc/conv_strided.hip): the three kernels against fp64
torch on the CPU, the adjoint identity that ties the two data kernels together, the reference fixture
(tests/golden/strided_conv.npz) through ``ConvSequence``, determinism, guard bands, a ConvRNN-sized encoder ->
decoder, and the proof that the stride-1 odd-kernel path launches nothing of the new family.

Tolerances: tests/test_kernels_gpu.py's for the exact-fp32 MFMA family (5e-6 forward, 2e-5 gradients, rel-L2) at
kernel level, tests/test_model_gpu.py's (1e-5 forward, 1e-4 gradients) against the reference fixture."""
import math
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from helpers import GOLDEN, close, is_noise_grad, rel_l2, running_stat_close

sys.path.insert(0, str(GOLDEN))
import make_strided_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 5e-6, 2e-5            # kernel level, against fp64
MODEL_FWD_TOL, MODEL_GRAD_TOL = 1e-5, 1e-4   # ConvSequence against the reference fixture


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _geometries(s, K):
    """(dil, pad, T) for one (stride, kernel): both dilations, "same-like" padding and none, an odd T and a T whose
    output ends in the middle of a 128-column tile."""
    out = []
    for dil in (1, 2):
        for pad in sorted({K // 2 * dil, 0}):
            for T in (131, 300):
                out.append((dil, pad, T))
    return out


# Cin and M off the 16-channel chunk and the 32-row MFMA block
B_K, CIN_K, M_K = 3, 19, 37


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_strided_conv_kernels_match_fp64(H, s, K):
    """nn.Conv1d with stride: forward (gather form), data gradient (scatter form at the input length) and weight
    gradient against F.conv1d and its autograd in fp64."""
    for dil, pad, T in _geometries(s, K):
        g = _gen(1000 * s + 100 * K + 10 * dil + pad + T)
        x = torch.randn(B_K, CIN_K, T, generator=g)
        w = torch.randn(M_K, CIN_K, K, generator=g) / math.sqrt(CIN_K * K)
        b = torch.randn(M_K, generator=g)
        x64 = x.double().requires_grad_(True)
        w64 = w.double().requires_grad_(True)
        y64 = F.conv1d(x64, w64, b.double(), stride=s, padding=pad, dilation=dil)
        dy = torch.randn(y64.shape, generator=g)
        y64.backward(dy.double())
        Tout = H.conv_out_len(T, K, s, dil, pad, False)
        assert Tout == y64.shape[2]
        xg, wg, bg, dyg = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        tag = f"s={s} K={K} dil={dil} pad={pad} T={T}"
        _, y, _ = H.conv_strided(xg, H.pack_strided_rows_first(wg), M_K, Tout, K, s, dil, pad, False, bias=bg)
        e = rel_l2(y, y64)
        print(f"strided fwd {tag}: {e:.2e}")
        assert e < FWD_TOL, (tag, e)
        _, dx, _ = H.conv_strided(dyg, H.pack_strided_rows_second(wg), CIN_K, T, K, s, dil, pad, True)
        e = rel_l2(dx, x64.grad)
        print(f"strided dgrad {tag}: {e:.2e}")
        assert e < GRAD_TOL, (tag, e)
        dw = H.conv_strided_wgrad(dyg, xg, K, s, dil, pad)
        e = rel_l2(dw, w64.grad)
        print(f"strided wgrad {tag}: {e:.2e}")
        assert e < GRAD_TOL, (tag, e)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_transposed_conv_kernels_match_fp64(H, s, K):
    """nn.ConvTranspose1d: forward (scatter form), data gradient (gather form at the input length) and weight gradient
    (operand roles swapped) against F.conv_transpose1d and its autograd in fp64."""
    for dil, pad, T in _geometries(s, K):
        if (T - 1) * s - 2 * pad + dil * (K - 1) + 1 < 1:
            continue
        g = _gen(2000 * s + 100 * K + 10 * dil + pad + T)
        x = torch.randn(B_K, CIN_K, T, generator=g)
        w = torch.randn(CIN_K, M_K, K, generator=g) / math.sqrt(CIN_K * K)
        b = torch.randn(M_K, generator=g)
        x64 = x.double().requires_grad_(True)
        w64 = w.double().requires_grad_(True)
        y64 = F.conv_transpose1d(x64, w64, b.double(), stride=s, padding=pad, dilation=dil)
        dy = torch.randn(y64.shape, generator=g)
        y64.backward(dy.double())
        Tout = H.conv_out_len(T, K, s, dil, pad, True)
        assert Tout == y64.shape[2]
        xg, wg, bg, dyg = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        tag = f"s={s} K={K} dil={dil} pad={pad} T={T}"
        _, y, _ = H.conv_strided(xg, H.pack_strided_rows_second(wg), M_K, Tout, K, s, dil, pad, True, bias=bg)
        e = rel_l2(y, y64)
        print(f"transposed fwd {tag}: {e:.2e}")
        assert e < FWD_TOL, (tag, e)
        _, dx, _ = H.conv_strided(dyg, H.pack_strided_rows_first(wg), CIN_K, T, K, s, dil, pad, False)
        e = rel_l2(dx, x64.grad)
        print(f"transposed dgrad {tag}: {e:.2e}")
        assert e < GRAD_TOL, (tag, e)
        dw = H.conv_strided_wgrad(xg, dyg, K, s, dil, pad)
        e = rel_l2(dw, w64.grad)
        print(f"transposed wgrad {tag}: {e:.2e}")
        assert e < GRAD_TOL, (tag, e)


def test_epilogue_outputs_and_batchnorm_partials(H):
    """One launch with every epilogue output: the pre-activation, affine + leaky activation, and per-tile partial sums
    whose fold is the per-channel (sum, sum of squares) of the pre-activation -- both forms."""
    g = _gen(77)
    B, Cin, M, T, K, s, dil, pad = 4, 21, 70, 301, 4, 2, 1, 2
    x = torch.randn(B, Cin, T, generator=g)
    b = torch.randn(M, generator=g)
    scale, shift = torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g)
    for transposed in (False, True):
        w = torch.randn((Cin, M, K) if transposed else (M, Cin, K), generator=g) / math.sqrt(Cin * K)
        conv = F.conv_transpose1d if transposed else F.conv1d
        pre64 = conv(x.double(), w.double(), b.double(), stride=s, padding=pad, dilation=dil)
        out64 = F.leaky_relu(pre64 * scale.double()[None, :, None] + shift.double()[None, :, None], 0.1)
        pack = H.pack_strided_rows_second if transposed else H.pack_strided_rows_first
        Tout = H.conv_out_len(T, K, s, dil, pad, transposed)
        pre, out, stats = H.conv_strided(x.cuda(), pack(w.cuda()), M, Tout, K, s, dil, pad, transposed, bias=b.cuda(),
                                         scale=scale.cuda(), shift=shift.cuda(), act=H.ACT_LEAKY, leak=0.1,
                                         want_pre=True, want_stats=True)
        assert rel_l2(pre, pre64) < FWD_TOL and rel_l2(out, out64) < FWD_TOL
        assert stats.shape == (H.lib().bm_conv_strided_stats_tiles(B, Tout, s, int(transposed)), M, 2)
        folded = stats.double().sum(0).cpu()
        assert rel_l2(folded[:, 0], pre64.sum((0, 2))) < 1e-4        # sums cancel: looser than the sums of squares
        assert rel_l2(folded[:, 1], (pre64 ** 2).sum((0, 2))) < FWD_TOL


@pytest.mark.parametrize("s,K,dil,pad", [(2, 4, 1, 2), (3, 5, 2, 4), (4, 3, 1, 0), (1, 4, 1, 2), (2, 1, 1, 0)])
def test_adjoint_identity(H, s, K, dil, pad):
    """<strided(x), y> = <x, transposed(y)> for one weight tensor: the two data kernels are each other's transpose."""
    g = _gen(31 * s + K)
    B, Cin, M, T = 3, 19, 37, 203
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(M, Cin, K, generator=g) / math.sqrt(Cin * K)
    sx64 = F.conv1d(x.double(), w.double(), None, stride=s, padding=pad, dilation=dil)
    # y correlated with strided(x): the inner product is far from zero, so "relative" means something
    y = (torch.randn(sx64.shape, generator=g) + sx64 / sx64.std()).float()
    Tout = sx64.shape[2]
    xg, wg, yg = x.cuda(), w.cuda(), y.cuda()
    _, sx, _ = H.conv_strided(xg, H.pack_strided_rows_first(wg), M, Tout, K, s, dil, pad, False)
    _, ty, _ = H.conv_strided(yg, H.pack_strided_rows_second(wg), Cin, T, K, s, dil, pad, True)
    lhs = float((sx.double().cpu() * y.double()).sum())
    rhs = float((x.double() * ty.double().cpu()).sum())
    print(f"adjoint s={s} K={K}: {lhs!r} vs {rhs!r}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


# ---- the reference fixture through ConvSequence ----------------------------------------------------------------------
def _fixture():
    z = np.load(GOLDEN / "strided_conv.npz")
    return {k: z[k] for k in z.files}


def _bias_in_front_of_batchnorm(model, key):
    """True for `<...>.sequence.<k>.<i>.bias` of a conv whose next module is a BatchNorm1d."""
    if not key.endswith(".bias"):
        return False
    *path, idx, _ = key.split(".")
    seq = model.get_submodule(".".join(path))
    mod = seq[int(idx)]
    nxt = seq[int(idx) + 1] if int(idx) + 1 < len(seq) else None
    return isinstance(mod, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)) and isinstance(nxt, torch.nn.BatchNorm1d)


@pytest.mark.parametrize("mode", ["f16x2", "f32x3", "f32"])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_fixture_through_conv_sequence(H, name, mode):
    from brainmagick_amd.models.common import ConvSequence
    z = _fixture()
    H.set_compute_dtype(mode)
    try:
        model = G.build_model(ConvSequence, name)
        sd0 = {k[len(name) + 4:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(f"{name}/sd/")}
        model.load_state_dict(sd0, strict=True)
        model = model.cuda()
        model.train(G.CASES[name]["train"])
        x = torch.from_numpy(z[f"{name}/x"]).cuda().requires_grad_(True)
        y = model(x)
        y_ref = torch.from_numpy(z[f"{name}/y"])
        assert y.shape == y_ref.shape
        e = rel_l2(y, y_ref)
        print(f"{name}[{mode}] forward: {e:.2e}")
        assert e < MODEL_FWD_TOL, (name, e)
        (y * G.cotangent(name, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        grads_ref = {k[len(name) + 6:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(f"{name}/grad/")}
        grads_ref["<input>"] = torch.from_numpy(z[f"{name}/gx"])
        grads = {k: p.grad for k, p in model.named_parameters()}
        grads["<input>"] = x.grad
        assert set(grads) == set(grads_ref)
        ref_scale = max(float(g.double().norm()) for g in grads_ref.values())
        skipped = []
        for k, g_ref in grads_ref.items():
            assert grads[k] is not None, k
            if is_noise_grad(g_ref, ref_scale):
                skipped.append(k)
                assert close(grads[k], g_ref, MODEL_GRAD_TOL, ref_scale), (name, k)
                continue
            e = rel_l2(grads[k], g_ref)
            print(f"{name}[{mode}] grad {k}: {e:.2e}")
            assert e < MODEL_GRAD_TOL, (name, k, e)
        # nothing but the round-off-noise gradients (the conv bias directly in front of a BatchNorm) was skipped
        assert all(_bias_in_front_of_batchnorm(model, k) for k in skipped), skipped
        if G.CASES[name]["train"]:
            for k, v in model.named_buffers():
                v_ref = torch.from_numpy(z[f"{name}/after/{k}"])
                if k.endswith("num_batches_tracked"):
                    assert int(v) == int(v_ref), k
                else:
                    assert running_stat_close(v, v_ref, 1), (name, k, rel_l2(v, v_ref))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def test_too_short_input_raises_before_any_launch(H):
    """A length torch refuses (a Conv1d input shorter than its dilated kernel: output length < 1) raises the same kind
    of error, with torch's wording, on the host.  ConvSequence's own padding (kernel // 2 * dilation) keeps every
    Conv1d layer clear of that, so the check goes through the autograd function; an even-kernel ConvTranspose1d fed one
    sample would have an EMPTY output ((1 - 1) * 2 - 4 + 3 + 1 = 0), which is refused as well."""
    from brainmagick_amd import functional as BF
    from brainmagick_amd.models.common import ConvSequence
    g = _gen(1)
    w = torch.randn(6, 4, 9, generator=g)
    x = torch.randn(2, 4, 3, generator=g)
    with pytest.raises(RuntimeError, match="Kernel size can't be greater than actual input size"):
        F.conv1d(x, w, None, stride=2)                      # what torch says
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        with pytest.raises(RuntimeError, match="Kernel size can't be greater than actual input size"):
            BF.Conv1dFn.apply(x.cuda(), w.cuda(), None, 1, H.ACT_NONE, 0., False, 2, 0)      # stride 2, padding 0
        torch.manual_seed(0)
        decoder = ConvSequence((4, 6), kernel=4, stride=2, decode=True).cuda()
        with pytest.raises(RuntimeError, match="Output size is too small"):
            decoder(torch.randn(2, 4, 1, generator=g).cuda())
    finally:
        H.set_kernel_timer(None)
    assert not timer.records


def test_training_step_is_deterministic(H):
    """Two runs of a training-mode forward + backward are bit-identical (split-K partials folded in a fixed order)."""
    from brainmagick_amd.models.common import ConvSequence
    g = _gen(5)
    x0 = torch.randn(16, 40, 364, generator=g).cuda()

    def run():
        torch.manual_seed(11)
        enc = ConvSequence((40, 96, 96), kernel=4, stride=2, batch_norm=True).cuda().train()
        dec = ConvSequence((96, 96, 40), kernel=4, stride=2, batch_norm=True, decode=True).cuda().train()
        x = x0.clone().requires_grad_(True)
        y = dec(enc(x))
        (y * y).sum().backward()
        torch.cuda.synchronize()
        out = [y.detach().clone(), x.grad.clone()]
        out += [p.grad.clone() for m in (enc, dec) for p in m.parameters()]
        out += [b.clone() for m in (enc, dec) for b in m.buffers()]
        return out

    first, second = run(), run()
    assert len(first) == len(second)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,Cin,M,T,K,s,dil,pad", [
    (5, 19, 37, 131, 4, 2, 1, 2),          # one partly filled tile, ragged channels
    (3, 48, 150, 777, 4, 2, 1, 2),         # several column tiles (the last holds a few columns), two row tiles
    (2, 33, 70, 300, 5, 3, 2, 4),          # stride 3, dilated
    (2, 20, 40, 257, 3, 4, 1, 0),          # stride 4, no padding
    (2, 150, 70, 300, 4, 2, 1, 2),         # data gradients with more than 64 rows (the tall tile)
])
def test_outputs_stay_inside_their_buffers(H, B, Cin, M, T, K, s, dil, pad):
    """Outputs, BatchNorm partials, gradients and split-K partial tiles are written inside canary-bordered,
    NaN-poisoned allocations, as tests/test_guard_bands_gpu.py does for the wide kernels."""
    from test_guard_bands_gpu import Arena, _no_nan
    g = _gen(B + Cin + M + T)
    x = torch.randn(B, Cin, T, generator=g)
    b = torch.randn(M, generator=g)
    for transposed in (False, True):
        w = torch.randn((Cin, M, K) if transposed else (M, Cin, K), generator=g) / math.sqrt(Cin * K)
        conv = F.conv_transpose1d if transposed else F.conv1d
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y64 = conv(x64, w64, b.double(), stride=s, padding=pad, dilation=dil)
        dy = torch.randn(y64.shape, generator=g)
        y64.backward(dy.double())
        xg, wg, bg, dyg = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        first, second = H.pack_strided_rows_first, H.pack_strided_rows_second
        arena = Arena()
        with arena.active():
            Tout = H.conv_out_len(T, K, s, dil, pad, transposed)
            pre, out, stats = H.conv_strided(xg, (second if transposed else first)(wg), M, Tout, K, s, dil, pad,
                                             transposed, bias=bg, want_pre=True, want_stats=True)
            _, dx, _ = H.conv_strided(dyg, (first if transposed else second)(wg), Cin, T, K, s, dil, pad, not transposed)
            dw = H.conv_strided_wgrad(xg, dyg, K, s, dil, pad, nsplit=3) if transposed else \
                H.conv_strided_wgrad(dyg, xg, K, s, dil, pad, nsplit=3)
        what = f"{'transposed' if transposed else 'strided'} B={B} Cin={Cin} M={M} T={T} K={K} s={s}"
        arena.check(what)
        for t in (pre, out, stats, dx, dw):
            _no_nan(t, what)
        assert rel_l2(pre, y64) < FWD_TOL and rel_l2(out, y64) < FWD_TOL
        assert rel_l2(dx, x64.grad) < GRAD_TOL and rel_l2(dw, w64.grad) < GRAD_TOL


# ---- ConvRNN-sized encoder -> decoder ----------------------------------------------------------------------------------
def _fp64_reference(model, x64):
    """fp64 CPU evaluation of a (BatchNorm-free) ConvSequence chain: its own nn.Conv1d / nn.ConvTranspose1d modules
    applied by torch, the activation markers as F.gelu / F.leaky_relu."""
    from brainmagick_amd.models.common import _Activation
    for seq_module in model:
        assert not seq_module.skip
        for layer in seq_module.sequence:
            for mod in layer:
                if isinstance(mod, _Activation):
                    x64 = F.gelu(x64) if mod.kind == "gelu" else F.leaky_relu(x64, mod.leak)
                else:
                    x64 = mod(x64)
    return x64


def test_convrnn_sized_encoder_and_decoder(H):
    """273 -> 512 -> 512 at kernel 4, stride 2, T = 364, batch 64 (ConvRNN's encoder on the paper's MEG shape) and the
    mirrored ConvTranspose1d decoder: forward and every gradient against fp64 on the CPU at the kernel tolerances.

    The activation is GELU, not the constructor's default LeakyReLU(0) = ReLU: a gradient through a kink cannot be held
    to 2e-5 against ANOTHER precision.  Of the 6e6 pre-activations of a layer, the ~10 that lie within fp32 round-off
    of zero take the other branch in fp64; each flips a whole gradient entry, and k flips out of N cost about
    sqrt(k / N) in rel-L2 -- measured 6.0e-4 on the input gradient with ReLU, while the forward pass of the same run
    was at 8.4e-7.  With a smooth activation the comparison measures the kernels."""
    import copy
    from functools import partial
    from brainmagick_amd.models.common import ConvSequence, _Activation
    torch.manual_seed(2024)
    gelu = partial(_Activation, "gelu")
    model = torch.nn.Sequential(ConvSequence((273, 512, 512), kernel=4, stride=2, activation=gelu),
                                ConvSequence((512, 512, 273), kernel=4, stride=2, decode=True, activation=gelu))
    g = _gen(364)
    x = torch.randn(64, 273, 364, generator=g)
    ref = copy.deepcopy(model).double()
    x64 = x.double().requires_grad_(True)
    y64 = _fp64_reference(ref, x64)
    dy = torch.randn(y64.shape, generator=g)
    y64.backward(dy.double())
    model = model.cuda().train()
    xg = x.cuda().requires_grad_(True)
    y = model(xg)
    assert y.shape == y64.shape
    e = rel_l2(y, y64)
    print(f"ConvRNN-sized forward: {e:.2e}")
    assert e < FWD_TOL, e
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    e = rel_l2(xg.grad, x64.grad)
    print(f"ConvRNN-sized grad <input>: {e:.2e}")
    assert e < GRAD_TOL, e
    ref_grads = dict(ref.named_parameters())
    for k, p in model.named_parameters():
        e = rel_l2(p.grad, ref_grads[k].grad)
        print(f"ConvRNN-sized grad {k}: {e:.2e}")
        assert e < GRAD_TOL, (k, e)


# ---- nothing leaks into the stride-1 odd-kernel path -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "f32x3", "f32"])
def test_same_padding_layers_launch_no_strided_kernel(H, mode):
    """A stride-1 odd-kernel DeepMel step dispatches exactly as before: no KernelTimer label of the new family; the
    same step with the reference's default stride does launch it (the labels are how one tells the families apart)."""
    from brainmagick_amd.models.features import DeepMel
    new_family = ("conv_strided_kernel", "conv_transposed_kernel", "conv_strided_wgrad_kernel")

    def labels(**kw):
        torch.manual_seed(3)
        model = DeepMel(20, 48, 3, 16, batch_norm=True, skip=True, glu=1, glu_context=1, **kw).cuda().train()
        x = torch.randn(4, 20, 150, generator=_gen(9)).cuda().requires_grad_(True)
        timer = H.KernelTimer()
        H.set_kernel_timer(timer)
        try:
            model(x).square().sum().backward()
            torch.cuda.synchronize()
        finally:
            H.set_kernel_timer(None)
        return {name for name, *_ in timer.records}

    H.set_compute_dtype(mode)
    try:
        same = labels(kernel=3, stride=1)
        assert same and not [n for n in same if n.startswith(new_family)], same
        strided = labels(kernel=4, stride=2)
        assert {n.split("<")[0] for n in strided if n.startswith(new_family)} == set(new_family), strided
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
