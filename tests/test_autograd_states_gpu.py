"""The autograd glue (brainmagick_amd/functional.py) in the states a training step never makes: every Function against
fp64 torch autograd on the CPU with subsets of its inputs requiring grad, non-contiguous operands and incoming
gradients, operands and gradients 4, 8 and 12 bytes off their 16-byte alignment, a graph that is used twice, outputs
consumed one at a time, and no tape at all.

Reference: the same operation restated with torch ops in float64 (F.conv1d / F.conv_transpose1d / F.batch_norm / F.gelu
/ F.glu / nn.LSTM / einsum, oracle.bm_oracle for the merger, the composed front end and ClipLoss, the fp64 forms of
tests/test_regression_gpu.py and tests/test_feature_decoding_gpu.py for the two losses), differentiated by torch.

Tolerances are the project's kernel-level ones (tests/test_kernels_gpu.py, tests/test_guard_bands_gpu.py): forward
rel-L2 <= 5e-6, gradients rel-L2 <= 2e-5 (through helpers.close: a gradient that is analytically zero -- the conv bias in
front of a training-mode BatchNorm -- is round-off noise in the reference too); the two regression-type losses 1e-6 on
the loss / terms and 1e-5 on the gradients, as in their own files.

Shapes.  Narrow: B = 5, 20 -> 24 channels, T = 48 (k in {1, 3}) and T = 49 (the dword paths): the narrow kernels in every
compute mode, so this class also runs in "f32" and "f32x3".  Wide: Cin = M = 256, B = 8, T = 192 (helpers.WIDE_DIMS) and
T = 132 (T % 4 == 0, T % 32 != 0: the FL / RS weight-gradient variants).  The issue's first proposal, B = 3 with T = 132,
is refused by bm_gemm_nt_h2_covers: B * ceil(T / 32) = 15 reduction chunks are fewer than the 32 the wide tiles want;
every wide case asserts from the launch labels that conv_nn_h2w / gemm_nt_h2w really ran."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import close, rel_l2, shifted
from oracle import bm_oracle as O
import test_feature_decoding_gpu as TFD

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 5e-6, 2e-5               # tests/test_kernels_gpu.py
LOSS_TOL_REL, LOSS_GRAD_TOL = 1e-6, 1e-5     # tests/test_regression_gpu.py, tests/test_feature_decoding_gpu.py
MODES = ["f16x2", "f32", "f32x3"]
GELU = 1                                     # hip_ops.ACT_GELU
B, C, M, T = 5, 20, 24, 48


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


@pytest.fixture
def mode(request, H):
    H.set_compute_dtype(request.param)
    yield request.param
    H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _BF():
    from brainmagick_amd import functional
    return functional


# ---- cases ------------------------------------------------------------------------------------------------------------
class Case:
    """``inputs``: name -> fp32 CPU tensor, the differentiable inputs in the Function's order.  ``hip(t)`` /
    ``ref(t)``: the differentiable outputs (a tuple) from a dict of GPU fp32 / CPU fp64 tensors.  ``cost``: name ->
    (conv launches, weight-gradient launches) that the backward pass saves when that input needs no gradient.
    ``loss``: the outputs are losses held to 1e-6 / 1e-5 instead of 5e-6 / 2e-5; ``l1``: the sign of e - o is not
    defined where e ~ o (tests/test_regression_gpu.py)."""

    def __init__(self, name, inputs, hip, ref, cost, loss=False, extra_subsets=()):
        self.name, self.inputs, self.hip, self.ref, self.cost = name, inputs, hip, ref, cost
        self.loss, self.extra_subsets = loss, tuple(extra_subsets)
        self._ref = None
        self._full_counts = {}

    def subsets(self):
        names = list(self.inputs)
        if len(names) <= 3:
            return [c for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]
        out = [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names] + [tuple(names)]
        return out + [s for s in self.extra_subsets if s not in out]

    def reference(self):
        """(outputs, incoming gradients, gradient per input) in fp64, computed once and never written again."""
        if self._ref is None:
            t = {k: v.double().requires_grad_(True) for k, v in self.inputs.items()}
            outs = self.ref(t)
            g = _gen(len(self.name) + 77)
            dys = [torch.randn(o.shape, generator=g) if o.dim() else torch.tensor(1.7) for o in outs]
            grads = torch.autograd.grad(outs, list(t.values()), [d.double() for d in dys])
            self._ref = ([o.detach() for o in outs], dys, dict(zip(t, grads)))
        return self._ref


def _conv_ref(t, KS, dil, act, kind, stride=1, pad=0):
    if kind == "thead":
        y = F.conv_transpose1d(t["x"], t["w"], t.get("b"))
    elif kind == "strided":
        y = F.conv1d(t["x"], t["w"], t.get("b"), stride=stride, padding=pad, dilation=dil)
    else:
        y = F.conv1d(t["x"], t["w"], t.get("b"), padding=dil * (KS // 2), dilation=dil)
    return F.gelu(y) if act else y


def conv1d_case(kind, act, Cin=C, Mo=M, Bn=B, Tn=None, KS=3, dil=1, seed=0):
    g = _gen(1000 + seed + 7 * act + len(kind))
    stride, pad = (2, 1) if kind == "strided" else (1, None)
    if kind in ("k1", "thead"):
        KS = 1
    Tn = Tn or (T + 1 if kind == "same" else T)
    wshape = (Cin, Mo, 1) if kind == "thead" else (Mo, Cin, KS)
    inputs = dict(x=torch.randn(Bn, Cin, Tn, generator=g), w=torch.randn(wshape, generator=g) / math.sqrt(Cin * KS),
                  b=torch.randn(Mo, generator=g))

    def hip(t):
        return (_BF().Conv1dFn.apply(t["x"], t["w"], t["b"], dil, GELU if act else 0, 0., kind == "thead", stride, pad),)
    return Case(f"conv1d-{kind}-{'gelu' if act else 'none'}-{Cin}x{Mo}x{Tn}", inputs, hip,
                lambda t: (_conv_ref(t, KS, dil, act, kind, stride, pad or 0),), dict(x=(1, 0), w=(0, 1), b=(0, 0)))


def convbn_case(training, residual, Cin=None, Mo=M, Bn=B, Tn=None, seed=0):
    Cin = Cin or (Mo if residual else C)
    Tn = Tn or (T + 1 if training else T)
    g = _gen(2000 + seed + 2 * training + residual)
    KS, dil, eps, momentum = 3, 2, 1e-5, 0.1
    inputs = dict(x=torch.randn(Bn, Cin, Tn, generator=g), w=torch.randn(Mo, Cin, KS, generator=g) / math.sqrt(Cin * KS),
                  b=torch.randn(Mo, generator=g), gamma=torch.rand(Mo, generator=g) + 0.5,
                  beta=torch.randn(Mo, generator=g) * 0.3)
    rm, rv = torch.randn(Mo, generator=g) * 0.2, torch.rand(Mo, generator=g) + 0.5

    def hip(t):
        return (_BF().ConvBNActFn.apply(t["x"], t["w"], t["b"], t["gamma"], t["beta"], rm.cuda(), rv.cuda(),
                                        torch.zeros((), dtype=torch.int64, device="cuda"), training, dil, GELU, 0.,
                                        residual, momentum, eps),)

    def ref(t):
        y = F.conv1d(t["x"], t["w"], t["b"], padding=dil, dilation=dil)
        y = F.gelu(F.batch_norm(y, rm.double(), rv.double(), t["gamma"], t["beta"], training, momentum, eps))
        return (y + t["x"] if residual else y,)
    return Case(f"convbn-{'train' if training else 'eval'}-{'res' if residual else 'nores'}-{Cin}x{Mo}x{Tn}", inputs,
                hip, ref, dict(x=(1, 0), w=(0, 1), b=(0, 0), gamma=(0, 0), beta=(0, 0)),
                extra_subsets=[("w", "b"), ("gamma", "beta")])


def glu_case(Cin=M, Bn=B, Tn=T + 1, seed=0):
    g = _gen(3000 + seed)
    inputs = dict(x=torch.randn(Bn, Cin, Tn, generator=g), w=torch.randn(2 * Cin, Cin, 3, generator=g) / math.sqrt(3 * Cin),
                  b=torch.randn(2 * Cin, generator=g))
    return Case(f"glu-{Cin}x{Tn}", inputs, lambda t: (_BF().GLUConvFn.apply(t["x"], t["w"], t["b"]),),
                lambda t: (F.glu(F.conv1d(t["x"], t["w"], t["b"], padding=1), dim=1),), dict(x=(1, 0), w=(0, 1), b=(0, 0)))


def subject_case():
    g = _gen(4000)
    S = 3
    subj = torch.randint(0, S, (B,), generator=g)
    inputs = dict(x=torch.randn(B, C, T, generator=g), w=torch.randn(S, C, M, generator=g) / math.sqrt(C))
    return Case("subject-layers", inputs, lambda t: (_BF().SubjectLayersFn.apply(t["x"], t["w"], subj.cuda()),),
                lambda t: (torch.einsum("bct,bcd->bdt", t["x"], t["w"][subj]),), dict(x=(1, 0), w=(0, 1)))


def _layouts(g, U=2, Dp=32):
    pos = torch.rand(U, C, 2, generator=g)
    layout = torch.randint(0, U, (B,), generator=g)
    layout[:U] = torch.arange(U)
    return pos, layout, torch.tensor([0.4, 0.5]), 0.2


def merger_case():
    g = _gen(5000)
    O_, Dp = 16, 32
    pos, layout, ban, radius = _layouts(g)
    inputs = dict(meg=torch.randn(B, C, T, generator=g), heads=torch.randn(O_, Dp, generator=g) / math.sqrt(Dp))

    def hip(t):
        return (_BF().ChannelMergerFn.apply(t["meg"], t["heads"], pos.cuda(), layout.cuda(), ban.cuda(), radius),)
    return Case("merger", inputs, hip,
                lambda t: (O.channel_merger(t["meg"], t["heads"], pos.double()[layout], True, radius, ban.double()),),
                dict(meg=(1, 0), heads=(1, 1)))


def frontend_case():
    g = _gen(6000)
    O_, Dp, L, S, D = 16, 32, 16, 3, M
    pos, layout, ban, radius = _layouts(g)
    subj = torch.randint(0, S, (B,), generator=g)
    inputs = dict(meg=torch.randn(B, C, T, generator=g), heads=torch.randn(O_, Dp, generator=g) / math.sqrt(Dp),
                  w1=torch.randn(L, O_, 1, generator=g) / math.sqrt(O_), b1=torch.randn(L, generator=g),
                  ws=torch.randn(S, L, D, generator=g) / math.sqrt(L))

    def hip(t):
        return (_BF().FusedFrontEndFn.apply(t["meg"], t["heads"], t["w1"], t["b1"], t["ws"], pos.cuda(), layout.cuda(),
                                            subj.cuda(), ban.cuda(), radius),)

    def ref(t):
        y = O.channel_merger(t["meg"], t["heads"], pos.double()[layout], True, radius, ban.double())
        return (O.subject_layers(F.conv1d(y, t["w1"], t["b1"]), t["ws"], subj),)
    return Case("front-end", inputs, hip, ref, dict(meg=(1, 0), heads=(2, 0), w1=(0, 1), b1=(0, 0), ws=(0, 1)))


def clip_case(symmetric):
    g = _gen(7000 + symmetric)
    Bc, Fd = 7, 24
    inputs = dict(est=torch.randn(B, Fd, T, generator=g), cand=torch.randn(Bc, Fd, T, generator=g))

    def hip(t):
        return (_BF().ClipLossFn.apply(t["est"], t["cand"], 0, None, symmetric)[0],)
    fn = O.clip_loss_symmetric if symmetric else O.clip_loss
    return Case(f"clip-{'symmetric' if symmetric else 'rows'}", inputs, hip, lambda t: (fn(t["est"], t["cand"]),),
                dict(est=(1, 0), cand=(1, 0)))


def regression_case(kind):
    g = _gen(8000 + len(kind))
    Fd = 7
    inputs = dict(est=torch.randn(B, Fd, T + 1, generator=g), out=torch.randn(B, Fd, T + 1, generator=g))
    mask = torch.rand(B, 1, T + 1, generator=g) > 0.3

    def ref(t):
        sel = mask.expand_as(t["est"])
        return ((torch.nn.L1Loss() if kind == "l1" else torch.nn.MSELoss())(t["est"][sel], t["out"][sel]),)
    case = Case(f"regression-{kind}", inputs,
                lambda t: (_BF().MaskedRegressionFn.apply(t["est"], t["out"], mask.cuda(), kind)[0],), ref,
                dict(est=(0, 0), out=(0, 0)), loss=True)
    case.l1 = kind == "l1"
    return case


def feature_decoding_case():
    builder, est, out, mask, weights = TFD._random_case([("emb", 3, None), ("ph", 1, 11), ("aux", 2, None)], B, T + 1, 0,
                                                        True, True, seed=9000)
    mod = []

    def hip(t):
        if not mod:
            from brainmagick_amd.losses import FeatureDecodingLoss
            mod.append(FeatureDecodingLoss(builder, TFD.Weights(weights)))
        return (mod[0](t["est"], out.cuda(), mask.cuda()),)

    def ref(t):
        e, o, sel = t["est"], out.double(), mask
        terms = []
        for f in builder.values():
            fe, fo = e[:, builder.get_slice(f.name, model_output=True)], o[:, builder.get_slice(f.name)]
            if f.categorical:
                terms.append(F.cross_entropy(fe.transpose(1, 2)[sel[:, 0]], fo[:, 0][sel[:, 0]].long(),
                                             weights[f.name].double()))
            else:
                m = sel.expand_as(fe)
                terms.append(F.mse_loss(fe[m], fo[m]))
        return (sum(terms),)
    return Case("feature-decoding", dict(est=est), hip, ref, dict(est=(0, 0)), loss=True)


LSTM_NAMES = ("w_ih", "w_hh", "b_ih", "b_hh")


def lstm_case(layers, bidirectional, outputs=(0, 1, 2)):
    """``outputs``: which of (y, h_n, c_n) the loss is taken from."""
    In, Hd, Tn = C, M, 17
    dirs = 2 if bidirectional else 1
    torch.manual_seed(layers * 10 + dirs)
    rnn = torch.nn.LSTM(In, Hd, layers, bidirectional=bidirectional)
    g = _gen(9500 + layers + dirs)
    inputs = dict(x=torch.randn(B, In, Tn, generator=g))
    for name in rnn._flat_weights_names:
        inputs[name] = getattr(rnn, name).detach().clone()
    pnames = list(rnn._flat_weights_names)

    def hip(t):
        res = _BF().LSTMFn.apply(t["x"], Hd, layers, bidirectional, 0., False, *[t[n] for n in pnames])
        return tuple(res[i] for i in outputs)

    def ref(t):
        zeros = torch.zeros(layers * dirs, B, Hd, dtype=torch.float64)
        y, h_n, c_n = torch._VF.lstm(t["x"].permute(2, 0, 1), (zeros, zeros), [t[n] for n in pnames], True, layers, 0.,
                                     False, bidirectional, False)
        res = (y.permute(1, 2, 0), h_n, c_n)
        return tuple(res[i] for i in outputs)
    cost = dict(x=(dirs, 0))
    for n in pnames:
        cost[n] = (0, 1) if n.startswith("weight") else (0, 0)
    last = [n for n in pnames if f"_l{layers - 1}" in n]
    extra = [tuple(n for n in last if n.startswith("bias")), tuple(n for n in pnames if n.startswith("weight_hh"))]
    tag = "".join("yhc"[i] for i in outputs)
    return Case(f"lstm-{layers}x{dirs}-{tag}", inputs, hip, ref, cost, extra_subsets=extra)


def _build_cases():
    cases = [conv1d_case(kind, act) for kind in ("same", "k1", "strided", "thead") for act in (0, 1)]
    cases += [convbn_case(tr, res) for tr in (True, False) for res in (False, True)]
    cases += [glu_case(), subject_case(), merger_case(), frontend_case(), clip_case(False), clip_case(True),
              regression_case("l1"), regression_case("mse"), feature_decoding_case(), lstm_case(1, True),
              lstm_case(2, False)]
    return {c.name: c for c in cases}


_CASES = _build_cases()         # CPU tensors only: nothing here touches the GPU or the library
SUBSET_IDS = [(c.name, sub) for c in _CASES.values() for sub in c.subsets()]


def _case(name):
    return _CASES[name]


# ---- engine -----------------------------------------------------------------------------------------------------------
def _launches(H, fn):
    """fn() under a KernelTimer -> (result, [label of every MFMA launch])."""
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        H.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def _counts(labels):
    """(conv launches, weight-gradient launches)."""
    wg = [n for n in labels if n.startswith("gemm_nt") or "wgrad" in n]
    return sum(1 for n in labels if n.startswith("conv") and "wgrad" not in n), len(wg)


def _leaves(case, subset):
    return {k: v.cuda().requires_grad_(k in subset) for k, v in case.inputs.items()}


def _step(case, t, dys):
    outs = case.hip(t)
    torch.autograd.backward(outs, [d.cuda() for d in dys])
    return outs


def _check_against_fp64(case, outs, grads, subset):
    ref_outs, _, ref_grads = case.reference()
    for o, r in zip(outs, ref_outs):
        if case.loss:
            o = float(o.detach())
            assert abs(o - float(r)) <= LOSS_TOL_REL * abs(float(r)), (case.name, o, float(r))
        else:
            assert o.shape == r.shape and rel_l2(o, r) <= FWD_TOL, (case.name, rel_l2(o, r))
    gscale = max(g.norm().item() for g in ref_grads.values())
    for k in case.inputs:
        if k not in subset:
            assert grads[k] is None, (case.name, k, "received a gradient it did not ask for")
            continue
        assert grads[k] is not None and grads[k].shape == case.inputs[k].shape, (case.name, k)
        got, want = grads[k].double().cpu(), ref_grads[k]
        if getattr(case, "l1", False):
            keep = (case.inputs["est"] - case.inputs["out"]).abs() >= 1e-6
            got, want = got[keep], want[keep]
        if case.loss:
            assert rel_l2(got, want) <= LOSS_GRAD_TOL, (case.name, k, rel_l2(got, want))
        else:
            assert close(got, want, GRAD_TOL, gscale), (case.name, k, rel_l2(got, want))


def _run_subset(H, name, subset):
    case = _case(name)
    dys = case.reference()[1]
    mode = H.get_compute_dtype()
    if mode not in case._full_counts:
        full = _leaves(case, tuple(case.inputs))
        case._full_counts[mode] = _counts(_launches(H, lambda: _step(case, full, dys))[1])
    t = _leaves(case, subset)
    outs, labels = _launches(H, lambda: _step(case, t, dys))
    _check_against_fp64(case, outs, {k: v.grad for k, v in t.items()}, subset)
    # the MFMA launch that belongs to a gradient nobody asked for did not happen
    conv, wg = case._full_counts[mode]
    for k in case.inputs:
        if k not in subset:
            conv, wg = conv - case.cost[k][0], wg - case.cost[k][1]
    assert _counts(labels) == (conv, wg), (name, subset, labels, case._full_counts[mode])


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("name,subset", SUBSET_IDS, ids=[f"{n}[{'+'.join(s)}]" for n, s in SUBSET_IDS])
def test_requires_grad_subsets(H, mode, name, subset):
    """Every required gradient meets the tolerance against fp64 autograd, every other one is None, and the launches
    of the skipped gradients are gone.  Narrow class, all three compute modes."""
    _run_subset(H, name, subset)


def test_a_frozen_weight_launches_no_weight_gradient_kernel(H):
    case = _case(f"conv1d-same-gelu-{C}x{M}x{T + 1}")
    t = _leaves(case, ("x", "b"))
    _, labels = _launches(H, lambda: _step(case, t, case.reference()[1]))
    assert labels and not [n for n in labels if n.startswith("gemm_nt")], labels


# ---- wide class ---------------------------------------------------------------------------------------------------------
def _wide_cases(Tn):
    W, Bn = 256, 8
    return [conv1d_case("same", 1, W, W, Bn, Tn, seed=Tn), conv1d_case("thead", 0, W, W, Bn, Tn, seed=Tn),
            convbn_case(True, True, W, W, Bn, Tn, seed=Tn), convbn_case(False, False, W, W, Bn, Tn, seed=Tn),
            glu_case(W, Bn, Tn, seed=Tn)]


_WIDE = {}


@pytest.mark.parametrize("Tn", [192, 132])
@pytest.mark.parametrize("idx", range(5))
def test_wide_kernels_with_subsets(H, idx, Tn):
    """Cin = M = 256, B = 8: the f16x2 conv and weight-gradient tiles, all inputs trainable, then the weight alone and
    the input alone."""
    assert H.get_compute_dtype() == "f16x2"
    L = H.lib()
    assert L.bm_conv_h2_covers(256, 256, Tn, 3, 1) and L.bm_gemm_nt_h2_covers(256, 256, 3, 8, Tn, 1, 1, 0)
    assert not L.bm_gemm_nt_h2_covers(256, 256, 3, 3, 132, 1, 1, 0)         # the shape the issue proposed first
    if Tn not in _WIDE:
        _WIDE[Tn] = _wide_cases(Tn)
    case = _WIDE[Tn][idx]
    dys = case.reference()[1]
    for subset in (tuple(case.inputs), ("w",), ("x",)):
        t = _leaves(case, subset)
        outs, labels = _launches(H, lambda: _step(case, t, dys))
        _check_against_fp64(case, outs, {k: v.grad for k, v in t.items()}, subset)
        assert any(n.startswith("conv_nn_h2w") for n in labels), labels
        assert ("w" in subset) == any(n.startswith("gemm_nt_h2w") for n in labels), (subset, labels)
        assert not [n for n in labels if n.startswith(("conv_nn_x3", "gemm_nt_x3", "conv_nn_kernel", "gemm_nt_kernel"))]


# ---- non-contiguous operands and gradients --------------------------------------------------------------------------------
NONCONTIG = [f"conv1d-same-gelu-{C}x{M}x{T + 1}", f"conv1d-thead-none-{C}x{M}x{T}", f"conv1d-strided-gelu-{C}x{M}x{T}",
             f"convbn-train-res-{M}x{M}x{T + 1}", f"convbn-eval-nores-{C}x{M}x{T}", f"glu-{M}x{T + 1}", "subject-layers",
             "merger", "front-end", "clip-rows", "clip-symmetric", "regression-l1", "regression-mse", "feature-decoding",
             "lstm-1x2-yhc", "lstm-2x1-yhc"]


def _views(case, how):
    """(leaves, tensors handed to the Function, leaf gradient -> gradient in the input's own layout).  Tensors with two
    or more dimensions arrive as transposed views of leaves stored the other way round (non-leaf, non-contiguous);
    ``how`` = "stepped": the first input is every second sample of a leaf twice as long instead."""
    leaves, used, back = {}, {}, {}
    for i, (k, v) in enumerate(case.inputs.items()):
        v = v.cuda()
        if v.dim() < 2:
            leaves[k] = v.clone().requires_grad_(True)
            used[k], back[k] = leaves[k], lambda g: g
        elif i == 0 and how == "stepped":
            big = torch.zeros(*v.shape[:-1], 2 * v.shape[-1], device="cuda")
            big[..., ::2] = v
            leaves[k] = big.requires_grad_(True)
            used[k], back[k] = leaves[k][..., ::2], lambda g: g[..., ::2]
        else:
            leaves[k] = v.transpose(-1, -2).contiguous().requires_grad_(True)
            used[k], back[k] = leaves[k].transpose(-1, -2), lambda g: g.transpose(-1, -2)
        assert torch.equal(used[k], v) and (v.dim() < 2 or v.shape[-1] == 1 or v.shape[-2] == 1
                                            or not used[k].is_contiguous())
    return leaves, used, back


@pytest.mark.parametrize("how", ["transposed", "stepped"])
@pytest.mark.parametrize("name", NONCONTIG)
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_non_contiguous_operands_change_no_bit(H, mode, name, how):
    """Transposed / stepped views of the inputs and non-leaf views of the weights against the contiguous run: the same
    kernels see the same numbers."""
    case = _case(name)
    dys = case.reference()[1]
    base = _leaves(case, tuple(case.inputs))
    base_outs = _step(case, base, dys)
    leaves, used, back = _views(case, how)
    outs = _step(case, used, dys)
    for a, b in zip(outs, base_outs):
        assert torch.equal(a, b), name
    for k in case.inputs:
        assert torch.equal(back[k](leaves[k].grad), base[k].grad), (name, k)


@pytest.mark.parametrize("grad", ["zero_stride", "transposed"])
@pytest.mark.parametrize("name", NONCONTIG)
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_non_contiguous_incoming_gradients_change_no_bit(H, mode, name, grad):
    """``out.sum().backward()`` hands the Function an expanded (zero-stride) gradient, ``out.transpose(1, 2).contiguous()
    .square().sum()`` a transposed one: both against the same numbers passed as a contiguous tensor."""
    case = _case(name)
    base = _leaves(case, tuple(case.inputs))
    outs = case.hip(base)
    if grad == "transposed" and not any(o.dim() >= 3 for o in outs):
        grad = "zero_stride"                       # a scalar loss: nothing to transpose
    if grad == "zero_stride":
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    else:
        torch.autograd.backward(outs, [2 * o.detach() for o in outs])
    t = _leaves(case, tuple(case.inputs))
    outs = case.hip(t)
    if grad == "zero_stride":
        sum(o.sum() for o in outs).backward()
    else:
        sum((o.transpose(1, 2).contiguous() if o.dim() >= 3 else o).square().sum() for o in outs).backward()
    for k in case.inputs:
        assert torch.equal(t[k].grad, base[k].grad), (name, k)


# ---- operands off their 16-byte alignment -----------------------------------------------------------------------------------
# Every input of two or more dimensions and every incoming gradient is a contiguous view 4, 8 or 12 bytes past a 16-byte
# boundary of a flat buffer (helpers.shifted): what a parameter is in FlatAdam's bucket behind one with numel % 4 != 0,
# and an activation that is a slice of a larger buffer.  Held to fp64 like every other state, and to the bits of the
# aligned run: the convs and contractions stage a shifted operand differently and multiply alike, the elementwise
# kernels compute each element alike.  What may differ is a per-channel SUM taken by a streaming kernel that reads
# 16-byte vectors behind aligned pointers and dwords otherwise (T % 4 == 0 only): the two walks add in different orders.
WIDE_T = (192, 132)
WIDE_NAMES = {f"wide-{Tn}-{idx}": (Tn, idx) for Tn in WIDE_T for idx in range(5)}

# case -> (the gradients that are NOT held to the aligned run's bits, the kernel whose sum they are or hang on, the two
# paths).  Everything else of these cases -- the output, the data gradient, the weight gradient -- IS held to the bits.
_SUM = "csrc/norm_act.hip channel_sum_kernel<4> (a thread adds the four lanes of every 256th vector) / <1> (every 256th sample)"
_BWD = ("csrc/norm_act.hip bn_bwd_apply_kernel<4> / <1>: dy is elementwise and equal, its per-channel sum (dbias) is "
        "folded per thread over vectors / over samples")
_BN = ("csrc/norm_act.hip bn_bwd_fused_kernel (one pass, float4, behind aligned dout / pre) / bn_bwd_reduce_kernel<1> + "
       "bn_bwd_apply_kernel<1> (two passes, dwords): the per-channel sums of dz and dz * xhat")
_GLU = "csrc/norm_act.hip glu_bwd_kernel<4> / <1>: du is elementwise and equal, its per-channel sum (dbias) is not"
BITS_EXEMPT = {
    f"conv1d-thead-none-{C}x{M}x{T}": (("b",), _SUM),                 # dbias = channel_sum(dout), dout shifted
    f"conv1d-strided-gelu-{C}x{M}x{T}": (("b",), _BWD),               # act_bn_bwd without BatchNorm: no sums feed dy
    f"convbn-eval-nores-{C}x{M}x{T}": (("b", "gamma", "beta"), _BN),  # eval: dy = scale * dz needs no sum
    "wide-192-0": (("b",), _BWD), "wide-132-0": (("b",), _BWD),       # conv1d-same-gelu
    "wide-192-1": (("b",), _SUM), "wide-132-1": (("b",), _SUM),       # conv1d-thead-none
    # train-mode BatchNorm: dy subtracts the channel means of dz and dz * xhat, so x and w hang on the sums too
    "wide-192-2": (("x", "w", "b", "gamma", "beta"), _BN), "wide-132-2": (("x", "w", "b", "gamma", "beta"), _BN),
    "wide-192-3": (("b", "gamma", "beta"), _BN), "wide-132-3": (("b", "gamma", "beta"), _BN),     # convbn-eval-nores
    "wide-192-4": (("b",), _GLU), "wide-132-4": (("b",), _GLU),       # glu
}
# the cases held to the aligned run's bits in every tensor (T = 49: every kernel takes its dword path either way)
BITS_EQUAL = [n for n in NONCONTIG + list(WIDE_NAMES) if n not in BITS_EXEMPT]
ALIGNMENT_IDS = [(m, n) for n in NONCONTIG for m in MODES] + [("f16x2", n) for n in WIDE_NAMES]


def _alignment_case(name):
    if name not in WIDE_NAMES:
        return _case(name)
    Tn, idx = WIDE_NAMES[name]
    if Tn not in _WIDE:
        _WIDE[Tn] = _wide_cases(Tn)
    return _WIDE[Tn][idx]


def _shifted_leaves(case, k):
    """(leaves, tensors handed to the Function, leaf gradient -> gradient in the input's own layout), as ``_views``:
    every input of two or more dimensions is a leaf that is itself the view buf[k:k + n] of a flat buffer."""
    leaves, used, back = {}, {}, {}
    for name, v in case.inputs.items():
        leaves[name] = (shifted(v, k) if v.dim() >= 2 else v.cuda()).requires_grad_(True)
        assert leaves[name].is_leaf and (v.dim() < 2 or leaves[name].data_ptr() % 16 == 4 * k)
        used[name], back[name] = leaves[name], lambda g: g
    return leaves, used, back


def test_the_bit_equality_exemptions_are_sums_of_the_streaming_kernels():
    """The exemption list holds per-channel sums of norm_act.hip only: no output, and a data or weight gradient only
    where train-mode BatchNorm feeds the sums back into dy."""
    assert set(BITS_EXEMPT) | set(BITS_EQUAL) == set(NONCONTIG) | set(WIDE_NAMES) and not set(BITS_EXEMPT) & set(BITS_EQUAL)
    for name, (tensors, why) in BITS_EXEMPT.items():
        case = _alignment_case(name)
        assert "csrc/norm_act.hip" in why and set(tensors) <= set(case.inputs), name
        assert case.inputs["x"].shape[-1] % 4 == 0, (name, "no 16-byte path to differ from")
        if set(tensors) & {"x", "w"}:
            assert case.name.startswith("convbn-train"), name
    print(f"bit-equality exemptions: {len(BITS_EXEMPT)} of {len(BITS_EXEMPT) + len(BITS_EQUAL)} cases, "
          f"{sum(len(t) for t, _ in BITS_EXEMPT.values())} gradients")


@pytest.mark.parametrize("mode,name", ALIGNMENT_IDS, indirect=["mode"], ids=[f"{n}-{m}" for m, n in ALIGNMENT_IDS])
def test_operands_off_16_byte_alignment(H, mode, name):
    """Shifts of 4, 8 and 12 bytes, applied to all tensors at once: outputs and every gradient against fp64, and
    against the bits of the aligned run but for ``BITS_EXEMPT``."""
    case = _alignment_case(name)
    exempt = set(BITS_EXEMPT[name][0]) if name in BITS_EXEMPT else set()
    dys = case.reference()[1]
    base = _leaves(case, tuple(case.inputs))
    base_outs, labels = _launches(H, lambda: _step(case, base, dys))
    if name in WIDE_NAMES:
        assert any(n.startswith("conv_nn_h2w") for n in labels) and any(n.startswith("gemm_nt_h2w") for n in labels), labels
    for k in (1, 2, 3):
        leaves, used, back = _shifted_leaves(case, k)
        outs = case.hip(used)
        torch.autograd.backward(outs, [shifted(d, k) if d.dim() else d.cuda() for d in dys])
        grads = {n: back[n](leaves[n].grad) for n in case.inputs}
        _check_against_fp64(case, outs, grads, tuple(case.inputs))
        for a, b in zip(outs, base_outs):
            assert torch.equal(a, b), (name, k, "output")
        for n in case.inputs:
            if n not in exempt:
                assert torch.equal(grads[n], base[n].grad), (name, k, n, rel_l2(grads[n], base[n].grad))


# ---- a graph used more than once ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NONCONTIG)
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_second_backward_over_a_retained_graph_is_bit_identical(H, mode, name):
    case = _case(name)
    dys = [d.cuda() for d in case.reference()[1]]
    t = _leaves(case, tuple(case.inputs))
    outs = case.hip(t)
    node = outs[0].grad_fn
    saved = [None if s is None else s.clone() for s in node.saved_tensors]
    assert saved, name
    first = torch.autograd.grad(outs, list(t.values()), dys, retain_graph=True)
    for s, now in zip(saved, node.saved_tensors):
        assert (s is None and now is None) or torch.equal(s, now), (name, "a saved tensor changed in the backward pass")
    second = torch.autograd.grad(outs, list(t.values()), dys)
    for k, a, b in zip(t, first, second):
        assert torch.equal(a, b), (name, k)
    _check_against_fp64(case, [o.detach() for o in outs], dict(zip(t, first)), tuple(case.inputs))


@pytest.mark.parametrize("name", [n for n in NONCONTIG if not n.startswith(("clip", "regression", "feature"))])
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_output_consumed_by_two_heads(H, mode, name):
    """Fan-out: autograd adds the two incoming gradients in fp32 and runs the backward once -- bit-identical to one
    backward with their fp32 sum."""
    case = _case(name)
    dys = [d.cuda() for d in case.reference()[1]]
    dys2 = [torch.randn(d.shape, generator=_gen(5)).cuda() for d in dys]
    base = _leaves(case, tuple(case.inputs))
    torch.autograd.backward(case.hip(base), [a + b for a, b in zip(dys, dys2)])
    t = _leaves(case, tuple(case.inputs))
    outs = case.hip(t)
    (sum((o * d).sum() for o, d in zip(outs, dys)) + sum((o * d).sum() for o, d in zip(outs, dys2))).backward()
    for k in case.inputs:
        assert torch.equal(t[k].grad, base[k].grad), (name, k)


@pytest.mark.parametrize("name", NONCONTIG)
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_one_weight_used_by_two_calls_in_one_graph(H, mode, name):
    """Two calls on different first inputs share every other input: their gradients are the sum of the two calls',
    against fp64 autograd over the same graph."""
    case = _case(name)
    first = next(iter(case.inputs))
    other = torch.randn(case.inputs[first].shape, generator=_gen(11))
    dys = case.reference()[1]

    def graph(t, x2, fn, dev):
        a = fn(t)
        b = fn({**t, first: x2})
        return sum((o * d.to(o)).sum() for o, d in zip(a, dys)) + sum((o * d.to(o)).sum() * 0.5 for o, d in zip(b, dys))
    t64 = {k: v.double().requires_grad_(True) for k, v in case.inputs.items()}
    x64 = other.double().requires_grad_(True)
    graph(t64, x64, case.ref, "cpu").backward()
    t = _leaves(case, tuple(case.inputs))
    x2 = other.cuda().requires_grad_(True)
    graph(t, x2, case.hip, "cuda").backward()
    gscale = max(v.grad.norm().item() for v in t64.values())
    tol = LOSS_GRAD_TOL if case.loss else GRAD_TOL
    for k in list(case.inputs) + ["second input"]:
        got, want = (x2.grad, x64.grad) if k == "second input" else (t[k].grad, t64[k].grad)
        if getattr(case, "l1", False):
            continue                      # sign(e - o) at e ~ o: held by the subset tests on the fixed inputs
        assert close(got, want, tol, gscale), (name, k, rel_l2(got, want))


# ---- LSTM outputs one at a time ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,bidirectional", [(1, True), (2, False)])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["y", "h_n", "c_n"])
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_lstm_outputs_used_one_at_a_time(H, mode, layers, bidirectional, which):
    """A loss from y only, from h_n only, from c_n only: the unused outputs' gradients arrive as materialised zeros."""
    case = lstm_case(layers, bidirectional, outputs=(which,))
    t = _leaves(case, tuple(case.inputs))
    outs = _step(case, t, case.reference()[1])
    _check_against_fp64(case, outs, {k: v.grad for k, v in t.items()}, tuple(case.inputs))


# ---- no tape ----------------------------------------------------------------------------------------------------------
def test_forward_without_a_tape_changes_no_bit(H):
    """SimpleConv under torch.no_grad() and torch.inference_mode() against the grad-enabled forward.  Inference tensors
    have no version counter (``t._version`` raises): ``hip_ops._note`` then simply does not cache."""
    import test_model_gpu as TM
    from brainmagick_amd import synthetic
    model, _ = TM._small_model(merger_dropout=0.0)
    model = model.cuda().train(False)
    sb = synthetic.make_batch(B, C, T, 10, 3, seed=13).to("cuda")
    want = model({"meg": sb.meg.clone()}, sb)
    assert want.requires_grad
    with torch.no_grad():
        got = model({"meg": sb.meg.clone()}, sb)
    assert not got.requires_grad and torch.equal(got, want)
    with torch.inference_mode():
        meg = sb.meg.clone()
        with pytest.raises(RuntimeError):
            meg._version
        got = model({"meg": meg}, sb)
        assert H.amax(meg) is not None and H._noted(meg, "_bm_amax") is None
    assert torch.equal(got, want)
