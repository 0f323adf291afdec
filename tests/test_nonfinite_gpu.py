"""What goes in non-finite comes out non-finite.

The reference asserts ``isfinite`` on its inputs (bm/solver.py:258-260) and, past that, relies on IEEE arithmetic: a NaN
that reaches a layer reaches the loss.  The HIP kernels use NaN-ignoring ``fmaxf`` / ``fminf`` and ``z > 0 ? ... : ...``
selects in many places; this file plants ONE NaN, +inf or -inf into an otherwise ordinary input of each kernel and holds
it to the same operation in torch on the CPU in float64:

* the set of non-finite output elements is the reference's (finite against non-finite, not NaN against inf: the
  reference is not consistent about the class itself -- ``F.gelu(+inf)`` is nan where 0.5 x (1 + erf) is inf, and the
  split contractions turn an inf operand into a NaN);
* the elements that stay finite still meet the kernel's usual tolerance.

Plant positions: the first element, the last, one in the tail behind the last whole 4-vector, one read by another
wavefront than the one that reads element 0.  Every case first proves on the CPU that its reference holds finite AND
non-finite elements (a scalar loss: that it is non-finite), so that neither assertion is vacuous; the few plants that
an operation legitimately swallows (relu(-inf) = 0, sigmoid(+inf) = 1, a sample a strided conv never reads) are marked
``swallowed`` per case and must then come out all finite on both sides."""
import math

import pytest
import torch
from torch.nn import functional as F

from helpers import rel_l2
from oracle import bm_oracle as O

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 5e-6, 2e-5          # tests/test_kernels_gpu.py
NAN, INF = float("nan"), float("inf")
VALUES = [("nan", NAN), ("+inf", INF), ("-inf", -INF)]


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _positions(n):
    """first, another wavefront's (element 261: thread 65 of a float4 walk, lane 5 of the second workgroup of a scalar
    one), the tail behind the last whole 4-vector of an n % 4 != 0 tensor (else the second to last), last."""
    tail = n - 1 - (n % 4 > 1) if n % 4 else n - 2
    return sorted({p for p in (0, 261, tail, n - 1) if 0 <= p < n})


def plant_check(what, x, run, ref, tol, values=VALUES, positions=None, swallowed=False, min_hits=1):
    """``x``: the fp32 CPU tensor that takes the plant; ``run(x on the GPU)`` -> the kernel's outputs; ``ref(x in fp64)`` ->
    the same outputs from torch on the CPU.  See the module text for what is asserted.  Returns the number of plants
    whose reference was non-finite somewhere."""
    cases = []
    for pos in positions if positions is not None else _positions(x.numel()):
        for name, val in values:
            xp = x.clone()
            xp.view(-1)[pos] = val
            want = [w.detach().double() for w in ref(xp.double())]
            bad = [~torch.isfinite(w) for w in want]
            tag = f"{what}: {name} at {pos}"
            hit = any(bool(b.any()) for b in bad)
            if not hit:
                assert swallowed, f"{tag}: the reference swallows the plant -- the case proves nothing"
            else:
                for w, b in zip(want, bad):
                    if w.numel() > 1 and bool(b.any()):
                        assert not bool(b.all()), f"{tag}: the reference leaves nothing finite to compare"
            cases.append((tag, xp, want, bad))
    hits = sum(any(bool(b.any()) for b in bad) for _, _, _, bad in cases)
    assert hits >= min_hits, f"{what}: every plant is swallowed by the reference"
    for tag, xp, want, bad in cases:
        got = [g.detach().double().cpu() for g in run(xp.cuda())]
        assert len(got) == len(want), tag
        for k, (g, w, b) in enumerate(zip(got, want, bad)):
            g = g.reshape(w.shape)
            gb = ~torch.isfinite(g)
            assert torch.equal(gb, b), (f"{tag}, output {k}: non-finite elements differ from the reference's: "
                                        f"{int(gb.sum())} here, {int(b.sum())} there, first difference at flat index "
                                        f"{int((gb != b).flatten().nonzero()[0])}")
            if bool((~b).any()):
                e = rel_l2(g[~b], w[~b])
                assert e < (tol[k] if isinstance(tol, (list, tuple)) else tol), (tag, k, e)
    return hits


def _same_values(a, b):
    """torch.equal that also demands NaN where the other holds NaN."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- center_scale: the CLASS must match torch's clamp_ -----------------------------------------------------------------
@pytest.mark.parametrize("B,C,T", [(3, 5, 68), (3, 5, 67)])              # the float4 walk and the scalar one
@pytest.mark.parametrize("clip", [True, False])
def test_center_scale_keeps_nan_and_clamps_inf(H, B, C, T, clip):
    g = _gen(B + C + T)
    limit = 20.0
    x = torch.randn(B, C, T, generator=g) * 2 + 0.5
    x[1, 2, 3] = 500.0                                   # segment 1 is over the limit on its own
    center = torch.randn(1, C, generator=g) * 0.3
    scale = torch.rand(1, C, generator=g) + 0.5
    seg = C * T
    for pos in sorted(set(_positions(B * seg)) | {seg + 7}):           # seg + 7: in the segment that is over the limit
        for name, val in VALUES:
            xp = x.clone()
            xp.view(-1)[pos] = val
            ref = (xp - center[0][None, :, None]) / scale[0][None, :, None]
            if clip:
                ref.clamp_(-limit, limit)                # bm/norm.py:333: NaN stays NaN, +-inf becomes +-limit
                assert math.isnan(val) == bool(torch.isnan(ref).any()) and bool(torch.isfinite(ref).any())
            out, maxabs = H.center_scale(xp.cuda(), center.cuda(), scale.cuda(), clip=clip, limit=limit,
                                         want_maxabs=True)
            assert _same_values(out, ref), f"center_scale clip={clip}: {name} at {pos}"
            # bm/norm.py:334-335: reject = max|meg| > limit with torch's NaN-propagating max: a segment that holds a NaN
            # has max = NaN, NaN > limit is False, the segment is KEPT -- even segment 1 with its 500 -- and the
            # finiteness assert behind it reports the batch.  +-inf (clip off) rejects the segment.
            ref_max = ref.abs().view(B, -1).max(-1)[0]
            keep_ref = ~(ref_max > limit)
            b = pos // seg
            if math.isnan(val):
                assert bool(keep_ref[b]) and math.isnan(float(ref_max[b]))
            elif not clip:
                assert not bool(keep_ref[b])
            assert _same_values(maxabs, ref_max), f"center_scale clip={clip} maxabs: {name} at {pos}"
            assert torch.equal(~(maxabs > limit).cpu(), keep_ref)        # what ScaleReject computes (norm.py here)


# ---- the streaming kernels of norm_act.hip -----------------------------------------------------------------------------
_ACTS = {"none": (lambda z: z), "gelu": F.gelu, "relu": F.relu, "leaky": (lambda z: F.leaky_relu(z, 0.1))}


@pytest.mark.parametrize("act", ["none", "gelu", "relu", "leaky"])
@pytest.mark.parametrize("T,affine,residual", [(68, True, True), (67, True, False), (68, False, False), (67, False, True)])
def test_affine_act_res(H, act, T, affine, residual):
    g = _gen(T + affine + 2 * residual)
    B, C = 2, 3
    y = torch.randn(B, C, T, generator=g)
    scale = torch.rand(C, generator=g) + 0.5 if affine else None         # positive: the sign of an inf is kept
    shift = torch.randn(C, generator=g) if affine else None
    res = torch.randn(B, C, T, generator=g) if residual else None
    code = {"none": H.ACT_NONE, "gelu": H.ACT_GELU, "relu": H.ACT_RELU, "leaky": H.ACT_LEAKY}[act]

    def run(yg):
        cu = lambda t: None if t is None else t.cuda()     # noqa: E731
        return [H.affine_act_res(yg, cu(scale), cu(shift), cu(res), code, 0.1)]

    def ref(yd):
        z = yd * scale.double()[None, :, None] + shift.double()[None, :, None] if affine else yd
        out = _ACTS[act](z)
        return [out + res.double() if residual else out]
    plant_check(f"affine_act_res[{act}] T={T} affine={affine} res={residual}", y, run, ref, FWD_TOL,
                swallowed=act == "relu")                   # relu(-inf) = 0


@pytest.mark.parametrize("mode", ["none", "eval", "train"])
@pytest.mark.parametrize("T", [68, 67])
def test_act_bn_bwd(H, mode, T):
    """NaN / inf in ``dout`` (every BatchNorm mode: in train mode the whole channel goes through the two sums) and in ``y``
    (no BatchNorm, eval mode)."""
    g = _gen(T)
    B, C = 3, 4
    y = torch.randn(B, C, T, generator=g) * 1.5 + 0.3
    dout = torch.randn(B, C, T, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5

    def reference(yd, dd):
        yr = yd.clone().requires_grad_(True)
        if mode == "none":
            z = yr
        else:
            z = F.batch_norm(yr, rm.double(), rv.double(), gamma.double(), beta.double(), training=mode == "train",
                             momentum=0.0, eps=1e-5)
        F.gelu(z).backward(dd)
        return [yr.grad, _bias_grad(yr.grad.sum((0, 2)))]

    def _bias_grad(db):
        # sum(dy) of a BatchNorm input is analytically 0 in train mode (round-off on both sides): only WHERE it is finite
        return torch.where(torch.isfinite(db), torch.zeros_like(db), db) if mode == "train" else db

    def kernel(yg, dg):
        if mode == "none":
            stats = [None] * 4
        else:
            yd = yg.double().cpu()
            mean = yd.mean((0, 2)) if mode == "train" else rm.double()
            var = yd.var((0, 2), unbiased=False) if mode == "train" else rv.double()
            invstd = 1.0 / torch.sqrt(var + 1e-5)
            sc = gamma.double() * invstd
            stats = [t.float().cuda() for t in (sc, beta.double() - mean * sc, mean, invstd)]
        dy, _, _, dbias = H.act_bn_bwd(dg, yg, *stats, mode == "train", H.ACT_GELU)
        return [dy, _bias_grad(dbias)]
    plant_check(f"act_bn_bwd[{mode}] T={T}, plant in dout", dout, lambda dg: kernel(y.cuda(), dg),
                lambda dd: reference(y.double(), dd), [GRAD_TOL, 1e-4])
    if mode != "train":
        plant_check(f"act_bn_bwd[{mode}] T={T}, plant in y", y, lambda yg: kernel(yg, dout.cuda()),
                    lambda yd: reference(yd, dout.double()), [GRAD_TOL, 1e-4])


def test_relu_backward_passes_the_gradient_of_a_nan_activation(H):
    """torch's relu backward is threshold_backward: 0 where the result is <= 0, the incoming gradient elsewhere -- a NaN
    activation is not <= 0, so the gradient passes."""
    g = _gen(4)
    y = torch.randn(2, 3, 68, generator=g)
    dout = torch.randn(2, 3, 68, generator=g)

    def ref(yd):
        yr = yd.clone().requires_grad_(True)
        F.relu(yr).backward(dout.double())
        return [yr.grad]
    n = plant_check("act_bn_bwd[relu], plant in y", y,
                    lambda yg: [H.act_bn_bwd(dout.cuda(), yg, None, None, None, None, False, H.ACT_RELU)[0]], ref,
                    GRAD_TOL, swallowed=True, min_hits=0)  # the gradient stays finite under every plant
    assert n == 0


@pytest.mark.parametrize("T", [68, 67])
def test_glu(H, T):
    g = _gen(T + 9)
    B, Hc = 2, 3
    u = torch.randn(B, 2 * Hc, T, generator=g)
    dout = torch.randn(B, Hc, T, generator=g)
    plant_check(f"glu_fwd T={T}", u, lambda ug: [H.glu_fwd(ug)], lambda ud: [F.glu(ud, dim=1)], FWD_TOL,
                swallowed=True)                            # sigmoid(+inf) = 1, sigmoid(-inf) = 0 in the gate half

    def bwd_ref(ud, dd):
        ur = ud.clone().requires_grad_(True)
        F.glu(ur, dim=1).backward(dd)
        return [ur.grad, ur.grad.sum((0, 2))]
    plant_check(f"glu_bwd T={T}, plant in dout", dout, lambda dg: list(H.glu_bwd(dg, u.cuda())),
                lambda dd: bwd_ref(u.double(), dd), [GRAD_TOL, 1e-4])
    plant_check(f"glu_bwd T={T}, NaN in u", u, lambda ug: list(H.glu_bwd(dout.cuda(), ug)),
                lambda ud: bwd_ref(ud, dout.double()), [GRAD_TOL, 1e-4], values=VALUES[:1])


@pytest.mark.parametrize("B,C,T", [(3, 4, 68), (9, 2, 67)])
def test_channel_reductions(H, B, C, T):
    x = torch.randn(B, C, T, generator=_gen(B + T)) + 0.3

    def stats(xg):
        s = H.channel_stats(xg).double().sum(0)
        return [s[:, 0], s[:, 1]]
    plant_check("channel_stats", x, stats, lambda xd: [xd.sum((0, 2)), (xd * xd).sum((0, 2))], 1e-5)
    plant_check("channel_sum", x, lambda xg: [H.channel_sum(xg)], lambda xd: [xd.sum((0, 2))], GRAD_TOL)
    plant_check("time_sums_t", x, lambda xg: [H.time_sums_t(xg)], lambda xd: [xd.sum(2).t()], FWD_TOL)


def test_bn_finalize_leaves_the_running_estimates_alone_on_nonfinite_statistics(H):
    """A DELIBERATE deviation from torch (which would write the NaN into running_mean / running_var for good): the Solver
    reports a non-finite batch a few launches later and rolls the step back (solver.py, ``_post_flags``), so bn_finalize
    keeps the running estimates of a channel whose batch statistics are not finite.  Pinned as it is: the batch
    statistics themselves ARE non-finite for that channel (the forward pass propagates), the other channels update."""
    C, ntiles, count = 5, 7, 7 * 50
    g = _gen(12)
    for name, val in VALUES:
        stats = torch.rand(ntiles, C, 2, generator=g) * 50
        stats[..., 1] += 60
        stats[3, 2, 0] = val                                          # channel 2's sum
        rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        rm_g, rv_g = rm.cuda(), rv.cuda()
        nb = torch.zeros((), dtype=torch.int64).cuda()
        mean, invstd, scale, shift = H.bn_finalize(stats.cuda(), count, torch.ones(C).cuda(), torch.zeros(C).cuda(),
                                                   rm_g, rv_g, nb, 0.1, 1e-5)
        bad = torch.zeros(C, dtype=torch.bool)
        bad[2] = True
        assert torch.equal(~torch.isfinite(mean).cpu(), bad) and torch.equal(~torch.isfinite(shift).cpu(), bad), name
        assert float(rm_g[2]) == float(rm[2]) and float(rv_g[2]) == float(rv[2]), name
        m64 = stats[..., 0].double().sum(0) / count
        assert rel_l2(rm_g[~bad.cuda()], (0.9 * rm.double() + 0.1 * m64)[~bad]) < 1e-6
        assert bool((rv_g.cpu() != rv)[~bad].all()) and int(nb) == 1


# ---- contractions ------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(32, 128, 1, 200, 1), (20, 24, 3, 50, 2)]        # Cin, M, KS, T, B


@pytest.mark.parametrize("mode", ["f16x2", "f32x3", "f32"])
@pytest.mark.parametrize("Cin,M,KS,T,B", CONV_SHAPES)
def test_conv_forward(H, mode, Cin, M, KS, T, B):
    """conv_nn and conv_strided in the three compute modes (an inf operand may come out NaN in the split modes: still
    non-finite), plain and through the ReLU epilogue."""
    g = _gen(Cin + M + KS)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(M, Cin, KS, generator=g) / math.sqrt(Cin * KS)
    b = torch.randn(M, generator=g)
    stride, pad = 2, KS // 2
    Tout = H.conv_out_len(T, KS, stride, 1, pad, False)
    H.set_compute_dtype(mode)
    try:
        for act, fn in ((H.ACT_NONE, lambda z: z), (H.ACT_RELU, F.relu)):
            plant_check(f"conv_nn[{mode}] act={act} {Cin}->{M} k{KS} T={T}", x,
                        lambda xg: [H.conv_nn(xg, H.pack_conv_fwd(w.cuda(), (T, 1)), M, KS, 1, bias=b.cuda(), act=act)[1]],
                        lambda xd: [fn(F.conv1d(xd, w.double(), b.double(), padding=pad))], FWD_TOL,
                        swallowed=act == H.ACT_RELU,           # relu(-inf) = 0
                        # ... which only exact fp32 can tell from relu(+inf): the split modes turn an inf operand into
                        # a NaN in every output it reaches, and relu keeps a NaN -- NaN plants only there
                        values=VALUES[:1] if act == H.ACT_RELU and mode != "f32" else VALUES)
            plant_check(f"conv_strided[{mode}] act={act} {Cin}->{M} k{KS} T={T}", x,
                        lambda xg: [H.conv_strided(xg, H.pack_strided_rows_first(w.cuda()), M, Tout, KS, stride, 1, pad,
                                                   False, bias=b.cuda(), act=act)[1]],
                        lambda xd: [fn(F.conv1d(xd, w.double(), b.double(), stride=stride, padding=pad))], FWD_TOL,
                        swallowed=True)                        # stride 2, one tap: the odd samples are never read
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("mode", ["f16x2", "f32x3", "f32"])
def test_gemm_nt(H, mode):
    g = _gen(6)
    S, M, Cn, T = 2, 24, 20, 50
    a = torch.randn(S, M, T, generator=g)
    x = torch.randn(S, Cn, T, generator=g)
    H.set_compute_dtype(mode)
    try:
        plant_check(f"gemm_nt[{mode}] plant in a", a, lambda ag: [H.gemm_nt(ag, x.cuda(), S, M, Cn, T)[0, :, :, 0]],
                    lambda ad: [torch.einsum("smt,sct->mc", ad, x.double())], GRAD_TOL)
        plant_check(f"gemm_nt[{mode}] plant in x", x, lambda xg: [H.gemm_nt(a.cuda(), xg, S, M, Cn, T)[0, :, :, 0]],
                    lambda xd: [torch.einsum("smt,sct->mc", a.double(), xd)], GRAD_TOL)
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


# ---- softmaxes ---------------------------------------------------------------------------------------------------------
def test_softmaxes(H):
    g = _gen(15)
    U, Oc, C = 2, 3, 67
    scores = torch.randn(U, Oc, C, generator=g)
    pos = torch.rand(U, C, 2, generator=g)
    pos[1, 60:] = O.INVALID                          # the LAST element of the scores sits under a masked sensor
    off = torch.zeros(U, C).masked_fill(O.is_invalid(pos), -INF).double()
    # -inf is swallowed (probability 0); NaN and +inf take the row with them -- under a masked sensor too: the reference
    # ADDS the -inf offset to the score (bm/models/common.py:356), NaN + -inf and +inf + -inf are NaN
    plant_check("masked_softmax", scores, lambda sg: [H.masked_softmax(sg, pos.cuda(), None, 0.0)],
                lambda sd: [torch.softmax(sd + off[:, None], 2)], FWD_TOL, swallowed=True)
    x = scores.view(U * Oc, C)
    plant_check("row_softmax", x, lambda xg: [H.row_softmax(xg)], lambda xd: [torch.softmax(xd, 1)], FWD_TOL,
                swallowed=True)
    w = torch.softmax(x.double(), 1).float()
    dw = torch.randn(U * Oc, C, generator=g)
    plant_check("softmax_bwd, plant in dw", dw, lambda dg: [H.softmax_bwd(w.cuda(), dg)],
                lambda dd: [w.double() * (dd - (w.double() * dd).sum(1, keepdim=True))], GRAD_TOL)
    plant_check("softmax_bwd, plant in w", w, lambda wg: [H.softmax_bwd(wg, dw.cuda())],
                lambda wd: [wd * (dw.double() - (wd * dw.double()).sum(1, keepdim=True))], GRAD_TOL)


# ---- retrieval ---------------------------------------------------------------------------------------------------------
def test_topk_rows(H):
    """Nothing is computed, so nothing propagates: what matters is WHERE the plant ranks.  ``probs.topk`` puts a NaN first
    (above +inf) and -inf last; bm_topk_rows returns torch.sort(descending, stable) cut to k (include/bm_hip.h), so a
    row of NaN probabilities -- all sensors banned -- retrieves the same candidates here as in the reference."""
    rows, cols = 5, 67
    x = torch.softmax(torch.randn(rows, cols, generator=_gen(21)), 1)
    labels = torch.arange(cols)
    for pos in _positions(rows * cols):
        for name, val in VALUES:
            xp = x.clone()
            xp.view(-1)[pos] = val
            r, c = divmod(pos, cols)
            for k in (1, 10, cols):
                want = torch.sort(xp.double(), dim=1, descending=True, stable=True).indices[:, :k]
                ref = xp.topk(k, dim=1)
                if val != -INF:
                    assert int(ref.indices[r, 0]) == c                   # the reference ranks NaN and +inf first
                elif k == cols:
                    assert int(ref.indices[r, -1]) == c
                idx, val_k, hits = H.topk_rows(xp.cuda(), k, labels.cuda(), torch.full((rows,), c).cuda())
                assert torch.equal(idx.cpu().long(), want), f"topk_rows k={k}: {name} at {pos}"
                assert _same_values(val_k, ref.values), f"topk_rows k={k}: {name} at {pos}"
                assert int(hits[r]) == (1 if val != -INF or k == cols else int(c in want[r].tolist()))
    xp = x.clone()
    xp[3] = NAN
    idx, val_k, _ = H.topk_rows(xp.cuda(), 10)
    assert idx[3].tolist() == list(range(10)) and bool(torch.isnan(val_k[3]).all()) and bool(torch.isfinite(val_k[:3]).all())


# ---- ClipLoss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [68, 67, 1023])
def test_clip_inv_norms(H, K):
    cand = torch.randn(5, K, generator=_gen(K)) + 0.2
    # 1 / (1e-8 + inf) = 0: an infinite candidate has a FINITE inverse norm in the reference too (swallowed)
    plant_check(f"clip_inv_norms K={K}", cand, lambda cg: [H.clip_inv_norms(cg)],
                lambda cd: [1 / (1e-8 + cd.norm(dim=1))], 1e-6, swallowed=True)


def test_clip_ce(H):
    """A NaN score makes its whole row NaN (scores, probabilities, gradient, the mean loss); a ``col_valid``-masked column
    keeps a gradient of exactly 0 beside it; a row whose columns are all masked is NaN like the reference's softmax of
    all -inf."""
    g = _gen(33)
    B, Bc, nsplit = 5, 70, 3
    part = torch.randn(nsplit, B, Bc, generator=g)
    inv = 1.0 / (torch.rand(Bc, generator=g) + 0.5)
    valid = torch.ones(Bc)
    valid[[9, 66]] = 0

    def ref(pd):
        s = (pd.sum(0) * inv.double()).masked_fill(valid == 0, -INF)
        pr = torch.softmax(s, 1)
        d = (pr - F.one_hot(torch.arange(B), Bc)) / B * inv.double()
        return [s, pr, d.masked_fill(valid == 0, 0.0), F.cross_entropy(s, torch.arange(B))]

    def run(pg):
        return list(H.clip_ce(pg, inv.cuda(), True, True, True, col_valid=valid.cuda()))
    at = [0, 2 * B * Bc + 3 * Bc + 64, nsplit * B * Bc - 1]          # split 0 row 0; split 2 row 3 second wavefront; last
    plant_check("clip_ce", part, run, ref, [FWD_TOL, 1e-5, GRAD_TOL, 1e-5], values=VALUES[:1], positions=at)
    for pos in at:
        pp = part.clone()
        pp.view(-1)[pos] = NAN
        row = pos % (B * Bc) // Bc
        scores, probs, dscaled, loss = run(pp.cuda())
        assert int(torch.isnan(scores).sum()) == 1 and bool(torch.isnan(probs[row]).all())
        assert int(torch.isnan(probs).sum()) == Bc
        assert float(dscaled[:, [9, 66]].abs().max()) == 0.0 and math.isnan(float(loss))
    # every column masked
    scores, probs, dscaled, loss = H.clip_ce(part.cuda(), inv.cuda(), True, True, True, col_valid=torch.zeros(Bc).cuda())
    assert bool(torch.isnan(torch.softmax(torch.full((B, Bc), -INF), 1)).all())            # the reference
    assert bool(torch.isnan(probs).all()) and math.isnan(float(loss)) and float(dscaled.abs().max()) == 0.0


def test_clip_ce_cols(H):
    """A NaN in a target column: that column's loss and its column of ``dscaled`` are NaN, the other columns stay finite
    and right (the mixed scalar loss is NaN)."""
    g = _gen(34)
    B, Bc, off = 5, 70, 60
    scores = torch.randn(B, Bc, generator=g) * 2
    inv = 1.0 / (torch.rand(Bc, generator=g) + 0.5)
    dscaled = torch.randn(B, Bc, generator=g) * 0.01

    def ref(sd):
        cols = sd[:, off:off + B]
        loss_col = torch.logsumexp(cols, 0) - torch.diagonal(cols)
        d = dscaled.double() * 0.5
        d[:, off:off + B] += 0.5 / B * inv.double()[off:off + B] * (torch.softmax(cols, 0) - torch.eye(B).double())
        return [loss_col, d, 0.5 * 1.25 + 0.5 * loss_col.mean()]

    def run(sg):
        d, loss = dscaled.cuda(), torch.tensor(1.25).cuda()
        return [H.clip_ce_cols(sg, inv.cuda(), d, loss, off), d, loss]
    at = [off, 3 * Bc + off + 2, B * Bc - 6]                           # rows 0, 3 and 4 of target columns 0, 2 and 4
    plant_check("clip_ce_cols", scores, run, ref, [FWD_TOL, GRAD_TOL, 1e-5], values=VALUES[:2], positions=at)
    for pos, j in zip(at, (0, 2, 4)):
        sp = scores.clone()
        sp.view(-1)[pos] = NAN
        loss_col, d, _ = run(sp.cuda())
        bad = torch.zeros(B, dtype=torch.bool)
        bad[j] = True
        assert torch.equal(torch.isnan(loss_col).cpu(), bad)
        assert bool(torch.isnan(d[:, off + j]).all()) and int(torch.isnan(d).sum()) == B


@pytest.mark.parametrize("mode,B,Bc,Fd,T,rows,off", [
    ("f32", 5, 30, 8, 12, 7, 12), ("f32x3", 5, 30, 8, 12, 7, 12), ("f16x2", 5, 30, 8, 12, 7, 12),
    ("f16x2", 130, 300, 24, 77, 128, 128),      # the wide f16x2 kernels run the first two blocks, the plant is in the third
])
def test_clip_loss_with_a_nan_candidate_in_a_late_block(H, monkeypatch, mode, B, Bc, Fd, T, rows, off):
    """The candidate set walked in row blocks (tests/test_clip_blocks_gpu.py, cases B and A), one NaN in a candidate of
    the LAST block.  The reference: that candidate's norm and so its score column are NaN, the other columns stay
    finite; every row's softmax holds a NaN, so the loss, all of dEst and all of dCand are NaN.

    f16x2: ``share_amax`` hands every block the maximum of the whole candidate tensor.  The amax pass folds with
    ``fmaxf``, which drops a NaN: the shared maximum is that of the FINITE elements (pinned below), the clean blocks are
    scaled as if the plant were not there and the NaN travels through the operand split of its own block alone -- a NaN
    maximum (scale 1, no scaling at all) would not have spoilt the other columns either, but it would have cost them
    their f16 headroom."""
    from brainmagick_amd import functional as BF
    g = _gen(B + Bc)
    K = Fd * T
    est = torch.randn(B, Fd, T, generator=g) * 0.5
    cand = torch.randn(Bc, Fd, T, generator=g) * 1.5 + 0.2
    est += 0.02 * cand[off:off + B]
    bad_row = Bc - 1
    cand[bad_row, Fd // 2, 5] = NAN
    finite_max = float(cand[torch.isfinite(cand)].abs().max())
    e = est.double().requires_grad_(True)
    c = cand.double().requires_grad_(True)
    s = e.flatten(1) @ c.flatten(1).t() / (1e-8 + c.flatten(1).norm(dim=1))
    ref_loss = F.cross_entropy(s, torch.arange(B) + off)
    (ref_loss * 1.7).backward()
    bad = ~torch.isfinite(s.detach())
    assert bool(bad[:, bad_row].all()) and int(bad.sum()) == B and math.isnan(float(ref_loss))
    assert bool(torch.isnan(e.grad).all()) and bool(torch.isnan(c.grad).all())
    monkeypatch.setattr(BF, "_CLIP_BLOCK_BYTES", rows * K * 4)
    blocks = BF._candidate_blocks(Bc, K)
    assert len(blocks) > 2 and blocks[-1][0] <= bad_row and blocks[-2][0] + blocks[-2][1] <= bad_row
    H.set_compute_dtype(mode)
    try:
        eg, cg = est.cuda().requires_grad_(True), cand.cuda().requires_grad_(True)
        loss, scores = BF.ClipLossFn.apply(eg, cg, off)
        (loss * 1.7).backward()
        if mode == "f16x2":
            assert float(H.amax(cg).max()) == finite_max
        no_grad_scores = BF.clip_scores(eg.detach(), cg.detach())
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
    for name, got in (("scores", scores), ("clip_scores", no_grad_scores)):
        got = got.double().cpu()
        assert torch.equal(~torch.isfinite(got), bad), f"{name}[{mode}]: non-finite elements differ from the reference's"
        assert rel_l2(got[~bad], s.detach()[~bad]) < FWD_TOL
    assert math.isnan(float(loss))
    assert bool(torch.isnan(eg.grad).all()) and bool(torch.isnan(cg.grad).all())


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("T", [68, 67])
def test_regress_loss(H, kind, T):
    """The plant under a TRUE mask bit reaches the loss and its own gradient element; under a FALSE bit the reference's
    ``est[mask]`` never reads it: loss and gradient are finite and right."""
    g = _gen(T + len(kind))
    B, Fd = 3, 4
    est = torch.randn(B, Fd, T, generator=g)
    out = torch.randn(B, Fd, T, generator=g)
    mask = torch.rand(B, 1, T, generator=g) > 0.3
    mask[0, 0, 0] = mask[-1, 0, -1] = True
    mask[0, 0, 5] = False
    fn = F.l1_loss if kind == "l1" else F.mse_loss

    def ref(ed):
        er = ed.clone().requires_grad_(True)
        sel = mask.expand_as(er)
        loss = fn(er[sel], out.double()[sel])
        loss.backward()
        return [loss.detach(), er.grad]

    def run(eg):
        loss, count = H.regress_loss_fwd(eg, out.cuda(), mask.cuda(), kind)
        dest, _ = H.regress_loss_bwd(eg, out.cuda(), mask.cuda(), kind, torch.ones((), device="cuda"), count)
        return [loss, dest]
    n = est.numel()
    assert plant_check(f"regress[{kind}] T={T} under a true bit", est, run, ref, [1e-5, GRAD_TOL],
                       positions=[0, n - 1]) == 6
    assert plant_check(f"regress[{kind}] T={T} under a false bit", est, run, ref, [1e-5, GRAD_TOL], positions=[5],
                       swallowed=True, min_hits=0) == 0


# ---- the small row kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1024, 1023])
def test_rowwise_dot_and_row_axpy_sub(H, K):
    g = _gen(K)
    a = torch.randn(3, K, generator=g)
    b = 0.5 * a + 0.3 * torch.randn(3, K, generator=g)
    coef = torch.randn(3, generator=g)
    plant_check(f"rowwise_dot K={K}", a, lambda ag: [H.rowwise_dot(ag, b.cuda())],
                lambda ad: [(ad * b.double()).sum(1)], FWD_TOL)
    plant_check(f"row_axpy_sub K={K}, plant in x", a, lambda ag: [H.row_axpy_sub(b.cuda(), ag, coef.cuda())],
                lambda ad: [b.double() - coef.double()[:, None] * ad], FWD_TOL)
    plant_check(f"row_axpy_sub K={K}, plant in y", b, lambda bg: [H.row_axpy_sub(bg, a.cuda(), coef.cuda())],
                lambda bd: [bd - coef.double()[:, None] * a.double()], FWD_TOL)


def test_adam_step_with_a_nonfinite_gradient_element(H):
    g = _gen(40)
    n = 1031
    p, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 0.01 + 1e-4

    def ref(gd):
        pd, md, vd = p.double(), m.double(), v.double()
        O.adam_step(pd, gd, md, vd, 2)
        return [pd, md, vd]

    def run(gg):
        pg, mg, vg = p.cuda(), m.cuda(), v.cuda()
        H.adam_step(pg, gg, mg, vg, 2, 3e-4, 0.9, 0.999, 1e-8)
        return [pg, mg, vg]
    # +-inf: exp_avg / sqrt(exp_avg_sq) = inf / inf = NaN in the parameter, like torch.optim.Adam
    assert plant_check("adam_step", grad, run, ref, 1e-6) == 12


# ---- LSTM --------------------------------------------------------------------------------------------------------------
def _lstm_reference(whh, gx, dy, dcn):
    """The fp64 recurrence of tests/test_convrnn_gpu.py::test_step_kernels_stay_inside_their_buffers:
    (y [T, H * dirs, B], dg [dirs, T, 4H, B])."""
    dirs, (T, H4, B) = len(whh), gx[0].shape
    Hd = H4 // 4
    ys, dgs = [], []
    for d in range(dirs):
        w = whh[d].double()
        pre = gx[d].double().clone().requires_grad_(True)
        h = torch.zeros(Hd, B, dtype=torch.float64)
        cc = torch.zeros(Hd, B, dtype=torch.float64)
        hs = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            a = w @ h + pre[t]
            i, f, gg, o = a[:Hd].sigmoid(), a[Hd:2 * Hd].sigmoid(), a[2 * Hd:3 * Hd].tanh(), a[3 * Hd:].sigmoid()
            cc = f * cc + i * gg
            h = o * cc.tanh()
            hs[t] = h
        y = torch.stack(hs)
        ((y * dy[:, d * Hd:(d + 1) * Hd].double()).sum() + (cc * dcn[d].double()).sum()).backward()
        ys.append(y.detach())
        dgs.append(pre.grad)
    return torch.cat(ys, 1), torch.stack(dgs)


def _lstm_setup(gain=1.0):
    g = _gen(45)
    Hd, B, T, dirs = 45, 5, 4, 2
    whh = [torch.randn(4 * Hd, Hd, generator=g) / Hd ** 0.5 for _ in range(dirs)]
    gx = [torch.randn(T, 4 * Hd, B, generator=g) * gain for _ in range(dirs)]
    dy = torch.randn(T, Hd * dirs, B, generator=g)
    dcn = torch.randn(dirs, Hd, B, generator=g)
    return Hd, B, T, dirs, whh, gx, dy, dcn


def _lstm_run(H, whh, gx, dy, dcn):
    whh_g = [w.cuda() for w in whh]
    y, gates, c = H.lstm_layer_fwd(whh_g, [t.cuda() for t in gx])
    dg = H.lstm_layer_bwd(whh_g, dy.cuda(), gates, c, dcn.cuda().clone())
    return y, dg


def test_lstm_layer(H):
    """H 45, B 5, T 4, two directions; the plant sits in ``gx`` of direction 0 at step 1: unit j of column b is non-finite
    from step 1 on, and through W_hh every unit of that column from step 2 on; direction 1 never sees it."""
    Hd, B, T, dirs, whh, gx, dy, dcn = _lstm_setup()
    step = 4 * Hd * B
    at = [step, step + 261, 2 * step - 2, 2 * step - 1]             # all inside step 1: gates i .. o, columns 0 .. B - 1

    def ref(g0):
        y, dg = _lstm_reference(whh, [g0.float(), gx[1]], dy, dcn)
        assert bool(torch.isfinite(y[0]).all()) and bool(torch.isfinite(y[:, Hd:]).all())      # step 0; direction 1
        return [y, dg]
    # (the output gate's sigmoid(-inf) = 0 times a finite tanh(c) is a finite h: swallowed in the forward pass)
    plant_check("lstm_layer", gx[0], lambda g0: list(_lstm_run(H, whh, [g0.cpu(), gx[1]], dy, dcn)), ref,
                [FWD_TOL, GRAD_TOL], values=VALUES[:1], positions=at)


# ---- the finiteness flags ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 1031])
def test_nonfinite_flags(H, n):
    """``amax(x, nonfinite_flag)`` and ``clip_inv_norms(cand, nonfinite_flag)`` (the reference's isfinite asserts): up for a
    NaN, +inf or -inf wherever it sits, down for the largest finite magnitudes."""
    x = torch.randn(n, generator=_gen(n))
    for maker in (lambda t, f: H.amax(t.cuda(), nonfinite_flag=f),
                  lambda t, f: H.clip_inv_norms(t.view(1, n).cuda(), nonfinite_flag=f),
                  lambda t, f: H.amax(torch.cat([torch.zeros(1), t]).cuda()[1:], nonfinite_flag=f)):     # misaligned head
        for pos in _positions(n):
            for val in (NAN, INF, -INF, 3e38, -3e38):
                xp = x.clone()
                xp[pos] = val
                flag = torch.zeros(1, dtype=torch.int32).cuda()
                maker(xp, flag)
                assert int(flag) == (0 if math.isfinite(val) else 1), (pos, val)


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_solver_reports_a_nan_that_scale_reject_used_to_clamp_away():
    """ScaleReject(clip=True) (the reference's configured default, conf/config.yaml:131) in front of the finiteness
    assert of bm/solver.py:258-260: a NaN MEG sample survives ``clamp_`` and the assert fires; a +inf sample clamps to
    ``limit``, is finite, and trains -- both like the reference."""
    from brainmagick_amd import synthetic
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    from brainmagick_amd.solver import Solver
    B, C, T, Fd, S = 6, 20, 60, 10, 3
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=32, merger_channels=16, initial_linear=16)
    torch.manual_seed(3)
    model = SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": 32}, n_subjects=S, **cfg)
    sr = ScaleReject(DeviceBatchScaler(torch.zeros(1, C), torch.ones(1, C)), limit=20, clip=True)
    solver = Solver(model, scale_reject=sr, check_finite=True)
    good = synthetic.make_batch(B, C, T, Fd, S, seed=1)
    assert torch.isfinite(solver.train_step(good))
    for at in ((0, 0, 0), (2, 7, 33), (B - 1, C - 1, T - 1)):
        bad = synthetic.make_batch(B, C, T, Fd, S, seed=2)
        bad.meg[at] = NAN
        with pytest.raises(AssertionError, match="non-finite values"):
            solver.train_step(bad)
            solver.check_pending_flags()
        inf = synthetic.make_batch(B, C, T, Fd, S, seed=2)
        inf.meg[at] = INF
        assert torch.isfinite(solver.train_step(inf))
        solver.check_pending_flags()


# ---- extreme but finite ------------------------------------------------------------------------------------------------
def test_extreme_finite_inputs_stay_finite_and_right(H):
    # LSTM with saturated gates: expf(-x) overflows to inf inside lstm_sigmoid for x < -88, 1 / (1 + inf) = 0
    Hd, B, T, dirs, whh, gx, dy, dcn = _lstm_setup(gain=30.0)
    assert float(torch.cat(gx).min()) < -89
    y64, dg64 = _lstm_reference(whh, gx, dy, dcn)
    y, dg = _lstm_run(H, whh, gx, dy, dcn)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dg).all())
    assert rel_l2(y, y64) < FWD_TOL and rel_l2(dg, dg64) < GRAD_TOL, (rel_l2(y, y64), rel_l2(dg, dg64))
    # clip_ce with scores of magnitude 1e4
    g = _gen(50)
    Bn, Bc = 5, 70
    part = torch.randn(2, Bn, Bc, generator=g) * 1e4
    inv = torch.ones(Bc)
    s64 = part.double().sum(0)
    scores, probs, dscaled, loss = H.clip_ce(part.cuda(), inv.cuda(), True, True, True)
    for t in (scores, probs, dscaled, loss):
        assert bool(torch.isfinite(t).all())
    assert rel_l2(scores, s64) < FWD_TOL
    s32 = scores.double().cpu()               # the softmax of scores this large amplifies their fp32 rounding: from the kernel's
    assert rel_l2(probs, torch.softmax(s32, 1)) < 1e-5
    ref_loss = F.cross_entropy(s32, torch.arange(Bn))
    assert abs(float(loss) - float(ref_loss)) < 1e-5 * float(ref_loss)
    # row_softmax with a spread of 200
    x = torch.linspace(-100, 100, 7 * 67).view(7, 67)[:, torch.randperm(67, generator=g)].contiguous()
    w = H.row_softmax(x.cuda())
    assert bool(torch.isfinite(w).all()) and rel_l2(w, torch.softmax(x.double(), 1)) < FWD_TOL
