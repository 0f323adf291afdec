"""The small row / column / flat kernels of csrc/clip.hip, scale.hip, merger.hip, adam.hip and norm_act.hip, each called
through its ``hip_ops`` wrapper and held to the same operation written in plain torch on the CPU in float64, at the
smallest shapes that reach every branch: one element, less than a wavefront, one more than a wavefront, a second
workgroup, a grid-stride loop that strides, the scalar path behind a misaligned pointer, empty segments.

Tolerances are tests/test_kernels_gpu.py's (rel-L2 5e-6 forward, 2e-5 gradients).  Every case prints the kernel's error
next to that of the same expression evaluated in fp32 on the CPU (both against fp64), and demands that the fp32 CPU
error stays below a quarter of the tolerance: an input on which plain fp32 is already marginal says nothing about the
kernel and has to be replaced, not tolerated."""
import pytest
import torch

from helpers import rel_l2
from oracle import bm_oracle as O
from test_kernels_gpu import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _held(what, got, ref64, ref32, tol):
    """rel-L2 of the kernel and of the fp32 CPU expression against fp64, printed; both asserted (see the module text)."""
    e, e32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    print(f"{what}: kernel {e:.2e}   fp32 CPU {e32:.2e}   (tolerance {tol:.0e})")
    assert e32 < tol / 4, f"{what}: the input is marginal for plain fp32 ({e32:.2e}): change the input"
    assert tuple(got.shape) == tuple(ref64.shape), (what, got.shape, ref64.shape)
    assert e < tol, (what, e)


# ---- row_softmax -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,gain", [(1, 1, 1.0), (3, 63, 1.0), (5, 64, 1.0), (6, 65, 1.0), (7, 300, 1.0),
                                            (7, 300, 40.0)])      # x 40: a spread above 88, expf underflows to 0
def test_row_softmax(H, rows, cols, gain):
    x = torch.randn(rows, cols, generator=_gen(rows * 1000 + cols)) * gain
    if gain > 1:
        assert float(x.max() - x.min()) > 88
    y = H.row_softmax(x.cuda())
    _held(f"row_softmax {rows}x{cols} gain {gain}", y, torch.softmax(x.double(), 1), torch.softmax(x, 1), FWD_TOL)
    assert float((y.double().sum(1) - 1).abs().max()) < 1e-5
    assert bool((y >= 0).all())


# ---- rowwise_dot -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(1, 1), (5, 255), (3, 257), (4, 43_200)])
@pytest.mark.parametrize("scaled", [False, True])
def test_rowwise_dot(H, rows, K, scaled):
    g = _gen(rows + K)
    a = torch.randn(rows, K, generator=g)
    b = 0.5 * a + 0.3 * torch.randn(rows, K, generator=g)          # <a, b> ~ K / 2: not cancellation-dominated
    scale = torch.rand(rows, generator=g) + 0.5 if scaled else None
    ref64 = (a.double() * b.double()).sum(1) * (scale.double() if scaled else 1.0)
    ref32 = (a * b).sum(1) * (scale if scaled else 1.0)
    got = H.rowwise_dot(a.cuda(), b.cuda(), scale.cuda() if scaled else None)
    _held(f"rowwise_dot {rows}x{K} scale={scaled}", got, ref64, ref32, FWD_TOL)
    assert torch.equal(got, H.rowwise_dot(a.cuda(), b.cuda(), scale.cuda() if scaled else None))      # deterministic


# ---- segment_sum_cols --------------------------------------------------------------------------------------------------
def _segments(V, cols, g):
    """seg [V + 1]: random cut points of [0, cols]; from V = 4 on with an empty segment at the front, in the middle and at
    the back."""
    cuts = sorted(torch.randint(0, cols + 1, (V - 1,), generator=g).tolist())
    seg = [0] + cuts + [cols]
    if V >= 4:
        seg[1] = 0
        seg[V - 1] = cols
        seg[V // 2 + 1] = seg[V // 2]
        empty = [v for v in range(V) if seg[v] == seg[v + 1]]
        assert 0 in empty and V - 1 in empty and V // 2 in empty
    assert all(a <= b for a, b in zip(seg, seg[1:]))
    return torch.tensor(seg, dtype=torch.int32)


@pytest.mark.parametrize("V", [1, 64, 65, 130])
def test_segment_sum_cols(H, V):
    cols = 70
    for rows in (1, 5, 9):
        g = _gen(V * 10 + rows)
        p = torch.rand(rows, cols, generator=g)
        order = torch.randperm(cols, generator=g).to(torch.int32)
        seg = _segments(V, cols, g)
        gathered = p[:, order.long()]
        ref64 = torch.stack([gathered[:, seg[v]:seg[v + 1]].double().sum(1) for v in range(V)], 1)
        ref32 = torch.stack([gathered[:, seg[v]:seg[v + 1]].sum(1) for v in range(V)], 1)
        got = H.segment_sum_cols(p.cuda(), order.cuda(), seg.cuda())
        _held(f"segment_sum_cols {rows}x{cols} V={V}", got, ref64, ref32, FWD_TOL)
        empty = (seg[1:] == seg[:-1])
        assert float(got[:, empty.cuda()].abs().sum()) == 0.0           # an empty segment sums to exactly 0


# ---- row_axpy_sub ------------------------------------------------------------------------------------------------------
def _axpy_case(rows, K, misaligned, seed):
    g = _gen(seed)
    y = torch.randn(rows, K, generator=g)
    x = torch.randn(rows, K, generator=g)
    coef = torch.randn(rows, generator=g)
    return y, x, coef


def _device_rows(t, misaligned):
    """``t`` on the GPU; ``misaligned``: as the view buf[1:] of a flat buffer, 4 bytes past a 16-byte boundary."""
    if not misaligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("rows,K,misaligned", [
    (3, 1, False), (3, 7, False), (2, 1023, False),      # K % 4 != 0: the scalar path
    (3, 1024, False),                                    # the vector path
    (3, 1024, True),                                     # K % 4 == 0 behind a misaligned pointer: the scalar path again
    (2, 4 * 256 * 256 + 4, False),                       # 65 537 vectors per row on 65 536 threads: the loop strides once
])
def test_row_axpy_sub(H, rows, K, misaligned):
    y, x, coef = _axpy_case(rows, K, misaligned, rows * 7 + K)
    yg = _device_rows(y, misaligned)
    out = H.row_axpy_sub(yg, x.cuda(), coef.cuda())
    assert out.data_ptr() == yg.data_ptr()
    ref64 = y.double() - coef.double()[:, None] * x.double()
    ref32 = y - coef[:, None] * x
    _held(f"row_axpy_sub {rows}x{K} misaligned={misaligned}", out, ref64, ref32, FWD_TOL)
    # Element by element.  hipcc contracts `y - c * x` to one FMA (-ffp-contract=fast is its default for device code:
    # the product is not rounded), torch on the CPU rounds the product and then the difference.  The two differ by the
    # rounding of the product, at most half an ulp of |c x|, and each is within half an ulp of its own result of what it
    # rounds: together one ulp of the result plus half an ulp of the product.
    ulp = (2.0 ** -24 * (2 * ref64.abs() + (coef[:, None] * x).abs().double()) * (1 + 1e-6)).float()
    assert bool(((out.cpu() - ref32).abs() <= ulp).all()), ((out.cpu() - ref32).abs() / ulp).max()
    # and against the exact value: half an ulp of the result (one rounding), whichever way the kernel was compiled,
    # plus the product's half ulp if it was not contracted
    bound = 2.0 ** -24 * (ref64.abs().float() + (coef[:, None] * x).abs()) * (1 + 1e-6)
    assert bool(((out.cpu().double() - ref64).abs() <= bound.double()).all())


# ---- clip_cand_coef ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Bc", [(1, 1), (5, 257), (40, 600)])           # 257, 600: a second and a third workgroup
@pytest.mark.parametrize("with_alpha", [False, True])
def test_clip_cand_coef(H, B, Bc, with_alpha):
    """coef_o = alpha * (sum_b dscaled[b, o] * scores[b, o]) / |cand_o| with |cand_o| = 1 / inv_norm_o - 1e-8 and coef_o = 0
    for |cand_o| <= 0 (csrc/clip.hip); a masked candidate (score -inf, gradient 0) contributes nothing."""
    g = _gen(B * 31 + Bc)
    scores = torch.randn(B, Bc, generator=g)
    dscaled = torch.randn(B, Bc, generator=g) * 0.01
    norms = torch.rand(Bc, generator=g) + 0.5
    masked, zero = ([3, Bc - 2], Bc // 2) if Bc > 1 else ([], None)
    for o in masked:
        scores[:, o] = float("-inf")
        dscaled[:, o] = 0.0
    if zero is not None:
        norms[zero] = 0.0                     # an all-zero candidate: its scores are 0, inv_norm = 1 / 1e-8
        scores[:, zero] = 0.0
    inv = 1.0 / (1e-8 + norms)
    alpha = torch.tensor(1.7) if with_alpha else None

    def formula(d, s, iv, a):
        r = torch.where(d != 0, d * s, torch.zeros_like(d)).sum(0)
        norm = 1.0 / iv - 1e-8
        return torch.where(norm > 0, a * r / norm, torch.zeros_like(r))
    ref64 = formula(dscaled.double(), scores.double(), inv.double(), 1.7 if with_alpha else 1.0)
    ref32 = formula(dscaled, scores, inv, 1.7 if with_alpha else 1.0)
    got = H.clip_cand_coef(dscaled.cuda(), scores.cuda(), inv.cuda(), alpha.cuda() if with_alpha else None)
    live = torch.ones(Bc, dtype=torch.bool)
    if zero is not None:
        live[zero] = False      # |cand| = 1 / 1e8 - 1e-8 is round-off around 0 in fp32 AND fp64: the value there is 0 / it
        assert float(got[zero]) == 0.0
    for o in masked:
        assert float(got[o]) == 0.0
    _held(f"clip_cand_coef {B}x{Bc} alpha={with_alpha}", got.cpu()[live], ref64[live], ref32[live], GRAD_TOL)


# ---- clip_ce_cols ------------------------------------------------------------------------------------------------------
def _ce_cols_reference(scores, inv, dscaled, loss, off, w_row, w_col):
    """(loss_col, dscaled', loss') in the dtype of ``scores``: the column log-softmax written out."""
    B, Bc = scores.shape
    cols = scores[:, off:off + B]                                     # column j belongs to target candidate off + j
    lse = torch.logsumexp(cols, 0)
    loss_col = lse - torch.diagonal(cols)
    d = dscaled * w_row
    pr = torch.softmax(cols, 0) - torch.eye(B, dtype=scores.dtype)
    d[:, off:off + B] = d[:, off:off + B] + (w_col / B) * inv[off:off + B][None, :] * pr
    return loss_col, d, w_row * loss + w_col * loss_col.mean()


@pytest.mark.parametrize("B,Bc,off", [(1, 1, 0), (5, 12, 0), (5, 12, 7), (65, 130, 64), (70, 70, 0)])
@pytest.mark.parametrize("w_row,w_col", [(0.5, 0.5), (0.3, 0.7)])
def test_clip_ce_cols(H, B, Bc, off, w_row, w_col):
    g = _gen(B * 17 + Bc + off)
    scores = torch.randn(B, Bc, generator=g) * 3
    inv = 1.0 / (torch.rand(Bc, generator=g) + 0.5)
    dscaled = torch.randn(B, Bc, generator=g) * 0.01
    loss = torch.tensor(1.234)
    what = f"clip_ce_cols B={B} Bc={Bc} off={off} w=({w_row}, {w_col})"
    lc64, d64, l64 = _ce_cols_reference(scores.double(), inv.double(), dscaled.double(), loss.double(), off, w_row, w_col)
    lc32, d32, l32 = _ce_cols_reference(scores, inv, dscaled.clone(), loss, off, w_row, w_col)
    sg, ig = scores.cuda(), inv.cuda()
    dg, lg = dscaled.cuda(), loss.cuda()
    loss_col = H.clip_ce_cols(sg, ig, dg, lg, off, w_row, w_col)
    _held(what + " loss_col", loss_col, lc64, lc32, FWD_TOL)
    _held(what + " dscaled", dg, d64, d32, GRAD_TOL)
    print(f"{what} loss: kernel {abs(float(lg) - float(l64)):.2e}   fp32 CPU {abs(float(l32) - float(l64)):.2e}")
    assert abs(float(lg) - float(l64)) < FWD_TOL * max(1.0, abs(float(l64)))
    # a candidate that is a negative only keeps w_row x its row term: one fp32 multiply, exactly
    neg = torch.ones(Bc, dtype=torch.bool)
    neg[off:off + B] = False
    assert torch.equal(dg.cpu()[:, neg], (dscaled * torch.tensor(w_row, dtype=torch.float32))[:, neg])
    # deterministic, and the optional outputs
    dg2, lg2 = dscaled.cuda(), loss.cuda()
    assert torch.equal(H.clip_ce_cols(sg, ig, dg2, lg2, off, w_row, w_col), loss_col)
    assert torch.equal(dg2, dg) and torch.equal(lg2, lg)
    lg3 = loss.cuda()
    assert torch.equal(H.clip_ce_cols(sg, ig, None, lg3, off, w_row, w_col), loss_col)         # dscaled=None: loss only
    assert torch.equal(lg3, lg)
    dg4 = dscaled.cuda()
    assert torch.equal(H.clip_ce_cols(sg, ig, dg4, None, off, w_row, w_col), loss_col)         # loss=None
    assert torch.equal(dg4, dg)


# ---- time_sums_t, sum_over_batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (3, 5, 63), (2, 3, 65), (7, 9, 360)])
def test_time_sums_t(H, B, C, T):
    x = torch.randn(B, C, T, generator=_gen(B + C + T)) + 0.3
    got = H.time_sums_t(x.cuda())
    _held(f"time_sums_t {B}x{C}x{T}", got, x.double().sum(2).t(), x.sum(2).t(), FWD_TOL)
    assert torch.equal(got, H.time_sums_t(x.cuda()))                       # deterministic


@pytest.mark.parametrize("n", [1, 255, 100_003])
def test_sum_over_batch(H, n):
    for B in (1, 2, 7):
        x = torch.randn(B, n, generator=_gen(B + n)) + 0.3
        _held(f"sum_over_batch {B}x{n}", H.sum_over_batch(x.cuda()), x.double().sum(0), x.sum(0), FWD_TOL)


# ---- flag_unless_all_set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 512 * 256 + 3])              # the last: 512 workgroups, the loop strides
def test_flag_unless_all_set(H, n):
    flag = torch.tensor([6, 0, 0], dtype=torch.int32).cuda()
    H.flag_unless_all_set(torch.ones(n, dtype=torch.bool).cuda(), flag)
    assert flag.tolist() == [6, 0, 0]                                     # all true: the word is untouched
    for at in sorted({0, n // 2 + (1 if n > 2 else 0), n - 1}):
        if at >= n:
            continue
        mask = torch.ones(n, dtype=torch.bool)
        mask[at] = False
        flag = torch.tensor([6, 0, 0], dtype=torch.int32).cuda()
        H.flag_unless_all_set(mask.cuda(), flag)
        assert flag.tolist() == [7, 0, 0], (n, at, flag.tolist())         # bit 0 goes up, bits 1 and 2 stay


# ---- center_scale ------------------------------------------------------------------------------------------------------
def _center_scale_reference(x, center, scale, group, clip, limit):
    """bm/norm.py:86-87 + :333 in the reference's fp32 op order: sub, then div, then clamp."""
    g = group if group is not None else torch.zeros(len(x), dtype=torch.int64)
    out = (x - center[g][:, :, None]) / scale[g][:, :, None]
    return out.clamp(-limit, limit) if clip else out


@pytest.mark.parametrize("B,C,T,misaligned", [(1, 1, 1, False), (3, 5, 7, False), (4, 30, 360, False), (2, 3, 8, True),
                                              (2, 184, 360, False)])      # 16 560 vectors on 64 x 256 threads: strides
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_center_scale(H, B, C, T, misaligned, grouped, clip):
    g = _gen(B * 100 + C + T + grouped)
    R, limit = (3, 2.5) if grouped else (1, 2.5)
    x = torch.randn(B, C, T, generator=g) * 2 + 0.5
    center = torch.randn(R, C, generator=g) * 0.3
    scale = torch.rand(R, C, generator=g) + 0.5
    group = torch.randint(0, R, (B,), generator=g) if grouped else None
    ref = _center_scale_reference(x, center, scale, group, clip, limit)
    assert B * C * T < 8 or bool((ref.abs() == limit).any()) == clip          # the clamp does something
    args = (center.cuda(), scale.cuda(), group.cuda() if grouped else None)
    xg = _device_rows(x, misaligned)
    out, maxabs = H.center_scale(xg, *args, clip=clip, limit=limit, want_maxabs=True)
    assert torch.equal(out.cpu(), ref), (out.cpu() - ref).abs().max()
    assert torch.equal(maxabs.cpu(), ref.abs().amax((1, 2)))
    out2, none = H.center_scale(xg, *args, clip=clip, limit=limit)
    assert none is None and torch.equal(out2, out)
    inplace, maxabs2 = H.center_scale(xg, *args, clip=clip, limit=limit, want_maxabs=True, inplace=True)
    assert inplace.data_ptr() == xg.data_ptr() and torch.equal(xg, out) and torch.equal(maxabs2, maxabs)


# ---- masked_softmax, softmax_bwd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 65, 273])
def test_masked_softmax_and_its_backward(H, C):
    """Scores + the oracle's mask rule (bm_oracle.is_invalid, the ban disc of bm/models/common.py:342-346) -> softmax over
    the sensors; U * O = 15 rows, no multiple of the 4 rows of a workgroup."""
    g = _gen(C)
    U, Oc, radius = 3, 5, 0.2
    pos = torch.rand(U, C, 2, generator=g)
    pos[1, C // 3:C // 2] = O.INVALID
    pos[2, :C - 1] = O.INVALID                       # layout 2: the only sensor left is the last one
    pos[2, C - 1] = torch.tensor([0.9, 0.9])
    ban = torch.tensor([0.4, 0.6])
    scores = torch.randn(U, Oc, C, generator=g) * 2
    for banned in (False, True):
        mask = O.is_invalid(pos)
        if banned:
            mask = mask | ((pos - ban).norm(dim=-1) <= radius)
            assert bool(mask[0].any()) and not bool(mask[2, C - 1])
        off = torch.zeros(U, C).masked_fill(mask, float("-inf"))
        ref64 = torch.softmax(scores.double() + off.double()[:, None], 2)
        ref32 = torch.softmax(scores + off[:, None], 2)
        w = H.masked_softmax(scores.cuda(), pos.cuda(), ban.cuda() if banned else None, radius if banned else 0.0)
        _held(f"masked_softmax C={C} ban={banned}", w, ref64, ref32, FWD_TOL)
        assert float(w.cpu()[mask[:, None].expand_as(w)].abs().sum()) == 0.0
        last = torch.zeros(C)
        last[C - 1] = 1.0
        assert torch.equal(w[2].cpu(), last.expand(Oc, C))
    sc = scores.double().requires_grad_(True)
    sm = torch.softmax(sc + off.double()[:, None], 2)
    dw = torch.randn(U, Oc, C, generator=g)
    sm.backward(dw.double())
    w32 = sm.detach().float()
    ref32 = w32 * (dw - (w32 * dw).sum(2, keepdim=True))
    ds = H.softmax_bwd(w32.cuda(), dw.cuda())
    # (layout 2's rows are w = one-hot: their gradient is exactly 0 in the reference and w * (dw - dw) = 0 here)
    _held(f"softmax_bwd C={C}", ds, sc.grad, ref32, GRAD_TOL)
    assert float(ds[2].abs().sum()) == 0.0


# ---- adam_step ---------------------------------------------------------------------------------------------------------
def test_adam_step_strided_with_grad_scale(H):
    """n = 4096 * 256 + 5: the grid-stride loop strides; grad_scale = 0.25; three steps from non-zero moments, against
    torch.optim.Adam in fp64 fed grad * grad_scale.  Each step moves an element by about lr, so the parameters are held
    to 1e-3 * lr * steps (the update itself to a part in a thousand) plus one fp32 rounding of the parameter."""
    n, lr, betas, eps, gs, steps = 4096 * 256 + 5, 3e-4, (0.9, 0.999), 1e-8, 0.25, 3
    g = _gen(9)
    p = torch.randn(n, generator=g) * 0.1         # (small |p|: three fp32 roundings of p stay far below the step bound)
    m = torch.randn(n, generator=g) * 0.05
    v = torch.rand(n, generator=g) * 0.01 + 1e-4
    p64 = torch.nn.Parameter(p.double())
    p32 = torch.nn.Parameter(p.clone())
    opts = []
    for q in (p64, p32):
        opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps)
        opt.state[q] = dict(step=torch.tensor(0.0), exp_avg=m.to(q.dtype).clone(), exp_avg_sq=v.to(q.dtype).clone())
        opts.append(opt)
    pg, mg, vg = p.cuda(), m.cuda(), v.cuda()
    for step in range(1, steps + 1):
        grad = torch.randn(n, generator=g) * 0.4
        for q, opt in zip((p64, p32), opts):
            q.grad = (grad * gs).to(q.dtype)
            opt.step()
        H.adam_step(pg, grad.cuda(), mg, vg, step, lr, *betas, eps, grad_scale=gs)
    ref, ref32 = p64.detach(), p32.detach()
    bound = 1e-3 * lr * steps + 2.0 ** -23 * float(ref.abs().max())
    err, err32 = float((pg.double().cpu() - ref).abs().max()), float((ref32.double() - ref).abs().max())
    print(f"adam_step n={n}: max|p - p64| kernel {err:.2e}   fp32 CPU {err32:.2e}   (bound {bound:.2e})")
    assert err32 < bound / 4 and err <= bound
    assert float((pg.double().cpu() - p.double()).abs().max()) > 0.5 * lr          # it did step
    st64, st32 = opts[0].state[p64], opts[1].state[p32]
    _held("adam_step exp_avg", mg, st64["exp_avg"], st32["exp_avg"], 1e-6)
    _held("adam_step exp_avg_sq", vg, st64["exp_avg_sq"], st32["exp_avg_sq"], 1e-6)


# ---- guard bands, once per kernel at an off-tile shape -------------------------------------------------------------------
def test_row_kernels_stay_inside_their_buffers(H):
    """Every output of the kernels above inside a canary-bordered, NaN-poisoned allocation (tests/test_guard_bands_gpu.py's
    arena; the kernels that write in place get their operand from it), and equal to what the plain call returns.
    (affine_act_res, act_bn_bwd, glu_fwd / glu_bwd have their own: test_streaming_kernels_stay_inside_their_buffers.)"""
    from test_guard_bands_gpu import Arena, _no_nan
    g = _gen(77)
    rows, cols, K, V, B, Bc, C, T = 7, 67, 1023, 65, 5, 259, 5, 63
    x = torch.randn(rows, cols, generator=g).cuda()
    a, b = torch.randn(rows, K, generator=g).cuda(), torch.randn(rows, K, generator=g).cuda()
    coef = torch.randn(rows, generator=g).cuda()
    order, seg = torch.randperm(cols, generator=g).to(torch.int32).cuda(), _segments(V, cols, g).cuda()
    scores, dscaled = torch.randn(B, Bc, generator=g).cuda(), (torch.randn(B, Bc, generator=g) * 0.01).cuda()
    inv = (1.0 / (torch.rand(Bc, generator=g) + 0.5)).cuda()
    x3 = (torch.randn(B, C, T, generator=g) * 2).cuda()
    center, scale = torch.randn(1, C, generator=g).cuda(), (torch.rand(1, C, generator=g) + 0.5).cuda()
    pos = torch.rand(3, cols, 2, generator=g).cuda()
    sc3 = torch.randn(3, 5, cols, generator=g).cuda()
    mask = torch.ones(1027, dtype=torch.bool)
    mask[1026] = False
    n = 4099
    p, gr = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    m, v = torch.zeros(n).cuda(), torch.zeros(n).cuda()

    def served(t):
        out = torch.empty_like(t)          # (from the arena while it is active)
        out.copy_(t)
        return out

    def run():
        w = H.masked_softmax(sc3, pos, None, 0.0)
        res = dict(row_softmax=H.row_softmax(x), rowwise_dot=H.rowwise_dot(a, b, coef),
                   segment_sum_cols=H.segment_sum_cols(x, order, seg),
                   row_axpy_sub=H.row_axpy_sub(served(a), b, coef),
                   clip_cand_coef=H.clip_cand_coef(dscaled, scores, inv),
                   time_sums_t=H.time_sums_t(x3), sum_over_batch=H.sum_over_batch(x3),
                   masked_softmax=w, softmax_bwd=H.softmax_bwd(w, sc3))
        d, loss = served(dscaled), served(torch.full((), 0.5, device="cuda"))
        res["clip_ce_cols loss_col"] = H.clip_ce_cols(scores, inv, d, loss, 3)
        res["clip_ce_cols dscaled"], res["clip_ce_cols loss"] = d, loss
        res["center_scale"], res["center_scale maxabs"] = H.center_scale(x3, center, scale, clip=True, limit=2.0,
                                                                         want_maxabs=True)
        res["center_scale inplace"], _ = H.center_scale(served(x3), center, scale, inplace=True)
        flag = served(torch.tensor([6, 0, 0], dtype=torch.int32).cuda())
        H.flag_unless_all_set(mask.cuda(), flag)
        res["flag_unless_all_set"] = flag
        pp, mm, vv = served(p), served(m), served(v)
        H.adam_step(pp, gr, mm, vv, 1, 3e-4, 0.9, 0.999, 1e-8, grad_scale=0.5)
        res["adam p"], res["adam m"], res["adam v"] = pp, mm, vv
        return res

    arena = Arena()
    with arena.active():
        guarded = run()
    arena.check("row kernels")
    plain = run()
    assert guarded["flag_unless_all_set"].tolist() == [7, 0, 0]
    for name, t in guarded.items():
        _no_nan(t, name)
        assert torch.equal(t, plain[name]), name
