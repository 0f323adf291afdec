"""A value that hip_ops remembers about a tensor never outlives the contents it describes: the f16x2 maxima
(``_bm_amax`` / ``_bm_row_amax``), the candidate norms (``_bm_inv_norms``) and the packed parameters (``_PackPlan``).
All cases run in "f16x2" mode, where those values are consumed.

Writers: every hip_ops wrapper that lets a kernel store into a tensor it did not allocate (``_p(...)`` of a
caller-supplied tensor in a store position).  torch's version counter does not see such a store, so each of them calls
``_touched`` on the destination:

  conv_nn(out=)                       y_out of the conv epilogue (ClipLossFn.backward, LSTMFn.backward accumulate in it)
  conv_strided_wgrad(out=)            the weight gradient, directly or through bm_reduce_splits
  gemm_nt(out=) direct                nsplit == 1 and canonical strides: the contraction stores into ``out``
  gemm_nt(out=) reduce_splits         otherwise bm_reduce_splits folds the partial tiles into ``out``
  row_axpy_sub(y)                     y -= coef * x
  center_scale(inplace=True)          x itself
  center_scale_inverse(inplace=True)  x itself
  clip_ce_cols(dscaled, loss)         the row term's gradient and loss, updated to the weighted sums
  lstm_layer_bwd(dc)                  the carried cell gradient
  adam_step(param, exp_avg, ...)      the parameters and both moments; FlatAdam hands it slices of its flat buffers, the
                                      notes live on the Parameter objects: those follow the weights epoch instead
  (bn_finalize's running statistics, regress / feature-decoding flag words, regress_metric_update's and
   class_acc_update's accumulators are written too, but are never the operand of a contraction and carry no note;
   regress_loss_fwd's ``out`` is the target tensor and is only read.)

Packed parameters: a parameter edited through ``.data`` moves neither the version counter nor the weights epoch, so the
library cannot see it -- INTEGRATION.md ("Packed parameters and edits through .data") states the rule: call
``brainmagick_amd.weights_changed()`` afterwards.  ``test_packed_parameters_follow_every_visible_change`` pins the
visible routes and that rule."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu

FWD_TOL = 5e-6                 # tests/test_kernels_gpu.py
BIG = float(2 ** 20)
WB, WC, WT = 8, 256, 192       # the wide shape (helpers.WIDE_DIMS: T = 192, B = 8) at 256 channels


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def h2_mode(H):
    H.set_compute_dtype("f16x2")
    yield
    H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _labels(H, fn):
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        H.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def _consume(H, dst):
    """A wide f16x2 conv that reads ``dst`` ([B, 256, T], the very tensor object the writer was given) against fp64."""
    Bn, Cn, Tn = dst.shape
    assert H.lib().bm_conv_h2_covers(Cn, 256, Tn, 1, 1)
    w = torch.randn(256, Cn, 1, generator=_gen(3)) / math.sqrt(Cn)
    (_, y, _), labels = _labels(H, lambda: H.conv_nn(dst, H.pack_conv_fwd(w.cuda(), (Tn, 1)), 256, 1, 1))
    assert any(n.startswith("conv_nn_h2w") for n in labels), labels
    err = rel_l2(y, F.conv1d(dst.cpu().double(), w.double()))
    assert err <= FWD_TOL, err


def _wide(g, scale=1.0, shape=(WB, WC, WT)):
    return (torch.randn(*shape, generator=g) * scale).cuda()


# ---- the writers: (destination, run the writer with operands 2^20 larger, whether a contraction may consume it) ---------
def _w_conv_nn_out(H, g):
    dst = _wide(g)
    w = torch.randn(WC, WC, 1, generator=g) / 16
    x = _wide(g, BIG)
    return dst, lambda: H.conv_nn(x, H.pack_conv_fwd(w.cuda(), (WT, 1)), WC, 1, 1, out=dst), True


def _w_conv_nn_out_res(H, g):
    """the accumulating form of ClipLossFn.backward: ``res`` and ``out`` are the same tensor"""
    dst = _wide(g)
    w = torch.randn(WC, WC, 1, generator=g) / 16
    x = _wide(g, BIG)
    return dst, lambda: H.conv_nn(x, H.pack_conv_fwd(w.cuda(), (WT, 1)), WC, 1, 1, res=dst, out=dst), True


def _w_strided_wgrad(H, g, nsplit):
    S, R, Q, L, KS, stride, pad = 3, 24, 20, 48, 3, 2, 1
    U = (L + 2 * pad - (KS - 1) - 1) // stride + 1
    dst = torch.randn(R, Q, KS, generator=g).cuda()
    a, xl = (torch.randn(S, R, U, generator=g) * BIG).cuda(), torch.randn(S, Q, L, generator=g).cuda()
    return dst, lambda: H.conv_strided_wgrad(a, xl, KS, stride, 1, pad, out=dst, nsplit=nsplit), False


def _w_gemm_nt(H, g, nsplit):
    """out [1][256][192][1] handed over as a [1, 256, 192] tensor: nsplit 1 = the direct path, 2 = reduce_splits"""
    dst = _wide(g, shape=(1, WC, WT))
    a, x = _wide(g, BIG, (WB, WC, WT)), _wide(g, 1.0, (WB, WT, WT))
    return dst, lambda: H.gemm_nt(a, x, WB, WC, WT, WT, 1, 1, out=dst, nsplit=nsplit), True


def _w_gemm_nt_strided_out(H, g):
    """non-canonical output strides (the composed front end's augmented matrices): always through reduce_splits"""
    dst = _wide(g, shape=(1, WC, WT + 1))
    a, x = _wide(g, BIG, (WB, WC, WT)), _wide(g, 1.0, (WB, WT, WT))
    return dst, lambda: H.gemm_nt(a, x, WB, WC, WT, WT, 1, 1, out=dst, out_strides=(0, WT + 1, 1, 0), nsplit=1), True


def _w_row_axpy_sub(H, g):
    dst = _wide(g)
    x, coef = _wide(g, BIG), torch.randn(WB, generator=g).cuda()
    return dst, lambda: H.row_axpy_sub(dst, x, coef), True


def _w_center_scale(H, g):
    dst = _wide(g)
    center, scale = torch.randn(1, WC, generator=g).cuda(), torch.full((1, WC), 1 / BIG).cuda()
    return dst, lambda: H.center_scale(dst, center, scale, inplace=True), True


def _w_center_scale_inverse(H, g):
    dst = _wide(g)
    center, scale = torch.randn(1, WC, generator=g).cuda(), torch.full((1, WC), BIG).cuda()
    return dst, lambda: H.center_scale_inverse(dst, center, scale, inplace=True), True


def _clip_state(H, g):
    Bn, Bc = 6, 9
    part = torch.randn(2, Bn, Bc, generator=g).cuda()
    inv = (torch.rand(Bc, generator=g) + 0.5).cuda()
    scores, _, dscaled, loss = H.clip_ce(part, inv, want_grad=True, want_loss=True)
    return scores, inv, dscaled, loss


def _w_clip_ce_cols_dscaled(H, g):
    scores, inv, dscaled, loss = _clip_state(H, g)
    dscaled.mul_(1 / BIG)                  # the old contents are 2^20 times smaller than what the column term adds
    return dscaled, lambda: H.clip_ce_cols(scores, inv, dscaled, loss), False


def _w_clip_ce_cols_loss(H, g):
    scores, inv, dscaled, loss = _clip_state(H, g)
    loss.mul_(1 / BIG)
    return loss, lambda: H.clip_ce_cols(scores, inv, dscaled, loss), False


def _w_lstm_dc(H, g):
    Hd, Bn, Tn = 24, 5, 6
    whh = [(torch.randn(4 * Hd, Hd, generator=g) / 5).cuda()]
    _, gates, c = H.lstm_layer_fwd(whh, [torch.randn(Tn, 4 * Hd, Bn, generator=g).cuda()])
    dy = (torch.randn(Tn, Hd, Bn, generator=g) * BIG).cuda()
    dst = torch.randn(1, Hd, Bn, generator=g).cuda()
    return dst, lambda: H.lstm_layer_bwd(whh, dy, gates, c, dst), False


def _w_adam(H, g, which):
    n = 4096
    ts = [(torch.randn(n, generator=g) / BIG).cuda() for _ in range(4)]
    ts[3].abs_()                                               # exp_avg_sq
    ts[1].mul_(BIG * BIG)                                      # the gradient
    return ts[which], lambda: H.adam_step(*ts, 1, 1.0, 0.9, 0.999, 1e-8), False


WRITERS = {
    "conv_nn(out=)": _w_conv_nn_out,
    "conv_nn(res=out)": _w_conv_nn_out_res,
    "conv_strided_wgrad(out=) direct": lambda H, g: _w_strided_wgrad(H, g, 1),
    "conv_strided_wgrad(out=) reduce_splits": lambda H, g: _w_strided_wgrad(H, g, 2),
    "gemm_nt(out=) direct": lambda H, g: _w_gemm_nt(H, g, 1),
    "gemm_nt(out=) reduce_splits": lambda H, g: _w_gemm_nt(H, g, 2),
    "gemm_nt(out=, out_strides=)": _w_gemm_nt_strided_out,
    "row_axpy_sub": _w_row_axpy_sub,
    "center_scale(inplace)": _w_center_scale,
    "center_scale_inverse(inplace)": _w_center_scale_inverse,
    "clip_ce_cols dscaled": _w_clip_ce_cols_dscaled,
    "clip_ce_cols loss": _w_clip_ce_cols_loss,
    "lstm_layer_bwd dc": _w_lstm_dc,
    "adam_step param": lambda H, g: _w_adam(H, g, 0),
    "adam_step exp_avg": lambda H, g: _w_adam(H, g, 2),
    "adam_step exp_avg_sq": lambda H, g: _w_adam(H, g, 3),
}


@pytest.mark.parametrize("writer", list(WRITERS))
def test_a_library_write_drops_the_noted_maximum(H, writer):
    dst, run, consumable = WRITERS[writer](H, _gen(len(writer)))
    old = float(H.amax(dst).max())
    assert old == float(dst.abs().max()) and H._noted(dst, "_bm_amax") is not None
    version = dst._version
    run()
    assert dst._version == version, "the write went through torch after all: this case proves nothing"
    now = float(dst.abs().max())
    assert now > 1000 * old, (writer, old, now)
    assert float(H.amax(dst).max()) == now, (writer, float(H.amax(dst).max()), now)
    if consumable:
        _consume(H, dst)


def test_a_library_write_drops_the_row_maxima_and_the_candidate_norms(H):
    """``_touched`` takes all three notes: a gradient whose per-channel maxima were published, then overwritten in
    place, and candidates whose inverse norms were noted."""
    g = _gen(1)
    dst = _wide(g)
    H._note(dst, "_bm_row_amax", dst.abs().amax(dim=(0, 2)).contiguous())
    inv = H.clip_inv_norms(dst)
    assert H.row_amax_of(dst) is not None and H.clip_inv_norms(dst) is inv
    H.row_axpy_sub(dst, _wide(g, BIG), torch.randn(WB, generator=g).cuda())
    assert H.row_amax_of(dst) is None
    inv2 = H.clip_inv_norms(dst)
    want = 1 / (1e-8 + dst.double().flatten(1).norm(dim=1))
    assert inv2 is not inv and rel_l2(inv2, want) <= FWD_TOL


def test_flat_adam_step_drops_the_maximum_noted_on_a_parameter(H):
    """FlatAdam.step writes the flat buffer; the note lives on the Parameter object (a view of it), whose version
    counter and address do not move.  ChannelMergerFn / FusedFrontEndFn read ``heads`` as a gemm_nt operand, which in
    f16x2 mode notes its maximum on the parameter."""
    from brainmagick_amd.optim import FlatAdam
    p = torch.nn.Parameter((torch.randn(WB, WC, WT, generator=_gen(2)) / BIG).cuda())
    opt = FlatAdam([p], lr=1.0)
    old = float(H.amax(p).max())
    scans = H.amax_scans
    assert H.amax(p) is not None and H.amax_scans == scans          # noted
    p.grad.copy_(torch.randn(p.shape, generator=_gen(3)).cuda())
    version, ptr = p._version, p.data_ptr()
    opt.step()
    assert (p._version, p.data_ptr()) == (version, ptr)
    now = float(p.detach().abs().max())
    assert now > 1000 * old and float(H.amax(p).max()) == now


# ---- torch-side edits -------------------------------------------------------------------------------------------------
def test_torch_side_edits_force_a_rescan(H):
    g = _gen(5)
    x = torch.randn(3, 64, 200, generator=g).cuda()
    first = H.amax(x)
    scans = H.amax_scans
    assert H.amax(x) is first and H.amax_scans == scans
    x.mul_(2.0)                                     # in place on the tensor
    assert float(H.amax(x).max()) == float(x.abs().max()) and H.amax_scans == scans + 1
    x[1].add_(100.0)                                # in place on a view: the version counter is shared
    assert float(H.amax(x).max()) == float(x.abs().max()) and H.amax_scans == scans + 2
    assert H.amax(x) is not first and H.amax_scans == scans + 2
    # a second view object gets a note of its own, and an edit through one view invalidates the other's
    v1, v2 = x.view(-1), x.view(-1)
    a1 = H.amax(v1)
    a2 = H.amax(v2)
    assert a1 is not a2 and H.amax_scans == scans + 4 and H.amax(v2) is a2
    v1.mul_(0.5)
    assert float(H.amax(v2).max()) == float(x.abs().max()) and H.amax_scans == scans + 5


def test_share_amax_bounds_the_slice(H):
    g = _gen(6)
    src = torch.randn(12, 40, generator=g).cuda()
    src[9, 3] = 50.0
    view = H.share_amax(src, src[2:6])
    noted = H._noted(view, "_bm_amax")
    assert noted is not None and float(noted.max()) == 50.0 >= float(view.abs().max())
    scans = H.amax_scans
    assert H.amax(view) is noted and H.amax_scans == scans


# ---- packed parameters --------------------------------------------------------------------------------------------------
def test_packed_parameters_follow_every_visible_change(H):
    """One wide conv layer; after every change of the weights the output is held to fp64 with the NEW weights and
    exactly one re-pack launch is counted; none between two forwards without a change, none without a tape.  A bare
    ``w.data.mul_(2)`` is invisible to the library (neither the version counter nor the weights epoch moves): the rule
    in INTEGRATION.md is to call ``weights_changed()`` after it, which is what is pinned here."""
    from brainmagick_amd import functional as BF
    from brainmagick_amd.optim import FlatAdam
    import brainmagick_amd
    g = _gen(7)
    conv = torch.nn.Conv1d(WC, WC, 3, padding=1).cuda()
    w = conv.weight
    x = _wide(g)
    x64 = x.cpu().double()

    def forward():
        return BF.Conv1dFn.apply(x, conv.weight, conv.bias, 1, H.ACT_NONE, 0., False)

    def check(repacks, what):
        n = H.pack_launches
        y, labels = _labels(H, forward)
        assert any(k.startswith("conv_nn_h2w") for k in labels), labels
        assert H.pack_launches - n == repacks, (what, H.pack_launches - n)
        ref = F.conv1d(x64, conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double(), padding=1)
        assert rel_l2(y, ref) <= FWD_TOL, (what, rel_l2(y, ref))
        n = H.pack_launches
        y2 = forward()
        with torch.no_grad():
            y3 = forward()
        assert H.pack_launches == n and torch.equal(y2, y) and torch.equal(y3, y), what
        return y

    check(1, "first use")
    with torch.no_grad():
        w.mul_(2)
    check(1, "in-place under no_grad")
    sd = {k: torch.randn(v.shape, generator=g) / 30 for k, v in conv.state_dict().items()}
    conv.load_state_dict(sd)
    check(1, "load_state_dict")
    opt = torch.optim.Adam(conv.parameters(), lr=1e-2)
    forward().square().mean().backward()
    opt.step()
    check(1, "torch.optim.Adam.step")
    conv.zero_grad(set_to_none=True)
    flat = FlatAdam(conv.parameters(), lr=1e-2)          # re-seats every p.data in the flat buffer
    assert conv.weight is w
    check(1, "FlatAdam construction")
    flat.zero_grad()
    before = w.detach().clone()
    forward().square().mean().backward()
    flat.step()
    assert not torch.equal(w.detach(), before)
    check(1, "FlatAdam.step")
    w.data = (torch.randn(w.shape, generator=g) / 30).cuda()
    check(1, "w.data = other")
    w.data.mul_(2)
    brainmagick_amd.weights_changed()
    check(1, "w.data.mul_(2) + weights_changed()")
