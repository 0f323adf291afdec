"""Every kernel that chooses between 16-byte and 4-byte accesses, behind operands that are only 4-byte aligned.

The C ABI (include/bm_hip.h) asks for 4-byte alignment of its fp32 pointers and nothing more: FlatAdam packs parameters
and gradients without padding, so every parameter behind one with numel % 4 != 0 starts 4, 8 or 12 bytes past a 16-byte
boundary, ``grad_destination`` hands the weight-gradient kernels such a view to store into, and a batch slice or a
``narrow`` gives the same for activations.  Here T % 4 == 0 (K % 4 == 0) throughout, so the 16-byte path is eligible by
shape and the BASE ALONE decides.  ``helpers.shifted(t, k)`` is ``t`` as the view ``buf[k:k + n]`` of a flat buffer;
``helpers.ShiftedOut`` an output view of that kind between canary floats, NaN-poisoned (a vector store one element past a
gradient view lands in the neighbouring parameter's gradient: the canaries see it).

Reference: the operation restated in torch on the CPU in float64, with the tolerances the kernels already have
(tests/test_kernels_gpu.py: rel-L2 5e-6 forward, 2e-5 gradients; 1e-5 for the BatchNorm partial sums) through
``_held`` of tests/test_row_kernels_gpu.py, which prints the error of the same expression in fp32 on the CPU next to the
kernel's.  On top of that, bits:
  * an elementwise output whose per-element formula does not depend on the path equals the aligned run's bit for bit;
  * all runs on the same side of the decision agree bit for bit, sums included (one kernel, one order);
  * per-channel sums across the decision walk the slab in another order: fp64 only;
  * the contractions stage differently and multiply alike: bit-identical to the aligned run.

What decides the 16-byte path of each C entry point, and the test on either side of the decision
(v = vector side, s = scalar side; "shape" alone means that no pointer takes part):

  entry point                 16-byte path taken when                              v / s
  --------------------------  ---------------------------------------------------  -----------------------------------
  bm_affine_act_res           T % 4, y | res | out                                 test_affine_act_res: aligned / each
                                                                                   pointer shifted
  bm_act_bn_bwd (one pass)    shape (fused_covers), dout | y | dy                  test_act_bn_bwd[fused=1]: aligned /
                                                                                   shifted (-> two passes, scalar)
  bm_act_bn_bwd (two passes)  T % 4, dout | y | dy                                 test_act_bn_bwd[fused=0]
  bm_channel_sum              T % 4, bstride % 4, x                                test_channel_sum_and_stats
  bm_channel_stats            T % 4, x                                             test_channel_sum_and_stats
  bm_glu_fwd                  T % 4, u | out                                       test_glu
  bm_glu_bwd                  T % 4, dout | u | du                                 test_glu
  bm_clip_inv_norms           K % 4, cand                                          test_clip_inv_norms_entry_points
  bm_clip_cand_prep           K % 4, cand                                          test_clip_inv_norms_entry_points
  bm_gemm_nt                  T % 4, strides % 4, a | x                            test_gemm_nt_narrow[f32]
  bm_gemm_nt_x3               shape only (dwordx4 buffer loads at any dword)       test_gemm_nt_narrow[f32x3, f16x2]:
                                                                                   the loads on / off their alignment
  bm_reduce_splits            per % 4, part                                        test_reduce_splits (part aligned /
                                                                                   shifted), test_gemm_nt_narrow
                                                                                   (nsplit = 2, out shifted)
  bm_gemm_nt_h2 / _h2_rows    shape only (T % 4, strides: RS / FL variants)        test_gemm_nt_wide, rows in {0, 1}
  bm_gemm_nt_h2_grouped       shape only                                           test_gemm_nt_wide_grouped
  bm_conv1d_nn                T % 4, x_bstride % 4, x (tiles below 5 blocks)       test_conv_nn[f32]
  bm_conv1d_nn_x3 / _h2       shape only (dword loads of x)                        test_conv_nn[f32x3, f16x2]
  bm_conv1d_strided,          shape only (dword loads of x, dword stores)          test_conv_strided_family
  bm_conv1d_transposed,
  bm_conv1d_strided_wgrad

For the "shape only" rows the two sides are the same kernel with its loads on and off their natural alignment; both are
run and must agree bit for bit.  The rows already tested behind ``buf[1:]`` elsewhere (encode, lowpass, scaler_fit,
regress, scale, segments, row_axpy_sub, amax) are not repeated here."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import ShiftedOut, rel_l2, shifted
from test_autograd_states_gpu import MODES, _launches, mode       # noqa: F401  (``mode``: the compute-mode fixture)
from test_kernels_gpu import FWD_TOL, GRAD_TOL
from test_row_kernels_gpu import _held

pytestmark = pytest.mark.gpu

STATS_TOL = 1e-5                # the BatchNorm partial sums (tests/test_kernels_gpu.py)
SHIFTS = (1, 2, 3)
NORM_SHAPES = [(3, 5, 8),       # one split, two vectors per row
               (9, 6, 40)]      # bm_bwd_nsplit = 4: ragged slabs of 2 and 3 segments


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the sweep ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _outputs_shifted(k, served):
    """While active, every fp32 GPU tensor that a ``hip_ops`` wrapper allocates with ``torch.empty`` /
    ``torch.empty_like`` -- the kernels' outputs -- is a ``ShiftedOut`` view ``4 * k`` bytes off alignment (appended to
    ``served``).  Other dtypes (the double workspaces) keep the allocator's alignment.  k = 0: nothing is patched."""
    if k == 0:
        yield
        return
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def serve(shape):
        so = ShiftedOut(shape, k)
        served.append(so)
        return so.view

    def empty(*shape, dtype=None, device=None, **kw):
        dims = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        if device is None or torch.device(device).type != "cuda" or dtype not in (None, torch.float32) or kw \
                or math.prod(dims) == 0:
            return real_empty(*shape, dtype=dtype, device=device, **kw)
        return serve(dims)

    def empty_like(t, **kw):
        if not t.is_cuda or t.dtype != torch.float32 or kw or t.numel() == 0:
            return real_empty_like(t, **kw)
        return serve(tuple(t.shape))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def _sweep(names):
    """(label, {input: shift}, shift of the outputs): the aligned run, then for k = 1, 2, 3 each input on its own, the
    outputs on their own, and everything together."""
    yield "aligned", {}, 0
    for k in SHIFTS:
        for n in names:
            yield f"{n}+{k}", {n: k}, 0
        yield f"outputs+{k}", {}, k
        yield f"all+{k}", {n: k for n in names}, k


def _runs(inputs, call, out_decides):
    """``call(dev)`` -> tuple of result tensors, over the sweep of ``inputs`` (name -> fp32 CPU tensor).  Returns
    [(label, on the scalar side?, results)]; shifted outputs are checked for stray stores and skipped elements."""
    runs = []
    for label, shifts, kout in _sweep(list(inputs)):
        dev = {n: shifted(t, shifts.get(n, 0)) for n, t in inputs.items()}
        served = []
        with _outputs_shifted(kout, served):
            res = call(dev)
        torch.cuda.synchronize()
        assert bool(served) == (kout > 0), label
        for so in served:
            so.check(label)
        runs.append((label, bool(shifts) or (out_decides and kout > 0), res))
    return runs


def _same_side_same_bits(what, runs):
    """All runs on one side of the decision are one kernel walking in one order: every result bit-identical."""
    for side in (False, True):
        group = [(label, res) for label, scalar, res in runs if scalar == side]
        assert group, (what, side)
        for label, res in group[1:]:
            for i, (a, b) in enumerate(zip(res, group[0][1])):
                assert (a is None and b is None) or torch.equal(a, b), \
                    f"{what}: result {i} of {label} differs in bits from {group[0][0]} (same path)"


def _equal_to_aligned(what, runs, i):
    base = runs[0][2][i]
    for label, _, res in runs[1:]:
        assert torch.equal(res[i], base), f"{what}: result {i} of {label} differs in bits from the aligned run"


def _published_maximum(H, t, what, rows=False):
    """The maximum that the producer published for ``t`` (f16x2 mode: no separate scan) is that of what it wrote."""
    slot = H._noted(t, "_bm_amax")
    assert slot is not None, f"{what}: no maximum was published"
    assert float(slot.max()) == float(t.abs().max()), what
    if rows:
        r = H.row_amax_of(t)
        assert r is not None and torch.equal(r.cpu(), t.abs().amax((0, 2)).cpu()), what


# ---- norm_act.hip ------------------------------------------------------------------------------------------------------
_NORM = {}


def _norm_inputs(B, C, T):
    """Inputs of the streaming kernels at one shape and the BatchNorm vectors (fp32, what the kernels get), built once."""
    if (B, C, T) not in _NORM:
        g = _gen(B * 100 + C * 10 + T)
        d = dict(y=torch.randn(B, C, T, generator=g) * 1.5 + 0.3, dout=torch.randn(B, C, T, generator=g),
                 res=torch.randn(B, C, T, generator=g), u=torch.randn(B, 2 * C, T, generator=g) * 1.5)
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        yd = d["y"].double()
        mean = yd.mean((0, 2))
        invstd = 1.0 / torch.sqrt(yd.var((0, 2), unbiased=False) + 1e-5)
        scale = gamma.double() * invstd
        d.update(mean=mean.float(), invstd=invstd.float(), scale=scale.float(),
                 shift=(beta.double() - mean * scale).float())
        _NORM[(B, C, T)] = d
    return _NORM[(B, C, T)]


def _bc(v):
    return v[None, :, None]


def _gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("B,C,T", NORM_SHAPES)
@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("with_res", [False, True])
def test_affine_act_res(H, B, C, T, act, with_res):
    """out = act(y * scale[c] + shift[c]) [+ res]: elementwise, so every run equals the aligned one bit for bit."""
    assert H.get_compute_dtype() == "f16x2" and T % 4 == 0
    d = _norm_inputs(B, C, T)
    code = H.ACT_GELU if act == "gelu" else H.ACT_NONE
    inputs = {"y": d["y"], **({"res": d["res"]} if with_res else {})}
    scale, shift = d["scale"].cuda(), d["shift"].cuda()

    def ref(dt):
        z = d["y"].to(dt) * _bc(d["scale"].to(dt)) + _bc(d["shift"].to(dt))
        z = F.gelu(z) if act == "gelu" else z
        return z + d["res"].to(dt) if with_res else z
    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    what = f"affine_act_res {(B, C, T)} {act} res={with_res}"
    runs = _runs(inputs, lambda t: (H.affine_act_res(t["y"], scale, shift, t.get("res"), code),), out_decides=True)
    for label, _, (out,) in runs:
        _held(f"{what} {label}", out, ref64, ref32, FWD_TOL)
        _published_maximum(H, out, f"{what} {label}")
    _equal_to_aligned(what, runs, 0)
    _same_side_same_bits(what, runs)


@pytest.mark.parametrize("B,C,T", NORM_SHAPES)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("fused", [1, 0], ids=["fused=1", "fused=0"])
def test_act_bn_bwd(H, B, C, T, train, fused):
    """Backward of GELU(BatchNorm(y)) with affine gradients and dbias.  ``fused=1``: the aligned run takes the one-pass
    kernel, every shifted one the two scalar passes; ``fused=0``: the two passes, 16-byte and scalar.

    dy bit for bit against the aligned run only in eval mode under ``fused=0``: there dy = scale * dz per element, from
    one template.  In train mode dy subtracts the channel's means of dz and dz * xhat, which the scalar walk sums in
    another order, and the one-pass kernel writes dz with an explicit fmaf: those are held to fp64, like the sums."""
    assert H.get_compute_dtype() == "f16x2" and T % 4 == 0
    L = H.lib()
    d = _norm_inputs(B, C, T)
    bn = [d[k].cuda() for k in ("scale", "shift", "mean", "invstd")]

    def ref(dt):
        y, dout = d["y"].to(dt), d["dout"].to(dt)
        sc, sh, mu, inv = (_bc(d[k].to(dt)) for k in ("scale", "shift", "mean", "invstd"))
        dz = dout * _gelu_grad(y * sc + sh)
        xh = (y - mu) * inv
        n = B * T
        dy = sc * (dz - dz.sum((0, 2), keepdim=True) / n - xh * (dz * xh).sum((0, 2), keepdim=True) / n) if train \
            else sc * dz
        return dy, (dz * xh).sum((0, 2)), dz.sum((0, 2)), dy.sum((0, 2))
    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    what = f"act_bn_bwd {(B, C, T)} {'train' if train else 'eval'} fused={fused}"

    def call(t):
        res = H.act_bn_bwd(t["dout"], t["y"], *bn, train, H.ACT_GELU, want_affine_grads=True, want_dbias=True)
        _published_maximum(H, res[0], what, rows=True)
        return res

    prev = L.bm_act_bn_bwd_set_fused(fused)
    try:
        if fused:
            assert L.bm_act_bn_bwd_fused_covers(B, C, T) == 1
        runs = _runs({"dout": d["dout"], "y": d["y"]}, call, out_decides=True)
    finally:
        L.bm_act_bn_bwd_set_fused(prev)
    for label, _, (dy, dgamma, dbeta, dbias) in runs:
        _held(f"{what} {label} dy", dy, ref64[0], ref32[0], GRAD_TOL)
        _held(f"{what} {label} dgamma", dgamma, ref64[1], ref32[1], GRAD_TOL)
        _held(f"{what} {label} dbeta", dbeta, ref64[2], ref32[2], GRAD_TOL)
        if train:       # sum(dy) of a BatchNorm input is analytically 0: the bound of tests/test_kernels_gpu.py
            assert float(dbias.abs().max()) < 1e-2 * max(1.0, float(dy.abs().max())), (what, label)
        else:
            _held(f"{what} {label} dbias", dbias, ref64[3], ref32[3], GRAD_TOL)
    if not train and not fused:
        _equal_to_aligned(what, runs, 0)
    _same_side_same_bits(what, runs)


@pytest.mark.parametrize("B,C,T", NORM_SHAPES)
def test_channel_sum_and_stats(H, B, C, T):
    """Per-channel sum, and (sum, sum of squares) partials: only ``x`` is read as vectors, so a shifted output stays on
    the 16-byte side.  The two sides sum in different orders: fp64 across them, bits within them."""
    assert T % 4 == 0
    d = _norm_inputs(B, C, T)
    x = d["y"]
    runs = _runs({"x": x}, lambda t: (H.channel_sum(t["x"]), H.channel_stats(t["x"])), out_decides=False)
    assert sum(1 for _, scalar, _ in runs if not scalar) == 1 + len(SHIFTS)
    for label, _, (s, stats) in runs:
        what = f"channel {(B, C, T)} {label}"
        _held(f"{what} sum", s, x.double().sum((0, 2)), x.sum((0, 2)), GRAD_TOL)
        assert stats.shape == (H.lib().bm_channel_stats_splits(B), C, 2)
        folded = stats.double().sum(0)
        _held(f"{what} stats sum", folded[:, 0], x.double().sum((0, 2)), x.sum((0, 2)), STATS_TOL)
        _held(f"{what} stats sumsq", folded[:, 1], (x.double() ** 2).sum((0, 2)), (x * x).sum((0, 2)), STATS_TOL)
    _same_side_same_bits(f"channel {(B, C, T)}", runs)


@pytest.mark.parametrize("B,C,T", NORM_SHAPES)
def test_glu(H, B, C, T):
    """GLU forward and backward: out and du are elementwise (bit-identical to the aligned run), dbias is a sum."""
    assert H.get_compute_dtype() == "f16x2" and T % 4 == 0
    d = _norm_inputs(B, C, T)
    u, dout = d["u"], d["dout"]

    def ref(dt):
        a, gate = u.to(dt)[:, :C], torch.sigmoid(u.to(dt)[:, C:])
        du = torch.cat([dout.to(dt) * gate, dout.to(dt) * a * gate * (1 - gate)], 1)
        return a * gate, du, du.sum((0, 2))
    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    what = f"glu {(B, C, T)}"
    fwd = _runs({"u": u}, lambda t: (H.glu_fwd(t["u"]),), out_decides=True)
    for label, _, (out,) in fwd:
        _held(f"{what} fwd {label}", out, ref64[0], ref32[0], FWD_TOL)
        _published_maximum(H, out, f"{what} fwd {label}")
    _equal_to_aligned(what + " fwd", fwd, 0)
    _same_side_same_bits(what + " fwd", fwd)

    def call(t):
        du, dbias = H.glu_bwd(t["dout"], t["u"])
        _published_maximum(H, du, what + " bwd", rows=True)
        return du, dbias
    bwd = _runs({"dout": dout, "u": u}, call, out_decides=True)
    for label, _, (du, dbias) in bwd:
        _held(f"{what} bwd {label} du", du, ref64[1], ref32[1], GRAD_TOL)
        _held(f"{what} bwd {label} dbias", dbias, ref64[2], ref32[2], GRAD_TOL)
    _equal_to_aligned(what + " bwd", bwd, 0)
    _same_side_same_bits(what + " bwd", bwd)


# ---- clip.hip ----------------------------------------------------------------------------------------------------------
def _clip_rows(K, planted):
    """Five candidate rows.  ``planted`` (K = 1 024): 4096 in the first 256 places and 1 elsewhere.  On the scalar path a
    thread adds the squares of the places i, i + 256, i + 512, i + 768 in fp32: 2^24 + 1 + 1 + 1 = 2^24 (each 1 is half an
    ulp, ties to even), 2^32 for the row.  On the 16-byte path it holds one vector, four accumulators of one square
    each, added in double: 2^32 + 768.  The square roots are 65536 and 65536 + 2^-7 in fp32: the inverse norms differ by
    two ulps, both 9e-8 from the exact value or closer."""
    if not planted:
        return torch.randn(5, K, generator=_gen(K))
    cand = torch.ones(5, K)
    cand[:, :256] = 4096.0
    return cand


@pytest.mark.parametrize("K,planted", [(8, False),          # two vectors per row on 256 threads
                                       (1024, False),       # one vector per thread
                                       (1024, True),        # ... and an input on which the two orders round apart
                                       (43_200, False)])    # a production candidate (120 features x 360 samples)
def test_clip_inv_norms_entry_points(H, K, planted):
    """bm_clip_cand_prep (behind ``H.clip_inv_norms``) promises the inverse norms of bm_clip_inv_norms bit for bit.
    Both sum four interleaved fp32 accumulators per thread on the 16-byte path and one on the scalar path: they agree
    only when they choose alike -- at any base.  (On random rows of this length the two orders round to the same fp32
    value nearly always: the planted rows tell them apart, see ``_clip_rows``.)"""
    Bc = 5
    cand = _clip_rows(K, planted)
    ref64 = 1.0 / (1e-8 + cand.double().square().sum(1).sqrt())
    ref32 = 1.0 / (1e-8 + cand.square().sum(1).sqrt())
    for k in (0,) + SHIFTS:
        c = shifted(cand, k)
        prep = H.clip_inv_norms(c)
        plain = torch.empty(Bc, device="cuda")
        H.check(H.lib().bm_clip_inv_norms(H._p(c), Bc, K, H._p(plain), H._stream()), "bm_clip_inv_norms")
        _held(f"clip_cand_prep K={K} planted={planted} base+{4 * k}", prep, ref64, ref32, FWD_TOL)
        _held(f"clip_inv_norms K={K} planted={planted} base+{4 * k}", plain, ref64, ref32, FWD_TOL)
        assert torch.equal(prep, plain), \
            (f"K={K}, cand {4 * k} bytes past a 16-byte boundary: bm_clip_cand_prep and bm_clip_inv_norms sum in "
             f"different orders (largest difference {float(((prep - plain) / plain).abs().max()):.3e} of the value)")


# ---- gemm_nt: the narrow kernels ------------------------------------------------------------------------------------------
def _nt_ref(a, x, KS, dil):
    halo = KS // 2 * dil
    xpad = F.pad(x.double(), (halo, halo))
    T = a.shape[2]
    return torch.stack([torch.einsum("smt,sct->mc", a.double(), xpad[..., j * dil:j * dil + T]) for j in range(KS)], -1)


def _operand_sweep():
    """(label, shift of a, shift of x): a, then x, then both, for k = 1, 2, 3."""
    for k in SHIFTS:
        yield f"a+{k}", k, 0
        yield f"x+{k}", 0, k
        yield f"both+{k}", k, k


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("KS", [1, 3])
def test_gemm_nt_narrow(H, mode, KS):
    """S = 5, M = 24, Cn = 20, T = 48.  "f32": dwordx4 staging behind aligned operands, dword staging otherwise; the
    3 x bf16 kernels ("f32x3", and "f16x2" at this shape) issue the same buffer loads on or off their alignment.  The
    staging differs, the MFMA order does not: bit-identical.  Then into a shifted, canary-bordered ``out``: by the
    kernel's own epilogue (nsplit = 1) and by bm_reduce_splits (nsplit = 2; per % 4 == 0)."""
    S, M, Cn, T, dil = 5, 24, 20, 48, 1
    g = _gen(700 + KS)
    a, x = torch.randn(S, M, T, generator=g), torch.randn(S, Cn, T, generator=g)
    assert (M * Cn * KS) % 4 == 0
    base = {ns: H.gemm_nt(a.cuda(), x.cuda(), S, M, Cn, T, KS, dil, nsplit=ns) for ns in (None, 1, 2)}
    ref = _nt_ref(a, x, KS, dil)
    for ns, out in base.items():
        err = rel_l2(out[0], ref)
        print(f"gemm_nt {mode} KS={KS} nsplit={ns}: rel-L2 {err:.3e}")
        assert out.shape == (1, M, Cn, KS) and err < GRAD_TOL
    for label, ka, kx in _operand_sweep():
        ag, xg = shifted(a, ka), shifted(x, kx)
        assert torch.equal(H.gemm_nt(ag, xg, S, M, Cn, T, KS, dil), base[None]), (mode, KS, label)
        for ns in (1, 2):
            for kout in (0,) + SHIFTS:
                dst = ShiftedOut((1, M, Cn, KS), kout)
                got = H.gemm_nt(ag, xg, S, M, Cn, T, KS, dil, out=dst.view, nsplit=ns)
                torch.cuda.synchronize()
                assert got.data_ptr() == dst.view.data_ptr()
                dst.check(f"gemm_nt {mode} KS={KS} {label} nsplit={ns} out+{kout}")
                assert torch.equal(got, base[ns]), (mode, KS, label, ns, kout)


@pytest.mark.parametrize("nsplit", [2, 3, 9])      # 9: one trip of the eight-splits-in-flight loop and a remainder
def test_reduce_splits(H, nsplit):
    """bm_reduce_splits directly: ``part`` aligned (four elements per thread, one dwordx4 per split) and shifted (one
    element per thread), ``out`` shifted inside canaries.  Both add the splits in the order k = 0, 1, ...: equal in bits
    to that sum written out in fp32."""
    M, Cn, KS = 24, 20, 3
    per = M * Cn * KS
    assert per % 4 == 0
    part = torch.randn(nsplit, M, Cn, KS, generator=_gen(nsplit))
    want = part[0].clone()
    for k in range(1, nsplit):
        want += part[k]
    for kp in (0,) + SHIFTS:
        for kout in (0,) + SHIFTS:
            dst = ShiftedOut((M, Cn, KS), kout)
            H.check(H.lib().bm_reduce_splits(H._p(shifted(part, kp)), H._p(dst.view), 1, nsplit, M, Cn, KS, per, Cn * KS,
                                             KS, 1, H._stream()), "bm_reduce_splits")
            torch.cuda.synchronize()
            dst.check(f"reduce_splits nsplit={nsplit} part+{kp} out+{kout}")
            assert torch.equal(dst.view.cpu(), want), (nsplit, kp, kout)


# ---- gemm_nt: the wide f16x2 tiles -------------------------------------------------------------------------------------
_WIDE = {}


def _wide_operands(T, KS, planted):
    """(a, x, fp64 result) at S = 8, M = Cn = 256, built once.  ``planted``: the largest magnitude of each operand sits
    in its last four floats -- a tail that a range check dropped would change the whole last row / column."""
    key = (T, KS, planted)
    if key not in _WIDE:
        g = _gen(T * 10 + KS)
        a, x = torch.randn(8, 256, T, generator=g), torch.randn(8, 256, T, generator=g)
        if planted:
            a.view(-1)[-1], x.view(-1)[-2] = 37.0, -41.0          # they meet in out[255][255][2], worth 37 * 41 alone
            assert float(a.abs().max()) == 37.0 and float(x.abs().max()) == 41.0
        _WIDE[key] = (a, x, _nt_ref(a, x, KS, 1))
    return _WIDE[key]


def _wide_call(H, a, x, T, KS, rows):
    """The weight-gradient contraction on ``a`` / ``x``; ``rows``: with the per-channel maxima of ``a`` noted on it as
    act_bn_bwd / glu_bwd publish them (the row-scaled kernels; at T = 132 and three taps, the flat time axis)."""
    if rows:
        H._note(a, "_bm_row_amax", a.abs().amax((0, 2)))
    out, labels = _launches(H, lambda: H.gemm_nt(a, x, 8, 256, 256, T, KS, 1))
    assert labels and all(n.startswith("gemm_nt_h2w") for n in labels), labels
    return out


@pytest.mark.parametrize("T", [192, 132])
@pytest.mark.parametrize("KS", [1, 3])
@pytest.mark.parametrize("rows", [False, True], ids=["tensor-scale", "row-scales"])
def test_gemm_nt_wide(H, T, KS, rows):
    """gemm_nt_h2w selects its variant from T % 4 and the strides, and issues dwordx4 buffer loads from the operand
    base: behind a shifted base every one of them is off its natural alignment, and a row's last piece ends at the
    descriptor's last byte."""
    assert H.get_compute_dtype() == "f16x2" and T % 4 == 0
    assert H.lib().bm_gemm_nt_h2_covers(256, 256, KS, 8, T, 1, 1, 0)
    a, x, ref = _wide_operands(T, KS, False)
    base = _wide_call(H, a.cuda(), x.cuda(), T, KS, rows)
    err = rel_l2(base[0], ref)
    print(f"gemm_nt wide T={T} KS={KS} rows={rows}: rel-L2 {err:.3e}")
    assert base.shape == (1, 256, 256, KS) and err < GRAD_TOL
    for label, ka, kx in _operand_sweep():
        got = _wide_call(H, shifted(a, ka), shifted(x, kx), T, KS, rows)
        assert torch.equal(got, base), (T, KS, rows, label, rel_l2(got[0], ref))


@pytest.mark.parametrize("T", [192, 132])
def test_gemm_nt_wide_keeps_the_tail_of_a_shifted_operand(H, T):
    assert H.get_compute_dtype() == "f16x2"
    a, x, ref = _wide_operands(T, 3, True)
    for rows in (False, True):
        base = _wide_call(H, a.cuda(), x.cuda(), T, 3, rows)
        assert rel_l2(base[0], ref) < GRAD_TOL       # (a lost 37 * 41 is 0.09 of the result's norm)
        for k in SHIFTS:
            got = _wide_call(H, shifted(a, k), shifted(x, k), T, 3, rows)
            assert torch.equal(got, base), (T, rows, k, rel_l2(got[0], ref))


def test_gemm_nt_wide_grouped(H):
    """The grouped call of tests/test_f16x2_gpu.py::test_grouped_weight_gradient_on_the_wide_kernels at its smallest
    shape that the wide tiles cover: three groups through order / seg, the last one empty."""
    assert H.get_compute_dtype() == "f16x2"
    M, Cn, T, B, G = 320, 192, 192, 64, 3
    assert H.lib().bm_gemm_nt_h2_covers(M, Cn, 1, B, T, G, 1, 1)
    g = _gen(M + Cn + G)
    a, x = torch.randn(B, M, T, generator=g), torch.randn(B, Cn, T, generator=g)
    idx = torch.randint(0, G - 1, (B,), generator=g)
    ref = torch.zeros(G, M, Cn, dtype=torch.float64)
    ref.index_add_(0, idx, torch.bmm(a.double(), x.double().transpose(1, 2)))
    order, seg = H.group_by_index(idx.cuda(), G)

    def call(ag, xg):
        out, labels = _launches(H, lambda: H.gemm_nt(ag, xg, B, M, Cn, T, 1, 1, order=order, seg=seg, G=G))
        assert labels and all("_h2w" in n for n in labels), labels
        return out.view(G, M, Cn)
    base = call(a.cuda(), x.cuda())
    assert rel_l2(base, ref) < GRAD_TOL and float(base[G - 1].abs().max()) == 0.0
    for label, ka, kx in _operand_sweep():
        assert torch.equal(call(shifted(a, ka), shifted(x, kx)), base), label


# ---- convolutions ------------------------------------------------------------------------------------------------------
def _conv_operands(B, Cin, M, T, KS, seed):
    g = _gen(seed)
    return (torch.randn(B, Cin, T, generator=g), torch.randn(M, Cin, KS, generator=g) / math.sqrt(Cin * KS),
            torch.randn(M, generator=g))


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("B,Cin,M,T,KS,dil", [(5, 20, 24, 48, 1, 1), (5, 20, 24, 48, 3, 1), (5, 20, 24, 48, 3, 4),
                                              (8, 256, 256, 132, 3, 1)])
def test_conv_nn(H, mode, B, Cin, M, T, KS, dil):
    """"Same"-padded conv with ``x`` shifted, and its output written into a shifted, canary-bordered ``out``.  "f32"
    stages x with dwordx4 loads behind an aligned base and dwords otherwise; the other kernels load dwords."""
    x, w, b = _conv_operands(B, Cin, M, T, KS, 900 + M + KS + dil)
    ref = F.conv1d(x.double(), w.double(), b.double(), padding=KS // 2 * dil, dilation=dil)
    wp, bg = H.pack_conv_fwd(w.cuda(), (T, dil)), b.cuda()
    if mode == "f16x2" and M == 256:
        assert H.lib().bm_conv_h2_covers(M, Cin, T, KS, dil)
    base = H.conv_nn(x.cuda(), wp, M, KS, dil, bias=bg)[1]
    assert base.shape == ref.shape and rel_l2(base, ref) < FWD_TOL, rel_l2(base, ref)
    for k in SHIFTS:
        xg = shifted(x, k)
        assert torch.equal(H.conv_nn(xg, wp, M, KS, dil, bias=bg)[1], base), (mode, k)
        for kout, kx in ((k, 0), (k, k)):
            dst = ShiftedOut((B, M, T), kout)
            got = H.conv_nn(xg if kx else x.cuda(), wp, M, KS, dil, bias=bg, out=dst.view)[1]
            torch.cuda.synchronize()
            assert got.data_ptr() == dst.view.data_ptr()
            dst.check(f"conv_nn {mode} {(B, Cin, M, T, KS, dil)} x+{kx} out+{kout}")
            assert torch.equal(got, base), (mode, kx, kout)


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("KS,dil", [(1, 1), (3, 1), (3, 4)])
def test_conv_strided_family(H, mode, KS, dil):
    """nn.Conv1d(stride=2), nn.ConvTranspose1d(stride=2) and the strided weight gradient (one exact-fp32 family in every
    compute mode) at B = 5, 20 -> 24 channels, T = 48 with their inputs shifted; the weight gradient also into a shifted,
    canary-bordered ``out``, by its own stores (nsplit = 1) and through bm_reduce_splits (nsplit = 2)."""
    B, Cin, M, T, stride = 5, 20, 24, 48, 2
    pad = KS // 2 * dil
    x, w, b = _conv_operands(B, Cin, M, T, KS, 950 + KS + dil)
    g = _gen(960 + KS + dil)
    # strided
    Tout = H.conv_out_len(T, KS, stride, dil, pad, False)
    ref = F.conv1d(x.double(), w.double(), b.double(), stride=stride, padding=pad, dilation=dil)
    wp, bg = H.pack_strided_rows_first(w.cuda()), b.cuda()
    base = H.conv_strided(x.cuda(), wp, M, Tout, KS, stride, dil, pad, False, bias=bg)[1]
    assert base.shape == ref.shape and rel_l2(base, ref) < FWD_TOL
    # transposed: 24 -> 20 channels with the weight read as [Cin = 24, M = 20, KS]
    xt = torch.randn(B, M, T, generator=g)
    Tt = H.conv_out_len(T, KS, stride, dil, pad, True)
    ref_t = F.conv_transpose1d(xt.double(), w.double(), None, stride=stride, padding=pad, dilation=dil)
    wpt = H.pack_strided_rows_second(w.cuda())
    base_t = H.conv_strided(xt.cuda(), wpt, Cin, Tt, KS, stride, dil, pad, True)[1]
    assert base_t.shape == ref_t.shape and rel_l2(base_t, ref_t) < FWD_TOL
    # weight gradient of the strided layer
    dy = torch.randn(B, M, Tout, generator=g)
    wd = w.double().requires_grad_(True)
    F.conv1d(x.double(), wd, None, stride=stride, padding=pad, dilation=dil).backward(dy.double())
    base_w = {ns: H.conv_strided_wgrad(dy.cuda(), x.cuda(), KS, stride, dil, pad, nsplit=ns) for ns in (1, 2)}
    for ns in (1, 2):
        assert base_w[ns].shape == (M, Cin, KS) and rel_l2(base_w[ns], wd.grad) < GRAD_TOL
    for k in SHIFTS:
        assert torch.equal(H.conv_strided(shifted(x, k), wp, M, Tout, KS, stride, dil, pad, False, bias=bg)[1], base), k
        assert torch.equal(H.conv_strided(shifted(xt, k), wpt, Cin, Tt, KS, stride, dil, pad, True)[1], base_t), k
        for label, ka, kx in ((f"a+{k}", k, 0), (f"x+{k}", 0, k), (f"both+{k}", k, k)):
            for ns in (1, 2):
                dst = ShiftedOut((M, Cin, KS), k)
                got = H.conv_strided_wgrad(shifted(dy, ka), shifted(x, kx), KS, stride, dil, pad, out=dst.view, nsplit=ns)
                torch.cuda.synchronize()
                assert got.data_ptr() == dst.view.data_ptr()
                dst.check(f"conv_strided_wgrad {mode} KS={KS} dil={dil} {label} nsplit={ns}")
                assert torch.equal(got, base_w[ns]), (mode, label, ns)
