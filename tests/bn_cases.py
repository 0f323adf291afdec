"""Shared by tests/test_bn_conditioning_cpu.py and tests/test_bn_conditioning_gpu.py: BatchNorm statistics of channels
whose mean dwarfs their spread.  CPU only: nothing here imports the GPU side.

The project takes the statistics in one pass: the conv epilogues and ``bm_channel_stats`` write fp32 partial sums
(sum y, sum y^2) per stats tile, ``bn_finalize_kernel`` folds them in fp64 and takes var = s2 / n - mean^2 (clamped at 0),
then rounds invstd, scale and shift = beta - (float)mean * scale to fp32.  The subtraction cancels when
r = |mean| / std is large.  What is held here:

  LADDER            the ratios r a test tensor carries, channel c gets +-LADDER[c % 8] (the sign flips every 8 channels)
  offset_bias       the conv bias that puts every channel of a conv output at its planned r (the conv adds the bias in
                    its epilogue before the sums are taken: the inputs stay ordinary randn)
  emulated_*        the ALGORITHM restated in torch on the CPU: the yardstick for the constant K of the law
                        |var_kernel - var64| <= K * 2^-24 * (mean^2 + var)
                    -- not the code under test
  chain_reference   F.batch_norm(train) -> activation -> + res and its autograd gradients, in fp64 and (the ``_held``
                    style of tests/test_row_kernels_gpu.py: what plain torch fp32 gives on the same input) in fp32
  chan_err          max|got - ref| / rms(ref) over a channel's (B, T) slab: a rel-L2 over the whole tensor would let the
                    well-conditioned channels hide the others
  bn_input_ratios   the largest |mean| / std that reaches a BatchNorm layer while a reference model runs"""
import contextlib
import math

import torch
from torch.nn import functional as F

LADDER = (0, 1, 3, 10, 30, 100, 300, 1000)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
U24, U23 = 2.0 ** -24, 2.0 ** -23
LAW_SLACK = 4          # a kernel may sum a tile in another order than the emulation: 4 x K_emu, no licence for longer sums

# stats-tile widths of the producers (csrc/conv_common.h: 128 columns; csrc/conv_h2_common.h: a wavefront's 96 columns;
# csrc/conv_strided.hip: 128 columns of one output phase; bm_channel_stats: a split's whole slab)
TILE_NARROW, TILE_WIDE, TILE_STRIDED = 128, 96, 128

# the shapes of the GPU file, the smallest with several stats tiles per channel and a ragged last one
NARROW = dict(B=3, Cin=20, M=24, T=200, dil=1)                       # KS in (1, 3)
WIDE = dict(B=2, Cin=48, M=120, KS=3, dil=4, T=777)                  # 5 column tiles, the last one 9 columns wide
STRIDED = dict(B=3, Cin=16, M=24, KS=4, stride=2, dil=1, pad=2, T=202)
STATS_SHAPES = ((9, 24, 40), (3, 24, 41))                            # four ragged splits (vector path); the scalar path
# ... and one shape per family with ~150 partials per channel: with a handful of partials an fp32 fold (or an fp32
# running sum across tiles) rounds a few times more and stays inside 4 x K_emu; with 144 it leaves the law by a factor
# 3 to 8 (tests/test_bn_conditioning_cpu.py shows it on the restatement)
NARROW_DEEP = dict(B=48, Cin=20, M=24, KS=3, T=360, dil=1)           # 3 tiles per segment, the last one 104 columns
WIDE_DEEP = dict(WIDE, B=16)
STATS_DEEP = (64, 24, 360)                                           # 16 splits


def gen(seed):
    return torch.Generator().manual_seed(seed)


def planned_ratios(C, ladder=LADDER):
    """r of channel c: +-ladder[c % len], the sign flipping every len(ladder) channels."""
    n = len(ladder)
    return torch.tensor([float(ladder[c % n]) * (1 if (c // n) % 2 == 0 else -1) for c in range(C)], dtype=torch.float64)


def moments64(y):
    """Two-pass fp64 (mean, biased variance) per channel of y [B, C, T]."""
    yd = y.double()
    mean = yd.mean((0, 2))
    var = ((yd - mean[None, :, None]) ** 2).mean((0, 2))
    return mean, var


def realised_ratios(y32):
    """mean / std per channel, in fp64, of the fp32 tensor the kernel sees."""
    mean, var = moments64(y32)
    return mean / torch.sqrt(var)


def offset_bias(ref_pre64, ladder=LADDER):
    """(bias fp32 [C], realised r [C]) for the fp64 conv output ``ref_pre64`` [B, C, T] computed with ZERO bias."""
    assert ref_pre64.dtype == torch.float64
    mean, var = moments64(ref_pre64)
    plan = planned_ratios(ref_pre64.shape[1], ladder)
    bias = (plan * torch.sqrt(var) - mean).float()
    seen = (ref_pre64 + bias.double()[None, :, None]).float()
    return bias, realised_ratios(seen)


def chan_err(got, ref):
    """[C]: max|got - ref| / rms(ref) over each channel's (B, T) slab."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rms = torch.sqrt((ref * ref).mean((0, 2)))
    return (got - ref).abs().amax((0, 2)) / rms


def chan_rel_l2(got, ref):
    """[C]: the rel-L2 error of each channel's (B, T) slab on its own."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return torch.sqrt(((got - ref) ** 2).sum((0, 2)) / (ref * ref).sum((0, 2)))


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------
def emulated_partials(y32, tile, phases=1, slabs=None):
    """[ntiles, C, 2] fp32 (sum, sum of squares): one partial per (segment, output phase, ``tile`` columns of that
    phase) -- or, with ``slabs`` = [(b0, nb), ...], one per slab of whole segments (bm_channel_stats' splits)."""
    assert y32.dtype == torch.float32
    B, C, T = y32.shape
    parts = []
    if slabs is not None:
        for b0, nb in slabs:
            sl = y32[b0:b0 + nb].transpose(0, 1).reshape(C, -1)
            parts.append(torch.stack([sl.sum(1), (sl * sl).sum(1)], 1))
        return torch.stack(parts)
    for b in range(B):
        for p in range(phases):
            cols = y32[b, :, p::phases]
            for n0 in range(0, cols.shape[1], tile):
                sl = cols[:, n0:n0 + tile].contiguous()
                parts.append(torch.stack([sl.sum(1), (sl * sl).sum(1)], 1))
    return torch.stack(parts)


def stats_slabs(B, nsplit):
    """The segments [b0, b0 + nb) of each split of bm_channel_stats (csrc/norm_act.hip, ``Slab``)."""
    return [(B * s // nsplit, B * (s + 1) // nsplit - B * s // nsplit) for s in range(nsplit)]


def fold32(partials, count):
    """What a kernel that adds the partials up in ONE fp32 running sum would get (tile-major partials)."""
    acc = torch.zeros_like(partials[0])
    for t in range(partials.shape[0]):
        acc = acc + partials[t]
    acc = acc.double()
    mean = acc[:, 0] / count
    return acc[:, 0], acc[:, 1], mean, acc[:, 1] / count - mean * mean


def fold64(partials, count, channel_major=False):
    """fp64 fold of fp32 partials ([ntiles, C, 2], or [C, ntiles, 2] channel-major) -> (sum, sumsq, mean, var unclamped)."""
    st = partials.detach().double().cpu()
    st = st.sum(1) if channel_major else st.sum(0)
    mean = st[:, 0] / count
    return st[:, 0], st[:, 1], mean, st[:, 1] / count - mean * mean


def emulated_finalize(partials, count, gamma, beta, eps=BN_EPS):
    """bn_finalize_kernel's arithmetic: fp64 fold and clamp, fp32 invstd / scale / shift."""
    _, _, mean, var = fold64(partials, count)
    var = var.clamp_min(0)
    invstd = (1.0 / torch.sqrt(var + eps)).float()
    scale = gamma.float() * invstd
    mean32 = mean.float()
    return dict(mean64=mean, var64=var, mean=mean32, invstd=invstd, scale=scale, shift=beta.float() - mean32 * scale)


def _act(z, act):
    return F.gelu(z) if act == "gelu" else z


def _act_grad(z, act):
    if act != "gelu":
        return torch.ones_like(z)
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def emulated_chain(y32, partials, gamma, beta, res, dout, act):
    """producer's partials -> finalize -> y * scale + shift -> act -> + res, and the training-mode backward, all in
    fp32 but the fold (and the backward's two sums, which the kernels also keep in fp64)."""
    B, C, T = y32.shape
    n = B * T
    fin = emulated_finalize(partials, n, gamma, beta)
    bc = lambda v: v[None, :, None]                     # noqa: E731
    z = y32 * bc(fin["scale"]) + bc(fin["shift"])
    out = _act(z, act)
    if res is not None:
        out = out + res
    dz = dout * _act_grad(z, act)
    xh = (y32 - bc(fin["mean"])) * bc(fin["invstd"])
    dgamma = (dz * xh).double().sum((0, 2)).float()
    dbeta = dz.double().sum((0, 2)).float()
    dy = bc(fin["scale"]) * (dz - bc(dbeta) / n - xh * bc(dgamma) / n)
    return dict(fin, out=out, dy=dy, dgamma=dgamma, dbeta=dbeta)


def law_K(var_got, y32):
    """[C]: |var_got - var64| / (2^-24 (mean^2 + var)) against the two-pass fp64 moments of ``y32``."""
    mean, var = moments64(y32.cpu())
    return (var_got.double().cpu() - var).abs() / (U24 * (mean * mean + var))


def var_bound(K_emu, y32):
    """[C]: the law's right-hand side with the slack: 4 K_emu 2^-24 (mean^2 + var)."""
    mean, var = moments64(y32.cpu())
    return LAW_SLACK * K_emu * U24 * (mean * mean + var)


def out_bound(K_emu, y32):
    """[C]: the law propagated to the chain's output, relative to the channel's rms:
    (1/2 dvar / var + 2^-23 (1 + |r|)) * 4."""
    mean, var = moments64(y32.cpu())
    return (0.5 * var_bound(K_emu, y32) / var + U23 * (1 + (mean / torch.sqrt(var)).abs())) * 4


# ---- the references -------------------------------------------------------------------------------------------------------
def chain_reference(y32, gamma, beta, res, dout, act, train=True, rm=None, rv=None, dtype=torch.float64, stats=None):
    """F.batch_norm -> activation -> + res and its autograd gradients in ``dtype`` on the CPU.  ``train=False``: eval-mode
    BatchNorm with the batch's own fp64 moments as running statistics (what ``act_bn_bwd(bn_train=False)`` is given in
    the tests), or with ``stats`` = (mean, var)."""
    to = lambda t: None if t is None else t.detach().cpu().to(dtype)          # noqa: E731
    y = to(y32).requires_grad_(True)
    g, b = to(gamma).requires_grad_(True), to(beta).requires_grad_(True)
    mean64, var64 = moments64(y32.cpu())
    n = y32.shape[0] * y32.shape[2]
    out = dict(mean=mean64, var=var64)
    if train:
        rm_, rv_ = (to(rm), to(rv)) if rm is not None else (None, None)
        z = F.batch_norm(y, rm_, rv_, g, b, training=True, momentum=BN_MOMENTUM, eps=BN_EPS)
        out.update(rm=rm_, rv=rv_)
    else:
        m, v = stats if stats is not None else (mean64, var64)
        z = F.batch_norm(y, m.to(dtype), v.to(dtype), g, b, training=False, eps=BN_EPS)
    o = _act(z, act)
    if res is not None:
        o = o + to(res)
    o.backward(to(dout))
    zd = z.detach()
    dz = to(dout) * _act_grad(zd, act)
    out.update(out=o.detach(), dy=y.grad, dgamma=g.grad, dbeta=b.grad, dz_norm=torch.sqrt((dz * dz).sum((0, 2))),
               unbiased=var64 * n / max(n - 1, 1))
    return out


def backward_given_stats(y32, dout, scale, shift, mean, invstd, act, train):
    """The backward's formula in fp64 on the forward's own fp32 (scale, shift, mean, invstd): what ``act_bn_bwd`` has
    to return for THOSE statistics, whatever their distance from the true ones."""
    d = lambda t: t.detach().double().cpu()                                   # noqa: E731
    bc = lambda v: d(v)[None, :, None]                                        # noqa: E731
    y, n = d(y32), y32.shape[0] * y32.shape[2]
    z = y * bc(scale) + bc(shift)
    dz = d(dout) * _act_grad(z, act)
    xh = (y - bc(mean)) * bc(invstd)
    dgamma, dbeta = (dz * xh).sum((0, 2)), dz.sum((0, 2))
    dy = bc(scale) * dz
    if train:
        dy = bc(scale) * (dz - dbeta[None, :, None] / n - xh * dgamma[None, :, None] / n)
    return dict(dy=dy, dgamma=dgamma, dbeta=dbeta)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def conv_case(kind, seed=0, ladder=LADDER, **dims):
    """Inputs of a producer case: x [B, Cin, T] randn, the weight (nn.Conv1d's [M, Cin, KS]; nn.ConvTranspose1d's
    [Cin, M, KS] for kind "transposed"), the offset bias, the fp64 conv output WITH that bias and the realised ratios.
    kind: "same" (stride 1, padding KS // 2 * dil), "strided", "transposed"."""
    g = gen(seed)
    B, Cin, M, KS, T = dims["B"], dims["Cin"], dims["M"], dims["KS"], dims["T"]
    dil = dims.get("dil", 1)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn((Cin, M, KS) if kind == "transposed" else (M, Cin, KS), generator=g) / math.sqrt(Cin * KS)
    if kind == "same":
        pre0 = F.conv1d(x.double(), w.double(), None, padding=KS // 2 * dil, dilation=dil)
    elif kind == "strided":
        pre0 = F.conv1d(x.double(), w.double(), None, stride=dims["stride"], padding=dims["pad"], dilation=dil)
    else:
        pre0 = F.conv_transpose1d(x.double(), w.double(), None, stride=dims["stride"], padding=dims["pad"], dilation=dil)
    bias, ratios = offset_bias(pre0, ladder)
    return dict(x=x, w=w, bias=bias, pre64=pre0 + bias.double()[None, :, None], ratios=ratios,
                plan=planned_ratios(M, ladder))


def ladder_tensor(B, C, T, seed=0, ladder=LADDER):
    """[B, C, T] fp32 with unit spread and the planned ratios, for the producers that read a tensor (bm_channel_stats)."""
    y = torch.randn(B, C, T, generator=gen(seed), dtype=torch.float64)
    mean, var = moments64(y)
    y = (y - mean[None, :, None]) / torch.sqrt(var)[None, :, None] + planned_ratios(C, ladder)[None, :, None]
    return y.float()


def chain_operands(C, shape, seed):
    """gamma, beta (away from 0), residual, cotangent, running statistics."""
    g = gen(seed + 77)
    return dict(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.rand(C, generator=g) + 0.5,
                res=torch.randn(shape, generator=g), dout=torch.randn(shape, generator=g),
                rm=torch.randn(C, generator=g) * 0.3, rv=torch.rand(C, generator=g) + 0.5)


def by_ladder(values, plan, ladder=LADDER):
    """{|r|: max of ``values`` over the channels planned at +-r}."""
    return {r: float(values[plan.abs() == r].max()) for r in ladder if bool((plan.abs() == r).any())}


def fmt_ladder(d):
    return "  ".join(f"r={r:g}: {v:.1e}" for r, v in d.items())


# ---- what training reaches ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def bn_input_ratios():
    """While active, every F.batch_norm call (nn.BatchNorm1d's included) records max_c |mean| / std of its input over
    (B, T), in fp64.  Yields the list of those maxima, one per call."""
    seen = []
    real = F.batch_norm

    def probe(x, *a, **kw):
        if x.dim() == 3 and x.shape[0] * x.shape[2] > 1:
            mean, var = moments64(x.detach())
            ok = var > 0
            if bool(ok.any()):
                seen.append(float((mean[ok].abs() / torch.sqrt(var[ok])).max()))
        return real(x, *a, **kw)
    F.batch_norm = probe
    try:
        yield seen
    finally:
        F.batch_norm = real


@contextlib.contextmanager
def bn_inputs():
    """While active, every F.batch_norm call appends its (detached) input to the list this yields."""
    seen = []
    real = F.batch_norm

    def probe(x, *a, **kw):
        seen.append(x.detach().clone())
        return real(x, *a, **kw)
    F.batch_norm = probe
    try:
        yield seen
    finally:
        F.batch_norm = real
