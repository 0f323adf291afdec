"""The kernels that decide something no later tolerance can repair, each called on its own: ``bm_topk_rows`` (which
candidate counts as retrieved), ``bm_bn_finalize`` / ``_cm`` / ``bm_bn_eval_affine`` (what a BatchNorm layer normalises
with), ``bm_group_by_index`` / ``bm_index_to_i32`` (which subject's weights a segment gets), the three weight packers
(what the weights look like afterwards), ``bm_reduce_splits`` (how split-K partials land in the Adam bucket) and
``bm_fourier_emb`` at the reference's width.

Style and tolerances are tests/test_row_kernels_gpu.py's: floating-point results go through ``_held`` (kernel and the
same expression in fp32 on the CPU, both against fp64, both printed; an input on which plain fp32 is marginal is
replaced, not tolerated); integer results and fixed-order sums are compared exactly.

BatchNorm statistics of a channel whose mean dwarfs its spread -- the finalize kernels form the variance as
E[x^2] - E[x]^2 from fp32 partial sums, which cancels when |mean| >> std, and the data below keeps every channel's |mean|
within a few standard deviations -- are held in tests/test_bn_conditioning_gpu.py (every producer of partials on a ladder
of |mean| / std up to 1000, the law the variance error obeys, the envelope R_SAFE of the whole chain)."""
import math

import pytest
import torch
from torch.nn import functional as F

from helpers import rel_l2
from oracle import bm_oracle as O
from test_row_kernels_gpu import FWD_TOL, GRAD_TOL, _device_rows, _gen, _held

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MODES = ("f32", "f32x3", "f16x2")


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)
    hip_ops.set_kernel_timer(None)


@pytest.fixture()
def index_flag(H):
    """The device's flag word, zeroed before and after: a raised flag must not leak into another test's Solver."""
    flag = H.index_error_flag("cuda")
    flag.zero_()
    yield flag
    flag.zero_()


def _same_bits(a, b):
    """Equal element by element, a NaN only against a NaN."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- 1. top-k ----------------------------------------------------------------------------------------------------------
def topk_expected(x, k):
    """include/bm_hip.h: torch.sort(descending, stable) cut to k (NaN first, equal values by ascending column), -1 past
    the last column.  NOT torch.topk's indices: its order among equal values is unspecified."""
    rows, cols = x.shape
    vals, idx = torch.sort(x.double(), dim=1, descending=True, stable=True)
    out = torch.full((rows, k), -1, dtype=torch.int64)
    out[:, :min(k, cols)] = idx[:, :k]
    return out


def check_topk(H, x, k, what):
    rows, cols = x.shape
    want = topk_expected(x, k)
    idx, val, none = H.topk_rows(x.cuda(), k)
    assert none is None
    idx, val = idx.cpu().long(), val.cpu()
    assert torch.equal(idx, want), (what, (idx != want).nonzero()[:4].tolist())
    kk = min(k, cols)
    ref = x.topk(kk, dim=1).values
    assert _same_bits(val[:, :kk], ref), what
    assert torch.equal(torch.isnan(val[:, :kk]), torch.isnan(ref)), what
    assert _same_bits(val[:, :kk], torch.gather(x, 1, idx[:, :kk])), what            # the values of THOSE columns
    return idx


TOPK_SHAPES = [(1, 1, 1), (3, 63, 5), (5, 64, 64), (6, 65, 10), (7, 301, 10), (2, 5, 8)]


@pytest.mark.parametrize("rows,cols,k", TOPK_SHAPES)
def test_topk_shapes(H, rows, cols, k):
    """rows % 4 != 0 (four rows per workgroup), cols below / at / one past a wavefront, k == cols, k > cols."""
    x = torch.randn(rows, cols, generator=_gen(rows * 1000 + cols))
    idx = check_topk(H, x, k, f"topk {rows}x{cols} k={k}")
    if k > cols:
        assert bool((idx[:, cols:] == -1).all()) and bool((idx[:, :cols] >= 0).all())


@pytest.mark.parametrize("rows,cols,k", TOPK_SHAPES)
def test_topk_ties(H, rows, cols, k):
    """Rows quantised to four distinct values: every cut falls inside a run of equal values."""
    x = torch.randint(0, 4, (rows, cols), generator=_gen(rows + cols)).float() / 4 - 0.25       # -0.25, 0, 0.25, 0.5
    check_topk(H, x, k, f"topk ties {rows}x{cols} k={k}")
    if cols >= 63:
        x[0, ::2] = -0.0                    # -0 and +0 are one value
        check_topk(H, x, k, f"topk ties with -0 {rows}x{cols} k={k}")


def test_topk_underflowed_softmax(H):
    """A softmax with a wide logit spread is exactly 0.0 in most columns: the cut falls inside the run of zeros."""
    x = torch.softmax(torch.randn(3, 301, generator=_gen(5)) * 60, 1)
    zeros = (x == 0).sum(1)
    assert bool((zeros > 200).all()), zeros.tolist()
    for k in (80, 150, 301):
        assert bool((301 - zeros < k).all())                   # more than the non-zero columns: the cut is among the zeros
        check_topk(H, x, k, f"topk underflowed softmax k={k}")


@pytest.mark.parametrize("name,val", [("nan", NAN), ("+inf", INF), ("-inf", -INF)])
def test_topk_nonfinite(H, name, val):
    """One plant at the first column, the last, and either side of the lane-63 / lane-64 boundary; NaN ranks first like
    torch.topk's, -inf last (k = cols shows it)."""
    rows, cols = 5, 301
    x = torch.randn(rows, cols, generator=_gen(17))
    for at in (0, 63, 64, cols - 1):
        xp = x.clone()
        xp[at % rows, at] = val
        for k in (10, cols):
            idx = check_topk(H, xp, k, f"topk {name} at column {at} k={k}")
            if val != -INF:
                assert int(idx[at % rows, 0]) == at
            elif k == cols:
                assert int(idx[at % rows, cols - 1]) == at
    xp = x.clone()                                     # several of each in one row, and the issue's row
    xp[1, [3, 64, 200]] = val
    xp[2, [0, 63, 300]] = NAN
    xp[2, [5, 128]] = INF
    xp[2, [7, 129]] = -INF
    for k in (1, 10, cols):
        check_topk(H, xp, k, f"topk mixed {name} k={k}")
    small = torch.tensor([[.2, NAN, .7, .7, INF, -INF, 0, -0.0]])
    assert _same_bits(small.topk(5).values, torch.tensor([[NAN, INF, .7, .7, .2]]))
    assert check_topk(H, small, 5, "topk the row of the contract")[0].tolist() == [1, 4, 2, 3, 0]
    assert check_topk(H, small, 8, "topk the row of the contract")[0].tolist() == [1, 4, 2, 3, 0, 6, 7, 5]


def test_topk_all_nan_row(H):
    """An all-sensors-banned row is NaN throughout, here and in the reference: it returns columns 0 .. k-1."""
    x = torch.randn(6, 130, generator=_gen(23))
    x[4] = NAN
    for k in (1, 10, 130, 140):
        idx = check_topk(H, x, k, f"topk all-NaN row k={k}")
        assert idx[4, :min(k, 130)].tolist() == list(range(min(k, 130)))


def _hits(H, x, k, col_labels, row_labels, what, open_in_the_reference=False):
    """The rule of scripts/run_eval_probs.py:237-264 over the expected indices: a row is retrieved when its own label is
    among the labels of its top-k columns.  No run of equal values may straddle the cut (the reference's probs.topk
    would leave the choice open): asserted, not skipped -- except for ``open_in_the_reference``, the all-NaN row, where
    only this library's contract (ascending column) says which columns are retrieved."""
    vals = torch.sort(x.double(), dim=1, descending=True, stable=True).values
    if k < x.shape[1] and not open_in_the_reference:
        a, b = vals[:, k - 1], vals[:, k]
        assert not bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).any()), f"{what}: a tie run straddles the cut"
    want_idx = topk_expected(x, k)
    want = torch.tensor([int((col_labels[want_idx[r][want_idx[r] >= 0]] == row_labels[r]).any())
                         for r in range(len(x))], dtype=torch.int32)
    idx, _, hits = H.topk_rows(x.cuda(), k, col_labels.cuda(), row_labels.cuda())
    assert torch.equal(idx.cpu().long(), want_idx), what
    assert torch.equal(hits.cpu(), want), (what, hits.tolist(), want.tolist())
    return want


def test_topk_hit_flag(H):
    g = _gen(31)
    rows, cols, k = 7, 301, 10
    x = torch.randn(rows, cols, generator=g)
    # duplicate column labels, one row label absent from the columns
    col = torch.randint(0, 40, (cols,), generator=g)
    row = torch.randint(0, 40, (rows,), generator=g)
    row[3] = 77
    top = topk_expected(x, k)
    row[0] = col[top[0, k - 1]]                         # the last column inside the cut
    row[1] = col[top[1, 0]]
    want = _hits(H, x, k, col, row, "duplicate labels")
    assert want[0] == 1 and want[1] == 1 and want[3] == 0 and 0 < int(want.sum()) < rows
    # labels above 2^31, all equal modulo 2^32: only the full 64 bits tell them apart
    col = 5 + 2 ** 32 * (torch.arange(cols) + 1)
    assert col.dtype == torch.int64 and bool((col > 2 ** 31).all()) and len(set((col % 2 ** 32).tolist())) == 1
    row = torch.empty(rows, dtype=torch.int64)
    for r in range(rows):
        row[r] = [col[top[r, r]], 5, 5 + 2 ** 32 * (cols + 9), col[top[r, 0]] + 2 ** 33][r % 4]
    want = _hits(H, x, k, col, row, "labels above 2^31")
    assert want.tolist() == [1 if r % 4 == 0 else 0 for r in range(rows)]
    # k > cols: the -1 padding never hits, whatever the label
    xs = torch.randn(2, 5, generator=g)
    want = _hits(H, xs, 8, torch.tensor([3, 3, 4, 9, 0]), torch.tensor([0, 7]), "k > cols")
    assert want.tolist() == [1, 0]
    # a NaN row: columns 0 .. k-1 are what it retrieves
    xn = x.clone()
    xn[2] = NAN
    col = torch.arange(cols)
    row = torch.tensor([cols, cols, k - 1, cols, cols, cols, cols])
    assert _hits(H, xn, k, col, row, "NaN row", open_in_the_reference=True)[2] == 1
    row[2] = k
    assert _hits(H, xn, k, col, row, "NaN row", open_in_the_reference=True)[2] == 0


# ---- 2. BatchNorm finalize and eval affine -----------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_reference(stats, count, gamma, beta, rm, rv, dtype):
    """torch's BatchNorm rule on the fp32 partials [ntiles][C][2], in ``dtype`` arithmetic: (mean, invstd, scale, shift,
    running_mean', running_var', the variance before the clamp)."""
    s = stats.to(dtype).sum(0)
    mean = s[:, 0] / count
    raw = s[:, 1] / count - mean * mean
    var = raw.clamp_min(0)
    invstd = 1 / torch.sqrt(var + BN_EPS)
    scale = invstd * (gamma.to(dtype) if gamma is not None else 1)
    shift = (beta.to(dtype) if beta is not None else 0) - mean * scale
    out = [mean, invstd, scale, shift]
    if rm is not None:
        unbiased = var * count / (count - 1) if count > 1 else var
        out += [(1 - BN_MOMENTUM) * rm.to(dtype) + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * rv.to(dtype) + BN_MOMENTUM * unbiased]
    return out + [raw]


def bn_partials(C, ntiles, count, seed):
    """fp32 partials of ``count`` samples per channel.  count = ntiles * 4: four samples per tile, per-channel mean
    within one standard deviation of zero (see the module text).  count = 1, 2: the samples sit in the first and the
    last tile and are multiples of 1/64 below 8 -- their squares and sums are exact in fp32, so that the fp32 and fp64
    evaluations of E[x^2] - E[x]^2 see the same numbers (count = 2: opposite signs, the mean does not dwarf the
    spread)."""
    g = _gen(seed)
    stats = torch.zeros(ntiles, C, 2)
    if count == ntiles * 4:
        std = torch.rand(C, generator=g) * 1.5 + 0.5
        mean = (torch.rand(C, generator=g) * 2 - 1) * std
        x = torch.randn(ntiles, C, 4, generator=g) * std[None, :, None] + mean[None, :, None]
        stats[..., 0], stats[..., 1] = x.sum(2), (x * x).sum(2)
        return stats
    a = torch.randint(32, 512, (C,), generator=g).float() / 64
    stats[0, :, 0], stats[0, :, 1] = a, a * a
    if count == 2:
        b = -torch.randint(32, 512, (C,), generator=g).float() / 64
        stats[-1, :, 0] += b
        stats[-1, :, 1] += b * b
    return stats


def bn_case(C, ntiles, count, affine, running, seed):
    g = _gen(seed + 1)
    stats = bn_partials(C, ntiles, count, seed)
    gamma = torch.rand(C, generator=g) + 0.5 if affine else None
    beta = torch.rand(C, generator=g) + 2.0 if affine else None        # (shift = beta - mean * scale stays away from 0)
    rm = torch.randn(C, generator=g) * 0.3 + 0.5 if running else None
    rv = torch.rand(C, generator=g) + 0.5 if running else None
    return stats, gamma, beta, rm, rv


BN_NAMES = ["mean", "invstd", "scale", "shift", "running_mean", "running_var"]


def bn_counts(ntiles):
    return [1, 2, ntiles * 4]


def test_bn_reference_is_batchnorm1d():
    """Proves the reference above, not a kernel: BatchNorm1d in float64 on a tensor whose per-tile sums were taken in
    fp32 (one rounding per partial: 1e-6)."""
    g = _gen(3)
    B, C, T = 6, 5, 40
    x = torch.randn(B, C, T, generator=g) * 1.3 + 0.4
    tiles = x.view(B, C, 4, 10).permute(0, 2, 1, 3).reshape(B * 4, C, 10)
    stats = torch.stack([tiles.sum(2), (tiles * tiles).sum(2)], 2)
    bn = torch.nn.BatchNorm1d(C, eps=BN_EPS, momentum=BN_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.uniform_(-1, 1, generator=g)
        bn.running_mean.uniform_(-1, 1, generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    y = bn(x.double())
    mean, invstd, scale, shift, rm2, rv2, _ = bn_reference(stats, B * T, bn.weight.detach(), bn.bias.detach(), rm, rv,
                                                            torch.float64)
    assert rel_l2(x.double() * scale[None, :, None] + shift[None, :, None], y) < 1e-6
    assert rel_l2(rm2, bn.running_mean) < 1e-6 and rel_l2(rv2, bn.running_var) < 1e-6
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("C", [1, 5, 320])
@pytest.mark.parametrize("ntiles", [1, 63, 64, 65, 1000])             # either side of the 64-thread fold, and a long one
def test_bn_finalize(H, C, ntiles):
    for count in bn_counts(ntiles):
        for affine in (True, False):
            for running in (True, False):
                what = f"bn_finalize C={C} ntiles={ntiles} count={count} affine={affine} running={running}"
                stats, gamma, beta, rm, rv = bn_case(C, ntiles, count, affine, running, C * 7 + ntiles)
                ref64 = bn_reference(stats, count, gamma, beta, rm, rv, torch.float64)[:-1]
                ref32 = bn_reference(stats, count, gamma, beta, rm, rv, torch.float32)[:-1]
                cu = lambda t: None if t is None else t.cuda()       # noqa: E731

                def run(st):
                    rmg, rvg = cu(rm), cu(rv)
                    nb = torch.tensor(41, dtype=torch.int64).cuda() if running else None
                    out = list(H.bn_finalize(st, count, cu(gamma), cu(beta), rmg, rvg, nb, BN_MOMENTUM, BN_EPS))
                    if running:
                        assert int(nb) == 42, (what, int(nb))                     # +1 per call, not per channel
                        H.bn_finalize(st, count, cu(gamma), cu(beta), rmg.clone(), rvg.clone(), nb, BN_MOMENTUM, BN_EPS)
                        assert int(nb) == 43, (what, int(nb))
                        out += [rmg, rvg]
                    return out
                got = run(stats.cuda())
                assert len(got) == len(ref64)
                for name, o, r64, r32 in zip(BN_NAMES, got, ref64, ref32):
                    assert bool(torch.isfinite(o).all()), (what, name)
                    _held(f"{what} {name}", o, r64, r32, FWD_TOL)
                # the channel-major layout of the same partials: bit for bit
                cm = stats.transpose(0, 1).contiguous().cuda()
                cm._bm_channel_major = True
                for name, o, o_cm in zip(BN_NAMES, got, run(cm)):
                    assert torch.equal(o, o_cm), (what, name, "channel-major differs")
                if count == 1 and running:
                    # one sample: variance 0, biased and "unbiased" alike (no division by count - 1 = 0)
                    assert rel_l2(got[5], (1 - BN_MOMENTUM) * rv.double()) < FWD_TOL


def test_bn_finalize_clamps_a_negative_variance(H):
    """A constant channel: E[x^2] - E[x]^2 of the fp32 partials is round-off, here negative.  No NaN;
    invstd = 1 / sqrt(eps) to fp32 rounding; the running variance takes 0."""
    C, ntiles = 3, 65
    v = next(torch.tensor(c) for c in (0.3, 0.7, 1.1, 1.3, 2.3) if float(torch.tensor(c) * torch.tensor(c)) < float(torch.tensor(c)) ** 2)
    stats = bn_partials(C, ntiles, ntiles * 4, 9)
    stats[:, 1, 0], stats[:, 1, 1] = 4 * v, 4 * (v * v)                 # four copies per tile: exact in fp32
    rm, rv = torch.zeros(C), torch.ones(C)
    ref = bn_reference(stats, ntiles * 4, None, None, rm, rv, torch.float64)
    assert float(ref[-1][1]) < 0 and float(ref[-1][0]) > 0.1              # the clamp is what the constant channel takes
    for cm in (False, True):
        st = (stats.transpose(0, 1).contiguous() if cm else stats).cuda()
        st._bm_channel_major = cm
        rmg, rvg = rm.cuda(), rv.cuda()
        got = list(H.bn_finalize(st, ntiles * 4, None, None, rmg, rvg, None, BN_MOMENTUM, BN_EPS)) + [rmg, rvg]
        for name, o, r in zip(BN_NAMES, got, ref):
            assert bool(torch.isfinite(o).all()), name
            assert rel_l2(o, r) < FWD_TOL, (name, rel_l2(o, r))
        want = 1 / math.sqrt(BN_EPS)
        assert abs(float(got[1][1]) - want) <= 2.0 ** -23 * want
        assert float(got[0][1]) == float(v) and float(rvg[1]) == pytest.approx(0.9, rel=1e-6)


@pytest.mark.parametrize("C", [1, 257])                                # 257: a second workgroup
@pytest.mark.parametrize("affine", [True, False])
def test_bn_eval_affine(H, C, affine):
    g = _gen(C + affine)
    gamma = torch.rand(C, generator=g) + 0.5 if affine else None
    beta = torch.rand(C, generator=g) + 2.0 if affine else None
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.1

    def formula(dt):
        invstd = 1 / torch.sqrt(rv.to(dt) + BN_EPS)
        scale = invstd * (gamma.to(dt) if affine else 1)
        return [rm.to(dt), invstd, scale, (beta.to(dt) if affine else 0) - rm.to(dt) * scale]
    got = H.bn_eval_affine(gamma.cuda() if affine else None, beta.cuda() if affine else None, rm.cuda(), rv.cuda(), BN_EPS)
    for name, o, r64, r32 in zip(BN_NAMES, got, formula(torch.float64), formula(torch.float32)):
        _held(f"bn_eval_affine C={C} affine={affine} {name}", o, r64, r32, FWD_TOL)
    assert torch.equal(got[0].cpu(), rm)


# ---- 3. grouping and index conversion ----------------------------------------------------------------------------------
def counting_sort(idx, G):
    """(order of the valid segments, seg [G + 1]): a stable counting sort in plain Python."""
    buckets = [[] for _ in range(G)]
    for b, v in enumerate(idx):
        if 0 <= v < G:
            buckets[v].append(b)
    seg = [0]
    for bk in buckets:
        seg.append(seg[-1] + len(bk))
    return [b for bk in buckets for b in bk], seg


def group_indices(B, G, pattern, g):
    if pattern == "one group" or G == 1:
        return torch.full((B,), G // 2, dtype=torch.int64)
    live = [v for v in range(G) if v not in (0, G // 2, G - 1)]          # empty at the front, in the middle, at the back
    return torch.tensor(live, dtype=torch.int64)[torch.randint(0, len(live), (B,), generator=g)]


def check_grouping(H, idx, G, what):
    order_ref, seg_ref = counting_sort(idx.tolist(), G)
    order, seg = H.group_by_index(idx.cuda(), G)
    assert seg.dtype == torch.int32 and order.dtype == torch.int32
    assert seg.tolist() == seg_ref, what
    assert order[:seg_ref[-1]].tolist() == order_ref, what
    order2, seg2 = H.group_by_index(idx.cuda(), G)                        # deterministic
    assert torch.equal(seg2, seg) and torch.equal(order2[:seg_ref[-1]], order[:seg_ref[-1]]), what
    i32 = H.index_i32(idx.cuda(), G)
    assert i32.dtype == torch.int32
    assert i32.tolist() == [v if 0 <= v < G else 0 for v in idx.tolist()], what
    return order_ref, seg_ref


@pytest.mark.parametrize("B", [0, 1, 7, 8, 9, 255, 256, 257, 1000])    # the 8-wide LDS scan, the 256 threads
@pytest.mark.parametrize("G", [1, 7, 300])                               # 300: the per-group fill loop strides
def test_group_by_index(H, index_flag, B, G):
    g = _gen(B * 31 + G)
    for pattern in ("empty groups", "one group"):
        idx = group_indices(B, G, pattern, g)
        _, seg = check_grouping(H, idx, G, f"group_by_index B={B} G={G} {pattern}")
        assert seg[-1] == B
        if G >= 7 and pattern == "empty groups":
            assert seg[1] == 0 and seg[G // 2] == seg[G // 2 + 1] and seg[G - 1] == B
    assert index_flag.tolist() == [0, 0, 0]


@pytest.mark.parametrize("bad", [-1, "G", 2 ** 31, 2 ** 32 + 1])         # 2^32 + 1 is 1 after an int32 truncation
def test_rejected_indices(H, index_flag, bad):
    g = _gen(44)
    for B, G in ((9, 7), (257, 7), (300, 300)):
        val = G if bad == "G" else bad
        for at in sorted({0, B // 2, B - 1}):
            idx = group_indices(B, G, "empty groups", g)
            idx[at] = val
            index_flag.zero_()
            order_ref, seg = check_grouping(H, idx, G, f"rejected {val} at {at} of B={B} G={G}")
            assert seg[-1] == B - 1 and at not in order_ref
            assert index_flag.tolist() == [1, 0, 0]
            index_flag.zero_()
            H.index_i32(idx.cuda(), G)                                      # either kernel raises it on its own
            assert index_flag.tolist() == [1, 0, 0]
            index_flag.zero_()
            H.group_by_index(idx.cuda(), G)
            assert index_flag.tolist() == [1, 0, 0]


def test_index_flag_is_sticky_and_raised_once(H, index_flag):
    g = _gen(45)
    good = group_indices(100, 7, "empty groups", g)
    bad = good.clone()
    bad[50] = 7
    H.group_by_index(bad.cuda(), 7)
    assert index_flag.tolist() == [1, 0, 0]
    check_grouping(H, good, 7, "in-range call after a rejected one")       # leaves the flag raised
    assert index_flag.tolist() == [1, 0, 0]
    index_flag[1:] = 1                                                        # the Solver's words
    with pytest.raises(IndexError):
        H.raise_if_index_error("cuda")
    assert index_flag.tolist() == [0, 1, 1]
    H.raise_if_index_error("cuda")                                           # once


def test_group_by_index_at_the_lds_bound(H, index_flag):
    """One workgroup holds (G + 1 + B) ints in dynamic LDS.  A HIP launch accepts hipDeviceProp_t::sharedMemPerBlock =
    64 KiB of it; beyond that (sharedMemPerBlockOptin) a kernel has to raise its
    hipFuncAttributeMaxDynamicSharedMemorySize first, which this one does not: B + G + 1 <= 16 384.  The largest
    accepted shape is sorted right; one int more is refused on the host, before any launch."""
    g = _gen(46)
    B, G = 16000, 383
    assert (B + G + 1) * 4 == 64 * 1024
    idx = group_indices(B, G, "empty groups", g)
    check_grouping(H, idx, G, f"group_by_index B={B} G={G}")
    idx[[0, 8000, B - 1]] = torch.tensor([-1, G, 2 ** 32 + 1])
    _, seg = check_grouping(H, idx, G, f"group_by_index B={B} G={G} with rejected indices")
    assert seg[-1] == B - 3 and index_flag.tolist() == [1, 0, 0]
    from brainmagick_amd._lib import BmHipError
    for B2, G2 in ((16000, 384), (16000, 16000), (8, 16376)):
        with pytest.raises(BmHipError, match="LDS"):
            H.group_by_index(torch.zeros(B2, dtype=torch.int64).cuda(), G2)


# ---- 4. the weight packers, through the conv they feed -----------------------------------------------------------------
NARROW = dict(Cin=20, M=12, T=48, B=3)
WIDE = dict(Cin=40, M=96, T=132, B=3)           # the smallest rows / length class the wide f16x2 kernel takes, 3 taps


def pack_case(dims, KS, layout, flip, alpha, seed):
    """(x, src, pack arguments, widx | None, effective weights [G, M, Cin, KS] as the strides describe them)."""
    Cin, M, T, B = dims["Cin"], dims["M"], dims["T"], dims["B"]
    g = _gen(seed)
    x = torch.randn(B, Cin, T, generator=g)
    G, widx = 1, None
    if layout == "conv":                         # nn.Conv1d [M, Cin, KS]
        src = torch.randn(M, Cin, KS, generator=g)
        sg, sm, sc, sj = 0, Cin * KS, KS, 1
        w = src[None]
    elif layout == "transposed":                 # nn.ConvTranspose1d [Cin, M, KS]
        src = torch.randn(Cin, M, KS, generator=g)
        sg, sm, sc, sj = 0, KS, M * KS, 1
        w = src.permute(1, 0, 2)[None]
    else:                                        # a table [G, Cin, M, KS], one group per segment through widx
        G, widx = 3, torch.tensor([2, 0, 2], dtype=torch.int32)
        assert B == 3
        src = torch.randn(G, Cin, M, KS, generator=g)
        sg, sm, sc, sj = Cin * M * KS, KS, M * KS, 1
        w = src.permute(0, 2, 1, 3)
    src = src / math.sqrt(Cin * KS)
    w = w / math.sqrt(Cin * KS)
    if flip:
        w = w.flip(-1)
    return x, src.contiguous(), (G, M, Cin, KS, sg, sm, sc, sj), widx, w.contiguous(), alpha


def conv_reference(x, w, widx, alpha, dt):
    KS = w.shape[-1]
    a = torch.tensor(1.0 if alpha is None else alpha, dtype=torch.float32).to(dt)
    sel = widx.long() if widx is not None else torch.zeros(len(x), dtype=torch.int64)
    return torch.cat([F.conv1d(x[b:b + 1].to(dt), a * w[sel[b]].to(dt), padding=KS // 2) for b in range(len(x))])


PACK_VARIANTS = [(layout, flip, alpha) for layout in ("conv", "transposed") for flip in (False, True)
                 for alpha in (None, 0.37)] + [("table", flip, alpha) for flip in (False, True) for alpha in (None, 0.37)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["narrow k5", "narrow k3", "wide k3"])
def test_packers_through_their_conv(H, mode, shape):
    """The packed layouts are private: each packer (exact fp32, 3 x bf16, 2 x f16) is seen through the conv it feeds,
    against F.conv1d in float64 on the weights as the strides describe them -- 5 taps, the tap flip, alpha from a
    device scalar, the ConvTranspose order, a grouped table behind widx."""
    dims, KS = (WIDE, 3) if shape == "wide k3" else (NARROW, 5 if shape == "narrow k5" else 3)
    layouts = {"narrow k5": ("conv", "transposed"), "narrow k3": ("table",),
               "wide k3": ("conv", "transposed", "table")}[shape]
    H.set_compute_dtype(mode)
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        if shape == "wide k3":
            assert H.lib().bm_conv_h2_covers(dims["Cin"], dims["M"], dims["T"], KS, 1)
            assert not H.lib().bm_conv_h2_covers(dims["Cin"], dims["M"], 128, KS, 1)       # T: the smallest class
        for layout, flip, alpha in PACK_VARIANTS:
            if layout not in layouts:
                continue
            what = f"pack[{mode}] {shape} {layout} flip={flip} alpha={alpha}"
            x, src, geom, widx, w, _ = pack_case(dims, KS, layout, flip, alpha, len(layout) + KS + flip)
            ag = torch.tensor(alpha).cuda() if alpha is not None else None         # a device scalar
            wp = H.pack_weights(src.cuda(), *geom, flip=flip, alpha=ag, shape=(dims["T"], 1))
            if mode == "f16x2":
                assert wp._bm_mode == ("f16x2" if shape == "wide k3" else "f32x3"), what
            n = len(timer.records)
            y = H.conv_nn(x.cuda(), wp, dims["M"], KS, 1, widx=widx.cuda() if widx is not None else None)[1]
            if mode == "f16x2" and shape == "wide k3":
                assert timer.records[n][0].startswith("conv_nn_h2w_kernel<3,"), timer.records[n][0]
            _held(what, y, conv_reference(x, w, widx, alpha, torch.float64),
                  conv_reference(x, w, widx, alpha, torch.float32), FWD_TOL)
    finally:
        H.set_kernel_timer(None)
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.fixture()
def h2_mode(H):
    H.set_compute_dtype("f16x2")
    yield
    H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


@pytest.mark.parametrize("zero", ["x", "segment", "weight row", "weights"])
def test_f16x2_zeros_through_the_wide_conv(H, h2_mode, zero):
    """A tensor, a segment or a weight row whose maximum is 0 (bm_scale_from_amax then takes s = 1): exactly 0.0 where
    the mathematics is zero, the usual tolerance elsewhere, no inf / NaN anywhere."""
    x, src, geom, _, w, _ = pack_case(WIDE, 3, "conv", False, None, 91)
    M, T = WIDE["M"], WIDE["T"]
    is_zero = torch.zeros(WIDE["B"], M, T, dtype=torch.bool)
    if zero == "x":
        x.zero_()
        is_zero[:] = True
    elif zero == "segment":
        x[1].zero_()
        is_zero[1] = True
    elif zero == "weight row":
        src[7].zero_()
        is_zero[:, 7] = True
    else:
        src.zero_()
        is_zero[:] = True
    wp = H.pack_weights(src.cuda(), *geom, shape=(T, 1))
    assert wp._bm_mode == "f16x2"
    y = H.conv_nn(x.cuda(), wp, M, 3, 1)[1].cpu()
    assert bool(torch.isfinite(y).all())
    ref64, ref32 = conv_reference(x, src[None], None, None, torch.float64), conv_reference(x, src[None], None, None, torch.float32)
    assert float(ref64[is_zero].abs().sum()) == 0.0
    assert float(y[is_zero].abs().max()) == 0.0, f"zero {zero}: {int((y[is_zero] != 0).sum())} elements are not 0"
    if not bool(is_zero.all()):
        _held(f"f16x2 conv with a zero {zero}", y[~is_zero], ref64[~is_zero], ref32[~is_zero], FWD_TOL)


def wgrad_reference(a, x, KS, dil, dt):
    """dw[m][c][j] = sum_{s, t} a[s][m][t] * x[s][c][t + (j - KS // 2) * dil]."""
    w = torch.zeros(a.shape[1], x.shape[1], KS, dtype=dt, requires_grad=True)
    F.conv1d(x.to(dt), w, padding=KS // 2 * dil, dilation=dil).backward(a.to(dt))
    return w.grad


@pytest.mark.parametrize("T", [132, 130])                  # the row-scaled kernel (T % 4 == 0) and its fall-back
def test_f16x2_weight_gradient_with_a_dead_channel(H, h2_mode, T):
    """bm_gemm_nt_h2_rows with one all-zero row of ``a`` (a dead ReLU channel: row maximum 0) in the 320-row family."""
    S, M, Cn, KS, dil, dead = 8, 320, 64, 3, 1, 37
    assert H.lib().bm_gemm_nt_h2_covers(M, Cn, KS, S, T, 1, dil, 0)
    g = _gen(T)
    a = torch.randn(S, M, T, generator=g)
    a[:, dead] = 0
    x = torch.randn(S, Cn, T, generator=g)
    ag = a.cuda()
    rows = ag.abs().amax(dim=(0, 2)).contiguous()
    assert float(rows[dead]) == 0.0
    ag._bm_row_amax = (ag._version, ag.data_ptr(), rows)              # as act_bn_bwd / glu_bwd publish them
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        dw = H.gemm_nt(ag, x.cuda(), S, M, Cn, T, KS, dil)[0].cpu()
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["gemm_nt_h2w_kernel<KS=3>"]
    assert bool(torch.isfinite(dw).all())
    assert float(dw[dead].abs().max()) == 0.0
    live = torch.ones(M, dtype=torch.bool)
    live[dead] = False
    _held(f"gemm_nt_h2_rows T={T} with a dead channel", dw[live], wgrad_reference(a, x, KS, dil, torch.float64)[live],
          wgrad_reference(a, x, KS, dil, torch.float32)[live], GRAD_TOL)


# ---- 5. split folding --------------------------------------------------------------------------------------------------
def fold_in_order(part):
    """part [G, nsplit, M, N] -> [G, M, N]: fp32, k = 0, 1, ..., one addition at a time (the order include/bm_hip.h
    promises)."""
    s = torch.zeros_like(part[:, 0])
    for k in range(part.shape[1]):
        s = s + part[:, k]
    return s


def reduce_splits(H, part, out, G, nsplit, M, Cn, KS, strides):
    from brainmagick_amd.hip_ops import _p, _stream, check
    check(H.lib().bm_reduce_splits(_p(part), _p(out), G, nsplit, M, Cn, KS, *strides, _stream()), "bm_reduce_splits")


@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 17])                    # the 8-wide unrolled fold and its tail
@pytest.mark.parametrize("G,M,Cn,KS", [(1, 3, 5, 1),                    # 15 elements: the scalar path
                                       (1, 8, 6, 3),                    # the float4 path
                                       (3, 4, 5, 3)])                   # float4, quads must not cross a group
def test_reduce_splits(H, nsplit, G, M, Cn, KS):
    what = f"reduce_splits G={G} nsplit={nsplit} M={M} Cn={Cn} KS={KS}"
    per = M * Cn * KS
    part = torch.randn(G, nsplit, M, Cn * KS, generator=_gen(nsplit * 100 + per))
    want = fold_in_order(part).view(G, M, Cn, KS)
    assert nsplit < 3 or not torch.equal(want, part.flip(1).double().sum(1).float().view(G, M, Cn, KS))   # order matters
    pg = part.cuda()
    assert pg.data_ptr() % 16 == 0
    # contiguous
    out = torch.full((G, M, Cn, KS), NAN).cuda()
    reduce_splits(H, pg, out, G, nsplit, M, Cn, KS, (per, Cn * KS, KS, 1))
    assert torch.equal(out.cpu(), want), what
    # behind a pointer 4 bytes past a 16-byte boundary: the scalar path, the identical bits
    if per % 4 == 0:
        out2 = torch.full((G, M, Cn, KS), NAN).cuda()
        reduce_splits(H, _device_rows(part, True), out2, G, nsplit, M, Cn, KS, (per, Cn * KS, KS, 1))
        assert torch.equal(out2, out), what + " misaligned"
    # transposed: [G][Cn][M][KS] (KS = 1: sm = 1, sc = M)
    out = torch.full((G, Cn, M, KS), NAN).cuda()
    reduce_splits(H, pg, out, G, nsplit, M, Cn, KS, (per, KS, M * KS, 1))
    assert torch.equal(out.cpu(), want.permute(0, 2, 1, 3)), what + " transposed"
    # a strided window inside a larger buffer (how gradients land in the flat Adam bucket): nothing else is touched
    sj, base = 2, 7
    sc = KS * sj + 1
    sm = Cn * sc + 5
    sg = M * sm + 11
    canary = -777.0
    buf = torch.full((base + G * sg + 13,), canary).cuda()
    reduce_splits(H, pg, buf[base:], G, nsplit, M, Cn, KS, (sg, sm, sc, sj))
    at = (base + torch.arange(G)[:, None, None, None] * sg + torch.arange(M)[None, :, None, None] * sm
          + torch.arange(Cn)[None, None, :, None] * sc + torch.arange(KS)[None, None, None, :] * sj)
    assert int(at.max()) < buf.numel() and at.unique().numel() == at.numel()
    got = buf.cpu()
    assert torch.equal(got[at], want), what + " strided"
    untouched = torch.ones(buf.numel(), dtype=torch.bool)
    untouched[at.flatten()] = False
    assert bool((got[untouched] == canary).all()), what + " strided: the canary moved"


# ---- 6. Fourier embedding at the reference's width ---------------------------------------------------------------------
def fourier_args(positions, D, margin):
    """The fp32 arguments of cos / sin, in the operation order of bm_oracle.fourier_emb (bm/models/common.py:254-271)."""
    nf = int(round((D // 2) ** 0.5))
    fy = torch.arange(float(nf)).to(positions)
    fx = fy[:, None]
    width = 1 + 2 * margin
    p = positions + margin
    px, py = 2 * math.pi * fx / width, 2 * math.pi * fy / width
    p = p[..., None, None, :]
    return (p[..., 0] * px + p[..., 1] * py).view(*positions.shape[:-1], -1)


@pytest.mark.parametrize("D", [2, 8, 288, 2048])                        # 2048: the reference's default, 32 frequencies
@pytest.mark.parametrize("rows", [1, 45, 273])
@pytest.mark.parametrize("margin", [0.2, 0.0])
def test_fourier_emb(H, D, rows, margin):
    """Against the oracle's fp32 operation order, largest absolute difference 5e-6.  A float64 evaluation of the
    embedding is NOT the yardstick: the fp32 argument of cos is itself rounded at about 3e-5 near 300 (D = 2048), which
    is why the kernel mirrors the reference's operation order and is held to cos / sin of the IDENTICAL fp32
    arguments.  Printed next to it: how far torch's own fp32 cos / sin and the kernel's are from float64 cos / sin of
    those arguments."""
    g = _gen(D + rows)
    pos = torch.rand(rows, 2, generator=g)
    if rows > 1:
        pos[rows // 3] = O.INVALID
        pos[-1] = O.INVALID
        assert bool(O.is_invalid(pos).any())
    ref = O.fourier_emb(pos, D, margin)
    loc = fourier_args(pos, D, margin)
    assert torch.equal(torch.cat([torch.cos(loc), torch.sin(loc)], -1), ref)           # the same arguments
    exact = torch.cat([torch.cos(loc.double()), torch.sin(loc.double())], -1)
    emb = H.fourier_emb(pos.cuda(), D, margin).cpu()
    assert emb.shape == (rows, D)
    err = float((emb - ref).abs().max())
    print(f"fourier_emb D={D} rows={rows} margin={margin}: max |arg| {float(loc.abs().max()):.0f}, kernel vs oracle "
          f"{err:.2e}; vs float64 cos / sin of the fp32 arguments: kernel {float((emb.double() - exact).abs().max()):.2e}"
          f", torch fp32 {float((ref.double() - exact).abs().max()):.2e}")
    if D == 2048 and rows > 1:
        assert float(loc.abs().max()) > 200
    assert err < 5e-6
