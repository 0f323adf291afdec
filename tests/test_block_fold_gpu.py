"""The shared last-arriver fold (csrc/bm_block.h) where it can go wrong: a maximum that sits on the border between two
workgroups' elements, a ticket counter that one grid hands to another, and the two finalize launches on the same
folds.  Every published maximum is compared exactly: a maximum is one of the tensor's own values.  All in f16x2 mode,
the only one that publishes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANT = -1234.5       # |.| far above everything else (<= 1), sign against a missing fabsf


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    hip_ops.set_compute_dtype("f16x2")
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


def _unit(shape, seed):
    """Values in [-1, 1]."""
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


# Each runner: input tensor(s) -> (published slot maximum, the tensor it describes); the asserts common to a kernel.
def _meg_init(H, meg):
    x = H.meg_init(meg, meg.shape[-1])                  # limit = T: everything is kept
    assert torch.equal(x, meg)
    return float(H._noted(x, "_bm_amax").max()), x


LOWPASS = dict(cutoff=0.25, zeros=2)                    # half = int(2 / 0.25 / 2) = 4 taps either side


def _lowpass(H, x):
    y = H.lowpass_filter(x, **LOWPASS)
    return float(H._noted(y, "_bm_amax").max()), y


def _regress_bwd(H, pair):
    est, out = pair
    _, count = H.regress_loss_fwd(est, out, None, "mse")
    dest, _ = H.regress_loss_bwd(est, out, None, "mse", torch.ones((), device="cuda"), count)
    assert torch.equal(H.row_amax_of(dest), dest.abs().amax((0, 2)))
    return float(H._noted(dest, "_bm_amax").max()), dest


# The smallest shapes with two workgroups, and the flat indices (first, last, last of the first workgroup, first of
# the second workgroup) of the output:
#   meg_init  (3, 9, 320): T % 4 == 0, 2 160 vectors of 4; a workgroup takes MI_THREADS * MI_UNROLL = 512 * 4 = 2 048
#             consecutive vectors = 8 192 elements, so two workgroups, the second with 112 vectors.
#   lowpass   (600, 16): R = ceil(600 / LP_MAX_BLOCKS = 256) = 3 rows per workgroup (far below the 8192 / 24 that fit
#             the LDS), 200 workgroups; workgroup 0 owns the rows 0 .. 2 = the elements [0, 48).  A sample only reaches
#             outputs of its own row.
#   regress   B = 4, F = 3, T = 8: nsplit = min(ceil(2048 / F), B) = 4 batch ranges of one segment, grid (4, 3);
#             workgroup (split 0, f 0) owns (b 0, f 0, :) = [0, 8), the next one, (split 1, f 0), starts at
#             (b 1, f 0, 0) = F * T = 24.
PLANTED = {
    "meg_init": ((3, 9, 320), (1, 1, 8), [0, 3 * 9 * 320 - 1, 8191, 8192]),
    "lowpass": ((600, 16), (1, 8), [0, 600 * 16 - 1, 47, 48]),
    "regress_bwd": ((4, 3, 8), (1, 1, 8), [0, 4 * 3 * 8 - 1, 7, 24]),
}


def _planted_case(H, kernel, shape, at, seed):
    """Runs `kernel` with PLANT at flat index `at`; returns (published, output, the planted row of the output)."""
    base = _unit(shape, seed)
    base.view(-1)[at] = PLANT
    T = shape[-1]
    if kernel == "meg_init":
        got, y = _meg_init(H, base)
    elif kernel == "lowpass":
        got, y = _lowpass(H, base)
    else:
        out = _unit(shape, seed + 1)
        base.view(-1)[at] = out.view(-1)[at] + PLANT    # the difference is what the gradient scales
        got, y = _regress_bwd(H, (base, out))
    return got, y, at // T


@pytest.mark.parametrize("kernel", sorted(PLANTED))
def test_planted_maximum_at_workgroup_borders(H, kernel):
    many, one, positions = PLANTED[kernel]
    cases = [(many, at) for at in positions] + [(one, 0), (one, one[-1] - 1)]
    for i, (shape, at) in enumerate(cases):
        got, y, row = _planted_case(H, kernel, shape, at, seed=10 * i)
        rows = y.abs().reshape(-1, shape[-1]).amax(1)
        assert int(rows.argmax()) == row, (kernel, shape, at)          # the plant is the maximum, where it was put
        if kernel == "meg_init":
            assert got == abs(PLANT), (kernel, shape, at)
        elif kernel == "regress_bwd":
            assert got == abs(float(y.view(-1)[at])), (kernel, shape, at)
        assert got == float(y.abs().max()), (kernel, shape, at)


@pytest.mark.parametrize("kernel", sorted(PLANTED))
def test_ticket_is_handed_from_grid_to_grid(H, kernel):
    """Many workgroups, one workgroup, many again with other data, on one stream = one workspace: a ticket counter that
    did not return to zero makes the wrong workgroup fold (a stale or missing maximum), or none."""
    many, one, _ = PLANTED[kernel]
    run = {"meg_init": _meg_init, "lowpass": _lowpass, "regress_bwd": _regress_bwd}[kernel]
    for i, shape in enumerate([many, one, many, one, many]):
        scale = [3.0, 0.25, 0.5, 7.0, 1.0][i]          # every launch has another maximum, also smaller than the one before
        data = _unit(shape, 100 + i) * scale
        arg = (data, _unit(shape, 200 + i)) if kernel == "regress_bwd" else data
        got, y = run(H, arg)
        assert got == float(y.abs().max()), (kernel, i, shape)


@pytest.mark.parametrize("n", [1, 1024 * 17 + 3])
def test_amax_scan_finalize(H, n):
    """bm_amax: per-workgroup maxima, then the one-workgroup fold.  The maximum is the last element."""
    x = _unit((n,), n)
    x[-1] = PLANT
    scans = H.amax_scans
    slot = H.amax(x)
    assert H.amax_scans == scans + 1 and slot.shape == (H.AMAX_SHARDS,)
    assert float(slot.max()) == abs(PLANT) and not bool(slot[1:].any())


def test_act_bn_bwd_row_maxima_small(H):
    """The per-row fold over [nsplit][C] partials at a shape with fewer channels than a wavefront has lanes."""
    dout, y = _unit((2, 3, 8), 1), _unit((2, 3, 8), 2)
    dout[1, 2, 7] = PLANT
    y[1, 2, 7] = 0.5                                    # ReLU passes the gradient there
    dy = H.act_bn_bwd(dout, y, None, None, None, None, False, H.ACT_RELU)[0]
    assert torch.equal(H.row_amax_of(dy), dy.abs().amax((0, 2)))
    assert float(H._noted(dy, "_bm_amax").max()) == float(dy.abs().max()) == abs(PLANT)
