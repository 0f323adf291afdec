"""The yardsticks of tests/test_bn_conditioning_gpu.py, proven before a kernel is judged by them (no GPU): the planted
ratios are the planned ones, the fp64 reference does not cancel, torch's own fp32 batch_norm -- what the reference project
runs -- stays inside the forward tolerance far up the ladder, and the CPU restatement of the project's one-pass algorithm
obeys |dvar| <= K * 2^-24 * (mean^2 + var) with a K that a tree sum of one stats tile explains."""
import math

import pytest
import torch
from torch.nn import functional as F

import bn_cases as BC
from test_alignment_gpu import STATS_TOL
from test_kernels_gpu import FWD_TOL, GRAD_TOL


def _cases():
    """name -> (fp32 tensor a producer's statistics are taken of, emulation arguments)."""
    out = {}
    for KS in (1, 3):
        c = BC.conv_case("same", seed=KS, KS=KS, **BC.NARROW)
        out[f"narrow KS={KS} (tile 128)"] = (c, dict(tile=BC.TILE_NARROW))
    c = BC.conv_case("same", seed=5, **BC.WIDE)
    out["wide (tile 96)"] = (c, dict(tile=BC.TILE_WIDE))
    c = BC.conv_case("strided", seed=6, **BC.STRIDED)
    out["strided (tile 128)"] = (c, dict(tile=BC.TILE_STRIDED))
    c = BC.conv_case("transposed", seed=7, **BC.STRIDED)
    out["transposed (tile 128 x 2 phases)"] = (c, dict(tile=BC.TILE_STRIDED, phases=BC.STRIDED["stride"]))
    c = BC.conv_case("same", seed=3, **BC.NARROW_DEEP)
    out["narrow, 144 partials (tile 128)"] = (c, dict(tile=BC.TILE_NARROW))
    c = BC.conv_case("same", seed=5, **BC.WIDE_DEEP)
    out["wide, 144 partials (tile 96)"] = (c, dict(tile=BC.TILE_WIDE))
    for B, C, T in BC.STATS_SHAPES + (BC.STATS_DEEP,):
        y = BC.ladder_tensor(B, C, T, seed=B)
        nsplit = 16 if B >= 64 else 4 if B >= 8 else 1
        out[f"channel_stats {B}x{C}x{T} ({nsplit} slabs)"] = (
            dict(pre64=y.double(), ratios=BC.realised_ratios(y), plan=BC.planned_ratios(C)),
            dict(tile=None, slabs=BC.stats_slabs(B, nsplit)))
    return out


CASES = _cases()


def test_the_constants_are_the_suites():
    assert (FWD_TOL, GRAD_TOL, STATS_TOL) == (5e-6, 2e-5, 1e-5)
    assert len(BC.LADDER) == 8 and BC.planned_ratios(24).tolist()[8:16] == [-float(r) for r in BC.LADDER]


@pytest.mark.parametrize("name", list(CASES))
def test_realised_ratios_are_the_planned_ones(name):
    case, _ = CASES[name]
    plan, got = case["plan"], case["ratios"]
    print(name, [f"{v:.4g}" for v in got.tolist()[:16]])
    for sign in (1, -1):
        for r in BC.LADDER:
            assert int((plan == sign * r).sum()) >= (1 if r else 2), (name, sign * r)     # both signs, r more than once
    assert int((plan.abs() == 1000).sum()) >= 2
    assert bool(((got - plan).abs() <= 0.02 * plan.abs().clamp_min(1.0)).all()), (name, (got - plan).abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_fp64_reference_does_not_cancel(name):
    """F.batch_norm in fp64 against a two-pass restatement (centre first, then square): 1e-12 per channel, at r = 1000
    as at r = 0; the running statistics with it."""
    case, _ = CASES[name]
    y32 = case["pre64"].float()
    ops = BC.chain_operands(y32.shape[1], y32.shape, 1)
    ref = BC.chain_reference(y32, ops["gamma"], ops["beta"], None, ops["dout"], "none", rm=ops["rm"], rv=ops["rv"])
    mean, var = BC.moments64(y32)
    two_pass = (y32.double() - mean[None, :, None]) / torch.sqrt(var + BC.BN_EPS)[None, :, None] \
        * ops["gamma"].double()[None, :, None] + ops["beta"].double()[None, :, None]
    assert float(BC.chan_err(ref["out"], two_pass).max()) < 1e-12
    rm = (1 - BC.BN_MOMENTUM) * ops["rm"].double() + BC.BN_MOMENTUM * mean
    rv = (1 - BC.BN_MOMENTUM) * ops["rv"].double() + BC.BN_MOMENTUM * ref["unbiased"]
    assert float((ref["rm"] - rm).abs().max()) < 1e-12 * 1000 and float(((ref["rv"] - rv) / rv).abs().max()) < 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_torch_fp32_batch_norm_holds_the_forward_tolerance_up_to_r_100(name):
    """What the reference project would show: nn.BatchNorm1d in fp32 does not cancel.  Held in rel-L2 PER CHANNEL (no
    channel hides behind another); the max-error metric of the GPU file is printed next to it: there plain fp32 itself
    arrives at the tolerance near r = 100 (one rounding of y * scale is 2^-24 r gamma of the channel's rms)."""
    case, _ = CASES[name]
    y32 = case["pre64"].float()
    ops = BC.chain_operands(y32.shape[1], y32.shape, 2)
    for act in ("none", "gelu"):
        r64 = BC.chain_reference(y32, ops["gamma"], ops["beta"], ops["res"], ops["dout"], act)
        r32 = BC.chain_reference(y32, ops["gamma"], ops["beta"], ops["res"], ops["dout"], act, dtype=torch.float32)
        err = BC.by_ladder(BC.chan_rel_l2(r32["out"], r64["out"]), case["plan"])
        print(f"{name} act={act} torch fp32 out, rel-L2:    {BC.fmt_ladder(err)}")
        emax = BC.by_ladder(BC.chan_err(r32["out"], r64["out"]), case["plan"])
        print(f"{name} act={act} torch fp32 out, max / rms: {BC.fmt_ladder(emax)}")
        assert all(e < FWD_TOL for r, e in err.items() if r <= 100), (name, act, err)


def tree_sum_K(n):
    """A bound on K for ONE fp32 tree sum of n terms of a channel at any r: the sum of squares carries at most
    (log2 n + 1) roundings of relative size 2^-24 (one for the square), the sum log2 n, and mean^2 doubles the sum's
    relative error: |dvar| <= 2^-24 ((log2 n + 1) E[y^2] + 2 log2 n mean^2) <= (3 log2 n + 1) 2^-24 (mean^2 + var)."""
    return 3 * math.log2(n) + 1


@pytest.mark.parametrize("name", list(CASES))
def test_emulation_obeys_the_law(name):
    """K_emu (printed: the GPU file computes the same on each producer's own output) is what a tree sum of one stats
    tile explains; the r at which the emulated chain leaves the tolerances is printed per tile width."""
    case, emu = CASES[name]
    y32 = case["pre64"].float()
    B, C, T = y32.shape
    parts = BC.emulated_partials(y32, **emu)
    _, _, _, var = BC.fold64(parts, B * T)
    K = BC.law_K(var, y32)
    longest = max(nb for _, nb in emu["slabs"]) * T if emu.get("slabs") else emu["tile"]
    print(f"{name}: K_emu = {float(K.max()):.3f}   by ladder: {BC.fmt_ladder(BC.by_ladder(K, case['plan']))}")
    assert float(K.max()) <= tree_sum_K(longest), (name, float(K.max()))
    ops = BC.chain_operands(C, y32.shape, 3)
    for act in ("none", "gelu"):
        got = BC.emulated_chain(y32, parts, ops["gamma"], ops["beta"], ops["res"], ops["dout"], act)
        ref = BC.chain_reference(y32, ops["gamma"], ops["beta"], ops["res"], ops["dout"], act)
        eo = BC.by_ladder(BC.chan_err(got["out"], ref["out"]), case["plan"])
        ed = BC.by_ladder(BC.chan_err(got["dy"], ref["dy"]), case["plan"])
        leaves = lambda e, tol: next((r for r in BC.LADDER if e[r] >= tol), None)       # noqa: E731
        print(f"{name} act={act} emulated out: {BC.fmt_ladder(eo)}  -> leaves FWD_TOL at r = {leaves(eo, FWD_TOL)}")
        print(f"{name} act={act} emulated dy:  {BC.fmt_ladder(ed)}  -> leaves GRAD_TOL at r = {leaves(ed, GRAD_TOL)}")
        assert eo[0] < FWD_TOL and ed[0] < GRAD_TOL           # at r = 0 the algorithm is plain fp32
        # the propagated law, on the emulation, where the GPU file applies it: above the ratios the tolerances cover
        bound, high = BC.out_bound(float(K.max()), y32), case["plan"].abs() >= 10
        assert bool((BC.chan_err(got["out"], ref["out"])[high] <= bound[high]).all()), name


DEEP = [n for n in CASES if "144 partials" in n or n.startswith(f"channel_stats {BC.STATS_DEEP[0]}x")]


@pytest.mark.parametrize("name", DEEP)
def test_an_fp32_fold_leaves_the_law_at_the_deep_shapes(name):
    """The power of the GPU file's check (b): the same partials added up in one fp32 running sum -- a split that is not
    folded in fp64, an epilogue that keeps summing across tiles -- land outside 4 x K_emu where a channel has ~150
    partials.  (With the 3 to 18 partials of the small shapes such a fold rounds a few times more and mostly stays
    inside, and a tile twice as wide moves K_emu by less than its channel-to-channel scatter: a tree sum's error
    grows with the logarithm of its length.  That is why the deep shapes are there.)"""
    case, emu = CASES[name]
    y32 = case["pre64"].float()
    n = y32.shape[0] * y32.shape[2]
    parts = BC.emulated_partials(y32, **emu)
    K_emu = float(BC.law_K(BC.fold64(parts, n)[3], y32).max())
    K32 = float(BC.law_K(BC.fold32(parts, n)[3], y32).max())
    print(f"{name}: {parts.shape[0]} partials, K_emu = {K_emu:.3f}, one fp32 running sum over them: K = {K32:.2f}")
    assert K32 > BC.LAW_SLACK * K_emu, (name, K32, K_emu)


def test_one_fp32_sum_per_channel_shows_in_K():
    """... and the constant grows with the length of the fp32 sums: the whole channel in ONE fp32 sum against
    128-column tiles, at 64 x 4096 samples per channel."""
    y32 = BC.ladder_tensor(64, 16, 4096, seed=9)
    n = 64 * 4096
    K = {}
    for tile, slabs in ((128, None), (None, [(0, 64)])):
        parts = BC.emulated_partials(y32, tile, slabs=slabs)
        K[tile] = float(BC.law_K(BC.fold64(parts, n)[3], y32).max())
    print(K)
    assert K[None] > BC.LAW_SLACK * K[128]
