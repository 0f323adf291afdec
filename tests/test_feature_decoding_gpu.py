"""FeatureDecodingLoss and ClassificationAcc on the MI355X: the fused kernels against the live reference (fixtures (a) and
(c) of tests/golden/feature_decoding.npz) and an fp64 torch restatement, non-finite inputs, the two deferred asserts,
determinism, and training through the Solver against the reference (fixture (b)).

Tolerances (the issue's): loss and per-feature terms 1e-6 relative (tests/test_regression_gpu.py's bound), gradients per
feature slice rel-L2 <= 1e-5 and max-abs error <= 1e-5 max|want| (FWD_TOL) -- the reference's own fp32 result lies within
3e-8 (loss) and 2.1e-7 (gradients) of fp64.  No absolute gradient bound: the gradients scale with 1 / count."""
import json
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from helpers import Golden, adam_params_close, rel_l2

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from make_feature_decoding_golden import CASES, STORED_BY_SEED, Builder, Weights, case_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 1e-4, 1e-4        # tests/test_model_gpu.py, tests/test_regression_gpu.py


def _g():
    return Golden("feature_decoding")


def _run(builder, est, out, mask, weights=None, flag=None):
    """(loss, terms, estimate.grad) of the HIP loss on the GPU."""
    from brainmagick_amd.losses import FeatureDecodingLoss
    loss_mod = FeatureDecodingLoss(builder, Weights(weights) if weights else None)
    loss_mod.no_mask_flag = flag
    e = est.detach().clone().cuda().requires_grad_(True)
    loss = loss_mod(e, out.cuda(), None if mask is None else mask.cuda())
    loss.backward()
    return loss.detach().cpu(), loss_mod.last_terms.cpu(), e.grad.cpu()


def _fp64(builder, est, out, mask, weights=None):
    """The reference's algorithm (bm/losses.py:127-173) in fp64 torch ops."""
    e, o = est.double().requires_grad_(True), out.double()
    sel = torch.ones(e.shape[0], 1, e.shape[2], dtype=torch.bool) if mask is None else mask
    terms = []
    for f in builder.values():
        fe, fo = e[:, builder.get_slice(f.name, model_output=True)], o[:, builder.get_slice(f.name)]
        if f.categorical:
            w = weights[f.name].double() if weights else None
            terms.append(F.cross_entropy(fe.transpose(1, 2)[sel[:, 0]], fo[:, 0][sel[:, 0]].long(), w))
        else:
            m = sel.expand_as(fe)
            terms.append(F.mse_loss(fe[m], fo[m]))
    loss = sum(terms)
    loss.backward()
    return loss.detach(), torch.stack([t.detach() for t in terms]), e.grad


def _check(builder, got, want, mask):
    (loss, terms, grad), (wloss, wterms, wgrad) = got, want
    print(f"loss {float(loss):.9g} want {float(wloss):.9g}")
    assert abs(float(loss) - float(wloss)) <= 1e-6 * abs(float(wloss)), (float(loss), float(wloss))
    for f, t, w in zip(builder.values(), terms.tolist(), wterms.tolist()):
        print(f"  term {f.name}: {t:.9g} want {w:.9g}")
        assert abs(t - w) <= 1e-6 * abs(w), (f.name, t, w)
    for f in builder.values():
        sl = builder.get_slice(f.name, model_output=True)
        a, b = grad[:, sl].double(), wgrad[:, sl].double()
        err, top = (a - b).abs().max().item(), b.abs().max().item()
        print(f"  grad {f.name}: rel_l2 {rel_l2(a, b):.3g} max-abs {err:.3g} of {top:.3g}")
        assert rel_l2(a, b) <= FWD_TOL, (f.name, rel_l2(a, b))
        assert err <= FWD_TOL * top, (f.name, err, top)
    if mask is not None:
        assert not grad[(~mask).expand_as(grad)].any(), "gradient at an unselected position"


def _fixture_case(g, case):
    builder, est, out, mask, _ = case_inputs(case)
    import helpers as Hh
    assert (Hh.tensor_digest(est) == g.raw[f"loss/{case}/est_digest"]).all()
    if case not in STORED_BY_SEED:
        est = g.t(f"loss/{case}/est")
    return builder, est, g.t(f"loss/{case}/out"), g.t(f"loss/{case}/mask")


@pytest.mark.parametrize("case,variant", [("mixed", "plain"), ("mixed", "weighted"), ("mixed", "plain_all"),
                                          ("mixed", "weighted_all"), ("cat_first", "plain"), ("cat_only", "plain"),
                                          ("reg_only", "plain")])
def test_loss_against_the_reference(case, variant):
    g = _g()
    builder, est, out, mask = _fixture_case(g, case)
    weights = {f.name: g.t(f"loss/{case}/weights/{f.name}") for f in builder.values() if f.categorical} \
        if variant.startswith("weighted") else None
    if weights:
        assert all(int((w == 0).sum()) == 1 for w in weights.values())        # one class of weight 0 each
    if variant.endswith("_all"):
        mask = torch.ones_like(mask)
    p = f"loss/{case}/{variant}/"
    want = (g.t(p + "loss"), g.t(p + "terms"), g.t(p + "grad"))
    _check(builder, _run(builder, est, out, mask, weights), want, mask)
    if variant == "plain_all":                        # mask=None means all true
        _check(builder, _run(builder, est, out, None, weights), want, None)


def _random_case(spec, B, T, t0, masked, weighted, seed):
    gen = torch.Generator().manual_seed(seed)
    builder = Builder(spec)
    est = (3 * torch.randn(B, builder.output_dimension, T, generator=gen))[..., t0:]
    out = torch.randn(B, builder.dimension, T, generator=gen)
    weights = {}
    for f in builder.values():
        if f.categorical:
            out[:, builder.get_slice(f.name)] = torch.randint(0, f.cardinality, (B, 1, T), generator=gen).float()
            weights[f.name] = torch.rand(f.cardinality, generator=gen) + 0.1
    out = out[..., t0:]
    mask = (torch.rand(B, 1, T, generator=gen) > 0.4)[..., t0:] if masked else None
    return builder, est, out, mask, (weights if weighted else None)


FP64_CASES = [
    # (B, T, t0, features, masked, weighted)
    (1, 3, 0, [("one", 1, 1)], False, False),                                            # K = 1: loss and gradient 0
    (1, 3, 0, [("seg", 1, 2), ("emb", 4, None)], True, False),                           # categorical first
    (3, 129, 0, [("emb", 3, None), ("hash", 1, 1025), ("aux", 2, None)], True, True),    # in the middle, K > 4 * 8 * n
    (3, 129, 0, [("a", 1, 3), ("emb", 2, None), ("b", 1, 41)], False, True),             # two categorical, first + last
    (7, 260, 17, [("emb", 5, None), ("hash", 1, 1025), ("seg", 1, 3)], True, False),     # a time window
    (64, 360, 0, [("ph", 1, 41), ("emb", 7, None), ("seg", 1, 2)], True, True),          # 360 workgroups
    (400, 360, 0, [("seg", 1, 3), ("emb", 2, None)], True, False),     # 2 250 tiles: forward workgroups take two
    (2920, 360, 0, [("emb", 2, None), ("seg", 1, 3)], True, False),    # 16 425 tiles: the backward's take two
]


@pytest.mark.parametrize("B,T,t0,spec,masked,weighted", FP64_CASES)
def test_loss_against_fp64_torch(B, T, t0, spec, masked, weighted):
    builder, est, out, mask, weights = _random_case(spec, B, T, t0, masked, weighted, seed=B * 1000 + T)
    _check(builder, _run(builder, est, out, mask, weights), _fp64(builder, est, out, mask, weights), mask)


# ---- extremes ---------------------------------------------------------------------------------------------------------
EXTREME_SPEC = [("emb", 2, None), ("ph", 1, 5)]


def _extreme_case():
    builder, est, out, mask, _ = _random_case(EXTREME_SPEC, 2, 70, 0, True, False, seed=9)
    mask[0, 0, 0] = mask[1, 0, 69] = True
    mask[0, 0, 1] = mask[1, 0, 3] = False
    return builder, est, out, mask


def test_huge_logits_stay_finite_and_equal_fp64():
    builder, est, out, mask = _extreme_case()
    est[:, 2 + 1] = 1e4
    est[:, 2 + 3] = -1e4
    got = _run(builder, est, out, mask)
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[2]).all())
    _check(builder, got, _fp64(builder, est, out, mask), mask)


def test_minus_infinity_off_and_on_target():
    builder, est, out, mask = _extreme_case()
    y = int(out[0, 2, 0])
    est[0, 2 + (y + 1) % 5, 0] = float("-inf")                 # off target: that class has probability 0
    got = _run(builder, est, out, mask)
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[2]).all())
    _check(builder, got, _fp64(builder, est, out, mask), mask)
    est[0, 2 + y, 0] = float("-inf")                           # on target: -log 0, as torch gives
    loss, terms, grad = _run(builder, est, out, mask)
    assert float(loss) == float("inf") and float(terms[1]) == float("inf") and bool(torch.isfinite(terms[0]))
    assert float(_fp64(builder, est, out, mask)[0]) == float("inf")


def test_nan_at_a_selected_position_gives_nan():
    builder, est, out, mask = _extreme_case()
    for channel in (0, 2 + 4):
        e = est.clone()
        e[1, channel, 69] = float("nan")
        assert bool(torch.isnan(_run(builder, e, out, mask)[0]))


def test_non_finite_values_at_unselected_positions_change_nothing():
    builder, est, out, mask = _extreme_case()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    clean = _run(builder, est, out, mask, flag=flag)
    e, o = est.clone(), out.clone()
    e[0, :, 1] = float("nan")
    e[1, 0, 3] = float("inf")
    e[1, 2:, 3] = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0, -1.0])
    o[0, :2, 1] = float("nan")
    o[1, 1, 3] = float("-inf")
    o[0, 2, 1] = float("nan")                                  # an unselected target: no class, no flag
    dirty = _run(builder, e, o, mask, flag=flag)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)
    assert int(flag) == 0


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flag_bits():
    from brainmagick_amd import hip_ops as H
    builder, est, out, mask = _extreme_case()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def bits(o, m):
        flag.zero_()
        loss = _run(builder, est, o, m, flag=flag)[0]
        return loss, int(flag)

    loss, got = bits(out, mask)
    assert got == 0 and bool(torch.isfinite(loss))                        # clean input sets nothing
    loss, got = bits(out, torch.zeros_like(mask))
    assert got == H.NO_MASK_BIT and bool(torch.isnan(loss))               # the reference's `assert mask.any()`
    o = out.clone()
    o[0, 2, 1] = 5.0                                                      # the class K at an UNSELECTED position
    want = _run(builder, est, out, mask)
    loss, got = bits(o, mask)
    assert got == H.CATEGORY_RANGE_BIT == 4 and torch.equal(loss, want[0])
    o = out.clone()
    o[0, 2, 0] = -1.0                                                     # a negative class at a selected position
    loss, got = bits(o, mask)
    assert got == H.CATEGORY_RANGE_BIT and bool(torch.isfinite(loss))     # ... which contributes nothing
    m = mask.clone()
    m[0, 0, 0] = False
    o[0, 2, 0] = 0.0
    terms = _run(builder, est, o, m)[1]
    flag.zero_()
    o[0, 2, 0] = -1.0
    assert torch.equal(_run(builder, est, o, mask, flag=flag)[1][1], terms[1])
    o[0, 2, 0] = -0.5                                                     # .long() truncates towards zero: class 0
    loss, got = bits(o, mask)
    assert got == 0


def test_launcher_refuses_tables_it_cannot_run():
    from brainmagick_amd import hip_ops as H
    est, out = torch.zeros(2, 6, 8, device="cuda"), torch.zeros(2, 3, 8, device="cuda")
    good = ((H.FEATURE_CONTINUOUS, 0, 2, 0, -1), (H.FEATURE_CATEGORICAL, 2, 4, 2, -1))
    assert bool(torch.isfinite(H.feature_decoding_fwd(est, out, None, good)[0]))
    for bad in (((H.FEATURE_CONTINUOUS, 0, 2, 0, -1),),                                   # does not span the channels
                ((H.FEATURE_CONTINUOUS, 0, 2, 0, -1), (H.FEATURE_CATEGORICAL, 3, 4, 2, -1)),    # a gap
                ((H.FEATURE_CONTINUOUS, 0, 2, 0, -1), (H.FEATURE_CATEGORICAL, 2, 4, 2, 0)),     # weights missing
                tuple((H.FEATURE_CONTINUOUS, i, 1, i, -1) for i in range(17))):
        with pytest.raises(H.BmHipError):
            H.feature_decoding_fwd(est, out, None, bad)
    wide = torch.zeros(1, 16385, 2, device="cuda")
    with pytest.raises(H.BmHipError, match="16384"):
        H.feature_decoding_fwd(wide, torch.zeros(1, 1, 2, device="cuda"), None, ((H.FEATURE_CATEGORICAL, 0, 16385, 0, -1),))


# ---- determinism and fill ---------------------------------------------------------------------------------------------
def test_same_call_twice_is_bit_identical():
    builder, est, out, mask, weights = _random_case([("emb", 6, None), ("ph", 1, 40), ("seg", 1, 3)], 256, 360, 0, True,
                                                    True, seed=3)
    a = _run(builder, est, out, mask, weights)
    b = _run(builder, est, out, mask, weights)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_backward_writes_every_element_of_a_nan_filled_buffer():
    """The caching allocator hands the block of a freed NaN-filled tensor to the backward's ``empty``: every element of
    dEst must be written (zeros where the mask does not select)."""
    builder, est, out, mask, _ = _random_case([("a", 1, 3), ("emb", 5, None), ("b", 1, 41)], 7, 131, 0, True, False, 5)
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import FeatureDecodingLoss
    e, o, m = est.cuda(), out.cuda(), mask.cuda()
    table, _ = FeatureDecodingLoss(builder, None)._plan()
    loss, terms, denoms, lse = H.feature_decoding_fwd(e, o, m, table)
    one = torch.ones((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()              # no other free block of this size: the next `empty` gets the poisoned one
    poison = torch.full_like(e, float("nan"))
    ptr = poison.data_ptr()
    del poison
    grad = H.feature_decoding_bwd(e, o, m, table, None, one, denoms, lse)
    assert grad.data_ptr() == ptr, "the allocator did not hand the poisoned block back"
    assert bool(torch.isfinite(grad).all())
    _check(builder, (loss.cpu(), terms.cpu(), grad.cpu()), _fp64(builder, est, out, mask), mask)


# ---- ClassificationAcc ------------------------------------------------------------------------------------------------
def test_classification_acc_against_the_reference():
    """Fixture (c): two recordings of three batches, K = 7, partial mask, trim 5: ratios of integer counts, equal."""
    from brainmagick_amd import metrics as M
    g = _g()
    d = json.loads(str(g.raw["meta"]))["metric_shape"]
    ctor = M.ClassificationAcc.get_constructor(slice(0, d["K"]), slice(0, 1), name="acc_ph")
    results = []
    for r in range(d["recordings"]):
        metric = ctor()
        for i in range(d["batches"]):
            metric.update(g.t(f"metrics/in/{r}/{i}/est").cuda(), g.t(f"metrics/in/{r}/{i}/gt").cuda(),
                          g.t(f"metrics/in/{r}/{i}/mask").cuda(), t0=d["trim"])
        value = metric.get().cpu()
        want = g.t(f"metrics/get/{r}/acc_ph")
        assert value.dtype == want.dtype == torch.float64 and value.shape == want.shape
        assert torch.equal(value, want)
        results.append(value.float())
    assert ctor().reduce(results) == float(g.raw["metrics/reduce/acc_ph"])


def test_classification_acc_ties_nan_window_and_fractional_targets():
    from brainmagick_amd import metrics as M
    est = torch.zeros(3, 4, 6)
    est[:, 2, 0] = est[:, 3, 0] = 1.0               # t = 0: a tie of classes 2 and 3 -> 2
    est[:, 1, 1] = float("nan")                     # t = 1: NaN counts as the maximum -> 1
    est[:, 3, 1] = 5.0
    est[:, 1, 2] = est[:, 2, 2] = float("nan")      # t = 2: the first NaN -> 1
    gt = torch.tensor([2., 1., 1., 0., 0.5, 3.]).repeat(3, 1)[:, None]        # t = 3: all equal -> 0; t = 4: 0.5 never hits
    gt[2, 0, 0] = 3.0                               # the second index of the tie is a miss
    mask = torch.ones(3, 1, 6, dtype=torch.bool)
    mask[1, 0, 3] = False
    acc = M.ClassificationAcc(slice(0, 4), slice(0, 1)).update(est.cuda(), gt.cuda(), mask.cuda())
    assert acc._acc.cpu().tolist() == [[2, 3, 3, 2, 0, 0], [3, 3, 3, 2, 3, 3]]
    want = torch.tensor([[2 / 3, 1., 1., 1., 0., 0.]], dtype=torch.float64)
    assert torch.equal(acc.get().cpu(), want)
    late = M.ClassificationAcc(slice(0, 4), slice(0, 1)).update(est.cuda(), gt.cuda(), None, t0=2)
    assert late._acc.cpu().tolist() == [[3, 3, 0, 0], [3, 3, 3, 3]]
    # slices of wider tensors are read in place
    wide_e, wide_g = torch.randn(3, 9, 6), torch.randn(3, 5, 6)
    wide_e[:, 5:9], wide_g[:, 2:3] = est, gt
    sliced = M.ClassificationAcc(slice(5, 9), slice(2, 3)).update(wide_e.cuda(), wide_g.cuda(), mask.cuda())
    assert torch.equal(sliced._acc, acc._acc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.update(est, gt, mask)


def test_update_all_takes_mixed_lists_and_get_before_update():
    from brainmagick_amd import metrics as M
    builder = Builder([("emb", 3, None), ("ph", 1, 5)])
    ctors = M.metric_constructors(builder)
    assert [c().name for c in ctors] == ["l2_emb", "corr_emb", "acc_ph"]
    assert ctors[2]().get().tolist() == [0.0]
    _, est, out, mask, _ = _random_case([("emb", 3, None), ("ph", 1, 5)], 6, 20, 0, True, False, seed=12)
    mask[0] = True
    est, out, mask = est.cuda(), out.cuda(), mask.cuda()
    together, alone = [c() for c in ctors], [c() for c in ctors]
    for _ in range(2):
        M.update_all(together, est, out, mask, 4)
        for m in alone:
            m.update(est, out, mask, t0=4)
    for a, b in zip(together, alone):
        assert torch.equal(a.get(), b.get()), a.name
    pred = est[:, 3:8, 4:].argmax(1, keepdim=True).cpu()
    m = mask[..., 4:].cpu()
    hits = ((pred == out[:, 3:4, 4:].cpu()) & m).sum(0).double()
    assert torch.equal(together[2].get().cpu(), hits / m.sum(0).double())


# ---- through the Solver -----------------------------------------------------------------------------------------------
SOLVER_SPEC = [("emb", 3, None), ("ph", 1, 5), ("seg", 1, 2)]         # 10 model outputs, 5 target channels


def _solver_batch(seed, T=48):
    from brainmagick_amd import synthetic
    builder = Builder(SOLVER_SPEC)
    sb = synthetic.make_batch(4, 20, T, builder.dimension, 3, seed=seed)
    _, _, out, mask, _ = _random_case(SOLVER_SPEC, 4, T, 0, True, False, seed=seed)
    mask[:, 0, 0] = True
    sb.features, sb.features_mask = out, mask
    return sb


def test_solver_raises_the_deferred_asserts_and_keeps_its_state():
    """An empty mask, the class K at an unselected position, the class -1 at a selected one: each raises
    AssertionError at the step's check point and leaves parameters, BatchNorm buffers and the last good batch as they
    were -- the next step continues exactly as if the batch had not existed."""
    from brainmagick_amd.losses import FeatureDecodingLoss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _small_model

    def poisoned(kind):
        sb = _solver_batch(99)
        if kind == "empty":
            sb.features_mask = torch.zeros_like(sb.features_mask)
        elif kind == "too_large":
            sb.features_mask[2, 0, 5] = False
            sb.features[2, 3, 5] = 5.0
        else:
            sb.features[1, 4, 0] = -1.0
        return sb

    def run(poison):
        model, _ = _small_model(merger_dropout=0.0)
        solver = Solver(model, loss=FeatureDecodingLoss(Builder(SOLVER_SPEC), None), mask_loss=True)
        good = [_solver_batch(10 + i) for i in range(2)]
        losses = [float(solver.train_step(good[0]))]
        for kind, match in poison:
            before = {k: v.clone() for k, v in model.state_dict().items()}
            with pytest.raises(AssertionError, match=match):
                solver.train_step(poisoned(kind))
            assert solver._last_batch is good[0]
            for k, v in model.state_dict().items():
                assert torch.equal(v, before[k]), (kind, k)
            with pytest.raises(AssertionError, match=match):
                solver.eval_step(poisoned(kind))
        losses.append(float(solver.train_step(good[1])))
        return losses, {k: v.clone() for k, v in model.state_dict().items()}

    clean_losses, clean_sd = run([])
    losses, sd = run([("empty", "no mask"), ("too_large", "bm/losses.py:150"), ("negative", "bm/losses.py:150")])
    assert losses == clean_losses, (losses, clean_losses)
    for k, v in sd.items():
        assert torch.equal(v, clean_sd[k]), k


def test_solver_trains_like_the_reference():
    """Fixture (b): two Solver.train_step of the wide model with the weighted loss under a partial mask against the live
    reference: losses, step-0 gradients, the parameters after two Adam steps (the rules of the regression training
    test)."""
    from brainmagick_amd.losses import FeatureDecodingLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    import helpers as Hh
    g = _g()
    p = "train/"
    d = Hh.WIDE_DIMS
    builder = Builder(CASES["mixed"])
    sb, _, ban_center, gen = Hh.wide_inputs()
    torch.manual_seed(d["seed"])
    model = SimpleConv(in_channels={"meg": d["C"]}, out_channels=builder.output_dimension, hidden={"meg": d["hidden"]},
                       n_subjects=d["S"], **Hh.WIDE_CFG)
    Hh.randomize_batchnorm(model, gen)
    for k, v in model.state_dict().items():
        assert (Hh.tensor_digest(v) == g.raw[f"{p}sd0_digest/{k}"]).all(), k
    assert (Hh.tensor_digest(sb.meg) == g.raw[p + "in_digest/meg"]).all()
    model.merger.ban_center_override = ban_center
    sb.features, sb.features_mask = g.t(p + "in/features"), g.t(p + "in/mask")
    weights = Weights({f.name: g.t(f"{p}in/weights/{f.name}") for f in builder.values() if f.categorical})
    solver = Solver(model, loss=FeatureDecodingLoss(builder, weights), mask_loss=True)
    gscale = max(float(g.raw[k]) for k in g.raw if k.startswith(p + "grad_norm/"))
    for step in range(2):
        loss = solver.train_step(sb)
        print(f"step {step}: loss {float(loss):.7f} want {g.raw[p + 'out/losses'][step]:.7f}")
        assert abs(float(loss) - g.raw[p + "out/losses"][step]) < LOSS_TOL, (step, float(loss))
        if step == 0:
            for k, prm in model.named_parameters():
                if float(g.raw[f"{p}grad_max/{k}"]) <= 1e-5 * gscale:
                    continue
                ref_norm = float(g.raw[f"{p}grad_norm/{k}"])
                gr = prm.grad.detach().flatten().cpu()
                assert abs(float(gr.double().norm()) - ref_norm) < GRAD_TOL * ref_norm, k
                idx = Hh.sample_indices(gr.numel())
                assert (gr[idx].double() - g.t(f"{p}grad_sample/{k}").double()).norm() < 5 * GRAD_TOL * ref_norm, k
    solver.check_pending_flags()
    got, want, g0 = [], [], []
    for k, prm in model.named_parameters():
        if float(g.raw[f"{p}grad_max/{k}"]) <= 1e-5 * gscale:
            continue          # round-off-noise gradient (conv bias in front of a BatchNorm): Adam makes it +-lr
        idx = Hh.sample_indices(prm.numel())
        got.append(prm.detach().flatten().cpu()[idx])
        want.append(g.t(f"{p}sd1_sample/{k}"))
        g0.append(g.t(f"{p}grad_sample/{k}"))
    ok, info = adam_params_close(torch.cat(got), torch.cat(want), 2, g_ref=torch.cat(g0), gscale=gscale)
    assert ok, info
