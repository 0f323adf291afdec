"""The regression objective on the MI355X: the L1 / MSE loss kernels against the live reference (fixture (a) of
tests/golden/regression.npz) and fp64 torch, training through the Solver against the reference (fixture (b)) and the
CPU oracle, and the test metrics against the reference's bm/metrics.py (fixture (c))."""
import copy

import pytest
import torch

from helpers import Golden, adam_params_close, close, is_noise_grad, rel_l2
from oracle import bm_oracle as O
from brainmagick_amd import synthetic

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 1e-4, 1e-4        # tests/test_model_gpu.py


def _g():
    return Golden("regression")


def _loss_cls(kind):
    from brainmagick_amd.losses import L1Loss, L2Loss
    return {"l1": L1Loss, "mse": L2Loss}[kind]


def _grads(kind, est, out, mask):
    e = est.detach().clone().cuda().requires_grad_(True)
    o = out.detach().clone().cuda().requires_grad_(True)
    loss = _loss_cls(kind)()(e, o, None if mask is None else mask.cuda())
    loss.backward()
    return loss.detach(), e.grad, o.grad


def _check_grad(kind, got, want, est, out):
    got, want = got.double().cpu(), want.double().cpu()
    if kind == "l1":          # sign(e - o) is not defined to 1e-6 where e ~ o
        keep = (est - out).abs() >= 1e-6
        got, want = got[keep], want[keep]
    assert (got - want).abs().max().item() <= 1e-6


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("form", ["none", "row", "full"])
def test_loss_kernels_against_the_reference(kind, form):
    g = _g()
    est, out = g.t("loss/est"), g.t("loss/out")
    mask = {"none": None, "row": g.t("loss/mask_row"), "full": g.t("loss/mask_full")}[form]
    loss, de, do = _grads(kind, est, out, mask)
    want = float(g.raw[f"loss/{kind}/{form}/loss"])
    assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)
    _check_grad(kind, de, g.t(f"loss/{kind}/{form}/grad_est"), est, out)
    _check_grad(kind, do, g.t(f"loss/{kind}/{form}/grad_out"), est, out)


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("B,F,T,t0,form", [(3, 5, 129, 0, "row"), (7, 13, 260, 17, "full"), (64, 120, 360, 0, "row"),
                                           (2, 1, 3, 0, "none")])
def test_loss_kernels_against_fp64_torch(kind, B, F, T, t0, form):
    """Vector (T % 4 == 0) and scalar paths, a time window (the Solver's offset slice), sizes that are no multiple of
    the workgroup."""
    gen = torch.Generator().manual_seed(B * 1000 + T)
    est = torch.randn(B, F, T, generator=gen)[..., t0:]
    out = torch.randn(B, F, T, generator=gen)[..., t0:]
    mask = None if form == "none" else \
        (torch.rand(B, 1 if form == "row" else F, T, generator=gen) > 0.3)[..., t0:]
    loss, de, do = _grads(kind, est, out, mask)
    e, o = est.double().requires_grad_(True), out.double().requires_grad_(True)
    sel = torch.ones_like(e, dtype=torch.bool) if mask is None else mask.expand_as(e)
    fn = torch.nn.L1Loss() if kind == "l1" else torch.nn.MSELoss()
    ref = fn(e[sel], o[sel])
    ref.backward()
    assert abs(float(loss) - ref.item()) <= 1e-6 * abs(ref.item())
    _check_grad(kind, de, e.grad, est, out)
    _check_grad(kind, do, o.grad, est, out)


def test_empty_mask_gives_nan_and_raises_the_flag_bit():
    from brainmagick_amd import hip_ops as H
    est, out = torch.randn(4, 3, 16, device="cuda"), torch.randn(4, 3, 16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss, count = H.regress_loss_fwd(est, out, torch.zeros(4, 1, 16, dtype=torch.bool, device="cuda"), "mse", flag)
    assert bool(torch.isnan(loss)) and float(count) == 0 and int(flag) == H.NO_MASK_BIT
    loss, count = H.regress_loss_fwd(est, out, None, "l1", flag)
    assert float(count) == 4 * 3 * 16 and bool(torch.isfinite(loss))


def test_same_call_twice_is_bit_identical():
    gen = torch.Generator().manual_seed(3)
    est, out = torch.randn(256, 120, 360, generator=gen), torch.randn(256, 120, 360, generator=gen)
    mask = torch.rand(256, 1, 360, generator=gen) > 0.2
    a = _grads("mse", est, out, mask)
    b = _grads("mse", est, out, mask)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_f16x2_backward_publishes_the_maxima_of_the_gradient():
    from brainmagick_amd import hip_ops as H
    if H.get_compute_dtype() != "f16x2":
        pytest.skip("BM_COMPUTE_DTYPE is not f16x2")
    gen = torch.Generator().manual_seed(5)
    est = torch.randn(32, 40, 96, generator=gen).cuda()
    out = torch.randn(32, 40, 96, generator=gen).cuda()
    mask = (torch.rand(32, 1, 96, generator=gen) > 0.5).cuda()
    loss, count = H.regress_loss_fwd(est, out, mask, "mse")
    before = H.amax_scans
    dest, _ = H.regress_loss_bwd(est, out, mask, "mse", torch.ones((), device="cuda"), count)
    slot, rows = H.amax(dest), H.row_amax_of(dest)
    assert H.amax_scans == before
    assert float(slot.max()) == float(dest.abs().max())
    assert torch.equal(rows, dest.abs().amax(dim=(0, 2)))


# ---- training ---------------------------------------------------------------------------------------------------------
def _wide_model(g, tag):
    import helpers as Hh
    from brainmagick_amd.models import SimpleConv
    d = Hh.WIDE_DIMS
    sb, features, ban_center, gen = Hh.wide_inputs()
    torch.manual_seed(d["seed"])
    model = SimpleConv(in_channels={"meg": d["C"]}, out_channels=d["F"], hidden={"meg": d["hidden"]},
                       n_subjects=d["S"], **Hh.WIDE_CFG)
    Hh.randomize_batchnorm(model, gen)
    for k, v in model.state_dict().items():
        assert (Hh.tensor_digest(v) == g.raw[f"train/{tag}/sd0_digest/{k}"]).all(), k
    assert (Hh.tensor_digest(sb.meg) == g.raw[f"train/{tag}/in_digest/meg"]).all()
    assert (Hh.tensor_digest(features) == g.raw[f"train/{tag}/in_digest/features"]).all()
    model.merger.ban_center_override = ban_center
    return model, sb


@pytest.mark.parametrize("tag", ["l2", "l1"])
def test_solver_trains_like_the_reference(tag):
    """Fixture (b): two Solver.train_step of the wide model (L2Loss with mask_loss under a partial [B, 1, T] mask, L1Loss
    unmasked) against the live reference: losses, step-0 gradients, the parameters after two Adam steps."""
    from brainmagick_amd.losses import L1Loss, L2Loss
    from brainmagick_amd.solver import Solver
    import helpers as Hh
    g = _g()
    p = f"train/{tag}/"
    model, sb = _wide_model(g, tag)
    sb.features_mask = g.t(p + "in/mask")
    solver = Solver(model, loss=L2Loss() if tag == "l2" else L1Loss(), mask_loss=tag == "l2")
    gscale = max(float(g.raw[k]) for k in g.raw if k.startswith(p + "grad_norm/"))
    for step in range(2):
        loss = solver.train_step(sb)
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
    bad = total = 0
    for k, prm in model.named_parameters():
        if float(g.raw[f"{p}grad_max/{k}"]) <= 1e-5 * gscale:
            continue
        idx = Hh.sample_indices(prm.numel())
        dlt = (prm.detach().flatten().cpu()[idx].double() - g.t(f"{p}sd1_sample/{k}").double()).abs()
        assert float(dlt.max()) <= 2.1 * 3e-4 * 2, k
        bad += int((dlt > 1e-6).sum())
        total += len(idx)
    assert bad <= 0.02 * total, (bad, total)


class _RegressionOracle(O.OracleModel):
    """The CPU oracle with the regression objective: MSE or L1 over est[mask.expand_as(est)] (bm/losses.py:11-26)."""

    def __init__(self, *a, mask=None, kind="mse", **kw):
        super().__init__(*a, **kw)
        self.mask = mask
        self.fn = {"mse": torch.nn.functional.mse_loss, "l1": torch.nn.functional.l1_loss}[kind]

    def loss_and_grads(self, meg, positions, subjects, candidates, training=True, ban_center=None,
                       update_buffers=True):
        for k in self.param_names:
            self.sd[k].requires_grad_(True)
            self.sd[k].grad = None
        new_buffers: dict = {}
        est = self.forward(meg, positions, subjects, training, ban_center, new_buffers)
        sel = self.mask.expand_as(est) if self.mask is not None else torch.ones_like(est, dtype=torch.bool)
        loss = self.fn(est[sel], candidates.to(self.dtype)[sel])
        loss.backward()
        grads = {k: self.sd[k].grad.detach().clone() for k in self.param_names if self.sd[k].grad is not None}
        for k in self.param_names:
            self.sd[k].requires_grad_(False)
            self.sd[k].grad = None
        if update_buffers:
            for k, v in new_buffers.items():
                self.sd[k] = v.detach()
        return loss.detach(), est.detach(), grads


def _partial_mask(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    mask = torch.ones(B, 1, T, dtype=torch.bool)
    for b in range(B):
        n = int(torch.randint(1, T // 2, (1,), generator=gen))
        s = int(torch.randint(0, T - n, (1,), generator=gen))
        mask[b, 0, s:s + n] = False
    return mask


def test_full_size_cfg2_mse_three_steps_against_the_oracle():
    """cfg2 at its full size (B = 256, F = 120 mel, T = 360): three Adam steps of L2Loss with mask_loss and a partial
    mask against the CPU oracle with the same objective."""
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _paper_model
    c = synthetic.CONFIGS["cfg2"]
    sb = synthetic.make_config_batch("cfg2", seed=2036)
    sb.features_mask = _partial_mask(len(sb.meg), c["T"], 11)
    model = _paper_model(c["C"], c["F"], c["S"], seed=2036)
    oracle = _RegressionOracle(copy.deepcopy(model.state_dict()), O.CLIP_CONV_CFG, 320, c["F"], mask=sb.features_mask)
    ban = torch.tensor([0.4, 0.6])
    model.merger.ban_center_override = ban
    solver = Solver(model, loss=L2Loss(), mask_loss=True)
    for step in range(3):
        loss = solver.train_step(sb)
        loss_ref, _, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index, sb.features, True,
                                                       ban)
        assert abs(float(loss) - float(loss_ref)) < LOSS_TOL * max(1.0, abs(float(loss_ref))), (step, float(loss),
                                                                                                 float(loss_ref))
        if step == 0:
            gscale = max(v.double().norm().item() for v in grads_ref.values())
            grads0 = grads_ref
            for k, p in model.named_parameters():
                tol = GRAD_TOL if p.dim() > 1 else 3 * GRAD_TOL
                assert close(p.grad, grads_ref[k], tol, gscale), (k, rel_l2(p.grad, grads_ref[k]))
        oracle.apply_adam(grads_ref)
    for k, p in model.named_parameters():
        if is_noise_grad(grads0[k], gscale):
            continue          # round-off-noise gradient (conv bias in front of a BatchNorm): Adam makes it +-lr
        ok, info = adam_params_close(p, oracle.sd[k], 3, g_ref=grads0[k], gscale=gscale)
        assert ok, (k, info)


def test_l1_two_steps_at_batch_64():
    """cfg2 at batch 64: two Adam steps of L1Loss (unmasked) against the CPU oracle with the same objective: the loss of
    both steps, every gradient of the first, the parameters after the second."""
    from brainmagick_amd.losses import L1Loss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _paper_model
    c = synthetic.CONFIGS["cfg2"]
    sb = synthetic.make_config_batch("cfg2", seed=5, batch=64)
    model = _paper_model(c["C"], c["F"], c["S"], seed=5)
    oracle = _RegressionOracle(copy.deepcopy(model.state_dict()), O.CLIP_CONV_CFG, 320, c["F"], kind="l1")
    ban = torch.tensor([0.3, 0.5])
    model.merger.ban_center_override = ban
    solver = Solver(model, loss=L1Loss())
    for step in range(2):
        loss = solver.train_step(sb)
        loss_ref, _, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index, sb.features, True,
                                                       ban)
        assert abs(float(loss) - float(loss_ref)) < LOSS_TOL * max(1.0, abs(float(loss_ref))), (step, float(loss),
                                                                                                 float(loss_ref))
        if step == 0:
            gscale = max(v.double().norm().item() for v in grads_ref.values())
            grads0 = grads_ref
            for k, p in model.named_parameters():
                tol = GRAD_TOL if p.dim() > 1 else 3 * GRAD_TOL
                assert close(p.grad, grads_ref[k], tol, gscale), (k, rel_l2(p.grad, grads_ref[k]))
        oracle.apply_adam(grads_ref)
    # after the second step: the rule of the consecutive-step tests (test_full_size_horizon_20_steps_against_oracle).
    # sign(e - o) of near-ties and the attention heads' near-cancelling gradients let Adam move single elements by
    # round-off-driven amounts; the tight statements are the losses of both steps and the step-0 gradients above
    lr = 3e-4
    for k, p in model.named_parameters():
        if is_noise_grad(grads0[k], gscale):
            continue          # round-off-noise gradient (conv bias in front of a BatchNorm): Adam makes it +-lr
        d = (p.detach().double().cpu() - oracle.sd[k].double()).abs()
        assert float((d > 2 * lr).double().mean()) <= 1e-2 and float(d.max()) <= 2.1 * lr * 2, (k, float(d.max()))
        assert float((d > 1e-6).double().mean()) <= 0.05, (k, float((d > 1e-6).double().mean()))


def test_world2_loopback_matches_joint_autograd():
    """sharded_step assumes nothing about ClipLoss: two replicas (loopback communicator) of an L2Loss step against the
    oracle run per rank, gradients averaged, one Adam step."""
    from loopback import run_replicas
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    world, B = 2, 6
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=48, initial_linear=48, depth=4, merger_dropout=0.0)
    C, T, Fd, S, hidden = 24, 96, 10, 3, 64

    def build():
        torch.manual_seed(1)
        return SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S, **cfg)

    sd0 = copy.deepcopy(build().state_dict())
    recordings = synthetic.make_layouts(2, [C], torch.Generator().manual_seed(4))
    batches = [synthetic.make_batch(B, C, T, Fd, S, seed=70 + r, recordings=recordings) for r in range(world)]
    for r, sb in enumerate(batches):
        sb.features_mask = _partial_mask(B, T, 20 + r)

    def body(r):
        model = build()
        solver = Solver(model, loss=L2Loss(), mask_loss=True)
        loss = float(solver.train_step(batches[r]))
        return loss, {k: v.detach().clone().cpu() for k, v in model.named_parameters()}

    res = run_replicas(world, body)
    oracles = [_RegressionOracle(copy.deepcopy(sd0), cfg, hidden, Fd, mask=batches[r].features_mask)
               for r in range(world)]
    per_rank = []
    for r in range(world):
        sb = batches[r]
        loss, _, grads = oracles[r].loss_and_grads(sb.meg, sb.positions(), sb.subject_index, sb.features, True)
        assert abs(res[r][0] - float(loss)) < LOSS_TOL, (r, res[r][0], float(loss))
        per_rank.append(grads)
    mean = {k: sum(gr[k] for gr in per_rank) / world for k in per_rank[0]}
    oracles[0].apply_adam(mean)
    gscale = max(v.double().norm().item() for v in mean.values())
    for k, p in res[0][1].items():
        assert torch.equal(p, res[1][1][k]), "replicas diverged"
        ok, info = adam_params_close(p, oracles[0].sd[k], 1, g_ref=mean[k], gscale=gscale)
        assert ok, (k, info)


def test_no_mask_assert_leaves_no_trace_in_the_solver_state():
    """bm/solver.py:354-356: a batch whose mask selects nothing raises AssertionError; the Solver continues exactly as
    if the batch had not existed (evaluated at the deferred check point, state put back by _rollback)."""
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _small_model

    def run(poison):
        model, _ = _small_model(merger_dropout=0.0)
        solver = Solver(model, loss=L2Loss(), mask_loss=True)
        good = [synthetic.make_batch(4, 20, 48, 10, 3, seed=10 + i) for i in range(2)]
        losses = [float(solver.train_step(good[0]))]
        if poison:
            empty = synthetic.make_batch(4, 20, 48, 10, 3, seed=99)
            empty.features_mask = torch.zeros_like(empty.features_mask)
            with pytest.raises(AssertionError, match="no mask"):
                solver.train_step(empty)
            assert solver._last_batch is good[0]
        losses.append(float(solver.train_step(good[1])))
        return losses, {k: v.clone() for k, v in model.state_dict().items()}

    clean_losses, clean_sd = run(False)
    losses, sd = run(True)
    assert losses == clean_losses, (losses, clean_losses)
    for k, v in sd.items():
        assert torch.equal(v, clean_sd[k]), k


def test_eval_step_raises_no_mask_at_once():
    from brainmagick_amd.losses import L1Loss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _small_model
    model, _ = _small_model()
    solver = Solver(model, loss=L1Loss(), mask_loss=True)
    sb = synthetic.make_batch(4, 20, 48, 10, 3, seed=1)
    assert bool(torch.isfinite(solver.eval_step(sb)))
    sb.features_mask = torch.zeros_like(sb.features_mask)
    with pytest.raises(AssertionError, match="no mask"):
        solver.eval_step(sb)


def test_deep_mel_with_l2_loss_trains_the_feature_model():
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.models import DeepMel
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _small_model
    model, _ = _small_model()
    torch.manual_seed(2)
    fm = DeepMel(10, 8, 2, 10, kernel=3, stride=1, dilation_growth=2, dilation_period=5, batch_norm=True,
                 activation_on_last=False, skip=True, glu_context=1, glu=2)
    before = {k: v.detach().clone() for k, v in fm.named_parameters()}
    solver = Solver(model, loss=L2Loss(), feature_model=fm)
    sb = synthetic.make_batch(4, 20, 48, 10, 3, seed=2)
    assert bool(torch.isfinite(solver.train_step(sb)))
    grads = [p.grad for p in fm.parameters()]
    assert all(g is not None for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0
    assert any(not torch.equal(p.detach().cpu(), before[k]) for k, p in fm.named_parameters())


# ---- metrics ----------------------------------------------------------------------------------------------------------
def test_metrics_against_the_reference():
    """Fixture (c): OnlineCorrelation, L2Reg, L1Reg over two recordings of three batches, partial mask, trim 5, at
    1e-10 relative (fp64)."""
    import json
    from brainmagick_amd import metrics as M
    g = _g()
    d = json.loads(str(g.raw["meta"]))["metric_shape"]
    ctors = [M.L2Reg.get_constructor(slice(None), slice(None), name="l2_feature"),
             M.OnlineCorrelation.get_constructor(slice(None), slice(None), name="corr_feature"),
             M.L1Reg.get_constructor(slice(None), slice(None), name="l1_feature")]
    results = {c().name: [] for c in ctors}
    for r in range(d["recordings"]):
        metrics = [c() for c in ctors]
        for i in range(d["batches"]):
            est = g.t(f"metrics/in/{r}/{i}/est").cuda()
            gt = g.t(f"metrics/in/{r}/{i}/gt").cuda()
            mask = g.t(f"metrics/in/{r}/{i}/mask").cuda()
            for metric in metrics:
                metric.update(est, gt, mask, t0=d["trim"])
        for metric in metrics:
            value = metric.get().cpu()
            want = g.t(f"metrics/get/{r}/{metric.name}")
            assert value.shape == want.shape
            assert (value - want).abs().max().item() <= 1e-10 * want.abs().max().item(), metric.name
            results[metric.name].append(value.float())
    for c in ctors:
        metric = c()
        want = float(g.raw[f"metrics/reduce/{metric.name}"])
        assert abs(metric.reduce(results[metric.name]) - want) <= 1e-6 * abs(want), metric.name


def test_update_all_shares_one_pass_and_never_counts_twice():
    """update_all: one kernel pass for the metrics of one pair of slices; a metric of that group updated on its own
    afterwards takes a private copy, so the others do not see its batch."""
    from brainmagick_amd import metrics as M
    gen = torch.Generator().manual_seed(8)
    batches = [(torch.randn(3, 4, 20, generator=gen).cuda(), torch.randn(3, 4, 20, generator=gen).cuda())
               for _ in range(3)]
    l2, corr = [c() for c in M.regression_metric_constructors("x")]
    M.update_all([l2, corr], *batches[0], None)
    M.update_all([l2, corr], *batches[1], None)
    l2.update(*batches[2], None)
    l2_ref, corr_ref = [c() for c in M.regression_metric_constructors("x")]
    for e, g in batches:
        l2_ref.update(e, g, None)
    for e, g in batches[:2]:
        corr_ref.update(e, g, None)
    assert torch.equal(l2.get(), l2_ref.get()) and torch.equal(corr.get(), corr_ref.get())


@pytest.mark.parametrize("mask_loss", [False, True])
def test_regression_test_metrics_end_to_end(mask_loss):
    """bm/play.py:get_test_metrics over two recordings with partial feature masks: the metrics see the batch's mask only
    under mask_loss, otherwise every sample (the reference's _process_batch hands torch.ones_like(features_mask) on).
    Expected values: torch fp64 on the model's estimates with the mask the test itself chooses."""
    from brainmagick_amd import metrics as M
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    from test_model_gpu import _small_model
    model, _ = _small_model()
    solver = Solver(model, loss=L2Loss(), mask_loss=mask_loss)
    recordings = [[synthetic.make_batch(4, 20, 48, 10, 3, seed=100 + 10 * r + i) for i in range(2)] for r in range(2)]
    for r, rec in enumerate(recordings):
        for i, sb in enumerate(rec):
            sb.features_mask = _partial_mask(4, 48, 30 + 2 * r + i)
            sb.features_mask[0] = True                 # every column keeps a sample
    got = M.regression_test_metrics(solver, recordings, trim_offset=6, metrics=M.regression_metric_constructors("mel"),
                                    reduce=False)
    assert set(got) == {"l2_mel", "corr_mel"}
    for r, rec in enumerate(recordings):         # the same by hand, torch fp64
        sums = None
        for sb in rec:
            est = solver.predict(sb)[0]
            m = (sb.features_mask if mask_loss else torch.ones(4, 1, 48, dtype=torch.bool))[..., 6:].double()
            e, t = est[..., 6:].double().cpu(), sb.features[..., 6:].double()
            part = [((e - t) * m).pow(2).sum(0), (e * t * m).sum(0), (e * m).sum(0), (t * m).sum(0),
                    (e * m).pow(2).sum(0), (t * m).pow(2).sum(0), m.expand_as(e).sum(0)]
            sums = part if sums is None else [a + b for a, b in zip(sums, part)]
        l2, dot, sl, sr, sll, srr, cnt = sums
        assert torch.allclose(got["l2_mel"][r].double(), (l2 / cnt), rtol=1e-5, atol=1e-7)
        nl = (sll - sl ** 2 / cnt).clamp(0).sqrt()
        nr = (srr - sr ** 2 / cnt).clamp(0).sqrt()
        corr = (dot - sl * sr / cnt) / (nl * nr).clamp(1e-8)
        assert torch.allclose(got["corr_mel"][r].double(), corr, rtol=1e-5, atol=1e-6)
    reduced = M.regression_test_metrics(solver, recordings, trim_offset=6, metrics=M.regression_metric_constructors("mel"))
    assert abs(reduced["l2_mel"] - float(got["l2_mel"].mean().sqrt())) < 1e-6
