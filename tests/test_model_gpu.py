"""End-to-end parity of the HIP SimpleConv + ClipLoss + fused Adam step (through the C-ABI) against
(a) the golden vectors produced by the live reference and (b) the CPU oracle on cfg-shaped
synthetic batches.  fp32 tolerances: forward rel-L2 <= 1e-5, gradients <= 1e-4,
step-0 loss |delta| <= 1e-4."""
import copy
import os

import pytest
import torch

from helpers import (Golden, MODEL_FIXTURES, OFF_PATH_FIXTURES, adam_params_close, close, is_noise_grad, rel_l2,
                     running_stat_close)
from oracle import bm_oracle as O
from brainmagick_amd import synthetic

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
LOSS_TOL = 1e-4


PARITY_NOISE = 2.5      # planted-noise level of the long-horizon parity run (calibrated: top-10 far from 0 % and 100 %)


class _Batch:
    def __init__(self, meg, subjects, recordings):
        self.meg = meg
        self.subject_index = subjects
        self._recordings = recordings

    def __len__(self):
        return len(self.meg)


def _batch_from_positions(meg, positions, subjects):
    """Rebuild per-sample recordings from a [B, C, 2] position tensor (golden fixtures)."""
    recs, seen = [], {}
    for i in range(len(meg)):
        key = positions[i].numpy().tobytes()
        if key not in seen:
            seen[key] = synthetic.Recording(len(seen), positions[i].clone())
        recs.append(seen[key])
    return _Batch(meg, subjects, recs)


def _build(meta, sd0):
    from brainmagick_amd.models import SimpleConv
    model = SimpleConv(in_channels={"meg": meta["C"], **meta.get("extra_inputs", {})}, out_channels=meta["F"],
                       hidden={"meg": meta["hidden"], **meta.get("extra_hidden", {})}, n_subjects=meta["S"],
                       **meta["cfg"])
    missing = model.load_state_dict(sd0, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.cuda()


@pytest.mark.parametrize("name", MODEL_FIXTURES + OFF_PATH_FIXTURES)
def test_against_reference_golden(name):
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.optim import FlatAdam
    g = Golden(name)
    meta = g.meta
    inp = g.group("in")
    model = _build(meta, g.group("sd0"))
    loss_mod = ClipLoss().cuda()
    batch = _batch_from_positions(inp["meg"].cuda(), inp["positions"], inp["subjects"].cuda())
    cand = inp["candidates"].cuda()
    mask = torch.ones(len(inp["meg"]), 1, meta["T"], dtype=torch.bool, device="cuda")
    extras = {k: inp[k].cuda() for k in meta.get("extra_inputs", {})}
    if model.merger is not None:
        model.merger.ban_center_override = inp["ban_center"]
    if getattr(model, "dropout", None) is not None:
        model.dropout.ban_center_override = inp["ban_center"]       # the fixture pinned every random centre to it
    ref_losses = g.raw["out/losses"]
    if meta["training"] and meta["n_steps"]:
        model.train()
        loss_mod.train()
        names = [k for k, _ in model.named_parameters()]
        optim = FlatAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.999))
        grads_ref = g.group("grad")
        gscale = max(v.double().norm().item() for v in grads_ref.values())
        for step in range(meta["n_steps"]):
            est = model({"meg": batch.meg.clone(), **extras}, batch)
            loss = loss_mod(est, cand, mask)
            optim.zero_grad()
            loss.backward()
            if step == 0:
                assert rel_l2(est, g.t("out/estimate")) < FWD_TOL
                params = dict(model.named_parameters())
                for k in names:
                    assert close(params[k].grad, grads_ref[k], GRAD_TOL, gscale), \
                        (k, rel_l2(params[k].grad, grads_ref[k]))
            assert abs(float(loss) - ref_losses[step]) < LOSS_TOL
            if "out/training_penalty" in g.raw and model.merger is not None:
                assert abs(float(model.merger.training_penalty) - float(g.raw["out/training_penalty"])) < 1e-6
            optim.step()
        sd1 = g.group("sd1")
        for k, v in model.state_dict().items():
            if k in grads_ref and is_noise_grad(grads_ref[k], gscale):
                continue
            if not v.is_floating_point():
                assert int(v) == int(sd1[k]), k
            elif k in grads_ref:
                ok, info = adam_params_close(v, sd1[k], meta["n_steps"], grads_ref[k], gscale)
                assert ok, (k, info)
            else:
                assert running_stat_close(v, sd1[k], meta["n_steps"]), k
    else:
        model.eval()
        loss_mod.eval()
        with torch.no_grad():
            est = model({"meg": batch.meg.clone(), **extras}, batch)
            loss = loss_mod(est, cand, mask)
            probs = loss_mod.get_probabilities(est, cand)
        assert rel_l2(est, g.t("out/estimate")) < FWD_TOL
        assert abs(float(loss) - ref_losses[0]) < LOSS_TOL
        assert rel_l2(probs, g.t("out/probabilities")) < 1e-5


def test_wide_kernels_against_reference_golden():
    """The headline wide f16x2 kernels held to the LIVE reference directly (not through the oracle): two training steps
    of the smallest model they cover (hidden 256, depth 4, 64 sensors, T = 192, batch 8; fixture
    tests/golden/wide_kernels_train.npz, parameters and inputs rebuilt from the seed and checked against the fixture's
    digests).  The launch labels of step 0 assert that the convs and weight gradients DID run in `conv_nn_h2w` /
    `gemm_nt_h2w`."""
    import helpers as Hh
    from test_oracle_golden import _wide_setup
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.optim import FlatAdam
    g, sb, candidates, ban_center, model = _wide_setup()
    d = Hh.WIDE_DIMS
    model = model.cuda()
    model.merger.ban_center_override = ban_center
    loss_mod = ClipLoss().cuda()
    batch = _Batch(sb.meg.cuda(), sb.subject_index.cuda(), sb._recordings)
    cand = candidates.cuda()
    mask = torch.ones(d["B"], 1, d["T"], dtype=torch.bool, device="cuda")
    model.train()
    loss_mod.train()
    optim = FlatAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.999))
    gscale = max(float(g.raw[k]) for k in g.raw if k.startswith("grad_norm/"))
    ref_losses = g.raw["out/losses"]
    for step in range(2):
        timer = H.KernelTimer() if step == 0 else None
        H.set_kernel_timer(timer)
        try:
            est = model({"meg": batch.meg.clone()}, batch)
            loss = loss_mod(est, cand, mask)
            optim.zero_grad()
            loss.backward()
        finally:
            H.set_kernel_timer(None)
        if step == 0:
            labels = [r[0] for r in timer.records]
            big = [r[0] for r in timer.records if r[1] >= 1e9]
            n_conv = sum(lb.startswith("conv_nn_h2w_kernel") for lb in labels)
            n_wg = sum(lb.startswith("gemm_nt_h2w_kernel") for lb in labels)
            # forward + data-gradient convs of the stack (4 + 2 GLU) and the front end / head; their weight gradients
            assert n_conv >= 2 * 6 and n_wg >= 6, sorted(set(labels))
            assert big and all(lb.startswith(("conv_nn_h2w_kernel", "gemm_nt_h2w_kernel")) for lb in big), sorted(set(big))
            assert rel_l2(est, g.t("out/estimate")) < FWD_TOL
            for k, p in model.named_parameters():
                ref_norm = float(g.raw[f"grad_norm/{k}"])
                if float(g.raw[f"grad_max/{k}"]) <= 1e-5 * gscale:
                    continue                      # round-off noise in the reference itself (conv bias before BatchNorm)
                gr = p.grad.detach().flatten().cpu()
                assert abs(float(gr.double().norm()) - ref_norm) < GRAD_TOL * ref_norm, k
                idx = Hh.sample_indices(gr.numel())
                assert (gr[idx].double() - g.t(f"grad_sample/{k}").double()).norm() < 5 * GRAD_TOL * ref_norm, \
                    (k, float((gr[idx].double() - g.t(f"grad_sample/{k}").double()).norm()), ref_norm)
        assert abs(float(loss) - ref_losses[step]) < LOSS_TOL, (step, float(loss), ref_losses[step])
        optim.step()
    # the sampled parameters after two Adam steps: an element may flip the sign of a noise-level first update
    # (adam_params_close), everything else agrees tightly
    lr, bad, total = 3e-4, 0, 0
    for k, p in model.named_parameters():
        if float(g.raw[f"grad_max/{k}"]) <= 1e-5 * gscale:
            continue
        idx = Hh.sample_indices(p.numel())
        dlt = (p.detach().flatten().cpu()[idx].double() - g.t(f"sd1_sample/{k}").double()).abs()
        assert float(dlt.max()) <= 2.1 * lr * 2, k
        bad += int((dlt > 1e-6).sum())
        total += len(idx)
    assert bad <= 0.02 * total, (bad, total)


@pytest.mark.parametrize("tag,kw", [("plain", {}), ("pool", dict(pool=True)),
                                    ("center", dict(center=True)), ("trim", None)])
def test_clip_loss_options_against_golden(tag, kw):
    from brainmagick_amd.losses import ClipLoss
    g = Golden("clip_loss")

    class DsetArgs:
        tmin = -0.5
        sample_rate = 20
    if kw is None:
        kw = dict(tmin=-0.2, tmax=0.9, dset_args=DsetArgs())
    mod = ClipLoss(**kw).cuda().eval()
    est = g.t("in/estimate").cuda().requires_grad_(True)
    cand = g.t("in/candidate").cuda()
    loss = mod(est, cand, torch.ones(5, 1, 33, dtype=torch.bool, device="cuda"))
    loss.backward()
    assert abs(float(loss) - float(g.raw[f"{tag}/loss"])) < 1e-5
    assert rel_l2(est.grad, g.t(f"{tag}/grad_estimate")) < GRAD_TOL
    assert rel_l2(mod.get_scores(est.detach(), cand), g.t(f"{tag}/scores")) < FWD_TOL
    assert rel_l2(mod.get_probabilities(est.detach(), cand), g.t(f"{tag}/probabilities")) < 1e-5


def _paper_model(C, F, S, seed=0):
    from brainmagick_amd.models import SimpleConv
    torch.manual_seed(seed)
    return SimpleConv(in_channels={"meg": C}, out_channels=F, hidden={"meg": 320}, n_subjects=S,
                      **O.CLIP_CONV_CFG)


@pytest.mark.parametrize("cfg_name,B,T", [("cfg2", 8, 360), ("cfg5", 6, 343), ("cfg1", 4, 361), ("cfg2", 3, 777),
                                          ("cfg2", 5, 130)])
def test_paper_model_step_against_oracle(cfg_name, B, T):
    """Full clip_conv architecture (9-16 M parameters) at reduced batch vs the CPU oracle: loss,
    estimate, every gradient, and the parameters after two Adam steps."""
    from brainmagick_amd.solver import Solver
    c = synthetic.CONFIGS[cfg_name]
    Fd = min(c["F"], 160)
    sb = synthetic.make_batch(B, c["C"], T, Fd, c["S"], seed=2036, mixed_eeg=cfg_name == "cfg5",
                              n_layouts=4 if cfg_name == "cfg1" else 1)
    model = _paper_model(c["C"], Fd, c["S"])
    sd0 = copy.deepcopy(model.state_dict())
    oracle = O.OracleModel(sd0, O.CLIP_CONV_CFG, 320, Fd)
    ban = torch.tensor([0.3, 0.7])
    model.merger.ban_center_override = ban
    solver = Solver(model)
    pos = sb.positions()
    noise = set()
    for step in range(2):
        loss_ref, est_ref, grads_ref = oracle.train_step(sb.meg, pos, sb.subject_index, sb.features,
                                                         ban)
        loss = solver.train_step(sb)
        assert abs(float(loss) - float(loss_ref)) < LOSS_TOL, (step, float(loss), float(loss_ref))
        gscale = max(v.double().norm().item() for v in grads_ref.values())
        noise |= {k for k, v in grads_ref.items() if is_noise_grad(v, gscale)}
        if step == 0:
            for k, p in model.named_parameters():
                assert close(p.grad, grads_ref[k], GRAD_TOL, gscale), (k, rel_l2(p.grad, grads_ref[k]))
    for k, v in model.state_dict().items():
        if k in noise:
            continue
        if not v.is_floating_point():
            continue
        if k in grads_ref:
            ok, info = adam_params_close(v, oracle.sd[k], 2, grads_ref[k], gscale)
            assert ok, (k, info)
        else:
            assert running_stat_close(v, oracle.sd[k], 2), k


@pytest.mark.parametrize("cfg_name,B", [("cfg2", 256), ("cfg3", 256), ("cfg5", 64), ("cfg5", 256), ("cfg2", 173)])
def test_full_size_step_against_oracle(cfg_name, B):
    """BASELINE.json configs[1] / configs[2] at their FULL size (batch 256, F = 120 / 1024; and cfg2 at 173 segments,
    the ragged last batch of an epoch: B * T is no multiple of any tile width) and the mixed
    MEG/EEG config (273 sensors, 115 subjects, two layouts) at batch 64 (layer-by-layer front end: more (layout,
    subject) pairs than segments) and at batch 256 (composed front end over 230 pairs): loss, estimate and every
    gradient of one training step against the CPU oracle (the oracle needs ~15 s per config on the GPU
    box's host cores).  Same tolerances as the reduced-size tests, except the 1-D parameters (biases,
    BatchNorm affine): their gradients are plain sums over B*T = 92 160 samples, where the fp32
    oracle's own summation order is worth ~2e-4 (measured round 1: 1.7e-4 on final.2.bias)."""
    from brainmagick_amd.solver import Solver
    c = synthetic.CONFIGS[cfg_name]
    sb = synthetic.make_config_batch(cfg_name, seed=2036, batch=B)
    model = _paper_model(c["C"], c["F"], c["S"], seed=2036)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), O.CLIP_CONV_CFG, 320, c["F"])
    ban = torch.tensor([0.4, 0.6])
    model.merger.ban_center_override = ban
    solver = Solver(model)
    loss = solver.train_step(sb)
    est = solver.predict(sb)[0]            # eval-mode forward of the updated model: finite, right shape
    assert est.shape == (B, c["F"], c["T"]) and bool(torch.isfinite(est).all())
    loss_ref, est_ref, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index,
                                                         sb.features, True, ban)
    assert abs(float(loss) - float(loss_ref)) < LOSS_TOL, (float(loss), float(loss_ref))
    gscale = max(v.double().norm().item() for v in grads_ref.values())
    worst = (0.0, "")
    for k, p in model.named_parameters():
        tol = GRAD_TOL if p.dim() > 1 else 3 * GRAD_TOL
        assert close(p.grad, grads_ref[k], tol, gscale), (k, rel_l2(p.grad, grads_ref[k]))
        if not is_noise_grad(grads_ref[k], gscale):
            worst = max(worst, (rel_l2(p.grad, grads_ref[k]), k))
    print(f"full-size {cfg_name} B={B}: loss {float(loss):.7f} vs oracle {float(loss_ref):.7f}, "
          f"worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("cfg_name,steps", [("cfg2", 20), ("cfg3", 10), ("cfg5", 10)])
def test_full_size_horizon_20_steps_against_oracle(cfg_name, steps):
    """The paper model at FULL size (batch 256, T = 360) for 20 (cfg2: 9 M parameters, mel features) / 10 (cfg3: the
    640 -> 1024 head and the K = 368 640 score contraction; cfg5: 273 sensors, two layouts, 115 subjects = 230 (layout,
    subject) groups, 16 M parameters) consecutive Adam steps on a stream of 4 distinct batches, side by side with the CPU
    oracle from the same initial state: the loss of EVERY step within LOSS_TOL (1e-4 absolute), i.e. drift that only
    shows at depth 10 with BatchNorm over 92 160 samples would show here.  After the last step: BatchNorm running
    statistics and the parameters (Adam's +-lr noise moves on round-off-level gradients excepted, see
    adam_params_close).  ~6 s of host time per oracle step on 32 threads."""
    from brainmagick_amd.solver import Solver
    c = synthetic.CONFIGS[cfg_name]
    # one study: the recordings (and their sensor layouts) are shared by the batches, like in a real training stream
    # (the layouts of a recording are cached by its identity, bm/models/common.py:196-222 does the same)
    if cfg_name == "cfg5":
        pool = synthetic.make_layouts(2, [c["C"], 128], torch.Generator().manual_seed(7))
    else:
        pool = synthetic.make_layouts(4, [c["C"]], torch.Generator().manual_seed(7))
    batches = [synthetic.make_config_batch(cfg_name, seed=2036 + i, batch=256, recordings=pool) for i in range(4)]
    model = _paper_model(c["C"], c["F"], c["S"], seed=2036)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), O.CLIP_CONV_CFG, 320, c["F"])
    ban = torch.tensor([0.4, 0.6])
    model.merger.ban_center_override = ban
    solver = Solver(model)
    dev_batches = [sb.to(solver.device) for sb in batches]
    prev = torch.get_num_threads()
    torch.set_num_threads(min(32, os.cpu_count() or prev))
    gaps, noise, grads_ref, gscale = [], set(), None, 1.0
    try:
        for step in range(steps):
            sb = batches[step % 4]
            loss = solver.train_step(dev_batches[step % 4])
            loss_ref, _, grads_ref = oracle.train_step(sb.meg, sb.positions(), sb.subject_index, sb.features, ban)
            gaps.append(abs(float(loss) - float(loss_ref)))
            assert gaps[-1] < LOSS_TOL, (step, float(loss), float(loss_ref), gaps)
            gscale = max(v.double().norm().item() for v in grads_ref.values())
            noise |= {k for k, v in grads_ref.items() if is_noise_grad(v, gscale)}
    finally:
        torch.set_num_threads(prev)
    print(f"full-size horizon {cfg_name}: {steps} steps, largest loss gap {max(gaps):.2e} (last loss {float(loss):.6f})")
    # the state after 20 steps.  The per-step losses above are the tight statement (step k + 1's loss sees step k's
    # update); element-wise, 20 Adam steps amplify every round-off-level gradient component into +-lr moves of either
    # sign (adam_params_close), so the parameters are held to: at most 1 % of a tensor's elements further apart than
    # two such moves, nothing further than every step flipping, and the tensor as a whole within 1e-3 (rel-L2) of the
    # distance it travelled
    lr = 3e-4
    worst = (0.0, "")
    for k, v in model.state_dict().items():
        if k in noise or not v.is_floating_point():
            continue
        ref = oracle.sd[k].double()
        d = (v.detach().double().cpu() - ref).abs()
        if k in grads_ref:
            assert float((d > 2 * lr).double().mean()) <= 1e-2 and float(d.max()) <= 2.1 * lr * steps, \
                (k, float((d > 2 * lr).double().mean()), float(d.max()))
            worst = max(worst, (rel_l2(v, ref), k))
        elif k.endswith("running_mean"):
            # the batch mean carries the conv bias in front of the BatchNorm, whose gradient is analytically zero and
            # whose Adam moves are therefore +-lr noise of either sign (is_noise_grad): up to 2 lr per step of drift
            assert float(d.max()) <= 2.1 * lr * steps, (k, float(d.max()))
        else:
            assert rel_l2(v, ref) < 1e-3, (k, rel_l2(v, ref))
    print(f"full-size horizon {cfg_name}: worst parameter rel-L2 after {steps} steps {worst[0]:.2e} ({worst[1]})")


def test_offset_meg_ms_slicing_like_the_reference():
    """bm/solver.py:262-274 with conf/config.yaml task.offset_meg_ms=150 at 120 Hz: the MEG window drops
    its first 18 samples, features and mask drop their last 18 (361 -> 343 samples)."""
    from brainmagick_amd.solver import Solver
    model, cfg = _small_model()
    T, off = 361, int(150 / 1000 * 120)
    assert off == 18
    sb = synthetic.make_batch(4, 20, T, 10, 3, seed=21)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), cfg, 32, 10)
    ban = torch.tensor([0.2, 0.3])
    model.merger.ban_center_override = ban
    solver = Solver(model, offset_meg_ms=150., sample_rate=120.)
    estimate, output, features_mask, reject_mask = solver._process_batch(sb, training=True)
    assert estimate.shape == (4, 10, T - off) and output.shape == (4, 10, T - off)
    assert features_mask.shape == (4, 1, T - off) and bool(reject_mask.all())
    assert torch.equal(output.cpu(), sb.features[..., :-off])
    loss = solver.train_step(sb)
    loss_ref, est_ref, grads_ref = oracle.loss_and_grads(
        sb.meg[..., off:].contiguous(), sb.positions(), sb.subject_index,
        sb.features[..., :-off].contiguous(), True, ban)
    assert rel_l2(estimate, est_ref) < FWD_TOL
    assert abs(float(loss) - float(loss_ref)) < LOSS_TOL
    gscale = max(v.double().norm().item() for v in grads_ref.values())
    for k, p in model.named_parameters():
        assert close(p.grad, grads_ref[k], GRAD_TOL, gscale), (k, rel_l2(p.grad, grads_ref[k]))


def test_out_of_range_subject_index_raises_like_the_reference_gather():
    """bm/models/common.py:57 gathers `weights[subjects]`: an index outside the table raises.  Here the
    device-side check clamps (no out-of-bounds read) and flags; the error surfaces at the Solver's
    next synchronisation point (or immediately under BM_CHECK_INDICES=1)."""
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.solver import Solver
    model, cfg = _small_model()
    sb = synthetic.make_batch(4, 20, 32, 10, 3, seed=5)
    solver = Solver(model)
    solver.train_step(sb)
    H.raise_if_index_error("cuda")                     # clean
    bad = sb.replace(subject_index=torch.tensor([0, 1, 7, 2]))
    solver.train_step(bad)                             # 7 >= 3 subjects: flagged, not read out of bounds
    with pytest.raises(IndexError):
        solver.train_step(sb)                          # reported at the next step's sync point
    solver.train_step(sb)                              # flag was cleared


def test_deferred_asserts_of_the_last_step_are_not_lost():
    """the ClipLoss mask assert (bm/losses.py:110) and the index check of a step ride on the device-side
    flag word that the NEXT step reads -- the last step of a run has no next one: `check_pending_flags()` (also called
    by eval_step / predict / state_dict) reports it, and raising one condition leaves the other pending."""
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.solver import Solver
    model, cfg = _small_model()
    sb = synthetic.make_batch(4, 20, 32, 10, 3, seed=5)
    solver = Solver(model)
    solver.train_step(sb)
    solver.check_pending_flags()                        # clean
    holes = sb.replace(features_mask=sb.features_mask.clone())
    holes.features_mask[1, 0, 3] = False
    solver.train_step(holes)                            # the optimizer step is taken; the verdict is on the device
    with pytest.raises(AssertionError, match="mask"):
        solver.check_pending_flags()
    solver.check_pending_flags()                        # reported once
    with pytest.raises(AssertionError, match="mask"):
        solver.eval_step(holes)                         # an evaluation loop reads its own step
    # an index error raised through hip_ops leaves a pending mask verdict alone
    bad = holes.replace(subject_index=torch.tensor([0, 1, 7, 2]))
    solver.train_step(bad)
    with pytest.raises(IndexError):
        H.raise_if_index_error("cuda")
    with pytest.raises(AssertionError, match="mask"):
        solver.check_pending_flags()


def test_node_negatives_accept_per_rank_rejection_with_constant_candidates():
    """Whole-node negatives next to a ScaleReject that can reject (round 4: equal blocks of the nominal batch size,
    padding rows masked -- test_replicas_with_per_rank_rejection_and_whole_node_negatives); still refused with a
    LEARNABLE feature model, whose autograd-aware gather needs equal blocks of real candidates."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.models import DeepMel
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    model, cfg = _small_model()
    scaler = DeviceBatchScaler(torch.zeros(2, 20), torch.ones(2, 20))
    assert Solver(model, negatives="node", scale_reject=ScaleReject(scaler, limit=16, clip=False))._ragged_node
    assert not Solver(model, negatives="node", scale_reject=ScaleReject(scaler, limit=16, clip=True))._ragged_node
    fm = DeepMel(10, 8, 2, 10, kernel=3, stride=1, dilation_growth=2, dilation_period=5, batch_norm=True,
                 activation_on_last=False, skip=True, glu_context=1, glu=2)
    with pytest.raises(ValueError):
        Solver(model, negatives="node", feature_model=fm, scale_reject=ScaleReject(scaler, limit=16, clip=False))


def test_flat_adam_is_a_torch_optimizer_and_checkpoints_round_trip():
    """bm/solver.py:64,115-117 put optimizer.state_dict() into the checkpoint and load it back."""
    from brainmagick_amd.solver import Solver
    model, cfg = _small_model(merger_dropout=0.0)      # no random sensor ban: two solvers must agree bitwise
    sb = synthetic.make_batch(4, 20, 32, 10, 3, seed=5)
    solver = Solver(model)
    assert isinstance(solver.optimizer, torch.optim.Optimizer)
    for _ in range(3):
        solver.train_step(sb)
    sd = copy.deepcopy(solver.optimizer.state_dict())
    assert set(sd) == {"state", "param_groups"} and sd["param_groups"][0]["lr"] == 3e-4
    assert float(sd["state"][0]["step"]) == 3.0
    # a torch.optim.Adam over the same parameters accepts the checkpoint (interchangeable layout)
    ref_opt = torch.optim.Adam([p.detach().clone().requires_grad_() for p in model.parameters()], lr=3e-4)
    ref_opt.load_state_dict(sd)
    # resume: a second solver loaded from the checkpoint continues bit-identically
    model2, _ = _small_model(merger_dropout=0.0)
    model2.load_state_dict(copy.deepcopy(model.state_dict()))
    solver2 = Solver(model2)
    solver2.optimizer.load_state_dict(sd)
    la, lb = solver.train_step(sb), solver2.train_step(sb)
    assert torch.equal(la, lb)
    assert torch.equal(solver.optimizer.flat_param, solver2.optimizer.flat_param)
    # lr schedulers reach the kernel through param_groups
    solver.optimizer.param_groups[0]["lr"] = 0.0
    before = solver.optimizer.flat_param.clone()
    solver.train_step(sb)
    assert torch.equal(before, solver.optimizer.flat_param)


def test_full_batch_properties():
    """BASELINE cfg2 at its full size (B=256): size-independent properties of the hot path --
    run-to-run bit determinism, finite loss, probabilities rows sum to 1, the diagonal target,
    and linearity of the encoder head in eval mode."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.losses import ClipLoss
    c = synthetic.CONFIGS["cfg2"]
    sb = synthetic.make_config_batch("cfg2", seed=7).to("cuda")
    model = _paper_model(c["C"], c["F"], c["S"], seed=1)
    sd0 = copy.deepcopy(model.state_dict())
    ban = torch.tensor([0.5, 0.5])
    model.merger.ban_center_override = ban
    solver = Solver(model)
    l1 = solver.train_step(sb)
    g1 = solver.optimizer.flat_grad.clone()
    p1 = solver.optimizer.flat_param.clone()
    model2 = _paper_model(c["C"], c["F"], c["S"], seed=1)
    model2.load_state_dict(sd0)
    model2.merger.ban_center_override = ban
    solver2 = Solver(model2)
    l2 = solver2.train_step(sb)
    assert torch.isfinite(l1)
    assert torch.equal(l1, l2)
    assert torch.equal(g1, solver2.optimizer.flat_grad)
    assert torch.equal(p1, solver2.optimizer.flat_param)
    est, cand = solver.predict(sb)
    probs = ClipLoss().cuda().get_probabilities(est, cand)
    assert probs.shape == (256, 256)
    assert (probs.sum(1) - 1).abs().max().item() < 1e-5
    # candidates used as estimates: every segment retrieves itself
    self_probs = ClipLoss().cuda().get_probabilities(cand, cand)
    assert (self_probs.argmax(1).cpu() == torch.arange(256)).all()
    # the CE loss equals -log of the diagonal probability
    loss = solver.eval_step(sb)
    diag = probs.diagonal().log().neg().mean()
    assert abs(float(loss) - float(diag)) < 1e-4


def test_eval_mode_single_kernel_layers_match_train_stats_path():
    """eval-mode ConvBNAct (one fused conv_nn launch) == conv + explicit affine/act/res kernels."""
    from brainmagick_amd import hip_ops as H
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 32, 200, generator=g).cuda()
    w = torch.randn(32, 32, 3, generator=g).cuda() * 0.1
    b = torch.randn(32, generator=g).cuda()
    scale = (torch.rand(32, generator=g) + 0.5).cuda()
    shift = torch.randn(32, generator=g).cuda()
    wp = H.pack_conv_fwd(w)
    pre, fused, _ = H.conv_nn(x, wp, 32, 3, 2, bias=b, scale=scale, shift=shift, res=x,
                              act=H.ACT_GELU, want_pre=True)
    two_pass = H.affine_act_res(pre, scale, shift, x, H.ACT_GELU)
    assert torch.equal(fused, two_pass)


NCCL_WORKER = r'''
import os, sys, copy, torch
sys.path.insert(0, sys.argv[1])
backend = sys.argv[2]
from brainmagick_amd import distrib, synthetic
from brainmagick_amd.models import SimpleConv
from brainmagick_amd.solver import Solver
cfg = dict(depth=4, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2,
           glu_context=1, complex_out=True, merger=True, merger_pos_dim=128, merger_channels=24,
           merger_dropout=0.0, initial_linear=24, subject_layers=True, subject_dim=0)
def run(negatives, prefetch=False):
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": 30}, out_channels=12, hidden={"meg": 32}, n_subjects=4, **cfg)
    solver = Solver(model, negatives=negatives)
    sb = synthetic.make_batch(8, 30, 64, 12, 4, seed=3)
    if prefetch:      # the next step's candidate all-gather is issued between this step's loss and backward
        copies = [sb.replace() for _ in range(4)]
        losses = [float(solver.train_step(copies[k], next_batch=copies[k + 1])) for k in range(3)]
    else:
        losses = [float(solver.train_step(sb)) for _ in range(3)]
    sd = solver.state_dict()["optimizer"]       # gathers the sharded moments (collective)
    return losses, solver.optimizer.flat_param.clone(), sd["state"][0]["exp_avg"].clone(), \
        model.state_dict()["encoders.meg.sequence.0.1.running_var"].clone()
plain = run("local")          # before init: world_size 1, no collectives
os.environ["BM_FORCE_DISTRIBUTED"] = "1"
distrib.init(backend)
assert distrib.is_distributed() and distrib.world_size() == 1
assert distrib.comm_kind() == {"rccl": "rccl/c-abi", "nccl": "torch.distributed/nccl"}[backend]
coll = run("node")            # reduce-scatter / all-gather / candidate gather / buffer all-reduce on RCCL
ahead = run("node", prefetch=True)
for other in (coll, ahead):
    assert plain[0] == other[0], (plain[0], other[0])
    for a, b in zip(plain[1:], other[1:]):
        assert torch.equal(a, b)
m = distrib.average_metrics({"loss": 2.0}, 3)
assert abs(m["loss"] - 2.0) < 1e-6
assert distrib.max_over_ranks(1.5) == 1.5
distrib.sync_buffers(torch.nn.BatchNorm1d(4).cuda())
distrib.barrier()
distrib.shutdown()
print("NCCL_WORKER_OK")
'''


@pytest.mark.parametrize("backend", ["rccl", "nccl"])
def test_rccl_code_path_world1(tmp_path, backend):
    """The real RCCL collectives -- behind the C-ABI (bm_comm_*: in-place reduce-scatter / all-gather on
    the flat bucket, candidate all-gather on the side stream, buffer all-reduce) and through the
    torch.distributed fallback -- at world_size 1 must reproduce the plain step bit for bit.  (Multi-rank
    semantics are covered by the 2-process gloo test on CPU and by the 2-GPU test below.)"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    script = tmp_path / "nccl_worker.py"
    script.write_text(NCCL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29551", WORLD_SIZE="1", RANK="0",
               LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BM_FORCE_DISTRIBUTED", None)
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([sys.executable, str(script), str(root), backend], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "NCCL_WORKER_OK" in out.stdout, out.stdout + out.stderr


TWO_RANK_WORKER = r'''
import os, sys, torch
sys.path.insert(0, sys.argv[1])
from brainmagick_amd import distrib, synthetic
from brainmagick_amd.models import SimpleConv
from brainmagick_amd.solver import Solver
distrib.init()
r, w = distrib.rank(), distrib.world_size()
assert w == 2 and distrib.comm_kind() == "rccl/c-abi"
cfg = dict(depth=4, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2,
           glu_context=1, complex_out=True, merger=True, merger_pos_dim=128, merger_channels=24,
           merger_dropout=0.0, initial_linear=24, subject_layers=True, subject_dim=0)
torch.manual_seed(0)
model = SimpleConv(in_channels={"meg": 30}, out_channels=12, hidden={"meg": 32}, n_subjects=4, **cfg)
solver = Solver(model, device=f"cuda:{r}", negatives="node")
sb = synthetic.make_batch(8, 30, 64, 12, 4, seed=3 + r)
losses = [float(solver.train_step(sb)) for _ in range(3)]
# replicas stay identical: parameters and BatchNorm buffers
flat = torch.cat([solver.optimizer.flat_param, solver._buffers.flat])
lo = flat.clone(); hi = flat.clone()
distrib.comm().all_reduce(hi, "max"); neg = -lo; distrib.comm().all_reduce(neg, "max")
assert torch.equal(hi, -neg), "replicas diverged"
assert all(l == l for l in losses)
distrib.barrier(); distrib.shutdown()
print("TWO_RANK_OK", r, losses)
'''


def test_two_ranks_over_rccl_when_two_gpus_are_visible(tmp_path):
    """2 processes x 1 GPU over the C-ABI RCCL communicator (skipped on the 1-GPU test box)."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 visible GPUs")
    script = tmp_path / "two_rank_worker.py"
    script.write_text(TWO_RANK_WORKER)
    root = Path(__file__).resolve().parent.parent
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", WORLD_SIZE="2", RANK=str(r),
                   LOCAL_RANK=str(r), HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("BM_FORCE_DISTRIBUTED", None)
        procs.append(subprocess.Popen([sys.executable, str(script), str(root)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"TWO_RANK_OK {r}" in out, out


@pytest.mark.parametrize("negatives,world", [("local", 2), ("node", 2), ("node", 4), ("node", 8)])
def test_replicas_match_the_data_parallel_oracle(negatives, world):
    """SURVEY.md §8(c) data-parallel oracle against the HIP path at world size 2, 4 and 8 on ONE GPU: `world` `Solver`
    replicas run the unmodified `train_step` in threads under an in-process loopback communicator (tests/loopback.py:
    the same interface as the RCCL communicator -- candidate all-gather + target_offset, in-place reduce-scatter
    of the flat gradient bucket, sharded Adam, in-place all-gather of the parameters, buffer all-reduce).
    Expectation = the oracle run once per rank on that rank's batch ("node": against the candidates of BOTH
    ranks, own block as targets), gradients averaged over the ranks (flashy.distrib.sync_model, bm/solver.py:386),
    one Adam step on the mean, BatchNorm running statistics averaged, per-rank batch statistics.  Then a
    checkpoint (`Solver.state_dict()`, which gathers the sharded Adam moments) is loaded into fresh replicas that
    must continue bit-identically.  At world 4 and 8 the replicas also hand over the NEXT batch (host tensors: staged
    on the copy stream; its candidate all-gather is prefetched next to the backward pass) -- rank 7's targets are the
    block at target_offset = 7 B of 8 B candidates."""
    from loopback import run_replicas
    from brainmagick_amd import distrib
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    B, steps = 8, 2
    prefetch = world > 2
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=96, initial_linear=96, depth=4, merger_dropout=0.0)
    C, T, Fd, S, hidden = 30, 160, 12, 4, 96

    def build():
        torch.manual_seed(0)
        return SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S, **cfg)

    sd0 = copy.deepcopy(build().state_dict())
    # one set of recordings for every batch: PositionGetter caches a layout per recording_index like the reference
    recordings = synthetic.make_layouts(2, [C], torch.Generator().manual_seed(9))
    batches = [[synthetic.make_batch(B, C, T, Fd, S, seed=50 + 10 * r + k, recordings=recordings)
                for k in range(steps + 1)] for r in range(world)]

    def body(r):
        assert distrib.is_distributed() and distrib.world_size() == world and distrib.rank() == r
        model = build()
        solver = Solver(model, negatives=negatives)
        names = [k for k, _ in model.named_parameters()]
        lo, hi = distrib.shard_bounds(solver.optimizer.padded, world, r)
        out = dict(losses=[], names=names, offsets=list(solver.optimizer.offsets), shard=(lo, hi))
        for k in range(steps):
            out["losses"].append(float(solver.train_step(batches[r][k],
                                                         next_batch=batches[r][k + 1] if prefetch else None)))
            if k == 0:
                out["grad_shard"] = solver.optimizer.flat_grad[lo:hi].clone().cpu()      # sum over the ranks
        out["flat_param"] = solver.optimizer.flat_param.clone().cpu()
        out["sd"] = {k: v.clone().cpu() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError, match="gather_moments"):
            solver.optimizer.state_dict()             # sharded moments: no hidden collective, a loud error
        state = copy.deepcopy(solver.state_dict())    # collective: every replica calls it
        out["exp_avg"] = state["optimizer"]["state"][0]["exp_avg"].clone().cpu()
        nxt = float(solver.train_step(batches[r][steps]))
        resumed = Solver(build(), negatives=negatives)
        resumed.load_state_dict(state)
        nxt2 = float(resumed.train_step(batches[r][steps]))
        assert nxt == nxt2, (nxt, nxt2)
        assert torch.equal(solver.optimizer.flat_param, resumed.optimizer.flat_param)
        assert torch.equal(solver._buffers.flat, resumed._buffers.flat)
        return out

    res = run_replicas(world, body)
    for r in range(1, world):
        assert torch.equal(res[0]["flat_param"], res[r]["flat_param"]), "replicas diverged"
        assert torch.equal(res[0]["exp_avg"], res[r]["exp_avg"]), "gathered moments differ between ranks"

    # the data-parallel oracle
    oracles = [O.OracleModel(copy.deepcopy(sd0), cfg, hidden, Fd) for _ in range(world)]
    for k in range(steps):
        per_rank = []
        for r in range(world):
            sb = batches[r][k]
            cands = sb.features
            if negatives == "node":
                cands = torch.roll(torch.cat([batches[q][k].features for q in range(world)]), -r * B, 0)
            loss, _, grads = oracles[r].loss_and_grads(sb.meg, sb.positions(), sb.subject_index, cands, True)
            assert abs(res[r]["losses"][k] - float(loss)) < LOSS_TOL, (k, r, res[r]["losses"][k], float(loss))
            per_rank.append(grads)
        mean = {n: sum(g[n] for g in per_rank) / world for n in per_rank[0]}
        if k == 0:
            gscale = max(v.double().norm().item() for v in mean.values())
            for r in range(world):
                flat = torch.zeros(res[r]["shard"][1] - res[r]["shard"][0] + res[r]["shard"][0], dtype=torch.float64)
                full = torch.zeros(max(res[r]["offsets"]) + 10 ** 6, dtype=torch.float64)
                for n, off in zip(res[r]["names"], res[r]["offsets"]):
                    full[off:off + mean[n].numel()] = mean[n].reshape(-1).double()
                lo, hi = res[r]["shard"]
                assert rel_l2(res[r]["grad_shard"] / world, full[lo:hi]) < GRAD_TOL
                del flat
        for r in range(world):
            oracles[r].apply_adam(mean)
        for n in oracles[0].sd:                         # flashy sync_model averages the float buffers
            if "running_" in n:
                avg = sum(o.sd[n] for o in oracles) / world
                for o in oracles:
                    o.sd[n] = avg.clone()
    for n, v in res[0]["sd"].items():
        if not v.is_floating_point():
            assert int(v) == int(oracles[0].sd[n]), n
        elif n in mean:
            if is_noise_grad(mean[n], gscale):
                continue
            ok, info = adam_params_close(v, oracles[0].sd[n], steps, mean[n], gscale)
            assert ok, (n, info)
        else:
            assert running_stat_close(v, oracles[0].sd[n], steps), n


def test_two_replicas_with_learnable_candidates_match_joint_autograd():
    """DeepMel feature model + whole-node negatives at world size 2 (loopback communicator, tests/loopback.py): the
    candidates of both ranks are gathered with the autograd-aware all-gather (its backward reduce-scatters dCand to
    the owner), so the feature model's gradient is that of the MEAN over ranks of the per-rank losses.  Oracle = torch
    autograd on the CPU over both ranks jointly; compared: per-rank losses and the reduce-scattered gradient shards."""
    from loopback import run_replicas
    from brainmagick_amd import distrib
    from brainmagick_amd.models import SimpleConv, DeepMel
    from brainmagick_amd.solver import Solver
    world, B = 2, 6
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=24, initial_linear=24, depth=4, merger_dropout=0.0)
    C, T, Fd, S, hidden, out_ch = 20, 64, 12, 3, 32, 16
    fm_kw = dict(n_hidden_channels=24, n_hidden_layers=4, n_out_channels=out_ch, kernel=3, stride=1,
                 dilation_growth=2, dilation_period=5, batch_norm=True, activation_on_last=False,
                 skip=True, glu_context=1, glu=2)

    def build():
        torch.manual_seed(2)
        model = SimpleConv(in_channels={"meg": C}, out_channels=out_ch, hidden={"meg": hidden}, n_subjects=S, **cfg)
        return model, DeepMel(n_in_channels=Fd, **fm_kw)

    m0, f0 = build()
    sd_m, sd_f = copy.deepcopy(m0.state_dict()), copy.deepcopy(f0.state_dict())
    recordings = synthetic.make_layouts(1, [C], torch.Generator().manual_seed(4))
    batches = [synthetic.make_batch(B, C, T, Fd, S, seed=70 + r, recordings=recordings) for r in range(world)]

    def body(r):
        model, fmodel = build()
        solver = Solver(model, feature_model=fmodel, negatives="node")
        loss = float(solver.train_step(batches[r]))
        opt = solver.optimizer
        lo, hi = distrib.shard_bounds(opt.padded, world, r)
        names = [("m", k) for k, _ in model.named_parameters()] + [("f", k) for k, _ in fmodel.named_parameters()]
        return dict(loss=loss, shard=(lo, hi), grad_shard=opt.flat_grad[lo:hi].clone().cpu(), names=names,
                    offsets=list(opt.offsets))

    res = run_replicas(world, body)

    om = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd_m.items()}
    of = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd_f.items()}
    ests, cands = [], []
    for r in range(world):
        sb = batches[r]
        ests.append(O.simpleconv_forward(om, cfg, sb.meg, sb.positions(), sb.subject_index, hidden, out_ch,
                                         training=True))
        cands.append(O.deep_mel_forward(of, sb.features, 24, 4, out_ch, training=True))
    allc = torch.cat(cands)
    losses = [O.clip_loss(ests[r], torch.roll(allc, -r * B, 0)) for r in range(world)]
    (sum(losses) / world).backward()
    for r in range(world):
        assert abs(res[r]["loss"] - float(losses[r])) < LOSS_TOL, (r, res[r]["loss"], float(losses[r]))
    full = torch.zeros(max(res[0]["offsets"]) + 10 ** 6, dtype=torch.float64)
    for (which, k), off in zip(res[0]["names"], res[0]["offsets"]):
        g = (om if which == "m" else of)[k].grad
        full[off:off + g.numel()] = g.reshape(-1).double()
    for r in range(world):
        lo, hi = res[r]["shard"]
        assert rel_l2(res[r]["grad_shard"] / world, full[lo:hi]) < GRAD_TOL, (r, rel_l2(res[r]["grad_shard"] / world, full[lo:hi]))


def test_two_replicas_with_the_symmetric_loss_gather_their_estimates():
    """``ClipLoss(symmetric=True)`` under whole-node negatives at world size 2 (loopback communicator): the estimates of
    both ranks are gathered with the autograd-aware all-gather, so each rank's target candidates classify the whole
    node's estimates and the gradient of a rank's column term reaches the OTHER rank's encoder through the
    reduce-scatter.  Oracle = torch autograd on the CPU over both ranks jointly (`clip_loss_symmetric_node`); compared:
    per-rank losses and the reduce-scattered gradient shards."""
    from loopback import run_replicas
    from brainmagick_amd import distrib
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    world, B = 2, 6
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=24, initial_linear=24, depth=4, merger_dropout=0.0)
    C, T, Fd, S, hidden = 20, 64, 12, 3, 32

    def build():
        torch.manual_seed(2)
        return SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S, **cfg)

    sd_m = copy.deepcopy(build().state_dict())
    recordings = synthetic.make_layouts(1, [C], torch.Generator().manual_seed(4))
    batches = [synthetic.make_batch(B, C, T, Fd, S, seed=90 + r, recordings=recordings) for r in range(world)]

    def body(r):
        model = build()
        solver = Solver(model, loss=ClipLoss(symmetric=True), negatives="node")
        loss = float(solver.train_step(batches[r]))
        opt = solver.optimizer
        lo, hi = distrib.shard_bounds(opt.padded, world, r)
        return dict(loss=loss, shard=(lo, hi), grad_shard=opt.flat_grad[lo:hi].clone().cpu(),
                    names=[k for k, _ in model.named_parameters()], offsets=list(opt.offsets))

    res = run_replicas(world, body)
    om = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd_m.items()}
    ests = [O.simpleconv_forward(om, cfg, sb.meg, sb.positions(), sb.subject_index, hidden, Fd, training=True)
            for sb in batches]
    cand_all = torch.cat([sb.features for sb in batches])
    losses = [O.clip_loss_symmetric_node(torch.cat(ests), cand_all, r, B) for r in range(world)]
    (sum(losses) / world).backward()
    for r in range(world):
        assert abs(res[r]["loss"] - float(losses[r])) < LOSS_TOL, (r, res[r]["loss"], float(losses[r]))
    full = torch.zeros(max(res[0]["offsets"]) + 10 ** 6, dtype=torch.float64)
    for k, off in zip(res[0]["names"], res[0]["offsets"]):
        full[off:off + om[k].grad.numel()] = om[k].grad.reshape(-1).double()
    for r in range(world):
        lo, hi = res[r]["shard"]
        assert rel_l2(res[r]["grad_shard"] / world, full[lo:hi]) < GRAD_TOL, (r, rel_l2(res[r]["grad_shard"] / world, full[lo:hi]))


def test_bench_self_launches_on_two_gpus_when_visible():
    """`python bench.py --gpus 2` outside a torchrun environment re-launches itself under torch.distributed.run, one
    rank per GPU over the C-ABI RCCL communicator, whole-node negatives with the candidate gather prefetched; rank 0
    prints ONE JSON line LAST on stdout (skipped on the 1-GPU test box)."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 visible GPUs")
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "BM_FORCE_DISTRIBUTED"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--no-cpu-baseline", "--accuracy-steps", "0", "--no-exact", "--no-clip"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["config"]["rccl_world"] == 2 and line["config"]["negatives"] == "node"
    assert line["config"]["global_batch"] == 512 and line["value"] > 0


def test_bench_under_a_launcher_prints_one_json_line_and_nothing_else():
    """The driver's contract for N > 1: started with RANK / WORLD_SIZE / MASTER_* in the environment, bench.py
    brings the C-ABI RCCL communicator up (here at world size 1: the same code path, `BM_FORCE_DISTRIBUTED`) and
    rank 0 prints exactly ONE line on stdout -- librccl's version banner goes to stderr."""
    import json
    import os
    import random
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BM_FORCE_DISTRIBUTED="1", RANK="0", LOCAL_RANK="0",
               WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(random.randint(20000, 28000)))
    out = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--negatives", "node", "--no-cpu-baseline", "--accuracy-steps", "0", "--no-exact",
                          "--no-clip"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines[:5]
    line = json.loads(lines[0])
    assert line["config"]["comm"] == "rccl/c-abi" and line["config"]["rccl_world"] == 1
    assert line["config"]["negatives"] == "node" and line["value"] > 0


def test_bench_dumps_what_its_last_timed_step_returned(tmp_path):
    """`bench.py --dump-outputs DIR` writes the loss of the last timed step (the one the result line reports) and
    the model state it left, in float32 / float64 and within 64 MB; `--steps` is the number of timed steps."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    import numpy as np
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "BM_FORCE_DISTRIBUTED"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path), "--no-cpu-baseline", "--accuracy-steps", "0", "--no-exact",
                          "--no-clip", "--no-side-blocks", "--no-pmc"], env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert float(np.load(tmp_path / "loss.npy")) == line["config"]["final_loss"]
    files = sorted(tmp_path.glob("*.npy"))
    assert len(files) == line["dump_outputs"]["arrays"] and sum(f.stat().st_size for f in files) <= 64e6
    heads = np.load(tmp_path / "merger.heads.npy")
    assert heads.dtype == np.float32 and np.isfinite(heads).all()


def test_bench_plain_run_prints_the_headline_only():
    """A plain `bench.py` run (no `--full`) sets up, warms up, times its steps and prints the result line with the
    driver's contract and the configuration; the side measurements are left to `--full`."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "BM_FORCE_DISTRIBUTED"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines[:5]
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "segments/s" and line["higher_is_better"] is True and line["dtype"].startswith("f32")
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] - 256e3) < 1e-6 * 256e3
    for k in ("roofline", "comm_ms", "sustained", "pcie_inclusive", "dvfs_probe", "other_fp32_modes", "roofline_clip",
              "roofline_retrieval", "retrieval", "retrieval_parity", "cpu_baseline"):
        assert k not in line, k


# Dimensions of the long-horizon parity runs (this test and bench.py's `retrieval_parity`): every contraction of the
# step runs in the SAME kernels as the headline benchmark -- the wide f16x2 conv (T > 128, M >= 96), the wide f16x2
# weight gradients (M a multiple of 256 / 320 within 25 %, Cn of 64) and the f16x2 score contraction (batch >= 128);
# like at full size, only the grouped (per-subject / per-layout) weight gradients, the layout logits and the
# narrow-M final-layer weight gradient run in the 3 x bf16 kernels.
PARITY_DIMS = dict(C=64, T=192, F=128, S=4, B=128, hidden=256, merger_channels=256, depth=4)


def parity_model_cfg():
    cfg = dict(O.CLIP_CONV_CFG)
    d = PARITY_DIMS
    # merger_pos_dim 288 = 2 * 12^2: the attention backward contracts over the embedding axis (a "time" axis > 128)
    cfg.update(merger_pos_dim=288, merger_channels=d["merger_channels"], initial_linear=d["merger_channels"],
               depth=d["depth"], merger_dropout=0.0)
    return cfg


def assert_headline_kernels(records):
    """`records`: (label, flops) of every MFMA launch of one training step (hip_ops.KernelTimer).  Every launch that
    carries real work (>= 1 GFLOP: all convs of the stack and the head, their weight gradients, the score
    contraction and its backward) must be a wide f16x2 kernel; the 3 x bf16 family may only serve the small
    products (per-layout attention logits, the composed front end's matrix products, the grouped per-(layout,
    subject) weight gradient) -- as in the headline run."""
    names = [n for n, _ in records]
    big = [(n, f) for n, f in records if f >= 1e9]
    assert len(big) >= 3 * (PARITY_DIMS["depth"] + PARITY_DIMS["depth"] // 2) + 4, big
    assert all(n.startswith(("conv_nn_h2w_kernel", "gemm_nt_h2w_kernel", "clip_scores:gemm_nt_h2w")) for n, _ in big), \
        sorted({n for n, _ in big})
    assert "clip_scores:gemm_nt_h2w" in names, sorted(set(names))
    assert not [n for n in names if n.startswith(("gemm_nt_kernel", "conv_nn_kernel"))], \
        sorted(set(names))


def test_training_curve_and_top10_parity(steps: int = 200, n_held: int = 2048):
    """SURVEY.md §8d accuracy parity THROUGH THE HEADLINE KERNELS: train the same initial state for 200 steps on the
    same learnable (planted-latent) batches with the HIP path and with the oracle; the loss curves must agree
    within 1 % (relative, every step) and the top-10 / top-1 segment-retrieval accuracy on 2 048 held-out segments
    within +-1 point of each other.  The planted noise keeps the task away from saturation so that a precision
    regression of the HIP path would move the number."""
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd import retrieval
    headline_mode = H.get_compute_dtype() == "f16x2"     # (tests/test_exact_f32_gpu.py re-runs this in the other modes)
    cfg = parity_model_cfg()
    d = PARITY_DIMS
    C, T, Fd, S, B, hidden = d["C"], d["T"], d["F"], d["S"], d["B"], d["hidden"]
    noise = PARITY_NOISE
    torch.manual_seed(5)
    model = SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden},
                       n_subjects=S, **cfg)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), cfg, hidden, Fd)
    solver = Solver(model)
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(min(32, prev_threads))       # the GPU box's 256 hardware threads slow torch's CPU pool down
    hip_losses, ref_losses = [], []
    try:
        for step in range(steps):
            # a fresh batch every step: the 2 M-parameter model would memorise a recycled set within 200 steps
            sb = synthetic.make_batch(B, C, T, Fd, S, seed=100 + step, planted=True, noise=noise)
            if step in (0, steps - 1):                     # which kernels ran, first and last step
                timer = H.KernelTimer()
                H.set_kernel_timer(timer)
            hip_losses.append(float(solver.train_step(sb)))
            if step in (0, steps - 1):
                H.set_kernel_timer(None)
                if headline_mode:
                    assert_headline_kernels([(r[0], r[1]) for r in timer.records])
            ref_losses.append(float(oracle.train_step(sb.meg, sb.positions(), sb.subject_index,
                                                      sb.features)[0]))
        hip, ref = torch.tensor(hip_losses), torch.tensor(ref_losses)
        if steps >= 200:
            assert ref[-8:].mean() < 0.8 * ref[:8].mean(), "planted task should be learnable"
        assert ((hip - ref).abs() / ref.abs()).max().item() < 1e-2, (hip_losses[-5:], ref_losses[-5:])
        held = synthetic.make_batch(n_held, C, T, Fd, S, seed=999, planted=True, noise=noise)
        est_hip, cand = solver.predict(held)
        est_ref = oracle.forward(held.meg, held.positions(), held.subject_index)
        acc_hip = retrieval.segment_topk_accuracy(ClipLoss().cuda(), est_hip, cand, topks=(1, 10))
        probs_ref = O.clip_probabilities(est_ref, held.features)
    finally:
        torch.set_num_threads(prev_threads)
        H.set_kernel_timer(None)
    labels = torch.arange(n_held)
    acc_ref = {k: O.topk_accuracy(probs_ref, labels, labels, k) for k in (1, 10)}
    print(f"parity run: loss {ref_losses[0]:.3f} -> {ref_losses[-1]:.3f}, top-10 hip {acc_hip['top10']:.4f} "
          f"oracle {acc_ref[10]:.4f}, top-1 hip {acc_hip['top1']:.4f} oracle {acc_ref[1]:.4f}")
    if steps >= 200:
        assert 0.15 <= acc_ref[10] <= 0.9, ("the planted task must stay away from saturation", acc_ref)
    for k in (1, 10):
        assert abs(acc_hip[f"top{k}"] - acc_ref[k]) <= 0.01 + 1e-9, (k, acc_hip, acc_ref)


def test_deep_mel_feature_model_step():
    """Next row §8(f)#3: DeepMel (ConvSequence on the mel candidates) trained jointly with the
    encoder; ClipLoss back-propagates into the candidates.  vs CPU oracle (torch autograd)."""
    from brainmagick_amd.models import SimpleConv, DeepMel
    from brainmagick_amd.solver import Solver
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=24, initial_linear=24, depth=4,
               merger_dropout=0.0)
    C, T, Fd, S, B, hidden, out_ch = 20, 64, 12, 3, 6, 32, 16
    sb = synthetic.make_batch(B, C, T, Fd, S, seed=11)
    torch.manual_seed(2)
    model = SimpleConv(in_channels={"meg": C}, out_channels=out_ch, hidden={"meg": hidden},
                       n_subjects=S, **cfg)
    fm_kw = dict(n_hidden_channels=24, n_hidden_layers=4, n_out_channels=out_ch, kernel=3, stride=1,
                 dilation_growth=2, dilation_period=5, batch_norm=True, activation_on_last=False,
                 skip=True, glu_context=1, glu=2)
    fmodel = DeepMel(n_in_channels=Fd, **fm_kw)
    sd_m, sd_f = copy.deepcopy(model.state_dict()), copy.deepcopy(fmodel.state_dict())
    solver = Solver(model, feature_model=fmodel)
    loss = solver.train_step(sb)

    # oracle: same two networks with torch autograd on CPU
    om = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k)
          for k, v in sd_m.items()}
    of = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k)
          for k, v in sd_f.items()}
    est = O.simpleconv_forward(om, cfg, sb.meg, sb.positions(), sb.subject_index, hidden, out_ch,
                               training=True)
    cand = O.deep_mel_forward(of, sb.features, 24, 4, out_ch, training=True)
    loss_ref = O.clip_loss(est, cand)
    loss_ref.backward()
    assert abs(float(loss) - float(loss_ref)) < LOSS_TOL
    gscale = max(v.grad.double().norm().item() for v in list(om.values()) + list(of.values())
                 if v.requires_grad and v.grad is not None)
    for name, mod, ref in (("model", model, om), ("feature_model", fmodel, of)):
        for k, p in mod.named_parameters():
            assert close(p.grad, ref[k].grad, GRAD_TOL, gscale), (name, k, rel_l2(p.grad, ref[k].grad))


def _small_model(C=20, Fd=10, S=3, hidden=32, seed=3, **over):
    from brainmagick_amd.models import SimpleConv
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=32, merger_channels=16, initial_linear=16)
    cfg.update(over)
    torch.manual_seed(seed)
    return SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S,
                      **cfg), cfg


@pytest.mark.parametrize("T,widths", [(48, dict()), (200, dict(hidden=96, merger_channels=96, initial_linear=96))])
def test_composed_front_end_matches_the_three_layer_chain(T, widths):
    """merger -> initial 1x1 -> subject layers composed into one grouped conv per (layout, subject) pair
    (functional.FusedFrontEndFn) against (a) the same model run layer by layer and (b) the CPU oracle: output, loss,
    every gradient.  Two layouts, three subjects, a (layout, subject) pair that no segment carries, a sensor ban."""
    from brainmagick_amd.models import simpleconv as SC
    from brainmagick_amd.losses import ClipLoss
    widths = dict(widths)
    hidden = widths.pop("hidden", 32)
    model, cfg = _small_model(S=3, hidden=hidden, merger_dropout=0.3, **widths)
    B, C, Fd = 12, 20, 10
    sb = synthetic.make_batch(B, C, T, Fd, 3, seed=4, n_layouts=2)
    sb.subject_index[sb.recording_index == 1] = 0          # layout 1 only ever meets subject 0: empty pairs
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), cfg, hidden, Fd)
    ban = torch.tensor([0.35, 0.55])
    loss_ref, est_ref, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index, sb.features,
                                                         True, ban)
    model = model.cuda().train()
    model.merger.ban_center_override = ban
    sbg = sb.to("cuda")
    mask = torch.ones(B, 1, T, dtype=torch.bool, device="cuda")
    results = {}
    for fuse in (True, False):
        SC._FUSE_FRONT_END = fuse
        try:
            model.zero_grad(set_to_none=True)
            est = model({"meg": sbg.meg.clone()}, sbg)
            assert model.front_end_fused == fuse
            loss = ClipLoss().cuda()(est, sbg.features, mask)
            loss.backward()
        finally:
            SC._FUSE_FRONT_END = True
        results[fuse] = (est.detach(), float(loss), {k: p.grad.clone() for k, p in model.named_parameters()})
    gscale = max(v.double().norm().item() for v in grads_ref.values())
    for fuse, (est, loss, grads) in results.items():
        assert rel_l2(est, est_ref) < FWD_TOL, (fuse, rel_l2(est, est_ref))
        assert abs(loss - float(loss_ref)) < LOSS_TOL
        for k, g in grads.items():
            assert close(g, grads_ref[k], GRAD_TOL, gscale), (fuse, k, rel_l2(g, grads_ref[k]))
    front = [k for k in results[True][2] if k.startswith(("merger.", "initial_linear.", "subject_layers."))]
    assert len(front) == 4, front
    for k in front:       # the two formulations of the same gradient agree far inside the tolerance to the oracle
        a, b = results[True][2][k], results[False][2][k]
        assert close(a, b, 2e-5, gscale), (k, rel_l2(a, b))


@pytest.mark.parametrize("B,T", [(1, 360), (2, 24), (3, 7), (5, 129)])
def test_edge_shapes_against_oracle(B, T):
    """Single-segment batches (BatchNorm over T only), windows shorter than the 16-sample dilation
    halo / one MFMA k-step, and a tile-boundary length."""
    from brainmagick_amd.solver import Solver
    model, cfg = _small_model()
    sb = synthetic.make_batch(B, 20, T, 10, 3, seed=T)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), cfg, 32, 10)
    ban = torch.tensor([0.9, 0.9])
    model.merger.ban_center_override = ban
    solver = Solver(model)
    loss_ref, est_ref, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index,
                                                         sb.features, True, ban)
    loss = solver.train_step(sb)
    assert abs(float(loss) - float(loss_ref)) < LOSS_TOL
    gscale = max(v.double().norm().item() for v in grads_ref.values())
    if B * T > 64:      # with a handful of samples per BatchNorm channel the problem is ill-conditioned
        for k, p in model.named_parameters():
            assert close(p.grad, grads_ref[k], 5 * GRAD_TOL, gscale), (k, rel_l2(p.grad, grads_ref[k]))


def test_empty_batch_and_rejected_batch():
    """bm/solver.py:255-256: a batch whose segments were all rejected yields four Nones."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    model, _ = _small_model()
    sb = synthetic.make_batch(4, 20, 48, 10, 3, seed=1)
    sb.meg = sb.meg * 1e4                       # every segment exceeds the rejection limit
    sr = ScaleReject(DeviceBatchScaler(torch.zeros(1, 20), torch.ones(1, 20)), limit=20, clip=False)
    solver = Solver(model, scale_reject=sr)
    assert solver._process_batch(sb) == (None, None, None, None)
    assert sr.rejection_rate == 1.0


def test_all_sensors_banned_is_nan_like_reference():
    """a sensor-dropout disc that covers every valid sensor gives an all -inf softmax row
    -> NaN in the reference; replicated, not 'fixed'."""
    model, cfg = _small_model(merger_dropout=5.0)        # radius covers the whole unit square
    sb = synthetic.make_batch(2, 20, 48, 10, 3, seed=2)
    oracle = O.OracleModel(copy.deepcopy(model.state_dict()), cfg, 32, 10)
    ban = torch.tensor([0.5, 0.5])
    est_ref = oracle.forward(sb.meg, sb.positions(), sb.subject_index, training=True, ban_center=ban)
    model = model.cuda().train()
    model.merger.ban_center_override = ban
    sbg = sb.to("cuda")
    est = model({"meg": sbg.meg}, sbg)
    assert torch.isnan(est_ref).all() and torch.isnan(est).all()


def test_target_offset_matches_rolled_candidates():
    """ClipLoss(target_offset=k) == reference ClipLoss on candidates rolled so that the targets come
    first (the whole-node negatives layout of a data-parallel rank)."""
    from brainmagick_amd.losses import ClipLoss
    g = torch.Generator().manual_seed(9)
    est = torch.randn(4, 6, 30, generator=g)
    cand = torch.randn(12, 6, 30, generator=g)
    mask = torch.ones(4, 1, 30, dtype=torch.bool, device="cuda")
    for off in (0, 4, 8):
        e = est.cuda().requires_grad_(True)
        loss = ClipLoss().cuda()(e, cand.cuda(), mask, target_offset=off)
        loss.backward()
        er = est.double().requires_grad_(True)
        ref = O.clip_loss(er, torch.roll(cand.double(), -off, 0))
        ref.backward()
        assert abs(float(loss) - float(ref)) < 1e-5
        assert rel_l2(e.grad, er.grad) < GRAD_TOL


def test_rejected_batch_reuses_last_and_nonfinite_asserts():
    """bm/solver.py:345-352 (empty batch -> last batch) and :258-260 (isfinite asserts)."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    model, _ = _small_model()
    good = synthetic.make_batch(4, 20, 48, 10, 3, seed=1)
    bad = synthetic.make_batch(4, 20, 48, 10, 3, seed=2)
    bad.meg = bad.meg * 1e4
    sr = ScaleReject(DeviceBatchScaler(torch.zeros(1, 20), torch.ones(1, 20)), limit=20, clip=False)
    solver = Solver(model, scale_reject=sr)
    with pytest.raises(RuntimeError, match="Empty batch"):
        solver.train_step(bad)
    l1 = solver.train_step(good)
    l2 = solver.train_step(bad)                 # silently re-processes `good`
    assert torch.isfinite(l1) and torch.isfinite(l2) and float(l2) < float(l1) + 1.0
    nan = synthetic.make_batch(4, 20, 48, 10, 3, seed=3)
    nan.features[0, 0, 0] = float("nan")
    fresh = Solver(_small_model()[0])
    with pytest.raises(AssertionError):
        fresh.train_step(nan)
    inf = synthetic.make_batch(4, 20, 48, 10, 3, seed=4)
    inf.meg[3, 19, 47] = float("-inf")                 # the very last element
    with pytest.raises(AssertionError):
        fresh.train_step(inf)
    assert torch.isfinite(fresh.train_step(good))      # the flag does not stick


def test_a_failed_assert_leaves_no_trace_in_the_solver_state():
    """The asserts of bm/solver.py:258-260 fire BEFORE the reference touches anything.  Here they are evaluated after
    the forward pass (asynchronous flag read), so what the forward pass touched is put back: the "last good batch",
    the negatives pool, the BatchNorm batch counters; the running statistics were never updated (bn_finalize skips a
    non-finite batch); a caller that catches the AssertionError continues exactly as if the batch had not existed."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject

    def run(poison):
        model, _ = _small_model(merger_dropout=0.0)      # (no draw on the device generator: the runs stay comparable)
        solver = Solver(model, n_negatives=6, scale_reject=ScaleReject(
            DeviceBatchScaler(torch.zeros(1, 20), torch.ones(1, 20)), limit=20, clip=False))
        solver.negative_generator = torch.Generator().manual_seed(3)
        good = [synthetic.make_batch(4, 20, 48, 10, 3, seed=10 + i) for i in range(3)]
        losses = [float(solver.train_step(good[0]))]
        if poison:
            nan = synthetic.make_batch(4, 20, 48, 10, 3, seed=99)
            nan.features[1, 2, 3] = float("nan")
            with pytest.raises(AssertionError):
                solver.train_step(nan)
            assert solver._last_batch is good[0]
            assert not any(bool(torch.isnan(b).any()) for b in solver.negative_pool.values() if b is not None)
        # a fully rejected batch now re-trains on the last GOOD batch
        rejected = synthetic.make_batch(4, 20, 48, 10, 3, seed=5)
        rejected.meg = rejected.meg * 1e4
        losses.append(float(solver.train_step(rejected)))
        losses.append(float(solver.train_step(good[1])))
        return losses, {k: v.clone() for k, v in model.state_dict().items()}

    clean_losses, clean_sd = run(False)
    losses, sd = run(True)
    assert losses == clean_losses, (losses, clean_losses)
    for k, v in sd.items():
        assert torch.equal(v, clean_sd[k]), k            # incl. num_batches_tracked and the running statistics


def test_a_failed_assert_drops_the_prefetch_that_stood_in_for_a_rejected_batch():
    """Whole-node negatives: a fully rejected NEXT batch is prefetched as the last good batch (so that the rank issues its
    candidate gather like the others) -- and between the loss and the deferred assert of a poisoned step the "last good
    batch" IS the poisoned one.  The rollback must drop that prefetch: a caller that catches the AssertionError and goes
    on re-trains on the last GOOD batch, with the same loss as if the poisoned batch had never existed; the BatchNorm
    batch counters come back from a copy."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject

    def run(poison):
        model, _ = _small_model(merger_dropout=0.0)
        solver = Solver(model, negatives="node", batch_size=4, scale_reject=ScaleReject(
            DeviceBatchScaler(torch.zeros(1, 20), torch.ones(1, 20)), limit=20, clip=False))
        good = [synthetic.make_batch(4, 20, 48, 10, 3, seed=10 + i) for i in range(2)]
        rejected = synthetic.make_batch(4, 20, 48, 10, 3, seed=5)
        rejected.meg = rejected.meg * 1e4
        losses = [float(solver.train_step(good[0]))]
        counters = [int(m.num_batches_tracked) for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
        if poison:
            nan = synthetic.make_batch(4, 20, 48, 10, 3, seed=99)
            nan.features[1, 2, 3] = float("nan")
            with pytest.raises(AssertionError):
                solver.train_step(nan, next_batch=rejected)
            assert solver._last_batch is good[0] and solver._prefetched is None
            assert counters == [int(m.num_batches_tracked) for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
        losses.append(float(solver.train_step(rejected)))          # re-trains on good[0]
        losses.append(float(solver.train_step(good[1])))
        assert all(l == l for l in losses), losses
        return losses

    assert run(True) == run(False)


def test_prefetch_is_by_identity_and_can_be_abandoned():
    """Solver.train_step(batch, next_batch=...) prepares the next batch ahead (device copy, max / finiteness pass, and
    with whole-node negatives the candidate gather); the prepared state is used only if the SAME batch object comes
    next, otherwise dropped -- losses equal those of plain stepping either way."""
    from brainmagick_amd.solver import Solver
    batches = [synthetic.make_batch(4, 20, 48, 10, 3, seed=30 + k) for k in range(4)]

    def run(mode):
        model, _ = _small_model(merger_dropout=0.0)
        solver = Solver(model)
        out = []
        for k in range(3):
            if mode == "plain":
                out.append(float(solver.train_step(batches[k])))
            elif mode == "ahead":
                out.append(float(solver.train_step(batches[k], next_batch=batches[k + 1])))
            else:                                   # announces one batch, trains on another
                out.append(float(solver.train_step(batches[k], next_batch=batches[3])))
        return out

    plain = run("plain")
    assert run("ahead") == plain
    assert run("abandoned") == plain


def test_mask_assert_is_deferred_to_the_next_sync_point():
    """bm/losses.py:110 `assert mask.all()`: stand-alone ClipLoss raises at once like the reference; under the Solver
    the verdict travels in the device flag word and is raised at the next step's single synchronisation point."""
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.solver import Solver
    est = torch.randn(4, 6, 30).cuda()
    cand = torch.randn(4, 6, 30).cuda()
    bad = torch.ones(4, 1, 30, dtype=torch.bool, device="cuda")
    bad[2, 0, 7] = False
    with pytest.raises(AssertionError):
        ClipLoss().cuda()(est, cand, bad)
    model, _ = _small_model()
    solver = Solver(model)
    good = synthetic.make_batch(4, 20, 48, 10, 3, seed=1)
    masked = good.replace(features_mask=good.features_mask.clone())
    masked.features_mask[1, 0, 5] = False
    solver.train_step(good)
    solver.train_step(masked)                      # flagged on the device, no sync in the middle of the step
    with pytest.raises(AssertionError, match="mask"):
        solver.train_step(good)
    assert torch.isfinite(solver.train_step(good))  # the flag does not stick


def test_deep_mel_shape_like_reference():
    """bm/test_model.py:53-68 (fake_batch features [2, 8, 128]): output keeps batch and time, n_out channels."""
    from brainmagick_amd.models import DeepMel
    torch.manual_seed(0)
    features = torch.randn(2, 8, 128).cuda()
    model = DeepMel(8, 3, 5, 2, kernel=3, stride=1, dilation_growth=2, dilation_period=5, batch_norm=True,
                    activation_on_last=False, skip=True, glu_context=1, glu=2).cuda()
    out = model(features)
    assert len(model.sequence) == 5
    assert out.shape == (features.shape[0], 2, features.shape[2])


def test_gradients_collected_by_copy_equal_accumulated_ones():
    """FlatAdam.zero_grad(set_to_none=True) + collect_grads() (what Solver.train_step does: autograd hands its
    gradient tensors over, one multi-tensor copy moves them into the flat bucket) gives bit-identical buckets to
    torch-style accumulation into the bucket views; parameters that got no gradient read as zero."""
    from brainmagick_amd.solver import Solver
    model, _ = _small_model(merger_dropout=0.0)
    solver = Solver(model)
    opt = solver.optimizer
    sb = synthetic.make_batch(4, 20, 40, 10, 3, seed=8)

    def loss_of():
        estimate, output, mask, _ = solver._process_batch(sb, training=True)
        return solver.loss(estimate, output, mask)

    opt.zero_grad()
    loss_of().backward()
    accumulated = opt.flat_grad.clone()
    opt.flat_grad.fill_(7.0)                                        # stale content must not survive
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in opt.params)
    loss_of().backward()
    opt.collect_grads()
    assert torch.equal(opt.flat_grad[:opt.numel], accumulated[:opt.numel])
    for p, off in zip(opt.params, opt.offsets):
        assert p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off
    # a parameter without a gradient reads as zero
    opt.zero_grad(set_to_none=True)
    opt.collect_grads()
    assert float(opt.flat_grad[:opt.numel].abs().max()) == 0.0


def test_replicas_with_per_rank_rejection_and_whole_node_negatives():
    """negatives="node" next to a ScaleReject that REJECTS (clip=False, bm/norm.py:335-343): the ranks end up with
    different numbers of segments; every rank still gathers equal blocks of the nominal batch size, the rejected rows
    are padding and ClipLoss masks them.  Loopback world 3; oracle = per-rank loss over the rank's kept segments
    against the kept candidates of all ranks (own ones first), gradients averaged over the ranks."""
    from loopback import run_replicas
    from brainmagick_amd import distrib
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    from brainmagick_amd.solver import Solver
    world, B = 3, 8
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=48, initial_linear=48, depth=2, merger_dropout=0.0)
    C, T, Fd, S, hidden = 24, 136, 10, 3, 48

    def build():
        torch.manual_seed(3)
        return SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S, **cfg)

    sd0 = copy.deepcopy(build().state_dict())
    recordings = synthetic.make_layouts(2, [C], torch.Generator().manual_seed(5))
    batches = [synthetic.make_batch(B, C, T, Fd, S, seed=90 + r, recordings=recordings) for r in range(world)]
    rejected = {0: [], 1: [2, 5], 2: [0, 1, 7]}                 # rank -> segments pushed over the limit
    for r, rows in rejected.items():
        for i in rows:
            batches[r].meg[i, 3, 10] = 19.0                      # > limit 16 (the synthetic clamp is +-20)
    keep = [[i for i in range(B) if i not in rejected[r]] for r in range(world)]

    def body(r):
        model = build()
        scaler = DeviceBatchScaler(torch.zeros(2, C), torch.ones(2, C))
        solver = Solver(model, negatives="node", scale_reject=ScaleReject(scaler, limit=16, clip=False))
        loss = float(solver.train_step(batches[r]))
        opt = solver.optimizer
        lo, hi = distrib.shard_bounds(opt.padded, world, r)
        return dict(loss=loss, shard=(lo, hi), grad_shard=opt.flat_grad[lo:hi].clone().cpu(),
                    names=[k for k, _ in model.named_parameters()], offsets=list(opt.offsets))

    res = run_replicas(world, body)
    per_rank = []
    for r in range(world):
        sb = batches[r]
        own = sb.features[keep[r]]
        others = [batches[q].features[keep[q]] for q in range(world) if q != r]
        oracle = O.OracleModel(copy.deepcopy(sd0), cfg, hidden, Fd)
        loss, _, grads = oracle.loss_and_grads(sb.meg[keep[r]], sb.positions()[keep[r]], sb.subject_index[keep[r]],
                                               torch.cat([own] + others), True)
        assert abs(res[r]["loss"] - float(loss)) < LOSS_TOL, (r, res[r]["loss"], float(loss))
        per_rank.append(grads)
    mean = {n: sum(g[n] for g in per_rank) / world for n in per_rank[0]}
    full = torch.zeros(max(res[0]["offsets"]) + 10 ** 6, dtype=torch.float64)
    for n, off in zip(res[0]["names"], res[0]["offsets"]):
        full[off:off + mean[n].numel()] = mean[n].reshape(-1).double()
    for r in range(world):
        lo, hi = res[r]["shard"]
        assert rel_l2(res[r]["grad_shard"] / world, full[lo:hi]) < GRAD_TOL, r


def test_host_batches_staged_on_the_copy_stream_change_no_bit():
    """bm/solver.py:243: batches handed over as PINNED host tensors, the next one staged on the copy stream while the
    step runs (Solver.stage / train_step(next_batch=...)), and as pageable host tensors (blocking copies), against the
    same batches resident on the device.  Three steps each: losses and parameters must be bit-identical -- the copy
    stream changes when the bytes travel, never what is computed."""
    from brainmagick_amd.solver import Solver
    from brainmagick_amd.models import SimpleConv
    cfg = dict(O.CLIP_CONV_CFG)
    cfg.update(merger_pos_dim=128, merger_channels=96, initial_linear=96, depth=4, merger_dropout=0.0)
    C, T, Fd, S, hidden, B = 30, 160, 12, 4, 96, 16
    recordings = synthetic.make_layouts(2, [C], torch.Generator().manual_seed(9))
    host = [synthetic.make_batch(B, C, T, Fd, S, seed=300 + k, recordings=recordings) for k in range(4)]

    def run(mode):
        torch.manual_seed(0)
        model = SimpleConv(in_channels={"meg": C}, out_channels=Fd, hidden={"meg": hidden}, n_subjects=S, **cfg)
        solver = Solver(model)
        if mode == "resident":
            batches = [b.to("cuda") for b in host]
            losses = [float(solver.train_step(batches[k])) for k in range(3)]
        else:
            batches = [b.pin() for b in host] if mode == "pinned" else host
            assert batches[0].meg.is_pinned() == (mode == "pinned")
            losses = [float(solver.train_step(batches[k], next_batch=batches[k + 1])) for k in range(3)]
            assert solver._copy_stream is not None
        return losses, solver.optimizer.flat_param.clone()

    base_l, base_p = run("resident")
    for mode in ("pinned", "pageable"):
        l, p_ = run(mode)
        assert l == base_l, (mode, l, base_l)
        assert torch.equal(p_, base_p), mode


def test_flat_bucket_views_are_handed_out_only_inside_writing_grads():
    """a gradient that aliases the optimizer's flat bucket may only come out of the training step's own
    backward pass (`with optimizer.writing_grads()`); torch.autograd.grad for analysis gets fresh tensors."""
    from brainmagick_amd.solver import Solver
    model, _ = _small_model(merger_dropout=0.0)
    solver = Solver(model)
    opt = solver.optimizer
    sb = synthetic.make_batch(4, 20, 40, 10, 3, seed=8)
    lo, hi = opt.flat_grad.data_ptr(), opt.flat_grad.data_ptr() + 4 * opt.padded

    def loss_of():
        estimate, output, mask, _ = solver._process_batch(sb, training=True)
        return solver.loss(estimate, output, mask)

    opt.zero_grad(set_to_none=True)
    grads = torch.autograd.grad(loss_of(), opt.params, allow_unused=True)
    assert all(g is None or not (lo <= g.data_ptr() < hi) for g in grads)
    opt.zero_grad(set_to_none=True)
    with opt.writing_grads():
        loss_of().backward()
    inside = sum(1 for p in opt.params if p.grad is not None and lo <= p.grad.data_ptr() < hi)
    assert inside > 0, "no weight gradient was written straight into the bucket"
    opt.collect_grads()
    direct = opt.flat_grad.clone()
    opt.zero_grad(set_to_none=True)
    loss_of().backward()                              # outside the context: fresh tensors, collected by copy
    assert all(p.grad is None or not (lo <= p.grad.data_ptr() < hi) for p in opt.params)
    opt.collect_grads()
    assert torch.equal(opt.flat_grad, direct)


@pytest.mark.parametrize("how", ["two_micro_batches", "one_graph_uses_every_weight_twice", "second_backward_retained"])
def test_flat_bucket_accumulates_like_fresh_gradients(how):
    """One ``zero_grad(set_to_none=True)``, then under ONE ``writing_grads()``: two micro-batches (the bucket view is
    handed out once, the second backward accumulates into it through autograd), one graph in which every weight takes
    part twice, and a second backward over a retained graph.  ``flat_grad`` must equal, bit for bit, the fp32 sum of the
    two gradients taken with fresh tensors (``torch.autograd.grad`` outside the context) -- exactly twice the first
    gradient in the retained case."""
    from brainmagick_amd.solver import Solver
    model, _ = _small_model(merger_dropout=0.0)
    solver = Solver(model)
    opt = solver.optimizer
    batches = [synthetic.make_batch(4, 20, 40, 10, 3, seed=8 + k) for k in range(2)]
    if how == "second_backward_retained":
        batches[1] = batches[0]

    def loss_of(sb):
        estimate, output, mask, _ = solver._process_batch(sb, training=True)
        return solver.loss(estimate, output, mask)

    opt.zero_grad(set_to_none=True)
    fresh = [torch.autograd.grad(loss_of(sb), opt.params, allow_unused=True) for sb in batches]
    want = torch.zeros_like(opt.flat_grad)
    for p, off, g1, g2 in zip(opt.params, opt.offsets, *fresh):
        assert (g1 is None) == (g2 is None)
        if g1 is not None:
            want[off:off + p.numel()] = (g1 + g2).reshape(-1)
    lo, hi = opt.flat_grad.data_ptr(), opt.flat_grad.data_ptr() + 4 * opt.padded
    opt.zero_grad(set_to_none=True)
    with opt.writing_grads():
        if how == "two_micro_batches":
            loss_of(batches[0]).backward()
            inside = sum(1 for p in opt.params if p.grad is not None and lo <= p.grad.data_ptr() < hi)
            assert inside > 0, "no weight gradient was written straight into the bucket"
            loss_of(batches[1]).backward()
        elif how == "one_graph_uses_every_weight_twice":
            (loss_of(batches[0]) + loss_of(batches[1])).backward()
        else:
            loss = loss_of(batches[0])
            loss.backward(retain_graph=True)
            loss.backward()
    opt.collect_grads()
    assert torch.equal(opt.flat_grad, want), (how, (opt.flat_grad - want).abs().max().item())


def test_negative_pool_completes_the_candidates_like_the_reference():
    """bm/solver.py:358-371 (`optim.negatives`): a batch with fewer candidates than `n_negatives` is completed with
    a random draw (torch.randperm) from the pool of earlier candidate sets, and the pool takes the completed set in
    front, cut to `negative_pool_size`.  Restated here on the CPU with the same generator seed; the loss of each
    step against the oracle's ClipLoss over the completed candidates."""
    from brainmagick_amd.solver import Solver
    model, _ = _small_model(merger_dropout=0.0)
    n_neg, pool_size, B = 10, 14, 6
    solver = Solver(model, n_negatives=n_neg, negative_pool_size=pool_size)
    solver.negative_generator = torch.Generator().manual_seed(123)
    ref_gen = torch.Generator().manual_seed(123)
    buf = torch.zeros(0, 10, 40)
    for k in range(4):
        sb = synthetic.make_batch(B, 20, 40, 10, 3, seed=600 + k)
        with torch.no_grad():
            solver.model.train(False)
            estimate, output, mask, _ = solver._process_batch(sb, training=False)
            completed = solver._complete_with_pool(output, training=True)
        out_ref = sb.features
        n_kept = n_neg - len(out_ref)
        kept = torch.randperm(len(buf), generator=ref_gen)[:n_kept]
        out_ref = torch.cat([out_ref, buf[kept]], dim=0)
        buf = torch.cat([out_ref, buf])[:pool_size]
        assert torch.equal(completed.cpu(), out_ref), k
        assert torch.equal(solver.negative_pool["train"].cpu(), buf), k
        loss = solver.loss(estimate, completed, mask)
        assert abs(float(loss) - float(O.clip_loss(estimate.cpu(), out_ref))) < LOSS_TOL


@pytest.mark.parametrize("penalty", [False, True], ids=["clip", "clip+svd"])
@pytest.mark.parametrize("dtype", ["f16x2", "f32"])
def test_parameter_bucket_at_every_phase(dtype, penalty):
    """FlatAdam packs parameters and gradients without padding, so a parameter starts wherever the ones in front of it
    end: a ``k``-element parameter in front of the model's (k = 0..3, outside the graph) moves every weight, bias and
    gradient view by 4 k bytes, through all four phases of a 16-byte boundary.  The kernels read the weights in place,
    the weight-gradient kernels store straight into the bucket views (``grad_destination``), ``spectral.hip`` reads
    the matrices in place (``penalty``: with ``svd_penalty`` over the model's weights).  One training step per k from
    the same weights: loss, estimate, every gradient, both Adam moments and every updated parameter are the same bits
    whatever k -- no kernel chooses a path, or a summation order, by a parameter's address.  The k = 0 run meets the
    CPU oracle (which has no penalty: with it only the estimate is held to the oracle)."""
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.optim import FlatAdam
    from brainmagick_amd.svd import penalized_weights, svd_penalty
    B, C, T, Fd, S, hidden = 12, 20, 48, 10, 3, 32
    sb = synthetic.make_batch(B, C, T, Fd, S, n_layouts=2)
    sbg = sb.to("cuda")
    model0, cfg = _small_model(merger_dropout=0.0)
    sd0 = copy.deepcopy(model0.state_dict())
    gen = torch.Generator().manual_seed(17)
    mats = [torch.randn(min(w.shape[0], w.numel() // w.shape[0]), 16, generator=gen)
            for _, w in penalized_weights(model0)]
    assert len(mats) >= 5
    runs = []
    H.set_compute_dtype(dtype)
    try:
        for k in range(4):
            model, _ = _small_model(merger_dropout=0.0)
            model.load_state_dict(sd0)
            model = model.cuda().train()
            pad = [torch.nn.Parameter(torch.zeros(k, device="cuda"))] if k else []
            opt = FlatAdam(pad + list(model.parameters()), lr=3e-4, betas=(0.9, 0.999))
            named = dict(model.named_parameters())
            assert opt.flat_param.data_ptr() % 16 == 0 and opt.flat_grad.data_ptr() % 16 == 0
            opt.zero_grad(set_to_none=True)
            est = model({"meg": sbg.meg.clone()}, sbg)
            loss = ClipLoss().cuda().train()(est, sbg.features, sbg.features_mask)
            if penalty:
                loss = loss + 0.1 * svd_penalty(model, test_matrices=mats)
            with opt.writing_grads():
                loss.backward()
            where = {n: (p.data_ptr() - opt.flat_param.data_ptr(), p.grad.data_ptr() - opt.flat_grad.data_ptr())
                     for n, p in named.items()}
            # the weight-gradient kernels stored straight into the bucket views: handed out by grad_destination, and
            # (without the penalty, which uses every matrix a second time and so makes autograd add) adopted as p.grad
            handed = [n for n, p in named.items() if p.dim() > 1 and p._bm_grad_dst[1][0]]
            direct = [n for n in handed if where[n][1] == where[n][0]]
            assert handed and (penalty or direct), "no weight gradient was written straight into the bucket"
            opt.step()
            for n, p in named.items():          # after the step every gradient is its view of the bucket
                assert p.grad.data_ptr() - opt.flat_grad.data_ptr() == where[n][0], n
            torch.cuda.synchronize()
            runs.append(dict(where=where, loss=loss.detach().clone(), est=est.detach().clone(),
                             grad={n: p.grad.clone() for n, p in named.items()},
                             m1={n: opt.state[p]["exp_avg"].clone() for n, p in named.items()},
                             m2={n: opt.state[p]["exp_avg_sq"].clone() for n, p in named.items()},
                             param={n: p.detach().clone() for n, p in named.items()}))
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
    base = runs[0]
    # the weights of the k = 0 run already sit at more than one phase, and every k moves all of them by 4 k bytes
    assert len({off % 16 for n, (off, _) in base["where"].items() if base["param"][n].dim() > 1}) > 1
    for k, run in enumerate(runs):
        for n, (off, _) in run["where"].items():
            assert off == base["where"][n][0] + 4 * k, (k, n)
    for k, run in enumerate(runs[1:], 1):
        assert torch.equal(run["loss"], base["loss"]), (k, float(run["loss"]), float(base["loss"]))
        assert torch.equal(run["est"], base["est"]), k
        for what in ("grad", "m1", "m2", "param"):
            for n in base[what]:
                assert torch.equal(run[what][n], base[what][n]), \
                    (f"{what} of {n} differs in bits with the bucket moved by {4 * k} bytes: "
                     f"rel-L2 {rel_l2(run[what][n], base[what][n]):.3e}")
    oracle = O.OracleModel(copy.deepcopy(sd0), cfg, hidden, Fd)
    loss_ref, est_ref, grads_ref = oracle.loss_and_grads(sb.meg, sb.positions(), sb.subject_index, sb.features, True)
    assert rel_l2(base["est"], est_ref) < FWD_TOL, rel_l2(base["est"], est_ref)
    if not penalty:
        assert abs(float(base["loss"]) - float(loss_ref)) < LOSS_TOL
        gscale = max(v.double().norm().item() for v in grads_ref.values())
        for n, g in base["grad"].items():
            assert close(g, grads_ref[n], GRAD_TOL, gscale), (n, rel_l2(g, grads_ref[n]))
