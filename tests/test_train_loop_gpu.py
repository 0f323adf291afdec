"""``Solver.run_epoch`` / ``fit`` / ``restore`` on the GPU (brainmagick_amd/train_loop.py) over resident segments: the loop
adds nothing to the steps it is made of.  Every comparison is ``torch.equal`` on ``state_dict()`` tensors (model,
BatchNorm buffers, Adam moments and step) and ``==`` on losses, against hand loops of ``train_step(batch, next_batch)`` /
``eval_step(batch)`` on a twin solver built from the same seed: no tolerance is involved.

The set-up is the smallest that has every edge: two recordings of 500 and 470 samples, 8 sensors, 8 feature channels,
windows of T = 37, 25 segments in batches of 7 (four batches, the last one of 4 and across the recordings' border), a
SimpleConv of hidden 16 and depth 2 without dropout, unshuffled loaders, the default f16x2 mode (f32 where noted)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SR = 120.
LENGTHS = (500, 470)
BATCH = 7
LIMIT = 6.0
CFG = dict(depth=2, kernel_size=3, dilation_period=5, batch_norm=True, skip=True, gelu=True, glu=2, glu_context=1,
           complex_out=True, merger=False, initial_linear=16, subject_layers=True, subject_dim=0)


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def make_segments(spikes=(), nans=()):
    """``spikes`` / ``nans``: segment numbers whose window gets one MEG sample past the ScaleReject limit / one NaN
    feature sample, 20 samples into the window: behind the baseline, and inside no neighbouring window."""
    import numpy as np
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    onsets = np.arange(20, 460, 36) / SR

    def build(marks):
        g = torch.Generator().manual_seed(11)
        recs = []
        for i, n in enumerate(LENGTHS):
            meg = torch.randn(8, n, generator=g).clamp(-3, 3)
            features = torch.randn(8, n, generator=g)
            for r, s, value in marks:
                if r == i:
                    (features if value != value else meg)[0, s] = value
            recs.append(DeviceRecording(meg.cuda(), features.cuda(), torch.ones(1, n, dtype=torch.bool).cuda(),
                                        recording=Recording(i, torch.rand(8, 2, generator=g)), subject_index=i))
        return DeviceSegments(recs, SR, tmin=-0.1, tmax=0.2, condition=onsets, meg_dimension=8)
    plain = build([])
    assert plain.T == 37 and len(plain) == 25 and int((plain.rec == 0).sum()) == 13
    if not spikes and not nans:
        return plain
    marks = [(int(plain.rec[i]), int(plain.start[i]) + 20, 50.0) for i in spikes] + \
            [(int(plain.rec[i]), int(plain.start[i]) + 20, float("nan")) for i in nans]
    return build(marks)


def loader_of(seg):
    from brainmagick_amd.dataset import DeviceSegmentLoader
    loader = DeviceSegmentLoader(seg, BATCH)
    assert len(loader) == 4
    return loader


def make_solver(kind="clip", reject=False):
    from brainmagick_amd.losses import ClipLoss, L1Loss, L2Loss
    from brainmagick_amd.models import ConvRNN, SimpleConv
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    from brainmagick_amd.solver import Solver
    torch.manual_seed(0)
    kw = {}
    if reject:
        kw["scale_reject"] = ScaleReject(DeviceBatchScaler(torch.zeros(2, 8), torch.ones(2, 8)), limit=LIMIT, clip=False)
    if kind == "encode_l1":
        model = ConvRNN(in_channels={"meg": 8, "features": 8}, out_channels=8, hidden={"meg": 16, "features": 8},
                        n_subjects=2, lstm=1)
        return Solver(model, L1Loss(), task="encode", meg_init=0.1, sample_rate=SR, **kw)
    model = SimpleConv(in_channels={"meg": 8}, out_channels=8, hidden={"meg": 16}, n_subjects=2, **CFG)
    if kind == "l2":
        return Solver(model, L2Loss(), sample_rate=SR, **kw)
    if kind == "clip_negatives":
        solver = Solver(model, ClipLoss(), sample_rate=SR, n_negatives=10, **kw)
        solver.negative_generator = torch.Generator().manual_seed(5)
        return solver
    return Solver(model, ClipLoss(), sample_rate=SR, **kw)


def bits(solver):
    """Every tensor of ``state_dict()``, cloned: model (BatchNorm buffers and counters included), Adam moments and step."""
    state = solver.state_dict()
    out = {f"model/{k}": v.detach().clone() for k, v in state["model"].items()}
    for i, st in state["optimizer"]["state"].items():
        for k, v in st.items():
            out[f"adam/{i}/{k}"] = v.detach().clone() if isinstance(v, torch.Tensor) else torch.tensor(v)
    assert any(k.endswith("exp_avg_sq") for k in out)
    return out


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def differ(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a)


def hand_train(solver, batches, look_ahead=True):
    """The parent's way of training: the bare step over the batches."""
    losses = []
    for i, batch in enumerate(batches):
        following = batches[i + 1] if look_ahead and i + 1 < len(batches) else None
        losses.append(solver.train_step(batch, following))
    return [float(x) for x in losses]


def hand_valid(solver, batches):
    return [float(solver.eval_step(b)) for b in batches]


def mean64(values):
    total = 0.0
    for v in values:
        total += v
    return total / len(values)


def count_reads(monkeypatch, solver):
    """(reads, steps): every ``read_losses`` call as (steps taken so far, slots read)."""
    from brainmagick_amd import train_loop
    reads, steps = [], []
    real_read, real_step, real_eval = train_loop.read_losses, solver.train_step, solver._eval_loss
    monkeypatch.setattr(train_loop, "read_losses", lambda r, n: reads.append((len(steps), n)) or real_read(r, n))
    solver.train_step = lambda batch, next_batch=None: steps.append(next_batch) or real_step(batch, next_batch)
    solver._eval_loss = lambda batch: steps.append("eval") or real_eval(batch)
    return reads, steps


def test_training_epoch_equals_the_hand_loop(monkeypatch):
    seg = make_segments()
    twin, solver = make_solver(), make_solver()
    before = bits(solver)
    losses = hand_train(twin, list(loader_of(seg)))
    reads, steps = count_reads(monkeypatch, solver)
    got = solver.run_epoch(loader_of(seg), True)
    assert got == {"loss": mean64(losses)} and len(set(losses)) == 4
    assert reads == [(4, 4)]                                      # once, after the last step
    assert [s is None for s in steps] == [False, False, False, True]
    assert solver._prefetched is None and solver.history == [] and solver.best_state is None
    assert_same(bits(solver), bits(twin))
    assert differ(bits(solver), before)


def test_max_batches_takes_two_steps_and_leaves_nothing_behind(monkeypatch):
    seg = make_segments()
    twin, solver = make_solver(), make_solver()
    batches = list(loader_of(seg))
    cut = hand_train(twin, batches[:2])                           # ... a solver that never saw the cut
    reads, steps = count_reads(monkeypatch, solver)
    got = solver.run_epoch(loader_of(seg), True, max_batches=2)
    assert got == {"loss": mean64(cut)} and len(steps) == 2 and steps[1] is None and reads == [(2, 2)]
    assert solver._prefetched is None and not solver._staged and solver._gather is None
    assert_same(bits(solver), bits(twin), "after the cut epoch")
    assert solver.run_epoch(loader_of(seg), True) == twin.run_epoch(loader_of(seg), True)
    assert_same(bits(solver), bits(twin), "after the following epoch")


def test_a_rejected_middle_batch_is_the_hand_made_substitution():
    seg = make_segments(spikes=range(7, 14))                      # the whole second batch, across the recordings' border
    batches = list(loader_of(seg))
    substituted = [batches[0], batches[0], batches[2], batches[3]]
    twin, solver = make_solver(reject=True), make_solver(reject=True)
    with torch.no_grad():
        probe = make_solver(reject=True)
        assert probe._process_batch(batches[1])[0] is None and probe._process_batch(batches[2])[0] is not None
    losses = hand_train(twin, substituted, look_ahead=False)
    assert solver.run_epoch(loader_of(seg), True) == {"loss": mean64(losses)}
    assert_same(bits(solver), bits(twin), "training")
    valid = hand_valid(twin, substituted)
    assert solver.run_epoch(loader_of(seg), False) == {"loss": mean64(valid)}
    assert valid[0] == valid[1] and solver.best_loss == mean64(valid)
    assert_same(bits(solver), bits(twin), "validation")
    assert solver.scale_reject.rejection_rate > 0


@pytest.mark.parametrize("training", [True, False])
def test_a_rejected_first_batch_raises(training):
    seg = make_segments(spikes=range(0, 7))
    solver = make_solver(reject=True)
    solver.train_step(next(iter(loader_of(make_segments()))))     # an earlier epoch's last good batch does not count
    before = bits(solver)
    with pytest.raises(RuntimeError, match="Empty batch and last batch is none"):
        solver.run_epoch(loader_of(seg), training)
    assert_same(bits(solver), before)
    assert solver._prefetched is None and solver.history == [] and solver.best_state is None


def test_validation_epoch_touches_nothing_and_best_state_is_a_clone(monkeypatch):
    seg = make_segments()
    twin, solver = make_solver(), make_solver()
    batches = list(loader_of(seg))
    hand_train(twin, batches[:2]), hand_train(solver, batches[:2])
    before = bits(solver)
    modes = []
    solver.model.register_forward_pre_hook(lambda m, a: modes.append((m.training, torch.is_grad_enabled())))
    reads, steps = count_reads(monkeypatch, solver)
    got = solver.run_epoch(loader_of(seg), False)
    assert got == {"loss": mean64(hand_valid(twin, batches))}
    assert modes == [(False, False)] * 4 and reads == [(4, 4)] and steps == ["eval"] * 4
    assert_same(bits(solver), before)
    # the best state: the models' tensors, cloned
    assert solver.best_loss == got["loss"] and solver.best_epoch == 1
    live = solver.model.state_dict()
    best = solver.best_state["model"]
    assert best.keys() == live.keys() and all(torch.equal(best[k], live[k]) for k in live)
    assert all(best[k].data_ptr() != live[k].data_ptr() for k in live if live[k].numel())
    kept = {k: v.clone() for k, v in best.items()}
    hand_train(solver, batches[2:])
    assert all(torch.equal(best[k], kept[k]) for k in kept)
    assert any(not torch.equal(best[k], solver.model.state_dict()[k]) for k in kept)
    solver.best_on = "cpu"
    solver.best_loss = float("inf")
    solver.run_epoch(loader_of(seg), False)
    assert all(v.device.type == "cpu" for v in solver.best_state["model"].values())
    assert all(torch.equal(solver.best_state["model"][k].cuda(), v) for k, v in solver.model.state_dict().items())


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_fit_tests_on_the_best_state_and_trains_on_as_if_it_had_not(H, mode):
    """No packed weight plane or cached maximum survives a swap: the stage's forward pass sees the best weights (a fresh
    solver that holds them computes the same loss), and the next training epochs the live ones (bit for bit a run that
    had no test stage)."""
    from brainmagick_amd import train_loop
    H.set_compute_dtype(mode)
    try:
        seg = make_segments()
        probe = next(iter(loader_of(seg)))
        twin, solver = make_solver(), make_solver()
        seen = []

        def test():
            assert not torch.is_grad_enabled() and not differ(solver.best_state["model"], solver.model.state_dict())
            seen.append((solver.epoch, {k: v.clone() for k, v in solver.best_state["model"].items()},
                         float(solver.eval_step(probe))))
            return {"probe": seen[-1][2]}
        history = solver.fit(loader_of(seg), loader_of(seg), epochs=3, test=test)
        plain = twin.fit(loader_of(seg), loader_of(seg), epochs=3)
        assert len(history) == 3 and seen and seen[0][0] == 1 and "test" in history[0]
        assert [{k: v for k, v in h.items() if k != "test"} for h in history] == plain
        assert solver.last_test_epoch == seen[-1][0] and twin.last_test_epoch == 0
        assert_same(bits(solver), bits(twin), "after three epochs")      # the live state came back, bit for bit
        # the stage ran on the best weights: a fresh solver that holds them computes the same loss
        for epoch, best, loss in seen:
            fresh = make_solver()
            train_loop.load_model_state(fresh, {"model": best})
            assert float(fresh.eval_step(probe)) == loss, epoch
        assert differ(seen[0][1], solver.model.state_dict())
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


def test_checkpoint_restore_continues_bit_for_bit(tmp_path):
    seg = make_segments()
    path = tmp_path / "checkpoint.th"
    whole, first = make_solver(), make_solver()
    whole.fit(loader_of(seg), loader_of(seg), epochs=3)
    first.fit(loader_of(seg), loader_of(seg), epochs=2, checkpoint=path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint.th"]
    second = make_solver()
    with torch.no_grad():
        for p in second.model.parameters():
            p.add_(1.0)                                           # whatever it held is overwritten
    assert second.restore(path) is True
    assert second.epoch == 3 and second.history == first.history == whole.history[:2]
    assert_same(bits(second), bits(first), "restored")
    assert (second.best_loss, second.best_epoch, second.last_test_epoch) == \
        (first.best_loss, first.best_epoch, first.last_test_epoch)
    assert not differ(second.best_state["model"], first.best_state["model"])
    assert all(v.is_cuda for v in second.best_state["model"].values())
    assert second.fit(loader_of(seg), loader_of(seg), epochs=3) == whole.history
    assert_same(bits(second), bits(whole), "resumed")
    assert (second.best_loss, second.best_epoch) == (whole.best_loss, whole.best_epoch)


def test_continue_from_loads_the_models_only(tmp_path):
    from brainmagick_amd import train_loop
    seg = make_segments()
    path = tmp_path / "other_run.th"
    source = make_solver()
    source.fit(loader_of(seg), loader_of(seg), epochs=1)
    source.run_epoch(loader_of(seg), True)                        # the live state moves on; the best one stays
    train_loop.save_checkpoint(source, path)
    live, best = source.model.state_dict(), source.best_state["model"]
    assert differ(live, best)
    for continue_best, want in ((True, best), (False, live)):
        solver = make_solver()
        fresh = bits(solver)
        assert solver.restore(tmp_path / "checkpoint.th", continue_from=path, continue_best=continue_best) is False
        assert not differ(solver.model.state_dict(), want)
        assert solver.history == [] and solver.best_state is None and solver.best_epoch == 0 and solver.epoch == 1
        after = bits(solver)
        assert all(torch.equal(after[k], fresh[k]) for k in after if k.startswith("adam/"))
        # the loaded weights are the ones the next forward pass uses
        probe = next(iter(loader_of(seg)))
        holder = make_solver()
        train_loop.load_model_state(holder, {"model": want})
        assert float(solver.eval_step(probe)) == float(holder.eval_step(probe))


def test_a_deferred_assert_propagates_and_leaves_the_state_of_step_2():
    seg = make_segments(nans=[15])                                # a NaN feature sample in the third batch
    clean = list(loader_of(make_segments()))                      # the same first two batches, and no NaN behind them
    twin, solver = make_solver(), make_solver()
    twin.train_step(clean[0], clean[1])
    twin.train_step(clean[1], clean[2])
    solver.history.append({"train": {"loss": 1.0}, "valid": {"loss": 0.5}})
    solver.best_loss, solver.best_epoch = 0.5, 1
    solver.best_state = {"model": {"marker": torch.zeros(1)}}
    best = solver.best_state
    with pytest.raises(AssertionError, match="non-finite"):
        solver.fit(loader_of(seg), loader_of(seg), epochs=2)
    torch.cuda.synchronize()
    assert_same(bits(solver), bits(twin))
    assert solver.history == [{"train": {"loss": 1.0}, "valid": {"loss": 0.5}}]
    assert (solver.best_loss, solver.best_epoch, solver.last_test_epoch) == (0.5, 1, 0) and solver.best_state is best
    assert solver._prefetched is None and not solver._staged


@pytest.mark.parametrize("kind", ["l2", "encode_l1", "clip_negatives"])
def test_every_objective_against_its_hand_loops(kind):
    seg = make_segments()
    batches = list(loader_of(seg))
    twin, solver = make_solver(kind), make_solver(kind)
    train = hand_train(twin, batches)
    assert solver.run_epoch(loader_of(seg), True) == {"loss": mean64(train)}
    assert_same(bits(solver), bits(twin), "training")
    valid = hand_valid(twin, batches)
    assert solver.run_epoch(loader_of(seg), False) == {"loss": mean64(valid)}
    assert_same(bits(solver), bits(twin), "validation")
    if kind == "clip_negatives":
        for phase in ("train", "valid"):
            assert torch.equal(solver.negative_pool[phase], twin.negative_pool[phase])
        assert solver.negative_generator.get_state().equal(twin.negative_generator.get_state())
