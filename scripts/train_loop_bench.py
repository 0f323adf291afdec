"""The training loop measured beside the steps it is made of: ``Solver.run_epoch`` (brainmagick_amd/train_loop.py) against
the bare ``train_step(batch, next_batch)`` / ``eval_step(batch)`` loops over the same ``DeviceSegmentLoader`` -- the way to
train before there was an epoch.  No threshold: the comparison is the hand loop on the same device, and its own
run-to-run spread is the yardstick.

    python scripts/train_loop_bench.py [--out profiles/train_loop_vs_steps.txt] [--reps 5]

cfg2 shapes (208 MEG channels, 120 feature channels, windows of 360 samples), batches of 256, 12 batches per epoch over
one resident recording, the paper's SimpleConv (hidden 320), ClipLoss, the default f16x2 mode, one card.

(a) a training epoch: ``run_epoch(loader, True)`` beside the hand loop with the same look-ahead; host clock around the
    epoch, which ends in a device synchronise; per step.
(b) a validation epoch: ``run_epoch(loader, False)`` beside the loop of ``eval_step``; per batch.  ``best_loss`` is held at
    -inf, so no epoch clones a best state: that is (c).
(c) one ``best_state`` clone (on the device, and to the host with ``best_on="cpu"``) and one ``swap_state`` round trip
    (clone of the live state, two loads); host clock and a synchronise.
(d) one checkpoint write (``state_dict()`` with the Adam moments, the temporary file, the rename); host clock.

Everything is warmed up; the repetitions of the implementations alternate; medians are reported.  The measurement runs
in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

B, MEG, F, SR = 256, 208, 120, 120.
BATCHES = 12


def _median(v):
    return sorted(v)[len(v) // 2]


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(impls, reps, scale=1.0):
    import torch
    for fn in impls.values():
        fn()
        torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(_clock(fn) / scale)
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), n=len(v)) for k, v in times.items()}


def make_segments():
    import numpy as np
    import torch
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.synthetic import Recording
    g = torch.Generator().manual_seed(7)
    onset = 64 + 8 * np.arange(B * BATCHES)
    n = int(onset[-1]) + 320
    rec = DeviceRecording(torch.randn(MEG, n, generator=g).cuda(), torch.randn(F, n, generator=g).cuda(),
                          torch.ones(1, n, dtype=torch.bool).cuda(), recording=Recording(0, torch.rand(MEG, 2, generator=g)),
                          subject_index=0)
    return DeviceSegments([rec], SR, tmin=-0.5, tmax=2.49, condition=onset / SR, meg_dimension=MEG)


def measure(reps: int) -> dict:
    import torch
    from brainmagick_amd import train_loop
    from brainmagick_amd.dataset import DeviceSegmentLoader
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from oracle import bm_oracle as O
    seg = make_segments()
    loader = DeviceSegmentLoader(seg, B)
    out = dict(device=torch.cuda.get_device_name(0), T=seg.T, batches=len(loader), segments=len(seg))
    assert len(loader) == BATCHES and seg.T == 360
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": MEG}, out_channels=F, hidden={"meg": 320}, n_subjects=1,
                       **dict(O.CLIP_CONV_CFG))
    solver = Solver(model, ClipLoss())
    res = {}

    def epoch_train():
        res["train"] = solver.run_epoch(loader, True)["loss"]

    def hand_train():
        it = iter(loader)
        batch = next(it)
        while batch is not None:
            following = next(it, None)
            loss = solver.train_step(batch, following)
            batch = following
        res["hand_train"] = loss

    def epoch_valid():
        solver.best_loss = -float("inf")
        res["valid"] = solver.run_epoch(loader, False)["loss"]

    def hand_valid():
        for batch in loader:
            loss = solver.eval_step(batch)
        res["hand_valid"] = loss
    keys = ("bm: run_epoch(loader, True)", "the hand loop: train_step(batch, next_batch)")
    out["train"] = interleaved(dict(zip(keys, (epoch_train, hand_train))), reps, BATCHES)
    keys = ("bm: run_epoch(loader, False)", "the hand loop: eval_step(batch)")
    out["valid"] = interleaved(dict(zip(keys, (epoch_valid, hand_valid))), reps, BATCHES)
    hand =[float(solver.eval_step(b)) for b in loader]
    out["valid_equal"] = bool(res["valid"] == train_loop.sequential_mean(hand))
    out["loss_finite"] = bool(res["train"] == res["train"] and abs(res["train"]) != float("inf"))

    # (c) the clones and the swap
    state = train_loop.copy_state(train_loop.model_state(solver))
    out["state_bytes"] = int(sum(v.numel() * v.element_size() for part in state.values() for v in part.values()))

    def swap():
        with train_loop.swap_state(solver, state):
            pass
    out["state"] = interleaved({
        "best_state clone on the device": lambda: train_loop.copy_state(train_loop.model_state(solver)),
        "best_state clone to the host (best_on = 'cpu')": lambda: train_loop.copy_state(train_loop.model_state(solver), "cpu"),
        "swap_state round trip (clone, load, load back)": swap}, reps)

    # (d) the checkpoint
    solver.best_state = state
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "checkpoint.th"
        out["checkpoint"] = interleaved({"save_checkpoint (state_dict, temporary file, rename)":
                                         lambda: train_loop.save_checkpoint(solver, path)}, reps)
        out["checkpoint_bytes"] = path.stat().st_size
    return out


def _row(label, v, width=58):
    return f"  {label:{width}s} {v['median_ms']:10.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]  n = {v['n']}"


def _verdict(ours, hand, what):
    spread = hand["max_ms"] - hand["min_ms"]
    diff = ours["median_ms"] - hand["median_ms"]
    ratio = ours["median_ms"] / hand["median_ms"]
    if diff <= spread:
        return (f"  bm / hand loop   x{ratio:.3f}   ({diff:+.3f} ms per {what}: inside the hand loop's own run-to-run spread of "
                f"{spread:.3f} ms)")
    return (f"  bm / hand loop   x{ratio:.3f}   (bm is SLOWER by {diff:.3f} ms per {what}, {100 * (ratio - 1):.1f} %: outside "
            f"the hand loop's own run-to-run spread of {spread:.3f} ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_loop_vs_steps.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps)))
        return
    cmd = ["timeout", "-k", "10", "400", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"train_loop_bench: the measurement ended with status {proc.returncode}")
    r = json.loads(proc.stdout.strip().splitlines()[-1])
    t_ours, t_hand = r["train"].values()
    v_ours, v_hand = r["valid"].values()
    lines = [f"The training loop beside the steps it is made of, {r['device']}: cfg2 shapes ({MEG} MEG channels, {F} feature",
             f"channels, windows of {r['T']} samples), batches of {B}, {r['batches']} batches per epoch over one resident "
             f"recording ({r['segments']} segments),",
             "SimpleConv of the paper's size (hidden 320), ClipLoss, f16x2, one card.  No threshold: the hand loop on the same",
             "device is the comparison.  Implementations alternate, medians after warm-up [min .. max], milliseconds.", "",
             "(a) A training epoch, per step; host clock around the epoch and a device synchronise:"]
    lines += [_row(name, v) for name, v in r["train"].items()]
    lines += [_verdict(t_ours, t_hand, "step"), f"  the epoch's loss is finite: {r['loss_finite']}.", "",
              "(b) A validation epoch, per batch (best_loss held at -inf: no clone inside):"]
    lines += [_row(name, v) for name, v in r["valid"].items()]
    lines += [_verdict(v_ours, v_hand, "batch"),
              f"  run_epoch's loss equals the sequential fp64 mean of the eval_step losses: {r['valid_equal']}.", "",
              f"(c) The models' state ({r['state_bytes'] / 1e6:.1f} MB), per call; host clock and a synchronise:"]
    lines += [_row(name, v) for name, v in r["state"].items()]
    lines += ["", f"(d) The checkpoint ({r['checkpoint_bytes'] / 1e6:.1f} MB on disk: the models, the Adam moments, the best state), "
              "per write; host clock:"]
    lines += [_row(name, v) for name, v in r["checkpoint"].items()]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
