"""The ClipLoss test epoch measured: ``hip_ops.word_hash_pick`` (csrc/wer.hip), ``retrieval.collect_wer`` and
``retrieval.wer_epoch`` beside the reference's way of doing the same on the same device.

    python scripts/wer_epoch_bench.py [--out profiles/wer_epoch_vs_torch.txt] [--reps 5]

1. The pick launch at B = 256, T = 361, F_all = 121 with every fifth row rejected, beside the torch chain of
   bm/wer.py:48, 58-64 (the channel slice, the boolean index per candidate and four ``torch.where``).  A timed repetition
   is 50 calls between two HIP events.
2. The collection over the 4 000 word windows of one recording (208 MEG channels, 120 mel channels + WordHash, paper-sized
   SimpleConv, batches of 256), beside the same loop with the reference's ``.cpu()`` of every estimate and output, its
   torch chain and its three ``torch.cat`` -- and beside the loop that only runs ``_process_batch``: what the collection
   adds to the forward passes.  Host clock around the loop, which ends in a device synchronise.
3. The full epoch with ranking over 10 000 windows of three recordings at 10 000 negatives.

Everything is warmed up; the repetitions of the implementations alternate; medians are reported.  The measurement runs
in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

B, T, F_ALL, MEG, SR = 256, 361, 121, 208, 120.
WORDS = (4000, 3000, 3000)
CALLS = 50


def _median(v):
    return sorted(v)[len(v) // 2]


def _events(fn, calls):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _clock(fn, calls=1):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(impls, reps, timer, calls=1):
    import torch
    for fn in impls.values():
        fn()
        torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(timer(fn, calls))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), n=len(v)) for k, v in times.items()}


def torch_chain(features, channel, t0, reject_mask):
    """bm/wer.py:48, 58-64 as written."""
    import torch
    word_hash = features[:, channel:channel + 1][:, 0]
    wh = word_hash[reject_mask][:, t0]
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 - 1], wh)
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 + 1], wh)
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 - 2], wh)
    wh = torch.where(wh == 0, word_hash[reject_mask][:, t0 + 2], wh)
    return wh


def make_segments():
    import numpy as np
    import torch
    from brainmagick_amd.dataset import DeviceRecording, DeviceSegments
    from brainmagick_amd.features import DeviceEvents, DeviceFeaturesBuilder, EventFeature
    from brainmagick_amd.synthetic import Recording
    builder = DeviceFeaturesBuilder([EventFeature("MelSpectrum", "resampled", "sound", 120, default_value=-5.0),
                                     EventFeature("WordHash", "constant", "word", cardinality=1001)], SR)
    rng = np.random.default_rng(7)
    g = torch.Generator().manual_seed(7)
    recs, onsets = [], {}
    for i, n_words in enumerate(WORDS):
        onset = 60 + 36 * np.arange(n_words)                               # a word every 0.3 s
        n = int(onset[-1]) + 320                                            # no room for a window behind the last word
        mel = torch.randn(120, n, generator=g)
        events = dict(sound=dict(start=np.array([0.0]), duration=np.array([n / SR]), MelSpectrum=[mel]),
                      word=dict(start=onset / SR, duration=rng.integers(1, 30, n_words) / SR,
                                WordHash=rng.integers(1, 1001, n_words).astype(np.float64)))
        recs.append(DeviceRecording(torch.randn(MEG, n, generator=g).cuda(), events=DeviceEvents(builder, events),
                                    recording=Recording(i, torch.rand(MEG, 2, generator=g)), subject_index=i))
        onsets[i] = onset / SR
    # the windows are the word onsets: every recording has a word every 0.3 s from 0.5 s on, the longest one's onsets
    # are the condition and a shorter recording keeps the windows that fit into it
    seg = DeviceSegments(recs, SR, tmin=-0.5, tmax=2.5, condition=onsets[0], meg_dimension=MEG)
    return seg, builder


def measure(reps: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd import retrieval
    from brainmagick_amd.dataset import DeviceSegmentLoader
    from brainmagick_amd.losses import ClipLoss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    from oracle import bm_oracle as O
    out = dict(device=torch.cuda.get_device_name(0))

    # 1. the pick launch
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, F_ALL, T, generator=gen)
    x[:, 120] = torch.randint(0, 50, (B, T), generator=gen).float()
    x = x.cuda()
    keep = (torch.arange(B) % 5 != 0).cuda()
    n_keep = int(keep.sum())
    dest = torch.zeros(B, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    t0 = retrieval.check_at_time(-0.5, SR)
    res = {}

    def pick_ours():
        H.word_hash_pick(x, 120, t0, keep, dest, 0, flag, count=n_keep)

    def pick_torch():
        res["wh"] = torch_chain(x, 120, t0, keep)
    out["pick"] = interleaved({"bm: word_hash_pick (one launch)": pick_ours,
                               "torch ops: slice, 5 boolean indices, 4 where": pick_torch}, reps, _events, CALLS)
    out["pick_equal"] = bool(torch.equal(dest[:n_keep], res["wh"].long()))
    out["t0"], out["n_keep"] = t0, n_keep

    # 2. the collection
    seg, builder = make_segments()
    out["n_total"], out["T"] = len(seg), seg.T
    one = seg.only(0)
    out["n_collect"] = len(one)
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": MEG}, out_channels=120, hidden={"meg": 320}, n_subjects=len(WORDS),
                       **dict(O.CLIP_CONV_CFG))
    solver = Solver(model, ClipLoss())
    for m in solver._all_models():
        m.train(False)
    names = ["MelSpectrum"]

    def loader_of(segments):
        return DeviceSegmentLoader(segments, B, shuffle=True, generator=torch.Generator().manual_seed(3))

    def collect_ours():
        res["ours"] = retrieval.collect_wer(solver, loader_of(one), len(one), builder, names, t0)

    def collect_cpu():
        est, outs, hashes = [], [], []
        with torch.no_grad():
            for batch in loader_of(one):
                features = builder.extract_features(batch.features, names)
                estimate, output, _, reject_mask = solver._process_batch(batch.replace(features=features))
                est.append(estimate.cpu())
                outs.append(output.cpu())
                hashes.append(torch_chain(batch.features, 120, t0, reject_mask))
        res["cpu"] = (torch.cat(est), torch.cat(outs), torch.cat(hashes).int())

    def forward_only():
        with torch.no_grad():
            for batch in loader_of(one):
                features = builder.extract_features(batch.features, names)
                solver._process_batch(batch.replace(features=features))
    out["collect"] = interleaved({"bm: collect_wer (resident arrays, one pick launch a batch)": collect_ours,
                                  "reference's way: .cpu() of estimate and output, torch chain, cat": collect_cpu,
                                  "the loader and _process_batch alone": forward_only}, min(reps, 3), _clock)
    out["collect_equal"] = bool(torch.equal(res["ours"][0].cpu(), res["cpu"][0]) and
                                torch.equal(res["ours"][2].cpu(), res["cpu"][2].long().cpu()))
    out["collect_bytes"] = int(res["cpu"][0].numel() * 4 + res["cpu"][1].numel() * 4)
    res.clear()

    # 3. the full epoch with ranking
    def epoch():
        res["epoch"] = retrieval.wer_epoch(solver, seg, builder, names, batch_size=B, wer_negatives=10_000,
                                           generator=torch.Generator().manual_seed(3),
                                           negatives_generator=torch.Generator().manual_seed(4))

    def collect_all():
        res["all"] = retrieval.collect_wer(solver, loader_of(seg), len(seg), builder, names, t0)
    out["epoch"] = interleaved({"bm: wer_epoch, 10 000 negatives": epoch,
                                "bm: its collection alone": collect_all}, min(reps, 3), _clock)
    out["epoch_result"] = res["epoch"]
    out["epoch_flop"] = 2.0 * len(seg) * min(10_000, len(seg)) * 120 * seg.T
    return out


def _row(label, v, width=66):
    return f"  {label:{width}s} {v['median_ms']:10.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]  n = {v['n']}"


def _versus(ours, base, what):
    return (f"  bm / {what}   x{ours / base:.3f}   "
            + (f"({what} takes {base / ours:.2f} times as long)" if ours <= base else f"(bm is SLOWER than {what})"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wer_epoch_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps)))
        return
    cmd = ["timeout", "-k", "10", "500", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"wer_epoch_bench: the measurement ended with status {proc.returncode}")
    r = json.loads(proc.stdout.strip().splitlines()[-1])
    p_ours, p_torch = (r["pick"][k]["median_ms"] for k in r["pick"])
    c_ours, c_cpu, c_fwd = (r["collect"][k]["median_ms"] for k in r["collect"])
    e_all, e_collect = (r["epoch"][k]["median_ms"] for k in r["epoch"])
    rank = e_all - e_collect
    fwd = list(r["collect"].values())[2]
    fwd_spread = fwd["max_ms"] - fwd["min_ms"]
    lines = [f"The ClipLoss test epoch (bm/wer.py:21-121), {r['device']}: windows of {r['T']} samples, {MEG} MEG channels, "
             f"{F_ALL} feature channels",
             f"(120 mel + WordHash), batches of {B}, check_at_time {r['t0']}; SimpleConv of the paper's size (hidden 320), "
             "ClipLoss, no ScaleReject.",
             "Same device, implementations alternate, medians after warm-up [min .. max], milliseconds.", "",
             f"1. The label launch, one batch ({r['n_keep']} of {B} rows kept); HIP events around {CALLS} calls, per call:"]
    lines += [_row(name, v) for name, v in r["pick"].items()]
    lines += [_versus(p_ours, p_torch, "the torch chain"),
              f"  equal labels: {r['pick_equal']}.  One workgroup reads 5 floats and a byte per row: the launch itself is what it "
              "costs; the torch chain is five boolean-index gathers, four comparisons and four selects.", "",
             f"2. The collection over {r['n_collect']} windows of one recording; host clock around the loop and a device "
             "synchronise:"]
    lines += [_row(name, v) for name, v in r["collect"].items()]
    lines += [_versus(c_ours, c_cpu, "the loop with .cpu() copies"),
              f"  equal estimates and labels: {r['collect_equal']}.  The copies to the host move {r['collect_bytes'] / 1e6:.0f} MB "
              f"through pageable memory, each one a synchronise; here the median differs from the {c_fwd:.1f} ms of the loader "
              f"and the forward passes alone by {c_ours - c_fwd:+.1f} ms ("
              + ("inside" if abs(c_ours - c_fwd) <= fwd_spread else "outside") + f" their spread of {fwd_spread:.1f} ms): "
              "they bound it.", "",
             f"3. The epoch over {r['n_total']} windows of three recordings, {min(10_000, r['n_total'])} negatives:"]
    lines += [_row(name, v) for name, v in r["epoch"].items()]
    lines += [f"  the ranking (get_wer) is the difference, {rank:.1f} ms: {r['epoch_flop'] / 1e12:.2f} TFLOP of scores = "
              f"{r['epoch_flop'] / 1e12 / max(rank, 1e-9) * 1e3:.1f} TFLOP/s of useful fp32 work in the default f16x2 mode over all of it (the gather of the negatives, "
              "the word grouping on the host, softmax, sums and top-k included).",
              f"  wer = {r['epoch_result']['wer']:.4f}, wer_vocab = {r['epoch_result']['wer_vocab']:.4f} "
              "(an untrained model on random data: chance)."]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
