"""The Pitch feature measured: ``hip_ops.yin_pitch`` (csrc/pitch.hip, one launch) beside a restatement of the same
algorithm in torch ops on the same device.

    python scripts/pitch_bench.py [--out profiles/pitch_vs_torch.txt] [--reps 7] [--inner 3]

16 kHz, the reference's defaults (frames of 256 samples every 64, 100 ... 350 Hz, threshold 0.1).

  (a) one sound of 30 minutes (28.8 M samples, 449 996 frames);
  (b) 400 sounds of 3 s (48 000 samples, 746 frames each) in ONE call.

torch ops, in fp64 as the reference: ``unfold`` into frames, the difference function by ``rfft`` / ``irfft`` and two
``cumsum`` (the reference's expression), the cumulative mean normalisation, the first lag under the threshold by
``argmax`` of the mask and the walk down as the first lag behind it that does not descend -- per sound, so (b) is a
Python loop of 400.

Everything is warmed up; a timed repetition is ``inner`` calls bracketed by HIP events on the stream; the repetitions of
the two implementations alternate; medians are reported.  The measurement runs in a child process under a time limit; a
failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

SR, W_LEN, W_STEP, THRESH, F0_MIN, F0_MAX = 16_000, 256, 64, 0.1, 100.0, 350.0
CASES = {"a": dict(n=1, L=30 * 60 * SR, what="one sound of 30 minutes"),
         "b": dict(n=400, L=3 * SR, what="400 sounds of 3 s in one call")}


def torch_yin(x, tau_min, tau_max, size_pad):
    import torch
    frames = x.double().unfold(0, W_LEN, W_STEP)
    frames = frames[:len(range(0, x.numel() - W_LEN, W_STEP))]
    csum = torch.cat([frames.new_zeros(frames.shape[0], 1), (frames * frames).cumsum(1)], dim=1)
    fc = torch.fft.rfft(frames, size_pad)
    conv = torch.fft.irfft(fc * fc.conj(), size_pad)[:, :tau_max]
    d = csum[:, W_LEN - tau_max + 1:W_LEN + 1].flip(1) + csum[:, W_LEN:W_LEN + 1] - csum[:, :tau_max] - 2 * conv
    taus = torch.arange(1, tau_max, device=x.device, dtype=torch.float64)
    c = torch.cat([d.new_zeros(d.shape[0], 1), d[:, 1:] * taus / d[:, 1:].cumsum(1)], dim=1)
    idx = torch.arange(tau_max, device=x.device)
    under = (c < THRESH) & (idx >= tau_min)
    first = torch.where(under.any(1), under.int().argmax(1), torch.zeros((), dtype=torch.long, device=x.device))
    stays = torch.cat([~(c[:, 1:] < c[:, :-1]), torch.ones_like(under[:, :1])], dim=1) & (idx >= first[:, None])
    tau = stays.int().argmax(1)
    return torch.where(first > 0, SR / tau.double(), torch.zeros((), dtype=torch.float64, device=x.device)).float()[None]


def measure(reps: int, inner: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    from resample_bench import interleaved
    tau_min, tau_max = H.yin_taus(SR, W_LEN, W_STEP, F0_MIN, F0_MAX)
    size = W_LEN + tau_max
    p2 = (size // 32).bit_length()
    size_pad = min(n * 2 ** p2 for n in (16, 18, 20, 24, 25, 27, 30, 32) if n * 2 ** p2 >= size)
    out = dict(device=torch.cuda.get_device_name(0), cases={})
    for key, c in CASES.items():
        gen = torch.Generator().manual_seed(5)
        t = torch.arange(c["L"], dtype=torch.float64) / SR
        waves = []
        for i in range(c["n"]):
            f0 = 150.0 + 60.0 * torch.sin(2 * torch.pi * (0.7 + 0.01 * i) * t)
            phase = 2 * torch.pi * torch.cumsum(f0, 0) / SR
            waves.append((0.5 * torch.sin(phase) + 0.2 * torch.sin(2 * phase) + 0.05 * torch.randn(c["L"], generator=gen,
                                                                                               dtype=torch.float64)).float().cuda())
        result = {}

        def ours():
            result["ours"] = H.yin_pitch(waves, SR, W_LEN, W_STEP, THRESH, F0_MIN, F0_MAX)

        def torch_ops():
            result["torch"] = [torch_yin(x, tau_min, tau_max, size_pad) for x in waves]

        times = interleaved({"bm: yin_pitch": ours, "torch ops": torch_ops}, reps, inner)
        frames = sum(o.shape[1] for o in result["ours"])
        differ = sum(int((a != b).sum()) for a, b in zip(result["ours"], result["torch"]))
        voiced = sum(int((a > 0).sum()) for a in result["ours"])
        out["cases"][key] = dict(times=times, frames=frames, differ=differ, voiced=voiced)
        del waves, result
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pitch_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, args.inner)))
        return
    cmd = ["timeout", "-k", "10", "400", sys.executable, str(Path(__file__).resolve()), "--child", "--reps", str(args.reps),
           "--inner", str(args.inner)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        raise SystemExit(f"pitch_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    lines = [f"Pitch (YIN): {SR} Hz, frames of {W_LEN} every {W_STEP}, {F0_MIN:g} ... {F0_MAX:g} Hz, threshold {THRESH}, {res['device']}:",
             "hip_ops.yin_pitch (csrc/pitch.hip: bm_yin_pitch, one launch per call, the difference function as a direct fp64 sum)",
             "beside the same algorithm from torch ops in fp64 (unfold, rfft / irfft, cumsum, argmax; a Python loop over the",
             f"sounds); same device, interleaved, HIP events around {args.inner} calls, median of {args.reps} after warm-up",
             "[min .. max], milliseconds per call."]
    for key, c in res["cases"].items():
        t = c["times"]
        ours, base = (t[k]["median_ms"] for k in t)
        flop = 3.0 * sum(W_LEN - tau for tau in range(1, int(SR / F0_MIN))) * c["frames"]
        lines += ["", f"({key}) {CASES[key]['what']}: {c['frames']} frames, {c['voiced']} voiced"]
        lines += [f"  {name:40s} {v['median_ms']:9.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]" for name, v in t.items()]
        lines += [f"  bm / torch ops   x{ours / base:.3f}   "
                  + (f"(the torch ops take {base / ours:.2f} times as long)" if ours <= base else "(bm is SLOWER than the torch ops)"),
                  f"  difference function: {flop / 1e9:.1f} GFLOP of fp64 in {ours:.3f} ms = {flop / 1e12 / (ours / 1e3):.2f} TFLOP/s",
                  f"  frames whose pitch differs between the two (the FFT form is good to 1e-13; near ties may flip): {c['differ']}"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
