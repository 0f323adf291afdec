"""The mel spectrogram measured: ``hip_ops.mel_spectrograms`` (csrc/mel.hip, two launches) beside the same result built
from torch ops on the same device.

    python scripts/mel_bench.py [--out profiles/mel_vs_torch.txt] [--reps 7] [--inner 5]

n_fft 512, n_mels 120, 16 kHz, every switch at the reference's default (``norm_audio``, ``normalized``, log scale).

  (a) one waveform of 30 minutes (28.8 M samples, 225 001 frames);
  (b) 400 waveforms of 3 s (48 000 samples, 376 frames each) in ONE call.

torch ops: ``(x - x.mean()) / (1e-8 + x.std())``, ``torch.stft`` (reflect padding, periodic Hann window), ``/ sqrt(sum
w^2)``, ``abs() ** 2``, ``matmul`` with the filterbank, ``log10(. + eps)`` -- per waveform, so (b) is a Python loop of 400.

Everything is warmed up; a timed repetition is ``inner`` calls bracketed by HIP events on the stream; the repetitions of
the two implementations alternate; medians are reported.  A device-to-device copy of the bytes the launches move is timed
the same way on the same box.  The measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_FFT, N_MELS, SR, EPS = 512, 120, 16_000, 1e-5
CASES = {"a": dict(n=1, L=30 * 60 * SR, what="one waveform of 30 minutes"),
         "b": dict(n=400, L=3 * SR, what="400 waveforms of 3 s in one call")}
MATRIX_PEAK_TF = 157.3          # exact-fp32 MFMA, MI355X_MICROARCH


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn, inner):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def _interleaved(impls, reps, inner):
    import torch
    for fn in impls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for k, fn in impls.items():
            times[k].append(_timed(fn, inner))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def measure(reps: int, inner: int) -> dict:
    import torch
    from brainmagick_amd import hip_ops as H
    fb, _, _ = H.mel_filterbank(N_FFT, N_MELS, SR)
    fb = fb.cuda()
    window = torch.hann_window(N_FFT, periodic=True, device="cuda")
    wnorm = window.pow(2.).sum().sqrt()
    out = dict(device=torch.cuda.get_device_name(0), cases={})
    for key, c in CASES.items():
        gen = torch.Generator().manual_seed(5)
        waves = [(0.2 * torch.randn(c["L"], generator=gen) + 0.05).cuda() for _ in range(c["n"])]
        result = {}

        def ours():
            result["ours"] = H.mel_spectrograms(waves, N_MELS, N_FFT, SR)

        def torch_ops():
            res = []
            for x in waves:
                x = (x - x.mean()) / (1e-8 + x.std())
                spec = torch.stft(x, N_FFT, hop_length=N_FFT // 4, win_length=N_FFT, window=window, center=True,
                                  pad_mode="reflect", normalized=False, onesided=True, return_complex=True) / wnorm
                res.append(torch.log10(torch.matmul(fb.t(), spec.abs().pow(2.)) + EPS))
            result["torch"] = res

        frames = sum(1 + x.numel() // (N_FFT // 4) for x in waves)
        nbytes = dict(mel=4 * c["n"] * c["L"] + 4 * N_MELS * frames, moments=2 * 4 * c["n"] * c["L"])
        src = torch.empty((nbytes["mel"] + nbytes["moments"]) // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)

        def copy():                                  # reads and writes as many bytes as the two launches move
            dst.copy_(src)

        timer = H.KernelTimer()
        H.set_kernel_timer(timer)
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        H.set_kernel_timer(None)
        kernels = {k: v["median_ms"] for k, v in timer.summary().items()}
        times = _interleaved({"bm: wave_moments + mel_spectrogram": ours, "torch ops": torch_ops,
                              "device copy of the same bytes": copy}, reps, inner)
        diff = max(float((a - b).abs().max()) for a, b in zip(result["ours"], result["torch"]))
        # which of the two is off: the first waveform again with the same torch ops in fp64
        x = waves[0].double()
        x = (x - x.mean()) / (1e-8 + x.std())
        spec = torch.stft(x, N_FFT, hop_length=N_FFT // 4, win_length=N_FFT, window=window.double(), center=True,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True) / window.double().pow(2.).sum().sqrt()
        truth = torch.log10(torch.matmul(H.mel_filterbank(N_FFT, N_MELS, SR)[0].cuda().double().t(), spec.abs().pow(2.)) + EPS)
        dev = {k: float((result[k][0].double() - truth).abs().max()) for k in ("ours", "torch")}
        del x, spec, truth
        out["cases"][key] = dict(times=times, kernels=kernels, frames=frames, nbytes=nbytes, max_abs_diff=diff, dev64=dev)
        del waves, result, src, dst
        torch.cuda.empty_cache()
    return out


def _row(label, v, width=40):
    return f"  {label:{width}s} {v['median_ms']:9.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mel_vs_torch.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
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
        raise SystemExit(f"mel_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    nbp = (N_FFT // 2 + 1 + 15) // 16 * 16
    lines = [f"MelSpectrum targets: n_fft {N_FFT}, n_mels {N_MELS}, {SR} Hz, norm_audio, normalized, log scale, {res['device']}:",
             "hip_ops.mel_spectrograms (csrc/mel.hip: bm_wave_moments + bm_mel_spectrogram, two launches per call) beside the",
             "same result from torch ops (mean / std, torch.stft, abs() ** 2, matmul, log10; a Python loop over the waveforms),",
             f"same device, interleaved, HIP events around {args.inner} calls, median of {args.reps} after warm-up [min .. max],",
             "milliseconds per call.  Kernel times: HIP events around each launch (hip_ops.KernelTimer), median of 3 calls."]
    for key, c in res["cases"].items():
        t = c["times"]
        ours, base, copy = (t[k]["median_ms"] for k in t)
        moved = c["nbytes"]["mel"] + c["nbytes"]["moments"]
        k_mel = c["kernels"]["mel_spectrogram"]
        flop_done = 2.0 * N_FFT * 2 * nbp * c["frames"]
        flop_needed = 2.0 * N_FFT * 2 * (N_FFT // 2 + 1) * c["frames"]
        lines += ["", f"({key}) {CASES[key]['what']}: {c['frames']} frames"]
        lines += [_row(name, v) for name, v in t.items()]
        lines += [f"  bm / torch ops   x{ours / base:.3f}   "
                  + (f"(the torch ops take {base / ours:.2f} times as long)" if ours <= base else "(bm is SLOWER than the torch ops)"),
                  f"  kernels: wave_moments {c['kernels']['wave_moments']:.3f} ms, mel_spectrogram {k_mel:.3f} ms",
                  f"  bytes from the shapes: the waveform twice for the moments ({c['nbytes']['moments'] / 1e6:.0f} MB), once more "
                  f"plus the output for the spectrogram ({c['nbytes']['mel'] / 1e6:.0f} MB) = {moved / 1e6:.0f} MB;",
                  f"  a device copy that reads and writes {moved / 1e6:.0f} MB in all takes {copy:.3f} ms "
                  f"({moved / 1e9 / (copy / 1e3):.0f} GB/s): the call takes {ours / copy:.1f} times as long",
                  f"  contraction: {flop_done / 1e9:.1f} GFLOP issued ({flop_needed / 1e9:.1f} needed; the bins are padded to {nbp}) in "
                  f"{k_mel:.3f} ms = {flop_done / 1e12 / (k_mel / 1e3):.1f} TFLOP/s, "
                  f"{100 * flop_done / 1e12 / (k_mel / 1e3) / MATRIX_PEAK_TF:.0f} % of the {MATRIX_PEAK_TF} TF exact-fp32 matrix peak",
                  f"  largest |difference| of the two results (log10 units): {c['max_abs_diff']:.2e}; of the first waveform's "
                  f"from the same torch ops in fp64: bm {c['dev64']['ours']:.2e}, torch ops in fp32 {c['dev64']['torch']:.2e}"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
