"""The resampler measured: ``hip_ops.resample_frac`` (csrc/resample.hip, one launch) beside the same algorithm built
from torch ops on the same device, and the whole ``DeviceMelSpectrum.compute(..., resample=True)`` beside them.

    python scripts/resample_bench.py [--out profiles/resample_vs_torch.txt] [--reps 7] [--inner 3]

44.1 kHz -> 16 kHz (441 / 160, 581 taps, julius' defaults).

  (a) one sound of 30 minutes (79.4 M samples in, 28.8 M out);
  (b) 400 sounds of 3 s (132 300 samples each) in ONE call.

torch ops: ``F.pad(replicate)``, ``F.conv1d(stride=old)`` with the ``new`` phases as output channels, transpose,
reshape, the first ``floor(new L / old)`` samples -- per sound, so (b) is a Python loop of 400.

Everything is warmed up; a timed repetition is ``inner`` calls bracketed by HIP events on the stream; the repetitions of
the implementations alternate; medians are reported.  The measurement runs in a child process under a time limit; a
failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

OLD_SR, NEW_SR = 44_100, 16_000
CASES = {"a": dict(n=1, L=30 * 60 * OLD_SR, what="one sound of 30 minutes"),
         "b": dict(n=400, L=3 * OLD_SR, what="400 sounds of 3 s in one call")}
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


def interleaved(impls, reps, inner):
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
    from torch.nn import functional as F
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.audio import DeviceMelSpectrum
    taps, old, new, width = H.resample_taps(OLD_SR, NEW_SR)
    kernel = taps[:, None].cuda()
    mel = DeviceMelSpectrum(120.0)
    out = dict(device=torch.cuda.get_device_name(0), ntaps=int(taps.shape[1]), old=old, new=new, cases={})
    for key, c in CASES.items():
        gen = torch.Generator().manual_seed(5)
        waves = [(0.2 * torch.randn(c["L"], generator=gen) + 0.05).cuda() for _ in range(c["n"])]
        result = {}

        def ours():
            result["ours"] = H.resample_frac(waves, OLD_SR, NEW_SR)

        def torch_ops():
            res = []
            for x in waves:
                padded = F.pad(x[None, None], (width, width + old), mode="replicate")
                y = F.conv1d(padded, kernel, stride=old).transpose(1, 2).reshape(-1)
                res.append(y[:new * x.numel() // old])
            result["torch"] = res

        def whole():
            result["mel"] = mel.compute(waves, OLD_SR, resample=True)

        timer = H.KernelTimer()
        H.set_kernel_timer(timer)
        for _ in range(3):
            whole()
        torch.cuda.synchronize()
        H.set_kernel_timer(None)
        kernels = {k: v["median_ms"] for k, v in timer.summary().items()}
        times = interleaved({"bm: resample_frac": ours, "torch ops": torch_ops,
                             "bm: DeviceMelSpectrum.compute(resample=True)": whole}, reps, inner)
        diff = max(float((a - b).abs().max()) for a, b in zip(result["ours"], result["torch"]))
        outputs = sum(o.numel() for o in result["ours"])
        out["cases"][key] = dict(times=times, kernels=kernels, outputs=outputs, max_abs_diff=diff)
        del waves, result
        torch.cuda.empty_cache()
    return out


def _row(label, v, width=48):
    return f"  {label:{width}s} {v['median_ms']:9.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample_vs_torch.txt"))
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
        raise SystemExit(f"resample_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    lines = [f"Resampling {OLD_SR} Hz -> {NEW_SR} Hz ({res['old']} / {res['new']}, {res['ntaps']} taps), {res['device']}:",
             "hip_ops.resample_frac (csrc/resample.hip: bm_resample_frac, one launch per call) beside the same algorithm from",
             "torch ops (F.pad replicate, F.conv1d(stride=old), transpose; a Python loop over the sounds), and the whole",
             "DeviceMelSpectrum.compute(resample=True) (n_fft 512, 40 mels: bm_wave_moments, bm_resample_frac,",
             f"bm_mel_spectrogram); same device, interleaved, HIP events around {args.inner} calls, median of {args.reps} after",
             "warm-up [min .. max], milliseconds per call.  Kernel times: HIP events around each launch of the whole compute",
             "(hip_ops.KernelTimer), median of 3 calls."]
    for key, c in res["cases"].items():
        t = c["times"]
        ours, base, _ = (t[k]["median_ms"] for k in t)
        k_rs = c["kernels"]["resample_frac"]
        ntp = (res["ntaps"] + 3) // 4 * 4
        flop = 2.0 * ntp * c["outputs"]
        lines += ["", f"({key}) {CASES[key]['what']}: {c['outputs']} samples out"]
        lines += [_row(name, v) for name, v in t.items()]
        lines += [f"  bm / torch ops   x{ours / base:.3f}   "
                  + (f"(the torch ops take {base / ours:.2f} times as long)" if ours <= base else "(bm is SLOWER than the torch ops)"),
                  "  kernels of the whole compute: " + ", ".join(f"{k} {v:.3f} ms" for k, v in c["kernels"].items()),
                  f"  contraction: {flop / 1e9:.1f} GFLOP in {k_rs:.3f} ms = {flop / 1e12 / (k_rs / 1e3):.1f} TFLOP/s, "
                  f"{100 * flop / 1e12 / (k_rs / 1e3) / MATRIX_PEAK_TF:.0f} % of the {MATRIX_PEAK_TF} TF exact-fp32 matrix peak",
                  f"  largest |difference| of the two results: {c['max_abs_diff']:.2e}"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
