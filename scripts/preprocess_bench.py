"""The MEG preprocessing measured: ``hip_ops.resample_rows`` (csrc/resample.hip) and ``hip_ops.highpass_filter``
(csrc/fir.hip), one launch each, beside the same two stages built from torch ops on the same device.

    python scripts/preprocess_bench.py [--out profiles/preprocess_vs_torch.txt] [--reps 5]

273 channels x 30 minutes at 1200 Hz -> 120 Hz (10 / 1, julius' defaults), then a highpass of 0.1 Hz (half = 4800, 9601
taps) over the 273 x 216 000 resampled samples.

torch ops, resample: ``F.pad(replicate)`` + ``F.conv1d(stride=10)``;  filter, direct: ``F.pad(replicate)`` +
``F.conv1d`` with the 9601 taps;  filter, FFT: ``torch.fft.rfft`` of the padded rows and of the taps at 2^18 points, the
product, ``irfft``, the slice (about a hundredth of the arithmetic of the direct sum, and no fixed summation order).

Everything is warmed up; a timed repetition is one call bracketed by HIP events on the stream; the repetitions of the
implementations alternate; medians are reported.  An implementation whose warm-up call takes more than two seconds is
timed once.  The measurement runs in a child process under a time limit; a failure ends the run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CHANNELS, OLD_SR, NEW_SR, MINUTES, HIGHPASS = 273, 1200, 120, 30, 0.1
MATRIX_PEAK_TF = 157.3          # exact-fp32 MFMA, MI355X_MICROARCH
SLOW_MS = 2000.0


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def interleaved(impls, reps):
    import torch
    slow = {}
    for k, fn in impls.items():
        fn()
        torch.cuda.synchronize()
        slow[k] = _timed(fn) > SLOW_MS
    times = {k: [] for k in impls}
    for rep in range(reps):
        for k, fn in impls.items():
            if rep == 0 or not slow[k]:
                times[k].append(_timed(fn))
    return {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), n=len(v)) for k, v in times.items()}


def measure(reps: int) -> dict:
    import torch
    from torch.nn import functional as F
    from brainmagick_amd import hip_ops as H
    L = MINUTES * 60 * OLD_SR
    gen = torch.Generator().manual_seed(5)
    raw = torch.empty(CHANNELS, L, device="cuda")
    for c in range(CHANNELS):                                    # a DC offset of 100 x the spread, as a raw recording has
        raw[c] = (torch.randn(L, generator=gen) + 100.0 * (1 + c % 7)).cuda()
    rtaps, old, new, width = H.resample_taps(OLD_SR, NEW_SR)
    rkernel = rtaps[:, None].cuda()
    cutoff = HIGHPASS / NEW_SR
    taps, half = H.lowpass_taps(cutoff, 8, "cuda")
    ntaps = 2 * half + 1
    z = H.resample_rows(raw, OLD_SR, NEW_SR)
    T = z.shape[1]
    nfft = 1 << (T + 2 * half + ntaps - 1).bit_length()
    taps_f = torch.fft.rfft(taps, nfft)
    result = {}

    def rs_ours():
        result["rs_ours"] = H.resample_rows(raw, OLD_SR, NEW_SR)

    def rs_torch():
        padded = F.pad(raw[:, None], (width, width + old), mode="replicate")
        result["rs_torch"] = F.conv1d(padded, rkernel, stride=old)[:, 0, :new * L // old]

    def fir_ours():
        result["fir_ours"] = H.highpass_filter(z, cutoff)

    def fir_torch():
        padded = F.pad(z[:, None], (half, half), mode="replicate")
        result["fir_torch"] = z - F.conv1d(padded, taps[None, None])[:, 0]

    def fir_fft():
        padded = F.pad(z[:, None], (half, half), mode="replicate")[:, 0]
        low = torch.fft.irfft(torch.fft.rfft(padded, nfft) * taps_f, nfft)[:, ntaps - 1:ntaps - 1 + T]
        result["fir_fft"] = z - low

    t_rs = interleaved({"bm: resample_rows": rs_ours, "torch ops: F.pad + F.conv1d(stride=10)": rs_torch}, reps)
    rs_diff = float((result["rs_ours"] - result["rs_torch"]).abs().max())
    del result["rs_torch"]
    torch.cuda.empty_cache()
    t_fir = interleaved({"bm: highpass_filter (fir_rows)": fir_ours, "torch ops: F.pad + F.conv1d, direct": fir_torch,
                         "torch ops: rfft product over the padded rows": fir_fft}, reps)
    return dict(device=torch.cuda.get_device_name(0), L=L, T=T, ntaps=ntaps, half=half, rs_ntaps=int(rtaps.shape[1]), nfft=nfft,
                resample=t_rs, fir=t_fir, rs_diff=rs_diff,
                fir_diff_direct=float((result["fir_ours"] - result["fir_torch"]).abs().max()),
                fir_diff_fft=float((result["fir_ours"] - result["fir_fft"]).abs().max()),
                fir_tile=H.fir_tile(), fir_chunk=H.fir_chunk())


def _row(label, v, width=48):
    return f"  {label:{width}s} {v['median_ms']:10.3f}  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]  n = {v['n']}"


def _versus(ours, base, what):
    return (f"  bm / {what}   x{ours / base:.3f}   "
            + (f"(the torch ops take {base / ours:.2f} times as long)" if ours <= base else f"(bm is SLOWER than {what})"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "preprocess_vs_torch.txt"))
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
        raise SystemExit(f"preprocess_bench: the measurement ended with status {proc.returncode}")
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    rs, fir = res["resample"], res["fir"]
    rs_ours, rs_base = (rs[k]["median_ms"] for k in rs)
    f_ours, f_direct, f_fft = (fir[k]["median_ms"] for k in fir)
    flop = 2.0 * res["ntaps"] * CHANNELS * res["T"]
    lines = [f"Preprocessing a raw recording, {res['device']}: {CHANNELS} channels x {MINUTES} min at {OLD_SR} Hz "
             f"({res['L']} samples a row)",
             f"-> {NEW_SR} Hz ({res['rs_ntaps']} taps a phase, {res['T']} samples a row), then a highpass of {HIGHPASS} Hz "
             f"(half = {res['half']}, {res['ntaps']} taps).",
             "hip_ops.resample_rows (csrc/resample.hip: bm_resample_frac, one launch) and hip_ops.highpass_filter",
             f"(csrc/fir.hip: bm_fir_rows, one launch; tiles of {res['fir_tile']} outputs, chunks of {res['fir_chunk']} taps) beside the "
             "same stages from torch ops;",
             f"same device, interleaved, HIP events around one call, median of up to {args.reps} after warm-up [min .. max], "
             "milliseconds per call",
             "(n = 1: the warm-up call took more than two seconds, so the implementation was timed once).",
             "", "Resample:"]
    lines += [_row(name, v) for name, v in rs.items()]
    lines += [_versus(rs_ours, rs_base, "the torch ops"),
              f"  largest |difference| of the two results: {res['rs_diff']:.2e}", "", "Highpass:"]
    lines += [_row(name, v) for name, v in fir.items()]
    lines += [_versus(f_ours, f_direct, "the direct F.conv1d"), _versus(f_ours, f_fft, "the FFT product"),
              f"  direct sum: {flop / 1e9:.1f} GFLOP in {f_ours:.3f} ms = {flop / 1e12 / (f_ours / 1e3):.1f} TFLOP/s, "
              f"{100 * flop / 1e12 / (f_ours / 1e3) / MATRIX_PEAK_TF:.0f} % of the {MATRIX_PEAK_TF} TF exact-fp32 matrix peak",
              f"  largest |difference| from the direct F.conv1d: {res['fir_diff_direct']:.2e}, from the FFT product "
              f"({res['nfft']} points): {res['fir_diff_fft']:.2e}",
              "  The direct form is kept for its fixed summation order and its per-sample bound; an FFT form is not built."]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
