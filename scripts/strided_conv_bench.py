"""Times the three kernels of csrc/conv_strided.hip at ConvRNN-sized shapes beside torch-ROCm's own convolutions on
the same GPU:   python scripts/strided_conv_bench.py [--batch 256] [--rounds 20] [--out profiles/strided_conv_vs_torch.txt]

Shapes: the encoder 273 -> 512 -> 512 at kernel 4, stride 2, T = 364 and the mirrored ConvTranspose1d decoder.  Per
layer: forward, data gradient and weight gradient of ours (HIP events around each launch, the split-K fold included in
the weight gradient) and F.conv1d / F.conv_transpose1d forward and backward (torch.autograd.grad of both operands, one
event pair).  Protocol: warm-up, then `rounds` rounds that run every candidate once, in turn (interleaved, so clock
and thermal drift hit all of them alike); medians are reported.  A stated baseline, not a gate."""
import argparse
import statistics
import sys
from pathlib import Path

import torch
from torch.nn import functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from brainmagick_amd import hip_ops as H  # noqa: E402

K, S, DIL, PAD = 4, 2, 1, 2
LAYERS = [("enc1 conv   273->512 T=364", False, 273, 512, 364),
          ("enc2 conv   512->512 T=183", False, 512, 512, 183),
          ("dec1 convT  512->512 T=92", True, 512, 512, 92),
          ("dec2 convT  512->273 T=182", True, 512, 273, 182)]


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    return start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    B = args.batch
    lines = [f"strided / transposed conv kernels vs torch {torch.__version__} on {torch.cuda.get_device_name(0)}",
             f"batch {B}, kernel {K}, stride {S}, padding {PAD}; medians of {args.rounds} interleaved rounds, ms",
             f"{'layer':30s} {'pass':6s} {'ours':>8s} {'torch':>8s} {'torch/ours':>10s} {'ours TFLOP/s':>12s}"]
    for name, transposed, cin, m, T in LAYERS:
        g = torch.Generator().manual_seed(T)
        x = torch.randn(B, cin, T, generator=g).cuda()
        w = (torch.randn((cin, m, K) if transposed else (m, cin, K), generator=g) / (cin * K) ** 0.5).cuda()
        b = torch.randn(m, generator=g).cuda()
        Tout = H.conv_out_len(T, K, S, DIL, PAD, transposed)
        dy = torch.randn(B, m, Tout, generator=g).cuda()
        first, second = H.pack_strided_rows_first, H.pack_strided_rows_second
        wp_f = (second if transposed else first)(w)
        wp_d = (first if transposed else second)(w)
        conv = F.conv_transpose1d if transposed else F.conv1d
        xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        flops = 2.0 * B * (T if transposed else Tout) * m * cin * K      # useful multiply-adds x 2, every pass

        def ours_fwd():
            H.conv_strided(x, wp_f, m, Tout, K, S, DIL, PAD, transposed, bias=b)

        def ours_dgrad():
            H.conv_strided(dy, wp_d, cin, T, K, S, DIL, PAD, not transposed)

        def ours_wgrad():
            if transposed:
                H.conv_strided_wgrad(x, dy, K, S, DIL, PAD)
            else:
                H.conv_strided_wgrad(dy, x, K, S, DIL, PAD)

        def torch_fwd():
            with torch.no_grad():
                conv(x, w, b, stride=S, padding=PAD, dilation=DIL)

        yt = conv(xt, wt, b, stride=S, padding=PAD, dilation=DIL)

        def torch_dgrad():
            torch.autograd.grad(yt, xt, dy, retain_graph=True)

        def torch_wgrad():
            torch.autograd.grad(yt, wt, dy, retain_graph=True)

        cands = [("fwd", ours_fwd, torch_fwd), ("dgrad", ours_dgrad, torch_dgrad), ("wgrad", ours_wgrad, torch_wgrad)]
        for _ in range(args.warmup):
            for _, a, t in cands:
                a()
                t()
        torch.cuda.synchronize()
        events = {(p, who): [] for p, _, _ in cands for who in ("ours", "torch")}
        for _ in range(args.rounds):
            for p, a, t in cands:
                events[(p, "ours")].append(timed(a))
                events[(p, "torch")].append(timed(t))
        torch.cuda.synchronize()
        for p, _, _ in cands:
            ours = statistics.median(s.elapsed_time(e) for s, e in events[(p, "ours")])
            ref = statistics.median(s.elapsed_time(e) for s, e in events[(p, "torch")])
            lines.append(f"{name:30s} {p:6s} {ours:8.3f} {ref:8.3f} {ref / ours:10.2f} {flops / ours / 1e9:12.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
