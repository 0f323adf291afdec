"""Shared helpers for the parity tests."""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
MODEL_FIXTURES = ["clip_conv_train", "clip_conv_eval", "no_merger_relu_noskip",
                  "no_subject_layers_leaky", "subject_embedding", "plain_out", "linear_out_k5",
                  "initial_depth2_hidden_subject", "subsample_channels", "extra_negatives"]


# options outside the paper's grids, implemented off the hot path (GPU torch ops + the 1x1 HIP conv): the HIP model is
# held to the live reference directly (the CPU oracle restates the hot path only)
OFF_PATH_FIXTURES = ["layer_scale_rewrite_post_skip", "channel_dropout_train", "conv_dropouts_eval",
                     "merger_per_subject", "groups2", "two_inputs", "two_inputs_concatenate",
                     "dual_path"]


class Golden:
    def __init__(self, name):
        self.name = name
        z = np.load(GOLDEN / f"{name}.npz")
        self.raw = {k: z[k] for k in z.files}
        self.meta = json.loads(str(self.raw["meta"])) if "meta" in self.raw else {}

    def group(self, prefix):
        out = {}
        for k, v in self.raw.items():
            if k.startswith(prefix + "/"):
                t = torch.from_numpy(np.array(v))
                out[k[len(prefix) + 1:]] = t
        return out

    def t(self, key):
        return torch.from_numpy(np.array(self.raw[key]))


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = b.norm().item()
    if denom == 0:
        return a.norm().item()
    return (a - b).norm().item() / denom


def shifted(t: torch.Tensor, k: int) -> torch.Tensor:
    """``t`` on the GPU as the view ``buf[k:k + n].view(t.shape)`` of a flat fp32 buffer: contiguous, its base ``4 * k``
    bytes past a 16-byte boundary (k in 0..3; k = 0: an aligned view, the same code path on the test's side)."""
    assert 0 <= k <= 3 and t.dtype == torch.float32 and t.numel() > 0
    n = t.numel()
    buf = torch.empty(n + 3, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return view


class ShiftedOut:
    """A NaN-poisoned fp32 output ``.view`` of ``shape``, ``4 * k`` bytes past a 16-byte boundary, inside a buffer that
    holds ``guard`` canary floats in front of it and behind it (tests/test_guard_bands_gpu.py's layout).  ``check`` after
    the kernel: every canary intact (no store left the view -- one element past a gradient view is the neighbouring
    parameter's gradient) and no NaN left (no element skipped)."""
    CANARY = -7.0e37

    def __init__(self, shape, k: int, guard: int = 1024):
        assert 0 <= k <= 3 and guard % 4 == 0
        n = 1
        for s in shape:
            n *= int(s)
        assert n > 0
        self.buf = torch.full((guard + k + n + guard,), self.CANARY, device="cuda", dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = guard + k, guard + k + n
        self.view = self.buf[self.lo:self.hi].view(tuple(shape))
        self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == 4 * k and self.view.is_contiguous()

    def check(self, what):
        assert bool((self.buf[:self.lo] == self.CANARY).all()), f"{what}: a store landed BELOW the view"
        assert bool((self.buf[self.hi:] == self.CANARY).all()), f"{what}: a store landed ABOVE the view"
        assert not bool(torch.isnan(self.view).any()), f"{what}: NaN left in the output (a skipped element)"


NOISE = 1e-6


def close(a, b, tol, ref_scale):
    """rel-L2 <= tol.  The only escape is for gradients that are round-off noise IN THE REFERENCE (analytically zero:
    the conv bias in front of a BatchNorm has sum(dy) == 0; recognised by max|g_ref| <= 1e-5 x the largest gradient
    norm of the model): there max|a-b| <= 1e-6 x that norm.  A parameter with a small but genuine gradient gets no
    absolute escape -- it has to meet the relative tolerance on its own norm."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if (a - b).norm().item() <= tol * b.norm().item():
        return True
    return is_noise_grad(b, ref_scale) and (a - b).abs().max().item() <= NOISE * ref_scale


def is_noise_grad(g, ref_scale):
    """Adam turns a round-off-noise gradient into a full +-lr update (g / (|g| + eps)), so the
    parameters behind such gradients are not reproducible across implementations (nor across
    BLAS/thread counts of the reference itself); they are excluded from after-step comparisons."""
    return g.abs().max().item() <= 10 * NOISE * ref_scale


def adam_params_close(p, p_ref, nsteps, g_ref=None, gscale=1.0, lr=3e-4):
    """After-step parameter check that is robust to Adam's sign amplification: at step 1 the update
    is lr * g / (|g| + eps) = +-lr whatever |g|, so an element whose gradient is round-off noise
    around 0 may legitimately move by +lr in one implementation and -lr in the other (sensor-attention
    heads have thousands of such near-cancelling entries).  Required: >= 99 % of the elements agree
    to 1e-6 absolute (a wrong lr / beta / bias-correction would move ALL of them) and nothing differs
    by more than the 2*lr*nsteps a sign flip can produce.  The tight checks are the per-step losses
    (step k+1's loss sees step k's update), the step-0 gradients and test_adam_kernel (bitwise-close
    Adam arithmetic given identical gradients)."""
    d = (p.detach().double().cpu() - p_ref.detach().double().cpu()).abs()
    bad = d > 1e-6
    if g_ref is not None:
        # elements whose reference gradient is itself round-off noise (e.g. the k=0 cosine column of
        # the attention heads: sum_c dsoftmax == 0) are not counted
        bad &= g_ref.detach().double().cpu().abs() > 10 * NOISE * gscale
    frac_bad = bad.double().mean().item()
    return frac_bad <= 1e-2 and d.max().item() <= 2.1 * lr * nsteps, (frac_bad, d.max().item())


def running_stat_close(v, v_ref, nsteps, lr=3e-4, momentum=0.1):
    """BatchNorm running statistics: tight (2e-5 rel-L2) after one step; from the second step on the
    batch mean absorbs the noise-driven +-lr drift of the conv bias in front of the BatchNorm (see
    is_noise_grad), i.e. up to momentum * 2*lr per extra step in absolute terms."""
    if rel_l2(v, v_ref) < 2e-5:
        return True
    d = (v.detach().double().cpu() - v_ref.detach().double().cpu()).abs().max().item()
    return d <= 2.1 * lr * momentum * (nsteps - 1) + 1e-6


# ---------------------------------------------------------------------------------------------------------------
# The "wide kernels" fixture (tests/golden/wide_kernels_train.npz): the smallest model whose convs and weight gradients
# run in the headline wide f16x2 kernels (T > 128, M >= 96), held to the LIVE reference directly.  Its 1.6 M
# parameters and its inputs are not stored: both sides rebuild them from the seed (same constructor RNG order, same
# synthetic batch generator) and the fixture keeps digests to prove that they did.
# ---------------------------------------------------------------------------------------------------------------
WIDE_DIMS = dict(B=8, C=64, T=192, F=32, S=4, hidden=256, seed=4077)
WIDE_CFG = dict(depth=4, kernel_size=3, dilation_growth=2, dilation_period=5, batch_norm=True, skip=True, gelu=True,
                glu=2, glu_context=1, glu_glu=True, complex_out=True, merger=True, merger_pos_dim=288,
                merger_channels=256, merger_dropout=0.2, initial_linear=256, initial_depth=1, subject_layers=True,
                subject_layers_dim="input", subject_dim=0)


def wide_inputs():
    """(synthetic batch, candidates, ban centre, generator positioned behind them) of the wide fixture."""
    from brainmagick_amd.synthetic import make_batch
    d = WIDE_DIMS
    sb = make_batch(d["B"], d["C"], d["T"], d["F"], d["S"], seed=d["seed"], n_layouts=2)
    gen = torch.Generator().manual_seed(d["seed"] + 1)
    ban_center = torch.rand(2, generator=gen)
    return sb, sb.features, ban_center, gen


def randomize_batchnorm(model, gen):
    """Non-trivial BatchNorm affine parameters / running statistics, drawn in module order from `gen`."""
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5, generator=gen)
                mod.bias.uniform_(-0.3, 0.3, generator=gen)
                mod.running_mean.uniform_(-0.2, 0.2, generator=gen)
                mod.running_var.uniform_(0.5, 1.5, generator=gen)


def tensor_digest(t: torch.Tensor):
    """(wrapping int64 sum, xor, element count) of the fp32 bit patterns: exact integer arithmetic, so the digest does
    not depend on the host's summation order (a floating-point sum differs between the build container and the GPU
    box).  Equal digests of two tensors built by the same code from the same seed mean identical tensors for every
    practical purpose."""
    t = t.detach().cpu().contiguous()
    if not t.is_floating_point():
        t = t.float()
    bits = t.float().view(torch.int32).flatten().numpy()
    total = int(bits.astype(np.int64).sum()) if bits.size else 0
    x = int(np.bitwise_xor.reduce(bits.view(np.uint32))) if bits.size else 0
    return np.array([total, x, bits.size], dtype=np.int64)


def sample_indices(numel: int, n: int = 64, seed: int = 0):
    gen = torch.Generator().manual_seed(seed + numel)
    return torch.randint(0, numel, (min(n, numel),), generator=gen)
