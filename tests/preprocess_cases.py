"""What the preprocessing tests share: the fixture of tests/golden/make_preprocess_golden.py, the body of the
reference's ``preprocess_mne`` restated over the restatements of its two filters (``audio_cases.ResampleFrac``;
julius' low-pass as ``hip_ops.lowpass_taps`` + replicate padding + ``F.conv1d``, always the direct sum), and the
per-element bounds of the two stages."""
import json
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional as F

import audio_cases as AC

GOLDEN = Path(__file__).resolve().parent / "golden" / "preprocess.npz"
U = 2.0 ** -24
# (highpass in Hz, sample rate in Hz) -> half = int(8 / (highpass / rate) / 2); the first is bm/studies/visualcheck.py:58
HALVES = [(0.1, 50, 2000), (0.1, 120, 4800), (0.1, 200, 8000), (0.05, 120, 9600), (0.5, 120, 960)]

_fixture = None


def fixture():
    """tests/golden/preprocess.npz, read once: ``dict(meta=..., arrays)``."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        _fixture = {k: z[k] for k in z.files}
        _fixture["meta"] = json.loads(str(z["meta"]))
    return _fixture


def gamma(n: int) -> float:
    return n * U / (1 - n * U)


def lowpass(x: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """The direct sum of ``taps`` (cast to ``x``'s dtype) over the replicate-padded last dimension of ``x`` [C, N]."""
    half = (taps.numel() - 1) // 2
    return F.conv1d(F.pad(x[:, None], (half, half), mode="replicate"), taps.to(x.dtype)[None, None])[:, 0]


def chain(raw: torch.Tensor, case: dict, dtype) -> torch.Tensor:
    """``preprocess_mne(raw, sample_rate, highpass).get_data()`` restated in ``dtype``: resample, then subtract the
    low-pass at ``highpass / sample_rate`` (``zeros = 8``)."""
    from brainmagick_amd import hip_ops as H
    data = AC.ResampleFrac(int(np.round(case["sfreq"])), case["sample_rate"])(raw.to(dtype))
    if case["highpass"]:
        data = data - lowpass(data, H.lowpass_taps(case["highpass"] / case["sample_rate"], 8)[0])
    return data


def stage_bounds(raw: torch.Tensor, case: dict) -> torch.Tensor:
    """[C, N] fp64: the resampler's ``(ntaps + 3) u (|taps| conv |x|)`` (tests/test_resample_gpu.py) plus, with a
    highpass, the FIR's ``gamma(ntaps + 2) (|taps| conv |z|) + u |truth|`` over the resampled rows ``z``."""
    from brainmagick_amd import hip_ops as H
    r = AC.ResampleFrac(int(np.round(case["sfreq"])), case["sample_rate"])
    z = r(raw.double())
    bound = torch.zeros_like(z)
    if r.old != r.new:
        bound = bound + (r.taps.shape[1] + 3) * U * r.magnitude(raw)
    if case["highpass"]:
        taps = H.lowpass_taps(case["highpass"] / case["sample_rate"], 8)[0]
        truth = z - lowpass(z, taps)
        bound = bound + gamma(taps.numel() + 2) * lowpass(z.abs(), taps.abs()) + U * truth.abs()
    return bound
