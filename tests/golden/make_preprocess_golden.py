"""Golden vectors of the MEG preprocessing, from the REAL reference ``preprocess_mne`` (bm/studies/api.py:334-363).

Run in the build container only:   python tests/golden/make_preprocess_golden.py [output directory]
Writes ``preprocess.npz`` (default: next to this file).

As in make_lowpass_golden.py the function is taken from the reference's source by AST and run, unmodified, against
stubs.  Neither ``julius`` nor ``mne`` can be imported here:

- ``julius.ResampleFrac`` is the restatement of tests/audio_cases.py (julius' published definition in torch ops);
- ``julius.lowpass_filter(x, cutoff, zeros=8)`` RESTATES julius' published formula (``restated_taps`` +
  ``F.pad(mode="replicate")`` + ``F.conv1d``), always as the direct sum, in the dtype of ``x``;
- ``mne.Info`` is a dict, ``mne.find_layout`` returns nothing, ``mne.io.RawArray`` holds ``(data, info)``.

So the fixture pins the WIRING to the live reference -- resample first, then the subtraction in place, the cutoff
expression ``highpass / sample_rate``, ``zeros = 8``, ``old_sr = int(np.round(sfreq))``, the ValueError -- and the two
filters to the restatements.  julius itself cannot be pinned here.  Every case runs twice: as the reference does
(``torch.Tensor(...)``: fp32) and with ``torch.Tensor`` bound to an fp64 conversion (the truth of the GPU tests).

``CASES``, 3 channels x 6000 samples each, a DC offset of 100 x the spread:
  ``down_1200_120``       1200 Hz -> 120 Hz, no highpass
  ``down_1000_120_hp``    1000 Hz -> 120 Hz, highpass 0.5 Hz (half 960)
  ``sfreq_1199_7``        sfreq = 1199.7 (rounds to 1200) -> 120 Hz, highpass 1 Hz (half 480)
  ``same_120_hp``         120 Hz -> 120 Hz, highpass 2 Hz (half 240): no resampling
``ERRORS``: ``sample_rate > old_sr`` (preprocess_mne) and a non-integer rate (``Recording.preprocessed``, the first
statement of the method, run from its source in the same way); the messages are stored.

Stored: ``raw`` [3, 6000] fp32, per case ``<case>/out32`` and ``<case>/out64`` and the ``sfreq`` of the array that came
back; ``meta`` (JSON).
"""
import ast
import json
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(1, str(HERE.parent))

import audio_cases as AC  # noqa: E402

C, L = 3, 6000
CASES = {
    "down_1200_120": dict(sfreq=1200.0, sample_rate=120, highpass=0.0),
    "down_1000_120_hp": dict(sfreq=1000.0, sample_rate=120, highpass=0.5),
    "sfreq_1199_7": dict(sfreq=1199.7, sample_rate=120, highpass=1.0),
    "same_120_hp": dict(sfreq=120.0, sample_rate=120, highpass=2.0),
}
ERRORS = {
    "rate_above": dict(sfreq=1000.0, sample_rate=1200, highpass=0.0),
    "rate_fraction": dict(sfreq=1000.0, sample_rate=120.5, highpass=0.0),
}


def raw_data() -> np.ndarray:
    """[C, L] fp32: slow drifts and noise around a DC offset of 100 x the spread, another one per channel."""
    g = torch.Generator().manual_seed(3343)
    t = torch.arange(L, dtype=torch.float64) / 1200
    slow = torch.stack([torch.sin(2 * math.pi * f * t + p) for f, p in ((0.3, 0.1), (1.7, 1.3), (7.0, 2.9))])
    noise = torch.randn(C, L, generator=g, dtype=torch.float64)
    dc = torch.tensor([[100.0], [-140.0], [75.0]], dtype=torch.float64)
    return (dc + 0.7 * slow + 0.5 * noise).float().numpy()


def restated_taps(cutoff: float, zeros: float = 8):
    """(taps, half) of julius' ``LowPassFilter(cutoff, zeros=zeros)``: its expressions, fp32, on the CPU."""
    half = int(zeros / cutoff / 2)
    time = torch.arange(-half, half + 1)
    win = torch.hann_window(2 * half + 1, periodic=False)
    arg = 2 * cutoff * math.pi * time
    sinc = torch.where(arg == 0, 1., torch.sin(arg) / arg)
    taps = 2 * cutoff * win * sinc
    taps /= taps.sum()
    return taps, half


def restated_lowpass_filter(x: torch.Tensor, cutoff: float, zeros: float = 8) -> torch.Tensor:
    taps, half = restated_taps(cutoff, zeros)
    flat = x.reshape(-1, 1, x.shape[-1])
    out = F.conv1d(F.pad(flat, (half, half), mode="replicate"), taps.to(x.dtype)[None, None])
    return out.reshape(x.shape)


class _Info(dict):
    pass


class _RawArray:
    def __init__(self, data, info):
        self.data, self.info = np.asarray(data), info

    def get_data(self):
        return self.data


def _function(tree_body, name):
    fn = next(n for n in tree_body if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.decorator_list = []
    fn.returns = None
    for arg in fn.args.args:
        arg.annotation = None
    return fn


def reference_functions(dtype):
    """``(preprocess_mne, Recording.preprocessed)`` of bm/studies/api.py as plain functions over the stubs, with
    ``torch.Tensor(array)`` converting to ``dtype`` (fp32: what the reference's own call does)."""
    from _ref_import import REF
    path = REF / "bm" / "studies" / "api.py"
    tree = ast.parse(path.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Recording")
    fns = [_function(tree.body, "preprocess_mne"), _function(cls.body, "preprocessed")]
    mne = types.SimpleNamespace(Info=_Info, find_layout=lambda info: None, io=types.SimpleNamespace(RawArray=_RawArray))
    julius = types.SimpleNamespace(ResampleFrac=AC.ResampleFrac, lowpass_filter=restated_lowpass_filter)
    torch_ns = types.SimpleNamespace(Tensor=lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).clone())
    scope = {"torch": torch_ns, "np": np, "mne": mne, "julius": julius, "tp": __import__("typing")}
    exec(compile(ast.Module(body=fns, type_ignores=[]), str(path), "exec"), scope)
    return scope["preprocess_mne"], scope["preprocessed"]


def build() -> dict:
    torch.set_num_threads(1)          # the CPU reductions in one fixed order: regeneration is bit-exact
    raw = raw_data()
    out = {"raw": raw}
    meta = dict(cases=CASES, errors={}, zeros=8, torch=torch.__version__)
    for name, case in CASES.items():
        for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
            preprocess_mne, _ = reference_functions(dtype)
            # mne hands out float64; the reference's torch.Tensor() makes fp32 of it
            arr = _RawArray(raw.astype(np.float64), _Info(sfreq=case["sfreq"]))
            low = preprocess_mne(arr, sample_rate=case["sample_rate"], highpass=case["highpass"])
            assert low.info["sfreq"] == case["sample_rate"] and low.get_data().dtype == \
                (np.float32 if dtype == torch.float32 else np.float64)
            out[f"{name}/{key}"] = low.get_data().copy()
    preprocess_mne, preprocessed = reference_functions(torch.float32)
    for name, case in ERRORS.items():
        arr = _RawArray(raw.astype(np.float64), _Info(sfreq=case["sfreq"]))
        try:
            if name == "rate_fraction":
                preprocessed(types.SimpleNamespace(), sample_rate=case["sample_rate"], highpass=case["highpass"])
            else:
                preprocess_mne(arr, sample_rate=case["sample_rate"], highpass=case["highpass"])
        except ValueError as exc:
            meta["errors"][name] = dict(case, message=str(exc))
        else:
            raise AssertionError(f"{name}: the reference raised nothing")
    out["meta"] = json.dumps(meta)
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "preprocess.npz", **out)
    print(f"preprocess: {len(out)} arrays -> {dest / 'preprocess.npz'} ({(dest / 'preprocess.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
