"""The host side of the MEG preprocessing without a GPU: the fixture's wiring cases (tests/golden/
make_preprocess_golden.py: the live reference's ``preprocess_mne`` around the restatements) against the same chain
restated, the filter lengths of the highpass rates in use, every limit, the declared entry points and the ISA of
csrc/fir.hip.  Reads the fixture only."""
import inspect
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import preprocess_cases as PC


def test_fixture_is_the_wiring_around_the_restatements():
    """Resample first, then ``data -= lowpass(data, highpass / sample_rate)`` with ``zeros = 8``, ``old_sr`` the rounded
    ``sfreq``: the same torch ops in the order the live reference ran them, equal up to the order of the CPU's
    reductions (the values are of order 100, and of order 1 behind a highpass)."""
    fx = PC.fixture()
    raw = torch.from_numpy(fx["raw"])
    assert raw.shape == (3, 6000) and raw.dtype == torch.float32
    assert float(raw.mean(1).abs().min()) > 70 * float((raw - raw.mean(1, keepdim=True)).std())   # why one high-passes
    assert set(fx["meta"]["cases"]) == {"down_1200_120", "down_1000_120_hp", "sfreq_1199_7", "same_120_hp"}
    assert fx["meta"]["zeros"] == 8
    for name, case in fx["meta"]["cases"].items():
        old_sr = int(np.round(case["sfreq"]))
        for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
            want = torch.from_numpy(fx[f"{name}/{key}"])
            got = PC.chain(raw, case, dtype)
            assert got.dtype == want.dtype == dtype and got.shape == want.shape == (3, case["sample_rate"] * 6000 // old_sr)
            assert torch.allclose(got, want, rtol=0, atol=2e-3 if dtype == torch.float32 else 1e-10), (name, key)
        if case["highpass"]:
            # the other order (filter, then resample) and another `zeros` are other functions: the fixture tells them apart
            from brainmagick_amd import hip_ops as H
            import audio_cases as AC
            want = torch.from_numpy(fx[f"{name}/out64"])
            assert float(want.abs().max()) < 10.0                              # the offsets are gone
            x = raw.double()
            if old_sr != case["sample_rate"]:
                first = x - PC.lowpass(x, H.lowpass_taps(case["highpass"] / case["sample_rate"], 8)[0])
                other = AC.ResampleFrac(old_sr, case["sample_rate"])(first)
                assert float((other - want).abs().max()) > 1e-3
            z = AC.ResampleFrac(old_sr, case["sample_rate"])(x)
            other = z - PC.lowpass(z, H.lowpass_taps(case["highpass"] / case["sample_rate"], 5)[0])
            assert float((other - want).abs().max()) > 1e-3
    a, b = fx["down_1200_120/out64"], fx["sfreq_1199_7/out64"]
    assert a.shape == b.shape and not np.array_equal(a, b)                     # 1199.7 rounds to 1200; that case high-passes
    errors = fx["meta"]["errors"]
    assert errors["rate_above"]["message"] == "The sample rate should be below 1000Hz, got 1200"
    assert "only integer sampling rates in Hz are allowed" in errors["rate_fraction"]["message"]


@pytest.mark.parametrize("highpass,rate,half", PC.HALVES)
def test_half_of_the_rates_in_use(highpass, rate, half):
    """``int()`` of a Python float division decides the length, as in julius."""
    from brainmagick_amd import hip_ops as H
    taps, h = H.lowpass_taps(highpass / rate, 8)
    assert h == half == int(8 / (highpass / rate) / 2) and taps.shape == (2 * half + 1,) and taps.dtype == torch.float32
    assert half <= H.FIR_MAX_HALF
    assert abs(float(taps.double().sum()) - 1.0) <= (2 * half + 1) * 2.0 ** -24


def test_every_limit_raises_its_value_error():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.dataset import DeviceRecording, preprocess_meg
    x = torch.zeros(3, 100)
    taps = torch.zeros(5)
    with pytest.raises(ValueError, match="odd length"):
        H.fir_rows(x, torch.zeros(4))
    with pytest.raises(ValueError, match="odd length"):
        H.fir_rows(x, torch.zeros(1, 5))
    with pytest.raises(ValueError, match=f"half <= {H.FIR_MAX_HALF}"):
        H.fir_rows(x, torch.zeros(2 * H.FIR_MAX_HALF + 3))
    with pytest.raises(ValueError, match=r"1 <= T < 2\^31"):
        H.fir_rows(torch.zeros(3, 0), taps)
    with pytest.raises(ValueError, match=r"1 <= T < 2\^31"):
        H.fir_rows(torch.empty(1, 2 ** 31, device="meta"), taps)
    with pytest.raises(ValueError, match="limit is 65535"):
        H.fir_rows(torch.empty(65536, 4, device="meta"), taps)
    with pytest.raises(RuntimeError):                                          # within the limits: no CPU fallback
        H.fir_rows(x, taps)
    for cutoff, match in ((-0.1, "larger than zero"), (0.6, "above 0.5"), (0.0, "not a filter")):
        with pytest.raises(ValueError, match=match):
            H.highpass_filter(x, cutoff)
    with pytest.raises(ValueError, match=f"half <= {H.FIR_MAX_HALF}"):
        H.highpass_filter(x, 0.01 / 120)                                       # half = 48 000
    with pytest.raises(NotImplementedError, match="stride"):
        H.highpass_filter(x, 0.1, stride=2)
    with pytest.raises(NotImplementedError, match="pad=False"):
        H.highpass_filter(x, 0.1, pad=False)
    with pytest.raises(RuntimeError):
        H.highpass_filter(x, 0.1, fft=True)
    with pytest.raises(ValueError, match="channels, samples"):
        H.resample_rows(torch.zeros(100), 10, 1)
    with pytest.raises(ValueError, match="integers"):
        H.resample_rows(x, 1000.5, 120)
    with pytest.raises(ValueError, match="at most 16384"):
        H.resample_rows(x, 1100, 1099)
    assert H.resample_rows(x, 120, 120) is x
    with pytest.raises(RuntimeError):
        H.resample_rows(x, 1200, 120)
    with pytest.raises(ValueError, match="only integer sampling rates in Hz are allowed"):
        preprocess_meg(x, 1000.0, 120.5)
    with pytest.raises(ValueError, match="The sample rate should be below 1000Hz, got 1200"):
        preprocess_meg(x, 1000.4, 1200)
    with pytest.raises(ValueError, match="above 0.5"):
        preprocess_meg(x, 1000.0, 120, 61.0)
    with pytest.raises(ValueError, match="channels, samples"):
        preprocess_meg(torch.zeros(100), 1000.0, 120)
    with pytest.raises(ValueError, match="should be below"):
        DeviceRecording.from_raw(x, 100.0, 120, recording=None, subject_index=0)


def test_library_declares_the_fir_entry_points():
    from brainmagick_amd import _lib
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.dataset import DeviceRecording, preprocess_meg
    L = _lib.lib()
    assert L.bm_version() >= 117
    protos = _lib.parse_header()
    assert {"bm_fir_rows", "bm_fir_tile", "bm_fir_chunk", "bm_fir_max_half"} <= set(protos)
    assert protos["bm_fir_rows"][2] == ["x", "row_stride", "y", "rows", "T", "taps", "ntaps", "subtract", "stream"]
    tile, chunk = H.fir_tile(), H.fir_chunk()
    assert tile >= 1024 and tile % 256 == 0 and chunk % 16 == 0 and chunk >= 16
    assert (tile + chunk + 15) * 4 <= 65536                                    # the staged samples: at most 64 KiB of LDS
    assert int(L.bm_fir_max_half()) == H.FIR_MAX_HALF >= 16384

    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}
    assert list(inspect.signature(H.fir_rows).parameters) == ["x", "taps", "subtract"]
    assert defaults(H.fir_rows) == dict(subtract=False)
    assert list(inspect.signature(H.highpass_filter).parameters) == ["x", "cutoff", "stride", "pad", "zeros", "fft"]
    assert defaults(H.highpass_filter) == dict(stride=1, pad=True, zeros=8, fft=None)
    assert list(inspect.signature(H.resample_rows).parameters) == ["x", "old_sr", "new_sr", "zeros", "rolloff"]
    assert defaults(H.resample_rows) == dict(zeros=24, rolloff=0.945)
    assert list(inspect.signature(preprocess_meg).parameters) == ["raw", "sfreq", "sample_rate", "highpass"]
    assert defaults(preprocess_meg) == dict(highpass=0.)
    assert list(inspect.signature(DeviceRecording.from_raw).parameters) == ["raw", "sfreq", "sample_rate", "highpass", "kw"]


def test_fir_kernel_uses_no_scratch_and_the_exact_fp32_mfma():
    """ISA audit of the cross-compiled unit; it reads the spill and private-segment metadata, the LDS size and the MFMA
    mnemonic."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = Path(__file__).resolve().parent.parent / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "fir.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "fir.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+\w*_kernel\w*):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 1 and "fir_rows_kernel" in next(iter(bodies)), sorted(bodies)
    body = next(iter(bodies.values()))
    assert body.count("v_mfma_f32_16x16x4_f32") >= 16                          # four blocks x four steps share the B operands
    assert not re.search(r"v_mfma_(?!f32_16x16x4_f32)", body)                  # and no other matrix instruction
    assert "atomic" not in body
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    lds = [int(l.split(":")[1]) for l in text.splitlines() if ".group_segment_fixed_size" in l]
    assert len(spills) == 2 and len(scratch) == 1 and len(lds) == 1
    assert all(s == 0 for s in spills) and scratch == [0], (spills, scratch)
    assert 0 < lds[0] <= 65536, lds
