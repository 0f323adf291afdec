"""CPU checks of ``task.lowpass``: the taps against the generator's restatement of julius' formula, the guards of
``hip_ops.lowpass_filter`` and of the Solver, the fixture's layout and its generator, the new entry points and the
kernel's register / scratch budget on the cross-compiled unit."""
import ctypes
import json
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import make_lowpass_golden as G  # noqa: E402

# (cutoff, zeros) -> half of the Python expression int(zeros / cutoff / 2), in double
HALVES = [((30 / 120, 5), 10), ((20 / 120, 5), 15), ((40 / 100, 5), 6), ((60 / 120, 5), 5), ((5 / 120, 5), 60),
          ((1 / 120, 5), 300), ((13 / 100, 5), 19), ((20 / 100, 5), 12), ((30 / 120, 8), 16)]


@pytest.fixture(scope="module")
def z():
    raw = np.load(ROOT / "tests" / "golden" / "lowpass.npz")
    return {k: raw[k] for k in raw.files}


@pytest.mark.parametrize("args,half", HALVES)
def test_taps_are_the_restatement_s_bit_for_bit(args, half):
    from brainmagick_amd import hip_ops as H
    taps, got_half = H.lowpass_taps(*args)
    want, want_half = G.restated_taps(*args)
    assert got_half == want_half == half
    assert taps.dtype == torch.float32 and taps.device.type == "cpu" and taps.shape == (2 * half + 1,)
    assert torch.equal(taps.view(torch.int32), want.view(torch.int32))
    assert abs(float(taps.double().sum()) - 1.) < 1e-6                   # DC gain 1
    assert torch.equal(taps, taps.flip(0)) or float((taps - taps.flip(0)).abs().max()) < 1e-7     # linear phase
    again, _ = H.lowpass_taps(*args)
    assert again is taps                                                 # cached


def test_default_zeros_is_julius_eight():
    from brainmagick_amd import hip_ops as H
    assert H.lowpass_taps(30 / 120)[1] == 16


@pytest.mark.parametrize("cutoff", [-0.1, 0., 0.5000001, 3.])
def test_cutoff_outside_the_band_is_a_value_error(cutoff):
    from brainmagick_amd import hip_ops as H
    with pytest.raises(ValueError):
        H.lowpass_taps(cutoff, 5)
    with pytest.raises(ValueError):
        H.lowpass_filter(torch.zeros(2, 3, 8), cutoff, zeros=5)


def test_decimation_and_valid_convolution_are_not_built():
    from brainmagick_amd import hip_ops as H
    x = torch.zeros(2, 3, 8)
    with pytest.raises(NotImplementedError):
        H.lowpass_filter(x, 0.25, stride=2)
    with pytest.raises(NotImplementedError):
        H.lowpass_filter(x, 0.25, pad=False)


def test_lowpass_filter_has_no_cpu_fallback():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd._lib import BmHipError
    with pytest.raises(BmHipError):
        H.lowpass_filter(torch.randn(2, 3, 8), 0.25, zeros=5)
    with pytest.raises(BmHipError):
        H.lowpass_filter(torch.randn(2, 3, 8), 0.25, zeros=5, fft=True)      # accepted, ignored


def test_rows_of_a_view_are_recognised():
    from brainmagick_amd import hip_ops as H
    base = torch.zeros(2, 4, 70)
    assert H._uniform_rows(base) == 70 and H._uniform_rows(base[..., 6:]) == 70
    assert H._uniform_rows(base[:, 1:, 6:]) is None                      # the segments are not a whole number of rows apart
    assert H._uniform_rows(base[..., ::2]) is None
    assert H._uniform_rows(base[:1, :, 6:]) == 70 and H._uniform_rows(base[:, :1, 6:]) == 280
    assert H._uniform_rows(base.transpose(0, 1)) is None
    assert H._uniform_rows(torch.zeros(5)) == 5 and H._uniform_rows(torch.zeros(3, 1)) == 1
    assert H._uniform_rows(base[0, 0].expand(3, 70)) is None             # rows on top of each other


@pytest.mark.parametrize("kw", [dict(lowpass=-1.), dict(lowpass=60.0001), dict(lowpass=51., sample_rate=100.)])
def test_solver_refuses_a_cutoff_outside_the_band(kw):
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    with pytest.raises(ValueError, match="lowpass"):
        Solver(torch.nn.Conv1d(4, 4, 1), loss=L2Loss(), device="cpu", **kw)


def test_solver_keywords_default_to_the_reference_s():
    import inspect
    from brainmagick_amd.solver import Solver
    params = inspect.signature(Solver.__init__).parameters
    got = tuple(params[k].default for k in ("lowpass", "lowpass_gt", "lowpass_gt_test"))
    assert got == (0., True, False)                                      # bm/conf/config.yaml:139-147


def test_fixture_keys_and_shapes(z):
    meta = json.loads(str(z["meta"]))
    assert list(meta["cases"]) == list(G.CASES) and meta["eval_cases"] == G.EVAL_CASES and meta["zeros"] == 5
    from brainmagick_amd.models import ConvRNN, SimpleConv
    from brainmagick_amd.solver import encode_limit
    for name, case in G.CASES.items():
        spec = G.base_spec(name)
        B, T = spec["B"], spec["T"]
        assert z[f"{name}/mask"].shape == (B, 1, T) and z[f"{name}/mask"].dtype == np.bool_
        assert z[f"{name}/subjects"].shape == (B,)
        assert z[f"{name}/losses"].shape == (2,) and np.isfinite(z[f"{name}/losses"]).all()
        want = encode_limit(spec["meg_init"], spec["sample_rate"]) if case["task"] == "encode" else 0
        assert int(z[f"{name}/limit"]) == want
        for what in ("y", "meg", "target"):
            assert z[f"{name}/{what}@sample"].shape == (256,) and z[f"{name}/{what}@norm"].shape == ()
        model = G.build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), name)
        for k, p in model.named_parameters():
            assert f"{name}/sd/{k}" in z and (f"{name}/grad/{k}" in z or f"{name}/grad/{k}@sample" in z), (name, k)
            assert f"{name}/sd1/{k}" in z or f"{name}/sd1/{k}@sample" in z, (name, k)
    for name in G.EVAL_CASES:
        for what in ("y", "meg", "target"):
            assert z[f"{name}/{what}@sample"].shape == (256,)
    # the wiring the fixture pins: the model input does not depend on which target is chosen, the targets do
    assert np.array_equal(z["encode_l1_gt/meg@sample"], z["encode_l1_raw_gt/meg@sample"])
    assert not np.array_equal(z["encode_l1_gt/target@sample"], z["encode_l1_raw_gt/target@sample"])
    assert np.array_equal(z["eval_raw_gt/target@sample"], z["encode_l1_raw_gt/target@sample"])
    assert np.array_equal(z["eval_gt_test/target@sample"], z["encode_l1_gt/target@sample"])
    assert all(v.dtype != object for v in z.values())                    # arrays and one JSON string only


def test_lowpass_golden_is_reproduced_by_its_generator(tmp_path, z):
    from _ref_import import REF
    if not REF.exists():
        pytest.skip("the reference sources are not available here")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "make_lowpass_golden.py"), str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(tmp_path / "lowpass.npz")
    assert sorted(new.files) == sorted(z)
    for k in z:
        assert np.array_equal(new[k], z[k]), k


def test_lowpass_entry_points_are_declared_and_exported():
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    restype, argtypes, argnames = protos["bm_lowpass"]
    assert restype is ctypes.c_int
    assert argnames == ["x", "row_stride", "y", "rows", "T", "keep", "taps", "half", "amax_out", "workspace",
                        "workspace_bytes", "stream"]
    assert argtypes == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    assert protos["bm_lowpass_workspace_bytes"][:2] == (ctypes.c_long, [])
    if not _lib.LIB_PATH.exists():
        pytest.skip("libbmhip.so is not built here")
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    handle.bm_version.restype = ctypes.c_int
    assert handle.bm_version() >= 110
    handle.bm_lowpass_workspace_bytes.restype = ctypes.c_long
    assert handle.bm_lowpass_workspace_bytes() >= 64 + 4
    # host-side argument checks run without a GPU: no rows succeeds without a launch, bad arguments do not
    fn = handle.bm_lowpass
    fn.restype, fn.argtypes = restype, argtypes
    handle.bm_last_error.restype = ctypes.c_char_p
    assert fn(None, 8, None, 0, 8, 8, None, 2, None, None, 0, None) == 0
    assert fn(None, 8, None, 2, 8, 8, None, 2, None, None, 0, None) != 0          # null pointers with rows > 0
    assert fn(None, 7, None, 0, 8, 8, None, 2, None, None, 0, None) != 0          # rows that overlap
    assert fn(None, 8, None, 0, 0, 0, None, 2, None, None, 0, None) != 0
    assert fn(None, 8192, None, 0, 8192, 8, None, 0, None, None, 0, None) == 0    # the largest padded row
    assert fn(None, 8192, None, 0, 8190, 8, None, 1, None, None, 0, None) == 0
    assert fn(None, 8192, None, 0, 8191, 8, None, 1, None, None, 0, None) != 0    # one sample more
    assert b"8192" in handle.bm_last_error()                                      # the message names the limit


def test_lowpass_kernel_uses_no_scratch():
    """ISA audit on the cross-compiled unit, the method of test_step_kernels_keep_their_loops_free_of_scratch: the four
    instantiations (scalar / 16-byte stores x scalar / 16-byte loads) spill nothing and have no private segment."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "lowpass.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "lowpass.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+lowpass_kernel\w+):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 4, sorted(bodies)
    for kname, body in bodies.items():
        assert "scratch_" not in body, kname
        assert "v_fma_f32" in body or "v_fmac_f32" in body or "v_pk_fma_f32" in body, kname
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 8 and len(scratch) == 4
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)
