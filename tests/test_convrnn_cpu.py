"""CPU-only checks of ConvRNN: the model keeps the reference's state_dict contract for every case of the fixture
(tests/golden/convrnn.npz), refuses CPU tensors, the LSTM entry points are declared and defined, the step kernels'
loops are free of scratch accesses, and ``DualPathRNN`` is untouched."""
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

from helpers import GOLDEN, tensor_digest

sys.path.insert(0, str(GOLDEN))
import make_convrnn_golden as G  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ALL_CASES = list(G.CASES) + list(G.TRAIN_CASES)


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN / "convrnn.npz")
    return {k: z[k] for k in z.files}


def test_convrnn_is_exported():
    import brainmagick_amd.models as models
    from brainmagick_amd.models.convrnn import LSTM, Attention, ConvRNN
    assert models.ConvRNN is ConvRNN
    assert isinstance(LSTM(4, 4, 1, 0., False).lstm, torch.nn.LSTM) and Attention(8, heads=2).radius == 50


def test_fixture_lists_the_cases_of_the_generator(fixture):
    meta = json.loads(str(fixture["meta"]))
    assert meta["cases"] == list(G.CASES) and meta["train_cases"] == list(G.TRAIN_CASES)
    assert (meta["B"], meta["S"], meta["F"]) == (G.B, G.S, G.F_OUT)


@pytest.mark.parametrize("name", ALL_CASES)
def test_state_dict_contract(fixture, name):
    """Same keys, order and shapes as the reference's state_dict; same-seed construction (BatchNorm tensors randomised
    by the shared recipe afterwards) reproduces the reference's values bit for bit (exact digests); a state_dict in
    the reference's layout loads with strict=True."""
    from brainmagick_amd.models import ConvRNN
    model = G.build_model(ConvRNN, name)
    sd = model.state_dict()
    keys = json.loads(str(fixture[f"{name}/keys"]))
    shapes = json.loads(str(fixture[f"{name}/shapes"]))
    assert list(sd.keys()) == keys
    assert [list(v.shape) for v in sd.values()] == shapes
    for k, v in sd.items():
        if G.is_table(k):
            # Attention's table is smoothed by a running sum: equal to the reference's up to the host's summation order
            ref = torch.from_numpy(fixture[f"{name}/table/{k}"])
            assert np.array_equal(tensor_digest(ref), fixture[f"{name}/sd/{k}"]), (name, k)
            assert torch.allclose(v, ref, rtol=1e-5, atol=1e-6), (name, k)
        else:
            assert np.array_equal(tensor_digest(v), fixture[f"{name}/sd/{k}"]), (name, k)
    reference_layout = {k: torch.full(shape, 0.5, dtype=sd[k].dtype) for k, shape in zip(keys, shapes)}
    fresh = G.build_model(ConvRNN, name)
    fresh.load_state_dict(reference_layout, strict=True)
    assert all(bool((v == 0.5).all()) for v in fresh.state_dict().values() if v.is_floating_point())
    for k, v in G.make_input(name).items():
        assert np.array_equal(tensor_digest(v), fixture[f"{name}/in/{k}"]), (name, k)


@pytest.mark.parametrize("name", list(G.CASES))
def test_valid_length_follows_the_reference(fixture, name):
    from brainmagick_amd.models import ConvRNN
    model = G.build_model(ConvRNN, name)
    for length, valid in fixture[f"{name}/valid_length"]:
        assert model.valid_length(int(length)) == int(valid), (name, int(length))


def test_no_cpu_fallback():
    from brainmagick_amd.models import ConvRNN
    model = G.build_model(ConvRNN, "defaults")

    class Batch:
        subject_index = G.make_subjects("defaults")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(G.make_input("defaults"), Batch())
    from brainmagick_amd import functional as BF
    rnn = torch.nn.LSTM(4, 4, 1)
    with pytest.raises(RuntimeError):
        BF.LSTMFn.apply(torch.randn(2, 4, 3), 4, 1, False, 0., False, *rnn._flat_weights)


def test_lstm_entry_points_are_declared_and_defined():
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    source = (ROOT / "brainmagick_amd" / "csrc" / "lstm.hip").read_text()
    for name in ("bm_lstm_layer_fwd", "bm_lstm_layer_bwd"):
        assert name in protos, name
        assert re.search(r'extern\s+"C"\s+int\s+' + name + r"\s*\(", source), name
        assert hasattr(_lib.lib(), name)
    assert protos["bm_lstm_layer_fwd"][2][-5:] == ["H", "B", "T", "dirs", "stream"]


def test_step_kernels_keep_their_loops_free_of_scratch():
    """ISA audit on the cross-compiled unit, in the style of test_host_cpu.py's: both step kernels use the exact-fp32
    MFMA, spill nothing, have no private segment, and nothing between their first and last MFMA touches scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "lstm.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "lstm.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+lstm_step_\w+_kernel\w+):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 2 and any("fwd" in k for k in bodies) and any("bwd" in k for k in bodies), sorted(bodies)
    for kname, body in bodies.items():
        lines = body.splitlines()
        mf = [i for i, l in enumerate(lines) if "v_mfma" in l]
        assert mf and all("v_mfma_f32_32x32x2_f32" in lines[i] for i in mf), kname
        assert not [l for l in lines[mf[0]:mf[-1] + 1] if "scratch_" in l], kname
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 2 and len(scratch) == 2
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)


def test_dual_path_keeps_torch_lstm_modules():
    from brainmagick_amd.models.common import DualPathRNN
    dual = DualPathRNN(8, 2)
    assert len(dual.lstms) == 8 and all(type(m) is torch.nn.LSTM for m in dual.lstms)
