"""CPU checks of ``optim.svd``: the fixture's layout, which weights are penalised, the ``penalty_rng`` / ``proba``
bookkeeping, the guards of ``svd_penalty`` and of the Solver, the entry points, the stage kernel's scratch budget -- and
the closed-form gradient itself: an fp64 torch restatement of what ``csrc/spectral.hip`` computes (Cholesky-orthonormalised
bases, the backward chain of skinny products and triangular solves, the sum of rank-16 terms) against the reference's
fp64 value and autograd gradient.  At the end, the proofs of tests/svd_cases.py, the harness of
tests/test_svd_conditioning_gpu.py."""
import ctypes
import inspect
import json
import math
import random
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
import make_svd_golden as G  # noqa: E402
import make_lowpass_golden as LPG  # noqa: E402

from helpers import tensor_digest  # noqa: E402
import svd_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def z():
    raw = np.load(ROOT / "tests" / "golden" / "svd_penalty.npz")
    return {k: raw[k] for k in raw.files}


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def case_weight(z, name: str) -> torch.Tensor:
    """The case's weight: rebuilt from the seed and proven by the digest, or read from the fixture."""
    if f"{name}/w" in z:
        return torch.from_numpy(z[f"{name}/w"])
    w = G.make_weight(name)
    assert np.array_equal(tensor_digest(w), z[f"{name}/w_digest"]), name
    return w


def closed_form(A: torch.Tensor, R: torch.Tensor, niters: int):
    """(value, d value / d A) of ``torch.svd_lowrank(A, R.shape[1], niters)[1][0] ** 2`` given its test matrix R, in
    A's dtype, the way the kernels compute it: everything padded to 16 columns, X_k = M_k Q_{k-1}, Q_k = X_k L_k^{-T}
    with L_k the Cholesky factor of X_k^T X_k, the value the largest eigenvalue of the last Gram matrix; backwards
    G_X = (G_Q - Q_k Q_k^T G_Q) L_k^{-1}, G_Q <- M_k^T G_X; dAt = sum of U_k V_k^T."""
    rows, cols = A.shape
    wide = rows < cols
    At = A.t() if wide else A
    mt, nt = At.shape
    q = min(R.shape[1], nt)
    S = 2 * niters + 2
    Rp = torch.zeros(nt, 16, dtype=A.dtype)
    Rp[:, :q] = R[:, :q]
    M = [At if k % 2 == 0 else At.t() for k in range(S)]
    X, Qm, Linv = [None] * S, [None] * S, [None] * S
    Qm[0] = Rp
    for k in range(S):
        if k > 0:
            gram = X[k - 1].t() @ X[k - 1]
            Li = torch.zeros(16, 16, dtype=A.dtype)
            Li[:q, :q] = torch.linalg.inv(torch.linalg.cholesky(gram[:q, :q]))
            Linv[k - 1] = Li
            Qm[k] = X[k - 1] @ Li.t()
        X[k] = M[k] @ Qm[k]
    lam, vec = torch.linalg.eigh(X[S - 1].t() @ X[S - 1])
    value, u = lam[-1], vec[:, -1]
    GX, GQ = [None] * S, [None] * S
    GX[S - 1] = X[S - 1] @ (2 * torch.outer(u, u))
    GQ[S - 2] = At @ GX[S - 1]
    for k in range(S - 2, -1, -1):
        C = Qm[k + 1].t() @ GQ[k]
        GX[k] = GQ[k] @ Linv[k] - Qm[k + 1] @ (C @ Linv[k])
        if k > 0:
            GQ[k - 1] = M[k].t() @ GX[k]
    dAt = torch.zeros_like(At)
    for k in range(S):
        U, V = (GX[k], Qm[k]) if k % 2 == 0 else (Qm[k], GX[k])
        dAt = dAt + U @ V.t()
    return value, (dAt.t() if wide else dAt)


def _case_keys(meta):
    return list(meta["cases"]) + list(meta["variants"])


def _case_args(meta, key):
    var = meta["variants"].get(key, {})
    return var.get("case", key), var.get("dim", 16), var.get("niters", 2)


def test_fixture_keys_and_shapes(z, meta):
    assert list(meta["cases"]) == list(G.CASES) and meta["variants"] == G.VARIANTS and meta["svd"] == G.SVD
    for key in _case_keys(meta):
        name, dim, _ = _case_args(meta, key)
        shape = tuple(G.make_layer(G.CASES[name]["layer"]).weight.shape)
        rows, cols = shape[0], math.prod(shape[1:])
        assert z[f"{key}/R"].shape == (min(rows, cols), dim) and z[f"{key}/R"].dtype == np.float32
        assert z[f"{key}/grad64"].shape == shape
        assert z[f"{key}/grad64"].dtype == (np.float32 if G.CASES[name].get("grad_fp32") else np.float64)
        assert z[f"{key}/value64"].dtype == np.float64 and z[f"{key}/value32"].dtype == np.float32
        assert len(meta["dev"][key]) == 2 and all(0 <= d < 1e-4 for d in meta["dev"][key])
        assert case_weight(z, name).shape == shape
    assert meta["dev_median"] == [float(np.median([meta["dev"][k][i] for k in G.CASES])) for i in range(2)]
    assert z["proba/applied"].shape == (8,) and z["proba/applied"].dtype == np.bool_
    assert z["train/losses"].shape == (2,) and np.isfinite(z["train/losses"]).all()
    from brainmagick_amd.models import ConvRNN, SimpleConv
    model = LPG.build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), meta["train_case"])
    for k, p in model.named_parameters():
        assert z[f"train/grad/{k}"].shape == tuple(p.shape)
    for k, v in model.state_dict().items():
        assert np.array_equal(tensor_digest(v), z[f"train/sd/{k}"]), k
        assert z[f"train/sd1/{k}"].shape == tuple(v.shape) and z[f"train/sd2/{k}"].shape == tuple(v.shape)
    for step in range(2):
        for i, name in enumerate(meta["names"]["simpleconv"]):
            w = dict(model.named_parameters())[name]
            assert z[f"train/R/{step}/{i}"].shape == (min(w.shape[0], w.numel() // w.shape[0]), 16)
    assert all(v.dtype != object for v in z.values())                    # arrays and one JSON string only
    assert (ROOT / "tests" / "golden" / "svd_penalty.npz").stat().st_size <= 1 << 20


def test_svd_golden_is_reproduced_by_its_generator(tmp_path, z):
    from _ref_import import REF
    if not REF.exists():
        pytest.skip("the reference sources are not available here")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "make_svd_golden.py"), str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(tmp_path / "svd_penalty.npz")
    assert sorted(new.files) == sorted(z)
    for k in z:
        assert np.array_equal(new[k], z[k]), k


@pytest.mark.parametrize("tag,case", [("simpleconv", G.TRAIN_CASE), ("convrnn", G.RNN_CASE)])
def test_penalized_weights_are_the_reference_s(meta, tag, case):
    from brainmagick_amd.models import ConvRNN, SimpleConv
    from brainmagick_amd.svd import penalized_weights
    model = LPG.build_model(dict(convrnn=ConvRNN, simpleconv=SimpleConv), case)
    got = penalized_weights(model)
    assert [k for k, _ in got] == meta["names"][tag]
    params = dict(model.named_parameters())
    assert all(p is params[k] for k, p in got)
    assert penalized_weights(model, min_size=1e9) == []


def test_the_size_threshold_keeps_256_elements_and_skips_255():
    from brainmagick_amd.svd import penalized_weights
    model = torch.nn.Sequential(G.make_layer(G.SKIPPED), G.make_layer(G.CASES["lin_16x16"]["layer"]), torch.nn.GELU(),
                                torch.nn.BatchNorm1d(300), G.make_layer(G.CASES["depthwise_300x1x1"]["layer"]))
    assert model[0].weight.shape == (15, 17)
    assert [k for k, _ in penalized_weights(model)] == ["1.weight", "4.weight"]
    assert [k for k, _ in penalized_weights(model, min_size=300 / 256)] == ["4.weight"]
    assert [k for k, _ in penalized_weights(model, min_size=0.)] == ["0.weight", "1.weight", "4.weight"]
    assert [k for k, _ in penalized_weights(torch.nn.Linear(16, 16))] == ["weight"]


def test_proba_draws_from_penalty_rng_like_the_reference(z, monkeypatch):
    """The reference's bookkeeping (bm/svd.py:30-31, 45) with the estimate patched to a constant: eight calls at
    proba = 0.5 from a fresh ``random.Random(1234)`` are applied where the fixture says, an applied call is the estimate
    over proba, a skipped one the float 0 and launches nothing."""
    from brainmagick_amd import svd
    assert isinstance(svd.penalty_rng, random.Random)
    monkeypatch.setattr(svd, "penalty_rng", random.Random(1234))
    calls = []

    def constant(weights, dim, niters, generator=None, test_matrices=None):
        calls.append((len(weights), dim, niters))
        return torch.tensor(3.)
    monkeypatch.setattr(svd, "_estimate_sum", constant)
    model = torch.nn.Linear(16, 16)
    got = [svd.svd_penalty(model, proba=0.5) for _ in range(8)]
    applied = [isinstance(v, torch.Tensor) for v in got]
    assert applied == z["proba/applied"].tolist()
    ratios = [float(v) / 3. for v in got if isinstance(v, torch.Tensor)]
    assert ratios == z["proba/ratio"].tolist() == [2.] * len(ratios)
    assert all(v == 0. and isinstance(v, float) for v in got if not isinstance(v, torch.Tensor))
    assert calls == [(1, 16, 2)] * sum(applied)
    # proba = 1 still draws (the reference does), and a model without a penalised weight returns 0. without a launch
    state = svd.penalty_rng.getstate()
    assert svd.svd_penalty(torch.nn.Linear(3, 3)) == 0. and svd.penalty_rng.getstate() != state
    assert len(calls) == sum(applied)


def test_limits_are_value_errors_that_name_the_limit():
    from brainmagick_amd import svd
    model = torch.nn.Linear(16, 16)
    state = svd.penalty_rng.getstate()
    with pytest.raises(ValueError, match="16"):
        svd.svd_penalty(model, dim=17)
    with pytest.raises(ValueError, match="16"):
        svd.svd_penalty(model, dim=0)
    with pytest.raises(ValueError, match="8"):
        svd.svd_penalty(model, niters=9)
    with pytest.raises(ValueError, match="8"):
        svd.svd_penalty(model, niters=-1)
    with pytest.raises(NotImplementedError, match="exact"):
        svd.svd_penalty(model, exact=True)
    assert svd.penalty_rng.getstate() == state
    with pytest.raises(ValueError, match="test matri"):
        svd._estimate_sum([model.weight], 16, 2, test_matrices=[])
    with pytest.raises(ValueError, match=r"\(16, 16\)"):
        svd._estimate_sum([model.weight], 16, 2, test_matrices=[torch.zeros(16, 15)])


def test_svd_penalty_has_no_cpu_fallback():
    from brainmagick_amd import svd
    from brainmagick_amd._lib import BmHipError
    with pytest.raises(BmHipError):
        svd.svd_penalty(torch.nn.Linear(16, 16), test_matrices=[torch.zeros(16, 16)])


def test_signatures_follow_the_reference():
    from brainmagick_amd import svd
    from brainmagick_amd.solver import Solver
    params = inspect.signature(svd.svd_penalty).parameters
    assert list(params) == ["model", "min_size", "dim", "niters", "proba", "exact", "generator", "test_matrices"]
    assert [params[k].default for k in list(params)[1:]] == [1., 16, 2, 1, False, None, None]     # bm/svd.py:17
    solver = inspect.signature(Solver.__init__).parameters
    assert list(solver)[-1] == "svd" and solver["svd"].default == 0.                                # bm/conf/config.yaml:52


def test_solver_refuses_a_negative_weight_before_it_touches_the_device():
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.solver import Solver
    with pytest.raises(ValueError, match="svd"):
        Solver(torch.nn.Conv1d(4, 4, 1), loss=L2Loss(), device="cpu", svd=-0.1)


def test_closed_form_reproduces_the_reference_in_fp64(z, meta):
    """The derivation itself, without a GPU: the restatement in fp64 with the fixture's R against the reference's fp64
    value and autograd gradient to 1e-10 (the case whose gradient is stored in fp32: to that rounding, 1e-7)."""
    for key in _case_keys(meta):
        name, dim, niters = _case_args(meta, key)
        w = case_weight(z, name).double()
        value, grad = closed_form(w.view(w.shape[0], -1), torch.from_numpy(z[f"{key}/R"]).double(), niters)
        want_v, want_g = float(z[f"{key}/value64"]), torch.from_numpy(z[f"{key}/grad64"]).double().view(w.shape[0], -1)
        tol = 1e-7 if G.CASES[name].get("grad_fp32") else 1e-10
        assert abs(float(value) - want_v) <= 1e-10 * want_v, (key, float(value), want_v)
        err = float((grad - want_g).norm() / want_g.norm())
        assert err <= tol, (key, err)


def test_a_frozen_subspace_gradient_is_not_the_gradient(z):
    """Why the chain terms exist: 2 sigma u v^T of the frozen basis misses the reference's gradient by tens of percent
    on an un-gapped matrix."""
    key = "gauss_160x480"
    w = case_weight(z, key).double()
    u, s, vh = torch.linalg.svd(w)
    want = torch.from_numpy(z[f"{key}/grad64"]).double()
    # even the EXACT top triple is far from the estimate's gradient; the frozen-basis one is no closer
    assert float((2 * s[0] * torch.outer(u[:, 0], vh[0]) - want).norm() / want.norm()) > 0.1


def test_spectral_entry_points_are_declared_and_exported():
    from brainmagick_amd import _lib
    protos = _lib.parse_header()
    assert protos["bm_spectral_fwd"][2] == ["table", "nmat", "max_slabs", "R", "dim", "niters", "ws_floats",
                                            "ws_doubles", "values", "total", "stream"]
    assert protos["bm_spectral_bwd"][2] == ["table", "nmat", "max_slabs", "max_tiles", "niters", "ws_floats",
                                            "ws_doubles", "gscale", "grads", "stream"]
    assert protos["bm_spectral_table_entry_bytes"][:2] == (ctypes.c_long, [])
    header = _lib.HEADER.read_text()
    assert "bm/svd.py:17-45" in header and "bm/solver.py:379-380" in header
    if not _lib.LIB_PATH.exists():
        pytest.skip("libbmhip.so is not built here")
    L = _lib.lib()
    assert L.bm_version() >= 111
    # host-side functions run without a GPU
    assert L.bm_spectral_ws_floats(320, 960, 2) == 4 * 6 * 960 * 16
    assert L.bm_spectral_ws_floats(17, 300, 0) == 4 * 2 * 320 * 16
    assert L.bm_spectral_ws_doubles(40, 17, 2) == 2 * 6 * 256 + 6 * 256 + 32
    entry = torch.zeros(L.bm_spectral_table_entry_bytes(), dtype=torch.uint8)
    fill = L.bm_spectral_table_fill
    assert fill(entry.data_ptr(), None, 40, 17, 17, 16, 0, 0, 0, 0) == 0
    assert fill(entry.data_ptr(), None, 40, 17, 16, 16, 0, 0, 0, 0) != 0            # rows that overlap
    assert fill(entry.data_ptr(), None, 40, 17, 17, 17, 0, 0, 0, 0) != 0 and b"16" in L.bm_last_error()
    assert fill(entry.data_ptr(), None, 40, 17, 17, 16, 0, 8, 0, 0) != 0            # 64-byte aligned operand rows
    assert L.bm_spectral_fwd(None, 0, 0, None, 16, 2, None, None, None, None, None) == 0      # no matrix: no launch
    assert L.bm_spectral_fwd(None, 0, 0, None, 16, 9, None, None, None, None, None) != 0 and b"8" in L.bm_last_error()
    assert L.bm_spectral_fwd(None, 1, 1, None, 16, 2, None, None, None, None, None) != 0      # null pointers
    assert L.bm_spectral_bwd(None, 0, 0, 0, 2, None, None, None, None, None) == 0
    assert L.bm_spectral_bwd(None, 1, 1, 1, 2, None, None, None, None, None) != 0


def test_spectral_kernels_use_no_scratch():
    """ISA audit on the cross-compiled unit: no kernel of spectral.hip spills or has a private segment, and the
    products are the exact-fp32 MFMA."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "spectral.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "spectral.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+spectral_\w+_kernel\w+):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 4, sorted(bodies)
    for kname, body in bodies.items():
        assert "scratch_" not in body, kname
        if "stage" in kname or "dw" in kname:
            assert "v_mfma_f32_16x16x4_f32" in body, kname
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 8 and len(scratch) == 4
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)


# ---- the harness of tests/test_svd_conditioning_gpu.py (tests/svd_cases.py), proven without a GPU -----------------------------
@pytest.mark.parametrize("name", ["gauss_150x70", "gauss_70x150"])
def test_lowrank_ref_is_torch_svd_lowrank_with_its_draw_given(name):
    """``svd_cases.lowrank_ref`` against ``torch.svd_lowrank`` itself in fp64, fed the same R through the tap the
    fixture's generator uses: 1e-12 relative (measured 1.5e-15), one tall and one wide matrix."""
    w, R, niters = SC.shape_case(name)
    with G.RandnTap(replay=[R]) as tap:
        want = torch.svd_lowrank(w.double(), SC.DIM, niters)[1][0] ** 2
    assert len(tap.seen) == 1
    got, _ = SC.lowrank_ref(w.double(), R, niters, want_grad=False)
    err = abs(float(got) - float(want)) / float(want)
    print(f"{name}: lowrank_ref against torch.svd_lowrank {err:.2e}")
    assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_shape_cases_keep_the_yardstick_meaningful(name):
    """The tolerance of a shape case is a multiple of its own fp32-vs-fp64 deviation of the reference: that deviation
    is capped, so a seed at which the reference itself is badly off cannot make the GPU test vacuous."""
    _, g64, dev = SC.shape_truth(name)
    cap = SC.GRAD_DEV_CAP * SC.dev_median()[1]
    print(f"{name}: reference fp32-vs-fp64 value {dev[0]:.2e}, gradient {dev[1]:.2e} / cap {cap:.2e}")
    assert bool(torch.isfinite(g64).all())
    assert dev[1] <= cap, (name, dev, cap)


@pytest.mark.parametrize("name", list(SC.LADDER))
def test_the_analytic_truth_is_the_estimate_s_on_the_ladder(name):
    """The condition for holding the kernels to ``sigma_1 ** 2`` and ``2 sigma_1 u v^T``: the reference's algorithm in
    fp64 gives them, value and autograd gradient, to 1e-9 (measured 2e-14 or better).  A case that fails this is
    replaced, not loosened."""
    w, R, niters = SC.ladder_case(name)
    value, grad, _ = SC.ladder_truth(name)
    v64, g64 = SC.lowrank_ref(w.double(), R, niters)
    err_v, err_g = abs(float(v64) - float(value)) / float(value), SC.rel(g64, grad)
    print(f"{name}: fp64 lowrank_ref against the analytic truth: value {err_v:.2e}, gradient {err_g:.2e}")
    assert err_v <= 1e-9 and err_g <= 1e-9, (name, err_v, err_g)


@pytest.mark.parametrize("name", list(SC.SINGULAR))
def test_the_analytic_truth_is_the_estimate_s_at_a_singular_gram_matrix(name):
    """With min(rows, cols) <= 16 the basis spans the whole row space: the reference's fp64 VALUE is ``sigma_1 ** 2`` to
    1e-9 (measured 2e-15).  Its autograd gradient divides by the zero pivot of R and is no truth; that the analytic one is
    the gradient of that value is shown by the value itself, as a central difference along a random direction."""
    w, R, niters = SC.ladder_case(name)
    value, grad, _ = SC.ladder_truth(name)
    v64, _ = SC.lowrank_ref(w.double(), R, niters, want_grad=False)
    err_v = abs(float(v64) - float(value)) / float(value)
    D = torch.randn(w.shape, generator=SC.gen(name + "/direction"), dtype=torch.float64)
    D = D / D.norm()
    h = 1e-5                                           # truncation ~ h^2 |f'''| / 6, rounding ~ 1e-16 / h: both ~ 1e-10
    up, _ = SC.lowrank_ref(w.double() + h * D, R, niters, want_grad=False)
    down, _ = SC.lowrank_ref(w.double() - h * D, R, niters, want_grad=False)
    slope, want = float(up - down) / (2 * h), float((grad * D).sum())
    err_d = abs(slope - want) / float(grad.norm())
    print(f"{name}: fp64 lowrank_ref value against sigma_1^2 {err_v:.2e}; directional derivative {err_d:.2e}")
    assert err_v <= 1e-9, (name, err_v)
    assert err_d <= 1e-7, (name, slope, want)
