"""ClipLoss over a candidate set that is walked in row blocks (brainmagick_amd/functional.py, ``_candidate_blocks``).

From ``_CLIP_BLOCK_BYTES`` on the candidates are cut into row blocks: the forward runs one ``gemm_nt`` per block into a
column window of one score matrix (strided scalar stores from a pointer that is only 4-byte aligned when the window
starts at an odd column), dEst accumulates in place over one ``conv_nn`` per block (in f16x2 mode every launch drops the
maximum published for ``dest`` and attaches a fresh slot), dCand takes one ``conv_nn`` per block into a row window, and
in f16x2 mode the blocks of one call need not run in one kernel family.  Production reaches this at 8 GPUs with
wav2vec2-sized candidates (3 GB); here the limit is lowered with ``monkeypatch`` and kilobyte-sized inputs take the
same path -- except in the one test at the real limit.

Every case first pins the block list, then holds scores, loss, dEst and dCand to the same expression in torch on the CPU
in float64 (tolerances and the ``_held`` rule of tests/test_row_kernels_gpu.py: the fp32 CPU error is printed beside the
kernel's and has to stay below a quarter of the tolerance), runs the blocked path twice (bit-identical) and once more
with the limit restored (both held to fp64; their distance is printed -- the split order differs, so not bit-equal).

| case | B | Bc | K = Fd x T | rows -> blocks | targets at | reaches |
| A | 130 | 300 | 24 x 77 | 128 -> 128, 128, 44 | 128 | 128-rounded blocks + ragged tail; targets span blocks 1 and 2 |
|   |     |     |         |          |     | f16x2: wide kernels for the full blocks (ragged last K chunk), 3 x bf16 for the 44 rows |
| B | 5 | 30 | 8 x 12 | 7 -> 7, 7, 7, 7, 2 | 12 | windows at r0 = 7, 14, 21 and a row stride of 30: misaligned both ways |
| C | 3 | 5 | 8 x 12 | 1 -> five blocks of one row | 1 | the max(1, ...) floor |
| D | 130 | 300 | 7 x 151 | 128 -> 128, 128, 44 | 170 | odd K: every candidate and estimate row is only 4-byte aligned |
| E | 256 | 256 | 24 x 77 | 128 -> 128, 128 | 0 | B == Bc, the reference's own configuration, no ragged block |"""
import functools
import time

import pytest
import torch
from torch.nn import functional as F

from helpers import rel_l2
from oracle import bm_oracle as O
from test_guard_bands_gpu import Arena
from test_kernels_gpu import FWD_TOL, GRAD_TOL
from test_row_kernels_gpu import _held

pytestmark = pytest.mark.gpu

MODES = ("f32", "f32x3", "f16x2")
SCALE = 1.7                     # the gradient that arrives at the loss
INF = float("inf")

CASES = {
    "A": dict(B=130, Bc=300, Fd=24, T=77, rows=128, blocks=[(0, 128), (128, 128), (256, 44)], off=128,
              masked=(3, 127, 299), seed=11),
    "B": dict(B=5, Bc=30, Fd=8, T=12, rows=7, blocks=[(0, 7), (7, 7), (14, 7), (21, 7), (28, 2)], off=12,
              masked=(0, 29), seed=12),
    "C": dict(B=3, Bc=5, Fd=8, T=12, rows=1, blocks=[(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)], off=1, masked=(), seed=13),
    "D": dict(B=130, Bc=300, Fd=7, T=151, rows=128, blocks=[(0, 128), (128, 128), (256, 44)], off=170, masked=(),
              seed=14),
    "E": dict(B=256, Bc=256, Fd=24, T=77, rows=128, blocks=[(0, 128), (128, 128)], off=0, masked=(), seed=15),
}
VARIANTS = {
    "plain": dict(),
    "valid": dict(valid=True),
    "symmetric": dict(symmetric=True),
    "cand": dict(cand_grad=True),
    "cand_nonorm": dict(cand_grad=True, normalize=False),
}
RUNS = [(c, v) for c, vs in (("A", ("plain", "valid", "symmetric", "cand")),
                             ("B", ("plain", "valid", "symmetric", "cand", "cand_nonorm")),
                             ("C", ("plain", "cand")), ("D", ("plain", "cand")), ("E", ("plain", "symmetric")))
        for v in vs]


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    yield hip_ops
    hip_ops.set_compute_dtype(hip_ops.DEFAULT_COMPUTE_DTYPE)


@pytest.fixture(scope="module")
def BF():
    from brainmagick_amd import functional
    return functional


@pytest.fixture(params=MODES)
def mode(request, H):
    H.set_compute_dtype(request.param)
    yield request.param
    H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)


# ---- inputs and the reference --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(est [B, Fd, T], cand [Bc, Fd, T], col_valid [Bc]) in fp32 on the CPU; the targets are planted (scores ~1 above
    the rest, far from saturation) and the masked candidates lie outside the target block (else the loss is inf)."""
    c = CASES[case]
    g = torch.Generator().manual_seed(c["seed"])
    est = torch.randn(c["B"], c["Fd"], c["T"], generator=g) * 0.5
    cand = torch.randn(c["Bc"], c["Fd"], c["T"], generator=g) * 1.5 + 0.2
    est += 0.02 * cand[c["off"]:c["off"] + c["B"]]
    valid = torch.ones(c["Bc"])
    valid[list(c["masked"])] = 0
    assert not any(c["off"] <= m < c["off"] + c["B"] for m in c["masked"])
    return est, cand, valid


def _clip_reference(est, cand, off, valid, symmetric, normalize, dtype):
    """The operation in plain torch on the CPU in ``dtype``: scores (masked columns -inf), row probabilities, loss, and
    the gradients of ``loss * SCALE`` w.r.t. estimates and candidates."""
    e = est.detach().to(dtype, copy=True).requires_grad_(True)
    c = cand.detach().to(dtype, copy=True).requires_grad_(True)
    B = e.shape[0]
    ef, cf = e.flatten(1), c.flatten(1)
    s = ef @ cf.t()
    if normalize:
        s = s / (1e-8 + cf.norm(dim=1))
    if valid is not None:
        s = s.masked_fill(valid == 0, -INF)
    loss = F.cross_entropy(s, torch.arange(B) + off)
    if symmetric:
        loss = 0.5 * (loss + F.cross_entropy(s[:, off:off + B].t(), torch.arange(B)))
    (loss * SCALE).backward()
    return dict(scores=s.detach(), probs=torch.softmax(s.detach(), 1), loss=loss.detach(), dest=e.grad, dcand=c.grad)


@functools.lru_cache(maxsize=None)
def _references(case, variant):
    """(fp64, fp32) references of a case, computed once and shared by every mode and test; never written to."""
    est, cand, valid = _inputs(case)
    kw = VARIANTS[variant]
    args = (est, cand, CASES[case]["off"], valid if kw.get("valid") else None, kw.get("symmetric", False),
            kw.get("normalize", True))
    return _clip_reference(*args, torch.float64), _clip_reference(*args, torch.float32)


def _block_limit(case):
    c = CASES[case]
    return c["rows"] * c["Fd"] * c["T"] * 4         # rows = limit // (K * 4), cut to a multiple of 128 from 128 on


def _force_blocks(BF, monkeypatch, case):
    c = CASES[case]
    monkeypatch.setattr(BF, "_CLIP_BLOCK_BYTES", _block_limit(case))
    assert BF._candidate_blocks(c["Bc"], c["Fd"] * c["T"]) == c["blocks"]
    assert len(c["blocks"]) > 1


def _run(BF, case, variant, device_inputs=None):
    """ClipLossFn forward and backward on the GPU -> scores, loss, dEst, dCand (None unless the variant asks)."""
    est, cand, valid = device_inputs if device_inputs is not None else (t.cuda() for t in _inputs(case))
    kw = VARIANTS[variant]
    eg = est.clone().requires_grad_(True)
    cg = cand.clone().requires_grad_(kw.get("cand_grad", False))
    loss, scores = BF.ClipLossFn.apply(eg, cg, CASES[case]["off"], valid if kw.get("valid") else None,
                                       kw.get("symmetric", False), kw.get("normalize", True))
    (loss * SCALE).backward()
    return dict(scores=scores.detach(), loss=loss.detach(), dest=eg.grad, dcand=cg.grad)


def _hold(tag, got, case, variant):
    """scores, loss, dEst and dCand of one run against the fp64 reference (``_held``: fp32 CPU printed alongside)."""
    ref64, ref32 = _references(case, variant)
    c = CASES[case]
    scores, want, want32 = got["scores"].cpu(), ref64["scores"], ref32["scores"]
    if VARIANTS[variant].get("valid"):
        masked = list(c["masked"])
        assert bool((scores[:, masked] == -INF).all()), f"{tag}: a masked candidate keeps a score"
        kept = [o for o in range(c["Bc"]) if o not in masked]
        scores, want, want32 = scores[:, kept], want[:, kept], want32[:, kept]
    _held(f"{tag} scores", scores, want, want32, FWD_TOL)
    dl, dl32 = abs(float(got["loss"]) - float(ref64["loss"])), abs(float(ref32["loss"]) - float(ref64["loss"]))
    print(f"{tag} loss: kernel |d| {dl:.2e}   fp32 CPU |d| {dl32:.2e}   (bound 1e-05)")
    assert dl32 < 1e-5 / 4 and dl < 1e-5, (tag, float(got["loss"]), float(ref64["loss"]))
    _held(f"{tag} dEst", got["dest"], ref64["dest"], ref32["dest"], GRAD_TOL)
    if VARIANTS[variant].get("cand_grad"):
        _held(f"{tag} dCand", got["dcand"], ref64["dcand"], ref32["dcand"], GRAD_TOL)
    else:
        assert got["dcand"] is None


# ---- the cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant", RUNS)
def test_blocked_clip_loss(H, BF, monkeypatch, mode, case, variant):
    c = CASES[case]
    K = c["Fd"] * c["T"]
    real_limit = BF._CLIP_BLOCK_BYTES
    dev = tuple(t.cuda() for t in _inputs(case))
    tag = f"{case}/{variant}[{mode}]"
    _force_blocks(BF, monkeypatch, case)
    blocked = _run(BF, case, variant, dev)
    _hold(tag + " blocked", blocked, case, variant)
    # bit-identical when run again
    again = _run(BF, case, variant, dev)
    for k, v in blocked.items():
        assert (v is None and again[k] is None) or torch.equal(v, again[k]), f"{tag}: {k} differs between two runs"
    ref64, ref32 = _references(case, variant)
    if variant == "plain":
        # the no-grad entries walk the same blocks
        from brainmagick_amd.losses import ClipLoss
        _held(f"{tag} clip_scores", BF.clip_scores(dev[0], dev[1]), ref64["scores"], ref32["scores"], FWD_TOL)
        probs = ClipLoss().cuda().get_probabilities(dev[0], dev[1])
        _held(f"{tag} get_probabilities", probs, ref64["probs"], ref32["probs"], 1e-5)
    if variant == "valid":
        # a masked candidate has probability exactly 0 and takes no gradient share
        masked = list(c["masked"])
        part = BF._clip_raw_scores(dev[0], dev[1], c["B"], c["Bc"], K)
        assert tuple(part.shape) == (1, c["B"], c["Bc"])
        _, probs, dscaled, _ = H.clip_ce(part, H.clip_inv_norms(dev[1]), want_probs=True, want_grad=True, want_loss=True,
                                         target_offset=c["off"], col_valid=dev[2])
        assert float(probs[:, masked].abs().max()) == 0.0 and float(dscaled[:, masked].abs().max()) == 0.0
        _held(f"{tag} probabilities", probs, ref64["probs"], ref32["probs"], 1e-5)
    # the same inputs in one block
    monkeypatch.setattr(BF, "_CLIP_BLOCK_BYTES", real_limit)
    assert BF._candidate_blocks(c["Bc"], K) == [(0, c["Bc"])]
    whole = _run(BF, case, variant, dev)
    _hold(tag + " one block", whole, case, variant)
    kept = [o for o in range(c["Bc"]) if o not in c["masked"]] if variant == "valid" else slice(None)
    print(f"{tag} blocked against one block: scores {rel_l2(blocked['scores'][:, kept], whole['scores'][:, kept]):.2e}"
          f"   dEst {rel_l2(blocked['dest'], whole['dest']):.2e}"
          + (f"   dCand {rel_l2(blocked['dcand'], whole['dcand']):.2e}" if whole["dcand"] is not None else ""))


def test_one_launch_per_block(H, BF, monkeypatch, mode):
    """Case A with learnable candidates under the kernel timer: the forward is three score contractions through
    ``gemm_nt`` (not the single ``gemm_nt_partials`` launch), the backward three ``conv_nn`` per requested gradient."""
    case = "A"
    nblocks = len(CASES[case]["blocks"])
    est, cand, _ = (t.cuda() for t in _inputs(case))
    eg, cg = est.requires_grad_(True), cand.requires_grad_(True)
    _force_blocks(BF, monkeypatch, case)

    def labels(fn):
        timer = H.KernelTimer()
        H.set_kernel_timer(timer)
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            H.set_kernel_timer(None)
        return out, [name for name, *_ in timer.records]
    (loss, _), fwd = labels(lambda: BF.ClipLossFn.apply(eg, cg, CASES[case]["off"]))
    assert len([n for n in fwd if n.startswith("gemm_nt")]) == nblocks, fwd
    assert not [n for n in fwd if n.startswith("clip_scores:")], fwd
    if mode == "f16x2":
        # two kernel families in one call: the full blocks in the wide kernels, the 44 rows in 3 x bf16
        assert [n.split("<")[0] for n in fwd] == ["gemm_nt_h2w_kernel", "gemm_nt_h2w_kernel", "gemm_nt_x3_kernel"], fwd
    _, bwd = labels(lambda: (loss * SCALE).backward())
    assert len([n for n in bwd if n.startswith("conv_nn")]) == 2 * nblocks, bwd
    # dEst alone
    eg.grad = None
    loss, _ = BF.ClipLossFn.apply(eg, cg.detach(), CASES[case]["off"])
    _, bwd = labels(lambda: loss.backward())
    assert len([n for n in bwd if n.startswith("conv_nn")]) == nblocks, bwd


@pytest.mark.parametrize("case", ["A", "B", "D"])
@pytest.mark.parametrize("arena_mode", ["f16x2", "f32"])
def test_blocked_windows_stay_inside_their_buffers(H, BF, monkeypatch, case, arena_mode):
    """Forward and backward inside the guard-band arena: ``raw`` [1, B, Bc] and ``dcand`` [Bc, K] are ``torch.empty``
    allocations, served NaN-poisoned between canaries -- a column or row that no block wrote shows up as a NaN, a
    window that runs over as a broken canary."""
    variant = "valid" if CASES[case]["masked"] else "cand"
    est, cand, valid = (t.cuda() for t in _inputs(case))
    H.set_compute_dtype(arena_mode)
    try:
        _force_blocks(BF, monkeypatch, case)
        arena = Arena()
        with arena.active():
            eg, cg = est.requires_grad_(True), cand.requires_grad_(True)
            loss, scores = BF.ClipLossFn.apply(eg, cg, CASES[case]["off"], valid if variant == "valid" else None)
            (loss * SCALE).backward()
        arena.check(f"blocked ClipLoss {case}[{arena_mode}]")
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
    for t, name in ((scores, "scores"), (loss, "loss"), (eg.grad, "dEst"), (cg.grad, "dCand")):
        assert t is not None and not bool(torch.isnan(t).any()), f"{name}: NaN (an element no block wrote)"
    ref64, _ = _references(case, "valid" if variant == "valid" else "cand")
    assert rel_l2(eg.grad, ref64["dest"]) < GRAD_TOL
    if variant == "cand":
        assert rel_l2(cg.grad, ref64["dcand"]) < GRAD_TOL


@pytest.mark.parametrize("case", ["A", "E"])
def test_backward_publishes_the_maximum_of_the_finished_sum(H, BF, monkeypatch, case):
    """f16x2: every ``conv_nn`` of the dEst loop drops the maximum published for ``dest`` and publishes that of the sum
    so far.  What the tensor handed back to autograd carries is what the model's last conv backward scales dEst by: it
    has to be the maximum of the FINISHED sum (one left over from the first block passes every numeric check above and
    overflows f16 one layer down), found without a stand-alone pass."""
    est, cand, _ = (t.cuda() for t in _inputs(case))
    H.set_compute_dtype("f16x2")
    try:
        _force_blocks(BF, monkeypatch, case)
        eg = est.requires_grad_(True)
        seen = []
        eg.register_hook(lambda grad: seen.append(grad))         # the tensor ClipLossFn.backward returned
        loss, _ = BF.ClipLossFn.apply(eg, cand, CASES[case]["off"])
        before = H.amax_scans
        (loss * SCALE).backward()
        dest, = seen
        slot = H.amax(dest)
        assert H.amax_scans == before, "dEst (or a candidate block) needed a stand-alone amax pass"
        assert float(slot.max()) == float(dest.abs().max())
    finally:
        H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
    assert rel_l2(dest, _references(case, "plain")[0]["dest"]) < GRAD_TOL


def test_node_wide_column_term_walks_the_gathered_estimates_in_blocks(H, BF, monkeypatch, mode):
    """``ClipLoss(symmetric=True)`` with ``estimate_all`` at world 2, rank 1, B = 130: the column term's "candidates" are
    the 260 gathered estimates (``normalize=False``, gradient into them), here in blocks of 128, 128 and 4 rows -- like
    the row term's candidates."""
    from brainmagick_amd.losses import ClipLoss
    world, rank, B, Fd, T = 2, 1, 130, 24, 77
    g = torch.Generator().manual_seed(21)
    cand = torch.randn(world * B, Fd, T, generator=g) * 1.5 + 0.2
    parts = [torch.randn(B, Fd, T, generator=g) * 0.5 + 0.02 * cand[r * B:(r + 1) * B] for r in range(world)]
    refs = []
    for dtype in (torch.float64, torch.float32):
        leaves = [p.to(dtype, copy=True).requires_grad_(True) for p in parts]
        ref = O.clip_loss_symmetric_node(torch.cat(leaves), cand.to(dtype), rank, B)
        (ref * SCALE).backward()
        refs.append((ref.detach(), [leaf.grad for leaf in leaves]))
    (ref64, grads64), (ref32, grads32) = refs
    monkeypatch.setattr(BF, "_CLIP_BLOCK_BYTES", 128 * Fd * T * 4)
    assert BF._candidate_blocks(world * B, Fd * T) == [(0, 128), (128, 128), (256, 4)]
    dev = [p.cuda().requires_grad_(True) for p in parts]
    mask = torch.ones(B, 1, T, dtype=torch.bool, device="cuda")
    loss = ClipLoss(symmetric=True).cuda()(dev[rank], cand.cuda(), mask, target_offset=rank * B,
                                           estimate_all=torch.cat(dev))
    (loss * SCALE).backward()
    dl, dl32 = abs(float(loss) - float(ref64)), abs(float(ref32) - float(ref64))
    print(f"node-wide[{mode}] loss: kernel |d| {dl:.2e}   fp32 CPU |d| {dl32:.2e}")
    assert dl32 < 1e-5 / 4 and dl < 1e-5, (float(loss), float(ref64))
    for r in range(world):
        _held(f"node-wide[{mode}] dEst of rank {r}", dev[r].grad, grads64[r], grads32[r], GRAD_TOL)


# ---- at the real limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_mode", ["f16x2", "f32x3"])
def test_the_smallest_set_that_crosses_the_real_limit(H, BF, big_mode):
    """Nothing patched: 768 candidates of K = 1024 x 360 (1.13 GB) are the blocks [(0, 640), (640, 128)]; the 943 MB
    window of the first is just under ``bm_conv_h2_covers``' 1 GiB bound and near the end of the 32-bit offsets the
    blocks exist for -- in f16x2 mode both blocks have to run in the wide kernels, forward and backward (pinned: a
    silent fall-back to 3 x bf16 would leave the numbers right and those offsets untested).  Scores, loss terms and
    dEst of 16 sampled estimate rows against all candidates, fp64 on the GPU in chunks of 128 candidate rows; the
    targets (576 .. 703) span both blocks."""
    B, Bc, K, off = 128, 768, 1024 * 360, 576
    blocks = [(0, 640), (640, 128)]
    assert BF._CLIP_BLOCK_BYTES == 0x3f000000
    assert BF._candidate_blocks(Bc, K) == blocks
    for _, n in blocks:
        assert H.lib().bm_gemm_nt_h2_covers(B, n, 1, 1, K, 1, 1, 0) and H.lib().bm_conv_h2_covers(n, B, K, 1, 1)
    cand = est = loss = scores = e64 = c2 = c64 = s64 = d64 = dest64 = sk = None       # released below whatever happens
    try:
        t0 = time.perf_counter()
        g = torch.Generator(device="cuda").manual_seed(31)
        cand = torch.randn(Bc, 1024, 360, device="cuda", generator=g)
        cand.mul_(1.5).add_(0.2)
        est = torch.randn(B, 1024, 360, device="cuda", generator=g)
        est.mul_(0.5).add_(cand[off:off + B], alpha=0.004)         # planted: target scores ~4 above the rest
        est.requires_grad_(True)
        timer = H.KernelTimer()
        H.set_compute_dtype(big_mode)
        H.set_kernel_timer(timer)
        try:
            loss, scores = BF.ClipLossFn.apply(est, cand, off)
            (loss * SCALE).backward()
            torch.cuda.synchronize()
        finally:
            H.set_kernel_timer(None)
            H.set_compute_dtype(H.DEFAULT_COMPUTE_DTYPE)
        t1 = time.perf_counter()
        family = "h2w" if big_mode == "f16x2" else "x3"
        labels = [name.split("<")[0] for name, *_ in timer.records]
        assert labels == [f"gemm_nt_{family}_kernel"] * 2 + [f"conv_nn_{family}_kernel"] * 2, labels
        rows = torch.arange(3, B, 8, device="cuda")                 # 16 rows
        e64 = est.detach()[rows].double().view(len(rows), K)
        c2 = cand.view(Bc, K)
        s64 = torch.empty(len(rows), Bc, device="cuda", dtype=torch.float64)
        inv64 = torch.empty(Bc, device="cuda", dtype=torch.float64)
        for c0 in range(0, Bc, 128):
            c64 = c2[c0:c0 + 128].double()
            inv64[c0:c0 + 128] = 1 / (1e-8 + c64.norm(dim=1))
            s64[:, c0:c0 + 128] = e64 @ c64.t() * inv64[c0:c0 + 128]
        onehot = F.one_hot(rows + off, Bc).double()
        d64 = (torch.softmax(s64, 1) - onehot) / B * inv64 * SCALE
        dest64 = torch.zeros(len(rows), K, device="cuda", dtype=torch.float64)
        for c0 in range(0, Bc, 128):
            c64 = c2[c0:c0 + 128].double()
            dest64 += d64[:, c0:c0 + 128] @ c64
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        e_s = rel_l2(scores[rows], s64)
        e_d = rel_l2(est.grad.view(B, K)[rows], dest64)
        # loss terms: the sampled rows' cross entropies out of the kernel's scores against the reference's, and the
        # kernel's mean against the mean over its own scores
        terms64 = torch.logsumexp(s64, 1) - s64.gather(1, (rows + off)[:, None])[:, 0]
        sk = scores.double()
        terms = torch.logsumexp(sk, 1) - sk.gather(1, (torch.arange(B, device="cuda") + off)[:, None])[:, 0]
        e_t = float((terms[rows] - terms64).abs().max())
        e_l = abs(float(loss) - float(terms.mean()))
        mean_term = float(terms64.mean())
        print(f"real limit[{big_mode}]: scores {e_s:.2e} (tolerance {FWD_TOL:.0e})   dEst {e_d:.2e} (tolerance "
              f"{GRAD_TOL:.0e})   loss terms |d| {e_t:.2e}   loss |d| {e_l:.2e}   "
              f"inputs + forward + backward {t1 - t0:.2f} s, reference {t2 - t1:.2f} s")
    finally:
        if est is not None:
            est.grad = None
        cand = est = loss = scores = e64 = c2 = c64 = s64 = d64 = dest64 = sk = None
        torch.cuda.empty_cache()
    assert 0.5 < mean_term < 6.0                                    # far from saturation
    assert e_s < FWD_TOL and e_d < GRAD_TOL
    assert e_t < 1e-5 and e_l < 1e-5
