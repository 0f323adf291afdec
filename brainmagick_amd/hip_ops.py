"""Typed Python wrappers over the libbmhip C-ABI (one wrapper per entry point group).

PyTorch is used here only as the owner of device memory and of the HIP stream: every function
checks that its tensors are fp32 / contiguous / on the GPU, allocates outputs with ``torch.empty``
and enqueues the HIP kernels on the current stream.  CPU tensors are rejected -- there is no
fallback path.
"""
import ctypes
import math
import typing as tp

import numpy as np
import torch

from ._lib import lib, check, BmHipError

ACT_NONE, ACT_GELU, ACT_RELU, ACT_LEAKY = 0, 1, 2, 3
BKC = 16

# Compute mode of the MFMA contractions.  Activations / parameters / gradients stay fp32 in HBM.
#   "f16x2" (default) fp32-ACCURATE contraction on the f16 matrix cores: every operand is scaled by a power of two (per
#           tensor for activations, per output row for weights) and split into TWO f16 planes, three partial
#           products per block, fp32 accumulate, exact inverse scaling; half the matrix-core work of "f32x3",
#           same parity tolerances (norm-wise error bound, see csrc/conv_nn_h2w.hip).  Shapes the wide f16x2
#           kernels do not cover run on the "f32x3" kernels;
#   "f32x3" fp32-ACCURATE contraction on the bf16 matrix cores: both fp32 operands are split
#           EXACTLY into three bf16 planes, six partial products per block, fp32 accumulate; measured
#           error vs fp64 <= the exact-fp32 MFMA path's, held to the same parity tolerances;
#   "f32"   exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), bit-identical to an fp32 FMA chain.
# (Round 4 removed the opt-in reduced-precision "bf16" mode and the wide-tile f32x3 kernels: every mode left is
# fp32-class and held to the same tolerances.)
import os as _os
DEFAULT_COMPUTE_DTYPE = "f16x2"
COMPUTE_DTYPES = ("f32", "f32x3", "f16x2")
_compute_dtype = _os.environ.get("BM_COMPUTE_DTYPE", DEFAULT_COMPUTE_DTYPE)
if _compute_dtype not in COMPUTE_DTYPES:
    raise ValueError(f"BM_COMPUTE_DTYPE must be one of {COMPUTE_DTYPES}, got {_compute_dtype!r}")


def set_compute_dtype(name: str):
    global _compute_dtype
    if name not in COMPUTE_DTYPES:
        raise ValueError(f"compute dtype must be one of {COMPUTE_DTYPES}, got {name!r}")
    _compute_dtype = name


def get_compute_dtype() -> str:
    return _compute_dtype


class KernelTimer:
    """Optional HIP-event timing of the MFMA kernels, on the stream they are launched on (the
    current torch stream).  ``bench.py`` installs one to measure the dominant kernel's average
    launch duration live inside the timed region; cost = two event records per launch."""

    def __init__(self):
        self.records: tp.List[tp.Tuple[str, float, torch.cuda.Event, torch.cuda.Event]] = []

    def launch(self, name: str, flops: float, fn):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        end.record()
        self.records.append((name, flops, start, end))
        return out

    def summary(self) -> tp.Dict[str, tp.Dict[str, float]]:
        """name -> {launches, avg_ms, median_ms, max_ms, outliers, flops_per_launch}; call after a device
        synchronize.  ``avg_ms`` is the mean over the launches whose duration is within 20x the label's median: an
        event pair also measures whatever keeps the queue from reaching the kernel (a host stall between the two
        records shows up as a launch of many milliseconds); the dropped samples are counted in ``outliers``."""
        samples: tp.Dict[str, tp.List[float]] = {}
        flops_sum: tp.Dict[str, float] = {}
        for name, flops, start, end in self.records:
            samples.setdefault(name, []).append(start.elapsed_time(end))
            flops_sum[name] = flops_sum.get(name, 0.0) + flops
        out = {}
        for name, v in samples.items():
            med = sorted(v)[len(v) // 2]
            kept = [t for t in v if t <= 20.0 * med]
            out[name] = dict(launches=len(v), avg_ms=sum(kept) / len(kept), median_ms=med, max_ms=max(v),
                             outliers=len(v) - len(kept), flops_per_launch=flops_sum[name] / len(v))
        return out


_timer: tp.Optional[KernelTimer] = None
_MODE_SUFFIX = {"f32": "", "f32x3": "_x3", "f16x2": "_h2w"}      # compute mode -> kernel family in the timer's labels


def set_kernel_timer(timer: tp.Optional[KernelTimer]):
    global _timer
    _timer = timer


def _timed(label, flops: float, launch):
    """Run ``launch()``, under the installed KernelTimer if there is one.  ``label`` is a string or -- so that nothing
    is formatted when no timer listens -- a function that returns it."""
    if _timer is None:
        return launch()
    return _timer.launch(label() if callable(label) else label, flops, launch)


def _p(t: tp.Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, name: str, dtype=torch.float32, contiguous: bool = True):
    """``contiguous=False``: the caller reads a strided view in place, or makes its own copy."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise BmHipError(f"{name}: expected a GPU tensor; the brainmagick_amd hot path has no CPU "
                         "fallback (got %s)" % (t.device if isinstance(t, torch.Tensor) else type(t)))
    if t.dtype != dtype:
        raise BmHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise BmHipError(f"{name}: expected a contiguous tensor")
    return t


def _opt(t, name, dtype=torch.float32):
    return None if t is None else _req(t, name, dtype)


# Scratch that the kernels of one stream share (they run in order): one buffer per (kind, device, stream).
# kind -> (size function of the library, dtype, zeroed).  A ZEROED buffer holds ticket counters next to its partials
# (csrc/bm_block.h): every launch leaves its counter at zero again.
_WS_KINDS = {
    "amax": ("bm_amax_ws_elems", torch.float32, False),                 # per-workgroup partial maxima of the producers
    "regress": ("bm_regress_workspace_bytes", torch.uint8, True),      # csrc/regress.hip
    "encode": ("bm_meg_init_workspace_bytes", torch.uint8, True),      # csrc/encode.hip
    "lowpass": ("bm_lowpass_workspace_bytes", torch.uint8, True),      # csrc/lowpass.hip
}
_stream_workspaces: tp.Dict[tp.Any, torch.Tensor] = {}


def _stream_ws(kind: str, device) -> torch.Tensor:
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream)
    ws = _stream_workspaces.get(key)
    if ws is None:
        size, dtype, zeroed = _WS_KINDS[kind]
        alloc = torch.zeros if zeroed else torch.empty
        ws = _stream_workspaces[key] = alloc(getattr(lib(), size)(), device=device, dtype=dtype)
    return ws


# ------------------------------------------------------------------------------------------------
def conv_mpad(M: int) -> int:
    return lib().bm_conv_mpad(M)


# A value that a kernel derived from a tensor's contents (its maximum, per-channel maxima, inverse row norms) is
# remembered ON the tensor as (version, data_ptr, value[, checked]); it holds for exactly those contents.  A leaf that
# requires grad is a parameter, which the library's own writers change through raw pointers (FlatAdam.step, the
# data-parallel gathers: ``weights_changed()``): its notes hold for the weights epoch they were taken in (``_bm_epoch``).
def _note(t: torch.Tensor, attr: str, value, *checked):
    try:
        setattr(t, attr, (t._version, t.data_ptr(), value) + checked)
        t._bm_epoch = _weights_epoch
    except Exception:       # tensors that refuse attributes or have no version counter (inference mode): do not cache
        pass


def _noted(t: torch.Tensor, attr: str, need_checked: bool = False):
    """The value noted on ``t`` if it still describes it, else None.  ``need_checked``: only a note taken together
    with the non-finite check will do."""
    note = getattr(t, attr, None)
    if note is not None and note[0] == t._version and note[1] == t.data_ptr() and (not need_checked or note[3]) and \
            (not (t.requires_grad and t.is_leaf) or getattr(t, "_bm_epoch", None) == _weights_epoch):
        return note[2]
    return None


AMAX_SHARDS = 8       # an amax slot is 8 floats (csrc/bm_common.h; the finalize kernels write all eight); max|x| = slot.max()
amax_scans = 0        # number of stand-alone amax passes launched (producers that publish their own maximum need none)


def amax(x: torch.Tensor, nonfinite_flag: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
    """[AMAX_SHARDS] fp32 tensor whose maximum is max |x| (device side, no sync).  Cached on the tensor object together with
    its version counter, so a tensor consumed by several contractions (forward conv, weight gradient) is
    scanned once and an in-place modification invalidates the cache.  ``nonfinite_flag`` (int32 device tensor):
    element 0 is set to 1 by the same pass if x holds an inf / nan (a cached tensor was checked when it was scanned)."""
    cached = _noted(x, "_bm_amax", nonfinite_flag is not None)
    if cached is not None:
        return cached
    _req(x, "amax.x")
    global amax_scans
    amax_scans += 1
    out = torch.empty(AMAX_SHARDS, device=x.device, dtype=torch.float32)
    check(lib().bm_amax_checked(_p(x), x.numel(), _p(out), _p(_stream_ws("amax", x.device)),
                                _p(_opt(nonfinite_flag, "nonfinite_flag", torch.int32)), _stream()), "bm_amax")
    _note(x, "_bm_amax", out, nonfinite_flag is not None)
    return out


_amax_pool: tp.Dict[torch.device, tp.List[tp.Any]] = {}


def _amax_slot(t: torch.Tensor) -> tp.Optional[torch.Tensor]:
    """An [AMAX_SHARDS] fp32 slot for a producer kernel to publish max|t| into (f16x2 mode only; None otherwise).
    Slots are carved out of pooled buffers, each slot is used once.  The slot is attached to the tensor like
    `amax()` would, so the consuming contraction finds it without a pass over the tensor."""
    if _compute_dtype != "f16x2" or t.numel() == 0:      # empty: the producer returns before it writes
        return None
    pool = _amax_pool.get(t.device)
    if pool is None or pool[1] >= pool[0].numel():
        # one zero fill per 4 096 slots (a slot nobody finalized reads as max|x| = 0)
        pool = _amax_pool[t.device] = [torch.zeros(4096 * AMAX_SHARDS, device=t.device, dtype=torch.float32), 0]
    slot = pool[0][pool[1]:pool[1] + AMAX_SHARDS]
    pool[1] += AMAX_SHARDS
    _note(t, "_bm_amax", slot, False)
    return slot


def _row_amax_out(t: torch.Tensor, slot) -> tp.Optional[torch.Tensor]:
    """[channels] fp32 buffer for a producer with a (channel, split) grid to publish max|t| PER CHANNEL into (next to the
    tensor slot).  A gradient channel is a row of the weight gradient: the f16x2 weight-gradient
    kernel then scales A row by row (csrc/gemm_nt_h2w.hip, RS kernels), so a channel far below its tensor's maximum keeps
    its 22 bits.  Attached to the tensor like the slot."""
    if slot is None:
        return None
    rows = torch.empty(t.shape[1], device=t.device, dtype=torch.float32)
    _note(t, "_bm_row_amax", rows)
    return rows


def row_amax_of(t: torch.Tensor) -> tp.Optional[torch.Tensor]:
    return _noted(t, "_bm_row_amax")


def _slot_args(slot):
    """(amax_out, amax_ws) arguments of a producer."""
    return (_p(slot), _p(_stream_ws("amax", slot.device)) if slot is not None else None)


def _touched(t: torch.Tensor) -> torch.Tensor:
    """Called by every wrapper that lets a library kernel write INTO an existing tensor through its raw pointer:
    torch's version counter does not see such writes, so a maximum published for the old contents must go."""
    for attr in ("_bm_amax", "_bm_row_amax", "_bm_inv_norms"):
        if getattr(t, attr, None) is not None:
            try:
                delattr(t, attr)
            except AttributeError:
                pass
    return t


def share_amax(src: torch.Tensor, view: torch.Tensor) -> torch.Tensor:
    """``view`` is a slice of ``src``: the maximum of the whole tensor bounds the slice (any upper bound within the
    f16 headroom serves as the scale), so the slice needs no pass of its own."""
    if _compute_dtype != "f16x2":     # nobody consumes a maximum in the other compute modes: no scan
        return view
    _note(view, "_bm_amax", amax(src), False)
    return view


# ------------------------------------------------------------------------------------------------
# Packed parameters.  A model's weights change once per optimizer step, so in "f16x2" mode the packed form of
# every PARAMETER (leaf tensor that requires grad) that the convs ask for lives in a persistent buffer, and all
# of them are refreshed together by one launch (bm_pack_weights_h2_batch) the first time one is asked for after
# the parameters changed -- instead of one small launch per conv, forward and backward.  "Changed" = the
# library's own writers said so (weights_changed(): FlatAdam.step, the data-parallel gathers) or the tensor's
# autograd version moved (load_state_dict, in-place edits); evaluation never re-packs.
_weights_epoch = 0
pack_launches = 0            # launches of either packing kernel (tests / bench bookkeeping)


def weights_changed():
    """Called by every library routine that writes parameters through raw pointers."""
    global _weights_epoch
    _weights_epoch += 1


class _PackPlan:
    MAX_JOBS = 512           # e.g. many models in one test session: start over rather than grow without bound
    KEEP = 3                 # parameter updates an entry survives without being asked for (a model that went away)

    def __init__(self, device):
        self.device = device
        self.entries: tp.Dict[tuple, dict] = {}
        self.table: tp.Optional[torch.Tensor] = None
        self.total_blocks = 0

    def get(self, src: torch.Tensor, geom: tuple) -> torch.Tensor:
        key = (src.data_ptr(),) + geom
        e = self.entries.get(key)
        if e is None:
            if len(self.entries) >= self.MAX_JOBS:
                self.entries.clear()
            G, M, Cin, KS = geom[:4]
            dst = torch.empty(lib().bm_packed_weight_bytes_h2(G, M, Cin, KS), device=src.device, dtype=torch.uint8)
            dst._bm_mode = "f16x2"
            dst._bm_groups = G
            # `src` is kept alive: the batched launch reads it through its raw pointer
            e = self.entries[key] = dict(src=src, ptr=src.data_ptr(), geom=geom, dst=dst, stamp=None)
            self.table = None
        e["used"] = _weights_epoch
        if e["stamp"] != (_weights_epoch, src._version):
            self.refresh()
        return e["dst"]

    def refresh(self):
        global pack_launches
        # parameters nobody asked for lately (another model of the process, a re-seated `.data`) leave the plan
        stale = [k for k, e in self.entries.items()
                 if e["used"] < _weights_epoch - self.KEEP or e["src"].data_ptr() != e["ptr"]]
        for k in stale:
            del self.entries[k]
        if stale:
            self.table = None
        ents = list(self.entries.values())
        if not ents:
            return
        if self.table is None:
            nb = lib().bm_pack_h2_job_bytes()
            host = ctypes.create_string_buffer(nb * len(ents))
            block0 = 0
            for i, e in enumerate(ents):
                n = lib().bm_pack_h2_job_fill(ctypes.c_void_p(ctypes.addressof(host) + i * nb), _p(e["src"]),
                                              _p(e["dst"]), *e["geom"], None, block0)
                if n < 0:
                    raise BmHipError("bm_pack_h2_job_fill: bad arguments %r" % (e["geom"],))
                block0 += n
            self.table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.device)
            self.total_blocks = block0
        max_nk = max(e["geom"][2] * e["geom"][3] for e in ents)          # Cin * KS
        check(lib().bm_pack_weights_h2_batch(_p(self.table), len(ents), self.total_blocks, max_nk, _stream()),
              "bm_pack_weights_h2_batch")
        pack_launches += 1
        for e in ents:
            e["stamp"] = (_weights_epoch, e["src"]._version)


_pack_plans: tp.Dict[tp.Tuple[str, int], _PackPlan] = {}


def _pack_plan(device) -> _PackPlan:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _pack_plans:
        _pack_plans[key] = _PackPlan(torch.device(*key))
    return _pack_plans[key]


def pack_weights(src: torch.Tensor, G: int, M: int, Cin: int, KS: int, sg: int, sm: int, sc: int,
                 sj: int, flip: bool = False, alpha: tp.Optional[torch.Tensor] = None,
                 shape: tp.Optional[tp.Tuple[int, int]] = None) -> torch.Tensor:
    """``shape`` = (T, dilation) of the conv that will consume the packed weights: in "f16x2" mode it decides
    between the wide f16x2 kernel's layout and the 3 x bf16 layout of the narrow kernels."""
    _req(src, "pack_weights.src")
    mode = _compute_dtype
    if mode == "f16x2":
        if shape is not None and lib().bm_conv_h2_covers(Cin, M, shape[0], KS, shape[1]):
            if alpha is None and src.requires_grad and src.is_leaf:
                return _pack_plan(src.device).get(src, (G, M, Cin, KS, sg, sm, sc, sj, int(flip)))
            nbytes = lib().bm_packed_weight_bytes_h2(G, M, Cin, KS)
            dst = torch.empty(nbytes, device=src.device, dtype=torch.uint8)
            check(lib().bm_pack_weights_h2(_p(src), _p(dst), G, M, Cin, KS, sg, sm, sc, sj, int(flip),
                                           _p(_opt(alpha, "alpha")), _stream()), "bm_pack_weights_h2")
            global pack_launches
            pack_launches += 1
            dst._bm_mode = "f16x2"
            dst._bm_groups = G
            return dst
        mode = "f32x3"
    if mode == "f32x3":
        n = lib().bm_packed_weight_elems_x3(G, M, Cin, KS)
        dst = torch.empty(n, device=src.device, dtype=torch.bfloat16)
        check(lib().bm_pack_weights_x3(_p(src), _p(dst), G, M, Cin, KS, sg, sm, sc, sj, int(flip),
                                       _p(_opt(alpha, "alpha")), _stream()), "bm_pack_weights_x3")
        dst._bm_mode = mode                      # tells conv_nn which kernel family packed it
        return dst
    return pack_weights_f32(src, M, Cin, KS, sm, sc, sj, G, sg, flip, alpha)


def pack_weights_f32(src: torch.Tensor, M: int, Cin: int, KS: int, sm: int, sc: int, sj: int, G: int = 1, sg: int = 0,
                     flip: bool = False, alpha: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp32 packed layout [group][chunk][tap][16][Mpad] whatever the compute mode (rows m = src[g*sg + m*sm + c*sc +
    j*sj]): what the exact-fp32 kernels read -- every conv in "f32" mode, the strided family in all modes."""
    _req(src, "pack_weights_f32.src")
    dst = torch.empty(lib().bm_packed_weight_elems(G, M, Cin, KS), device=src.device, dtype=torch.float32)
    check(lib().bm_pack_weights(_p(src), _p(dst), G, M, Cin, KS, sg, sm, sc, sj, int(flip), _p(_opt(alpha, "alpha")),
                                _stream()), "bm_pack_weights")
    return dst


def pack_conv_fwd(weight: torch.Tensor, shape=None) -> torch.Tensor:
    """nn.Conv1d weight [M, Cin, KS] for the forward conv."""
    M, Cin, KS = weight.shape
    return pack_weights(weight, 1, M, Cin, KS, 0, Cin * KS, KS, 1, shape=shape)


def pack_conv_dgrad(weight: torch.Tensor, shape=None) -> torch.Tensor:
    """nn.Conv1d weight [M, Cin, KS] for the data gradient: roles of M/Cin swapped, taps flipped."""
    M, Cin, KS = weight.shape
    return pack_weights(weight, 1, Cin, M, KS, 0, KS, Cin * KS, 1, flip=True, shape=shape)


def _conv_outputs(x: torch.Tensor, M: int, T: int, want_pre: bool, want_out: bool, stats_shape=None):
    """(y_pre | None, y_out | None, stats | None) of a conv on x [B, Cin, .]: fp32 [B, M, T] outputs and, with a
    ``stats_shape``, its BatchNorm partials."""
    def new(shape, want=True):
        return torch.empty(shape, device=x.device, dtype=torch.float32) if want and shape is not None else None
    return new((x.shape[0], M, T), want_pre), new((x.shape[0], M, T), want_out), new(stats_shape)


def conv_nn(x: torch.Tensor, wpacked: torch.Tensor, M: int, KS: int = 1, dil: int = 1,
            widx: tp.Optional[torch.Tensor] = None, bias=None, scale=None, shift=None, res=None,
            act: int = ACT_NONE, leak: float = 0., want_pre: bool = False, want_out: bool = True,
            want_stats: bool = False, out: tp.Optional[torch.Tensor] = None, bias_gstride: int = 0,
            publish_amax: bool = True):
    """Returns (y_pre | None, y_out | None, stats | None); x is [B, Cin, T].  ``out``: write y_out there instead of
    allocating (it may be ``res`` itself: every element is read and written by the same thread, which is how the
    ClipLoss backward accumulates over candidate blocks).  ``bias_gstride`` > 0: ``bias`` holds one vector per weight
    group, ``bias_gstride`` floats apart, selected by ``widx`` like the weights.  ``publish_amax=False``: the output
    goes to an elementwise kernel (the data gradients of the conv stack), nobody needs its maximum."""
    _req(x, "conv_nn.x")
    mode = getattr(wpacked, "_bm_mode", "f32")      # set by pack_weights
    _req(wpacked, "conv_nn.w", {"f32": torch.float32, "f16x2": torch.uint8}.get(mode, torch.bfloat16))
    B, Cin, T = x.shape
    channel_major = want_stats and mode == "f16x2"     # a channel's partials are one contiguous run for bn_finalize
    stats_shape = None if not want_stats else (M, lib().bm_conv_h2_stats_tiles(B, T), 2) if channel_major else \
        (lib().bm_conv_stats_tiles(B, T), M, 2)
    y_pre, y_out, stats = _conv_outputs(x, M, T, want_pre, want_out and out is None, stats_shape)
    if channel_major:
        stats._bm_channel_major = True
    if out is not None:
        _req(out, "conv_nn.out")
        assert want_out and out.numel() == B * M * T, (out.shape, (B, M, T))
        y_out = _touched(out)
    if res is not None:
        _req(res, "conv_nn.res")
        assert res.shape == (B, M, T), (res.shape, (B, M, T))
    common = (_p(_opt(widx, "widx", torch.int32)), _p(_opt(bias, "bias")), bias_gstride, _p(_opt(scale, "scale")),
              _p(_opt(shift, "shift")), _p(res), M * T, _p(y_pre), _p(y_out), M * T, _p(stats), B, Cin, M, T,
              KS, dil, act, leak)
    if mode == "f16x2":
        x_amax = amax(x)
        y_slot = _amax_slot(y_out) if (y_out is not None and publish_amax) else None

        def launch():
            check(lib().bm_conv1d_nn_h2(_p(x), Cin * T, _p(x_amax), _p(wpacked), *common, wpacked._bm_groups,
                                        *_slot_args(y_slot), _stream()), "bm_conv1d_nn_h2")
    else:
        fn = {"f32": lib().bm_conv1d_nn, "f32x3": lib().bm_conv1d_nn_x3}[mode]

        def launch():
            check(fn(_p(x), Cin * T, _p(wpacked), *common, _stream()), f"bm_conv1d_nn[{mode}]")

    def label():
        if mode == "f16x2":
            tile = f"{KS},{lib().bm_conv_h2_mw_for(M)}"
        else:
            tile = (lib().bm_conv_mt_for if mode == "f32" else lib().bm_conv_x3_mt_for)(M)
        return f"conv_nn{_MODE_SUFFIX[mode]}_kernel<{tile}>"
    _timed(label, 2.0 * B * T * M * Cin * KS, launch)
    return y_pre, y_out, stats


# ------------------------------------------------------------------------------------------------
# Strided / transposed convs (csrc/conv_strided.hip): nn.Conv1d with stride, nn.ConvTranspose1d, their data and weight
# gradients.  One kernel family, exact-fp32 MFMA, for all three compute modes (an f16x2 variant is a follow-up; the
# timer labels below tell which family ran).
def conv_out_len(T: int, KS: int, stride: int, dil: int, pad: int, transposed: bool) -> int:
    """Output length of nn.Conv1d / nn.ConvTranspose1d (output_padding 0); raises like torch when there is none."""
    Tout = lib().bm_conv1d_out_len(T, KS, stride, dil, pad, int(transposed))
    if Tout < 1:
        if transposed:
            raise RuntimeError(f"ConvTranspose1d: input of {T} samples (kernel {KS}, stride {stride}, dilation {dil}, "
                               f"padding {pad}) gives an output of {Tout} samples. Output size is too small")
        raise RuntimeError(f"Calculated padded input size per channel: ({T + 2 * pad}). Kernel size: "
                           f"({dil * (KS - 1) + 1}). Kernel size can't be greater than actual input size")
    return Tout


def pack_strided_rows_first(weight: torch.Tensor) -> torch.Tensor:
    """[rows, reduced, KS] (nn.Conv1d's [M, Cin, KS] forward; nn.ConvTranspose1d's [Cin, M, KS] data gradient)."""
    R, C, KS = weight.shape
    return pack_weights_f32(weight, R, C, KS, C * KS, KS, 1)


def pack_strided_rows_second(weight: torch.Tensor) -> torch.Tensor:
    """[reduced, rows, KS] (nn.ConvTranspose1d's [Cin, M, KS] forward; nn.Conv1d's [M, Cin, KS] data gradient)."""
    C, R, KS = weight.shape
    return pack_weights_f32(weight, R, C, KS, KS, R * KS, 1)


def conv_strided(x: torch.Tensor, wpacked: torch.Tensor, M: int, Tout: int, KS: int, stride: int, dil: int, pad: int,
                 transposed: bool, bias=None, scale=None, shift=None, act: int = ACT_NONE, leak: float = 0.,
                 want_pre: bool = False, want_out: bool = True, want_stats: bool = False):
    """Gather form (``transposed=False``: strided nn.Conv1d) or scatter form (nn.ConvTranspose1d) of
    csrc/conv_strided.hip on x [B, Cin, T] -> [B, M, Tout]; returns (y_pre | None, y_out | None, stats | None) like
    ``conv_nn``.  ``Tout`` is the caller's (``conv_out_len`` forward, the layer's input length as a data gradient)."""
    _req(x, "conv_strided.x")
    _req(wpacked, "conv_strided.w")
    B, Cin, T = x.shape
    if Tout < 1:
        raise RuntimeError(f"conv_strided: output length {Tout} < 1")
    y_pre, y_out, stats = _conv_outputs(
        x, M, Tout, want_pre, want_out,
        (lib().bm_conv_strided_stats_tiles(B, Tout, stride, int(transposed)), M, 2) if want_stats else None)
    fn = lib().bm_conv1d_transposed if transposed else lib().bm_conv1d_strided
    name = "conv_transposed_kernel" if transposed else "conv_strided_kernel"

    def launch():
        check(fn(_p(x), Cin * T, _p(wpacked), _p(_opt(bias, "bias")), _p(_opt(scale, "scale")), _p(_opt(shift, "shift")),
                 _p(y_pre), _p(y_out), M * Tout, _p(stats), B, Cin, M, T, Tout, KS, stride, dil, pad, act, leak,
                 _stream()), "bm_conv1d_transposed" if transposed else "bm_conv1d_strided")
    taps = KS if not transposed else -(-KS // stride)
    _timed(f"{name}<K={KS},s={stride}>", 2.0 * B * (Tout if not transposed else T * stride) * M * Cin * taps, launch)
    return y_pre, y_out, stats


def conv_strided_wgrad(a: torch.Tensor, xl: torch.Tensor, KS: int, stride: int, dil: int, pad: int,
                       out: tp.Optional[torch.Tensor] = None, nsplit: tp.Optional[int] = None) -> torch.Tensor:
    """out[r][q][j] = sum_{b,u} a[b][r][u] * xl[b][q][u*stride + j*dil - pad]: a = dY, xl = x for the strided layer
    (-> [M, Cin, KS]); a = x, xl = dY for the transposed one (-> [Cin, M, KS]).  Deterministic split-K."""
    _req(a, "conv_strided_wgrad.a")
    _req(xl, "conv_strided_wgrad.xl")
    S, R, U = a.shape
    S2, Q, L = xl.shape
    assert S == S2, (a.shape, xl.shape)
    if out is None:
        out = torch.empty(R, Q, KS, device=a.device, dtype=torch.float32)
    else:
        _req(out, "conv_strided_wgrad.out")
        assert out.numel() == R * Q * KS
        _touched(out)
    if nsplit is None:
        nsplit = lib().bm_conv1d_strided_wgrad_suggest_splits(R, Q, KS, S, U)
    part = out if nsplit == 1 else torch.empty(nsplit * R * Q * KS, device=a.device, dtype=torch.float32)

    def launch():
        check(lib().bm_conv1d_strided_wgrad(_p(a), R * U, _p(xl), Q * L, _p(part), S, R, Q, U, L, KS, stride, dil, pad,
                                            nsplit, _stream()), "bm_conv1d_strided_wgrad")
    _timed(f"conv_strided_wgrad_kernel<K={KS},s={stride}>", 2.0 * S * U * R * Q * KS, launch)
    if part is not out:
        check(lib().bm_reduce_splits(_p(part), _p(out), 1, nsplit, R, Q, KS, R * Q * KS, Q * KS, KS, 1, _stream()),
              "bm_reduce_splits")
    return out


class DeviceFlag:
    """A word of flag bits per device that kernels raise and the host reads at a synchronisation point of its choosing:
    ``n_words`` int32, zero when first asked for.  Every owner (this module's index flag, the dataset's range flag, the
    two test epochs' label flags) is ONE instance: the words of two owners are never the same memory."""

    def __init__(self, n_words: int = 1):
        self.n_words = n_words
        self._words: tp.Dict[torch.device, torch.Tensor] = {}

    def __call__(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        flag = self._words.get(device)
        if flag is None:
            flag = self._words[device] = torch.zeros(self.n_words, device=device, dtype=torch.int32)
        return flag

    def take(self, device=None, word: int = 0) -> int:
        """Synchronising: the bits of ``word``, which it clears when any is set (the other words stay).  ``device=None``:
        of the first device, among those that have the flag, on which any is set."""
        for flag in (list(self._words.values()) if device is None else [self(device)]):
            bits = int(flag[word].item())
            if bits:
                flag[word:word + 1].zero_()
                return bits
        return 0


# Device-side "index out of range" flag (one int32 per device).  The grouped kernels never read outside
# their weight tables (bad indices are clamped to group 0 by bm_index_to_i32 / skipped by
# bm_group_by_index); the flag is raised as an IndexError at the next synchronisation point the caller
# chooses (`raise_if_index_error`, called by Solver next to the reference's isfinite asserts), or
# immediately with BM_CHECK_INDICES=1.
# Three words: [index out of range, non-finite input, loss mask bits: 1 = ClipLoss mask not all-true, NO_MASK_BIT,
# CATEGORY_RANGE_BIT]
index_error_flag = DeviceFlag(3)
_CHECK_INDICES_NOW = _os.environ.get("BM_CHECK_INDICES", "0") == "1"


def raise_if_index_error(device=None):
    """Synchronising check of the flag; raises like the reference's out-of-range gather would."""
    if index_error_flag.take(device):       # (the other two words -- non-finite input, bad mask -- belong to the Solver)
        raise IndexError("subject / layout index out of range for the weight table "
                         "(bm/models/common.py:57 would raise in `weights.gather`)")


def index_i32(idx: torch.Tensor, G: int) -> torch.Tensor:
    """idx [B] int64 -> int32 group indices, range-checked against [0, G) on the device."""
    _req(idx, "index_i32.idx", torch.int64)
    out = torch.empty(idx.numel(), device=idx.device, dtype=torch.int32)
    check(lib().bm_index_to_i32(_p(idx), idx.numel(), G, _p(out), _p(index_error_flag(idx.device)),
                                _stream()), "bm_index_to_i32")
    if _CHECK_INDICES_NOW:
        raise_if_index_error(idx.device)
    return out


def group_by_index(idx: torch.Tensor, G: int):
    """idx [B] int64 -> (order [B] int32, seg [G+1] int32)."""
    _req(idx, "group_by_index.idx", torch.int64)
    B = idx.numel()
    order = torch.empty(B, device=idx.device, dtype=torch.int32)
    seg = torch.empty(G + 1, device=idx.device, dtype=torch.int32)
    check(lib().bm_group_by_index(_p(idx), B, G, _p(order), _p(seg), _p(index_error_flag(idx.device)),
                                  _stream()), "bm_group_by_index")
    return order, seg


# The "NT" time contractions (csrc/gemm_nt*.hip).  Which kernel family serves a call, whether its operands are swapped
# and how many ways its reduction is split is decided in ONE place, _nt_plan; _nt_launch issues what it decided.
# Families: "f32" / "f32x3" (bm_gemm_nt / bm_gemm_nt_x3, any shape), and the wide f16x2 tiles "h2", "h2_rows",
# "h2_grouped" (bm_gemm_nt_h2*) and "scores" (bm_clip_scores_h2), which cover only some shapes.
_NT_SUFFIX = {"f32": "", "f32x3": "_x3"}        # family -> kernel family in the timer's labels (the wide tiles: "_h2w")


def _nt_plan(M, Cn, KS, S, T, G, dil, grouped, a_strides, x_strides, nsplit=None, partials=False):
    """(family, operands swapped, nsplit) of one contraction; ``partials``: the caller consumes the partial tiles
    themselves (the ClipLoss scores, one group, KS = 1).  A caller's ``nsplit`` is kept."""
    L = lib()
    family, swapped = _compute_dtype, False
    if family == "f16x2":
        family = "f32x3"        # shapes without a wide f16x2 kernel: the (equally fp32-accurate) 3 x bf16 kernels
        if partials:
            if L.bm_gemm_nt_h2_covers(M, Cn, 1, S, T, 1, 1, 0):
                # the score contraction proper (dense [M][T] x [Cn][T]): 256 x 256 tiles, transposed vector stores
                dense = S == 1 and tuple(a_strides) == (0, T) and tuple(x_strides) == (0, T)
                family = "scores" if dense and L.bm_clip_scores_h2_covers(M, Cn, T) else "h2"
        # rows T apart; the segment stride only matters when there is more than one segment
        elif a_strides[1] == T and x_strides[1] == T and \
                (S == 1 or (a_strides[0] == M * T and x_strides[0] == Cn * T)):
            # sum_t a[m][t] x[c][t] is symmetric in its operands: with the roles swapped the (M, Cn) rectangle may fit
            # the wide tiles (208 x 270 per (layout, subject) pair: 256 x 128 tiles) where (270, 208) does not
            covered = bool(L.bm_gemm_nt_h2_covers(M, Cn, KS, S, T, G, dil, int(grouped)))
            swapped = not covered and KS == 1 and bool(L.bm_gemm_nt_h2_covers(Cn, M, KS, S, T, G, dil, int(grouped)))
            if swapped:
                M, Cn = Cn, M
            if covered or swapped:
                family = "h2_grouped" if grouped else "h2_rows"
    if nsplit is None:
        if family == "scores":
            nsplit = L.bm_clip_scores_h2_suggest_splits(M, Cn, T)
        elif partials:
            nsplit = L.bm_gemm_nt_h2_suggest_splits(M, Cn, 1, S, T) if family == "h2" else \
                L.bm_clip_suggest_splits(M, Cn, S, T)
        elif family in _NT_SUFFIX:
            nsplit = L.bm_gemm_nt_suggest_splits(M, Cn, KS, S, T, G)
        else:
            nsplit = L.bm_gemm_nt_h2_suggest_splits_grouped(M, Cn, KS, S, T, G)
    return family, swapped, nsplit


def _nt_launch(family, label, a, x, part, S, G, M, Cn, T, KS, dil, a_strides, x_strides, order, seg, nsplit):
    """part[g, split][m][c*KS + j] (family "scores": [split][m][c]) by the entry point of ``family``, timed as ``label``."""
    L = lib()
    if family in _NT_SUFFIX:
        fn = L.bm_gemm_nt if family == "f32" else L.bm_gemm_nt_x3

        def launch():
            check(fn(_p(a), a_strides[0], a_strides[1], _p(x), x_strides[0], x_strides[1],
                     _p(_opt(order, "order", torch.int32)), _p(_opt(seg, "seg", torch.int32)), _p(part), S,
                     G, M, Cn, T, KS, dil, nsplit, _stream()), "bm_gemm_nt")
    else:
        a_amax, x_amax = amax(a), amax(x)
        a_rows = row_amax_of(a) if family == "h2_rows" else None    # published by the producer of `a` (act_bn_bwd / glu_bwd)
        if a_rows is not None and a_rows.numel() != M:
            a_rows = None

        def launch():
            if family == "scores":
                check(L.bm_clip_scores_h2(_p(a), _p(a_amax), _p(x), _p(x_amax), _p(part), M, Cn, T, nsplit, _stream()),
                      "bm_clip_scores_h2")
            elif family == "h2_grouped":
                check(L.bm_gemm_nt_h2_grouped(_p(a), a_strides[0], a_strides[1], _p(a_amax), _p(x), x_strides[0],
                                              x_strides[1], _p(x_amax), _p(_opt(order, "order", torch.int32)),
                                              _p(_opt(seg, "seg", torch.int32)), _p(part), S, G, M, Cn, T, nsplit,
                                              _stream()), "bm_gemm_nt_h2_grouped")
            elif family == "h2_rows":
                check(L.bm_gemm_nt_h2_rows(_p(a), a_strides[0], a_strides[1], _p(a_amax), _p(a_rows), _p(x),
                                           x_strides[0], x_strides[1], _p(x_amax), _p(part), S, M, Cn, T, KS, dil,
                                           nsplit, _stream()), "bm_gemm_nt_h2")
            else:
                check(L.bm_gemm_nt_h2(_p(a), a_strides[0], a_strides[1], _p(a_amax), _p(x), x_strides[0],
                                      x_strides[1], _p(x_amax), _p(part), S, M, Cn, T, KS, dil, nsplit, _stream()),
                      "bm_gemm_nt_h2")
    _timed(label.format(_NT_SUFFIX.get(family, "_h2w")), 2.0 * S * T * M * Cn * KS, launch)


def gemm_nt(a: torch.Tensor, x: torch.Tensor, S: int, M: int, Cn: int, T: int, KS: int = 1,
            dil: int = 1, a_strides=None, x_strides=None, order=None, seg=None, G: int = 1,
            out: tp.Optional[torch.Tensor] = None, out_strides=None, nsplit: tp.Optional[int] = None):
    """out[g*sg + m*sm + c*sc + j*sj] = sum_{s in g} sum_t a[s][m][t] * x[s][c][t + shift_j].

    a_strides / x_strides = (segment stride, row stride) in elements; defaults are contiguous
    [S][rows][T].  Default ``out`` is [G][M][Cn][KS] contiguous."""
    _req(a, "gemm_nt.a")
    _req(x, "gemm_nt.x")
    if a_strides is None:
        a_strides = (M * T, T)
    if x_strides is None:
        x_strides = (Cn * T, T)
    if out_strides is None:
        out_strides = (M * Cn * KS, Cn * KS, KS, 1)
    if out is None:
        out = torch.empty(G, M, Cn, KS, device=a.device, dtype=torch.float32)
    else:
        _touched(out)
    grouped = order is not None or seg is not None
    family, swapped, nsplit = _nt_plan(M, Cn, KS, S, T, G, dil, grouped, a_strides, x_strides, nsplit)
    if swapped:         # the result lands through the swapped output strides
        a, x, M, Cn, a_strides, x_strides = x, a, Cn, M, x_strides, a_strides
        out_strides = (out_strides[0], out_strides[2], out_strides[1], out_strides[3])
    canonical = tuple(out_strides) == (M * Cn * KS, Cn * KS, KS, 1)
    if nsplit == 1 and canonical:
        part = out
    else:
        part = torch.empty(G * nsplit * M * Cn * KS, device=a.device, dtype=torch.float32)
    _nt_launch(family, f"gemm_nt{{}}_kernel<KS={KS}>", a, x, part, S, G, M, Cn, T, KS, dil, a_strides, x_strides,
               order, seg, nsplit)
    if part is not out:
        check(lib().bm_reduce_splits(_p(part), _p(out), G, nsplit, M, Cn, KS, *out_strides,
                                     _stream()), "bm_reduce_splits")
    return out


class _DirectArmed:
    """(a plain counter, not thread-local: the autograd engine runs the backward nodes on its own worker thread)"""
    depth = 0

    @property
    def on(self):
        return self.depth > 0


_direct_armed = _DirectArmed()


class direct_grads_armed:
    """Context in which ``grad_destination`` hands out the flat-bucket views (``FlatAdam.writing_grads``): the
    backward pass of the training step, and nothing else -- gradients returned by ``torch.autograd.grad`` or produced
    by a stray backward must not alias the optimizer's bucket."""

    def __enter__(self):
        _direct_armed.depth += 1
        return self

    def __exit__(self, *exc):
        _direct_armed.depth -= 1
        return False


def grad_destination(param: torch.Tensor) -> tp.Optional[torch.Tensor]:
    """Where the weight gradient of ``param`` may be written directly: its view of the optimizer's flat gradient bucket
    (``FlatAdam`` registers it as ``param._bm_grad_dst``), handed out ONCE per ``zero_grad`` -- a parameter that
    takes part in the graph twice gets a fresh tensor the second time, and autograd accumulates as usual.  The
    returned view becomes ``param.grad`` without a copy (``FlatAdam.collect_grads`` recognises the address)."""
    dst = getattr(param, "_bm_grad_dst", None)
    if dst is None or dst[1][0] or param.grad is not None or not _direct_armed.on:
        return None
    dst[1][0] = True
    return dst[0]


def gemm_nt_partials(a, x, S, M, Cn, T, a_strides, x_strides, nsplit=None):
    """Split-K partial tiles [nsplit][M][Cn] (KS=1, one group), consumed by clip_ce."""
    _req(a, "gemm_nt.a")
    _req(x, "gemm_nt.x")
    family, _, nsplit = _nt_plan(M, Cn, 1, S, T, 1, 1, False, a_strides, x_strides, nsplit, partials=True)
    part = torch.empty(nsplit, M, Cn, device=a.device, dtype=torch.float32)
    _nt_launch(family, "clip_scores:gemm_nt{}", a, x, part, S, 1, M, Cn, T, 1, 1, a_strides, x_strides, None, None, nsplit)
    return part


def sum_over_batch(x: torch.Tensor) -> torch.Tensor:
    _req(x, "sum_over_batch.x")
    B = x.shape[0]
    out = torch.empty(x.shape[1:], device=x.device, dtype=torch.float32)
    check(lib().bm_sum_over_batch(_p(x), _p(out), B, out.numel(), _stream()), "bm_sum_over_batch")
    return out


# ------------------------------------------------------------------------------------------------
def bn_finalize(stats, count: int, gamma, beta, running_mean, running_var, num_batches,
                momentum: float, eps: float):
    _req(stats, "bn_finalize.stats")
    channel_major = getattr(stats, "_bm_channel_major", False)
    (C, ntiles, _) = stats.shape if channel_major else (stats.shape[1], stats.shape[0], 2)
    mean, invstd, scale, shift = (torch.empty(C, device=stats.device, dtype=torch.float32)
                                  for _ in range(4))
    check((lib().bm_bn_finalize_cm if channel_major else lib().bm_bn_finalize)(_p(stats), ntiles, C, count, _p(_opt(gamma, "gamma")),
                               _p(_opt(beta, "beta")), _p(_opt(running_mean, "running_mean")),
                               _p(_opt(running_var, "running_var")),
                               _p(_opt(num_batches, "num_batches", torch.int64)), momentum, eps,
                               _p(mean), _p(invstd), _p(scale), _p(shift), _stream()),
          "bm_bn_finalize")
    return mean, invstd, scale, shift


def bn_eval_affine(gamma, beta, running_mean, running_var, eps: float):
    _req(running_mean, "running_mean")
    C = running_mean.numel()
    mean, invstd, scale, shift = (torch.empty(C, device=running_mean.device, dtype=torch.float32)
                                  for _ in range(4))
    check(lib().bm_bn_eval_affine(C, _p(_opt(gamma, "gamma")), _p(_opt(beta, "beta")),
                                  _p(running_mean), _p(_req(running_var, "running_var")), eps,
                                  _p(mean), _p(invstd), _p(scale), _p(shift), _stream()),
          "bm_bn_eval_affine")
    return mean, invstd, scale, shift


def affine_act_res(y, scale, shift, res, act: int, leak: float = 0.):
    _req(y, "affine_act_res.y")
    B, C, T = y.shape
    out = torch.empty_like(y)
    check(lib().bm_affine_act_res(_p(y), _p(_opt(scale, "scale")), _p(_opt(shift, "shift")),
                                  _p(_opt(res, "res")), _p(out), B, C, T, act, leak, *_slot_args(_amax_slot(out)),
                                  _stream()), "bm_affine_act_res")
    return out


def act_bn_bwd(dout, y, scale, shift, mean, invstd, bn_train: bool, act: int, leak: float = 0.,
               want_affine_grads: bool = False, want_dbias: bool = True):
    """Returns (dy, dgamma | None, dbeta | None, dbias | None)."""
    _req(dout, "act_bn_bwd.dout")
    _req(y, "act_bn_bwd.y")
    B, C, T = y.shape
    dy = torch.empty_like(y)
    dgamma = torch.empty(C, device=y.device, dtype=torch.float32) if want_affine_grads else None
    dbeta = torch.empty(C, device=y.device, dtype=torch.float32) if want_affine_grads else None
    dbias = torch.empty(C, device=y.device, dtype=torch.float32) if want_dbias else None
    nbytes = lib().bm_act_bn_bwd_workspace_bytes(B, C)
    ws = torch.empty(nbytes, device=y.device, dtype=torch.uint8)
    slot = _amax_slot(dy)
    check(lib().bm_act_bn_bwd(_p(dout), _p(y), _p(_opt(scale, "scale")), _p(_opt(shift, "shift")),
                              _p(_opt(mean, "mean")), _p(_opt(invstd, "invstd")), int(bn_train),
                              _p(dy), _p(dgamma), _p(dbeta), _p(dbias), _p(ws), nbytes, B, C, T, act,
                              leak, *_slot_args(slot), _p(_row_amax_out(dy, slot)), _stream()), "bm_act_bn_bwd")
    return dy, dgamma, dbeta, dbias


def channel_sum(x: torch.Tensor) -> torch.Tensor:
    _req(x, "channel_sum.x")
    B, C, T = x.shape
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    nbytes = lib().bm_channel_sum_workspace_bytes(B, C)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    check(lib().bm_channel_sum(_p(x), C * T, _p(out), _p(ws), nbytes, B, C, T, _stream()),
          "bm_channel_sum")
    return out


def channel_stats(x: torch.Tensor) -> torch.Tensor:
    """[B, C, T] -> per-split (sum, sumsq) partials [nsplit, C, 2] for bn_finalize."""
    _req(x, "channel_stats.x")
    B, C, T = x.shape
    stats = torch.empty(lib().bm_channel_stats_splits(B), C, 2, device=x.device, dtype=torch.float32)
    check(lib().bm_channel_stats(_p(x), _p(stats), B, C, T, _stream()), "bm_channel_stats")
    return stats


def time_sums_t(x: torch.Tensor) -> torch.Tensor:
    """[B, C, T] -> [C, B]: out[c][b] = sum_t x[b][c][t]."""
    _req(x, "time_sums_t.x")
    B, C, T = x.shape
    out = torch.empty(C, B, device=x.device, dtype=torch.float32)
    check(lib().bm_time_sums_t(_p(x), _p(out), B, C, T, _stream()), "bm_time_sums_t")
    return out


def glu_fwd(u: torch.Tensor) -> torch.Tensor:
    _req(u, "glu_fwd.u")
    B, C2, T = u.shape
    out = torch.empty(B, C2 // 2, T, device=u.device, dtype=torch.float32)
    check(lib().bm_glu_fwd(_p(u), _p(out), B, C2 // 2, T, *_slot_args(_amax_slot(out)), _stream()), "bm_glu_fwd")
    return out


def glu_bwd(dout: torch.Tensor, u: torch.Tensor, want_dbias: bool = True):
    _req(dout, "glu_bwd.dout")
    _req(u, "glu_bwd.u")
    B, C2, T = u.shape
    H = C2 // 2
    du = torch.empty_like(u)
    dbias = torch.empty(C2, device=u.device, dtype=torch.float32) if want_dbias else None
    nbytes = lib().bm_glu_bwd_workspace_bytes(B, H)
    ws = torch.empty(nbytes, device=u.device, dtype=torch.uint8)
    slot = _amax_slot(du)
    check(lib().bm_glu_bwd(_p(dout), _p(u), _p(du), _p(dbias), _p(ws), nbytes, B, H, T,
                           *_slot_args(slot), _p(_row_amax_out(du, slot)), _stream()), "bm_glu_bwd")
    return du, dbias


# ------------------------------------------------------------------------------------------------
def fourier_emb(positions: torch.Tensor, D: int, margin: float = 0.2) -> torch.Tensor:
    _req(positions, "fourier_emb.positions")
    rows = positions.numel() // 2
    emb = torch.empty(*positions.shape[:-1], D, device=positions.device, dtype=torch.float32)
    check(lib().bm_fourier_emb(_p(positions), _p(emb), rows, D, margin, _stream()), "bm_fourier_emb")
    return emb


def masked_softmax(scores, positions, ban_center, ban_radius: float) -> torch.Tensor:
    _req(scores, "masked_softmax.scores")
    _req(positions, "masked_softmax.positions")
    U, O, C = scores.shape
    w = torch.empty_like(scores)
    check(lib().bm_masked_softmax(_p(scores), _p(positions), _p(_opt(ban_center, "ban_center")),
                                  float(ban_radius), _p(w), U, O, C, _stream()), "bm_masked_softmax")
    return w


def softmax_bwd(w, dw) -> torch.Tensor:
    _req(w, "softmax_bwd.w")
    _req(dw, "softmax_bwd.dw")
    ds = torch.empty_like(w)
    C = w.shape[-1]
    check(lib().bm_softmax_bwd(_p(w), _p(dw), _p(ds), w.numel() // C, C, _stream()),
          "bm_softmax_bwd")
    return ds


# ------------------------------------------------------------------------------------------------
def clip_inv_norms(cand: torch.Tensor, nonfinite_flag: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
    """1 / (1e-8 + ||cand[o]||) per candidate (bm/losses.py:91).  ONE pass over the candidates also yields what else
    a step needs from them: max |cand| (attached to the tensor like ``amax`` would, f16x2 mode) and -- with
    ``nonfinite_flag`` -- the reference's finiteness assert.  Cached on the tensor object together with its version
    counter: the Solver runs it when the batch arrives, ClipLoss finds the result."""
    checked = nonfinite_flag is not None
    cached = _noted(cand, "_bm_inv_norms", checked)
    if cached is not None:
        return cached
    _req(cand, "clip_inv_norms.cand")
    Bc = cand.shape[0]
    K = cand.numel() // max(Bc, 1)
    out = torch.empty(Bc, device=cand.device, dtype=torch.float32)
    have = _noted(cand, "_bm_amax", checked) is not None
    slot = None if have else _amax_slot(cand)            # None outside f16x2 mode
    check(lib().bm_clip_cand_prep(_p(cand), Bc, K, _p(out), _p(slot),
                                  _p(_opt(nonfinite_flag, "nonfinite_flag", torch.int32)), _stream()),
          "bm_clip_cand_prep")
    if slot is not None:
        _note(cand, "_bm_amax", slot, checked)
    _note(cand, "_bm_inv_norms", out, checked)
    return out


def flag_unless_all_set(mask: torch.Tensor, flag: torch.Tensor) -> None:
    """flag[0] |= 1 (device side, no sync) when the bool ``mask`` holds a False."""
    _req(mask, "flag_unless_all_set.mask", torch.bool)
    check(lib().bm_flag_unless_all_set(_p(mask), mask.numel(), _p(_req(flag, "flag", torch.int32)), _stream()),
          "bm_flag_unless_all_set")


# ------------------------------------------------------------------------------------------------
# Regression objective (csrc/regress.hip): L1Loss / L2Loss forward + backward, the test metrics' accumulators.
REGRESS_KINDS = {"l1": 0, "mse": 1}
METRIC_PLANES = 8          # sum l r m, sum l m, sum r m, sum (l m)^2, sum (r m)^2, sum m, sum ((l-r) m)^2, sum |(l-r) m|
NO_MASK_BIT = 2            # flag word slot 2: "no mask!" (bm/solver.py:354-356); bit 1 there is ClipLoss' mask assert


def _regress_mask(mask: tp.Optional[torch.Tensor], shape, what: str):
    """(mask | None, mask mode): None = all true, 1 = [B, 1, T] broadcast over F, 2 = [B, F, T]."""
    if mask is None:
        return None, 0
    _req(mask, f"{what}.mask", torch.bool)
    B, F, T = shape
    if tuple(mask.shape) == (B, 1, T):
        return mask, 1
    if tuple(mask.shape) == (B, F, T):
        return mask, 2
    raise BmHipError(f"{what}: mask of shape {tuple(mask.shape)} is neither [B, 1, T] nor [B, F, T] for {tuple(shape)}")


def regress_loss_fwd(est: torch.Tensor, out: torch.Tensor, mask: tp.Optional[torch.Tensor], kind: str,
                     flag: tp.Optional[torch.Tensor] = None):
    """(loss [] fp32, count [] fp64) of L1 / MSE over the selected elements, device side, no sync.  ``flag`` (int32
    device tensor, nullable): element 0 gets NO_MASK_BIT when nothing is selected (the loss is then NaN)."""
    _req(est, "regress_loss.est")
    _req(out, "regress_loss.out")
    if est.dim() != 3 or out.shape != est.shape:
        raise BmHipError(f"regress_loss: est {tuple(est.shape)} and out {tuple(out.shape)} must be the same [B, F, T]")
    mask, mode = _regress_mask(mask, est.shape, "regress_loss")
    B, F, T = est.shape
    loss = torch.empty((), device=est.device, dtype=torch.float32)
    count = torch.empty((), device=est.device, dtype=torch.float64)
    ws = _stream_ws("regress", est.device)
    check(lib().bm_regress_loss_fwd(_p(est), _p(out), _p(mask), mode, B, F, T, REGRESS_KINDS[kind], _p(loss),
                                    _p(count), _p(ws), ws.numel(), _p(_opt(flag, "flag", torch.int32)), _stream()),
          "bm_regress_loss_fwd")
    return loss, count


def regress_loss_bwd(est: torch.Tensor, out: torch.Tensor, mask: tp.Optional[torch.Tensor], kind: str,
                     grad_out: torch.Tensor, count: torch.Tensor, want_dout: bool = False):
    """(dEst, dOut | None).  In f16x2 mode dEst carries its maximum and per-channel maxima (published by the same
    launch) for the head's backward contractions."""
    _req(est, "regress_loss_bwd.est")
    _req(out, "regress_loss_bwd.out")
    mask, mode = _regress_mask(mask, est.shape, "regress_loss_bwd")
    B, F, T = est.shape
    dest = torch.empty_like(est)
    dout = torch.empty_like(out) if want_dout else None
    slot = _amax_slot(dest)
    ws = _stream_ws("regress", est.device)
    check(lib().bm_regress_loss_bwd(_p(est), _p(out), _p(mask), mode, B, F, T, REGRESS_KINDS[kind],
                                    _p(_req(grad_out, "grad_out")), _p(_req(count, "count", torch.float64)),
                                    _p(dest), _p(dout), _p(slot), _p(_row_amax_out(dest, slot)), _p(ws), ws.numel(),
                                    _stream()), "bm_regress_loss_bwd")
    return dest, dout


def regress_metric_update(est: torch.Tensor, out: torch.Tensor, mask: tp.Optional[torch.Tensor], acc: torch.Tensor,
                          t0: int = 0) -> torch.Tensor:
    """acc [METRIC_PLANES, F, T - t0] fp64 += the per-(f, t) sums over the batch of est / out [B, F, T] (fp32; a channel
    slice of a contiguous tensor is read in place), columns t >= t0 only.  mask: bool [B, 1, T] or [B, F, T], or None."""
    _req(est, "regress_metric_update.est", contiguous=False)
    _req(out, "regress_metric_update.out", contiguous=False)
    if est.dim() != 3 or out.shape != est.shape:
        raise BmHipError(f"regress_metric_update: est {tuple(est.shape)} / out {tuple(out.shape)}: same [B, F, T]")
    B, F, T = est.shape
    # rows T apart, channels contiguous: a channel slice of a [B, F', T] tensor keeps its segment stride
    est = est if est.stride()[1:] == (T, 1) else est.contiguous()
    out = out if out.stride()[1:] == (T, 1) else out.contiguous()
    if mask is not None:
        if not mask.is_contiguous():
            mask = mask.contiguous()
    mask, mode = _regress_mask(mask, est.shape, "regress_metric_update")
    _req(acc, "regress_metric_update.acc", torch.float64)
    if not 0 <= t0 < T or tuple(acc.shape) != (METRIC_PLANES, F, T - t0):
        raise BmHipError(f"regress_metric_update: acc {tuple(acc.shape)} / t0 {t0} for {tuple(est.shape)}")
    check(lib().bm_regress_metric_update(_p(est), est.stride(0), _p(out), out.stride(0), _p(mask),
                                         mask[0].numel() if mask is not None else 0, int(mode == 2), B, F, T, t0,
                                         _p(acc), _stream()), "bm_regress_metric_update")
    return acc


# The encode task's model input (csrc/encode.hip).
def meg_init(meg: torch.Tensor, limit: int) -> torch.Tensor:
    """x = meg for the samples t < limit, 0 for the others (bm/solver.py:288-292, ``mask * meg``): contiguous fp32
    [B, C, T] in, a new tensor out -- one launch that reads only the head and, in f16x2 mode, publishes max |x| (the
    first layer needs no pass over a tensor that is mostly zeros).  The tail is +0.0 whatever ``meg`` holds there."""
    _req(meg, "meg_init.meg")
    if meg.dim() != 3:
        raise BmHipError(f"meg_init: meg {tuple(meg.shape)} must be [B, C, T]")
    B, C, T = meg.shape
    x = torch.empty_like(meg)
    slot = _amax_slot(x)
    ws = _stream_ws("encode", meg.device) if slot is not None else None
    check(lib().bm_meg_init(_p(meg), _p(x), B, C, T, max(0, min(int(limit), T)), _p(slot), _p(ws), ws.numel() if ws is not None else 0,
                            _stream()), "bm_meg_init")
    return x


# task.lowpass (csrc/lowpass.hip): julius.lowpass_filter with stride 1 and pad=True.
_lowpass_taps: tp.Dict[tp.Any, tp.Tuple[torch.Tensor, int]] = {}


def _check_cutoff(cutoff: float) -> None:
    if cutoff < 0:
        raise ValueError("Minimum cutoff must be larger than zero.")
    if cutoff > 0.5:
        raise ValueError("A cutoff above 0.5 does not make sense.")
    if cutoff == 0:
        raise ValueError("A cutoff of 0 is not a filter (julius would return a null signal).")


def lowpass_taps(cutoff: float, zeros: float = 8, device=None) -> tp.Tuple[torch.Tensor, int]:
    """(taps, half): the ``2 * half + 1`` fp32 coefficients of julius' ``LowPassFilter(cutoff, zeros=zeros)`` -- a
    Hann-windowed sinc, normalised to a DC gain of 1 -- computed on the CPU with julius' own fp32 torch expressions, and
    uploaded to ``device`` if one is given; cached per (cutoff, zeros, device).  ``cutoff`` is a fraction of the sample
    rate in (0, 0.5]; julius raises ValueError outside [0, 0.5], and so does this, for 0 as well (julius then returns a
    null signal: not a filter this project has a use for)."""
    import math
    _check_cutoff(cutoff)
    device = torch.device(device) if device is not None else None
    key = (float(cutoff), float(zeros), device)
    hit = _lowpass_taps.get(key)
    if hit is not None:
        return hit
    half = int(zeros / cutoff / 2)
    time = torch.arange(-half, half + 1)
    win = torch.hann_window(2 * half + 1, periodic=False)
    arg = 2 * cutoff * math.pi * time
    sinc = torch.where(arg == 0, 1., torch.sin(arg) / arg)
    taps = 2 * cutoff * win * sinc
    taps /= taps.sum()
    assert taps.dtype == torch.float32 and taps.shape == (2 * half + 1,)
    if device is not None:
        taps = taps.to(device)
    if len(_lowpass_taps) >= 64:
        _lowpass_taps.clear()
    _lowpass_taps[key] = (taps, half)
    return taps, half


def _uniform_rows(x: torch.Tensor) -> tp.Optional[int]:
    """The distance in elements between consecutive rows of ``x`` seen as [rows, T] -- unit stride in the last
    dimension, every leading dimension a whole number of the one behind it -- or None when ``x`` has no such form."""
    T = x.shape[-1]
    if T != 1 and x.stride(-1) != 1:
        return None
    lead = [(n, s) for n, s in zip(x.shape[:-1], x.stride()[:-1]) if n != 1]
    if not lead:
        return T
    for (_, outer), (n, inner) in zip(lead[:-1], lead[1:]):
        if outer != n * inner:
            return None
    row_stride = lead[-1][1]
    return row_stride if row_stride >= T else None


def lowpass_filter(x: torch.Tensor, cutoff: float, stride: int = 1, pad: bool = True, zeros: float = 8,
                   fft: tp.Optional[bool] = None, keep: tp.Optional[int] = None,
                   publish_amax: bool = True) -> torch.Tensor:
    """``julius.lowpass_filter(x, cutoff, stride, pad, zeros, fft)`` over the last dimension (bm/solver.py:279 calls it
    with ``zeros=5``) in one launch of ``bm_lowpass``: replicate padding, same length out, a new contiguous tensor of
    ``x.shape``.  ``x``: fp32 on the GPU, any leading dimensions; a view whose rows are uniformly strided (``meg[...,
    offset:]``) is read in place, anything else is made contiguous first.  ``keep``: only the samples t < keep are
    computed, the others are +0.0 (the encode task's ``mask * lowpass(meg)``, bm/solver.py:288-292).

    Against julius: the result is always the direct sum (fp32 fmaf, taps ascending), where julius switches to an FFT
    convolution above 32 half-taps (``fft`` is accepted and ignored) -- the same mathematics, other last bits;
    ``stride != 1`` and ``pad=False`` are not built.  In f16x2 mode with ``publish_amax`` the launch also publishes
    max |y|: ``amax(y)`` costs no scan."""
    if stride != 1:
        raise NotImplementedError("lowpass_filter: stride != 1 (julius' decimating form) is not built")
    if not pad:
        raise NotImplementedError("lowpass_filter: pad=False (julius' valid convolution) is not built")
    _check_cutoff(cutoff)
    _req(x, "lowpass_filter.x", contiguous=False)
    if x.dim() < 1 or x.shape[-1] < 1:
        raise BmHipError(f"lowpass_filter: x {tuple(x.shape)} has no samples in its last dimension")
    taps, half = lowpass_taps(cutoff, zeros, x.device)
    T = x.shape[-1]
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    rows = y.numel() // T
    if rows == 0:
        return y
    row_stride = _uniform_rows(x)
    if row_stride is None:
        x, row_stride = x.contiguous(), T
    slot = _amax_slot(y) if publish_amax else None
    ws = _stream_ws("lowpass", x.device) if slot is not None else None
    check(lib().bm_lowpass(_p(x), row_stride, _p(y), rows, T, T if keep is None else max(0, min(int(keep), T)),
                           _p(taps), half, _p(slot), _p(ws), ws.numel() if ws is not None else 0, _stream()),
          "bm_lowpass")
    return y


# The long FIR of the MEG preprocessing (csrc/fir.hip; bm/studies/api.py:334-363): rows tiled in time, taps walked in chunks.
FIR_MAX_HALF, FIR_MAX_ROWS = 16384, 65535


def fir_tile() -> int:
    """Consecutive outputs of one row that a workgroup of ``bm_fir_rows`` owns."""
    return int(lib().bm_fir_tile())


def fir_chunk() -> int:
    """Values of ``j = tap + column`` (``ntaps + 15`` in all) that ``bm_fir_rows`` stages at a time."""
    return int(lib().bm_fir_chunk())


def fir_rows(x: torch.Tensor, taps: torch.Tensor, subtract: bool = False) -> torch.Tensor:
    """``s[..., t] = sum_k taps[k] * x[..., clamp(t + k - half, 0, T - 1)]`` over the last dimension, ``half = (ntaps - 1)
    / 2`` -- ``lowpass_filter``'s replicate padding without its limit on ``T + 2 half`` -- and ``x - s`` with
    ``subtract``: ONE launch of ``bm_fir_rows``, a new contiguous tensor of ``x.shape``.  ``x``: fp32 on the GPU, any
    leading dimensions; a view whose rows are uniformly strided is read in place, anything else is made contiguous
    first.  ``taps``: 1-D fp32 on the same device, of odd length.

    The sum is the exact-fp32 MFMA's fmaf chain, taps ascending from 0.f, whatever the compute mode: an output's bits
    depend on its own window alone, and for finite ``x`` the outputs equal ``lowpass_filter``'s as numbers wherever
    that applies.  A non-finite sample makes non-finite every output within ``half`` of it, may do so up to 15 samples
    further, and nothing beyond.  Limits (``ValueError`` before any launch): ``1 <= T < 2^31``, at most 65535 rows,
    ``ntaps`` odd, ``half <= 16384``."""
    if not isinstance(taps, torch.Tensor) or taps.dim() != 1 or taps.numel() % 2 != 1:
        raise ValueError(f"fir_rows: taps of shape {tuple(getattr(taps, 'shape', ()))}; a 1-D tensor of odd length "
                         "(2 half + 1)")
    half = (taps.numel() - 1) // 2
    if half > FIR_MAX_HALF:
        raise ValueError(f"fir_rows: half = {half}; the kernel takes half <= {FIR_MAX_HALF}")
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("fir_rows: x has no last dimension")
    T = x.shape[-1]
    if not 1 <= T < 2 ** 31:
        raise ValueError(f"fir_rows: rows of {T} samples; the kernel takes 1 <= T < 2^31")
    rows = x.numel() // T
    if rows > FIR_MAX_ROWS:
        raise ValueError(f"fir_rows: {rows} rows in one call, the limit is {FIR_MAX_ROWS}")
    _req(x, "fir_rows.x", contiguous=False)
    _req(taps, "fir_rows.taps")
    if taps.device != x.device:
        raise BmHipError(f"fir_rows: taps on {taps.device}, x on {x.device}")
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    if rows == 0:
        return y
    row_stride = _uniform_rows(x)
    if row_stride is None:
        x, row_stride = x.contiguous(), T

    def launch():
        check(lib().bm_fir_rows(_p(x), row_stride, _p(y), rows, T, _p(taps), taps.numel(), int(bool(subtract)),
                                _stream()), "bm_fir_rows")
    _timed("fir_rows", 2. * taps.numel() * rows * T, launch)
    return y


def highpass_filter(x: torch.Tensor, cutoff: float, stride: int = 1, pad: bool = True, zeros: float = 8,
                    fft: tp.Optional[bool] = None) -> torch.Tensor:
    """``julius.highpass_filter(x, cutoff, stride, pad, zeros, fft)`` over the last dimension: ``x - lowpass(x)``, what
    ``julius.HighPassFilter`` computes, as ``lowpass_taps(cutoff, zeros)`` and ONE ``bm_fir_rows`` launch that
    subtracts in its epilogue.  ``x`` as for ``fir_rows``.  Always the direct sum (``fft`` is accepted and ignored);
    ``stride != 1`` and ``pad=False`` are not built."""
    if stride != 1:
        raise NotImplementedError("highpass_filter: stride != 1 (julius' decimating form) is not built")
    if not pad:
        raise NotImplementedError("highpass_filter: pad=False (julius' valid convolution) is not built")
    _check_cutoff(cutoff)
    half = int(zeros / cutoff / 2)
    if half > FIR_MAX_HALF:
        raise ValueError(f"highpass_filter: cutoff {cutoff} with zeros = {zeros} is half = {half}; the kernel takes "
                         f"half <= {FIR_MAX_HALF}")
    device = x.device if isinstance(x, torch.Tensor) else None
    taps, _ = lowpass_taps(cutoff, zeros, device)
    return fir_rows(x, taps, subtract=True)


# FeatureDecodingLoss / ClassificationAcc (csrc/regress.hip). ``table``: one row per feature, (kind, est_start, width,
# out_start, weight_off) with kind 0 = continuous, 1 = categorical (width = number of classes) and weight_off the
# feature's offset into ``weights`` or -1.
FEATURE_CONTINUOUS, FEATURE_CATEGORICAL = 0, 1
CATEGORY_RANGE_BIT = 4     # flag word slot 2: a class outside [0, K) (the assert of bm/losses.py:150)


def _feature_table(table):
    flat = [int(v) for row in table for v in row]
    if not table or len(flat) != 5 * len(table):
        raise BmHipError("feature_decoding: table must hold rows (kind, est_start, width, out_start, weight_off)")
    return (ctypes.c_int * len(flat))(*flat), len(table)


def _feature_decoding_args(est, out, mask, weights, what):
    _req(est, f"{what}.est")
    _req(out, f"{what}.out")
    if est.dim() != 3 or out.dim() != 3 or est.shape[0] != out.shape[0] or est.shape[2] != out.shape[2]:
        raise BmHipError(f"{what}: est {tuple(est.shape)} / out {tuple(out.shape)} must be [B, C, T] and [B, Co, T]")
    B, C, T = est.shape
    if mask is not None:
        _req(mask, f"{what}.mask", torch.bool)
        if tuple(mask.shape) != (B, 1, T):
            raise BmHipError(f"{what}: mask of shape {tuple(mask.shape)} is not [B, 1, T] for {tuple(est.shape)}")
    _opt(weights, f"{what}.weights")
    return B, C, out.shape[1], T


def feature_decoding_fwd(est: torch.Tensor, out: torch.Tensor, mask: tp.Optional[torch.Tensor], table,
                         weights: tp.Optional[torch.Tensor] = None, flag: tp.Optional[torch.Tensor] = None):
    """(loss [] fp32, terms [n_features] fp32, denoms [n_features] fp64, lse [n_categorical, B, T] fp32) of
    FeatureDecodingLoss, device side, no sync.  ``flag`` (int32 device tensor, nullable): element 0 gets NO_MASK_BIT when
    nothing is selected (the loss is NaN) and CATEGORY_RANGE_BIT when a class is outside [0, K)."""
    B, C, Co, T = _feature_decoding_args(est, out, mask, weights, "feature_decoding")
    rows, n = _feature_table(table)
    n_cat = sum(1 for row in table if row[0] == FEATURE_CATEGORICAL)
    loss = torch.empty((), device=est.device, dtype=torch.float32)
    terms = torch.empty(n, device=est.device, dtype=torch.float32)
    denoms = torch.empty(n, device=est.device, dtype=torch.float64)
    lse = torch.empty(n_cat, B, T, device=est.device, dtype=torch.float32)
    ws = _stream_ws("regress", est.device)
    check(lib().bm_feature_decoding_fwd(_p(est), _p(out), _p(mask), _p(weights),
                                        0 if weights is None else weights.numel(), rows, n, B, C, Co, T, _p(loss),
                                        _p(terms), _p(denoms), _p(lse), _p(ws), ws.numel(),
                                        _p(_opt(flag, "flag", torch.int32)), _stream()), "bm_feature_decoding_fwd")
    return loss, terms, denoms, lse


def feature_decoding_bwd(est: torch.Tensor, out: torch.Tensor, mask: tp.Optional[torch.Tensor], table,
                         weights: tp.Optional[torch.Tensor], grad_out: torch.Tensor, denoms: torch.Tensor,
                         lse: torch.Tensor) -> torch.Tensor:
    """dEst of FeatureDecodingLoss: allocated with ``empty``, every element written by the one launch.  (The gradient's
    maximum is not published: an f16x2 consumer finds it with the generic ``amax`` scan.)"""
    B, C, Co, T = _feature_decoding_args(est, out, mask, weights, "feature_decoding_bwd")
    rows, n = _feature_table(table)
    dest = torch.empty_like(est)
    check(lib().bm_feature_decoding_bwd(_p(est), _p(out), _p(mask), _p(weights),
                                        0 if weights is None else weights.numel(), rows, n, B, C, Co, T,
                                        _p(_req(grad_out, "grad_out")), _p(_req(denoms, "denoms", torch.float64)),
                                        _p(_req(lse, "lse")), _p(dest), _stream()), "bm_feature_decoding_bwd")
    return dest


def class_acc_update(est: torch.Tensor, target: torch.Tensor, mask: tp.Optional[torch.Tensor], acc: torch.Tensor,
                     t0: int = 0) -> torch.Tensor:
    """acc [2, T - t0] int64 (hits, selected count) += over the batch of est [B, K, T] (logits) against target [B, 1, T]
    (the class as a float), columns t >= t0 only; channel slices of contiguous tensors are read in place.  mask: bool
    [B, 1, T] or None."""
    _req(est, "class_acc_update.est", contiguous=False)
    _req(target, "class_acc_update.target", contiguous=False)
    if est.dim() != 3 or target.dim() != 3 or tuple(target.shape) != (est.shape[0], 1, est.shape[2]):
        raise BmHipError(f"class_acc_update: est {tuple(est.shape)} / target {tuple(target.shape)}: [B, K, T] and "
                         "[B, 1, T]")
    B, K, T = est.shape
    est = est if est.stride()[1:] == (T, 1) else est.contiguous()
    target = target if target.stride(2) == 1 else target.contiguous()
    if mask is not None:
        if mask.dtype != torch.bool or tuple(mask.shape) != (B, 1, T):
            raise BmHipError(f"class_acc_update: mask must be bool [B, 1, T], got {mask.dtype} {tuple(mask.shape)}")
        mask = _req(mask if mask.is_contiguous() else mask.contiguous(), "class_acc_update.mask", torch.bool)
    _req(acc, "class_acc_update.acc", torch.int64)
    if not 0 <= t0 < T or tuple(acc.shape) != (2, T - t0):
        raise BmHipError(f"class_acc_update: acc {tuple(acc.shape)} / t0 {t0} for {tuple(est.shape)}")
    check(lib().bm_class_acc_update(_p(est), est.stride(0), _p(target), target.stride(0), _p(mask),
                                    T if mask is not None else 0, B, K, T, t0, _p(acc), _stream()),
          "bm_class_acc_update")
    return acc


def clip_ce(part, inv_norm, want_probs=False, want_grad=False, want_loss=False,
            target_offset: int = 0, col_valid: tp.Optional[torch.Tensor] = None):
    """part [nsplit][B][B'] -> (scores, probs|None, dscaled|None, loss|None).  ``col_valid`` ([B'] fp32, optional):
    candidates with 0 there are masked out of every row (score -inf, probability 0, gradient 0)."""
    _req(part, "clip_ce.part")
    nsplit, B, Bc = part.shape
    dev = part.device
    scores = torch.empty(B, Bc, device=dev, dtype=torch.float32)
    probs = torch.empty(B, Bc, device=dev, dtype=torch.float32) if want_probs else None
    dscaled = torch.empty(B, Bc, device=dev, dtype=torch.float32) if want_grad else None
    loss_row = torch.empty(B, device=dev, dtype=torch.float32) if want_loss else None
    loss = torch.empty((), device=dev, dtype=torch.float32) if want_loss else None
    check(lib().bm_clip_ce_masked(_p(part), nsplit, _p(_req(inv_norm, "inv_norm")), _p(_opt(col_valid, "col_valid")),
                                  _p(scores), _p(probs), _p(dscaled), _p(loss_row), _p(loss), B, Bc, target_offset,
                                  _stream()), "bm_clip_ce")
    return scores, probs, dscaled, loss


def clip_ce_cols(scores, inv_norm, dscaled, loss, target_offset: int = 0, w_row: float = 0.5, w_col: float = 0.5):
    """Column term of the symmetric objective on top of ``clip_ce``'s outputs: ``dscaled`` (row term) and ``loss``
    (row loss) are updated in place to the weighted sums; returns the per-target column losses [B]."""
    _req(scores, "clip_ce_cols.scores")
    B, Bc = scores.shape
    loss_col = torch.empty(B, device=scores.device, dtype=torch.float32)
    for t in (dscaled, loss):
        if t is not None:
            _touched(t)
    check(lib().bm_clip_ce_cols(_p(scores), _p(_req(inv_norm, "inv_norm")), _p(_opt(dscaled, "dscaled")),
                                _p(loss_col), _p(_opt(loss, "loss")), B, Bc, target_offset, w_row, w_col, _stream()),
          "bm_clip_ce_cols")
    return loss_col


def clip_cand_coef(dscaled, scores, inv_norm, alpha=None) -> torch.Tensor:
    _req(dscaled, "clip_cand_coef.dscaled")
    _req(scores, "clip_cand_coef.scores")
    B, Bc = dscaled.shape
    coef = torch.empty(Bc, device=dscaled.device, dtype=torch.float32)
    check(lib().bm_clip_cand_coef(_p(dscaled), _p(scores), _p(_req(inv_norm, "inv_norm")),
                                  _p(_opt(alpha, "alpha")), _p(coef), B, Bc, _stream()),
          "bm_clip_cand_coef")
    return coef


def row_axpy_sub(y: torch.Tensor, x: torch.Tensor, coef: torch.Tensor):
    """y[r] -= coef[r] * x[r] (in place), rows = first dimension."""
    _req(y, "row_axpy_sub.y")
    _req(x, "row_axpy_sub.x")
    rows = y.shape[0]
    check(lib().bm_row_axpy_sub(_p(y), _p(x), _p(_req(coef, "coef")), rows, y.numel() // max(rows, 1),
                                _stream()), "bm_row_axpy_sub")
    return _touched(y)


def center_scale(x: torch.Tensor, center: torch.Tensor, scale: torch.Tensor,
                 group: tp.Optional[torch.Tensor] = None, clip: bool = False, limit: float = 0.,
                 want_maxabs: bool = False, inplace: bool = False):
    """(x - center[group[b]]) / scale[group[b]] [clamped]; returns (out, maxabs [B] | None)."""
    _req(x, "center_scale.x")
    _req(center, "center_scale.center")
    _req(scale, "center_scale.scale")
    B, C, T = x.shape
    assert center.shape[-1] == C and scale.shape == center.shape
    out = _touched(x) if inplace else torch.empty_like(x)
    maxabs = torch.zeros(B, device=x.device, dtype=torch.float32) if want_maxabs else None
    check(lib().bm_center_scale(_p(x), _p(out), _p(_opt(group, "group", torch.int64)), _p(center),
                                _p(scale), B, C, T, int(clip), float(limit), _p(maxabs), _stream()),
          "bm_center_scale")
    return out, maxabs


def center_scale_inverse(x: torch.Tensor, center: torch.Tensor, scale: torch.Tensor,
                         group: tp.Optional[torch.Tensor] = None, inplace: bool = False) -> torch.Tensor:
    """(x * scale[group[b]]) + center[group[b]], two roundings (bm/norm.py:85-86, 110-111)."""
    _req(x, "center_scale_inverse.x")
    _req(center, "center_scale_inverse.center")
    _req(scale, "center_scale_inverse.scale")
    B, C, T = x.shape
    assert center.shape[-1] == C and scale.shape == center.shape
    out = _touched(x) if inplace else torch.empty_like(x)
    check(lib().bm_center_scale_inverse(_p(x), _p(out), _p(_opt(group, "group", torch.int64)), _p(center), _p(scale),
                                        B, C, T, _stream()), "bm_center_scale_inverse")
    return out


MAX_QUANTILE_RANKS = 8
MAX_CATEGORY_CARDINALITY = 16384
CATEGORY_NOT_INTEGER, CATEGORY_MAX, CATEGORY_MIN = 1, 2, 4      # bits of category_counts' flag word


def quantile_select(x: torch.Tensor, ranks: tp.Sequence[int]) -> torch.Tensor:
    """out [C, Q]: the values at the (ascending) indices ``ranks`` of every column x[:, c, :] of x [N, C, T] sorted
    ascending -- what ``torch.sort`` leaves there, NaNs last.  No host synchronisation."""
    _req(x, "quantile_select.x")
    if x.dim() != 3:
        raise BmHipError(f"quantile_select: x {tuple(x.shape)} must be [N, C, T]")
    N, C, T = x.shape
    ranks = [int(r) for r in ranks]
    Q = len(ranks)
    if not 1 <= Q <= MAX_QUANTILE_RANKS:
        raise BmHipError(f"quantile_select: 1 to {MAX_QUANTILE_RANKS} ranks, got {Q}")
    out = torch.empty(C, Q, device=x.device, dtype=torch.float32)
    ws = torch.zeros(lib().bm_quantile_select_workspace_bytes(C, Q), device=x.device, dtype=torch.uint8)
    host_ranks = (ctypes.c_long * Q)(*ranks)
    check(lib().bm_quantile_select(_p(x), ctypes.cast(host_ranks, ctypes.c_void_p), _p(out), N, C, T, Q, _p(ws),
                                   ws.numel(), _stream()), "bm_quantile_select")
    return out


def masked_moments(x: torch.Tensor, mask: tp.Optional[torch.Tensor], f0: int, f1: int, per_channel: bool):
    """(count fp64, mean fp32, std fp32), each [f1 - f0]: masked mean and unbiased std of the channels [f0, f1) of
    x [N, F, T]; without ``per_channel`` one statistic over the whole slice, written to every channel."""
    _req(x, "masked_moments.x")
    if x.dim() != 3:
        raise BmHipError(f"masked_moments: x {tuple(x.shape)} must be [N, F, T]")
    mask, mode = _regress_mask(mask, x.shape, "masked_moments")
    N, F, T = x.shape
    if not 0 <= f0 < f1 <= F:
        raise BmHipError(f"masked_moments: channel range [{f0}, {f1}) outside [0, {F})")
    nch = f1 - f0
    mean = torch.empty(nch, device=x.device, dtype=torch.float32)
    std = torch.empty(nch, device=x.device, dtype=torch.float32)
    count = torch.empty(nch, device=x.device, dtype=torch.float64)
    ws = torch.zeros(lib().bm_masked_moments_workspace_bytes(nch), device=x.device, dtype=torch.uint8)
    check(lib().bm_masked_moments(_p(x), _p(mask), mode, N, F, T, f0, f1, int(per_channel), _p(mean), _p(std),
                                  _p(count), _p(ws), ws.numel(), _stream()), "bm_masked_moments")
    return count, mean, std


def category_counts(x: torch.Tensor, mask: tp.Optional[torch.Tensor], f: int, cardinality: int):
    """(counts fp32 [cardinality], flags int32 [1]) of channel ``f`` of x [N, F, T]: how often every category occurs
    among the selected values, and the CATEGORY_* bits of the reference's assert over all values."""
    if cardinality > MAX_CATEGORY_CARDINALITY:
        raise ValueError(f"category_counts: cardinality {cardinality} exceeds the cap of {MAX_CATEGORY_CARDINALITY} "
                         "bins (the histogram lives in LDS)")
    _req(x, "category_counts.x")
    if x.dim() != 3:
        raise BmHipError(f"category_counts: x {tuple(x.shape)} must be [N, F, T]")
    mask, mode = _regress_mask(mask, x.shape, "category_counts")
    N, F, T = x.shape
    counts = torch.zeros(cardinality, device=x.device, dtype=torch.float32)
    flags = torch.zeros(1, device=x.device, dtype=torch.int32)
    ws = torch.zeros(lib().bm_category_counts_workspace_bytes(cardinality), device=x.device, dtype=torch.uint8)
    check(lib().bm_category_counts(_p(x), _p(mask), mode, N, F, T, f, cardinality, _p(counts), _p(flags), _p(ws),
                                   ws.numel(), _stream()), "bm_category_counts")
    return counts, flags


def row_softmax(x: torch.Tensor) -> torch.Tensor:
    _req(x, "row_softmax.x")
    y = torch.empty_like(x)
    check(lib().bm_row_softmax(_p(x), _p(y), x.shape[0], x.shape[1], _stream()), "bm_row_softmax")
    return y


def rowwise_dot(a: torch.Tensor, b: torch.Tensor, scale=None) -> torch.Tensor:
    _req(a, "rowwise_dot.a")
    _req(b, "rowwise_dot.b")
    rows = a.shape[0]
    out = torch.empty(rows, device=a.device, dtype=torch.float32)
    check(lib().bm_rowwise_dot(_p(a), _p(b), _p(_opt(scale, "scale")), _p(out), rows,
                               a.numel() // max(rows, 1), _stream()), "bm_rowwise_dot")
    return out


def segment_sum_cols(p: torch.Tensor, order: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    _req(p, "segment_sum_cols.p")
    rows, cols = p.shape
    V = seg.numel() - 1
    pv = torch.empty(rows, V, device=p.device, dtype=torch.float32)
    check(lib().bm_segment_sum_cols(_p(p), _p(_req(order, "order", torch.int32)),
                                    _p(_req(seg, "seg", torch.int32)), _p(pv), rows, cols, V, _stream()),
          "bm_segment_sum_cols")
    return pv


def topk_rows(x: torch.Tensor, k: int, col_labels=None, row_labels=None):
    """x [N, V] -> (idx [N, k] int32, values [N, k], hits [N] int32 | None)."""
    _req(x, "topk_rows.x")
    N, V = x.shape
    idx = torch.empty(N, k, device=x.device, dtype=torch.int32)
    val = torch.empty(N, k, device=x.device, dtype=torch.float32)
    hits = torch.empty(N, device=x.device, dtype=torch.int32) if col_labels is not None else None
    check(lib().bm_topk_rows(_p(x), N, V, k, _p(idx), _p(val),
                             _p(_opt(col_labels, "col_labels", torch.int64)),
                             _p(_opt(row_labels, "row_labels", torch.int64)), _p(hits), _stream()),
          "bm_topk_rows")
    return idx, val, hits


def adam_step(param, grad, exp_avg, exp_avg_sq, step: int, lr: float, beta1: float, beta2: float,
              eps: float, grad_scale: float = 1.0):
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, f"adam_step.{n}")
    check(lib().bm_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), step,
                             lr, beta1, beta2, eps, grad_scale, _stream()), "bm_adam_step")
    for t in (param, exp_avg, exp_avg_sq):
        _touched(t)
    weights_changed()


# ------------------------------------------------------------------------------------------------
# LSTM recurrence (csrc/lstm.hip): one call per (layer, pass) enqueues all T step launches, both directions of a
# bidirectional layer in the same launches.  Exact-fp32 MFMA in every compute mode; time-major tensors [T][C][B].
def _per_dir(ts, name=None, shape=None):
    """The two pointer arguments of a per-direction operand (None for the direction a one-directional layer lacks);
    ``ts`` = a list of tensors or one tensor [dirs, ...].  With a ``name`` every entry is checked against ``shape``."""
    if name is not None:
        for t in ts:
            _req(t, name)
            assert tuple(t.shape) == shape, (name, tuple(t.shape), shape)
    return [_p(t) for t in ts] + [None] * (2 - len(ts))


def lstm_layer_fwd(whh: tp.Sequence[torch.Tensor], gx: tp.Sequence[torch.Tensor]):
    """whh[d] = weight_hh [4H, H] (the parameter itself), gx[d] [T, 4H, B] = W_ih x + b_ih + b_hh per direction ->
    (y [T, H * dirs, B], gates [dirs, T, 4H, B] activated i, f, g, o, c [dirs, T, H, B]); zero initial state."""
    dirs = len(whh)
    assert dirs in (1, 2) and len(gx) == dirs
    T, H4, B = gx[0].shape
    Hd = H4 // 4
    dev = gx[0].device
    whh_p = _per_dir(whh, "lstm_layer_fwd.whh", (H4, Hd))
    gx_p = _per_dir(gx, "lstm_layer_fwd.gx", (T, H4, B))
    y = torch.empty(T, Hd * dirs, B, device=dev, dtype=torch.float32)
    gates = torch.empty(dirs, T, H4, B, device=dev, dtype=torch.float32)
    c = torch.empty(dirs, T, Hd, B, device=dev, dtype=torch.float32)

    def launch():
        check(lib().bm_lstm_layer_fwd(*whh_p, *gx_p, _p(y), *_per_dir(gates), *_per_dir(c), Hd, B, T, dirs, _stream()),
              "bm_lstm_layer_fwd")
    _timed(f"lstm_step_fwd_kernel<dirs={dirs}>", 2.0 * T * dirs * H4 * Hd * B, launch)
    return y, gates, c


def lstm_layer_bwd(whh: tp.Sequence[torch.Tensor], dy: torch.Tensor, gates: torch.Tensor, c: torch.Tensor,
                   dc: torch.Tensor) -> torch.Tensor:
    """dy [T, H * dirs, B] (dL/dh_n already added at each direction's last step), the saved gates / c of
    ``lstm_layer_fwd``, dc [dirs, H, B] = dL/dc_n (OVERWRITTEN: the carried cell gradient) -> dg [dirs, T, 4H, B]."""
    dirs = len(whh)
    _req(dy, "lstm_layer_bwd.dy")
    _req(gates, "lstm_layer_bwd.gates")
    _req(c, "lstm_layer_bwd.c")
    _req(dc, "lstm_layer_bwd.dc")
    _, T, H4, B = gates.shape
    Hd = H4 // 4
    assert gates.shape[0] == dirs and tuple(dy.shape) == (T, Hd * dirs, B) and tuple(c.shape) == (dirs, T, Hd, B) \
        and tuple(dc.shape) == (dirs, Hd, B), (dy.shape, gates.shape, c.shape, dc.shape)
    whh_p = _per_dir(whh, "lstm_layer_bwd.whh", (H4, Hd))
    dg = torch.empty_like(gates)
    _touched(dc)

    def launch():
        check(lib().bm_lstm_layer_bwd(*whh_p, _p(dy), *_per_dir(gates), *_per_dir(c), *_per_dir(dg), *_per_dir(dc),
                                      Hd, B, T, dirs, _stream()), "bm_lstm_layer_bwd")
    _timed(f"lstm_step_bwd_kernel<dirs={dirs}>", 2.0 * T * dirs * H4 * Hd * B, launch)
    return dg


# ------------------------------------------------------------------------------------------------
# optim.svd (csrc/spectral.hip, bm/svd.py:17-45): the low-rank estimate of every weight's largest singular value, squared,
# and its closed-form gradient -- all matrices of a model in the same launches.  Exact-fp32 MFMA in every compute mode.
SPECTRAL_MAX_DIM = 16
SPECTRAL_MAX_NITERS = 8


def spectral_check_limits(dim: int, niters: int) -> None:
    if not 1 <= dim <= SPECTRAL_MAX_DIM:
        raise ValueError(f"svd_penalty: dim = {dim}, the kernels take 1..{SPECTRAL_MAX_DIM} (the projection is one "
                         f"{SPECTRAL_MAX_DIM}-wide MFMA operand)")
    if not 0 <= niters <= SPECTRAL_MAX_NITERS:
        raise ValueError(f"svd_penalty: niters = {niters}, the kernels take 0..{SPECTRAL_MAX_NITERS}")


class SpectralPlan:
    """The device table of ``bm_spectral_*`` for one list of weights (viewed as ``p.view(p.shape[0], -1)``, read in
    place) and the two workspaces.  ``sizes[i]`` = min(rows, cols): the rows matrix i takes of the test matrix R.
    ``generation`` counts the forward passes: the backward needs the workspaces as ITS forward left them."""

    def __init__(self, weights: tp.Sequence[torch.Tensor], dim: int, niters: int):
        spectral_check_limits(dim, niters)
        L = lib()
        self.dim, self.niters, self.nmat = dim, niters, len(weights)
        self.device = weights[0].device
        self.shapes = [tuple(w.shape) for w in weights]
        entry = L.bm_spectral_table_entry_bytes()
        host = torch.zeros(self.nmat, entry, dtype=torch.uint8)
        self.sizes, self.grad_offsets = [], []
        wsf = wsd = r_off = g_off = 0
        self.max_slabs = self.max_tiles = 1
        for i, w in enumerate(weights):
            _req(w, "spectral.weight")
            if w.dim() < 2 or w.numel() == 0 or w.device != self.device:
                raise BmHipError(f"spectral: weight {i} of shape {tuple(w.shape)} on {w.device} is no matrix of this plan")
            rows, cols = w.shape[0], w.numel() // w.shape[0]
            check(L.bm_spectral_table_fill(ctypes.c_void_p(host[i].data_ptr()), _p(w), rows, cols, cols, dim, r_off, wsf,
                                           wsd, g_off), "bm_spectral_table_fill")
            self.sizes.append(min(rows, cols))
            self.grad_offsets.append(g_off)
            r_off += min(rows, cols)
            g_off += rows * cols
            wsf += L.bm_spectral_ws_floats(rows, cols, niters)
            wsd += L.bm_spectral_ws_doubles(rows, cols, niters)
            self.max_slabs = max(self.max_slabs, -(-max(rows, cols) // 64))
            self.max_tiles = max(self.max_tiles, -(-rows // 64) * -(-cols // 64))
        self.r_rows, self.grad_numel = r_off, g_off
        self.table = host.to(self.device)
        self.ws_floats = torch.empty(wsf, device=self.device, dtype=torch.float32)
        self.ws_doubles = torch.empty(wsd, device=self.device, dtype=torch.float64)
        self.generation = 0


_spectral_plans: tp.Dict[tuple, SpectralPlan] = {}


def spectral_plan(weights: tp.Sequence[torch.Tensor], dim: int, niters: int) -> SpectralPlan:
    """The plan of these weights, kept while their addresses and shapes stay (a model's parameters do)."""
    for w in weights:
        _req(w, "spectral.weight")
    key = (tuple((w.data_ptr(), tuple(w.shape)) for w in weights), dim, niters, weights[0].device,
           torch.cuda.current_stream(weights[0].device).cuda_stream)
    plan = _spectral_plans.get(key)
    if plan is None:
        if len(_spectral_plans) >= 8:
            _spectral_plans.clear()
        plan = _spectral_plans[key] = SpectralPlan(weights, dim, niters)
    return plan


def spectral_fwd(plan: SpectralPlan, R: torch.Tensor) -> tp.Tuple[torch.Tensor, torch.Tensor]:
    """R [sum of min(rows, cols), dim] -> (sum of the estimates (0-dim), the estimates [nmat])."""
    _req(R, "spectral_fwd.R")
    if tuple(R.shape) != (plan.r_rows, plan.dim):
        raise BmHipError(f"spectral_fwd: R is {tuple(R.shape)}, these weights need {(plan.r_rows, plan.dim)}")
    values = torch.empty(plan.nmat, device=plan.device, dtype=torch.float32)
    total = torch.empty((), device=plan.device, dtype=torch.float32)
    plan.generation += 1

    def launch():
        check(lib().bm_spectral_fwd(_p(plan.table), plan.nmat, plan.max_slabs, _p(R), plan.dim, plan.niters,
                                    _p(plan.ws_floats), _p(plan.ws_doubles), _p(values), _p(total), _stream()),
              "bm_spectral_fwd")
    _timed("spectral_fwd", 0., launch)
    return total, values


def spectral_bwd(plan: SpectralPlan, gscale: torch.Tensor) -> tp.List[torch.Tensor]:
    """After ``spectral_fwd`` on the same plan: ``gscale`` (one fp32 element on the device) times the gradient of every
    estimate, as fresh tensors of the weights' shapes (views of one new buffer)."""
    _req(gscale, "spectral_bwd.gscale")
    assert gscale.numel() == 1
    flat = torch.empty(plan.grad_numel, device=plan.device, dtype=torch.float32)

    def launch():
        check(lib().bm_spectral_bwd(_p(plan.table), plan.nmat, plan.max_slabs, plan.max_tiles, plan.niters,
                                    _p(plan.ws_floats), _p(plan.ws_doubles), _p(gscale), _p(flat), _stream()),
              "bm_spectral_bwd")
    _timed("spectral_bwd", 0., launch)
    return [flat[off:off + torch.Size(shape).numel()].view(shape) for off, shape in zip(plan.grad_offsets, plan.shapes)]


# ------------------------------------------------------------------------------------------------
# The data loader's batch (csrc/segments.hip, bm/dataset.py:349-364, 263-278, 172-175): windows gathered out of
# recordings that stay resident on the device.
class SegmentTable:
    """The device table of ``bm_segment_gather`` for one array per recording (``[rows_r, n_r]``, fp32 or bool, read in
    place: the table keeps the tensors alive)."""

    def __init__(self, arrays: tp.Sequence[torch.Tensor]):
        L = lib()
        if not arrays:
            raise BmHipError("segment table: no recording")
        self.dtype, self.device = arrays[0].dtype, arrays[0].device
        if self.dtype not in (torch.float32, torch.bool):
            raise BmHipError(f"segment table: fp32 or bool, got {self.dtype}")
        entry = L.bm_segment_table_entry_bytes()
        host = torch.zeros(len(arrays), entry, dtype=torch.uint8)
        for i, a in enumerate(arrays):
            _req(a, f"segment table: recording {i}", self.dtype)
            if a.dim() != 2 or a.device != self.device:
                raise BmHipError(f"segment table: recording {i} of shape {tuple(a.shape)} on {a.device}")
            check(L.bm_segment_table_fill(ctypes.c_void_p(host[i].data_ptr()), _p(a), a.shape[1], a.shape[0]),
                  "bm_segment_table_fill")
        self.arrays = list(arrays)
        self.table = host.to(self.device)

    def __len__(self) -> int:
        return len(self.arrays)


def segment_gather(table: SegmentTable, rec: torch.Tensor, start: torch.Tensor, first: int, count: int, channels: int,
                   T: int, flag: torch.Tensor, baseline: tp.Optional[tp.Tuple[int, int]] = None,
                   dest: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[count, channels, T]``: segment ``b`` is the window ``start[first + b] ... + T - 1`` of recording
    ``rec[first + b]``, rows beyond the recording's are +0.0.  ``rec`` / ``start``: int32 device arrays (a whole epoch;
    the batch is an offset, nothing is copied).  ``baseline`` = (first, last) window sample, inclusive: the fp64 mean of
    those samples is subtracted (fp32 only).  ``flag``: one int32 on the device, set to 1 when a segment is out of range
    (that segment is +0.0).  ``dest``: write into this contiguous tensor instead of a new one."""
    _req(rec, "segment_gather.rec", torch.int32)
    _req(start, "segment_gather.start", torch.int32)
    _req(flag, "segment_gather.flag", torch.int32)
    if rec.numel() != start.numel() or flag.numel() < 1:
        raise BmHipError("segment_gather: rec and start differ in length, or the flag is empty")
    base0, base1 = (-1, -1) if baseline is None else (int(baseline[0]), int(baseline[1]))
    if dest is None:
        dest = torch.empty(count, channels, T, device=table.device, dtype=table.dtype)
    else:
        _req(dest, "segment_gather.dest", table.dtype)
        if tuple(dest.shape) != (count, channels, T):
            raise BmHipError(f"segment_gather: dest is {tuple(dest.shape)}, the batch is {(count, channels, T)}")
        _touched(dest)

    def launch():
        check(lib().bm_segment_gather(_p(table.table), len(table), _p(rec), _p(start), rec.numel(), first, count,
                                      channels, T, base0, base1, dest.element_size(), _p(dest), _p(flag), _stream()),
              "bm_segment_gather")
    _timed("segment_gather", 0., launch)
    return dest


# The batch's features from resident events (csrc/features.hip, bm/features/base.py:68-122, 238-267,
# bm/features/audio.py:78-83, 211-274).
FEATURE_RULES = {"constant": 0, "resampled": 1, "chunk": 2}


class EventTable:
    """The device tables of ``bm_segment_features``.  ``plan``: one ``(kind slot, rule, first channel, channels, default)``
    per feature, tiling the channels in order; ``n_kinds`` event kinds; ``mask_kind``: the slot whose events make the mask
    (-1: all true).  ``recordings``: per recording ``(kinds, sources)`` -- ``kinds``: per slot None (no event) or
    ``(start, duration, running maximum of start + duration)``, float64 device tensors in painting order; ``sources``: per
    feature None (no event of its kind), a float32 device tensor ``[n, channels]`` (constant) or ``(arrays, er)``: the
    events' ``[channels, L]`` float32 device tensors, read in place, and ``L / duration`` of each.  The table keeps every
    tensor alive."""

    def __init__(self, plan, n_kinds: int, mask_kind: int, recordings, device):
        L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise BmHipError("event table: the events are not on a GPU; the features builder is a HIP kernel and has no "
                             "CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_features, self.n_kinds, self.mask_kind = len(plan), int(n_kinds), int(mask_kind)
        self.feat_table = np.ascontiguousarray([[p[0], FEATURE_RULES.get(p[1], p[1]), p[2], p[3]] for p in plan],
                                               dtype=np.int32).reshape(-1, 4)
        self.feat_default = np.ascontiguousarray([p[4] for p in plan], dtype=np.float32)
        self.channels = int(sum(p[3] for p in plan))
        kb, sb, ab = (L.bm_features_table_entry_bytes(i) for i in range(3))
        R = len(recordings)
        kinds = torch.zeros(R, max(self.n_kinds, 1), kb, dtype=torch.uint8)
        srcs = torch.zeros(R, max(self.n_features, 1), sb, dtype=torch.uint8)
        self.keep: tp.List[tp.Any] = []
        for r, (rec_kinds, rec_sources) in enumerate(recordings):
            if len(rec_kinds) != self.n_kinds or len(rec_sources) != self.n_features:
                raise BmHipError(f"event table: recording {r} has {len(rec_kinds)} kinds and {len(rec_sources)} sources")
            counts = []
            for k, triple in enumerate(rec_kinds):
                n = 0
                if triple is not None:
                    for t in triple:
                        _req(t, f"event table: recording {r}, kind {k}", torch.float64)
                    n = triple[0].numel()
                    if any(t.numel() != n or t.device != self.device for t in triple):
                        raise BmHipError(f"event table: recording {r}, kind {k}: the event arrays differ in length")
                    self.keep.append(triple)
                start, dur, runmax = triple if n else (None, None, None)
                check(L.bm_features_kind_fill(ctypes.c_void_p(kinds[r, k].data_ptr()), _p(start), _p(dur), _p(runmax), n),
                      "bm_features_kind_fill")
                counts.append(n)
            for f, source in enumerate(rec_sources):
                slot, rule, _, dim = (int(v) for v in self.feat_table[f])
                n = counts[slot]
                if n == 0:
                    continue                                    # a null source: the kernel finds no event to read it for
                if rule == 0:
                    _req(source, f"event table: recording {r}, feature {f}")
                    if tuple(source.shape) != (n, dim) or source.device != self.device:
                        raise BmHipError(f"event table: recording {r}, feature {f}: values of shape {tuple(source.shape)} "
                                         f"for {n} events of {dim} channels")
                    data = source
                else:
                    arrays, ers = source
                    if len(arrays) != n or len(ers) != n:
                        raise BmHipError(f"event table: recording {r}, feature {f}: {len(arrays)} arrays for {n} events")
                    host = torch.zeros(n, ab, dtype=torch.uint8)
                    for e, (a, er) in enumerate(zip(arrays, ers)):
                        _req(a, f"event table: recording {r}, feature {f}, event {e}")
                        if a.dim() != 2 or a.shape[0] != dim or a.device != self.device:
                            raise BmHipError(f"event table: recording {r}, feature {f}, event {e}: an array of shape "
                                             f"{tuple(a.shape)} for {dim} channels")
                        check(L.bm_features_array_fill(ctypes.c_void_p(host[e].data_ptr()), _p(a), a.shape[1], float(er)),
                              "bm_features_array_fill")
                    data = host.to(self.device)
                    self.keep.append(arrays)
                self.keep.append(data)
                check(L.bm_features_source_fill(ctypes.c_void_p(srcs[r, f].data_ptr()), _p(data)),
                      "bm_features_source_fill")
        self.n_recordings = R
        self.kinds, self.srcs = kinds.to(self.device), srcs.to(self.device)

    def __len__(self) -> int:
        return self.n_recordings


def segment_features(table: EventTable, rec: torch.Tensor, wstart: torch.Tensor, wdur: torch.Tensor, first: int,
                     count: int, T: int, sample_rate: float, flag: torch.Tensor,
                     dest: tp.Optional[torch.Tensor] = None, dest_mask: tp.Optional[torch.Tensor] = None):
    """``(features [count, F, T] fp32, mask [count, 1, T] bool)`` of the segments ``first ... first + count - 1``: ONE
    launch that writes every element once.  ``rec`` (int32), ``wstart`` / ``wdur`` (float64: the window's start and
    duration in seconds): device arrays of a whole epoch.  ``flag``: one int32 on the device, set to 1 when a recording
    index is out of range (that segment is defaults).  ``dest`` / ``dest_mask``: write into these contiguous tensors."""
    _req(rec, "segment_features.rec", torch.int32)
    _req(wstart, "segment_features.wstart", torch.float64)
    _req(wdur, "segment_features.wdur", torch.float64)
    _req(flag, "segment_features.flag", torch.int32)
    if rec.numel() != wstart.numel() or rec.numel() != wdur.numel() or flag.numel() < 1:
        raise BmHipError("segment_features: rec, wstart and wdur differ in length, or the flag is empty")
    for name, t in (("rec", rec), ("wstart", wstart), ("wdur", wdur), ("flag", flag), ("dest", dest), ("dest_mask", dest_mask)):
        if t is not None and t.device != table.device:                 # an address of another card is not one of this one
            raise BmHipError(f"segment_features: {name} is on {t.device}, the event table on {table.device}")
    F = table.channels
    if dest is None:
        dest = torch.empty(count, F, T, device=table.device, dtype=torch.float32)
    else:
        _req(dest, "segment_features.dest")
        if tuple(dest.shape) != (count, F, T):
            raise BmHipError(f"segment_features: dest is {tuple(dest.shape)}, the batch is {(count, F, T)}")
        _touched(dest)
    if dest_mask is None:
        dest_mask = torch.empty(count, 1, T, device=table.device, dtype=torch.bool)
    else:
        _req(dest_mask, "segment_features.dest_mask", torch.bool)
        if tuple(dest_mask.shape) != (count, 1, T):
            raise BmHipError(f"segment_features: dest_mask is {tuple(dest_mask.shape)}, the batch's is {(count, 1, T)}")

    def launch():
        check(lib().bm_segment_features(ctypes.c_void_p(table.feat_table.ctypes.data),
                                        ctypes.c_void_p(table.feat_default.ctypes.data), table.n_features, table.n_kinds,
                                        table.mask_kind, _p(table.kinds), _p(table.srcs), len(table), _p(rec), _p(wstart),
                                        _p(wdur), rec.numel(), first, count, F, T, float(sample_rate), _p(dest),
                                        _p(dest_mask), _p(flag), _stream()), "bm_segment_features")
    _timed("segment_features", 0., launch)
    return dest, dest_mask


# ------------------------------------------------------------------------------------------------
# The MelSpectrum targets from resident waveforms (csrc/mel.hip, bm/features/audio.py:31-76).  torchaudio is not part
# of this stack: its MelSpectrogram is restated from its documentation (torch.stft with center=True, reflect padding and
# a periodic Hann window of n_fft samples; "normalized" divides by sqrt(sum w^2); |.|^2; the htk filterbank of
# melscale_fbanks with norm=None, f_min = 0, f_max = in_sampling // 2).
MEL_FRAME_TILE = 32            # frames per workgroup for n_fft <= 1024 (``mel_frame_tile``: 16 beyond)
MEL_MIN_NFFT, MEL_MAX_NFFT, MEL_MAX_MELS = 8, 2048, 256
_mel_host_cache: tp.Dict[tp.Any, tp.Any] = {}
_mel_device_cache: tp.Dict[tp.Any, tp.Any] = {}


def mel_frame_tile(n_fft: int) -> int:
    """Frames that one workgroup of ``bm_mel_spectrogram`` owns."""
    return int(lib().bm_mel_frame_tile(int(n_fft)))


def mel_check_limits(n_fft: int, n_mels: int) -> None:
    if not (isinstance(n_fft, int) and MEL_MIN_NFFT <= n_fft <= MEL_MAX_NFFT):
        raise ValueError(f"mel spectrogram: n_fft = {n_fft}; the kernel takes {MEL_MIN_NFFT} <= n_fft <= {MEL_MAX_NFFT}")
    if n_fft % 4:
        raise ValueError(f"mel spectrogram: n_fft = {n_fft} is not a multiple of 4 (hop_length = n_fft // 4)")
    if not (isinstance(n_mels, int) and 1 <= n_mels <= MEL_MAX_MELS):
        raise ValueError(f"mel spectrogram: n_mels = {n_mels}; the kernel takes 1 <= n_mels <= {MEL_MAX_MELS}")


def mel_filterbank(n_fft: int, n_mels: int, in_sampling: int):
    """``(fb, lo, hi)``: ``melscale_fbanks(n_fft // 2 + 1, 0, in_sampling // 2, n_mels, in_sampling, norm=None,
    mel_scale="htk")`` evaluated in fp64 and rounded once -- ``fb`` [n_fft // 2 + 1, n_mels] fp32 (CPU) -- and the bins
    ``[lo[m], hi[m])`` that hold every non-zero weight of filter ``m`` (int32; ``lo == hi``: an all-zero filter, the
    case torchaudio warns about).  Cached."""
    key = ("fb", int(n_fft), int(n_mels), int(in_sampling))
    hit = _mel_host_cache.get(key)
    if hit is None:
        mel_check_limits(n_fft, n_mels)
        if int(in_sampling) < 2:
            raise ValueError(f"mel spectrogram: in_sampling = {in_sampling}")
        n_freqs = n_fft // 2 + 1
        f_max = float(int(in_sampling) // 2)
        all_freqs = np.linspace(0., f_max, n_freqs)
        m_pts = np.linspace(0., 2595. * np.log10(1. + f_max / 700.), n_mels + 2)
        f_pts = 700. * (10. ** (m_pts / 2595.) - 1.)
        f_diff = f_pts[1:] - f_pts[:-1]
        slopes = f_pts[None, :] - all_freqs[:, None]
        fb64 = np.maximum(0., np.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))
        fb = fb64.astype(np.float32)
        lo, hi = np.zeros(n_mels, np.int32), np.zeros(n_mels, np.int32)
        for m in range(n_mels):
            nz = np.flatnonzero(fb[:, m])
            if len(nz):
                lo[m], hi[m] = nz[0], nz[-1] + 1
        hit = _mel_host_cache[key] = (torch.from_numpy(fb), torch.from_numpy(lo), torch.from_numpy(hi))
    return hit


def mel_basis(n_fft: int, normalized: bool) -> torch.Tensor:
    """The DFT basis of the kernel, ``[n_fft, 2 * (n_fft // 2 + 1)]`` fp32 (CPU): column ``b`` is ``w[k] cos(2 pi k b /
    n_fft) / norm``, column ``n_fft // 2 + 1 + b`` is ``-w[k] sin(2 pi k b / n_fft) / norm`` -- ``w`` the periodic Hann
    window, ``norm = sqrt(sum w^2)`` when ``normalized`` else 1 -- evaluated in fp64, rounded once.  Cached."""
    key = ("basis", int(n_fft), bool(normalized))
    hit = _mel_host_cache.get(key)
    if hit is None:
        mel_check_limits(n_fft, 1)
        k = np.arange(n_fft, dtype=np.int64)
        w = 0.5 - 0.5 * np.cos(2. * np.pi * k / n_fft)
        norm = np.sqrt(np.sum(w * w)) if normalized else 1.
        angle = 2. * np.pi * ((k[:, None] * np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]) % n_fft) / n_fft
        basis = np.concatenate([w[:, None] * np.cos(angle), -w[:, None] * np.sin(angle)], axis=1) / norm
        hit = _mel_host_cache[key] = torch.from_numpy(basis.astype(np.float32))
    return hit


def _mel_device_tables(n_fft, n_mels, in_sampling, normalized, device):
    """(basis [n_fft, 2 nbp] with the bins padded to a multiple of 16, nbp, fbw [n_mels, n_freqs], range [n_mels, 2] on
    the device, the same range on the host), cached per device."""
    n_freqs = n_fft // 2 + 1
    nbp = (n_freqs + 15) // 16 * 16
    kb = ("basis", n_fft, bool(normalized), device)
    basis = _mel_device_cache.get(kb)
    if basis is None:
        host = mel_basis(n_fft, normalized)
        padded = torch.zeros(n_fft, 2, nbp, dtype=torch.float32)
        padded[:, 0, :n_freqs], padded[:, 1, :n_freqs] = host[:, :n_freqs], host[:, n_freqs:]
        basis = _mel_device_cache[kb] = padded.reshape(n_fft, 2 * nbp).to(device)
    kf = ("fb", n_fft, n_mels, int(in_sampling), device)
    fb = _mel_device_cache.get(kf)
    if fb is None:
        w, lo, hi = mel_filterbank(n_fft, n_mels, in_sampling)
        rng = torch.stack([lo, hi], dim=1).contiguous()
        fb = _mel_device_cache[kf] = (w.t().contiguous().to(device), rng.to(device), rng.numpy())
    return (basis, nbp) + fb


# The wave table (csrc/bm_wave.h): what mel_spectrograms, resample_frac, yin_pitch and wave_moments share before they launch.
WAVE_MAX_WAVES = 65535
_wave_ticket_cache: tp.Dict[tp.Any, torch.Tensor] = {}


def _wave_list(waves, what, wrong=lambda L: None):
    """The waveforms as a checked list.  The limits come first -- they need no device: at most 65535 waveforms, each of
    ``1 <= L < 2^31`` samples with nothing ``wrong(L)`` (the caller's own limit in words) -- then fp32, 1-D, one device."""
    waves = list(waves)
    if len(waves) > WAVE_MAX_WAVES:
        raise ValueError(f"{what}: {len(waves)} waveforms in one call, the limit is {WAVE_MAX_WAVES}")
    for i, x in enumerate(waves):
        if isinstance(x, torch.Tensor) and x.dim() == 1:
            L = x.numel()
            why = wrong(L) if 1 <= L < 2 ** 31 else "the kernels take 1 <= L < 2^31"
            if why is not None:
                raise ValueError(f"{what}: waveform {i} has {L} samples; {why}")
    for i, x in enumerate(waves):
        _req(x, f"{what}: waveform {i}")
        if x.dim() != 1 or x.device != waves[0].device:
            raise BmHipError(f"{what}: waveform {i} of shape {tuple(x.shape)} on {x.device}; expected 1-D waveforms on one "
                             "device")
    return waves


def _wave_batch(waves, what, out_shape=None, wrong=lambda L: None):
    """``(waves, outs, table, lengths)`` of one launch over a wave table: the checked list (``_wave_list``); with
    ``out_shape`` the fp32 output of shape ``out_shape(L)`` of every waveform, all carved from ONE allocation; the device
    table (a host buffer and one copy: no launch); the lengths on the host.  No waveform: ``([], [], None, None)``."""
    waves = _wave_list(waves, what, wrong)
    if not waves:
        return waves, [], None, None
    L, device = lib(), waves[0].device
    outs = []
    if out_shape is not None:
        shapes = [out_shape(x.numel()) for x in waves]
        sizes = [math.prod(shape) for shape in shapes]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=device)
        outs = [piece.view(shape) for piece, shape in zip(flat.split(sizes), shapes)]
    entry = L.bm_wave_table_entry_bytes()
    host = torch.zeros(len(waves), entry, dtype=torch.uint8)
    for i, x in enumerate(waves):
        check(L.bm_wave_table_fill(host.data_ptr() + i * entry, _p(x), x.numel(), _p(outs[i]) if outs else None),
              "bm_wave_table_fill")
    return waves, outs, host.to(device), np.ascontiguousarray([x.numel() for x in waves], dtype=np.int64)


def _wave_moments(table, lengths, device) -> torch.Tensor:
    n = len(lengths)
    max_splits = max(int(lib().bm_wave_moments_splits(int(v))) for v in lengths)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    tickets = _wave_ticket_cache.get(key)       # zeroed counters of this stream: a launch leaves them at zero (csrc/bm_block.h)
    if tickets is None or tickets.numel() < n:
        tickets = _wave_ticket_cache[key] = torch.zeros(max(n, 1024), dtype=torch.int32, device=device)
    part = torch.empty(n, max_splits, 2, dtype=torch.float64, device=device)
    mom = torch.empty(n, 2, dtype=torch.float64, device=device)

    def launch():
        check(lib().bm_wave_moments(_p(table), ctypes.c_void_p(lengths.ctypes.data), n, _p(tickets), _p(part), max_splits,
                                    _p(mom), _stream()), "bm_wave_moments")
    _timed("wave_moments", 0., launch)
    return mom


def _moments_arg(moments, n: int, device, what: str) -> torch.Tensor:
    _req(moments, f"{what}: moments", torch.float64)
    if tuple(moments.shape) != (n, 2) or moments.device != device:
        raise BmHipError(f"{what}: moments of shape {tuple(moments.shape)} on {moments.device}; expected [{n}, 2] on {device}")
    return moments


def wave_moments(waves: tp.Sequence[torch.Tensor]) -> torch.Tensor:
    """``[n, 2]`` float64 on the device: ``(mean, 1 / (1e-8 + unbiased std))`` of every 1-D fp32 device waveform, in fp64,
    ONE launch for all of them and no host read-back -- the ``(shift, scale)`` of MelSpectrum's ``norm_audio``."""
    waves, _, table, lengths = _wave_batch(waves, "wave_moments")
    if not waves:
        raise BmHipError("wave_moments: no waveform")
    return _wave_moments(table, lengths, waves[0].device)


def mel_spectrograms(waves: tp.Sequence[torch.Tensor], n_mels: int = 40, n_fft: int = 512, in_sampling: int = 16_000,
                     normalized: bool = True, use_log_scale: bool = True, log_scale_eps: float = 1e-5,
                     norm_audio: bool = True, moments: tp.Optional[torch.Tensor] = None) -> tp.List[torch.Tensor]:
    """What ``MelSpectrum._compute`` (bm/features/audio.py:61-76) returns for every mono waveform at ``in_sampling``:
    a list of ``[n_mels, 1 + L // (n_fft // 4)]`` fp32 tensors, carved from one allocation.  ``waves``: 1-D fp32 device
    tensors, read in place (4-byte alignment is all that is assumed).  Two launches for the whole list (one with
    ``norm_audio=False``): the statistics, then framing, reflect padding, window, DFT, power, filterbank and log.
    ``moments`` (``[n, 2]`` float64 on the device, ``(shift, scale)`` per waveform): used as they are instead of the
    statistics launch, whatever ``norm_audio`` says -- waveforms that were normalised before they were resampled."""
    mel_check_limits(n_fft, n_mels)
    hop = n_fft // 4
    waves, outs, table, lengths = _wave_batch(
        waves, "mel_spectrograms", out_shape=lambda L: (n_mels, 1 + L // hop),
        wrong=lambda L: f"the reflect padding needs L > n_fft // 2 = {n_fft // 2}" if L <= n_fft // 2 else None)
    if not waves:
        return []
    device = waves[0].device
    basis, nbp, fbw, rng, rng_host = _mel_device_tables(n_fft, n_mels, in_sampling, normalized, device)
    if moments is not None:
        mom = _moments_arg(moments, len(waves), device, "mel_spectrograms")
    else:
        mom = _wave_moments(table, lengths, device) if norm_audio else None

    def launch():
        check(lib().bm_mel_spectrogram(_p(table), ctypes.c_void_p(lengths.ctypes.data), len(waves), _p(mom), _p(basis),
                                       n_fft, nbp, _p(fbw), _p(rng), ctypes.c_void_p(rng_host.ctypes.data), n_mels,
                                       int(bool(use_log_scale)), float(log_scale_eps), _stream()), "bm_mel_spectrogram")
    _timed("mel_spectrogram", 4. * n_fft * nbp * sum(o.shape[1] for o in outs), launch)
    return outs


# ------------------------------------------------------------------------------------------------
# julius.resample.ResampleFrac over resident waveforms (csrc/resample.hip; bm/features/audio.py:66, 113, 186).  julius is
# not part of this stack: the filter is restated from its published definition, with julius' own fp32 torch expressions.
RESAMPLE_MAX_NEW, RESAMPLE_MAX_SPAN = 4096, 16384      # phases; floats of LDS that 16 frames cover: 15 old + ntaps (to 4)
_resample_taps: tp.Dict[tp.Any, tp.Any] = {}


def resample_ratio(old_sr: int, new_sr: int) -> tp.Tuple[int, int]:
    """``(old, new)``: the two rates divided by their gcd.  Integer rates of at least 1 Hz, else ``ValueError``."""
    for name, sr in (("old_sr", old_sr), ("new_sr", new_sr)):
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr < 1:
            raise ValueError(f"resample: {name} = {sr!r}; the rates are integers of at least 1 Hz")
    g = math.gcd(int(old_sr), int(new_sr))
    return int(old_sr) // g, int(new_sr) // g


def resample_check_limits(old: int, new: int, width: int) -> None:
    """``ValueError`` naming the limit that the reduced ratio ``old / new`` with ``width`` is outside of."""
    ntp = (2 * width + old + 3) // 4 * 4
    if new > RESAMPLE_MAX_NEW:
        raise ValueError(f"resample: {new} phases (new_sr / gcd); the kernel takes at most {RESAMPLE_MAX_NEW}")
    if 15 * old + ntp > RESAMPLE_MAX_SPAN:
        raise ValueError(f"resample: ratio {old} / {new} with {2 * width + old} taps: 16 frames cover 15 * old + ntaps = "
                         f"{15 * old + ntp} samples, the LDS span holds at most {RESAMPLE_MAX_SPAN}")


def resample_taps(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945, device=None):
    """``(taps, old, new, width)``: the ``[new, 2 * width + old]`` fp32 table of julius' ``ResampleFrac(old_sr, new_sr,
    zeros, rolloff)`` -- phase ``i`` is a sinc at ``min(old, new) * rolloff`` under a ``cos^2`` window of ``zeros`` zero
    crossings, normalised to a sum of 1 -- computed on the CPU with julius' own fp32 torch expressions.  With ``device``
    the first element is the kernel's table instead: ``[ntaps to a multiple of 4, new to a multiple of 16]`` on that
    device, tap-major, zero-padded.  Cached per (old, new, zeros, rolloff, device).  ``old == new``: ``ValueError`` (the
    identity has no filter)."""
    old, new = resample_ratio(old_sr, new_sr)
    if old == new:
        raise ValueError(f"resample: {old_sr} Hz -> {new_sr} Hz is the identity; it has no filter")
    if isinstance(zeros, bool) or not isinstance(zeros, int) or zeros < 1:
        raise ValueError(f"resample: zeros = {zeros!r}; a positive integer")
    if not 0. < float(rolloff) <= 1.:
        raise ValueError(f"resample: rolloff = {rolloff!r}; 0 < rolloff <= 1")
    device = torch.device(device) if device is not None else None
    key = (old, new, zeros, float(rolloff), device)
    hit = _resample_taps.get(key)
    if hit is not None:
        return hit
    sr = min(old, new) * rolloff
    width = math.ceil(zeros * old / sr)
    resample_check_limits(old, new, width)
    if device is not None:
        taps = resample_taps(old_sr, new_sr, zeros, rolloff)[0]
        ntaps = taps.shape[1]
        packed = torch.zeros((ntaps + 3) // 4 * 4, (new + 15) // 16 * 16, dtype=torch.float32)
        packed[:ntaps, :new] = taps.t()
        hit = (packed.to(device), old, new, width)
    else:
        idx = torch.arange(-width, width + old).float()
        rows = []
        for i in range(new):
            t = (-i / new + idx / old) * sr
            t.clamp_(-zeros, zeros)
            t *= math.pi
            window = torch.cos(t / zeros / 2) ** 2
            kernel = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window
            kernel.div_(kernel.sum())
            rows.append(kernel)
        taps = torch.stack(rows)
        assert taps.dtype == torch.float32 and tuple(taps.shape) == (new, 2 * width + old)
        hit = (taps, old, new, width)
    if len(_resample_taps) >= 64:
        _resample_taps.clear()
    _resample_taps[key] = hit
    return hit


def resample_length(length: int, old: int, new: int) -> int:
    """``floor(new * length / old)`` in integers (julius forms it through a default-dtype tensor)."""
    return new * int(length) // old


def resample_frames_tile(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945) -> int:
    """julius frames (``new`` outputs each, ``old`` inputs apart) that one workgroup of ``bm_resample_frac`` owns."""
    _, old, new, width = resample_taps(old_sr, new_sr, zeros, rolloff)
    return int(lib().bm_resample_frames_tile(old, new, width))


def resample_frac(waves: tp.Sequence[torch.Tensor], old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945,
                  moments: tp.Optional[torch.Tensor] = None) -> tp.List[torch.Tensor]:
    """``julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff)(wave)`` for every 1-D fp32 device waveform, all at
    ``old_sr``: a list of 1-D fp32 tensors of ``floor(new * L / old)`` samples, carved from one allocation, ONE launch
    (``bm_resample_frac``).  Equal rates return the waveforms themselves, as julius does.  ``moments`` (``[n, 2]``
    float64 on the device, what ``wave_moments`` gives): every sample enters as ``(x - mean) * inv`` in fp64, rounded once
    -- the reference normalises at the source rate.  Limits (``ValueError`` before any launch): ``new <= 4096`` phases,
    ``15 * old + ntaps <= 16384`` staged samples, ``L < 2^31`` in and out, 65535 waveforms."""
    old, new = resample_ratio(old_sr, new_sr)
    if old == new:
        if moments is not None:
            raise ValueError("resample_frac: equal rates return the waveforms as they are; moments cannot be applied")
        return _wave_list(waves, "resample_frac")
    _, _, _, width = resample_taps(old_sr, new_sr, zeros, rolloff)              # the limits first: they need no device
    waves, outs, table, lengths = _wave_batch(
        waves, "resample_frac", out_shape=lambda L: (resample_length(L, old, new),),
        wrong=lambda L: (f"they give {resample_length(L, old, new)} outputs, the kernel takes fewer than 2^31"
                         if resample_length(L, old, new) >= 2 ** 31 else None))
    if not waves:
        return []
    device = waves[0].device
    taps = resample_taps(old_sr, new_sr, zeros, rolloff, device)[0]
    mom = _moments_arg(moments, len(waves), device, "resample_frac") if moments is not None else None

    def launch():
        check(lib().bm_resample_frac(_p(table), ctypes.c_void_p(lengths.ctypes.data), len(waves), _p(mom), _p(taps), old,
                                     new, width, _stream()), "bm_resample_frac")
    _timed("resample_frac", 2. * (2 * width + old) * sum(o.numel() for o in outs), launch)
    return outs


def resample_rows(x: torch.Tensor, old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945) -> torch.Tensor:
    """``julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff)(x)`` for a ``[C, L]`` fp32 device tensor (the
    channels of a recording): a contiguous ``[C, floor(new * L / old)]``.  The rows are the waveforms of ONE
    ``resample_frac`` launch (rows of unit stride are read in place, whatever lies between them), whose outputs, carved
    from one allocation, are the result: the same bits as ``resample_frac`` over the rows, the same limits.  Equal rates
    return ``x`` itself, as julius does."""
    old, new = resample_ratio(old_sr, new_sr)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"resample_rows: expected [channels, samples], got {tuple(getattr(x, 'shape', ()))}")
    if old == new:
        return x
    C, L = x.shape
    if C and L != 1 and x.stride(1) != 1:
        x = x.contiguous()
    n = resample_length(L, old, new)
    outs = resample_frac(list(x.unbind(0)), old_sr, new_sr, zeros, rolloff)
    if not outs:
        return torch.empty(0, n, dtype=torch.float32, device=x.device)
    return outs[0].as_strided((C, n), (n, 1))                   # the one allocation behind the outputs


# The Pitch feature (csrc/pitch.hip; bm/features/audio.py:110-124, bm/lib/pitch_calc/yin.py).
YIN_MAX_WLEN, YIN_MAX_WSTEP = 1024, 512


def yin_taus(sr: float, w_len: int, w_step: int, f0_min: float, f0_max: float) -> tp.Tuple[int, int]:
    """``(tau_min, tau_max) = (int(sr / f0_max), int(sr / f0_min))`` behind every limit's ``ValueError``."""
    if not (isinstance(w_len, int) and 2 <= w_len <= YIN_MAX_WLEN):
        raise ValueError(f"yin_pitch: w_len = {w_len!r}; the kernel takes 2 <= w_len <= {YIN_MAX_WLEN}")
    if not (isinstance(w_step, int) and 1 <= w_step <= YIN_MAX_WSTEP):
        raise ValueError(f"yin_pitch: w_step = {w_step!r}; the kernel takes 1 <= w_step <= {YIN_MAX_WSTEP}")
    if not (sr > 0 and f0_min > 0 and f0_max > 0):
        raise ValueError(f"yin_pitch: sr = {sr}, f0_min = {f0_min}, f0_max = {f0_max}; all three are positive")
    tau_min, tau_max = int(sr / f0_max), int(sr / f0_min)
    if tau_min < 1:
        raise ValueError(f"yin_pitch: tau_min = int(sr / f0_max) = {tau_min}; f0_max = {f0_max} is above sr = {sr}")
    if tau_max > w_len:
        raise ValueError(f"yin_pitch: tau_max = int(sr / f0_min) = {tau_max} is above w_len = {w_len}")
    return tau_min, tau_max


def yin_frames(length: int, w_len: int, w_step: int) -> int:
    return len(range(0, int(length) - w_len, w_step))


def yin_pitch(waves: tp.Sequence[torch.Tensor], sr: float = 16_000, w_len: int = 256, w_step: int = 64,
              harmo_thresh: float = 0.1, f0_min: float = 100.0, f0_max: float = 350.0) -> tp.List[torch.Tensor]:
    """The ``pitches`` of ``compute_yin(sig, sr, w_len, w_step, f0_min, f0_max, harmo_thresh)`` for every 1-D fp32 device
    waveform: a list of ``[1, len(range(0, L - w_len, w_step))]`` fp32 tensors carved from one allocation, ONE launch
    (``bm_yin_pitch``): the difference function as a direct fp64 sum, its cumulative mean normalisation, the first dip
    under the threshold walked to its bottom, ``sr / tau``; 0.0 for an unvoiced, a silent or a non-finite frame.
    ``ValueError``: ``L <= w_len``, ``tau_max > w_len``, ``tau_min < 1``, ``w_len > 1024``, ``w_step > 512``."""
    tau_min, tau_max = yin_taus(sr, w_len, w_step, f0_min, f0_max)
    waves, outs, table, lengths = _wave_batch(
        waves, "yin_pitch", out_shape=lambda L: (1, yin_frames(L, w_len, w_step)),
        wrong=lambda L: f"a frame needs L > w_len = {w_len}" if L <= w_len else None)
    if not waves:
        return []

    def launch():
        check(lib().bm_yin_pitch(_p(table), ctypes.c_void_p(lengths.ctypes.data), len(waves), float(sr), w_len, w_step,
                                 tau_min, tau_max, float(harmo_thresh), _stream()), "bm_yin_pitch")
    _timed("yin_pitch", 3. * w_len * tau_max * sum(o.shape[1] for o in outs), launch)
    return outs


# The word label of every kept test segment (csrc/wer.hip, bm/wer.py:48, 58-66).
WORD_HASH_ALL_ZERO_BIT = 1      # every candidate of a kept row is zero: the assert of bm/wer.py:65
WORD_HASH_VALUE_BIT = 2         # the chosen value is not finite, not an integer, or |v| >= 2^63
WORD_HASH_DEST_BIT = 4          # a kept row had no element of dest left


def _labels_shape_check(name: str, reach: int, cite: str, cols: tp.Optional[int], shape: tp.Sequence[int], c: int,
                        check_at_time: int, dest, n0: int, count: tp.Optional[int]) -> None:
    """The shape checks of the two label launches (``word_hash_pick``: ``reach`` 2, ``dest`` = its number of labels,
    ``cols`` None; ``segment_eval_labels``: ``reach`` 1, ``dest`` = its shape, ``[rows, cols]``), in one order: the
    features, ``check_at_time`` (``cite``: the reference's lines that would wrap around), the channel, the shape of
    ``dest``, ``count``, the room in ``dest``."""
    if len(shape) != 3:
        raise ValueError(f"{name}: the features are {tuple(shape)}, expected [B, F_all, T]")
    B, F, T = (int(s) for s in shape)
    if check_at_time < 0 or check_at_time + reach >= T:
        raise ValueError(f"{name}: check_at_time = {check_at_time} reads the samples {check_at_time - reach} .. "
                         f"{check_at_time + reach} of a window of {T} ({cite} would wrap around or raise IndexError)")
    if not 0 <= c < F:
        raise ValueError(f"{name}: channel {c} of {F}")
    rows, unit = dest, "labels"
    if cols is not None:
        if len(dest) != 2 or int(dest[1]) != cols:
            raise ValueError(f"{name}: dest is {tuple(dest)}, expected [rows, {cols}]")
        rows, unit = int(dest[0]), "rows"
    count = B if count is None else int(count)
    if not 0 <= count <= B:
        raise ValueError(f"{name}: {count} kept rows of a batch of {B}")
    if n0 < 0 or n0 + count > rows:
        raise ValueError(f"{name}: dest holds {rows} {unit}, the batch writes {n0} .. {n0 + count - 1}")


def _labels_tensor_check(name: str, features: torch.Tensor, dest: torch.Tensor, flag: torch.Tensor,
                         reject_mask: tp.Optional[torch.Tensor]) -> None:
    """What the two label launches ask of their tensors, behind the shape checks."""
    _req(features, f"{name}.features")
    _req(dest, f"{name}.dest", torch.int64)
    _req(flag, f"{name}.flag", torch.int32)
    if reject_mask is not None:
        _req(reject_mask, f"{name}.reject_mask", torch.bool)
        if reject_mask.shape != (features.shape[0],):
            raise ValueError(f"{name}: reject_mask is {tuple(reject_mask.shape)} for a batch of {features.shape[0]}")


def word_hash_pick_check(shape: tp.Sequence[int], c: int, check_at_time: int, n_dest: int, n0: int = 0,
                         count: tp.Optional[int] = None) -> None:
    """The ``ValueError``s of ``word_hash_pick``, from the shapes alone (nothing is launched, no tensor is touched):
    features that are not ``[B, F_all, T]``; ``check_at_time < 0`` or ``check_at_time + 2 >= T`` (the reference's
    ``word_hash[:, check_at_time + 2]`` would wrap around or raise ``IndexError``); ``c`` outside ``[0, F_all)``; a
    negative ``n0``; a ``dest`` with fewer than ``n0 + count`` elements (``count``: the kept rows when the caller knows
    them, else all ``B``)."""
    _labels_shape_check("word_hash_pick", 2, "bm/wer.py:58-64", None, shape, c, check_at_time, n_dest, n0, count)


def word_hash_pick(features: torch.Tensor, c: int, check_at_time: int, reject_mask: tp.Optional[torch.Tensor],
                   dest: torch.Tensor, n0: int, flag: torch.Tensor, count: tp.Optional[int] = None) -> None:
    """``dest[n0 + r]`` = the word label of the kept row of rank ``r`` of the batch's full ``features`` ``[B, F_all, T]``
    (fp32, contiguous, read in place): the first non-zero of channel ``c`` at ``check_at_time``, ``- 1`` (only if
    ``check_at_time > 0``), ``+ 1``, ``- 2`` (only if ``> 1``), ``+ 2``, as the exact int64 of the fp32 value -- the
    ``torch.where`` chain of bm/wer.py:58-64 over ``word_hash[reject_mask]``, ONE launch (``bm_word_hash_pick``).
    ``reject_mask``: bool ``[B]`` (true = kept) or None (all kept); ``dest``: int64, contiguous; ``flag``: one int32 on
    the device, see the ``WORD_HASH_*_BIT``s; ``count``: the number of kept rows when the caller knows it (it only
    tightens the length check of ``dest``).  ``ValueError``s: ``word_hash_pick_check``, before any launch."""
    if not isinstance(features, torch.Tensor) or not isinstance(dest, torch.Tensor):
        raise BmHipError("word_hash_pick: features and dest are tensors")
    word_hash_pick_check(features.shape, c, check_at_time, dest.numel(), n0, count)
    _labels_tensor_check("word_hash_pick", features, dest, flag, reject_mask)
    B, F, T = features.shape
    if dest.dim() != 1 or flag.numel() < 1:
        raise ValueError("word_hash_pick: dest is one-dimensional and the flag holds one word")

    def launch():
        check(lib().bm_word_hash_pick(_p(features), B, F, T, int(c), int(check_at_time), _p(reject_mask), _p(dest),
                                      dest.numel(), int(n0), _p(flag), _stream()), "bm_word_hash_pick")
    _timed("word_hash_pick", 0., launch)


# The labels of the segment-level evaluation (csrc/segment_eval.hip, scripts/run_eval_probs.py:27-57, 105-158).
SEGMENT_EVAL_COLUMNS = ("word_hash", "word_index", "sequence_id", "segment_id", "subject_index", "recording_index",
                        "word_event")
SEGMENT_EVAL_VALUE_BIT = 1      # the word hash is not finite, not an integer, or |v| >= 2^63
SEGMENT_EVAL_DEST_BIT = 2       # a kept row had no row of dest left
SEGMENT_EVAL_RANGE_BIT = 4      # a recording index outside the tables (the row gets the no-word values)
FIRST_OCCURRENCE_RANGE_BIT = 8  # an id outside [0, n_ids) (the row is masked out)


class WordInfoTable:
    """The device table of ``bm_segment_eval_labels`` for the word information: per recording None (it is not part of
    the evaluated set) or an int64 array ``[n_words, 3]`` = ``(word_index, sequence_id, segment_id)`` in the order of the
    recording's word events (a numpy array or a tensor; uploaded once, the table keeps it alive).  ``n_ids``: segment ids
    are in ``[0, n_ids)``, 0 = no word."""

    def __init__(self, rows: tp.Sequence[tp.Any], n_ids: int, device):
        L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise BmHipError("word-info table: not on a GPU; the evaluation's labels are a HIP kernel and have no CPU "
                             "fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        entry = L.bm_segment_eval_info_entry_bytes()
        host = torch.zeros(max(len(rows), 1), entry, dtype=torch.uint8)
        self.arrays: tp.List[tp.Optional[torch.Tensor]] = []
        for r, a in enumerate(rows):
            if a is None:
                self.arrays.append(None)
                continue
            a = torch.as_tensor(a)
            if a.dim() != 2 or a.shape[1] != 3 or a.dtype != torch.int64:
                raise BmHipError(f"word-info table: recording {r}: {a.dtype} of shape {tuple(a.shape)}, expected int64 "
                                 "[n_words, 3]")
            a = a.to(self.device).contiguous()
            check(L.bm_segment_eval_info_fill(ctypes.c_void_p(host[r].data_ptr()), _p(a) if a.numel() else None,
                                              a.shape[0]), "bm_segment_eval_info_fill")
            self.arrays.append(a)
        self.n_recordings, self.n_ids = len(rows), int(n_ids)
        self.table = host.to(self.device)

    def __len__(self) -> int:
        return self.n_recordings


def segment_eval_labels_check(shape: tp.Sequence[int], c: int, check_at_time: int, dest_shape: tp.Sequence[int],
                              n0: int = 0, count: tp.Optional[int] = None) -> None:
    """The ``ValueError``s of ``segment_eval_labels`` that come from the shapes alone (nothing is launched, no tensor is
    touched): features that are not ``[B, F_all, T]``; ``check_at_time < 0`` or ``check_at_time + 1 >= T`` (the
    reference's ``word_hash[:, check_at_time + 1]`` would wrap around or raise ``IndexError``); ``c`` outside
    ``[0, F_all)``; a ``dest`` that is not ``[rows, 7]``; a negative ``n0``; fewer than ``n0 + count`` rows (``count``:
    the kept rows when the caller knows them, else all ``B``)."""
    _labels_shape_check("segment_eval_labels", 1, "scripts/run_eval_probs.py:116-130", len(SEGMENT_EVAL_COLUMNS), shape, c,
                        check_at_time, dest_shape, n0, count)


def segment_eval_labels(features: torch.Tensor, c: int, check_at_time: int, reject_mask: tp.Optional[torch.Tensor],
                        arrays: tp.Mapping[str, torch.Tensor], first: int, events: "EventTable", word_kind: int,
                        infos: WordInfoTable, sample_rate: float, dest: torch.Tensor, n0: int, flag: torch.Tensor,
                        count: tp.Optional[int] = None) -> None:
    """``dest[n0 + r]`` = the seven labels (``SEGMENT_EVAL_COLUMNS``) of the kept row of rank ``r`` of the batch whose
    full ``features`` ``[B, F_all, T]`` (fp32, contiguous, read in place) were built for the segments ``first ... first +
    B - 1`` of the epoch's ``arrays`` (``DeviceSegmentLoader.epoch_arrays``: ``rec``, ``wstart``, ``subject_index``,
    ``recording_index``): ``_get_extra_info`` and scripts/run_eval_probs.py:105-130, 155-158 as ONE launch
    (``bm_segment_eval_labels``).  ``events``: the segments' ``EventTable``, ``word_kind`` the slot of its word events;
    ``infos``: the ``WordInfoTable`` of the evaluated set; ``dest``: int64 ``[rows, 7]``, contiguous; ``flag``: one int32
    on the device, see the ``SEGMENT_EVAL_*_BIT``s.  ``ValueError``s (``segment_eval_labels_check``, and events without
    words or word information) before any launch."""
    if not isinstance(features, torch.Tensor) or not isinstance(dest, torch.Tensor):
        raise BmHipError("segment_eval_labels: features and dest are tensors")
    segment_eval_labels_check(features.shape, c, check_at_time, dest.shape, n0, count)
    if events is None or infos is None:
        raise ValueError("segment_eval_labels: the segments carry no events or no word information (word_index / "
                         "sequence_id columns of the word events)")
    if not 0 <= word_kind < events.n_kinds:
        raise ValueError(f"segment_eval_labels: the word kind {word_kind} of {events.n_kinds} event kinds")
    if len(infos) != len(events):
        raise ValueError(f"segment_eval_labels: word information for {len(infos)} recordings, events for {len(events)}")
    _labels_tensor_check("segment_eval_labels", features, dest, flag, reject_mask)
    B, F, T = features.shape
    rec, wstart = arrays["rec"], arrays["wstart"]
    subject, recording = arrays["subject_index"], arrays["recording_index"]
    _req(rec, "segment_eval_labels.rec", torch.int32)
    _req(wstart, "segment_eval_labels.wstart", torch.float64)
    _req(subject, "segment_eval_labels.subject_index", torch.int64)
    _req(recording, "segment_eval_labels.recording_index", torch.int64)
    n_index = rec.numel()
    if wstart.numel() != n_index or subject.numel() != n_index or recording.numel() != n_index or flag.numel() < 1:
        raise BmHipError("segment_eval_labels: the epoch's arrays differ in length, or the flag is empty")
    if first < 0 or first + B > n_index:
        raise ValueError(f"segment_eval_labels: segments {first} .. {first + B - 1} of an epoch of {n_index}")
    for name, t in (("rec", rec), ("wstart", wstart), ("subject_index", subject), ("recording_index", recording),
                    ("flag", flag), ("dest", dest), ("features", features), ("reject_mask", reject_mask)):
        if t is not None and t.device != events.device:
            raise BmHipError(f"segment_eval_labels: {name} is on {t.device}, the event table on {events.device}")

    def launch():
        check(lib().bm_segment_eval_labels(_p(features), B, F, T, int(c), int(check_at_time), _p(reject_mask), _p(rec),
                                           _p(wstart), _p(subject), _p(recording), n_index, int(first), _p(events.kinds),
                                           events.n_kinds, int(word_kind), _p(infos.table), len(infos),
                                           float(sample_rate), _p(dest), dest.shape[0], int(n0), _p(flag), _stream()),
              "bm_segment_eval_labels")
    _timed("segment_eval_labels", 0., launch)


def first_occurrence(ids: torch.Tensor, n_ids: int, flag: tp.Optional[torch.Tensor] = None):
    """``(mask [N] bool, first_row [N] int32)`` of ``ids`` (int64 ``[N]``, values in ``[0, n_ids)``): ``mask[i]`` is true
    when row ``i`` is the first that carries its id, ``first_row[i]`` is that first row -- the ``seen_segment_hashes``
    loop of scripts/run_eval_probs.py:141-149 over a whole epoch, two launches (``bm_first_occurrence``: an integer
    ``atomicMin`` per row into a table of ``n_ids`` entries, then one compare per row; the same result on every run).
    An id out of range raises ``FIRST_OCCURRENCE_RANGE_BIT`` in ``flag`` (one int32 on the device), its row is masked
    out and its ``first_row`` is -1.  ``N < 2^31``."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
        raise ValueError("first_occurrence: ids is a one-dimensional tensor")
    N = ids.numel()
    if N >= 2 ** 31:
        raise ValueError(f"first_occurrence: {N} rows; N < 2^31")
    if n_ids < 0:
        raise ValueError(f"first_occurrence: n_ids = {n_ids}")
    _req(ids, "first_occurrence.ids", torch.int64)
    if flag is None:
        flag = torch.zeros(1, device=ids.device, dtype=torch.int32)
    _req(flag, "first_occurrence.flag", torch.int32)
    first = torch.full((max(int(n_ids), 1),), 2 ** 31 - 1, device=ids.device, dtype=torch.int32)
    mask = torch.empty(N, device=ids.device, dtype=torch.bool)
    first_row = torch.empty(N, device=ids.device, dtype=torch.int32)

    def launch():
        check(lib().bm_first_occurrence(_p(ids), N, int(n_ids), _p(first), _p(mask), _p(first_row), _p(flag), _stream()),
              "bm_first_occurrence")
    _timed("first_occurrence", 0., launch)
    return mask, first_row
