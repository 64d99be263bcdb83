"""Torch-tensor front end of the C ABI (``include/wan_hip.h``).

Every function takes CUDA(HIP) tensors, validates dtype/layout, and enqueues the
kernel on torch's current stream.  Nothing here computes on the host and nothing
falls back to eager PyTorch: a CPU tensor raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import functools
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import RopeParams

EPI_BF16, EPI_GELU_BF16, EPI_F32, EPI_RESID_F32, EPI_BF16_T = (
    _lib.EPI_BF16, _lib.EPI_GELU_BF16, _lib.EPI_F32, _lib.EPI_RESID_F32, _lib.EPI_BF16_T)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _on_tensor_device(fn):
    """Launch on the device that holds the operands: the kernels take raw pointers, so HIP's current device (and
    torch's current stream, which is per device) must be the tensors' device.  Entering ``torch.cuda.device`` only when
    it differs keeps the common single-device case free of extra calls."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = next((a for a in args if torch.is_tensor(a)), None)
        if t is None and args and isinstance(args[0], (list, tuple)):       # lincomb: list of (coefficient, tensor)
            t = next((x[1] for x in args[0] if isinstance(x, tuple) and torch.is_tensor(x[1])), None)
        if t is not None and t.is_cuda and t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return wrapper


def set_tuning(key: str, value: int) -> None:
    """Developer switch of the library (``wan_set_tuning``, include/wan_hip.h)."""
    _lib.check(_lib.load().wan_set_tuning(key.encode(), int(value)), "wan_set_tuning")


def get_tuning(key: str) -> int:
    return int(_lib.load().wan_get_tuning(key.encode()))


def box_probe(device=None, target_ms: int = 300) -> dict:
    """``wan_box_probe`` (include/wan_hip.h): the fixed calibration workload of the library -- what the matrix pipes of this box hold
    at the power limit under a flash-attention instruction mix, and its plain copy rate.  SYNCHRONISES; a measurement for benchmarks
    (bench.py's `box` object), never part of the product path.  The 512 MiB scratch is allocated here and freed on return."""
    import ctypes
    dev = torch.device(device if device is not None else torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("box_probe needs a GPU")
    lib = _lib.load()
    with torch.cuda.device(dev):
        n = int(lib.wan_box_probe_scratch_bytes())
        scratch = torch.empty(n, device=dev, dtype=torch.uint8)
        res = _lib.BoxProbeResult()
        _lib.check(lib.wan_box_probe(ctypes.byref(res), ctypes.c_void_p(scratch.data_ptr()), n, int(target_ms), _stream()), "wan_box_probe")
        del scratch
    return {"mfma_mix_tflops": round(float(res.mfma_mix_tflops), 1), "copy_tbps": round(float(res.copy_tbps), 3),
            "mfma_ms": round(float(res.mfma_ms), 2), "copy_ms": round(float(res.copy_ms), 2)}


def _need(t: torch.Tensor, dtype, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------
def _ln_modulate_args(who: str, x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                      rows_per_batch: int) -> Tuple[int, int]:
    """The input checks of ``ln_modulate`` and ``ln_modulate_fp8`` (``who``, for the messages) -> (rows, dim)."""
    _need(x, torch.float32, who + ".x")
    if not x.is_contiguous() or x.dim() != 2:
        raise ValueError(f"{who}.x must be a contiguous [rows, dim] tensor")
    rows, dim = x.shape
    for nm, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _need(t, torch.float32, f"{who}.{nm}")
            if not t.is_contiguous() or t.shape[-1] != dim or t.numel() * rows_per_batch < rows * dim:
                raise ValueError(f"{who}.{nm}: shape {tuple(t.shape)} does not cover {rows} rows of {dim}")
    return rows, dim


def _rmsnorm_rope_args(who: str, x0: torch.Tensor, w0: torch.Tensor, x1: Optional[torch.Tensor], w1: Optional[torch.Tensor],
                       head_dim: int, rope, rope_params, outs=(), out_dtype=None):
    """The argument checks of ``rmsnorm_rope_``, ``rmsnorm_rope_sp`` and ``rmsnorm_rope_fp8`` (``who``, for the messages).
    ``outs``: (name, tensor) of the outputs of the two forms that write elsewhere, x0's then x1's.
    -> (rows, dim, ld, cos, sin, reference to rope_params or None)."""
    _need(x0, torch.bfloat16, who + ".x0")
    _need(w0, torch.float32, who + ".w0")
    rows, dim = x0.shape
    ld = x0.stride(0)
    for nm, t in outs:
        if t is not None:
            _need(t, out_dtype, f"{who}.{nm}")
            if not t.is_contiguous() or t.numel() < rows * dim:
                raise ValueError(f"{who}.{nm} must be contiguous with >= rows * dim elements")
    if x1 is not None:
        _need(x1, torch.bfloat16, who + ".x1")
        _need(w1, torch.float32, who + ".w1")
        if x1.shape != x0.shape or x1.stride(0) != ld:
            raise ValueError(f"{who}: x0 and x1 must have the same shape and row stride")
        if outs and outs[1][1] is None:
            raise ValueError(f"{who}: x1 needs {outs[1][0]}")
    cos = sin = None
    if rope is not None:
        cos, sin = rope
        _need(cos, torch.float32, who + ".cos")
        _need(sin, torch.float32, who + ".sin")
        if cos.shape != sin.shape or cos.shape[1] != head_dim // 2 or not (cos.is_contiguous() and sin.is_contiguous()):
            raise ValueError(f"{who}: cos/sin must be contiguous [max_pos, head_dim/2]")
        if rope_params is None:
            raise ValueError(f"{who}: rope tables given without rope_params")
    return rows, dim, ld, cos, sin, (ctypes.byref(rope_params) if rope_params is not None else None)


@_on_tensor_device
def ln_modulate(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                add_one: bool, rows_per_batch: int, eps: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [rows, dim]; scale/shift fp32 [nbatch, dim] or None -> bf16 [rows, dim]."""
    rows, dim = _ln_modulate_args("ln_modulate", x, scale, shift, rows_per_batch)
    if out is None:
        out = torch.empty(rows, dim, device=x.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "ln_modulate.out")
    lib = _lib.load()
    _lib.check(lib.wan_ln_modulate(_p(x), _p(scale), _p(shift), int(bool(add_one)), _p(out), rows, dim,
                                   int(rows_per_batch), float(eps), _stream()), "wan_ln_modulate")
    return out


@_on_tensor_device
def rmsnorm_rope_(x0: torch.Tensor, w0: torch.Tensor, x1: Optional[torch.Tensor], w1: Optional[torch.Tensor],
                  head_dim: int, eps: float, rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  rope_params: Optional[RopeParams] = None, x0_scale: float = 1.0) -> None:
    """In-place RMSNorm(+RoPE) of one or two bf16 [rows, dim] views sharing a row stride.
    ``x0_scale`` multiplies the x0 result before its bf16 rounding (``q_prescale(softmax_scale)`` to
    feed ``attention_fwd(..., q_prescaled=True)``)."""
    rows, dim, ld, cos, sin, rp = _rmsnorm_rope_args("rmsnorm_rope", x0, w0, x1, w1, head_dim, rope, rope_params)
    lib = _lib.load()
    _lib.check(lib.wan_rmsnorm_rope(_p(x0), _p(w0), _p(x1), _p(w1), ld, rows, dim, head_dim, float(eps),
                                    _p(cos), _p(sin), rp, float(x0_scale), _stream()), "wan_rmsnorm_rope")


@_on_tensor_device
def rmsnorm_rope_sp(x0: torch.Tensor, w0: torch.Tensor, x1: Optional[torch.Tensor], w1: Optional[torch.Tensor], head_dim: int,
                    eps: float, rope: Tuple[torch.Tensor, torch.Tensor], rope_params: RopeParams, wire0: torch.Tensor,
                    wire1: Optional[torch.Tensor], slabs: int, batch: int, x0_scale: float = 1.0, split: int = 0) -> None:
    """``rmsnorm_rope_`` that leaves x0 / x1 untouched and writes the results into Ulysses token-major wire buffers
    ``[slabs][rows_per_batch][batch][dim / slabs]`` (include/wan_hip.h, a21).  ``split`` > 0: two head groups, channels [0, split) and
    [split, dim / slabs) of every slab, each a complete wire buffer, one behind the other (``wan_rmsnorm_rope_sp_split``)."""
    rows, dim, ld, cos, sin, rp = _rmsnorm_rope_args("rmsnorm_rope_sp", x0, w0, x1, w1, head_dim, rope, rope_params,
                                                     (("wire0", wire0), ("wire1", wire1)), torch.bfloat16)
    lib = _lib.load()
    if split:
        _lib.check(lib.wan_rmsnorm_rope_sp_split(_p(x0), _p(w0), _p(x1), _p(w1), ld, rows, dim, head_dim, float(eps), _p(cos), _p(sin),
                                                 rp, float(x0_scale), _p(wire0), _p(wire1), int(slabs), int(batch),
                                                 int(split), _stream()), "wan_rmsnorm_rope_sp_split")
        return
    _lib.check(lib.wan_rmsnorm_rope_sp(_p(x0), _p(w0), _p(x1), _p(w1), ld, rows, dim, head_dim, float(eps), _p(cos), _p(sin),
                                       rp, float(x0_scale), _p(wire0), _p(wire1), int(slabs), int(batch),
                                       _stream()), "wan_rmsnorm_rope_sp")


@_on_tensor_device
def sp_pack_heads(x: torch.Tensor, wire: torch.Tensor, P: int, T: int, B: int, split: int = 0) -> torch.Tensor:
    """x bf16 [B*T, ldx >= C] (C = P * Cl) -> token-major wire [P][T][B][Cl] (``split`` > 0: two head-group wires, see ``rmsnorm_rope_sp``)."""
    _need(x, torch.bfloat16, "sp_pack_heads.x")
    _need(wire, torch.bfloat16, "sp_pack_heads.wire")
    C = x.shape[1]
    if x.shape[0] != B * T or C % P or not wire.is_contiguous() or wire.numel() < B * T * C:
        raise ValueError("sp_pack_heads: shapes disagree")
    lib = _lib.load()
    if split:
        _lib.check(lib.wan_sp_pack_heads_split(_p(x), x.stride(0), _p(wire), P, T, B, C // P, int(split), _stream()), "wan_sp_pack_heads_split")
    else:
        _lib.check(lib.wan_sp_pack_heads(_p(x), x.stride(0), _p(wire), P, T, B, C // P, _stream()), "wan_sp_pack_heads")
    return wire


@_on_tensor_device
def sp_unpack_heads(wire: torch.Tensor, x: torch.Tensor, P: int, T: int, B: int, split: int = 0) -> torch.Tensor:
    """token-major wire [P][T][B][Cl] -> x bf16 [B*T, ldx >= P*Cl] (column s * Cl + c); ``split`` > 0: from two head-group wires."""
    _need(x, torch.bfloat16, "sp_unpack_heads.x")
    _need(wire, torch.bfloat16, "sp_unpack_heads.wire")
    C = x.shape[1]
    if x.shape[0] != B * T or C % P or not wire.is_contiguous() or wire.numel() < B * T * C:
        raise ValueError("sp_unpack_heads: shapes disagree")
    lib = _lib.load()
    if split:
        _lib.check(lib.wan_sp_unpack_heads_split(_p(wire), _p(x), x.stride(0), P, T, B, C // P, int(split), _stream()),
                   "wan_sp_unpack_heads_split")
    else:
        _lib.check(lib.wan_sp_unpack_heads(_p(wire), _p(x), x.stride(0), P, T, B, C // P, _stream()), "wan_sp_unpack_heads")
    return x


@_on_tensor_device
def sp_unpack_vt(wire: torch.Tensor, vt: torch.Tensor, P: int, T: int) -> torch.Tensor:
    """arrived channel-major wire [P][Cl][B][T] -> vt bf16 [B, Cl, ldvt >= P*T], column s * T + t."""
    _need(vt, torch.bfloat16, "sp_unpack_vt.vt")
    _need(wire, torch.bfloat16, "sp_unpack_vt.wire")
    B, Cl, ldvt = vt.shape
    if not wire.is_contiguous() or wire.numel() < P * Cl * B * T or not vt.is_contiguous():
        raise ValueError("sp_unpack_vt: shapes disagree")
    lib = _lib.load()
    _lib.check(lib.wan_sp_unpack_vt(_p(wire), _p(vt), ldvt, P, B, Cl, T, _stream()), "wan_sp_unpack_vt")
    return vt


@_on_tensor_device
def sp_channel_copy(dst: torch.Tensor, src: torch.Tensor, channels: int = 16, threads: int = 512) -> torch.Tensor:
    """``wan_sp_channel_copy`` (MEASUREMENT ONLY): dst <- src, byte for byte, by a grid of exactly ``channels`` workgroups of
    ``threads`` lanes on the current stream -- the launch footprint assumed for a collective with that many channels (include/wan_hip.h).
    Contiguous device tensors of equal byte size, any dtypes, not overlapping."""
    for t, name in ((dst, "sp_channel_copy.dst"), (src, "sp_channel_copy.src")):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path has no CPU fallback")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes or dst.device != src.device:
        raise ValueError("sp_channel_copy: dst / src must hold the same number of bytes on one device")
    _lib.check(_lib.load().wan_sp_channel_copy(_p(dst), _p(src), nbytes, int(channels), int(threads), _stream()), "wan_sp_channel_copy")
    return dst


def q_prescale(head_dim: int, softmax_scale: Optional[float] = None) -> float:
    """The factor q must carry for ``attention_fwd(q_prescaled=True)``: softmax_scale * log2(e)."""
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(head_dim)
    return float(scale) * _lib.LOG2E


@_on_tensor_device
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epilogue: int,
         out: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
         rows_per_batch: int = 0, ldo_t: int = 0) -> torch.Tensor:
    """acc = a @ w.T (+bias) with one of the fused epilogues.  a bf16 [M,K] (row stride free),
    w bf16 [N,K] (nn.Linear layout).  For EPI_RESID_F32 `out` is updated in place.  For
    EPI_BF16_T the result is [N, ldo_t] with out[n, m] (ldo_t >= M)."""
    _need(a, torch.bfloat16, "gemm.a")
    _need(w, torch.bfloat16, "gemm.w")
    M, K = a.shape
    N, Kw = w.shape
    if K != Kw:
        raise ValueError(f"gemm: a is [{M},{K}] but w is [{N},{Kw}]")
    if bias is not None:
        _need(bias, torch.float32, "gemm.bias")
        if bias.numel() != N:
            raise ValueError("gemm: bias length != N")
    dev = a.device
    if epilogue in (EPI_BF16, EPI_GELU_BF16):
        if out is None:
            out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        _need(out, torch.bfloat16, "gemm.out")
    elif epilogue == EPI_F32:
        if out is None:
            out = torch.empty(M, N, device=dev, dtype=torch.float32)
        _need(out, torch.float32, "gemm.out")
    elif epilogue == EPI_RESID_F32:
        if out is None:
            raise ValueError("gemm: EPI_RESID_F32 needs the residual stream as `out`")
        _need(out, torch.float32, "gemm.out")
        if gate is not None:
            _need(gate, torch.float32, "gemm.gate")
            if not gate.is_contiguous() or gate.shape[-1] != N:
                raise ValueError("gemm.gate must be contiguous [nbatch, N]")
    elif epilogue == EPI_BF16_T:
        if out is None:
            ldo_t = ldo_t or round_up(M, 64)
            out = torch.zeros(N, ldo_t, device=dev, dtype=torch.bfloat16)
        _need(out, torch.bfloat16, "gemm.out")
        if out.shape[0] != N or out.shape[1] < M:
            raise ValueError(f"gemm: transposed out must be [N={N}, >= M={M}], got {tuple(out.shape)}")
    else:
        raise ValueError(f"gemm: unknown epilogue {epilogue}")
    if epilogue != EPI_BF16_T and tuple(out.shape) != (M, N):
        raise ValueError(f"gemm: out shape {tuple(out.shape)} != ({M},{N})")
    lib = _lib.load()
    ws = gemm_workspace(dev, M, N, K)
    _lib.check(lib.wan_gemm_bf16_ws(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0),
                                    M, N, K, epilogue, _p(gate), int(rows_per_batch), _p(ws), ws.numel() if ws is not None else 0,
                                    _stream()), "wan_gemm_bf16_ws")
    return out


_GEMM_WS = {}


def gemm_workspace(dev: torch.device, M: int, N: int, K: int, fp8: bool = False) -> Optional[torch.Tensor]:
    """The caller-owned workspace of ``wan_gemm_bf16_ws`` (the persistent stream-K GEMM's partial tiles, arrival and
    ticket counters): ONE buffer per (device, STREAM), grown to the largest request and then kept for the life of the
    process.  The kernel keeps its counters and split-tile partial sums in it, so two launches that share a workspace must
    be stream-ordered: keyed by the current stream, GEMMs issued on different streams of one device (two pipelines, a
    caller's side stream) can never meet in one buffer.  Launches recorded under stream capture share one per-device
    "capture" workspace (the capturing stream is a pool stream that differs from capture to capture; a graph bakes the
    address in and the entry stays alive with this table); like the model's activation buffers it is owned by the graphs
    of that device, whose replays must not overlap each other; when a capture asks for more than the capture workspace holds, a new
    buffer is allocated and the old one stays alive for the launches already recorded.  The buffer is NOT cleared here -- the launch clears the
    4 KiB of counters it uses with a memset node of its own.  None when the shape does not use a workspace
    (``wan_gemm_workspace_bytes`` == 0).  ``fp8``: the request of the e4m3 Linear (``wan_gemm_fp8_workspace_bytes``; same buffer)."""
    need = int(_lib.load().wan_gemm_fp8_workspace_bytes(M, N, K) if fp8 else _lib.load().wan_gemm_workspace_bytes(M, N, K))
    if need <= 0:
        return None
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    capturing = torch.cuda.is_current_stream_capturing()
    key = (index, "capture" if capturing else int(torch.cuda.current_stream(index).cuda_stream))
    ws = _GEMM_WS.get(key)
    if ws is None or ws.numel() < need:
        if capturing:
            # a graph bakes addresses in: launches already recorded keep the buffer they were given (a workspace only has to live
            # through its own launch), so a grown request gets a NEW buffer and the old one is kept alive for the recorded nodes.
            # The first capture buffer of a device is sized like the largest eager workspace (the eager warm-up call of
            # GraphedForward / GraphedLoop has run every shape), so this branch is normally taken once.
            if ws is not None:
                _GEMM_WS_RETIRED.append(ws)
            need = max([need] + [t.numel() for (i, _), t in _GEMM_WS.items() if i == index])
        ws = torch.empty(need, device=torch.device("cuda", index), dtype=torch.uint8)
        _GEMM_WS[key] = ws
    return ws


_GEMM_WS_RETIRED = []


def release_gemm_workspaces(include_capture: bool = False) -> int:
    """Drop the cached persistent-GEMM workspaces (~128 MiB per (device, stream) that ever issued a Linear): the eager entries
    always -- each is re-allocated by the next GEMM of its stream, and a buffer goes back to the caching allocator on the stream
    whose launches used it, so nothing in flight loses it -- and, with ``include_capture``, the per-device capture workspaces and
    the retired ones as well -- ONLY once every hipGraph of the process that recorded launches on them is gone (a graph holds raw
    addresses, not references; ``WanTransformer3DModel.release_workspaces()`` therefore never passes True).  Returns the bytes released."""
    freed = 0
    for key in [k for k in _GEMM_WS if include_capture or k[1] != "capture"]:
        freed += _GEMM_WS.pop(key).numel()
    if include_capture:
        freed += sum(t.numel() for t in _GEMM_WS_RETIRED)
        _GEMM_WS_RETIRED.clear()
    return freed


class AttentionWorkspace:
    """Scratch of one ``wan_attention_fwd`` CALL SITE (the flags of the max-free attempt, its sticky "fast path off"
    word, the partial results of the split tail round).  One object per call site and stream: the sticky word then
    describes the inputs of THAT site only (a self-attention layer with out-of-window scores does not switch the
    kernel of cross-attention or of another model), and two streams never share flags.  Launches that use one
    workspace must be stream-ordered."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, device: torch.device, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.device != device or self.buf.numel() < nbytes:
            self.buf = torch.zeros(nbytes, device=device, dtype=torch.uint8)       # zeroed header (sticky word off)
        return self.buf

    def reset(self) -> None:
        """Forget the sticky decision (e.g. after loading other weights)."""
        if self.buf is not None:
            self.buf[:16].zero_()


# ---------------------------------------------------------------------------------------------
# FP8 (OCP e4m3) projections -- SURVEY.md 8f-4; an explicit, lossy option (WanTransformer3DModel.enable_fp8_linear)
# ---------------------------------------------------------------------------------------------
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


@_on_tensor_device
def ln_modulate_fp8(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], add_one: bool,
                    rows_per_batch: int, eps: float, out: Optional[torch.Tensor] = None,
                    out_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ln_modulate`` with per-token-row e4m3 quantisation fused in: returns (q [rows, dim] float8_e4m3fn, s fp32 [rows])
    with y ~= q * s[:, None]."""
    rows, dim = _ln_modulate_args("ln_modulate_fp8", x, scale, shift, rows_per_batch)
    if out is None:
        out = torch.empty(rows, dim, device=x.device, dtype=FP8)
    if out_scale is None:
        out_scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    _need(out, FP8, "ln_modulate_fp8.out")
    _need(out_scale, torch.float32, "ln_modulate_fp8.out_scale")
    if not out.is_contiguous() or tuple(out.shape) != (rows, dim) or out_scale.numel() < rows:
        raise ValueError("ln_modulate_fp8: out must be contiguous [rows, dim] and out_scale hold one value per row")
    lib = _lib.load()
    _lib.check(lib.wan_ln_modulate_fp8(_p(x), _p(scale), _p(shift), int(bool(add_one)), _p(out), _p(out_scale), rows, dim,
                                       int(rows_per_batch), float(eps), _stream()), "wan_ln_modulate_fp8")
    return out, out_scale


@_on_tensor_device
def quantize_rows_fp8(x: torch.Tensor, out: Optional[torch.Tensor] = None,
                      out_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 [rows, cols] -> (e4m3 [rows, cols], fp32 row scales = max|x| / 448)."""
    _need(x, torch.bfloat16, "quantize_rows_fp8.x")
    if x.dim() != 2:
        raise ValueError("quantize_rows_fp8.x must be 2-D")
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=FP8)
    if out_scale is None:
        out_scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    _need(out, FP8, "quantize_rows_fp8.out")
    _need(out_scale, torch.float32, "quantize_rows_fp8.out_scale")
    lib = _lib.load()
    _lib.check(lib.wan_quantize_rows_fp8(_p(x), x.stride(0), _p(out), out.stride(0), _p(out_scale), rows, cols, _stream()),
               "wan_quantize_rows_fp8")
    return out, out_scale


def quantize_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One-off weight preparation (torch): [N, K] -> (e4m3 [N, K], fp32 per-output-channel scales = max|w[n,:]| / 448)."""
    wf = w.float()
    s = wf.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX
    return (wf / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8).contiguous(), s.contiguous()


@_on_tensor_device
def gemm_fp8(a: torch.Tensor, a_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
             epilogue: int, out: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
             rows_per_batch: int = 0, ldo_t: int = 0) -> torch.Tensor:
    """acc = (a_q @ w_q.T) * a_scale[:, None] * w_scale[None, :] (+ bias) with the epilogues of ``gemm``.
    a e4m3 [M, K] (row stride free), w e4m3 [N, K]; K % 128 == 0."""
    _need(a, FP8, "gemm_fp8.a")
    _need(w, FP8, "gemm_fp8.w")
    _need(a_scale, torch.float32, "gemm_fp8.a_scale")
    _need(w_scale, torch.float32, "gemm_fp8.w_scale")
    M, K = a.shape
    N, Kw = w.shape
    if K != Kw or a_scale.numel() < M or w_scale.numel() != N:
        raise ValueError(f"gemm_fp8: a is [{M},{K}], w is [{N},{Kw}], scales {a_scale.numel()} / {w_scale.numel()}")
    if bias is not None:
        _need(bias, torch.float32, "gemm_fp8.bias")
        if bias.numel() != N:
            raise ValueError("gemm_fp8: bias length != N")
    dev = a.device
    if epilogue in (EPI_BF16, EPI_GELU_BF16):
        if out is None:
            out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        _need(out, torch.bfloat16, "gemm_fp8.out")
    elif epilogue == EPI_F32:
        if out is None:
            out = torch.empty(M, N, device=dev, dtype=torch.float32)
        _need(out, torch.float32, "gemm_fp8.out")
    elif epilogue == EPI_RESID_F32:
        if out is None:
            raise ValueError("gemm_fp8: EPI_RESID_F32 needs the residual stream as `out`")
        _need(out, torch.float32, "gemm_fp8.out")
        if gate is not None:
            _need(gate, torch.float32, "gemm_fp8.gate")
    elif epilogue == EPI_BF16_T:
        if out is None:
            out = torch.zeros(N, ldo_t or round_up(M, 64), device=dev, dtype=torch.bfloat16)
        _need(out, torch.bfloat16, "gemm_fp8.out")
        if out.shape[0] != N or out.shape[1] < M:
            raise ValueError(f"gemm_fp8: transposed out must be [N={N}, >= M={M}], got {tuple(out.shape)}")
    else:
        raise ValueError(f"gemm_fp8: unknown epilogue {epilogue}")
    if epilogue != EPI_BF16_T and tuple(out.shape) != (M, N):
        raise ValueError(f"gemm_fp8: out shape {tuple(out.shape)} != ({M},{N})")
    lib = _lib.load()
    # the persistent stream-K kernel's e4m3 instantiation where the plan says so (its workspace is the bf16 GEMM's: one per stream)
    ws = gemm_workspace(dev, M, N, K, fp8=True)
    _lib.check(lib.wan_gemm_fp8_ws(_p(a), a.stride(0), _p(a_scale), _p(w), w.stride(0), _p(w_scale), _p(bias), _p(out),
                                   out.stride(0), M, N, K, epilogue, _p(gate), int(rows_per_batch), _p(ws),
                                   ws.numel() if ws is not None else 0, _stream()), "wan_gemm_fp8_ws")
    return out


_ATTN_WS = {}          # ad-hoc callers without their own workspace: one per (device, stream)


@_on_tensor_device
def attention_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, num_heads: int, k_len: Optional[int] = None,
                  softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                  q_prescaled: bool = False, workspace: Optional[AttentionWorkspace] = None,
                  k_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q bf16 [B,Lq,H*128], k bf16 [B,Lk,H*128], vt bf16 [B,H*128,ldvt] (V transposed, ldvt >=
    roundup(k_len,64), finite padding) -> bf16 [B,Lq,H*128].  Keys >= k_len are masked.
    ``q_prescaled``: q already carries softmax_scale*log2(e) (see ``rmsnorm_rope_``'s x0_scale).
    ``workspace``: the call site's ``AttentionWorkspace`` (default: one per device and stream).
    ``k_lens``: int32 [B] ON THE DEVICE -- a ragged batch in one launch (``wan_attention_fwd_varlen``): sample b attends keys
    [0, k_lens[b]); the kernel reads the counts, the host never does."""
    for nm, t in (("q", q), ("k", k), ("vt", vt)):
        _need(t, torch.bfloat16, "attention." + nm)
        if t.dim() != 3:
            raise ValueError(f"attention.{nm} must be 3-D [B, rows, cols]")
    B, Lq, C = q.shape
    Lk = k.shape[1] if k_len is None else int(k_len)
    if Lk > k.shape[1] or Lk <= 0:
        raise ValueError(f"attention: k_len={Lk} outside (0, {k.shape[1]}]")
    head_dim = C // num_heads
    if out is None:
        out = torch.empty(B, Lq, C, device=q.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "attention.out")
    if vt.shape[1] != C or k.shape[2] != C or k.shape[0] != B or vt.shape[0] != B:
        raise ValueError("attention: q/k/vt shapes disagree")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(head_dim)
    lib = _lib.load()
    ws, ws_bytes = None, int(lib.wan_attention_workspace_bytes(B, Lq, Lk, num_heads, head_dim))
    if ws_bytes > 0:
        if workspace is None:
            key = (q.device, _stream())
            workspace = _ATTN_WS.get(key)
            if workspace is None:
                workspace = _ATTN_WS[key] = AttentionWorkspace()
        ws = workspace.get(q.device, ws_bytes)
    if k_lens is not None:
        _need(k_lens, torch.int32, "attention.k_lens")
        if k_lens.shape != (B,) or not k_lens.is_contiguous():
            raise ValueError(f"attention.k_lens must be a contiguous int32 [{B}]")
        _lib.check(lib.wan_attention_fwd_varlen(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0),
                                                _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1), out.stride(0),
                                                B, Lq, Lk, _p(k_lens), num_heads, head_dim, float(scale),
                                                _lib.ATTN_Q_PRESCALED if q_prescaled else 0, _p(ws),
                                                ws_bytes if ws is not None else 0, _stream()), "wan_attention_fwd_varlen")
        return out
    _lib.check(lib.wan_attention_fwd(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0),
                                     _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1), out.stride(0),
                                     B, Lq, Lk, num_heads, head_dim, float(scale),
                                     _lib.ATTN_Q_PRESCALED if q_prescaled else 0, _p(ws), ws_bytes if ws is not None else 0,
                                     _stream()), "wan_attention_fwd")
    return out


def attn_sparse_validate(row_ptr, tiles, n_qblocks: int, n_ktiles: int) -> None:
    """``wan_attn_sparse_validate`` (host arithmetic, no GPU): ValueError naming the first offence of the list contract."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    tl = np.ascontiguousarray(tiles, dtype=np.int32)
    if rp.ndim != 1 or tl.ndim != 1 or rp.size != int(n_qblocks) + 1 or int(rp.max()) > tl.size:       # the library reads tiles[row_ptr[..]]
        raise ValueError(f"attn_sparse: row_ptr must hold n_qblocks + 1 = {int(n_qblocks) + 1} offsets into the {tl.size} tiles")
    _lib.check(_lib.load().wan_attn_sparse_validate(rp.ctypes.data, tl.ctypes.data if tl.size else None, int(n_qblocks), int(n_ktiles)),
               "wan_attn_sparse_validate")


class AttnSparsePlan:
    """Owns one ``wan_attn_sparse`` handle: the validated key-tile lists of a local-attention plan (``local_attention.py``) and their
    device copy, for calls with exactly these ``Lq`` / ``Lk`` on ``device``.  Create it outside a graph capture (the upload is a
    synchronous copy); keep it alive while launches that use it are in flight."""

    def __init__(self, row_ptr, tiles, Lq: int, Lk: int, device):
        self.device = torch.device(device)
        self.Lq, self.Lk = int(Lq), int(Lk)
        self.n_qblocks, self.n_ktiles = (self.Lq + 255) // 256, (self.Lk + 63) // 64
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        tl = np.ascontiguousarray(tiles, dtype=np.int32)
        attn_sparse_validate(rp, tl, self.n_qblocks, self.n_ktiles)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().wan_attn_sparse_create(rp.ctypes.data, tl.ctypes.data, self.Lq, self.Lk, ctypes.byref(self._handle)),
                       "wan_attn_sparse_create")

    @property
    def listed(self) -> int:
        return int(_lib.load().wan_attn_sparse_listed(self._handle))

    @property
    def density(self) -> float:
        return self.listed / float(self.n_qblocks * self.n_ktiles)

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _lib.load().wan_attn_sparse_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: the library may be gone
            pass


@_on_tensor_device
def attention_fwd_sparse(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, num_heads: int, plan: AttnSparsePlan,
                         k_len: Optional[int] = None, softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                         q_prescaled: bool = False) -> torch.Tensor:
    """``wan_attention_fwd_sparse``: operands as ``attention_fwd``; query block i (256 rows) attends exactly the keys of the 64-key
    tiles ``plan`` lists for it.  One launch, no workspace.  LOSSY against dense attention unless every tile is listed."""
    for nm, t in (("q", q), ("k", k), ("vt", vt)):
        _need(t, torch.bfloat16, "attention_sparse." + nm)
        if t.dim() != 3:
            raise ValueError(f"attention_sparse.{nm} must be 3-D [B, rows, cols]")
    B, Lq, C = q.shape
    Lk = k.shape[1] if k_len is None else int(k_len)
    if Lk > k.shape[1] or Lk <= 0:
        raise ValueError(f"attention_sparse: k_len={Lk} outside (0, {k.shape[1]}]")
    if not isinstance(plan, AttnSparsePlan) or not plan._handle:
        raise ValueError("attention_sparse: plan must be a live ops.AttnSparsePlan")
    if plan.device != q.device:
        raise ValueError(f"attention_sparse: the plan lives on {plan.device}, q on {q.device}")
    head_dim = C // num_heads
    if out is None:
        out = torch.empty(B, Lq, C, device=q.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "attention_sparse.out")
    if vt.shape[1] != C or k.shape[2] != C or k.shape[0] != B or vt.shape[0] != B:
        raise ValueError("attention_sparse: q/k/vt shapes disagree")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(head_dim)
    _lib.check(_lib.load().wan_attention_fwd_sparse(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0),
                                                    _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1), out.stride(0),
                                                    B, Lq, Lk, plan._handle, num_heads, head_dim, float(scale),
                                                    _lib.ATTN_Q_PRESCALED if q_prescaled else 0, _stream()), "wan_attention_fwd_sparse")
    return out


def cross_fold_plan(rows: int, num_heads: int, text_len: int, kept: int, weights_bf16: bool = True) -> bool:
    """``wan_cross_fold_plan`` (include/wan_hip.h a9f): THE rule -- whether `rows` query rows take the folded cross-attention branch."""
    return bool(_lib.load().wan_cross_fold_plan(int(rows), int(num_heads), int(text_len), int(kept), int(bool(weights_bf16))))


@_on_tensor_device
def cross_probs(q: torch.Tensor, k: torch.Tensor, num_heads: int, kept: int, pad_count: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wan_cross_probs``: q bf16 [B, L, H*128] pre-scaled (dense samples: L rows of stride q.stride(1) each), k bf16 [B, T, H*128]
    -> softmax weights bf16 [B*L, H*64] over keys 0..kept (key `kept` standing for `pad_count` identical rows)."""
    _need(q, torch.bfloat16, "cross_probs.q")
    _need(k, torch.bfloat16, "cross_probs.k")
    B, L, C = q.shape
    if k.dim() != 3 or k.shape[0] != B or k.shape[2] != C or C != num_heads * 128 or k.shape[1] < kept + 1:
        raise ValueError(f"cross_probs: q {tuple(q.shape)} / k {tuple(k.shape)} / heads {num_heads} / kept {kept} disagree")
    if B > 1 and q.stride(0) != L * q.stride(1):
        raise ValueError("cross_probs: the samples of q must follow each other without a gap")
    if out is None:
        out = torch.empty(B * L, num_heads * 64, device=q.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "cross_probs.out")
    if tuple(out.shape) != (B * L, num_heads * 64):
        raise ValueError(f"cross_probs: out shape {tuple(out.shape)} != ({B * L},{num_heads * 64})")
    _lib.check(_lib.load().wan_cross_probs(_p(q), q.stride(1), _p(k), k.stride(1), k.stride(0), _p(out), out.stride(0), B, L,
                                           int(num_heads), int(kept), int(pad_count), _stream()), "wan_cross_probs")
    return out


@_on_tensor_device
def cross_fold_values(w_co: torch.Tensor, vt: torch.Tensor, num_heads: int, kept: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wan_cross_fold_values``: w_co bf16 [C, C], vt bf16 [B, C, T] (the text V^T) -> V'^T bf16 [B, C, H*64] in nn.Linear layout."""
    _need(w_co, torch.bfloat16, "cross_fold_values.w_co")
    _need(vt, torch.bfloat16, "cross_fold_values.vt")
    B, C, T = vt.shape
    if tuple(w_co.shape) != (C, C) or C != num_heads * 128:
        raise ValueError(f"cross_fold_values: w_co {tuple(w_co.shape)} / vt {tuple(vt.shape)} / heads {num_heads} disagree")
    if out is None:
        out = torch.empty(B, C, num_heads * 64, device=vt.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "cross_fold_values.out")
    if tuple(out.shape) != (B, C, num_heads * 64):
        raise ValueError(f"cross_fold_values: out shape {tuple(out.shape)} != ({B},{C},{num_heads * 64})")
    _lib.check(_lib.load().wan_cross_fold_values(_p(w_co), w_co.stride(0), _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1),
                                                 out.stride(0), B, C, int(num_heads), int(kept), _stream()), "wan_cross_fold_values")
    return out


@_on_tensor_device
def rmsnorm_rope_fp8(x0: torch.Tensor, w0: torch.Tensor, x1: Optional[torch.Tensor], w1: Optional[torch.Tensor], head_dim: int,
                     eps: float, rope: Optional[Tuple[torch.Tensor, torch.Tensor]], rope_params: Optional[RopeParams],
                     out0: torch.Tensor, out1: Optional[torch.Tensor], x0_scale: float = 1.0, x1_scale: float = 1.0) -> None:
    """``rmsnorm_rope_`` that leaves x0 / x1 untouched and writes OCP e4m3 copies of the results (dense ``FP8`` [rows, dim]):
    ``out = e4m3(bf16(result * scale))`` -- the operands of ``attention_fwd_qk8`` (include/wan_hip.h, a9')."""
    rows, dim, ld, cos, sin, rp = _rmsnorm_rope_args("rmsnorm_rope_fp8", x0, w0, x1, w1, head_dim, rope, rope_params,
                                                     (("out0", out0), ("out1", out1)), FP8)
    lib = _lib.load()
    _lib.check(lib.wan_rmsnorm_rope_fp8(_p(x0), _p(w0), _p(x1), _p(w1), ld, rows, dim, head_dim, float(eps), _p(cos), _p(sin),
                                        rp, float(x0_scale), float(x1_scale), _p(out0), _p(out1), _stream()), "wan_rmsnorm_rope_fp8")


@_on_tensor_device
def vt_quantize_mx(vt: torch.Tensor, num_heads: int, k_len: int, v8: Optional[torch.Tensor] = None,
                   scales: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """V^T bf16 [B, H*128, ldvt] -> (MX e4m3 [B, H*128, ldvt] with the keys of every 64-tile in the attention kernel's register order,
    uint8 E8M0 scales, one per channel row and 32 consecutive keys): the V operand of ``attention_fwd_f8`` (include/wan_hip.h a9'')."""
    _need(vt, torch.bfloat16, "vt_quantize_mx.vt")
    if vt.dim() != 3:
        raise ValueError("vt_quantize_mx.vt must be [B, H*128, ldvt]")
    B, C, ld = vt.shape
    lib = _lib.load()
    nsc = int(lib.wan_vt_mx_scale_bytes(B, num_heads, int(k_len)))
    if v8 is None:
        v8 = torch.empty(B, C, ld, device=vt.device, dtype=FP8)
    if scales is None:
        scales = torch.empty(nsc, device=vt.device, dtype=torch.uint8)
    _need(v8, FP8, "vt_quantize_mx.v8")
    _need(scales, torch.uint8, "vt_quantize_mx.scales")
    if v8.shape != vt.shape or scales.numel() < nsc or not scales.is_contiguous():
        raise ValueError("vt_quantize_mx: v8 must have vt's shape and scales wan_vt_mx_scale_bytes() contiguous bytes")
    _lib.check(lib.wan_vt_quantize_mx(_p(vt), vt.stride(1), vt.stride(0), B, int(num_heads), int(k_len), _p(v8), v8.stride(1), v8.stride(0),
                                      _p(scales), _stream()), "wan_vt_quantize_mx")
    return v8, scales


@_on_tensor_device
def attention_fwd_f8(q8: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, v8_scales: torch.Tensor, vt: torch.Tensor, num_heads: int,
                     q_exp: int, k_exp: int, k_len: Optional[int] = None, out: Optional[torch.Tensor] = None,
                     workspace: Optional[AttentionWorkspace] = None) -> torch.Tensor:
    """Self-attention with BOTH products on the fp8 matrix pipe (LOSSY, opt-in; include/wan_hip.h a9'').  q8 / k8 as
    ``attention_fwd_qk8``; v8 / v8_scales from ``vt_quantize_mx(vt, ...)``; the bf16 ``vt`` serves the workgroups whose max-free
    softmax check fails (and the split-KV tail round)."""
    for nm, t, dt in (("q8", q8, FP8), ("k8", k8, FP8), ("v8", v8, FP8), ("vt", vt, torch.bfloat16)):
        _need(t, dt, "attention_f8." + nm)
        if t.dim() != 3:
            raise ValueError(f"attention_f8.{nm} must be 3-D [B, rows, cols]")
    _need(v8_scales, torch.uint8, "attention_f8.v8_scales")
    B, Lq, C = q8.shape
    Lk = k8.shape[1] if k_len is None else int(k_len)
    if Lk > k8.shape[1] or Lk <= 0:
        raise ValueError(f"attention_f8: k_len={Lk} outside (0, {k8.shape[1]}]")
    head_dim = C // num_heads
    if out is None:
        out = torch.empty(B, Lq, C, device=q8.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "attention_f8.out")
    if vt.shape[1] != C or v8.shape != vt.shape or k8.shape[2] != C or k8.shape[0] != B or vt.shape[0] != B:
        raise ValueError("attention_f8: q8/k8/v8/vt shapes disagree")
    lib = _lib.load()
    ws_bytes = max(int(lib.wan_attention_workspace_bytes(B, Lq, Lk, num_heads, head_dim)), 16)
    if workspace is None:
        key = (q8.device, _stream())
        workspace = _ATTN_WS.get(key)
        if workspace is None:
            workspace = _ATTN_WS[key] = AttentionWorkspace()
    ws = workspace.get(q8.device, ws_bytes)
    _lib.check(lib.wan_attention_fwd_f8(_p(q8), q8.stride(1), q8.stride(0), int(q_exp), _p(k8), k8.stride(1), k8.stride(0), int(k_exp),
                                        _p(v8), v8.stride(1), v8.stride(0), _p(v8_scales), _p(vt), vt.stride(1), vt.stride(0),
                                        _p(out), out.stride(1), out.stride(0), B, Lq, Lk, num_heads, head_dim, _p(ws), ws_bytes, _stream()),
               "wan_attention_fwd_f8")
    return out


@_on_tensor_device
def col_mean(x: torch.Tensor, rows_per_batch: int, valid_rows: int, batch: int, out: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [batch, dim]: mean over the first ``valid_rows`` rows of every sample of bf16 x [batch * rows_per_batch, dim] (row
    stride free).  Two-stage, fixed summation order.  ``workspace``: fp32, >= wan_col_mean_workspace_bytes / 4 elements."""
    _need(x, torch.bfloat16, "col_mean.x")
    dim = x.shape[1]
    lib = _lib.load()
    need = int(lib.wan_col_mean_workspace_bytes(batch, dim)) // 4
    if workspace is None:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    _need(workspace, torch.float32, "col_mean.workspace")
    if workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError(f"col_mean.workspace needs {need} contiguous fp32 elements")
    if out is None:
        out = torch.empty(batch, dim, device=x.device, dtype=torch.float32)
    _need(out, torch.float32, "col_mean.out")
    _lib.check(lib.wan_col_mean_bf16(_p(x), x.stride(0), int(rows_per_batch), int(valid_rows), int(batch), dim, _p(workspace), _p(out),
                                     _stream()), "wan_col_mean_bf16")
    return out


@_on_tensor_device
def qk_quantize_fp8(q: Optional[torch.Tensor], k: Optional[torch.Tensor], rows_per_batch: int, k_mean: Optional[torch.Tensor],
                    q_scale: float, k_scale: float, q8: Optional[torch.Tensor], k8: Optional[torch.Tensor]) -> None:
    """q8 = e4m3(q * q_scale), k8 = e4m3((k - k_mean[sample]) * k_scale) from bf16 [rows, dim] views (when both are given they
    share shape and row stride; ``k_mean`` fp32 [batch, dim] or None); dense ``FP8`` [rows, dim] outputs.  Either operand may be
    None together with its output (the Ulysses head-group pipeline quantises k once and every q group on arrival)."""
    if (q is None) != (q8 is None) or (k is None) != (k8 is None) or (q is None and k is None):
        raise ValueError("qk_quantize_fp8: q comes with q8, k with k8, and at least one pair is needed")
    if k is None and k_mean is not None:
        raise ValueError("qk_quantize_fp8: k_mean without k")
    ref = q if q is not None else k
    for nm, t in (("q", q), ("k", k)):
        if t is not None:
            _need(t, torch.bfloat16, "qk_quantize_fp8." + nm)
            if t.dim() != 2 or t.shape != ref.shape or t.stride(0) != ref.stride(0):
                raise ValueError("qk_quantize_fp8: q and k must be 2-D and share shape and row stride")
    rows, dim = ref.shape
    for nm, t in (("q8", q8), ("k8", k8)):
        if t is None:
            continue
        _need(t, FP8, "qk_quantize_fp8." + nm)
        if not t.is_contiguous() or t.numel() < rows * dim:
            raise ValueError(f"qk_quantize_fp8.{nm} must be contiguous with >= rows * dim bytes")
    if k_mean is not None:
        _need(k_mean, torch.float32, "qk_quantize_fp8.k_mean")
        if not k_mean.is_contiguous() or k_mean.shape[-1] != dim:
            raise ValueError("qk_quantize_fp8.k_mean must be contiguous [batch, dim]")
    lib = _lib.load()
    _lib.check(lib.wan_qk_quantize_fp8(_p(q), _p(k), ref.stride(0), rows, dim, int(rows_per_batch), _p(k_mean), float(q_scale),
                                       float(k_scale), _p(q8), _p(k8), _stream()), "wan_qk_quantize_fp8")


@_on_tensor_device
def attention_fwd_qk8(q8: torch.Tensor, k8: torch.Tensor, vt: torch.Tensor, num_heads: int, q_exp: int, k_exp: int,
                      k_len: Optional[int] = None, out: Optional[torch.Tensor] = None,
                      workspace: Optional[AttentionWorkspace] = None) -> torch.Tensor:
    """Self-attention with QK^T on the fp8 matrix pipe (LOSSY, opt-in; include/wan_hip.h a9').
    q8 e4m3 [B,Lq,H*128] = e4m3(q * softmax_scale * log2(e) * 2^q_exp), k8 e4m3 [B,Lk,H*128] = e4m3(k * 2^k_exp)
    (``rmsnorm_rope_fp8`` writes both), vt / out as ``attention_fwd``."""
    for nm, t, dt in (("q8", q8, FP8), ("k8", k8, FP8), ("vt", vt, torch.bfloat16)):
        _need(t, dt, "attention_qk8." + nm)
        if t.dim() != 3:
            raise ValueError(f"attention_qk8.{nm} must be 3-D [B, rows, cols]")
    B, Lq, C = q8.shape
    Lk = k8.shape[1] if k_len is None else int(k_len)
    if Lk > k8.shape[1] or Lk <= 0:
        raise ValueError(f"attention_qk8: k_len={Lk} outside (0, {k8.shape[1]}]")
    head_dim = C // num_heads
    if out is None:
        out = torch.empty(B, Lq, C, device=q8.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "attention_qk8.out")
    if vt.shape[1] != C or k8.shape[2] != C or k8.shape[0] != B or vt.shape[0] != B:
        raise ValueError("attention_qk8: q8/k8/vt shapes disagree")
    lib = _lib.load()
    ws, ws_bytes = None, int(lib.wan_attention_workspace_bytes(B, Lq, Lk, num_heads, head_dim))
    if ws_bytes > 0:
        if workspace is None:
            key = (q8.device, _stream())
            workspace = _ATTN_WS.get(key)
            if workspace is None:
                workspace = _ATTN_WS[key] = AttentionWorkspace()
        ws = workspace.get(q8.device, ws_bytes)
    _lib.check(lib.wan_attention_fwd_qk8(_p(q8), q8.stride(1), q8.stride(0), int(q_exp), _p(k8), k8.stride(1), k8.stride(0), int(k_exp),
                                         _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1), out.stride(0),
                                         B, Lq, Lk, num_heads, head_dim, _p(ws), ws_bytes if ws is not None else 0, _stream()),
               "wan_attention_fwd_qk8")
    return out


@_on_tensor_device
def transpose_pad(v: torch.Tensor, ldt: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [rows, cols] -> [cols, ldt] (zero padded columns), ldt default roundup(rows, 64)."""
    _need(v, torch.bfloat16, "transpose.v")
    rows, cols = v.shape
    ldt = ldt or round_up(rows, 64)
    if out is None:
        out = torch.empty(cols, ldt, device=v.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "transpose.out")
    lib = _lib.load()
    _lib.check(lib.wan_transpose_bf16(_p(v), v.stride(0), _p(out), out.stride(0), rows, cols, _stream()),
               "wan_transpose_bf16")
    return out


@_on_tensor_device
def patchify(latent: torch.Tensor, patch: Tuple[int, int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """latent [Cin,F,H,W] fp32|bf16 -> bf16 tokens [L, Cin*pt*ph*pw]."""
    if latent.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"patchify: latent dtype {latent.dtype} not supported (fp32 or bf16)")
    _need(latent, latent.dtype, "patchify.latent")
    if not latent.is_contiguous() or latent.dim() != 4:
        raise ValueError("patchify: latent must be contiguous [Cin,F,H,W]")
    Cin, F, H, W = latent.shape
    pt, ph, pw = patch
    L = (F // pt) * (H // ph) * (W // pw)
    K = Cin * pt * ph * pw
    if out is None:
        out = torch.empty(L, K, device=latent.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "patchify.out")
    lib = _lib.load()
    _lib.check(lib.wan_patchify(_p(latent), 0 if latent.dtype == torch.float32 else 1, _p(out), out.stride(0),
                                Cin, F, H, W, pt, ph, pw, _stream()), "wan_patchify")
    return out


@_on_tensor_device
def unpatchify(tokens: torch.Tensor, grid: Tuple[int, int, int], patch: Tuple[int, int, int], cout: int,
               out_dtype: torch.dtype, zero_frames: int = 0, out: Optional[torch.Tensor] = None,
               rep: Optional[int] = None, rep_stride: Optional[int] = None) -> torch.Tensor:
    """tokens fp32 [L, pt*ph*pw*Cout] -> [Cout, F*pt, Hp*ph, Wp*pw] in out_dtype (fp32|bf16); output frames
    < zero_frames are written as zeros (the CoF mask of pipeline_wan.py:736).
    ``rep`` (``wan_unpatchify_rep``): the result is written ``rep`` times in the same pass, copy k at ``out`` + k * ``rep_stride``
    elements -- ``out`` is then the first copy's [Cout, ...] view of a larger buffer the caller owns (``rep_stride`` defaults
    to one result, i.e. a fresh [rep, Cout, ...] tensor is returned when ``out`` is None)."""
    if rep is not None:
        return _unpatchify_rep(tokens, grid, patch, cout, out_dtype, zero_frames, out, int(rep), rep_stride)
    _need(tokens, torch.float32, "unpatchify.tokens")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"unpatchify: out dtype {out_dtype} not supported")
    F, Hp, Wp = grid
    pt, ph, pw = patch
    if tokens.shape[0] < F * Hp * Wp:
        raise ValueError("unpatchify: fewer token rows than the grid")
    shape = (cout, F * pt, Hp * ph, Wp * pw)
    if out is None:
        out = torch.empty(shape, device=tokens.device, dtype=out_dtype)
    _need(out, out_dtype, "unpatchify.out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"unpatchify: out must be contiguous {shape}")
    lib = _lib.load()
    _lib.check(lib.wan_unpatchify(_p(tokens), tokens.stride(0), _p(out), 0 if out_dtype == torch.float32 else 1,
                                  cout, F, Hp, Wp, pt, ph, pw, int(zero_frames), _stream()), "wan_unpatchify")
    return out


def _unpatchify_rep(tokens, grid, patch, cout, out_dtype, zero_frames, out, rep, rep_stride):
    _need(tokens, torch.float32, "unpatchify.tokens")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"unpatchify: out dtype {out_dtype} not supported")
    F, Hp, Wp = grid
    pt, ph, pw = patch
    if tokens.shape[0] < F * Hp * Wp:
        raise ValueError("unpatchify: fewer token rows than the grid")
    shape = (cout, F * pt, Hp * ph, Wp * pw)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    if rep < 1:
        raise ValueError(f"unpatchify: rep={rep}")
    ret = out
    if out is None:
        if rep_stride not in (None, n):
            raise ValueError("unpatchify: rep_stride needs the caller's out buffer")
        ret = torch.empty((rep,) + shape, device=tokens.device, dtype=out_dtype)
        out, rep_stride = ret[0], n
    rep_stride = n if rep_stride is None else int(rep_stride)
    _need(out, out_dtype, "unpatchify.out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"unpatchify: out must be contiguous {shape}")
    # every copy must lie inside the storage `out` is a view of (the kernel writes rep - 1 copies behind it)
    room = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()
    if rep > 1 and (rep_stride < n or (rep - 1) * rep_stride + n > room):
        raise ValueError(f"unpatchify: {rep} copies {rep_stride} elements apart do not fit behind out ({room} elements)")
    lib = _lib.load()
    _lib.check(lib.wan_unpatchify_rep(_p(tokens), tokens.stride(0), _p(out), 0 if out_dtype == torch.float32 else 1,
                                      cout, F, Hp, Wp, pt, ph, pw, int(zero_frames), rep, rep_stride, _stream()), "wan_unpatchify_rep")
    return ret


# ---------------------------------------------------------------------------------------------
# WanVAE kernels (channels-last bf16 activations [T, H, W, C])
# ---------------------------------------------------------------------------------------------
@_on_tensor_device
def conv_cl(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], cout: int, kernel, stride=(1, 1, 1),
            pad=(0, 0, 0), out_thw=None, hist: Optional[torch.Tensor] = None, upsample2x: bool = False,
            time_interleave: bool = False, resid: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 [T,H,W,Cin]; w bf16 [Cout, Kpad] packed (kt,kh,kw,ci); hist bf16 [n<=2,H,W,Cin] or None.
    Returns bf16 [T_out,H_out,W_out,Cout] (time_interleave: [2*T_out,H_out,W_out,Cout/2]).
    out: optional preallocated result of that shape whose pixels are dense rows of a [pixels, ldo] buffer -- channel stride 1, row
    stride ldo >= channels, ldo % 4 == 0 (the ABI's rule); columns [channels, ldo) are not written.  resid then has out's strides
    (the kernels read it at out's offsets)."""
    _need(x, torch.bfloat16, "conv_cl.x")
    _need(w, torch.bfloat16, "conv_cl.w")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("conv_cl.x must be contiguous [T,H,W,C]")
    T, H, W, Cin = x.shape
    To, Ho, Wo = out_thw
    nh = 0
    if hist is not None:
        _need(hist, torch.bfloat16, "conv_cl.hist")
        if not hist.is_contiguous() or tuple(hist.shape[1:]) != (H, W, Cin):
            raise ValueError("conv_cl.hist must be contiguous [n,H,W,Cin]")
        nh = hist.shape[0]
    if bias is not None:
        _need(bias, torch.float32, "conv_cl.bias")
    ch = cout // 2 if time_interleave else cout
    shape = ((2 * To if time_interleave else To), Ho, Wo, ch)
    ldo = ch
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.bfloat16)
    else:
        _need(out, torch.bfloat16, "conv_cl.out")
        if tuple(out.shape) != shape:
            raise ValueError(f"conv_cl.out must have shape {shape}, got {tuple(out.shape)}")
        ldo = out.stride(2)
        want = (Ho * Wo * ldo, Wo * ldo, ldo, 1)
        if ldo < ch or ldo % 4 != 0 or any(n > 1 and a != b for n, a, b in zip(shape[:2], out.stride(), want)) or out.stride(3) != 1:
            raise ValueError(f"conv_cl.out: pixels must be dense rows of a [pixels, ldo] buffer with ldo >= {ch} and ldo % 4 == 0, "
                             f"got strides {tuple(out.stride())}")
    if resid is not None:
        _need(resid, torch.bfloat16, "conv_cl.resid")
        if resid.shape != out.shape or any(n > 1 and a != b for n, a, b in zip(out.shape, resid.stride(), out.stride())):
            raise ValueError("conv_cl.resid must match the output (shape and strides)")
    p = _lib.ConvParams(T, H, W, Cin, To, Ho, Wo, cout, kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2],
                        pad[0], pad[1], pad[2], int(upsample2x), int(time_interleave))
    lib = _lib.load()
    _lib.check(lib.wan_conv_cl(_p(x), _p(hist), nh, _p(w), w.stride(0), _p(bias), _p(resid), _p(out), ldo,
                               ctypes.byref(p), _stream()), "wan_conv_cl")
    return out


@_on_tensor_device
def rmsnorm_silu_cl(x: torch.Tensor, gamma: torch.Tensor, silu: bool) -> torch.Tensor:
    _need(x, torch.bfloat16, "rmsnorm_silu_cl.x")
    _need(gamma, torch.float32, "rmsnorm_silu_cl.gamma")
    if not x.is_contiguous():
        raise ValueError("rmsnorm_silu_cl.x must be contiguous")
    C = x.shape[-1]
    out = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.wan_rmsnorm_silu_cl(_p(x), _p(gamma), _p(out), x.numel() // C, C, int(silu), _stream()),
               "wan_rmsnorm_silu_cl")
    return out


@_on_tensor_device
def softmax_rows(scores: torch.Tensor, n: int, npad: int, scale: float) -> torch.Tensor:
    _need(scores, torch.float32, "softmax_rows.scores")
    rows = scores.shape[0]
    out = torch.empty(rows, npad, device=scores.device, dtype=torch.bfloat16)
    lib = _lib.load()
    _lib.check(lib.wan_softmax_rows(_p(scores), scores.stride(0), _p(out), npad, rows, n, npad, float(scale), _stream()),
               "wan_softmax_rows")
    return out


@_on_tensor_device
def video_to_cl(video: torch.Tensor, cpad: int = 8) -> torch.Tensor:
    """[C,T,H,W] fp32|bf16 -> bf16 [T,H,W,cpad] (extra channels zero)."""
    if video.dtype not in (torch.float32, torch.bfloat16):
        video = video.float()
    _need(video, video.dtype, "video_to_cl.video")
    video = video.contiguous()
    C, T, H, W = video.shape
    out = torch.empty(T, H, W, cpad, device=video.device, dtype=torch.bfloat16)
    lib = _lib.load()
    _lib.check(lib.wan_video_to_cl(_p(video), 0 if video.dtype == torch.float32 else 1, _p(out), C, cpad, T * H * W,
                                   _stream()), "wan_video_to_cl")
    return out


@_on_tensor_device
def cl_to_video(x: torch.Tensor, cv: int, out_dtype: torch.dtype, clamp: bool) -> torch.Tensor:
    """bf16 [T,H,W,C>=cv] -> [cv,T,H,W] in out_dtype (fp32|bf16), optional clamp to [-1,1]."""
    _need(x, torch.bfloat16, "cl_to_video.x")
    if not x.is_contiguous():
        raise ValueError("cl_to_video.x must be contiguous")
    T, H, W, C = x.shape
    dt = out_dtype if out_dtype in (torch.float32, torch.bfloat16) else torch.float32
    out = torch.empty(cv, T, H, W, device=x.device, dtype=dt)
    lib = _lib.load()
    _lib.check(lib.wan_cl_to_video(_p(x), C, _p(out), 0 if dt == torch.float32 else 1, cv, T * H * W, int(clamp),
                                   _stream()), "wan_cl_to_video")
    return out.to(out_dtype)


@_on_tensor_device
def frames_u8_to_video(frames: torch.Tensor, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """uint8 [B,T,H,W,3] frames as a video reader yields them -> [B,3,T,H,W] in out_dtype (fp32|bf16),
    ``float32(u) * (2.0 / 255.0) - 1.0`` rounded as the reference's host code rounds it (fast_infer.py:88-90)."""
    _need(frames, torch.uint8, "frames_u8_to_video.frames")
    if frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError(f"frames_u8_to_video.frames: expected [B, T, H, W, 3], got {tuple(frames.shape)}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames_u8_to_video: dtype {out_dtype} not supported (float32 or bfloat16)")
    frames = frames.contiguous()
    B, T, H, W, _ = frames.shape
    out = torch.empty(B, 3, T, H, W, device=frames.device, dtype=out_dtype)
    lib = _lib.load()
    _lib.check(lib.wan_frames_u8_to_video(_p(frames), _p(out), 0 if out_dtype == torch.float32 else 1, B, T, H, W, _stream()),
               "wan_frames_u8_to_video")
    return out


@_on_tensor_device
def video_to_frames_u8(video: torch.Tensor, out: Optional[torch.Tensor] = None, frame_range: Optional[Tuple[int, int]] = None,
                       dst_frame: int = 0) -> torch.Tensor:
    """The decoder's [B,3,T,H,W] (fp32|bf16) -> uint8 [B,T,H,W,3], ``trunc(clamp(x / 2 + 0.5, 0, 1) * 255)`` with the inner
    arithmetic rounded in the video's dtype (pipeline_wan.py:423-428, utils.py:59-68).  ``frame_range`` = (first, end) picks
    frames of ``video``; ``out`` = a contiguous uint8 [B,T_out,H,W,3] device clip that receives them from frame ``dst_frame`` on
    (returned as given); without ``out`` a clip of exactly the chosen frames is allocated."""
    if video.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"video_to_frames_u8.video: expected float32 or bfloat16, got {video.dtype}")
    _need(video, video.dtype, "video_to_frames_u8.video")
    if video.dim() != 5 or video.shape[1] != 3:
        raise ValueError(f"video_to_frames_u8.video: expected [B, 3, T, H, W], got {tuple(video.shape)}")
    video = video.contiguous()
    B, _, T, H, W = video.shape
    t0, t1 = (0, T) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
    if not 0 <= t0 <= t1 <= T:
        raise ValueError(f"video_to_frames_u8: frame_range {(t0, t1)} of {T} frames")
    if out is None:
        if dst_frame != 0:
            raise ValueError("video_to_frames_u8: dst_frame needs `out`")
        out = torch.empty(B, t1 - t0, H, W, 3, device=video.device, dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "video_to_frames_u8.out")
        if out.dim() != 5 or not out.is_contiguous() or out.device != video.device or \
                (out.shape[0], out.shape[2], out.shape[3], out.shape[4]) != (B, H, W, 3):
            raise ValueError(f"video_to_frames_u8.out: expected a contiguous [{B}, T_out, {H}, {W}, 3] on {video.device}, got "
                             f"{tuple(out.shape)} on {out.device}")
        if not 0 <= dst_frame <= out.shape[1] - (t1 - t0):
            raise ValueError(f"video_to_frames_u8: {t1 - t0} frames at dst_frame {dst_frame} of a {out.shape[1]}-frame clip")
    if t1 > t0:
        lib = _lib.load()
        _lib.check(lib.wan_video_to_frames_u8(_p(video), 0 if video.dtype == torch.float32 else 1, _p(out), B, T, H, W,
                                              t0, t1 - t0, out.shape[1], int(dst_frame), _stream()), "wan_video_to_frames_u8")
    return out


def _pixel_box(box, name: str, what: str = "box"):
    if not hasattr(box, "__len__") or len(box) != 4:
        raise ValueError(f"{name}: {what} = (y, x, h, w) in pixels, got {box!r}")
    return tuple(int(v) for v in box)


@_on_tensor_device
def frames_u8_box_to_video(frames: torch.Tensor, box, out_dtype: torch.dtype = torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The box ``box`` = (y, x, h, w) in pixels of uint8 [B,T,H,W,3] frames -> [B,3,T,h,w] in out_dtype (fp32|bf16) in ONE launch
    (``wan_frames_u8_box_to_video``): ``frames_u8_to_video``'s arithmetic on the box only, and with the whole-frame box its bits.
    Any box inside the frame; ``out``: a contiguous tensor of that shape and dtype to write into."""
    _need(frames, torch.uint8, "frames_u8_box_to_video.frames")
    if frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError(f"frames_u8_box_to_video.frames: expected [B, T, H, W, 3], got {tuple(frames.shape)}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames_u8_box_to_video: dtype {out_dtype} not supported (float32 or bfloat16)")
    by, bx, bh, bw = _pixel_box(box, "frames_u8_box_to_video")
    frames = frames.contiguous()
    B, T, H, W, _ = (int(v) for v in frames.shape)
    shape = (B, 3, T, max(bh, 0), max(bw, 0))
    if out is None:
        out = torch.empty(shape, device=frames.device, dtype=out_dtype)
    elif tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"frames_u8_box_to_video.out: {out.dtype} {tuple(out.shape)} on {out.device} for contiguous {out_dtype} "
                         f"{shape} on {frames.device}")
    _lib.check(_lib.load().wan_frames_u8_box_to_video(_p(frames), _p(out), 0 if out_dtype == torch.float32 else 1, B, T, H, W, by, bx,
                                                      bh, bw, _stream()), "wan_frames_u8_box_to_video")
    return out


@_on_tensor_device
def video_box_stitch_u8(video: torch.Tensor, source: torch.Tensor, box, rect, feather: int = 0, out: Optional[torch.Tensor] = None,
                        frame_range: Optional[Tuple[int, int]] = None, dst_frame: int = 0, src_frame: int = 0) -> torch.Tensor:
    """The decoder's output on the box, ``video`` [B,3,T,bh,bw] (fp32|bf16), stitched into the uint8 ``source`` frames [Bs,Ts,H,W,3]
    (Bs = 1 or B) in ONE launch (``wan_video_box_stitch_u8``): uint8 [B,T_out,H,W,3] frames that are the source's bytes outside the
    rectangle ``rect`` = (y, x, h, w) (frame pixels, inside ``box`` = (y, x, bh, bw)) and inside it the decoder's bytes
    (``video_to_frames_u8``'s conversion), blended over the source along a linear ramp of ``feather`` pixels on the inside of every
    edge of the rectangle that is not the frame's border (edit_region.reference_video_box_stitch is the definition; 0 = the literal
    stitch).  ``frame_range`` = (first, end) picks frames of ``video``; they stitch against the source frames from ``src_frame`` on and
    land in ``out`` (a contiguous uint8 [B,T_out,H,W,3] device clip, not overlapping ``source``; returned as given) from frame
    ``dst_frame`` on; without ``out`` a clip of exactly the chosen frames is allocated."""
    if video.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"video_box_stitch_u8.video: expected float32 or bfloat16, got {video.dtype}")
    _need(video, video.dtype, "video_box_stitch_u8.video")
    _need(source, torch.uint8, "video_box_stitch_u8.source")
    if video.dim() != 5 or video.shape[1] != 3:
        raise ValueError(f"video_box_stitch_u8.video: expected [B, 3, T, bh, bw], got {tuple(video.shape)}")
    if source.dim() != 5 or source.shape[-1] != 3 or source.device != video.device:
        raise ValueError(f"video_box_stitch_u8.source: expected uint8 [Bs, Ts, H, W, 3] on {video.device}, got {tuple(source.shape)} "
                         f"on {source.device}")
    video, source = video.contiguous(), source.contiguous()
    B, _, T, vh, vw = (int(v) for v in video.shape)
    Bs, Ts, H, W, _ = (int(v) for v in source.shape)
    by, bx, bh, bw = _pixel_box(box, "video_box_stitch_u8")
    ry, rx, rh, rw = _pixel_box(rect, "video_box_stitch_u8", "rect")
    if (bh, bw) != (vh, vw):
        raise ValueError(f"video_box_stitch_u8: a box of {bh} x {bw} pixels for decoder frames of {vh} x {vw}")
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)):
        raise ValueError(f"video_box_stitch_u8: feather={feather!r} is not an integer pixel count")
    t0, t1 = (0, T) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
    if not 0 <= t0 <= t1 <= T:
        raise ValueError(f"video_box_stitch_u8: frame_range {(t0, t1)} of {T} frames")
    if out is None:
        if dst_frame != 0:
            raise ValueError("video_box_stitch_u8: dst_frame needs `out`")
        out = torch.empty(B, t1 - t0, H, W, 3, device=video.device, dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "video_box_stitch_u8.out")
        if out.dim() != 5 or not out.is_contiguous() or out.device != video.device or \
                (out.shape[0], out.shape[2], out.shape[3], out.shape[4]) != (B, H, W, 3):
            raise ValueError(f"video_box_stitch_u8.out: expected a contiguous [{B}, T_out, {H}, {W}, 3] on {video.device}, got "
                             f"{tuple(out.shape)} on {out.device}")
    _lib.check(_lib.load().wan_video_box_stitch_u8(_p(video), 0 if video.dtype == torch.float32 else 1, _p(source), _p(out), B, Bs, T, Ts,
                                                   int(out.shape[1]), H, W, by, bx, bh, bw, ry, rx, rh, rw, int(feather), t0, t1 - t0,
                                                   int(src_frame), int(dst_frame), _stream()), "wan_video_box_stitch_u8")
    return out


@_on_tensor_device
def frames_u8_resample(frames: torch.Tensor, out_height: int, out_width: int, xtab: torch.Tensor, kx: int, ytab: torch.Tensor,
                       ky: int) -> torch.Tensor:
    """uint8 [B,T,H,W,3] -> uint8 [B,T,out_height,out_width,3]: the integer antialiased-triangle resample and crop of
    ``wan_frames_u8_resample``.  ``xtab`` / ``ytab``: the int32 device tables of include/wan_hip.h for ``out_width`` / ``out_height``
    output indices with ``kx`` / ``ky`` taps (video_io.resample_axis_table builds them)."""
    _need(frames, torch.uint8, "frames_u8_resample.frames")
    if frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError(f"frames_u8_resample.frames: expected [B, T, H, W, 3], got {tuple(frames.shape)}")
    frames = frames.contiguous()
    B, T, H, W, _ = frames.shape
    lib = _lib.load()
    for name, tab, n_out, k in (("xtab", xtab, out_width, kx), ("ytab", ytab, out_height, ky)):
        _need(tab, torch.int32, f"frames_u8_resample.{name}")
        if tab.device != frames.device or not tab.is_contiguous() or \
                tab.numel() * 4 != lib.wan_frames_resample_table_bytes(int(n_out), int(k)):
            raise ValueError(f"frames_u8_resample.{name}: expected {n_out} * (2 + {k}) contiguous int32 on {frames.device}, got "
                             f"{tuple(tab.shape)} on {tab.device}")
    out = torch.empty(B, T, int(out_height), int(out_width), 3, device=frames.device, dtype=torch.uint8)
    _lib.check(lib.wan_frames_u8_resample(_p(frames), _p(out), B, T, H, W, int(out_height), int(out_width), _p(xtab), int(kx),
                                          _p(ytab), int(ky), _stream()), "wan_frames_u8_resample")
    return out


_COMPOSE_KIND = {torch.uint8: _lib.COMPOSE_U8, torch.float32: _lib.COMPOSE_F32, torch.bfloat16: _lib.COMPOSE_BF16}
COMPOSE_COPY, COMPOSE_LOADER_ROUNDTRIP, COMPOSE_WRITER, COMPOSE_NORMALIZE = (
    _lib.COMPOSE_COPY, _lib.COMPOSE_LOADER_ROUNDTRIP, _lib.COMPOSE_WRITER, _lib.COMPOSE_NORMALIZE)


@_on_tensor_device
def video_range_flag(x: torch.Tensor) -> torch.Tensor:
    """``_normalize_to_01``'s range rule (fast_infer.py:185-187) over every element of ``x`` (float32 | bfloat16, or uint8 frames
    standing for the loader's float video of them) as an int32 ``[1]`` ON THE DEVICE (``wan_video_range_flag``): 1 = rescale by
    ``(x + 1) / 2``.  Nothing is read back; ``frames_u8_compose`` takes the tensor as a source's ``flag``."""
    if x.dtype not in _COMPOSE_KIND:
        raise ValueError(f"video_range_flag.x: expected uint8, float32 or bfloat16, got {x.dtype}")
    _need(x, x.dtype, "video_range_flag.x")
    x = x.contiguous()
    if x.numel() == 0:
        raise ValueError("video_range_flag.x: empty tensor")
    flag = torch.empty(1, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().wan_video_range_flag(_p(x), _COMPOSE_KIND[x.dtype], x.numel(), _p(flag), _stream()), "wan_video_range_flag")
    return flag


@_on_tensor_device
def frames_u8_compose(canvas: torch.Tensor, sources, pad: int = 0) -> torch.Tensor:
    """Place clips into rectangles of ``canvas`` (a contiguous uint8 [T_out, Hc, Wc, 3] device tensor; EVERY byte of it is written,
    what no source covers with the byte ``pad``) in one launch of ``wan_frames_u8_compose``.  ``sources``: dicts with

        tensor   uint8 [T, H, W, 3] (the three channels of a pixel adjacent) or float32 / bfloat16 [3, T, H, W]; any other strides
        mode     COMPOSE_COPY | COMPOSE_LOADER_ROUNDTRIP (uint8), COMPOSE_WRITER | COMPOSE_NORMALIZE (float): include/wan_hip.h
        window   (t0, y0, x0, nt, h, w) of the tensor; default: all of it
        dst      (y, x) on the canvas; default (0, 0)
        rescale  WRITER's ``rescale``
        flag     the int32 device tensor of ``video_range_flag`` (NORMALIZE: required; LOADER_ROUNDTRIP: optional)
    """
    _need(canvas, torch.uint8, "frames_u8_compose.canvas")
    if canvas.dim() != 4 or canvas.shape[-1] != 3 or not canvas.is_contiguous():
        raise ValueError(f"frames_u8_compose.canvas: expected a contiguous [T, H, W, 3], got {tuple(canvas.shape)}")
    sources = list(sources)
    if len(sources) > _lib.COMPOSE_MAX_SRC:
        raise RuntimeError(f"frames_u8_compose: {len(sources)} sources; the kernel takes {_lib.COMPOSE_MAX_SRC} per canvas")
    arr = (_lib.ComposeSrc * max(len(sources), 1))()
    for k, s in enumerate(sources):
        t = s["tensor"]
        if t.dtype not in _COMPOSE_KIND:
            raise ValueError(f"frames_u8_compose.sources[{k}]: expected uint8, float32 or bfloat16, got {t.dtype}")
        if not t.is_cuda:
            raise RuntimeError(f"frames_u8_compose.sources[{k}]: tensor is on {t.device}; the HIP path has no CPU fallback")
        u8 = t.dtype == torch.uint8
        if t.dim() != 4 or t.shape[-1 if u8 else 0] != 3 or t.device != canvas.device:
            raise ValueError(f"frames_u8_compose.sources[{k}]: expected {'[T, H, W, 3]' if u8 else '[3, T, H, W]'} on {canvas.device}, "
                             f"got {tuple(t.shape)} on {t.device}")
        T, H, W = (t.shape[0], t.shape[1], t.shape[2]) if u8 else (t.shape[1], t.shape[2], t.shape[3])
        st = t.stride()
        d = arr[k]
        d.stride_t, d.stride_y, d.stride_x, d.stride_c = (st[0], st[1], st[2], st[3]) if u8 else (st[1], st[2], st[3], st[0])
        d.base = t.data_ptr()
        d.extent = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        d.kind, d.mode, d.rescale = _COMPOSE_KIND[t.dtype], int(s["mode"]), int(bool(s.get("rescale", False)))
        d.t0, d.y0, d.x0, d.nt, d.h, d.w = (int(v) for v in s.get("window", (0, 0, 0, T, H, W)))
        if d.t0 + d.nt > T or d.y0 + d.h > H or d.x0 + d.w > W:
            raise ValueError(f"frames_u8_compose.sources[{k}]: window {tuple(s['window'])} of a {T} x {H} x {W} clip")
        d.dst_y, d.dst_x = (int(v) for v in s.get("dst", (0, 0)))
        flag = s.get("flag")
        if flag is not None:
            _need(flag, torch.int32, f"frames_u8_compose.sources[{k}].flag")
            if flag.numel() != 1 or flag.device != canvas.device:
                raise ValueError(f"frames_u8_compose.sources[{k}].flag: expected one int32 on {canvas.device}")
            d.rescale_flag = flag.data_ptr()
    T_out, Hc, Wc, _ = canvas.shape
    _lib.check(_lib.load().wan_frames_u8_compose(arr, len(sources), _p(canvas), T_out, Hc, Wc, int(pad), _stream()),
               "wan_frames_u8_compose")
    return canvas


def _yuv_planes(y: torch.Tensor, cb: Optional[torch.Tensor], cr: Optional[torch.Tensor], sub_x: bool, sub_y: bool, cosited: bool,
                what: str) -> "_lib.YuvPlanes":
    """``wan_yuv_planes`` of three strided uint8 views: luma ``[T, H, W]`` (unit column stride), chroma ``[T, Ch, Cw]`` with a column
    stride of 1 (planar) or 2 (interleaved CbCr), both chroma planes with the same strides, or both ``None`` (mono)."""
    _need(y, torch.uint8, what + ".y")
    if y.dim() != 3:
        raise ValueError(f"{what}.y: expected [T, H, W], got {tuple(y.shape)}")
    T, H, W = (int(v) for v in y.shape)
    p = _lib.YuvPlanes()
    p.y, p.y_extent, p.y_frame, p.y_row = y.data_ptr(), _avail(y), y.stride(0), max(y.stride(1), W)
    p.sub_x, p.sub_y, p.cosited, p.c_step = int(bool(sub_x)), int(bool(sub_y)), int(bool(cosited)), 1
    if (cb is None) != (cr is None):
        raise ValueError(f"{what}: pass both chroma planes or neither (mono)")
    if cb is not None:
        ch, cw = ((H + 1) // 2 if sub_y else H), ((W + 1) // 2 if sub_x else W)
        for name, t in (("cb", cb), ("cr", cr)):
            if not t.is_cuda:
                raise RuntimeError(f"{what}.{name}: tensor is on {t.device}; the HIP path has no CPU fallback")
            if t.dtype != torch.uint8 or t.device != y.device or tuple(t.shape) != (T, ch, cw):
                raise ValueError(f"{what}.{name}: expected uint8 [{T}, {ch}, {cw}] on {y.device}, got {t.dtype} {tuple(t.shape)} on "
                                 f"{t.device}")
        step = cb.stride(2) if cw > 1 else 1
        if step not in (1, 2) or (cw > 1 and cr.stride(2) != step) or cb.stride()[:2] != cr.stride()[:2]:
            raise ValueError(f"{what}: chroma strides {cb.stride()} / {cr.stride()}: expected the same for both planes and a column "
                             "stride of 1 (planar) or 2 (interleaved CbCr)")
        p.cb, p.cr, p.cb_extent, p.cr_extent = cb.data_ptr(), cr.data_ptr(), _avail(cb), _avail(cr)
        p.c_frame, p.c_row, p.c_step = cb.stride(0), max(cb.stride(1), (cw - 1) * step + 1), step
    return p


def _yuv_coef(k, yo: int) -> "_lib.YuvCoef":
    k = [int(v) for v in k]
    if len(k) != 9:
        raise ValueError(f"expected the 9 coefficients of a 3 x 3 matrix, got {len(k)}")
    return _lib.YuvCoef((ctypes.c_int * 9)(*k), int(yo))


@_on_tensor_device
def yuv_to_frames_u8(y: torch.Tensor, cb: Optional[torch.Tensor], cr: Optional[torch.Tensor], sub_x: bool, sub_y: bool, cosited: bool,
                     inverse, yo: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """8-bit YCbCr planes -> uint8 [T,H,W,3] RGB frames (``wan_yuv_to_frames_u8``, include/wan_hip.h).  ``y`` [T,H,W], ``cb`` / ``cr``
    [T,Ch,Cw] (or None: mono): strided views of any alignment.  ``inverse``: the 9 fixed-point coefficients, row-major; ``yo``: the luma
    offset.  ``out``: a contiguous uint8 [T,H,W,3] device tensor that receives the frames (returned as given)."""
    planes = _yuv_planes(y, cb, cr, sub_x, sub_y, cosited, "yuv_to_frames_u8")
    T, H, W = (int(v) for v in y.shape)
    if out is None:
        out = torch.empty(T, H, W, 3, device=y.device, dtype=torch.uint8)
    else:
        _need(out, torch.uint8, "yuv_to_frames_u8.out")
        if tuple(out.shape) != (T, H, W, 3) or not out.is_contiguous() or out.device != y.device:
            raise ValueError(f"yuv_to_frames_u8.out: expected a contiguous [{T}, {H}, {W}, 3] on {y.device}, got {tuple(out.shape)} on "
                             f"{out.device}")
    coef = _yuv_coef(inverse, yo)
    _lib.check(_lib.load().wan_yuv_to_frames_u8(ctypes.byref(planes), ctypes.byref(coef), _p(out), T, H, W, _stream()),
               "wan_yuv_to_frames_u8")
    return out


@_on_tensor_device
def frames_u8_to_yuv(frames: torch.Tensor, y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, subsampled: bool, forward,
                     yo: int) -> None:
    """uint8 [T,H,W,3] RGB frames -> 8-bit YCbCr written into the strided views ``y`` [T,H,W], ``cb`` / ``cr`` [T,Ch,Cw]
    (``wan_frames_u8_to_yuv``): 4:2:0 with ``subsampled``, else 4:4:4.  No byte outside the views' rows is written."""
    _need(frames, torch.uint8, "frames_u8_to_yuv.frames")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames_u8_to_yuv.frames: expected [T, H, W, 3], got {tuple(frames.shape)}")
    frames = frames.contiguous()
    T, H, W, _ = (int(v) for v in frames.shape)
    if tuple(y.shape) != (T, H, W) or y.device != frames.device or cb is None or cr is None:
        raise ValueError(f"frames_u8_to_yuv.y: expected [{T}, {H}, {W}] on {frames.device} and both chroma planes, got "
                         f"{tuple(y.shape)} on {y.device}")
    planes = _yuv_planes(y, cb, cr, subsampled, subsampled, False, "frames_u8_to_yuv")
    coef = _yuv_coef(forward, yo)
    _lib.check(_lib.load().wan_frames_u8_to_yuv(_p(frames), ctypes.byref(planes), ctypes.byref(coef), T, H, W, _stream()),
               "wan_frames_u8_to_yuv")


@_on_tensor_device
def change_mask(source: torch.Tensor, edit: torch.Tensor, threshold: int, smooth: int, grow: int, grow_t: int,
                feather: int) -> torch.Tensor:
    """uint8 [B,T,H,W,3] source and edit frames -> the feathered uint8 [B,T,H,W] mask of where they differ (``wan_change_mask``,
    include/wan_hip.h: three launches, integer arithmetic).  The b / g planes live in a workspace allocated here."""
    _need(source, torch.uint8, "change_mask.source")
    _need(edit, torch.uint8, "change_mask.edit")
    if source.dim() != 5 or source.shape[-1] != 3 or edit.shape != source.shape or edit.device != source.device:
        raise ValueError(f"change_mask: expected two [B, T, H, W, 3] clips of one shape on one device, got {tuple(source.shape)} on "
                         f"{source.device} and {tuple(edit.shape)} on {edit.device}")
    source, edit = source.contiguous(), edit.contiguous()
    B, T, H, W, _ = (int(v) for v in source.shape)
    lib = _lib.load()
    nws = int(lib.wan_change_mask_workspace_bytes(B, T, H, W))
    ws = torch.empty(max(nws, 1), device=source.device, dtype=torch.uint8)
    alpha = torch.empty(B, T, H, W, device=source.device, dtype=torch.uint8)
    _lib.check(lib.wan_change_mask(_p(source), _p(edit), _p(alpha), B, T, H, W, int(threshold), int(smooth), int(grow), int(grow_t),
                                   int(feather), _p(ws), nws, _stream()), "wan_change_mask")
    return alpha


@_on_tensor_device
def plane_u8_resample(planes: torch.Tensor, out_height: int, out_width: int, xtab: torch.Tensor, kx: int, ytab: torch.Tensor,
                      ky: int) -> torch.Tensor:
    """uint8 [N,H,W] -> uint8 [N,out_height,out_width]: ``frames_u8_resample``'s two passes and tables on one-channel planes
    (``wan_plane_u8_resample``); the horizontal pass' bytes go through a temporary allocated here."""
    _need(planes, torch.uint8, "plane_u8_resample.planes")
    if planes.dim() != 3:
        raise ValueError(f"plane_u8_resample.planes: expected [N, H, W], got {tuple(planes.shape)}")
    planes = planes.contiguous()
    N, H, W = (int(v) for v in planes.shape)
    lib = _lib.load()
    for name, tab, n_out, k in (("xtab", xtab, out_width, kx), ("ytab", ytab, out_height, ky)):
        _need(tab, torch.int32, f"plane_u8_resample.{name}")
        if tab.device != planes.device or not tab.is_contiguous() or \
                tab.numel() * 4 != lib.wan_frames_resample_table_bytes(int(n_out), int(k)):
            raise ValueError(f"plane_u8_resample.{name}: expected {n_out} * (2 + {k}) contiguous int32 on {planes.device}, got "
                             f"{tuple(tab.shape)} on {tab.device}")
    tmp = torch.empty(N, H, int(out_width), device=planes.device, dtype=torch.uint8)
    out = torch.empty(N, int(out_height), int(out_width), device=planes.device, dtype=torch.uint8)
    _lib.check(lib.wan_plane_u8_resample(_p(planes), _p(tmp), _p(out), N, H, W, int(out_height), int(out_width), _p(xtab), int(kx),
                                         _p(ytab), int(ky), _stream()), "wan_plane_u8_resample")
    return out


@_on_tensor_device
def frames_u8_composite(original: torch.Tensor, edit: torch.Tensor, alpha: torch.Tensor, window: Tuple[int, int, int, int]) -> torch.Tensor:
    """``(a * e + (255 - a) * o + 127) // 255`` per byte inside ``window`` = (y, x, h, w) of the original's frames, the original's
    bytes outside it (``wan_frames_u8_composite``).  original uint8 [N,Ho,Wo,3], edit uint8 [N,h,w,3], alpha uint8 [N,h,w]."""
    for name, t in (("original", original), ("edit", edit), ("alpha", alpha)):
        _need(t, torch.uint8, f"frames_u8_composite.{name}")
    wy, wx, wh, ww = (int(v) for v in window)
    if original.dim() != 4 or original.shape[-1] != 3:
        raise ValueError(f"frames_u8_composite.original: expected [N, H, W, 3], got {tuple(original.shape)}")
    N, Ho, Wo, _ = (int(v) for v in original.shape)
    if tuple(edit.shape) != (N, wh, ww, 3) or tuple(alpha.shape) != (N, wh, ww) or edit.device != original.device or \
            alpha.device != original.device:
        raise ValueError(f"frames_u8_composite: window {(wy, wx, wh, ww)} of {N} frames needs edit [{N}, {wh}, {ww}, 3] and alpha "
                         f"[{N}, {wh}, {ww}] on {original.device}, got {tuple(edit.shape)} on {edit.device} and {tuple(alpha.shape)} on "
                         f"{alpha.device}")
    original, edit, alpha = original.contiguous(), edit.contiguous(), alpha.contiguous()
    out = torch.empty_like(original)
    _lib.check(_lib.load().wan_frames_u8_composite(_p(original), _p(edit), _p(alpha), _p(out), N, Ho, Wo, wy, wx, wh, ww, _stream()),
               "wan_frames_u8_composite")
    return out


CLIP_STATS_WORDS = 514             # WAN_CLIP_STATS_WORDS of include/wan_hip.h


@_on_tensor_device
def clip_stats(a: torch.Tensor, b: torch.Tensor, alpha: Optional[torch.Tensor], smooth: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two uint8 [B,T,H,W,3] clips and an optional uint8 [B,T,H,W] mask -> int64 [B,T,2,514] on the device: per frame and region
    (alpha == 0, alpha != 0) the histogram of byte differences, the histogram of the smoothed pixel difference and the SSIM sum and
    window count (``wan_clip_stats``, include/wan_hip.h: four launches, exact integers).  ``out``: a contiguous int64 tensor of that
    shape, every word of which is overwritten.  The workgroups' partial counts live in a workspace allocated here."""
    _need(a, torch.uint8, "clip_stats.a")
    _need(b, torch.uint8, "clip_stats.b")
    if a.dim() != 5 or a.shape[-1] != 3 or b.shape != a.shape or b.device != a.device:
        raise ValueError(f"clip_stats: expected two [B, T, H, W, 3] clips of one shape on one device, got {tuple(a.shape)} on "
                         f"{a.device} and {tuple(b.shape)} on {b.device}")
    a, b = a.contiguous(), b.contiguous()
    B, T, H, W, _ = (int(v) for v in a.shape)
    if alpha is not None:
        _need(alpha, torch.uint8, "clip_stats.alpha")
        if tuple(alpha.shape) != (B, T, H, W) or alpha.device != a.device:
            raise ValueError(f"clip_stats.alpha: expected [{B}, {T}, {H}, {W}] on {a.device}, got {tuple(alpha.shape)} on {alpha.device}")
        alpha = alpha.contiguous()
    if out is None:
        out = torch.empty(B, T, 2, CLIP_STATS_WORDS, device=a.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, T, 2, CLIP_STATS_WORDS) or out.device != a.device or not out.is_contiguous():
        raise ValueError(f"clip_stats.out: expected contiguous int64 [{B}, {T}, 2, {CLIP_STATS_WORDS}] on {a.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    lib = _lib.load()
    nws = int(lib.wan_clip_stats_workspace_bytes(B * T, H, W))
    ws = torch.empty(max(nws, 1), device=a.device, dtype=torch.uint8)
    _lib.check(lib.wan_clip_stats(_p(a), _p(b), _p(alpha), _p(out), B * T, H, W, int(smooth), _p(ws), nws, _stream()),
               "wan_clip_stats")
    return out


COLOR_STATS_WORDS, COLOR_ONE, COLOR_MAX_POOL_T = 16, 4096, 8             # WAN_COLOR_* of include/wan_hip.h


@_on_tensor_device
def color_stats(ref: torch.Tensor, edit: torch.Tensor, alpha: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ref uint8 [B,T,H,W,3] or [B,1,H,W,3], edit uint8 [B,T,H,W,3], alpha uint8 of ref's [B,.,H,W] or None -> int64 [B,T,16] on the
    device: per frame n, then (A, E, AA, EE) per channel over the pixels whose alpha is 0, three zero words (``wan_color_stats``,
    include/wan_hip.h: two launches, exact integers).  ``out``: a contiguous int64 tensor of that shape, every word of which is
    overwritten.  The workgroups' partial sums live in a workspace allocated here."""
    _need(ref, torch.uint8, "color_stats.ref")
    _need(edit, torch.uint8, "color_stats.edit")
    if edit.dim() != 5 or edit.shape[-1] != 3:
        raise ValueError(f"color_stats.edit: expected [B, T, H, W, 3], got {tuple(edit.shape)}")
    B, T, H, W, _ = (int(v) for v in edit.shape)
    if ref.dim() != 5 or tuple(ref.shape) not in ((B, T, H, W, 3), (B, 1, H, W, 3)) or ref.device != edit.device:
        raise ValueError(f"color_stats.ref: expected [{B}, {T}, {H}, {W}, 3] or [{B}, 1, {H}, {W}, 3] on {edit.device}, got "
                         f"{tuple(ref.shape)} on {ref.device}")
    ref_T = int(ref.shape[1])
    ref, edit = ref.contiguous(), edit.contiguous()
    if alpha is not None:
        _need(alpha, torch.uint8, "color_stats.alpha")
        if tuple(alpha.shape) != (B, ref_T, H, W) or alpha.device != edit.device:
            raise ValueError(f"color_stats.alpha: expected [{B}, {ref_T}, {H}, {W}] on {edit.device}, got {tuple(alpha.shape)} on "
                             f"{alpha.device}")
        alpha = alpha.contiguous()
    if out is None:
        out = torch.empty(B, T, COLOR_STATS_WORDS, device=edit.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, T, COLOR_STATS_WORDS) or out.device != edit.device or not out.is_contiguous():
        raise ValueError(f"color_stats.out: expected contiguous int64 [{B}, {T}, {COLOR_STATS_WORDS}] on {edit.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    lib = _lib.load()
    nws = int(lib.wan_color_stats_workspace_bytes(B * T, H, W))
    ws = torch.empty(max(nws, 1), device=edit.device, dtype=torch.uint8)
    _lib.check(lib.wan_color_stats(_p(ref), _p(edit), _p(alpha), _p(out), B, T, ref_T, H, W, _p(ws), nws, _stream()), "wan_color_stats")
    return out


@_on_tensor_device
def color_coef(stats: torch.Tensor, pool_t: int, gain: bool, min_pixels: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [B,T,16] sums of ``color_stats`` -> int32 [B,T,3,2] = (g, b) per frame and channel (``wan_color_coef``: the sums pooled
    over ``pool_t`` frames either side within a sample, 128-bit variances, integer division and square root; one launch)."""
    _need(stats, torch.int64, "color_coef.stats")
    if stats.dim() != 3 or stats.shape[-1] != COLOR_STATS_WORDS or not stats.is_contiguous():
        raise ValueError(f"color_coef.stats: expected contiguous int64 [B, T, {COLOR_STATS_WORDS}], got {tuple(stats.shape)}")
    B, T = int(stats.shape[0]), int(stats.shape[1])
    if out is None:
        out = torch.empty(B, T, 3, 2, device=stats.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, T, 3, 2) or out.device != stats.device or not out.is_contiguous():
        raise ValueError(f"color_coef.out: expected contiguous int32 [{B}, {T}, 3, 2] on {stats.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    _lib.check(_lib.load().wan_color_coef(_p(stats), _p(out), B, T, int(pool_t), int(bool(gain)), int(min_pixels), _stream()),
               "wan_color_coef")
    return out


@_on_tensor_device
def frames_u8_affine(frames: torch.Tensor, coef: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``clamp((g * x + b + 2048) >> 12, 0, 255)`` per byte of uint8 [N,H,W,3] frames with int32 [N,3,2] = (g, b) per frame and
    channel (``wan_frames_u8_affine``, one launch).  ``out``: a contiguous uint8 tensor of the frames' shape; it may be ``frames``."""
    _need(frames, torch.uint8, "frames_u8_affine.frames")
    _need(coef, torch.int32, "frames_u8_affine.coef")
    if frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f"frames_u8_affine.frames: expected contiguous [N, H, W, 3], got {tuple(frames.shape)}")
    N, H, W, _ = (int(v) for v in frames.shape)
    if tuple(coef.shape) != (N, 3, 2) or coef.device != frames.device or not coef.is_contiguous():
        raise ValueError(f"frames_u8_affine.coef: expected contiguous [{N}, 3, 2] on {frames.device}, got {tuple(coef.shape)} on "
                         f"{coef.device}")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"frames_u8_affine.out: expected contiguous uint8 {tuple(frames.shape)} on {frames.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    _lib.check(_lib.load().wan_frames_u8_affine(_p(frames), _p(coef), _p(out), N, H, W, _stream()), "wan_frames_u8_affine")
    return out


@_on_tensor_device
def lincomb(terms, out_dtype: torch.dtype) -> torch.Tensor:
    """sum_i c_i * x_i over <= 4 same-shape CUDA tensors in one pass (fp32 accumulate); `terms` is a list
    of (coefficient, tensor).  Inputs are brought to `out_dtype` (fp32 or bf16) if they differ."""
    terms = [(float(c), t) for c, t in terms if t is not None and c != 0.0]
    if not terms or len(terms) > 4:
        raise ValueError("lincomb needs 1..4 non-zero terms")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"lincomb: dtype {out_dtype} not supported")
    xs = []
    for _, t in terms:
        _need(t, t.dtype, "lincomb.x")
        xs.append(t.to(out_dtype).contiguous())
    out = torch.empty_like(xs[0])
    cs = [c for c, _ in terms] + [0.0] * (4 - len(terms))
    ps = [_p(x) for x in xs] + [None] * (4 - len(xs))
    lib = _lib.load()
    _lib.check(lib.wan_lincomb(_p(out), 0 if out_dtype == torch.float32 else 1, ps[0], ps[1], ps[2], ps[3],
                               cs[0], cs[1], cs[2], cs[3], out.numel(), _stream()), "wan_lincomb")
    return out


solver_step_launches = 0          # wan_solver_step launches so far (read by the tests that count launches per scheduler step)


@_on_tensor_device
def solver_step(sample: torch.Tensor, v: torch.Tensor, a_s: float, a_v: float, m1: Optional[torch.Tensor],
                m2: Optional[torch.Tensor], noise: Optional[torch.Tensor], c_s: float, c_0: float, c_1: float, c_2: float,
                c_n: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """One flow DPM-Solver++ step in one pass (``wan_solver_step``): returns ``(x0, prev)`` with
    x0 = a_s*sample + a_v*v in the latents' dtype and prev = c_s*sample + c_0*x0 + c_1*m1 + c_2*m2 + c_n*noise (x0 as stored,
    fp32 accumulate, written in the latents' dtype).  sample, v, m1, m2: same shape, all fp32 or all bf16; noise fp32 or None;
    m1 / m2 may be None."""
    global solver_step_launches
    dt = sample.dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise ValueError(f"solver_step: dtype {dt} not supported (fp32 or bf16)")
    xs = []
    for name, t, want in (("sample", sample, dt), ("v", v, dt), ("m1", m1, dt), ("m2", m2, dt), ("noise", noise, torch.float32)):
        if t is None:
            xs.append(None)
            continue
        _need(t, want, "solver_step." + name)
        if t.shape != sample.shape:
            raise ValueError(f"solver_step.{name}: shape {tuple(t.shape)} != sample {tuple(sample.shape)}")
        xs.append(t.contiguous())
    x0 = torch.empty(sample.shape, device=sample.device, dtype=dt)
    prev = torch.empty_like(x0)
    if x0.numel() == 0:
        return x0, prev                          # (an empty tensor has no storage to point at: nothing to launch)
    lib = _lib.load()
    _lib.check(lib.wan_solver_step(_p(x0), _p(prev), 0 if dt == torch.float32 else 1, *[_p(t) for t in xs],
                                   float(a_s), float(a_v), float(c_s), float(c_0), float(c_1), float(c_2), float(c_n),
                                   x0.numel(), _stream()), "wan_solver_step")
    solver_step_launches += 1
    return x0, prev


# ------------------------------------------------------------------ temporal context windows (videocof_amd/windows.py)
def _window_args(starts, frames: int, window: int, ground: int, name: str):
    starts = [int(a) for a in starts]
    if not starts:
        raise ValueError(f"{name}: no windows")
    return (ctypes.c_int * len(starts))(*starts), len(starts), int(frames), int(window), int(ground)


@_on_tensor_device
def window_gather(state: torch.Tensor, starts, window: int, ground: int, k0: int = 0, k1: Optional[int] = None, rep: int = 1,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Windows [k0, k1) of the loop state [B, C, Fs + K*G + Fs, h, w] = [source | ground_0 .. ground_{K-1} | target] as the model's
    input batch [rep * (k1 - k0) * B, C, n + G + n, h, w] in ONE launch (``wan_window_gather``): window k is
    [source[a_k : a_k + n] | ground_k | target[a_k : a_k + n]], the batch reads [rep][window][sample].  fp32 or bf16."""
    if state.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"window_gather: dtype {state.dtype} not supported (fp32 or bf16)")
    _need(state, state.dtype, "window_gather.state")
    if state.dim() != 5 or not state.is_contiguous():
        raise ValueError(f"window_gather.state: a contiguous [B, C, F, h, w] tensor, got {tuple(state.shape)}")
    B, C, Ftot, h, w = state.shape
    K = len(starts)
    if (Ftot - K * int(ground)) % 2 or Ftot - K * int(ground) < 2:
        raise ValueError(f"window_gather.state: {Ftot} frames are not [Fs | {K} x {ground} | Fs]")
    arr, K, Fs, n, G = _window_args(starts, (Ftot - K * int(ground)) // 2, window, ground, "window_gather")
    k1 = K if k1 is None else int(k1)
    nk = max(k1 - int(k0), 0)
    shape = (int(rep) * nk * B, C, 2 * n + G, h, w)
    if out is None:
        out = torch.empty(shape, device=state.device, dtype=state.dtype)
    elif tuple(out.shape) != shape or out.dtype != state.dtype or not out.is_contiguous() or out.device != state.device:
        raise ValueError(f"window_gather.out: {out.dtype} {tuple(out.shape)} for {state.dtype} {shape}")
    _lib.check(_lib.load().wan_window_gather(_p(out), _p(state), 0 if state.dtype == torch.float32 else 1, arr, K, int(k0), k1,
                                             B, C, Fs, n, G, h * w, int(rep), nk * B * C * (2 * n + G) * h * w, _stream()),
               "wan_window_gather")
    return out


@_on_tensor_device
def window_blend(pred: torch.Tensor, alpha: torch.Tensor, starts, frames: int, ground: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The K window predictions [K * B, C, n + G + n, h, w] (window-major, after guidance) as the prediction for the loop state
    [B, C, Fs + K*G + Fs, h, w] in ONE launch (``wan_window_blend``): source frames 0, ground_k = window k's grounding block,
    target frame f = sum_k alpha[k, f] * pred_k[f - a_k] over the covering windows in ascending k -- float32, every product and
    sum rounded on its own.  ``alpha``: device float32 [K, Fs] (``window_plan(...).alpha``).  fp32 or bf16, in and out alike."""
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"window_blend: dtype {pred.dtype} not supported (fp32 or bf16)")
    _need(pred, pred.dtype, "window_blend.pred")
    _need(alpha, torch.float32, "window_blend.alpha")
    if pred.dim() != 5 or not pred.is_contiguous():
        raise ValueError(f"window_blend.pred: a contiguous [K * B, C, F, h, w] tensor, got {tuple(pred.shape)}")
    KB, C, Fw, h, w = pred.shape
    if (Fw - int(ground)) % 2 or Fw - int(ground) < 2:
        raise ValueError(f"window_blend.pred: {Fw} frames are not [n | {ground} | n]")
    arr, K, Fs, n, G = _window_args(starts, frames, (Fw - int(ground)) // 2, ground, "window_blend")
    if KB % K:
        raise ValueError(f"window_blend.pred: {KB} samples for {K} windows")
    if tuple(alpha.shape) != (K, Fs) or not alpha.is_contiguous() or alpha.device != pred.device:
        raise ValueError(f"window_blend.alpha: {tuple(alpha.shape)} on {alpha.device} for [{K}, {Fs}] on {pred.device}")
    B = KB // K
    shape = (B, C, 2 * Fs + K * G, h, w)
    if out is None:
        out = torch.empty(shape, device=pred.device, dtype=pred.dtype)
    elif tuple(out.shape) != shape or out.dtype != pred.dtype or not out.is_contiguous() or out.device != pred.device:
        raise ValueError(f"window_blend.out: {out.dtype} {tuple(out.shape)} for {pred.dtype} {shape}")
    _lib.check(_lib.load().wan_window_blend(_p(out), _p(pred), 0 if pred.dtype == torch.float32 else 1, _p(alpha), arr, K, B, C,
                                            Fs, n, G, h * w, _stream()), "wan_window_blend")
    return out


# ------------------------------------------------------------------ spatial context windows (videocof_amd/windows.py, TilePlan)
def _tile_starts(starts, name: str):
    if len(starts) != 3:
        raise ValueError(f"{name}: starts = (t_starts, y_starts, x_starts), got {len(starts)} entries")
    axes = [[int(a) for a in s] for s in starts]
    if not all(axes):
        raise ValueError(f"{name}: an axis without windows")
    return [(ctypes.c_int * len(a))(*a) for a in axes], [len(a) for a in axes]


@_on_tensor_device
def tile_gather(state: torch.Tensor, starts, tile, ground: int, k0: int = 0, k1: Optional[int] = None, rep: int = 1,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tiles [k0, k1) of the loop state [B, C, Fs + Kt*G + Fs, H, W] = [source | ground_0 .. ground_{Kt-1} | target] as the model's
    input batch [rep * (k1 - k0) * B, C, n + G + n, th, tw] in ONE launch (``wan_tile_gather``).  ``starts`` = (t_starts, y_starts,
    x_starts), ``tile`` = (n, th, tw), all in latent cells (``TilePlan``); tile k = (kt * Ky + ky) * Kx + kx is
    [source[a_t : a_t + n, tile] | ground_kt[:, tile] | target[a_t : a_t + n, tile]].  fp32 or bf16."""
    if state.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"tile_gather: dtype {state.dtype} not supported (fp32 or bf16)")
    _need(state, state.dtype, "tile_gather.state")
    if state.dim() != 5 or not state.is_contiguous():
        raise ValueError(f"tile_gather.state: a contiguous [B, C, F, H, W] tensor, got {tuple(state.shape)}")
    B, C, Ftot, H, W = state.shape
    arrs, (Kt, Ky, Kx) = _tile_starts(starts, "tile_gather")
    n, th, tw = (int(v) for v in tile)
    G = int(ground)
    if (Ftot - Kt * G) % 2 or Ftot - Kt * G < 2:
        raise ValueError(f"tile_gather.state: {Ftot} frames are not [Fs | {Kt} x {G} | Fs]")
    Fs = (Ftot - Kt * G) // 2
    k1 = Kt * Ky * Kx if k1 is None else int(k1)
    nk = max(k1 - int(k0), 0)
    shape = (int(rep) * nk * B, C, 2 * n + G, th, tw)
    if min(shape[2:]) < 1:
        raise ValueError(f"tile_gather: tile {(n, th, tw)} with {G} grounding frames")
    if out is None:
        out = torch.empty(shape, device=state.device, dtype=state.dtype)
    elif tuple(out.shape) != shape or out.dtype != state.dtype or not out.is_contiguous() or out.device != state.device:
        raise ValueError(f"tile_gather.out: {out.dtype} {tuple(out.shape)} for {state.dtype} {shape}")
    _lib.check(_lib.load().wan_tile_gather(_p(out), _p(state), 0 if state.dtype == torch.float32 else 1, *arrs, Kt, Ky, Kx, int(k0), k1,
                                           B, C, Fs, H, W, n, th, tw, G, int(rep), nk * B * C * (2 * n + G) * th * tw, _stream()),
               "wan_tile_gather")
    return out


@_on_tensor_device
def tile_blend(pred: torch.Tensor, tables, starts, extent, ground: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The K = Kt * Ky * Kx tile predictions [K * B, C, n + G + n, th, tw] (tile-major, after guidance) as the prediction for the
    loop state [B, C, Fs + Kt*G + Fs, H, W] in ONE launch (``wan_tile_blend``): source frames 0; a grounding frame of block kt and a
    target frame at (y, x) = the sum over the covering tiles in ascending k of w * p, w = (at * ay) * ax -- float32, every product
    and sum rounded on its own (at = 1 for grounding frames).  ``tables`` = (at [Kt, Fs], ay [Ky, H], ax [Kx, W]): device float32,
    the three axes' ``window_plan(...).alpha``; ``starts`` = (t_starts, y_starts, x_starts); ``extent`` = (Fs, H, W)."""
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"tile_blend: dtype {pred.dtype} not supported (fp32 or bf16)")
    _need(pred, pred.dtype, "tile_blend.pred")
    if pred.dim() != 5 or not pred.is_contiguous():
        raise ValueError(f"tile_blend.pred: a contiguous [K * B, C, F, th, tw] tensor, got {tuple(pred.shape)}")
    KB, C, Fw, th, tw = pred.shape
    G = int(ground)
    if (Fw - G) % 2 or Fw - G < 2:
        raise ValueError(f"tile_blend.pred: {Fw} frames are not [n | {G} | n]")
    n = (Fw - G) // 2
    arrs, (Kt, Ky, Kx) = _tile_starts(starts, "tile_blend")
    Fs, H, W = (int(v) for v in extent)
    K = Kt * Ky * Kx
    if KB % K:
        raise ValueError(f"tile_blend.pred: {KB} samples for {K} tiles")
    if len(tables) != 3:
        raise ValueError(f"tile_blend: tables = (at, ay, ax), got {len(tables)} entries")
    for name, tab, shape in zip(("at", "ay", "ax"), tables, ((Kt, Fs), (Ky, H), (Kx, W))):
        _need(tab, torch.float32, f"tile_blend.{name}")
        if tuple(tab.shape) != shape or not tab.is_contiguous() or tab.device != pred.device:
            raise ValueError(f"tile_blend.{name}: {tuple(tab.shape)} on {tab.device} for {list(shape)} on {pred.device}")
    B = KB // K
    shape = (B, C, 2 * Fs + Kt * G, H, W)
    if out is None:
        out = torch.empty(shape, device=pred.device, dtype=pred.dtype)
    elif tuple(out.shape) != shape or out.dtype != pred.dtype or not out.is_contiguous() or out.device != pred.device:
        raise ValueError(f"tile_blend.out: {out.dtype} {tuple(out.shape)} for {pred.dtype} {shape}")
    _lib.check(_lib.load().wan_tile_blend(_p(out), _p(pred), 0 if pred.dtype == torch.float32 else 1, *[_p(t) for t in tables], *arrs,
                                          Kt, Ky, Kx, B, C, Fs, H, W, n, th, tw, G, _stream()), "wan_tile_blend")
    return out


# ------------------------------------------------------------------ umT5 text encoder rows
# ------------------------------------------------------------------ edit inside a mask
LATENT_MASK_MAX_GROW, LATENT_MASK_MAX_GROW_T = 4, 2          # WAN_LATENT_MASK_MAX_* of include/wan_hip.h
LATENT_MASK_RATIOS = (8, 4)                                   # pixels per latent cell, pixel frames per latent frame


@_on_tensor_device
def latent_mask(alpha: torch.Tensor, grow: int, grow_t: int, feather: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A pixel mask uint8 [B,T,H,W] -> latent-cell weights uint8 [B, 1 + ceil((T-1)/4), H/8, W/8] (``wan_latent_mask_u8``,
    include/wan_hip.h: three launches, integer arithmetic).  ``out``: a contiguous uint8 tensor of that shape, every byte of which
    is overwritten.  The two intermediate planes live in a workspace allocated here."""
    _need(alpha, torch.uint8, "latent_mask.alpha")
    if alpha.dim() != 4:
        raise ValueError(f"latent_mask.alpha: expected [B, T, H, W], got {tuple(alpha.shape)}")
    alpha = alpha.contiguous()
    B, T, H, W = (int(v) for v in alpha.shape)
    rs, rt = LATENT_MASK_RATIOS
    shape = (B, 1 + (max(T, 1) - 1 + rt - 1) // rt, H // rs, W // rs)
    if out is None:
        out = torch.empty(shape, device=alpha.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != alpha.device or not out.is_contiguous():
        raise ValueError(f"latent_mask.out: expected contiguous uint8 {shape} on {alpha.device}, got {out.dtype} {tuple(out.shape)} on "
                         f"{out.device}")
    lib = _lib.load()
    nws = int(lib.wan_latent_mask_workspace_bytes(B, T, H, W))
    ws = torch.empty(max(nws, 1), device=alpha.device, dtype=torch.uint8)
    _lib.check(lib.wan_latent_mask_u8(_p(alpha), _p(out), B, T, H, W, rs, rt, int(grow), int(grow_t), int(feather), _p(ws), nws,
                                      _stream()), "wan_latent_mask_u8")
    return out


@_on_tensor_device
def masked_prediction_(pred: torch.Tensor, sample: torch.Tensor, weights: torch.Tensor, Fs: int, target_frame0: int,
                       sigma: float) -> torch.Tensor:
    """IN PLACE on ``pred``, the prediction for the loop state ``sample`` = [B, C, F, h, w] = [source | grounding | target]: outside
    the mask the target's prediction becomes the one whose x0 is the source (``wan_masked_prediction``).  Per element of the target
    frames [target_frame0, target_frame0 + Fs): ``w * v + (1 - w) * ((x_t - s) / sigma)`` with ``w = weights / 255``, float32 with
    every operation rounded on its own; weight 255 leaves the element unwritten.  ``weights``: uint8 [Bm, Fs, h, w], Bm in {1, B},
    shared by the channels.  fp32 or bf16, ``pred`` and ``sample`` alike.  Returns ``pred``."""
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"masked_prediction_: dtype {pred.dtype} not supported (fp32 or bf16)")
    _need(pred, pred.dtype, "masked_prediction_.pred")
    _need(sample, pred.dtype, "masked_prediction_.sample")
    _need(weights, torch.uint8, "masked_prediction_.weights")
    if pred.dim() != 5 or not pred.is_contiguous():
        raise ValueError(f"masked_prediction_.pred: a contiguous [B, C, F, h, w] tensor (it is written in place), got {tuple(pred.shape)}")
    if sample.shape != pred.shape or sample.device != pred.device:
        raise ValueError(f"masked_prediction_.sample: {tuple(sample.shape)} on {sample.device} for the prediction's {tuple(pred.shape)} "
                         f"on {pred.device}")
    B, C, F, h, w = (int(v) for v in pred.shape)
    Fs = int(Fs)
    if weights.dim() != 4 or tuple(weights.shape[1:]) != (Fs, h, w) or int(weights.shape[0]) not in (1, B) or weights.device != pred.device:
        raise ValueError(f"masked_prediction_.weights: expected uint8 [1 or {B}, {Fs}, {h}, {w}] on {pred.device}, got "
                         f"{tuple(weights.shape)} on {weights.device}")
    sample, weights = sample.contiguous(), weights.contiguous()
    _lib.check(_lib.load().wan_masked_prediction(_p(pred), _p(sample), 0 if pred.dtype == torch.float32 else 1, _p(weights), B,
                                                 int(weights.shape[0]), C, F, Fs, int(target_frame0), h * w, float(sigma), _stream()),
               "wan_masked_prediction")
    return pred


# ------------------------------------------------------------------ edit region
def _region_out(out: Optional[torch.Tensor], shape, like: torch.Tensor, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, device=like.device, dtype=like.dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"{name}: {out.dtype} {tuple(out.shape)} on {out.device} for contiguous {like.dtype} {tuple(shape)} on {like.device}")
    return out


@_on_tensor_device
def mask_bounds(weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Latent-cell weights uint8 [Bm, Fs, h, w] -> device int32 [Fs, 4] = (y_lo, y_hi, x_lo, x_hi) per latent frame: the inclusive bounds
    of the non-zero weights over all samples, (h, -1, w, -1) for a frame without one (``wan_mask_bounds``: one workgroup per frame, no
    atomics, every word written once).  Never synchronises: the caller copies the 16 * Fs bytes to the host."""
    _need(weights, torch.uint8, "mask_bounds.weights")
    if weights.dim() != 4 or not weights.is_contiguous():
        raise ValueError(f"mask_bounds.weights: a contiguous uint8 [Bm, Fs, h, w] tensor, got {tuple(weights.shape)}")
    Bm, Fs, h, w = (int(v) for v in weights.shape)
    if out is None:
        out = torch.empty((Fs, 4), device=weights.device, dtype=torch.int32)
    elif tuple(out.shape) != (Fs, 4) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != weights.device:
        raise ValueError(f"mask_bounds.out: {out.dtype} {tuple(out.shape)} on {out.device} for contiguous int32 {(Fs, 4)} on {weights.device}")
    _lib.check(_lib.load().wan_mask_bounds(_p(weights), _p(out), Bm, Fs, h, w, _stream()), "wan_mask_bounds")
    return out


def _region_box(region, name: str):
    if len(region) != 4:
        raise ValueError(f"{name}: region = (y0, x0, h, w) in cells, got {region!r}")
    return tuple(int(v) for v in region)


@_on_tensor_device
def region_crop(x: torch.Tensor, region, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sub-box ``region`` = (y0, x0, h, w) of every frame of a contiguous ``x`` [..., H, W] as a contiguous [..., h, w] tensor in
    ONE launch (``wan_region_crop``); elements of 1, 2 or 4 bytes, bits unchanged.  Serves the loop state and the mask's weights."""
    if not x.is_cuda:
        raise RuntimeError(f"region_crop.x: tensor is on {x.device}; the HIP path has no CPU fallback")
    if x.element_size() not in (1, 2, 4):
        raise ValueError(f"region_crop: dtype {x.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if x.dim() < 2 or not x.is_contiguous():
        raise ValueError(f"region_crop.x: a contiguous [..., H, W] tensor, got {tuple(x.shape)}")
    y0, x0, hr, wr = _region_box(region, "region_crop")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    R = int(math.prod(x.shape[:-2]))
    out = _region_out(out, tuple(x.shape[:-2]) + (max(hr, 0), max(wr, 0)), x, "region_crop.out")
    _lib.check(_lib.load().wan_region_crop(_p(out), _p(x), x.element_size(), R, H, W, y0, x0, hr, wr, _stream()), "wan_region_crop")
    return out


@_on_tensor_device
def region_restore(source: torch.Tensor, state: torch.Tensor, origin, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The full-frame source block ``source`` [B, C, cc, H, W] and the loop's final state on the region ``state`` [B, C, cc + G + cc, hr,
    wr], whose corner is ``origin`` = (y0, x0), as the full-frame state [B, C, cc + G + cc, H, W] in ONE launch
    (``wan_region_restore``): source frames are the source; grounding frame g and target frame f are the region's inside its box and
    source frames g and f outside it, so outside the box the target is the source bit for bit.  Elements of 1, 2 or 4 bytes."""
    if not source.is_cuda or not state.is_cuda:
        raise RuntimeError(f"region_restore: tensors are on {source.device} and {state.device}; the HIP path has no CPU fallback")
    if source.element_size() not in (1, 2, 4):
        raise ValueError(f"region_restore: dtype {source.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype \
            or source.device != state.device:
        raise ValueError(f"region_restore: source {source.dtype} {tuple(source.shape)} on {source.device} and state {state.dtype} "
                         f"{tuple(state.shape)} on {state.device}: expected [B, C, cc, H, W] and [B, C, cc + G + cc, hr, wr] of one dtype")
    source, state = source.contiguous(), state.contiguous()
    B, C, cc, H, W = (int(v) for v in source.shape)
    Ftot, hr, wr = (int(v) for v in state.shape[2:])
    if len(origin) != 2:
        raise ValueError(f"region_restore: origin = (y0, x0) in cells, got {origin!r}")
    out = _region_out(out, (B, C, Ftot, H, W), source, "region_restore.out")
    _lib.check(_lib.load().wan_region_restore(_p(out), _p(source), _p(state), source.element_size(), B, C, cc, Ftot - 2 * cc, H, W,
                                              int(origin[0]), int(origin[1]), hr, wr, _stream()), "wan_region_restore")
    return out


@_on_tensor_device
def region_crop_frames(x: torch.Tensor, runs, region, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sub-box ``region`` = (y0, x0, h, w) of the frames that ``runs`` lists of a contiguous ``x`` [..., F, H, W], as a contiguous
    [..., Fo, h, w] tensor in ONE launch (``wan_region_crop_frames``).  ``runs``: 1 to 3 pairs (start, count) of frames, ascending and not
    overlapping; Fo is the sum of the counts.  Elements of 1, 2 or 4 bytes, bits unchanged.  Serves the loop state (the runs of its
    source, grounding and target segments) and the mask's weights (one run)."""
    if not x.is_cuda:
        raise RuntimeError(f"region_crop_frames.x: tensor is on {x.device}; the HIP path has no CPU fallback")
    if x.element_size() not in (1, 2, 4):
        raise ValueError(f"region_crop_frames: dtype {x.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if x.dim() < 3 or not x.is_contiguous():
        raise ValueError(f"region_crop_frames.x: a contiguous [..., F, H, W] tensor, got {tuple(x.shape)}")
    y0, x0, hr, wr = _region_box(region, "region_crop_frames")
    runs = list(runs)
    if any(not hasattr(pair, "__len__") or len(pair) != 2 for pair in runs):
        raise ValueError(f"region_crop_frames: runs = pairs (start, count) of frames, got {runs!r}")
    flat = [int(v) for pair in runs for v in pair]
    F, H, W = (int(v) for v in x.shape[-3:])
    R = int(math.prod(x.shape[:-3]))
    Fo = sum(max(c, 0) for c in flat[1::2])
    out = _region_out(out, tuple(x.shape[:-3]) + (Fo, max(hr, 0), max(wr, 0)), x, "region_crop_frames.out")
    _lib.check(_lib.load().wan_region_crop_frames(_p(out), _p(x), x.element_size(), R, F, H, W, (ctypes.c_int * max(len(flat), 1))(*flat),
                                                  len(flat) // 2, y0, x0, hr, wr, _stream()), "wan_region_crop_frames")
    return out


@_on_tensor_device
def region_restore_frames(source: torch.Tensor, state: torch.Tensor, origin, frames, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The whole source block ``source`` [B, C, cc, H, W] and the loop's final state ``state`` [B, C, n + G + n, hr, wr] on the source
    frames ``frames`` = (t0, n) and the box whose corner is ``origin`` = (y0, x0), as the whole state [B, C, cc + G + cc, H, W] in ONE
    launch (``wan_region_restore_frames``): source frames are the source; grounding frame g is the region's inside the box and source
    frame g outside it; target frame f is the region's where t0 <= f < t0 + n and inside the box, and source frame f everywhere else,
    bit for bit.  Elements of 1, 2 or 4 bytes."""
    if not source.is_cuda or not state.is_cuda:
        raise RuntimeError(f"region_restore_frames: tensors are on {source.device} and {state.device}; the HIP path has no CPU fallback")
    if source.element_size() not in (1, 2, 4):
        raise ValueError(f"region_restore_frames: dtype {source.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype \
            or source.device != state.device:
        raise ValueError(f"region_restore_frames: source {source.dtype} {tuple(source.shape)} on {source.device} and state {state.dtype} "
                         f"{tuple(state.shape)} on {state.device}: expected [B, C, cc, H, W] and [B, C, n + G + n, hr, wr] of one dtype")
    source, state = source.contiguous(), state.contiguous()
    B, C, cc, H, W = (int(v) for v in source.shape)
    Fr, hr, wr = (int(v) for v in state.shape[2:])
    if len(origin) != 2:
        raise ValueError(f"region_restore_frames: origin = (y0, x0) in cells, got {origin!r}")
    if len(frames) != 2:
        raise ValueError(f"region_restore_frames: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    G = Fr - 2 * n
    out = _region_out(out, (B, C, max(2 * cc + G, 0), H, W), source, "region_restore_frames.out")
    _lib.check(_lib.load().wan_region_restore_frames(_p(out), _p(source), _p(state), source.element_size(), B, C, cc, G, H, W, t0, n,
                                                     int(origin[0]), int(origin[1]), hr, wr, _stream()), "wan_region_restore_frames")
    return out


def _track_origins(origins, name: str):
    """A table of corners as the C side takes it: (ctypes int array or None for an empty table, rows)."""
    import numpy as np
    o = np.asarray(origins.cpu() if torch.is_tensor(origins) else origins)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError(f"{name}: origins = integer [frames, 2] pairs (y0, x0) in cells, got {o.dtype} {o.shape}")
    if o.shape[0] == 0:
        return None, 0
    if int(o.min()) < -2 ** 31 or int(o.max()) >= 2 ** 31:
        raise ValueError(f"{name}: origins leave the int32 range")
    return (ctypes.c_int * o.size).from_buffer_copy(np.ascontiguousarray(o, dtype=np.int32)), int(o.shape[0])


@_on_tensor_device
def region_crop_track(x: torch.Tensor, runs, origins, size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``region_crop_frames`` with a box that moves: ``origins`` integer [F, 2] on the HOST = the corner (y0, x0) of every input frame's
    box, ``size`` = (h, w), one for all -> contiguous [..., Fo, h, w] in ONE launch (``wan_region_crop_track``: the table travels in
    the kernel's arguments, at most 512 frames; nothing is allocated, copied to the device or synchronised).  The loop state takes a
    table over its 2 cc + G frames (grounding g at source frame g's corner, target f at source frame f's), the weights the source
    frames' table."""
    if not x.is_cuda:
        raise RuntimeError(f"region_crop_track.x: tensor is on {x.device}; the HIP path has no CPU fallback")
    if x.element_size() not in (1, 2, 4):
        raise ValueError(f"region_crop_track: dtype {x.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if x.dim() < 3 or not x.is_contiguous():
        raise ValueError(f"region_crop_track.x: a contiguous [..., F, H, W] tensor, got {tuple(x.shape)}")
    if len(size) != 2:
        raise ValueError(f"region_crop_track: size = (h, w) in cells, got {size!r}")
    hr, wr = int(size[0]), int(size[1])
    runs = list(runs)
    if any(not hasattr(pair, "__len__") or len(pair) != 2 for pair in runs):
        raise ValueError(f"region_crop_track: runs = pairs (start, count) of frames, got {runs!r}")
    flat = [int(v) for pair in runs for v in pair]
    F, H, W = (int(v) for v in x.shape[-3:])
    table, rows = _track_origins(origins, "region_crop_track")
    if rows != F:
        raise ValueError(f"region_crop_track: {rows} rows of origins for {F} input frames (one each)")
    R = int(math.prod(x.shape[:-3]))
    Fo = sum(max(c, 0) for c in flat[1::2])
    out = _region_out(out, tuple(x.shape[:-3]) + (Fo, max(hr, 0), max(wr, 0)), x, "region_crop_track.out")
    _lib.check(_lib.load().wan_region_crop_track(_p(out), _p(x), x.element_size(), R, F, H, W, (ctypes.c_int * max(len(flat), 1))(*flat),
                                                 len(flat) // 2, table, hr, wr, _stream()), "wan_region_crop_track")
    return out


@_on_tensor_device
def region_restore_track(source: torch.Tensor, state: torch.Tensor, origins, frames, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``region_restore_frames`` with a box that moves: ``origins`` integer [cc, 2] on the HOST = the corner of source frame f's box
    (grounding g uses origins[g]).  Outside its frame's box, and outside the range ``frames`` = (t0, n), the target is the source bit
    for bit.  ONE launch (``wan_region_restore_track``); at most 512 source frames."""
    if not source.is_cuda or not state.is_cuda:
        raise RuntimeError(f"region_restore_track: tensors are on {source.device} and {state.device}; the HIP path has no CPU fallback")
    if source.element_size() not in (1, 2, 4):
        raise ValueError(f"region_restore_track: dtype {source.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype \
            or source.device != state.device:
        raise ValueError(f"region_restore_track: source {source.dtype} {tuple(source.shape)} on {source.device} and state {state.dtype} "
                         f"{tuple(state.shape)} on {state.device}: expected [B, C, cc, H, W] and [B, C, n + G + n, hr, wr] of one dtype")
    source, state = source.contiguous(), state.contiguous()
    B, C, cc, H, W = (int(v) for v in source.shape)
    Fr, hr, wr = (int(v) for v in state.shape[2:])
    if len(frames) != 2:
        raise ValueError(f"region_restore_track: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    G = Fr - 2 * n
    table, rows = _track_origins(origins, "region_restore_track")
    if rows != cc:
        raise ValueError(f"region_restore_track: {rows} rows of origins for {cc} source frames (one each)")
    out = _region_out(out, (B, C, max(2 * cc + G, 0), H, W), source, "region_restore_track.out")
    _lib.check(_lib.load().wan_region_restore_track(_p(out), _p(source), _p(state), source.element_size(), B, C, cc, G, H, W, t0, n,
                                                    table, hr, wr, _stream()), "wan_region_restore_track")
    return out


@_on_tensor_device
def mask_spans(weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Latent-cell weights uint8 [Bm, Fs, h, w] -> device int16 [Fs, h + w, 2]: per latent frame and row the inclusive (x_lo, x_hi) of
    the non-zero weights over all samples, (w, -1) for a row without one, then per column (y_lo, y_hi), (h, -1) for a column without
    one (``wan_mask_spans``: one workgroup per frame, no atomics, every word written once).  A frame's bounds (``mask_bounds``) are the
    min and max of its spans.  Never synchronises: the caller copies the 4 * (h + w) * Fs bytes to the host."""
    _need(weights, torch.uint8, "mask_spans.weights")
    if weights.dim() != 4 or not weights.is_contiguous():
        raise ValueError(f"mask_spans.weights: a contiguous uint8 [Bm, Fs, h, w] tensor, got {tuple(weights.shape)}")
    Bm, Fs, h, w = (int(v) for v in weights.shape)
    if out is None:
        out = torch.empty((Fs, h + w, 2), device=weights.device, dtype=torch.int16)
    elif tuple(out.shape) != (Fs, h + w, 2) or out.dtype != torch.int16 or not out.is_contiguous() or out.device != weights.device:
        raise ValueError(f"mask_spans.out: {out.dtype} {tuple(out.shape)} on {out.device} for contiguous int16 {(Fs, h + w, 2)} on "
                         f"{weights.device}")
    _lib.check(_lib.load().wan_mask_spans(_p(weights), _p(out), Bm, Fs, h, w, _stream()), "wan_mask_spans")
    return out


def _split_boxes(origins, cuts, name: str):
    """The boxes of a split as the C side takes them: (origins, cuts as ctypes int arrays or None, K)."""
    import numpy as np
    o = np.asarray(origins.cpu() if torch.is_tensor(origins) else origins)
    c = np.asarray(cuts.cpu() if torch.is_tensor(cuts) else cuts)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError(f"{name}: origins = integer [K, 2] pairs (y0, x0) in cells, got {o.dtype} {o.shape}")
    if c.ndim != 1 or c.dtype.kind not in "iu" or c.shape[0] != o.shape[0] + 1:
        raise ValueError(f"{name}: cuts = {o.shape[0] + 1} integers for {o.shape[0]} boxes, got {c.dtype} {c.shape}")
    if o.shape[0] == 0:
        return None, None, 0
    if min(int(o.min()), int(c.min())) < -2 ** 31 or max(int(o.max()), int(c.max())) >= 2 ** 31:
        raise ValueError(f"{name}: origins or cuts leave the int32 range")
    as_c = lambda a: (ctypes.c_int * a.size).from_buffer_copy(np.ascontiguousarray(a, dtype=np.int32))
    return as_c(o), as_c(c), int(o.shape[0])


@_on_tensor_device
def region_crop_split(x: torch.Tensor, runs, origins, cuts, axis: int, size, clip: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``region_crop_frames`` for the K boxes of a split at once: ``origins`` integer [K, 2] and ``cuts`` integer [K + 1] on the HOST,
    ``axis`` 1 (the cuts are columns) or 0 (rows) as in ``edit_region.SplitPlan``, ``size`` = (h, w), one for all -> contiguous
    [K, ..., Fo, h, w], box-major, in ONE launch (``wan_region_crop_split``: the table travels in the kernel's arguments, at most 8
    boxes).  ``clip``: everything outside what band k owns is zero in box k -- the form for the mask's weights."""
    if not x.is_cuda:
        raise RuntimeError(f"region_crop_split.x: tensor is on {x.device}; the HIP path has no CPU fallback")
    if x.element_size() not in (1, 2, 4):
        raise ValueError(f"region_crop_split: dtype {x.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if x.dim() < 3 or not x.is_contiguous():
        raise ValueError(f"region_crop_split.x: a contiguous [..., F, H, W] tensor, got {tuple(x.shape)}")
    if len(size) != 2:
        raise ValueError(f"region_crop_split: size = (h, w) in cells, got {size!r}")
    hr, wr = int(size[0]), int(size[1])
    runs = list(runs)
    if any(not hasattr(pair, "__len__") or len(pair) != 2 for pair in runs):
        raise ValueError(f"region_crop_split: runs = pairs (start, count) of frames, got {runs!r}")
    flat = [int(v) for pair in runs for v in pair]
    F, H, W = (int(v) for v in x.shape[-3:])
    table, bounds, K = _split_boxes(origins, cuts, "region_crop_split")
    R = int(math.prod(x.shape[:-3]))
    Fo = sum(max(c, 0) for c in flat[1::2])
    out = _region_out(out, (K,) + tuple(x.shape[:-3]) + (Fo, max(hr, 0), max(wr, 0)), x, "region_crop_split.out")
    _lib.check(_lib.load().wan_region_crop_split(_p(out), _p(x), x.element_size(), R, F, H, W, (ctypes.c_int * max(len(flat), 1))(*flat),
                                                 len(flat) // 2, table, bounds, K, int(axis), int(bool(clip)), hr, wr, _stream()),
               "wan_region_crop_split")
    return out


@_on_tensor_device
def region_restore_split(source: torch.Tensor, state: torch.Tensor, origins, cuts, axis: int, frames,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``region_restore_frames`` for the K boxes of a split: ``source`` [B, C, cc, H, W] and ``state`` [K B, C, n + G + n, hr, wr],
    box-major -> [B, C, cc + G + cc, H, W] in ONE launch (``wan_region_restore_split``).  A grounding or target cell takes box k's
    value where it lies inside box k AND inside what band k owns (the target only in the frames ``frames`` = (t0, n)); everywhere
    else it is the source, bit for bit."""
    if not source.is_cuda or not state.is_cuda:
        raise RuntimeError(f"region_restore_split: tensors are on {source.device} and {state.device}; the HIP path has no CPU fallback")
    if source.element_size() not in (1, 2, 4):
        raise ValueError(f"region_restore_split: dtype {source.dtype} not supported (elements of 1, 2 or 4 bytes)")
    if source.dim() != 5 or state.dim() != 5 or source.shape[1] != state.shape[1] or source.dtype != state.dtype \
            or source.device != state.device:
        raise ValueError(f"region_restore_split: source {source.dtype} {tuple(source.shape)} on {source.device} and state {state.dtype} "
                         f"{tuple(state.shape)} on {state.device}: expected [B, C, cc, H, W] and [K B, C, n + G + n, hr, wr] of one dtype")
    source, state = source.contiguous(), state.contiguous()
    B, C, cc, H, W = (int(v) for v in source.shape)
    Fr, hr, wr = (int(v) for v in state.shape[2:])
    if len(frames) != 2:
        raise ValueError(f"region_restore_split: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    G = Fr - 2 * n
    table, bounds, K = _split_boxes(origins, cuts, "region_restore_split")
    if int(state.shape[0]) != K * B:
        raise ValueError(f"region_restore_split: {int(state.shape[0])} state samples for {K} boxes of {B} samples (box-major)")
    out = _region_out(out, (B, C, max(2 * cc + G, 0), H, W), source, "region_restore_split.out")
    _lib.check(_lib.load().wan_region_restore_split(_p(out), _p(source), _p(state), source.element_size(), B, C, cc, G, H, W, t0, n,
                                                    table, bounds, K, int(axis), hr, wr, _stream()), "wan_region_restore_split")
    return out


def _avail(t: torch.Tensor) -> int:
    """Elements from t's first element to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


@_on_tensor_device
def gemm_batched(a: torch.Tensor, stride_a: int, w: torch.Tensor, stride_w: int, out: torch.Tensor, stride_o: int,
                 M: int, N: int, K: int, batch: int, epilogue: int) -> torch.Tensor:
    """`batch` independent products out_z[m,n] = sum_k a_z[m,k] * w_z[n,k] (one per attention head).
    a / w / out are 2-D views (unit inner stride) of problem 0; problem z starts `stride_*` elements later
    in the same storage.  EPI_BF16 or EPI_F32."""
    _need(a, torch.bfloat16, "gemm_batched.a")
    _need(w, torch.bfloat16, "gemm_batched.w")
    _need(out, torch.float32 if epilogue == EPI_F32 else torch.bfloat16, "gemm_batched.out")
    for nm, t in (("a", a), ("w", w), ("out", out)):
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"gemm_batched.{nm} must be a 2-D view with unit inner stride")
    lda, ldw, ldo = a.stride(0), w.stride(0), out.stride(0)
    if min(batch, M, N, K) < 1 or min(stride_a, stride_w, stride_o) < 0:
        raise ValueError("gemm_batched: empty problem or negative stride")
    if (_avail(a) < (batch - 1) * stride_a + (M - 1) * lda + K or _avail(w) < (batch - 1) * stride_w + (N - 1) * ldw + K
            or _avail(out) < (batch - 1) * stride_o + (M - 1) * ldo + N):
        raise ValueError("gemm_batched: the strided problem runs past the end of an operand's storage")
    lib = _lib.load()
    _lib.check(lib.wan_gemm_bf16_batched(_p(a), lda, stride_a, _p(w), ldw, stride_w, _p(out), ldo, stride_o,
                                         M, N, K, batch, epilogue, _stream()), "wan_gemm_bf16_batched")
    return out


@_on_tensor_device
def embedding_rows(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """ids int64 [n] -> fp32 [n, dim] rows of the bf16 table [vocab, dim]."""
    _need(ids, torch.int64, "embedding.ids")
    _need(table, torch.bfloat16, "embedding.table")
    if ids.dim() != 1 or table.dim() != 2 or not (ids.is_contiguous() and table.is_contiguous()):
        raise ValueError("embedding: ids must be contiguous [n] and table contiguous [vocab, dim]")
    out = torch.empty(ids.numel(), table.shape[1], device=ids.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.wan_embedding_rows(_p(ids), _p(table), table.shape[0], _p(out), ids.numel(), table.shape[1],
                                      _stream()), "wan_embedding_rows")
    return out


@_on_tensor_device
def rmsnorm_rows(x: torch.Tensor, w: torch.Tensor, eps: float, out_dtype: torch.dtype = torch.bfloat16,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T5LayerNorm of fp32 rows [rows, dim] -> bf16 (GEMM input) or fp32."""
    _need(x, torch.float32, "rmsnorm_rows.x")
    _need(w, torch.float32, "rmsnorm_rows.w")
    if x.dim() != 2 or not x.is_contiguous() or w.numel() != x.shape[1]:
        raise ValueError("rmsnorm_rows: x must be contiguous [rows, dim] and w [dim]")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("rmsnorm_rows: out_dtype must be float32 or bfloat16")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    _need(out, out_dtype, "rmsnorm_rows.out")
    if out.shape != x.shape or not out.is_contiguous():
        raise ValueError(f"rmsnorm_rows.out must be contiguous and of x's shape {tuple(x.shape)}, got {tuple(out.shape)} with strides {out.stride()}")
    lib = _lib.load()
    _lib.check(lib.wan_rmsnorm_rows(_p(x), _p(w), _p(out), 0 if out_dtype == torch.float32 else 1, x.shape[0],
                                    x.shape[1], float(eps), _stream()), "wan_rmsnorm_rows")
    return out


@_on_tensor_device
def t5_softmax_bias(scores: torch.Tensor, table: torch.Tensor, lut: torch.Tensor, num_heads: int, k_len: int,
                    npad: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scores fp32 [H, L, L] -> probs bf16 [H, L, npad] = softmax_j(scores + rel-pos bias), keys >= k_len masked."""
    _need(scores, torch.float32, "t5_softmax.scores")
    _need(table, torch.float32, "t5_softmax.table")
    _need(lut, torch.int32, "t5_softmax.lut")
    H, Lq, Lk = scores.shape
    if H != num_heads or not scores.is_contiguous() or table.shape != (table.shape[0], H) or not table.is_contiguous():
        raise ValueError("t5_softmax: scores must be contiguous [H, Lq, Lk], table contiguous [num_buckets, H]")
    if lut.numel() != Lq + Lk - 1:
        raise ValueError("t5_softmax: lut must have Lq + Lk - 1 entries")
    if out is None:
        out = torch.empty(H, Lq, npad, device=scores.device, dtype=torch.bfloat16)
    _need(out, torch.bfloat16, "t5_softmax.out")
    # the kernel addresses row (h, i) at (h * Lq + i) * ldp: heads must follow each other without a gap
    if out.dim() != 3 or out.shape[0] != H or out.shape[1] != Lq or out.shape[2] < npad:
        raise ValueError(f"t5_softmax.out must be [H, Lq, >= npad] = [{H}, {Lq}, >= {int(npad)}], got {tuple(out.shape)}")
    if out.stride(2) != 1 or out.stride(1) < npad or out.stride(0) != Lq * out.stride(1):
        raise ValueError(f"t5_softmax.out: strides {out.stride()} must be (Lq * ldp, ldp, 1) with ldp >= npad")
    lib = _lib.load()
    _lib.check(lib.wan_t5_softmax_bias(_p(scores), Lk, _p(table), _p(lut), _p(out), out.stride(1), H, Lq, Lk,
                                       int(k_len), int(npad), _stream()), "wan_t5_softmax_bias")
    return out


@_on_tensor_device
def mul_bf16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _need(a, torch.bfloat16, "mul.a")
    _need(b, torch.bfloat16, "mul.b")
    if a.shape != b.shape or not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("mul_bf16: operands must be contiguous and of equal shape")
    if out is None:
        out = torch.empty_like(a)
    _need(out, torch.bfloat16, "mul.out")
    if out.shape != a.shape or not out.is_contiguous():
        raise ValueError(f"mul_bf16.out must be contiguous and of the operands' shape {tuple(a.shape)}, got {tuple(out.shape)} with strides {out.stride()}")
    lib = _lib.load()
    _lib.check(lib.wan_mul_bf16(_p(a), _p(b), _p(out), a.numel(), _stream()), "wan_mul_bf16")
    return out
