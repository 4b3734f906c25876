"""Tensor-level bindings: the operator boundary of the QSpec path.

Each function mirrors the call signature of the reference extension op it
replaces (names in the docstrings, paths relative to the reference checkout),
takes caller-owned contiguous HIP tensors, enqueues on the current torch stream
and never synchronises.  PyTorch is used for memory and streams only.
"""
from __future__ import annotations

import contextlib
import os
import threading
from typing import Optional

import torch

from . import _lib

_F16, _I8, _U8, _I64, _I32, _F32 = torch.float16, torch.int8, torch.uint8, torch.int64, torch.int32, torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _device_index(device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _stream_id(device) -> int:
    """The current stream of `device`: the ONE place the workspace registry learns which stream it is on."""
    return torch.cuda.current_stream(device).cuda_stream


# kind -> (library function giving the size in bytes, sized by rows, zero-filled (else merely allocated), dtype)
_WS_KINDS = {
    "xwg":     ("qspec_xwg_workspace_bytes", False, True, _I32),              # spread-Hadamard exchange
    "ln":      ("qspec_ln_linear_workspace_bytes", False, True, _U8),         # norm hand-off of the LN-prologue GEMMs
    "w4a16":   ("qspec_w4a16_workspace_bytes", False, True, _U8),             # split-K scratch of the W4A16 kernels
    "sampler": ("qspec_sampler_workspace_bytes", True, False, _U8),           # chunked softmax / rejection partials
    "lm_head": ("qspec_lm_head_sampler_workspace_bytes", True, False, _U8),   # row maxima of lm_head_softmax_argmax
    "sample":  ("qspec_sample_workspace_bytes", True, True, _U8),             # histogram of sample_top_k_top_p
}
# int32 index of the sticky error word of the kinds that carry one; mirrors QS_XWG_ERR_WORD (csrc/hadamard.hip) and
# the hand-off kernel's `sync[31]` (csrc/gemm_stream_w4a4.hip; "int32 word 31" in include/qspec_hip.h)
_ERROR_WORD = {"xwg": 0, "ln": 31}
_workspaces = {}    # (kind, device.type, device.index, stream[, rows]) -> tensor
_tls = threading.local()    # .no_handoffs: how many no_handoffs() blocks this thread is inside


def _workspace(kind: str, device, *, rows=None):
    """The process-wide scratch / hand-off workspace of `kind`.  Workspaces carry ticket, flag or generation state and are
    safe for ONE stream at a time (launches on a stream are serialised), so each (device, stream[, rows]) gets its own.
    Created lazily at the first use of its key -- also when that use falls inside a graph capture, where the zero fill
    becomes a memset node of the graph.  Creating them ahead of capture (on sample_workspace) changes
    the captured cycle and is left to a change of its own; this is the one place it has to be made."""
    size_fn, by_rows, zeroed, dtype = _WS_KINDS[kind]
    assert (rows is not None) == by_rows, kind
    device = torch.device(device)
    rows = (rows,) if by_rows else ()
    key = (kind, device.type, _device_index(device), _stream_id(device)) + rows
    ws = _workspaces.get(key)
    if ws is None:
        nbytes = int(getattr(_lib.load(), size_fn)(*rows))
        ws = _workspaces[key] = (torch.zeros if zeroed else torch.empty)(nbytes // dtype.itemsize, dtype=dtype, device=device)
    return ws


def error_words(device, current_stream_only: bool = False, kind=None):
    """One-element int32 views of the sticky error words of the device's hand-off workspaces: those of EVERY stream (a
    captured graph keeps the workspaces of its capture stream), or of the current stream only; `kind`: of that kind only."""
    device = torch.device(device)
    want = (device.type, _device_index(device)) + ((_stream_id(device),) if current_stream_only else ())
    # (list(): a snapshot -- ranks run as threads of one process create workspaces of their own devices meanwhile)
    return [ws.view(_I32).narrow(0, _ERROR_WORD[key[0]], 1) for key, ws in list(_workspaces.items())
            if key[0] in _ERROR_WORD and kind in (None, key[0]) and key[1:1 + len(want)] == want]


def clear_error_words(device) -> None:
    for w in error_words(device):
        w.zero_()


@contextlib.contextmanager
def no_handoffs():
    """On the calling thread only: xwg_workspace() and ln_linear_workspace() return None, so the kernels that wait for
    partner workgroups take their one-workgroup / recompute forms (bit-identical).  XWG_SPREAD / LN_HANDOFF, the process
    defaults, are not touched: other engines of the process (ranks run as threads) keep their launch forms.  Nests."""
    depth = getattr(_tls, "no_handoffs", 0)
    _tls.no_handoffs = depth + 1
    try:
        yield
    finally:
        _tls.no_handoffs = depth


def _chk(t: torch.Tensor, name: str, dtype=None):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP/CUDA tensor (the QSpec hot path has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None:
        ok = t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype
        if not ok:
            raise RuntimeError(f"{name} has dtype {t.dtype}, expected {dtype}")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype=None):
    return None if t is None else _chk(t, name, dtype)


_KV8 = (torch.uint8, torch.float8_e4m3fn)


def _kv(key_cache, value_cache, k_scale: float = 1.0, v_scale: float = 1.0):
    """Cache arguments of an entry that takes (key_cache, value_cache): the name suffix and the argument tuple.
    fp16 caches -> the base entry; uint8 / float8_e4m3fn caches (kv_cache_dtype = "fp8") -> its `_kv8` form, which takes the
    per-tensor scales behind the two pointers.  A scale other than 1 with an fp16 cache is an error, not ignored."""
    if key_cache.dtype != value_cache.dtype:
        raise RuntimeError(f"key_cache is {key_cache.dtype}, value_cache {value_cache.dtype}")
    if key_cache.dtype in _KV8:
        k_scale, v_scale = float(k_scale), float(v_scale)
        if not (0.0 < k_scale < float("inf") and 0.0 < v_scale < float("inf")):
            raise ValueError(f"k_scale={k_scale}, v_scale={v_scale} must be positive and finite")
        return "_kv8", (_chk(key_cache, "key_cache", _KV8), _chk(value_cache, "value_cache", _KV8), k_scale, v_scale)
    if float(k_scale) != 1.0 or float(v_scale) != 1.0:
        raise ValueError("k_scale / v_scale belong to an fp8 KV cache; the cache tensors are fp16")
    return "", (_chk(key_cache, "key_cache", _F16), _chk(value_cache, "value_cache", _F16))


def _call(name: str, *args):
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args), lib)


# ------------------------------------------------------------------ norm + quant

def rms_norm_general_fuse_sum_i4(out_q, x, input_sum, scaling, eps: float, use_per_token_quant: bool = True):
    """qserve_backend.layernorm_ops.rms_norm_general_fuse_sum_i4 (third-party/kernels/csrc/layernorm.cpp:80-83)."""
    if not use_per_token_quant:
        raise RuntimeError("only per-token quantisation exists in the reference launcher (layernorm_kernels.cu:903)")
    H = x.shape[-1]
    T = x.numel() // H
    _call("qspec_rms_norm_general_fuse_sum_i4", _chk(out_q, "out_q", _I8), _chk(x, "x", _F16),
          _opt(input_sum, "input_sum", _F16), _chk(scaling, "scaling", _F16), float(eps), T, H, _stream())


def rms_norm_general_fuse_sum_fp16(out, x, eps: float):
    """layernorm_ops.rms_norm_general_fuse_sum_fp16 (layernorm.cpp:85-87)."""
    H = x.shape[-1]
    T = x.numel() // H
    _call("qspec_rms_norm_general_fuse_sum_fp16", _chk(out, "out", _F16), _chk(x, "x", _F16), float(eps), T, H,
          _stream())


def add_rms_norm_i4(out_q, scaling, hidden_out, x, delta, eps: float):
    """hidden_out = x + delta (fp16), then the i4 norm of hidden_out (quarot_llama.py:380-388 fused)."""
    H = x.shape[-1]
    T = x.numel() // H
    _call("qspec_add_rms_norm_i4", _chk(out_q, "out_q", _I8), _chk(scaling, "scaling", _F16),
          _opt(hidden_out, "hidden_out", _F16), _chk(x, "x", _F16), _opt(delta, "delta", _F16), float(eps), T, H,
          _stream())


def _xp_tile(t, name, K, tokens: int = 16):
    """A fragment-major activation tile always holds 16 rows (w4a16_act_layout_supported); 17..32 tokens: two tiles."""
    rows = 16 if tokens <= 16 else 32
    if t.numel() < rows * K:
        raise RuntimeError(f"{name}: {rows // 16} fragment-major tile(s) of 16 x {K} halves, got {tuple(t.shape)}")
    return t


def w4a16_act_layout_supported(M: int, K: int) -> bool:
    """True when the W4A16 GEMMs at (M <= 16 tokens, K) read the FRAGMENT-MAJOR activation tile the `xp=True` producers
    write (norm, head transform, MLP transform): [K/128][4][4 k-groups][16 rows][8 halves], the order the MFMA operand
    registers hold them, so the GEMM loads them straight from global memory with no LDS staging pass."""
    return bool(_lib.load().qspec_w4a16_act_layout_supported(M, K))


def w4a16_act_layout32_supported(M: int, N: int, K: int) -> bool:
    """17..32 tokens: the two-token-tile W4A16 streaming kernel takes (M, N, K); x is then two fragment-major tiles [2, 16, K]."""
    return bool(_lib.load().qspec_w4a16_act_layout32_supported(M, N, K))


def _xp32_tiles(t, name, K):
    if t.numel() < 32 * K:
        raise RuntimeError(f"{name}: two fragment-major tiles are 2 x 16 x {K} halves, got {tuple(t.shape)}")
    return _chk(t, name, _F16)


def w4a16_linear_xp32(x, wq, w_scale, out, tokens: int):
    N, K = wq.shape[0], wq.shape[1] * 2
    _call("qspec_w4a16_linear_xp32", _xp32_tiles(x, "x", K), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _chk(out, "out", _F16), tokens, N, K, _stream())
    return out


def w4a16_linear_partial_slices_xp32(M: int, N: int, K: int) -> int:
    return int(_lib.load().qspec_w4a16_linear_partial_slices_xp32(M, N, K))


def w4a16_linear_partial_xp32(x, wq, part, slices: int, tokens: int):
    N, K = wq.shape[0], wq.shape[1] * 2
    _call("qspec_w4a16_linear_partial_xp32", _xp32_tiles(x, "x", K), _chk(wq, "wq", (_I8, _U8)), _chk(part, "part", _F32), tokens, N, K,
          slices, _stream())
    return part


def qkv_rope_linear_xp32(x, wq, w_scale, qkv, positions, cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads,
                         num_kv_heads, head_size, tokens: int, k_scale: float = 1.0, v_scale: float = 1.0):
    N, K = wq.shape[0], wq.shape[1] * 2
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    _call("qspec_qkv_rope_linear_w4a16_xp32" + kv8, _xp32_tiles(x, "x", K), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _chk(qkv, "qkv", _F16), tokens, N, K, _chk(positions, "positions", _I64), _chk(cos_sin_cache, "cos_sin_cache", _F16),
          *caches, _chk(slot_mapping, "slot_mapping", _I64),
          num_heads, num_kv_heads, head_size, cos_sin_cache.shape[-1], _stream())
    return qkv


def gate_up_silu_linear_xp32(x, wq, w_scale, act, tokens: int):
    I, K = wq.shape[0] // 2, wq.shape[1] * 2
    _call("qspec_gate_up_silu_linear_w4a16_xp32", _xp32_tiles(x, "x", K), _chk(wq, "wq", (_I8, _U8)),
          _chk(w_scale, "w_scale", _F16), _chk(act, "act", _F16), tokens, I, K, _stream())
    return act


def mlp_hadamard_act_layout_supported(T: int, I: int, K: int) -> bool:
    """mlp_hadamard(..., xp=True) exists at this shape (the spread forms and the one-workgroup form both store the tiles, so the
    answer does not depend on XWG_SPREAD: a recovery replay without hand-off kernels takes the same GEMM forms)."""
    return bool(_lib.load().qspec_mlp_hadamard_act_layout_supported(T, I, K))


def add_rms_norm_fp16(out, hidden_out, x, delta, eps: float, xp: bool = False):
    H = x.shape[-1]
    T = x.numel() // H
    if xp:
        _xp_tile(out, "out", H, T)
    _call("qspec_add_rms_norm_fp16" + ("_xp" if xp else ""), _chk(out, "out", _F16), _opt(hidden_out, "hidden_out", _F16),
          _chk(x, "x", _F16), _opt(delta, "delta", _F16), float(eps), T, H, _stream())


def fuse_sym_quant(x, scale, q, clip_ratio: float = 1.0):
    """quarot._CUDA.fuse_sym_quant(x, scale, q, clip) (third-party/QuaRot/quarot/kernels/bindings.cpp:128-147)."""
    T, K = x.shape
    _call("qspec_fuse_sym_quant", _chk(x, "x", _F16), _chk(scale, "scale", _F16), _chk(q, "q", _I8),
          float(clip_ratio), T, K, _stream())


# ------------------------------------------------------------------ hadamard

def faster_fast_hadamard_transform(x, scale: float, out):
    """fast_hadamard_transform_cuda.faster_fast_hadamard_transform(x, scale, out)
    (third-party/fast-hadamard-transform/csrc/fast_hadamard_transform.cpp:69-110)."""
    n = x.shape[-1]
    rows = x.numel() // n
    _call("qspec_fast_hadamard_transform", _chk(x, "x", _F16), float(scale), _chk(out, "out", _F16), rows, n,
          _stream())
    return out


def fast_hadamard_transform(x, scale: float = 1.0):
    """fast_hadamard_transform_cuda.fast_hadamard_transform(x, scale) -> new tensor (:113-154)."""
    return faster_fast_hadamard_transform(x, scale, torch.empty_like(x))


def hadamard_mix(y, hadK, out):
    """`hadK @ y.view(-1, K, m)` (quarot/functional/hadamard.py:104-108)."""
    T, K, m = y.shape
    _call("qspec_hadamard_mix", _chk(y, "y", _F16), _chk(hadK, "hadK", _F16), _chk(out, "out", _F16), T, K, m,
          _stream())
    return out


def heads_hadamard(attn, had_scale: float, out_f16=None, q=None, scale=None, clip_ratio: float = 1.0, heads=None):
    """quarot_llama.py:231-238 in one kernel; attn [T, heads, d] (or [T, heads*d] with heads given)."""
    if attn.dim() == 3:
        T, heads, d = attn.shape
    else:
        T = attn.shape[0]
        d = attn.shape[1] // heads
    _call("qspec_heads_hadamard", _chk(attn, "attn", _F16), _opt(out_f16, "out_f16", _F16), _opt(q, "q", _I8),
          _opt(scale, "scale", _F16), float(had_scale), float(clip_ratio), T, heads, d, _stream())


def heads_hadamard_mix(attn, hadK, K: int, had_scale: float, out):
    """Head transform for head counts K * 2^p with a table factor (matmul_hadU_cuda between the transposes of
    quarot_llama.py:231-234); attn [T, heads, d], out the same number of elements, fp16."""
    if attn.dim() != 3:
        raise RuntimeError("heads_hadamard_mix: attn must be [T, heads, d]")
    T, heads, d = attn.shape
    _call("qspec_heads_hadamard_mix", _chk(attn, "attn", _F16), _chk(hadK, "hadK", _F16), _chk(out, "out", _F16),
          float(had_scale), T, heads, d, K, _stream())
    return out


def silu_mul(gate_up, out):
    """`act_fn(gate) * up` over the fused gate_up row (quarot_llama.py:279-284)."""
    T, two_i = gate_up.shape
    _call("qspec_silu_mul", _chk(gate_up, "gate_up", _F16), _chk(out, "out", _F16), T, two_i // 2, _stream())
    return out


def silu_mul_hadamard(gate_up, hadK, K: int, had_scale: float, out_f16=None, q=None, scale=None,
                      clip_ratio: float = 1.0):
    """quarot_llama.py:279-295 in one kernel; gate_up [T, 2I] with up first."""
    T, two_i = gate_up.shape
    _call("qspec_silu_mul_hadamard", _chk(gate_up, "gate_up", _F16), _opt(hadK, "hadK", _F16),
          _opt(out_f16, "out_f16", _F16), _opt(q, "q", _I8), _opt(scale, "scale", _F16), float(had_scale),
          float(clip_ratio), T, two_i // 2, K, _stream())


XWG_SPREAD = os.environ.get("QSPEC_XWG_SPREAD", "1") != "0"   # False: one workgroup per token (no workspace)


def xwg_workspace(device):
    """Exchange workspace of the kernels that spread one token over several workgroups (mlp_hadamard,
    heads_hadamard_merged): zero-filled once, never reset.  None: the one-workgroup forms.  Sticky error flag: _ERROR_WORD."""
    if not XWG_SPREAD or getattr(_tls, "no_handoffs", 0):
        return None
    return _workspace("xwg", device)


def xwg_error_word(device):
    """Sticky error flags of EVERY exchange workspace of the device: int32 [n] (one word per workspace), or None if none."""
    words = error_words(device, kind="xwg")
    return torch.cat(words) if words else None


def mlp_hadamard(act, hadK, K: int, had_scale: float, out_f16=None, q=None, scale=None, clip_ratio: float = 1.0,
                 workspace="auto", xp: bool = False):
    """Hadamard (+ quantiser) tail of silu_mul_hadamard on act = silu(gate)*up, [T, I]."""
    T, I = act.shape
    ws = xwg_workspace(act.device) if isinstance(workspace, str) else workspace
    if xp:
        _xp_tile(out_f16, "out_f16", I, T)
    _call("qspec_mlp_hadamard" + ("_xp" if xp else ""), _chk(act, "act", _F16), _opt(hadK, "hadK", _F16), _opt(out_f16, "out_f16", _F16),
          _opt(q, "q", _I8), _opt(scale, "scale", _F16), float(had_scale), float(clip_ratio), T, I, K,
          None if ws is None else ws.data_ptr(), _stream())


# ------------------------------------------------------------------ linear

def qkv_rope_linear_supported(w4a4: bool, M: int, N: int, K: int, head_size: int) -> bool:
    """The fused qkv GEMM + RoPE + KV write exists for head size 128 (every shape) and 64 (streaming shapes)."""
    return bool(_lib.load().qspec_qkv_rope_linear_supported(int(bool(w4a4)), M, N, K, head_size))


def qkv_rope_linear(x, x_scale, wq, w_scale, qkv, positions, cos_sin_cache, key_cache, value_cache, slot_mapping,
                    num_heads, num_kv_heads, head_size, xp: bool = False, tokens=None, k_scale: float = 1.0,
                    v_scale: float = 1.0):
    """qkv GEMM + rotary_embedding + reshape_and_cache_flash in one launch (quarot_llama.py:183-226).
    x_scale is None -> W4A16 (x fp16 [M,K]); else W4A4 (x packed int4 [M,K/2])."""
    N = wq.shape[0]
    K = wq.shape[1] * 2
    M = x.shape[0] if tokens is None else tokens    # xp: x is the 16-row tile, tokens the rows in use
    if xp:
        _xp_tile(x, "x", K)
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    common = (_chk(positions, "positions", _I64), _chk(cos_sin_cache, "cos_sin_cache", _F16), *caches,
              _chk(slot_mapping, "slot_mapping", _I64), num_heads, num_kv_heads, head_size, cos_sin_cache.shape[-1])
    if x_scale is not None:
        _call("qspec_qkv_rope_linear_s4s4" + kv8, _chk(x, "xq", (_I8, _U8)), _chk(x_scale, "x_scale", _F16),
              _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16), _chk(qkv, "qkv", _F16), M, N, K, *common,
              _stream())
    else:
        _call("qspec_qkv_rope_linear_w4a16" + ("_xp" if xp else "") + kv8, _chk(x, "x", _F16), _chk(wq, "wq", (_I8, _U8)),
              _chk(w_scale, "w_scale", _F16), _chk(qkv, "qkv", _F16), M, N, K, *common,
              w4a16_workspace(x.device).data_ptr(), _stream())
    return qkv


def gate_up_silu_linear(x, x_scale, wq, w_scale, act, xp: bool = False, tokens=None):
    """gate_up GEMM + silu(gate)*up in one launch (quarot_llama.py:276-284); act [M, I]."""
    M = x.shape[0] if tokens is None else tokens
    I = wq.shape[0] // 2
    K = wq.shape[1] * 2
    if xp:
        _xp_tile(x, "x", K)
    if x_scale is not None:
        _call("qspec_gate_up_silu_linear_s4s4", _chk(x, "xq", (_I8, _U8)), _chk(x_scale, "x_scale", _F16),
              _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16), _chk(act, "act", _F16), M, I, K, _stream())
    else:
        _call("qspec_gate_up_silu_linear_w4a16" + ("_xp" if xp else ""), _chk(x, "x", _F16), _chk(wq, "wq", (_I8, _U8)),
              _chk(w_scale, "w_scale", _F16), _chk(act, "act", _F16), M, I, K, w4a16_workspace(x.device).data_ptr(),
              _stream())
    return act


def prefetch(t, workgroups: int = 128):
    """Cache hint (qspec_prefetch): pull tensor `t` into the Infinity Cache on the current stream.  EXPERIMENTAL build only
    (QSPEC_HIP_LIB=.../libqspec_hip_experimental.so): measured and left out of the engine."""
    _call("qspec_prefetch", t.data_ptr(), t.numel() * t.element_size(), workgroups, _stream())


def prefetch_tiles(wq, first_tile: int = 0, ntiles: Optional[int] = None, workgroups: int = 256):
    """Cache hint, tile aligned: workgroup b touches weight tiles b, b + workgroups, ... (16 rows each) of wq [N, K/2]."""
    tile_bytes = 16 * wq.shape[1] * wq.element_size()
    n = wq.shape[0] // 16 if ntiles is None else ntiles
    _call("qspec_prefetch_tiles", wq.data_ptr(), tile_bytes, first_tile, n, workgroups, _stream())


def ln_linear_s4s4_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().qspec_ln_linear_s4s4_supported(M, N, K))


LN_HANDOFF_MIN_M = int(os.environ.get("QSPEC_LN_HANDOFF_MIN_M", "8"))
LN_HANDOFF = os.environ.get("QSPEC_LN_HANDOFF", "1") != "0"   # False: every workgroup recomputes the norm (no workspace)


def ln_linear_workspace(device, M: int = 16):
    """Hand-off workspace of the LN-prologue GEMMs (zero-filled once; every call leaves it zeroed).  Measured on
    MI355X: up to 4 tokens every workgroup recomputing the norm is faster (10.4 vs 12.2 us for qkv_proj), from 8
    tokens the producer / hand-off form wins (15 vs 25 us at 16 tokens)."""
    if not LN_HANDOFF or M < LN_HANDOFF_MIN_M or getattr(_tls, "no_handoffs", 0):
        return None
    return _workspace("ln", device)


def ln_qkv_rope_linear(hidden_in, delta, hidden_out, eps, wq, w_scale, qkv, positions, cos_sin_cache, key_cache,
                       value_cache, slot_mapping, num_heads, num_kv_heads, head_size, k_scale: float = 1.0,
                       v_scale: float = 1.0):
    """Draft pass: hidden_out = hidden_in + delta; LN + int4 quant; qkv GEMM; RoPE; KV write -- one launch
    (quarot_llama.py:373-374 + 183-226)."""
    M, K = hidden_in.shape
    N = wq.shape[0]
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    _call("qspec_ln_qkv_rope_linear_s4s4" + kv8, _chk(hidden_in, "hidden_in", _F16), _opt(delta, "delta", _F16),
          _opt(hidden_out, "hidden_out", _F16), float(eps), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _chk(qkv, "qkv", _F16), M, N, K, _chk(positions, "positions", _I64), _chk(cos_sin_cache, "cos_sin_cache", _F16),
          *caches,
          _chk(slot_mapping, "slot_mapping", _I64), num_heads, num_kv_heads, head_size, cos_sin_cache.shape[-1],
          _opt(ln_linear_workspace(hidden_in.device, M), "sync_workspace"), _stream())
    return qkv


def ln_gate_up_silu_linear(hidden_in, delta, hidden_out, eps, wq, w_scale, act):
    """Draft pass: hidden_out = hidden_in + delta; LN + int4 quant; gate_up GEMM; silu(gate)*up -- one launch
    (quarot_llama.py:380-388 + 276-284)."""
    M, K = hidden_in.shape
    I = wq.shape[0] // 2
    _call("qspec_ln_gate_up_silu_linear_s4s4", _chk(hidden_in, "hidden_in", _F16), _opt(delta, "delta", _F16),
          _opt(hidden_out, "hidden_out", _F16), float(eps), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _chk(act, "act", _F16), M, I, K, _opt(ln_linear_workspace(hidden_in.device, M), "sync_workspace"), _stream())
    return act


def rowwise_scaled_linear_cutlass_s4s4_unified(xq, x_scale, wq, w_scale, bias, out):
    """torch.ops.torchao.rowwise_scaled_linear_cutlass_s4s4_unified (third-party/ao/torchao/ops.py:600-636)."""
    M, Kb = xq.shape
    N = wq.shape[0]
    if wq.shape[1] != Kb:
        raise RuntimeError(f"xq and wq disagree on K: {xq.shape} vs {wq.shape}")
    if out.shape[0] != M or out.shape[1] != N:
        raise RuntimeError(f"out has shape {tuple(out.shape)}, expected ({M}, {N})")
    _call("qspec_rowwise_scaled_linear_s4s4", _chk(xq, "xq", (_I8, _U8)), _chk(x_scale, "x_scale", _F16),
          _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16), _opt(bias, "bias", _F16),
          _chk(out, "out", _F16), M, N, Kb * 2, _stream())
    return out


def rowwise_scaled_linear_s4s4_residual(xq, x_scale, wq, w_scale, resid_in, resid_out):
    """resid_out = resid_in + linear_s4s4(xq) (fp16 add of the fp16 GEMM result) in one launch (quarot_llama.py:380,390)."""
    M, Kb = xq.shape
    N = wq.shape[0]
    _call("qspec_rowwise_scaled_linear_s4s4_residual", _chk(xq, "xq", (_I8, _U8)), _chk(x_scale, "x_scale", _F16),
          _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16), _chk(resid_in, "resid_in", _F16),
          _chk(resid_out, "resid_out", _F16), M, N, Kb * 2, _stream())
    return resid_out


def rowwise_scaled_linear_s4s4_residual_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().qspec_rowwise_scaled_linear_s4s4_residual_supported(M, N, K))


def rowwise_scaled_linear_s4s4_residual_hq(x16, part_amax, clip_ratio, wq, w_scale, resid_in, resid_out):
    """rowwise_scaled_linear_s4s4_residual on UNQUANTISED fp16 rows: the row-absmax int4 quantiser (quarot_llama.py:235-238,
    quant.cu:102-167) runs in the GEMM's prologue from `part_amax` [M, n_parts] partial row maxima."""
    M, K = x16.shape
    N = wq.shape[0]
    _call("qspec_rowwise_scaled_linear_s4s4_residual_hq", _chk(x16, "x16", _F16), _chk(part_amax, "part_amax", _F32),
          part_amax.shape[1], float(clip_ratio), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _chk(resid_in, "resid_in", _F16), _chk(resid_out, "resid_out", _F16), M, N, K, _stream())
    return resid_out


def rowwise_scaled_linear_s4s4_residual_hq_supported(M: int, N: int, K: int, n_parts: int = 8) -> bool:
    return bool(_lib.load().qspec_rowwise_scaled_linear_s4s4_residual_hq_supported(M, N, K, n_parts))


def w4a16_workspace(device):
    """Zero-initialised split-K scratch of the W4A16 kernels, one per (device, stream): calls on one stream are
    serialised, so they can share it (every call leaves the ticket counters at zero); two streams must not."""
    return _workspace("w4a16", device)


def w4a16_linear(x, wq, w_scale, out, bias=None, xp: bool = False, tokens=None):
    """bitblas.Matmul(x, w ^ 0x88, output=out, scale=w_scale, bias=bias) on the SAME packed buffer
    (quarot_nn/linear.py:122)."""
    M, K = x.shape
    N = wq.shape[0]
    if wq.shape[1] * 2 != K:
        raise RuntimeError(f"x and wq disagree on K: {x.shape} vs {wq.shape}")
    if xp:
        M = M if tokens is None else tokens
        _xp_tile(x, "x", K)
    _call("qspec_w4a16_linear" + ("_xp" if xp else ""), _chk(x, "x", _F16), _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16),
          _opt(bias, "bias", _F16), _chk(out, "out", _F16), M, N, K, w4a16_workspace(x.device).data_ptr(), _stream())
    return out


def w4a16_linear_partial_slices(M: int, N: int, K: int) -> int:
    """Slices the long-K W4A16 path cuts K into for this shape (0: use w4a16_linear)."""
    return int(_lib.load().qspec_w4a16_linear_partial_slices(M, N, K))


def w4a16_linear_partial(x, wq, part, slices: int, xp: bool = False, tokens=None):
    """Raw fp32 K-slice sums of x @ dequant(wq)^T into part [slices, M, N] (finished by add_rms_norm_fp16_partial)."""
    M, K = x.shape
    N = wq.shape[0]
    if xp:
        M = M if tokens is None else tokens
        _xp_tile(x, "x", K)
    _call("qspec_w4a16_linear_partial" + ("_xp" if xp else ""), _chk(x, "x", _F16), _chk(wq, "wq", (_I8, _U8)), _chk(part, "part", _F32), M, N, K,
          slices, _stream())
    return part


def add_rms_norm_fp16_partial(out, hidden_out, x, part, w_scale, slices: int, eps: float, xp: bool = False):
    """hidden_out = x + h(sum_s part[s] * w_scale); out = LN(hidden_out) -- the finish of w4a16_linear_partial fused in."""
    H = x.shape[-1]
    T = x.numel() // H
    if xp:
        _xp_tile(out, "out", H, T)
    _call("qspec_add_rms_norm_fp16_partial" + ("_xp" if xp else ""), _chk(out, "out", _F16), _chk(hidden_out, "hidden_out", _F16),
          _chk(x, "x", _F16), _chk(part, "part", _F32), _chk(w_scale, "w_scale", _F16), slices, float(eps), T, H, _stream())


def rowwise_scaled_linear_s4s4_partial_slices(M: int, N: int, K: int) -> int:
    """K slices the s4s4 linear is cut into at this shape (17..32 tokens, one weight tile per workgroup); 0: use the plain entry."""
    return int(_lib.load().qspec_rowwise_scaled_linear_s4s4_partial_slices(M, N, K))


def rowwise_scaled_linear_s4s4_partial(xq, wq, ipart, slices: int):
    """Raw int32 K-slice sums of xq @ wq^T into ipart [slices, M, N] (finished by add_rms_norm_ipartial)."""
    M, N, K = xq.shape[0], wq.shape[0], 2 * xq.shape[1]
    _call("qspec_rowwise_scaled_linear_s4s4_partial", _chk(xq, "xq", (_I8, _U8)), _chk(wq, "wq", (_I8, _U8)),
          _chk(ipart, "ipart", _I32), M, N, K, slices, _stream())
    return ipart


def add_rms_norm_ipartial(hidden_out, x, ipart, x_scale, w_scale, slices: int, eps: float, q=None, scale=None, out_f16=None):
    """hidden_out = x + h((sum_s ipart[s]) * x_scale[row] * w_scale[col]) (the s4s4 epilogue + residual add); then the norm of
    hidden_out: int4 rows q + scale, or fp16 rows out_f16."""
    H = x.shape[-1]
    T = x.numel() // H
    _call("qspec_add_rms_norm_ipartial", _opt(q, "q", _I8), _opt(scale, "scale", _F16), _opt(out_f16, "out_f16", _F16),
          _chk(hidden_out, "hidden_out", _F16), _chk(x, "x", _F16), _chk(ipart, "ipart", _I32), _chk(x_scale, "x_scale", _F16),
          _chk(w_scale, "w_scale", _F16), slices, float(eps), T, H, _stream())


def w4a16_linear_ksliced(x, wq, w_scale, out, k0: int, k1: int):
    """Row-parallel shard: out = x[:, k0:k1] @ dequant(wq)[:, k0:k1]^T * w_scale (partial sum; caller all-reduces).
    x [M,K] and wq [N,K/2] are the FULL tensors; only the K range is read."""
    M, K = x.shape
    N = wq.shape[0]
    _chk(x, "x", _F16); _chk(wq, "wq", (_I8, _U8))
    _call("qspec_w4a16_linear_ksliced", x.data_ptr() + 2 * k0, K, wq.data_ptr() + k0 // 2, K // 2,
          _chk(w_scale, "w_scale", _F16), _chk(out, "out", _F16), M, N, k1 - k0, w4a16_workspace(x.device).data_ptr(),
          _stream())
    return out


def w4a16_linear_ksliced_raw(x, wq, part, k0: int, k1: int):
    """Row-parallel shard as raw fp32 sums: part [M, N] = x[:, k0:k1] @ dequant(wq)[:, k0:k1]^T (no scale, no
    rounding); reduced across ranks in fp32, finished by add_rms_norm_fp16_partial(..., slices=1)."""
    M, K = x.shape
    N = wq.shape[0]
    _chk(x, "x", _F16); _chk(wq, "wq", (_I8, _U8))
    _call("qspec_w4a16_linear_ksliced_raw", x.data_ptr() + 2 * k0, K, wq.data_ptr() + k0 // 2, K // 2,
          _chk(part, "part", _F32), M, N, k1 - k0, w4a16_workspace(x.device).data_ptr(), _stream())
    return part


def gate_up_silu_linear_shard(x, wq, w_scale, act, ch0: int, nch: int):
    """Column-parallel shard of the fused gate_up + silu*up: writes act[:, ch0:ch0+nch] (act is the full [M, I])."""
    M = x.shape[0]
    I = wq.shape[0] // 2
    K = wq.shape[1] * 2
    _call("qspec_gate_up_silu_linear_w4a16_shard", _chk(x, "x", _F16), _chk(wq, "wq", (_I8, _U8)),
          _chk(w_scale, "w_scale", _F16), _chk(act, "act", _F16), M, I, K, ch0, nch,
          w4a16_workspace(x.device).data_ptr(), _stream())
    return act


def linear_f16(x, w, out):
    M, K = x.shape
    N = w.shape[0]
    _call("qspec_linear_f16", _chk(x, "x", _F16), _chk(w, "w", _F16), _chk(out, "out", _F16), M, N, K, _stream())
    return out


def dequant_w4(wq, w_scale, out):
    N, Kb = wq.shape
    _call("qspec_dequant_w4", _chk(wq, "wq", (_I8, _U8)), _chk(w_scale, "w_scale", _F16), _chk(out, "out", _F16), N,
          Kb * 2, _stream())
    return out


# ------------------------------------------------------------------ attention side

def rotary_embedding(positions, query, key, head_size: int, cos_sin_cache, is_neox: bool = True):
    """torch.ops._C.rotary_embedding (csrc/pos_encoding_kernels.cu:124); query/key [T, n*head_size], last dim contiguous."""
    if not is_neox:
        raise RuntimeError("only the NeoX layout is on the QSpec path (quarot_llama.py:104)")
    T = positions.numel()
    for t, n in ((query, "query"), (key, "key")):
        if t.stride(-1) != 1 or t.dtype != _F16 or not t.is_cuda:
            raise RuntimeError(f"{n}: need fp16 HIP tensor with unit inner stride")
    nq, nk = query.shape[-1] // head_size, key.shape[-1] // head_size
    _call("qspec_rotary_embedding", _chk(positions, "positions", _I64), query.data_ptr(), key.data_ptr(),
          _chk(cos_sin_cache, "cos_sin_cache", _F16), T, nq, nk, head_size, cos_sin_cache.shape[-1],
          query.stride(0), key.stride(0), _stream())


def reshape_and_cache_flash(key, value, key_cache, value_cache, slot_mapping, k_scale: float = 1.0, v_scale: float = 1.0):
    """torch.ops._C_cache_ops.reshape_and_cache_flash (csrc/cache_kernels.cu:304); key/value [T, n_kv, d]."""
    T, nkv, d = key.shape
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    _call("qspec_reshape_and_cache_flash" + kv8, key.data_ptr(), value.data_ptr(), *caches, _chk(slot_mapping, "slot_mapping", _I64), T, nkv, d, key.stride(0),
          value.stride(0), _stream())


def rope_kv_write(positions, qkv, cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads,
                  head_size, k_scale: float = 1.0, v_scale: float = 1.0):
    T = qkv.shape[0]
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    _call("qspec_rope_kv_write" + kv8, _chk(positions, "positions", _I64), _chk(qkv, "qkv", _F16),
          _chk(cos_sin_cache, "cos_sin_cache", _F16), *caches, _chk(slot_mapping, "slot_mapping", _I64), T, num_heads,
          num_kv_heads, head_size, cos_sin_cache.shape[-1], _stream())


def paged_attention_workspace_bytes(max_tokens, num_heads, head_size, n_splits) -> int:
    return int(_lib.load().qspec_paged_attention_workspace_bytes(max_tokens, num_heads, head_size, n_splits))


# attention_common.cuh: AttnFamily, as paged_attention_family returns it
ATTN_NO_LAUNCH, ATTN_GENERIC, ATTN_GENERIC_VEC, ATTN_PREFILL, ATTN_WAVES, ATTN_CHUNK, ATTN_PREFILL_SPLIT = range(7)


def paged_attention_family(n_seqs, max_q_len, num_heads, num_kv_heads, head_size, block_size, max_blocks_per_seq, n_splits,
                           merged: bool) -> int:
    """The kernel family paged_attention() launches for a call of this shape (0: refused, or nothing to launch); merged: `out`
    given.  The library's own launch plan, evaluated without a device."""
    return int(_lib.load().qspec_paged_attention_family(n_seqs, max_q_len, num_heads, num_kv_heads, head_size, block_size,
                                                        max_blocks_per_seq, n_splits, int(bool(merged))))


def paged_attention(q, q_stride, key_cache, value_cache, block_tables, ctx_lens, q_start, tokens, max_q_len,
                    num_heads, sm_scale, n_splits, workspace, out, k_scale: float = 1.0, v_scale: float = 1.0):
    """flash_attn_with_kvcache / flash_attn_varlen_func over the paged cache (flash_attn.py:741-830); an fp8 cache
    (uint8 / float8_e4m3fn tensors) is read as float(e4m3) * scale (paged_attn.py, kv_cache_dtype = "fp8")."""
    nb, bs, nkv, d = key_cache.shape
    n_seqs = ctx_lens.numel()
    kv8, caches = _kv(key_cache, value_cache, k_scale, v_scale)
    _call("qspec_paged_attention" + kv8, q.data_ptr(), q_stride, *caches, _chk(block_tables, "block_tables", _I32), block_tables.shape[1],
          _chk(ctx_lens, "ctx_lens", _I32), _chk(q_start, "q_start", _I32), n_seqs, tokens, max_q_len, num_heads, nkv,
          d, bs, float(sm_scale), n_splits, workspace.data_ptr(), _opt(out, "out", _F16), _stream())


def heads_hadamard_merged(workspace, max_tokens, n_splits, tokens, heads, head_dim, had_scale: float, out_f16=None,
                          q=None, scale=None, clip_ratio: float = 1.0, xp: bool = False):
    """Split merge of paged_attention(..., out=None) + heads_hadamard in one launch."""
    if xp:
        _xp_tile(out_f16, "out_f16", heads * head_dim, tokens)
    _call("qspec_heads_hadamard_merged" + ("_xp" if xp else ""), workspace.data_ptr(), max_tokens, n_splits, _opt(out_f16, "out_f16", _F16),
          _opt(q, "q", _I8), _opt(scale, "scale", _F16), float(had_scale), float(clip_ratio), tokens, heads, head_dim,
          _stream())


def heads_hadamard_merged_spread(workspace, max_tokens, n_splits, tokens, heads, head_dim, had_scale: float, out_f16, part_amax):
    """heads_hadamard_merged spread over 8 workgroups per token: fp16 rows + part_amax [tokens, 8] (the quantiser then runs in
    rowwise_scaled_linear_s4s4_residual_hq)."""
    _call("qspec_heads_hadamard_merged_spread", workspace.data_ptr(), max_tokens, n_splits, _chk(out_f16, "out_f16", _F16),
          _chk(part_amax, "part_amax", _F32), float(had_scale), tokens, heads, head_dim, _stream())


def heads_hadamard_merged_spread_supported(tokens: int, heads: int, head_dim: int) -> bool:
    return bool(_lib.load().qspec_heads_hadamard_merged_spread_supported(tokens, heads, head_dim))


def heads_hadamard_mix_merged_spread(workspace, max_tokens, n_splits, tokens, heads, head_dim, hadK, K: int, had_scale: float,
                                     out_f16, part_amax=None, xp: bool = False):
    """The spread merge + head transform for head counts with a table factor (40 heads = had40): fp16 rows, and with
    part_amax [tokens, 8] the partial row maxima for rowwise_scaled_linear_s4s4_residual_hq."""
    if xp:
        _xp_tile(out_f16, "out_f16", heads * head_dim, tokens)
    _call("qspec_heads_hadamard_mix_merged_spread" + ("_xp" if xp else ""), workspace.data_ptr(), max_tokens, n_splits, _chk(hadK, "hadK", _F16), K,
          _chk(out_f16, "out_f16", _F16), _opt(part_amax, "part_amax", _F32), float(had_scale), tokens, heads, head_dim,
          _stream())


def heads_hadamard_mix_merged_spread_supported(tokens: int, heads: int, head_dim: int, K: int) -> bool:
    return bool(_lib.load().qspec_heads_hadamard_mix_merged_spread_supported(tokens, heads, head_dim, K))


# ------------------------------------------------------------------ token side

def embedding(ids, table, out):
    T = ids.numel()
    V, H = table.shape
    _call("qspec_embedding", _chk(ids, "ids", _I64), _chk(table, "table", _F16), _chk(out, "out", _F16), T, H, V,
          _stream())
    return out


def _sampler_ws(rows: int, device, workspace=None):
    """Scratch for the chunked softmax / rejection kernels (64 partials per row); cached per (device, stream, rows)."""
    return workspace if workspace is not None else _workspace("sampler", device, rows=rows)


def softmax_argmax(logits, probs, token, workspace=None):
    T, V = logits.shape
    ws = _sampler_ws(T, logits.device, workspace)
    _call("qspec_softmax_argmax", _chk(logits, "logits", _F16), _chk(probs, "probs", _F32), _chk(token, "token", _I64),
          T, V, ws.data_ptr(), _stream())


def lm_head_softmax_argmax_supported(T: int, V: int, K: int) -> bool:
    return bool(_lib.load().qspec_lm_head_softmax_argmax_supported(T, V, K))


def lm_head_softmax_argmax(hidden, lm_head, logits, probs, token):
    """logits = hidden @ lm_head^T (fp16, scratch), probs = softmax(float(logits)), token = argmax -- the lm_head launch
    hands its row maxima to the softmax, probs is written once (logits_processor.py:92-97 + sampler.py:270-287)."""
    T, K = hidden.shape
    V = lm_head.shape[0]
    _call("qspec_lm_head_softmax_argmax", _chk(hidden, "hidden", _F16), _chk(lm_head, "lm_head", _F16),
          _chk(logits, "logits", _F16), _chk(probs, "probs", _F32), _chk(token, "token", _I64), T, V, K,
          _workspace("lm_head", hidden.device, rows=T).data_ptr(), _stream())


def _seq_seed_args(seq_seeds, seq_seeded, base_pos, nseq: int):
    """The per-sequence arrays of the seeded entries: all three or none."""
    given = [t is not None for t in (seq_seeds, seq_seeded, base_pos)]
    if not any(given):
        return None
    if not all(given):
        raise RuntimeError("seq_seeds, seq_seeded and base_pos go together")
    for t, name in ((seq_seeds, "seq_seeds"), (seq_seeded, "seq_seeded"), (base_pos, "base_pos")):
        if t.numel() < nseq:
            raise RuntimeError(f"{name} has {t.numel()} entries, {nseq} sequences need one each")
    return (_chk(seq_seeds, "seq_seeds", _I64), _chk(seq_seeded, "seq_seeded", _I32), _chk(base_pos, "base_pos", _I32))


def rejection_sample(target_with_bonus_probs, bonus_token_ids, draft_probs, draft_token_ids, out_tokens, accepted,
                     recovered, counters=None, uniform=None, exponential=None, seed: int = 0, offset: int = 0,
                     rng_state=None, workspace=None, active_lens=None, seq_seeds=None, seq_seeded=None, base_pos=None):
    """seq_seeds [B] int64 / seq_seeded [B] int32 / base_pos [B] int32 (all or none): rows b with seq_seeded[b] != 0 draw
    from Philox keyed by (seq_seeds[b], base_pos[b]) alone -- qspec_rejection_sample_seeded (include/qspec_hip.h)."""
    B, k, V = draft_probs.shape
    # draft_probs / draft_token_ids / bonus_token_ids may be strided views (step-major draft buffers)
    if draft_probs.stride(2) != 1 or draft_probs.dtype != _F32 or draft_token_ids.dtype != _I64 \
            or bonus_token_ids.dtype != _I64 or not draft_probs.is_cuda:
        raise RuntimeError("draft_probs must be fp32 with unit inner stride; ids int64; all on the GPU")
    seeded = _seq_seed_args(seq_seeds, seq_seeded, base_pos, B)
    args = (_chk(target_with_bonus_probs, "target_with_bonus_probs", _F32),
            bonus_token_ids.data_ptr(), draft_probs.data_ptr(), draft_token_ids.data_ptr(),
            _opt(uniform, "uniform", _F32), _opt(exponential, "exponential", _F32), seed, offset,
            _opt(rng_state, "rng_state", _I64), B, k, V, draft_probs.stride(0), draft_probs.stride(1),
            draft_token_ids.stride(0), draft_token_ids.stride(1),
            bonus_token_ids.stride(0) if bonus_token_ids.numel() > 1 else 1, _chk(out_tokens, "out_tokens", _I64),
            _chk(accepted, "accepted", _U8), _chk(recovered, "recovered", _I64), _opt(counters, "counters", _I64),
            _opt(active_lens, "active_lens", _I32))
    ws = _sampler_ws(B * k, draft_probs.device, workspace).data_ptr()
    if seeded is None:
        _call("qspec_rejection_sample", *args, ws, _stream())
    else:
        _call("qspec_rejection_sample_seeded", *args, *seeded, ws, _stream())


def sample_workspace(rows: int, device):
    """Histogram workspace of sample_top_k_top_p: zero-filled once per (device, stream, rows), left zeroed by every call."""
    return _workspace("sample", device, rows=rows)


def new_sample_workspace(rows: int, device):
    """A private zero-filled histogram workspace of sample_top_k_top_p for `rows` rows (callers that must not rely on the
    lazily created shared one being zeroed outside a graph capture)."""
    return torch.zeros(int(_lib.load().qspec_sample_workspace_bytes(rows)), dtype=torch.uint8, device=device)


def sample_top_k_top_p(logits, probs, token, temperature=None, top_k=None, top_p=None, exponential=None, seed: int = 0,
                       offset: int = 0, rng_state=None, workspace=None, seq_seeds=None, seq_seeded=None, base_pos=None,
                       rows_per_seq: int = 1, j_base: int = 0, draw_stream: int = 2, min_p=None):
    """Sampler.forward for non-greedy rows (sampler.py:216-316): temperature, top-k / top-p masking, softmax, multinomial by
    exponential noise.  temperature / top_p [T] fp32, top_k [T] int32 on the device (None: 1.0 / off).
    seq_seeds int64 / seq_seeded int32 / base_pos int32, one entry per SEQUENCE (all or none): row t belongs to sequence
    t // rows_per_seq, and rows of seeded sequences draw from Philox keyed by (seed, base_pos, draw_stream,
    j_base + t % rows_per_seq) alone -- qspec_sample_top_k_top_p_seeded (include/qspec_hip.h).
    min_p [T] fp32 (None: the entry points without it): _apply_min_p behind top-k / top-p, tokens whose probability is below
    min_p x the row's largest are masked -- qspec_sample_top_k_top_p_min_p(_seeded)."""
    T, V = logits.shape
    if min_p is not None and min_p.numel() < T:
        raise RuntimeError(f"min_p has {min_p.numel()} entries, {T} rows need one each")
    ws = workspace if workspace is not None else sample_workspace(T, logits.device)
    nseq = (T + rows_per_seq - 1) // max(1, rows_per_seq)
    seeded = _seq_seed_args(seq_seeds, seq_seeded, base_pos, nseq)
    args = (_chk(logits, "logits", _F16), _opt(temperature, "temperature", _F32),
            _opt(top_k, "top_k", _I32), _opt(top_p, "top_p", _F32), _opt(exponential, "exponential", _F32), seed, offset,
            _opt(rng_state, "rng_state", _I64), _chk(probs, "probs", _F32), token.data_ptr(), token.stride(0) if token.dim() else 1,
            T, V)
    suffix = ""
    if min_p is not None:   # (the min_p array sits behind top_p in the argument list)
        args = args[:4] + (_chk(min_p, "min_p", _F32),) + args[4:]
        suffix = "_min_p"
    if seeded is None:
        _call("qspec_sample_top_k_top_p" + suffix, *args, ws.data_ptr(), _stream())
    else:
        _call("qspec_sample_top_k_top_p" + suffix + "_seeded", *args, *seeded, seq_seeds.numel(), rows_per_seq, j_base,
              draw_stream, ws.data_ptr(), _stream())


# ------------------------------------------------------------------ logprobs (include/qspec_hip.h, "Logprobs")
MAX_LOGPROBS = 32   # QS_MAX_LOGPROBS


def _token_logprobs(entry, x, dtype, token_ids, num_top: int, token_logprob, token_rank, top_ids, top_logprobs):
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != dtype or not x.is_cuda:
        raise RuntimeError(f"x must be a [rows, vocab] {dtype} HIP tensor with unit inner stride (rows may be strided: no CPU "
                           "fallback, no copy)")
    rows, vocab = x.shape
    if not 0 <= num_top <= MAX_LOGPROBS:
        raise ValueError(f"num_top = {num_top} outside 0..{MAX_LOGPROBS}")
    for t, name, n in ((token_ids, "token_ids", rows), (token_logprob, "token_logprob", rows), (token_rank, "token_rank", rows)) \
            + (((top_ids, "top_ids", rows * num_top), (top_logprobs, "top_logprobs", rows * num_top)) if num_top else ()):
        if t is None or t.numel() < n:
            raise RuntimeError(f"{name} needs {n} entries")
    _call(entry, x.data_ptr(), x.stride(0) if rows > 1 else max(x.stride(0), vocab), _chk(token_ids, "token_ids", _I64), rows, vocab,
          num_top, _chk(token_logprob, "token_logprob", _F32), _chk(token_rank, "token_rank", _I32),
          _chk(top_ids, "top_ids", _I32) if num_top else None, _chk(top_logprobs, "top_logprobs", _F32) if num_top else None,
          _stream())


def token_logprobs_from_probs(probs, token_ids, num_top: int, token_logprob, token_rank, top_ids=None, top_logprobs=None):
    """Sampler logprobs of the PROCESSED distribution (sampler.py:284, _get_ranks :861-879, get_logprobs :882 ff.): per row of
    probs [rows, V] fp32 the logprob logf(max(p, FLT_MIN)) and rank of token_ids[row] (int64; outside [0, V): 0.0 / -1) and the
    num_top most probable ids (int32, ties lowest id first) with their logprobs -- qspec_token_logprobs_from_probs."""
    _token_logprobs("qspec_token_logprobs_from_probs", probs, _F32, token_ids, num_top, token_logprob, token_rank, top_ids,
                    top_logprobs)


def token_logprobs_from_logits(logits, token_ids, num_top: int, token_logprob, token_rank, top_ids=None, top_logprobs=None):
    """The same from raw fp16 logits [rows, V]: lp = log_softmax(logits.float(), -1) -- qspec_token_logprobs_from_logits."""
    _token_logprobs("qspec_token_logprobs_from_logits", logits, _F16, token_ids, num_top, token_logprob, token_rank, top_ids,
                    top_logprobs)


# ------------------------------------------------------------------ logit processors (include/qspec_hip.h, "logit processors")
MAX_STOP_IDS = 16   # QS_MAX_STOP_IDS


def new_logit_table(num_slots: int, vocab: int, device):
    """(tok_table [num_slots, vocab] int32 -- bit 31: in the prompt, low bits: output count --, counted_len [num_slots] int32)."""
    return (torch.zeros(num_slots, vocab, dtype=_I32, device=device), torch.zeros(num_slots, dtype=_I32, device=device))


def logit_table_set_prompt(tok_table, counted_len, slot: int, prompt_ids, output_ids=None):
    """Rebuild the table row of `slot` at admission: prompt_ids / output_ids int64 device tensors (output_ids: the outputs a
    re-admitted request already has); counted_len[slot] = 0."""
    B, V = tok_table.shape
    n_out = 0 if output_ids is None else output_ids.numel()
    _call("qspec_logit_table_set_prompt", _chk(tok_table, "tok_table", _I32), _chk(counted_len, "counted_len", _I32), B, V,
          int(slot), _chk(prompt_ids, "prompt_ids", _I64), prompt_ids.numel(),
          _chk(output_ids, "output_ids", _I64) if n_out else None, n_out, _stream())


def logit_table_catch_up(tok_table, counted_len, need_counts, gen_tokens, gen_lens):
    """Count gen_tokens[slot][counted_len .. gen_lens) of every slot with need_counts != 0; counted_len = gen_lens.  Idempotent."""
    B, V = tok_table.shape
    if gen_tokens.shape[0] < B or gen_lens.numel() < B or need_counts.numel() < B or counted_len.numel() < B:
        raise RuntimeError("the per-slot arrays are shorter than the table")
    _call("qspec_logit_table_catch_up", _chk(tok_table, "tok_table", _I32), _chk(counted_len, "counted_len", _I32),
          _chk(need_counts, "need_counts", _I32), B, V, _chk(gen_tokens, "gen_tokens", _I64), gen_tokens.shape[1],
          _chk(gen_lens, "gen_lens", _I32), _stream())


def _process_logits_args(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                         num_stop_ids, draft_ids, rows_per_seq: int, j_base: int, slot_ids, active_lens):
    """The checks and the leading C arguments process_logits and process_logits_constrained share."""
    T, V = logits.shape
    B = tok_table.shape[0]
    if tok_table.shape[1] != V or out.shape != logits.shape:
        raise RuntimeError("tok_table / out do not match the logits")
    for t, name in ((repetition, "repetition"), (frequency, "frequency"), (presence, "presence"), (min_tokens, "min_tokens"),
                    (gen_base, "gen_base"), (gen_lens, "gen_lens"), (num_stop_ids, "num_stop_ids")):
        if t.numel() < B:
            raise RuntimeError(f"{name} has {t.numel()} entries, the table has {B} slots")
    if stop_ids.dim() != 2 or stop_ids.shape[0] < B:
        raise RuntimeError("stop_ids must be [num_slots, width]")
    nseq = (T + rows_per_seq - 1) // max(1, rows_per_seq)
    if slot_ids is not None and slot_ids.numel() < nseq:
        raise RuntimeError(f"slot_ids has {slot_ids.numel()} entries, {nseq} sequences need one each")
    if active_lens is not None and active_lens.numel() < B:
        raise RuntimeError("active_lens is shorter than the table")
    n_draft, di_sb, di_sk, di_ptr = 0, 0, 0, None
    if draft_ids is not None:
        if draft_ids.dim() != 2 or draft_ids.shape[1] < B or draft_ids.dtype != _I64 or not draft_ids.is_cuda:
            raise RuntimeError("draft_ids must be an int64 [steps, num_slots] GPU tensor")
        n_draft, di_sk, di_sb, di_ptr = draft_ids.shape[0], draft_ids.stride(0), draft_ids.stride(1), draft_ids.data_ptr()
    return (_chk(logits, "logits", _F16), _chk(out, "out", _F16), T, V, _chk(tok_table, "tok_table", _I32), B,
            _opt(slot_ids, "slot_ids", _I32), _opt(active_lens, "active_lens", _I32), _chk(repetition, "repetition", _F16),
            _chk(frequency, "frequency", _F16), _chk(presence, "presence", _F16), _chk(min_tokens, "min_tokens", _I32),
            _chk(gen_base, "gen_base", _I32), _chk(gen_lens, "gen_lens", _I32), _chk(stop_ids, "stop_ids", _I32),
            _chk(num_stop_ids, "num_stop_ids", _I32), stop_ids.shape[1], di_ptr, n_draft, di_sb, di_sk, rows_per_seq, j_base)


def process_logits(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                   num_stop_ids, draft_ids=None, rows_per_seq: int = 1, j_base: int = 0, slot_ids=None, active_lens=None):
    """_apply_min_tokens_penalty + apply_penalties per row (sampler.py:258-266), out of place: out [T, V] fp16.  Row t belongs to
    sequence t // rows_per_seq (slot slot_ids[sequence] or the sequence index) with j = j_base + t % rows_per_seq and sees the
    in-flight tokens draft_ids[0 .. j, slot] (draft_ids [n, num_slots] int64, step-major as the engine keeps them; any strides).
    The per-slot arrays are device tensors read when the call runs."""
    _call("qspec_process_logits", *_process_logits_args(logits, out, tok_table, repetition, frequency, presence, min_tokens,
                                                        gen_base, gen_lens, stop_ids, num_stop_ids, draft_ids, rows_per_seq,
                                                        j_base, slot_ids, active_lens), _stream())
    return out


# ------------------------------------------------------------------ token constraints (include/qspec_hip.h, "token constraints")
MAX_LOGIT_BIAS = 512     # QS_MAX_LOGIT_BIAS
MAX_BAD_WORDS = 32       # QS_MAX_BAD_WORDS (multi-token words; single-token ones live in the deny bitmask)
MAX_BAD_WORD_LEN = 8     # QS_MAX_BAD_WORD_LEN


class TokenConstraints:
    """The per-slot device arrays of logit_bias / allowed_token_ids / bad words (all zero: no slot is constrained)."""

    def __init__(self, num_slots: int, vocab: int, device):
        z = lambda *shape, dtype=_I32: torch.zeros(*shape, dtype=dtype, device=device)   # noqa: E731
        self.num_slots, self.vocab = num_slots, vocab
        self.deny = z(num_slots, (vocab + 31) // 32)          # bit v: not allowed, or a single-token bad word
        self.meta = z(num_slots, 4)                           # flags, biases, multi-token words, tail tokens
        self.bias_ids = z(num_slots, MAX_LOGIT_BIAS)
        self.bias_vals = z(num_slots, MAX_LOGIT_BIAS, dtype=_F32)
        self.words = z(num_slots, MAX_BAD_WORDS, MAX_BAD_WORD_LEN)
        self.word_lens = z(num_slots, MAX_BAD_WORDS)
        self.tail = z(num_slots, MAX_BAD_WORD_LEN - 1)        # right-aligned: the outputs a request had before admission

    def arrays(self):
        return (self.deny, self.meta, self.bias_ids, self.bias_vals, self.words, self.word_lens, self.tail)


def token_constraints_set(tc: TokenConstraints, slot: int, logit_bias=None, allowed_token_ids=None, bad_words_token_ids=None):
    """Rebuild the constraint state of `slot` (admission time, outside any graph).  logit_bias: {id: bias} (ids distinct),
    allowed_token_ids: ids or None, bad_words_token_ids: lists of ids -- validated by the caller (the engine); here only the
    caps are enforced.  All None / empty: the slot's flags are cleared.  The tail (meta[3]) is reset to 0."""
    dev = tc.deny.device
    bias = sorted((int(t), float(b)) for t, b in (logit_bias or {}).items())
    allowed = sorted(set(int(t) for t in allowed_token_ids)) if allowed_token_ids is not None else []
    words = [[int(t) for t in w] for w in (bad_words_token_ids or [])]
    single = sorted(set(w[0] for w in words if len(w) == 1))
    multi = []
    for w in words:
        if len(w) > 1 and w not in multi:
            multi.append(w)
    if len(bias) > MAX_LOGIT_BIAS:
        raise ValueError(f"{len(bias)} logit_bias entries: at most {MAX_LOGIT_BIAS} are supported")
    if len(multi) > MAX_BAD_WORDS:
        raise ValueError(f"{len(multi)} multi-token bad words: at most {MAX_BAD_WORDS} are supported")
    if any(len(w) > MAX_BAD_WORD_LEN for w in multi):
        raise ValueError(f"a bad word is longer than {MAX_BAD_WORD_LEN} tokens")

    def dev_t(vals, dtype):
        return torch.tensor(vals, dtype=dtype).to(dev) if len(vals) else None
    a_t, s_t = dev_t(allowed, _I64), dev_t(single, _I64)
    bi_t, bv_t = dev_t([t for t, _ in bias], _I32), dev_t([b for _, b in bias], _F32)
    w_t = dev_t([w + [-1] * (MAX_BAD_WORD_LEN - len(w)) for w in multi], _I32)
    wl_t = dev_t([len(w) for w in multi], _I32)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _call("qspec_token_constraints_set", _chk(tc.deny, "deny", _I32), tc.deny.shape[1], _chk(tc.meta, "meta", _I32),
          _chk(tc.bias_ids, "bias_ids", _I32), _chk(tc.bias_vals, "bias_vals", _F32), _chk(tc.words, "words", _I32),
          _chk(tc.word_lens, "word_lens", _I32), tc.num_slots, tc.vocab, int(slot), ptr(a_t), len(allowed), ptr(s_t), len(single),
          ptr(bi_t), ptr(bv_t), len(bias), ptr(w_t), ptr(wl_t), len(multi), int(bool(words)), _stream())
    # (the staging tensors are freed behind the launch: the caching allocator reuses memory in stream order)


def token_constraints_set_tail(tc: TokenConstraints, slot: int, outputs_before_admission) -> None:
    """The last MAX_BAD_WORD_LEN - 1 outputs a re-admitted request had before its admission (right-aligned) and their number."""
    n = MAX_BAD_WORD_LEN - 1
    last = [int(t) for t in list(outputs_before_admission)[-n:]]
    tc.tail[slot].copy_(torch.tensor([-1] * (n - len(last)) + last, dtype=_I32))
    tc.meta[slot, 3] = len(last)


def process_logits_constrained(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                               num_stop_ids, deny, meta, bias_ids, bias_vals, words, word_lens, tail, gen_tokens,
                               draft_ids=None, rows_per_seq: int = 1, j_base: int = 0, slot_ids=None, active_lens=None):
    """process_logits with the token constraints in front of it, in the same launch: logit_bias, the deny bitmask (tokens outside
    allowed_token_ids, single-token bad words) and the multi-token bad words matched against the request's outputs -- the tail
    it had before admission, gen_tokens[slot][:gen_lens], the in-flight draft_ids[0 .. j, slot].  The arrays are those of a
    TokenConstraints; a slot whose meta row is zero gets the bits of process_logits."""
    V, B = logits.shape[1], tok_table.shape[0]
    args = _process_logits_args(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                                num_stop_ids, draft_ids, rows_per_seq, j_base, slot_ids, active_lens)
    if deny.dim() != 2 or deny.shape[0] < B or deny.shape[1] * 32 < V:
        raise RuntimeError("deny must be [num_slots, >= ceil(vocab / 32)]")
    for t, shape, name in ((meta, (4,), "meta"), (bias_ids, (MAX_LOGIT_BIAS,), "bias_ids"), (bias_vals, (MAX_LOGIT_BIAS,), "bias_vals"),
                           (words, (MAX_BAD_WORDS, MAX_BAD_WORD_LEN), "words"), (word_lens, (MAX_BAD_WORDS,), "word_lens"),
                           (tail, (MAX_BAD_WORD_LEN - 1,), "tail")):
        if t.shape[0] < B or tuple(t.shape[1:]) != shape:
            raise RuntimeError(f"{name} must be [num_slots, {', '.join(str(d) for d in shape)}]")
    if gen_tokens.dim() != 2 or gen_tokens.shape[0] < B:
        raise RuntimeError("gen_tokens must be [num_slots, capacity]")
    _call("qspec_process_logits_constrained", *args, _chk(deny, "deny", _I32), deny.shape[1], _chk(meta, "meta", _I32),
          _chk(bias_ids, "bias_ids", _I32), _chk(bias_vals, "bias_vals", _F32), _chk(words, "words", _I32),
          _chk(word_lens, "word_lens", _I32), _chk(tail, "tail", _I32), _chk(gen_tokens, "gen_tokens", _I64),
          gen_tokens.shape[1], _stream())
    return out


# ------------------------------------------------------------------ token guides (include/qspec_hip.h, "token guides")
MAX_GUIDE_WORDS = 8192   # words of an allow row the build kernel assembles in LDS: vocabularies up to 262144


class TokenGuides:
    """The device arena of the resident guides (allow / rank rows per state, offsets, transitions) and the per-slot guide state
    gslot [num_slots, 4] = {state, g_len, miss state, guided}; all zero: no slot is guided.  Where a guide sits in the arena
    is the caller's bookkeeping (spec_decode.guides.GuideArena)."""

    def __init__(self, num_slots: int, vocab: int, device, max_states: int, max_transitions: int):
        z = lambda *shape: torch.zeros(*shape, dtype=_I32, device=device)   # noqa: E731
        self.num_slots, self.vocab, self.max_states, self.max_transitions = num_slots, vocab, int(max_states), int(max_transitions)
        self.words = ((vocab + 31) // 32 + 3) // 4 * 4
        if self.words > MAX_GUIDE_WORDS:
            raise ValueError(f"vocabulary {vocab}: guides support at most {MAX_GUIDE_WORDS * 32} tokens")
        self.allow, self.rank = z(self.max_states, self.words), z(self.max_states, self.words)
        self.off, self.nxt = z(self.max_states), z(self.max_transitions)
        self.gslot = z(num_slots, 4)

    def arrays(self):
        return (self.allow, self.rank, self.off, self.nxt, self.gslot)

    def set_slot(self, slot: int, state: int = 0, miss: int = 0, guided: bool = False, g_len: int = 0) -> None:
        self.gslot[slot].copy_(torch.tensor([state, g_len, miss, 1] if guided else [0, 0, 0, 0], dtype=_I32))


def guide_build(tg: TokenGuides, state_base: int, trans_base: int, row_ptr, tokens, next_states, row_stride=None) -> None:
    """Build the rows of one guide (numpy CSR, validated by the caller: spec_decode.guides.TokenFSM) at arena rows state_base ..
    and transitions trans_base .. (admission time, outside any graph)."""
    dev = tg.allow.device
    S, N = int(row_ptr.shape[0]) - 1, int(tokens.shape[0])
    if S < 1 or N < 1 or state_base < 0 or trans_base < 0 or state_base + S > tg.max_states or trans_base + N > tg.max_transitions:
        raise ValueError(f"a guide of {S} states and {N} transitions at ({state_base}, {trans_base}) does not fit the arena "
                         f"({tg.max_states} states, {tg.max_transitions} transitions)")
    up = lambda a: torch.from_numpy(a.astype("int32")).to(dev)   # noqa: E731
    rp, tk, nx = up(row_ptr), up(tokens), up(next_states)
    stride = tg.allow.stride(0) if row_stride is None else int(row_stride)
    _call("qspec_guide_build", _chk(tg.allow, "guide_allow", _I32), _chk(tg.rank, "guide_rank", _I32), _chk(tg.off, "guide_off", _I32),
          _chk(tg.nxt, "guide_next", _I32), tg.words, stride, tg.vocab, tg.max_states, tg.max_transitions, int(state_base),
          int(trans_base), S, N, _chk(rp, "row_ptr", _I32), _chk(tk, "tokens", _I32), _chk(nx, "next_states", _I32), _stream())
    # (the staging tensors are freed behind the launch: the caching allocator reuses memory in stream order)


def _guide_args(tg_arrays):
    allow, rank, off, nxt, gslot = tg_arrays
    if allow.dim() != 2 or rank.shape != allow.shape or off.numel() < allow.shape[0] or gslot.dim() != 2 or gslot.shape[1] != 4:
        raise RuntimeError("the guide arrays are those of a TokenGuides")
    return (_chk(allow, "guide_allow", _I32), _chk(rank, "guide_rank", _I32), _chk(off, "guide_off", _I32),
            _chk(nxt, "guide_next", _I32)), _chk(gslot, "guide_slots", _I32), (allow.shape[1], allow.shape[0], nxt.numel())


def guide_catch_up(guide_allow, guide_rank, guide_off, guide_next, guide_slots, vocab: int, gen_tokens, gen_lens):
    """Advance the state of every guided slot over gen_tokens[slot][g_len .. gen_lens); g_len = gen_lens.  Idempotent."""
    B = guide_slots.shape[0]
    if gen_tokens.shape[0] < B or gen_lens.numel() < B:
        raise RuntimeError("the per-slot arrays are shorter than guide_slots")
    arena, gslot, sizes = _guide_args((guide_allow, guide_rank, guide_off, guide_next, guide_slots))
    _call("qspec_guide_catch_up", gslot, B, int(vocab), *arena, *sizes, _chk(gen_tokens, "gen_tokens", _I64), gen_tokens.shape[1],
          _chk(gen_lens, "gen_lens", _I32), _stream())


def process_logits_guided(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                          num_stop_ids, deny, meta, bias_ids, bias_vals, words, word_lens, tail, gen_tokens, guide_allow,
                          guide_rank, guide_off, guide_next, guide_slots, draft_ids=None, rows_per_seq: int = 1, j_base: int = 0,
                          slot_ids=None, active_lens=None):
    """process_logits_constrained with the token guides in front of it, in the same launch: a row of a guided slot (guide_slots
    [num_slots, 4]) is masked with the allow row of the state reached from the slot's state over the in-flight
    draft_ids[0 .. j, slot], and gets an fp32 zero added to every element.  The guide arrays are those of a TokenGuides; a slot
    whose guide_slots row is zero gets the bits of process_logits_constrained."""
    V, B = logits.shape[1], tok_table.shape[0]
    args = _process_logits_args(logits, out, tok_table, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids,
                                num_stop_ids, draft_ids, rows_per_seq, j_base, slot_ids, active_lens)
    if deny.dim() != 2 or deny.shape[0] < B or deny.shape[1] * 32 < V:
        raise RuntimeError("deny must be [num_slots, >= ceil(vocab / 32)]")
    for t, shape, name in ((meta, (4,), "meta"), (bias_ids, (MAX_LOGIT_BIAS,), "bias_ids"), (bias_vals, (MAX_LOGIT_BIAS,), "bias_vals"),
                           (words, (MAX_BAD_WORDS, MAX_BAD_WORD_LEN), "words"), (word_lens, (MAX_BAD_WORDS,), "word_lens"),
                           (tail, (MAX_BAD_WORD_LEN - 1,), "tail")):
        if t.shape[0] < B or tuple(t.shape[1:]) != shape:
            raise RuntimeError(f"{name} must be [num_slots, {', '.join(str(d) for d in shape)}]")
    if gen_tokens.dim() != 2 or gen_tokens.shape[0] < B:
        raise RuntimeError("gen_tokens must be [num_slots, capacity]")
    if guide_slots.shape[0] < B or guide_allow.shape[1] * 32 < V:
        raise RuntimeError("guide_slots must cover the slots and the allow rows the vocabulary")
    arena, gslot, sizes = _guide_args((guide_allow, guide_rank, guide_off, guide_next, guide_slots))
    _call("qspec_process_logits_guided", *args, _chk(deny, "deny", _I32), deny.shape[1], _chk(meta, "meta", _I32),
          _chk(bias_ids, "bias_ids", _I32), _chk(bias_vals, "bias_vals", _F32), _chk(words, "words", _I32),
          _chk(word_lens, "word_lens", _I32), _chk(tail, "tail", _I32), _chk(gen_tokens, "gen_tokens", _I64),
          gen_tokens.shape[1], *arena, gslot, *sizes, _stream())
    return out


def typical_acceptance_sample(target_with_bonus_probs, bonus_token_ids, draft_token_ids, posterior_threshold: float,
                              posterior_alpha: float, out_tokens, accepted, recovered, counters=None, workspace=None,
                              active_lens=None):
    B, k1, V = target_with_bonus_probs.shape
    k = k1 - 1
    if draft_token_ids.dtype != _I64 or bonus_token_ids.dtype != _I64 or not target_with_bonus_probs.is_cuda:
        raise RuntimeError("ids must be int64; all tensors on the GPU")
    _call("qspec_typical_acceptance_sample", _chk(target_with_bonus_probs, "target_with_bonus_probs", _F32),
          bonus_token_ids.data_ptr(), draft_token_ids.data_ptr(), float(posterior_threshold), float(posterior_alpha), B, k, V,
          draft_token_ids.stride(0), draft_token_ids.stride(1),
          bonus_token_ids.stride(0) if bonus_token_ids.numel() > 1 else 1, _chk(out_tokens, "out_tokens", _I64),
          _chk(accepted, "accepted", _U8), _chk(recovered, "recovered", _I64), _opt(counters, "counters", _I64),
          _opt(active_lens, "active_lens", _I32), _sampler_ws(B * k, target_with_bonus_probs.device, workspace).data_ptr(), _stream())


def advance_step_flashattn(num_seqs, num_queries, block_size, input_tokens, sampled_token_ids, input_positions,
                           seq_lens, slot_mapping, block_tables):
    """ops.advance_step_flashattn (vllm/_custom_ops.py; csrc/prepare_inputs/advance_step.cu:192)."""
    if num_seqs != num_queries:
        raise RuntimeError("CUDA-graph padding (num_seqs != num_queries) is not used on this path")
    _call("qspec_advance_step_flashattn", num_seqs, block_size, _chk(input_tokens, "input_tokens", _I64),
          _chk(sampled_token_ids, "sampled_token_ids", _I64), _chk(input_positions, "input_positions", _I64),
          _chk(seq_lens, "seq_lens", _I32), _chk(slot_mapping, "slot_mapping", _I64),
          _chk(block_tables, "block_tables", _I32), block_tables.stride(0), _stream())


# ------------------------------------------------------------------ spec-decode cycle glue

def _embed_args(embed):
    """embed = (embed_tokens [V, H], hidden_out [rows, H]): the forward's embedding lookup rides in the bookkeeping launch."""
    table, out = embed
    return (_chk(table, "embed_tokens", _F16), _chk(out, "hidden_out", _F16), table.shape[1], table.shape[0])


def spec_advance_draft(block_size, input_tokens, sampled_token_ids, positions, ctx_lens, slot_mapping, block_tables, embed=None):
    """_gpu_advance_step between two draft steps (draft_model_runner.py:78-135) with the engine's empty-slot and
    out-of-blocks rules (include/qspec_hip.h)."""
    B = ctx_lens.numel()
    if embed is not None:
        _call("qspec_spec_advance_draft_embed", B, block_size, block_tables.shape[1], _chk(input_tokens, "input_tokens", _I64),
              _chk(sampled_token_ids, "sampled_token_ids", _I64), _chk(positions, "positions", _I64),
              _chk(ctx_lens, "ctx_lens", _I32), _chk(slot_mapping, "slot_mapping", _I64),
              _chk(block_tables, "block_tables", _I32), block_tables.stride(0), *_embed_args(embed), _stream())
        return
    _call("qspec_spec_advance_draft", B, block_size, block_tables.shape[1], _chk(input_tokens, "input_tokens", _I64),
          _chk(sampled_token_ids, "sampled_token_ids", _I64), _chk(positions, "positions", _I64),
          _chk(ctx_lens, "ctx_lens", _I32), _chk(slot_mapping, "slot_mapping", _I64),
          _chk(block_tables, "block_tables", _I32), block_tables.stride(0), _stream())


def spec_prepare_draft(last_token, seq_lens, block_tables, block_size, input_tokens, positions, slot_mapping,
                       ctx_lens, embed=None, step_mask=None, eff_lens=None):
    """embed given: the fused form; step_mask / eff_lens (fused form only): eff_lens = seq_lens * step_mask, used as the lengths."""
    B = seq_lens.numel()
    if embed is not None:
        _call("qspec_spec_prepare_draft_embed", B, block_size, block_tables.shape[1], _chk(last_token, "last_token", _I64),
              _chk(seq_lens, "seq_lens", _I32), _opt(step_mask, "step_mask", _I32), _opt(eff_lens, "eff_lens", _I32),
              _chk(block_tables, "block_tables", _I32), block_tables.stride(0),
              _chk(input_tokens, "input_tokens", _I64), _chk(positions, "positions", _I64),
              _chk(slot_mapping, "slot_mapping", _I64), _chk(ctx_lens, "ctx_lens", _I32), *_embed_args(embed), _stream())
        return
    if step_mask is not None:
        raise RuntimeError("step_mask rides in the fused form only (embed=...)")
    _call("qspec_spec_prepare_draft", B, block_size, block_tables.shape[1], _chk(last_token, "last_token", _I64),
          _chk(seq_lens, "seq_lens", _I32), _chk(block_tables, "block_tables", _I32), block_tables.stride(0),
          _chk(input_tokens, "input_tokens", _I64), _chk(positions, "positions", _I64),
          _chk(slot_mapping, "slot_mapping", _I64), _chk(ctx_lens, "ctx_lens", _I32), _stream())


def spec_prepare_verify(last_token, draft_token_ids, seq_lens, block_tables, block_size, tokens, positions,
                        slot_mapping, ctx_lens, embed=None):
    B, k = draft_token_ids.shape
    if embed is not None:
        _call("qspec_spec_prepare_verify_embed", B, k, block_size, block_tables.shape[1], _chk(last_token, "last_token", _I64),
              draft_token_ids.data_ptr(), draft_token_ids.stride(0), draft_token_ids.stride(1),
              _chk(seq_lens, "seq_lens", _I32),
              _chk(block_tables, "block_tables", _I32), block_tables.stride(0), _chk(tokens, "tokens", _I64),
              _chk(positions, "positions", _I64), _chk(slot_mapping, "slot_mapping", _I64),
              _chk(ctx_lens, "ctx_lens", _I32), *_embed_args(embed), _stream())
        return
    _call("qspec_spec_prepare_verify", B, k, block_size, block_tables.shape[1], _chk(last_token, "last_token", _I64),
          draft_token_ids.data_ptr(), draft_token_ids.stride(0), draft_token_ids.stride(1),
          _chk(seq_lens, "seq_lens", _I32),
          _chk(block_tables, "block_tables", _I32), block_tables.stride(0), _chk(tokens, "tokens", _I64),
          _chk(positions, "positions", _I64), _chk(slot_mapping, "slot_mapping", _I64),
          _chk(ctx_lens, "ctx_lens", _I32), _stream())


def spec_commit(out_tokens, seq_lens, last_token, gen_tokens=None, gen_lens=None):
    B, k1 = out_tokens.shape
    cap = gen_tokens.shape[1] if gen_tokens is not None else 0
    _call("qspec_spec_commit", B, k1 - 1, _chk(out_tokens, "out_tokens", _I64), _chk(seq_lens, "seq_lens", _I32),
          _chk(last_token, "last_token", _I64), _opt(gen_tokens, "gen_tokens", _I64),
          _opt(gen_lens, "gen_lens", _I32), cap, _stream())


def spec_snapshot(seq_lens, gen_lens, last_token, counters, rng_state, snap_i32, snap_i64, restore: bool = False):
    """The small per-cycle sequence state copied aside (or back): what a recovery replay of a cycle starts from."""
    B = seq_lens.numel()
    assert snap_i32.numel() >= 2 * B and snap_i64.numel() >= B + 5 and counters.numel() == 3 and rng_state.numel() == 2
    _call("qspec_spec_snapshot", B, 1 if restore else 0, _chk(seq_lens, "seq_lens", _I32), _chk(gen_lens, "gen_lens", _I32),
          _chk(last_token, "last_token", _I64), _chk(counters, "counters", _I64), _chk(rng_state, "rng_state", _I64),
          _chk(snap_i32, "snap_i32", _I32), _chk(snap_i64, "snap_i64", _I64), _stream())


def stream_error_words(device, extra=()):
    """Raw device addresses of the sticky error words of the CURRENT stream's hand-off workspaces (the ones the launches
    being enqueued on this stream use) plus `extra` addresses (the one-shot all-reduce's word)."""
    return [w.data_ptr() for w in error_words(device, current_stream_only=True)] + [int(p) for p in extra if p]


def collect_error_words(word_addrs, out=None, clear: bool = False):
    """out[0] (int64) = OR of the sticky error words at `word_addrs` (stream_error_words; at most four); clear: zero them."""
    assert len(word_addrs) <= 4, "at most four error words per call"
    w = list(word_addrs) + [None] * (4 - len(word_addrs))
    _call("qspec_collect_error_words", w[0], w[1], w[2], w[3], 1 if clear else 0, _opt(out, "out", _I64), _stream())


# ------------------------------------------------------------------ KV block operations (include/qspec_hip.h, "KV block operations")

def validate_block_pairs(pairs, num_src: int, num_dst: int, same_space: bool = True):
    """The (src, dst) block pairs of one copy / swap call as a list of int pairs, or ValueError -- a pure function, called
    before anything is enqueued.  src must lie in [0, num_src), dst in [0, num_dst), the dst values must be distinct, and
    with same_space (a copy inside one cache) no dst may also be a src of the call: the kernels rely on all of it."""
    out = []
    for p in pairs:
        if len(p) != 2:
            raise ValueError(f"block pair {p!r}: expected (src, dst)")
        s, d = int(p[0]), int(p[1])
        if not 0 <= s < num_src:
            raise ValueError(f"block pair ({s}, {d}): src outside 0..{num_src - 1}")
        if not 0 <= d < num_dst:
            raise ValueError(f"block pair ({s}, {d}): dst outside 0..{num_dst - 1}")
        out.append((s, d))
    dsts = [d for _, d in out]
    if len(set(dsts)) != len(dsts):
        raise ValueError("a dst block appears twice in one call")
    if same_space:
        both = set(dsts) & set(s for s, _ in out)
        if both:
            raise ValueError(f"blocks {sorted(both)[:8]} are src and dst of the same call")
    return out


class KVBlocks:
    """The cache tensors the block operations move blocks of: key_caches / value_caches, one [num_blocks, ...] tensor per layer,
    all of one shape and dtype (fp16 or the byte cache).  Holds the device array of their 2 * num_layers base pointers (K0, V0,
    K1, V1, ...: the plane order of a staging record), built ONCE here, and keeps the tensors alive."""

    def __init__(self, key_caches, value_caches):
        caches = [t for kv in zip(key_caches, value_caches) for t in kv]
        if not caches or len(key_caches) != len(value_caches):
            raise RuntimeError("key_caches and value_caches: one tensor per layer each")
        first = caches[0]
        for t in caches:
            _chk(t, "cache", (_F16,) + _KV8)
            if t.shape != first.shape or t.dtype != first.dtype or t.device != first.device or t.dim() < 2:
                raise RuntimeError("the cache tensors must share one [num_blocks, ...] shape, dtype and device")
        self.caches = caches
        self.num_layers, self.num_blocks = len(key_caches), int(first.shape[0])
        self.block_bytes = int(first[0].numel()) * first.element_size()
        if self.block_bytes % 16 or any(t.data_ptr() % 16 for t in caches):
            raise RuntimeError(f"blocks of {self.block_bytes} bytes: the block operations move 16-byte vectors")
        self.record_bytes = 2 * self.num_layers * self.block_bytes
        self.device = first.device
        self.layer_ptrs = torch.tensor([t.data_ptr() for t in caches], dtype=_I64).to(self.device)

    def _ids(self, ids):
        return torch.tensor(ids, dtype=_I64).to(self.device)


def copy_blocks(blocks: KVBlocks, pairs) -> None:
    """torch.ops._C_cache_ops.copy_blocks (csrc/cache_kernels.cu): cache[dst] = cache[src] in every layer's K and V for the
    (src, dst) pairs, ONE launch -- qspec_copy_blocks.  ValueError (out of range, a dst twice, a dst that is also a src) before
    anything is enqueued; no pairs: nothing is enqueued."""
    pairs = validate_block_pairs(pairs, blocks.num_blocks, blocks.num_blocks)
    if not pairs:
        return
    dev_pairs = blocks._ids(pairs)
    _call("qspec_copy_blocks", blocks.layer_ptrs.data_ptr(), blocks.num_layers, dev_pairs.data_ptr(), len(pairs),
          blocks.block_bytes, _stream())


def _staging_args(blocks: KVBlocks, block_ids, staging, distinct: bool):
    ids = [int(b) for b in block_ids]
    if any(not 0 <= b < blocks.num_blocks for b in ids):
        raise ValueError(f"block id outside 0..{blocks.num_blocks - 1}")
    if distinct and len(set(ids)) != len(ids):
        raise ValueError("a block appears twice in one scatter")
    if ids:
        _chk(staging, "staging", _U8)
        if staging.numel() < len(ids) * blocks.record_bytes or staging.data_ptr() % 16:
            raise RuntimeError(f"staging needs {len(ids)} records of {blocks.record_bytes} bytes, 16-byte aligned")
    return ids


def gather_blocks(blocks: KVBlocks, block_ids, staging) -> None:
    """The device half of a swap out: staging (uint8, [n, num_layers, 2, block_bytes]) record i = block block_ids[i] of every
    layer's K and V, ONE launch -- qspec_gather_blocks."""
    ids = _staging_args(blocks, block_ids, staging, distinct=False)
    if not ids:
        return
    dev_ids = blocks._ids(ids)
    _call("qspec_gather_blocks", blocks.layer_ptrs.data_ptr(), blocks.num_layers, dev_ids.data_ptr(), len(ids),
          blocks.block_bytes, staging.data_ptr(), _stream())


def scatter_blocks(blocks: KVBlocks, block_ids, staging) -> None:
    """The device half of a swap in: block block_ids[i] of every layer's K and V = staging record i (distinct ids), ONE launch
    -- qspec_scatter_blocks."""
    ids = _staging_args(blocks, block_ids, staging, distinct=True)
    if not ids:
        return
    dev_ids = blocks._ids(ids)
    _call("qspec_scatter_blocks", blocks.layer_ptrs.data_ptr(), blocks.num_layers, dev_ids.data_ptr(), len(ids),
          blocks.block_bytes, staging.data_ptr(), _stream())
