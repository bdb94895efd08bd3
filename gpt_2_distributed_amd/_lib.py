"""ctypes binding of libgpt2mi.so (the C ABI in include/gpt2mi.h).

This is the only route from Python to the GPU math. There is no fallback: if the library is
missing or the device is not a GPU, calls raise. Tensors are passed as raw device pointers;
launches go on torch's current HIP stream.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPT2MI_LIB: an alternative build of the same library (A/B kernel experiments, tools/kbench.py)
LIB_PATH = os.environ.get("GPT2MI_LIB") or os.path.join(_HERE, "libgpt2mi.so")

# the ABI these bindings are written against (include/gpt2mi.h GPT2MI_ABI_VERSION): a stale or foreign
# library is refused at load instead of being called with the wrong argument lists
ABI_VERSION = 24
# additions within that version (GPT2MI_ABI_MINOR): the bindings need at least this many
ABI_MINOR = 6

_c_int, _c_float, _c_size, _c_u64, _p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p

# name -> argtypes (all return int status unless listed in _RESTYPES)
_SIGS = {
    "gpt2mi_last_error": [],
    "gpt2mi_abi_version": [],
    "gpt2mi_abi_minor": [],
    "gpt2mi_embed_fwd": [_p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_embed_bwd": [_p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_layernorm_fwd": [_p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_float, _p],
    "gpt2mi_layernorm_bwd": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_float, _c_u64, _c_int, _p],
    "gpt2mi_colsum_bf16": [_p, _p, _c_int, _c_int, _c_int, _p],
    "gpt2mi_gemm": [_c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _p, _p, _p, _c_int,
                    _c_float, _p, _c_int, _c_int, _c_float, _c_u64, _p, _c_int, _p],
    "gpt2mi_attn_fwd": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_attn_bwd": [_p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_xent_fwd": [_p, _c_int, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gpt2mi_adamw": [_p, _p, _p, _p, _p, _c_size, _c_float, _c_float, _c_float, _c_float, _c_float, _c_int,
                     _c_float, _p, _p, _p],
    "gpt2mi_grad_norm": [_p, _c_size, _c_float, _p, _p, _p],
    "gpt2mi_norm_finalize": [_p, _c_int, _p, _p],
    "gpt2mi_norm_partials_size": [],
    "gpt2mi_sumsq_partials": [_p, _c_size, _c_float, _p, _p],
    "gpt2mi_clip_coef": [_p, _c_int, _c_float, _p, _p, _p, _p],
    "gpt2mi_adamw_clipped": [_p, _p, _p, _p, _p, _c_size, _c_float, _c_float, _c_float, _c_float, _c_float, _c_int,
                             _c_float, _p, _p, _p, _p],
    "gpt2mi_cast_f32_bf16": [_p, _p, _c_size, _p],
    "gpt2mi_transpose_bf16": [_p, _p, _c_int, _c_int, _c_int, _c_int, _p],
    "gpt2mi_transpose_bf16_batched": [_p, _p, _p, _c_int, ctypes.c_int64, _p],
    "gpt2mi_scale_mul": [_p, _p, _p, _p],
    "gpt2mi_memset_zero": [_p, _c_size, _p],
    "gpt2mi_zero_ranges": [_p, _p, _c_int, _p],
    "gpt2mi_gemm_f32": [_c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _p, _p, _p,
                        _c_int, _c_float, _p, _c_int, _c_int, _c_float, _c_u64, _p, _p],
    "gpt2mi_attn_fwd_f32": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_attn_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_layernorm_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_float, _c_u64, _c_int,
                                 _p],
    "gpt2mi_colsum_f32": [_p, _p, _c_int, _c_int, _c_int, _p],
    "gpt2mi_xent_fwd_f32": [_p, _c_int, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gpt2mi_cast_bf16_f32": [_p, _p, _c_size, _p],
    "gpt2mi_dlogits_accum": [_p, _c_int, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_int, _p],
    "gpt2mi_dlogits_accum_f32": [_p, _c_int, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_int, _p],
    "gpt2mi_branch_bwd": [_p, _p, _p, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_branch_bwd_f32": [_p, _p, _p, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_scale_f32": [_p, _c_size, _c_float, _p],
    "gpt2mi_fsdp_unpack": [_p, _c_int, _p, _p, _c_size, _p],
    "gpt2mi_fsdp_pack": [_p, _p, _c_int, _c_size, _c_size, _p],
    "gpt2mi_fsdp_accum": [_p, _c_int, _p, _c_size, _c_int, _p],
    "gpt2mi_gemm_wgrad": [_c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _c_int, _c_float, _p, _p,
                          _c_size, _c_int, _c_int, _p],
    "gpt2mi_gemm_wgrad_kt": [_c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _c_int, _c_float, _p, _p,
                             _c_size, _c_int, _c_int, _p],
    # count, M[], N[], K, A[], lda[], B[], ldb[], C[] (host arrays), accumulate, alpha, alpha_dev, ws, ws_floats, splits,
    # sched, stream
    "gpt2mi_gemm_wgrad_grouped": [_c_int, _p, _p, _c_int, _p, _p, _p, _p, _p, _c_int, _c_float, _p, _p, _c_size,
                                  _c_int, _c_int, _p],
    # v24.3: count, M[], N[], K, A[], lda[], B[], ldb[], C[], ldc[] (host arrays), accumulate, alpha, alpha_dev, table
    # (device scratch), table_bytes, sched, stream
    "gpt2mi_gemm_wgrad_batch": [_c_int, _p, _p, _c_int, _p, _p, _p, _p, _p, _p, _c_int, _c_float, _p, _p, _c_size,
                                _c_int, _p],
    "gpt2mi_gemm_wgrad_batch_scratch": [_c_int],
    "gpt2mi_gemm_wgrad_batch_max": [],
    # v14 decode: epilogue, M, N, K, A, lda, W, ldw, C, ldc, bias, resid, workspace, workspace_floats, stream
    "gpt2mi_gemm_skinny": [_c_int, _c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _p, _p, _p, _c_size, _p],
    "gpt2mi_gemm_skinny_workspace": [_c_int, _c_int, _c_int],
    "gpt2mi_kv_store": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p],
    "gpt2mi_attn_decode": [_p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _c_int, _p],
    "gpt2mi_attn_decode_workspace": [_c_int, _c_int, _c_int],
    "gpt2mi_embed_decode": [_p, _p, _p, _p, _c_int, _c_int, _c_int, _p],
    "gpt2mi_decode_step": [_p, _p, _c_int, _p],
    # v17 sampling: logits, ldl, B, V, temperature, top_k, top_p, seed, pos, eos, done, tok_out, seq_out, ld_seq,
    # probs_out, stream
    "gpt2mi_sample": [_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_u64, _c_int, ctypes.c_int64, _p, _p,
                      _p, _c_int, _p, _p],
    # plan, V, temperature, top_k, top_p, seed, eos, pos0, n, tok, seq, ld_seq, done, stream
    "gpt2mi_decode_generate": [_p, _c_int, _c_float, _c_int, _c_float, _c_u64, ctypes.c_int64, _c_int, _c_int, _p, _p,
                               _c_int, _p, _p],
    # v18 evaluation: x, ldx, w, ldw, w_rows, labels, M, V, K, ignore_index, loss_rows, lse, loss_sum, count, accumulate,
    # loss_mean, workspace, stream
    "gpt2mi_lm_loss": [_p, _c_int, _p, _c_int, _c_int, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _c_int, _p,
                       _p, _p],
    "gpt2mi_lm_loss_workspace": [_c_int, _c_int],
    # v19 ragged decode: the scalar entries' lists with pos -> const int* pos (HOST array of B ints) and, for the sampler
    # and the loop, const uint32_t* row_id (HOST array, may be NULL) after it. v20: these are the implementation, the
    # scalar entries above forward to them (and take B <= DECODE_MAX_B like them)
    "gpt2mi_attn_decode_ragged": [_p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _p, _p],
    "gpt2mi_embed_decode_ragged": [_p, _p, _p, _p, _c_int, _c_int, _p, _p],
    "gpt2mi_sample_ragged": [_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_u64, _p, _p, ctypes.c_int64, _p,
                             _p, _p, _c_int, _p, _p],
    "gpt2mi_decode_step_ragged": [_p, _p, _p, _p],
    "gpt2mi_decode_generate_ragged": [_p, _c_int, _c_float, _c_int, _c_float, _c_u64, ctypes.c_int64, _p, _p, _c_int,
                                      _p, _p, _c_int, _p, _p],
    # v21 extend: qkv, kcache, vcache, out, workspace, workspace_floats, R, B, H, head_dim, Tcap, seq, pos (HOST arrays
    # of R ints), stream; plan, R, tok, seq, pos, stream
    "gpt2mi_attn_extend": [_p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gpt2mi_decode_extend": [_p, _c_int, _p, _p, _p, _p],
    # v22 penalties: gpt2mi_sample_ragged's list with (const gpt2mi_penalties* pen, logits_out) before the stream;
    # gpt2mi_decode_generate_ragged's list, then repetition, presence, frequency, gen_start (HOST array, may be NULL)
    "gpt2mi_sample_penalized": [_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_u64, _p, _p, ctypes.c_int64,
                                _p, _p, _p, _c_int, _p, _p, _p, _p],
    "gpt2mi_decode_generate_penalized": [_p, _c_int, _c_float, _c_int, _c_float, _c_u64, ctypes.c_int64, _p, _p, _c_int,
                                         _p, _p, _c_int, _p, _p, _c_float, _c_float, _c_float, _p],
    # v23 fp8 cache: the bf16 siblings' lists with (kscale, vscale) behind (kcache, vcache)
    "gpt2mi_kv_store_fp8": [_p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p],
    "gpt2mi_attn_decode_fp8_ragged": [_p, _p, _p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _p, _p],
    "gpt2mi_attn_extend_fp8": [_p, _p, _p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p,
                               _p],
    # v24 shared prompt cache: attn_decode_ragged's / attn_decode_fp8_ragged's lists with (share_group, share_len), HOST
    # arrays of B ints (both may be NULL), behind pos
    "gpt2mi_attn_decode_shared": [_p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p],
    "gpt2mi_attn_decode_shared_fp8": [_p, _p, _p, _p, _p, _p, _p, _c_size, _c_int, _c_int, _c_int, _c_int, _p, _p, _p,
                                      _p],
    # v24.1 log-probabilities: gpt2mi_sample_penalized's list with (const gpt2mi_logprobs* lp) before the stream;
    # gpt2mi_decode_generate_penalized's list with it at the end
    "gpt2mi_sample_logprobs": [_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_u64, _p, _p, ctypes.c_int64,
                               _p, _p, _p, _c_int, _p, _p, _p, _p, _p],
    "gpt2mi_decode_generate_logprobs": [_p, _c_int, _c_float, _c_int, _c_float, _c_u64, ctypes.c_int64, _p, _p, _c_int,
                                        _p, _p, _c_int, _p, _p, _c_float, _c_float, _c_float, _p, _p],
    # v24.2 beam search: top_id, top_logprob, cum, done, G, W, eos, tok_out, parent_out, cum_out, done_out, stream
    "gpt2mi_beam_select": [_p, _p, _p, _p, _c_int, _c_int, ctypes.c_int64, _p, _p, _p, _p, _p],
    # kv_format, L, H, R, window
    "gpt2mi_beam_reorder_workspace": [_c_int, _c_int, _c_int, _c_int, _c_int],
    # kcache, vcache, kscale, vscale, kv_format, L, layer_rows, B, H, Tcap, seq, ld_seq, parent (device), G, W, lo, hi (HOST
    # arrays of G W ints), workspace, workspace_bytes, stream
    "gpt2mi_beam_reorder": [_p, _p, _p, _p, _c_int, _c_int, _c_size, _c_int, _c_int, _c_int, _p, _c_int, _p, _c_int, _c_int,
                            _p, _p, _p, _c_size, _p],
    # plan, V, W, eos, pos0, lo (HOST arrays), n, tok, seq, ld_seq, cum, done, parents, workspace, workspace_bytes, stream
    "gpt2mi_decode_beam_search": [_p, _c_int, _c_int, ctypes.c_int64, _p, _p, _c_int, _p, _p, _c_int, _p, _p, _p, _p,
                                  _c_size, _p],
    # v24.4 constraints: gpt2mi_sample_logprobs' list with (const gpt2mi_constraints* con) before the stream;
    # gpt2mi_decode_generate_logprobs' list with it at the end
    "gpt2mi_sample_constrained": [_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_u64, _p, _p, ctypes.c_int64,
                                  _p, _p, _p, _c_int, _p, _p, _p, _p, _p, _p],
    "gpt2mi_decode_generate_constrained": [_p, _c_int, _c_float, _c_int, _c_float, _c_u64, ctypes.c_int64, _p, _p, _c_int,
                                           _p, _p, _c_int, _p, _p, _c_float, _c_float, _c_float, _p, _p, _p],
    # v24.5 document masking: idx, B, T, T_valid, eot, eot_begin, start, end, stream; the attention lists with doc_start
    # (forward) or (doc_start, doc_end) (backward) before B
    "gpt2mi_doc_bounds": [_p, _c_int, _c_int, _c_int, ctypes.c_int64, _c_int, _p, _p, _p],
    "gpt2mi_attn_fwd_doc": [_p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_attn_bwd_doc": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_attn_fwd_f32_doc": [_p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_attn_bwd_f32_doc": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64,
                                _p],
    # v24.6 positions per document: the embedding lists with doc_start before B
    "gpt2mi_embed_fwd_doc": [_p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
    "gpt2mi_embed_bwd_doc": [_p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_u64, _p],
}
# the entries a library of minor m lacks: what came with a minor above m
_SINCE_MINOR = {"gpt2mi_abi_minor": 1, "gpt2mi_sample_logprobs": 1, "gpt2mi_decode_generate_logprobs": 1,
                "gpt2mi_beam_select": 2, "gpt2mi_beam_reorder_workspace": 2, "gpt2mi_beam_reorder": 2,
                "gpt2mi_decode_beam_search": 2, "gpt2mi_gemm_wgrad_batch": 3, "gpt2mi_gemm_wgrad_batch_scratch": 3,
                "gpt2mi_gemm_wgrad_batch_max": 3, "gpt2mi_sample_constrained": 4,
                "gpt2mi_decode_generate_constrained": 4, "gpt2mi_doc_bounds": 5, "gpt2mi_attn_fwd_doc": 5,
                "gpt2mi_attn_bwd_doc": 5, "gpt2mi_attn_fwd_f32_doc": 5, "gpt2mi_attn_bwd_f32_doc": 5,
                "gpt2mi_embed_fwd_doc": 6, "gpt2mi_embed_bwd_doc": 6}
_RESTYPES = {"gpt2mi_last_error": ctypes.c_char_p, "gpt2mi_gemm_skinny_workspace": _c_size,
             "gpt2mi_attn_decode_workspace": _c_size, "gpt2mi_lm_loss_workspace": _c_size,
             "gpt2mi_beam_reorder_workspace": _c_size, "gpt2mi_gemm_wgrad_batch_scratch": _c_size}

EXPORTED = tuple(_SIGS)

_lib: Optional[ctypes.CDLL] = None


class KernelError(RuntimeError):
    pass


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load (once) and type the library. Raises if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise KernelError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                          " (or make -C gpt_2_distributed_amd/csrc)")
    _lib = open_library(path)
    return _lib


def open_library(path: str, min_minor: int = ABI_MINOR) -> ctypes.CDLL:
    """A build of the library at ``path``, typed and refused unless its C ABI is the bindings': the version equal, the
    minor at least ``min_minor`` (a library from before the minor number existed has minor 0). An A/B tool that loads
    an older build of the same version passes the minor it can do with; the entries that build lacks stay untyped."""
    lib = ctypes.CDLL(path)
    minor = lib.gpt2mi_abi_minor() if hasattr(lib, "gpt2mi_abi_minor") else 0
    if lib.gpt2mi_abi_version() != ABI_VERSION or minor < min_minor:
        raise KernelError(f"{path} has C ABI v{lib.gpt2mi_abi_version()}.{minor}, the bindings expect v{ABI_VERSION}."
                          f"{min_minor} or a later minor: rebuild it")
    for name, args in _SIGS.items():
        if _SINCE_MINOR.get(name, 0) > minor:
            continue
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    return lib


@contextlib.contextmanager
def using(lib: ctypes.CDLL):
    """Within the block every binding calls ``lib`` (from ``open_library``) instead of the product library: how an A/B
    tool runs the package's own call paths over another build in one process."""
    global _lib
    product = load()
    _lib = lib
    try:
        yield lib
    finally:
        _lib = product


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise KernelError("gpt2mi kernels take device tensors only (got a CPU tensor)")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t: Optional[torch.Tensor]) -> bool:
    """Activation dtype selects the kernel family: fp32 tensors -> the fp32 (no-autocast) kernels."""
    if t is None:
        return False
    if t.dtype == torch.float32:
        return True
    if t.dtype != torch.bfloat16:
        raise KernelError(f"gpt2mi kernels take bf16 or fp32 activations (got {t.dtype})")
    return False


def _call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.gpt2mi_last_error().decode(errors="replace")
        raise KernelError(f"{name} failed ({rc}): {msg}")


# ---- typed wrappers ------------------------------------------------------------------------------
EPI_BF16, EPI_F32, EPI_RESID, EPI_GELU, EPI_GELU_BWD, EPI_ATOMIC = range(6)
FWD, DGRAD, WGRAD = 0, 1, 2
# GEMM schedule per call (gpt2mi.h GPT2MI_SCHED_*): auto, or the flag that keeps the persistent schedule off while
# RCCL kernels may share the CUs; the low byte picks a kernel for A/B experiments and kernel-equivalence tests
SCHED_AUTO, SCHED_NO_PERSISTENT = 0, 0x100
# other kernels (RCCL) may hold CUs: persistent GEMMs take tiles from work queues (gpt2mi.h GPT2MI_SCHED_SHARED_CUS)
SCHED_SHARED_CUS = 0x400
# gemm_wgrad / gemm_wgrad_kt: split-K partial sums rounded to bf16 slabs (gpt2mi.h GPT2MI_SCHED_BF16_SLABS)
SCHED_BF16_SLABS = 0x200


def embed_fwd(idx, wte, wpe, x, B, T, C, p=0.0, seed=0, T_valid=None):
    _call("gpt2mi_embed_fwd", _ptr(idx), _ptr(wte), _ptr(wpe), _ptr(x), B, T, T if T_valid is None else T_valid, C, p,
          seed, _stream())


def embed_bwd(idx, dres, dwte, dwpe, B, T, C, p=0.0, seed=0, T_valid=None):
    _call("gpt2mi_embed_bwd", _ptr(idx), _ptr(dres), _ptr(dwte), _ptr(dwpe), B, T, T if T_valid is None else T_valid,
          C, p, seed, _stream())


def _doc_start(name, start, B, T):
    if start.dtype != torch.int32 or tuple(start.shape) != (B, T) or not start.is_contiguous():
        raise KernelError(f"{name}: start must be a contiguous int32 [B={B}, T={T}] tensor")
    return _ptr(start)


def embed_fwd_doc(idx, wte, wpe, x, start, B, T, C, p=0.0, seed=0, T_valid=None):
    """embed_fwd with the position of (b, t) restarting at its document: wpe[t - start[b, t]] (packing.doc_positions)."""
    _call("gpt2mi_embed_fwd_doc", _ptr(idx), _ptr(wte), _ptr(wpe), _ptr(x), _doc_start("embed_fwd_doc", start, B, T),
          B, T, T if T_valid is None else T_valid, C, p, seed, _stream())


def embed_bwd_doc(idx, dres, dwte, dwpe, start, B, T, C, p=0.0, seed=0, T_valid=None):
    _call("gpt2mi_embed_bwd_doc", _ptr(idx), _ptr(dres), _ptr(dwte), _ptr(dwpe),
          _doc_start("embed_bwd_doc", start, B, T), B, T, T if T_valid is None else T_valid, C, p, seed, _stream())


def layernorm_fwd(x, w, b, y_bf16, y_f32, mean, rstd, M, C, eps):
    if y_bf16 is not None and _f32(y_bf16):  # fp32 mode: the GEMM-operand output is fp32
        y_bf16, y_f32 = None, y_bf16
    _call("gpt2mi_layernorm_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y_bf16), _ptr(y_f32), _ptr(mean), _ptr(rstd),
          M, C, eps, _stream())


def layernorm_bwd(x, w, mean, rstd, dy, dres, dw, db, out_bf16, dbias_out, M, C, p_out=0.0, seed_out=0,
                  dres_init=False):
    name = "gpt2mi_layernorm_bwd_f32" if _f32(dy) else "gpt2mi_layernorm_bwd"
    _call(name, _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dy), _ptr(dres), _ptr(dw),
          _ptr(db), _ptr(out_bf16), _ptr(dbias_out), M, C, p_out, seed_out, int(dres_init), _stream())


def colsum_bf16(g, db, M, N, ld):
    _call("gpt2mi_colsum_f32" if _f32(g) else "gpt2mi_colsum_bf16", _ptr(g), _ptr(db), M, N, ld, _stream())


def gemm(layout, epilogue, M, N, K, A, lda, B, ldb, C, ldc, bias=None, resid=None, aux=None, ldaux=0,
         alpha=1.0, alpha_dev=None, accumulate=False, splits=1, p_drop=0.0, seed=0, dbias=None, sched=SCHED_AUTO):
    args = (layout, epilogue, M, N, K, _ptr(A), lda, _ptr(B), ldb, _ptr(C), ldc, _ptr(bias), _ptr(resid), _ptr(aux),
            ldaux, alpha, _ptr(alpha_dev), int(accumulate), splits, p_drop, seed, _ptr(dbias))
    if _f32(A):  # the fp32 kernels have one schedule
        _call("gpt2mi_gemm_f32", *args, _stream())
    else:
        _call("gpt2mi_gemm", *args, int(sched), _stream())


def gemm_wgrad(M, N, K, A, lda, B, ldb, C, ldc, accumulate=True, alpha=1.0, alpha_dev=None, workspace=None,
               splits=1, sched=SCHED_AUTO):
    ws_n = workspace.numel() if workspace is not None else 0
    _call("gpt2mi_gemm_wgrad", M, N, K, _ptr(A), lda, _ptr(B), ldb, _ptr(C), ldc, int(accumulate), alpha,
          _ptr(alpha_dev), _ptr(workspace), ws_n, splits, int(sched), _stream())


def gemm_wgrad_kt(M, N, K, A, lda, Bt, ldbt, C, ldc, accumulate=True, alpha=1.0, alpha_dev=None, workspace=None,
                  splits=1, sched=SCHED_AUTO):
    """gemm_wgrad with B given transposed (Bt [N][K], k-contiguous): the same C[M][N] (+)= alpha A^T B, same bits."""
    ws_n = workspace.numel() if workspace is not None else 0
    _call("gpt2mi_gemm_wgrad_kt", M, N, K, _ptr(A), lda, _ptr(Bt), ldbt, _ptr(C), ldc, int(accumulate), alpha,
          _ptr(alpha_dev), _ptr(workspace), ws_n, splits, int(sched), _stream())


def gemm_wgrad_grouped(problems, K, accumulate=True, alpha=1.0, alpha_dev=None, workspace=None, splits=1,
                       sched=SCHED_AUTO):
    """Up to 4 weight gradients over the same K tokens in one launch (+ one reduction): problems = [(M, N, A, lda, B,
    ldb, C)], each C[M][N] (+)= alpha A^T B as gemm_wgrad with the same splits and fp32 slabs would form it."""
    n = len(problems)
    ints = lambda vals: (_c_int * n)(*vals)  # noqa: E731
    ptrs = lambda vals: (_p * n)(*vals)  # noqa: E731
    ws_n = workspace.numel() if workspace is not None else 0
    _call("gpt2mi_gemm_wgrad_grouped", n, ints([q[0] for q in problems]), ints([q[1] for q in problems]), K,
          ptrs([_ptr(q[2]) for q in problems]), ints([q[3] for q in problems]), ptrs([_ptr(q[4]) for q in problems]),
          ints([q[5] for q in problems]), ptrs([_ptr(q[6]) for q in problems]), int(accumulate), alpha,
          _ptr(alpha_dev), _ptr(workspace), ws_n, splits, int(sched), _stream())


def wgrad_group_splits(shapes, K, cus=256):
    """Split-K factor of a grouped weight-gradient launch over output shapes [(M, N)] (256-multiples): the
    wgrad_splits cost model on the summed tile count, so that the last round of blocks is not mostly idle (a GPT2Block
    of GPT-2 124M: 108 tiles x 7 splits = 756 blocks, 2.95 rounds of 256)."""
    tiles = sum((m // 256) * (n // 256) for m, n in shapes)
    elems = sum(m * n for m, n in shapes)
    best, best_cost = 1, None
    for s in range(1, 33):
        if K // s < 256:
            break
        rounds = -(-tiles * s // cus)
        cost = rounds * (K / s) * 22e-9 + (s * elems * 8 / 5e12 if s > 1 else 0.0)
        if best_cost is None or cost < best_cost * 0.99:
            best, best_cost = s, cost
    return best


GROUP_MAX = 4  # problems of one gemm_wgrad_grouped launch (gemm_plan.h kGroupMax)


def gemm_wgrad_batch_max() -> int:
    return load().gpt2mi_gemm_wgrad_batch_max()


def gemm_wgrad_batch_scratch(count: int) -> int:
    """Bytes of device scratch the problem table of a gemm_wgrad_batch launch of ``count`` problems takes."""
    return load().gpt2mi_gemm_wgrad_batch_scratch(count)


def gemm_wgrad_batch(problems, K, accumulate=True, alpha=1.0, alpha_dev=None, table=None, sched=SCHED_AUTO):
    """Any number of weight gradients (up to gemm_wgrad_batch_max()) over the same K tokens in ONE launch without
    split-K: problems = [(M, N, A, lda, B, ldb, C[, ldc])], each C[M][N] (+)= alpha A^T B with the bits of
    gemm_wgrad(splits=1). table: a device byte tensor of gemm_wgrad_batch_scratch(len(problems)) bytes, which receives
    the problem table stream-ordered ahead of the launch."""
    n = len(problems)
    ints = lambda vals: (_c_int * n)(*vals)  # noqa: E731
    ptrs = lambda vals: (_p * n)(*vals)  # noqa: E731
    tb = table.numel() * table.element_size() if table is not None else 0
    _call("gpt2mi_gemm_wgrad_batch", n, ints([q[0] for q in problems]), ints([q[1] for q in problems]), K,
          ptrs([_ptr(q[2]) for q in problems]), ints([q[3] for q in problems]), ptrs([_ptr(q[4]) for q in problems]),
          ints([q[5] for q in problems]), ptrs([_ptr(q[6]) for q in problems]),
          ints([q[7] if len(q) > 7 else q[1] for q in problems]), int(accumulate), alpha, _ptr(alpha_dev), _ptr(table),
          tb, int(sched), _stream())


def wgrad_batch_plan(shapes, K, cus=256):
    """How the weight gradients of output shapes [(M, N)] (256-multiples) over the same K tokens run as one deferred
    family: (body, tail, tail_split), index lists into ``shapes``. The body's whole problems go into one
    gemm_wgrad_batch launch, one unsplit tile per block, and fill whole rounds of ``cus`` blocks as nearly as whole
    problems allow: the tail is the set of problems with the fewest tiles that still covers the tiles past the last
    whole round (fewest problems, then the first listed, among equals); everything when there is no whole round. The
    tail runs split-K through gemm_wgrad_grouped at the wgrad_group_splits cost model's factor for it (its rounds of
    ``cus`` blocks x K per split + the slab term; no split below 256 tokens). GPT-2 124M, 12 blocks: 1 296 tiles = a
    body of 1 278 (4.99 rounds of 256) and two proj problems (18 tiles x 14 splits = 252 blocks, one round)."""
    tiles = [(m // 256) * (n // 256) for m, n in shapes]
    total = sum(tiles)
    need = total if total < cus else total % cus
    tail = []
    if need == total:
        tail = list(range(len(shapes)))
    elif need > 0:
        # subset sums up to need + the largest problem: best[s] = the index tuple reaching s (fewest, then first)
        cap = need + max(tiles)
        best = {0: ()}
        for i, t in enumerate(tiles):
            for s, idx in sorted(best.items(), reverse=True):
                if s + t <= cap:
                    cand = idx + (i,)
                    old = best.get(s + t)
                    if old is None or (len(cand), cand) < (len(old), old):
                        best[s + t] = cand
        tail = list(best[min(s for s in best if s >= need)])
    chosen = set(tail)
    body = [i for i in range(len(shapes)) if i not in chosen]
    split = wgrad_group_splits([shapes[i] for i in tail], K, cus) if tail else 1
    return body, tail, split


def gemm_wgrad_planned(problems, K, plan, accumulate=True, alpha=1.0, alpha_dev=None, table=None, workspace=None,
                       sched=SCHED_AUTO):
    """The launches of a wgrad_batch_plan over problems = [(M, N, A, lda, B, ldb, C)] (dense C): the body as one
    gemm_wgrad_batch launch, the tail as gemm_wgrad_grouped launches of at most GROUP_MAX problems at the plan's
    split (workspace: split x the largest such group's outputs, in floats)."""
    body, tail, split = plan
    if body:
        gemm_wgrad_batch([problems[i] for i in body], K, accumulate=accumulate, alpha=alpha, alpha_dev=alpha_dev,
                         table=table, sched=sched)
    for j in range(0, len(tail), GROUP_MAX):
        gemm_wgrad_grouped([problems[i] for i in tail[j:j + GROUP_MAX]], K, accumulate=accumulate, alpha=alpha,
                           alpha_dev=alpha_dev, workspace=workspace, splits=split, sched=sched)


def wgrad_splits(M, N, K, cus=256):
    """Split-K factor for a wgrad output of M x N (K tokens) on 256x256 tiles (one block per CU).

    Minimises (rounds of `cus` blocks) x (K per split) + the slab reduction, so the last round of
    blocks is not mostly idle: the tied lm_head wgrad (197 x 3 = 591 tiles = 2.3 rounds) runs as 3
    splits (1773 blocks = 6.9 rounds of 1/3 the depth); the small block wgrads fill one round.
    Each split keeps >= 4 K-tiles of 64."""
    tiles = -(-M // 256) * -(-N // 256)  # (a partial last tile counts as a tile)
    if tiles == 0:
        return 1
    best, best_cost = 1, None
    for s in range(1, 33):
        if K // s < 256:
            break
        rounds = -(-tiles * s // cus)
        # GEMM time ~ rounds * K/s * 22 ns per token-row of a 256x256 tile; reduce ~ s*M*N*8 B at 5 TB/s
        cost = rounds * (K / s) * 22e-9 + (s * M * N * 8 / 5e12 if s > 1 else 0.0)
        if best_cost is None or cost < best_cost * 0.99:
            best, best_cost = s, cost
    return best


def _doc_ptrs(doc, B, T):
    """(start, end) pointers of a packing.DocBounds for the _doc attention entries, its tensors checked against [B, T]
    (metadata only: no host synchronisation). A None member stays None: the C entry's NULL refusal."""
    start, end = doc
    for name, t in (("start", start), ("end", end)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B, T) or not t.is_contiguous()):
            raise KernelError(f"doc bounds: {name} must be a contiguous int32 [B={B}, T={T}] tensor "
                              f"(got {t.dtype} {tuple(t.shape)})")
    return _ptr(start), _ptr(end)


def doc_bounds(idx, eot, eot_begin, start, end, T_valid=None):
    """gpt2mi_doc_bounds (packing.doc_bounds_reference is the rule): the document [start, end) of every position of idx
    int64 [B, T] into the int32 [B, T] tensors start / end; eot_begin False: eot closes a document, True: it opens one."""
    B, T = idx.shape
    if idx.dtype != torch.int64 or not idx.is_contiguous():
        raise KernelError("doc_bounds: idx must be a contiguous int64 [B, T] tensor")
    s, e = _doc_ptrs((start, end), B, T)
    _call("gpt2mi_doc_bounds", _ptr(idx), B, T, T if T_valid is None else T_valid, int(eot), int(bool(eot_begin)), s, e,
          _stream())


def attn_fwd(qkv, out, lse, B, T, H, D, p_drop=0.0, seed=0, doc=None):
    """doc: a packing.DocBounds (int32 [B, T] start, end) -> the document-masked entry; None: the call as it was."""
    f32 = _f32(qkv)
    if doc is None:
        _call("gpt2mi_attn_fwd_f32" if f32 else "gpt2mi_attn_fwd", _ptr(qkv), _ptr(out), _ptr(lse), B, T, H, D, p_drop, seed, _stream())
        return
    start, _ = _doc_ptrs(doc, B, T)
    _call("gpt2mi_attn_fwd_f32_doc" if f32 else "gpt2mi_attn_fwd_doc", _ptr(qkv), _ptr(out), _ptr(lse), start, B, T, H,
          D, p_drop, seed, _stream())


def attn_bwd(qkv, out, dout, lse, delta, dqkv, B, T, H, D, p_drop=0.0, seed=0, colsum=None, doc=None):
    """colsum: optional fp32 [B*T/32, 3C] partial column sums of dqkv (bf16 path; sum rows with colsum_bf16).
    doc: as attn_fwd."""
    f32 = _f32(qkv)
    if doc is None:
        _call("gpt2mi_attn_bwd_f32" if f32 else "gpt2mi_attn_bwd", _ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse),
              _ptr(delta), _ptr(dqkv), _ptr(colsum), B, T, H, D, p_drop, seed, _stream())
        return
    start, end = _doc_ptrs(doc, B, T)
    _call("gpt2mi_attn_bwd_f32_doc" if f32 else "gpt2mi_attn_bwd_doc", _ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse),
          _ptr(delta), _ptr(dqkv), _ptr(colsum), start, end, B, T, H, D, p_drop, seed, _stream())


def xent_fwd(logits, ld, labels, loss_rows, lse, dlogits, ldd, M, V, loss, inv_count, ignore_index=-100):
    _call("gpt2mi_xent_fwd_f32" if _f32(logits) else "gpt2mi_xent_fwd", _ptr(logits), ld, _ptr(labels), _ptr(loss_rows), _ptr(lse), _ptr(dlogits), ldd, M, V,
          ignore_index, _ptr(loss), _ptr(inv_count), _stream())


def adamw(p, g, m, v, p_bf16, n, lr, wd, b1, b2, eps, step, grad_scale, partials, grad_norm):
    _call("gpt2mi_adamw", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), n, lr, wd, b1, b2, eps, step,
          grad_scale, _ptr(partials), _ptr(grad_norm), _stream())


def grad_norm(g, n, scale, partials, out):
    _call("gpt2mi_grad_norm", _ptr(g), n, scale, _ptr(partials), _ptr(out), _stream())


def norm_finalize(partials, n, out):
    """out[0] = sqrt(sum(partials[:n])) (the norm of adamw launches given grad_norm=None)."""
    _call("gpt2mi_norm_finalize", _ptr(partials), n, _ptr(out), _stream())


def sumsq_partials(g, n, scale, partials):
    """norm_partials_size() partial sums of (g*scale)^2 over g[:n] (no finalisation; slices of one buffer)."""
    _call("gpt2mi_sumsq_partials", _ptr(g), n, scale, _ptr(partials), _stream())


def clip_coef(partials, n, max_norm, sumsq_out, norm_out, coef_out):
    """norm_out[0] = sqrt(sum(partials[:n])), coef_out[0] = min(1, max_norm / (norm + 1e-6)), sumsq_out[0] (or None) =
    the sum: clip_grad_norm_'s coefficient, left on the device."""
    _call("gpt2mi_clip_coef", _ptr(partials), n, max_norm, _ptr(sumsq_out), _ptr(norm_out), _ptr(coef_out), _stream())


def adamw_clipped(p, g, m, v, p_bf16, n, lr, wd, b1, b2, eps, step, grad_scale, coef_dev, partials=None,
                  grad_norm=None):
    _call("gpt2mi_adamw_clipped", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), n, lr, wd, b1, b2, eps, step,
          grad_scale, _ptr(coef_dev), _ptr(partials), _ptr(grad_norm), _stream())


def norm_partials_size() -> int:
    return load().gpt2mi_norm_partials_size()


def cast_f32_bf16(x, y, n):
    _call("gpt2mi_cast_f32_bf16", _ptr(x), _ptr(y), n, _stream())


def cast_bf16_f32(x, y, n):
    _call("gpt2mi_cast_bf16_f32", _ptr(x), _ptr(y), n, _stream())


def dlogits_accum(dl, ldd, g, ldg, B, Tp, Tv, V, alpha_dev=None, init=False):
    """dl (the lm_head backward's dlogits) = alpha*dl + g over the [B, Tv, V] logits the caller saw."""
    name = "gpt2mi_dlogits_accum_f32" if _f32(dl) else "gpt2mi_dlogits_accum"
    if g.dtype != dl.dtype:
        raise KernelError(f"dlogits_accum: grad dtype {g.dtype} != dlogits dtype {dl.dtype}")
    _call(name, _ptr(dl), ldd, _ptr(g), ldg, B, Tp, Tv, V, _ptr(alpha_dev), int(init), _stream())


def branch_bwd(dres, out, dbias, M, C, p=0.0, seed=0):
    _call("gpt2mi_branch_bwd_f32" if _f32(out) else "gpt2mi_branch_bwd", _ptr(dres), _ptr(out), _ptr(dbias), M, C, p,
          seed, _stream())


def scale_(x: torch.Tensor, s: float):
    _call("gpt2mi_scale_f32", _ptr(x), x.numel(), s, _stream())


def fsdp_unpack(src, dst_f32, dst_bf16, n):
    _call("gpt2mi_fsdp_unpack", _ptr(src), int(src.dtype == torch.float32), _ptr(dst_f32), _ptr(dst_bf16), n,
          _stream())


def fsdp_pack(src, dst, n, n_pad):
    _call("gpt2mi_fsdp_pack", _ptr(src), _ptr(dst), int(dst.dtype == torch.float32), n, n_pad, _stream())


def fsdp_accum(src, dst, n, accumulate=True):
    _call("gpt2mi_fsdp_accum", _ptr(src), int(src.dtype == torch.float32), _ptr(dst), n, int(accumulate), _stream())


def transpose_bf16(src, dst, R, C, ld_src=None, ld_dst=None):
    _call("gpt2mi_transpose_bf16", _ptr(src), _ptr(dst), R, C, ld_src or C, ld_dst or R, _stream())


def transpose_bf16_batched(src, dst, desc, n, total_tiles):
    """desc: device int64 [n, 4] = (element offset, R, C, first tile) per matrix (see include/gpt2mi.h)."""
    _call("gpt2mi_transpose_bf16_batched", _ptr(src), _ptr(dst), _ptr(desc), n, total_tiles, _stream())


def scale_mul(a, b, out):
    _call("gpt2mi_scale_mul", _ptr(a), _ptr(b), _ptr(out), _stream())


def zero_(t: torch.Tensor):
    _call("gpt2mi_memset_zero", _ptr(t), t.numel() * t.element_size(), _stream())


def zero_ranges(t: torch.Tensor, ranges: torch.Tensor):
    """Zero the element ranges of fp32 t given as a cuda int64 [n, 2] tensor of (offset, count)."""
    assert t.dtype == torch.float32 and ranges.dtype == torch.int64 and ranges.is_cuda
    _call("gpt2mi_zero_ranges", _ptr(t), _ptr(ranges), ranges.shape[0], _stream())


# ---- v14: autoregressive decode (csrc/decode.hip) -------------------------------------------------
class DecodeLayer(ctypes.Structure):
    """gpt2mi_decode_layer (include/gpt2mi.h)."""
    _fields_ = [(n, _p) for n in ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "qkv_w", "proj_w", "fc1_w", "fc2_w",
                                  "qkv_b", "proj_b", "fc1_b", "fc2_b", "kcache", "vcache", "kscale", "vscale")]


class DecodePlan(ctypes.Structure):
    """gpt2mi_decode_plan (include/gpt2mi.h). `layers` points at a host array the owner keeps alive."""
    _fields_ = ([(n, _c_int) for n in ("B", "C", "H", "L", "Vp", "Tcap")] + [("eps", _c_float)] +
                [(n, _p) for n in ("wte", "wpe", "lnf_w", "lnf_b", "wte_bf16")] +
                [("layers", ctypes.POINTER(DecodeLayer))] +
                [(n, _p) for n in ("x", "xmid", "ln", "qkv", "ao", "h", "mean", "rstd")] +
                [("attn_ws", _p), ("attn_ws_floats", _c_size), ("gemm_ws", _p), ("gemm_ws_floats", _c_size),
                 ("logits", _p), ("rows", _c_int)])

    # v23 appends `int kv_format` behind `rows`. An int behind a pointer-aligned struct's last int lands in what was the
    # struct's tail padding: no offset moved and sizeof did not change. The field list above stays the one of v21
    # (tests/test_extend_cpu.py pins its last two names), so the new field is a property over those four bytes, which
    # ctypes allocates and zeroes with the rest of the structure: a plan that never sets it means bf16.
    @property
    def kv_format(self) -> int:
        return _c_int.from_address(ctypes.addressof(self) + self.KV_FORMAT_OFFSET).value

    @kv_format.setter
    def kv_format(self, value: int) -> None:
        _c_int.from_address(ctypes.addressof(self) + self.KV_FORMAT_OFFSET).value = value


    # v24 appends `const int* share_group, *share_len` behind kv_format: the C struct grows by two pointers. The field
    # list still stays v21's, so an instance is laid over a zeroed buffer of the C struct's size (``__new__``) and the
    # two pointers are properties over its tail, like kv_format: a plan that never sets them shares nothing.
    #
    # THE TRAP: ctypes.sizeof(DecodePlan) is therefore 16 bytes SHORT of sizeof(gpt2mi_decode_plan) (PLAN_BYTES), and
    # only ``DecodePlan()`` makes an object the library may read. An element of ``(DecodePlan * n)()``, a
    # ``from_buffer_copy`` or a ``from_address`` has no tail, and the C side would read past its end; a memmove of sizeof
    # bytes leaves the tail behind. Every binding below passes a plan through ``ref()``, which refuses an object that
    # ``DecodePlan()`` did not make (tests/test_share_cabi.py). The way out of this, when
    # the pin on the field list may move, is to put kv_format, share_group and share_len into ``_fields_`` and delete
    # ``__new__``, the properties and ``ref()``'s check.
    def __new__(cls, *args, **kw):
        buf = (ctypes.c_char * cls.PLAN_BYTES)()
        self = cls.from_buffer(buf)  # (keeps buf alive)
        self._whole = True
        return self

    def ref(self):
        """``ctypes.byref(self)`` for a C entry, refused unless the object is PLAN_BYTES long (made by DecodePlan())."""
        if not getattr(self, "_whole", False):
            raise KernelError(f"this DecodePlan was not made by DecodePlan(): it is {ctypes.sizeof(DecodePlan)} bytes "
                              f"and gpt2mi_decode_plan is {self.PLAN_BYTES} (array element, copy or from_buffer_copy?)")
        return ctypes.byref(self)

    def _tail_ptr(self, offset: int):
        self.ref()  # (an object without the tail has nothing at this offset)
        return _p.from_address(ctypes.addressof(self) + offset)

    def set_share(self, share_group, share_len) -> None:
        """Point the plan at the share map: two ctypes int arrays of B entries the owner keeps alive and may update in
        place, or (None, None) for no sharing."""
        if (share_group is None) != (share_len is None):
            raise KernelError("share_group and share_len go together")
        self._share = (share_group, share_len)  # the plan keeps what it points at alive
        self._tail_ptr(self.SHARE_GROUP_OFFSET).value = None if share_group is None else ctypes.addressof(share_group)
        self._tail_ptr(self.SHARE_LEN_OFFSET).value = None if share_len is None else ctypes.addressof(share_len)

    @property
    def share_group(self):
        return self._tail_ptr(self.SHARE_GROUP_OFFSET).value

    @property
    def share_len(self):
        return self._tail_ptr(self.SHARE_LEN_OFFSET).value


DecodePlan.KV_FORMAT_OFFSET = DecodePlan.rows.offset + ctypes.sizeof(_c_int)
assert DecodePlan.KV_FORMAT_OFFSET + ctypes.sizeof(_c_int) <= ctypes.sizeof(DecodePlan)
DecodePlan.SHARE_GROUP_OFFSET = ctypes.sizeof(DecodePlan)  # (pointer-aligned: the struct holds pointers)
DecodePlan.SHARE_LEN_OFFSET = DecodePlan.SHARE_GROUP_OFFSET + ctypes.sizeof(_p)
DecodePlan.PLAN_BYTES = DecodePlan.SHARE_LEN_OFFSET + ctypes.sizeof(_p)  # sizeof(gpt2mi_decode_plan) since v24


def gemm_skinny_workspace(M, N, K) -> int:
    """fp32 elements of workspace gemm_skinny needs at this shape (0: the strips alone cover the chip)."""
    return load().gpt2mi_gemm_skinny_workspace(M, N, K)


def gemm_skinny(epilogue, M, N, K, A, lda, W, ldw, C, ldc, bias=None, resid=None, workspace=None):
    """C[m][n] = epi(sum_k A[m][k] W[n][k] + bias[n]) for 1 <= M <= 64 rows (EPI_BF16 / EPI_F32 / EPI_RESID / EPI_GELU)."""
    ws_n = workspace.numel() if workspace is not None else 0
    _call("gpt2mi_gemm_skinny", epilogue, M, N, K, _ptr(A), lda, _ptr(W), ldw, _ptr(C), ldc, _ptr(bias), _ptr(resid),
          _ptr(workspace), ws_n, _stream())


# The entries that take a key/value cache, and their forms over an fp8 cache (v23): the same list with
# (kscale, vscale) behind (kcache, vcache).
_FP8_ENTRY = {"gpt2mi_kv_store": "gpt2mi_kv_store_fp8", "gpt2mi_attn_decode_ragged": "gpt2mi_attn_decode_fp8_ragged",
              "gpt2mi_attn_extend": "gpt2mi_attn_extend_fp8", "gpt2mi_attn_decode_shared": "gpt2mi_attn_decode_shared_fp8"}


def _kv_call(name, qkv, kcache, vcache, kscale, vscale, *tail, fp8=None):
    """Entry `name` on (qkv, the cache, *tail, the stream): over a bf16 cache, or with `fp8` (None: when either scale is
    given, so half a pair is the C entry's NULL refusal and never a bf16 read of codes) its fp8 form over uint8 codes
    [B][H][Tcap][64] and fp32 scales [B][H][Tcap] (generation.kv_quantize)."""
    if fp8 is None:
        fp8 = kscale is not None or vscale is not None
    scales = (_ptr(kscale), _ptr(vscale)) if fp8 else ()
    _call(_FP8_ENTRY[name] if fp8 else name, _ptr(qkv), _ptr(kcache), _ptr(vcache), *scales, *tail, _stream())


def kv_store(qkv, kcache, vcache, B, T_src, n, t0, H, D, Tcap, kscale=None, vscale=None):
    """Copy the K / V columns of the first n rows of each sequence of qkv [B*T_src, 3C] to cache positions t0.. (with
    kscale / vscale: quantised, gpt2mi_kv_store_fp8)."""
    _kv_call("gpt2mi_kv_store", qkv, kcache, vcache, kscale, vscale, B, T_src, n, t0, H, D, Tcap)


def attn_decode_workspace(B, H, Tcap) -> int:
    return load().gpt2mi_attn_decode_workspace(B, H, Tcap)


def attn_decode(qkv, kcache, vcache, out, workspace, B, H, D, Tcap, pos):
    """The new token's attention over cache positions 0..pos (its own k / v are written at pos first): attn_decode_ragged
    with every row at pos."""
    _call("gpt2mi_attn_decode", _ptr(qkv), _ptr(kcache), _ptr(vcache), _ptr(out), _ptr(workspace), workspace.numel(),
          B, H, D, Tcap, pos, _stream())


def embed_decode(tok, wte, wpe, x, B, C, pos):
    _call("gpt2mi_embed_decode", _ptr(tok), _ptr(wte), _ptr(wpe), _ptr(x), B, C, pos, _stream())


def decode_step(plan: DecodePlan, tok, pos):
    """One token step of the whole network (gpt2mi_decode_step) into plan.logits: decode_step_ragged with every row at
    pos. The package steps through decode_step_ragged; this binding serves the test that holds the two equal."""
    _call("gpt2mi_decode_step", plan.ref(), _ptr(tok), pos, _stream())


# ---- v17: device-side sampling (csrc/sample.hip) --------------------------------------------------
SAMPLE_MAX_V = 51200  # gpt2mi.h GPT2MI_SAMPLE_MAX_V


def _sampler_args(temperature, top_k, top_p, seed, eos):
    """The sampler's scalars as the C entries take them (top_k <= 0 and top_p >= 1 mean off, eos -1 none)."""
    return (float(temperature), 0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p),
            int(seed) & 0xFFFFFFFFFFFFFFFF, -1 if eos is None else int(eos))


def sample(logits, V, temperature, top_k, top_p, seed, pos, tok_out, eos=None, done=None, seq_out=None, probs_out=None):
    """gpt2mi_sample: one token per row of fp32 logits [B, ldl] (V valid columns) into tok_out (int64 [B]), column pos
    of seq_out (int64 [B, ld_seq]) and probs_out (fp32 [B, V], tests)."""
    t, k, p, s, e = _sampler_args(temperature, top_k, top_p, seed, eos)
    _call("gpt2mi_sample", _ptr(logits), logits.stride(0), logits.size(0), V, t, k, p, s, pos, e, _ptr(done),
          _ptr(tok_out), _ptr(seq_out), 0 if seq_out is None else seq_out.stride(0), _ptr(probs_out), _stream())


def decode_generate(plan: DecodePlan, V, temperature, top_k, top_p, seed, pos0, n, tok, eos=None, seq=None, done=None):
    """gpt2mi_decode_generate: n sample-then-step rounds from plan.logits without leaving C: decode_generate_ragged with
    every row starting at pos0 (as decode_step, kept for the test of that)."""
    t, k, p, s, e = _sampler_args(temperature, top_k, top_p, seed, eos)
    _call("gpt2mi_decode_generate", plan.ref(), V, t, k, p, s, e, pos0, n, _ptr(tok), _ptr(seq),
          0 if seq is None else seq.stride(0), _ptr(done), _stream())


# ---- v18: evaluation (csrc/lm_loss.hip) -------------------------------------------------------------
def lm_loss_workspace(M, V) -> int:
    """fp32 elements of workspace lm_loss needs for M rows over a vocabulary of V."""
    return load().gpt2mi_lm_loss_workspace(M, V) // 4


def lm_loss(x, ldx, w, ldw, w_rows, labels, M, V, K, loss_rows, lse, workspace, loss_sum=None, count=None,
            accumulate=False, loss_mean=None, ignore_index=-100):
    """gpt2mi_lm_loss: the rows of F.cross_entropy(x @ w[:V].T, labels) from bf16 x [M, ldx] and w [w_rows, ldw] without
    forming the logits; loss_sum / count (+)= this call's sum and number of valid labels, loss_mean = their ratio."""
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise KernelError(f"lm_loss takes bf16 operands (got {x.dtype}, {w.dtype})")
    if workspace.dtype != torch.float32 or workspace.numel() < lm_loss_workspace(M, V):
        raise KernelError(f"lm_loss: workspace of {workspace.numel()} {workspace.dtype} elements, needs "
                          f"{lm_loss_workspace(M, V)} fp32")
    _call("gpt2mi_lm_loss", _ptr(x), ldx, _ptr(w), ldw, w_rows, _ptr(labels), M, V, K, ignore_index, _ptr(loss_rows),
          _ptr(lse), _ptr(loss_sum), _ptr(count), int(accumulate), _ptr(loss_mean), _ptr(workspace), _stream())


# ---- v19: ragged decode (csrc/decode.hip, csrc/sample.hip) ------------------------------------------
DECODE_MAX_B = 64  # gpt2mi.h GPT2MI_DECODE_MAX_B


def _host_ints(vals, ctype=_c_int):
    """A host array for a `const int* pos` / `const uint32_t* row_id` argument (None: NULL). The entry reads it before it
    returns, so the temporary need not outlive the call."""
    if vals is None:
        return None
    vals = [int(v) for v in vals]
    return (ctype * len(vals))(*vals)


def _row_ids(row_id, B):
    if row_id is not None and len(row_id) != B:
        raise KernelError(f"row_id has {len(row_id)} entries for B={B} rows")
    return _host_ints(row_id, ctypes.c_uint32)


def _positions(pos, B):
    if len(pos) != B:
        raise KernelError(f"the position array has {len(pos)} entries for B={B} rows")
    return _host_ints(pos)


def attn_decode_ragged(qkv, kcache, vcache, out, workspace, B, H, D, Tcap, pos, kscale=None, vscale=None):
    """attn_decode with row b at pos[b] (a host sequence of B ints); with kscale / vscale over an fp8 cache."""
    _kv_call("gpt2mi_attn_decode_ragged", qkv, kcache, vcache, kscale, vscale, _ptr(out), _ptr(workspace),
             workspace.numel(), B, H, D, Tcap, _positions(pos, B))


def embed_decode_ragged(tok, wte, wpe, x, B, C, pos):
    _call("gpt2mi_embed_decode_ragged", _ptr(tok), _ptr(wte), _ptr(wpe), _ptr(x), B, C, _positions(pos, B), _stream())


def decode_step_ragged(plan: DecodePlan, tok, pos):
    """gpt2mi_decode_step_ragged: one token step with row b at pos[b], into plan.logits."""
    _call("gpt2mi_decode_step_ragged", plan.ref(), _ptr(tok), _positions(pos, plan.B), _stream())


# ---- v21: several rows of a launch in one sequence (csrc/decode.hip) -----------------------------------
def attn_extend(qkv, kcache, vcache, out, workspace, R, B, H, D, Tcap, seq, pos, kscale=None, vscale=None):
    """gpt2mi_attn_extend: attention of R rows, row r at position pos[r] of sequence seq[r] (host sequences of R ints);
    with kscale / vscale over an fp8 cache."""
    _kv_call("gpt2mi_attn_extend", qkv, kcache, vcache, kscale, vscale, _ptr(out), _ptr(workspace), workspace.numel(),
             R, B, H, D, Tcap, _positions(seq, R), _positions(pos, R))


def decode_extend(plan: DecodePlan, tok, seq, pos):
    """gpt2mi_decode_extend: the step's launch list on len(pos) rows of the row map (seq, pos), into plan.logits."""
    R = len(pos)
    _call("gpt2mi_decode_extend", plan.ref(), R, _ptr(tok), _positions(seq, R), _positions(pos, R), _stream())


# ---- v23: the fp8 key/value cache (csrc/decode.hip) ----------------------------------------------------
KV_BF16, KV_FP8 = 0, 1  # gpt2mi.h GPT2MI_KV_*: gpt2mi_decode_plan.kv_format


# The fp8 names forward to _kv_call's fp8 form whatever the scales are, so a missing scale is the C entry's refusal.
def kv_store_fp8(qkv, kcache, vcache, kscale, vscale, B, T_src, n, t0, H, D, Tcap):
    """kv_store into an fp8 cache: uint8 codes [B][H][Tcap][64] and fp32 scales [B][H][Tcap] (generation.kv_quantize)."""
    _kv_call("gpt2mi_kv_store", qkv, kcache, vcache, kscale, vscale, B, T_src, n, t0, H, D, Tcap, fp8=True)


def attn_decode_fp8_ragged(qkv, kcache, vcache, kscale, vscale, out, workspace, B, H, D, Tcap, pos):
    """attn_decode_ragged over an fp8 cache."""
    _kv_call("gpt2mi_attn_decode_ragged", qkv, kcache, vcache, kscale, vscale, _ptr(out), _ptr(workspace),
             workspace.numel(), B, H, D, Tcap, _positions(pos, B), fp8=True)


def attn_extend_fp8(qkv, kcache, vcache, kscale, vscale, out, workspace, R, B, H, D, Tcap, seq, pos):
    """attn_extend over an fp8 cache."""
    _kv_call("gpt2mi_attn_extend", qkv, kcache, vcache, kscale, vscale, _ptr(out), _ptr(workspace), workspace.numel(),
             R, B, H, D, Tcap, _positions(seq, R), _positions(pos, R), fp8=True)


# ---- v22: penalties in the sampler (csrc/sample.hip, csrc/decode.hip) -----------------------------------
PENALTY_MAX_HISTORY = 8192  # gpt2mi.h GPT2MI_PENALTY_MAX_HISTORY


class Penalties(ctypes.Structure):
    """gpt2mi_penalties"""
    _fields_ = [("repetition", _c_float), ("presence", _c_float), ("frequency", _c_float), ("hist", _p),
                ("ld_hist", _c_int), ("hist_rows", _c_int), ("hist_row", _p), ("gen_start", _p)]


def _penalties_arg(B, repetition, presence, frequency, hist, hist_row, gen_start):
    """(the gpt2mi_penalties of the keywords, the host arrays it points at, which must outlive the call)."""
    rows, starts = _host_ints(hist_row), _host_ints(gen_start)
    if any(a is not None and len(a) != B for a in (rows, starts)):
        raise KernelError(f"hist_row / gen_start must have B={B} entries")
    pen = Penalties(float(repetition), float(presence), float(frequency), _ptr(hist),
                    0 if hist is None else hist.stride(0), 0 if hist is None else hist.size(0),
                    ctypes.cast(rows, _p) if rows is not None else None,
                    ctypes.cast(starts, _p) if starts is not None else None)
    return pen, (rows, starts)


# ---- v24: rows that share a prompt cache (csrc/decode.hip) -------------------------------------------
def attn_decode_shared(qkv, kcache, vcache, out, workspace, B, H, D, Tcap, pos, share_group=None, share_len=None,
                       kscale=None, vscale=None):
    """gpt2mi_attn_decode_shared (with kscale / vscale: gpt2mi_attn_decode_shared_fp8): attn_decode_ragged with the share
    map (share_group, share_len), host sequences of B ints or both None. The bits of attn_decode_ragged."""
    sg, sl = _host_ints(share_group), _host_ints(share_len)
    if any(a is not None and len(a) != B for a in (sg, sl)):
        raise KernelError(f"share_group / share_len must have B={B} entries")
    _kv_call("gpt2mi_attn_decode_shared", qkv, kcache, vcache, kscale, vscale, _ptr(out), _ptr(workspace),
             workspace.numel(), B, H, D, Tcap, _positions(pos, B), sg, sl)


# ---- v24.1: per-token log-probabilities from the sampler (csrc/sample.hip, csrc/decode.hip) ------------------
LOGPROBS_MAX_TOP = 20  # gpt2mi.h GPT2MI_LOGPROBS_MAX_TOP


class Logprobs(ctypes.Structure):
    """gpt2mi_logprobs"""
    _fields_ = [("logprob", _p), ("ld", _c_int), ("top_n", _c_int), ("top_id", _p), ("top_logprob", _p), ("col", _p)]


def _logprobs_arg(logprob, top_ids, top_logprobs, col, B):
    """(the gpt2mi_logprobs of the tensors, what must outlive the call); (None, None) for logprob None: lp = NULL.
    logprob is fp32 [B, ld] (or [B]: ld 1), top_ids int32 / top_logprobs fp32 [B, ld, top_n], all contiguous."""
    if logprob is None:
        if top_ids is not None or top_logprobs is not None or col is not None:
            raise KernelError("top_ids / top_logprobs / col go with logprob")
        return None, None
    ld = logprob.size(1) if logprob.dim() == 2 else 1
    if logprob.dtype != torch.float32 or not logprob.is_contiguous() or logprob.numel() != B * ld:
        raise KernelError(f"logprob must be a contiguous fp32 [B={B}, ld] (or [B]) tensor")
    if (top_ids is None) != (top_logprobs is None):
        raise KernelError("top_ids and top_logprobs go together")
    n = 0 if top_ids is None else top_ids.size(-1)
    if n and (top_ids.dtype != torch.int32 or top_logprobs.dtype != torch.float32 or not top_ids.is_contiguous()
              or not top_logprobs.is_contiguous() or top_ids.numel() != B * ld * n or top_logprobs.numel() != B * ld * n):
        raise KernelError(f"top_ids (int32) and top_logprobs (fp32) must be contiguous [B={B}, ld={ld}, top_n]")
    cols = _host_ints(col)
    if cols is not None and len(cols) != B:
        raise KernelError(f"col has {len(cols)} entries for B={B} rows")
    lp = Logprobs(_ptr(logprob), ld, n, _ptr(top_ids) if n else None, _ptr(top_logprobs) if n else None,
                  ctypes.cast(cols, _p) if cols is not None else None)
    return ctypes.byref(lp), (lp, cols)


# ---- v24.4: logit bias, min-p, minimum length and stop sequences in the sampler (csrc/sample_con.hip, csrc/decode.hip) --
STOP_MAX_SEQS, STOP_MAX_LEN = 8, 16  # gpt2mi.h GPT2MI_STOP_MAX_SEQS / GPT2MI_STOP_MAX_LEN


class Constraints(ctypes.Structure):
    """gpt2mi_constraints"""
    _fields_ = [("bias", _p), ("ld_bias", _c_int), ("bias_rows", _c_int), ("bias_row", _p), ("min_p", _c_float),
                ("min_new", _c_int), ("n_stop", _c_int), ("stop", _p), ("stop_len", _p)]


def _constraints_arg(logit_bias, bias_row, min_p, min_new_tokens, stop, B):
    """(the gpt2mi_constraints of the keywords, what must outlive the call). logit_bias is a device fp32 [rows, ld] tensor
    with contiguous rows (None: no bias), bias_row B ints (-1: none; None: row b reads row b), stop a list of token
    lists. The values go to the entry as they are: it is the one that refuses them."""
    if logit_bias is not None and (logit_bias.dtype != torch.float32 or logit_bias.dim() != 2 or logit_bias.stride(1) != 1):
        raise KernelError("logit_bias must be an fp32 [rows, V] tensor with contiguous rows")
    rows = _host_ints(bias_row)
    if rows is not None and len(rows) != B:
        raise KernelError(f"bias_row has {len(rows)} entries for B={B} rows")
    stop = [[int(t) for t in s] for s in (stop or [])]
    lens = _host_ints([len(s) for s in stop]) if stop else None
    table = None
    if stop:  # (a length the entry refuses still gets its row: the tokens past STOP_MAX_LEN are not passed on)
        table = (ctypes.c_int32 * (len(stop) * STOP_MAX_LEN))()
        for i, s in enumerate(stop):
            table[i * STOP_MAX_LEN:i * STOP_MAX_LEN + min(len(s), STOP_MAX_LEN)] = s[:STOP_MAX_LEN]
    con = Constraints(_ptr(logit_bias), 0 if logit_bias is None else logit_bias.stride(0),
                      0 if logit_bias is None else logit_bias.size(0), ctypes.cast(rows, _p) if rows is not None else None,
                      float(min_p), int(min_new_tokens), len(stop), ctypes.cast(table, _p) if stop else None,
                      ctypes.cast(lens, _p) if stop else None)
    return ctypes.byref(con), (con, rows, lens, table)


# ---- the per-row sampler entries and generate loops: v19 ragged, v22 penalized, v24.1 logprobs, v24.4 constrained --------
# Each entry takes its predecessor's keywords and C arguments and adds a block of its own: below, per block, the keywords
# with their neutral values and the C arguments they become (before the sampler's stream, behind the loop's).
_ENTRIES = ("ragged", "penalized", "logprobs", "constrained")
_CON_OPTIONS = dict(logit_bias=None, bias_row=None, min_p=0.0, min_new_tokens=0, stop=None)
_SAMPLE_OPTIONS = (dict(row_id=None, eos=None, done=None, seq_out=None, probs_out=None),
                   dict(repetition=1.0, presence=0.0, frequency=0.0, hist=None, hist_row=None, gen_start=None,
                        logits_out=None),                                                    # pen, logits_out
                   dict(logprob=None, top_ids=None, top_logprobs=None, col=None), _CON_OPTIONS)  # lp; con
_GENERATE_OPTIONS = (dict(row_id=None, eos=None, seq=None, done=None),
                     dict(repetition=1.0, presence=0.0, frequency=0.0, gen_start=None),      # the four themselves
                     dict(logprob=None, top_ids=None, top_logprobs=None), _CON_OPTIONS)       # lp; con
_SAMPLE_TAIL, _GENERATE_TAIL = (0, 2, 3, 4), (0, 4, 5, 6)  # how much of the full tail an entry's C signature has


def _entry_options(name, blocks, given):
    """(the level of entry `name` in _ENTRIES, every block's keywords: `given` over the neutral values). A keyword of a
    later entry is a TypeError, as from a signature without it."""
    level = _ENTRIES.index(name.rsplit("_", 1)[1])
    for key in given:
        if not any(key in block for block in blocks[:level + 1]):
            raise TypeError(f"{name}() got an unexpected keyword argument '{key}'")
    return level, SimpleNamespace(**{**{k: v for block in blocks for k, v in block.items()}, **given})


def _sample_entry(name, logits, V, temperature, top_k, top_p, seed, pos, tok_out, **given):
    """gpt2mi_<name>, one of the four per-row sampler entries: one token per row of fp32 logits [B, ldl] (V valid
    columns) into tok_out (int64 [B]), row b drawing from (seed, row_id[b] (None: b), pos[b]) into column pos[b] of
    seq_out (int64 [B, ld_seq]); probs_out (fp32 [B, V], tests). The keywords: the forwarders below."""
    level, o = _entry_options(name, _SAMPLE_OPTIONS, given)
    (t, k, p, s, e), B = _sampler_args(temperature, top_k, top_p, seed, o.eos), logits.size(0)
    pen, _alive_pen = _penalties_arg(B, o.repetition, o.presence, o.frequency, o.hist, o.hist_row, o.gen_start)
    lp, _alive_lp = _logprobs_arg(o.logprob, o.top_ids, o.top_logprobs, o.col, B)
    con, _alive_con = _constraints_arg(o.logit_bias, o.bias_row, o.min_p, o.min_new_tokens, o.stop, B)
    tail = (ctypes.byref(pen), _ptr(o.logits_out), lp, con)[:_SAMPLE_TAIL[level]]
    _call("gpt2mi_" + name, _ptr(logits), logits.stride(0), B, V, t, k, p, s, _positions(pos, B), _row_ids(o.row_id, B), e,
          _ptr(o.done), _ptr(tok_out), _ptr(o.seq_out), 0 if o.seq_out is None else o.seq_out.stride(0),
          _ptr(o.probs_out), *tail, _stream())


def _generate_entry(name, plan, V, temperature, top_k, top_p, seed, pos0, n, tok, **given):
    """gpt2mi_<name>, one of the four per-row generate loops: n sample-then-step rounds from plan.logits without leaving
    C, row b starting at pos0[b], the tokens into tok and seq as the sampler writes tok_out and seq_out."""
    level, o = _entry_options(name, _GENERATE_OPTIONS, given)
    scalars, B = _sampler_args(temperature, top_k, top_p, seed, o.eos), plan.B
    if o.gen_start is not None and len(o.gen_start) != B:
        raise KernelError(f"gen_start has {len(o.gen_start)} entries for B={B} rows")
    lp, _alive_lp = _logprobs_arg(o.logprob, o.top_ids, o.top_logprobs, None, B)
    con, _alive_con = _constraints_arg(o.logit_bias, o.bias_row, o.min_p, o.min_new_tokens, o.stop, B)
    tail = (float(o.repetition), float(o.presence), float(o.frequency), _host_ints(o.gen_start), lp, con)
    _call("gpt2mi_" + name, plan.ref(), V, *scalars, _positions(pos0, B), _row_ids(o.row_id, B), n, _ptr(tok), _ptr(o.seq),
          0 if o.seq is None else o.seq.stride(0), _ptr(o.done), _stream(), *tail[:_GENERATE_TAIL[level]])


# The public names: (logits, V, temperature, top_k, top_p, seed, pos, tok_out, **keywords) and
# (plan, V, temperature, top_k, top_p, seed, pos0, n, tok, **keywords), the keywords being the entry's blocks above.
def sample_ragged(*head, **keywords):
    """gpt2mi_sample_ragged: `sample` with row b drawing from (seed, row_id[b] (None: b), pos[b]) into column pos[b];
    row_id, eos, done, seq_out, probs_out."""
    _sample_entry("sample_ragged", *head, **keywords)


def sample_penalized(*head, **keywords):
    """gpt2mi_sample_penalized: `sample_ragged` with row b's logits moved (repetition, presence, frequency) by its
    history hist[hist_row[b], :pos[b]] (int64 [rows, ld]; hist_row None: b), the generated part from gen_start[b] (None:
    0); logits_out (fp32 [B, V]) takes the penalised logits."""
    _sample_entry("sample_penalized", *head, **keywords)


def sample_logprobs(*head, **keywords):
    """gpt2mi_sample_logprobs: `sample_penalized`, and row b's raw log-probability of the token it draws into
    logprob[b, col[b]] (col None: pos[b]), its top_n alternatives into top_ids / top_logprobs[b, col[b]]
    (generation.token_logprobs). logprob None: lp = NULL, gpt2mi_sample_penalized itself under this entry's name."""
    _sample_entry("sample_logprobs", *head, **keywords)


def sample_constrained(*head, **keywords):
    """gpt2mi_sample_constrained: `sample_logprobs` under generation.apply_constraints (logit_bias fp32 [rows, V], row b
    reading row bias_row[b]; min_new_tokens holding eos back while pos[b] - gen_start[b] < it), sample_reference's min_p
    and generation.stop_match over hist (stop: up to 8 lists of up to 16 tokens; a match sets done[b]). logits_out takes
    the row after the bias and the eos suppression. Every keyword neutral: sample_logprobs itself under this name."""
    _sample_entry("sample_constrained", *head, **keywords)


def decode_generate_ragged(*head, **keywords):
    """gpt2mi_decode_generate_ragged: `decode_generate` with row b starting at pos0[b]; row_id, eos, seq, done."""
    _generate_entry("decode_generate_ragged", *head, **keywords)


def decode_generate_penalized(*head, **keywords):
    """gpt2mi_decode_generate_penalized: `decode_generate_ragged` with repetition, presence, frequency and gen_start, seq
    as the history the sampler reads."""
    _generate_entry("decode_generate_penalized", *head, **keywords)


def decode_generate_logprobs(*head, **keywords):
    """gpt2mi_decode_generate_logprobs: `decode_generate_penalized`, step i writing column pos0[b] + i of logprob /
    top_ids / top_logprobs as it does of seq."""
    _generate_entry("decode_generate_logprobs", *head, **keywords)


def decode_generate_constrained(*head, **keywords):
    """gpt2mi_decode_generate_constrained: `decode_generate_logprobs` with sample_constrained's keywords (logit_bias,
    bias_row, min_p, min_new_tokens, stop), seq the history the stop sequences are matched in."""
    _generate_entry("decode_generate_constrained", *head, **keywords)


# ---- v24.2: beam search on the device (csrc/beam.hip) ---------------------------------------------------------
BEAM_LOOP_BYTES = DECODE_MAX_B * (8 * LOGPROBS_MAX_TOP + 4)  # gpt2mi.h GPT2MI_BEAM_LOOP_BYTES


def beam_select(top_ids, top_logprobs, cum, done, G, W, eos, tok_out, parent_out, cum_out, done_out):
    """gpt2mi_beam_select (generation.beam_select is the rule): top_ids int32 / top_logprobs fp32 [G W, W], cum fp32 and
    done uint8 [G W]; the new beams' tok_out int64, parent_out int32 (absolute rows), cum_out, done_out [G W]."""
    for name, t, dt in (("top_ids", top_ids, torch.int32), ("top_logprobs", top_logprobs, torch.float32),
                        ("cum", cum, torch.float32), ("done", done, torch.uint8), ("tok_out", tok_out, torch.int64),
                        ("parent_out", parent_out, torch.int32), ("cum_out", cum_out, torch.float32),
                        ("done_out", done_out, torch.uint8)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < G * W * (W if name.startswith("top_") else 1):
            raise KernelError(f"beam_select: {name} must be a contiguous {dt} tensor of G W{' W' * name.startswith('top_')} "
                              f"elements")
    _call("gpt2mi_beam_select", _ptr(top_ids), _ptr(top_logprobs), _ptr(cum), _ptr(done), G, W,
          -1 if eos is None else int(eos), _ptr(tok_out), _ptr(parent_out), _ptr(cum_out), _ptr(done_out), _stream())


def beam_reorder_workspace(kv_format, L, H, R, window) -> int:
    """Bytes of staging gpt2mi_beam_reorder needs for R rows and windows of up to `window` positions."""
    return load().gpt2mi_beam_reorder_workspace(kv_format, L, H, R, window)


def beam_reorder(kcache, vcache, parent, G, W, lo, hi, workspace, seq=None, kscale=None, vscale=None):
    """gpt2mi_beam_reorder on cache tensors [L, B, H, Tcap, 64] (bf16, or uint8 codes with kscale / vscale fp32
    [L, B, H, Tcap]): rows r < G W with parent[r] != r (device int32) take positions [lo[r], hi[r]) of row parent[r], in
    the caches and in seq (int64 [>= G W, ld]); lo / hi are host sequences of G W ints."""
    fp8 = kscale is not None or vscale is not None
    tensors = [kcache, vcache] + ([kscale, vscale] if fp8 else [])
    if kcache.dim() != 5 or any(t is None or not t.is_contiguous() for t in tensors) or vcache.shape != kcache.shape:
        raise KernelError("beam_reorder takes contiguous cache tensors [L, B, H, Tcap, 64] (and scales [L, B, H, Tcap])")
    if parent.dtype != torch.int32 or not parent.is_contiguous() or parent.numel() < G * W:
        raise KernelError("beam_reorder: parent must be a contiguous int32 tensor of G W rows")
    if seq is not None and (seq.dtype != torch.int64 or seq.dim() != 2 or seq.stride(1) != 1 or seq.size(0) < G * W):
        raise KernelError("beam_reorder: seq must be int64 [>= G W, ld] with contiguous rows")
    L, B, H, Tcap = kcache.shape[:4]
    _call("gpt2mi_beam_reorder", _ptr(kcache), _ptr(vcache), _ptr(kscale), _ptr(vscale), KV_FP8 if fp8 else KV_BF16, L,
          B * H * Tcap, B, H, Tcap, _ptr(seq), 0 if seq is None else seq.stride(0), _ptr(parent), G, W,
          _positions(lo, G * W), _positions(hi, G * W), _ptr(workspace),
          0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())


def decode_beam_search(plan: DecodePlan, V, W, pos0, lo, n, tok, seq, cum, done, workspace, eos=None, parents=None):
    """gpt2mi_decode_beam_search: n rounds of (top W, select, reorder, step) over the plan's rows, groups of W; cum fp32 /
    done uint8 [B] carry the state, parents (int32 [n, B], optional) receives every step's parent rows."""
    _call("gpt2mi_decode_beam_search", plan.ref(), V, W, -1 if eos is None else int(eos), _positions(pos0, plan.B),
          _positions(lo, plan.B), n, _ptr(tok), _ptr(seq), 0 if seq is None else seq.stride(0), _ptr(cum), _ptr(done),
          _ptr(parents), _ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
          _stream())
