"""The indexer MQA logits of the reference's attention section (``csrc/apis/attention.hpp``), FP8 operands only.

Names, argument order, keywords and defaults follow the reference's bindings (``register_apis``).  Each call checks its arguments before any
device work (``RuntimeError`` as the reference's host asserts), allocates the logits the way the reference does -- rows padded to a
multiple of ``128 / H`` (dense), row stride a multiple of 1024 bytes, so ``.shape`` and ``.stride(0)`` match -- and launches on the
current torch stream without synchronising: ``get_paged_mqa_logits_metadata`` + ``fp8_paged_mqa_logits`` capture in one graph.

Every element is ``sum_h w[i, h] * relu(sf[j] * sum_d q[i, h, d] * kv[j, d])``: exact FP8 products, FP32 accumulation in one fixed order
that does not depend on the work split (``set_num_sms``), a BF16 result rounded once.  Out of scope: FP4 operands (``q_sf`` given),
the varlen ``indices`` form, 1-D ``context_lens`` and ``clean_logits`` on the paged form (the reference rejects it with 2-D lengths).
"""
from typing import Optional, Tuple

import torch

from ._lib import lib, check, current_stream_ptr, require_device
from .errors import host_assert
from . import runtime

_HEADS = (8, 16, 32, 64)
_HEAD_DIMS = (32, 64, 128)
_BLOCK_QH = 128              # Q rows (tokens x heads) of one dense block: logits rows are padded to a multiple of 128 / H
_BLOCK_KV = 256              # KV columns of a split: slack / alignment of the logits row stride
_DG_BF16, _DG_FP32 = 0, 1


def _align(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _logits_code(logits_dtype: torch.dtype) -> int:
    host_assert(logits_dtype in (torch.float32, torch.bfloat16), 'logits_dtype == torch::kFloat32 or logits_dtype == torch::kBFloat16')
    return _DG_FP32 if logits_dtype == torch.float32 else _DG_BF16


def _fp8_q(q: Tuple[torch.Tensor, Optional[torch.Tensor]], dims: int) -> torch.Tensor:
    host_assert(isinstance(q, (tuple, list)) and len(q) == 2, 'q is a tuple (q_fp8, q_sf)')
    q_fp, q_sf = q
    host_assert(q_sf is None, 'FP4 is not supported: q_sf must be None (FP8 q only)')
    host_assert(isinstance(q_fp, torch.Tensor) and q_fp.dim() == dims, f'q.dim() == {dims}')
    host_assert(q_fp.size(-2) in _HEADS, 'num_heads == 8 or num_heads == 16 or num_heads == 32 or num_heads == 64')
    host_assert(q_fp.size(-1) in _HEAD_DIMS, 'head_dim == 32 or head_dim == 64 or head_dim == 128')
    host_assert(q_fp.is_contiguous(), 'q_fp.is_contiguous()')
    host_assert(q_fp.dtype == torch.float8_e4m3fn, 'q_fp.scalar_type() == torch::kFloat8_e4m3fn')
    return q_fp


def _weights_code(weights: torch.Tensor, rows: int, num_heads: int, logits_dtype: torch.dtype) -> int:
    host_assert(weights.dim() == 2 and tuple(weights.shape) == (rows, num_heads), 'weights shape == [rows, num_heads]')
    host_assert(weights.stride(1) == 1, 'weights.stride(1) == 1')
    host_assert(weights.dtype in (torch.float32, torch.bfloat16), 'weights.scalar_type() == torch::kFloat or torch::kBFloat16')
    host_assert(weights.dtype != torch.bfloat16 or logits_dtype == torch.bfloat16,
                'weights.scalar_type() != torch::kBFloat16 or logits_dtype == torch::kBFloat16')
    return _DG_FP32 if weights.dtype == torch.float32 else _DG_BF16


def _int32_vector(t: torch.Tensor, n: int, what: str) -> None:
    host_assert(isinstance(t, torch.Tensor) and t.dim() == 1 and t.size(0) == n, f'{what}.size(0) == seq_len')
    host_assert(t.is_contiguous(), f'{what}.is_contiguous()')
    host_assert(t.dtype == torch.int32, f'{what}.scalar_type() == torch::kInt')


def fp8_fp4_mqa_logits(q: Tuple[torch.Tensor, Optional[torch.Tensor]], kv: Tuple[torch.Tensor, torch.Tensor], weights: torch.Tensor,
                       cu_seq_len_k_start: torch.Tensor, cu_seq_len_k_end: torch.Tensor,
                       clean_logits: bool = True, max_seqlen_k: int = 0, logits_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Prefill logits ``[S, S_kv]`` (or ``[S, max_seqlen_k]``, compressed) of ``q [S, H, D]`` against ``kv = (kv_fp8 [S_kv, D],
    kv_sf [S_kv])``.  Row i holds the columns ``max(ks[i], 0) <= j < min(ke[i], S_kv)`` -- at j, or at ``j - ks[i]`` when compressed;
    ``clean_logits`` makes every other column ``-inf`` (not allowed together with ``max_seqlen_k > 0``)."""
    q_fp = _fp8_q(q, 3)
    seq_len, num_heads, head_dim = q_fp.shape
    host_assert(isinstance(kv, (tuple, list)) and len(kv) == 2, 'kv is a tuple (kv_fp8, kv_sf)')
    kv_fp, kv_sf = kv
    host_assert(kv_fp.dim() == 2 and kv_fp.size(1) == head_dim, 'kv_fp shape == [seq_len_kv, head_dim]')
    host_assert(kv_fp.is_contiguous(), 'kv_fp.is_contiguous()')
    host_assert(kv_fp.dtype == torch.float8_e4m3fn, 'kv_fp.scalar_type() == torch::kFloat8_e4m3fn')
    seq_len_kv = kv_fp.size(0)
    host_assert(kv_sf.dim() == 1 and kv_sf.size(0) == seq_len_kv, 'kv_sf shape == [seq_len_kv]')
    host_assert(kv_sf.is_contiguous(), 'kv_sf.is_contiguous()')
    host_assert(kv_sf.dtype == torch.float32, 'kv_sf.scalar_type() == torch::kFloat')
    code = _logits_code(logits_dtype)
    w_code = _weights_code(weights, seq_len, num_heads, logits_dtype)
    _int32_vector(cu_seq_len_k_start, seq_len, 'cu_seq_len_k_start')
    _int32_vector(cu_seq_len_k_end, seq_len, 'cu_seq_len_k_end')
    max_seqlen_k = int(max_seqlen_k)
    host_assert(max_seqlen_k >= 0, 'max_seqlen_k >= 0')
    host_assert(not (clean_logits and max_seqlen_k > 0), 'not clean_logits (with max_seqlen_k > 0)')
    require_device(q_fp, kv_fp, kv_sf, weights, cu_seq_len_k_start, cu_seq_len_k_end)

    # allocation of the reference (attention.hpp:159-178)
    block_q = _BLOCK_QH // num_heads
    stride_alignment = 1024 // (torch.finfo(logits_dtype).bits // 8)
    cols = max_seqlen_k if max_seqlen_k > 0 else seq_len_kv
    stride = _align(_align(max_seqlen_k, _BLOCK_KV), stride_alignment) if max_seqlen_k > 0 else _align(seq_len_kv + _BLOCK_KV, stride_alignment)
    logits = torch.empty((_align(seq_len, block_q), stride), dtype=logits_dtype, device=q_fp.device)[:seq_len, :cols]
    if seq_len == 0 or seq_len_kv == 0:
        return logits
    stream = current_stream_ptr()
    check(lib.dg_fp8_mqa_logits(q_fp.data_ptr(), kv_fp.data_ptr(), kv_sf.data_ptr(), weights.data_ptr(), cu_seq_len_k_start.data_ptr(),
                                cu_seq_len_k_end.data_ptr(), logits.data_ptr(), seq_len, seq_len_kv, num_heads, head_dim, weights.stride(0),
                                stride, max_seqlen_k, code, w_code, stream))
    if clean_logits:
        check(lib.dg_clean_logits(cu_seq_len_k_start.data_ptr(), cu_seq_len_k_end.data_ptr(), logits.data_ptr(), seq_len, seq_len_kv,
                                  stride, code, stream))
    return logits


def fp8_mqa_logits(q: torch.Tensor, kv: Tuple[torch.Tensor, torch.Tensor], weights: torch.Tensor,
                   cu_seq_len_k_start: torch.Tensor, cu_seq_len_k_end: torch.Tensor,
                   clean_logits: bool = True, max_seqlen_k: int = 0) -> torch.Tensor:
    """``fp8_fp4_mqa_logits((q, None), ..., logits_dtype=torch.float32)``, the reference's legacy entry."""
    return fp8_fp4_mqa_logits((q, None), kv, weights, cu_seq_len_k_start, cu_seq_len_k_end, clean_logits, max_seqlen_k, torch.float32)


def _context_lens(context_lens: torch.Tensor) -> None:
    host_assert(isinstance(context_lens, torch.Tensor) and context_lens.dim() == 2, 'context_lens.dim() == 2 (only 2-D context lens)')
    host_assert(context_lens.dtype == torch.int32, 'context_lens.scalar_type() == torch::kInt')
    host_assert(context_lens.is_contiguous(), 'context_lens.is_contiguous()')


def get_paged_mqa_logits_metadata(context_lens: torch.Tensor, block_kv: int, num_sms: int,
                                  indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The work split of ``fp8_paged_mqa_logits`` over ``num_sms`` workgroups, ``[num_sms + 1, 2]`` int32, computed on the device
    from ``context_lens [B, next_n]``.  Its contents are this implementation's own; only the paged kernel reads them."""
    host_assert(indices is None, 'indices is not supported (the varlen form)')
    _context_lens(context_lens)
    host_assert(block_kv in (32, 64), 'block_kv == 64 or block_kv == 32')
    num_sms = int(num_sms)
    host_assert(num_sms >= 1, 'num_sms >= 1')
    require_device(context_lens)
    schedule = torch.empty((num_sms + 1, 2), dtype=torch.int32, device=context_lens.device)
    check(lib.dg_paged_mqa_logits_metadata(context_lens.data_ptr(), schedule.data_ptr(), context_lens.size(0), context_lens.size(1),
                                           block_kv, num_sms, current_stream_ptr()))
    return schedule


def fp8_fp4_paged_mqa_logits(q: Tuple[torch.Tensor, Optional[torch.Tensor]], kv_cache: torch.Tensor, weights: torch.Tensor,
                             context_lens: torch.Tensor, block_table: torch.Tensor, schedule_meta: torch.Tensor, max_context_len: int,
                             clean_logits: bool = False, logits_dtype: torch.dtype = torch.float32,
                             indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode logits ``[B * next_n, max_context_len]`` of ``q [B, next_n, H, D]`` against the paged cache ``kv_cache [blocks, block_kv,
    1, D + 4]`` (per block: block_kv FP8 rows, then block_kv FP32 scales).  Row ``b * next_n + t`` holds the columns below
    ``context_lens[b, t]``; the rest are unspecified.  ``schedule_meta`` comes from ``get_paged_mqa_logits_metadata`` with the current
    ``get_num_sms()``."""
    q_fp = _fp8_q(q, 4)
    batch, next_n, num_heads, head_dim = q_fp.shape
    host_assert(next_n >= 1, 'next_n >= 1')
    host_assert(indices is None, 'indices is not supported (the varlen form)')
    host_assert(kv_cache.dim() == 4, 'kv_cache.dim() == 4')
    num_kv_blocks, block_kv, num_heads_kv, head_dim_with_sf = kv_cache.shape
    host_assert(block_kv in (32, 64), 'block_kv == 32 or block_kv == 64')
    host_assert(num_heads_kv == 1 and head_dim_with_sf == head_dim + 4, 'num_heads_kv == 1 and head_dim_with_sf == head_dim + sizeof(float)')
    host_assert(kv_cache.stride(1) == head_dim_with_sf and kv_cache.stride(3) == 1,
                'fused_kv_cache.stride(1) == head_dim_with_sf and fused_kv_cache.stride(3) == 1')
    host_assert(kv_cache.dtype == torch.uint8, 'fused_kv_cache.scalar_type() == torch::kByte')
    host_assert(kv_cache.stride(0) % 4 == 0 and kv_cache.data_ptr() % 4 == 0, 'kv_cache_stride_bytes % sizeof(float) == 0')
    code = _logits_code(logits_dtype)
    w_code = _weights_code(weights, batch * next_n, num_heads, logits_dtype)
    host_assert(weights.is_contiguous(), 'weights.is_contiguous()')
    host_assert(block_table.dim() == 2 and block_table.size(0) == batch, 'block_table shape == [batch_size, max_blocks]')
    host_assert(block_table.stride(1) == 1, 'block_table.stride(1) == 1')
    host_assert(block_table.dtype == torch.int32, 'block_table.scalar_type() == torch::kInt')
    num_sms = runtime.get_num_sms()
    host_assert(schedule_meta.dim() == 2 and tuple(schedule_meta.shape) == (num_sms + 1, 2),
                'schedule_meta shape == [get_num_sms() + 1, 2] (rebuild it after set_num_sms)')
    host_assert(schedule_meta.is_contiguous(), 'schedule_meta.is_contiguous()')
    host_assert(schedule_meta.dtype == torch.int32, 'schedule_meta.scalar_type() == torch::kInt')
    _context_lens(context_lens)
    host_assert(tuple(context_lens.shape) == (batch, next_n), 'context_lens shape == [batch_size, next_n]')
    host_assert(not clean_logits, 'not clean_logits (with 2-D context lens)')
    max_context_len = int(max_context_len)
    host_assert(max_context_len >= 0, 'max_context_len >= 0')
    require_device(q_fp, kv_cache, weights, context_lens, block_table, schedule_meta)

    # allocation of the reference (attention.hpp:372-379)
    stride = _align(_align(max_context_len, _BLOCK_KV), 1024 // (torch.finfo(logits_dtype).bits // 8))
    logits = torch.empty((batch * next_n, stride), dtype=logits_dtype, device=q_fp.device)[:, :max_context_len]
    if batch == 0 or max_context_len == 0 or num_kv_blocks == 0 or block_table.size(1) == 0:
        return logits
    check(lib.dg_fp8_paged_mqa_logits(q_fp.data_ptr(), kv_cache.data_ptr(), weights.data_ptr(), context_lens.data_ptr(),
                                      block_table.data_ptr(), schedule_meta.data_ptr(), logits.data_ptr(), batch, next_n, num_heads,
                                      head_dim, block_kv, block_table.size(1), kv_cache.stride(0), block_table.stride(0),
                                      weights.stride(0), stride, max_context_len, num_sms, code, w_code, current_stream_ptr()))
    return logits


def fp8_paged_mqa_logits(q: torch.Tensor, kv_cache: torch.Tensor, weights: torch.Tensor, context_lens: torch.Tensor,
                         block_table: torch.Tensor, schedule_meta: torch.Tensor, max_context_len: int,
                         clean_logits: bool = False, indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``fp8_fp4_paged_mqa_logits((q, None), ..., logits_dtype=torch.float32)``, the reference's legacy entry."""
    return fp8_fp4_paged_mqa_logits((q, None), kv_cache, weights, context_lens, block_table, schedule_meta, max_context_len,
                                    clean_logits, torch.float32, indices)
