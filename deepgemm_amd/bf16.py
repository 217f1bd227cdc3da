"""The BF16 GEMM operator surface (host side): validation, trivial cases, re-majoring of MN-major operands, C-ABI call.

Names, argument order, keywords and defaults follow the reference's bindings (``csrc/apis/gemm.hpp:404-560``, ``m.def`` table).
``compiled_dims`` is accepted and does not affect results (there is no JIT).  ``nn`` / ``tn`` / ``tt`` are the ``nt`` call on transposed
views; an MN-major operand is re-majored into a K-major temporary by ``dg_transpose_bf16`` (stream-ordered, one pass) whatever its size,
and the K-major kernels run on it.  Arithmetic: ``D = round_to_d_dtype(acc_fp32 + float(C))``, rounded once.
Every call is asynchronous on the current torch stream and never synchronises.
"""
from typing import Optional

import torch

from ._lib import lib, check, current_stream_ptr, require_device
from .errors import host_assert
from .gemm import _early_return, _sig, _split_k_workspace, _dtype_code
from .layout import check_major_type_cd, major_check
from . import runtime

_NORMAL, _CONTIGUOUS, _CONTIGUOUS_PSUM, _MASKED = 0, 1, 2, 3

# Validated call signatures of the dense entry -> the integer arguments of its C call (the FP8 entries' host-overhead diet: a repeated
# decode-sized call skips the checks).  set_forced_config clears it: whether a call passes the K-split workspace depends on the configuration.
_VALIDATED_BF16 = {}


def _check_ab_bf16(t: torch.Tensor, dims: int):
    host_assert(t.dim() == dims, f't.dim() == {dims}')
    host_assert(t.dtype == torch.bfloat16, 'ab.scalar_type() == torch::kBFloat16')
    return tuple(int(s) for s in t.shape)


def _k_major(t: torch.Tensor) -> torch.Tensor:
    """A BF16 operand ``[.., mn, k]`` as the kernels read it: as it is when K-major, else (an MN-major view: unit stride along mn, the
    row-major ``[.., k, mn]`` it was made from) a fresh K-major copy made by dg_transpose_bf16.  K-major rows must be whole 16-byte chunks:
    the reference's TMA condition on row strides."""
    if t.stride(-2) != 1 or t.stride(-1) == 1:
        host_assert(t.stride(-1) == 1, 'the operand is K-major or MN-major')
        host_assert((t.size(-2) <= 1 or t.stride(-2) % 8 == 0) and (t.dim() == 2 or t.size(0) <= 1 or t.stride(0) % 8 == 0),
                    'row strides of a K-major BF16 operand are multiples of 8 elements (16 bytes)')
        host_assert(t.data_ptr() % 16 == 0, 'BF16 operands are 16-byte aligned')
        return t
    require_device(t)
    mn, k = t.size(-2), t.size(-1)
    batches = t.size(0) if t.dim() == 3 else 1
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)          # contiguous: K-major
    check(lib.dg_transpose_bf16(t.data_ptr(), out.data_ptr(), batches, k, mn, t.stride(-1), k,
                                t.stride(0) if t.dim() == 3 else 0, mn * k, current_stream_ptr()))
    return out


def _require_k_multiple_of_8(k: int) -> None:
    host_assert(k % 8 == 0, 'k % 8 == 0 (BF16 rows in whole 16-byte chunks)')


def bf16_gemm_nt(a: torch.Tensor, b: torch.Tensor, d: torch.Tensor, c: Optional[torch.Tensor] = None,
                 compiled_dims: str = 'nk') -> None:
    """D = C + A @ B^T; ``a [M, K]``, ``b [N, K]`` BF16, ``d [M, N]`` BF16 or FP32 (row-major)."""
    same_cd = c is not None and c.data_ptr() == d.data_ptr()
    key = (_sig(a), _sig(b), _sig(d), _sig(c), same_cd)
    plan = _VALIDATED_BF16.get(key)
    if plan is not None and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0:
        args, device_index, wants_ws = plan
        if c is not None and not same_cd:
            d.copy_(c)
        stream = current_stream_ptr(device_index)
        ws = _split_k_workspace(d.device, stream) if wants_ws else None
        check(lib.dg_bf16_gemm_nt(a.data_ptr(), b.data_ptr(), d.data_ptr(), *args,
                                  ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream))
        return
    major_check(a), major_check(b)
    check_major_type_cd(d)
    m, k = _check_ab_bf16(a, 2)
    n, k_ = _check_ab_bf16(b, 2)
    host_assert(d.dim() == 2, 'd.dim() == 2')
    host_assert((m, n) == tuple(d.shape) and k == k_, 'm == m_ and n == n_ and k == k_')
    host_assert(d.dtype in (torch.bfloat16, torch.float), 'd.scalar_type() == torch::kBFloat16 or d.scalar_type() == torch::kFloat')
    if c is not None:
        host_assert(c.dtype == d.dtype, 'd.scalar_type() == c.value().scalar_type()')
    if _early_return(m, n, k, d, c):
        return
    _require_k_multiple_of_8(k)
    a_km, b_km = _k_major(a), _k_major(b)
    require_device(a, b, d)
    args = (m, n, k, a_km.stride(0), b_km.stride(0), d.stride(0), _dtype_code(d), int(c is not None))
    picked = lib.dg_bf16_select_config(_NORMAL, m, n, k, 1, 0, 0, 1)
    wants_ws = b'_ks_' in picked or b'_ks_' in lib.dg_get_forced_config()
    if a_km is a and b_km is b and len(_VALIDATED_BF16) < 4096:
        _VALIDATED_BF16[key] = (args, d.device.index if d.device.index is not None else -1, wants_ws)
    stream = current_stream_ptr()
    ws = _split_k_workspace(d.device, stream) if wants_ws else None
    check(lib.dg_bf16_gemm_nt(a_km.data_ptr(), b_km.data_ptr(), d.data_ptr(), *args,
                              ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream))


def bf16_gemm_nn(a, b, d, c=None, compiled_dims='nk') -> None:
    """``b [K, N]``: a transposed view of NT (csrc/apis/gemm.hpp:404-560)."""
    bf16_gemm_nt(a, b.transpose(0, 1), d, c, compiled_dims)


def bf16_gemm_tn(a, b, d, c=None, compiled_dims='mn') -> None:
    """``a [K, M]``, ``b [K, N]``."""
    bf16_gemm_nt(a.transpose(0, 1), b.transpose(0, 1), d, c, compiled_dims)


def bf16_gemm_tt(a, b, d, c=None, compiled_dims='mn') -> None:
    """``a [K, M]``, ``b [N, K]``."""
    bf16_gemm_nt(a.transpose(0, 1), b, d, c, compiled_dims)


def m_grouped_bf16_gemm_nt_contiguous(a: torch.Tensor, b: torch.Tensor, d: torch.Tensor, grouped_layout: torch.Tensor,
                                      compiled_dims: str = 'nk', use_psum_layout: bool = False, ensure_zero_padding: bool = True,
                                      expected_m_for_psum_layout: Optional[int] = None) -> None:
    """Rows of ``a [M, K]`` grouped contiguously (each group padded to the M alignment), ``b [G, N, K]``, ``d [M, N]`` BF16; rows whose
    ``grouped_layout`` entry is -1 are written as zeros.  ``use_psum_layout``: ``grouped_layout [G]`` holds the groups' cumulative ends."""
    host_assert(a.dim() == 2 and a.stride(-1) == 1, 'major_a == cute::UMMA::Major::K')
    major_check(b)
    host_assert(grouped_layout.is_contiguous(), 'grouped_layout.is_contiguous()')
    m, k = _check_ab_bf16(a, 2)
    num_groups, n, k_ = _check_ab_bf16(b, 3)
    host_assert(d.dim() == 2, 'd.dim() == 2')
    host_assert((m, n) == tuple(d.shape) and k == k_, 'm == m_ and n == n_ and k == k_')
    host_assert(n > 0 and k > 0 and num_groups > 0, 'n > 0 and k > 0 and num_groups > 0')
    host_assert(d.dtype == torch.bfloat16, 'd.scalar_type() == torch::kBFloat16')
    host_assert(grouped_layout.dtype == torch.int, 'grouped_layout.scalar_type() == torch::kInt')
    host_assert(grouped_layout.dim() == 1, 'grouped_layout.dim() == 1')
    if use_psum_layout:
        host_assert(grouped_layout.numel() == num_groups, 'num_groups == num_groups_')
    else:
        host_assert(grouped_layout.numel() == m, 'm == m__')
        host_assert(expected_m_for_psum_layout is None, 'not expected_m_for_psum_layout.has_value()')
    check_major_type_cd(d)
    if m == 0:
        return
    _require_k_multiple_of_8(k)
    a_km, b_km = _k_major(a), _k_major(b)
    require_device(a, b, d, grouped_layout)
    check(lib.dg_m_grouped_bf16_gemm_nt_contiguous(
        a_km.data_ptr(), b_km.data_ptr(), d.data_ptr(), grouped_layout.data_ptr(), num_groups, m, n, k,
        a_km.stride(0), b_km.stride(0), b_km.stride(1), d.stride(0), int(use_psum_layout),
        runtime.get_mk_alignment_for_contiguous_layout(), current_stream_ptr()))


def m_grouped_bf16_gemm_nn_contiguous(a, b, d, grouped_layout, compiled_dims='nk', use_psum_layout=False, ensure_zero_padding=True,
                                      expected_m_for_psum_layout=None) -> None:
    """``b [G, K, N]``: a transposed view of the NT form."""
    m_grouped_bf16_gemm_nt_contiguous(a, b.transpose(1, 2), d, grouped_layout, compiled_dims, use_psum_layout, ensure_zero_padding,
                                      expected_m_for_psum_layout)


def m_grouped_bf16_gemm_nt_masked(a: torch.Tensor, b: torch.Tensor, d: torch.Tensor, masked_m: torch.Tensor, expected_m: int,
                                  compiled_dims: str = 'nk') -> None:
    """``a [G, M, K]``, ``b [G, N, K]``, ``d [G, M, N]`` BF16; only ``d[g, :masked_m[g]]`` is written; ``masked_m`` stays on the device,
    ``expected_m`` is a selection hint."""
    host_assert(a.dim() == 3 and b.dim() == 3 and a.stride(-1) == 1 and b.stride(-1) == 1,
                'major_a == cute::UMMA::Major::K and major_b == cute::UMMA::Major::K')
    host_assert(masked_m.is_contiguous(), 'masked_m.is_contiguous()')
    num_groups, m, k = _check_ab_bf16(a, 3)
    num_groups_, n, k_ = _check_ab_bf16(b, 3)
    host_assert(d.dim() == 3, 'd.dim() == 3')
    host_assert(num_groups == num_groups_ == d.size(0) == masked_m.numel(),
                'num_groups == num_groups_ and num_groups == num_groups__ and num_groups == num_groups___')
    host_assert((m, n) == tuple(d.shape[1:]) and k == k_, 'm == m_ and n == n_ and k == k_')
    host_assert(expected_m > 0 and m > 0 and n > 0 and k > 0 and num_groups > 0,
                'expected_m > 0 and m > 0 and n > 0 and k > 0 and num_groups > 0')
    host_assert(d.dtype == torch.bfloat16, 'd.scalar_type() == torch::kBFloat16')
    host_assert(masked_m.dtype == torch.int, 'masked_m.scalar_type() == torch::kInt')
    check_major_type_cd(d)
    _require_k_multiple_of_8(k)
    a_km, b_km = _k_major(a), _k_major(b)
    require_device(a, b, d, masked_m)
    check(lib.dg_m_grouped_bf16_gemm_nt_masked(
        a_km.data_ptr(), b_km.data_ptr(), d.data_ptr(), masked_m.data_ptr(), num_groups, m, n, k, int(expected_m),
        a_km.stride(0), a_km.stride(1), b_km.stride(0), b_km.stride(1), d.stride(0), d.stride(1), current_stream_ptr()))


# the reference's legacy name (deep_gemm/__init__.py)
bf16_m_grouped_gemm_nt_masked = m_grouped_bf16_gemm_nt_masked
