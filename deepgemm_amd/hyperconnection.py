"""The hyper-connection pre-norm GEMM of the reference (``csrc/apis/hyperconnection.hpp``): ``tf32_hc_prenorm_gemm``.

The name, argument order, keywords and default follow the reference's binding (``register_apis``), and so does its contract, the SM90 one:
``n % 8 == 0``, ``n <= 32``, ``k % 64 == 0``, ``n, k > 0``.  Every argument is checked before any device work (``RuntimeError`` as the
reference's host asserts); the call launches on the current torch stream without synchronising and can be captured in a graph.
"""
from typing import Optional

import torch

from ._lib import lib, check, current_stream_ptr, require_device
from .errors import host_assert
from .gemm import _split_k_workspace

_BLOCK_K = 64


def tf32_hc_prenorm_gemm(a: torch.Tensor, b: torch.Tensor, d: torch.Tensor, sqr_sum: torch.Tensor,
                         num_splits: Optional[int] = None) -> None:
    """``d = a @ b.T`` and ``sqr_sum = (a * a).sum(-1)`` in one pass over ``a``, in FP32.

    ``a [m, k]`` BF16 and ``b [n, k]`` FP32, both K-major (``stride(1) == 1``, the row stride may exceed ``k``); ``d`` FP32 with
    ``stride(-1) == 1``; ``sqr_sum`` FP32 and contiguous.  With ``num_splits=None``, ``d`` is ``[m, n]`` and ``sqr_sum`` ``[m]``.  With
    ``num_splits=S``, ``d`` is ``[S, m, n]`` and ``sqr_sum`` ``[S, m]``, and split ``s`` holds the partial sums over the reference's K
    partition: K in blocks of 64, ``(k / 64) // S`` blocks per split and one more for the first ``(k / 64) % S`` splits; a split without
    blocks is zeros.  Every element of ``d`` and ``sqr_sum`` is written.

    gfx950 has no TF32 matrix instruction.  Each ``b`` is split into ``b_hi = bf16(b)`` and ``b_lo = bf16(b - b_hi)``, and both are
    multiplied with ``a`` on the BF16 MFMA, exactly, accumulating in FP32: the error of ``b_hi + b_lo`` is at most ``2^-16 |b|``, tighter
    than TF32.  Non-finite ``b`` is outside the contract: ``inf - inf`` in the split gives NaN.  Results are bitwise repeatable for a given
    shape and CU count (``set_num_sms``).  A ``num_splits=None`` call may cut K internally into the stream's split-K scratch buffer; a
    graph captured on a stream that has no buffer yet runs without the cut, so its bits can differ from an eager call's.
    """
    for name, t in (('a', a), ('b', b), ('d', d), ('sqr_sum', sqr_sum)):
        host_assert(isinstance(t, torch.Tensor), f'{name} is a torch.Tensor')
    host_assert(a.dim() == 2 and b.dim() == 2, 'a.dim() == 2 and b.dim() == 2')
    # A and B must be K-major, D must be N-major; S must be contiguous
    host_assert(a.stride(1) == 1, 'get_major_type_ab(a) == cute::UMMA::Major::K')
    host_assert(b.stride(1) == 1, 'get_major_type_ab(b) == cute::UMMA::Major::K')
    host_assert(d.dim() >= 1 and d.stride(-1) == 1, 'd.stride(-1) == 1')
    host_assert(sqr_sum.is_contiguous(), 'sqr_sum.is_contiguous()')
    m, k = a.shape
    n, k_ = b.shape
    if num_splits is not None:
        host_assert(isinstance(num_splits, int) and num_splits >= 1, 'num_splits.value() >= 1')
        host_assert(d.dim() == 3 and sqr_sum.dim() == 2, 'd.dim() == 3 and sqr_sum.dim() == 2')
        host_assert(d.size(0) == num_splits and sqr_sum.size(0) == num_splits,
                    'num_splits.value() == num_splits_ and num_splits.value() == num_splits__')
        host_assert(m == d.size(1) and m == sqr_sum.size(1) and n == d.size(2) and k == k_, 'm == m_ and m == m__ and n == n_ and k == k_')
    else:
        host_assert(d.dim() == 2 and sqr_sum.dim() == 1, 'd.dim() == 2 and sqr_sum.dim() == 1')
        host_assert(m == d.size(0) and m == sqr_sum.size(0) and n == d.size(1) and k == k_, 'm == m_ and m == m__ and n == n_ and k == k_')
    host_assert(n > 0 and k > 0, 'n > 0 and k > 0')
    host_assert(a.dtype == torch.bfloat16, 'a.scalar_type() == torch::kBFloat16')
    host_assert(b.dtype == torch.float, 'b.scalar_type() == torch::kFloat')
    host_assert(d.dtype == torch.float, 'd.scalar_type() == torch::kFloat')
    host_assert(sqr_sum.dtype == torch.float, 'sqr_sum.scalar_type() == torch::kFloat')
    # the SM90 kernel's limits (the SM100 form's n <= 128 is not provided)
    host_assert(n % 8 == 0 and n <= 32, 'n % 8 == 0 and n <= 32')
    host_assert(k % _BLOCK_K == 0, 'k % 64 == 0')
    if m == 0:
        return
    require_device(a, b, d, sqr_sum)
    # 16-byte aligned rows, as the reference's TMA descriptors need
    host_assert(a.data_ptr() % 16 == 0 and a.stride(0) % 8 == 0, 'a rows are 16-byte aligned')
    host_assert(b.data_ptr() % 16 == 0 and b.stride(0) % 4 == 0, 'b rows are 16-byte aligned')
    stream = current_stream_ptr()
    ws = _split_k_workspace(d.device, stream) if num_splits is None else None
    check(lib.dg_tf32_hc_prenorm_gemm(a.data_ptr(), b.data_ptr(), d.data_ptr(), sqr_sum.data_ptr(), m, n, k, a.stride(0), b.stride(0),
                                      d.stride(-2), d.stride(0) if num_splits is not None else 0, num_splits or 0,
                                      ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream))
