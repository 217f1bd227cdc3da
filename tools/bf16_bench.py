#!/usr/bin/env python3
"""Times every BF16 entry on the reference's BF16 shape lists (tests/test_bf16.py) with HIP events, weights cold: each timed call reads
the next of a rotation of weight copies larger than the 256 MiB Infinity Cache.  Prints us, TFLOPS, the fraction of the 2.5 PF BF16 dense
peak and of 8 TB/s (bytes of A, B and D once), and torch.matmul (hipBLASLt) on the same shapes.   python tools/bf16_bench.py [--quick]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepgemm_amd as dg                         # noqa: E402
from deepgemm_amd.testing import generators as gen  # noqa: E402

PEAK_FLOPS, PEAK_BYTES, CACHE_BYTES = 2.5e15, 8e12, 256 << 20


def _rotation(make, bytes_each):
    return [make() for _ in range(max(2, -(-2 * CACHE_BYTES // max(bytes_each, 1)) + 1))]


def _time(fn, bs, iters=20):
    for i in range(3):
        fn(bs[i % len(bs)])
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(bs[i % len(bs)])
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def _row(label, us, flops, nbytes, us_ref):
    print(f'{label:44s} {us:9.1f} us {flops / us * 1e-6:8.1f} TFLOPS {flops / us * 1e6 / PEAK_FLOPS:5.2f} of 2.5 PF '
          f'{nbytes / us * 1e6 / PEAK_BYTES:5.2f} of 8 TB/s | torch.matmul {us_ref:9.1f} us', flush=True)


def dense(m, n, k, out=torch.bfloat16):
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    bs = _rotation(lambda: torch.randn((n, k), device='cuda', dtype=torch.bfloat16), n * k * 2)
    d = torch.empty((m, n), device='cuda', dtype=out)
    us = _time(lambda b: dg.bf16_gemm_nt(a, b, d), bs)
    cfg = dg.last_config()
    us_ref = _time(lambda b: torch.matmul(a, b.t(), out=d) if out == torch.bfloat16 else torch.matmul(a, b.t()), bs)
    _row(f'nt {m} x {n} x {k} {str(out)[6:]} [{cfg}]', us, 2 * m * n * k, (m * k + n * k) * 2 + m * n * d.element_size(), us_ref)


def contiguous(groups, expected, n, k):
    t = gen.generate_bf16_m_grouped_contiguous(groups, expected, n, k)
    bs = _rotation(lambda: torch.randn((groups, n, k), device='cuda', dtype=torch.bfloat16), groups * n * k * 2)
    us = _time(lambda b: dg.m_grouped_bf16_gemm_nt_contiguous(t.a, b, t.d, t.layout), bs)
    cfg = dg.last_config()
    rows = [(s, e, g) for g, s, e in t.group_rows]
    us_ref = _time(lambda b: [torch.matmul(t.a[s:e], b[g].t()) for s, e, g in rows], bs)
    valid = sum(e - s for s, e, _ in rows)
    _row(f'contiguous {groups} x {expected} x {n} x {k} [{cfg}]', us, 2 * valid * n * k, (t.m * k + groups * n * k + t.m * n) * 2, us_ref)


def masked(groups, expected, n, k, max_m=4096):
    t = gen.generate_bf16_m_grouped_masked(groups, max_m, expected, n, k)
    bs = _rotation(lambda: torch.randn((groups, n, k), device='cuda', dtype=torch.bfloat16), groups * n * k * 2)
    us = _time(lambda b: dg.m_grouped_bf16_gemm_nt_masked(t.a, b, t.d, t.masked_m, expected), bs)
    cfg = dg.last_config()
    ms = t.masked_m.tolist()
    us_ref = _time(lambda b: torch.bmm(t.a[:, :expected], b.transpose(1, 2)), bs)
    valid = sum(ms)
    _row(f'masked {groups} x {expected} x {n} x {k} [{cfg}]', us, 2 * valid * n * k, (valid * k + groups * n * k + valid * n) * 2, us_ref)


def main():
    gen.reset_seed(0)
    quick = '--quick' in sys.argv
    for m, n, k in ((4096, 4096, 7168), (1, 4096, 7168), (128, 4096, 7168)):
        dense(m, n, k)
    if not quick:
        for m in (1, 128, 4096):
            for n, k in gen.DENSE_NK:
                dense(m, n, k)
            for n, k in gen.BF16_FP32_OUTPUT_NK:
                if m * n < (1 << 28):
                    dense(m, n, k, torch.float)
    contiguous(8, 4096, 4096, 7168)
    masked(32, 192, 4096, 7168)
    if not quick:
        for groups, expected in gen.CONTIGUOUS_GROUPS:
            for n, k in gen.GROUPED_NK:
                contiguous(groups, expected, n, k)
        for groups, expected in gen.MASKED_GROUPS:
            for n, k in gen.GROUPED_NK:
                masked(groups, expected, n, k)


if __name__ == '__main__':
    main()
