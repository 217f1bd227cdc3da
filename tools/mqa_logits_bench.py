#!/usr/bin/env python3
"""Times the MQA logits entries on the reference's shape lists (tests/test_attention.py enumerate_mqa_logits /
enumerate_paged_mqa_logits, FP8 operands) beside a chunked torch composition of the same arithmetic on the same GPU.

Per line: us, TFLOPS (2 * cost * H * D, cost = unmasked scores), score*head products per CU per cycle (the reference's "relu/cyc/SM",
at 2.4 GHz), GB/s, the fraction of the bound (dense: ~5 PF FP8 MFMA; paged: 8 TB/s HBM), the torch composition's us and, for the
paged lines, the time of get_paged_mqa_logits_metadata.  --quick: the dense lines at D = 128, H = 32 / 64 only (the paged list is the same).
    python tools/mqa_logits_bench.py [--quick] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepgemm_amd as dg                      # noqa: E402
from deepgemm_amd.testing.bench import bench   # noqa: E402

FP8_PEAK = 5.0e15
HBM_PEAK = 8.0e12
CLOCK = 2.4e9


def cast_rows(x):
    sf = x.abs().float().amax(dim=-1).clamp(1e-4) / 448.0
    return (x.float() / sf.unsqueeze(-1)).to(torch.float8_e4m3fn), sf


def torch_dense(q, kv, w, ks, ke):
    """The reference test's ref_fp8_mqa_logits: FP32 einsums over KV chunks of bounded score size."""
    s, h, _ = q.shape
    s_kv = kv.shape[0]
    qf, kf = q.float(), kv.float()
    chunk = max(1, (256 * 1024 * 1024) // max(1, s * h * 4))
    cols = torch.arange(s_kv, device='cuda')
    out = torch.empty(s, s_kv, device='cuda')
    for n0 in range(0, s_kv, chunk):
        sc = torch.einsum('mhd,nd->hmn', qf, kf[n0:n0 + chunk]).relu_()
        part = torch.einsum('hmn,mh->mn', sc, w)
        c = cols[n0:n0 + chunk]
        out[:, n0:n0 + chunk] = part.masked_fill_(~((c[None] >= ks[:, None]) & (c[None] < ke[:, None])), float('-inf'))
    return out


def torch_paged(q, kv_fp8, sf, w, ctx, table, block_kv, rows_per_chunk=32):
    b, n, h, d = q.shape
    out = torch.empty(b * n, table.shape[1] * block_kv, device='cuda')
    for b0 in range(0, b, rows_per_chunk):
        t = table[b0:b0 + rows_per_chunk].long()
        k = (kv_fp8[t].float() * sf[t].unsqueeze(-1)).flatten(1, 2)               # [rows, blocks * block_kv, d]
        sc = torch.einsum('bthd,bld->bthl', q[b0:b0 + rows_per_chunk].float(), k).relu_()
        out[b0 * n:(b0 + rows_per_chunk) * n] = torch.einsum('bthl,bth->btl', sc, w[b0 * n:(b0 + rows_per_chunk) * n].view(-1, n, h)).flatten(0, 1)
    return out


def dense_cases(quick):
    # enumerate_mqa_logits (FP8): seq_len in (2048, 8192), seq_len_kv in (8192, 65536), H in (8, 16, 32, 64), D in (32, 64, 128), CP or not
    for s, s_kv in ((2048, 8192), (2048, 65536), (8192, 65536)):
        for h in (8, 16, 32, 64):
            for d in (32, 64, 128):
                if quick and (d != 128 or h not in (32, 64)):
                    continue
                yield s, s_kv, h, d


def paged_cases(quick):
    # enumerate_paged_mqa_logits (FP8): B in (256, 4096), avg context in (8192, 65536) with B * avg <= 32 M, next_n in (1, 2) (SM90) and (1, 6) (SM100); H = 32 / 64, D = 128 here
    for b, avg in ((256, 8192), (256, 65536), (4096, 8192)):
        for n in (1, 2, 6):
            for h in (32, 64):
                for bkv in (32, 64):
                    yield b, n, h, 128, bkv, avg


def run_dense(s, s_kv, h, d, with_torch):
    q = torch.randn(s, h, d, device='cuda', dtype=torch.bfloat16)
    kv_fp8, sf = cast_rows(torch.randn(s_kv, d, device='cuda', dtype=torch.bfloat16))
    q_fp8 = q.to(torch.float8_e4m3fn)
    w = torch.randn(s, h, device='cuda')
    ks = torch.zeros(s, dtype=torch.int32, device='cuda')
    ke = torch.arange(s, dtype=torch.int32, device='cuda') + (s_kv - s)          # the non-CP generator
    cost = float((ke.clamp(0, s_kv) - ks.clamp(0, s_kv)).clamp(min=0).sum())
    t = bench(lambda: dg.fp8_mqa_logits(q_fp8, (kv_fp8, sf), w, ks, ke, clean_logits=True), num_warmups=3, num_tests=10)
    t_torch = bench(lambda: torch_dense(q_fp8, kv_fp8.float() * sf[:, None], w, ks, ke), num_warmups=1, num_tests=2) if with_torch else None
    heads = cost * h
    nbytes = q_fp8.numel() + kv_fp8.numel() + sf.numel() * 4 + w.numel() * 4 + s * s_kv * 4
    return dict(form='dense', S=s, S_kv=s_kv, H=h, D=d, us=t * 1e6, tflops=2 * heads * d / t / 1e12,
                per_cu_cycle=heads / (t * dg.get_num_sms() * CLOCK), gbs=nbytes / t / 1e9,
                bound_fraction=(2 * heads * d / t) / FP8_PEAK, torch_us=t_torch * 1e6 if t_torch else None)


def run_paged(b, n, h, d, bkv, avg, with_torch):
    lens = torch.randint(int(0.7 * avg), int(1.3 * avg), (b,), dtype=torch.int32)
    blocks = (lens + bkv - 1) // bkv
    used = int(blocks.sum())
    table = torch.zeros(b, int(blocks.max()), dtype=torch.int32)
    perm = torch.randperm(used, dtype=torch.int32)
    off = 0
    for i, nb in enumerate(blocks.tolist()):
        table[i, :nb] = perm[off:off + nb]
        off += nb
    table = table.cuda()
    kv_fp8, sf = cast_rows(torch.randn(used, bkv, d, device='cuda', dtype=torch.bfloat16))
    cache = torch.empty(used, bkv * (d + 4), dtype=torch.uint8, device='cuda')
    cache[:, :bkv * d] = kv_fp8.view(torch.uint8).view(used, -1)
    cache[:, bkv * d:] = sf.view(torch.uint8).view(used, -1)
    cache = cache.view(used, bkv, 1, d + 4)
    q_fp8 = torch.randn(b, n, h, d, device='cuda', dtype=torch.bfloat16).to(torch.float8_e4m3fn)
    w = torch.randn(b * n, h, device='cuda')
    ctx = lens.cuda().unsqueeze(1).repeat(1, n).contiguous()
    max_len = table.shape[1] * bkv
    meta = dg.get_paged_mqa_logits_metadata(ctx, bkv, dg.get_num_sms())
    t_meta = bench(lambda: dg.get_paged_mqa_logits_metadata(ctx, bkv, dg.get_num_sms()), num_warmups=3, num_tests=10)
    t = bench(lambda: dg.fp8_paged_mqa_logits(q_fp8, cache, w, ctx, table, meta, max_len), num_warmups=3, num_tests=10)
    t_torch = None
    if with_torch and b * avg <= 4 * 1024 * 1024:
        t_torch = bench(lambda: torch_paged(q_fp8, kv_fp8, sf, w, ctx, table, bkv), num_warmups=1, num_tests=1)
    total = float(lens.sum())
    heads = total * n * h
    nbytes = q_fp8.numel() + w.numel() * 4 + total * (d + 4) + total * n * 4
    return dict(form='paged', B=b, N=n, H=h, D=d, block_kv=bkv, avg=avg, us=t * 1e6, tflops=2 * heads * d / t / 1e12,
                per_cu_cycle=heads / (t * dg.get_num_sms() * CLOCK), gbs=nbytes / t / 1e9, bound_fraction=nbytes / t / HBM_PEAK, metadata_us=t_meta * 1e6,
                torch_us=t_torch * 1e6 if t_torch else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--json')
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    for c in dense_cases(args.quick):
        rows.append(run_dense(*c, not args.no_torch))
        r = rows[-1]
        print(f"dense S={r['S']:5d} S_kv={r['S_kv']:6d} H={r['H']:2d} D={r['D']:3d}: {r['us']:9.1f} us {r['tflops']:6.0f} TFLOPS "
              f"{r['per_cu_cycle']:5.1f} /CU/cyc {r['gbs']:6.0f} GB/s {100 * r['bound_fraction']:5.1f}% MFMA | torch "
              f"{r['torch_us'] or float('nan'):10.1f} us", flush=True)
        torch.cuda.empty_cache()
    for c in paged_cases(args.quick):
        rows.append(run_paged(*c, not args.no_torch))
        r = rows[-1]
        print(f"paged B={r['B']:4d} N={r['N']} H={r['H']:2d} D={r['D']:3d} bkv={r['block_kv']} L={r['avg']:5d}: {r['us']:9.1f} us "
              f"{r['tflops']:6.0f} TFLOPS {r['per_cu_cycle']:5.1f} /CU/cyc {r['gbs']:6.0f} GB/s {100 * r['bound_fraction']:5.1f}% HBM "
              f"| metadata {r['metadata_us']:6.1f} us | torch "
              f"{r['torch_us'] or float('nan'):10.1f} us", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
