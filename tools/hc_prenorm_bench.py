#!/usr/bin/env python3
"""Times tf32_hc_prenorm_gemm on the reference's grid (tests/test_hyperconnection.py) beside the torch composition of the same result on
the same GPU (`a.float() @ b.T` plus `a.float().square().sum(-1)`).

Per line: us per call (all launches of the call included; a long kernel is queued first so the host does not limit the short ones), the
bytes of a, b, d and sqr_sum (the reference's count_bytes) per second, their share of 8 TB/s, the K pieces of the launch and the torch
composition's us.
    python tools/hc_prenorm_bench.py [--no-torch] [--json [out.json]]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepgemm_amd as dg                      # noqa: E402
from deepgemm_amd._lib import lib              # noqa: E402
from deepgemm_amd.testing.bench import bench   # noqa: E402

HBM_PEAK = 8.0e12
GRID_M = (13, 137, 4096, 8192)
GRID_NK = ((24, 28672), (24, 7680), (24, 7168))
GRID_SPLITS = (None, 16)


def run(m, n, k, num_splits, with_torch):
    a = torch.randn((m, k), dtype=torch.bfloat16, device='cuda')
    b = torch.randn((n, k), dtype=torch.float, device='cuda')
    d = torch.empty((m, n) if num_splits is None else (num_splits, m, n), dtype=torch.float, device='cuda')
    s = torch.empty((m,) if num_splits is None else (num_splits, m), dtype=torch.float, device='cuda')
    t = bench(lambda: dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits), num_warmups=3, num_tests=20, high_precision=True)
    t_torch = None
    if with_torch:
        t_torch = bench(lambda: (a.float() @ b.T, a.float().square().sum(-1)), num_warmups=2, num_tests=5, high_precision=True)
    nbytes = sum(x.numel() * x.element_size() for x in (a, b, d, s))
    pieces = lib.dg_hc_prenorm_pieces(m, n, k, num_splits or 0, int(lib.dg_split_k_workspace_bytes()))
    return dict(m=m, n=n, k=k, num_splits=num_splits, pieces=pieces, us=t * 1e6, gbs=nbytes / t / 1e9, hbm_fraction=nbytes / t / HBM_PEAK,
                torch_us=t_torch * 1e6 if t_torch else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--json', nargs='?', const='-', help='write the rows as JSON to this file ("-" or no value: stdout)')
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    for m in GRID_M:
        for n, k in GRID_NK:
            for num_splits in GRID_SPLITS:
                r = run(m, n, k, num_splits, not args.no_torch)
                rows.append(r)
                print(f"m={m:5d} n={n:2d} k={k:5d} num_splits={num_splits or 0:2d}: {r['us']:8.1f} us {r['gbs']:7.0f} GB/s "
                      f"{100 * r['hbm_fraction']:5.1f}% of 8 TB/s (pieces {r['pieces']:3d}) | torch {r['torch_us'] or float('nan'):8.1f} us",
                      file=sys.stderr if args.json == '-' else sys.stdout, flush=True)
                torch.cuda.empty_cache()
    if args.json == '-':
        print(json.dumps(rows))
    elif args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
