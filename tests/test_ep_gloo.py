"""Expert-parallel harness on CPU: world_size 2 over gloo, the local grouped GEMM replaced by the oracle (tests may use it
as the checker; the product path only ever calls the HIP operator).  Covers the N > 1 path of SURVEY.md section 8e:
expert sharding, count + payload all-to-all, masked-layout packing, combine ordering."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Every rank is a process that loads torch and with it the ROCm runtime.  A machine that shares its GPUs admits at most 6 such
# processes per GPU, the test runner included, so 8 ranks run only where no GPU is visible (the CPU test machines).
EIGHT_RANKS = pytest.mark.skipif(torch.cuda.is_available(), reason='8 rank processes exceed the 6 processes a shared GPU admits; runs without a GPU')


def _oracle_local_gemm(a, b, d, masked_m, expected_m):
    import oracle
    oracle.m_grouped_fp8_gemm_nt_masked(a[0], a[1], b[0], b[1], d, masked_m)


def _worker(rank: int, world: int, port: int, num_experts: int, tokens: int, top_k: int, n: int, k: int, max_m: int, fail_queue):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        import oracle
        from deepgemm_amd import ep
        from deepgemm_amd.utils.math import per_block_cast_to_fp8, per_token_cast_to_fp8

        torch.manual_seed(1234)                                   # same expert weights on every rank
        w = torch.randn((num_experts, n, k), dtype=torch.bfloat16)
        b_all = [per_block_cast_to_fp8(w[e], use_ue8m0=False) for e in range(num_experts)]
        first, last = ep.expert_range(num_experts, rank, world)
        b_local = (torch.stack([b_all[e][0] for e in range(first, last)]), torch.stack([b_all[e][1] for e in range(first, last)]))

        torch.manual_seed(100 + rank)                             # different tokens and routing per rank
        x = torch.randn((tokens + rank, k), dtype=torch.bfloat16)  # uneven token counts across ranks
        expert_ids = torch.stack([torch.randperm(num_experts)[:top_k] for _ in range(x.size(0))])
        xq = per_token_cast_to_fp8(x, use_ue8m0=False)

        out = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm)
        assert out.shape == (x.size(0), top_k, n) and out.dtype == torch.bfloat16

        # unsharded check: every (token, expert) pair computed directly against the full weight set
        for t in range(x.size(0)):
            for j in range(top_k):
                e = int(expert_ids[t, j])
                want = torch.empty((1, n), dtype=torch.bfloat16)
                oracle.fp8_gemm_nt(xq[0][t:t + 1], xq[1][t:t + 1], b_all[e][0], b_all[e][1], want)
                assert torch.equal(out[t, j], want[0]), (rank, t, j, e)

        # top-k weighted reduce on the token's owner: FP32 accumulation of the combined rows
        weights = torch.softmax(torch.randn((x.size(0), top_k)), dim=-1)
        reduced = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm,
                                                     topk_weights=weights)
        assert reduced.shape == (x.size(0), n) and reduced.dtype == torch.bfloat16
        assert torch.equal(reduced, (out.float() * weights.unsqueeze(-1)).sum(dim=1).to(torch.bfloat16))

        # the fixed-capacity exchange (no host synchronisation): same rows, same bits
        fixed = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm,
                                                   capacity=tokens + world)      # (the same on every rank)
        assert torch.equal(fixed, out)
        fixed_reduced = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm,
                                                           topk_weights=weights, capacity=tokens + world)
        assert torch.equal(fixed_reduced, reduced)
        (a_fixed, _), plan_fixed = ep.dispatch_fixed(xq, expert_ids, num_experts, max_m, 2)      # capacity 2: rows may be dropped
        assert a_fixed.shape[1] == max_m and a_fixed.is_contiguous()
        busiest = int(torch.bincount(expert_ids.reshape(-1), minlength=num_experts).max())
        flag_local = torch.tensor([int(busiest > 2)])
        assert bool(plan_fixed.overflow) or int(flag_local) == 0                 # my own over-full blocks are always reported

        # an expert over max_m on the RECEIVER: the rows that fitted come back right, the dropped ones as zeros (never another pair's row)
        small = 4
        to_zero = torch.zeros((x.size(0), 1), dtype=torch.int64)
        (a_small, sf_small), plan_small = ep.dispatch_fixed(xq, to_zero, num_experts, small, tokens + world)
        d_small = torch.zeros((last - first, small, n), dtype=torch.bfloat16)
        _oracle_local_gemm((a_small, sf_small), b_local, d_small, plan_small.masked_m, small)
        back = ep.combine_fixed(d_small, plan_small, x.size(0), 1, world, tokens + world)
        kept = small if rank == 0 else 0                                # slots go to the rows of earlier sources first
        for t in range(x.size(0)):
            want = torch.zeros((1, n), dtype=torch.bfloat16)
            if t < kept:
                oracle.fp8_gemm_nt(xq[0][t:t + 1], xq[1][t:t + 1], b_all[0][0], b_all[0][1], want)
            assert torch.equal(back[t, 0], want[0]), (rank, t)
        if rank == 0:
            assert bool(plan_small.overflow) and int(plan_small.masked_m[0]) == small

        # capacity overflow is an error, not silent truncation
        crowded = torch.zeros((max_m + 1, 1), dtype=torch.int64)  # every row to expert 0
        xs = per_token_cast_to_fp8(torch.randn((max_m + 1, k), dtype=torch.bfloat16), use_ue8m0=False)
        try:
            ep.dispatch(xs, crowded, num_experts, max_m)
            overflowed = False
        except RuntimeError:
            overflowed = True
        flag = torch.tensor([int(overflowed)])
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        assert int(flag) == 1                                     # the owner of expert 0 must have refused
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:                                      # noqa: BLE001
        fail_queue.put(f'rank {rank}: {type(exc).__name__}: {exc}')
        raise


@pytest.mark.parametrize('world,num_experts,top_k', [(2, 4, 2), (2, 8, 3)])
def test_ep_masked_gemm_world2(world, num_experts, top_k):
    ctx = mp.get_context('spawn')
    fail_queue = ctx.SimpleQueue()
    port = 29650 + num_experts
    procs = [ctx.Process(target=_worker, args=(r, world, port, num_experts, 11, top_k, 128, 256, 64, fail_queue))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    failures = []
    while not fail_queue.empty():
        failures.append(fail_queue.get())
    assert not failures, failures
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def _expert_weights(e: int, n: int, k: int):
    """Expert e's quantised weights, reproducible on any rank (the owner keeps them resident; a checker regenerates them)."""
    from deepgemm_amd.utils.math import per_block_cast_to_fp8
    g = torch.Generator().manual_seed(5000 + e)
    return per_block_cast_to_fp8(torch.randn((n, k), dtype=torch.bfloat16, generator=g), use_ue8m0=False)


def _worker_baseline_partition(rank: int, world: int, port: int, fail_queue):
    """BASELINE configs[4] as it is partitioned: 64 experts over 8 ranks (8 resident experts each, `expert_range(64, r, 8)`), top-8
    routing, the rank-local problem at its real shape N = 4096, K = 7168 (decode: a handful of rows per expert), both exchange forms."""
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        os.environ['OMP_NUM_THREADS'] = '1'
        torch.set_num_threads(1)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        import oracle
        from deepgemm_amd import ep
        from deepgemm_amd.utils.math import per_token_cast_to_fp8
        num_experts, top_k, n, k, max_m = 64, 8, 4096, 7168, 64
        first, last = ep.expert_range(num_experts, rank, world)
        assert (first, last) == (8 * rank, 8 * rank + 8)
        local = [_expert_weights(e, n, k) for e in range(first, last)]
        b_local = (torch.stack([q[0] for q in local]), torch.stack([q[1] for q in local]))
        del local
        torch.manual_seed(200 + rank)
        tokens = 3 + rank % 2                                       # uneven token counts across ranks
        xq = per_token_cast_to_fp8(torch.randn((tokens, k), dtype=torch.bfloat16), use_ue8m0=False)
        expert_ids = torch.stack([torch.randperm(num_experts)[:top_k] for _ in range(tokens)])
        weights = torch.softmax(torch.randn((tokens, top_k)), dim=-1)

        out = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm)
        assert out.shape == (tokens, top_k, n) and out.dtype == torch.bfloat16
        # unsharded check on sampled (token, expert) pairs -- local AND remote experts -- against regenerated weights
        checked_remote = 0
        for t, j in ((0, 0), (0, 5), (tokens - 1, 3), (tokens - 1, 7), (1, 2)):
            e = int(expert_ids[t, j])
            checked_remote += int(not first <= e < last)
            w_e = _expert_weights(e, n, k)
            want = torch.empty((1, n), dtype=torch.bfloat16)
            oracle.fp8_gemm_nt(xq[0][t:t + 1], xq[1][t:t + 1], w_e[0], w_e[1], want)
            assert torch.equal(out[t, j], want[0]), (rank, t, j, e)
        # the fixed-capacity exchange (no host synchronisation) and the top-k weighted reduce: same bits
        fixed = ep.ep_m_grouped_fp8_gemm_nt_masked(xq, expert_ids, b_local, num_experts, max_m, local_gemm=_oracle_local_gemm,
                                                   capacity=4, topk_weights=weights)
        assert torch.equal(fixed, (out.float() * weights.unsqueeze(-1)).sum(dim=1).to(torch.bfloat16))
        total_remote = torch.tensor([checked_remote])
        dist.all_reduce(total_remote)
        assert int(total_remote) > 0                                # the sample did cross ranks
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:                                        # noqa: BLE001
        fail_queue.put(f'rank {rank}: {type(exc).__name__}: {exc}')
        raise


@EIGHT_RANKS
def test_ep_masked_gemm_world8_baseline_partition():
    """The only multi-rank evidence obtainable without an 8-GPU node (SCALE is skipped on 1-GPU leases): the exact BASELINE split on
    8 gloo ranks with the oracle as the local GEMM.  The all-to-all terms remain UNMEASURED on hardware."""
    ctx = mp.get_context('spawn')
    fail_queue = ctx.SimpleQueue()
    world, port = 8, 29683
    procs = [ctx.Process(target=_worker_baseline_partition, args=(r, world, port, fail_queue)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    failures = []
    while not fail_queue.empty():
        failures.append(fail_queue.get())
    assert not failures, failures
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_expert_range():
    from deepgemm_amd import ep
    assert ep.expert_range(64, 0, 8) == (0, 8) and ep.expert_range(64, 7, 8) == (56, 64)
    with pytest.raises(RuntimeError):
        ep.expert_range(10, 0, 4)
