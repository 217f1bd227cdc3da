"""BF16 GEMMs on the GPU through the public entries: the reference's tests/test_bf16.py sweeps (calc_diff < 1e-5 against the FP32
expression), ragged shapes against an FP64 CPU statement element by element, every bf16_* configuration forced by name, repeatability,
hipGraph replay, the M-grouped contiguous (both layouts) and masked forms."""
import pytest
import torch

import deepgemm_amd as dg
from deepgemm_amd.testing import calc_diff
from deepgemm_amd.testing import generators as gen

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _seed_and_auto():
    gen.reset_seed(0)
    yield
    dg.set_forced_config('auto')


def _call(a, b, d, c, a_k_major, b_k_major):
    fn = {(True, True): dg.bf16_gemm_nt, (True, False): dg.bf16_gemm_nn, (False, False): dg.bf16_gemm_tn,
          (False, True): dg.bf16_gemm_tt}[(a_k_major, b_k_major)]
    fn(a, b, d, c)


@pytest.mark.parametrize('case', list(gen.enumerate_bf16_normal()), ids=lambda c: '-'.join(str(x) for x in c))
def test_reference_sweep(case):
    m, n, k, a_k, b_k, acc, out = case
    t = gen.generate_bf16_normal(m, n, k, a_k, b_k, acc, out)
    _call(t.a, t.b, t.d, t.c, a_k, b_k)
    assert calc_diff(t.d, t.ref_d) < 1e-5, (case, dg.last_config())


def _fp64_check(d, a, b, c=None):
    """|d - ref| <= 0.5 ulp_d(|ref|) + k 2^-24 sum|a b| (+ |c| rounding): a, b [m, k] / [n, k] BF16 on any device."""
    a64, b64 = a.double().cpu(), b.double().cpu()
    ref = a64 @ b64.t()
    bound = a.shape[1] * 2.0 ** -24 * (a64.abs() @ b64.abs().t())
    if c is not None:
        ref = ref + c.double().cpu()
        bound = bound + c.double().cpu().abs() * 2.0 ** -24
    eps = 2.0 ** -8 if d.dtype == torch.bfloat16 else 2.0 ** -24
    bound = bound + 0.5 * eps * 2 * ref.abs() + 1e-30
    err = (d.double().cpu() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), f'{int(bad.sum())} elements off; worst {float((err - bound).max())}'


RAGGED = [(1, 72, 200), (37, 100, 8 + 64), (70, 136, 200), (129, 300, 8 + 64 * 5), (300, 520, 200), (257, 257, 8 + 64 * 3)]


@pytest.mark.parametrize('out', [torch.bfloat16, torch.float])
@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('mnk', RAGGED)
def test_ragged_against_fp64(mnk, acc, out):
    m, n, k = mnk
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((n, k), device='cuda', dtype=torch.bfloat16)
    d = (torch.randn((m, n), device='cuda') * 4).to(out)
    c0 = d.clone() if acc else None
    dg.bf16_gemm_nt(a, b, d, d if acc else None)
    _fp64_check(d, a, b, c0)


@pytest.mark.parametrize('mnk', [(64, 128, 512), (200, 264, 200), (16, 96, 8 + 64 * 9)])
@pytest.mark.parametrize('name', ['bf16_256x256', 'bf16_128x256', 'bf16_stream_64x32', 'bf16_stream_ks_64x32'])
def test_forced_configs(name, mnk):
    m, n, k = mnk
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((n, k), device='cuda', dtype=torch.bfloat16)
    for out in (torch.bfloat16, torch.float):
        d = torch.empty((m, n), device='cuda', dtype=out)
        dg.set_forced_config(name)
        dg.bf16_gemm_nt(a, b, d)
        assert dg.last_config() == name
        dg.set_forced_config('auto')
        _fp64_check(d, a, b)


@pytest.mark.parametrize('mnk', [(1, 4096, 7168), (64, 2112, 7168), (4096, 4096, 7168), (300, 520, 200)])
def test_repeatable(mnk):
    m, n, k = mnk
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((n, k), device='cuda', dtype=torch.bfloat16)
    d0 = torch.empty((m, n), device='cuda', dtype=torch.bfloat16)
    d1 = torch.full((m, n), float('nan'), device='cuda', dtype=torch.bfloat16)
    dg.bf16_gemm_nt(a, b, d0)
    dg.bf16_gemm_nt(a, b, d1)
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))


def test_c_not_d_and_strided_d():
    m, n, k = 130, 200, 264
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((n, k), device='cuda', dtype=torch.bfloat16)
    for out in (torch.bfloat16, torch.float):
        c = torch.randn((m, n), device='cuda').to(out)
        d = torch.empty((m, n), device='cuda', dtype=out)
        dg.bf16_gemm_nt(a, b, d, c)
        _fp64_check(d, a, b, c)
        wide = torch.full((m, n + 24), 7.0, device='cuda', dtype=out)
        dv = wide[:, :n]
        dg.bf16_gemm_nt(a, b, dv)
        _fp64_check(dv, a, b)
        assert bool((wide[:, n:] == 7.0).all())


def test_hipgraph_replay_m1():
    m, n, k = 1, 4096, 7168
    a = torch.randn((m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((n, k), device='cuda', dtype=torch.bfloat16)
    eager = torch.empty((m, n), device='cuda', dtype=torch.bfloat16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dg.bf16_gemm_nt(a, b, eager)            # (warm-up on the capture stream: its K-split workspace exists before the capture)
    torch.cuda.current_stream().wait_stream(s)
    out = torch.zeros((m, n), device='cuda', dtype=torch.bfloat16)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dg.bf16_gemm_nt(a, b, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16))


@pytest.mark.parametrize('case', list(gen.enumerate_bf16_m_grouped_contiguous()), ids=lambda c: '-'.join(str(x) for x in c))
def test_m_grouped_contiguous(case):
    groups, expected, n, k, b_k_major, psum = case
    t = gen.generate_bf16_m_grouped_contiguous(groups, expected, n, k, b_k_major, psum)
    t.d.fill_(float('nan'))
    fn = dg.m_grouped_bf16_gemm_nt_contiguous if b_k_major else dg.m_grouped_bf16_gemm_nn_contiguous
    fn(t.a, t.b, t.d, t.layout, use_psum_layout=psum)
    for g, start, end in t.group_rows:
        assert calc_diff(t.d[start:end], t.ref_d[start:end]) < 1e-5, (g, dg.last_config())
    # padding rows (-1 in the per-row layout; the gaps up to the next aligned start in the psum layout) come out as exact zeros
    last_end = t.group_rows[-1][2]
    pad = torch.ones(t.m, dtype=torch.bool, device='cuda')
    for _, start, end in t.group_rows:
        pad[start:end] = False
    pad[last_end:] = False if psum else pad[last_end:]
    assert bool((t.d[pad] == 0).all())


@pytest.mark.parametrize('case', list(gen.enumerate_bf16_m_grouped_masked()), ids=lambda c: '-'.join(str(x) for x in c))
def test_m_grouped_masked(case):
    groups, max_m, expected, n, k = case
    ms = [min(max_m, int(expected * f)) for f in ([0.7, 1.3] * groups)[:groups]]
    ms[0], ms[-1] = 0, max_m
    t = gen.generate_bf16_m_grouped_masked(groups, max_m, expected, n, k, masked_ms=ms)
    t.d.fill_(float('nan'))
    dg.m_grouped_bf16_gemm_nt_masked(t.a, t.b, t.d, t.masked_m, expected)
    for g, rows in enumerate(ms):
        if rows:
            assert calc_diff(t.d[g, :rows], t.ref_d[g, :rows]) < 1e-5, (g, dg.last_config())
        assert bool(torch.isnan(t.d[g, rows:]).all())


def test_legacy_masked_alias_ragged():
    groups, max_m, n, k = 3, 100, 72, 200
    a = torch.randn((groups, max_m, k), device='cuda', dtype=torch.bfloat16)
    b = torch.randn((groups, n, k), device='cuda', dtype=torch.bfloat16)
    d = torch.full((groups, max_m, n), float('nan'), device='cuda', dtype=torch.bfloat16)
    ms = [5, 0, 100]
    dg.bf16_m_grouped_gemm_nt_masked(a, b, d, torch.tensor(ms, dtype=torch.int32, device='cuda'), 40)
    for g, rows in enumerate(ms):
        if rows:
            _fp64_check(d[g, :rows], a[g, :rows], b[g])
        assert bool(torch.isnan(d[g, rows:]).all())
