"""tf32_hc_prenorm_gemm on the GPU against an FP64 statement of the same inputs: the reference's grid (tests/test_hyperconnection.py),
per-split partials on the reference's K partition, every output element written, the precision of the B split, layouts and small sizes,
bitwise repeatability and graph capture."""
import pytest
import torch

import deepgemm_amd as dg
from deepgemm_amd.testing import calc_diff

pytestmark = pytest.mark.gpu

GRID_MN_K = [(24, 28672), (24, 7680), (24, 7168)]


def _inputs(m, n, k, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.randn((m, k), dtype=torch.float, device='cuda', generator=g).to(torch.bfloat16)
    b = torch.randn((n, k), dtype=torch.float, device='cuda', generator=g)
    return a, b


def _outputs(m, n, num_splits, fill=float('nan')):
    if num_splits is None:
        return torch.full((m, n), fill, device='cuda'), torch.full((m,), fill, device='cuda')
    return torch.full((num_splits, m, n), fill, device='cuda'), torch.full((num_splits, m), fill, device='cuda')


def _split_bounds(k, num_splits):
    """The reference's K partition (sm90_tf32_hc_prenorm_gemm.cuh k_offset), in elements."""
    kb = k // 64
    per, rem = kb // num_splits, kb % num_splits
    out = []
    for s in range(num_splits):
        start = s * per + min(s, rem)
        out.append((start * 64, (start + per + (1 if s < rem else 0)) * 64))
    return out


def _check_total(a, b, d, s):
    ref_d = a.double() @ b.double().T
    ref_s = a.double().square().sum(-1)
    assert not torch.isnan(d).any() and not torch.isnan(s).any()
    diff_d, diff_s = calc_diff(d, ref_d), calc_diff(s, ref_s)
    assert max(diff_d, diff_s) < 1e-8, (diff_d, diff_s)          # the reference's gate
    assert diff_d < 1e-9, diff_d                                 # plain BF16 B gives ~1e-6: this tells the hi/lo split apart
    assert ((s.double() - ref_s).abs() <= 2e-5 * ref_s).all()


@pytest.mark.parametrize('num_splits', [None, 16])
@pytest.mark.parametrize('n, k', GRID_MN_K)
@pytest.mark.parametrize('m', [13, 137, 4096, 8192])
def test_reference_grid(m, n, k, num_splits):
    a, b = _inputs(m, n, k)
    d, s = _outputs(m, n, num_splits)
    dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
    if num_splits is not None:
        d, s = d.sum(0), s.sum(0)
    _check_total(a, b, d, s)


@pytest.mark.parametrize('m, n, k, num_splits', [(137, 24, 7168, 16), (13, 32, 7680, 7), (64, 16, 1024, 3),
                                                 (40, 8, 256, 9), (300, 24, 192, 5), (5, 24, 64, 2)])
def test_per_split_partials(m, n, k, num_splits):
    """Each split against its own FP64 partial; num_splits > k / 64 leaves empty splits, which must be zeros."""
    a, b = _inputs(m, n, k, seed=1)
    d, s = _outputs(m, n, num_splits)
    dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
    for i, (k0, k1) in enumerate(_split_bounds(k, num_splits)):
        if k0 == k1:
            assert (d[i] == 0).all() and (s[i] == 0).all(), i
            continue
        ref_d = a[:, k0:k1].double() @ b[:, k0:k1].double().T
        ref_s = a[:, k0:k1].double().square().sum(-1)
        assert not torch.isnan(d[i]).any() and not torch.isnan(s[i]).any(), i
        assert calc_diff(d[i], ref_d) < 1e-9, i
        assert ((s[i].double() - ref_s).abs() <= 2e-5 * ref_s).all(), i


def test_precision_probe():
    """a = 1, b[j] = 1 + j 2^-12: bf16(b) loses the j term, the hi/lo split keeps it exactly."""
    m, n, k = 40, 32, 7168
    a = torch.ones((m, k), dtype=torch.bfloat16, device='cuda')
    col = 1 + torch.arange(n, dtype=torch.float, device='cuda') * 2.0 ** -12
    b = col[:, None].expand(n, k).contiguous()
    for num_splits in (None, 4):
        d, s = _outputs(m, n, num_splits)
        dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
        if num_splits is not None:
            d, s = d.sum(0), s.sum(0)
        assert torch.equal(d, (k * col)[None, :].expand(m, n))
        assert torch.equal(s, torch.full((m,), float(k), device='cuda'))


@pytest.mark.parametrize('n', [8, 16, 32])
@pytest.mark.parametrize('m', [1, 13, 137])
@pytest.mark.parametrize('k', [64, 1024])
@pytest.mark.parametrize('num_splits', [None, 2])
def test_small_sizes(m, n, k, num_splits):
    a, b = _inputs(m, n, k, seed=2)
    d, s = _outputs(m, n, num_splits)
    dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
    if num_splits is not None:
        d, s = d.sum(0), s.sum(0)
    _check_total(a, b, d, s)


@pytest.mark.parametrize('num_splits', [None, 3])
def test_strided_operands_and_padded_d(num_splits):
    """a and b as views into wider rows; d with padded row and split strides (non-contiguous)."""
    m, n, k = 200, 24, 1536
    wide_a, wide_b = _inputs(m, n, k + 128, seed=3)
    a, b = wide_a[:, 64:64 + k], wide_b[:, :k]
    assert not a.is_contiguous() and not b.is_contiguous()
    if num_splits is None:
        d_store = torch.full((m, n + 8), float('nan'), device='cuda')
        d = d_store[:, :n]
        s = torch.full((m,), float('nan'), device='cuda')
    else:
        d_store = torch.full((num_splits, m + 3, n + 2), float('nan'), device='cuda')       # (row stride not a multiple of 4)
        d = d_store[:, 1:m + 1, :n]
        s = torch.full((num_splits, m), float('nan'), device='cuda')
    assert not d.is_contiguous()
    dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
    outside = torch.ones_like(d_store, dtype=torch.bool)
    if num_splits is None:
        outside[:, :n] = False
    else:
        outside[:, 1:m + 1, :n] = False
    assert torch.isnan(d_store[outside]).all()          # nothing outside the view is touched
    _check_total(a, b, d if num_splits is None else d.sum(0), s if num_splits is None else s.sum(0))


def test_m_zero_launches_nothing():
    a = torch.zeros((0, 128), dtype=torch.bfloat16, device='cuda')
    b = torch.ones((24, 128), device='cuda')
    d, s = torch.full((0, 24), 1.0, device='cuda'), torch.full((0,), 1.0, device='cuda')
    dg.tf32_hc_prenorm_gemm(a, b, d, s)
    d3, s3 = torch.full((2, 0, 24), 1.0, device='cuda'), torch.full((2, 0), 1.0, device='cuda')
    dg.tf32_hc_prenorm_gemm(a, b, d3, s3, num_splits=2)
    torch.cuda.synchronize()


@pytest.mark.parametrize('m, k, num_splits', [(13, 28672, None), (8192, 7168, None), (4096, 7680, 16)])
def test_repeatable(m, k, num_splits):
    a, b = _inputs(m, 24, k, seed=4)
    d1, s1 = _outputs(m, 24, num_splits)
    d2, s2 = _outputs(m, 24, num_splits)
    dg.tf32_hc_prenorm_gemm(a, b, d1, s1, num_splits=num_splits)
    dg.tf32_hc_prenorm_gemm(a, b, d2, s2, num_splits=num_splits)
    assert torch.equal(d1, d2) and torch.equal(s1, s2)


@pytest.mark.parametrize('m, k, num_splits', [(137, 7168, None), (4096, 7680, None), (13, 28672, 16)])
def test_graph_capture(m, k, num_splits):
    a, b = _inputs(m, 24, k, seed=5)
    d_eager, s_eager = _outputs(m, 24, num_splits)
    d, s = _outputs(m, 24, num_splits)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        # eager on the capture stream first: it creates the stream's split-K scratch buffer, so the graph makes the same K cut
        dg.tf32_hc_prenorm_gemm(a, b, d_eager, s_eager, num_splits=num_splits)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dg.tf32_hc_prenorm_gemm(a, b, d, s, num_splits=num_splits)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d, d_eager) and torch.equal(s, s_eager)
