"""BF16 GEMM surface without a GPU: exported names and the reference's defaults, validation errors raised before any launch, the
trivial-shape early returns, and the kernel the selection picks at representative shapes (dg_bf16_select_config, nothing launched)."""
import inspect

import pytest
import torch

import deep_gemm
import deepgemm_amd as dg
from deepgemm_amd._lib import lib

NAMES = ['bf16_gemm_nt', 'bf16_gemm_nn', 'bf16_gemm_tn', 'bf16_gemm_tt', 'm_grouped_bf16_gemm_nt_contiguous',
         'm_grouped_bf16_gemm_nn_contiguous', 'm_grouped_bf16_gemm_nt_masked', 'bf16_m_grouped_gemm_nt_masked']


@pytest.mark.parametrize('name', NAMES)
def test_exported(name):
    assert callable(getattr(dg, name)) and getattr(deep_gemm, name) is getattr(dg, name)


def _defaults(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_follow_the_reference():
    e = inspect.Parameter.empty
    assert _defaults(dg.bf16_gemm_nt) == [('a', e), ('b', e), ('d', e), ('c', None), ('compiled_dims', 'nk')]
    assert _defaults(dg.bf16_gemm_nn) == [('a', e), ('b', e), ('d', e), ('c', None), ('compiled_dims', 'nk')]
    assert _defaults(dg.bf16_gemm_tn) == [('a', e), ('b', e), ('d', e), ('c', None), ('compiled_dims', 'mn')]
    assert _defaults(dg.bf16_gemm_tt) == [('a', e), ('b', e), ('d', e), ('c', None), ('compiled_dims', 'mn')]
    for fn in (dg.m_grouped_bf16_gemm_nt_contiguous, dg.m_grouped_bf16_gemm_nn_contiguous):
        assert _defaults(fn) == [('a', e), ('b', e), ('d', e), ('grouped_layout', e), ('compiled_dims', 'nk'), ('use_psum_layout', False),
                                 ('ensure_zero_padding', True), ('expected_m_for_psum_layout', None)]
    assert _defaults(dg.m_grouped_bf16_gemm_nt_masked) == [('a', e), ('b', e), ('d', e), ('masked_m', e), ('expected_m', e),
                                                           ('compiled_dims', 'nk')]
    assert dg.bf16_m_grouped_gemm_nt_masked is dg.m_grouped_bf16_gemm_nt_masked


def _bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


@pytest.mark.parametrize('bad', ['a_dtype', 'b_dtype', 'd_dtype', 'shape', 'd_major', 'cd_dtype', 'k8', 'row_stride'])
def test_dense_validation(bad):
    m, n, k = 4, 8, 64
    a, b, d, c = _bf(m, k), _bf(n, k), _bf(m, n), None
    if bad == 'a_dtype':
        a = a.float()
    elif bad == 'b_dtype':
        b = b.to(torch.float8_e4m3fn)
    elif bad == 'd_dtype':
        d = d.half()
    elif bad == 'shape':
        b = _bf(n, k + 8)
    elif bad == 'd_major':
        d = _bf(n, m).t()
    elif bad == 'cd_dtype':
        c = torch.zeros((m, n))
    elif bad == 'k8':
        a, b = _bf(m, 60), _bf(n, 60)
    elif bad == 'row_stride':
        a = _bf(m, k + 4)[:, :k]
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.bf16_gemm_nt(a, b, d, c)


def test_grouped_validation():
    a, b, d = _bf(256, 64), _bf(2, 32, 64), _bf(256, 32)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_contiguous(a, b, d, torch.zeros(256, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_contiguous(a, b, d, torch.zeros(255, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_contiguous(a, b, d, torch.zeros(3, dtype=torch.int32), use_psum_layout=True)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_contiguous(a, b, d.float(), torch.zeros(256, dtype=torch.int32))
    a3, d3 = _bf(2, 16, 64), _bf(2, 16, 32)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_masked(a3, b, d3, torch.zeros(2, dtype=torch.int64), 8)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_masked(a3, b, d3, torch.zeros(3, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.m_grouped_bf16_gemm_nt_masked(a3.float(), b, d3, torch.zeros(2, dtype=torch.int32), 8)


def test_early_returns():
    # m == 0 / n == 0: nothing; k == 0: D = C (c is not d) or zeros; no kernel, so CPU tensors pass
    dg.bf16_gemm_nt(_bf(0, 64), _bf(8, 64), _bf(0, 8))
    dg.bf16_gemm_nt(_bf(4, 64), _bf(0, 64), _bf(4, 0))
    d = torch.full((4, 8), 3.0, dtype=torch.bfloat16)
    dg.bf16_gemm_nt(_bf(4, 0), _bf(8, 0), d)
    assert bool((d == 0).all())
    c = torch.full((4, 8), 2.0)
    d = torch.full((4, 8), 5.0)
    dg.bf16_gemm_nt(_bf(4, 0), _bf(8, 0), d, c)
    assert bool((d == 2.0).all())
    d = torch.full((4, 8), 5.0)
    dg.bf16_gemm_nt(_bf(4, 0), _bf(8, 0), d, d)
    assert bool((d == 5.0).all())


def _pick(gemm_type, m, n=4096, k=7168, groups=1, expected_m=0, alignment=0, ws=1):
    return lib.dg_bf16_select_config(gemm_type, m, n, k, groups, expected_m, alignment, ws).decode()


@pytest.mark.parametrize('cus', [0, 64])
def test_selection_pins(cus):
    lib.dg_set_num_cus(cus)
    try:
        small = 'bf16_stream_ks_64x32' if cus == 0 else 'bf16_stream_64x32'      # (64 CUs: 128 tiles of 64 x 32 already fill the chip)
        assert _pick(0, 1) == small
        assert _pick(0, 64) == small
        assert _pick(0, 1, ws=0) == 'bf16_stream_64x32'
        assert _pick(0, 128) == 'bf16_256x256'
        assert _pick(0, 4096) == 'bf16_256x256'
        assert _pick(3, 4096, groups=32, expected_m=20) == 'bf16_stream_64x32'
        assert _pick(3, 4096, groups=32, expected_m=192) == 'bf16_256x256'
        assert _pick(1, 8192, groups=8, alignment=128) == 'bf16_256x256'
        assert _pick(2, 8192, groups=8, alignment=128) == 'bf16_128x256'
        assert _pick(1, 8192, groups=8, alignment=64) == 'bf16_stream_64x32'
    finally:
        lib.dg_set_num_cus(0)


def test_forced_names_are_per_family():
    names = dg.list_configs()
    bf16 = [x for x in names if x.startswith('bf16_')]
    assert bf16 == ['bf16_256x256', 'bf16_128x256', 'bf16_stream_64x32', 'bf16_stream_ks_64x32']
    try:
        dg.set_forced_config('bf16_128x256')
        assert lib.dg_get_forced_config() == b'bf16_128x256'
        # the FP8 selection does not see a BF16 name
        assert lib.dg_select_config(0, 4096, 4096, 7168, 1, 0, 0, 0, 128, 0, 0, 0) != b''
    finally:
        dg.set_forced_config('auto')
