"""tf32_hc_prenorm_gemm surface without a GPU: the exported name, the reference's signature, every validation rule raising RuntimeError
before any device work, host tensors failing with the "no CPU path" message, and the K pieces the library picks."""
import inspect

import pytest
import torch

import deep_gemm
import deepgemm_amd as dg
from deepgemm_amd._lib import lib

E = inspect.Parameter.empty


def test_exported():
    assert callable(dg.tf32_hc_prenorm_gemm)
    assert deep_gemm.tf32_hc_prenorm_gemm is dg.tf32_hc_prenorm_gemm


def test_signature_follows_the_reference():
    params = [(p.name, p.default) for p in inspect.signature(dg.tf32_hc_prenorm_gemm).parameters.values()]
    assert params == [('a', E), ('b', E), ('d', E), ('sqr_sum', E), ('num_splits', None)]


def _args(m=16, n=24, k=128, num_splits=None):
    a = torch.zeros(m, k, dtype=torch.bfloat16)
    b = torch.zeros(n, k, dtype=torch.float)
    if num_splits is None:
        return dict(a=a, b=b, d=torch.zeros(m, n), sqr_sum=torch.zeros(m))
    return dict(a=a, b=b, d=torch.zeros(num_splits, m, n), sqr_sum=torch.zeros(num_splits, m), num_splits=num_splits)


def _raises(match=None, **kw):
    with pytest.raises(RuntimeError, match=match):
        dg.tf32_hc_prenorm_gemm(**kw)


def _with(base, **kw):
    out = dict(base)
    out.update(kw)
    return out


@pytest.mark.parametrize('num_splits', [None, 4])
def test_cpu_tensors_have_no_path(num_splits):
    _raises('no CPU path', **_args(num_splits=num_splits))


@pytest.mark.parametrize('field, dtype', [('a', torch.float), ('a', torch.float16), ('b', torch.bfloat16), ('b', torch.float64),
                                          ('d', torch.bfloat16), ('sqr_sum', torch.bfloat16)])
def test_dtypes(field, dtype):
    base = _args()
    _raises('Assertion error', **_with(base, **{field: base[field].to(dtype)}))


@pytest.mark.parametrize('n', [4, 12, 20, 40, 64, 128])
def test_n_rules(n):
    _raises('Assertion error', **_args(n=n))


@pytest.mark.parametrize('k', [32, 96, 100, 200])
def test_k_multiple_of_64(k):
    _raises('Assertion error', **_args(k=k))


def test_n_and_k_positive():
    _raises('Assertion error', **_args(n=0))
    _raises('Assertion error', **_args(k=0))


def test_k_major_operands():
    base = _args()
    _raises('Assertion error', **_with(base, a=torch.zeros(128, 16, dtype=torch.bfloat16).t()))
    _raises('Assertion error', **_with(base, b=torch.zeros(128, 24).t()))


def test_d_n_major():
    base = _args()
    _raises('Assertion error', **_with(base, d=torch.zeros(24, 16).t()))
    split = _args(num_splits=2)
    _raises('Assertion error', **_with(split, d=torch.zeros(2, 24, 16).transpose(1, 2)))


def test_sqr_sum_contiguous():
    _raises('Assertion error', **_with(_args(), sqr_sum=torch.zeros(32)[::2]))
    _raises('Assertion error', **_with(_args(num_splits=2), sqr_sum=torch.zeros(16, 2).t()))


@pytest.mark.parametrize('num_splits', [0, -1])
def test_num_splits_at_least_one(num_splits):
    base = _args(num_splits=1)
    _raises('Assertion error', **_with(base, num_splits=num_splits))


def test_shapes_follow_num_splits():
    plain, split = _args(), _args(num_splits=3)
    _raises('Assertion error', **_with(plain, num_splits=3))                        # 2-D d with num_splits
    _raises('Assertion error', **_with(split, num_splits=None))                     # 3-D d without
    _raises('Assertion error', **_with(split, num_splits=2))                        # leading dim != num_splits
    _raises('Assertion error', **_with(split, sqr_sum=torch.zeros(2, 16)))
    _raises('Assertion error', **_with(split, d=torch.zeros(3, 16, 16)))            # n mismatch
    _raises('Assertion error', **_with(split, d=torch.zeros(3, 8, 24)))             # m mismatch
    _raises('Assertion error', **_with(split, sqr_sum=torch.zeros(3, 8)))
    _raises('Assertion error', **_with(plain, d=torch.zeros(8, 24)))
    _raises('Assertion error', **_with(plain, sqr_sum=torch.zeros(8)))
    _raises('Assertion error', **_with(plain, sqr_sum=torch.zeros(16, 1)))
    _raises('Assertion error', **_with(plain, b=torch.zeros(24, 192)))              # k mismatch


def test_m_zero_returns_before_the_device():
    for num_splits in (None, 2):
        kw = _args(m=0, num_splits=num_splits)
        dg.tf32_hc_prenorm_gemm(**kw)           # no launch, no "no CPU path" error


def test_c_abi_checks_the_contract():
    for n, k in [(12, 128), (40, 128), (24, 96)]:
        assert lib.dg_tf32_hc_prenorm_gemm(None, None, None, None, 16, n, k, k, k, n, 0, 0, None, 0, None) != 0


def test_pieces():
    ws = int(lib.dg_split_k_workspace_bytes())
    # the caller's splits are the cut
    assert lib.dg_hc_prenorm_pieces(8192, 24, 28672, 16, ws) == 16
    # no workspace: no internal cut
    assert lib.dg_hc_prenorm_pieces(8192, 24, 28672, 0, 0) == 1
    # small m: K is cut (at least one 64-wide K block per wave and piece), large m over many row tiles as well
    for m, k in [(13, 7168), (137, 28672), (4096, 7680), (8192, 28672)]:
        pieces = lib.dg_hc_prenorm_pieces(m, 24, k, 0, ws)
        assert 1 < pieces <= k // 64 // 4, (m, k, pieces)
    # the partials must fit the workspace
    assert lib.dg_hc_prenorm_pieces(8192, 24, 28672, 0, 8192 * 25 * 4 * 2) <= 2
