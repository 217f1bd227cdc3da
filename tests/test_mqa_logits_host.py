"""MQA logits surface without a GPU: exported names, the reference's keyword names and defaults, and every validation rule raising
RuntimeError before any device work; host tensors fail with the "no CPU path" message."""
import inspect

import pytest
import torch

import deep_gemm
import deepgemm_amd as dg

NAMES = ['fp8_fp4_mqa_logits', 'fp8_mqa_logits', 'get_paged_mqa_logits_metadata', 'fp8_fp4_paged_mqa_logits', 'fp8_paged_mqa_logits']
E = inspect.Parameter.empty


@pytest.mark.parametrize('name', NAMES)
def test_exported(name):
    assert callable(getattr(dg, name)) and getattr(deep_gemm, name) is getattr(dg, name)


def _defaults(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_follow_the_reference():
    dense = [('q', E), ('kv', E), ('weights', E), ('cu_seq_len_k_start', E), ('cu_seq_len_k_end', E), ('clean_logits', True),
             ('max_seqlen_k', 0)]
    assert _defaults(dg.fp8_fp4_mqa_logits) == dense + [('logits_dtype', torch.float32)]
    assert _defaults(dg.fp8_mqa_logits) == dense
    assert _defaults(dg.get_paged_mqa_logits_metadata) == [('context_lens', E), ('block_kv', E), ('num_sms', E), ('indices', None)]
    paged = [('q', E), ('kv_cache', E), ('weights', E), ('context_lens', E), ('block_table', E), ('schedule_meta', E),
             ('max_context_len', E), ('clean_logits', False)]
    assert _defaults(dg.fp8_fp4_paged_mqa_logits) == paged + [('logits_dtype', torch.float32), ('indices', None)]
    assert _defaults(dg.fp8_paged_mqa_logits) == paged + [('indices', None)]


def _dense(s=4, s_kv=40, h=32, d=64):
    return dict(q=(torch.zeros(s, h, d, dtype=torch.float8_e4m3fn), None),
                kv=(torch.zeros(s_kv, d, dtype=torch.float8_e4m3fn), torch.ones(s_kv)),
                weights=torch.zeros(s, h), cu_seq_len_k_start=torch.zeros(s, dtype=torch.int32),
                cu_seq_len_k_end=torch.full((s,), s_kv, dtype=torch.int32))


DENSE_BAD = {
    'heads': lambda a: a.update(q=(torch.zeros(4, 12, 64, dtype=torch.float8_e4m3fn), None), weights=torch.zeros(4, 12)),
    'head_dim': lambda a: a.update(q=(torch.zeros(4, 32, 96, dtype=torch.float8_e4m3fn), None),
                                   kv=(torch.zeros(40, 96, dtype=torch.float8_e4m3fn), torch.ones(40))),
    'q_dtype': lambda a: a.update(q=(torch.zeros(4, 32, 64, dtype=torch.bfloat16), None)),
    'q_noncontiguous': lambda a: a.update(q=(torch.zeros(4, 64, 32, dtype=torch.float8_e4m3fn).transpose(1, 2), None)),
    'fp4': lambda a: a.update(q=(a['q'][0], torch.zeros(4, 32, dtype=torch.int32))),
    'kv_dtype': lambda a: a.update(kv=(torch.zeros(40, 64, dtype=torch.bfloat16), torch.ones(40))),
    'kv_sf_length': lambda a: a.update(kv=(a['kv'][0], torch.ones(39))),
    'kv_sf_dtype': lambda a: a.update(kv=(a['kv'][0], torch.ones(40, dtype=torch.float64))),
    'weights_shape': lambda a: a.update(weights=torch.zeros(4, 16)),
    'weights_dtype': lambda a: a.update(weights=torch.zeros(4, 32, dtype=torch.float16)),
    'bf16_weights_fp32_logits': lambda a: a.update(weights=torch.zeros(4, 32, dtype=torch.bfloat16)),
    'weights_stride': lambda a: a.update(weights=torch.zeros(32, 4).t()),
    'ks_dtype': lambda a: a.update(cu_seq_len_k_start=torch.zeros(4, dtype=torch.int64)),
    'ke_length': lambda a: a.update(cu_seq_len_k_end=torch.zeros(5, dtype=torch.int32)),
    'clean_with_max_seqlen_k': lambda a: a.update(clean_logits=True, max_seqlen_k=16),
    'logits_dtype': lambda a: a.update(logits_dtype=torch.float16),
}


@pytest.mark.parametrize('bad', sorted(DENSE_BAD))
def test_dense_validation(bad):
    args = _dense()
    DENSE_BAD[bad](args)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.fp8_fp4_mqa_logits(**args)


def test_fp4_message_and_legacy_entry():
    args = _dense()
    args['q'] = (args['q'][0], torch.zeros(4, 32, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='FP4 is not supported'):
        dg.fp8_fp4_mqa_logits(**args)
    args = _dense()
    args['q'] = torch.zeros(4, 32, 63, dtype=torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match='head_dim'):
        dg.fp8_mqa_logits(**args)


def test_host_tensors_have_no_cpu_path():
    with pytest.raises(RuntimeError, match='no CPU path'):
        dg.fp8_fp4_mqa_logits(**_dense())
    with pytest.raises(RuntimeError, match='no CPU path'):
        dg.get_paged_mqa_logits_metadata(torch.ones(2, 1, dtype=torch.int32), 64, dg.get_num_sms())
    with pytest.raises(RuntimeError, match='no CPU path'):
        dg.fp8_fp4_paged_mqa_logits(**_paged())


def _paged(b=2, n=1, h=32, d=128, block_kv=64, blocks=4, num_sms=None):
    num_sms = dg.get_num_sms() if num_sms is None else num_sms
    return dict(q=(torch.zeros(b, n, h, d, dtype=torch.float8_e4m3fn), None),
                kv_cache=torch.zeros(blocks, block_kv, 1, d + 4, dtype=torch.uint8), weights=torch.zeros(b * n, h),
                context_lens=torch.ones(b, n, dtype=torch.int32), block_table=torch.zeros(b, 2, dtype=torch.int32),
                schedule_meta=torch.zeros(num_sms + 1, 2, dtype=torch.int32), max_context_len=128)


PAGED_BAD = {
    'heads': lambda a: a.update(q=(torch.zeros(2, 1, 24, 128, dtype=torch.float8_e4m3fn), None), weights=torch.zeros(2, 24)),
    'head_dim': lambda a: a.update(q=(torch.zeros(2, 1, 32, 256, dtype=torch.float8_e4m3fn), None)),
    'q_dtype': lambda a: a.update(q=(torch.zeros(2, 1, 32, 128, dtype=torch.bfloat16), None)),
    'q_noncontiguous': lambda a: a.update(q=(torch.zeros(2, 1, 128, 32, dtype=torch.float8_e4m3fn).transpose(2, 3), None)),
    'fp4': lambda a: a.update(q=(a['q'][0], torch.zeros(2, 1, 32, dtype=torch.int32))),
    'block_kv_128': lambda a: a.update(kv_cache=torch.zeros(4, 128, 1, 132, dtype=torch.uint8)),
    'cache_row_bytes': lambda a: a.update(kv_cache=torch.zeros(4, 64, 1, 128, dtype=torch.uint8)),
    'cache_dtype': lambda a: a.update(kv_cache=torch.zeros(4, 64, 1, 132, dtype=torch.int8)),
    'cache_stride0': lambda a: a.update(kv_cache=torch.zeros(4 * 64 * 132 + 8, dtype=torch.uint8).as_strided((4, 64, 1, 132), (64 * 132 + 2, 132, 132, 1))),
    'weights_shape': lambda a: a.update(weights=torch.zeros(3, 32)),
    'context_lens_1d': lambda a: a.update(context_lens=torch.ones(2, dtype=torch.int32)),
    'context_lens_dtype': lambda a: a.update(context_lens=torch.ones(2, 1, dtype=torch.int64)),
    'block_table_stride': lambda a: a.update(block_table=torch.zeros(2, 2, dtype=torch.int32).t()),
    'block_table_dtype': lambda a: a.update(block_table=torch.zeros(2, 2, dtype=torch.int64)),
    'schedule_rows': lambda a: a.update(schedule_meta=torch.zeros(dg.get_num_sms() // 2 + 1, 2, dtype=torch.int32)),
    'clean_logits': lambda a: a.update(clean_logits=True),
    'indices': lambda a: a.update(indices=torch.zeros(2, dtype=torch.int32)),
    'logits_dtype': lambda a: a.update(logits_dtype=torch.float16),
    'bf16_weights_fp32_logits': lambda a: a.update(weights=torch.zeros(2, 32, dtype=torch.bfloat16)),
}


@pytest.mark.parametrize('bad', sorted(PAGED_BAD))
def test_paged_validation(bad):
    args = _paged()
    PAGED_BAD[bad](args)
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.fp8_fp4_paged_mqa_logits(**args)


@pytest.mark.parametrize('bad', ['indices', 'context_lens_1d', 'block_kv', 'num_sms', 'dtype'])
def test_metadata_validation(bad):
    ctx, block_kv, num_sms, indices = torch.ones(2, 1, dtype=torch.int32), 64, 256, None
    if bad == 'indices':
        indices = torch.zeros(2, dtype=torch.int32)
    elif bad == 'context_lens_1d':
        ctx = torch.ones(2, dtype=torch.int32)
    elif bad == 'block_kv':
        block_kv = 128
    elif bad == 'num_sms':
        num_sms = 0
    else:
        ctx = ctx.long()
    with pytest.raises(RuntimeError, match='Assertion error'):
        dg.get_paged_mqa_logits_metadata(ctx, block_kv, num_sms, indices)


def test_legacy_paged_entry_rejects_clean_logits():
    args = _paged()
    args['q'] = args['q'][0]
    with pytest.raises(RuntimeError, match='clean_logits'):
        dg.fp8_paged_mqa_logits(**args, clean_logits=True)
