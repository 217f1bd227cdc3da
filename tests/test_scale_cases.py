"""CPU proof that the data of tests/scale_cases.py can see every class of scale-addressing bug, before any GPU time is spent.

For each class the scale tensor is rewritten the way a buggy kernel would read it, the C oracle (or the FP64 K-grouped restatement)
runs on the mutated scales, and the gate of tests/test_scale_addressing_gpu.py must REJECT the result: in exact mode any differing bit,
in spread mode ``gpu_helpers.assert_close_to_oracle`` against the oracle on the correct scales."""
import pytest
import torch

import oracle
import scale_cases as sc
from gpu_helpers import assert_close_to_oracle


# ------------------------------------------------------------------------------------------------------------------------------------
# How a buggy kernel would read the scales (logical FP32 tensors in, logical FP32 tensors out)
# ------------------------------------------------------------------------------------------------------------------------------------
def sfa_row_plus_one_in_last_group(sfa, rows_per_group):
    """Rows of the last partial ``rows_per_group`` group read row r + 1 (the last row keeps its own: nothing past the end is read)."""
    m = sfa.size(0)
    out = sfa.clone()
    first = (m - 1) // rows_per_group * rows_per_group
    assert first < m - 1, 'the last group must hold at least two rows'
    out[first:m - 1] = sfa[first + 1:m]
    return out


def last_k_block_reads_neighbour(sf):
    out = sf.clone()
    out[..., -1] = sf[..., -2]
    return out


def second_piece_reads_first(sf):
    """A K split in two pieces whose second piece indexes from the first piece's start."""
    out = sf.clone()
    half = sf.size(-1) // 2
    out[..., half:2 * half] = sf[..., :half]
    return out


def last_n_block_reads_previous(sfb):
    out = sfb.clone()
    out[..., -1, :] = sfb[..., -2, :]
    return out


def columns_off_by_one_in_tail(sfb, tile=128):
    n = sfb.size(-2)
    first = (n - 1) // tile * tile
    out = sfb.clone()
    out[..., first:n - 1, :] = sfb[..., first + 1:n, :]
    return out


def group_reads_next(sf):
    out = sf.clone()
    out[:-1] = sf[1:]
    return out


def packed_bytes_reversed(sf):
    """Byte j of every whole packed word read as byte 3 - j (a partial last word keeps its order)."""
    out = sf.clone()
    whole = sf.size(-1) // 4 * 4
    out[..., :whole] = sf[..., :whole].unflatten(-1, (-1, 4)).flip(-1).flatten(-2)
    return out


def word_stride_floor(sf):
    """K-major packed words addressed with a row stride of sf_k / 4 (rounded down) instead of ceil(sf_k / 4)."""
    sf_k = sf.size(-1)
    words = sc.pack_ue8m0(sf)
    rows, per_row = words.shape
    flat = (torch.arange(rows).unsqueeze(1) * (sf_k // 4) + torch.arange(per_row).unsqueeze(0)).clamp(max=rows * per_row - 1)
    return sc.unpack_ue8m0(words.reshape(-1)[flat], sf_k)


def k_group_reads_previous_rows(sf, real_ks, gran_k=128):
    """Group g >= 1 of a K-grouped operand reads its scale rows from group g - 1's (same local block, clamped to that group's count)."""
    out = sf.clone()
    firsts, row = [], 0
    for kg in real_ks:
        firsts.append(row)
        row += -(-kg // gran_k)
    for g in range(1, len(real_ks)):
        blocks, prev = -(-real_ks[g] // gran_k), -(-real_ks[g - 1] // gran_k)
        for j in range(blocks):
            out[firsts[g] + j] = sf[firsts[g - 1] + min(j, prev - 1)]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# Gates
# ------------------------------------------------------------------------------------------------------------------------------------
def exact_rejects(got, want64, label):
    with pytest.raises(AssertionError):
        sc.assert_exact(got, want64, label)


def spread_rejects(got, want, label):
    with pytest.raises(AssertionError):
        assert_close_to_oracle(got, want, label)


def dense(a, sfa, b, sfb, dtype=torch.float32, gran_n=128, gran_k=128):
    d = torch.empty((a.size(0), b.size(0)), dtype=dtype)
    return oracle.fp8_gemm_nt(a, sfa, b, sfb, d, gran_n=gran_n, gran_k=gran_k)


DENSE_CLASSES = {
    # name: (m, n, k, gran_n, gran_k, mutate (sfa, sfb) -> (sfa, sfb))
    'sfa_row_plus_one_last_4_rows': (7, 136, 384, 128, 128, lambda a, b: (sfa_row_plus_one_in_last_group(a, 4), b)),
    'sfa_row_plus_one_last_128_rows': (131, 136, 256, 128, 128, lambda a, b: (sfa_row_plus_one_in_last_group(a, 128), b)),
    'k_tail_block_reads_neighbour': (9, 136, 400, 128, 128, lambda a, b: (a, last_k_block_reads_neighbour(b))),
    'second_k_piece_reads_first': (9, 136, 1024, 128, 128, lambda a, b: (second_piece_reads_first(a), b)),
    'sfb_n_block_off_by_one_in_tail': (9, 264, 256, 128, 128, lambda a, b: (a, last_n_block_reads_previous(b))),
    'per_column_sfb_off_by_one': (9, 136, 256, 1, 128, lambda a, b: (a, columns_off_by_one_in_tail(b))),
    'packed_bytes_reversed': (9, 136, 1024, 1, 128, lambda a, b: (a, packed_bytes_reversed(b))),
    'packed_bytes_reversed_gran_32': (9, 136, 256, 1, 32, lambda a, b: (packed_bytes_reversed(a), b)),
    'word_stride_floor_k_not_512': (9, 136, 640, 1, 128, lambda a, b: (a, word_stride_floor(b))),
}


@pytest.mark.parametrize('name', list(DENSE_CLASSES))
def test_dense_mutation_is_caught(name):
    m, n, k, gran_n, gran_k, mutate = DENSE_CLASSES[name]
    for mode in ('exact', 'spread'):
        if mode == 'spread' and gran_k == 32:
            continue                            # (granularity 32 exists only as packed UE8M0: powers of two)
        a, sfa = sc.operand(m, k, gran_k=gran_k, mode=mode, seed=1)
        b, sfb = sc.operand(n, k, gran_mn=gran_n, gran_k=gran_k, mode=mode, a_side=False, seed=1)
        bad_sfa, bad_sfb = mutate(sfa, sfb)
        assert not (torch.equal(bad_sfa, sfa) and torch.equal(bad_sfb, sfb)), 'the mutation must change what is read'
        if mode == 'exact':
            sc.exact_bound(k)
            want = sc.reference(a, sfa, b, sfb, gran_n, gran_k)
            for dtype in (torch.float32, torch.bfloat16):
                sc.assert_exact(dense(a, sfa, b, sfb, dtype, gran_n, gran_k), want, f'{name}: oracle on the correct scales')
                exact_rejects(dense(a, bad_sfa, b, bad_sfb, dtype, gran_n, gran_k), want, name)
        else:
            want = dense(a, sfa, b, sfb, torch.bfloat16, gran_n)
            assert_close_to_oracle(dense(a, sfa, b, sfb, torch.bfloat16, gran_n), want, name)
            spread_rejects(dense(a, bad_sfa, b, bad_sfb, torch.bfloat16, gran_n), want, name)


@pytest.mark.parametrize('psum', [False, True])
def test_contiguous_group_reads_next_groups_sfb(psum):
    actual_ms = [37, 128, 0, 90]
    n, k = 136, 384
    for mode in ('exact', 'spread'):
        (a, sfa, b, sfb), starts, aligned = sc.contiguous_case(actual_ms, n, k, mode=mode, seed=2)
        layout, _, _ = sc.contiguous_layout(actual_ms, psum=psum)

        def run(sfb_used):
            d = torch.zeros((a.size(0), n), dtype=torch.bfloat16)
            return oracle.m_grouped_fp8_gemm_nt_contiguous(a, sfa, b, sfb_used, d, layout, use_psum_layout=psum)
        bad = group_reads_next(sfb)
        if mode == 'exact':
            want = sc.contiguous_reference(a, sfa, b, sfb, actual_ms, starts)
            sc.assert_exact(run(sfb), want, 'contiguous oracle')
            exact_rejects(run(bad), want, 'contiguous group + 1')
        else:
            spread_rejects(run(bad), run(sfb), 'contiguous group + 1')


def test_masked_group_reads_next_groups_sfb():
    groups, max_m, n, k = 3, 24, 136, 384
    masked = torch.tensor([5, 24, 17], dtype=torch.int32)
    for mode in ('exact', 'spread'):
        a, sfa, b, sfb = sc.masked_case(groups, max_m, n, k, mode=mode, seed=3)

        def run(sfb_used):
            d = torch.zeros((groups, max_m, n), dtype=torch.bfloat16)
            return oracle.m_grouped_fp8_gemm_nt_masked(a, sfa, b, sfb_used, d, masked)
        want = sc.reference(a, sfa, b, sfb)
        for g, rows in enumerate(masked.tolist()):
            want[g, rows:] = 0
        bad = group_reads_next(sfb)
        if mode == 'exact':
            sc.assert_exact(run(sfb), want, 'masked oracle')
            exact_rejects(run(bad), want, 'masked group + 1')
        else:
            spread_rejects(run(bad), run(sfb), 'masked group + 1')


@pytest.mark.parametrize('k_alignment,gran_k', [(128, 128), (160, 128), (32, 32)])
def test_k_grouped_sfa_reads_previous_groups_rows(k_alignment, gran_k):
    real_ks = [256, 96, 384] if k_alignment != 128 else [256, 128, 384]
    a, sfa, b, sfb, ends, starts = sc.k_grouped_case(24, 40, real_ks, k_alignment, gran_k, seed=4)
    c = sc.addend((3, 24, 40))
    want = sc.k_grouped_reference(a, sfa, b, sfb, real_ks, starts, gran_k, c)
    sc.exact_bound(max(real_ks), sc.C_MAX)
    # the FP32 form of the same sums (group by group, the C oracle's dense form on K-major copies) is exact
    for g, (kg, s) in enumerate(zip(real_ks, starts)):
        rows = slice(sum(-(-x // gran_k) for x in real_ks[:g]), sum(-(-x // gran_k) for x in real_ks[:g + 1]))
        d = c[g].clone()
        oracle.fp8_gemm_nt(a[s:s + kg].t().contiguous(), sfa[rows].t().contiguous(), b[s:s + kg].t().contiguous(), sfb[rows].t().contiguous(),
                           d, c=d, gran_n=1, gran_k=gran_k)
        sc.assert_exact(d, want[g], f'k-grouped oracle group {g}')
    bad = sc.k_grouped_reference(a, k_group_reads_previous_rows(sfa, real_ks, gran_k), b, sfb, real_ks, starts, gran_k, c)
    exact_rejects(bad.float(), want, 'k-grouped sfa from the previous group')


def test_neighbouring_scales_differ_by_at_least_two():
    """The fingerprint property itself: along every dimension, neighbours, the two ends, the four bytes of a packed word against their
    reversal and the same block of neighbouring groups differ by a factor of two or more."""
    for shape, coefs in (((7, 5), (1, 2)), ((131, 6), (2, 1)), ((3, 9, 11), (3, 1, 2)), ((2, 1, 4), (3, 2, 1)), ((6, 16), (1, 2))):
        e = sc.exponents(shape, coefs)
        assert int(e.min()) >= sc.EXP_LO and int(e.max()) <= sc.EXP_HI
        for d, length in enumerate(shape):
            if length < 2:
                continue
            assert bool((e.diff(dim=d) != 0).all()), (shape, d)
            assert bool((e.select(d, 0) != e.select(d, length - 1)).all()), (shape, d, 'wrap-around')
        words = e.size(-1) // 4 * 4
        if words:
            q = e[..., :words].unflatten(-1, (-1, 4))
            assert bool((q != q.flip(-1)).all()), (shape, 'packed word reversal')
        assert not bool((sc.exponents(shape, coefs, salt=1) == e).any()), 'a second fingerprint changes every scale'
    a_sf = sc.operand(130, 640, seed=0)[1]
    b_sf = sc.operand(136, 640, gran_mn=128, a_side=False, seed=0)[1]
    assert not torch.equal(a_sf[:2], b_sf), 'A and B are fingerprinted differently'
    spread = sc.operand(130, 640, mode='spread', seed=0)[1]
    ratio = spread[:, 1:] / spread[:, :-1]
    assert bool(((ratio >= 1.2) | (ratio <= 1 / 1.2)).all())


def test_packing_round_trip_and_exact_bound():
    sf = sc.scales((5, 7), (1, 2))
    words = sc.pack_ue8m0(sf)
    assert words.shape == (5, 2)
    assert torch.equal(sc.unpack_ue8m0(words, 7), sf)
    assert torch.equal(words, oracle.pack_sf_ue8m0(sf).contiguous())
    sc.exact_bound(7168, sc.C_MAX)
    with pytest.raises(AssertionError):
        sc.exact_bound(32768)
