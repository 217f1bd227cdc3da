"""Scale-factor addressing of every FP8 GEMM kernel, on operands whose scales cannot be confused with one another (tests/scale_cases.py).

Exact mode: FP8 integers and power-of-two scales keep every sum exact in FP32, so a correct kernel returns exactly the FP64 value --
FP32 outputs bit for bit, BF16 outputs bit-equal to its round-to-nearest-even cast -- whatever its accumulation order, K split or MFMA
internals; a kernel that reads any neighbouring scale instead changes the result by a factor of two somewhere.  Spread mode (FP32-scale
kernels): non-power-of-two scales, against the C oracle under the gates of tests/gpu_helpers.py.

  * every FP8 configuration of ``dg.list_configs()``, forced by name on a shape that breaks its tiles (CONFIG_CASES: a configuration
    without an entry fails);
  * the automatic selection of the public operators across the shape bands where it changes, both SFA layouts, the grouped, masked and
    K-grouped forms, the 'sm100' scaling-factor mode and the four BASELINE shapes at full size, every element compared;
  * captured graphs replayed after the scale tensors were rewritten in place with a second fingerprint."""
import pytest
import torch

import deepgemm_amd as dg
import oracle
import scale_cases as sc
from gpu_helpers import assert_close_to_oracle

pytestmark = pytest.mark.gpu

FP8_CONFIGS = [c for c in dg.list_configs() if not c.startswith('bf16_')]


@pytest.fixture(autouse=True)
def _defaults():
    dg.set_forced_config('auto')
    dg.set_sf_cast_mode('sm90')
    dg.set_mk_alignment_for_contiguous_layout(128)
    yield
    dg.set_forced_config('auto')
    dg.set_sf_cast_mode('sm90')


def run_dense(m, n, k, a_mn=False, b_mn=False, gran_n=128, gran_k=128, packed=False, sfa_rm=False, out=torch.bfloat16, accumulate=False,
              mode='exact', seed=0):
    """fp8_gemm_nt on fingerprinted operands: (d, FP64 reference, CPU operands).  ``packed``: UE8M0 words (per-column SFB)."""
    assert not packed or gran_n == 1
    a, sfa = sc.operand(m, k, gran_k=gran_k, mode=mode, seed=seed)
    b, sfb = sc.operand(n, k, gran_mn=gran_n, gran_k=gran_k, mode=mode, a_side=False, seed=seed)
    a_d, sfa_d, b_d, sfb_d = (t.cuda() for t in (a, sfa, b, sfb))
    a_op, b_op = (sc.mn_major(a_d) if a_mn else a_d), (sc.mn_major(b_d) if b_mn else b_d)
    if packed:
        sfa_op, sfb_op, recipe = sc.pack_ue8m0(sfa_d), sc.pack_ue8m0(sfb_d), (1, 1, gran_k)
    else:
        sfa_op = sfa_d if sfa_rm else dg.get_mn_major_tma_aligned_tensor(sfa_d)
        sfb_op, recipe = sfb_d, ((1, 1, 128) if gran_n == 1 else None)
    c = sc.addend((m, n), seed, 'cuda') if accumulate else None
    if mode == 'exact':
        sc.exact_bound(k, sc.C_MAX if accumulate else 0)
    d = c.to(out, copy=True) if accumulate else torch.full((m, n), float('nan'), dtype=out, device='cuda')
    dg.fp8_gemm_nt((a_op, sfa_op), (b_op, sfb_op), d, c=d if accumulate else None, recipe=recipe)
    want = sc.reference(a_d, sfa_d, b_d, sfb_d, gran_n, gran_k, None if c is None else c.to(out))
    return d, want, (a, sfa, b, sfb)


# ------------------------------------------------------------------------------------------------------------------------------------
# One case per configuration: the operand form, recipe and a shape that breaks the configuration's tiles
#   m = 259 / 101: m % 128 != 0 and m % 4 != 0 (the last 4-row group of the MN-major SFA is partial); m = 272: m % 16 == 0, needed by an
#   MN-major A; n = 520: n % 128 == 8; n = 528: n % 16 == 0, needed by an MN-major B; k = 640: five K blocks, k % 512 != 0 (the last packed
#   word holds one byte); k = 656: a partial last K block; k = 1024 / 2048: whole packed words / enough K blocks for in-kernel K pieces.
# ------------------------------------------------------------------------------------------------------------------------------------
RAGGED = dict(m=259, n=520, k=640)
K_PIECES = dict(m=101, n=392, k=2048)
SKINNY_16, SKINNY_32 = dict(m=13, n=392, k=640), dict(m=29, n=392, k=640)
B_MN, A_MN, AB_MN = dict(m=259, n=528, k=640, b_mn=True), dict(m=272, n=520, k=640, a_mn=True), dict(m=272, n=528, k=640, a_mn=True, b_mn=True)
K_TAIL, K_TAIL_B_MN = dict(m=259, n=520, k=656), dict(m=259, n=528, k=656, b_mn=True)
PER_COL = dict(gran_n=1)
PACKED, PACKED_32 = dict(gran_n=1, packed=True), dict(gran_n=1, packed=True, gran_k=32)

CONFIG_CASES = {}
for _name in ('duo_256x256', 'duo_p_256x256', 'duo_128x256', 'duo_sk_128x256', 'pipe_256x256', 'pipe_128x256', 'pipe_128x128', 'pipe_64x256',
              'pipe_32x256', 'pipe_16x256', 'stream_64x128', 'stream_nt_64x128', 'stream2_64x128', 'stream_nt2_64x128', 'stream_64x32',
              'stream_l8_64x32', 'generic_128x128'):
    CONFIG_CASES[_name] = RAGGED
for _name in ('stream_ks_64x128', 'stream_ks_64x32', 'stream_ks_64x64'):
    CONFIG_CASES[_name] = K_PIECES
for _name in ('skinny_16', 'skinny_16w', 'skinny_16c', 'skinny_16wc', 'skinny_16ca'):
    CONFIG_CASES[_name] = SKINNY_16
for _name in ('skinny_32', 'skinny_32c', 'skinny_32ca'):
    CONFIG_CASES[_name] = SKINNY_32
CONFIG_CASES.update({
    'duo_bmn_256x256': B_MN, 'duo_bmn_128x256': B_MN, 'duo_sk_bmn_128x256': B_MN,
    'duo_amn_256x256': A_MN, 'duo_abmn_256x256': AB_MN,
    'duo_kt_256x256': K_TAIL, 'duo_kt_128x256': K_TAIL, 'duo_bmn_kt_256x256': K_TAIL_B_MN, 'duo_bmn_kt_128x256': K_TAIL_B_MN,
    'pipe_pc_256x256': dict(RAGGED, **PER_COL), 'pipe_pc_192x256': dict(RAGGED, **PER_COL), 'pipe_pc_mn_256x256': dict(AB_MN, **PER_COL),
})
for _name in ('e8_quad_256x256', 'e8_quad_h_256x256', 'e8_quad_h2_256x256'):          # (whole packed words only)
    CONFIG_CASES[_name] = dict(RAGGED, k=1024, **PACKED)
for _name in ('e8_quad_128x256', 'e8_duo_256x256', 'e8_stream_64x128', 'e8_stream_nt_64x128', 'e8_stream_64x32', 'e8_stream2_64x128',
              'e8_stream_nt2_64x128', 'e8_stream_l8_64x32'):
    CONFIG_CASES[_name] = dict(RAGGED, **PACKED)
for _name in ('e8_quad_g32_256x256', 'e8_quad_g32_128x256', 'e8_stream_g32_64x32', 'e8_stream_l8_g32_64x32', 'e8_stream2_g32_64x128',
              'e8_stream_nt2_g32_64x128'):
    CONFIG_CASES[_name] = dict(RAGGED, **PACKED_32)
CONFIG_CASES.update({
    'e8_stream_ks_64x128': dict(K_PIECES, **PACKED), 'e8_stream_ks_64x32': dict(K_PIECES, **PACKED),
    'e8_stream_ks_g32_64x128': dict(K_PIECES, **PACKED_32), 'e8_stream_ks_g32_64x32': dict(K_PIECES, **PACKED_32),
    'e8_skinny_16': dict(SKINNY_16, **PACKED), 'e8_skinny_32': dict(SKINNY_32, **PACKED),
    'e8_skinny_g32_16': dict(SKINNY_16, **PACKED_32), 'e8_skinny_g32_32': dict(SKINNY_32, **PACKED_32),
    'e8_quad_kt_128x256': dict(K_TAIL, **PACKED),
    'e8_duo_bmn_256x256': dict(B_MN, **PACKED), 'e8_duo_amn_256x256': dict(A_MN, **PACKED), 'e8_duo_abmn_256x256': dict(AB_MN, **PACKED),
    'e8_duo_bmn_kt_256x256': dict(K_TAIL_B_MN, **PACKED),
})


@pytest.mark.parametrize('name', FP8_CONFIGS)
def test_every_config_reads_the_right_scales(name):
    spec = CONFIG_CASES.get(name)
    assert spec is not None, f'no scale-addressing case for config {name}'
    dg.set_forced_config(name)
    d, want, _ = run_dense(**spec, seed=len(name))
    assert dg.last_config() == name, f'{name} refused its table case (ran {dg.last_config()}): fix CONFIG_CASES'
    sc.assert_exact(d, want, f'{name} {spec}')
    if not spec.get('packed'):
        # spread mode: FP32 scales that are not powers of two, against the C oracle
        d, _, (a, sfa, b, sfb) = run_dense(**spec, mode='spread', seed=len(name))
        assert dg.last_config() == name
        want = torch.empty(d.shape, dtype=torch.bfloat16)
        oracle.fp8_gemm_nt(a, sfa, b, sfb, want, gran_n=spec.get('gran_n', 128))
        assert_close_to_oracle(d, want, f'{name} spread')


def test_config_table_has_no_stale_entries():
    assert sorted(set(CONFIG_CASES) - set(FP8_CONFIGS)) == []


# ------------------------------------------------------------------------------------------------------------------------------------
# Automatic selection
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scales', ['fp32', 'fp32_rowmajor_sfa', 'packed', 'sm100'])
@pytest.mark.parametrize('n,k', [(4096, 7168), (576, 7168), (2112, 2048)])
def test_auto_dense_across_m_bands(scales, n, k):
    for m in (1, 24, 100, 200, 1024):
        if scales == 'sm100':
            dg.set_sf_cast_mode('sm100')
        d, want, _ = run_dense(m, n, k, packed=scales == 'packed', gran_n=1 if scales == 'packed' else 128, sfa_rm=scales == 'fp32_rowmajor_sfa',
                               seed=m)
        sc.assert_exact(d, want, f'{scales} {m}x{n}x{k} ({dg.last_config()})')


@pytest.mark.parametrize('packed', [False, True])
def test_auto_dense_fp32_output_and_accumulation(packed):
    kw = dict(gran_n=1, packed=True) if packed else {}
    for m, n, k in ((259, 520, 640), (24, 4096, 7168), (200, 576, 7168)):
        d, want, _ = run_dense(m, n, k, out=torch.float, **kw)
        sc.assert_exact(d, want, f'FP32 out {m}x{n}x{k} ({dg.last_config()})')
        d, want, _ = run_dense(m, n, k, out=torch.float, accumulate=True, **kw)
        sc.assert_exact(d, want, f'FP32 accumulate {m}x{n}x{k} ({dg.last_config()})')
        d, want, _ = run_dense(m, n, k, accumulate=True, **kw)
        c = sc.addend((m, n), 0, 'cuda').bfloat16().double()
        # (BF16 accumulation: the reduce-add rounds the exact product to BF16 before adding C, as the oracle does -- its gate, with the addend's term)
        want = ((want - c).float().bfloat16().double() + c).float().bfloat16()
        assert_close_to_oracle(d, want, f'BF16 accumulate {m}x{n}x{k} ({dg.last_config()})', addend=c)


@pytest.mark.parametrize('layout', ['nn', 'tn', 'tt'])
@pytest.mark.parametrize('packed', [False, True])
def test_auto_public_layouts(layout, packed):
    m, n, k = 272, 528, 640
    a, sfa = sc.operand(m, k, seed=5)
    b, sfb = sc.operand(n, k, gran_mn=1 if packed else 128, a_side=False, seed=5)
    a, sfa, b, sfb = (t.cuda() for t in (a, sfa, b, sfb))
    want = sc.reference(a, sfa, b, sfb, gran_n=1 if packed else 128)
    sfa_op, sfb_op = (sc.pack_ue8m0(sfa), sc.pack_ue8m0(sfb)) if packed else (sfa, sfb)
    a_arg = (a.t().contiguous(), sfa_op.t()) if layout[0] == 't' else (a, sfa_op)          # t: A stored [K, M]
    b_arg = (b.t().contiguous(), sfb_op.t()) if layout[1] == 'n' else (b, sfb_op)          # n: B stored [K, N]
    d = torch.full((m, n), float('nan'), dtype=torch.bfloat16, device='cuda')
    getattr(dg, f'fp8_gemm_{layout}')(a_arg, b_arg, d, recipe=(1, 1, 128) if packed else None)
    sc.assert_exact(d, want, f'{layout} packed={packed} ({dg.last_config()})')


def _contiguous(actual_ms, n, k, psum, scales, seed=0):
    (a, sfa, b, sfb), starts, aligned = sc.contiguous_case(actual_ms, n, k, seed=seed, device='cuda')
    layout, _, _ = sc.contiguous_layout(actual_ms, psum=psum, device='cuda')
    want = sc.contiguous_reference(a, sfa, b, sfb, actual_ms, starts)
    if scales == 'packed':           # per-row SFB words: the 128-row SFB broadcast to its rows
        sfb_rows = sfb.repeat_interleave(128, dim=1)[:, :n]
        a_arg, b_arg = (a, sc.pack_ue8m0(sfa)), (b, sc.pack_ue8m0(sfb_rows))
    else:
        a_arg, b_arg = (a, sfa), (b, sfb)
    d = torch.full((a.size(0), n), float('nan'), dtype=torch.bfloat16, device='cuda')
    if scales == 'sm100':
        dg.set_sf_cast_mode('sm100')
    dg.m_grouped_fp8_gemm_nt_contiguous(a_arg, b_arg, d, layout, use_psum_layout=psum)
    return d, want


@pytest.mark.parametrize('psum', [False, True])
def test_forced_configs_on_group_relative_tiles(psum):
    """The configurations that take the contiguous layouts, forced by name: every group indexes its own SFB (the per-config table above
    runs dense problems, whose group is always 0)."""
    fp32 = ['generic_128x128', 'pipe_128x256', 'pipe_128x128', 'pipe_64x256', 'duo_128x256'] + ([] if psum else ['duo_256x256', 'duo_p_256x256'])
    packed = ['e8_quad_128x256'] + ([] if psum else ['e8_quad_256x256'])
    actual_ms, n = [37, 300, 0, 129, 256], 520
    for scales, names, k in (('fp32', fp32, 640), ('packed', packed, 1024)):
        for name in names:
            dg.set_forced_config(name)
            d, want = _contiguous(actual_ms, n, k, psum, scales, seed=len(name))
            assert dg.last_config() == name, (name, dg.last_config())
            sc.assert_exact(d, want, f'contiguous psum={psum} forced {name}')


@pytest.mark.parametrize('scales', ['fp32', 'packed', 'sm100'])
@pytest.mark.parametrize('psum', [False, True])
def test_auto_m_grouped_contiguous(psum, scales):
    for actual_ms, n, k in (([37, 300, 0, 129, 256], 520, 640), ([128] * 6 + [77], 4096, 2048), ([500, 3, 260, 0], 2112, 7168)):
        d, want = _contiguous(actual_ms, n, k, psum, scales, seed=len(actual_ms))
        sc.assert_exact(d, want, f'contiguous psum={psum} {scales} {actual_ms} ({dg.last_config()}); padding rows must be zeros')


@pytest.mark.parametrize('scales', ['fp32', 'packed', 'sm100'])
def test_auto_m_grouped_masked(scales):
    for groups, max_m, n, k, masked_ms in ((4, 64, 520, 640, [5, 0, 64, 33]), (6, 128, 4096, 2048, [128, 1, 97, 0, 64, 17]),
                                          (3, 256, 2112, 7168, [256, 130, 200])):
        a, sfa, b, sfb = sc.masked_case(groups, max_m, n, k, seed=groups, device='cuda')
        masked = torch.tensor(masked_ms, dtype=torch.int32, device='cuda')
        want = sc.reference(a, sfa, b, sfb)
        for g, rows in enumerate(masked_ms):
            want[g, rows:] = float('nan')
        if scales == 'packed':
            a_arg, b_arg = (a, sc.pack_ue8m0(sfa)), (b, sc.pack_ue8m0(sfb.repeat_interleave(128, dim=1)[:, :n]))
        else:
            a_arg, b_arg = (a, sfa), (b, sfb)
        if scales == 'sm100':
            dg.set_sf_cast_mode('sm100')
        d = torch.full((groups, max_m, n), float('nan'), dtype=torch.bfloat16, device='cuda')
        dg.m_grouped_fp8_gemm_nt_masked(a_arg, b_arg, d, masked, max(1, sum(masked_ms) // groups))
        sc.assert_exact(d, want, f'masked {scales} {masked_ms} ({dg.last_config()}); rows >= masked_m must stay NaN')


@pytest.mark.parametrize('form', ['fp32_128', 'fp32_psum_160', 'ue8m0_128', 'ue8m0_psum_160', 'ue8m0_g32_psum_32', 'nt_fp32'])
def test_auto_k_grouped(form):
    m, n = 96, 144
    gran_k = 32 if 'g32' in form else 128
    k_alignment = 160 if '160' in form else (32 if form.endswith('_32') else 128)
    psum = 'psum' in form
    real_ks = [256, 0, 384, 128] if k_alignment == 128 else [256, 96, 0, 400]
    a, sfa, b, sfb, ends, starts = sc.k_grouped_case(m, n, real_ks, k_alignment, gran_k, seed=len(form), device='cuda')
    c = sc.addend((len(real_ks), m, n), 1, 'cuda')
    sc.exact_bound(max(real_ks), sc.C_MAX)
    want = sc.k_grouped_reference(a, sfa, b, sfb, real_ks, starts, gran_k, c)
    d = c.clone()
    dg.set_mk_alignment_for_contiguous_layout(k_alignment)
    if form == 'nt_fp32':           # the SM90 operand form: each group's [m, k_g] K-major block, one after another
        flat_a = torch.cat([a[s:s + kg].t().contiguous().reshape(-1) for kg, s in zip(real_ks, starts) if kg])
        flat_b = torch.cat([b[s:s + kg].t().contiguous().reshape(-1) for kg, s in zip(real_ks, starts) if kg])
        layout = torch.tensor(real_ks, dtype=torch.int32, device='cuda')
        dg.k_grouped_fp8_gemm_nt_contiguous((flat_a, sfa.t()), (flat_b, sfb.t()), d, real_ks, layout, c=d)
    else:
        if form.startswith('ue8m0') and gran_k == 128:
            dg.set_sf_cast_mode('sm100')
        layout = torch.tensor(ends if psum else real_ks, dtype=torch.int32, device='cuda')
        ks_cpu = None if psum else real_ks
        dg.k_grouped_fp8_gemm_tn_contiguous((a, sfa), (b, sfb), d, ks_cpu, layout, c=d, recipe=(1, 1, gran_k), use_psum_layout=psum)
    sc.assert_exact(d, want, f'k-grouped {form}')


# ------------------------------------------------------------------------------------------------------------------------------------
# BASELINE shapes at full size, every element
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('packed', [False, True])
def test_baseline_c2_exact(packed):
    d, want, _ = run_dense(4096, 4096, 7168, gran_n=1 if packed else 128, packed=packed)
    sc.assert_exact(d, want, f'C2 packed={packed} ({dg.last_config()})')


@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn', 'tt'])
def test_baseline_c3_exact(layout):
    d, want, _ = run_dense(2048, 7168, 2048, a_mn=layout[0] == 't', b_mn=layout[1] == 'n')
    sc.assert_exact(d, want, f'C3 {layout} ({dg.last_config()})')


def test_baseline_c4_exact():
    actual_ms = [461, 512, 600, 389, 530, 512, 475, 640]
    d, want = _contiguous(actual_ms, 4096, 7168, False, 'fp32')
    sc.assert_exact(d, want, f'C4 ({dg.last_config()})')


def test_baseline_c5_exact():
    masked_ms = [48, 64, 0, 33, 57, 41, 64, 17]
    a, sfa, b, sfb = sc.masked_case(8, 64, 4096, 7168, device='cuda')
    masked = torch.tensor(masked_ms, dtype=torch.int32, device='cuda')
    want = sc.reference(a, sfa, b, sfb)
    for g, rows in enumerate(masked_ms):
        want[g, rows:] = float('nan')
    d = torch.full((8, 64, 4096), float('nan'), dtype=torch.bfloat16, device='cuda')
    dg.m_grouped_fp8_gemm_nt_masked((a, sfa), (b, sfb), d, masked, 48)
    sc.assert_exact(d, want, f'C5 ({dg.last_config()})')


# ------------------------------------------------------------------------------------------------------------------------------------
# Captured graphs: scales rewritten in place between replays
# ------------------------------------------------------------------------------------------------------------------------------------
def _capture(fn):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()                                # warm-up on the capture stream: its K-split scratch buffer exists before capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        fn()
    return graph


def test_graph_replay_reads_rewritten_scales_k_split():
    m, n, k = 128, 576, 7168
    a, sfa = sc.operand(m, k, seed=11)
    b, sfb = sc.operand(n, k, gran_mn=128, a_side=False, seed=11)
    a, sfa, b, sfb = (t.cuda() for t in (a, sfa, b, sfb))
    sfa_mn = dg.get_mn_major_tma_aligned_tensor(sfa)          # (the layout the kernels read: no copy inside the graph)
    d = torch.full((m, n), float('nan'), dtype=torch.bfloat16, device='cuda')
    graph = _capture(lambda: dg.fp8_gemm_nt((a, sfa_mn), (b, sfb), d))
    captured = dg.last_config()
    assert '_ks_' in captured or '_sk_' in captured, f'this shape is meant to capture a K-split kernel, got {captured}'
    graph.replay()
    torch.cuda.synchronize()
    sc.assert_exact(d, sc.reference(a, sfa, b, sfb), f'first replay ({captured})')
    new_sfa = sc.operand(m, k, salt=1, seed=11)[1].cuda()
    new_sfb = sc.operand(n, k, gran_mn=128, a_side=False, salt=1, seed=11)[1].cuda()
    sfa_mn.copy_(new_sfa)
    sfb.copy_(new_sfb)
    d.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    sc.assert_exact(d, sc.reference(a, new_sfa, b, new_sfb), f'replay after the scales were rewritten ({captured})')


@pytest.mark.parametrize('packed', [False, True])
def test_graph_replay_reads_rewritten_scales_grouped(packed):
    actual_ms, n, k = [200, 64, 300, 0], 1024, 2048
    (a, sfa, b, sfb), starts, _ = sc.contiguous_case(actual_ms, n, k, seed=12, device='cuda')
    layout, _, _ = sc.contiguous_layout(actual_ms, device='cuda')
    if packed:
        sfa_op, sfb_op = sc.pack_ue8m0(sfa), sc.pack_ue8m0(sfb.repeat_interleave(128, dim=1)[:, :n])
    else:
        sfa_op, sfb_op = dg.get_mn_major_tma_aligned_tensor(sfa), sfb
    d = torch.full((a.size(0), n), float('nan'), dtype=torch.bfloat16, device='cuda')
    graph = _capture(lambda: dg.m_grouped_fp8_gemm_nt_contiguous((a, sfa_op), (b, sfb_op), d, layout))
    captured = dg.last_config()
    graph.replay()
    torch.cuda.synchronize()
    sc.assert_exact(d, sc.contiguous_reference(a, sfa, b, sfb, actual_ms, starts), f'first replay ({captured})')
    (_, new_sfa, _, new_sfb), _, _ = sc.contiguous_case(actual_ms, n, k, salt=1, seed=12, device='cuda')
    if packed:
        sfa_op.copy_(sc.pack_ue8m0(new_sfa))
        sfb_op.copy_(sc.pack_ue8m0(new_sfb.repeat_interleave(128, dim=1)[:, :n]))
    else:
        sfa_op.copy_(new_sfa)
        sfb_op.copy_(new_sfb)
    d.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    sc.assert_exact(d, sc.contiguous_reference(a, new_sfa, b, new_sfb, actual_ms, starts), f'replay after the scales were rewritten ({captured})')
