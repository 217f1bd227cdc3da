"""Indexer MQA logits on the GPU through the public entries: every (H, D) with ragged sizes and random / CP / non-CP ranges, FP32 and
BF16 logits, BF16 weights, the compressed form; the paged form over batch sizes, next_n, both block sizes, a shuffled block table whose
unused entries name a NaN block and a padded cache stride.  Gates: exact -inf masks, calc_diff < 1e-8 against an FP64 statement of the
FP8 inputs themselves (BF16 logits: within one BF16 ulp of it), and the reference test's own gates.  Also repeatability, independence
from set_num_sms, hipGraph replay, and one full-size case of each form."""
import pytest
import torch

import deepgemm_amd as dg
from deepgemm_amd.testing import calc_diff
from deepgemm_amd.testing import generators as gen

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')


@pytest.fixture(autouse=True)
def _seed():
    gen.reset_seed(0)
    num_sms = dg.get_num_sms()
    yield
    dg.set_num_sms(num_sms)


# ---------------------------------------------------------------- inputs

def _cast_rows_fp8(x: torch.Tensor):
    """Per-row FP8 cast of the reference's tests (amax / 448 scales)."""
    sf = x.abs().float().amax(dim=-1).clamp(1e-4) / 448.0
    return (x.float() / sf.unsqueeze(-1)).to(torch.float8_e4m3fn), sf


def _dense_inputs(s, s_kv, h, d, weights_dtype=torch.float32):
    q = torch.randn(s, h, d, device='cuda', dtype=torch.bfloat16)
    kv = torch.randn(s_kv, d, device='cuda', dtype=torch.bfloat16)
    w = torch.randn(s, h, device='cuda', dtype=torch.float32).to(weights_dtype)
    kv_fp8, kv_sf = _cast_rows_fp8(kv)
    return q, kv, w, q.to(torch.float8_e4m3fn), kv_fp8, kv_sf


def _ks_ke(kind, s, s_kv):
    if kind == 'noncp':                                     # the reference's generator with CP disabled
        return (torch.zeros(s, dtype=torch.int32, device='cuda'),
                (torch.arange(s, dtype=torch.int32, device='cuda') + (s_kv - s)))
    if kind == 'cp':                                        # ... with CP (an arbitrary rank)
        chunk, cp_size = s // 2, s_kv // s
        cp_id = cp_size // 3
        i = torch.arange(chunk, dtype=torch.int32)
        ke = torch.cat([cp_id * chunk + i, (cp_size * 2 - 1 - cp_id) * chunk + i])
        return torch.zeros(s, dtype=torch.int32, device='cuda'), ke.int().cuda()
    # random ranges: empty rows, ranges clipped at 0 and at S_kv
    ks = torch.randint(-40, s_kv, (s,), dtype=torch.int32)
    ke = ks + torch.randint(-20, s_kv // 2 + 40, (s,), dtype=torch.int32)
    ks[::7], ke[::7] = 5, 5
    ks[1::9] = -3
    ke[2::9] = s_kv + 17
    return ks.cuda(), ke.cuda()


# ---------------------------------------------------------------- FP64 statements

def _dense_ref(q, kv, w, ks, ke, chunk=4096, with_mag=False):
    """FP64 logits [S, S_kv] (-inf outside the ranges) and mag = sum_h |w| sum_d |q k| (the scale of the kernel's rounding errors).
    q [S, H, D] and kv [S_kv, D] as float64 values (FP8 inputs: q.double(), kv_fp8.double() * sf)."""
    s_kv = kv.shape[0]
    out = torch.empty(q.shape[0], s_kv, dtype=torch.float64, device='cuda')
    mag = torch.empty_like(out)
    w64 = w.double()
    cols = torch.arange(s_kv, device='cuda')
    for c0 in range(0, s_kv, chunk):
        score = torch.einsum('shd,nd->shn', q, kv[c0:c0 + chunk]).relu()
        out[:, c0:c0 + chunk] = torch.einsum('shn,sh->sn', score, w64)
        del score
        if with_mag:
            mag[:, c0:c0 + chunk] = torch.einsum('shn,sh->sn', torch.einsum('shd,nd->shn', q.abs(), kv[c0:c0 + chunk].abs()), w64.abs())
    inside = (cols[None, :] >= ks[:, None].long()) & (cols[None, :] < ke[:, None].long())
    return out.masked_fill(~inside, NEG_INF), mag, inside


def _check_fp32(out, ref, inside, bound=1e-8):
    assert torch.equal(torch.isneginf(out) & ~inside, ~inside), 'every column outside the range is -inf'
    got = out.double().masked_fill(~inside, 0)
    assert not torch.isnan(got).any()
    diff = calc_diff(got, ref.masked_fill(~inside, 0))
    assert diff < bound, diff


# Absolute rounding allowance, relative to mag = sum_h |w| sf sum_d |q k|.  The FP8 matrix instruction's dot product over D is not
# FP32-exact: measured on MI355X its error is up to ~1e-5 of sum_d |q k| (median ~2e-6 of the head sum's magnitude), FP8 denormals
# included.  Where the head sum cancels to a tiny value that error exceeds a BF16 ulp of the result, so the BF16 gate is one ulp plus
# 2^-14 mag (several times the largest error measured).
MAG_ALLOWANCE = 2.0 ** -14


def _check_bf16(out, ref, mag, inside):
    """Within one BF16 ulp of the FP64 value rounded to BF16, plus MAG_ALLOWANCE * mag."""
    assert torch.equal(torch.isneginf(out) & ~inside, ~inside)
    r = ref.masked_fill(~inside, 0).to(torch.bfloat16).double()
    _, e = torch.frexp(r)
    ulp = torch.ldexp(torch.ones_like(r), e - 8)
    allowed = ulp + MAG_ALLOWANCE * mag
    err = (out.double().masked_fill(~inside, 0) - r).abs()
    assert bool((err <= allowed).all()), float((err - allowed).max())


def _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke, logits_dtype=torch.float32, **kw):
    return dg.fp8_fp4_mqa_logits((q_fp8, None), (kv_fp8, kv_sf), w, ks, ke, logits_dtype=logits_dtype, **kw)


def _fp8_values(q_fp8, kv_fp8, kv_sf):
    return q_fp8.double(), kv_fp8.double() * kv_sf.double().unsqueeze(1)


# ---------------------------------------------------------------- dense

@pytest.mark.parametrize('h', [8, 16, 32, 64])
@pytest.mark.parametrize('d', [32, 64, 128])
def test_dense_every_shape_ragged(h, d):
    s, s_kv = 37, 300                                      # S not a multiple of 128 / H, S_kv not a multiple of 256
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(s, s_kv, h, d)
    ks, ke = _ks_ke('random', s, s_kv)
    out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    assert out.shape == (s, s_kv) and out.dtype == torch.float32
    assert out.stride(0) % 256 == 0 and out.stride(0) >= s_kv + 256
    ref, _, inside = _dense_ref(*_fp8_values(q_fp8, kv_fp8, kv_sf), w, ks, ke)
    _check_fp32(out, ref, inside)


@pytest.mark.parametrize('kind,s,s_kv,h,d', [('noncp', 256, 1024, 64, 128), ('cp', 256, 1024, 32, 64), ('noncp', 130, 700, 8, 32),
                                              ('cp', 128, 512, 16, 128)])
@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'bf16_weights', 'compressed'])
def test_dense_reference_generators(kind, s, s_kv, h, d, mode):
    logits_dtype = torch.float32 if mode in ('fp32', 'compressed') else torch.bfloat16
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(s, s_kv, h, d, torch.bfloat16 if mode == 'bf16_weights' else torch.float32)
    ks, ke = _ks_ke(kind, s, s_kv)
    q64, kv64 = _fp8_values(q_fp8, kv_fp8, kv_sf)
    ref, mag, inside = _dense_ref(q64, kv64, w, ks, ke, with_mag=logits_dtype == torch.bfloat16)
    if mode == 'compressed':
        max_k = int((ke - ks).max())
        out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke, clean_logits=False, max_seqlen_k=max_k)
        assert out.shape == (s, max_k) and out.stride(0) % 256 == 0
        full = torch.full((s, s_kv), NEG_INF, dtype=torch.float32, device='cuda')
        cols = torch.arange(s_kv, device='cuda')
        src = (cols[None, :] - ks[:, None]).clamp(0, max_k - 1)
        full = torch.where(inside, out.gather(1, src.long()), full)
        _check_fp32(full, ref, inside)
        return
    out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke, logits_dtype)
    assert out.dtype == logits_dtype and out.stride(0) * out.element_size() % 1024 == 0
    if logits_dtype == torch.float32:
        _check_fp32(out, ref, inside)
    else:
        _check_bf16(out, ref, mag, inside)
    # the reference test's gates: unquantised inputs < 1e-3, BF16-simulated FP8 inputs < 5e-6 (FP32) / 3e-5 (BF16)
    wf = w.float()
    plain, _, _ = _dense_ref(q.double(), kv.double(), wf, ks, ke)
    sim, _, _ = _dense_ref(q_fp8.to(torch.bfloat16).double(), (kv_fp8.float() * kv_sf[:, None]).to(torch.bfloat16).double(), wf, ks, ke)
    got = out.double().masked_fill(~inside, 0)
    assert calc_diff(got, plain.masked_fill(~inside, 0)) < 1e-3
    assert calc_diff(got, sim.masked_fill(~inside, 0)) < (5e-6 if logits_dtype == torch.float32 else 3e-5)


def test_dense_empty_and_clean_rows():
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(0, 64, 64, 128)
    out = _dense_call(q_fp8, kv_fp8, kv_sf, w, torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(0, dtype=torch.int32, device='cuda'))
    assert out.shape == (0, 64)
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(5, 100, 32, 64)
    ks = torch.tensor([10, 50, 0, -5, 99], dtype=torch.int32, device='cuda')
    ke = torch.tensor([10, 20, 100, 3, 1000], dtype=torch.int32, device='cuda')
    out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    assert bool(torch.isneginf(out[:2]).all())
    assert bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(out[3, :3]).all()) and bool(torch.isneginf(out[3, 3:]).all())
    assert bool(torch.isfinite(out[4, 99:]).all()) and bool(torch.isneginf(out[4, :99]).all())


def _fresh(fn, nbytes):
    """Fill and free a NaN buffer of the result's whole allocation (nbytes: its storage, row padding included) first, so the caching
    allocator cannot hand back a buffer that already holds the answer (0xff bytes are NaN in FP32 and BF16)."""
    junk = torch.full((nbytes,), 0xff, dtype=torch.uint8, device='cuda')
    del junk
    return fn()


def test_dense_repeatable_and_schedule_independent():
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(300, 2000, 64, 128)
    ks, ke = _ks_ke('random', 300, 2000)
    call = lambda: _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    first = call()
    nbytes = first.untyped_storage().nbytes()
    for _ in range(5):
        assert torch.equal(_fresh(call, nbytes).view(torch.int32), first.view(torch.int32))
    for sms in (64, 256):
        dg.set_num_sms(sms)
        assert torch.equal(_fresh(call, nbytes).view(torch.int32), first.view(torch.int32))


def test_dense_graph_replay():
    s, s_kv = 200, 1500
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(s, s_kv, 32, 128)
    ks, ke = _ks_ke('random', s, s_kv)
    _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    for _ in range(3):
        nks, nke = _ks_ke('random', s, s_kv)
        ks.copy_(nks)
        ke.copy_(nke)
        graph.replay()
        assert torch.equal(out.view(torch.int32), _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke).view(torch.int32))


def test_dense_full_size():
    s, s_kv, h, d = 2048, 65536, 64, 128
    q, kv, w, q_fp8, kv_fp8, kv_sf = _dense_inputs(s, s_kv, h, d)
    ks, ke = _ks_ke('noncp', s, s_kv)
    out = _dense_call(q_fp8, kv_fp8, kv_sf, w, ks, ke)
    q64, kv64 = _fp8_values(q_fp8, kv_fp8, kv_sf)
    # calc_diff over column chunks, accumulated in FP64 (the whole FP64 statement would take several GB)
    xy = nn = 0.0
    for r0 in range(0, s, 512):
        rows = slice(r0, r0 + 512)
        ref, _, inside = _dense_ref(q64[rows], kv64, w[rows], ks[rows], ke[rows], chunk=2048)
        o = out[rows]
        assert torch.equal(torch.isneginf(o) & ~inside, ~inside)
        x, y = o.double().masked_fill(~inside, 0), ref.masked_fill(~inside, 0)
        xy += float((x * y).sum())
        nn += float((x * x + y * y).sum())
        del ref, inside
    assert 1 - 2 * xy / nn < 1e-8


# ---------------------------------------------------------------- paged

class Paged:
    """A paged FP8 cache with a shuffled block table.  Unused table entries name the last block, which is filled with NaN (values and
    scales): a kernel that read past a context would show NaN in a checked position instead of faulting."""

    def __init__(self, batch, next_n, h, d, block_kv, avg_ctx, pad_bytes=64, lens=None):
        self.batch, self.next_n, self.h, self.d, self.block_kv = batch, next_n, h, d, block_kv
        base = lens if lens is not None else torch.randint(max(1, int(0.7 * avg_ctx)), int(1.3 * avg_ctx) + 2, (batch,), dtype=torch.int32)
        ctx = ((base.unsqueeze(1) + 1) * torch.rand(batch, next_n)).int()
        ctx[:, -1] = base                                  # the reference's per-token lengths: the last token sees the whole row
        self.ctx = ctx.cuda()
        blocks = (base + block_kv - 1) // block_kv
        used = int(blocks.sum())
        self.max_blocks = int(blocks.max()) + 2
        self.num_blocks = used + 1
        nan_block = used
        table = torch.full((batch, self.max_blocks), nan_block, dtype=torch.int32)
        perm = torch.randperm(used, dtype=torch.int32)
        off = 0
        for b, n in enumerate(blocks.tolist()):
            table[b, :n] = perm[off:off + n]
            off += n
        self.table = table.cuda()
        kv = torch.randn(self.num_blocks, block_kv, d, device='cuda', dtype=torch.bfloat16)
        self.kv_fp8, self.sf = _cast_rows_fp8(kv)
        self.kv_fp8.view(torch.uint8)[nan_block] = 0x7f          # e4m3fn NaN
        self.sf[nan_block] = float('nan')
        self.stride0 = block_kv * (d + 4) + pad_bytes
        storage = torch.zeros(self.num_blocks, self.stride0, dtype=torch.uint8, device='cuda')
        storage[:, :block_kv * d] = self.kv_fp8.view(torch.uint8).view(self.num_blocks, -1)
        storage[:, block_kv * d:block_kv * (d + 4)] = self.sf.view(torch.uint8).view(self.num_blocks, -1)
        self.cache = storage.as_strided((self.num_blocks, block_kv, 1, d + 4), (self.stride0, d + 4, d + 4, 1))
        self.q_fp8 = torch.randn(batch, next_n, h, d, device='cuda', dtype=torch.bfloat16).to(torch.float8_e4m3fn)
        self.w = torch.randn(batch * next_n, h, device='cuda', dtype=torch.float32)
        self.max_len = self.max_blocks * block_kv

    def call(self, logits_dtype=torch.float32, weights=None):
        meta = dg.get_paged_mqa_logits_metadata(self.ctx, self.block_kv, dg.get_num_sms())
        return dg.fp8_fp4_paged_mqa_logits((self.q_fp8, None), self.cache, self.w if weights is None else weights, self.ctx, self.table, meta,
                                           self.max_len, logits_dtype=logits_dtype)

    def inside(self):
        cols = torch.arange(self.max_len, device='cuda')
        return cols[None, :] < self.ctx.view(-1, 1)

    def reference(self, w=None, with_mag=False):
        """FP64 [B * next_n, max_len] (0 outside the contexts) and mag (see _dense_ref)."""
        w = (self.w if w is None else w).double()
        out = torch.zeros(self.batch * self.next_n, self.max_len, dtype=torch.float64, device='cuda')
        mag = torch.zeros_like(out)
        span = self.ctx.max(dim=1).values.tolist()
        for b in range(self.batch):
            n = (span[b] + self.block_kv - 1) // self.block_kv
            if n == 0:
                continue
            idx = self.table[b, :n].long()
            k = (self.kv_fp8[idx].double() * self.sf[idx].double().unsqueeze(-1)).reshape(-1, self.d)
            qb = self.q_fp8[b].double()
            rows = slice(b * self.next_n, (b + 1) * self.next_n)
            out[rows, :k.shape[0]] = torch.einsum('thn,th->tn', torch.einsum('thd,nd->thn', qb, k).relu(), w[rows])
            if with_mag:
                mag[rows, :k.shape[0]] = torch.einsum('thn,th->tn', torch.einsum('thd,nd->thn', qb.abs(), k.abs()), w[rows].abs())
        inside = self.inside()
        return out.masked_fill(~inside, 0), mag.masked_fill(~inside, 0), inside


PAGED_CASES = [  # batch, next_n, block_kv, H, D, average context, cache row padding (bytes)
    (1, 1, 64, 64, 128, 1, 64), (1, 2, 32, 8, 32, 1, 4),
    (7, 1, 32, 8, 64, 77, 64), (7, 2, 32, 32, 64, 100, 4), (7, 2, 64, 16, 32, 150, 64), (7, 6, 64, 64, 128, 300, 64),
    (7, 6, 32, 8, 32, 200, 4), (7, 6, 64, 32, 128, 90, 64), (7, 6, 32, 16, 64, 333, 64),
    (256, 1, 64, 16, 128, 500, 64), (256, 2, 32, 64, 64, 300, 64), (256, 6, 64, 8, 128, 120, 64), (256, 1, 32, 32, 32, 250, 4),
    (256, 6, 64, 64, 128, 400, 64),     # next_n > 128 / H: three token groups share each KV tile through the Q staged in LDS
    (5, 20, 32, 8, 32, 90, 4),          # two groups at H = 8
    (3, 16, 64, 64, 128, 200, 64),      # a row's Q past the LDS budget: the columns are walked once per group
]


@pytest.mark.parametrize('case', PAGED_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_paged(case):
    batch, next_n, block_kv, h, d, avg, pad = case
    pg = Paged(batch, next_n, h, d, block_kv, avg, pad)
    out = pg.call()
    assert out.shape == (batch * next_n, pg.max_len) and out.stride(0) % 256 == 0 and out.stride(0) >= pg.max_len
    ref, _, inside = pg.reference()
    got = out.double().masked_fill(~inside, 0)
    assert not torch.isnan(got).any(), 'a NaN block was read'
    assert calc_diff(got, ref) < 1e-8


@pytest.mark.parametrize('mode', ['bf16', 'bf16_weights'])
def test_paged_bf16(mode):
    pg = Paged(7, 2, h=64, d=128, block_kv=64, avg_ctx=400)
    w = pg.w.to(torch.bfloat16) if mode == 'bf16_weights' else pg.w
    out = pg.call(torch.bfloat16, w)
    ref, mag, inside = pg.reference(w.float(), with_mag=True)
    assert out.dtype == torch.bfloat16 and out.stride(0) * 2 % 1024 == 0
    r = ref.to(torch.bfloat16).double()
    _, e = torch.frexp(r)
    allowed = torch.ldexp(torch.ones_like(r), e - 8) + MAG_ALLOWANCE * mag
    err = (out.double().masked_fill(~inside, 0) - r).abs()
    assert bool((err <= allowed).all())


def test_paged_repeatable_and_schedule_independent():
    pg = Paged(64, 6, h=64, d=128, block_kv=64, avg_ctx=700)        # three token groups: the LDS-staged path
    inside = pg.inside()
    raw = pg.call()
    nbytes = raw.untyped_storage().nbytes()
    first = raw.masked_fill(~inside, 0)
    for _ in range(5):
        again = _fresh(pg.call, nbytes).masked_fill(~inside, 0)
        assert torch.equal(again.view(torch.int32), first.view(torch.int32))
    results = {}
    for sms in (256, 64):
        dg.set_num_sms(sms)
        results[sms] = _fresh(pg.call, nbytes).masked_fill(~inside, 0)
    assert torch.equal(results[256].view(torch.int32), results[64].view(torch.int32))
    assert torch.equal(results[256].view(torch.int32), first.view(torch.int32))


def test_paged_graph_replay():
    pg = Paged(16, 2, h=32, d=128, block_kv=64, avg_ctx=500)
    pg.call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pg.call()
    full = pg.ctx.clone()
    for step in range(3):
        pg.ctx.copy_((full.float() * torch.rand(full.shape, device='cuda')).int() if step < 2 else full)
        graph.replay()
        inside = pg.inside()
        want = pg.call().masked_fill(~inside, 0)
        assert torch.equal(out.masked_fill(~inside, 0).view(torch.int32), want.view(torch.int32))


def test_paged_full_size():
    pg = Paged(256, 1, h=64, d=128, block_kv=64, avg_ctx=65536)
    out = pg.call()
    ref, _, inside = pg.reference()
    got = out.double().masked_fill(~inside, 0)
    assert not torch.isnan(got).any()
    assert calc_diff(got, ref) < 1e-8
