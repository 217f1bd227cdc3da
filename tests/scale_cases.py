"""FP8 GEMM operands whose scales a kernel cannot confuse with one another (plain helper module, imported like ``gpu_helpers``).

The quantisers of ``deepgemm_amd.utils`` give almost the same scale to every block of ``randn`` data (per-block UE8M0: one value for a
whole 4096 x 7168 tensor), so a kernel that reads the scale of the wrong row, K block, N block, group or packed byte returns the same
bits.  The builders here write the scales directly, from a fingerprint in which every pair of scales a kernel could swap differs by at
least a factor of two:

  * neighbouring rows of a per-token SFA, neighbouring 128-row SFB blocks, neighbouring columns of a per-column SFB;
  * neighbouring K blocks, hence also the four blocks of one packed UE8M0 word and their reversed order;
  * the same block in neighbouring groups;
  * the first and the last index of every dimension (wrap-around).

Exponent of the element at index (i_0, i_1, ...) = (sum_d c_d * seq(len_d)[i_d] + salt) mod 5 - 2, with coefficients c_d in {1, 2, 3}:
``seq`` never repeats between neighbours nor between its two ends modulo 5, and 5 is prime, so a step along any one dimension always
changes the exponent.  ``salt`` gives a second fingerprint in which every scale differs from the first one.

Two modes:
  * ``exact``: FP8 values are the integers -2 .. 2 and scales 2^-2 .. 2^2.  Every product is a multiple of 2^-4 of magnitude <= 64, so
    every partial sum of up to ``MAX_EXACT_K`` terms (plus an addend of multiples of 2^-4 within ``C_MAX``) is exact in FP32: whatever
    the accumulation order, K split or MFMA internals, a correct kernel returns exactly the FP64 value (``exact_bound`` asserts it);
  * ``spread``: FP8 values from ``randn``, FP32 scales 2^e * U(0.75, 1.25) with the same exponent fingerprint -- the FP32-scale path's
    arithmetic on scales that are not powers of two, checked against the C oracle under the ``gpu_helpers`` gates.
"""
import torch

EXP_LO, EXP_HI = -2, 2
VALUE_MAX = 2
C_MAX = 256.0


def exact_bound(k: int, c_max: float = 0.0) -> None:
    """Every partial sum of ``k`` products (and ``c``) is a multiple of 2^(2 EXP_LO) below 2^(24 + 2 EXP_LO): exact in FP32."""
    largest = k * VALUE_MAX ** 2 * 2.0 ** (2 * EXP_HI) + c_max
    assert largest <= 2.0 ** (24 + 2 * EXP_LO), f'exact mode: K = {k} (+ |c| <= {c_max}) can round in FP32'


def assert_exact(got: torch.Tensor, want64: torch.Tensor, label: str = '') -> None:
    """The exact-mode gate: FP32 outputs bit-equal to the FP64 value, BF16 outputs bit-equal to its round-to-nearest-even cast."""
    want = want64.float()
    if got.dtype == torch.bfloat16:
        want = want.bfloat16()
    else:
        assert got.dtype == torch.float32, got.dtype
    want = want.to(got.device)
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if not bool(same.all()):
        bad = (~same).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f'{label}: {bad.size(0)} of {got.numel()} elements differ from the exact value '
                             f'(first at {first}: got {got[first].item()!r}, want {want[first].item()!r})')


def seq(length: int) -> torch.Tensor:
    """0, 1, 2, 3, 4, 0, 1, ... with the last entry moved off the first one's residue where they would meet (last = 3 then: it differs
    from the first (0), its predecessor (4) and, inside a packed word, its mirror (2))."""
    s = torch.arange(length, dtype=torch.int64) % 5
    if length > 1 and (length - 1) % 5 == 0:
        s[-1] = 3
    return s


def exponents(shape, coefs, salt: int = 0) -> torch.Tensor:
    assert len(shape) == len(coefs) and all(c in (1, 2, 3) for c in coefs)
    e = torch.full(tuple(shape), salt, dtype=torch.int64)
    for d, (length, c) in enumerate(zip(shape, coefs)):
        view = [1] * len(shape)
        view[d] = length
        e = e + c * seq(length).view(view)
    return e % 5 + EXP_LO


def scales(shape, coefs, mode: str = 'exact', salt: int = 0, gen: torch.Generator = None) -> torch.Tensor:
    """FP32 scales 2^e (exact) or 2^e * U(0.75, 1.25) (spread) on the CPU."""
    sf = torch.pow(2.0, exponents(shape, coefs, salt).float())
    if mode == 'spread':
        sf = sf * (0.75 + 0.5 * torch.rand(tuple(shape), generator=gen))
    else:
        assert mode == 'exact', mode
    return sf


def values(shape, mode: str = 'exact', gen: torch.Generator = None) -> torch.Tensor:
    """FP8 e4m3 values on the CPU: integers -VALUE_MAX .. VALUE_MAX (exact) or randn (spread)."""
    if mode == 'exact':
        x = torch.randint(-VALUE_MAX, VALUE_MAX + 1, tuple(shape), generator=gen).float()
    else:
        x = torch.randn(tuple(shape), generator=gen)
    return x.to(torch.float8_e4m3fn)


def operand(mn: int, k: int, gran_mn: int = 1, gran_k: int = 128, groups: int = None, mode: str = 'exact', salt: int = 0,
            a_side: bool = True, seed: int = 0, device='cpu'):
    """(fp8 [(G,) mn, k] K-major, FP32 scales [(G,) ceil(mn / gran_mn), ceil(k / gran_k)] row-major).  A and B use different exponent
    coefficients so that a kernel that swaps the two scale tensors is caught as well."""
    gen = torch.Generator().manual_seed(seed * 2 + int(a_side))
    lead = () if groups is None else (groups,)
    sf_shape = lead + (-(-mn // gran_mn), -(-k // gran_k))
    coefs = ((3,) if groups is not None else ()) + ((1, 2) if a_side else (2, 1))
    data = values(lead + (mn, k), mode, gen)
    return data.to(device), scales(sf_shape, coefs, mode, salt, gen).to(device)


def mn_major(data: torch.Tensor) -> torch.Tensor:
    """The same logical [.., mn, k] FP8 tensor stored with unit stride along mn."""
    return data.mT.contiguous().mT


def expand_sf(sf: torch.Tensor, mn: int, k: int, gran_mn: int, gran_k: int) -> torch.Tensor:
    """Scales broadcast to one per element [.., mn, k] (float64)."""
    sf = sf.double().repeat_interleave(gran_k, dim=-1)[..., :k]
    return sf.repeat_interleave(gran_mn, dim=-2)[..., :mn, :]


def reference(a, sfa, b, sfb, gran_n: int = 128, gran_k: int = 128, c=None) -> torch.Tensor:
    """dequant(a) @ dequant(b)^T (+ c) in float64 on the operands' device; a [.., m, k], b [.., n, k] (any strides), sfa per row."""
    m, k = a.shape[-2:]
    n = b.shape[-2]
    a64 = a.double() * expand_sf(sfa, m, k, 1, gran_k)
    b64 = b.double() * expand_sf(sfb, n, k, gran_n, gran_k)
    out = a64 @ b64.mT
    return out if c is None else out + c.double()


def addend(shape, seed: int = 0, device='cpu') -> torch.Tensor:
    """An FP32 C operand that keeps exact mode exact: multiples of 2^-4 within +-C_MAX."""
    gen = torch.Generator().manual_seed(seed + 7)
    return (torch.randint(-int(C_MAX) * 16, int(C_MAX) * 16 + 1, tuple(shape), generator=gen).float() / 16).to(device)


def pack_ue8m0(sf: torch.Tensor) -> torch.Tensor:
    """FP32 power-of-two scales [.., mn, sf_k] -> packed UE8M0 words [.., mn, ceil(sf_k / 4)] int32 (byte j of word q = the exponent of
    scale block 4 q + j, zero past the last block), row-major: the public operators bring them to the MN-major layout."""
    exps = (sf.contiguous().view(torch.int32) >> 23) & 0xff
    sf_k = sf.size(-1)
    pad = -(-sf_k // 4) * 4 - sf_k
    if pad:
        exps = torch.cat([exps, torch.zeros(exps.shape[:-1] + (pad,), dtype=torch.int32, device=sf.device)], dim=-1)
    q = exps.view(exps.shape[:-1] + (-1, 4))
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)).contiguous()


def unpack_ue8m0(words: torch.Tensor, sf_k: int) -> torch.Tensor:
    shifts = torch.tensor([0, 8, 16, 24], dtype=torch.int32, device=words.device)
    exps = ((words.unsqueeze(-1) >> shifts) & 0xff).flatten(-2)[..., :sf_k]
    return (exps << 23).view(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------
# Grouped layouts
# ------------------------------------------------------------------------------------------------------------------------------------
def contiguous_layout(actual_ms, alignment: int = 128, psum: bool = False, device='cpu'):
    """(grouped_layout int32, row starts, aligned sizes): per-row group ids with -1 on padding rows, or the psum form (group ends)."""
    aligned = [-(-x // alignment) * alignment for x in actual_ms]
    starts = [sum(aligned[:g]) for g in range(len(aligned))]
    if psum:
        layout = torch.tensor([s + x for s, x in zip(starts, actual_ms)], dtype=torch.int32)
    else:
        layout = torch.full((sum(aligned),), -1, dtype=torch.int32)
        for g, (s, x) in enumerate(zip(starts, actual_ms)):
            layout[s:s + x] = g
    return layout.to(device), starts, aligned


def contiguous_case(actual_ms, n: int, k: int, mode: str = 'exact', salt: int = 0, seed: int = 0, device='cpu'):
    """M-grouped contiguous operands: a [M, k] with zero padding rows, sfa [M, sf_k], b [G, n, k], sfb [G, ceil(n / 128), sf_k]."""
    layout, starts, aligned = contiguous_layout(actual_ms)
    a, sfa = operand(sum(aligned), k, mode=mode, salt=salt, seed=seed)
    for s, x, al in zip(starts, actual_ms, aligned):
        a[s + x:s + al] = 0
    b, sfb = operand(n, k, gran_mn=128, groups=len(actual_ms), mode=mode, salt=salt, a_side=False, seed=seed)
    return tuple(t.to(device) for t in (a, sfa, b, sfb)), starts, aligned


def contiguous_reference(a, sfa, b, sfb, actual_ms, starts, gran_n: int = 128, gran_k: int = 128) -> torch.Tensor:
    """FP64 result of the valid rows, zeros on padding rows."""
    out = torch.zeros((a.size(0), b.size(1)), dtype=torch.float64, device=a.device)
    for g, (s, x) in enumerate(zip(starts, actual_ms)):
        if x:
            out[s:s + x] = reference(a[s:s + x], sfa[s:s + x], b[g], sfb[g], gran_n, gran_k)
    return out


def masked_case(groups: int, max_m: int, n: int, k: int, mode: str = 'exact', salt: int = 0, seed: int = 0, device='cpu'):
    a, sfa = operand(max_m, k, groups=groups, mode=mode, salt=salt, seed=seed)
    b, sfb = operand(n, k, gran_mn=128, groups=groups, mode=mode, salt=salt, a_side=False, seed=seed)
    return tuple(t.to(device) for t in (a, sfa, b, sfb))


def k_grouped_case(mn_a: int, mn_b: int, real_ks, k_alignment: int = 128, gran_k: int = 128, mode: str = 'exact', salt: int = 0,
                   seed: int = 0, device='cpu'):
    """K-grouped operands in the reference's psum form: MN-major a [total_k, m], b [total_k, n]; group g's rows start at the previous
    group's end rounded up to ``k_alignment`` (zeros in between); scales [sum over groups of ceil(k_g / gran_k), mn], compact, counted
    from each group's own start, fingerprinted by (group, K block, column).  Returns (a, sfa, b, sfb, ends, starts)."""
    starts, ends, end = [], [], 0
    for kg in real_ks:
        start = -(-end // k_alignment) * k_alignment
        starts.append(start)
        end = start + kg
        ends.append(end)
    total_k = -(-end // k_alignment) * k_alignment
    out = []
    for mn, a_side in ((mn_a, True), (mn_b, False)):
        gen = torch.Generator().manual_seed(seed * 2 + int(a_side))
        data = torch.zeros((total_k, mn), dtype=torch.float8_e4m3fn)
        rows = []
        for g, (kg, s) in enumerate(zip(real_ks, starts)):
            if kg == 0:
                continue
            data[s:s + kg] = values((kg, mn), mode, gen)
            blocks = -(-kg // gran_k)
            e = exponents((blocks, mn), (2, 1) if a_side else (1, 2), salt + 3 * int(seq(len(real_ks))[g]))
            sf = torch.pow(2.0, e.float())
            if mode == 'spread':
                sf = sf * (0.75 + 0.5 * torch.rand((blocks, mn), generator=gen))
            rows.append(sf)
        out += [data.to(device), (torch.cat(rows) if rows else torch.empty((0, mn))).to(device)]
    return out[0], out[1], out[2], out[3], ends, starts


def k_grouped_reference(a, sfa, b, sfb, real_ks, starts, gran_k: int = 128, c=None) -> torch.Tensor:
    """[G, m, n] float64: c[g] + dequant(a_g)^T @ dequant(b_g) per group (scale rows counted from the group's own start)."""
    out = torch.zeros((len(real_ks), a.size(1), b.size(1)), dtype=torch.float64, device=a.device)
    row = 0
    for g, (kg, s) in enumerate(zip(real_ks, starts)):
        if kg == 0:
            continue
        blocks = -(-kg // gran_k)
        ea = sfa[row:row + blocks].double().repeat_interleave(gran_k, 0)[:kg]
        eb = sfb[row:row + blocks].double().repeat_interleave(gran_k, 0)[:kg]
        out[g] = (a[s:s + kg].double() * ea).t() @ (b[s:s + kg].double() * eb)
        row += blocks
    return out if c is None else out + c.double()
