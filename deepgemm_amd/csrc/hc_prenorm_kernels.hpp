// CDNA4 (gfx950) device code of the hyper-connection pre-norm GEMM (reference: csrc/apis/hyperconnection.hpp tf32_hc_prenorm_gemm).
//
// What it computes, for A [m, k] BF16 and B [n, k] FP32 (both K-major), split s of the reference's K partition:
//   d[s][i][j] = sum_{kk in split s} a[i][kk] * b[j][kk]        sqr_sum[s][i] = sum_{kk in split s} a[i][kk]^2
// The K partition is the reference's (sm90_tf32_hc_prenorm_gemm.cuh, k_offset): K in blocks of 64; split s of S gets KB / S blocks, the
// first KB % S splits one more; a split without blocks writes zeros.
// How it is built:
//   * gfx950 has no TF32 / xf32 MFMA, and the exact FP32 one (16x16x4) runs at 1/16 of the BF16 rate.  A is exact in BF16, so only B needs
//     more than BF16: each FP32 b is split in registers into b_hi = bf16(b) and b_lo = bf16(b - b_hi) (both round to nearest even), and
//     every fragment pair feeds four v_mfma_f32_16x16x32_bf16 (hi and lo, two K halves) accumulating in FP32.  The products are exact;
//     |b - b_hi - b_lo| <= 2^-16 |b|, far below TF32's 2^-11.  Non-finite b is outside the contract (inf - inf gives NaN);
//   * B rows (n, padded to 16 or 32) go to the MFMA's A slot and A rows (tokens) to its B slot: in the C/D map (col = lane & 15,
//     row = 4 * (lane >> 4) + reg) a lane owns one token row and four consecutive n;
//   * sqr_sum runs on the VALU from the same A registers (FMAs of exact BF16 squares), so A is read once;
//   * operands go global -> registers with buffer loads (rows past m or n, and nothing else, are out of range and read as zeros); lane
//     (r, g) holds the 16 contiguous K values [16 g, 16 g + 16) of a 64-value block of row r, for both operands -- a K permutation the
//     operands share.  The next K block is loaded while the current one is multiplied;
//   * a workgroup is a tile of 16 * MS rows and one K piece; its 4 waves take the piece's K blocks round-robin (neighbouring waves read
//     neighbouring 128 bytes of each row) and every wave multiplies all rows of the tile, so a B block is split once per workgroup.  The
//     waves' partial sums meet in LDS and are added in wave order: every result is one fixed reduction for a given launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dg {
namespace hc {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

constexpr int kWaves = 4;
constexpr int kBlockK = 64;
constexpr int kSumBatch = 16;             // pieces whose loads the sum launch issues together
constexpr unsigned kOob = 0x80000000u;      // a voffset past every buffer range: the load returns zeros

struct HcParams {
    const uint8_t* a;                   // [m, k] BF16, row stride a_stride elements
    const float* b;                     // [n, k] FP32, row stride b_stride elements
    float* d;                           // split s, row i at d + s * d_ss + i * d_sm
    float* s;                           // split s at s + s * s_ss
    int64_t a_stride, b_stride, d_sm, d_ss, s_ss;
    int m, n, k;
    int tiles;                          // row tiles of 16 * MS rows
    int splits;                         // K pieces (the caller's splits, or the internal cut of a num_splits=None call)
    int d_vec;                          // d, d_sm and d_ss allow 16-byte stores
};

// acc += the 16 x 16 tile of one 64-value K block for one B operand (hi or lo): two K halves
__device__ __forceinline__ void mfma_k64(v4f& acc, const v8i& w, const v8i& x) {
    const v4i w0 = __builtin_shufflevector(w, w, 0, 1, 2, 3), w1 = __builtin_shufflevector(w, w, 4, 5, 6, 7);
    const v4i x0 = __builtin_shufflevector(x, x, 0, 1, 2, 3), x1 = __builtin_shufflevector(x, x, 4, 5, 6, 7);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, w0), __builtin_bit_cast(v8bf, x0), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, w1), __builtin_bit_cast(v8bf, x1), acc, 0, 0, 0);
}

// 16 FP32 values -> their BF16 high parts and BF16 residuals, packed in the K order of the A fragment (element 2j in the low half of
// dword j)
__device__ __forceinline__ void split_b(const v4f (&raw)[4], v8i& hi, v8i& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x0 = raw[j >> 1][(2 * j) & 3], x1 = raw[j >> 1][(2 * j + 1) & 3];
        v2bf h;
        h[0] = static_cast<__bf16>(x0);
        h[1] = static_cast<__bf16>(x1);
        const uint32_t hb = __builtin_bit_cast(uint32_t, h);
        v2bf l;
        l[0] = static_cast<__bf16>(x0 - __builtin_bit_cast(float, hb << 16));
        l[1] = static_cast<__bf16>(x1 - __builtin_bit_cast(float, hb & 0xffff0000u));
        hi[j] = static_cast<int>(hb);
        lo[j] = __builtin_bit_cast(int, l);
    }
}

// sum of the squares of the 16 BF16 values of a fragment: exact squares, FP32 sums (v_dot2_f32_bf16 is not exact here: it rounds)
__device__ __forceinline__ float sqr_k16(const v8i& x) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float lo = __builtin_bit_cast(float, static_cast<uint32_t>(x[j]) << 16);
        const float hi = __builtin_bit_cast(float, static_cast<uint32_t>(x[j]) & 0xffff0000u);
        s0 = __builtin_fmaf(lo, lo, s0);
        s1 = __builtin_fmaf(hi, hi, s1);
    }
    return s0 + s1;
}

template <int MS, int NS>
__global__ __launch_bounds__(kWaves * 64)
void dg_hc_prenorm_gemm_kernel(const HcParams p) {
    constexpr int R = MS * 16;
    constexpr int SLOTS = MS * NS * 4 + MS;
    __shared__ float red[kWaves][SLOTS][64];

    const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x % p.tiles, split = blockIdx.x / p.tiles;
    const int kb_total = p.k / kBlockK, per = kb_total / p.splits, rem = kb_total % p.splits;
    const int kb0 = split * per + (split < rem ? split : rem), nkb = per + (split < rem ? 1 : 0);
    const int m0 = tile * R, rows = (p.m - m0 < R) ? p.m - m0 : R;

    // bases at the piece's first K block; the host keeps every in-range offset below 2^31
    const uint8_t* a_base = p.a + (static_cast<int64_t>(m0) * p.a_stride + static_cast<int64_t>(kb0) * kBlockK) * 2;
    const float* b_base = p.b + static_cast<int64_t>(kb0) * kBlockK;
    const int k_left = p.k - kb0 * kBlockK;
    const auto a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a_base), 0,
                                                          static_cast<int>((rows - 1) * p.a_stride * 2 + k_left * 2), 0x00020000);
    const auto b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b_base), 0,
                                                          static_cast<int>(((p.n - 1) * p.b_stride + k_left) * 4), 0x00020000);
    int a_off[MS], b_off[NS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
        a_off[ms] = (ms * 16 + r16 < rows) ? static_cast<int>((ms * 16 + r16) * p.a_stride * 2) + g * 32 : static_cast<int>(kOob);
#pragma unroll
    for (int ns = 0; ns < NS; ++ns)
        b_off[ns] = (ns * 16 + r16 < p.n) ? static_cast<int>((ns * 16 + r16) * p.b_stride * 4) + g * 64 : static_cast<int>(kOob);

    v4f acc[MS][NS];
    float sq[MS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
        sq[ms] = 0.f;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
            acc[ms][ns] = v4f{0.f, 0.f, 0.f, 0.f};
    }

    // K block j of the piece: A fragments (32 bytes per lane and row tile) and raw B (64 bytes per lane and n tile); A is streamed (nt),
    // B stays in L2 for the other row tiles
    auto load = [&](v8i (&af)[MS], v4f (&bf)[NS][4], int j) {
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
            const v4i x0 = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_off[ms], j * 128, 2));
            const v4i x1 = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_off[ms], j * 128 + 16, 2));
            af[ms] = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                bf[ns][c] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_off[ns], j * 256 + c * 16, 0));
    };
    auto compute = [&](const v8i (&af)[MS], const v4f (&bf)[NS][4]) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            v8i hi, lo;
            split_b(bf[ns], hi, lo);
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
                mfma_k64(acc[ms][ns], hi, af[ms]);
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
                mfma_k64(acc[ms][ns], lo, af[ms]);
        }
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
            sq[ms] += sqr_k16(af[ms]);
    };

    // two register sets, ping-pong; the load after the last block re-reads that block (an L2 hit) so the loop body has no branch
    int j = wave;
    if (j < nkb) {
        v8i a0[MS], a1[MS];
        v4f b0[NS][4], b1[NS][4];
        load(a0, b0, j);
        while (true) {
            load(a1, b1, (j + kWaves < nkb) ? j + kWaves : nkb - 1);
            __builtin_amdgcn_sched_barrier(0);          // (keep the next block's loads ahead of this block's math)
            compute(a0, b0);
            j += kWaves;
            if (j >= nkb)
                break;
            load(a0, b0, (j + kWaves < nkb) ? j + kWaves : nkb - 1);
            __builtin_amdgcn_sched_barrier(0);
            compute(a1, b1);
            j += kWaves;
            if (j >= nkb)
                break;
        }
    }

#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                red[wave][(ms * NS + ns) * 4 + i][lane] = acc[ms][ns][i];
        red[wave][MS * NS * 4 + ms][lane] = sq[ms];
    }
    __syncthreads();

    // wave w stores row tiles w, w + 4, ...: the waves' partials are added in wave order, the four lane groups' squares in group order
    float* d_split = p.d + static_cast<int64_t>(split) * p.d_ss;
    for (int ms = wave; ms < MS; ms += kWaves) {
        const int row = m0 + ms * 16 + r16;
        if (row >= p.m)
            continue;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int col = ns * 16 + g * 4;
            if (col >= p.n)
                continue;
            v4f v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t = red[0][(ms * NS + ns) * 4 + i][lane];
#pragma unroll
                for (int w = 1; w < kWaves; ++w)
                    t += red[w][(ms * NS + ns) * 4 + i][lane];
                v[i] = t;
            }
            float* dst = d_split + static_cast<int64_t>(row) * p.d_sm + col;
            if (p.d_vec) {
                *reinterpret_cast<v4f*>(dst) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dst[i] = v[i];
            }
        }
        if (g == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    t += red[w][MS * NS * 4 + ms][q * 16 + r16];
            p.s[static_cast<int64_t>(split) * p.s_ss + row] = t;
        }
    }
}

#ifndef DG_SHARD_TU   // (plain kernels: defined once, in the dg_api.hip translation unit -- see kernel_instances.inc)
// Second launch of an internal K cut: d[i][j] = sum over pieces q in order of ws[q][i][j], sqr_sum[i] = sum over q of ws_s[q][i], with
// ws [pieces][m][n] FP32 followed by ws_s [pieces][m].  The loads of kSumBatch pieces are issued together and then added in order.
__global__ __launch_bounds__(256)
void dg_hc_prenorm_sum_kernel(const float* __restrict__ ws, int pieces, int m, int n, float* d, int64_t d_sm, float* s) {
    const int64_t slab = static_cast<int64_t>(m) * n;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < slab + m; e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        // element e of the [m][n] slab, or row e - slab of the [m] vector behind the pieces' slabs
        const float* src = e < slab ? ws + e : ws + pieces * slab + (e - slab);
        const int64_t stride = e < slab ? slab : m;
        float t = -0.f;
        for (int q0 = 0; q0 < pieces; q0 += kSumBatch) {
            float v[kSumBatch];
#pragma unroll
            for (int u = 0; u < kSumBatch; ++u)
                v[u] = q0 + u < pieces ? src[(q0 + u) * stride] : -0.f;
#pragma unroll
            for (int u = 0; u < kSumBatch; ++u)
                t += v[u];
        }
        if (e < slab) {
            const int r = static_cast<int>(e / n), c = static_cast<int>(e - static_cast<int64_t>(r) * n);
            d[static_cast<int64_t>(r) * d_sm + c] = t;
        } else {
            s[e - slab] = t;
        }
    }
}
#endif

}  // namespace hc
}  // namespace dg
