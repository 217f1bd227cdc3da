// CDNA4 (gfx950) device code of the indexer MQA logits (reference: csrc/apis/attention.hpp fp8_fp4_mqa_logits /
// fp8_fp4_paged_mqa_logits / get_paged_mqa_logits_metadata, FP8 operands only).
//
// What it computes, for every (token i, KV column j) the caller asks for:
//   logits[i, j] = sum_h w[i, h] * relu(sf[j] * sum_d q[i, h, d] * kv[j, d])
// How it is built:
//   * the Q rows of a wave are (token, head) pairs, token-major: one 16-row M tile holds 16 / H tokens (H = 8) or 16 heads of one token
//     (H >= 16).  They feed the MFMA's A slot and 16 KV rows its B slot, so in the C/D map (col = lane & 15, row = 4 * (lane >> 4) + reg)
//     every lane owns ONE KV column and four consecutive heads of one token: the head reduction is 4 in-lane terms, then a sum over the
//     M tiles of the token, then (H >= 16) two xor-shuffles over the lane groups -- a fixed tree, so every element is one fixed reduction
//     over D (inside the MFMA) and H, whatever the work split;
//   * per element that is one v_med3_f32 and one v_fma_f32: sf * relu-or-clamp.  relu(sf * s) = sf * med3(s, 0, sign(sf) * inf), so the
//     scale multiplies the head sum once per column instead of once per head;
//   * D = 128 runs one v_mfma_f32_16x16x128_f8f6f4 per 16x16 tile, D = 64 / 32 two / one v_mfma_f32_16x16x32_fp8_fp8.  Lane (r, g) of a
//     fragment holds the D / 4 contiguous bytes [g * D / 4, (g + 1) * D / 4) of row r, for both operands: a K permutation the two operands
//     share, so the contraction is the full dot product;
//   * operands go global -> registers (no LDS): the Q fragments and weights of a wave stay in registers for its whole KV range, the KV
//     fragments of the next 16 columns are loaded while the current ones are multiplied.  Waves of one workgroup walk the same KV rows
//     at about the same time and share them through the L1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dg {
namespace mqa {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
// 4-byte aligned vector views: a paged cache block may start at any multiple of 4 bytes (kv_cache.stride(0) % 4 == 0)
typedef int v4i_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int v2i_a4 __attribute__((ext_vector_type(2), aligned(4)));

constexpr int kDenseWaves = 4;          // one 128-row Q block per wave
constexpr int kPagedWaves = 8;          // waves of one persistent paged workgroup split the KV columns of a batch row
constexpr int kPagedSplit = 256;        // KV columns per schedule unit (get_paged_mqa_logits_metadata)
constexpr int kCleanCols = 1024;        // columns per workgroup of the clean kernel

struct MqaParams {
    const uint8_t* q;                   // dense [S, H, D]; paged [B, N, H, D]
    const uint8_t* kv;                  // dense [S_kv, D]; paged: the fused cache, block b at kv + b * kv_block_stride
    const float* kv_sf;                 // dense [S_kv]
    const void* weights;                // [rows, H] FP32 or BF16, row stride w_stride elements
    const int32_t* ks;                  // dense [S]
    const int32_t* ke;                  // dense [S]
    const int32_t* context_lens;        // paged [B, N]
    const int32_t* block_table;         // paged [B, max_blocks], row stride block_table_stride
    const int32_t* schedule;            // paged [num_wg + 1, 2]
    void* logits;                       // row stride logits_stride elements
    int64_t logits_stride, w_stride, kv_block_stride, block_table_stride;
    int seq_len, seq_len_kv, max_seqlen_k, kv_chunk;            // dense; max_seqlen_k > 0: compressed rows
    int batch, next_n, block_kv, max_blocks, max_context_len;   // paged
    int logits_bf16, weights_bf16;
};

__device__ __forceinline__ float bf16_bits_to_float(uint16_t v) { return __uint_as_float(static_cast<uint32_t>(v) << 16); }

// round to nearest even, once (NaN stays NaN)
__device__ __forceinline__ uint16_t float_to_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u)
        return static_cast<uint16_t>((u >> 16) | 0x40u);
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ void store_logit(const MqaParams& p, int64_t offset, float v) {
    if (p.logits_bf16)
        static_cast<uint16_t*>(p.logits)[offset] = float_to_bf16_rne(v);
    else
        static_cast<float*>(p.logits)[offset] = v;
}

// The D / 4 bytes of one fragment (lane group g's share of a row).
template <int D>
__device__ __forceinline__ void load_frag(const uint8_t* src, int (&f)[D / 16]) {
    if constexpr (D == 128) {
        const v4i_a4 a = reinterpret_cast<const v4i_a4*>(src)[0], b = reinterpret_cast<const v4i_a4*>(src)[1];
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    } else if constexpr (D == 64) {
        const v4i_a4 a = reinterpret_cast<const v4i_a4*>(src)[0];
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
    } else {
        const v2i_a4 a = reinterpret_cast<const v2i_a4*>(src)[0];
        f[0] = a[0]; f[1] = a[1];
    }
}

// acc[r] = sum_d Q[row 4 * (lane >> 4) + r][d] * KV[col lane & 15][d] of one 16 x 16 tile
template <int D>
__device__ __forceinline__ v4f tile_dot(const int (&a)[D / 16], const int (&b)[D / 16]) {
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (D == 128) {
        const v8i av = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
        const v8i bv = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]};
        // zero scale operands: the unscaled e4m3 x e4m3 encoding (cbsz = blgp = 0)
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, zero, 0, 0, 0, 0, 0, 0);
    } else {
        v4f acc = zero;
#pragma unroll
        for (int c = 0; c < D / 32; ++c) {
            const long al = static_cast<long>(static_cast<uint32_t>(a[2 * c])) | (static_cast<long>(a[2 * c + 1]) << 32);
            const long bl = static_cast<long>(static_cast<uint32_t>(b[2 * c])) | (static_cast<long>(b[2 * c + 1]) << 32);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(al, bl, acc, 0, 0, 0);
        }
        return acc;
    }
}

// The Q side of one wave: MT 16-row tiles = TOK tokens x H heads (token-major), their fragments and the matching weights.
template <int H, int D, int MT>
struct QGroup {
    static constexpr int TOK = MT * 16 / H;
    static_assert(MT * 16 % H == 0 && H % 4 == 0, "a token's heads fill whole lane groups");
    int qf[MT][D / 16];
    float w[MT][4];

    // q_tok0: row (token 0, head 0) of the group; w_row0: its weight row index; tokens >= n_tok are padding (clamped loads, zero weight)
    __device__ __forceinline__ void load(const MqaParams& p, const uint8_t* q_tok0, int64_t w_row0, int n_tok, int lane) {
        const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int row = m * 16 + r16, tok = min(row / H, n_tok - 1);
            load_frag<D>(q_tok0 + (static_cast<int64_t>(tok) * H + row % H) * D + g * (D / 4), qf[m]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int wrow = m * 16 + 4 * g + i, wt = wrow / H;
                const int64_t off = (w_row0 + min(wt, n_tok - 1)) * p.w_stride + wrow % H;
                const float v = p.weights_bf16 ? bf16_bits_to_float(static_cast<const uint16_t*>(p.weights)[off])
                                               : static_cast<const float*>(p.weights)[off];
                w[m][i] = wt < n_tok ? v : 0.f;
            }
        }
    }

    // The same from the row's Q staged in LDS (pitch `pitch` bytes per (token, head) row) and its weights as FP32; tok_base: the group's
    // first token within the row.
    __device__ __forceinline__ void load_lds(const uint8_t* lds_q, const float* lds_w, int pitch, int tok_base, int n_tok, int lane) {
        const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int row = m * 16 + r16, tok = min(row / H, n_tok - 1);
            load_frag<D>(lds_q + ((tok_base + tok) * H + row % H) * pitch + g * (D / 4), qf[m]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int wrow = m * 16 + 4 * g + i, wt = wrow / H;
                const float v = lds_w[(tok_base + min(wt, n_tok - 1)) * H + wrow % H];
                w[m][i] = wt < n_tok ? v : 0.f;
            }
        }
    }

    // The logits of the 16 KV columns whose fragment is kvf (this lane's column has scale sf): store(t, value) is called by the lanes
    // that hold token t's value, one lane group per token, each lane for its own column.
    template <typename Store>
    __device__ __forceinline__ void score(const int (&kvf)[D / 16], float sf, int lane, Store&& store) const {
        const int g = lane >> 4;
        const float bound = sf >= 0.f ? __builtin_huge_valf() : -__builtin_huge_valf();
        v4f acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            acc[m] = tile_dot<D>(qf[m], kvf);
        if constexpr (H >= 16) {
            constexpr int TILES = H / 16;
#pragma unroll
            for (int t = 0; t < TOK; ++t) {
                float part = 0.f;
#pragma unroll
                for (int m = t * TILES; m < (t + 1) * TILES; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        part = __builtin_fmaf(__builtin_amdgcn_fmed3f(acc[m][i], 0.f, bound), w[m][i], part);
                part += __shfl_xor(part, 16);
                part += __shfl_xor(part, 32);
                if (g == (t & 3))
                    store(t, part * sf);
            }
        } else {                                    // H == 8: lane groups 0, 1 hold token 2m, groups 2, 3 token 2m + 1
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    part = __builtin_fmaf(__builtin_amdgcn_fmed3f(acc[m][i], 0.f, bound), w[m][i], part);
                part += __shfl_xor(part, 16);
                if ((g & 1) == 0)
                    store(2 * m + (g >> 1), part * sf);
            }
        }
    }
};

// Dense (prefill) form.  Workgroup (x, y): Q blocks 4x .. 4x + 3 (one per wave, 128 / H tokens each) against KV columns
// [y * kv_chunk, (y + 1) * kv_chunk), cut to the union of the wave's [ks, ke) ranges.  Writes only columns inside a token's own range.
template <int H, int D>
__global__ __launch_bounds__(kDenseWaves * 64) void dg_mqa_logits_kernel(const MqaParams p) {
    constexpr int MT = 8;
    using QG = QGroup<H, D, MT>;
    constexpr int TOK = QG::TOK;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int tok0 = (blockIdx.x * kDenseWaves + wave) * TOK;
    if (tok0 >= p.seq_len)
        return;
    const int n_tok = min(TOK, p.seq_len - tok0);
    int ks[TOK], ke[TOK];
    int lo = p.seq_len_kv, hi = 0;
#pragma unroll
    for (int t = 0; t < TOK; ++t) {
        const bool valid = t < n_tok;
        ks[t] = valid ? max(p.ks[tok0 + (valid ? t : 0)], 0) : 0;
        ke[t] = valid ? min(p.ke[tok0 + (valid ? t : 0)], p.seq_len_kv) : 0;
        if (ks[t] < ke[t]) {
            lo = min(lo, ks[t]);
            hi = max(hi, ke[t]);
        }
    }
    const int c0 = blockIdx.y * p.kv_chunk;
    lo = max(lo, c0) & ~15;
    hi = min(hi, min(c0 + p.kv_chunk, p.seq_len_kv));
    if (lo >= hi)
        return;

    QG qg;
    qg.load(p, p.q + static_cast<int64_t>(tok0) * H * D, tok0, n_tok, lane);
    const int last_row = p.seq_len_kv - 1;
    int kvf[D / 16];
    load_frag<D>(p.kv + static_cast<int64_t>(min(lo + r16, last_row)) * D + g * (D / 4), kvf);
    float sf = p.kv_sf[min(lo + r16, last_row)];
    for (int j0 = lo; j0 < hi; j0 += 16) {
        int nf[D / 16];
        const int nrow = min(j0 + 16 + r16, last_row);
        load_frag<D>(p.kv + static_cast<int64_t>(nrow) * D + g * (D / 4), nf);
        const float nsf = p.kv_sf[nrow];
        const int col = j0 + r16;
        qg.score(kvf, sf, lane, [&](int t, float v) {
            int s = 0, e = 0;
#pragma unroll
            for (int u = 0; u < TOK; ++u)
                if (u == t) { s = ks[u]; e = ke[u]; }
            if (col >= s && col < e) {
                const int dst = p.max_seqlen_k > 0 ? col - p.ks[tok0 + t] : col;
                if (p.max_seqlen_k == 0 || dst < p.max_seqlen_k)
                    store_logit(p, static_cast<int64_t>(tok0 + t) * p.logits_stride + dst, v);
            }
        });
#pragma unroll
        for (int k = 0; k < D / 16; ++k)
            kvf[k] = nf[k];
        sf = nsf;
    }
}

__device__ __forceinline__ int paged_span(const MqaParams& p, int b) {
    int len = 0;
    for (int t = 0; t < p.next_n; ++t)
        len = max(len, p.context_lens[static_cast<int64_t>(b) * p.next_n + t]);
    return len;
}

// schedule units of row b (256-column pieces of its longest context); no int overflow near INT_MAX
__device__ __forceinline__ int paged_units(const MqaParams& p, int b) {
    const int span = paged_span(p, b);
    return span / kPagedSplit + (span % kPagedSplit != 0);
}

#ifndef DG_SHARD_TU   // (plain kernels: defined once, in the dg_api.hip translation unit -- see kernel_instances.inc)
// -inf outside [max(ks, 0), min(ke, S_kv)) of every row (uncompressed dense logits); the main kernel writes the inside.
__global__ __launch_bounds__(256) void dg_mqa_clean_logits_kernel(const MqaParams p) {
    const int row = blockIdx.x;                          // rows on x (no 65535 limit), column chunks strided over y
    const int s = max(p.ks[row], 0), e = min(p.ke[row], p.seq_len_kv);
    for (int64_t c0 = static_cast<int64_t>(blockIdx.y) * kCleanCols; c0 < p.seq_len_kv; c0 += static_cast<int64_t>(gridDim.y) * kCleanCols) {
        if (s < e && c0 >= s && c0 + kCleanCols <= e)
            continue;
        const int c1 = static_cast<int>(min(c0 + kCleanCols, static_cast<int64_t>(p.seq_len_kv)));
        for (int c = static_cast<int>(c0) + static_cast<int>(threadIdx.x); c < c1; c += 256)
            if (c < s || c >= e)
                store_logit(p, static_cast<int64_t>(row) * p.logits_stride + c, -__builtin_huge_valf());
    }
}

// Schedule of the paged kernel: unit u of batch row b = KV columns [u * 256, (u + 1) * 256) of its longest context.  The units of all
// rows, in order, are cut into num_wg equal shares; entry i = (row, unit) where share i starts, entry num_wg = (batch, 0).  One
// workgroup, no host involvement: the schedule can be captured in a graph with the logits call.
__global__ __launch_bounds__(1024) void dg_paged_mqa_logits_metadata_kernel(const int32_t* context_lens, int32_t* schedule, int batch,
                                                                           int next_n, int num_wg) {
    __shared__ int64_t scan[1024];
    __shared__ int64_t total_s;
    const int tid = threadIdx.x;
    MqaParams p{};
    p.context_lens = context_lens;
    p.next_n = next_n;
    int64_t total = 0;
    for (int base = 0; base < batch; base += 1024) {     // pass 1: the number of units
        const int b = base + tid;
        scan[tid] = b < batch ? paged_units(p, b) : 0;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) {
            if (tid < s)
                scan[tid] += scan[tid + s];
            __syncthreads();
        }
        total += scan[0];
        __syncthreads();
    }
    if (tid == 0)
        total_s = total;
    __syncthreads();
    total = total_s;
    if (total == 0) {
        for (int i = tid; i <= num_wg; i += 1024) {
            schedule[2 * i] = batch;
            schedule[2 * i + 1] = 0;
        }
        return;
    }
    int64_t running = 0;
    for (int base = 0; base < batch; base += 1024) {     // pass 2: share i starts at unit floor(i * total / num_wg)
        const int b = base + tid;
        const int64_t units = b < batch ? paged_units(p, b) : 0;
        scan[tid] = units;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {       // inclusive Hillis-Steele scan
            const int64_t v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int64_t first = running + scan[tid] - units;
        if (units > 0) {
            for (int64_t i = (first * num_wg + total - 1) / total; i < num_wg && i * total / num_wg < first + units; ++i) {
                schedule[2 * i] = b;
                schedule[2 * i + 1] = static_cast<int>(i * total / num_wg - first);
            }
        }
        running += scan[1023];
        __syncthreads();
    }
    if (tid == 0) {
        schedule[2 * num_wg] = batch;
        schedule[2 * num_wg + 1] = 0;
    }
}
#endif

// Paged (decode) form.  Workgroup i walks the schedule units [schedule[i], schedule[i + 1]); inside one batch row its waves take the
// 16-column tiles round-robin.  A row's next_n tokens are walked in groups of 128 / H (MT tiles).  One group: its Q fragments and weights
// stay in registers for the whole row.  Several groups (next_n > 128 / H): the row's Q and weights are staged in LDS once and every KV
// tile, loaded once, is multiplied by each group in turn -- a KV tile is read from memory once for all tokens and heads of its row as
// long as the row's Q fits kPagedQLds (next_n * H * (D + 20) bytes, next_n <= 13 at H = 64, D = 128) and H >= 16; past that (and at
// H = 8 past next_n = 16) the row's columns are walked once per group.  Block-table
// entries are read only for columns below the row's longest context.
constexpr int kPagedQLds = 128 * 1024;

template <int H, int D, int MT>
__global__ __launch_bounds__(kPagedWaves * 64) void dg_paged_mqa_logits_kernel(const MqaParams p) {
    using QG = QGroup<H, D, MT>;
    constexpr int TOK = QG::TOK;
    constexpr int QROW = D + 16;                            // LDS pitch of a staged Q row: 16 bytes of skew per row
    // only the MT = 8 kernels are launched with more than one token group (dg_api.hip picks the smallest MT that holds next_n)
    __shared__ __attribute__((aligned(16))) uint8_t lds[MT == 8 && H >= 16 ? kPagedQLds : 16];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int b_begin = p.schedule[2 * blockIdx.x], u_begin = p.schedule[2 * blockIdx.x + 1];
    const int b_end = p.schedule[2 * blockIdx.x + 2], u_end = p.schedule[2 * blockIdx.x + 3];
    const int max_cols = min(p.max_context_len, p.max_blocks * p.block_kv);
    const int bkv_shift = p.block_kv == 64 ? 6 : 5;
    const int groups = (p.next_n + TOK - 1) / TOK;
    const int row_q = p.next_n * H;
    // (H = 8 keeps one path: 16 tokens of a group leave no registers for a second copy of the tile loop; it has several groups only
    // past next_n = 16)
    constexpr bool kStaging = MT == 8 && H >= 16;
    const bool staged = kStaging && groups > 1 && static_cast<int64_t>(row_q) * (QROW + 4) <= kPagedQLds;
    for (int b = b_begin; b <= b_end && b < p.batch; ++b) {
        const int span = paged_span(p, b);
        const int c_begin = b == b_begin ? static_cast<int>(min(static_cast<int64_t>(u_begin) * kPagedSplit, static_cast<int64_t>(span))) : 0;
        const int c_end = static_cast<int>(min(b == b_end ? static_cast<int64_t>(u_end) * kPagedSplit : span, static_cast<int64_t>(min(span, max_cols))));
        if (c_begin >= c_end)
            continue;
        const int32_t* table = p.block_table + static_cast<int64_t>(b) * p.block_table_stride;
        const int64_t row_b = static_cast<int64_t>(b) * p.next_n;

        // The wave's tiles of this row: tile(kvf, sf, col) for columns j0 + r16, j0 = c_begin + 16 * wave (+ 16 * kPagedWaves ...); the
        // next tile's fragment is loaded while the current one is used.  Tile j: block table entry j / block_kv (a 16-column tile never
        // straddles a block), row j % block_kv + r16 of that block.
        auto walk_tiles = [&](auto&& tile) {
            int j0 = c_begin + wave * 16;
            if (j0 >= c_end)
                return;
            auto tile_ptr = [&](int j) {
                const int64_t blk = table[j >> bkv_shift];
                return p.kv + blk * p.kv_block_stride;
            };
            const uint8_t* base = tile_ptr(j0);
            int kvf[D / 16];
            const int rin = (j0 & (p.block_kv - 1)) + r16;
            load_frag<D>(base + rin * D + g * (D / 4), kvf);
            float sf = reinterpret_cast<const float*>(base + p.block_kv * D)[rin];
            for (; j0 < c_end; j0 += 16 * kPagedWaves) {
                const int jn = min(j0 + 16 * kPagedWaves, c_end - 1);       // clamped: never a table entry past the context
                const uint8_t* nbase = tile_ptr(jn);
                const int nrin = (jn & (p.block_kv - 16)) + r16;
                int nf[D / 16];
                load_frag<D>(nbase + nrin * D + g * (D / 4), nf);
                const float nsf = reinterpret_cast<const float*>(nbase + p.block_kv * D)[nrin];
                tile(kvf, sf, j0 + r16);
#pragma unroll
                for (int k = 0; k < D / 16; ++k)
                    kvf[k] = nf[k];
                sf = nsf;
            }
        };
        // the context lengths of group t0's tokens (0 for padding tokens)
        auto group_ctx = [&](int t0, int (&ctx)[TOK]) {
            const int n_tok = min(TOK, p.next_n - t0);
#pragma unroll
            for (int t = 0; t < TOK; ++t)
                ctx[t] = t < n_tok ? min(p.context_lens[row_b + t0 + (t < n_tok ? t : 0)], p.max_context_len) : 0;
        };
        // group t0's logits of one tile
        auto score_group = [&](const QG& qg, int t0, const int (&ctx)[TOK], const int (&kvf)[D / 16], float sf, int col) {
            qg.score(kvf, sf, lane, [&](int t, float v) {
                int c = 0;
#pragma unroll
                for (int u = 0; u < TOK; ++u)
                    if (u == t) c = ctx[u];
                if (col < c)
                    store_logit(p, (row_b + t0 + t) * p.logits_stride + col, v);
            });
        };

        if constexpr (kStaging) {
            if (staged) {
                float* lds_w = reinterpret_cast<float*>(lds + row_q * QROW);
                __syncthreads();                                                // the previous row's readers are done
                const uint8_t* q_src = p.q + row_b * H * D;
                for (int i = threadIdx.x; i < row_q * (D / 16); i += kPagedWaves * 64) {
                    const int r = i / (D / 16), c = i % (D / 16);
                    *reinterpret_cast<v4i_a4*>(lds + r * QROW + c * 16) = *reinterpret_cast<const v4i_a4*>(q_src + static_cast<int64_t>(r) * D + c * 16);
                }
                for (int i = threadIdx.x; i < row_q; i += kPagedWaves * 64) {
                    const int64_t off = (row_b + i / H) * p.w_stride + i % H;
                    lds_w[i] = p.weights_bf16 ? bf16_bits_to_float(static_cast<const uint16_t*>(p.weights)[off])
                                                  : static_cast<const float*>(p.weights)[off];
                }
                __syncthreads();
                walk_tiles([&](const int (&kvf)[D / 16], float sf, int col) {
                    for (int t0 = 0; t0 < p.next_n; t0 += TOK) {
                        QG qg;
                        qg.load_lds(lds, lds_w, QROW, t0, min(TOK, p.next_n - t0), lane);
                        int ctx[TOK];
                        group_ctx(t0, ctx);
                        score_group(qg, t0, ctx, kvf, sf, col);
                    }
                });
                continue;
            }
        }
        for (int t0 = 0; t0 < p.next_n; t0 += TOK) {
            const int n_tok = min(TOK, p.next_n - t0);
            const int64_t row0 = row_b + t0;
            int ctx[TOK];
#pragma unroll
            for (int t = 0; t < TOK; ++t)
                ctx[t] = t < n_tok ? min(p.context_lens[row0 + (t < n_tok ? t : 0)], p.max_context_len) : 0;
            QG qg;
            qg.load(p, p.q + row0 * H * D, row0, n_tok, lane);
            int j0 = c_begin + wave * 16;
            if (j0 >= c_end)
                continue;
            auto tile_ptr = [&](int j) {
                const int64_t blk = table[j >> bkv_shift];
                return p.kv + blk * p.kv_block_stride;
            };
            const uint8_t* base = tile_ptr(j0);
            int kvf[D / 16];
            const int rin = (j0 & (p.block_kv - 1)) + r16;
            load_frag<D>(base + rin * D + g * (D / 4), kvf);
            float sf = reinterpret_cast<const float*>(base + p.block_kv * D)[rin];
            for (; j0 < c_end; j0 += 16 * kPagedWaves) {
                const int jn = min(j0 + 16 * kPagedWaves, c_end - 1);       // clamped: never a table entry past the context
                const uint8_t* nbase = tile_ptr(jn);
                const int nrin = (jn & (p.block_kv - 16)) + r16;
                int nf[D / 16];
                load_frag<D>(nbase + nrin * D + g * (D / 4), nf);
                const float nsf = reinterpret_cast<const float*>(nbase + p.block_kv * D)[nrin];
                const int col = j0 + r16;
                qg.score(kvf, sf, lane, [&](int t, float v) {
                    int c = 0;
#pragma unroll
                    for (int u = 0; u < TOK; ++u)
                        if (u == t) c = ctx[u];
                    if (col < c)
                        store_logit(p, (row0 + t) * p.logits_stride + col, v);
                });
#pragma unroll
                for (int k = 0; k < D / 16; ++k)
                    kvf[k] = nf[k];
                sf = nsf;
            }
        }
    }
}

}  // namespace mqa
}  // namespace dg
