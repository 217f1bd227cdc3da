// CDNA4 (gfx950) device code of the BF16 GEMM path: D = round(C + A B^T), A [M, K] and B [N, K] BF16, K-major.
//
// A BF16 K block of 64 values is 128 bytes, the size of an FP8 K block of 128 values, so the LDS image, the LDS-DMA staging and the
// fragment reads of fp8_gemm_kernels.hpp carry over byte for byte: tile rows of 128 bytes with the 16-byte chunk index XOR-ed by
// (row & 7), pieces of 8 rows x 128 bytes issued by global_load_lds_dwordx4 with the swizzle on the per-lane source address, and a
// fragment of 32 bytes per lane ({chunk g, chunk g + 4} of row lane & 15, g = lane >> 4) read by two ds_read_b128.  What changes is
// the matrix instruction: a fragment pair feeds two v_mfma_f32_16x16x32_bf16 -- chunk g (K values 8g .. 8g + 7 of the block) to the
// first, chunk g + 4 (32 + 8g ..) to the second -- the same K permutation on both operands, so each pair sums the whole 64-value block.
// BF16 products are exact in FP32: the MFMAs accumulate in place, there is no per-block promotion.
//
// Conventions of the BF16 launches (GemmParams is shared with the FP8 kernels; its scale fields are unused here):
//   * a_sg / a_sm and b_sg / b_sn are BYTE strides (multiples of 16), k is in elements (a multiple of 8);
//   * D strides are in elements, as for the FP8 kernels (store_tile);
//   * the K tail (k % 64 != 0) is zero-filled by the loader: a lane whose 16-byte chunk starts at or past k issues its piece out of
//     range, and an out-of-range lane of an LDS-DMA piece writes zeros -- on both operands, so no garbage product reaches an accumulator.
#pragma once
#include "fp8_gemm_kernels.hpp"

namespace dg {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

// Both K halves of a 64-value block: acc += B(rows of the MFMA's A slot) x A(rows of its B slot), as in mfma_fp8_k128.
__device__ __forceinline__ void mfma_bf16_k64(v4f& acc, const v8i& rows_operand, const v8i& cols_operand) {
    const v4i r_lo = __builtin_shufflevector(rows_operand, rows_operand, 0, 1, 2, 3);
    const v4i r_hi = __builtin_shufflevector(rows_operand, rows_operand, 4, 5, 6, 7);
    const v4i c_lo = __builtin_shufflevector(cols_operand, cols_operand, 0, 1, 2, 3);
    const v4i c_hi = __builtin_shufflevector(cols_operand, cols_operand, 4, 5, 6, 7);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, r_lo), __builtin_bit_cast(v8bf, c_lo), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, r_hi), __builtin_bit_cast(v8bf, c_hi), acc, 0, 0, 0);
}

// BF16 output with accumulation, rounded ONCE: D = bf16(acc + float(D)) (the FP8 epilogue rounds the product first, the reference's FP8
// semantics; the BF16 GEMM's statement is one rounding of the FP32 sum).  Rows of the permuted column order of store_tile: a lane holds
// the 8 consecutive columns n_lane + h * 32 .. + 7 of pair h of N-subtiles.
template <int MS, int NS>
__device__ __forceinline__ void store_tile_bf16_acc(const GemmParams& p, const Tile& t, int64_t d_group_off, v4f (&acc)[MS][NS],
                                                    int m_base, int n_base) {
    static_assert(NS % 2 == 0, "pairs of N-subtiles");
    const int lane = threadIdx.x & 63, lg = lane >> 4;
    const int n_lane = n_base + lg * 8;
    const bool full_n = n_lane + (NS / 2 - 1) * 32 + 8 <= p.n && p.d_vec_ok;
    #pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
        const int row = m_base + (lane & 15) * MS + ms;           // (interleaved A rows, as in the FP8 stream tile)
        if (row < t.m_begin || row >= t.m_end)
            continue;
        uint16_t* drow = reinterpret_cast<uint16_t*>(p.d) + d_group_off + static_cast<int64_t>(row) * p.d_sm;
        #pragma unroll
        for (int h = 0; h < NS / 2; ++h) {
            if (full_n) {
                uint4* dst = reinterpret_cast<uint4*>(drow + n_lane + h * 32);
                const uint4 old = *dst;
                const uint32_t o[4] = {old.x, old.y, old.z, old.w};
                uint32_t w[4];
                #pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const v4f v = acc[ms][2 * h + j];
                    w[2 * j] = pack_bf16(v[0] + bf16_lo(o[2 * j]), v[1] + bf16_hi(o[2 * j]));
                    w[2 * j + 1] = pack_bf16(v[2] + bf16_lo(o[2 * j + 1]), v[3] + bf16_hi(o[2 * j + 1]));
                }
                *dst = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                #pragma unroll
                for (int j = 0; j < 2; ++j)
                    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int col = n_lane + h * 32 + j * 4 + r;
                        if (col < p.n) {
                            const float v = acc[ms][2 * h + j][r] + bf16_lo(static_cast<uint32_t>(drow[col]));
                            drow[col] = static_cast<uint16_t>(pack_bf16(v, 0.f) & 0xffffu);
                        }
                    }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The BF16 tile kernel: the FP8 stream tile's data movement (stream_kernel_body) without scales, on any tile of whole 8-row pieces.
// A STAGES-deep LDS ring of K blocks (A tile, then B tile, 128 bytes per row); every wave issues its pieces of a block, waits with a
// counted vmcnt for its pieces of the block it is about to read (the younger STAGES - 2 blocks stay in flight), and one barrier per K
// block both publishes the block and frees the slot of the block before it, which the next block's pieces refill.
//   256 x 256, 2 x 4 waves, 2 stages (128 KiB): the large tile -- wave tile 128 x 64, 64 MFMAs of 16 x 16 x 32 per wave and K block;
//   128 x 256, 2 x 4 waves, 3 stages (144 KiB): the psum layout's tile (a tile may not straddle two groups: BM divides the alignment);
//   64 x 32, 4 x 1 waves, 8 stages (96 KiB): the weight-streaming small-M tile (dense m <= 64, masked expected_m <= 64).
// A rows are interleaved (LDS row position ms * 16 + i holds tile row i * MS + ms) and B rows permuted (b_row_perm) as in the FP8 stream
// tile, so the FP8 epilogue (store_tile<MS, NS, true>) stores the accumulators as they are.
// KSPLIT (the small-M tile of a dense problem that fills too few CUs): work item w = (tile w % tiles, K piece w / tiles); piece q computes
// K blocks [q kb / f, (q + 1) kb / f) and stores its FP32 partial tile to D + q * d_sg -- the host points D at the caller's workspace
// ([f][m][n] FP32) -- and dg_bf16_split_k_sum_kernel, the second launch on the stream, sums the pieces in order into the real D.
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, int STAGES, bool KSPLIT = false>
__device__ __forceinline__ void bf16_kernel_body(const GemmParams& p) {
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MS = WM / 16, NS = WN / 16;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int LDS_BYTES = STAGES * STAGE_BYTES;
    constexpr int A_ITERS = BM / 8 / NW, B_ITERS = BN / 8 / NW, PIECES = A_ITERS + B_ITERS;
    constexpr unsigned OOB = 0x80000000u;
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "every wave issues the same number of pieces");
    static_assert(NS % 2 == 0 && MS >= 1, "pairs of N-subtiles (permuted B rows)");
    static_assert((NW * 8) % 16 == 0 && ((NW * 8) % WN == 0 || WN % (NW * 8) == 0), "the row permutation of a B piece must be lane-independent");
    static_assert((STAGES - 2) * PIECES < 64 && STAGES >= 2, "vmcnt is a 6-bit counter");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

    __shared__ __attribute__((aligned(1024))) uint8_t lds[LDS_BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int num_kb_total = (p.k + 63) / 64;
    const int piece_row = lane >> 3;
    const int src_chunk = (lane & 7) ^ piece_row;
    const int chunk_k = src_chunk * 8;                              // first K value of the lane's chunk within a block
    const int frag_off = (lane & 15) * 128 + ((((lane >> 4) ^ (lane & 7))) << 4);
    const int lda = static_cast<int>(p.a_sm), ldb = static_cast<int>(p.b_sn);
    auto a_unit_row = [](int u) { return (u / (WM / 8)) * WM + (u & 1) * 8 * MS + ((u % (WM / 8)) >> 1); };
    const int a_voff = piece_row * MS * lda + src_chunk * 16;
    const int b_voff = b_row_perm<WN>(wave * 8 + piece_row) * ldb + src_chunk * 16;

    MaskedWalk walk;
    const int num_launched = gridDim.x;
    int tile_id = blockIdx.x, pass = 0;
    while (true) {
        int tile = tile_id, kb0 = 0, num_kb = num_kb_total;
        [[maybe_unused]] int ks_piece = 0;
        if constexpr (KSPLIT) {
            const int tiles = p.num_m_tiles * p.num_n_tiles;
            if (tile_id >= tiles * p.sk_factor)
                break;
            tile = tile_id % tiles;
            ks_piece = tile_id / tiles;
            kb0 = ks_piece * num_kb_total / p.sk_factor;
            num_kb = (ks_piece + 1) * num_kb_total / p.sk_factor - kb0;
        }
        const Tile t = get_tile<BM, BN>(p, tile, walk, pass);
        if (!t.valid)
            break;
        const int64_t ad_group = (p.gemm_type == kMasked) ? t.group : 0;

        v4f acc[MS][NS];
        #pragma unroll
        for (int ms = 0; ms < MS; ++ms)
            #pragma unroll
            for (int ns = 0; ns < NS; ++ns)
                acc[ms][ns] = v4f{0.f, 0.f, 0.f, 0.f};

        if (t.m_end > t.m0 && num_kb > 0) {
            const uint8_t* a_base = uniform_pointer(p.a + ad_group * p.a_sg + static_cast<int64_t>(t.m0) * p.a_sm);
            const uint8_t* b_base = uniform_pointer(p.b + static_cast<int64_t>(t.group) * p.b_sg + static_cast<int64_t>(t.n0) * p.b_sn);
            const int a_rows = uniform_int(imin(t.m_end - t.m0, BM)), b_rows = uniform_int(imin(p.n - t.n0, BN));
            const auto a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a_base), 0, (a_rows - 1) * lda + p.k * 2, 0x00020000);
            const auto b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(b_base), 0, (b_rows - 1) * ldb + p.k * 2, 0x00020000);

            // all of this wave's pieces of K block j (of the work item) into the ring slot at slot_off; blocks past the end are issued out
            // of range (no-ops that write zeros) so that the vmcnt arithmetic stays exact
            auto issue_block = [&](int slot_off, int j) {
                const int kb = kb0 + j;
                const unsigned oob = (j < num_kb && kb * 64 + chunk_k < p.k) ? 0u : OOB;
                uint8_t* stage = lds + slot_off;
                #pragma unroll
                for (int q = 0; q < A_ITERS; ++q) {
                    const int unit = wave + NW * q;
                    const int voff = static_cast<int>((static_cast<unsigned>(a_voff) + static_cast<unsigned>(a_unit_row(unit) * lda)) | oob);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        a_rsrc, (__attribute__((address_space(3))) void*)(stage + unit * 1024), 16, voff, kb * 128, 0, 0);
                }
                #pragma unroll
                for (int q = 0; q < B_ITERS; ++q) {
                    const int unit = wave + NW * q;
                    const int voff = static_cast<int>((static_cast<unsigned>(b_voff) + static_cast<unsigned>(b_row_perm<WN>(q * (NW * 8)) * ldb)) | oob);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        b_rsrc, (__attribute__((address_space(3))) void*)(stage + A_BYTES + unit * 1024), 16, voff, kb * 128, 0, 0);
                }
            };
            #pragma unroll
            for (int j = 0; j < STAGES - 1; ++j)
                issue_block(j * STAGE_BYTES, j);

            int cur = 0, fill = (STAGES - 1) * STAGE_BYTES;
            for (int j = 0; j < num_kb; ++j) {
                // block j: my pieces have landed (the STAGES - 2 younger blocks may still fly); after the barrier everybody's have, and
                // everybody is done reading block j - 1, whose slot takes block j + STAGES - 1
                asm volatile("s_waitcnt vmcnt(%c0)" :: "i"((STAGES - 2) * PIECES) : "memory");
                raw_barrier();
                issue_block(fill, j + STAGES - 1);
                const uint8_t* a_tile = lds + cur + (wm * WM) * 128;
                const uint8_t* b_tile = lds + cur + A_BYTES + (wn * WN) * 128;
                v8i bf[NS];
                #pragma unroll
                for (int ns = 0; ns < NS; ++ns)
                    bf[ns] = load_fragment(b_tile + ns * 2048, frag_off);
                #pragma unroll
                for (int ms = 0; ms < MS; ++ms) {
                    const v8i af = load_fragment(a_tile + ms * 2048, frag_off);
                    #pragma unroll
                    for (int ns = 0; ns < NS; ++ns)
                        mfma_bf16_k64(acc[ms][ns], bf[ns], af);
                }
                fill = cur;
                cur = (cur == (STAGES - 1) * STAGE_BYTES) ? 0 : cur + STAGE_BYTES;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const int m_base = t.m0 + wm * WM, n_base = t.n0 + wn * WN;
        if (KSPLIT)
            store_tile<MS, NS, true>(p, t, ks_piece * p.d_sg, acc, m_base, n_base);          // FP32 partial, no accumulation (host)
        else if (p.d_dtype == 0 && p.accumulate)
            store_tile_bf16_acc<MS, NS>(p, t, ad_group * p.d_sg, acc, m_base, n_base);
        else
            store_tile<MS, NS, true>(p, t, ad_group * p.d_sg, acc, m_base, n_base);
        if (t.second_pass) {
            pass = 1;                   // contiguous layout, BM = 2 x alignment: the tile's other half belongs to another group
        } else {
            pass = 0;
            tile_id += num_launched;
        }
    }
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int STAGES, bool KSPLIT = false>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64)
void dg_bf16_gemm_kernel(const GemmParams p) {
    bf16_kernel_body<BM, BN, WAVES_M, WAVES_N, STAGES, KSPLIT>(p);
}

#ifndef DG_SHARD_TU   // (plain kernels: defined once, in the dg_api.hip translation unit -- see kernel_instances.inc)
// Second launch of the K split: D[r][c] = round(sum over pieces q in order of ws[q][r][c] (+ float(D[r][c]) if accumulating)), four
// columns per thread where n allows it.
__global__ __launch_bounds__(256)
void dg_bf16_split_k_sum_kernel(const float* __restrict__ ws, int pieces, int m, int n, void* d, int64_t d_sm, int d_dtype, int accumulate) {
    const int64_t slab = static_cast<int64_t>(m) * n;
    const int vec = (n % 4 == 0) ? 4 : 1;
    const int64_t items = slab / vec;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < items; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e = i * vec;
        const int r = static_cast<int>(e / n), c = static_cast<int>(e - static_cast<int64_t>(r) * n);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < pieces; ++q)
            for (int v = 0; v < vec; ++v)
                s[v] = q == 0 ? ws[e + v] : s[v] + ws[q * slab + e + v];
        const int64_t off = static_cast<int64_t>(r) * d_sm + c;
        for (int v = 0; v < vec; ++v) {
            if (d_dtype == 0) {
                uint16_t* d16 = static_cast<uint16_t*>(d) + off + v;
                const float x = accumulate ? s[v] + bf16_lo(static_cast<uint32_t>(*d16)) : s[v];
                *d16 = static_cast<uint16_t>(pack_bf16(x, 0.f) & 0xffffu);
            } else {
                float* d32 = static_cast<float*>(d) + off + v;
                *d32 = accumulate ? s[v] + *d32 : s[v];
            }
        }
    }
}

// Re-majoring of an MN-major BF16 operand: dst[b][c][r] = src[b][r][c] (2-byte elements, leading dimensions in elements), one 64 x 64
// tile per workgroup through LDS (one padding column: the column reads of the second phase hit 64 different banks).
__global__ __launch_bounds__(256)
void dg_transpose_bf16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int rows, int cols, int64_t src_ld,
                              int64_t dst_ld, int64_t src_batch_stride, int64_t dst_batch_stride) {
    __shared__ uint16_t tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    src += blockIdx.z * src_batch_stride;
    dst += blockIdx.z * dst_batch_stride;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        if (r0 + r < rows && c0 + c < cols)
            tile[r][c] = src[static_cast<int64_t>(r0 + r) * src_ld + c0 + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (r0 + r < rows && c0 + c < cols)
            dst[static_cast<int64_t>(c0 + c) * dst_ld + r0 + r] = tile[r][c];
    }
}
#endif

}  // namespace dg
