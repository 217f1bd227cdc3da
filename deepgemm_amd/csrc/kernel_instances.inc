// Every template kernel instantiation of the library, by build shard.
//
// The library is built from one small translation unit (dg_api.hip: host code + the plain kernels) and DG_NUM_SHARDS instantiation
// units (dg_shard.hip compiled with -DDG_SHARD=<n>), in parallel -- one hipcc device pass over all ~60 instantiations took six minutes.
// dg_api.hip includes this file with DG_KERNEL_INSTANCE(...) = `extern template __global__ ...;` (it takes the kernels' addresses, it does
// not compile them); shard n includes it with DG_SHARD == n and DG_KERNEL_INSTANCE(...) = `template __global__ ...;`.
// A kernel that dg_api.hip names but this list lacks is instantiated implicitly in dg_api.hip: correct, only slower to build.
// (Inside namespace dg.)
#define DG_P const GemmParams
#if !defined(DG_SHARD) || DG_SHARD == 0        // duo, 256-row tiles, K-major operands
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, false, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_tab_fused_kernel<256, 128, 256, 2, 4>(DG_P, DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 1        // duo, 256-row tiles, MN-major operands
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true, false, false, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 2        // duo, 128-row tiles (two-segment schedule), K split
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, false, false, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, false, false, false, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, true, false, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, true, false, false, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, true, false, true, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_kernel<128, 256, 2, 4, true, true, true, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_split_k_reduce_kernel<128, 256, 2, 4, false>(DG_P))
DG_KERNEL_INSTANCE(void dg_split_k_reduce_kernel<128, 256, 2, 4, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 3        // two-stage pipe kernels; recipe (1, 1, 128)
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<256, 256, 2, 4, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<128, 256, 2, 4, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<128, 128, 2, 2, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<64, 256, 1, 4, 1>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<32, 256, 1, 4, 0>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_kernel<16, 256, 1, 4, 0>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, false>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_pipe_pc_kernel<192, 256, 2, 4, 1, false>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 4        // hardware-scaled (packed UE8M0) quad kernels
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 5        // ... the register-resident forms, the 8-wave hardware-scaled kernels
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 1>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true, false, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 6        // stream tiles, fused expert-MLP L1
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, false, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, false, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 64, 4, 1, 4, 0, 2, false, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, false, 4>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 2, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 4>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true, 0, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 0, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 4, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 0, 1, true, 0, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2, 1, true, 0, false, true>(DG_P))
#ifdef DG_HAVE_MOE_HPP
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_swiglu_kernel<3>(DG_P, const SwigluOut))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_stream_swiglu_kernel<6>(DG_P, const SwigluOut))
#endif
#endif
#if !defined(DG_SHARD) || DG_SHARD == 7        // skinny (decode) kernels
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<2, 4, 1, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 2, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true, true, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 8        // K-grouped hardware-scaled quad kernels (packed UE8M0, granularity 128 / 32)
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, false, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, true, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 9        // ... with the MN-major operands read in place (transposing fragment reads)
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, false, true, true>(DG_P))
DG_KERNEL_INSTANCE(void dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true, true, true>(DG_P))
#endif
#if !defined(DG_SHARD) || DG_SHARD == 10       // BF16 tiles (bf16_gemm_kernels.hpp)
DG_KERNEL_INSTANCE(void dg_bf16_gemm_kernel<256, 256, 2, 4, 2>(DG_P))
DG_KERNEL_INSTANCE(void dg_bf16_gemm_kernel<128, 256, 2, 4, 3>(DG_P))
DG_KERNEL_INSTANCE(void dg_bf16_gemm_kernel<64, 32, 4, 1, 8>(DG_P))
DG_KERNEL_INSTANCE(void dg_bf16_gemm_kernel<64, 32, 4, 1, 8, true>(DG_P))
#endif
#undef DG_P
