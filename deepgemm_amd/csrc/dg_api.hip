// Host side of the C ABI declared in include/deepgemm_amd.h: argument checks, tile-configuration heuristics
// (the analogue of get_best_config, reference csrc/jit_kernels/heuristics/common.hpp:14-52, re-derived for 256 CUs /
// 160 KiB LDS / wave64) and kernel launches.  Kernels are compiled ahead of time for gfx950; there is no JIT.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/deepgemm_amd.h"
#include "fp8_gemm_kernels.hpp"
#include "fp8_gemm_quad.hpp"
#include "fp8_gemm_moe.hpp"
#include "bf16_gemm_kernels.hpp"
#include "mqa_logits_kernels.hpp"
#include "hc_prenorm_kernels.hpp"
#ifndef DG_MONOLITHIC   // (the default build: the template kernels are compiled by the dg_shard.hip units, see kernel_instances.inc)
namespace dg {
#define DG_HAVE_MOE_HPP 1
#define DG_KERNEL_INSTANCE(...) extern template __global__ __VA_ARGS__;
#include "kernel_instances.inc"
#undef DG_KERNEL_INSTANCE
}  // namespace dg
#endif
#ifdef DG_EXPERIMENTS   // the lab notebook lives outside the product sources: tools/experiments/ (build.py adds the include path)
#include "fp8_gemm_experiments.hpp"
#endif

namespace {

// Error text and the name of the last selected configuration are per calling thread (errno style); the tuning knobs are
// process-wide like the reference's runtime singletons (csrc/apis/runtime.hpp:12-49) and safe to set from any thread.
thread_local std::string g_last_error;
thread_local std::string g_last_config = "";
std::atomic<unsigned> g_stream_ks_epoch{0};         // exchange epochs of the stream_ks launches (FP32-scale and packed forms share the workspace's flags)
thread_local size_t g_workspace_bytes = 0;          // size of the workspace behind GemmParams::sk_workspace for the call in flight
std::atomic<int> g_num_cus_override{0};
std::atomic<long long*> g_debug_buffer{nullptr};
std::mutex g_forced_config_mutex;
std::string g_forced_config = "auto";              // guarded by g_forced_config_mutex

std::string forced_name() {
    std::lock_guard<std::mutex> lock(g_forced_config_mutex);
    return g_forced_config;
}

// One forced name for both families (set_forced_config): a BF16 name (prefix bf16_) forces the BF16 entries only -- the FP8 selection
// sees "auto" -- and an FP8 name the FP8 entries only.
bool is_bf16_config_name(const std::string& name) { return name.compare(0, 5, "bf16_") == 0; }
std::string forced_config() {
    std::string name = forced_name();
    return is_bf16_config_name(name) ? std::string("auto") : name;
}
std::string forced_bf16_config() {
    std::string name = forced_name();
    return is_bf16_config_name(name) ? name : std::string("auto");
}

int fail(const char* file, int line, const char* what) {
    g_last_error = std::string("Assertion error (") + file + ":" + std::to_string(line) + "): " + what;
    return 1;
}

#define DG_CHECK(cond)                                 \
    do {                                               \
        if (!(cond))                                   \
            return fail(__FILE__, __LINE__, #cond);    \
    } while (0)

#define DG_HIP_CHECK(expr)                                                                  \
    do {                                                                                    \
        const hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                             \
            g_last_error = std::string("HIP error (" __FILE__ ":") + std::to_string(__LINE__) + \
                           "): " + hipGetErrorString(e_);                                   \
            return 2;                                                                       \
        }                                                                                   \
    } while (0)

// CU count of the CURRENT device, cached per device ordinal (mixed-device nodes, threads bound to different devices).
int device_cu_count() {
    constexpr int kMaxDevices = 64;
    static std::atomic<int> cached[kMaxDevices];    // zero-initialised: 0 = not queried yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return 256;                                 // MI355X; only reached when no device is visible (host-only unit tests)
    if (dev >= 0 && dev < kMaxDevices) {
        const int known = cached[dev].load(std::memory_order_relaxed);
        if (known > 0)
            return known;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 256;
    if (dev >= 0 && dev < kMaxDevices)
        cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

int num_cus() {
    const int forced = g_num_cus_override.load(std::memory_order_relaxed);
    return forced > 0 ? forced : device_cu_count();
}

using KernelFn = void (*)(const dg::GemmParams);

struct Config {
    const char* name;
    int bm, bn, threads;
    int blocks_per_cu;      // residency by LDS (2 stages x (bm + bn) x 128 B of 160 KiB) and registers
    float efficiency;       // relative MFMA efficiency of the tile shape (heuristic weight, refined by measurement)
    bool fast;
    KernelFn fn;
    bool ring = false;      // ring kernels read SFA through a buffer descriptor that assumes the MN-major layout
    bool two_pass = false;  // contiguous layout: BM may be twice the M alignment (halves of two groups => two passes)
    bool persistent = false;  // one workgroup per CU walks the tile list and prefetches the next tile's first K blocks
    bool per_col = false;     // recipe (1, 1, 128): one SFB value per row of B (all other fast kernels: one per 128 rows)
    bool split_k = false;     // persistent launch whose partial last round is cut along K over the idle CUs (needs a workspace)
    bool k_tail = false;      // handles a partial last K block (k % 128 != 0, k % 16 == 0, k > 128): the duo kernels
    bool sfa_rm = false;      // reads a ROW-major SFA ([M][K / 128], sfa_stride_k == 1) in place -- every other ring kernel wants it MN-major
};

const Config kConfigs[] = {
    {"duo_256x256", 256, 256, 512, 1, 1.10f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4>, true, true},
    {"duo_p_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true>, true, true, true},
    // 128-row duo tile: grouped-contiguous layouts (BM must divide the 128-row alignment) and tile counts that quantise
    // badly at 256 x 256.  Measured per-tile: 116 k cycles vs 167 k for twice the work (L2->LDS bytes per flop are 1.5x).
    // Every 128-row form runs the two-segment schedule (MERGED: one load + one 16-step matrix segment per K block, 3-slot B
    // ring): 1.47-1.50 k cycles per K block against 1.60-1.63 k for the four-segment schedule of the 256-row tile, same bits.
    {"duo_128x256", 128, 256, 512, 1, 0.78f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, false, false, false, false, true>, true},
    // the same tile in a persistent launch whose partial last round is split along K (2.25 rounds of tiles cost 2 + ~0.4 instead
    // of 3): picked instead of duo_128x256 when the caller provides the workspace and the tail is at most half a round
    {"duo_sk_128x256", 128, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, true, false, true, false, false, true>, true, false, true,
     false, true},
    {"duo_sk_bmn_128x256", 128, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, true, true, true, false, false, true>, true,
     false, true, false, true},
    // operand B MN-major ([K][N]; the nn / tn layouts): the same kernels with LDS-DMA row pieces + transpose reads for B
    {"duo_bmn_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true>, true, true, true},
    {"duo_bmn_128x256", 128, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, true, false, false, false, true>, true},
    // operand A MN-major ([K][M]; the tt / tn layouts of the dense GEMM): A through row pieces + transpose reads, B K-major / MN-major
    {"duo_amn_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, false, false, true>, true, false, true},
    {"duo_abmn_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true, false, true>, true, false, true},
    // K not a multiple of 128 (whole 16-byte chunks; the dgrad shapes K = 2112, 576): the same kernels with the partial last K
    // block computed after the loop (dense problems; K-major A; B K-major or MN-major)
    {"duo_kt_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, false, false, false, true>, true, false,
     true, false, false, true},
    {"duo_kt_128x256", 128, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, false, false, false, true, true>, true, false,
     false, false, false, true},
    {"duo_bmn_kt_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true, true, false, false, true>, true, false,
     true, false, false, true},
    {"duo_bmn_kt_128x256", 128, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, false, true, false, false, true, true>, true, false,
     false, false, false, true},
    {"pipe_256x256", 256, 256, 512, 1, 1.00f, true, dg::dg_fp8_gemm_pipe_kernel<256, 256, 2, 4, 2>},
    {"pipe_128x256", 128, 256, 512, 1, 0.66f, true, dg::dg_fp8_gemm_pipe_kernel<128, 256, 2, 4, 2>},
    {"pipe_128x128", 128, 128, 256, 2, 0.80f, true, dg::dg_fp8_gemm_pipe_kernel<128, 128, 2, 2, 2>},
    {"pipe_64x256", 64, 256, 256, 2, 0.60f, true, dg::dg_fp8_gemm_pipe_kernel<64, 256, 1, 4, 1>},
    {"pipe_32x256", 32, 256, 256, 2, 0.35f, true, dg::dg_fp8_gemm_pipe_kernel<32, 256, 1, 4, 0>},
    {"pipe_16x256", 16, 256, 256, 2, 0.20f, true, dg::dg_fp8_gemm_pipe_kernel<16, 256, 1, 4, 0>},
    {"stream_64x128", 64, 128, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6>, true},
    // the same with the non-temporal policy on the weight stream's LDS-DMA: +3-5 % when the weights of one launch exceed the 256 MiB
    // Infinity Cache anyway (32 experts x 6144 x 7168: 254 -> 245 us), neutral to -8 % below that (they would have stayed resident)
    {"stream_nt_64x128", 64, 128, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 2>, true},
    // round 5: a 3-stage ring (77 KiB of LDS) so that TWO workgroups share a CU: 257 .. 512 tiles of 64 x 128 are then ONE resident round
    // instead of a full round and a mostly idle one (the masked GEMM2 of the expert MLP: 8 experts x 7168 x 2048 = 448 tiles)
    // round 6: the 6-stage 64 x 128 stream tile with every tile cut along K into sk_factor pieces, one work item per (tile, piece), partials
    // exchanged inside the kernel (stream_kernel_body, KSPLIT): dense mid-M problems whose tiles fill a quarter of the chip or less
    // (m = 128, 4096 x 7168: 64 tiles x 4 pieces, 344 KB per CU instead of 688 KB on 64 x 32 tiles); needs the caller's workspace
    {"stream_ks_64x128", 64, 128, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, false, 0, true>, true, false, false,
     false, true},
    // ... and the 64 x 32 tile (four K blocks per stage) likewise: narrow layers at small M, whose 64 x 32 tiles fill a quarter of the chip or less
    // (m = 128, n = 576 -- the MLA down-projection of the reference's sweep: 36 tiles, one K loop of 56 blocks on 36 CUs)
    {"stream_ks_64x32", 64, 32, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, false, 0, true>, true, false, false,
     false, true},
    // ... and a 64 x 64 tile (two K blocks per stage, four stages): m = 128, 4096 x 7168 as 128 tiles x 2 pieces, 459 KB per CU and ONE partner per tile
    {"stream_ks_64x64", 64, 64, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 64, 4, 1, 4, 0, 2, false, 0, true>, true, false, false,
     false, true},
    {"stream2_64x128", 64, 128, 256, 2, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3>, true},
    {"stream_nt2_64x128", 64, 128, 256, 2, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2>, true},
    // (64 x 32: four K blocks per ring stage -- a quarter of the barriers: 4-7 % on the small-M shapes; no gain on the 64 x 128 tile)
    {"stream_64x32", 64, 32, 256, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4>, true},
    // round 4: the same tiles with loader waves (4 compute waves + 4 / 12 that only issue LDS-DMA pieces): a stream tile is bound by the
    // LDS-DMA issue rate of its workgroup, and that rate grows with the number of issuing waves (50 / 80 / 96 GB/s per CU at 4 / 8 / 16)
    {"stream_l8_64x32", 64, 32, 512, 1, 0.0f, true, dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, false, 4>, true},
    // M <= 16 / 32 (decode batches): 16 output columns per workgroup over the whole K, the 8 waves split K; weights straight into registers
    {"skinny_16", 16, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<1>},
    {"skinny_32", 32, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<2>},
    // two N-subtiles per workgroup, 17 .. 32 columns (GemmParams::skinny_cols): one round where n / 16 is between one and two rounds
    {"skinny_16w", 16, 32, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<1, 4, 2>},
    // round 5: the same three with coalesced weight loads (8 rows x 128 bytes per instruction) turned into MFMA operands through wave-private LDS
    {"skinny_16c", 16, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<1, 4, 1, true>},
    {"skinny_32c", 32, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<2, 4, 1, true>},
    {"skinny_16wc", 16, 32, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<1, 4, 2, true>},
    // ... and coalesced activation loads as well (m > 1: A is up to as many bytes per workgroup as the weights)
    {"skinny_16ca", 16, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true>},
    // (the 32-row form with coalesced activation loads and four K blocks per chunk spills inside its K loop -- 24 VGPRs -- and loses at
    //  32 x 4096 x 7168: 15.7 against 13.6 us; with three K blocks per chunk it fits)
    {"skinny_32ca", 32, 16, 512, 1, 0.0f, true, dg::dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true>},
    {"pipe_pc_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, false>, true, false,
     false, true},
    {"pipe_pc_mn_256x256", 256, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, true>, true,
     false, false, true},
    // round 5: 192-row tiles (wave tile 96 x 64, 24 steps per K block) where they cover M with fewer rows than 256-row tiles do -- the
    // recipe is VALU-issue bound, so a row that is not computed is time saved (576 rows: 3 x 192 against 3 x 256; per_col_bm)
    {"pipe_pc_192x256", 192, 256, 512, 1, 0.0f, true, dg::dg_fp8_gemm_pipe_pc_kernel<192, 256, 2, 4, 1, false>, true, false,
     false, true},
    {"generic_128x128", 128, 128, 256, 4, 0.15f, false, dg::dg_fp8_gemm_generic_kernel},
#ifdef DG_EXPERIMENTS   // (tools/experiments/, on the include path of DG_EXPERIMENTS builds only)
#define DG_EXPERIMENT_ROWS_FP32
#include "experiment_configs.inc"
#undef DG_EXPERIMENT_ROWS_FP32
#endif
};
constexpr int kNumConfigs = sizeof(kConfigs) / sizeof(kConfigs[0]);

// Kernels of the packed-UE8M0 entry points (hardware-scaled MFMA); selected by launch_e8, forced by name for A/B runs.
struct E8Config { const char* name; KernelFn fn; int bm, bn, threads; bool whole_quads; bool grouped_ok; bool stream; int per_cu = 1; bool g32 = false; };
const E8Config kE8Configs[] = {
    {"e8_quad_256x256", dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0>, 256, 256, 256, true, true, false},
    {"e8_quad_128x256", dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0>, 128, 256, 256, false, true, false},
    {"e8_duo_256x256", dg::dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4>, 256, 256, 512, false, false, false},
    // decode-sized M (masked / dense, M <= 64 per group): the deep-ring stream tile with the quad's words riding in every stage
    {"e8_stream_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true>, 64, 128, 256, false, true, true},
    {"e8_stream_nt_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 2, 1, true>, 64, 128, 256, false, true, true},
    {"e8_stream_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true>, 64, 32, 256, false, true, true},
    // round 4: k % 128 != 0 (whole 16-byte chunks, k > 128; dense): the 128-row quad form with the partial last block zero-filled by the
    // buffer range check -- packed-scale dgrad shapes (K = 2112, 576) no longer leave the hardware-scaled path
    {"e8_quad_kt_128x256", dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, true>, 128, 256, 256, false, false, false},
    // round 4: operand B MN-major ([K][N]: the nn layout of a packed-scale dgrad) read in place by the 8-wave hardware-scaled kernel
    // (transpose reads, natural column order) -- instead of a re-majoring pass over B in front of the quad kernel
    // (round 5: also the contiguous layout -- grouped nn with packed scales, the weights [G][K][N] read in place; launch_e8 refuses the other grouped forms)
    {"e8_duo_bmn_256x256", dg::dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true>, 256, 256, 512, false, true, false},
    // ... and A MN-major ([K][M]: the tt layout), both (tn): scale words of A in natural row order
    {"e8_duo_amn_256x256", dg::dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, false, true>, 256, 256, 512, false, false, false},
    {"e8_duo_abmn_256x256", dg::dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true, true>, 256, 256, 512, false, false, false},
    // round 5: ... with a partial last K block (the nn layout of a packed-scale dgrad whose K is not a multiple of 128: 2112, 576)
    {"e8_duo_bmn_kt_256x256", dg::dg_fp8_gemm_duo_e8_kernel<256, 256, 2, 4, true, false, true>, 256, 256, 512, false, false, false},
    // round 5: the quad kernel with all sixteen fragments of a K block register-resident, two LDS buffers per operand, three barriers per
    // K block, fragment reads and LDS-DMA pieces in separate phases (fp8_gemm_quad.hpp, HS)
    {"e8_quad_h_256x256", dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 1>, 256, 256, 256, true, true, false},
    {"e8_quad_h2_256x256", dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 2>, 256, 256, 256, true, true, false},
    // round 5: the stream tile on a 3-stage ring (74 KiB of LDS), two workgroups per CU (stream2_64x128 above)
    {"e8_stream2_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 0, 1, true>, 64, 128, 256, false, true, true, 2},
    {"e8_stream_nt2_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2, 1, true>, 64, 128, 256, false, true, true, 2},
    // round 6: scale granularity 32 along K (the reference's SM100 MX recipe; one packed word per row and 128-K block, every lane group of the
    // scaled MFMA takes its own byte): the two four-wave forms, selected by the *_g32 entry points only (E8Config::g32)
    {"e8_quad_g32_256x256", dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true>, 256, 256, 256, false, true, false, 1, true},
    {"e8_quad_g32_128x256", dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, true>, 128, 256, 256, false, true, false, 1, true},
    // round 6: batch-1 .. 32 decode with packed scales: the skinny weight-stream kernel with the scaled MFMA (one workgroup per 16 columns)
    // ... the 64 x 32 stream tile with four loader waves beside its four compute waves (the packed words ride in the group ring: stream_kernel_body, GSE)
    {"e8_stream_l8_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 4>, 64, 32, 512, false, true, true},
    // ... and the stream tiles cut along K inside the kernel (stream_kernel_body, KSPLIT: pieces of whole K quads; the rules of stream_ks_64x128 / _64x32)
    {"e8_stream_ks_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true, 0, true>, 64, 128, 256, false, false, true},
    {"e8_stream_ks_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, true>, 64, 32, 256, false, false, true},
    {"e8_stream_ks_g32_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 6, 0, 1, true, 0, true, true>, 64, 128, 256, false, false, true, 1, true},
    {"e8_stream_ks_g32_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, true, true>, 64, 32, 256, false, false, true, 1, true},
    {"e8_skinny_16", dg::dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true, true>, 16, 16, 512, false, false, false},
    {"e8_skinny_32", dg::dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true, true>, 32, 16, 512, false, false, false},
    {"e8_skinny_g32_16", dg::dg_fp8_gemm_skinny_kernel<1, 4, 1, true, true, true, true>, 16, 16, 512, false, false, false, 1, true},
    {"e8_skinny_g32_32", dg::dg_fp8_gemm_skinny_kernel<2, 3, 1, true, true, true, true>, 32, 16, 512, false, false, false, 1, true},
    // ... and the decode-sized stream tiles (every stage carries its K block's words)
    {"e8_stream_g32_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 0, false, true>, 64, 32, 256, false, true, true, 1, true},
    {"e8_stream_l8_g32_64x32", dg::dg_fp8_gemm_stream_kernel<64, 32, 4, 1, 3, 0, 4, true, 4, false, true>, 64, 32, 512, false, true, true, 1, true},
    {"e8_stream2_g32_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 0, 1, true, 0, false, true>, 64, 128, 256, false, true, true, 2, true},
    {"e8_stream_nt2_g32_64x128", dg::dg_fp8_gemm_stream_kernel<64, 128, 1, 4, 3, 2, 1, true, 0, false, true>, 64, 128, 256, false, true, true, 2, true},
#ifdef DG_EXPERIMENTS
#define DG_EXPERIMENT_ROWS_E8
#include "experiment_configs.inc"
#undef DG_EXPERIMENT_ROWS_E8
#endif
};

// Tuning / diagnostic environment variables are read ONCE (first use): the launch paths are hot (a cached dense call is ~8 us of host time).
// A launch reads them through an immutable snapshot behind an atomic pointer; dg_reload_env publishes a fresh snapshot (the old one is
// leaked on purpose: a launch on another thread may still be reading it, and a reload is a tools / tests event, a few dozen bytes each).
// Variables set after the first launch are therefore ignored until dg_reload_env() is called (README, "Environment").
struct EnvKnobs {
    bool print_configs, table_kernel, tab_unfused, sk_exchange, sfa_rowmajor_in_place, swiglu_one_per_cu;
    int group_m, ks_pieces, pc_bm;
    bool e8_tab_unsplit;
    int ks_max_pieces;      // DG_STREAM_KS_PIECES: upper bound of the K pieces of the stream_ks tile (tuning; default 8)
    int swiglu_fault;       // DG_TEST_SWIGLU_FAULT (tests only): 1 = odd tiles of the fused SwiGLU kernel never publish their amax
    bool e8_split_quad_model_only;   // (tuning: e8_split_pieces prices the unsplit call as the 128-row kernel even up to 256 rows -- the rule before the end of round 6)
    EnvKnobs()
        : print_configs(getenv("DG_PRINT_CONFIGS") != nullptr), table_kernel(getenv("DG_TABLE_KERNEL") != nullptr),
          tab_unfused(getenv("DG_TAB_UNFUSED") != nullptr), sk_exchange(getenv("DG_SK_EXCHANGE") != nullptr),
          sfa_rowmajor_in_place(getenv("DG_SFA_ROWMAJOR_IN_PLACE") != nullptr), swiglu_one_per_cu(getenv("DG_SWIGLU_ONE_PER_CU") != nullptr),
          group_m(getenv("DG_GROUP_M") ? atoi(getenv("DG_GROUP_M")) : 0), ks_pieces(getenv("DG_KS_PIECES") ? atoi(getenv("DG_KS_PIECES")) : 0),
          pc_bm(getenv("DG_PC_BM") ? atoi(getenv("DG_PC_BM")) : 0), e8_tab_unsplit(getenv("DG_E8_TAB_UNSPLIT") != nullptr),
          ks_max_pieces(getenv("DG_STREAM_KS_PIECES") ? std::max(1, std::min(8, atoi(getenv("DG_STREAM_KS_PIECES")))) : 8),
          swiglu_fault(getenv("DG_TEST_SWIGLU_FAULT") ? atoi(getenv("DG_TEST_SWIGLU_FAULT")) : 0),
          e8_split_quad_model_only(getenv("DG_E8_SPLIT_QUAD_MODEL_ONLY") != nullptr) {}
};
std::atomic<const EnvKnobs*> g_env_knobs{nullptr};
const EnvKnobs& env_knobs() {
    const EnvKnobs* k = g_env_knobs.load(std::memory_order_acquire);
    if (k == nullptr) {
        const EnvKnobs* fresh = new EnvKnobs();
        if (g_env_knobs.compare_exchange_strong(k, fresh, std::memory_order_acq_rel))
            return *fresh;
        delete fresh;           // another thread published first
    }
    return *k;
}

// Weight bytes of one launch from which the stream tiles read them with the non-temporal policy.  Round 5 set 80 MB on rotations that fitted the
// Infinity Cache (59 MB: 14.3 us against 14.0); with cold weights -- what a model's layer sees -- the policy wins from the smallest sweep entries
// up (m = 1, 24576 x 1536 = 38 MB: 12.3 -> 10.8 us; 32768 x 512 = 17 MB: 6.8 -> 6.6; m = 128: 19.0 -> 18.5, 10.5 -> 10.0; 7168 x 2048 = 15 MB: equal)
// -- profiles/r06_probe/small_m_sweep_forced.log.
constexpr double kNonTemporalWeightBytes = 16e6;

bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

// whole_k_blocks = false: a partial last K block of whole 16-byte chunks is allowed (the duo kernels' tail stage)
bool k_extent_ok(int k, bool whole_k_blocks) { return whole_k_blocks ? k % 128 == 0 : (k % 16 == 0 && k > 128); }

bool fast_eligible(const dg::GemmParams& p, bool whole_k_blocks = true) {
    if (p.a_sk != 1 || p.b_sk != 1 || !k_extent_ok(p.k, whole_k_blocks))
        return false;
    if (!aligned16(p.a) || !aligned16(p.b) || p.a_sm % 16 || p.b_sn % 16 || p.a_sg % 16 || p.b_sg % 16)
        return false;
    // The LDS-DMA source offsets are 32-bit: one tile's rows must stay within 2 GiB of its base.
    if (p.a_sm > (1 << 22) || p.b_sn > (1 << 22))
        return false;
    return true;
}

// The stream kernels fetch the row scales of four K blocks with 16-byte requests: MN-major SFA whose K-block rows start on 16-byte
// boundaries (what get_mn_major_tma_aligned_tensor produces: rows padded to a multiple of four floats).
bool sfa_quads_ok(const dg::GemmParams& p) {
    return p.sfa_sm == 1 && aligned16(p.sfa) && p.sfa_sk % 4 == 0 && p.sfa_sg % 4 == 0;
}

// A K-major, B MN-major ([K][N], unit stride along n): the B_MN forms of the duo kernels.
bool bmn_eligible(const dg::GemmParams& p) {
    return p.sfb_gran_n == 128 && p.a_sk == 1 && p.b_sn == 1 && p.b_sk != 1 && (p.k % 128 == 0 || k_extent_ok(p.k, p.gemm_type != dg::kNormal)) &&
           p.sfa_sm == 1 && (p.gemm_type == dg::kNormal || p.gemm_type == dg::kContiguous || p.gemm_type == dg::kContiguousPsum) &&
           aligned16(p.a) && aligned16(p.b) && p.a_sm % 16 == 0 && p.b_sk % 16 == 0 && p.a_sg % 16 == 0 && p.b_sg % 16 == 0 &&
           p.n % 16 == 0 && p.a_sm <= (1 << 22) && p.b_sk <= (1 << 22) && static_cast<int64_t>(p.k) * p.b_sk < (1LL << 31);
}

// A MN-major ([K][M], unit stride along m), dense problems only; B either K-major (fast_eligible's B half) or MN-major (bmn_eligible's
// B half): the A_MN forms of the 256 x 256 duo kernel.
bool amn_eligible(const dg::GemmParams& p) {
    const bool a_ok = p.a_sm == 1 && p.a_sk != 1 && aligned16(p.a) && p.a_sk % 16 == 0 && p.a_sk <= (1 << 22) &&
                      static_cast<int64_t>(p.k) * p.a_sk < (1LL << 31);
    const bool b_k_major = p.b_sk == 1 && aligned16(p.b) && p.b_sn % 16 == 0 && p.b_sn <= (1 << 22);
    const bool b_mn_major = p.b_sn == 1 && p.b_sk != 1 && aligned16(p.b) && p.b_sk % 16 == 0 && p.n % 16 == 0 &&
                            p.b_sk <= (1 << 22) && static_cast<int64_t>(p.k) * p.b_sk < (1LL << 31);
    return p.sfb_gran_n == 128 && p.gemm_type == dg::kNormal && p.k % 128 == 0 && p.sfa_sm == 1 && a_ok &&
           (b_k_major || b_mn_major);
}

// Packed-UE8M0 dense problem with at least one MN-major operand that the 8-wave hardware-scaled kernel reads in place (e8_duo_bmn / _amn /
// _abmn_256x256: whole K blocks, scale words MN-major, 16-byte aligned rows / k-rows).
bool e8_mn_eligible(const dg::GemmParams& p) {
    const bool a_mn = p.a_sk != 1, b_mn = p.b_sk != 1;
    // round 5: also the contiguous layout (not psum) with MN-major weights [G][K][N] -- the grouped nn form; 256-row tiles, two passes over a
    // tile whose 128-row halves belong to two groups (alignment 128) or one (alignment a multiple of 256)
    const bool grouped_nn = p.gemm_type == dg::kContiguous && !a_mn && b_mn && p.k % 128 == 0 && p.b_sg % 16 == 0 &&
                            (p.m_alignment == 128 || p.m_alignment % 256 == 0);
    if (!(a_mn || b_mn) || (p.gemm_type != dg::kNormal && !grouped_nn) || p.sfa_sm != 1 || p.sfb_sn != 1 || p.head_lr != 0)
        return false;
    // K tail (whole 16-byte chunks, K > 128): the nn layout only -- A K-major, B [K][N] (round 5: e8_duo_bmn_kt_256x256, the packed-scale dgrad shapes)
    if (p.k % 128 != 0 && (a_mn || p.k % 16 != 0 || p.k <= 128))
        return false;
    const bool a_ok = a_mn ? (p.a_sm == 1 && aligned16(p.a) && p.a_sk % 16 == 0 && p.m % 16 == 0 && p.a_sk <= (1 << 22) &&
                              static_cast<int64_t>(p.k) * p.a_sk < (1LL << 31))
                           : (aligned16(p.a) && p.a_sm % 16 == 0 && p.a_sm <= (1 << 22));
    const bool b_ok = b_mn ? (p.b_sn == 1 && aligned16(p.b) && p.b_sk % 16 == 0 && p.n % 16 == 0 && p.b_sk <= (1 << 22) &&
                              static_cast<int64_t>(p.k) * p.b_sk < (1LL << 31))
                           : (aligned16(p.b) && p.b_sn % 16 == 0 && p.b_sn <= (1 << 22));
    return a_ok && b_ok;
}
const char* e8_mn_config_name(const dg::GemmParams& p) {
    if (p.k % 128 != 0)
        return "e8_duo_bmn_kt_256x256";
    return p.a_sk != 1 ? (p.b_sk != 1 ? "e8_duo_abmn_256x256" : "e8_duo_amn_256x256") : "e8_duo_bmn_256x256";
}
// ... and is better off there than re-majored in front of the quad kernel: tile-kernel territory (the stream tiles of small M want K-major
// weights), and the pass(es) over the MN-major operand(s) -- 3 us + twice their bytes at 4.5 TB/s each -- cost more than the 8-wave
// kernel's slower K loop (a quarter of the quad kernel's time at 3 PFLOP/s).  Measured (profiles/r04_probe/e8_mn_in_place_ab.log): nn
// 2048 x 7168 x 2048 35.1 against 43.1 us, tn 35.7 / 44.4; 4096 x 4096 x 7168: nn 102.0 / 100.8, tt 106.5 / 101.3 (re-majored: what the
// model picks), tn 106.0 / 115.4.
bool e8_mn_pays(const dg::GemmParams& p) {
    if (p.m <= 256 || 2L * ((p.m + 255) / 256) * ((p.n + 255) / 256) < num_cus())
        return false;
    if (p.k % 128 != 0)         // K tail: the alternative is a pass over B in front of the 128-ROW quad kernel (fp8_gemm_nn 4096 x 7168 x 2112:
        return true;            // 86 us against the FP32-scale kernel's 71 on the same operands) -- reading in place always pays
    double remajor_us = 0;
    const double b_mats = p.gemm_type == dg::kNormal ? 1.0 : static_cast<double>(p.num_groups);     // (grouped: the pass covers every group's weights)
    if (p.a_sk != 1) remajor_us += 3.0 + static_cast<double>(p.m) * p.k / 2.25e6;
    if (p.b_sk != 1) remajor_us += 3.0 + b_mats * p.n * p.k / 2.25e6;
    return remajor_us > static_cast<double>(p.m) * p.n * p.k / 6e9;
}

// Recipe (1, 1, 128) on the fast path: both scale tensors MN-major with 16-byte aligned K-block rows (each block's 256
// row scales are fetched as one 1 KiB LDS-DMA piece).
bool per_col_eligible(const dg::GemmParams& p) {
    return fast_eligible(p) && p.sfb_gran_n == 1 && p.gemm_type == dg::kNormal && p.sfa_sm == 1 && p.sfb_sn == 1 &&
           aligned16(p.sfa) && aligned16(p.sfb) && p.sfa_sk % 4 == 0 && p.sfb_sk % 4 == 0;
}

// The same recipe with BOTH operands MN-major ([K][M] and [K][N], unit stride along m / n): the transpose-read form of the
// kernel takes them as they are (dense TN wgrad GEMMs, the TN form of the K-grouped GEMM).
bool per_col_mn_eligible(const dg::GemmParams& p) {
    return p.sfb_gran_n == 1 && p.gemm_type == dg::kNormal && p.a_sm == 1 && p.b_sn == 1 && p.k % 128 == 0 &&
           aligned16(p.a) && aligned16(p.b) && p.a_sk % 16 == 0 && p.b_sk % 16 == 0 && p.a_sk <= (1 << 22) &&
           p.b_sk <= (1 << 22) && static_cast<int64_t>(p.k) * p.a_sk < (1LL << 31) &&
           static_cast<int64_t>(p.k) * p.b_sk < (1LL << 31) && p.sfa_sm == 1 && p.sfb_sn == 1 && aligned16(p.sfa) &&
           aligned16(p.sfb) && p.sfa_sk % 4 == 0 && p.sfb_sk % 4 == 0;
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Tile height of the K-major recipe-(1, 1, 128) kernel, 256 or 192 rows.  The recipe is VALU-issue bound, so time follows the rows a
// workgroup computes: with the K axis split over the idle CUs (`split`) the total counts -- ceil(m / bm) * bm, m = 576: 576 against 768 --,
// otherwise the rounds of resident tiles times the tile height (m = 2112, n = 4096: one round of 176 tiles of 192 rows against one round of
// 144 tiles of 256; m = 4096: 352 tiles = two rounds of 192 against one of 256).
int per_col_bm(const dg::GemmParams& p, bool split) {
    if (env_knobs().pc_bm == 192 || env_knobs().pc_bm == 256)          // (tuning runs, DG_PC_BM)
        return env_knobs().pc_bm;
    const long nt = ceil_div(p.n, 256), cus = num_cus();
    const long t192 = ceil_div(p.m, 192) * nt, t256 = ceil_div(p.m, 256) * nt;
    const long c192 = split ? ceil_div(p.m, 192) * 192L : (t192 + cus - 1) / cus * 192;
    const long c256 = split ? ceil_div(p.m, 256) * 256L : (t256 + cus - 1) / cus * 256;
    return c192 < c256 ? 192 : 256;
}

// Non-temporal output stores (GemmParams::d_nt): when one launch writes at least half of the chip's 32 MiB of L2 the output cannot stay
// cache-resident for its consumer anyway, and streaming it out is 5-6 % of a C2 call (see store_rows_full_line_packed).
int output_streams_past_l2(const dg::GemmParams& p) {
    const int64_t rows = p.gemm_type == dg::kMasked ? static_cast<int64_t>(p.num_groups) * p.m : p.m;
    return !p.accumulate && rows * p.n * (p.d_dtype == DG_BF16 ? 2 : 4) >= (16LL << 20) ? 1 : 0;
}

// K pieces per tile of the partial last round (0 = no split): as many as the idle workgroup slots allow, at most 8 and at most
// one per K block.  A launch of fewer tiles than slots is all "last round": every tile is cut (dense problems with few tiles
// and a long K loop, e.g. the dgrad shape 4096 x 512 x 32768: 64 tiles of 128 x 256).
long split_k_pieces(long tiles, long slots, long num_kb) {
    const long tail = tiles % slots;
    if (tiles <= 0 || tail == 0)
        return 0;
    long pieces = slots / tail;
    if (pieces > 8) pieces = 8;
    if (pieces > num_kb) pieces = num_kb;
    return pieces >= 2 ? pieces : 0;
}

// Does the split pay?  It trades (1 - 1/pieces) of a tile's K loop (~1 us per K block of a 128 x 256 tile) for the partial-tile
// exchange: the FP32 partials go to the workspace and a second kernel sums them (~11 us + 1 us per piece with the kernel
// boundary; the single-kernel form with a last-arriver reduction cost 17 us + 1.3 us per piece).  tools/grouped_bench.py,
// 8 groups x N 4096 with 16..128 tail tiles: K = 7168 gains 15..25 us of ~175, K = 4096 5..12 us of ~100, K = 2048 about even.
bool split_k_pays(long pieces, long num_kb) {
    return pieces >= 2 && num_kb * (pieces - 1) * 100 > (1100 + 100 * pieces) * pieces;
}

// SFA as the reference's callers hold it before the layout step: [M][ceil(K / 128)] floats, unit stride along K.
bool sfa_row_major(const dg::GemmParams& p) { return p.sfa_sk == 1 && p.sfa_sm != 1 && p.m > 1; }

// Picks the configuration with the lowest modelled time: (#rounds of resident blocks) x (tile work / efficiency).
const Config* select_config(const dg::GemmParams& p, int m_for_tiling, int expected_m, int bm_must_divide, bool ignore_forced = false) {
    const std::string forced = ignore_forced ? std::string("auto") : forced_config();
    if (forced != "auto") {
        for (int i = 0; i < kNumConfigs; ++i)
            if (forced == kConfigs[i].name)
                return &kConfigs[i];
        return nullptr;
    }
    if (sfa_row_major(p) && env_knobs().sfa_rowmajor_in_place) {
        // (DG_SFA_ROWMAJOR_IN_PLACE=1 + a DG_EXPERIMENTS build only: a measured negative, 141 against 92 us -- never part of the automatic selection)
        // a row-major SFA: taken in place where the MN-major twin of the problem would run duo_p_256x256 (dg_dense_rowmajor_sfa_native tells
        // the host layer, which otherwise transposes first)
        if (p.gemm_type == dg::kNormal && p.sfb_gran_n == 128 && p.head_lr == 0 && fast_eligible(p)) {
            dg::GemmParams q = p;
            q.sfa_sm = 1; q.sfa_sk = (p.m + 3) / 4 * 4; q.sk_workspace = nullptr;
            const Config* twin = select_config(q, m_for_tiling, expected_m, bm_must_divide, true);
            if (twin != nullptr && std::strcmp(twin->name, "duo_p_256x256") == 0)
                for (int i = 0; i < kNumConfigs; ++i)
                    if (std::strcmp(kConfigs[i].name, "duo_p_rm_256x256") == 0)
                        return &kConfigs[i];
        }
    }
    if (p.sfb_gran_n == 1) {
        const char* pick = per_col_eligible(p) && p.m > 64 ? (per_col_bm(p, false) == 192 ? "pipe_pc_192x256" : "pipe_pc_256x256")
                         : (per_col_mn_eligible(p) && p.m > 64 ? "pipe_pc_mn_256x256" : "generic_128x128");
        for (int i = 0; i < kNumConfigs; ++i)
            if (std::strcmp(kConfigs[i].name, pick) == 0)
                return &kConfigs[i];
    }
    if (amn_eligible(p) && m_for_tiling > 256) {
        const char* pick = p.b_sk == 1 ? "duo_amn_256x256" : "duo_abmn_256x256";
        for (int i = 0; i < kNumConfigs; ++i)
            if (std::strcmp(kConfigs[i].name, pick) == 0)
                return &kConfigs[i];
    }
    if (bmn_eligible(p) && m_for_tiling > 256) {
        const bool contiguous = p.gemm_type != dg::kNormal;
        const long tiles256 = static_cast<long>(ceil_div(m_for_tiling, 256)) * ceil_div(p.n, 256);
        // dense: rounds x tile work of the two tile shapes, with the weights of the K-major table (duo_256x256 1.10, duo_128x256 0.78):
        // e.g. 4096 x 2048 x 7168 = 128 / 256 tiles: one round either way, 76.1 us on 256-row tiles, 60.6 on 128-row tiles
        const long tiles128r = static_cast<long>(ceil_div(m_for_tiling, 128)) * ceil_div(p.n, 256);
        const double cost256 = static_cast<double>((tiles256 + num_cus() - 1) / num_cus()) * (256.0 * 256.0 / 1.10 + 4096.0);
        const double cost128 = static_cast<double>((tiles128r + num_cus() - 1) / num_cus()) * (128.0 * 256.0 / 0.78 + 4096.0);
        const char* pick = (contiguous || cost128 < cost256) ? "duo_bmn_128x256" : "duo_bmn_256x256";
        if (p.k % 128 != 0)             // (dense only, see bmn_eligible) the forms with the K-tail stage
            pick = cost128 < cost256 ? "duo_bmn_kt_128x256" : "duo_bmn_kt_256x256";
        else if (std::strcmp(pick, "duo_bmn_128x256") == 0 && p.sk_workspace != nullptr &&
                 (!contiguous || bm_must_divide % 128 == 0)) {
            // a partial last round (or an under-filled launch) of 128 x 256 tiles: cut it along K over the idle CUs
            const long tiles = static_cast<long>(ceil_div(m_for_tiling, 128)) * ceil_div(p.n, 256);
            if (split_k_pays(split_k_pieces(tiles, num_cus(), p.k / 128), p.k / 128))
                pick = "duo_sk_bmn_128x256";
        }
        // many rounds of a contiguous layout aligned to 128 rows: the two-pass 256-row tile (same rule as for K-major B)
        if (p.gemm_type == dg::kContiguous && bm_must_divide == 128 && tiles256 >= 4L * num_cus())
            pick = "duo_bmn_256x256";     // (persistent, two-pass walk: 4-14 % over the one-tile-per-workgroup launch)
        if (!contiguous || bm_must_divide % 128 == 0)
            for (int i = 0; i < kNumConfigs; ++i)
                if (std::strcmp(kConfigs[i].name, pick) == 0)
                    return &kConfigs[i];
    }
    const bool fast_ok = fast_eligible(p);
    const bool tail_ok = fast_eligible(p, false);       // k % 128 != 0: only the kernels with a tail stage
    if (!fast_ok && tail_ok && p.sfb_gran_n == 128 && p.sfa_sm == 1 && p.gemm_type == dg::kNormal) {
        const long tiles256 = static_cast<long>(ceil_div(m_for_tiling, 256)) * ceil_div(p.n, 256);
        const char* pick = tiles256 <= num_cus() / 2 ? "duo_kt_128x256" : "duo_kt_256x256";
        for (int i = 0; i < kNumConfigs; ++i)
            if (std::strcmp(kConfigs[i].name, pick) == 0)
                return &kConfigs[i];
    }
    // Decode batches (M <= 32), dense: the skinny weight-stream kernel (every CU streams its own 16 columns with 128 KiB in flight;
    // tools/survey.py m = 1 rows: 19-21 us on the stream tiles -> see DESIGN.md)
    // (tools/skinny_bench.py, whole eager call / hipGraph replay: m = 1, 4096 x 7168: 18.4 -> 12.1 / 7.4 us; 7168 x 16384: 36.0 -> 27.8 us;
    // short K loops -- k = 512, 1536: 4 and 12 K blocks for 8 waves -- and wide N stay on the stream tiles (12.4 us against 18-23);
    // 17..32 rows re-read A twice as often as they read B: only the k = 7168, n <= 4608 class gains, 18.4 -> 15 us)
    if (fast_ok && p.gemm_type == dg::kNormal && p.sfb_gran_n == 128 && p.head_lr == 0 && p.n % 16 == 0) {
        const int num_kb = p.k / 128;
        const char* pick = nullptr;
        // round 5: the coalesced-load forms ('c': 8 weight rows x 128 bytes per load instruction, operands through wave-private LDS) -- same
        // bits, 10-18 % faster on every shape measured (profiles/r05_probe/skinny_coalesced_ab.jsonl: m = 1, 4096 x 7168 9.2 -> 8.3 us,
        // 7168 x 16384 27.8 -> 24.4 / 23.7, m = 16 11.9 -> 10.0, m = 32 15.8 -> 13.4)
        // ... and, up to 16 rows, the activation loads too ('ca': m = 1, 4096 x 7168 8.4 -> 7.7 us, m = 16 10.0 -> 9.0; skinny_coalesced_activations_ab.jsonl)
        if (m_for_tiling <= 16 && num_kb >= 16)
            pick = (p.n > 16 * num_cus() && p.n <= 32 * num_cus() && !p.accumulate && p.n % 4 == 0 && num_kb < 32) ? "skinny_16wc" : "skinny_16ca";
        // (two N-subtiles per workgroup -- one round instead of 1.x -- only pay with short K loops now: 16 x 8192 x 2048 7.4 against 8.0 us, but
        //  1 x 7168 x 4096 8.7 against 8.6, 1 x 6144 x 7168 13.3 against 12.8, 4 x 7168 x 16384 25.0 against 24.7)
        // (17 .. 32 rows: coalesced activation loads with three K blocks per chunk from K = 6144 -- 32 x 4096 x 7168 13.3 -> 12.1 us, 32 x 4608 x 8192
        //  23.6 -> 21.1; four K blocks per wave (K = 4096) want the four-block chunks: 7.6 against 8.3; skinny_32_coalesced_activations_ab.jsonl)
        // (end of round 6: narrow layers -- at most 48 tiles of 64 x 32 -- with K >= 7168 and the caller's workspace leave 17 .. 32 rows to the
        //  64 x 32 stream tile cut along K, below: a skinny launch is one workgroup per 16 columns, 36 for n = 576.  hipGraph replays, cold weights,
        //  m = 17 / 24 / 32: 576 x 7168 9.8 / 10.4 / 11.2 -> 8.9 / 9.0 / 9.0 us, 1536 x 7168 10.1 / 10.7 / 11.5 -> 9.1 / 9.2 / 9.3; from n = 2112 the
        //  skinny kernel ties or wins -- profiles/r06_probe/m17_32_skinny_vs_ks.log)
        else if (m_for_tiling > 16 && m_for_tiling <= 32 && num_kb >= 32 && num_kb <= 64 && p.n <= 4608 &&
                 !(p.sk_workspace != nullptr && num_kb >= 56 && ceil_div(p.n, 32) <= 48 &&
                   4096 + 32768 + static_cast<size_t>(ceil_div(p.n, 32)) * 8 * 64 * 32 * sizeof(float) <= g_workspace_bytes))
            pick = num_kb >= 48 ? "skinny_32ca" : "skinny_32c";
        if (pick != nullptr)
            for (int i = 0; i < kNumConfigs; ++i)
                if (std::strcmp(kConfigs[i].name, pick) == 0)
                    return &kConfigs[i];
    }
    // HBM-bound shapes (M up to a few 64-row tiles: every weight byte is streamed once or twice): the deep-ring stream
    // kernels.  A CU sustains only ~25 GB/s of HBM stream (bytes in flight / latency), so the tile count has to cover
    // the chip: 64 x 128 tiles when there are enough of them, 64 x 32 otherwise (measured: tools/ref_shapes.py).
    const int m_hint = expected_m > 0 ? expected_m : m_for_tiling;
    if (fast_ok && sfa_quads_ok(p) && p.gemm_type != dg::kContiguous && p.gemm_type != dg::kContiguousPsum) {
        const int groups = (p.gemm_type == dg::kMasked) ? p.num_groups : 1;
        const long tiles128 = static_cast<long>(groups) * ceil_div(m_hint, 64) * ceil_div(p.n, 128);
        const char* pick = nullptr;
        if (m_hint <= 64)
            pick = tiles128 >= 96 ? "stream_64x128" : "stream_64x32";
        else if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal && p.k >= 4096 ? 128 : 96))
            pick = "stream_64x32";      // (dense: up to half a round of 64 x 128 tiles while the K loop is long; with a short one the two-per-CU
                                        //  64 x 128 tile wins -- m = 128, 7168 x 2048, 112 tiles, cold: 12.7 us against 14.2: small_m_sweep_forced.log)
        else if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal ? 2L * num_cus() + 1 : 256))
            pick = "stream_64x128";     // (dense: up to ONE resident round of two tiles per CU -- end of round 6, cold weights, m = 128:
                                        //  24576 x 1536 21.4 us on 96 tiles of 128 x 256 -> 18.5, 32768 x 512 12.7 -> 10.0)
        else if (m_hint > 256 && tiles128 <= num_cus())
            pick = "stream_64x128";     // one resident round of 64 x 128 tiles (512 x 4096 x 7168: 36.9 us against 47.3 on 128 x 256 tiles)
        // ... unless the K loop is long and the caller lent a workspace: cutting every 128 x 256 tile along K over the idle CUs
        // beats one deep-ring tile per CU (tools/sweep.py: 4096 x 512 x 32768: 88.6 us against 166.4; 1024 x 1024 x 16384: 41.3 / 79.5;
        // 1024 x 512 x 8192: 30.5 / 42.8; break-even near K = 7168 -- 512 x 4096 x 7168: 38.7 / 39.7, 4096 x 512 x 4096: 32.6 / 25.3).
        // Model: stream = 5 us + 0.66 (64 x 128) or 0.27 (64 x 32, four K blocks per stage) us per K block, split = 16 us + 1.05 us per K block of a piece
        // (two-phase exchange: 1024 x 512 x 8192 21.8 us, 1024 x 1024 x 16384 33.2, 512 x 4096 x 7168 31.3, 4096 x 512 x 4096 25.2 / stream 24.2).
        // (Rounds 2-4 sent decode-sized M with MORE 64 x 128 tiles than CUs to the 128 x 256 duo tile -- the second round of one-tile-per-CU
        // stream tiles was mostly idle.  With two workgroups per CU, below, the stream tile wins or ties on every shape of that class:
        // 8 experts x 7168 x 2048 25.5 us against 29.9, 6 x 7168 x 3072 33.8 / 36.7, 16 x 7168 x 2048 49.4 / 56.1, 8 x 7168 x 4096 49.8 / 57.6,
        // 12 x 4096 x 7168 71.5 / 73.3, 6 x 6144 x 7168 64.9 / 64.0, 32 x 4096 x 7168 164.7 / 165.8 -- profiles/r05_probe/stream2_masked.jsonl.)
        // round 5: the 64 x 128 stream tile runs with a 3-stage ring and TWO workgroups per CU (stream2_64x128): 8 waves issue the CU's LDS-DMA
        // pieces instead of 4, 257 .. 512 tiles are one resident round, and ramps of one workgroup hide behind the other's steady state --
        // rotating input sets, same box: C5 43.4 -> 41.6 us, dense 64 x 24576 x 1536 13.1 -> 11.2, 256 x 7168 x 2048 14.6 -> 12.9
        // (profiles/r05_probe/stream2_masked.jsonl, stream2_dense.jsonl).  Non-temporal weight stream from 80 MB of weights per launch
        // (117 MB: 25.5 us against 28.3 with the default policy; 59 MB: 14.3 against 14.0).
        if (pick != nullptr && std::strcmp(pick, "stream_64x128") == 0)
            pick = static_cast<double>(groups) * p.n * p.k >= kNonTemporalWeightBytes ? "stream_nt2_64x128" : "stream2_64x128";
        // round 6: 129 .. 256 rows whose 64 x 128 tiles fill at most half the chip: the same tile with every tile cut along K inside the kernel
        // (stream_ks_64x128: one launch, pieces x tiles resident, FP32 partials through written-through slabs, the last piece of a tile sums
        // them in piece order).  Cold inputs, us: 160 x 4096 x 7168 27.5 -> 23.4, 192 x .. 30.4 -> 23.7, 256 x .. 30.6 -> 24.5 (was duo_sk_128x256),
        // 256 x 2112 x 7168 27.2 -> 19.4, 192 x 4096 x 4096 20.4 -> 17.3.  NOT up to 128 rows (128 x 4096 x 7168 16.7 -> 18.0, 128 x 2112 x 7168
        // 16.3 -> 24.4: the 64 x 32 tiles with loader waves already cover the chip), not with short K loops (256 x 4096 x 2048 12.7 -> 13.4), not
        // under 64 tiles (192 x 2112 x 7168 16.6 -> 16.8) unless the K loop is so long that the 8-wave K split below would take the problem (33 .. 63
        // tiles -- up to 32 the 64 x 32 tile is cut -- from K = 10240: 192 x 1536 x 16384 28.1 (duo_sk_128x256) -> 21.4, 192 x 2048 x 16384 29.2 -> 24.1:
        // profiles/r06_probe/ks_vs_duo_sk_ab.log).  profiles/r06_probe/stream_ks_mid_m_ab.log
        // ... and 65 .. 128 rows on WIDE layers (last session, profiles/r06_probe/m128_long_k_ab.log): over 64 tiles (> 256 tiles of 64 x 32: 128 x 5120 x 7168
        // 29.1 -> 20.0 us, stream_ks_64x64_ab.log) the 64 x 32 tiles'
        // second half-round costs more than the exchange -- 128 x 6144 x 7168 29.8 -> 23.8 us, 128 x 7168 x 8192 32.8 -> 26.8 (K up to 10240: at
        // 128 x 7168 x 16384 the 8-wave K split runs 40.2 against 48.9) -- and 64 .. 95 tiles with K >= 10240 (128 x 4096 x 10240 26.9 -> 22.3,
        // 128 x 4096 x 16384 32.0 -> 28.2; at K = 7168 the 64 x 32 tiles stay: 16.7 against 18.0)
        const bool ks_rows_129_256 = m_for_tiling > 128 && m_for_tiling <= 256 && (tiles128 >= 64 || (tiles128 > 32 && p.k >= 10240));
        const bool ks_rows_65_128 = m_for_tiling > 64 && m_for_tiling <= 128 &&
                                    ((tiles128 > 64 && p.k >= 7168 && p.k <= 10240) || (tiles128 == 64 && p.k >= 10240));
        if (pick != nullptr && p.gemm_type == dg::kNormal && p.sk_workspace != nullptr && p.sfb_gran_n == 128 && p.head_lr == 0 &&
            (ks_rows_129_256 || ks_rows_65_128) && p.k >= 4096 && tiles128 * 2 <= num_cus() &&
            4096 + 32768 + static_cast<size_t>(tiles128) * 8 * 64 * 128 * sizeof(float) <= g_workspace_bytes) {
            for (int i = 0; i < kNumConfigs; ++i)
                if (std::strcmp(kConfigs[i].name, "stream_ks_64x128") == 0)
                    return &kConfigs[i];
        }
        // last session: a 64 x 64 tile (two K blocks per stage, four stages) cut likewise, where its tiles get three or more pieces and the 64 x 32 tiles
        // would get two or none -- 48 .. CUs / 3 tiles, K >= 7168, 33 .. 128 rows: 128 x 2112 x 7168 15.6 -> 13.6 us, 128 x 1536 x 7168 12.6-13.4 -> 11.8,
        // 64 x 4096 x 7168 14.0 -> 13.1; NOT at two pieces (128 x 4096 x 7168 16.1 -> 17.3, 128 x 3072 x 7168 15.9 -> 15.7) -- profiles/r06_probe/stream_ks_64x64_ab.log
        if (pick != nullptr && p.gemm_type == dg::kNormal && p.sk_workspace != nullptr && p.sfb_gran_n == 128 && p.head_lr == 0 && p.k >= 7168 &&
            m_for_tiling > 32 && m_for_tiling <= 128) {
            const long tiles64 = static_cast<long>(ceil_div(m_for_tiling, 64)) * ceil_div(p.n, 64);
            if (tiles64 >= 48 && tiles64 * 3 <= num_cus() && 4096 + 32768 + static_cast<size_t>(tiles64) * 8 * 64 * 64 * sizeof(float) <= g_workspace_bytes)
                for (int i = 0; i < kNumConfigs; ++i)
                    if (std::strcmp(kConfigs[i].name, "stream_ks_64x64") == 0)
                        return &kConfigs[i];
        }
        // end of round 6: dense problems whose 64 x 32 tiles fill at most half the chip, with a long K loop and the caller's workspace: the tile cut
        // along K inside the kernel (stream_ks_64x32: min(8, CUs / tiles, K blocks / 4) pieces).  Eager calls, cold weights, us: 128 x 576 x 7168 (the
        // MLA down-projection of the reference's sweep, 36 tiles) 15.4 -> 9.6, 64 x 2112 x 7168 16.0 -> 11.7, 256 x 576 x 7168 15.6 -> 11.3,
        // 64 x 4096 x 7168 (128 tiles, two pieces) 16.2 -> 13.2, 128 x 576 x 16384 27.7 (duo_sk_128x256) -> 12.4 -- profiles/r06_probe/stream_ks_64x32_ab.log
        if (pick != nullptr && p.gemm_type == dg::kNormal && std::strcmp(pick, "stream_64x32") == 0 && p.sk_workspace != nullptr && p.sfb_gran_n == 128 &&
            p.head_lr == 0 && p.k >= 4096) {
            const long tiles32 = static_cast<long>(ceil_div(m_for_tiling, 64)) * ceil_div(p.n, 32);
            if (tiles32 * 2 <= num_cus() && 4096 + 32768 + static_cast<size_t>(tiles32) * 8 * 64 * 32 * sizeof(float) <= g_workspace_bytes)
                for (int i = 0; i < kNumConfigs; ++i)
                    if (std::strcmp(kConfigs[i].name, "stream_ks_64x32") == 0)
                        return &kConfigs[i];
        }
        if (pick != nullptr && p.gemm_type == dg::kNormal && p.sk_workspace != nullptr && p.sfb_gran_n == 128 && m_hint > 64) {
            const long tiles = static_cast<long>(ceil_div(m_for_tiling, 128)) * ceil_div(p.n, 256);
            const long num_kb = p.k / 128;
            const long pieces = split_k_pieces(tiles, num_cus(), num_kb);
            if (pieces >= 2 && tiles < num_cus()) {
                const double t_stream = 5.0 + num_kb * (std::strcmp(pick, "stream_64x32") == 0 ? 0.27 : 0.66);
                const double t_split = 16.0 + static_cast<double>((num_kb + pieces - 1) / pieces) * 1.05;
                if (t_split < t_stream)
                    pick = "duo_sk_128x256";
            }
        }
        // round 4: dense 64 x 32 stream tiles run with four loader waves beside the four compute waves (8 waves issue the LDS-DMA pieces:
        // m = 128, 4096 x 7168: 20.9 -> 18.0 us, 2112 x 7168: 20.4 -> 17.0, 7168 x 2048: 16.8 -> 15.3; profiles/r04_probe/sweep_midm_loader_waves.jsonl;
        // the 64 x 128 tile and the masked C5 did not move: 39.8 against 38.4, 43.7 against 43.6)
        if (pick != nullptr && p.gemm_type == dg::kNormal && std::strcmp(pick, "stream_64x32") == 0)
            pick = "stream_l8_64x32";
        if (pick != nullptr)
            for (int i = 0; i < kNumConfigs; ++i)
                if (std::strcmp(kConfigs[i].name, pick) == 0)
                    return &kConfigs[i];
    }
    const Config* best = nullptr;
    double best_cost = 0;
    for (int i = 0; i < kNumConfigs; ++i) {
        const Config& c = kConfigs[i];
        if ((c.fast && !(fast_ok || (c.k_tail && tail_ok))) || c.efficiency <= 0.f || (c.ring && p.sfa_sm != 1))
            continue;
        if (bm_must_divide > 0 && bm_must_divide % c.bm != 0 &&
            !(c.two_pass && p.gemm_type == dg::kContiguous && c.bm == 2 * bm_must_divide))
            continue;
        const int m_eff = expected_m > 0 ? expected_m : m_for_tiling;
        const int groups = (p.gemm_type == dg::kMasked) ? p.num_groups : 1;
        long tiles = static_cast<long>(groups) * ceil_div(m_eff, c.bm) * ceil_div(p.n, c.bn);
        const long slots = static_cast<long>(num_cus()) * c.blocks_per_cu;
        if (bm_must_divide > 0 && bm_must_divide % c.bm != 0) {
            // two-pass tiles (BM = 2 x alignment): tiles whose halves belong to two groups cost twice and land anywhere
            // in the schedule, so the big tile only pays when there are several rounds to average over
            if (tiles < 4 * slots)
                continue;
            tiles += tiles / 4;
        }
        const long rounds = (tiles + slots - 1) / slots;
        // A round costs the work of blocks_per_cu co-resident tiles per CU; tiny tiles are HBM/latency dominated.
        const double tile_work = static_cast<double>(c.bm) * c.bn / c.efficiency + 4096.0;
        const double cost = static_cast<double>(rounds) * c.blocks_per_cu * tile_work;
        if (best == nullptr || cost < best_cost) {
            best = &c;
            best_cost = cost;
        }
    }
    // A partial last round (or an under-filled launch) of 128 x 256 tiles: split it along K over the idle CUs (needs the caller's
    // workspace; see split_k_pays).
    if (best != nullptr && std::strcmp(best->name, "duo_128x256") == 0 && p.sk_workspace != nullptr &&
        p.gemm_type != dg::kMasked) {
        const long tiles = static_cast<long>(ceil_div(m_for_tiling, 128)) * ceil_div(p.n, 256);
        if (split_k_pays(split_k_pieces(tiles, num_cus(), p.k / 128), p.k / 128))
            for (int i = 0; i < kNumConfigs; ++i)
                if (std::strcmp(kConfigs[i].name, "duo_sk_128x256") == 0)
                    return &kConfigs[i];
    }
    // Several tiles per CU: the persistent variant of the duo kernel (the next tile's first K blocks are fetched and
    // drained in front of the current tile's stores, which then overlap the next tile's first K block).
    // (Every layout: masked, 32 groups x ~192 rows: 2-4 %; contiguous two-pass walks of 8 x ~4096 / 4 x ~8192 rows: 4-15 % --
    // 378.8 -> 329.5 us at N 4096, K 2048, tools/grouped_bench.py.)
    if (best != nullptr && std::strcmp(best->name, "duo_256x256") == 0) {
        // (also with one tile per CU: 98.0 against 99.4 us sustained on 4096 x 4096 x 7168, tools/sustained.py)
        for (int i = 0; i < kNumConfigs; ++i)
            if (std::strcmp(kConfigs[i].name, "duo_p_256x256") == 0)
                return &kConfigs[i];
    }
    return best;
}

// Under-filled recipe-(1, 1, 128) launches (wgrad of a narrow layer: 576 x 4096 x 7168 = 48 tiles of 256 x 256 for 256 CUs, 56 K blocks at
// ~2.2 us each): the K axis is cut into `pieces` ranges that run as the groups of ONE K-grouped launch of the same kernel, each writing
// an FP32 partial matrix into the caller's workspace; dg_sum_partials_kernel then adds them in piece order and performs the operator's
// output step.  Returns the number of pieces (0 = one ordinary launch).  Model (us): one launch 15 + 2.2 per K block; split 30 + 2.2 per
// K block of a piece + the partials' write and read at ~4 TB/s.  workspace_bytes = 0: "as large as needed" (the host layer's query).
int per_col_split_pieces(const dg::GemmParams& p, size_t workspace_bytes, bool ignore_forced = false) {
    if (p.sfb_gran_n != 1 || p.gemm_type != dg::kNormal || p.head_lr > 0 || p.m <= 64 || p.k % 128 != 0 ||
        (!ignore_forced && forced_config() != "auto"))
        return 0;
    if (!per_col_eligible(p) && !per_col_mn_eligible(p))
        return 0;
    const long tiles = static_cast<long>(ceil_div(p.m, per_col_eligible(p) ? per_col_bm(p, true) : 256)) * ceil_div(p.n, 256), num_kb = p.k / 128;
    const size_t per_piece = static_cast<size_t>(p.m) * p.n * sizeof(float);
    long pieces = std::min<long>(std::min<long>(8, num_cus() / tiles), num_kb / 4);
    const long fit = workspace_bytes > 0 ? (workspace_bytes > 4096 ? static_cast<long>((workspace_bytes - 4096) / per_piece) : 0) : 8;
    pieces = std::min<long>(pieces, fit);
    if (pieces < 2 || num_kb < 24)
        return 0;
    if (env_knobs().ks_pieces >= 2)             // (tuning runs, DG_KS_PIECES: force the number of K pieces)
        return static_cast<int>(std::min<long>(std::min<long>(env_knobs().ks_pieces, fit), std::min<long>(8, num_kb / 4)));
    const double t_one = 15.0 + 2.2 * num_kb;
    const double t_split = 30.0 + 2.2 * ((num_kb + pieces - 1) / pieces) + static_cast<double>(pieces) * per_piece / 4.0e6;
    return t_split < 0.75 * t_one ? static_cast<int>(pieces) : 0;
}

int launch_per_col_split(const dg::GemmParams& dense, int pieces, void* stream) {
    dg::GemmParams p = dense;
    const bool mn_major = !per_col_eligible(dense);
    float* parts = reinterpret_cast<float*>(static_cast<uint8_t*>(dense.sk_workspace) + 4096);
    p.d = parts; p.d_sm = dense.n; p.d_sg = static_cast<int64_t>(dense.m) * dense.n; p.d_dtype = DG_FP32; p.accumulate = 0;
    p.gemm_type = dg::kKGrouped; p.num_groups = pieces; p.kg_blocks = 0; p.kg_psum = 0;
    p.sk_workspace = nullptr; p.sk_first_tile = 0; p.sk_tiles = 0; p.sk_factor = 1;
    const int num_kb = dense.k / 128;
    for (int i = 0; i <= pieces; ++i)
        p.kg_prefix[i] = 128 * static_cast<int>(static_cast<long>(i) * num_kb / pieces);
    const int bm = mn_major ? 256 : per_col_bm(dense, true);
    p.num_m_tiles = ceil_div(p.m, bm);
    p.num_n_tiles = ceil_div(p.n, 256);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    p.d_vec_ok = dense.n % 4 == 0;
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * pieces;
    g_last_config = mn_major ? "pipe_pc_mn_ks_256x256" : (bm == 192 ? "pipe_pc_ks_192x256" : "pipe_pc_ks_256x256");
    if (mn_major)
        hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, true>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                           static_cast<hipStream_t>(stream), p);
    else if (bm == 192)
        hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<192, 256, 2, 4, 1, false>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                           static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, false>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                           static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    const size_t elem = dense.d_dtype == DG_BF16 ? 2 : 4;
    const int vec_ok = dense.n % 4 == 0 && (dense.d_dtype == DG_BF16 || (aligned16(dense.d) && (dense.d_sm * elem) % 16 == 0));
    const long quads = static_cast<long>(dense.m) * ((dense.n + 3) / 4);
    const long blocks = std::min<long>((quads + 255) / 256, static_cast<long>(num_cus()) * 8);
    hipLaunchKernelGGL(dg::dg_sum_partials_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       parts, pieces, static_cast<int64_t>(dense.m) * dense.n, dense.d, dense.m, dense.n, dense.d_sm, dense.d_dtype,
                       dense.accumulate, vec_ok);
    DG_HIP_CHECK(hipGetLastError());
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] type=%d m=%d n=%d k=%d -> %s pieces=%d grid=%ld\n", dense.gemm_type, dense.m, dense.n, dense.k,
                g_last_config.c_str(), pieces, grid);
    return 0;
}

int launch_gemm(dg::GemmParams& p, int expected_m, void* stream) {
    if (p.sk_workspace != nullptr)
        if (const int pieces = per_col_split_pieces(p, g_workspace_bytes); pieces >= 2)
            return launch_per_col_split(p, pieces, stream);
    const int bm_must_divide =
        (p.gemm_type == dg::kContiguous || p.gemm_type == dg::kContiguousPsum) ? p.m_alignment : 0;
    const Config* cfg = select_config(p, p.m, expected_m, bm_must_divide);
    if (cfg == nullptr) {
        g_last_error = "no kernel configuration available (forced config '" + forced_config() + "')";
        return 3;
    }
    const bool amn_form = std::strcmp(cfg->name, "duo_amn_256x256") == 0 || std::strcmp(cfg->name, "duo_abmn_256x256") == 0;
    if (amn_form && !(amn_eligible(p) && (p.b_sk == 1) == (std::strcmp(cfg->name, "duo_amn_256x256") == 0))) {
        g_last_error = std::string("forced config '") + cfg->name + "' needs a dense problem with MN-major 16-byte aligned A, B of the "
                       "majorness in its name and MN-major SFA";
        return 3;
    }
    const bool bmn_form = std::strstr(cfg->name, "_bmn") != nullptr;       // duo_bmn_*, duo_sk_bmn_*
    if (bmn_form && !bmn_eligible(p)) {
        g_last_error = std::string("forced config '") + cfg->name + "' needs K-major A, MN-major 16-byte aligned B and MN-major SFA";
        return 3;
    }
    if (std::strncmp(cfg->name, "skinny", 6) == 0 && (p.m > cfg->bm || p.gemm_type != dg::kNormal || p.head_lr != 0)) {
        g_last_error = std::string("forced config '") + cfg->name + "' implements dense problems with m <= its row count";
        return 3;
    }
    if (std::strncmp(cfg->name, "stream", 6) == 0 && !sfa_quads_ok(p)) {
        g_last_error = std::string("forced config '") + cfg->name + "' needs MN-major SFA with 16-byte aligned K-block rows";
        return 3;
    }
    if (p.k % 128 != 0 && cfg->fast && !cfg->k_tail) {
        g_last_error = std::string("forced config '") + cfg->name + "' needs k % 128 == 0";
        return 3;
    }
    if (cfg->k_tail && (p.gemm_type != dg::kNormal || p.sfb_gran_n != 128 || p.sfa_sm != 1)) {
        g_last_error = std::string("forced config '") + cfg->name + "' implements dense problems with per-128 SFB and MN-major SFA";
        return 3;
    }
    const bool pc_mn_form = std::strcmp(cfg->name, "pipe_pc_mn_256x256") == 0;
    const bool mn_form = pc_mn_form || bmn_form || amn_form;
    if (cfg->fast && !bmn_form && !amn_form &&
        (pc_mn_form ? !per_col_mn_eligible(p) : (cfg->per_col ? !per_col_eligible(p) : p.sfb_gran_n != 128))) {
        g_last_error = std::string("forced config '") + cfg->name + "' does not implement this scaling recipe / SF layout";
        return 3;
    }
    if (cfg->fast && !mn_form && !fast_eligible(p, !cfg->k_tail)) {
        g_last_error = std::string("forced config '") + cfg->name + "' needs K-major 16-byte aligned operands and k % 128 == 0" +
                       (cfg->k_tail ? " (or k % 16 == 0 and k > 128)" : "");
        return 3;
    }
    if (cfg->sfa_rm ? !(sfa_row_major(p) && p.gemm_type == dg::kNormal && p.sfb_gran_n == 128 && p.head_lr == 0) : (cfg->ring && p.sfa_sm != 1)) {
        g_last_error = std::string("forced config '") + cfg->name + (cfg->sfa_rm ? "' needs a dense problem with a row-major SFA (sfa_stride_k == 1)"
                                                                                 : "' needs MN-major SFA (sfa_stride_m == 1)");
        return 3;
    }
    if (bm_must_divide > 0 && bm_must_divide % cfg->bm != 0 &&
        !(cfg->two_pass && p.gemm_type == dg::kContiguous && cfg->bm == 2 * bm_must_divide)) {
        g_last_error = std::string("config '") + cfg->name + "' does not divide the contiguous-layout M alignment";
        return 3;
    }
    g_last_config = cfg->name;
    p.num_m_tiles = ceil_div(p.m, cfg->bm);
    p.num_n_tiles = ceil_div(p.n, cfg->bn);
    if (std::strncmp(cfg->name, "skinny_16w", 10) == 0) {
        if (p.accumulate) {
            g_last_error = "config 'skinny_16w' does not implement accumulating outputs (neighbouring workgroups overlap by up to 15 columns)";
            return 3;
        }
        // columns per workgroup: one round over the CUs if that needs at most 32 columns, a multiple of 4 (8-byte BF16 stores)
        int cols = ceil_div(ceil_div(p.n, num_cus()), 4) * 4;
        cols = cols < 20 ? 20 : (cols > 32 ? 32 : cols);
        p.skinny_cols = cols;
        p.num_n_tiles = ceil_div(p.n, cols);
    }
    // L2 grouping: with 8 XCDs each chunk of tiles should be a compact rectangle (see swizzled_tile).
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    if (env_knobs().group_m > 0)                     // (tuning runs, DG_GROUP_M: M tiles per L2 group of the tile walk)
        p.group_m = std::max(1, std::min(env_knobs().group_m, p.num_m_tiles));
    const size_t elem = p.d_dtype == DG_BF16 ? 2 : 4;
    p.d_vec_ok = aligned16(p.d) && (p.d_sm * elem) % 16 == 0 && (p.d_sg * elem) % 16 == 0;
    p.d_nt = output_streams_past_l2(p);
    if (p.head_lr > 0 && ((p.head_lr - p.head_right) % 8 != 0 || p.head_mid % 8 != 0 || p.head_right % 8 != 0))
        p.d_vec_ok = 0;                  // a 16-byte store would straddle a head split: element-wise stores
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);

    long grid;
    const long total = static_cast<long>(p.num_m_tiles) * p.num_n_tiles;
    p.sk_first_tile = static_cast<int>(total);
    p.sk_tiles = 0;
    p.sk_factor = 1;
    const bool stream_ks = std::strncmp(cfg->name, "stream_ks_", 10) == 0;
    if (stream_ks) {
        // K pieces of the stream tile (see stream_kernel_body, KSPLIT): as many as keep tiles x pieces within one resident round, at most 8 and
        // at least four K blocks each; flags and slabs live in the caller's workspace
        const long slots = num_cus();
        long pieces = std::min<long>(std::min<long>(env_knobs().ks_max_pieces, total > 0 ? slots / total : 0), p.k / 128 / 4);
        const size_t need = 4096 + 32768 + static_cast<size_t>(total) * 8 * cfg->bm * cfg->bn * sizeof(float);
        if (p.gemm_type != dg::kNormal || p.sfb_gran_n != 128 || p.head_lr != 0 || !sfa_quads_ok(p) || total > 1024) {
            g_last_error = "the stream_ks configurations implement dense problems with per-128 SFB and MN-major SFA with 16-byte aligned K-block rows";
            return 3;
        }
        if (pieces < 2 || p.sk_workspace == nullptr || need > g_workspace_bytes)
            pieces = 1;                             // whole tiles (no workspace, too many tiles): the plain 6-stage stream tile
        p.sk_factor = static_cast<int>(pieces);
        p.sk_exchange = 0x7fc00000u | (g_stream_ks_epoch.fetch_add(1, std::memory_order_relaxed) & 0xfffffu) | 0x100000u;
        const long items = total * pieces;
        hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(std::min<long>(items, slots))), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), p);
        DG_HIP_CHECK(hipGetLastError());
        if (env_knobs().print_configs)
            fprintf(stderr, "[deepgemm_amd] type=%d m=%d n=%d k=%d -> %s pieces=%ld items=%ld\n", p.gemm_type, p.m, p.n, p.k, cfg->name, pieces, items);
        return 0;
    }
    if (cfg->split_k) {
        if (p.gemm_type == dg::kMasked) {
            g_last_error = std::string("config '") + cfg->name + "' does not implement the masked layout";
            return 3;
        }
        const long slots = static_cast<long>(num_cus()) * cfg->blocks_per_cu;
        const long tail = total % slots;
        const long pieces = split_k_pieces(total, slots, p.k / 128);
        const size_t need = 4096 + static_cast<size_t>(tail) * pieces * cfg->bm * cfg->bn * sizeof(float);
        if (tail > 0 && pieces >= 2 && p.sk_workspace != nullptr && need <= g_workspace_bytes) {
            p.sk_first_tile = static_cast<int>(total - tail);
            p.sk_tiles = static_cast<int>(tail);
            p.sk_factor = static_cast<int>(pieces);
        }                                           // otherwise: a plain persistent walk over all tiles
    }
    if (p.gemm_type == dg::kMasked) {
        const long slots = static_cast<long>(num_cus()) * cfg->blocks_per_cu;
        const long max_tiles = total * p.num_groups;
        grid = max_tiles < slots ? max_tiles : slots;
    } else if (cfg->persistent) {
        const long slots = static_cast<long>(num_cus()) * cfg->blocks_per_cu;
        const long items = static_cast<long>(p.sk_first_tile) + static_cast<long>(p.sk_tiles) * p.sk_factor;     // = total without a split
        grid = items < slots ? items : slots;
    } else {
        grid = total;
    }
    if (grid <= 0)
        return 0;
    if (grid > 0x7fffffffL)
        return fail(__FILE__, __LINE__, "grid too large");
    hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(grid)), dim3(cfg->threads), 0,
                       static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    if (cfg->split_k && p.sk_tiles > 0 && p.sk_factor >= 2) {
        // second phase of the K split: the partial tiles' sum and the output stores, one workgroup per (tile, M-subtile row)
        const KernelFn reduce = bmn_form ? dg::dg_split_k_reduce_kernel<128, 256, 2, 4, true>
                                         : dg::dg_split_k_reduce_kernel<128, 256, 2, 4, false>;
        hipLaunchKernelGGL(reduce, dim3(static_cast<unsigned>(p.sk_tiles * 4)), dim3(512), 0, static_cast<hipStream_t>(stream), p);
        DG_HIP_CHECK(hipGetLastError());
    }
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] type=%d m=%d n=%d k=%d groups=%d -> %s grid=%ld\n", p.gemm_type, p.m, p.n, p.k,
                p.num_groups, cfg->name, grid);
    return 0;
}

// Contiguous layout, M alignment 128, K-major operands, at least a round of 128-row tiles: the group-relative tiling.
//   launch 0: dg_build_contiguous_tile_table_kernel writes two tile tables into the workspace's 4 KiB header (counts on the device only);
//   launch 1: duo_p_256x256 over the 256-row tiles (two 128-row blocks of ONE group: no tile is walked twice);
//   launch 2: duo_sk_128x256 over the 128-row remainders (at most one per group) and padding blocks, EVERY tile cut along K -- there are
//             too few of them to fill the chip (C4: 4 x 16 tiles for 256 CUs) -- + dg_split_k_reduce_kernel.
// C4 (8 groups x ~512 rows, N 4096, K 7168): 16 x 16 = 256 tiles of 256 rows = exactly one round at the C2 rate, then 64 remainder
// tiles x 4 K pieces; against 2.25 rounds of 128-row tiles (whose L2 -> LDS traffic per flop is 1.5x) with a split tail.
// Returns 1 if the path does not apply (the caller continues with the ordinary selection), 0 = launched, >= 2 = error.
int launch_contiguous_tabled(const dg::GemmParams& base, void* stream) {
    if (base.gemm_type != dg::kContiguous || base.m_alignment != 128 || base.sk_workspace == nullptr || forced_config() != "auto")
        return 1;
    if (!fast_eligible(base) || base.sfa_sm != 1 || base.sfb_gran_n != 128 || base.head_lr != 0)
        return 1;
    const int nb = ceil_div(base.m, 128), n_tiles = ceil_div(base.n, 256);
    const size_t tile_bytes = 128 * 256 * sizeof(float);
    if (nb > 500 || static_cast<long>(nb) * n_tiles < num_cus() || base.k < 1024 || g_workspace_bytes < 4096 + 64 * tile_bytes)
        return 1;
    int32_t* header = static_cast<int32_t*>(base.sk_workspace);
    int32_t* big = header;                   // [0] count, [1 ..] first rows: at most nb / 2 entries
    int32_t* rem = header + 512;             // at most nb entries (nb <= 500)
    // up to 64 blocks (M <= 8192: C4 has 36) every workgroup derives the tile list itself (GemmParams::table_mode): no table kernel and no
    // kernel boundary in front of the GEMM (the builder cost C4 6.2 us of 141.5)
    const bool in_kernel = nb <= 64 && !env_knobs().table_kernel;
    if (!in_kernel) {
        hipLaunchKernelGGL(dg::dg_build_contiguous_tile_table_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                           base.layout, base.m, big, rem);
        DG_HIP_CHECK(hipGetLastError());
    }
    const size_t elem = 2;
    auto common = [&](dg::GemmParams& q, int bm) {
        q.num_m_tiles = ceil_div(q.m, bm);      // upper bound (grouping, grid); the table holds the real count
        q.num_n_tiles = n_tiles;
        q.group_m = q.num_m_tiles >= 2 ? 2 : 1;  // two M tiles (usually one group: they share B) per L2 group: C4 143.4 -> 141.5 us against 4
        q.d_vec_ok = aligned16(q.d) && (q.d_sm * elem) % 16 == 0;
        q.d_nt = output_streams_past_l2(q);
        q.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    };
    // ONE launch for both walks (dg_fp8_gemm_duo_tab_fused_kernel) when the tile list is derived in the kernel; DG_TAB_UNFUSED=1 keeps
    // the two launches of round 3 (A/B)
    const bool fused = in_kernel && !env_knobs().tab_unfused && !env_knobs().sk_exchange;
    dg::GemmParams q = base;
    {   // the 256-row tiles
        q.tile_table = in_kernel ? nullptr : big;
        q.table_mode = in_kernel ? 1 : 0;
        q.sk_workspace = nullptr; q.sk_first_tile = 0; q.sk_tiles = 0; q.sk_factor = 1; q.sk_capacity = 0;
        common(q, 256);
        const long items = static_cast<long>(nb / 2) * n_tiles;
        const long grid = std::min<long>(items, num_cus());
        if (grid > 0 && !fused)
            hipLaunchKernelGGL((dg::dg_fp8_gemm_duo_kernel<256, 256, 2, 4, true>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                               static_cast<hipStream_t>(stream), q);
        DG_HIP_CHECK(hipGetLastError());
    }
    {   // the remainders, all K-split
        dg::GemmParams r = base;
        r.tile_table = in_kernel ? nullptr : rem;
        r.table_mode = in_kernel ? 2 : 0;
        common(r, 128);
        r.sk_capacity = static_cast<int>(std::min<size_t>((g_workspace_bytes - 4096) / tile_bytes, 1u << 20));
        // pieces: at most 8 and one per K block, and only where a split pays at all (split_k_pays); how many of them a launch really
        // uses is decided on the device from the table's tile count: one round of pieces over the slots (table_pieces)
        long pieces = std::min<long>(8, base.k / 128);
        if (!split_k_pays(2, base.k / 128))
            pieces = 1;
        // DG_SK_EXCHANGE=1 (experiment, round 3): cut in TWO and let the second piece add the first one's partial itself
        // (GemmParams::sk_exchange) -- no reduction kernel, half the partial traffic.  Measured on C4: with agent-scope release / acquire
        // (a writeback and an invalidate of the whole L2 per workgroup) 151 us against 142 with the reduction kernel; with written-through
        // stores and cache-bypassing loads 141-143 against 143.5: a 1 % gain does not pay for a spin-wait in the product path.
        static std::atomic<unsigned> exchange_epoch{0};
        const bool exchange = in_kernel && pieces >= 2 && static_cast<long>(nb) * n_tiles <= 1024 && env_knobs().sk_exchange;
        if (exchange) {
            pieces = 2;
            r.sk_exchange = 0x7fd00000u | (exchange_epoch.fetch_add(1, std::memory_order_relaxed) & 0xfffffu);
        }
        r.sk_factor = static_cast<int>(std::max<long>(pieces, 1));
        r.sk_first_tile = 0;
        r.sk_tiles = num_cus();              // (table launch: the slot count; the kernels read the tile count from the table)
        const long max_items = static_cast<long>(nb) * n_tiles * r.sk_factor;
        const long grid = std::min<long>(max_items, num_cus());
        if (fused)          // every workgroup slot: both walks are persistent (stride = the grid) and end on their own
            hipLaunchKernelGGL((dg::dg_fp8_gemm_duo_tab_fused_kernel<256, 128, 256, 2, 4>), dim3(static_cast<unsigned>(num_cus())), dim3(512), 0,
                               static_cast<hipStream_t>(stream), q, r);
        else
            hipLaunchKernelGGL((dg::dg_fp8_gemm_duo_kernel<128, 256, 2, 4, true, false, true, false, false, true>), dim3(static_cast<unsigned>(grid)),
                               dim3(512), 0, static_cast<hipStream_t>(stream), r);
        DG_HIP_CHECK(hipGetLastError());
        if (r.sk_factor >= 2 && r.sk_exchange == 0) {
            // grid: an upper bound on the remainder tiles that can be split at all (capacity / 2 pieces) x 4 subtile rows; surplus
            // workgroups return at once
            const long max_split_tiles = std::min<long>(static_cast<long>(nb) * n_tiles, r.sk_capacity / 2);
            hipLaunchKernelGGL((dg::dg_split_k_reduce_kernel<128, 256, 2, 4, false>), dim3(static_cast<unsigned>(max_split_tiles * 4)), dim3(512), 0,
                               static_cast<hipStream_t>(stream), r);
            DG_HIP_CHECK(hipGetLastError());
        }
        if (env_knobs().print_configs)
            fprintf(stderr, "[deepgemm_amd] contiguous m=%d n=%d k=%d groups=%d -> duo_tab_256x256 + duo_sk_128x256 (pieces <= %d)\n", base.m, base.n,
                    base.k, base.num_groups, r.sk_factor);
    }
    g_last_config = "duo_tab_256x256";
    return 0;
}

// Launch of a packed-UE8M0 problem (GemmParams filled by the entry point, scale pointers = packed words).  Kernel choice:
// the 4-wave in-place-accumulating quad kernels -- 256 x 256 tiles for dense problems of whole K quads that fill the chip and
// for contiguous layouts with several rounds of two-pass tiles, 128 x 256 tiles otherwise; the 8-wave forms only by name.
// Automatic choice among the packed-UE8M0 kernels (forced names are resolved by the caller).
const E8Config* e8_config_by_name(const char* name) {
    for (const E8Config& c : kE8Configs)
        if (std::strcmp(c.name, name) == 0)
            return &c;
    return nullptr;
}

// Decode batches (M <= 32), dense, packed scales: the rule of the FP32-scale skinny kernels (select_config).  nullptr = not this class.
const char* e8_skinny_pick(const dg::GemmParams& p, bool g32) {
    if (p.gemm_type != dg::kNormal || p.head_lr != 0 || p.n % 16 != 0 || p.k % 128 != 0 || p.sfa_sm != 1 || p.sfb_sn != 1 || !fast_eligible(p))
        return nullptr;
    const int num_kb = p.k / 128;
    if (p.m <= 16 && num_kb >= 16)
        return g32 ? "e8_skinny_g32_16" : "e8_skinny_16";
    // (narrow layers with K >= 7168 and the caller's workspace: the 64 x 32 stream tile cut along K -- the FP32-scale rule of select_config)
    // (from 32 K blocks, as the FP32-scale rule: 17 .. 32 x 4096 x 4096 at granularity 32 8.2-9.1 us against 9.9-10.1 on the K-split tile -- m17_32_skinny_vs_ks.log)
    if (p.m > 16 && p.m <= 32 && num_kb >= 32 && num_kb <= 64 && p.n <= 4608 &&
        !(p.sk_workspace != nullptr && num_kb >= 56 && ceil_div(p.n, 32) <= 48 &&
          4096 + 32768 + static_cast<size_t>(ceil_div(p.n, 32)) * 8 * 64 * 32 * sizeof(float) <= g_workspace_bytes))
        return g32 ? "e8_skinny_g32_32" : "e8_skinny_32";
    return nullptr;
}

// Packed-scale dense problems the stream tile is cut along K for (the FP32-scale rules of select_config: stream_ks_64x128 for 129 .. 256 rows with
// 64 .. CUs / 2 tiles, stream_ks_64x32 where the 64 x 32 tiles fill at most half the chip; K >= 4096, the caller's workspace).  nullptr = not this class.
const char* e8_stream_ks_pick(const dg::GemmParams& p, bool g32) {
    if (p.gemm_type != dg::kNormal || p.head_lr != 0 || p.sk_workspace == nullptr || p.k < 4096 || p.k % 128 != 0 || p.sfa_sm != 1 || p.sfb_sn != 1 ||
        !fast_eligible(p) || p.m > 256)
        return nullptr;
    const long tiles128 = static_cast<long>(ceil_div(p.m, 64)) * ceil_div(p.n, 128), tiles32 = static_cast<long>(ceil_div(p.m, 64)) * ceil_div(p.n, 32);
    const size_t fixed = 4096 + 32768;
    // (65 .. 128 rows on wide layers: from 96 tiles with K >= 7168 -- 128 x 7168 x 16384 55.1 -> 42.5 us, 128 x 7168 x 8192 31.7 -> 26.3, 128 x 6144 x 7168
    //  28.4 -> 22.9 -- and 64 .. 95 tiles from K = 12288: 128 x 4096 x 16384 29.7 -> 27.5; profiles/r06_probe/m128_long_k_ab.log)
    const bool rows_129_256 = p.m > 128 && (tiles128 >= 64 || (tiles128 > 32 && p.k >= 10240));
    const bool rows_65_128 = p.m > 64 && p.m <= 128 && ((tiles128 > 64 && p.k >= 7168) || (tiles128 == 64 && p.k >= 12288));
    if ((rows_129_256 || rows_65_128) && tiles128 * 2 <= num_cus() &&
        fixed + static_cast<size_t>(tiles128) * 8 * 64 * 128 * sizeof(float) <= g_workspace_bytes)
        return g32 ? "e8_stream_ks_g32_64x128" : "e8_stream_ks_64x128";
    if (p.m > 16 && tiles128 < 128 && tiles32 * 2 <= num_cus() && fixed + static_cast<size_t>(tiles32) * 8 * 64 * 32 * sizeof(float) <= g_workspace_bytes)
        return g32 ? "e8_stream_ks_g32_64x32" : "e8_stream_ks_64x32";
    return nullptr;
}

const E8Config* select_e8_config(const dg::GemmParams& p, int expected_m) {
    const E8Config* cfg = nullptr;
    if (const char* skinny = e8_skinny_pick(p, false))
        return e8_config_by_name(skinny);
    if (const char* ks = e8_stream_ks_pick(p, false))
        return e8_config_by_name(ks);
    {
        const int m_hint = expected_m > 0 ? expected_m : p.m;
        const long groups = p.gemm_type == dg::kMasked ? p.num_groups : 1;
        const long tiles256 = groups * ceil_div(m_hint, 256) * ceil_div(p.n, 256);
        bool big = p.k % 512 == 0 && m_hint > 128 && 2 * tiles256 >= num_cus();
        if (p.gemm_type == dg::kContiguous)         // two-pass tiles (halves of two groups): only with rounds to average over
            big = big && p.m_alignment == 128 && tiles256 >= 4L * num_cus();
        if (p.gemm_type == dg::kContiguousPsum)
            big = false;                            // the psum walk is written for tiles that divide the alignment
        cfg = big ? &kE8Configs[0] : &kE8Configs[1];
        // decode-sized M with a round of 64 x 128 tiles to fill the chip (the rule of the FP32-scale stream kernel): weights stream
        // once, five K blocks in flight per CU; non-temporal weight policy when the launch's weights exceed the Infinity Cache
        const long tiles128 = groups * ceil_div(m_hint, 64) * ceil_div(p.n, 128);
        if ((p.gemm_type == dg::kMasked || p.gemm_type == dg::kNormal) && p.sfa_sm == 1 && p.sfb_sn == 1) {
            // the tile rules of the FP32-scale stream kernels (select_config): 64 x 128 when a round of them covers the chip, 64 x 32 below
            const E8Config* pick = nullptr;
            if (m_hint <= 64)
                pick = tiles128 >= 96 ? &kE8Configs[3] : &kE8Configs[5];
            else if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal && p.k >= 4096 ? 128 : 96))
                pick = &kE8Configs[5];          // (the FP32-scale rule; m = 128, 7168 x 16384, 112 tiles: 63.5 us on 64 x 128 tiles, 56.8 here)
            else if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal ? 2L * num_cus() + 1 : 256))
                pick = &kE8Configs[3];          // (dense: up to one resident round of two tiles per CU -- m = 128, 24576 x 1536: 23.5 -> 18.1 us, 32768 x 512: 13.1 -> 9.8)
            if (pick == &kE8Configs[3])         // two workgroups per CU on a 3-stage ring, non-temporal weights from kNonTemporalWeightBytes per launch (select_config)
                pick = e8_config_by_name(static_cast<double>(groups) * p.n * p.k >= kNonTemporalWeightBytes ? "e8_stream_nt2_64x128" : "e8_stream2_64x128");
            // dense: the 64 x 32 tile with loader waves (the FP32-scale rule: stream_l8_64x32)
            if (pick == &kE8Configs[5] && p.gemm_type == dg::kNormal)
                if (const E8Config* l8 = e8_config_by_name("e8_stream_l8_64x32"))
                    pick = l8;
            if (pick != nullptr)
                cfg = pick;
        }
    }
    return cfg;
}

// Packed scales on the contiguous layout at the M alignment of 128 (round 5): the group-relative tiling of launch_contiguous_tabled for the
// hardware-scaled kernels -- launch 1: e8_quad_256x256 over the 256-row tiles of the in-kernel tile list (two 128-row blocks of ONE group: no
// tile is walked twice), launch 2: e8_quad_128x256 over the remainders (at most one per group) and padding blocks.  No K split (the quad
// kernels accumulate in AGPRs and have no partial-tile form), so no workspace.  Against 128-row tiles everywhere: C4 with packed scales
// (8 x ~512 rows, N 4096, K 7168) 576 tiles = 2.25 rounds -> 256 big tiles + 80 remainder tiles.
bool e8_contiguous_tabled(const dg::GemmParams& p, int gran_k = 128) {
    // (granularity 32: one word per K block -- no whole-quad condition)
    if (gran_k == 32 && p.k % 128 != 0)
        return false;
    // (K >= 4096: with a short K loop the second launch costs what the taller tiles save -- profiles/r05_probe/packed_contiguous_group_relative_tiles_ab.jsonl:
    //  8 x ~512 rows, N 4096, K 7168 202.9 -> 153.2 us; K 2048: 78.6 -> 82.3 and 84.9 -> 83.9)
    if (p.gemm_type != dg::kContiguous || p.m_alignment != 128 || (gran_k != 32 && p.k % 512 != 0) || p.k < 4096 || !fast_eligible(p))
        return false;
    const int nb = ceil_div(p.m, 128);
    return nb <= 64 && static_cast<long>(nb) * ceil_div(p.n, 256) >= num_cus();
}

int launch_e8_contiguous_tabled(const dg::GemmParams& base, void* stream, int gran_k = 128) {
    const int nb = ceil_div(base.m, 128), n_tiles = ceil_div(base.n, 256);
    // With the caller's workspace the remainder walk is cut along K (TABSK: one work item per (tile, piece), FP32 partial tiles, a second kernel
    // sums them): 64 .. 96 remainder tiles of C4 are a quarter of a round, each streaming its group's whole weight panel -- 58 us for a ninth of
    // the work.  Pieces: whole K quads, at most 8; how many a launch really uses is decided on the device from the tile count (table_pieces).
    const size_t slab_bytes = 128 * 256 * sizeof(float);
    // (granularity 32: whole remainder tiles -- the K-split form cuts at K quads of the gran-128 words)
    const bool split = gran_k != 32 && base.sk_workspace != nullptr && g_workspace_bytes >= 4096 + 64 * slab_bytes && !env_knobs().e8_tab_unsplit;
    for (int mode = 1; mode <= 2; ++mode) {
        dg::GemmParams q = base;
        const int bm = mode == 1 ? 256 : 128;
        q.tile_table = nullptr; q.table_mode = mode;
        q.num_m_tiles = ceil_div(q.m, bm);          // upper bound (grouping, grid); the in-kernel list holds the real count
        q.num_n_tiles = n_tiles;
        q.group_m = q.num_m_tiles >= 2 ? 2 : 1;
        q.d_vec_ok = aligned16(q.d) && (q.d_sm * 2) % 16 == 0;
        q.d_nt = output_streams_past_l2(q);
        q.dbg = g_debug_buffer.load(std::memory_order_relaxed);
        q.sk_first_tile = 0; q.sk_tiles = 0; q.sk_factor = 1; q.sk_capacity = 0;
        if (mode == 1 || !split)
            q.sk_workspace = nullptr;
        const long items = static_cast<long>(mode == 1 ? nb / 2 : nb) * n_tiles;
        long grid = std::min<long>(items, num_cus());
        if (grid <= 0)
            continue;
        if (gran_k == 32) {
            if (mode == 1)
                hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                                   static_cast<hipStream_t>(stream), q);
            else
                hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                                   static_cast<hipStream_t>(stream), q);
        } else if (mode == 1) {
            hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), q);
        } else if (!split) {
            hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), q);
        } else {
            q.sk_factor = static_cast<int>(std::min<long>(8, base.k / 512));
            q.sk_tiles = num_cus();                 // (table launch: the slot count; the kernels read the tile count from the tile list)
            q.sk_capacity = static_cast<int>(std::min<size_t>((g_workspace_bytes - 4096) / slab_bytes, 1u << 20));
            grid = std::min<long>(items * q.sk_factor, num_cus());
            hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), q);
            DG_HIP_CHECK(hipGetLastError());
            // grid: an upper bound on the tiles that can be split at all (capacity / 2 pieces) x 4 row quarters; surplus workgroups return at once
            const long max_split_tiles = std::min<long>(items, q.sk_capacity / 2);
            if (q.sk_factor >= 2 && max_split_tiles > 0)
                hipLaunchKernelGGL(dg::dg_e8_tab_reduce_kernel, dim3(static_cast<unsigned>(max_split_tiles * 4)), dim3(256), 0,
                                   static_cast<hipStream_t>(stream), q);
        }
        DG_HIP_CHECK(hipGetLastError());
    }
    g_last_config = gran_k == 32 ? "e8_quad_g32_tab_256x256" : "e8_quad_tab_256x256";
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] ue8m0 contiguous m=%d n=%d k=%d groups=%d -> e8_quad_256x256 + e8_quad_128x256 over the group-relative tile list\n",
                base.m, base.n, base.k, base.num_groups);
    return 0;
}

// The granularity-32 launch (round 6): K-major operands, k % 128 == 0; the two four-wave G32 forms by the tile rule of the gran-128 selection
// (256 x 256 when the problem fills the chip with them, 128 x 256 otherwise and for every grouped layout but the group-relative tiling).
const E8Config* select_e8_g32_config(const dg::GemmParams& p, int expected_m) {
    const int m_hint = expected_m > 0 ? expected_m : p.m;
    const long groups = p.gemm_type == dg::kMasked ? p.num_groups : 1;
    const long tiles256 = groups * ceil_div(m_hint, 256) * ceil_div(p.n, 256);
    bool big = m_hint > 128 && 2 * tiles256 >= num_cus();
    if (p.gemm_type == dg::kContiguous)
        big = big && p.m_alignment == 128 && tiles256 >= 4L * num_cus();
    if (p.gemm_type == dg::kContiguousPsum)
        big = false;
    if (const char* skinny = e8_skinny_pick(p, true))
        return e8_config_by_name(skinny);
    if (const char* ks = e8_stream_ks_pick(p, true))
        return e8_config_by_name(ks);
    // decode-sized M: the stream tiles, by the rule of the granularity-128 selection (select_e8_config)
    if ((p.gemm_type == dg::kMasked || p.gemm_type == dg::kNormal) && p.sfa_sm == 1 && p.sfb_sn == 1) {
        const long tiles128 = groups * ceil_div(m_hint, 64) * ceil_div(p.n, 128);
        const char* wide = static_cast<double>(groups) * p.n * p.k >= kNonTemporalWeightBytes ? "e8_stream_nt2_g32_64x128" : "e8_stream2_g32_64x128";
        // (dense: the 64 x 32 tile with four loader waves, as at granularity 128)
        const char* narrow = p.gemm_type == dg::kNormal ? "e8_stream_l8_g32_64x32" : "e8_stream_g32_64x32";
        if (m_hint <= 64)
            return e8_config_by_name(tiles128 >= 96 ? wide : narrow);
        if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal && p.k >= 4096 ? 128 : 96))
            return e8_config_by_name(narrow);
        if (m_hint <= 256 && tiles128 < (p.gemm_type == dg::kNormal ? 2L * num_cus() + 1 : 256))
            return e8_config_by_name(wide);
    }
    return e8_config_by_name(big ? "e8_quad_g32_256x256" : "e8_quad_g32_128x256");
}

// Under-filled dense launches of the hardware-scaled kernels (round 6: packed-scale dgrad shapes with a narrow N and a long K -- 4096 x 512 x 32768 is
// 32 tiles of 256 x 256, one K loop of 256 blocks on an eighth of the chip -- and narrow-layer weight gradients): the K axis is cut into `pieces`
// ranges of whole K quads that run as the groups of ONE launch of the K-grouped kernel, each writing an FP32 partial matrix into the caller's
// workspace; dg_sum_partials_kernel adds them in piece order and performs the operator's output step (the recipe-(1, 1, 128) split's scheme,
// launch_per_col_split).  Returns the number of pieces (0 = one ordinary launch; the model is at the end of the function).  workspace_bytes = 0:
// "as large as needed" (the host layer's query).
int e8_split_pieces(const dg::GemmParams& p, size_t workspace_bytes) {
    if (p.gemm_type != dg::kNormal || p.head_lr > 0 || p.m <= 128 || p.k % 512 != 0 || forced_config() != "auto" || !fast_eligible(p))
        return 0;
    if (p.sfa_sm != 1 || p.sfb_sn != 1)
        return 0;
    const long tiles = static_cast<long>(ceil_div(p.m, 256)) * ceil_div(p.n, 256), num_kb = p.k / 128;
    const size_t per_piece = static_cast<size_t>(p.m) * p.n * sizeof(float);
    long pieces = std::min<long>(std::min<long>(8, num_cus() / tiles), num_kb / 8);        // (at least two K quads per piece)
    const long fit = workspace_bytes > 0 ? (workspace_bytes > 4096 ? static_cast<long>((workspace_bytes - 4096) / per_piece) : 0) : 8;
    pieces = std::min<long>(pieces, fit);
    if (pieces < 2 || num_kb < 24)
        return 0;
    // calibrated on profiles/r06_probe/packed_dense_ksplit_ab.log: one launch = the 128-row kernel at ~0.75 us per K block while its tiles fit the chip
    // (576 x 4096 x 7168: 54 us), 1.35 per round of 256-row tiles otherwise; the split's pieces run 256-row tiles at 1.35 us per K block and the
    // summing kernel moves (pieces + 2) x m x n x 4 bytes at ~3.7 TB/s (4096 x 512 x 32768: 255 -> 105 us, 1024 x 1024 x 16384: 96 -> 59; at 56 K
    // blocks the split loses 5 us and is not taken)
    const long tiles128 = static_cast<long>(ceil_div(p.m, 128)) * ceil_div(p.n, 256);
    double t_one = tiles128 <= num_cus() ? 12.0 + 0.75 * num_kb : 12.0 + 1.35 * num_kb * ceil_div(static_cast<int>(tiles), num_cus());
    // up to 256 rows the unsplit call runs the stream tiles (select_e8_config), not the 128-row kernel: the model of select_config (5 us + 0.27 us per
    // K block on 64 x 32 tiles, 0.66 on 64 x 128) -- packed 192 x 2112 x 7168 was cut for a modelled 42 us where the stream tile runs ~17
    // (profiles/r06_probe/e8_split_small_m_ab.log)
    if (p.m <= 256 && !env_knobs().e8_split_quad_model_only)
        t_one = std::min(t_one, 5.0 + num_kb * (static_cast<long>(ceil_div(p.m, 64)) * ceil_div(p.n, 128) < 128 ? 0.27 : 0.66));
    const double t_split = 27.0 + 1.35 * ((num_kb + pieces - 1) / pieces) + static_cast<double>(pieces + 2) * per_piece / 3.7e6;
    return t_split < 0.85 * t_one ? static_cast<int>(pieces) : 0;
}

int launch_e8_split(const dg::GemmParams& dense, int pieces, void* stream, int gran_k) {
    dg::GemmParams p = dense;
    float* parts = reinterpret_cast<float*>(static_cast<uint8_t*>(dense.sk_workspace) + 4096);
    p.d = parts; p.d_sm = dense.n; p.d_sg = static_cast<int64_t>(dense.m) * dense.n; p.d_dtype = DG_FP32; p.accumulate = 0;
    p.gemm_type = dg::kKGrouped; p.num_groups = pieces; p.kg_blocks = 0; p.kg_psum = 0; p.m_alignment = 128; p.layout = nullptr;
    p.b_sg = 0; p.sfb_sg = 0; p.sfb_gran_n = 1;
    p.sk_workspace = nullptr; p.sk_first_tile = 0; p.sk_tiles = 0; p.sk_factor = 1;
    const int num_kq = dense.k / 512;
    for (int i = 0; i <= pieces; ++i)
        p.kg_prefix[i] = 512 * static_cast<int>(static_cast<long>(i) * num_kq / pieces);
    p.num_m_tiles = ceil_div(p.m, 256);
    p.num_n_tiles = ceil_div(p.n, 256);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    p.d_vec_ok = dense.n % 4 == 0;
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * pieces;
    g_last_config = gran_k == 32 ? "e8_quad_ks_g32_256x256" : "e8_quad_ks_256x256";
    if (gran_k == 32)
        hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, false, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    const size_t elem = dense.d_dtype == DG_BF16 ? 2 : 4;
    const int vec_ok = dense.n % 4 == 0 && (dense.d_dtype == DG_BF16 || (aligned16(dense.d) && (dense.d_sm * elem) % 16 == 0));
    const long quads = static_cast<long>(dense.m) * ((dense.n + 3) / 4);
    const long blocks = std::min<long>((quads + 255) / 256, static_cast<long>(num_cus()) * 8);
    hipLaunchKernelGGL(dg::dg_sum_partials_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       parts, pieces, static_cast<int64_t>(dense.m) * dense.n, dense.d, dense.m, dense.n, dense.d_sm, dense.d_dtype,
                       dense.accumulate, vec_ok);
    DG_HIP_CHECK(hipGetLastError());
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] ue8m0 dense m=%d n=%d k=%d -> %s pieces=%d grid=%ld\n", dense.m, dense.n, dense.k, g_last_config.c_str(), pieces, grid);
    return 0;
}

int launch_e8(dg::GemmParams& p, int expected_m, void* stream, int gran_k = 128) {
    const bool k_tail = p.k % 128 != 0;
    // (m <= 256 inside the rule of the stream tiles cut along K in one launch -- e8_stream_ks_pick -- stays with them: 256 x 576 x 16384)
    if (p.sk_workspace != nullptr && p.gemm_type == dg::kNormal && !(forced_config() == "auto" && e8_stream_ks_pick(p, gran_k == 32) != nullptr))
        if (const int pieces = e8_split_pieces(p, g_workspace_bytes); pieces >= 2)
            return launch_e8_split(p, pieces, stream, gran_k);
    const bool mn_form = gran_k != 32 && e8_mn_eligible(p);           // an MN-major operand read in place
    if (gran_k == 32 && (k_tail || !fast_eligible(p))) {
        g_last_error = "packed-UE8M0 GEMMs with scale granularity 32 need K-major, 16-byte aligned FP8 operands and k % 128 == 0";
        return 3;
    }
    if (!mn_form && forced_config() == "auto" && e8_contiguous_tabled(p, gran_k))
        return launch_e8_contiguous_tabled(p, stream, gran_k);
    if (!mn_form && (!fast_eligible(p, !k_tail) || (k_tail && p.gemm_type != dg::kNormal))) {
        g_last_error = "packed-UE8M0 GEMMs need K-major, 16-byte aligned FP8 operands and k % 128 == 0 (dense: or k % 16 == 0 and k > 128)";
        return 3;
    }
    const bool grouped = p.gemm_type != dg::kNormal;
    const std::string forced = forced_config();
    const E8Config* cfg = nullptr;
    for (const E8Config& c : kE8Configs)
        if (forced == c.name)
            cfg = &c;
    if (k_tail && !mn_form) {
        for (const E8Config& c : kE8Configs)
            if (std::strcmp(c.name, "e8_quad_kt_128x256") == 0) {
                if (cfg != nullptr && cfg != &c) {
                    g_last_error = std::string("forced config '") + cfg->name + "' needs k % 128 == 0";
                    return 3;
                }
                cfg = &c;
            }
    } else if (cfg != nullptr && std::strcmp(cfg->name, "e8_quad_kt_128x256") == 0) {
        cfg = nullptr;                              // (the tail form is only for tails; a forced name falls back to the selection)
    }
    if (mn_form) {                                  // MN-major operand(s): one kernel reads this combination (a forced name of another one is refused)
        const char* want = e8_mn_config_name(p);
        for (const E8Config& c : kE8Configs)
            if (std::strcmp(c.name, want) == 0) {
                if (cfg != nullptr && cfg != &c) {
                    g_last_error = std::string("forced config '") + cfg->name + "' does not read this operand majorness (" + want + " does)";
                    return 3;
                }
                cfg = &c;
            }
    } else if (cfg != nullptr && std::strncmp(cfg->name, "e8_duo_", 7) == 0 && std::strstr(cfg->name, "mn_") != nullptr) {
        g_last_error = std::string("config '") + cfg->name + "' reads MN-major operands";
        return 3;
    }
    if (gran_k == 32 && (cfg == nullptr || !cfg->g32))
        cfg = select_e8_g32_config(p, expected_m);          // (a forced name of a gran-128 kernel does not apply to these entries)
    if (cfg == nullptr)
        cfg = select_e8_config(p, expected_m);
    if (cfg->g32 != (gran_k == 32)) {
        g_last_error = std::string("config '") + cfg->name + "' reads scale words of granularity " + (cfg->g32 ? "32" : "128");
        return 3;
    }
    if (cfg->stream && (p.gemm_type == dg::kContiguous || p.gemm_type == dg::kContiguousPsum)) {
        g_last_error = std::string("config '") + cfg->name + "' does not implement the contiguous layouts";
        return 3;
    }
    if (cfg->whole_quads && p.k % 512 != 0) {
        g_last_error = std::string("config '") + cfg->name + "' needs k % 512 == 0 (whole packed scale words)";
        return 3;
    }
    if (grouped && (!cfg->grouped_ok || (std::strncmp(cfg->name, "e8_duo_", 7) == 0 && p.gemm_type != dg::kContiguous))) {
        g_last_error = std::string("config '") + cfg->name + "' implements the dense form only" +
                       (cfg->grouped_ok ? " (and the contiguous layout without psum)" : "");
        return 3;
    }
    if ((p.gemm_type == dg::kContiguous || p.gemm_type == dg::kContiguousPsum) && p.m_alignment % cfg->bm != 0 &&
        !(p.gemm_type == dg::kContiguous && cfg->bm == 2 * p.m_alignment)) {
        g_last_error = std::string("config '") + cfg->name + "' does not divide the contiguous-layout M alignment";
        return 3;
    }
    const bool skinny = std::strncmp(cfg->name, "e8_skinny", 9) == 0;
    if (skinny && (p.m > cfg->bm || p.gemm_type != dg::kNormal || p.head_lr != 0 || k_tail || mn_form || p.sfa_sm != 1 || p.sfb_sn != 1)) {
        g_last_error = std::string("config '") + cfg->name + "' implements dense K-major problems with m <= its row count and whole K blocks";
        return 3;
    }
    g_last_config = cfg->name;
    p.num_m_tiles = ceil_div(p.m, cfg->bm);
    p.num_n_tiles = ceil_div(p.n, cfg->bn);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    const size_t elem = p.d_dtype == DG_BF16 ? 2 : 4;
    p.d_vec_ok = aligned16(p.d) && (p.d_sm * elem) % 16 == 0 && (p.d_sg * elem) % 16 == 0;
    p.d_nt = output_streams_past_l2(p);
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    if (skinny) {                       // one workgroup per 16 output columns (not a tile walk)
        p.skinny_cols = 0;
        hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(p.num_n_tiles)), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), p);
        DG_HIP_CHECK(hipGetLastError());
        if (env_knobs().print_configs)
            fprintf(stderr, "[deepgemm_amd] ue8m0 m=%d n=%d k=%d -> %s grid=%d\n", p.m, p.n, p.k, cfg->name, p.num_n_tiles);
        return 0;
    }
    long total = static_cast<long>(p.num_m_tiles) * p.num_n_tiles;
    if (std::strncmp(cfg->name, "e8_stream_ks_", 13) == 0) {
        // K pieces of the stream tile (launch_gemm's stream_ks branch): as many as keep tiles x pieces within one resident round, at most 8, whole K quads
        if (p.gemm_type != dg::kNormal || p.head_lr != 0 || k_tail || mn_form || p.sfa_sm != 1 || p.sfb_sn != 1 || total > 1024) {
            g_last_error = std::string("config '") + cfg->name + "' implements dense K-major problems with whole K blocks and at most 1024 tiles";
            return 3;
        }
        const long slots = num_cus();
        long pieces = std::min<long>(std::min<long>(env_knobs().ks_max_pieces, total > 0 ? slots / total : 0), p.k / 128 / 4);
        const size_t need = 4096 + 32768 + static_cast<size_t>(total) * 8 * cfg->bm * cfg->bn * sizeof(float);
        if (pieces < 2 || p.sk_workspace == nullptr || need > g_workspace_bytes)
            pieces = 1;                             // whole tiles (no workspace, too many tiles)
        p.sk_factor = static_cast<int>(pieces);
        p.sk_exchange = 0x7fc00000u | (g_stream_ks_epoch.fetch_add(1, std::memory_order_relaxed) & 0xfffffu) | 0x100000u;
        const long items = total * pieces;
        hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(std::min<long>(items, slots))), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), p);
        DG_HIP_CHECK(hipGetLastError());
        if (env_knobs().print_configs)
            fprintf(stderr, "[deepgemm_amd] ue8m0 m=%d n=%d k=%d -> %s pieces=%ld items=%ld\n", p.m, p.n, p.k, cfg->name, pieces, items);
        return 0;
    }
    if (p.gemm_type == dg::kMasked)
        total *= p.num_groups;
    const long slots = static_cast<long>(num_cus()) * cfg->per_cu;
    const long grid = total < slots ? total : slots;                  // every kernel walks tile_id += gridDim.x
    if (grid <= 0)
        return 0;
    hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(grid)), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] ue8m0 type=%d m=%d n=%d k=%d groups=%d -> %s grid=%ld\n", p.gemm_type, p.m, p.n, p.k,
                p.num_groups, cfg->name, grid);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// BF16 GEMMs (bf16_gemm_kernels.hpp).  Selection from the shape and the CU count only:
//   dense m <= 64 / masked expected_m <= 64: the 64 x 32 weight-streaming tile; a dense problem whose tiles fill at most half of the CUs is
//     cut along K into pieces (FP32 partials in the caller's workspace + dg_bf16_split_k_sum_kernel) when the caller passes a workspace;
//   everything else: the 256 x 256 tile, except the psum layout and contiguous alignments that 256 neither divides nor halves (128 x 256,
//     then the 64-row tile).
// ---------------------------------------------------------------------------------------------------------------------
struct Bf16Config { const char* name; KernelFn fn; int bm, bn, threads; int per_cu; bool ksplit; };
const Bf16Config kBf16Configs[] = {
    {"bf16_256x256", dg::dg_bf16_gemm_kernel<256, 256, 2, 4, 2>, 256, 256, 512, 1, false},
    {"bf16_128x256", dg::dg_bf16_gemm_kernel<128, 256, 2, 4, 3>, 128, 256, 512, 1, false},
    {"bf16_stream_64x32", dg::dg_bf16_gemm_kernel<64, 32, 4, 1, 8>, 64, 32, 256, 1, false},
    {"bf16_stream_ks_64x32", dg::dg_bf16_gemm_kernel<64, 32, 4, 1, 8, true>, 64, 32, 256, 1, true},
};
constexpr int kBf16SmallM = 64;

const Bf16Config* bf16_config_by_name(const std::string& name) {
    for (const Bf16Config& c : kBf16Configs)
        if (name == c.name)
            return &c;
    return nullptr;
}

// K pieces of the dense small-M tile: as many as keep tiles x pieces within one round over the CUs, at most 8, at least 8 K blocks each;
// 1 = no split (the tiles fill more than half the chip, or the workspace cannot hold the FP32 partials)
int bf16_split_pieces(const dg::GemmParams& p, size_t workspace_bytes) {
    if (p.gemm_type != dg::kNormal || p.m > kBf16SmallM)
        return 1;
    const long tiles = static_cast<long>(ceil_div(p.m, 64)) * ceil_div(p.n, 32);
    long pieces = std::min<long>(std::min<long>(8, num_cus() / std::max<long>(tiles, 1)), ceil_div(p.k, 64) / 8);
    if (pieces < 2 || static_cast<size_t>(pieces) * p.m * p.n * sizeof(float) > workspace_bytes)
        return 1;
    return static_cast<int>(pieces);
}

// The automatic choice (forced names are resolved by the caller); nullptr = no BF16 kernel takes this contiguous alignment.
const Bf16Config* select_bf16_config(const dg::GemmParams& p, int expected_m, size_t workspace_bytes) {
    switch (p.gemm_type) {
        case dg::kNormal:
            if (p.m <= kBf16SmallM)
                return bf16_config_by_name(bf16_split_pieces(p, workspace_bytes) >= 2 ? "bf16_stream_ks_64x32" : "bf16_stream_64x32");
            return bf16_config_by_name("bf16_256x256");
        case dg::kMasked:
            return bf16_config_by_name((expected_m > 0 ? expected_m : p.m) <= kBf16SmallM ? "bf16_stream_64x32" : "bf16_256x256");
        case dg::kContiguous:
            if (p.m_alignment % 256 == 0 || p.m_alignment == 128)
                return bf16_config_by_name("bf16_256x256");       // (alignment 128: tiles of two halves, walked twice where two groups meet)
            [[fallthrough]];
        default:                                                  // kContiguousPsum: a tile must not straddle two groups
            if (p.m_alignment % 128 == 0)
                return bf16_config_by_name("bf16_128x256");
            return p.m_alignment % 64 == 0 ? bf16_config_by_name("bf16_stream_64x32") : nullptr;
    }
}

int launch_bf16(dg::GemmParams& p, int expected_m, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string forced = forced_bf16_config();
    const Bf16Config* cfg = forced == "auto" ? select_bf16_config(p, expected_m, workspace != nullptr ? workspace_bytes : 0)
                                             : bf16_config_by_name(forced);
    if (cfg == nullptr) {
        g_last_error = forced == "auto" ? "no BF16 kernel configuration takes a contiguous-layout M alignment that is not a multiple of 64"
                                        : "unknown BF16 kernel configuration '" + forced + "'";
        return 3;
    }
    if (p.gemm_type == dg::kContiguous || p.gemm_type == dg::kContiguousPsum) {
        const bool divides = p.m_alignment % cfg->bm == 0;
        const bool halves = p.gemm_type == dg::kContiguous && cfg->bm == 2 * p.m_alignment;
        if (!divides && !halves) {
            g_last_error = std::string("config '") + cfg->name + "' does not divide the contiguous-layout M alignment";
            return 3;
        }
    }
    if (cfg->ksplit && p.gemm_type != dg::kNormal) {
        g_last_error = std::string("config '") + cfg->name + "' implements dense problems only";
        return 3;
    }
    // K pieces: the automatic rule's, or four (at most one per K block, at least two) for the form forced by name
    const int pieces = !cfg->ksplit ? 1 : forced == "auto" ? bf16_split_pieces(p, workspace_bytes) : std::max(2, std::min(4, ceil_div(p.k, 64)));
    if (cfg->ksplit && (workspace == nullptr || static_cast<size_t>(pieces) * p.m * p.n * sizeof(float) > workspace_bytes)) {
        g_last_error = std::string("config '") + cfg->name + "' needs a workspace of pieces x m x n FP32 values";
        return 3;
    }
    g_last_config = cfg->name;
    p.num_m_tiles = ceil_div(p.m, cfg->bm);
    p.num_n_tiles = ceil_div(p.n, cfg->bn);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    const size_t elem = p.d_dtype == DG_BF16 ? 2 : 4;
    p.d_vec_ok = aligned16(p.d) && (p.d_sm * elem) % 16 == 0 && (p.d_sg * elem) % 16 == 0;
    p.d_nt = output_streams_past_l2(p);
    const long total = static_cast<long>(p.num_m_tiles) * p.num_n_tiles;
    long grid = total;
    if (p.gemm_type == dg::kMasked)
        grid = std::min<long>(total * p.num_groups, static_cast<long>(num_cus()) * cfg->per_cu);
    if (grid <= 0)
        return 0;
    if (grid > 0x7fffffffL)
        return fail(__FILE__, __LINE__, "grid too large");
    if (cfg->ksplit) {
        // the K pieces as work items writing FP32 partial tiles into the workspace ([pieces][m][n]), then the summing launch into D
        const int f = pieces;
        dg::GemmParams part = p;
        part.d = workspace;
        part.d_dtype = DG_FP32;
        part.accumulate = 0;
        part.d_sm = p.n;
        part.d_sg = static_cast<int64_t>(p.m) * p.n;
        part.d_vec_ok = p.n % 4 == 0;
        part.d_nt = 0;
        part.sk_factor = f;
        hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(total * f)), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), part);
        DG_HIP_CHECK(hipGetLastError());
        const long items = (static_cast<long>(p.m) * p.n) / (p.n % 4 == 0 ? 4 : 1);
        const unsigned sum_grid = static_cast<unsigned>(std::max<long>(1, std::min<long>((items + 255) / 256, 4L * num_cus())));
        hipLaunchKernelGGL(dg::dg_bf16_split_k_sum_kernel, dim3(sum_grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const float*>(workspace), f, p.m, p.n, p.d, static_cast<int64_t>(p.d_sm), p.d_dtype, p.accumulate);
        DG_HIP_CHECK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(cfg->fn, dim3(static_cast<unsigned>(grid)), dim3(cfg->threads), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] bf16 type=%d m=%d n=%d k=%d groups=%d -> %s grid=%ld\n", p.gemm_type, p.m, p.n, p.k, p.num_groups,
                cfg->name, grid);
    return 0;
}

// Operand rows of a BF16 launch: K-major, 16-byte aligned (row strides multiples of 8 elements), k a multiple of 8, and a tile's rows
// within reach of the LDS-DMA's 32-bit offsets.
bool bf16_operand_ok(const void* ptr, int64_t row_stride, int64_t group_stride = 0) {
    return aligned16(ptr) && row_stride % 8 == 0 && group_stride % 8 == 0 && row_stride * 2 * 256 < (1LL << 31);
}

}  // namespace

// ---- indexer MQA logits (mqa_logits_kernels.hpp) ----

namespace {

int mqa_head_index(int h) { return h == 8 ? 0 : h == 16 ? 1 : h == 32 ? 2 : h == 64 ? 3 : -1; }
int mqa_dim_index(int d) { return d == 32 ? 0 : d == 64 ? 1 : d == 128 ? 2 : -1; }

using MqaKernelFn = void (*)(const dg::mqa::MqaParams);

#define DG_MQA_DENSE_ROW(H) {dg::mqa::dg_mqa_logits_kernel<H, 32>, dg::mqa::dg_mqa_logits_kernel<H, 64>, dg::mqa::dg_mqa_logits_kernel<H, 128>}
const MqaKernelFn kMqaDense[4][3] = {DG_MQA_DENSE_ROW(8), DG_MQA_DENSE_ROW(16), DG_MQA_DENSE_ROW(32), DG_MQA_DENSE_ROW(64)};
#undef DG_MQA_DENSE_ROW

// paged kernels by [head index][dim index][log2 MT]; a group holds at least one token (MT * 16 >= H): none below MT = 2 at H = 32, 4 at 64
template <int H, int D, int MT>
constexpr MqaKernelFn mqa_paged_or_null() {
    if constexpr (MT * 16 >= H)
        return dg::mqa::dg_paged_mqa_logits_kernel<H, D, MT>;
    else
        return nullptr;
}
#define DG_MQA_PAGED_D(H, D) {mqa_paged_or_null<H, D, 1>(), mqa_paged_or_null<H, D, 2>(), mqa_paged_or_null<H, D, 4>(), mqa_paged_or_null<H, D, 8>()}
#define DG_MQA_PAGED_H(H) {DG_MQA_PAGED_D(H, 32), DG_MQA_PAGED_D(H, 64), DG_MQA_PAGED_D(H, 128)}
const MqaKernelFn kMqaPaged[4][3][4] = {DG_MQA_PAGED_H(8), DG_MQA_PAGED_H(16), DG_MQA_PAGED_H(32), DG_MQA_PAGED_H(64)};
#undef DG_MQA_PAGED_H
#undef DG_MQA_PAGED_D

bool mqa_dtypes_ok(int logits_dtype, int weights_dtype) {
    return (logits_dtype == DG_FP32 || logits_dtype == DG_BF16) && (weights_dtype == DG_FP32 || weights_dtype == DG_BF16) &&
           (weights_dtype == DG_FP32 || logits_dtype == DG_BF16);
}

}  // namespace

extern "C" {

int dg_fp8_mqa_logits(const void* q, const void* kv, const float* kv_sf, const void* weights, const int32_t* ks, const int32_t* ke,
                      void* logits, int seq_len, int seq_len_kv, int num_heads, int head_dim, int64_t weights_stride, int64_t logits_stride,
                      int max_seqlen_k, int logits_dtype, int weights_dtype, void* stream) {
    const int hi = mqa_head_index(num_heads), di = mqa_dim_index(head_dim);
    DG_CHECK(hi >= 0 && di >= 0);
    DG_CHECK(seq_len >= 0 && seq_len_kv >= 0 && max_seqlen_k >= 0);
    DG_CHECK(mqa_dtypes_ok(logits_dtype, weights_dtype));
    if (seq_len == 0 || seq_len_kv == 0)
        return 0;
    DG_CHECK(q != nullptr && kv != nullptr && kv_sf != nullptr && weights != nullptr && ks != nullptr && ke != nullptr && logits != nullptr);
    DG_CHECK(weights_stride >= num_heads && logits_stride >= (max_seqlen_k > 0 ? max_seqlen_k : seq_len_kv));
    dg::mqa::MqaParams p{};
    p.q = static_cast<const uint8_t*>(q); p.kv = static_cast<const uint8_t*>(kv); p.kv_sf = kv_sf;
    p.weights = weights; p.ks = ks; p.ke = ke; p.logits = logits;
    p.logits_stride = logits_stride; p.w_stride = weights_stride;
    p.seq_len = seq_len; p.seq_len_kv = seq_len_kv; p.max_seqlen_k = max_seqlen_k;
    p.logits_bf16 = logits_dtype == DG_BF16; p.weights_bf16 = weights_dtype == DG_BF16;
    // KV chunks of 256-column multiples, enough of them for ~2048 workgroups; the chunking never changes a value (each element is
    // computed by one lane with one fixed reduction)
    const int tokens_per_wg = 128 / num_heads * dg::mqa::kDenseWaves;
    const int q_groups = (seq_len + tokens_per_wg - 1) / tokens_per_wg;
    const int max_chunks = (seq_len_kv + 255) / 256;
    const int chunks = std::max(1, std::min(max_chunks, (2048 + q_groups - 1) / q_groups));
    p.kv_chunk = ((seq_len_kv + chunks - 1) / chunks + 255) / 256 * 256;
    const dim3 grid(q_groups, (seq_len_kv + p.kv_chunk - 1) / p.kv_chunk);
    DG_CHECK(grid.y <= 65535);
    hipLaunchKernelGGL(kMqaDense[hi][di], grid, dim3(dg::mqa::kDenseWaves * 64), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_clean_logits(const int32_t* ks, const int32_t* ke, void* logits, int seq_len, int seq_len_kv, int64_t logits_stride,
                    int logits_dtype, void* stream) {
    DG_CHECK(seq_len >= 0 && seq_len_kv >= 0);
    DG_CHECK(logits_dtype == DG_FP32 || logits_dtype == DG_BF16);
    if (seq_len == 0 || seq_len_kv == 0)
        return 0;
    DG_CHECK(ks != nullptr && ke != nullptr && logits != nullptr && logits_stride >= seq_len_kv);
    dg::mqa::MqaParams p{};
    p.ks = ks; p.ke = ke; p.logits = logits; p.logits_stride = logits_stride;
    p.seq_len = seq_len; p.seq_len_kv = seq_len_kv; p.logits_bf16 = logits_dtype == DG_BF16;
    // rows on x, column chunks on y (strided inside the kernel past 65535 chunks): no size limit beyond the int arguments
    const dim3 grid(seq_len, std::min((seq_len_kv + dg::mqa::kCleanCols - 1) / dg::mqa::kCleanCols, 65535));
    hipLaunchKernelGGL(dg::mqa::dg_mqa_clean_logits_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_paged_mqa_logits_metadata(const int32_t* context_lens, int32_t* schedule, int batch, int next_n, int block_kv, int num_sms,
                                 void* stream) {
    DG_CHECK(block_kv == 32 || block_kv == 64);
    DG_CHECK(batch >= 0 && next_n >= 1 && num_sms >= 1);
    DG_CHECK(schedule != nullptr && (batch == 0 || context_lens != nullptr));
    hipLaunchKernelGGL(dg::mqa::dg_paged_mqa_logits_metadata_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       context_lens, schedule, batch, next_n, num_sms);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_fp8_paged_mqa_logits(const void* q, const void* kv_cache, const void* weights, const int32_t* context_lens, const int32_t* block_table,
                            const int32_t* schedule, void* logits, int batch, int next_n, int num_heads, int head_dim, int block_kv,
                            int max_blocks, int64_t kv_block_stride, int64_t block_table_stride, int64_t weights_stride,
                            int64_t logits_stride, int max_context_len, int num_sms, int logits_dtype, int weights_dtype, void* stream) {
    const int hi = mqa_head_index(num_heads), di = mqa_dim_index(head_dim);
    DG_CHECK(hi >= 0 && di >= 0);
    DG_CHECK(block_kv == 32 || block_kv == 64);
    DG_CHECK(batch >= 0 && next_n >= 1 && max_blocks >= 0 && max_context_len >= 0 && num_sms >= 1);
    DG_CHECK(mqa_dtypes_ok(logits_dtype, weights_dtype));
    DG_CHECK(kv_block_stride % 4 == 0 && kv_block_stride >= static_cast<int64_t>(block_kv) * (head_dim + 4));
    if (batch == 0 || max_context_len == 0 || max_blocks == 0)
        return 0;
    DG_CHECK(q != nullptr && kv_cache != nullptr && weights != nullptr && context_lens != nullptr && block_table != nullptr &&
             schedule != nullptr && logits != nullptr);
    DG_CHECK(weights_stride >= num_heads && logits_stride >= max_context_len && block_table_stride >= max_blocks);
    // the wave's Q group: all next_n tokens when they fit 128 rows, else groups of 128 / H tokens; MT = its 16-row tiles (>= H / 16)
    const int tokens = std::min(next_n, 128 / num_heads);
    const int tiles = (tokens * num_heads + 15) / 16;
    const int mt_index = tiles <= 1 ? 0 : tiles <= 2 ? 1 : tiles <= 4 ? 2 : 3;
    const MqaKernelFn fn = kMqaPaged[hi][di][mt_index];
    DG_CHECK(fn != nullptr);
    dg::mqa::MqaParams p{};
    p.q = static_cast<const uint8_t*>(q); p.kv = static_cast<const uint8_t*>(kv_cache); p.weights = weights;
    p.context_lens = context_lens; p.block_table = block_table; p.schedule = schedule; p.logits = logits;
    p.logits_stride = logits_stride; p.w_stride = weights_stride; p.kv_block_stride = kv_block_stride;
    p.block_table_stride = block_table_stride;
    p.batch = batch; p.next_n = next_n; p.block_kv = block_kv; p.max_blocks = max_blocks; p.max_context_len = max_context_len;
    p.logits_bf16 = logits_dtype == DG_BF16; p.weights_bf16 = weights_dtype == DG_BF16;
    hipLaunchKernelGGL(fn, dim3(num_sms), dim3(dg::mqa::kPagedWaves * 64), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- hyper-connection pre-norm GEMM (hc_prenorm_kernels.hpp) ----

namespace {

using HcKernelFn = void (*)(const dg::hc::HcParams);
const HcKernelFn kHcKernels[2][2] = {{dg::hc::dg_hc_prenorm_gemm_kernel<1, 1>, dg::hc::dg_hc_prenorm_gemm_kernel<1, 2>},
                                     {dg::hc::dg_hc_prenorm_gemm_kernel<8, 1>, dg::hc::dg_hc_prenorm_gemm_kernel<8, 2>}};

// Row tile of a launch: 16 rows while m <= 64 (the MFMAs of a taller tile would multiply zeros), else 128.
int hc_tile_rows(int m) { return m <= 64 ? 16 : 128; }

// K pieces of a num_splits=None launch: enough work items for two workgroups per CU, at least one K block per wave and piece, at most
// 4 load batches of the sum launch (whose per-element chain is the latency of the small shapes), and the partials ([pieces][m][n + 1]
// FP32) inside the workspace; 1 = no cut, the kernel writes d and sqr_sum itself.
int hc_pieces(int m, int n, int k, int64_t workspace_bytes) {
    const int tiles = (m + hc_tile_rows(m) - 1) / hc_tile_rows(m);
    const int64_t per_piece = static_cast<int64_t>(m) * (n + 1) * static_cast<int64_t>(sizeof(float));
    int pieces = (2 * num_cus() + tiles - 1) / tiles;
    pieces = std::min({pieces, std::max(1, k / dg::hc::kBlockK / dg::hc::kWaves), 4 * dg::hc::kSumBatch});
    pieces = static_cast<int>(std::min<int64_t>(pieces, workspace_bytes / per_piece));
    return std::max(1, pieces);
}

}  // namespace

extern "C" {

int dg_hc_prenorm_pieces(int m, int n, int k, int num_splits, int64_t workspace_bytes) {
    if (m <= 0 || n <= 0 || k <= 0)
        return 0;
    return num_splits > 0 ? num_splits : hc_pieces(m, n, k, workspace_bytes);
}

int dg_tf32_hc_prenorm_gemm(const void* a, const float* b, float* d, float* sqr_sum, int m, int n, int k, int64_t a_stride,
                            int64_t b_stride, int64_t d_stride_m, int64_t d_stride_split, int num_splits, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    DG_CHECK(m >= 0 && n > 0 && k > 0 && num_splits >= 0);                              // reference hyperconnection.hpp
    DG_CHECK(n % 8 == 0 && n <= 32 && k % dg::hc::kBlockK == 0);                         // reference sm90_tf32_hc_prenorm_gemm.hpp
    DG_CHECK(a_stride >= k && b_stride >= k && d_stride_m >= n && (num_splits == 0 || d_stride_split >= 0));
    if (m == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && d != nullptr && sqr_sum != nullptr);
    const int rows = hc_tile_rows(m);
    // every in-range buffer offset of a workgroup fits 31 bits (its bases sit at the row tile and the K piece)
    DG_CHECK((static_cast<int64_t>(rows) - 1) * a_stride * 2 + static_cast<int64_t>(k) * 2 < (int64_t{1} << 31));
    DG_CHECK(static_cast<int64_t>(n - 1) * b_stride * 4 + static_cast<int64_t>(k) * 4 < (int64_t{1} << 31));
    const int pieces = num_splits > 0 ? num_splits : hc_pieces(m, n, k, workspace != nullptr ? workspace_bytes : 0);
    const bool cut = num_splits == 0 && pieces > 1;
    dg::hc::HcParams p{};
    p.a = static_cast<const uint8_t*>(a);
    p.b = b;
    p.m = m; p.n = n; p.k = k;
    p.a_stride = a_stride; p.b_stride = b_stride;
    p.tiles = (m + rows - 1) / rows;
    p.splits = pieces;
    if (cut) {                          // partials [pieces][m][n] then [pieces][m], summed in piece order by the second launch
        float* ws = static_cast<float*>(workspace);
        p.d = ws; p.d_sm = n; p.d_ss = static_cast<int64_t>(m) * n;
        p.s = ws + static_cast<int64_t>(pieces) * m * n; p.s_ss = m;
    } else {
        p.d = d; p.d_sm = d_stride_m; p.d_ss = num_splits > 0 ? d_stride_split : 0;
        p.s = sqr_sum; p.s_ss = m;
    }
    p.d_vec = reinterpret_cast<uintptr_t>(p.d) % 16 == 0 && p.d_sm % 4 == 0 && p.d_ss % 4 == 0;
    DG_CHECK(static_cast<int64_t>(p.tiles) * pieces <= 0x7fffffff);
    const HcKernelFn fn = kHcKernels[rows == 128][n > 16];
    hipLaunchKernelGGL(fn, dim3(p.tiles * pieces), dim3(dg::hc::kWaves * 64), 0, static_cast<hipStream_t>(stream), p);
    DG_HIP_CHECK(hipGetLastError());
    if (cut) {
        const int64_t items = static_cast<int64_t>(m) * (n + 1);
        const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 4 * static_cast<int64_t>(num_cus())));
        hipLaunchKernelGGL(dg::hc::dg_hc_prenorm_sum_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const float*>(workspace), pieces, m, n, d, d_stride_m, sqr_sum);
        DG_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"

extern "C" {

int dg_fp8_gemm_nt(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                   int m, int n, int k,
                   int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                   int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k,
                   int sfb_gran_n, int64_t d_stride_m, int d_dtype, int accumulate, void* stream) {
    return dg_fp8_gemm_nt_ws(a, sfa, b, sfb, d, m, n, k, a_stride_m, a_stride_k, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_k,
                             sfb_stride_n, sfb_stride_k, sfb_gran_n, d_stride_m, d_dtype, accumulate, nullptr, 0, stream);
}

int dg_fp8_gemm_nt_ws(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                      int m, int n, int k,
                      int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                      int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k,
                      int sfb_gran_n, int64_t d_stride_m, int d_dtype, int accumulate,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    DG_CHECK(m >= 0 && n >= 0 && k >= 0);
    if (m == 0 || n == 0)
        return 0;
    DG_CHECK(k > 0);   // k == 0 is resolved by the caller (D = C or 0) without a kernel, as in the reference
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr);
    DG_CHECK(a_stride_m == 1 || a_stride_k == 1);
    DG_CHECK(b_stride_n == 1 || b_stride_k == 1);
    DG_CHECK(sfb_gran_n == 1 || sfb_gran_n == 128);
    DG_CHECK(d_dtype == DG_BF16 || d_dtype == DG_FP32);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.sfa = sfa; p.b = static_cast<const uint8_t*>(b); p.sfb = sfb; p.d = d;
    p.layout = nullptr;
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_stride_m; p.a_sk = a_stride_k; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.d_sm = d_stride_m;
    p.sfb_gran_n = sfb_gran_n; p.d_dtype = d_dtype; p.accumulate = accumulate ? 1 : 0;
    p.gemm_type = dg::kNormal; p.m_alignment = 0;
    DG_CHECK(workspace == nullptr || (aligned16(workspace) && workspace_bytes >= 4096));
    p.sk_workspace = workspace;
    g_workspace_bytes = workspace != nullptr ? static_cast<size_t>(workspace_bytes) : 0;
    return launch_gemm(p, 0, stream);
}

int dg_fp8_gemm_nt_skip_head_mid(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                                 int m, int n, int k,
                                 int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                                 int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                 int sfb_gran_n, int64_t d_stride_m, int d_dtype,
                                 int head_left, int head_mid, int head_right, void* stream) {
    DG_CHECK(m >= 0 && n > 0 && k > 0);
    if (m == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr);
    DG_CHECK(a_stride_m == 1 || a_stride_k == 1);
    DG_CHECK(b_stride_n == 1 || b_stride_k == 1);
    DG_CHECK(sfb_gran_n == 1 || sfb_gran_n == 128);
    DG_CHECK(d_dtype == DG_BF16 || d_dtype == DG_FP32);
    DG_CHECK(head_left >= 0 && head_mid >= 0 && head_right >= 0 && head_left + head_right > 0);
    DG_CHECK(n % (head_left + head_right) == 0);
    DG_CHECK(d_stride_m >= n + static_cast<int64_t>(n / (head_left + head_right)) * head_mid);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.sfa = sfa; p.b = static_cast<const uint8_t*>(b); p.sfb = sfb; p.d = d;
    p.layout = nullptr;
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_stride_m; p.a_sk = a_stride_k; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.d_sm = d_stride_m;
    p.sfb_gran_n = sfb_gran_n; p.d_dtype = d_dtype; p.accumulate = 0;
    p.gemm_type = dg::kNormal; p.m_alignment = 0;
    p.head_lr = head_left + head_right; p.head_mid = head_mid; p.head_right = head_right;
    return launch_gemm(p, 0, stream);
}

static int dg_fp8_gemm_nt_ue8m0_impl(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed, void* d,
                         int m, int n, int k,
                         int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                         int64_t sfa_stride_m, int64_t sfa_stride_kq, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                         int64_t d_stride_m, int d_dtype, int accumulate, void* stream, int gran_k,
                         void* workspace = nullptr, int64_t workspace_bytes = 0) {
    DG_CHECK(m >= 0 && n >= 0 && k > 0);
    if (m == 0 || n == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa_packed != nullptr && sfb_packed != nullptr && d != nullptr);
    DG_CHECK(d_dtype == DG_BF16 || d_dtype == DG_FP32);
    DG_CHECK(d_stride_m >= n);
    DG_CHECK(sfa_stride_m == 1 && sfb_stride_n == 1);       // MN-major packed scale words (the reference's TMA layout)
    DG_CHECK(workspace == nullptr || (aligned16(workspace) && workspace_bytes >= 4096));
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.sfa = reinterpret_cast<const float*>(sfa_packed); p.sfb = reinterpret_cast<const float*>(sfb_packed);
    p.layout = nullptr;
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_stride_m; p.a_sk = a_stride_k; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = 1; p.sfa_sk = sfa_stride_kq; p.sfb_sn = 1; p.sfb_sk = sfb_stride_kq;
    p.d_sm = d_stride_m;
    p.sfb_gran_n = 128; p.d_dtype = d_dtype; p.accumulate = accumulate ? 1 : 0;
    p.gemm_type = dg::kNormal; p.m_alignment = 0;
    p.sfb_gran_n = 128;                                      // only so that the K-major / alignment test below applies
    p.sk_workspace = workspace;
    g_workspace_bytes = workspace != nullptr ? static_cast<size_t>(workspace_bytes) : 0;
    if (!fast_eligible(p, p.k % 128 == 0) && !e8_mn_eligible(p)) {
        g_last_error = "dg_fp8_gemm_nt_ue8m0 needs 16-byte aligned FP8 operands: K-major (k % 128 == 0, or k % 16 == 0 and k > 128) or, with "
                       "k % 128 == 0, MN-major (m resp. n % 16 == 0)";
        return 3;
    }
    return launch_e8(p, 0, stream, gran_k);
}

int dg_fp8_gemm_nt_ue8m0(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed, void* d,
                         int m, int n, int k,
                         int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                         int64_t sfa_stride_m, int64_t sfa_stride_kq, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                         int64_t d_stride_m, int d_dtype, int accumulate, void* stream) {
    return dg_fp8_gemm_nt_ue8m0_impl(a, sfa_packed, b, sfb_packed, d, m, n, k, a_stride_m, a_stride_k, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq, sfb_stride_n, sfb_stride_kq, d_stride_m, d_dtype, accumulate, stream, 128);
}

int dg_fp8_gemm_nt_ue8m0_ws(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed, void* d,
                            int m, int n, int k,
                            int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                            int64_t sfa_stride_m, int64_t sfa_stride_kq, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                            int64_t d_stride_m, int d_dtype, int accumulate, int gran_k, void* workspace, int64_t workspace_bytes, void* stream) {
    DG_CHECK(gran_k == 128 || gran_k == 32);
    return dg_fp8_gemm_nt_ue8m0_impl(a, sfa_packed, b, sfb_packed, d, m, n, k, a_stride_m, a_stride_k, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq,
                                     sfb_stride_n, sfb_stride_kq, d_stride_m, d_dtype, accumulate, stream, gran_k, workspace, workspace_bytes);
}

int dg_ue8m0_dense_wants_workspace(int m, int n, int k) {
    // would the automatic selection cut this packed-scale dense problem (K-major, 16-byte aligned, densely packed operands) along K if the caller
    // lent it a workspace?  The host layer asks before it creates / passes one (dg_dense_wants_workspace's twin for the hardware-scaled path).
    if (m <= 0 || n <= 0 || k <= 0)
        return 0;
    dg::GemmParams p{};
    p.a = p.b = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(1) << 20);
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = k; p.a_sk = 1; p.b_sn = k; p.b_sk = 1; p.sfa_sm = 1; p.sfb_sn = 1;
    p.gemm_type = dg::kNormal;
    if (e8_split_pieces(p, 0) >= 2)
        return 1;
    if (forced_config().find("_ks_") != std::string::npos)     // (a K-split form forced by name -- tuning runs, tests -- gets the buffer too)
        return 1;
    // the stream tiles cut along K inside the kernel (e8_stream_ks_pick: the question is asked BEFORE a workspace exists -- assume the host layer's size)
    p.sk_workspace = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 23);
    const size_t saved = g_workspace_bytes;
    g_workspace_bytes = static_cast<size_t>(dg_split_k_workspace_bytes());
    const bool ks = forced_config() == "auto" && e8_skinny_pick(p, false) == nullptr && e8_stream_ks_pick(p, false) != nullptr;
    g_workspace_bytes = saved;
    return ks ? 1 : 0;
}

int dg_fp8_gemm_nt_ue8m0_g32(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed, void* d,
                         int m, int n, int k,
                         int64_t a_stride_m, int64_t a_stride_k, int64_t b_stride_n, int64_t b_stride_k,
                         int64_t sfa_stride_m, int64_t sfa_stride_kq, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                         int64_t d_stride_m, int d_dtype, int accumulate, void* stream) {
    return dg_fp8_gemm_nt_ue8m0_impl(a, sfa_packed, b, sfb_packed, d, m, n, k, a_stride_m, a_stride_k, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq, sfb_stride_n, sfb_stride_kq, d_stride_m, d_dtype, accumulate, stream, 32);
}

int dg_ue8m0_dense_operand_plan(const void* a, const void* b, int m, int n, int k, int64_t a_stride_m, int64_t a_stride_k,
                                int64_t b_stride_n, int64_t b_stride_k) {
    // Which MN-major FP8 operands of a packed-UE8M0 dense problem the caller should re-major into K-major scratch first (bit 0: A, bit 1: B);
    // 0 = hand them over as they are.  The predicates launch_e8 applies, plus the model of when reading in place pays (e8_mn_pays) -- the
    // host layer keeps no copy.  (One kernel per majorness combination: either every MN-major operand stays, or all are re-majored.)
    const int all = (a_stride_k != 1 ? 1 : 0) | (b_stride_k != 1 ? 2 : 0);
    if (all == 0)
        return 0;
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b);
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_stride_m; p.a_sk = a_stride_k; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = 1; p.sfb_sn = 1; p.gemm_type = dg::kNormal;
    if (!e8_mn_eligible(p))
        return all;
    const std::string forced = forced_config();
    if (forced == e8_mn_config_name(p))
        return 0;
    return forced == "auto" && e8_mn_pays(p) ? 0 : all;
}

int dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                              void* d, const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                              int64_t a_stride_m, int64_t a_stride_k,
                                              int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                              int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                              int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                              int64_t d_stride_m, int use_psum, int m_alignment, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_ws(a, sfa_packed, b, sfb_packed, d, grouped_layout, num_groups, m, n, k, a_stride_m, a_stride_k,
                                                        b_stride_g, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq, sfb_stride_g, sfb_stride_n,
                                                        sfb_stride_kq, d_stride_m, use_psum, m_alignment, nullptr, 0, stream);
}

static int dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_ws_impl(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                                 void* d, const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                                 int64_t a_stride_m, int64_t a_stride_k,
                                                 int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                                 int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                                 int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                                 int64_t d_stride_m, int use_psum, int m_alignment,
                                                 void* workspace, int64_t workspace_bytes, void* stream, int gran_k) {
    DG_CHECK(m >= 0 && n > 0 && k > 0 && num_groups > 0);
    DG_CHECK(workspace == nullptr || (aligned16(workspace) && workspace_bytes >= 4096));
    if (m == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa_packed != nullptr && sfb_packed != nullptr && d != nullptr && grouped_layout != nullptr);
    // K-major A (reference gemm.hpp:181); B K-major or -- round 5 -- MN-major ([G][K][N], the nn form) where dg_ue8m0_grouped_operand_plan
    // answered 0 (launch_e8 refuses what no kernel reads in place)
    DG_CHECK(a_stride_k == 1 && (b_stride_k == 1 || b_stride_n == 1));
    DG_CHECK(sfa_stride_m == 1 && sfb_stride_n == 1);   // MN-major packed scale words
    DG_CHECK(m_alignment > 0 && m_alignment % 128 == 0);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.sfa = reinterpret_cast<const float*>(sfa_packed); p.sfb = reinterpret_cast<const float*>(sfb_packed);
    p.layout = grouped_layout;
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sm = a_stride_m; p.a_sk = 1;
    p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = 1; p.sfa_sk = sfa_stride_kq;
    p.sfb_sg = sfb_stride_g; p.sfb_sn = 1; p.sfb_sk = sfb_stride_kq;
    p.d_sm = d_stride_m;
    p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = use_psum ? dg::kContiguousPsum : dg::kContiguous;
    p.m_alignment = m_alignment;
    p.sk_workspace = workspace;
    g_workspace_bytes = workspace != nullptr ? static_cast<size_t>(workspace_bytes) : 0;
    if (b_stride_k != 1 && !e8_mn_eligible(p)) {
        g_last_error = "dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0: MN-major B is read in place only in the contiguous layout without psum, with "
                       "k % 128 == 0, n % 16 == 0, 16-byte aligned k-rows and an M alignment of 128 or a multiple of 256 (dg_ue8m0_grouped_operand_plan)";
        return 3;
    }
    return launch_e8(p, 0, stream, gran_k);
}

int dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_ws(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                                 void* d, const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                                 int64_t a_stride_m, int64_t a_stride_k,
                                                 int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                                 int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                                 int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                                 int64_t d_stride_m, int use_psum, int m_alignment,
                                                 void* workspace, int64_t workspace_bytes, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_ws_impl(a, sfa_packed, b, sfb_packed, d, grouped_layout, num_groups, m, n, k, a_stride_m, a_stride_k, b_stride_g, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq, sfb_stride_g, sfb_stride_n, sfb_stride_kq, d_stride_m, use_psum, m_alignment, workspace, workspace_bytes, stream, 128);
}

int dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_g32(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                                 void* d, const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                                 int64_t a_stride_m, int64_t a_stride_k,
                                                 int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                                 int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                                 int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                                 int64_t d_stride_m, int use_psum, int m_alignment,
                                                 void* workspace, int64_t workspace_bytes, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_contiguous_ue8m0_ws_impl(a, sfa_packed, b, sfb_packed, d, grouped_layout, num_groups, m, n, k, a_stride_m, a_stride_k, b_stride_g, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_kq, sfb_stride_g, sfb_stride_n, sfb_stride_kq, d_stride_m, use_psum, m_alignment, workspace, workspace_bytes, stream, 32);
}

int dg_ue8m0_grouped_operand_plan(const void* a, const void* b, int num_groups, int m, int n, int k, int64_t a_stride_m,
                                  int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k, int use_psum, int m_alignment) {
    // The grouped (contiguous-layout) twin of dg_ue8m0_dense_operand_plan: 2 = re-major B into K-major scratch first, 0 = hand it over as it is.
    if (b_stride_k == 1)
        return 0;
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b);
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sm = a_stride_m; p.a_sk = 1; p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = 1; p.sfb_sn = 1; p.gemm_type = use_psum ? dg::kContiguousPsum : dg::kContiguous; p.m_alignment = m_alignment;
    if (!e8_mn_eligible(p))
        return 2;
    const std::string forced = forced_config();
    if (forced == e8_mn_config_name(p))
        return 0;
    return forced == "auto" && e8_mn_pays(p) ? 0 : 2;
}

static int dg_m_grouped_fp8_gemm_nt_masked_ue8m0_impl(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                          void* d, const int32_t* masked_m, int num_groups, int m_max, int n, int k,
                                          int expected_m,
                                          int64_t a_stride_g, int64_t a_stride_m, int64_t a_stride_k,
                                          int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                          int64_t sfa_stride_g, int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                          int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                          int64_t d_stride_g, int64_t d_stride_m, void* stream, int gran_k) {
    DG_CHECK(expected_m > 0 && m_max > 0 && n > 0 && k > 0 && num_groups > 0);   // reference gemm.hpp:274
    DG_CHECK(a != nullptr && b != nullptr && sfa_packed != nullptr && sfb_packed != nullptr && d != nullptr && masked_m != nullptr);
    DG_CHECK(a_stride_k == 1 && b_stride_k == 1);       // reference gemm.hpp:263
    DG_CHECK(sfa_stride_m == 1 && sfb_stride_n == 1);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.sfa = reinterpret_cast<const float*>(sfa_packed); p.sfb = reinterpret_cast<const float*>(sfb_packed);
    p.layout = masked_m;
    p.m = m_max; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sg = a_stride_g; p.a_sm = a_stride_m; p.a_sk = 1;
    p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = 1;
    p.sfa_sg = sfa_stride_g; p.sfa_sm = 1; p.sfa_sk = sfa_stride_kq;
    p.sfb_sg = sfb_stride_g; p.sfb_sn = 1; p.sfb_sk = sfb_stride_kq;
    p.d_sg = d_stride_g; p.d_sm = d_stride_m;
    p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = dg::kMasked; p.m_alignment = 0;
    return launch_e8(p, expected_m < m_max ? expected_m : m_max, stream, gran_k);
}

int dg_m_grouped_fp8_gemm_nt_masked_ue8m0(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                          void* d, const int32_t* masked_m, int num_groups, int m_max, int n, int k,
                                          int expected_m,
                                          int64_t a_stride_g, int64_t a_stride_m, int64_t a_stride_k,
                                          int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                          int64_t sfa_stride_g, int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                          int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                          int64_t d_stride_g, int64_t d_stride_m, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_masked_ue8m0_impl(a, sfa_packed, b, sfb_packed, d, masked_m, num_groups, m_max, n, k, expected_m, a_stride_g, a_stride_m, a_stride_k, b_stride_g, b_stride_n, b_stride_k, sfa_stride_g, sfa_stride_m, sfa_stride_kq, sfb_stride_g, sfb_stride_n, sfb_stride_kq, d_stride_g, d_stride_m, stream, 128);
}

int dg_m_grouped_fp8_gemm_nt_masked_ue8m0_g32(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed,
                                          void* d, const int32_t* masked_m, int num_groups, int m_max, int n, int k,
                                          int expected_m,
                                          int64_t a_stride_g, int64_t a_stride_m, int64_t a_stride_k,
                                          int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                          int64_t sfa_stride_g, int64_t sfa_stride_m, int64_t sfa_stride_kq,
                                          int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_kq,
                                          int64_t d_stride_g, int64_t d_stride_m, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_masked_ue8m0_impl(a, sfa_packed, b, sfb_packed, d, masked_m, num_groups, m_max, n, k, expected_m, a_stride_g, a_stride_m, a_stride_k, b_stride_g, b_stride_n, b_stride_k, sfa_stride_g, sfa_stride_m, sfa_stride_kq, sfb_stride_g, sfb_stride_n, sfb_stride_kq, d_stride_g, d_stride_m, stream, 32);
}

int dg_m_grouped_fp8_gemm_nt_contiguous_ws(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                                        const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                        int64_t a_stride_m, int64_t a_stride_k,
                                        int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                        int64_t sfa_stride_m, int64_t sfa_stride_k,
                                        int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                        int64_t d_stride_m, int use_psum, int m_alignment, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
    DG_CHECK(m >= 0 && n > 0 && k > 0 && num_groups > 0);
    if (m == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr && grouped_layout != nullptr);
    DG_CHECK(a_stride_k == 1);                          // reference gemm.hpp:181: A must be K-major
    DG_CHECK(b_stride_n == 1 || b_stride_k == 1);
    DG_CHECK(m_alignment > 0 && m_alignment % 16 == 0);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.sfa = sfa; p.b = static_cast<const uint8_t*>(b); p.sfb = sfb; p.d = d;
    p.layout = grouped_layout;
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sm = a_stride_m; p.a_sk = a_stride_k;
    p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k;
    p.sfb_sg = sfb_stride_g; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.d_sm = d_stride_m;
    p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = use_psum ? dg::kContiguousPsum : dg::kContiguous;
    p.m_alignment = m_alignment;
    DG_CHECK(workspace == nullptr || (workspace_bytes >= 4096 && aligned16(workspace)));
    p.sk_workspace = workspace;
    g_workspace_bytes = workspace != nullptr ? static_cast<size_t>(workspace_bytes) : 0;
    if (const int rc = launch_contiguous_tabled(p, stream); rc != 1)
        return rc;
    return launch_gemm(p, 0, stream);
}

int dg_m_grouped_fp8_gemm_nt_contiguous(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                                        const int32_t* grouped_layout, int num_groups, int m, int n, int k,
                                        int64_t a_stride_m, int64_t a_stride_k,
                                        int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                        int64_t sfa_stride_m, int64_t sfa_stride_k,
                                        int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                        int64_t d_stride_m, int use_psum, int m_alignment, void* stream) {
    return dg_m_grouped_fp8_gemm_nt_contiguous_ws(a, sfa, b, sfb, d, grouped_layout, num_groups, m, n, k, a_stride_m, a_stride_k,
                                                  b_stride_g, b_stride_n, b_stride_k, sfa_stride_m, sfa_stride_k, sfb_stride_g,
                                                  sfb_stride_n, sfb_stride_k, d_stride_m, use_psum, m_alignment, nullptr, 0, stream);
}

int64_t dg_split_k_workspace_bytes(void) {
    // 4 KiB header + one FP32 partial tile of 256 x 256 per CU: the K split of the duo kernels needs half of it (at most half a round
    // of 128 x 256 tiles, one partial tile per CU of the round), the recipe-(1, 1, 128) split all of it (pieces x tiles <= CUs)
    return 4096 + static_cast<int64_t>(device_cu_count()) * 256 * 256 * static_cast<int64_t>(sizeof(float));
}

int dg_m_grouped_fp8_gemm_nt_masked(const void* a, const float* sfa, const void* b, const float* sfb, void* d,
                                    const int32_t* masked_m, int num_groups, int m_max, int n, int k, int expected_m,
                                    int64_t a_stride_g, int64_t a_stride_m, int64_t a_stride_k,
                                    int64_t b_stride_g, int64_t b_stride_n, int64_t b_stride_k,
                                    int64_t sfa_stride_g, int64_t sfa_stride_m, int64_t sfa_stride_k,
                                    int64_t sfb_stride_g, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                    int64_t d_stride_g, int64_t d_stride_m, void* stream) {
    DG_CHECK(expected_m > 0 && m_max > 0 && n > 0 && k > 0 && num_groups > 0);   // reference gemm.hpp:274
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr && masked_m != nullptr);
    DG_CHECK(a_stride_k == 1 && b_stride_k == 1);       // reference gemm.hpp:263
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.sfa = sfa; p.b = static_cast<const uint8_t*>(b); p.sfb = sfb; p.d = d;
    p.layout = masked_m;
    p.m = m_max; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sg = a_stride_g; p.a_sm = a_stride_m; p.a_sk = a_stride_k;
    p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = b_stride_k;
    p.sfa_sg = sfa_stride_g; p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k;
    p.sfb_sg = sfb_stride_g; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.d_sg = d_stride_g; p.d_sm = d_stride_m;
    p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = dg::kMasked; p.m_alignment = 0;
    return launch_gemm(p, expected_m < m_max ? expected_m : m_max, stream);
}

// 256-byte header (word 0: exchange waits that timed out) + one 64-word slot row per 64 x 128 tile
int64_t dg_swiglu_workspace_bytes(int num_groups, int m_max, int n) {
    return 256 + static_cast<int64_t>(num_groups) * ceil_div(m_max, 64) * (n / 128) * 64 * 4;
}

namespace {
std::atomic<long long> g_swiglu_timeout_us{10LL * 1000 * 1000};     // 10 s; the reference's grid / NVLink barriers give up after 60 s
}
void dg_set_swiglu_exchange_timeout_us(int64_t us) { g_swiglu_timeout_us.store(us > 0 ? us : 1, std::memory_order_relaxed); }

int dg_m_grouped_fp8_gemm_nt_masked_swiglu(const void* a, const float* sfa, const void* b_interleaved, const float* sfb, void* out_fp8,
                                           float* out_sf, const int32_t* masked_m, int num_groups, int m_max, int n, int k, int expected_m,
                                           int64_t a_stride_g, int64_t a_stride_m, int64_t b_stride_g, int64_t b_stride_n,
                                           int64_t sfa_stride_g, int64_t sfa_stride_k, int64_t sfb_stride_g, int64_t sfb_stride_n,
                                           int64_t sfb_stride_k, int64_t out_stride_g, int64_t out_stride_m, int64_t out_sf_stride_g,
                                           int64_t out_sf_stride_k, float activation_clamp, int use_ue8m0, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
    return dg_m_grouped_fp8_gemm_nt_masked_swiglu_weighted(a, sfa, b_interleaved, sfb, out_fp8, out_sf, masked_m, num_groups, m_max, n, k, expected_m,
                                                           a_stride_g, a_stride_m, b_stride_g, b_stride_n, sfa_stride_g, sfa_stride_k, sfb_stride_g,
                                                           sfb_stride_n, sfb_stride_k, out_stride_g, out_stride_m, out_sf_stride_g, out_sf_stride_k,
                                                           activation_clamp, use_ue8m0, nullptr, 0, workspace, workspace_bytes, stream);
}

int dg_m_grouped_fp8_gemm_nt_masked_swiglu_weighted(const void* a, const float* sfa, const void* b_interleaved, const float* sfb, void* out_fp8,
                                                    float* out_sf, const int32_t* masked_m, int num_groups, int m_max, int n, int k, int expected_m,
                                                    int64_t a_stride_g, int64_t a_stride_m, int64_t b_stride_g, int64_t b_stride_n,
                                                    int64_t sfa_stride_g, int64_t sfa_stride_k, int64_t sfb_stride_g, int64_t sfb_stride_n,
                                                    int64_t sfb_stride_k, int64_t out_stride_g, int64_t out_stride_m, int64_t out_sf_stride_g,
                                                    int64_t out_sf_stride_k, float activation_clamp, int use_ue8m0, const float* row_weight,
                                                    int64_t row_weight_stride_g, void* workspace, int64_t workspace_bytes, void* stream) {
    DG_CHECK(expected_m > 0 && m_max > 0 && n > 0 && k > 0 && num_groups > 0);
    DG_CHECK(row_weight == nullptr || (aligned16(row_weight) && row_weight_stride_g % 4 == 0 && row_weight_stride_g >= ceil_div(m_max, 64) * 64));
    DG_CHECK(a != nullptr && b_interleaved != nullptr && sfa != nullptr && sfb != nullptr && out_fp8 != nullptr && out_sf != nullptr &&
             masked_m != nullptr);
    DG_CHECK(n % 256 == 0);                             // whole pairs of [64 gate | 64 up] column tiles = whole 128-wide blocks of the intermediate
    DG_CHECK(k % 128 == 0);
    DG_CHECK(out_stride_m >= n / 2 && out_stride_m % 8 == 0 && (reinterpret_cast<uintptr_t>(out_fp8) & 7) == 0);
    DG_CHECK(out_sf_stride_k >= m_max);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.sfa = sfa; p.b = static_cast<const uint8_t*>(b_interleaved); p.sfb = sfb; p.d = nullptr;
    p.layout = masked_m;
    p.m = m_max; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sg = a_stride_g; p.a_sm = a_stride_m; p.a_sk = 1;
    p.b_sg = b_stride_g; p.b_sn = b_stride_n; p.b_sk = 1;
    p.sfa_sg = sfa_stride_g; p.sfa_sm = 1; p.sfa_sk = sfa_stride_k;
    p.sfb_sg = sfb_stride_g; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = dg::kMasked; p.m_alignment = 0;
    if (!fast_eligible(p) || !aligned16(sfa) || (sfa_stride_k * 4) % 16 != 0 || (sfa_stride_g * 4) % 16 != 0) {
        g_last_error = "dg_m_grouped_fp8_gemm_nt_masked_swiglu needs K-major 16-byte aligned FP8 operands and MN-major 16-byte aligned SFA rows";
        return 3;
    }
    p.num_m_tiles = ceil_div(m_max, 64);
    p.num_n_tiles = n / 128;
    p.group_m = 1;
    p.dbg = nullptr;
    const long max_tiles = static_cast<long>(num_groups) * p.num_m_tiles * p.num_n_tiles;
    if (workspace == nullptr || workspace_bytes < dg_swiglu_workspace_bytes(num_groups, m_max, n) || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0) {
        g_last_error = "dg_m_grouped_fp8_gemm_nt_masked_swiglu needs a zero-initialised workspace of dg_swiglu_workspace_bytes(num_groups, m_max, n) bytes";
        return 3;
    }
    dg::SwigluOut o{};
    o.errors = static_cast<uint32_t*>(workspace);
    o.amax_ws = static_cast<uint32_t*>(workspace) + 64;
    o.timeout_ticks = g_swiglu_timeout_us.load(std::memory_order_relaxed) * 100;       // s_memrealtime: 100 MHz
    o.fault = env_knobs().swiglu_fault;          // (tests only: DG_TEST_SWIGLU_FAULT + dg_reload_env; no entry point arms it)
    o.q = static_cast<uint8_t*>(out_fp8); o.sf = out_sf;
    o.q_sg = out_stride_g; o.q_sm = out_stride_m; o.sf_sg = out_sf_stride_g; o.sf_sk = out_sf_stride_k;
    o.clamp = activation_clamp; o.use_ue8m0 = use_ue8m0 ? 1 : 0;
    o.row_weight = row_weight; o.rw_sg = row_weight_stride_g;
    // round 5: 3-stage ring, two workgroups per CU (the stream2_64x128 form of select_config); DG_SWIGLU_ONE_PER_CU=1 keeps the 6-stage ring (A/B)
    const bool two = !env_knobs().swiglu_one_per_cu;
    const long slots = two ? 2L * num_cus() : num_cus();
    const long grid = std::min<long>(max_tiles, std::max<long>(2, slots & ~1L));  // even: tile t and its partner t ^ 1 run in the same iteration
    g_last_config = two ? "stream_swiglu2_64x128" : "stream_swiglu_64x128";
    if (two)
        hipLaunchKernelGGL(dg::dg_fp8_gemm_stream_swiglu_kernel<3>, dim3(static_cast<unsigned>(grid)), dim3(256), 0, static_cast<hipStream_t>(stream), p, o);
    else
        hipLaunchKernelGGL(dg::dg_fp8_gemm_stream_swiglu_kernel<6>, dim3(static_cast<unsigned>(grid)), dim3(256), 0, static_cast<hipStream_t>(stream), p, o);
    DG_HIP_CHECK(hipGetLastError());
    (void)expected_m;
    return 0;
}

int dg_moe_scatter_to_masked(const void* x_fp8, const float* x_sf, const void* topk_idx, int topk_idx_is_int64, const float* topk_weights,
                             int tokens, int hidden, int topk, int num_experts, int max_m, int64_t x_stride_m, int64_t x_sf_stride_m,
                             void* a_out, float* sfa_out, float* row_weight_out, int32_t* slot_out, int32_t* masked_m_out, void* error_word,
                             int64_t a_stride_g, int64_t a_stride_m, int64_t sfa_stride_g, int64_t sfa_stride_k, int64_t row_weight_stride_g,
                             void* stream) {
    DG_CHECK(tokens >= 0 && hidden > 0 && hidden % 128 == 0 && topk > 0 && topk <= dg::kMoeMaxTopk && num_experts > 0 && max_m > 0);
    DG_CHECK(x_fp8 != nullptr && x_sf != nullptr && topk_idx != nullptr && topk_weights != nullptr && a_out != nullptr && sfa_out != nullptr &&
             row_weight_out != nullptr && slot_out != nullptr && masked_m_out != nullptr && error_word != nullptr);
    DG_CHECK(aligned16(x_fp8) && aligned16(a_out) && x_stride_m % 16 == 0 && a_stride_m % 16 == 0 && a_stride_g % 16 == 0);
    DG_HIP_CHECK(hipMemsetAsync(masked_m_out, 0, sizeof(int32_t) * num_experts, static_cast<hipStream_t>(stream)));
    if (tokens == 0)
        return 0;
    dg::MoeRoute r{};
    r.x = static_cast<const uint8_t*>(x_fp8); r.x_sf = x_sf; r.topk_idx = topk_idx; r.topk_w = topk_weights;
    r.tokens = tokens; r.hidden = hidden; r.topk = topk; r.num_experts = num_experts; r.max_m = max_m; r.idx64 = topk_idx_is_int64 ? 1 : 0;
    r.x_sm = x_stride_m; r.xsf_sm = x_sf_stride_m;
    r.a = static_cast<uint8_t*>(a_out); r.sfa = sfa_out; r.rw = row_weight_out; r.slot = slot_out; r.counts = masked_m_out;
    r.errors = static_cast<uint32_t*>(error_word);
    r.a_sg = a_stride_g; r.a_sm = a_stride_m; r.sfa_sg = sfa_stride_g; r.sfa_sk = sfa_stride_k; r.rw_sg = row_weight_stride_g;
    hipLaunchKernelGGL(dg::dg_moe_scatter_kernel, dim3(static_cast<unsigned>(tokens)), dim3(256), 0, static_cast<hipStream_t>(stream), r);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_moe_combine_from_masked(const void* y2_bf16, const int32_t* slot, int tokens, int topk, int hidden, int64_t y2_row_stride, void* y_bf16,
                               int64_t y_stride_m, void* stream) {
    DG_CHECK(tokens >= 0 && topk > 0 && hidden > 0 && hidden % 8 == 0 && y2_row_stride % 8 == 0 && y_stride_m % 8 == 0);
    DG_CHECK(y2_bf16 != nullptr && slot != nullptr && y_bf16 != nullptr && aligned16(y2_bf16) && aligned16(y_bf16));
    if (tokens == 0)
        return 0;
    hipLaunchKernelGGL(dg::dg_moe_combine_kernel, dim3(static_cast<unsigned>(tokens), static_cast<unsigned>((hidden + 2047) / 2048)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t*>(y2_bf16), slot, tokens, topk, hidden, y2_row_stride, static_cast<uint16_t*>(y_bf16), y_stride_m);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- in-kernel dispatch / combine over peer-mapped memory (fp8_gemm_moe.hpp, "In-kernel dispatch / combine") ----
namespace {
std::atomic<long long> g_p2p_timeout_us{10LL * 1000 * 1000};        // 10 s, as the fused L1 kernel's partner wait

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

dg::P2pLayout p2p_layout(int local_experts, int cap, int hidden, int max_tokens, int topk, int world) {
    dg::P2pLayout l{};
    int64_t off = 0;
    l.counts = off;   off += align_up(4LL * local_experts, 256);
    l.arrived = off;  off += align_up(4LL * world, 256);
    l.combined = off; off += align_up(4LL * world, 256);
    l.done = off;     off += 256;
    off = align_up(off, 4096);
    l.l1_acts = off;  off += align_up(static_cast<int64_t>(local_experts) * cap * hidden, 256);
    l.l1_sf = off;    off += align_up(4LL * local_experts * (hidden / 128) * cap, 256);
    l.row_w = off;    off += align_up(4LL * local_experts * cap, 256);
    l.src_info = off; off += align_up(4LL * local_experts * cap, 256);
    l.y_rows = off;   off += align_up(2LL * max_tokens * topk * hidden, 256);
    l.bytes = off;
    return l;
}

int fill_p2p_args(dg::P2pArgs& a, const void* const* peer_regions, int world, int rank, int local_experts, int cap, int hidden, int max_tokens,
                  int topk, int tokens, unsigned epoch, void* errors) {
    DG_CHECK(peer_regions != nullptr && world >= 1 && world <= dg::kMaxPeers && rank >= 0 && rank < world);
    DG_CHECK(local_experts >= 1 && cap >= 1 && cap % 4 == 0 && hidden > 0 && hidden % 128 == 0 && topk >= 1 && topk <= dg::kP2pMaxTopk && max_tokens >= 1);
    DG_CHECK(tokens >= 0 && tokens <= max_tokens && static_cast<int64_t>(max_tokens) * topk < (1 << 24) && epoch != 0 && errors != nullptr);
    for (int r = 0; r < world; ++r) {
        DG_CHECK(peer_regions[r] != nullptr && aligned16(peer_regions[r]));
        a.peer[r] = static_cast<uint8_t*>(const_cast<void*>(peer_regions[r]));
    }
    a.lay = p2p_layout(local_experts, cap, hidden, max_tokens, topk, world);
    a.world = world; a.rank = rank; a.tokens = tokens; a.hidden = hidden; a.topk = topk; a.num_experts = local_experts * world;
    a.local_experts = local_experts; a.cap = cap; a.epoch = epoch;
    a.stamps = g_debug_buffer.load(std::memory_order_relaxed);       // (tuning: the phase stamps live 65536 words into the debug buffer)
    if (a.stamps != nullptr) a.stamps += 65536;
    a.timeout_ticks = g_p2p_timeout_us.load(std::memory_order_relaxed) * 100;        // wall_clock64: 100 MHz
    a.errors = static_cast<uint32_t*>(errors);
    return 0;
}
}  // namespace

void dg_set_moe_p2p_timeout_us(int64_t us) { g_p2p_timeout_us.store(us > 0 ? us : 1, std::memory_order_relaxed); }

int dg_symm_alloc(int64_t bytes, void** out_ptr, int* out_fine_grained) {
    DG_CHECK(bytes > 0 && out_ptr != nullptr);
    void* ptr = nullptr;
    int fine = 0;
    // fine-grained device memory where the runtime grants it (coherent for peers without cache maintenance); ordinary device memory otherwise
    // -- or when the caller asks for it: DG_SYMM_COARSE=1 (tests compare both)
    if (getenv("DG_SYMM_COARSE") == nullptr && hipExtMallocWithFlags(&ptr, static_cast<size_t>(bytes), hipDeviceMallocFinegrained) == hipSuccess && ptr != nullptr)
        fine = 1;
    else {
        (void)hipGetLastError();
        ptr = nullptr;
        DG_HIP_CHECK(hipMalloc(&ptr, static_cast<size_t>(bytes)));
    }
    DG_HIP_CHECK(hipMemset(ptr, 0, static_cast<size_t>(bytes)));
    DG_HIP_CHECK(hipDeviceSynchronize());
    *out_ptr = ptr;
    if (out_fine_grained != nullptr)
        *out_fine_grained = fine;
    return 0;
}

int dg_symm_free(void* ptr) {
    if (ptr != nullptr)
        DG_HIP_CHECK(hipFree(ptr));
    return 0;
}

int dg_ipc_get_handle(void* ptr, void* handle_out_64_bytes) {
    DG_CHECK(ptr != nullptr && handle_out_64_bytes != nullptr);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the handle crosses the ABI as 64 opaque bytes");
    hipIpcMemHandle_t h;
    DG_HIP_CHECK(hipIpcGetMemHandle(&h, ptr));
    std::memcpy(handle_out_64_bytes, &h, sizeof(h));
    return 0;
}

int dg_ipc_open_handle(const void* handle_64_bytes, void** out_ptr) {
    DG_CHECK(handle_64_bytes != nullptr && out_ptr != nullptr);
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle_64_bytes, sizeof(h));
    void* ptr = nullptr;
    DG_HIP_CHECK(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
    *out_ptr = ptr;
    return 0;
}

int dg_ipc_close_handle(void* ptr) {
    if (ptr != nullptr)
        DG_HIP_CHECK(hipIpcCloseMemHandle(ptr));
    return 0;
}

int dg_moe_p2p_layout(int local_experts, int capacity, int hidden, int max_tokens, int topk, int world, int64_t* offsets_out_10) {
    DG_CHECK(offsets_out_10 != nullptr && local_experts >= 1 && capacity >= 1 && hidden % 128 == 0 && hidden > 0 && max_tokens >= 1 && topk >= 1 && world >= 1);
    const dg::P2pLayout l = p2p_layout(local_experts, capacity, hidden, max_tokens, topk, world);
    const int64_t v[10] = {l.counts, l.arrived, l.combined, l.done, l.l1_acts, l.l1_sf, l.row_w, l.src_info, l.y_rows, l.bytes};
    std::memcpy(offsets_out_10, v, sizeof(v));
    return 0;
}

int dg_moe_p2p_dispatch(const void* const* peer_regions, int world, int rank, int local_experts, int capacity, int hidden, int max_tokens, int topk,
                        const void* x_fp8, const float* x_sf, const void* topk_idx, int topk_idx_is_int64, const float* topk_weights, int tokens,
                        int64_t x_stride_m, int64_t x_sf_stride_m, uint32_t epoch, int32_t* masked_m_out, void* pair_ok_out, void* errors,
                        void* stream) {
    dg::P2pArgs a{};
    if (const int rc = fill_p2p_args(a, peer_regions, world, rank, local_experts, capacity, hidden, max_tokens, topk, tokens, epoch, errors))
        return rc;
    DG_CHECK(masked_m_out != nullptr && pair_ok_out != nullptr);
    DG_CHECK(tokens == 0 || (x_fp8 != nullptr && x_sf != nullptr && topk_idx != nullptr && topk_weights != nullptr && aligned16(x_fp8) && x_stride_m % 16 == 0));
    a.x = static_cast<const uint8_t*>(x_fp8); a.x_sf = x_sf; a.topk_idx = topk_idx; a.topk_w = topk_weights; a.idx64 = topk_idx_is_int64 ? 1 : 0;
    a.x_sm = x_stride_m; a.xsf_sm = x_sf_stride_m; a.masked_m = masked_m_out; a.pair_ok = static_cast<uint8_t*>(pair_ok_out);
    // (a rank without tokens still announces itself to every peer: one workgroup)
    hipLaunchKernelGGL(dg::dg_moe_p2p_dispatch_kernel, dim3(static_cast<unsigned>(std::max(tokens, 1))), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_moe_p2p_combine(const void* const* peer_regions, int world, int rank, int local_experts, int capacity, int hidden, int max_tokens, int topk,
                       const void* l2_out_bf16, int64_t l2_stride_g, int64_t l2_stride_m, const int32_t* masked_m, uint32_t epoch, void* errors,
                       void* stream) {
    dg::P2pArgs a{};
    if (const int rc = fill_p2p_args(a, peer_regions, world, rank, local_experts, capacity, hidden, max_tokens, topk, 0, epoch, errors))
        return rc;
    DG_CHECK(l2_out_bf16 != nullptr && masked_m != nullptr && aligned16(l2_out_bf16) && l2_stride_m % 8 == 0 && l2_stride_g % 8 == 0);
    a.l2_out = static_cast<const uint16_t*>(l2_out_bf16); a.l2_sg = l2_stride_g; a.l2_sm = l2_stride_m; a.masked_m = const_cast<int32_t*>(masked_m);
    const long rows = static_cast<long>(local_experts) * capacity;
    const long grid = std::max<long>(1, std::min<long>(rows, 4L * num_cus()));
    hipLaunchKernelGGL(dg::dg_moe_p2p_combine_kernel, dim3(static_cast<unsigned>(grid)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_moe_p2p_reduce(const void* const* peer_regions, int world, int rank, int local_experts, int capacity, int hidden, int max_tokens, int topk,
                      const void* pair_ok, int tokens, void* y_bf16, int64_t y_stride_m, const void* swiglu_workspace, uint32_t epoch, void* errors,
                      void* stream) {
    dg::P2pArgs a{};
    if (const int rc = fill_p2p_args(a, peer_regions, world, rank, local_experts, capacity, hidden, max_tokens, topk, tokens, epoch, errors))
        return rc;
    DG_CHECK(pair_ok != nullptr && (tokens == 0 || (y_bf16 != nullptr && aligned16(y_bf16) && y_stride_m % 8 == 0)));
    a.pair_ok = static_cast<uint8_t*>(const_cast<void*>(pair_ok)); a.y = static_cast<uint16_t*>(y_bf16); a.y_sm = y_stride_m;
    a.swiglu_errors = static_cast<const uint32_t*>(swiglu_workspace);
    // (a rank without tokens still waits for -- and thereby orders itself behind -- every owner's combine: one workgroup)
    hipLaunchKernelGGL(dg::dg_moe_p2p_reduce_kernel, dim3(static_cast<unsigned>(std::max(tokens, 1)), static_cast<unsigned>((hidden + 2047) / 2048)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_k_grouped_fp8_gemm_nt_contiguous(const void* a, const float* sfa, const void* b, const float* sfb, float* d,
                                        int m, int n, const int32_t* ks_host, int num_groups, int ab_layout,
                                        int64_t a_stride_m, int64_t b_stride_n,
                                        int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                        void* stream) {
    DG_CHECK(m >= 0 && n >= 0 && num_groups >= 0);
    if (m == 0 || n == 0 || num_groups == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr && ks_host != nullptr);
    DG_CHECK(ab_layout == DG_KGROUPED_BLOCKS || ab_layout == DG_KGROUPED_COLUMNS || ab_layout == DG_KGROUPED_ROWS);
    for (int g = 0; g < num_groups; ++g)
        DG_CHECK(ks_host[g] >= 0 && ks_host[g] % 128 == 0);
    // One launch over all groups when the per-column-SFB LDS-DMA kernel applies: tile order is group-major and the hardware
    // hands the next workgroup to whichever CU frees up, so groups of different K extents balance without per-group tails.
    {
        dg::GemmParams p{};
        p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.sfa = sfa; p.sfb = sfb; p.d = d;
        p.layout = nullptr;
        p.m = m; p.n = n; p.num_groups = num_groups;
        p.a_sk = 1; p.b_sk = 1;
        p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
        p.d_sm = n; p.d_sg = static_cast<int64_t>(m) * n;
        p.sfb_gran_n = 1; p.d_dtype = DG_FP32; p.accumulate = 1; p.m_alignment = 0;
        p.kg_blocks = ab_layout == DG_KGROUPED_BLOCKS ? 1 : 0;
        const bool mn_major = ab_layout == DG_KGROUPED_ROWS;
        int64_t sum_k = 0;
        int k_min = 1 << 30;
        for (int g = 0; g < num_groups && g <= dg::kMaxKGroups; ++g) {
            if (g < dg::kMaxKGroups) p.kg_prefix[g] = static_cast<int>(sum_k);
            sum_k += ks_host[g];
            if (ks_host[g] > 0 && ks_host[g] < k_min) k_min = ks_host[g];
        }
        bool single = num_groups <= dg::kMaxKGroups && sum_k > 0 && sum_k < (1LL << 31) && m > 64 &&
                      forced_config() == "auto";
        if (mn_major) {
            // MN-major operands [sum_k, m] / [sum_k, n] (row pitches a_stride_m / b_stride_n): only the single launch of the
            // transpose-read kernel takes them; everything else needs the K-major forms (the host layer re-majors)
            const bool ok = single && aligned16(a) && aligned16(b) && a_stride_m % 16 == 0 && b_stride_n % 16 == 0 &&
                            a_stride_m >= m && b_stride_n >= n && a_stride_m <= (1 << 22) && b_stride_n <= (1 << 22) &&
                            sum_k * a_stride_m < (1LL << 31) && sum_k * b_stride_n < (1LL << 31) &&
                            sfa_stride_m == 1 && sfb_stride_n == 1 && aligned16(sfa) && aligned16(sfb) &&
                            sfa_stride_k % 4 == 0 && sfb_stride_k % 4 == 0;
            if (!ok) {
                g_last_error = "DG_KGROUPED_ROWS needs 16-byte aligned MN-major operands, MN-major scales, m > 64, at most 64 "
                               "groups and automatic kernel selection; re-major the operands and use DG_KGROUPED_COLUMNS";
                return 3;
            }
            p.a_sm = 1; p.a_sk = a_stride_m; p.b_sn = 1; p.b_sk = b_stride_n;
            p.kg_prefix[num_groups] = static_cast<int>(sum_k);
            p.gemm_type = dg::kKGrouped;
            p.k = static_cast<int>(sum_k);
            p.num_m_tiles = ceil_div(m, 256);
            p.num_n_tiles = ceil_div(n, 256);
            p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
            p.d_vec_ok = aligned16(p.d) && (p.d_sm * 4) % 16 == 0 && (p.d_sg * 4) % 16 == 0;
            p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
            const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * num_groups;
            if (grid > 0x7fffffffL)
                return fail(__FILE__, __LINE__, "grid too large");
            g_last_config = "pipe_pc_mn_256x256";
            hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, true>),
                               dim3(static_cast<unsigned>(grid)), dim3(512), 0, static_cast<hipStream_t>(stream), p);
            DG_HIP_CHECK(hipGetLastError());
            return 0;
        }
        if (single) {
            p.kg_prefix[num_groups] = static_cast<int>(sum_k);
            // eligibility is that of a dense launch on the most constrained group (smallest row stride in the blocks form)
            p.gemm_type = dg::kNormal;
            p.k = k_min;
            p.a_sm = p.kg_blocks ? k_min : a_stride_m; p.b_sn = p.kg_blocks ? k_min : b_stride_n;
            single = per_col_eligible(p);
            if (single && p.kg_blocks)
                for (int g = 0; g < num_groups; ++g)
                    single = single && (ks_host[g] % 16 == 0) && (static_cast<int64_t>(p.kg_prefix[g]) * m) % 16 == 0 &&
                             (static_cast<int64_t>(p.kg_prefix[g]) * n) % 16 == 0;
        }
        if (single) {
            p.gemm_type = dg::kKGrouped;
            p.a_sm = a_stride_m; p.b_sn = b_stride_n;          // blocks form: the kernel takes k_g as the row stride
            p.k = static_cast<int>(sum_k);
            p.num_m_tiles = ceil_div(m, 256);
            p.num_n_tiles = ceil_div(n, 256);
            p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
            p.d_vec_ok = aligned16(p.d) && (p.d_sm * 4) % 16 == 0 && (p.d_sg * 4) % 16 == 0;
            p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
            const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * num_groups;
            if (grid > 0x7fffffffL)
                return fail(__FILE__, __LINE__, "grid too large");
            g_last_config = "pipe_pc_256x256";
            hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, false>), dim3(static_cast<unsigned>(grid)),
                               dim3(512), 0, static_cast<hipStream_t>(stream), p);
            DG_HIP_CHECK(hipGetLastError());
            return 0;
        }
    }
    // Otherwise one dense per-column-SFB launch per non-empty group on the caller's stream.
    int64_t k_begin = 0;
    for (int g = 0; g < num_groups; ++g) {
        const int k = ks_host[g];
        if (k > 0) {
            dg::GemmParams p{};
            if (ab_layout == DG_KGROUPED_BLOCKS) {
                p.a = static_cast<const uint8_t*>(a) + k_begin * m; p.a_sm = k;
                p.b = static_cast<const uint8_t*>(b) + k_begin * n; p.b_sn = k;
            } else {
                p.a = static_cast<const uint8_t*>(a) + k_begin; p.a_sm = a_stride_m;
                p.b = static_cast<const uint8_t*>(b) + k_begin; p.b_sn = b_stride_n;
            }
            p.a_sk = 1; p.b_sk = 1;
            p.sfa = sfa + (k_begin / 128) * sfa_stride_k; p.sfb = sfb + (k_begin / 128) * sfb_stride_k;
            p.d = d + static_cast<int64_t>(g) * m * n;
            p.layout = nullptr;
            p.m = m; p.n = n; p.k = k; p.num_groups = 1;
            p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
            p.d_sm = n;
            p.sfb_gran_n = 1; p.d_dtype = DG_FP32; p.accumulate = 1;
            p.gemm_type = dg::kNormal; p.m_alignment = 0;
            const int rc = launch_gemm(p, 0, stream);
            if (rc != 0)
                return rc;
        }
        k_begin += k;
    }
    return 0;
}

int dg_k_grouped_fp8_gemm_tn_psum(const void* a, const float* sfa, const void* b, const float* sfb, float* d, int m, int n, int total_k,
                                  const int32_t* psum_layout, int num_groups, int ab_layout, int64_t a_stride_m, int64_t b_stride_n,
                                  int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k, void* stream) {
    return dg_k_grouped_fp8_gemm_tn_psum_aligned(a, sfa, b, sfb, d, m, n, total_k, psum_layout, num_groups, ab_layout, a_stride_m, b_stride_n,
                                                 sfa_stride_m, sfa_stride_k, sfb_stride_n, sfb_stride_k, 128, stream);
}

int dg_k_grouped_fp8_gemm_tn_psum_aligned(const void* a, const float* sfa, const void* b, const float* sfb, float* d, int m, int n, int total_k,
                                          const int32_t* psum_layout, int num_groups, int ab_layout, int64_t a_stride_m, int64_t b_stride_n,
                                          int64_t sfa_stride_m, int64_t sfa_stride_k, int64_t sfb_stride_n, int64_t sfb_stride_k,
                                          int k_alignment, void* stream) {
    DG_CHECK(m >= 0 && n >= 0 && num_groups >= 0 && total_k >= 0);
    if (m == 0 || n == 0 || num_groups == 0 || total_k == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa != nullptr && sfb != nullptr && d != nullptr && psum_layout != nullptr);
    DG_CHECK(ab_layout == DG_KGROUPED_COLUMNS || ab_layout == DG_KGROUPED_ROWS);
    DG_CHECK(k_alignment > 0 && k_alignment % 32 == 0 && total_k % k_alignment == 0);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.sfa = sfa; p.sfb = sfb; p.d = d;
    p.layout = psum_layout;
    p.m = m; p.n = n; p.k = total_k; p.num_groups = num_groups;
    p.sfa_sm = sfa_stride_m; p.sfa_sk = sfa_stride_k; p.sfb_sn = sfb_stride_n; p.sfb_sk = sfb_stride_k;
    p.d_sm = n; p.d_sg = static_cast<int64_t>(m) * n;
    p.sfb_gran_n = 1; p.d_dtype = DG_FP32; p.accumulate = 1;
    p.m_alignment = k_alignment == 128 ? 0 : k_alignment;       // (kernel: the K alignment of the psum layout; 0 = whole 128-blocks)
    p.kg_blocks = 0; p.kg_psum = 1;
    const bool mn_major = ab_layout == DG_KGROUPED_ROWS;
    // (a K alignment other than 128 means partial last blocks: masked by the operand descriptors of the MN-major form only)
    bool ok = m > 64 && (k_alignment == 128 || mn_major);
    if (mn_major) {
        ok = ok && aligned16(a) && aligned16(b) && a_stride_m % 16 == 0 && b_stride_n % 16 == 0 && a_stride_m >= m && b_stride_n >= n &&
             a_stride_m <= (1 << 22) && b_stride_n <= (1 << 22) && static_cast<int64_t>(total_k) * a_stride_m < (1LL << 31) &&
             static_cast<int64_t>(total_k) * b_stride_n < (1LL << 31) && sfa_stride_m == 1 && sfb_stride_n == 1 && aligned16(sfa) &&
             aligned16(sfb) && sfa_stride_k % 4 == 0 && sfb_stride_k % 4 == 0;
        p.a_sm = 1; p.a_sk = a_stride_m; p.b_sn = 1; p.b_sk = b_stride_n;
    } else {
        p.a_sm = a_stride_m; p.a_sk = 1; p.b_sn = b_stride_n; p.b_sk = 1;
        p.gemm_type = dg::kNormal;
        ok = ok && per_col_eligible(p);
    }
    if (!ok) {
        g_last_error = "the psum form of the K-grouped GEMM needs m > 64, 16-byte aligned operand rows and MN-major, 16-byte aligned "
                       "scales (nothing was launched; DG_KGROUPED_ROWS callers re-major the operands and retry with DG_KGROUPED_COLUMNS)";
        return 3;
    }
    p.gemm_type = dg::kKGrouped;
    p.num_m_tiles = ceil_div(m, 256);
    p.num_n_tiles = ceil_div(n, 256);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    p.d_vec_ok = aligned16(p.d) && (p.d_sm * 4) % 16 == 0 && (p.d_sg * 4) % 16 == 0;
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * num_groups;
    if (grid > 0x7fffffffL)
        return fail(__FILE__, __LINE__, "grid too large");
    if (mn_major) {
        g_last_config = "pipe_pc_mn_256x256";
        hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, true>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                           static_cast<hipStream_t>(stream), p);
    } else {
        g_last_config = "pipe_pc_256x256";
        hipLaunchKernelGGL((dg::dg_fp8_gemm_pipe_pc_kernel<256, 256, 2, 4, 1, false>), dim3(static_cast<unsigned>(grid)), dim3(512), 0,
                           static_cast<hipStream_t>(stream), p);
    }
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_k_grouped_fp8_gemm_ue8m0(const void* a, const int32_t* sfa_packed, const void* b, const int32_t* sfb_packed, float* d,
                                int m, int n, int total_k, const int32_t* ks_host, const int32_t* psum_layout, int num_groups,
                                int k_alignment, int gran_k, int ab_layout, int64_t a_stride_m, int64_t b_stride_n,
                                int64_t sfa_stride_k, int64_t sfb_stride_k, void* stream) {
    DG_CHECK(m >= 0 && n >= 0 && num_groups >= 0 && total_k >= 0);
    DG_CHECK(ab_layout == DG_KGROUPED_COLUMNS || ab_layout == DG_KGROUPED_ROWS);
    if (m == 0 || n == 0 || num_groups == 0 || total_k == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && sfa_packed != nullptr && sfb_packed != nullptr && d != nullptr);
    DG_CHECK(gran_k == 128 || gran_k == 32);
    DG_CHECK(k_alignment > 0 && k_alignment % 32 == 0);
    const bool psum = psum_layout != nullptr;
    DG_CHECK(psum || ks_host != nullptr);
    DG_CHECK(num_groups <= (psum ? 128 : dg::kMaxKGroups));
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.sfa = reinterpret_cast<const float*>(sfa_packed); p.sfb = reinterpret_cast<const float*>(sfb_packed);
    p.layout = psum_layout;
    p.m = m; p.n = n; p.k = total_k; p.num_groups = num_groups;
    const bool mn_major = ab_layout == DG_KGROUPED_ROWS;       // a [total_k, m], b [total_k, n] as they are: a_stride_m / b_stride_n are the k-row pitches
    if (mn_major) { p.a_sm = 1; p.a_sk = a_stride_m; p.b_sn = 1; p.b_sk = b_stride_n; }
    else { p.a_sm = a_stride_m; p.a_sk = 1; p.b_sn = b_stride_n; p.b_sk = 1; }
    p.sfa_sm = 1; p.sfa_sk = sfa_stride_k; p.sfb_sn = 1; p.sfb_sk = sfb_stride_k;
    p.d_sm = n; p.d_sg = static_cast<int64_t>(m) * n;
    p.sfb_gran_n = 1; p.d_dtype = DG_FP32; p.accumulate = 1;
    p.m_alignment = k_alignment; p.kg_blocks = 0; p.kg_psum = psum ? 1 : 0;
    if (!psum) {
        int64_t sum_k = 0;
        for (int g = 0; g < num_groups; ++g) {
            DG_CHECK(ks_host[g] >= 0 && ks_host[g] % 32 == 0);
            p.kg_prefix[g] = static_cast<int>(sum_k);
            sum_k += ks_host[g];
            DG_CHECK(sum_k <= total_k);
        }
        p.kg_prefix[num_groups] = static_cast<int>(sum_k);
    }
    // K-major rows the LDS-DMA pieces can address (16-byte chunks, 32-bit offsets), scale rows the 16-byte loads can (see fast_eligible)
    const bool sf_ok = aligned16(sfa_packed) && aligned16(sfb_packed) && sfa_stride_k % 4 == 0 && sfb_stride_k % 4 == 0 && sfa_stride_k >= m && sfb_stride_k >= n;
    const bool ok = mn_major
        // in place: the 256-row form only, k-rows the LDS-DMA pieces can address with 32-bit offsets
        ? sf_ok && m > 128 && aligned16(a) && aligned16(b) && a_stride_m % 16 == 0 && b_stride_n % 16 == 0 && a_stride_m >= m && b_stride_n >= n &&
          static_cast<int64_t>(total_k) * a_stride_m < (1LL << 31) && static_cast<int64_t>(total_k) * b_stride_n < (1LL << 31) && forced_config() == "auto"
        : sf_ok && aligned16(a) && aligned16(b) && a_stride_m % 16 == 0 && b_stride_n % 16 == 0 && a_stride_m >= total_k && b_stride_n >= total_k &&
          a_stride_m <= (1 << 22) && b_stride_n <= (1 << 22);
    if (!ok) {
        g_last_error = mn_major ? "dg_k_grouped_fp8_gemm_ue8m0(DG_KGROUPED_ROWS) needs m > 128, 16-byte aligned MN-major operands (pitch x total_k < 2 GiB) and "
                                  "packed scale rows whose pitch is a multiple of four words (nothing was launched: re-major and use DG_KGROUPED_COLUMNS)"
                                : "dg_k_grouped_fp8_gemm_ue8m0 needs K-major FP8 operands with 16-byte aligned rows (pitch <= 4 MiB) and packed scale rows "
                                  "whose pitch is a multiple of four words behind a 16-byte aligned base (nothing was launched)";
        return 3;
    }
    p.gemm_type = dg::kKGrouped;
    const bool big = m > 128;
    const int bm = big ? 256 : 128;
    p.num_m_tiles = ceil_div(m, bm);
    p.num_n_tiles = ceil_div(n, 256);
    p.group_m = p.num_m_tiles >= 8 ? 4 : (p.num_m_tiles >= 2 ? 2 : 1);
    p.d_vec_ok = aligned16(p.d) && (p.d_sm * 4) % 16 == 0 && (p.d_sg * 4) % 16 == 0;
    p.dbg = g_debug_buffer.load(std::memory_order_relaxed);
    const long grid = static_cast<long>(p.num_m_tiles) * p.num_n_tiles * num_groups;
    if (grid > 0x7fffffffL)
        return fail(__FILE__, __LINE__, "grid too large");
    // One workgroup per tile, group-major: the hardware hands the next tile to whichever CU frees up, so groups of different K extents balance.
    const dim3 g3(static_cast<unsigned>(grid)), b3(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mn_major) {
        g_last_config = gran_k == 32 ? "e8_quad_kg_mn_g32_256x256" : "e8_quad_kg_mn_256x256";
        if (gran_k == 32) hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true, true, true>), g3, b3, 0, s, p);
        else hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, false, true, true>), g3, b3, 0, s, p);
    } else if (gran_k == 32) {
        g_last_config = big ? "e8_quad_kg_g32_256x256" : "e8_quad_kg_g32_128x256";
        if (big) hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, true, true>), g3, b3, 0, s, p);
        else hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, true, true>), g3, b3, 0, s, p);
    } else {
        g_last_config = big ? "e8_quad_kg_256x256" : "e8_quad_kg_128x256";
        if (big) hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<256, 256, 0, false, 2, false, 0, false, false, true>), g3, b3, 0, s, p);
        else hipLaunchKernelGGL((dg::dg_fp8_gemm_quad_e8_kernel<128, 256, 0, false, 2, false, 0, false, false, true>), g3, b3, 0, s, p);
    }
    DG_HIP_CHECK(hipGetLastError());
    if (env_knobs().print_configs)
        fprintf(stderr, "[deepgemm_amd] ue8m0 k-grouped m=%d n=%d total_k=%d groups=%d gran_k=%d -> %s\n", m, n, total_k, num_groups, gran_k,
                g_last_config.c_str());
    return 0;
}

namespace dg {
// FP32 power-of-two scales of a K-grouped operand -> the packed words of the K-grouped hardware-scaled kernels (see the header).  One thread per
// (packed row, four consecutive mn): finds the packed row's group by one pass over the groups, reads up to four scale rows, keeps the exponent bytes.
__global__ __launch_bounds__(256)
void dg_pack_sf_k_grouped_ue8m0_kernel(const float* sf, int32_t* out, const int32_t* group_ks, int num_groups, int mn, int sf_k, int packed_sf_k,
                                       int gran_k, int k_alignment, int use_psum) {
    const int packed_row = blockIdx.y;
    const int mn4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (mn4 >= mn)
        return;
    int sf_rows = 0, packed_rows = 0, prev_end = 0, row0 = -1, row_end = 0, first_packed = 0;
    for (int g = 0; g < num_groups; ++g) {
        int group_k;
        if (use_psum) {
            const int end = group_ks[g];
            group_k = end - (prev_end + k_alignment - 1) / k_alignment * k_alignment;
            prev_end = end;
        } else {
            group_k = group_ks[g];
        }
        const int rows = group_k > 0 ? (group_k + gran_k - 1) / gran_k : 0;
        if (packed_row < packed_rows + (rows + 3) / 4) {
            row0 = sf_rows; row_end = sf_rows + rows; first_packed = packed_rows;
            break;
        }
        sf_rows += rows;
        packed_rows += (rows + 3) / 4;
    }
    if (row0 < 0)
        return;                                         // a packed row beyond the groups' last: left as it is (the reference returns as well)
    uint32_t word[4] = {0, 0, 0, 0};
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = row0 + (packed_row - first_packed) * 4 + j;
        if (r < row_end && r < sf_k) {
            const uint4 v = *reinterpret_cast<const uint4*>(sf + static_cast<int64_t>(r) * mn + mn4);
            word[0] |= ((v.x >> 23) & 0xffu) << (8 * j);
            word[1] |= ((v.y >> 23) & 0xffu) << (8 * j);
            word[2] |= ((v.z >> 23) & 0xffu) << (8 * j);
            word[3] |= ((v.w >> 23) & 0xffu) << (8 * j);
        }
    }
    *reinterpret_cast<uint4*>(out + static_cast<int64_t>(packed_row) * mn + mn4) = make_uint4(word[0], word[1], word[2], word[3]);
}
}  // namespace dg

int dg_pack_sf_k_grouped_ue8m0(const float* sf, int32_t* out, const int32_t* group_ks, int num_groups, int mn, int sf_k, int packed_sf_k,
                               int gran_k, int k_alignment, int use_psum, void* stream) {
    DG_CHECK(num_groups >= 0 && mn >= 0 && sf_k >= 0 && packed_sf_k >= 0);
    if (num_groups == 0 || mn == 0 || packed_sf_k == 0)
        return 0;
    DG_CHECK(sf != nullptr && out != nullptr && group_ks != nullptr);
    DG_CHECK(num_groups <= 128 && mn % 4 == 0);
    DG_CHECK(gran_k == 128 || gran_k == 32);
    DG_CHECK(k_alignment > 0 && k_alignment % 32 == 0);
    DG_CHECK(aligned16(sf) && aligned16(out));
    DG_CHECK(packed_sf_k <= 65535);
    const dim3 grid((mn / 4 + 255) / 256, packed_sf_k);
    hipLaunchKernelGGL(dg::dg_pack_sf_k_grouped_ue8m0_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), sf, out, group_ks, num_groups, mn,
                       sf_k, packed_sf_k, gran_k, k_alignment, use_psum);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_transpose_sf_fp32(const float* sf, float* out, int batches, int mn, int sf_k, void* stream) {
    DG_CHECK(batches >= 0 && mn >= 0 && sf_k >= 0);
    if (batches == 0 || mn == 0 || sf_k == 0)
        return 0;
    DG_CHECK(sf != nullptr && out != nullptr);
    DG_CHECK(batches <= 65535);
    const int aligned_mn = (mn + 3) / 4 * 4;
    if (sf_k % 4 == 0 && aligned16(sf) && sf_k / 4 <= 65535) {
        // (rows of sf_k floats behind a 16-byte aligned base: every row is 16-byte aligned)
        const dim3 grid((mn + 255) / 256, sf_k / 4, batches);
        hipLaunchKernelGGL(dg::dg_transpose_sf_fp32_vec4_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           sf, out, mn, sf_k, aligned_mn);
        DG_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const dim3 grid((mn + 63) / 64, (sf_k + 63) / 64, batches);
    hipLaunchKernelGGL(dg::dg_transpose_sf_fp32_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       sf, out, mn, sf_k, aligned_mn);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_pack_sf_ue8m0(const float* sf, int32_t* out, int batches, int mn, int sf_k,
                     int64_t sf_stride_b, int64_t sf_stride_mn, int64_t sf_stride_k, void* stream) {
    return dg_pack_sf_ue8m0_ex(sf, out, batches, mn, sf_k, sf_stride_b, sf_stride_mn, sf_stride_k, 1, nullptr, 0, 0, stream);
}

namespace {
int64_t pack_items(const dg::PackSfArgs& a) { return static_cast<int64_t>(a.blocks_mn) * ((a.sf_k + 3) / 4) * a.batches; }

int fill_pack_args(dg::PackSfArgs& a, const float* sf, int32_t* out, int batches, int mn, int sf_k, int64_t sf_stride_b,
                   int64_t sf_stride_mn, int64_t sf_stride_k, int gran_mn, const int32_t* psum_layout, int num_psum_groups,
                   int m_alignment) {
    DG_CHECK(batches >= 0 && mn >= 0 && sf_k >= 0);
    a = dg::PackSfArgs{};
    if (batches == 0 || mn == 0 || sf_k == 0)
        return 0;
    DG_CHECK(sf != nullptr && out != nullptr);
    DG_CHECK(gran_mn >= 1);
    DG_CHECK(psum_layout == nullptr || (batches == 1 && num_psum_groups > 0 && m_alignment > 0));      // smxx_layout.hpp:190-194
    a.sf = sf; a.out = out; a.mn = mn; a.sf_k = sf_k; a.aligned_mn = (mn + 3) / 4 * 4;
    a.stride_b = sf_stride_b; a.stride_mn = sf_stride_mn; a.stride_k = sf_stride_k; a.gran_mn = gran_mn;
    a.psum_layout = psum_layout; a.num_psum_groups = psum_layout != nullptr ? num_psum_groups : 0; a.m_alignment = m_alignment;
    a.blocks_mn = (mn + 255) / 256; a.batches = batches;
    DG_CHECK(pack_items(a) < (1LL << 30));
    return 0;
}
}  // namespace

int dg_pack_sf_ue8m0_ex(const float* sf, int32_t* out, int batches, int mn, int sf_k,
                        int64_t sf_stride_b, int64_t sf_stride_mn, int64_t sf_stride_k, int gran_mn,
                        const int32_t* psum_layout, int num_psum_groups, int m_alignment, void* stream) {
    dg::PackSfArgs a, none{};
    if (const int rc = fill_pack_args(a, sf, out, batches, mn, sf_k, sf_stride_b, sf_stride_mn, sf_stride_k, gran_mn, psum_layout,
                                      num_psum_groups, m_alignment); rc != 0)
        return rc;
    const int64_t grid = pack_items(a);
    if (grid == 0)
        return 0;
    hipLaunchKernelGGL(dg::dg_pack_sf_ue8m0_kernel, dim3(static_cast<unsigned>(grid)), dim3(256), 0, static_cast<hipStream_t>(stream), a, none);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_pack_sf_pair_ue8m0(const float* sfa, int32_t* out_a, int batches_a, int m, int64_t sfa_stride_b, int64_t sfa_stride_m,
                          int64_t sfa_stride_k, int gran_m, const int32_t* psum_layout, int num_psum_groups, int m_alignment,
                          const float* sfb, int32_t* out_b, int batches_b, int n, int64_t sfb_stride_b, int64_t sfb_stride_n,
                          int64_t sfb_stride_k, int gran_n, int sf_k, void* stream) {
    dg::PackSfArgs a, b;
    if (const int rc = fill_pack_args(a, sfa, out_a, batches_a, m, sf_k, sfa_stride_b, sfa_stride_m, sfa_stride_k, gran_m, psum_layout,
                                      num_psum_groups, m_alignment); rc != 0)
        return rc;
    if (const int rc = fill_pack_args(b, sfb, out_b, batches_b, n, sf_k, sfb_stride_b, sfb_stride_n, sfb_stride_k, gran_n, nullptr, 0, 0); rc != 0)
        return rc;
    const int64_t grid = pack_items(a) + pack_items(b);
    if (grid == 0)
        return 0;
    hipLaunchKernelGGL(dg::dg_pack_sf_ue8m0_kernel, dim3(static_cast<unsigned>(grid)), dim3(256), 0, static_cast<hipStream_t>(stream), a, b);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_per_token_cast_to_fp8(const void* x_bf16, void* out_fp8, float* sf, int m, int n,
                             int64_t x_stride_m, int64_t out_stride_m, int64_t sf_stride_m, int64_t sf_stride_k,
                             int use_ue8m0, void* stream) {
    DG_CHECK(m >= 0 && n >= 0);
    if (m == 0 || n == 0)
        return 0;
    DG_CHECK(x_bf16 != nullptr && out_fp8 != nullptr && sf != nullptr);
    DG_CHECK(x_stride_m >= n && out_stride_m >= n);
    const int64_t blocks = static_cast<int64_t>(m) * ((n + 127) / 128);
    // 16 blocks per 256-thread workgroup and pass; a few passes per workgroup once the chip is covered several times over
    int64_t grid = (blocks + 15) / 16;
    const int64_t cap = static_cast<int64_t>(num_cus()) * 32;
    if (grid > cap)
        grid = cap;
    hipLaunchKernelGGL(dg::dg_per_token_cast_to_fp8_kernel, dim3(static_cast<unsigned>(grid)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x_bf16),
                       static_cast<uint8_t*>(out_fp8), sf, m, n, x_stride_m, out_stride_m, sf_stride_m, sf_stride_k,
                       use_ue8m0 ? 1 : 0);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_block_cast_to_fp8(const void* x_bf16, void* out_fp8, float* sf, int rows, int cols,
                         int64_t x_stride_r, int64_t out_stride_r, int64_t sf_stride_r, int64_t sf_stride_c,
                         int per_channel, int use_ue8m0, void* stream) {
    DG_CHECK(rows >= 0 && cols >= 0);
    if (rows == 0 || cols == 0)
        return 0;
    DG_CHECK(x_bf16 != nullptr && out_fp8 != nullptr && sf != nullptr);
    DG_CHECK(x_stride_r >= cols && out_stride_r >= cols);
    DG_CHECK((rows + 127) / 128 <= 65535);
    const dim3 grid((cols + 127) / 128, (rows + 127) / 128);
    if (per_channel)
        hipLaunchKernelGGL(dg::dg_block_cast_to_fp8_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const uint16_t*>(x_bf16), static_cast<uint8_t*>(out_fp8), sf, rows, cols, x_stride_r,
                           out_stride_r, sf_stride_r, sf_stride_c, use_ue8m0 ? 1 : 0);
    else
        hipLaunchKernelGGL(dg::dg_block_cast_to_fp8_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const uint16_t*>(x_bf16), static_cast<uint8_t*>(out_fp8), sf, rows, cols, x_stride_r,
                           out_stride_r, sf_stride_r, sf_stride_c, use_ue8m0 ? 1 : 0);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_transpose_fp8(const void* src, void* dst, int batches, int rows, int cols,
                     int64_t src_ld, int64_t dst_ld, int64_t src_batch_stride, int64_t dst_batch_stride, void* stream) {
    DG_CHECK(batches >= 0 && rows >= 0 && cols >= 0);
    if (batches == 0 || rows == 0 || cols == 0)
        return 0;
    DG_CHECK(src != nullptr && dst != nullptr && src != dst);
    DG_CHECK(src_ld >= cols && dst_ld >= rows);
    DG_CHECK(batches <= 65535 && (rows + 63) / 64 <= 65535);
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64, batches);
    hipLaunchKernelGGL(dg::dg_transpose_bytes_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), rows, cols, src_ld, dst_ld,
                       src_batch_stride, dst_batch_stride);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

int dg_bf16_gemm_nt(const void* a, const void* b, void* d, int m, int n, int k, int64_t a_stride_m, int64_t b_stride_n,
                    int64_t d_stride_m, int d_dtype, int accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
    DG_CHECK(m >= 0 && n >= 0 && k >= 0);
    if (m == 0 || n == 0)
        return 0;
    DG_CHECK(k > 0);   // k == 0 is resolved by the caller (D = C or 0) without a kernel, as in the reference
    DG_CHECK(a != nullptr && b != nullptr && d != nullptr);
    DG_CHECK(k % 8 == 0);
    DG_CHECK(bf16_operand_ok(a, a_stride_m) && bf16_operand_ok(b, b_stride_n));
    DG_CHECK(a_stride_m >= k && b_stride_n >= k);
    DG_CHECK(d_dtype == DG_BF16 || d_dtype == DG_FP32);
    DG_CHECK(d_stride_m >= n);
    DG_CHECK(workspace == nullptr || (aligned16(workspace) && workspace_bytes >= 0));
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_stride_m * 2; p.a_sk = 1; p.b_sn = b_stride_n * 2; p.b_sk = 1;       // (BF16 launches: operand strides in bytes)
    p.d_sm = d_stride_m;
    p.d_dtype = d_dtype; p.accumulate = accumulate ? 1 : 0;
    p.gemm_type = dg::kNormal;
    return launch_bf16(p, 0, workspace, workspace != nullptr ? static_cast<size_t>(workspace_bytes) : 0, stream);
}

int dg_m_grouped_bf16_gemm_nt_contiguous(const void* a, const void* b, void* d, const int32_t* grouped_layout, int num_groups,
                                         int m, int n, int k, int64_t a_stride_m, int64_t b_stride_g, int64_t b_stride_n,
                                         int64_t d_stride_m, int use_psum, int m_alignment, void* stream) {
    DG_CHECK(m >= 0 && n > 0 && k > 0 && num_groups > 0);
    if (m == 0)
        return 0;
    DG_CHECK(a != nullptr && b != nullptr && d != nullptr && grouped_layout != nullptr);
    DG_CHECK(k % 8 == 0);
    DG_CHECK(bf16_operand_ok(a, a_stride_m) && bf16_operand_ok(b, b_stride_n, b_stride_g));
    DG_CHECK(a_stride_m >= k && b_stride_n >= k);
    DG_CHECK(m_alignment > 0 && m_alignment % 16 == 0);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.layout = grouped_layout;
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sm = a_stride_m * 2; p.a_sk = 1; p.b_sg = b_stride_g * 2; p.b_sn = b_stride_n * 2; p.b_sk = 1;
    p.d_sm = d_stride_m;
    p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = use_psum ? dg::kContiguousPsum : dg::kContiguous;
    p.m_alignment = m_alignment;
    return launch_bf16(p, 0, nullptr, 0, stream);
}

int dg_m_grouped_bf16_gemm_nt_masked(const void* a, const void* b, void* d, const int32_t* masked_m, int num_groups, int m_max, int n,
                                     int k, int expected_m, int64_t a_stride_g, int64_t a_stride_m, int64_t b_stride_g, int64_t b_stride_n,
                                     int64_t d_stride_g, int64_t d_stride_m, void* stream) {
    DG_CHECK(expected_m > 0 && m_max > 0 && n > 0 && k > 0 && num_groups > 0);
    DG_CHECK(a != nullptr && b != nullptr && d != nullptr && masked_m != nullptr);
    DG_CHECK(k % 8 == 0);
    DG_CHECK(bf16_operand_ok(a, a_stride_m, a_stride_g) && bf16_operand_ok(b, b_stride_n, b_stride_g));
    DG_CHECK(a_stride_m >= k && b_stride_n >= k);
    DG_CHECK(d_stride_m >= n);
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b); p.d = d;
    p.layout = masked_m;
    p.m = m_max; p.n = n; p.k = k; p.num_groups = num_groups;
    p.a_sg = a_stride_g * 2; p.a_sm = a_stride_m * 2; p.a_sk = 1;
    p.b_sg = b_stride_g * 2; p.b_sn = b_stride_n * 2; p.b_sk = 1;
    p.d_sg = d_stride_g; p.d_sm = d_stride_m;
    p.d_dtype = DG_BF16; p.accumulate = 0;
    p.gemm_type = dg::kMasked;
    return launch_bf16(p, expected_m < m_max ? expected_m : m_max, nullptr, 0, stream);
}

int dg_transpose_bf16(const void* src, void* dst, int batches, int rows, int cols,
                      int64_t src_ld, int64_t dst_ld, int64_t src_batch_stride, int64_t dst_batch_stride, void* stream) {
    DG_CHECK(batches >= 0 && rows >= 0 && cols >= 0);
    if (batches == 0 || rows == 0 || cols == 0)
        return 0;
    DG_CHECK(src != nullptr && dst != nullptr && src != dst);
    DG_CHECK(src_ld >= cols && dst_ld >= rows);
    DG_CHECK(batches <= 65535 && (rows + 63) / 64 <= 65535);
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64, batches);
    hipLaunchKernelGGL(dg::dg_transpose_bf16_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t*>(src), static_cast<uint16_t*>(dst), rows, cols, src_ld, dst_ld,
                       src_batch_stride, dst_batch_stride);
    DG_HIP_CHECK(hipGetLastError());
    return 0;
}

const char* dg_bf16_select_config(int gemm_type, int m, int n, int k, int num_groups, int expected_m, int m_alignment, int has_workspace) {
    // the BF16 kernel the automatic selection would launch for this shape (K-major, 16-byte aligned operands); nothing is launched and no
    // device is needed (256 CUs are assumed when none is visible).  has_workspace: the caller would pass one of dg_split_k_workspace_bytes().
    static thread_local std::string name;
    dg::GemmParams p{};
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups > 0 ? num_groups : 1;
    p.gemm_type = gemm_type; p.m_alignment = m_alignment;
    const Bf16Config* cfg = select_bf16_config(p, expected_m, has_workspace ? static_cast<size_t>(dg_split_k_workspace_bytes()) : 0);
    name = cfg != nullptr ? cfg->name : "";
    return name.c_str();
}

int dg_set_num_cus(int n) {
    if (n < 0)
        return fail(__FILE__, __LINE__, "num_cus >= 0");
    g_num_cus_override.store(n, std::memory_order_relaxed);
    return 0;
}

int dg_get_num_cus(void) { return num_cus(); }

void dg_reload_env(void) { g_env_knobs.store(new EnvKnobs(), std::memory_order_release); }

int dg_set_forced_config(const char* name) {
    if (name == nullptr)
        return fail(__FILE__, __LINE__, "name != nullptr");
    if (std::strcmp(name, "auto") != 0) {
        bool known = false;
        for (int i = 0; i < kNumConfigs; ++i)
            known = known || std::strcmp(name, kConfigs[i].name) == 0;
        for (const E8Config& c : kE8Configs)
            known = known || std::strcmp(name, c.name) == 0;
        known = known || bf16_config_by_name(name) != nullptr;
        if (!known) {
            g_last_error = std::string("unknown kernel configuration '") + name + "'";
            return 1;
        }
    }
    std::lock_guard<std::mutex> lock(g_forced_config_mutex);
    g_forced_config = name;
    return 0;
}

int dg_set_debug_buffer(void* device_buffer) {
    g_debug_buffer.store(static_cast<long long*>(device_buffer), std::memory_order_relaxed);
    return 0;
}

const char* dg_list_configs(void) {
    static std::string joined;
    if (joined.empty()) {
        for (int i = 0; i < kNumConfigs; ++i)
            joined += std::string(i ? "," : "") + kConfigs[i].name;
        for (const E8Config& c : kE8Configs)
            joined += std::string(",") + c.name;
        for (const Bf16Config& c : kBf16Configs)
            joined += std::string(",") + c.name;
    }
    return joined.c_str();
}

const char* dg_get_forced_config(void) {
    thread_local std::string copy;
    copy = forced_name();
    return copy.c_str();
}

const char* dg_select_config(int gemm_type, int m, int n, int k, int num_groups, int expected_m, int a_mn_major, int b_mn_major,
                             int sfb_gran_n, int m_alignment, int has_workspace, int packed_ue8m0) {
    // the kernel the automatic selection would launch for a problem of this shape with 16-byte aligned, densely packed operands and
    // MN-major SFA; nothing is launched and no device is needed (256 CUs are assumed when none is visible)
    static thread_local std::string name;
    dg::GemmParams p{};
    p.a = p.b = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(1) << 20);
    p.sfa = p.sfb = reinterpret_cast<const float*>(static_cast<uintptr_t>(1) << 21);
    p.d = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 22);
    p.m = m; p.n = n; p.k = k; p.num_groups = num_groups > 0 ? num_groups : 1;
    p.a_sm = a_mn_major ? 1 : k; p.a_sk = a_mn_major ? m : 1; p.a_sg = static_cast<int64_t>(m) * k;
    p.b_sn = b_mn_major ? 1 : k; p.b_sk = b_mn_major ? n : 1; p.b_sg = static_cast<int64_t>(n) * k;
    p.sfa_sm = 1; p.sfa_sk = (m + 3) / 4 * 4; p.sfb_sn = packed_ue8m0 || sfb_gran_n == 1 ? 1 : (k + 127) / 128;
    p.sfb_sk = packed_ue8m0 || sfb_gran_n == 1 ? (n + 3) / 4 * 4 : 1;
    p.d_sm = n; p.sfb_gran_n = sfb_gran_n; p.d_dtype = DG_BF16; p.gemm_type = gemm_type; p.m_alignment = m_alignment;
    p.sk_workspace = has_workspace ? reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 23) : nullptr;
    if (packed_ue8m0) {
        p.sfb_gran_n = 128;
        if (e8_mn_eligible(p) && e8_mn_pays(p))     // an MN-major operand read in place (otherwise the host re-majors it: the K-major choice below)
            name = e8_mn_config_name(p);
        else {
            p.a_sm = k; p.a_sk = 1; p.b_sn = k; p.b_sk = 1;
            const size_t saved = g_workspace_bytes;     // (has_workspace: of the size the host layer creates)
            g_workspace_bytes = has_workspace ? static_cast<size_t>(dg_split_k_workspace_bytes()) : 0;
            name = e8_contiguous_tabled(p) ? "e8_quad_tab_256x256"
                 : fast_eligible(p)        ? select_e8_config(p, expected_m)->name
                                           : (gemm_type == dg::kNormal && fast_eligible(p, false) ? "e8_quad_kt_128x256" : "");
            g_workspace_bytes = saved;
        }
    } else if (has_workspace && per_col_split_pieces(p, 0, true) >= 2) {
        name = per_col_eligible(p) ? (per_col_bm(p, true) == 192 ? "pipe_pc_ks_192x256" : "pipe_pc_ks_256x256") : "pipe_pc_mn_ks_256x256";     // (K pieces as the groups of one launch + the summing kernel)
    } else if (gemm_type == dg::kContiguous && m_alignment == 128 && has_workspace && !b_mn_major && sfb_gran_n == 128 && k % 128 == 0 && k >= 1024 &&
               (m + 127) / 128 <= 500 && static_cast<long>((m + 127) / 128) * ((n + 255) / 256) >= num_cus()) {
        name = "duo_tab_256x256";           // launch_contiguous_tabled: group-relative 256-row tiles + K-split remainders (_sk_: needs the workspace)
    } else {
        const int bm_must_divide = (gemm_type == dg::kContiguous || gemm_type == dg::kContiguousPsum) ? m_alignment : 0;
        const size_t saved = g_workspace_bytes;     // (has_workspace: of the size the host layer creates)
        g_workspace_bytes = has_workspace ? static_cast<size_t>(dg_split_k_workspace_bytes()) : 0;
        const Config* cfg = select_config(p, p.m, expected_m, bm_must_divide, true);
        g_workspace_bytes = saved;
        name = cfg != nullptr ? cfg->name : "";
    }
    return name.c_str();
}

int dg_dense_rowmajor_sfa_native(int m, int n, int k) {
    // would a dense call with K-major 16-byte aligned operands, per-128 SFB and a ROW-major SFA [m][ceil(k / 128)] read the SFA in place
    // (duo_p_rm_256x256)?  The host layer asks before it launches the layout step's transpose; the rule lives in select_config only.
    if (m <= 1 || n <= 0 || k <= 0 || forced_config() != "auto" || !env_knobs().sfa_rowmajor_in_place)
        return 0;
    dg::GemmParams p{};
    p.a = p.b = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(1) << 20);
    p.sfa = p.sfb = reinterpret_cast<const float*>(static_cast<uintptr_t>(1) << 21);
    p.d = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 22);
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = k; p.a_sk = 1; p.b_sn = k; p.b_sk = 1;
    p.sfa_sm = (k + 127) / 128; p.sfa_sk = 1; p.sfb_sn = (k + 127) / 128; p.sfb_sk = 1;
    p.d_sm = n; p.sfb_gran_n = 128; p.d_dtype = DG_BF16; p.gemm_type = dg::kNormal;
    const Config* cfg = select_config(p, p.m, 0, 0, true);
    return cfg != nullptr && cfg->sfa_rm ? 1 : 0;
}

int dg_dense_wants_workspace(int m, int n, int k, int a_mn_major, int b_mn_major, int sfb_gran_n) {
    // would the automatic selection cut this dense problem (16-byte aligned, densely packed operands, MN-major scales) along K if the
    // caller lent it a workspace?  The host layer asks before it creates / passes one; no model is kept on that side.
    if (m <= 0 || n <= 0 || k <= 0)
        return 0;
    dg::GemmParams p{};
    p.a = p.b = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(1) << 20);
    p.sfa = p.sfb = reinterpret_cast<const float*>(static_cast<uintptr_t>(1) << 21);
    p.d = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 22);
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_mn_major ? 1 : k; p.a_sk = a_mn_major ? m : 1;
    p.b_sn = b_mn_major ? 1 : k; p.b_sk = b_mn_major ? n : 1;
    p.sfa_sm = 1; p.sfa_sk = (m + 3) / 4 * 4; p.sfb_sn = sfb_gran_n == 1 ? 1 : (k + 127) / 128; p.sfb_sk = sfb_gran_n == 1 ? (n + 3) / 4 * 4 : 1;
    p.d_sm = n; p.sfb_gran_n = sfb_gran_n; p.d_dtype = DG_BF16; p.gemm_type = dg::kNormal;
    p.sk_workspace = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 23);
    if (per_col_split_pieces(p, 0, true) >= 2)
        return 1;
    {   // (a K-split form forced by name -- tuning runs, tests -- gets the buffer too)
        const std::string forced = forced_config();
        if (forced.find("_sk_") != std::string::npos || forced.find("_ks_") != std::string::npos)
            return 1;
    }
    const size_t saved = g_workspace_bytes;         // (the question is asked BEFORE a workspace exists: assume the size the host layer creates)
    g_workspace_bytes = static_cast<size_t>(dg_split_k_workspace_bytes());
    const Config* cfg = select_config(p, p.m, 0, 0, true);
    g_workspace_bytes = saved;
    return cfg != nullptr && cfg->split_k ? 1 : 0;
}

int dg_operand_plan(int gemm_type, const void* a, const void* b, int m, int n, int k, int64_t a_sm, int64_t a_sk, int64_t b_sn,
                    int64_t b_sk, int64_t b_sg, int64_t sfa_sm, int sfb_gran_n, int m_alignment) {
    // Which MN-major FP8 operands the caller should re-major into K-major scratch before the launch (bit 0: A, bit 1: B), decided
    // with the very predicates select_config() / launch_gemm() apply, so that an operand left as it is always finds its kernel.
    const bool a_mn = a_sk != 1, b_mn = b_sk != 1;
    const int all = (a_mn ? 1 : 0) | (b_mn ? 2 : 0);
    if (all == 0)
        return 0;
    if (const std::string forced = forced_config(); forced != "auto") {
        // a forced configuration (tuning runs, A/B scripts) is not bound by the automatic predicates below: it gets the operand forms
        // its own name asks for -- MN-major B for *_bmn_*, MN-major A for *_amn_*, both for *_abmn_* / pipe_pc_mn_* -- and K-major
        // operands (which every other configuration takes) otherwise
        if (forced.find("_abmn") != std::string::npos || forced.find("pc_mn") != std::string::npos)
            return 0;
        if (forced.find("_bmn") != std::string::npos)
            return all & 1;
        if (forced.find("_amn") != std::string::npos)
            return all & 2;
        return all;
    }
    const uint8_t* scratch = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(1) << 20);    // (a fresh allocation: aligned, dense)
    dg::GemmParams p{};
    p.a = static_cast<const uint8_t*>(a); p.b = static_cast<const uint8_t*>(b);
    p.sfa = p.sfb = reinterpret_cast<const float*>(static_cast<uintptr_t>(1) << 21);
    p.m = m; p.n = n; p.k = k; p.num_groups = 1;
    p.a_sm = a_sm; p.a_sk = a_sk; p.b_sn = b_sn; p.b_sk = b_sk; p.b_sg = b_sg;
    p.sfa_sm = sfa_sm; p.sfa_sk = (m + 3) / 4 * 4; p.sfb_sn = 1; p.sfb_sk = (n + 3) / 4 * 4;
    p.sfb_gran_n = sfb_gran_n; p.gemm_type = gemm_type; p.m_alignment = m_alignment;
    if (gemm_type != dg::kNormal)       // contiguous layouts: A is K-major by contract; B as it is when the B_MN kernels take it
        return (b_mn && bmn_eligible(p) && m > 256 && m_alignment % 128 == 0) ? 0 : all;
    if (sfb_gran_n == 1)                // recipe (1, 1, 128): the transpose-read kernel wants BOTH operands MN-major
        return (a_mn && b_mn && per_col_mn_eligible(p) && m > 64) ? 0 : all;
    if (sfb_gran_n != 128 || sfa_sm != 1)
        return all;
    if (a_mn && m > 256) {
        // The MN-major-A kernels exist for 256 x 256 tiles only and are never K-split: a problem whose 256 x 256 tiles cover at most
        // half the chip while the K loop is long (wgrad of a narrow layer: 576 x 4096 x 7168 = 48 tiles) is better served by
        // re-majoring A (a few microseconds) and the 128 x 256 tiles of the K-major-A kernels, which the K split spreads out.
        const bool few_tiles_long_k = static_cast<long>(ceil_div(m, 256)) * ceil_div(n, 256) * 2 <= num_cus() && k >= 2048;
        if (!few_tiles_long_k) {
            if (amn_eligible(p))
                return 0;
            dg::GemmParams q = p;       // B re-majored
            q.b = scratch; q.b_sn = k; q.b_sk = 1;
            if (b_mn && amn_eligible(q))
                return 2;
        }
    }
    dg::GemmParams q = p;               // A K-major (as given, or re-majored)
    if (a_mn) { q.a = scratch; q.a_sm = k; q.a_sk = 1; }
    if (b_mn && bmn_eligible(q) && m > 256)
        return a_mn ? 1 : 0;
    return all;
}

const char* dg_last_config(void) { return g_last_config.c_str(); }
const char* dg_last_error(void) { return g_last_error.c_str(); }
const char* dg_version(void) { return "deepgemm_amd 0.1.0 (gfx950)"; }

}  // extern "C"
