// conv_dma_kernel.h -- the kernel template of conv_dma.hip (whole-64-channel taps) and conv_dma_ragged.hip (RAGGED: the last
// K-step of a tap is partial): implicit-GEMM convolution (forward and data gradient) whose operand tiles travel HBM/L2 -> LDS by
// LDS-DMA (buffer_load_dwordx4 ... lds) instead of through registers.
//
// Same GEMM view, data layout and epilogue as conv_igemm_p2_kernel (conv.hip; call sites
// symbols/faster/resnet_mx_101_e2e.py:43-66,121-155,256,288-303): Y[m][n] = sum_{tap,c} A(m,tap,c) * Wt[n][tap][c],
// channels-last fp16, BK = 64 channels per K-step, 128-byte LDS rows whose 16-byte slots are XOR-swizzled with (row & 7).
// What changes is the staging pipeline, which is what bounded the register-staged kernel (8
// ds_write_b128 per thread per K-step on the LDS store path ~ the time of the step's MFMAs, 64 staging VGPRs):
//
//   * one LDS-DMA instruction moves 8 tile rows x 128 B: lane l supplies the global address of row (l >> 3), 16-byte chunk
//     (l & 7) ^ (l >> 3), and the hardware writes lane l's 16 bytes at (wave-uniform base) + 16 l -- i.e. the swizzle
//     is applied on the SOURCE side and the LDS image is the one the fragment reads expect.  Out-of-range voffsets
//     (padding taps, rows beyond M / Nout) deliver zeros, as with the register loads.
//   * no ds_write, no staging registers, no VALU on the load path except the per-tap voffset update;
//   * an S-deep ring of stages: in iteration t the stage t+S-1 is issued right after the barrier that retires stage t, so
//     S-1 stages are in flight under every compute phase, one barrier per K-step, counted s_waitcnt vmcnt (never 0 in
//     the steady state for S > 2).  The whole LDS footprint is ONE __shared__ array: with two, hipcc orders every
//     LDS-DMA against every later ds_read with vmcnt(0) (cdna_hip_programming.md section 5, trap (a)), which is what made
//     round 1's attempt a no-gain.
//
// The tile shape is a template parameter set (BM x BN outputs, WMW x WNW waves, S stages); conv_plan() in conv.hip picks
// one per layer from the measured table (tools/conv_tune.py).  Nine configurations are instantiated (kCfg below).
#pragma once
#include "conv_common.h"
#include <type_traits>

// sum over the 16 lanes of a DPP row (the lanes that share lane >> 4), result in every lane: four VALU adds with DPP operands
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) instead of four ds_bpermute round trips per value
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror: lane i <-> 7 - i of its half row (the other quad)
  return dpp_add<0x140>(v);   // row_mirror: lane i <-> 15 - i (the other half row)
}

// 16-byte global load the compiler's wait-count pass does not see (PERSIST: the next tile's residual rows are requested behind one
// tile's epilogue and consumed in the next one's; tracked loads in flight across the tile loop's back edge make hipcc drain the
// whole queue -- vmcnt(0) -- wherever it is unsure, and loads return in order).  The consumer waits by hand: wait_vmcnt + tie().
__device__ __forceinline__ half8 load16_untracked(const half_t *ptr) {
  floatx4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(ptr) : "memory");
  return __builtin_bit_cast(half8, v);
}
// 16-byte LDS read the wait-count pass does not see either: a tracked ds_read of an LDS range an LDS-DMA wrote earlier gets a vmcnt
// wait in front of it (the pass cannot know that DMA was waited for by hand), which in the epilogue means waiting for the stores
__device__ __forceinline__ floatx4 lds_read16_untracked(const void *ptr) {
  floatx4 v;
  const unsigned a = (unsigned)(unsigned long)(lds_ptr_t)const_cast<void *>(ptr);
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ void tie(floatx4 &v) { asm volatile("" : "+v"(v)); }
// orders later uses of x behind the asm statements in front of this one (an s_waitcnt): x is "redefined" here
__device__ __forceinline__ void tie(half8 &x) {
  floatx4 v = __builtin_bit_cast(floatx4, x);
  asm volatile("" : "+v"(v));
  x = __builtin_bit_cast(half8, v);
}

// PS ("producer / consumer specialised", round 3): the workgroup has WMW x WNW CONSUMER waves (one per SIMD for 2 x 2) that only read
// fragments and multiply, plus four PRODUCER waves (the second wave of each SIMD) that only compute gather addresses and issue the
// LDS-DMA pieces, S - 1 stages ahead.  A wave's instruction stream is in order, so in the unspecialised kernel a K-step costs
// DMA issue (~70 cycles per piece) PLUS the MFMAs (tools/probes/dma_rate_probe.hip); with the two jobs in different waves a step
// costs the longer of the two (the same split made the weight gradient's K loop 2x faster: conv_wgrad_ps.hip).  The consumers keep
// the two 32-channel halves of a K-step in two register sets; the step's barrier sits between the two MFMA blocks and every set is
// re-read for the next half right behind the block that used it, so no step begins with barrier -> ds_read -> wait.
//
// PERSIST (round 6): the workgroup walks `tpw` output tiles (tile b, b + G, b + 2 G, ... of the XCD-ordered list, G = the grid) as ONE
// pipeline: the stage ring does not drain at a tile boundary -- the last K-step of tile k issues the first stage of tile k + 1, which
// lands under that step's MFMAs, and the residual / BatchNorm-input tile of k + 1 is requested from inside the epilogue of k (each
// register group right after the epilogue consumed it), so the fill that every workgroup of the one-tile-per-workgroup launch pays
// in front of its first MFMA (profiles/r05_conv_trace_s3.txt: 8 of a workgroup's 28 thousand cycles on the 4-K-step layers, more
// with a cold residual) is paid once per workgroup instead of once per tile.  Taken for launches of >= 4 tiles per CU whose tile
// count divides over the 512 resident workgroups (conv_dma_choice_balanced: the stage-3 expansions forward, the reductions' data gradients,
// stages 2 and 4).  The statistics scratch sits behind the ring (the ring is live while a tile's statistics are reduced).
//
// RAGGED (conv_dma_ragged.hip): Cin is a multiple of 8 but not of 64 (the data gradient of a 72-channel offset layer contracts
// over 72 channels per tap).  A tap then has kpt = ceil(Cin / 64) K-steps and its last one covers channels [64 (kpt - 1), Cin): the
// lanes whose 16-byte chunk lies at or beyond Cin would fetch the next tap's weights and the next pixel's (or the row padding's)
// activations, so for that step they carry an out-of-range voffset and the buffer range check zero-fills BOTH operands (the device
// of conv_wgrad_ps.hip's kPoison).  Every lane keeps two offsets per piece, "full" and "last", chosen per step by a uniform
// branch around the issue loop; LDS image, swizzle, fragment reads and MFMA schedule are those of the whole-tap kernel.
// The body (conv_dma_body.h) is included into both entry points: conv_dma_kernel keeps the template arguments, hence the symbol
// names and the code, it always had; conv_dma_ragged_kernel is the same text with RAGGED = true.
template <bool DGRAD, int BM, int BN, int WMW, int WNW, int S, int MINW, bool PS = false, bool PERSIST = false>
__global__ __launch_bounds__(64 * (WMW * WNW + (PS ? 4 : 0)), MINW) void conv_dma_kernel(const ConvParams p, int mtiles, int ntiles) {
  constexpr bool RAGGED = false;
#include "conv_dma_body.h"
}
template <bool DGRAD, int BM, int BN, int WMW, int WNW, int S, int MINW, bool PS = false, bool PERSIST = false>
__global__ __launch_bounds__(64 * (WMW * WNW + (PS ? 4 : 0)), MINW) void conv_dma_ragged_kernel(const ConvParams p, int mtiles, int ntiles) {
  constexpr bool RAGGED = true;
#include "conv_dma_body.h"
}

template <bool DGRAD, int BM, int BN, int WMW, int WNW, int S, int MINW, bool PS = false, bool PERSIST = false, bool RAGGED = false>
static void launch_one(const ConvParams &p, hipStream_t s) {
  const int mtiles = (DGRAD && !PS && p.cls && BM * BN <= 160 * 128) ? 4 * sn_div_up(p.cls_mc, BM) : sn_div_up(p.M, BM), ntiles = sn_div_up(p.Nout, BN);
  const int base = sn_div_up(mtiles, 8) * 8 * ntiles;
  ConvParams q = p;
  q.ksplit_grid = base;
  if constexpr (PERSIST) {
    q.tiles_per_wg = conv_persist_tiles_per_wg(p.M, p.Nout, BM, BN);      // (conv_plan chose this configuration only where it is > 0)
    q.ksplit = 1;
    hipLaunchKernelGGL((conv_dma_kernel<DGRAD, BM, BN, WMW, WNW, S, MINW, PS, true>), dim3((unsigned)(base / q.tiles_per_wg)),
                       dim3(64 * WMW * WNW), 0, s, q, mtiles, ntiles);
  } else {
    const dim3 grid((unsigned)base * (unsigned)((!DGRAD && p.ksplit > 1 && BM * BN <= 160 * 128) ? p.ksplit : 1));
    const dim3 block(64 * (WMW * WNW + (PS ? 4 : 0)));
    if constexpr (RAGGED) hipLaunchKernelGGL((conv_dma_ragged_kernel<DGRAD, BM, BN, WMW, WNW, S, MINW, PS>), grid, block, 0, s, q, mtiles, ntiles);
    else hipLaunchKernelGGL((conv_dma_kernel<DGRAD, BM, BN, WMW, WNW, S, MINW, PS>), grid, block, 0, s, q, mtiles, ntiles);
  }
}


// cfg -> tile shape.  LDS = stages * (bm + bn) * 128 B.  The numbers are those of round 2's seventeen-entry table (profiles/r02_conv_tune*.txt
// name them); the entries no selection rule and no whole-step A/B ever chose were removed in round 3 (bm = 0: no such configuration).
constexpr ConvDmaConfig kCfg[kConvDmaConfigs + 1] = {
    {0, 0, 0, 0, 0},
    {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0},
    {128, 256, 512, 3, 3 * 384 * 128},   // 4: 144 KB, 8 waves: FullyConnected over 6000 RoIs with >= 1024 outputs
    {64, 128, 256, 3, 3 * 192 * 128},    // 5: 72 KB, 2 / CU, wave tile 32 x 64: narrow heads, long contractions
    {64, 128, 256, 2, 2 * 192 * 128},    // 6: 48 KB, 3 / CU: narrow heads, FC, single-K-step layers
    {256, 256, 512, 2, 2 * 512 * 128},   // 7: 128 KB, wave tile 64 x 128: >= 3.75 tiles of 256 x 256 per CU
    {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0},
    // 160-row tiles: 20 480 pixels (20 chips x 32 x 32) = 128 row tiles, i.e. 256 / 512 / 1024 workgroups for 256 / 512 / 1024
    // output channels -- whole multiples of the 256 CUs
    {160, 128, 256, 2, 2 * 288 * 128},   // 14: 72 KB, 4 waves, 2 workgroups / CU (forward default)
    {0, 0, 0, 0, 0},
    {160, 128, 512, 2, 2 * 288 * 128},   // 16: 8 waves (2 x 4), wave tile 80 x 32, 2 workgroups / CU (data-gradient default)
    {0, 0, 0, 0, 0},
    // producer / consumer specialised (round 3): 4 multiplying waves (2 x 2) + 4 staging waves, one workgroup per CU
    {160, 128, 512, 4, 4 * 288 * 128},   // 18: 144 KB, wave tile 80 x 64: long contractions with about one tile per CU
    {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0},
    // persistent tile loop (round 6; PERSIST in conv_dma_kernel): 512 workgroups walk tiles / 512 tiles each as one pipeline
    {160, 128, 256, 2, 2 * 288 * 128 + 2048},   // 24: 14's shape (forward)
    {0, 0, 0, 0, 0},
    {160, 128, 512, 2, 2 * 288 * 128 + 2048 + 3072},   // 26: 16's shape (data gradient; + the BatchNorm coefficients' 3 KB)
};

// cfg -> template arguments: the one table both translation units launch from, held against kCfg at compile time
template <bool DGRAD, int CFG, bool RAGGED, int BM, int BN, int WMW, int WNW, int S, int MINW, bool PS = false, bool PERSIST = false>
static void launch_checked(const ConvParams &p, hipStream_t s) {
  static_assert(kCfg[CFG].bm == BM && kCfg[CFG].bn == BN && kCfg[CFG].threads == 64 * (WMW * WNW + (PS ? 4 : 0)) && kCfg[CFG].stages == S &&
                    kCfg[CFG].lds_bytes >= S * (BM + BN) * 128,
                "kCfg and the template arguments of a configuration disagree");
  launch_one<DGRAD, BM, BN, WMW, WNW, S, MINW, PS, PERSIST, RAGGED>(p, s);
}
template <bool DGRAD, int CFG, bool RAGGED = false>
static void launch_config(const ConvParams &p, hipStream_t s) {
  if constexpr (CFG == 4) launch_checked<DGRAD, CFG, RAGGED, 128, 256, 2, 4, 3, 2>(p, s);
  else if constexpr (CFG == 5) launch_checked<DGRAD, CFG, RAGGED, 64, 128, 2, 2, 3, 2>(p, s);
  else if constexpr (CFG == 6) launch_checked<DGRAD, CFG, RAGGED, 64, 128, 2, 2, 2, 3>(p, s);
  else if constexpr (CFG == 7) launch_checked<DGRAD, CFG, RAGGED, 256, 256, 4, 2, 2, 1>(p, s);
  else if constexpr (CFG == 14) launch_checked<DGRAD, CFG, RAGGED, 160, 128, 2, 2, 2, 2>(p, s);
  else if constexpr (CFG == 16) launch_checked<DGRAD, CFG, RAGGED, 160, 128, 2, 4, 2, 2>(p, s);
  else if constexpr (CFG == 18) launch_checked<DGRAD, CFG, RAGGED, 160, 128, 2, 2, 4, 1, true>(p, s);
  else if constexpr (CFG == 24) launch_checked<DGRAD, CFG, false, 160, 128, 2, 2, 2, 2, false, true>(p, s);
  else if constexpr (CFG == 26) launch_checked<DGRAD, CFG, false, 160, 128, 2, 4, 2, 4, false, true>(p, s);
  else static_assert(CFG < 0, "no such configuration");
}
