// conv_dma.hip -- the LDS-DMA pipelined implicit-GEMM convolution (kernel template and configuration table: conv_dma_kernel.h):
// the launches of the whole-64-channel-tap instantiations, forward and data gradient of each.  A launch whose Cin is not a multiple
// of 64 goes to conv_dma_ragged.hip.
#include "conv_dma_kernel.h"

ConvDmaConfig conv_dma_config(int cfg) { return (cfg >= 1 && cfg <= kConvDmaConfigs) ? kCfg[cfg] : kCfg[0]; }

template <bool DGRAD>
static int launch_cfg(const ConvParams &p, int cfg, hipStream_t s) {
  switch (cfg) {
    case 4: launch_config<DGRAD, 4>(p, s); break;
    case 5: launch_config<DGRAD, 5>(p, s); break;
    case 6: launch_config<DGRAD, 6>(p, s); break;
    case 7: launch_config<DGRAD, 7>(p, s); break;
    case 14: launch_config<DGRAD, 14>(p, s); break;
    case 16: launch_config<DGRAD, 16>(p, s); break;
    case 18: launch_config<DGRAD, 18>(p, s); break;
    case 24: launch_config<DGRAD, 24>(p, s); break;
    case 26: launch_config<DGRAD, 26>(p, s); break;
    default: SN_REQUIRE(false, "conv_dma_launch: unknown configuration %d", cfg);
  }
  SN_CHECK_LAUNCH();
  return SN_OK;
}

// diagnostics: phase timeline of the next launches' workgroups into buf (>= 8 x grid 64-bit words; tools/conv_trace.py), NULL = off
static std::atomic<unsigned long long *> g_conv_trace{nullptr};
void conv_dma_set_trace(unsigned long long *buf) { g_conv_trace.store(buf, std::memory_order_relaxed); }

int conv_dma_launch(const ConvParams &p, bool dgrad, int cfg, hipStream_t s) {
  ConvParams q = p;
  q.trace = g_conv_trace.load(std::memory_order_relaxed);
  if (p.Cin % 64 != 0) return conv_dma_ragged_launch(q, dgrad, cfg, s);
  return dgrad ? launch_cfg<true>(q, cfg, s) : launch_cfg<false>(q, cfg, s);
}
