// conv_dma_ragged.hip -- the RAGGED instantiations of the LDS-DMA pipelined convolution (conv_dma_kernel.h): launches whose
// contraction per tap is a multiple of 8 channels but not of 64.  In the training step those are data gradients, whose contraction
// is the layer's OUTPUT width: the three 72-channel deformable offset layers (20 480 pixels x 512 <- 72, 3 x 3 dilation 2: 18
// K-steps), the RPN heads and the R-CNN heads.  Only the configurations such launches are planned onto exist here
// (conv_dma_ragged_cfg); the whole-tap instantiations of conv_dma.hip are untouched.
#include "conv_dma_kernel.h"

// the configuration a ragged launch runs for the planner's (or a forced) choice `cfg`: 64 x 128 two-stage (6) for the narrow
// and single-step launches, the 160 x 128 pair (14 forward / 16 data gradient) for everything else
int conv_dma_ragged_cfg(int cfg, bool dgrad) {
  if (cfg == 4 || cfg == 5 || cfg == 6) return 6;
  return dgrad ? 16 : 14;
}

int conv_dma_ragged_launch(const ConvParams &p, bool dgrad, int cfg, hipStream_t s) {
  SN_REQUIRE(cfg == conv_dma_ragged_cfg(cfg, dgrad), "conv_dma_ragged_launch: configuration %d is not instantiated", cfg);
  if (cfg == 6) {
    if (dgrad) launch_config<true, 6, true>(p, s);
    else launch_config<false, 6, true>(p, s);
  } else if (dgrad) {
    launch_config<true, 16, true>(p, s);
  } else {
    launch_config<false, 14, true>(p, s);
  }
  SN_CHECK_LAUNCH();
  return SN_OK;
}
