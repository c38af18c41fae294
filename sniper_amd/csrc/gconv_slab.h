// gconv_slab.h -- launch shape and LDS image geometry of the 32-channel-slab MFMA kernels, shared by the grouped convolution
// (gconv.hip) and the grouped deformable convolution (gdeform.hip).  Internal, not part of the C ABI.
#pragma once
#include "common.h"

constexpr int kTP = 40;       // halfs per row of a [32 pixels][32 channels] LDS image (80 B: 16-byte aligned rows)

// tr_frag (conv_common.h) on these images: rows = pixels 8q + {0..3} and 8q + {4..7} -- the second read is 4 rows down -- columns =
// the 16 channels of a block: lane (r, q) receives channel r of pixels 8q .. 8q + 7.
constexpr int kTrSecond = 4 * kTP;

// waves per workgroup: every wave of a workgroup owns a slab that exists
static inline int gc_waves(int nslab) { return nslab % 4 == 0 ? 4 : (nslab % 2 == 0 ? 2 : 1); }

// weight gradient over M pixels in 32-pixel chunks: -> pixel blocks (= partial slabs in the workspace), chunks per block
static inline int gc_chunk_blocks(long M, int nslab, int *per_block) {
  const int gy = nslab / gc_waves(nslab);
  const long chunks = (M + 31) / 32;
  long blocks = sn_div_up(512, gy);               // about two workgroups per CU
  if (blocks > chunks) blocks = chunks;
  *per_block = (int)((chunks + blocks - 1) / blocks);
  return (int)((chunks + *per_block - 1) / *per_block);
}
