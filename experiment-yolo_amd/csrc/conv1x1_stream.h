// Host interface of the streaming 1x1 convolution (conv1x1_stream.hip); conv.hip selects it in conv_forward_impl.
#pragma once
#include "common.h"
#include "dealyolo_hip.h"

#define DY_STREAM_MAX_KSTEPS 4  // 32-channel k-steps whose A fragments a wave keeps in registers (Cin <= 128)

struct Conv1x1StreamArgs {
  const f16* w;     // packed weights (dy_pack_weights*: [cout group][k-step][16*MT rows][32])
  void* y;          // (npix, ldy) fp16; unused with a segmented output
  double* acc;      // DY_EPI_STATS | DY_EPI_STATS_ACC: [DY_BN_COPIES][2][round16(cout)]
  int ldy, npix, cout, epi;
  int pp_grid;      // launches with statistics: workgroups the ping-pong kernel would run this launch with (pp_grid, conv.hip)
  int cpk;          // real channels per 32-wide k-step: 32, or 16 (16-channel chunks: the upper half of the step is zero weights)
  int N, H, W;      // the map (an up-sampled input segment reads pixel (n, y >> 1, x >> 1) of a (N, H/2, W/2) tensor)
  DySegs xs;        // the input, always as segments (a plain tensor is one segment)
  DySegs ys;        // nseg > 0: the output is a segmented concatenation, stored or added per segment
};

// 1 when an instantiation exists for this many k-steps and this cout-group width
int conv1x1_stream_has(int nks, int mt);
// launches conv1x1_stream_kernel<nks, mt> over `ngroups` cout groups
int conv1x1_stream_launch(const Conv1x1StreamArgs& a, int nks, int mt, int ngroups, hipStream_t stream);
