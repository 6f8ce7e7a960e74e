// Space-to-depth of SPDConv (reference nn/extra_modules/block.py:2504-2507):
//   torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
// on NHWC fp16 tensors addressed as (pointer, pixel stride):  y[n, i, j, (a + 2b) C + k] = x[n, 2i + a, 2j + b, k], a = row parity,
// b = column parity -- the reference's channel order, so the 3x3 conv behind it keeps its weights in state_dict order.  A pure
// permutation: the backward moves the same bytes the other way (and adds where the gradient has another writer already).
// One 16-byte piece (8 channels) per work item; consecutive lanes take consecutive pieces of an OUTPUT pixel, so a wave writes
// contiguous bytes of y and touches two contiguous spans of x (rows 2i and 2i + 1, pixels 2j and 2j + 1 side by side).  No LDS, every
// element offset is 64-bit, and nothing outside the C (4C) channels of either operand is read or written: both may be channel slices
// of wider tensors.
#include "common.h"
#include "dealyolo_hip.h"

struct SpdArgs {
  f16* x;  // (n, H, W, C) at pixel stride ldx
  f16* y;  // (n, H/2, W/2, 4C) at pixel stride ldy
  int ldx, ldy, C, N, Ho, Wo;  // Ho, Wo: extent of y
};

// MODE 0: y <- x;  1: x <- y (gradient store);  2: x += y (gradient fan-in, one fp16 addition per element)
template <int MODE>
__global__ __launch_bounds__(256) void spd_kernel(SpdArgs s) {
  const int cpp = s.C >> 3, ppp = 4 * cpp;  // pieces per parity group / per output pixel
  const long total = (long)s.N * s.Ho * s.Wo * ppp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / ppp;
    const int q = (int)(idx - pix * ppp);
    const int g = q / cpp, c0 = (q - g * cpp) * 8;  // g = a + 2b
    const int j = (int)(pix % s.Wo);
    const long t = pix / s.Wo;
    const int i = (int)(t % s.Ho);
    const long n = t / s.Ho;
    const long src = (n * (2 * s.Ho) + 2 * i + (g & 1)) * (2L * s.Wo) + 2 * j + (g >> 1);
    f16* px = s.x + src * s.ldx + c0;
    f16* py = s.y + pix * s.ldy + (long)g * s.C + c0;
    if (MODE == 0) {
      *reinterpret_cast<uint4*>(py) = *reinterpret_cast<const uint4*>(px);
    } else if (MODE == 1) {
      *reinterpret_cast<uint4*>(px) = *reinterpret_cast<const uint4*>(py);
    } else {
      const half8 d = *reinterpret_cast<const half8*>(py), o = *reinterpret_cast<const half8*>(px);
      half8 r;
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = (f16)((float)o[k] + (float)d[k]);
      *reinterpret_cast<half8*>(px) = r;
    }
  }
}

extern "C" int dy_space_to_depth(void* x, int ldx, void* y, int ldy, int n, int h, int w, int C, int backward, int accumulate,
                                 hipStream_t stream) {
  if (!x || !y || n < 1 || C < 8 || h < 2 || w < 2 || (h & 1) || (w & 1)) return DY_ERR_ARG;
  if ((C & 7) || (ldx & 7) || (ldy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return DY_ERR_ALIGN;
  if (ldx < C || (long)ldy < 4L * C) return DY_ERR_ARG;
  SpdArgs s{(f16*)x, (f16*)y, ldx, ldy, C, n, h >> 1, w >> 1};
  long blocks = ((long)n * h * w * (C >> 3) + 255) / 256;  // as many pieces as x has
  if (blocks > 8192) blocks = 8192;
  const dim3 grid((unsigned)blocks), block(256);
  if (!backward)
    hipLaunchKernelGGL(spd_kernel<0>, grid, block, 0, stream, s);
  else if (!accumulate)
    hipLaunchKernelGGL(spd_kernel<1>, grid, block, 0, stream, s);
  else
    hipLaunchKernelGGL(spd_kernel<2>, grid, block, 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
