// GSConv's channel shuffle (reference nn/extra_modules/block.py:896-908) and its autograd, on NHWC fp16 tensors addressed as
// (pointer, pixel stride).  With x2 = cat(x1, d) of 2 c_ channels (x1 = cv1's output, d = the depthwise cv2's output, c_ each), the
// reference's reshape / permute / reshape / cat chain is exactly
//   y = cat(x2[:, 0::2], x2[:, 1::2])          y[j] = x2[2 j],  y[c_ + j] = x2[2 j + 1],  j < c_
// -- all even channels of x2, then all odd ones.  x2 is never built: the kernels read x1 and d where they are.
// x2 is viewed as c_ / 8 groups of 16 consecutive channels; group q is the source granules 2 q and 2 q + 1 of the virtual
// concatenation [x1 | d]: granule g < c_ / 8 is channels 8 g .. 8 g + 7 of x1, any other channels 8 (g - c_ / 8) .. of d.  With
// c_ % 16 == 8 the middle group (q = c_ / 16, rounded down) takes its first granule from x1 and its second from d; c_ == 8 has that
// group alone.  The group's 8 even channels are output granule q, its 8 odd ones output granule q + c_ / 8.
// Forward work item = (pixel, OUTPUT granule), granule fastest: two 16-byte loads (both granules of the group; the item of the
// group's other output granule, gpp lanes on, loads the same two), one 16-byte store -- consecutive lanes store consecutive granules.
// (The first form, one item per (pixel, group) with two loads and two stores, stored runs of 2 c_ bytes per instruction and was
// further from a copy of the same bytes than this one: the measurements of both are in profiles/r24_slimneck.md.)
// Backward, the inverse interleave: a work item reads granules q and q + c_ / 8 of dy and writes ONE source granule's gradient (the
// first or the second half of the group).  Each of the two destinations (dx1, dd) is stored, or -- its accumulate flag set -- written
// as fp16(old + v) with one fp32 addition; a null destination is skipped (the tensor needs no gradient), both null launches nothing.
// Pure data movement: no arithmetic in the forward, no atomics anywhere, two runs give the same bits.  Every element offset is
// 64-bit; nothing outside the c_ channels of an operand (2 c_ of y / dy) is read or written, so every operand may be a channel slice
// of a wider tensor.  Grid-stride loop over a capped grid, as fusion_fwd_kernel.
#include "common.h"
#include "dealyolo_hip.h"

#define GS_MAX_BLOCKS 4096  // 256 work items each: a launch of more than 2^20 granules to store loops

// the 8 channels of source granule g (of [x1 | d]) at pixel ``pix``
static __device__ __forceinline__ const f16* gs_src(const f16* x1, int ld1, const f16* d, int ldd, long pix, int g, int gpp) {
  return g < gpp ? x1 + pix * ld1 + g * 8 : d + pix * ldd + (g - gpp) * 8;
}

// Work item = (pixel, OUTPUT granule j), j < 2 gpp fastest: j < gpp holds the even channels of group q = j, any other the odd channels
// of group q = j - gpp.  Consecutive lanes store consecutive 16-byte granules of y.
__global__ __launch_bounds__(256) void gs_shuffle_fwd_kernel(const f16* __restrict__ x1, int ld1, const f16* __restrict__ d, int ldd,
                                                             f16* __restrict__ y, int ldy, long total, int gpp) {
  const int opp = 2 * gpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / opp;
    const int j = (int)(idx - pix * opp);
    const int odd = j >= gpp, q = odd ? j - gpp : j;
    const half8 a = *reinterpret_cast<const half8*>(gs_src(x1, ld1, d, ldd, pix, 2 * q, gpp));
    const half8 b = *reinterpret_cast<const half8*>(gs_src(x1, ld1, d, ldd, pix, 2 * q + 1, gpp));
    const half8 e = {a[0], a[2], a[4], a[6], b[0], b[2], b[4], b[6]};
    const half8 o = {a[1], a[3], a[5], a[7], b[1], b[3], b[5], b[7]};
    *reinterpret_cast<half8*>(y + pix * ldy + j * 8) = odd ? o : e;
  }
}

// Work item = (destination, pixel, SOURCE granule g of that destination), g < gpp fastest, the pixels of dx1 before those of dd:
// consecutive lanes store (or add to) consecutive 16-byte granules of one gradient tensor.  ``first`` / ``nside``: which destinations
// the launch covers (a null one is left out of the index range).  ``pixmajor`` (both destinations, c_ == 8: the one group straddles
// them, so BOTH sides read the same two granules of dy): work item = (pixel, destination) instead, the two readers of a pixel's dy
// side by side in one wave and dy read from memory once; each tensor still receives consecutive granules.  Source granule G = g
// (dx1) or gpp + g (dd) of [x1 | d] belongs to group q = G / 2 and is its first (G even) or second (G odd) half: channels 0..3 or 4..7 of the group's even and odd granules of dy.
__global__ __launch_bounds__(256) void gs_shuffle_bwd_kernel(const f16* __restrict__ dy, int ldy, f16* dx1, int ld1, int acc1, f16* dd,
                                                             int ldd, int accd, long per_side, int first, int nside, int pixmajor, int gpp) {
  const long total = per_side * nside;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int side, g;
    long pix;
    if (pixmajor) {  // (gpp == 1, nside == 2)
      pix = idx >> 1, side = (int)(idx & 1), g = 0;
    } else {
      side = first + (idx >= per_side ? 1 : 0);
      const long r = idx >= per_side ? idx - per_side : idx;
      pix = r / gpp;
      g = (int)(r - pix * gpp);
    }
    const int G = side ? gpp + g : g, q = G >> 1;
    const f16* src = dy + pix * ldy + q * 8;
    const half8 e = *reinterpret_cast<const half8*>(src);
    const half8 o = *reinterpret_cast<const half8*>(src + gpp * 8);
    const half8 lo = {e[0], o[0], e[1], o[1], e[2], o[2], e[3], o[3]};
    const half8 hi = {e[4], o[4], e[5], o[5], e[6], o[6], e[7], o[7]};
    half8 v = (G & 1) ? hi : lo;
    f16* dst = side ? dd + pix * ldd + g * 8 : dx1 + pix * ld1 + g * 8;
    if (side ? accd : acc1) {
      const half8 old = *reinterpret_cast<const half8*>(dst);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (f16)((float)old[k] + (float)v[k]);
    }
    *reinterpret_cast<half8*>(dst) = v;
  }
}

static inline unsigned gs_grid(long items) {
  long blocks = (items + 255) / 256;
  if (blocks > GS_MAX_BLOCKS) blocks = GS_MAX_BLOCKS;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// DY_ERR_ARG / DY_ERR_ALIGN of one operand of ``width`` channels (null allowed: the caller decided)
static int gs_check_op(const void* p, int ld, int width) {
  if (ld < width) return DY_ERR_ARG;
  if ((ld & 7) || ((uintptr_t)p & 15)) return DY_ERR_ALIGN;
  return DY_OK;
}

extern "C" int dy_gs_shuffle_forward(const void* x1, int ld1, const void* d, int ldd, void* y, int ldy, int n, int H, int W, int c_,
                                     hipStream_t stream) {
  if (!x1 || !d || !y || n < 1 || H < 1 || W < 1 || c_ < 8) return DY_ERR_ARG;
  if (c_ & 7) return DY_ERR_ALIGN;
  int rc;
  if ((rc = gs_check_op(x1, ld1, c_)) != DY_OK || (rc = gs_check_op(d, ldd, c_)) != DY_OK || (rc = gs_check_op(y, ldy, 2 * c_)) != DY_OK)
    return rc;
  const int gpp = c_ >> 3;
  const long total = (long)n * H * W * gpp * 2;
  hipLaunchKernelGGL(gs_shuffle_fwd_kernel, dim3(gs_grid(total)), dim3(256), 0, stream, (const f16*)x1, ld1, (const f16*)d, ldd, (f16*)y,
                     ldy, total, gpp);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_gs_shuffle_backward(const void* dy, int ldy, void* dx1, int ld1, int acc1, void* dd, int ldd, int accd, int n, int H,
                                      int W, int c_, hipStream_t stream) {
  if (!dy || n < 1 || H < 1 || W < 1 || c_ < 8) return DY_ERR_ARG;
  if (c_ & 7) return DY_ERR_ALIGN;
  int rc;
  if ((rc = gs_check_op(dy, ldy, 2 * c_)) != DY_OK) return rc;
  if (dx1 && (rc = gs_check_op(dx1, ld1, c_)) != DY_OK) return rc;
  if (dd && (rc = gs_check_op(dd, ldd, c_)) != DY_OK) return rc;
  if (!dx1 && !dd) return DY_OK;  // neither source needs a gradient: nothing to launch
  const int gpp = c_ >> 3;
  const long per_side = (long)n * H * W * gpp;
  const int first = dx1 ? 0 : 1, nside = (dx1 && dd) ? 2 : 1;
  hipLaunchKernelGGL(gs_shuffle_bwd_kernel, dim3(gs_grid(per_side * nside)), dim3(256), 0, stream, (const f16*)dy, ldy, (f16*)dx1, ld1,
                     acc1 ? 1 : 0, (f16*)dd, ldd, accd ? 1 : 0, per_side, first, nside, (nside == 2 && gpp == 1) ? 1 : 0, gpp);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
