// The pooled front of ADown, the YOLOv9 down-sampler (reference nn/extra_modules/block.py:4685-4698):
//   x = avg_pool2d(x, 2, 1, 0, False, True);  x1, x2 = x.chunk(2, 1);  x1 -> cv1 (3x3 s2 p1);  max_pool2d(x2, 3, 2, 1) -> cv2 (1x1)
// on NHWC fp16 tensors addressed as (pointer, pixel stride).  With Ho = H / 2, Wo = W / 2 and c = C / 2:
//   a (n, 2Ho, 2Wo, c)  the averaged FIRST half.  The averaged map is (H-1) x (W-1); an even H (W) leaves one more row (column) in the
//                       buffer, which every launch writes as zero: the 3x3 s2 p1 convolution behind it then reads a stored zero where the
//                       reference reads zero padding, and never sees an odd-sized map.
//   p (n, Ho, Wo, c)    the 3x3 s2 p1 max over the fp16 averages of the SECOND half (out-of-range taps skipped), with the winning tap
//                       3 ky + kx as one byte per element when the caller asks for it.
// Arithmetic.  An average is ((x00 + x01) + x10) + x11 in fp32 (row-major over the 2x2 window), times 0.25, rounded once to fp16.  The
// max compares those fp16 values as if the averaged map had been stored; taps are visited in row-major (ky, kx) order and a tap wins
// only when it is GREATER (or NaN), so ties go to the first maximum, as ATen's forward / backward pair has it; the recorded tap of a
// window that no tap ever wins (all -inf) is its first in-range one.
// Forward: one work item per (output pixel of p, 8-channel granule g of c).  It writes the 2x2 block of ``a`` at (2oy.., 2ox..) for
// granule g of the first half (a 3x3 patch of x) and p's granule g of the second half (a 4x4 patch of x): consecutive lanes take
// consecutive granules, then pixels, so a wave reads both halves of the same pixels of x.  All loads are 16 bytes, addresses clamped
// into the map and unused values dropped; no LDS.
// Backward: a gather, one work item per (pixel of x, granule g of c), no atomics.  First half: 0.25 x the sum of the <= 4 entries of da
// whose average read the pixel, in the order (y-1, x-1), (y-1, x), (y, x-1), (y, x) -- the zero border of ``a`` has no average behind
// it and its gradient is never read.  Second half: the dp of every window whose recorded tap names one of those averages -- a tap
// names exactly one average, so each of the <= 4 windows (oy-, ox-), (oy-, ox+), (oy+, ox-), (oy+, ox+) that can hold one of them
// enters at most once, in that order; one running fp32 sum, times 0.25.  accumulate: one fp32 addition of the stored fp16 value.  One
// fp16 rounding either way.
// Every element offset is 64-bit; nothing outside the C (c) channels of an operand is read or written: all of them may be channel
// slices of wider tensors.
#include "common.h"
#include "dealyolo_hip.h"

struct AdownFwdArgs {
  const f16* x;   // (n, H, W, C) at ldx
  f16* a;         // (n, 2Ho, 2Wo, c) at lda
  f16* p;         // (n, Ho, Wo, c) at ldp
  uint8_t* arg;   // (n, Ho, Wo, c) dense, or null: not written
  int ldx, lda, ldp, c, N, H, W, Ho, Wo;
};
struct AdownBwdArgs {
  const f16* da;       // gradient of a, (n, 2Ho, 2Wo, c) at ldda
  const f16* dp;       // gradient of p, (n, Ho, Wo, c) at lddp
  const uint8_t* arg;  // (n, Ho, Wo, c) dense, as the forward recorded it
  f16* dx;             // (n, H, W, C) at lddx
  int ldda, lddp, lddx, c, N, H, W, Ho, Wo, accumulate;
};

static __device__ __forceinline__ half8 adown_avg(const half8& v00, const half8& v01, const half8& v10, const half8& v11) {
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (f16)(((((float)v00[j] + (float)v01[j]) + (float)v10[j]) + (float)v11[j]) * 0.25f);
  return o;
}

__global__ __launch_bounds__(256) void adown_pool_kernel(AdownFwdArgs s) {
  const int cpp = s.c >> 3;
  const long total = (long)s.N * s.Ho * s.Wo * cpp;
  const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / cpp;
    const int c0 = (int)(idx - pix * cpp) * 8;
    const int ox = (int)(pix % s.Wo);
    const long t = pix / s.Wo;
    const int oy = (int)(t % s.Ho);
    const long n = t / s.Ho;
    const f16* xn = s.x + n * s.H * s.W * s.ldx;
    // ---- first half: the 2x2 block of averages at (2oy, 2ox) from the 3x3 patch of x at the same corner
    {
      half8 v[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int yy = min(2 * oy + r, s.H - 1);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int xx = min(2 * ox + q, s.W - 1);
          v[r][q] = *reinterpret_cast<const half8*>(xn + ((long)yy * s.W + xx) * s.ldx + c0);
        }
      }
      f16* an = s.a + n * (2L * s.Ho) * (2L * s.Wo) * s.lda + c0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int i = 2 * oy + r, j = 2 * ox + q;
          const bool ok = i < s.H - 1 && j < s.W - 1;  // (otherwise: the zero border of an even side)
          const half8 o = adown_avg(v[r][q], v[r][q + 1], v[r + 1][q], v[r + 1][q + 1]);
          *reinterpret_cast<half8*>(an + ((long)i * (2 * s.Wo) + j) * s.lda) = ok ? o : zero;
        }
      }
    }
    // ---- second half: 3x3 s2 p1 max over the averages at (2oy - 1 + ky, 2ox - 1 + kx), from the 4x4 patch of x at (2oy - 1, 2ox - 1)
    {
      half8 v[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int yy = min(max(2 * oy - 1 + r, 0), s.H - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int xx = min(max(2 * ox - 1 + q, 0), s.W - 1);
          v[r][q] = *reinterpret_cast<const half8*>(xn + ((long)yy * s.W + xx) * s.ldx + s.c + c0);
        }
      }
      float best[8];
      int bi[8];
      const int first = (oy == 0 ? 3 : 0) + (ox == 0 ? 1 : 0);  // the first in-range tap: what a window nothing wins records
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        best[j] = -INFINITY;
        bi[j] = first;
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int ay = 2 * oy - 1 + ky;
        const bool yok = ay >= 0 && ay < s.H - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ax = 2 * ox - 1 + kx;
          const bool ok = yok && ax >= 0 && ax < s.W - 1;
          const half8 av = adown_avg(v[ky][kx], v[ky][kx + 1], v[ky + 1][kx], v[ky + 1][kx + 1]);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float f = (float)av[j];
            if (ok && (f > best[j] || f != f)) {
              best[j] = f;
              bi[j] = 3 * ky + kx;
            }
          }
        }
      }
      half8 o;
      uint8_t ai[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o[j] = (f16)best[j];
        ai[j] = (uint8_t)bi[j];
      }
      *reinterpret_cast<half8*>(s.p + pix * s.ldp + c0) = o;
      if (s.arg) *reinterpret_cast<uint2*>(s.arg + pix * s.c + c0) = *reinterpret_cast<uint2*>(ai);
    }
  }
}

__global__ __launch_bounds__(256) void adown_pool_bwd_kernel(AdownBwdArgs s) {
  const int cpp = s.c >> 3;
  const long total = (long)s.N * s.H * s.W * cpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / cpp;
    const int c0 = (int)(idx - pix * cpp) * 8;
    const int x0 = (int)(pix % s.W);
    const long t = pix / s.W;
    const int y0 = (int)(t % s.H);
    const long n = t / s.H;
    // the four averages that read this pixel: (y0 - 1 + (k >> 1), x0 - 1 + (k & 1)), in range of the (H-1) x (W-1) averaged map or not
    bool aok[4];
    int ay[4], ax[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ay[k] = y0 - 1 + (k >> 1);
      ax[k] = x0 - 1 + (k & 1);
      aok[k] = ay[k] >= 0 && ay[k] < s.H - 1 && ax[k] >= 0 && ax[k] < s.W - 1;
    }
    f16* dxp = s.dx + pix * s.lddx;
    // ---- first half
    {
      const f16* dan = s.da + n * (2L * s.Ho) * (2L * s.Wo) * s.ldda + c0;
      half8 g[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int yy = aok[k] ? ay[k] : 0, xx = aok[k] ? ax[k] : 0;  // (0, 0) is an average of every map: H, W >= 2
        g[k] = *reinterpret_cast<const half8*>(dan + ((long)yy * (2 * s.Wo) + xx) * s.ldda);
      }
      half8 old;
      if (s.accumulate) old = *reinterpret_cast<const half8*>(dxp + c0);
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) sum += aok[k] ? (float)g[k][j] : 0.f;
        sum *= 0.25f;
        if (s.accumulate) sum = (float)old[j] + sum;
        o[j] = (f16)sum;
      }
      *reinterpret_cast<half8*>(dxp + c0) = o;
    }
    // ---- second half: the 2x2 windows (wy, wx) that can contain one of the four averages.  A window's recorded tap names exactly one
    // average, so a window contributes its dp at most once: ``hit`` has bit 3 ky + kx set for the taps of the window that land on one of
    // this pixel's in-range averages, and the window counts when its recorded tap is one of them.
    {
      const int wyh = (y0 + 1) >> 1, wxh = (x0 + 1) >> 1;
      int rm[2], cm[2];  // per window row / column: bit k set when tap k lands on an average row / column of this pixel
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int wy = wyh - 1 + r, wx = wxh - 1 + r;
        rm[r] = cm[r] = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int ya = 2 * wy - 1 + k, xa = 2 * wx - 1 + k;
          rm[r] |= (wy >= 0 && wy < s.Ho && (ya == y0 - 1 || ya == y0) && ya >= 0 && ya < s.H - 1) ? 1 << k : 0;
          cm[r] |= (wx >= 0 && wx < s.Wo && (xa == x0 - 1 || xa == x0) && xa >= 0 && xa < s.W - 1) ? 1 << k : 0;
        }
      }
      float sum[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum[j] = 0.f;
      half8 g[4];
      uint2 raw[4];
      int hit[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int r = w >> 1, q = w & 1;
        hit[w] = ((rm[r] & 1) ? cm[q] : 0) | ((rm[r] & 2) ? cm[q] << 3 : 0) | ((rm[r] & 4) ? cm[q] << 6 : 0);
        const int wy = hit[w] ? wyh - 1 + r : 0, wx = hit[w] ? wxh - 1 + q : 0;  // (no tap of it counts: any address of the map will do)
        const long wp = (n * s.Ho + wy) * s.Wo + wx;
        g[w] = *reinterpret_cast<const half8*>(s.dp + wp * s.lddp + c0);
        raw[w] = *reinterpret_cast<const uint2*>(s.arg + wp * s.c + c0);
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint8_t* ai = reinterpret_cast<const uint8_t*>(&raw[w]);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += ((hit[w] >> (ai[j] & 15)) & 1) ? (float)g[w][j] : 0.f;
      }
      half8 old;
      if (s.accumulate) old = *reinterpret_cast<const half8*>(dxp + s.c + c0);
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float r = sum[j] * 0.25f;
        if (s.accumulate) r = (float)old[j] + r;
        o[j] = (f16)r;
      }
      *reinterpret_cast<half8*>(dxp + s.c + c0) = o;
    }
  }
}

static inline unsigned adown_grid(long items) {
  long blocks = (items + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int dy_adown_pool(const void* x, int ldx, void* a, int lda, void* p, int ldp, void* argmax, int n, int H, int W, int C,
                             hipStream_t stream) {
  if (!x || !a || !p || n < 1 || H < 2 || W < 2 || C < 1) return DY_ERR_ARG;
  if ((C & 15) || (ldx & 7) || (lda & 7) || (ldp & 7) || ((uintptr_t)x & 15) || ((uintptr_t)a & 15) || ((uintptr_t)p & 15) ||
      ((uintptr_t)argmax & 15))
    return DY_ERR_ALIGN;
  const int c = C >> 1;
  if (ldx < C || lda < c || ldp < c) return DY_ERR_ARG;
  AdownFwdArgs s{};
  s.x = (const f16*)x, s.a = (f16*)a, s.p = (f16*)p, s.arg = (uint8_t*)argmax;
  s.ldx = ldx, s.lda = lda, s.ldp = ldp, s.c = c, s.N = n, s.H = H, s.W = W, s.Ho = H >> 1, s.Wo = W >> 1;
  hipLaunchKernelGGL(adown_pool_kernel, dim3(adown_grid((long)n * s.Ho * s.Wo * (c >> 3))), dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_adown_pool_backward(const void* da, int ldda, const void* dp, int lddp, const void* argmax, void* dx, int lddx,
                                      int accumulate, int n, int H, int W, int C, hipStream_t stream) {
  if (!da || !dp || !argmax || !dx || n < 1 || H < 2 || W < 2 || C < 1) return DY_ERR_ARG;
  if ((C & 15) || (ldda & 7) || (lddp & 7) || (lddx & 7) || ((uintptr_t)da & 15) || ((uintptr_t)dp & 15) || ((uintptr_t)dx & 15) ||
      ((uintptr_t)argmax & 15))
    return DY_ERR_ALIGN;
  const int c = C >> 1;
  if (lddx < C || ldda < c || lddp < c) return DY_ERR_ARG;
  AdownBwdArgs s{};
  s.da = (const f16*)da, s.dp = (const f16*)dp, s.arg = (const uint8_t*)argmax, s.dx = (f16*)dx;
  s.ldda = ldda, s.lddp = lddp, s.lddx = lddx, s.c = c, s.N = n, s.H = H, s.W = W, s.Ho = H >> 1, s.Wo = W >> 1;
  s.accumulate = accumulate ? 1 : 0;
  hipLaunchKernelGGL(adown_pool_bwd_kernel, dim3(adown_grid((long)n * H * W * (c >> 3))), dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
