// CARAFE (content-aware reassembly of features, arXiv 1905.02188; reference nn/extra_modules/block.py:3898-3936) with k_up = 5 and
// scale = 2: the reassembly stage, forward and backward.
//
// The reference shuffles the encoder's 100 channels into 25 channels at twice the resolution (pixel_shuffle :3926), takes the
// softmax over those 25 (:3927), up-samples X by nearest, unfolds 5x5 windows at dilation 2 (:3929-3931) and contracts (:3933).
// That reduces to: the four sub-pixels (i, j) of base pixel (h, w) read the SAME 5x5 neighbourhood of the low-resolution map,
//     p[(h,w),(i,j),k] = softmax_k L[4k + 2i + j, h, w],     Y[c, 2h+i, 2w+j] = sum_{a,b} p[.., 5a+b] X[c, h+a-2, w+b-2],
// with X = 0 outside the map.  Nothing of size 25 C is formed and the weights are never stored: the backward kernels read the fp16
// logits again and recompute them through cf_softmax, the one definition all three kernels share.
//
// A workgroup owns a run of <= 32 base pixels of one row.  Forward: 4 tw softmaxes go to LDS as fp32, the 5 x (tw + 4) pixel
// neighbourhood of X goes to LDS in chunks of <= 64 channels (zeros outside the map, so the tap loop has no border test), then work
// item = (pixel, j, 8-channel granule) with the granule fastest -- a wave's stores are contiguous spans of an output row --
// accumulates both rows i in fp32 over the 25 taps in a fixed order.  dlogits: one lane per (pixel, i, j) keeps its 25 sums
// g_k = sum_c dY_c X_{k,c} in registers over the channel loop, applies the softmax backward and leaves through an LDS tile, so that
// the 104 lanes of a pixel (100..103 zero) go out as 16-byte stores.  dX: a gather -- every input pixel walks the 5 base rows that
// reach it; per base row the workgroup recomputes the weights of tw + 4 base pixels and stages the two rows of dY they own --
// <= 100 terms per element in a fixed order, no atomics: both gradients are bit-repeatable.
#include "common.h"
#include "dealyolo_hip.h"

#define CF_TW 32   // base pixels per workgroup (at most)
#define CF_CCH 64  // channels per LDS chunk (at most)
#define CF_LP 104  // physical lanes of a logit pixel

struct CfArgs {
  const f16* x;   // (N,H,W,C) at ldx
  const f16* lg;  // (N,H,W,100) at ldl >= 104: the encoder's output
  f16* y;         // forward: (N,2H,2W,C) at ldy
  const f16* dy;  // backward: gradient of y at lddy
  f16* dx;        // backward: (N,H,W,C) at lddx
  f16* dl;        // backward: (N,H,W,104) at lddl
  int ldx, ldl, ldy, lddy, lddx, lddl;
  int N, H, W, C, tw, ntile, accumulate;
};

// softmax over the 25 logits of one (base pixel, sub-pixel): lrow points at channel 2i + j of the pixel, the 25 are 4 apart.
// d = L - max is taken as an exact two-term sum (both operands are fp16 values, but their exponents may be far enough apart that
// the fp32 difference rounds): e^d = e^hi (1 + lo).  Sum in the order k = 0..24; division correctly rounded.
static __device__ __forceinline__ void cf_softmax(const f16* lrow, float (&p)[25]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 25; ++k) {
    p[k] = (float)lrow[4 * k];
    m = fmaxf(m, p[k]);
  }
  const float nm = -m;
  float S = 0.f;
#pragma unroll
  for (int k = 0; k < 25; ++k) {
    const float l = p[k], hi = l + nm, bb = hi - l, lo = (l - (hi - bb)) + (nm - bb);
    float e = expf(hi);
    e = fmaf(e, lo, e);
    p[k] = e;
    S += e;
  }
  const float r = 1.f / S;
#pragma unroll
  for (int k = 0; k < 25; ++k) p[k] *= r;
}

struct CfTile { int img, h, w0, wn; };
static __device__ __forceinline__ CfTile cf_tile(const CfArgs& a) {
  CfTile t;
  const int tile = blockIdx.x % a.ntile, rest = blockIdx.x / a.ntile;
  t.h = rest % a.H;
  t.img = rest / a.H;
  t.w0 = tile * a.tw;
  t.wn = min(a.tw, a.W - t.w0);
  return t;
}

// rows h-2..h+2, columns w0-2..w0+wn+1 of channels [c0, c0 + 8 gc) of X -> xs[a][col][ps], zeros outside the map
static __device__ __forceinline__ void cf_stage_x(const CfArgs& a, const CfTile& t, int c0, int gc, int ps, f16* xs, int nthr) {
  const int cols = t.wn + 4, items = 5 * cols * gc;
  for (int it = threadIdx.x; it < items; it += nthr) {
    const int g = it % gc, q = it / gc, col = q % cols, r = q / cols;
    const int hh = t.h + r - 2, ww = t.w0 + col - 2;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W)
      v = *reinterpret_cast<const half8*>(a.x + (((long)t.img * a.H + hh) * a.W + ww) * a.ldx + c0 + g * 8);
    *reinterpret_cast<half8*>(xs + (r * (a.tw + 4) + col) * ps + g * 8) = v;
  }
}

extern __shared__ __attribute__((aligned(16))) unsigned char cf_smem[];

// The LDS carve is sized at launch from the run width tw and the chunk width, so that narrow runs and few channels leave room for
// more workgroups per CU (these launches wait on loads more than they compute); host and kernels agree through these.  Every piece
// is a multiple of 16 bytes.
static __host__ __device__ __forceinline__ int cf_xs_bytes(int tw, int C) { return 5 * (tw + 4) * ((C < CF_CCH ? C : CF_CCH) + 8) * 2; }
static __host__ __device__ __forceinline__ int cf_dys_bytes(int tw, int C) { return 2 * 2 * (tw + 4) * ((C < CF_CCH ? C : CF_CCH) + 8) * 2; }
static __host__ __device__ __forceinline__ int cf_fwd_lds(int tw, int C) { return cf_xs_bytes(tw, C) + tw * 100 * 4; }
static __host__ __device__ __forceinline__ int cf_dl_lds(int tw, int C) { return cf_xs_bytes(tw, C) + tw * CF_LP * 2; }
static __host__ __device__ __forceinline__ int cf_dx_lds(int tw, int C) { return cf_dys_bytes(tw, C) + (tw + 4) * 100 * 4; }

__global__ __launch_bounds__(256) void carafe_fwd_kernel(CfArgs a) {
  f16* xs = reinterpret_cast<f16*>(cf_smem);
  float* wl = reinterpret_cast<float*>(cf_smem + cf_xs_bytes(a.tw, a.C));  // [pixel][k][2i + j]
  const int xw = a.tw + 4;
  const CfTile t = cf_tile(a);
  const long pix0 = ((long)t.img * a.H + t.h) * a.W + t.w0;
  for (int s = threadIdx.x; s < t.wn * 4; s += 256) {
    const int p = s >> 2, ij = s & 3;
    float pr[25];
    cf_softmax(a.lg + (pix0 + p) * a.ldl + ij, pr);
#pragma unroll
    for (int k = 0; k < 25; ++k) wl[p * 100 + k * 4 + ij] = pr[k];
  }
  for (int c0 = 0; c0 < a.C; c0 += CF_CCH) {
    const int gc = min(CF_CCH, a.C - c0) >> 3, ps = gc * 8 + 8;
    __syncthreads();  // the weights are written; the previous chunk's readers are done
    cf_stage_x(a, t, c0, gc, ps, xs, 256);
    __syncthreads();
    for (int it = threadIdx.x; it < t.wn * 2 * gc; it += 256) {
      const int g = it % gc, q = it / gc, j = q & 1, p = q >> 1;
      float acc[2][8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[0][k] = acc[1][k] = 0.f;
      const float* wp = wl + p * 100 + j;
#pragma unroll
      for (int r = 0; r < 5; ++r) {
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const half8 xv = *reinterpret_cast<const half8*>(xs + (r * xw + p + b) * ps + g * 8);
          const float w0 = wp[(5 * r + b) * 4], w1 = wp[(5 * r + b) * 4 + 2];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float xf = (float)xv[k];
            acc[0][k] = fmaf(w0, xf, acc[0][k]);
            acc[1][k] = fmaf(w1, xf, acc[1][k]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        half8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (f16)acc[i][k];
        const long opix = ((long)t.img * (2 * a.H) + (2 * t.h + i)) * (2 * a.W) + 2 * (t.w0 + p) + j;
        *reinterpret_cast<half8*>(a.y + opix * a.ldy + c0 + g * 8) = o;
      }
    }
  }
}

// Logit gradient.  128 threads: one per (pixel, i, j) of the tile.
__global__ __launch_bounds__(128) void carafe_dlogits_kernel(CfArgs a) {
  f16* xs = reinterpret_cast<f16*>(cf_smem);
  f16* dls = reinterpret_cast<f16*>(cf_smem + cf_xs_bytes(a.tw, a.C));  // [pixel][104]
  const int xw = a.tw + 4;
  const CfTile t = cf_tile(a);
  const long pix0 = ((long)t.img * a.H + t.h) * a.W + t.w0;
  const int p = threadIdx.x >> 2, ij = threadIdx.x & 3, i = ij >> 1, j = ij & 1;
  const bool active = p < t.wn;
  float g[25];
#pragma unroll
  for (int k = 0; k < 25; ++k) g[k] = 0.f;
  const long opix = ((long)t.img * (2 * a.H) + (2 * t.h + i)) * (2 * a.W) + 2 * (t.w0 + p) + j;
  for (int c0 = 0; c0 < a.C; c0 += CF_CCH) {
    const int gc = min(CF_CCH, a.C - c0) >> 3, ps = gc * 8 + 8;
    __syncthreads();
    cf_stage_x(a, t, c0, gc, ps, xs, 128);
    __syncthreads();
    if (active) {
      for (int q = 0; q < gc; ++q) {
        const half8 dv = *reinterpret_cast<const half8*>(a.dy + opix * a.lddy + c0 + q * 8);
        float df[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) df[k] = (float)dv[k];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
#pragma unroll
          for (int b = 0; b < 5; ++b) {
            const half8 xv = *reinterpret_cast<const half8*>(xs + (r * xw + p + b) * ps + q * 8);
            float s = g[5 * r + b];
#pragma unroll
            for (int k = 0; k < 8; ++k) s = fmaf(df[k], (float)xv[k], s);
            g[5 * r + b] = s;
          }
        }
      }
    }
  }
  if (active) {
    float pr[25];
    cf_softmax(a.lg + (pix0 + p) * a.ldl + ij, pr);
    float tsum = 0.f;
#pragma unroll
    for (int k = 0; k < 25; ++k) tsum = fmaf(pr[k], g[k], tsum);
#pragma unroll
    for (int k = 0; k < 25; ++k) dls[p * CF_LP + 4 * k + ij] = (f16)(pr[k] * (g[k] - tsum));
    dls[p * CF_LP + 100 + ij] = (f16)0.f;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < t.wn * (CF_LP / 8); it += 128) {
    const int q = it % (CF_LP / 8), pp = it / (CF_LP / 8);
    *reinterpret_cast<half8*>(a.dl + (pix0 + pp) * a.lddl + q * 8) = *reinterpret_cast<const half8*>(dls + pp * CF_LP + q * 8);
  }
}

// Input gradient by gather.  Thread = (input pixel of the tile, granule of the chunk).
__global__ __launch_bounds__(256) void carafe_dx_kernel(CfArgs a) {
  f16* dys = reinterpret_cast<f16*>(cf_smem);                    // [i][output column][ps]
  float* wl = reinterpret_cast<float*>(cf_smem + cf_dys_bytes(a.tw, a.C));  // [base column][k][2i + j]
  const int xw = a.tw + 4;
  const CfTile t = cf_tile(a);
  const int cols = t.wn + 4;
  for (int c0 = 0; c0 < a.C; c0 += CF_CCH) {
    const int gc = min(CF_CCH, a.C - c0) >> 3, ps = gc * 8 + 8;
    const int p = threadIdx.x / gc, g = threadIdx.x % gc;
    const bool active = p < t.wn;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int dr = -2; dr <= 2; ++dr) {
      const int hb = t.h + dr;  // base row (uniform over the workgroup)
      if (hb < 0 || hb >= a.H) continue;
      __syncthreads();
      for (int s = threadIdx.x; s < cols * 4; s += 256) {
        const int pc = s >> 2, ij = s & 3, wb = t.w0 + pc - 2;
        float pr[25];
        if (wb >= 0 && wb < a.W) {
          cf_softmax(a.lg + (((long)t.img * a.H + hb) * a.W + wb) * a.ldl + ij, pr);
        } else {
#pragma unroll
          for (int k = 0; k < 25; ++k) pr[k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 25; ++k) wl[pc * 100 + k * 4 + ij] = pr[k];
      }
      for (int it = threadIdx.x; it < 2 * 2 * cols * gc; it += 256) {
        const int gg = it % gc, q = it / gc, oc = q % (2 * cols), i = q / (2 * cols);
        const int ow = 2 * (t.w0 - 2) + oc;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ow >= 0 && ow < 2 * a.W)
          v = *reinterpret_cast<const half8*>(a.dy + (((long)t.img * (2 * a.H) + (2 * hb + i)) * (2 * a.W) + ow) * a.lddy + c0 + gg * 8);
        *reinterpret_cast<half8*>(dys + (i * (2 * xw) + oc) * ps + gg * 8) = v;
      }
      __syncthreads();
      if (active) {
        const int ar = 2 - dr;  // tap row of base row hb that lands on this input row
#pragma unroll
        for (int dc = -2; dc <= 2; ++dc) {
          const int pc = p + dc + 2, k = 5 * ar + (2 - dc);
#pragma unroll
          for (int ij = 0; ij < 4; ++ij) {
            const float wgt = wl[pc * 100 + k * 4 + ij];
            const half8 dv = *reinterpret_cast<const half8*>(dys + ((ij >> 1) * (2 * xw) + 2 * pc + (ij & 1)) * ps + g * 8);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fmaf(wgt, (float)dv[c], acc[c]);
          }
        }
      }
    }
    if (active) {
      f16* d = a.dx + (((long)t.img * a.H + t.h) * a.W + t.w0 + p) * a.lddx + c0 + g * 8;
      half8 o;
      if (a.accumulate) o = *reinterpret_cast<const half8*>(d);
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = (f16)(acc[c] + (a.accumulate ? (float)o[c] : 0.f));
      *reinterpret_cast<half8*>(d) = o;
    }
  }
}

extern "C" int dy_carafe_supported(int C, int k_up, int scale) { return k_up == 5 && scale == 2 && C >= 8 && C % 8 == 0; }

// tile geometry + the int32 limits: the grid (N H ntile workgroups) and the output pixel count 4 N H W stay below 2^31
static bool cf_geometry(CfArgs& a) {
  a.ntile = (a.W + CF_TW - 1) / CF_TW;
  a.tw = (a.W + a.ntile - 1) / a.ntile;
  return (double)a.N * a.H * a.ntile < 2147483648.0 && 4.0 * a.N * a.H * a.W < 2147483648.0;
}

extern "C" int dy_carafe(const void* x, int ldx, const void* logits, int ldl, void* y, int ldy, int n, int H, int W, int C,
                         hipStream_t stream) {
  if (!x || !logits || !y || n < 1 || H < 1 || W < 1 || !dy_carafe_supported(C, 5, 2)) return DY_ERR_ARG;
  if ((ldx & 7) || (ldy & 7) || (ldl & 7) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)logits & 15)) return DY_ERR_ALIGN;
  if (ldx < C || ldy < C || ldl < CF_LP) return DY_ERR_ARG;
  CfArgs a{};
  a.x = (const f16*)x; a.lg = (const f16*)logits; a.y = (f16*)y; a.ldx = ldx; a.ldl = ldl; a.ldy = ldy;
  a.N = n; a.H = H; a.W = W; a.C = C;
  if (!cf_geometry(a)) return DY_ERR_ARG;
  hipLaunchKernelGGL(carafe_fwd_kernel, dim3(n * H * a.ntile), dim3(256), cf_fwd_lds(a.tw, C), stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_carafe_backward(const void* x, int ldx, const void* logits, int ldl, const void* dy, int lddy, void* dx, int lddx,
                                  int accumulate, void* dlogits, int lddl, int n, int H, int W, int C, hipStream_t stream) {
  if (!x || !logits || !dy || !dlogits || n < 1 || H < 1 || W < 1 || !dy_carafe_supported(C, 5, 2)) return DY_ERR_ARG;
  if ((ldx & 7) || (lddy & 7) || (ldl & 7) || (lddl & 7) || ((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || ((uintptr_t)logits & 15) ||
      ((uintptr_t)dlogits & 15))
    return DY_ERR_ALIGN;
  if (dx && ((lddx & 7) || ((uintptr_t)dx & 15))) return DY_ERR_ALIGN;
  if (ldx < C || lddy < C || ldl < CF_LP || lddl < CF_LP || (dx && lddx < C)) return DY_ERR_ARG;
  CfArgs a{};
  a.x = (const f16*)x; a.lg = (const f16*)logits; a.dy = (const f16*)dy; a.dx = (f16*)dx; a.dl = (f16*)dlogits;
  a.ldx = ldx; a.ldl = ldl; a.lddy = lddy; a.lddx = lddx; a.lddl = lddl;
  a.N = n; a.H = H; a.W = W; a.C = C; a.accumulate = accumulate;
  if (!cf_geometry(a)) return DY_ERR_ARG;
  hipLaunchKernelGGL(carafe_dlogits_kernel, dim3(n * H * a.ntile), dim3(128), cf_dl_lds(a.tw, C), stream, a);
  if (dx) hipLaunchKernelGGL(carafe_dx_kernel, dim3(n * H * a.ntile), dim3(256), cf_dx_lds(a.tw, C), stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
