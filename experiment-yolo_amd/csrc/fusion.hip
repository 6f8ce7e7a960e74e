// Fusion in 'bifpn' mode, BiFPN's fast normalised fusion (reference nn/extra_modules/block.py:485-488):
//   w = relu(fusion_weight);  f = w / sum(w);  y = sum_i f[i] * x[i]            (no epsilon: the reference never uses the one it sets)
// on NHWC fp16 tensors addressed as (pointer, pixel stride), 2 or 3 operands of one (n, H, W, C).  An operand flagged ``half`` is stored
// at half resolution, (n, H/2, W/2, C): the nn.Upsample(None, 2, 'nearest') in front of it was never executed and pixel (h, w) reads
// (h/2, w/2).  Its GRADIENT is written at full resolution (the up-sampling's own backward folds it).
// The weights.  ``p`` (fp32, nops values) is read from device memory by every work item: w[i] = max(p[i], 0), s = (w[0] + w[1]) + w[2]
// (s = w[0] + w[1] for two operands), f[i] = w[i] / s with the correctly rounded division -- one definition (fusion_weights) shared
// by the three kernels.  All weights <= 0: s = 0 and every f is NaN, as the reference's 0 / 0; nothing guards it.
// Forward: one work item per (pixel, 8-channel granule), consecutive lanes on consecutive granules, then pixels; 16-byte loads and
// stores.  y = fp16((f0 x0 + f1 x1) + f2 x2) in fp32, one fp16 rounding.
// Backward, ONE pass over dy and the operands: dx[i] = fp16(f[i] * dy) (accumulate: fp16(old + f[i] * dy), one fp32 addition of the
// stored value), for every operand that has a dx.  Dot products g[i] = <dy, x[i]>: a work item adds the 8 products of a granule one
// after the other to one running fp32 sum per operand, over the FUSION_ITEMS (or more: the grid is capped) granules it visits in
// grid-stride order; the 64 sums of a wave fold by xor-shuffles (32, 16, ... 1), the four waves' sums are added in wave order, and
// workgroup b stores its sum of g[i] to ws[i * nparts + b].  The grid IS dy_fusion_num_partials(npix, C) workgroups.  A null ``ws``
// selects the frozen variant: no load of any x[i], no dot product.
// Finish, one workgroup: lane t adds ws[i][t], ws[i][t + 256], ... in fp64, an LDS tree in fixed order gives g[i] (fp64, rounded to
// fp32), then in fp32  t = (f0 g0 + f1 g1) + f2 g2,  dL/dp[j] = p[j] > 0 ? (g[j] - t) / s : 0, stored to gw[j] or added to it.
// No atomics anywhere: two runs give the same bits.  Every element offset is 64-bit; nothing outside the C channels of an operand is
// read or written, so every operand may be a channel slice of a wider tensor.
#include "common.h"
#include "dealyolo_hip.h"

#define FUSION_MAX_OPS 3
#define FUSION_ITEMS 4        // granules per work item the partial count is sized for
#define FUSION_MAX_PARTS 1024

struct FusionFwdArgs {
  const f16* x[FUSION_MAX_OPS];
  const float* p;
  f16* y;
  int ld[FUSION_MAX_OPS], half[FUSION_MAX_OPS];
  int ldy, nops, N, H, W, C;
};
struct FusionBwdArgs {
  const f16* dy;
  const f16* x[FUSION_MAX_OPS];
  f16* dx[FUSION_MAX_OPS];  // null: the operand needs no gradient
  const float* p;
  float* ws;                // [nops][gridDim.x], or null (frozen variant)
  int ld[FUSION_MAX_OPS], half[FUSION_MAX_OPS], lddx[FUSION_MAX_OPS], acc[FUSION_MAX_OPS];
  int lddy, nops, N, H, W, C;
};

static __device__ __forceinline__ float fusion_weights(const float* p, int nops, float* f) {
  float w[FUSION_MAX_OPS];
#pragma unroll
  for (int i = 0; i < FUSION_MAX_OPS; ++i) w[i] = i < nops ? fmaxf(p[i], 0.f) : 0.f;
  float s = w[0] + w[1];
  if (nops > 2) s += w[2];
#pragma unroll
  for (int i = 0; i < FUSION_MAX_OPS; ++i) f[i] = i < nops ? w[i] / s : 0.f;
  return s;
}

// element offset of pixel ``pix`` (of the (N, H, W) map) in an operand stored at full or at half resolution
static __device__ __forceinline__ long fusion_src(long pix, int half, int H, int W, int ld) {
  if (!half) return pix * ld;
  const int w = (int)(pix % W);
  const long t = pix / W;
  const int h = (int)(t % H);
  const long n = t / H;
  return ((n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * ld;
}

__global__ __launch_bounds__(256) void fusion_fwd_kernel(FusionFwdArgs s) {
  float f[FUSION_MAX_OPS];
  fusion_weights(s.p, s.nops, f);
  const int cpp = s.C >> 3;
  const long total = (long)s.N * s.H * s.W * cpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / cpp;
    const int c0 = (int)(idx - pix * cpp) * 8;
    const half8 a = *reinterpret_cast<const half8*>(s.x[0] + fusion_src(pix, s.half[0], s.H, s.W, s.ld[0]) + c0);
    const half8 b = *reinterpret_cast<const half8*>(s.x[1] + fusion_src(pix, s.half[1], s.H, s.W, s.ld[1]) + c0);
    half8 c = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s.nops > 2) c = *reinterpret_cast<const half8*>(s.x[2] + fusion_src(pix, s.half[2], s.H, s.W, s.ld[2]) + c0);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = f[0] * (float)a[j] + f[1] * (float)b[j];
      if (s.nops > 2) v += f[2] * (float)c[j];
      o[j] = (f16)v;
    }
    *reinterpret_cast<half8*>(s.y + pix * s.ldy + c0) = o;
  }
}

template <bool DOTS>
__global__ __launch_bounds__(256) void fusion_bwd_kernel(FusionBwdArgs s) {
  float f[FUSION_MAX_OPS];
  fusion_weights(s.p, s.nops, f);
  float g[FUSION_MAX_OPS] = {0.f, 0.f, 0.f};
  const int cpp = s.C >> 3;
  const long total = (long)s.N * s.H * s.W * cpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long pix = idx / cpp;
    const int c0 = (int)(idx - pix * cpp) * 8;
    const half8 d = *reinterpret_cast<const half8*>(s.dy + pix * s.lddy + c0);
#pragma unroll
    for (int i = 0; i < FUSION_MAX_OPS; ++i) {
      if (i >= s.nops) break;
      if (DOTS) {
        const half8 xv = *reinterpret_cast<const half8*>(s.x[i] + fusion_src(pix, s.half[i], s.H, s.W, s.ld[i]) + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[i] += (float)d[j] * (float)xv[j];
      }
      if (s.dx[i]) {
        f16* dst = s.dx[i] + pix * s.lddx[i] + c0;
        half8 old;
        if (s.acc[i]) old = *reinterpret_cast<const half8*>(dst);
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = f[i] * (float)d[j];
          if (s.acc[i]) v = (float)old[j] + v;
          o[j] = (f16)v;
        }
        *reinterpret_cast<half8*>(dst) = o;
      }
    }
  }
  if (DOTS) {
    __shared__ float red[FUSION_MAX_OPS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < FUSION_MAX_OPS; ++i) {
      const float v = wave_sum(g[i]);
      if (lane == 0) red[i][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < s.nops) {
      const int i = threadIdx.x;
      s.ws[(long)i * gridDim.x + blockIdx.x] = ((red[i][0] + red[i][1]) + red[i][2]) + red[i][3];
    }
  }
}

__global__ __launch_bounds__(256) void fusion_finish_kernel(const float* ws, int nparts, const float* p, float* gw, int nops, int accumulate) {
  __shared__ double red[FUSION_MAX_OPS][256];
  const int t = threadIdx.x;
  for (int i = 0; i < nops; ++i) {
    double a = 0.0;
    for (int b = t; b < nparts; b += 256) a += (double)ws[(long)i * nparts + b];
    red[i][t] = a;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o)
      for (int i = 0; i < nops; ++i) red[i][t] += red[i][t + o];
    __syncthreads();
  }
  if (t < nops) {
    float f[FUSION_MAX_OPS];
    const float sum = fusion_weights(p, nops, f);
    float g[FUSION_MAX_OPS];
#pragma unroll
    for (int i = 0; i < FUSION_MAX_OPS; ++i) g[i] = i < nops ? (float)red[i][0] : 0.f;
    float dot = f[0] * g[0] + f[1] * g[1];
    if (nops > 2) dot += f[2] * g[2];
    const float d = p[t] > 0.f ? (g[t] - dot) / sum : 0.f;
    gw[t] = accumulate ? gw[t] + d : d;
  }
}

static inline unsigned fusion_grid(long items) {
  long blocks = (items + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int dy_fusion_num_partials(long npix, int C) {
  if (npix < 1 || C < 8 || (C & 7)) return DY_ERR_ARG;
  const long items = npix * (C >> 3);
  long parts = (items + 256L * FUSION_ITEMS - 1) / (256L * FUSION_ITEMS);
  if (parts > FUSION_MAX_PARTS) parts = FUSION_MAX_PARTS;
  return (int)(parts < 1 ? 1 : parts);
}

static int fusion_check_op(const void* x, int ld, int half, int C, int H, int W) {
  if (!x || ld < C) return DY_ERR_ARG;
  if (half && ((H | W) & 1)) return DY_ERR_ARG;
  if ((ld & 7) || ((uintptr_t)x & 15)) return DY_ERR_ALIGN;
  return DY_OK;
}

extern "C" int dy_fusion_forward(const void* x0, int ld0, int half0, const void* x1, int ld1, int half1, const void* x2, int ld2, int half2,
                                 const float* p, void* y, int ldy, int nops, int n, int H, int W, int C, hipStream_t stream) {
  if (nops < 2 || nops > FUSION_MAX_OPS || !p || !y || n < 1 || H < 1 || W < 1 || C < 1 || ldy < C) return DY_ERR_ARG;
  if ((C & 7) || (ldy & 7) || ((uintptr_t)y & 15) || ((uintptr_t)p & 3)) return DY_ERR_ALIGN;
  const void* xs[3] = {x0, x1, x2};
  const int lds[3] = {ld0, ld1, ld2}, hs[3] = {half0, half1, half2};
  FusionFwdArgs s{};
  for (int i = 0; i < nops; ++i) {
    const int rc = fusion_check_op(xs[i], lds[i], hs[i], C, H, W);
    if (rc != DY_OK) return rc;
    s.x[i] = (const f16*)xs[i], s.ld[i] = lds[i], s.half[i] = hs[i] ? 1 : 0;
  }
  s.p = p, s.y = (f16*)y, s.ldy = ldy, s.nops = nops, s.N = n, s.H = H, s.W = W, s.C = C;
  hipLaunchKernelGGL(fusion_fwd_kernel, dim3(fusion_grid((long)n * H * W * (C >> 3))), dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_fusion_backward(const void* dy, int lddy, const void* x0, int ld0, int half0, void* dx0, int lddx0, int acc0,
                                  const void* x1, int ld1, int half1, void* dx1, int lddx1, int acc1, const void* x2, int ld2, int half2,
                                  void* dx2, int lddx2, int acc2, const float* p, float* ws, int nops, int n, int H, int W, int C,
                                  hipStream_t stream) {
  if (nops < 2 || nops > FUSION_MAX_OPS || !p || !dy || n < 1 || H < 1 || W < 1 || C < 1 || lddy < C) return DY_ERR_ARG;
  if ((C & 7) || (lddy & 7) || ((uintptr_t)dy & 15) || ((uintptr_t)p & 3) || ((uintptr_t)ws & 3)) return DY_ERR_ALIGN;
  const void* xs[3] = {x0, x1, x2};
  void* dxs[3] = {dx0, dx1, dx2};
  const int lds[3] = {ld0, ld1, ld2}, hs[3] = {half0, half1, half2}, ldd[3] = {lddx0, lddx1, lddx2}, accs[3] = {acc0, acc1, acc2};
  FusionBwdArgs s{};
  for (int i = 0; i < nops; ++i) {
    if (ws || xs[i]) {  // (the frozen variant reads no operand: its pointers may be null)
      const int rc = fusion_check_op(xs[i], lds[i], hs[i], C, H, W);
      if (rc != DY_OK) return rc;
    }
    if (dxs[i]) {
      if (ldd[i] < C) return DY_ERR_ARG;
      if ((ldd[i] & 7) || ((uintptr_t)dxs[i] & 15)) return DY_ERR_ALIGN;
    }
    s.x[i] = (const f16*)xs[i], s.ld[i] = lds[i], s.half[i] = hs[i] ? 1 : 0;
    s.dx[i] = (f16*)dxs[i], s.lddx[i] = ldd[i], s.acc[i] = accs[i] ? 1 : 0;
  }
  s.dy = (const f16*)dy, s.lddy = lddy, s.p = p, s.ws = ws, s.nops = nops, s.N = n, s.H = H, s.W = W, s.C = C;
  const int parts = dy_fusion_num_partials((long)n * H * W, C);
  if (ws)
    hipLaunchKernelGGL(fusion_bwd_kernel<true>, dim3(parts), dim3(256), 0, stream, s);
  else
    hipLaunchKernelGGL(fusion_bwd_kernel<false>, dim3(fusion_grid((long)n * H * W * (C >> 3))), dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_fusion_wgrad_finish(const float* ws, int nparts, const float* p, float* gw, int nops, int accumulate, hipStream_t stream) {
  if (!ws || !p || !gw || nops < 2 || nops > FUSION_MAX_OPS || nparts < 1) return DY_ERR_ARG;
  if (((uintptr_t)ws & 3) || ((uintptr_t)p & 3) || ((uintptr_t)gw & 3)) return DY_ERR_ALIGN;
  hipLaunchKernelGGL(fusion_finish_kernel, dim3(1), dim3(256), 0, stream, ws, nparts, p, gw, nops, accumulate ? 1 : 0);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
