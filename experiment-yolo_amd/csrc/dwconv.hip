// Depthwise convolution with channel multiplier m = c2 / c1 in {1, 2} (reference nn/modules/conv.py:106-111 DWConv -- Conv with
// g = gcd(c1, c2) --, :113-122 DSConv; nn.Conv2d(groups = c1), k in {3, 5}, s in {1, 2}, 'same' padding k / 2, d = 1): forward with
// its three epilogues, input gradient, weight gradient.  NHWC fp16 activations, fp32 master weights (c2, 1, k, k) read straight from
// the flat parameter buffer -- at most 25 c2 floats, so there is no pack.
//
// Output channel o reads input channel o / m.  A work item is (pixel, 8-channel granule): the forward's output granule reads 8 input
// channels (one 16-byte load) when m = 1 and 4 (one 8-byte load) when m = 2.  Threads of a workgroup are laid out granule fastest,
// then pixel: thread t owns granule t % gc of pixel slot t / gc (gc = granules of the workgroup's chunk of <= 256 output channels,
// blockIdx.y; 256 / gc pixel slots, the threads behind them idle), so consecutive lanes walk the granules of a pixel, then the
// pixels of a row, and a thread keeps ITS granule over its whole pixel loop.  The chunk's weights sit in LDS tap-major
// (ws[tap][channel]): a lane reads the 8 weights of a tap as two 16-byte LDS loads.  Tap reuse of the activations is left to L1 / L2.
//
// Summation orders (fixed: two calls give the same bits; no atomics anywhere):
//   forward     acc = fma(w, x, acc) over the taps (ky, kx) ascending, taps in the padding skipped; fp16(acc) is the raw output.
//               bias epilogue: act(fp16(acc) + bias) -- from the value the raw epilogue stores, so fused and un-fused eval differ by
//               BatchNorm folding only.  Statistics: per thread sum / fma sum of squares of the STORED fp16 values over its pixels
//               ascending, then over the pixel slots ascending: row [block][2][c2] of the partials (dy_bn_finalize's layout).
//   input grad  per input pixel: taps (ky, kx) ascending that reach it (stride 2: those of its parity class), per tap the m output
//               channels of the group ascending; fp32; stored, or added to the fp16 value there (one more rounding).
//   weight grad per thread: its pixels ascending (one fma each and tap) -> pixel slots ascending -> slab [block][c2 k k]; then
//               dw_reduce_kernel: 8 interleaved runs of slabs (p = q, q + 8, ...), the 8 runs ascending.  k = 5 runs one tap row per
//               blockIdx.z so that the 8 k accumulators of a tap row, not 8 k k, live in registers.
#include "common.h"
#include "dealyolo_hip.h"

#define DW_CH 256        // output channels per workgroup (chunk)
#define DW_FWD_MAXB 1024 // rows of statistics partials at most
#define DW_WG_MAXB 512   // weight-gradient slabs at most
#define DW_EPI_STATS DY_EPI_STATS  // the epilogue flags are dy_conv_forward's (include/dealyolo_hip.h)
#define DW_EPI_BIAS DY_EPI_BIAS
#define DW_EPI_SILU DY_EPI_SILU

struct DwArgs {
  const f16* x;       // (N,H,W,C1) at ldx
  const float* w;     // (C2,1,K,K)
  const float* bias;  // [C2] (bias epilogue)
  f16* y;             // (N,Ho,Wo,C2) at ldy
  float* part;        // [gridDim.x][2][C2] (statistics epilogue)
  const f16* dy;      // d(raw): (N,Ho,Wo,C2) at lddy
  f16* dx;            // (N,H,W,C1) at lddx
  float* slabs;       // [gridDim.x][C2 K K]
  int ldx, ldy, lddy, lddx;
  int N, H, W, Ho, Wo, C1, C2, s, epi, accumulate;
  long npix;          // pixels the launch walks: N Ho Wo (forward, weight gradient), N H W (input gradient)
};

extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];

// the chunk's weights -> ws[tap][channel of the chunk] (global reads contiguous: channel-major there)
template <int K>
static __device__ __forceinline__ void dw_stage_w(const float* w, int c0, int cn, float* ws) {
  for (int i = threadIdx.x; i < K * K * cn; i += 256) {
    const int cc = i / (K * K), t = i - cc * (K * K);
    ws[t * cn + cc] = w[(long)c0 * (K * K) + i];
  }
}

template <int K, int M>
__global__ __launch_bounds__(256) void dw_fwd_kernel(DwArgs a) {
  constexpr int P = K / 2;
  const int c0 = blockIdx.y * DW_CH, cn = min(DW_CH, a.C2 - c0), gc = cn >> 3, ps = 256 / gc;
  float* ws = reinterpret_cast<float*>(dw_smem);
  float* red = ws + K * K * cn;  // [2][ps][cn]
  dw_stage_w<K>(a.w, c0, cn, ws);
  __syncthreads();
  const int slot = threadIdx.x / gc, g = threadIdx.x - slot * gc;
  const int co = c0 + g * 8;       // first output channel of the granule
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (slot < ps) {
    for (long pix = (long)blockIdx.x * ps + slot; pix < a.npix; pix += (long)gridDim.x * ps) {
      const int ox = (int)(pix % a.Wo);
      const long r = pix / a.Wo;
      const int oy = (int)(r % a.Ho), n = (int)(r / a.Ho);
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = oy * a.s + ky - P;
        if (iy < 0 || iy >= a.H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ox * a.s + kx - P;
          if (ix < 0 || ix >= a.W) continue;
          const f16* xp = a.x + (((long)n * a.H + iy) * a.W + ix) * a.ldx + co / M;
          const float* wp = ws + (ky * K + kx) * cn + g * 8;
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
          if (M == 1) {
            const half8 xv = *reinterpret_cast<const half8*>(xp);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[j] = fmaf(w0[j], (float)xv[j], acc[j]);
              acc[j + 4] = fmaf(w1[j], (float)xv[j + 4], acc[j + 4]);
            }
          } else {
            const half4 xv = *reinterpret_cast<const half4*>(xp);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[j] = fmaf(w0[j], (float)xv[j >> 1], acc[j]);
              acc[j + 4] = fmaf(w1[j], (float)xv[2 + (j >> 1)], acc[j + 4]);
            }
          }
        }
      }
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (f16)acc[j];
      if (a.epi & DW_EPI_BIAS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float z = (float)o[j] + a.bias[co + j];
          o[j] = (f16)((a.epi & DW_EPI_SILU) ? act_fwd_t<DY_ACT_SILU>(z) : z);
        }
      }
      *reinterpret_cast<half8*>(a.y + pix * a.ldy + co) = o;
      if (a.epi & DW_EPI_STATS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = (float)o[j];
          s1[j] += v;
          s2[j] = fmaf(v, v, s2[j]);
        }
      }
    }
  }
  if (!(a.epi & DW_EPI_STATS)) return;  // (uniform)
  if (slot < ps) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[slot * cn + g * 8 + j] = s1[j];
      red[(ps + slot) * cn + g * 8 + j] = s2[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < cn) {
    float t1 = 0.f, t2 = 0.f;
    for (int q = 0; q < ps; ++q) {
      t1 += red[q * cn + threadIdx.x];
      t2 += red[(ps + q) * cn + threadIdx.x];
    }
    a.part[((long)blockIdx.x * 2 + 0) * a.C2 + c0 + threadIdx.x] = t1;
    a.part[((long)blockIdx.x * 2 + 1) * a.C2 + c0 + threadIdx.x] = t2;
  }
}

// dX: a gather over the taps that reach an input pixel.  The chunk is DW_CH output channels = DW_CH / M input channels.
template <int K, int M>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(DwArgs a) {
  constexpr int P = K / 2;
  const int c0 = blockIdx.y * DW_CH, cn = min(DW_CH, a.C2 - c0), gi = (cn / M) >> 3, ps = 256 / gi;
  float* ws = reinterpret_cast<float*>(dw_smem);
  dw_stage_w<K>(a.w, c0, cn, ws);
  __syncthreads();
  const int slot = threadIdx.x / gi, g = threadIdx.x - slot * gi;
  if (slot >= ps) return;
  const int sh = a.s - 1;  // s in {1, 2}: t % s == t & sh, t / s == t >> sh for t >= 0
  for (long pix = (long)blockIdx.x * ps + slot; pix < a.npix; pix += (long)gridDim.x * ps) {
    const int ix = (int)(pix % a.W);
    const long r = pix / a.W;
    const int iy = (int)(r % a.H), n = (int)(r / a.H);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int ty = iy + P - ky;
      if (ty < 0 || (ty & sh) || (ty >> sh) >= a.Ho) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int tx = ix + P - kx;
        if (tx < 0 || (tx & sh) || (tx >> sh) >= a.Wo) continue;
        const f16* dp = a.dy + (((long)n * a.Ho + (ty >> sh)) * a.Wo + (tx >> sh)) * a.lddy + c0 + g * 8 * M;
        const float* wp = ws + (ky * K + kx) * cn + g * 8 * M;
        if (M == 1) {
          const half8 dv = *reinterpret_cast<const half8*>(dp);
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf(w0[j], (float)dv[j], acc[j]);
            acc[j + 4] = fmaf(w1[j], (float)dv[j + 4], acc[j + 4]);
          }
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) {  // input channels 4 h .. 4 h + 3 of the granule <- output channels 8 h .. 8 h + 7
            const half8 dv = *reinterpret_cast<const half8*>(dp + 8 * h);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + 8 * h), w1 = *reinterpret_cast<const f32x4*>(wp + 8 * h + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float& t = acc[4 * h + (j >> 1)];
              t = fmaf(w0[j], (float)dv[j], t);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float& t = acc[4 * h + 2 + (j >> 1)];
              t = fmaf(w1[j], (float)dv[4 + j], t);
            }
          }
        }
      }
    }
    f16* d = a.dx + pix * a.lddx + c0 / M + g * 8;
    half8 o;
    if (a.accumulate) o = *reinterpret_cast<const half8*>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(a.accumulate ? acc[j] + (float)o[j] : acc[j]);
    *reinterpret_cast<half8*>(d) = o;
  }
}

// dW, stage 1: TR tap rows per workgroup (blockIdx.z * TR is the first), per-workgroup slabs.
template <int K, int M, int TR>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(DwArgs a) {
  constexpr int P = K / 2;
  __shared__ float red[256 * 8];
  const int c0 = blockIdx.y * DW_CH, cn = min(DW_CH, a.C2 - c0), gc = cn >> 3, ps = 256 / gc;
  const int slot = threadIdx.x / gc, g = threadIdx.x - slot * gc;
  const int co = c0 + g * 8, ky0 = blockIdx.z * TR;
  float acc[TR * K][8];
#pragma unroll
  for (int t = 0; t < TR * K; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
  if (slot < ps) {
    for (long pix = (long)blockIdx.x * ps + slot; pix < a.npix; pix += (long)gridDim.x * ps) {
      const int ox = (int)(pix % a.Wo);
      const long r = pix / a.Wo;
      const int oy = (int)(r % a.Ho), n = (int)(r / a.Ho);
      const half8 dv = *reinterpret_cast<const half8*>(a.dy + pix * a.lddy + co);
#pragma unroll
      for (int tr = 0; tr < TR; ++tr) {
        const int iy = oy * a.s + ky0 + tr - P;
        if (iy < 0 || iy >= a.H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ox * a.s + kx - P;
          if (ix < 0 || ix >= a.W) continue;
          const f16* xp = a.x + (((long)n * a.H + iy) * a.W + ix) * a.ldx + co / M;
          if (M == 1) {
            const half8 xv = *reinterpret_cast<const half8*>(xp);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[tr * K + kx][j] = fmaf((float)dv[j], (float)xv[j], acc[tr * K + kx][j]);
          } else {
            const half4 xv = *reinterpret_cast<const half4*>(xp);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[tr * K + kx][j] = fmaf((float)dv[j], (float)xv[j >> 1], acc[tr * K + kx][j]);
          }
        }
      }
    }
  }
  const long E = (long)a.C2 * K * K;
#pragma unroll
  for (int t = 0; t < TR * K; ++t) {
    __syncthreads();  // the previous tap's readers are done
    if (slot < ps) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[slot * cn + g * 8 + j] = acc[t][j];
    }
    __syncthreads();
    if ((int)threadIdx.x < cn) {
      float v = 0.f;
      for (int q = 0; q < ps; ++q) v += red[q * cn + threadIdx.x];
      a.slabs[blockIdx.x * E + (long)(c0 + threadIdx.x) * K * K + ky0 * K + t] = v;
    }
  }
}

// dW, stage 2: dw[e] (+)= sum over the slabs, 8 interleaved runs then the runs in order
__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* slabs, int nslabs, long E, float* dw, int accumulate) {
  __shared__ float r[8][32];
  const int q = threadIdx.x >> 5, l = threadIdx.x & 31;
  const long e = (long)blockIdx.x * 32 + l;
  float v = 0.f;
  if (e < E)
    for (int p = q; p < nslabs; p += 8) v += slabs[p * E + e];
  r[q][l] = v;
  __syncthreads();
  if (q == 0 && e < E) {
    float t = r[0][l];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += r[k][l];
    dw[e] = accumulate ? dw[e] + t : t;
  }
}

// ---------------------------------------------------------------------------------------------- host side
extern "C" int dy_dwconv_supported(int C1, int m, int k, int s) {
  return C1 >= 8 && C1 % 8 == 0 && (m == 1 || m == 2) && (k == 3 || k == 5) && (s == 1 || s == 2);
}

static inline int dw_out(int h, int k, int s) { return (h + 2 * (k / 2) - k) / s + 1; }
static inline int dw_slots(int C2) { return 256 / ((C2 < DW_CH ? C2 : DW_CH) >> 3); }  // pixel slots of a workgroup (its widest chunk)
static inline int dw_blocks(double npix, int slots, int cap) {
  const double b = (npix + slots - 1) / slots;
  return b < 1 ? 1 : b > cap ? cap : (int)b;
}
static bool dw_geometry(int n, int H, int W, int C1, int m, int k, int s) {
  return n >= 1 && H >= 1 && W >= 1 && dy_dwconv_supported(C1, m, k, s) && (double)n * H * W < 2147483648.0 && (double)C1 * m < 65536.0 * 8;
}

extern "C" int dy_dwconv_num_partials(int n, int H, int W, int C1, int m, int k, int s) {
  if (!dw_geometry(n, H, W, C1, m, k, s)) return DY_ERR_ARG;
  return dw_blocks((double)n * dw_out(H, k, s) * dw_out(W, k, s), dw_slots(C1 * m), DW_FWD_MAXB);
}

extern "C" int dy_dwconv_wgrad_slabs(int n, int H, int W, int C1, int m, int k, int s) {
  if (!dw_geometry(n, H, W, C1, m, k, s)) return DY_ERR_ARG;
  return dw_blocks((double)n * dw_out(H, k, s) * dw_out(W, k, s), dw_slots(C1 * m), DW_WG_MAXB);
}

#define DW_DISPATCH(KERNEL, grid, lds, stream, args)                                                       \
  do {                                                                                                     \
    if (k == 3 && m == 1) hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(256), lds, stream, args);           \
    else if (k == 3) hipLaunchKernelGGL((KERNEL<3, 2>), grid, dim3(256), lds, stream, args);                \
    else if (m == 1) hipLaunchKernelGGL((KERNEL<5, 1>), grid, dim3(256), lds, stream, args);                \
    else hipLaunchKernelGGL((KERNEL<5, 2>), grid, dim3(256), lds, stream, args);                            \
  } while (0)

extern "C" int dy_dwconv_forward(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, float* partials, int n,
                                 int H, int W, int C1, int m, int k, int s, int epi, hipStream_t stream) {
  if (!x || !w || !y || !dw_geometry(n, H, W, C1, m, k, s)) return DY_ERR_ARG;
  if ((epi & ~(DW_EPI_STATS | DW_EPI_BIAS | DW_EPI_SILU)) || ((epi & DW_EPI_STATS) && ((epi & DW_EPI_BIAS) || !partials)) ||
      ((epi & DW_EPI_BIAS) && !bias) || ((epi & DW_EPI_SILU) && !(epi & DW_EPI_BIAS)))
    return DY_ERR_ARG;
  const int C2 = C1 * m;
  if ((ldx & 7) || (ldy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)w & 15) || ((uintptr_t)bias & 15) ||
      ((uintptr_t)partials & 15))
    return DY_ERR_ALIGN;
  if (ldx < C1 || ldy < C2) return DY_ERR_ARG;
  DwArgs a{};
  a.x = (const f16*)x; a.w = w; a.bias = bias; a.y = (f16*)y; a.part = partials; a.ldx = ldx; a.ldy = ldy;
  a.N = n; a.H = H; a.W = W; a.Ho = dw_out(H, k, s); a.Wo = dw_out(W, k, s); a.C1 = C1; a.C2 = C2; a.s = s; a.epi = epi;
  a.npix = (long)n * a.Ho * a.Wo;
  const int cn = C2 < DW_CH ? C2 : DW_CH;
  const dim3 grid(dw_blocks((double)a.npix, dw_slots(C2), DW_FWD_MAXB), (C2 + DW_CH - 1) / DW_CH);
  const int lds = k * k * cn * 4 + 2 * 256 * 8 * 4;
  DW_DISPATCH(dw_fwd_kernel, grid, lds, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_dwconv_input_grad(const void* draw, int lddy, const float* w, void* dx, int lddx, int accumulate, int n, int H,
                                    int W, int C1, int m, int k, int s, hipStream_t stream) {
  if (!draw || !w || !dw_geometry(n, H, W, C1, m, k, s)) return DY_ERR_ARG;
  const int C2 = C1 * m;
  if ((lddy & 7) || ((uintptr_t)draw & 15) || ((uintptr_t)w & 15) || (dx && ((lddx & 7) || ((uintptr_t)dx & 15)))) return DY_ERR_ALIGN;
  if (lddy < C2 || (dx && lddx < C1)) return DY_ERR_ARG;
  if (!dx) return DY_OK;  // nothing asks for the gradient: no launch
  DwArgs a{};
  a.dy = (const f16*)draw; a.w = w; a.dx = (f16*)dx; a.lddy = lddy; a.lddx = lddx; a.accumulate = accumulate;
  a.N = n; a.H = H; a.W = W; a.Ho = dw_out(H, k, s); a.Wo = dw_out(W, k, s); a.C1 = C1; a.C2 = C2; a.s = s;
  a.npix = (long)n * H * W;
  const int cn = C2 < DW_CH ? C2 : DW_CH;
  const dim3 grid(dw_blocks((double)a.npix, 256 / ((cn / m) >> 3), 4096), (C2 + DW_CH - 1) / DW_CH);
  const int lds = k * k * cn * 4;
  DW_DISPATCH(dw_dgrad_kernel, grid, lds, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_dwconv_wgrad(const void* x, int ldx, const void* draw, int lddy, float* slabs, float* dw, int accumulate, int n, int H,
                               int W, int C1, int m, int k, int s, hipStream_t stream) {
  if (!x || !draw || !slabs || !dw || !dw_geometry(n, H, W, C1, m, k, s)) return DY_ERR_ARG;
  const int C2 = C1 * m;
  if ((ldx & 7) || (lddy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)draw & 15) || ((uintptr_t)slabs & 15) || ((uintptr_t)dw & 15))
    return DY_ERR_ALIGN;
  if (ldx < C1 || lddy < C2) return DY_ERR_ARG;
  DwArgs a{};
  a.x = (const f16*)x; a.dy = (const f16*)draw; a.slabs = slabs; a.ldx = ldx; a.lddy = lddy;
  a.N = n; a.H = H; a.W = W; a.Ho = dw_out(H, k, s); a.Wo = dw_out(W, k, s); a.C1 = C1; a.C2 = C2; a.s = s;
  a.npix = (long)n * a.Ho * a.Wo;
  const int nslabs = dw_blocks((double)a.npix, dw_slots(C2), DW_WG_MAXB), chunks = (C2 + DW_CH - 1) / DW_CH;
  if (k == 3 && m == 1) hipLaunchKernelGGL((dw_wgrad_kernel<3, 1, 3>), dim3(nslabs, chunks, 1), dim3(256), 0, stream, a);
  else if (k == 3) hipLaunchKernelGGL((dw_wgrad_kernel<3, 2, 3>), dim3(nslabs, chunks, 1), dim3(256), 0, stream, a);
  else if (m == 1) hipLaunchKernelGGL((dw_wgrad_kernel<5, 1, 1>), dim3(nslabs, chunks, 5), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((dw_wgrad_kernel<5, 2, 1>), dim3(nslabs, chunks, 5), dim3(256), 0, stream, a);
  const long E = (long)C2 * k * k;
  hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)((E + 31) / 32)), dim3(256), 0, stream, slabs, nslabs, E, dw, accumulate);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
