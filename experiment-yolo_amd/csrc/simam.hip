// SimAM, the parameter-free attention of reference nn/extra_modules/attention.py:53-77.  Per image b and channel c, over the
// M = H W values of the plane, n = M - 1, lambda = e_lambda:
//   mu = mean(x)   d = x - mu   S = sum(d^2)   D = 4 (S / n + lambda)   e = d^2 / D + 0.5   a = sigmoid(e)   y = x a
// and, with g = dy,  q = g x a (1 - a),  T = sum(q d^2),  U = sum(q d):
//   dx = g a + (2 d / D) (q - 4 T / (n D)) - 2 U / (M D)
// on NHWC fp16 tensors addressed as (pointer, pixel stride), C a multiple of 8.  A plane of one pixel has n = 0: S / n = 0 / 0 and
// every y of the plane is NaN, as in the reference; nothing guards it.
// Work split.  A plane is strided by the pixel pitch, so a workgroup per plane would read 16 bytes of every pitch; instead a
// workgroup takes ALL channels (up to 2,048: blockIdx.y counts blocks of 256 granules) of a run of ``ppc`` consecutive pixels of one
// image: thread t holds granule t % G of pixel row t / G (G = granules per pixel in this block, 256 / G rows per sweep), so a wave
// reads consecutive 16-byte granules of consecutive pixels.  simam_geom() sizes ppc for SIMAM_SWEEPS sweeps and caps the runs per
// image at SIMAM_MAX_PARTS (ppc grows instead).
// Two launches each way, no finalize launch:
//   stats pass   per thread fp64 running sums of x and x^2 (forward) or q d^2 and q d (backward) for its 8 channels -- an fp16 value
//                and its square are exact in fp64, so the mean >> spread case needs no second pass --, an LDS tree over the rows in
//                fixed order, one fp64 partial per (image, run, sum, channel) stored to the caller's workspace;
//   apply pass   every workgroup folds its image's partials in a fixed order in fp64 (the bn_act scheme; simam_fold_each), forms the
//                fp32 plane constants in LDS and applies them; run 0 of the forward also stores (mu, 1 / D) to the statistics buffer [n][2][C] that the
//                backward reads.  ``a`` is recomputed, never stored.
// fp32 arithmetic of an element (one definition each, shared by the three kernels that need it):
//   d = x - mu;  e = fma(d * d, invD, 0.5);  a = 1 / (1 + exp(-e));  y = fp16(x * a)
//   p = a - a * a;  q = (g * x) * p;  dx = fp16(fma(g, a, fma((2 d) * invD, q - k1, -k2)))     k1 = 4 T invD / n, k2 = 2 U invD / M
//   accumulate: fp16(stored + that sum), one more fp32 addition.
// No atomics: two runs give the same bits.  Every element offset is 64-bit; nothing outside the C channels is read or written.
#include "common.h"
#include "dealyolo_hip.h"

#define SIMAM_SWEEPS 16      // sweeps of 256 / G pixel rows a workgroup's run is sized for (8 and 32 measured: DESIGN section 35)
#define SIMAM_MAX_PARTS 64   // runs (= partials per plane sum) per image at the most
#define SIMAM_GBLOCK 256     // granules of a pixel one workgroup covers

struct SimamGeom {
  long ppc;    // pixels per run
  int parts;   // runs per image
};

static inline SimamGeom simam_geom(long M, int C) {
  const int cpp = C >> 3;
  const int G = cpp < SIMAM_GBLOCK ? cpp : SIMAM_GBLOCK;
  long ppc = (long)(256 / G) * SIMAM_SWEEPS;
  long parts = (M + ppc - 1) / ppc;
  if (parts > SIMAM_MAX_PARTS) {
    ppc = (M + SIMAM_MAX_PARTS - 1) / SIMAM_MAX_PARTS;
    parts = (M + ppc - 1) / ppc;
  }
  return {ppc, (int)parts};
}

struct SimamArgs {
  const f16* x;     // the block's input
  const f16* g;     // dy (backward)
  f16* out;         // y (forward apply) or dx (backward apply)
  float* stats;     // [n][2][C]: mu, 1 / D
  double* ws;       // [n][parts][2][C]
  long ldx, ldg, ldo;
  long M, ppc;
  int parts, C, accumulate;
  float lambda;
};

static __device__ __forceinline__ float simam_attn(float x, float mu, float invD, float& d) {
  d = x - mu;
  const float e = __builtin_fmaf(d * d, invD, 0.5f);
  return sigmoid_f(e);
}

// thread geometry of a workgroup: granule block, granules per pixel in it, rows per sweep, this thread's granule and row
struct SimamLane {
  int c0, G, R, tx, ty;
  long img, p0, p1;
};
static __device__ __forceinline__ SimamLane simam_lane(const SimamArgs& s) {
  SimamLane l;
  const int cpp = s.C >> 3, gb = blockIdx.y * SIMAM_GBLOCK;
  l.G = min(cpp - gb, SIMAM_GBLOCK);
  l.R = 256 / l.G;
  l.ty = threadIdx.x / l.G;
  l.tx = threadIdx.x - l.ty * l.G;
  l.c0 = (gb + l.tx) * 8;
  l.img = blockIdx.x / s.parts;
  const long run = blockIdx.x - l.img * s.parts;
  l.p0 = run * s.ppc;
  l.p1 = min(s.M, l.p0 + s.ppc);
  return l;
}

// the 16 fp64 sums of a thread -> the workgroup's sums over its rows (tree in fixed order) -> ws[(img, run)][2][C]
static __device__ __forceinline__ void simam_store_partials(const SimamArgs& s, const SimamLane& l, const double* acc, double (*red)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 16; ++k) red[k][t] = acc[k];
  __syncthreads();
  int o = 1;
  while (o < l.R) o <<= 1;
  int rows = l.R;
  for (o >>= 1; o >= 1; o >>= 1) {
    if (l.ty < o && l.ty + o < rows) {
#pragma unroll
      for (int k = 0; k < 16; ++k) red[k][t] += red[k][t + o * l.G];
    }
    __syncthreads();
    rows = o;
  }
  if (l.ty == 0) {
    double* dst = s.ws + (long)blockIdx.x * 2 * s.C + l.c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dst[j] = red[j][t];
      dst[s.C + j] = red[8 + j][t];
    }
  }
}

// sum ``which`` of channel c of image img over the runs, in run order
static __device__ __forceinline__ double simam_fold(const SimamArgs& s, long img, int which, int c) {
  const double* src = s.ws + (img * s.parts * 2 + which) * s.C + c;
  double a = 0.0;
  for (int p = 0; p < s.parts; ++p) a += src[(long)p * 2 * s.C];
  return a;
}

// f(c, sum 0, sum 1) for every channel c < nch of the block, the sums folded over the image's runs in a fixed order.  Up to 64 channels
// (128 sums) the 256 threads share the runs: thread t adds the runs slot, slot + slots, ... of sum t % (2 nch), slot = t / (2 nch),
// and the channel's thread adds the slots' parts in slot order -- 2 x 25 dependent loads of a 32-channel map become 7.  Wider blocks
// have a thread per sum already.  Ends with a barrier: what f stored to LDS is visible.
template <class F>
static __device__ __forceinline__ void simam_fold_each(const SimamArgs& s, const SimamLane& l, int cb, double* part, F f) {
  const int nch = l.G * 8, t = threadIdx.x;
  if (2 * nch <= 128) {
    const int V = 2 * nch, slots = 256 / V, slot = t / V, v = t - slot * V;
    double a = 0.0;
    if (slot < slots) {
      const int which = v >= nch, c = v - which * nch;
      const double* src = s.ws + (l.img * s.parts * 2 + which) * s.C + cb + c;
      for (int p = slot; p < s.parts; p += slots) a += src[(long)p * 2 * s.C];
    }
    part[t] = a;
    __syncthreads();
    if (t < nch) {
      double a0 = 0.0, a1 = 0.0;
      for (int k = 0; k < slots; ++k) a0 += part[k * V + t], a1 += part[k * V + nch + t];
      f(t, a0, a1);
    }
    __syncthreads();
    return;
  }
  for (int c = t; c < nch; c += 256) f(c, simam_fold(s, l.img, 0, cb + c), simam_fold(s, l.img, 1, cb + c));
  __syncthreads();
}

__global__ __launch_bounds__(256) void simam_fwd_stats_kernel(SimamArgs s) {
  __shared__ double red[16][256];
  const SimamLane l = simam_lane(s);
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  if (l.ty < l.R) {
    const f16* x = s.x + l.img * s.M * s.ldx + l.c0;
#pragma unroll 2
    for (long p = l.p0 + l.ty; p < l.p1; p += l.R) {
      const half8 v = *reinterpret_cast<const half8*>(x + p * s.ldx);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double xv = (double)(float)v[j];
        acc[j] += xv;
        acc[8 + j] = __builtin_fma(xv, xv, acc[8 + j]);
      }
    }
  }
  simam_store_partials(s, l, acc, red);
}

__global__ __launch_bounds__(256) void simam_fwd_apply_kernel(SimamArgs s) {
  __shared__ float smu[SIMAM_GBLOCK * 8], sinv[SIMAM_GBLOCK * 8];
  __shared__ double part[256];
  const SimamLane l = simam_lane(s);
  const int cb = blockIdx.y * SIMAM_GBLOCK * 8;
  simam_fold_each(s, l, cb, part, [&](int c, double sum, double sq) {
    const double mu = sum / (double)s.M;
    double S = sq - sum * mu;
    S = S > 0.0 ? S : 0.0;
    const double D = 4.0 * (S / (double)(s.M - 1) + (double)s.lambda);
    smu[c] = (float)mu;
    sinv[c] = (float)(1.0 / D);
    if (l.p0 == 0) {
      s.stats[l.img * 2 * s.C + cb + c] = smu[c];
      s.stats[l.img * 2 * s.C + s.C + cb + c] = sinv[c];
    }
  });
  if (l.ty >= l.R) return;
  float mu[8], inv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = smu[l.tx * 8 + j], inv[j] = sinv[l.tx * 8 + j];
  const f16* x = s.x + l.img * s.M * s.ldx + l.c0;
  f16* y = s.out + l.img * s.M * s.ldo + l.c0;
#pragma unroll 2
  for (long p = l.p0 + l.ty; p < l.p1; p += l.R) {
    const half8 v = *reinterpret_cast<const half8*>(x + p * s.ldx);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d;
      const float xv = (float)v[j];
      o[j] = (f16)(xv * simam_attn(xv, mu[j], inv[j], d));
    }
    *reinterpret_cast<half8*>(y + p * s.ldo) = o;
  }
}

__global__ __launch_bounds__(256) void simam_bwd_stats_kernel(SimamArgs s) {
  __shared__ double red[16][256];
  const SimamLane l = simam_lane(s);
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  if (l.ty < l.R) {
    float mu[8], inv[8];
    const float* st = s.stats + l.img * 2 * s.C + l.c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) mu[j] = st[j], inv[j] = st[s.C + j];
    const f16* x = s.x + l.img * s.M * s.ldx + l.c0;
    const f16* g = s.g + l.img * s.M * s.ldg + l.c0;
#pragma unroll 2
    for (long p = l.p0 + l.ty; p < l.p1; p += l.R) {
      const half8 v = *reinterpret_cast<const half8*>(x + p * s.ldx);
      const half8 gv = *reinterpret_cast<const half8*>(g + p * s.ldg);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d;
        const float xv = (float)v[j];
        const float a = simam_attn(xv, mu[j], inv[j], d);
        const float q = ((float)gv[j] * xv) * (a - a * a);
        const float qd = q * d;
        acc[j] += (double)(qd * d);   // T
        acc[8 + j] += (double)qd;     // U
      }
    }
  }
  simam_store_partials(s, l, acc, red);
}

__global__ __launch_bounds__(256) void simam_bwd_apply_kernel(SimamArgs s) {
  __shared__ float sk1[SIMAM_GBLOCK * 8], sk2[SIMAM_GBLOCK * 8];
  __shared__ double part[256];
  const SimamLane l = simam_lane(s);
  const int cb = blockIdx.y * SIMAM_GBLOCK * 8;
  simam_fold_each(s, l, cb, part, [&](int c, double T, double U) {
    const double invD = (double)s.stats[l.img * 2 * s.C + s.C + cb + c];
    sk1[c] = (float)(4.0 * T * invD / (double)(s.M - 1));
    sk2[c] = (float)(2.0 * U * invD / (double)s.M);
  });
  if (l.ty >= l.R) return;
  float mu[8], inv[8], k1[8], k2[8];
  const float* st = s.stats + l.img * 2 * s.C + l.c0;
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = st[j], inv[j] = st[s.C + j], k1[j] = sk1[l.tx * 8 + j], k2[j] = sk2[l.tx * 8 + j];
  const f16* x = s.x + l.img * s.M * s.ldx + l.c0;
  const f16* g = s.g + l.img * s.M * s.ldg + l.c0;
  f16* dx = s.out + l.img * s.M * s.ldo + l.c0;
#pragma unroll 2
  for (long p = l.p0 + l.ty; p < l.p1; p += l.R) {
    const half8 v = *reinterpret_cast<const half8*>(x + p * s.ldx);
    const half8 gv = *reinterpret_cast<const half8*>(g + p * s.ldg);
    half8 old;
    if (s.accumulate) old = *reinterpret_cast<const half8*>(dx + p * s.ldo);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d;
      const float xv = (float)v[j], gj = (float)gv[j];
      const float a = simam_attn(xv, mu[j], inv[j], d);
      const float q = (gj * xv) * (a - a * a);
      float r = __builtin_fmaf(gj, a, __builtin_fmaf((2.f * d) * inv[j], q - k1[j], -k2[j]));
      if (s.accumulate) r = (float)old[j] + r;
      o[j] = (f16)r;
    }
    *reinterpret_cast<half8*>(dx + p * s.ldo) = o;
  }
}

extern "C" int dy_simam_num_partials(long M, int C) {
  if (M < 1 || C < 8 || (C & 7)) return DY_ERR_ARG;
  return simam_geom(M, C).parts;
}

static int simam_check(const void* p, int ld, int C) {
  if (!p || ld < C) return DY_ERR_ARG;
  if ((ld & 7) || ((uintptr_t)p & 15)) return DY_ERR_ALIGN;
  return DY_OK;
}

static int simam_launch(SimamArgs& s, int n, int H, int W, int C, void (*stats_k)(SimamArgs), void (*apply_k)(SimamArgs), hipStream_t stream) {
  s.M = (long)H * W;
  const SimamGeom g = simam_geom(s.M, C);
  s.ppc = g.ppc, s.parts = g.parts, s.C = C;
  const long blocks = (long)n * g.parts;
  const int gblocks = ((C >> 3) + SIMAM_GBLOCK - 1) / SIMAM_GBLOCK;
  if (blocks > 0x7fffffffL || gblocks > 65535) return DY_ERR_ARG;
  const dim3 grid((unsigned)blocks, (unsigned)gblocks);
  hipLaunchKernelGGL(stats_k, grid, dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(apply_k, grid, dim3(256), 0, stream, s);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_simam_forward(const void* x, int ldx, void* y, int ldy, float* stats, double* ws, float e_lambda, int n, int H, int W, int C,
                                hipStream_t stream) {
  if (!stats || !ws || n < 1 || H < 1 || W < 1 || C < 8 || (C & 7)) return DY_ERR_ARG;
  int rc = simam_check(x, ldx, C);
  if (rc == DY_OK) rc = simam_check(y, ldy, C);
  if (rc != DY_OK) return rc;
  if (((uintptr_t)stats & 15) || ((uintptr_t)ws & 7)) return DY_ERR_ALIGN;
  SimamArgs s{};
  s.x = (const f16*)x, s.out = (f16*)y, s.stats = stats, s.ws = ws, s.ldx = ldx, s.ldo = ldy, s.lambda = e_lambda;
  return simam_launch(s, n, H, W, C, simam_fwd_stats_kernel, simam_fwd_apply_kernel, stream);
}

extern "C" int dy_simam_backward(const void* dy, int lddy, const void* x, int ldx, const float* stats, void* dx, int lddx, int accumulate,
                                 double* ws, int n, int H, int W, int C, hipStream_t stream) {
  if (!stats || !ws || n < 1 || H < 1 || W < 1 || C < 8 || (C & 7)) return DY_ERR_ARG;
  int rc = simam_check(dy, lddy, C);
  if (rc == DY_OK) rc = simam_check(x, ldx, C);
  if (rc == DY_OK) rc = simam_check(dx, lddx, C);
  if (rc != DY_OK) return rc;
  if (((uintptr_t)stats & 15) || ((uintptr_t)ws & 7)) return DY_ERR_ALIGN;
  SimamArgs s{};
  s.x = (const f16*)x, s.g = (const f16*)dy, s.out = (f16*)dx, s.stats = const_cast<float*>(stats), s.ws = ws;
  s.ldx = ldx, s.ldg = lddy, s.ldo = lddx, s.accumulate = accumulate ? 1 : 0;
  return simam_launch(s, n, H, W, C, simam_bwd_stats_kernel, simam_bwd_apply_kernel, stream);
}
