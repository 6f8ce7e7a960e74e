// DySample (learned dynamic up-sampling, reference nn/extra_modules/block.py:3819-3892, style 'lp' without dyscope): sampling stage,
// forward and backward.
//
// The reference adds init_pos to 0.25 * offset(x) (:3878), builds a normalised grid through pixel_shuffle (:3860-3870) and calls
// F.grid_sample(bilinear, align_corners=False, padding_mode='border') per channel group (:3871-3872).  The normalisation cancels:
// output pixel (s h + i, s w + j) of group g reads x at
//     px = clamp(w + 0.25 o_x + t[j], 0, W-1),  py = clamp(h + 0.25 o_y + t[i], 0, H-1),   t[k] = (k - (s-1)/2) / s,
// with o_x / o_y the RAW outputs of the 1x1 offset convolution at channels g s^2 + i s + j and G s^2 + g s^2 + i s + j.  Here one
// kernel reads those fp32 offsets, applies the 0.25 and the closed-form init_pos itself and blends the four corners straight from
// the NHWC fp16 map, one 16-byte granule (8 channels) per load and per store.  Work item = (base pixel, column sub-position j,
// granule): consecutive lanes walk the granules of an output pixel, then j, then w, so a wave's store covers one contiguous span of
// an output row; the item holds its 2 s offsets in registers and loops over the s output rows.
// Backward: the offset gradient (0.25 folded in; grid_sample's border rule: no gradient where the unclamped position is at or
// beyond 0 / size-1) by one lane per (base pixel, j, group) in a fixed summation order, and the input gradient as a deterministic
// GATHER, the contract of dy_ldconv_sample_backward_gather: every input pixel walks the base pixels that can reach it, their range
// from the largest |0.25 o| of the layer measured on the device and capped at rmax; samples displaced further (|0.25 o| > rmax - 1) are
// scattered with fp32 atomics into a side accumulator that the gather folds in.  No host decision, the same launches every step.
#include "common.h"
#include "dealyolo_hip.h"

struct DsArgs {
  const f16* x;      // (N,H,W,C) at ldx
  const float* off;  // (N,H,W,2*G*s*s) at ldoff: raw offset-convolution output
  f16* y;            // forward: (N,sH,sW,C) at ldy
  const f16* dy;     // backward: gradient of y at lddy
  f16* dx;           // backward: (N,H,W,C) at lddx
  float* dx32;       // backward: (N,H,W,C) dense fp32 side accumulator of the far samples
  f16* doff;         // backward: (N,H,W,lddoff), channels [0, 2*G*s*s)
  int ldx, ldoff, ldy, lddy, lddx, lddoff;
  int N, H, W, C, G, cpp, gpg;  // cpp = C/8 granules per pixel, gpg = C/(8G) granules per group
};

// q = x / d, r = x % d (32-bit where the value allows it: a 64-bit division is ~100 VALU instructions, csrc/ldconv.hip)
static __device__ __forceinline__ void ds_divmod(long x, int d, long& q, int& r) {
  if (x >= 0 && x < 0x7fffffffL) {
    const unsigned xx = (unsigned)x, qq = xx / (unsigned)d;
    q = (long)qq;
    r = (int)(xx - qq * (unsigned)d);
  } else {
    q = x / d;
    r = (int)(x - q * d);
  }
}

// init_pos (:3856-3858) in closed form: exact in fp32 for s = 2 (+-0.25) and s = 4 (+-0.125, +-0.375)
template <int S>
static __device__ __forceinline__ float ds_init(int k) { return ((float)k - 0.5f * (float)(S - 1)) / (float)S; }

// Landing geometry of one coordinate: base + 0.25 o + init, clamped to [0, size-1]; c0 = floor, c1 = c0 + 1 held inside the map (its
// weight f is 0 whenever it had to be); in: grid_sample's border rule passes a gradient only strictly inside (0, size-1).
// ONE definition for every kernel below, so that forward, gather and scatter agree on every index.  NaN clamps to 0.
struct DsCoord { int c0, c1; float f; bool in; };
static __device__ __forceinline__ DsCoord ds_coord(int base, float o, float init, int size) {
  const float m = (float)(size - 1);
  const float u = (float)base + fmaf(0.25f, o, init);
  const float p = fminf(fmaxf(u, 0.f), m);
  const float fl = floorf(p);
  DsCoord r;
  r.c0 = (int)fl;
  r.c1 = min(r.c0 + 1, size - 1);
  r.f = p - fl;
  r.in = u > 0.f && u < m;
  return r;
}

template <int S>
__global__ __launch_bounds__(256) void dysample_fwd_kernel(DsArgs a) {
  const int SS = S * S;
  const long total = (long)a.N * a.H * a.W * S * a.cpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int part, j, w, h;
    long t, pix, img;
    ds_divmod(idx, a.cpp, t, part);
    ds_divmod(t, S, pix, j);
    ds_divmod(pix, a.W, t, w);
    ds_divmod(t, a.H, img, h);
    const int g = part / a.gpg;
    const float* o = a.off + pix * a.ldoff + g * SS + j;
    float ox[S], oy[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      ox[i] = o[i * S];
      oy[i] = o[a.G * SS + i * S];
    }
    const f16* xb = a.x + img * a.H * a.W * a.ldx + part * 8;
    const float tj = ds_init<S>(j);
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const DsCoord cx = ds_coord(w, ox[i], tj, a.W), cy = ds_coord(h, oy[i], ds_init<S>(i), a.H);
      const half8 v00 = *reinterpret_cast<const half8*>(xb + ((long)cy.c0 * a.W + cx.c0) * a.ldx);
      const half8 v01 = *reinterpret_cast<const half8*>(xb + ((long)cy.c0 * a.W + cx.c1) * a.ldx);
      const half8 v10 = *reinterpret_cast<const half8*>(xb + ((long)cy.c1 * a.W + cx.c0) * a.ldx);
      const half8 v11 = *reinterpret_cast<const half8*>(xb + ((long)cy.c1 * a.W + cx.c1) * a.ldx);
      const float ax = 1.f - cx.f, ay = 1.f - cy.f;
      const float w00 = ay * ax, w01 = ay * cx.f, w10 = cy.f * ax, w11 = cy.f * cx.f;
      half8 out;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        out[k] = (f16)(w00 * (float)v00[k] + w01 * (float)v01[k] + w10 * (float)v10[k] + w11 * (float)v11[k]);
      const long opix = (img * (S * a.H) + (S * h + i)) * (long)(S * a.W) + (S * w + j);
      *reinterpret_cast<half8*>(a.y + opix * a.ldy + part * 8) = out;
    }
  }
}

// Offset gradient: one lane per (base pixel, j, group) walks the s rows and the group's granules in a fixed order.
template <int S>
__global__ __launch_bounds__(256) void dysample_doff_kernel(DsArgs a) {
  const int SS = S * S;
  const long total = (long)a.N * a.H * a.W * S * a.G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int g, j, w, h;
    long t, pix, img;
    ds_divmod(idx, a.G, t, g);
    ds_divmod(t, S, pix, j);
    ds_divmod(pix, a.W, t, w);
    ds_divmod(t, a.H, img, h);
    const float* o = a.off + pix * a.ldoff + g * SS + j;
    const f16* xb = a.x + img * a.H * a.W * a.ldx + g * a.gpg * 8;
    f16* d = a.doff + pix * a.lddoff + g * SS + j;
    const float tj = ds_init<S>(j);
    for (int i = 0; i < S; ++i) {
      const DsCoord cx = ds_coord(w, o[i * S], tj, a.W), cy = ds_coord(h, o[a.G * SS + i * S], ds_init<S>(i), a.H);
      const long opix = (img * (S * a.H) + (S * h + i)) * (long)(S * a.W) + (S * w + j);
      const f16* gp = a.dy + opix * a.lddy + g * a.gpg * 8;
      const f16* p00 = xb + ((long)cy.c0 * a.W + cx.c0) * a.ldx;
      const f16* p01 = xb + ((long)cy.c0 * a.W + cx.c1) * a.ldx;
      const f16* p10 = xb + ((long)cy.c1 * a.W + cx.c0) * a.ldx;
      const f16* p11 = xb + ((long)cy.c1 * a.W + cx.c1) * a.ldx;
      const float ax = 1.f - cx.f, ay = 1.f - cy.f;
      float sx = 0.f, sy = 0.f;
      for (int q = 0; q < a.gpg; ++q) {
        const half8 v00 = *reinterpret_cast<const half8*>(p00 + q * 8), v01 = *reinterpret_cast<const half8*>(p01 + q * 8);
        const half8 v10 = *reinterpret_cast<const half8*>(p10 + q * 8), v11 = *reinterpret_cast<const half8*>(p11 + q * 8);
        const half8 g8 = *reinterpret_cast<const half8*>(gp + q * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float a00 = (float)v00[k], a01 = (float)v01[k], a10 = (float)v10[k], a11 = (float)v11[k], gg = (float)g8[k];
          sx += gg * (ay * (a01 - a00) + cy.f * (a11 - a10));
          sy += gg * (ax * (a10 - a00) + cx.f * (a11 - a01));
        }
      }
      d[i * S] = (f16)(cx.in ? 0.25f * sx : 0.f);
      d[a.G * SS + i * S] = (f16)(cy.in ? 0.25f * sy : 0.f);
    }
  }
}

// Largest |0.25 o| of the layer as the bit pattern of a non-negative float (integer max orders those and puts NaN above all).
__global__ __launch_bounds__(256) void dysample_maxabs_kernel(DsArgs a, int nch, unsigned* maxabs) {
  unsigned mbits = 0;
  const long total = (long)a.N * a.H * a.W * nch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int ch;
    long pix;
    ds_divmod(idx, nch, pix, ch);
    mbits = max(mbits, __float_as_uint(0.25f * a.off[pix * a.ldoff + ch]) & 0x7fffffffu);
  }
  for (int o = 1; o < 64; o <<= 1) mbits = max(mbits, (unsigned)__shfl_xor((int)mbits, o, 64));
  if ((threadIdx.x & 63) == 0 && mbits > __atomic_load_n(maxabs, __ATOMIC_RELAXED)) atomicMax(maxabs, mbits);
}

// A sample is NEAR when both |0.25 o| <= rmax - 1: with |init_pos| < 1/2 it lands less than rmax from its base pixel.
static __device__ __forceinline__ bool ds_has_far(unsigned bits, int rmax) { return !(__uint_as_float(bits) <= (float)(rmax - 1)); }
static __device__ __forceinline__ bool ds_is_far(float ox, float oy, float thr) {
  return !(fabsf(0.25f * ox) <= thr) || !(fabsf(0.25f * oy) <= thr);
}

__global__ __launch_bounds__(256) void ds_zero_if_far_kernel(float4* p, long n16, const unsigned* maxabs, int rmax) {
  if (!ds_has_far(*maxabs, rmax)) return;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Side pass: fp32-atomic scatter of the FAR samples only.  One lane per (output pixel, channel): the lanes of a sample's group are
// adjacent, so each corner's atomics cover a run of contiguous floats.
template <int S>
__global__ __launch_bounds__(256) void dysample_scatter_far_kernel(DsArgs a, const unsigned* maxabs, int rmax) {
  if (!ds_has_far(*maxabs, rmax)) return;
  const int SS = S * S, cpg = a.gpg * 8;
  const float thr = (float)(rmax - 1);
  const long total = (long)a.N * a.H * a.W * SS * a.C;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int c, k, w, h;
    long t, pix, img;
    ds_divmod(idx, a.C, t, c);
    ds_divmod(t, SS, pix, k);
    const int g = c / cpg, i = k / S, j = k - i * S;
    const float* o = a.off + pix * a.ldoff + g * SS + k;
    const float ox = o[0], oy = o[a.G * SS];
    if (!ds_is_far(ox, oy, thr)) continue;
    ds_divmod(pix, a.W, t, w);
    ds_divmod(t, a.H, img, h);
    const DsCoord cx = ds_coord(w, ox, ds_init<S>(j), a.W), cy = ds_coord(h, oy, ds_init<S>(i), a.H);
    const long opix = (img * (S * a.H) + (S * h + i)) * (long)(S * a.W) + (S * w + j);
    const float gg = (float)a.dy[opix * a.lddy + c];
    const float ax = 1.f - cx.f, ay = 1.f - cy.f;
    float* db = a.dx32 + img * a.H * a.W * a.C + c;
    atomicAdd(db + ((long)cy.c0 * a.W + cx.c0) * a.C, gg * (ay * ax));
    atomicAdd(db + ((long)cy.c0 * a.W + cx.c1) * a.C, gg * (ay * cx.f));
    atomicAdd(db + ((long)cy.c1 * a.W + cx.c0) * a.C, gg * (cy.f * ax));
    atomicAdd(db + ((long)cy.c1 * a.W + cx.c1) * a.C, gg * (cy.f * cx.f));
  }
}

// Input gradient by gather.  Thread = (input pixel (r, c), GP granules of one group).  A near sample at sub-position j of base column b
// lands at p = b + t[j] + d with |d| <= m, m = the largest |0.25 o| of the layer (rmax - 1 when it has far samples), and touches
// column c only when p is in [c - 1, c + 1): b in [c - 1 - t[j] - m, c + 1 - t[j] + m), two base columns per sub-position for a
// freshly initialised layer.  Clamped positions need no extension: a sample pulled in to column 0 or W-1 has its base inside the
// same range cut at the map's border.  The ranges carry 0.001 of slack for the fp32 rounding of p (over-wide only costs time), and
// every candidate is then tested exactly with ds_coord: column weight = [c0 == c](1 - f) + [c1 == c] f (both when the border folds
// the two corners onto one column, where f = 0), the same for rows, and the forward's four corner products factorise into
// row * column.  fp32 accumulation in a fixed order: run-to-run deterministic (the far side pass, when the layer has far samples
// at all, is not).
template <int S, int GP>
__global__ __launch_bounds__(256) void dysample_gather_kernel(DsArgs a, int accumulate, const unsigned* maxabs, int rmax) {
  const int SS = S * S;
  const unsigned mb = *maxabs;
  const bool has_far = ds_has_far(mb, rmax);
  const float thr = (float)(rmax - 1);
  const float ms = (has_far ? thr : __uint_as_float(mb)) + 0.001f;
  const int tpp = a.cpp / GP;  // threads per pixel
  const long total = (long)a.N * a.H * a.W * tpp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    int part, c, r;
    long t, ipix, img;
    ds_divmod(idx, tpp, ipix, part);
    ds_divmod(ipix, a.W, t, c);
    ds_divmod(t, a.H, img, r);
    const int g = part * GP / a.gpg;
    float acc[GP][8];
#pragma unroll
    for (int q = 0; q < GP; ++q)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[q][k] = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float ti = ds_init<S>(i);
      const int bh_lo = max((int)ceilf((float)r - 1.f - ti - ms), 0), bh_hi = min((int)floorf((float)r + 1.f - ti + ms), a.H - 1);
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const float tj = ds_init<S>(j);
        const int bw_lo = max((int)ceilf((float)c - 1.f - tj - ms), 0), bw_hi = min((int)floorf((float)c + 1.f - tj + ms), a.W - 1);
        for (int bh = bh_lo; bh <= bh_hi; ++bh) {
          for (int bw = bw_lo; bw <= bw_hi; ++bw) {
            const long pix = (img * a.H + bh) * a.W + bw;
            const float* o = a.off + pix * a.ldoff + g * SS + i * S + j;
            const float ox = o[0], oy = o[a.G * SS];
            if (ds_is_far(ox, oy, thr)) continue;  // the side pass owns it
            const DsCoord cx = ds_coord(bw, ox, tj, a.W);
            if (cx.c0 != c && cx.c1 != c) continue;
            const DsCoord cy = ds_coord(bh, oy, ti, a.H);
            if (cy.c0 != r && cy.c1 != r) continue;
            const float wc = (cx.c0 == c ? 1.f - cx.f : 0.f) + (cx.c1 == c ? cx.f : 0.f);
            const float wr = (cy.c0 == r ? 1.f - cy.f : 0.f) + (cy.c1 == r ? cy.f : 0.f);
            const float wgt = wr * wc;
            const long opix = (img * (S * a.H) + (S * bh + i)) * (long)(S * a.W) + (S * bw + j);
            const f16* gp = a.dy + opix * a.lddy + part * (GP * 8);
#pragma unroll
            for (int q = 0; q < GP; ++q) {
              const half8 g8 = *reinterpret_cast<const half8*>(gp + q * 8);
#pragma unroll
              for (int k = 0; k < 8; ++k) acc[q][k] += wgt * (float)g8[k];
            }
          }
        }
      }
    }
    if (has_far) {
      const float4* f = reinterpret_cast<const float4*>(a.dx32 + ipix * a.C + part * (GP * 8));
#pragma unroll
      for (int q = 0; q < GP; ++q) {
        const float4 f0 = f[2 * q], f1 = f[2 * q + 1];
        acc[q][0] += f0.x; acc[q][1] += f0.y; acc[q][2] += f0.z; acc[q][3] += f0.w;
        acc[q][4] += f1.x; acc[q][5] += f1.y; acc[q][6] += f1.z; acc[q][7] += f1.w;
      }
    }
    f16* d = a.dx + ipix * a.lddx + part * (GP * 8);
#pragma unroll
    for (int q = 0; q < GP; ++q) {
      half8 o8;
      if (accumulate) o8 = *reinterpret_cast<const half8*>(d + q * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) o8[k] = (f16)(acc[q][k] + (accumulate ? (float)o8[k] : 0.f));
      *reinterpret_cast<half8*>(d + q * 8) = o8;
    }
  }
}

extern "C" int dy_dysample_supported(int C, int G, int s) {
  return (s == 2 || s == 4) && G >= 1 && C >= 8 && G <= C / 8 && C % (8 * G) == 0;
}

static int ds_grid(long items, long cap) {
  long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

extern "C" int dy_dysample(const void* x, int ldx, const float* off, int ldoff, void* y, int ldy, int n, int H, int W, int C, int G,
                           int s, hipStream_t stream) {
  if (!x || !off || !y || n < 1 || H < 1 || W < 1 || !dy_dysample_supported(C, G, s)) return DY_ERR_ARG;
  if ((ldx & 7) || (ldy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)off & 3)) return DY_ERR_ALIGN;
  if (ldx < C || ldy < C || ldoff < 2 * G * s * s) return DY_ERR_ARG;
  DsArgs a{};
  a.x = (const f16*)x; a.off = off; a.y = (f16*)y; a.ldx = ldx; a.ldoff = ldoff; a.ldy = ldy;
  a.N = n; a.H = H; a.W = W; a.C = C; a.G = G; a.cpp = C >> 3; a.gpg = C / (8 * G);
  const int grid = ds_grid((long)n * H * W * s * a.cpp, 16384);
  if (s == 2) hipLaunchKernelGGL(dysample_fwd_kernel<2>, dim3(grid), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(dysample_fwd_kernel<4>, dim3(grid), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_dysample_backward(const void* x, int ldx, const float* off, int ldoff, const void* dy, int lddy, void* dx, int lddx,
                                    int accumulate, float* dx32, void* doff, int lddoff, void* scratch, int rmax, int n, int H, int W,
                                    int C, int G, int s, hipStream_t stream) {
  if (!x || !off || !dy || n < 1 || H < 1 || W < 1 || !dy_dysample_supported(C, G, s)) return DY_ERR_ARG;
  if (dx && (!dx32 || !scratch || rmax < 1 || rmax > 16)) return DY_ERR_ARG;
  if ((ldx & 7) || (lddy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || ((uintptr_t)off & 3)) return DY_ERR_ALIGN;
  if (dx && ((lddx & 7) || ((uintptr_t)dx & 15) || ((uintptr_t)dx32 & 15) || ((uintptr_t)scratch & 3))) return DY_ERR_ALIGN;
  if (doff && ((lddoff & 7) || ((uintptr_t)doff & 15))) return DY_ERR_ALIGN;
  const int nch = 2 * G * s * s;
  if (ldx < C || lddy < C || ldoff < nch || (dx && lddx < C) || (doff && lddoff < nch)) return DY_ERR_ARG;
  DsArgs a{};
  a.x = (const f16*)x; a.off = off; a.dy = (const f16*)dy; a.dx = (f16*)dx; a.dx32 = dx32; a.doff = (f16*)doff;
  a.ldx = ldx; a.ldoff = ldoff; a.lddy = lddy; a.lddx = lddx; a.lddoff = lddoff;
  a.N = n; a.H = H; a.W = W; a.C = C; a.G = G; a.cpp = C >> 3; a.gpg = C / (8 * G);
  const long npix = (long)n * H * W;
  if (doff) {
    const int grid = ds_grid(npix * s * G, 16384);
    if (s == 2) hipLaunchKernelGGL(dysample_doff_kernel<2>, dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(dysample_doff_kernel<4>, dim3(grid), dim3(256), 0, stream, a);
  }
  if (dx) {
    // the far side pass returns at once when the layer has no far sample (decided on the device: no host sync, the same launch
    // sequence every step, so the chain captures into a hipGraph)
    unsigned* maxabs = (unsigned*)scratch;
    if (hipMemsetAsync(maxabs, 0, 4, stream) != hipSuccess) return DY_ERR_LAUNCH;
    hipLaunchKernelGGL(dysample_maxabs_kernel, dim3(ds_grid(npix * nch, 1024)), dim3(256), 0, stream, a, nch, maxabs);
    hipLaunchKernelGGL(ds_zero_if_far_kernel, dim3(2048), dim3(256), 0, stream, (float4*)dx32, npix * C / 4, maxabs, rmax);
    const int gp = (a.gpg & 1) ? 1 : 2;  // granules per gather thread: two where a group holds an even number (one geometry for both)
    const int sg = ds_grid(npix * s * s * C, 4096), gg = ds_grid(npix * (a.cpp / gp), 65536);
    if (s == 2) {
      hipLaunchKernelGGL(dysample_scatter_far_kernel<2>, dim3(sg), dim3(256), 0, stream, a, maxabs, rmax);
      if (gp == 2) hipLaunchKernelGGL((dysample_gather_kernel<2, 2>), dim3(gg), dim3(256), 0, stream, a, accumulate, maxabs, rmax);
      else hipLaunchKernelGGL((dysample_gather_kernel<2, 1>), dim3(gg), dim3(256), 0, stream, a, accumulate, maxabs, rmax);
    } else {
      hipLaunchKernelGGL(dysample_scatter_far_kernel<4>, dim3(sg), dim3(256), 0, stream, a, maxabs, rmax);
      if (gp == 2) hipLaunchKernelGGL((dysample_gather_kernel<4, 2>), dim3(gg), dim3(256), 0, stream, a, accumulate, maxabs, rmax);
      else hipLaunchKernelGGL((dysample_gather_kernel<4, 1>), dim3(gg), dim3(256), 0, stream, a, accumulate, maxabs, rmax);
    }
  }
  DY_CHECK_LAUNCH();
  return DY_OK;
}
