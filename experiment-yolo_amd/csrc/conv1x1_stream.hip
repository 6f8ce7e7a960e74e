// Streaming 1x1 convolution on MFMA (v_mfma_f32_16x16x32_f16) for NHWC fp16 activations: the forward pass and the input gradient of
// every 1x1 Conv of the training step (reference nn/modules/conv.py:49-55 and its autograd backward) whose weights fit a wave's registers.
//
// A 1x1 layer is a plain stream of [pixels x Cin] . [Cin x Cout] at about 32 FLOP per byte: there is no halo to share and 8-32 KB of
// weights, so none of what conv_mfma_pp_kernel (conv.hip) builds for 3x3 layers -- a resident weight image in LDS, staged activation
// tiles, two wave groups swapping roles between workgroup barriers -- pays here.  Instead
//   * every wave is on its own: it walks wave tiles of NT x 16 pixels of its work list and meets no barrier before the statistics tail;
//   * the cout group's A fragments are loaded once and stay in registers (NKS * MT * 4 VGPRs);
//   * the B fragments come STRAIGHT from global memory in the MFMA operand layout -- lane (p, q) reads the 16 bytes of pixel p, channels
//     32 k + 8 q .. + 7 -- so the input is never transposed and a segmented input (DySegs) costs one base pointer per k-step;
//   * two wave tiles of loads are in flight per wave beside the one being multiplied (register double buffer, the compiler's counted
//     s_waitcnt vmcnt), and the old values of an accumulating store are requested one tile ahead;
//   * results leave through the per-wave LDS transpose of the ping-pong kernel's fast epilogue (wavefront-scope fences only), so that
//     consecutive lanes write one pixel's whole channel block.
// GEMM orientation (M = Cout from the packed weights, N = pixels), MFMA and k order are those of conv_mfma_pp_kernel's 1x1 branch:
// every output element is the same chain of MFMAs and has the same bits.  BatchNorm sums are taken from the fp32 accumulators and
// leave through the same fp64 accumulator copies (blockIdx.x % DY_BN_COPIES); launches with sums run on the ping-pong kernel's pixel
// map (PP below), so the sums have its bits too.
#include "conv1x1_stream.h"
#include <stdio.h>
#include <type_traits>

#define DY_STREAM_WAVES 4        // waves per workgroup
#define DY_STREAM_WGS_PER_CU 2   // 8 waves per CU, two per SIMD (each holds up to 256 VGPRs)

// floor(a / d) for 0 <= a < 2^24 with inv = 1.0f / d: the float quotient is off by at most one
static __device__ __forceinline__ int div_f(int a, int d, float inv) {
  int qv = (int)((float)a * inv);
  const int r = a - qv * d;
  qv += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
  return qv;
}

// PP ("ping-pong pixel map", the launches with BatchNorm statistics): the workgroup is the ping-pong kernel's -- eight waves, wave w = 4 g + wg
// owns pixels [64 wg, 64 wg + 64) of the 256-pixel tiles 2 blockIdx.x + g, + 2 gridDim.x, ... on the grid pp_grid gives that kernel -- so
// every lane adds the pixels conv_mfma_pp_kernel's lane would add, in its order, the rows and the eight waves are reduced the same way,
// and each workgroup adds the SAME fp32 partial sums to the same accumulator copy: the statistics, and with them every number a
// training run computes, keep the ping-pong kernel's bits.  The other launches have no sums to keep and take the free-running map.
template <int NKS, int MT, bool PP>
__global__ __launch_bounds__((PP ? 8 : DY_STREAM_WAVES) * 64, PP ? 1 : DY_STREAM_WGS_PER_CU) void conv1x1_stream_kernel(Conv1x1StreamArgs a) {
  constexpr int NW = PP ? 8 : DY_STREAM_WAVES;          // waves per workgroup
  constexpr int NT = NKS <= 2 ? 4 : 2;                  // 16-pixel N-tiles per wave tile (B double buffer: 2 * NT * NKS * 4 VGPRs)
  constexpr int TP = NT * 16;                           // pixels per wave tile
  constexpr int NC = 4 * MT;                            // consecutive output channels a lane holds per pixel
  constexpr int RB = 4 * NC * 2;                        // bytes of one pixel's channel block of this cout group
  constexpr int XROW = RB + 16;                         // pitch of the per-wave store-transpose scratch (16 rows)
  constexpr int PPR = RB / 16;                          // 16-byte pieces per pixel row
  constexpr int PIXPASS = 64 / PPR;                     // pixels one store instruction covers
  constexpr int NPASS = PIXPASS >= 16 ? 1 : 16 / PIXPASS;
  __shared__ __attribute__((aligned(16))) char lds[NW * 16 * XROW];

  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, p = lane & 15, q = lane >> 4;
  const int grp = blockIdx.y;
  // the wave's work list: unit u is the wave tile that starts at pixel pix_of(u) (a.npix: none)
  const int ntiles = PP ? (a.npix + 255) / 256 : (a.npix + TP - 1) / TP;
  const int stride = PP ? 2 * gridDim.x : gridDim.x * NW;
  const int tile0 = PP ? blockIdx.x * 2 + (wave >> 2) : blockIdx.x * NW + wave;
  constexpr int SUB = PP ? 64 / TP : 1;                  // wave tiles per 64-pixel block of a ping-pong tile
  const int nunits = tile0 < ntiles ? ((ntiles - tile0 + stride - 1) / stride) * SUB : 0;
  auto pix_of = [&](int u) {
    if (u >= nunits) return a.npix;
    if (PP) return (tile0 + (u / SUB) * stride) * 256 + (wave & 3) * 64 + (u % SUB) * TP;
    return (tile0 + u * stride) * TP;
  };

  // ---- A fragments of this cout group: resident in registers for the whole launch
  half8 af[NKS][MT];
#pragma unroll
  for (int k = 0; k < NKS; ++k)
#pragma unroll
    for (int m = 0; m < MT; ++m)
      af[k][m] = *reinterpret_cast<const half8*>(a.w + ((size_t)((grp * NKS + k) * (16 * MT) + m * 16 + p) * 32 + q * 8));

  // ---- where this lane's 8 channels of k-step k live: base pointer at the channel, pixel stride in bytes (bit 31: up-sampled segment)
  const char* xb[NKS];
  unsigned xld[NKS];
  bool anyup = false;
#pragma unroll
  for (int k = 0; k < NKS; ++k) {
    const int c = k * a.cpk + ((q * 8) & (a.cpk - 1));  // (16-channel steps: lanes q >= 2 meet zero weights and re-read channels 0-15)
    int sg = 0;
    while (sg + 1 < a.xs.nseg && c >= a.xs.c_end[sg]) ++sg;
    const int cb = sg ? a.xs.c_end[sg - 1] : 0;
    xb[k] = reinterpret_cast<const char*>(a.xs.ptr[sg]) + (c - cb) * 2;
    const bool up = (a.xs.acc[sg] & 2) != 0;
    xld[k] = ((unsigned)a.xs.ld[sg] * 2u) | (up ? 0x80000000u : 0u);
  }
  for (int s = 0; s < a.xs.nseg; ++s) anyup = anyup || (a.xs.acc[s] & 2) != 0;  // wave-uniform
  const int hw = a.H * a.W, Hh = a.H >> 1, Wh = a.W >> 1;
  const float inv_hw = 1.0f / (float)hw, inv_w = 1.0f / (float)a.W;

  // B fragments of wave tile `tile` -> registers.  Every load is unconditional: pixels past the end (and whole tiles past the last one,
  // which the prefetch runs into) re-read the last pixel; nothing of them is stored or summed.
  auto issue = [&](half8 (&b)[NT][NKS], int pix0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int gp = pix0 + t * 16 + p;
      gp = gp < a.npix ? gp : a.npix - 1;
      int gu = gp;
      if (anyup) {  // pixel (n, y, x) of the concatenation reads (n, y >> 1, x >> 1) of the low-resolution tensor
        const int n = div_f(gp, hw, inv_hw), r = gp - n * hw;
        const int yy = div_f(r, a.W, inv_w), xx = r - yy * a.W;
        gu = (n * Hh + (yy >> 1)) * Wh + (xx >> 1);
      }
#pragma unroll
      for (int k = 0; k < NKS; ++k) {
        const unsigned ldb = xld[k] & 0x7fffffffu;
        const int px = (xld[k] >> 31) ? gu : gp;
        b[t][k] = *reinterpret_cast<const half8*>(xb[k] + (size_t)px * ldb);
      }
    }
  };

  // ---- epilogue addressing (conv_mfma_pp_kernel's fast epilogue, for a wave that owns TP consecutive pixels)
  char* const xs = lds + wave * (16 * XROW);
  const int dpix = lane / PPR, piece = lane % PPR;
  const int chn = grp * (16 * MT) + piece * 8;          // first channel of this lane's stores
  const bool chok = chn < a.cout;                        // padded cout groups: whole 8-channel pieces drop
  const unsigned loff = (unsigned)((dpix * a.ldy + chn) * 2);
  char* const xw = xs + p * XROW + q * (NC * 2);
  const char* const xr = xs + dpix * XROW + piece * 16;
  // segmented output: this lane's piece lives in ONE segment for the whole launch
  char* sbase = nullptr;
  unsigned sld2 = 0;
  bool sacc = false, seg_any_acc = false;
  if (a.ys.nseg > 0) {
    int sg = 0;
    while (sg + 1 < a.ys.nseg && chn >= a.ys.c_end[sg]) ++sg;
    const int cb = sg ? a.ys.c_end[sg - 1] : 0;
    sbase = reinterpret_cast<char*>(const_cast<void*>(a.ys.ptr[sg])) + (chn - cb) * 2;
    sld2 = (unsigned)a.ys.ld[sg] * 2u;
    sacc = a.ys.acc[sg] != 0;
    for (int s = 0; s < a.ys.nseg; ++s) seg_any_acc = seg_any_acc || a.ys.acc[s] != 0;
  }
  f32x2 s1[NC / 2], s2[NC / 2];
#pragma unroll
  for (int j = 0; j < NC / 2; ++j) s1[j] = s2[j] = (f32x2){0.f, 0.f};

  typedef uint2 __attribute__((may_alias)) uint2_a;
  typedef uint4 __attribute__((may_alias)) uint4_a;
  union U4 { uint4 u; half2_ h[4]; };

  auto run = [&](auto acc_tag, auto stats_tag, auto segy_tag) {
    constexpr bool ACCUM = decltype(acc_tag)::value, STATS = decltype(stats_tag)::value, SEGY = decltype(segy_tag)::value;
    // lanes exchange data through LDS inside one wave: the hardware keeps a wave's LDS operations in order, the fences keep the compiler
    // from moving N-tile t+1's write above N-tile t's read (LDS address space only: no wait for earlier global stores)
    auto lds_order = []() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    };
    auto dest = [&](int wp0, int t, int ps, bool& valid) {
      const int c0 = t * 16 + ps * PIXPASS;  // wave-uniform
      valid = chok && dpix < 16 && c0 + dpix < a.npix - wp0;
      if (SEGY) {
        char* const pzs = sbase + (size_t)(unsigned)(wp0 + c0 + dpix) * sld2;
        return reinterpret_cast<uint4*>(valid ? pzs : reinterpret_cast<char*>(const_cast<void*>(a.ys.ptr[0])));
      }
      // lanes without a destination get the tensor base: the accumulate variant LOADS through this pointer whatever `valid` says
      char* const pz = reinterpret_cast<char*>(a.y) + (long)(wp0 + c0) * a.ldy * 2 + loff;
      return reinterpret_cast<uint4*>(valid ? pz : reinterpret_cast<char*>(a.y));
    };
    U4 o[ACCUM ? NT : 1][NPASS];  // old values of the tile whose epilogue comes next
    auto issue_old = [&](int pix0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
          bool valid;
          uint4* const pd = dest(pix0, t, ps, valid);
          o[ACCUM ? t : 0][ps].u = (!SEGY || (valid && sacc)) ? *pd : make_uint4(0, 0, 0, 0);  // only segments that accumulate have one
        }
    };
    f32x4 acc[MT][NT];
    auto convert_write = [&](int t, int collim) {
      union { half2_ h[NC / 2]; uint4 u4[NC / 8 > 0 ? NC / 8 : 1]; uint2 u2; } hv;
      const float keep = (t * 16 + p < collim) ? 1.f : 0.f;
      const f32x2 k2 = {keep, keep};
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const f32x2 lo = {acc[m][t][0], acc[m][t][1]}, hi = {acc[m][t][2], acc[m][t][3]};
        hv.h[m * 2] = __builtin_convertvector(lo, half2_);
        hv.h[m * 2 + 1] = __builtin_convertvector(hi, half2_);
        if (STATS) {  // BatchNorm sums from the fp32 accumulators, pixels past the end masked by 0 / 1
          const f32x2 l2 = lo * k2, h2 = hi * k2;
          s1[m * 2] += l2; s1[m * 2 + 1] += h2;
          s2[m * 2] += l2 * lo; s2[m * 2 + 1] += h2 * hi;
        }
      }
      if (NC == 4) {
        *reinterpret_cast<uint2_a*>(xw) = hv.u2;
      } else {
#pragma unroll
        for (int jj = 0; jj < NC / 8; ++jj) reinterpret_cast<uint4_a*>(xw)[jj] = hv.u4[jj];
      }
    };
    // one wave tile: multiply from b, refill b with the tile two steps ahead, then convert / transpose / store
    auto step = [&](half8 (&b)[NT][NKS], int u) {
      const int pix0 = pix_of(u);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NKS; ++k)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[k][m], b[t][k], acc[m][t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue(b, pix_of(u + 2));
      __builtin_amdgcn_sched_barrier(0);
      const int collim = a.npix - pix0;
      U4 d[2][NPASS];
      convert_write(0, collim);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        lds_order();
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) d[t & 1][ps].u = *reinterpret_cast<const uint4_a*>(xr + ps * PIXPASS * XROW);
        lds_order();
        if (t + 1 < NT) convert_write(t + 1, collim);
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
          bool valid;
          uint4* const yp = dest(pix0, t, ps, valid);
          U4 v = d[t & 1][ps];
          if (ACCUM) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              v.h[k] = __builtin_convertvector(__builtin_convertvector(v.h[k], f32x2) + __builtin_convertvector(o[ACCUM ? t : 0][ps].h[k], f32x2), half2_);
          }
          if (valid) *yp = v.u;
        }
      }
      if (ACCUM) {  // after this tile's stores; the next tile's input is already in flight in front of them
        __builtin_amdgcn_sched_barrier(0);
        issue_old(pix_of(u + 1));
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    half8 b0[NT][NKS], b1[NT][NKS];
    if (nunits > 0) {
      issue(b0, pix_of(0));
      issue(b1, pix_of(1));
      if (ACCUM) issue_old(pix_of(0));
      __builtin_amdgcn_sched_barrier(0);
      for (int u = 0; u < nunits; u += 2) {
        step(b0, u);
        if (u + 1 >= nunits) break;
        step(b1, u + 1);
      }
    }
  };
  constexpr std::true_type Y{};
  constexpr std::false_type N_{};
  if constexpr (PP) {
    run(N_, Y, N_);
  } else {
    if (a.ys.nseg > 0) {
      if (seg_any_acc) run(Y, N_, Y);
      else run(N_, N_, Y);
    } else if (a.epi & DY_EPI_ACCUM) run(Y, N_, N_);
    else run(N_, N_, N_);
  }

  if constexpr (PP) {
    // lanes of a row -> one value, waves -> LDS, then one fp64 atomic add per (sum, channel) into this workgroup's accumulator copy
    __syncthreads();  // (every wave is done with its transpose scratch)
    float* red = reinterpret_cast<float*>(lds);  // [wave][2][16*MT]
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float r1 = quad16_sum(s1[j >> 1][j & 1]), r2 = quad16_sum(s2[j >> 1][j & 1]);
      if (p == 0) {
        red[(wave * 2 + 0) * (16 * MT) + q * NC + j] = r1;
        red[(wave * 2 + 1) * (16 * MT) + q * NC + j] = r2;
      }
    }
    __syncthreads();
    if (tid < 2 * 16 * MT) {
      const int which = tid / (16 * MT), ch = tid - which * (16 * MT);
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) sum += red[(w * 2 + which) * (16 * MT) + ch];
      const int ctot = (a.cout + 15) & ~15, c = grp * (16 * MT) + ch;
      if (c < ctot) unsafeAtomicAdd(a.acc + ((size_t)(blockIdx.x % DY_BN_COPIES) * 2 + which) * ctot + c, (double)sum);
    }
  }
}

int conv1x1_stream_has(int nks, int mt) { return nks >= 1 && nks <= DY_STREAM_MAX_KSTEPS && (mt == 1 || mt == 2 || mt == 4); }

template <int NKS, int MT>
static int launch_stream(const Conv1x1StreamArgs& a, int ngroups, hipStream_t s) {
  if (a.epi & DY_EPI_STATS) {  // the ping-pong kernel's workgroups and pixel map: its grid
    if (a.pp_grid <= 0) return DY_ERR_ARG;
    hipLaunchKernelGGL((conv1x1_stream_kernel<NKS, MT, true>), dim3(a.pp_grid, ngroups), dim3(512), 0, s, a);
    DY_CHECK_LAUNCH();
    return DY_OK;
  }
  constexpr int TP = (NKS <= 2 ? 4 : 2) * 16;
  const int ntiles = cdiv(a.npix, TP);
  // one cout group: every workgroup resident at once (two per CU); two groups halve the grid each, so that together they are; with more
  // groups the later ones wait for a free slot (grid-stride loops: residency is a matter of speed only)
  const int cap = DY_NUM_CUS * DY_STREAM_WGS_PER_CU / (ngroups >= 2 ? 2 : 1);
  int gx = cdiv(ntiles, DY_STREAM_WAVES);
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL((conv1x1_stream_kernel<NKS, MT, false>), dim3(gx, ngroups), dim3(DY_STREAM_WAVES * 64), 0, s, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

int conv1x1_stream_launch(const Conv1x1StreamArgs& a, int nks, int mt, int ngroups, hipStream_t stream) {
  if (a.npix <= 0 || ngroups <= 0) return DY_ERR_ARG;
#define DY_SCASE(K, M) if (nks == K && mt == M) return launch_stream<K, M>(a, ngroups, stream);
  DY_SCASE(1, 1) DY_SCASE(1, 2) DY_SCASE(1, 4)
  DY_SCASE(2, 1) DY_SCASE(2, 2) DY_SCASE(2, 4)
  DY_SCASE(3, 1) DY_SCASE(3, 2) DY_SCASE(3, 4)
  DY_SCASE(4, 1) DY_SCASE(4, 2) DY_SCASE(4, 4)
#undef DY_SCASE
  return DY_ERR_ARG;
}
