// Bootstrap resampling of the validation statistics: AP of every (resample, class, IoU threshold) in ONE launch.
//
// Replaces the loop of reference testandcox.py:150-227 -- per resample a temporary dataset file and a full ``model.val`` -- by
// ``compute_ap`` / ``ap_per_class`` (ultralytics/utils/metrics.py) evaluated on the statistics of ONE validation pass, in which
// every detection and label of image i counts ``mult[s, i]`` times in resample s.  Neither the resampled list nor an S x D array
// exists anywhere: one 256-thread workgroup per (resample, class) walks the class's detections (sorted by confidence, descending)
// in 256-detection chunks and keeps O(1) state between chunks.
//
// What ``compute_ap`` computes, in terms of the weighted list.  Replica r (1..m) of detection d is a point with
// tpc = Tb + r b, fpc = Fb + r (1 - b) (Tb / Fb: weighted true / false positives before d; b: its flag at the threshold),
// recall = tpc / (n_l + 1e-16), precision = tpc / (tpc + fpc); the curve gets the sentinels (0, 1) and (1, 0), the precision is
// replaced by its right-to-left running maximum (the envelope), np.interp samples it at x_k = k / 100 and the trapezoid rule
// integrates.  np.interp picks, for x, the LAST node whose recall is <= x; if that recall equals x the result is the envelope there,
// otherwise the line to the next node -- the FIRST node of the next recall value.  Nodes group by their integer true-positive
// count t ("level" t: the replica that reaches t, then the false positives up to the next true positive; level 0 holds the
// sentinel and the leading false positives).  With P(t) the precision of the replica that reaches t and S(t) = max_{t' >= t} P(t'):
//   envelope at the first node of level t >= 1:  S(t)            (a false positive's precision is below the next true positive's)
//   envelope at the last node of level t < T:    S(t) if the level is that single node (1.0 for t = 0), else S(t + 1)
//   envelope at the last node of level T:        T / N           (T, N: weighted true positives / detections of the whole list)
// and the sentinel (1, 0) follows.  So the 101 samples need S and the false-positive count at the levels t_k and t_k + 1 only,
// t_k = the largest t with t / (n_l + 1e-16) <= x_k, which depends on n_l alone.  Within one detection the replicas' precision rises,
// so its last replica (e = Tb + m) stands for the levels Tb + 1 .. e: S(t) = the maximum of e / (e + Fb) over the true-positive
// detections from the one that owns level t to the end of the list.
//
// Pass 1 sums n_l, N and the ten T.  Pass 2 walks the chunks from the last to the first: a weighted wave scan (+ LDS across the four
// waves) rebuilds (Tb, Fb) of every detection from the running totals, a suffix-maximum scan over the chunk joined with the maximum
// carried from the later chunks gives S at every true positive, and the detections that own a level t_k or t_k + 1 write (S, Fb)
// into two 100-entry LDS tables per threshold.  All counts are integers; quotients and the integral are fp64.
#include "common.h"
#include "dealyolo_hip.h"
#pragma clang fp contract(off)  // the quotients and the interpolation as numpy evaluates them (no fused multiply-add)

#define BS_THREADS 256
#define BS_WAVES 4
#define BS_NT 10         // IoU thresholds of the validator: bit j of tp_bits
#define BS_GRID 100      // grid points below 1.0 (x_100 = 1.0 always samples the sentinel: 0)
#define BS_LDS_IMGS 8192 // a resample's multiplicity row is staged in LDS up to this many images, gathered from global beyond

struct BsArgs {
  const unsigned short* tp_bits;  // (D)
  const int* det_img;             // (D)
  const int* cls_off;             // (nc + 1)
  const int* lab_cnt;             // (n_img, nc)
  const unsigned short* mult;     // (S, n_img)
  double* ap;                     // (S, nc, 10)
  int* nl;                        // (S, nc)
  int D, n_img, nc;
};

__global__ __launch_bounds__(BS_THREADS) void bootstrap_ap_kernel(BsArgs a) {
  __shared__ unsigned short mrow[BS_LDS_IMGS];
  __shared__ double envA[BS_NT][BS_GRID], envB[BS_NT][BS_GRID];  // S at level t_k / t_k + 1
  __shared__ unsigned fpA[BS_NT][BS_GRID], fpB[BS_NT][BS_GRID];  // false positives before the replica that reaches the level
  __shared__ double ycurve[BS_NT][BS_GRID + 1];
  __shared__ long long lvl[BS_GRID];                              // t_k
  __shared__ unsigned long long tot[BS_NT + 2];                   // N, T_0 .. T_9, n_l
  __shared__ unsigned wsum[2][BS_WAVES][BS_NT + 1];
  __shared__ double wmax[2][BS_WAVES][BS_NT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / a.nc, c = blockIdx.x - s * a.nc;
  const unsigned short* mg = a.mult + (size_t)s * a.n_img;
  const bool staged = a.n_img <= BS_LDS_IMGS;
  if (staged)
    for (int i = tid; i < a.n_img; i += BS_THREADS) mrow[i] = mg[i];
  if (tid < BS_NT + 2) tot[tid] = 0ull;
  __syncthreads();
  int d0 = a.cls_off[c], d1 = a.cls_off[c + 1];
  d0 = min(max(d0, 0), a.D);
  d1 = min(max(d1, d0), a.D);

  // ---- pass 1: labels of the class in this resample, weighted detections and true positives per threshold
  {
    unsigned long long acc[BS_NT + 1], labs = 0ull;
#pragma unroll
    for (int i = 0; i <= BS_NT; ++i) acc[i] = 0ull;
    for (int i = tid; i < a.n_img; i += BS_THREADS)
      labs += (unsigned long long)(staged ? mrow[i] : mg[i]) * (unsigned long long)max(a.lab_cnt[(size_t)i * a.nc + c], 0);
    for (int d = d0 + tid; d < d1; d += BS_THREADS) {
      const int img = a.det_img[d];
      const unsigned m = (img >= 0 && img < a.n_img) ? (staged ? mrow[img] : mg[img]) : 0u;
      const unsigned bits = a.tp_bits[d];
      acc[0] += m;
#pragma unroll
      for (int j = 0; j < BS_NT; ++j) acc[1 + j] += ((bits >> j) & 1u) ? m : 0u;
    }
#pragma unroll
    for (int i = 0; i <= BS_NT; ++i)
      if (acc[i]) atomicAdd(&tot[i], acc[i]);
    if (labs) atomicAdd(&tot[BS_NT + 1], labs);
  }
  __syncthreads();
  const long long n_l = (long long)tot[BS_NT + 1], N = (long long)tot[0];
  if (tid == 0) a.nl[blockIdx.x] = (int)n_l;
  double* out = a.ap + (size_t)blockIdx.x * BS_NT;
  if (n_l == 0 || N == 0) {  // ap_per_class: ``if n_p == 0 or n_l == 0: continue`` leaves the row at zero
    if (tid < BS_NT) out[tid] = 0.0;
    return;
  }
  const double den = (double)n_l + 1e-16;

  // ---- t_k: the largest t with t / (n_l + 1e-16) <= x_k, by the very comparison np.interp's search makes
  if (tid < BS_GRID) {
    const double x = tid * (1.0 / 100);
    long long t = (long long)(x * den);
    while ((double)(t + 1) / den <= x) ++t;
    while (t > 0 && (double)t / den > x) --t;
    lvl[tid] = t;
  }
  __syncthreads();
  for (int i = tid; i < BS_NT * BS_GRID; i += BS_THREADS) {
    const int j = i / BS_GRID, k = i - j * BS_GRID;
    envA[j][k] = lvl[k] == 0 ? 1.0 : 0.0;  // level 0 starts at the sentinel (0, 1), no false positive before it
    envB[j][k] = 0.0;
    fpA[j][k] = 0u;
    fpB[j][k] = 0u;
  }
  __syncthreads();

  // ---- pass 2: chunks from the last to the first
  const double inv = 100.0 / den;  // level -> grid index, a lower bound good to +-1 (the table decides)
  long long Tend[BS_NT], Nend = N;  // weighted counts up to the end of the current chunk
  double R[BS_NT];                  // max precision over the true positives of the later chunks
#pragma unroll
  for (int j = 0; j < BS_NT; ++j) {
    Tend[j] = (long long)tot[1 + j];
    R[j] = 0.0;
  }
  const int nchunk = (d1 - d0 + BS_THREADS - 1) / BS_THREADS;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int par = ch & 1;
    const int d = d0 + ch * BS_THREADS + tid;
    unsigned m = 0u, bits = 0u;
    if (d < d1) {
      const int img = a.det_img[d];
      m = (img >= 0 && img < a.n_img) ? (staged ? mrow[img] : mg[img]) : 0u;
      bits = a.tp_bits[d];
    }
    unsigned w[BS_NT + 1];  // inclusive weighted scan: detections, true positives per threshold
    w[0] = m;
#pragma unroll
    for (int j = 0; j < BS_NT; ++j) w[1 + j] = ((bits >> j) & 1u) ? m : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
      for (int i = 0; i <= BS_NT; ++i) {
        const unsigned t = __shfl_up(w[i], o, 64);
        if (lane >= o) w[i] += t;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i <= BS_NT; ++i) wsum[par][wave][i] = w[i];
    }
    __syncthreads();
    unsigned ctot[BS_NT + 1];
#pragma unroll
    for (int i = 0; i <= BS_NT; ++i) {
      unsigned p = 0u, t = 0u;
#pragma unroll
      for (int ww = 0; ww < BS_WAVES; ++ww) {
        const unsigned x = wsum[par][ww][i];
        t += x;
        if (ww < wave) p += x;
      }
      w[i] += p;
      ctot[i] = t;
    }
    const long long nb = Nend - (long long)ctot[0] + (long long)w[0] - (long long)m;  // weighted detections before this one
    double v[BS_NT];
#pragma unroll
    for (int j = 0; j < BS_NT; ++j) {
      v[j] = 0.0;
      if (m && ((bits >> j) & 1u)) {
        const long long e = Tend[j] - (long long)ctot[1 + j] + (long long)w[1 + j];  // true positives up to its last replica
        const long long fb = nb - (e - (long long)m);
        v[j] = (double)e / (double)(e + fb);
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
      for (int j = 0; j < BS_NT; ++j) {
        const double t = __shfl_down(v[j], o, 64);
        if (lane + o < 64) v[j] = fmax(v[j], t);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < BS_NT; ++j) wmax[par][wave][j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BS_NT; ++j) {
      double later = R[j], all = R[j];
#pragma unroll
      for (int ww = 0; ww < BS_WAVES; ++ww) {
        const double x = wmax[par][ww][j];
        all = fmax(all, x);
        if (ww > wave) later = fmax(later, x);
      }
      if (m && ((bits >> j) & 1u)) {
        const double sfx = fmax(v[j], later);  // S at the levels this detection owns
        const long long hi = Tend[j] - (long long)ctot[1 + j] + (long long)w[1 + j], lo = hi - (long long)m + 1;
        const unsigned fb = (unsigned)(nb - (lo - 1));
        const double q = (double)(lo - 1) * inv;
        int k = q >= (double)BS_GRID ? BS_GRID : max((int)q - 2, 0);
        while (k < BS_GRID && lvl[k] < lo - 1) ++k;
        for (; k < BS_GRID && lvl[k] <= hi; ++k) {
          const long long t = lvl[k];
          if (t >= lo) {  // level t_k
            envA[j][k] = sfx;
            fpA[j][k] = fb;
          }
          if (t < hi) {  // level t_k + 1
            envB[j][k] = sfx;
            fpB[j][k] = fb;
          }
        }
      }
      R[j] = all;
      Tend[j] -= (long long)ctot[1 + j];
    }
    Nend -= (long long)ctot[0];
  }
  __syncthreads();

  // ---- the 101 samples of np.interp(x, mrec, envelope) and their trapezoid integral
  for (int i = tid; i < BS_NT * (BS_GRID + 1); i += BS_THREADS) {
    const int j = i / (BS_GRID + 1), k = i - j * (BS_GRID + 1);
    double y = 0.0;  // x = 1.0: the last node with recall <= 1 is the sentinel (1, 0)
    if (k < BS_GRID) {
      const long long T = (long long)tot[1 + j];
      const double x = k * (1.0 / 100);
      const long long t = lvl[k] < T ? lvl[k] : T;
      const double r = (double)t / den;
      double left, right, rn;
      if (t >= T) {  // last level: its last node, then the sentinel
        left = (double)T / (double)N;
        right = 0.0;
        rn = 1.0;
      } else {
        left = fpA[j][k] == fpB[j][k] ? envA[j][k] : envB[j][k];
        right = envB[j][k];
        rn = (double)(t + 1) / den;
      }
      y = r == x ? left : (right - left) / (rn - r) * (x - r) + left;
    }
    ycurve[j][k] = y;
  }
  __syncthreads();
  if (tid < BS_NT) {
    double sum = 0.0;
    for (int k = 0; k < BS_GRID; ++k) {
      const double x0 = k * (1.0 / 100), x1 = k + 1 < BS_GRID ? (k + 1) * (1.0 / 100) : 1.0;
      sum += (x1 - x0) * (ycurve[tid][k + 1] + ycurve[tid][k]) / 2.0;
    }
    out[tid] = sum;
  }
}

extern "C" int dy_bootstrap_ap(const unsigned short* tp_bits, const int* det_img, const int* cls_off, const int* lab_cnt,
                               const unsigned short* mult, int D, int n_img, int nc, int S, double* ap, int* nl,
                               hipStream_t stream) {
  if (D < 0 || n_img < 1 || nc < 1 || S < 1 || !cls_off || !lab_cnt || !mult || !ap || !nl) return DY_ERR_ARG;
  if (D > 0 && (!tp_bits || !det_img)) return DY_ERR_ARG;
  if ((long)S * nc > 0x7fffffffL) return DY_ERR_ARG;
  BsArgs a{tp_bits, det_img, cls_off, lab_cnt, mult, ap, nl, D, n_img, nc};
  hipLaunchKernelGGL(bootstrap_ap_kernel, dim3(S * nc), dim3(BS_THREADS), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
