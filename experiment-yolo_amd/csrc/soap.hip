// SOAP ("Shampoo with Adam in the preconditioner's eigenbasis", arXiv 2409.11321) as the reference trainer ships it
// (engine/trainer.py:54-473), over the flat fp32 parameter / gradient buffers: one table-driven launch per kind of work in place of
// the ~35 ATen calls per tensor of the host-driven restatement (ultralytics/hip/soap.py, class Soap).  The table (DySoapDesc,
// include/dealyolo_hip.h) has one entry per trainable tensor; a launch finds its tensor by a binary search over the first-block
// columns of the table, so the number of launches does not depend on the number of tensors.
//
// Numerics: plain fp32 FMAs, every dot product summed by ONE thread (rotation) or by one workgroup in a fixed order (Gram), no float
// atomics anywhere: two runs from the same state give the same bits.  Every kernel reads found_inf (state[2]) and leaves its outputs
// untouched when it is set.
#include "common.h"
#include "dealyolo_hip.h"

#define SOAP_EW 1024  // elements per workgroup of the element-wise kernels / of a pass-through copy
#define SOAP_T 32     // tile edge of the rotation and Gram kernels

// the last tensor whose first workgroup in this launch (first_block(i): a *_blk column of the table, non-decreasing in i) is <= bid
template <typename F>
static __device__ __forceinline__ int find_tensor(int nt, int bid, F first_block) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first_block(mid) <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// (A, n, B) around dimension k of a tensor
static __device__ __forceinline__ void mode_geometry(const DySoapDesc& d, int k, int& A, int& n, int& B) {
  A = 1; B = 1; n = 1;
#pragma unroll
  for (int i = 0; i < DY_SOAP_MAX_DIMS; ++i) {
    const int s = d.shape[i];
    if (i < k) A *= s;
    else if (i == k) n = s;
    else if (i < d.ndim) B *= s;
  }
}

// unscale x clip, as optim_step_kernel applies it
static __device__ __forceinline__ float grad_factor(const float* state) { return (1.f / state[0]) * state[4]; }

// ---- mode product: out[a, j, b] = sum_i t[a, i, b] * Q[i, j] (back: Q[j, i]) -------------------------------------------------------
// One workgroup: a 32 (j) x 32 (columns c = a * B + b) tile of one tensor's output, Q tiled over both its dimensions, i ascending.
// A tensor without a basis in this dimension (or with fewer dimensions) is copied, 1024 elements per workgroup.
__global__ __launch_bounds__(256) void soap_rotate_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                          const DySoapDesc* __restrict__ table, int nt, const float* __restrict__ basis,
                                                          int k, int back, int scaled, const float* __restrict__ state) {
  if (state[2] != 0.f) return;
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int t = find_tensor(nt, bid, [&](int i) { return table[i].rot_blk[k]; });
  const DySoapDesc& d = table[t];
  const int lb = bid - d.rot_blk[k];
  const float f = scaled ? grad_factor(state) : 1.f;
  const float* s = src + d.off;
  float* o = dst + d.off;
  if (k >= d.ndim || !d.has_q[k]) {
    const long e0 = (long)lb * SOAP_EW;
#pragma unroll
    for (int r = 0; r < SOAP_EW / 256; ++r) {
      const long e = e0 + r * 256 + tid;
      if (e < d.numel) o[e] = scaled ? s[e] * f : s[e];
    }
    return;
  }
  int A, n, B;
  mode_geometry(d, k, A, n, B);
  const int C = A * B, jt = (n + SOAP_T - 1) / SOAP_T;
  const int j0 = (lb % jt) * SOAP_T, c0 = (lb / jt) * SOAP_T;
  const float* q = basis + d.pool_off[k];
  __shared__ float qs[SOAP_T][SOAP_T + 1];  // [i][j]
  __shared__ float ts[SOAP_T][SOAP_T + 1];  // [i][c]
  const int tx = tid & 15, ty = tid >> 4;   // outputs (j0 + ty, j0 + ty + 16) x (c0 + tx, c0 + tx + 16)
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int i0 = 0; i0 < n; i0 += SOAP_T) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = r * 256 + tid, row = e >> 5, col = e & 31;
      {  // Q: forward reads Q[i][j] (row = i, col = j: contiguous in j); back reads Q[j][i] (row = j, col = i: contiguous in i)
        const int i = back ? i0 + col : i0 + row, j = back ? j0 + row : j0 + col;
        const float v = (i < n && j < n) ? q[back ? (long)j * n + i : (long)i * n + j] : 0.f;
        if (back) qs[col][row] = v; else qs[row][col] = v;
      }
      {  // T: B == 1 makes i the contiguous index, otherwise the column is
        const int i = B == 1 ? i0 + col : i0 + row, c = B == 1 ? c0 + row : c0 + col;
        float v = 0.f;
        if (i < n && c < C) {
          const int a = c / B, b = c - a * B;
          v = s[((long)a * n + i) * B + b];
          if (scaled) v *= f;
        }
        if (B == 1) ts[col][row] = v; else ts[row][col] = v;
      }
    }
    __syncthreads();
    const int lim = n - i0 < SOAP_T ? n - i0 : SOAP_T;
    for (int i = 0; i < lim; ++i) {
      const float q0 = qs[i][ty], q1 = qs[i][ty + 16], t0 = ts[i][tx], t1 = ts[i][tx + 16];
      acc[0][0] = fmaf(t0, q0, acc[0][0]);
      acc[0][1] = fmaf(t1, q0, acc[0][1]);
      acc[1][0] = fmaf(t0, q1, acc[1][0]);
      acc[1][1] = fmaf(t1, q1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int j = j0 + ty + 16 * jj, c = c0 + tx + 16 * cc;
      if (j < n && c < C) {
        const int a = c / B, b = c - a * B;
        o[((long)a * n + j) * B + b] = acc[jj][cc];
      }
    }
}

// ---- Gram update: GG <- GG + (1 - beta2) * (G_(k) G_(k)^T - GG) for every (tensor, dimension) that keeps one ------------------------
// n <= 8 (the 3x3 taps, the stem's 3 input channels, nc-wide heads): ONE workgroup, every thread sums the outer products of the
// columns tid, tid + 256, ... in registers, then a fixed shuffle tree per output and the four wave partials in order.
// n > 8: a 32 x 32 output tile per workgroup, the unfolded length walked in chunks of 32, each output summed by one thread in order.
// The n <= 8 workgroup walks the WHOLE unfolded length (numel / n columns, 256 at a time): 1,152 iterations per thread for the widest
// 3x3 weight of DEAL-YOLO-N (256 x 128), about 3,000 for the 512 x 512 one of yolov8n-p2.  It is the tail of this launch for wider
// models; only DEAL-YOLO-N has been measured (profiles/r19_soap.md).  Splitting it would need a second, ordered reduction pass.
__global__ __launch_bounds__(256) void soap_gram_kernel(float* __restrict__ gram, const float* __restrict__ grads,
                                                        const DySoapDesc* __restrict__ table, int nt, float omb2,
                                                        const float* __restrict__ state) {
  if (state[2] != 0.f) return;
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int t = find_tensor(nt, bid, [&](int i) { return table[i].gram_blk[0]; });
  const DySoapDesc& d = table[t];
  int k = 0;
  for (int i = 0; i < d.ndim; ++i)
    if (d.has_q[i] && d.gram_blk[i] <= bid) k = i;
  const int lb = bid - d.gram_blk[k];
  int A, n, B;
  mode_geometry(d, k, A, n, B);
  const int C = A * B;
  const float f = grad_factor(state);
  const float* g = grads + d.off;
  float* gg = gram + d.pool_off[k];
  if (n <= 8) {
    if (lb != 0) return;  // (one workgroup owns the matrix: a grid larger than the table implies must not apply the update twice)
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int c = tid; c < C; c += 256) {
      const int a = c / B, b = c - a * B;
      float x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = i < n ? g[((long)a * n + i) * B + b] * f : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(x[i], x[j], acc[i][j]);
    }
    __shared__ float part[4][64];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = wave_sum(acc[i][j]);
        if ((tid & 63) == 0) part[tid >> 6][i * 8 + j] = s;
      }
    __syncthreads();
    if (tid < 64) {
      const int i = tid >> 3, j = tid & 7;
      if (i < n && j < n) {
        const float s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        const float old = gg[i * n + j];
        gg[i * n + j] = old + omb2 * (s - old);
      }
    }
    return;
  }
  const int it = (n + SOAP_T - 1) / SOAP_T;
  const int i0 = (lb / it) * SOAP_T, j0 = (lb % it) * SOAP_T;
  __shared__ float xs[SOAP_T][SOAP_T + 1];  // [c][i]
  __shared__ float ys[SOAP_T][SOAP_T + 1];  // [c][j]
  const int tx = tid & 15, ty = tid >> 4;   // outputs (i0 + ty, i0 + ty + 16) x (j0 + tx, j0 + tx + 16)
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int c0 = 0; c0 < C; c0 += SOAP_T) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = r * 256 + tid, row = e >> 5, col = e & 31;
      const int ii = B == 1 ? col : row, c = c0 + (B == 1 ? row : col);  // (B == 1: the mode index is the contiguous one)
      float vx = 0.f, vy = 0.f;
      if (c < C) {
        const int a = c / B, b = c - a * B;
        if (i0 + ii < n) vx = g[((long)a * n + i0 + ii) * B + b] * f;
        if (j0 + ii < n) vy = g[((long)a * n + j0 + ii) * B + b] * f;
      }
      const int cl = c - c0;
      xs[cl][ii] = vx;
      ys[cl][ii] = vy;
    }
    __syncthreads();
    const int lim = C - c0 < SOAP_T ? C - c0 : SOAP_T;
    for (int c = 0; c < lim; ++c) {
      const float x0 = xs[c][ty], x1 = xs[c][ty + 16], y0 = ys[c][tx], y1 = ys[c][tx + 16];
      acc[0][0] = fmaf(x0, y0, acc[0][0]);
      acc[0][1] = fmaf(x0, y1, acc[0][1]);
      acc[1][0] = fmaf(x1, y0, acc[1][0]);
      acc[1][1] = fmaf(x1, y1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2) {
      const int i = i0 + ty + 16 * a2, j = j0 + tx + 16 * b2;
      if (i < n && j < n) {
        const float old = gg[(long)i * n + j];
        gg[(long)i * n + j] = old + omb2 * (acc[a2][b2] - old);
      }
    }
}

// ---- element-wise kernels: 1024 elements of one tensor per workgroup -----------------------------------------------------------------
struct SoapEw {
  const DySoapDesc* table;
  int nt;
  const float* state;
};
#define SOAP_EW_PROLOGUE()                                                                    \
  if (a.state[2] != 0.f) return;                                                              \
  const int t_ = find_tensor(a.nt, (int)blockIdx.x, [&](int i) { return a.table[i].ew_blk; }); \
  const DySoapDesc& d = a.table[t_];                                                          \
  const long e0 = (long)((int)blockIdx.x - d.ew_blk) * SOAP_EW

// m <- beta1 m + (1 - beta1) gp, v <- beta2 v + (1 - beta2) gp^2, u = m / (sqrt(v) + eps); gp and u may be the same buffer
__global__ __launch_bounds__(256) void soap_adam_kernel(SoapEw a, float* __restrict__ m, float* __restrict__ v, const float* gp, float* u,
                                                        float beta1, float omb1, float beta2, float omb2, float eps) {
  SOAP_EW_PROLOGUE();
#pragma unroll
  for (int r = 0; r < SOAP_EW / 256; ++r) {
    const long e = e0 + r * 256 + threadIdx.x;
    if (e < d.numel) {
      const long i = d.off + e;
      const float g = gp[i];
      const float mm = m[i] * beta1 + omb1 * g;
      const float vv = v[i] * beta2 + omb2 * (g * g);
      m[i] = mm;
      v[i] = vv;
      u[i] = mm / (sqrtf(vv) + eps);
    }
  }
}

struct Soap3 { float v[3]; };
// p <- p - size_g * upd, then p <- p - (lr_g wd_g) p where wd_g > 0
__global__ __launch_bounds__(256) void soap_apply_kernel(SoapEw a, float* __restrict__ p, const float* __restrict__ upd, Soap3 size,
                                                         Soap3 decay) {
  SOAP_EW_PROLOGUE();
  const float sz = size.v[d.group], dc = decay.v[d.group];
#pragma unroll
  for (int r = 0; r < SOAP_EW / 256; ++r) {
    const long e = e0 + r * 256 + threadIdx.x;
    if (e < d.numel) {
      const long i = d.off + e;
      float x = p[i] - sz * upd[i];
      if (dc > 0.f) x = x - dc * x;
      p[i] = x;
    }
  }
}

// out[a, j, b] = v[a, order[j], b] around dimension k (a copy where the dimension keeps no basis)
__global__ __launch_bounds__(256) void soap_permute_kernel(SoapEw a, float* __restrict__ dst, const float* __restrict__ src,
                                                           const int* __restrict__ order, int k) {
  SOAP_EW_PROLOGUE();
  const bool perm = k < d.ndim && d.has_q[k];
  int A = 1, n = 1, B = 1;
  if (perm) mode_geometry(d, k, A, n, B);
  const int* ord = order + d.ord_off[perm ? k : 0];
#pragma unroll
  for (int r = 0; r < SOAP_EW / 256; ++r) {
    const long e = e0 + r * 256 + threadIdx.x;
    if (e < d.numel) {
      long s = e;
      if (perm) {
        const long ab = e / B;
        const int b = (int)(e - ab * B), j = (int)(ab % n);
        const long a_ = ab / n;
        int oj = ord[j];
        oj = oj < 0 ? 0 : (oj >= n ? n - 1 : oj);  // (a corrupt order vector must not read outside the tensor)
        s = (a_ * n + oj) * B + b;
      }
      dst[d.off + e] = src[d.off + s];
    }
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int dy_soap_desc_bytes(void) { return (int)sizeof(DySoapDesc); }

extern "C" int dy_soap_rotate(float* dst, const float* src, const DySoapDesc* table, int n_tensors, int n_blocks, const float* basis,
                              int dim, int back, int scaled, const float* state, hipStream_t stream) {
  if (!dst || !src || dst == src || !table || !basis || !state || n_tensors <= 0 || n_blocks <= 0 || dim < 0 || dim >= DY_SOAP_MAX_DIMS)
    return DY_ERR_ARG;
  hipLaunchKernelGGL(soap_rotate_kernel, dim3(n_blocks), dim3(256), 0, stream, dst, src, table, n_tensors, basis, dim, back, scaled, state);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_soap_gram(float* gram, const float* grads, const DySoapDesc* table, int n_tensors, int n_blocks, float one_minus_beta2,
                            const float* state, hipStream_t stream) {
  if (!gram || !grads || !table || !state || n_tensors <= 0 || n_blocks < 0) return DY_ERR_ARG;
  if (n_blocks == 0) return DY_OK;  // a model of 1-D tensors only keeps no Gram matrix
  hipLaunchKernelGGL(soap_gram_kernel, dim3(n_blocks), dim3(256), 0, stream, gram, grads, table, n_tensors, one_minus_beta2, state);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_soap_adam(float* m, float* v, const float* gp, float* upd, const DySoapDesc* table, int n_tensors, int n_blocks,
                            float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* state,
                            hipStream_t stream) {
  if (!m || !v || !gp || !upd || !table || !state || n_tensors <= 0 || n_blocks <= 0) return DY_ERR_ARG;
  hipLaunchKernelGGL(soap_adam_kernel, dim3(n_blocks), dim3(256), 0, stream, SoapEw{table, n_tensors, state}, m, v, gp, upd, beta1,
                     one_minus_beta1, beta2, one_minus_beta2, eps);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_soap_apply(float* params, const float* upd, const DySoapDesc* table, int n_tensors, int n_blocks, const float* size3,
                             const float* decay3, const float* state, hipStream_t stream) {
  if (!params || !upd || !table || !size3 || !decay3 || !state || n_tensors <= 0 || n_blocks <= 0) return DY_ERR_ARG;
  Soap3 s, w;  // host values, copied at enqueue time (kernel arguments)
  for (int i = 0; i < 3; ++i) s.v[i] = size3[i], w.v[i] = decay3[i];
  hipLaunchKernelGGL(soap_apply_kernel, dim3(n_blocks), dim3(256), 0, stream, SoapEw{table, n_tensors, state}, params, upd, s, w);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

extern "C" int dy_soap_permute_v(float* dst, const float* src, const DySoapDesc* table, int n_tensors, int n_blocks, const int* order,
                                 int dim, const float* state, hipStream_t stream) {
  if (!dst || !src || dst == src || !table || !order || !state || n_tensors <= 0 || n_blocks <= 0 || dim < 0 || dim >= DY_SOAP_MAX_DIMS)
    return DY_ERR_ARG;
  hipLaunchKernelGGL(soap_permute_kernel, dim3(n_blocks), dim3(256), 0, stream, SoapEw{table, n_tensors, state}, dst, src, order, dim);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
