// Test-time augmentation of the eval forward (reference nn/tasks.py:335-371 DetectionModel._predict_augment / _descale_pred /
// _clip_augmented, utils/torch_utils.py:355-366 scale_img): the flip + bilinear resize + pad of the image batch in front of a pass,
// and the merge of the passes' outputs behind them.  Both are HBM-bound streams; the geometry (sizes, kept column ranges) is host
// arithmetic (ultralytics/hip/tta.py).
#include "common.h"
#include "dealyolo_hip.h"

// ---- scale_img: out (B, 3, Hp, Wp) = pad(interpolate(flip(x), (Ho, Wo), 'bilinear', align_corners=False), value=0.447) --------
// Index and weight arithmetic of ATen's upsample_bilinear2d_out_frame (size given, no scale factor), written in the same order so
// that the compiler contracts it the same way.  A flip is taken on the SOURCE index after the weights are formed for the flipped
// image: interpolating at the mirrored position would round differently from flip-then-interpolate.
// One thread = 4 consecutive output pixels of one row: one 16-byte store (pad pixels included).
struct ScaleArgs {
  const float* x;
  float* out;
  int H, W, Ho, Wo, Hp, Wp, flip;
  float rh, rw;  // (float)H / Ho, (float)W / Wo
};

static __device__ __forceinline__ float bilinear_src(float scale, int dst) {
  const float s = scale * (dst + 0.5f) - 0.5f;
  return s < 0.f ? 0.f : s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void scale_img_kernel(ScaleArgs a) {
  const int wq = (a.Wp + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;  // within one (image, channel) plane
  if (q >= a.Hp * wq) return;
  const int oy = q / wq, ox0 = (q - oy * wq) * 4;
  const long plane = blockIdx.y;
  const float* src = a.x + plane * a.H * a.W;
  float* dst = a.out + plane * a.Hp * a.Wp + (long)oy * a.Wp;
  const float pad = 0.447f;
  float v[4] = {pad, pad, pad, pad};
  if (oy < a.Ho) {
    if (a.Ho == a.H && a.Wo == a.W) {  // same size: ATen copies (the flip still applies)
      const float* r0 = src + (long)(a.flip == 2 ? a.H - 1 - oy : oy) * a.W;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ox0 + j < a.Wo) v[j] = r0[a.flip == 3 ? a.W - 1 - (ox0 + j) : ox0 + j];
    } else {
      const float hr = bilinear_src(a.rh, oy);
      int h0 = min((int)hr, a.H - 1);
      int h1 = h0 + (h0 < a.H - 1 ? 1 : 0);
      const float lh1 = hr - h0, lh0 = 1.f - lh1;
      if (a.flip == 2) h0 = a.H - 1 - h0, h1 = a.H - 1 - h1;
      const float* r0 = src + (long)h0 * a.W;
      const float* r1 = src + (long)h1 * a.W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ox = ox0 + j;
        if (ox >= a.Wo) break;
        const float wr = bilinear_src(a.rw, ox);
        int w0 = min((int)wr, a.W - 1);
        int w1 = w0 + (w0 < a.W - 1 ? 1 : 0);
        const float lw1 = wr - w0, lw0 = 1.f - lw1;
        if (a.flip == 3) w0 = a.W - 1 - w0, w1 = a.W - 1 - w1;
        v[j] = lh0 * (lw0 * r0[w0] + lw1 * r0[w1]) + lh1 * (lw0 * r1[w0] + lw1 * r1[w1]);
      }
    }
  }
  if (VEC) {
    *(f32x4*)(dst + ox0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ox0 + j < a.Wp) dst[ox0 + j] = v[j];
  }
}

extern "C" int dy_scale_img(const float* x, int B, int H, int W, int flip, int Ho, int Wo, int Hp, int Wp, float* out,
                            hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Ho > Hp || Wo > Wp || (flip != 0 && flip != 2 && flip != 3)) return DY_ERR_ARG;
  if ((long)B * 3 > 65535 || (long)Hp * ((Wp + 3) / 4) > (1L << 30)) return DY_ERR_ARG;
  ScaleArgs a{x, out, H, W, Ho, Wo, Hp, Wp, flip, (float)H / Ho, (float)W / Wo};
  const int per_plane = Hp * ((Wp + 3) / 4);
  const dim3 grid((per_plane + 255) / 256, B * 3);
  if (Wp % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(scale_img_kernel<true>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(scale_img_kernel<false>, grid, dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

// ---- _descale_pred + _clip_augmented + torch.cat(y, -1): out (B, no, sum_k (hi_k - lo_k)) ------------------------------------
// Output column c of row (b, r) comes from pass k = the one whose slot holds c, column lo_k + (c - base_k).  Rows 0-3 are divided by
// the pass's scale, then x = W - x (flip 3) or y = H - y (flip 2).  The quotient is the correctly rounded one (what ATen's CPU
// division gives), formed from the host's correctly rounded reciprocal by two fma corrections: the first brings the product within
// one ulp, the second then rounds correctly (Markstein's theorem) for finite, normal operands.  No v_div_fmas sequence.
#define DY_TTA_MAX_PASS 4
struct MergeArgs {
  const float* y[DY_TTA_MAX_PASS];
  int A[DY_TTA_MAX_PASS], lo[DY_TTA_MAX_PASS], base[DY_TTA_MAX_PASS + 1], flip[DY_TTA_MAX_PASS];
  float s[DY_TTA_MAX_PASS], rs[DY_TTA_MAX_PASS];
  float* out;
  int n_pass, no, total;  // total = base[n_pass]
  float H, W;
};

#include "div_rn.h"

#define DY_MERGE_PER_THREAD 4
__global__ __launch_bounds__(256) void tta_merge_kernel(MergeArgs a) {
  const long row = blockIdx.y;  // b * no + r
  const int r = (int)(row % a.no);
  float* out = a.out + row * a.total;
#pragma unroll
  for (int j = 0; j < DY_MERGE_PER_THREAD; ++j) {
    const int c = (blockIdx.x * DY_MERGE_PER_THREAD + j) * 256 + threadIdx.x;
    if (c >= a.total) return;
    int k = 0;
    while (k + 1 < a.n_pass && c >= a.base[k + 1]) ++k;
    float v = a.y[k][row * a.A[k] + a.lo[k] + (c - a.base[k])];
    if (r < 4) {
      v = div_rn(v, a.s[k], a.rs[k]);
      if (r == 0 && a.flip[k] == 3) v = a.W - v;
      if (r == 1 && a.flip[k] == 2) v = a.H - v;
    }
    out[c] = v;
  }
}

extern "C" int dy_tta_merge(int n_pass, const float* const* y_ptrs, const int* A, const int* col_lo, const int* col_hi,
                            const float* scale, const int* flip, int B, int no, int H, int W, float* out, hipStream_t stream) {
  if (n_pass < 1 || n_pass > DY_TTA_MAX_PASS || B < 1 || no < 4 || (long)B * no > 65535) return DY_ERR_ARG;
  MergeArgs a{};
  a.base[0] = 0;
  for (int k = 0; k < n_pass; ++k) {
    if (col_lo[k] < 0 || col_hi[k] < col_lo[k] || col_hi[k] > A[k] || !(scale[k] > 0.f) || (flip[k] != 0 && flip[k] != 2 && flip[k] != 3))
      return DY_ERR_ARG;
    a.y[k] = y_ptrs[k];
    a.A[k] = A[k], a.lo[k] = col_lo[k], a.flip[k] = flip[k];
    a.s[k] = scale[k], a.rs[k] = 1.f / scale[k];
    if ((long)a.base[k] + (col_hi[k] - col_lo[k]) > (1L << 30)) return DY_ERR_ARG;
    a.base[k + 1] = a.base[k] + (col_hi[k] - col_lo[k]);
  }
  a.out = out, a.n_pass = n_pass, a.no = no, a.total = a.base[n_pass], a.H = (float)H, a.W = (float)W;
  if (a.total == 0) return DY_OK;
  const int per_block = 256 * DY_MERGE_PER_THREAD;
  hipLaunchKernelGGL(tta_merge_kernel, dim3((a.total + per_block - 1) / per_block, B * no), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
