// Two-stage inference over a chunk of images (reference double_inference.py main :509-562 around process_image_optimized :404-449) --
// the device half of ultralytics/utils/double_inference.py:double_inference_batch.  two_stage.hip handles one image per launch; a drone
// frame with a handful of animals fills neither a launch nor a forward, so here the crops of MANY images of different sizes are cut in
// one launch, their refinements chosen in one launch, and the replacement + per-class NMS + the script's greedy TP/FP/FN count
// (calculate_metrics_optimized :306-333) done in one launch with a workgroup per image:
//   crop_letterbox_multi   K crops of N images held back to back in one byte pool -> (K, S, S, 3); the bits of crop_letterbox_kernel
//   refine_select_multi    refine_select_kernel with the image bounds of each crop's own image
//   two_stage_merge        apply the refinements, nms_hard_kernel's sweep, greedy count against the labels
#include "common.h"
#include "dealyolo_hip.h"
#pragma clang fp contract(off)
#include "two_stage_iou.h"
#include "crop_pixel.h"

struct CropMultiArgs {
  const unsigned char* pool;  // uint8 HWC images back to back
  const long* img_off;        // (N) byte offset of each image in the pool, any alignment
  const int* img_hw;          // (N, 2) height, width
  const int* crop_img;        // (K) image of each crop
  const int* rects;           // (K, 4) x1 y1 x2 y2, x2/y2 exclusive
  const int* geom;            // (K, 4) new_w, new_h, pad_x, pad_y
  unsigned char* out;         // (K, S, S, 3)
  int K, S;
};

struct __attribute__((aligned(4))) Px4 { unsigned int w[3]; };  // four RGB pixels = three dwords

// PX = 4: a thread owns four consecutive pixels of one output row (S % 4 == 0, so they never straddle a row and byte 12 * item of the
// 256-byte-aligned batch is dword aligned): 12 bytes leave as dwords, not as twelve byte stores.  PX = 1: any S.  The source is read
// with byte loads either way: an image starts wherever the one before it ended.
template <int PX>
__global__ __launch_bounds__(256) void crop_letterbox_multi_kernel(CropMultiArgs a) {
  const long row_items = a.S / PX, per = row_items * a.S, total = per * a.K;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int k = (int)(idx / per);
    const int r = (int)(idx - (long)k * per);
    const int oy = r / (int)row_items, ox0 = (r - oy * (int)row_items) * PX;
    const int b = a.crop_img[k];
    const unsigned char* img = a.pool + a.img_off[b];
    const int W = a.img_hw[b * 2 + 1];
    const int x1 = a.rects[k * 4 + 0], y1 = a.rects[k * 4 + 1], cw = a.rects[k * 4 + 2] - x1, ch = a.rects[k * 4 + 3] - y1;
    const int nw = a.geom[k * 4 + 0], nh = a.geom[k * 4 + 1], px = a.geom[k * 4 + 2], py = a.geom[k * 4 + 3];
    unsigned char v[3 * PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) crop_pixel(img, W, x1, y1, cw, ch, nw, nh, px, py, ox0 + p, oy, v + 3 * p);
    if (PX == 4) {
      Px4 o;
#pragma unroll
      for (int w = 0; w < 3; ++w)
        o.w[w] = (unsigned)v[4 * w] | ((unsigned)v[4 * w + 1] << 8) | ((unsigned)v[4 * w + 2] << 16) | ((unsigned)v[4 * w + 3] << 24);
      *reinterpret_cast<Px4*>(a.out + idx * 12) = o;
    } else {
      unsigned char* o = a.out + idx * 3;
      o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
  }
}

extern "C" int dy_crop_letterbox_u8_multi(const void* pool, const long* img_off, const int* img_hw, const int* crop_img, const int* rects,
                                          const int* geom, int K, int S, void* out, hipStream_t stream) {
  if (K <= 0) return DY_OK;
  if (S <= 0) return DY_ERR_ARG;
  CropMultiArgs a{(const unsigned char*)pool, img_off, img_hw, crop_img, rects, geom, (unsigned char*)out, K, S};
  if (S % 4 == 0 && ((uintptr_t)out & 3) == 0)
    hipLaunchKernelGGL(crop_letterbox_multi_kernel<4>, dim3(grid_for((long)K * S * (S / 4))), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(crop_letterbox_multi_kernel<1>, dim3(grid_for((long)K * S * S)), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

struct RefineMultiArgs {
  const float* dets;    // second-stage NMS rows (x1 y1 x2 y2 conf cls) of all crops, packed
  const int* off;       // (K+1) row offsets per crop
  const float* orig;    // (K, 6) the first-stage detection each crop was cut around
  const int* rects;     // (K, 4)
  const float* scale;   // (K, 3) ratio, pad_x, pad_y
  const int* crop_img;  // (K)
  const int* img_hw;    // (N, 2) height, width
  float* out;           // (K, 6) refined detection
  int* found;           // (K) 1 when a refinement replaces the original
};

// refine_select_kernel (two_stage.hip) with img_w / img_h of the crop's own image: one wave per first-stage detection, the FIRST
// candidate reaching the best combined score wins.
__global__ __launch_bounds__(64) void refine_select_multi_kernel(RefineMultiArgs a) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int b = a.crop_img[k];
  const float img_h = (float)a.img_hw[b * 2 + 0], img_w = (float)a.img_hw[b * 2 + 1];
  const float ox1 = a.orig[k * 6 + 0], oy1 = a.orig[k * 6 + 1], ox2 = a.orig[k * 6 + 2], oy2 = a.orig[k * 6 + 3];
  const float oscore = a.orig[k * 6 + 4], ocls = a.orig[k * 6 + 5];
  const float ratio = a.scale[k * 3 + 0], padx = a.scale[k * 3 + 1], pady = a.scale[k * 3 + 2];
  const float cx = (float)a.rects[k * 4 + 0], cy = (float)a.rects[k * 4 + 1];
  float best = -1.f;
  int besti = 0x7fffffff;
  for (int i = a.off[k] + lane; i < a.off[k + 1]; i += 64) {
    const float* d = a.dets + (long)i * 6;
    if (d[5] != ocls) continue;
    const float x1 = (d[0] - padx) / ratio + cx, y1 = (d[1] - pady) / ratio + cy;
    const float x2 = (d[2] - padx) / ratio + cx, y2 = (d[3] - pady) / ratio + cy;
    if (!(x2 > x1 && y2 > y1 && x1 >= 0.f && y1 >= 0.f && x2 <= img_w && y2 <= img_h)) continue;
    const float iou = iou_plain(ox1, oy1, ox2, oy2, x1, y1, x2, y2);
    if (iou < 0.25f) continue;
    const float comb = d[4] * 0.6f + iou * 0.4f;
    if (comb > best) { best = comb; besti = i; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if (lane == 0) {
    int ok = 0;
    if (best >= 0.f && besti != 0x7fffffff) {
      const float* d = a.dets + (long)besti * 6;
      if (d[4] > oscore) {
        ok = 1;
        a.out[k * 6 + 0] = (d[0] - padx) / ratio + cx;
        a.out[k * 6 + 1] = (d[1] - pady) / ratio + cy;
        a.out[k * 6 + 2] = (d[2] - padx) / ratio + cx;
        a.out[k * 6 + 3] = (d[3] - pady) / ratio + cy;
        a.out[k * 6 + 4] = d[4];
        a.out[k * 6 + 5] = d[5];
      }
    }
    a.found[k] = ok;
  }
}

extern "C" int dy_refine_select_multi(const float* dets, const int* offsets, const float* orig, const int* rects, const float* scale,
                                      const int* crop_img, const int* img_hw, int K, float* out, int* found, hipStream_t stream) {
  if (K <= 0) return DY_OK;
  RefineMultiArgs a{dets, offsets, orig, rects, scale, crop_img, img_hw, out, found};
  hipLaunchKernelGGL(refine_select_multi_kernel, dim3(K), dim3(64), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

#define TM_ROWS 2048    // NH_MAX of two_stage.hip
#define TM_LABELS 1024  // the label capacity of the project's other matchers (metrics.hip, confusion.hip)

struct MergeArgs {
  float* rows;            // (M, 6) x1 y1 x2 y2 conf cls of the chunk's first-stage detections, in/out
  const int* row_off;     // (N+1)
  const float* refined;   // (K, 6) dy_refine_select_multi's out
  const int* found;       // (K)
  const int* crop_row;    // (K) index into rows, ascending within an image
  const int* crop_off;    // (N+1)
  const float* labels;    // (L, 5) cls x1 y1 x2 y2, native pixels
  const int* lab_off;     // (N+1)
  unsigned char* keep;    // (M)
  int* counts;            // (N, 3) tp fp fn
  int* status;
  int aligned;
  float nms_iou, match_iou;
};

// One workgroup per image.  The row tables are those of nms_hard_kernel (about 59 KB); the labels stay in global memory (a few KB per
// image, L2) with only their matched flags in LDS.
__global__ __launch_bounds__(256) void two_stage_merge_kernel(MergeArgs a) {
  __shared__ float sb[TM_ROWS * 4];
  __shared__ float ss[TM_ROWS], sl[TM_ROWS];
  __shared__ short order[TM_ROWS], rank[TM_ROWS];
  __shared__ unsigned char alive[TM_ROWS];
  __shared__ unsigned char matched[TM_LABELS];
  __shared__ int part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r0 = a.row_off[b], n = a.row_off[b + 1] - r0;
  const int c0 = a.crop_off[b], nc = a.crop_off[b + 1] - c0;
  const int l0 = a.lab_off[b], nl = a.lab_off[b + 1] - l0;
  if (n > TM_ROWS || nl > TM_LABELS || nc > n || n < 0 || nl < 0 || nc < 0) {  // uniform: the image gets no result
    if (tid == 0) atomicOr(a.status, 1);
    return;
  }
  float* rows = a.rows + (long)r0 * 6;
  for (int i = tid; i < n; i += 256) {
    sb[i * 4 + 0] = rows[i * 6 + 0]; sb[i * 4 + 1] = rows[i * 6 + 1];
    sb[i * 4 + 2] = rows[i * 6 + 2]; sb[i * 4 + 3] = rows[i * 6 + 3];
    ss[i] = rows[i * 6 + 4];
    sl[i] = rows[i * 6 + 5];
  }
  for (int j = tid; j < nl; j += 256) matched[j] = 0;
  // ---- 1. apply (process_image_optimized :430-435).  aligned: a found refinement replaces the row its crop was cut for.  Otherwise the
  // script's zip of the SUCCESSFUL refinements with all candidate rows: the j-th found one replaces the row of the image's j-th crop
  // slot, j = the number of found flags before it.  Thread t ranks the crops [t * per, (t + 1) * per).
  const int per = (nc + 255) / 256;
  const int k_lo = min(tid * per, nc), k_hi = min(k_lo + per, nc);
  int mine = 0;
  for (int k = k_lo; k < k_hi; ++k) mine += a.found[c0 + k] != 0;
  part[tid] = mine;
  __syncthreads();  // also orders the row loads above before the replacements below
  int j = 0;
  for (int t = 0; t < tid; ++t) j += part[t];
  for (int k = k_lo; k < k_hi; ++k) {
    if (!a.found[c0 + k]) continue;
    const int i = a.crop_row[c0 + (a.aligned ? k : j)] - r0;
    ++j;
    if (i < 0 || i >= n) continue;  // a table that does not belong to this image: nothing is written outside it
    const float* f = a.refined + (long)(c0 + k) * 6;
    sb[i * 4 + 0] = f[0]; sb[i * 4 + 1] = f[1]; sb[i * 4 + 2] = f[2]; sb[i * 4 + 3] = f[3];
    ss[i] = f[4];
    sl[i] = f[5];
#pragma unroll
    for (int c = 0; c < 6; ++c) rows[i * 6 + c] = f[c];
  }
  __syncthreads();
  // ---- 2. per-class greedy hard NMS, nms_hard_kernel's sweep (torchvision_nms :164-203); nms_iou < 0 keeps every row
  for (int i = tid; i < n; i += 256) {
    int r = 0;
    const float s = ss[i];
    for (int q = 0; q < n; ++q) r += (ss[q] > s) || (ss[q] == s && q < i);
    rank[i] = (short)r;
    order[r] = (short)i;
    alive[i] = 1;
  }
  __syncthreads();
  if (a.nms_iou >= 0.f) {
    for (int t = 0; t < n; ++t) {
      const int i = order[t];
      if (alive[i]) {  // uniform: every thread reads the same shared byte after the barrier below
        const float x1 = sb[i * 4], y1 = sb[i * 4 + 1], x2 = sb[i * 4 + 2], y2 = sb[i * 4 + 3], l = sl[i];
        for (int q = tid; q < n; q += 256)
          if (alive[q] && rank[q] > t && sl[q] == l && iou_plain(x1, y1, x2, y2, sb[q * 4], sb[q * 4 + 1], sb[q * 4 + 2], sb[q * 4 + 3]) > a.nms_iou)
            alive[q] = 0;
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += 256) a.keep[r0 + i] = alive[i];
  // ---- 3. greedy count (calculate_metrics_optimized :306-333), the first wave: kept rows in stored order, each takes the unmatched
  // label of its class with the largest IoU >= match_iou (strictly larger than the best so far, which starts at 0: ties go to the
  // first label, an IoU of 0 never matches).  Lane L looks at the labels L, L + 64, ... and is the only one to read or set their
  // flags, so the flags need no barrier.  No kept row: (0, 0, nl); no label: (0, kept, 0) -- the script's early returns.
  if (tid >= 64) return;
  const float* lab = a.labels + (long)l0 * 5;
  int tp = 0, kept = 0;
  for (int i = 0; i < n; ++i) {
    if (!alive[i]) continue;
    ++kept;
    const float x1 = sb[i * 4], y1 = sb[i * 4 + 1], x2 = sb[i * 4 + 2], y2 = sb[i * 4 + 3], l = sl[i];
    float best = 0.f;
    int bestj = 0x7fffffff;
    for (int q = tid; q < nl; q += 64) {
      if (matched[q] || lab[q * 5] != l) continue;
      const float iou = iou_plain(x1, y1, x2, y2, lab[q * 5 + 1], lab[q * 5 + 2], lab[q * 5 + 3], lab[q * 5 + 4]);
      if (iou > best && iou >= a.match_iou) { best = iou; bestj = q; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oj = __shfl_xor(bestj, o, 64);
      if (ob > best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
    }
    if (bestj != 0x7fffffff) {
      ++tp;
      if ((bestj & 63) == tid) matched[bestj] = 1;
    }
  }
  if (tid == 0) {
    a.counts[b * 3 + 0] = tp;
    a.counts[b * 3 + 1] = kept - tp;
    a.counts[b * 3 + 2] = nl - tp;
  }
}

extern "C" int dy_two_stage_merge(float* rows, const int* row_off, const float* refined, const int* found, const int* crop_row,
                                  const int* crop_off, int aligned, float nms_iou, const float* labels, const int* lab_off,
                                  float match_iou, int N, void* keep, int* counts, int* status, hipStream_t stream) {
  if (N <= 0) return DY_OK;
  MergeArgs a{rows, row_off, refined, found, crop_row, crop_off, labels, lab_off, (unsigned char*)keep, counts, status, aligned, nms_iou, match_iou};
  hipLaunchKernelGGL(two_stage_merge_kernel, dim3(N), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
