// Evaluation kernels beside the mAP path: the detection confusion matrix and the false-positive count of gt_fails.py.
//
// dy_confusion_matrix replaces, for a whole batch in ONE launch (one workgroup per image), the reference's
// ConfusionMatrix.process_batch (ultralytics/utils/metrics.py:935-986), which the reference validator calls per labelled image
// (models/yolo/detect/val.py:136-152) with an IoU matrix copied to the host, two argsorts and two uniques.  The rule that code
// implements: keep the detections with conf > conf_thr; every kept detection chooses the label with its largest IoU among those with
// IoU > iou_thres, whatever the classes; every label keeps, of the detections that chose it, the one with the largest IoU.  A label with
// a winner counts in matrix[cls(winner), cls(label)], one without in matrix[nc, cls(label)]; and ONLY IF the image has at least one
// matched pair (the reference's ``if n:``, :983) every kept detection that won nothing counts in matrix[cls(det), nc].
// Exact-IoU ties are undefined in the reference (numpy's unstable argsort): here they go to the lower label index, then to the lower
// detection index.
//
// dy_count_fp replaces the triple Python loop of gt_fails.py:35-84 for a batch of images in one launch, one wave per image: the
// detections with conf >= conf_thr, in their stored order, each take the FIRST label in file order that is unused, of the same class
// and reaches iou_thr (first fit, not best fit); a detection that finds none is one false positive.  The script mixes float32 and
// float64 (whichever operand Python's max / min return); here the arithmetic is double on the fp32 detections, so the two agree
// wherever an IoU is not within rounding of the threshold.
#include "common.h"
#include "dealyolo_hip.h"
#pragma clang fp contract(off)  // keep the fp32 evaluation order of box_iou (no fused multiply-add)

#define CM_MAXL 1024  // labels of one image (staged in LDS / one bit per chunk and lane)

struct CmArgs {
  const float* predn;    // (Ntot, 6) x1 y1 x2 y2 conf cls, native space
  const int* pred_off;   // (B+1), or null: one image, detections [0, n_preds)
  const float* t_bidx;   // (n_targets), or null: one image, every label is its own
  const float* t_cls;
  const float* t_box;    // (n_targets, 4): xywh normalised with geom, native xyxy without
  const float* geom;     // (B,5) gain, padw, padh, ori_h, ori_w, or null
  int* matrix;           // (nc+1, nc+1), [predicted, true], index nc = background
  int* status;           // |= 1: an image has more than CM_MAXL labels; |= 2: a class outside [0, nc)
  int n_preds, n_targets, B, nc, skip_unlabelled;
  float img_h, img_w, conf, iou_thres;
};

static __device__ __forceinline__ float cm_clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// the label a detection chooses: largest IoU above the threshold, the lower index on a tie; -1 if none
static __device__ __forceinline__ int cm_best_label(const float* p, const float* lbox, int nl, float thr, float* best_iou) {
  const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
  const float area_d = (x2 - x1) * (y2 - y1);
  float best = thr;
  int bl = -1;
  for (int l = 0; l < nl; ++l) {
    const float lx1 = lbox[l * 4], ly1 = lbox[l * 4 + 1], lx2 = lbox[l * 4 + 2], ly2 = lbox[l * 4 + 3];
    const float iw = fmaxf(fminf(lx2, x2) - fmaxf(lx1, x1), 0.f), ih = fmaxf(fminf(ly2, y2) - fmaxf(ly1, y1), 0.f);
    const float inter = iw * ih;
    const float iou = inter / ((lx2 - lx1) * (ly2 - ly1) + area_d - inter + 1e-7f);  // box_iou(labels, detections)
    if (iou > best) {
      best = iou;
      bl = l;
    }
  }
  *best_iou = best;
  return bl;
}

__global__ __launch_bounds__(256) void confusion_matrix_kernel(CmArgs a) {
  __shared__ float lbox[CM_MAXL * 4];
  __shared__ int lcls[CM_MAXL];
  __shared__ unsigned long long win[CM_MAXL];  // (IoU bits << 32) | ~local detection index: the maximum is the winner
  __shared__ int nl_s, any_s;
  const int b = blockIdx.x, tid = threadIdx.x, nc = a.nc, ld = a.nc + 1;
  // ---- this image's labels, in their original order (wave 0: ballot compaction), moved to native space
  if (tid < 64) {
    int nl = 0;
    for (int base = 0; base < a.n_targets; base += 64) {
      const int i = base + tid;
      const bool mine = i < a.n_targets && (!a.t_bidx || (int)a.t_bidx[i] == b);
      const unsigned long long m = __ballot(mine);
      if (mine) {
        const int slot = nl + __popcll(m & ((1ull << tid) - 1ull));
        if (slot < CM_MAXL) {
          const float x = a.t_box[i * 4 + 0], y = a.t_box[i * 4 + 1], w = a.t_box[i * 4 + 2], h = a.t_box[i * 4 + 3];
          if (a.geom) {  // the formulas of match_predictions_kernel: ops.xywh2xyxy, * (w, h, w, h), scale_boxes + clip_boxes
            const float gain = a.geom[b * 5 + 0], padw = a.geom[b * 5 + 1], padh = a.geom[b * 5 + 2];
            const float oh = a.geom[b * 5 + 3], ow = a.geom[b * 5 + 4];
            const float dw = w / 2.f, dh = h / 2.f;
            lbox[slot * 4 + 0] = cm_clampf(((x - dw) * a.img_w - padw) / gain, 0.f, ow);
            lbox[slot * 4 + 1] = cm_clampf(((y - dh) * a.img_h - padh) / gain, 0.f, oh);
            lbox[slot * 4 + 2] = cm_clampf(((x + dw) * a.img_w - padw) / gain, 0.f, ow);
            lbox[slot * 4 + 3] = cm_clampf(((y + dh) * a.img_h - padh) / gain, 0.f, oh);
          } else {
            lbox[slot * 4 + 0] = x; lbox[slot * 4 + 1] = y; lbox[slot * 4 + 2] = w; lbox[slot * 4 + 3] = h;
          }
          lcls[slot] = (int)a.t_cls[i];
        }
      }
      nl += __popcll(m);
    }
    if (tid == 0) {
      if (nl > CM_MAXL) {
        atomicOr(a.status, 1);
        nl = CM_MAXL;
      }
      nl_s = nl;
      any_s = 0;
    }
  }
  __syncthreads();
  const int nl = nl_s;
  const int d0 = a.pred_off ? a.pred_off[b] : 0, d1 = a.pred_off ? a.pred_off[b + 1] : a.n_preds;
  if (nl == 0) {  // metrics.py:945-951 (a direct call); the validator never gets here (val.py:131-152)
    if (a.skip_unlabelled) return;
    for (int d = d0 + tid; d < d1; d += 256) {
      const float* p = a.predn + (size_t)d * 6;
      if (!(p[4] > a.conf)) continue;
      const int dc = (int)p[5];
      if (dc < 0 || dc >= nc) atomicOr(a.status, 2);
      else atomicAdd(&a.matrix[dc * ld + nc], 1);
    }
    return;
  }
  for (int l = tid; l < nl; l += 256) win[l] = 0ull;
  __syncthreads();
  // ---- pass 1: every kept detection bids for its best label
  for (int d = d0 + tid; d < d1; d += 256) {
    const float* p = a.predn + (size_t)d * 6;
    if (!(p[4] > a.conf)) continue;
    float best;
    const int bl = cm_best_label(p, lbox, nl, a.iou_thres, &best);
    if (bl >= 0) {
      atomicMax(&win[bl], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)~(unsigned)(d - d0));
      any_s = 1;
    }
  }
  __syncthreads();
  // ---- the labels: matched to their winner's class, or background (false negative)
  for (int l = tid; l < nl; l += 256) {
    const int gc = lcls[l];
    if (gc < 0 || gc >= nc) {
      atomicOr(a.status, 2);
      continue;
    }
    const unsigned long long w = win[l];
    int row = nc;
    if (w) {
      row = (int)a.predn[(size_t)(d0 + (int)~(unsigned)w) * 6 + 5];
      if (row < 0 || row >= nc) {
        atomicOr(a.status, 2);
        continue;
      }
    }
    atomicAdd(&a.matrix[row * ld + gc], 1);
  }
  if (!any_s) return;  // no pair above the threshold: no false positive is counted (metrics.py:983)
  // ---- pass 2: kept detections that won no label (same thread, same detections: the choice is recomputed)
  for (int d = d0 + tid; d < d1; d += 256) {
    const float* p = a.predn + (size_t)d * 6;
    if (!(p[4] > a.conf)) continue;
    float best;
    const int bl = cm_best_label(p, lbox, nl, a.iou_thres, &best);
    if (bl >= 0 && (int)~(unsigned)win[bl] == d - d0) continue;
    const int dc = (int)p[5];
    if (dc < 0 || dc >= nc) atomicOr(a.status, 2);
    else atomicAdd(&a.matrix[dc * ld + nc], 1);
  }
}

extern "C" int dy_confusion_matrix(const float* predn, const int* pred_off, int n_preds, const float* t_batch_idx, const float* t_cls,
                                   const float* t_boxes, int n_targets, const float* geom, int B, int img_h, int img_w, int nc, float conf,
                                   float iou_thres, int skip_unlabelled, int* matrix, int* status, hipStream_t stream) {
  if (B < 1 || nc < 1 || nc > 32767 || n_preds < 0 || n_targets < 0 || !matrix || !status) return DY_ERR_ARG;
  if ((n_preds > 0 && !predn) || (n_targets > 0 && (!t_cls || !t_boxes))) return DY_ERR_ARG;
  if (B > 1 && (!pred_off || (n_targets > 0 && !t_batch_idx))) return DY_ERR_ARG;
  if (!(iou_thres >= 0.f) || conf != conf) return DY_ERR_ARG;  // a negative IoU threshold would let IoU 0 pairs match
  CmArgs a{predn, pred_off, t_batch_idx, t_cls, t_boxes, geom, matrix, status, n_preds, n_targets, B, nc, skip_unlabelled,
           (float)img_h, (float)img_w, conf, iou_thres};
  hipLaunchKernelGGL(confusion_matrix_kernel, dim3(B), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

// ---- gt_fails.py:35-84 ---------------------------------------------------------------------------------------------------------------
struct FpArgs {
  const float* dets;      // (Ntot, 6) x1 y1 x2 y2 conf cls, native pixels
  const int* det_off;     // (B+1)
  const double* labels;   // (Ltot, 5) cls xc yc w h as the label file has them
  const int* lab_off;     // (B+1)
  const int* wh;          // (B, 2) image width, height
  int* fp;                // (B)
  int* status;            // |= 1: an image has more than CM_MAXL labels
  int B;
  float conf;
  double iou_thr;
};

__global__ __launch_bounds__(64) void count_fp_kernel(FpArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int l0 = a.lab_off[b];
  int nl = a.lab_off[b + 1] - l0;
  if (nl > CM_MAXL) {
    if (lane == 0) atomicOr(a.status, 1);
    nl = CM_MAXL;
  }
  const double w = (double)a.wh[b * 2], h = (double)a.wh[b * 2 + 1];
  const int nchunk = (nl + 63) >> 6;
  unsigned used = 0;  // bit c: label c * 64 + lane is taken
  int count = 0;
  for (int d = a.det_off[b]; d < a.det_off[b + 1]; ++d) {  // stored order; every lane reads the same row
    const float* p = a.dets + (size_t)d * 6;
    if (!(p[4] >= a.conf)) continue;
    const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3], pc = p[5];
    const double area_a = fmax(0.0, (x2 - x1) * (y2 - y1));
    bool matched = false;
    for (int c = 0; c < nchunk && !matched; ++c) {  // lowest chunk first, lowest lane inside it: the first label in file order
      const int j = c * 64 + lane;
      bool fit = false;
      if (j < nl && !((used >> c) & 1u)) {
        const double* g = a.labels + (size_t)(l0 + j) * 5;
        if ((double)(long long)g[0] == pc) {  // int(cls)
          const double xc = g[1] * w, yc = g[2] * h, bw = g[3] * w, bh = g[4] * h;  // yolo_to_xyxy: no clipping
          const double x3 = xc - bw / 2, y3 = yc - bh / 2, x4 = xc + bw / 2, y4 = yc + bh / 2;
          const double ix = fmax(0.0, fmin(x2, x4) - fmax(x1, x3)), iy = fmax(0.0, fmin(y2, y4) - fmax(y1, y3));
          const double inter = ix * iy;
          const double area_b = fmax(0.0, (x4 - x3) * (y4 - y3));
          fit = inter / (area_a + area_b - inter + 1e-6) >= a.iou_thr;
        }
      }
      const unsigned long long m = __ballot(fit);
      if (m) {
        if (lane == __ffsll((long long)m) - 1) used |= 1u << c;
        matched = true;
      }
    }
    if (!matched) ++count;
  }
  if (lane == 0) a.fp[b] = count;
}

extern "C" int dy_count_fp(const float* dets, const int* det_off, const double* labels, const int* lab_off, const int* wh, int B, float conf,
                           double iou_thr, int* fp, int* status, hipStream_t stream) {
  if (B < 1 || !det_off || !lab_off || !wh || !fp || !status || conf != conf || iou_thr != iou_thr) return DY_ERR_ARG;
  FpArgs a{dets, det_off, labels, lab_off, wh, fp, status, B, conf, iou_thr};
  hipLaunchKernelGGL(count_fp_kernel, dim3(B), dim3(64), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
