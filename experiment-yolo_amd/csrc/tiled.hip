// Sliced (tiled) inference for large aerial frames -- the device half of ultralytics/utils/tiled.py.  A frame is
// cut into overlapping model-sized tiles plus, optionally, one letterboxed view of the whole frame; every record is detected on at
// native resolution and the detections of all records are merged per frame:
//   tile_gather_f32   K records of N images held back to back in one byte pool -> (K, 3, S, S) fp32 planar in [0, 1], the tensor the
//                     stem of a recorded inference plan reads: crop_pixel's uint8 (the bits of dy_crop_letterbox_u8_multi), converted
//   tile_merge        every record's detections mapped into their image, clipped, and swept by a greedy NMS across records (IoU or
//                     intersection over the smaller box), one workgroup per image, up to 8,192 rows each
#include "common.h"
#include "dealyolo_hip.h"
#pragma clang fp contract(off)
#include "two_stage_iou.h"
#include "crop_pixel.h"
#include "div_rn.h"

struct TileGatherArgs {
  const unsigned char* pool;  // uint8 HWC images back to back
  const long* img_off;        // (N) byte offset of each image in the pool, any alignment
  const int* img_hw;          // (N, 2) height, width
  const int* tile_img;        // (K) image of each record; < 0: a pad canvas, nothing of the pool is read
  const int* rects;           // (K, 4) x1 y1 x2 y2, x2/y2 exclusive
  const int* geom;            // (K, 4) new_w, new_h, pad_x, pad_y
  const float* lut;           // (256) the float of every byte value
  float* out;                 // (K, 3, S, S)
  int K, S;
};

// PX = 4: a thread owns four consecutive pixels of one output row (S % 4 == 0 and a 16-byte aligned batch: they never straddle a row
// and every plane's piece is one 16-byte store, so a wave writes 1 KiB contiguous per plane and instruction).  PX = 1: any S.  The
// kernel is write bound (12 bytes out per pixel against 3 in); the source is read with byte loads, as an image starts wherever the
// one before it ended.  The byte -> float table sits in LDS: 12 look-ups per item.
template <int PX>
__global__ __launch_bounds__(256) void tile_gather_kernel(TileGatherArgs a) {
  __shared__ float lut[256];
  lut[threadIdx.x] = a.lut[threadIdx.x];
  __syncthreads();
  const long row_items = a.S / PX, per = row_items * a.S, total = per * a.K, plane = (long)a.S * a.S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int k = (int)(idx / per);
    const int r = (int)(idx - (long)k * per);
    const int oy = r / (int)row_items, ox0 = (r - oy * (int)row_items) * PX;
    const int b = a.tile_img[k];
    unsigned char v[3 * PX];
    if (b >= 0) {
      const unsigned char* img = a.pool + a.img_off[b];
      const int W = a.img_hw[b * 2 + 1];
      const int x1 = a.rects[k * 4 + 0], y1 = a.rects[k * 4 + 1], cw = a.rects[k * 4 + 2] - x1, ch = a.rects[k * 4 + 3] - y1;
      const int nw = a.geom[k * 4 + 0], nh = a.geom[k * 4 + 1], px = a.geom[k * 4 + 2], py = a.geom[k * 4 + 3];
#pragma unroll
      for (int p = 0; p < PX; ++p) crop_pixel(img, W, x1, y1, cw, ch, nw, nh, px, py, ox0 + p, oy, v + 3 * p);
    } else {
#pragma unroll
      for (int p = 0; p < 3 * PX; ++p) v[p] = 114;
    }
    float* o = a.out + (long)k * 3 * plane + (long)oy * a.S + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (PX == 4)
        *reinterpret_cast<f32x4*>(o + c * plane) = (f32x4){lut[v[c]], lut[v[3 + c]], lut[v[6 + c]], lut[v[9 + c]]};
      else
        o[c * plane] = lut[v[c]];
    }
  }
}

extern "C" int dy_tile_gather_f32(const void* pool, const long* img_off, const int* img_hw, const int* tile_img, const int* rects,
                                  const int* geom, const float* lut, int K, int S, float* out, hipStream_t stream) {
  if (K <= 0) return DY_OK;
  if (S <= 0 || !lut || !out) return DY_ERR_ARG;
  TileGatherArgs a{(const unsigned char*)pool, img_off, img_hw, tile_img, rects, geom, lut, out, K, S};
  if (S % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(grid_for((long)K * S * (S / 4))), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(grid_for((long)K * S * S)), dim3(256), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}

// ---- cross-record merge ------------------------------------------------------------------------------------------------------------
#define TG_ROWS DY_TILE_MERGE_MAX_ROWS  // 8,192 = 4 x NH_MAX of two_stage.hip
#define TG_THREADS 1024
#define TG_SLOTS (TG_ROWS / TG_THREADS)  // rows a thread owns: q = tid + k * TG_THREADS

struct TileMergeArgs {
  const float* rows;      // (M, 6) x1 y1 x2 y2 score label in canvas coordinates, packed image-major
  const int* row_off;     // (N+1)
  const int* row_tile;    // (M) index into tiles
  const float* tiles;     // (Kt, 6) x1, y1, pad_x, pad_y, r, 1/r
  const int* img_hw;      // (N, 2) height, width
  float* out;             // (M, 6) mapped rows
  int* order;             // (M) kept row indices (into rows) in sweep order, packed from row_off[i]
  int* nkeep;             // (N)
  int* status;
  int Kt, metric, agnostic;
  float thr;
};

// intersection over the smaller box, with iou_plain's zero rules
static __device__ __forceinline__ float ios_plain(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
  const float x1 = fmaxf(ax1, bx1), y1 = fmaxf(ay1, by1), x2 = fminf(ax2, bx2), y2 = fminf(ay2, by2);
  if (x2 <= x1 || y2 <= y1) return 0.f;
  const float inter = (x2 - x1) * (y2 - y1);
  const float a1 = (ax2 - ax1) * (ay2 - ay1), a2 = (bx2 - bx1) * (by2 - by1);
  if (a1 <= 0.f || a2 <= 0.f) return 0.f;
  const float m = fminf(a1, a2);
  return m > 0.f ? inter / m : 0.f;
}

// One workgroup of 1,024 threads per image; everything the sweep reads is in LDS (152 KiB): the boxes in sweep order (128 KiB), a
// 16-bit label class per position (16 KiB; the class of a label is the first row of the image that carries it, so equal classes =
// equal labels) and the alive flags (8 KiB).  While the ranks are counted the box region is borrowed: scores in its first 32 KiB,
// labels in the next 32, the sweep order in the 16 after that.  The mapped rows go to global memory once and come back in sweep
// order.  The sweep is nms_hard_kernel's, with two differences: a dead pivot costs no barrier (nothing was written since the last
// one), and the pivot at position t only looks at positions > t.  Position p belongs to thread p % 1024, which alone writes alive[p].
__global__ __launch_bounds__(TG_THREADS) void tile_merge_kernel(TileMergeArgs a) {
  __shared__ __attribute__((aligned(16))) float sbox[TG_ROWS * 4];
  __shared__ unsigned short lid[TG_ROWS];
  __shared__ unsigned char alive[TG_ROWS];
  __shared__ int wsum[TG_THREADS / 64];
  __shared__ int s_nv;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r0 = a.row_off[b], n = a.row_off[b + 1] - r0;
  if (n > TG_ROWS || n < 0) {  // uniform: the image gets no result (the launcher's max_rows said otherwise)
    if (tid == 0) { atomicOr(a.status, 1); a.nkeep[b] = 0; }
    return;
  }
  const float W = (float)a.img_hw[b * 2 + 1], H = (float)a.img_hw[b * 2 + 0];
  float* skey = sbox;
  float* slab = sbox + TG_ROWS;
  unsigned short* perm = reinterpret_cast<unsigned short*>(sbox + 2 * TG_ROWS);
  if (tid == 0) s_nv = 0;
  __syncthreads();
  // ---- 1. map into the image, clip, drop.  A dropped row (or a NaN score) gets a NaN key: it compares false with everything below.
  float myscore[TG_SLOTS], mylab[TG_SLOTS];
  int bad_tile = 0, valid = 0;
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k) {
    const int i = tid + k * TG_THREADS;
    myscore[k] = __builtin_nanf("");
    mylab[k] = 0.f;
    if (i < n) {
      const float* row = a.rows + (long)(r0 + i) * 6;
      float* o = a.out + (long)(r0 + i) * 6;
      const int t = a.row_tile[r0 + i];
      float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
      const float sc = row[4];
      mylab[k] = row[5];
      if (t >= 0 && t < a.Kt) {
        const float* g = a.tiles + (long)t * 6;
        const float gx = g[0], gy = g[1], px = g[2], py = g[3], rr = g[4], rs = g[5];
        x1 = fminf(fmaxf(div_rn(x1 - px, rr, rs) + gx, 0.f), W);
        y1 = fminf(fmaxf(div_rn(y1 - py, rr, rs) + gy, 0.f), H);
        x2 = fminf(fmaxf(div_rn(x2 - px, rr, rs) + gx, 0.f), W);
        y2 = fminf(fmaxf(div_rn(y2 - py, rr, rs) + gy, 0.f), H);
        if (x2 - x1 > 0.f && y2 - y1 > 0.f && sc == sc) {
          myscore[k] = sc;
          ++valid;
        }
      } else {
        bad_tile = 1;  // a row without a record: written through unmapped, dropped, reported
      }
      o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = sc; o[5] = mylab[k];
      skey[i] = myscore[k];
      slab[i] = mylab[k];
    }
  }
  if (bad_tile) atomicOr(a.status, 2);
  if (valid) atomicAdd(&s_nv, valid);
  __syncthreads();
  const int nv = s_nv;
  // ---- 2. rank (score descending, ties to the lower row index) and label class (the first row with the same label).  All pairs of
  // rows are compared, which is the long part of the kernel at 8,192 rows, so a wave does it for the slots it has rows in only, and
  // in three stretches: rows below the wave's 64 (a tie counts, and the class can only be found here), its own 64 (the full rule),
  // rows above (a tie does not count).  The keys are LDS broadcasts.
  int rank[TG_SLOTS], cls[TG_SLOTS];
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k) {
    const int i = tid + k * TG_THREADS, lo = i - (tid & 63);  // lo: the wave's first row in this slot
    const float ms = myscore[k], ml = mylab[k];
    int r = 0, c = i;
    if (lo < n) {  // wave-uniform
      const int mid = min(lo + 64, n);
#pragma unroll 4
      for (int q = 0; q < lo; ++q) {
        r += skey[q] >= ms;
        c = min(c, slab[q] == ml ? q : TG_ROWS);
      }
      for (int q = lo; q < mid; ++q) {
        const float sq = skey[q];
        r += (sq > ms) || (sq == ms && q < i);
        c = min(c, slab[q] == ml ? q : TG_ROWS);
      }
#pragma unroll 4
      for (int q = mid; q < n; ++q) r += skey[q] > ms;
    }
    rank[k] = r;
    cls[k] = c;
  }
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k)
    if (myscore[k] == myscore[k] && rank[k] < nv) {
      perm[rank[k]] = (unsigned short)(tid + k * TG_THREADS);
      lid[rank[k]] = (unsigned short)cls[k];
    }
  __syncthreads();
  // ---- 3. the rows in sweep order.  The barrier between the two loops ends the borrowing; it also makes this workgroup's own
  // writes to a.out visible to it.
  int myrow[TG_SLOTS], mycls[TG_SLOTS];
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k) {
    const int p = tid + k * TG_THREADS;
    myrow[k] = p < nv ? (int)perm[p] : 0;
    mycls[k] = p < nv ? (int)lid[p] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k) {
    const int p = tid + k * TG_THREADS;
    if (p < nv) {
      const float* o = a.out + (long)(r0 + myrow[k]) * 6;
      *reinterpret_cast<f32x4*>(sbox + p * 4) = (f32x4){o[0], o[1], o[2], o[3]};
      alive[p] = 1;
    }
  }
  __syncthreads();
  // ---- 4. the sweep
  const int nk = (nv + TG_THREADS - 1) / TG_THREADS;
  for (int t = 0; t < nv; ++t) {
    if (!alive[t]) continue;  // uniform: every thread reads the same byte, written before the last barrier
    const f32x4 pb = *reinterpret_cast<const f32x4*>(sbox + t * 4);
    const int l = lid[t];
#pragma unroll
    for (int k = 0; k < TG_SLOTS; ++k) {
      const int q = tid + k * TG_THREADS;
      if (k < nk && q > t && q < nv && alive[q] && (a.agnostic || mycls[k] == l)) {
        const f32x4 qb = *reinterpret_cast<const f32x4*>(sbox + q * 4);
        const float m = a.metric ? ios_plain(pb[0], pb[1], pb[2], pb[3], qb[0], qb[1], qb[2], qb[3])
                                 : iou_plain(pb[0], pb[1], pb[2], pb[3], qb[0], qb[1], qb[2], qb[3]);
        if (m > a.thr) alive[q] = 0;
      }
    }
    __syncthreads();
  }
  // ---- 5. compact, 1,024 positions per round: thread t owns position 1024 k + t
  const int lane = tid & 63, wave = tid >> 6;
  int base = 0;
#pragma unroll
  for (int k = 0; k < TG_SLOTS; ++k) {
    if (k >= nk) break;  // uniform
    const int p = tid + k * TG_THREADS;
    const bool keep = p < nv && alive[p];
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1)), total = 0;
    for (int w = 0; w < TG_THREADS / 64; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (keep) a.order[r0 + base + before] = r0 + myrow[k];
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.nkeep[b] = base;
}

extern "C" int dy_tile_merge(const float* rows, const int* row_off, const int* row_tile, const float* tiles, const int* img_hw, int N,
                             int Kt, int max_rows, float thr, int metric, int agnostic, float* out, int* order, int* nkeep, int* status,
                             hipStream_t stream) {
  if (N <= 0) return DY_OK;
  if (max_rows > DY_TILE_MERGE_MAX_ROWS) return DY_ERR_CAPACITY;
  if (Kt < 0 || max_rows < 0 || (metric != 0 && metric != 1) || !nkeep || !status) return DY_ERR_ARG;
  TileMergeArgs a{rows, row_off, row_tile, tiles, img_hw, out, order, nkeep, status, Kt, metric, agnostic != 0, thr};
  hipLaunchKernelGGL(tile_merge_kernel, dim3(N), dim3(TG_THREADS), 0, stream, a);
  DY_CHECK_LAUNCH();
  return DY_OK;
}
