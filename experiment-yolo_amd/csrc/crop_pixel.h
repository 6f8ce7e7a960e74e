// The crop + resize + letterbox pixel of the batched two-stage path, shared by two_stage_batch.hip (uint8 HWC crops) and tiled.hip
// (fp32 planar tiles) so that both evaluate one expression.  Include after `#pragma clang fp contract(off)`.
#pragma once
#pragma clang fp contract(off)

// One output pixel: the expressions of crop_letterbox_kernel (two_stage.hip), in its order.
static __device__ __forceinline__ void crop_pixel(const unsigned char* img, int W, int x1, int y1, int cw, int ch, int nw, int nh, int px,
                                                  int py, int ox, int oy, unsigned char* v) {
  v[0] = 114; v[1] = 114; v[2] = 114;
  const int dx = ox - px, dy = oy - py;
  if (dx >= 0 && dx < nw && dy >= 0 && dy < nh && cw > 0 && ch > 0) {
    float fx = ((float)dx + 0.5f) * ((float)cw / (float)nw) - 0.5f;
    float fy = ((float)dy + 0.5f) * ((float)ch / (float)nh) - 0.5f;
    int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= (float)sx;
    fy -= (float)sy;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= cw - 1) { sx = cw - 1; fx = 0.f; }
    if (sy < 0) { sy = 0; fy = 0.f; }
    if (sy >= ch - 1) { sy = ch - 1; fy = 0.f; }
    const int sx1 = min(sx + 1, cw - 1), sy1 = min(sy + 1, ch - 1);
    const unsigned char* p00 = img + ((long)(y1 + sy) * W + x1 + sx) * 3;
    const unsigned char* p01 = img + ((long)(y1 + sy) * W + x1 + sx1) * 3;
    const unsigned char* p10 = img + ((long)(y1 + sy1) * W + x1 + sx) * 3;
    const unsigned char* p11 = img + ((long)(y1 + sy1) * W + x1 + sx1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = (float)p00[c] * (1.f - fx) + (float)p01[c] * fx, bot = (float)p10[c] * (1.f - fx) + (float)p11[c] * fx;
      v[c] = (unsigned char)fminf(fmaxf(rintf(top * (1.f - fy) + bot * fy), 0.f), 255.f);
    }
  }
}

// Blocks of 256 threads for a grid-stride loop over `total` items, capped.
static inline int grid_for(long total) {
  long b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}
