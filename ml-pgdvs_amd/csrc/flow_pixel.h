// One pixel of the forward-backward flow consistency (preprocess/common.py:211-233, 314-325), shared by the kernel of
// pgdvs_flow_consistency (preprocess.hip) and the first pass of pgdvs_flow_pair_export (flow_export.hip), so that both give
// the same bits: everything float32 in upstream's order, every operation rounded on its own.  Also the internal launcher of
// the flow picture, whose kernel lives beside the PNG row pass it reuses (png.hip).
#pragma once
#include "common.h"

namespace pgdvs {

// img[y][x] when (x, y), float integers, lies in the image, else zero (grid_sample's padding_mode="zeros")
__device__ __forceinline__ float2 texel_or_zero(const float2 *__restrict__ img, float x, float y, int H, int W) {
  if (x >= 0.0f && x <= (float)(W - 1) && y >= 0.0f && y <= (float)(H - 1)) return img[(size_t)(int)y * W + (int)x];
  return make_float2(0.0f, 0.0f);
}

// coord_diff at pixel (x, y) whose own flow is f, checked against `other`[H,W]
__device__ __forceinline__ float2 coord_diff_pixel(float2 f, const float2 *__restrict__ other, int x, int y, int H, int W) {
  const float px = (float)x, py = (float)y;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const float c1x = px + f.x, c1y = py + f.y;
  const float gx = 2.0f * c1x / wm1 - 1.0f, gy = 2.0f * c1y / hm1 - 1.0f;
  const float ix = ((gx + 1.0f) / 2.0f) * wm1, iy = ((gy + 1.0f) / 2.0f) * hm1;
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float w = ix - x0, n = iy - y0;
  const float e = 1.0f - w, s = 1.0f - n;
  const float2 nw = texel_or_zero(other, x0, y0, H, W), ne = texel_or_zero(other, x0 + 1.0f, y0, H, W);
  const float2 sw = texel_or_zero(other, x0, y0 + 1.0f, H, W), se = texel_or_zero(other, x0 + 1.0f, y0 + 1.0f, H, W);
  const float wnw = e * s, wne = w * s, wsw = e * n, wse = w * n;
  const float sx = ((nw.x * wnw + ne.x * wne) + sw.x * wsw) + se.x * wse;
  const float sy = ((nw.y * wnw + ne.y * wne) + sw.y * wsw) + se.y * wse;
  return make_float2(px - (c1x + sx), py - (c1y + sy));
}

// The radius maximum travels as an unsigned key whose integer order is np.max's: the bits of a radius (never negative: a
// square root of a sum of squares), all ones for a NaN, which so beats every number.
constexpr uint32_t kRadNan = 0xffffffffu;
__device__ __forceinline__ uint32_t rad_key(float rad) { return rad == rad ? __float_as_uint(rad) : kRadNan; }
__device__ __forceinline__ float rad_of_key(uint32_t key) { return key == kRadNan ? __uint_as_float(0x7fc00000u) : __uint_as_float(key); }

// png.hip: the scanlines of the n_img (1 or 2) flow pictures, out[n_img,H,1+3W]; keys[n_img][n_keys] are the per-block radius
// keys of the first pass, reduced again by every row's workgroup; rad_max[n_img] is written by the first row of each picture.
int launch_flow_pictures(const float *flow12, const float *flow21, int n_img, int H, int W, int adaptive, const uint32_t *keys, int n_keys,
                         float *rad_max, uint8_t *out, hipStream_t stream);

}  // namespace pgdvs
