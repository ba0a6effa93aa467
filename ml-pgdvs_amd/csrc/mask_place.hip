// pgdvs_mask_place (include/pgdvs_hip.h states the contract): a decoded mask into its place.  One gather with two kinds of
// output: the byte itself, through the index map of a NEAREST resize, into a frame's slot of the resident store's mask table;
// or the evaluation mask float32(convert("RGB")[..., ::-1] > 1e-3) of a grey or RGB file.  A thread per output pixel, rows
// of the grid's y; plain loads and stores, no workspace, no atomics.  A map entry outside the source reads as 0.
#include "common.h"

namespace pgdvs {
namespace {

__global__ void __launch_bounds__(256) mask_place_kernel(const uint8_t *__restrict__ src, int h, int w, int C, int64_t src_row_stride,
                                                         const int32_t *__restrict__ map, int H, int W, int mode, uint8_t *__restrict__ out,
                                                         int64_t out_row_stride) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W || y >= H) return;
  int sy = y, sx = x;
  bool inside = true;
  if (map != nullptr) {
    const int32_t k = map[(int64_t)y * W + x];
    inside = k >= 0 && (int64_t)k < (int64_t)h * w;
    sy = inside ? k / w : 0, sx = inside ? k % w : 0;
  }
  const uint8_t *p = src + (int64_t)sy * src_row_stride + (int64_t)sx * C;
  if (mode == PGDVS_MASK_PLACE_U8) {
    out[(int64_t)y * out_row_stride + x] = inside ? p[0] : (uint8_t)0;
  } else {
    float *o = reinterpret_cast<float *>(out + (int64_t)y * out_row_stride) + (int64_t)x * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = inside && p[C == 1 ? 0 : 2 - k] > 0 ? 1.0f : 0.0f;
  }
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_mask_place(const uint8_t *src, int32_t h, int32_t w, int32_t channels, int64_t src_row_stride, const int32_t *map, int32_t H, int32_t W,
                               int32_t mode, void *out, int64_t out_row_stride, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(src && out, "pgdvs_mask_place: null pointer");
  PGDVS_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1 && h <= 16384 && w <= 16384 && H <= 16384 && W <= 16384, "pgdvs_mask_place: sizes of 1 .. 16384 expected");
  PGDVS_REQUIRE(mode == PGDVS_MASK_PLACE_U8 || mode == PGDVS_MASK_PLACE_BGR_F32, "pgdvs_mask_place: mode %d", mode);
  PGDVS_REQUIRE(channels == 1 || (channels == 3 && mode == PGDVS_MASK_PLACE_BGR_F32), "pgdvs_mask_place: %d channels (1, or 3 for the float output)", channels);
  PGDVS_REQUIRE(src_row_stride >= (int64_t)w * channels, "pgdvs_mask_place: a source row stride below a row");
  PGDVS_REQUIRE(map != nullptr || (H == h && W == w), "pgdvs_mask_place: without a map the sizes are equal");
  if (mode == PGDVS_MASK_PLACE_U8)
    PGDVS_REQUIRE(out_row_stride >= W, "pgdvs_mask_place: an output row stride below a row");
  else
    PGDVS_REQUIRE(out_row_stride >= (int64_t)W * 12 && out_row_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                  "pgdvs_mask_place: the float output's row stride is at least 12 W bytes, a multiple of 4, and out 4-byte aligned");
  PGDVS_REQUIRE(map == nullptr || (reinterpret_cast<uintptr_t>(map) & 3) == 0, "pgdvs_mask_place: map must be 4-byte aligned");
  PGDVS_LAUNCH("mask_place", mask_place_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, as_stream(stream), src, h, w, channels,
               src_row_stride, map, H, W, mode, static_cast<uint8_t *>(out), out_row_stride);
  return check_launch("pgdvs_mask_place");
}
