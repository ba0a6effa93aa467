// The device half of the JPEG reader: everything behind the entropy decoder (csrc/jpeg_entropy.cpp), in libjpeg's integer
// arithmetic.  include/pgdvs_hip.h states what is computed; this is how.
//
// idct      jpeg_idct_islow with its dequantisation.  A lane takes one row of one block: 8 int16 with one 16-byte load, so a
//           wavefront's load instruction moves 8 whole blocks (1 KiB), and the row of the component's table with another.
//           The products go to LDS (a block's 64 ints 72 apart: the column reads of the 8 blocks then fall on different
//           banks), the lane reads column `row` back, does the column pass (DESCALE 11), writes the column back, reads its row
//           and does the row pass (DESCALE 18, + 128, clamp): 8 bytes of the component's plane with one store.  A lane only
//           ever reads what its own wavefront wrote, and between the column read and the column write only its own words.
// colour    jdsample.c's fancy upsampling and jdcolor.c's ycc_rgb_convert.  A lane makes four consecutive pixels of a row: one
//           dword of luma, the chroma samples around them (columns j - 1 .. j + 2 of the near and, for 4:2:0, the far row,
//           indices clamped: a clamped sample is never one the formulas use; a plane of at most two columns is replicated),
//           and three dwords out where the row's address is a multiple of 4, as item_target_kernel stores; bytes otherwise
//           and for a row's last pixels.
// No atomics, no scratch, no floating point.
#include "common.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kLdsBlock = 72;  // ints from one block to the next in LDS
constexpr int kMaxSize = PGDVS_RESAMPLE_MAX_SIZE;

struct Planes {
  int64_t blocks[3];  // blocks of each component: the coefficient planes follow each other
  int32_t bw[3];      // blocks across
  int64_t off[3];     // the component's 8-bit plane in the workspace (bytes), pitch 8 * bw
};

// one pass of jidctint.c's 8-point inverse DCT; `shift` 11 (columns) or 18 (rows)
__device__ __forceinline__ void idct8(const int *in, int *out, int shift) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * -15137;
  int tmp3 = z1 + z2 * 6270;
  z2 = in[0], z3 = in[4];
  int tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  const int half = 1 << (shift - 1);
  out[0] = (tmp10 + tmp3 + half) >> shift, out[7] = (tmp10 - tmp3 + half) >> shift;
  out[1] = (tmp11 + tmp2 + half) >> shift, out[6] = (tmp11 - tmp2 + half) >> shift;
  out[2] = (tmp12 + tmp1 + half) >> shift, out[5] = (tmp12 - tmp1 + half) >> shift;
  out[3] = (tmp13 + tmp0 + half) >> shift, out[4] = (tmp13 - tmp0 + half) >> shift;
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ void __launch_bounds__(kBlock) jpeg_idct_kernel(const int16_t *__restrict__ coef, const uint16_t *__restrict__ quant, Planes pl,
                                                           uint8_t *__restrict__ ws) {
  __shared__ int lds[(kBlock / 8) * kLdsBlock];
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 3;  // the block, over all three components
  const int r = threadIdx.x & 7;
  int *mine = lds + (threadIdx.x >> 3) * kLdsBlock;
  const int64_t total = pl.blocks[0] + pl.blocks[1] + pl.blocks[2];
  const bool live = g < total;
  const int c = g < pl.blocks[0] ? 0 : (g < pl.blocks[0] + pl.blocks[1] ? 1 : 2);
  int v[8], w[8];
  if (live) {
    const uint4 cw = *reinterpret_cast<const uint4 *>(coef + g * 64 + r * 8);
    const uint4 qw = *reinterpret_cast<const uint4 *>(quant + c * 64 + r * 8);
    const uint32_t cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mine[r * 8 + 2 * i] = (int)(int16_t)(cs[i] & 0xffffu) * (int)(qs[i] & 0xffffu);
      mine[r * 8 + 2 * i + 1] = (int)(int16_t)(cs[i] >> 16) * (int)(qs[i] >> 16);
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = mine[i * 8 + r];  // column r
    idct8(v, w, 11);
#pragma unroll
    for (int i = 0; i < 8; ++i) mine[i * 8 + r] = w[i];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = mine[r * 8 + i];  // row r
    idct8(v, w, 18);
    const int64_t b = g - (c == 0 ? 0 : (c == 1 ? pl.blocks[0] : pl.blocks[0] + pl.blocks[1]));
    const int64_t by = b / pl.bw[c], bx = b % pl.bw[c];
    uint2 o;
    o.x = (uint32_t)clamp8(w[0] + 128) | ((uint32_t)clamp8(w[1] + 128) << 8) | ((uint32_t)clamp8(w[2] + 128) << 16) |
          ((uint32_t)clamp8(w[3] + 128) << 24);
    o.y = (uint32_t)clamp8(w[4] + 128) | ((uint32_t)clamp8(w[5] + 128) << 8) | ((uint32_t)clamp8(w[6] + 128) << 16) |
          ((uint32_t)clamp8(w[7] + 128) << 24);
    *reinterpret_cast<uint2 *>(ws + pl.off[c] + ((by * 8 + r) * pl.bw[c] + bx) * 8) = o;
  }
}

// the four upsampled samples of one chroma component for pixels x .. x + 3 of row y (x a multiple of 4)
template <int SAMPLING>
__device__ __forceinline__ void chroma4(const uint8_t *__restrict__ p, int pitch, int cw, int ch, int y, int x, int *out) {
  if (SAMPLING == PGDVS_JPEG_444) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p + (int64_t)y * pitch + x);
    out[0] = w & 0xff, out[1] = (w >> 8) & 0xff, out[2] = (w >> 16) & 0xff, out[3] = w >> 24;
    return;
  }
  const int j0 = x >> 1;
  const int near = SAMPLING == PGDVS_JPEG_420 ? y >> 1 : y;
  const uint8_t *rn = p + (int64_t)near * pitch, *rf = rn;
  if (SAMPLING == PGDVS_JPEG_420) {
    int far = (y & 1) ? near + 1 : near - 1;
    far = far < 0 ? 0 : (far > ch - 1 ? ch - 1 : far);
    rf = p + (int64_t)far * pitch;
  }
  int n[4], s[4];  // columns j0 - 1 .. j0 + 2: the near row's samples, and what the horizontal filter takes
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int j = j0 - 1 + k;
    j = j < 0 ? 0 : (j > cw - 1 ? cw - 1 : j);
    n[k] = rn[j];
    s[k] = SAMPLING == PGDVS_JPEG_420 ? 3 * n[k] + (int)rf[j] : n[k];
  }
  const bool replicate = cw <= 2;  // h2v1_upsample / h2v2_upsample
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = 1 + (q >> 1), j = j0 + (q >> 1);
    int v;
    if (SAMPLING == PGDVS_JPEG_420) {
      if (q & 1) v = j >= cw - 1 ? (4 * s[t] + 7) >> 4 : (3 * s[t] + s[t + 1] + 7) >> 4;
      else v = j == 0 ? (4 * s[t] + 8) >> 4 : (3 * s[t] + s[t - 1] + 8) >> 4;
    } else {
      if (q & 1) v = j >= cw - 1 ? s[t] : (3 * s[t] + s[t + 1] + 2) >> 2;
      else v = j == 0 ? s[t] : (3 * s[t] + s[t - 1] + 1) >> 2;
    }
    out[q] = replicate ? n[t] : v;
  }
}

// block (64, 4): lane threadIdx.x of row threadIdx.y; planes' pitches p0 (luma) and p1 (both chroma)
template <int SAMPLING>
__global__ void __launch_bounds__(kBlock) jpeg_colour_kernel(const uint8_t *__restrict__ py, const uint8_t *__restrict__ pcb,
                                                             const uint8_t *__restrict__ pcr, int p0, int p1, int cw, int ch, int W, int H,
                                                             uint8_t *__restrict__ out, int64_t row_stride) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const uint32_t yw = *reinterpret_cast<const uint32_t *>(py + (int64_t)y * p0 + x);
  int cb[4], cr[4];
  chroma4<SAMPLING>(pcb, p1, cw, ch, y, x, cb);
  chroma4<SAMPLING>(pcr, p1, cw, ch, y, x, cr);
  uint8_t px[12];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int Y = (yw >> (8 * q)) & 0xff, b = cb[q] - 128, r = cr[q] - 128;
    px[3 * q] = (uint8_t)clamp8(Y + ((91881 * r + 32768) >> 16));
    px[3 * q + 1] = (uint8_t)clamp8(Y + ((-22554 * b + 32768 - 46802 * r) >> 16));
    px[3 * q + 2] = (uint8_t)clamp8(Y + ((116130 * b + 32768) >> 16));
  }
  uint8_t *dst = out + (int64_t)y * row_stride + (int64_t)x * 3;
  if (x + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      d[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    return;
  }
  const int valid = (W - x < 4 ? W - x : 4) * 3;
#pragma unroll
  for (int k = 0; k < 12; ++k)
    if (k < valid) dst[k] = px[k];
}

// the info, checked: the grids are the ones its sizes give; fills the planes' layout
int check_info(const char *what, const pgdvs_jpeg_info *info, Planes *pl, int64_t *bytes) {
  PGDVS_REQUIRE(info != nullptr, "%s: null info", what);
  PGDVS_REQUIRE(info->width >= 1 && info->width <= kMaxSize && info->height >= 1 && info->height <= kMaxSize, "%s: %d x %d pixels (1 .. %d each)",
                what, info->width, info->height, kMaxSize);
  PGDVS_REQUIRE(info->sampling == PGDVS_JPEG_444 || info->sampling == PGDVS_JPEG_422 || info->sampling == PGDVS_JPEG_420,
                "%s: sampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", what, info->sampling);
  const int h = info->sampling == PGDVS_JPEG_444 ? 1 : 2, v = info->sampling == PGDVS_JPEG_420 ? 2 : 1;
  const int mw = (int)cdiv(info->width, 8 * h), mh = (int)cdiv(info->height, 8 * v);
  Carver ws{nullptr};
  int64_t blocks = 0;
  for (int c = 0; c < 3; ++c) {
    const int bw = c == 0 ? mw * h : mw, bh = c == 0 ? mh * v : mh;
    PGDVS_REQUIRE(info->blocks_w[c] == bw && info->blocks_h[c] == bh, "%s: component %d has %d x %d blocks, %d x %d pixels at sampling %d take %d x %d",
                  what, c, info->blocks_w[c], info->blocks_h[c], info->width, info->height, info->sampling, bw, bh);
    pl->blocks[c] = (int64_t)bw * bh;
    pl->bw[c] = bw;
    pl->off[c] = ws.off;
    ws.take<uint8_t>(pl->blocks[c] * 64);
    blocks += pl->blocks[c];
  }
  PGDVS_REQUIRE(info->coef_bytes == blocks * 128, "%s: coef_bytes %lld, the grids hold %lld", what, (long long)info->coef_bytes,
                (long long)(blocks * 128));
  *bytes = ws.off;
  return PGDVS_OK;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_jpeg_reconstruct_workspace_bytes(const pgdvs_jpeg_info *info) {
  Planes pl;
  int64_t bytes;
  if (check_info("pgdvs_jpeg_reconstruct_workspace_bytes", info, &pl, &bytes)) return -1;
  return bytes;
}

PGDVS_API int pgdvs_jpeg_reconstruct(const int16_t *coef, const uint16_t *quant, const pgdvs_jpeg_info *info, uint8_t *out, int64_t row_stride,
                                     void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  Planes pl;
  int64_t need;
  if (int rc = check_info("pgdvs_jpeg_reconstruct", info, &pl, &need)) return rc;
  PGDVS_REQUIRE(coef && quant && out, "pgdvs_jpeg_reconstruct: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 15) == 0 && (reinterpret_cast<uintptr_t>(quant) & 15) == 0,
                "pgdvs_jpeg_reconstruct: coef and quant must be 16-byte aligned");
  PGDVS_REQUIRE(row_stride >= (int64_t)info->width * 3, "pgdvs_jpeg_reconstruct: rows %lld bytes apart, a row has %lld", (long long)row_stride,
                (long long)info->width * 3);
  PGDVS_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "pgdvs_jpeg_reconstruct: workspace of %lld bytes, %lld needed (256-byte aligned)", (long long)workspace_bytes, (long long)need);
  const hipStream_t st = as_stream(stream);
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  const int64_t total = pl.blocks[0] + pl.blocks[1] + pl.blocks[2];
  PGDVS_LAUNCH("jpeg_idct", jpeg_idct_kernel, dim3((unsigned)cdiv(total * 8, kBlock)), dim3(kBlock), 0, st, coef, quant, pl, ws);
  if (int rc = check_launch("pgdvs_jpeg_reconstruct")) return rc;
  const int W = info->width, H = info->height;
  const int cw = info->sampling == PGDVS_JPEG_444 ? W : (W + 1) / 2, ch = info->sampling == PGDVS_JPEG_420 ? (H + 1) / 2 : H;
  const dim3 grid((unsigned)cdiv(cdiv(W, 4), 64), (unsigned)cdiv(H, 4)), block(64, 4);
  const int p0 = pl.bw[0] * 8, p1 = pl.bw[1] * 8;
#define PGDVS_JPEG_COLOUR(S) \
  PGDVS_LAUNCH("jpeg_colour", jpeg_colour_kernel<S>, grid, block, 0, st, ws + pl.off[0], ws + pl.off[1], ws + pl.off[2], p0, p1, cw, ch, W, H, out, row_stride)
  if (info->sampling == PGDVS_JPEG_444) PGDVS_JPEG_COLOUR(PGDVS_JPEG_444);
  else if (info->sampling == PGDVS_JPEG_422) PGDVS_JPEG_COLOUR(PGDVS_JPEG_422);
  else PGDVS_JPEG_COLOUR(PGDVS_JPEG_420);
#undef PGDVS_JPEG_COLOUR
  return check_launch("pgdvs_jpeg_reconstruct");
}
