// The final motion mask of one frame (pgdvs/preprocess/compute_mask.py:341-471 combine_masks, :184-193 warp_flow, :827-829
// the next frame's previous mask) and the class-id look-up in front of it (:367-380).  include/pgdvs_hip.h states what is
// computed; this is how.  Six launches and one small memset on the caller's stream, nothing read back:
//
// warp    (later frames) one thread per pixel: the 4 x 4 cubic taps of the previous mask and of the previous count around
//         p + flow, with the 32 x 4 weight table the host built (kernel argument, staged in LDS).  float32, every operation
//         rounded on its own (the library is built with -ffp-contract=off), the division __fdiv_rn.  The coordinate is
//         clamped as a FLOAT to [-8, W + 8] before it becomes an integer, and every tap index is compared with the image
//         before it is used: no flow value reaches an address.  Writes warp_prev, dyn_track, their conjunction (workspace)
//         and the warped count, which waits in dyn_cnt for the union pass.
// erode2  one workgroup per 64 x 16 tile, one byte per pixel in LDS (as epipolar_mask_kernel): the conjunction over the tile
//         and a 4-pixel halo, raw = raw_no_warp | erode(conjunction) over the tile and a 2-pixel halo, raw_eroded =
//         erode(raw) over the tile.  Outside the image both erosions read set pixels.  Frame 0 has no conjunction.
// bits    raw_eroded as one bit per pixel (a ballot per wavefront), so that the count pass reads 2 bytes of it per 16 of sam.
// count   sam is read ONCE, 16 bytes per lane and step from the first 16-byte boundary of each segment (H W is in general
//         no multiple of 16, so every segment starts at another phase); the up to 15 bytes in front and behind go one per
//         lane.  n_pix and n_overlap are integer sums: shuffles within a wavefront, LDS across the four, then one integer
//         atomic add per workgroup, segment and counter.  Any non-zero byte of sam counts as set.
// union   selection per segment in float64, then one thread per pixel ors the SELECTED segments (each workgroup first turns
//         the flags into a list in LDS; the others are never read) into raw_eroded and finishes dyn_cnt.
// close   one workgroup per tile: final = dilate(final_raw), reading clear pixels outside the image, and next_prev =
//         erode(final_raw), reading set ones, from one staged tile with a 2-pixel halo.
#include "common.h"
#include "wave.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 16;
constexpr float kConsistThres = 1.0f;  // read_optical_flow's default (compute_mask.py:197), which combine_masks never overrides
constexpr float kWarpClamp = 8.0f;
// skimage.morphology.disk(2): the 13 offsets with dx^2 + dy^2 <= 4
__device__ const int8_t kDiskDx[13] = {0, -1, 0, 1, -2, -1, 0, 1, 2, -1, 0, 1, 0};
__device__ const int8_t kDiskDy[13] = {-2, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 2};

struct CubicTable {
  float w[32 * 4];
};

// ---- warp ----

struct WarpParams {
  const uint8_t *prev_mask;  // [H,W]
  const float *prev_cnt;     // [H,W]
  const float2 *flow;        // [H,W]
  const float2 *coord_diff;  // [H,W]
  uint8_t *warp_prev, *dyn_track, *conj;
  float *cnt_warp;
  int H, W;
  float frames;  // float32(img_idx + 1)
  float track_thres;
  CubicTable tab;
};

// the integer cell and the table row of one map coordinate; n is the image's extent along it
__device__ __forceinline__ void split_coord(float c, int n, int &cell, int &k) {
  c = fminf(fmaxf(c, -kWarpClamp), (float)n + kWarpClamp);  // a NaN becomes -8
  const int s = (int)rintf(c * 32.0f);
  cell = s >> 5;
  k = s & 31;
}

__global__ void __launch_bounds__(kBlock) warp_kernel(WarpParams p) {
  __shared__ float tab[32 * 4];
  if (threadIdx.x < 32 * 4) tab[threadIdx.x] = p.tab.w[threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (int64_t)p.H * p.W) return;
  const int y = (int)(i / p.W), x = (int)(i - (int64_t)y * p.W);
  const float2 f = p.flow[i], cd = p.coord_diff[i];
  int ix, kx, iy, ky;
  split_coord(f.x + (float)x, p.W, ix, kx);
  split_coord(f.y + (float)y, p.H, iy, ky);
  float mask_acc = 0.0f, cnt_acc = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ty = iy - 1 + j;
    const bool row_in = ty >= 0 && ty < p.H;
    const float cy = tab[ky * 4 + j];
    float vm[4], vc[4], w[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int tx = ix - 1 + t;
      vm[t] = 0.0f;
      vc[t] = 0.0f;
      if (row_in && tx >= 0 && tx < p.W) {
        const int64_t q = (int64_t)ty * p.W + tx;
        vm[t] = p.prev_mask[q] ? 1.0f : 0.0f;
        vc[t] = p.prev_cnt[q];
      }
      w[t] = cy * tab[kx * 4 + t];
    }
    const float rm = ((vm[0] * w[0] + vm[1] * w[1]) + vm[2] * w[2]) + vm[3] * w[3];
    const float rc = ((vc[0] * w[0] + vc[1] * w[1]) + vc[2] * w[2]) + vc[3] * w[3];
    mask_acc = j == 0 ? rm : mask_acc + rm;
    cnt_acc = j == 0 ? rc : cnt_acc + rc;
  }
  const float bwd_mask = (fabsf(cd.x) + fabsf(cd.y)) <= kConsistThres ? 1.0f : 0.0f;
  const uint8_t wp = ((mask_acc >= 0.5f ? 1.0f : 0.0f) * bwd_mask) > 1e-3f ? 1 : 0;
  const uint8_t dt = (__fdiv_rn(cnt_acc, p.frames) * bwd_mask) > p.track_thres ? 1 : 0;
  p.warp_prev[i] = wp;
  p.dyn_track[i] = dt;
  p.conj[i] = wp & dt;
  p.cnt_warp[i] = cnt_acc;
}

// ---- the two chained erosions ----

constexpr int kE0W = kTileW + 8, kE0H = kTileH + 8;  // the tile and a 4-pixel halo
constexpr int kE1W = kTileW + 4, kE1H = kTileH + 4;  // the tile and a 2-pixel halo

struct ErodeParams {
  const uint8_t *raw_no_warp;  // [H,W]
  const uint8_t *conj;         // [H,W] or null (frame 0)
  uint8_t *raw, *raw_eroded;
  int H, W;
};

__global__ void __launch_bounds__(kBlock) erode2_kernel(ErodeParams p) {
  __shared__ uint8_t s0[kE0H][kE0W];
  __shared__ uint8_t s1[kE1H][kE1W];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  if (p.conj) {
    for (int k = threadIdx.x; k < kE0H * kE0W; k += kBlock) {
      const int ry = k / kE0W, rx = k - ry * kE0W;
      const int x = tx0 + rx - 4, y = ty0 + ry - 4;
      uint8_t bit = 1;  // outside the image: set, the erosion's border value
      if (x >= 0 && x < p.W && y >= 0 && y < p.H) bit = p.conj[(int64_t)y * p.W + x] ? 1 : 0;
      s0[ry][rx] = bit;
    }
    __syncthreads();
  }
  // raw over the tile and its 2-pixel halo; the tile's own pixels are written by this workgroup alone
  for (int k = threadIdx.x; k < kE1H * kE1W; k += kBlock) {
    const int ry = k / kE1W, rx = k - ry * kE1W;
    const int x = tx0 + rx - 2, y = ty0 + ry - 2;
    uint8_t bit = 1;
    if (x >= 0 && x < p.W && y >= 0 && y < p.H) {
      const int64_t i = (int64_t)y * p.W + x;
      bit = p.raw_no_warp[i] ? 1 : 0;
      if (p.conj) {
        uint8_t e = 1;
#pragma unroll
        for (int t = 0; t < 13; ++t) e &= s0[ry + 2 + kDiskDy[t]][rx + 2 + kDiskDx[t]];
        bit |= e;
      }
      if (rx >= 2 && rx < kTileW + 2 && ry >= 2 && ry < kTileH + 2) p.raw[i] = bit;
    }
    s1[ry][rx] = bit;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kTileH * kTileW; k += kBlock) {
    const int ty = k / kTileW, tx = k - ty * kTileW;
    const int x = tx0 + tx, y = ty0 + ty;
    if (x >= p.W || y >= p.H) continue;
    uint8_t e = 1;
#pragma unroll
    for (int t = 0; t < 13; ++t) e &= s1[ty + 2 + kDiskDy[t]][tx + 2 + kDiskDx[t]];
    p.raw_eroded[(int64_t)y * p.W + x] = e;
  }
}

// ---- raw_eroded as bits ----

// bits[w] holds pixels 64 w .. 64 w + 63, pixel i in bit i & 63; n_words covers the pixels and two words of zeros behind them
__global__ void __launch_bounds__(kBlock) pack_bits_kernel(const uint8_t *__restrict__ mask, int64_t n, unsigned long long *__restrict__ bits,
                                                           int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // whole wavefronts: n_words * 64 threads
  const unsigned long long b = __ballot(i < n && mask[i] != 0);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < n_words) bits[i >> 6] = b;
}

// ---- segment counts ----

constexpr int kCountSteps = 8;  // 16-byte steps per lane: a workgroup covers 32 KiB of one segment

// bit 7 of every non-zero byte of x
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) { return (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; }
// bits 7, 15, 23, 31 gathered into bits 0..3 (the four partial products do not overlap)
__device__ __forceinline__ uint32_t gather4(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 0xfu; }

// 16 bits of the bit image from pixel i on
__device__ __forceinline__ uint32_t bits16(const unsigned long long *__restrict__ bits, int64_t i) {
  const int64_t w = i >> 6;
  const int sh = (int)(i & 63);
  const unsigned long long lo = bits[w] >> sh;
  const unsigned long long hi = sh ? bits[w + 1] << (64 - sh) : 0ull;
  return (uint32_t)((lo | hi) & 0xffffull);
}

struct CountParams {
  const uint8_t *sam;               // [n_seg, n]
  const unsigned long long *bits;   // raw_eroded, one bit per pixel
  int32_t *counts;                  // [n_seg, 2], zeroed
  int64_t n;                        // H W
};

__global__ void __launch_bounds__(kBlock) seg_count_kernel(CountParams p) {
  __shared__ int part[2][kBlock / kWave];
  const int seg = blockIdx.y;
  const uint8_t *__restrict__ base = p.sam + (int64_t)seg * p.n;
  // the segment's first 16-byte boundary, and how many whole 16-byte groups follow it
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15);
  if (head > p.n) head = p.n;
  const int64_t groups = (p.n - head) >> 4;
  int n_pix = 0, n_overlap = 0;
  const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(base + head);
  const int64_t g0 = (int64_t)blockIdx.x * (kBlock * kCountSteps) + threadIdx.x;
#pragma unroll
  for (int s = 0; s < kCountSteps; ++s) {
    const int64_t g = g0 + (int64_t)s * kBlock;
    if (g < groups) {
      const uint4 v = body[g];
      const uint32_t m = gather4(nonzero_bytes(v.x)) | (gather4(nonzero_bytes(v.y)) << 4) | (gather4(nonzero_bytes(v.z)) << 8) |
                         (gather4(nonzero_bytes(v.w)) << 12);
      n_pix += __popc(m);
      n_overlap += __popc(m & bits16(p.bits, head + (g << 4)));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 32) {  // lanes 0..15: the bytes in front of the boundary; 16..31: those behind the groups
    const int t = threadIdx.x & 15;
    const int64_t tail0 = head + (groups << 4);
    const int64_t i = threadIdx.x < 16 ? (t < head ? (int64_t)t : -1) : (tail0 + t < p.n ? tail0 + t : -1);
    if (i >= 0 && base[i]) {
      n_pix += 1;
      n_overlap += (int)((p.bits[i >> 6] >> (i & 63)) & 1ull);
    }
  }
  n_pix = wave_sum_all(n_pix);
  n_overlap = wave_sum_all(n_overlap);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = n_pix;
    part[1][threadIdx.x >> 6] = n_overlap;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) s += part[threadIdx.x][w];
    if (s) __hip_atomic_fetch_add(&p.counts[seg * 2 + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- selection and union ----

__global__ void __launch_bounds__(kBlock) seg_select_kernel(const int32_t *__restrict__ counts, int n_seg, double overlap_thres,
                                                            uint8_t *__restrict__ selected) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_seg) return;
  const int n_pix = counts[2 * s], n_overlap = counts[2 * s + 1];
  selected[s] = (n_overlap > 0 && (double)n_overlap > overlap_thres * (double)n_pix) ? 1 : 0;
}

struct UnionParams {
  const uint8_t *sam;          // [n_seg, n]
  const uint8_t *selected;     // [n_seg]
  const uint8_t *raw_eroded;   // [n]
  const uint8_t *raw_no_warp;  // [n]
  uint8_t *final_raw;
  float *dyn_cnt;              // holds the warped count on later frames
  int64_t n;
  int n_seg, first_frame;
};

constexpr int kUnionChunk = 1024;  // segments whose flags one round of the union pass turns into a list

__global__ void __launch_bounds__(kBlock) union_kernel(UnionParams p) {
  __shared__ int list[kUnionChunk];
  __shared__ int count;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.n;  // no early return: every thread meets the barriers
  uint8_t bit = live ? p.raw_eroded[i] : 0;
  for (int s0 = 0; s0 < p.n_seg; s0 += kUnionChunk) {
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const int s1 = s0 + kUnionChunk < p.n_seg ? s0 + kUnionChunk : p.n_seg;
    for (int s = s0 + threadIdx.x; s < s1; s += kBlock)
      if (p.selected[s]) list[atomicAdd(&count, 1)] = s;  // any order: the union does not depend on it
    __syncthreads();
    const int m = count;
    if (live)
      for (int k = 0; k < m; ++k) bit |= p.sam[(int64_t)list[k] * p.n + i] ? 1 : 0;
    __syncthreads();
  }
  if (!live) return;
  p.final_raw[i] = bit;
  p.dyn_cnt[i] = p.first_frame ? (p.raw_no_warp[i] ? 1.0f : 0.0f) : p.dyn_cnt[i] + (bit ? 1.0f : 0.0f);
}

// ---- dilation and the next frame's erosion ----

struct CloseParams {
  const uint8_t *final_raw;
  uint8_t *final_mask, *next_prev;
  int H, W;
};

__global__ void __launch_bounds__(kBlock) close_kernel(CloseParams p) {
  __shared__ uint8_t s[kE1H][kE1W];  // 0 clear, 1 set, 2 outside the image
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  for (int k = threadIdx.x; k < kE1H * kE1W; k += kBlock) {
    const int ry = k / kE1W, rx = k - ry * kE1W;
    const int x = tx0 + rx - 2, y = ty0 + ry - 2;
    uint8_t v = 2;
    if (x >= 0 && x < p.W && y >= 0 && y < p.H) v = p.final_raw[(int64_t)y * p.W + x] ? 1 : 0;
    s[ry][rx] = v;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kTileH * kTileW; k += kBlock) {
    const int ty = k / kTileW, tx = k - ty * kTileW;
    const int x = tx0 + tx, y = ty0 + ty;
    if (x >= p.W || y >= p.H) continue;
    uint8_t any_set = 0, all_set = 1;
#pragma unroll
    for (int t = 0; t < 13; ++t) {
      const uint8_t v = s[ty + 2 + kDiskDy[t]][tx + 2 + kDiskDx[t]];
      any_set |= v == 1 ? 1 : 0;   // the dilation reads clear pixels outside the image
      all_set &= v != 0 ? 1 : 0;   // the erosion set ones
    }
    const int64_t i = (int64_t)y * p.W + x;
    p.final_mask[i] = any_set;
    p.next_prev[i] = all_set;
  }
}

// ---- class ids ----

struct SemanticParams {
  const int64_t *ids[2];  // [n] each: ADE20K, COCO
  uint8_t *out[2], *sem;
  int64_t n;
  uint32_t listed[2][16];  // bit c: class id c (counted from 0) is dynamic
};

__global__ void __launch_bounds__(kBlock) semantic_mask_kernel(SemanticParams p) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  uint8_t bit[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int64_t c = p.ids[k][i];
    bit[k] = (c >= 0 && c < 512) ? (uint8_t)((p.listed[k][c >> 5] >> (c & 31)) & 1u) : 0;
    p.out[k][i] = bit[k];
  }
  p.sem[i] = bit[0] | bit[1];
}

// grid.y carries tile rows (H / 16) and segments: both stay below 65536; flat pixel indices are int64 throughout, so H W
// < 2^31 only keeps the pixel counts in int32
bool shape_ok(int H, int W) { return H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (1ll << 31); }

int64_t bit_words(int64_t n) { return cdiv(n, 64) + 2; }

struct Workspace {
  uint8_t *conj;
  unsigned long long *bits;
  int32_t *counts;
  uint8_t *selected;
  int64_t bytes;
};

Workspace carve(void *base, int H, int W, int n_seg) {
  const int64_t n = (int64_t)H * W;
  Carver c{static_cast<char *>(base)};
  Workspace w;
  w.conj = c.take<uint8_t>(n);
  w.bits = c.take<unsigned long long>(bit_words(n) * 8);
  w.counts = c.take<int32_t>((int64_t)n_seg * 2 * 4);
  w.selected = c.take<uint8_t>(n_seg);
  w.bytes = c.off;
  return w;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define MC_SHAPE_MSG "%s: bad shape H=%d W=%d n_seg=%d (H, W >= 1, each < 2^20, H W < 2^31, 0 <= n_seg < 65536)"

PGDVS_API int64_t pgdvs_mask_combine_workspace_bytes(int H, int W, int n_seg) {
  PGDVS_REQUIRE(shape_ok(H, W) && n_seg >= 0 && n_seg < 65536, MC_SHAPE_MSG, "pgdvs_mask_combine_workspace_bytes", H, W, n_seg);
  return carve(nullptr, H, W, n_seg).bytes;
}

PGDVS_API int pgdvs_mask_combine(const uint8_t *raw_no_warp, const uint8_t *sam, int n_seg, int H, int W, const uint8_t *prev_mask,
                                 const float *prev_cnt, const float *bwd_flow, const float *bwd_coord_diff, const float *cubic_table,
                                 int img_idx, double dyn_track_thres, double sam_overlap_thres, uint8_t *warp_prev,
                                 uint8_t *dyn_track, float *dyn_cnt, uint8_t *raw, uint8_t *raw_eroded, uint8_t *final_raw,
                                 uint8_t *final_mask, uint8_t *next_prev, int32_t *seg_counts, uint8_t *seg_selected,
                                 void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(H, W) && n_seg >= 0 && n_seg < 65536, MC_SHAPE_MSG, "pgdvs_mask_combine", H, W, n_seg);
  PGDVS_REQUIRE(img_idx >= 0 && img_idx < (1 << 24), "pgdvs_mask_combine: img_idx %d (0 <= img_idx < 2^24: img_idx + 1 as float32)", img_idx);
  PGDVS_REQUIRE(raw_no_warp && dyn_cnt && raw && raw_eroded && final_raw && final_mask && next_prev && workspace,
                "pgdvs_mask_combine: null pointer");
  PGDVS_REQUIRE(n_seg == 0 || sam, "pgdvs_mask_combine: %d segments and no sam", n_seg);
  const bool has_prev = prev_mask != nullptr;
  PGDVS_REQUIRE(has_prev == (prev_cnt != nullptr) && has_prev == (bwd_flow != nullptr) && has_prev == (bwd_coord_diff != nullptr),
                "pgdvs_mask_combine: prev_mask, prev_cnt, bwd_flow and bwd_coord_diff go together (all NULL on the first frame)");
  PGDVS_REQUIRE(!has_prev || (cubic_table && warp_prev && dyn_track), "pgdvs_mask_combine: a previous frame needs cubic_table, warp_prev and dyn_track");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(bwd_flow) & 7) == 0 && (reinterpret_cast<uintptr_t>(bwd_coord_diff) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(prev_cnt) & 3) == 0 && (reinterpret_cast<uintptr_t>(dyn_cnt) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(seg_counts) & 3) == 0,
                "pgdvs_mask_combine: bwd_flow and bwd_coord_diff must be 8-byte aligned, prev_cnt, dyn_cnt and seg_counts 4-byte");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "pgdvs_mask_combine: the workspace must be 256-byte aligned");
  const Workspace ws = carve(workspace, H, W, n_seg);
  PGDVS_REQUIRE(workspace_bytes >= ws.bytes, "pgdvs_mask_combine: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)ws.bytes);
  const hipStream_t st = as_stream(stream);
  const int64_t n = (int64_t)H * W;
  const unsigned pixel_blocks = (unsigned)cdiv(n, kBlock);
  const dim3 tiles((unsigned)cdiv(W, kTileW), (unsigned)cdiv(H, kTileH));

  if (has_prev) {
    WarpParams p;
    p.prev_mask = prev_mask;
    p.prev_cnt = prev_cnt;
    p.flow = reinterpret_cast<const float2 *>(bwd_flow);
    p.coord_diff = reinterpret_cast<const float2 *>(bwd_coord_diff);
    p.warp_prev = warp_prev;
    p.dyn_track = dyn_track;
    p.conj = ws.conj;
    p.cnt_warp = dyn_cnt;
    p.H = H;
    p.W = W;
    p.frames = (float)(img_idx + 1);
    p.track_thres = (float)dyn_track_thres;  // numpy compares the float32 array with the Python scalar in float32
    for (int k = 0; k < 32 * 4; ++k) p.tab.w[k] = cubic_table[k];
    PGDVS_LAUNCH("mask_warp", warp_kernel, dim3(pixel_blocks), dim3(kBlock), 0, st, p);
  }
  {
    ErodeParams p;
    p.raw_no_warp = raw_no_warp;
    p.conj = has_prev ? ws.conj : nullptr;
    p.raw = raw;
    p.raw_eroded = raw_eroded;
    p.H = H;
    p.W = W;
    PGDVS_LAUNCH("mask_erode2", erode2_kernel, tiles, dim3(kBlock), 0, st, p);
  }
  int32_t *counts = seg_counts ? seg_counts : ws.counts;
  uint8_t *selected = seg_selected ? seg_selected : ws.selected;
  if (n_seg > 0) {
    const int64_t words = bit_words(n);
    PGDVS_LAUNCH("mask_pack_bits", pack_bits_kernel, dim3((unsigned)cdiv(words * 64, kBlock)), dim3(kBlock), 0, st, raw_eroded, n,
                 ws.bits, words);
    if (hipMemsetAsync(counts, 0, (size_t)n_seg * 2 * sizeof(int32_t), st) != hipSuccess) {
      set_error("pgdvs_mask_combine: clearing the segment counts failed: %s", hipGetErrorString(hipGetLastError()));
      return PGDVS_ERR_LAUNCH;
    }
    CountParams c;
    c.sam = sam;
    c.bits = ws.bits;
    c.counts = counts;
    c.n = n;
    const dim3 grid((unsigned)cdiv(cdiv(n, 16), kBlock * kCountSteps), (unsigned)n_seg);
    PGDVS_LAUNCH("mask_seg_count", seg_count_kernel, grid, dim3(kBlock), 0, st, c);
    PGDVS_LAUNCH("mask_seg_select", seg_select_kernel, dim3((unsigned)cdiv(n_seg, kBlock)), dim3(kBlock), 0, st, counts, n_seg,
                 sam_overlap_thres, selected);
  }
  {
    UnionParams p;
    p.sam = sam;
    p.selected = selected;
    p.raw_eroded = raw_eroded;
    p.raw_no_warp = raw_no_warp;
    p.final_raw = final_raw;
    p.dyn_cnt = dyn_cnt;
    p.n = n;
    p.n_seg = n_seg;
    p.first_frame = has_prev ? 0 : 1;
    PGDVS_LAUNCH("mask_union", union_kernel, dim3(pixel_blocks), dim3(kBlock), 0, st, p);
  }
  {
    CloseParams p;
    p.final_raw = final_raw;
    p.final_mask = final_mask;
    p.next_prev = next_prev;
    p.H = H;
    p.W = W;
    PGDVS_LAUNCH("mask_close", close_kernel, tiles, dim3(kBlock), 0, st, p);
  }
  return check_launch("pgdvs_mask_combine");
}

PGDVS_API int pgdvs_semantic_mask(const int64_t *sem_ade20k, const int64_t *sem_coco, int H, int W, const int32_t *ids_ade20k,
                                  int n_ade20k, const int32_t *ids_coco, int n_coco, uint8_t *ade20k, uint8_t *coco, uint8_t *sem,
                                  pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(H, W), "pgdvs_semantic_mask: bad shape H=%d W=%d (H, W >= 1, each < 2^20, H W < 2^31)", H, W);
  PGDVS_REQUIRE(sem_ade20k && sem_coco && ade20k && coco && sem && n_ade20k >= 0 && n_coco >= 0 && (ids_ade20k || !n_ade20k) &&
                    (ids_coco || !n_coco),
                "pgdvs_semantic_mask: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(sem_ade20k) & 7) == 0 && (reinterpret_cast<uintptr_t>(sem_coco) & 7) == 0,
                "pgdvs_semantic_mask: the class-id maps must be 8-byte aligned");
  SemanticParams p;
  const int32_t *lists[2] = {ids_ade20k, ids_coco};
  const int counts[2] = {n_ade20k, n_coco};
  for (int k = 0; k < 2; ++k) {
    for (int w = 0; w < 16; ++w) p.listed[k][w] = 0;
    for (int j = 0; j < counts[k]; ++j) {
      const int c = lists[k][j] - 1;  // the lists count from 1, the maps from 0
      PGDVS_REQUIRE(c >= 0 && c < 512, "pgdvs_semantic_mask: class id %d (1 <= id <= 512)", lists[k][j]);
      p.listed[k][c >> 5] |= 1u << (c & 31);
    }
  }
  p.ids[0] = sem_ade20k;
  p.ids[1] = sem_coco;
  p.out[0] = ade20k;
  p.out[1] = coco;
  p.sem = sem;
  p.n = (int64_t)H * W;
  PGDVS_LAUNCH("semantic_mask", semantic_mask_kernel, dim3((unsigned)cdiv(p.n, kBlock)), dim3(kBlock), 0, as_stream(stream), p);
  return check_launch("pgdvs_semantic_mask");
}
