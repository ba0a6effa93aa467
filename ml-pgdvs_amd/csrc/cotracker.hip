// CoTracker's correlation step (pgdvs/models/cotracker/models/core/cotracker/blocks.py:269-328 CorrBlock) without the
// correlation volume.  include/pgdvs_hip.h states what is computed; this is how.
//
// pyramid  level 0 is fmaps[S,128,H,W] turned channels-last through a 32-pixel x 128-channel LDS tile (reads coalesced
//          along x, writes along c); levels 1..3 are 2 x 2 means of the level before, one thread per pixel and four
//          channels: ((a00 + a01) + a10) + a11, then * 0.25, avg_pool2d's own order.  Four launches.
// lookup   one workgroup per (s, n), one wavefront per level.  Bilinear sampling is linear, so <feat, bilinear(fmap)> =
//          bilinear(<feat, fmap>): the 49 samples of a level lie on one 7 x 7 unit grid and read an 8 x 8 block of taps.
//          A half-wavefront covers one tap line (32 lanes x 16 bytes = 128 channels), so a step takes two taps; after 32
//          steps every lane holds 32 partial dots, which a halving butterfly (16 + 8 + 4 + 2 + 1 shuffles) turns into one
//          finished dot per lane: lane 32 h + c holds tap 2 c + h.  The 64 dots go through LDS, and lanes 0..48 each
//          blend one sample from its 2 x 2 taps.  A tap outside the level is 0 and is never addressed.  One launch.
//          Within a few float32 spacings of an integer coordinate the reference's round trip can put the first sample
//          just below its integer and the last just above: the samples then touch nine taps along that axis, and the
//          wavefront fetches the ninth column and row in a short second pass (half-wavefront sums by five shuffles).
#include "common.h"

namespace pgdvs {
namespace {

constexpr int kC = 128;           // CoTracker's latent_dim; a tap line is 512 bytes
constexpr int kLevels = 4;        // corr_levels
constexpr int kRadius = 3;        // corr_radius: 7 x 7 samples, 8 x 8 taps
constexpr int kSamples = 2 * kRadius + 1;
constexpr int kTaps = kSamples + 1;
constexpr int kPerLevel = kSamples * kSamples;  // 49
constexpr int kOut = kLevels * kPerLevel;       // 196
constexpr int kBlock = 256;
constexpr int kTilePx = 32;
constexpr float kCoordClamp = 16.0f;  // a centre this far outside the level has no tap inside it

struct Levels {
  float *base[kLevels];  // [S, H_l, W_l, 128]
  int H[kLevels], W[kLevels];
  int64_t bytes;
};

Levels carve(void *ws, int S, int H, int W) {
  Carver c{static_cast<char *>(ws)};
  Levels l;
  for (int i = 0; i < kLevels; ++i) {
    l.H[i] = H >> i;
    l.W[i] = W >> i;
    l.base[i] = c.take<float>((int64_t)S * l.H[i] * l.W[i] * kC * (int64_t)sizeof(float));
  }
  l.bytes = c.off;
  return l;
}

bool shape_ok(int S, int C, int H, int W) {
  return S >= 1 && C == kC && H >= (2 << (kLevels - 1)) && W >= (2 << (kLevels - 1)) && H < (1 << 15) && W < (1 << 15) &&
         (int64_t)S * H * W < (1ll << 31);
}

// ---- level 0: [S,128,H,W] -> [S,H,W,128] ----

__global__ void __launch_bounds__(kBlock) channels_last_kernel(const float *__restrict__ fmaps, float *__restrict__ out, int64_t HW) {
  __shared__ float tile[kC][kTilePx + 1];
  const int s = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * kTilePx;
  const float *__restrict__ src = fmaps + (int64_t)s * kC * HW;
  for (int k = threadIdx.x; k < kC * kTilePx; k += kBlock) {
    const int c = k / kTilePx, px = k - c * kTilePx;
    if (p0 + px < HW) tile[c][px] = src[(int64_t)c * HW + p0 + px];
  }
  __syncthreads();
  float *__restrict__ dst = out + ((int64_t)s * HW + p0) * kC;
  for (int k = threadIdx.x; k < kC * kTilePx; k += kBlock) {
    const int px = k / kC, c = k - px * kC;
    if (p0 + px < HW) dst[(int64_t)px * kC + c] = tile[c][px];
  }
}

// ---- levels 1..3: avg_pool2d(2, stride 2), an odd last row or column dropped ----

__global__ void __launch_bounds__(kBlock) pool_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, int S, int Hi, int Wi,
                                                      int Ho, int Wo) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (int64_t)S * Ho * Wo * (kC / 4)) return;
  const int c4 = (int)(i % (kC / 4));
  int64_t r = i / (kC / 4);
  const int x = (int)(r % Wo);
  r /= Wo;
  const int y = (int)(r % Ho), s = (int)(r / Ho);
  const int64_t row0 = ((int64_t)s * Hi + 2 * y) * Wi + 2 * x;  // 2 y + 1 < Hi and 2 x + 1 < Wi: Ho = Hi / 2, Wo = Wi / 2
  const float4 a = in[row0 * (kC / 4) + c4], b = in[(row0 + 1) * (kC / 4) + c4];
  const float4 c = in[(row0 + Wi) * (kC / 4) + c4], d = in[(row0 + Wi + 1) * (kC / 4) + c4];
  float4 o;
  o.x = (((a.x + b.x) + c.x) + d.x) * 0.25f;
  o.y = (((a.y + b.y) + c.y) + d.y) * 0.25f;
  o.z = (((a.z + b.z) + c.z) + d.z) * 0.25f;
  o.w = (((a.w + b.w) + c.w) + d.w) * 0.25f;
  out[i] = o;
}

// ---- lookup ----

struct LookupParams {
  const float *lvl[kLevels];
  int H[kLevels], W[kLevels];
  const float *feats;   // [S,N,128]
  const float *coords;  // [S,N,2]
  float *out;
  int64_t row_stride, col_offset;
  int N;
};

// bilinear_sampler followed by grid_sample(align_corners=True)'s own unnormalisation, every operation rounded to float32
__device__ __forceinline__ float round_trip(float x, float extent_m1) {
  const float g = __fdiv_rn(2.0f * x, extent_m1) - 1.0f;
  return __fdiv_rn(g + 1.0f, 2.0f) * extent_m1;
}

// the cell of a round-tripped position: clamped as a FLOAT before it becomes an integer (a NaN becomes -16); beyond the
// clamp no tap lies in the level either way
__device__ __forceinline__ int cell(float pos, int extent) {
  return (int)floorf(fminf(fmaxf(pos, -kCoordClamp), (float)extent + kCoordClamp));
}

// The taps of one axis: the 7 samples sit one pixel apart, so their cells are first + i ... except within a few float32
// spacings of an integer, where the round trip puts some samples one cell lower than others.  first = the lowest
// cell_i - i; ninth = whether the last sample then reaches a ninth tap (first + 8).
__device__ __forceinline__ int axis_taps(float centre, float extent_m1, int extent, bool &ninth) {
  int first = INT32_MAX, last = 0;
#pragma unroll
  for (int i = 0; i < kSamples; ++i) {
    last = cell(round_trip(centre + (float)(i - kRadius), extent_m1), extent) - i;
    first = last < first ? last : first;
  }
  ninth = last > first;
  return first;
}

// weight of tap k (counted from the first tap) for a sample p taps from the first one: the hat 1 - |p - k|, which is
// grid_sample's (x_se - x) on the sample's own cell and (x - x_nw) on the next
__device__ __forceinline__ float hat(float p, int k) { return fmaxf(1.0f - fabsf(p - (float)k), 0.0f); }

__device__ __forceinline__ float dot4(float4 f, float4 v) { return ((f.x * v.x + f.y * v.y) + f.z * v.z) + f.w * v.w; }

constexpr int kDotsW = kTaps + 1;  // 9 x 9: the 8 x 8 block and the ninth column and row

__global__ void __launch_bounds__(kBlock) corr_lookup_kernel(LookupParams p) {
  __shared__ float dots[kLevels][kDotsW * kDotsW];
  const int lane = threadIdx.x & (kWave - 1), level = threadIdx.x / kWave;
  const int half = lane >> 5, c = lane & 31;
  const int64_t sn = blockIdx.x;
  const int s = (int)(sn / p.N);
  const int H = p.H[level], W = p.W[level];
  const float scale = 1.0f / (float)(1 << level);
  const float cx = p.coords[sn * 2] * scale, cy = p.coords[sn * 2 + 1] * scale;  // coords / 2^level, exact
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  bool ninth_x, ninth_y;  // the same in every lane of the wavefront
  const int x0 = axis_taps(cx, wm1, W, ninth_x), y0 = axis_taps(cy, hm1, H, ninth_y);
  const float norm = sqrtf((float)kC);  // corrs / sqrt(C): the reference divides by the float32 square root

  const float4 f = reinterpret_cast<const float4 *>(p.feats + sn * kC)[c];
  const float *__restrict__ base = p.lvl[level] + (int64_t)s * H * W * kC;
  float acc[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {  // this half-wavefront's tap of step k: row k / 4, column 2 (k % 4) + half
    const int ty = y0 + (k >> 2), tx = x0 + 2 * (k & 3) + half;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ty >= 0 && ty < H && tx >= 0 && tx < W) v = reinterpret_cast<const float4 *>(base + ((int64_t)ty * W + tx) * kC)[c];
    acc[k] = dot4(f, v);
  }
  // halving butterfly over the 32 lanes of a half: at width w a lane keeps the half of its values that its bit w selects
  // and adds the partner's copy of them; lane c ends with the whole dot of step c
#pragma unroll
  for (int w = 16; w >= 1; w >>= 1) {
    const bool upper = (c & w) != 0;
#pragma unroll
    for (int j = 0; j < w; ++j) {
      const float keep = upper ? acc[j + w] : acc[j];
      const float send = upper ? acc[j] : acc[j + w];
      acc[j] = keep + __shfl_xor(send, w, kWave);
    }
  }
  dots[level][(c >> 2) * kDotsW + 2 * (c & 3) + half] = __fdiv_rn(acc[0], norm);
  if (ninth_x || ninth_y) {  // rare: coordinates within a few float32 spacings of integers
    for (int e0 = 0; e0 < 2 * kTaps + 1; e0 += 2) {  // e < 9: column 8, row e; else row 8, column e - 9
      const int e = e0 + half;
      const int kx = e < kDotsW ? kTaps : e - kDotsW, ky = e < kDotsW ? e : kTaps;
      const int tx = x0 + kx, ty = y0 + ky;
      const bool live = e <= 2 * kTaps && (kx < kTaps || ninth_x) && (ky < kTaps || ninth_y);
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (live && ty >= 0 && ty < H && tx >= 0 && tx < W) v = reinterpret_cast<const float4 *>(base + ((int64_t)ty * W + tx) * kC)[c];
      float d = dot4(f, v);
      for (int off = 16; off > 0; off >>= 1) d += __shfl_xor(d, off, kWave);
      if (c == 0 && live) dots[level][ky * kDotsW + kx] = __fdiv_rn(d, norm);
    }
  }
  __syncthreads();
  if (lane >= kPerLevel) return;
  const int i = lane / kSamples, j = lane - i * kSamples;  // the slow index moves x (delta is (dy, dx) added to (x, y))
  const float px = round_trip(cx + (float)(i - kRadius), wm1) - (float)x0;
  const float py = round_trip(cy + (float)(j - kRadius), hm1) - (float)y0;
  // the sample's cell among the taps; one that is not finite or far outside gets a cell without taps, or weights 0
  const int kx = (int)floorf(fminf(fmaxf(px, -1.0f), (float)kDotsW)), ky = (int)floorf(fminf(fmaxf(py, -1.0f), (float)kDotsW));
  float v = 0.0f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int tx = kx + dx, ty = ky + dy;
      const bool have = tx >= 0 && ty >= 0 && (tx < kTaps || (tx == kTaps && ninth_x)) && (ty < kTaps || (ty == kTaps && ninth_y));
      if (have) v += dots[level][ty * kDotsW + tx] * (hat(px, tx) * hat(py, ty));
    }
  p.out[sn * p.row_stride + p.col_offset + level * kPerLevel + lane] = v;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define CT_SHAPE_MSG "%s: bad shape S=%d C=%d H=%d W=%d (S >= 1, C = 128, 16 <= H, W < 2^15 so that every level is 2 x 2 or more, S H W < 2^31)"

PGDVS_API int64_t pgdvs_cotracker_pyramid_workspace_bytes(int S, int C, int H, int W) {
  PGDVS_REQUIRE(shape_ok(S, C, H, W), CT_SHAPE_MSG, "pgdvs_cotracker_pyramid_workspace_bytes", S, C, H, W);
  return carve(nullptr, S, H, W).bytes;
}

PGDVS_API int pgdvs_cotracker_pyramid(const float *fmaps, int S, int C, int H, int W, void *workspace, int64_t workspace_bytes,
                                      pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(S, C, H, W), CT_SHAPE_MSG, "pgdvs_cotracker_pyramid", S, C, H, W);
  PGDVS_REQUIRE(fmaps && workspace, "pgdvs_cotracker_pyramid: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(fmaps) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "pgdvs_cotracker_pyramid: fmaps must be 4-byte aligned, the workspace 256-byte");
  const Levels l = carve(workspace, S, H, W);
  PGDVS_REQUIRE(workspace_bytes >= l.bytes, "pgdvs_cotracker_pyramid: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)l.bytes);
  PGDVS_REQUIRE(S < 65536, "pgdvs_cotracker_pyramid: S=%d (frames ride grid.y: S < 65536)", S);
  const hipStream_t st = as_stream(stream);
  const int64_t HW = (int64_t)H * W;
  PGDVS_LAUNCH("cotracker_channels_last", channels_last_kernel, dim3((unsigned)cdiv(HW, kTilePx), (unsigned)S), dim3(kBlock), 0, st, fmaps,
               l.base[0], HW);
  for (int i = 1; i < kLevels; ++i) {
    const int64_t n = (int64_t)S * l.H[i] * l.W[i] * (kC / 4);
    PGDVS_LAUNCH("cotracker_pool", pool_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st,
                 reinterpret_cast<const float4 *>(l.base[i - 1]), reinterpret_cast<float4 *>(l.base[i]), S, l.H[i - 1], l.W[i - 1], l.H[i],
                 l.W[i]);
  }
  return check_launch("pgdvs_cotracker_pyramid");
}

PGDVS_API int pgdvs_cotracker_corr_lookup(const void *pyramid, int S, int H, int W, const float *feats, const float *coords, int N,
                                          float *out, int64_t row_stride, int64_t col_offset, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(S, kC, H, W), CT_SHAPE_MSG, "pgdvs_cotracker_corr_lookup", S, kC, H, W);
  PGDVS_REQUIRE(N >= 1 && (int64_t)S * N * kOut < (1ll << 31), "pgdvs_cotracker_corr_lookup: S=%d N=%d (N >= 1, S N 196 < 2^31)", S, N);
  PGDVS_REQUIRE(col_offset >= 0 && row_stride >= col_offset + kOut,
                "pgdvs_cotracker_corr_lookup: row_stride=%lld col_offset=%lld (0 <= col_offset, col_offset + 196 <= row_stride)",
                (long long)row_stride, (long long)col_offset);
  PGDVS_REQUIRE(pyramid && feats && coords && out, "pgdvs_cotracker_corr_lookup: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(pyramid) & 255) == 0 && (reinterpret_cast<uintptr_t>(feats) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(coords) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "pgdvs_cotracker_corr_lookup: the pyramid must be 256-byte aligned, feats 16-byte, coords and out 4-byte");
  const Levels l = carve(const_cast<void *>(pyramid), S, H, W);
  LookupParams p;
  for (int i = 0; i < kLevels; ++i) {
    p.lvl[i] = l.base[i];
    p.H[i] = l.H[i];
    p.W[i] = l.W[i];
  }
  p.feats = feats;
  p.coords = coords;
  p.out = out;
  p.row_stride = row_stride;
  p.col_offset = col_offset;
  p.N = N;
  PGDVS_LAUNCH("cotracker_corr_lookup", corr_lookup_kernel, dim3((unsigned)((int64_t)S * N)), dim3(kBlock), 0, as_stream(stream), p);
  return check_launch("pgdvs_cotracker_corr_lookup");
}
