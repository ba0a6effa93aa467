// The two stages of upstream's pgdvs/preprocess/ that are its own per-pixel arithmetic (the rest wraps networks).
//
// flow consistency (preprocess/common.py:211-233, 314-325 compute_occlusion(return_raw=True); compute_flow.py:335-340): one
//   thread per pixel and direction (blockIdx.z).  Its own flow is one coalesced 8-byte load; the four corners of the other
//   flow are gathered straight from global memory (neighbouring lanes land on neighbouring texels; nothing is staged).
//   Everything is float32 in upstream's order, every operation rounded on its own (the library is built with
//   -ffp-contract=off): c1 = p + flow, g = 2 c1 / (W - 1) - 1, then grid_sample's own ((g + 1) / 2) (W - 1), the weights
//   w = ix - floor(ix) and 1 - w, the sum nw + ne + sw + se, c2 = c1 + sample, p - c2.  Whether a corner lies in the image
//   is decided on the float coordinate, before any conversion to int: no flow value, however large, reaches an address.
//
// epipolar mask (preprocess/compute_mask.py:160-181, 196-215, 311-338): one workgroup per 64 x 16 tile of the mask.  It
//   computes raw = (e_dist > threshold) for the tile and a 2-pixel halo straight from coalesced loads of flow and
//   coord_diff, keeps only the BITS in LDS (one byte per pixel), erodes the tile plus a 1-pixel halo and dilates the tile,
//   both with the 3 x 3 cross = skimage's disk(1).  Borders as skimage's binary_opening: the erosion reads set pixels
//   outside the image, the dilation clear ones.  The distance is float64 in numpy's order; l = F p follows the BLAS
//   product (k ascending, fused), which the fixture's guard band makes immaterial for the mask.
#include <cmath>

#include "common.h"
#include "flow_pixel.h"

namespace pgdvs {
namespace {

// ---- flow consistency ----

constexpr int kFcBlockX = 64, kFcBlockY = 4;

struct FcParams {
  const float2 *flow[2];  // [H,W] (x, y) each: flow12, flow21
  float2 *out[2];         // coord_diff_1, coord_diff_2
  int H, W;
};

__global__ void __launch_bounds__(kFcBlockX *kFcBlockY) flow_consistency_kernel(FcParams p) {
  const int x = blockIdx.x * kFcBlockX + threadIdx.x, y = blockIdx.y * kFcBlockY + threadIdx.y;
  if (x >= p.W || y >= p.H) return;
  const int dir = blockIdx.z;
  const float2 *__restrict__ mine = p.flow[dir];
  const float2 *__restrict__ other = p.flow[1 - dir];
  const size_t i = (size_t)y * p.W + x;
  p.out[dir][i] = coord_diff_pixel(mine[i], other, x, y, p.H, p.W);
}

// ---- epipolar mask ----

constexpr int kTileW = 64, kTileH = 16, kEpiBlock = 256;
constexpr int kRawW = kTileW + 4, kRawH = kTileH + 4;  // the tile and a 2-pixel halo
constexpr int kEroW = kTileW + 2, kEroH = kTileH + 2;  // the tile and a 1-pixel halo

struct EpiParams {
  const float2 *flow;        // [H,W]
  const float2 *coord_diff;  // [H,W]
  uint8_t *mask;             // [H,W]
  double *e_dist;            // [H,W] or null
  int H, W;
  double F[9];
  double threshold;
  float consist_thres;
};

__global__ void __launch_bounds__(kEpiBlock) epipolar_mask_kernel(EpiParams p) {
  __shared__ uint8_t raw[kRawH][kRawW];
  __shared__ uint8_t ero[kEroH][kEroW];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;

  // raw over the tile and its 2-pixel halo; consecutive threads walk a row: coalesced 8-byte loads
  for (int k = threadIdx.x; k < kRawH * kRawW; k += kEpiBlock) {
    const int ry = k / kRawW, rx = k - ry * kRawW;
    const int x = tx0 + rx - 2, y = ty0 + ry - 2;
    uint8_t bit = 1;  // outside the image: set, as the erosion's border_value
    if (x >= 0 && x < p.W && y >= 0 && y < p.H) {
      const size_t i = (size_t)y * p.W + x;
      const float2 f = p.flow[i], cd = p.coord_diff[i];
      const double xd = (double)x, yd = (double)y;
      const double p2x = (double)((float)x + f.x), p2y = (double)((float)y + f.y);
      double l[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) l[r] = __builtin_fma(p.F[r * 3 + 2], 1.0, __builtin_fma(p.F[r * 3 + 1], yd, p.F[r * 3 + 0] * xd));
      const double alg = (p2x * l[0] + p2y * l[1]) + 1.0 * l[2];
      const double n_term = sqrt(l[0] * l[0] + l[1] * l[1]) + 1e-8;
      const double d = fabs(alg / n_term);
      const bool consistent = (fabsf(cd.x) + fabsf(cd.y)) <= p.consist_thres;
      const double e = d * (consistent ? 1.0 : 0.0);
      bit = e > p.threshold ? 1 : 0;
      // the tile's own pixels are written by this workgroup alone
      if (p.e_dist && rx >= 2 && rx < kTileW + 2 && ry >= 2 && ry < kTileH + 2) p.e_dist[i] = e;
    }
    raw[ry][rx] = bit;
  }
  __syncthreads();

  // erosion over the tile and its 1-pixel halo; outside the image the result is clear, as the dilation's border_value
  for (int k = threadIdx.x; k < kEroH * kEroW; k += kEpiBlock) {
    const int ey = k / kEroW, ex = k - ey * kEroW;
    const int x = tx0 + ex - 1, y = ty0 + ey - 1;
    uint8_t bit = 0;
    if (x >= 0 && x < p.W && y >= 0 && y < p.H) {
      const int ry = ey + 1, rx = ex + 1;
      bit = raw[ry][rx] & raw[ry - 1][rx] & raw[ry + 1][rx] & raw[ry][rx - 1] & raw[ry][rx + 1];
    }
    ero[ey][ex] = bit;
  }
  __syncthreads();

  // dilation over the tile
  for (int k = threadIdx.x; k < kTileH * kTileW; k += kEpiBlock) {
    const int ty = k / kTileW, tx = k - ty * kTileW;
    const int x = tx0 + tx, y = ty0 + ty;
    if (x >= p.W || y >= p.H) continue;
    const int ey = ty + 1, ex = tx + 1;
    p.mask[(size_t)y * p.W + x] = ero[ey][ex] | ero[ey - 1][ex] | ero[ey + 1][ex] | ero[ey][ex - 1] | ero[ey][ex + 1];
  }
}

// grid.y carries rows: H / 4 (flow consistency) stays below 65536 up to H = 262140
bool shape_ok(int H, int W) {
  return H >= 2 && W >= 2 && H <= (1 << 18) - 4 && (int64_t)H * W < (1ll << 31);
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define FC_SHAPE_MSG "pgdvs_flow_consistency: bad shape H=%d W=%d (each >= 2: upstream divides by W - 1; H < 2^18 - 4, H W < 2^31)"

PGDVS_API int pgdvs_flow_consistency(const float *flow12, const float *flow21, int H, int W, float *coord_diff_1,
                                     float *coord_diff_2, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(flow12 && flow21 && coord_diff_1 && coord_diff_2, "pgdvs_flow_consistency: null pointer");
  PGDVS_REQUIRE(shape_ok(H, W), FC_SHAPE_MSG, H, W);
  const float *in[2] = {flow12, flow21};
  float *out[2] = {coord_diff_1, coord_diff_2};
  for (int k = 0; k < 2; ++k)
    PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(in[k]) & 7) == 0 && (reinterpret_cast<uintptr_t>(out[k]) & 7) == 0,
                  "pgdvs_flow_consistency: pointers must be 8-byte aligned");
  FcParams p;
  for (int k = 0; k < 2; ++k) {
    p.flow[k] = reinterpret_cast<const float2 *>(in[k]);
    p.out[k] = reinterpret_cast<float2 *>(out[k]);
  }
  p.H = H;
  p.W = W;
  const dim3 grid((unsigned)cdiv(W, kFcBlockX), (unsigned)cdiv(H, kFcBlockY), 2);
  PGDVS_LAUNCH("flow_consistency", flow_consistency_kernel, grid, dim3(kFcBlockX, kFcBlockY), 0, as_stream(stream), p);
  return check_launch("pgdvs_flow_consistency");
}

#define EPI_SHAPE_MSG "pgdvs_epipolar_mask: bad shape H=%d W=%d (each >= 2, H < 2^18 - 4, H W < 2^31)"

PGDVS_API int pgdvs_epipolar_mask(const float *flow, const float *coord_diff, int H, int W, const double *F, double consist_thres,
                                  double threshold, uint8_t *mask, double *e_dist, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(flow && coord_diff && F && mask, "pgdvs_epipolar_mask: null pointer");
  PGDVS_REQUIRE(shape_ok(H, W), EPI_SHAPE_MSG, H, W);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 7) == 0 && (reinterpret_cast<uintptr_t>(coord_diff) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(e_dist) & 7) == 0,
                "pgdvs_epipolar_mask: flow, coord_diff and e_dist must be 8-byte aligned");
  EpiParams p;
  p.flow = reinterpret_cast<const float2 *>(flow);
  p.coord_diff = reinterpret_cast<const float2 *>(coord_diff);
  p.mask = mask;
  p.e_dist = e_dist;
  p.H = H;
  p.W = W;
  for (int k = 0; k < 9; ++k) p.F[k] = F[k];
  p.threshold = threshold;
  p.consist_thres = (float)consist_thres;  // numpy compares the float32 sum with the Python scalar in float32
  const dim3 grid((unsigned)cdiv(W, kTileW), (unsigned)cdiv(H, kTileH));
  PGDVS_LAUNCH("epipolar_mask", epipolar_mask_kernel, grid, dim3(kEpiBlock), 0, as_stream(stream), p);
  return check_launch("pgdvs_epipolar_mask");
}
