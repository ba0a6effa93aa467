// What upstream's flow stage does with a pair's flows besides running the network (pgdvs/preprocess/compute_flow.py).
//
// tile blend (compute_flow.py:138-165 compute_weight, :182-209, the tile branch of compute_flow_flowformer): one thread per
//   output pixel walks the tiles in index order; a tile that covers the pixel adds tile * w to the pixel's two sums and w to
//   its count, product and sum rounded separately (the library is built with -ffp-contract=off), and the pixel leaves as
//   sum / count, a correctly rounded division.  Upstream adds a zero-padded product for every tile; a tile that does not
//   cover the pixel adds +0 there, which leaves a sum that started at +0 as it is, so skipping it gives the same bits.  The
//   weights at a tile's rim are float32 denormals (sigma 0.05): nothing here flushes them, no reciprocal, no fast division.
//   The tiles arrive planar, as the network returns them, and the flow leaves channel-last, as the .npz stores it.
//
// pair export, first pass (compute_flow.py:335-340 and preprocess/common.py:198-201): a grid-strided kernel over the pixels
//   of both directions (blockIdx.y) that reads a pixel's own flow once, writes its coord_diff (flow_pixel.h, the statement
//   pgdvs_flow_consistency runs) unless the caller wants the pictures alone, and keeps the maximum of
//   rad = sqrt(u u + v v) as an unsigned key (NaN above everything, as np.max).  Each workgroup leaves one key; the second
//   pass (png.hip, flow_pictures_kernel) reduces them again in every row's workgroup, so there is no atomic, no memset and no
//   third launch, and the maximum does not depend on any order.
#include <algorithm>
#include <vector>

#include "common.h"
#include "flow_pixel.h"
#include "wave.h"

namespace pgdvs {
namespace {

// ---- tile blend ----

constexpr int kMaxTiles = 128;
constexpr int kTbBlockX = 64, kTbBlockY = 4;

struct BlendParams {
  const float *tiles;   // [n,2,ph,pw]
  const float *weight;  // [ph,pw]
  float2 *flow;         // [H,W]
  int n, ph, pw, H, W;
  int org[kMaxTiles][2];  // (h, w) per tile
};

__global__ void __launch_bounds__(kTbBlockX *kTbBlockY) flow_tile_blend_kernel(BlendParams p) {
  const int x = blockIdx.x * kTbBlockX + threadIdx.x, y = blockIdx.y * kTbBlockY + threadIdx.y;
  if (x >= p.W || y >= p.H) return;
  const size_t plane = (size_t)p.ph * p.pw;
  float ax = 0.0f, ay = 0.0f, cnt = 0.0f;
  for (int t = 0; t < p.n; ++t) {
    const int ty = y - p.org[t][0], tx = x - p.org[t][1];
    if ((unsigned)ty < (unsigned)p.ph && (unsigned)tx < (unsigned)p.pw) {
      const size_t k = (size_t)ty * p.pw + tx;
      const float w = p.weight[k];
      ax = ax + p.tiles[(2 * (size_t)t) * plane + k] * w;
      ay = ay + p.tiles[(2 * (size_t)t + 1) * plane + k] * w;
      cnt = cnt + w;
    }
  }
  p.flow[(size_t)y * p.W + x] = make_float2(ax / cnt, ay / cnt);
}

// Do the tiles cover [0,H) x [0,W)?  On the grid of the tiles' own edges: every cell lies wholly inside or outside a tile.
bool tiles_cover(const int32_t *origins, int n, int ph, int pw, int H, int W) {
  auto edges = [n, origins](int axis, int size, int limit) {
    std::vector<int> e{0, limit};
    for (int t = 0; t < n; ++t) {
      e.push_back(origins[2 * t + axis]);
      e.push_back(origins[2 * t + axis] + size);
    }
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());
    return e;
  };
  const std::vector<int> ys = edges(0, ph, H), xs = edges(1, pw, W);
  const int ny = (int)ys.size() - 1, nx = (int)xs.size() - 1;
  std::vector<uint8_t> hit((size_t)ny * nx, 0);
  for (int t = 0; t < n; ++t) {
    const int h = origins[2 * t], w = origins[2 * t + 1];
    for (int j = 0; j < ny; ++j) {
      if (ys[j] < h || ys[j + 1] > h + ph) continue;
      for (int i = 0; i < nx; ++i)
        if (xs[i] >= w && xs[i + 1] <= w + pw) hit[(size_t)j * nx + i] = 1;
    }
  }
  for (uint8_t v : hit)
    if (!v) return false;
  return true;
}

// ---- pair export, first pass ----

constexpr int kP1Block = 256;
constexpr int kP1Blocks = 1024;  // workgroups per direction at most: one grid round is kP1Blocks kP1Block pixels

struct Pass1Params {
  const float2 *flow[2];  // flow12, flow21
  float2 *out[2];         // coord_diff_1, coord_diff_2, or both null
  uint32_t *keys;         // [2][gridDim.x]
  int H, W;
};

__global__ void __launch_bounds__(kP1Block) flow_pair_pass1_kernel(Pass1Params p) {
  __shared__ uint32_t s_key[kP1Block / kWave];
  const int dir = blockIdx.y;
  const float2 *__restrict__ mine = p.flow[dir];
  const float2 *__restrict__ other = p.flow[1 - dir];  // (null, and unread, for one picture alone)
  float2 *__restrict__ out = p.out[dir];
  const int64_t n = (int64_t)p.H * p.W, stride = (int64_t)gridDim.x * kP1Block;
  uint32_t key = 0u;
  for (int64_t i = (int64_t)blockIdx.x * kP1Block + threadIdx.x; i < n; i += stride) {
    const float2 f = mine[i];
    if (out) {
      const int y = (int)(i / p.W), x = (int)(i - (int64_t)y * p.W);
      out[i] = coord_diff_pixel(f, other, x, y, p.H, p.W);
    }
    key = max(key, rad_key(sqrtf(f.x * f.x + f.y * f.y)));
  }
  key = wave_reduce_all<OpMax>(key);  // (every lane is here: the loop has no early exit)
  if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kP1Block / kWave; ++w) key = max(key, s_key[w]);
    p.keys[(size_t)dir * gridDim.x + blockIdx.x] = key;
  }
}

int64_t pass1_blocks(int H, int W) {
  const int64_t b = cdiv((int64_t)H * W, kP1Block);
  return b < kP1Blocks ? b : kP1Blocks;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_flow_tile_blend(const float *tiles, const int32_t *origins, int n, int ph, int pw, const float *weight, int H,
                                    int W, float *flow, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(tiles && origins && weight && flow, "pgdvs_flow_tile_blend: null pointer");
  PGDVS_REQUIRE(n >= 1 && n <= kMaxTiles, "pgdvs_flow_tile_blend: %d tiles (1 .. %d)", n, kMaxTiles);
  PGDVS_REQUIRE(ph >= 1 && pw >= 1 && H >= ph && W >= pw && H <= (1 << 18) - 4 && (int64_t)H * W < (1ll << 31),
                "pgdvs_flow_tile_blend: bad shape H=%d W=%d for %d x %d tiles (1 <= ph <= H, 1 <= pw <= W, H < 2^18 - 4, H W < 2^31)",
                H, W, ph, pw);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(tiles) & 3) == 0 && (reinterpret_cast<uintptr_t>(weight) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(flow) & 7) == 0,
                "pgdvs_flow_tile_blend: tiles and weight must be 4-byte aligned, flow 8-byte aligned");
  for (int t = 0; t < n; ++t)
    PGDVS_REQUIRE(origins[2 * t] >= 0 && origins[2 * t] <= H - ph && origins[2 * t + 1] >= 0 && origins[2 * t + 1] <= W - pw,
                  "pgdvs_flow_tile_blend: origin %d = (%d, %d) puts a %d x %d tile outside the %d x %d image", t, origins[2 * t],
                  origins[2 * t + 1], ph, pw, H, W);
  PGDVS_REQUIRE(tiles_cover(origins, n, ph, pw, H, W), "pgdvs_flow_tile_blend: the %d tiles leave a pixel of the %d x %d image uncovered",
                n, H, W);
  BlendParams p;
  p.tiles = tiles;
  p.weight = weight;
  p.flow = reinterpret_cast<float2 *>(flow);
  p.n = n;
  p.ph = ph;
  p.pw = pw;
  p.H = H;
  p.W = W;
  for (int t = 0; t < kMaxTiles; ++t) {
    p.org[t][0] = t < n ? origins[2 * t] : 0;
    p.org[t][1] = t < n ? origins[2 * t + 1] : 0;
  }
  const dim3 grid((unsigned)cdiv(W, kTbBlockX), (unsigned)cdiv(H, kTbBlockY));
  PGDVS_LAUNCH("flow_tile_blend", flow_tile_blend_kernel, grid, dim3(kTbBlockX, kTbBlockY), 0, as_stream(stream), p);
  return check_launch("pgdvs_flow_tile_blend");
}

PGDVS_API int64_t pgdvs_flow_pair_export_workspace_bytes(int H, int W) {
  if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) {
    set_error("pgdvs_flow_pair_export_workspace_bytes: bad shape H=%d W=%d (each >= 1, H W < 2^31)", H, W);
    return PGDVS_ERR_INVALID;
  }
  Carver c{nullptr};
  c.take<uint32_t>(2 * pass1_blocks(H, W) * (int64_t)sizeof(uint32_t));
  return c.off;
}

PGDVS_API int pgdvs_flow_pair_export(const float *flow12, const float *flow21, int H, int W, int adaptive, float *coord_diff_1,
                                     float *coord_diff_2, float *rad_max, uint8_t *out, void *workspace, int64_t workspace_bytes,
                                     pgdvs_stream_t stream) {
  PGDVS_REQUIRE(flow12 && rad_max && out && workspace, "pgdvs_flow_pair_export: null pointer");
  PGDVS_REQUIRE(flow21 || !coord_diff_1, "pgdvs_flow_pair_export: flow21 may be NULL only for one picture alone (no coord_diff)");
  const int n_img = flow21 ? 2 : 1;
  PGDVS_REQUIRE((coord_diff_1 == nullptr) == (coord_diff_2 == nullptr),
                "pgdvs_flow_pair_export: coord_diff_1 and coord_diff_2 go together (both NULL: the pictures alone)");
  const int min_side = coord_diff_1 ? 2 : 1;
  PGDVS_REQUIRE(H >= min_side && W >= min_side && (int64_t)H * W < (1ll << 31) && 2 * (int64_t)H * (1 + 3 * (int64_t)W) < (1ll << 31),
                "pgdvs_flow_pair_export: bad shape H=%d W=%d (each >= %d: upstream's consistency divides by W - 1; "
                "2 H (1 + 3 W) < 2^31)", H, W, min_side);
  PGDVS_REQUIRE(adaptive == 0 || adaptive == 1, "pgdvs_flow_pair_export: adaptive %d (0 / 1)", adaptive);
  PGDVS_REQUIRE(((reinterpret_cast<uintptr_t>(flow12) | reinterpret_cast<uintptr_t>(flow21) | reinterpret_cast<uintptr_t>(coord_diff_1) |
                  reinterpret_cast<uintptr_t>(coord_diff_2)) & 7) == 0 && (reinterpret_cast<uintptr_t>(rad_max) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "pgdvs_flow_pair_export: flows and coord_diffs must be 8-byte aligned, rad_max 4-byte, the workspace 256-byte");
  const int64_t need = pgdvs_flow_pair_export_workspace_bytes(H, W);
  PGDVS_REQUIRE(workspace_bytes >= need, "pgdvs_flow_pair_export: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)need);
  const int blocks = (int)pass1_blocks(H, W);
  Carver c{static_cast<char *>(workspace)};
  Pass1Params p;
  p.flow[0] = reinterpret_cast<const float2 *>(flow12);
  p.flow[1] = reinterpret_cast<const float2 *>(flow21);
  p.out[0] = reinterpret_cast<float2 *>(coord_diff_1);
  p.out[1] = reinterpret_cast<float2 *>(coord_diff_2);
  p.keys = c.take<uint32_t>(2 * (int64_t)blocks * (int64_t)sizeof(uint32_t));
  p.H = H;
  p.W = W;
  PGDVS_LAUNCH("flow_pair_pass1", flow_pair_pass1_kernel, dim3((unsigned)blocks, (unsigned)n_img), dim3(kP1Block), 0, as_stream(stream), p);
  const int rc = check_launch("pgdvs_flow_pair_export");
  if (rc != PGDVS_OK) return rc;
  return launch_flow_pictures(flow12, flow21, n_img, H, W, adaptive, p.keys, blocks, rad_max, out, as_stream(stream));
}
