// SURVEY 8f-3 NVIDIA: the depth range of one NVIDIA-family loader item (nvidia_eval.py:446-456, nvidia_vis.py:405-417,
// mono_vis.py), bit-identical to the loaders' numpy path (pgdvs_amd/datasets/nvidia_eval.py compute_pcl +
// depth_range_from_points): near = max(1e-16, 0.8 min z), far = max(2e-16, 1.2 np.quantile(z, 0.9)), z the spatial
// sources' world points in the target camera.
//
// points   one thread per spatial pixel (view-major, as the loaders concatenate them).  Unprojection as compute_pcl's
//          float32 `M @ pix` reaches BLAS: d = fma(M[:,1], v, M[:,0] u) + M[:,2] (fused, k ascending), then X = o + d depth
//          as a separately rounded multiply and add.  z = row 2 of inv(c2w_tgt) @ [X,1] in float64, same order; its
//          order-preserving key goes to the workspace.
// select   three ranks through the shared radix select (radix_select.h, 6 passes of 11-bit digits): rank 0 (np.min) and
//          the two neighbours of np.quantile's virtual index (n - 1) 0.9.  The last select pass interpolates with numpy's
//          _lerp, scales, clamps as Python's max compares and writes both outputs.
//
// ZoeDepth (nvidia_eval.py:869-945): pgdvs_nvidia_zoe_depth_range puts the loader's alignment of a monocular prediction in
// front of the same select.  zoe_points turns each prediction into the aligned depth (float32 reciprocal, then scale,
// shift and reciprocal in float64, every operation rounded on its own, as NumPy 2 promotes upstream's three lines), stores
// its float32 rounding and, on the range path, unprojects with the float64 depth still in registers: X = o + d depth in
// float64, as upstream's float32 torch rays times a float64 numpy depth give.  Without the range arguments it is the
// conversion alone (temporal and tracker views): one launch per kZoeViews views, no workspace.
#include <cmath>

#include "common.h"
#include "radix_select.h"

namespace pgdvs {
namespace {

using radix::Key;
using radix::kBins;
using radix::kBlock;
constexpr int kRanks = 3;  // min, quantile floor, quantile floor + 1
typedef Key<double>::U U;

struct Params {
  const float *depth;  // [V,H,W]
  const float *rays;   // [V,12]: M (3x3 row-major), o
  int H, W;
  int64_t n;           // V H W
  double A2[4];        // row 2 of inv(c2w_tgt)
  int64_t rank[kRanks];
  double gamma;
};

struct State {
  radix::Sel<kRanks> sel;
  uint32_t nan_seen;
};

__global__ void __launch_bounds__(kBlock) points_kernel(Params p, U *__restrict__ keys, State *__restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const int64_t HW = (int64_t)p.H * p.W;
  const int v = (int)(i / HW);
  const int64_t pix = i - (int64_t)v * HW;
  const int row = (int)(pix / p.W), col = (int)(pix - (int64_t)row * p.W);
  const float *r = p.rays + (size_t)v * 12;
  const float u = (float)col, w = (float)row, d = p.depth[i];
  double X[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float dir = __fadd_rn(__builtin_fmaf(r[ax * 3 + 1], w, __fmul_rn(r[ax * 3 + 0], u)), r[ax * 3 + 2]);
    X[ax] = (double)__fadd_rn(r[9 + ax], __fmul_rn(dir, d));
  }
  const double z = __builtin_fma(p.A2[2], X[2], __builtin_fma(p.A2[1], X[1], __dmul_rn(p.A2[0], X[0]))) + p.A2[3];
  keys[i] = Key<double>::enc(z);
  if (z != z) atomicOr(&st->nan_seen, 1u);
}

// per-view scale and shift travel as kernel arguments (HOST values, no copy to wait for): kZoeViews views per launch
constexpr int kZoeViews = 64;

struct ZoeParams {
  const float *pred;  // [V,H,W]
  float *depth;       // [V,H,W] out
  const float *rays;  // [V,12], null: conversion only
  int H, W, v0;       // v0: first view of this launch
  int64_t end;        // one past this launch's last pixel
  double A2[4];
  double ss[kZoeViews][2];  // (scale, shift) of views v0 ...
};

__global__ void __launch_bounds__(kBlock) zoe_points_kernel(ZoeParams p, U *__restrict__ keys, State *__restrict__ st) {
#pragma clang fp contract(off)
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t i = (int64_t)p.v0 * HW + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.end) return;
  const int v = (int)(i / HW);
  // raw_disp = 1.0 / (depth_pred + 1e-16) in float32: numpy rounds the Python scalar to float32 first
  const float raw = __fdiv_rn(1.0f, __fadd_rn(p.pred[i], (float)1e-16));
  // disp = scale * raw_disp + shift, depth = 1 / (disp + 1e-16) in float64
  const double disp = __dadd_rn(__dmul_rn(p.ss[v - p.v0][0], (double)raw), p.ss[v - p.v0][1]);
  const double d = __ddiv_rn(1.0, __dadd_rn(disp, 1e-16));
  p.depth[i] = (float)d;
  if (!p.rays) return;
  const int64_t pix = i - (int64_t)v * HW;
  const int row = (int)(pix / p.W), col = (int)(pix - (int64_t)row * p.W);
  const float *r = p.rays + (size_t)v * 12;
  const float u = (float)col, w = (float)row;
  double X[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float dir = __fadd_rn(__builtin_fmaf(r[ax * 3 + 1], w, __fmul_rn(r[ax * 3 + 0], u)), r[ax * 3 + 2]);
    X[ax] = __dadd_rn((double)r[9 + ax], __dmul_rn((double)dir, d));
  }
  const double z = __builtin_fma(p.A2[2], X[2], __builtin_fma(p.A2[1], X[1], __dmul_rn(p.A2[0], X[0]))) + p.A2[3];
  keys[i] = Key<double>::enc(z);
  if (z != z) atomicOr(&st->nan_seen, 1u);
}

__global__ void init_kernel(Params p, State *__restrict__ st) {
  if (threadIdx.x != 0) return;
  radix::sel_init<kRanks>(&st->sel, p.rank);
  st->nan_seen = 0;
}

// one block, one wavefront per rank; the last pass writes depth_range (float32) and near / far (float64)
__global__ void __launch_bounds__(kRanks * 64) select_kernel(Params p, int pass, int last_pass, State *__restrict__ st,
                                                             const uint32_t *__restrict__ hist, float *__restrict__ out,
                                                             double *__restrict__ near_far) {
  radix::select_digits<double, kRanks>(pass, &st->sel, hist);
  if (threadIdx.x != 0 || pass != last_pass) return;
  double zmin = radix::rank_value<double, kRanks>(&st->sel, 0);
  double q = radix::lerp_np(radix::rank_value<double, kRanks>(&st->sel, 1), radix::rank_value<double, kRanks>(&st->sel, 2),
                            p.gamma);
  if (st->nan_seen) zmin = q = NAN;  // np.min and np.quantile return NaN when z holds one
  // Python's max(bound, x): x when x > bound (False for NaN), else the bound
  double lo = 0.8 * zmin, hi = 1.2 * q;
  lo = lo > 1e-16 ? lo : 1e-16;
  hi = hi > 2e-16 ? hi : 2e-16;
  out[0] = (float)lo;
  out[1] = (float)hi;
  if (near_far) {
    near_far[0] = lo;
    near_far[1] = hi;
  }
}

struct Layout {
  int64_t keys, hist, state, total;
};

constexpr int kPasses = (64 + radix::kDigit - 1) / radix::kDigit;

Layout layout(int64_t n) {
  Layout l;
  l.keys = 0;
  l.hist = align_up(n * (int64_t)sizeof(U), 256);
  l.state = l.hist + align_up((int64_t)kPasses * kRanks * kBins * 4, 256);
  l.total = l.state + align_up((int64_t)sizeof(State), 256);
  return l;
}

// H W >= 2: a one-pixel view is a matrix-vector product in numpy (M @ pix with one column), which BLAS orders
// differently from the matrix product the op follows
bool shape_ok(int V, int H, int W) {
  return V > 0 && H > 0 && W > 0 && (int64_t)H * W >= 2 && (int64_t)V * H * W < (1ll << 31);
}

// the three ranks of the n keys, then depth_range / near_far from the last pass
void select_passes(const Params &p, const U *keys, uint32_t *hist, State *state, float *depth_range, double *near_far,
                   hipStream_t st) {
  for (int pass = 0; pass < kPasses; ++pass) {
    uint32_t *hp = hist + (size_t)pass * kRanks * kBins;
    PGDVS_LAUNCH("nvidia_range_hist", (radix::hist_kernel<double, kRanks>), dim3(radix::hist_grid(p.n)), dim3(kBlock), 0, st,
                 keys, p.n, pass, &state->sel, hp);
    PGDVS_LAUNCH("nvidia_range_select", select_kernel, dim3(1), dim3(kRanks * 64), 0, st, p, pass, kPasses - 1, state, hp,
                 depth_range, near_far);
  }
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define NVR_SHAPE_MSG "pgdvs_nvidia_depth_range: bad shape V=%d H=%d W=%d (each > 0, H W >= 2, V H W < 2^31)"

PGDVS_API int64_t pgdvs_nvidia_depth_range_workspace_bytes(int V, int H, int W) {
  if (!shape_ok(V, H, W)) {
    set_error(NVR_SHAPE_MSG, V, H, W);
    return PGDVS_ERR_INVALID;
  }
  return layout((int64_t)V * H * W).total;
}

PGDVS_API int pgdvs_nvidia_depth_range(const float *depth, const float *rays, int V, int H, int W, const double *inv_c2w_tgt,
                                       float *depth_range, double *near_far, void *workspace, int64_t workspace_bytes,
                                       pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth && rays && inv_c2w_tgt && depth_range, "pgdvs_nvidia_depth_range: null pointer");
  PGDVS_REQUIRE(shape_ok(V, H, W), NVR_SHAPE_MSG, V, H, W);
  const int64_t n = (int64_t)V * H * W;
  const Layout l = layout(n);
  if (!workspace || workspace_bytes < l.total) {
    set_error("pgdvs_nvidia_depth_range: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)l.total);
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  Params p;
  p.depth = depth;
  p.rays = rays;
  p.H = H;
  p.W = W;
  p.n = n;
  for (int c = 0; c < 4; ++c) p.A2[c] = inv_c2w_tgt[8 + c];
  p.rank[0] = 0;
  radix::quantile_setup<double>(n, 0.9, p.rank[1], p.rank[2], p.gamma);
  char *ws = static_cast<char *>(workspace);
  U *keys = reinterpret_cast<U *>(ws + l.keys);
  uint32_t *hist = reinterpret_cast<uint32_t *>(ws + l.hist);
  State *state = reinterpret_cast<State *>(ws + l.state);
  const hipError_t e = hipMemsetAsync(hist, 0, (size_t)(l.state - l.hist), st);
  if (e != hipSuccess) {
    set_error("pgdvs_nvidia_depth_range: %s", hipGetErrorString(e));
    return PGDVS_ERR_LAUNCH;
  }
  PGDVS_LAUNCH("nvidia_range_init", init_kernel, dim3(1), dim3(64), 0, st, p, state);
  PGDVS_LAUNCH("nvidia_range_points", points_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, p, keys, state);
  select_passes(p, keys, hist, state, depth_range, near_far, st);
  return check_launch("pgdvs_nvidia_depth_range");
}

#define NVZ_SHAPE_MSG "pgdvs_nvidia_zoe_depth_range: bad shape V=%d H=%d W=%d (each > 0, V H W < 2^31; with a range, H W >= 2)"

PGDVS_API int64_t pgdvs_nvidia_zoe_depth_range_workspace_bytes(int V, int H, int W) {
  if (!shape_ok(V, H, W)) {
    set_error(NVZ_SHAPE_MSG, V, H, W);
    return PGDVS_ERR_INVALID;
  }
  return layout((int64_t)V * H * W).total;
}

PGDVS_API int pgdvs_nvidia_zoe_depth_range(const float *depth_pred, const double *scale_shift, const float *rays, int V, int H,
                                           int W, const double *inv_c2w_tgt, float *depth, float *depth_range,
                                           double *near_far, void *workspace, int64_t workspace_bytes,
                                           pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth_pred && scale_shift && depth, "pgdvs_nvidia_zoe_depth_range: null pointer");
  const bool range = rays && inv_c2w_tgt && depth_range;
  PGDVS_REQUIRE(range || (!rays && !inv_c2w_tgt && !depth_range && !near_far),
                "pgdvs_nvidia_zoe_depth_range: rays, inv_c2w_tgt and depth_range go together (near_far only with them)");
  PGDVS_REQUIRE(V > 0 && H > 0 && W > 0 && (int64_t)V * H * W < (1ll << 31) && (!range || shape_ok(V, H, W)), NVZ_SHAPE_MSG, V,
                H, W);
  const int64_t HW = (int64_t)H * W, n = (int64_t)V * HW;
  hipStream_t st = as_stream(stream);
  Params p;
  U *keys = nullptr;
  uint32_t *hist = nullptr;
  State *state = nullptr;
  ZoeParams z;
  z.pred = depth_pred;
  z.depth = depth;
  z.rays = range ? rays : nullptr;
  z.H = H;
  z.W = W;
  for (int c = 0; c < 4; ++c) z.A2[c] = range ? inv_c2w_tgt[8 + c] : 0.0;
  if (range) {
    const Layout l = layout(n);
    if (!workspace || workspace_bytes < l.total) {
      set_error("pgdvs_nvidia_zoe_depth_range: workspace too small (%lld < %lld)", (long long)workspace_bytes,
                (long long)l.total);
      return PGDVS_ERR_WORKSPACE;
    }
    p.depth = depth;
    p.rays = rays;
    p.H = H;
    p.W = W;
    p.n = n;
    for (int c = 0; c < 4; ++c) p.A2[c] = z.A2[c];
    p.rank[0] = 0;
    radix::quantile_setup<double>(n, 0.9, p.rank[1], p.rank[2], p.gamma);
    char *ws = static_cast<char *>(workspace);
    keys = reinterpret_cast<U *>(ws + l.keys);
    hist = reinterpret_cast<uint32_t *>(ws + l.hist);
    state = reinterpret_cast<State *>(ws + l.state);
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)(l.state - l.hist), st);
    if (e != hipSuccess) {
      set_error("pgdvs_nvidia_zoe_depth_range: %s", hipGetErrorString(e));
      return PGDVS_ERR_LAUNCH;
    }
    PGDVS_LAUNCH("nvidia_range_init", init_kernel, dim3(1), dim3(64), 0, st, p, state);
  }
  for (int v0 = 0; v0 < V; v0 += kZoeViews) {
    const int nv = V - v0 < kZoeViews ? V - v0 : kZoeViews;
    z.v0 = v0;
    z.end = (int64_t)(v0 + nv) * HW;
    for (int v = 0; v < kZoeViews; ++v)
      for (int c = 0; c < 2; ++c) z.ss[v][c] = v < nv ? scale_shift[(size_t)(v0 + v) * 2 + c] : 0.0;
    PGDVS_LAUNCH("nvidia_zoe_points", zoe_points_kernel, dim3((unsigned)cdiv((int64_t)nv * HW, kBlock)), dim3(kBlock), 0, st, z,
                 keys, state);
  }
  if (range) select_passes(p, keys, hist, state, depth_range, near_far, st);
  return check_launch("pgdvs_nvidia_zoe_depth_range");
}
