// the loaders' depth-range ops, each bit-identical to its loader's numpy path.  One pipeline serves them all:
// unproject the spatial pixels, take z in the target camera, radix-select a few order statistics of z, finish.
//
// points   one thread per spatial pixel (view-major, as the loaders concatenate them).  The ray direction is float32, as
//          `M @ pix` reaches BLAS: d = fma(M[:,1], v, M[:,0] u) + M[:,2] (fused, k ascending).  X = o + d depth and
//          z = row 2 of inv(c2w_tgt) @ [X,1] (BLAS order again) follow in the op's type; z's order-preserving key goes to the
//          workspace, and a NaN raises a flag, since np.min and np.quantile return NaN when z holds one.
// select   the ranks the op needs, found exactly and together by the shared radix select (radix_select.h: 3 passes for
//          float keys, 6 for double).  The last select pass interpolates with numpy's _lerp and finishes the op.
//
// DyCheck (pgdvs/datasets/dycheck_iphone_eval.py:455-524; pgdvs_amd/datasets/dycheck_iphone.py depth_range_numpy), per
// pixel.  T is the points' type: float for float32 depth (the iPhone files; then upstream's arithmetic is float32 end to
// end, and np.quantile keeps float32), double for float64 depth (numpy promotes every step after the rays to float64).
// X = o + d depth in T, z against inv(raw_c2w_tgt).  Static points (dyn_mask == 0) are also moved by inv(c2w_tgt) and
// projected in T the same way, divided by (z + 1e-8), kept when 0 <= col <= W-1 and 0 <= row <= H-1 (no z > 0 test, as
// upstream), truncated, and the pixel keeps the largest flat index (numpy's fancy assignment: the last point wins) through
// atomicMax.  Four ranks: the neighbours of np.quantile(z, q, method="linear") for q = 0.1, 0.9; the finish clamps with
// near / far as Python's max / min compare.  write: one thread per target pixel, the winning point's z -+ 1e-4 in T, or
// the constant range when no point hit it.
//
// NVIDIA family (nvidia_eval.py:446-456, nvidia_vis.py:405-417, mono_vis.py; pgdvs_amd/datasets/nvidia_eval.py compute_pcl
// + depth_range_from_points), per item: near = max(1e-16, 0.8 min z), far = max(2e-16, 1.2 np.quantile(z, 0.9)).
// X = o + d depth as a float32 multiply and add, widened; z in float64.  Three ranks: 0 (np.min) and the neighbours of
// the virtual index (n - 1) 0.9; the finish scales, clamps as Python's max compares and writes both outputs.
//
// ZoeDepth (nvidia_eval.py:869-945): pgdvs_nvidia_zoe_depth_range puts the loader's alignment of a monocular prediction in
// front of the NVIDIA select.  zoe_points turns each prediction into the aligned depth (float32 reciprocal, then scale,
// shift and reciprocal in float64, every operation rounded on its own, as NumPy 2 promotes upstream's three lines), stores
// its float32 rounding and, on the range path, unprojects with the float64 depth still in registers: X = o + d depth in
// float64, as upstream's float32 torch rays times a float64 numpy depth give.  Without the range arguments it is the
// conversion alone (temporal and tracker views): one launch per kZoeViews views, no workspace.
// pgdvs_item_zoe_depths is the same alignment over the resident store's prediction table (datasets/resident.py): item_zoe
// gathers every view of an item by frame id, one launch with grid.y = the view and the per-view scale and shift as kernel
// arguments, writes the float32 depths of all groups and, for the views of the spatial group, the keys of the select.
// Both kernels call ONE device function for upstream's three lines (zoe_aligned_depth), so they cannot drift.
//
// Rounding: the library is built with -ffp-contract=off -fno-fast-math, so a plain * + / rounds once, exactly as the
// __f*_rn / __d*_rn intrinsics would.  This file writes plain operators throughout and spells out only the fused steps.
#include <cmath>

#include "common.h"
#include "radix_select.h"

namespace pgdvs {
namespace {

using radix::Key;
using radix::kBins;
using radix::kBlock;

__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- one spatial pixel: decode, ray direction, world point, target z, key ----

struct Pixel {
  int v;       // view
  float u, w;  // column, row
};

__device__ __forceinline__ Pixel decode(int64_t i, int H, int W) {
  const int64_t HW = (int64_t)H * W;
  const int v = (int)(i / HW);
  const int64_t pix = i - (int64_t)v * HW;
  const int row = (int)(pix / W), col = (int)(pix - (int64_t)row * W);
  return {v, (float)col, (float)row};
}

// X = o + dir depth in T, dir in float32; rays [V,12]: M (3x3 row-major), o.  The flavours differ in T alone: DyCheck's
// points' type, float for NVIDIA (the caller widens X), double for ZoeDepth.
template <typename T> __device__ __forceinline__ void world_point(const float *rays, const Pixel &px, T depth, T X[3]) {
  const float *r = rays + (size_t)px.v * 12;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float dir = __builtin_fmaf(r[ax * 3 + 1], px.w, r[ax * 3 + 0] * px.u) + r[ax * 3 + 2];
    X[ax] = (T)r[9 + ax] + (T)dir * depth;
  }
}

// A2 . [X,1], A2 = row 2 of the target's inverse pose
template <typename T> __device__ __forceinline__ T target_z(const T A2[4], const T X[3]) {
  return fmaT(A2[2], X[2], fmaT(A2[1], X[1], A2[0] * X[0])) + A2[3];
}

template <typename T>
__device__ __forceinline__ void store_key(T z, typename Key<T>::U *__restrict__ keys, int64_t i, uint32_t *nan_seen) {
  keys[i] = Key<T>::enc(z);
  if (z != z) atomicOr(nan_seen, 1u);
}

// ---- select state, workspace and the pass loop ----

template <int NR> struct State {
  static constexpr int kRanks = NR;
  radix::Sel<NR> sel;
  uint32_t nan_seen;
};

struct DyState : State<4> {
  float lo32, hi32;
  double q[2];
};

template <int NR> struct Ranks {
  int64_t rank[NR];
};

template <int NR> __global__ void init_kernel(Ranks<NR> ranks, State<NR> *__restrict__ st) {
  if (threadIdx.x != 0) return;
  radix::sel_init<NR>(&st->sel, ranks.rank);
  st->nan_seen = 0;
}

struct Labels {
  const char *init, *hist, *select;
};
constexpr Labels kDyLabels = {"dycheck_range_init", "dycheck_range_hist", "dycheck_range_select"};
constexpr Labels kNvLabels = {"nvidia_range_init", "nvidia_range_hist", "nvidia_range_select"};

// keys at 0, then the per-pixel plane (DyCheck's int32 `last`; absent when per_pixel_bytes == 0), histograms, state
struct Layout {
  int64_t per_pixel, hist, state, total;
};

static_assert(sizeof(DyState) <= 256 && sizeof(State<3>) <= 256, "the state takes one 256-byte slot");

Layout layout(int64_t n, int key_bytes, int passes, int NR, int64_t per_pixel_bytes) {
  Layout l;
  l.per_pixel = align_up(n * key_bytes, 256);
  l.hist = l.per_pixel + align_up(per_pixel_bytes, 256);
  l.state = l.hist + align_up((int64_t)passes * NR * kBins * 4, 256);
  l.total = l.state + 256;
  return l;
}

template <typename T, typename S> struct Work {
  typename Key<T>::U *keys;
  int32_t *last;  // per-pixel plane, set to -1
  uint32_t *hist;
  S *state;
};

// checks the workspace, carves it, clears the histograms (and `last`) and starts the select at `ranks`
template <typename T, typename S>
int setup(const char *op, const Labels &lb, int64_t n, int64_t per_pixel_bytes, const Ranks<S::kRanks> &ranks, void *workspace,
          int64_t workspace_bytes, hipStream_t st, Work<T, S> &w) {
  const Layout l = layout(n, (int)sizeof(typename Key<T>::U), radix::passes_for(Key<T>::kBits), S::kRanks, per_pixel_bytes);
  if (!workspace || workspace_bytes < l.total) {
    set_error("%s: workspace too small (%lld < %lld)", op, (long long)workspace_bytes, (long long)l.total);
    return PGDVS_ERR_WORKSPACE;
  }
  char *ws = static_cast<char *>(workspace);
  w.keys = reinterpret_cast<typename Key<T>::U *>(ws);
  w.last = reinterpret_cast<int32_t *>(ws + l.per_pixel);
  w.hist = reinterpret_cast<uint32_t *>(ws + l.hist);
  w.state = reinterpret_cast<S *>(ws + l.state);
  hipError_t e = per_pixel_bytes ? hipMemsetAsync(w.last, 0xff, (size_t)per_pixel_bytes, st) : hipSuccess;
  if (e == hipSuccess) e = hipMemsetAsync(w.hist, 0, (size_t)(l.state - l.hist), st);
  if (e != hipSuccess) {
    set_error("%s: %s", op, hipGetErrorString(e));
    return PGDVS_ERR_LAUNCH;
  }
  PGDVS_LAUNCH(lb.init, init_kernel<S::kRanks>, dim3(1), dim3(64), 0, st, ranks, w.state);
  return PGDVS_OK;
}

// one block, one wavefront per rank: pick this pass's digit of every rank; the last pass finishes the op
template <typename T, typename Fin>
__global__ void __launch_bounds__(Fin::State::kRanks * 64) select_kernel(Fin fin, int pass, int last_pass,
                                                                         typename Fin::State *__restrict__ st,
                                                                         const uint32_t *__restrict__ hist) {
  radix::select_digits<T, Fin::State::kRanks>(pass, &st->sel, hist);
  if (threadIdx.x == 0 && pass == last_pass) fin(st);
}

template <typename T, int NR, typename Fin>
void select_passes(const Labels &lb, const Work<T, typename Fin::State> &w, int64_t n, const Fin &fin, hipStream_t st) {
  const int passes = radix::passes_for(Key<T>::kBits);
  const unsigned hgrid = radix::hist_grid(n);
  for (int pass = 0; pass < passes; ++pass) {
    uint32_t *hp = w.hist + (size_t)pass * NR * kBins;
    PGDVS_LAUNCH(lb.hist, (radix::hist_kernel<T, NR>), dim3(hgrid), dim3(kBlock), 0, st, w.keys, n, pass, &w.state->sel, hp);
    PGDVS_LAUNCH(lb.select, (select_kernel<T, Fin>), dim3(1), dim3(NR * 64), 0, st, fin, pass, passes - 1, w.state, hp);
  }
}

// ---- DyCheck ----

template <typename T> struct DyParams {
  const void *depth;      // [V,H,W] T
  const float *dyn_mask;  // [V,H,W], static where == 0
  const float *rays;      // [V,12]
  int H, W;
  int64_t n;              // V H W
  T A2[4];                // row 2 of inv(raw_c2w_tgt)
  T B[12];                // rows 0..2 of inv(c2w_tgt)
  T K[9];                 // K_tgt[:3,:3]
};

template <typename T> __device__ __forceinline__ void unproject(const DyParams<T> &p, int64_t i, T X[3]) {
  world_point<T>(p.rays, decode(i, p.H, p.W), static_cast<const T *>(p.depth)[i], X);
}

// static point -> (camera z, projected column / row) in T, numpy's matmul order
template <typename T>
__device__ __forceinline__ void project_static(const DyParams<T> &p, const T X[3], T &z, T &col, T &row) {
  T c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = fmaT(p.B[r * 4 + 2], X[2], fmaT(p.B[r * 4 + 1], X[1], p.B[r * 4 + 0] * X[0])) + p.B[r * 4 + 3];
  T q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = fmaT(p.K[r * 3 + 2], c[2], fmaT(p.K[r * 3 + 1], c[1], p.K[r * 3 + 0] * c[0]));
  const T den = q[2] + (T)1e-8;
  z = c[2];
  col = q[0] / den;
  row = q[1] / den;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) dy_points_kernel(DyParams<T> p, typename Key<T>::U *__restrict__ keys,
                                                           int32_t *__restrict__ last, DyState *__restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  T X[3];
  unproject(p, i, X);
  store_key<T>(target_z<T>(p.A2, X), keys, i, &st->nan_seen);
  if (p.dyn_mask[i] == 0.0f) {
    T zc, col, row;
    project_static(p, X, zc, col, row);
    if (row >= (T)0 && row <= (T)(p.H - 1) && col >= (T)0 && col <= (T)(p.W - 1))
      atomicMax(&last[(int64_t)(int)row * p.W + (int)col], (int32_t)i);  // i < 2^31 (checked on entry)
  }
}

// the two clamped quantiles; set up on the host with numpy's float semantics of T
template <typename T> struct DyFinish {
  typedef DyState State;
  T gamma[2];  // weight of q = 0.1 and q = 0.9 between their two ranks
  T near_t, far_t;
  float near32, far32;
  __device__ void operator()(DyState *st) const {
    T q[2];
    for (int j = 0; j < 2; ++j)
      q[j] = radix::lerp_np(radix::rank_value<T, 4>(&st->sel, 2 * j), radix::rank_value<T, 4>(&st->sel, 2 * j + 1), gamma[j]);
    if (st->nan_seen) q[0] = q[1] = (T)NAN;
    // Python's max(near, q) / min(far, q): q when q > near (resp. q < far), compared in T; else the bound
    st->lo32 = q[0] > near_t ? (float)q[0] : near32;
    st->hi32 = q[1] < far_t ? (float)q[1] : far32;
    st->q[0] = (double)q[0];
    st->q[1] = (double)q[1];
  }
};

template <typename T>
__global__ void __launch_bounds__(kBlock) dy_write_kernel(DyParams<T> p, const int32_t *__restrict__ last,
                                                          const DyState *__restrict__ st, float *__restrict__ out) {
  const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (pix >= (int64_t)p.H * p.W) return;
  const int32_t j = last[pix];
  float lo = st->lo32, hi = st->hi32;
  if (j >= 0) {
    T X[3], z, col, row;
    unproject(p, (int64_t)j, X);
    project_static(p, X, z, col, row);
    lo = (float)(z - (T)1e-4);
    hi = (float)(z + (T)1e-4);
  }
  out[pix * 2 + 0] = lo;
  out[pix * 2 + 1] = hi;
}

bool dy_shape_ok(int V, int H, int W) {
  return V > 0 && H > 0 && W > 0 && (int64_t)V * H * W < (1ll << 31);
}

template <typename T>
int dy_run(const void *depth, const float *dyn_mask, const float *rays, int V, int H, int W, const double *inv_raw_c2w_tgt,
           const double *inv_c2w_tgt, const double *K_tgt, double near_v, double far_v, float *out, double *quantiles,
           void *workspace, int64_t workspace_bytes, hipStream_t st) {
  const char *op = "pgdvs_dycheck_depth_range";
  const int64_t n = (int64_t)V * H * W, hw = (int64_t)H * W;
  Ranks<4> ranks;
  DyFinish<T> fin;
  radix::quantile_setup<T>(n, (T)0.1, ranks.rank[0], ranks.rank[1], fin.gamma[0]);
  radix::quantile_setup<T>(n, (T)0.9, ranks.rank[2], ranks.rank[3], fin.gamma[1]);
  fin.near_t = (T)near_v;
  fin.far_t = (T)far_v;
  fin.near32 = (float)near_v;
  fin.far32 = (float)far_v;
  Work<T, DyState> w;
  if (const int rc = setup<T>(op, kDyLabels, n, hw * 4, ranks, workspace, workspace_bytes, st, w)) return rc;
  DyParams<T> p = {depth, dyn_mask, rays, H, W, n};
  for (int c = 0; c < 4; ++c) p.A2[c] = (T)inv_raw_c2w_tgt[8 + c];
  for (int k = 0; k < 12; ++k) p.B[k] = (T)inv_c2w_tgt[k];
  for (int k = 0; k < 9; ++k) p.K[k] = (T)K_tgt[k];
  PGDVS_LAUNCH("dycheck_range_points", dy_points_kernel<T>, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, p, w.keys, w.last,
               w.state);
  select_passes<T, 4>(kDyLabels, w, n, fin, st);
  PGDVS_LAUNCH("dycheck_range_write", dy_write_kernel<T>, dim3((unsigned)cdiv(hw, kBlock)), dim3(kBlock), 0, st, p, w.last, w.state,
               out);
  if (quantiles) {
    const hipError_t e = hipMemcpyAsync(quantiles, &w.state->q[0], 2 * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      set_error("%s: %s", op, hipGetErrorString(e));
      return PGDVS_ERR_LAUNCH;
    }
  }
  return check_launch(op);
}

// ---- NVIDIA family and ZoeDepth ----

typedef Key<double>::U U64;
typedef State<3> NvState;  // ranks: min, quantile floor, quantile floor + 1

struct NvParams {
  const float *depth;  // [V,H,W]
  const float *rays;   // [V,12]
  int H, W;
  int64_t n;           // V H W
  double A2[4];        // row 2 of inv(c2w_tgt)
};

__global__ void __launch_bounds__(kBlock) nv_points_kernel(NvParams p, U64 *__restrict__ keys, NvState *__restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  float X32[3];
  world_point<float>(p.rays, decode(i, p.H, p.W), p.depth[i], X32);
  const double X[3] = {(double)X32[0], (double)X32[1], (double)X32[2]};
  store_key<double>(target_z<double>(p.A2, X), keys, i, &st->nan_seen);
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

// upstream's three lines on one prediction: the ONE statement of the alignment, for the stacked predictions
// (zoe_points_kernel) and for the resident store's (item_zoe_kernel)
__device__ __forceinline__ double zoe_aligned_depth(float pred, double scale, double shift) {
  // raw_disp = 1.0 / (depth_pred + 1e-16) in float32: numpy rounds the Python scalar to float32 first
  const float raw = 1.0f / (pred + (float)1e-16);
  // disp = scale * raw_disp + shift, depth = 1 / (disp + 1e-16) in float64
  const double disp = scale * (double)raw + shift;
  return 1.0 / (disp + 1e-16);
}

// the aligned float64 depth of pixel px, still in registers -> the key of its target-camera z
__device__ __forceinline__ U64 zoe_key(const float *rays, const double A2[4], const Pixel &px, double d, uint32_t *nan_seen) {
  double X[3];
  world_point<double>(rays, px, d, X);
  const double z = target_z<double>(A2, X);
  if (z != z) atomicOr(nan_seen, 1u);
  return Key<double>::enc(z);
}

__global__ void __launch_bounds__(kBlock) zoe_points_kernel(ZoeParams p, U64 *__restrict__ keys, NvState *__restrict__ st) {
  const int64_t i = (int64_t)p.v0 * p.H * p.W + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.end) return;
  const Pixel px = decode(i, p.H, p.W);
  const double d = zoe_aligned_depth(p.pred[i], p.ss[px.v - p.v0][0], p.ss[px.v - p.v0][1]);
  p.depth[i] = (float)d;
  if (!p.rays) return;
  keys[i] = zoe_key(p.rays, p.A2, px, d, &st->nan_seen);
}

// The resident store's ZoeDepth gather (datasets/resident.py, a scene in prediction mode): the slots hold the predictions, the
// per-view scale and shift travel as kernel arguments like the frame ids, and the item's aligned depths are written group by
// group in one launch, grid.y = the view.  A lane takes four pixels: 16 bytes of prediction in, 16 bytes of depth out where
// the view's output base is 16-byte aligned (uniform per view; H W % 4 == 0 guarantees it behind an aligned tensor), else
// the scalar statement for the whole view; the scalar statement also finishes the H W % 4 pixels behind the quads.  The
// first n_range views (group 0, the spatial one) also unproject the float64 depth and store the key of view-major pixel
// v H W + i, 32 bytes per lane in two 16-byte stores where v H W is even.  One fp64 divide, one fp32 divide and, on range
// views, 12 fp64 multiply-adds per pixel: far below the rate the 4 + 4 (+ 8) bytes per pixel stream at.
struct ItemZoeParams {
  const float *pred;   // the store: frame f at + f * slot bytes
  int64_t slot, n;     // n = H W
  int W, n_groups, n_range;
  const float *rays;   // [n_range,12]; unused when n_range == 0
  double A2[4];
  float *out[PGDVS_ITEM_MAX_GROUPS];  // [n,H,W] per group
  int first[PGDVS_ITEM_MAX_GROUPS];   // the group's first view in ids
  int ids[PGDVS_ITEM_MAX_VIEWS];
  double ss[PGDVS_ITEM_MAX_VIEWS][2];
};

__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ void __launch_bounds__(kBlock) item_zoe_kernel(ItemZoeParams p, U64 *__restrict__ keys, NvState *__restrict__ st) {
  const int v = blockIdx.y;
  int g = 0;
#pragma unroll
  for (int k = 1; k < PGDVS_ITEM_MAX_GROUPS; ++k)
    if (k < p.n_groups && v >= p.first[k]) g = k;
  const float *__restrict__ src = reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.pred) + (int64_t)p.ids[v] * p.slot);
  float *__restrict__ out = p.out[g] + (int64_t)(v - p.first[g]) * p.n;
  const double scale = p.ss[v][0], shift = p.ss[v][1];
  const bool range = v < p.n_range;
  U64 *__restrict__ kv = range ? keys + (int64_t)v * p.n : nullptr;

  const int64_t quads = aligned16(out) ? p.n >> 2 : 0;
  const bool kvec = aligned16(kv);
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;

  for (int64_t q = t; q < quads; q += stride) {  // (the grid covers the quads: one trip)
    const float4 x = reinterpret_cast<const float4 *>(src)[q];
    const double d[4] = {zoe_aligned_depth(x.x, scale, shift), zoe_aligned_depth(x.y, scale, shift),
                         zoe_aligned_depth(x.z, scale, shift), zoe_aligned_depth(x.w, scale, shift)};
    reinterpret_cast<float4 *>(out)[q] = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
    if (range) {
      int row = (int)((q << 2) / p.W), col = (int)((q << 2) - (int64_t)row * p.W);
      U64 k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = zoe_key(p.rays, p.A2, Pixel{v, (float)col, (float)row}, d[j], &st->nan_seen);
        if (++col == p.W) {
          col = 0;
          ++row;
        }
      }
      if (kvec) {
        ulonglong2 *k2 = reinterpret_cast<ulonglong2 *>(kv + (q << 2));
        k2[0] = make_ulonglong2(k[0], k[1]);
        k2[1] = make_ulonglong2(k[2], k[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) kv[(q << 2) + j] = k[j];
      }
    }
  }

  for (int64_t i = (quads << 2) + t; i < p.n; i += stride) {  // the scalar statement: the tail, or a whole unaligned view
    const double d = zoe_aligned_depth(src[i], scale, shift);
    out[i] = (float)d;
    if (range) {
      const int row = (int)(i / p.W), col = (int)(i - (int64_t)row * p.W);
      kv[i] = zoe_key(p.rays, p.A2, Pixel{v, (float)col, (float)row}, d, &st->nan_seen);
    }
  }
}

// the scaled min and quantile: depth_range (float32) and near / far (float64)
struct NvFinish {
  typedef NvState State;
  double gamma;
  float *out;
  double *near_far;  // nullable
  __device__ void operator()(NvState *st) const {
    double zmin = radix::rank_value<double, 3>(&st->sel, 0);
    double q = radix::lerp_np(radix::rank_value<double, 3>(&st->sel, 1), radix::rank_value<double, 3>(&st->sel, 2), gamma);
    if (st->nan_seen) zmin = q = NAN;
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
};

// H W >= 2: a one-pixel view is a matrix-vector product in numpy (M @ pix with one column), which BLAS orders
// differently from the matrix product the op follows
bool nv_shape_ok(int V, int H, int W) {
  return dy_shape_ok(V, H, W) && (int64_t)H * W >= 2;
}

int64_t nv_workspace_bytes(int V, int H, int W) {
  return layout((int64_t)V * H * W, 8, radix::passes_for(64), 3, 0).total;
}

// set-up of both NVIDIA range paths: rank 0 and the neighbours of np.quantile(z, 0.9)
int nv_setup(const char *op, int64_t n, float *depth_range, double *near_far, void *workspace, int64_t workspace_bytes,
             hipStream_t st, Work<double, NvState> &w, NvFinish &fin) {
  Ranks<3> ranks;
  ranks.rank[0] = 0;
  radix::quantile_setup<double>(n, 0.9, ranks.rank[1], ranks.rank[2], fin.gamma);
  fin.out = depth_range;
  fin.near_far = near_far;
  return setup<double>(op, kNvLabels, n, 0, ranks, workspace, workspace_bytes, st, w);
}

// ---- np.percentile of float32 values (mono_vis' near depths under device_depth) ----

typedef State<2> PctState;  // ranks: the virtual index's floor and floor + 1
constexpr Labels kPctLabels = {"percentile_init", "percentile_hist", "percentile_select"};

__global__ void __launch_bounds__(kBlock) pct_keys_kernel(const float *__restrict__ values, int64_t n, Key<float>::U *__restrict__ keys,
                                                          PctState *__restrict__ st) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) store_key<float>(values[i], keys, i, &st->nan_seen);
}

struct PctFinish {
  typedef PctState State;
  float gamma;
  float *out;
  __device__ void operator()(PctState *st) const {
    const float q = radix::lerp_np(radix::rank_value<float, 2>(&st->sel, 0), radix::rank_value<float, 2>(&st->sel, 1), gamma);
    *out = st->nan_seen ? NAN : q;
  }
};

int64_t pct_frame_bytes(int64_t n) { return layout(n, 4, radix::passes_for(32), 2, 0).total; }

bool pct_counts_ok(const int64_t *counts, int32_t nframes) {
  if (!counts || nframes < 1) return false;
  for (int32_t f = 0; f < nframes; ++f)
    if (counts[f] < 1 || counts[f] >= (1ll << 31)) return false;
  return true;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define PCT_COUNTS_MSG "%s: at least one frame, each of 1 .. 2^31 - 1 values"

PGDVS_API int64_t pgdvs_percentile_f32_workspace_bytes(const int64_t *counts, int32_t nframes) {
  if (!pct_counts_ok(counts, nframes)) {
    set_error(PCT_COUNTS_MSG, "pgdvs_percentile_f32_workspace_bytes");
    return PGDVS_ERR_INVALID;
  }
  int64_t total = 0;
  for (int32_t f = 0; f < nframes; ++f) total += pct_frame_bytes(counts[f]);
  return total;
}

PGDVS_API int pgdvs_percentile_f32(const float *const *values, const int64_t *counts, int32_t nframes, double q_percent, float *out, void *workspace,
                                   int64_t workspace_bytes, pgdvs_stream_t stream) {
  const char *op = "pgdvs_percentile_f32";
  PGDVS_REQUIRE(values && out && workspace, "%s: null pointer", op);
  PGDVS_REQUIRE(pct_counts_ok(counts, nframes), PCT_COUNTS_MSG, op);
  PGDVS_REQUIRE(q_percent >= 0.0 && q_percent <= 100.0, "%s: q = %g percent (0 .. 100)", op, q_percent);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "%s: the workspace must be 256-byte aligned, out 4-byte", op);
  const float q = (float)q_percent / 100.0f;  // np.true_divide(q, float32(100)): the weak Python scalar becomes float32
  hipStream_t st = as_stream(stream);
  int64_t at = 0;
  for (int32_t f = 0; f < nframes; ++f) {
    PGDVS_REQUIRE(values[f] && (reinterpret_cast<uintptr_t>(values[f]) & 3) == 0, "%s: frame %d's values are NULL or not 4-byte aligned", op, f);
    const int64_t n = counts[f];
    Ranks<2> ranks;
    PctFinish fin;
    radix::quantile_setup<float>(n, q, ranks.rank[0], ranks.rank[1], fin.gamma);
    fin.out = out + f;
    Work<float, PctState> w;
    if (const int rc = setup<float>(op, kPctLabels, n, 0, ranks, static_cast<char *>(workspace) + at, workspace_bytes - at, st, w)) return rc;
    at += pct_frame_bytes(n);
    PGDVS_LAUNCH("percentile_keys", pct_keys_kernel, dim3(radix::hist_grid(n)), dim3(kBlock), 0, st, values[f], n, w.keys, w.state);
    select_passes<float, 2>(kPctLabels, w, n, fin, st);
  }
  return check_launch(op);
}

#define DYR_SHAPE_MSG "pgdvs_dycheck_depth_range: bad shape V=%d H=%d W=%d (each > 0, V H W < 2^31)"

PGDVS_API int64_t pgdvs_dycheck_depth_range_workspace_bytes(int V, int H, int W, int depth_f64) {
  if (!dy_shape_ok(V, H, W)) {
    set_error(DYR_SHAPE_MSG, V, H, W);
    return PGDVS_ERR_INVALID;
  }
  const int kbits = depth_f64 ? 64 : 32;
  return layout((int64_t)V * H * W, kbits / 8, radix::passes_for(kbits), 4, (int64_t)H * W * 4).total;
}

PGDVS_API int pgdvs_dycheck_depth_range(const void *depth, int depth_f64, const float *dyn_mask, const float *rays, int V, int H,
                                        int W, const double *inv_raw_c2w_tgt, const double *inv_c2w_tgt, const double *K_tgt,
                                        double near_v, double far_v, float *depth_range, double *quantiles, void *workspace,
                                        int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth && dyn_mask && rays && inv_raw_c2w_tgt && inv_c2w_tgt && K_tgt && depth_range,
                "pgdvs_dycheck_depth_range: null pointer");
  PGDVS_REQUIRE(dy_shape_ok(V, H, W), DYR_SHAPE_MSG, V, H, W);
  // upstream's matrices are float32 (DyCheckCamera's extrinsics and flat_cam); numpy promotes them to the points' type
  const double *mats[3] = {inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt};
  const int counts[3] = {16, 16, 9};
  for (int m = 0; m < 3; ++m)
    for (int k = 0; k < counts[m]; ++k)
      PGDVS_REQUIRE((double)(float)mats[m][k] == mats[m][k] || mats[m][k] != mats[m][k],
                    "pgdvs_dycheck_depth_range: matrix %d entry %d is not a float32 value", m, k);
  return (depth_f64 ? dy_run<double> : dy_run<float>)(depth, dyn_mask, rays, V, H, W, inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt, near_v,
                                                      far_v, depth_range, quantiles, workspace, workspace_bytes,
                                                      as_stream(stream));
}

#define NVR_SHAPE_MSG "pgdvs_nvidia_depth_range: bad shape V=%d H=%d W=%d (each > 0, H W >= 2, V H W < 2^31)"

PGDVS_API int64_t pgdvs_nvidia_depth_range_workspace_bytes(int V, int H, int W) {
  if (!nv_shape_ok(V, H, W)) {
    set_error(NVR_SHAPE_MSG, V, H, W);
    return PGDVS_ERR_INVALID;
  }
  return nv_workspace_bytes(V, H, W);
}

PGDVS_API int pgdvs_nvidia_depth_range(const float *depth, const float *rays, int V, int H, int W, const double *inv_c2w_tgt,
                                       float *depth_range, double *near_far, void *workspace, int64_t workspace_bytes,
                                       pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth && rays && inv_c2w_tgt && depth_range, "pgdvs_nvidia_depth_range: null pointer");
  PGDVS_REQUIRE(nv_shape_ok(V, H, W), NVR_SHAPE_MSG, V, H, W);
  const int64_t n = (int64_t)V * H * W;
  hipStream_t st = as_stream(stream);
  Work<double, NvState> w;
  NvFinish fin;
  if (const int rc = nv_setup("pgdvs_nvidia_depth_range", n, depth_range, near_far, workspace, workspace_bytes, st, w, fin)) return rc;
  NvParams p = {depth, rays, H, W, n};
  for (int c = 0; c < 4; ++c) p.A2[c] = inv_c2w_tgt[8 + c];
  PGDVS_LAUNCH("nvidia_range_points", nv_points_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, p, w.keys, w.state);
  select_passes<double, 3>(kNvLabels, w, n, fin, st);
  return check_launch("pgdvs_nvidia_depth_range");
}

#define NVZ_SHAPE_MSG "pgdvs_nvidia_zoe_depth_range: bad shape V=%d H=%d W=%d (each > 0, V H W < 2^31; with a range, H W >= 2)"

PGDVS_API int64_t pgdvs_nvidia_zoe_depth_range_workspace_bytes(int V, int H, int W) {
  if (!nv_shape_ok(V, H, W)) {
    set_error(NVZ_SHAPE_MSG, V, H, W);
    return PGDVS_ERR_INVALID;
  }
  return nv_workspace_bytes(V, H, W);
}

PGDVS_API int pgdvs_nvidia_zoe_depth_range(const float *depth_pred, const double *scale_shift, const float *rays, int V, int H,
                                           int W, const double *inv_c2w_tgt, float *depth, float *depth_range,
                                           double *near_far, void *workspace, int64_t workspace_bytes,
                                           pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth_pred && scale_shift && depth, "pgdvs_nvidia_zoe_depth_range: null pointer");
  const bool range = rays && inv_c2w_tgt && depth_range;
  PGDVS_REQUIRE(range || (!rays && !inv_c2w_tgt && !depth_range && !near_far),
                "pgdvs_nvidia_zoe_depth_range: rays, inv_c2w_tgt and depth_range go together (near_far only with them)");
  PGDVS_REQUIRE(dy_shape_ok(V, H, W) && (!range || nv_shape_ok(V, H, W)), NVZ_SHAPE_MSG, V, H, W);
  const int64_t HW = (int64_t)H * W, n = (int64_t)V * HW;
  hipStream_t st = as_stream(stream);
  Work<double, NvState> w = {};  // no keys and no state without a range
  NvFinish fin;
  if (range)
    if (const int rc = nv_setup("pgdvs_nvidia_zoe_depth_range", n, depth_range, near_far, workspace, workspace_bytes, st, w, fin))
      return rc;
  ZoeParams z = {depth_pred, depth, range ? rays : nullptr, H, W};
  for (int c = 0; c < 4; ++c) z.A2[c] = range ? inv_c2w_tgt[8 + c] : 0.0;
  for (int v0 = 0; v0 < V; v0 += kZoeViews) {
    const int nv = V - v0 < kZoeViews ? V - v0 : kZoeViews;
    z.v0 = v0;
    z.end = (int64_t)(v0 + nv) * HW;
    for (int v = 0; v < kZoeViews; ++v)
      for (int c = 0; c < 2; ++c) z.ss[v][c] = v < nv ? scale_shift[(size_t)(v0 + v) * 2 + c] : 0.0;
    PGDVS_LAUNCH("nvidia_zoe_points", zoe_points_kernel, dim3((unsigned)cdiv((int64_t)nv * HW, kBlock)), dim3(kBlock), 0, st, z,
                 w.keys, w.state);
  }
  if (range) select_passes<double, 3>(kNvLabels, w, n, fin, st);
  return check_launch("pgdvs_nvidia_zoe_depth_range");
}

#define IZD_SHAPE_MSG "pgdvs_item_zoe_depths: bad shape F=%d H=%d W=%d (F, H, W >= 1, H, W < 2^20, H W < 2^31)"

namespace pgdvs {
namespace {
bool item_shape_ok(int H, int W) { return H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (1ll << 31); }
}  // namespace
}  // namespace pgdvs

PGDVS_API int64_t pgdvs_item_zoe_depths_workspace_bytes(int n_range, int H, int W) {
  if (!item_shape_ok(H, W) || n_range < 1 || n_range > PGDVS_ITEM_MAX_VIEWS || !nv_shape_ok(n_range, H, W)) {
    set_error("pgdvs_item_zoe_depths_workspace_bytes: bad shape n_range=%d H=%d W=%d (1 <= n_range <= %d, H, W >= 1, each < 2^20, "
              "H W >= 2, n_range H W < 2^31)", n_range, H, W, PGDVS_ITEM_MAX_VIEWS);
    return PGDVS_ERR_INVALID;
  }
  return nv_workspace_bytes(n_range, H, W);
}

PGDVS_API int pgdvs_item_zoe_depths(const float *pred, int F, int H, int W, int64_t pred_slot, const int32_t *ids, int n_views,
                                    const double *scale_shift, const int32_t *group_sizes, int n_groups, float *const *out,
                                    const float *rays, const double *inv_c2w_tgt, float *depth_range, double *near_far,
                                    void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  const char *op = "pgdvs_item_zoe_depths";
  PGDVS_REQUIRE(item_shape_ok(H, W) && F >= 1, IZD_SHAPE_MSG, F, H, W);
  PGDVS_REQUIRE(pred && ids && scale_shift && group_sizes && out, "%s: null pointer", op);
  PGDVS_REQUIRE(n_views >= 1 && n_views <= PGDVS_ITEM_MAX_VIEWS && n_groups >= 1 && n_groups <= PGDVS_ITEM_MAX_GROUPS,
                "%s: %d views in %d groups (1 <= views <= %d, 1 <= groups <= %d)", op, n_views, n_groups, PGDVS_ITEM_MAX_VIEWS,
                PGDVS_ITEM_MAX_GROUPS);
  const bool range = rays && inv_c2w_tgt && depth_range;
  PGDVS_REQUIRE(range || (!rays && !inv_c2w_tgt && !depth_range && !near_far),
                "%s: rays, inv_c2w_tgt and depth_range go together (near_far only with them)", op);
  const int64_t n = (int64_t)H * W;
  PGDVS_REQUIRE(aligned16(pred) && pred_slot % 16 == 0 && pred_slot >= n * 4,
                "%s: the table at %p with slots of %lld bytes (both multiples of 16, a slot at least one frame of %lld pixels)", op,
                (const void *)pred, (long long)pred_slot, (long long)n);
  ItemZoeParams p;
  p.pred = pred;
  p.slot = pred_slot;
  p.n = n;
  p.W = W;
  p.n_groups = n_groups;
  int first = 0;
  for (int g = 0; g < PGDVS_ITEM_MAX_GROUPS; ++g) {
    p.out[g] = nullptr;
    p.first[g] = n_views;
    if (g >= n_groups) continue;
    PGDVS_REQUIRE(group_sizes[g] >= 1 && group_sizes[g] <= n_views - first, "%s: group %d has %d views (of %d left)", op, g,
                  group_sizes[g], n_views - first);
    PGDVS_REQUIRE(out[g] && (reinterpret_cast<uintptr_t>(out[g]) & 3) == 0, "%s: group %d's output is NULL or not 4-byte aligned", op, g);
    p.out[g] = out[g];
    p.first[g] = first;
    first += group_sizes[g];
  }
  PGDVS_REQUIRE(first == n_views, "%s: the groups hold %d views, ids %d", op, first, n_views);
  for (int v = 0; v < PGDVS_ITEM_MAX_VIEWS; ++v) {
    PGDVS_REQUIRE(v >= n_views || (ids[v] >= 0 && ids[v] < F), "%s: ids[%d] = %d, the store has %d frames", op, v,
                  v < n_views ? ids[v] : 0, F);
    p.ids[v] = v < n_views ? ids[v] : 0;
    for (int c = 0; c < 2; ++c) p.ss[v][c] = v < n_views ? scale_shift[(size_t)v * 2 + c] : 0.0;
  }
  p.n_range = range ? group_sizes[0] : 0;
  p.rays = range ? rays : nullptr;
  for (int c = 0; c < 4; ++c) p.A2[c] = range ? inv_c2w_tgt[8 + c] : 0.0;
  PGDVS_REQUIRE(!range || nv_shape_ok(p.n_range, H, W), "%s: a range over %d views of %d x %d (H W >= 2, views H W < 2^31)", op,
                p.n_range, H, W);
  PGDVS_REQUIRE(!range || aligned16(workspace), "%s: the workspace must be 16-byte aligned", op);
  hipStream_t st = as_stream(stream);
  Work<double, NvState> w = {};  // no keys and no state without a range
  NvFinish fin;
  if (range)
    if (const int rc = nv_setup(op, (int64_t)p.n_range * n, depth_range, near_far, workspace, workspace_bytes, st, w, fin)) return rc;
  const int64_t work = n >= 4 ? n >> 2 : n;  // quads; a view that takes the scalar statement strides over them
  PGDVS_LAUNCH("item_zoe_depths", item_zoe_kernel, dim3((unsigned)cdiv(work, kBlock), (unsigned)n_views), dim3(kBlock), 0, st, p, w.keys,
               w.state);
  if (range) select_passes<double, 3>(kNvLabels, w, (int64_t)p.n_range * n, fin, st);
  return check_launch(op);
}
