// SURVEY 8f-3 DyCheck: the per-pixel depth range of one DyCheck iPhone item (pgdvs/datasets/dycheck_iphone_eval.py:455-524),
// bit-identical to the loader's numpy path (pgdvs_amd/datasets/dycheck_iphone.py depth_range_numpy).
//
// T is the points' type: float for float32 depth (the iPhone files; then upstream's arithmetic is float32 end to end, and
// np.quantile keeps float32), double for float64 depth (numpy promotes every step after the rays to float64).
//
// points   one thread per spatial pixel (view-major, as upstream concatenates them).  Unprojection as _compute_pcl through
//          torch's CPU bmm: d = fma(M[:,1], v, M[:,0] u) + M[:,2] in fp32, X = o + d depth in T.  z = row 2 of
//          inv(raw_c2w_tgt) @ [X,1] with numpy's BLAS order (fused multiply-adds, k ascending); its order-preserving key goes
//          to the workspace.  Static points (dyn_mask == 0) are moved and projected in T the same way, divided by
//          (z + 1e-8), kept when 0 <= col <= W-1 and 0 <= row <= H-1 (no z > 0 test, as upstream), truncated, and the pixel
//          keeps the largest flat index (numpy's fancy assignment: the last point wins) through atomicMax.
// select   np.quantile(z, q, method="linear") for q = 0.1, 0.9: the two neighbouring ranks of each virtual index, found
//          exactly by the shared radix select (radix_select.h: 3 passes for float, 6 for double, the four ranks together).
//          The last select pass interpolates with numpy's _lerp and clamps with near / far as Python's max / min compare.
// write    one thread per target pixel: the winning point's z -+ 1e-4 in T, or the constant range when no point hit it.
#include <cmath>

#include "common.h"
#include "radix_select.h"

namespace pgdvs {
namespace {

using radix::Key;
using radix::kBins;
using radix::kBlock;
constexpr int kRanks = 4;

__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T> struct Params {
  const void *depth;       // [V,H,W] T
  const float *dyn_mask;   // [V,H,W], static where == 0
  const float *rays;       // [V,12]: M (3x3 row-major), o
  int V, H, W;
  int64_t n;               // V H W
  T A2[4];                 // row 2 of inv(raw_c2w_tgt)
  T B[12];                 // rows 0..2 of inv(c2w_tgt)
  T K[9];                  // K_tgt[:3,:3]
  // quantile set-up (host, numpy's float semantics of T): ranks a/b and weight t of q = 0.1 and q = 0.9
  int64_t rank[kRanks];
  T gamma[2];
  T near_t, far_t;
  float near32, far32;
};

struct State {
  radix::Sel<kRanks> sel;
  uint32_t nan_seen;
  float lo32, hi32;
  double q[2];
};

// world point of spatial pixel i (in T)
template <typename T>
__device__ __forceinline__ void unproject(const Params<T> &p, int64_t i, T X[3]) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int v = (int)(i / HW);
  const int64_t pix = i - (int64_t)v * HW;
  const int row = (int)(pix / p.W), col = (int)(pix - (int64_t)row * p.W);
  const float *r = p.rays + (size_t)v * 12;
  const float u = (float)col, w = (float)row;
  const T d = static_cast<const T *>(p.depth)[i];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float dir = __builtin_fmaf(r[ax * 3 + 1], w, r[ax * 3 + 0] * u) + r[ax * 3 + 2];
    X[ax] = (T)r[9 + ax] + (T)dir * d;
  }
}

// static point -> (camera z, projected column / row) in T, numpy's matmul order
template <typename T>
__device__ __forceinline__ void project_static(const Params<T> &p, const T X[3], T &z, T &col, T &row) {
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
__global__ void __launch_bounds__(kBlock) points_kernel(Params<T> p, typename Key<T>::U *__restrict__ keys,
                                                        int32_t *__restrict__ last, State *__restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  T X[3];
  unproject(p, i, X);
  const T z = fmaT(p.A2[2], X[2], fmaT(p.A2[1], X[1], p.A2[0] * X[0])) + p.A2[3];
  keys[i] = Key<T>::enc(z);
  if (z != z) atomicOr(&st->nan_seen, 1u);
  if (p.dyn_mask[i] == 0.0f) {
    T zc, col, row;
    project_static(p, X, zc, col, row);
    if (row >= (T)0 && row <= (T)(p.H - 1) && col >= (T)0 && col <= (T)(p.W - 1))
      atomicMax(&last[(int64_t)(int)row * p.W + (int)col], (int32_t)i);  // i < 2^31 (checked on entry)
  }
}

template <typename T> __global__ void init_kernel(Params<T> p, State *__restrict__ st) {
  if (threadIdx.x != 0) return;
  radix::sel_init<kRanks>(&st->sel, p.rank);
  st->nan_seen = 0;
}

// one block, one wavefront per rank: pick this pass's digit of every rank; the last pass finishes the range
template <typename T>
__global__ void __launch_bounds__(kBlock) select_kernel(Params<T> p, int pass, int last_pass, State *__restrict__ st,
                                                        const uint32_t *__restrict__ hist) {
  radix::select_digits<T, kRanks>(pass, &st->sel, hist);
  if (threadIdx.x == 0 && pass == last_pass) {
    T q[2];
    for (int j = 0; j < 2; ++j)
      q[j] = radix::lerp_np(radix::rank_value<T, kRanks>(&st->sel, 2 * j), radix::rank_value<T, kRanks>(&st->sel, 2 * j + 1),
                            p.gamma[j]);
    if (st->nan_seen) q[0] = q[1] = (T)NAN;  // np.quantile returns NaN when z holds one
    // Python's max(near, q) / min(far, q): q when q > near (resp. q < far), compared in T; else the bound
    st->lo32 = q[0] > p.near_t ? (float)q[0] : p.near32;
    st->hi32 = q[1] < p.far_t ? (float)q[1] : p.far32;
    st->q[0] = (double)q[0];
    st->q[1] = (double)q[1];
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) write_kernel(Params<T> p, const int32_t *__restrict__ last, const State *__restrict__ st,
                                                       float *__restrict__ out) {
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

struct Layout {
  int64_t keys, last, hist, state, total;
};

Layout layout(int64_t n, int64_t hw, int key_bytes, int passes) {
  Layout l;
  l.keys = 0;
  l.last = align_up(n * key_bytes, 256);
  l.hist = l.last + align_up(hw * 4, 256);
  l.state = l.hist + align_up((int64_t)passes * kRanks * kBins * 4, 256);
  l.total = l.state + align_up((int64_t)sizeof(State), 256);
  return l;
}

bool shape_ok(int V, int H, int W) {
  return V > 0 && H > 0 && W > 0 && (int64_t)V * H * W < (1ll << 31);
}

template <typename T>
int run(const void *depth, const float *dyn_mask, const float *rays, int V, int H, int W, const double *inv_raw_c2w_tgt,
        const double *inv_c2w_tgt, const double *K_tgt, double near_v, double far_v, float *out, double *quantiles,
        void *workspace, int64_t workspace_bytes, hipStream_t st) {
  typedef typename Key<T>::U U;
  const int64_t n = (int64_t)V * H * W, hw = (int64_t)H * W;
  const int passes = radix::passes_for(Key<T>::kBits);
  const Layout l = layout(n, hw, (int)sizeof(U), passes);
  if (!workspace || workspace_bytes < l.total) {
    set_error("pgdvs_dycheck_depth_range: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)l.total);
    return PGDVS_ERR_WORKSPACE;
  }
  Params<T> p;
  p.depth = depth;
  p.dyn_mask = dyn_mask;
  p.rays = rays;
  p.V = V;
  p.H = H;
  p.W = W;
  p.n = n;
  for (int c = 0; c < 4; ++c) p.A2[c] = (T)inv_raw_c2w_tgt[8 + c];
  for (int k = 0; k < 12; ++k) p.B[k] = (T)inv_c2w_tgt[k];
  for (int k = 0; k < 9; ++k) p.K[k] = (T)K_tgt[k];
  radix::quantile_setup<T>(n, (T)0.1, p.rank[0], p.rank[1], p.gamma[0]);
  radix::quantile_setup<T>(n, (T)0.9, p.rank[2], p.rank[3], p.gamma[1]);
  p.near_t = (T)near_v;
  p.far_t = (T)far_v;
  p.near32 = (float)near_v;
  p.far32 = (float)far_v;
  char *ws = static_cast<char *>(workspace);
  U *keys = reinterpret_cast<U *>(ws + l.keys);
  int32_t *last = reinterpret_cast<int32_t *>(ws + l.last);
  uint32_t *hist = reinterpret_cast<uint32_t *>(ws + l.hist);
  State *state = reinterpret_cast<State *>(ws + l.state);
  hipError_t e = hipMemsetAsync(last, 0xff, (size_t)hw * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(hist, 0, (size_t)(l.state - l.hist), st);
  if (e != hipSuccess) {
    set_error("pgdvs_dycheck_depth_range: %s", hipGetErrorString(e));
    return PGDVS_ERR_LAUNCH;
  }
  PGDVS_LAUNCH("dycheck_range_init", init_kernel<T>, dim3(1), dim3(64), 0, st, p, state);
  PGDVS_LAUNCH("dycheck_range_points", points_kernel<T>, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, p, keys, last, state);
  const unsigned hgrid = radix::hist_grid(n);
  for (int pass = 0; pass < passes; ++pass) {
    uint32_t *hp = hist + (size_t)pass * kRanks * kBins;
    PGDVS_LAUNCH("dycheck_range_hist", (radix::hist_kernel<T, kRanks>), dim3(hgrid), dim3(kBlock), 0, st, keys, n, pass,
                 &state->sel, hp);
    PGDVS_LAUNCH("dycheck_range_select", select_kernel<T>, dim3(1), dim3(kBlock), 0, st, p, pass, passes - 1, state, hp);
  }
  PGDVS_LAUNCH("dycheck_range_write", write_kernel<T>, dim3((unsigned)cdiv(hw, kBlock)), dim3(kBlock), 0, st, p, last, state, out);
  if (quantiles) {
    e = hipMemcpyAsync(quantiles, &state->q[0], 2 * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      set_error("pgdvs_dycheck_depth_range: %s", hipGetErrorString(e));
      return PGDVS_ERR_LAUNCH;
    }
  }
  return check_launch("pgdvs_dycheck_depth_range");
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_dycheck_depth_range_workspace_bytes(int V, int H, int W, int depth_f64) {
  if (!shape_ok(V, H, W)) {
    set_error("pgdvs_dycheck_depth_range: bad shape V=%d H=%d W=%d (each > 0, V H W < 2^31)", V, H, W);
    return PGDVS_ERR_INVALID;
  }
  const int kbits = depth_f64 ? 64 : 32;
  return layout((int64_t)V * H * W, (int64_t)H * W, kbits / 8, radix::passes_for(kbits)).total;
}

PGDVS_API int pgdvs_dycheck_depth_range(const void *depth, int depth_f64, const float *dyn_mask, const float *rays, int V, int H,
                                        int W, const double *inv_raw_c2w_tgt, const double *inv_c2w_tgt, const double *K_tgt,
                                        double near_v, double far_v, float *depth_range, double *quantiles, void *workspace,
                                        int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(depth && dyn_mask && rays && inv_raw_c2w_tgt && inv_c2w_tgt && K_tgt && depth_range,
                "pgdvs_dycheck_depth_range: null pointer");
  PGDVS_REQUIRE(shape_ok(V, H, W), "pgdvs_dycheck_depth_range: bad shape V=%d H=%d W=%d (each > 0, V H W < 2^31)", V, H, W);
  // upstream's matrices are float32 (DyCheckCamera's extrinsics and flat_cam); numpy promotes them to the points' type
  const double *mats[3] = {inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt};
  const int counts[3] = {16, 16, 9};
  for (int m = 0; m < 3; ++m)
    for (int k = 0; k < counts[m]; ++k)
      PGDVS_REQUIRE((double)(float)mats[m][k] == mats[m][k] || mats[m][k] != mats[m][k],
                    "pgdvs_dycheck_depth_range: matrix %d entry %d is not a float32 value", m, k);
  hipStream_t st = as_stream(stream);
  if (depth_f64)
    return run<double>(depth, dyn_mask, rays, V, H, W, inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt, near_v, far_v, depth_range,
                       quantiles, workspace, workspace_bytes, st);
  return run<float>(depth, dyn_mask, rays, V, H, W, inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt, near_v, far_v, depth_range, quantiles,
                    workspace, workspace_bytes, st);
}
