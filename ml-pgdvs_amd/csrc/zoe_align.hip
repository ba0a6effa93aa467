// The arithmetic of upstream's ZoeDepth stage (pgdvs/preprocess/compute_zoedepth.py): where the COLMAP points land in a
// frame, what the motion mask and the predicted depth are there, and the scale and shift that align the prediction with
// the points in disparity.  Float64 throughout, as scipy and NumPy 2 run it.
//
// pgdvs_zoe_sample (:262-294)
//   prefilter  scipy.ndimage.map_coordinates(order=3, mode="constant") first turns the whole image into cubic B-spline
//              coefficients: per axis the line times the gain (1 - z)(1 - 1/z), z = sqrt(3) - 2, the causal recursion
//              c[i] += z c[i-1] from scipy's mirror start, the anticausal one c[i] = z (c[i+1] - c[i]) from its mirror end;
//              axis 0 first.  Both images (mask, prediction) go through together.
//              columns: one thread per column, so a wavefront reads and writes 64 neighbouring doubles per step.
//              rows: a workgroup takes 32 rows x 128 columns; the window with a 40-column halo on either side goes through
//              LDS (coalesced loads, row stride 209 doubles: the 32 walking lanes fall on 32 different bank pairs), one lane
//              walks each row there.  A window that does not start at column 0 starts the recursion from the raw sample
//              40 columns early, one that does not end at the last column ends it 40 columns late: |z|^40 < 1e-22 of the
//              data's scale is what the chunk's own columns see of either.  The start sum at column 0 stops after 64 terms
//              (|z|^64 < 1e-36) on lines longer than 65.
//   flags      one thread per point: the projection, then upstream's three tests in its order, each on the float
//              coordinate: inside [0,W) x [0,H), spline(mask) < 0.1, depth > 1e-3.  Only a coordinate that passed the first
//              test reaches the spline, and the spline forms indices only from a coordinate inside [0, n-1]: outside it the
//              sample is 0, which is scipy's answer in (n-1, n) too.
//   compact    scan.hip's ordered compaction of the flags.
//   gather     one thread per kept point: its projection again (the same code, the same bits), the prediction's sample
//              rounded to float32 as scipy's float32 output is, the point's index.
//
// pgdvs_zoe_fit (:309-388) and pgdvs_zoe_errors (:424-465)
//   elementwise kernels in upstream's types (float32 nn_disp and its median, TINY_VAL added in float32, float64 ratios and
//   mvs_disp); every median and the two neighbours of np.quantile(., 0.8) through the shared radix select
//   (radix_select.h), on the trimmed subset by giving the other elements the largest key and taking the ranks from the
//   subset's device-side count; the means from one-workgroup float64 tree sums (deterministic).  flag_trim is
//   diff <= threshold, upstream's comparison.
//
// The library is built with -ffp-contract=off -fno-fast-math: a plain * + / rounds once.
#include <cmath>

#include "common.h"
#include "radix_select.h"
#include "scan.h"
#include "wave.h"

namespace pgdvs {
namespace {

using radix::Key;
using radix::kBins;
using radix::kBlock;

// ---------------------------------------------------------------------------- spline prefilter

constexpr double kPole = 1.7320508075688772 - 2.0;  // sqrt(3.0) - 2.0 as scipy's C evaluates it
constexpr double kGain = (1.0 - kPole) * (1.0 - 1.0 / kPole);
constexpr int kHalo = 40, kInitTerms = 64;
constexpr int kRowTile = 32, kChunk = 128, kWin = kChunk + 2 * kHalo, kWinPad = kWin + 1;
static_assert(kWin > kInitTerms + 1, "the first window holds every term of the start sum");

// scipy's _init_causal_mirror on the gained line x(0) .. x(n-1), n >= 2
template <typename Load> __device__ __forceinline__ double causal_init(Load x, int n) {
  if (n - 1 <= kInitTerms) {
    double zn1 = 1.0;
    for (int i = 0; i < n - 1; ++i) zn1 *= kPole;
    double zi = kPole, c0 = x(0) + zn1 * x(n - 1);
    for (int i = 1; i < n - 1; ++i) {
      c0 += zi * (x(i) + zn1 * x(n - 1 - i));
      zi *= kPole;
    }
    return c0 / (1.0 - zn1 * zn1);
  }
  double zi = kPole, c0 = x(0);
  for (int i = 1; i <= kInitTerms; ++i) {
    c0 += zi * x(i);
    zi *= kPole;
  }
  return c0;
}

// scipy's _init_anticausal_mirror from the last two causal values
__device__ __forceinline__ double anticausal_init(double before_last, double last) {
  return (kPole * before_last + last) * kPole / (kPole * kPole - 1.0);
}

// axis 0: grid (ceil(W / 256), 2 images), one thread per column; tmp[2,H,W]
__global__ void __launch_bounds__(256) zoe_col_kernel(const float *__restrict__ img0, const float *__restrict__ img1, int H, int W,
                                                      double *__restrict__ tmp) {
  const int col = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (col >= W) return;
  const float *src = (blockIdx.y ? img1 : img0) + col;
  double *c = tmp + (size_t)blockIdx.y * H * W + col;
  auto x = [&](int i) { return (double)src[(size_t)i * W] * kGain; };
  double prev = causal_init(x, H), before = prev;
  c[0] = prev;
  for (int i = 1; i < H; ++i) {
    before = prev;
    prev = x(i) + kPole * prev;
    c[(size_t)i * W] = prev;
  }
  double next = anticausal_init(before, prev);
  c[(size_t)(H - 1) * W] = next;
  for (int i = H - 2; i >= 0; --i) {
    next = kPole * (next - c[(size_t)i * W]);
    c[(size_t)i * W] = next;
  }
}

// axis 1: grid (ceil(W / kChunk), ceil(H / kRowTile), 2 images); tmp[2,H,W] -> coef[2,H,W]
__global__ void __launch_bounds__(256) zoe_row_kernel(const double *__restrict__ tmp, int H, int W, double *__restrict__ coef) {
  __shared__ double t[kRowTile][kWinPad];
  const int r0 = (int)blockIdx.y * kRowTile, s = (int)blockIdx.x * kChunk;
  const int e = s + kChunk < W ? s + kChunk : W;
  const int w0 = s - kHalo > 0 ? s - kHalo : 0, w1 = e + kHalo < W ? e + kHalo : W;
  const int wl = w1 - w0;  // 2 <= wl <= kWin: the first window is min(W, 168) long, a later one reaches back 40 columns
  const size_t img = (size_t)blockIdx.z * H * W;
  for (int k = threadIdx.x; k < kRowTile * wl; k += 256) {
    const int r = k / wl, j = k - r * wl;
    if (r0 + r < H) t[r][j] = tmp[img + (size_t)(r0 + r) * W + w0 + j] * kGain;
  }
  __syncthreads();
  if ((int)threadIdx.x < kRowTile && r0 + (int)threadIdx.x < H) {
    double *row = t[threadIdx.x];
    double prev = w0 == 0 ? causal_init([&](int i) { return row[i]; }, W) : row[0], before = prev;
    row[0] = prev;
    for (int j = 1; j < wl; ++j) {
      before = prev;
      prev = row[j] + kPole * prev;
      row[j] = prev;
    }
    double next = anticausal_init(before, prev);  // scipy's end at the last column; 40 columns from the chunk otherwise
    row[wl - 1] = next;
    for (int j = wl - 2; j >= s - w0; --j) {
      next = kPole * (next - row[j]);
      row[j] = next;
    }
  }
  __syncthreads();
  const int cl = e - s;
  for (int k = threadIdx.x; k < kRowTile * cl; k += 256) {
    const int r = k / cl, j = k - r * cl;
    if (r0 + r < H) coef[img + (size_t)(r0 + r) * W + s + j] = t[r][s - w0 + j];
  }
}

// ---------------------------------------------------------------------------- projection and look-up

struct Cam {
  double w2c[12];  // rows 0..2 of the frame's world-to-camera matrix
  double K[9];
};

// out = w2c @ [X,1]; im = K @ out[:3]; depth = im[2]; (x, y, one) = im / im[2]
__device__ __forceinline__ void project(const Cam &cam, const float *__restrict__ p, double &x, double &y, double &one, double &depth) {
  const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
  double o[3], q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = ((cam.w2c[r * 4 + 0] * X + cam.w2c[r * 4 + 1] * Y) + cam.w2c[r * 4 + 2] * Z) + cam.w2c[r * 4 + 3];
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = (cam.K[r * 3 + 0] * o[0] + cam.K[r * 3 + 1] * o[1]) + cam.K[r * 3 + 2] * o[2];
  depth = q[2];
  x = q[0] / q[2];
  y = q[1] / q[2];
  one = q[2] / q[2];
}

// whole-sample symmetric reflection of a tap index, n >= 2
__device__ __forceinline__ int mirror(int i, int n) {
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// scipy's cubic weights of the taps floor(x) - 1 .. floor(x) + 2, f = x - floor(x)
__device__ __forceinline__ void cubic_weights(double f, double w[4]) {
  const double z = 1.0 - f;
  w[1] = (f * f * (f - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = z * z * z / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
}

// map_coordinates(order=3, mode="constant", cval=0) at (row, col), rounded to float32.  No index is formed unless the
// coordinate lies in [0, H-1] x [0, W-1] (NaN fails the test).
__device__ __forceinline__ float spline_at(const double *__restrict__ c, int H, int W, double row, double col) {
  if (!(row >= 0.0 && row <= (double)(H - 1) && col >= 0.0 && col <= (double)(W - 1))) return 0.0f;
  const double fr = floor(row), fc = floor(col);
  double wr[4], wc[4];
  cubic_weights(row - fr, wr);
  cubic_weights(col - fc, wc);
  const int rs = (int)fr - 1, cs = (int)fc - 1;
  int cj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cj[j] = mirror(cs + j, W);
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double *line = c + (size_t)mirror(rs + i, H) * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) t += line[cj[j]] * wr[i] * wc[j];
  }
  return (float)t;
}

struct SampleParams {
  Cam cam;
  const float *pts;  // [P,3]
  int64_t P;
  int H, W;
  const double *coef;  // [2,H,W]: mask, prediction
};

__global__ void __launch_bounds__(256) zoe_flags_kernel(SampleParams p, uint8_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.P) return;
  double x, y, one, depth;
  project(p.cam, p.pts + i * 3, x, y, one, depth);
  bool keep = x >= 0.0 && x < (double)p.W && y >= 0.0 && y < (double)p.H;
  if (keep) keep = spline_at(p.coef, p.H, p.W, y, x) < 0.1f;
  flags[i] = keep && depth > 1e-3;
}

__global__ void __launch_bounds__(256) zoe_gather_kernel(SampleParams p, const int32_t *__restrict__ idx, const int32_t *__restrict__ count,
                                                         double *__restrict__ proj, double *__restrict__ depth_mvs,
                                                         float *__restrict__ depth_pred, int64_t *__restrict__ index) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (int64_t)*count) return;
  const int64_t i = idx[k];
  double x, y, one, depth;
  project(p.cam, p.pts + i * 3, x, y, one, depth);
  proj[k] = x;
  proj[p.P + k] = y;
  proj[2 * p.P + k] = one;
  depth_mvs[k] = depth;
  depth_pred[k] = spline_at(p.coef + (size_t)p.H * p.W, p.H, p.W, y, x);
  index[k] = i;
}

bool sample_shape_ok(int H, int W, int64_t P) {
  return H >= 2 && W >= 2 && (int64_t)H * W < (1ll << 30) && P >= 1 && P < (1ll << 31);
}

// tmp and coef [2,H,W] double each, flags, idx, the compaction's block counts
struct SampleLayout {
  int64_t coef, flags, idx, compact, total;
};

SampleLayout sample_layout(int H, int W, int64_t P) {
  SampleLayout l;
  l.coef = align_up((int64_t)2 * H * W * 8, 256);
  l.flags = 2 * l.coef;
  l.idx = l.flags + align_up(P, 256);
  l.compact = l.idx + align_up(P * 4, 256);
  l.total = l.compact + compact_workspace_bytes(P);
  return l;
}

// ---------------------------------------------------------------------------- fit

constexpr float kTiny32 = (float)1.0e-16;  // TINY_VAL where numpy adds it to a float32 array
constexpr double kTiny = 1.0e-16;
constexpr int kSumBlock = 1024;

struct FitState {
  radix::Sel<2> sel;
  int64_t count;  // elements that take part in the running select
  float nn_med, nn_scale;
  double mvs_med, mvs_scale, thres, gamma;
  double fit[4];  // scale_med, shift_med, scale_trim, shift_trim
  int32_t status;
};
static_assert(sizeof(FitState) <= 256, "the state takes one 256-byte slot");

struct FitWork {
  int64_t n;
  const float *pred;
  const double *mvs;
  float *nn_disp;
  double *mvs_disp, *ratio, *diff;
  void *keys;
  uint32_t *hist;
  FitState *st;
  uint8_t *flag;
};

struct FitLayout {
  int64_t mvs_disp, ratio, diff, keys, hist, state, total;
};

FitLayout fit_layout(int64_t n) {
  FitLayout l;
  l.mvs_disp = align_up(n * 4, 256);
  l.ratio = l.mvs_disp + align_up(n * 8, 256);
  l.diff = l.ratio + align_up(n * 8, 256);
  l.keys = l.diff + align_up(n * 8, 256);
  l.hist = l.keys + align_up(n * 8, 256);
  l.state = l.hist + (int64_t)radix::passes_for(64) * 2 * kBins * 4;
  l.total = l.state + 256;
  return l;
}

// the ranks of np.median over `count` elements: (count - 1) / 2 and count / 2
__global__ void median_init_kernel(FitState *__restrict__ st, int64_t count) {
  if (threadIdx.x != 0) return;
  if (count >= 0) st->count = count;
  const int64_t m = st->count > 0 ? st->count : 1;
  const int64_t rank[2] = {(m - 1) / 2, m / 2};
  radix::sel_init<2>(&st->sel, rank);
}

// the neighbours of np.quantile(., 0.8, method="linear") over the whole array (set up on the host)
__global__ void quantile_init_kernel(FitState *__restrict__ st, int64_t a, int64_t b, double gamma) {
  if (threadIdx.x != 0) return;
  const int64_t rank[2] = {a, b};
  radix::sel_init<2>(&st->sel, rank);
  st->gamma = gamma;
}

template <typename T, typename Fin>
__global__ void __launch_bounds__(128) fit_select_kernel(Fin fin, int pass, int last_pass, FitState *__restrict__ st,
                                                         const uint32_t *__restrict__ hist) {
  radix::select_digits<T, 2>(pass, &st->sel, hist);
  if (threadIdx.x == 0 && pass == last_pass) fin(st, radix::rank_value<T, 2>(&st->sel, 0), radix::rank_value<T, 2>(&st->sel, 1));
}

template <typename T, typename Fin> int run_select(const char *op, const FitWork &w, const Fin &fin, hipStream_t st) {
  const int passes = radix::passes_for(Key<T>::kBits);
  if (hipMemsetAsync(w.hist, 0, (size_t)passes * 2 * kBins * 4, st) != hipSuccess) {
    set_error("%s: clearing the histograms failed", op);
    return PGDVS_ERR_LAUNCH;
  }
  const unsigned hgrid = radix::hist_grid(w.n);
  typedef typename Key<T>::U U;
  for (int pass = 0; pass < passes; ++pass) {
    uint32_t *hp = w.hist + (size_t)pass * 2 * kBins;
    PGDVS_LAUNCH("zoe_fit_hist", (radix::hist_kernel<T, 2>), dim3(hgrid), dim3(kBlock), 0, st, static_cast<const U *>(w.keys), w.n, pass,
                 &w.st->sel, hp);
    PGDVS_LAUNCH("zoe_fit_select", (fit_select_kernel<T, Fin>), dim3(1), dim3(128), 0, st, fin, pass, passes - 1, w.st, hp);
  }
  return PGDVS_OK;
}

// np.median's mean of the two middle elements in the array's type: (a + b) / 2, or a / 1 when they are one element
struct FinNnMedian {
  __device__ void operator()(FitState *st, float a, float b) const { st->nn_med = st->count & 1 ? a : (a + b) / 2.0f; }
};
struct FinMvsMedian {
  __device__ void operator()(FitState *st, double a, double b) const { st->mvs_med = st->count & 1 ? a : (a + b) / 2.0; }
};
// a scale: negative medians are clamped to 0 (NaN stays, as upstream's `< 0` leaves it); a shift: the median itself
struct FinFit {
  int slot;
  __device__ void operator()(FitState *st, double a, double b) const {
    double m = st->count & 1 ? a : (a + b) / 2.0;
    if ((slot & 1) == 0 && m < 0.0) m = 0.0;
    st->fit[slot] = m;
  }
};
struct FinThreshold {
  __device__ void operator()(FitState *st, double a, double b) const { st->thres = radix::lerp_np(a, b, st->gamma); }
};

__device__ __forceinline__ double block_sum(double v, double *sh) {
  v = wave_sum_down(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kSumBlock / 64; ++w) s += sh[w];
  __syncthreads();
  return s;  // thread 0 holds the sum
}

// nn_disp = 1 / (nn_depth + TINY) in float32, mvs_disp in float64; upstream's asserts become status bits
__global__ void __launch_bounds__(256) fit_disp_kernel(FitWork w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w.n) return;
  const float d = w.pred[i];
  const double m = w.mvs[i];
  if (!(d >= 0.0f)) atomicOr(&w.st->status, 1);
  if (!(m >= 0.0)) atomicOr(&w.st->status, 2);
  const float nd = 1.0f / (d + kTiny32);
  w.nn_disp[i] = nd;
  w.mvs_disp[i] = 1.0 / (m + kTiny);
  static_cast<uint32_t *>(w.keys)[i] = Key<float>::enc(nd);
}

__global__ void __launch_bounds__(256) fit_key_mvs_kernel(FitWork w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < w.n) static_cast<uint64_t *>(w.keys)[i] = Key<double>::enc(w.mvs_disp[i]);
}

// ratio = mvs_disp_shifted / (nn_disp_shifted + TINY): the sum in float32, the quotient in float64
__global__ void __launch_bounds__(256) fit_ratio_kernel(FitWork w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w.n) return;
  const float ns = w.nn_disp[i] - w.st->nn_med;
  const double ms = w.mvs_disp[i] - w.st->mvs_med;
  const double r = ms / (double)(ns + kTiny32);
  w.ratio[i] = r;
  static_cast<uint64_t *>(w.keys)[i] = Key<double>::enc(r);
}

// np.mean(|nn_disp_shifted|) (a float32 mean: numpy's float32 sum, here the float64 sum rounded to float32, over n) and
// np.mean(|mvs_disp_shifted|); one workgroup
__global__ void __launch_bounds__(kSumBlock) fit_scales_kernel(FitWork w) {
  __shared__ double sh[kSumBlock / 64];
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < w.n; i += kSumBlock) {
    a += (double)fabsf(w.nn_disp[i] - w.st->nn_med);
    b += fabs(w.mvs_disp[i] - w.st->mvs_med);
  }
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  if (threadIdx.x == 0) {
    w.st->nn_scale = (float)((double)(float)a / (double)w.n);
    w.st->mvs_scale = b / (double)w.n;
  }
}

// keys of mvs_disp - nn_disp scale (float32 nn_disp widened, as NumPy 2 multiplies it by a float64 scalar); with
// `trimmed`, elements outside flag_trim get the largest key and sort behind the subset
__global__ void __launch_bounds__(256) fit_shift_keys_kernel(FitWork w, int slot, int trimmed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w.n) return;
  const double v = w.mvs_disp[i] - (double)w.nn_disp[i] * w.st->fit[slot];
  static_cast<uint64_t *>(w.keys)[i] = (!trimmed || w.flag[i]) ? Key<double>::enc(v) : ~0ull;
}

// |nn_disp_normalized - mvs_disp_normalized|: the first quotient in float32, the rest in float64
__global__ void __launch_bounds__(256) fit_diff_kernel(FitWork w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w.n) return;
  const float nn = (w.nn_disp[i] - w.st->nn_med) / (w.st->nn_scale + kTiny32);
  const double mv = (w.mvs_disp[i] - w.st->mvs_med) / (w.st->mvs_scale + kTiny);
  const double d = fabs((double)nn - mv);
  w.diff[i] = d;
  static_cast<uint64_t *>(w.keys)[i] = Key<double>::enc(d);
}

// flag_trim = diff <= threshold, its count, and the trimmed ratios' keys; one workgroup
__global__ void __launch_bounds__(kSumBlock) fit_trim_kernel(FitWork w) {
  __shared__ double sh[kSumBlock / 64];
  double c = 0.0;
  for (int64_t i = threadIdx.x; i < w.n; i += kSumBlock) {
    const bool f = w.diff[i] <= w.st->thres;
    w.flag[i] = f;
    static_cast<uint64_t *>(w.keys)[i] = f ? Key<double>::enc(w.ratio[i]) : ~0ull;
    c += f ? 1.0 : 0.0;
  }
  c = block_sum(c, sh);
  if (threadIdx.x == 0) w.st->count = (int64_t)c;
}

__global__ void fit_finish_kernel(const FitState *__restrict__ st, double *__restrict__ fit, int32_t *__restrict__ status) {
  if (threadIdx.x < 4) fit[threadIdx.x] = st->fit[threadIdx.x];
  if (threadIdx.x == 0) *status = st->status;
}

// ---------------------------------------------------------------------------- errors

struct ErrParams {
  const float *pred;
  const double *mvs;
  const uint8_t *flag;
  int64_t n;
  double ss[4][2];  // (scale, shift) of med_share, med_indiv, trim_share, trim_indiv
};

// over flag_trim: diff = mvs_depth - 1 / (nn_disp scale + shift); mae = mean |diff|, me = mean diff; one workgroup
__global__ void __launch_bounds__(kSumBlock) zoe_errors_kernel(ErrParams p, double *__restrict__ out) {
  __shared__ double sh[kSumBlock / 64];
  double mae[4] = {0.0, 0.0, 0.0, 0.0}, me[4] = {0.0, 0.0, 0.0, 0.0}, c = 0.0;
  for (int64_t i = threadIdx.x; i < p.n; i += kSumBlock) {
    if (!p.flag[i]) continue;
    const double nd = (double)(1.0f / (p.pred[i] + kTiny32));
    const double m = p.mvs[i];
    c += 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = m - 1.0 / (nd * p.ss[k][0] + p.ss[k][1]);
      mae[k] += fabs(d);
      me[k] += d;
    }
  }
  c = block_sum(c, sh);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = block_sum(mae[k], sh), b = block_sum(me[k], sh);
    if (threadIdx.x == 0) {
      out[k] = a / c;
      out[4 + k] = b / c;
    }
  }
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

#define ZS_SHAPE_MSG "pgdvs_zoe_sample: bad shape H=%d W=%d P=%lld (H, W >= 2, H W < 2^30, 1 <= P < 2^31)"

PGDVS_API int64_t pgdvs_zoe_sample_workspace_bytes(int H, int W, int64_t P) {
  if (!sample_shape_ok(H, W, P)) {
    set_error(ZS_SHAPE_MSG, H, W, (long long)P);
    return PGDVS_ERR_INVALID;
  }
  return sample_layout(H, W, P).total;
}

PGDVS_API int pgdvs_zoe_sample(const float *pred_depth, const float *mask, int H, int W, const float *pts3d, int64_t P,
                               const double *w2c, const double *K, double *proj_pcl, double *pcl_depth_mvs, float *pcl_depth_pred,
                               int64_t *index, int32_t *count, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_depth && mask && pts3d && w2c && K && proj_pcl && pcl_depth_mvs && pcl_depth_pred && index && count,
                "pgdvs_zoe_sample: null pointer");
  PGDVS_REQUIRE(sample_shape_ok(H, W, P), ZS_SHAPE_MSG, H, W, (long long)P);
  const SampleLayout l = sample_layout(H, W, P);
  if (!workspace || workspace_bytes < l.total) {
    set_error("pgdvs_zoe_sample: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)l.total);
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char *ws = static_cast<char *>(workspace);
  double *tmp = reinterpret_cast<double *>(ws), *coef = reinterpret_cast<double *>(ws + l.coef);
  uint8_t *flags = reinterpret_cast<uint8_t *>(ws + l.flags);
  int32_t *idx = reinterpret_cast<int32_t *>(ws + l.idx);
  PGDVS_LAUNCH("zoe_spline_cols", zoe_col_kernel, dim3((unsigned)cdiv(W, 256), 2), dim3(256), 0, st, mask, pred_depth, H, W, tmp);
  PGDVS_LAUNCH("zoe_spline_rows", zoe_row_kernel, dim3((unsigned)cdiv(W, kChunk), (unsigned)cdiv(H, kRowTile), 2), dim3(256), 0, st, tmp,
               H, W, coef);
  SampleParams p;
  for (int r = 0; r < 12; ++r) p.cam.w2c[r] = w2c[r];
  for (int k = 0; k < 9; ++k) p.cam.K[k] = K[k];
  p.pts = pts3d;
  p.P = P;
  p.H = H;
  p.W = W;
  p.coef = coef;
  const unsigned grid = (unsigned)cdiv(P, 256);
  PGDVS_LAUNCH("zoe_sample_flags", zoe_flags_kernel, dim3(grid), dim3(256), 0, st, p, flags);
  if (const int rc = compact_u8(flags, P, idx, count, ws + l.compact, l.total - l.compact, st)) return rc;
  PGDVS_LAUNCH("zoe_sample_gather", zoe_gather_kernel, dim3(grid), dim3(256), 0, st, p, idx, count, proj_pcl, pcl_depth_mvs,
               pcl_depth_pred, index);
  return check_launch("pgdvs_zoe_sample");
}

#define ZF_SHAPE_MSG "%s: bad count n=%lld (1 <= n < 2^31)"

PGDVS_API int64_t pgdvs_zoe_fit_workspace_bytes(int64_t n) {
  if (n < 1 || n >= (1ll << 31)) {
    set_error(ZF_SHAPE_MSG, "pgdvs_zoe_fit", (long long)n);
    return PGDVS_ERR_INVALID;
  }
  return fit_layout(n).total;
}

PGDVS_API int pgdvs_zoe_fit(const float *pcl_depth_pred, const double *pcl_depth_mvs, int64_t n, double *fit, uint8_t *flag_trim,
                            int32_t *status, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  const char *op = "pgdvs_zoe_fit";
  PGDVS_REQUIRE(pcl_depth_pred && pcl_depth_mvs && fit && flag_trim && status, "pgdvs_zoe_fit: null pointer");
  PGDVS_REQUIRE(n >= 1 && n < (1ll << 31), ZF_SHAPE_MSG, op, (long long)n);
  const FitLayout l = fit_layout(n);
  if (!workspace || workspace_bytes < l.total) {
    set_error("pgdvs_zoe_fit: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)l.total);
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char *ws = static_cast<char *>(workspace);
  FitWork w;
  w.n = n;
  w.pred = pcl_depth_pred;
  w.mvs = pcl_depth_mvs;
  w.nn_disp = reinterpret_cast<float *>(ws);
  w.mvs_disp = reinterpret_cast<double *>(ws + l.mvs_disp);
  w.ratio = reinterpret_cast<double *>(ws + l.ratio);
  w.diff = reinterpret_cast<double *>(ws + l.diff);
  w.keys = ws + l.keys;
  w.hist = reinterpret_cast<uint32_t *>(ws + l.hist);
  w.st = reinterpret_cast<FitState *>(ws + l.state);
  w.flag = flag_trim;
  if (hipMemsetAsync(w.st, 0, 256, st) != hipSuccess) {
    set_error("pgdvs_zoe_fit: clearing the state failed");
    return PGDVS_ERR_LAUNCH;
  }
  const dim3 grid((unsigned)cdiv(n, 256)), block(256), one(1), lane(64), wide(kSumBlock);
  int rc;
  // the medians of nn_disp (float32) and mvs_disp
  PGDVS_LAUNCH("zoe_fit_disp", fit_disp_kernel, grid, block, 0, st, w);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, n);
  if ((rc = run_select<float>(op, w, FinNnMedian(), st))) return rc;
  PGDVS_LAUNCH("zoe_fit_keys", fit_key_mvs_kernel, grid, block, 0, st, w);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, n);
  if ((rc = run_select<double>(op, w, FinMvsMedian(), st))) return rc;
  // the median fit: scale, then shift
  PGDVS_LAUNCH("zoe_fit_ratio", fit_ratio_kernel, grid, block, 0, st, w);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, n);
  if ((rc = run_select<double>(op, w, FinFit{0}, st))) return rc;
  PGDVS_LAUNCH("zoe_fit_keys", fit_shift_keys_kernel, grid, block, 0, st, w, 0, 0);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, n);
  if ((rc = run_select<double>(op, w, FinFit{1}, st))) return rc;
  // the trim set: the normalised difference against its 0.8 quantile
  PGDVS_LAUNCH("zoe_fit_scales", fit_scales_kernel, one, wide, 0, st, w);
  PGDVS_LAUNCH("zoe_fit_diff", fit_diff_kernel, grid, block, 0, st, w);
  int64_t qa, qb;
  double gamma;
  radix::quantile_setup<double>(n, 0.8, qa, qb, gamma);
  PGDVS_LAUNCH("zoe_fit_init", quantile_init_kernel, one, lane, 0, st, w.st, qa, qb, gamma);
  if ((rc = run_select<double>(op, w, FinThreshold(), st))) return rc;
  // the trimmed fit over the subset
  PGDVS_LAUNCH("zoe_fit_trim", fit_trim_kernel, one, wide, 0, st, w);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, (int64_t)-1);
  if ((rc = run_select<double>(op, w, FinFit{2}, st))) return rc;
  PGDVS_LAUNCH("zoe_fit_keys", fit_shift_keys_kernel, grid, block, 0, st, w, 2, 1);
  PGDVS_LAUNCH("zoe_fit_init", median_init_kernel, one, lane, 0, st, w.st, (int64_t)-1);
  if ((rc = run_select<double>(op, w, FinFit{3}, st))) return rc;
  PGDVS_LAUNCH("zoe_fit_finish", fit_finish_kernel, one, lane, 0, st, w.st, fit, status);
  return check_launch(op);
}

PGDVS_API int pgdvs_zoe_errors(const float *pcl_depth_pred, const double *pcl_depth_mvs, const uint8_t *flag_trim, int64_t n,
                               const double *scale_shift, double *errors, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pcl_depth_pred && pcl_depth_mvs && flag_trim && scale_shift && errors, "pgdvs_zoe_errors: null pointer");
  PGDVS_REQUIRE(n >= 1 && n < (1ll << 31), ZF_SHAPE_MSG, "pgdvs_zoe_errors", (long long)n);
  ErrParams p = {pcl_depth_pred, pcl_depth_mvs, flag_trim, n};
  for (int k = 0; k < 4; ++k)
    for (int c = 0; c < 2; ++c) p.ss[k][c] = scale_shift[k * 2 + c];
  PGDVS_LAUNCH("zoe_errors", zoe_errors_kernel, dim3(1), dim3(kSumBlock), 0, as_stream(stream), p, errors);
  return check_launch("pgdvs_zoe_errors");
}
