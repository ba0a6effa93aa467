// Pillow's 8-bit resampler (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc,
// ImagingResampleVertical_8bpc) for the BOX and LANCZOS filters, on decoded frames that are already on the device.
// include/pgdvs_hip.h states what is computed; this is how.
//
// resample_table  HOST.  One axis' bounds (first input index, tap count) and 22-bit fixed-point coefficients, the doubles in
//                 Pillow's order (this library is built with -ffp-contract=off; sin is libm's, as Pillow's).
// horizontal      grid (x tiles, rows, frames).  A block stages the span of its input row that its tile of output pixels
//                 reads in LDS: aligned dword loads for the interior, byte loads for the up to three bytes in front of the
//                 first aligned address and behind the last, so a wavefront's loads cover whole lines whatever the row's
//                 address.  A lane then makes four consecutive output bytes (taps from LDS, coefficients from the table,
//                 which the L1 holds: lanes of one pixel read the same words) and writes them with one dword store where
//                 the address allows, byte stores otherwise.  Only the rows the vertical pass reads are made.
// vertical        grid (x, output rows, frames).  A row's taps and coefficients are uniform over the block (scalar loads);
//                 a lane takes four consecutive bytes of every tap row with one dword load where the source's base and
//                 pitch are multiples of 4 (always for the intermediate image, whose pitch is padded), one byte per lane
//                 otherwise.
// Both passes: acc = 2^21 + sum k * byte in int32, then clamp(acc >> 22, 0, 255); the 8-bit rounding between them is Pillow's.
// No atomics, no scratch, no floating point on the device.  A table that does not fit the sizes it is used with (the caller
// uploads it) makes taps vanish, never an access outside the images: every lane checks its taps against the staged span
// (horizontal) or the source's rows (vertical).
#include <math.h>

#include "common.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int kLdsBytes = 16384;            // the staged span of an input row
constexpr int kMaxSize = PGDVS_RESAMPLE_MAX_SIZE, kMaxTaps = PGDVS_RESAMPLE_MAX_TAPS;

// ---------------------------------------------------------------------------- the table (host)
double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

struct AxisPlan {
  double scale, filterscale, support;
  int ksize;
};

AxisPlan axis_plan(int in_size, int out_size, int filter) {
  AxisPlan a;
  a.filterscale = a.scale = (double)in_size / out_size;
  if (a.filterscale < 1.0) a.filterscale = 1.0;
  a.support = (filter == PGDVS_RESAMPLE_BOX ? 0.5 : 3.0) * a.filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;  // (at most 6 * 16384 + 1)
  return a;
}

// output index xx reads inputs xmin .. xmin + n - 1 around `center`
void axis_bounds(const AxisPlan &a, int in_size, int xx, int *xmin, int *n, double *center) {
  *center = (xx + 0.5) * a.scale;
  int lo = (int)(*center - a.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(*center + a.support + 0.5);
  if (hi > in_size) hi = in_size;
  *xmin = lo;
  *n = hi - lo;
}

// the sizes and the filter, checked; what every entry point refuses
int check_axis(const char *what, int in_size, int out_size, int filter) {
  PGDVS_REQUIRE(filter == PGDVS_RESAMPLE_BOX || filter == PGDVS_RESAMPLE_LANCZOS, "%s: filter %d (0 = box, 1 = lanczos)", what, filter);
  PGDVS_REQUIRE(in_size >= 1 && in_size <= kMaxSize && out_size >= 1 && out_size <= kMaxSize, "%s: %d -> %d pixels (1 .. %d each)", what,
                in_size, out_size, kMaxSize);
  const int ksize = axis_plan(in_size, out_size, filter).ksize;
  PGDVS_REQUIRE(ksize <= kMaxTaps, "%s: %d -> %d pixels takes %d taps per output, at most %d", what, in_size, out_size, ksize, kMaxTaps);
  return PGDVS_OK;
}

// ---------------------------------------------------------------------------- the kernels
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrecisionBits;  // (arithmetic)
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// four consecutive output bytes at dst, `valid` of them inside the row: one dword where all four are and dst is aligned
__device__ __forceinline__ void store4(uint8_t *dst, const int *acc, int valid) {
  if (valid >= 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    *reinterpret_cast<uint32_t *>(dst) = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) |
                                         ((uint32_t)clip8(acc[3]) << 24);
    return;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (b < valid) dst[b] = (uint8_t)clip8(acc[b]);
}

// src: input row `row_lo + blockIdx.y` of frame blockIdx.z -> dst: row blockIdx.y of that frame, output pixels
// blockIdx.x * tx .. + tx - 1.  tx is a multiple of 4.
template <int C>
__global__ void __launch_bounds__(kBlock) resample_h_kernel(const uint8_t *__restrict__ src, int64_t src_frame, int64_t src_pitch, int row_lo,
                                                            uint8_t *__restrict__ dst, int64_t dst_frame, int64_t dst_pitch, int w_in, int w_out,
                                                            int tx, const int32_t *__restrict__ bounds, const int32_t *__restrict__ kk,
                                                            int ksize) {
  __shared__ uint32_t lds_w[kLdsBytes / 4 + 1];
  uint8_t *lds = reinterpret_cast<uint8_t *>(lds_w);
  const int x0 = blockIdx.x * tx;
  const int x1 = x0 + tx < w_out ? x0 + tx : w_out;
  // the tile's span of input pixels: xmin and xmin + n both grow with x
  int p0 = bounds[2 * x0], p1 = bounds[2 * (x1 - 1)] + bounds[2 * (x1 - 1) + 1];
  p0 = p0 < 0 ? 0 : (p0 > w_in ? w_in : p0);
  p1 = p1 < p0 ? p0 : (p1 > w_in ? w_in : p1);
  if ((p1 - p0) * C > kLdsBytes) p1 = p0 + kLdsBytes / C;
  const int nb = (p1 - p0) * C;
  const uint8_t *row = src + blockIdx.z * src_frame + (int64_t)(row_lo + (int)blockIdx.y) * src_pitch + (int64_t)p0 * C;
  // byte i of the span lives at lds[pad + i]: the first aligned global dword lands on an aligned LDS dword
  int head = (int)((4 - (reinterpret_cast<uintptr_t>(row) & 3)) & 3);
  if (head > nb) head = nb;
  const int pad = (4 - head) & 3;
  const int words = (nb - head) >> 2;
  const uint32_t *row_w = reinterpret_cast<const uint32_t *>(row + head);
  for (int w = threadIdx.x; w < words; w += kBlock) lds_w[((pad + head) >> 2) + w] = row_w[w];
  const int tail0 = head + 4 * words;
  if ((int)threadIdx.x < head) lds[pad + threadIdx.x] = row[threadIdx.x];
  if ((int)threadIdx.x < nb - tail0) lds[pad + tail0 + threadIdx.x] = row[tail0 + threadIdx.x];
  __syncthreads();

  const int count = (x1 - x0) * C;  // the tile's output bytes
  uint8_t *out = dst + blockIdx.z * dst_frame + (int64_t)blockIdx.y * dst_pitch + (int64_t)x0 * C;
  for (int q = threadIdx.x; q * 4 < count; q += kBlock) {
    int acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc[b] = 1 << (kPrecisionBits - 1);
      const int e = q * 4 + b;
      if (e >= count) continue;
      const int x = x0 + e / C, c = e % C;
      const int xmin = bounds[2 * x];
      int n = bounds[2 * x + 1];
      if (n > ksize || xmin < p0 || xmin + n > p1) n = 0;  // (a table of other sizes)
      const int32_t *k = kk + (int64_t)x * ksize;
      const uint8_t *px = lds + pad + (xmin - p0) * C + c;
      for (int t = 0; t < n; ++t) acc[b] += k[t] * (int)px[t * C];
    }
    store4(out + q * 4, acc, count - q * 4);
  }
}

// src: rows row_lo .. row_lo + src_rows - 1 of the input (the intermediate image starts at the first row the pass reads)
// -> output row blockIdx.y of frame blockIdx.z.  VEC: src, src_frame and src_pitch are multiples of 4.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) resample_v_kernel(const uint8_t *__restrict__ src, int64_t src_frame, int64_t src_pitch, int src_rows,
                                                            int row_lo, uint8_t *__restrict__ dst, int64_t dst_frame, int row_bytes,
                                                            const int32_t *__restrict__ bounds, const int32_t *__restrict__ kk, int ksize) {
  constexpr int kPer = VEC ? 4 : 1;
  const int y = blockIdx.y;
  const int ymin = bounds[2 * y] - row_lo;
  int n = bounds[2 * y + 1];
  if (n > ksize || ymin < 0 || ymin + n > src_rows) n = 0;  // (a table of other sizes)
  const int32_t *k = kk + (int64_t)y * ksize;
  const int j = (blockIdx.x * kBlock + threadIdx.x) * kPer;
  if (j >= row_bytes) return;
  const uint8_t *col = src + blockIdx.z * src_frame + (int64_t)ymin * src_pitch + j;
  int acc[4] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
  for (int t = 0; t < n; ++t) {
    const int kt = k[t];
    if (VEC) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(col + (int64_t)t * src_pitch);  // (the pitch covers j + 3)
      acc[0] += kt * (int)(w & 0xffu);
      acc[1] += kt * (int)((w >> 8) & 0xffu);
      acc[2] += kt * (int)((w >> 16) & 0xffu);
      acc[3] += kt * (int)(w >> 24);
    } else {
      acc[0] += kt * (int)col[(int64_t)t * src_pitch];
    }
  }
  uint8_t *out = dst + blockIdx.z * dst_frame + (int64_t)y * row_bytes + j;
  store4(out, acc, VEC ? row_bytes - j : 1);
}

__global__ void __launch_bounds__(kBlock) resample_copy_kernel(const uint8_t *__restrict__ src, int64_t src_frame, uint8_t *__restrict__ dst,
                                                               int64_t dst_frame, int64_t frame_bytes) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < frame_bytes) dst[blockIdx.y * dst_frame + i] = src[blockIdx.y * src_frame + i];
}

struct Shape {
  int n, h_in, w_in, c, h_out, w_out, filter;
  bool horizontal() const { return w_in != w_out; }
  bool vertical() const { return h_in != h_out; }
  // the input rows the vertical pass reads: those of its first and of its last output row
  void rows(int *lo, int *count) const {
    if (!vertical()) {
      *lo = 0, *count = h_in;
      return;
    }
    const AxisPlan a = axis_plan(h_in, h_out, filter);
    int xmin, n, last, last_n;
    double center;
    axis_bounds(a, h_in, 0, &xmin, &n, &center);
    axis_bounds(a, h_in, h_out - 1, &last, &last_n, &center);
    *lo = xmin, *count = last + last_n - xmin;
  }
  int64_t tmp_pitch() const { return align_up((int64_t)w_out * c, 4); }
};

int check_shape(const char *what, const Shape &s) {
  PGDVS_REQUIRE(s.n >= 1 && s.n <= 65535 && (s.c == 1 || s.c == 3), "%s: %d frames of %d channels (1 .. 65535 frames, 1 or 3 channels)", what,
                s.n, s.c);
  if (int rc = check_axis(what, s.w_in, s.w_out, s.filter)) return rc;
  return check_axis(what, s.h_in, s.h_out, s.filter);
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_resample_table(int in_size, int out_size, int filter, int32_t *bounds, int32_t *kk) {
  if (check_axis("pgdvs_resample_table", in_size, out_size, filter)) return -1;
  const AxisPlan a = axis_plan(in_size, out_size, filter);
  if (!bounds && !kk) return a.ksize;
  if (!bounds || !kk) {
    set_error("pgdvs_resample_table: bounds and kk go together (%s is NULL)", bounds ? "kk" : "bounds");
    return -1;
  }
  double (*const f)(double) = filter == PGDVS_RESAMPLE_BOX ? box_filter : lanczos_filter;
  double w[kMaxTaps];
  const double ss = 1.0 / a.filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    int xmin, n;
    double center, ww = 0.0;
    axis_bounds(a, in_size, xx, &xmin, &n, &center);
    for (int x = 0; x < n; ++x) {
      w[x] = f((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t *k = kk + (int64_t)xx * a.ksize;
    for (int x = 0; x < a.ksize; ++x) {
      if (x >= n) {
        k[x] = 0;
        continue;
      }
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << kPrecisionBits)) : (int)(0.5 + w[x] * (1 << kPrecisionBits));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return a.ksize;
}

PGDVS_API int64_t pgdvs_resample_u8_workspace_bytes(int N, int Hin, int Win, int C, int Hout, int Wout, int filter) {
  const Shape s{N, Hin, Win, C, Hout, Wout, filter};
  if (check_shape("pgdvs_resample_u8_workspace_bytes", s)) return -1;
  if (!s.horizontal() || !s.vertical()) return 0;
  int lo, count;
  s.rows(&lo, &count);
  return (int64_t)N * count * s.tmp_pitch();
}

PGDVS_API int pgdvs_resample_u8(const uint8_t *in, int64_t in_stride, int N, int Hin, int Win, int C, uint8_t *out, int64_t out_stride,
                                int Hout, int Wout, int filter, const int32_t *bounds_h, const int32_t *kk_h, const int32_t *bounds_v,
                                const int32_t *kk_v, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  const Shape s{N, Hin, Win, C, Hout, Wout, filter};
  if (int rc = check_shape("pgdvs_resample_u8", s)) return rc;
  PGDVS_REQUIRE(in && out, "pgdvs_resample_u8: null pointer");
  const int64_t in_pitch = (int64_t)Win * C, out_pitch = (int64_t)Wout * C;
  PGDVS_REQUIRE(in_stride >= Hin * in_pitch && out_stride >= Hout * out_pitch,
                "pgdvs_resample_u8: frames %lld and %lld bytes apart, an input frame has %lld bytes, an output frame %lld", (long long)in_stride,
                (long long)out_stride, (long long)(Hin * in_pitch), (long long)(Hout * out_pitch));
  PGDVS_REQUIRE((!s.horizontal() || (bounds_h && kk_h)) && (!s.vertical() || (bounds_v && kk_v)),
                "pgdvs_resample_u8: an axis that changes needs its table (horizontal %d -> %d, vertical %d -> %d)", Win, Wout, Hin, Hout);
  const hipStream_t st = as_stream(stream);
  if (!s.horizontal() && !s.vertical()) {
    const int64_t frame = Hin * in_pitch;
    PGDVS_LAUNCH("resample_copy", resample_copy_kernel, dim3((unsigned)cdiv(frame, kBlock), (unsigned)N), dim3(kBlock), 0, st, in, in_stride,
                 out, out_stride, frame);
    return check_launch("pgdvs_resample_u8");
  }
  int row_lo, rows;
  s.rows(&row_lo, &rows);
  const uint8_t *v_src = in;
  int64_t v_frame = in_stride, v_pitch = in_pitch;
  if (s.horizontal()) {
    uint8_t *h_dst = out;
    int64_t h_frame = out_stride, h_pitch = out_pitch;
    if (s.vertical()) {  // into the intermediate image: rows row_lo .. row_lo + rows - 1, the pitch padded to 4
      const int64_t need = pgdvs_resample_u8_workspace_bytes(N, Hin, Win, C, Hout, Wout, filter);
      PGDVS_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                    "pgdvs_resample_u8: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)workspace_bytes, (long long)need);
      h_dst = static_cast<uint8_t *>(workspace);
      h_pitch = s.tmp_pitch();
      h_frame = rows * h_pitch;
      v_src = h_dst, v_frame = h_frame, v_pitch = h_pitch;
    }
    // the widest tile (a multiple of 4 output pixels, at most a block's) whose input span fits the LDS stage
    const AxisPlan a = axis_plan(Win, Wout, filter);
    const int budget = kLdsBytes / C;
    int tx = kBlock;
    while (tx > 4 && (int64_t)ceil((tx - 1) * a.scale) + a.ksize + 2 > budget) tx -= 4;
    const dim3 grid((unsigned)cdiv(Wout, tx), (unsigned)rows, (unsigned)N);
    if (C == 1)
      PGDVS_LAUNCH("resample_h", resample_h_kernel<1>, grid, dim3(kBlock), 0, st, in, in_stride, in_pitch, s.vertical() ? row_lo : 0, h_dst,
                   h_frame, h_pitch, Win, Wout, tx, bounds_h, kk_h, a.ksize);
    else
      PGDVS_LAUNCH("resample_h", resample_h_kernel<3>, grid, dim3(kBlock), 0, st, in, in_stride, in_pitch, s.vertical() ? row_lo : 0, h_dst,
                   h_frame, h_pitch, Win, Wout, tx, bounds_h, kk_h, a.ksize);
    if (int rc = check_launch("pgdvs_resample_u8")) return rc;
  }
  if (s.vertical()) {
    const int ksize = axis_plan(Hin, Hout, filter).ksize;
    const int row_bytes = (int)out_pitch;
    const int v_rows = s.horizontal() ? rows : Hin, v_lo = s.horizontal() ? row_lo : 0;
    const bool vec = (reinterpret_cast<uintptr_t>(v_src) & 3) == 0 && v_frame % 4 == 0 && v_pitch % 4 == 0;
    if (vec)
      PGDVS_LAUNCH("resample_v", resample_v_kernel<true>, dim3((unsigned)cdiv(cdiv(row_bytes, 4), kBlock), (unsigned)Hout, (unsigned)N),
                   dim3(kBlock), 0, st, v_src, v_frame, v_pitch, v_rows, v_lo, out, out_stride, row_bytes, bounds_v, kk_v, ksize);
    else
      PGDVS_LAUNCH("resample_v", resample_v_kernel<false>, dim3((unsigned)cdiv(row_bytes, kBlock), (unsigned)Hout, (unsigned)N), dim3(kBlock),
                   0, st, v_src, v_frame, v_pitch, v_rows, v_lo, out, out_stride, row_bytes, bounds_v, kk_v, ksize);
  }
  return check_launch("pgdvs_resample_u8");
}
