// SURVEY 8f visualiser export: one pass from the renderer's planar float image to ready-to-deflate PNG scanlines
// (pgdvs/engines/visualizer_pgdvs.py:118-139: torchvision.utils.save_image for *_combined.png, a numpy cast for *_gnt.png).
//
// One workgroup per output row.  The row and the row above it are quantised from the input into LDS as interleaved RGB
// bytes (the row above is re-quantised, not read back from the output, so rows are independent; every input row is read
// twice, once as "current" and once as "above", the second time from the cache).  The scanline -- the filter-type byte
// followed by 3 W filtered bytes -- is then walked in 4-byte groups aligned to the OUTPUT address: a group's seven
// neighbouring bytes of either row come from three aligned LDS words and a byte alignment, full groups leave as one
// dword store, and only the partial groups at the head and the tail of a row are stored byte by byte (rows are 1 + 3 W
// bytes long, so they start at every alignment).
//
// adaptive: pass 1 sums, for the five PNG filter types, libpng's default cost of the filtered row (sum of v < 128 ? v :
// 256 - v); integer sums, reduced over the wavefront by shuffles and over the block through LDS, so the choice (least
// cost, lowest type on a tie) does not depend on the reduction order.  Pass 2 filters with the chosen type and stores.
// Rows wider than kChunk pixels are staged chunk by chunk (with a one-pixel halo) and staged again for pass 2; up to
// kChunk pixels the row pair stays in LDS between the passes.
//
// Quantisation: clamp(0, 1) first; NaN -> 0 (upstream's NaN-to-uint8 cast is undefined behaviour).
//   quant 0  x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): multiply and add rounded separately (no fma), truncation
//   quant 1  (x * 255).astype(uint8): truncation
//
// Evaluator export (pgdvs/engines/evaluator_pgdvs.py:417-465, save_vis_for_eval): the same row pass over the two or three
// images of a view in ONE launch -- ground truth, prediction and, given, the static render, all with quant 1 (upstream's
// quantise / 255 * 255 / cast chain is the truncating cast of the clamped raw image for every one of the 256 levels).  The
// ground truth is channel-last: a row of it is already in PNG byte order, so it is staged with contiguous 16-byte loads
// (stage_row<kHwc>) instead of three plane reads; everything behind the staging is scanline_row, shared with the
// visualiser's kernel.
//
// Flow pictures (pgdvs/preprocess/common.py:93-205 flow_to_image, called at compute_flow.py:354-361): a third staging,
// stage_row<kFlow>, computes a row's Middlebury colour-wheel bytes from the flow itself instead of quantising an image; the
// scanlines of both pictures of a pair leave in one launch (flow_pictures_kernel, the second pass of
// pgdvs_flow_pair_export; the first, in flow_export.hip, left the radius maximum as per-block keys).
#include "common.h"
#include "flow_pixel.h"
#include "quant8.h"
#include "wave.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 2048;                     // pixels of a row held in LDS at a time
constexpr int kLead = 8;                         // bytes in front of a chunk's first pixel: 5 unused, 3 of the pixel to its left
constexpr int kWords = (kLead + 3 * kChunk + 8) / 4;  // + 8 bytes behind the last pixel that a tail group may read (never use)

constexpr int kPlanar = 0;  // [3,H,W]: a row is three plane rows of W floats
constexpr int kHwc = 1;     // [H,W,3]: a row is 3 W contiguous floats, already in PNG byte order
constexpr int kFlow = 2;    // flow[H,W,2]: a row is W (u, v) pairs, coloured by flow_colour

struct Params {
  const float *img;  // [B,3,H,W] (kPlanar) or [H,W,3] (kHwc)
  uint8_t *out;      // [B,H,1+3W]
  int H, W;
  int quant, adaptive;
  int vec4;          // W % 4 == 0 and img 16-byte aligned: float4 loads
  float denom;       // kFlow: float32(rad_max + float32(1e-5)), what upstream divides u and v by
};

// The Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow", ICCV 2007): six
// segments of 15, 6, 4, 11, 13 and 6 entries, red -> yellow -> green -> cyan -> blue -> magenta -> red; along a segment one
// channel ramps by floor(255 j / length), up or down, one stays 255 and one 0.  Held as entry / 255 in double, the value
// upstream's tmp[k] / 255.0 has (one correctly rounded division either way).
constexpr int kWheelN = 55;
struct Wheel {
  double v[kWheelN][3];
};
constexpr Wheel make_wheel() {
  constexpr int len[6] = {15, 6, 4, 11, 13, 6};
  constexpr int full[6] = {0, 1, 1, 2, 2, 0};  // the channel at 255
  constexpr int ramp[6] = {1, 0, 2, 1, 0, 2};  // the channel that ramps, up in the even segments and down in the odd ones
  Wheel w{};
  int k = 0;
  for (int s = 0; s < 6; ++s)
    for (int j = 0; j < len[s]; ++j, ++k) {
      const int r = 255 * j / len[s];
      for (int c = 0; c < 3; ++c) w.v[k][c] = 0.0;
      w.v[k][full[s]] = 255.0 / 255.0;
      w.v[k][ramp[s]] = (double)(s % 2 == 0 ? r : 255 - r) / 255.0;
    }
  return w;
}
__device__ const Wheel kWheel = make_wheel();

// One pixel of flow_to_image as R | G << 8 | B << 16, upstream's types under NumPy 2: the normalisation, the radius, the angle
// and fk in float32, every operation rounded on its own; from the interpolation on in double (the wheel table is float64).
// A NaN in the normalised u or v gives 0 0 0; the table index is clamped, so no flow value becomes an address.
__device__ __forceinline__ uint32_t flow_colour(float2 f, float denom) {
  const float u = f.x / denom, v = f.y / denom;
  if (!(u == u) || !(v == v)) return 0u;
  const float rad = sqrtf(u * u + v * v);
  const float a = atan2f(-v, -u) / 3.14159274101257324f;
  const float fk = (a + 1.0f) / 2.0f * (float)(kWheelN - 1);
  const float k0f = floorf(fk);
  const int k0 = k0f >= 0.0f ? (k0f <= (float)(kWheelN - 1) ? (int)k0f : kWheelN - 1) : 0;  // (a NaN lands on 0)
  const int k1 = k0 + 1 == kWheelN ? 0 : k0 + 1;
  const double fr = (double)fk - (double)k0;
  uint32_t rgb = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double col = (1.0 - fr) * kWheel.v[k0][c] + fr * kWheel.v[k1][c];
    col = rad <= 1.0f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
    const double b = floor(255.0 * col);
    rgb |= (uint32_t)(int)fmin(fmax(b, 0.0), 255.0) << (8 * c);
  }
  return rgb;
}

// quant: 0 save_image, 1 truncate (quant8.h)
__device__ __forceinline__ uint32_t quantise(float x, int quant) { return quantise8(x, quant == 0); }

// Stage pixels [c0, c0 + n) of an image row (kPlanar: plane 0 of it at `src`; kHwc, kFlow: its first float at `src`) into `dst`: pixel
// c0 + i at bytes kLead + 3 i, the pixel to the left of c0 (zero for c0 = 0) at bytes 5..7.  zero: the row above row 0.
template <int L>
__device__ void stage_row(const Params &p, const float *__restrict__ src, bool zero, int c0, int n, uint32_t *__restrict__ dst) {
  if (L == kHwc) {
    // float 3 c0 + f of the row -> LDS byte kLead + f: one 16-byte load and one LDS word per thread and step
    const float *__restrict__ row = src + 3 * (size_t)c0;
    const int n_bytes = 3 * n, words = (n_bytes + 3) >> 2;
    for (int q = threadIdx.x; q < words; q += kBlock) {
      uint32_t v[4];
      if (zero) {
        v[0] = v[1] = v[2] = v[3] = 0u;
      } else if (p.vec4) {  // (W % 4 == 0: 3 n is a multiple of 4, no read past the chunk)
        const float4 f = *reinterpret_cast<const float4 *>(row + 4 * q);
        v[0] = quantise(f.x, p.quant);
        v[1] = quantise(f.y, p.quant);
        v[2] = quantise(f.z, p.quant);
        v[3] = quantise(f.w, p.quant);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = 4 * q + i < n_bytes ? quantise(row[4 * q + i], p.quant) : 0u;
      }
      dst[kLead / 4 + q] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    }
    if (threadIdx.x == kBlock - 1) {
      uint32_t halo = 0u;
      if (!zero && c0 > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) halo |= quantise(row[c - 3], p.quant) << (8 * (c + 1));
      }
      dst[0] = 0u;
      dst[1] = halo;
    }
    return;
  }
  const int quads = (n + 3) >> 2;
  if (L == kFlow) {
    // four pixels, twelve bytes, three LDS words per thread and step, as the planar staging below
    const float2 *__restrict__ row = reinterpret_cast<const float2 *>(src) + c0;
    for (int q = threadIdx.x; q < quads; q += kBlock) {
      uint32_t c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = (!zero && 4 * q + i < n) ? flow_colour(row[4 * q + i], p.denom) : 0u;
      uint32_t *w = dst + kLead / 4 + 3 * q;
      w[0] = c[0] | (c[1] << 24);
      w[1] = (c[1] >> 8) | (c[2] << 16);
      w[2] = (c[2] >> 16) | (c[3] << 8);
    }
    if (threadIdx.x == kBlock - 1) {
      dst[0] = 0u;
      dst[1] = (!zero && c0 > 0) ? flow_colour(row[-1], p.denom) << 8 : 0u;
    }
    return;
  }
  const size_t plane = (size_t)p.H * p.W;
  for (int q = threadIdx.x; q < quads; q += kBlock) {
    uint32_t v[12];
    if (zero) {
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = 0u;
    } else if (p.vec4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 f = *reinterpret_cast<const float4 *>(src + c * plane + c0 + 4 * q);
        v[c] = quantise(f.x, p.quant);
        v[3 + c] = quantise(f.y, p.quant);
        v[6 + c] = quantise(f.z, p.quant);
        v[9 + c] = quantise(f.w, p.quant);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = 4 * q + i < n;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * i + c] = in ? quantise(src[c * plane + c0 + 4 * q + i], p.quant) : 0u;
      }
    }
    uint32_t *w = dst + kLead / 4 + 3 * q;
    w[0] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    w[1] = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
    w[2] = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
  }
  if (threadIdx.x == kBlock - 1) {
    uint32_t halo = 0u;
    if (!zero && c0 > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) halo |= quantise(src[c * plane + c0 - 1], p.quant) << (8 * (c + 1));
    }
    dst[0] = 0u;
    dst[1] = halo;
  }
}

// bytes [off - 3, off + 4] of an LDS row (off >= 3): a = bytes off-3 .. off (the left neighbours), x = bytes off .. off+3
__device__ __forceinline__ void window(const uint32_t *__restrict__ row, int off, uint32_t &a, uint32_t &x) {
  const int lo = off - 3, w = lo >> 2;
  const uint32_t s = (uint32_t)(lo & 3);
  const uint32_t w0 = row[w], w1 = row[w + 1], w2 = row[w + 2];
  a = __builtin_amdgcn_alignbyte(w1, w0, s);
  const uint32_t hi = __builtin_amdgcn_alignbyte(w2, w1, s);
  x = __builtin_amdgcn_alignbyte(hi, a, 3u);
}

template <int T>
__device__ __forceinline__ uint32_t filter_byte(int x, int a, int b, int c) {
  int pred;
  if (T == 0) {
    pred = 0;
  } else if (T == 1) {
    pred = a;
  } else if (T == 2) {
    pred = b;
  } else if (T == 3) {
    pred = (a + b) >> 1;
  } else {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (uint32_t)(x - pred) & 255u;
}

template <int T>
__device__ __forceinline__ uint32_t filter_word(uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    r |= filter_byte<T>((x >> (8 * j)) & 255, (a >> (8 * j)) & 255, (b >> (8 * j)) & 255, (c >> (8 * j)) & 255) << (8 * j);
  return r;
}

__device__ __forceinline__ uint32_t filter_word_dyn(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  switch (type) {  // (uniform over the block)
    case 1: return filter_word<1>(x, a, b, c);
    case 2: return filter_word<2>(x, a, b, c);
    case 3: return filter_word<3>(x, a, b, c);
    case 4: return filter_word<4>(x, a, b, c);
    default: return x;
  }
}

// libpng's default heuristic over the bytes of `f` selected by `mask` (0xff per selected byte)
__device__ __forceinline__ uint32_t cost_word(uint32_t f, uint32_t mask) {
  uint32_t s = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t v = (f >> (8 * j)) & 255u;
    s += ((mask >> (8 * j)) & 1u) ? (v < 128u ? v : 256u - v) : 0u;
  }
  return s;
}

// The 4-byte groups, aligned to the output address, that hold a chunk's part of the scanline.  Coordinates are relative to the
// chunk: u = t - 3 c0 for scanline byte t (t = 0 is the filter type, t >= 1 is filtered image byte t - 1), so that every index
// stays small however wide the row is.  Byte u lies at LDS byte u + kLead - 1 and at out + u; the chunk owns u in
// [u_lo, u_hi); group g starts at u = 4 g - mis (mis = the address of out mod 4).
struct Groups {
  uint8_t *out;
  int g_lo, g_hi, mis, u_lo, u_hi;
};

__device__ __forceinline__ Groups groups_of(uint8_t *out_row, int c0, int n) {
  Groups g;
  g.out = out_row + 3 * (size_t)c0;
  g.mis = (int)(reinterpret_cast<uintptr_t>(g.out) & 3);
  g.u_lo = c0 == 0 ? 0 : 1;
  g.u_hi = 1 + 3 * n;
  g.g_lo = (g.mis + g.u_lo) >> 2;
  g.g_hi = (g.mis + g.u_hi - 1) >> 2;
  return g;
}

// a workgroup's LDS (at namespace scope, so that a kernel that instantiates both layouts holds it once)
__shared__ uint32_t s_cur[kWords];
__shared__ uint32_t s_up[kWords];
__shared__ unsigned long long s_cost[kBlock / kWave][5];
__shared__ int s_type;

// One scanline by one workgroup: row y of an image in layout L (`cur`: plane 0 of the row / its first float) -> out_row[1 + 3 W]
template <int L>
__device__ __forceinline__ void scanline_row(const Params &p, const float *__restrict__ cur, int y, uint8_t *__restrict__ out_row) {
  const int W = p.W;
  const float *up = y > 0 ? cur - (L == kHwc ? 3 * W : L == kFlow ? 2 * W : W) : cur;  // (row 0 has zeros above it: stage_row's `zero`)
  const int n_chunks = (W + kChunk - 1) / kChunk;
  int type = 0;

  if (p.adaptive) {
    uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int c0 = ch * kChunk, n = min(kChunk, W - c0);
      if (ch > 0) __syncthreads();
      stage_row<L>(p, cur, false, c0, n, s_cur);
      stage_row<L>(p, up, y == 0, c0, n, s_up);
      __syncthreads();
      const Groups g = groups_of(out_row, c0, n);
      for (int gi = g.g_lo + (int)threadIdx.x; gi <= g.g_hi; gi += kBlock) {
        const int u0 = 4 * gi - g.mis;
        uint32_t mask = 0u;  // (u = 1 is the chunk's first image byte: the type byte of chunk 0 costs nothing)
#pragma unroll
        for (int j = 0; j < 4; ++j) mask |= (u0 + j >= 1 && u0 + j < g.u_hi) ? (0xffu << (8 * j)) : 0u;
        uint32_t x, a, bb, c;
        window(s_cur, u0 + kLead - 1, a, x);
        window(s_up, u0 + kLead - 1, c, bb);
        cost[0] += cost_word(x, mask);
        cost[1] += cost_word(filter_word<1>(x, a, bb, c), mask);
        cost[2] += cost_word(filter_word<2>(x, a, bb, c), mask);
        cost[3] += cost_word(filter_word<3>(x, a, bb, c), mask);
        cost[4] += cost_word(filter_word<4>(x, a, bb, c), mask);
      }
    }
    // a thread's sum is at most 128 * 4 * ceil(groups / 256) < 2^31; the block's needs 64 bits for very wide rows
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const unsigned long long v = wave_sum_down((unsigned long long)cost[f]);
      if ((threadIdx.x & (kWave - 1)) == 0) s_cost[threadIdx.x / kWave][f] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int best = 0;
      unsigned long long best_cost = ~0ull;
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) v += s_cost[w][f];
        if (v < best_cost) {
          best_cost = v;
          best = f;
        }
      }
      s_type = best;
    }
    __syncthreads();
    type = s_type;
  }

  for (int ch = 0; ch < n_chunks; ++ch) {
    const int c0 = ch * kChunk, n = min(kChunk, W - c0);
    if (!p.adaptive || n_chunks > 1) {  // (otherwise the row pair is still staged)
      if (ch > 0) __syncthreads();
      stage_row<L>(p, cur, false, c0, n, s_cur);
      if (type >= 2) stage_row<L>(p, up, y == 0, c0, n, s_up);
      __syncthreads();
    }
    const Groups g = groups_of(out_row, c0, n);
    for (int gi = g.g_lo + (int)threadIdx.x; gi <= g.g_hi; gi += kBlock) {
      const int u0 = 4 * gi - g.mis;
      uint32_t x, a, bb = 0u, c = 0u;
      window(s_cur, u0 + kLead - 1, a, x);
      if (type >= 2) window(s_up, u0 + kLead - 1, c, bb);
      uint32_t f = filter_word_dyn(type, x, a, bb, c);
      if (c0 == 0 && u0 <= 0) f = (f & ~(0xffu << (8 * -u0))) | ((uint32_t)type << (8 * -u0));  // the filter-type byte
      if (u0 >= g.u_lo && u0 + 4 <= g.u_hi) {
        *reinterpret_cast<uint32_t *>(g.out + u0) = f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (u0 + j >= g.u_lo && u0 + j < g.u_hi) g.out[u0 + j] = (uint8_t)(f >> (8 * j));
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock) png_scanlines_kernel(Params p) {
  const int H = p.H;
  const int b = blockIdx.x / H, y = blockIdx.x - b * H;
  scanline_row<kPlanar>(p, p.img + ((size_t)b * 3 * H + y) * p.W, y, p.out + (size_t)blockIdx.x * (1 + 3 * (size_t)p.W));
}

struct ExportParams {
  const float *gt;      // [H,W,3]
  const float *planar[2];  // pred, static (or null): [3,H,W]
  uint8_t *out;         // [n,H,1+3W]: gt, pred, static
  int H, W, adaptive;
  int vec4_gt, vec4_planar[2];
};

// image = blockIdx.x / H: 0 the channel-last ground truth, 1 the prediction, 2 the static render (block-uniform branch)
__global__ void __launch_bounds__(kBlock) eval_export_scanlines_kernel(ExportParams e) {
  const int H = e.H, W = e.W;
  const int img = blockIdx.x / H, y = blockIdx.x - img * H;
  Params p;
  p.out = e.out;
  p.H = H;
  p.W = W;
  p.quant = 1;
  p.adaptive = e.adaptive;
  uint8_t *out_row = e.out + (size_t)blockIdx.x * (1 + 3 * (size_t)W);
  if (img == 0) {
    p.img = e.gt;
    p.vec4 = e.vec4_gt;
    scanline_row<kHwc>(p, e.gt + (size_t)y * 3 * W, y, out_row);
  } else {
    p.img = img == 1 ? e.planar[0] : e.planar[1];
    p.vec4 = img == 1 ? e.vec4_planar[0] : e.vec4_planar[1];
    scanline_row<kPlanar>(p, p.img + (size_t)y * W, y, out_row);
  }
}

struct FlowPicParams {
  const float *flow[2];  // [H,W,2] each (one or two pictures: the grid says)
  const uint32_t *keys;  // [n_img][n_keys] radius keys of the first pass (flow_pixel.h)
  float *rad_max;        // [n_img]
  uint8_t *out;          // [n_img,H,1+3W]
  int n_keys, H, W, adaptive;
};

// picture = blockIdx.x / H.  Every row's workgroup reduces the picture's keys itself (a few KB from the cache) rather than
// wait for a launch that would do it once; integer maxima, so every workgroup holds the same bits.
__global__ void __launch_bounds__(kBlock) flow_pictures_kernel(FlowPicParams e) {
  __shared__ uint32_t s_key[kBlock / kWave];
  const int H = e.H, W = e.W;
  const int img = blockIdx.x / H, y = blockIdx.x - img * H;
  uint32_t key = 0u;
  for (int i = threadIdx.x; i < e.n_keys; i += kBlock) key = max(key, e.keys[(size_t)img * e.n_keys + i]);
  key = wave_reduce_all<OpMax>(key);
  if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
  __syncthreads();
  key = s_key[0];
#pragma unroll
  for (int w = 1; w < kBlock / kWave; ++w) key = max(key, s_key[w]);
  const float rad_max = rad_of_key(key);
  if (y == 0 && threadIdx.x == 0) e.rad_max[img] = rad_max;
  Params p;
  p.img = e.flow[img];
  p.out = e.out;
  p.H = H;
  p.W = W;
  p.quant = 0;
  p.adaptive = e.adaptive;
  p.vec4 = 0;
  p.denom = rad_max + 1e-5f;
  scanline_row<kFlow>(p, p.img + (size_t)y * 2 * W, y, e.out + (size_t)blockIdx.x * (1 + 3 * (size_t)W));
}

}  // namespace

int launch_flow_pictures(const float *flow12, const float *flow21, int n_img, int H, int W, int adaptive, const uint32_t *keys, int n_keys,
                         float *rad_max, uint8_t *out, hipStream_t stream) {
  FlowPicParams e;
  e.flow[0] = flow12;
  e.flow[1] = flow21;
  e.keys = keys;
  e.rad_max = rad_max;
  e.out = out;
  e.n_keys = n_keys;
  e.H = H;
  e.W = W;
  e.adaptive = adaptive;
  PGDVS_LAUNCH("flow_pictures", flow_pictures_kernel, dim3((unsigned)(n_img * H)), dim3(kBlock), 0, stream, e);
  return check_launch("pgdvs_flow_pair_export");
}

}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_png_scanlines(const float *img_planar, int B, int H, int W, int quant, int adaptive, uint8_t *out,
                                  pgdvs_stream_t stream) {
  PGDVS_REQUIRE(img_planar && out, "pgdvs_png_scanlines: null pointer");
  PGDVS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * (1 + 3 * (int64_t)W) < (1ll << 31),
                "pgdvs_png_scanlines: bad shape B=%d H=%d W=%d (each >= 1, B H (1 + 3 W) < 2^31)", B, H, W);
  PGDVS_REQUIRE((quant == 0 || quant == 1) && (adaptive == 0 || adaptive == 1),
                "pgdvs_png_scanlines: quant %d (0 save_image, 1 truncate), adaptive %d (0 / 1)", quant, adaptive);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(img_planar) & 3) == 0, "pgdvs_png_scanlines: img_planar is not 4-byte aligned");
  Params p;
  p.img = img_planar;
  p.out = out;
  p.H = H;
  p.W = W;
  p.quant = quant;
  p.adaptive = adaptive;
  p.vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(img_planar) & 15) == 0;
  p.denom = 0.0f;
  PGDVS_LAUNCH("png_scanlines", png_scanlines_kernel, dim3((unsigned)(B * H)), dim3(kBlock), 0, as_stream(stream), p);
  return check_launch("pgdvs_png_scanlines");
}

PGDVS_API int pgdvs_eval_export_scanlines(const float *pred_planar, const float *gt_hwc, const float *static_planar, int H, int W,
                                          int adaptive, uint8_t *out, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_planar && gt_hwc && out, "pgdvs_eval_export_scanlines: null pointer");
  const int n = static_planar ? 3 : 2;
  PGDVS_REQUIRE(H >= 1 && W >= 1 && (int64_t)n * H * (1 + 3 * (int64_t)W) < (1ll << 31),
                "pgdvs_eval_export_scanlines: bad shape H=%d W=%d (each >= 1, n H (1 + 3 W) < 2^31 for n = %d images)", H, W, n);
  PGDVS_REQUIRE(adaptive == 0 || adaptive == 1, "pgdvs_eval_export_scanlines: adaptive %d (0 / 1)", adaptive);
  PGDVS_REQUIRE(((reinterpret_cast<uintptr_t>(pred_planar) | reinterpret_cast<uintptr_t>(gt_hwc) |
                  reinterpret_cast<uintptr_t>(static_planar)) & 3) == 0,
                "pgdvs_eval_export_scanlines: an input image is not 4-byte aligned");
  auto vec4 = [W](const float *q) { return (int)((W % 4 == 0) && (reinterpret_cast<uintptr_t>(q) & 15) == 0); };
  ExportParams e;
  e.gt = gt_hwc;
  e.planar[0] = pred_planar;
  e.planar[1] = static_planar;
  e.out = out;
  e.H = H;
  e.W = W;
  e.adaptive = adaptive;
  e.vec4_gt = vec4(gt_hwc);
  e.vec4_planar[0] = vec4(pred_planar);
  e.vec4_planar[1] = static_planar ? vec4(static_planar) : 0;
  PGDVS_LAUNCH("eval_export_scanlines", eval_export_scanlines_kernel, dim3((unsigned)(n * H)), dim3(kBlock), 0, as_stream(stream), e);
  return check_launch("pgdvs_eval_export_scanlines");
}
