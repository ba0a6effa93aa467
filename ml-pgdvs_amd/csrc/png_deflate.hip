// The deflate of the PNG export (pgdvs/engines/visualizer_pgdvs.py:118-139 and evaluator_pgdvs.py:417-465 write their images
// through PIL / torchvision, whose zlib runs on the host): the scanlines csrc/png.hip leaves on the GPU become a zlib stream
// there, so png.PngWriter's workers only wrap and write.  pgdvs_amd/png.py holds the same stream in Python / numpy integers
// (deflate_rle), the kernels follow it byte for byte.
//
// The stream: 0x78 0x01; per segment of seg_bytes input bytes one non-final dynamic-Huffman block and an empty stored block
// (000, pad, 00 00 FF FF), so every segment starts and ends on a byte; one final empty fixed block; the Adler-32.  Tokens are
// zlib's Z_RLE idea at distance 1 only, independent per segment: a run of n equal bytes is a literal, then (n - 1) / 258 matches
// of 258 and, of the r bytes left, one match (r >= 3) or r literals.  A byte's token follows from its run's start and from the
// run's extent over the next 258 bytes alone, so tokenising is two segmented scans.  ONE literal/length code per image, limited
// to 15 bits and complete, repeated in every segment's header; one distance code of length 1; the code-length code is the
// fixed complete code "lengths 0 .. 15 in 4 bits".
//
// pgdvs_png_deflate: three launches, no workgroup waits for another, no global atomics, every loop bound is known at launch.
//   1 deflate_count   one workgroup of 256 threads per (image, segment); a thread owns 16 consecutive bytes of a 4096-byte
//                     window whose last 272 bytes are look-ahead only (kPayload = 3824 bytes of tokens per step).  Histogram of
//                     the tokens in LDS -> workspace; the segment's two Adler sums.
//   2 deflate_table   one workgroup per image: sums the histograms, sorts the used symbols by rank, ONE thread merges the two
//                     queues (at most 285 steps) and repairs the level counts, then lengths, canonical bit-reversed codes and
//                     the header bits in parallel; every segment's exact size from its histogram, scanned into its offset;
//                     the image's length, its first two and last six bytes (or -1 and nothing if out_stride is too small).
//   3 deflate_encode  one workgroup per (image, segment) derives the tokens a second time (nothing is stored between the
//                     launches but the histograms), scans their bit lengths, ORs the codes into an LDS bit buffer and writes
//                     its whole bytes straight to the segment's final place.
#include <limits.h>

#include "common.h"
#include "wave.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
// (tests/test_png_deflate_host.py reads these constants and compares them with ops.PNG_DEFLATE_* and png.DEFLATE_*)
constexpr int kPer = 16;
constexpr int kWindow = kBlock * kPer;
constexpr int kHalo = 272;
constexpr int kPayload = kWindow - kHalo;
constexpr int kMaxMatch = 258;
static_assert(kHalo >= kMaxMatch && kHalo % kPer == 0 && kPer % 4 == 0, "a token's group must end inside the window; a thread reads its bytes as words");

constexpr int kLitLen = 286, kEob = 256, kMaxBits = 15;
constexpr int kHeaderBits = 17 + 3 * 19 + 4 * kLitLen + 4;  // 1222
constexpr int kHeaderWords = (kHeaderBits + 31) / 32;
constexpr int kHeaderStride = 40, kTableStride = 288;
constexpr int kSegOverhead = (kHeaderBits + kMaxBits + 3 + 7) / 8 + 1 + 4;  // 160: png.DEFLATE_SEG_OVERHEAD
constexpr uint32_t kAdler = 65521u;
constexpr uint32_t kNoToken = 0xffffffffu;
// a step's bits at most: the header or a carry, 15 per byte (a literal; a match pays 15 + 5 + 1 for at least 3), the end of block,
// the stored block's 3 bits, the padding and 00 00 FF FF; + the word a code may spill into
constexpr int kBufWords = (kHeaderBits + kMaxBits * kPayload + kMaxBits + 3 + 7 + 32 + 31) / 32 + 2;
constexpr int kSegMin = 4096;
constexpr int kSegMax = 65536;

struct Params {
  const uint8_t *in;  // [n_img][img_bytes]
  int64_t img_bytes;
  int seg_bytes, n_seg;  // per image
  uint32_t *hist;        // [n_img n_seg][kLitLen]
  uint32_t *adler;       // [n_img n_seg][2]
  uint32_t *seg_size;    // [n_img n_seg] bytes of the segment's two blocks
  uint32_t *seg_off;     // [n_img n_seg] their offset in the image's stream
  uint32_t *table;       // [n_img][kTableStride] bit-reversed code | length << 16
  uint32_t *header;      // [n_img][kHeaderStride] the kHeaderBits bits in front of every segment
  uint8_t *out;
  int64_t out_stride;
  int32_t *nbytes;  // [n_img]
};

// a token: symbol | extra bits << 9 | extra value << 13
__device__ __forceinline__ uint32_t length_token(int len) {
  if (len == kMaxMatch) return 285u;
  const int x = len - 3;
  const int e = max(32 - __clz(x) - 3, 0);
  return (uint32_t)(257 + 4 * e + (x >> e)) | ((uint32_t)e << 9) | ((uint32_t)(x & ((1 << e) - 1)) << 13);
}
__device__ __forceinline__ int extra_bits_of(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

struct Bytes {  // a thread's kPer consecutive bytes
  uint32_t w[kPer / 4];
  __device__ __forceinline__ uint32_t operator[](int i) const { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
};
struct Fetched {  // what a thread loads for one step: bytes tid, tid + kBlock, ... of the window, and the byte in front of it
  uint8_t b[kPer];
  uint8_t front;
};
__device__ __forceinline__ void fetch(const uint8_t *__restrict__ seg, const int L, const int base, Fetched &f) {
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int pos = base + (int)threadIdx.x + k * kBlock;
    f.b[k] = pos < L ? seg[pos] : (uint8_t)0;
  }
  f.front = (threadIdx.x == 0 && base > 0) ? seg[base - 1] : (uint8_t)0;
}

struct TokenLds {
  __attribute__((aligned(16))) uint8_t in[kPer + kWindow];  // in[kPer + w]: byte w of the window; in[kPer - 1]: the byte in front
  int wmax[kWaves], wmin[kWaves];
  int carry;  // where the run of the last token byte of the step before began
};

// One step over the segment's bytes [0, L): the window starts at byte `base` (a multiple of kPayload) and `f` holds what
// fetch() loaded for it (the callers fetch the next step's bytes before they work on this one's).  Every thread of the block
// calls it (two barriers).  tok[i]: the token that begins at byte base + kPer tid + i, kNoToken where none does (inside a
// match, past kPayload, past L); bytes: the thread's 8 bytes.
__device__ __forceinline__ void step_tokens(const Fetched &f, const int L, const int base, TokenLds &s, uint32_t (&tok)[kPer], Bytes &bytes) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
  for (int k = 0; k < kPer; ++k) s.in[kPer + tid + k * kBlock] = f.b[k];
  if (tid == 0) s.in[kPer - 1] = f.front;
  __syncthreads();
  const int carry = base > 0 ? s.carry : -1;
  const int w0 = tid * kPer, p0 = base + w0;
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) bytes.w[k] = reinterpret_cast<const uint32_t *>(&s.in[kPer + w0])[k];
  uint32_t prev = s.in[kPer - 1 + w0];
  unsigned first = 0u;  // bit i: a run begins at byte i (bytes past L count as beginnings: they end the last run)
  int ls = -1, fs = INT_MAX;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const uint32_t b = bytes[i];
    const int pos = p0 + i;
    if (pos >= L || pos == 0 || b != prev) {
      first |= 1u << i;
      ls = pos;
      fs = min(fs, pos);
    }
    prev = b;
  }
  const int up = wave_incl_scan_up<OpMax>(ls), down = wave_incl_scan_down<OpMin>(fs);
  if (lane == kWave - 1) s.wmax[wave] = up;
  if (lane == 0) s.wmin[wave] = down;
  int run_start = __shfl_up(up, 1, kWave), run_end = __shfl_down(down, 1, kWave);
  if (lane == 0) run_start = -1;
  if (lane == kWave - 1) run_end = INT_MAX;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) run_start = max(run_start, s.wmax[w]);
    if (w > wave) run_end = min(run_end, s.wmin[w]);
  }
  run_start = max(run_start, carry);
  run_end = min(run_end, min(base + kWindow, L));  // exact up to 258 bytes past every token byte, which is all a token needs
  int start[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    if ((first >> i) & 1u) run_start = p0 + i;
    start[i] = run_start;
  }
#pragma unroll
  for (int i = kPer - 1; i >= 0; --i) {
    const int pos = p0 + i;
    const uint32_t b = bytes[i];
    uint32_t t = kNoToken;
    if (w0 + i < kPayload && pos < L) {
      const int k = pos - start[i];
      if (k == 0) {
        t = b;
      } else {
        const int g = (k - 1) / kMaxMatch, r = (k - 1) - g * kMaxMatch;
        const int len = min(kMaxMatch, run_end - (start[i] + 1 + kMaxMatch * g));  // the bytes of this byte's group
        if (len < 3) t = b;
        else if (r == 0) t = length_token(len);
      }
    }
    tok[i] = t;
    if (w0 + i == kPayload - 1) s.carry = start[i];
    if ((first >> i) & 1u) run_end = pos;
  }
}

struct Where {
  int img, blk, L;
  const uint8_t *seg;
};
__device__ __forceinline__ Where locate(const Params &p) {
  Where w;
  w.blk = blockIdx.x;
  w.img = w.blk / p.n_seg;
  const int sg = w.blk - w.img * p.n_seg;
  const int64_t seg0 = (int64_t)sg * p.seg_bytes;
  const int64_t left = p.img_bytes - seg0;
  w.L = (int)(left < p.seg_bytes ? left : p.seg_bytes);
  w.seg = p.in + (size_t)w.img * p.img_bytes + seg0;
  return w;
}

__global__ void __launch_bounds__(kBlock) deflate_count_kernel(Params p) {
  __shared__ TokenLds s;
  __shared__ uint32_t s_hist[kLitLen];
  __shared__ uint32_t s_sum[2][kWaves];
  const int tid = threadIdx.x;
  const Where at = locate(p);
  for (int i = tid; i < kLitLen; i += kBlock) s_hist[i] = i == kEob ? 1u : 0u;  // (the first step's barrier orders this)
  uint32_t a = 0u, b = 0u;  // this thread's part of sum byte and sum (L - i) byte, b reduced every step
  Fetched next;
  fetch(at.seg, at.L, 0, next);
  for (int base = 0; base < at.L; base += kPayload) {
    const Fetched cur = next;
    if (base + kPayload < at.L) fetch(at.seg, at.L, base + kPayload, next);
    uint32_t tok[kPer];
    Bytes bytes;
    step_tokens(cur, at.L, base, s, tok, bytes);
    uint32_t sb = 0u;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if (tok[i] != kNoToken) atomicAdd(&s_hist[tok[i] & 511u], 1u);
      const int pos = base + tid * kPer + i;
      if (tid * kPer + i < kPayload && pos < at.L) {
        const uint32_t v = bytes[i];
        a += v;
        sb += (uint32_t)(at.L - pos) * v;  // kPer x 65536 x 255 < 2^32
      }
    }
    b = (b + sb % kAdler) % kAdler;
  }
  a = wave_sum_down(a);  // (at most 65536 x 255 in all: far below 2^32)
  b = wave_sum_down(b);
  if ((tid & (kWave - 1)) == 0) {
    s_sum[0][tid / kWave] = a;
    s_sum[1][tid / kWave] = b;
  }
  __syncthreads();
  for (int i = tid; i < kLitLen; i += kBlock) p.hist[(size_t)at.blk * kLitLen + i] = s_hist[i];
  if (tid < 2) {
    uint32_t v = 0u;
    for (int w = 0; w < kWaves; ++w) v += s_sum[tid][w];
    p.adler[(size_t)at.blk * 2 + tid] = v % kAdler;
  }
}

__device__ __forceinline__ void or_bits(uint32_t *buf, int pos, uint32_t value) {  // value of at most 32 bits at stream bit pos
  const uint64_t x = (uint64_t)value << (pos & 31);
  atomicOr(&buf[pos >> 5], (uint32_t)x);
  if ((uint32_t)(x >> 32)) atomicOr(&buf[(pos >> 5) + 1], (uint32_t)(x >> 32));
}
__device__ __forceinline__ uint32_t rev4(uint32_t v) { return __brev(v) >> 28; }

__global__ void __launch_bounds__(kBlock) deflate_table_kernel(Params p) {
  __shared__ uint32_t s_freq[kLitLen], s_w[kLitLen], s_inner[kLitLen];
  __shared__ uint16_t s_sym[kLitLen], s_leaf_parent[kLitLen], s_inner_parent[kLitLen], s_depth[kLitLen];
  __shared__ uint8_t s_len[kLitLen], s_cost[kLitLen];
  __shared__ int s_level[kMaxBits + 1], s_next[kMaxBits + 1];
  __shared__ uint32_t s_header[kHeaderStride];
  __shared__ int s_wsum[kWaves];
  __shared__ uint32_t s_adler[2][kWaves];
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int img = blockIdx.x;
  const size_t seg0 = (size_t)img * p.n_seg;
  const uint32_t *hist = p.hist + seg0 * kLitLen;
  for (int sym = tid; sym < kLitLen; sym += kBlock) {
    uint32_t f = 0u;
#pragma unroll 8
    for (int g = 0; g < p.n_seg; ++g) f += hist[(size_t)g * kLitLen + sym];  // (independent loads: eight in flight)
    s_freq[sym] = f;
    s_len[sym] = 0;
  }
  if (tid <= kMaxBits) s_level[tid] = 0;
  if (tid < kHeaderStride) s_header[tid] = 0u;
  __syncthreads();
  // the used symbols by (count, symbol): every one finds its own rank
  for (int sym = tid; sym < kLitLen; sym += kBlock) {
    const uint32_t f = s_freq[sym];
    if (f == 0u) continue;
    int r = 0;
    for (int o = 0; o < kLitLen; ++o) {
      const uint32_t fo = s_freq[o];
      r += (fo != 0u && (fo < f || (fo == f && o < sym))) ? 1 : 0;
    }
    s_sym[r] = (uint16_t)sym;
    s_w[r] = f;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int o = 0; o < kLitLen; ++o) n += s_freq[o] != 0u ? 1 : 0;  // >= 2: the end of block and a literal
    if (n < 2) n = 0;  // (cannot happen: the count kernel gives every segment an end of block and its first literal)
    s_n = n;
    // two queues, the sorted leaves and the inner nodes in the order they are made; a leaf goes first on equal weights
    int li = 0, ii = 0;
    for (int k = 0; k < n - 1; ++k) {
      uint32_t total = 0u;
      for (int t = 0; t < 2; ++t) {
        if (li < n && (ii >= k || s_w[li] <= s_inner[ii])) {
          total += s_w[li];
          s_leaf_parent[li++] = (uint16_t)k;
        } else {
          total += s_inner[ii];
          s_inner_parent[ii++] = (uint16_t)k;
        }
      }
      s_inner[k] = total;
    }
    if (n >= 2) s_depth[n - 2] = 0;
    for (int k = n - 3; k >= 0; --k) s_depth[k] = (uint16_t)(s_depth[s_inner_parent[k]] + 1);
  }
  __syncthreads();
  const int n = s_n;
  for (int i = tid; i < n; i += kBlock) atomicAdd(&s_level[min((int)s_depth[s_leaf_parent[i]] + 1, kMaxBits)], 1);
  __syncthreads();
  if (tid == 0) {
    // leaves deeper than 15 now sit at 15 and the Kraft sum exceeds 1 by `excess` / 2^15, less than their number: each
    // repair moves the deepest leaf above level 15 one level down, with a level-15 leaf as its sibling, and takes 2^-15 off
    int excess = -(1 << kMaxBits);
    for (int l = 1; l <= kMaxBits; ++l) excess += s_level[l] << (kMaxBits - l);
    for (int it = 0; it < kLitLen && excess > 0; ++it, --excess) {
      int bits = kMaxBits - 1;
      while (bits > 1 && s_level[bits] == 0) --bits;
      s_level[bits] -= 1;
      s_level[bits + 1] += 2;
      s_level[kMaxBits] -= 1;
    }
    int code = 0;
    s_next[0] = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
      code = (code + (l > 1 ? s_level[l - 1] : 0)) << 1;
      s_next[l] = code;
    }
  }
  __syncthreads();
  // levels along the sorted order, the longest to the rarest
  for (int r = tid; r < n; r += kBlock) {
    int c = 0, len = 0;
    for (int l = kMaxBits; l >= 1; --l) {
      c += s_level[l];
      if (len == 0 && r < c) len = l;
    }
    s_len[s_sym[r]] = (uint8_t)len;
  }
  __syncthreads();
  // canonical codes, bit-reversed, and the header's 4 bits per symbol
  for (int sym = tid; sym < kLitLen; sym += kBlock) {
    const int len = s_len[sym];
    uint32_t entry = 0u;
    if (len) {
      uint32_t c = (uint32_t)s_next[len];
      for (int o = 0; o < sym; ++o) c += s_len[o] == len ? 1u : 0u;
      entry = (__brev(c) >> (32 - len)) | ((uint32_t)len << 16);
    }
    p.table[(size_t)img * kTableStride + sym] = entry;
    s_cost[sym] = (uint8_t)(len + extra_bits_of(sym) + (sym > kEob ? 1 : 0));
    or_bits(s_header, 17 + 3 * 19 + 4 * sym, rev4((uint32_t)len));
  }
  if (tid == 0) {
    // BFINAL 0, BTYPE 10, HLIT 29, HDIST 0, HCLEN 15; code-length-code lengths in the order 16 17 18 0 8 7 ...: 0 0 0, then 4s
    or_bits(s_header, 0, (2u << 1) | ((uint32_t)(kLitLen - 257) << 3) | (15u << 13));
    for (int i = 3; i < 19; ++i) or_bits(s_header, 17 + 3 * i, 4u);
    or_bits(s_header, kHeaderBits - 4, rev4(1u));  // the distance code: one code of length 1
  }
  __syncthreads();
  if (tid < kHeaderStride) p.header[(size_t)img * kHeaderStride + tid] = s_header[tid];
  // every segment's size: a wavefront per segment
  for (int g = wave; g < p.n_seg; g += kWaves) {
    uint32_t bits = 0u;
    for (int sym = lane; sym < kLitLen; sym += kWave) bits += hist[(size_t)g * kLitLen + sym] * s_cost[sym];
    bits = wave_sum_all(bits);
    if (lane == 0) p.seg_size[seg0 + g] = ((kHeaderBits + bits + 3u + 7u) >> 3) + 4u;
  }
  __syncthreads();
  int64_t total = 2;
  for (int g0 = 0; g0 < p.n_seg; g0 += kBlock) {
    const int g = g0 + tid;
    const int c = g < p.n_seg ? (int)p.seg_size[seg0 + g] : 0;
    int sum;
    const int off = block_excl_scan<kWaves>(c, s_wsum, sum);
    if (g < p.n_seg) p.seg_off[seg0 + g] = (uint32_t)(total + off);
    total += sum;
    __syncthreads();
  }
  total += 6;
  // Adler-32 of the image from the segments' sums: a = 1 + sum A_g, b = N + sum (B_g + A_g x (bytes behind segment g))
  uint32_t a = 0u, b = 0u;
  for (int g = tid; g < p.n_seg; g += kBlock) {
    const uint32_t ag = p.adler[(seg0 + g) * 2], bg = p.adler[(seg0 + g) * 2 + 1];
    const int64_t end = (int64_t)(g + 1) * p.seg_bytes;
    const uint64_t behind = (uint64_t)(end < p.img_bytes ? p.img_bytes - end : 0) % kAdler;
    a = (a + ag) % kAdler;
    b = (uint32_t)((b + bg + behind * ag) % kAdler);
  }
  a = wave_sum_down(a);
  b = wave_sum_down(b);
  if (lane == 0) {
    s_adler[0][wave] = a;
    s_adler[1][wave] = b;
  }
  __syncthreads();
  if (tid == 0) {
    a = 1u;
    b = (uint32_t)(p.img_bytes % kAdler);
    for (int w = 0; w < kWaves; ++w) {
      a += s_adler[0][w];
      b += s_adler[1][w];
    }
    a %= kAdler;
    b %= kAdler;
    if (total > p.out_stride) {
      p.nbytes[img] = -1;
    } else {
      uint8_t *o = p.out + (size_t)img * p.out_stride;
      o[0] = 0x78;
      o[1] = 0x01;
      uint8_t *t = o + total - 6;
      t[0] = 0x03;  // BFINAL 1, BTYPE 01, the 7-bit end of block
      t[1] = 0x00;
      t[2] = (uint8_t)(b >> 8);
      t[3] = (uint8_t)b;
      t[4] = (uint8_t)(a >> 8);
      t[5] = (uint8_t)a;
      p.nbytes[img] = (int32_t)total;
    }
  }
}

// bits are little-endian throughout, as deflate packs them: bit k of the buffer is bit k & 31 of word k >> 5, byte i of the
// buffer bits 8 (i & 3) .. 8 (i & 3) + 7 of word i >> 2
__global__ void __launch_bounds__(kBlock) deflate_encode_kernel(Params p) {
  __shared__ TokenLds s;
  __shared__ uint32_t s_tab[kLitLen];
  __shared__ uint32_t s_buf[kBufWords];
  __shared__ int s_wsum[kWaves];
  const int tid = threadIdx.x;
  const Where at = locate(p);
  if (p.nbytes[at.img] < 0) return;  // (the whole workgroup: the image does not fit its row)
  uint8_t *dst = p.out + (size_t)at.img * p.out_stride + p.seg_off[at.blk];
  const uint32_t size = p.seg_size[at.blk];
  for (int i = tid; i < kLitLen; i += kBlock) s_tab[i] = p.table[(size_t)at.img * kTableStride + i];
  for (int w = tid; w < kBufWords; w += kBlock) s_buf[w] = w < kHeaderWords ? p.header[(size_t)at.img * kHeaderStride + w] : 0u;
  int pre = kHeaderBits;  // bits the buffer holds already: the header, later the 0 .. 7 bits the step before left over
  uint32_t written = 0u;
  Fetched next;
  fetch(at.seg, at.L, 0, next);
  for (int base = 0; base < at.L; base += kPayload) {
    const Fetched cur = next;
    if (base + kPayload < at.L) fetch(at.seg, at.L, base + kPayload, next);
    uint32_t tok[kPer];
    Bytes bytes;
    step_tokens(cur, at.L, base, s, tok, bytes);  // (its barriers order the buffer's set-up before the ORs below)
    int len = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (tok[i] != kNoToken) len += (int)(s_tab[tok[i] & 511u] >> 16) + (int)((tok[i] >> 9) & 15u) + ((tok[i] & 511u) > (uint32_t)kEob ? 1 : 0);
    int total;
    const int pos0 = pre + block_excl_scan<kWaves>(len, s_wsum, total);
    total += pre;
    if (len) {
      int pos = pos0, w = pos0 >> 5;
      uint32_t cur = 0u;
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        if (tok[i] == kNoToken) continue;
        const uint32_t sym = tok[i] & 511u, t = s_tab[sym];
        const int cl = (int)(t >> 16);
        const uint32_t v = (t & 0xffffu) | ((tok[i] >> 13) << cl);  // (a match's distance bit, 0, lies behind them)
        const int nb = cl + (int)((tok[i] >> 9) & 15u) + (sym > (uint32_t)kEob ? 1 : 0);  // at most 21
        const uint64_t x = (uint64_t)v << (pos & 31);
        cur |= (uint32_t)x;
        pos += nb;
        if ((pos >> 5) != w) {
          atomicOr(&s_buf[w], cur);
          ++w;
          cur = (uint32_t)(x >> 32);
        }
      }
      if (cur) atomicOr(&s_buf[w], cur);
    }
    int n_bits = total;
    if (base + kPayload >= at.L) {  // the last step: end of block, the empty stored block
      const uint32_t eob = s_tab[kEob];
      const int n_byte = (total + (int)(eob >> 16) + 3 + 7) >> 3;
      n_bits = (n_byte + 4) * 8;
      if (tid == 0) {
        or_bits(s_buf, total, eob & 0xffffu);
        or_bits(s_buf, (n_byte + 2) * 8, 0xffffu);
      }
    }
    __syncthreads();
    const int n_bytes = n_bits >> 3;
    const uint32_t carry = (s_buf[n_bytes >> 2] >> (8 * (n_bytes & 3))) & 255u;  // (bits past n_bits are 0)
    for (int i = tid; i < n_bytes; i += kBlock)
      if (written + (uint32_t)i < size) dst[written + (uint32_t)i] = (uint8_t)(s_buf[i >> 2] >> (8 * (i & 3)));  // (size: the table's count; equal by construction)
    written += (uint32_t)n_bytes;
    __syncthreads();
    for (int w = tid; w <= (n_bits >> 5) + 1 && w < kBufWords; w += kBlock) s_buf[w] = w == 0 ? carry : 0u;
    pre = n_bits & 7;
  }
}

struct Shape {
  int64_t n_seg, capacity;
};
bool deflate_shape(int n_img, int64_t img_bytes, int seg_bytes, Shape &s) {
  if (n_img < 1 || img_bytes < 1 || img_bytes > (1ll << 30) || seg_bytes < kSegMin || seg_bytes > kSegMax || (seg_bytes & (seg_bytes - 1))) return false;
  s.n_seg = cdiv(img_bytes, seg_bytes);
  s.capacity = 8 + kSegOverhead * s.n_seg + (15 * img_bytes + 7) / 8;
  return (int64_t)n_img * s.n_seg <= (1ll << 20) && s.capacity < (1ll << 31);
}
constexpr const char *kShapeText = "(n_img >= 1, img_bytes in 1 .. 2^30, seg_bytes a power of two in 4096 .. 65536, n_img x segments <= 2^20)";

struct Workspace {
  uint32_t *hist, *adler, *seg_size, *seg_off, *table, *header;
  int64_t bytes;
  Workspace(void *base, int n_img, const Shape &s) {
    Carver c{static_cast<char *>(base)};
    const int64_t n = (int64_t)n_img * s.n_seg;
    hist = c.take<uint32_t>(n * kLitLen * 4);
    adler = c.take<uint32_t>(n * 2 * 4);
    seg_size = c.take<uint32_t>(n * 4);
    seg_off = c.take<uint32_t>(n * 4);
    table = c.take<uint32_t>((int64_t)n_img * kTableStride * 4);
    header = c.take<uint32_t>((int64_t)n_img * kHeaderStride * 4);
    bytes = c.off;
  }
};

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_png_deflate_workspace_bytes(int n_img, int64_t img_bytes, int seg_bytes) {
  Shape s;
  if (!deflate_shape(n_img, img_bytes, seg_bytes, s)) {
    set_error("pgdvs_png_deflate_workspace_bytes: bad shape n_img=%d img_bytes=%lld seg_bytes=%d %s", n_img, (long long)img_bytes, seg_bytes,
              kShapeText);
    return -1;
  }
  return Workspace(nullptr, n_img, s).bytes;
}

PGDVS_API int pgdvs_png_deflate(const uint8_t *scanlines, int n_img, int64_t img_bytes, int seg_bytes, uint8_t *out, int64_t out_stride,
                                int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(scanlines && out && nbytes && workspace, "pgdvs_png_deflate: null pointer");
  Shape s;
  PGDVS_REQUIRE(deflate_shape(n_img, img_bytes, seg_bytes, s), "pgdvs_png_deflate: bad shape n_img=%d img_bytes=%lld seg_bytes=%d %s", n_img,
                (long long)img_bytes, seg_bytes, kShapeText);
  PGDVS_REQUIRE(out_stride >= 1 && (int64_t)n_img * out_stride < (1ll << 40), "pgdvs_png_deflate: out_stride %lld", (long long)out_stride);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(nbytes) & 3) == 0,
                "pgdvs_png_deflate: workspace must be 256-byte and nbytes 4-byte aligned");
  Workspace ws(workspace, n_img, s);
  PGDVS_REQUIRE(workspace_bytes >= ws.bytes, "pgdvs_png_deflate: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)ws.bytes);
  Params p;
  p.in = scanlines;
  p.img_bytes = img_bytes;
  p.seg_bytes = seg_bytes;
  p.n_seg = (int)s.n_seg;
  p.hist = ws.hist;
  p.adler = ws.adler;
  p.seg_size = ws.seg_size;
  p.seg_off = ws.seg_off;
  p.table = ws.table;
  p.header = ws.header;
  p.out = out;
  p.out_stride = out_stride;
  p.nbytes = nbytes;
  const hipStream_t st = as_stream(stream);
  const unsigned n_blk = (unsigned)(n_img * s.n_seg);
  PGDVS_LAUNCH("deflate_count", deflate_count_kernel, dim3(n_blk), dim3(kBlock), 0, st, p);
  PGDVS_LAUNCH("deflate_table", deflate_table_kernel, dim3((unsigned)n_img), dim3(kBlock), 0, st, p);
  PGDVS_LAUNCH("deflate_encode", deflate_encode_kernel, dim3(n_blk), dim3(kBlock), 0, st, p);
  return check_launch("pgdvs_png_deflate");
}
