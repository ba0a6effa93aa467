// The core of the parallel JPEG scan reader, shared by the device kernels (csrc/jpeg_scan_decode.hip) and their host
// emulation (csrc/jpeg_entropy.cpp: pgdvs_jpeg_scan_prepare, pgdvs_jpeg_scan_decode_host).  Plain C++ and nothing of HIP but
// the __host__ __device__ marks: tools/jpeg_scan_fuzz.cpp builds it with the host compiler and its sanitizers.
//
// The scan is cut into SUBSEQUENCES of a fixed number of bytes inside each restart segment.  decode_sub reads one of them
// from an ENTRY STATE -- bit position, block within the MCU (which selects the component and its DC / AC table), zigzag
// position -- until the position leaves the subsequence, counts the blocks it completes and returns its EXIT STATE: the entry
// of the next one.  A subsequence that begins a segment knows its entry; every other one starts with a guess (block 0, zigzag
// 0 at its first bit) and is decoded again whenever its predecessor's exit turns out to be something else.  The true states
// are the one fixed point of "exit[i] = decode(exit[i - 1])"; a decoder started wrong falls into step with the true one after
// a few symbols, which is why the fixed point is reached after a few rounds and not after as many as there are subsequences.
//
// Two modes, one function: speculative (writes nothing, reports nothing: a bad code, a run past coefficient 63 or a symbol
// that leaves the segment's data ends the subsequence quietly with the one INVALID state, and a subsequence handed that state
// starts from the guess again) and
// verified (the entry is the true one: the coefficients are written, and the same events are reported as long as the block
// they happen in is one the segment owes).  Both return the same exit for the same entry.
//
// Table semantics are jdhuff.c's, as csrc/jpeg_entropy.cpp derives them: a 9-bit look-ahead table in front of maxcode /
// valoffset / huffval.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // (spelled as attributes: csrc/jpeg_entropy.cpp is compiled as HIP without the runtime's header)
#define PGDVS_SCAN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PGDVS_SCAN_HD inline
#endif

namespace pgdvs {
namespace jscan {

constexpr int kLook = 9;
constexpr uint32_t kMagic = 0x314e4353u;  // "SCN1"
constexpr int kSubsPerGroup = 256;        // subsequences of one workgroup: one per thread
constexpr int kMinSubBytes = 16, kMaxSubBytes = 4096;
constexpr int64_t kMaxScanBytes = (int64_t)1 << 25;  // = PGDVS_JPEG_SCAN_MAX_BYTES: bit positions fit 32 bits 8 times over
constexpr int kMaxMcusSide = 2048;                   // 16384 pixels of 8 x 8 blocks at 4:4:4

// the status word (include/pgdvs_hip.h, PGDVS_JPEG_SCAN_*)
constexpr uint32_t kStatusShort = 1, kStatusBadCode = 2, kStatusDcRange = 4, kStatusNotSynchronised = 8, kStatusLeftOver = 16;

struct Table {  // one derived Huffman table
  uint16_t look[1 << kLook];  // (length << 8) | symbol for every 9-bit prefix of a code of up to 9 bits, 0 = longer
  int32_t maxcode[18];        // the largest code of each length, -1 where there is none
  int32_t valoff[17];         // vals index of a code = code + valoff[length]
  int32_t n;                  // symbols
  uint8_t vals[256];
};
constexpr int kTables = 6;  // DC, AC of component 0, then 1, then 2

struct Segment {                  // one restart segment (the whole scan where the file has no restart interval)
  uint32_t bit_begin, bit_end;    // its data in the unstuffed stream
  int32_t mcu_first, mcu_count;   // the MCUs it owes
  int32_t sub_first, sub_count;   // its subsequences: at least one
};

struct Header {  // the front of the prepared buffer; every offset is in bytes from the buffer's start, a multiple of 8
  uint32_t magic;
  int32_t sub_bytes;
  int32_t nseg, nsub;
  int32_t h, v;            // luma sampling factors: an MCU has h * v + 2 blocks
  int32_t mcus_w, mcus_h;
  int32_t restart_mcus;    // MCUs of a segment: the file's restart interval, or every MCU where it has none
  int32_t reserved0;
  int64_t coef_bytes;
  int64_t stream_bytes;    // unstuffed, the RSTn markers taken out
  int64_t off_quant, off_tables, off_segments, off_sub_segment, off_stream, total_bytes;
  int64_t reserved[4];
};

struct Geo {  // what the kernels need of the header, checked on the host (check_header)
  int32_t nseg, nsub, sub_bits, bpm, h, v, mcus_w, nmcu, restart_mcus;
  uint32_t stream_bits;
  int32_t blocks_w[3];
  int32_t plane[3];  // the component's first coefficient in coef, in blocks
  int32_t nblocks;   // of all three components
};

// the workspace of pgdvs_jpeg_scan_decode(_host): offsets in bytes
struct Workspace {
  int64_t flags, info, head, state, count, first, mcu_prefix, tile_sum, tile_off, total;  // head: the bytes zeroed per call
  int32_t ngroups, ntiles;
};
constexpr int kDcTile = 256;  // MCUs of one workgroup of the DC kernels
constexpr int kInfoWords = 4;  // rounds of the first launch (the largest of any workgroup), fix-up launches that ran, 0, 0

inline int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

inline void workspace_layout(const Geo &g, Workspace *w) {
  w->ngroups = (g.nsub + kSubsPerGroup - 1) / kSubsPerGroup;
  w->ntiles = (g.nmcu + kDcTile - 1) / kDcTile;
  int64_t off = 0;
  w->info = off, off += kInfoWords * 4;                          // info and flags: one block at the start, zeroed per call
  w->flags = off, off += up((int64_t)(w->ngroups + 1) * 4, 16);
  w->head = off;
  off = up(off, 256);
  w->state = off, off += up((int64_t)g.nsub * 8, 256);
  w->count = off, off += up((int64_t)g.nsub * 4, 256);
  w->first = off, off += up((int64_t)(g.nsub + 1) * 4, 256);
  w->mcu_prefix = off, off += up((int64_t)g.nmcu * 12, 256);
  w->tile_sum = off, off += up((int64_t)w->ntiles * 12, 256);
  w->tile_off = off, off += up((int64_t)w->ntiles * 12, 256);
  w->total = off;
}

// The header, checked against the buffer's size and the caller's coef_bytes; fills the geometry.  nullptr = fine, else why
// not.  What lies behind the header (tables, segments, stream) is the device's to clamp: nothing there is trusted for an
// address.
inline const char *check_header(const Header *hd, int64_t prep_bytes, int64_t coef_bytes, Geo *g) {
  if (prep_bytes < (int64_t)sizeof(Header) || hd->magic != kMagic) return "not a buffer pgdvs_jpeg_scan_prepare filled";
  if (hd->total_bytes > prep_bytes) return "the prepared buffer is shorter than its header says";
  if (hd->sub_bytes < kMinSubBytes || hd->sub_bytes > kMaxSubBytes || hd->sub_bytes % 4) return "subsequence size out of range";
  const bool sampling = (hd->h == 1 && hd->v == 1) || (hd->h == 2 && hd->v == 1) || (hd->h == 2 && hd->v == 2);
  if (!sampling || hd->mcus_w < 1 || hd->mcus_h < 1 || hd->mcus_w > kMaxMcusSide || hd->mcus_h > kMaxMcusSide) return "MCU grid out of range";
  const int64_t nmcu = (int64_t)hd->mcus_w * hd->mcus_h;
  if (hd->stream_bytes < 0 || hd->stream_bytes > kMaxScanBytes) return "stream size out of range";
  if (hd->restart_mcus < 1 || hd->nseg != (nmcu + hd->restart_mcus - 1) / hd->restart_mcus) return "restart interval and segment count disagree";
  if (hd->nseg < 1 || hd->nseg > nmcu || hd->nsub < hd->nseg || hd->nsub > hd->stream_bytes / hd->sub_bytes + hd->nseg) return "segment or subsequence count out of range";
  const int64_t ends[5] = {hd->off_quant + 3 * 128, hd->off_tables + (int64_t)kTables * (int64_t)sizeof(Table), hd->off_segments + (int64_t)hd->nseg * (int64_t)sizeof(Segment),
                           hd->off_sub_segment + (int64_t)hd->nsub * 4, hd->off_stream + up(hd->stream_bytes, 8) + 8};
  const int64_t begins[5] = {hd->off_quant, hd->off_tables, hd->off_segments, hd->off_sub_segment, hd->off_stream};
  int64_t last = (int64_t)sizeof(Header);
  for (int i = 0; i < 5; ++i) {
    if (begins[i] < last || begins[i] % 8 || ends[i] > hd->total_bytes) return "a region of the prepared buffer is out of place";
    last = ends[i];
  }
  g->nseg = hd->nseg, g->nsub = hd->nsub, g->sub_bits = hd->sub_bytes * 8, g->h = hd->h, g->v = hd->v, g->bpm = hd->h * hd->v + 2;
  g->mcus_w = hd->mcus_w, g->nmcu = (int32_t)nmcu, g->restart_mcus = hd->restart_mcus, g->stream_bits = (uint32_t)(hd->stream_bytes * 8);
  g->blocks_w[0] = hd->mcus_w * hd->h, g->blocks_w[1] = g->blocks_w[2] = hd->mcus_w;
  g->plane[0] = 0, g->plane[1] = (int32_t)(nmcu * hd->h * hd->v), g->plane[2] = g->plane[1] + (int32_t)nmcu;
  g->nblocks = (int32_t)(nmcu * g->bpm);
  if (hd->coef_bytes != (int64_t)g->nblocks * 128 || coef_bytes != hd->coef_bytes) return "coef_bytes is not the stream's";
  return nullptr;
}

// ---- states -----------------------------------------------------------------------------------------------------------
constexpr uint64_t kInvalid = 1ull << 41;
PGDVS_SCAN_HD uint64_t pack_state(uint32_t pos, int blk, int zz) { return (uint64_t)pos | ((uint64_t)blk << 32) | ((uint64_t)zz << 35); }

// the entry of a subsequence that begins a segment (known), or of any other before anything is known (the guess)
PGDVS_SCAN_HD uint64_t first_entry(uint32_t sub_begin) { return pack_state(sub_begin, 0, 0); }

// the 32 bits at bit `pos` of the stream, first bit highest.  words: the stream as 32-bit words, two of them readable behind
// the word that holds bit stream_bits (the prepared buffer pads so)
PGDVS_SCAN_HD uint32_t peek32(const uint32_t *words, uint32_t stream_bits, uint32_t pos) {
  if (pos > stream_bits) pos = stream_bits;
  const uint32_t i = pos >> 5;
  const uint64_t v = ((uint64_t)__builtin_bswap32(words[i]) << 32) | __builtin_bswap32(words[i + 1]);
  return (uint32_t)(v >> (32 - (pos & 31)));
}

// one Huffman symbol of the 32 bits at the position; -1 for a code the table lacks
PGDVS_SCAN_HD int huff_symbol(const Table &t, uint32_t bits, int *len) {
  const uint32_t e = t.look[bits >> (32 - kLook)];
  if (e) {
    *len = (int)(e >> 8);
    return (int)(e & 255);
  }
  int l = kLook;
  int32_t code = (int32_t)(bits >> (32 - kLook));
  while (l < 16) {
    ++l;
    code = (int32_t)(bits >> (32 - l));
    if (code <= t.maxcode[l]) break;
  }
  if (code > t.maxcode[l]) return -1;
  const int32_t i = code + t.valoff[l];
  if (i < 0 || i >= t.n) return -1;
  *len = l;
  return t.vals[i & 255];
}

PGDVS_SCAN_HD int natural_order(int zz) {
  constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return kNatural[zz & 63];
}

// block `block` of the stream (MCU by MCU; inside an MCU the luma blocks row by row, then Cb, then Cr) -> its first
// coefficient in coef[component][block row][block col][64]; the ordinal is clamped into the grids
PGDVS_SCAN_HD int64_t block_offset(const Geo &g, int32_t block) {
  block = block < 0 ? 0 : (block >= g.nblocks ? g.nblocks - 1 : block);
  const int32_t mcu = block / g.bpm, b = block - mcu * g.bpm;
  const int32_t my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
  const int hv = g.h * g.v;
  const int c = b < hv ? 0 : (b == hv ? 1 : 2);
  const int by = c == 0 ? b / g.h : 0, bx = c == 0 ? b - by * g.h : 0;
  const int hc = c == 0 ? g.h : 1, vc = c == 0 ? g.v : 1;
  return ((int64_t)g.plane[c] + (int64_t)(my * vc + by) * g.blocks_w[c] + (mx * hc + bx)) * 64;
}

// the verified mode's side of decode_sub
struct Verify {
  int16_t *coef;
  int32_t block;      // the stream's ordinal of the block the entry state is in
  int32_t block_end;  // one past the last block the segment owes: blocks from here on are padding, not written nor checked
  bool last_segment;  // (behind the last segment's last block anything may follow; behind another's, less than a byte)
  uint32_t err;       // kStatus* bits, or-ed in
};

// One subsequence: from `entry` while the position is in front of `sub_end`; seg_end: where the segment's data ends (a
// symbol that reaches beyond is "the data ran out").  *count: blocks completed.  max_iter: the loop's bound (a symbol takes
// at least one bit: the subsequence's bits).
template <bool kVerified>
PGDVS_SCAN_HD uint64_t decode_sub(const Table *tabs, const uint32_t *words, const Geo &g, uint64_t entry, uint32_t sub_begin, uint32_t sub_end,
                                  uint32_t seg_end, int max_iter, int32_t *count, Verify *vf) {
  *count = 0;
  if (entry & kInvalid) entry = first_entry(sub_begin);  // the predecessor ended on a fault: guess, as at the start
  uint32_t pos = (uint32_t)entry;
  int blk = (int)((entry >> 32) & 7), zz = (int)((entry >> 35) & 63);
  if (blk >= g.bpm) blk = 0;
  const int hv = g.h * g.v;
  bool live = false;
  int16_t *dst = nullptr;
  if (kVerified) {
    live = vf->block < vf->block_end;
    if (live) dst = vf->coef + block_offset(g, vf->block);
  }
  int n = 0;
  for (int it = 0; it < max_iter && pos < sub_end; ++it) {
    const uint32_t bits = peek32(words, g.stream_bits, pos);
    const int comp = blk < hv ? 0 : (blk == hv ? 1 : 2);
    int len = 1;
    const int sym = huff_symbol(tabs[2 * comp + (zz ? 1 : 0)], bits, &len);
    bool bad = sym < 0, done = false;
    int s = 0, at = zz;
    if (!bad) {
      if (zz == 0) {  // DC: the difference's size
        s = sym;
        bad = s > 15;
        zz = 1;
      } else {
        const int r = sym >> 4;
        s = sym & 15;
        if (s == 0) {
          if (r == 15) {  // ZRL
            zz += 16;
            bad = zz > 64;
            done = zz == 64;
          } else {  // EOB
            done = true;
          }
        } else {
          at = zz + r;
          bad = at > 63;
          zz = at + 1;
          done = zz == 64;
        }
      }
      pos += (uint32_t)(len + s);
      bad = bad || pos > seg_end;
    }
    if (bad) {
      if (kVerified && live) vf->err |= kStatusBadCode;
      *count = n;
      return kInvalid;
    }
    if (kVerified && live && s) {  // Figure F.12's EXTEND of the s bits behind the code
      const int x = (int)((bits << len) >> (32 - s));
      dst[natural_order(at)] = (int16_t)(x < (1 << (s - 1)) ? x - (1 << s) + 1 : x);
    }
    if (done) {
      ++n;
      zz = 0;
      blk = blk + 1 == g.bpm ? 0 : blk + 1;
      if (kVerified && live) {
        if (++vf->block == vf->block_end) {
          live = false;
          if (!vf->last_segment && seg_end - pos >= 8) vf->err |= kStatusLeftOver;
        } else {
          dst = vf->coef + block_offset(g, vf->block);
        }
      }
    }
  }
  *count = n;
  return pack_state(pos, blk, zz);
}

// the extent of subsequence `i` (clamped into the tables): its segment, whether it begins it, its bits
struct SubRange {
  int32_t seg;
  bool begins, ends, last_segment;
  uint32_t begin, end, seg_end;
  int32_t mcu_first, mcu_count, sub_first;
};
PGDVS_SCAN_HD SubRange sub_range(const Geo &g, const Segment *segs, const int32_t *sub_segment, int32_t i) {
  SubRange r;
  int32_t s = sub_segment[i];
  s = s < 0 ? 0 : (s >= g.nseg ? g.nseg - 1 : s);
  const Segment sg = segs[s];
  const int32_t k = i - sg.sub_first;
  r.seg = s;
  r.begins = k <= 0;
  r.ends = k >= sg.sub_count - 1;
  r.last_segment = s == g.nseg - 1;
  r.seg_end = sg.bit_end > g.stream_bits ? g.stream_bits : sg.bit_end;
  const uint64_t b = (uint64_t)sg.bit_begin + (uint64_t)(k < 0 ? 0 : k) * (uint32_t)g.sub_bits;
  r.begin = b > r.seg_end ? r.seg_end : (uint32_t)b;
  const uint64_t e = b + (uint32_t)g.sub_bits;
  r.end = e > r.seg_end ? r.seg_end : (uint32_t)e;
  r.mcu_first = sg.mcu_first, r.mcu_count = sg.mcu_count, r.sub_first = sg.sub_first < 0 ? 0 : (sg.sub_first >= g.nsub ? g.nsub - 1 : sg.sub_first);
  return r;
}

}  // namespace jscan
}  // namespace pgdvs
