// The core of the PNG reader's inflate, shared by the device kernel (csrc/png_inflate.hip) and its host emulation
// (csrc/png_decode_host.cpp: pgdvs_png_decode_host).  Plain C++ and nothing of HIP but the __host__ __device__ marks:
// tools/png_inflate_fuzz.cpp builds it with the host compiler and its sanitizers.
//
// One TEAM of kThreads threads owns one zlib stream and walks its deflate blocks.  Everything the team shares lives in one
// Shared struct (LDS on the device, a plain struct on the host), and every step is a function of (Shared, thread index t)
// that reads only what an earlier step wrote: the kernel runs a step on all threads and puts a barrier behind it, the
// emulation runs it for t = 0 .. kThreads - 1.  Both therefore see the same windows, rounds and workspace.
//
// Inside one block the code is fixed, so a decoder that only ever starts on a TOKEN -- a literal; a length with its extra
// bits, the distance and its extra bits; or end-of-block -- has the bit position as its whole state.  The block's bits are
// cut into windows of kThreads SUBSEQUENCES of sub_bits bits.  decode_sub reads the tokens from an entry position until
// the position leaves the subsequence and returns that position: the entry of the next one.  Thread 0 knows its entry;
// every other thread guesses its subsequence's first bit and decodes again whenever its predecessor's exit says otherwise.
// The true entries are the one fixed point of exit[t] = decode_sub(exit[t - 1]); round r makes thread r right, so kThreads
// rounds always suffice and the loop leaves as soon as a round changes no exit.  An end-of-block sets kEob in the exit; a
// thread handed such an entry keeps to its guess, and what the threads behind the chain's first end-of-block decoded is
// dropped once the exits stand (handing the end-of-block on instead would cost a round per thread behind it).
//
// Two modes, one function.  Speculative (kWrite = false): counts the bytes the tokens produce and writes nothing; any fault
// ends the subsequence with the one kInvalid exit (and the fault's status bit in *err, which only counts once the entry is
// known to be the true one), and a thread handed kInvalid starts from its guess again.  Verified (kWrite = true): the entry
// and the output offset are the true ones; literals are written at once and a match is copied once every byte it reads is
// final -- in front of the window, written by this thread, or owned by threads that finished in an earlier round; else the
// call returns kStall with the cursor where it stopped and is taken up again in the next round.  Round r finishes thread
// r, so kThreads rounds bound this too.
//
// Every bit position, table index, output offset and distance that comes from stream data is clamped or checked before it
// is used: peek() reads zero behind the stream's words, tokens that end behind the stream's last bit are faults, symbols
// index tables of their full range, and a store goes to out[o] only under o < cap.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define PGDVS_PNG_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PGDVS_PNG_HD inline
#endif

namespace pgdvs {
namespace pnginf {

constexpr int kThreads = 256;  // threads of a team = subsequences of a window
constexpr int kLitLook = 10, kDistLook = 9;
constexpr int kLitSyms = 288, kDistSyms = 32, kClSyms = 19;
constexpr int kMinSubBytes = 8, kMaxSubBytes = 1024, kDefaultSubBytes = 64;  // = PGDVS_PNG_INFLATE_SUB_BYTES
constexpr int64_t kMaxBytes = (int64_t)1 << 28;  // = PGDVS_PNG_INFLATE_MAX_BYTES, compressed and inflated: bit positions stay below 2^31
constexpr int kMaxSide = 16384;
constexpr int kHdrWords = 256;    // the words of a dynamic header staged in LDS: 17 + 19 * 3 + 320 * (7 + 7) bits fit 143
constexpr int kInfoWords = 4;     // per stream: windows, most synchronisation rounds of a window, most resolve rounds, blocks

constexpr uint32_t kInvalid = 0xFFFFFFFFu, kStall = 0xFFFFFFFEu, kEob = 0x80000000u;

// the status word (include/pgdvs_hip.h, PGDVS_PNG_*)
constexpr uint32_t kStBlock = 1, kStCode = 2, kStDistance = 4, kStStored = 8, kStDataOut = 16, kStSize = 32, kStLeftOver = 64, kStAdler = 128,
                   kStFilter = 256, kStNotSynchronised = 512;

// One stream of a batch, as the caller states it (pgdvs_png_image in include/pgdvs_hip.h, field for field): 8-bit colour
// (channels 3 or 4, bit_depth 8, scale 1), or one channel of bit_depth 1, 2, 4 or 8 -- grey or palette indices -- whose
// samples leave as bytes, times `scale`.
struct Image {
  int64_t offset, size;  // the zlib stream (header and Adler-32 included) in the batch buffer, offset a multiple of 16
  int32_t height, width, channels, out_channels;
  int64_t row_stride;    // bytes between two rows of out
  uint64_t out;          // address of the image's first byte
  int32_t bit_depth, scale;
};
// A batch's table: n entries at the batch buffer's start.
struct Table {
  const Image *base;
  int32_t n;
};
PGDVS_PNG_HD const Image &at(const Table &t, int32_t i) { return t.base[i]; }

inline int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// a row's bytes behind its filter byte: samples below a byte are packed, the last byte padded
PGDVS_PNG_HD int64_t row_bytes(const Image &s) { return ((int64_t)s.width * s.channels * s.bit_depth + 7) / 8; }
PGDVS_PNG_HD int64_t inflated_bytes(const Image &s) { return (int64_t)s.height * (1 + row_bytes(s)); }
// the workspace: kInfoWords words per stream, then per stream its inflated rows (work_offset) and one reconstructed row
// (carry_offset: the last row of a block of 64 rows, which the next block's first row needs), each 16-byte aligned
PGDVS_PNG_HD int64_t work_head(int32_t n) { return ((int64_t)n * kInfoWords * 4 + 255) / 256 * 256; }
PGDVS_PNG_HD int64_t pad16(int64_t a) { return (a + 15) / 16 * 16; }
PGDVS_PNG_HD int64_t work_offset(const Table &t, int32_t i) {
  int64_t off = work_head(t.n);
  for (int32_t k = 0; k < i && k < t.n; ++k) {
    const Image s = at(t, k);
    off += pad16(inflated_bytes(s)) + pad16(row_bytes(s));
  }
  return off;
}
PGDVS_PNG_HD int64_t carry_offset(const Table &t, int32_t i) { return work_offset(t, i) + pad16(inflated_bytes(at(t, i))); }

// an image's size and sample format alone (the workspace query's check); nullptr = fine, else why not
inline const char *check_format(const Image &s) {
  if (s.height < 1 || s.width < 1 || s.height > kMaxSide || s.width > kMaxSide) return "image size out of range";
  if (s.channels == 1) {
    if (s.bit_depth != 1 && s.bit_depth != 2 && s.bit_depth != 4 && s.bit_depth != 8) return "one channel at bit depth 1, 2, 4 or 8";
    if (s.scale < 1 || (int64_t)s.scale * ((1 << s.bit_depth) - 1) > 255) return "a sample scale that leaves the byte";
  } else {
    if (s.channels != 3 && s.channels != 4) return "3 or 4 channels";
    if (s.bit_depth != 8 || s.scale != 1) return "colour streams have bit depth 8 and scale 1";
  }
  if (inflated_bytes(s) > kMaxBytes) return "inflated size above PGDVS_PNG_INFLATE_MAX_BYTES";
  return nullptr;
}

// The table, checked on the host in front of any launch; nullptr = fine, else why not.
inline const char *check_streams(const Table &t, int64_t batch_bytes, int32_t sub_bytes) {
  const int32_t n = t.n;
  if (n < 1 || n > 65535) return "1 .. 65535 streams";
  if (sub_bytes < kMinSubBytes || sub_bytes > kMaxSubBytes || sub_bytes % 4) return "subsequence size out of range";
  const int64_t table = up((int64_t)n * (int64_t)sizeof(Image), 16);
  if (batch_bytes < table) return "the batch buffer is shorter than its table";
  for (int32_t i = 0; i < n; ++i) {
    const Image s = at(t, i);
    if (const char *why = check_format(s)) return why;
    if (s.out_channels != s.channels && (s.out_channels != 3 || s.channels == 1)) return "out_channels is 3 or the file's";
    if (s.size < 6 || s.size > kMaxBytes - 16) return "stream size out of range";
    if (s.offset < table || s.offset % 16 || s.offset > batch_bytes || up(s.size, 4) > batch_bytes - s.offset) return "stream outside the batch buffer";
    if (s.out == 0 || s.row_stride < (int64_t)s.width * s.out_channels) return "null out or a row stride below a row";
  }
  return nullptr;
}

// ---- the bit stream: 32-bit words, least significant bit first ---------------------------------------------------------------
struct Src {
  const uint32_t *words;
  uint32_t nwords, nbits;  // nbits = 8 * the stream's bytes; the words behind them read as zero
  const uint32_t *win;     // the window's words staged by the team (Shared::win): words[win_first .. win_first + win_count)
  uint32_t win_first, win_count;
};
constexpr int kStagedSubBytes = 128;                              // windows of larger subsequences are read from the stream itself
constexpr int kWinWords = kThreads * kStagedSubBytes / 4 + 4;     // a window's words and the three a last token may reach into

PGDVS_PNG_HD uint32_t word_at(const Src &s, uint32_t wi) {
  const uint32_t k = wi - s.win_first;  // (wraps for a word in front of the window)
  if (k < s.win_count) return s.win[k];
  return wi < s.nwords ? s.words[wi] : 0u;
}
PGDVS_PNG_HD uint64_t peek_src(const Src &s, uint32_t bit) {  // peek() through the staged window
  const uint32_t wi = bit >> 5, sh = bit & 31;
  const uint64_t w0 = word_at(s, wi), w1 = word_at(s, wi + 1), w2 = word_at(s, wi + 2);
  uint64_t v = (w0 | (w1 << 32)) >> sh;
  if (sh) v |= w2 << (64 - sh);
  return v;
}
// thread t's share of staging the window that begins at bit wbeg; every thread sets its own Src the same way
PGDVS_PNG_HD uint32_t window_words(int sub_bits) { return sub_bits <= kStagedSubBytes * 8 ? (uint32_t)(kThreads * (sub_bits / 32) + 4) : 0u; }
PGDVS_PNG_HD void stage_window(uint32_t *win, Src *src, int t, uint32_t wbeg, int sub_bits) {
  src->win = win, src->win_first = wbeg >> 5, src->win_count = window_words(sub_bits);
  for (uint32_t k = (uint32_t)t; k < src->win_count; k += kThreads) win[k] = src->win_first + k < src->nwords ? src->words[src->win_first + k] : 0u;
}

PGDVS_PNG_HD uint64_t peek(const uint32_t *words, uint32_t nwords, uint32_t bit) {  // the 64 bits from `bit` on
  const uint32_t wi = bit >> 5, sh = bit & 31;
  const uint64_t w0 = wi < nwords ? words[wi] : 0u, w1 = wi + 1 < nwords ? words[wi + 1] : 0u, w2 = wi + 2 < nwords ? words[wi + 2] : 0u;
  uint64_t v = (w0 | (w1 << 32)) >> sh;
  if (sh) v |= w2 << (64 - sh);
  return v;
}

PGDVS_PNG_HD uint32_t rev15(uint32_t x) {  // the low 15 bits, reversed
  x = ((x >> 1) & 0x5555u) | ((x & 0x5555u) << 1);
  x = ((x >> 2) & 0x3333u) | ((x & 0x3333u) << 2);
  x = ((x >> 4) & 0x0F0Fu) | ((x & 0x0F0Fu) << 4);
  x = ((x >> 8) | (x << 8)) & 0xFFFFu;
  return x >> 1;
}

// ---- the tables: canonical codes, maxcode / valoffset behind a look-ahead --------------------------------------------------------
struct Code {             // one derived code
  int32_t maxcode[16];    // the largest code of each length, -1 where there is none
  int32_t valoff[16];     // sorted index of a code = code + valoff[length]
  int32_t nsorted;        // symbols with a length
};

struct Shared {
  uint16_t lit_look[1 << kLitLook];    // (length << 9) | symbol for the first kLitLook bits of the stream, 0 = longer or none
  uint16_t dist_look[1 << kDistLook];
  uint16_t lit_sorted[kLitSyms], dist_sorted[kDistSyms];  // the symbols in code order
  Code lit, dist;
  uint8_t lens[kLitSyms + kDistSyms + 8];  // the block's code lengths: literal/length ones, then distance ones
  Code cl_code;                            // the code-length code of a dynamic header, and what thread 0 needs to derive a code:
  uint16_t cl_sorted[kClSyms + 1];         // (indexed by stream data, so kept here and not in a thread's private memory)
  uint8_t cl_lens[kClSyms + 1];
  int32_t count[16], next[16];
  uint32_t hdr[kHdrWords];                 // the stream's words from the block header on
  uint32_t win[kWinWords];                 // the window's words (stage_window)
  // one entry per thread
  uint32_t exit[kThreads], pend[kThreads], entry[kThreads], nout[kThreads], err[kThreads];
  uint32_t off[kThreads + 1];              // absolute output offset of each thread's first byte
  uint32_t cur_pos[kThreads], cur_out[kThreads];
  uint8_t done[kThreads], done_pend[kThreads];
  uint32_t adler_a[kThreads], adler_b[kThreads];
  // the walk, written by thread 0 alone
  uint32_t pos, out, hlit, hdist, block_err, final_block, kind;  // kind: 0 stored, 1 dynamic, 2 fixed, 3 = stop
  uint32_t stored_from, stored_len;
};

// lens[0 .. n) -> counts, maxcode, valoff and the sorted symbols; false for a set zlib's inflate_table refuses
// (over-subscribed; incomplete unless it is empty or one code of one bit; `strict`: the code-length code, never incomplete)
PGDVS_PNG_HD bool derive(const uint8_t *lens, int n, bool strict, Code *c, uint16_t *sorted, int max_sorted, int32_t *count, int32_t *next) {
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int s = 0; s < n; ++s) ++count[lens[s] & 15];
  int32_t left = 1, total = 0, code = 0, k = 0;
  for (int l = 1; l < 16; ++l) {
    left = left * 2 - count[l];
    if (left < 0) return false;
    total += count[l];
  }
  if (left > 0 && (strict || !(total == 0 || (total == 1 && count[1] == 1)))) return false;
  if (strict && total == 0) return false;
  c->maxcode[0] = -1, c->valoff[0] = 0;
  for (int l = 1; l < 16; ++l) {
    c->valoff[l] = k - code;
    next[l] = k;
    k += count[l], code += count[l];
    c->maxcode[l] = count[l] ? code - 1 : -1;
    code <<= 1;
  }
  c->nsorted = total;
  for (int s = 0; s < n; ++s) {
    const int l = lens[s] & 15;
    if (l && next[l] < max_sorted) sorted[next[l]++] = (uint16_t)s;
  }
  return true;
}

// the canonical walk over lengths first .. last of the 15 reversed bits; 0 = no such code, else (length << 9) | symbol
PGDVS_PNG_HD uint32_t walk(const Code &c, const uint16_t *sorted, uint32_t r15, int first, int last) {
  for (int l = first; l <= last; ++l) {
    const int32_t code = (int32_t)(r15 >> (15 - l));
    if (code <= c.maxcode[l]) {
      const int32_t k = code + c.valoff[l];
      if (k < 0 || k >= c.nsorted) return 0;
      return ((uint32_t)l << 9) | sorted[k];
    }
  }
  return 0;
}

// entry i of a look-ahead table of `bits` bits (the team fills the tables entry by entry)
PGDVS_PNG_HD uint16_t look_entry(const Code &c, const uint16_t *sorted, uint32_t i, int bits) { return (uint16_t)walk(c, sorted, rev15(i), 1, bits); }

PGDVS_PNG_HD uint32_t symbol(const uint16_t *look, int bits, const Code &c, const uint16_t *sorted, uint32_t v) {
  const uint32_t e = look[v & ((1u << bits) - 1)];
  return e ? e : walk(c, sorted, rev15(v & 0x7FFFu), bits + 1, 15);
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------
struct Token {
  uint32_t kind;  // 0 literal (len = the byte), 1 match, 2 end of block, 3 fault (len = the status bit)
  uint32_t bits, len, dist;
};

PGDVS_PNG_HD Token decode_token(const Shared &S, const Src &src, uint32_t pos) {
  Token tk;
  tk.kind = 3, tk.bits = 0, tk.len = kStCode, tk.dist = 0;
  uint64_t v = peek_src(src, pos);
  uint32_t e = symbol(S.lit_look, kLitLook, S.lit, S.lit_sorted, (uint32_t)v);
  if (e == 0) return tk;
  uint32_t used = e >> 9;
  const uint32_t sym = e & 511;
  v >>= used;
  if (sym < 256) {
    tk.kind = 0, tk.len = sym;
  } else if (sym == 256) {
    tk.kind = 2;
  } else {
    if (sym > 285) return tk;
    uint32_t len = 258, ex = 0;
    if (sym < 265) len = sym - 254;
    else if (sym < 285) ex = (sym - 261) >> 2, len = ((4 + ((sym - 261) & 3)) << ex) + 3;
    len += (uint32_t)v & ((1u << ex) - 1);
    v >>= ex, used += ex;
    e = symbol(S.dist_look, kDistLook, S.dist, S.dist_sorted, (uint32_t)v);
    if (e == 0) return tk;
    const uint32_t dsym = e & 511;
    if (dsym > 29) return tk;
    v >>= e >> 9, used += e >> 9;
    uint32_t dist = dsym + 1, dex = 0;
    if (dsym > 3) dex = (dsym >> 1) - 1, dist = ((2 + (dsym & 1)) << dex) + 1;
    dist += (uint32_t)v & ((1u << dex) - 1);
    used += dex;
    tk.kind = 1, tk.len = len, tk.dist = dist;
  }
  tk.bits = used;
  if (pos + used > src.nbits) tk.kind = 3, tk.len = kStDataOut;
  return tk;
}

// whether out[s .. e) is final for thread t: in front of the window, or owned by threads that were done a round ago
PGDVS_PNG_HD bool is_final(const Shared &S, int t, uint32_t s, uint32_t e) {
  if (e > S.off[t]) e = S.off[t];  // (the rest is this thread's own, written in order)
  if (s >= e || e <= S.off[0]) return true;
  if (s < S.off[0]) s = S.off[0];
  int ab[2];
  const uint32_t x[2] = {s, e - 1};
  for (int k = 0; k < 2; ++k) {  // the last u < t with off[u] <= x
    int lo = 0, hi = t - 1;
    for (int step = 0; step < 9 && lo < hi; ++step) {
      const int mid = (lo + hi + 1) >> 1;
      if (S.off[mid] <= x[k]) lo = mid;
      else hi = mid - 1;
    }
    ab[k] = lo;
  }
  bool ok = true;
  for (int u = ab[0]; u <= ab[1] && u < kThreads; ++u) ok = ok && S.done[u];
  return ok;
}

// out[q .. q + len) = the bytes `dist` in front of each, as if copied one after the other (dist < len repeats); nothing at or
// behind cap is written.  A byte-by-byte copy waits for one load per byte, and for dist < len each load for the store in
// front of it.  So: a distance below 8 is a pattern of `dist` bytes, loaded once into a register and stored round and round;
// any other distance goes eight bytes at a time, the eight loads in flight together in front of the eight stores (dist >= 8:
// none of them reads what this group writes).  len is at most 258.
PGDVS_PNG_HD void copy_match(uint8_t *out, uint32_t q, uint32_t len, uint32_t dist, uint32_t cap) {
  if (q >= cap) return;
  if (len > cap - q) len = cap - q;
  if (dist < 8) {
    uint64_t pat = 0;
    for (uint32_t j = 0; j < 8; ++j)
      if (j < dist) pat |= (uint64_t)out[q - dist + j] << (8 * j);
    uint32_t k = 0;
    for (uint32_t i = 0; i < len; ++i) {
      out[q + i] = (uint8_t)(pat >> (8 * k));
      k = k + 1 == dist ? 0 : k + 1;
    }
  } else {
    for (uint32_t i = 0; i < len; i += 8) {
      const uint32_t n = len - i < 8 ? len - i : 8;
      uint64_t v = 0;
      for (uint32_t j = 0; j < 8; ++j)
        if (j < n) v |= (uint64_t)out[q + i - dist + j] << (8 * j);
      for (uint32_t j = 0; j < 8; ++j)
        if (j < n) out[q + i + j] = (uint8_t)(v >> (8 * j));
    }
  }
}

// The subsequence from *pos (the entry) to `end`; *o counts the bytes (speculative: from the caller's 0; verified: the
// absolute output offset).  Returns the exit, kInvalid (a fault, its bit in *err) or kStall (verified alone; *pos and *o
// say where to go on).  max_tokens bounds the loop: sub_bits + 1 tokens can never all fit.
template <bool kWrite>
PGDVS_PNG_HD uint32_t decode_sub(const Shared &S, const Src &src, uint32_t *pos, uint32_t end, uint32_t *o, uint32_t *err, int max_tokens, int t,
                                 uint8_t *out, uint32_t cap) {
  uint32_t p = *pos, q = *o, ret = kInvalid;
  *err = 0;
  for (int k = 0; k <= max_tokens; ++k) {
    if (p >= end) {
      ret = p;
      break;
    }
    const Token tk = decode_token(S, src, p);
    if (tk.kind == 3) {
      *err = tk.len;
      break;
    }
    if (tk.kind == 2) {
      ret = (p + tk.bits) | kEob;
      break;
    }
    if (tk.kind == 0) {
      if (kWrite && q < cap) out[q] = (uint8_t)tk.len;
      q += 1;
    } else {
      if (kWrite) {
        if (tk.dist > q) {
          *err = kStDistance;
          break;
        }
        if (!is_final(S, t, q - tk.dist, q - tk.dist + (tk.len < tk.dist ? tk.len : tk.dist))) {
          ret = kStall;
          break;
        }
        copy_match(out, q, tk.len, tk.dist, cap);
      }
      q += tk.len;
    }
    p += tk.bits;
    if (q > cap) {  // (more than the image's rows: the stream is given up where it is)
      *err = kStSize;
      break;
    }
  }
  *pos = p, *o = q;
  return ret;
}

// ---- the steps of a window -----------------------------------------------------------------------------------------------------------
PGDVS_PNG_HD uint32_t sub_end(const Src &src, uint32_t wbeg, int t, int sub_bits) {
  const uint64_t e = (uint64_t)wbeg + (uint64_t)(t + 1) * (uint32_t)sub_bits;
  return e < src.nbits ? (uint32_t)e : src.nbits;
}

// decode thread t's subsequence from `entry` (kInvalid: from its guess) into pend / nout / err; true if the exit changed
PGDVS_PNG_HD bool sync_step(Shared &S, const Src &src, int t, uint32_t wbeg, int sub_bits, uint32_t entry, bool first, uint32_t cap) {
  if (entry == kInvalid || (entry & kEob)) entry = (uint32_t)((uint64_t)wbeg + (uint64_t)t * (uint32_t)sub_bits < src.nbits ? wbeg + (uint32_t)t * (uint32_t)sub_bits : src.nbits);
  if (!first && entry == S.entry[t]) return false;
  S.entry[t] = entry;
  uint32_t n = 0, err = 0, p = entry;
  const uint32_t ex = decode_sub<false>(S, src, &p, sub_end(src, wbeg, t, sub_bits), &n, &err, sub_bits, t, nullptr, cap);
  S.nout[t] = ex == kInvalid ? 0 : n, S.err[t] = err;
  S.pend[t] = ex;
  return first || ex != S.exit[t];
}

PGDVS_PNG_HD uint32_t pred_exit(const Shared &S, int t, uint32_t wbeg) { return t == 0 ? wbeg : S.exit[t - 1]; }

// The chain is true up to its first exit that is kInvalid or an end of block: thread `stop` (kThreads: none).  What the
// threads behind it decoded from their guesses is dropped: they produce nothing and pass the stop's exit on.
PGDVS_PNG_HD bool stops(const Shared &S, int t) { return (S.exit[t] & kEob) != 0; }  // (kInvalid has the bit too)
PGDVS_PNG_HD void drop_behind(Shared &S, int t, int stop, uint32_t stop_exit) {
  if (t > stop) S.nout[t] = 0, S.err[t] = 0, S.entry[t] = S.exit[t] = stop_exit;
}

// one resolve round of thread t
PGDVS_PNG_HD void resolve_step(Shared &S, const Src &src, int t, uint32_t wbeg, int sub_bits, uint8_t *out, uint32_t cap) {
  S.done_pend[t] = S.done[t];
  if (S.done[t]) return;
  uint32_t err = 0, r = S.entry[t];
  if (!(S.entry[t] & kEob)) r = decode_sub<true>(S, src, &S.cur_pos[t], sub_end(src, wbeg, t, sub_bits), &S.cur_out[t], &err, sub_bits, t, out, cap);
  if (r == kStall) return;
  if (r == kInvalid) S.err[t] = err ? err : kStNotSynchronised;
  else if (r != S.exit[t] || S.cur_out[t] != S.off[t] + S.nout[t]) S.err[t] = kStNotSynchronised;
  S.done_pend[t] = 1;
}

// ---- the block header, read by thread 0 from the staged words ------------------------------------------------------------------------
PGDVS_PNG_HD void fixed_lengths(Shared &S, int t) {
  for (int s = t; s < kLitSyms + kDistSyms; s += kThreads) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
}

// BFINAL / BTYPE at S.pos and what follows: a stored block's LEN / NLEN, or a dynamic block's lengths into S.lens.  Sets
// S.kind, S.pos (the first token, or the stored bytes' end), S.block_err.  hdr holds the words from bit (S.pos & ~31) on.
PGDVS_PNG_HD void read_header(Shared &S, const Src &src) {
  const uint32_t base = S.pos & ~31u;
  uint32_t p = S.pos - base;  // position inside hdr
  S.kind = 3, S.block_err = 0;
  if (S.pos + 3 > src.nbits) {
    S.block_err = kStDataOut;
    return;
  }
  const uint32_t h = (uint32_t)peek(S.hdr, kHdrWords, p);
  S.final_block = h & 1;
  const uint32_t type = (h >> 1) & 3;
  p += 3;
  if (type == 3) {
    S.block_err = kStBlock;
  } else if (type == 0) {
    const uint32_t byte = (base + p + 7) >> 3;
    if ((uint64_t)byte * 8 + 32 > src.nbits) {
      S.block_err = kStDataOut;
      return;
    }
    const uint32_t ln = (uint32_t)peek(S.hdr, kHdrWords, byte * 8 - base);
    const uint32_t len = ln & 0xFFFF;
    if ((len ^ (ln >> 16)) != 0xFFFF) {
      S.block_err = kStStored;
    } else if ((uint64_t)(byte + 4 + len) * 8 > src.nbits) {
      S.block_err = kStDataOut;
    } else {
      S.kind = 0, S.stored_from = byte + 4, S.stored_len = len, S.pos = (byte + 4 + len) * 8;
    }
  } else if (type == 1) {
    S.kind = 2, S.hlit = kLitSyms, S.hdist = kDistSyms, S.pos = base + p;  // (the team writes the fixed lengths)
  } else {
    const uint32_t hlit = (h >> 3 & 31) + 257, hdist = (h >> 8 & 31) + 1, hclen = (h >> 13 & 15) + 4;
    p += 14;
    if (hlit > 286 || hdist > 30) {
      S.block_err = kStBlock;
      return;
    }
    const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < kClSyms; ++i) S.cl_lens[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i, p += 3) S.cl_lens[order[i]] = (uint8_t)(peek(S.hdr, kHdrWords, p) & 7);
    if (!derive(S.cl_lens, kClSyms, true, &S.cl_code, S.cl_sorted, kClSyms, S.count, S.next)) {
      S.block_err = kStBlock;
      return;
    }
    uint32_t n = 0, prev = 0;
    for (int k = 0; k < kLitSyms + kDistSyms && n < hlit + hdist; ++k) {  // (every symbol gives at least one length)
      const uint32_t v = (uint32_t)peek(S.hdr, kHdrWords, p);
      const uint32_t e = walk(S.cl_code, S.cl_sorted, rev15(v & 0x7FFFu), 1, 7);
      if (e == 0) {
        S.block_err = kStBlock;
        return;
      }
      p += e >> 9;
      const uint32_t sym = e & 511;
      uint32_t rep = 1, val = sym;
      if (sym == 16) {
        if (n == 0) {
          S.block_err = kStBlock;
          return;
        }
        val = prev, rep = 3 + ((v >> (e >> 9)) & 3), p += 2;
      } else if (sym == 17) {
        val = 0, rep = 3 + ((v >> (e >> 9)) & 7), p += 3;
      } else if (sym == 18) {
        val = 0, rep = 11 + ((v >> (e >> 9)) & 127), p += 7;
      }
      if (n + rep > hlit + hdist) {
        S.block_err = kStBlock;
        return;
      }
      for (uint32_t i = 0; i < rep; ++i) S.lens[n++] = (uint8_t)val;
      prev = val;
    }
    if (n != hlit + hdist || S.lens[256] == 0) {  // (zlib: "missing end-of-block")
      S.block_err = kStBlock;
      return;
    }
    if ((uint64_t)base + p > src.nbits) {
      S.block_err = kStDataOut;
      return;
    }
    S.kind = 1, S.hlit = hlit, S.hdist = hdist, S.pos = base + p;
  }
}

// the two codes from S.lens (thread 0), then the look-ahead tables entry by entry (the team)
PGDVS_PNG_HD void derive_block(Shared &S) {
  if (!derive(S.lens, (int)S.hlit, false, &S.lit, S.lit_sorted, kLitSyms, S.count, S.next) ||
      !derive(S.lens + S.hlit, (int)S.hdist, false, &S.dist, S.dist_sorted, kDistSyms, S.count, S.next))
    S.kind = 3, S.block_err = kStBlock;
}
PGDVS_PNG_HD void fill_look(Shared &S, int t) {
  for (uint32_t i = (uint32_t)t; i < (1u << kLitLook); i += kThreads) S.lit_look[i] = look_entry(S.lit, S.lit_sorted, i, kLitLook);
  for (uint32_t i = (uint32_t)t; i < (1u << kDistLook); i += kThreads) S.dist_look[i] = look_entry(S.dist, S.dist_sorted, i, kDistLook);
}

// ---- Adler-32 over out[0 .. n): thread t's share, then thread 0's sum -------------------------------------------------------------
constexpr uint32_t kAdlerMod = 65521;
PGDVS_PNG_HD void adler_part(Shared &S, int t, const uint8_t *out, uint32_t n) {
  const uint32_t chunk = (n + kThreads - 1) / kThreads;
  const uint32_t b = (uint64_t)chunk * (uint32_t)t < n ? chunk * (uint32_t)t : n, e = n - b < chunk ? n : b + chunk;
  uint64_t a = 0, s = 0;  // a = the bytes' sum, s = the sum of the running sums
  for (uint32_t i = b; i < e; ++i) {
    a += out[i], s += a;
    if (((i - b) & 4095) == 4095) a %= kAdlerMod, s %= kAdlerMod;
  }
  a %= kAdlerMod, s %= kAdlerMod;
  S.adler_a[t] = (uint32_t)a;
  S.adler_b[t] = (uint32_t)((s + a * ((n - e) % kAdlerMod)) % kAdlerMod);  // every byte behind the share adds the share's sum once more
}
PGDVS_PNG_HD uint32_t adler_sum(const Shared &S, uint32_t n) {
  uint64_t a = 1, b = n % kAdlerMod;
  for (int t = 0; t < kThreads; ++t) a += S.adler_a[t], b += S.adler_b[t];
  return (uint32_t)((b % kAdlerMod) << 16 | (a % kAdlerMod));
}

// what is left behind the final block: exactly the four Adler bytes, most significant first
PGDVS_PNG_HD uint32_t trailer(const Src &src, uint32_t pos, uint32_t adler) {
  const uint32_t byte = (pos + 7) >> 3;
  if ((uint64_t)byte * 8 + 32 > src.nbits) return kStDataOut;
  if (byte * 8 + 32 != src.nbits) return kStLeftOver;
  const uint32_t v = (uint32_t)peek(src.words, src.nwords, byte * 8);
  const uint32_t stored = (v & 0xFF) << 24 | (v >> 8 & 0xFF) << 16 | (v >> 16 & 0xFF) << 8 | v >> 24;
  return stored == adler ? 0 : kStAdler;
}

// ---- the row filters ------------------------------------------------------------------------------------------------------------------
PGDVS_PNG_HD uint32_t unfilter_byte(uint32_t ft, uint32_t raw, uint32_t a, uint32_t b, uint32_t c) {  // a left, b up, c up-left
  uint32_t pred = 0;
  if (ft == 1) pred = a;
  else if (ft == 2) pred = b;
  else if (ft == 3) pred = (a + b) >> 1;
  else if (ft == 4) {
    const int32_t p = (int32_t)a + (int32_t)b - (int32_t)c;
    const int32_t pa = p > (int32_t)a ? p - (int32_t)a : (int32_t)a - p, pb = p > (int32_t)b ? p - (int32_t)b : (int32_t)b - p,
                  pc = p > (int32_t)c ? p - (int32_t)c : (int32_t)c - p;
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (raw + pred) & 0xFF;
}


// the 8 / depth samples of a reconstructed byte (depth 1, 2 or 4), most significant bits first, as bytes times `scale`: byte
// `unit` of its row holds pixels unit * (8 / depth) and on; those at or behind `width` are padding and dropped
PGDVS_PNG_HD void unpack_byte(uint32_t v, int depth, uint32_t scale, int64_t unit, int width, uint8_t *row_out) {
  const int per = 8 / depth;
  for (int j = 0; j < 8; ++j) {
    const int64_t x = unit * per + j;
    if (j < per && x < width) row_out[x] = (uint8_t)(((v >> (8 - depth * (j + 1))) & ((1u << depth) - 1)) * scale);
  }
}

}  // namespace pnginf
}  // namespace pgdvs
