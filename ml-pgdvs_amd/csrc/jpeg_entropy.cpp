// The host half of the JPEG reader: the markers (pgdvs_jpeg_parse) and the Huffman scan (pgdvs_jpeg_entropy_decode) of a
// baseline YCbCr file; and for the scan read on the device (csrc/jpeg_scan_decode.hip) its preparation
// (pgdvs_jpeg_scan_prepare) and the kernels' host emulation (pgdvs_jpeg_scan_decode_host, over csrc/jpeg_scan_core.h).
// include/pgdvs_hip.h states what is served and what each entry returns; this is how.
//
// Plain C++: no HIP, no GPU, nothing of the rest of the library but set_error -- tools/jpeg_entropy_fuzz.cpp and
// tools/jpeg_scan_fuzz.cpp build this file alone with the host compiler and its sanitizers.  Every read of the stream goes
// through a bounds-checked cursor; every write of a coefficient through a block pointer computed from the checked grids.
//
// The scan: a 64-bit accumulator refilled a byte at a time (FF 00 unstuffed; a marker or the end of the scan feeds zero bits
// that are counted, and consuming one of them is "data ran out"), and per Huffman table a 9-bit lookahead table (code length
// and symbol of every code of up to 9 bits) with the canonical maxcode walk for the longer ones.
#include <stdarg.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pgdvs_hip.h"
#include "jpeg_scan_core.h"

namespace pgdvs {
void set_error(const char *fmt, ...);
}

namespace {

using pgdvs::set_error;

constexpr int kLook = 9;
constexpr int kMaxSize = PGDVS_RESAMPLE_MAX_SIZE;
constexpr int kServed = 0, kRefused = 1, kBadArgument = -1;

const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
  bool defined = false;
  uint8_t bits[17];        // codes of each length 1 .. 16
  uint8_t vals[256];       // the symbols in code order
  int n = 0;               // symbols
  uint16_t look[1 << kLook];  // (length << 8) | symbol for every kLook-bit prefix of a code of up to kLook bits, 0 = longer
  int32_t maxcode[18];     // the largest code of each length, -1 where there is none
  int32_t valoff[17];      // vals index of a code = code + valoff[length]
};

// jdhuff.c's jpeg_make_d_derived_tbl; false for counts that are no prefix code
bool derive(HuffTable &t) {
  int code = 0, k = 0;
  memset(t.look, 0, sizeof(t.look));
  for (int l = 1; l <= 16; ++l) {
    t.valoff[l] = k - code;
    for (int i = 0; i < t.bits[l]; ++i, ++k, ++code) {
      if (code >= (1 << l)) return false;
      if (l <= kLook) {
        const int first = code << (kLook - l);
        for (int f = 0; f < (1 << (kLook - l)); ++f) t.look[first + f] = (uint16_t)((l << 8) | t.vals[k]);
      }
    }
    t.maxcode[l] = t.bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return true;
}

struct Component {
  int id, h, v, tq, td, ta;
};

struct Header {
  pgdvs_jpeg_info info;
  Component comp[3];
  HuffTable dc[4], ac[4];
  int64_t scan_begin, scan_end;  // the entropy-coded bytes: data[scan_begin .. scan_end), data[scan_end] = FF of the EOI
  int mcus_w, mcus_h;
};

int refuse(const char *why) {
  set_error("jpeg: %s", why);
  return kRefused;
}

// the markers up to SOS and the scan's extent
int read_header(const uint8_t *d, int64_t n, Header &hdr) {
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return refuse("no SOI marker: not a JPEG stream");
  uint16_t quant[4][64];
  bool quant_defined[4] = {false, false, false, false};
  bool jfif = false, adobe = false, sof = false;
  int restart = 0, width = 0, height = 0;
  int64_t p = 2;
  for (;;) {
    if (p + 2 > n) return refuse("truncated in front of the scan");
    if (d[p] != 0xFF) return refuse("a marker was expected");
    while (p < n && d[p] == 0xFF) ++p;  // (fill bytes)
    if (p >= n) return refuse("truncated in front of the scan");
    const int m = d[p++];
    if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) return refuse("a marker out of place in front of the scan");
    if (p + 2 > n) return refuse("truncated in front of the scan");
    const int64_t len = (d[p] << 8) | d[p + 1];
    if (len < 2 || p + len > n) return refuse("a segment runs past the end of the stream");
    const uint8_t *s = d + p + 2;
    const int64_t sl = len - 2;
    p += len;
    if (m == 0xC0) {
      if (sof) return refuse("a second frame header");
      if (sl < 6 || s[0] != 8) return refuse("sample precision is not 8 bits");
      height = (s[1] << 8) | s[2], width = (s[3] << 8) | s[4];
      if (s[5] != 3) return refuse("not three components (greyscale, CMYK and YCCK are left to Pillow)");
      if (sl != 6 + 3 * 3) return refuse("frame header of the wrong length");
      if (width < 1 || height < 1 || width > kMaxSize || height > kMaxSize) return refuse("width or height outside 1 .. 16384");
      for (int c = 0; c < 3; ++c) {
        Component &k = hdr.comp[c];
        k.id = s[6 + 3 * c], k.h = s[7 + 3 * c] >> 4, k.v = s[7 + 3 * c] & 15, k.tq = s[8 + 3 * c];
        if (k.tq > 3) return refuse("quantisation table selector above 3");
      }
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return refuse("not a baseline (SOF0) frame: progressive, extended, lossless and arithmetic streams are left to Pillow");
    } else if (m == 0xCC) {
      return refuse("arithmetic coding conditioning");
    } else if (m == 0xC4) {  // DHT: one or more tables
      int64_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return refuse("Huffman table runs past its segment");
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return refuse("Huffman table class or id out of range");
        HuffTable &t = tc ? hdr.ac[th] : hdr.dc[th];
        int count = 0;
        t.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) count += (t.bits[l] = s[q + l]);
        if (count > 256 || q + 17 + count > sl) return refuse("Huffman table runs past its segment");
        memcpy(t.vals, s + q + 17, (size_t)count);
        t.n = count;
        if (!derive(t)) return refuse("Huffman table is no prefix code");
        t.defined = true;
        q += 17 + count;
      }
    } else if (m == 0xDB) {  // DQT: one or more tables
      int64_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq != 0) return refuse("16-bit quantisation table");
        if (tq > 3 || q + 65 > sl) return refuse("quantisation table id out of range or past its segment");
        for (int i = 0; i < 64; ++i) quant[tq][kNatural[i]] = s[q + 1 + i];
        quant_defined[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return refuse("restart interval segment of the wrong length");
      restart = (s[0] << 8) | s[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 5 && memcmp(s, "Adobe", 5) == 0) adobe = true;
    } else if (m == 0xDA) {
      if (!sof) return refuse("scan in front of the frame header");
      if (sl != 1 + 2 * 3 + 3 || s[0] != 3) return refuse("the scan does not interleave all three components");
      for (int c = 0; c < 3; ++c) {
        if (s[1 + 2 * c] != hdr.comp[c].id) return refuse("the scan lists the components in another order");
        hdr.comp[c].td = s[2 + 2 * c] >> 4, hdr.comp[c].ta = s[2 + 2 * c] & 15;
        if (hdr.comp[c].td > 3 || hdr.comp[c].ta > 3 || !hdr.dc[hdr.comp[c].td].defined || !hdr.ac[hdr.comp[c].ta].defined)
          return refuse("the scan names a Huffman table that was not defined");
      }
      if (s[7] != 0 || s[8] != 63 || s[9] != 0) return refuse("the scan is not a full sequential one (Ss 0, Se 63, Ah Al 0)");
      break;
    }
    // (APPn, COM and the rest: skipped)
  }
  if (adobe) return refuse("Adobe APP14 marker: the colour transform is Pillow's to decide");
  const Component *k = hdr.comp;
  if (!jfif && !(k[0].id == 1 && k[1].id == 2 && k[2].id == 3)) return refuse("no JFIF marker and component ids other than 1 2 3: not read as YCbCr");
  if (k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1) return refuse("chroma sampling factors other than 1x1");
  int sampling;
  if (k[0].h == 1 && k[0].v == 1) sampling = PGDVS_JPEG_444;
  else if (k[0].h == 2 && k[0].v == 1) sampling = PGDVS_JPEG_422;
  else if (k[0].h == 2 && k[0].v == 2) sampling = PGDVS_JPEG_420;
  else return refuse("luma sampling other than 1x1, 2x1 or 2x2 (4:1:1, 4:4:0, ...)");
  pgdvs_jpeg_info &info = hdr.info;
  memset(&info, 0, sizeof(info));
  info.width = width, info.height = height, info.sampling = sampling, info.restart_interval = restart;
  hdr.mcus_w = (width + 8 * k[0].h - 1) / (8 * k[0].h), hdr.mcus_h = (height + 8 * k[0].v - 1) / (8 * k[0].v);
  int64_t blocks = 0;
  for (int c = 0; c < 3; ++c) {
    if (!quant_defined[k[c].tq]) return refuse("a component names a quantisation table that was not defined");
    info.blocks_w[c] = hdr.mcus_w * k[c].h, info.blocks_h[c] = hdr.mcus_h * k[c].v;
    blocks += (int64_t)info.blocks_w[c] * info.blocks_h[c];
    memcpy(info.quant[c], quant[k[c].tq], sizeof(info.quant[c]));
  }
  info.coef_bytes = blocks * 128;
  // the scan's extent: up to the first marker that is neither a stuffed FF 00 nor an RSTn; it must be EOI
  hdr.scan_begin = p;
  const uint8_t *q = d + p, *const end = d + n;
  for (;;) {
    q = static_cast<const uint8_t *>(memchr(q, 0xFF, (size_t)(end - q)));
    if (q == nullptr || q + 1 >= end) return refuse("truncated: the scan has no EOI marker");
    const int m = q[1];
    if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) {
      q += 2;
    } else if (m == 0xFF) {
      q += 1;
    } else if (m == 0xD9) {
      break;
    } else {
      return refuse("a marker other than EOI behind the scan (several scans or tables between them)");
    }
  }
  hdr.scan_end = q - d;
  return kServed;
}

struct Bits {
  const uint8_t *p, *end;
  uint64_t acc = 0;
  int n = 0;    // bits in acc (its low n bits)
  int pad = 0;  // of which zero bits fed behind the data: the lowest
  void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (p < end && (*p != 0xFF || (p + 1 < end && p[1] == 0x00))) {
        b = *p;
        p += b == 0xFF ? 2 : 1;
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
    if (pad > n) pad = n;
  }
  unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1); }
  bool drop(int k) {  // false: the data ran out
    n -= k;
    return n >= pad;
  }
};

// one Huffman symbol; -1 for a code the table lacks or data that ran out
inline int symbol(Bits &b, const HuffTable &t) {
  if (b.n < 16) b.fill();
  const unsigned e = t.look[b.peek(kLook)];
  if (e) return b.drop(e >> 8) ? (int)(e & 255) : -1;
  int code = (int)b.peek(kLook), l = kLook;
  while (l < 16) {
    ++l;
    code = (int)b.peek(l);
    if (code <= t.maxcode[l]) break;
  }
  if (code > t.maxcode[l]) return -1;
  const int i = code + t.valoff[l];
  if (i < 0 || i >= t.n || !b.drop(l)) return -1;
  return t.vals[i];
}

// s further bits as a signed value (Figure F.12's EXTEND); s 1 .. 16
inline bool receive_extend(Bits &b, int s, int *v) {
  if (b.n < s) b.fill();
  const int x = (int)b.peek(s);
  if (!b.drop(s)) return false;
  *v = x < (1 << (s - 1)) ? x - (1 << s) + 1 : x;
  return true;
}

int decode_scan(const uint8_t *d, const Header &hdr, int16_t *coef) {
  const pgdvs_jpeg_info &info = hdr.info;
  int16_t *plane[3];
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    plane[c] = coef + off;
    off += (int64_t)info.blocks_w[c] * info.blocks_h[c] * 64;
  }
  Bits b;
  b.p = d + hdr.scan_begin, b.end = d + hdr.scan_end;
  int pred[3] = {0, 0, 0};
  int until_restart = info.restart_interval, next_rst = 0;
  for (int my = 0; my < hdr.mcus_h; ++my) {
    for (int mx = 0; mx < hdr.mcus_w; ++mx) {
      if (info.restart_interval && until_restart == 0) {  // process_restart: the rest of the byte goes, then RSTn
        if (b.n - b.pad >= 8) return refuse("corrupt scan: bytes left over in front of a restart marker");
        while (b.p + 1 < b.end && b.p[0] == 0xFF && b.p[1] == 0xFF) ++b.p;
        if (b.p + 2 > b.end || b.p[0] != 0xFF || b.p[1] != 0xD0 + next_rst) return refuse("corrupt scan: a restart marker is missing or misnumbered");
        b.p += 2;
        b.acc = 0, b.n = 0, b.pad = 0;
        pred[0] = pred[1] = pred[2] = 0;
        next_rst = (next_rst + 1) & 7;
        until_restart = info.restart_interval;
      }
      for (int c = 0; c < 3; ++c) {
        const Component &k = hdr.comp[c];
        const HuffTable &dc = hdr.dc[k.td], &ac = hdr.ac[k.ta];
        for (int by = 0; by < k.v; ++by) {
          for (int bx = 0; bx < k.h; ++bx) {
            int16_t *blk = plane[c] + ((int64_t)(my * k.v + by) * info.blocks_w[c] + (mx * k.h + bx)) * 64;
            memset(blk, 0, 128);
            int s = symbol(b, dc), v;
            if (s < 0 || s > 15) return refuse("corrupt scan: bad DC code, or the data ran out");
            if (s) {
              if (!receive_extend(b, s, &v)) return refuse("corrupt scan: the data ran out");
              pred[c] += v;
              if (pred[c] < -32768 || pred[c] > 32767) return refuse("corrupt scan: DC value outside 16 bits");
            }
            blk[0] = (int16_t)pred[c];
            for (int i = 1; i < 64;) {
              const int rs = symbol(b, ac);
              if (rs < 0) return refuse("corrupt scan: bad AC code, or the data ran out");
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;  // EOB
                i += 16;
                if (i > 64) return refuse("corrupt scan: more than 64 coefficients in a block");
                continue;
              }
              i += r;
              if (i > 63) return refuse("corrupt scan: more than 64 coefficients in a block");
              if (!receive_extend(b, s, &v)) return refuse("corrupt scan: the data ran out");
              blk[kNatural[i++]] = (int16_t)v;
            }
          }
        }
      }
      if (info.restart_interval) --until_restart;
    }
  }
  return kServed;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int64_t pgdvs_jpeg_info_size(void) { return (int64_t)sizeof(pgdvs_jpeg_info); }

extern "C" __attribute__((visibility("default"))) int pgdvs_jpeg_parse(const uint8_t *data, int64_t nbytes, pgdvs_jpeg_info *info) {
  if (info == nullptr || nbytes < 0 || (data == nullptr && nbytes > 0)) {
    set_error("pgdvs_jpeg_parse: null pointer or negative size");
    return kBadArgument;
  }
  Header hdr;
  if (data == nullptr) return refuse("no SOI marker: not a JPEG stream");
  const int rc = read_header(data, nbytes, hdr);
  if (rc == kServed) *info = hdr.info;
  return rc;
}

extern "C" __attribute__((visibility("default"))) int pgdvs_jpeg_entropy_decode(const uint8_t *data, int64_t nbytes, int16_t *coef,
                                                                                 int64_t coef_bytes) {
  if (coef == nullptr || nbytes < 0 || (data == nullptr && nbytes > 0)) {
    set_error("pgdvs_jpeg_entropy_decode: null pointer or negative size");
    return kBadArgument;
  }
  Header hdr;
  if (data == nullptr) return refuse("no SOI marker: not a JPEG stream");
  const int rc = read_header(data, nbytes, hdr);
  if (rc != kServed) return rc;
  if (coef_bytes != hdr.info.coef_bytes) {
    set_error("pgdvs_jpeg_entropy_decode: coef_bytes %lld, the stream's coefficients take %lld", (long long)coef_bytes,
              (long long)hdr.info.coef_bytes);
    return kBadArgument;
  }
  return decode_scan(data, hdr, coef);
}

// ---------------------------------------------------------------------------------------------------------------------
// The scan read on the device: its preparation, and the kernels' emulation on the host.
namespace {

namespace js = pgdvs::jscan;
static_assert(js::kMaxScanBytes == PGDVS_JPEG_SCAN_MAX_BYTES && js::kMinSubBytes <= PGDVS_JPEG_SCAN_SUB_BYTES, "include/pgdvs_hip.h and jpeg_scan_core.h disagree");

struct PrepLayout {
  int nseg;
  int64_t max_subs, scan_len;
  js::Header hd;  // the offsets and total_bytes
};

int prep_layout(const Header &hdr, int32_t sub_bytes, PrepLayout *pl) {
  pl->scan_len = hdr.scan_end - hdr.scan_begin;
  if (pl->scan_len > js::kMaxScanBytes) return refuse("the scan is larger than PGDVS_JPEG_SCAN_MAX_BYTES: left to the host decoder");
  const int64_t nmcu = (int64_t)hdr.mcus_w * hdr.mcus_h;
  const int64_t ri = hdr.info.restart_interval ? hdr.info.restart_interval : nmcu;
  pl->nseg = (int)((nmcu + ri - 1) / ri);
  pl->max_subs = pl->scan_len / sub_bytes + pl->nseg;
  js::Header &h = pl->hd;
  memset(&h, 0, sizeof(h));
  int64_t off = js::up((int64_t)sizeof(js::Header), 16);  // (pgdvs_jpeg_reconstruct takes the tables 16-byte aligned)
  h.off_quant = off, off += 3 * 128;
  h.off_tables = off, off += js::up((int64_t)js::kTables * (int64_t)sizeof(js::Table), 8);
  h.off_segments = off, off += js::up((int64_t)pl->nseg * (int64_t)sizeof(js::Segment), 8);
  h.off_sub_segment = off, off += js::up(pl->max_subs * 4, 8);
  h.off_stream = off, off += js::up(pl->scan_len, 8) + 8;
  h.total_bytes = off;
  return kServed;
}

int sub_bytes_or_default(const char *what, int32_t sub_bytes, int32_t *out) {
  *out = sub_bytes == 0 ? PGDVS_JPEG_SCAN_SUB_BYTES : sub_bytes;
  if (*out < js::kMinSubBytes || *out > js::kMaxSubBytes || *out % 4) {
    set_error("%s: sub_bytes %d (0 for the default, or a multiple of 4 in %d .. %d)", what, sub_bytes, js::kMinSubBytes, js::kMaxSubBytes);
    return kBadArgument;
  }
  return kServed;
}

void copy_table(const HuffTable &t, js::Table *o) {
  memcpy(o->look, t.look, sizeof(o->look));
  memcpy(o->maxcode, t.maxcode, sizeof(o->maxcode));
  memcpy(o->valoff, t.valoff, sizeof(o->valoff));
  o->valoff[0] = 0;
  o->maxcode[0] = -1;
  o->n = t.n;
  memset(o->vals, 0, sizeof(o->vals));
  memcpy(o->vals, t.vals, (size_t)t.n);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int64_t pgdvs_jpeg_scan_prepare_bytes(const uint8_t *data, int64_t nbytes, int32_t sub_bytes) {
  if (nbytes < 0 || (data == nullptr && nbytes > 0)) {
    set_error("pgdvs_jpeg_scan_prepare_bytes: null pointer or negative size");
    return kBadArgument;
  }
  if (sub_bytes_or_default("pgdvs_jpeg_scan_prepare_bytes", sub_bytes, &sub_bytes)) return kBadArgument;
  Header hdr;
  PrepLayout pl;
  if (data == nullptr) {
    refuse("no SOI marker: not a JPEG stream");
    return 0;
  }
  if (read_header(data, nbytes, hdr) != kServed || prep_layout(hdr, sub_bytes, &pl) != kServed) return 0;
  return pl.hd.total_bytes;
}

extern "C" __attribute__((visibility("default"))) int pgdvs_jpeg_scan_prepare(const uint8_t *data, int64_t nbytes, int32_t sub_bytes, void *prepared,
                                                                               int64_t prepared_bytes, pgdvs_jpeg_info *info) {
  if (prepared == nullptr || info == nullptr || nbytes < 0 || (data == nullptr && nbytes > 0) || (reinterpret_cast<uintptr_t>(prepared) & 7) != 0) {
    set_error("pgdvs_jpeg_scan_prepare: null pointer, negative size, or a buffer that is not 8-byte aligned");
    return kBadArgument;
  }
  if (sub_bytes_or_default("pgdvs_jpeg_scan_prepare", sub_bytes, &sub_bytes)) return kBadArgument;
  Header hdr;
  if (data == nullptr) return refuse("no SOI marker: not a JPEG stream");
  int rc = read_header(data, nbytes, hdr);
  if (rc != kServed) return rc;
  PrepLayout pl;
  if ((rc = prep_layout(hdr, sub_bytes, &pl)) != kServed) return rc;
  if (prepared_bytes < pl.hd.total_bytes) {
    set_error("pgdvs_jpeg_scan_prepare: a buffer of %lld bytes, the stream takes %lld (pgdvs_jpeg_scan_prepare_bytes)", (long long)prepared_bytes,
              (long long)pl.hd.total_bytes);
    return kBadArgument;
  }
  uint8_t *base = static_cast<uint8_t *>(prepared);
  js::Header &h = pl.hd;
  js::Segment *segs = reinterpret_cast<js::Segment *>(base + h.off_segments);
  int32_t *sub_segment = reinterpret_cast<int32_t *>(base + h.off_sub_segment);
  uint8_t *out = base + h.off_stream;
  // one pass over the scan's bytes: FF 00 unstuffed, the RSTn markers checked and taken out, a segment's data up to its marker
  const uint8_t *p = data + hdr.scan_begin, *const end = data + hdr.scan_end;
  const int64_t nmcu = (int64_t)hdr.mcus_w * hdr.mcus_h;
  const int64_t ri = hdr.info.restart_interval ? hdr.info.restart_interval : nmcu;
  int64_t o = 0, nsub = 0;
  for (int k = 0; k < pl.nseg; ++k) {
    const int64_t begin = o;
    for (;;) {
      const uint8_t *q = static_cast<const uint8_t *>(p < end ? memchr(p, 0xFF, (size_t)(end - p)) : nullptr);
      const uint8_t *stop = q ? q : end;
      memcpy(out + o, p, (size_t)(stop - p));
      o += stop - p;
      p = stop;
      if (q == nullptr || !(q + 1 < end && q[1] == 0x00)) break;  // the end of the scan, or a marker
      out[o++] = 0xFF;
      p = q + 2;
    }
    if (k < pl.nseg - 1) {  // process_restart's demands (the bits left over in front of the marker are the decoder's to check)
      while (p + 1 < end && p[0] == 0xFF && p[1] == 0xFF) ++p;
      if (p + 2 > end || p[0] != 0xFF || p[1] != 0xD0 + (k & 7)) return refuse("corrupt scan: a restart marker is missing or misnumbered");
      p += 2;
    }
    js::Segment &sg = segs[k];
    sg.bit_begin = (uint32_t)(begin * 8), sg.bit_end = (uint32_t)(o * 8);
    sg.mcu_first = (int32_t)(k * ri), sg.mcu_count = (int32_t)(nmcu - k * ri < ri ? nmcu - k * ri : ri);
    const int64_t subs = o - begin > 0 ? (o - begin + sub_bytes - 1) / sub_bytes : 1;
    sg.sub_first = (int32_t)nsub, sg.sub_count = (int32_t)subs;
    for (int64_t i = 0; i < subs; ++i) sub_segment[nsub + i] = k;
    nsub += subs;
  }
  memset(out + o, 0, (size_t)(js::up(pl.scan_len, 8) + 8 - o));
  memset(sub_segment + nsub, 0, (size_t)(pl.max_subs - nsub) * 4);
  h.magic = js::kMagic, h.sub_bytes = sub_bytes, h.nseg = pl.nseg, h.nsub = (int32_t)nsub;
  h.h = hdr.comp[0].h, h.v = hdr.comp[0].v, h.mcus_w = hdr.mcus_w, h.mcus_h = hdr.mcus_h;
  h.restart_mcus = (int32_t)ri;
  h.coef_bytes = hdr.info.coef_bytes, h.stream_bytes = o;
  memcpy(base, &h, sizeof(h));
  memcpy(base + h.off_quant, hdr.info.quant, 3 * 128);
  js::Table *tabs = reinterpret_cast<js::Table *>(base + h.off_tables);
  for (int c = 0; c < 3; ++c) {
    copy_table(hdr.dc[hdr.comp[c].td], tabs + 2 * c);
    copy_table(hdr.ac[hdr.comp[c].ta], tabs + 2 * c + 1);
  }
  *info = hdr.info;
  return kServed;
}

// The kernels of csrc/jpeg_scan_decode.hip, one after the other on the host: the same core, the same rounds (a workgroup is a
// chunk of kSubsPerGroup subsequences; a round reads every predecessor's exit first and decodes afterwards), the same
// launches behind their flags, the same workspace.  `prepared` is read twice, as the device entry reads its two copies.
extern "C" __attribute__((visibility("default"))) int pgdvs_jpeg_scan_decode_host(const void *prepared_host, const void *prepared, int64_t prepared_bytes,
                                                                                   int16_t *coef, int64_t coef_bytes, uint32_t *status, void *workspace,
                                                                                   int64_t workspace_bytes) {
  if (prepared_host == nullptr || prepared == nullptr || coef == nullptr || status == nullptr || workspace == nullptr ||
      (reinterpret_cast<uintptr_t>(prepared) & 7) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
    set_error("pgdvs_jpeg_scan_decode_host: null pointer, or a buffer that is not 8-byte aligned");
    return kBadArgument;
  }
  js::Header hd;
  if (prepared_bytes >= (int64_t)sizeof(hd)) memcpy(&hd, prepared_host, sizeof(hd));
  js::Geo g;
  if (const char *why = js::check_header(&hd, prepared_bytes, coef_bytes, &g)) {
    set_error("pgdvs_jpeg_scan_decode_host: %s", why);
    return kBadArgument;
  }
  js::Workspace w;
  js::workspace_layout(g, &w);
  if (workspace_bytes < w.total) {
    set_error("pgdvs_jpeg_scan_decode_host: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)w.total);
    return kBadArgument;
  }
  const uint8_t *base = static_cast<const uint8_t *>(prepared);
  const js::Table *tabs = reinterpret_cast<const js::Table *>(base + hd.off_tables);
  const js::Segment *segs = reinterpret_cast<const js::Segment *>(base + hd.off_segments);
  const int32_t *sub_segment = reinterpret_cast<const int32_t *>(base + hd.off_sub_segment);
  const uint32_t *words = reinterpret_cast<const uint32_t *>(base + hd.off_stream);
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  uint32_t *flags = reinterpret_cast<uint32_t *>(ws + w.flags), *infow = reinterpret_cast<uint32_t *>(ws + w.info);
  uint64_t *state = reinterpret_cast<uint64_t *>(ws + w.state);
  int32_t *count = reinterpret_cast<int32_t *>(ws + w.count), *first = reinterpret_cast<int32_t *>(ws + w.first);
  memset(ws, 0, (size_t)w.head);
  memset(coef, 0, (size_t)coef_bytes);
  uint32_t st = 0;
  constexpr int G = js::kSubsPerGroup;
  uint64_t entry[G], ex[G], fresh[G];
  // launch 0: every group on its own, from the known entries and the guesses
  for (int grp = 0; grp < w.ngroups; ++grp) {
    const int n = g.nsub - grp * G < G ? g.nsub - grp * G : G;
    js::SubRange rg[G];
    for (int t = 0; t < n; ++t) {
      const int i = grp * G + t;
      rg[t] = js::sub_range(g, segs, sub_segment, i);
      entry[t] = js::first_entry(rg[t].begin);
      ex[t] = js::decode_sub<false>(tabs, words, g, entry[t], rg[t].begin, rg[t].end, rg[t].seg_end, g.sub_bits, &count[i], nullptr);
    }
    uint32_t rounds = 1;
    for (int r = 1; r < G + 1; ++r) {
      bool changed = false;
      for (int t = 0; t < n; ++t) fresh[t] = rg[t].begins || t == 0 ? entry[t] : ex[t - 1];
      for (int t = 0; t < n; ++t) {
        if (fresh[t] == entry[t]) continue;
        const int i = grp * G + t;
        entry[t] = fresh[t];
        const uint64_t e = js::decode_sub<false>(tabs, words, g, entry[t], rg[t].begin, rg[t].end, rg[t].seg_end, g.sub_bits, &count[i], nullptr);
        if (e != ex[t]) ex[t] = e, changed = true;
      }
      if (!changed) break;
      ++rounds;
    }
    for (int t = 0; t < n; ++t) state[grp * G + t] = ex[t];
    if (rounds > infow[0]) infow[0] = rounds;
  }
  // the fix-up launches: a group's first subsequence takes what the group in front left; a launch in front of which
  // nothing changed leaves at once
  for (int launch = 1; launch < w.ngroups; ++launch) {
    if (launch >= 2 && flags[launch - 1] == 0) continue;
    ++infow[1];
    for (int grp = 1; grp < w.ngroups; ++grp) {
      const int n = g.nsub - grp * G < G ? g.nsub - grp * G : G;
      js::SubRange rg[G];
      bool any = false;
      for (int t = 0; t < n; ++t) {
        const int i = grp * G + t;
        rg[t] = js::sub_range(g, segs, sub_segment, i);
        entry[t] = rg[t].begins ? js::first_entry(rg[t].begin) : state[i - 1];
        ex[t] = state[i];
      }
      for (int r = 0; r < G + 1; ++r) {
        bool changed = false;
        for (int t = 0; t < n; ++t) fresh[t] = rg[t].begins || t == 0 ? entry[t] : ex[t - 1];
        for (int t = 0; t < n; ++t) {
          if (fresh[t] == entry[t] && !(r == 0 && t == 0)) continue;  // (the first one's stored exit may be a guess's)
          const int i = grp * G + t;
          entry[t] = fresh[t];
          const uint64_t e = js::decode_sub<false>(tabs, words, g, entry[t], rg[t].begin, rg[t].end, rg[t].seg_end, g.sub_bits, &count[i], nullptr);
          if (e != ex[t]) ex[t] = e, changed = true;
        }
        if (!changed) break;
        any = true;
      }
      if (any) {
        for (int t = 0; t < n; ++t) state[grp * G + t] = ex[t];
        flags[launch] = 1;
      }
    }
  }
  // every subsequence's first block: the exclusive sum of the counts
  first[0] = 0;
  for (int i = 0; i < g.nsub; ++i) first[i + 1] = first[i] + count[i];
  // the verified pass
  for (int i = 0; i < g.nsub; ++i) {
    const js::SubRange r = js::sub_range(g, segs, sub_segment, i);
    const int64_t ord = (int64_t)first[i] - first[r.sub_first];
    const int64_t owed = (int64_t)r.mcu_count * g.bpm, at = (int64_t)r.mcu_first * g.bpm;
    js::Verify vf;
    vf.coef = coef, vf.err = 0, vf.last_segment = r.last_segment;
    vf.block_end = (int32_t)(at + owed < g.nblocks ? at + owed : g.nblocks);
    vf.block = (int32_t)(at + ord < vf.block_end ? at + ord : vf.block_end);
    int32_t n;
    const uint64_t e = js::decode_sub<true>(tabs, words, g, r.begins ? js::first_entry(r.begin) : state[i - 1], r.begin, r.end, r.seg_end, g.sub_bits, &n, &vf);
    st |= vf.err;
    if (e != state[i] || n != count[i]) st |= js::kStatusNotSynchronised;
    if (r.ends && ord + n < owed) st |= js::kStatusShort;
  }
  // the DC differences summed per component in stream order, from zero at every segment
  const int hv = g.h * g.v;
  int32_t pred[3] = {0, 0, 0};
  for (int32_t m = 0; m < g.nmcu; ++m) {
    if (m % g.restart_mcus == 0) pred[0] = pred[1] = pred[2] = 0;
    for (int k = 0; k < g.bpm; ++k) {
      const int c = k < hv ? 0 : (k == hv ? 1 : 2);
      int16_t *dc = coef + js::block_offset(g, m * g.bpm + k);
      pred[c] += *dc;
      if (pred[c] < -32768 || pred[c] > 32767) {
        st |= js::kStatusDcRange;
        pred[c] = 0;
      }
      *dc = (int16_t)pred[c];
    }
  }
  *status = st;
  return kServed;
}
