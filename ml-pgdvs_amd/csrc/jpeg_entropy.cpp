// The host half of the JPEG reader: the markers (pgdvs_jpeg_parse) and the Huffman scan (pgdvs_jpeg_entropy_decode) of a
// baseline YCbCr file.  include/pgdvs_hip.h states what is served and what each entry returns; this is how.
//
// Plain C++: no HIP, no GPU, nothing of the rest of the library but set_error -- tools/jpeg_entropy_fuzz.cpp builds this file
// alone with the host compiler and its sanitizers.  Every read of the stream goes through a bounds-checked cursor; every
// write of a coefficient through a block pointer computed from the checked grids.
//
// The scan: a 64-bit accumulator refilled a byte at a time (FF 00 unstuffed; a marker or the end of the scan feeds zero bits
// that are counted, and consuming one of them is "data ran out"), and per Huffman table a 9-bit lookahead table (code length
// and symbol of every code of up to 9 bits) with the canonical maxcode walk for the longer ones.
#include <stdarg.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pgdvs_hip.h"

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
