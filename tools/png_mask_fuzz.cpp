// Stand-alone driver of the mask PNG reader's host emulation -- pgdvs_png_decode_host of csrc/png_decode_host.cpp:
// the inflate core, the byte-unit row filters and unpack_byte of csrc/png_inflate_core.h, the code the device kernels run --
// for the host compiler's sanitizers (tests/test_png_mask_host.py builds and runs it; nothing here touches a GPU or Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/png_mask_fuzz.cpp ml-pgdvs_amd/csrc/png_decode_host.cpp -o png_mask_fuzz
//   ./png_mask_fuzz SEED MUTATIONS file.png [file.png ...]
//
// Every file is a non-interlaced PNG of colour type 0 or 3 at bit depth 1, 2, 4 or 8 (the chunk walk and the CRCs are the
// Python side's, not this driver's).  Its zlib stream and MUTATIONS copies with one byte replaced go through the emulation at
// the default subsequence size and at the smallest, alone and as the second stream of a batch behind an 8-bit RGB stream of
// garbage (a mixed table).  The batch buffer, the image (exactly height * width bytes, the row stride the width), the status
// words and the workspace are heap blocks of exactly the sizes the entries ask for, so a read or write past any of them is
// the sanitizer's to report.  Held: no call returns an argument error, "not synchronised" is never set, the two subsequence
// sizes and the two batches agree on whether the stream is served and on every byte of the image, and every pixel of a served
// image (filled with 0xA5 beforehand) is a sample of the file's depth times its scale (equality with Pillow is the Python
// tests').  Exit status 0: all of that held and the unmodified streams were decoded; 1 otherwise.  One line of counts per file.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/pgdvs_hip.h"
#include "../ml-pgdvs_amd/csrc/png_inflate_core.h"

namespace pgdvs {
static char g_err[512];
void set_error(const char *fmt, ...) {  // the library's lives in error.cpp, with the HIP runtime
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace pgdvs

namespace pi = pgdvs::pnginf;

struct Counts {
  long decoded = 0, given_up = 0, bad = 0;
};

struct Mask {
  int32_t h = 0, w = 0, depth = 0, scale = 1;
  std::vector<uint8_t> z;
};

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

static bool read_png(const std::vector<uint8_t> &f, Mask *im) {
  size_t pos = 8;
  while (pos + 12 <= f.size()) {
    const uint32_t n = be32(&f[pos]);
    if (n > f.size() - pos - 12) return false;
    if (memcmp(&f[pos + 4], "IHDR", 4) == 0 && n == 13) {
      im->w = (int32_t)be32(&f[pos + 8]), im->h = (int32_t)be32(&f[pos + 12]), im->depth = f[pos + 16];
      const int colour = f[pos + 17];
      if ((colour != 0 && colour != 3) || (im->depth != 1 && im->depth != 2 && im->depth != 4 && im->depth != 8) || f[pos + 20] != 0) return false;
      im->scale = colour == 3 ? 1 : im->depth == 2 ? 85 : im->depth == 4 ? 17 : 1;
    } else if (memcmp(&f[pos + 4], "IDAT", 4) == 0) {
      im->z.insert(im->z.end(), f.begin() + (long)pos + 8, f.begin() + (long)pos + 8 + n);
    }
    pos += 12 + (size_t)n;
  }
  return im->h > 0 && im->w > 0 && im->z.size() >= 6;
}

static size_t up16(size_t a) { return (a + 15) / 16 * 16; }

// one variant at one subsequence size into `image` (exactly h * w bytes); `mixed`: behind a colour stream of garbage in one
// table.  The status, or 0xFFFFFFFF for a refused call
static uint32_t run(const Mask &im, const uint8_t *z, size_t n, int32_t sub_bytes, bool mixed, uint8_t *image, Counts *k) {
  const int32_t ns = mixed ? 2 : 1;
  const size_t table = up16((size_t)ns * sizeof(pgdvs_png_image)), first = mixed ? 16 : 0, bytes = table + first + (n + 3) / 4 * 4;
  uint8_t *batch = static_cast<uint8_t *>(malloc(bytes));
  memset(batch, 0x5A, bytes);
  uint8_t *colour = static_cast<uint8_t *>(malloc(2 * 3 * 3));  // the garbage stream's 2 x 3 RGB image
  pgdvs_png_image st[2];
  memset(st, 0, sizeof(st));
  if (mixed) {
    st[0].offset = (int64_t)table, st[0].size = 12, st[0].height = 2, st[0].width = 3, st[0].channels = 3, st[0].out_channels = 3;
    st[0].row_stride = 9, st[0].out = colour, st[0].bit_depth = 8, st[0].scale = 1;
  }
  pgdvs_png_image &m = st[ns - 1];
  m.offset = (int64_t)(table + first), m.size = (int64_t)n, m.height = im.h, m.width = im.w, m.channels = 1, m.out_channels = 1;
  m.row_stride = im.w, m.out = image, m.bit_depth = im.depth, m.scale = im.scale;
  memcpy(batch, st, (size_t)ns * sizeof(pgdvs_png_image));
  memcpy(batch + table + first, z, n);
  const int64_t need = pgdvs_png_inflate_workspace_bytes(reinterpret_cast<const pgdvs_png_image *>(batch), ns);
  uint32_t status = 0xFFFFFFFFu;
  if (need <= 0) {
    ++k->bad;
    fprintf(stderr, "the workspace query refuses the table: %s\n", pgdvs::g_err);
  } else {
    void *ws = malloc((size_t)need);
    uint32_t *words = static_cast<uint32_t *>(malloc(4 * (size_t)ns));
    const int rc = pgdvs_png_decode_host(batch, batch, (int64_t)bytes, ns, sub_bytes, words, ws, need);
    if (rc != 0) {
      ++k->bad;
      fprintf(stderr, "argument error (%d): %s\n", rc, pgdvs::g_err);
    } else {
      status = words[ns - 1];
      if (status & pi::kStNotSynchronised) {
        ++k->bad;
        fprintf(stderr, "not synchronised (status %u, %zu bytes, sub_bytes %d)\n", status, n, sub_bytes);
      }
      if (mixed && words[0] == 0) {
        ++k->bad;
        fprintf(stderr, "the garbage colour stream was served\n");
      }
    }
    free(words), free(ws);
  }
  free(colour), free(batch);
  return status;
}

// one variant at both sizes, alone and in the mixed table; true: served
static bool all_four(const Mask &im, const uint8_t *src, size_t n, Counts *k) {
  uint8_t *z = static_cast<uint8_t *>(malloc(n ? n : 1));  // (exactly its size: the entry copies nothing, the batch buffer is the bound)
  memcpy(z, src, n);
  const size_t pixels = (size_t)im.h * im.w;
  uint8_t *img[4];
  uint32_t st[4];
  for (int v = 0; v < 4; ++v) {
    img[v] = static_cast<uint8_t *>(malloc(pixels));
    memset(img[v], 0xA5, pixels);
    st[v] = run(im, z, n, v & 1 ? pi::kMinSubBytes : 0, (v & 2) != 0, img[v], k);
  }
  bool served = st[0] == 0, fine = true;
  for (int v = 1; v < 4 && fine; ++v) {
    if ((st[v] == 0) != served) {
      ++k->bad, fine = false;
      fprintf(stderr, "the variants disagree: status %u and %u (%zu bytes)\n", st[0], st[v], n);
    } else if (served && memcmp(img[0], img[v], pixels) != 0) {
      ++k->bad, fine = false;
      fprintf(stderr, "the variants give other images (%zu bytes)\n", n);
    }
  }
  if (fine && served) {
    const int top = ((1 << im.depth) - 1) * im.scale;
    for (size_t p = 0; p < pixels && fine; ++p)
      if (img[0][p] > top || img[0][p] % im.scale) {  // (a pixel never written keeps 0xA5 where the format cannot give it)
        ++k->bad, fine = false;
        fprintf(stderr, "pixel %zu is %u: no sample of depth %d times %d\n", p, img[0][p], im.depth, im.scale);
      }
  }
  if (fine) ++(served ? k->decoded : k->given_up);
  for (int v = 0; v < 4; ++v) free(img[v]);
  free(z);
  return served && fine;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s SEED MUTATIONS file.png [file.png ...]\n", argv[0]);
    return 2;
  }
  uint64_t state = strtoull(argv[1], nullptr, 10) * 2 + 1;
  const long mutations = strtol(argv[2], nullptr, 10);
  auto next = [&state]() {  // (Knuth's MMIX multiplier; the high bits)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
  };
  int status = 0;
  for (int a = 3; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (f == nullptr) {
      fprintf(stderr, "%s: cannot open\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> file;
    uint8_t chunk[4096];
    for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + got);
    fclose(f);
    Mask im;
    if (!read_png(file, &im)) {
      fprintf(stderr, "%s: not a grey or palette PNG of 1, 2, 4 or 8 bits\n", argv[a]);
      return 2;
    }
    Counts k;
    if (!all_four(im, im.z.data(), im.z.size(), &k)) {
      fprintf(stderr, "%s: the unmodified stream is not decoded: %s\n", argv[a], pgdvs::g_err);
      status = 1;
    }
    std::vector<uint8_t> v(im.z);
    for (long m = 0; m < mutations; ++m) {
      const size_t at = next() % v.size();
      v[at] = (uint8_t)next();
      all_four(im, v.data(), v.size(), &k);
      v[at] = im.z[at];
    }
    printf("%s: stream of %zu bytes, decoded %ld, given up %ld, failures %ld\n", argv[a], im.z.size(), k.decoded, k.given_up, k.bad);
    if (k.bad) status = 1;
  }
  return status;
}
