// Stand-alone driver of the PNG reader's host emulation -- pgdvs_png_decode_host of csrc/png_decode_host.cpp over
// csrc/png_inflate_core.h, the core the device kernels run -- for the host compiler's sanitizers
// (tests/test_png_decode_host.py builds and runs it; nothing here touches a GPU or Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/png_inflate_fuzz.cpp ml-pgdvs_amd/csrc/png_decode_host.cpp -o png_inflate_fuzz
//   ./png_inflate_fuzz SEED MUTATIONS file.png [file.png ...]
//
// Every file is a non-interlaced 8-bit RGB or RGBA PNG; its IDAT payloads are joined into the zlib stream (the chunk walk
// and the CRCs are the Python side's, not this driver's).  The stream itself, every truncation of it (from 6 bytes on: the
// entry takes no shorter one) and MUTATIONS copies with one byte replaced go through the emulation at the default
// subsequence size and at the smallest.  Each variant lives in a batch buffer of exactly table + stream bytes (rounded up
// to 4, as the entry asks), the image, the status word and the workspace in heap blocks of exactly the sizes the entries
// ask for, so a read or write past any of them is the sanitizer's to report.  Held: no call returns an argument error, "not
// synchronised" is never set, and the two subsequence sizes agree on whether the stream is served and on every byte of the
// image.  Exit status 0: all of that held and the unmodified streams were decoded; 1 otherwise.  One line of counts per file.
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

struct Image {
  int32_t h = 0, w = 0, c = 0;
  std::vector<uint8_t> z;
};

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

static bool read_png(const std::vector<uint8_t> &f, Image *im) {
  size_t pos = 8;
  while (pos + 12 <= f.size()) {
    const uint32_t n = be32(&f[pos]);
    if (n > f.size() - pos - 12) return false;
    if (memcmp(&f[pos + 4], "IHDR", 4) == 0 && n == 13) {
      im->w = (int32_t)be32(&f[pos + 8]), im->h = (int32_t)be32(&f[pos + 12]);
      if (f[pos + 16] != 8 || (f[pos + 17] != 2 && f[pos + 17] != 6) || f[pos + 20] != 0) return false;
      im->c = f[pos + 17] == 2 ? 3 : 4;
    } else if (memcmp(&f[pos + 4], "IDAT", 4) == 0) {
      im->z.insert(im->z.end(), f.begin() + (long)pos + 8, f.begin() + (long)pos + 8 + n);
    }
    pos += 12 + (size_t)n;
  }
  return im->h > 0 && im->w > 0 && im->z.size() >= 6;
}

// one variant at one subsequence size into `image` (exactly h * w * c bytes); the status, or 0xFFFFFFFF for a refused call
static uint32_t run(const Image &im, const uint8_t *z, size_t n, int32_t sub_bytes, uint8_t *image, Counts *k) {
  const size_t table = sizeof(pgdvs_png_image) + (16 - sizeof(pgdvs_png_image) % 16) % 16, bytes = table + (n + 3) / 4 * 4;
  uint8_t *batch = static_cast<uint8_t *>(malloc(bytes));
  memset(batch, 0, bytes);
  pgdvs_png_image st;
  st.offset = (int64_t)table, st.size = (int64_t)n, st.height = im.h, st.width = im.w, st.channels = im.c, st.out_channels = im.c;
  st.row_stride = (int64_t)im.w * im.c, st.out = image, st.bit_depth = 8, st.scale = 1;
  memcpy(batch, &st, sizeof(st));
  memcpy(batch + table, z, n);
  const int64_t need = pgdvs_png_inflate_workspace_bytes(reinterpret_cast<const pgdvs_png_image *>(batch), 1);
  uint32_t status = 0xFFFFFFFFu;
  if (need <= 0) {
    ++k->bad;
    fprintf(stderr, "the workspace query refuses the table: %s\n", pgdvs::g_err);
  } else {
    void *ws = malloc((size_t)need);
    uint32_t *word = static_cast<uint32_t *>(malloc(4));
    const int rc = pgdvs_png_decode_host(batch, batch, (int64_t)bytes, 1, sub_bytes, word, ws, need);
    if (rc != 0) {
      ++k->bad;
      fprintf(stderr, "argument error (%d): %s\n", rc, pgdvs::g_err);
    } else {
      status = *word;
      if (status & pi::kStNotSynchronised) {
        ++k->bad;
        fprintf(stderr, "not synchronised (status %u, %zu bytes, sub_bytes %d)\n", status, n, sub_bytes);
      }
    }
    free(word), free(ws);
  }
  free(batch);
  return status;
}

// one variant at both sizes; true: served
static bool both(const Image &im, const uint8_t *src, size_t n, Counts *k) {
  uint8_t *z = static_cast<uint8_t *>(malloc(n ? n : 1));  // (exactly its size: the entry copies nothing, the batch buffer is the bound)
  memcpy(z, src, n);
  const size_t pixels = (size_t)im.h * im.w * im.c;
  uint8_t *a = static_cast<uint8_t *>(malloc(pixels)), *b = static_cast<uint8_t *>(malloc(pixels));
  const uint32_t sa = run(im, z, n, 0, a, k), sb = run(im, z, n, pi::kMinSubBytes, b, k);
  bool served = false;
  if ((sa == 0) != (sb == 0)) {
    ++k->bad;
    fprintf(stderr, "the subsequence sizes disagree: status %u and %u (%zu bytes)\n", sa, sb, n);
  } else if (sa == 0 && memcmp(a, b, pixels) != 0) {
    ++k->bad;
    fprintf(stderr, "the subsequence sizes give other images (%zu bytes)\n", n);
  } else if (sa == 0) {
    ++k->decoded, served = true;
  } else {
    ++k->given_up;
  }
  free(b), free(a), free(z);
  return served;
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
    Image im;
    if (!read_png(file, &im)) {
      fprintf(stderr, "%s: not an 8-bit RGB or RGBA PNG\n", argv[a]);
      return 2;
    }
    Counts k;
    if (!both(im, im.z.data(), im.z.size(), &k)) {
      fprintf(stderr, "%s: the unmodified stream is not decoded: %s\n", argv[a], pgdvs::g_err);
      status = 1;
    }
    for (size_t n = 6; n < im.z.size(); ++n) both(im, im.z.data(), n, &k);
    std::vector<uint8_t> v(im.z);
    for (long m = 0; m < mutations; ++m) {
      const size_t at = next() % v.size();
      v[at] = (uint8_t)next();
      both(im, v.data(), v.size(), &k);
      v[at] = im.z[at];
    }
    printf("%s: stream of %zu bytes, decoded %ld, given up %ld, failures %ld\n", argv[a], im.z.size(), k.decoded, k.given_up, k.bad);
    if (k.bad) status = 1;
  }
  return status;
}
