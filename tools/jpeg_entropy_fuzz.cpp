// Stand-alone driver of csrc/jpeg_entropy.cpp for the host compiler's sanitizers (tests/test_jpeg_decode_host.py builds and
// runs it; nothing here touches a GPU or Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/jpeg_entropy_fuzz.cpp ml-pgdvs_amd/csrc/jpeg_entropy.cpp -o jpeg_entropy_fuzz
//   ./jpeg_entropy_fuzz SEED MUTATIONS file.jpg [file.jpg ...]
//
// For every file: the stream itself, every truncation of it, and MUTATIONS copies with one byte replaced (a seeded
// generator picks the place and the value) go through pgdvs_jpeg_parse and, where that serves them, through
// pgdvs_jpeg_entropy_decode.  Each variant lives in a heap block of exactly its size and the coefficients in one of exactly
// coef_bytes, so a read or write past either is the sanitizer's to report.  Exit status 0: every call returned 0 or 1 (and
// the unmodified stream 0); 1 otherwise.  One line of counts per file on stdout.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/pgdvs_hip.h"

namespace pgdvs {
static char g_err[512];
void set_error(const char *fmt, ...) {  // the library's lives in error.cpp, with the HIP runtime
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace pgdvs

struct Counts {
  long served = 0, refused_by_parse = 0, refused_by_scan = 0, bad = 0;
};

// one variant: 0 served, 1 refused, anything else is a failure
static int run(const uint8_t *src, size_t n, Counts *k) {
  uint8_t *data = static_cast<uint8_t *>(malloc(n ? n : 1));
  memcpy(data, src, n);
  pgdvs_jpeg_info info;
  int rc = pgdvs_jpeg_parse(data, (int64_t)n, &info);
  if (rc == 1) {
    ++k->refused_by_parse;
  } else if (rc == 0) {
    int16_t *coef = static_cast<int16_t *>(malloc((size_t)info.coef_bytes));
    rc = pgdvs_jpeg_entropy_decode(data, (int64_t)n, coef, info.coef_bytes);
    free(coef);
    if (rc == 1) ++k->refused_by_scan;
    else if (rc == 0) ++k->served;
  }
  free(data);
  if (rc != 0 && rc != 1) {
    ++k->bad;
    fprintf(stderr, "a call returned %d: %s\n", rc, pgdvs::g_err);
  }
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s SEED MUTATIONS file.jpg [file.jpg ...]\n", argv[0]);
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
    Counts k;
    if (run(file.data(), file.size(), &k) != 0) {
      fprintf(stderr, "%s: the unmodified stream is not served: %s\n", argv[a], pgdvs::g_err);
      status = 1;
    }
    for (size_t n = 0; n < file.size(); ++n) run(file.data(), n, &k);
    std::vector<uint8_t> v(file);
    for (long m = 0; m < mutations && !file.empty(); ++m) {
      const size_t at = next() % file.size();
      v[at] = (uint8_t)next();
      run(v.data(), v.size(), &k);
      v[at] = file[at];
    }
    printf("%s: %zu bytes, served %ld, refused by the markers %ld, by the scan %ld, other returns %ld\n", argv[a], file.size(), k.served,
           k.refused_by_parse, k.refused_by_scan, k.bad);
    if (k.bad) status = 1;
  }
  return status;
}
