// Stand-alone driver of the scan reader's host side -- pgdvs_jpeg_scan_prepare and pgdvs_jpeg_scan_decode_host of
// csrc/jpeg_entropy.cpp over csrc/jpeg_scan_core.h, the core the device kernels run -- for the host compiler's sanitizers
// (tests/test_jpeg_scan_host.py builds and runs it; nothing here touches a GPU or Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/jpeg_scan_fuzz.cpp ml-pgdvs_amd/csrc/jpeg_entropy.cpp -o jpeg_scan_fuzz
//   ./jpeg_scan_fuzz SEED MUTATIONS file.jpg [file.jpg ...]
//
// For every file: the stream itself, every truncation of it, and MUTATIONS copies with one byte replaced (the generator of
// tools/jpeg_entropy_fuzz.cpp) go through the preparation and, where that serves them, through the emulation, at the default
// subsequence size and at the smallest.  Each variant lives in a heap block of exactly its size, the prepared buffer, the
// coefficients and the workspace in blocks of exactly the sizes the entries ask for, so a read or write past any of them is
// the sanitizer's to report.  Each result is held against pgdvs_jpeg_entropy_decode: a scan it refuses must not come back
// with status 0, one it serves comes back with the same coefficients or a non-zero status, and "not synchronised" is never
// set.  Exit status 0: all of that held and the unmodified streams were decoded; 1 otherwise.  One line of counts per file.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/pgdvs_hip.h"
#include "../ml-pgdvs_amd/csrc/jpeg_scan_core.h"

namespace pgdvs {
static char g_err[512];
void set_error(const char *fmt, ...) {  // the library's lives in error.cpp, with the HIP runtime
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace pgdvs

namespace js = pgdvs::jscan;

struct Counts {
  long decoded = 0, refused = 0, fell_back = 0, agreed_corrupt = 0, bad = 0;
};

static void fail(Counts *k, const char *what, int a, unsigned b) {
  ++k->bad;
  fprintf(stderr, "%s (%d, status %u): %s\n", what, a, b, pgdvs::g_err);
}

// one variant at one subsequence size; true: the scan was decoded with status 0
static bool run(const uint8_t *src, size_t n, int32_t sub_bytes, Counts *k) {
  uint8_t *data = static_cast<uint8_t *>(malloc(n ? n : 1));
  memcpy(data, src, n);
  bool decoded = false;
  pgdvs_jpeg_info parsed, info;
  const int rc_parse = pgdvs_jpeg_parse(data, (int64_t)n, &parsed);
  const int64_t need = pgdvs_jpeg_scan_prepare_bytes(data, (int64_t)n, sub_bytes);
  if (need < 0 || (rc_parse != 0 && need != 0)) fail(k, "the size query disagrees with the parser", (int)need, 0);
  if (need <= 0) {
    ++k->refused;
    free(data);
    return false;
  }
  void *prepared = malloc((size_t)need);
  const int rc = pgdvs_jpeg_scan_prepare(data, (int64_t)n, sub_bytes, prepared, need, &info);
  if (rc == 1) {
    ++k->refused;
  } else if (rc != 0 || memcmp(&info, &parsed, sizeof(info)) != 0) {
    fail(k, "the preparation failed or filled another info than the parser", rc, 0);
  } else {
    js::Header hd;
    memcpy(&hd, prepared, sizeof(hd));
    js::Geo g;
    js::Workspace w;
    const char *why = js::check_header(&hd, need, info.coef_bytes, &g);
    if (why != nullptr) {
      fail(k, why, 0, 0);
    } else {
      js::workspace_layout(g, &w);
      int16_t *coef = static_cast<int16_t *>(malloc((size_t)info.coef_bytes)), *want = static_cast<int16_t *>(malloc((size_t)info.coef_bytes));
      void *ws = malloc((size_t)w.total);
      uint32_t *status = static_cast<uint32_t *>(malloc(4));
      const int rc_dev = pgdvs_jpeg_scan_decode_host(prepared, prepared, need, coef, info.coef_bytes, status, ws, w.total);
      const int rc_host = pgdvs_jpeg_entropy_decode(data, (int64_t)n, want, info.coef_bytes);
      if (rc_dev != 0 || (rc_host != 0 && rc_host != 1)) fail(k, "a call returned an argument error", rc_dev, *status);
      else if (*status & js::kStatusNotSynchronised) fail(k, "not synchronised", rc_host, *status);
      else if (rc_host == 1 && *status == 0) fail(k, "the host decoder refuses a scan the emulation decodes", rc_host, *status);
      else if (rc_host == 0 && *status == 0 && memcmp(coef, want, (size_t)info.coef_bytes) != 0) fail(k, "other coefficients than the host decoder's", 0, 0);
      else if (*status == 0) ++k->decoded, decoded = true;
      else if (rc_host == 0) ++k->fell_back;
      else ++k->agreed_corrupt;
      free(status), free(ws), free(want), free(coef);
    }
  }
  free(prepared);
  free(data);
  return decoded;
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
  const int32_t sizes[2] = {0, js::kMinSubBytes};
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
    for (int32_t sub : sizes) {
      if (!run(file.data(), file.size(), sub, &k)) {
        fprintf(stderr, "%s: the unmodified stream is not decoded at sub_bytes %d: %s\n", argv[a], sub, pgdvs::g_err);
        status = 1;
      }
      for (size_t n = 0; n < file.size(); ++n) run(file.data(), n, sub, &k);
    }
    std::vector<uint8_t> v(file);
    for (long m = 0; m < mutations && !file.empty(); ++m) {
      const size_t at = next() % file.size();
      v[at] = (uint8_t)next();
      run(v.data(), v.size(), sizes[m & 1], &k);
      v[at] = file[at];
    }
    printf("%s: %zu bytes, decoded %ld, refused by the preparation %ld, corrupt for both %ld, fell back %ld, failures %ld\n", argv[a], file.size(),
           k.decoded, k.refused, k.agreed_corrupt, k.fell_back, k.bad);
    if (k.bad) status = 1;
  }
  return status;
}
