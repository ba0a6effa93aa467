// The host side of the PNG reader's C ABI: the workspace size and pgdvs_png_decode_host, the emulation of the kernels of
// csrc/png_inflate.hip and csrc/png_unfilter.hip over csrc/png_inflate_core.h.  include/pgdvs_hip.h states the contract.
//
// Plain C++: no HIP, no GPU, nothing of the rest of the library but set_error -- tools/png_inflate_fuzz.cpp builds this file
// alone with the host compiler and its sanitizers.  The emulation runs every step of the core for thread 0 .. kThreads - 1
// where the kernel runs it on its threads and puts a barrier: the same windows, the same rounds (a round reads what the
// round in front committed), the same workspace.  The row filters run row by row: the kernel's skew is an order of
// evaluation, not another result.
#include <stdint.h>
#include <string.h>

#include "../../include/pgdvs_hip.h"
#include "png_inflate_core.h"

namespace pgdvs {
void set_error(const char *fmt, ...);
}

namespace {

namespace pi = pgdvs::pnginf;
using pgdvs::set_error;

static_assert(sizeof(pgdvs_png_image) == sizeof(pi::Image) && sizeof(pi::Image) % 8 == 0, "pgdvs_png_image and pnginf::Image are one layout");

// one stream through the team's walk; returns the status bits
uint32_t inflate_stream(pi::Shared &S, pi::Src &src, uint8_t *out, uint32_t cap, int sub_bits, int64_t max_iters, uint32_t *info) {
  constexpr int T = pi::kThreads;
  uint32_t err = 0, windows = 0, max_sync = 0, max_resolve = 0, blocks = 0;
  bool need_header = true, finished = false;
  S.pos = 16, S.out = 0, S.final_block = 0, S.kind = 3;
  for (int64_t it = 0; it < max_iters; ++it) {
    if (need_header) {
      const uint32_t w0 = S.pos >> 5;
      for (int k = 0; k < pi::kHdrWords; ++k) S.hdr[k] = (uint64_t)w0 + k < src.nwords ? src.words[w0 + k] : 0u;
      pi::read_header(S, src);
      ++blocks;
      if (S.kind == 3) {
        err = S.block_err;
        break;
      }
      if (S.kind == 0) {
        if ((uint64_t)S.out + S.stored_len > cap) {
          err = pi::kStSize;
          break;
        }
        memcpy(out + S.out, reinterpret_cast<const uint8_t *>(src.words) + S.stored_from, S.stored_len);
        S.out += S.stored_len;
        if (S.final_block) {
          finished = true;
          break;
        }
        continue;
      }
      if (S.kind == 2)
        for (int t = 0; t < T; ++t) pi::fixed_lengths(S, t);
      pi::derive_block(S);
      if (S.kind == 3) {
        err = S.block_err;
        break;
      }
      for (int t = 0; t < T; ++t) pi::fill_look(S, t);
      need_header = false;
    }
    const uint32_t wbeg = S.pos, obase = S.out;
    if (wbeg >= src.nbits) {
      err = pi::kStDataOut;
      break;
    }
    ++windows;
    for (int t = 0; t < T; ++t) pi::stage_window(S.win, &src, t, wbeg, sub_bits);
    for (int t = 0; t < T; ++t) {
      pi::sync_step(S, src, t, wbeg, sub_bits, t == 0 ? wbeg : pi::kInvalid, true, cap);
      S.exit[t] = S.pend[t];
    }
    uint32_t rounds = 1;
    for (int r = 1; r <= T; ++r) {
      bool changed[T], any = false;
      for (int t = 0; t < T; ++t) any |= changed[t] = pi::sync_step(S, src, t, wbeg, sub_bits, pi::pred_exit(S, t, wbeg), false, cap);
      if (!any) break;
      for (int t = 0; t < T; ++t)
        if (changed[t]) S.exit[t] = S.pend[t];
      ++rounds;
    }
    max_sync = rounds > max_sync ? rounds : max_sync;
    int stop = T;
    for (int t = T - 1; t >= 0; --t)
      if (pi::stops(S, t)) stop = t;
    const uint32_t last = S.exit[stop < T ? stop : T - 1];
    if (last == pi::kInvalid) {
      err = S.err[stop] ? S.err[stop] : pi::kStNotSynchronised;
      break;
    }
    for (int t = 0; t < T; ++t) pi::drop_behind(S, t, stop, last);
    uint64_t total = 0;
    for (int t = 0; t < T; ++t) S.off[t] = obase + (uint32_t)total, total += S.nout[t];
    S.off[T] = obase + (uint32_t)total;
    if (obase + total > cap) {
      err = pi::kStSize;
      break;
    }
    for (int t = 0; t < T; ++t) S.cur_pos[t] = S.entry[t], S.cur_out[t] = S.off[t], S.done[t] = 0;
    uint32_t rrounds = 0;
    for (int r = 0; r <= T; ++r) {
      bool left = false;
      for (int t = 0; t < T; ++t) pi::resolve_step(S, src, t, wbeg, sub_bits, out, cap);
      for (int t = 0; t < T; ++t) left |= !S.done_pend[t], S.done[t] = S.done_pend[t];
      ++rrounds;
      if (!left) break;
    }
    max_resolve = rrounds > max_resolve ? rrounds : max_resolve;
    for (int t = 0; t < T; ++t) err |= S.err[t];
    for (int t = 0; t < T; ++t)
      if (!S.done[t]) err |= pi::kStNotSynchronised;
    if (err) break;
    S.pos = last & ~pi::kEob, S.out = obase + (uint32_t)total;
    need_header = (last & pi::kEob) != 0;
    if (need_header && S.final_block) {
      finished = true;
      break;
    }
  }
  if (!finished && !err) err = pi::kStNotSynchronised;
  if (!err && S.out != cap) err = pi::kStSize;
  if (!err) {
    for (int t = 0; t < T; ++t) pi::adler_part(S, t, out, cap);
    err = pi::trailer(src, S.pos, pi::adler_sum(S, cap));
  }
  info[0] = windows, info[1] = max_sync, info[2] = max_resolve, info[3] = blocks;
  return err;
}

// the filters undone row by row, the filter byte and (out_channels < channels) the alpha byte dropped; the reconstructed
// row in front is kept in the stream's carry row, the inflated rows stay as they are.  Below 8 bits the filter's unit is the
// byte (one channel): each reconstructed byte leaves as its 8 / depth samples (unpack_byte)
uint32_t unfilter(const pi::Image &st, const uint8_t *rows, uint8_t *carry) {
  const int C = st.channels, OC = st.out_channels, D = st.bit_depth;
  const int64_t units = D == 8 ? st.width : pi::row_bytes(st), pitch = 1 + units * C;
  uint32_t err = 0;
  for (int y = 0; y < st.height; ++y) {
    const uint8_t *row = rows + y * pitch + 1;
    uint32_t ft = row[-1];
    if (ft > 4) err = pi::kStFilter, ft = 0;
    uint8_t *dst = reinterpret_cast<uint8_t *>(st.out) + y * st.row_stride;
    uint8_t left[4] = {0, 0, 0, 0}, upleft[4] = {0, 0, 0, 0};
    for (int64_t x = 0; x < units; ++x)
      for (int c = 0; c < C; ++c) {
        const int64_t k = x * C + c;
        const uint8_t b = y ? carry[k] : 0;
        const uint8_t v = (uint8_t)pi::unfilter_byte(ft, row[k], left[c], b, upleft[c]);
        left[c] = v, upleft[c] = b, carry[k] = v;
        if (D < 8) pi::unpack_byte(v, D, (uint32_t)st.scale, x, st.width, dst);
        else if (c < OC) dst[x * OC + c] = v;
      }
  }
  return err;
}

}  // namespace

#define PGDVS_HOST_API extern "C" __attribute__((visibility("default")))

PGDVS_HOST_API int64_t pgdvs_png_inflate_workspace_bytes(const pgdvs_png_image *streams, int32_t nstreams) {
  const pi::Table t = {reinterpret_cast<const pi::Image *>(streams), nstreams};
  if (t.base == nullptr || t.n < 1 || t.n > 65535) {
    set_error("pgdvs_png_inflate_workspace_bytes: null table or a stream count outside 1 .. 65535");
    return -1;
  }
  for (int32_t i = 0; i < t.n; ++i)
    if (const char *why = pi::check_format(pi::at(t, i))) {
      set_error("pgdvs_png_inflate_workspace_bytes: stream %d: %s", i, why);
      return -1;
    }
  return pi::up(pi::work_offset(t, t.n), 256);
}

PGDVS_HOST_API int pgdvs_png_decode_host(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t nstreams, int32_t sub_bytes, uint32_t *status,
                                         void *workspace, int64_t workspace_bytes) {
  if (batch_host == nullptr || batch == nullptr || status == nullptr || workspace == nullptr || (reinterpret_cast<uintptr_t>(batch) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(batch_host) & 7) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
    set_error("pgdvs_png_decode_host: null pointer, or a buffer that is not 8-byte aligned");
    return -1;
  }
  if (sub_bytes == 0) sub_bytes = pi::kDefaultSubBytes;
  const pi::Table t = {static_cast<const pi::Image *>(batch_host), nstreams};
  if (const char *why = nstreams >= 1 && batch_bytes >= (int64_t)nstreams * (int64_t)sizeof(pi::Image) ? pi::check_streams(t, batch_bytes, sub_bytes)
                                                                                                      : "the batch buffer is shorter than its table") {
    set_error("pgdvs_png_decode_host: %s", why);
    return -1;
  }
  const int64_t need = pi::up(pi::work_offset(t, nstreams), 256);
  if (workspace_bytes < need) {
    set_error("pgdvs_png_decode_host: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    return -1;
  }
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  memset(ws, 0, (size_t)pi::work_head(nstreams));
  pi::Shared *S = new pi::Shared;
  for (int32_t i = 0; i < nstreams; ++i) {
    const pi::Image st = pi::at(t, i);
    pi::Src src;
    src.words = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(batch) + st.offset);
    src.nwords = (uint32_t)((st.size + 3) / 4), src.nbits = (uint32_t)st.size * 8;
    src.win = nullptr, src.win_first = 0, src.win_count = 0;
    uint8_t *rows = ws + pi::work_offset(t, i);
    status[i] = inflate_stream(*S, src, rows, (uint32_t)pi::inflated_bytes(st), sub_bytes * 8, 2 * st.size + 2, reinterpret_cast<uint32_t *>(ws) + (int64_t)i * pi::kInfoWords);
    if (status[i] == 0) status[i] = unfilter(st, rows, ws + pi::carry_offset(t, i));
  }
  delete S;
  return 0;
}
