// The zlib streams of a batch of PNG files, inflated on the device: pgdvs_png_decode gives the images a PNG reader gives,
// byte for byte, from a batch buffer of stream table and streams.  include/pgdvs_hip.h states the contract,
// csrc/png_inflate_core.h the decoder and why guessed entries converge; this file is the inflate kernel and the entry,
// csrc/png_unfilter.hip the row filters.  pgdvs_png_decode_host (csrc/png_decode_host.cpp) is the same walk on the CPU.
//
// One workgroup of kThreads threads owns one stream; the grid is the batch.  The workgroup walks the stream's blocks:
//   header    the words from the header on are staged in LDS and thread 0 reads BFINAL / BTYPE and, for a dynamic block,
//             the code-length code and the HLIT + HDIST lengths (serial, at most 320 symbols); a stored block is copied by
//             all threads; for a coded block thread 0 derives maxcode / valoffset and the sorted symbols and all threads
//             fill the two look-ahead tables entry by entry.
//   sync      a window of kThreads subsequences, its words staged in LDS: every thread decodes from its known entry (thread 0) or its guess, then
//             rounds over LDS: a thread whose predecessor's exit is not the entry it used decodes again, until
//             __syncthreads_or reports that no exit changed (round r makes thread r right: kThreads rounds always suffice).
//   count     the chain is true up to its first end-of-block or fault (thread `stop`); what later threads decoded is
//             dropped; block_excl_scan over the bytes each subsequence produces gives every thread its output offset.
//   resolve   every thread decodes once more, verified: literals are written at once, a match once its source bytes are
//             final (in front of the window, its own, or of threads done a round ago); a thread that meets a match it may
//             not copy yet goes on from there in the next round.  Round r finishes thread r, so kThreads rounds bound this too.
//             A workgroup-scope fence and a barrier stand between a round's stores and the next round's loads.
// The first end-of-block ends the block and the walk continues at the next header; a window without one is followed by
// the next window under the same tables.  Behind the final block: the size, the Adler-32 of the inflated bytes (each
// thread a share, thread 0 the sum) and the stream's last four bytes.
// Every loop's bound is a launch argument or a constant; no workgroup waits for another; the only global atomic is the
// status word's OR, which nothing waits on.
#include "common.h"
#include "png_inflate_core.h"
#include "wave.h"

namespace pgdvs {

int png_unfilter_launch(const pnginf::Table &table, uint8_t *workspace, uint32_t *status, int max_rows, int max_width, hipStream_t st);

namespace {

namespace pi = pnginf;
constexpr int T = pi::kThreads;

__device__ __forceinline__ void team_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

__global__ void __launch_bounds__(T) png_inflate_kernel(const pi::Table table, const uint8_t *__restrict__ batch, uint8_t *workspace,
                                                        uint32_t *__restrict__ status, int sub_bits, int max_iters) {
  __shared__ pi::Shared S;
  __shared__ uint32_t s_wsum[T / kWave];
  __shared__ int s_stop;
  const int t = threadIdx.x, i = blockIdx.x;
  const pi::Image st = pi::at(table, i);
  pi::Src src;
  src.words = reinterpret_cast<const uint32_t *>(batch + st.offset);
  src.nwords = (uint32_t)((st.size + 3) / 4), src.nbits = (uint32_t)st.size * 8;
  src.win = nullptr, src.win_first = 0, src.win_count = 0;
  uint8_t *out = workspace + pi::work_offset(table, i);
  const uint32_t cap = (uint32_t)pi::inflated_bytes(st);
  uint32_t err = 0, windows = 0, max_sync = 0, max_resolve = 0, blocks = 0;
  bool need_header = true, finished = false, gave_up = false;  // gave_up: the status word has the reason already
  if (t == 0) S.pos = 16, S.out = 0, S.final_block = 0, S.kind = 3;
  __syncthreads();
  for (int it = 0; it < max_iters; ++it) {
    if (need_header) {
      const uint32_t w0 = S.pos >> 5;
      for (int k = t; k < pi::kHdrWords; k += T) S.hdr[k] = (uint64_t)w0 + k < src.nwords ? src.words[w0 + k] : 0u;
      __syncthreads();
      if (t == 0) pi::read_header(S, src);
      __syncthreads();
      ++blocks;
      if (S.kind == 3) {
        err = S.block_err;
        break;
      }
      if (S.kind == 0) {
        const uint32_t at = S.out, len = S.stored_len, from = S.stored_from;
        if ((uint64_t)at + len > cap) {
          err = pi::kStSize;
          break;
        }
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(src.words);
        for (uint32_t k = t; k < len; k += T) out[at + k] = bytes[from + k];  // (read_header held from + len inside the stream)
        team_fence();
        __syncthreads();
        if (t == 0) S.out = at + len;
        __syncthreads();
        if (S.final_block) {
          finished = true;
          break;
        }
        continue;
      }
      if (S.kind == 2) pi::fixed_lengths(S, t);
      __syncthreads();
      if (t == 0) pi::derive_block(S);
      __syncthreads();
      if (S.kind == 3) {
        err = S.block_err;
        break;
      }
      pi::fill_look(S, t);
      need_header = false;
      __syncthreads();
    }
    const uint32_t wbeg = S.pos, obase = S.out;
    if (wbeg >= src.nbits) {
      err = pi::kStDataOut;
      break;
    }
    ++windows;
    pi::stage_window(S.win, &src, t, wbeg, sub_bits);  // (the barrier at the window's end stands in front of these stores)
    __syncthreads();
    // ---- sync
    pi::sync_step(S, src, t, wbeg, sub_bits, t == 0 ? wbeg : pi::kInvalid, true, cap);
    S.exit[t] = S.pend[t];
    if (t == 0) s_stop = T;
    uint32_t rounds = 1;
    for (int r = 1; r <= T; ++r) {
      __syncthreads();
      const bool changed = pi::sync_step(S, src, t, wbeg, sub_bits, pi::pred_exit(S, t, wbeg), false, cap);
      if (!__syncthreads_or(changed)) break;  // (every thread has read its predecessor's exit by now)
      if (changed) S.exit[t] = S.pend[t];
      ++rounds;
    }
    max_sync = rounds > max_sync ? rounds : max_sync;
    // ---- count
    if (pi::stops(S, t)) atomicMin(&s_stop, t);
    __syncthreads();
    const int stop = s_stop;
    const uint32_t last = S.exit[stop < T ? stop : T - 1];
    if (last == pi::kInvalid) {
      err = S.err[stop < T ? stop : T - 1];
      err = err ? err : pi::kStNotSynchronised;
      break;
    }
    pi::drop_behind(S, t, stop, last);
    uint32_t total;
    const uint32_t off = block_excl_scan<T / kWave>(S.nout[t], s_wsum, total);
    if ((uint64_t)obase + total > cap) {
      err = pi::kStSize;
      break;
    }
    S.off[t] = obase + off;
    if (t == T - 1) S.off[T] = obase + total;
    S.cur_pos[t] = S.entry[t], S.cur_out[t] = obase + off, S.done[t] = 0;
    __syncthreads();
    // ---- resolve
    uint32_t rrounds = 0;
    int left = 1;
    for (int r = 0; r <= T; ++r) {
      pi::resolve_step(S, src, t, wbeg, sub_bits, out, cap);
      team_fence();
      left = __syncthreads_or(!S.done_pend[t]);
      S.done[t] = S.done_pend[t];
      ++rrounds;
      if (!left) break;
      __syncthreads();
    }
    max_resolve = rrounds > max_resolve ? rrounds : max_resolve;
    uint32_t mine = S.err[t];
    if (left) mine |= pi::kStNotSynchronised;
    if (mine) atomicOr(status + i, mine);
    if (__syncthreads_or(mine != 0)) {
      gave_up = true;
      break;
    }
    if (t == 0) S.pos = last & ~pi::kEob, S.out = obase + total;
    need_header = (last & pi::kEob) != 0;
    __syncthreads();
    if (need_header && S.final_block) {
      finished = true;
      break;
    }
  }
  if (!finished && !err && !gave_up) err = pi::kStNotSynchronised;
  if (!err && !gave_up && S.out != cap) err = pi::kStSize;
  if (!err && !gave_up) {  // (uniform: err and the walk's words are the same in every thread)
    team_fence();
    __syncthreads();
    pi::adler_part(S, t, out, cap);
    __syncthreads();
    if (t == 0) err = pi::trailer(src, S.pos, pi::adler_sum(S, cap));
  }
  if (t == 0) {
    if (err) atomicOr(status + i, err);
    uint32_t *info = reinterpret_cast<uint32_t *>(workspace) + (int64_t)i * pi::kInfoWords;
    info[0] = windows, info[1] = max_sync, info[2] = max_resolve, info[3] = blocks;
  }
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_png_decode(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t nstreams, int32_t sub_bytes, uint32_t *status,
                               void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(batch_host && batch && status && workspace, "pgdvs_png_decode: null pointer");
  PGDVS_REQUIRE(nstreams >= 1 && batch_bytes >= (int64_t)nstreams * (int64_t)sizeof(pi::Image), "pgdvs_png_decode: the batch buffer is shorter than its table");
  if (sub_bytes == 0) sub_bytes = pi::kDefaultSubBytes;
  const pi::Table table = {static_cast<const pi::Image *>(batch_host), nstreams};
  const char *why = pi::check_streams(table, batch_bytes, sub_bytes);
  PGDVS_REQUIRE(why == nullptr, "pgdvs_png_decode: %s", why);
  const int64_t need = pi::up(pi::work_offset(table, nstreams), 256);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(batch) & 15) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                "pgdvs_png_decode: the batch buffer must be 16-byte aligned, status 4-byte");
  PGDVS_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "pgdvs_png_decode: workspace of %lld bytes, %lld needed (256-byte aligned)",
                (long long)workspace_bytes, (long long)need);
  int64_t max_size = 0;
  int max_rows = 0, max_width = 0;
  for (int32_t i = 0; i < nstreams; ++i) {
    const pi::Image &im = pi::at(table, i);
    max_size = im.size > max_size ? im.size : max_size;
    max_rows = im.height > max_rows ? im.height : max_rows;
    max_width = im.width > max_width ? im.width : max_width;  // (a row of packed samples has no more bytes than pixels)
  }
  const hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)pi::work_head(nstreams), st);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)nstreams * 4, st);
  if (e != hipSuccess) {
    set_error("pgdvs_png_decode: %s", hipGetErrorString(e));
    return PGDVS_ERR_LAUNCH;
  }
  const pi::Table dtable = {static_cast<const pi::Image *>(batch), nstreams};
  // (a window without a header uses at least 10 bits together with the iteration in front of it: 2 * size + 2 iterations bound the walk)
  PGDVS_LAUNCH("png_inflate", png_inflate_kernel, dim3((unsigned)nstreams), dim3(T), 0, st, dtable, static_cast<const uint8_t *>(batch),
               static_cast<uint8_t *>(workspace), status, sub_bytes * 8, (int)(2 * max_size + 2));
  if (int rc = png_unfilter_launch(dtable, static_cast<uint8_t *>(workspace), status, max_rows, max_width, st)) return rc;
  return check_launch("pgdvs_png_decode");
}
