// The Huffman scan of a baseline JPEG, read on the device: pgdvs_jpeg_scan_decode gives the coefficients
// pgdvs_jpeg_entropy_decode gives, bit for bit, from the buffer pgdvs_jpeg_scan_prepare filled (csrc/jpeg_entropy.cpp).
// include/pgdvs_hip.h states the contract, csrc/jpeg_scan_core.h the decoder and why guessed entry states converge; this file
// is the launches.  pgdvs_jpeg_scan_decode_host (csrc/jpeg_entropy.cpp) is the same sequence on the CPU.
//
// A thread owns one subsequence; a workgroup kSubsPerGroup consecutive ones, the scan's six Huffman tables in LDS.
//   sync, launch 0        every subsequence is decoded from its known entry (it begins a restart segment) or from the guess;
//                         then rounds: a thread whose predecessor's exit (in LDS) is not the entry it used decodes again.
//                         Round r makes thread r's exit right relative to the group's first entry, so kSubsPerGroup rounds
//                         always suffice and the loop leaves as soon as a round changes no exit.
//   sync, launch 1 ..     the fix-ups across workgroups: a group's first thread takes the exit the group in front left in
//     ngroups - 1         global memory and the change runs through the group as above.  Launch L makes group L final, so
//                         ngroups - 1 launches always suffice; a launch writes flags[L] when it changed anything, and launch
//                         L + 1 leaves at once where flags[L] is still zero (nothing changed: the states are the fixed
//                         point).  A group reads one word another group may be writing in the same launch: either value is
//                         a state of that subsequence, and a stale one is met again by the next launch, which then runs.
//   first                 the exclusive sum of the blocks each subsequence completed: its first block in the stream.
//   write                 every subsequence once more, verified: its coefficients de-zigzagged into coef (zeroed before), the
//                         DC as the difference; a block that straddles two subsequences is written by both, each its own
//                         zigzag range; blocks beyond what the segment owes are neither written nor checked.  The exit and
//                         the count must be what the synchronisation left, or the status says "not synchronised".
//   dc tile / tiles /     the DC differences summed per component in stream order, from zero at every restart segment: sums
//     apply               within tiles of kDcTile MCUs, the tiles' offsets, then each MCU's running values applied with the
//                         host decoder's 16-bit check.  Unsigned wrap-around sums; the segment's sum is a difference of two.
// Every loop's bound is a launch argument; no workgroup waits for another; the only global atomics are the status word's OR and
// the round statistic's MAX, which nothing waits on.  Every index that comes from the prepared buffer is clamped
// (jscan::sub_range, block_offset, peek32) before it is used.
#include <string.h>

#include "common.h"
#include "jpeg_scan_core.h"
#include "wave.h"

namespace pgdvs {
namespace {

namespace js = jscan;
constexpr int kGroup = js::kSubsPerGroup;
constexpr int kFirstBlock = 1024;

struct Prep {
  const js::Table *tabs;
  const js::Segment *segs;
  const int32_t *sub_segment;
  const uint32_t *words;
};

__device__ __forceinline__ void load_tables(js::Table *lds, const js::Table *src) {
  constexpr int kWords = (int)(sizeof(js::Table) * js::kTables / 4);
  uint32_t *d = reinterpret_cast<uint32_t *>(lds);
  const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
  for (int k = threadIdx.x; k < kWords; k += blockDim.x) d[k] = s[k];
}

__device__ __forceinline__ uint64_t load_state(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_state(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kGroup) jpeg_scan_sync_kernel(Prep p, js::Geo g, uint64_t *__restrict__ state, int32_t *__restrict__ count,
                                                                uint32_t *__restrict__ flags, uint32_t *__restrict__ info, int launch) {
  __shared__ js::Table s_tabs[js::kTables];
  __shared__ uint64_t s_exit[kGroup];
  if (launch >= 1 && blockIdx.x == 0) return;             // (final since launch 0)
  if (launch >= 2 && flags[launch - 1] == 0) return;      // nothing changed in the launch in front
  load_tables(s_tabs, p.tabs);
  const int t = threadIdx.x;
  const int32_t i = (int32_t)blockIdx.x * kGroup + t;
  const bool have = i < g.nsub;
  const js::SubRange r = js::sub_range(g, p.segs, p.sub_segment, have ? i : g.nsub - 1);
  uint64_t entry = js::first_entry(r.begin), ex = js::kInvalid;
  int32_t n = 0;
  __syncthreads();
  if (launch == 0) {
    if (have) ex = js::decode_sub<false>(s_tabs, p.words, g, entry, r.begin, r.end, r.seg_end, g.sub_bits, &n, nullptr);
  } else if (have) {
    if (!r.begins) entry = load_state(state + i - 1);
    ex = load_state(state + i);
    n = count[i];
  }
  s_exit[t] = ex;
  uint32_t rounds = 1;
  bool any = false, decoded = launch == 0;
  for (int rnd = launch ? 0 : 1; rnd < kGroup + 1; ++rnd) {
    __syncthreads();
    const uint64_t fresh = (r.begins || t == 0) ? entry : s_exit[t - 1];
    bool changed = false;
    if (have && (fresh != entry || (launch && rnd == 0 && t == 0))) {  // (a fix-up's first exit may still be a guess's)
      entry = fresh;
      const uint64_t e = js::decode_sub<false>(s_tabs, p.words, g, entry, r.begin, r.end, r.seg_end, g.sub_bits, &n, nullptr);
      changed = e != ex;
      ex = e;
      decoded = true;  // (the count follows the entry even where the exit does not)
    }
    if (!__syncthreads_or(changed)) break;  // (every thread has read its predecessor's word by now)
    if (changed) s_exit[t] = ex;
    any = true;
    ++rounds;
  }
  if (have && decoded) {
    store_state(state + i, ex);
    count[i] = n;
  }
  if (t == 0) {
    if (launch == 0) atomicMax(info, rounds);
    else if (any) flags[launch] = 1;
    if (launch && blockIdx.x == 1) info[1] += 1;  // one thread of one launch at a time
  }
}

__global__ void __launch_bounds__(kFirstBlock) jpeg_scan_first_kernel(const int32_t *__restrict__ count, int32_t *__restrict__ first, int nsub) {
  __shared__ int s_wsum[kFirstBlock / kWave];
  int carry = 0;
  for (int base = 0; base < nsub; base += kFirstBlock) {
    const int i = base + (int)threadIdx.x;
    const int c = i < nsub ? count[i] : 0;
    int total;
    const int off = block_excl_scan<kFirstBlock / kWave>(c, s_wsum, total);
    if (i < nsub) first[i] = carry + off;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) first[nsub] = carry;
}

__global__ void __launch_bounds__(kGroup) jpeg_scan_write_kernel(Prep p, js::Geo g, const uint64_t *__restrict__ state, const int32_t *__restrict__ count,
                                                                 const int32_t *__restrict__ first, int16_t *__restrict__ coef,
                                                                 uint32_t *__restrict__ status) {
  __shared__ js::Table s_tabs[js::kTables];
  load_tables(s_tabs, p.tabs);
  __syncthreads();
  const int32_t i = (int32_t)blockIdx.x * kGroup + (int)threadIdx.x;
  if (i >= g.nsub) return;
  const js::SubRange r = js::sub_range(g, p.segs, p.sub_segment, i);
  int64_t ord = (int64_t)first[i] - first[r.sub_first];
  ord = ord < 0 ? 0 : ord;
  const int64_t owed = (int64_t)r.mcu_count * g.bpm, at = (int64_t)r.mcu_first * g.bpm;
  js::Verify vf;
  vf.coef = coef, vf.err = 0, vf.last_segment = r.last_segment;
  vf.block_end = (int32_t)(at + owed < g.nblocks ? (at + owed < 0 ? 0 : at + owed) : g.nblocks);
  vf.block = (int32_t)(at + ord < vf.block_end ? (at + ord < 0 ? 0 : at + ord) : vf.block_end);
  int32_t n;
  const uint64_t entry = r.begins ? js::first_entry(r.begin) : state[i - (i > 0)];
  const uint64_t e = js::decode_sub<true>(s_tabs, p.words, g, entry, r.begin, r.end, r.seg_end, g.sub_bits, &n, &vf);
  uint32_t err = vf.err;
  if (e != state[i] || n != count[i]) err |= js::kStatusNotSynchronised;
  if (r.ends && ord + n < owed) err |= js::kStatusShort;
  if (err) atomicOr(status, err);
}

// ---- the DC values --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(js::kDcTile) jpeg_dc_tile_kernel(const int16_t *__restrict__ coef, js::Geo g, uint32_t *__restrict__ mcu_prefix,
                                                                   uint32_t *__restrict__ tile_sum) {
  __shared__ uint32_t s_wsum[js::kDcTile / kWave];
  const int32_t m = (int32_t)blockIdx.x * js::kDcTile + (int)threadIdx.x;
  const bool live = m < g.nmcu;
  const int hv = g.h * g.v;
  uint32_t sum[3] = {0, 0, 0};
  if (live) {
    for (int k = 0; k < g.bpm; ++k) {
      const uint32_t d = (uint32_t)(int32_t)coef[js::block_offset(g, m * g.bpm + k)];
      if (k < hv) sum[0] += d;
      else if (k == hv) sum[1] += d;
      else sum[2] += d;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t total;
    const uint32_t off = block_excl_scan<js::kDcTile / kWave>(sum[c], s_wsum, total);
    if (live) mcu_prefix[(int64_t)m * 3 + c] = off;
    if (threadIdx.x == 0) tile_sum[(int64_t)blockIdx.x * 3 + c] = total;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(js::kDcTile) jpeg_dc_tiles_kernel(const uint32_t *__restrict__ tile_sum, uint32_t *__restrict__ tile_off, int ntiles) {
  __shared__ uint32_t s_wsum[js::kDcTile / kWave];
  uint32_t carry[3] = {0, 0, 0};
  for (int base = 0; base < ntiles; base += js::kDcTile) {
    const int i = base + (int)threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t total;
      const uint32_t off = block_excl_scan<js::kDcTile / kWave>(i < ntiles ? tile_sum[(int64_t)i * 3 + c] : 0u, s_wsum, total);
      if (i < ntiles) tile_off[(int64_t)i * 3 + c] = carry[c] + off;
      carry[c] += total;
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(js::kDcTile) jpeg_dc_apply_kernel(int16_t *__restrict__ coef, js::Geo g, const uint32_t *__restrict__ mcu_prefix,
                                                                    const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ status) {
  const int32_t m = (int32_t)blockIdx.x * js::kDcTile + (int)threadIdx.x;
  if (m >= g.nmcu) return;
  const int32_t s = m / g.restart_mcus * g.restart_mcus;  // the segment's first MCU
  const int hv = g.h * g.v;
  int32_t run[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    run[c] = (int32_t)((tile_off[(int64_t)(m / js::kDcTile) * 3 + c] + mcu_prefix[(int64_t)m * 3 + c]) -
                       (tile_off[(int64_t)(s / js::kDcTile) * 3 + c] + mcu_prefix[(int64_t)s * 3 + c]));
  bool range = false;
  for (int k = 0; k < g.bpm; ++k) {
    int16_t *dc = coef + js::block_offset(g, m * g.bpm + k);
    int32_t &v = run[k < hv ? 0 : (k == hv ? 1 : 2)];
    v = (int32_t)((uint32_t)v + (uint32_t)(int32_t)*dc);
    range = range || v < -32768 || v > 32767;
    *dc = (int16_t)v;
  }
  if (range) atomicOr(status, js::kStatusDcRange);
}

int plan(const char *what, const void *prepared_host, int64_t prepared_bytes, int64_t coef_bytes, js::Header *hd, js::Geo *g, js::Workspace *w) {
  PGDVS_REQUIRE(prepared_host != nullptr && prepared_bytes >= (int64_t)sizeof(js::Header), "%s: null or short prepared buffer", what);
  memcpy(hd, prepared_host, sizeof(*hd));
  const char *why = js::check_header(hd, prepared_bytes, coef_bytes < 0 ? hd->coef_bytes : coef_bytes, g);
  PGDVS_REQUIRE(why == nullptr, "%s: %s", what, why);
  js::workspace_layout(*g, w);
  return PGDVS_OK;
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_jpeg_scan_decode_workspace_bytes(const void *prepared_host, int64_t prepared_bytes) {
  js::Header hd;
  js::Geo g;
  js::Workspace w;
  if (plan("pgdvs_jpeg_scan_decode_workspace_bytes", prepared_host, prepared_bytes, -1, &hd, &g, &w)) return -1;
  return w.total;
}

PGDVS_API int pgdvs_jpeg_scan_decode(const void *prepared_host, const void *prepared, int64_t prepared_bytes, int16_t *coef, int64_t coef_bytes,
                                     uint32_t *status, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  js::Header hd;
  js::Geo g;
  js::Workspace w;
  PGDVS_REQUIRE(coef_bytes >= 0, "pgdvs_jpeg_scan_decode: negative coef_bytes");
  if (int rc = plan("pgdvs_jpeg_scan_decode", prepared_host, prepared_bytes, coef_bytes, &hd, &g, &w)) return rc;
  PGDVS_REQUIRE(prepared && coef && status, "pgdvs_jpeg_scan_decode: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 15) == 0 && (reinterpret_cast<uintptr_t>(coef) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                "pgdvs_jpeg_scan_decode: the prepared buffer and coef must be 16-byte aligned, status 4-byte");
  PGDVS_REQUIRE(workspace && workspace_bytes >= w.total && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "pgdvs_jpeg_scan_decode: workspace of %lld bytes, %lld needed (256-byte aligned)", (long long)workspace_bytes, (long long)w.total);
  const hipStream_t st = as_stream(stream);
  const char *base = static_cast<const char *>(prepared);
  Prep p;
  p.tabs = reinterpret_cast<const js::Table *>(base + hd.off_tables);
  p.segs = reinterpret_cast<const js::Segment *>(base + hd.off_segments);
  p.sub_segment = reinterpret_cast<const int32_t *>(base + hd.off_sub_segment);
  p.words = reinterpret_cast<const uint32_t *>(base + hd.off_stream);
  char *ws = static_cast<char *>(workspace);
  uint32_t *flags = reinterpret_cast<uint32_t *>(ws + w.flags), *info = reinterpret_cast<uint32_t *>(ws + w.info);
  uint64_t *state = reinterpret_cast<uint64_t *>(ws + w.state);
  int32_t *count = reinterpret_cast<int32_t *>(ws + w.count), *first = reinterpret_cast<int32_t *>(ws + w.first);
  uint32_t *mcu_prefix = reinterpret_cast<uint32_t *>(ws + w.mcu_prefix), *tile_sum = reinterpret_cast<uint32_t *>(ws + w.tile_sum),
           *tile_off = reinterpret_cast<uint32_t *>(ws + w.tile_off);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)w.head, st);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4, st);
  if (e == hipSuccess) e = fill_async(coef, 0, (size_t)coef_bytes, st);
  if (e != hipSuccess) {
    set_error("pgdvs_jpeg_scan_decode: %s", hipGetErrorString(e));
    return PGDVS_ERR_LAUNCH;
  }
  for (int launch = 0; launch < (w.ngroups > 1 ? w.ngroups : 1); ++launch)
    PGDVS_LAUNCH("jpeg_scan_sync", jpeg_scan_sync_kernel, dim3((unsigned)w.ngroups), dim3(kGroup), 0, st, p, g, state, count, flags, info, launch);
  PGDVS_LAUNCH("jpeg_scan_first", jpeg_scan_first_kernel, dim3(1), dim3(kFirstBlock), 0, st, count, first, g.nsub);
  PGDVS_LAUNCH("jpeg_scan_write", jpeg_scan_write_kernel, dim3((unsigned)w.ngroups), dim3(kGroup), 0, st, p, g, state, count, first, coef, status);
  PGDVS_LAUNCH("jpeg_dc_tile", jpeg_dc_tile_kernel, dim3((unsigned)w.ntiles), dim3(js::kDcTile), 0, st, coef, g, mcu_prefix, tile_sum);
  PGDVS_LAUNCH("jpeg_dc_tiles", jpeg_dc_tiles_kernel, dim3(1), dim3(js::kDcTile), 0, st, tile_sum, tile_off, w.ntiles);
  PGDVS_LAUNCH("jpeg_dc_apply", jpeg_dc_apply_kernel, dim3((unsigned)w.ntiles), dim3(js::kDcTile), 0, st, coef, g, mcu_prefix, tile_off, status);
  return check_launch("pgdvs_jpeg_scan_decode");
}
