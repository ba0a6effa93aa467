// Wavefront-level primitives of libpgdvs_hip.so: the one scan, the two butterfly reductions, the block-wide exclusive
// offset built on the scan, the run-aggregated tile counters and the DPP maximum.  Everything here is written for the
// 64-wide wavefront of gfx950 (kWave) and must be called by ALL 64 lanes of a wavefront together (callers pad their loops
// to whole wavefronts and pass a neutral value for lanes without work).
//
// Floats: the direction of a butterfly fixes the order of the operations and with it the bits of a sum.  A site that
// reduced "down" (__shfl_down: result in lane 0) stays on wave_reduce_down, a site that reduced over "all" (__shfl_xor:
// result in every lane) stays on wave_reduce_all; never swap one for the other, and keep the operands the way round the
// functors apply them, op(mine, other): fminf / fmaxf are not symmetric on NaN.
//
// Left alone on purpose -- these are not the idioms above, do not route them through this header:
//  - the partial-width butterflies of the MFMA layouts (gnt_mfma.h: steps 16 and 32 only; gnt_view.hip: step 32 only);
//  - the width-8 shuffles that pack eight lanes' words in static_agg.hip (agg_bits kernels);
//  - the in-register array trees of knn.hip and knn_grid.hip (they merge per-lane arrays, not one value per lane);
//  - the halving butterfly of cotracker.hip (corr_lookup_kernel: 32 values per lane in, one finished sum per lane out);
//  - block_partials in eval_common.h: the same tree as wave_sum_down, spelled out, because two metric kernels allocate
//    more registers through the helper.
// Block offsets that use wave_incl_scan with cross-wavefront lines of their own instead of block_excl_scan: those that
// need more from the totals (compact_gather_bbox, grid_rank, grid_scan, stat_select_block, raster_tile, select_digits),
// and compact_scan, compact_scatter, grid_sample and raster_scan, whose register allocation the helper's unrolled
// predicated sum changes.
#pragma once
#include "common.h"

namespace pgdvs {

// ---- operations for the reductions: op(mine, other) ----------------------------------------------------------------
struct OpSum {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMin {  // integers
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct OpMax {  // integers
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct OpFmin {
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct OpFmax {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// Reduction towards lane 0 (steps 32, 16, ..., 1 of __shfl_down).  All 64 lanes call; the result is in LANE 0 ONLY.
template <class Op, class T> __device__ __forceinline__ T wave_reduce_down(T x, Op op = Op()) {
  for (int off = kWave / 2; off > 0; off >>= 1) x = op(x, __shfl_down(x, off, kWave));
  return x;
}

// Butterfly over all lanes (steps 32, 16, ..., 1 of __shfl_xor).  All 64 lanes call; EVERY lane holds the result.
template <class Op, class T> __device__ __forceinline__ T wave_reduce_all(T x, Op op = Op()) {
  for (int off = kWave / 2; off > 0; off >>= 1) x = op(x, __shfl_xor(x, off, kWave));
  return x;
}

// x + shuffled, in that order.  All 64 lanes call; the sum is in lane 0 only (down) / in every lane (all).
template <class T> __device__ __forceinline__ T wave_sum_down(T x) { return wave_reduce_down<OpSum>(x); }
template <class T> __device__ __forceinline__ T wave_sum_all(T x) { return wave_reduce_all<OpSum>(x); }

// Inclusive scan over the wavefront (int, unsigned, uint32_t).  All 64 lanes call; lane l holds x[0] + ... + x[l], lane 63
// the wavefront's total.
template <class T> __device__ __forceinline__ T wave_incl_scan(T x) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int off = 1; off < kWave; off <<= 1) {
    const T y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  return x;
}

// Inclusive scans under any of the operations above (OpMax for "the last run start at or before me", OpMin for "the first
// one at or after me": the segmented scans of png_deflate.hip).  All 64 lanes call.  up: lane l holds op over lanes 0 .. l;
// down: over lanes l .. 63.
template <class Op, class T> __device__ __forceinline__ T wave_incl_scan_up(T x, Op op = Op()) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int off = 1; off < kWave; off <<= 1) {
    const T y = __shfl_up(x, off, kWave);
    if (lane >= off) x = op(x, y);
  }
  return x;
}
template <class Op, class T> __device__ __forceinline__ T wave_incl_scan_down(T x, Op op = Op()) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int off = 1; off < kWave; off <<= 1) {
    const T y = __shfl_down(x, off, kWave);
    if (lane + off < kWave) x = op(x, y);
  }
  return x;
}

// The value of the lane in front (wave_shr:1 through the DPP path, no LDS round trip): lane l holds lane l - 1's x, lane 0
// its own.  All 64 lanes call.  The skewed row pass of png_unfilter.hip hands a pixel from row to row with it.
__device__ __forceinline__ uint32_t wave_prev_lane(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x138, 0xf, 0xf, false);
}

// Block-wide exclusive offset of `c` (int, or unsigned where the sums may wrap) in thread order, for a block of kWaves
// whole wavefronts; `total` = the block's sum (in every thread).  Every thread of the block calls it: it contains ONE __syncthreads().  The caller owns
// s_wsum[kWaves] (shared memory) and puts a barrier of its own before the array is written again.
// (The value type is s_wsum's: `c` converts to it, as it did when the helper was int alone.)
template <class T> struct scan_value { using type = T; };
template <int kWaves, class T> __device__ __forceinline__ T block_excl_scan(const typename scan_value<T>::type c, T *s_wsum, T &total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const T x = wave_incl_scan(c);
  if (lane == kWave - 1) s_wsum[wave] = x;
  __syncthreads();
  T wave_off = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) wave_off += s_wsum[w];
    total += s_wsum[w];
  }
  return wave_off + x - c;
}

// maximum over the wavefront as a scalar: DPP butterflies inside each row of 16 lanes, row
// broadcasts across rows (the total lands in lane 63), no LDS round trips.  All 64 lanes call; every lane gets the result.
__device__ __forceinline__ int wave_max_i32_scalar(int v) {
  int t;
  t = __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  v = t > v ? t : v;
  t = __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  v = t > v ? t : v;
  t = __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false);  // row_half_mirror
  v = t > v ? t : v;
  t = __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false);  // row_mirror
  v = t > v ? t : v;
  t = __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v = t > v ? t : v;
  t = __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  v = t > v ? t : v;
  return __builtin_amdgcn_readlane(v, 63);
}

// Wave-aggregated tile counter update.  Clouds arrive in the raster order of their source
// frames, so consecutive lanes of a wavefront mostly hit the same tile: lanes form RUNS of
// equal tile id, the first lane of each run adds the run length for all of them, and every
// run leader is active in ONE atomic wave-instruction (the atomic units are paced per
// instruction, not per lane).  Any order is correct -- less coherent input only means
// shorter runs.  Returns the slot reserved for this lane (fill) or nothing (count).
struct RunInfo {
  int leader;   // lane index of this lane's run leader
  int length;   // run length (valid on the leader)
  bool is_leader;
};

// PRECONDITION: all 64 lanes of the wavefront call it together (callers pad their loops to whole wavefronts and pass
// t < 0 for lanes without work).  An inactive left neighbour leaves the DPP read at the lane's own value; the ballot of
// active lanes below makes such a lane a leader anyway, so a partial wavefront still gets correct (shorter) runs.
__device__ __forceinline__ RunInfo wave_runs(int t) {
  const int lane = threadIdx.x & 63;
  // wave_shr:1 -- lane i reads lane i-1 through the DPP path (no LDS round trip); lane 0 is a leader anyway
  int prev = __builtin_amdgcn_update_dpp(t, t, 0x138, 0xf, 0xf, false);
  const unsigned long long act = __ballot(1);
  bool lead = lane == 0 || prev != t || !((act >> (lane ? lane - 1 : 0)) & 1ull);
  unsigned long long L = __ballot(lead);
  RunInfo r;
  r.is_leader = lead;
  unsigned long long below = L & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));  // leaders at or below this lane
  r.leader = 63 - __builtin_clzll(below);
  unsigned long long above = lane == 63 ? 0ull : (L >> (lane + 1));  // leaders after this lane
  r.length = above ? (int)__builtin_ctzll(above) + 1 : 64 - lane;
  return r;
}

__device__ __forceinline__ void wave_tile_count(int32_t *__restrict__ counter, int t) {
  RunInfo r = wave_runs(t);
  if (r.is_leader && t >= 0)
    __hip_atomic_fetch_add(&counter[t], r.length, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int wave_tile_reserve(int32_t *__restrict__ counter, int t) {
  const int lane = threadIdx.x & 63;
  RunInfo r = wave_runs(t);
  int base = 0;
  if (r.is_leader && t >= 0) base = atomicAdd(&counter[t], r.length);
  base = __shfl(base, r.leader, 64);
  return base + (lane - r.leader);
}

}  // namespace pgdvs
