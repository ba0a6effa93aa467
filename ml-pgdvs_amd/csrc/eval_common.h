// Shared by the metric kernels (eval.hip, eval_ssim.hip, lpips.hip, eval_dycheck.hip): the evaluator's quantisation
// (pgdvs/engines/evaluator_pgdvs.py:52-77), so that every metric sees the same 8-bit images, and the two fixed-order float64
// reductions that make the metric sums independent of scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "quant8.h"
#include "wave.h"

namespace pgdvs {

// x.clamp(0, 1) -> nan_to_num(nan=0) -> (x * 255).byte(): the 8-bit code, fp32 like torch
__device__ __forceinline__ uint32_t quantise_code(float x) { return quantise_truncate(x); }

// ... .float() / 255.0
__device__ __forceinline__ float quantise_u8(float x) { return (float)quantise_code(x) / 255.0f; }

// One block's partials row: each of the kSums values is summed over a wave by a fixed shuffle tree, the waves' totals go to
// red[wave][k], and thread k < kSums adds waves 0, 1, ... in order and writes row[k].  Every thread of the block calls this
// with tid = threadIdx.x (passed in: a kernel that keeps its own copy keeps its register budget).
template <int kSums, int kThreads>
__device__ __forceinline__ void block_partials(int tid, const double (&v)[kSums], double (&red)[kThreads / kWave][kSums], double *row) {
  const int lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double s = v[k];
    // (wave_sum_down's tree, spelled out: through the helper eval_partials and dycheck_lpips_upsample allocate more registers)
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid < kSums) {
    double s = 0.0;
    for (int w = 0; w < kThreads / kWave; ++w) s += red[w][tid];
    row[tid] = s;
  }
}

// The ordered cross-block sum of one wave: lane l adds p[b * stride] for the blocks b = b0 + l, b0 + l + 64, ... below b1 in
// order, then a fixed shuffle tree; the total is in lane 0.
__device__ __forceinline__ double ordered_block_sum(const double *__restrict__ p, int b0, int b1, int stride) {
  double v = 0.0;
  for (int b = b0 + (int)(threadIdx.x & (kWave - 1)); b < b1; b += kWave) v += p[(size_t)b * stride];
  return wave_sum_down(v);
}

}  // namespace pgdvs
