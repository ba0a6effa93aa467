// The evaluator's quantisation of an image value (pgdvs/engines/evaluator_pgdvs.py:52-77), shared by the metric kernels
// (eval.hip, eval_ssim.hip) so that PSNR and SSIM see the same 8-bit images.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgdvs {

// x.clamp(0, 1) -> nan_to_num(nan=0) -> (x * 255).byte(): the 8-bit code, fp32 like torch
__device__ __forceinline__ uint32_t quantise_code(float x) {
  x = x != x ? 0.0f : (x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x));
  return (uint32_t)(uint8_t)(x * 255.0f);
}

// ... .float() / 255.0
__device__ __forceinline__ float quantise_u8(float x) { return (float)quantise_code(x) / 255.0f; }

}  // namespace pgdvs
