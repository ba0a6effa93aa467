// The two float -> 8-bit rules of the product, stated once: every exported PNG and video frame (png.hip, jpeg.hip) and every
// metric (eval_common.h) quantises through these, so that what is measured is what is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgdvs {

// Both rules: clamp to [0, 1] and scale by 255 in fp32, NaN -> 0; then either round as save_image does or truncate.
__device__ __forceinline__ uint32_t quantise8(float x, bool save_image) {
  if (!(x == x)) return 0u;
  x = fminf(fmaxf(x, 0.0f), 1.0f);
  float v = __fmul_rn(x, 255.0f);
  if (save_image) v = fminf(fmaxf(__fadd_rn(v, 0.5f), 0.0f), 255.0f);
  return (uint32_t)(int)v;
}

// torchvision.utils.save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8), the multiply and the add rounded separately
__device__ __forceinline__ uint32_t quantise_save_image(float x) { return quantise8(x, true); }

// the truncating cast: (x * 255).astype(uint8) of the *_gnt.png writer, (x * 255).byte() of the evaluator
__device__ __forceinline__ uint32_t quantise_truncate(float x) { return quantise8(x, false); }

}  // namespace pgdvs
