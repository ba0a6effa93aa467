// The LPIPS AlexNet backbone of lpips.hip (features[0:12]: implicit-GEMM convolutions on the fp32 matrix instruction and
// 3/2 max-pools), shared by the metric passes that run it: lpips.hip (the NVIDIA protocol, 2 images per view) and
// eval_dycheck.hip (the DyCheck iPhone protocol, 4 images per view).  The kernels live in lpips.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgdvs {

constexpr int kLpLayers = 5;
constexpr int kLpCin[kLpLayers] = {3, 64, 192, 384, 256};
constexpr int kLpCout[kLpLayers] = {64, 192, 384, 256, 256};
constexpr int kLpKs[kLpLayers] = {11, 5, 3, 3, 3};

// the backbone's maps for n_img images of H x W in one workspace, each region rounded up to 256 bytes:
// x[n_img,3,H,W], relu1, pool1, relu2, pool2, relu3, relu4, relu5 (each [n_img,C,h,w] fp32); `end` = the first free byte
struct LpipsNetPlan {
  int h[kLpLayers], w[kLpLayers];  // relu_k map sizes
  int ph[2], pw[2];                // pool1 / pool2 outputs
  int64_t off_x, off_relu[kLpLayers], off_pool[2], end;
};

// false: the image is too small for the backbone (an empty relu5 map) or too large for the 32-bit pixel indices
bool lpips_net_plan(int H, int W, int n_img, LpipsNetPlan &pl);

// the packed weights (include/pgdvs_hip.h, pgdvs_lpips_sums) split per layer
void lpips_net_weights(const float *conv_weights, const float *conv_biases, const float *lin_weights, const float *(&wk)[kLpLayers],
                       const float *(&bk)[kLpLayers], const float *(&lk)[kLpLayers]);

// enqueue conv1 .. conv5 (with the two pools) on the n_img images at ws + pl.off_x
void lpips_net_forward(char *ws, const LpipsNetPlan &pl, int n_img, int H, int W, const float *const (&wk)[kLpLayers],
                       const float *const (&bk)[kLpLayers], hipStream_t st);

}  // namespace pgdvs
