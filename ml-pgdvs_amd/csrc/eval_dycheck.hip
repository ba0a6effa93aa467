// SURVEY 8f-1, the evaluator's second metric protocol, quant_type "dycheck_iphone" (pgdvs/engines/evaluator_pgdvs.py:282-409
// obtain_quantitative_dycheck_iphone through pgdvs/utils/dycheck/metrics.py:63-230), for one view: PSNR, SSIM and LPIPS with
// a full mask and with the covisibility mask eval_mask[H,W,1].
//
// psnr_ssim  ONE pass per view.  The PSNR pass's 8-bit quantisation (eval_common.h); the squared differences and the mask sum of
//            masked_mean (metrics.py:63-90: sum(d^2 m) / max(sum(m broadcast to 3 channels), 1e-6)) in float64; and the two
//            partial-convolution SSIM maps (metrics.py:93-186, modelled on tf.image.ssim: an 11-tap Gaussian with sigma 1.5,
//            applied separably with mode "valid", first along W, then along H; each pass forms
//            z' = conv(z m, f) 11 / conv(m, 1) where conv(m, 1) != 0 and 0 elsewhere, and passes on the mask conv(m, 1) != 0)
//            for the full mask and the covisibility mask.  Blocks of blockIdx.y = 0 run the full mask, blockIdx.y = 1 the
//            covisibility mask and the PSNR sums.  A block owns a 32 x 32 tile of the (H - 10) x (W - 10) map: its 42 x 42
//            haloed input tile sits in LDS, the W pass writes its 42 x 32 moments to LDS, and the H pass reads them back.
//            The inputs are the fp32 quantised values; moments, map and sums are float64, the sums in a fixed order.
// lpips      lpips 0.1.4 LPIPS(net="alex", spatial=True), version "0.1" (so the ScalingLayer IS applied), called as
//            metrics.py:189-230 calls it: im2tensor(img m, factor=1/2) = 2 img m - 1 of the quantised images, AlexNet
//            relu1..relu5 (lpips.hip's backbone, here on FOUR images: gt, pred, gt m, pred m), normalize_tensor, the squared
//            difference and the 1x1 lin_k per pixel for both pairs, each lin map upsampled to H x W (bilinear,
//            align_corners=False, lpips 0.1.4's size-based source coordinate), summed over the layers, then masked_mean with
//            the full mask (unmasked pair) and with eval_mask (masked pair).
#include <cmath>

#include "common.h"
#include "eval_common.h"
#include "lpips_net.h"

namespace pgdvs {

// ---------------------------------------------------------------- PSNR + SSIM
constexpr int kDcTaps = 11, kDcHalo = kDcTaps - 1;
constexpr int kDcT = 32;                      // output tile: 32 x 32
constexpr int kDcIn = kDcT + kDcHalo;          // 42 x 42 haloed input tile
constexpr int kDcInPitch = kDcIn + 1, kDcHPitch = kDcT + 1;
constexpr int kDcThreads = 256;
constexpr int kDcRows = kDcT / (kDcThreads / kDcT);  // H pass: 4 output rows per thread
constexpr int kDcSums = 4;                      // per block: sum S, sum d2, sum d2 m, sum m
constexpr int kDcMoments = 5;                   // a, b, a^2, b^2, a b
static_assert(kDcRows * (kDcThreads / kDcT) == kDcT, "the H pass covers the tile");

struct DcFilter {
  double f[kDcTaps];
};

// the value of moment j (a, b, a^2, b^2, a b) at one pixel; the products of two fp32 values are exact in float64
__device__ __forceinline__ double dc_moment(int j, float a, float b) {
  return j == 0 ? (double)a : j == 1 ? (double)b : j == 2 ? (double)a * (double)a : j == 3 ? (double)b * (double)b : (double)a * (double)b;
}

__global__ void __launch_bounds__(kDcThreads)
dycheck_ssim_partials_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask, int H, int W,
                             int tiles_x, int tiles_y, DcFilter filt, double *__restrict__ partials) {
  __shared__ float qa[kDcIn][kDcInPitch], qb[kDcIn][kDcInPitch], mk[kDcIn][kDcInPitch];
  __shared__ double msum[kDcIn][kDcHPitch];  // conv(m, 1) of the W pass
  __shared__ double hz[kDcIn][kDcHPitch];    // z' of the W pass, one moment at a time
  __shared__ double red[kDcThreads / kWave][kDcSums];

  const int tid = threadIdx.x;
  const bool covis = blockIdx.y == 1;
  const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
  const int x0 = tx * kDcT, y0 = ty * kDcT;
  const int Ho = H - kDcHalo, Wo = W - kDcHalo;
  const uint32_t P = (uint32_t)H * (uint32_t)W;
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const double ntaps = (double)kDcTaps;

  // ---- the mask of the haloed tile (the full mask: 1 on the image) and its W-pass sums.  Elements past the image edge are 0;
  // only outputs outside the valid map read them, and those are discarded.
  for (int e = tid; e < kDcIn * kDcIn; e += kDcThreads) {
    const int r = e / kDcIn, q = e - r * kDcIn;
    const int gy = y0 + r, gx = x0 + q;
    const bool in = gy < H && gx < W;
    mk[r][q] = in ? (covis ? mask[(uint32_t)gy * (uint32_t)W + (uint32_t)gx] : 1.0f) : 0.0f;
  }
  __syncthreads();
  for (int t = tid; t < kDcIn * kDcT; t += kDcThreads) {
    const int r = t / kDcT, x = t - r * kDcT;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kDcTaps; ++k) s += (double)mk[r][x + k];
    msum[r][x] = s;
  }

  // The moments, the map entry and this thread's <= 12 entries are float64.  In fp32 the variances mu[2] - mu00 of a flat image
  // are pure rounding (the entry then lands anywhere within 7e-5 of its value, by the order of the taps alone), a steep ramp
  // loses 4.5e-6 to the eleven sequential taps, and an fp32 sum of 12 entries near 1 is off by 1.8e-7 on a constant map.
  double ssim = 0.0;
  double psnr[3] = {0.0, 0.0, 0.0};
  const int vx = tid % kDcT, vr0 = (tid / kDcT) * kDcRows;
  for (int c = 0; c < 3; ++c) {
    // ---- quantised inputs of the haloed tile; the covisibility blocks also sum PSNR's terms over the pixels they own
    // (the tile's 32 x 32 core, plus the halo past the last tile row / column: every pixel exactly once)
    float pd = 0.0f, pdm = 0.0f, pm = 0.0f;
    for (int e = tid; e < kDcIn * kDcIn; e += kDcThreads) {
      const int r = e / kDcIn, q = e - r * kDcIn;
      const int gy = y0 + r, gx = x0 + q;
      float a = 0.0f, b = 0.0f;
      if (gy < H && gx < W) {
        const uint32_t p = (uint32_t)gy * (uint32_t)W + (uint32_t)gx;
        a = quantise_u8(gt[p * 3u + (uint32_t)c]);    // img0 = ground truth [H,W,3]
        b = quantise_u8(pred[(uint32_t)c * P + p]);  // img1 = prediction, planar [3,H,W]
        if (covis && (r < kDcT || ty == tiles_y - 1) && (q < kDcT || tx == tiles_x - 1)) {
          const float d = a - b, d2 = d * d, m = mk[r][q];
          pd += d2;
          pdm += d2 * m;
          pm += m;
        }
      }
      qa[r][q] = a;
      qb[r][q] = b;
    }
    psnr[0] += (double)pd;
    psnr[1] += (double)pdm;
    if (c == 0) psnr[2] += (double)pm;
    __syncthreads();
    // ---- one moment at a time: the W pass (42 rows x 32 outputs) to LDS, then the H pass, one column x 4 output rows per thread
    double mu[kDcMoments][kDcRows];
#pragma unroll
    for (int j = 0; j < kDcMoments; ++j) {
      for (int t = tid; t < kDcIn * kDcT; t += kDcThreads) {
        const int r = t / kDcT, x = t - r * kDcT;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kDcTaps; ++k) s += filt.f[k] * (dc_moment(j, qa[r][x + k], qb[r][x + k]) * (double)mk[r][x + k]);
        const double ms = msum[r][x];
        hz[r][x] = ms != 0.0 ? s * ntaps / ms : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int o = 0; o < kDcRows; ++o) {
        const int y = vr0 + o;
        double s = 0.0, cnt = 0.0;
#pragma unroll
        for (int k = 0; k < kDcTaps; ++k) {
          const double m = msum[y + k][vx] != 0.0 ? 1.0 : 0.0;
          cnt += m;
          s += filt.f[k] * (hz[y + k][vx] * m);
        }
        mu[j][o] = cnt != 0.0 ? s * ntaps / cnt : 0.0;
      }
      __syncthreads();  // (the next moment, or the next channel, overwrites the moments and the tile)
    }
#pragma unroll
    for (int o = 0; o < kDcRows; ++o) {
      if (y0 + vr0 + o < Ho && x0 + vx < Wo) {
        const double mu00 = mu[0][o] * mu[0][o], mu11 = mu[1][o] * mu[1][o], mu01 = mu[0][o] * mu[1][o];
        const double s00 = fmax(0.0, mu[2][o] - mu00), s11 = fmax(0.0, mu[3][o] - mu11);
        double s01 = mu[4][o] - mu01;
        const double sg = s01 > 0.0 ? 1.0 : (s01 < 0.0 ? -1.0 : 0.0);
        s01 = sg * fmin(sqrt(s00 * s11), fabs(s01));
        const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
        const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
        ssim += numer / denom;  // (IEEE division: an unmasked window gives exactly c1 c2 / (c1 c2) = 1)
      }
    }
  }
  const double v[kDcSums] = {ssim, psnr[0], psnr[1], psnr[2]};
  block_partials<kDcSums, kDcThreads>(tid, v, red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kDcSums);
}

// fixed-order final sums (wave k reduces one sum with ordered_block_sum) into the row: sum d2, sum d2 m, sum S (full), 3 H W,
// 3 sum m, sum S (covisible), *count_dev, *status_dev
__global__ void __launch_bounds__(5 * kWave)
dycheck_ssim_final_kernel(const double *__restrict__ partials, int n_blocks, double count, const int64_t *__restrict__ count_dev,
                          const int32_t *__restrict__ status_dev, double *__restrict__ sums) {
  // wave k -> (the mask's blocks, partial slot, row slot): 0 d2, 1 d2 m, 2 S full, 3 m, 4 S covisible
  const int k = threadIdx.x / kWave;
  const int src_mask = k == 2 ? 0 : 1, src_slot = k == 0 ? 1 : (k == 1 ? 2 : (k == 3 ? 3 : 0)), dst = k < 3 ? k : k + 1;
  const double v = ordered_block_sum(partials + (size_t)src_mask * n_blocks * kDcSums + src_slot, 0, n_blocks, kDcSums);
  if ((threadIdx.x & (kWave - 1)) == 0) sums[dst] = k == 3 ? 3.0 * v : v;
  if (threadIdx.x == 0) {
    sums[3] = count;
    sums[6] = count_dev ? (double)*count_dev : -1.0;
    sums[7] = status_dev ? (double)*status_dev : 0.0;
  }
}

static int dycheck_tiles(int n) { return (n - kDcHalo + kDcT - 1) / kDcT; }

// ---------------------------------------------------------------- LPIPS
constexpr int kDlImages = 4;  // gt, pred, gt m, pred m
constexpr int kDlThreads = 256;
constexpr int kDlFinalBlocks = 512;
constexpr int kDlSums = 3;  // sum v (unmasked pair), sum v m (masked pair), sum m
// lpips 0.1.4 ScalingLayer (lpips/lpips.py): (x - shift) / scale
__constant__ float kDlShift[3] = {-.030f, -.088f, -.188f};
__constant__ float kDlScale[3] = {.458f, .448f, .450f};

// quantised images -> x[4][3][H][W]: gt, pred, gt m, pred m, each im2tensor(., factor=1/2) = . / 0.5 - 1, then the ScalingLayer
__global__ void __launch_bounds__(kDlThreads)
dycheck_lpips_prep_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask, int P,
                          float *__restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float m = mask[i];
  const size_t plane = (size_t)P, img = 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float g = quantise_u8(gt[(size_t)i * 3 + c]), p = quantise_u8(pred[(size_t)c * P + i]);
    const float sh = kDlShift[c], sc = kDlScale[c];
    float *xc = x + (size_t)c * plane + i;
    xc[0] = (g / 0.5f - 1.0f - sh) / sc;
    xc[img] = (p / 0.5f - 1.0f - sh) / sc;
    xc[2 * img] = ((g * m) / 0.5f - 1.0f - sh) / sc;
    xc[3 * img] = ((p * m) / 0.5f - 1.0f - sh) / sc;
  }
}

struct DlHeadLayer {
  const float *feat;  // [4][C][h][w]
  const float *lin;   // [C]
  float *out;         // [2][h][w]: the lin map of the pair (0, 1), then of the pair (2, 3)
  int C, h, w, block0;
};
struct DlHeadArgs {
  DlHeadLayer l[kLpLayers];
};

// per layer, pixel and pair: normalize_tensor of both images (f / (sqrt(sum_c f^2) + 1e-10)), the squared difference and lin_k
__global__ void __launch_bounds__(kDlThreads) dycheck_lpips_head_kernel(DlHeadArgs a) {
  int L = 0;
#pragma unroll
  for (int k = 1; k < kLpLayers; ++k)
    if ((int)blockIdx.x >= a.l[k].block0) L = k;
  const DlHeadLayer ly = a.l[L];
  const int hw = ly.h * ly.w;
  const int t = ((int)blockIdx.x - ly.block0) * kDlThreads + (int)threadIdx.x;
  if (t >= 2 * hw) return;
  const int pair = t / hw, i = t - pair * hw;
  const float *f0 = ly.feat + (size_t)(2 * pair) * ly.C * hw + i, *f1 = f0 + (size_t)ly.C * hw;
  float n0 = 0.0f, n1 = 0.0f;
  for (int c = 0; c < ly.C; ++c) {
    const float a0 = f0[(size_t)c * hw], a1 = f1[(size_t)c * hw];
    n0 += a0 * a0;
    n1 += a1 * a1;
  }
  const float d0 = sqrtf(n0) + 1e-10f, d1 = sqrtf(n1) + 1e-10f;
  float d = 0.0f;
  for (int c = 0; c < ly.C; ++c) {
    const float e = f0[(size_t)c * hw] / d0 - f1[(size_t)c * hw] / d1;
    d += ly.lin[c] * (e * e);
  }
  ly.out[t] = d;
}

struct DlFinalArgs {
  const float *map[kLpLayers];  // [2][h][w] per layer
  int h[kLpLayers], w[kLpLayers];
  const float *mask;  // [H][W]
  int H, W;
};

// torch's bilinear source index with align_corners=False and an output size (UpSample.h area_pixel_compute_source_index with
// scale = (float)in / out): src = max(scale (dst + 0.5) - 0.5, 0), i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1),
// lambda1 = src - i0
__device__ __forceinline__ void dl_bilinear(int dst, int in, int out, int &i0, int &i1, float &l0, float &l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i0 = i0 < in - 1 ? i0 : in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
  l0 = 1.0f - l1;
}

// per output pixel: v = sum over the layers (0..4, in order) of the upsampled lin maps, for both pairs; then the fixed
// grid-stride float64 partials of sum v0, sum v1 m, sum m
__global__ void __launch_bounds__(kDlThreads) dycheck_lpips_upsample_kernel(DlFinalArgs a, double *__restrict__ partials) {
  __shared__ double red[kDlThreads / kWave][kDlSums];
  const int P = a.H * a.W;
  double acc[kDlSums] = {0.0, 0.0, 0.0};
  for (int p = blockIdx.x * kDlThreads + threadIdx.x; p < P; p += kDlFinalBlocks * kDlThreads) {
    const int Y = p / a.W, X = p - Y * a.W;
    float v0 = 0.0f, v1 = 0.0f;
#pragma unroll
    for (int k = 0; k < kLpLayers; ++k) {
      int y0, y1, x0, x1;
      float hy0, hy1, wx0, wx1;
      dl_bilinear(Y, a.h[k], a.H, y0, y1, hy0, hy1);
      dl_bilinear(X, a.w[k], a.W, x0, x1, wx0, wx1);
      const int hw = a.h[k] * a.w[k];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float *m = a.map[k] + (size_t)q * hw;
        const float t0 = m[y0 * a.w[k] + x0] * wx0 + m[y0 * a.w[k] + x1] * wx1;
        const float t1 = m[y1 * a.w[k] + x0] * wx0 + m[y1 * a.w[k] + x1] * wx1;
        const float u = t0 * hy0 + t1 * hy1;
        if (q == 0) v0 = k == 0 ? u : v0 + u;
        else v1 = k == 0 ? u : v1 + u;
      }
    }
    const float mm = a.mask[p];
    acc[0] += (double)v0;
    acc[1] += (double)(v1 * mm);
    acc[2] += (double)mm;
  }
  block_partials<kDlSums, kDlThreads>(threadIdx.x, acc, red, partials + (size_t)blockIdx.x * kDlSums);
}

// the row: LPIPS full, LPIPS covisible (masked_mean: sum / max(sum m, 1e-6)), sum v0, H W, sum v1 m, sum m, 0, 0
__global__ void __launch_bounds__(kDlSums * kWave)
dycheck_lpips_final_kernel(const double *__restrict__ partials, double pixels, double *__restrict__ sums) {
  __shared__ double tot[kDlSums];
  const int k = threadIdx.x / kWave;
  const double v = ordered_block_sum(partials + k, 0, kDlFinalBlocks, kDlSums);
  if ((threadIdx.x & (kWave - 1)) == 0) tot[k] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[0] = tot[0] / (pixels > 1e-6 ? pixels : 1e-6);
    sums[1] = tot[1] / (tot[2] > 1e-6 ? tot[2] : 1e-6);
    sums[2] = tot[0];
    sums[3] = pixels;
    sums[4] = tot[1];
    sums[5] = tot[2];
    sums[6] = 0.0;
    sums[7] = 0.0;
  }
}

struct DlPlan {
  LpipsNetPlan net;  // x[4,3,H,W] and the backbone's maps
  int64_t off_map[kLpLayers], off_part, total;
  int head_block0[kLpLayers + 1];
};

static bool dycheck_lpips_plan(int H, int W, DlPlan &pl) {
  if (!lpips_net_plan(H, W, kDlImages, pl.net)) return false;
  int64_t o = pl.net.end;
  int nb = 0;
  for (int k = 0; k < kLpLayers; ++k) {
    const int64_t hw = (int64_t)pl.net.h[k] * pl.net.w[k];
    pl.off_map[k] = o;
    o += align_up(2 * hw * 4, 256);
    pl.head_block0[k] = nb;
    nb += (int)((2 * hw + kDlThreads - 1) / kDlThreads);
  }
  pl.head_block0[kLpLayers] = nb;
  pl.off_part = o;
  o += align_up((int64_t)kDlFinalBlocks * kDlSums * 8, 256);
  pl.total = o;
  return true;
}

}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_dycheck_psnr_ssim_workspace_bytes(int H, int W) {
  if (H < kDcTaps || W < kDcTaps || (int64_t)H * W >= (1ll << 30)) {
    set_error("pgdvs_dycheck_psnr_ssim_workspace_bytes: the image (%d x %d) is outside the 11 x 11 window's range", H, W);
    return PGDVS_ERR_INVALID;
  }
  return (int64_t)2 * dycheck_tiles(H) * dycheck_tiles(W) * kDcSums * 8;
}

PGDVS_API int pgdvs_dycheck_psnr_ssim_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hw, int H, int W,
                                           const int64_t *count_dev, const int32_t *status_dev, double *sums, void *workspace,
                                           int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_planar && gt_hwc && mask_hw && sums && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30),
                "pgdvs_dycheck_psnr_ssim_sums: bad arguments");
  PGDVS_REQUIRE(H >= kDcTaps && W >= kDcTaps, "pgdvs_dycheck_psnr_ssim_sums: the image (%d x %d) is smaller than the 11 x 11 window",
                H, W);
  if (!workspace || workspace_bytes < pgdvs_dycheck_psnr_ssim_workspace_bytes(H, W)) {
    set_error("pgdvs_dycheck_psnr_ssim_sums: workspace too small");
    return PGDVS_ERR_WORKSPACE;
  }
  // the 1-D Gaussian of metrics.py:148-153 in float64
  DcFilter filt;
  {
    double g[kDcTaps], s = 0.0;
    for (int k = 0; k < kDcTaps; ++k) {
      const double u = (k - kDcTaps / 2) / 1.5;
      g[k] = std::exp(-0.5 * u * u);
      s += g[k];
    }
    for (int k = 0; k < kDcTaps; ++k) filt.f[k] = g[k] / s;
  }
  hipStream_t st = as_stream(stream);
  double *partials = reinterpret_cast<double *>(workspace);
  const int tiles_x = dycheck_tiles(W), tiles_y = dycheck_tiles(H);
  const int nb = tiles_x * tiles_y;
  PGDVS_LAUNCH("dycheck_ssim_partials", dycheck_ssim_partials_kernel, dim3((unsigned)nb, 2), dim3(kDcThreads), 0, st, pred_planar, gt_hwc,
               mask_hw, H, W, tiles_x, tiles_y, filt, partials);
  PGDVS_LAUNCH("dycheck_ssim_final", dycheck_ssim_final_kernel, dim3(1), dim3(5 * kWave), 0, st, (const double *)partials, nb,
               3.0 * (double)H * (double)W, count_dev, status_dev, sums);
  return check_launch("dycheck_psnr_ssim_sums");
}

PGDVS_API int64_t pgdvs_dycheck_lpips_workspace_bytes(int H, int W) {
  DlPlan pl;
  if (!dycheck_lpips_plan(H, W, pl)) {
    set_error("pgdvs_dycheck_lpips_workspace_bytes: the image (%d x %d) is outside the backbone's range (H, W >= 31, H W < 2^26)", H, W);
    return PGDVS_ERR_INVALID;
  }
  return pl.total;
}

PGDVS_API int pgdvs_dycheck_lpips(const float *pred_planar, const float *gt_hwc, const float *mask_hw, int H, int W, const float *conv_weights,
                                  const float *conv_biases, const float *lin_weights, double *sums, void *workspace, int64_t workspace_bytes,
                                  pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_planar && gt_hwc && mask_hw && conv_weights && conv_biases && lin_weights && sums && H > 0 && W > 0,
                "pgdvs_dycheck_lpips: bad arguments");
  DlPlan pl;
  PGDVS_REQUIRE(dycheck_lpips_plan(H, W, pl),
                "pgdvs_dycheck_lpips: the image (%d x %d) is outside the backbone's range (H, W >= 31, H W < 2^26)", H, W);
  if (!workspace || workspace_bytes < pl.total) {
    set_error("pgdvs_dycheck_lpips: workspace too small");
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  const float *wk[kLpLayers], *bk[kLpLayers], *lk[kLpLayers];
  lpips_net_weights(conv_weights, conv_biases, lin_weights, wk, bk, lk);
  const int P = H * W;
  PGDVS_LAUNCH("dycheck_lpips_prep", dycheck_lpips_prep_kernel, dim3((unsigned)((P + kDlThreads - 1) / kDlThreads)), dim3(kDlThreads), 0, st,
               pred_planar, gt_hwc, mask_hw, P, reinterpret_cast<float *>(ws + pl.net.off_x));
  lpips_net_forward(ws, pl.net, kDlImages, H, W, wk, bk, st);
  DlHeadArgs ha;
  DlFinalArgs fa;
  for (int k = 0; k < kLpLayers; ++k) {
    float *map = reinterpret_cast<float *>(ws + pl.off_map[k]);
    ha.l[k] = DlHeadLayer{reinterpret_cast<const float *>(ws + pl.net.off_relu[k]), lk[k], map, kLpCout[k], pl.net.h[k], pl.net.w[k],
                          pl.head_block0[k]};
    fa.map[k] = map;
    fa.h[k] = pl.net.h[k];
    fa.w[k] = pl.net.w[k];
  }
  fa.mask = mask_hw;
  fa.H = H;
  fa.W = W;
  PGDVS_LAUNCH("dycheck_lpips_head", dycheck_lpips_head_kernel, dim3((unsigned)pl.head_block0[kLpLayers]), dim3(kDlThreads), 0, st, ha);
  double *partials = reinterpret_cast<double *>(ws + pl.off_part);
  PGDVS_LAUNCH("dycheck_lpips_upsample", dycheck_lpips_upsample_kernel, dim3(kDlFinalBlocks), dim3(kDlThreads), 0, st, fa, partials);
  PGDVS_LAUNCH("dycheck_lpips_final", dycheck_lpips_final_kernel, dim3(1), dim3(kDlSums * kWave), 0, st, (const double *)partials,
               (double)H * (double)W, sums);
  return check_launch("dycheck_lpips");
}
