// SURVEY 8f-1, the evaluator's masked SSIM (pgdvs/engines/evaluator_pgdvs.py:190-283 through
// pgdvs/utils/training.py:316-346 calculate_ssim = skimage 0.20 structural_similarity(full=True, channel_axis=2,
// data_range=2.0) -> sum(S * mask) / (sum(mask) + 1e-8)) as ONE pass per view: the same 8-bit quantisation as the PSNR
// pass (eval_common.h), the five 7x7 box sums of every channel EXACTLY in integers (separable: a horizontal then a
// vertical sliding sum over a haloed tile in LDS, scipy's half-sample-symmetric "reflect" border), S from those sums in
// fp32, and the masked sums in float64 (a thread's 8 rows of one channel are summed in fp32 first).  Upstream this is a
// device-to-host copy and three skimage calls per view, each running 15 float32 box filters on the CPU.
//
// With integer codes a = 255 x, b = 255 y and the window sums Sa, Sb, Saa, Sbb, Sab over the 49 pixels, skimage's
//   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  ux = Sa / (49*255),
//   vxy = 49/48 (uxy - ux uy) = (49 Sab - Sa Sb) / (48*49*255^2)
// is, after cancelling the common scales, (2 Sa Sb + c1)(2 Dab + c2) / ((Sa^2 + Sb^2 + c1)(Daa + Dbb + c2)) with
// Dab = 49 Sab - Sa Sb, c1 = C1 (49*255)^2 and c2 = C2 48*49*255^2.  Every integer there is below 2^31.
#include "common.h"
#include "eval_common.h"

namespace pgdvs {

constexpr int kSsimWin = 7, kSsimHalo = 3;
constexpr int kSsimTW = 64, kSsimTH = 32;  // output tile: 64 columns x 32 rows per block
constexpr int kSsimThreads = 256;
constexpr int kSsimHR = kSsimTH + 2 * kSsimHalo;  // 38 halo rows
constexpr int kSsimHC = kSsimTW + 2 * kSsimHalo;  // 70 halo columns
// odd row pitches: the horizontal pass reads / writes one row per lane, the vertical pass one column per lane, and
// both are then free of bank conflicts
constexpr int kSsimCodePitch = kSsimHC + 1;
constexpr int kSsimSumPitch = kSsimTW + 1;
constexpr int kSsimHSeg = 8;                               // horizontal pass: outputs per task (row segment)
constexpr int kSsimHTasks = kSsimHR * (kSsimTW / kSsimHSeg);  // 304
constexpr int kSsimVSeg = kSsimTH / (kSsimThreads / kSsimTW);  // vertical pass: 8 rows per thread
constexpr int kSsimLoads = (kSsimHR * kSsimHC + kSsimThreads - 1) / kSsimThreads;  // halo elements per thread: 11
constexpr int kSsimSums = 5;  // per block: sum S, sum S m, sum S (1 - m), sum m, sum (1 - m)
static_assert(kSsimTW == 64 && kSsimVSeg * (kSsimThreads / kSsimTW) == kSsimTH, "one column per lane in the vertical pass");
static_assert(kSsimWin * 255 < 65536 && kSsimWin * kSsimWin * 255 < 65536, "two code sums share one 32-bit word");

// scipy.ndimage mode "reflect" (numpy "symmetric"): -1 -> 0, -2 -> 1, n -> n - 1; one reflection suffices for n >= 4.
// The clamp keeps the halo of a tile that lies past the image edge (its outputs are discarded) in bounds.
__device__ __forceinline__ int ssim_reflect(int i, int n) {
  i = i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// issue the loads of one channel's haloed tile (raw values; quantised when they are stored to LDS)
__device__ __forceinline__ void ssim_load_tile(const float *__restrict__ pred, const float *__restrict__ gt, int H, int W, int x0, int y0,
                                               int c, float (&ga)[kSsimLoads], float (&pa)[kSsimLoads]) {
#pragma unroll
  for (int k = 0; k < kSsimLoads; ++k) {
    const int e = threadIdx.x + k * kSsimThreads;
    if (e < kSsimHR * kSsimHC) {
      const int r = e / kSsimHC, q = e - r * kSsimHC;
      const int p = ssim_reflect(y0 - kSsimHalo + r, H) * W + ssim_reflect(x0 - kSsimHalo + q, W);
      ga[k] = gt[(uint32_t)p * 3u + (uint32_t)c];  // (H W < 2^30: every offset fits 32 bits)
      pa[k] = pred[(uint32_t)c * (uint32_t)(H * W) + (uint32_t)p];
    }
  }
}

__global__ void __launch_bounds__(kSsimThreads)
eval_ssim_partials_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask, int H, int W,
                          int tiles_x, float *__restrict__ smap, double *__restrict__ partials) {
  // codes of the haloed tile, a | b << 16 (a = ground truth = img1, b = prediction = img2)
  __shared__ uint32_t codes[kSsimHR][kSsimCodePitch];
  // horizontal 7-sums of the halo rows: packed Sa | Sb << 16, Saa, Sbb, Sab
  __shared__ uint32_t h_ab[kSsimHR][kSsimSumPitch];
  __shared__ int h_aa[kSsimHR][kSsimSumPitch], h_bb[kSsimHR][kSsimSumPitch], h_xy[kSsimHR][kSsimSumPitch];
  __shared__ double red[kSsimThreads / kWave][kSsimSums];

  const int tid = threadIdx.x;
  const int x0 = (blockIdx.x % tiles_x) * kSsimTW, y0 = (blockIdx.x / tiles_x) * kSsimTH;
  const int P = H * W;
  const float c1 = (float)(0.01 * 2.0 * 0.01 * 2.0 * (49.0 * 255.0) * (49.0 * 255.0));
  const float c2 = (float)(0.03 * 2.0 * 0.03 * 2.0 * (48.0 * 49.0 * 255.0 * 255.0));
  double acc[kSsimSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int vj = tid % kSsimTW, vr0 = (tid / kSsimTW) * kSsimVSeg;  // this thread's column / first row in the vertical pass
  const int gx = x0 + vj;
  // software pipeline: the loads of channel c + 1's tile are in flight while channel c is computed, and the mask values of
  // channel c while its horizontal pass runs (one thread has 11 halo elements and 8 mask values per channel)
  float ga[kSsimLoads], pa[kSsimLoads];
  ssim_load_tile(pred, gt, H, W, x0, y0, 0, ga, pa);

  for (int c = 0; c < 3; ++c) {
    float mk[kSsimVSeg];
#pragma unroll
    for (int o = 0; o < kSsimVSeg; ++o) {
      const int gy = y0 + vr0 + o;
      mk[o] = (gx < W && gy < H) ? mask[(uint32_t)(gy * W + gx) * 3u + (uint32_t)c] : 0.0f;
    }
    // ---- codes of the haloed tile
#pragma unroll
    for (int k = 0; k < kSsimLoads; ++k) {
      const int e = tid + k * kSsimThreads;
      if (e < kSsimHR * kSsimHC) {
        const int r = e / kSsimHC;
        codes[r][e - r * kSsimHC] = quantise_code(ga[k]) | (quantise_code(pa[k]) << 16);
      }
    }
    __syncthreads();
    if (c < 2) ssim_load_tile(pred, gt, H, W, x0, y0, c + 1, ga, pa);
    // ---- horizontal sliding sums: one halo row x 8 output columns per task
    for (int t = tid; t < kSsimHTasks; t += kSsimThreads) {
      const int r = t % kSsimHR, q0 = (t / kSsimHR) * kSsimHSeg;
      uint32_t v[kSsimHSeg + kSsimWin - 1];
#pragma unroll
      for (int k = 0; k < kSsimHSeg + kSsimWin - 1; ++k) v[k] = codes[r][q0 + k];
      uint32_t s_ab = 0;
      int s_aa = 0, s_bb = 0, s_xy = 0;
#pragma unroll
      for (int k = 0; k < kSsimHSeg + kSsimWin - 1; ++k) {
        const int a = (int)(v[k] & 0xffffu), b = (int)(v[k] >> 16);
        s_ab += v[k];
        s_aa += a * a;
        s_bb += b * b;
        s_xy += a * b;
        if (k >= kSsimWin - 1) {
          const int o = k - (kSsimWin - 1);
          h_ab[r][q0 + o] = s_ab;
          h_aa[r][q0 + o] = s_aa;
          h_bb[r][q0 + o] = s_bb;
          h_xy[r][q0 + o] = s_xy;
          const int a0 = (int)(v[o] & 0xffffu), b0 = (int)(v[o] >> 16);
          s_ab -= v[o];
          s_aa -= a0 * a0;
          s_bb -= b0 * b0;
          s_xy -= a0 * b0;
        }
      }
    }
    __syncthreads();
    // ---- vertical sliding sums, S and the masked sums: one column x 8 output rows per thread (the 8 rows of one channel
    // summed in fp32, then added to the float64 accumulators)
    {
      float cs[kSsimSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      uint32_t s_ab = 0;
      int s_aa = 0, s_bb = 0, s_xy = 0;
#pragma unroll
      for (int k = 0; k < kSsimVSeg + kSsimWin - 1; ++k) {
        const int r = vr0 + k;
        s_ab += h_ab[r][vj];
        s_aa += h_aa[r][vj];
        s_bb += h_bb[r][vj];
        s_xy += h_xy[r][vj];
        if (k >= kSsimWin - 1) {
          const int gy = y0 + r - (kSsimWin - 1);
          if (gx < W && gy < H) {
            const int sa = (int)(s_ab & 0xffffu), sb = (int)(s_ab >> 16);
            const int d_aa = 49 * s_aa - sa * sa, d_bb = 49 * s_bb - sb * sb, d_ab = 49 * s_xy - sa * sb;
            const float num = ((float)(2 * sa * sb) + c1) * ((float)(2 * d_ab) + c2);
            const float den = ((float)(sa * sa + sb * sb) + c1) * ((float)(d_aa + d_bb) + c2);
            const float S = num * __builtin_amdgcn_rcpf(den);  // (1 ulp; den >= c1 c2 > 0)
            if (smap) smap[(uint32_t)c * (uint32_t)P + (uint32_t)(gy * W + gx)] = S;
            const float m = mk[k - (kSsimWin - 1)];
            const float ms = 1.0f - m;  // (the static mask is formed in fp32 upstream, :243-246)
            cs[0] += S;
            cs[1] += S * m;
            cs[2] += S * ms;
            cs[3] += m;
            cs[4] += ms;
          }
          const int rr = r - (kSsimWin - 1);
          s_ab -= h_ab[rr][vj];
          s_aa -= h_aa[rr][vj];
          s_bb -= h_bb[rr][vj];
          s_xy -= h_xy[rr][vj];
        }
      }
#pragma unroll
      for (int j = 0; j < kSsimSums; ++j) acc[j] += (double)cs[j];
    }
    __syncthreads();  // (the next channel overwrites the tile)
  }
  block_partials<kSsimSums, kSsimThreads>(tid, acc, red, partials + (size_t)blockIdx.x * kSsimSums);
}

// fixed-order final sum (wave k reduces sum k with ordered_block_sum): the result does not depend on scheduling.  Layout of
// the PSNR row: sums[3] = 3HW, sums[6..7] = 0.
__global__ void __launch_bounds__(kSsimSums * kWave)
eval_ssim_final_kernel(const double *__restrict__ partials, int n_blocks, double count, double *__restrict__ sums) {
  const int k = threadIdx.x / kWave;
  const double v = ordered_block_sum(partials + k, 0, n_blocks, kSsimSums);
  if ((threadIdx.x & (kWave - 1)) == 0) sums[k < 3 ? k : k + 1] = v;
  if (threadIdx.x == 0) {
    sums[3] = count;
    sums[6] = 0.0;
    sums[7] = 0.0;
  }
}

static int64_t ssim_blocks(int H, int W) {
  return (int64_t)((W + kSsimTW - 1) / kSsimTW) * ((H + kSsimTH - 1) / kSsimTH);
}

}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_eval_ssim_workspace_bytes(int H, int W) {
  if (H < kSsimWin || W < kSsimWin || (int64_t)H * W >= (1ll << 30)) return PGDVS_ERR_INVALID;
  return ssim_blocks(H, W) * kSsimSums * 8;
}

PGDVS_API int pgdvs_eval_ssim_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hwc, int H, int W, float *ssim_map,
                                   double *sums, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_planar && gt_hwc && mask_hwc && sums && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30),
                "pgdvs_eval_ssim_sums: bad arguments");
  PGDVS_REQUIRE(H >= kSsimWin && W >= kSsimWin, "pgdvs_eval_ssim_sums: the image (%d x %d) is smaller than the 7 x 7 window", H, W);
  if (!workspace || workspace_bytes < pgdvs_eval_ssim_workspace_bytes(H, W)) {
    set_error("pgdvs_eval_ssim_sums: workspace too small");
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double *partials = reinterpret_cast<double *>(workspace);
  const int64_t nb = ssim_blocks(H, W);
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  PGDVS_LAUNCH("eval_ssim_partials", eval_ssim_partials_kernel, dim3((unsigned)nb), dim3(kSsimThreads), 0, st, pred_planar, gt_hwc,
               mask_hwc, H, W, tiles_x, ssim_map, partials);
  PGDVS_LAUNCH("eval_ssim_final", eval_ssim_final_kernel, dim3(1), dim3(kSsimSums * kWave), 0, st, (const double *)partials, (int)nb,
               3.0 * (double)H * (double)W, sums);
  return check_launch("eval_ssim_sums");
}
