// SURVEY 8f-1, the evaluator's masked LPIPS (pgdvs/engines/evaluator_pgdvs.py:94-110,190-283 through
// pgdvs/utils/nsff_lpips: PerceptualLoss(model="net-lin", net="alex", version=0.1), trainer_pgdvs.py:132-137) for one view:
//   prep   the PSNR pass's 8-bit quantisation (eval_common.h), then 2 q - 1 (modify_rgb_range "0_1" -> "-1_1"), into ONE
//          [2,3,H,W] batch, ground truth first: every backbone layer runs once for both images (upstream runs the backbone
//          on both images for each of the three masks).  No ScalingLayer: PNetLin.forward tests `version == "0.1"` against a
//          string while the evaluator passes the float 0.1 (networks_basic.py:94-99), so the shift / scale never applies.
//   conv   AlexNet features[0:12] (pretrained_networks.py:63-105): an implicit-GEMM convolution with fused bias + ReLU on
//          the 16x16x4 fp32 matrix instruction (fp32 products and accumulation, no reduced-precision split: run.py:21-24
//          turns TF32 off), templated on kernel size / stride / padding; a standalone 3/2 max-pool between layers.
//   head   one launch over the five relu maps: per pixel normalize_tensor (f / (sqrt(sum_c f^2) + 1e-10)) of both images,
//          the squared difference, the 1x1 lin_k weights (no bias; dropout is inactive in eval mode), and the masked sums
//          of spatial_average (networks_basic.py:15-25) with the mask's channel 0 resampled to the layer's size by torch's
//          "nearest" rule, evaluated in-kernel; fixed-order float64 block partials.
//   final  per layer sum(x m) / (sum(m) + 1e-8) for the masks ones / eval_mask / 1 - eval_mask, summed over the layers.
#include "common.h"
#include "eval_common.h"
#include "gnt_mfma.h"
#include "lpips_net.h"

namespace pgdvs {

// ---- the network (torchvision alexnet().features[0:12] and the LPIPS v0.1 lin layers): shapes in lpips_net.h

// ---- the convolution: block tile 64 output channels x 128 output pixels, K in steps of 16; four waves in 2 x 2, a wave's
// 32 x 64 is 2 x 4 tiles of the 16x16x4 instruction.  Every Cout is a multiple of 64.
constexpr int kCvBM = 64, kCvBN = 128, kCvBK = 16, kCvThreads = 256;
constexpr int kCvPitchA = kCvBM + 16, kCvPitchB = kCvBN + 16;  // rows 4 apart land 16 banks apart: the operand reads are free of conflicts
constexpr int kCvLoadsA = kCvBM * kCvBK / kCvThreads;          // 4
constexpr int kCvLoadsB = kCvBN * kCvBK / kCvThreads;          // 8

// out[n][co][oy][ox] = relu(bias[co] + sum_{ci,kh,kw} w[co][ci][kh][kw] in[n][ci][oy*ST-PD+kh][ox*ST-PD+kw]) with zero padding;
// GEMM rows = co, columns = the n*Hout*Wout output pixels, K = ci*KS*KS + kh*KS + kw ascending (torch's weight layout).
template <int KS, int ST, int PD>
__global__ void __launch_bounds__(kCvThreads)
lpips_conv_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ out,
                  int Cin, int Hin, int Win, int Cout, int Hout, int Wout, int P) {
  __shared__ float As[kCvBK][kCvPitchA];
  __shared__ float Bs[kCvBK][kCvPitchB];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int bn = blockIdx.x * kCvBN, bm = blockIdx.y * kCvBM;
  const int K = Cin * KS * KS, HWo = Hout * Wout, HWi = Hin * Win;

  // this thread's im2col column: one output pixel, fixed for the whole K loop
  const int bcol = tid % kCvBN, brow0 = tid / kCvBN;
  const int p = bn + bcol;
  const bool p_ok = p < P;
  int iy0 = 0, ix0 = 0;
  const float *ibase = in;
  if (p_ok) {
    const int img = p / HWo, r = p - img * HWo;
    const int oy = r / Wout, ox = r - oy * Wout;
    iy0 = oy * ST - PD;
    ix0 = ox * ST - PD;
    ibase = in + (size_t)img * Cin * HWi;
  }
  // this thread's weight elements: K index acol, rows arow0 + 16 j
  const int acol = tid % kCvBK, arow0 = tid / kCvBK;
  const float *wbase = w + (size_t)(bm + arow0) * K;

  float ra[kCvLoadsA], rb[kCvLoadsB];
  auto load = [&](int k0) {
    const int ka = k0 + acol;
#pragma unroll
    for (int j = 0; j < kCvLoadsA; ++j) ra[j] = ka < K ? wbase[(size_t)(16 * j) * K + ka] : 0.0f;
#pragma unroll
    for (int j = 0; j < kCvLoadsB; ++j) {
      const int k = k0 + brow0 + 2 * j;
      const int ci = k / (KS * KS), rr = k - ci * (KS * KS);
      const int kh = rr / KS, kw = rr - kh * KS;
      const int iy = iy0 + kh, ix = ix0 + kw;
      const bool ok = p_ok && k < K && iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
      rb[j] = ok ? ibase[(size_t)ci * HWi + iy * Win + ix] : 0.0f;
    }
  };

  const int wm = wave & 1, wn = wave >> 1;
  const int li = lane & 15, lk = lane >> 4;
  floatx4 acc[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
  for (int k0 = 0; k0 < K; k0 += kCvBK) {
#pragma unroll
    for (int j = 0; j < kCvLoadsA; ++j) As[acol][arow0 + 16 * j] = ra[j];
#pragma unroll
    for (int j = 0; j < kCvLoadsB; ++j) Bs[brow0 + 2 * j][bcol] = rb[j];
    __syncthreads();
    if (k0 + kCvBK < K) load(k0 + kCvBK);  // (in flight while this tile is multiplied)
#pragma unroll
    for (int ks = 0; ks < kCvBK / 4; ++ks) {
      const int kr = 4 * ks + lk;  // A[i][k] from lane i + 16 k, B[k][j] from lane j + 16 k
      float a[2], b[4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = As[kr][32 * wm + 16 * mt + li];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) b[nt] = Bs[kr][64 * wn + 16 * nt + li];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16(a[mt], b[nt], acc[mt][nt]);
    }
    __syncthreads();
  }
  // D[4 lk + r][li] of each tile: output channel bm + 32 wm + 16 mt + 4 lk + r, pixel bn + 64 wn + 16 nt + li
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int q = bn + 64 * wn + 16 * nt + li;
    if (q >= P) continue;
    const int img = q / HWo, r = q - img * HWo;
    float *ob = out + (size_t)img * Cout * HWo + r;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = bm + 32 * wm + 16 * mt + 4 * lk + e;
        const float v = acc[mt][nt][e] + bias[co];
        ob[(size_t)co * HWo] = v > 0.0f ? v : 0.0f;
      }
  }
}

// nn.MaxPool2d(kernel_size=3, stride=2) (no padding, floor mode) over planes [n_planes, Hin, Win]
__global__ void __launch_bounds__(256)
lpips_maxpool_kernel(const float *__restrict__ in, float *__restrict__ out, int n_planes, int Hin, int Win, int Hout, int Wout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)n_planes * Hout * Wout;
  if (i >= n) return;
  const int ox = (int)(i % Wout), oy = (int)((i / Wout) % Hout);
  const int64_t pl = i / ((int64_t)Hout * Wout);
  const float *b = in + pl * Hin * Win + (size_t)(2 * oy) * Win + 2 * ox;
  float m = b[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, b[dy * Win + dx]);
  out[i] = m;
}

// quantised prediction / ground truth -> x[2][3][H][W] in [-1, 1]: x[0] = ground truth, x[1] = prediction
__global__ void __launch_bounds__(256)
lpips_prep_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int P, float *__restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x[(size_t)c * P + i] = 2.0f * quantise_u8(gt[(size_t)i * 3 + c]) - 1.0f;
    x[(size_t)(3 + c) * P + i] = 2.0f * quantise_u8(pred[(size_t)c * P + i]) - 1.0f;
  }
}

// ---- the head
constexpr int kHdThreads = 256;
constexpr int kHdSums = 5;  // per block: sum x, sum x m, sum x (1 - m), sum m, sum (1 - m)
struct LpipsHeadLayer {
  const float *feat;  // [2][C][h][w], image 0 = ground truth
  const float *lin;   // [C]
  int C, h, w, block0;
};
struct LpipsHeadArgs {
  LpipsHeadLayer l[kLpLayers];
  const float *mask;  // [H][W][3]; channel 0 is used
  int H, W;
};

// torch's "nearest" (UpSample.h nearest_idx): src = min(floor(dst * (float)in / out), in - 1), the product in fp32 (the
// in == out and out == 2 in special cases give the same index)
__device__ __forceinline__ int lpips_nearest(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

__global__ void __launch_bounds__(kHdThreads) lpips_head_kernel(LpipsHeadArgs a, double *__restrict__ partials) {
  __shared__ double red[kHdThreads / kWave][kHdSums];
  int L = 0;
#pragma unroll
  for (int k = 1; k < kLpLayers; ++k)
    if ((int)blockIdx.x >= a.l[k].block0) L = k;
  const LpipsHeadLayer ly = a.l[L];
  const int hw = ly.h * ly.w;
  const int i = ((int)blockIdx.x - ly.block0) * kHdThreads + (int)threadIdx.x;
  double v[kHdSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < hw) {
    const float *f0 = ly.feat + i, *f1 = ly.feat + (size_t)ly.C * hw + i;
    float n0 = 0.0f, n1 = 0.0f;
    for (int c = 0; c < ly.C; ++c) {
      const float a0 = f0[(size_t)c * hw], a1 = f1[(size_t)c * hw];
      n0 += a0 * a0;
      n1 += a1 * a1;
    }
    const float d0 = sqrtf(n0) + 1e-10f, d1 = sqrtf(n1) + 1e-10f;
    float d = 0.0f;
    for (int c = 0; c < ly.C; ++c) {
      const float e = f0[(size_t)c * hw] / d0 - f1[(size_t)c * hw] / d1;  // normalise, subtract, square, weight
      d += ly.lin[c] * (e * e);
    }
    const int y = i / ly.w, x = i - y * ly.w;
    const int sy = lpips_nearest(y, a.H, ly.h), sx = lpips_nearest(x, a.W, ly.w);
    const float m = a.mask[((size_t)sy * a.W + sx) * 3];
    const float ms = 1.0f - m;
    v[0] = (double)d;
    v[1] = (double)(d * m);
    v[2] = (double)(d * ms);
    v[3] = (double)m;
    v[4] = (double)ms;
  }
  block_partials<kHdSums, kHdThreads>(threadIdx.x, v, red, partials + (size_t)blockIdx.x * kHdSums);
}

struct LpipsFinalArgs {
  int block0[kLpLayers + 1];
  double pixels[kLpLayers];  // h w of each relu map: the sum of the all-ones mask
};

// wave k reduces sum k of every layer's blocks (ordered_block_sum); thread 0 forms the ratios in the reference's order (per
// layer, then the sum over the layers 0..4).  Deterministic.
__global__ void __launch_bounds__(kHdSums * kWave)
lpips_final_kernel(const double *__restrict__ partials, LpipsFinalArgs a, double *__restrict__ sums) {
  __shared__ double tot[kLpLayers][kHdSums];
  const int k = threadIdx.x / kWave;
  for (int L = 0; L < kLpLayers; ++L) {
    const double v = ordered_block_sum(partials + k, a.block0[L], a.block0[L + 1], kHdSums);
    if ((threadIdx.x & (kWave - 1)) == 0) tot[L][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r[3] = {0.0, 0.0, 0.0};
    for (int l = 0; l < kLpLayers; ++l) {
      r[0] += tot[l][0] / (a.pixels[l] + 1e-8);
      r[1] += tot[l][1] / (tot[l][3] + 1e-8);
      r[2] += tot[l][2] / (tot[l][4] + 1e-8);
    }
    sums[0] = r[0];
    sums[1] = r[1];
    sums[2] = r[2];
    sums[3] = a.pixels[0];
    sums[4] = tot[0][3];
    sums[5] = tot[0][4];
    sums[6] = 0.0;
    sums[7] = 0.0;
  }
}

// ---- shapes and the workspace
struct LpipsPlan {
  LpipsNetPlan net;  // x[2,3,H,W] and the backbone's maps
  int64_t off_part, total;
  int head_block0[kLpLayers + 1];
};

static int conv_out(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }
static int pool_out(int n) { return (n - 3) / 2 + 1; }

bool lpips_net_plan(int H, int W, int n_img, LpipsNetPlan &pl) {
  if (H < 31 || W < 31 || (int64_t)H * W >= (1ll << 26)) return false;
  pl.h[0] = conv_out(H, 11, 4, 2);
  pl.w[0] = conv_out(W, 11, 4, 2);
  pl.ph[0] = pool_out(pl.h[0]);
  pl.pw[0] = pool_out(pl.w[0]);
  pl.h[1] = pl.ph[0];
  pl.w[1] = pl.pw[0];
  pl.ph[1] = pool_out(pl.h[1]);
  pl.pw[1] = pool_out(pl.w[1]);
  for (int k = 2; k < kLpLayers; ++k) {
    pl.h[k] = pl.ph[1];
    pl.w[k] = pl.pw[1];
  }
  if (pl.h[4] < 1 || pl.w[4] < 1) return false;
  int64_t o = 0;
  pl.off_x = o;
  o += align_up((int64_t)n_img * 3 * H * W * 4, 256);
  for (int k = 0; k < kLpLayers; ++k) {
    pl.off_relu[k] = o;
    o += align_up((int64_t)n_img * kLpCout[k] * pl.h[k] * pl.w[k] * 4, 256);
    if (k < 2) {
      pl.off_pool[k] = o;
      o += align_up((int64_t)n_img * kLpCout[k] * pl.ph[k] * pl.pw[k] * 4, 256);
    }
  }
  pl.end = o;
  return true;
}

static bool lpips_plan(int H, int W, LpipsPlan &pl) {
  if (!lpips_net_plan(H, W, 2, pl.net)) return false;
  int64_t o = pl.net.end;
  pl.off_part = o;
  int nb = 0;
  for (int k = 0; k < kLpLayers; ++k) {
    pl.head_block0[k] = nb;
    nb += (pl.net.h[k] * pl.net.w[k] + kHdThreads - 1) / kHdThreads;
  }
  pl.head_block0[kLpLayers] = nb;
  o += align_up((int64_t)nb * kHdSums * 8, 256);
  pl.total = o;
  return true;
}

// the convolution over n_img images: one GEMM column per output pixel of every image
template <int KS, int ST, int PD>
static void launch_conv(const float *in, const float *w, const float *b, float *out, int n_img, int Cin, int Hin, int Win, int Cout,
                        int Hout, int Wout, hipStream_t st, const char *name) {
  const int P = n_img * Hout * Wout;
  PGDVS_LAUNCH(name, (lpips_conv_kernel<KS, ST, PD>), dim3((unsigned)((P + kCvBN - 1) / kCvBN), (unsigned)(Cout / kCvBM)), dim3(kCvThreads),
               0, st, in, w, b, out, Cin, Hin, Win, Cout, Hout, Wout, P);
}

static void launch_pool(const float *in, float *out, int n_planes, int Hin, int Win, int Hout, int Wout, hipStream_t st, const char *name) {
  const int64_t n = (int64_t)n_planes * Hout * Wout;
  PGDVS_LAUNCH(name, lpips_maxpool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n_planes, Hin, Win, Hout, Wout);
}

void lpips_net_weights(const float *conv_weights, const float *conv_biases, const float *lin_weights, const float *(&wk)[kLpLayers],
                       const float *(&bk)[kLpLayers], const float *(&lk)[kLpLayers]) {
  size_t ow = 0, ob = 0;
  for (int k = 0; k < kLpLayers; ++k) {
    wk[k] = conv_weights + ow;
    bk[k] = conv_biases + ob;
    lk[k] = lin_weights + ob;
    ow += (size_t)kLpCout[k] * kLpCin[k] * kLpKs[k] * kLpKs[k];
    ob += (size_t)kLpCout[k];
  }
}

void lpips_net_forward(char *ws, const LpipsNetPlan &pl, int n_img, int H, int W, const float *const (&wk)[kLpLayers],
                       const float *const (&bk)[kLpLayers], hipStream_t st) {
  const float *x = reinterpret_cast<const float *>(ws + pl.off_x);
  float *relu[kLpLayers], *pool[2];
  for (int k = 0; k < kLpLayers; ++k) relu[k] = reinterpret_cast<float *>(ws + pl.off_relu[k]);
  for (int k = 0; k < 2; ++k) pool[k] = reinterpret_cast<float *>(ws + pl.off_pool[k]);
  launch_conv<11, 4, 2>(x, wk[0], bk[0], relu[0], n_img, 3, H, W, 64, pl.h[0], pl.w[0], st, "lpips_conv1");
  launch_pool(relu[0], pool[0], n_img * 64, pl.h[0], pl.w[0], pl.ph[0], pl.pw[0], st, "lpips_pool1");
  launch_conv<5, 1, 2>(pool[0], wk[1], bk[1], relu[1], n_img, 64, pl.ph[0], pl.pw[0], 192, pl.h[1], pl.w[1], st, "lpips_conv2");
  launch_pool(relu[1], pool[1], n_img * 192, pl.h[1], pl.w[1], pl.ph[1], pl.pw[1], st, "lpips_pool2");
  launch_conv<3, 1, 1>(pool[1], wk[2], bk[2], relu[2], n_img, 192, pl.ph[1], pl.pw[1], 384, pl.h[2], pl.w[2], st, "lpips_conv3");
  launch_conv<3, 1, 1>(relu[2], wk[3], bk[3], relu[3], n_img, 384, pl.h[2], pl.w[2], 256, pl.h[3], pl.w[3], st, "lpips_conv4");
  launch_conv<3, 1, 1>(relu[3], wk[4], bk[4], relu[4], n_img, 256, pl.h[3], pl.w[3], 256, pl.h[4], pl.w[4], st, "lpips_conv5");
}

}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int64_t pgdvs_lpips_workspace_bytes(int H, int W) {
  LpipsPlan pl;
  if (!lpips_plan(H, W, pl)) {
    set_error("pgdvs_lpips_workspace_bytes: the image (%d x %d) is outside the backbone's range (H, W >= 31, H W < 2^26)", H, W);
    return PGDVS_ERR_INVALID;
  }
  return pl.total;
}

PGDVS_API int pgdvs_lpips_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hwc, int H, int W, const float *conv_weights,
                               const float *conv_biases, const float *lin_weights, double *sums, void *workspace, int64_t workspace_bytes,
                               pgdvs_stream_t stream) {
  PGDVS_REQUIRE(pred_planar && gt_hwc && mask_hwc && conv_weights && conv_biases && lin_weights && sums && H > 0 && W > 0,
                "pgdvs_lpips_sums: bad arguments");
  LpipsPlan pl;
  PGDVS_REQUIRE(lpips_plan(H, W, pl), "pgdvs_lpips_sums: the image (%d x %d) is outside the backbone's range (H, W >= 31, H W < 2^26)",
                H, W);
  if (!workspace || workspace_bytes < pl.total) {
    set_error("pgdvs_lpips_sums: workspace too small");
    return PGDVS_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  float *x = reinterpret_cast<float *>(ws + pl.net.off_x);
  float *relu[kLpLayers];
  for (int k = 0; k < kLpLayers; ++k) relu[k] = reinterpret_cast<float *>(ws + pl.net.off_relu[k]);
  const float *wk[kLpLayers], *bk[kLpLayers], *lk[kLpLayers];
  lpips_net_weights(conv_weights, conv_biases, lin_weights, wk, bk, lk);
  const int P = H * W;
  PGDVS_LAUNCH("lpips_prep", lpips_prep_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, pred_planar, gt_hwc, P, x);
  lpips_net_forward(ws, pl.net, 2, H, W, wk, bk, st);
  LpipsHeadArgs ha;
  for (int k = 0; k < kLpLayers; ++k) ha.l[k] = LpipsHeadLayer{relu[k], lk[k], kLpCout[k], pl.net.h[k], pl.net.w[k], pl.head_block0[k]};
  ha.mask = mask_hwc;
  ha.H = H;
  ha.W = W;
  double *partials = reinterpret_cast<double *>(ws + pl.off_part);
  PGDVS_LAUNCH("lpips_head", lpips_head_kernel, dim3((unsigned)pl.head_block0[kLpLayers]), dim3(kHdThreads), 0, st, ha, partials);
  LpipsFinalArgs fa;
  for (int k = 0; k <= kLpLayers; ++k) fa.block0[k] = pl.head_block0[k];
  for (int k = 0; k < kLpLayers; ++k) fa.pixels[k] = (double)pl.net.h[k] * (double)pl.net.w[k];
  PGDVS_LAUNCH("lpips_final", lpips_final_kernel, dim3(1), dim3(kHdSums * kWave), 0, st, (const double *)partials, fa, sums);
  return check_launch("lpips_sums");
}
