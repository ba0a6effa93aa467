// The resident loaders' item builder (pgdvs_amd/datasets/resident.py): a scene's source frames stay on the device as they
// are stored (colour bytes, mask bytes, float32 depth), and every item is gathered from them.  include/pgdvs_hip.h states
// what is computed; this is how.
//
// item_views  one launch per item, grid.y = the view, over all of the item's groups.  The frame ids and the groups' output
//             bases are kernel arguments: nothing is uploaded.  A lane takes four pixels: three dwords of colour (12
//             bytes), one of mask, 16 bytes of depth, and writes eleven 16-byte stores: 3 each of rgb, dyn_rgb and
//             static_rgb, one of dyn_mask, one of depth.  About 8 bytes read and 44 written per pixel and view, no LDS,
//             no atomics, no view waits for another: repeated ids in any order are independent work.
//             The frame slots are 16-byte aligned by the caller (checked); a view's OUTPUT bases are 16-byte aligned only
//             when the view's offset in its group is, which H W % 4 == 0 guarantees.  Otherwise (the odd sizes of the
//             tests) a view whose bases are not aligned takes the scalar statement for all of its pixels: the choice is
//             uniform over the launch's y.  The scalar statement also finishes the H W % 4 pixels behind the quads.
//             rgb = byte / 255 is a true division (__fdiv_rn): a multiply by 1 / 255 differs at 126 of the 256 values.
// item_target one launch per item of the DyCheck loader: the target's colour bytes and covisible bytes, uploaded as stored, to
//             the float32 image and mask.  The layout of item_views: a lane takes four pixels, three dwords of colour and
//             one of mask, and writes four 16-byte stores (three without a mask); 4 bytes read and 16 written per pixel.
//             The four bases decide on the host: all 16-byte aligned, or the scalar statement for the whole image.
// flow_occ    one pixel per lane: float32 |cd.x| + |cd.y|, then a strict compare; a NaN compares false, as numpy's >.
#include "common.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxViews = PGDVS_ITEM_MAX_VIEWS, kMaxGroups = PGDVS_ITEM_MAX_GROUPS;

struct ItemGroup {
  float *rgb, *dyn_mask, *dyn_rgb, *static_rgb, *depth;  // [n,H,W,3] / [n,H,W,1]; depth null: the group has none
  int first;                                             // the group's first view in ids
};

struct ItemParams {
  const uint8_t *rgb, *mask;  // the store: frame f at + f * slot
  const float *depth;
  int64_t rgb_slot, mask_slot, depth_slot;  // bytes, multiples of 16
  int64_t n;                                // H W
  int n_groups;
  ItemGroup groups[kMaxGroups];
  int ids[kMaxViews];
};

__device__ __forceinline__ float unit(uint32_t word, int byte) { return __fdiv_rn((float)((word >> (8 * byte)) & 0xffu), 255.0f); }

__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ void __launch_bounds__(kBlock) item_views_kernel(ItemParams p) {
  const int v = blockIdx.y;
  int g = 0;
#pragma unroll
  for (int k = 1; k < kMaxGroups; ++k)
    if (k < p.n_groups && v >= p.groups[k].first) g = k;
  const int64_t f = p.ids[v];
  const int64_t view_off = (int64_t)(v - p.groups[g].first) * p.n;  // pixels in front of this view in its group
  const uint8_t *__restrict__ src_c = p.rgb + f * p.rgb_slot;
  const uint8_t *__restrict__ src_m = p.mask + f * p.mask_slot;
  const float *__restrict__ src_d = reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.depth) + f * p.depth_slot);
  float *__restrict__ o_rgb = p.groups[g].rgb + view_off * 3;
  float *__restrict__ o_dyn = p.groups[g].dyn_rgb + view_off * 3;
  float *__restrict__ o_st = p.groups[g].static_rgb + view_off * 3;
  float *__restrict__ o_m = p.groups[g].dyn_mask + view_off;
  float *__restrict__ o_d = p.groups[g].depth ? p.groups[g].depth + view_off : nullptr;

  const bool vec = aligned16(o_rgb) && aligned16(o_dyn) && aligned16(o_st) && aligned16(o_m) && aligned16(o_d);
  const int64_t quads = vec ? p.n >> 2 : 0;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;

  for (int64_t q = t; q < quads; q += stride) {  // (the grid covers the quads: one trip)
    const uint32_t *cw = reinterpret_cast<const uint32_t *>(src_c) + q * 3;
    const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
    const uint32_t mw = reinterpret_cast<const uint32_t *>(src_m)[q];
    struct {
      float4 c[3], m;  // 4 pixels x rgb, interleaved as stored; their masks
    } x;
    x.c[0] = make_float4(unit(w0, 0), unit(w0, 1), unit(w0, 2), unit(w0, 3));  // r0 g0 b0 r1
    x.c[1] = make_float4(unit(w1, 0), unit(w1, 1), unit(w1, 2), unit(w1, 3));  // g1 b1 r2 g2
    x.c[2] = make_float4(unit(w2, 0), unit(w2, 1), unit(w2, 2), unit(w2, 3));  // b2 r3 g3 b3
    x.m = make_float4((float)(mw & 0xffu), (float)((mw >> 8) & 0xffu), (float)((mw >> 16) & 0xffu), (float)(mw >> 24));
    const float4 im = make_float4(1.0f - x.m.x, 1.0f - x.m.y, 1.0f - x.m.z, 1.0f - x.m.w);
    // each pixel's mask over its three channels, in the interleaved order of c
    const float4 m0 = make_float4(x.m.x, x.m.x, x.m.x, x.m.y), m1 = make_float4(x.m.y, x.m.y, x.m.z, x.m.z),
                 m2 = make_float4(x.m.z, x.m.w, x.m.w, x.m.w);
    const float4 i0 = make_float4(im.x, im.x, im.x, im.y), i1 = make_float4(im.y, im.y, im.z, im.z),
                 i2 = make_float4(im.z, im.w, im.w, im.w);
    float4 *r4 = reinterpret_cast<float4 *>(o_rgb) + q * 3;
    float4 *d4 = reinterpret_cast<float4 *>(o_dyn) + q * 3;
    float4 *s4 = reinterpret_cast<float4 *>(o_st) + q * 3;
    r4[0] = x.c[0];
    r4[1] = x.c[1];
    r4[2] = x.c[2];
    d4[0] = mul4(x.c[0], m0);
    d4[1] = mul4(x.c[1], m1);
    d4[2] = mul4(x.c[2], m2);
    s4[0] = mul4(x.c[0], i0);
    s4[1] = mul4(x.c[1], i1);
    s4[2] = mul4(x.c[2], i2);
    reinterpret_cast<float4 *>(o_m)[q] = x.m;
    if (o_d) reinterpret_cast<float4 *>(o_d)[q] = reinterpret_cast<const float4 *>(src_d)[q];
  }

  for (int64_t i = (quads << 2) + t; i < p.n; i += stride) {  // the scalar statement: the tail, or a whole unaligned view
    const float m = (float)src_m[i];
    const float im = 1.0f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = __fdiv_rn((float)src_c[i * 3 + c], 255.0f);
      o_rgb[i * 3 + c] = x;
      o_dyn[i * 3 + c] = x * m;
      o_st[i * 3 + c] = x * im;
    }
    o_m[i] = m;
    if (o_d) o_d[i] = src_d[i];
  }
}

__global__ void __launch_bounds__(kBlock) flow_occ_kernel(const float2 *__restrict__ cd, int64_t n, float thres, float *__restrict__ occ) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float2 d = cd[i];
  occ[i] = (fabsf(d.x) + fabsf(d.y)) > thres ? 1.0f : 0.0f;
}

// One image, both outputs: rgb_out = byte / 255 (the division of unit()), mask_out = covisible > 0.  `quads`: the pixels
// taken four per lane (0 when a base is not 16-byte aligned: the host decides, the choice is uniform over the launch).
__global__ void __launch_bounds__(kBlock) item_target_kernel(const uint8_t *__restrict__ rgb, const uint8_t *__restrict__ cov, int64_t n,
                                                             int64_t quads, float *__restrict__ rgb_out, float *__restrict__ mask_out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t q = t; q < quads; q += stride) {  // (the grid covers the quads: one trip)
    const uint32_t *cw = reinterpret_cast<const uint32_t *>(rgb) + q * 3;
    const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
    float4 *r4 = reinterpret_cast<float4 *>(rgb_out) + q * 3;
    r4[0] = make_float4(unit(w0, 0), unit(w0, 1), unit(w0, 2), unit(w0, 3));
    r4[1] = make_float4(unit(w1, 0), unit(w1, 1), unit(w1, 2), unit(w1, 3));
    r4[2] = make_float4(unit(w2, 0), unit(w2, 1), unit(w2, 2), unit(w2, 3));
    if (cov) {
      const uint32_t mw = reinterpret_cast<const uint32_t *>(cov)[q];
      reinterpret_cast<float4 *>(mask_out)[q] = make_float4((mw & 0xffu) ? 1.0f : 0.0f, (mw & 0xff00u) ? 1.0f : 0.0f,
                                                            (mw & 0xff0000u) ? 1.0f : 0.0f, (mw & 0xff000000u) ? 1.0f : 0.0f);
    }
  }
  for (int64_t i = (quads << 2) + t; i < n; i += stride) {  // the scalar statement: the tail, or a whole unaligned image
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb_out[i * 3 + c] = __fdiv_rn((float)rgb[i * 3 + c], 255.0f);
    if (cov) mask_out[i] = cov[i] > 0 ? 1.0f : 0.0f;
  }
}

bool shape_ok(int H, int W) { return H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20) && (int64_t)H * W < (1ll << 31); }

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_item_views(const uint8_t *rgb, const uint8_t *dyn_mask, const float *depth, int F, int H, int W, int64_t rgb_slot,
                               int64_t mask_slot, int64_t depth_slot, const int32_t *ids, int n_views, const int32_t *group_sizes,
                               int n_groups, float *const *out, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(H, W) && F >= 1, "pgdvs_item_views: bad shape F=%d H=%d W=%d (F, H, W >= 1, H, W < 2^20, H W < 2^31)", F, H, W);
  PGDVS_REQUIRE(rgb && dyn_mask && ids && group_sizes && out, "pgdvs_item_views: null pointer");
  PGDVS_REQUIRE(n_views >= 1 && n_views <= kMaxViews && n_groups >= 1 && n_groups <= kMaxGroups,
                "pgdvs_item_views: %d views in %d groups (1 <= views <= %d, 1 <= groups <= %d)", n_views, n_groups, kMaxViews, kMaxGroups);
  const int64_t n = (int64_t)H * W;
  PGDVS_REQUIRE(aligned16(rgb) && aligned16(dyn_mask) && aligned16(depth), "pgdvs_item_views: the store's tables must be 16-byte aligned");
  PGDVS_REQUIRE(rgb_slot % 16 == 0 && mask_slot % 16 == 0 && depth_slot % 16 == 0 && rgb_slot >= n * 3 && mask_slot >= n &&
                    depth_slot >= n * 4,
                "pgdvs_item_views: slots of %lld, %lld, %lld bytes (multiples of 16, at least one frame of %lld pixels each)",
                (long long)rgb_slot, (long long)mask_slot, (long long)depth_slot, (long long)n);
  ItemParams p;
  p.rgb = rgb;
  p.mask = dyn_mask;
  p.depth = depth;
  p.rgb_slot = rgb_slot;
  p.mask_slot = mask_slot;
  p.depth_slot = depth_slot;
  p.n = n;
  p.n_groups = n_groups;
  int first = 0;
  for (int g = 0; g < kMaxGroups; ++g) {
    ItemGroup &G = p.groups[g];
    if (g >= n_groups) {
      G = ItemGroup{nullptr, nullptr, nullptr, nullptr, nullptr, n_views};
      continue;
    }
    PGDVS_REQUIRE(group_sizes[g] >= 1, "pgdvs_item_views: group %d has %d views", g, group_sizes[g]);
    float *const *o = out + g * 5;
    PGDVS_REQUIRE(o[0] && o[1] && o[2] && o[3], "pgdvs_item_views: group %d lacks an output (only depth may be NULL)", g);
    PGDVS_REQUIRE(!o[4] || depth, "pgdvs_item_views: group %d asks for depth and the store has none", g);
    for (int k = 0; k < 5; ++k)
      PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(o[k]) & 3) == 0, "pgdvs_item_views: group %d, output %d is not 4-byte aligned", g, k);
    G = ItemGroup{o[0], o[1], o[2], o[3], o[4], first};
    first += group_sizes[g];
  }
  PGDVS_REQUIRE(first == n_views, "pgdvs_item_views: the groups hold %d views, ids %d", first, n_views);
  for (int v = 0; v < kMaxViews; ++v) {
    PGDVS_REQUIRE(v >= n_views || (ids[v] >= 0 && ids[v] < F), "pgdvs_item_views: ids[%d] = %d, the store has %d frames", v,
                  v < n_views ? ids[v] : 0, F);
    p.ids[v] = v < n_views ? ids[v] : 0;
  }
  const int64_t work = n >= 4 ? n >> 2 : n;  // quads; a view that takes the scalar statement strides over them
  const dim3 grid((unsigned)cdiv(work, kBlock), (unsigned)n_views);
  PGDVS_LAUNCH("item_views", item_views_kernel, grid, dim3(kBlock), 0, as_stream(stream), p);
  return check_launch("pgdvs_item_views");
}

PGDVS_API int pgdvs_item_target(const uint8_t *rgb, const uint8_t *covisible, int H, int W, float *rgb_out, float *mask_out,
                                 pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(H, W), "pgdvs_item_target: bad shape H=%d W=%d (H, W >= 1, each < 2^20, H W < 2^31)", H, W);
  PGDVS_REQUIRE(rgb && rgb_out, "pgdvs_item_target: null pointer");
  PGDVS_REQUIRE((covisible != nullptr) == (mask_out != nullptr), "pgdvs_item_target: covisible and mask_out go together (%s is NULL)",
                covisible ? "mask_out" : "covisible");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(rgb_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(mask_out) & 3) == 0,
                "pgdvs_item_target: the outputs must be 4-byte aligned");
  const int64_t n = (int64_t)H * W;
  const bool vec = aligned16(rgb) && aligned16(covisible) && aligned16(rgb_out) && aligned16(mask_out);  // (NULL counts as aligned)
  const int64_t quads = vec ? n >> 2 : 0;
  const int64_t work = quads > n - (quads << 2) ? quads : n - (quads << 2);  // the longer of the two loops (the tail is under 4)
  PGDVS_LAUNCH("item_target", item_target_kernel, dim3((unsigned)cdiv(work, kBlock)), dim3(kBlock), 0, as_stream(stream), rgb, covisible,
               n, quads, rgb_out, mask_out);
  return check_launch("pgdvs_item_target");
}

PGDVS_API int pgdvs_flow_occ(const float *coord_diff, int H, int W, float thres, float *occ, pgdvs_stream_t stream) {
  PGDVS_REQUIRE(shape_ok(H, W), "pgdvs_flow_occ: bad shape H=%d W=%d (H, W >= 1, each < 2^20, H W < 2^31)", H, W);
  PGDVS_REQUIRE(coord_diff && occ, "pgdvs_flow_occ: null pointer");
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(coord_diff) & 7) == 0 && (reinterpret_cast<uintptr_t>(occ) & 3) == 0,
                "pgdvs_flow_occ: coord_diff must be 8-byte aligned, occ 4-byte");
  const int64_t n = (int64_t)H * W;
  PGDVS_LAUNCH("flow_occ", flow_occ_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, as_stream(stream),
               reinterpret_cast<const float2 *>(coord_diff), n, thres, occ);
  return check_launch("pgdvs_flow_occ");
}
