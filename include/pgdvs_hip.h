/*
 * pgdvs_hip.h -- C ABI of libpgdvs_hip.so: the MI355X (gfx950) implementation of
 * the PGDVS per-target-view rendering inner loop.
 *
 * The reference (apple/ml-pgdvs) has no C FFI: its hot path is Python/torch plus
 * three CUDA kernels embedded as strings (pgdvs/utils/softsplat.py) and the
 * un-vendored pytorch3d ops.  Each entry point below names the reference
 * function (file:line, relative to the upstream tree) it replaces; the Python
 * host layer (ml-pgdvs_amd/pgdvs_amd) binds them with ctypes and keeps the
 * reference's renderer plugin API on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is documented "host";
 *   - all buffers are caller-allocated, contiguous, fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t (NULL = default stream); every call only enqueues
 *     work on it and never synchronises or allocates (the diagnostics option knn_stats
 *     does synchronise);
 *   - return value: 0 on success, negative pgdvs_status on error, message via
 *     pgdvs_last_error() (thread-local);
 *   - re-entrant per stream.  Process-wide state is limited to (i) the options below, (ii) the
 *     opt-in profiling records of pgdvs_prof_*, (iii) per-device pools of fork / join events
 *     and the host-side statistics of pgdvs_view_geo_host_stats (mutex-protected).
 *
 * Options: a handful of process-wide switches, read from the ENVIRONMENT ONCE, when the
 * library is loaded, and changed afterwards only through pgdvs_option_set (never by a later
 * setenv: no entry point calls getenv).  An entry point reads the options it needs once, at
 * its start.  Results are identical for every setting (bit for bit for the index paths).
 *   name                  environment at load          meaning
 *   agg_ordered           PGDVS_AGG_ORDERED=1          A12 as the ordered chain of round 2: per frame an ordered
 *                                                      selection + a push that builds the rows (second implementation)
 *   agg_stage             PGDVS_AGG_STAGE=0 -> 0       0: A12's links leave no (depth, colour) rows, agg_rows gathers
 *                                                      them itself (the path of videos too long for the staging block)
 *   gnt_fp32              PGDVS_GNT_FP32=1             every GNT product on the fp32 matrix instruction (default:
 *                                                      exact bf16x3 products where they pay, see pgdvs_gnt_view_layer)
 *   raster_bound_density  PGDVS_RASTER_BOUND_DENSITY   rows per pixel from which the rasteriser computes its depth
 *                                                      bound and runs its long-list launch (default 2.2)
 *   knn_no_tpq            PGDVS_KNN_NO_TPQ=1           diagnostics: the wavefront-per-query search for every query
 *   knn_stats             PGDVS_KNN_STATS=1            diagnostics: ring histogram to stderr (synchronises)
 *   side_thread           PGDVS_SIDE_THREAD=0 -> 0     0: pgdvs_view_geo_forward enqueues the dynamic branch (side stream) from the
 *                                                      calling thread behind the static branch, as in rounds 4-5; default 1: a
 *                                                      worker thread of the library enqueues it while the caller enqueues the static
 *                                                      branch (the host's ~60 launches per view in two halves side by side)
 *
 * Camera block: 80 floats of derived per-camera constants produced by
 * pgdvs_cam_prep from the reference's flat_cam[34] = [h, w, K(4x4), c2w(4x4)]
 * (pgdvs/renderers/pgdvs_renderer.py:354-357).  Layout: see PGDVS_CAM_* below.
 */
#ifndef PGDVS_HIP_H_
#define PGDVS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *pgdvs_stream_t; /* hipStream_t */

enum pgdvs_status {
  PGDVS_OK = 0,
  PGDVS_ERR_INVALID = -1,   /* bad argument */
  PGDVS_ERR_LAUNCH = -2,    /* HIP launch / runtime error */
  PGDVS_ERR_WORKSPACE = -3, /* workspace too small */
  PGDVS_ERR_UNSUPPORTED = -4
};

#define PGDVS_CAM_KINV 0 /* [9]  inverse(K[:3,:3])                 */
#define PGDVS_CAM_M 9    /* [9]  c2w[:3,:3] @ Kinv                 */
#define PGDVS_CAM_O 18   /* [3]  c2w[:3,3]                         */
#define PGDVS_CAM_P 21   /* [16] K(4x4) @ inverse(c2w)             */
#define PGDVS_CAM_W2C 37 /* [16] inverse(c2w)                      */
#define PGDVS_CAM_R 53   /* [9]  c2w[:3,:3]                        */
#define PGDVS_CAM_HW 62  /* [2]  h, w                              */
#define PGDVS_CAM_K 64   /* [16] K as given                        */
#define PGDVS_CAM_BLOCK 80

const char *pgdvs_last_error(void);

/* Options (see the table at the top).  pgdvs_option_set: 0, or PGDVS_ERR_INVALID for an unknown name; flags take
 * value != 0.  pgdvs_option_get: the current value, NaN for an unknown name. */
int pgdvs_option_set(const char *name, double value);
double pgdvs_option_get(const char *name);
/* library/ABI version and the gfx target the device code was built for */
int pgdvs_abi_version(void);
const char *pgdvs_build_arch(void);

/* Optional per-kernel timing: when enabled every kernel launch is bracketed by HIP events
 * on its launch stream.  pgdvs_prof_report synchronises them, writes "name calls total_ms"
 * lines into buf and clears the records; returns the number of distinct names.  Process-
 * wide switch meant for bench.py; leave it off in production. */
void pgdvs_prof_enable(int on);
int pgdvs_prof_report(char *buf, int buf_len);
/* the fixed cost of one (event, launch, event) bracket that pgdvs_prof_report subtracts from
 * every record (measured once with an empty kernel) */
double pgdvs_prof_overhead_ms(void);

/* ---- cameras ------------------------------------------------------------- */
/* flat_cams[n,34] -> cam_blocks[n,80].  Replaces the torch.inverse / bmm chains of
 * pgdvs/renderers/pgdvs_renderer_base.py:40-45 and pgdvs/models/gnt/projector.py:49-60. */
int pgdvs_cam_prep(const float *flat_cams, int n, float *cam_blocks, pgdvs_stream_t stream);

/* A1: PGDVSBaseRenderer.get_batched_rays, batch_size=1
 * (pgdvs/renderers/pgdvs_renderer_base.py:17-57).  n = ceil(H/stride)*ceil(W/stride);
 * rays_o[n,3] rays_d[n,3] uvs[n,2]. */
int pgdvs_get_rays(const float *cam_block, int H, int W, int stride, float *rays_o,
                   float *rays_d, float *uvs, pgdvs_stream_t stream);

/* ---- dynamic branch -------------------------------------------------------- */
/* A2+A3: unproject frame 1, follow the flow into frame 2, unproject there, lerp in
 * time -- the dense part of PGDVSDynamicRenderer.compute_dyn_pcl
 * (pgdvs/renderers/pgdvs_renderer_dyn.py:299-388).
 *   dyn_mask1[H,W] occ[H,W] flow12[H,W,2] depth1[H,W] depth2[H,W] rgb1[H,W,3] rgb2[H,W,3]
 *   times[3] = (time_1, time_2, time_tgt) on the device
 *   mask_eff[H,W] u8 : dyn mask after the optional flow-consistency test (:304-308)
 *   valid[H,W]    u8 : mask_eff && flow target inside the image (:309-316)
 *   pcl[H,W,3], rgbf[H,W,3] : world point / attached colour, written where valid. */
int pgdvs_dyn_warp(int H, int W, const float *dyn_mask1, const float *occ,
                   int use_flow_consistency, const float *flow12, const float *depth1,
                   const float *depth2, const float *rgb1, const float *rgb2,
                   const float *cam1, const float *cam2, const float *times,
                   uint8_t *mask_eff, uint8_t *valid, float *pcl, float *rgbf,
                   pgdvs_stream_t stream);

/* Ordered stream compaction: idx_out[0..count) = ascending positions p with flags[p]!=0
 * (the boolean-mask indexing / torch.nonzero of pgdvs_renderer_dyn.py:309-320,477).
 * count_out: one int32 on the device.  workspace >= pgdvs_compact_workspace_bytes(n). */
int64_t pgdvs_compact_workspace_bytes(int64_t n);
int pgdvs_compact_u8(const uint8_t *flags, int64_t n, int32_t *idx_out, int32_t *count_out,
                     void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* gather rows: dst[i,:] = src[idx[i],:] for i < *count (row = `width` floats). */
int pgdvs_gather_rows(const float *src, const int32_t *idx, const int32_t *count,
                      int64_t capacity, int width, float *dst, pgdvs_stream_t stream);

/* A4: statistical outlier filter = pytorch3d.ops.knn_points(X, X, K+1) + mean of the K
 * non-self squared distances (pgdvs_renderer_dyn.py:405-419, st_geo_renderer.py:37-51).
 * pts[capacity,3], *count points used (count on device); avg_out[capacity].
 * algo: 0 = auto, 1 = brute force (O(N^2), what pytorch3d does), 2 = exact uniform-grid
 * search (needs K+1 <= 64; two grid levels, then an exhaustive scan for what is still open).
 * Both return identical values.  workspace >= pgdvs_knn_workspace_bytes(capacity). */
int64_t pgdvs_knn_workspace_bytes(int64_t capacity);
int pgdvs_knn_mean_dist(const float *pts, const int32_t *count, int64_t capacity, int K,
                        float *avg_out, int algo, void *workspace, int64_t workspace_bytes,
                        pgdvs_stream_t stream);

/* threshold = lower-median(avg) + unbiased-std(avg) * std_thres; flag = avg < threshold
 * (pgdvs_renderer_dyn.py:419-427).  thres_out: 1 float; flag_out[capacity] u8.
 * remove_outlier == 0 -> all flags 1 (:453-457), threshold still produced.  flag_out[i] = 0
 * for *count <= i < capacity. */
int64_t pgdvs_outlier_workspace_bytes(int64_t capacity);
int pgdvs_outlier_flags(const float *avg, const int32_t *count, int64_t capacity,
                        float std_thres, int remove_outlier, float *thres_out,
                        uint8_t *flag_out, void *workspace, int64_t workspace_bytes,
                        pgdvs_stream_t stream);

/* keep[P] u8 <- 0 everywhere, 1 at idx[i] where flag[i] (i < *count). */
int pgdvs_scatter_keep(const int32_t *idx, const uint8_t *flag, const int32_t *count,
                       int64_t capacity, uint8_t *keep, int64_t P, pgdvs_stream_t stream);

/* A5: project the surviving points into the target camera and scatter the dense
 * flow (pgdvs/models/gnt/projector.py:41-73 via pgdvs_renderer_dyn.py:470-503).
 * flow_1_to_tgt[2,H,W] (planar x then y), valid_dyn_mask_1[H,W] (0/1 floats). */
int pgdvs_project_flow_dense(int H, int W, const float *cam_tgt, const float *pcl,
                             const uint8_t *keep, float *flow_1_to_tgt,
                             float *valid_dyn_mask_1, pgdvs_stream_t stream);
/* sparse form: uv[n,2] = projection of pts[n,3] (Projector.compute_projections). */
int pgdvs_project_points(const float *cam_tgt, const float *pts, int64_t n, float *uv,
                         pgdvs_stream_t stream);

/* A6: softsplat importance metric, mean_c |rgb1 - backwarp(rgb2, flow)|
 * (pgdvs/renderers/pgdvs_renderer_base.py:68-78,91-138).  NCHW planar:
 * rgb1[B,3,H,W] rgb2[B,3,H,W] flow[B,2,H,W] -> l1[B,1,H,W]. */
int pgdvs_backwarp_l1(const float *rgb1, const float *rgb2, const float *flow, float *l1,
                      int B, int H, int W, pgdvs_stream_t stream);

/* A7: softsplat.softsplat / kernel softsplat_out (pgdvs/utils/softsplat.py:280-333,
 * 352-402).  in[B,C,H,W] flow[B,2,H,W] metric[B,1,H,W] (NULL for sum/avg) -> out[B,C,H,W].
 * mode: 0 sum, 1 avg, 2 linear, 3 soft; eps: 0 addeps (default), 1 zeroeps, 2 clipeps.
 * workspace >= pgdvs_softsplat_workspace_bytes(B,C,H,W,mode). */
int64_t pgdvs_softsplat_workspace_bytes(int B, int C, int H, int W, int mode);
int pgdvs_softsplat_fwd(const float *in, const float *flow, const float *metric, float *out,
                        int B, int C, int H, int W, int mode, int eps, void *workspace,
                        int64_t workspace_bytes, pgdvs_stream_t stream);

/* Backward of the raw splat (mode "sum"; softsplat.py:459-617, kernels softsplat_ingrad /
 * softsplat_flowgrad): ingrad[B,C,H,W] and flowgrad[B,2,H,W] (either nullable) from
 * outgrad[B,C,H,W].  The normalised modes differentiate through their torch pre/post-processing
 * exactly as upstream (softsplat.py:294-333). */
int pgdvs_softsplat_bwd(const float *in, const float *flow, const float *outgrad, float *ingrad,
                        float *flowgrad, int B, int C, int H, int W, pgdvs_stream_t stream);

/* A6+A7+A8+A11 fused for the renderer: noise-fill of static texels, metric, soft
 * splat of rgb and mask with the shared metric, threshold 1e-3, masking and the
 * final static/dynamic composite (pgdvs_renderer_dyn.py:157-202, pgdvs_renderer.py:169-178).
 *   rgb1[H,W,3] rgb2[H,W,3] (channels-last, as in the data dict), flow12[H,W,2],
 *   flow_1_to_tgt[2,H,W], valid_dyn_mask_1[H,W], noise[3,H,W] (un-clamped randn, may be NULL = 0),
 *   static_rgb[3,H,W] (may be NULL -> combined outputs skipped)
 *   outputs (planar): render_dyn_rgb[3,H,W] render_dyn_mask[H,W]
 *                     combined[3,H,W] combined_static[3,H,W] combined_dyn[3,H,W] (nullable)
 *   workspace >= pgdvs_dyn_splat_workspace_bytes(H,W). */
int64_t pgdvs_dyn_splat_workspace_bytes(int H, int W);
int pgdvs_dyn_splat_composite(int H, int W, const float *rgb1, const float *rgb2,
                              const float *flow12, const float *flow_1_to_tgt,
                              const float *valid_dyn_mask_1, const float *noise, float alpha,
                              const float *static_rgb, float *render_dyn_rgb,
                              float *render_dyn_mask, float *combined, float *combined_static,
                              float *combined_dyn, void *workspace, int64_t workspace_bytes,
                              pgdvs_stream_t stream);

/* The same with the noise drawn inside the scatter kernel where it is consumed (upstream: torch.randn_like per forward,
 * pgdvs_renderer_dyn.py:177-182): rng_state = DEVICE uint64[2] {seed, draw number}; the field is a pure function of
 * (seed, draw number, pixel) -- Philox4x32-10 + Box-Muller -- and the call increments the draw number, so a replayed
 * HIP graph draws a fresh field per replay.  pgdvs_splat_noise_field writes the field [3,H,W] the NEXT such call will
 * use (tests: the injected-noise entry point fed with it gives the same images). */
int pgdvs_dyn_splat_composite_rng(int H, int W, const float *rgb1, const float *rgb2, const float *flow12,
                                  const float *flow_1_to_tgt, const float *valid_dyn_mask_1, uint64_t *rng_state,
                                  float alpha, const float *static_rgb, float *render_dyn_rgb, float *render_dyn_mask,
                                  float *combined, float *combined_static, float *combined_dyn, void *workspace,
                                  int64_t workspace_bytes, pgdvs_stream_t stream);
int pgdvs_splat_noise_field(int H, int W, const uint64_t *rng_state, float *noise_out, pgdvs_stream_t stream);

/* ---- static branch --------------------------------------------------------- */
/* A9: pytorch3d PointsRasterizer(bin_size=0) + PointsRenderer + NormWeightedCompositor
 * as used by StaticGeoPointRenderer.forward (pgdvs/renderers/st_geo_renderer.py:77-120)
 * and render_dyn_pcl (pgdvs/renderers/pgdvs_renderer_dyn.py:671-724).
 *   points: xyz at pts[i*pts_stride..+3), features at feat[i*feat_stride..+3)
 *   n_points: host count; n_points_dev (nullable): device int64 count that overrides
 *   it (n_points is then the capacity: a larger or negative device count is clamped to [0, n_points]).
 *   Returns PGDVS_ERR_UNSUPPORTED (and the workspace query a negative size) when n_points times the
 *   tiles a disc of this radius can touch reaches 2^31 list entries.
 *   Workspace: 16 bytes per list entry the rows can produce (n_points x the tiles a disc can touch), 4 bytes per pixel, and --
 *   images of at least 16 tiles -- one segment per tile for the direct binning pass: twice the average list the rows allow,
 *   256 .. 4096 entries (0.53 GB at 1080p).  Sparse clouds (fewer rows than option raster_bound_density x pixels) are
 *   binned straight into the segments, without a counting pass; an entry that finds its segment full raises a device flag
 *   and the exact counting / scan / fill passes, enqueued behind the direct one either way, redo the binning.
 *   outputs (any may be NULL): idx[H,W,K] int64 (-1 pad), zbuf[H,W,K] (-1 pad),
 *   dist2[H,W,K] (-1 pad), rgb ([H,W,3] if rgb_planar == 0, [3,H,W] otherwise),
 *   mask[H,W] ((ones-render) > 0 as 0/1 floats).  K (points_per_pixel) in [1, 8]. */
int64_t pgdvs_points_raster_workspace_bytes(int64_t n_points, int H, int W, float radius);
int pgdvs_points_raster(const float *pts, int64_t pts_stride, const float *feat,
                        int64_t feat_stride, int64_t n_points, const int64_t *n_points_dev,
                        const float *cam_tgt, float radius, int K, int H, int W, int64_t *idx,
                        float *zbuf, float *dist2, float *rgb, int rgb_planar, float *mask,
                        void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* The same with a workspace sized for `row_bound` rows -- pgdvs_points_raster_workspace_bytes(row_bound, ...) -- instead
 * of the arrays' capacity n_points (callers keep capacity-sized cloud buffers with a device-side count; a hint such as
 * the previous view's count plus a margin saves gigabytes of tile lists per view in flight).  status_dev: DEVICE int32,
 * written by the call: 0 = all rows drawn, 1 = the device count exceeds row_bound (the rows beyond it are not drawn: the
 * images are not valid), 2 = the device count is negative (the producer's error status; nothing drawn). */
int pgdvs_points_raster_bounded(const float *pts, int64_t pts_stride, const float *feat, int64_t feat_stride,
                                int64_t n_points, const int64_t *n_points_dev, int64_t row_bound, int32_t *status_dev,
                                const float *cam_tgt, float radius, int K, int H, int W, int64_t *idx, float *zbuf,
                                float *dist2, float *rgb, int rgb_planar, float *mask, void *workspace,
                                int64_t workspace_bytes, pgdvs_stream_t stream);

/* A12: static point-cloud aggregation across the S frames of a video with the
 * projection-occupancy dedup (pgdvs/datasets/nvidia_eval_pure_geo.py:183-277,
 * pgdvs/datasets/nvidia_eval.py:840-847, pgdvs/datasets/base.py:507-546).
 *   rgbs[S,H,W,3] in [0,1]; depths[S,H,W]; dyn_masks[S,H,W] u8 (non-zero = dynamic)
 *   K3s: HOST double[S,9]; c2ws: HOST double[S,16]   (float64 numpy upstream)
 *   out[capacity,6] (xyz,rgb) in the reference's order; count_out: device int64 = the number
 *   of rows written, or -1 if the kernels' internal ordering protocol reported an error (the rows are
 *   then not valid; pgdvs_points_raster treats a negative device count as 0).  A count EQUAL to `capacity` means the
 *   cloud did not fit: rows were dropped (which ones is unspecified beyond frame 0's prefix) and the cloud must not be
 *   used -- size the buffer so that the count stays below it (S*H*W rows always suffice).
 *   The workspace holds one occupancy byte per (frame, pixel), the later frames' selection bits, 12 bytes per row of
 *   capacity and -- unless it would exceed 4 GB -- a staging block of 16 bytes per (frame, pixel) in which the chain's links
 *   leave (depth, colour) of the pixels they select (address space: a few per cent of it is ever touched, but all of it is
 *   part of the size this query returns: 0.85 GB at 1080p x 24 frames, 1.7 GB at x 48). */
int64_t pgdvs_static_aggregate_workspace_bytes(int S, int H, int W, int64_t capacity);
int pgdvs_static_aggregate(const float *rgbs, const float *depths, const uint8_t *dyn_masks,
                           const double *K3s_host, const double *c2ws_host, int S, int H, int W,
                           float *out, int64_t capacity, int64_t *count_out, void *workspace,
                           int64_t workspace_bytes, pgdvs_stream_t stream);
/* The same, and xyz_out[capacity,3] receives the coordinates alone (12 bytes per point): pass it as `pts` with
 * pts_stride 3 (and out + 3 with stride 6 as `feat`) to pgdvs_points_raster, whose binning passes then read half
 * the bytes.  Same workspace size. */
int pgdvs_static_aggregate_packed(const float *rgbs, const float *depths, const uint8_t *dyn_masks,
                                  const double *K3s_host, const double *c2ws_host, int S, int H, int W,
                                  float *out, float *xyz_out, int64_t capacity, int64_t *count_out,
                                  void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- GNT static renderer ---------------------------------------------------- */
/* A13: ray sampling + Projector.compute (pgdvs/models/gnt/ray_sampler.py:59-123,
 * pgdvs/models/gnt/projector.py:41-115,117-308) for R rays x S samples x V source views.
 *   ray_o/ray_d[R,3]; depth_range[1,2] or [R,2] (depth_range_per_ray); deterministic sampling,
 *   inverse-depth uniform when inv_uniform != 0; z_samples[R,S] (nullable) = explicit sample
 *   depths instead (the importance-resampled fine pass, ray_sampler.py:183-220)
 *   cam_tgt: camera block of the target; cams_src[V,80]; src_rgbs[V,H,W,3];
 *   featmaps_cl[V,hf,wf,C] (channels-last); inv_masks[V,H,W] (nullable: dynamic masks)
 *   outputs: pts[R,S,3] z_vals[R,S] (nullable), rgb_feat[R,S,V,3+C], ray_diff[R,S,V,4],
 *   mask_inbound / mask_invalid (nullable) / mask [R,S,V] as 0/1 floats. */
int pgdvs_gnt_gather(const float *ray_o, const float *ray_d, const float *depth_range,
                     int depth_range_per_ray, const float *z_samples, int R, int S, int inv_uniform,
                     const float *cam_tgt,
                     const float *cams_src, int V, const float *src_rgbs, int H, int W,
                     const float *featmaps_cl, int hf, int wf, int C, const float *inv_masks,
                     float *pts, float *z_vals, float *rgb_feat, float *ray_diff,
                     float *mask_inbound, float *mask_invalid, float *mask, pgdvs_stream_t stream);

/* A14 (entry of GNT.forward, pgdvs/models/gnt/models/transformer_network.py:455-474):
 * feat = rgbfeat_fc(rgb_feat) (Linear(3+C,64) -> ReLU -> Linear(64,64)) on the fp32 MFMA, fused
 * with the reductions over the source views that follow it upstream.
 *   weights: pgdvs_gnt_embed_weight_floats(Cin) floats = W1 input-major [4*ceil(Cin/4)][64]
 *            (rows >= Cin zero), b1[64], W2 input-major [64][64], b2[64]
 *            (pgdvs_amd.ops.pack_embed); Cin = 3 + C must be in (32, 36]
 *   rgb_feat[N,V,Cin] -> feat[N,V,64]; q0[N,64] = max over the V views (:458);
 *   stats[N,2] (nullable) = mean over features of the unbiased std over views and of
 *   std / (mean |feat| + 1e-6) (:464-472; all views, no mask). */
int64_t pgdvs_gnt_embed_weight_floats(int Cin);
int pgdvs_gnt_embed(const float *weights, const float *rgb_feat, int64_t N, int V, int Cin,
                    float *feat, float *q0, float *stats, pgdvs_stream_t stream);

/* A14, positional re-embedding of the even layers (transformer_network.py:482-486):
 * q <- q_fc(cat(q, posenc(pts), posenc(viewdir))) with q_fc = Linear(64+P+P',64) -> ReLU ->
 * Linear(64,64).  The caller forms the position part T[N,*] = posenc(pts) W1[:,64:64+P]^T and the
 * direction part tv[R,*] = posenc(viewdir) W1[:,64+P:]^T + b1 (row strides in floats, multiples
 * of 4, so that the slices of all even layers can share one GEMM); the kernel computes
 * q_out = W2 relu(W1[:, :64] q + T[g] + tv[g / S]) + b2.
 *   weights: W1[:, :64] input-major [64][64], W2 input-major [64][64], b2[64]. */
int pgdvs_gnt_posfc(const float *weights, const float *q_in, const float *T, int64_t t_stride,
                    const float *tv, int64_t tv_stride, int64_t N, int S, float *q_out,
                    pgdvs_stream_t stream);

/* A14, exit of GNT.forward (transformer_network.py:533-535):
 * rgb_out[R,3] = rgb_fc(mean over the S samples of LayerNorm(q[R,S,64])), eps 1e-5.
 *   weights: gamma[64], beta[64], rgb_fc weight [3][64], rgb_fc bias[3]. */
int pgdvs_gnt_head(const float *weights, const float *q, int R, int S, float *rgb_out,
                   pgdvs_stream_t stream);

/* A14 (view transformer): one fused fp32-MFMA kernel per GNT layer = Transformer2D +
 * Attention2D of pgdvs/models/gnt/models/transformer_network.py:59-169,197-223 (width 64).
 *   weights: pgdvs_gnt_view_weight_floats() floats, packed input-major as laid out in
 *            csrc/gnt_view.hip (VW_* offsets); built by pgdvs_amd.ops.pack_view_layer
 *   q_in[N,64]; feat[N,V,64] (rgbfeat_fc output); ray_diff[N,V,4]; valid[N,V] u8 (rows
 *   without any valid view must be passed as all-valid, :124-129); q_out[N,64]
 *   stats[N,3] (nullable): view entropy (:497-500, evaluated online as log l - sum e a / l, within
 *   2e-7 of the upstream expression), masked std of k, normalised std; means over features.
 *   Arithmetic: fp32 inputs, weights and results; the 64 x 64 products of the attention (k = Wk f and vv = Wv k per source view,
 *   q' and out_fc per tile) and the feed-forward block that closes the layer (also in pgdvs_gnt_ray_layer) run on the bf16
 *   matrix instructions with both operands split EXACTLY into three bf16 pieces (the six partial products above 2^-24 of the
 *   product, fp32 accumulation: the accuracy of an fp32 multiply-add chain, in about half its time); the weight blob carries
 *   the feed-forward weights a second time as pre-split images (pgdvs_amd.ops.ff_bf16x3_images).  The option gnt_fp32
 *   (PGDVS_GNT_FP32=1 at load time, pgdvs_option_set) keeps every product on the fp32 matrix instructions.
 *   Inputs below 2^-110 in magnitude or non-finite are outside the split path's contract: the truncation residues of a
 *   split underflow (the product loses its low pieces) and inf / NaN turn into NaN (inf - inf in the residue), where the
 *   fp32 instruction would carry them through; image features and LayerNorm outputs never get there. */
int64_t pgdvs_gnt_view_weight_floats(void);
int pgdvs_gnt_view_layer(const float *weights, const float *q_in, const float *feat,
                         const float *ray_diff, const uint8_t *valid, int64_t N, int V, float *q_out,
                         float *stats, pgdvs_stream_t stream);

/* A14 (ray transformer): Transformer + Attention(attn_mode="qk", 4 heads) of
 * pgdvs/models/gnt/models/transformer_network.py:231-338 for R rays x S samples (S <= 256),
 * width 64, fused with its feed-forward block.  weights: same packed layout as the view
 * layer (LN1 = attn_norm, WQ/WK/WV, WO = out_fc, LN2/F1/F2 = ff_norm/ff; the view-only
 * regions are unused).  q_out[R,S,64]; sample_weights[R,S] (nullable) = attention row of
 * query sample 0 averaged over heads (:336). */
int pgdvs_gnt_ray_layer(const float *weights, const float *q_in, int R, int S, float *q_out,
                        float *sample_weights, pgdvs_stream_t stream);

/* A10, dyn_render_type = "mesh" (pgdvs_renderer_dyn.py:542-669): triangulates the kept source
 * pixels (two triangles per pixel quad whose corners are all kept; faces touching the first
 * kept pixel are dropped, as upstream :597 does) and renders them into the target camera
 * with pytorch3d MeshRasterizer semantics (blur_radius 0, 1 face per pixel, perspective-
 * correct barycentrics) + vertex colours + hard blend on black.
 *   keep[H*W] u8 (valid_dyn_mask_1), pcl[H*W,3], rgb[H*W,3]: dense over the source frame
 *   img_planar[3,H,W], mask[H,W] (1 where a face covers the pixel centre),
 *   face_out[H*W] int32 (nullable): kind*H*W + source pixel of the winning face, -1 = none. */
int64_t pgdvs_mesh_render_workspace_bytes(int H, int W);
int pgdvs_mesh_render(const float *cam_tgt, int H, int W, const uint8_t *keep, const float *pcl,
                      const float *rgb, float *img_planar, float *mask, int32_t *face_out,
                      void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* A17: tracker-window point aggregation (pgdvs_renderer_dyn_track.py:98-396); tracks and
 * visibilities are inputs.  Frames are ordered as prepare_data orders them (:599-716):
 * [fwd2tgt tracks..., temporally-closest..., bwd2tgt tracks...].
 *   tracks[P,N,2] (col,row), visibles[P,N] u8, frame_kind_host[N] (HOST array; 1 = temporally
 *   closest frame, 2 = real track frame), times[N] / time_tgt[1] raw time stamps (device;
 *   shifted to start at 0 internally as :718-721), rgbs[N,H,W,3], depths[N,H,W],
 *   cams[N,PGDVS_CAM_BLOCK].
 *   valid[P] u8 : invisible in every closest frame and visible in >= 2 track frames (:115-127)
 *   pcl[P,3]    : the two visible frames nearest in time (:146-166) unprojected with the
 *                 nearest-sampled depth (:220-253) and inter/extrapolated to time_tgt (:278-284)
 *   rgb[P,3]    : mean of the two bilinear (align_corners=True) colour samples (:197-218,:271-276)
 * Rows of invalid tracks are zero.  N <= 64. */
int pgdvs_track_points(const float *tracks, const uint8_t *visibles, int64_t P, int N,
                       const uint8_t *frame_kind_host, const float *times, const float *time_tgt,
                       const float *rgbs, const float *depths, int H, int W, const float *cams,
                       uint8_t *valid, float *pcl, float *rgb, pgdvs_stream_t stream);

/* pytorch3d.ops.knn_points(queries, pts, K=KK) + mean over ALL KK squared distances (the
 * track-to-base filter, :299-312; no self column).  Exact uniform-grid search over `pts`;
 * counts on the device; KK <= 64; missing columns (fewer than KK points) count as 0.
 * avg_out[query_capacity].  workspace >= pgdvs_knn_cross_workspace_bytes(capacity, query_capacity). */
int64_t pgdvs_knn_cross_workspace_bytes(int64_t capacity, int64_t query_capacity);
int pgdvs_knn_cross_mean_dist(const float *queries, const int32_t *query_count, int64_t query_capacity,
                              const float *pts, const int32_t *count, int64_t capacity, int KK,
                              float *avg_out, void *workspace, int64_t workspace_bytes,
                              pgdvs_stream_t stream);

/* flag[i] = avg[i] < (*thres * mult) for i < *count (:314-318, :363-371).  gate_count
 * (nullable, device): when *gate_count == 0 ("no base cloud", :296-298) the test becomes
 * avg[i] < *alt_thres, or passes everything if alt_thres is null.  flag_out[i] = 0 for
 * *count <= i < capacity. */
int pgdvs_threshold_flags(const float *avg, const int32_t *count, int64_t capacity, const float *thres,
                          float mult, const float *alt_thres, const int32_t *gate_count,
                          uint8_t *flag_out, pgdvs_stream_t stream);

/* out = concat(a[0:*count_a], b[0:*count_b]) by rows of `width` floats, *count_out = rows
 * written (torch.cat of :390-394).  require_a != 0: the result is empty when *count_a == 0.
 * b may be null.  out holds capacity_a + capacity_b rows. */
int pgdvs_concat_rows(const float *a, const int32_t *count_a, int64_t capacity_a, const float *b,
                      const int32_t *count_b, int64_t capacity_b, int width, int require_a,
                      float *out, int32_t *count_out, pgdvs_stream_t stream);

/* A11 alone: combined = (1-m)*static + m*dyn (pgdvs_renderer.py:169-178), n elements per
 * channel, planar [3,n] with mask [n]. */
int pgdvs_combine(const float *static_rgb, const float *dyn_rgb, const float *dyn_mask,
                  int64_t n, float *combined, float *combined_static, float *combined_dyn,
                  pgdvs_stream_t stream);

/* ---- 8f-1, the caller's metric: PGDVSEvaluator.eval_step's image statistics for one view in one pass
 * (pgdvs/engines/evaluator_pgdvs.py:52-77: clamp -> NaN to 0 -> (x*255).byte().float()/255 of prediction and ground
 * truth; :190-283 with pgdvs/utils/training.py:281-313: sum((gt - pred)^2 * mask) and sum(mask) in float64 for the
 * masks ones / eval_mask / 1 - eval_mask).
 *   pred_planar[3,H,W] raw render (combined_rgb); gt_hwc[H,W,3] raw ground truth; mask_hwc[H,W,3] eval_mask
 *   pred_q / gt_q [3,H,W] (nullable): the quantised images
 *   sums: DEVICE double[8] = sum d2, sum d2*m, sum d2*(1-m), 3*H*W, sum m, sum (1-m), then two words that ride along so that
 *   the evaluator's step reads ONE block back: (double)*count_dev (the static cloud's device count; -1 when NULL) and
 *   (double)*status_dev (pgdvs_points_raster_bounded's status word; 0 when NULL)
 *   PSNR_k = 10 log10(1 / (sums[k] / (sums[3+k] + 1e-8))), 0 when the sum of squares is 0 (upstream's quirk). */
int64_t pgdvs_eval_psnr_workspace_bytes(void);
int pgdvs_eval_psnr_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hwc, int H, int W,
                         float *pred_q, float *gt_q, const int64_t *count_dev, const int32_t *status_dev, double *sums,
                         void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- 8f-1, the caller's metric: the evaluator's masked SSIM for one view in one pass (pgdvs/engines/evaluator_pgdvs.py:190-283
 * with pgdvs/utils/training.py:316-346 calculate_ssim: skimage 0.20 structural_similarity(gt, pred, full=True, channel_axis=2,
 * data_range=2.0) -- per channel, 7x7 box means with scipy's "reflect" (half-sample symmetric) border, sample covariance
 * 49/48, C1 = (0.01*2)^2, C2 = (0.03*2)^2, the full map without a border crop -- then sum(S*mask) / (sum(mask) + 1e-8) for
 * the masks ones / eval_mask / 1 - eval_mask).  Inputs are quantised as for pgdvs_eval_psnr_sums; the window sums are exact
 * in integers and S is formed from them in fp32 (skimage filters in float32: the two differ by ~1e-7 per mean).
 *   pred_planar[3,H,W] raw render (combined_rgb); gt_hwc[H,W,3] raw ground truth; mask_hwc[H,W,3] eval_mask
 *   ssim_map [3,H,W] (nullable): S
 *   sums: DEVICE double[8] = sum S, sum S*m, sum S*(1-m), 3*H*W, sum m, sum (1-m), 0, 0 (the layout of the PSNR row, so that
 *   both come back in one transfer); SSIM_k = sums[k] / (sums[3+k] + 1e-8).
 *   H or W below 7 (skimage raises ValueError): PGDVS_ERR_INVALID, and the workspace query returns PGDVS_ERR_INVALID.
 *   workspace >= pgdvs_eval_ssim_workspace_bytes(H,W) (40 bytes per 64x32 tile); deterministic (fixed-order sums). */
int64_t pgdvs_eval_ssim_workspace_bytes(int H, int W);
int pgdvs_eval_ssim_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hwc, int H, int W, float *ssim_map,
                         double *sums, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- 8f-1, the caller's metric: the evaluator's masked LPIPS for one view (pgdvs/engines/evaluator_pgdvs.py:94-110,190-283
 * with trainer_pgdvs.py:132-137 PerceptualLoss(model="net-lin", net="alex", use_gpu=False, version=0.1) -> nsff_lpips/
 * dist_model.py:70-135, networks_basic.py:15-170, pretrained_networks.py:63-105).  Both images are quantised as for
 * pgdvs_eval_psnr_sums and mapped to [-1, 1] (2 q - 1); NO ScalingLayer (PNetLin.forward compares the float version 0.1 with
 * the string "0.1", so the shift / scale never applies on this protocol); AlexNet features[0:12] (conv 11x11/4 pad 2, ReLU,
 * maxpool 3/2, conv 5x5 pad 2, ReLU, maxpool 3/2, conv 3x3 pad 1 + ReLU three times) on the fp32 matrix instruction, once for
 * both images; per relu_k map normalize_tensor, squared difference, the 1x1 lin_k (no bias), and spatial_average with the
 * mask's channel 0 resized to the map by torch's "nearest" rule (src = min(floor(dst * (float)in / out), in - 1)).
 *   pred_planar[3,H,W] raw render (combined_rgb); gt_hwc[H,W,3] raw ground truth; mask_hwc[H,W,3] eval_mask (channel 0 used)
 *   conv_weights: features.{0,3,6,8,10}.weight concatenated in that order, torch layout [Cout][Cin][k][k] (2468544 floats)
 *   conv_biases:  features.{0,3,6,8,10}.bias concatenated (64 + 192 + 384 + 256 + 256 = 1152 floats)
 *   lin_weights:  lin{0..4}.model.1.weight concatenated (1152 floats)
 *   sums: DEVICE double[8] = LPIPS full, LPIPS dyn, LPIPS static, then h1 w1, sum m, sum (1 - m) of the relu1 map, 0, 0.
 *   The kernel finishes the ratios: each of sums[0..2] is already sum_k sum(x_k m_k) / (sum(m_k) + 1e-8) over the five layers
 *   (the division per layer precedes the sum over layers, so a row of plain sums could not carry it); the row keeps the
 *   PSNR / SSIM rows' width so that all of them come back in one transfer.
 *   H or W below 31 (the relu5 map would be empty) or H W >= 2^26: PGDVS_ERR_INVALID, and the workspace query returns
 *   PGDVS_ERR_INVALID.  workspace >= pgdvs_lpips_workspace_bytes(H,W), laid out as (each region rounded up to 256 bytes):
 *   x[2,3,H,W], relu1, pool1, relu2, pool2, relu3, relu4, relu5 (each [2,C,h,w] fp32, ground truth first), head partials.
 *   Deterministic (fixed-order float64 sums). */
int64_t pgdvs_lpips_workspace_bytes(int H, int W);
int pgdvs_lpips_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hwc, int H, int W, const float *conv_weights,
                     const float *conv_biases, const float *lin_weights, double *sums, void *workspace, int64_t workspace_bytes,
                     pgdvs_stream_t stream);

/* ---- 8f-1, the caller's metric, DyCheck iPhone protocol (quant_type "dycheck_iphone", pgdvs/engines/evaluator_pgdvs.py:282-409
 * through pgdvs/utils/dycheck/metrics.py:63-186): PSNR and SSIM of one view with the full mask and the covisibility mask, in
 * one pass.  Both images are quantised as for pgdvs_eval_psnr_sums.  PSNR = -10/ln 10 ln(sum(d^2 m) / max(sum(m over 3
 * channels), 1e-6)) with d over all three channels.  SSIM (modelled on tf.image.ssim): an 11-tap Gaussian (sigma 1.5, sum 1),
 * k1 = 0.01, k2 = 0.03, max_val 1, the mask applied as a partial convolution, separably in two "valid" passes (first along W,
 * then along H; each z' = conv(z m, f) 11 / conv(m, 1) where conv(m, 1) != 0, else 0, the next pass's mask conv(m, 1) != 0),
 * variances clamped at 0, covariance clipped to sign(s01) min(sqrt(s00 s11), |s01|), then the mean over ALL (H-10)(W-10) 3
 * map entries (a window that saw no mask gives exactly 1).  float64 arithmetic on the fp32 quantised values, fixed-order sums
 * (deterministic).
 *   pred_planar[3,H,W] raw render (combined_rgb); gt_hwc[H,W,3] raw ground truth; mask_hw[H,W] eval_mask (its one channel)
 *   sums: DEVICE double[8] (the width of the PSNR row, so that all rows of a step come back in one transfer):
 *     [0] sum d^2   [1] sum d^2 m   [2] sum S (full mask)   [3] 3 H W   [4] 3 sum m   [5] sum S (covisibility mask)
 *     [6] (double)*count_dev (-1 when NULL)   [7] (double)*status_dev (0 when NULL), as in pgdvs_eval_psnr_sums
 *   PSNR = -10/ln 10 ln(sums[0] / max(sums[3], 1e-6)), mPSNR likewise with sums[1] / max(sums[4], 1e-6) (an exact match or an
 *   empty mask gives +inf, as upstream); SSIM = sums[2] / (3 (H-10)(W-10)), mSSIM = sums[5] / (3 (H-10)(W-10)).
 *   H or W below 11 (upstream's map would be empty and its mean NaN): PGDVS_ERR_INVALID, and the workspace query returns
 *   PGDVS_ERR_INVALID.  workspace >= pgdvs_dycheck_psnr_ssim_workspace_bytes(H,W) (64 bytes per 32x32 output tile). */
int64_t pgdvs_dycheck_psnr_ssim_workspace_bytes(int H, int W);
int pgdvs_dycheck_psnr_ssim_sums(const float *pred_planar, const float *gt_hwc, const float *mask_hw, int H, int W,
                                 const int64_t *count_dev, const int32_t *status_dev, double *sums, void *workspace,
                                 int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- 8f-1, the caller's metric, DyCheck iPhone protocol: LPIPS of one view with the full mask and the covisibility mask
 * (metrics.py:189-230 with lpips 0.1.4 LPIPS(net="alex", spatial=True), trainer_pgdvs.py:138-139).  Four images, quantised as for
 * pgdvs_eval_psnr_sums: gt, pred, gt m, pred m, each im2tensor(., factor=1/2) = 2 x - 1 and passed through the ScalingLayer
 * (shift [-.030,-.088,-.188], scale [.458,.448,.450]: version is the string "0.1" here); the AlexNet backbone of
 * pgdvs_lpips_sums on all four; per layer normalize_tensor, squared difference and lin_k for the pairs (gt, pred) and
 * (gt m, pred m); each lin map upsampled to H x W (bilinear, align_corners=False, source (dst + 0.5) in/out - 0.5 clamped at 0),
 * summed over the layers; masked_mean = sum(v m) / max(sum(m), 1e-6) with the full mask on the first pair and eval_mask on the
 * second.  The weights are packed as for pgdvs_lpips_sums.
 *   mask_hw[H,W] eval_mask (its one channel)
 *   sums: DEVICE double[8] = LPIPS full, LPIPS covisible, sum v (first pair), H W, sum v m (second pair), sum m, 0, 0.
 *   H or W below 31 or H W >= 2^26: PGDVS_ERR_INVALID, and the workspace query returns PGDVS_ERR_INVALID.
 *   workspace >= pgdvs_dycheck_lpips_workspace_bytes(H,W), laid out as (each region rounded up to 256 bytes): x[4,3,H,W], relu1,
 *   pool1, relu2, pool2, relu3, relu4, relu5 (each [4,C,h,w] fp32), the five lin maps [2,h,w], the upsampling partials.
 *   Deterministic (fixed-order float64 sums). */
int64_t pgdvs_dycheck_lpips_workspace_bytes(int H, int W);
int pgdvs_dycheck_lpips(const float *pred_planar, const float *gt_hwc, const float *mask_hw, int H, int W, const float *conv_weights,
                        const float *conv_biases, const float *lin_weights, double *sums, void *workspace, int64_t workspace_bytes,
                        pgdvs_stream_t stream);

/* ---- 8f-3 DyCheck, the loader's per-item depth range (pgdvs/datasets/dycheck_iphone_eval.py:455-524): the spatial sources'
 * world points moved into the target camera, np.quantile(z, 0.1 / 0.9) clamped by the scene's near / far as the constant
 * range, then every static point that projects into the image overwrites its pixel with z -+ 1e-4 (the last point wins).
 * Bit-identical to the loader's numpy path (pgdvs_amd/datasets/dycheck_iphone.py depth_range_numpy):
 *   depth [V,H,W] float32 (depth_f64 = 0) or float64 (depth_f64 = 1): the points' type T, as numpy promotes it
 *   dyn_mask [V,H,W] float32, static where == 0
 *   rays [V,12] float32: per view M = c2w[:3,:3] @ inverse(K[:3,:3]) row-major and the origin c2w[:3,3], as
 *     _get_rays_single_image (base.py:507-546) forms them with torch; d = fma(M[:,1], v, M[:,0] u) + M[:,2] (torch's CPU bmm
 *     order), X = o + d depth in T
 *   inv_raw_c2w_tgt[16], inv_c2w_tgt[16], K_tgt[9]: HOST doubles holding float32 values (numpy's float32 inverses of the
 *     target's raw camera-to-world and of flat_cam_tgt's c2w, and flat_cam_tgt's K[:3,:3]); any other value is rejected
 *   near, far: the scene's bounds
 *   depth_range [H,W,2] float32 output; quantiles: DEVICE double[2] (nullable) = np.quantile(z, 0.1), np.quantile(z, 0.9)
 *   as computed in T (NaN when z holds a NaN)
 * Products follow numpy's BLAS order (fused multiply-adds, k ascending; DESIGN.md 8f-3 DyCheck); the quantiles are exact
 * order statistics (radix select on the order-preserving bit patterns, -0.0 counted as +0.0) combined by numpy's _lerp.
 * V, H or W < 1, or V H W >= 2^31: PGDVS_ERR_INVALID, and the workspace query returns PGDVS_ERR_INVALID.
 * workspace >= pgdvs_dycheck_depth_range_workspace_bytes(V,H,W,depth_f64): the keys (V H W x sizeof(T)), a per-pixel int32,
 * the radix histograms and a small state block. */
int64_t pgdvs_dycheck_depth_range_workspace_bytes(int V, int H, int W, int depth_f64);
int pgdvs_dycheck_depth_range(const void *depth, int depth_f64, const float *dyn_mask, const float *rays, int V, int H, int W,
                              const double *inv_raw_c2w_tgt, const double *inv_c2w_tgt, const double *K_tgt, double near_v,
                              double far_v, float *depth_range, double *quantiles, void *workspace, int64_t workspace_bytes,
                              pgdvs_stream_t stream);

/* ---- 8f-3 NVIDIA, the NVIDIA-family loaders' per-item depth range (pgdvs/datasets/nvidia_eval.py:446-456, nvidia_vis.py,
 * mono_vis.py): the spatial sources' world points moved into the target camera, near = max(1e-16, 0.8 min z) and
 * far = max(2e-16, 1.2 np.quantile(z, 0.9)).  Bit-identical to the loaders' numpy path (pgdvs_amd/datasets/nvidia_eval.py:
 * depth_range_from_points over the concatenated compute_pcl of every view):
 *   depth [V,H,W] float32
 *   rays [V,12] float32: per view M = c2w[:3,:3] @ inv(K[:3,:3]) row-major and the origin c2w[:3,3], formed on the host as
 *     compute_pcl forms them (nvidia_eval.ray_constants); d = fma(M[:,1], v, M[:,0] u) + M[:,2] (numpy's float32 BLAS order),
 *     X = o + d depth rounded after the multiply and after the add
 *   inv_c2w_tgt[16]: HOST doubles, numpy's float64 inverse of the target camera-to-world; z = row 2 of it @ [X,1] in float64
 *   depth_range [2] float32 output (DEVICE); near_far: DEVICE double[2] (nullable) = the float64 (near, far) before the cast
 * Products follow numpy's BLAS order (fused multiply-adds, k ascending; DESIGN.md 8f-3 DyCheck).  np.min and the quantile's
 * two order statistics are exact (radix select on the order-preserving bit patterns, -0.0 counted as +0.0), combined by
 * numpy's _lerp.  A NaN in z makes both NaN, so near / far become 1e-16 / 2e-16 (Python's max); infinite depths order as
 * numpy orders them.
 * V, H or W < 1, H W == 1 (a one-pixel view, which numpy unprojects as a matrix-vector product in another order), or
 * V H W >= 2^31: PGDVS_ERR_INVALID, and the workspace query returns PGDVS_ERR_INVALID.
 * workspace >= pgdvs_nvidia_depth_range_workspace_bytes(V,H,W): the keys (V H W x 8 bytes), the radix histograms and a
 * small state block.  One stream, no host synchronisation. */
int64_t pgdvs_nvidia_depth_range_workspace_bytes(int V, int H, int W);
int pgdvs_nvidia_depth_range(const float *depth, const float *rays, int V, int H, int W, const double *inv_c2w_tgt,
                             float *depth_range, double *near_far, void *workspace, int64_t workspace_bytes,
                             pgdvs_stream_t stream);

/* ---- 8f-3 NVIDIA, ZoeDepth inputs (pgdvs/datasets/nvidia_eval.py:869-945): the loader's alignment of a monocular depth
 * prediction with the stored disparity-domain scale and shift, fused with the depth range above (:446-456).  Per pixel, in
 * upstream's order and in the types NumPy 2 gives its three lines (the scale and shift come out of the .npz as 0-d float64
 * arrays, which promote; NumPy 1.x would stay in float32 and is not what this entry computes):
 *   raw_disp = 1.0 / (depth_pred + 1e-16)   float32: an add of float32(1e-16), then a correctly rounded divide
 *   disp     = scale * raw_disp + shift     float64: multiply and add rounded separately (no fused multiply-add)
 *   depth64  = 1 / (disp + 1e-16)           float64
 *   depth    = float32(depth64)             round to nearest, +-inf above the float32 maximum
 * A prediction of exactly 0 has raw_disp = 1e16; disp + 1e-16 == 0 gives inf, a negative one a negative depth; NaN
 * predictions stay NaN (the canonical quiet NaN keeps its bits).
 *   depth_pred [V,H,W] float32; scale_shift [V,2] HOST doubles (scale, shift per view); depth [V,H,W] float32 output
 * With rays, inv_c2w_tgt and depth_range given (all three, or none), the range of pgdvs_nvidia_depth_range follows in the
 * same pass over the pixels, with the world point formed from the float64 depth as upstream's float32 torch rays times a
 * float64 numpy depth are: X = double(o) + double(d) * depth64, multiply and add rounded separately, d the float32
 * direction of the entry above.  z, the order statistics, the NaN rule, -0.0 and the clamps are that entry's; the float64
 * depth is never stored.  near_far (nullable) only with the range.
 * With the three null it is the conversion alone (temporal and tracker views) and workspace may be null.
 * V, H or W < 1, V H W >= 2^31, or H W == 1 with a range: PGDVS_ERR_INVALID; the workspace query (range path's size)
 * returns PGDVS_ERR_INVALID for the same shapes, H W == 1 included.  One stream, no host synchronisation; the scale and
 * shift are read before the call returns. */
int64_t pgdvs_nvidia_zoe_depth_range_workspace_bytes(int V, int H, int W);
int pgdvs_nvidia_zoe_depth_range(const float *depth_pred, const double *scale_shift, const float *rays, int V, int H, int W,
                                 const double *inv_c2w_tgt, float *depth, float *depth_range, double *near_far,
                                 void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- one native call per target view -------------------------------------------------
 * PGDVSRenderer.forward with static_renderer = StaticGeoPointRenderer, dyn_render_type = "softsplat",
 * batch item of size 1, render_stride 1, no tracker (pgdvs/renderers/pgdvs_renderer.py:84-178 ->
 * st_geo_renderer.py:77-120 + pgdvs_renderer_dyn.py:63-257,275-540), as the evaluator drives it once per
 * target view (pgdvs/engines/evaluator_pgdvs.py:36-54) -- and, when agg_S > 0, the static cloud aggregated
 * first from the resident video (A12, nvidia_eval_pure_geo.py:183-277).  Enqueues the whole chain (A12, A9,
 * A2-A5 with the kNN outlier filter, A6-A8, A11) from C++: one ctypes call instead of ~85, same kernels, same
 * results as the per-op entry points above.
 * Every pointer is a DEVICE pointer except agg_K3s_host / agg_c2ws_host. */
typedef struct pgdvs_view_geo_desc {
  int32_t H, W;                 /* source and target resolution (render_stride 1)                      */
  /* cameras and times: rows of the data dict (A0)                                                    */
  const float *flat_cam_tgt;    /* [34]                                                                */
  const float *flat_cam_src;    /* [2,34]  the two temporally closest source frames                    */
  const float *time_src;        /* [2]     time_src_temporal                                           */
  const float *time_tgt;        /* [1]                                                                 */
  /* dynamic branch inputs                                                                            */
  const float *rgb1, *rgb2;     /* [H,W,3] each (rgb_src_temporal[0], [1])                             */
  const float *depth1, *depth2; /* [H,W]                                                               */
  const float *dyn_mask1;       /* [H,W]   0/1 floats (dyn_mask_src_temporal[0])                       */
  const float *flow12;          /* [H,W,2] flow_fwd                                                    */
  const float *flow_occ;        /* [H,W]   flow_fwd_occ_mask (needed when use_flow_consistency)        */
  int32_t use_flow_consistency; /* render_cfg.dyn_render_use_flow_consistency                          */
  int32_t remove_outlier;       /* render_cfg.dyn_pcl_remove_outlier                                   */
  int32_t outlier_knn;          /* render_cfg.dyn_pcl_outlier_knn                                      */
  float outlier_std_thres;      /* render_cfg.dyn_pcl_outlier_std_thres                                */
  float alpha;                  /* softsplat_metric_abs_alpha                                          */
  const float *noise;           /* [3,H,W] injected normal field, or NULL                              */
  uint64_t *rng_state;          /* {seed, draw number} (pgdvs_dyn_splat_composite_rng), or NULL; both NULL: zeros */
  /* static cloud, given ...                                                                          */
  const float *st_pcl_rgb;      /* [st_rows,6] (xyz,rgb); ignored when agg_S > 0                       */
  const float *st_pcl_xyz;      /* [st_rows,3] packed coordinates or NULL                              */
  int64_t st_rows;              /* rows of the two buffers                                             */
  const int64_t *st_count_dev;  /* device count (rows actually present) or NULL = st_rows              */
  /* ... or aggregated inside the call (A12; arguments of pgdvs_static_aggregate_packed)              */
  int32_t agg_S;                /* 0: use st_pcl_rgb                                                   */
  const float *agg_rgbs;        /* [S,H,W,3]                                                           */
  const float *agg_depths;      /* [S,H,W]                                                             */
  const uint8_t *agg_masks;     /* [S,H,W]                                                             */
  const double *agg_K3s_host;   /* HOST [S,9]                                                          */
  const double *agg_c2ws_host;  /* HOST [S,16]                                                         */
  float *agg_cloud_out;         /* [agg_capacity,6]                                                    */
  float *agg_xyz_out;           /* [agg_capacity,3]                                                    */
  int64_t agg_capacity;
  int64_t *agg_count_out;       /* device int64 (or -1, see pgdvs_static_aggregate)                    */
  /* rasteriser                                                                                       */
  int64_t row_bound;            /* rows the tile lists are sized for (<= the buffers' rows); <= 0: all rows */
  float radius;                 /* render_cfg.st_render_pcl_pt_radius                                  */
  int32_t K;                    /* render_cfg.st_render_pcl_pts_per_pixel                              */
  /* outputs, planar                                                                                  */
  float *static_rgb;            /* [3,H,W] geo_static_rgb                                              */
  float *static_mask;           /* [H,W]   geo_static_mask                                             */
  int32_t *raster_status;       /* device int32 (pgdvs_points_raster_bounded)                          */
  float *render_dyn_rgb;        /* [3,H,W]                                                             */
  float *render_dyn_mask;       /* [H,W]                                                               */
  float *combined;              /* [3,H,W] combined_rgb                                                */
  float *combined_static;       /* [3,H,W]                                                             */
  float *combined_dyn;          /* [3,H,W]                                                             */
  /* optional: the dynamic branch's geometry (A2-A5) on a second stream, joined before the splat       */
  pgdvs_stream_t side_stream;   /* NULL: everything on `stream`                                        */
  /* agg_S > 0 only: non-zero = this workspace ran the previous pgdvs_view_geo_forward with the SAME agg_S, H, W,
   * agg_capacity, agg_K3s_host and agg_c2ws_host and nothing else has written to it since: the per-frame camera constants
   * are still in it and are not uploaded again (five launches less per view).  0 is always correct. */
  int32_t agg_params_cached;
} pgdvs_view_geo_desc;

/* sizeof(pgdvs_view_geo_desc) as this library was compiled: a binding checks its own struct against it */
int64_t pgdvs_view_geo_desc_size(void);
/* bytes of workspace pgdvs_view_geo_forward needs for this description (negative status on a bad one) */
int64_t pgdvs_view_geo_workspace_bytes(const pgdvs_view_geo_desc *desc);
int pgdvs_view_geo_forward(const pgdvs_view_geo_desc *desc, void *workspace, int64_t workspace_bytes,
                           pgdvs_stream_t stream);
/* What the fast paths of the LAST pgdvs_view_geo_forward on this (description, workspace) left to their slower exits, read
 * from device words the kernels write anyway: counters_dev = DEVICE int64[PGDVS_VIEW_COUNTERS], written on `stream` (enqueue
 * it behind the forward call, before the workspace is used again). */
#define PGDVS_VIEW_CNT_STATIC_ROWS 0         /* rows of the static cloud (device count)                                   */
#define PGDVS_VIEW_CNT_RASTER_ENTRIES 1      /* tile-list entries of the rasteriser                                       */
#define PGDVS_VIEW_CNT_RASTER_LONGEST 2      /* longest tile list                                                         */
#define PGDVS_VIEW_CNT_RASTER_TILES_LONG 3   /* tiles whose list exceeds the LDS-sorted path's 2048 entries (general path) */
#define PGDVS_VIEW_CNT_RASTER_TILES_TIES 4   /* tiles the sorted path handed to the general path for > 64 equal depths     */
#define PGDVS_VIEW_CNT_KNN_QUERIES 5         /* points of the dynamic cloud the outlier filter searched                   */
#define PGDVS_VIEW_CNT_KNN_TO_RING 6         /* queries the thread-per-query pass left to the ring search                 */
#define PGDVS_VIEW_CNT_KNN_TO_COARSE 7       /* queries the ring search left to the coarse grid                           */
#define PGDVS_VIEW_CNT_KNN_TO_EXHAUSTIVE 8   /* queries scanned exhaustively                                              */
#define PGDVS_VIEW_CNT_AGG_FP64_POINTS 9     /* aggregation: points with projections the fp32 screening left to the fp64 queue */
#define PGDVS_VIEW_CNT_AGG_REFERENCE_ORDER 10 /* aggregation: projections evaluated in the reference's operation order      */
#define PGDVS_VIEW_COUNTERS 12
int pgdvs_view_geo_counters(const pgdvs_view_geo_desc *desc, const void *workspace, int64_t workspace_bytes,
                            int64_t *counters_dev, pgdvs_stream_t stream);
/* host enqueue statistics of pgdvs_view_geo_forward since the last call of this function: calls made and the
 * wall-clock seconds spent inside them (bench.py's host_enqueue figure); resets both. */
void pgdvs_view_geo_host_stats(int64_t *calls, double *seconds);

/* ---- visualiser export ---------------------------------------------------- */
/* The visualiser's two image writers (pgdvs/engines/visualizer_pgdvs.py:118-139) up to the deflate: img_planar[B,3,H,W] ->
 * out[B,H,1+3W] uint8, per row one PNG filter-type byte and then 3 W bytes R G B R G B ... (8-bit truecolour), ready for
 * zlib and an IDAT chunk.  One streaming pass (csrc/png.hip): no workspace, no atomics; rows are independent.
 *   quant     the image is clamped to [0, 1] first, as the visualiser does, then
 *             0  x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- torchvision.utils.save_image (*_combined.png): a float32
 *                multiply and a float32 add, rounded separately, then truncation
 *             1  (x * 255).astype(uint8) -- the numpy cast of *_gnt.png: float32 multiply, truncation
 *             NaN gives 0 in both (upstream casts NaN to uint8, which is undefined: no value to match); +inf 255, -inf 0.
 *   adaptive  0  filter type 0 on every row: out[..., 1:] is the packed [H,W,3] uint8 image
 *             1  per row the PNG specification's filter (None, Sub, Up, Average, Paeth; bytes per pixel 3) with the least
 *                sum over the filtered bytes of v < 128 ? v : 256 - v (libpng's default heuristic), the lowest type number
 *                on a tie.  Integer sums: bit-exact whatever the reduction order.
 * out needs no alignment.  Shapes: B, H, W >= 1 and B H (1 + 3 W) < 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_png_scanlines(const float *img_planar, int B, int H, int W, int quant, int adaptive, uint8_t *out,
                        pgdvs_stream_t stream);

/* ---- visualiser video ------------------------------------------------------ */
/* The frames of the visualiser's video (pgdvs/engines/visualizer_pgdvs.py:141-177, pgdvs/utils/rendering.py:79-116
 * images_to_video) as baseline JPEG, compressed on the device (csrc/jpeg.hip); pgdvs_amd/video.py holds the same codec in
 * numpy integers, the JPEG headers and the AVI container.  Upstream encodes H.264 through ffmpeg; this is Motion-JPEG.
 *
 * Coefficients: img_planar[B,3,H,W] float32 -> coef[B,nby,nbx,3,64] int16 with nby = ceil(H / 8), nbx = ceil(W / 8): per
 * 8 x 8 pixel block the quantised DCT coefficients of Y, Cb and Cr in zigzag order.  One pass: the pixel is quantised as
 * pgdvs_png_scanlines' quant 0 quantises it (so a frame and its *_combined.png hold the same 8-bit image), pixels past the
 * right / bottom edge replicate the last column / row; Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R -
 * 21709 G + 32768 B + 8421375) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16, each - 128; the 13-bit integer
 * DCT of Loeffler, Ligtenberg and Moschytz in the Independent JPEG Group's scaling, rows then columns in int32, which gives
 * 8 x the coefficient; quantisation with one rounding, sign(c) ((|c| + 4 Q) / (8 Q)).  These are libjpeg's coefficients: at
 * the same tables and 4:4:4 PIL writes the same scan.  qtab_luma[64], qtab_chroma[64]: HOST uint16 in natural
 * (row-major) order, each 1 .. 255.  One wavefront per block triple, no atomics, no workspace.  img_planar and coef 4-byte
 * aligned.  Shapes: B >= 1, H and W in 1 .. 65535, 3 B H W and 192 B nby nbx below 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_jpeg_coefficients(const float *img_planar, int B, int H, int W, const uint16_t *qtab_luma, const uint16_t *qtab_chroma,
                            int16_t *coef, pgdvs_stream_t stream);
/* Entropy coding (rendering.py:79-116, the frame writer's place): coef[B,nby,nbx,3,64] int16 -> per frame b the scan data
 * of its one interleaved scan, everything between the SOS header and EOI, contiguous from out + b out_stride, its length in
 * nbytes[b] (device int32); bytes of the slot past that length are not written.  The four typical Huffman tables of T.81
 * Annex K.3; DC as the difference to the previous block of the component, 0 at the start of a restart segment; AC run / size
 * symbols, ZRL, EOB unless coefficient 63 is non-zero; every segment padded with ones to a byte, 0xFF followed by 0x00; RSTm
 * (m cycling 0 .. 7) between segments of restart_mcus MCUs.  On read DC is clamped to -1024 .. 1023 and AC to +-1023, so
 * every symbol exists in the tables whatever the input holds (pgdvs_jpeg_coefficients stays inside those ranges).
 * restart_mcus in 1 .. 65535 (larger than the frame: one segment, no marker); 0, a scan without restart markers, is
 * host-only (video.encode_scan): the device pass compresses segments independently and they must end on bytes.  Three
 * launches, no global atomics, no workgroup waits for another.  out_stride >= 1248 nby nbx + 2 (segments - 1) with
 * segments = ceil(nby nbx / min(restart_mcus, nby nbx)): a block costs at most 20 + 63 x 26 = 1658 bits = 208 bytes,
 * doubled by stuffing.  workspace: pgdvs_jpeg_scan_workspace_bytes bytes, 256-byte aligned (-1 for shapes the call rejects);
 * coef 16-byte aligned, out none.  Shapes: B >= 1, nby and nbx in 1 .. 8192, B out_stride and the workspace below 2^31, else
 * PGDVS_ERR_INVALID. */
int64_t pgdvs_jpeg_scan_workspace_bytes(int B, int nby, int nbx, int restart_mcus);
int pgdvs_jpeg_scan(const int16_t *coef, int B, int nby, int nbx, int restart_mcus, uint8_t *out, int64_t out_stride,
                    int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
/* The same codec at 4:2:0, upstream's chroma format (visualizer_pgdvs.py:141-177 / rendering.py:79-116: imageio's ffmpeg
 * writer without a pixelformat writes yuv420p): chroma at half resolution in both directions, MCUs of 16 x 16 pixels and six
 * blocks in the order Y00, Y01, Y10, Y11, Cb, Cr.  With nmy = ceil(H / 16), nmx = ceil(W / 16), nby = ceil(H / 8), nbx =
 * ceil(W / 8): img_planar[B,3,H,W] float32 -> coef[B,nmy,nmx,6,64] int16 in zigzag order, bit for bit
 * video.jpeg_coefficients(..., subsampling="4:2:0"); PIL writes the same scan at the same tables and subsampling=2.
 *   1 colour   the pixel quantised and transformed as above; columns beyond W - 1 replicate column W - 1 out to 16 nmx.
 *   2 luma     a block with block column < nbx and block row < nby is coded as at 4:4:4 (rows beyond H - 1 replicate row
 *              H - 1).  Every other luma block of the MCU is a dummy block: 63 zero AC coefficients and a QUANTISED DC copied
 *              inside the MCU: a right-edge dummy (block column >= nbx) takes its left neighbour's (Y01 from Y00, Y11 from
 *              Y10); a bottom dummy row (block row >= nby) gives both its blocks the DC of Y01, the block in front of the row
 *              in MCU order, dummy or not, and wins over the right-edge rule.
 *   3 chroma   sample (j, i) with j < ceil(H / 2) is (a + b + c + d + bias) >> 2 over rows min(2j, H - 1), min(2j + 1, H - 1)
 *              and columns 2i, 2i + 1 of the column-replicated Cb (Cr) plane, bias 1 for even i and 2 for odd i, then - 128;
 *              rows j >= ceil(H / 2) replicate the DOWNSAMPLED row ceil(H / 2) - 1.  Chroma has no dummy blocks.
 * One wavefront per MCU, no atomics, no workspace; pointers, tables and the limits on B, H and W as pgdvs_jpeg_coefficients,
 * with 3 B H W and 384 B nmy nmx below 2^31, else PGDVS_ERR_INVALID.
 * pgdvs_jpeg_scan_420: coef[B,nmy,nmx,6,64] -> the one interleaved scan as pgdvs_jpeg_scan writes it, six blocks per MCU:
 * luminance tables for blocks 0 .. 3, chrominance tables for 4 and 5; DC prediction per component in stream order (Y from
 * the previous Y block, across MCUs; Cb from the previous Cb; Cr from the previous Cr), all three 0 at the start of a
 * restart segment; dummy blocks are coded like any other (DC difference, EOB).  restart_mcus counts 16 x 16 MCUs, 1 .. 65535;
 * 0 is host-only as above.  Shapes: B >= 1, nmy and nmx in 1 .. 4096, out_stride >= 2496 nmy nmx + 2 (segments - 1) (six
 * blocks of at most 416 bytes), B out_stride and the workspace below 2^31, else PGDVS_ERR_INVALID (-1 from the query).
 * Alignment and workspace as pgdvs_jpeg_scan. */
int pgdvs_jpeg_coefficients_420(const float *img_planar, int B, int H, int W, const uint16_t *qtab_luma, const uint16_t *qtab_chroma,
                                int16_t *coef, pgdvs_stream_t stream);
int64_t pgdvs_jpeg_scan_420_workspace_bytes(int B, int nmy, int nmx, int restart_mcus);
int pgdvs_jpeg_scan_420(const int16_t *coef, int B, int nmy, int nmx, int restart_mcus, uint8_t *out, int64_t out_stride,
                        int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- PNG deflate ------------------------------------------------------------ */
/* The deflate of the PNG export.  Upstream's images leave through PIL / torchvision (pgdvs/engines/visualizer_pgdvs.py:118-139,
 * evaluator_pgdvs.py:417-465), whose zlib runs on the host, and png.PngWriter's default does the same with
 * zlib.compress(scanlines, 1); this entry point (csrc/png_deflate.hip) writes a zlib stream on the device instead, so that
 * only the compressed bytes cross to the host.  scanlines[n_img][img_bytes]: any bytes (the call knows nothing of rows) ->
 * per image i a complete zlib stream, contiguous from out + i out_stride, its length in nbytes[i] (device int32); bytes of
 * the row past that length are not written.  If the stream would not fit out_stride, nbytes[i] = -1 and nothing of the row
 * is written.  The stream, which pgdvs_amd/png.py restates in integers (deflate_rle) and zlib.decompress accepts: 0x78 0x01;
 * per segment of seg_bytes input bytes (the last one shorter) one non-final dynamic-Huffman block and an empty stored block,
 * so segments start and end on bytes; one final empty fixed block; the Adler-32.  Tokens: runs of equal bytes, cut at segment
 * starts; a run of n is a literal, then (n - 1) / 258 matches of length 258 and distance 1, then for the r bytes left one
 * match if r >= 3, else r literals.  One literal/length code per image from the image's token histogram (286 symbols, the end
 * of block once per segment), limited to 15 bits, canonical and complete, its lengths repeated in every segment's header at
 * 4 bits each; one distance code of length 1.  Three launches, no global atomics, no workgroup waits for another.
 * out_stride >= 8 + 160 segments + ceil(15 img_bytes / 8) always fits (png.deflate_capacity).  workspace:
 * pgdvs_png_deflate_workspace_bytes bytes, 256-byte aligned (-1 for shapes the call rejects); scanlines and out need no
 * alignment.  Shapes: n_img >= 1, img_bytes in 1 .. 2^30, seg_bytes a power of two in 4096 .. 65536, n_img x segments <= 2^20,
 * else PGDVS_ERR_INVALID. */
int64_t pgdvs_png_deflate_workspace_bytes(int n_img, int64_t img_bytes, int seg_bytes);
int pgdvs_png_deflate(const uint8_t *scanlines, int n_img, int64_t img_bytes, int seg_bytes, uint8_t *out, int64_t out_stride,
                      int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);

/* ---- evaluator export ------------------------------------------------------ */
/* The images save_vis_for_eval writes for one view (pgdvs/engines/evaluator_pgdvs.py:417-465: *_gt.png :432-433,
 * *_combined.png :435-440, *_gnt.png :442-452 / *_geo_static.png :453-465) up to the deflate, in ONE launch from the RAW
 * images: gt_hwc[H,W,3] (channel-last, as the dataset gives it), pred_planar[3,H,W], static_planar[3,H,W] or NULL ->
 * out[n,H,1+3W] uint8 with n = 2 or 3, in the order gt, pred, static; each image's scanlines as pgdvs_png_scanlines writes
 * them with quant 1: clamp(0, 1), NaN -> 0, (x * 255) in float32, truncation.  (Upstream writes gt and pred from the
 * evaluator's quantised images, (q / 255 * 255).astype(uint8); for every level q = 0..255 that is q again, so the cast of
 * the clamped raw image gives the same bytes.)  adaptive as for pgdvs_png_scanlines; the bytes of each image are identical
 * to pgdvs_png_scanlines(quant 1) on its planar form.  A row of the channel-last ground truth is already in PNG byte order
 * and is read with contiguous 16-byte loads (W % 4 == 0 and a 16-byte aligned pointer; scalar loads otherwise).  No
 * workspace, no atomics, integer sums; out needs no alignment, the inputs 4 bytes.  Shapes: H, W >= 1 and
 * n H (1 + 3 W) < 2^31, adaptive 0 / 1, else PGDVS_ERR_INVALID. */
int pgdvs_eval_export_scanlines(const float *pred_planar, const float *gt_hwc, const float *static_planar, int H, int W,
                                int adaptive, uint8_t *out, pgdvs_stream_t stream);

/* ---- preprocessing ---------------------------------------------------------- */
/* Forward-backward flow consistency, both directions in ONE launch (pgdvs/preprocess/common.py:211-233 bilinear_sampler /
 * coords_grid, :314-325 compute_occlusion(return_raw=True); compute_flow.py:335-340, 351-358: the ``coord_diff`` of the
 * flows/interval_k/<a>_<b>.npz files): flow12[H,W,2], flow21[H,W,2] float32 (x, y), the layout the .npz stores ->
 * coord_diff_1[H,W,2] (flow12 checked against flow21) and coord_diff_2[H,W,2] (flow21 against flow12).  Per pixel p, in
 * float32 and upstream's operation order, every operation rounded on its own: c1 = p + flow12(p); g = 2 c1 / (W - 1) - 1
 * (rows: H - 1); grid_sample(align_corners=True, padding zeros) of flow21 at g: ix = ((g + 1) / 2) (W - 1), weights
 * w = ix - floor(ix) and 1 - w, the products summed nw, ne, sw, se, a corner outside the image contributing zero (not a
 * clamped texel); coord_diff = p - (c1 + sample).  No flow value is ever turned into an address before it is known to lie
 * in the image.  NaN flows: undefined values, no fault.  No workspace.  Pointers 8-byte aligned.
 * Shapes: H, W >= 2 (upstream divides by W - 1), H < 2^18 - 4, H W < 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_flow_consistency(const float *flow12, const float *flow21, int H, int W, float *coord_diff_1, float *coord_diff_2,
                           pgdvs_stream_t stream);
/* The flow_epi motion mask of one direction in ONE launch (pgdvs/preprocess/compute_mask.py:164-181
 * compute_epipolar_distance, :196-215 read_optical_flow, :311-338 compute_mask_epipolar_flow): flow[H,W,2] and
 * coord_diff[H,W,2] float32 on the device, F = HOST double[9], the row-major fundamental matrix with l_2 = F p_1 (by the
 * convention of inv_c2w_tgt above) -> mask[H,W] uint8 (0 / 1) and, unless NULL, e_dist[H,W] double, already multiplied by
 * the consistency mask.  Per pixel p = (x, y): p2 = p + flow in float32, widened; l = F (x, y, 1); d = |p2x l0 + p2y l1 +
 * l2| / (sqrt(l0^2 + l1^2) + 1e-8) in double; consistent = |cd0| + |cd1| <= consist_thres in float32; e_dist = d
 * consistent; raw = e_dist > threshold.  mask = skimage's binary_opening(raw, disk(1)): erosion with the 3 x 3 cross
 * reading SET pixels outside the image, then dilation reading CLEAR ones.  Distance, threshold, erosion and dilation are
 * one kernel over 64 x 16 tiles with a 2-pixel halo of recomputed raw bits in LDS.  No workspace.  flow, coord_diff and
 * e_dist 8-byte aligned.  Shapes: H, W >= 2, H < 2^18 - 4, H W < 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_epipolar_mask(const float *flow, const float *coord_diff, int H, int W, const double *F, double consist_thres,
                        double threshold, uint8_t *mask, double *e_dist, pgdvs_stream_t stream);
/* FlowFormer's tiled inference after the network (pgdvs/preprocess/compute_flow.py:138-165 compute_weight, :182-209, the tile
 * branch of compute_flow_flowformer; csrc/flow_export.hip): tiles[n,2,ph,pw] float32 on the device, planar, as the network
 * returns them; origins = HOST int32[n][2], (h, w) per tile in upstream's order (:61-82 compute_grid_indices); weight[ph,pw]
 * float32 on the device -> flow[H,W,2] float32, the layout the .npz stores.  Per pixel and component, in float32: acc = +0,
 * cnt = +0; over the tiles in index order that cover the pixel acc = acc + tile w and cnt = cnt + w, product and sum rounded
 * separately; flow = acc / cnt, correctly rounded.  That is upstream's flows += F.pad(flow_pre * weights[idx]),
 * flow_count += F.pad(weights[idx]), flows / flow_count: a tile that does not cover the pixel adds +0 there.  Denormal
 * weights (the rim of a tile at sigma 0.05) are kept, nothing is flushed.  Origins may be unsorted and overlap in any way.
 * One launch, no workspace.  tiles and weight 4-byte aligned, flow 8-byte.  PGDVS_ERR_INVALID unless 1 <= n <= 128,
 * 1 <= ph <= H, 1 <= pw <= W, 0 <= h <= H - ph and 0 <= w <= W - pw for every origin, the tiles cover every pixel (else a
 * pixel were 0 / 0), H < 2^18 - 4 and H W < 2^31. */
int pgdvs_flow_tile_blend(const float *tiles, const int32_t *origins, int n, int ph, int pw, const float *weight, int H, int W,
                          float *flow, pgdvs_stream_t stream);
/* Everything upstream's flow stage derives from a pair's flows, in TWO launches (compute_flow.py:335-340 compute_occlusion,
 * :351-361 the two .npz and the two flow_to_image PNGs; preprocess/common.py:93-205 make_colorwheel, flow_uv_to_colors,
 * flow_to_image; csrc/flow_export.hip, csrc/png.hip): flow12[H,W,2], flow21[H,W,2] float32 on the device ->
 *   coord_diff_1, coord_diff_2 [H,W,2]  exactly pgdvs_flow_consistency's values (the same per-pixel statement); both NULL:
 *                                       the pictures alone, and then H, W >= 1 suffice and flow21 may be NULL as well:
 *                                       ONE picture, rad_max[1] and out[1,H,1+3W]
 *   rad_max[2] float32                  per flow the maximum over the frame of rad = sqrt(u u + v v), float32, square, sum
 *                                       and root rounded on their own; NaN if any radius is NaN, as np.max
 *   out[2,H,1+3W] uint8                 the PNG scanlines of flow_to_image(flow12) and flow_to_image(flow21), filtered as
 *                                       pgdvs_png_scanlines filters (adaptive 0 / 1); out needs no alignment
 * The colour of a pixel, upstream's types under NumPy 2: u, v divided by float32(rad_max + float32(1e-5)); rad again from the
 * normalised pair; a = atan2f(-v, -u) / float32(pi); fk = (a + 1) / 2 * 54; k0 = floor(fk), k1 = k0 + 1 wrapped to 0 at 55,
 * f = fk - k0, all float32; then in double col = (1 - f) wheel[k0] / 255 + f wheel[k1] / 255, col = 1 - rad (1 - col) where
 * rad <= 1, else 0.75 col, and the byte floor(255 col).  wheel is the 55 x 3 Middlebury table (segments 15, 6, 4, 11, 13, 6).
 * rad_max and the normalised u, v are correctly rounded IEEE and equal numpy's bit for bit; atan2f is the device library's,
 * so a byte may differ by one level from a given machine's numpy where 255 col lies next to an integer.  A pixel whose
 * normalised u or v is NaN gives 0 0 0 (upstream's NaN-to-integer cast is undefined); k0 is clamped before it indexes the
 * table.  An infinite flow makes rad_max inf: finite pixels normalise to 0 and come out white, infinite ones are NaN.
 * First launch: coord_diff and the radius maximum, one key per workgroup, grid-strided; second launch: one workgroup per
 * row of either picture reduces the keys, colours the row and the row above it into LDS and filters (each flow is read from
 * memory twice, the second time as "the row above" from the cache).  No atomics.  workspace:
 * pgdvs_flow_pair_export_workspace_bytes(H, W) bytes, 256-byte aligned.  Flows and coord_diffs 8-byte aligned.  Shapes:
 * H, W >= 2 (>= 1 without coord_diff), H W < 2^31, 2 H (1 + 3 W) < 2^31, else PGDVS_ERR_INVALID. */
int64_t pgdvs_flow_pair_export_workspace_bytes(int H, int W);
int pgdvs_flow_pair_export(const float *flow12, const float *flow21, int H, int W, int adaptive, float *coord_diff_1,
                           float *coord_diff_2, float *rad_max, uint8_t *out, void *workspace, int64_t workspace_bytes,
                           pgdvs_stream_t stream);
/* The ZoeDepth stage's look-ups for one frame (pgdvs/preprocess/compute_zoedepth.py:262-294; csrc/zoe_align.hip):
 * pred_depth[H,W] and mask[H,W] float32 and pts3d[P,3] float32 on the device, w2c = HOST double[16] and K = HOST double[9],
 * row-major -> the kept points, in ascending point order: proj_pcl[3,P] double (rows x, y, 1; the first *count entries of
 * each row), pcl_depth_mvs[P] double, pcl_depth_pred[P] float32, index[P] int64 and the device int32 *count.  Float64
 * throughout.  Per point: out = w2c [X,1], im = K out[:3], depth = im[2], (x, y) = im[:2] / im[2]; kept when
 * 0 <= x < W and 0 <= y < H (:272-277), then spline(mask)(y, x) < 0.1 (:282-283), then depth > 1e-3 (:286), upstream's
 * order, each test on the float coordinate; pcl_depth_pred = spline(pred_depth)(y, x) (:290).  spline is
 * scipy.ndimage.map_coordinates(order=3, mode="constant") with float32 output: cubic B-spline coefficients of the whole
 * image in double (per axis, axis 0 first: gain (1 - z)(1 - 1/z), z = sqrt(3) - 2, causal start
 * c0 = (c0 + sum z^i (c_i + z^(n-1) c_(n-1-i))) / (1 - z^(2n-2)), anticausal start
 * c_(n-1) = (z c_(n-2) + c_(n-1)) z / (z^2 - 1)), then 0 for a coordinate outside [0, H-1] x [0, W-1] (so also in the last
 * fractional row and column, which pass the first test: upstream's quirk, kept), else the 4 x 4 taps with mirrored tap
 * indices, rounded to float32 once.  The row pass works on 128-column chunks with a 40-column warm-up on either side and the
 * start sum stops after 64 terms: both below 1e-22 of the image's scale.  No coordinate becomes an index before it is known
 * to lie in the image; NaN coordinates are dropped.  workspace: pgdvs_zoe_sample_workspace_bytes(H, W, P) bytes, 256-byte
 * aligned.  Shapes: H, W >= 2, H W < 2^30, 1 <= P < 2^31, else PGDVS_ERR_INVALID. */
int64_t pgdvs_zoe_sample_workspace_bytes(int H, int W, int64_t P);
int pgdvs_zoe_sample(const float *pred_depth, const float *mask, int H, int W, const float *pts3d, int64_t P, const double *w2c,
                     const double *K, double *proj_pcl, double *pcl_depth_mvs, float *pcl_depth_pred, int64_t *index,
                     int32_t *count, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
/* The scale and shift that align one frame's predicted depths with its COLMAP depths in disparity
 * (compute_zoedepth.py:309-388): pcl_depth_pred[n] float32 and pcl_depth_mvs[n] double on the device ->
 * fit[4] double on the device (disp_indiv_scale_med, disp_indiv_shift_med, disp_indiv_scale_trim, disp_indiv_shift_trim),
 * flag_trim[n] uint8 (0 / 1) and the device int32 *status: bit 0 a sampled prediction < 0 or NaN, bit 1 a COLMAP depth < 0
 * or NaN (upstream's assertions, :313-319; the outputs are then undefined).  Upstream's types under NumPy 2: nn_disp =
 * 1 / (pred + 1e-16) and its median in float32 with 1e-16 added in float32, mvs_disp, the ratios and everything after them
 * in double; np.median of an even count is (a + b) / 2 in the array's type; a negative scale becomes 0; np.quantile(., 0.8)
 * by numpy's linear rule; flag_trim = diff <= threshold.  Medians and the quantile's neighbours are exact order statistics
 * (radix select), the two means float64 tree sums of one workgroup.  workspace: pgdvs_zoe_fit_workspace_bytes(n) bytes,
 * 256-byte aligned.  1 <= n < 2^31, else PGDVS_ERR_INVALID. */
int64_t pgdvs_zoe_fit_workspace_bytes(int64_t n);
int pgdvs_zoe_fit(const float *pcl_depth_pred, const double *pcl_depth_mvs, int64_t n, double *fit, uint8_t *flag_trim,
                  int32_t *status, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
/* The error table of one frame (compute_zoedepth.py:424-465): over the samples of flag_trim[n], diff = pcl_depth_mvs -
 * 1 / (nn_disp scale + shift) in double, nn_disp as above, for scale_shift = HOST double[4][2], the (scale, shift) of
 * med_share, med_indiv, trim_share, trim_indiv -> errors[8] double on the device: mean |diff| of the four pairs, then mean
 * diff of the four.  One workgroup, float64 tree sums.  No workspace.  1 <= n < 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_zoe_errors(const float *pcl_depth_pred, const double *pcl_depth_mvs, const uint8_t *flag_trim, int64_t n,
                     const double *scale_shift, double *errors, pgdvs_stream_t stream);
/* The final motion mask of one frame (pgdvs/preprocess/compute_mask.py:341-471 combine_masks, :184-193 warp_flow, :827-829;
 * csrc/mask_combine.hip), ONE call per frame, no host synchronisation.  On the device: raw_no_warp[H,W] uint8 (the frame's
 * flow_epi or semantic mask), sam[n_seg,H,W] uint8 or bool (any non-zero byte is set; NULL when n_seg = 0) and, from the
 * second frame on, prev_mask[H,W] uint8 (the previous call's next_prev), prev_cnt[H,W] float32 (its dyn_cnt),
 * bwd_flow[H,W,2] and bwd_coord_diff[H,W,2] float32 of <frame>_<previous>.npz; all four NULL on the first frame.
 * cubic_table = HOST float[32][4], the warp's weights (below); may be NULL on the first frame.  img_idx is upstream's frame
 * number.  Outputs, uint8 0 / 1 unless said: warp_prev, dyn_track (untouched on the first frame, may be NULL there),
 * dyn_cnt float32, raw, raw_eroded, final_raw, final_mask, next_prev and, unless NULL, seg_counts[n_seg,2] int32 (n_pix,
 * n_overlap) and seg_selected[n_seg].  dyn_cnt may not alias prev_cnt, nor next_prev prev_mask.
 *   first frame: raw = raw_no_warp; dyn_cnt = raw_no_warp as float (:420).
 *   later frames: bwd_mask = |cd0| + |cd1| <= 1 in float32 (:213); warp_prev = warp(prev_mask) >= 0.5 and bwd_mask (:401,
 *     see the warp); dyn_track = (warp(prev_cnt) / float32(img_idx + 1) * bwd_mask) > float32(dyn_track_thres), the
 *     division correctly rounded (:407); raw = raw_no_warp | erode(warp_prev & dyn_track) (:411-418);
 *     dyn_cnt = warp(prev_cnt) + final_raw, without bwd_mask (:446).
 *   raw_eroded = erode(raw) (:427).  Per segment n_pix and n_overlap = |segment & raw_eroded|, exact integers; selected when
 *     n_overlap > 0 and double(n_overlap) > sam_overlap_thres * double(n_pix), strictly (:437-439); final_raw = raw_eroded |
 *     every selected segment (:441); final_mask = dilate(final_raw) (:449); next_prev = erode(final_raw) (:827).
 *   erode / dilate: skimage's binary_erosion / binary_dilation with disk(2), the 13 pixels with dx^2 + dy^2 <= 4; the
 *     erosion reads SET pixels outside the image, the dilation CLEAR ones.
 *   warp(img)(p): this project's statement of cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0), float32, every operation rounded
 *     on its own: x = flow_x + col clamped to [-8, W + 8] (a NaN becomes -8; y alike); s = rint(32 x), half to even;
 *     ix = s >> 5, k = s & 31; cx = cubic_table[k]; the 4 x 4 taps at ix - 1 .. ix + 2, iy - 1 .. iy + 2, a tap outside
 *     the image 0; w[j][i] = cy[j] cx[i]; each row ((v0 w0 + v1 w1) + v2 w2) + v3 w3, the rows added top to bottom.  The
 *     mask is warped as 0.0 / 1.0.  No flow value becomes an address before it is known to lie in the image; NaN flows:
 *     undefined values, no fault.
 * workspace: pgdvs_mask_combine_workspace_bytes(H, W, n_seg) bytes, 256-byte aligned.  bwd_flow and bwd_coord_diff 8-byte
 * aligned.  Shapes: H, W >= 1, each < 2^20 (tile rows ride grid.y), H W < 2^31 (the counts are int32), 0 <= n_seg < 65536
 * (segments ride grid.y), 0 <= img_idx < 2^24, else PGDVS_ERR_INVALID (the workspace query too) and nothing is launched. */
int64_t pgdvs_mask_combine_workspace_bytes(int H, int W, int n_seg);
int pgdvs_mask_combine(const uint8_t *raw_no_warp, const uint8_t *sam, int n_seg, int H, int W, const uint8_t *prev_mask,
                       const float *prev_cnt, const float *bwd_flow, const float *bwd_coord_diff, const float *cubic_table,
                       int img_idx, double dyn_track_thres, double sam_overlap_thres, uint8_t *warp_prev, uint8_t *dyn_track,
                       float *dyn_cnt, uint8_t *raw, uint8_t *raw_eroded, uint8_t *final_raw, uint8_t *final_mask,
                       uint8_t *next_prev, int32_t *seg_counts, uint8_t *seg_selected, void *workspace, int64_t workspace_bytes,
                       pgdvs_stream_t stream);
/* The semantic raw mask (compute_mask.py:367-380): sem_ade20k[H,W] and sem_coco[H,W] int64 class ids on the device, counted
 * from 0, -1 for "no class"; ids_ade20k[n_ade20k] and ids_coco[n_coco] = HOST int32 lists of the dynamic classes, counted
 * from 1 (1 <= id <= 512) -> ade20k, coco and sem = ade20k | coco, uint8 [H,W] 0 / 1: a pixel is set when its id + 1 is
 * listed.  One launch, no workspace.  Shapes: H, W >= 1, each < 2^20, H W < 2^31, else PGDVS_ERR_INVALID. */
int pgdvs_semantic_mask(const int64_t *sem_ade20k, const int64_t *sem_coco, int H, int W, const int32_t *ids_ade20k, int n_ade20k,
                        const int32_t *ids_coco, int n_coco, uint8_t *ade20k, uint8_t *coco, uint8_t *sem, pgdvs_stream_t stream);
/* CoTracker's correlation step without the correlation volume (csrc/cotracker.hip).
 * pgdvs_cotracker_pyramid replaces CorrBlock.__init__ (pgdvs/models/cotracker/models/core/cotracker/blocks.py:270-284):
 * fmaps[S,C=128,H,W] float32 on the device -> the four levels fmaps, avg_pool2d(2, stride=2) of it, and so on, level l of
 * H >> l x W >> l pixels (an odd last row or column is dropped), each mean ((a00 + a01) + a10) + a11 times 0.25.  The
 * levels are stored channels-last, [S, H_l, W_l, 128], one after the other in `workspace`, each from a 256-byte boundary: a
 * pixel's 128 channels are one 512-byte line.  The workspace IS the pyramid that pgdvs_cotracker_corr_lookup reads.
 * workspace: pgdvs_cotracker_pyramid_workspace_bytes(S, C, H, W) bytes, 256-byte aligned.  Shapes: S >= 1 (the call itself:
 * S < 65536), C = 128, 16 <= H, W < 2^15 (every level 2 x 2 or more: on a 1-pixel level the reference divides by W - 1 = 0),
 * S H W < 2^31, else PGDVS_ERR_INVALID (the workspace query too) and nothing is launched.
 * pgdvs_cotracker_corr_lookup replaces CorrBlock.corr followed by CorrBlock.sample (:286-328, bilinear_sampler :251-266):
 * pyramid as above for (S, H, W), feats[S,N,128] and coords[S,N,2] (x, y in level-0 pixels) float32 on the device ->
 * 196 float32 per (s, n) at out[(s N + n) row_stride + col_offset + level 49 + i 7 + j], nothing else of out written:
 * the sample of corr_l = <feats[s,n], level l> / sqrt(128) (float32 square root and division) at
 * (x / 2^l + (i - 3), y / 2^l + (j - 3)): the SLOW index i moves x, as in the reference, whose delta is (dy, dx) added to
 * (x, y).  Sampling is grid_sample(align_corners=True, zero padding) after the float32 round trip g = 2 x / (W_l - 1) - 1,
 * ix = (g + 1) / 2 * (W_l - 1), every operation rounded on its own.  Since bilinear sampling is linear the samples are
 * taken from the dots <feats, tap> of the 8 x 8 taps they touch, each sample blending the 2 x 2 taps around its own
 * round-tripped position with grid_sample's weights; a tap outside the level is 0.  Within a few float32 spacings of an
 * integer the round trip can put the samples of an axis on either side of their integers; they then touch nine taps along
 * it, and all nine are fetched.  No coordinate becomes an index before it is known to lie in the level: positions are
 * clamped as floats to [-16, W_l + 16] before they become integers (nothing that far out touches the level), every tap is
 * compared with the level; non-finite coordinates give unspecified values and no fault.  No atomics: sums have a fixed
 * order and two calls give the same bits.  feats 16-byte aligned.  Shapes as above and N >= 1, S N 196 < 2^31, 0 <=
 * col_offset, col_offset + 196 <= row_stride (in floats), else PGDVS_ERR_INVALID and nothing is launched. */
int64_t pgdvs_cotracker_pyramid_workspace_bytes(int S, int C, int H, int W);
int pgdvs_cotracker_pyramid(const float *fmaps, int S, int C, int H, int W, void *workspace, int64_t workspace_bytes,
                            pgdvs_stream_t stream);
int pgdvs_cotracker_corr_lookup(const void *pyramid, int S, int H, int W, const float *feats, const float *coords, int N, float *out,
                                int64_t row_stride, int64_t col_offset, pgdvs_stream_t stream);
/* The resident loaders' item builder (csrc/item_gather.hip; pgdvs_amd/datasets/resident.py).  A scene's source frames stay on
 * the device as stored: rgb uint8 [H,W,3] (the pixels before / 255), dyn_mask uint8 [H,W], depth float32 [H,W], frame f of
 * each table at base + f * slot BYTES; bases and slots are multiples of 16.  depth may be NULL when no group asks for it.
 * pgdvs_item_views builds every source-view entry of one item in one launch: ids[n_views] (HOST, 0 <= id < F, repeats in
 * any order allowed) are the frames of the item's groups one after the other, group g of group_sizes[g] (HOST) views;
 * out[5 g + 0..4] (HOST array of device pointers) are group g's rgb [n,H,W,3], dyn_mask [n,H,W,1], dyn_rgb [n,H,W,3],
 * static_rgb [n,H,W,3] and depth [n,H,W,1] or NULL (a group without depth), float32, 4-byte aligned.  Ids and bases travel
 * as kernel arguments.  For view v of frame f: rgb = float(byte) / 255.0f (an IEEE division), dyn_mask = float(mask byte),
 * dyn_rgb = rgb * dyn_mask, static_rgb = rgb * (1 - dyn_mask), depth copied: the bits of the loaders' numpy statements.
 * Four pixels per lane with 16-byte stores where a view's output bases are 16-byte aligned (always when H W % 4 == 0 and
 * the tensors' bases are), one pixel per lane otherwise and for the last H W % 4 pixels.  Nothing outside the outputs is
 * written.  Shapes: F, H, W >= 1, H, W < 2^20, H W < 2^31, 1 <= n_views <= PGDVS_ITEM_MAX_VIEWS, 1 <= n_groups <=
 * PGDVS_ITEM_MAX_GROUPS, every group_sizes[g] >= 1 and their sum n_views, else PGDVS_ERR_INVALID and nothing is launched.
 * pgdvs_flow_occ is the flow files' occlusion mask (pgdvs/datasets/nvidia_eval.py:1005-1009): coord_diff[H,W,2] float32, 8-byte
 * aligned -> occ[H,W] float32 = |cd.x| + |cd.y| > thres ? 1 : 0, the sum in float32, the compare strict; NaN gives 0. */
#define PGDVS_ITEM_MAX_VIEWS 64
#define PGDVS_ITEM_MAX_GROUPS 4
int pgdvs_item_views(const uint8_t *rgb, const uint8_t *dyn_mask, const float *depth, int F, int H, int W, int64_t rgb_slot,
                     int64_t mask_slot, int64_t depth_slot, const int32_t *ids, int n_views, const int32_t *group_sizes, int n_groups,
                     float *const *out, pgdvs_stream_t stream);
int pgdvs_flow_occ(const float *coord_diff, int H, int W, float thres, float *occ, pgdvs_stream_t stream);
/* The resident store's ZoeDepth depths (csrc/depth_range.hip; a scene of pgdvs_amd/datasets/resident.py opened in prediction
 * mode): the depth table holds each frame's depth_pred (float32 [H,W], frame f at pred + f * pred_slot BYTES, base and slot
 * multiples of 16), and one launch writes the aligned depths of all of an item's groups.  ids[n_views] and group_sizes
 * [n_groups] as pgdvs_item_views takes them (HOST; ids may repeat, in any order); scale_shift[n_views][2] HOST doubles, the
 * (scale, shift) of every VIEW, read before the call returns (they travel as kernel arguments); out[g] (HOST array of
 * device pointers) group g's depth [n,H,W] float32, 4-byte aligned.  Per pixel exactly the three lines of
 * pgdvs_nvidia_zoe_depth_range (one device function serves both entries): raw = 1.0f / (pred + float32(1e-16)) in float32,
 * disp = scale * double(raw) + shift with multiply and add rounded separately, depth64 = 1.0 / (disp + 1e-16), and the
 * output float32(depth64).  With rays [n_range,12] (DEVICE float32), inv_c2w_tgt[16] (HOST) and depth_range[2] (DEVICE
 * float32) given (all three or none; near_far, DEVICE double[2], only with them), n_range = group_sizes[0], the spatial
 * group: the float64 depths of its views are unprojected as that entry unprojects them, view-major, and the select passes
 * and the finish of pgdvs_nvidia_depth_range give the range; the float64 depth is never stored.
 * Four pixels per lane with 16-byte loads and stores where a view's output base is 16-byte aligned, one pixel per lane for
 * the last H W % 4 pixels and for a whole view otherwise.  Nothing outside the outputs and the workspace is written.
 * A call without a range takes no workspace (NULL, 0); with one, workspace >= pgdvs_item_zoe_depths_workspace_bytes(n_range,
 * H, W), 16-byte aligned.  F, H, W >= 1, H, W < 2^20, H W < 2^31, 1 <= n_views <= PGDVS_ITEM_MAX_VIEWS, 1 <= n_groups <=
 * PGDVS_ITEM_MAX_GROUPS, every group_sizes[g] >= 1 and their sum n_views, 0 <= ids[v] < F; with a range H W >= 2 and n_range
 * H W < 2^31: else PGDVS_ERR_INVALID (the workspace query too) and nothing is launched.  One stream, no host
 * synchronisation. */
int64_t pgdvs_item_zoe_depths_workspace_bytes(int n_range, int H, int W);
int pgdvs_item_zoe_depths(const float *pred, int F, int H, int W, int64_t pred_slot, const int32_t *ids, int n_views,
                          const double *scale_shift, const int32_t *group_sizes, int n_groups, float *const *out, const float *rays,
                          const double *inv_c2w_tgt, float *depth_range, double *near_far, void *workspace, int64_t workspace_bytes,
                          pgdvs_stream_t stream);
/* The DyCheck loader's target (pgdvs/datasets/dycheck_iphone_eval.py:410-417, 617, 642), expanded on the device from the bytes
 * the files hold: rgb uint8 [H,W,3] -> rgb_out float32 [H,W,3] = float(byte) / 255.0f (an IEEE division: the bits of
 * ``raw.astype(np.float32) / 255.0``); covisible uint8 [H,W] -> mask_out float32 [H,W,1] = covisible > 0 ? 1 : 0 (the bits of
 * ``(covisible > 0).astype(np.float32)``).  covisible and mask_out are both NULL (an image alone) or both given.  Four
 * pixels per lane with 16-byte stores where the inputs and the outputs are 16-byte aligned, one pixel per lane for the last
 * H W % 4 pixels and for the whole image otherwise; outputs 4-byte aligned.  Nothing outside the outputs is written.  H, W
 * >= 1, H, W < 2^20, H W < 2^31, else PGDVS_ERR_INVALID and nothing is launched. */
int pgdvs_item_target(const uint8_t *rgb, const uint8_t *covisible, int H, int W, float *rgb_out, float *mask_out,
                      pgdvs_stream_t stream);
/* The loaders' image resize on the device (csrc/resample.hip): Pillow's 8-bit resampler, Image.resize(resample=BOX) and
 * Image.resize(resample=LANCZOS) of "L" and "RGB" images, bit for bit.
 * pgdvs_resample_table (HOST only; never touches the GPU) replaces precompute_coeffs + normalize_coeffs_8bpc
 * (src/libImaging/Resample.c) for one axis of in_size -> out_size pixels: bounds[out_size][2] = (first input index, tap
 * count n) and kk[out_size][ksize] = the 22-bit fixed-point coefficients, zero past n, the doubles formed in Pillow's order
 * with libm's sin.  Returns ksize = 2 ceil(support max(in / out, 1)) + 1 (support 0.5 for box, 3 for lanczos); with bounds
 * and kk both NULL only that.  Sizes outside 1 .. PGDVS_RESAMPLE_MAX_SIZE, another filter, or ksize above
 * PGDVS_RESAMPLE_MAX_TAPS (a lanczos reduction beyond 42 : 1, a box reduction beyond 254 : 1; the horizontal pass stages a
 * tile's taps in 16 KB of LDS): -1 with a pgdvs_last_error text, nothing written.
 * pgdvs_resample_u8 replaces ImagingResampleHorizontal_8bpc + ImagingResampleVertical_8bpc: in uint8 [N,Hin,Win,C], C 1 or 3,
 * frame i at in + i * in_stride BYTES, -> out [N,Hout,Wout,C], frame i at out + i * out_stride bytes (a frame contiguous; the
 * strides at least a frame, so the output may be a padded slot of the resident store; bytes between frames are not
 * written).  The tables of the axes that change are DEVICE pointers, as pgdvs_resample_table made them for (Win, Wout) and
 * (Hin, Hout) with the same filter: the caller uploads them; for an axis that keeps its size they are ignored and the pass
 * is skipped, and with both kept the op is a copy.  Horizontal pass first, over the input rows the vertical pass reads,
 * into a uint8 intermediate image in the workspace (its 8-bit rounding is part of the result); each pass is
 * clamp((2^21 + sum k * byte) >> 22, 0, 255) in int32.  No alignment is asked of in or out; the workspace is 4-byte aligned,
 * >= pgdvs_resample_u8_workspace_bytes (0 unless both axes change).  One stream, no host synchronisation.  1 <= N <= 65535
 * and the table entry's limits, else PGDVS_ERR_INVALID (the workspace query too) and nothing is launched. */
#define PGDVS_RESAMPLE_BOX 0
#define PGDVS_RESAMPLE_LANCZOS 1
#define PGDVS_RESAMPLE_MAX_SIZE 16384
#define PGDVS_RESAMPLE_MAX_TAPS 256
int pgdvs_resample_table(int in_size, int out_size, int filter, int32_t *bounds, int32_t *kk);
int64_t pgdvs_resample_u8_workspace_bytes(int N, int Hin, int Win, int C, int Hout, int Wout, int filter);
int pgdvs_resample_u8(const uint8_t *in, int64_t in_stride, int N, int Hin, int Win, int C, uint8_t *out, int64_t out_stride, int Hout,
                      int Wout, int filter, const int32_t *bounds_h, const int32_t *kk_h, const int32_t *bounds_v, const int32_t *kk_v,
                      void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
/* The loaders' JPEG reader (csrc/jpeg_entropy.cpp on the host, csrc/jpeg_decode.hip on the device): what
 * np.array(PIL.Image.open(f)) gives for a baseline YCbCr file, byte for byte (Pillow over libjpeg-turbo: the islow inverse
 * DCT, fancy upsampling, jdcolor's tables).
 * SERVED: SOF0 (baseline, 8 bit, Huffman), exactly three components read as YCbCr (a JFIF APP0, or component ids 1 2 3; no
 * Adobe APP14), luma sampling 1x1, 2x1 or 2x2 with chroma 1x1, one interleaved scan (Ss 0, Se 63, Ah Al 0), 8-bit DQT, width
 * and height 1 .. PGDVS_RESAMPLE_MAX_SIZE, with or without restart intervals, the scan closed by EOI.  Everything else --
 * progressive, SOF1/2/..., arithmetic coding, greyscale, CMYK/YCCK, RGB (keep_rgb) streams, 4:1:1, 4:4:0 and other
 * factors, 16-bit tables, several scans, anything truncated or malformed -- is refused, never approximated.  APPn / COM
 * segments are skipped (EXIF orientation is not applied, as Pillow does not).
 * The two HOST entries never touch the GPU.  Both return 0 = served, 1 = a stream this path does not serve (the reason in
 * pgdvs_last_error; the caller falls back to Pillow; nothing was written, but for a scan found corrupt while it was decoded:
 * coef then holds the blocks in front of the fault) and -1 for argument errors alone (a null pointer, a coef_bytes that is not
 * the stream's).
 * pgdvs_jpeg_parse replaces jpeg_read_header (jdmarker.c, jdinput.c's initial_setup / per_scan_setup): the markers up to
 * SOS, then the scan's extent up to its EOI.  blocks_w / blocks_h: every component's block grid padded to whole MCUs
 * (ceil(width / (8 hmax)) MCUs of h blocks across); coef_bytes = 128 * the blocks of all three; quant[c] = component c's
 * table de-zigzagged into natural (row-major) order.
 * pgdvs_jpeg_entropy_decode replaces decode_mcu (jdhuff.c) with process_restart: the scan's quantised coefficients as int16
 * in natural order, coef[component][block row][block col][64] over the padded grids, every block an MCU carries included,
 * zero where the stream gives none.  A bad code, a missing or misnumbered RSTn, data running out before the last MCU or a
 * run past the 64th coefficient returns 1 (libjpeg would warn and go on: Pillow then decides).  Never reads outside
 * data[0 .. nbytes) nor writes outside coef[0 .. coef_bytes). */
#define PGDVS_JPEG_444 0
#define PGDVS_JPEG_422 1
#define PGDVS_JPEG_420 2
typedef struct pgdvs_jpeg_info {
  int32_t width, height;
  int32_t sampling;         /* PGDVS_JPEG_444 / _422 / _420 */
  int32_t restart_interval; /* MCUs; 0 = none */
  int32_t blocks_w[3], blocks_h[3];
  int64_t coef_bytes;
  uint16_t quant[3][64];
} pgdvs_jpeg_info;
int64_t pgdvs_jpeg_info_size(void); /* sizeof(pgdvs_jpeg_info), for bindings that restate the struct */
int pgdvs_jpeg_parse(const uint8_t *data, int64_t nbytes, pgdvs_jpeg_info *info);
int pgdvs_jpeg_entropy_decode(const uint8_t *data, int64_t nbytes, int16_t *coef, int64_t coef_bytes);
/* pgdvs_jpeg_reconstruct replaces everything behind the entropy decoder: jpeg_idct_islow with its dequantisation
 * (jidctint.c), jdsample.c's h2v1 / h2v2 fancy upsampling and jdcolor.c's ycc_rgb_convert.  coef: DEVICE int16, as
 * pgdvs_jpeg_entropy_decode wrote them, 16-byte aligned; quant: DEVICE uint16 [3][64] = info->quant, 16-byte aligned; info:
 * HOST, as pgdvs_jpeg_parse filled it (its sizes are checked again: the block grids must be the ones width, height and
 * sampling give); out: DEVICE uint8 [height][width][3], row y at out + y * row_stride bytes (row_stride >= 3 width, any
 * alignment: a row whose address is a multiple of 4 is written in dwords), nothing between rows or outside the image is
 * written.  Two launches on `stream`, no host synchronisation:
 *   1. dequantise and inverse DCT into 8-bit component planes over the padded grids, in the workspace: columns first,
 *      DESCALE(.., 11), then rows, DESCALE(.., 18), + 128, clamped to 0 .. 255, all in int32.  (For sums outside -384 .. 639
 *      libjpeg's C code wraps through its range table and its SIMD code saturates; such sums do not come from an encoder
 *      fed 8-bit images, and this path clamps.)
 *   2. chroma to full size over the component's ceil(width / 2) x ceil(height / 2) real samples (4:2:0; 4:2:2: full height):
 *      h2v1 (3a + b + 1) >> 2, (3a + b + 2) >> 2 with the end samples copied; h2v2 column sums 3 near + far, then (3s + last +
 *      8) >> 4, (3s + next + 7) >> 4, (4s + 8) >> 4 and (4s + 7) >> 4 at the ends, the rows beyond the first and last
 *      repeating them; plain replication where the component is at most 2 samples wide; then R = Y + ((91881 cr + 32768)
 *      >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), cb cr less 128, clamped.
 * workspace: 256-byte aligned, >= pgdvs_jpeg_reconstruct_workspace_bytes(info) (-1 for an info it refuses). */
int64_t pgdvs_jpeg_reconstruct_workspace_bytes(const pgdvs_jpeg_info *info);
int pgdvs_jpeg_reconstruct(const int16_t *coef, const uint16_t *quant, const pgdvs_jpeg_info *info, uint8_t *out, int64_t row_stride,
                           void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
/* The same scan read on the device (csrc/jpeg_scan_core.h: the decoder; csrc/jpeg_entropy.cpp: preparation and host
 * emulation; csrc/jpeg_scan_decode.hip: the kernels): pgdvs_jpeg_entropy_decode's coefficients bit for bit, with only the
 * file's bytes crossing the bus.  The scan is cut into subsequences of sub_bytes bytes inside each restart segment; each is
 * decoded from a guessed entry state and again whenever its predecessor's exit state says otherwise, until no state changes
 * (the bounds are the counts themselves: an intact stream always converges); then every subsequence writes its coefficients
 * and the DC differences are summed.
 * pgdvs_jpeg_scan_prepare: HOST, one pass over the scan's bytes and no Huffman work.  Refuses (1, the reason in
 * pgdvs_last_error) exactly what pgdvs_jpeg_parse refuses, a missing or misnumbered RSTn marker, and a scan of more than
 * PGDVS_JPEG_SCAN_MAX_BYTES bytes (such files stay with the host decoder; the cap keeps every workspace below 2^31 bytes and
 * bit positions in 32 bits).  Fills `prepared` (8-byte aligned, prepared_bytes >= pgdvs_jpeg_scan_prepare_bytes(..): pinned
 * memory for one asynchronous copy) with a header, info->quant, the scan's six derived Huffman tables (jdhuff's maxcode /
 * valoffset / huffval behind a 9-bit look-ahead), the segment table (bit start and end, first MCU and MCU count =
 * restart_interval but for the last, first subsequence), every subsequence's segment, and the scan with its FF 00 stuffing
 * and RSTn markers removed; and `info` as pgdvs_jpeg_parse does.  sub_bytes: 0 for PGDVS_JPEG_SCAN_SUB_BYTES, else a
 * multiple of 4 in 16 .. 4096.  -1 for argument errors alone.  Never reads outside data[0 .. nbytes) nor writes outside
 * prepared[0 .. prepared_bytes).  pgdvs_jpeg_scan_prepare_bytes: the size to provide; 0 for a stream prepare refuses, -1
 * for argument errors.
 * pgdvs_jpeg_scan_decode: prepared_host: HOST, the buffer as filled (only its header is read, and checked: the launch list
 * follows from it alone); prepared: DEVICE, a copy of the same prepared_bytes bytes, 16-byte aligned; coef: DEVICE int16,
 * coef_bytes = info->coef_bytes, 16-byte aligned, laid out as pgdvs_jpeg_entropy_decode does; status: DEVICE, one word;
 * workspace: DEVICE, 256-byte aligned, >= pgdvs_jpeg_scan_decode_workspace_bytes(prepared_host, prepared_bytes) (-1 for a
 * header it refuses).  Launches on `stream` and returns: no host synchronisation.  *status is 0 only if every restart
 * segment produced exactly its MCUs (PGDVS_JPEG_SCAN_SHORT otherwise; _LEFT_OVER: a byte or more of data between a
 * segment's last MCU and its RSTn), no verified decode met a code the table lacks, a DC size above 15, a run past
 * coefficient 63 or the end of its segment's data (_BAD_CODE), no DC value left 16 bits (_DC_RANGE) and the verified pass
 * met the states the synchronisation left (_NOT_SYNCHRONISED; never set by construction).  With a non-zero status coef
 * holds no result: the caller reruns the file through pgdvs_jpeg_entropy_decode, which decides.  Whatever the bytes of
 * `prepared` hold, nothing outside it is read and nothing outside coef, status and the workspace is written.
 * The workspace's first two words, for tools: the rounds of the first launch (the largest of any workgroup) and the fix-up
 * launches that did not leave at once.
 * pgdvs_jpeg_scan_decode_host: the same launches one after the other on the CPU, HOST pointers throughout (prepared_host and
 * prepared may be the same buffer; 8-byte alignment suffices): the same core, rounds, flags and workspace.  0, or -1 for
 * argument errors. */
#define PGDVS_JPEG_SCAN_SUB_BYTES 64
#define PGDVS_JPEG_SCAN_MAX_BYTES (1 << 25)
#define PGDVS_JPEG_SCAN_SHORT 1
#define PGDVS_JPEG_SCAN_BAD_CODE 2
#define PGDVS_JPEG_SCAN_DC_RANGE 4
#define PGDVS_JPEG_SCAN_NOT_SYNCHRONISED 8
#define PGDVS_JPEG_SCAN_LEFT_OVER 16
int64_t pgdvs_jpeg_scan_prepare_bytes(const uint8_t *data, int64_t nbytes, int32_t sub_bytes);
int pgdvs_jpeg_scan_prepare(const uint8_t *data, int64_t nbytes, int32_t sub_bytes, void *prepared, int64_t prepared_bytes,
                            pgdvs_jpeg_info *info);
int64_t pgdvs_jpeg_scan_decode_workspace_bytes(const void *prepared_host, int64_t prepared_bytes);
int pgdvs_jpeg_scan_decode(const void *prepared_host, const void *prepared, int64_t prepared_bytes, int16_t *coef, int64_t coef_bytes,
                           uint32_t *status, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
int pgdvs_jpeg_scan_decode_host(const void *prepared_host, const void *prepared, int64_t prepared_bytes, int16_t *coef, int64_t coef_bytes,
                                uint32_t *status, void *workspace, int64_t workspace_bytes);

/* PNG frames and mask files read on the device (csrc/png_inflate_core.h: the inflate core; csrc/png_inflate.hip and
 * csrc/png_unfilter.hip: the kernels; csrc/png_decode_host.cpp: the host emulation): the zlib stream of a non-interlaced file
 * is inflated, checked against its Adler-32 and unfiltered into uint8 [H,W,out_channels], byte for byte what a PNG reader
 * gives.  The host parses the chunks (Python: ops.png_info) and does no Huffman work; a launch takes a BATCH of streams, one
 * workgroup each.
 * The batch buffer: a table of nstreams pgdvs_png_image, padded to 16 bytes, then the streams, each at a 16-byte aligned
 * `offset` from the buffer's start with `size` bytes (the two zlib header bytes, which the caller has checked -- deflate,
 * a window of at most 32K, no preset dictionary --, the deflate blocks and the four Adler bytes), padded to a multiple of 4
 * bytes.  height, width: 1 .. 16384; out / row_stride: the image's first byte and the bytes between rows, row_stride >=
 * width * out_channels, any alignment.  An entry is one of two, and both may share a batch:
 *   a COLOUR stream  an 8-bit RGB or RGBA file.  channels: the file's, 3 or 4; out_channels: 3 (an RGBA file's alpha is
 *                    dropped) or `channels`; bit_depth 8 and scale 1, stated.
 *   a ONE-CHANNEL stream  a file of colour type 0 (grey) or 3 (palette; its indices, the palette is never applied) -- the mask
 *                    files.  channels = out_channels = 1, bit_depth 1, 2, 4 or 8 and scale >= 1 with
 *                    scale * (2^bit_depth - 1) <= 255: out is uint8 [H,W], every sample times scale (Pillow's array of a grey
 *                    file: scale 1, 85, 17, 1 at depth 1, 2, 4, 8; of a palette file: 1).  Below 8 bits a row is
 *                    ceil(width * bit_depth / 8) bytes behind its filter byte, the filters work on those bytes, each
 *                    reconstructed byte gives 8 / bit_depth pixels from its most significant bits on, and pixels at
 *                    x >= width are dropped whatever the padding bits hold.
 * The inflated size, height * (1 + ceil(width * channels * bit_depth / 8)), and size stay at or below
 * PGDVS_PNG_INFLATE_MAX_BYTES: positions fit 32 bits.
 * pgdvs_png_decode: batch_host: HOST, the buffer as filled (only its table is read, and checked: the launches follow from
 * it alone); batch: DEVICE, a copy of the same batch_bytes bytes, 16-byte aligned; sub_bytes: 0 for
 * PGDVS_PNG_INFLATE_SUB_BYTES, else a multiple of 4 in 8 .. 1024; status: DEVICE, nstreams words; workspace: DEVICE, 256-byte
 * aligned, >= pgdvs_png_inflate_workspace_bytes(table, nstreams) (-1 for a table it refuses).  Two launches on `stream`, no
 * host synchronisation.  status[i] is 0 only if stream i inflated to exactly its inflated size, the bytes
 * behind its final block were exactly the four of the Adler-32 of those bytes, and every row's filter byte was 0 .. 4; else
 * PGDVS_PNG_* bits say what was met (_BLOCK: block type 3, a length set that is over-subscribed or incomplete as zlib judges
 * it, a bad repeat, no end-of-block code; _CODE: a code the table lacks, length symbols 286 / 287, distance symbols 30 / 31;
 * _DISTANCE: a distance in front of the output; _STORED: LEN / NLEN disagree; _DATA_OUT: the data ran out; _SIZE: more or
 * fewer bytes than the image's; _LEFT_OVER; _ADLER; _FILTER; _NOT_SYNCHRONISED: never set by construction) and out[i] holds
 * no result: the caller hands the file to a host reader, which decides.  Whatever the streams' bytes hold, nothing outside
 * the batch buffer is read and nothing outside the images' rows, status and the workspace is written.
 * The workspace's first words, for tools, four per stream: windows, the most synchronisation rounds of a window, the most
 * resolve rounds of a window, blocks.
 * pgdvs_png_decode_host: the same walk on the CPU, HOST pointers throughout (batch_host and batch may be the same buffer;
 * 8-byte alignment suffices): the same core, windows, rounds and workspace.  0, or -1 for argument errors. */
#define PGDVS_PNG_INFLATE_SUB_BYTES 64
#define PGDVS_PNG_INFLATE_MAX_BYTES (1 << 28)
#define PGDVS_PNG_BLOCK 1
#define PGDVS_PNG_CODE 2
#define PGDVS_PNG_DISTANCE 4
#define PGDVS_PNG_STORED 8
#define PGDVS_PNG_DATA_OUT 16
#define PGDVS_PNG_SIZE 32
#define PGDVS_PNG_LEFT_OVER 64
#define PGDVS_PNG_ADLER 128
#define PGDVS_PNG_FILTER 256
#define PGDVS_PNG_NOT_SYNCHRONISED 512
typedef struct pgdvs_png_image {
  int64_t offset, size;
  int32_t height, width, channels, out_channels;
  int64_t row_stride;
  void *out;
  int32_t bit_depth, scale;
} pgdvs_png_image;
int64_t pgdvs_png_inflate_workspace_bytes(const pgdvs_png_image *streams, int32_t nstreams);
int pgdvs_png_decode(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t nstreams, int32_t sub_bytes, uint32_t *status,
                     void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream);
int pgdvs_png_decode_host(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t nstreams, int32_t sub_bytes,
                          uint32_t *status, void *workspace, int64_t workspace_bytes);

/* A decoded mask into its place (csrc/mask_place.hip): one gather over src uint8 [h,w,C] on the DEVICE, src_row_stride bytes
 * between its rows (>= w * C), pixels contiguous.  map: nullptr (then H = h and W = w: pixel (y, x) comes from (y, x)), or
 * DEVICE int32 [H,W], the source pixel's index y' * w + x' of every output pixel (a NEAREST resize's picks); an index outside
 * 0 .. h * w - 1 reads as 0.
 *   mode PGDVS_MASK_PLACE_U8      C = 1: out uint8 [H,W], out_row_stride bytes between rows (>= W): the picked byte
 *   mode PGDVS_MASK_PLACE_BGR_F32 C = 1 or 3: out float32 [H,W,3], out_row_stride BYTES between rows (>= 12 W, a multiple
 *                                 of 4): out[y,x,k] = src[..., C - 1 - k] > 0 ? 1 : 0 (C = 1: the one channel thrice) --
 *                                 float32(convert("RGB")[..., ::-1] > 1e-3) of a grey or RGB mask file
 * h, w, H, W: 1 .. 16384.  One launch on `stream`, no workspace, no atomics, no host synchronisation. */
#define PGDVS_MASK_PLACE_U8 0
#define PGDVS_MASK_PLACE_BGR_F32 1
int pgdvs_mask_place(const uint8_t *src, int32_t h, int32_t w, int32_t channels, int64_t src_row_stride, const int32_t *map, int32_t H, int32_t W,
                     int32_t mode, void *out, int64_t out_row_stride, pgdvs_stream_t stream);

/* The float32 payloads of a batch of depth files into their places (csrc/depth_place.hip): what the loaders'
 * numpy statements make of a `.npy` / stored `.npz` payload, bit for bit, written straight into the frames' slots of the
 * resident store.  The batch buffer, as pgdvs_png_decode's: a table of n pgdvs_depth_entry, padded to 16 bytes, then the
 * payloads as the files store them (little-endian float32 [h,w], C order), each at its entry's `offset` from the buffer's
 * start, a multiple of 4 (a caller that stages payloads at multiples of 16 gets 16-byte loads).  Per entry:
 *   h, w            the source's size; H, W: the output's; each 1 .. 16384
 *   op              PGDVS_DEPTH_COPY out = x;  PGDVS_DEPTH_RECIPROCAL out = 1.0f / (x + 1e-8f), NumPy 2's `1 / (disp + 1e-8)` on
 *                   a float32 array;  PGDVS_DEPTH_SCALE out = x * scale.  Each add, multiply and divide is one correctly
 *                   rounded float32 operation; denormals are kept; NaN, +-inf and -0 propagate as IEEE 754 has it.
 *   map             nullptr (then H = h and W = w), or DEVICE int32 [H,W]: the source index y' * w + x' of every output pixel
 *                   (a NEAREST resize's picks, as pgdvs_mask_place takes them); an index outside 0 .. h * w - 1 reads x = 0
 *   out             DEVICE float32 [H,W], 4-byte aligned, out_row_stride BYTES between rows (>= 4 W, a multiple of 4)
 * batch_host: HOST, the buffer as filled (only its table is read, and checked: sizes, ops, strides, and that every payload
 * lies behind the table and inside batch_bytes); batch: DEVICE, a copy of the same batch_bytes bytes, 16-byte aligned.
 * One launch on `stream`; no workspace, no atomics, no host synchronisation, no status: nothing can fail on the device.
 * Nothing outside the entries' rows is written.  0, or PGDVS_ERR_INVALID (nothing is launched). */
#define PGDVS_DEPTH_COPY 0
#define PGDVS_DEPTH_RECIPROCAL 1
#define PGDVS_DEPTH_SCALE 2
#define PGDVS_DEPTH_MAX_ENTRIES 4096
typedef struct pgdvs_depth_entry {
  int64_t offset;
  int32_t h, w;
  int32_t op;
  float scale;
  const int32_t *map;
  void *out;
  int64_t out_row_stride;
  int32_t H, W;
} pgdvs_depth_entry;
int pgdvs_depth_place(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t n, pgdvs_stream_t stream);

/* np.percentile(values, q) of the installed NumPy 2 (method "linear") over float32 values, per frame of a batch, bit for
 * bit (csrc/depth_range.hip, over radix_select.h as the depth-range ops): q / 100 is formed in float32, the virtual index is
 * (n - 1) q in float32, its two neighbouring ranks are selected exactly and joined by NumPy's _lerp in float32.  Any NaN
 * among a frame's values gives NaN.  (-0.0 and +0.0 compare equal; a zero comes back as +0.0.)
 * values: HOST array of nframes DEVICE pointers, 4-byte aligned; counts: HOST, each 1 .. 2^31 - 1; q_percent in [0, 100];
 * out: DEVICE float32 [nframes]; workspace >= pgdvs_percentile_f32_workspace_bytes(counts, nframes), 256-byte aligned.
 * Launches on `stream` alone, no host synchronisation. */
int64_t pgdvs_percentile_f32_workspace_bytes(const int64_t *counts, int32_t nframes);
int pgdvs_percentile_f32(const float *const *values, const int64_t *counts, int32_t nframes, double q_percent, float *out, void *workspace,
                         int64_t workspace_bytes, pgdvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PGDVS_HIP_H_ */
