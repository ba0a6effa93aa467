#!/usr/bin/env python3
"""Edge fixtures of the dynamic branch, made by RUNNING THE REFERENCE ITSELF.

The fixtures of make_golden.py draw every flow as ``normal * 1.5 + (2.3, -1.2)``, every time stamp as
(3, 4, 3.4) and every depth strictly positive, so the branch's integer decisions are almost never met
there.  This generator runs the same reference functions on constructed inputs that do meet them, and
writes ``dyn_edges_*.npz`` next to this script.  Like make_golden.py it runs only in the build container,
where the upstream tree is mounted read-only, and imports the reference's modules under the
``sys.modules`` stubs of make_golden.py (it imports ``_install_stubs``, ``_cpu_splat``, ``_flat_cam`` and
``_pose`` from there).  The fixtures are data only: tests/test_oracle_dyn_edges.py replays them against
oracle/ (CPU) and tests/test_gpu_dyn_edges.py against the HIP path.

What the stubs stand in for (and therefore what is NOT pinned by these vectors), as in make_golden.py:
  * pytorch3d.ops.knn_points -> exact brute-force kNN on squared L2 (pytorch3d's contract; only the
    order among equal distances is unpinned -- it does not change a mean).
  * pgdvs.utils.softsplat.softsplat_func (cupy / CUDA only) -> a vectorised torch scatter written from
    the kernel text softsplat.py:352-402.  The torch pre/post-processing of softsplat() runs unmodified.

Which ``grid_sample`` the fixtures pin.  The reference ran on CUDA; here torch runs on the CPU.  The warp
samples depth_2 with ``grid_sample(mode="nearest", align_corners=False)`` (pgdvs_renderer_dyn.py:342-348),
whose source index the two backends compute differently:
  * CPU (vectorised GridSamplerKernel):  ix = (g + 1) * (W / 2) - 0.5, then round half to even;
  * CUDA (GridSampler.cuh):               ix = ((g + 1) * W - 1) / 2, then nearbyint (half to even),
    where nvcc may fuse ``(g + 1) * W - 1`` into one FMA ("fma") or not ("seq").
At an integer flow, ix lands on or one ulp beside a .5 tie, so the flavours could pick different
pixels of depth_2.  They are not settled with a tolerance: while the reference runs, every nearest
sample is checked against all three flavours (``_checked_grid_sample``), and the generator stops if
any of them picks another pixel than the CPU did.  So each integer output here is the one the CUDA
reference gives whichever way it was compiled; the HIP kernel and the oracle implement "seq".
The bilinear samples (the frame-2 colours, the backwarp of the softsplat metric) differ between the
backends only in float rounding and are compared with the existing float tolerances.

Cases (odd, non-square sizes; every dyn_pcl item holds the inputs of compute_dyn_pcl, its render
settings and its outputs under ``<item>__<key>``, where an item after the first omits the arrays
equal to the first item's; ``fwd__*`` is a batch-1 PGDVSRenderer.forward through
the ``rgb_gnt`` shortcut on the case's first item, with the ``randn_like`` draw recorded as in
make_golden.py's _forward_case).  The forward records replace the item's colours with slowly varying ones,
equal in both frames.  With random colours the softsplat metric (alpha = 100) drives exp(-100 L1) towards
1e-15; where a pixel's splat normaliser falls below the 1e-7 epsilon of softsplat's "soft" mode its colour
is proportional to the bilinear weights, and the ~1e-5 px by which two float projections of the same point
differ (CPU and CUDA torch, or the kernels) then moves it by more than the 1e-4 image tolerance.  That is
the conditioning of the reference's arithmetic, not an edge of the kernels, so these records keep away from
it: the generator checks each record's conditioning (``_conditioned_forward``) and, where a pixel fails,
moves the target's principal point by a hundredth of a pixel.  (In the depth case the target's rows
coincide with frame 1's, so every splat lands within an ulp of a pixel row: the record's target is moved.
Exact 0 / 1 corner weights are pinned by the standalone softsplat fixture, whose flows are given.)  The cases:
  dyn_edges_integer   37 x 61.  Every flow an integer in [-3, 3], zero included; a dynamic mask that
                      touches all four borders, so some pixels land on u = 0, u = W-1, v = 0, v = H-1.
                      Nearest-sample ties everywhere.  Outlier removal off and on; forward.
  dyn_edges_half      37 x 61.  Flows at k + 0.5 and one ulp either side; dynamic pixels with +-0.0,
                      NaN and +-inf flow components.  Outlier removal off and on.
  dyn_edges_bounds    37 x 61.  Flows that put uv exactly on 0, W-1 and H-1 and one ulp beyond each
                      (beyond 0: the smallest subnormal and one ulp of the flow); flow consistency on
                      with occluded pixels inside the mask; forward.
  dyn_edges_time      37 x 61.  tt == t1, tt == t2, tt < t1 and tt > t2 (w1 < 0 or w2 < 0), with the
                      same inputs otherwise.
  dyn_edges_depth     37 x 61.  Frame 1 and the target are pure translations with dyadic values, so
                      points with depth_1 == 0 lie exactly on the target's z = 0 plane and points with
                      depth_1 < 0 behind it: the z clamp (1e-8) and the +-1e6 pixel clamp of
                      projector.py:64-68, i.e. +-1e6 target flows that the splat must drop.  Zeros of
                      depth_2 at nearest-sampled positions.  Same time, tt == t1 and tt = 3.4; forward.
  dyn_edges_large     67 x 71 (more than 4096 valid pixels: the compaction crosses a tile).  Random
                      flows, about 30 % of them integer, outlier removal on; forward with smooth
                      colours (random colours would not fit the size limit of a committed file).
  dyn_edges_ops       standalone ops.  project: points at z = 0, +-tiny, negative and huge, and points
                      exactly on pixel centres (dyadic camera: the products are exact on every backend),
                      plus a general camera.  backwarp_l1: integer flows and flows onto and one pixel
                      past the borders.  softsplat: integer flows, flows onto the last row and column,
                      every mode.

Two runs write byte-identical files (fixed seeds, one torch thread, fixed zip timestamps).

Usage:  python tests/golden/make_golden_dyn_edges.py
"""
import io
import pathlib
import sys
import types
import zipfile

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_golden import OUT, _cpu_splat, _flat_cam, _install_stubs, _pose  # noqa: E402

F32 = np.float32
KNN, STD_THRES, ALPHA = 8, 0.1, 100.0
T = torch.from_numpy


def _save(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that two runs give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


# ---------------------------------------------------------------- the nearest-sample flavour check
_real_grid_sample = torch.nn.functional.grid_sample
_nearest_checked = [0]


def _checked_grid_sample(input, grid, mode="bilinear", padding_mode="zeros", align_corners=None):
    out = _real_grid_sample(input, grid, mode=mode, padding_mode=padding_mode, align_corners=align_corners)
    if mode == "nearest":
        assert padding_mode == "zeros" and not align_corners
        H, W = input.shape[-2:]
        lab = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)  # 0 = zero padding
        cpu = _real_grid_sample(lab, grid[:1], mode="nearest", padding_mode="zeros", align_corners=False).reshape(-1)
        g = grid[:1].reshape(-1, 2)
        for flavour in ("seq", "fma"):
            n = []
            for c, size in ((0, W), (1, H)):
                if flavour == "seq":
                    i = ((g[:, c] + 1.0) * float(size) - 1.0) / 2.0
                else:  # one rounding for (g + 1) * size - 1: exact in float64, then rounded once
                    i = (((g[:, c] + 1.0).double() * float(size) - 1.0).float()) / 2.0
                n.append(torch.round(i))  # round half to even == nearbyint
            nx, ny = n
            ok = (nx >= 0) & (nx <= W - 1) & (ny >= 0) & (ny <= H - 1)
            cuda = torch.where(ok, ny * W + nx + 1, torch.zeros_like(nx))
            bad = int((cuda != cpu).sum())
            if bad:
                raise RuntimeError(f"nearest grid_sample: CUDA ({flavour}) and CPU pick different pixels at {bad} positions")
        _nearest_checked[0] += g.shape[0]
    return out


# ---------------------------------------------------------------- scenes
def _depth(H, W, ph):
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    return (2.0 + 0.5 * np.sin(xx / W * 3 + ph) + 0.3 * np.cos(yy / H * 2 + ph)).astype(F32)


def _border_mask(H, W):
    """a blob plus stripes along (and one or two pixels inside) all four borders"""
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    m = ((xx - W * 0.45) ** 2 + (yy - H * 0.5) ** 2) < (0.3 * min(H, W)) ** 2
    m[0:2, 5:25] = True
    m[H - 2:H, W - 30:W - 8] = True
    m[4:20, 0:3] = True
    m[12:30, W - 3:W] = True
    m[1, 1] = True  # isolated pixel -> an outlier
    return m.astype(F32)


def _smooth_rgb(H, W, ph, amp=0.4, freq=1.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    return np.stack([0.5 + amp * np.sin(freq * (xx / W * (3 + k) + yy / H * (2 - k)) + ph + k) for k in range(3)], -1).astype(F32)


def _scene(rng, H, W, *, times=(3.0, 4.0, 3.4), smooth=False, cams=None):
    f = 0.9 * W
    if cams is None:
        cams = (_flat_cam(H, W, f, _pose(1.5, -0.5, [0.00, 0.01, 0.0])),
                _flat_cam(H, W, f * 1.02, _pose(-2.0, 0.7, [0.05, 0.00, 0.01]), cx=W / 2 + 0.7, cy=H / 2 - 0.4),
                _flat_cam(H, W, f * 0.98, _pose(0.4, 0.3, [0.02, -0.01, -0.02])))
    rgb = np.stack([_smooth_rgb(H, W, 0.0), _smooth_rgb(H, W, 0.3)]) if smooth else rng.random((2, H, W, 3), dtype=F32)
    return dict(
        dyn_mask_1=_border_mask(H, W)[..., None], rgb_1=rgb[0], rgb_2=rgb[1], depth_1=_depth(H, W, 0.0)[..., None],
        depth_2=_depth(H, W, 0.4)[..., None], flow_12=np.zeros((H, W, 2), F32),
        flow_12_occ_mask=(rng.random((H, W, 1)) < 0.1).astype(F32), flat_cam_1=cams[0], flat_cam_2=cams[1],
        flat_cam_tgt=cams[2], time_1=F32(times[0]), time_2=F32(times[1]), time_tgt=F32(times[2]))


def _fwd_inputs(inp, ph=0.0):
    """the inputs of a forward record: the item's, with slowly varying colours equal in both frames (a pixel moved
    by one still changes colour by ~4e-3, forty times the image tolerance)"""
    H, W = inp["dyn_mask_1"].shape[:2]
    c = _smooth_rgb(H, W, ph, amp=0.3, freq=0.5)
    return dict(inp, rgb_1=c, rgb_2=c.copy())


def _trans_cam(H, W, f, cx, cy, t):
    """identity rotation, dyadic translation / intrinsics: its inverse and projection are exact in fp32"""
    c2w = np.eye(4)
    c2w[:3, 3] = t
    return _flat_cam(H, W, f, c2w, cx=cx, cy=cy)


def _int_flows(rng, H, W):
    return rng.integers(-3, 4, (H, W, 2)).astype(F32)


# ---------------------------------------------------------------- reference calls
class Ref:
    def __init__(self):
        import pgdvs.models.gnt.projector as PJ
        import pgdvs.renderers.pgdvs_renderer as RR
        import pgdvs.renderers.pgdvs_renderer_base as RB
        import pgdvs.renderers.pgdvs_renderer_dyn as RD
        import pgdvs.utils.softsplat as SS
        from pgdvs.models.gnt.renderer import BaseRenderer as GNTRenderer

        SS.softsplat_func = types.SimpleNamespace(apply=_cpu_splat)
        self.SS, self.RR, self.GNTRenderer = SS, RR, GNTRenderer
        self.proj = PJ.Projector()
        self.cfg_ns = types.SimpleNamespace(rgb_range="0_1", tracker=None)
        self.base = RB.PGDVSBaseRenderer()
        self.RD = RD
        self.dyn = RD.PGDVSDynamicRenderer(cfg=self.cfg_ns, softsplat_metric_abs_alpha=ALPHA,
                                           proj_func=self.proj.compute_projections)

    def dyn_pcl(self, inp, use_fc, rm):
        H, W = inp["dyn_mask_1"].shape[:2]
        rc = types.SimpleNamespace(dyn_render_use_flow_consistency=use_fc, dyn_pcl_remove_outlier=rm,
                                   dyn_pcl_outlier_knn=KNN, dyn_pcl_outlier_std_thres=STD_THRES,
                                   dyn_render_type="softsplat")
        fc1, fc2 = T(inp["flat_cam_1"]), T(inp["flat_cam_2"])
        ro, rd, uvs, _, _ = self.dyn.get_batched_rays(device="cpu", batch_size=1, H=H, W=W, render_stride=1,
                                                      intrinsics=fc1[2:18].reshape(1, 4, 4), c2w=fc1[18:34].reshape(1, 4, 4))
        flow, valid, info = self.dyn.compute_dyn_pcl(
            dyn_mask_1=T(inp["dyn_mask_1"]), rgb_1=T(inp["rgb_1"]), uvs_1=uvs, ray_o_1=ro, ray_d_1=rd,
            depth_1=T(inp["depth_1"]), flow_12=T(inp["flow_12"]), flow_12_occ_mask=T(inp["flow_12_occ_mask"]),
            rgb_2=T(inp["rgb_2"]), depth_2=T(inp["depth_2"]), K_2=fc2[2:18].reshape(4, 4), c2w_2=fc2[18:34].reshape(4, 4),
            flat_cam_tgt=T(inp["flat_cam_tgt"]), time_1=torch.tensor(inp["time_1"]), time_2=torch.tensor(inp["time_2"]),
            time_tgt=torch.tensor(inp["time_tgt"]), render_cfg=rc)
        return dict(**inp, use_flow_consistency=use_fc, remove_outlier=rm, outlier_knn=KNN, outlier_std_thres=STD_THRES,
                    out_flow_1_to_tgt=flow.numpy(), out_valid_dyn_mask_1=valid.numpy(), out_pcl=info["pcl"].numpy(),
                    out_pcl_rgbs=info["pcl_rgbs"].numpy(), out_nn_dist_thres=info["pcl_nn_dist_thres"].numpy())

    def forward(self, inp, use_fc, rm, rgb_gnt, seed):
        """batch-1 PGDVSRenderer.forward through the rgb_gnt shortcut (as make_golden.py's _forward_case)"""
        H, W = inp["dyn_mask_1"].shape[:2]
        data = {
            "rgb_src_temporal": np.stack([inp["rgb_1"], inp["rgb_2"]])[None],
            "depth_src_temporal": np.stack([inp["depth_1"], inp["depth_2"]])[None],
            "dyn_mask_src_temporal": np.stack([inp["dyn_mask_1"], inp["dyn_mask_1"]])[None],
            "flow_fwd": inp["flow_12"][None], "flow_fwd_occ_mask": inp["flow_12_occ_mask"][None],
            "flat_cam_tgt": inp["flat_cam_tgt"][None],
            "flat_cam_src_temporal": np.stack([inp["flat_cam_1"], inp["flat_cam_2"]])[None],
            "time_tgt": np.array([[inp["time_tgt"]]], F32),
            "time_src_temporal": np.array([[inp["time_1"], inp["time_2"]]], F32),
            "rgb_gnt": rgb_gnt[None].astype(F32),
        }
        rc = types.SimpleNamespace(
            render_stride=1, pure_gnt=False, pure_gnt_with_dyn_mask=False, gnt_use_dyn_mask=False,
            gnt_use_masked_spatial_src=False, dyn_render_use_flow_consistency=use_fc, dyn_pcl_remove_outlier=rm,
            dyn_pcl_outlier_knn=KNN, dyn_pcl_outlier_std_thres=STD_THRES, dyn_render_type="softsplat",
            dyn_render_track_temporal="none")
        model = self.RR.PGDVSRenderer.__new__(self.RR.PGDVSRenderer)
        torch.nn.Module.__init__(model)
        model.cfg = self.cfg_ns
        model.flag_debug = False
        st = self.GNTRenderer.__new__(self.GNTRenderer)
        torch.nn.Module.__init__(st)
        st.projector = self.proj
        model.static_renderer = st
        model.softsplat_metric_abs_alpha = ALPHA
        model.dyn_renderer = self.RD.PGDVSDynamicRenderer(cfg=self.cfg_ns, softsplat_metric_abs_alpha=ALPHA,
                                                          proj_func=self.proj.compute_projections)
        tdata = {k: T(np.ascontiguousarray(v)) for k, v in data.items()}
        tdata["depth_range"] = torch.tensor([[0.5, 5.0]])
        tdata["rgb_src_spatial"] = tdata["rgb_src_temporal"]
        tdata["dyn_mask_src_spatial"] = tdata["dyn_mask_src_temporal"]
        tdata["flat_cam_src_spatial"] = tdata["flat_cam_src_temporal"]
        # record the actual draw of torch.randn_like(rgb_src_1) (pgdvs_renderer_dyn.py:181)
        torch.manual_seed(seed)
        drawn = []
        real_randn_like = torch.randn_like

        def _recording_randn_like(t, *a, **k):
            r = real_randn_like(t, *a, **k)
            drawn.append(r.clone())
            return r

        torch.randn_like = _recording_randn_like
        try:
            with torch.no_grad():
                ret = model.forward(tdata, render_cfg=rc, disable_tqdm=True)
        finally:
            torch.randn_like = real_randn_like
        assert len(drawn) == 1 and tuple(drawn[0].shape) == (1, 3, H, W)
        out = {"in_" + k: v for k, v in data.items()}
        out.update(static_noise=drawn[0].contiguous().numpy(), remove_outlier=rm, use_flow_consistency=use_fc,
                   outlier_knn=KNN, outlier_std_thres=STD_THRES, render_stride=1)
        out.update({"out_" + k: v.numpy() for k, v in ret.items() if torch.is_tensor(v)})
        return out


def _shift_centre(flat_cam, d):
    fc = flat_cam.copy()
    fc[2 + 2] += F32(d)  # K[0, 2]
    fc[2 + 6] += F32(d)  # K[1, 2]
    return fc


def _conditioned_forward(ref, inp, use_fc, rm, rgb_gnt, seed):
    """a forward record whose outputs do not hang on the last bits of the projection: moving every target pixel
    by +-2e-5 px (the target camera's principal point) changes no mask pixel and no colour by more than 2e-5.
    Where that does not hold, the target's principal point is moved by 0.013 px and the check repeated."""
    for k in range(16):
        fi = dict(inp, flat_cam_tgt=_shift_centre(inp["flat_cam_tgt"], 0.013 * k))
        rec = ref.forward(fi, use_fc, rm, rgb_gnt, seed)
        stable = True
        for d in (2e-5, -2e-5):
            alt = ref.forward(dict(fi, flat_cam_tgt=_shift_centre(fi["flat_cam_tgt"], d)), use_fc, rm, rgb_gnt, seed)
            stable &= np.array_equal(alt["out_render_dyn_mask"], rec["out_render_dyn_mask"])
            stable &= float(np.abs(alt["out_render_dyn_rgb"] - rec["out_render_dyn_rgb"]).max()) <= 2e-5
        if stable:
            return rec
    raise RuntimeError("no well-conditioned forward record")


def _write_case(name, items, fwd=None):
    """an item stores only the arrays that differ from the first item's (the tests merge them back)"""
    arrays = {"items": np.array(list(items))}
    first = next(iter(items.values()))
    for j, (item, d) in enumerate(items.items()):
        arrays.update({f"{item}__{k}": v for k, v in d.items()
                       if j == 0 or not (np.asarray(v).dtype == np.asarray(first[k]).dtype
                                         and np.array_equal(v, first[k], equal_nan=np.asarray(v).dtype.kind == "f"))})
    if fwd is not None:
        arrays.update({f"fwd__{k}": v for k, v in fwd.items()})
    _save(OUT / f"{name}.npz", arrays)


def _lands(inp, item):
    """which borders the valid flows of an item reach exactly (a check that the case does what it claims)"""
    H, W = inp["dyn_mask_1"].shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    ux, uy = xx + inp["flow_12"][..., 0], yy + inp["flow_12"][..., 1]
    m = inp["dyn_mask_1"][..., 0] != 0
    hit = {"u=0": np.any(m & (ux == 0)), "u=W-1": np.any(m & (ux == W - 1)),
           "v=0": np.any(m & (uy == 0)), "v=H-1": np.any(m & (uy == H - 1))}
    assert all(hit.values()), (item, hit)


# ---------------------------------------------------------------- cases
def case_integer(ref):
    rng = np.random.default_rng(101)
    H, W = 37, 61
    inp = _scene(rng, H, W)
    inp["flow_12"] = _int_flows(rng, H, W)
    _lands(inp, "integer")
    items = {"rm0": ref.dyn_pcl(inp, False, False), "rm1": ref.dyn_pcl(inp, False, True)}
    fwd = _conditioned_forward(ref, _fwd_inputs(inp), False, True, rng.random((H, W, 3), dtype=F32), seed=11)
    _write_case("dyn_edges_integer", items, fwd)


def case_half(ref):
    rng = np.random.default_rng(202)
    H, W = 37, 61
    inp = _scene(rng, H, W)
    fl = rng.integers(-3, 3, (H, W, 2)).astype(F32) + F32(0.5)
    side = rng.integers(0, 3, (H, W, 2))
    fl = np.where(side == 1, np.nextafter(fl, F32(np.inf)), np.where(side == 2, np.nextafter(fl, F32(-np.inf)), fl))
    ys, xs = np.nonzero(inp["dyn_mask_1"][..., 0])
    pick = rng.choice(ys.size, 16, replace=False)
    specials = [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (np.nan, 0.5), (0.5, np.nan), (np.nan, np.nan), (np.inf, 0.0),
                (-np.inf, 0.0), (0.0, np.inf), (0.0, -np.inf), (np.inf, -np.inf), (np.nan, np.inf), (-0.0, 1.0),
                (1.0, -0.0), (-np.inf, np.nan), (0.0, 0.0)]
    for (a, b), i in zip(specials, pick):
        fl[ys[i], xs[i]] = (a, b)
    inp["flow_12"] = fl.astype(F32)
    items = {"rm0": ref.dyn_pcl(inp, False, False), "rm1": ref.dyn_pcl(inp, False, True)}
    _write_case("dyn_edges_half", items)


def case_bounds(ref):
    rng = np.random.default_rng(303)
    H, W = 37, 61
    inp = _scene(rng, H, W)
    fl = (rng.normal(size=(H, W, 2)) * 1.5).astype(F32)
    m = inp["dyn_mask_1"][..., 0] != 0
    up, dn = lambda x: np.nextafter(F32(x), F32(np.inf)), lambda x: np.nextafter(F32(x), F32(-np.inf))
    tiny = np.nextafter(F32(0), F32(1))  # smallest subnormal
    # x: targets on and one ulp beyond 0 and W-1; (column, flow_x) pairs, each over several masked rows
    xt = [(0, F32(0)), (0, -tiny), (0, F32(-0.0)), (1, F32(-1)), (1, dn(-1)), (2, F32(-2)), (2, dn(-2)),
          (W - 1, F32(0)), (W - 1, tiny), (W - 2, F32(1)), (W - 2, up(1)), (W - 3, F32(2)), (W - 3, up(2)),
          (0, F32(W - 1)), (0, up(W - 1)), (1, F32(W - 2)), (1, up(W - 2))]
    yt = [(0, F32(0)), (0, -tiny), (1, F32(-1)), (1, dn(-1)), (H - 1, F32(0)), (H - 1, tiny), (H - 2, F32(1)),
          (H - 2, up(1)), (0, F32(H - 1)), (0, up(H - 1)), (1, F32(H - 2)), (1, up(H - 2))]
    # several targets share a border column / row: they take its masked pixels in turn
    for c in sorted({c for c, _ in xt}):
        fs = [f for cc, f in xt if cc == c]
        rows = np.nonzero(m[:, c])[0]
        for i, f in enumerate(fs):
            for r in rows[i::len(fs)]:
                fl[r, c, 0] = f
                fl[r, c, 1] = F32(rng.integers(-1, 2))
    for r in sorted({r for r, _ in yt}):
        fs = [f for rr, f in yt if rr == r]
        cols = np.nonzero(m[r, :])[0]
        for i, f in enumerate(fs):
            for c in cols[i::len(fs)]:
                fl[r, c, 1] = f
    inp["flow_12"] = fl
    inp["flow_12_occ_mask"][m & (rng.random((H, W)) < 0.15)] = 1.0  # occluded pixels inside the mask
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    ux, uy = xx + fl[..., 0], yy + fl[..., 1]
    assert np.any(m & (ux == up(W - 1))) and np.any(m & (ux < 0) & (ux > -1e-30)) and np.any(m & (uy == up(H - 1)))
    _lands(inp, "bounds")
    items = {"fc1_rm0": ref.dyn_pcl(inp, True, False), "fc1_rm1": ref.dyn_pcl(inp, True, True),
             "fc0_rm0": ref.dyn_pcl(inp, False, False)}
    fwd = _conditioned_forward(ref, _fwd_inputs(inp), True, False, rng.random((H, W, 3), dtype=F32), seed=13)
    _write_case("dyn_edges_bounds", items, fwd)


def case_time(ref):
    rng = np.random.default_rng(404)
    H, W = 37, 61
    base = _scene(rng, H, W)
    fl = (rng.normal(size=(H, W, 2)) * 1.5).astype(F32)
    isint = rng.random((H, W, 1)) < 0.5
    base["flow_12"] = np.where(isint, np.round(fl), fl).astype(F32)
    items = {}
    for name, tt, rm in (("tt_eq_t1", 3.0, False), ("tt_eq_t2", 4.0, True), ("tt_lt_t1", 2.3, False), ("tt_gt_t2", 4.6, True)):
        inp = dict(base, time_tgt=F32(tt))
        items[name] = ref.dyn_pcl(inp, False, rm)
    _write_case("dyn_edges_time", items)


def case_depth(ref):
    rng = np.random.default_rng(505)
    H, W = 37, 61
    # frame 1 and the target: identity rotation, dyadic translation and intrinsics (f = 64, centre 30.5 / 18.5):
    # the target sits at frame 1's z, so a point with depth_1 == 0 (= frame 1's centre) is on its z = 0 plane
    cam1 = _trans_cam(H, W, 64.0, 30.5, 18.5, [0.25, -0.5, 0.125])
    camt = _trans_cam(H, W, 64.0, 30.5, 18.5, [0.75, -0.5, 0.125])
    cam2 = _flat_cam(H, W, 0.9 * W * 1.02, _pose(-2.0, 0.7, [0.05, 0.00, 0.01]), cx=W / 2 + 0.7, cy=H / 2 - 0.4)
    base = _scene(rng, H, W, cams=(cam1, cam2, camt))
    fl = (rng.normal(size=(H, W, 2)) * 1.5).astype(F32)
    base["flow_12"] = np.where(rng.random((H, W, 1)) < 0.5, np.round(fl), fl).astype(F32)
    m = base["dyn_mask_1"][..., 0] != 0
    d1 = base["depth_1"][..., 0].copy()
    u = rng.random((H, W))
    d1[m & (u < 0.10)] = 0.0                                         # on the target's z = 0 plane
    d1[m & (u >= 0.10) & (u < 0.16)] = -rng.uniform(0.2, 2.0, (H, W))[m & (u >= 0.10) & (u < 0.16)]  # behind it
    d1[m & (u >= 0.16) & (u < 0.19)] = F32(1e-9)                     # rounds onto the plane
    base["depth_1"] = d1[..., None]
    # zeros of depth_2 where flows of masked pixels sample it (nearest of uv2 - 0.5 and its neighbours)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    ux, uy = xx + base["flow_12"][..., 0], yy + base["flow_12"][..., 1]
    d2 = base["depth_2"][..., 0].copy()
    sel = m & (u > 0.7) & (ux >= 0) & (ux <= W - 1) & (uy >= 0) & (uy <= H - 1)
    for y, x in zip(np.floor(uy[sel]).astype(int), np.floor(ux[sel]).astype(int)):
        d2[max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = 0.0
    base["depth_2"] = d2[..., None]
    items = {
        "tt_eq_t1": ref.dyn_pcl(dict(base, time_tgt=F32(3.0)), False, False),
        "same_time": ref.dyn_pcl(dict(base, time_2=F32(3.0), time_tgt=F32(3.0)), False, False),
        "tt_34": ref.dyn_pcl(base, False, False),
        "tt_34_rm1": ref.dyn_pcl(base, False, True),
    }
    f1t = items["tt_eq_t1"]["out_flow_1_to_tgt"]
    assert np.sum(np.abs(f1t[..., 0] + xx) == 1e6) > 20, "the +-1e6 clamp is not reached"
    fwd = _conditioned_forward(ref, _fwd_inputs(dict(base, time_tgt=F32(3.0))), False, False, rng.random((H, W, 3), dtype=F32), seed=17)
    _write_case("dyn_edges_depth", items, fwd)


def case_large(ref):
    rng = np.random.default_rng(606)
    H, W = 67, 71
    inp = _scene(rng, H, W, smooth=True)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    m = ~((((xx - 20) ** 2 + (yy - 50) ** 2) < 36) | (((xx - 55) ** 2 + (yy - 15) ** 2) < 25))
    m[33, 35] = True
    inp["dyn_mask_1"] = m.astype(F32)[..., None]
    fl = (rng.normal(size=(H, W, 2)) * 1.2 + np.array([0.4, -0.3])).astype(F32)
    inp["flow_12"] = np.where(rng.random((H, W, 1)) < 0.3, np.round(fl), fl).astype(F32)
    items = {"rm1": ref.dyn_pcl(inp, False, True)}
    ux, uy = xx + inp["flow_12"][..., 0], yy + inp["flow_12"][..., 1]
    assert np.sum(m & (ux >= 0) & (ux <= W - 1) & (uy >= 0) & (uy <= H - 1)) > 4096  # points before the outlier filter
    fwd = _conditioned_forward(ref, _fwd_inputs(inp), False, True, _smooth_rgb(H, W, 1.1), seed=19)
    _write_case("dyn_edges_large", items, fwd)


def case_ops(ref):
    rng = np.random.default_rng(707)
    out = {}
    # ---- A5 projection
    H, W = 37, 61
    cam = _trans_cam(H, W, 64.0, 30.5, 18.5, [0.25, -0.5, 0.0])  # z_cam = X[2] exactly
    pts = []
    for z in (0.0, -0.0, 1e-12, -1e-12, 1e-9, 1e-8, 2e-8, -1.0, -1e-3, 1e30, 3e37, 1e-30):
        for x, y in ((0.25, -0.5), (1.25, 0.5), (-3.0, 2.0), (0.25 + 1e-6, -0.5)):
            pts.append((x, y, z))
    for z in (2.0, 0.5, 8.0):  # exactly on pixel centres: X = t + (u - c) z / f, dyadic
        for uu, vv in ((0, 0), (W - 1, H - 1), (30, 18), (31, 19), (7, 33), (-2, 40), (W, -1)):
            pts.append((0.25 + (uu - 30.5) * z / 64.0, -0.5 + (vv - 18.5) * z / 64.0, z))
    xyz_a = np.array(pts, F32)
    cam_b = _flat_cam(30, 40, 35.0, _pose(5.0, 3.0, [0.2, 0.1, -0.3]))
    xyz_b = (rng.normal(size=(300, 3)) * np.array([1.0, 1.0, 2.0]) + np.array([0, 0, 1.2])).astype(F32)
    for tag, fc, xyz in (("a", cam, xyz_a), ("b", cam_b, xyz_b)):
        uv, msk = ref.proj.compute_projections(T(xyz[:, None, :]), T(fc[None]))
        out.update({f"project_{tag}_flat_cam": fc, f"project_{tag}_xyz": xyz, f"project_{tag}_uv": uv[0, :, 0].numpy(),
                    f"project_{tag}_mask": msk[0, :, 0].numpy()})
    assert np.all(np.abs(out["project_a_uv"][-21:] - np.round(out["project_a_uv"][-21:])) == 0)
    # ---- A6 backwarp + L1, integer flows and flows onto / one pixel past the borders
    rgb1 = rng.random((2, 3, H, W), dtype=F32)
    rgb2 = rng.random((2, 3, H, W), dtype=F32)
    flow = rng.integers(-3, 4, (2, 2, H, W)).astype(F32)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    sel = rng.random((H, W)) < 0.25
    flow[0, 0][sel] = np.where(rng.random((H, W)) < 0.5, -xx, W - 1 - xx)[sel]
    flow[0, 1][sel] = np.where(rng.random((H, W)) < 0.5, -yy, H - 1 - yy)[sel]
    sel = rng.random((H, W)) < 0.2
    flow[1, 0][sel] = np.where(rng.random((H, W)) < 0.5, -1 - xx, W - xx)[sel]
    flow[1, 1][sel] = np.where(rng.random((H, W)) < 0.5, -1 - yy, H - yy)[sel]
    warp = ref.base.backwarp_for_softsplat_metric(tenIn=T(rgb2), tenFlow=T(flow))
    l1 = torch.nn.functional.l1_loss(T(rgb1), warp, reduction="none").mean(dim=1, keepdim=True)
    out.update(backwarp_rgb1=rgb1, backwarp_rgb2=rgb2, backwarp_flow=flow, backwarp_l1=l1.numpy())
    # ---- A7 softsplat, integer flows and flows onto the last row / column, every mode
    ten_in = rng.random((2, 3, H, W), dtype=F32)
    ten_flow = rng.integers(-3, 4, (2, 2, H, W)).astype(F32)
    sel = rng.random((H, W)) < 0.3
    ten_flow[0, 0][sel] = (W - 1 - xx)[sel]
    ten_flow[0, 1][sel] = (H - 1 - yy)[sel]
    sel = rng.random((H, W)) < 0.2
    ten_flow[1, 0][sel] = (W - 1 - xx)[sel]
    ten_flow[1, 1][sel] = (H - 1 - yy)[sel] + np.where(rng.random((H, W)) < 0.5, 0, 1)[sel]  # last row, and one past it
    ten_metric = (rng.normal(size=(2, 1, H, W)) * 2.0).astype(F32)
    out.update(softsplat_ten_in=ten_in, softsplat_ten_flow=ten_flow, softsplat_ten_metric=ten_metric)
    for mode in ["sum", "avg", "linear", "soft", "soft-zeroeps", "soft-clipeps"]:
        mtr = None if mode in ("sum", "avg") else T(ten_metric if not mode.startswith("linear") else np.abs(ten_metric) + 0.1)
        out["softsplat_out_" + mode.replace("-", "_")] = ref.SS.softsplat(T(ten_in), T(ten_flow), mtr, mode).numpy()
    _save(OUT / "dyn_edges_ops.npz", out)


def main():
    torch.set_num_threads(1)
    _install_stubs()
    torch.nn.functional.grid_sample = _checked_grid_sample
    ref = Ref()
    for case in (case_integer, case_half, case_bounds, case_time, case_depth, case_large, case_ops):
        case(ref)
    print(f"nearest samples checked against both CUDA flavours: {_nearest_checked[0]}")
    total = 0
    for f in sorted(OUT.glob("dyn_edges_*.npz")):
        total += f.stat().st_size
        print(f"  {f.name:28s} {f.stat().st_size / 1024:8.1f} KiB")
    print(f"  {'total':28s} {total / 1024:8.1f} KiB")


if __name__ == "__main__":
    main()
