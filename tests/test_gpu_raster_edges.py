"""GPU (MI355X): csrc/raster.hip through ops.points_raster and PGDVSRenderer.forward on the cases of tests/raster_cases.py
-- NaN, +-inf, +-0, subnormal and near-FLT_MAX rows below the count; discs whose edge passes through a pixel centre at
the image corners, the tile borders and a partial tile's last row and column; radii one float32 step either side of the
kernel's switches; images of one pixel, one row, one column and strips up to 4 x 8192 -- against the oracle's naive loop
(which tests/test_raster_edges_host.py holds to the second statement of oracle/p3d_second.py without a GPU): idx equal,
zbuf, dist2 and mask bit for bit, rgb to 1e-6 and within the host test's float64 margin; both template instantiations of
the tile kernel, both output layouts, the depth bound forced on (with the second tile launch) and off (with the direct
binning pass where the image has 16 tiles), and the row bound at the count and one below it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import raster_cases as rc  # noqa: E402
from raster_cases import COMPOSITE_VS_F64_ATOL, F32, W_MIN_F64  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (checker only)
from pgdvs_amd import _lib, ops, synth  # noqa: E402

DEV = "cuda:0"
TAIL = 37  # rows of NaN behind the count in the capacity-sized buffers


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()  # fails loudly if the HIP extension is missing


def _oracle_fragments(c, n):
    """the oracle on the first n rows of a case"""
    if c.H * c.W * n > 5e7:
        return orc.rasterize_points_pointmajor(orc.points_to_ndc(c.pts[:n], c.cam, c.H, c.W), c.H, c.W, c.radius, c.K)
    return orc.rasterize_points(c.pts[:n], c.cam, c.H, c.W, c.radius, c.K)


def _check_fragments(r, idx, zbuf, d2, what):
    assert np.array_equal(N(r["idx"]), idx), what
    assert np.array_equal(_bits(N(r["zbuf"])), _bits(zbuf)), what
    assert np.array_equal(_bits(N(r["dist2"])), _bits(d2)), what


# ---------------------------------------------------------------- every case, every call
@pytest.mark.parametrize("name", rc.names())
def test_points_raster_case(name):
    c = rc.cases()[name]
    idx, zbuf, d2, img, mask = rc.oracle(name)
    n = c.pts.shape[0]
    pts, feat, cam = T(c.pts), T(c.feat), ops.cam_prep(T(c.cam))
    args = (pts, feat, cam, c.radius, c.K, c.H, c.W)
    runs = {}
    for density in (0.0, 1e9):  # 0: depth bound (where the radius and K allow one) and second tile launch; 1e9: neither
        with ops.option("raster_bound_density", density):
            runs[density] = (ops.points_raster(*args, want_fragments=True), ops.points_raster(*args, want_fragments=False),
                             ops.points_raster(*args, want_fragments=False, rgb_planar=True))
    a = runs[0.0][0]
    _check_fragments(a, idx, zbuf, d2, "fragments")
    assert np.array_equal(_bits(N(a["mask"])), _bits(mask))
    rgb = N(a["rgb"])
    np.testing.assert_allclose(rgb, img, rtol=0, atol=1e-6)
    hi, wmin = rc.composite_f64(idx, d2, c.radius, c.feat)
    ok = np.isfinite(wmin) & (wmin >= W_MIN_F64)
    assert np.abs(rgb.astype(np.float64) - hi)[ok].max(initial=0.0) <= COMPOSITE_VS_F64_ATOL
    for density, (frag, lean, planar) in runs.items():
        for k in ("idx", "zbuf", "dist2", "rgb", "mask"):
            assert torch.equal(frag[k], a[k]), (density, k)
        assert lean["idx"] is None and torch.equal(lean["rgb"], a["rgb"]) and torch.equal(lean["mask"], a["mask"]), density
        assert torch.equal(planar["rgb"], a["rgb"].permute(2, 0, 1)) and torch.equal(planar["mask"], a["mask"]), density
    # the row bound: the case's rows at the front of a capacity buffer whose tail is NaN, the count on the device
    cap_pts = torch.cat([pts, torch.full((TAIL, 3), float("nan"), device=DEV)])
    cap_feat = torch.cat([feat, torch.full((TAIL, 3), float("nan"), device=DEV)])
    cnt = torch.tensor([n], dtype=torch.int64, device=DEV)
    at = ops.points_raster(cap_pts, cap_feat, cam, c.radius, c.K, c.H, c.W, n_points_dev=cnt, want_fragments=True, row_bound=n)
    assert int(at["status"]) == 0
    for k in ("idx", "zbuf", "dist2", "rgb", "mask"):
        assert torch.equal(at[k], a[k]), k
    cut = ops.points_raster(cap_pts, cap_feat, cam, c.radius, c.K, c.H, c.W, n_points_dev=cnt, want_fragments=True, row_bound=n - 1)
    assert int(cut["status"]) == 1
    c_idx, c_z, c_d2 = _oracle_fragments(c, n - 1)
    _check_fragments(cut, c_idx, c_z, c_d2, "first n - 1 rows")
    np.testing.assert_allclose(N(cut["rgb"]), orc.composite(c_idx, c_d2, c.radius, c.feat), rtol=0, atol=1e-6)
    assert np.array_equal(N(cut["mask"]) > 0, (c_idx >= 0).any(-1))


# ---------------------------------------------------------------- degenerate rows
@pytest.mark.parametrize("tag", ["dyadic", "rotated"])
def test_undrawn_rows_behave_like_points_behind_the_camera(tag):
    """replacing every undrawn NaN / inf / zero-depth / far-outside row by a point behind the camera changes no output bit"""
    outs = []
    for name in (f"degen_{tag}", f"degen_{tag}_behind"):
        c = rc.cases()[name]
        per = []
        for density in (0.0, 1e9):
            with ops.option("raster_bound_density", density):
                per.append(ops.points_raster(T(c.pts), T(c.feat), ops.cam_prep(T(c.cam)), c.radius, c.K, c.H, c.W, want_fragments=True))
        outs.append(per)
    assert len(rc.cases()[f"degen_{tag}_behind"].claims["replaced"]) >= 10
    for a, b in zip(*outs):
        for k in ("idx", "zbuf", "dist2", "rgb", "mask"):
            assert torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a["rgb"]).all()) and bool(torch.isfinite(a["zbuf"]).all()) and bool(torch.isfinite(a["dist2"]).all())


def _view_forward(c):
    """a case's cloud as data["st_pcl_rgb"] through PGDVSRenderer.forward (the native view call) with the case's camera,
    radius and K -> (ret, the view's counters)"""
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    cfg = load_config(static_renderer="geo")
    cfg_rc = cfg.engine.engine_cfg.render_cfg
    for k, v in dict(dyn_pcl_remove_outlier=False, st_render_pcl_pts_per_pixel=c.K, st_render_pcl_pt_radius=c.radius).items():
        cfg_rc[k] = v
    model = PGDVSRenderer(cfg, render_cfg=cfg_rc, softsplat_metric_abs_alpha=100.0).to(DEV).eval()
    v = synth.make_video(4, c.H, c.W, seed=11)
    data = synth.to_torch(synth.make_view(v, 1, frac=0.4, seed=2), DEV)
    data["st_pcl_rgb"] = T(np.concatenate([c.pts, c.feat], 1))[None]
    data["flat_cam_tgt"] = T(c.cam)[None]
    with torch.no_grad():
        ret = model.forward(data, render_cfg=cfg_rc)
    return ret, model.view_counters()


def test_dense_degenerate_tile_leaves_the_sorted_path_for_equal_depth_buckets():
    """degen_dense through PGDVSRenderer.forward with data["st_pcl_rgb"]: the rows at z = 1e-30 and z = 3e38 stretch the
    sorted path's buckets over the whole float range, the 1700 points at z in [1, 3] share a few of them, and the view's
    counter says that a tile went to the general path for it -- with the per-op call's image, which is the oracle's"""
    c = rc.cases()["degen_dense"]
    ret, cnt = _view_forward(c)
    assert cnt["static_rows"] == c.pts.shape[0]
    assert cnt["raster_tiles_general_path_equal_depths"] >= 1 and cnt["raster_tiles_general_path_long_list"] == 0, cnt
    assert 1000 < cnt["raster_longest_tile_list"] <= 2048, cnt
    per_op = ops.points_raster(T(c.pts), T(c.feat), ops.cam_prep(T(c.cam)), c.radius, c.K, c.H, c.W, rgb_planar=True)
    assert torch.equal(ret["geo_static_rgb"][0], per_op["rgb"])
    assert torch.equal(ret["geo_static_mask"].reshape(c.H, c.W), per_op["mask"])
    idx, _, _, img, mask = rc.oracle("degen_dense")
    np.testing.assert_allclose(N(per_op["rgb"]).transpose(1, 2, 0), img, rtol=0, atol=1e-6)
    assert np.array_equal(N(per_op["mask"]), mask)
    where = c.claims["special"]
    assert idx[c.H // 2, c.W // 2, 0] == where["zden_axis"] and idx[c.H // 2, c.W // 2, 1] == where["z1e-30_axis"]


@pytest.mark.parametrize("name", ["thr_b4_at_64x64_K3", "thr_b4_below_48x64_K4"])
def test_depth_bound_shortens_the_tile_lists_of_a_threshold_cloud(name):
    """a threshold cloud through PGDVSRenderer.forward with the depth bound forced on (raster_bound_density = 0) and off
    (1e9): the view's own counter of list entries shrinks -- the bound is finite in the cloud's dense tile and drops
    entries there, as tests/test_raster_edges_host.py works out on the host -- and the image does not change"""
    c = rc.cases()[name]
    assert c.claims["bound_runs"]
    out = {}
    for density in (0.0, 1e9):
        with ops.option("raster_bound_density", density):
            out[density] = _view_forward(c)
    (on, cnt_on), (off, cnt_off) = out[0.0], out[1e9]
    assert cnt_on["static_rows"] == cnt_off["static_rows"] == c.pts.shape[0]
    assert 0 < cnt_on["raster_list_entries"] < cnt_off["raster_list_entries"], (cnt_on, cnt_off)
    assert torch.equal(on["geo_static_rgb"], off["geo_static_rgb"]) and torch.equal(on["geo_static_mask"], off["geo_static_mask"])
    _, _, _, img, mask = rc.oracle(name)
    np.testing.assert_allclose(N(on["geo_static_rgb"][0]).transpose(1, 2, 0), img, rtol=0, atol=1e-6)
    assert np.array_equal(N(on["geo_static_mask"]).reshape(c.H, c.W), mask)


# ---------------------------------------------------------------- the disc edge under the compositor's clamp
@pytest.mark.parametrize("name", rc.names("graze_"))
def test_grazing_pixels_keep_mask_one_and_the_scaled_colour(name):
    """a pixel whose only fragment grazes the disc edge (w = 1 - d2 / r2 of a few 1e-6, below the clamp 1e-4): mask 1 and
    the colour w f / 1e-4 -- the oracle's float32 operations in its order, so a few ulps at the most (2^-21 relative);
    a disc with d2 == r2 exactly, or one float32 step beyond, leaves no fragment"""
    c = rc.cases()[name]
    idx, _, d2, img, mask = rc.oracle(name)
    r = ops.points_raster(T(c.pts), T(c.feat), ops.cam_prep(T(c.cam)), c.radius, c.K, c.H, c.W, want_fragments=True)
    g_idx, g_rgb, g_mask = N(r["idx"]), N(r["rgb"]), N(r["mask"])
    r2 = F32(F32(c.radius) * F32(c.radius))
    w0 = np.where(idx[..., 0] >= 0, F32(1) - d2[..., 0] / r2, F32(1)).astype(F32)
    graze = w0 < F32(1e-4)
    lone = graze & ((idx >= 0).sum(-1) == 1)
    assert graze.sum() >= c.claims["front_min"] and lone.sum() >= c.claims["lone_min"]
    assert (g_mask[graze] == 1).all() and np.array_equal(g_idx[graze], idx[graze])
    assert np.all(g_rgb[lone] > 0) and np.all(g_rgb[lone] < 0.2)
    np.testing.assert_allclose(g_rgb[lone], img[lone], rtol=2.0 ** -21, atol=0)
    for row, yi, xi, kind in c.claims["graze"]:
        if kind in ("eq", "gt"):
            assert not (g_idx[yi, xi] == row).any(), (row, yi, xi, kind)
        elif kind == "in":
            assert g_idx[yi, xi, 0] == row, (row, yi, xi)


# ---------------------------------------------------------------- nothing is written outside the outputs
GUARD = 256  # bytes on either side of a buffer (keeps the 256-byte alignment of what lies between)


class _Guarded:
    """``nbytes`` of device memory between two guard blocks, everything filled with 0xA5"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD)

    def body(self, dtype):
        return N(self.buf[GUARD:GUARD + self.nbytes]).view(dtype)

    def guards_intact(self):
        b = N(self.buf)
        return bool(np.all(b[:GUARD] == 0xA5) and np.all(b[GUARD + self.nbytes:] == 0xA5))

    def untouched(self):
        return bool(np.all(N(self.buf) == 0xA5))


@pytest.mark.parametrize("with_fragments", [True, False])
@pytest.mark.parametrize("name", ["shape_1x1", "shape_1x300", "shape_300x1", "shape_2x2", "shape_4x2048", "shape_2048x4", "shape_4x8192",
                                  "thr_b4_at_15x17_K8", "graze_17x15_layer_K3"])
def test_points_raster_writes_only_its_outputs(name, with_fragments):
    """partial tiles on every side of the image: rgb, mask, the fragment tensors and the workspace keep their guard blocks,
    and without fragment pointers the fragment tensors are not touched at all"""
    c = rc.cases()[name]
    idx, zbuf, d2, img, mask = rc.oracle(name)
    lib = _lib.load()
    P, n = c.H * c.W, c.pts.shape[0]
    ws_bytes = int(lib.pgdvs_points_raster_workspace_bytes(n, c.H, c.W, c.radius))
    assert ws_bytes > 0
    g_idx, g_z, g_d2 = _Guarded(8 * P * c.K), _Guarded(4 * P * c.K), _Guarded(4 * P * c.K)
    g_rgb, g_mask, g_ws = _Guarded(12 * P), _Guarded(4 * P), _Guarded(ws_bytes)
    pts, feat, cam = T(c.pts), T(c.feat), ops.cam_prep(T(c.cam))
    null = C.c_void_p(0)
    status = lib.pgdvs_points_raster(C.c_void_p(pts.data_ptr()), 3, C.c_void_p(feat.data_ptr()), 3, n, null, C.c_void_p(cam.data_ptr()),
                                     c.radius, c.K, c.H, c.W, g_idx.ptr if with_fragments else null,
                                     g_z.ptr if with_fragments else null, g_d2.ptr if with_fragments else null, g_rgb.ptr, 0, g_mask.ptr,
                                     g_ws.ptr, ws_bytes, ops._stream())
    torch.cuda.synchronize()
    assert status == 0
    for g in (g_idx, g_z, g_d2, g_rgb, g_mask, g_ws):
        assert g.guards_intact()
    assert np.array_equal(_bits(g_mask.body(np.float32).reshape(c.H, c.W)), _bits(mask))
    np.testing.assert_allclose(g_rgb.body(np.float32).reshape(c.H, c.W, 3), img, rtol=0, atol=1e-6)
    if with_fragments:
        assert np.array_equal(g_idx.body(np.int64).reshape(c.H, c.W, c.K), idx)
        assert np.array_equal(g_z.body(np.uint32).reshape(c.H, c.W, c.K), _bits(zbuf))
        assert np.array_equal(g_d2.body(np.uint32).reshape(c.H, c.W, c.K), _bits(d2))
    else:
        assert g_idx.untouched() and g_z.untouched() and g_d2.untouched()
