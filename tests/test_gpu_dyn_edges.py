"""GPU (MI355X): the HIP dynamic branch against the reference's edge fixtures (tests/golden/make_golden_dyn_edges.py)
-- integer and half-integer flows (nearest-sample ties), flows onto and one ulp past the borders, non-finite flows, time
stamps at and outside [t1, t2], zero and negative depths (the projection's clamps), a frame above 4096 pixels -- through
the per-op path, the standalone ops, PGDVSRenderer.forward on the per-op path and the one native call per view.
Integer outputs equal to the reference's; float outputs bit-exact against the oracle where the operation order is
shared, and within the tolerances of test_gpu_parity.py against the reference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402  (checker only)
from pgdvs_amd import ops  # noqa: E402
from pgdvs_amd.instantiate import AttrDict, load_config  # noqa: E402
from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer  # noqa: E402
from pgdvs_amd.utils.softsplat import softsplat  # noqa: E402

DEV = "cuda:0"
DYN_ITEMS = [
    ("integer", "rm0"), ("integer", "rm1"), ("half", "rm0"), ("half", "rm1"),
    ("bounds", "fc1_rm0"), ("bounds", "fc1_rm1"), ("bounds", "fc0_rm0"),
    ("time", "tt_eq_t1"), ("time", "tt_eq_t2"), ("time", "tt_lt_t1"), ("time", "tt_gt_t2"),
    ("depth", "tt_eq_t1"), ("depth", "same_time"), ("depth", "tt_34"), ("depth", "tt_34_rm1"),
    ("large", "rm1"),
]
FWD_CASES = ["integer", "bounds", "depth", "large"]
MODES = ["sum", "avg", "linear", "soft", "soft-zeroeps", "soft-clipeps"]


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def _case(golden_dir, case):
    return dict(np.load(golden_dir / f"dyn_edges_{case}.npz"))


def _item(g, item):
    """an item's arrays; those it shares with the case's first item are stored once, under the first"""
    first = str(g["items"][0])
    d = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(first + "__")}
    d.update({k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(item + "__")})
    return d


def _fwd(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("fwd__")}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()  # fails loudly if the HIP extension is missing


# ---------------------------------------------------------------- per-op path
@pytest.mark.parametrize("case,item", DYN_ITEMS, ids=[f"{c}-{i}" for c, i in DYN_ITEMS])
def test_compute_dyn_pcl_edges(golden_dir, case, item):
    g = _item(_case(golden_dir, case), item)
    cams = ops.cam_prep(T(np.stack([g["flat_cam_1"], g["flat_cam_2"], g["flat_cam_tgt"]])))
    times = T(np.array([g["time_1"], g["time_2"], g["time_tgt"]], np.float32))
    rc = AttrDict(dyn_render_use_flow_consistency=bool(g["use_flow_consistency"]),
                  dyn_pcl_remove_outlier=bool(g["remove_outlier"]), dyn_pcl_outlier_knn=int(g["outlier_knn"]),
                  dyn_pcl_outlier_std_thres=float(g["outlier_std_thres"]))
    from pgdvs_amd.renderers.pgdvs_renderer_dyn import PGDVSDynamicRenderer

    dyn = PGDVSDynamicRenderer(cfg=AttrDict(rgb_range="0_1"), proj_func=None)
    flow, vmask, info = dyn.compute_dyn_pcl(
        dyn_mask_1=T(g["dyn_mask_1"][..., 0]), rgb_1=T(g["rgb_1"]), depth_1=T(g["depth_1"][..., 0]),
        flow_12=T(g["flow_12"]), flow_12_occ_mask=T(g["flow_12_occ_mask"][..., 0]), rgb_2=T(g["rgb_2"]),
        depth_2=T(g["depth_2"][..., 0]), cam_1=cams[0], cam_2=cams[1], cam_tgt=cams[2], times=times,
        render_cfg=rc, need_points=True)
    o = orc.compute_dyn_pcl(
        dyn_mask_1=g["dyn_mask_1"], rgb_1=g["rgb_1"], depth_1=g["depth_1"], flow_12=g["flow_12"],
        flow_12_occ_mask=g["flow_12_occ_mask"], rgb_2=g["rgb_2"], depth_2=g["depth_2"], flat_cam_1=g["flat_cam_1"],
        flat_cam_2=g["flat_cam_2"], flat_cam_tgt=g["flat_cam_tgt"], time_1=float(g["time_1"]), time_2=float(g["time_2"]),
        time_tgt=float(g["time_tgt"]), dyn_render_use_flow_consistency=rc.dyn_render_use_flow_consistency,
        dyn_pcl_remove_outlier=rc.dyn_pcl_remove_outlier, dyn_pcl_outlier_knn=rc.dyn_pcl_outlier_knn,
        dyn_pcl_outlier_std_thres=rc.dyn_pcl_outlier_std_thres)
    # integer paths: equal to the reference (and to the oracle)
    assert np.array_equal(N(info["valid"]).astype(bool), o["valid"])
    assert np.array_equal(N(vmask), g["out_valid_dyn_mask_1"][..., 0])
    n = int(info["n_pts"].item())
    assert n == g["out_pcl"].shape[0]
    # float paths: the oracle's operation order -> bit-exact; against the reference within tolerance
    vb = o["valid"]
    assert np.array_equal(N(info["pcl_dense"])[vb].view(np.uint32), o["pcl_dense"][vb].view(np.uint32))
    f_gpu = N(flow).transpose(1, 2, 0)
    assert np.array_equal(f_gpu.view(np.uint32), o["flow_1_to_tgt"].view(np.uint32))
    np.testing.assert_allclose(f_gpu, g["out_flow_1_to_tgt"], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(N(info["pcl"])[:n], g["out_pcl"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(N(info["pcl_rgbs"])[:n], g["out_pcl_rgbs"], rtol=1e-5, atol=1e-5)
    if rc.dyn_pcl_remove_outlier:
        np.testing.assert_allclose(N(info["pcl_nn_dist_thres"])[0], g["out_nn_dist_thres"], rtol=1e-5)


# ---------------------------------------------------------------- standalone ops
@pytest.mark.parametrize("tag", ["a", "b"])
def test_project_points_edges(golden_dir, tag):
    g = _case(golden_dir, "ops")
    fc, xyz, ref_uv = g[f"project_{tag}_flat_cam"], g[f"project_{tag}_xyz"], g[f"project_{tag}_uv"]
    uv = N(ops.project_points(ops.cam_prep(T(fc)), T(xyz)))
    assert np.array_equal(uv.view(np.uint32), orc.project(fc, xyz).view(np.uint32))
    np.testing.assert_allclose(uv, ref_uv, rtol=2e-5, atol=2e-4)
    if tag == "a":  # dyadic camera and points: the clamps and the pixel centres are exact
        assert np.array_equal(uv, ref_uv)


def test_backwarp_l1_edges(golden_dir):
    g = _case(golden_dir, "ops")
    l1 = N(ops.backwarp_l1(T(g["backwarp_rgb1"]), T(g["backwarp_rgb2"]), T(g["backwarp_flow"])))
    np.testing.assert_allclose(l1, g["backwarp_l1"], rtol=1e-5, atol=2e-6)
    for b in range(l1.shape[0]):
        o = orc.backwarp_l1(g["backwarp_rgb1"][b], g["backwarp_rgb2"][b], g["backwarp_flow"][b])
        np.testing.assert_allclose(l1[b, 0], o, rtol=0, atol=1e-7)


@pytest.mark.parametrize("mode", MODES)
def test_softsplat_edges(golden_dir, mode):
    g = _case(golden_dir, "ops")
    m = g["softsplat_ten_metric"]
    metric = None if mode in ("sum", "avg") else (m if mode != "linear" else np.abs(m) + 0.1)
    out = N(softsplat(T(g["softsplat_ten_in"]), T(g["softsplat_ten_flow"]), None if metric is None else T(metric), mode))
    np.testing.assert_allclose(out, g["softsplat_out_" + mode.replace("-", "_")], rtol=2e-5, atol=2e-6)  # vs reference
    np.testing.assert_allclose(out, orc.softsplat(g["softsplat_ten_in"], g["softsplat_ten_flow"], metric, mode),
                               rtol=2e-5, atol=2e-6)


# ---------------------------------------------------------------- PGDVSRenderer.forward
def _renderer(static, g):
    cfg = load_config(static_renderer=static)
    rc = cfg.engine.engine_cfg.render_cfg
    for k, v in dict(render_stride=int(g["render_stride"]), dyn_render_use_flow_consistency=bool(g["use_flow_consistency"]),
                     dyn_pcl_remove_outlier=bool(g["remove_outlier"]), dyn_pcl_outlier_knn=int(g["outlier_knn"]),
                     dyn_pcl_outlier_std_thres=float(g["outlier_std_thres"])).items():
        rc[k] = v
    return PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(DEV).eval(), rc


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_per_op_edges(golden_dir, case, monkeypatch):
    """batch 1 through the rgb_gnt shortcut on the per-op path"""
    monkeypatch.setenv("PGDVS_NATIVE_VIEW", "0")
    g = _fwd(_case(golden_dir, case))
    data = {k[3:]: T(v) for k, v in g.items() if k.startswith("in_")}
    data["static_noise"] = T(g["static_noise"])
    model, rc = _renderer("gnt", g)
    assert not model._native_view_ok(data, rc)
    with torch.no_grad():
        ret = model.forward(data, render_cfg=rc, disable_tqdm=True)
    assert np.array_equal(N(ret["render_dyn_mask"]), g["out_render_dyn_mask"])  # thresholded: exact
    for k in ["render_dyn_rgb", "combined_rgb", "combined_rgb_static", "combined_rgb_dyn", "static_coarse_rgb",
              "render_dyn_temporal_closest_rgb", "render_dyn_temporal_track_rgb"]:
        np.testing.assert_allclose(N(ret[k]), g["out_" + k], rtol=0, atol=1e-4, err_msg=k)


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_native_view_edges(golden_dir, case):
    """the same inputs through the one native call per view (pgdvs_view_geo_forward, what bench.py measures): the
    dynamic mask and colours do not depend on the static renderer, so they must be the reference's"""
    g = _fwd(_case(golden_dir, case))
    data = {k[3:]: T(v) for k, v in g.items() if k.startswith("in_") and k != "in_rgb_gnt"}
    data["static_noise"] = T(g["static_noise"])
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.normal(size=(64, 3)) * 0.5 + np.array([0.0, 0.0, 2.5]), rng.random((64, 3))], 1)
    data["st_pcl_rgb"] = T(cloud.astype(np.float32)[None])
    model, rc = _renderer("geo", g)
    assert model._native_view_ok(data, rc)  # no silent fallback to the per-op path
    with torch.no_grad():
        ret = model.forward(data, render_cfg=rc)
    torch.cuda.synchronize()
    assert np.array_equal(N(ret["render_dyn_mask"]), g["out_render_dyn_mask"])
    np.testing.assert_allclose(N(ret["render_dyn_rgb"]), g["out_render_dyn_rgb"], rtol=0, atol=1e-4)
