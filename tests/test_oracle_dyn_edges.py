"""CPU: the oracle (oracle/) against the dynamic branch's edge fixtures, made by the reference itself
(tests/golden/make_golden_dyn_edges.py): integer and half-integer flows (nearest-sample ties), flows onto and
one ulp past the borders, NaN / inf / -0.0 flows, time stamps at and outside [t1, t2], zero and negative
depths (the projection's z and pixel clamps), a frame above 4096 pixels, and the standalone projection,
backwarp metric and softsplat at the same edges.  Integer outputs exact; float outputs at the tolerances of
test_oracle_golden.py."""
import numpy as np
import pytest

from oracle import oracle as orc

DYN_ITEMS = [
    ("integer", "rm0"), ("integer", "rm1"), ("half", "rm0"), ("half", "rm1"),
    ("bounds", "fc1_rm0"), ("bounds", "fc1_rm1"), ("bounds", "fc0_rm0"),
    ("time", "tt_eq_t1"), ("time", "tt_eq_t2"), ("time", "tt_lt_t1"), ("time", "tt_gt_t2"),
    ("depth", "tt_eq_t1"), ("depth", "same_time"), ("depth", "tt_34"), ("depth", "tt_34_rm1"),
    ("large", "rm1"),
]
FWD_CASES = ["integer", "bounds", "depth", "large"]
MODES = ["sum", "avg", "linear", "soft", "soft-zeroeps", "soft-clipeps"]
CAM_P = 21  # offset of the 4 x 4 projection K @ w2c in a camera block (pgdvs_oracle.c)


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


def _oracle_dyn_pcl(g):
    return orc.compute_dyn_pcl(
        dyn_mask_1=g["dyn_mask_1"], rgb_1=g["rgb_1"], depth_1=g["depth_1"], flow_12=g["flow_12"],
        flow_12_occ_mask=g["flow_12_occ_mask"], rgb_2=g["rgb_2"], depth_2=g["depth_2"],
        flat_cam_1=g["flat_cam_1"], flat_cam_2=g["flat_cam_2"], flat_cam_tgt=g["flat_cam_tgt"],
        time_1=float(g["time_1"]), time_2=float(g["time_2"]), time_tgt=float(g["time_tgt"]),
        dyn_render_use_flow_consistency=bool(g["use_flow_consistency"]),
        dyn_pcl_remove_outlier=bool(g["remove_outlier"]), dyn_pcl_outlier_knn=int(g["outlier_knn"]),
        dyn_pcl_outlier_std_thres=float(g["outlier_std_thres"]))


@pytest.mark.parametrize("case,item", DYN_ITEMS, ids=[f"{c}-{i}" for c, i in DYN_ITEMS])
def test_compute_dyn_pcl_edges(golden_dir, case, item):
    g = _item(_case(golden_dir, case), item)
    r = _oracle_dyn_pcl(g)
    # integer path: which pixels survive the bounds test, the nearest sample's depth and the outlier filter
    assert np.array_equal(r["valid_dyn_mask_1"], g["out_valid_dyn_mask_1"])
    assert r["pcl"].shape == g["out_pcl"].shape  # n_pts
    np.testing.assert_allclose(r["pcl"], g["out_pcl"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["pcl_rgbs"], g["out_pcl_rgbs"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["pcl_nn_dist_thres"], g["out_nn_dist_thres"], rtol=1e-4)
    np.testing.assert_allclose(r["flow_1_to_tgt"], g["out_flow_1_to_tgt"], rtol=1e-4, atol=2e-4)


def test_edge_cases_reach_their_edges(golden_dir):
    """the fixtures do what they claim: border landings survive, the clamps produce +-1e6 flows, the
    non-finite flows are dropped, and the large frame keeps more than 4096 points"""
    g = _item(_case(golden_dir, "bounds"), "fc0_rm0")
    H, W = g["dyn_mask_1"].shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ux, uy = xx + g["flow_12"][..., 0], yy + g["flow_12"][..., 1]
    v = g["out_valid_dyn_mask_1"][..., 0] > 0
    for on in (ux == 0, ux == W - 1, uy == 0, uy == H - 1):
        assert np.any(v & on)
    assert not np.any(v & ((ux < 0) | (ux > W - 1) | (uy < 0) | (uy > H - 1)))
    assert np.any((g["dyn_mask_1"][..., 0] > 0) & (ux < 0) & (ux > -1e-30))  # one subnormal below 0
    g = _item(_case(golden_dir, "half"), "rm0")
    bad = ~np.isfinite(g["flow_12"]).all(-1) & (g["dyn_mask_1"][..., 0] > 0)
    assert bad.sum() >= 10 and not np.any(g["out_valid_dyn_mask_1"][..., 0][bad])
    g = _item(_case(golden_dir, "depth"), "tt_eq_t1")
    assert np.sum(np.abs(g["out_flow_1_to_tgt"][..., 0] + np.arange(g["flow_12"].shape[1])) == 1e6) > 20
    assert _item(_case(golden_dir, "large"), "rm1")["out_pcl"].shape[0] > 2048


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_edges(golden_dir, case):
    g = _fwd(_case(golden_dir, case))
    data = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    cfg = dict(
        dyn_render_use_flow_consistency=bool(g["use_flow_consistency"]), dyn_pcl_remove_outlier=bool(g["remove_outlier"]),
        dyn_pcl_outlier_knn=int(g["outlier_knn"]), dyn_pcl_outlier_std_thres=float(g["outlier_std_thres"]),
        dyn_render_type="softsplat")
    ret = orc.render_view(data, cfg, static_noise=g["static_noise"], alpha=100.0)
    assert np.array_equal(ret["render_dyn_mask"], g["out_render_dyn_mask"])  # thresholded mask: exact
    for k in ["render_dyn_rgb", "combined_rgb", "combined_rgb_static", "combined_rgb_dyn"]:
        np.testing.assert_allclose(ret[k], g["out_" + k], rtol=0, atol=1e-4, err_msg=k)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_project_edges(golden_dir, tag):
    g = _case(golden_dir, "ops")
    fc, xyz, ref_uv = g[f"project_{tag}_flat_cam"], g[f"project_{tag}_xyz"], g[f"project_{tag}_uv"]
    uv = orc.project(fc, xyz)
    np.testing.assert_allclose(uv, ref_uv, rtol=2e-5, atol=2e-4)
    if tag == "a":  # dyadic camera and points: every product exact, so the clamps and pixel centres are exact
        assert np.array_equal(uv, ref_uv)
    # in-front mask (projections[..., 2] > 0): z in the oracle's operation order
    P = orc.cam_prep(fc)[CAM_P:CAM_P + 16].reshape(4, 4)
    z = P[2, 0] * xyz[:, 0]
    z = z + P[2, 1] * xyz[:, 1]
    z = z + P[2, 2] * xyz[:, 2]
    z = z + P[2, 3]
    assert np.array_equal(z > 0, g[f"project_{tag}_mask"])


def test_backwarp_l1_edges(golden_dir):
    g = _case(golden_dir, "ops")
    for b in range(g["backwarp_flow"].shape[0]):
        l1 = orc.backwarp_l1(g["backwarp_rgb1"][b], g["backwarp_rgb2"][b], g["backwarp_flow"][b])
        np.testing.assert_allclose(l1, g["backwarp_l1"][b, 0], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("mode", MODES)
def test_softsplat_edges(golden_dir, mode):
    g = _case(golden_dir, "ops")
    m = g["softsplat_ten_metric"]
    metric = None if mode in ("sum", "avg") else (m if mode != "linear" else np.abs(m) + 0.1)
    out = orc.softsplat(g["softsplat_ten_in"], g["softsplat_ten_flow"], metric, mode)
    np.testing.assert_allclose(out, g["softsplat_out_" + mode.replace("-", "_")], rtol=2e-5, atol=2e-6)
