"""CPU: the GNT oracle (oracle/gnt_oracle.py) against the edge fixtures of the gather stage, made by the reference itself
(tests/golden/make_golden_gnt_edges.py): projections exactly on and one ulp beyond the four borders, p.z at, below and
around the 1e-8 clamp, samples on a source camera's centre, source cameras coinciding with the target, bilinear mask
values on either side of 1e-3, images smaller than the cameras' (h, w) with (h, w) differing between views, channel
counts 30 / 32 / 64 / 68, uniform and inverse sampling with per-view and per-ray ranges, and the importance
re-sampling.  Masks exact; float outputs at the tolerances of test_oracle_golden.py and test_gpu_parity.py."""
import numpy as np
import pytest

from oracle import gnt_oracle as G

GATHER_ITEMS = [
    ("bounds", "mask1"), ("bounds", "mask0"), ("depth", "mask1"), ("angle", "mask1"), ("mask", "mask1"), ("mask", "mask0"),
    ("sizes", "c32_v3_perray_uniform"), ("sizes", "c64_v7_perview_inverse"), ("sizes", "c30_v1_fine"),
    ("sizes", "c68_v3_perray_inverse"), ("sizes", "c32_v3_perview_uniform_nomask"),
]
CASES = ["bounds", "depth", "angle", "mask", "sizes"]
COARSE = [f"coarse_{rk}_iu{iu}_s{S}" for rk in ("perview", "perray") for iu in (0, 1) for S in (2, 3, 64)]
FINE = [f"fine_{rk}_iu{iu}" for rk in ("perview", "perray") for iu in (0, 1)]


def _case(golden_dir, case):
    return dict(np.load(golden_dir / f"gnt_edges_{case}.npz"))


def _item(g, item):
    """an item's arrays; those it shares with the case's first item are stored once, under the first"""
    first = str(g["items"][0])
    d = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(first + "__")}
    d.update({k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(item + "__")})
    if str(d["route"]) == "z_in":  # explicit depths
        d["S"] = np.int64(d["z_in"].shape[1])
    return d


def _oracle_gather(g):
    V, C = int(g["V"]), int(g["C"])
    if str(g["route"]) == "z_in":  # explicit depths: the route of the fine pass
        z = g["z_in"]
        pts = (z[:, :, None] * g["ray_d"][:, None, :] + g["ray_o"][:, None, :]).astype(np.float32)
    else:
        pts, z = G.sample_along_camera_ray(g["ray_o"], g["ray_d"], np.broadcast_to(g["depth_range"], (g["ray_o"].shape[0], 2)),
                                           int(g["S"]), bool(g["inv_uniform"]))
    o = G.projector_compute(pts, g["cam_tgt"], g["src_rgbs"][:V], g["cams_src"][:V], g["featmaps"][:V, :C],
                            g["inv_masks"][:V] if bool(g["use_mask"]) else None)
    o.update(pts=pts, z_vals=z)
    return o


@pytest.mark.parametrize("case,item", GATHER_ITEMS, ids=[f"{c}-{i}" for c, i in GATHER_ITEMS])
def test_oracle_gather_edges(golden_dir, case, item):
    g = _item(_case(golden_dir, case), item)
    o = _oracle_gather(g)
    for k in ("mask_inbound", "mask_invalid", "mask"):  # decisions: exact, no item left out
        assert np.array_equal(o[k], g["out_" + k]), (k, int((o[k] != g["out_" + k]).sum()))
    np.testing.assert_allclose(o["pts"], g["out_pts"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(o["z_vals"], g["out_z_vals"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(o["rgb_feat"], g["out_rgb_feat"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(o["ray_diff"], g["out_ray_diff"], rtol=0, atol=5e-5)


@pytest.mark.parametrize("case", CASES)
def test_fixture_margins(golden_dir, case):
    """every decision of every item is settled: its quantity is bit-identical in the reference's float32 and float64
    runs, or 64 x the case's float32-to-float64 difference away from the decision; the reference's own float error
    is at most half the tolerance; the case reaches the borders as often as the generator recorded"""
    gc = _case(golden_dir, case)
    n_border = 0
    for item in (str(i) for i in gc["items"]):
        g = _item(gc, item)
        assert float(g["margin"]) == 64.0
        h, w = (float(x) for x in g["cams_src"][0][:2])
        u, v, pz, mv, same = g["m_pix64"][..., 0], g["m_pix64"][..., 1], g["m_pz64"], g["m_mval64"], g["m_same"]
        dp, dz, dm = float(g["diff_pix"]), float(g["diff_pz"]), float(g["diff_mval"])
        conds = [(u, 0), (w - 1.0 - u, 0), (v, 1), (h - 1.0 - v, 1)]
        holds = [c >= 0 for c, _ in conds] + [pz > 0]
        settled = [same[..., q] | (np.abs(c) >= 64.0 * dp) for c, q in conds] + [same[..., 2] | (np.abs(pz) >= 64.0 * dz)]
        inb = np.all(holds, 0)
        ok = np.where(inb, np.all(settled, 0), np.any([~a & b for a, b in zip(holds, settled)], 0))
        assert ok.all(), (item, int((~ok).sum()))
        assert np.array_equal(inb, g["out_mask_inbound"][..., 0].transpose(2, 0, 1) > 0)
        if bool(g["use_mask"]):
            assert np.all(same[..., 3] | (np.abs(mv - 1e-3) >= 64.0 * dm))
            # (the threshold of the float32 run: one item of the mask case holds float32(1e-3) itself)
            assert np.array_equal(mv > float(np.float32(1e-3)), g["out_mask_invalid"][..., 0].transpose(2, 0, 1) > 0)
        near = (pz > 0) & (u >= -1) & (u <= w) & (v >= -1) & (v <= h) & (
            (np.abs(u) <= 1) | (np.abs(u - (w - 1)) <= 1) | (np.abs(v) <= 1) | (np.abs(v - (h - 1)) <= 1))
        assert int(near.sum()) == int(g["n_border"]) and near.size == int(g["n_items"])
        n_border += int(near.sum())
        for k, (rtol, atol) in {"pts": (1e-6, 1e-6), "z_vals": (1e-6, 1e-6), "rgb_feat": (0, 5e-5), "ray_diff": (0, 5e-5)}.items():
            err = np.abs(g["out_" + k].astype(np.float64) - g["out64_" + k])
            assert np.all(err <= 0.5 * (atol + rtol * np.abs(g["out64_" + k]))), (item, k)
            assert float(err.max()) == float(g["err_" + k])
    assert n_border >= 40, n_border  # the case visibly exercises the border


def test_edge_cases_reach_their_edges(golden_dir):
    g = _item(_case(golden_dir, "bounds"), "mask1")
    u, v = g["m_pix64"][0, :, :, 0], g["m_pix64"][0, :, :, 1]
    inb = g["out_mask_inbound"][:, :, 0, 0] > 0
    for on in (u == 0, u == 32, v == 0, v == 16, (u == 0) & (v == 0), (u == 32) & (v == 16), (u == 0) & (v == 16), (u == 32) & (v == 0)):
        assert np.any(on & inb)
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    for out in (u == -tiny, v == -tiny, u == float(np.nextafter(np.float32(32), np.float32(64))),
                v == float(np.nextafter(np.float32(16), np.float32(64)))):
        assert np.any(out) and not np.any(out & inb)
    g = _item(_case(golden_dir, "depth"), "mask1")
    pz = g["m_pz64"]
    assert np.any(pz == 0) and np.any((pz > 0) & (pz < 1e-8)) and np.any((pz > 1e-8) & (pz < 1e-7)) and np.any((pz < 0) & (pz > -1e-8))
    assert np.sum(np.abs(g["m_pix64"]) == 1e6) > 20
    assert np.any((pz > 0) & (pz < 1e-7) & (g["out_mask_inbound"][..., 0].transpose(2, 0, 1) > 0))  # tiny z, inside the image
    g = _item(_case(golden_dir, "mask"), "mask1")
    mv = g["m_mval64"][0]
    for val in (0.0, 2.0 ** -10, 2.0 ** -9, 1.0):
        assert np.sum(mv == val) >= 5
    thr = np.float32(1e-3)
    for val in (thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0))):
        assert np.sum(mv == float(val)) >= 1
    g = _item(_case(golden_dir, "angle"), "mask1")
    assert np.array_equal(g["cams_src"][0], g["cam_tgt"]) and np.all(g["out_ray_diff"][:, :, :2, :3] == 0)
    gc = _case(golden_dir, "sizes")
    g = _item(gc, "c64_v7_perview_inverse")
    assert g["src_rgbs"].shape[1] * 2 == g["cams_src"][0, 0] and len({tuple(c[:2]) for c in g["cams_src"]}) > 3
    assert _item(gc, "c30_v1_fine")["out_rgb_feat"].shape[-1] == 33 and _item(gc, "c68_v3_perray_inverse")["out_rgb_feat"].shape[-1] == 71


RENDER = ["uni", "inv"]
RENDER_TOL = {"out_": 2e-4, "fine_": 3e-4}  # of test_gnt_renderer_end_to_end_vs_reference


def render_keys(g, tag):
    """(output group prefix, key) of a render record's stored float32 outputs"""
    return [(pre, k[len(tag) + 2 + len(pre):]) for pre in RENDER_TOL for k in g
            if k.startswith(f"{tag}__{pre}") and not k.endswith("_64")]


@pytest.mark.parametrize("tag", RENDER)
def test_oracle_render_edges(golden_dir, tag):
    """BaseRenderer.forward at B = 2 with per-ray ranges: render_rays per batch item on its slice of the rays and ranges"""
    g = _case(golden_dir, "render")
    small = np.load(golden_dir / "gnt_small.npz")
    Wt = {k[2:]: small[k] for k in small.files if k.startswith("w_")}
    B, s = int(g["B"]), int(g["render_stride"])
    per_ray = g["depth_range_map"][:, ::s, ::s].reshape(-1, 2)
    n = g["ray_o"].shape[0] // B
    n_fine = int(g[tag + "__n_fine"])
    parts = []
    for b in range(B):
        sl = slice(b * n, (b + 1) * n)
        r = G.render_rays(Wt, g["ray_o"][sl], g["ray_d"][sl], per_ray[sl], int(g["Ss"]), g["cam_tgt"][b], g["src_rgbs"][b], g["cams_src"][b],
                          g["featmaps"][b], g["inv_masks"][b], inv_uniform=bool(g[tag + "__inv_uniform"]), n_fine=n_fine)
        parts.append(r if n_fine > 0 else (r, None))
    keys = render_keys(g, tag)
    assert ("fine_", "rgb") in keys if n_fine > 0 else all(pre == "out_" for pre, _ in keys)
    for pre, k in keys:
        ref = g[f"{tag}__{pre}{k}"]
        o = np.concatenate([p[pre == "fine_"][k].reshape(n, -1) for p in parts]).reshape(ref.shape)
        np.testing.assert_allclose(o, ref, rtol=0, atol=RENDER_TOL[pre], err_msg=pre + k)
    assert float(g["err_coarse"]) <= 1e-4 and float(g["err_fine"]) <= 1.5e-4  # the reference's own float32 error: half the tolerance


@pytest.mark.parametrize("name", COARSE)
def test_oracle_coarse_sampling(golden_dir, name):
    g = _case(golden_dir, "sampling")
    rk, iu, S = name.split("_")[1], int(name.split("_")[2][2:]), int(name.split("_")[3][1:])
    R = g["ray_o"].shape[0]
    pts, z = G.sample_along_camera_ray(g["ray_o"], g["ray_d"], np.broadcast_to(g["range_" + rk], (R, 2)), S, bool(iu))
    np.testing.assert_allclose(z, g[name + "__z_vals"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(pts, g[name + "__pts"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", FINE)
def test_oracle_fine_sampling(golden_dir, name):
    g = _case(golden_dir, "sampling")
    iu = int(g[name + "__inv_uniform"])
    z_all = G.sample_fine_z(bool(iu), int(g[name + "__n_fine"]), g[f"fine_weights_iu{iu}"], g[name + "__z_coarse"])
    np.testing.assert_allclose(z_all, g[name + "__z_all"], rtol=1e-6, atol=0)
    err = np.abs(g[name + "__z_all"].astype(np.float64) - g[name + "__z_all64"])
    assert np.all(err <= 0.5e-6 * (1 + np.abs(g[name + "__z_all64"])))  # conditioned: see the generator
    w = g[f"fine_weights_iu{iu}"]
    assert len(g["fine_special_rows"]) >= 8 and np.all(w[:3] == 0) and np.all((w[3:6] != 0).sum(1) == 1)


# ---------------------------------------------------------------- inputs of the sweep at the size the product runs
SWEEP = dict(H=288, W=550, V=10, hf=72, wf=138, C=32, R=4096, S=64)


def _cam(h, w, f, yaw, pitch, t, cx, cy):
    y, p = np.deg2rad(yaw), np.deg2rad(pitch)
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    c2w, K = np.eye(4), np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Ry @ Rx, t
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = cx, cy
    return np.concatenate(([h, w], K.flatten(), c2w.flatten())).astype(np.float32)


def _smooth(rng, shape, ay, ax, mean, amp):
    """O(1) values that vary slowly along the two image axes `ay`, `ax` (at most ~0.05 per pixel), with a random phase and
    frequency per remaining index"""
    ny, nx = shape[ay], shape[ax]
    other = tuple(1 if i in (ay, ax) else n for i, n in enumerate(shape))
    yy = np.arange(ny).reshape(tuple(ny if i == ay else 1 for i in range(len(shape)))) / ny
    xx = np.arange(nx).reshape(tuple(nx if i == ax else 1 for i in range(len(shape)))) / nx
    fy, fx, ph = (rng.random(other) * 4 + 1 for _ in range(3))
    # ... and fall to 0 on the border rows and columns: outside the map grid_sample's zero padding is a ramp of one pixel from
    # the border value to 0, whose slope would otherwise be O(1) per pixel
    win = np.sin(np.pi * np.arange(ny).reshape(yy.shape) / (ny - 1)) * np.sin(np.pi * np.arange(nx).reshape(xx.shape) / (nx - 1))
    return ((mean + amp * np.sin(fy * yy + fx * xx + 2 * ph)) * np.clip(win, 0, None) ** 0.5).astype(np.float32)


def sweep_inputs(seed=7):
    """seeded synthetic inputs: a 288 x 550 view, 10 source views on an arc around the target, a 72 x 138 x 32 feature
    map, 4 096 rays through random pixels with per-ray ranges, half-plane dynamic masks (a mask sample is then 0, 1 or
    the fractional pixel coordinate, so its 1e-3 threshold is one more line in the image).  Images and features are
    smooth: at u ~ 500 a pixel coordinate carries a few float32 ulps (~1e-4 px) of rounding in any arithmetic, which
    white noise (a slope of ~1 per pixel) would turn into more than the 2e-5 tolerance -- conditioning, not the kernel.
    For the same reason they fall to 0 towards the borders (the zero-padding ramp just outside a map)"""
    p = SWEEP
    rng = np.random.default_rng(seed)
    H, W, V, R = p["H"], p["W"], p["V"], p["R"]
    f = 0.9 * W
    cam_tgt = _cam(H, W, f, 0.5, -0.4, [0.03, -0.02, 0.0], W / 2, H / 2)
    cams = np.stack([_cam(H, W, f * (1 + 0.01 * i), 2.5 * (i - 4.5), 0.6 * (i - 4.5), [0.12 * (i - 4.5), 0.03 * (i % 3 - 1), 0.01 * i],
                          W / 2 + 0.3 * i, H / 2 - 0.2 * i) for i in range(V)])
    K, c2w = cam_tgt[2:18].reshape(4, 4).astype(np.float64), cam_tgt[18:34].reshape(4, 4).astype(np.float64)
    uv = rng.random((R, 2)) * [W - 1, H - 1]
    d = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(R)], -1) @ c2w[:3, :3].T
    near = 0.5 + rng.random(R)
    rng_ = np.stack([near, near * (2 + 3 * rng.random(R))], 1).astype(np.float32)
    masks = np.zeros((V, H, W, 1), np.float32)
    for v in range(V):
        if v % 2:
            masks[v, :, 150 + 25 * v:] = 1
        else:
            masks[v, :40 + 15 * v] = 1
    return dict(ray_o=np.tile(c2w[:3, 3], (R, 1)).astype(np.float32), ray_d=d.astype(np.float32), depth_range=rng_, cam_tgt=cam_tgt,
                cams_src=cams, src_rgbs=_smooth(rng, (V, H, W, 3), 1, 2, 0.5, 0.5), featmaps=_smooth(rng, (V, p["C"], p["hf"], p["wf"]), 2, 3, 0.0, 1.0),
                inv_masks=masks)


def sweep_oracle(x, inv_uniform):
    pts, z = G.sample_along_camera_ray(x["ray_o"], x["ray_d"], x["depth_range"], SWEEP["S"], inv_uniform)
    o = G.projector_compute(pts, x["cam_tgt"], x["src_rgbs"], x["cams_src"], x["featmaps"], x["inv_masks"], geometry=True)
    o.update(pts=pts, z_vals=z)
    h, w = (float(c) for c in x["cams_src"][0][:2])
    u, v = o["pix"][..., 0:1].astype(np.float64), o["pix"][..., 1:2].astype(np.float64)
    near_bound = np.minimum.reduce([np.abs(u), np.abs(u - (w - 1)), np.abs(v), np.abs(v - (h - 1))]) <= 1e-3
    # The dynamic masks are half-planes, so a mask sample is 0, 1 or the pixel's distance from the region's edge: the
    # 1e-3 threshold of the mask is one more bound in the image, 1e-3 px inside the edge.  Within 5e-4 px of it is exempt.
    near_thr = np.abs(o["mval"].astype(np.float64) - 1e-3) <= 5e-4
    o["exempt"] = near_bound | (np.abs(o["pz"]) <= 1e-6) | near_thr
    return o


@pytest.mark.parametrize("inv_uniform", [False, True])
def test_sweep_inputs_are_well_posed(inv_uniform):
    """the oracle alone: the exempt set (pixel within 1e-3 px of a bound of the image or 5e-4 px of the mask's 1e-3 line,
    p.z within 1e-6 of 0) holds at most 1e-4 of the items, and the sweep reaches every decision in bulk"""
    o = sweep_oracle(sweep_inputs(), inv_uniform)
    share = float(o["exempt"].mean())
    print(f"exempt share {share:.2e}, inbound share {float(o['mask_inbound'].mean()):.2f}, invalid share {float(o['mask_invalid'].mean()):.2f}")
    assert share <= 1e-4
    assert float(o["mask_inbound"].mean()) > 0.3 and 0.05 < float(o["mask_invalid"].mean()) < 0.9
