"""GPU (MI355X): the HIP gather stage (pgdvs_gnt_gather through ops.gnt_gather) and the importance re-sampling against
the reference's edge fixtures (tests/golden/make_golden_gnt_edges.py) -- projections on and one ulp beyond the borders,
p.z at, below and around the 1e-8 clamp, samples on a source camera's centre, source cameras coinciding with the
target, mask values on either side of 1e-3, images smaller than the cameras' (h, w), C = 30 / 32 / 64 / 68, uniform and
inverse sampling with per-view and per-ray ranges, explicit depths.  Masks equal to the reference's on every item;
float outputs within the tolerances of test_gnt_gather_vs_reference_and_oracle against the float32 reference and within
4 x the reference's own float32 error (floor: one ulp of the output's largest magnitude) against the float64 one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pgdvs_amd import ops  # noqa: E402
from pgdvs_amd.models.gnt.ray_sampler import sample_fine_z  # noqa: E402

import test_oracle_gnt_edges as E  # noqa: E402  (fixture helpers, item lists and the sweep's inputs)
from test_oracle_gnt_edges import COARSE, FINE, GATHER_ITEMS, RENDER, RENDER_TOL, _case, _item  # noqa: E402

DEV = "cuda:0"
OUTS = ("pts", "z_vals", "rgb_feat", "ray_diff", "mask_inbound", "mask_invalid", "mask")
TOL = {"pts": (1e-6, 1e-6), "z_vals": (1e-6, 1e-6), "rgb_feat": (0, 5e-5), "ray_diff": (0, 5e-5)}


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()  # fails loudly if the HIP extension is missing


def _misaligned(t):
    """the same values as a contiguous view one float into a larger buffer: data_ptr() is 4 mod 16, which the dispatch of
    pgdvs_gnt_gather answers with the thread-per-item kernel"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _gather(g, n_rays=None, misalign=False):
    """the item through ops.gnt_gather, by the route that produced its record"""
    V, C = int(g["V"]), int(g["C"])
    R = g["ray_o"].shape[0] if n_rays is None else n_rays
    feat = T(g["featmaps"][:V, :C]).permute(0, 2, 3, 1).contiguous()
    if misalign:
        feat = _misaligned(feat)
    if str(g["route"]) == "z_in":  # the fine pass's call: explicit depths next to the record's own range
        dr, iu, zs = T(g["depth_range"]), False, T(g["z_in"][:R])
    else:
        dr, iu, zs = T(g["depth_range"]), bool(g["inv_uniform"]), None
    if dr.shape[0] != 1:
        dr = dr[:R].contiguous()
    return ops.gnt_gather(T(g["ray_o"][:R]), T(g["ray_d"][:R]), dr, int(g["S"]), iu, ops.cam_prep(T(g["cam_tgt"])),
                          ops.cam_prep(T(g["cams_src"][:V])), T(g["src_rgbs"][:V]), feat,
                          T(g["inv_masks"][:V, ..., 0]) if bool(g["use_mask"]) else None, z_samples=zs)


def _ulp(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("case,item", GATHER_ITEMS, ids=[f"{c}-{i}" for c, i in GATHER_ITEMS])
def test_gnt_gather_edges(golden_dir, case, item):
    gc = _case(golden_dir, case)
    g = _item(gc, item)
    out = {k: N(v) for k, v in _gather(g).items()}
    items = [_item(gc, str(i)) for i in gc["items"]]
    err_ref = {k: max(float(i["err_" + k]) for i in items) for k in TOL}  # the reference's own float32 error, per case
    mag = {k: max(float(i["mag_" + k]) for i in items) for k in TOL}
    # the decisions: equal to the reference's on every item
    for k in ("mask_inbound", "mask_invalid", "mask"):
        bad = np.argwhere(out[k] != g["out_" + k])
        assert bad.shape[0] == 0, (k, bad.shape[0], bad[:8].tolist())
    for k, (rtol, atol) in TOL.items():
        # 1. against the reference's float32 outputs, at the tolerances of test_gnt_gather_vs_reference_and_oracle
        err32 = float(np.abs(out[k] - g["out_" + k]).max())
        # 2. against its float64 outputs: at most 4 x the reference's own float32 error of the case, floor one ulp
        err64 = float(np.abs(out[k].astype(np.float64) - g["out64_" + k]).max())
        bound = max(4.0 * err_ref[k], _ulp(mag[k]))
        print(f"{case}-{item} {k}: |gpu-ref32| {err32:.3e}  |gpu-ref64| {err64:.3e}  bound {bound:.3e}  (ref32-ref64 {err_ref[k]:.3e})")
        np.testing.assert_allclose(out[k], g["out_" + k], rtol=rtol, atol=atol, err_msg=k)
        assert err64 <= bound, (k, err64, bound)


@pytest.mark.parametrize("case,item", [("bounds", "mask1"), ("depth", "mask1"), ("mask", "mask1"), ("sizes", "c32_v3_perray_uniform"),
                                       ("sizes", "c64_v7_perview_inverse")])
def test_gnt_gather_both_kernels_bit_identical(golden_dir, case, item):
    """the eight-lanes-per-item kernel and the thread-per-item kernel share gather_item and the accumulation order"""
    g = _item(_case(golden_dir, case), item)
    a, b = _gather(g), _gather(g, misalign=True)
    for k in OUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.parametrize("item", ["c32_v3_perray_uniform", "c64_v7_perview_inverse", "c30_v1_fine", "c68_v3_perray_inverse"])
@pytest.mark.parametrize("misalign", [False, True])
def test_gnt_gather_prefix_and_determinism(golden_dir, item, misalign):
    """a prefix of the rays gives exactly the prefix of the full result (item counts off the 8 items a wavefront owns,
    per-ray ranges and explicit depths sliced with the rays), and two runs are bit-identical"""
    g = _item(_case(golden_dir, "sizes"), item)
    full, again = _gather(g, misalign=misalign), _gather(g, misalign=misalign)
    for k in OUTS:
        assert torch.equal(full[k].view(torch.int32), again[k].view(torch.int32)), k
    for n in (1, 5, 12):
        part = _gather(g, n_rays=n, misalign=misalign)
        assert n == 1 or part["mask"].numel() % 8 != 0
        for k in OUTS:
            assert torch.equal(part[k].view(torch.int32), full[k][:n].view(torch.int32)), (k, n)


@pytest.mark.parametrize("name", COARSE)
def test_gnt_gather_sampling_edges(golden_dir, name):
    """the ray sampling fused into the gather: both values of inv_uniform, per-view and per-ray ranges over two orders of
    magnitude (some far barely above near), S = 2, 3, 64"""
    g = _case(golden_dir, "sampling")
    rk, iu, S = name.split("_")[1], int(name.split("_")[2][2:]), int(name.split("_")[3][1:])
    rng = np.random.default_rng(5)
    cam = np.concatenate(([8, 8], np.diag([8.0, 8.0, 1.0, 1.0]).flatten(), np.eye(4).flatten())).astype(np.float32)
    out = ops.gnt_gather(T(g["ray_o"]), T(g["ray_d"]), T(g["range_" + rk]), S, bool(iu), ops.cam_prep(T(cam)), ops.cam_prep(T(cam[None])),
                         T(rng.random((1, 8, 8, 3), dtype=np.float32)), T(rng.random((1, 3, 5, 32), dtype=np.float32)))
    for k in ("z_vals", "pts"):
        np.testing.assert_allclose(N(out[k]), g[f"{name}__{k}"], rtol=1e-6, atol=1e-6, err_msg=k)
        err64 = float(np.abs(N(out[k]).astype(np.float64) - g[f"{name}__{k}64"]).max())
        bound = max(4.0 * float(g[f"{name}__err_{k}"]), _ulp(np.abs(g[f"{name}__{k}64"]).max()))
        print(f"{name} {k}: |gpu-ref64| {err64:.3e}  bound {bound:.3e}")
        assert err64 <= bound, (k, err64, bound)


@pytest.mark.parametrize("name", FINE)
def test_sample_fine_z_edges(golden_dir, name):
    """the importance re-sampling on the GPU: all-zero, one-hot and dominant-bin weight rows (the denom < 1e-5 branch and
    the u == cdf ties of sample_pdf), both values of inv_uniform"""
    g = _case(golden_dir, "sampling")
    iu = int(g[name + "__inv_uniform"])
    z_all = sample_fine_z(bool(iu), int(g[name + "__n_fine"]), True, T(g[f"fine_weights_iu{iu}"]).clone(), T(g[name + "__z_coarse"]))
    np.testing.assert_allclose(N(z_all), g[name + "__z_all"], rtol=1e-6, atol=0)
    # and through the gather by the route of the fine pass: explicit depths, the record's range
    cam = np.concatenate(([8, 8], np.diag([8.0, 8.0, 1.0, 1.0]).flatten(), np.eye(4).flatten())).astype(np.float32)
    rng = np.random.default_rng(5)
    out = ops.gnt_gather(T(g["ray_o"]), T(g["ray_d"]), T(g["range_" + str(g[name + "__range"])]), z_all.shape[1], False,
                         ops.cam_prep(T(cam)), ops.cam_prep(T(cam[None])), T(rng.random((1, 8, 8, 3), dtype=np.float32)),
                         T(rng.random((1, 3, 5, 32), dtype=np.float32)), z_samples=z_all)
    assert torch.equal(out["z_vals"], z_all)
    np.testing.assert_allclose(N(out["pts"]), g[name + "__pts"], rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------- BaseRenderer.forward, per-ray ranges across batch items
def _render_model(golden_dir):
    from test_gpu_parity import _gnt_model

    from pgdvs_amd.models.gnt.renderer import BaseRenderer

    m, _ = _gnt_model(golden_dir)
    br = BaseRenderer(model_cfg=None)
    br.model = m
    return br.to(DEV).eval()


def _check_render(g, tag, ret):
    keys = E.render_keys(g, tag)
    assert (ret["outputs_fine"] is None) == (int(g[tag + "__n_fine"]) == 0)
    for pre, k in keys:
        out = ret["outputs_fine" if pre == "fine_" else "outputs_coarse"][k]
        ref = g[f"{tag}__{pre}{k}"]
        assert tuple(out.shape) == ref.shape, (pre, k)
        err = float(np.abs(N(out) - ref).max())
        print(f"render {tag} {pre}{k}: |gpu-ref32| {err:.3e}  |gpu-ref64| {float(np.abs(N(out) - g[f'{tag}__{pre}{k}_64']).max()):.3e}")
        np.testing.assert_allclose(N(out), ref, rtol=0, atol=RENDER_TOL[pre], err_msg=pre + k)


def _forward(br, g, tag, ray_batch):
    with torch.no_grad():
        return br.forward(ray_batch=ray_batch, chunk_size=int(g[tag + "__chunk_size"]), inv_uniform=bool(g[tag + "__inv_uniform"]),
                          n_coarse_samples_per_ray=int(g["Ss"]), n_fine_samples_per_ray=int(g[tag + "__n_fine"]), use_dyn_mask=True,
                          flag_deterministic=True, render_stride=int(g["render_stride"]), ret_view_entropy=True, ret_view_std=True)


@pytest.mark.parametrize("merge", [None, 0], ids=["merge_default", "merge_0"])
@pytest.mark.parametrize("tag", RENDER)
def test_gnt_renderer_per_ray_ranges(golden_dir, tag, merge):
    """B = 2, render_stride 2, ranges [B rh rw, 2], dynamic masks, chunks that straddle the two batch items: the mirror
    BaseRenderer.forward with chunks merged (the default) and executed as given"""
    g = _case(golden_dir, "render")
    br = _render_model(golden_dir)
    if merge is not None:
        br.merge_chunks_up_to = merge
    else:
        assert br.merge_chunks_up_to >= 2 * int(g[tag + "__chunk_size"])  # the default merges these chunks
    s = int(g["render_stride"])
    per_ray = np.ascontiguousarray(g["depth_range_map"][:, ::s, ::s].reshape(-1, 2))
    ray_batch = {"ray_o": T(g["ray_o"]), "ray_d": T(g["ray_d"]), "camera": T(g["cam_tgt"]), "raw_h": int(g["H"]), "raw_w": int(g["W"]),
                 "depth_range": T(per_ray), "depth_range_per_ray": True, "src_rgbs": T(g["src_rgbs"]),
                 "src_invalid_masks": T(g["inv_masks"]), "src_cameras": T(g["cams_src"])}
    _check_render(g, tag, _forward(br, g, tag, ray_batch))


@pytest.mark.parametrize("tag", RENDER)
def test_gnt_renderer_through_prepare_ray_batch(golden_dir, tag):
    """the same records with the ray batch made by PGDVSRenderer.prepare_ray_batch from a 4-d depth_range: its strided
    per-ray slicing and its rays are what feed the renderer"""
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    g = _case(golden_dir, "render")
    cfg = load_config(static_renderer="gnt")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.gnt_use_masked_spatial_src = False
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    model.static_renderer = _render_model(golden_dir)
    B, H, W, s = int(g["B"]), int(g["H"]), int(g["W"]), int(g["render_stride"])
    data = {"flat_cam_tgt": T(g["cam_tgt"]), "rgb_src_temporal": T(g["src_rgbs"][:, :2]), "rgb_src_spatial": T(g["src_rgbs"]),
            "dyn_mask_src_spatial": T(g["inv_masks"]), "flat_cam_src_spatial": T(g["cams_src"]), "depth_range": T(g["depth_range_map"])}
    assert data["depth_range"].ndim == 4
    rb = model.prepare_ray_batch(data=data, B=B, H=H, W=W, render_stride=s, render_cfg=rc)
    assert rb["depth_range_per_ray"] and tuple(rb["depth_range"].shape) == (g["ray_o"].shape[0], 2)
    np.testing.assert_allclose(N(rb["ray_d"]), g["ray_d"], rtol=1e-5, atol=1e-5)
    _check_render(g, tag, _forward(model.static_renderer, g, tag, rb))


# ---------------------------------------------------------------- one sweep at the size the product runs
@pytest.mark.parametrize("inv_uniform", [False, True])
def test_gnt_gather_sweep_at_product_size(inv_uniform):
    """288 x 550 image, V = 10, 72 x 138 x 32 feature map, 4 096 rays x 64 samples, per-ray ranges, against the oracle
    that test_oracle_gnt_edges.py pins: floats within the oracle tolerance (atol 2e-5; pts and z_vals at theirs), masks
    equal on every item outside the exempt set, which holds at most 1e-4 of the items"""
    x = E.sweep_inputs()
    o = E.sweep_oracle(x, inv_uniform)
    out = ops.gnt_gather(T(x["ray_o"]), T(x["ray_d"]), T(x["depth_range"]), E.SWEEP["S"], inv_uniform, ops.cam_prep(T(x["cam_tgt"])),
                         ops.cam_prep(T(x["cams_src"])), T(x["src_rgbs"]), T(x["featmaps"]).permute(0, 2, 3, 1).contiguous(),
                         T(x["inv_masks"][..., 0]))
    out = {k: N(v) for k, v in out.items()}
    exempt = o["exempt"]
    share = float(exempt.mean())
    assert share <= 1e-4, share
    for k in ("mask_inbound", "mask_invalid", "mask"):
        diff = out[k] != o[k]
        print(f"sweep iu={int(inv_uniform)} {k}: {int(diff.sum())} items differ, {int((diff & ~exempt).sum())} outside the exempt set ({share:.2e})")
        assert not np.any(diff & ~exempt), (k, np.argwhere(diff & ~exempt)[:8].tolist())
    np.testing.assert_allclose(out["pts"], o["pts"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out["z_vals"], o["z_vals"], rtol=1e-6, atol=1e-6)
    keep = ~(out["mask_inbound"] != o["mask_inbound"])  # (an exempt item on the other side of a bound samples another pixel)
    for k in ("rgb_feat", "ray_diff"):
        err = np.abs(out[k] - o[k])
        print(f"sweep iu={int(inv_uniform)} {k}: max |gpu-oracle| {float(err.max()):.3e}")
        assert float((err * keep).max()) <= 2e-5, k
