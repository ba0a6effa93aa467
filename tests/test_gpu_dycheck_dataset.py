"""The DyCheck loader's depth range on the MI355X (csrc/depth_range.hip, DESIGN.md 8f-3 DyCheck): bit-identical to the
numpy path on every fixture item and on a 10 x 360 x 480 scene (many points per pixel, points behind the camera, hits on the
last row / column), the quantile stage exact against np.quantile on adversarial sets, the loader's two paths key for key,
and a DyCheck item through the HIP renderer (GNT static branch) and eval_step(quant_type="dycheck_iphone")."""
import math
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
          scene_ids=[DT.SCENE], n_src_views_spatial=3, n_src_views_spatial_cluster=4, n_src_views_temporal_track_one_side=2,
          flow_consist_thres=1.0)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DT.build_tree(tmp_path_factory.mktemp("dycheck"))


def _dataset(root, typ, device):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    return DyCheckiPhoneEvaluationDataset(data_root=root, spatial_src_view_type=typ, device=device, **KW)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


@pytest.mark.parametrize("typ", ["closest_wo_temporal", "clustered"])
def test_depth_range_fixture_items_vs_numpy(golden_dir, tree, typ):
    """the device path returns the reference's depth_range bit for bit on every fixture item (the numpy path does too:
    tests/test_dycheck_dataset_host.py)"""
    g = dict(np.load(golden_dir / "dycheck_items.npz"))
    ds = _dataset(tree, typ, DEV)
    raising = set(g[f"{typ}_raising"].tolist())
    n = 0
    for i in range(len(ds)):
        if i in raising:
            continue
        dr = ds[i]["depth_range"]
        assert dr.dtype == torch.float32 and dr.device.type == "cpu"
        assert np.array_equal(_bits(dr), g[f"{typ}_i{i}_depth_range"].view(np.uint32)), (typ, i)
        n += 1
    assert n >= 4


def _scene(V, H, W, seed, depth_dtype=np.float32):
    """V source cameras along a short arc looking at a wavy surface; the target is source 0's camera (even seeds) or one
    turned and moved into the surface (odd seeds); returns the inputs of both paths"""
    from pgdvs_amd.datasets.dycheck_iphone import ray_constants

    rng = np.random.default_rng(seed)
    K3 = np.array([[0.9 * W, 1.3, W / 2 + 0.3], [0, 0.93 * W, H / 2 - 0.2], [0, 0, 1]], np.float32)
    K4 = np.eye(4)
    K4[:3, :3] = K3

    def pose(a, t):
        c, s = np.cos(a), np.sin(a)
        w2c = np.eye(4, dtype=np.float32)
        w2c[:3, :3] = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], np.float32)
        w2c[:3, 3] = t
        return w2c

    c2ws = [np.linalg.inv(np.linalg.inv(np.linalg.inv(pose(0.02 * v - 0.1, np.array([0.05 * v, 0.01 * v, 0], np.float32)))))
            for v in range(V)]
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([(2.0 + 0.5 * np.sin(xx / 17.0 + v) + 0.2 * rng.random((H, W))) for v in range(V)]).astype(depth_dtype)
    dyn = (rng.random((V, H, W)) < 0.3).astype(np.float32)
    if seed % 2:  # turned and moved into the surface: part of the cloud lies behind the target
        R = pose(0.3, np.zeros(3, np.float32))[:3, :3]
        raw_c2w_tgt = np.linalg.inv(pose(0.3, (-R @ np.array([0.2, 0.0, 2.2])).astype(np.float32)))
    else:  # source 0's camera: its last column / row reproject onto W - 1 / H - 1
        raw_c2w_tgt = np.linalg.inv(pose(-0.1, np.zeros(3, np.float32)))
    c2w_tgt = np.linalg.inv(np.linalg.inv(raw_c2w_tgt))
    flat_cam_tgt = np.concatenate(([H, W], K4.flatten(), c2w_tgt.flatten())).astype(np.float32)
    rays = [ray_constants(K4, c) for c in c2ws]
    return dict(depth=depth, dyn=dyn, rays=rays, raw_c2w_tgt=raw_c2w_tgt, flat_cam_tgt=flat_cam_tgt, K3=K3)


def _both(s, near, far):
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.dycheck_iphone import compute_pcl, depth_range_numpy

    V, H, W = s["depth"].shape
    pcl = np.concatenate([compute_pcl(H, W, M, o, d) for (M, o), d in zip(s["rays"], s["depth"])], axis=0)
    want = depth_range_numpy(pcl, s["dyn"], s["raw_c2w_tgt"], s["flat_cam_tgt"], near, far, H, W)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    rays = np.stack([np.concatenate([M.reshape(-1), o]) for M, o in s["rays"]])
    got = ops.dycheck_depth_range(T(s["depth"]), T(s["dyn"]), T(rays), np.linalg.inv(s["raw_c2w_tgt"]),
                                  np.linalg.inv(s["flat_cam_tgt"][18:34].reshape(4, 4)), s["K3"], near, far)
    torch.cuda.synchronize()
    return pcl, want, got.cpu().numpy()


@pytest.mark.parametrize("V,H,W,seed,dt", [(10, 360, 480, 0, np.float32), (10, 360, 480, 1, np.float32),
                                           (3, 60, 80, 2, np.float64), (3, 60, 80, 3, np.float64), (2, 3, 5, 4, np.float32)])
def test_depth_range_synthetic_vs_numpy(V, H, W, seed, dt):
    s = _scene(V, H, W, seed, dt)
    pcl, want, got = _both(s, 0.5, 4.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if V == 10:
        # what the scene exercises: overwritten pixels, many static points per pixel, points behind the camera (seed 1)
        # and exact hits on the last column / row (seed 0: the target is source 0's camera)
        assert np.unique(want[..., 0]).size > 1000
        homo = np.pad(pcl, ((0, 0), (0, 1)), constant_values=1)
        cam = np.matmul(np.linalg.inv(s["flat_cam_tgt"][18:34].reshape(4, 4)), homo.T).T[:, :3]
        pix = np.matmul(s["K3"], cam.T).T
        pix = pix[:, :2] / (pix[:, 2:] + 1e-8)
        st = s["dyn"].reshape(-1) == 0
        if seed == 1:
            assert (cam[st, 2] < 0).sum() > 0
        else:
            assert ((pix[st, 0] == W - 1).sum() > 0) and ((pix[st, 1] == H - 1).sum() > 0)
    # near / far that clamp both ends, and a mask without static points: the constant range
    _, want2, got2 = _both(dict(s, dyn=np.ones_like(s["dyn"])), 2.2, 2.3)
    assert np.array_equal(got2.view(np.uint32), want2.view(np.uint32)) and np.unique(want2[..., 0]).size == 1


def _quantiles(z):
    """the op's quantile stage on z: one view of 1 x n pixels whose points are (0, 0, z) in an identity target camera"""
    from pgdvs_amd import ops

    n = z.size
    rays = torch.tensor([[0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device=DEV)
    q = torch.zeros(2, dtype=torch.float64, device=DEV)
    out = ops.dycheck_depth_range(torch.from_numpy(z.reshape(1, 1, n)).to(DEV), torch.ones(1, 1, n, device=DEV), rays, np.eye(4),
                                  np.eye(4), np.eye(3), -np.inf, np.inf, quantiles=q)
    return q.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_quantile_stage_exact_vs_np_quantile(dt):
    rng = np.random.default_rng(5)
    ties = np.concatenate([np.full(40, 1.5), np.full(41, 2.5), rng.uniform(0, 5, 19)])
    cases = {
        "n1": np.array([3.25]), "n2": np.array([-1.0, 7.0]), "equal": np.full(1000, 0.7), "ties": rng.permutation(ties),
        "negative": -rng.exponential(3, 5001), "signed_zeros": rng.permutation(np.concatenate([np.zeros(30), -np.zeros(30),
                                                                                                rng.normal(size=7)])),
        "wide": rng.permutation(np.concatenate([rng.normal(size=70001) * 10.0 ** rng.integers(-30, 30, 70001)])),
        "close_bits": 1.0 + rng.integers(0, 4096, 100003) * np.finfo(dt).eps,
    }
    for name, z in cases.items():
        z = z.astype(dt)
        q, out = _quantiles(z)
        want = np.array([np.quantile(z, 0.1), np.quantile(z, 0.9)])
        assert np.quantile(z, 0.1).dtype == dt
        assert np.array_equal(q, want.astype(np.float64)), (name, q, want)  # == : -0.0 and +0.0 are equal
        assert np.array_equal(out[0, 0], want.astype(np.float32)), name


def test_loader_paths_agree_key_for_key(tree):
    for typ in ("closest_wo_temporal", "closest_with_temporal", "clustered"):
        a, b = _dataset(tree, typ, None), _dataset(tree, typ, DEV)
        for i in range(len(a)):
            try:
                x = a[i]
            except ValueError:
                with pytest.raises(ValueError):
                    b[i]
                continue
            y = b[i]
            assert x.keys() == y.keys() and x["misc"] == y["misc"] and x["scene_id"] == y["scene_id"]
            for k in x:
                if isinstance(x[k], torch.Tensor):
                    assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), (typ, i, k)


def test_dycheck_item_through_renderer_and_eval_step(tree):
    """a fixture-tree item -> to_device -> PGDVSRenderer (GNT static branch, a small seeded net) ->
    eval_step(quant_type="dycheck_iphone"): every DyCheck key, finite, equal to the torch restatement"""
    import test_dycheck_host as R
    from pgdvs_amd.harness import DYCHECK_KEYS, eval_step, to_device
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    ds = _dataset(tree, "closest_wo_temporal", DEV)
    idx = [i for i, e in enumerate(ds.valid_fs) if (int(e[3]), int(e[2])) == (1, 10)][0]
    item = ds[idx]
    batch = {k: (v[None] if isinstance(v, torch.Tensor) else v) for k, v in item.items()}
    batch["misc"] = [item["misc"]]
    batch["scene_id"] = [item["scene_id"]]
    batch = to_device(batch, DEV)
    torch.manual_seed(0)
    cfg = load_config(static_renderer="gnt")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    md, ex = eval_step(model, batch, rc, device=DEV, quant_type="dycheck_iphone", return_images=True)
    assert set(md) == {"eval/count"} | {f"eval/{k}" for k in DYCHECK_KEYS}
    assert int(md["eval/count"]) == 1
    for k in DYCHECK_KEYS:
        assert math.isfinite(float(md[f"eval/{k}"])), k
    g, p, m = ex["gt"][0].cpu(), ex["pred"][0].cpu(), ex["eval_mask"][0].cpu()
    H, W = g.shape[1:]
    md_t, ex_t = eval_step(R._fake_model(p[None]), {"rgb_src_temporal": torch.zeros(1, 2, H, W, 3), "rgb_tgt": g.permute(1, 2, 0)[None],
                                                    "eval_mask": m.permute(1, 2, 0)[None], "misc": [{}]},
                           "rc", device="cpu", quant_type="dycheck_iphone", return_images=True)
    for k in DYCHECK_KEYS:
        np.testing.assert_allclose(ex["per_view"][k], ex_t["per_view"][k], rtol=0, atol=1e-4, err_msg=k)
