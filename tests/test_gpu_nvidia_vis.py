"""The NVIDIA-family depth range on the MI355X (csrc/depth_range.hip, DESIGN.md 8f-3 NVIDIA): bit-identical to the numpy
path (float32 depth_range and float64 near / far) on the visualisation fixture tree, on 288 x 550 scenes of 10 and 24
views and on adversarial inputs; the three loaders' device paths item for item against their numpy paths; and an
nvidia_vis item through PGDVSRenderer.forward (GNT static renderer, softsplat dynamic branch)."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def vis_tree(tmp_path_factory):
    return VT.build_tree(tmp_path_factory.mktemp("nvidia_vis"))


def _vis(root, device):
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    return NvidiaDynVisualizationDataset(data_root=root, device=device, **VT.KW)


def _both(depths, Ks, c2ws, c2w_tgt):
    """(numpy float64 pair, numpy float32 range) of the loaders' host path and (float64 pair, float32 range) of the op"""
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.nvidia_eval import compute_pcl, depth_range_from_points, ray_constants

    V, H, W = depths.shape
    pcl = np.concatenate([compute_pcl(H, W, K, c, d) for K, c, d in zip(Ks, c2ws, depths)], axis=0)
    want64 = depth_range_from_points(pcl, c2w_tgt)
    rays = np.stack([np.concatenate([M.reshape(-1), o]) for M, o in (ray_constants(K, c) for K, c in zip(Ks, c2ws))])
    nf = torch.zeros(2, dtype=torch.float64, device=DEV)
    got = ops.nvidia_depth_range(torch.from_numpy(np.ascontiguousarray(depths, np.float32)).to(DEV),
                                 torch.from_numpy(rays.astype(np.float32)).to(DEV), np.linalg.inv(c2w_tgt), near_far=nf)
    torch.cuda.synchronize()
    return want64, want64.astype(np.float32), nf.cpu().numpy(), got.cpu().numpy()


def _check(depths, Ks, c2ws, c2w_tgt, what):
    want64, want32, got64, got32 = _both(depths, Ks, c2ws, c2w_tgt)
    assert np.array_equal(got64.view(np.uint64), want64.view(np.uint64)), (what, got64, want64)
    assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32)), (what, got32, want32)
    return want64


def test_fixture_tree_every_item_vs_numpy_and_reference(vis_tree, golden_dir):
    g = dict(np.load(golden_dir / "nvidia_vis_items.npz"))
    ds = _vis(vis_tree, None)
    for i in range(len(ds)):
        _, _, _, _, tgt_c2w, _ = ds.valid_fs[i]
        item = ds[i]
        spatial = sorted(set(item["seq_ids"][1:1 + VT.KW["n_src_views_spatial"]].tolist()))
        all_c2w, all_hwf = ds.c2w_dict[VT.SCENE], ds.hwf_dict[VT.SCENE]
        views = ds._stack_views(VT.SCENE, spatial, all_c2w, all_hwf, (NT.H, NT.W))
        _check(views["depth"], views["K"], views["c2w"], ds._aug_c2w(tgt_c2w), i)
        dev = _vis(vis_tree, DEV)[i]["depth_range"]
        assert np.array_equal(dev.numpy().view(np.uint32), item["depth_range"].numpy().view(np.uint32)), i
        if i in VT.ITEMS:
            n = VT.ITEMS.index(i)
            assert np.array_equal(dev.numpy().view(np.uint32), g[f"i{n}_depth_range"].view(np.uint32)), i


def _scene(V, H, W, seed):
    """V cameras along a short arc and a dolly looking at a wavy surface (DynIBaR-like disparities), the target between
    them and slightly turned"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    disp = np.stack([1.0 / (2.0 + 0.5 * np.sin(xx / 37.0 + v) + 0.3 * np.cos(yy / 23.0)) + 0.02 * rng.random((H, W))
                     for v in range(V)]).astype(np.float32)
    depths = 1 / (disp + 1e-8)
    Ks, c2ws = [], []
    for v in range(V):
        K = np.eye(4)
        K[:3, :3] = [[0.9 * W + v, 0, W / 2.0], [0, 0.9 * W + v, H / 2.0], [0, 0, 1]]
        Ks.append(K)
        c2ws.append(NT.opencv_c2w(v))
    tgt = NT.opencv_c2w(3) @ np.linalg.inv(np.array([[1, 0, 0, 0.013], [0, 1, 0, -0.007], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    return depths, np.stack(Ks), np.stack(c2ws), np.linalg.inv(np.linalg.inv(tgt))


@pytest.mark.parametrize("V", [10, 24])
def test_nvidia_size_scenes_vs_numpy(V):
    depths, Ks, c2ws, tgt = _scene(V, 288, 550, V)
    want = _check(depths, Ks, c2ws, tgt, V)
    assert 1e-16 < want[0] < want[1]


def _flat(z_views, c2w_tgt=None):
    """views whose points are (u d, v d, d) in an identity world: K = I, c2w = I, so z = depth in an identity target"""
    V = len(z_views)
    eye = np.stack([np.eye(4)] * V)
    return _check(np.stack(z_views).astype(np.float32), eye, eye, np.eye(4) if c2w_tgt is None else c2w_tgt, "flat")


def test_adversarial_inputs_vs_numpy():
    from pgdvs_amd.ops import PgdvsHipError

    rng = np.random.default_rng(11)
    _flat([np.full((4, 9), 0.7, np.float32)])                                       # all-equal z
    ties = np.concatenate([np.full(40, 1.5), np.full(41, 2.5), rng.uniform(0, 5, 19)])
    _flat([rng.permutation(ties).reshape(10, 10)])                                  # ties at the quantile's two ranks
    v = _flat([rng.uniform(0.5, 3, (1, 11)).astype(np.float32)])                    # n - 1 = 10: integral virtual index 9
    assert v[1] > 2e-16
    _flat([-rng.exponential(3, (7, 13))])                                           # negative z: near clamps
    zs = rng.permutation(np.concatenate([np.zeros(30), -np.zeros(30), rng.normal(size=6)])).reshape(6, 11)
    _flat([zs])                                                                     # +-0.0
    for bad in (np.inf, -np.inf, np.nan):
        d = rng.uniform(1, 2, (5, 8)).astype(np.float32)
        d[2, 3] = bad
        d[4, 0] = bad
        got = _flat([d, rng.uniform(1, 2, (5, 8))])                                 # infinite / NaN depths
        if bad != bad:
            assert got.tolist() == [1e-16, 2e-16]
    inf_disp = np.full((3, 4), -1e-8, np.float32)                                   # disparity exactly -1e-8: depth inf
    _flat([1 / (inf_disp + 1e-8), rng.uniform(1, 2, (3, 4))])
    # a general camera with inf depths: points with a zero ray component become NaN
    depths, Ks, c2ws, tgt = _scene(3, 20, 30, 4)
    depths[1, :3, :5] = np.inf
    _check(depths, Ks, c2ws, tgt, "inf general")
    # the documented rejection: one-pixel views (numpy's matrix-vector order)
    from pgdvs_amd import ops

    for shape in ((1, 1, 1), (3, 1, 1)):
        with pytest.raises(PgdvsHipError):
            ops.nvidia_depth_range(torch.ones(shape, device=DEV), torch.zeros(shape[0], 12, device=DEV), np.eye(4))


def _assert_items_equal(x, y, what):
    assert x.keys() == y.keys() and x["misc"] == y["misc"] and x["scene_id"] == y["scene_id"], what
    for k in x:
        if isinstance(x[k], torch.Tensor):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (what, k)
            assert np.array_equal(x[k].numpy().view(np.uint8), y[k].numpy().view(np.uint8)), (what, k)


def test_loader_paths_agree_key_for_key(vis_tree, tmp_path):
    from pgdvs_amd.datasets.mono_vis import MonoVisualizationDataset
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    a, b = _vis(vis_tree, None), _vis(vis_tree, DEV)
    for i in range(len(a)):
        _assert_items_equal(a[i], b[i], ("nvidia_vis", i))
    root = NT.build_tree(tmp_path / "eval")
    kw = dict(data_root=root, raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows",
              max_hw=-1, mode="eval", scene_ids=[NT.SCENE], n_src_views_spatial=4, n_src_views_temporal_track_one_side=2)
    a, b = NvidiaDynEvaluationDataset(**kw), NvidiaDynEvaluationDataset(device=DEV, **kw)
    for i in range(0, len(a), 7):
        _assert_items_equal(a[i], b[i], ("nvidia_eval", i))
    root = NT.build_mono_tree(tmp_path / "mono")
    kw = dict(data_root=root, max_hw=-1, mode="vis", scene_ids=[NT.MONO_SCENE], n_src_views_spatial=3,
              n_src_views_temporal_track_one_side=2, vis_center_time=4, n_render_frames=16, vis_time_interval=3, vis_bt_max_disp=8)
    a, b = MonoVisualizationDataset(**kw), MonoVisualizationDataset(device=DEV, **kw)
    for i in range(len(a)):
        _assert_items_equal(a[i], b[i], ("mono_vis", i))


def test_nvidia_vis_item_through_renderer(vis_tree):
    """an nvidia_vis item (either path) -> PGDVSRenderer.forward with a seeded random-init GNT static renderer and the
    softsplat dynamic branch, as the visualiser config sets them: finite; the static branch bit-identical for the two
    paths' items.  The splat accumulates with float atomics, so two forwards of one item differ in the last bits there:
    with the splat noise fixed, every output agrees within that run-to-run spread"""
    from pgdvs_amd.harness import to_device
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    torch.manual_seed(0)
    cfg = load_config(engine="visualizer_pgdvs")
    assert cfg.static_renderer._target_ == "pgdvs_amd.models.gnt.renderer.BaseRenderer"
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    assert rc.dyn_render_type == "softsplat"
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False

    def render(device):
        item = _vis(vis_tree, device)[10]
        batch = {k: (v[None] if isinstance(v, torch.Tensor) else v) for k, v in item.items()}
        batch["misc"], batch["scene_id"] = [item["misc"]], [item["scene_id"]]
        batch["static_noise"] = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, NT.H, NT.W)).astype(np.float32))
        with torch.no_grad():
            ret = model.forward(to_device(batch, DEV), render_cfg=rc)
        torch.cuda.synchronize()
        return ret

    render(None)  # warm-up: the library picks its convolution algorithms on the first call
    outs = [render(None), render(DEV), render(None)]
    rgb = outs[0]["combined_rgb"]
    assert rgb.shape[-3:-1] == (NT.H, NT.W) or rgb.shape[-2:] == (NT.H, NT.W), rgb.shape
    assert torch.isfinite(rgb).all()
    for k, v in outs[0].items():
        if isinstance(v, torch.Tensor):
            d01 = (v.double() - outs[1][k].double()).abs().max().item()
            d02 = (v.double() - outs[2][k].double()).abs().max().item()
            if k.startswith("static"):
                assert torch.equal(v, outs[1][k]), (k, d01, d02)
            assert d01 <= 1e-6 and d02 <= 1e-6, (k, d01, d02)
