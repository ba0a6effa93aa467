"""The NVIDIA visualisation loader (datasets/nvidia_vis.py) against the reference's own output on a synthetic tree
(tests/golden/make_golden_nvidia_vis.py), its place in the config surface, its argument checks, and the host-side
contract of the NVIDIA-family depth-range op (csrc/depth_range.hip): the library exports it, its workspace query rejects
the documented shapes, and numpy's float32 unprojection at the NVIDIA size follows the order the op follows."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return VT.build_tree(tmp_path_factory.mktemp("nvidia_vis"))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "nvidia_vis_items.npz"))


def _dataset(root, **kw):
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    args = dict(VT.KW)
    args.update(kw)
    return NvidiaDynVisualizationDataset(data_root=root, **args)


def _digest(a):
    a = np.asarray(a, np.float64).reshape(-1)
    w = np.random.default_rng(12345).random(a.size)
    return np.array([a @ w, a.sum(), a.min(), a.max()])


def test_camera_path_matches_reference(tree, golden):
    ds = _dataset(tree)
    assert len(ds) == int(golden["n_items"]) == VT.KW["n_render_frames"]
    c2w = np.stack([e[4] for e in ds.valid_fs])
    assert np.array_equal(c2w.view(np.uint64), golden["all_tgt_c2w"].view(np.uint64))
    assert np.array_equal(np.array([e[2] for e in ds.valid_fs]), golden["all_tgt_time"])
    assert [e[3] for e in ds.valid_fs] == golden["all_tgt_idx"].tolist()
    assert golden["all_tgt_time"][0] == 0.0 and golden["all_tgt_time"][-1] == NT.F - 2


@pytest.mark.parametrize("n", range(len(VT.ITEMS)))
def test_items_match_reference(tree, golden, n):
    """every key of the recorded items, bit for bit (digests for the bulky arrays), depth_range and the track windows
    of t = 0 and of the last time included"""
    ds = _dataset(tree)
    item = ds[VT.ITEMS[n]]
    assert sorted(item.keys()) == golden[f"i{n}_keys"].tolist()
    assert item["scene_id"] == item["misc"]["scene_id"] == VT.SCENE
    assert [item["misc"]["tgt_time"], item["misc"]["tgt_idx"]] == golden[f"i{n}_misc"].tolist()
    checked = 0
    for k, v in item.items():
        if k in ("scene_id", "misc"):
            continue
        v = v.numpy()
        if k.startswith("dyn_rgb") or k.startswith("static_rgb"):
            sfx = k.split("_rgb_", 1)[1]
            rgb, m = item[f"rgb_{sfx}"].numpy(), item[f"dyn_mask_{sfx}"].numpy()
            want = rgb * m if k.startswith("dyn") else rgb * (1 - m)
            assert np.array_equal(v, want), k
            continue
        if k.startswith("rgb_"):
            v = np.round(v * 255.0).astype(np.uint8)
        elif "mask" in k:
            v = v.astype(np.uint8)
        if f"i{n}_{k}__digest" in golden:
            assert tuple(v.shape) == tuple(golden[f"i{n}_{k}__shape"]), k
            assert np.array_equal(_digest(v), golden[f"i{n}_{k}__digest"]), k
        else:
            g = golden[f"i{n}_{k}"]
            assert v.dtype == g.dtype and v.shape == g.shape, (k, v.dtype, g.dtype, v.shape, g.shape)
            assert np.array_equal(v.view(np.uint8), g.view(np.uint8)), k
        checked += 1
    assert checked >= 25 and "depth_range" in item
    if n == 0:  # t = 0: no older frame; the newer window starts at the newer frame and is one longer
        assert item["n_actual_temporal"].item() == 2 and item["time_src_temporal"].tolist() == [1.0, 1.0]
        assert item["n_actual_temporal_track_fwd2tgt"].item() == 0
        assert item["time_src_temporal_track_bwd2tgt"].tolist() == [1.0, 2.0, 3.0]


def test_dataset_class_and_visualiser_config_without_reference(tree, monkeypatch):
    """the visualiser config's default dataset list resolves to the mirror, and instantiates and indexes with the
    reference package un-importable"""
    from pgdvs_amd.datasets.combined import CombinedDataset, dataset_class
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset
    from pgdvs_amd.instantiate import instantiate, load_config

    monkeypatch.setitem(sys.modules, "pgdvs", None)  # `import pgdvs...` raises ImportError
    assert dataset_class("nvidia_vis") is NvidiaDynVisualizationDataset
    ds_cfg = load_config(engine="visualizer_pgdvs").dataset
    assert list(ds_cfg.dataset_list.vis) == ["nvidia_vis"]
    spec = dict(ds_cfg.dataset_specifics.nvidia_vis)
    spec.update(scene_ids=[VT.SCENE], raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows",
                n_src_views_spatial=4, n_render_frames=16, vis_center_time=6, vis_time_interval=8)
    node = dict(ds_cfg)
    node.update(data_root=str(tree), dataset_specifics={"nvidia_vis": spec})
    ds = instantiate(node, mode="vis")
    assert isinstance(ds, CombinedDataset) and len(ds) == 16
    assert isinstance(ds.datasets["nvidia_vis"], NvidiaDynVisualizationDataset)
    item = ds[15]
    assert item["misc"]["tgt_idx"] == 15 and item["depth_range"].shape == (2,)
    assert torch.equal(item["depth_range"], ds.datasets["nvidia_vis"][15]["depth_range"])


def test_constructor_rejects_unsupported_settings(tree):
    with pytest.raises(AssertionError):
        _dataset(tree, mode="eval")
    with pytest.raises(AssertionError):
        _dataset(tree, max_hw=512)
    with pytest.raises(NotImplementedError):
        _dataset(tree, use_zoe_depth="moe", zoe_depth_data_f="zoe.zip")


def test_device_path_refuses_dataloader_workers(tree):
    """all three NVIDIA-family loaders: a forked DataLoader worker must not touch the GPU, so the device path raises
    there (before any GPU call), naming the setting to use"""
    from pgdvs_amd.datasets.mono_vis import MonoVisualizationDataset
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    eval_root = NT.build_tree(pathlib.Path(tree).parent / "eval_tree")
    mono_root = NT.build_mono_tree(pathlib.Path(tree).parent / "mono_tree")
    kw = dict(raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1, mode="eval",
              scene_ids=[NT.SCENE], n_src_views_spatial=4, n_src_views_temporal_track_one_side=2)
    loaders = [_dataset(tree, device="cuda"), NvidiaDynEvaluationDataset(data_root=eval_root, device="cuda", **kw),
               MonoVisualizationDataset(data_root=mono_root, max_hw=-1, mode="vis", scene_ids=[NT.MONO_SCENE], n_src_views_spatial=3,
                                        n_src_views_temporal_track_one_side=2, vis_center_time=4, n_render_frames=16,
                                        vis_time_interval=3, vis_bt_max_disp=8, device="cuda")]
    for ds in loaders:
        dl = torch.utils.data.DataLoader(ds, batch_size=None, num_workers=1)
        with pytest.raises(RuntimeError, match="n_dataloader_workers=0"):
            next(iter(dl))


def test_library_exports_nvidia_depth_range():
    from pgdvs_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "pgdvs_nvidia_depth_range") and hasattr(lib, "pgdvs_nvidia_depth_range_workspace_bytes")
    ws = lib.pgdvs_nvidia_depth_range_workspace_bytes(10, 288, 550)
    assert ws >= 10 * 288 * 550 * 8
    assert lib.pgdvs_nvidia_depth_range_workspace_bytes(2, 1, 2) > 0
    for bad in ((0, 288, 550), (1, 0, 5), (3, 1, 1), (1, 1, 1), (2, 1 << 15, 1 << 15), (-1, 4, 4)):
        assert lib.pgdvs_nvidia_depth_range_workspace_bytes(*bad) == -1, bad  # PGDVS_ERR_INVALID


def test_numpy_unprojection_order_at_nvidia_size():
    """compute_pcl's float32 `M @ pix` over a 288 x 550 view (the size the loaders run at, column tails included) is
    a0 x0, then fma(a_k, x_k, acc) for k ascending, and the point o + d depth is a rounded multiply then a rounded add:
    the order pgdvs_nvidia_depth_range follows"""
    from fractions import Fraction

    from pgdvs_amd.datasets.nvidia_eval import compute_pcl, ray_constants

    h, w = 288, 550
    rng = np.random.default_rng(5)
    c2w = np.eye(4)
    c2w[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    c2w[:3, 3] = rng.normal(size=3)
    K = np.eye(4)
    K[:3, :3] = [[0.9 * w + 0.3, 0, w / 2.0], [0, 0.9 * w + 0.3, h / 2.0], [0, 0, 1]]
    depth = (1.0 / (0.3 + rng.random((h, w)))).astype(np.float32)
    pcl = compute_pcl(h, w, K, c2w, depth)
    M, o = ray_constants(K, c2w)
    f32 = np.float32
    idx = np.unique(np.concatenate([np.arange(40), h * w - 1 - np.arange(40), rng.integers(0, h * w, 300)]))
    for i in idx:
        u, v = f32(i % w), f32(i // w)
        for ax in range(3):
            acc = f32(M[ax, 0] * u)
            acc = f32(Fraction(float(M[ax, 1])) * Fraction(float(v)) + Fraction(float(acc)))
            acc = f32(acc + M[ax, 2])
            x = f32(o[ax] + f32(acc * depth.reshape(-1)[i]))
            assert pcl[i, ax].view(np.uint32) == x.view(np.uint32), (i, ax)
