"""DyCheck iPhone loader (DESIGN.md 8f-3 DyCheck), CPU only: the mirror against the reference's own
DyCheckiPhoneEvaluationDataset on the synthetic tree (tests/golden/make_golden_dycheck_items.py), the parser / camera, the
selection rules, the config surface, the DataLoader-worker guard of the device path, and the float orders the numpy path
and the HIP op share."""
import json
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402

TYPES = ["closest_wo_temporal", "closest_with_temporal", "clustered"]
KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
          scene_ids=[DT.SCENE], n_src_views_spatial=3, n_src_views_spatial_cluster=4, n_src_views_temporal_track_one_side=2,
          flow_consist_thres=1.0)


def _digest(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a @ np.random.default_rng(12345).random(a.size), a.sum(), a.min(), a.max()])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DT.build_tree(tmp_path_factory.mktemp("dycheck"))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(golden_dir / "dycheck_items.npz"))


def _dataset(root, typ, **kw):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    return DyCheckiPhoneEvaluationDataset(data_root=root, spatial_src_view_type=typ, **{**KW, **kw})


@pytest.mark.parametrize("typ", TYPES)
def test_dycheck_items_vs_reference(tree, gold, typ):
    """every val item, for each spatial_src_view_type, equals what the reference returned on the same tree: integers and
    depth_range exactly, cameras / times at 1e-6, images by fingerprint; items on which the reference raised raise"""
    ds = _dataset(tree, typ)
    assert [str(e[1]) for e in ds.valid_fs] == gold["valid_fs_names"].tolist()
    assert np.array_equal(np.array([[int(e[2]), int(e[3])] for e in ds.valid_fs]), gold["valid_fs_ids"])
    raising = set(gold[f"{typ}_raising"].tolist())
    assert (len(raising) > 0) == (typ == "clustered")
    for i in range(len(ds)):
        if i in raising:
            with pytest.raises(ValueError, match="RGB image not found"):
                ds[i]
            continue
        item = ds[i]
        e = ds.valid_fs[i]
        assert item["misc"] == {"scene_id": DT.SCENE, "tgt_frame_id": e[2], "tgt_cam_id": e[3], "tgt_frame_name": e[1]}
        assert isinstance(item["misc"]["tgt_frame_id"], np.uint32)
        pre = f"{typ}_i{i}_"
        ref_keys = {k[len(pre):].split("__")[0] for k in gold if k.startswith(pre)}
        derived = {k for k in item if k.startswith("dyn_rgb") or k.startswith("static_rgb")}
        assert set(item) - {"scene_id", "misc"} - derived == ref_keys
        for k in sorted(ref_keys):
            v = item[k].numpy()
            assert item[k].dtype == (torch.int64 if k.startswith("n_actual") or k == "seq_ids" else torch.float32), k
            if k.startswith("rgb_"):
                v = np.round(v * 255.0)
            if pre + k in gold:
                ref = gold[pre + k]
                assert v.shape == ref.shape, k
                if np.issubdtype(ref.dtype, np.integer) or k == "depth_range":
                    assert np.array_equal(v, ref), k
                else:
                    np.testing.assert_allclose(v, ref, rtol=1e-6, atol=1e-7, err_msg=k)
            else:
                assert tuple(v.shape) == tuple(gold[pre + k + "__shape"]), k
                np.testing.assert_allclose(_digest(v), gold[pre + k + "__digest"], rtol=1e-7, atol=1e-9, err_msg=k)
        for sfx in ("spatial", "temporal", "temporal_track_fwd2tgt", "temporal_track_bwd2tgt"):
            m = item[f"dyn_mask_src_{sfx}"]
            assert torch.equal(item[f"dyn_rgb_src_{sfx}"], item[f"rgb_src_{sfx}"] * m)
            assert torch.equal(item[f"static_rgb_src_{sfx}"], item[f"rgb_src_{sfx}"] * (1 - m))


def test_dycheck_fixture_covers_the_edge_cases(gold):
    """the tree exercises what the issue asks for: constant ranges (no static point), near / far clamping, per-pixel
    overwrites, and a target whose spatial sources are all dynamic"""
    const, clamped = 0, 0
    for k, v in gold.items():
        if k.endswith("_depth_range"):
            const += int(np.unique(v[..., 0]).size == 1)
            clamped += int(np.float32(DT.NEAR) in v[..., 0] or np.float32(DT.FAR) in v[..., 1])
    assert const >= 1 and clamped >= 1
    assert np.unique(gold["closest_wo_temporal_i2_depth_range"][..., 0]).size > 100


def test_dycheck_parser_camera_and_split_creation(tree, gold):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckCamera, iPhoneParser

    sd = pathlib.Path(tree) / "iphone" / DT.SCENE
    p = iPhoneParser(DT.SCENE, data_root=str(sd.parent))
    for split, want in (("train", [(0, t) for t in DT.TRAIN_T]), ("val", DT.VAL)):
        d = json.loads((sd / "splits" / f"{split}.json").read_text())  # written when missing, as upstream
        assert list(zip(d["camera_ids"], d["time_ids"])) == want
        assert d["frame_names"] == [DT.frame_name(c, t) for c, t in want]
        names, t_ids, c_ids = p.load_split(split)
        assert t_ids.dtype == np.uint32 and c_ids.dtype == np.uint32
    assert np.array_equal(p.load_split("train")[1], gold["train_time_ids"])
    cam = p.load_camera(10, 1)
    assert cam.intrin.dtype == np.float32 and cam.extrin.dtype == np.float32
    assert np.array_equal(cam.intrin, gold["cam_1_10_intrin"]) and np.array_equal(cam.extrin, gold["cam_1_10_extrin"])
    assert np.array_equal(np.asarray(cam.image_size), gold["cam_1_10_image_size"])
    assert cam.intrin[0, 1] != 0 and cam.intrin[1, 1] != cam.intrin[0, 0]  # skew, pixel aspect
    raw = DyCheckCamera.fromjson(sd / "camera" / f"{DT.frame_name(1, 10)}.json")
    assert np.array_equal(raw.rescale_image_domain(0.5).focal_length, np.float32(raw.focal_length * np.float32(0.5)))
    assert p.load_rgba(10, 1).shape == (DT.H, DT.W, 4) and p.load_depth(10, 0).shape == (DT.H, DT.W, 1)
    assert p.load_covisible(10, 1, "val").shape == (DT.H, DT.W)
    ds = _dataset(tree, "closest_wo_temporal")
    np.testing.assert_array_equal(ds.train_info_dict[DT.SCENE]["train_c2w"], gold["train_c2w"])


def test_dycheck_selection_rules(tree):
    from pgdvs_amd.datasets.dycheck_iphone import kmeans_labels, select_temporal_frames

    t_ids = np.array(DT.TRAIN_T)
    s = select_temporal_frames(np.uint32(1), t_ids, 2)  # before the first train instant: one neighbour + placeholder
    assert s["temporal"] == [3, 3] and s["n_actual_temporal"] == 1 and s["n_actual_fwd2tgt"] == 0
    assert s["bwd2tgt"] == [4, 5] and s["n_actual_bwd2tgt"] == 2
    s = select_temporal_frames(np.uint32(18), t_ids, 2)  # last instant
    assert s["temporal"] == [18, 18] and s["fwd2tgt"] == [16, 17] and s["bwd2tgt"] == [18, 18] and s["n_actual_bwd2tgt"] == 0
    s = select_temporal_frames(np.uint32(4), t_ids, 3)  # the window is cut at the first train instant
    assert s["fwd2tgt"] == [4, 4, 3] and s["n_actual_fwd2tgt"] == 1
    ds = _dataset(tree, "clustered")
    centres, labels = ds.scene_clusters(DT.SCENE)
    fresh = kmeans_labels(ds.train_info_dict[DT.SCENE]["train_c2w"][:, :3, 3], 4)
    assert np.array_equal(labels, fresh[1]) and np.array_equal(centres, fresh[0])
    idx = [i for i in range(len(ds)) if ds.valid_fs[i][2] >= 12][0]
    item = ds[idx]
    assert ds.scene_clusters(DT.SCENE)[1] is labels  # cached per scene, not refitted per item
    spatial = item["seq_ids"][1:4].tolist()
    tgt_t, tgt_c = ds.valid_fs[idx][2], ds.valid_fs[idx][3]
    raw_c2w = np.linalg.inv(ds.parser_dict[DT.SCENE].load_camera(tgt_t, tgt_c).extrin)
    want = []
    for lab in np.argsort(np.linalg.norm(centres - raw_c2w[:3, 3][None], axis=1))[:3]:
        members = np.nonzero(labels == lab)[0]  # indices into the train list
        want.append(int(members[np.argmin(np.abs(members - float(tgt_t)))]))
    assert spatial == sorted(want)
    # ... which are then used as TIME ids: the first source is the frame of time id spatial[0], not train frame spatial[0]
    c2w = np.linalg.inv(np.linalg.inv(np.linalg.inv(ds.parser_dict[DT.SCENE].load_camera(spatial[0], 0).extrin)))
    assert np.array_equal(item["flat_cam_src_spatial"][0, 18:].numpy(), c2w.reshape(-1).astype(np.float32))
    assert spatial[0] - min(DT.TRAIN_T) != spatial[0]


def test_dycheck_dataset_class_and_combined(tree):
    from pgdvs_amd.datasets.combined import CombinedDataset, dataset_class
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset
    from pgdvs_amd.instantiate import instantiate, load_config

    assert dataset_class("dycheck_iphone_eval") is DyCheckiPhoneEvaluationDataset
    ds_cfg = load_config().dataset
    spec = dict(ds_cfg.dataset_specifics.dycheck_iphone_eval)
    assert spec["spatial_src_view_type"] == "clustered" and spec["raw_data_dir"] == "iphone"
    spec.update(scene_ids=[DT.SCENE], mask_data_dir="flow_mask", flow_data_dir="flow_mask", n_src_views_spatial=3,
                spatial_src_view_type="closest_wo_temporal", n_src_views_temporal_track_one_side=2)
    node = dict(ds_cfg)
    node.update(data_root=tree, dataset_list={"eval": ["dycheck_iphone_eval"]}, dataset_specifics={"dycheck_iphone_eval": spec})
    ds = instantiate(node, mode="eval")
    assert isinstance(ds, CombinedDataset) and len(ds) == len(DT.VAL)
    assert isinstance(ds.datasets["dycheck_iphone_eval"], DyCheckiPhoneEvaluationDataset)
    assert torch.equal(ds[2]["depth_range"], ds.datasets["dycheck_iphone_eval"][2]["depth_range"])


def test_dycheck_device_path_refuses_dataloader_workers(tree):
    """forked DataLoader workers must not touch the GPU: the device path raises there, naming the setting to use"""
    ds = _dataset(tree, "closest_wo_temporal", device="cuda")
    dl = torch.utils.data.DataLoader(ds, batch_size=None, num_workers=1)
    with pytest.raises(RuntimeError, match="n_dataloader_workers=0"):
        next(iter(dl))


def test_dycheck_read_flow(tree):
    ds = _dataset(tree, "closest_wo_temporal")
    flow, occ = ds._read_flow(DT.SCENE, 5, 7, (DT.H, DT.W))
    info = np.load(pathlib.Path(tree) / "flow_mask" / DT.SCENE / "flows" / "interval_2" / "0_00005_0_00007.npz")
    assert np.array_equal(flow, info["flow"])
    assert np.array_equal(occ, (np.abs(info["coord_diff"]).sum(2) > 1.0).astype(np.float32))
    z, zo = ds._read_flow(DT.SCENE, 6, 6, (DT.H, DT.W))
    assert not z.any() and not zo.any() and z.shape == (DT.H, DT.W, 2)


# ---------------------------------------------------------------- the float orders the numpy path and the HIP op share
def test_fma32_is_correctly_rounded():
    from pgdvs_amd.datasets.dycheck_iphone import _fma32

    rng = np.random.default_rng(3)
    a = rng.normal(size=4000).astype(np.float32)
    b = np.round(rng.uniform(0, 2000, 4000)).astype(np.float32)
    c = (rng.normal(size=4000) * 10.0 ** rng.integers(-12, 4, 4000)).astype(np.float32)
    # exact midpoints: a*b + c lands halfway between two float32 values by construction
    a[:8], b[:8], c[:8] = np.float32(1 + 2 ** -23), np.float32(1 + 2 ** -23), np.float32(-1)
    got = _fma32(a, b, c)
    from fractions import Fraction

    for x, y, z, g in zip(a, b, c, got):  # nearest float32 to the exact a b + c (ties: either neighbour is as near)
        ex = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(Fraction(float(g)) - ex) <= min(abs(Fraction(float(lo)) - ex), abs(Fraction(float(hi)) - ex))


def _fused(A, X, dt):
    """acc = a0 x0, then acc = fma(a_k, x_k, acc) for k ascending, in dt (exact fma emulated with Fractions per entry)"""
    from fractions import Fraction

    out = np.empty((A.shape[0], X.shape[1]), dt)
    for i in range(A.shape[0]):
        for j in range(X.shape[1]):
            acc = dt(Fraction(float(A[i, 0])) * Fraction(float(X[0, j])))
            for k in range(1, A.shape[1]):
                acc = dt(Fraction(float(A[i, k])) * Fraction(float(X[k, j])) + Fraction(float(acc)))
            out[i, j] = acc
    return out


def _sequential(A, X, dt):
    out = (A[:, 0:1] * X[0:1, :]).astype(dt)
    for k in range(1, A.shape[1]):
        out = (out + (A[:, k:k + 1] * X[k:k + 1, :]).astype(dt)).astype(dt)
    return out


@pytest.mark.parametrize("n", [2, 7, 300, 5000])
def test_numpy_matmul_and_torch_bmm_orders_are_fused_ascending(n):
    """The products depth_range_numpy / compute_pcl hand to BLAS, on the installed numpy and torch: np.matmul in float32
    (4x4 and 3x3 @ points) and float64 (4x4 @ points), and torch's CPU bmm of the rays, accumulate with fused
    multiply-adds over k ascending -- the order the HIP op uses -- and not sequentially (DESIGN.md 8f-3 DyCheck).  One
    point (n = 1) is a matrix-vector product, which BLAS orders differently (float32: pairwise sums); see DESIGN.md"""
    rng = np.random.default_rng(n)
    pts = (rng.normal(size=(n, 3)) * 3).astype(np.float32)
    homo = np.pad(pts, ((0, 0), (0, 1)), constant_values=1)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, rng.normal(size=3)
    A32 = np.linalg.inv(A.astype(np.float32))
    m = min(n, 400)
    r32 = np.matmul(A32, homo.T)
    assert np.array_equal(r32[:, :m], _fused(A32, homo.T[:, :m], np.float32))
    r64 = np.matmul(A32, homo.T.astype(np.float64))
    assert np.array_equal(r64[:, :m], _fused(A32.astype(np.float64), homo.T[:, :m].astype(np.float64), np.float64))
    K = np.array([[50.3, 0.7, 31.2], [0, 55.1, 23.9], [0, 0, 1]], np.float32)
    rk = np.matmul(K, r32[:3])
    assert np.array_equal(rk[:, :m], _fused(K, r32[:3, :m], np.float32))
    if n >= 300:  # the orders really differ on these sizes
        assert not np.array_equal(r32, _sequential(A32, homo.T, np.float32))
    # torch's bmm of the rays: compute_pcl's restatement
    from pgdvs_amd.datasets.dycheck_iphone import compute_pcl, ray_constants

    K4 = np.eye(4)
    K4[:3, :3] = K
    c2w = A.astype(np.float32)
    M, o = ray_constants(K4, c2w)
    h, w = 6, max(1, n // 6)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    pix = np.stack([u.reshape(-1), v.reshape(-1), np.ones(h * w)]).astype(np.float32)
    rays = torch.FloatTensor(c2w)[None, :3, :3].bmm(torch.inverse(torch.FloatTensor(K4)[None, :3, :3])).bmm(
        torch.from_numpy(pix)[None]).transpose(1, 2).reshape(-1, 3).numpy()
    depth = rng.uniform(1, 3, (h, w)).astype(np.float32)
    assert np.array_equal(compute_pcl(h, w, M, o, depth), torch.FloatTensor(c2w)[:3, 3].numpy()[None] + rays * depth.reshape(-1, 1))
