"""The NVIDIA evaluation loader's ZoeDepth branch (datasets/nvidia_eval.py) on the host: its items against the reference's
own on the synthetic tree of tests/golden/nvidia_zoe_tree.py (tests/golden/make_golden_nvidia_zoe.py), bit for bit, from the
directory and from the zip; the "moe" choice frame by frame, ties included; the constructor's checks; pickling; the loaders
that keep refusing ZoeDepth; the pieces the device path relies on (float64 unprojection, nearest resize of a float64 image,
the stored dtypes); and the host-side contract of pgdvs_nvidia_zoe_depth_range (exports, shape and pointer checks)."""
import ctypes as C
import hashlib
import pathlib
import pickle
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402

# the exact-0 prediction's depth overflows on the way to float32, as it does upstream
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return ZT.build_tree(tmp_path_factory.mktemp("nvidia_zoe"))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "nvidia_zoe_items.npz"))


def _digest(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a @ np.random.default_rng(12345).random(a.size), a.sum(), a.min(), a.max()])


def _sha256(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).digest(), np.uint8)


def _dataset(root, setting, container, **kw):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    return NvidiaDynEvaluationDataset(data_root=root, use_zoe_depth=setting, zoe_depth_data_path=ZT.CONTAINERS[container],
                                      **{**ZT.KW, **kw})


def assert_item_equals_fixture(item, g, prefix):
    """every stored array, or shape and digest, of one item: equal bit for bit"""
    names = {k[len(prefix):].split("__")[0] for k in g if k.startswith(prefix)}
    assert names == {k for k in item if k.startswith(("depth_range", "depth_src_", "flat_cam_", "seq_ids"))}, prefix
    for k in sorted(names):
        v = item[k].numpy()
        if prefix + k in g:
            ref = g[prefix + k]
            assert v.dtype == ref.dtype and v.shape == ref.shape, (prefix, k, v.dtype, ref.dtype)
            assert np.array_equal(v.view(np.uint8), ref.view(np.uint8)), (prefix, k, v, ref)
        else:
            assert tuple(v.shape) == tuple(g[f"{prefix}{k}__shape"]) and v.dtype == np.float32, (prefix, k)
            # bit for bit through the hash of the bytes; the digest's float64 sums run in an order the CPU's BLAS / SIMD
            # width picks, so they agree to the sibling fixture's tolerance (41472 terms: rounding stays below 1e-11)
            assert np.array_equal(_sha256(v), g[f"{prefix}{k}__sha256"]), (prefix, k, _digest(v), g[f"{prefix}{k}__digest"])
            np.testing.assert_allclose(_digest(v), g[f"{prefix}{k}__digest"], rtol=1e-7, atol=1e-9, err_msg=prefix + k)


@pytest.mark.parametrize("container", ["dir", "zip"])
@pytest.mark.parametrize("setting", ZT.SETTINGS)
def test_items_equal_the_reference_exactly(tree, golden, setting, container):
    assert str(golden["numpy_version"]).split(".")[0] == np.__version__.split(".")[0] == "2", "the fixture pins NumPy 2's promotion"
    ds = _dataset(tree, setting, container)
    assert ds.zoe_depth_data_path.is_file() == (container == "zip")  # each name resolved to its other form
    assert len(ds) == NT.F * NT.N_CAMS
    for n, (f, c) in enumerate(golden["items"]):
        item = ds[int(f) * NT.N_CAMS + int(c)]
        assert item["misc"] == {"scene_id": NT.SCENE, "tgt_frame_id": int(f), "tgt_cam_id": int(c)}
        assert_item_equals_fixture(item, golden, f"{setting}_{container}_i{n}_")
    # the tree's edge frames reached the fixture: the exact-0 prediction pins near at its floor in item 0
    assert golden[f"{setting}_{container}_i0_depth_range"][0] == np.float32(1e-16)
    assert golden[f"{setting}_{container}_i2_depth_range"][0] > 0.1  # ... and no other frame does


@pytest.mark.parametrize("container", ["dir", "zip"])
def test_moe_choice_per_frame(tree, golden, container):
    from pgdvs_amd.datasets.nvidia_eval import make_zoe_k_dict, read_zoe_npz, select_zoe_pair, zoe_scale_shift_keys

    assert list(make_zoe_k_dict().values()) == ZT.PAIRS
    ds = _dataset(tree, "moe", container)
    zobj = ds._zoe_zip_obj()
    assert (zobj is not None) == (container == "zip")
    picked = set()
    for f in range(NT.F):
        pair = select_zoe_pair(ds.zoe_depth_data_path, zobj, NT.SCENE, f, "moe")
        assert list(pair) == golden[f"moe_choice_{container}"][f].tolist() == list(ZT.mean_errors(f)[1]), f
        picked.add(pair)
        pred, scale, shift = read_zoe_npz(ds.zoe_depth_data_path, zobj, NT.SCENE, f, "moe")
        raw = np.load(tree / ZT.ZOE_DIR / NT.SCENE / "dense" / f"zoe_depths_{pair[0]}" / f"{f:05d}.npz")
        ks, kh = zoe_scale_shift_keys(pair[1])
        assert np.array_equal(pred, raw["depth_pred"]) and scale == raw[ks] and shift == raw[kh]
        assert pred.dtype == np.float32 and scale.dtype == shift.dtype == np.float64 and scale.ndim == 0
    assert len(picked) >= 10
    # frame 9: two pairs tie in magnitude, the later one of the tree's own ranking comes first in the key order
    me, best = ZT.mean_errors(9)
    tied = [ZT.PAIRS[j] for j in np.flatnonzero(np.abs(me) == np.abs(me).min())]
    assert len(tied) == 2 and best == tied[0] and me[ZT.PAIRS.index(tied[0])] == -me[ZT.PAIRS.index(tied[1])]
    # a fixed key never opens the other files
    assert select_zoe_pair("/nonexistent", None, NT.SCENE, 0, "k_me_med_share") == ("k", "me_med_share")
    assert zoe_scale_shift_keys("me_med_share") == ("disp_share_scale_med", "disp_share_shift_med")
    assert zoe_scale_shift_keys("mae_trim_indiv") == ("disp_indiv_scale_trim", "disp_indiv_shift_trim")


def test_constructor_checks(tree):
    with pytest.raises(AssertionError):
        _dataset(tree, "k_mae_med_share", "dir")  # upstream's comment names such keys; its table has none
    with pytest.raises(AssertionError):
        _dataset(tree, "zoe", "dir")
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    for missing in ("no_such_zoe", "no_such_zoe.zip"):
        with pytest.raises(AssertionError):
            NvidiaDynEvaluationDataset(data_root=tree, use_zoe_depth="moe", zoe_depth_data_path=missing, **ZT.KW)
    # exact names work too, and "none" never looks at the path
    assert NvidiaDynEvaluationDataset(data_root=tree, use_zoe_depth="moe", zoe_depth_data_path=ZT.ZOE_DIR,
                                      **ZT.KW).zoe_depth_data_path.is_dir()
    assert NvidiaDynEvaluationDataset(data_root=tree, use_zoe_depth="moe", zoe_depth_data_path=f"{ZT.ZOE_ZIP}.zip",
                                      **ZT.KW).zoe_depth_data_path.is_file()
    assert NvidiaDynEvaluationDataset(data_root=tree, use_zoe_depth="none", zoe_depth_data_path="no_such_zoe",
                                      **ZT.KW).zoe_depth_data_path is None


@pytest.mark.parametrize("container", ["dir", "zip"])
def test_pickles_before_and_after_an_item_without_a_zip_handle(tree, container):
    import zipfile

    ds = _dataset(tree, "moe", container)
    idx = 5 * NT.N_CAMS + 5
    before = pickle.loads(pickle.dumps(ds))
    want = ds[idx]
    assert (ds._zoe_zip is not None) == (container == "zip")  # opened by the first item only
    blob = pickle.dumps(ds)
    after = pickle.loads(blob)
    for clone in (before, after):
        assert not any(isinstance(v, zipfile.ZipFile) or (isinstance(v, tuple) and any(isinstance(x, zipfile.ZipFile) for x in v))
                       for v in clone.__dict__.values())
        assert clone._zoe_zip is None
        got = clone[idx]
        for k in ("depth_range", "depth_src_spatial", "depth_src_temporal", "depth_src_temporal_track_fwd2tgt"):
            assert np.array_equal(got[k].numpy().view(np.uint8), want[k].numpy().view(np.uint8)), k
    # a DataLoader worker (a forked process) opens its own handle
    dl = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, [idx]), batch_size=None, num_workers=1)
    got = next(iter(dl))
    assert torch.equal(got["depth_range"], want["depth_range"]) and torch.equal(got["depth_src_spatial"], want["depth_src_spatial"])


def test_other_loaders_keep_refusing_zoe_depth(tree):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynPureGeoEvaluationDataset
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    kw = {k: v for k, v in ZT.KW.items() if k != "mode"}
    with pytest.raises(NotImplementedError):  # upstream's own visualisation loader cannot read them either
        NvidiaDynVisualizationDataset(data_root=tree, mode="vis", use_zoe_depth="moe", zoe_depth_data_f=f"{ZT.ZOE_ZIP}.zip", **kw)
    with pytest.raises(TypeError):  # the pure-geometry loader has no such keyword: upstream forces "none"
        NvidiaDynPureGeoEvaluationDataset(data_root=tree, use_zoe_depth="moe", **ZT.KW)


def test_disparity_items_unchanged_beside_the_zoe_files(tree, golden_dir):
    """use_zoe_depth="none" on the tree with the ZoeDepth containers beside the scene: the items of nvidia_items.npz,
    through the comparison of tests/test_host_cpu.py"""
    import test_host_cpu as THC

    THC.test_nvidia_dataset_items_vs_reference(golden_dir, (NT, tree))


def test_device_path_refuses_dataloader_workers(tree):
    ds = _dataset(tree, "moe", "zip", device="cuda")
    dl = torch.utils.data.DataLoader(ds, batch_size=None, num_workers=1)
    with pytest.raises(RuntimeError, match="n_dataloader_workers=0"):
        next(iter(dl))


def test_evaluator_config_with_zoe_depth_loads_items(tree, golden):
    """the run type st_gnt_masked_attn_dy_zoed_pcl_clean's dataset overrides on the mirrored config"""
    from pgdvs_amd.datasets.combined import CombinedDataset
    from pgdvs_amd.instantiate import instantiate, load_config

    ds_cfg = load_config().dataset
    spec = dict(ds_cfg.dataset_specifics.nvidia_eval)
    assert spec["use_zoe_depth"] == "none" and spec["zoe_depth_data_path"] == "nvidia_long_zoedepth.zip"
    spec.update({k: v for k, v in ZT.KW.items() if k not in ("max_hw", "mode")})
    spec.update(use_zoe_depth="k_me_med_share", zoe_depth_data_path=f"{ZT.ZOE_ZIP}.zip")
    node = dict(ds_cfg)
    node.update(data_root=str(tree), dataset_specifics={"nvidia_eval": spec})
    ds = instantiate(node, mode="eval")
    assert isinstance(ds, CombinedDataset) and len(ds) == NT.F * NT.N_CAMS
    f, c = (int(x) for x in golden["items"][0])
    assert_item_equals_fixture(ds[f * NT.N_CAMS + c], golden, "k_me_med_share_zip_i0_")


# ---------------------------------------------------------------------------- the pieces the two paths share
def test_alignment_dtypes_and_float64_unprojection():
    """zoe_align keeps upstream's types (float32 disparity, float64 from the 0-d float64 scale on), and compute_pcl with a
    float64 depth is double(o) + double(d) depth, multiply and add rounded on their own, d the float32 direction"""
    from fractions import Fraction

    from pgdvs_amd.datasets.nvidia_eval import compute_pcl, ray_constants, zoe_align

    rng = np.random.default_rng(3)
    h, w = 5, 7
    pred = rng.uniform(0.5, 4, (h, w)).astype(np.float32)
    pred[0, 0] = 0.0
    scale, shift = np.asarray(np.float64(1.1)), np.asarray(np.float64(-0.02))
    depth = zoe_align(pred, scale, shift)
    assert depth.dtype == np.float64
    raw = np.float32(1.0) / (pred + np.float32(1e-16))
    assert raw.dtype == np.float32 and raw[0, 0] == np.float32(1.0) / np.float32(1e-16)
    assert np.array_equal(depth, 1.0 / ((1.1 * raw.astype(np.float64) - 0.02) + 1e-16))
    x = float(raw[1, 2])  # one element in exact arithmetic, rounded after every operation
    rnd = lambda q: float(q)  # noqa: E731  (Fraction -> nearest double)
    disp = rnd(Fraction(rnd(Fraction(1.1) * Fraction(x))) + Fraction(-0.02))
    assert depth[1, 2] == rnd(1 / (Fraction(disp) + Fraction(1e-16)))
    c2w = np.eye(4)
    c2w[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    c2w[:3, 3] = rng.normal(size=3)
    K = np.eye(4)
    K[:3, :3] = [[0.9 * w, 0, w / 2.0], [0, 0.9 * w, h / 2.0], [0, 0, 1]]
    d32 = compute_pcl(h, w, K, c2w, np.ones((h, w), np.float32))  # o + d in float32
    pcl = compute_pcl(h, w, K, c2w, depth, f64_depth=True)
    assert pcl.dtype == np.float64 and compute_pcl(h, w, K, c2w, depth).dtype == np.float32  # only on request
    M, o = ray_constants(K, c2w)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    dirs = (M @ np.stack([u.reshape(-1), v.reshape(-1), np.ones(h * w, np.float32)], 0)).T
    assert dirs.dtype == np.float32 and np.allclose(o + dirs, d32, rtol=1e-6)
    for i in (1, 9, 34):
        for ax in range(3):
            prod = rnd(Fraction(float(dirs[i, ax])) * Fraction(float(depth.reshape(-1)[i])))
            assert pcl[i, ax] == rnd(Fraction(float(o[ax])) + Fraction(prod)), (i, ax)


def test_nearest_resize_of_a_float64_image_picks_pils_pixels():
    from pgdvs_amd.datasets.nvidia_eval import _resize, _resize_nearest_f64

    rng = np.random.default_rng(8)
    src = rng.integers(0, 1 << 20, (9, 14)).astype(np.float32)  # exact in float32, so PIL's own resize is the check
    for h, w in ((288, 36), (5, 9), (9, 14), (13, 3)):
        got = _resize_nearest_f64(src.astype(np.float64) + 1e-9, h, w)
        assert got.dtype == np.float64 and got.shape == (h, w)
        assert np.array_equal(got - 1e-9, _resize(src, h, w, PIL.Image.Resampling.NEAREST).astype(np.float64))


def test_stored_size_other_than_the_target_is_resized_after_alignment(tree, tmp_path):
    """a prediction stored at twice the size: the aligned float64 depth is resized (nearest), on either path's loader"""
    from pgdvs_amd.datasets.nvidia_eval import _resize_nearest_f64, zoe_align

    ds = _dataset(tree, "k_me_med_share", "dir")
    pred, scale, shift = ds._read_zoe(NT.SCENE, 6)
    big = np.repeat(np.repeat(pred, 2, axis=0), 2, axis=1)
    aligned = _resize_nearest_f64(zoe_align(big, scale, shift), NT.H, NT.W)
    assert aligned.dtype == np.float64 and np.array_equal(aligned, zoe_align(pred, scale, shift))


# ---------------------------------------------------------------------------- the entry point's host side
def test_library_exports_and_argument_checks_without_a_gpu():
    from pgdvs_amd import _lib

    lib = _lib.load()
    q, f = lib.pgdvs_nvidia_zoe_depth_range_workspace_bytes, lib.pgdvs_nvidia_zoe_depth_range
    assert q(10, 288, 550) == lib.pgdvs_nvidia_depth_range_workspace_bytes(10, 288, 550) >= 10 * 288 * 550 * 8
    assert q(2, 1, 2) > 0
    for bad in ((0, 288, 550), (1, 0, 5), (3, 1, 1), (1, 1, 1), (2, 1 << 15, 1 << 15), (-1, 4, 4)):
        assert q(*bad) == -1, bad  # PGDVS_ERR_INVALID
    # rejected before anything is launched (no GPU here): the pointers are never followed
    ss = (C.c_double * 4)(1.0, 0.0, 1.0, 0.0)
    inv = (C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
    p = C.c_void_p(4096)
    assert f(p, ss, None, 0, 4, 4, None, p, None, None, None, 0, None) == -1             # V = 0
    assert f(p, ss, None, 2, 1 << 15, 1 << 15, None, p, None, None, None, 0, None) == -1  # V H W >= 2^31
    assert f(p, ss, p, 2, 1, 1, inv, p, p, None, p, 1 << 20, None) == -1                  # H W == 1 with a range
    assert f(None, ss, None, 1, 4, 4, None, p, None, None, None, 0, None) == -1           # null prediction
    assert f(p, ss, None, 1, 4, 4, None, None, None, None, None, 0, None) == -1           # null output
    assert f(p, None, None, 1, 4, 4, None, p, None, None, None, 0, None) == -1            # null scale / shift
    assert f(p, ss, p, 1, 4, 4, None, p, None, None, None, 0, None) == -1                 # rays without the target
    assert f(p, ss, None, 1, 4, 4, None, p, None, p, None, 0, None) == -1                 # near_far without a range
    assert f(p, ss, p, 1, 4, 4, inv, p, p, None, None, 0, None) == -3                     # PGDVS_ERR_WORKSPACE
    assert b"pgdvs_nvidia_zoe_depth_range" in lib.pgdvs_last_error()


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from pgdvs_amd import ops

    with pytest.raises(ops.PgdvsHipError):
        ops.nvidia_zoe_depth(torch.ones(1, 2, 3), np.array([[1.0, 0.0]]))
