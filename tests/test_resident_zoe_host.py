"""ZoeDepth inputs from the resident store on the host (``NvidiaDynEvaluationDataset(resident=True, use_zoe_depth=...)``,
datasets/resident.py in prediction mode): the items against the disk path's and against the reference's own fixture, bit for
bit; the pair kept per slot under "moe"; a second pass that opens no ZoeDepth file; predictions stored at another size (the
resize commutes with the alignment); the refusals; and the host side of ``pgdvs_item_zoe_depths`` (exports, the workspace
query's and the entry point's checks, the op's refusal of host tensors).

Bit identity is derived: the host store restates the disk path's statements (``zoe_align`` with the stored 0-d float64 scale
and shift, ``spatial_depth_range``) on the same float32 predictions, and NEAREST picks pixels, so it commutes with a
pointwise alignment."""
import ctypes as C
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402
import resident_cases as RC  # noqa: E402
from test_nvidia_zoe_host import assert_item_equals_fixture  # noqa: E402

# the exact-0 prediction's depth overflows on the way to float32, as it does upstream
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

BIG, F64_PRED, F32_SCALE = "zoe_big", "zoe_f64_pred", "zoe_f32_scale"  # variants of the tree's ZoeDepth directory


def _variant(root, name, change):
    """the tree's ZoeDepth directory copied to ``root/name``, every file's entries passed through ``change(entries, type)``"""
    for src in sorted((root / ZT.ZOE_DIR).rglob("*.npz")):
        info = dict(np.load(src))
        change(info, src.parent.name.rsplit("_", 1)[1])
        dst = root / name / src.relative_to(root / ZT.ZOE_DIR)
        dst.parent.mkdir(parents=True, exist_ok=True)
        np.savez(dst, **info)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = ZT.build_tree(tmp_path_factory.mktemp("resident_zoe"))
    rng = np.random.default_rng(77)

    def big(info, t):  # fresh predictions at twice the size: which pixel NEAREST picks decides the item
        info["depth_pred"] = rng.uniform(0.5, 5.0, (2 * NT.H, 2 * NT.W)).astype(np.float32)

    def f64_pred(info, t):
        info["depth_pred"] = info["depth_pred"].astype(np.float64)

    def f32_scale(info, t):
        info["disp_share_scale_med"] = np.asarray(info["disp_share_scale_med"], np.float32)

    _variant(root, BIG, big)
    _variant(root, F64_PRED, f64_pred)
    _variant(root, F32_SCALE, f32_scale)
    return root


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "nvidia_zoe_items.npz"))


def _dataset(root, setting, path, **kw):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    return NvidiaDynEvaluationDataset(data_root=root, use_zoe_depth=setting, zoe_depth_data_path=path, **{**ZT.KW, **kw})


def _index(f, c):
    return int(f) * NT.N_CAMS + int(c)


# ---------------------------------------------------------------------------- items
@pytest.mark.parametrize("container", ["dir", "zip"])
@pytest.mark.parametrize("setting", ZT.SETTINGS)
def test_host_store_items_equal_the_disk_items_and_the_reference(tree, golden, setting, container):
    assert [tuple(int(x) for x in fc) for fc in golden["items"]] == ZT.ITEMS
    disk = _dataset(tree, setting, ZT.CONTAINERS[container])
    res = _dataset(tree, setting, ZT.CONTAINERS[container], resident=True)
    assert res.store is not None and res.store.device is None
    for n, (f, c) in enumerate(ZT.ITEMS):
        item = res[_index(f, c)]
        RC.assert_items_equal(item, disk[_index(f, c)], (setting, container, n))
        assert_item_equals_fixture(item, golden, f"{setting}_{container}_i{n}_")
    scene = res.store.scenes[NT.SCENE]
    assert scene.prediction and scene.scale_shift.dtype == np.float64 and scene.depth.dtype == torch.float32
    filled = set(np.flatnonzero(scene.filled).tolist())
    assert ZT.ZERO_PRED_FRAME in filled and ZT.ZERO_SCALE_FRAME in filled and filled & set(ZT.TIE_FRAMES), sorted(filled)
    assert res.store.stats["frames_decoded"] == len(filled) and res.store.stats["items_built"] == len(ZT.ITEMS)


@pytest.mark.parametrize("container", ["dir", "zip"])
def test_moe_pair_kept_per_slot(tree, container):
    from pgdvs_amd.datasets.nvidia_eval import zoe_scale_shift_keys

    res = _dataset(tree, "moe", ZT.CONTAINERS[container], resident=True)
    for f, c in ZT.ITEMS:
        res[_index(f, c)]
    scene = res.store.scenes[NT.SCENE]
    filled = np.flatnonzero(scene.filled).tolist()
    assert len(filled) >= 10 and set(filled) & set(ZT.TIE_FRAMES)
    for f in filled:
        pair = ZT.mean_errors(f)[1]
        assert tuple(scene.zoe_pairs[f]) == pair, f
        raw = np.load(tree / ZT.ZOE_DIR / NT.SCENE / "dense" / f"zoe_depths_{pair[0]}" / f"{f:05d}.npz")
        ks, kh = zoe_scale_shift_keys(pair[1])
        assert scene.scale_shift[f, 0] == raw[ks] and scene.scale_shift[f, 1] == raw[kh]
        assert np.array_equal(scene.depth[f].numpy().view(np.uint32), raw["depth_pred"].view(np.uint32)), f
    assert len({tuple(scene.zoe_pairs[f]) for f in filled}) >= 6  # the choice moves from frame to frame
    assert all(scene.zoe_pairs[f] is None for f in range(NT.F) if f not in filled)


@pytest.mark.parametrize("setting", ["k_me_med_share", "moe"])
def test_second_pass_opens_no_zoe_file(tree, monkeypatch, setting):
    from pgdvs_amd.datasets import nvidia_eval as NE

    calls = []
    real = NE._load_zoe_npz

    def counted(*a, **kw):
        calls.append(a[-2:])
        return real(*a, **kw)

    monkeypatch.setattr(NE, "_load_zoe_npz", counted)
    res = _dataset(tree, setting, ZT.CONTAINERS["zip"], resident=True)
    first = [res[_index(f, c)] for f, c in ZT.ITEMS]
    stats = dict(res.store.stats)
    assert len(calls) == stats["zoe_files_read"] == stats["frames_decoded"] * (4 if setting == "moe" else 1) > 0
    del calls[:]
    second = [res[_index(f, c)] for f, c in ZT.ITEMS]
    assert calls == []
    assert res.store.stats["zoe_files_read"] == stats["zoe_files_read"] and res.store.stats["frames_decoded"] == stats["frames_decoded"]
    assert res.store.stats["items_built"] == 2 * len(ZT.ITEMS)
    for a, b in zip(first, second):
        RC.assert_items_equal(b, a, setting)
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()) if isinstance(x, torch.Tensor))


# ---------------------------------------------------------------------------- another stored size
@pytest.mark.parametrize("setting", ["n_me_trim_indiv", "moe"])
def test_predictions_stored_at_twice_the_size(tree, setting):
    disk, res = _dataset(tree, setting, BIG), _dataset(tree, setting, BIG, resident=True)
    small = _dataset(tree, setting, ZT.ZOE_DIR)
    for n, (f, c) in enumerate(ZT.ITEMS[:2]):
        want = disk[_index(f, c)]
        RC.assert_items_equal(res[_index(f, c)], want, (setting, n))
        assert not torch.equal(want["depth_src_spatial"], small[_index(f, c)]["depth_src_spatial"])  # other predictions indeed
    scene = res.store.scenes[NT.SCENE]
    assert tuple(scene.depth.shape[1:]) == (NT.H, NT.W)


@pytest.mark.parametrize("src,dst", [((576, 72), (288, 36)), ((100, 37), (288, 36)), ((289, 35), (288, 36)), ((300, 40), (288, 36)),
                                     ((7, 5), (13, 11))])
def test_nearest_resize_commutes_with_the_alignment(src, dst):
    """resize-after-alignment (the disk path: float64 under NumPy 2, through _resize_nearest_f64) against
    alignment-after-resize (the store: the float32 prediction through PIL's NEAREST)"""
    from pgdvs_amd.datasets.nvidia_eval import _resize, _resize_nearest_f64, zoe_align

    rng = np.random.default_rng(src[0] * 1000 + src[1])
    pred = rng.uniform(0.3, 6.0, src).astype(np.float32)
    pred.reshape(-1)[rng.permutation(pred.size)[:3]] = [0.0, np.inf, 1e-20]
    scale, shift = np.asarray(np.float64(1.07)), np.asarray(np.float64(-0.013))
    with np.errstate(all="ignore"):
        after = zoe_align(pred, scale, shift)
        after = (_resize_nearest_f64(after, *dst) if after.dtype == np.float64 else _resize(after, *dst, PIL.Image.Resampling.NEAREST))
        before = zoe_align(_resize(pred, *dst, PIL.Image.Resampling.NEAREST), scale, shift)
    assert before.shape == after.shape == dst and before.dtype == after.dtype
    assert np.array_equal(before.view(np.uint8), after.view(np.uint8))
    assert len(np.unique(before)) > min(pred.size, before.size) // 2  # pixels, not a constant


# ---------------------------------------------------------------------------- refusals
def test_refusals(tree):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynPureGeoEvaluationDataset

    res = _dataset(tree, "k_me_med_share", F64_PRED, resident=True)
    with pytest.raises(ValueError, match=r"zoe_depths_k/\d{5}\.npz.*depth_pred is float64"):
        res[_index(*ZT.ITEMS[0])]
    assert not res.store.scenes[NT.SCENE].filled.any()
    res = _dataset(tree, "k_me_med_share", F32_SCALE, resident=True)
    with pytest.raises(ValueError, match=r"zoe_depths_k/\d{5}\.npz.*disp_share_scale_med float32"):
        res[_index(*ZT.ITEMS[0])]
    # ... and only the entries the setting reads matter
    other = _dataset(tree, "k_me_trim_indiv", F32_SCALE, resident=True)
    RC.assert_items_equal(other[_index(*ZT.ITEMS[0])], _dataset(tree, "k_me_trim_indiv", ZT.ZOE_DIR)[_index(*ZT.ITEMS[0])], "other entries")
    with pytest.raises(ValueError, match="use_zoe_depth"):
        _dataset(tree, "k_mae_med_share", ZT.ZOE_DIR, resident=True)
    for missing in ("no_such_zoe", "no_such_zoe.zip"):
        with pytest.raises(ValueError, match="use_zoe_depth"):
            _dataset(tree, "moe", missing, resident=True)
    with pytest.raises(AssertionError):  # the non-resident constructor keeps its asserts
        _dataset(tree, "k_mae_med_share", ZT.ZOE_DIR)
    with pytest.raises(AssertionError):
        _dataset(tree, "moe", "no_such_zoe")
    with pytest.raises(TypeError):  # the pure-geometry loader keeps refusing ZoeDepth
        NvidiaDynPureGeoEvaluationDataset(data_root=tree, use_zoe_depth="moe", resident=True, **ZT.KW)
    # the store itself: a prediction scene takes the pair with the frame, any other scene none
    from pgdvs_amd.datasets.resident import SceneStore

    store = SceneStore()
    rgb, mask, pred = np.zeros((2, 3, 3), np.uint8), np.zeros((2, 3), np.uint8), np.ones((2, 3), np.float32)
    ss = (np.asarray(np.float64(1.0)), np.asarray(np.float64(0.0)))
    with pytest.raises(ValueError, match="prediction mode"):
        store.put(store.scene("a", 2, (2, 3), prediction=True), 0, rgb, mask, pred)
    with pytest.raises(ValueError, match="prediction mode"):
        store.put(store.scene("b", 2, (2, 3)), 0, rgb, mask, pred, ss)
    with pytest.raises(ValueError, match="float64"):
        store.put(store.scene("c", 2, (2, 3), prediction=True), 0, rgb, mask, pred.astype(np.float64), ss)
    with pytest.raises(ValueError, match="float32"):
        store.put(store.scene("d", 2, (2, 3), prediction=True), 0, rgb, mask, pred, (np.float32(1.0), ss[1]))
    scene = store.scene("e", 2, (2, 3), prediction=True)
    store.put(scene, 1, rgb, mask, pred, ss, ("k", "me_med_share"))
    assert scene.filled.tolist() == [False, True] and scene.scale_shift[1].tolist() == [1.0, 0.0]
    with pytest.raises(ValueError, match="prediction mode"):
        store.views(scene, [([1], True)], None)


# ---------------------------------------------------------------------------- the entry point's host side
def test_library_exports_and_argument_checks_without_a_gpu():
    import test_host_cpu as THC
    from pgdvs_amd import _lib

    THC.test_library_exports_every_declared_symbol()
    assert {"pgdvs_item_zoe_depths", "pgdvs_item_zoe_depths_workspace_bytes"} <= set(_lib.SIGNATURES) & set(THC._declared_symbols())
    lib = _lib.load()
    q, f = lib.pgdvs_item_zoe_depths_workspace_bytes, lib.pgdvs_item_zoe_depths
    assert q(10, 288, 550) == lib.pgdvs_nvidia_zoe_depth_range_workspace_bytes(10, 288, 550) >= 10 * 288 * 550 * 8
    assert q(1, 1, 2) > 0 and q(64, 3, 5) > 0
    for bad in ((0, 288, 550), (1, 0, 5), (3, 1, 1), (65, 4, 4), (2, 1 << 15, 1 << 15), (-1, 4, 4), (1, 1 << 20, 1), (1, 2, 1 << 20)):
        assert q(*bad) == -1, bad  # PGDVS_ERR_INVALID
    # rejected before anything is launched (no GPU here): the device pointers are never followed
    p = C.c_void_p(4096)
    inv = (C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
    ids, sizes, ss, out = (C.c_int32 * 3)(2, 0, 2), (C.c_int32 * 2)(2, 1), (C.c_double * 6)(1, 0, 1, 0, 1, 0), (C.c_void_p * 2)(4096, 8192)

    def call(pred=p, F=3, H=4, W=4, slot=64, ids=ids, n_views=3, ss=ss, sizes=sizes, n_groups=2, out=out, rays=None, inv=None,
             rng=None, nf=None, ws=None, ws_bytes=0):
        return f(pred, F, H, W, slot, ids, n_views, ss, sizes, n_groups, out, rays, inv, rng, nf, ws, ws_bytes, None)

    for what, kw in {
        "null table": dict(pred=None), "null ids": dict(ids=None), "null scale_shift": dict(ss=None), "null sizes": dict(sizes=None),
        "null out": dict(out=None), "a null group output": dict(out=(C.c_void_p * 2)(4096, 0)),
        "an output off 4 bytes": dict(out=(C.c_void_p * 2)(4096, 8194)), "a table off 16 bytes": dict(pred=C.c_void_p(4100)),
        "a slot off 16 bytes": dict(slot=72), "a slot under a frame": dict(slot=48), "no frames": dict(F=0), "H = 0": dict(H=0),
        "W = 2^20": dict(W=1 << 20, slot=1 << 24), "no views": dict(n_views=0), "65 views": dict(n_views=65), "no groups": dict(n_groups=0),
        "5 groups": dict(n_groups=5), "an empty group": dict(sizes=(C.c_int32 * 2)(3, 0)), "groups short of the ids": dict(sizes=(C.c_int32 * 2)(1, 1)),
        "groups beyond the ids": dict(sizes=(C.c_int32 * 2)(2, 2)), "an id equal to F": dict(F=2), "a negative id": dict(ids=(C.c_int32 * 3)(0, -1, 0)),
        "rays alone": dict(rays=p), "rays and the pose without depth_range": dict(rays=p, inv=inv), "near_far without a range": dict(nf=p),
        "depth_range alone": dict(rng=p),
        "H W == 1 with a range": dict(H=1, W=1, slot=16, rays=p, inv=inv, rng=p, ws=p, ws_bytes=1 << 20),
        "a workspace off 16 bytes": dict(rays=p, inv=inv, rng=p, ws=C.c_void_p(4104), ws_bytes=1 << 20),
    }.items():
        assert call(**kw) == -1, what
        assert b"pgdvs_item_zoe_depths" in lib.pgdvs_last_error(), what
    assert call(rays=p, inv=inv, rng=p) == -3                                # PGDVS_ERR_WORKSPACE: none given
    assert call(rays=p, inv=inv, rng=p, ws=p, ws_bytes=q(2, 4, 4) - 1) == -3   # ... and one byte short


def test_op_refuses_cpu_tensors_and_bad_arguments():
    from pgdvs_amd import ops

    with pytest.raises(ops.PgdvsHipError):
        ops.item_zoe_depth(torch.ones(3, 4, 4), [[0, 1]], np.ones((2, 2)))
    with pytest.raises(ValueError):
        ops.item_zoe_depth(torch.ones(3, 4, 4), [[0], []], np.ones((1, 2)))
    with pytest.raises(ValueError):
        ops.item_zoe_depth(torch.ones(3, 4, 4), [[0]] * 5, np.ones((5, 2)))
    with pytest.raises(ValueError):
        ops.item_zoe_depth(torch.ones(3, 4, 4), [[0] * 65], np.ones((65, 2)))
