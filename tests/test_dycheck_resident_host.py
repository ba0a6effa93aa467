"""The DyCheck loader's resident source frames on the host (``resident=True, device=None``; pgdvs_amd/datasets/resident.py,
dycheck_iphone.py): every item of the fixture tree equals the disk loader's, keys in the disk order, bit for bit, for the
three ``spatial_src_view_type``s, and the items that raise on disk raise the same error; a train frame is decoded once, a
second pass opens no flow file and parses no camera JSON; an item never aliases the store or the camera cache; float64
depths, a byte cap below the tables, ``device="cpu"`` and NumPy thresholds are refused; ``CombinedDataset`` passes the keyword."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import resident_cases as RC  # noqa: E402

KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
          scene_ids=[DT.SCENE], n_src_views_spatial=3, n_src_views_spatial_cluster=4, n_src_views_temporal_track_one_side=2,
          flow_consist_thres=1.0)
TYPES = ("closest_wo_temporal", "closest_with_temporal", "clustered")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DT.build_tree(tmp_path_factory.mktemp("dycheck_resident"))


def make(root, typ="closest_wo_temporal", **kw):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    return DyCheckiPhoneEvaluationDataset(data_root=root, spatial_src_view_type=typ, **{**KW, **kw})


def assert_items_identical(got, want, what):
    """resident_cases.assert_items_equal, and the keys in the same order"""
    assert list(got) == list(want), (what, list(got), list(want))
    RC.assert_items_equal(got, want, what)


def compare_all(res, disk, typ, on_device=False):
    """every index: equal items, or the disk path's ValueError with its message; returns the number of raising items"""
    assert len(res) == len(disk) == len(DT.VAL)
    raised = 0
    for i in range(len(disk)):
        try:
            want = disk[i]
        except ValueError as e:
            with pytest.raises(ValueError) as got:
                res[i]
            assert str(got.value) == str(e) and "RGB image not found" in str(e), (typ, i, str(got.value), str(e))
            raised += 1
            continue
        got = res[i]
        if on_device:
            off = [k for k, v in got.items() if isinstance(v, torch.Tensor) and not v.is_cuda]
            assert not off, (typ, i, off)
        assert_items_identical(got, want, (typ, i))
    return raised


@pytest.mark.parametrize("typ", TYPES)
def test_items_equal_the_disk_loader(tree, typ):
    disk, res = make(tree, typ), make(tree, typ, resident=True)
    assert disk.store is None and res.store is not None and res.store.device is None
    raised = compare_all(res, disk, typ)
    assert (raised > 0) == (typ == "clustered") and raised < len(disk)  # the clustered rule's train-list indices 0..2 are no time ids
    st = res.store.stats
    assert 0 < st["frames_decoded"] <= len(DT.TRAIN_T) and st["items_built"] == len(disk) - raised
    scene = res.store.scenes[DT.SCENE]
    assert (scene.first_id, scene.n_frames, scene.h, scene.w) == (DT.TRAIN_T[0], len(DT.TRAIN_T), DT.H, DT.W)
    assert int(scene.filled.sum()) == st["frames_decoded"]


def test_second_pass_decodes_nothing_and_parses_no_camera(tree, monkeypatch):
    from pgdvs_amd.datasets import _common, dycheck_iphone as D

    res = make(tree, resident=True)
    first = [res[i] for i in range(len(res))]
    st = dict(res.store.stats)
    # (train time ids are consecutive, so every target's temporal pair is the placeholder one: the tree's items read no flow file)
    assert 0 < st["frames_decoded"] <= len(DT.TRAIN_T) and st["flow_files_read"] == 0
    calls = {"json": 0, "flow": 0}
    real_json, real_flow = D.DyCheckCamera.fromjson.__func__, _common.read_flow_npz

    def fromjson(cls, filename):
        calls["json"] += 1
        return real_json(cls, filename)

    def read_flow(*a, **kw):
        calls["flow"] += 1
        return real_flow(*a, **kw)

    monkeypatch.setattr(D.DyCheckCamera, "fromjson", classmethod(fromjson))
    for mod in (_common, sys.modules["pgdvs_amd.datasets.resident"]):
        monkeypatch.setattr(mod, "read_flow_npz", read_flow)
    second = [res[i] for i in range(len(res))]
    assert calls == {"json": 0, "flow": 0}
    assert res.store.stats["frames_decoded"] == st["frames_decoded"] and res.store.stats["flow_files_read"] == st["flow_files_read"]
    assert res.store.stats["items_built"] == 2 * st["items_built"]
    for i, (a, b) in enumerate(zip(first, second)):
        assert_items_identical(b, a, i)
    # the wrapper counts: the disk path parses a camera for every view of every item
    disk = make(tree)
    disk[0]
    assert calls["json"] > 10


def test_items_do_not_alias_the_store(tree):
    disk, res = make(tree), make(tree, resident=True)
    for i in (1, 5):
        want = disk[i]
        first = res[i]
        assert_items_identical(first, want, (i, "first"))
        for v in first.values():
            if isinstance(v, torch.Tensor):
                v.fill_(7)
        assert_items_identical(res[i], want, (i, "after writing into the first item"))


def test_a_real_flow_pair_through_the_store(tree):
    """the tree's items all carry the placeholder pair; a real pair of the train camera, as the store reads and hands it out"""
    from pgdvs_amd.datasets._common import flow_entries

    disk, res = make(tree), make(tree, resident=True)
    res[0]
    scene = res.store.scenes[DT.SCENE]
    want = flow_entries(disk._read_flow(DT.SCENE, 5, 7, (DT.H, DT.W)), disk._read_flow(DT.SCENE, 7, 5, (DT.H, DT.W)))
    for _ in range(2):
        got = {}
        for key, (a, b) in (("fwd", (5, 7)), ("bwd", (7, 5))):
            got[f"flow_{key}"], got[f"flow_{key}_occ_mask"] = res.store.flow(scene, a, b, res._flow_path(DT.SCENE, a, b))
        assert_items_identical(got, want, "flow 5 <-> 7")
    assert res.store.stats["flow_files_read"] == 2 and res._flow_path(DT.SCENE, 6, 6) is None


def test_float64_depths_are_refused(tmp_path):
    root = DT.build_tree(tmp_path)
    f = root / "iphone" / DT.SCENE / f"depth/{DT.FACTOR}x" / f"{DT.frame_name(0, 10)}.npy"
    np.save(f, np.load(f).astype(np.float64))
    res = make(root, resident=True)
    idx = [i for i, e in enumerate(res.valid_fs) if int(e[2]) == 10][0]
    with pytest.raises(ValueError, match=f"{DT.frame_name(0, 10)}.npy"):
        res[idx]
    assert not res.store.scenes[DT.SCENE].filled[10 - DT.TRAIN_T[0]]
    make(root)[idx]  # the disk path takes the file


def test_wrong_sized_target_is_refused(tmp_path):
    import PIL.Image

    root = DT.build_tree(tmp_path)
    cam, t = DT.VAL[1]
    n = DT.frame_name(cam, t)
    PIL.Image.fromarray(np.zeros((DT.H + 2, DT.W, 3), np.uint8)).save(root / "iphone" / DT.SCENE / f"rgb/{DT.FACTOR}x" / f"{n}.png")
    PIL.Image.fromarray(np.zeros((DT.H + 2, DT.W), np.uint8)).save(root / "iphone" / DT.SCENE / f"covisible/{DT.FACTOR}x/val" / f"{n}.png")
    res = make(root, resident=True)
    idx = [i for i, e in enumerate(res.valid_fs) if (int(e[3]), int(e[2])) == (cam, t)][0]
    with pytest.raises(ValueError) as e:
        res[idx]
    assert str((DT.H + 2, DT.W)) in str(e.value) and str((DT.H, DT.W)) in str(e.value)
    assert not res.store.scenes  # nothing was allocated


def test_refusals(tree):
    from pgdvs_amd.datasets import resident

    need = resident.table_bytes(len(DT.TRAIN_T), DT.H, DT.W)
    ds = make(tree, resident=True, resident_max_bytes=need - 1)
    with pytest.raises(ValueError, match="resident_max_bytes"):
        ds[0]
    assert not ds.store.scenes and ds.store.nbytes == 0
    make(tree, resident=True, resident_max_bytes=need + 2 * DT.H * DT.W * 12)[0]
    with pytest.raises(ValueError):
        make(tree, resident=True, device="cpu")
    with pytest.raises(TypeError):
        make(tree, resident=True, flow_consist_thres=np.float64(1.0))
    assert make(tree, flow_consist_thres=np.float64(1.0)).store is None  # the disk path is as it was


def test_combined_dataset_passes_the_keyword(tree):
    from pgdvs_amd.datasets.combined import CombinedDataset
    from pgdvs_amd.instantiate import instantiate, load_config

    ds_cfg = load_config().dataset
    spec = dict(ds_cfg.dataset_specifics.dycheck_iphone_eval)
    spec.update(scene_ids=[DT.SCENE], mask_data_dir="flow_mask", flow_data_dir="flow_mask", n_src_views_spatial=3,
                spatial_src_view_type="closest_wo_temporal", n_src_views_temporal_track_one_side=2, resident=True)
    node = dict(ds_cfg)
    node.update(data_root=tree, dataset_list={"eval": ["dycheck_iphone_eval"]}, dataset_specifics={"dycheck_iphone_eval": spec})
    ds = instantiate(node, mode="eval")
    assert isinstance(ds, CombinedDataset) and ds.datasets["dycheck_iphone_eval"].store is not None
    direct = make(tree, resident=True)
    for i in (0, 2, len(direct) - 1):
        assert_items_identical(ds[i], direct[i], i)
