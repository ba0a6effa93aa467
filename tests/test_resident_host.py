"""The resident source frames on the host (pgdvs_amd/datasets/resident.py, ``resident=True, device=None``): the four loaders'
items equal the disk loaders' bit for bit over every index of the fixture trees; every source file is read once; scenes
leave and come back as ``resident_scenes`` says; an item never aliases the store; the byte cap and ZoeDepth inputs are
refused; the library exports the two kernels' entry points."""
import pathlib
import re
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import resident_cases as RC  # noqa: E402
from resident_cases import NT, VT  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("resident"))


@pytest.fixture()
def stub_cloud(monkeypatch):
    """the pure-geometry loader aggregates its static cloud on a GPU at construction; the cloud is not what is compared here"""
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynPureGeoEvaluationDataset

    cloud = torch.arange(30, dtype=torch.float32).reshape(5, 6)
    monkeypatch.setattr(NvidiaDynPureGeoEvaluationDataset, "_aggregate_static_pcl", lambda self, scene_id: cloud)


@pytest.mark.parametrize("name", RC.LOADERS)
def test_items_equal_the_disk_loaders(name, trees, stub_cloud):
    """every index: the first and last frames (placeholder temporal pair, padded tracker windows) and, for the evaluation
    loaders, targets in and out of the monocular video"""
    disk, res = RC.make(name, trees, device=None), RC.make(name, trees, device=None, resident=True)
    assert len(disk) == len(res) > 0
    for i in range(len(disk)):
        RC.assert_items_equal(res[i], disk[i], (name, i))
    assert res.store.stats["items_built"] == len(disk)
    n_frames = NT.MF if name == "mono_vis" else NT.F
    assert res.store.stats["frames_decoded"] == n_frames and res.store.nbytes > 0
    if name in ("nvidia_eval", "nvidia_pure_geo"):
        in_mono = [frame_id % NT.N_CAMS == cam_id for _, _, frame_id, cam_id, _ in disk.valid_fs]
        assert 0 < sum(in_mono) < len(disk)


class _Opens:
    """counts PIL.Image.open and np.load per file"""

    def __init__(self, monkeypatch):
        self.paths = []
        real_open, real_load = PIL.Image.open, np.load

        def counted(real):
            def f(path, *a, **kw):
                self.paths.append(pathlib.Path(path))
                return real(path, *a, **kw)
            return f

        monkeypatch.setattr(PIL.Image, "open", counted(real_open))
        monkeypatch.setattr(np, "load", counted(real_load))

    def take(self):
        got, self.paths = self.paths, []
        return got


@pytest.mark.parametrize("name", ["nvidia_vis", "mono_vis"])
def test_every_source_file_is_read_once(name, trees, monkeypatch):
    ds = RC.make(name, trees, device=None, resident=True)
    opens = _Opens(monkeypatch)
    for i in range(len(ds)):
        ds[i]
    first = opens.take()
    assert first and len(first) == len(set(first)), sorted(p for p in set(first) if first.count(p) > 1)
    images = [p for p in first if p.parent.name in ("rgbs",) or "mv_images" in p.parts]
    masks = [p for p in first if p.name.endswith("_final.png")]
    depths = [p for p in first if p.parent.name in ("disp", "depths")]
    flows = [p for p in first if p.parent.name.startswith("interval_")]
    assert len(images) + len(masks) + len(depths) + len(flows) == len(first), first
    assert len(images) == len(masks) == len(depths) == ds.store.stats["frames_decoded"] > 0
    assert len(flows) == ds.store.stats["flow_files_read"] > 0
    for i in range(len(ds)):
        ds[i]
    assert opens.take() == []
    assert ds.store.stats["items_built"] == 2 * len(ds) and ds.store.stats["frames_decoded"] == len(images)


def test_two_scenes_and_eviction(tmp_path):
    trees = {"nvidia": RC.add_second_scene(VT.build_tree(tmp_path / "nvidia"))}
    kw = dict(scene_ids=[NT.SCENE, RC.SCENE_B])
    disk = RC.make("nvidia_vis", trees, device=None, **kw)
    n = len(disk) // 2
    a, b = 3, n + 10
    assert disk[a]["scene_id"] == NT.SCENE and disk[b]["scene_id"] == RC.SCENE_B
    decoded = {}
    for scenes in (1, 2):
        res = RC.make("nvidia_vis", trees, device=None, resident=True, resident_scenes=scenes, **kw)
        counts = []
        for i in (a, b, a):
            RC.assert_items_equal(res[i], disk[i], (scenes, i))
            counts.append(res.store.stats["frames_decoded"])
        decoded[scenes] = counts
        assert len(res.store.scenes) == scenes
    n_a, n_b = decoded[1][0], decoded[1][1] - decoded[1][0]
    assert n_a > 0 and n_b > 0
    assert decoded[1] == [n_a, n_a + n_b, 2 * n_a + n_b]  # one scene stays: A is decoded again
    assert decoded[2] == [n_a, n_a + n_b, n_a + n_b]      # both stay: A is decoded once


@pytest.mark.parametrize("name", ["nvidia_vis", "nvidia_eval"])
def test_items_do_not_alias_the_store(name, trees):
    disk, res = RC.make(name, trees, device=None), RC.make(name, trees, device=None, resident=True)
    i = 10
    want = disk[i]
    first = res[i]
    RC.assert_items_equal(first, want, (name, "first"))
    for v in first.values():
        if isinstance(v, torch.Tensor):
            v.fill_(7)
    RC.assert_items_equal(res[i], want, (name, "after writing into the first item"))


def test_byte_cap_is_checked_before_any_file_is_read(trees, monkeypatch):
    from pgdvs_amd.datasets import resident

    need = resident.table_bytes(NT.F, NT.H, NT.W)
    assert need == NT.F * NT.H * NT.W * 8  # 3 + 1 + 4 bytes per pixel, the slots of this size unpadded
    assert resident.table_bytes(3, 5, 7) == 3 * (112 + 48 + 144)  # 105, 35 and 140 bytes padded to 16
    ds = RC.make("nvidia_vis", trees, device=None, resident=True, resident_max_bytes=need - 1)
    opens = _Opens(monkeypatch)
    with pytest.raises(ValueError, match=str(need)):
        ds[0]
    assert opens.take() == [] and ds.store.nbytes == 0 and not ds.store.scenes
    for name in ("nvidia_eval", "mono_vis"):
        with pytest.raises(ValueError, match="resident_max_bytes"):
            RC.make(name, trees, device=None, resident=True, resident_max_bytes=1000)[0]
    # flow pairs beyond the cap leave, least recently used first; the tables stay
    pair = NT.H * NT.W * 12
    ds = RC.make("nvidia_vis", trees, device=None, resident=True, resident_max_bytes=need + 3 * pair)
    disk = RC.make("nvidia_vis", trees, device=None)
    for i in range(len(ds)):
        RC.assert_items_equal(ds[i], disk[i], i)
        assert ds.store.nbytes <= need + 3 * pair
    scene = ds.store.scenes[NT.SCENE]
    assert len(scene.flows) == 3 and ds.store.nbytes == need + 3 * pair
    read = ds.store.stats["flow_files_read"]
    RC.assert_items_equal(ds[3], disk[3], "again")  # its pairs had left: both files are read again
    assert ds.store.stats["flow_files_read"] == read + 2 and ds.store.nbytes == need + 3 * pair


def test_zoe_depth_and_numpy_thresholds_are_refused(trees):
    with pytest.raises(ValueError, match="use_zoe_depth"):
        RC.make("nvidia_eval", trees, device=None, resident=True, use_zoe_depth="nk", zoe_depth_data_path="zoe")
    with pytest.raises(TypeError):
        RC.make("nvidia_vis", trees, device=None, resident=True, flow_consist_thres=np.float64(1.0))
    with pytest.raises(ValueError):
        RC.make("nvidia_vis", trees, device="cpu", resident=True)
    # the default stays the disk path
    assert RC.make("nvidia_vis", trees, device=None).store is None and RC.make("mono_vis", trees, device=None).store is None


def test_library_exports_the_kernels_and_ops_refuse_host_tensors():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pgdvs_hip.h").read_text(), flags=re.S)
    for name in ("pgdvs_item_views", "pgdvs_flow_occ"):
        assert hasattr(lib, name), name
        m = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "item_gather.hip" in (ROOT / "ml-pgdvs_amd" / "csrc" / "Makefile").read_text()
    with pytest.raises(ops.PgdvsHipError):
        ops.item_views(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 2, 2), [([0], True)])
    with pytest.raises(ops.PgdvsHipError):
        ops.flow_occ(torch.zeros(2, 2, 2), 1.0)
    # the entry points validate on the host before anything is launched
    import ctypes as C

    ids, sizes, out = (C.c_int32 * 1)(5), (C.c_int32 * 1)(1), (C.c_void_p * 5)(16, 16, 16, 16, 0)
    assert lib.pgdvs_item_views(C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 3, 2, 2, 16, 16, 16, ids, 1, sizes, 1, out, None) == -1
    assert b"ids[0] = 5" in lib.pgdvs_last_error()
    assert lib.pgdvs_flow_occ(C.c_void_p(8), 0, 4, 1.0, C.c_void_p(8), None) == -1
