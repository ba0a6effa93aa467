"""What tests/test_resident_host.py and tests/test_gpu_resident.py share: the fixture trees, the four loaders over them with
and without ``resident=True``, and the item comparison (same keys, same non-tensor entries, tensors of the same dtype, shape
and bits)."""
import pathlib
import shutil
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402

LOADERS = ("nvidia_eval", "nvidia_pure_geo", "nvidia_vis", "mono_vis")
SCENE_B = "Balloon2"  # the second scene of the eviction test: a name of ALL_SCENE_IDS_NVIDIA_DYN
EVAL_KW = dict(raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1, mode="eval",
               scene_ids=[NT.SCENE], flow_consist_thres=1.0)
MONO_KW = dict(max_hw=-1, mode="vis", scene_ids=[NT.MONO_SCENE], n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
               vis_center_time=4, n_render_frames=16, vis_time_interval=3, vis_bt_max_disp=8)


def build_trees(tmp):
    """{"nvidia": the visualisation tree (the evaluation tree plus its .jpg names), "mono": the monocular tree}"""
    return {"nvidia": VT.build_tree(pathlib.Path(tmp) / "nvidia"), "mono": NT.build_mono_tree(pathlib.Path(tmp) / "mono")}


def add_second_scene(root):
    """the NVIDIA tree's scene copied under a second name"""
    for sub in ("raw", "masks", "depths", "flows"):
        shutil.copytree(pathlib.Path(root) / sub / NT.SCENE, pathlib.Path(root) / sub / SCENE_B)
    return root


def make(name, trees, **kw):
    """loader ``name`` over its tree; ``kw``: device, resident, ... and overrides"""
    from pgdvs_amd.datasets.mono_vis import MonoVisualizationDataset
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset, NvidiaDynPureGeoEvaluationDataset
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    if name == "nvidia_eval":
        return NvidiaDynEvaluationDataset(**{**dict(data_root=trees["nvidia"], n_src_views_spatial=4,
                                                    n_src_views_temporal_track_one_side=2, **EVAL_KW), **kw})
    if name == "nvidia_pure_geo":
        return NvidiaDynPureGeoEvaluationDataset(**{**dict(data_root=trees["nvidia"], **EVAL_KW), **kw})
    if name == "nvidia_vis":
        return NvidiaDynVisualizationDataset(**{**dict(data_root=trees["nvidia"], **VT.KW), **kw})
    assert name == "mono_vis", name
    return MonoVisualizationDataset(**{**dict(data_root=trees["mono"], **MONO_KW), **kw})


def bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()


def assert_items_equal(got, want, what):
    assert got.keys() == want.keys(), (what, sorted(set(got) ^ set(want)))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, torch.Tensor):
            assert isinstance(g, torch.Tensor) and g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(bits(g), bits(w)), (what, k)
        else:
            assert g == w, (what, k)
