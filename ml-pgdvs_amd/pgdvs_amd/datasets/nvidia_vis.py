"""NVIDIA Dynamic Scenes sequence -> the renderer's ``data`` dict along a bullet-time camera path.

Mirror of ``pgdvs.datasets.nvidia_vis.NvidiaDynVisualizationDataset`` (pgdvs/datasets/nvidia_vis.py:46-669), the loader
behind the visualiser config's default ``dataset_list.vis``: same constructor keywords, same ``valid_fs`` order, same
``__getitem__`` keys / shapes / values.  It reads the evaluation tree of ``datasets/nvidia_eval.py``; the target cameras
are the camera path of ``datasets/mono_vis.py`` (slerp between neighbouring input poses composed with a circular
offset), sized by frame 0's full-resolution focal and the 5th percentile of the scene's near bounds.

Upstream behaviours kept: ``n_actual_temporal`` is counted after the placeholder duplicate (always 2); the spatial pool
is +-12 frames around the two temporal frames (not the target), ordered by camera-centre distance to the target pose;
source images are ``mv_images/<frame>/cam<frame % 12 + 1>.jpg``; the target camera goes through
``_compute_cam_info`` / ``augment_cam("none")``, i.e. ``inv(inv(c2w))`` in float64.  ``depth_range`` comes from
``nvidia_eval.spatial_depth_range``: numpy with ``device=None``, the HIP op on a GPU ``device``.  ZoeDepth inputs are not
mirrored (upstream's own branch reads an attribute it never sets).
"""
import pathlib

import numpy as np
import PIL.Image
import torch

from .mono_vis import render_path, select_frames_for_time
from .nvidia_eval import (ALL_SCENE_IDS_NVIDIA_DYN, N_CAMS, TGT_HEIGHT, NvidiaDynEvaluationDataset, read_llff_cams,
                          spatial_depth_range)
from .static_aggregation import hwf_to_K


def _mono_size(scene_dir):
    """(h, w) of the scene's ``images_<W>x288`` directory"""
    mono = list(pathlib.Path(scene_dir).glob(f"images_*x{TGT_HEIGHT}"))
    assert len(mono) == 1, mono
    w, h = (int(x) for x in mono[0].name.split("images_")[1].split("x"))
    return h, w


class NvidiaDynVisualizationDataset(NvidiaDynEvaluationDataset):
    dataset_name = "NVIDIA_Dyn Visualization"
    dataset_fname = "nvidia_vis"

    def __init__(self, *, data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir, max_hw, mode,
                 rgb_range="0_1", use_aug=False, scene_ids=None, n_src_views_spatial=10,
                 n_src_views_temporal_track_one_side=5, use_zoe_depth="none", zoe_depth_data_f=None,
                 flow_consist_thres=1.0, vis_center_time=50, n_render_frames=200, vis_time_interval=10, vis_bt_max_disp=32,
                 device=None):
        assert max_hw == -1, f"We enforce to use raw resolution. However, we receive max_hw of {max_hw}"
        assert not use_aug
        assert mode in ["vis"], mode
        assert rgb_range == "0_1", rgb_range
        if use_zoe_depth != "none":
            raise NotImplementedError("ZoeDepth inputs are read by nvidia_eval only (upstream's visualisation loader never sets the path "
                                      "it reads them from); use the DynIBaR disparities (use_zoe_depth='none')")
        self.mode, self.max_hw, self.use_aug, self.rgb_range = mode, max_hw, use_aug, rgb_range
        self.n_src_views_spatial = n_src_views_spatial
        self.n_src_views_temporal_track_one_side = n_src_views_temporal_track_one_side
        self.flow_consist_thres = flow_consist_thres
        self.depth_device = None if device is None else torch.device(device)
        root = pathlib.Path(data_root)
        self.raw_data_dir, self.depth_data_dir = root / raw_data_dir, root / depth_data_dir
        self.mask_data_dir, self.flow_data_dir = root / mask_data_dir, root / flow_data_dir
        for d in (self.raw_data_dir, self.depth_data_dir, self.mask_data_dir, self.flow_data_dir):
            assert d.exists(), d
        scene_ids = ALL_SCENE_IDS_NVIDIA_DYN if scene_ids is None else scene_ids
        self.c2w_dict, self.hwf_dict, self.valid_fs = {}, {}, []
        for scene in scene_ids:  # (:158-260)
            scene_dir = self.raw_data_dir / scene / "dense"
            all_hwf, all_c2w = read_llff_cams(scene_dir / "poses_bounds_cvd.npy")
            bds = np.load(scene_dir / "poses_bounds_cvd.npy", allow_pickle=True)[:, -2:].astype(np.float32)
            all_hwf[:, 0], all_hwf[:, 1] = _mono_size(scene_dir)  # the focal stays at the stored resolution
            self.c2w_dict[scene], self.hwf_dict[scene] = all_c2w.copy(), all_hwf.copy()
            for t, i, c2w in render_path(all_hwf[0, 2], all_c2w, bds[:, 0], vis_center_time=vis_center_time,
                                         n_render_frames=n_render_frames, vis_time_interval=vis_time_interval,
                                         vis_bt_max_disp=vis_bt_max_disp):
                self.valid_fs.append([scene, scene_dir, t, i, c2w, 1.0])  # pose_sc = 1: poses neither rescaled nor centred

    def _aug_c2w(self, c2w):
        """_compute_cam_info(aug_type="none"): augment_cam returns inv(inv(c2w)) (base.py:100-157), whose zeros are +0.0"""
        return np.linalg.inv(np.linalg.inv(c2w))

    def _src_img_f(self, scene_id, frame_id):
        """_get_img_f_for_src_view (:640-653): camera frame % 12 of time step ``frame``, always a .jpg name"""
        return self.raw_data_dir / scene_id / "dense" / "mv_images" / f"{frame_id:05d}" / f"cam{frame_id % N_CAMS + 1:02d}.jpg"

    def __getitem__(self, index):
        scene_id, scene_dir, tgt_time, tgt_idx, tgt_c2w, _ = self.valid_fs[index]
        all_c2w, all_hwf = self.c2w_dict[scene_id].copy(), self.hwf_dict[scene_id].copy()
        n_frames = all_c2w.shape[0]
        sel = select_frames_for_time(tgt_time, n_frames, self.n_src_views_temporal_track_one_side)
        assert self.n_src_views_spatial < N_CAMS * 2
        pool = list(range(max(0, sel["temporal"][0] - N_CAMS), min(n_frames, sel["temporal"][1] + N_CAMS)))
        d = np.linalg.norm(tgt_c2w[None, :3, 3] - all_c2w[pool, :3, 3], axis=1)  # sort_poses_wrt_ref(dist_method="dist")
        spatial_ids = sorted(pool[i] for i in np.argsort(d)[: self.n_src_views_spatial])
        tgt_shape = _mono_size(scene_dir)
        assert tgt_shape[0] == TGT_HEIGHT, tgt_shape
        aug_c2w = self._aug_c2w(tgt_c2w)
        aug_K = np.eye(4)
        aug_K[:3, :3] = hwf_to_K(*all_hwf[0], tgt_shape=tgt_shape)
        flat_cam_tgt = np.concatenate(([tgt_shape[0], tgt_shape[1]], aug_K.flatten(), aug_c2w.flatten())).astype(np.float32)
        stack = lambda ids: self._stack_views(scene_id, ids, all_c2w, all_hwf, tgt_shape)  # noqa: E731
        spatial = stack(spatial_ids)
        depth_range = spatial_depth_range(spatial, aug_c2w, self.depth_device, type(self).__name__)
        temporal = stack(sel["temporal"])
        flow_fwd, occ_fwd = self._read_flow(scene_id, sel["temporal"][0], sel["temporal"][1], tgt_shape)
        flow_bwd, occ_bwd = self._read_flow(scene_id, sel["temporal"][1], sel["temporal"][0], tgt_shape)
        F32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
        item = {
            "scene_id": scene_id,
            "seq_ids": torch.LongTensor(np.array([tgt_time, *spatial_ids, *sel["temporal"]])),  # (time truncated, as upstream)
            "rgb_src_spatial": F32(spatial["rgb"]), "dyn_rgb_src_spatial": F32(spatial["dyn_rgb"]),
            "static_rgb_src_spatial": F32(spatial["static_rgb"]),
            "n_actual_temporal": torch.LongTensor([sel["n_actual_temporal"]]),
            "rgb_src_temporal": F32(temporal["rgb"]), "dyn_rgb_src_temporal": F32(temporal["dyn_rgb"]),
            "static_rgb_src_temporal": F32(temporal["static_rgb"]),
            "dyn_mask_src_spatial": F32(spatial["dyn_mask"])[..., None], "dyn_mask_src_temporal": F32(temporal["dyn_mask"])[..., None],
            "flow_fwd": F32(flow_fwd), "flow_fwd_occ_mask": F32(occ_fwd)[..., None],
            "flow_bwd": F32(flow_bwd), "flow_bwd_occ_mask": F32(occ_bwd)[..., None],
            "flat_cam_tgt": F32(flat_cam_tgt),
            "flat_cam_src_spatial": F32(spatial["flat_cam"]), "flat_cam_src_temporal": F32(temporal["flat_cam"]),
            "depth_src_temporal": F32(temporal["depth"])[..., None],
            "depth_range": depth_range,
            "time_tgt": torch.FloatTensor([tgt_time]), "time_src_temporal": torch.FloatTensor(sel["temporal"]),
            "misc": {"scene_id": scene_id, "tgt_time": tgt_time, "tgt_idx": tgt_idx},
        }
        for side, key in (("fwd2tgt", "n_actual_fwd2tgt"), ("bwd2tgt", "n_actual_bwd2tgt")):
            tr = stack(sel[side])
            sfx = f"src_temporal_track_{side}"
            item.update({
                f"n_actual_temporal_track_{side}": torch.LongTensor([sel[key]]),
                f"rgb_{sfx}": F32(tr["rgb"]), f"dyn_rgb_{sfx}": F32(tr["dyn_rgb"]), f"static_rgb_{sfx}": F32(tr["static_rgb"]),
                f"dyn_mask_{sfx}": F32(tr["dyn_mask"])[..., None], f"flat_cam_{sfx}": F32(tr["flat_cam"]),
                f"depth_{sfx}": F32(tr["depth"])[..., None], f"time_{sfx}": torch.FloatTensor(sel[side]),
            })
        return item
