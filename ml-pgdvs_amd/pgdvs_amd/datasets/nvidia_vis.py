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
mirrored (upstream's own branch reads an attribute it never sets).  ``resident=True``: the source frames are decoded once
and the items built from a ``datasets.resident.SceneStore`` (see ``nvidia_eval``); ``device_resize=True``: their
images are resized on the device; ``device_decode=True``: their .jpg files are decoded there.
"""
import numpy as np
import torch

from ._common import F32, device_depth as check_device_depth, device_input, flat_cam, flow_entries, group_entries, mono_size, tracker_entries
from .mono_vis import render_path, select_frames_for_time
from .nvidia_eval import (ALL_SCENE_IDS_NVIDIA_DYN, N_CAMS, TGT_HEIGHT, NvidiaDynEvaluationDataset, read_llff_cams,
                          spatial_depth_range)
from .resident import DEFAULT_MAX_BYTES
from .static_aggregation import hwf_to_K


class NvidiaDynVisualizationDataset(NvidiaDynEvaluationDataset):
    dataset_name = "NVIDIA_Dyn Visualization"
    dataset_fname = "nvidia_vis"

    def __init__(self, *, data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir, max_hw, mode,
                 rgb_range="0_1", use_aug=False, scene_ids=None, n_src_views_spatial=10,
                 n_src_views_temporal_track_one_side=5, use_zoe_depth="none", zoe_depth_data_f=None,
                 flow_consist_thres=1.0, vis_center_time=50, n_render_frames=200, vis_time_interval=10, vis_bt_max_disp=32,
                 device=None, resident=False, resident_scenes=1, resident_max_bytes=DEFAULT_MAX_BYTES, device_resize=False,
                 device_decode=False, device_entropy=False, device_png=False, device_mask=False, device_depth=False):
        options = device_input(type(self).__name__, resident=resident, device=device, device_resize=device_resize, device_decode=device_decode,
                               device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        device_depth = check_device_depth(type(self).__name__, options, device_depth)
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
        self._init_resident(resident, resident_scenes, resident_max_bytes, self.depth_device, options, device_depth)
        self._set_dirs(data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir)
        scene_ids = ALL_SCENE_IDS_NVIDIA_DYN if scene_ids is None else scene_ids
        self.c2w_dict, self.hwf_dict, self.valid_fs = {}, {}, []
        for scene in scene_ids:  # (:158-260)
            scene_dir = self.raw_data_dir / scene / "dense"
            all_hwf, all_c2w = read_llff_cams(scene_dir / "poses_bounds_cvd.npy")
            bds = np.load(scene_dir / "poses_bounds_cvd.npy", allow_pickle=True)[:, -2:].astype(np.float32)
            all_hwf[:, 0], all_hwf[:, 1] = mono_size(scene_dir)  # the focal stays at the stored resolution
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
        tgt_shape = mono_size(scene_dir)
        assert tgt_shape[0] == TGT_HEIGHT, tgt_shape
        aug_c2w = self._aug_c2w(tgt_c2w)
        aug_K = np.eye(4)
        aug_K[:3, :3] = hwf_to_K(*all_hwf[0], tgt_shape=tgt_shape)
        if self.store is not None:
            return self._resident_item(
                scene_id, tgt_shape, all_c2w, all_hwf, sel=sel, spatial_ids=spatial_ids, spatial_depth=False, c2w_tgt=aug_c2w,
                trackers=True, fixed={"scene_id": scene_id, "misc": {"scene_id": scene_id, "tgt_time": tgt_time, "tgt_idx": tgt_idx}},
                host={"seq_ids": torch.LongTensor(np.array([tgt_time, *spatial_ids, *sel["temporal"]])),
                      "flat_cam_tgt": F32(flat_cam(*tgt_shape, aug_K, aug_c2w)), "time_tgt": torch.FloatTensor([tgt_time])})
        stack = lambda ids: self._stack_views(scene_id, ids, all_c2w, all_hwf, tgt_shape)  # noqa: E731
        spatial = stack(spatial_ids)
        item = {
            "scene_id": scene_id,
            "seq_ids": torch.LongTensor(np.array([tgt_time, *spatial_ids, *sel["temporal"]])),  # (time truncated, as upstream)
            "flat_cam_tgt": F32(flat_cam(*tgt_shape, aug_K, aug_c2w)),
            "depth_range": spatial_depth_range(spatial, aug_c2w, self.depth_device, type(self).__name__),
            "time_tgt": torch.FloatTensor([tgt_time]),
            "misc": {"scene_id": scene_id, "tgt_time": tgt_time, "tgt_idx": tgt_idx},
        }
        item.update(group_entries("spatial", spatial, depth=False))
        item.update(group_entries("temporal", stack(sel["temporal"]), sel["temporal"], sel["n_actual_temporal"]))
        item.update(flow_entries(self._read_flow(scene_id, sel["temporal"][0], sel["temporal"][1], tgt_shape),
                                 self._read_flow(scene_id, sel["temporal"][1], sel["temporal"][0], tgt_shape)))
        item.update(tracker_entries(sel, stack))
        return item
