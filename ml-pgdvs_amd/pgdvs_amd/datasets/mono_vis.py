"""In-the-wild monocular video -> the renderer's ``data`` dict along a bullet-time camera path.

Mirror of ``pgdvs.datasets.mono_vis.MonoVisualizationDataset`` (pgdvs/datasets/mono_vis.py:34-738):
same constructor keywords, same per-scene directory layout (the one the reference's preprocessing
writes: ``rgbs/``, ``poses/*.npz {K, c2w}``, ``depths/*.npz {depth}``, ``masks/final/*_final.png``,
``flows/interval_k/<a>_<b>.npz {flow, coord_diff}``), same ``__getitem__`` keys and values.

The target cameras are not input cameras: ``n_render_frames`` time stamps are spread around
``vis_center_time``; at each, the pose is interpolated between the two neighbouring input poses
(linear translation, quaternion slerp exactly as the reference evaluates it -- without a
shortest-arc sign flip or re-normalisation, ``utils/geometry.py:468-515``) and composed with a
small circular "bullet-time" offset whose radius follows the scene's near depth
(``nvidia_vis.py:692-722``).

Host-side numpy / PIL input plumbing, like ``datasets/nvidia_eval.py``; resizes that upstream
does with OpenCV (only taken when files differ in size) use PIL filters.  ``depth_range`` comes from
``nvidia_eval.spatial_depth_range``: numpy with ``device=None``, the HIP op on a GPU ``device``.  ``resident=True``: the
source frames are decoded once and the items built from a ``datasets.resident.SceneStore``.
"""
import pathlib
from math import acos, sin

import numpy as np
import PIL.Image
import torch
from torch.utils.data import Dataset

from ._common import (F32, device_depth as check_device_depth, device_input, flat_cam, flow_entries, group_entries, read_flow_pair_or_zeros, resize, stack_views,
                      tracker_entries)
from .nvidia_eval import spatial_depth_range
from .resident import DEFAULT_MAX_BYTES, SceneStore, build_item

N_BT_REPS = 8


# ---------------------------------------------------------------------------- camera path
def rotmat_to_qvec(R):
    """(w, x, y, z) of a rotation matrix, COLMAP's eigenvector form (utils/geometry.py:448-465)."""
    Rxx, Ryx, Rzx, Rxy, Ryy, Rzy, Rxz, Ryz, Rzz = np.asarray(R).flat
    K = np.array([
        [Rxx - Ryy - Rzz, 0, 0, 0],
        [Ryx + Rxy, Ryy - Rxx - Rzz, 0, 0],
        [Rzx + Rxz, Rzy + Ryz, Rzz - Rxx - Ryy, 0],
        [Ryz - Rzy, Rzx - Rxz, Rxy - Ryx, Rxx + Ryy + Rzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


def qvec_to_rotmat(q):
    w, x, y, z = q
    return np.array([
        [1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
        [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
        [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


def interpolate_pose(c2w_a, c2w_b, ratio):
    """pose at ``ratio`` in [0,1] between two camera-to-world matrices (utils/geometry.py:468-515)"""
    qa, qb = rotmat_to_qvec(c2w_a[:3, :3]), rotmat_to_qvec(c2w_b[:3, :3])
    theta = acos(float(np.dot(qa, qb)))
    q = qa if theta == 0 else (sin((1 - ratio) * theta) * qa + sin(ratio * theta) * qb) / sin(theta)
    out = np.eye(4)
    out[:3, :3] = qvec_to_rotmat(q)
    out[:3, 3] = c2w_a[:3, 3] + (c2w_b[:3, 3] - c2w_a[:3, 3]) * ratio
    return out


def bullet_time_offsets(focal, num_frames, sc, max_disp):
    """inverse of small circular translations in the image plane (nvidia_vis.py:692-722)"""
    max_trans = (max_disp / sc if sc is not None else max_disp) / focal
    poses = []
    for i in range(num_frames):
        t = np.eye(4)
        t[0, 3] = max_trans * np.sin(2.0 * np.pi * float(i) / float(num_frames))
        t[1, 3] = max_trans * np.cos(2.0 * np.pi * float(i) / float(num_frames)) / 2.0
        poses.append(np.linalg.inv(t))
    return poses


def render_path(focal, all_c2w, near_depths, *, vis_center_time, n_render_frames, vis_time_interval, vis_bt_max_disp):
    """[(time, index, c2w)] of the visualisation cameras of one scene (:113-197; nvidia_vis.py:158-260): ``focal`` sizes the
    bullet-time offsets, ``near_depths`` their scale"""
    n = all_c2w.shape[0]
    times = np.linspace(max(0, vis_center_time - vis_time_interval), min(n - 2, vis_center_time + vis_time_interval),
                        n_render_frames).tolist()
    bt_sc = 1.0 / (np.percentile(near_depths, 5) * 0.9)
    offsets = bullet_time_offsets(focal, len(times) // N_BT_REPS, bt_sc, vis_bt_max_disp) * (N_BT_REPS + 1)
    path = []
    for i, t in enumerate(times):
        t0 = int(np.floor(t))
        path.append((t, i, interpolate_pose(all_c2w[t0], all_c2w[t0 + 1], t - np.floor(t)) @ offsets[i]))
    return path


def select_frames_for_time(tgt_time, n_frames, n_track_one_side):
    """the two input frames around a fractional time stamp and the tracker windows (:281-336; note
    the newer-side window starts AT the newer frame and is one longer, as upstream)"""
    older, newer = int(np.floor(tgt_time)), int(np.floor(tgt_time)) + 1
    temporal = sorted(set(([older] if tgt_time > 0 else []) + ([newer] if tgt_time < n_frames - 1 else [])))
    if len(temporal) == 1:
        temporal = temporal * 2
    n_actual = len(temporal)  # (counted after the placeholder, as upstream :300-305)
    fwd = [temporal[0]] * n_track_one_side
    fwd_actual = list(range(max(0, older - n_track_one_side), temporal[0])) if tgt_time > 0 else []
    fwd[: len(fwd_actual)] = fwd_actual
    bwd = [temporal[1]] * n_track_one_side
    bwd_actual = list(range(newer, min(n_frames, newer + 1 + n_track_one_side))) if tgt_time < n_frames - 1 else []
    bwd[: len(bwd_actual)] = bwd_actual
    return {"temporal": temporal, "n_actual_temporal": n_actual, "fwd2tgt": fwd, "n_actual_fwd2tgt": len(fwd_actual),
            "bwd2tgt": bwd, "n_actual_bwd2tgt": len(bwd_actual)}


# ---------------------------------------------------------------------------- dataset
class MonoVisualizationDataset(Dataset):
    dataset_name = "Monocular Visualization"
    dataset_fname = "mono_vis"

    def __init__(self, *, data_root, max_hw, mode, rgb_range="0_1", use_aug=False, scene_ids=None, n_src_views_spatial=10,
                 n_src_views_temporal_track_one_side=5, vis_center_time=50, n_render_frames=200, vis_time_interval=10,
                 vis_bt_max_disp=32, flow_consist_thres=1.0, device=None, resident=False, resident_scenes=1,
                 resident_max_bytes=DEFAULT_MAX_BYTES, device_resize=False, device_decode=False, device_entropy=False, device_png=False,
                 device_mask=False, device_depth=False):
        options = device_input(type(self).__name__, resident=resident, device=device, device_resize=device_resize, device_decode=device_decode,
                               device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        device_depth = check_device_depth(type(self).__name__, options, device_depth)
        assert max_hw == -1, f"We enforce to use raw resolution. However, we receive max_hw of {max_hw}"
        assert not use_aug and mode in ["vis"] and rgb_range == "0_1" and scene_ids is not None
        self.mode, self.max_hw, self.use_aug, self.rgb_range = mode, max_hw, use_aug, rgb_range
        self.n_src_views_spatial = n_src_views_spatial
        self.n_src_views_temporal_track_one_side = n_src_views_temporal_track_one_side
        self.flow_consist_thres = flow_consist_thres
        self.depth_device = None if device is None else torch.device(device)
        # the source frames kept in memory (datasets/resident.py)
        self.store = (SceneStore(self.depth_device, resident_scenes, resident_max_bytes, flow_consist_thres, device_input=options, device_depth=device_depth)
                      if resident else None)
        self.data_root = pathlib.Path(data_root)
        assert self.data_root.exists(), self.data_root
        self.c2w_dict, self.K_dict, self.valid_fs = {}, {}, []
        for scene in scene_ids:
            sd = self.data_root / scene
            cams = [np.load(f) for f in sorted((sd / "poses").glob("*.npz"))]
            all_K, all_c2w = np.array([c["K"] for c in cams]), np.array([c["c2w"] for c in cams])
            if device_depth:  # each file read once, the payloads selected on the device, one wait per scene (resident.py)
                near = np.array(self.store.depth_percentiles(sorted((sd / "depths").glob("*.npz")), "depth", 5))
            else:
                near = np.array([np.percentile(np.load(f)["depth"].reshape(-1), 5) for f in sorted((sd / "depths").glob("*.npz"))])
            self.c2w_dict[scene], self.K_dict[scene] = all_c2w.copy(), all_K.copy()
            for t, i, c2w in render_path(all_K[0, 0, 0], all_c2w, near, vis_center_time=vis_center_time, n_render_frames=n_render_frames,
                                         vis_time_interval=vis_time_interval, vis_bt_max_disp=vis_bt_max_disp):
                self.valid_fs.append([scene, sd, t, i, c2w, 1.0])

    def __len__(self):
        return len(self.valid_fs)

    @staticmethod
    def _mask_f(scene_dir, img_f):
        return scene_dir / "masks" / "final" / f"{pathlib.Path(img_f).stem}_final.png"

    @staticmethod
    def _decode_frame(scene_dir, img_f, tgt_shape, raw=None, resize_rgb=True, mask=None, depth=None):
        """(image uint8, dynamic mask, depth) of an input frame at the target's size; ``raw``: the image file's pixels, where
        the caller has opened it already; ``resize_rgb`` False (``device_resize``): the image as decoded, the store resizes it;
        ``mask`` (``device_mask``): the mask at the target's size as the store decoded it; ``depth`` (``device_depth``): the depth
        as the fill placed it in its slot"""
        h, w = tgt_shape
        rgb = np.array(PIL.Image.open(img_f)) if raw is None else raw
        if resize_rgb:
            rgb = resize(rgb, h, w, PIL.Image.Resampling.BOX)
        name = pathlib.Path(img_f).stem
        if mask is None:
            mask = resize(np.array(PIL.Image.open(scene_dir / "masks" / "final" / f"{name}_final.png")), h, w, PIL.Image.Resampling.NEAREST)
        if depth is None:
            depth = resize(np.load(scene_dir / "depths" / f"{name}.npz")["depth"], h, w, PIL.Image.Resampling.NEAREST)
        return rgb, mask, depth

    def _source_view(self, scene_dir, img_f, c2w, K, tgt_shape):
        h, w = tgt_shape
        rgb, mask, depth = self._decode_frame(scene_dir, img_f, tgt_shape)
        rgb, mask = rgb.astype(np.float32) / 255.0, mask.astype(np.float32)
        return {"rgb": rgb, "flat_cam": flat_cam(h, w, K, c2w), "dyn_mask": mask, "depth": depth, "dyn_rgb": rgb * mask[..., None],
                "static_rgb": rgb * (1 - mask[..., None]), "K": np.asarray(K), "c2w": np.asarray(c2w)}

    def _stack_views(self, scene_dir, img_fs, frame_ids, all_c2w, all_K, tgt_shape):
        return stack_views([self._source_view(scene_dir, img_fs[f], all_c2w[f], all_K[f], tgt_shape) for f in frame_ids])

    @staticmethod
    def _flow_path(scene_dir, img_fs, a, b):
        """the pair's flow file; None for the placeholder pair (a frame with itself)"""
        return None if a == b else scene_dir / "flows" / f"interval_{abs(b - a)}" / f"{img_fs[a].stem}_{img_fs[b].stem}.npz"

    def _read_flow(self, scene_dir, img_fs, a, b, tgt_shape):
        return read_flow_pair_or_zeros(self._flow_path(scene_dir, img_fs, a, b), tgt_shape, self.flow_consist_thres)

    def _tgt_shape(self, scene_id, scene_dir, img_fs):
        """(h, w) of frame 0, the items' size.  With the store the opened frame goes into its slot, so its files are read once."""
        if self.store is None:
            return np.array(PIL.Image.open(img_fs[0])).shape[:2]
        scene = self.store.scenes.get(scene_id)
        if scene is None:
            raw = self.store.decode_image(img_fs[0])  # (device_decode: a JPEG frame comes back on the device)
            scene = self.store.scene(scene_id, len(img_fs), tuple(raw.shape[:2]))
            decode = lambda f: self._decode_frame(scene_dir, img_fs[0], tuple(raw.shape[:2]), raw=raw, mask=self._store_mask(scene_dir, img_fs[0], scene, 0),  # noqa: E731
                                                  depth=self._store_depth(scene, 0))
            if self.store.device_depth:  # a fill of the one frame: its depth is placed like every other frame's
                self.store._fill(scene, [0], decode, depth_request=lambda f: self._depth_request(scene_dir, img_fs[f]))
            else:
                self.store.put(scene, 0, *decode(0))
        return scene.h, scene.w

    def _store_mask(self, scene_dir, img_f, scene, f):
        """``device_mask``: the frame's mask as the store decodes it (in its slot where the device path serves the file); else None"""
        return self.store.decode_mask(self._mask_f(scene_dir, img_f), (scene.h, scene.w), into=(scene, f)) if self.store.device_mask else None

    def _store_depth(self, scene, f):
        """``device_depth``: the frame's depth where the fill placed it in its slot; else None (the host statement reads the file)"""
        staged = self.store.staged_depth(scene, f)
        return None if staged is None else staged.depth

    @staticmethod
    def _depth_request(scene_dir, img_f):
        """the frame's depth file and this loader's statement over it, as ``SceneStore._stage_depths`` takes them: ``depth`` as it is"""
        return scene_dir / "depths" / f"{pathlib.Path(img_f).stem}.npz", "depth", "copy", 1.0

    def _resident_item(self, scene_id, scene_dir, img_fs, shape, all_c2w, all_K, **kw):
        """``resident.build_item`` over this loader's readers and cameras"""
        def cams(ids):
            return np.stack([flat_cam(*shape, all_K[f], all_c2w[f]) for f in ids]), all_K[list(ids)], all_c2w[list(ids)]

        scene = self.store.scene(scene_id, len(img_fs), shape)

        def decode(f):  # device_resize: the image as the store decodes it, at the file's size
            raw = self.store.decode_image(img_fs[f], into=(scene, f)) if self.store.device_resize else None
            return self._decode_frame(scene_dir, img_fs[f], shape, raw=raw, resize_rgb=not self.store.device_resize,
                                      mask=self._store_mask(scene_dir, img_fs[f], scene, f), depth=self._store_depth(scene, f))

        return build_item(self.store, scene, decode, cams=cams, image_path=lambda f: img_fs[f], mask_path=lambda f: self._mask_f(scene_dir, img_fs[f]),
                          depth_request=lambda f: self._depth_request(scene_dir, img_fs[f]),
                          flow_path=lambda a, b: self._flow_path(scene_dir, img_fs, a, b), owner=type(self).__name__, **kw)

    def __getitem__(self, index):
        scene_id, scene_dir, tgt_time, tgt_idx, tgt_c2w, _ = self.valid_fs[index]
        exts = {ex for ex, f in PIL.Image.registered_extensions().items() if f in PIL.Image.OPEN}
        img_fs = sorted(f for f in (pathlib.Path(scene_dir) / "rgbs").iterdir() if f.suffix in exts)
        all_c2w, all_K = self.c2w_dict[scene_id].copy(), self.K_dict[scene_id].copy()
        n = len(img_fs)
        assert n == all_c2w.shape[0] == all_K.shape[0], (n, all_c2w.shape, all_K.shape)
        sel = select_frames_for_time(tgt_time, n, self.n_src_views_temporal_track_one_side)
        d = np.linalg.norm(tgt_c2w[None, :3, 3] - all_c2w[:, :3, 3], axis=1)
        spatial_ids = sorted(np.argsort(d)[: self.n_src_views_spatial].tolist())
        tgt_h, tgt_w = self._tgt_shape(scene_id, scene_dir, img_fs)
        shape = (tgt_h, tgt_w)
        if self.store is not None:
            return self._resident_item(
                scene_id, scene_dir, img_fs, shape, all_c2w, all_K, sel=sel, spatial_ids=spatial_ids, spatial_depth=False,
                c2w_tgt=tgt_c2w, trackers=True,
                fixed={"scene_id": scene_id, "misc": {"scene_id": scene_id, "tgt_time": tgt_time, "tgt_idx": tgt_idx}},
                host={"seq_ids": torch.LongTensor(np.array([tgt_time, *spatial_ids, *sel["temporal"]])),
                      "flat_cam_tgt": F32(flat_cam(tgt_h, tgt_w, all_K[0], tgt_c2w)), "time_tgt": torch.FloatTensor([tgt_time])})
        stack = lambda ids: self._stack_views(scene_dir, img_fs, ids, all_c2w, all_K, shape)  # noqa: E731
        spatial = stack(spatial_ids)
        item = {
            "scene_id": scene_id,
            "seq_ids": torch.LongTensor(np.array([tgt_time, *spatial_ids, *sel["temporal"]])),  # (time truncated, as upstream)
            "flat_cam_tgt": F32(flat_cam(tgt_h, tgt_w, all_K[0], tgt_c2w)),
            "depth_range": spatial_depth_range(spatial, tgt_c2w, self.depth_device, type(self).__name__),
            "time_tgt": torch.FloatTensor([tgt_time]),
            "misc": {"scene_id": scene_id, "tgt_time": tgt_time, "tgt_idx": tgt_idx},
        }
        item.update(group_entries("spatial", spatial, depth=False))
        item.update(group_entries("temporal", stack(sel["temporal"]), sel["temporal"], sel["n_actual_temporal"]))
        item.update(flow_entries(self._read_flow(scene_dir, img_fs, sel["temporal"][0], sel["temporal"][1], shape),
                                 self._read_flow(scene_dir, img_fs, sel["temporal"][1], sel["temporal"][0], shape)))
        item.update(tracker_entries(sel, stack))
        return item
