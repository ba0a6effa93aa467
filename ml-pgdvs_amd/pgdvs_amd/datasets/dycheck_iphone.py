"""On-disk DyCheck iPhone scene -> the renderer's ``data`` dict.

Mirror of ``pgdvs.datasets.dycheck_iphone_eval.DyCheckiPhoneEvaluationDataset`` (pgdvs/datasets/dycheck_iphone_eval.py:35-983)
with the parts of ``iPhoneParser`` (pgdvs/datasets/dycheck_utils.py:11-360) and ``DyCheckCamera``
(pgdvs/utils/dycheck/camera.py) it uses: same constructor keywords, same ``valid_fs`` order, same ``__getitem__`` keys /
shapes / dtypes / values (``misc`` included), so a ``DataLoader`` over it feeds ``PGDVSRenderer.forward`` and
``harness.eval_step(..., quant_type="dycheck_iphone")`` as upstream's does.

Host code is numpy + PIL (input plumbing), except the per-item ``depth_range[H,W,2]`` (:455-524): with ``device=None`` it
is computed in numpy statement for statement as upstream; with a GPU ``device`` by the HIP op ``ops.dycheck_depth_range``,
bit-identical (DESIGN.md, row 8f-3 DyCheck).  Differences, all outside what the fixture exercises: no zip containers, no
undistortion (upstream asserts it off; distortion terms are read and ignored), and resizes that upstream does with OpenCV
(image ``INTER_AREA``, depth ``INTER_NEAREST``; taken only when a file's size differs from the target's) use PIL's BOX /
NEAREST filters.  The point clouds upstream computes for the temporal and tracker views and then discards are skipped.

``resident=True`` (with ``resident_scenes``, ``resident_max_bytes``; Python keywords only): every train frame is decoded once
and kept in a ``datasets.resident.SceneStore`` on ``device`` (None: host memory), slots addressed by time id; what is derived
from the camera JSON files is cached per scene, time id and camera; the items' source views are built from the store, on a
GPU by ``ops.item_views`` in one launch, with ``depth_range`` left on the device and the target's colour and covisible bytes
expanded by ``ops.item_target``: the same keys in the same order, shapes, dtypes and bits, every tensor on the store's
device.  ``device_resize=True`` (what each ``device_*`` keyword builds on: datasets/resident.py): a train frame whose file is not of the
scene's size goes to the store as decoded and is BOX-resized on the device; the target sets the item's size
and is never resized.  The default is the disk path, unchanged.
"""
import json
import os
import pathlib

import numpy as np
import PIL.Image
import torch
from torch.utils.data import Dataset

from ._common import (F32, device_depth as check_device_depth, device_input, flat_cam, flow_entries, group_entries, ray_rows, read_flow_pair_or_zeros, refuse_gpu_in_worker,
                      resize, stack_views, tracker_entries)
from .resident import DEFAULT_MAX_BYTES, SceneStore, build_item

ALL_SCENE_IDS_DYCHECK_IPHONE = ["apple", "block", "paper-windmill", "space-out", "spin", "teddy", "wheel"]


# ---------------------------------------------------------------------------- camera and parser
class DyCheckCamera:
    """The used subset of pgdvs/utils/dycheck/camera.py:9-211 (OpenCV axes: right, down, forward)."""

    def __init__(self, orientation, position, focal_length, principal_point, image_size, skew=0.0, pixel_aspect_ratio=1.0,
                 radial_distortion=None, tangential_distortion=None):
        self.orientation = np.array(orientation, np.float32)
        self.position = np.array(position, np.float32)
        self.focal_length = np.array(focal_length, np.float32)
        self.principal_point = np.array(principal_point, np.float32)
        self.image_size = np.array(image_size, np.uint32)
        self.skew = np.array(skew, np.float32)
        self.pixel_aspect_ratio = np.array(pixel_aspect_ratio, np.float32)
        # read for completeness; undistortion is off upstream (dycheck_utils.py:56-57)
        self.radial_distortion = np.array([0, 0, 0] if radial_distortion is None else radial_distortion, np.float32)
        self.tangential_distortion = np.array([0, 0] if tangential_distortion is None else tangential_distortion, np.float32)

    @classmethod
    def fromjson(cls, filename):
        with open(filename) as f:
            d = json.load(f)
        if "tangential" in d:  # old camera JSON (camera.py:75-77)
            d["tangential_distortion"] = d["tangential"]
        return cls(orientation=np.asarray(d["orientation"]), position=np.asarray(d["position"]), focal_length=d["focal_length"],
                   principal_point=np.asarray(d["principal_point"]), image_size=np.asarray(d["image_size"]), skew=d["skew"],
                   pixel_aspect_ratio=d["pixel_aspect_ratio"], radial_distortion=np.asarray(d["radial_distortion"]),
                   tangential_distortion=np.asarray(d["tangential_distortion"]))

    def copy(self):
        c = DyCheckCamera.__new__(DyCheckCamera)
        c.__dict__ = {k: np.copy(v) for k, v in self.__dict__.items()}
        return c

    def rescale_image_domain(self, scale):
        if scale <= 0:
            raise ValueError("scale needs to be positive.")
        c = self.copy()
        c.focal_length *= scale  # in place on float32: the product is rounded to float32 (the skew is not rescaled)
        c.principal_point *= scale
        c.image_size = np.array((int(round(self.image_size[0] * scale)), int(round(self.image_size[1] * scale))))
        return c

    def translate(self, transl):
        c = self.copy()
        c.position += transl
        return c

    def rescale(self, scale):
        if scale <= 0:
            raise ValueError("scale needs to be positive.")
        c = self.copy()
        c.position *= scale
        return c

    @property
    def translation(self):
        return -self.orientation @ self.position

    @property
    def intrin(self):
        return np.array([[self.focal_length, self.skew, self.principal_point[0]],
                         [0, self.focal_length * self.pixel_aspect_ratio, self.principal_point[1]], [0, 0, 1]], np.float32)

    @property
    def extrin(self):
        """4x4 world-to-camera transform (float32)."""
        return np.concatenate([np.concatenate([self.orientation, self.translation[..., None]], axis=-1),
                               np.array([[0, 0, 0, 1]], np.float32)], axis=-2)


class iPhoneParser:  # noqa: N801 -- upstream's name
    """Reads ``scene.json``, ``dataset.json``, ``metadata.json``, ``extra.json`` and ``splits/`` of one sequence
    (dycheck_utils.py:11-360).  As upstream, missing ``splits/*.json`` are WRITTEN on construction (train = camera 0,
    val = every other camera, :286-309); the ``splits`` directory is created first, as DyCheck's own ``io.dump`` does
    (upstream's ``open`` would fail on a missing directory)."""

    SPLITS = ["train", "val"]

    def __init__(self, sequence, *, data_root, use_undistort=False):
        assert not use_undistort
        self.sequence = sequence
        self.data_root = data_root
        self.data_dir = os.path.join(data_root, sequence)
        with open(os.path.join(self.data_dir, "scene.json")) as f:
            sc = json.load(f)
        self._center = np.array(sc["center"], np.float32)
        self._scale, self._near, self._far = sc["scale"], sc["near"], sc["far"]
        with open(os.path.join(self.data_dir, "dataset.json")) as f:
            names = np.array(json.load(f)["ids"])
        with open(os.path.join(self.data_dir, "metadata.json")) as f:
            meta = json.load(f)
        self._time_ids = np.array([meta[k]["warp_id"] for k in names], np.uint32)
        self._camera_ids = np.array([meta[k]["camera_id"] for k in names], np.uint32)
        self._frame_names_map = np.zeros((self._time_ids.max() + 1, self._camera_ids.max() + 1), names.dtype)
        for i, (t, c) in enumerate(zip(self._time_ids, self._camera_ids)):
            self._frame_names_map[t, c] = names[i]
        with open(os.path.join(self.data_dir, "extra.json")) as f:
            ex = json.load(f)
        self._factor, self._fps = ex["factor"], ex["fps"]
        self._bbox = np.array(ex["bbox"], np.float32)
        self._lookat, self._up = np.array(ex["lookat"], np.float32), np.array(ex["up"], np.float32)
        self.splits_dir = os.path.join(self.data_dir, "splits")
        if not os.path.exists(self.splits_dir):
            self._create_splits()

    def _create_splits(self):
        os.makedirs(self.splits_dir, exist_ok=True)
        for split in self.SPLITS:
            mask = self.camera_ids == 0 if split == "train" else self.camera_ids != 0
            d = {"camera_ids": self.camera_ids[mask].tolist(), "frame_names": self.frame_names[mask].tolist(),
                 "time_ids": self.time_ids[mask].tolist()}
            with open(os.path.join(self.splits_dir, f"{split}.json"), "w") as f:
                json.dump(d, f, sort_keys=True, indent=4, separators=(",", ": "))

    def load_split(self, split):
        assert split in self.SPLITS
        with open(os.path.join(self.splits_dir, f"{split}.json")) as f:
            d = json.load(f)
        return np.array(d["frame_names"]), np.array(d["time_ids"], np.uint32), np.array(d["camera_ids"], np.uint32)

    def get_frame_name(self, time_id, camera_id):
        return self._frame_names_map[time_id, camera_id]

    def rgb_path(self, time_id, camera_id):
        """the file ``load_rgba`` opens"""
        return os.path.join(self.data_dir, "rgb", f"{self._factor}x", self._frame_names_map[time_id, camera_id] + ".png")

    def load_rgba(self, time_id, camera_id):
        path = os.path.join(self.data_dir, "rgb", f"{self._factor}x", self._frame_names_map[time_id, camera_id] + ".png")
        if not os.path.exists(path):
            raise ValueError(f"RGB image not found: {path}.")
        rgba = np.array(PIL.Image.open(path))
        if rgba.shape[-1] == 3:
            rgba = np.concatenate([rgba, np.full_like(rgba[..., :1], 255)], axis=-1)
        return rgba

    def depth_path(self, time_id, camera_id):
        return os.path.join(self.data_dir, "depth", f"{self._factor}x", self._frame_names_map[time_id, camera_id] + ".npy")

    def load_depth(self, time_id, camera_id):
        return np.load(self.depth_path(time_id, camera_id), allow_pickle=True) * self.scale

    def load_camera(self, time_id, camera_id):
        name = self._frame_names_map[time_id, camera_id]
        return (DyCheckCamera.fromjson(os.path.join(self.data_dir, "camera", name + ".json"))
                .rescale_image_domain(1 / self._factor).translate(-self._center).rescale(self._scale))

    def covisible_path(self, time_id, camera_id, split):
        """the file ``load_covisible`` opens; a missing one is refused as there"""
        path = os.path.join(self.data_dir, "covisible", f"{self._factor}x", split, self._frame_names_map[time_id, camera_id] + ".png")
        if not os.path.exists(path):
            raise ValueError(f"Covisible image not found: {path}.")
        return path

    def load_covisible(self, time_id, camera_id, split):
        return np.array(PIL.Image.open(self.covisible_path(time_id, camera_id, split)))

    frame_names = property(lambda self: self._frame_names_map[self.time_ids, self.camera_ids])
    time_ids = property(lambda self: self._time_ids)
    camera_ids = property(lambda self: self._camera_ids)
    center = property(lambda self: self._center)
    scale = property(lambda self: self._scale)
    near = property(lambda self: self._near)
    far = property(lambda self: self._far)
    factor = property(lambda self: self._factor)


# ---------------------------------------------------------------------------- selection rules
def _angular_dist_rot(R1, R2):
    """batched_angular_dist_rot_matrix (pgdvs/datasets/base.py:583-603)"""
    return np.arccos(np.clip((np.trace(np.matmul(R2.transpose(0, 2, 1), R1), axis1=1, axis2=2) - 1) / 2.0, -1 + 1e-6, 1 - 1e-6))


def sort_poses_dist_matrix(tgt_pose, ref_poses):
    """sort_poses_wrt_ref(dist_method="dist_matrix", tgt_id=-1) (base.py:413-474): normalised rotation angle plus
    normalised centre distance, ascending."""
    b = tgt_pose[None, ...].repeat(len(ref_poses), 0)
    d1 = _angular_dist_rot(b[:, :3, :3], ref_poses[:, :3, :3])
    d1 = (d1 - np.min(d1)) / (np.max(d1) - np.min(d1) + 1e-8)
    d2 = np.linalg.norm(b[:, :3, 3] - ref_poses[:, :3, 3], axis=1)
    d2 = (d2 - np.min(d2)) / (np.max(d2) - np.min(d2) + 1e-8)
    return np.argsort(d1 + d2)


def select_temporal_frames(tgt_time_id, train_time_ids, n_track_one_side):
    """Temporally closest train frames and the tracker windows (dycheck_iphone_eval.py:227-311).  DyCheck's train time ids
    are consecutive, so a target inside their range is itself a train instant: one neighbour plus the placeholder duplicate."""
    t_ids = train_time_ids
    lo, hi = min(t_ids), max(t_ids)
    temporal = []
    if tgt_time_id in t_ids:
        temporal.append(tgt_time_id)
    else:
        if tgt_time_id > lo:
            temporal.append(max(t for t in t_ids if t < tgt_time_id))
        if tgt_time_id < hi:
            temporal.append(min(t for t in t_ids if t > tgt_time_id))
    assert len(set(temporal)) == len(temporal), temporal
    temporal = sorted(temporal)
    n_actual = len(temporal)
    if n_actual == 1:
        temporal.append(temporal[0])  # placeholder duplicate (:263-265)
    fwd = [temporal[0] for _ in range(n_track_one_side)]
    n_fwd = 0
    if tgt_time_id > lo:
        tmp = np.arange(max(lo, temporal[0] - n_track_one_side), temporal[0]).tolist()
        n_fwd = len(tmp)
        for i in range(n_fwd):
            if tmp[i] in t_ids:
                fwd[-(n_fwd - i)] = tmp[i]
    bwd = [temporal[1] for _ in range(n_track_one_side)]
    n_bwd = 0
    if tgt_time_id < hi:
        tmp = np.arange(temporal[1] + 1, min(hi + 1, temporal[1] + 1 + n_track_one_side)).tolist()
        n_bwd = len(tmp)
        for i in range(n_bwd):
            if tmp[i] in t_ids:
                bwd[i] = tmp[i]
    return {"temporal": temporal, "n_actual_temporal": n_actual, "fwd2tgt": fwd, "n_actual_fwd2tgt": n_fwd,
            "bwd2tgt": bwd, "n_actual_bwd2tgt": n_bwd}


def kmeans_labels(centres, n_clusters):
    """sklearn KMeans(n_clusters, random_state=0, n_init="auto") on the train camera centres -> (centres, labels)
    (:357-366); sklearn is imported here, so only the clustered selection needs it."""
    from sklearn.cluster import KMeans

    km = KMeans(n_clusters=n_clusters, random_state=0, n_init="auto").fit(centres)
    return km.cluster_centers_, km.labels_


def select_spatial_frames(view_type, tgt_time_id, raw_c2w_tgt, train_time_ids, train_c2w, n_views, clusters=None):
    """The three ``spatial_src_view_type`` rules (:313-400), sorted ascending.  ``clusters`` = (centres, labels) of the
    scene's KMeans fit for "clustered".  Quirk kept: the clustered rule returns INDICES into the train list (:379-393),
    which upstream then uses as time ids."""
    if view_type == "closest_wo_temporal":
        order = sort_poses_dist_matrix(raw_c2w_tgt, np.copy(train_c2w))
        ids = [train_time_ids[i] for i in order][:n_views]
    elif view_type == "closest_with_temporal":
        dist = np.abs(np.array(train_time_ids).astype(np.float32) - float(tgt_time_id))
        pool = train_time_ids[np.argsort(dist)[: n_views * 4].tolist()]
        lo = min(train_time_ids)
        order = sort_poses_dist_matrix(raw_c2w_tgt, np.copy(train_c2w[[t - lo for t in pool], ...]))
        ids = pool[order][:n_views]
    elif view_type == "clustered":
        centres, labels = clusters
        assert len(set(labels.tolist())) == len(centres), (len(set(labels.tolist())), len(centres))
        order = np.argsort(np.linalg.norm(centres - raw_c2w_tgt[:3, 3].reshape((1, 3)), axis=1))
        ids = []
        for lab in order[:n_views]:
            members = np.nonzero(labels == lab)[0]
            ids.append(members[np.argsort(np.abs(members.astype(np.float32) - float(tgt_time_id))).tolist()[0]])
    else:
        raise ValueError(view_type)
    assert len(set(ids)) == len(ids), ids
    return sorted(ids)


# ---------------------------------------------------------------------------- geometry
def _fma32(a, b, c):
    """float32 fused multiply-add a*b + c, correctly rounded (float64 product is exact; TwoSum carries the sum's error,
    which decides the rare case where the float64 sum sits exactly between two float32 values)."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf))).astype(np.float64)
    mid = (s != r64) & (s - r64 == other - s) & (e != 0) & (np.sign(e) == np.sign(other - s))
    return np.where(mid, other, r64).astype(np.float32)


def ray_constants(K, c2w):
    """Per-view ray constants as _get_rays_single_image forms them (base.py:507-546): c2w and K cast to torch float32,
    M = c2w[:3,:3] @ inverse(K[:3,:3]) (torch bmm), origin c2w[:3,3].  Returns float32 (M[3,3], o[3])."""
    K_t, c2w_t = torch.FloatTensor(np.asarray(K))[None, ...], torch.FloatTensor(np.asarray(c2w))[None, ...]
    M = c2w_t[:, :3, :3].bmm(torch.inverse(K_t[:, :3, :3]))[0]
    return M.numpy().astype(np.float32), c2w_t[0, :3, 3].numpy().astype(np.float32)


def compute_pcl(h, w, M, o, depth):
    """_compute_pcl (:903-910): rays_o + rays_d * depth through integer pixel centres.  torch's CPU bmm forms rays_d with
    fused multiply-adds over k ascending (DESIGN.md 8f-3 DyCheck): d = fma(M[:,1], v, M[:,0] u) + M[:,2]."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    u, v = u.reshape(-1), v.reshape(-1)
    d = np.stack([_fma32(M[ax, 1], v, M[ax, 0] * u) + M[ax, 2] for ax in range(3)], axis=1)  # [HW,3] float32
    return o[None, :] + d * depth.reshape((-1, 1))


def depth_range_numpy(pcl_src_spatial, dyn_mask_src_spatial, raw_c2w_tgt, flat_cam_tgt, near, far, tgt_h, tgt_w):
    """Per-pixel depth range [H,W,2], statement for statement as dycheck_iphone_eval.py:455-524 (float32 result)."""
    coords_world_homo = np.pad(pcl_src_spatial, ((0, 0), (0, 1)), "constant", constant_values=1)
    coords_cam_tgt = np.matmul(np.linalg.inv(raw_c2w_tgt), coords_world_homo.T).T
    depth_range_min = max(near, np.quantile(coords_cam_tgt[:, 2], 0.1))
    depth_range_max = min(far, np.quantile(coords_cam_tgt[:, 2], 0.9))
    depth_range = np.tile(np.array([depth_range_min, depth_range_max]).reshape((1, 1, 2)), (tgt_h, tgt_w, 1))
    flat_static = dyn_mask_src_spatial.reshape((-1)) == 0
    assert flat_static.shape[0] == pcl_src_spatial.shape[0]
    if np.sum(flat_static) > 0:
        static_pcl = pcl_src_spatial[flat_static, :]
        tgt_K = flat_cam_tgt[2:18].reshape((4, 4))
        tgt_c2w = flat_cam_tgt[18:34].reshape((4, 4))
        homo = np.pad(static_pcl, ((0, 0), (0, 1)), mode="constant", constant_values=1)
        cam = np.matmul(np.linalg.inv(tgt_c2w), homo.T).T[:, :3]
        static_depth = cam[:, 2]
        pix = np.matmul(tgt_K[:3, :3], cam.T).T
        pix = pix[:, :2] / (pix[:, 2:] + 1e-8)
        valid = (pix[:, 1] >= 0) & (pix[:, 1] <= tgt_h - 1) & (pix[:, 0] >= 0) & (pix[:, 0] <= tgt_w - 1)
        if np.sum(valid) > 0:
            pix = np.round(pix[valid, :].astype(int)).astype(int)  # astype(int) truncates; the round is a no-op
            z = static_depth[valid]
            depth_range[pix[:, 1], pix[:, 0], 0] = z - 1e-4  # duplicates: the last point wins
            depth_range[pix[:, 1], pix[:, 0], 1] = z + 1e-4
    return depth_range.astype(np.float32)


# ---------------------------------------------------------------------------- dataset
class DyCheckiPhoneEvaluationDataset(Dataset):
    dataset_name = "DyCheck iPhone Eval"
    dataset_fname = "dycheck_iphone_eval"

    def __init__(self, *, data_root, raw_data_dir, mask_data_dir, flow_data_dir, max_hw, mode, rgb_range="0_1", use_aug=False,
                 scene_ids=None, spatial_src_view_type="clustered", n_src_views_spatial=10, n_src_views_spatial_cluster=None,
                 n_src_views_temporal_track_one_side=5, flow_consist_thres=1.0, device=None, resident=False, resident_scenes=1,
                 resident_max_bytes=DEFAULT_MAX_BYTES, device_resize=False, device_decode=False, device_entropy=False, device_png=False,
                 device_mask=False, device_depth=False):
        options = device_input(type(self).__name__, resident=resident, device=device, device_resize=device_resize, device_decode=device_decode,
                               device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        device_depth = check_device_depth(type(self).__name__, options, device_depth)
        assert max_hw == -1, f"We enforce to use raw resolution. However, we receive max_hw of {max_hw}"
        assert not use_aug
        assert mode in ["eval"], mode
        assert rgb_range == "0_1", rgb_range
        self.mode, self.max_hw, self.use_aug, self.rgb_range = mode, max_hw, use_aug, rgb_range
        self.n_src_views_spatial = n_src_views_spatial
        self.spatial_src_view_type = spatial_src_view_type
        self.n_src_views_spatial_cluster = n_src_views_spatial if n_src_views_spatial_cluster is None else n_src_views_spatial_cluster
        self.n_src_views_temporal_track_one_side = n_src_views_temporal_track_one_side
        self.flow_consist_thres = flow_consist_thres
        self.device = None if device is None else torch.device(device)
        # resident source frames (datasets/resident.py): the store, and per scene the frame size and the cameras' derived values
        self.store = (SceneStore(self.device, resident_scenes, resident_max_bytes, flow_consist_thres, device_input=options, device_depth=device_depth)
                      if resident else None)
        self._scene_shape, self._cam_cache = {}, {}
        root = pathlib.Path(data_root)
        self.raw_data_dir, self.mask_data_dir, self.flow_data_dir = root / raw_data_dir, root / mask_data_dir, root / flow_data_dir
        for d in (self.raw_data_dir, self.mask_data_dir, self.flow_data_dir):
            assert d.exists(), d
        scene_ids = ALL_SCENE_IDS_DYCHECK_IPHONE if scene_ids is None else scene_ids
        self.parser_dict, self.train_info_dict = {}, {}
        all_data = []
        for scene_id in scene_ids:
            p = self.parser_dict[scene_id] = iPhoneParser(scene_id, data_root=self.raw_data_dir)
            names, t_ids, c_ids = p.load_split("train")
            assert len(names) == len(t_ids) == len(c_ids), (len(names), len(t_ids), len(c_ids))
            assert len(t_ids) == max(t_ids) - min(t_ids) + 1, "train time ids must be consecutive"
            info = {"frame_names": names, "time_ids": t_ids.astype(int), "camera_ids": c_ids.astype(int),
                    "unique_ids": [(names[i], t_ids[i], c_ids[i]) for i in range(len(names))]}
            info["train_c2w"] = np.array([np.linalg.inv(p.load_camera(t_ids[i], c_ids[i]).extrin) for i in range(len(names))])
            self.train_info_dict[scene_id] = info
            v_names, v_t, v_c = p.load_split("val")
            assert len(v_names) == len(v_t) == len(v_c)
            all_data += [(scene_id, v_names[i], v_t[i], v_c[i]) for i in range(len(v_names))]
        assert len(set(all_data)) == len(all_data)
        self.valid_fs = sorted(set(all_data))  # same order on every worker / rank
        self._clusters = {}

    def __len__(self):
        return len(self.valid_fs)

    def get_train_cam_id(self, scene_id):
        c = self.train_info_dict[scene_id]["camera_ids"]
        assert len(set(c)) == 1, set(c)
        return c[0]

    def scene_clusters(self, scene_id):
        """The scene's KMeans fit on the train camera centres.  Upstream refits per item on the same data with a fixed
        seed; the fit is cached here per scene (tests check the cached labels against a fresh fit)."""
        if scene_id not in self._clusters:
            self._clusters[scene_id] = kmeans_labels(self.train_info_dict[scene_id]["train_c2w"][:, :3, 3], self.n_src_views_spatial_cluster)
        return self._clusters[scene_id]

    # ------------------------------------------------------------------ one view
    def _process_view(self, scene_id, time_id, cam_id, tgt_shape, with_geometry):
        """_process_for_single_src_view (:777-901) for aug "none": rgb [0,1], flat_cam[34] and, for source views, the
        dynamic mask, depth and the ray constants of _compute_pcl."""
        p = self.parser_dict[scene_id]
        raw = p.load_rgba(time_id, cam_id)[..., :3]
        cam = p.load_camera(time_id, cam_id)
        K, w2c = cam.intrin, cam.extrin
        h, w = tgt_shape
        raw = resize(raw, h, w, PIL.Image.Resampling.BOX)
        out = {}
        if with_geometry:
            name = p.get_frame_name(time_id, cam_id)
            m = np.array(PIL.Image.open(self.mask_data_dir / scene_id / f"masks/final/{name}_final.png"))  # True = dynamic
            out["dyn_mask"] = resize(m, h, w, PIL.Image.Resampling.NEAREST).astype(np.float32)
            depth = p.load_depth(time_id, cam_id)[..., 0]
            out["depth"] = resize(depth, h, w, PIL.Image.Resampling.NEAREST)
        # base.augment_cam("none") inverts twice more: every inverse is LAPACK's float32 one, as upstream
        c2w = np.linalg.inv(np.linalg.inv(np.linalg.inv(w2c)))
        K4 = np.eye(4)
        K4[:3, :3] = K
        rgb = raw.astype(np.float32) / 255.0
        if with_geometry:
            out["dyn_rgb"] = rgb * out["dyn_mask"][..., None]
            out["static_rgb"] = rgb * (1 - out["dyn_mask"][..., None])
            out["K"], out["c2w"] = K4, c2w
        out["rgb"] = rgb
        out["flat_cam"] = flat_cam(h, w, K4, c2w)
        return out

    def _stack_views(self, scene_id, time_ids, tgt_shape):
        cam_id = self.get_train_cam_id(scene_id)
        return stack_views([self._process_view(scene_id, t, cam_id, tgt_shape, True) for t in time_ids])

    def _read_flow(self, scene_id, src_time_id, tgt_time_id, tgt_shape):
        """:920-983 -- zeros for the placeholder pair; otherwise flows/interval_k/<a>_<b>.npz with the occlusion mask
        sum|coord_diff| > flow_consist_thres."""
        return read_flow_pair_or_zeros(self._flow_path(scene_id, src_time_id, tgt_time_id), tgt_shape, self.flow_consist_thres)

    def _flow_path(self, scene_id, src_time_id, tgt_time_id):
        """the pair's file; None for the placeholder pair (a frame with itself)"""
        if src_time_id == tgt_time_id:
            return None
        p, cam = self.parser_dict[scene_id], self.get_train_cam_id(scene_id)
        return (self.flow_data_dir / f"{scene_id}" / f"flows/interval_{abs(tgt_time_id - src_time_id)}" /
                f"{p.get_frame_name(src_time_id, cam)}_{p.get_frame_name(tgt_time_id, cam)}.npz")

    def _depth_range(self, spatial, raw_c2w_tgt, flat_cam_tgt, near, far, tgt_shape):
        h, w = tgt_shape
        rays = [ray_constants(K, c2w) for K, c2w in zip(spatial["K"], spatial["c2w"])]
        if self.device is None:
            pcl = np.concatenate([compute_pcl(h, w, M, o, d) for (M, o), d in zip(rays, spatial["depth"])], axis=0)
            return torch.from_numpy(depth_range_numpy(pcl, spatial["dyn_mask"], raw_c2w_tgt, flat_cam_tgt, near, far, h, w))
        refuse_gpu_in_worker(type(self).__name__)
        from .. import ops

        dev = self.device
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        out = ops.dycheck_depth_range(
            T(spatial["depth"]), T(spatial["dyn_mask"]), T(ray_rows(rays)),
            np.linalg.inv(raw_c2w_tgt), np.linalg.inv(flat_cam_tgt[18:34].reshape((4, 4))), flat_cam_tgt[2:18].reshape((4, 4))[:3, :3],
            near, far)
        return out.cpu()

    # ------------------------------------------------------------------ resident source frames (datasets/resident.py)
    def _scene_frame_shape(self, scene_id):
        """(h, w) of the scene's tables: the size of its first train frame, from the file's header"""
        if scene_id not in self._scene_shape:
            p, info = self.parser_dict[scene_id], self.train_info_dict[scene_id]
            with PIL.Image.open(os.path.join(p.data_dir, "rgb", f"{p.factor}x", info["frame_names"][0] + ".png")) as im:
                self._scene_shape[scene_id] = (im.size[1], im.size[0])
        return self._scene_shape[scene_id]

    def _cam(self, scene_id, time_id, cam_id):
        """what __getitem__, _process_view and _depth_range derive from a frame's camera JSON, by the same statements, made
        once: raw_c2w (the inverse of extrin), K4, the thrice-inverted c2w, flat_cam and the ray constants"""
        key = (scene_id, int(time_id), int(cam_id))
        c = self._cam_cache.get(key)
        if c is None:
            cam = self.parser_dict[scene_id].load_camera(time_id, cam_id)
            K, w2c = cam.intrin, cam.extrin
            c2w = np.linalg.inv(np.linalg.inv(np.linalg.inv(w2c)))
            K4 = np.eye(4)
            K4[:3, :3] = K
            c = self._cam_cache[key] = {"raw_c2w": np.linalg.inv(w2c), "K4": K4, "c2w": c2w, "rays": ray_constants(K4, c2w),
                                        "flat_cam": flat_cam(*self._scene_frame_shape(scene_id), K4, c2w)}
        return c

    def _decode_frame(self, scene_id, time_id, shape):
        """(image uint8, dynamic mask, depth) of a train frame at the scene's size, as _process_view reads them"""
        p, cam_id, (h, w) = self.parser_dict[scene_id], self.get_train_cam_id(scene_id), shape
        if self.store.device_resize:  # the image as the store decodes it (device_png: on the device); the store resizes it
            raw = self._store_rgb(p, time_id, cam_id, into=(self.store.scenes.get(scene_id), time_id))
        else:
            raw = resize(p.load_rgba(time_id, cam_id)[..., :3], h, w, PIL.Image.Resampling.BOX)
        if self.store.device_mask:  # the mask as the store decodes it, in its slot where the device path serves the file
            mask = self.store.decode_mask(self._mask_f(scene_id, time_id), (h, w), into=(self.store.scenes.get(scene_id), time_id))
        else:
            mask = resize(np.array(PIL.Image.open(self._mask_f(scene_id, time_id))), h, w, PIL.Image.Resampling.NEAREST)
        staged = self.store.staged_depth(self.store.scenes.get(scene_id), time_id)
        if staged is not None and staged.depth is not None:  # (device_depth: the fill placed depth * scale, float32, in the slot)
            return raw, mask, staged.depth
        depth = p.load_depth(time_id, cam_id)
        if depth.dtype == np.float64:
            raise ValueError(f"{p.depth_path(time_id, cam_id)}: the depth times the scene's scale is float64; resident=True keeps "
                             "float32 depths, and the disk path would take the depth range over the doubles")
        return raw, mask, resize(depth[..., 0], h, w, PIL.Image.Resampling.NEAREST)

    def _depth_request(self, scene_id, time_id):
        """``device_depth``: a train frame's depth file and ``load_depth``'s statement over it, as ``SceneStore._stage_depths`` takes
        them -- where ``depth * scale`` is float32 on the host (a Python number as the scale); else None: the host statement"""
        p = self.parser_dict[scene_id]
        if (np.zeros(1, np.float32) * p.scale).dtype != np.float32:
            return None
        return p.depth_path(time_id, self.get_train_cam_id(scene_id)), None, "scale", np.float32(p.scale)

    def _mask_f(self, scene_id, time_id):
        """a train frame's final mask file"""
        name = self.parser_dict[scene_id].get_frame_name(time_id, self.get_train_cam_id(scene_id))
        return self.mask_data_dir / scene_id / f"masks/final/{name}_final.png"

    def _store_rgb(self, p, time_id, cam_id, **kw):
        """``load_rgba(...)[..., :3]`` through the store's ``decode_image``: the same bytes, the missing file's error included"""
        path = p.rgb_path(time_id, cam_id)
        if not os.path.exists(path):
            raise ValueError(f"RGB image not found: {path}.")
        return self.store.decode_image(path, channels="rgb", **kw)

    @staticmethod
    def _item_key_order():
        """the disk item's keys in its order"""
        def group(name, timed):
            return [f"{k}_src_{name}" for k in ("rgb", "dyn_rgb", "static_rgb", "flat_cam", "dyn_mask", "depth") + (("time",) if timed else ())] + \
                ([f"n_actual_{name}"] if timed else [])

        return (["scene_id", "seq_ids", "rgb_tgt", "eval_mask", "flat_cam_tgt", "depth_range", "time_tgt", "misc"] + group("spatial", False) +
                group("temporal", True) + ["flow_fwd", "flow_fwd_occ_mask", "flow_bwd", "flow_bwd_occ_mask"] +
                group("temporal_track_fwd2tgt", True) + group("temporal_track_bwd2tgt", True))

    def _resident_item(self, index):
        """``resident.build_item`` over this loader's readers and cached cameras.  The target image and the covisible mask, one
        item's each, stay disk reads; on a GPU store they cross as bytes in the item's packed copy and ``ops.item_target``
        expands them there"""
        scene_id, tgt_frame_name, tgt_time_id, tgt_cam_id = self.valid_fs[index]
        info, p = self.train_info_dict[scene_id], self.parser_dict[scene_id]
        assert (tgt_frame_name, tgt_time_id, tgt_cam_id) not in info["unique_ids"]
        shape, dev, cam_id = self._scene_frame_shape(scene_id), self.store.device, self.get_train_cam_id(scene_id)
        tgt_cam = self._cam(scene_id, tgt_time_id, tgt_cam_id)
        raw_c2w_tgt, flat_cam_tgt = tgt_cam["raw_c2w"], tgt_cam["flat_cam"]
        sel = select_temporal_frames(tgt_time_id, info["time_ids"], self.n_src_views_temporal_track_one_side)
        clusters = self.scene_clusters(scene_id) if self.spatial_src_view_type == "clustered" else None
        spatial_ids = select_spatial_frames(self.spatial_src_view_type, tgt_time_id, raw_c2w_tgt, info["time_ids"], info["train_c2w"],
                                            self.n_src_views_spatial, clusters)
        frame_ids = np.array([tgt_time_id, *spatial_ids, *sel["temporal"]]).astype(int)
        tgt_rgb = (self._store_rgb(p, tgt_time_id, tgt_cam_id, target=True) if self.store.device_resize else
                   p.load_rgba(tgt_time_id, tgt_cam_id)[..., :3])
        tgt_shape = tuple(tgt_rgb.shape[:2])
        if self.store.device_mask:  # decoded on the device where that path serves the file: no host bytes cross
            covis = self.store.decode_mask(p.covisible_path(tgt_time_id, tgt_cam_id, "val"))
        else:
            covis = p.load_covisible(tgt_time_id, tgt_cam_id, "val")
        assert tuple(covis.shape[:2]) == tgt_shape, (covis.shape, tgt_shape)
        if tuple(tgt_shape) != shape:
            raise ValueError(f"{scene_id}: target {tgt_frame_name} is {tuple(tgt_shape)}, the scene's tables hold frames of {shape}")
        train = {int(t) for t in info["time_ids"]}
        for t in (*spatial_ids, *sel["temporal"], *sel["fwd2tgt"], *sel["bwd2tgt"]):  # (the disk path's order)
            if int(t) not in train:  # e.g. the clustered rule's train-list indices: no slot is touched
                self._process_view(scene_id, t, cam_id, tgt_shape, True)  # raises what the disk path raises
                raise ValueError(f"{scene_id}: frame id {int(t)} is no train frame ({min(train)}..{max(train)})")
        host = {"seq_ids": torch.LongTensor(frame_ids), "flat_cam_tgt": F32(np.array(flat_cam_tgt)),
                "time_tgt": torch.FloatTensor([tgt_time_id])}
        on_device = isinstance(tgt_rgb, torch.Tensor)  # (device_png decoded it there: uint8 [H,W,3])
        as_bytes = on_device or (dev is not None and tgt_rgb.dtype == np.uint8 and tgt_rgb.ndim == 3 and tgt_rgb.shape[2] == 3)
        if on_device:
            pass
        elif as_bytes:
            host["__rgb_tgt"] = torch.from_numpy(np.ascontiguousarray(tgt_rgb))
        else:
            host["rgb_tgt"] = F32(tgt_rgb.astype(np.float32) / 255.0)
        covis_on_device = isinstance(covis, torch.Tensor)  # (device_mask decoded it there: uint8 [H,W])
        if covis_on_device and not as_bytes:  # (no byte target beside it: the host statement below)
            covis, covis_on_device = covis.cpu().numpy(), False
        if covis_on_device:
            pass
        elif as_bytes and covis.ndim == 2 and covis.dtype in (np.bool_, np.uint8):
            host["__covisible"] = torch.from_numpy(np.ascontiguousarray(covis).view(np.uint8))
        else:
            host["eval_mask"] = F32((covis > 0).astype(np.float32))[..., None]

        def cams(ids):
            cs = [self._cam(scene_id, t, cam_id) for t in ids]
            return tuple(np.stack([c[k] for c in cs]) for k in ("flat_cam", "K4", "c2w"))

        def depth_range(depth, dyn_mask, rays):
            if dev is None:
                pcl = np.concatenate([compute_pcl(*shape, r[:9].reshape(3, 3), r[9:], d) for r, d in zip(rays, depth.numpy())], axis=0)
                return torch.from_numpy(depth_range_numpy(pcl, dyn_mask.numpy(), raw_c2w_tgt, flat_cam_tgt, p.near, p.far, *shape))
            from .. import ops

            return ops.dycheck_depth_range(depth, dyn_mask, rays, np.linalg.inv(raw_c2w_tgt), np.linalg.inv(flat_cam_tgt[18:34].reshape((4, 4))),
                                           flat_cam_tgt[2:18].reshape((4, 4))[:3, :3], p.near, p.far)

        scene = self.store.scene(scene_id, len(info["time_ids"]), shape, first_id=int(min(info["time_ids"])))
        item = build_item(self.store, scene, lambda t: self._decode_frame(scene_id, t, shape),
                          fixed={"scene_id": scene_id, "misc": {"scene_id": scene_id, "tgt_frame_id": tgt_time_id, "tgt_cam_id": tgt_cam_id,
                                                                "tgt_frame_name": tgt_frame_name}},
                          host=host, cams=cams, sel=sel, spatial_ids=spatial_ids, spatial_depth=True, c2w_tgt=None,
                          flow_path=lambda a, b: self._flow_path(scene_id, a, b),
                          trackers=True, owner=type(self).__name__, depth_range=depth_range,
                          ray_rows=lambda ids: ray_rows([self._cam(scene_id, t, cam_id)["rays"] for t in ids]),
                          image_path=lambda t: (p.rgb_path(t, cam_id), "rgb"), mask_path=lambda t: self._mask_f(scene_id, t),
                          depth_request=lambda t: self._depth_request(scene_id, t))
        if as_bytes:
            from .. import ops

            rgb, mask = ops.item_target(tgt_rgb if on_device else item.pop("__rgb_tgt"), covis if covis_on_device else item.pop("__covisible", None))
            item["rgb_tgt"] = rgb
            if mask is not None:
                item["eval_mask"] = mask
        order = self._item_key_order()
        assert len(order) == len(item), sorted(set(order) ^ set(item))
        return {k: item[k] for k in order}

    # ------------------------------------------------------------------ item
    def __getitem__(self, index):
        if self.store is not None:
            return self._resident_item(index)
        scene_id, tgt_frame_name, tgt_time_id, tgt_cam_id = self.valid_fs[index]
        info, p = self.train_info_dict[scene_id], self.parser_dict[scene_id]
        assert (tgt_frame_name, tgt_time_id, tgt_cam_id) not in info["unique_ids"]
        raw_c2w_tgt = np.linalg.inv(p.load_camera(tgt_time_id, tgt_cam_id).extrin)
        sel = select_temporal_frames(tgt_time_id, info["time_ids"], self.n_src_views_temporal_track_one_side)
        clusters = self.scene_clusters(scene_id) if self.spatial_src_view_type == "clustered" else None
        spatial_ids = select_spatial_frames(self.spatial_src_view_type, tgt_time_id, raw_c2w_tgt, info["time_ids"], info["train_c2w"],
                                            self.n_src_views_spatial, clusters)
        frame_ids = np.array([tgt_time_id, *spatial_ids, *sel["temporal"]]).astype(int)
        tgt_rgb = p.load_rgba(tgt_time_id, tgt_cam_id)[..., :3]
        tgt_shape = tgt_rgb.shape[:2]
        covis = (p.load_covisible(tgt_time_id, tgt_cam_id, "val") > 0).astype(np.float32)
        assert covis.shape[:2] == tgt_shape, (covis.shape, tgt_shape)
        tgt = self._process_view(scene_id, tgt_time_id, tgt_cam_id, tgt_shape, False)
        spatial = self._stack_views(scene_id, spatial_ids, tgt_shape)
        depth_range = self._depth_range(spatial, raw_c2w_tgt, tgt["flat_cam"], p.near, p.far, tgt_shape)
        stack = lambda ids: self._stack_views(scene_id, ids, tgt_shape)  # noqa: E731
        ret = {"scene_id": scene_id, "seq_ids": torch.LongTensor(frame_ids), "rgb_tgt": F32(tgt["rgb"]),
               "eval_mask": F32(covis)[..., None], "flat_cam_tgt": F32(tgt["flat_cam"]), "depth_range": depth_range,
               "time_tgt": torch.FloatTensor([tgt_time_id]),
               "misc": {"scene_id": scene_id, "tgt_frame_id": tgt_time_id, "tgt_cam_id": tgt_cam_id, "tgt_frame_name": tgt_frame_name}}
        ret.update(group_entries("spatial", spatial))
        ret.update(group_entries("temporal", stack(sel["temporal"]), sel["temporal"], sel["n_actual_temporal"]))
        ret.update(flow_entries(self._read_flow(scene_id, sel["temporal"][0], sel["temporal"][1], tgt_shape),
                                self._read_flow(scene_id, sel["temporal"][1], sel["temporal"][0], tgt_shape)))
        ret.update(tracker_entries(sel, stack))
        return ret
