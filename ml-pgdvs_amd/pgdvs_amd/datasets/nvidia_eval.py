"""On-disk NVIDIA Dynamic Scenes sequence -> the renderer's ``data`` dict.

Mirror of ``pgdvs.datasets.nvidia_eval.NvidiaDynEvaluationDataset``
(pgdvs/datasets/nvidia_eval.py:59-1040) and of
``pgdvs.datasets.nvidia_eval_pure_geo.NvidiaDynPureGeoEvaluationDataset``
(nvidia_eval_pure_geo.py:41-470) for the evaluation configuration the benchmark scripts
use (raw resolution, no augmentation, DynIBaR disparities or aligned ZoeDepth predictions):
same constructor keywords, same directory layout, same ``__getitem__`` keys / shapes / value
conventions, so a ``DataLoader`` over it feeds ``PGDVSRenderer.forward`` exactly like upstream's.

Host-side numpy + PIL (this is input plumbing, not the hot path).  Differences, all outside
what the golden fixtures exercise: resizes that upstream does with OpenCV (image
``INTER_AREA``, depth / evaluation mask ``INTER_NEAREST``; only taken when a file's size
differs from the 288-row target) use PIL's BOX / NEAREST filters.

ZoeDepth inputs (``use_zoe_depth`` = "moe" or one of ``{n,k,nk}_me_{med,trim}_{share,indiv}``,
:116-160, :230-243, :869-945; evaluation loader only, the pure-geometry loader forces "none"
and ``nvidia_vis`` refuses them): ``<zoe_depth_data_path>/<scene>/dense/zoe_depths_{n,k,nk}/
<frame>.npz`` from a directory or from the members ``<stem>/<scene>/...`` of a zip opened
lazily per process.  ``read_zoe_npz`` picks the file and the stored scale / shift (for "moe"
the pair with the smallest |mean error|, ties to the first in ``zoe_k_dict``'s order),
``zoe_align`` restates upstream's three lines.  Under NumPy 2 the stored 0-d float64 scale and
shift promote, so the aligned depth and the spatial sources' cloud are float64 (NumPy 1.x
would stay in float32; the fixture and the HIP op pin NumPy 2's result).  With a GPU ``device``
a group of views whose files have the target size and the released dtypes goes through
``ops.nvidia_zoe_depth`` instead: the spatial group gets depth and ``depth_range`` from one
fused pass, the temporal and tracker groups the conversion alone, all bit-identical to the numpy
path; any other file takes the numpy path for that group.

The pure-geometry variant builds the static cloud once per scene with the HIP aggregator
(``aggregate_static_pcl``) instead of upstream's numpy loop.

The per-item ``depth_range`` (:446-456) is computed in numpy with ``device=None``; with a GPU ``device`` by the HIP op
``ops.nvidia_depth_range``, bit-identical (DESIGN.md, row 8f-3 NVIDIA), and then no host point cloud is formed.  The
point clouds upstream computes for the temporal and tracker views and then discards are skipped on both paths.

``resident=True`` (with ``resident_scenes``, ``resident_max_bytes``): every source frame is decoded
once and kept in a ``datasets.resident.SceneStore`` on ``device`` (None: host memory), and the items' source views are built
from it, on a GPU by ``ops.item_views`` in one launch; the same keys, shapes, dtypes and bits, every tensor on the store's
device.  The target image and the evaluation mask, one item's each, stay disk reads.  DESIGN.md 7f.  With ZoeDepth inputs
the store keeps each frame's prediction (float32) and the selected pair's float64 scale and shift, read once per frame, and
the alignment is restated per item: by ``ops.item_zoe_depth`` on a GPU store (one launch for all groups' depths and the
range over the float64 depths of the spatial group; NumPy 2's result, as ``ops.nvidia_zoe_depth``), by ``zoe_align`` and
``spatial_depth_range`` on a host store (the installed NumPy's, as the disk path).  There an unknown key or a missing path
raises ``ValueError``, and so does, when its slot is filled, a file in other dtypes than the released ones.

``device_resize=True`` (what each ``device_*`` keyword builds on: datasets/resident.py): a source frame's image goes to the store as decoded and is
BOX-resized on the device into its slot (``ops.resample_u8``, Pillow's resampler bit for bit); the target image is decoded
once, its shape is the file's (height 288) or the monocular video's, and its bytes are resized and expanded on the device, so
``rgb_tgt`` is a device tensor; the pure-geometry loader's LANCZOS stack is one batched call.  Masks and depths keep the host
NEAREST resize, and an image the device path does not serve takes the host statements.  DESIGN.md 7g.
"""
import io
import os
import pathlib
import zipfile
from collections import defaultdict

import numpy as np
import PIL.Image
import torch
from torch.utils.data import Dataset

from ._common import (F32, TGT_HEIGHT, device_input, flat_cam, flow_entries, group_entries, mono_size, read_flow_npz,  # noqa: F401
                      read_flow_pair_or_zeros, refuse_gpu_in_worker, stack_views, tracker_entries)
from ._common import device_depth as check_device_depth, ray_rows as _ray_rows, resize as _resize, resize_nearest_f64 as _resize_nearest_f64
from .resident import DEFAULT_MAX_BYTES, SceneStore, build_item
from .static_aggregation import hwf_to_K

ALL_SCENE_IDS_NVIDIA_DYN = ["Balloon1", "Balloon2", "Jumping", "Playground", "Skating", "Truck", "Umbrella", "dynamicFace"]
N_CAMS = 12
ZOE_TYPES = ("n", "k", "nk")  # ZoeDepth checkpoints: NYU, KITTI, both
ZOE_PRINCIPLES = ("me_med_share", "me_med_indiv", "me_trim_share", "me_trim_indiv")


def make_zoe_k_dict():
    """``use_zoe_depth`` key -> (model type, alignment principle), in upstream's order (:116-125)"""
    return {f"{t}_{k}": (t, k) for t in ZOE_TYPES for k in ZOE_PRINCIPLES}


def zoe_scale_shift_keys(principle):
    """ZOE_DEPTH_PRINCIPLE_DICT (:39-50): ``m[a]e_<fit>_<scope>`` -> the .npz's disparity-domain scale and shift names"""
    err, fit, scope = principle.split("_")
    assert err in ("me", "mae") and fit in ("med", "trim") and scope in ("share", "indiv"), principle
    return f"disp_{scope}_scale_{fit}", f"disp_{scope}_shift_{fit}"


# ---------------------------------------------------------------------------- file formats
def read_llff_cams(poses_bounds_path):
    """``poses_bounds_cvd.npy`` [F,17] -> (hwf [F,3] float32, c2w [F,4,4] float64, OpenCV axes)
    (:608-645).  Stored columns are [down, right, back | t | hwf]; LLFF's fix-up gives
    [right, up, back], the final sign flip [right, down, forward]."""
    arr = np.load(poses_bounds_path, allow_pickle=True)
    n = arr.shape[0]
    m = arr[:, :15].reshape(n, 3, 5)
    rot_t = np.concatenate([m[:, :, 1:2], -m[:, :, 0:1], m[:, :, 2:4]], axis=2).astype(np.float32)  # [F,3,4]
    hwf = m[:, :, 4].astype(np.float32)
    c2w = np.zeros((n, 4, 4), np.float64)
    c2w[:, :3, :] = rot_t
    c2w[:, 3, 3] = 1.0
    c2w[..., 1:3] *= -1.0
    return hwf, c2w


def select_temporal_frames(tgt_frame_id, tgt_cam_id, n_frames, n_track_one_side):
    """Temporally closest source frames and the tracker windows on either side (:250-318).
    Returns dict(temporal=[a,b], n_actual_temporal, fwd2tgt=[...], n_actual_fwd2tgt,
    bwd2tgt=[...], n_actual_bwd2tgt); the lists are padded with the nearest frame id."""
    in_mono = tgt_frame_id % N_CAMS == tgt_cam_id
    if in_mono:  # the target itself is a frame of the input video: its neighbours
        temporal = [f for f in (tgt_frame_id - 1, tgt_frame_id + 1) if 0 <= f < n_frames]
    else:  # another camera at the same instant: the input frame of that instant
        temporal = [tgt_frame_id]
    n_actual = len(temporal)
    if n_actual == 1:
        temporal = temporal * 2  # placeholder duplicate (:277-279)
    fwd = [temporal[0]] * n_track_one_side
    older = list(range(max(0, temporal[0] - n_track_one_side), temporal[0])) if tgt_frame_id > 0 else []
    fwd[: len(older)] = older
    bwd = [temporal[1]] * n_track_one_side
    newer = list(range(temporal[1] + 1, min(n_frames, temporal[1] + 1 + n_track_one_side))) if tgt_frame_id < n_frames - 1 else []
    bwd[: len(newer)] = newer
    return {"in_mono": in_mono, "temporal": temporal, "n_actual_temporal": n_actual, "fwd2tgt": fwd,
            "n_actual_fwd2tgt": len(older), "bwd2tgt": bwd, "n_actual_bwd2tgt": len(newer)}


def select_spatial_frames(tgt_frame_id, tgt_cam_id, n_frames, c2w_all, n_views):
    """The ``n_views`` input frames whose camera centres are nearest to the target camera, from
    the +-12-frame window around the target instant, returned in ascending frame order
    (:320-358)."""
    in_mono = tgt_frame_id % N_CAMS == tgt_cam_id
    lo, hi = max(0, tgt_frame_id - N_CAMS), min(n_frames, tgt_frame_id + N_CAMS)
    pool = [f for f in range(lo, hi) if not (in_mono and f == tgt_frame_id)]
    d = np.linalg.norm(c2w_all[tgt_cam_id, :3, 3][None, :] - c2w_all[pool, :3, 3], axis=1)
    order = np.argsort(d)
    return sorted(pool[i] for i in order[:n_views])


def ray_constants(K, c2w):
    """float32 (M = c2w[:3,:3] @ inv(K[:3,:3]), o = c2w[:3,3]) of one view, as compute_pcl forms them"""
    K32, c32 = np.asarray(K, np.float32), np.asarray(c2w, np.float32)
    return c32[:3, :3] @ np.linalg.inv(K32[:3, :3]).astype(np.float32), c32[:3, 3]


def compute_pcl(h, w, K, c2w, depth, f64_depth=False):
    """_compute_pcl (:840-847): fp32 rays through integer pixel centres times z-depth.  ``f64_depth`` (the ZoeDepth
    branch under NumPy 2): the float32 rays times a float64 depth promote, so the points are float64, multiply and add
    rounded separately."""
    M, o = ray_constants(K, c2w)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    pix = np.stack([u.reshape(-1), v.reshape(-1), np.ones(h * w, np.float32)], 0)
    rays_d = (M @ pix).T
    if f64_depth:
        return o[None, :].astype(np.float64) + rays_d.astype(np.float64) * np.asarray(depth, np.float64).reshape(-1, 1)
    return o[None, :] + rays_d * np.asarray(depth, np.float32).reshape(-1, 1)


def depth_range_from_points(pcl_world, c2w_tgt):
    """near = 0.8 * min z, far = 1.2 * 90th-percentile z of the spatial sources' points in the
    target camera (:446-456)."""
    homo = np.pad(pcl_world, ((0, 0), (0, 1)), "constant", constant_values=1)
    z = (np.linalg.inv(c2w_tgt) @ homo.T).T[:, 2]
    return np.array([max(1e-16, 0.8 * np.min(z)), max(2e-16, 1.2 * np.quantile(z, 0.9))])


def ray_rows(Ks, c2ws):
    """[V,12] float32: every view's ray_constants, M row-major then o, as the depth-range ops take them"""
    return _ray_rows(ray_constants(K, c2w) for K, c2w in zip(Ks, c2ws))


def spatial_depth_range(views, c2w_tgt, device=None, owner="NvidiaDynEvaluationDataset", f64_depth=False):
    """float32 depth_range[2] of the stacked spatial ``views`` (depth[V,H,W], K[V,4,4], c2w[V,4,4]) seen from ``c2w_tgt``:
    depth_range_from_points over every view's compute_pcl with ``device=None``, else ``ops.nvidia_depth_range`` on that
    device (bit-identical; no host points).  ``f64_depth``: the ZoeDepth branch's float64 depths, always in numpy (its
    device path is the fused ``ops.nvidia_zoe_depth``, which starts from the predictions)."""
    depths, Ks, c2ws = views["depth"], views["K"], views["c2w"]
    h, w = depths.shape[1:3]
    if device is None or f64_depth:
        pcl = np.concatenate([compute_pcl(h, w, K, c2w, d, f64_depth) for K, c2w, d in zip(Ks, c2ws, depths)], axis=0)
        return torch.from_numpy(np.ascontiguousarray(depth_range_from_points(pcl, c2w_tgt), dtype=np.float32))
    refuse_gpu_in_worker(owner)
    from .. import ops

    return ops.nvidia_depth_range(F32(depths).to(device), F32(ray_rows(Ks, c2ws)).to(device), np.linalg.inv(c2w_tgt)).cpu()


# ---------------------------------------------------------------------------- ZoeDepth files
def _load_zoe_npz(zoe_path, zip_obj, scene_id, zoe_type, frame_id):
    """the frame's NpzFile of one model type: a file of the directory tree, or a member of the zip (:878-939)"""
    rel = f"{scene_id}/dense/zoe_depths_{zoe_type}/{frame_id:05d}.npz"
    if zip_obj is None:
        return np.load(pathlib.Path(zoe_path) / rel)
    return np.load(io.BytesIO(zip_obj.read(f"{pathlib.Path(zoe_path).stem}/{rel}")), allow_pickle=True)


def select_zoe_pair(zoe_path, zip_obj, scene_id, frame_id, use_zoe_depth, zoe_k_dict=None):
    """(model type, principle) of a frame: the key's entry of ``zoe_k_dict``, or for "moe" the pair whose stored mean error
    is smallest in magnitude, the first in the dict's order among equals (upstream's stable sort, :874-911)"""
    zoe_k_dict = make_zoe_k_dict() if zoe_k_dict is None else zoe_k_dict
    if use_zoe_depth != "moe":
        return zoe_k_dict[use_zoe_depth]
    files = {t: _load_zoe_npz(zoe_path, zip_obj, scene_id, t, frame_id) for t in {t for t, _ in zoe_k_dict.values()}}
    errs = [(t, k, float(files[t][k])) for t, k in zoe_k_dict.values()]
    return sorted(errs, key=lambda e: abs(e[2]))[0][:2]


def read_zoe_npz(zoe_path, zip_obj, scene_id, frame_id, use_zoe_depth, zoe_k_dict=None, pair=None):
    """(depth_pred [H,W], scale, shift) of a frame as stored (the released files: float32, and 0-d float64 arrays) from
    ``zoe_path`` (a directory, or the zip behind the open ``zip_obj``), for the pair ``select_zoe_pair`` picks"""
    zoe_type, principle = pair or select_zoe_pair(zoe_path, zip_obj, scene_id, frame_id, use_zoe_depth, zoe_k_dict)
    info = _load_zoe_npz(zoe_path, zip_obj, scene_id, zoe_type, frame_id)
    k_scale, k_shift = zoe_scale_shift_keys(principle)
    return info["depth_pred"], info[k_scale], info[k_shift]


def zoe_align(depth_pred, scale, shift):
    """upstream's three lines (:941-943) in the types they meet: float32 disparity; under NumPy 2 the 0-d float64 scale
    and shift promote ``disp`` and the depth to float64"""
    raw_disp = 1.0 / (depth_pred + 1e-16)
    disp = scale * raw_disp + shift
    return 1 / (disp + 1e-16)


# ---------------------------------------------------------------------------- dataset
class NvidiaDynEvaluationDataset(Dataset):
    dataset_name = "NVIDIA_Dyn Eval"
    dataset_fname = "nvidia_eval"

    def __init__(self, *, data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir, max_hw, mode,
                 rgb_range="0_1", use_aug=False, scene_ids=None, n_src_views_spatial=10,
                 n_src_views_temporal_track_one_side=5, use_zoe_depth="none", zoe_depth_data_path=None,
                 flow_consist_thres=1.0, device=None, resident=False, resident_scenes=1, resident_max_bytes=DEFAULT_MAX_BYTES,
                 device_resize=False, device_decode=False, device_entropy=False, device_png=False, device_mask=False, device_depth=False):
        options = device_input(type(self).__name__, resident=resident, device=device, device_resize=device_resize, device_decode=device_decode,
                               device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        device_depth = check_device_depth(type(self).__name__, options, device_depth)
        assert max_hw == -1, f"We enforce to use raw resolution. However, we receive max_hw of {max_hw}"
        assert not use_aug
        assert mode in ["eval"], mode
        assert rgb_range == "0_1", rgb_range
        self.zoe_k_dict = make_zoe_k_dict()
        if resident and use_zoe_depth not in ["none", "moe"] + list(self.zoe_k_dict):  # (the store's checks raise ValueError)
            raise ValueError(f"resident=True: use_zoe_depth={use_zoe_depth!r} is none of 'none', 'moe', {', '.join(self.zoe_k_dict)}")
        assert use_zoe_depth in ["none", "moe"] + list(self.zoe_k_dict), f"{use_zoe_depth}, {self.zoe_k_dict.keys()}"
        self.use_zoe_depth = use_zoe_depth
        if use_zoe_depth != "none":  # a directory or a .zip; whichever of the two forms exists (:131-147)
            zp = pathlib.Path(data_root) / zoe_depth_data_path
            if not zp.exists():
                zp = zp.parent / zp.stem if zp.suffix in [".zip"] else zp.parent / f"{zp.name}.zip"
            if resident and not zp.exists():
                raise ValueError(f"resident=True, use_zoe_depth={use_zoe_depth!r}: zoe_depth_data_path={zoe_depth_data_path!r} exists "
                                 f"neither as a directory nor as a .zip under {data_root}")
            assert zp.exists(), zp
            self.zoe_depth_data_path = zp
        self.mode, self.max_hw, self.use_aug, self.rgb_range = mode, max_hw, use_aug, rgb_range
        self.n_src_views_spatial = n_src_views_spatial
        self.n_src_views_temporal_track_one_side = n_src_views_temporal_track_one_side
        self.flow_consist_thres = flow_consist_thres
        self.depth_device = None if device is None else torch.device(device)
        self._init_resident(resident, resident_scenes, resident_max_bytes, self.depth_device, options, device_depth)
        self._set_dirs(data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir)
        scene_ids = ALL_SCENE_IDS_NVIDIA_DYN if scene_ids is None else scene_ids
        exts = {ex for ex, f in PIL.Image.registered_extensions().items() if f in PIL.Image.OPEN}
        # e.g. Balloon1/dense/mv_images/00000/cam01.jpg
        self.scene_img_dict = defaultdict(lambda: defaultdict(dict))
        entries = set()
        for f in self.raw_data_dir.glob("*/dense/mv_images/*/*"):
            if f.suffix not in exts:
                continue
            scene = f.parents[3].name
            if scene not in scene_ids:
                continue
            frame_id, cam_id = int(f.parent.name), int(f.stem.split("cam")[1]) - 1  # cameras are 1-based on disk
            self.scene_img_dict[scene][frame_id][cam_id] = str(f)
            entries.add((scene, str(self.raw_data_dir / scene / "dense"), frame_id, cam_id, str(f)))
        self.scene_img_dict = {k: dict(v) for k, v in self.scene_img_dict.items()}
        self.valid_fs = sorted(entries)  # same order on every worker / rank
        self._cam_cache = {}

    def _set_dirs(self, data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir):
        root = pathlib.Path(data_root)
        self.raw_data_dir, self.depth_data_dir = root / raw_data_dir, root / depth_data_dir
        self.mask_data_dir, self.flow_data_dir = root / mask_data_dir, root / flow_data_dir
        for d in (self.raw_data_dir, self.depth_data_dir, self.mask_data_dir, self.flow_data_dir):
            assert d.exists(), d

    def __len__(self):
        return len(self.valid_fs)

    # ------------------------------------------------------------------ resident source frames (datasets/resident.py)
    store = None  # the SceneStore of ``resident=True``

    def _init_resident(self, resident, resident_scenes, resident_max_bytes, device, options, device_depth=False):
        if resident:
            self.store = SceneStore(device, resident_scenes, resident_max_bytes, self.flow_consist_thres, device_input=options, device_depth=device_depth)

    def _decode_frame(self, scene_id, frame_id, tgt_shape):
        """(image uint8, dynamic mask, depth) of an input frame at the target's size, as _source_view reads them; with
        ``device_resize`` the image as decoded: the store resizes it (``device_decode``: decoded on the device, where the file is
        a JPEG that path serves, straight into the frame's slot when it has the slot's size); with ``device_mask`` the mask as the
        store decodes it, in its slot where the device path serves the file; with ``device_depth`` the depth as the fill placed it in
        its slot, where ``npy_file`` serves the file"""
        h, w = tgt_shape
        zoe = ()
        staged = self.store.staged_depth(self.store.scenes.get(scene_id), frame_id)  # (device_depth, inside a fill; else None)
        if self.use_zoe_depth != "none":  # the prediction and its (scale, shift): the store aligns them per item
            depth, *zoe = self._decode_zoe(scene_id, frame_id, staged)
        elif staged is not None and staged.depth is not None:
            depth = staged.depth
        else:
            depth = self._read_depth(scene_id, frame_id)
        if not isinstance(depth, torch.Tensor):  # (a placed depth went through Pillow's NEAREST picks on the device)
            depth = _resize(depth, h, w, PIL.Image.Resampling.NEAREST)
        img_f = self._src_img_f(scene_id, frame_id)
        rgb = (self.store.decode_image(img_f, into=(self.store.scenes.get(scene_id), frame_id)) if self.store.device_resize else
               self._read_src_rgb(img_f, h, w))
        mask = (self.store.decode_mask(self._mask_f(scene_id, frame_id), (h, w), into=(self.store.scenes.get(scene_id), frame_id))
                if self.store.device_mask else self._read_mask(scene_id, frame_id, h, w))
        return (rgb, mask, depth, *zoe)

    def _decode_zoe(self, scene_id, frame_id, staged=None):
        """(depth_pred float32, (scale, shift) 0-d float64, (model type, principle)) of a frame for its slot of the store:
        the pair is selected once, and a file in other dtypes than the released ones is refused (the store keeps float32
        predictions; the disk path would follow such a file's own promotion).  ``staged`` (``device_depth``): the file's bytes as
        ``_zoe_depth_request`` read them, and the prediction in its slot where the fill placed it: scale and shift come from the
        same bytes, and so does a prediction the device path did not serve"""
        fresh = self.__dict__.setdefault("_zoe_fresh", set())  # (pairs the depth request selected a moment ago: counted here, as before)
        known = (scene_id, frame_id) in self.__dict__.get("_zoe_pairs", {}) and (scene_id, frame_id) not in fresh
        fresh.discard((scene_id, frame_id))
        if staged is not None and staged.data is not None:
            info = np.load(io.BytesIO(staged.data), allow_pickle=True)
            k_scale, k_shift = zoe_scale_shift_keys(self._zoe_pairs[scene_id, frame_id][1])
            pred, scale, shift = (staged.depth if staged.depth is not None else info["depth_pred"]), info[k_scale], info[k_shift]
        else:
            pred, scale, shift = self._read_zoe(scene_id, frame_id)
        pair = self._zoe_pairs[scene_id, frame_id]
        self.store.stats["zoe_files_read"] += 1 + (len(ZOE_TYPES) if self.use_zoe_depth == "moe" and not known else 0)
        if (not isinstance(pred, torch.Tensor) and pred.dtype != np.float32) or scale.dtype != np.float64 or shift.dtype != np.float64:
            rel = f"{scene_id}/dense/zoe_depths_{pair[0]}/{frame_id:05d}.npz"
            k_scale, k_shift = zoe_scale_shift_keys(pair[1])
            raise ValueError(f"{self.zoe_depth_data_path} : {rel}: depth_pred is {pred.dtype}, {k_scale} {scale.dtype}, {k_shift} "
                             f"{shift.dtype}; resident=True keeps float32 predictions with float64 scales and shifts (use_zoe_depth="
                             f"{self.use_zoe_depth!r} without resident=True follows the file's own types)")
        return pred, (scale, shift), pair

    def _resident_item(self, scene_id, tgt_shape, all_c2w, all_hwf, **kw):
        """``resident.build_item`` over this loader's readers and cameras"""
        def cams(ids):
            Kc = [self._view_cam(all_c2w[f], all_hwf[f], tgt_shape) for f in ids]
            return (np.stack([flat_cam(*tgt_shape, K, c) for K, c in Kc]), np.stack([K for K, _ in Kc]), np.stack([c for _, c in Kc]))

        zoe = self.use_zoe_depth != "none"
        scene = self.store.scene(scene_id, all_c2w.shape[0], tgt_shape, prediction=zoe)
        if zoe:  # depths and range come from the predictions; the cameras keep _aug_c2w's double inversion
            kw["depths"] = lambda ids, range_cams, rays: self.store.zoe_depths(scene, ids, range_cams, rays, kw["c2w_tgt"])
        return build_item(self.store, scene, lambda f: self._decode_frame(scene_id, f, tgt_shape), cams=cams,
                          image_path=lambda f: self._src_img_f(scene_id, f), mask_path=lambda f: self._mask_f(scene_id, f),
                          depth_request=lambda f: self._depth_request(scene_id, f),
                          flow_path=lambda a, b: self._flow_path(scene_id, a, b), owner=type(self).__name__, **kw)

    def _depth_request(self, scene_id, frame_id):
        """``device_depth``: the frame's depth file and this loader's statement over it, as ``SceneStore._stage_depths`` takes them:
        the DynIBaR disparity ``disp/%05d.npy`` with ``1 / (disp + 1e-8)``, or the ZoeDepth file's bytes with ``depth_pred`` as it is"""
        if self.use_zoe_depth != "none":
            return self._zoe_depth_request(scene_id, frame_id)
        return self.depth_data_dir / scene_id / "disp" / f"{frame_id:05d}.npy", None, "reciprocal", 1.0

    def _zoe_depth_request(self, scene_id, frame_id):
        """the bytes of the frame's ``.npz`` of the selected model type -- from the directory, or the zip's member -- read once: the
        store places ``depth_pred`` from them, ``_decode_zoe`` takes scale and shift from them"""
        zobj, cache = self._zoe_zip_obj(), self.__dict__.setdefault("_zoe_pairs", {})
        if (scene_id, frame_id) not in cache:
            cache[scene_id, frame_id] = select_zoe_pair(self.zoe_depth_data_path, zobj, scene_id, frame_id, self.use_zoe_depth, self.zoe_k_dict)
            self.__dict__.setdefault("_zoe_fresh", set()).add((scene_id, frame_id))
        rel = f"{scene_id}/dense/zoe_depths_{cache[scene_id, frame_id][0]}/{frame_id:05d}.npz"
        if zobj is None:
            data = (pathlib.Path(self.zoe_depth_data_path) / rel).read_bytes()
        else:
            data = zobj.read(f"{pathlib.Path(self.zoe_depth_data_path).stem}/{rel}")
        return data, "depth_pred", "copy", 1.0

    # ------------------------------------------------------------------ ZoeDepth
    use_zoe_depth, zoe_depth_data_path = "none", None  # (subclasses that build themselves never read ZoeDepth)
    _zoe_zip = None  # (pid, ZipFile): opened on the first item of every process, never pickled

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_zoe_zip", None)
        return state

    def _zoe_zip_obj(self):
        if not self.zoe_depth_data_path.is_file():
            return None
        if self._zoe_zip is None or self._zoe_zip[0] != os.getpid():
            self._zoe_zip = (os.getpid(), zipfile.ZipFile(self.zoe_depth_data_path))
        return self._zoe_zip[1]

    def _read_zoe(self, scene_id, frame_id):
        """read_zoe_npz of a frame; the "moe" choice is a property of the files, so it is kept per (scene, frame)"""
        zobj, cache = self._zoe_zip_obj(), self.__dict__.setdefault("_zoe_pairs", {})
        if (scene_id, frame_id) not in cache:
            cache[scene_id, frame_id] = select_zoe_pair(self.zoe_depth_data_path, zobj, scene_id, frame_id, self.use_zoe_depth,
                                                        self.zoe_k_dict)
        return read_zoe_npz(self.zoe_depth_data_path, zobj, scene_id, frame_id, self.use_zoe_depth, self.zoe_k_dict,
                            pair=cache[scene_id, frame_id])

    def _zoe_group_on_device(self, scene_id, frame_ids, tgt_shape):
        """(depth_pred [V,H,W] float32, scale_shift [V,2] float64) when ``ops.nvidia_zoe_depth`` serves the group: a GPU
        ``device`` and files of the target size in the released dtypes; else None (the numpy path)"""
        if self.use_zoe_depth == "none" or self.depth_device is None:
            return None
        refuse_gpu_in_worker(type(self).__name__)
        read = [self._read_zoe(scene_id, f) for f in frame_ids]
        if any(p.shape != tuple(tgt_shape) or p.dtype != np.float32 or a.dtype != np.float64 or b.dtype != np.float64
               for p, a, b in read):
            return None
        return np.stack([p for p, _, _ in read]), np.array([[float(a), float(b)] for _, a, b in read], np.float64)

    # ------------------------------------------------------------------ readers
    def _read_cam(self, scene_id):
        if scene_id not in self._cam_cache:
            hwf, c2w = read_llff_cams(self.raw_data_dir / scene_id / "dense" / "poses_bounds_cvd.npy")
            assert len(self.scene_img_dict[scene_id]) == hwf.shape[0], (len(self.scene_img_dict[scene_id]), hwf.shape[0])
            self._cam_cache[scene_id] = (hwf, c2w)
        hwf, c2w = self._cam_cache[scene_id]
        return hwf.copy(), c2w.copy()

    def _mask_f(self, scene_id, frame_id):
        return self.mask_data_dir / scene_id / "dense" / "masks" / "final" / f"{frame_id:05d}_final.png"

    def _read_mask(self, scene_id, frame_id, tgt_h, tgt_w):
        m = np.array(PIL.Image.open(self._mask_f(scene_id, frame_id)))
        return _resize(m, tgt_h, tgt_w, PIL.Image.Resampling.NEAREST)  # True = dynamic

    def _read_depth(self, scene_id, frame_id):
        if self.use_zoe_depth != "none":
            return zoe_align(*self._read_zoe(scene_id, frame_id))
        return 1 / (np.load(self.depth_data_dir / scene_id / "disp" / f"{frame_id:05d}.npy") + 1e-8)

    def _read_flow(self, scene_id, src_frame_id, tgt_frame_id, tgt_shape):
        return read_flow_pair_or_zeros(self._flow_path(scene_id, src_frame_id, tgt_frame_id), tgt_shape, self.flow_consist_thres)

    def _flow_path(self, scene_id, src_frame_id, tgt_frame_id):
        """the pair's flow file; None for the placeholder pair (a frame with itself)"""
        k = abs(tgt_frame_id - src_frame_id)
        if k == 0:
            return None
        return self.flow_data_dir / scene_id / "dense" / "flows" / f"interval_{k}" / f"{src_frame_id:05d}_{tgt_frame_id:05d}.npz"

    def _read_eval_mask(self, scene_id, frame_id, cam_id, h, w):
        """float32 [h,w,3]; with ``device_mask`` a tensor on the store's device where it serves the file (a grey or 8-bit RGB PNG
        of the target's size), else this host statement's array"""
        f = self.raw_data_dir / scene_id / "dense" / "mv_masks" / f"{frame_id:05d}" / f"cam{cam_id + 1:02d}.png"
        if self.store is not None and self.store.device_mask:
            m = self.store.decode_eval_mask(f, (h, w))
            if m is not None:
                return m
        m = np.float32(np.array(PIL.Image.open(f).convert("RGB"))[..., ::-1] > 1e-3)  # channel order as cv2.imread
        return _resize(m, h, w, PIL.Image.Resampling.NEAREST)

    def _target_rgb(self, scene_dir, img_f):
        """the target image; multi-view frames stored at another height are brought to the mono
        video's size with LANCZOS as upstream (:367-380)"""
        raw = np.array(PIL.Image.open(img_f))
        if raw.shape[0] != TGT_HEIGHT:
            new_h, new_w = mono_size(scene_dir)
            raw = np.array(PIL.Image.fromarray(raw).resize((new_w, new_h), resample=PIL.Image.Resampling.LANCZOS))
        assert raw.shape[0] == TGT_HEIGHT, raw.shape
        return raw

    # ------------------------------------------------------------------ one source view
    def _aug_c2w(self, c2w):
        """the camera-to-world of _compute_cam_info (:947-955); upstream's augment_cam("none") inverts twice, which the
        disparity path's fixture does not see and that path leaves out.  The ZoeDepth fixture is compared bit for bit, so
        that branch inverts twice like upstream (and like nvidia_vis)."""
        if self.use_zoe_depth != "none":
            return np.linalg.inv(np.linalg.inv(c2w))
        return c2w

    def _src_img_f(self, scene_id, frame_id):
        """Frame i of the monocular video is camera i % 12 of time step i (:647-653)."""
        return self.scene_img_dict[scene_id][frame_id][frame_id % N_CAMS]

    @staticmethod
    def _read_src_rgb(img_f, h, w):
        return _resize(np.array(PIL.Image.open(img_f)), h, w, PIL.Image.Resampling.BOX)

    def _view_cam(self, c2w, hwf, tgt_shape):
        """(K [4,4], c2w [4,4]) of a view at the target's size"""
        K = np.eye(4)
        K[:3, :3] = hwf_to_K(*hwf, tgt_shape=tgt_shape)
        return K, self._aug_c2w(np.asarray(c2w))

    def _source_view(self, scene_id, frame_id, c2w, hwf, tgt_shape, with_geometry=True, img_f=None, depth=None):
        """image, flat camera and (optionally) dynamic mask / depth / camera matrices of an input
        frame (:728-838); spatial_depth_range makes the world points from depth, K and c2w.
        ``depth``: taken as the view's depth in place of the file's (the ZoeDepth device path)."""
        h, w = tgt_shape
        if img_f is None:
            img_f = self._src_img_f(scene_id, frame_id)
        rgb = self._read_src_rgb(img_f, h, w).astype(np.float32) / 255.0
        K, c2w = self._view_cam(c2w, hwf, tgt_shape)
        out = {"rgb": rgb, "flat_cam": flat_cam(h, w, K, c2w)}
        if with_geometry:
            mask = self._read_mask(scene_id, frame_id, h, w).astype(np.float32)
            if depth is None:
                depth = self._read_depth(scene_id, frame_id)
                depth = (_resize_nearest_f64(depth, h, w) if depth.dtype == np.float64 and self.use_zoe_depth != "none" else
                         _resize(depth, h, w, PIL.Image.Resampling.NEAREST))
            out.update(dyn_mask=mask, depth=depth, dyn_rgb=rgb * mask[..., None], static_rgb=rgb * (1 - mask[..., None]),
                       K=K, c2w=c2w)
        return out

    def _stack_views(self, scene_id, frame_ids, all_c2w, all_hwf, tgt_shape, range_c2w_tgt=None):
        """the stacked views of ``frame_ids``.  ZoeDepth on a GPU ``device``: their depths come from one
        ``ops.nvidia_zoe_depth`` call, with ``range_c2w_tgt`` fused with the group's ``depth_range`` (an extra key)."""
        zoe = self._zoe_group_on_device(scene_id, frame_ids, tgt_shape)
        preds = [None] * len(frame_ids) if zoe is None else zoe[0]
        views = [self._source_view(scene_id, f, all_c2w[f], all_hwf[f], tgt_shape, depth=p) for f, p in zip(frame_ids, preds)]
        out = stack_views(views)
        if zoe is not None:
            from .. import ops

            dev = self.depth_device
            pred = torch.from_numpy(zoe[0]).to(dev)
            if range_c2w_tgt is None:
                out["depth"] = ops.nvidia_zoe_depth(pred, zoe[1]).cpu().numpy()
            else:
                rays = F32(ray_rows(out["K"], out["c2w"])).to(dev)
                depth, rng = ops.nvidia_zoe_depth(pred, zoe[1], rays, np.linalg.inv(range_c2w_tgt))
                out["depth"], out["depth_range"] = depth.cpu().numpy(), rng.cpu()
        return out

    # ------------------------------------------------------------------ item
    def _item_head(self, index):
        """the target's entries and the item's selection: everything in front of the source views"""
        scene_id, scene_dir, tgt_frame_id, tgt_cam_id, img_f = self.valid_fs[index]
        all_hwf, all_c2w = self._read_cam(scene_id)
        n_frames = all_hwf.shape[0]
        sel = select_temporal_frames(tgt_frame_id, tgt_cam_id, n_frames, getattr(self, "n_src_views_temporal_track_one_side", 0))
        on_device = self.store is not None and self.store.device_resize
        if on_device:  # decoded once: the LANCZOS pass of _target_rgb gave the shape alone, and the shape is known without it
            raw_rgb = self.store.decode_image(img_f, target=True)  # (device_decode: a tensor on the device)
            raw_h, raw_w = tuple(raw_rgb.shape[:2]) if raw_rgb.shape[0] == TGT_HEIGHT else mono_size(scene_dir)
            assert raw_h == TGT_HEIGHT, (raw_h, raw_w)
        else:
            raw_rgb = self._target_rgb(scene_dir, img_f)
            raw_h, raw_w = raw_rgb.shape[:2]
        all_hwf[:, 0], all_hwf[:, 1] = raw_h, raw_w  # the stored h, w belong to the full-resolution capture (:399-401)
        tgt_shape = (raw_h, raw_w)
        # NOTE upstream indexes the poses with the CAMERA id: the 12 camera poses repeat (:319-323)
        if on_device:
            tgt = {"flat_cam": flat_cam(raw_h, raw_w, *self._view_cam(all_c2w[tgt_cam_id], all_hwf[tgt_cam_id], tgt_shape))}
            if self.store.serves_target(raw_rgb, tgt_shape):  # the bytes travel with the item's small entries, or are there already
                rgb_tgt = ("__rgb_tgt", raw_rgb if isinstance(raw_rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(raw_rgb)))
            else:  # _source_view's statements on the decoded image
                if isinstance(raw_rgb, torch.Tensor):  # (a size the device resize refuses: back to the host, which waits)
                    raw_rgb = raw_rgb.cpu().numpy()
                rgb_tgt = ("rgb_tgt", F32(_resize(raw_rgb, raw_h, raw_w, PIL.Image.Resampling.BOX).astype(np.float32) / 255.0))
        else:
            tgt = self._source_view(scene_id, tgt_frame_id, all_c2w[tgt_cam_id], all_hwf[tgt_cam_id], tgt_shape,
                                    with_geometry=False, img_f=img_f)
            rgb_tgt = ("rgb_tgt", F32(tgt["rgb"]))
        eval_mask = self._read_eval_mask(scene_id, tgt_frame_id, tgt_cam_id, raw_h, raw_w)
        item = {
            "scene_id": scene_id,
            rgb_tgt[0]: rgb_tgt[1],
            "eval_mask": eval_mask if isinstance(eval_mask, torch.Tensor) else F32(eval_mask),  # (device_mask: on the device already)
            "flat_cam_tgt": F32(tgt["flat_cam"]),
            "time_tgt": torch.FloatTensor([tgt_frame_id]),
            "misc": {"scene_id": scene_id, "tgt_frame_id": tgt_frame_id, "tgt_cam_id": tgt_cam_id},
        }
        ctx = dict(scene_id=scene_id, tgt_frame_id=tgt_frame_id, tgt_cam_id=tgt_cam_id, all_hwf=all_hwf, all_c2w=all_c2w,
                   n_frames=n_frames, sel=sel, tgt_shape=tgt_shape)
        return item, ctx

    def _common_item(self, index):
        item, c = self._item_head(index)
        sel, scene_id, tgt_shape = c["sel"], c["scene_id"], c["tgt_shape"]
        temporal = self._stack_views(scene_id, sel["temporal"], c["all_c2w"], c["all_hwf"], tgt_shape)
        item.update(group_entries("temporal", temporal, sel["temporal"], sel["n_actual_temporal"]))
        item.update(flow_entries(self._read_flow(scene_id, sel["temporal"][0], sel["temporal"][1], tgt_shape),
                                 self._read_flow(scene_id, sel["temporal"][1], sel["temporal"][0], tgt_shape)))
        return item, c

    def _resident_eval_item(self, index, with_spatial):
        """the evaluation loaders' item from the store; the target image and the evaluation mask, one item's each, stay disk
        reads and travel with the small entries"""
        head, c = self._item_head(index)
        spatial_ids = None
        seq = [c["tgt_frame_id"], *c["sel"]["temporal"]]
        if with_spatial:
            spatial_ids = select_spatial_frames(c["tgt_frame_id"], c["tgt_cam_id"], c["n_frames"], c["all_c2w"], self.n_src_views_spatial)
            assert self.n_src_views_spatial < N_CAMS * 2
            seq = [c["tgt_frame_id"], *spatial_ids, *c["sel"]["temporal"]]
        host = {k: v for k, v in head.items() if isinstance(v, torch.Tensor)}
        host["seq_ids"] = torch.LongTensor(np.array(seq))
        item = self._resident_item(c["scene_id"], c["tgt_shape"], c["all_c2w"], c["all_hwf"],
                                   fixed={k: v for k, v in head.items() if k not in host}, host=host, sel=c["sel"],
                                   spatial_ids=spatial_ids, spatial_depth=True, c2w_tgt=c["all_c2w"][c["tgt_cam_id"]],
                                   trackers=with_spatial)
        if "__rgb_tgt" in item:  # device_resize: the target's bytes as decoded
            item["rgb_tgt"] = self.store.expand_target(item.pop("__rgb_tgt"), c["tgt_shape"])
        return item

    def __getitem__(self, index):
        if self.store is not None:
            return self._resident_eval_item(index, with_spatial=True)
        item, c = self._common_item(index)
        sel, scene_id = c["sel"], c["scene_id"]
        spatial_ids = select_spatial_frames(c["tgt_frame_id"], c["tgt_cam_id"], c["n_frames"], c["all_c2w"], self.n_src_views_spatial)
        assert self.n_src_views_spatial < N_CAMS * 2
        c2w_tgt = c["all_c2w"][c["tgt_cam_id"]]
        spatial = self._stack_views(scene_id, spatial_ids, c["all_c2w"], c["all_hwf"], c["tgt_shape"], range_c2w_tgt=c2w_tgt)
        depth_range = spatial.get("depth_range")  # the fused ZoeDepth pass has it already
        if depth_range is None:
            depth_range = spatial_depth_range(spatial, c2w_tgt, self.depth_device, type(self).__name__,
                                              f64_depth=self.use_zoe_depth != "none" and spatial["depth"].dtype == np.float64)
        item["seq_ids"] = torch.LongTensor(np.array([c["tgt_frame_id"], *spatial_ids, *sel["temporal"]]))
        item.update(group_entries("spatial", spatial), depth_range=depth_range)
        item.update(tracker_entries(sel, lambda ids: self._stack_views(scene_id, ids, c["all_c2w"], c["all_hwf"], c["tgt_shape"])))
        return item


class NvidiaDynPureGeoEvaluationDataset(NvidiaDynEvaluationDataset):
    """nvidia_eval_pure_geo.py:41-470 -- no spatial sources / tracker windows, plus the static
    cloud ``st_pcl_rgb`` of the whole monocular video, aggregated once per scene on the GPU
    (``device``; upstream: numpy at construction time, :166-178)."""
    dataset_name = "NVIDIA_Dyn Pure Geometry Eval"
    dataset_fname = "nvidia_eval_pure_geo"

    def __init__(self, *, data_root, raw_data_dir, depth_data_dir, mask_data_dir, flow_data_dir, max_hw, mode,
                 rgb_range="0_1", use_aug=False, scene_ids=None, flow_consist_thres=1.0, device="cuda", resident=False,
                 resident_scenes=1, resident_max_bytes=DEFAULT_MAX_BYTES, device_resize=False, device_decode=False, device_entropy=False, device_png=False,
                 device_mask=False, device_depth=False):
        options = device_input(type(self).__name__, resident=resident, device=device, device_resize=device_resize, device_decode=device_decode,
                               device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        device_depth = check_device_depth(type(self).__name__, options, device_depth)
        super().__init__(data_root=data_root, raw_data_dir=raw_data_dir, depth_data_dir=depth_data_dir,
                         mask_data_dir=mask_data_dir, flow_data_dir=flow_data_dir, max_hw=max_hw, mode=mode,
                         rgb_range=rgb_range, use_aug=use_aug, scene_ids=scene_ids, n_src_views_spatial=0,
                         n_src_views_temporal_track_one_side=0, flow_consist_thres=flow_consist_thres)
        self.device = device
        self._init_resident(resident, resident_scenes, resident_max_bytes, device, options, device_depth)  # (where the cloud is built)
        self.st_pcl_dict = {scene: self._aggregate_static_pcl(scene) for scene in sorted(self.scene_img_dict)}

    def _load_mono_video(self, scene_id):
        """frames, depths, dynamic masks and cameras of the monocular video (:183-222)"""
        scene_dir = self.raw_data_dir / scene_id / "dense"
        tgt_h, tgt_w = mono_size(scene_dir)
        all_hwf, all_c2w = self._read_cam(scene_id)
        all_hwf[:, 0], all_hwf[:, 1] = tgt_h, tgt_w
        n = all_hwf.shape[0]
        mono = scene_dir / f"images_{tgt_w}x{tgt_h}"
        if self.store is not None and self.store.device_resize:  # the frames of another size in one batched call
            files = [mono / f"{i:05d}.png" for i in range(n)]
            raws = self.store.decode_stack(files) if self.store.device_png else [np.array(PIL.Image.open(f)) for f in files]
            imgs = self.store.resize_stack(raws, (tgt_h, tgt_w), "lanczos")
            imgs = np.stack(imgs).astype(np.float32) / 255.0
        else:
            imgs = np.stack([_resize(np.array(PIL.Image.open(mono / f"{i:05d}.png")), tgt_h, tgt_w, PIL.Image.Resampling.LANCZOS)
                             for i in range(n)]).astype(np.float32) / 255.0
        depths = np.stack([self._read_depth(scene_id, i) for i in range(n)]).astype(np.float32)
        masks = np.stack([self._read_mask(scene_id, i, tgt_h, tgt_w).astype(bool) for i in range(n)])
        K3s = np.stack([hwf_to_K(*all_hwf[i]) for i in range(n)])
        return imgs, depths, masks, K3s, all_c2w

    def _aggregate_static_pcl(self, scene_id):
        from .static_aggregation import aggregate_static_pcl

        imgs, depths, masks, K3s, c2ws = self._load_mono_video(scene_id)
        dev = self.device
        cloud = aggregate_static_pcl(torch.from_numpy(imgs).to(dev), torch.from_numpy(depths).to(dev),
                                     torch.from_numpy(masks).to(dev), K3s, c2ws)
        return cloud.cpu()

    def __getitem__(self, index):
        if self.store is not None:
            item = self._resident_eval_item(index, with_spatial=False)
            if self.store.device is not None:  # the scene's cloud, moved once: the item's tensors are all on the store's device
                on_dev = self.__dict__.setdefault("_st_pcl_on_device", {})
                if item["scene_id"] not in on_dev:
                    on_dev[item["scene_id"]] = self.st_pcl_dict[item["scene_id"]].to(self.store.device)
                item["st_pcl_rgb"] = on_dev[item["scene_id"]]
            else:
                item["st_pcl_rgb"] = self.st_pcl_dict[item["scene_id"]]
            return item
        item, c = self._common_item(index)
        item["seq_ids"] = torch.LongTensor(np.array([c["tgt_frame_id"], *c["sel"]["temporal"]]))
        item["st_pcl_rgb"] = self.st_pcl_dict[c["scene_id"]]  # [#pt, 6]: xyz, rgb
        return item
