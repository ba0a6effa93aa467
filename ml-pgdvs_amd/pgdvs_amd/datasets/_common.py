"""What the four loader modules (``nvidia_eval`` with its two classes, ``nvidia_vis``, ``mono_vis``, ``dycheck_iphone``) share: file readers, resizes,
the per-view camera row and the item's per-group and flow entries.  Host numpy / PIL input plumbing."""
import collections
import pathlib

import numpy as np
import PIL.Image
import torch

TGT_HEIGHT = 288


def F32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def resize(arr, h, w, resample):
    if arr.shape[0] == h and arr.shape[1] == w:
        return arr
    return np.array(PIL.Image.fromarray(arr).resize((w, h), resample=resample))


def resize_nearest_f64(arr, h, w):
    """resize(..., NEAREST) of a float64 image (PIL has no such mode): the filter picks pixels, so resize their indices"""
    if arr.shape[0] == h and arr.shape[1] == w:
        return arr
    idx = np.arange(arr.shape[0] * arr.shape[1], dtype=np.int32).reshape(arr.shape[:2])
    return arr.reshape(-1)[resize(idx, h, w, PIL.Image.Resampling.NEAREST)]


def mono_size(scene_dir):
    """(h, w) of an NVIDIA scene's ``images_<W>x288`` directory, the monocular video's size"""
    mono = list(pathlib.Path(scene_dir).glob(f"images_*x{TGT_HEIGHT}"))
    assert len(mono) == 1, mono
    w, h = (int(x) for x in mono[0].name.split("images_")[1].split("x"))
    return h, w


def read_flow_npz(path, occ_thres=1.0):
    """``flows/interval_k/<a>_<b>.npz`` {flow[H,W,2], coord_diff[H,W,2]} -> (flow, occlusion
    mask = sum|coord_diff| > thres as float32) (nvidia_eval.py:957-1011)."""
    info = np.load(path)
    flow = info["flow"]
    occ = (np.sum(np.abs(info["coord_diff"]), axis=2) > occ_thres).astype(np.float32)
    return flow, occ


def read_flow_pair_or_zeros(path, tgt_shape, occ_thres):
    """read_flow_npz of ``path`` at the target's size; ``path`` None is the placeholder pair (a frame with itself): zeros"""
    if path is None:
        return np.zeros(list(tgt_shape) + [2], np.float32), np.zeros(tgt_shape, np.float32)
    flow, occ = read_flow_npz(path, occ_thres)
    assert flow.shape[:2] == tuple(tgt_shape), (flow.shape, tgt_shape)
    return flow, occ


def flat_cam(h, w, K4, c2w):
    """[34] float32: h, w, K[4,4], c2w[4,4]"""
    return np.concatenate(([h, w], np.asarray(K4).flatten(), np.asarray(c2w).flatten())).astype(np.float32)


def stack_views(views):
    return {k: np.stack([v[k] for v in views], axis=0) for k in views[0]}


def ray_rows(consts):
    """[V,12]: every view's ray constants (M[3,3], o[3]), M row-major then o, as the depth-range ops take them"""
    return np.stack([np.concatenate([M.reshape(-1), o]) for M, o in consts])


def refuse_gpu_in_worker(owner):
    if torch.utils.data.get_worker_info() is not None:
        raise RuntimeError(f"{owner}(device=...) computes depth_range on the GPU, which forked DataLoader workers must not "
                           "touch: use n_dataloader_workers=0 (or device=None)")


# which parts of the image input run on the device: ``device_input`` checks them, datasets/resident.py describes them
DeviceInput = collections.namedtuple("DeviceInput", "resize decode entropy png mask")


def device_input(owner, *, resident, device, device_resize=False, device_decode=False, device_entropy=False, device_png=False, device_mask=False):
    """The five image-input keywords of ``owner`` (a loader, or the store) as a ``DeviceInput``.  Each option builds on
    another: the first rule broken, in this order, is refused with a ValueError that names what is missing."""
    if device_entropy and not device_decode:
        raise ValueError(f"{owner}(device_entropy=True) decodes the scan of the JPEG frames that device_decode=True reads: it needs device_decode=True")
    if device_png and not device_resize:
        raise ValueError(f"{owner}(device_png=True) decodes PNG frames on the device at the file's size: it needs device_resize=True")
    if device_mask and not device_resize:
        raise ValueError(f"{owner}(device_mask=True) decodes mask PNGs on the device into the resident store: it needs device_resize=True")
    if device_decode and not device_resize:
        raise ValueError(f"{owner}(device_decode=True) decodes JPEG frames on the device at the file's size: it needs device_resize=True")
    if device_resize and not resident:
        raise ValueError(f"{owner}(device_resize=True) resizes decoded frames into the resident store: it needs resident=True")
    if device_resize and (device is None or torch.device(device).type != "cuda"):
        raise ValueError(f"{owner}(device_resize=True) resizes on the device: it needs the store on a GPU, got device={device!r}")
    return DeviceInput(bool(device_resize), bool(device_decode), bool(device_entropy), bool(device_png), bool(device_mask))


def device_depth(owner, options, device_depth=False):
    """The sixth keyword of ``owner``, checked behind the five of ``options`` (the ``DeviceInput`` that ``device_input`` returned,
    which stays the five-field record): ``device_depth`` places the depth files' floats in the resident store on the device
    (datasets/resident.py), so it needs ``device_resize`` -- and with it ``resident=True`` and the store on a GPU."""
    if device_depth and not options.resize:
        raise ValueError(f"{owner}(device_depth=True) places the depth files' payloads in the resident store on the device: it needs device_resize=True")
    return bool(device_depth)


def group_entries(group, views, times=None, n_actual=None, depth=True):
    """The item's entries of one group of stacked source views: "spatial", "temporal" or "temporal_track_{fwd,bwd}2tgt".
    The temporal and tracker groups also carry their frames' ``times`` and ``n_actual``, the count before padding; the
    visualisation loaders' spatial group goes without its ``depth``, as upstream's."""
    out = {f"{k}_src_{group}": F32(views[k]) for k in ("rgb", "dyn_rgb", "static_rgb", "flat_cam")}
    out.update({f"{k}_src_{group}": F32(views[k])[..., None] for k in (("dyn_mask", "depth") if depth else ("dyn_mask",))})
    if times is not None:
        out[f"time_src_{group}"] = torch.FloatTensor(times)
    if n_actual is not None:
        out[f"n_actual_{group}"] = torch.LongTensor([n_actual])
    return out


def tracker_entries(sel, stack):
    """group_entries of both tracker windows of ``sel``; ``stack(frame_ids)`` gives a window's stacked views"""
    out = {}
    for side in ("fwd2tgt", "bwd2tgt"):
        out.update(group_entries(f"temporal_track_{side}", stack(sel[side]), sel[side], sel[f"n_actual_{side}"]))
    return out


def flow_entries(fwd, bwd):
    """The item's four flow keys from the two (flow, occlusion mask) pairs between the temporal frames"""
    return {"flow_fwd": F32(fwd[0]), "flow_fwd_occ_mask": F32(fwd[1])[..., None],
            "flow_bwd": F32(bwd[0]), "flow_bwd_occ_mask": F32(bwd[1])[..., None]}
