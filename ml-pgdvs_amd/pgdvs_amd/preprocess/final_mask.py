"""The final motion mask (pgdvs/preprocess/compute_mask.py:341-471 combine_masks, :184-193 warp_flow, :706-861 the per-frame
loop of ``__main__``): the raw mask of a frame (``flow_epi`` or the semantic classes), the previous frame's result and a
per-pixel "how often dynamic" count warped along the backward flow, an erosion, the growth to whole segments of a
SAM-style segmenter, a dilation; and ``run_masks``, the writer of ``masks/final/<frame>_final.png``, which ``run_zoedepth``
and the loaders read.  The segmenter and the semantic networks are plug-ins, as the flow and depth networks are.

``device=None`` restates upstream's lines with numpy and scipy.ndimage on the host; a device makes one call of
``ops.mask_combine`` (csrc/mask_combine.hip) per frame and leaves everything on the GPU.

Upstream's semantics, kept:
  :420   frame 0 (no previous state): dyn_cnt = raw_no_warp.astype(float32).
  :446   later frames: dyn_cnt = dyn_cnt_warp_prev + final_raw, WITHOUT the consistency mask (upstream's open TODO, :444).
  :213   bwd_mask = (|cd0| + |cd1| <= 1.0), the sum in float32.
  :401   warp_prev = (warp(prev_mask as uint8) * bwd_mask) > 1e-3.
  :407   dyn_track = (warp(prev_cnt) / (img_idx + 1) * bwd_mask) > 0.5, a float32 array against Python scalars: all of it
         float32, the division correctly rounded.
  :414, :427, :449  skimage's erosion reads SET pixels outside the image, its dilation CLEAR ones (``scipy.ndimage`` with
         border_value 1 / 0, as ``mask.binary_opening_disk1``), with disk(2), the 5 x 5 footprint of 13 pixels.
  :418   raw = raw_no_warp | erode(warp_prev & dyn_track);  :427 raw_eroded = erode(raw).
  :437   per segment n_pix and n_overlap with raw_eroded; selected when n_overlap > 0 and n_overlap > sam_overlap_thres *
         n_pix, a float64 product and a strict comparison (5 of 50 is NOT selected: 0.1 * 50 >= 5 in float64).
  :441   final_raw = raw_eroded | every selected segment;  :449 final = dilate(final_raw).  n_seg = 0: final_raw = raw_eroded.
  :827   the next frame's prev_mask_final_raw is erode(final_raw), returned here as ``next_prev``.
  :780   mask_type "flow_depth" raises NotImplementedError; :664 any other unknown type ValueError.

The warp is this project's own statement of ``cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0)`` with a float32 map, after
OpenCV's generic interior path; ``warp_flow_numpy`` and the kernel implement it operation for operation, in float32, every
operation rounded on its own:
  x = flow_x + col in float32 (y alike), clamped to [-8, W + 8] (fmax, then fmin: a NaN becomes -8), which stands in for
  OpenCV's saturation to int16 (beyond it every tap is outside the image either way);
  s = rint(32 x), half to even;  ix = s >> 5;  k = s & 31;
  the weights of k from ``cubic_table()`` (A = -0.75; f = k / 32; g = 1 - f):
    c0 = ((A (f + 1) - 5 A) (f + 1) + 8 A) (f + 1) - 4 A;  c1 = ((A + 2) f - (A + 3)) f f + 1;
    c2 = ((A + 2) g - (A + 3)) g g + 1;  c3 = 1 - c0 - c1 - c2;
  4 x 4 taps at ix - 1 .. ix + 2, iy - 1 .. iy + 2, a tap outside the image 0;  w[j][i] = cy[j] cx[i];  each row
  ((v0 w0 + v1 w1) + v2 w2) + v3 w3, the rows added top to bottom.
Two stated differences from OpenCV: the accumulation order above decides a value that lies exactly on a threshold (OpenCV's
own order differs between its interior path, its border path and its builds), and the mask, which upstream warps as uint8,
is warped as 0.0 / 1.0 with "the rounded uint8 is at least 1" taken as v >= 0.5 (OpenCV's uint8 path has 15-bit fixed-point
weights and may differ for v within about 2^-11 of 0.5)."""
import functools
import pathlib

import numpy as np
import PIL.Image

from .flow import list_images
from .mask import epipolar_motion_mask
from .zoedepth import read_cameras

# compute_mask.py:71-125, class ids counted from 1
DYNAMIC_IDS_ADE20K = [13, 21, 77, 81, 84, 91, 93, 103, 104, 109, 116, 117, 118, 120, 127, 128, 140, 150]
DYNAMIC_IDS_COCO = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 26, 31, 32, 37, 38, 39]

DISK2 = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], dtype=bool)  # skimage.morphology.disk(2)
CONSIST_THRES = 1.0  # read_optical_flow's default, which combine_masks never overrides
WARP_CLAMP = 8       # the map coordinate is clamped to [-8, W + 8]
KEYS = ("ade20k", "coco", "sem", "warp_prev", "dyn_track", "dyn_cnt", "raw_no_warp", "raw", "raw_eroded", "final_raw", "final",
        "next_prev")


def erode_disk2(mask):
    from scipy import ndimage as ndi

    return ndi.binary_erosion(mask, structure=DISK2, border_value=True)


def dilate_disk2(mask):
    from scipy import ndimage as ndi

    return ndi.binary_dilation(mask, structure=DISK2, border_value=0)


def semantic_mask(sem_ade20k, sem_coco):
    """(ade20k, coco, sem) bool [H,W] (compute_mask.py:367-380): a pixel is set when its class id + 1 is in the list; -1,
    upstream's "probability below 0.1", is in neither"""
    ade20k = np.isin(np.asarray(sem_ade20k), np.array(DYNAMIC_IDS_ADE20K) - 1)
    coco = np.isin(np.asarray(sem_coco), np.array(DYNAMIC_IDS_COCO) - 1)
    return ade20k, coco, ade20k | coco


@functools.lru_cache(maxsize=None)
def _cubic_table():
    A, one = np.float32(-0.75), np.float32(1.0)
    f = np.arange(32, dtype=np.float32) * np.float32(1.0 / 32)
    g = one - f
    f1 = f + one
    c0 = ((A * f1 - np.float32(5) * A) * f1 + np.float32(8) * A) * f1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c2 = ((A + np.float32(2)) * g - (A + np.float32(3))) * g * g + one
    c3 = one - c0 - c1 - c2
    tab = np.stack([c0, c1, c2, c3], axis=1)
    assert tab.dtype == np.float32
    tab.setflags(write=False)
    return tab


def cubic_table():
    """the warp's 32 x 4 float32 weights: row k holds the four taps' weights of the fraction k / 32"""
    return _cubic_table()


def _split(coord, n):
    c = np.fmin(np.fmax(coord, np.float32(-WARP_CLAMP)), np.float32(n + WARP_CLAMP))
    s = np.rint(c * np.float32(32)).astype(np.int32)
    return s >> 5, s & 31


def warp_flow_numpy(img, flow):
    """img[H,W] sampled at p + flow[H,W,2] by the warp of the header comment: float32 in, float32 out"""
    img = np.ascontiguousarray(img, dtype=np.float32)
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    H, W = flow.shape[:2]
    if img.shape != (H, W) or flow.shape != (H, W, 2):
        raise ValueError(f"warp_flow_numpy: img {img.shape}, flow {flow.shape}")
    tab = cubic_table()
    ix, kx = _split(flow[..., 0] + np.arange(W, dtype=np.float32)[None, :], W)
    iy, ky = _split(flow[..., 1] + np.arange(H, dtype=np.float32)[:, None], H)
    cx, cy = tab[kx], tab[ky]
    pad = WARP_CLAMP + 4
    padded = np.zeros((H + 2 * pad, W + 2 * pad), np.float32)
    padded[pad:pad + H, pad:pad + W] = img
    with np.errstate(invalid="ignore", over="ignore"):
        acc = None
        for j in range(4):
            v = [padded[iy + (pad - 1 + j), ix + (pad - 1 + i)] for i in range(4)]
            w = [cy[..., j] * cx[..., i] for i in range(4)]
            row = ((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3]
            acc = row if j == 0 else acc + row
    return acc


def segment_counts(mask_sam, raw_eroded):
    """(n_pix, n_overlap) int64 [n_seg] each"""
    sam = np.asarray(mask_sam).astype(bool)
    n, size = sam.shape[0], raw_eroded.size
    return sam.reshape(n, size).sum(1), (sam & raw_eroded[None]).reshape(n, size).sum(1)


def segments_selected(n_pix, n_overlap, sam_overlap_thres=0.1):
    return (n_overlap > 0) & (n_overlap.astype(np.float64) > sam_overlap_thres * n_pix.astype(np.float64))


def _check_type(mask_type):
    if mask_type == "flow_depth":
        raise NotImplementedError("mask_type 'flow_depth': upstream's loop raises here too (compute_mask.py:780)")
    if mask_type not in ("semantic", "flow_epi"):
        raise ValueError(mask_type)


def _is_tensor(a):
    return hasattr(a, "is_cuda")


def _on(device, a, dtype=None):
    """``a`` on ``device``: a tensor already there is used in place, anything else is copied"""
    import torch

    t = a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device)


def combine_masks(*, mask_type, img_idx, mask_sam, sem_seg_ade20k=None, sem_seg_coco=None, mask_flow_epi=None,
                  prev_mask_final_raw=None, prev_dyn_cnt=None, bwd_flow=None, bwd_coord_diff=None,
                  normalized_dyn_track_thres=0.5, sam_overlap_thres=0.1, device=None):
    """upstream's combine_masks for frame ``img_idx`` with the backward flow handed in (``bwd_flow``, ``bwd_coord_diff``
    [H,W,2] float32: ``<frame>_<frame - k>.npz``) instead of read: its dict {ade20k, coco, sem, warp_prev, dyn_track, dyn_cnt,
    raw_no_warp, raw, raw_eroded, final_raw, final} (None where upstream has None) plus ``next_prev``, the next frame's
    ``prev_mask_final_raw``.  ``mask_sam`` is [n_seg,H,W] bool, n_seg >= 0.  ``device=None``: numpy in, numpy out.  A device:
    one ``ops.mask_combine``; masks come back as bool tensors and dyn_cnt as a float32 tensor on it, and ``mask_sam``,
    ``prev_*`` and ``bwd_*`` that already are tensors on it are used in place."""
    _check_type(mask_type)
    has_prev = prev_mask_final_raw is not None
    if has_prev and (prev_dyn_cnt is None or bwd_flow is None or bwd_coord_diff is None):
        raise ValueError("combine_masks: prev_mask_final_raw needs prev_dyn_cnt, bwd_flow and bwd_coord_diff")
    if device is not None:
        return _combine_device(mask_type, img_idx, mask_sam, sem_seg_ade20k, sem_seg_coco, mask_flow_epi, prev_mask_final_raw,
                               prev_dyn_cnt, bwd_flow, bwd_coord_diff, normalized_dyn_track_thres, sam_overlap_thres, device)
    ade20k = coco = sem = None
    if mask_type == "semantic":
        ade20k, coco, sem = semantic_mask(sem_seg_ade20k, sem_seg_coco)
        raw_no_warp = sem
    else:
        raw_no_warp = np.asarray(mask_flow_epi).astype(bool)
    mask_sam = np.asarray(mask_sam).astype(bool)
    if mask_sam.ndim != 3 or mask_sam.shape[1:] != raw_no_warp.shape:
        raise ValueError(f"combine_masks: mask_sam {mask_sam.shape} for a {raw_no_warp.shape} frame")
    warp_prev = dyn_track = None
    if has_prev:
        bwd_mask = (np.sum(np.abs(np.asarray(bwd_coord_diff, dtype=np.float32)), axis=2) <= CONSIST_THRES).astype(np.float32)
        warped = warp_flow_numpy(np.asarray(prev_mask_final_raw).astype(bool).astype(np.float32), bwd_flow)
        with np.errstate(invalid="ignore", over="ignore"):
            warp_prev = ((warped >= np.float32(0.5)).astype(np.float32) * bwd_mask) > np.float32(1e-3)
            cnt_warp = warp_flow_numpy(prev_dyn_cnt, bwd_flow)
            dyn_track = (cnt_warp / np.float32(img_idx + 1) * bwd_mask) > np.float32(normalized_dyn_track_thres)
        raw = raw_no_warp | erode_disk2(warp_prev & dyn_track)
    else:
        raw = raw_no_warp
    raw_eroded = erode_disk2(raw)
    n_pix, n_overlap = segment_counts(mask_sam, raw_eroded)
    final_raw = raw_eroded.copy()
    for k in np.nonzero(segments_selected(n_pix, n_overlap, sam_overlap_thres))[0]:
        final_raw |= mask_sam[k]
    if has_prev:
        with np.errstate(invalid="ignore", over="ignore"):
            dyn_cnt = cnt_warp + final_raw.astype(np.float32)
    else:
        dyn_cnt = raw_no_warp.astype(np.float32)
    return dict(ade20k=ade20k, coco=coco, sem=sem, warp_prev=warp_prev, dyn_track=dyn_track, dyn_cnt=dyn_cnt,
                raw_no_warp=raw_no_warp, raw=raw, raw_eroded=raw_eroded, final_raw=final_raw, final=dilate_disk2(final_raw),
                next_prev=erode_disk2(final_raw))


def _combine_device(mask_type, img_idx, mask_sam, sem_ade20k, sem_coco, mask_flow_epi, prev_mask, prev_cnt, bwd_flow,
                    bwd_coord_diff, dyn_track_thres, sam_overlap_thres, device):
    import torch

    from .. import ops

    ade20k = coco = sem = None
    if mask_type == "semantic":
        ade20k, coco, sem = ops.semantic_mask(_on(device, sem_ade20k, torch.int64), _on(device, sem_coco, torch.int64),
                                              DYNAMIC_IDS_ADE20K, DYNAMIC_IDS_COCO)
        raw_no_warp = sem
    else:
        raw_no_warp = _on(device, mask_flow_epi)
    prev = {}
    if prev_mask is not None:
        prev = dict(prev_mask=_on(device, prev_mask), prev_cnt=_on(device, prev_cnt, torch.float32),
                    bwd_flow=_on(device, bwd_flow, torch.float32), bwd_coord_diff=_on(device, bwd_coord_diff, torch.float32))
    out = ops.mask_combine(raw_no_warp, _on(device, mask_sam), img_idx=img_idx, dyn_track_thres=dyn_track_thres,
                           sam_overlap_thres=sam_overlap_thres, **prev)
    as_bool = lambda t: None if t is None else t.view(torch.bool)  # noqa: E731
    ret = {k: as_bool(out[k]) for k in ("warp_prev", "dyn_track", "raw", "raw_eroded", "final_raw", "final", "next_prev")}
    ret.update(ade20k=as_bool(ade20k), coco=as_bool(coco), sem=as_bool(sem), dyn_cnt=out["dyn_cnt"],
               raw_no_warp=as_bool(out["raw_no_warp"]))
    return {k: ret[k] for k in KEYS}


def _read_bgr(path):
    """detectron2's read_image(format="BGR"): the RGB image with its channels reversed, uint8 [H,W,3]"""
    return np.ascontiguousarray(np.asarray(PIL.Image.open(path).convert("RGB"))[:, :, ::-1])


def _segments(segmenter, img, device):
    seg = segmenter(np.copy(img))
    if device is None:
        seg = seg.detach().cpu().numpy() if _is_tensor(seg) else np.asarray(seg)
        seg = seg.astype(bool)
    else:
        import torch

        seg = _on(device, seg)
        seg = seg if seg.dtype in (torch.bool, torch.uint8) else seg != 0
    if seg.ndim != 3 or tuple(seg.shape[1:]) != img.shape[:2]:
        raise ValueError(f"run_masks: the segmenter's masks must be [n_seg,{img.shape[0]},{img.shape[1]}], got {tuple(seg.shape)}")
    return seg


def run_masks(*, root_dir, save_dir, segmenter, mask_type="flow_epi", semantic=None, flow_interval=1, flow_epi_thres=2.0,
              for_colmap=False, flag_dycheck_format=False, image_subdir="rgbs", device=None):
    """Writes upstream's motion masks for every image of ``<root_dir>/<image_subdir>`` (compute_mask.py:624-861 without
    argparse): ``<save_dir>/masks/final/<stem>_final.png`` and, for ``flow_epi``, ``<save_dir>/masks/flow_epi/<stem>.png``
    (uint8 0 / 255); with ``for_colmap`` everything goes under ``<save_dir>/masks_for_colmap/`` and instead of
    ``_final.png`` the INVERTED mask is written as ``masks_for_colmap/<image file name>.png``.  Masks are saved through PIL
    from bool arrays, as upstream.  Reads ``<root_dir>/flows/interval_<flow_interval>/`` (``flows_for_colmap/`` with
    ``for_colmap``) and, for ``flow_epi``, ``poses_bounds_cvd.npy`` or, with ``flag_dycheck_format``, ``camera.npz`` {all_K,
    all_w2c}.  ``segmenter(img_bgr uint8 [H,W,3]) -> bool [n_seg,H,W]`` (numpy or a tensor on any device) and, for
    ``mask_type="semantic"``, ``semantic(img_bgr) -> (ade20k, coco)``, int64 [H,W] class ids with -1 for invalid; both get
    BGR, as upstream hands its networks.  With a device the state (``next_prev``, ``dyn_cnt``) stays on it between frames and
    only ``final`` comes back per frame.  As upstream, frame i > 0 reads ``<stem i>_<stem i - flow_interval>.npz``.  The
    numbered debug PNGs, the SAM / OneFormer visualisations and the mp4 are not written.  Returns the paths written."""
    _check_type(mask_type)
    if segmenter is None:
        raise ValueError("run_masks needs a segmenter (segmenter(img_bgr[H,W,3]) -> bool [n_seg,H,W]); none is given")
    if mask_type == "semantic" and semantic is None:
        raise ValueError("run_masks needs semantic (semantic(img_bgr[H,W,3]) -> (ade20k, coco) int64 [H,W]) for "
                         "mask_type='semantic'; none is given")
    root_dir = pathlib.Path(root_dir)
    data_dirs = list(root_dir.glob(image_subdir))
    if len(data_dirs) != 1:
        raise ValueError(f"run_masks: {image_subdir!r} names {len(data_dirs)} directories of {root_dir}")
    images = list_images(data_dirs[0])
    names = [f.stem for f in images]
    flow_dir = root_dir / ("flows_for_colmap" if for_colmap else "flows") / f"interval_{flow_interval}"
    out_dir = pathlib.Path(save_dir) / ("masks_for_colmap" if for_colmap else "masks")
    out_dir_final = out_dir / "final"
    out_dir_final.mkdir(parents=True, exist_ok=True)
    if mask_type == "flow_epi":
        (out_dir / "flow_epi").mkdir(parents=True, exist_ok=True)
        if flag_dycheck_format:
            cam_info = np.load(root_dir / "camera.npz")
            all_K, all_w2c = cam_info["all_K"], cam_info["all_w2c"]
        else:
            all_w2c, all_K = read_cameras(root_dir, len(images), np.array(PIL.Image.open(images[0])).shape[:2])

    written = []
    prev_mask = prev_cnt = None
    for i, img_f in enumerate(images):
        img = _read_bgr(img_f)
        kw = {}
        if mask_type == "semantic":
            kw["sem_seg_ade20k"], kw["sem_seg_coco"] = semantic(np.copy(img))
        else:
            kw["mask_flow_epi"] = epipolar_motion_mask(i, len(images), all_w2c, all_K, flow_dir, names, flow_interval=flow_interval,
                                                       threshold=flow_epi_thres, device=device)
        if prev_mask is not None:
            info = np.load(flow_dir / f"{names[i]}_{names[i - flow_interval]}.npz")
            kw["bwd_flow"], kw["bwd_coord_diff"] = info["flow"], info["coord_diff"]
        res = combine_masks(mask_type=mask_type, img_idx=i, mask_sam=_segments(segmenter, img, device), prev_mask_final_raw=prev_mask,
                            prev_dyn_cnt=prev_cnt, device=device, **kw)
        prev_mask, prev_cnt = res["next_prev"], res["dyn_cnt"]
        final = res["final"] if device is None else res["final"].cpu().numpy()
        if mask_type == "flow_epi":
            written.append(out_dir / "flow_epi" / f"{img_f.stem}.png")
            PIL.Image.fromarray((kw["mask_flow_epi"] * 255).astype(np.uint8)).save(written[-1])
        if for_colmap:
            # "features will only be extracted from areas with mask values of 1"
            written.append(out_dir / f"{img_f.name}.png")
            PIL.Image.fromarray(~final).save(written[-1])
        else:
            written.append(out_dir_final / f"{img_f.stem}_final.png")
            PIL.Image.fromarray(final).save(written[-1])
    return written
