"""The ZoeDepth stage's own arithmetic (pgdvs/preprocess/compute_zoedepth.py): where the COLMAP points land in a frame
(:262-294 sample_frame), the median and trimmed-median scale and shift that align the predicted depth with them in
disparity (:309-388 fit_frame), the error table ``use_zoe_depth="moe"`` chooses by (:424-465 frame_errors), and the
``zoe_depths_<type>/<frame>.npz`` writer (run_zoedepth, the script with ``--save_space``).  The depth network is a
plug-in, as the flow network is for ``run_flow``: ``model(img[1,3,H,W]) -> [1,1,H,W]`` metric depth, and none ships.

``device=None`` restates upstream's lines with the same numpy and scipy calls on the host (scipy is imported on first
use); a device runs the HIP ops (``ops.zoe_sample``, ``ops.zoe_fit``, ``ops.zoe_errors``; csrc/zoe_align.hip).  The values
are those of NumPy 2, whose promotion rules keep ``nn_disp`` and its median float32 and make the ratios float64.

``spline_coefficients_numpy`` / ``spline_sample_numpy`` state in plain numpy what the kernels compute for
``scipy.ndimage.map_coordinates(order=3, mode="constant")``; they document the kernel and are pinned against scipy by
the tests, nothing here calls them."""
import pathlib
import struct

import numpy as np
import PIL.Image

from .flow import list_images

TINY_VAL = 1.0e-16
FIT_KEYS = ("disp_indiv_scale_med", "disp_indiv_shift_med", "disp_indiv_scale_trim", "disp_indiv_shift_trim")
# the (scale, shift) pairs the error table is made for, in the order of the op's outputs
ERROR_PAIRS = ("med_share", "med_indiv", "trim_share", "trim_indiv")


# ---------------------------------------------------------------------------- the spline, restated
POLE = np.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)


def _filter_line(c):
    """scipy's cubic spline prefilter of one line, float64, in place: gain, causal recursion from the mirror start,
    anticausal recursion from the mirror end"""
    n = c.shape[0]
    z = POLE
    c *= GAIN
    zn1 = z ** (n - 1)
    c0 = c[0] + zn1 * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 += zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= z
    c[0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])


def spline_coefficients_numpy(img):
    """float64 cubic B-spline coefficients of img[H,W], H, W >= 2: axis 0, then axis 1"""
    c = np.array(img, dtype=np.float64)
    for col in range(c.shape[1]):
        _filter_line(c[:, col])
    for row in range(c.shape[0]):
        _filter_line(c[row, :])
    return c


def _mirror(i, n):
    p = 2 * (n - 1)
    i = i % p
    return i if i < n else p - i


def _cubic_weights(f):
    z = 1.0 - f
    w1 = (f * f * (f - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return w0, w1, w2, 1.0 - w0 - w1 - w2


def spline_sample_numpy(coef, rows, cols):
    """float32 samples of the coefficients at (rows, cols): 0 outside [0, H-1] x [0, W-1], else the 4 x 4 taps with
    mirrored indices, summed row-major in float64 and rounded once"""
    H, W = coef.shape
    out = np.zeros(len(rows), np.float32)
    for k, (r, c) in enumerate(zip(rows, cols)):
        if not (0.0 <= r <= H - 1 and 0.0 <= c <= W - 1):
            continue
        fr, fc = np.floor(r), np.floor(c)
        wr, wc = _cubic_weights(r - fr), _cubic_weights(c - fc)
        t = 0.0
        for i in range(4):
            line = coef[_mirror(int(fr) - 1 + i, H)]
            for j in range(4):
                t += line[_mirror(int(fc) - 1 + j, W)] * wr[i] * wc[j]
        out[k] = np.float32(t)
    return out


# ---------------------------------------------------------------------------- inputs
def _image(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError(f"{name}: float32 [H,W] with H, W >= 2 expected, got {a.shape}")
    return a


def _frame_name(frame):
    return "the frame" if frame is None else f"frame {frame}"


def _samples(pcl_depth_pred, pcl_depth_mvs, frame):
    pred = np.ascontiguousarray(pcl_depth_pred, dtype=np.float32).reshape(-1)
    mvs = np.ascontiguousarray(pcl_depth_mvs, dtype=np.float64).reshape(-1)
    if pred.shape != mvs.shape:
        raise ValueError(f"{_frame_name(frame)}: {pred.shape[0]} predicted and {mvs.shape[0]} MVS depths")
    if pred.shape[0] == 0:
        raise ValueError(f"{_frame_name(frame)}: no COLMAP point is left to fit to (none projects into a static area in front of "
                         "the camera)")
    return pred, mvs


def _to(device, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------- sample_frame
def sample_frame(pred_depth, mask, pts3d, w2c, K, device=None):
    """(proj_pcl [3,n] float64, pcl_depth_mvs [n] float64, pcl_depth_pred [n] float32, kept [n] int64, ascending): the
    points ``pts3d[P,3]`` projected with ``w2c[4,4]`` and ``K[3,3]``, kept inside [0,W) x [0,H), where the cubic-spline
    sample of ``mask`` is < 0.1 and the depth > 1e-3, and the spline sample of ``pred_depth`` there (:262-294).  As
    upstream, a point in the last fractional column or row samples 0 from both images: it counts as static and carries a
    predicted depth of 0.  ``pred_depth`` may already be a tensor on ``device``."""
    on_device = device is not None and hasattr(pred_depth, "is_cuda")
    pred = pred_depth if on_device else _image(pred_depth, "pred_depth")
    mask = _image(mask, "mask")
    if tuple(pred.shape) != mask.shape:
        raise ValueError(f"sample_frame: pred_depth {tuple(pred.shape)} and mask {mask.shape} differ")
    pts3d = np.ascontiguousarray(pts3d, dtype=np.float32).reshape(-1, 3)
    w2c, K = np.asarray(w2c, dtype=np.float64).reshape(4, 4), np.asarray(K, dtype=np.float64).reshape(3, 3)
    if pts3d.shape[0] == 0:
        return np.zeros((3, 0)), np.zeros(0), np.zeros(0, np.float32), np.zeros(0, np.int64)
    if device is not None:
        from .. import ops

        out = ops.zoe_sample(pred if on_device else _to(device, pred), _to(device, mask), _to(device, pts3d), w2c, K)
        return tuple(t.cpu().numpy() for t in out)
    from scipy.ndimage import map_coordinates

    img_h, img_w = mask.shape
    h_pt = np.ones([pts3d.shape[0], 4])
    h_pt[:, :3] = pts3d
    h_pt = h_pt.T
    with np.errstate(divide="ignore", invalid="ignore"):
        out = w2c @ h_pt
        im_pt = K @ out[:3, :]
        depth = im_pt[2, :].copy()
        im_pt = im_pt / im_pt[2:, :]
        kept = np.where((im_pt[0, :] >= 0) * (im_pt[0, :] < img_w) * (im_pt[1, :] >= 0) * (im_pt[1, :] < img_h))[0]
    pts, depth = im_pt[:, kept], depth[kept]
    sel = np.where(map_coordinates(mask, [pts[1, :], pts[0, :]]) < 0.1)[0]  # static areas
    pts, depth, kept = pts[:, sel], depth[sel], kept[sel]
    sel = np.where(depth > 1e-3)[0]
    pts, depth, kept = pts[:, sel], depth[sel], kept[sel]
    return pts, depth, map_coordinates(pred, [pts[1, :], pts[0, :]]), kept.astype(np.int64)


# ---------------------------------------------------------------------------- fit_frame
def _clamped(scale):
    return 0.0 if scale < 0 else scale  # "We should not change the relative order of predicted depth"


def fit_frame(pcl_depth_pred, pcl_depth_mvs, device=None, frame=None):
    """({disp_indiv_scale_med, disp_indiv_shift_med, disp_indiv_scale_trim, disp_indiv_shift_trim} as float64,
    flag_trim [n] bool) of one frame's samples (:309-388): scale = median of the ratio of the median-centred disparities
    (negative: 0), shift = median of mvs_disp - nn_disp scale; once over all samples, once over those whose normalised
    disparities differ by no more than the 0.8 quantile of that difference.  An empty frame or a negative depth raises
    ValueError naming ``frame`` (upstream dies there on np.min of an empty array or on its assertion)."""
    pred, mvs = _samples(pcl_depth_pred, pcl_depth_mvs, frame)
    if device is not None:
        from .. import ops

        fit, flag, status = ops.zoe_fit(_to(device, pred), _to(device, mvs))
        _raise_negative(int(status.item()) & 1, int(status.item()) & 2, frame)
        return dict(zip(FIT_KEYS, fit.cpu().numpy())), flag.cpu().numpy()
    _raise_negative(np.min(pred) < 0 or np.isnan(pred).any(), np.min(mvs) < 0 or np.isnan(mvs).any(), frame)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nn_disp = 1 / (pred + TINY_VAL)  # float32: the Python scalar joins the array's type
        mvs_disp = 1 / (mvs + TINY_VAL)
        nn_disp_shifted = nn_disp - np.median(nn_disp)
        mvs_disp_shifted = mvs_disp - np.median(mvs_disp)
        ratio = mvs_disp_shifted / (nn_disp_shifted + TINY_VAL)
        scale_med = _clamped(np.median(ratio))
        shift_med = np.median(mvs_disp - nn_disp * scale_med)
        nn_disp_normalized = nn_disp_shifted / (np.mean(np.abs(nn_disp_shifted)) + TINY_VAL)
        mvs_disp_normalized = mvs_disp_shifted / (np.mean(np.abs(mvs_disp_shifted)) + TINY_VAL)
        diff = np.abs(nn_disp_normalized - mvs_disp_normalized)
        flag_trim = diff <= np.quantile(diff, 0.8)
        scale_trim = _clamped(np.median(ratio[flag_trim]))
        shift_trim = np.median(mvs_disp[flag_trim] - nn_disp[flag_trim] * scale_trim)
    return dict(zip(FIT_KEYS, (np.float64(v) for v in (scale_med, shift_med, scale_trim, shift_trim)))), flag_trim


def _raise_negative(pred_negative, mvs_negative, frame):
    if pred_negative:
        raise ValueError(f"{_frame_name(frame)}: the predicted depth is negative at a sampled point")
    if mvs_negative:
        raise ValueError(f"{_frame_name(frame)}: a kept COLMAP point has a negative depth")


# ---------------------------------------------------------------------------- frame_errors
def frame_errors(pcl_depth_pred, pcl_depth_mvs, flag_trim, scales_shifts, device=None):
    """{mae_<fit>_<scope>, me_<fit>_<scope>} float64 for fit in (med, trim), scope in (share, indiv) (:424-465): over the
    samples of ``flag_trim``, the mean absolute and the mean error of mvs_depth - 1 / (nn_disp scale + shift), with the
    ``disp_<scope>_{scale,shift}_<fit>`` entries of ``scales_shifts``."""
    pred, mvs = _samples(pcl_depth_pred, pcl_depth_mvs, None)
    flag = np.ascontiguousarray(flag_trim, dtype=bool).reshape(-1)
    pairs = [(scales_shifts[f"disp_{scope}_scale_{fit}"], scales_shifts[f"disp_{scope}_shift_{fit}"])
             for fit, scope in (p.split("_") for p in ERROR_PAIRS)]
    if device is not None:
        from .. import ops

        err = ops.zoe_errors(_to(device, pred), _to(device, mvs), _to(device, flag), np.array(pairs, np.float64)).cpu().numpy()
        return {f"{kind}_{p}": err[4 * k + j] for k, kind in enumerate(("mae", "me")) for j, p in enumerate(ERROR_PAIRS)}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mvs_depth_trim = mvs[flag]
        nn_disp_trim = 1 / (pred[flag] + TINY_VAL)
        out = {}
        for p, (scale, shift) in zip(ERROR_PAIRS, pairs):
            diff = mvs_depth_trim - 1 / (nn_disp_trim * scale + shift)
            out[f"mae_{p}"], out[f"me_{p}"] = np.mean(np.abs(diff)), np.mean(diff)
    return {f"{kind}_{p}": np.float64(out[f"{kind}_{p}"]) for kind in ("mae", "me") for p in ERROR_PAIRS}


# ---------------------------------------------------------------------------- the scene's files
def read_points3d_xyz(path):
    """xyz [P,3] float64 of COLMAP's ``points3D.bin``, in file order: a uint64 count, then per point a uint64 id, three
    doubles xyz, three bytes rgb, a double error, a uint64 track length and that many (int32 image, int32 point2D) pairs;
    little endian"""
    data = pathlib.Path(path).read_bytes()
    (n,) = struct.unpack_from("<Q", data, 0)
    xyz = np.empty((n, 3), np.float64)
    off = 8
    for i in range(n):
        xyz[i] = struct.unpack_from("<3d", data, off + 8)
        (track,) = struct.unpack_from("<Q", data, off + 43)
        off += 51 + 8 * track
    if off != len(data):
        raise ValueError(f"{path}: {len(data) - off} bytes left after {n} points")
    return xyz


def read_cameras(root_dir, n_frames, shape):
    """(w2c [F,4,4], K [F,3,3]) float64 from ``poses_bounds_cvd.npy`` (common.py read_poses_nvidia_long, hwf_to_K; the
    script's :200-220): float32 poses widened, OpenCV axes, the focal length of ``hwf`` with the image's own size"""
    from ..datasets.nvidia_eval import read_llff_cams

    hwf, c2w = read_llff_cams(pathlib.Path(root_dir) / "poses_bounds_cvd.npy")
    if hwf.shape[0] != n_frames:
        raise ValueError(f"poses_bounds_cvd.npy holds {hwf.shape[0]} cameras for {n_frames} images")
    img_h, img_w = shape
    hwf[:, 0], hwf[:, 1] = img_h, img_w
    Ks = []
    for h, w, f in hwf:
        K = np.eye(3)
        K[0, 0] = K[1, 1] = f
        K[0, 2], K[1, 2] = w / 2.0, h / 2.0
        K[0, :] = K[0, :] * img_w / w
        K[1, :] = K[1, :] * img_h / h
        Ks.append(K)
    return np.array([np.linalg.inv(m) for m in c2w]), np.array(Ks)


def _predict(model, img, shape, device):
    """the plug-in's [1,1,H,W] for img[H,W,3] in [0,1] -> float32 [H,W]: numpy on the host path, a tensor on ``device``"""
    import torch

    X = torch.from_numpy(np.ascontiguousarray(img))[None].permute(0, 3, 1, 2)
    with torch.no_grad():
        pred = model(X if device is None else X.to(device))
    if not hasattr(pred, "detach"):
        pred = torch.from_numpy(np.asarray(pred, dtype=np.float32))
    pred = pred.detach().float()
    if pred.ndim != 4 or tuple(pred.shape[:2]) != (1, 1) or tuple(pred.shape[2:]) != tuple(shape):
        raise ValueError(f"run_zoedepth: the model's depth must be [1,1,{shape[0]},{shape[1]}], got {tuple(pred.shape)}")
    return pred[0, 0].cpu().numpy() if device is None else pred[0, 0].contiguous().to(device)


def run_zoedepth(root_dir, save_dir, mask_dir, model, zoedepth_type, image_subdir="rgbs", device=None):
    """Writes upstream's ``<save_dir>/zoe_depths_<type>/<i:05d>.npz`` for every image of ``<root_dir>/<image_subdir>``
    (compute_zoedepth.py with ``--save_space``): upstream's 22 entries (``datasets.nvidia_eval`` reads 13 of them), in its dtypes and
    shapes.  Reads ``<root_dir>/poses_bounds_cvd.npy``, ``<root_dir>/sparse/points3D.bin`` and the motion masks
    ``<mask_dir>/masks/final/<i:05d>_final.png``.  ``model(img[1,3,H,W] float32 in [0,1]) -> [1,1,H,W]`` metric depth.  The
    share values are np.mean of the per-frame fits, on the host.  No ``.ply`` is written.  Returns the paths written."""
    if model is None:
        raise ValueError("run_zoedepth needs a depth model (model(img[1,3,H,W]) -> [1,1,H,W]); none is given")
    if zoedepth_type not in ("N", "K", "NK"):
        raise ValueError(zoedepth_type)
    root_dir = pathlib.Path(root_dir)
    data_dirs = list(root_dir.glob(image_subdir))
    if len(data_dirs) != 1:
        raise ValueError(f"run_zoedepth: {image_subdir!r} names {len(data_dirs)} directories of {root_dir}")
    images = list_images(data_dirs[0])
    masks = [pathlib.Path(mask_dir) / "masks/final" / f"{int(f.stem):05d}_final.png" for f in images]
    for f in masks:
        if not f.exists():
            raise FileNotFoundError(f)
    depth_dir = pathlib.Path(save_dir) / f"zoe_depths_{zoedepth_type.lower()}"
    depth_dir.mkdir(parents=True, exist_ok=True)
    shape = np.array(PIL.Image.open(images[0])).shape[:2]
    all_w2c, all_K = read_cameras(root_dir, len(images), shape)
    pts3d = read_points3d_xyz(root_dir / "sparse/points3D.bin").astype(np.float32)

    frames = []
    for i, (img_f, mask_f) in enumerate(zip(images, masks)):
        img = np.asarray(PIL.Image.open(img_f)).astype(np.float32) / 255
        pred = _predict(model, img, img.shape[:2], device)
        mask = np.array(PIL.Image.open(mask_f)).astype(np.float32)  # a true value means dynamic
        pts, mvs, sampled, _ = sample_frame(pred, mask, pts3d, all_w2c[i], all_K[i], device=device)
        full = pred if device is None else pred.cpu().numpy()
        if full.min() < 0:
            raise ValueError(f"frame {i}: the predicted depth is negative ({full.min()})")
        fit, flag_trim = fit_frame(sampled, mvs, device=device, frame=i)
        frames.append(dict(proj_pcl=pts, pcl_depth_mvs=mvs, pcl_depth_pred=sampled, depth_pred=full, fit=fit, flag_trim=flag_trim))

    share = {k.replace("indiv", "share"): np.mean([fr["fit"][k] for fr in frames]) for k in FIT_KEYS}
    written = []
    for i, fr in enumerate(frames):
        scales_shifts = dict(fr["fit"], **share)
        errors = frame_errors(fr["pcl_depth_pred"], fr["pcl_depth_mvs"], fr["flag_trim"], scales_shifts, device=device)
        save_dict = dict(scales_shifts, sparse_pcl=pts3d, proj_pcl=fr["proj_pcl"], pcl_depth_mvs=fr["pcl_depth_mvs"],
                         pcl_depth_pred=fr["pcl_depth_pred"], depth_pred=fr["depth_pred"], depth_is_disp=False, **errors)
        with open(depth_dir / f"{i:05d}.npz", "wb") as f:
            np.savez(f, **save_dict)
        written.append(depth_dir / f"{i:05d}.npz")
    return written
