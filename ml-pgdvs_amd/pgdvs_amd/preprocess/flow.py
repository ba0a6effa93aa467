"""Flow consistency and the ``flows/interval_<k>/`` writer (pgdvs/preprocess/common.py:314-325 compute_occlusion,
compute_flow.py:27-58 DiffFlowDataset, :274-361 run).  The optical-flow network is a plug-in, as the tracker is for the
renderer: ``model(img_f1, img_f2) -> (flow12, flow21)`` and none ships."""
import pathlib

import numpy as np
import PIL.Image


def _hw2(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 2 or a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError(f"{name}: float32 [H,W,2] with H, W >= 2 expected, got {a.shape}")
    return a


def _sample_zeros(img, ix, iy):
    """grid_sample(bilinear, padding zeros) of img[H,W,2] at the pixel coordinates (ix, iy), float32: the weights
    w = ix - floor(ix), e = 1 - w (rows alike), a corner outside the image contributes zero, and the four products
    are summed nw, ne, sw, se."""
    H, W = img.shape[:2]
    one = np.float32(1.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    w, n = ix - x0, iy - y0
    e, s = one - w, one - n
    out = np.zeros(ix.shape + (2,), np.float32)
    for k, (cx, cy, wt) in enumerate(((x0, y0, e * s), (x0 + one, y0, w * s), (x0, y0 + one, e * n), (x0 + one, y0 + one, w * n))):
        ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
        xi = np.where(ok, cx, 0).astype(np.int64)
        yi = np.where(ok, cy, 0).astype(np.int64)
        val = np.where(ok[..., None], img[yi, xi], np.float32(0.0))
        term = val * wt[..., None]
        out = term if k == 0 else out + term
    return out


def coord_diff_numpy(flow12, flow21):
    """coord_diff of compute_occlusion(image1, flow12, flow21, return_raw=True) as [H,W,2], in float32 and in upstream's
    operation order: c1 = p + flow12, g = 2 c1 / (W - 1) - 1, ix = ((g + 1) / 2) (W - 1), the bilinear sample of flow21,
    p - (c1 + sample).  (The C ABI's pgdvs_flow_consistency is this statement per pixel; include/pgdvs_hip.h.)"""
    H, W = flow12.shape[:2]
    two, one = np.float32(2.0), np.float32(1.0)
    p = np.stack(np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)), axis=-1)
    c1 = p + flow12
    gx = two * c1[..., 0] / np.float32(W - 1) - one
    gy = two * c1[..., 1] / np.float32(H - 1) - one
    ix = ((gx + one) / two) * np.float32(W - 1)
    iy = ((gy + one) / two) * np.float32(H - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        c2 = c1 + _sample_zeros(flow21, ix, iy)
    return p - c2


def flow_consistency(flow12, flow21, device=None):
    """(coord_diff_1, coord_diff_2), float32 [H,W,2] numpy each: the forward-backward residual of flow12 checked against
    flow21 and of flow21 against flow12 (compute_flow.py:335-340).  ``device=None``: numpy on the host;
    otherwise one HIP launch on ``device`` (``ops.flow_consistency``)."""
    f12, f21 = _hw2(flow12, "flow12"), _hw2(flow21, "flow21")
    if f12.shape != f21.shape:
        raise ValueError(f"flow_consistency: flow12 {f12.shape} and flow21 {f21.shape} differ")
    if device is None:
        return coord_diff_numpy(f12, f21), coord_diff_numpy(f21, f12)
    import torch

    from .. import ops

    cd1, cd2 = ops.flow_consistency(torch.from_numpy(f12).to(device), torch.from_numpy(f21).to(device))
    return cd1.cpu().numpy(), cd2.cpu().numpy()


def write_flow_pair(flow_dir, stem1, stem2, flow12, flow21, device=None):
    """Writes ``<stem1>_<stem2>.npz`` {flow: flow12, coord_diff: coord_diff_1} and ``<stem2>_<stem1>.npz`` {flow: flow21,
    coord_diff: coord_diff_2} into ``flow_dir`` (compute_flow.py:351-358), the files ``datasets._common.read_flow_npz``
    reads.  Returns the two paths."""
    flow_dir = pathlib.Path(flow_dir)
    f12, f21 = _hw2(flow12, "flow12"), _hw2(flow21, "flow21")
    cd1, cd2 = flow_consistency(f12, f21, device=device)
    paths = (flow_dir / f"{stem1}_{stem2}.npz", flow_dir / f"{stem2}_{stem1}.npz")
    np.savez(paths[0], flow=f12, coord_diff=cd1)
    np.savez(paths[1], flow=f21, coord_diff=cd2)
    return paths


def list_images(input_dir):
    """every file of ``input_dir`` with an extension PIL can open, sorted (DiffFlowDataset, compute_flow.py:38-47)"""
    exts = PIL.Image.registered_extensions()
    found = []
    for ext in {ex for ex, f in exts.items() if f in PIL.Image.OPEN}:
        found += list(pathlib.Path(input_dir).glob(f"*{ext}"))
    return sorted(found)


def _model_flow(flow, name):
    """the model's [1,2,H,W] (a tensor on any device, or an array) -> float32 [H,W,2] numpy"""
    if hasattr(flow, "detach"):
        flow = flow.detach().cpu().numpy()
    flow = np.asarray(flow, dtype=np.float32)
    if flow.ndim != 4 or flow.shape[0] != 1 or flow.shape[1] != 2:
        raise ValueError(f"run_flow: the model's {name} must be [1,2,H,W], got {flow.shape}")
    return np.ascontiguousarray(flow[0].transpose(1, 2, 0))


def run_flow(input_dir, out_dir, model, img_pair_max_diff=3, device=None):
    """Writes upstream's flow tree (compute_flow.py:274-361 run): ``out_dir/interval_<k>/`` for k = 1..img_pair_max_diff,
    in it both ``.npz`` of every pair (i, i + k) of the sorted images of ``input_dir``.  ``model(img_f1, img_f2)`` takes the
    two image paths and returns (flow12, flow21), each [1,2,H,W].  Neither the colour-wheel PNGs nor the debug collage are
    written.  Returns the paths written, in order."""
    if model is None:
        raise RuntimeError("run_flow needs an optical-flow model (model(img_f1, img_f2) -> (flow12, flow21)); none is given")
    images = list_images(input_dir)
    written = []
    for k in range(1, int(img_pair_max_diff) + 1):
        flow_dir = pathlib.Path(out_dir) / f"interval_{k}"
        flow_dir.mkdir(parents=True, exist_ok=True)
        for i in range(0, len(images) - k):
            fn1, fn2 = images[i], images[i + k]
            flow12, flow21 = model(fn1, fn2)
            written += write_flow_pair(flow_dir, fn1.stem, fn2.stem, _model_flow(flow12, "flow12"), _model_flow(flow21, "flow21"),
                                       device=device)
    return written
