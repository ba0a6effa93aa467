"""The flow stage of upstream's preprocessing (pgdvs/preprocess/compute_flow.py): flow consistency (common.py:314-325
compute_occlusion), the colour-wheel picture of a flow (common.py:93-205 flow_to_image), FlowFormer's tiled inference around
a tile-sized network (compute_flow.py:61-82 compute_grid_indices, :138-165 compute_weight, :168-212 the tile branch of
compute_flow_flowformer) and the ``flows/interval_<k>/`` writer (:27-58 DiffFlowDataset, :274-361 run).  The optical-flow
network is a plug-in, as the tracker is for the renderer: ``model(img_f1, img_f2) -> (flow12, flow21)`` and none ships."""
import math
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


# ---- the flow picture ----

WHEEL_SEGMENTS = (15, 6, 4, 11, 13, 6)  # red-yellow, yellow-green, green-cyan, cyan-blue, blue-magenta, magenta-red


def colour_wheel():
    """The Middlebury colour wheel (Baker et al., ICCV 2007), float64 [55,3]: six segments of WHEEL_SEGMENTS entries; along a
    segment one channel stays 255, one ramps by floor(255 j / length) -- up in the even segments, down in the odd ones -- and
    one stays 0."""
    full, ramp = (0, 1, 1, 2, 2, 0), (1, 0, 2, 1, 0, 2)
    wheel = np.zeros((sum(WHEEL_SEGMENTS), 3))
    k = 0
    for s, n in enumerate(WHEEL_SEGMENTS):
        r = np.floor(255 * np.arange(n) / n)
        wheel[k:k + n, full[s]] = 255
        wheel[k:k + n, ramp[s]] = r if s % 2 == 0 else 255 - r
        k += n
    return wheel


def _flow_hw2(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name}: float32 [H,W,2] expected, got {a.shape}")
    return a


def flow_normalised(flow):
    """(rad_max, u, v) of flow_to_image (common.py:198-204), float32: the largest radius sqrt(u u + v v) of the frame (NaN if
    any radius is NaN) and both components divided by float32(rad_max + float32(1e-5))"""
    f = _flow_hw2(flow, "flow")
    u, v = f[..., 0], f[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        rad_max = np.max(np.sqrt(u * u + v * v))
        denom = np.float32(rad_max + np.float32(1e-5))
        return rad_max, u / denom, v / denom


def wheel_colours(u, v):
    """flow_uv_to_colors (common.py:143-179) on the normalised components, upstream's types under NumPy 2: radius, angle and
    fk = (atan2(-v, -u) / pi + 1) / 2 * 54 in float32; from the interpolation between the wheel entries floor(fk) and its
    successor (55 wraps to 0) on in float64: col = 1 - rad (1 - col) where rad <= 1, else 0.75 col; byte floor(255 col).  A
    pixel whose u or v is NaN gives 0 0 0 (upstream casts NaN to an integer there, which is undefined)."""
    wheel = colour_wheel()
    n = wheel.shape[0]
    one, two = np.float32(1.0), np.float32(2.0)
    bad = np.isnan(u) | np.isnan(v)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(u * u + v * v)
        a = np.arctan2(-v, -u) / np.float32(np.pi)
        fk = (a + one) / two * np.float32(n - 1)
        k0 = np.clip(np.where(bad, 0, np.floor(fk)), 0, n - 1).astype(np.int32)
        k1 = np.where(k0 + 1 == n, 0, k0 + 1)
        f = fk.astype(np.float64) - k0
        img = np.zeros(u.shape + (3,), np.uint8)
        for c in range(3):
            col = (1 - f) * (wheel[k0, c] / 255.0) + f * (wheel[k1, c] / 255.0)
            col = np.where(rad <= 1, 1 - rad.astype(np.float64) * (1 - col), col * 0.75)
            img[..., c] = np.where(bad, 0, np.clip(np.floor(255 * col), 0, 255)).astype(np.uint8)
    return img


def flow_to_image(flow, device=None):
    """The colour-wheel picture of flow[H,W,2] as uint8 [H,W,3] (common.py:182-205 flow_to_image): hue from the direction,
    saturation from the radius relative to the frame's largest.  ``device=None``: numpy on the host, in upstream's
    operation order and types; otherwise the HIP kernel on ``device`` (``ops.flow_image``), whose ``atan2f`` may move a byte
    by one level where 255 col lies next to an integer."""
    f = _flow_hw2(flow, "flow")
    if device is None:
        _, u, v = flow_normalised(f)
        return wheel_colours(u, v)
    import torch

    from .. import ops

    _, lines = ops.flow_image(torch.from_numpy(f).to(device), adaptive=False)
    H, W = f.shape[:2]
    return np.ascontiguousarray(lines[:, 1:].cpu().numpy().reshape(H, W, 3))


# ---- tiled inference ----

PATCH_SIZE = (432, 960)  # FlowFormer's training size


def tile_origins(image_shape, patch_size=PATCH_SIZE, min_overlap=20):
    """Upstream's list of tile origins (h, w) for an image (compute_flow.py:61-82): per axis every ``patch - min_overlap``
    pixels from 0 (a dimension equal to the patch: the one origin 0), the last one moved so that its tile ends flush with the
    border -- which may put it before its predecessor -- and the rows of the list in h-major order."""
    H, W = int(image_shape[0]), int(image_shape[1])
    ph, pw = int(patch_size[0]), int(patch_size[1])
    if min_overlap >= ph or min_overlap >= pw:
        raise ValueError(f"tile_origins: min_overlap {min_overlap} must be smaller than the patch {(ph, pw)}")
    if H < ph or W < pw:
        raise ValueError(f"tile_origins: the image {(H, W)} is smaller than the patch {(ph, pw)}")
    hs = list(range(0, H, ph if H == ph else ph - min_overlap))
    ws = list(range(0, W, pw if W == pw else pw - min_overlap))
    hs[-1], ws[-1] = H - ph, W - pw
    return [(h, w) for h in hs for w in ws]


def tile_weight(patch_size=PATCH_SIZE, sigma=0.05):
    """Upstream's Gaussian tile weight, float32 [ph,pw] torch on the CPU, in its operation order (compute_flow.py:147-153):
    the distance of (i / ph - 0.5, j / pw - 0.5) from the origin over sigma, through exp(-d^2 / 2) / (sigma sqrt(2 pi)).  At
    sigma 0.05 the corners are float32 denormals, none is zero."""
    import torch

    ph, pw = int(patch_size[0]), int(patch_size[1])
    h, w = torch.meshgrid(torch.arange(ph), torch.arange(pw), indexing="ij")
    h, w = h / float(ph), w / float(pw)
    h, w = h - 0.5, w - 0.5
    d = (h ** 2 + w ** 2) ** 0.5 / sigma
    return (1 / (sigma * math.sqrt(2 * math.pi))) * torch.exp(-0.5 * d ** 2)


def _as_tiles(tile_flows, device):
    import torch

    if isinstance(tile_flows, (list, tuple)):
        tile_flows = torch.stack([torch.as_tensor(np.asarray(t) if not hasattr(t, "detach") else t) for t in tile_flows])
    t = torch.as_tensor(tile_flows).detach().to(torch.float32)
    if t.ndim == 5 and t.shape[1] == 1:
        t = t[:, 0]
    if t.ndim != 4 or t.shape[1] != 2:
        raise ValueError(f"blend_tiles: tile flows [n,2,ph,pw] expected, got {tuple(t.shape)}")
    return t.to(device if device is not None else "cpu")


def blend_tiles(tile_flows, origins, image_shape, weight, device=None):
    """The flow of an image from the flows of its tiles (compute_flow.py:183-209): tile_flows[n,2,ph,pw] (or n arrays
    [2,ph,pw]), their ``origins`` and the weight[ph,pw] -> flow[H,W,2] float32.  ``device=None``: torch on the CPU as
    upstream -- flows += pad(tile * weight), count += pad(weight), flows / count -- returned as numpy; otherwise one HIP
    launch (``ops.flow_tile_blend``) and a tensor on ``device``."""
    import torch

    H, W = int(image_shape[0]), int(image_shape[1])
    t = _as_tiles(tile_flows, device)
    wt = torch.as_tensor(weight).detach().to(torch.float32)
    org = [(int(h), int(w)) for h, w in origins]
    n, _, ph, pw = t.shape
    if len(org) != n or tuple(wt.shape) != (ph, pw):
        raise ValueError(f"blend_tiles: {n} tiles of {(ph, pw)}, {len(org)} origins, weight {tuple(wt.shape)}")
    if device is not None:
        from .. import ops

        return ops.flow_tile_blend(t, org, wt.to(device), H, W)
    wt = wt.cpu()[None, None]
    flows, count = 0, 0
    for idx, (h, w) in enumerate(org):
        if not (0 <= h <= H - ph and 0 <= w <= W - pw):
            raise ValueError(f"blend_tiles: origin {(h, w)} puts a {(ph, pw)} tile outside the {(H, W)} image")
        padding = (w, W - w - pw, h, H - h - ph, 0, 0)
        flows += torch.nn.functional.pad(t[idx:idx + 1] * wt, padding)
        count += torch.nn.functional.pad(wt, padding)
    if not bool((count != 0).all()):
        raise ValueError(f"blend_tiles: the tiles leave a pixel of the {(H, W)} image uncovered")
    return np.ascontiguousarray((flows / count)[0].permute(1, 2, 0).numpy())


def tiled_flow(tile_model, image1, image2, sigma=0.05, patch_size=PATCH_SIZE, device=None, weight=None):
    """The tile branch of compute_flow_flowformer (compute_flow.py:182-212) around a tile-sized network: image1, image2
    [1,3,H,W] float tensors; ``tile_model(img1_tile[1,3,ph,pw], img2_tile)`` returns the tile's flow [1,2,ph,pw], or a tuple
    whose first element is that (FlowFormer returns ``(flow_pre, _)``).  Returns the image's flow [1,2,H,W], the form
    ``run_flow`` takes from its model: a CPU tensor, or with ``device`` a view of the blended [H,W,2] tensor on it -- the
    images go to ``device`` before the network sees them, and the tile flows never leave it.  ``weight``: a table [ph,pw] to
    use instead of ``tile_weight(patch_size, sigma)``."""
    import torch

    image1, image2 = torch.as_tensor(image1), torch.as_tensor(image2)
    if image1.ndim != 4 or image1.shape[0] != 1 or image1.shape != image2.shape:
        raise ValueError(f"tiled_flow: two images [1,C,H,W] of one shape expected, got {tuple(image1.shape)}, {tuple(image2.shape)}")
    if device is not None:
        image1, image2 = image1.to(device), image2.to(device)
    H, W = int(image1.shape[2]), int(image1.shape[3])
    ph, pw = int(patch_size[0]), int(patch_size[1])
    origins = tile_origins((H, W), (ph, pw))
    weight = tile_weight((ph, pw), sigma) if weight is None else weight
    tiles = []
    for h, w in origins:
        out = tile_model(image1[:, :, h:h + ph, w:w + pw], image2[:, :, h:h + ph, w:w + pw])
        out = out[0] if isinstance(out, (tuple, list)) else out
        out = torch.as_tensor(out)
        if tuple(out.shape) != (1, 2, ph, pw):
            raise ValueError(f"tiled_flow: the tile model must return [1,2,{ph},{pw}], got {tuple(out.shape)}")
        tiles.append(out.detach()[0].to(device if device is not None else "cpu"))
    flow = blend_tiles(torch.stack(tiles), origins, (H, W), weight, device=device)
    flow = torch.from_numpy(flow) if device is None else flow
    return flow.permute(2, 0, 1)[None]


# ---- the writer ----

MAX_PNG_THREADS = 8


def _on_device(flow, name, device):
    """a flow [H,W,2] (array or tensor, anywhere) as a contiguous float32 tensor on ``device``: uploaded once, or left there"""
    import torch

    t = flow.detach() if hasattr(flow, "detach") else torch.from_numpy(_hw2(flow, name))
    if t.ndim != 3 or t.shape[2] != 2 or t.shape[0] < 2 or t.shape[1] < 2:
        raise ValueError(f"{name}: float32 [H,W,2] with H, W >= 2 expected, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


def write_flow_pair(flow_dir, stem1, stem2, flow12, flow21, device=None, flow_png=False, writer=None):
    """Writes ``<stem1>_<stem2>.npz`` {flow: flow12, coord_diff: coord_diff_1} and ``<stem2>_<stem1>.npz`` {flow: flow21,
    coord_diff: coord_diff_2} into ``flow_dir`` (compute_flow.py:351-358), the files ``datasets._common.read_flow_npz``
    reads, and with ``flow_png`` the colour-wheel pictures ``<stem1>_<stem2>.png`` and ``<stem2>_<stem1>.png`` beside them
    (:354-361) through ``writer``, a ``png.PngWriter`` that stays open for its owner; without one, a writer of at most
    MAX_PNG_THREADS threads is made here and closed before returning.  With ``device`` the flows (arrays, or tensors that
    may already be there) go through ``ops.flow_pair_export`` and come to the host once.  Returns the two ``.npz`` paths."""
    flow_dir = pathlib.Path(flow_dir)
    paths = (flow_dir / f"{stem1}_{stem2}.npz", flow_dir / f"{stem2}_{stem1}.npz")
    own = None
    if flow_png and writer is None:
        from ..png import PngWriter

        writer = own = PngWriter(n_threads=2)
    try:
        if device is None:
            flow12, flow21 = (f.detach().cpu().numpy() if hasattr(f, "detach") else f for f in (flow12, flow21))
            f12, f21 = _hw2(flow12, "flow12"), _hw2(flow21, "flow21")
            cd1, cd2 = flow_consistency(f12, f21)
            lines = None
            if flow_png:
                from ..png import filter_scanlines

                lines = [filter_scanlines(flow_to_image(f)) for f in (f12, f21)]
        else:
            from .. import ops

            t12, t21 = _on_device(flow12, "flow12", device), _on_device(flow21, "flow21", device)
            if t12.shape != t21.shape:
                raise ValueError(f"write_flow_pair: flow12 {tuple(t12.shape)} and flow21 {tuple(t21.shape)} differ")
            lines = None
            if flow_png:
                cd1, cd2, _, lines = ops.flow_pair_export(t12, t21, adaptive=True)
            else:
                cd1, cd2 = ops.flow_consistency(t12, t21)
            if lines is not None:  # (the writer's copy stream takes the scanlines while the arrays below come over)
                for path, ln in zip(paths, lines):
                    writer.submit(path.with_suffix(".png"), ln)
                lines = None
            f12 = flow12 if isinstance(flow12, np.ndarray) and flow12.dtype == np.float32 else t12.cpu().numpy()
            f21 = flow21 if isinstance(flow21, np.ndarray) and flow21.dtype == np.float32 else t21.cpu().numpy()
            cd1, cd2 = cd1.cpu().numpy(), cd2.cpu().numpy()
        if lines is not None:
            for path, ln in zip(paths, lines):
                writer.submit(path.with_suffix(".png"), ln)
        np.savez(paths[0], flow=f12, coord_diff=cd1)
        np.savez(paths[1], flow=f21, coord_diff=cd2)
    finally:
        if own is not None:
            own.close()
    return paths


def list_images(input_dir):
    """every file of ``input_dir`` with an extension PIL can open, sorted (DiffFlowDataset, compute_flow.py:38-47)"""
    exts = PIL.Image.registered_extensions()
    found = []
    for ext in {ex for ex, f in exts.items() if f in PIL.Image.OPEN}:
        found += list(pathlib.Path(input_dir).glob(f"*{ext}"))
    return sorted(found)


def _model_flow(flow, name, device=None):
    """the model's [1,2,H,W] (a tensor on any device, or an array) -> float32 [H,W,2]: numpy, or with ``device`` a GPU
    tensor left where it is, permuted there"""
    if hasattr(flow, "detach") and device is not None and flow.is_cuda:
        if flow.ndim != 4 or flow.shape[0] != 1 or flow.shape[1] != 2:
            raise ValueError(f"run_flow: the model's {name} must be [1,2,H,W], got {tuple(flow.shape)}")
        return flow.detach()[0].permute(1, 2, 0).float().contiguous()
    if hasattr(flow, "detach"):
        flow = flow.detach().cpu().numpy()
    flow = np.asarray(flow, dtype=np.float32)
    if flow.ndim != 4 or flow.shape[0] != 1 or flow.shape[1] != 2:
        raise ValueError(f"run_flow: the model's {name} must be [1,2,H,W], got {flow.shape}")
    return np.ascontiguousarray(flow[0].transpose(1, 2, 0))


def run_flow(input_dir, out_dir, model, img_pair_max_diff=3, device=None, flow_png=False, writer=None):
    """Writes upstream's flow tree (compute_flow.py:274-361 run): ``out_dir/interval_<k>/`` for k = 1..img_pair_max_diff,
    in it both ``.npz`` of every pair (i, i + k) of the sorted images of ``input_dir`` and, with ``flow_png``, both
    colour-wheel ``.png`` beside them.  ``model(img_f1, img_f2)`` takes the two image paths and returns (flow12, flow21),
    each [1,2,H,W]; with ``device``, tensors it returns on the GPU stay there until the pair's arrays come to the host once.
    ``writer``: the ``png.PngWriter`` for the pictures, left open for its owner; without one, a writer of at most
    MAX_PNG_THREADS threads lives for this call.  The debug collage is not written.  Returns the ``.npz`` paths written, in
    order."""
    if model is None:
        raise RuntimeError("run_flow needs an optical-flow model (model(img_f1, img_f2) -> (flow12, flow21)); none is given")
    images = list_images(input_dir)
    written = []
    own = None
    if flow_png and writer is None:
        from ..png import PngWriter

        writer = own = PngWriter(n_threads=MAX_PNG_THREADS)
    try:
        for k in range(1, int(img_pair_max_diff) + 1):
            flow_dir = pathlib.Path(out_dir) / f"interval_{k}"
            flow_dir.mkdir(parents=True, exist_ok=True)
            for i in range(0, len(images) - k):
                fn1, fn2 = images[i], images[i + k]
                flow12, flow21 = model(fn1, fn2)
                written += write_flow_pair(flow_dir, fn1.stem, fn2.stem, _model_flow(flow12, "flow12", device),
                                           _model_flow(flow21, "flow21", device), device=device, flow_png=flow_png, writer=writer)
    finally:
        if own is not None:
            own.close()
    return written
