"""torch-tensor front end of the C ABI (include/pgdvs_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
function below only validates tensors, allocates outputs / scratch with
``torch.empty`` and enqueues hand-written HIP kernels through ctypes.  Nothing in
this module computes on the CPU; CPU tensors are rejected.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import CAM_BLOCK, PgdvsHipError, check


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    # torch.cuda.current_stream() builds a Stream object through several Python layers (~8 us, 13
    # times per view); the raw handle of the current device's current stream is one C call
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise PgdvsHipError(
            f"{name}: tensor is on {t.device}; the MI355X path has no CPU fallback "
            "(move the data dict to the GPU as pgdvs.engines does)"
        )
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """2-D fp32 GPU tensor whose rows are contiguous (row stride arbitrary): views such as
    ``cloud[:, 3:]`` are passed to the kernels as (pointer, row stride) without a copy."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PgdvsHipError(f"{name}: expected a GPU tensor (no CPU fallback)")
    assert t.ndim == 2 and t.shape[1] >= 3, (name, t.shape)
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[0] > 0 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def _ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _ws(nbytes: int, device) -> torch.Tensor:
    if int(nbytes) < 0:  # the *_workspace_bytes entry points return a negative status for shapes they reject
        msg = _lib.load().pgdvs_last_error().decode("utf-8", "replace")
        raise PgdvsHipError(f"workspace query rejected the shape (status {int(nbytes)}): {msg}")
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _out(out, shape, dtype, device, what, *, at_least=None, flat=False, shown=None):
    """A caller's ``out=`` tensor after its check -- a contiguous ``dtype`` tensor of ``shape`` on the GPU ``device`` -- or a
    fresh one when ``out`` is None.  ``at_least``: the last dimension may be anything from ``at_least`` up (rows with room to
    spare).  ``flat``: only the element count has to be ``shape``'s.  The ValueError names the argument as ``what``
    ("op: out") and the shape as ``shown`` (by default ``shape`` itself, or its rows and ``at_least``)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    ok = isinstance(out, torch.Tensor) and out.is_cuda and out.device == device and out.dtype == dtype and out.is_contiguous()
    if ok and flat:
        ok = out.numel() == math.prod(shape)
    elif ok and at_least is not None:
        ok = out.ndim == len(shape) and out.shape[:-1] == shape[:-1] and out.shape[-1] >= at_least
    elif ok:
        ok = tuple(out.shape) == tuple(shape)
    if not ok:
        if shown is None:
            shown = f"tensor of {shape}" if at_least is None else f"tensor [{', '.join(str(s) for s in shape[:-1])}, >= {at_least}]"
        raise ValueError(f"{what} must be a contiguous {str(dtype).rpartition('.')[2]} {shown} on {device}")
    return out


def _planar_batch(img, what):
    """img [B,3,H,W] or [3,H,W] -> (the float32 contiguous GPU tensor [B,3,H,W], B, H, W)"""
    x = _req(img, torch.float32, "img")
    if x.ndim == 3:
        x = x[None]
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"{what}: img [B,3,H,W] expected, got {tuple(x.shape)}")
    return (x, int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))


# ---------------------------------------------------------------------------
def cam_prep(flat_cams: torch.Tensor) -> torch.Tensor:
    """flat_cams[..., 34] -> camera blocks[..., 80]."""
    fc = _req(flat_cams, torch.float32, "flat_cams")
    assert fc.shape[-1] == 34, fc.shape
    n = fc.numel() // 34
    out = torch.empty(fc.shape[:-1] + (CAM_BLOCK,), dtype=torch.float32, device=fc.device)
    check(_lib.load().pgdvs_cam_prep(_ptr(fc), n, _ptr(out), _stream()), "pgdvs_cam_prep")
    return out


def get_rays(cam_block: torch.Tensor, H: int, W: int, stride: int = 1):
    cam = _req(cam_block, torch.float32, "cam_block")
    rh, rw = (H + stride - 1) // stride, (W + stride - 1) // stride
    n = rh * rw
    ro = torch.empty((n, 3), dtype=torch.float32, device=cam.device)
    rd = torch.empty((n, 3), dtype=torch.float32, device=cam.device)
    uv = torch.empty((n, 2), dtype=torch.float32, device=cam.device)
    check(_lib.load().pgdvs_get_rays(_ptr(cam), H, W, stride, _ptr(ro), _ptr(rd), _ptr(uv), _stream()), "pgdvs_get_rays")
    return ro, rd, uv, (rh, rw)


def dyn_warp(dyn_mask1, occ, use_fc, flow12, depth1, depth2, rgb1, rgb2, cam1, cam2, times):
    H, W = dyn_mask1.shape[0], dyn_mask1.shape[1]
    dev = dyn_mask1.device
    m = _req(dyn_mask1, torch.float32, "dyn_mask1")
    o = _req(occ, torch.float32, "occ") if occ is not None else None
    args = [_req(t, torch.float32, n) for t, n in [
        (flow12, "flow12"), (depth1, "depth1"), (depth2, "depth2"), (rgb1, "rgb1"), (rgb2, "rgb2"),
        (cam1, "cam1"), (cam2, "cam2"), (times, "times")]]
    mask_eff = torch.empty((H, W), dtype=torch.uint8, device=dev)
    valid = torch.empty((H, W), dtype=torch.uint8, device=dev)
    pcl = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    rgbf = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    check(_lib.load().pgdvs_dyn_warp(
        H, W, _ptr(m), _ptr(o), int(bool(use_fc)), *[_ptr(a) for a in args],
        _ptr(mask_eff), _ptr(valid), _ptr(pcl), _ptr(rgbf), _stream()), "pgdvs_dyn_warp")
    return mask_eff, valid, pcl, rgbf


def compact_u8(flags: torch.Tensor):
    """-> (idx[int32, capacity n], count[int32, 1]) both on the device."""
    f = _req(flags, torch.uint8, "flags").reshape(-1)
    n = f.numel()
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=f.device)
    cnt = torch.empty(1, dtype=torch.int32, device=f.device)
    if n == 0:
        cnt.zero_()
        return idx, cnt
    lib = _lib.load()
    ws = _ws(lib.pgdvs_compact_workspace_bytes(n), f.device)
    check(lib.pgdvs_compact_u8(_ptr(f), n, _ptr(idx), _ptr(cnt), _ptr(ws), ws.numel(), _stream()), "pgdvs_compact_u8")
    return idx, cnt


def gather_rows(src: torch.Tensor, idx: torch.Tensor, cnt: torch.Tensor) -> torch.Tensor:
    s = _req(src, torch.float32, "src")
    width = s.shape[-1]
    cap = idx.numel()
    dst = torch.empty((cap, width), dtype=torch.float32, device=s.device)
    if s.shape[0] == 0:  # nothing to gather from (an empty tensor has no pointer to pass): the count is 0
        return dst
    check(_lib.load().pgdvs_gather_rows(_ptr(s), _ptr(idx), _ptr(cnt), cap, width, _ptr(dst), _stream()), "pgdvs_gather_rows")
    return dst


def knn_mean_dist(pts: torch.Tensor, cnt: torch.Tensor, K: int, algo: int = 0) -> torch.Tensor:
    """algo: 0 auto (grid when K+1 <= 64), 1 brute force, 2 grid."""
    p = _req(pts, torch.float32, "pts").reshape(-1, 3)
    c = _req(cnt, torch.int32, "count")
    out = torch.empty(max(p.shape[0], 1), dtype=torch.float32, device=p.device)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_knn_workspace_bytes(p.shape[0]), p.device)
    check(lib.pgdvs_knn_mean_dist(_ptr(p), _ptr(c), p.shape[0], int(K), _ptr(out), int(algo), _ptr(ws), ws.numel(),
                                  _stream()), "pgdvs_knn_mean_dist")
    return out


def outlier_flags(avg: torch.Tensor, cnt: torch.Tensor, std_thres: float, remove_outlier: bool):
    a = _req(avg, torch.float32, "avg")
    thres = torch.empty(1, dtype=torch.float32, device=a.device)
    flag = torch.empty(max(a.numel(), 1), dtype=torch.uint8, device=a.device)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_outlier_workspace_bytes(a.numel()), a.device)
    check(lib.pgdvs_outlier_flags(_ptr(a), _ptr(cnt), a.numel(), float(std_thres), int(bool(remove_outlier)),
                                  _ptr(thres), _ptr(flag), _ptr(ws), ws.numel(), _stream()), "pgdvs_outlier_flags")
    return thres, flag


def knn_cross_mean_dist(queries: torch.Tensor, qcnt: torch.Tensor, pts: torch.Tensor, cnt: torch.Tensor, KK: int) -> torch.Tensor:
    """mean of the KK smallest squared distances from each query to ``pts`` (all columns)."""
    q = _req(queries, torch.float32, "queries").reshape(-1, 3)
    p = _req(pts, torch.float32, "pts").reshape(-1, 3)
    out = torch.empty(max(q.shape[0], 1), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_knn_cross_workspace_bytes(p.shape[0], q.shape[0]), q.device)
    check(lib.pgdvs_knn_cross_mean_dist(_ptr(q), _ptr(_req(qcnt, torch.int32, "query_count")), q.shape[0], _ptr(p),
                                        _ptr(_req(cnt, torch.int32, "count")), p.shape[0], int(KK), _ptr(out), _ptr(ws),
                                        ws.numel(), _stream()), "pgdvs_knn_cross_mean_dist")
    return out


def threshold_flags(avg, cnt, thres, mult: float = 1.0, alt_thres=None, gate_count=None) -> torch.Tensor:
    a = _req(avg, torch.float32, "avg")
    flag = torch.empty(max(a.numel(), 1), dtype=torch.uint8, device=a.device)
    check(_lib.load().pgdvs_threshold_flags(_ptr(a), _ptr(cnt), a.numel(), _ptr(_req(thres, torch.float32, "thres")), float(mult),
                                            _ptr(alt_thres), _ptr(gate_count), _ptr(flag), _stream()), "pgdvs_threshold_flags")
    return flag


def concat_rows(a, cnt_a, b=None, cnt_b=None, require_a: bool = False):
    """[a[:cnt_a], b[:cnt_b]] with device-side counts -> (rows, count)."""
    a = _req(a, torch.float32, "a")
    assert a.ndim == 2
    nb = 0
    if b is not None:
        b = _req(b, torch.float32, "b")
        assert b.ndim == 2 and b.shape[1] == a.shape[1], (a.shape, b.shape)
        nb = b.shape[0]
    out = torch.empty((max(a.shape[0] + nb, 1), a.shape[1]), dtype=torch.float32, device=a.device)
    cnt = torch.empty(1, dtype=torch.int32, device=a.device)
    check(_lib.load().pgdvs_concat_rows(_ptr(a), _ptr(cnt_a), a.shape[0], _ptr(b), _ptr(cnt_b), nb, a.shape[1],
                                        int(bool(require_a)), _ptr(out), _ptr(cnt), _stream()), "pgdvs_concat_rows")
    return out, cnt


def track_points(tracks, visibles, frame_kind, times, time_tgt, rgbs, depths, cams):
    """A17 per-track validity, 3-D point at the target time and colour.
    tracks[P,N,2], visibles[P,N] bool, frame_kind: N host ints (1 closest / 2 track frame),
    times[N], time_tgt[1] (raw, device), rgbs[N,H,W,3], depths[N,H,W], cams[N,80]."""
    t = _req(tracks, torch.float32, "tracks")
    P, N = t.shape[0], t.shape[1]
    v = visibles
    if not v.is_cuda:
        raise PgdvsHipError("visibles: expected a GPU tensor (no CPU fallback)")
    v = v.contiguous().view(torch.uint8) if v.dtype == torch.bool else _req(v, torch.uint8, "visibles")
    rg = _req(rgbs, torch.float32, "rgbs")
    H, W = rg.shape[1], rg.shape[2]
    kind = (C.c_uint8 * N)(*[int(k) for k in frame_kind])
    valid = torch.empty(max(P, 1), dtype=torch.uint8, device=t.device)
    pcl = torch.empty((max(P, 1), 3), dtype=torch.float32, device=t.device)
    rgb = torch.empty((max(P, 1), 3), dtype=torch.float32, device=t.device)
    if P == 0:  # no track (empty tensors have no pointer to pass; the entry point launches nothing for P = 0)
        return valid[:0], pcl[:0], rgb[:0]
    check(_lib.load().pgdvs_track_points(_ptr(t), _ptr(v), P, N, C.cast(kind, C.c_void_p), _ptr(_req(times, torch.float32, "times")),
                                         _ptr(_req(time_tgt, torch.float32, "time_tgt")), _ptr(rg),
                                         _ptr(_req(depths, torch.float32, "depths")), H, W, _ptr(_req(cams, torch.float32, "cams")),
                                         _ptr(valid), _ptr(pcl), _ptr(rgb), _stream()), "pgdvs_track_points")
    return valid[:P], pcl[:P], rgb[:P]


def scatter_keep(idx, flag, cnt, P: int) -> torch.Tensor:
    keep = torch.empty(P, dtype=torch.uint8, device=idx.device)
    check(_lib.load().pgdvs_scatter_keep(_ptr(idx), _ptr(flag), _ptr(cnt), idx.numel(), _ptr(keep), P, _stream()), "pgdvs_scatter_keep")
    return keep


def project_flow_dense(cam_tgt, pcl, keep, H: int, W: int):
    cam = _req(cam_tgt, torch.float32, "cam_tgt")
    flow = torch.empty((2, H, W), dtype=torch.float32, device=cam.device)
    mask = torch.empty((H, W), dtype=torch.float32, device=cam.device)
    check(_lib.load().pgdvs_project_flow_dense(H, W, _ptr(cam), _ptr(_req(pcl, torch.float32, "pcl")),
                                               _ptr(_req(keep, torch.uint8, "keep")), _ptr(flow), _ptr(mask), _stream()),
          "pgdvs_project_flow_dense")
    return flow, mask


def project_points(cam_tgt, pts):
    p = _req(pts, torch.float32, "pts").reshape(-1, 3)
    uv = torch.empty((p.shape[0], 2), dtype=torch.float32, device=p.device)
    check(_lib.load().pgdvs_project_points(_ptr(_req(cam_tgt, torch.float32, "cam_tgt")), _ptr(p), p.shape[0], _ptr(uv), _stream()),
          "pgdvs_project_points")
    return uv


def backwarp_l1(rgb1, rgb2, flow):
    a, b, f = _req(rgb1, torch.float32, "rgb1"), _req(rgb2, torch.float32, "rgb2"), _req(flow, torch.float32, "flow")
    B, _, H, W = a.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=a.device)
    check(_lib.load().pgdvs_backwarp_l1(_ptr(a), _ptr(b), _ptr(f), _ptr(out), B, H, W, _stream()), "pgdvs_backwarp_l1")
    return out


_MODES = {"sum": 0, "avg": 1, "linear": 2, "soft": 3}
_EPS = {"addeps": 0, "zeroeps": 1, "clipeps": 2}


def softsplat_fwd(ten_in, ten_flow, ten_metric, mode: int, eps: int):
    x = _req(ten_in, torch.float32, "tenIn")
    f = _req(ten_flow, torch.float32, "tenFlow")
    m = _req(ten_metric, torch.float32, "tenMetric") if ten_metric is not None else None
    B, Cc, H, W = x.shape
    assert f.shape == (B, 2, H, W), f.shape
    out = torch.empty_like(x)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_softsplat_workspace_bytes(B, Cc, H, W, mode), x.device)
    check(lib.pgdvs_softsplat_fwd(_ptr(x), _ptr(f), _ptr(m), _ptr(out), B, Cc, H, W, mode, eps, _ptr(ws), ws.numel(), _stream()),
          "pgdvs_softsplat_fwd")
    return out


def softsplat_bwd(ten_in, ten_flow, grad_out, need_in: bool = True, need_flow: bool = True):
    """gradients of the raw ("sum") splat wrt input and flow."""
    i = _req(ten_in, torch.float32, "tenIn")
    f = _req(ten_flow, torch.float32, "tenFlow")
    g = _req(grad_out, torch.float32, "tenOutgrad")
    B, Cc, H, W = i.shape
    gi = torch.empty_like(i) if need_in else None
    gf = torch.empty_like(f) if need_flow else None
    check(_lib.load().pgdvs_softsplat_bwd(_ptr(i), _ptr(f), _ptr(g), _ptr(gi), _ptr(gf), B, Cc, H, W, _stream()),
          "pgdvs_softsplat_bwd")
    return gi, gf


def splat_rng_state(device, seed: int | None = None) -> torch.Tensor:
    """Device-resident state {seed, draw number} of the splat kernel's own noise (``dyn_splat_composite(rng_state=...)``);
    the seed defaults to torch's (``torch.initial_seed()``)."""
    s = torch.initial_seed() if seed is None else int(seed)
    return torch.tensor([s & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)


def splat_noise_field(rng_state, H: int, W: int) -> torch.Tensor:
    """[3,H,W]: the un-clamped normal field the NEXT ``dyn_splat_composite(rng_state=rng_state)`` call draws."""
    st = _req(rng_state, torch.int64, "rng_state")
    out = torch.empty((3, H, W), dtype=torch.float32, device=st.device)
    check(_lib.load().pgdvs_splat_noise_field(H, W, _ptr(st), _ptr(out), _stream()), "pgdvs_splat_noise_field")
    return out


def dyn_splat_composite(rgb1, rgb2, flow12, flow_1_to_tgt, valid_mask, noise, alpha, static_rgb, out_combined=None,
                        rng_state=None):
    """Returns planar (render_dyn_rgb[3,H,W], render_dyn_mask[H,W], combined, combined_static, combined_dyn).
    ``out_combined``: optional caller-owned contiguous [3,H,W] fp32 buffer the kernel writes the composite into
    (e.g. a slice of the caller's image stack: no copy afterwards).  ``noise`` [3,H,W]: the injected normal field
    (parity tests); ``noise=None`` with ``rng_state`` (``splat_rng_state``): the kernel draws it itself and advances
    the state; both None: zeros."""
    r1 = _req(rgb1, torch.float32, "rgb1")
    H, W = r1.shape[0], r1.shape[1]
    dev = r1.device
    dyn_rgb = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    dyn_mask = torch.empty((H, W), dtype=torch.float32, device=dev)
    st = _req(static_rgb, torch.float32, "static_rgb") if static_rgb is not None else None
    comb = None
    if st is not None:
        if out_combined is not None:
            if not (out_combined.is_cuda and out_combined.dtype == torch.float32 and out_combined.is_contiguous()
                    and tuple(out_combined.shape) == (3, H, W)):
                raise PgdvsHipError(f"out_combined: expected a contiguous fp32 GPU tensor [3,{H},{W}], got {tuple(out_combined.shape)}")
            two = torch.empty((2, 3, H, W), dtype=torch.float32, device=dev)
            comb = (out_combined, two[0], two[1])
        else:
            three = torch.empty((3, 3, H, W), dtype=torch.float32, device=dev)
            comb = (three[0], three[1], three[2])
    nz = _req(noise, torch.float32, "noise") if noise is not None else None
    lib = _lib.load()
    ws = _ws(lib.pgdvs_dyn_splat_workspace_bytes(H, W), dev)
    draw = nz is None and rng_state is not None
    fn = lib.pgdvs_dyn_splat_composite_rng if draw else lib.pgdvs_dyn_splat_composite
    check(fn(
        H, W, _ptr(r1), _ptr(_req(rgb2, torch.float32, "rgb2")), _ptr(_req(flow12, torch.float32, "flow12")),
        _ptr(_req(flow_1_to_tgt, torch.float32, "flow_1_to_tgt")), _ptr(_req(valid_mask, torch.float32, "valid_mask")),
        _ptr(_req(rng_state, torch.int64, "rng_state") if draw else nz), float(alpha), _ptr(st), _ptr(dyn_rgb), _ptr(dyn_mask),
        _ptr(comb[0] if comb is not None else None), _ptr(comb[1] if comb is not None else None),
        _ptr(comb[2] if comb is not None else None), _ptr(ws), ws.numel(), _stream()),
        "pgdvs_dyn_splat_composite_rng" if draw else "pgdvs_dyn_splat_composite")
    if comb is None:
        return dyn_rgb, dyn_mask, None, None, None
    return dyn_rgb, dyn_mask, comb[0], comb[1], comb[2]


def points_raster(pts, feat, cam_tgt, radius: float, K: int, H: int, W: int, *, n_points_dev=None,
                  want_fragments: bool = False, rgb_planar: bool = False, want_rgb: bool = True, row_bound: int | None = None):
    """pts[N,>=3] (xyz in the first 3 columns of each row), feat[N,>=3] rows.
    Returns dict(rgb, mask[, idx, zbuf, dist2]).  ``row_bound``: size the workspace for that many rows instead of N
    (capacity-sized cloud buffers with a device count: ``n_points_dev``); the dict then carries ``status`` (device
    int32[1]: 0 fine, 1 = the count exceeded the bound and rows were cut off, 2 = negative count; ``check_raster_status``)."""
    p = _rows(pts, "pts")
    n = p.shape[0]
    dev = p.device
    ft = _rows(feat, "feat") if feat is not None else None
    cam = _req(cam_tgt, torch.float32, "cam_tgt")
    idx = torch.empty((H, W, K), dtype=torch.int64, device=dev) if want_fragments else None
    zbuf = torch.empty((H, W, K), dtype=torch.float32, device=dev) if want_fragments else None
    d2 = torch.empty((H, W, K), dtype=torch.float32, device=dev) if want_fragments else None
    rgb = None
    if want_rgb and ft is not None:
        rgb = torch.empty((3, H, W) if rgb_planar else (H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.float32, device=dev)
    lib = _lib.load()
    if row_bound is None:
        ws = _ws(lib.pgdvs_points_raster_workspace_bytes(n, H, W, float(radius)), dev)
        check(lib.pgdvs_points_raster(
            _ptr(p), p.stride(0) if n else 3, _ptr(ft), ft.stride(0) if (ft is not None and n) else 3, n,
            _ptr(n_points_dev), _ptr(cam),
            float(radius), int(K), H, W, _ptr(idx), _ptr(zbuf), _ptr(d2), _ptr(rgb), int(bool(rgb_planar)), _ptr(mask),
            _ptr(ws), ws.numel(), _stream()), "pgdvs_points_raster")
        return {"rgb": rgb, "mask": mask, "idx": idx, "zbuf": zbuf, "dist2": d2}
    bound = max(0, min(int(row_bound), n))
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _ws(lib.pgdvs_points_raster_workspace_bytes(bound, H, W, float(radius)), dev)
    check(lib.pgdvs_points_raster_bounded(
        _ptr(p), p.stride(0) if n else 3, _ptr(ft), ft.stride(0) if (ft is not None and n) else 3, n,
        _ptr(n_points_dev), bound, _ptr(status), _ptr(cam),
        float(radius), int(K), H, W, _ptr(idx), _ptr(zbuf), _ptr(d2), _ptr(rgb), int(bool(rgb_planar)), _ptr(mask),
        _ptr(ws), ws.numel(), _stream()), "pgdvs_points_raster_bounded")
    return {"rgb": rgb, "mask": mask, "idx": idx, "zbuf": zbuf, "dist2": d2, "status": status}


def check_raster_status(status, what: str = "pgdvs_points_raster_bounded") -> None:
    """Host read of the bounded rasteriser's status word (synchronises): raises when rows were cut off."""
    if status is None:
        return
    for v in status.reshape(-1).tolist():
        if v == 1:
            raise PgdvsHipError(f"{what}: the device-side point count exceeds the row bound the workspace was sized for; "
                                "rows were cut off and the static image is not valid -- pass a larger bound")
        if v != 0:
            raise PgdvsHipError(f"{what}: the device-side point count is negative (the producer's error status); nothing was drawn")


def mesh_render(cam_tgt, keep, pcl, rgb, H: int, W: int, want_faces: bool = False):
    """A10 mesh variant -> dict(rgb[3,H,W], mask[H,W][, face[H,W] int32])."""
    cam = _req(cam_tgt, torch.float32, "cam_tgt")
    img = torch.empty((3, H, W), dtype=torch.float32, device=cam.device)
    mask = torch.empty((H, W), dtype=torch.float32, device=cam.device)
    face = torch.empty((H, W), dtype=torch.int32, device=cam.device) if want_faces else None
    lib = _lib.load()
    ws = _ws(lib.pgdvs_mesh_render_workspace_bytes(H, W), cam.device)
    check(lib.pgdvs_mesh_render(_ptr(cam), H, W, _ptr(_req(keep, torch.uint8, "keep")), _ptr(_req(pcl, torch.float32, "pcl")),
                                _ptr(_req(rgb, torch.float32, "rgb")), _ptr(img), _ptr(mask), _ptr(face), _ptr(ws), ws.numel(),
                                _stream()), "pgdvs_mesh_render")
    out = {"rgb": img, "mask": mask}
    if want_faces:
        out["face"] = face
    return out


def static_aggregate(rgbs, depths, dyn_masks, K3s, c2ws, capacity: int | None = None, return_xyz: bool = False):
    """rgbs[S,H,W,3] fp32 in [0,1]; depths[S,H,W]; dyn_masks[S,H,W] bool/uint8 (GPU tensors);
    K3s[S,3,3], c2ws[S,4,4] float64 numpy (host).  -> (cloud[capacity,6], count[int64 dev]) and, with
    ``return_xyz``, the packed coordinates [capacity,3] (``data["st_pcl_xyz"]`` for the renderer)."""
    r = _req(rgbs, torch.float32, "rgbs")
    d = _req(depths, torch.float32, "depths")
    m = _req(dyn_masks.contiguous().view(torch.uint8) if dyn_masks.dtype == torch.bool else dyn_masks, torch.uint8, "dyn_masks")
    S, H, W = d.shape
    K3 = np.ascontiguousarray(K3s, dtype=np.float64).reshape(S, 9)
    c2w = np.ascontiguousarray(c2ws, dtype=np.float64).reshape(S, 16)
    cap = int(capacity) if capacity is not None else S * H * W
    out = torch.empty((cap, 6), dtype=torch.float32, device=r.device)
    cnt = torch.empty(1, dtype=torch.int64, device=r.device)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_static_aggregate_workspace_bytes(S, H, W, cap), r.device)
    if return_xyz:
        xyz = torch.empty((cap, 3), dtype=torch.float32, device=r.device)
        check(lib.pgdvs_static_aggregate_packed(
            _ptr(r), _ptr(d), _ptr(m), K3.ctypes.data_as(C.c_void_p), c2w.ctypes.data_as(C.c_void_p), S, H, W,
            _ptr(out), _ptr(xyz), cap, _ptr(cnt), _ptr(ws), ws.numel(), _stream()), "pgdvs_static_aggregate_packed")
        return out, cnt, xyz
    check(lib.pgdvs_static_aggregate(
        _ptr(r), _ptr(d), _ptr(m), K3.ctypes.data_as(C.c_void_p), c2w.ctypes.data_as(C.c_void_p), S, H, W,
        _ptr(out), cap, _ptr(cnt), _ptr(ws), ws.numel(), _stream()), "pgdvs_static_aggregate")
    return out, cnt


class ViewGeoState:
    """What ``view_geo_forward`` keeps between calls for ONE HIP stream: the workspace of the native call (reused, so a
    view costs no allocator round trips beyond its outputs) and the description struct.  Views in flight on different
    streams need different states (``PGDVSRenderer`` keeps one per stream it is called on)."""

    def __init__(self):
        self.desc = _lib.ViewGeoDesc()
        self.workspace = None
        self.ws_key = None
        self.ws_bytes = 0
        self.agg_key = None  # (shape, cameras) whose per-frame constants the workspace holds
        self.default_side_stream = None  # PGDVSRenderer._forward_native: the dynamic branch's stream when the caller names none


def view_geo_forward(state: ViewGeoState, *, H: int, W: int, flat_cam_tgt, flat_cam_src, time_src, time_tgt, rgb1, rgb2, depth1,
                     depth2, dyn_mask1, flow12, flow_occ, use_flow_consistency: bool, remove_outlier: bool, outlier_knn: int,
                     outlier_std_thres: float, alpha: float, noise=None, rng_state=None, st_pcl_rgb=None, st_pcl_xyz=None,
                     st_count=None, video=None, row_bound=None, radius: float, K: int, out_combined=None, side_stream=None):
    """ONE native call for the whole geometric per-view path (``pgdvs_view_geo_forward``): A12 (when ``video`` is given)
    + A9 + A2-A5 + A6-A8 + A11.  All tensors fp32 contiguous on the GPU (checked; no conversions are made here -- the
    caller falls back to the per-op path for anything else).
    ``video``: dict(rgbs[S,H,W,3], depths[S,H,W], dyn_masks[S,H,W] u8, K3s, c2ws (float64 numpy), capacity) -- the cloud
    is aggregated inside the call and returned (``st_pcl_rgb``, ``st_pcl_xyz``, ``st_pcl_rgb_count``).
    Returns a dict of planar images (see the keys below)."""
    lib = _lib.load()
    d = state.desc
    dev = rgb1.device
    P = H * W

    def ptr(t, name, dtype=torch.float32, numel=None):
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise PgdvsHipError(f"view_geo_forward: {name} must be a contiguous {dtype} GPU tensor (got {t.dtype}, {t.device}, "
                                f"contiguous={t.is_contiguous()})")
        if numel is not None and t.numel() != numel:
            raise PgdvsHipError(f"view_geo_forward: {name} has {t.numel()} elements, expected {numel}")
        return t.data_ptr()

    d.H, d.W = H, W
    d.flat_cam_tgt = ptr(flat_cam_tgt, "flat_cam_tgt", numel=34)
    d.flat_cam_src = ptr(flat_cam_src, "flat_cam_src", numel=68)
    d.time_src = ptr(time_src, "time_src")
    d.time_tgt = ptr(time_tgt, "time_tgt")
    if time_src.numel() < 2 or time_tgt.numel() < 1:
        raise PgdvsHipError("view_geo_forward: time_src needs 2 entries, time_tgt 1")
    d.rgb1, d.rgb2 = ptr(rgb1, "rgb1", numel=3 * P), ptr(rgb2, "rgb2", numel=3 * P)
    d.depth1, d.depth2 = ptr(depth1, "depth1", numel=P), ptr(depth2, "depth2", numel=P)
    d.dyn_mask1 = ptr(dyn_mask1, "dyn_mask1", numel=P)
    d.flow12 = ptr(flow12, "flow12", numel=2 * P)
    d.flow_occ = ptr(flow_occ, "flow_occ", numel=P)
    d.use_flow_consistency, d.remove_outlier, d.outlier_knn = int(bool(use_flow_consistency)), int(bool(remove_outlier)), int(outlier_knn)
    d.outlier_std_thres, d.alpha = float(outlier_std_thres), float(alpha)
    d.noise = ptr(noise, "noise", numel=3 * P)
    d.rng_state = ptr(rng_state, "rng_state", torch.int64, 2) if noise is None else None
    out = {}
    keep_alive = None
    if video is not None:
        r, dp, m = video["rgbs"], video["depths"], video["dyn_masks"]
        S = dp.shape[0]
        cap = int(video.get("capacity") or S * P)
        K3 = np.ascontiguousarray(video["K3s"], dtype=np.float64).reshape(S, 9)
        c2w = np.ascontiguousarray(video["c2ws"], dtype=np.float64).reshape(S, 16)
        keep_alive = (K3, c2w)
        block = torch.empty(cap * 9, dtype=torch.float32, device=dev)  # cloud rows and packed coordinates in one block
        cloud, xyz = block[: cap * 6].view(cap, 6), block[cap * 6:].view(cap, 3)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        d.agg_S = S
        d.agg_rgbs, d.agg_depths = ptr(r, "video.rgbs", numel=S * P * 3), ptr(dp, "video.depths", numel=S * P)
        d.agg_masks = ptr(m, "video.dyn_masks", torch.uint8, S * P)
        d.agg_K3s_host, d.agg_c2ws_host = K3.ctypes.data, c2w.ctypes.data
        d.agg_cloud_out, d.agg_xyz_out, d.agg_capacity, d.agg_count_out = cloud.data_ptr(), xyz.data_ptr(), cap, cnt.data_ptr()
        d.st_pcl_rgb = d.st_pcl_xyz = d.st_count_dev = None
        d.st_rows = 0
        rows = cap
        out.update(st_pcl_rgb=cloud, st_pcl_xyz=xyz, st_pcl_rgb_count=cnt)
        agg_key = (S, H, W, cap, K3.tobytes(), c2w.tobytes())
    else:
        agg_key = None
        d.agg_S = 0
        rows = st_pcl_rgb.shape[0]
        d.st_pcl_rgb = ptr(st_pcl_rgb, "st_pcl_rgb", numel=rows * 6) if rows else None
        d.st_pcl_xyz = ptr(st_pcl_xyz, "st_pcl_xyz", numel=rows * 3) if (st_pcl_xyz is not None and rows) else None
        d.st_rows = rows
        d.st_count_dev = ptr(st_count, "st_pcl_rgb_count", torch.int64, 1)
    d.row_bound = int(row_bound) if (row_bound is not None and (video is not None or st_count is not None)) else 0
    d.radius, d.K = float(radius), int(K)
    # outputs: one block for the images, one for the masks
    n_img = 4 if out_combined is not None else 5
    imgs = torch.empty((n_img, 3, H, W), dtype=torch.float32, device=dev)
    masks = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    if out_combined is not None:
        if not (out_combined.is_cuda and out_combined.dtype == torch.float32 and out_combined.is_contiguous()
                and out_combined.numel() == 3 * P):
            raise PgdvsHipError(f"out_combined: expected a contiguous fp32 GPU tensor [3,{H},{W}], got {tuple(out_combined.shape)}")
        comb = out_combined.view(3, H, W)
    else:
        comb = imgs[4]
    d.static_rgb, d.render_dyn_rgb, d.combined_static, d.combined_dyn = (imgs[i].data_ptr() for i in range(4))
    d.combined = comb.data_ptr()
    d.static_mask, d.render_dyn_mask = masks[0].data_ptr(), masks[1].data_ptr()
    d.raster_status = status.data_ptr()
    d.side_stream = side_stream.cuda_stream if side_stream is not None else None
    # workspace: reused while the shape of the problem stays the same
    key = (H, W, d.agg_S, int(d.agg_capacity) if d.agg_S else rows, int(d.row_bound), d.radius, d.remove_outlier, dev)
    if state.ws_key != key:
        need = lib.pgdvs_view_geo_workspace_bytes(C.byref(d))
        if need < 0:
            check(int(need), "pgdvs_view_geo_workspace_bytes")
        if state.workspace is None or state.ws_bytes < need or state.workspace.device != dev:
            state.workspace = None  # (release first: two of these do not have to coexist)
            state.workspace = torch.empty(int(need), dtype=torch.uint8, device=dev)
            state.ws_bytes = int(need)
        state.ws_key = key
        state.agg_key = None  # (another layout, or a fresh block: nothing is cached in it)
    # the camera constants of the aggregation stay in the workspace between calls with the same video
    d.agg_params_cached = int(agg_key is not None and agg_key == state.agg_key)
    state.agg_key = None  # (until the call has gone through)
    check(lib.pgdvs_view_geo_forward(C.byref(d), state.workspace.data_ptr(), state.ws_bytes, _stream()), "pgdvs_view_geo_forward")
    del keep_alive
    state.agg_key = agg_key
    out.update(geo_static_rgb=imgs[0], geo_static_mask=masks[0], render_dyn_rgb=imgs[1], render_dyn_mask=masks[1],
               combined_rgb=comb, combined_rgb_static=imgs[2], combined_rgb_dyn=imgs[3], raster_status=status)
    return out


VIEW_COUNTER_NAMES = ("static_rows", "raster_list_entries", "raster_longest_tile_list", "raster_tiles_general_path_long_list",
                      "raster_tiles_general_path_equal_depths", "knn_queries", "knn_queries_to_ring_search",
                      "knn_queries_to_coarse_grid", "knn_queries_scanned_exhaustively", "agg_points_in_fp64_queue",
                      "agg_projections_in_reference_order")


def view_geo_counters(state: ViewGeoState) -> dict:
    """What the fast paths of the last ``view_geo_forward`` on ``state`` left to their slower exits
    (``pgdvs_view_geo_counters``; enqueued on the current stream, which must be the one the view ran on; synchronises)."""
    if state.workspace is None:
        raise PgdvsHipError("view_geo_counters: no view has been rendered with this state")
    out = torch.empty(12, dtype=torch.int64, device=state.workspace.device)
    check(_lib.load().pgdvs_view_geo_counters(C.byref(state.desc), state.workspace.data_ptr(), state.ws_bytes, out.data_ptr(), _stream()),
          "pgdvs_view_geo_counters")
    vals = out.tolist()
    return {k: int(vals[i]) for i, k in enumerate(VIEW_COUNTER_NAMES)}


def view_geo_host_stats():
    """(calls, seconds) spent inside ``pgdvs_view_geo_forward`` since the last call of this function (resets)."""
    calls, secs = C.c_int64(0), C.c_double(0.0)
    _lib.load().pgdvs_view_geo_host_stats(C.byref(calls), C.byref(secs))
    return int(calls.value), float(secs.value)


def _images(pred_planar, gt_hwc, mask_hwc=None):
    """pred[3,H,W] and gt[H,W,3] -- and, given, mask[H,W,3] -- of a metric-row call as float32 GPU tensors -> p, g, m, H, W"""
    p = _req(pred_planar, torch.float32, "pred")
    g = _req(gt_hwc, torch.float32, "gt")
    m = _req(mask_hwc, torch.float32, "eval_mask") if mask_hwc is not None else None
    _, H, W = p.shape
    assert tuple(g.shape) == (H, W, 3) and (m is None or tuple(m.shape) == (H, W, 3)), (p.shape, g.shape, getattr(m, "shape", None))
    return p, g, m, H, W


def _min_size(what: str, H: int, W: int, n: int, limit: str) -> None:
    if H < n or W < n:
        raise ValueError(f"{what}: the image ({H} x {W}) is smaller than {limit}")


def _lpips_weights(weights, device):
    """the three packed buffers of a ``harness.LpipsAlex`` (on ``device``) as the C ABI takes them"""
    cw, cb, lw = (_req(t, torch.float32, n) for t, n in ((weights.conv_weights, "conv_weights"), (weights.conv_biases, "conv_biases"),
                                                         (weights.lin_weights, "lin_weights")))
    assert cw.device == device, (cw.device, device)
    return cw, cb, lw


def _metric_row(name: str, nbytes: int, device, *args):
    """The common tail of the metric-row entry points, which all end in (sums, workspace, workspace_bytes, stream): the
    workspace query's answer ``nbytes`` (negative: raises with the library's message) rounded up to 64 bytes, ONE buffer
    holding the workspace and then the eight doubles, and the call ``name(*args, ...)`` -> (the row float64[8], the buffer)."""
    nws = int(nbytes)
    if nws < 0:
        _ws(nws, device)  # raises with the library's message
    nws = (nws + 63) // 64 * 64
    buf = torch.empty(nws + 64, dtype=torch.uint8, device=device)
    sums = buf[nws:nws + 64].view(torch.float64)
    check(getattr(_lib.load(), name)(*args, _ptr(sums), _ptr(buf), nws, _stream()), name)
    return sums, buf


def eval_psnr_sums(pred_planar, gt_hwc, mask_hwc, want_images: bool = False, count_dev=None, status_dev=None):
    """The evaluator's per-view statistics in one pass (``pgdvs_eval_psnr_sums``): pred[3,H,W] raw render, gt[H,W,3] raw,
    mask[H,W,3] -> device float64[8] (sum d2, sum d2 m, sum d2 (1-m), count, sum m, sum (1-m), then ``count_dev`` -- int64[1],
    -1 when None -- and ``status_dev`` -- int32[1], 0 when None -- as doubles, so that one transfer brings everything back)
    and, with ``want_images``, the quantised prediction / ground truth [3,H,W]."""
    p, g, m, H, W = _images(pred_planar, gt_hwc, mask_hwc)
    pq = torch.empty_like(p) if want_images else None
    gq = torch.empty_like(p) if want_images else None
    cd = _req(count_dev, torch.int64, "count_dev") if count_dev is not None else None
    sd = _req(status_dev, torch.int32, "status_dev") if status_dev is not None else None
    sums, _ = _metric_row("pgdvs_eval_psnr_sums", _lib.load().pgdvs_eval_psnr_workspace_bytes(), p.device,
                          _ptr(p), _ptr(g), _ptr(m), H, W, _ptr(pq), _ptr(gq), _ptr(cd), _ptr(sd))
    return sums, pq, gq


def eval_ssim_sums(pred_planar, gt_hwc, mask_hwc, want_map: bool = False):
    """The evaluator's masked SSIM statistics in one pass (``pgdvs_eval_ssim_sums``): pred[3,H,W] raw render, gt[H,W,3] raw,
    mask[H,W,3] -> device float64[8] (sum S, sum S m, sum S (1-m), count, sum m, sum (1-m), 0, 0 -- the layout of
    ``eval_psnr_sums``' row, so that ``read_back_rows`` brings both back in one transfer) and, with ``want_map``, the SSIM map
    S[3,H,W].  Raises ValueError when H or W is below the 7x7 window, as skimage does."""
    p, g, m, H, W = _images(pred_planar, gt_hwc, mask_hwc)
    _min_size("eval_ssim_sums", H, W, 7, "SSIM's 7 x 7 window")
    smap = torch.empty_like(p) if want_map else None
    sums, _ = _metric_row("pgdvs_eval_ssim_sums", _lib.load().pgdvs_eval_ssim_workspace_bytes(H, W), p.device,
                          _ptr(p), _ptr(g), _ptr(m), H, W, _ptr(smap))
    return sums, smap


LPIPS_CHANNELS = (64, 192, 384, 256, 256)  # AlexNet relu1..relu5
LPIPS_MIN_SIZE = 31  # conv1 11x11/4 pad 2, then two 3/2 pools: relu5 is empty below this
_LPIPS_LIMIT = "AlexNet's 31 x 31 minimum (relu5 would be empty)"


def lpips_map_sizes(H: int, W: int):
    """[(h, w)] of relu1..relu5 and [(h, w)] of pool1, pool2 for an H x W image (the backbone's shape rule)."""
    conv1 = ((H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1)
    pool1 = ((conv1[0] - 3) // 2 + 1, (conv1[1] - 3) // 2 + 1)
    pool2 = ((pool1[0] - 3) // 2 + 1, (pool1[1] - 3) // 2 + 1)
    return [conv1, pool1, pool2, pool2, pool2], [pool1, pool2]


def _lpips_features(buf, H, W):
    """relu1..relu5 as [2,C,h,w] views of the workspace (include/pgdvs_hip.h: x, relu1, pool1, relu2, pool2, relu3, relu4,
    relu5, each region rounded up to 256 bytes)"""
    relu, pool = lpips_map_sizes(H, W)
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    off = a256(2 * 3 * H * W * 4)
    out = []
    for k, (C, (h, w)) in enumerate(zip(LPIPS_CHANNELS, relu)):
        n = 2 * C * h * w
        out.append(buf[off:off + 4 * n].view(torch.float32).view(2, C, h, w))
        off += a256(4 * n)
        if k < 2:
            off += a256(4 * 2 * C * pool[k][0] * pool[k][1])
    return out


def lpips_sums(pred_planar, gt_hwc, mask_hwc, weights, want_features: bool = False):
    """The evaluator's masked LPIPS of one view (``pgdvs_lpips_sums``): pred[3,H,W] raw render, gt[H,W,3] raw, mask[H,W,3]
    (channel 0 used), ``weights`` a ``harness.LpipsAlex`` on the same device -> device float64[8] (LPIPS full, dyn, static,
    then the relu1 map's pixel count, sum m, sum (1 - m), 0, 0 -- the width of ``eval_psnr_sums``' row, so that
    ``read_back_rows`` brings them all back in one transfer) and, with ``want_features``, relu1..relu5 of both images as
    [2,C,h,w] (ground truth first; views of the call's workspace).  Raises ValueError when H or W is below 31 (the relu5 map
    would be empty)."""
    p, g, m, H, W = _images(pred_planar, gt_hwc, mask_hwc)
    _min_size("lpips_sums", H, W, LPIPS_MIN_SIZE, _LPIPS_LIMIT)
    cw, cb, lw = _lpips_weights(weights, p.device)
    sums, buf = _metric_row("pgdvs_lpips_sums", _lib.load().pgdvs_lpips_workspace_bytes(H, W), p.device,
                            _ptr(p), _ptr(g), _ptr(m), H, W, _ptr(cw), _ptr(cb), _ptr(lw))
    return sums, (_lpips_features(buf, H, W) if want_features else None)


def _dycheck_mask(mask, H, W, what):
    """eval_mask of the DyCheck protocol, [H,W,1] (or [H,W]) -> a contiguous [H,W] float32 tensor"""
    m = mask[..., 0] if mask.ndim == 3 else mask
    if tuple(m.shape) != (H, W) or (mask.ndim == 3 and mask.shape[-1] != 1):
        raise ValueError(f"{what}: eval_mask must be [H,W,1] (got {tuple(mask.shape)} for a {H} x {W} image)")
    return _req(m.contiguous(), torch.float32, "eval_mask")


DYCHECK_SSIM_MIN_SIZE = 11  # the 11-tap window in "valid" mode: the map is (H - 10) x (W - 10)


def dycheck_psnr_ssim_sums(pred_planar, gt_hwc, mask_hw1, count_dev=None, status_dev=None):
    """The DyCheck iPhone protocol's PSNR and SSIM of one view, full and covisible, in one pass
    (``pgdvs_dycheck_psnr_ssim_sums``): pred[3,H,W] raw render, gt[H,W,3] raw, mask[H,W,1] -> device float64[8] (sum d2,
    sum d2 m, sum S full, 3HW, 3 sum m, sum S covisible, then ``count_dev`` -- -1 when None -- and ``status_dev`` -- 0 when
    None -- as in ``eval_psnr_sums``' row, so that ``read_back_rows`` brings it back with the others; include/pgdvs_hip.h).
    Raises ValueError when H or W is below the 11-tap window."""
    p, g, _, H, W = _images(pred_planar, gt_hwc)
    m = _dycheck_mask(mask_hw1, H, W, "dycheck_psnr_ssim_sums")
    _min_size("dycheck_psnr_ssim_sums", H, W, DYCHECK_SSIM_MIN_SIZE, "SSIM's 11 x 11 window")
    cd = _req(count_dev, torch.int64, "count_dev") if count_dev is not None else None
    sd = _req(status_dev, torch.int32, "status_dev") if status_dev is not None else None
    return _metric_row("pgdvs_dycheck_psnr_ssim_sums", _lib.load().pgdvs_dycheck_psnr_ssim_workspace_bytes(H, W), p.device,
                       _ptr(p), _ptr(g), _ptr(m), H, W, _ptr(cd), _ptr(sd))[0]


def dycheck_lpips(pred_planar, gt_hwc, mask_hw1, weights):
    """The DyCheck iPhone protocol's LPIPS of one view, full and covisible (``pgdvs_dycheck_lpips``): pred[3,H,W] raw render,
    gt[H,W,3] raw, mask[H,W,1], ``weights`` a ``harness.LpipsAlex`` on the same device -> device float64[8] (LPIPS full,
    LPIPS covisible, sum v, HW, sum v m, sum m, 0, 0; include/pgdvs_hip.h).  Raises ValueError when H or W is below 31."""
    p, g, _, H, W = _images(pred_planar, gt_hwc)
    m = _dycheck_mask(mask_hw1, H, W, "dycheck_lpips")
    _min_size("dycheck_lpips", H, W, LPIPS_MIN_SIZE, _LPIPS_LIMIT)
    cw, cb, lw = _lpips_weights(weights, p.device)
    return _metric_row("pgdvs_dycheck_lpips", _lib.load().pgdvs_dycheck_lpips_workspace_bytes(H, W), p.device,
                       _ptr(p), _ptr(g), _ptr(m), H, W, _ptr(cw), _ptr(cb), _ptr(lw))[0]


def _mat64(a, n: int):
    """``a`` as a contiguous float64 ``c_double * n`` array (host matrices travel by value)."""
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float64).reshape(-1)
    assert a.size == n, a.shape
    return (C.c_double * n)(*a.tolist())


def _out64(t):
    """The depth-range ops' optional output, a contiguous device float64 tensor of at least two elements: its pointer or None."""
    assert t is None or (t.is_cuda and t.dtype == torch.float64 and t.numel() >= 2 and t.is_contiguous())
    return _ptr(t)


def dycheck_depth_range(depth, dyn_mask, rays, inv_raw_c2w_tgt, inv_c2w_tgt, K_tgt, near, far, quantiles=None):
    """The DyCheck loader's per-pixel depth range (``pgdvs_dycheck_depth_range``; include/pgdvs_hip.h): depth[V,H,W] float32
    or float64 and dyn_mask[V,H,W] on the GPU, rays[V,12] float32 on the GPU (per view ``M`` row-major and the origin, as
    ``datasets.dycheck_iphone.ray_constants`` forms them), the target's numpy float32 inverses ``inv_raw_c2w_tgt[4,4]`` and
    ``inv_c2w_tgt[4,4]`` and ``K_tgt[3,3]``, the scene's ``near`` / ``far`` -> depth_range[H,W,2] float32 on the GPU,
    bit-identical to ``depth_range_numpy``.  ``quantiles``: optional device float64[2] that receives np.quantile(z, 0.1 / 0.9)."""
    if depth.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dycheck_depth_range: depth must be float32 or float64, got {depth.dtype}")
    d = _req(depth, depth.dtype, "depth")
    m = _req(dyn_mask, torch.float32, "dyn_mask")
    r = _req(rays, torch.float32, "rays")
    if d.ndim != 3 or tuple(m.shape) != tuple(d.shape) or tuple(r.shape) != (d.shape[0], 12):
        raise ValueError(f"dycheck_depth_range: shapes depth {tuple(d.shape)}, dyn_mask {tuple(m.shape)}, rays {tuple(r.shape)}")
    V, H, W = (int(x) for x in d.shape)
    f64 = int(d.dtype == torch.float64)
    mats = [_mat64(inv_raw_c2w_tgt, 16), _mat64(inv_c2w_tgt, 16), _mat64(K_tgt, 9)]
    lib = _lib.load()
    ws = _ws(lib.pgdvs_dycheck_depth_range_workspace_bytes(V, H, W, f64), d.device)
    out = torch.empty((H, W, 2), dtype=torch.float32, device=d.device)
    check(lib.pgdvs_dycheck_depth_range(_ptr(d), f64, _ptr(m), _ptr(r), V, H, W, mats[0], mats[1], mats[2], float(near), float(far),
                                        _ptr(out), _out64(quantiles), _ptr(ws), ws.numel(), _stream()), "pgdvs_dycheck_depth_range")
    return out


def nvidia_depth_range(depth, rays, inv_c2w_tgt, near_far=None):
    """The NVIDIA-family loaders' per-item depth range (``pgdvs_nvidia_depth_range``; include/pgdvs_hip.h): depth[V,H,W]
    float32 on the GPU, rays[V,12] float32 on the GPU (per view ``M`` row-major and the origin, as
    ``datasets.nvidia_eval.ray_constants`` forms them), the target's numpy float64 ``inv_c2w_tgt[4,4]`` -> depth_range[2]
    float32 on the GPU = (max(1e-16, 0.8 min z), max(2e-16, 1.2 np.quantile(z, 0.9))), bit-identical to
    ``depth_range_from_points`` over the views' ``compute_pcl``.  ``near_far``: optional device float64[2] that receives the
    float64 pair before the cast.  One-pixel views (H W == 1) are rejected."""
    d = _req(depth, torch.float32, "depth")
    r = _req(rays, torch.float32, "rays")
    if d.ndim != 3 or tuple(r.shape) != (d.shape[0], 12):
        raise ValueError(f"nvidia_depth_range: shapes depth {tuple(d.shape)}, rays {tuple(r.shape)}")
    V, H, W = (int(x) for x in d.shape)
    mat = _mat64(inv_c2w_tgt, 16)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_nvidia_depth_range_workspace_bytes(V, H, W), d.device)
    out = torch.empty((2,), dtype=torch.float32, device=d.device)
    check(lib.pgdvs_nvidia_depth_range(_ptr(d), _ptr(r), V, H, W, mat, _ptr(out), _out64(near_far), _ptr(ws), ws.numel(),
                                       _stream()), "pgdvs_nvidia_depth_range")
    return out


def nvidia_zoe_depth(depth_pred, scale_shift, rays=None, inv_c2w_tgt=None, near_far=None):
    """The NVIDIA evaluation loader's ZoeDepth alignment (``pgdvs_nvidia_zoe_depth_range``; include/pgdvs_hip.h):
    depth_pred[V,H,W] float32 on the GPU and the numpy float64 ``scale_shift[V,2]`` (scale, shift per view) -> depth[V,H,W]
    float32 on the GPU, bit-identical to ``datasets.nvidia_eval.zoe_align`` rounded to float32.  With ``rays[V,12]`` (float32
    on the GPU, as in ``nvidia_depth_range``) and the target's float64 ``inv_c2w_tgt[4,4]`` it returns (depth, depth_range[2])
    from the same pass, the range over the cloud unprojected with the float64 depth; ``near_far``: optional device float64[2]
    for the pair before the cast.  One-pixel views are rejected on the range path only."""
    d = _req(depth_pred, torch.float32, "depth_pred")
    if d.ndim != 3:
        raise ValueError(f"nvidia_zoe_depth: depth_pred [V,H,W] expected, got {tuple(d.shape)}")
    V, H, W = (int(x) for x in d.shape)
    ss = np.ascontiguousarray(np.asarray(scale_shift), dtype=np.float64)
    if ss.shape != (V, 2):
        raise ValueError(f"nvidia_zoe_depth: scale_shift {ss.shape}, expected {(V, 2)}")
    if (rays is None) != (inv_c2w_tgt is None) or (near_far is not None and rays is None):
        raise ValueError("nvidia_zoe_depth: rays and inv_c2w_tgt go together, near_far only with them")
    ssv = _mat64(ss, 2 * V) if V else None
    lib = _lib.load()
    out = torch.empty((V, H, W), dtype=torch.float32, device=d.device)
    if rays is None:
        check(lib.pgdvs_nvidia_zoe_depth_range(_ptr(d), ssv, None, V, H, W, None, _ptr(out), None, None, None, 0, _stream()),
              "pgdvs_nvidia_zoe_depth_range")
        return out
    r = _req(rays, torch.float32, "rays")
    if tuple(r.shape) != (V, 12):
        raise ValueError(f"nvidia_zoe_depth: shapes depth_pred {tuple(d.shape)}, rays {tuple(r.shape)}")
    mat = _mat64(inv_c2w_tgt, 16)
    ws = _ws(lib.pgdvs_nvidia_zoe_depth_range_workspace_bytes(V, H, W), d.device)
    rng = torch.empty((2,), dtype=torch.float32, device=d.device)
    check(lib.pgdvs_nvidia_zoe_depth_range(_ptr(d), ssv, _ptr(r), V, H, W, mat, _ptr(out), _ptr(rng), _out64(near_far), _ptr(ws),
                                           ws.numel(), _stream()), "pgdvs_nvidia_zoe_depth_range")
    return out, rng


ITEM_MAX_VIEWS, ITEM_MAX_GROUPS = 64, 4
ITEM_VIEW_KEYS = ("rgb", "dyn_mask", "dyn_rgb", "static_rgb", "depth")


def _store_table(t, dtype, shape, name):
    """a table of the resident store: frames [F, *shape] of ``dtype`` on the GPU, each frame contiguous, the base and (for
    F > 1) the frame stride multiples of 16 bytes -> (tensor, frame stride in bytes)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PgdvsHipError(f"{name}: expected a GPU tensor (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape[1:]) != tuple(shape) or t.ndim != len(shape) + 1:
        raise ValueError(f"item_views: {name} {t.dtype} {tuple(t.shape)}, expected {dtype} [F, {', '.join(str(s) for s in shape)}]")
    if t.shape[0] < 1 or not t[0].is_contiguous():
        raise ValueError(f"item_views: {name} needs at least one frame and contiguous frames, strides {t.stride()}")
    frame = int(np.prod(shape)) * t.element_size()
    slot = t.stride(0) * t.element_size() if t.shape[0] > 1 else -(-frame // 16) * 16
    if t.data_ptr() % 16 or slot % 16 or slot < frame:
        raise ValueError(f"item_views: {name} at {t.data_ptr():#x} with frames {slot} bytes apart: both must be multiples of 16 "
                         "(pad the frame slots)")
    return t, slot


def item_views(rgb, dyn_mask, depth, groups, out=None):
    """The resident loaders' item builder (``pgdvs_item_views``; include/pgdvs_hip.h).  The store's tables on the GPU: rgb
    uint8 [F,H,W,3], dyn_mask uint8 [F,H,W], depth float32 [F,H,W], frames contiguous and a multiple of 16 bytes apart.
    ``groups``: up to 4 pairs (frame ids, with_depth) of together up to 64 views; ids may repeat.  Returns one dict per
    group: rgb, dyn_rgb, static_rgb float32 [n,H,W,3], dyn_mask [n,H,W,1] and, with depth, depth [n,H,W,1], filled by one
    launch: rgb = byte / 255, dyn_mask = float(byte), dyn_rgb = rgb * dyn_mask, static_rgb = rgb * (1 - dyn_mask), the bits
    of the loaders' numpy statements.  ``out``: such dicts of contiguous GPU tensors to fill in place.  Does not synchronise."""
    groups = [([int(i) for i in ids], bool(with_depth)) for ids, with_depth in groups]
    if not 1 <= len(groups) <= ITEM_MAX_GROUPS or any(not ids for ids, _ in groups):
        raise ValueError(f"item_views: {len(groups)} groups of {[len(ids) for ids, _ in groups]} views (1 to {ITEM_MAX_GROUPS} "
                         "groups, none empty)")
    ids = [i for g, _ in groups for i in g]
    if len(ids) > ITEM_MAX_VIEWS:
        raise ValueError(f"item_views: {len(ids)} views, at most {ITEM_MAX_VIEWS}")
    if rgb.ndim != 4:
        raise ValueError(f"item_views: rgb [F,H,W,3] expected, got {tuple(rgb.shape)}")
    F, H, W = (int(x) for x in rgb.shape[:3])
    c, c_slot = _store_table(rgb, torch.uint8, (H, W, 3), "rgb")
    m, m_slot = _store_table(dyn_mask, torch.uint8, (H, W), "dyn_mask")
    d, d_slot = _store_table(depth, torch.float32, (H, W), "depth")
    if not (m.shape[0] == d.shape[0] == F and m.device == d.device == c.device):
        raise ValueError(f"item_views: tables of {F}, {m.shape[0]}, {d.shape[0]} frames on {c.device}, {m.device}, {d.device}")
    if min(ids) < 0 or max(ids) >= F:
        raise ValueError(f"item_views: frame ids {ids} outside the store's {F} frames")
    shapes = {"rgb": 3, "dyn_mask": 1, "dyn_rgb": 3, "static_rgb": 3, "depth": 1}
    if out is None:
        out = [{k: torch.empty((len(g), H, W, shapes[k]), dtype=torch.float32, device=c.device)
                for k in ITEM_VIEW_KEYS if k != "depth" or with_depth} for g, with_depth in groups]
    ptrs = []
    for (g, with_depth), o in zip(groups, out):
        if set(o) != set(ITEM_VIEW_KEYS) - (set() if with_depth else {"depth"}):
            raise ValueError(f"item_views: out keys {sorted(o)} for a group with{'' if with_depth else 'out'} depth")
        for k in ITEM_VIEW_KEYS:
            t = o.get(k)
            if t is not None and (not t.is_cuda or t.device != c.device or t.dtype != torch.float32 or not t.is_contiguous() or
                                  tuple(t.shape) != (len(g), H, W, shapes[k])):
                raise ValueError(f"item_views: out[{k!r}] must be a contiguous float32 {(len(g), H, W, shapes[k])} tensor on {c.device}")
            ptrs.append(0 if t is None else t.data_ptr())
    if len(out) != len(groups):
        raise ValueError(f"item_views: {len(out)} out dicts for {len(groups)} groups")
    sizes = [len(g) for g, _ in groups]
    check(_lib.load().pgdvs_item_views(_ptr(c), _ptr(m), _ptr(d), F, H, W, c_slot, m_slot, d_slot, (C.c_int32 * len(ids))(*ids), len(ids),
                                       (C.c_int32 * len(sizes))(*sizes), len(sizes), (C.c_void_p * len(ptrs))(*ptrs), _stream()),
          "pgdvs_item_views")
    return out


def item_zoe_depth(pred_table, ids_by_group, scale_shift, rays=None, inv_c2w_tgt=None, near_far=None, out=None):
    """The resident store's ZoeDepth depths (``pgdvs_item_zoe_depths``; include/pgdvs_hip.h).  ``pred_table``: the store's
    depth table in prediction mode, float32 [F,H,W] on the GPU, frames contiguous and a multiple of 16 bytes apart.
    ``ids_by_group``: up to 4 lists of frame ids, together up to 64 views; ids may repeat.  ``scale_shift``: numpy float64
    [views, 2], the (scale, shift) of every view in the groups' order.  Returns ([depth float32 [n,H,W,1] per group], None):
    ``datasets.nvidia_eval.zoe_align`` of every view under NumPy 2, rounded to float32, in one launch.  With ``rays``
    (float32 [len(ids_by_group[0]),12] on the GPU, as in ``nvidia_depth_range``) and the target's float64
    ``inv_c2w_tgt[4,4]`` the second entry is depth_range[2] float32 on the GPU over the first group's cloud, unprojected
    with the float64 depths (``nvidia_zoe_depth``'s bits); ``near_far``: optional device float64[2] for the pair before the
    cast.  ``out``: one contiguous float32 GPU tensor [n,H,W,1] per group to fill in place.  Does not synchronise."""
    groups = [[int(i) for i in ids] for ids in ids_by_group]
    if not 1 <= len(groups) <= ITEM_MAX_GROUPS or any(not g for g in groups):
        raise ValueError(f"item_zoe_depth: {len(groups)} groups of {[len(g) for g in groups]} views (1 to {ITEM_MAX_GROUPS} "
                         "groups, none empty)")
    ids = [i for g in groups for i in g]
    if len(ids) > ITEM_MAX_VIEWS:
        raise ValueError(f"item_zoe_depth: {len(ids)} views, at most {ITEM_MAX_VIEWS}")
    if not isinstance(pred_table, torch.Tensor) or pred_table.ndim != 3:
        raise ValueError(f"item_zoe_depth: pred_table [F,H,W] expected, got {tuple(getattr(pred_table, 'shape', ()))}")
    F, H, W = (int(x) for x in pred_table.shape)
    p, slot = _store_table(pred_table, torch.float32, (H, W), "pred_table")
    if min(ids) < 0 or max(ids) >= F:
        raise ValueError(f"item_zoe_depth: frame ids {ids} outside the store's {F} frames")
    ss = np.ascontiguousarray(np.asarray(scale_shift), dtype=np.float64)
    if ss.shape != (len(ids), 2):
        raise ValueError(f"item_zoe_depth: scale_shift {ss.shape}, expected {(len(ids), 2)}")
    if (rays is None) != (inv_c2w_tgt is None) or (near_far is not None and rays is None):
        raise ValueError("item_zoe_depth: rays and inv_c2w_tgt go together, near_far only with them")
    if out is None:
        out = [torch.empty((len(g), H, W, 1), dtype=torch.float32, device=p.device) for g in groups]
    if len(out) != len(groups):
        raise ValueError(f"item_zoe_depth: {len(out)} out tensors for {len(groups)} groups")
    for g, t in zip(groups, out):
        _out(t, (len(g), H, W, 1), torch.float32, p.device, "item_zoe_depth: out[g]")
    lib = _lib.load()
    sizes = [len(g) for g in groups]
    head = (_ptr(p), F, H, W, slot, (C.c_int32 * len(ids))(*ids), len(ids), _mat64(ss, 2 * len(ids)), (C.c_int32 * len(sizes))(*sizes),
            len(sizes), (C.c_void_p * len(out))(*[t.data_ptr() for t in out]))
    if rays is None:
        check(lib.pgdvs_item_zoe_depths(*head, None, None, None, None, None, 0, _stream()), "pgdvs_item_zoe_depths")
        return out, None
    r = _req(rays, torch.float32, "rays")
    if tuple(r.shape) != (sizes[0], 12) or r.device != p.device:
        raise ValueError(f"item_zoe_depth: rays {tuple(r.shape)} on {r.device}, expected {(sizes[0], 12)} (the first group's views) on "
                         f"{p.device}")
    mat = _mat64(inv_c2w_tgt, 16)
    ws = _ws(lib.pgdvs_item_zoe_depths_workspace_bytes(sizes[0], H, W), p.device)
    rng = torch.empty((2,), dtype=torch.float32, device=p.device)
    check(lib.pgdvs_item_zoe_depths(*head, _ptr(r), mat, _ptr(rng), _out64(near_far), _ptr(ws), ws.numel(), _stream()),
          "pgdvs_item_zoe_depths")
    return out, rng


def flow_occ(coord_diff, thres):
    """A flow file's occlusion mask (``pgdvs_flow_occ``; include/pgdvs_hip.h): coord_diff[H,W,2] float32 on the GPU and the
    Python number ``thres`` -> float32 [H,W] = sum |coord_diff| > thres, the sum and the compare in float32 as NumPy 2
    compares a float32 array with a Python scalar (``datasets._common.read_flow_npz``); NaN gives 0.  Does not synchronise."""
    cd = _req(coord_diff, torch.float32, "coord_diff")
    if cd.ndim != 3 or cd.shape[2] != 2 or cd.shape[0] < 1 or cd.shape[1] < 1:
        raise ValueError(f"flow_occ: coord_diff [H,W,2] expected, got {tuple(cd.shape)}")
    if type(thres) not in (int, float):  # (np.float64 is a float subclass)
        raise TypeError(f"flow_occ: thres must be a Python number (a NumPy scalar would change the compare's type), got {type(thres)}")
    H, W = int(cd.shape[0]), int(cd.shape[1])
    occ = torch.empty((H, W), dtype=torch.float32, device=cd.device)
    check(_lib.load().pgdvs_flow_occ(_ptr(cd), H, W, float(np.float32(thres)), _ptr(occ), _stream()), "pgdvs_flow_occ")
    return occ


def _bytes_image(t, shape, name):
    """a contiguous uint8 GPU tensor of ``shape``, passed as it lies (no copy: its address decides the kernel's path)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PgdvsHipError(f"item_target: {name}: expected a GPU tensor (no CPU fallback)")
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"item_target: {name} {t.dtype} {tuple(t.shape)}, expected a contiguous uint8 {tuple(shape)}")
    return t


def item_target(rgb_u8, covisible_u8=None, out=None):
    """The DyCheck loader's target from its bytes (``pgdvs_item_target``; include/pgdvs_hip.h): rgb_u8 uint8 [H,W,3] and,
    optionally, covisible_u8 uint8 [H,W] on the GPU -> (rgb float32 [H,W,3] = byte / 255, mask float32 [H,W,1] = covisible
    > 0, or None without a covisible image), the bits of ``raw.astype(np.float32) / 255.0`` and ``(covisible >
    0).astype(np.float32)[..., None]``.  ``out``: such a pair of contiguous float32 GPU tensors to fill in place (the
    second None exactly when there is no covisible image).  One launch; does not synchronise."""
    if not isinstance(rgb_u8, torch.Tensor) or rgb_u8.ndim != 3 or rgb_u8.shape[2] != 3:
        raise ValueError(f"item_target: rgb_u8 [H,W,3] expected, got {tuple(getattr(rgb_u8, 'shape', ()))}")
    H, W = int(rgb_u8.shape[0]), int(rgb_u8.shape[1])
    c = _bytes_image(rgb_u8, (H, W, 3), "rgb_u8")
    m = None if covisible_u8 is None else _bytes_image(covisible_u8, (H, W), "covisible_u8")
    if m is not None and m.device != c.device:
        raise ValueError(f"item_target: rgb_u8 on {c.device}, covisible_u8 on {m.device}")
    if out is None:
        out = (torch.empty((H, W, 3), dtype=torch.float32, device=c.device),
               None if m is None else torch.empty((H, W, 1), dtype=torch.float32, device=c.device))
    if not isinstance(out, (tuple, list)) or len(out) != 2 or (out[1] is None) != (m is None):
        raise ValueError("item_target: out is a pair (rgb, mask), the mask None exactly when covisible_u8 is")
    for t, shape, name in ((out[0], (H, W, 3), "out[0]"), (out[1], (H, W, 1), "out[1]")):
        if t is not None:
            _out(t, shape, torch.float32, c.device, f"item_target: {name}", shown=f"{shape} tensor")
    check(_lib.load().pgdvs_item_target(_ptr(c), _ptr(m), H, W, _ptr(out[0]), _ptr(out[1]), _stream()), "pgdvs_item_target")
    return out[0], out[1]


RESAMPLE_FILTERS = {"box": 0, "lanczos": 1}
RESAMPLE_PLANS = 32  # the plans kept, least recently used first out
_resample_plans = OrderedDict()


class ResamplePlan:
    """The tables of one resize on one device: ``tables`` = (bounds_h, kk_h, bounds_v, kk_v), int32 GPU tensors as
    ``pgdvs_resample_table`` makes them, None for an axis that keeps its size."""

    def __init__(self, in_hw, out_hw, filter, device, tables):
        self.in_hw, self.out_hw, self.filter, self.device, self.tables = in_hw, out_hw, filter, device, tables


def _resample_axis(n_in, n_out, filter_id, device):
    """one axis' (bounds [out,2], kk [out,ksize]) on ``device``, None when the axis keeps its size or the table entry refuses
    it (the message stays in ``pgdvs_last_error``); the second value tells the two apart"""
    lib = _lib.load()
    ksize = lib.pgdvs_resample_table(n_in, n_out, filter_id, None, None)
    if ksize < 0:
        return None, False
    if n_in == n_out:
        return None, True
    host = torch.empty(n_out * (2 + ksize), dtype=torch.int32, pin_memory=True)
    bounds, kk = host[:n_out * 2], host[n_out * 2:]
    if lib.pgdvs_resample_table(n_in, n_out, filter_id, C.c_void_p(bounds.data_ptr()), C.c_void_p(kk.data_ptr())) != ksize:
        raise PgdvsHipError("pgdvs_resample_table: " + lib.pgdvs_last_error().decode("utf-8", "replace"))
    dev = host.to(device, non_blocking=True)  # one copy from pinned memory; the stream orders it in front of its first use
    return (dev[:n_out * 2].view(n_out, 2), dev[n_out * 2:].view(n_out, ksize)), True


def resample_plan(in_hw, out_hw, filter, device, reject_ok: bool = False):
    """The coefficient tables of ``resample_u8`` for images of ``in_hw`` = (H, W) resized to ``out_hw`` with ``filter`` ("box"
    or "lanczos"): built on the host by ``pgdvs_resample_table`` (Pillow's precompute_coeffs and normalize_coeffs_8bpc),
    uploaded to ``device`` and kept in an LRU of ``RESAMPLE_PLANS`` entries keyed by sizes, filter and device.  A size the
    table entry refuses (outside 1 .. 16384, or more than 256 taps per output pixel) raises ValueError; with ``reject_ok``
    it returns None instead, for callers that keep a host path.  Does not synchronise."""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"resample: filter {filter!r}, expected one of {sorted(RESAMPLE_FILTERS)}")
    in_hw, out_hw, device = tuple(int(x) for x in in_hw), tuple(int(x) for x in out_hw), torch.device(device)
    if len(in_hw) != 2 or len(out_hw) != 2:
        raise ValueError(f"resample: sizes (H, W) expected, got {in_hw} -> {out_hw}")
    if device.type != "cuda":
        raise ValueError(f"resample: the tables live on a GPU, got device {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (in_hw, out_hw, filter, device)
    plan = _resample_plans.get(key)
    if plan is not None:
        _resample_plans.move_to_end(key)
        return plan
    fid = RESAMPLE_FILTERS[filter]
    (tab_v, ok_v), (tab_h, ok_h) = (_resample_axis(in_hw[i], out_hw[i], fid, device) for i in (0, 1))
    if not (ok_v and ok_h):
        if reject_ok:
            return None
        raise ValueError(f"resample: {in_hw} -> {out_hw} ({filter}) is refused: " + _lib.load().pgdvs_last_error().decode("utf-8", "replace"))
    plan = _resample_plans[key] = ResamplePlan(in_hw, out_hw, filter, device, (tab_h or (None, None)) + (tab_v or (None, None)))
    while len(_resample_plans) > RESAMPLE_PLANS:
        _resample_plans.popitem(last=False)
    return plan


def resample_u8(img, out_hw, filter, out=None):
    """Pillow's ``Image.resize((w, h), resample=BOX | LANCZOS)`` of 8-bit images on the GPU, bit for bit (``pgdvs_resample_u8``;
    include/pgdvs_hip.h).  ``img``: uint8 [H,W], [H,W,C] or [N,H,W,C] on the GPU, C 1 or 3, every frame contiguous (frames may
    lie any distance apart, as a store's padded slots do); ``out_hw`` = (h, w); ``filter`` "box" or "lanczos".  Returns the
    resized images in ``img``'s layout.  ``out``: a uint8 GPU tensor of that shape to fill in place, its frames contiguous
    (e.g. a frame's slot of the resident store: the bytes between frames are left alone).  An axis that keeps its size is
    skipped; with both kept the result is a copy.  Wrong dtype, device, channels, ``out`` or a refused size: ValueError before
    anything is launched.  Does not synchronise."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or not img.is_cuda:
        raise ValueError(f"resample_u8: img must be a uint8 GPU tensor, got {getattr(img, 'dtype', type(img))} on {getattr(img, 'device', None)}")
    if img.ndim not in (2, 3, 4):
        raise ValueError(f"resample_u8: img [H,W], [H,W,C] or [N,H,W,C] expected, got {tuple(img.shape)}")
    x = img[None, ..., None] if img.ndim == 2 else (img[None] if img.ndim == 3 else img)
    N, H, W, ch = (int(s) for s in x.shape)
    if ch not in (1, 3) or N < 1:
        raise ValueError(f"resample_u8: {N} frames of {ch} channels (at least one frame, 1 or 3 channels)")
    if not x[0].is_contiguous() or (N > 1 and x.stride(0) < H * W * ch):
        x = x.contiguous()
    h, w = (int(s) for s in out_hw)
    plan = resample_plan((H, W), (h, w), filter, x.device)
    shape = {2: (h, w), 3: (h, w, ch), 4: (N, h, w, ch)}[img.ndim]
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != x.device or tuple(out.shape) != shape):
        raise ValueError(f"resample_u8: out must be a uint8 {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    o = out[None, ..., None] if img.ndim == 2 else (out[None] if img.ndim == 3 else out)
    if not o[0].is_contiguous() or (N > 1 and o.stride(0) < h * w * ch):
        raise ValueError(f"resample_u8: out's frames must be contiguous and not overlap, strides {tuple(out.stride())}")
    lib = _lib.load()
    fid = RESAMPLE_FILTERS[filter]
    ws = _ws(lib.pgdvs_resample_u8_workspace_bytes(N, H, W, ch, h, w, fid), x.device)
    check(lib.pgdvs_resample_u8(_ptr(x), x.stride(0) if N > 1 else H * W * ch, N, H, W, ch, _ptr(o), o.stride(0) if N > 1 else h * w * ch,
                                h, w, fid, *(_ptr(t) for t in plan.tables), _ptr(ws), ws.numel(), _stream()), "pgdvs_resample_u8")
    return out


JPEG_SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")  # pgdvs_jpeg_info.sampling


def _file_bytes(data, codec):
    """the file as a read-only byte buffer and its address (no copy for bytes, bytearray or a contiguous uint8 array);
    ``codec``: who asks, the first word of the TypeError's text"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1 or not data.flags.c_contiguous:
            raise TypeError(f"{codec}: data as an array must be contiguous uint8 [n], got {data.dtype} {data.shape}")
        return data, C.c_void_p(data.ctypes.data), data.size
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError(f"{codec}: data must be bytes, bytearray, memoryview or a uint8 array, got {type(data)}")
    arr = np.frombuffer(data, dtype=np.uint8)
    return arr, C.c_void_p(arr.ctypes.data if arr.size else 0), arr.size


def _jpeg_parse(data):
    """(JpegInfo, keep-alive, pointer, size) of a served stream, or None with the reason in ``pgdvs_last_error``"""
    keep, ptr, n = _file_bytes(data, "jpeg")
    info = _lib.JpegInfo()
    rc = _lib.load().pgdvs_jpeg_parse(ptr, n, C.byref(info))
    if rc < 0:
        check(rc, "pgdvs_jpeg_parse")
    return None if rc else (info, keep, ptr, n)


def jpeg_info(data):
    """What ``pgdvs_jpeg_parse`` reads from a JPEG stream (bytes-like or a uint8 array; host only, include/pgdvs_hip.h): a dict
    of width, height, sampling ("4:4:4", "4:2:2" or "4:2:0"), restart_interval (MCUs, 0 = none), blocks (per component, (rows,
    columns) of 8 x 8 blocks, padded to whole MCUs), coef_bytes and quant (uint16 [3,64], natural order) -- or None when
    ``jpeg_decode`` does not serve the stream (the reason is ``pgdvs_last_error``'s)."""
    got = _jpeg_parse(data)
    if got is None:
        return None
    info = got[0]
    return {"width": info.width, "height": info.height, "sampling": JPEG_SAMPLINGS[info.sampling], "restart_interval": info.restart_interval,
            "blocks": [(info.blocks_h[c], info.blocks_w[c]) for c in range(3)], "coef_bytes": info.coef_bytes,
            "quant": np.ctypeslib.as_array(info.quant).copy()}


JPEG_SCAN_SUB_BYTES = 64  # PGDVS_JPEG_SCAN_SUB_BYTES
JPEG_SCAN_MAX_BYTES = 1 << 25  # PGDVS_JPEG_SCAN_MAX_BYTES
JPEG_ENTROPY_MODES = ("host", "device")
_side_streams = {}  # (codec, device) -> the stream that codec's decode launches run on


def image_kind(data):
    """ "png", "jpeg" or None by the file's first bytes: its signature decides, as it does for Pillow, not its name"""
    head = bytes(data[:8])
    return "png" if head == PNG_SIGNATURE else "jpeg" if head[:2] == b"\xff\xd8" else None


def _cuda_device(device, what, outs=()):
    """the GPU an op runs on, with its index: ``device`` where given, else that of the first GPU tensor of ``outs``, else the
    current GPU; anything but a GPU is refused"""
    if device is None:
        device = next((o.device for o in outs if isinstance(o, torch.Tensor) and o.is_cuda), None)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{what} on a GPU, got device {device}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


@contextlib.contextmanager
def _side_stream(codec, device, written=()):
    """A decode op's launches on the side stream of its codec and device.  On entry that stream waits for the caller's (an
    ``out`` may still be read or written there) and becomes the current one; the body uploads, launches and calls the yielded
    ``fetch(status)`` where the host's wait shall end: the status words are copied to pinned memory and an event is recorded
    right there.  On exit the caller's stream waits for the side stream, the tensors of ``written`` (allocated on the caller's
    stream, filled on this one) are recorded on it, and the host waits for that one event: ``fetch``'s words are then valid."""
    with torch.cuda.device(device):
        main = torch.cuda.current_stream(device)
        side = _side_streams.get((codec, device))
        if side is None:
            side = _side_streams[codec, device] = torch.cuda.Stream(device)
        fetched = torch.cuda.Event()

        def fetch(status):
            words = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
            words.copy_(status, non_blocking=True)
            fetched.record(side)
            return words

        side.wait_stream(main)
        with torch.cuda.stream(side):
            yield fetch
        main.wait_stream(side)
        for t in written:
            t.record_stream(side)
        fetched.synchronize()  # the call's one wait


def jpeg_scan_prepare(data, sub_bytes: int = 0):
    """``pgdvs_jpeg_scan_prepare`` (host only; include/pgdvs_hip.h): (prepared, info) -- a pinned uint8 tensor with the tables,
    the segment table and the unstuffed scan of a baseline JPEG cut into subsequences of ``sub_bytes`` bytes (0: the
    default, ``JPEG_SCAN_SUB_BYTES``), and the ``JpegInfo`` -- or None where the stream is refused (``pgdvs_last_error`` says
    why: what ``jpeg_info`` refuses, a bad RSTn marker, or a scan above ``JPEG_SCAN_MAX_BYTES``)."""
    lib = _lib.load()
    keep, ptr, n = _file_bytes(data, "jpeg")
    need = lib.pgdvs_jpeg_scan_prepare_bytes(ptr, n, sub_bytes)
    if need < 0:
        check(int(need), "pgdvs_jpeg_scan_prepare_bytes")
    if need == 0:
        return None
    prepared = torch.empty(int(need), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    info = _lib.JpegInfo()
    rc = lib.pgdvs_jpeg_scan_prepare(ptr, n, sub_bytes, C.c_void_p(prepared.data_ptr()), prepared.numel(), C.byref(info))
    if rc < 0:
        check(rc, "pgdvs_jpeg_scan_prepare")
    return None if rc else (prepared, info)


def _jpeg_scan_launch(prepared, info, device):
    """the copy and the scan kernels on the current stream -> (device copy of ``prepared``, coef, status word, workspace)"""
    lib = _lib.load()
    dev = prepared.to(device, non_blocking=True)
    coef = torch.empty(info.coef_bytes // 2, dtype=torch.int16, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    ws = _ws(lib.pgdvs_jpeg_scan_decode_workspace_bytes(C.c_void_p(prepared.data_ptr()), prepared.numel()), device)
    check(lib.pgdvs_jpeg_scan_decode(C.c_void_p(prepared.data_ptr()), _ptr(dev), prepared.numel(), _ptr(coef), info.coef_bytes, _ptr(status),
                                     _ptr(ws), ws.numel(), _stream()), "pgdvs_jpeg_scan_decode")
    return dev, coef, status, ws


def jpeg_scan_decode(data, device=None, sub_bytes: int = 0, return_rounds: bool = False):
    """The Huffman scan of a baseline YCbCr JPEG decoded on the GPU (``pgdvs_jpeg_scan_prepare`` on the host, then
    ``pgdvs_jpeg_scan_decode``; include/pgdvs_hip.h): (coef, status) -- the int16 coefficients ``pgdvs_jpeg_entropy_decode``
    gives, flat, on ``device``, and the status word as an int (0: decoded; else ``PGDVS_JPEG_SCAN_*`` bits, and ``coef`` holds
    no result).  For tests and tools: it waits for the device.  A stream the preparation refuses raises ValueError.
    ``return_rounds``: a third value, (rounds of the first launch, fix-up launches that ran)."""
    device = _cuda_device(device, "jpeg_scan_decode: the scan is decoded")
    got = jpeg_scan_prepare(data, sub_bytes)
    if got is None:
        raise ValueError("jpeg_scan_decode: the stream is not served: " + _lib.load().pgdvs_last_error().decode("utf-8", "replace"))
    prepared, info = got
    with torch.cuda.device(device):
        _, coef, status, ws = _jpeg_scan_launch(prepared, info, device)
        st = int(status.cpu()[0]) & 0xFFFFFFFF
        if return_rounds:
            return coef, st, tuple(int(x) for x in ws[:8].cpu().view(torch.int32))  # (the workspace's first two words)
    return coef, st


def jpeg_decode(data, out=None, device=None, reject_ok: bool = False, entropy: str = "host"):
    """``np.array(PIL.Image.open(BytesIO(data)))`` of a baseline YCbCr JPEG as a uint8 [H,W,3] GPU tensor, byte for byte (Pillow
    over libjpeg-turbo).  The markers and the Huffman scan are read on the host (``pgdvs_jpeg_parse``,
    ``pgdvs_jpeg_entropy_decode``: C, the GIL released) into a fresh pinned int16 buffer that also carries the three
    quantisation tables; one asynchronous copy takes it to ``device`` (default: ``out``'s, else the current GPU) and
    ``pgdvs_jpeg_reconstruct`` dequantises, inverts the DCT, upsamples the chroma and converts the colours there, on the
    current stream.  ``out``: a contiguous uint8 [H,W,3] tensor on the device to fill (e.g. a frame's slot of the resident
    store).  A stream the path does not serve (include/pgdvs_hip.h lists what it does) raises ValueError with the library's
    reason, or returns None under ``reject_ok`` -- in front of any device work, so the caller can hand the file to Pillow.
    Does not synchronise.

    ``entropy="device"``: the scan is decoded on the GPU too.  The host only prepares it (``pgdvs_jpeg_scan_prepare``: one
    pass over the bytes, no Huffman work) into a pinned buffer; one asynchronous copy takes that buffer -- the file's size,
    not the coefficients' -- to the device; ``pgdvs_jpeg_scan_decode`` and ``pgdvs_jpeg_reconstruct`` run on this op's side
    stream, ordered against the caller's (``_side_stream``), and THIS CALL WAITS for the scan's status word: once per file,
    the mode's price -- "does not synchronise" belongs to ``entropy="host"`` alone.  A non-zero status (a corrupt scan, or
    anything the device path does not settle) reruns the file through the host path above, which serves it, refuses it or
    leaves it to the caller exactly as ``entropy="host"`` does; the second value of ``jpeg_decode_device`` tells the two apart."""
    if entropy not in JPEG_ENTROPY_MODES:
        raise ValueError(f"jpeg_decode: entropy {entropy!r}, expected one of {JPEG_ENTROPY_MODES}")
    if entropy == "device":
        return jpeg_decode_device(data, out=out, device=device, reject_ok=reject_ok)[0]
    lib = _lib.load()

    def refused():
        if reject_ok:
            return None
        raise ValueError("jpeg_decode: the stream is not served: " + lib.pgdvs_last_error().decode("utf-8", "replace"))

    got = _jpeg_parse(data)
    if got is None:
        return refused()
    info, keep, ptr, n = got
    device = _cuda_device(device, "jpeg_decode: the image is reconstructed", (out,))
    out = _out(out, (info.height, info.width, 3), torch.uint8, device, "jpeg_decode: out")
    nq = C.sizeof(info.quant)
    host = torch.empty((info.coef_bytes + nq) // 2, dtype=torch.int16, pin_memory=True)
    rc = lib.pgdvs_jpeg_entropy_decode(ptr, n, C.c_void_p(host.data_ptr()), info.coef_bytes)
    if rc < 0:
        check(rc, "pgdvs_jpeg_entropy_decode")
    if rc:
        return refused()
    C.memmove(host.data_ptr() + info.coef_bytes, info.quant, nq)
    dev = host.to(device, non_blocking=True)
    ws = _ws(lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)), device)
    check(lib.pgdvs_jpeg_reconstruct(_ptr(dev), C.c_void_p(dev.data_ptr() + info.coef_bytes), C.byref(info), _ptr(out), info.width * 3, _ptr(ws),
                                     ws.numel(), _stream()), "pgdvs_jpeg_reconstruct")
    return out


def jpeg_decode_device(data, out=None, device=None, reject_ok: bool = False):
    """``jpeg_decode(..., entropy="device")`` with its account: (image or None, scan_decoded_on_device).  False: the device
    path gave the file up (the preparation refused it, or the scan's status word was not zero) and the image, the None or the
    ValueError is the host path's.  After a non-zero status ``out`` has been written by the reconstruction of an unfinished
    scan before the host path fills or refuses it."""
    lib = _lib.load()
    got = jpeg_scan_prepare(data)
    if got is None:  # what the markers refuse, a bad RSTn, an oversized scan: the host path says which and decides
        return jpeg_decode(data, out=out, device=device, reject_ok=reject_ok), False
    prepared, info = got
    device = _cuda_device(device, "jpeg_decode: the image is reconstructed", (out,))
    out = _out(out, (info.height, info.width, 3), torch.uint8, device, "jpeg_decode: out")
    hd = _lib.JpegScanHeader.from_address(prepared.data_ptr())
    with _side_stream("jpeg", device) as fetch:
        dev, coef, status, _ = _jpeg_scan_launch(prepared, info, device)
        word = fetch(status)  # behind the scan, in front of the reconstruction: the mode's one wait is for the scan alone
        ws = _ws(lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)), device)
        check(lib.pgdvs_jpeg_reconstruct(_ptr(coef), C.c_void_p(dev.data_ptr() + hd.off_quant), C.byref(info), _ptr(out), info.width * 3,
                                         _ptr(ws), ws.numel(), _stream()), "pgdvs_jpeg_reconstruct")
    if int(word[0]) == 0:
        return out, True
    return jpeg_decode(data, out=out, device=device, reject_ok=reject_ok), False


PNG_INFLATE_SUB_BYTES = 64  # PGDVS_PNG_INFLATE_SUB_BYTES
PNG_INFLATE_MAX_BYTES = 1 << 28  # PGDVS_PNG_INFLATE_MAX_BYTES
PNG_MAX_SIZE = 16384
PNG_CHANNEL_MODES = ("file", "rgb")
PNG_STATUS_BITS = ("block", "code", "distance", "stored", "data_out", "size", "left_over", "adler", "filter", "not_synchronised")
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_KINDS = ("colour", "mask")  # what a call admits: 8-bit RGB / RGBA files; grey and palette files of 1, 2, 4 or 8 bits
PNG_GREY_SCALE = {1: 1, 2: 85, 4: 17, 8: 1}  # what Pillow's array multiplies a grey sample by (depth 1: its bool array)


def _png_kinds(kinds):
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    if not kinds or any(k not in PNG_KINDS for k in kinds):
        raise ValueError(f"png_decode: kinds {kinds!r}, expected some of {PNG_KINDS}")
    return kinds


def png_parse(data, kinds=("colour",)):
    """(info, None) of a PNG file ``png_decode`` serves, else (None, reason).  The chunk walk of the host side: signature,
    lengths, every CRC (``zlib.crc32``), chunk order, IHDR, and the two zlib header bytes -- no Huffman work, no inflate.
    ``info`` is ``png_info``'s dict and the file's bytes; a caller that walks a file itself (to size its ``out``) hands the
    pair back to ``png_decode_batch(parsed=...)`` as it is.  ``kinds``: "colour" admits 8-bit RGB and RGBA files, "mask"
    grey (colour type 0) and palette (3) files of bit depth 1, 2, 4 or 8, whose info has channels 1 and bit_depth and scale."""
    kinds = _png_kinds(kinds)
    import struct
    import zlib

    keep, _, n = _file_bytes(data, "png")
    mv = memoryview(keep)
    if n < 8 or bytes(mv[:8]) != PNG_SIGNATURE:
        return None, "not a PNG signature"
    pos, ihdr, spans, state = 8, None, [], 0  # state: 0 before IDAT, 1 inside the IDAT run, 2 behind it, 3 after IEND
    while state != 3:
        if pos + 12 > n:
            return None, "truncated: a chunk header or IEND is missing"
        (length,) = struct.unpack_from(">I", mv, pos)
        kind = bytes(mv[pos + 4:pos + 8])
        if length > 0x7FFFFFFF or pos + 12 + length > n:
            return None, f"truncated: chunk {kind!r} of {length} bytes runs past the file"
        if zlib.crc32(mv[pos + 4:pos + 8 + length]) != struct.unpack_from(">I", mv, pos + 8 + length)[0]:
            return None, f"bad CRC in chunk {kind!r}"
        if (ihdr is None) != (kind == b"IHDR"):
            return None, "chunk order: IHDR comes first, once"
        if kind == b"IHDR":
            if length != 13:
                return None, "IHDR of another length than 13"
            ihdr = struct.unpack_from(">IIBBBBB", mv, pos + 8)
        elif kind == b"IDAT":
            if state == 2:
                return None, "chunk order: IDAT chunks must follow each other"
            state = 1
            if length:
                spans.append((pos + 8, length))
        elif kind == b"IEND":
            if state == 0 or length:
                return None, "chunk order: IEND without IDAT, or with data"
            state = 3
        else:
            if kind in (b"tRNS", b"acTL", b"fcTL", b"fdAT"):
                return None, f"chunk {kind!r} (transparency or APNG) is left to the host reader"
            if not kind[0] & 0x20 and kind != b"PLTE":
                return None, f"unknown critical chunk {kind!r}"
            if state == 1:
                state = 2
        pos += 12 + length
    width, height, depth, colour, compression, filt, interlace = ihdr
    is_mask = "mask" in kinds and colour in (0, 3) and depth in (1, 2, 4, 8)
    if not is_mask and not ("colour" in kinds and depth == 8 and colour in (2, 6)):
        served = {"colour": "8-bit RGB and RGBA", "mask": "grey and palette files of 1, 2, 4 or 8 bits"}
        return None, f"colour type {colour} at bit depth {depth}: {' and '.join(served[k] for k in PNG_KINDS if k in kinds)} are served"
    if compression or filt or interlace:
        return None, "interlaced, or an unknown compression or filter method"
    if not (1 <= width <= PNG_MAX_SIZE and 1 <= height <= PNG_MAX_SIZE):
        return None, f"{width} x {height}: 1 .. {PNG_MAX_SIZE} pixels each way are served"
    channels = 1 if is_mask else 3 if colour == 2 else 4
    size = sum(length for _, length in spans)
    inflated = height * (1 + -(-width * channels * depth // 8))
    if inflated > PNG_INFLATE_MAX_BYTES or size > PNG_INFLATE_MAX_BYTES - 16:
        return None, f"stream of {size} bytes or image of {inflated}: above PNG_INFLATE_MAX_BYTES"
    if size < 6:
        return None, "truncated: a zlib stream of fewer than 6 bytes"
    head = bytearray()
    for o, length in spans:  # (the two header bytes may lie in two chunks)
        head += mv[o:o + min(length, 2 - len(head))]
        if len(head) == 2:
            break
    cmf, flg = head[0], head[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31:
        return None, "zlib header: not deflate with a window of 32K or less"
    if flg & 0x20:
        return None, "zlib header: preset dictionary"
    info = {"width": width, "height": height, "channels": channels, "stream_bytes": size, "idat": spans, "data": keep}
    if is_mask:  # the samples leave as bytes: a grey file's as Pillow scales them, a palette file's indices as they are
        info.update(bit_depth=depth, scale=PNG_GREY_SCALE[depth] if colour == 0 else 1, palette=colour == 3)
    return info, None


def png_info(data, kinds=("colour",)):
    """What the host side reads from a PNG file (bytes-like or a uint8 array; Python only): a dict of width, height, channels
    (3 or 4; a mask file: 1, with bit_depth and scale), stream_bytes (the zlib stream over all IDAT chunks) and idat (the
    payloads' (offset, length) in the file) -- or None when ``png_decode`` does not serve the file (``png_refusal`` gives the
    reason)."""
    info = png_parse(data, kinds)[0]
    return None if info is None else {k: v for k, v in info.items() if k != "data"}


def png_refusal(data, kinds=("colour",)):
    """why ``png_decode`` refuses the file on the host, or None where it does not"""
    return png_parse(data, kinds)[1]


def _png_inflated(info):
    """(the bytes a file inflates to, the bytes of a row behind its filter byte)"""
    row = -(-info["width"] * info["channels"] * info.get("bit_depth", 8) // 8)
    return info["height"] * (1 + row), row


def png_status_text(status: int) -> str:
    return "+".join(name for bit, name in enumerate(PNG_STATUS_BITS) if status >> bit & 1) or "ok"


def _png_batch(infos, out_channels, outs, pin):
    """the batch buffer of ``pgdvs_png_decode``: the stream table, then every file's IDAT payloads joined, 16-byte aligned;
    ``outs``: per stream (address, row stride in bytes).  An entry carries bit depth and scale: a mask file's, 8 and 1 for a
    colour file"""
    n = len(infos)
    offsets, at = [], -(-n * C.sizeof(_lib.PngImage) // 16) * 16
    for info in infos:
        offsets.append(at)
        at += -(-info["stream_bytes"] // 16) * 16
    buf = torch.zeros(at, dtype=torch.uint8, pin_memory=pin)
    view = buf.numpy()
    table = (_lib.PngImage * n).from_address(buf.data_ptr())
    for i, info in enumerate(infos):
        src, o = info["data"], offsets[i]
        table[i].bit_depth, table[i].scale = info.get("bit_depth", 8), info.get("scale", 1)
        for off, length in info["idat"]:
            view[o:o + length] = src[off:off + length]
            o += length
        table[i].offset, table[i].size = offsets[i], info["stream_bytes"]
        table[i].height, table[i].width, table[i].channels, table[i].out_channels = info["height"], info["width"], info["channels"], out_channels[i]
        table[i].out, table[i].row_stride = outs[i]
    return buf


def _png_out(out, shape, device, what):
    """``out`` after its check: uint8 ``shape`` ([H,W,C], or a mask's [H,W]) on ``device`` whose pixels are contiguous (the row
    stride is free)"""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    row = shape[1] * (shape[2] if len(shape) == 3 else 1)
    ok = (isinstance(out, torch.Tensor) and out.is_cuda and out.device == device and out.dtype == torch.uint8 and tuple(out.shape) == tuple(shape)
          and out.stride(-1) == 1 and (len(shape) == 2 or out.stride(1) == shape[2]) and (out.stride(0) >= row or shape[0] == 1))
    if not ok:
        raise ValueError(f"{what} must be a uint8 {tuple(shape)} tensor on {device} with contiguous rows, got {getattr(out, 'dtype', type(out))} "
                         f"{tuple(getattr(out, 'shape', ()))} strides {tuple(out.stride()) if isinstance(out, torch.Tensor) else ()} "
                         f"on {getattr(out, 'device', None)}")
    return out


def _png_shape(info, out_channels):
    return (info["height"], info["width"]) if "bit_depth" in info else (info["height"], info["width"], out_channels)


def png_decode_batch(datas, outs=None, channels: str = "file", device=None, reject_ok: bool = False, sub_bytes: int = 0, reasons=None, stats=None, parsed=None,
                     kinds=("colour",)):
    """``np.array(PIL.Image.open(BytesIO(data)))`` of every PNG file of ``datas`` as uint8 [H,W,C] GPU tensors, byte for byte
    (DESIGN.md 7j).  Served: non-interlaced 8-bit RGB (C = 3) and RGBA (C = 4) files of 1 .. 16384 pixels each way with one
    zlib stream over any number of IDAT chunks; ``channels="rgb"`` gives an RGBA file's first three channels.  The host
    walks the chunks and checks every CRC (Python; no Huffman work, no inflate) and joins all files' IDAT payloads behind
    one stream table in ONE pinned buffer; one asynchronous copy takes it to ``device`` (default: the outs', else the current
    GPU) and ONE batched ``pgdvs_png_decode`` -- a workgroup per file inflates it, then a wavefront per file undoes the row
    filters -- runs on this op's side stream, ordered against the caller's (``_side_stream``).  THIS CALL WAITS for the status
    words of all files, once per batch.  ``outs``: None, or per file None or a uint8 [H,W,C] tensor on the device to fill, its
    rows contiguous and its row stride free (a frame's slot of the resident store).

    A file the path does not serve is refused, never approximated: on the host, in front of any device work (another colour
    type or bit depth, interlace, tRNS or APNG chunks, a bad signature, CRC or chunk order, a truncated file, a zlib header
    that is not deflate / 32K or has a preset dictionary, sizes above ``PNG_INFLATE_MAX_BYTES``), or on the device by a
    non-zero status word (include/pgdvs_hip.h lists the bits; the file's ``out`` then holds no result).  Either way the
    file's entry of the result is None under ``reject_ok`` (``reasons``, a list, receives one text or None per file), else the
    first such file raises ValueError -- the caller hands the file to Pillow, which decides.  ``stats`` (a list, for tools: it
    waits for the device once more) receives per file None or the workspace's four words: windows, the most synchronisation
    rounds of a window, the most resolve rounds of a window, blocks.  ``parsed``: what ``png_parse`` gave for each file, where the
    caller has walked them already (``SceneStore``, to find each file's slot): the files are not walked again.

    ``kinds`` (``png_parse``): with "mask" in it, non-interlaced grey and palette files of bit depth 1, 2, 4 or 8 are served as
    well, each as a uint8 [H,W] tensor, byte for byte ``np.array(PIL.Image.open(...)).astype(np.uint8)``: grey
    samples as Pillow scales them, a palette file's indices; ``outs``: [H,W] with a free row stride.  Such files share the batch
    with the colour files: the same one buffer, copy, launch pair and wait."""
    if channels not in PNG_CHANNEL_MODES:
        raise ValueError(f"png_decode: channels {channels!r}, expected one of {PNG_CHANNEL_MODES}")
    kinds = _png_kinds(kinds)
    datas = list(datas)
    outs = [None] * len(datas) if outs is None else list(outs)
    if len(outs) != len(datas):
        raise ValueError(f"png_decode_batch: {len(datas)} files, {len(outs)} outs")
    why = [None] * len(datas)
    images = [None] * len(datas)
    walked, parsed = parsed, []
    for i, data in enumerate(datas):
        info, why[i] = png_parse(data, kinds) if walked is None else walked[i]
        if info is not None:
            parsed.append((i, info))
        elif not reject_ok:
            raise ValueError(f"png_decode: file {i} is not served: {why[i]}")
    if parsed:
        device = _cuda_device(device, "png_decode: the files are decoded", outs)
        lib = _lib.load()
        out_ch = [3 if channels == "rgb" and info["channels"] != 1 else info["channels"] for _, info in parsed]
        targets = [_png_out(outs[i], _png_shape(info, c), device, f"png_decode: out of file {i}") for (i, info), c in zip(parsed, out_ch)]
        batch = _png_batch([info for _, info in parsed], out_ch, [(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else t[0].numel()) for t in targets],
                           pin=True)
        n = len(parsed)
        with _side_stream("png", device, written=targets) as fetch:
            dev = batch.to(device, non_blocking=True)
            status = torch.empty(n, dtype=torch.int32, device=device)
            ws = _ws(lib.pgdvs_png_inflate_workspace_bytes(C.c_void_p(batch.data_ptr()), n), device)
            check(lib.pgdvs_png_decode(C.c_void_p(batch.data_ptr()), _ptr(dev), batch.numel(), n, sub_bytes, _ptr(status), _ptr(ws), ws.numel(), _stream()),
                  "pgdvs_png_decode")
            words = fetch(status)  # behind the whole batch: its one wait
        if stats is not None:
            rows = ws[:16 * n].cpu().view(torch.int32).view(n, 4).tolist()
            stats[:] = [None] * len(datas)
            for (i, _), row in zip(parsed, rows):
                stats[i] = tuple(row)
        for (i, _), target, word in zip(parsed, targets, words.tolist()):
            if word == 0:
                images[i] = target
            else:
                why[i] = f"the device gave the stream up: status {word & 0xFFFFFFFF:#x} ({png_status_text(word & 0xFFFFFFFF)})"
                if not reject_ok:
                    raise ValueError(f"png_decode: file {i} is not served: {why[i]}")
    if reasons is not None:
        reasons[:] = why
    return images


def png_decode(data, out=None, channels: str = "file", device=None, reject_ok: bool = False, sub_bytes: int = 0, kinds=("colour",)):
    """``png_decode_batch`` of one file: the uint8 [H,W,C] (a mask file: [H,W]) GPU tensor, or None under ``reject_ok`` where the
    file is not served."""
    return png_decode_batch([data], outs=[out], channels=channels, device=device, reject_ok=reject_ok, sub_bytes=sub_bytes, kinds=kinds)[0]


def png_decode_host(datas, channels: str = "file", sub_bytes: int = 0, guard: int = 0, kinds=("colour",)):
    """The host emulation of the same batch (``pgdvs_png_decode_host``: the kernels' core, windows, rounds and workspace on
    the CPU; for the tests and tools, no GPU): per file None where the host side refuses it, else a dict of status, image
    (uint8 [H,W,C] numpy, meaningful at status 0), inflated (the workspace's inflated rows) and info (windows, most
    synchronisation rounds, most resolve rounds, blocks).  ``guard``: that many bytes of 0xA5 are put around the images, the
    status words and the workspace, and checked afterwards.  ``kinds``: as ``png_decode_batch``; a mask file's image is [H,W]."""
    if channels not in PNG_CHANNEL_MODES:
        raise ValueError(f"png_decode: channels {channels!r}, expected one of {PNG_CHANNEL_MODES}")
    kinds = _png_kinds(kinds)
    lib = _lib.load()
    results = [None] * len(datas)
    parsed = [(i, info) for i, info in ((i, png_parse(d, kinds)[0]) for i, d in enumerate(datas)) if info is not None]
    if not parsed:
        return results
    n = len(parsed)
    out_ch = [3 if channels == "rgb" and info["channels"] != 1 else info["channels"] for _, info in parsed]

    def guarded(nbytes, align=1):
        raw = np.full(nbytes + 2 * guard + 256, 0xA5, np.uint8)
        start = guard + (-(raw.ctypes.data + guard) % align)
        return raw, raw[start:start + nbytes]

    holds = [guarded(info["height"] * info["width"] * c) for (_, info), c in zip(parsed, out_ch)]
    batch = _png_batch([info for _, info in parsed], out_ch, [(h[1].ctypes.data, info["width"] * c) for h, (_, info), c in zip(holds, parsed, out_ch)],
                       pin=False)
    need = lib.pgdvs_png_inflate_workspace_bytes(C.c_void_p(batch.data_ptr()), n)
    if need < 0:
        check(int(need), "pgdvs_png_inflate_workspace_bytes")
    ws_raw, ws = guarded(int(need), 256)
    st_raw, st = guarded(4 * n, 8)
    check(lib.pgdvs_png_decode_host(C.c_void_p(batch.data_ptr()), C.c_void_p(batch.data_ptr()), batch.numel(), n, sub_bytes, C.c_void_p(st.ctypes.data),
                                    C.c_void_p(ws.ctypes.data), int(need)), "pgdvs_png_decode_host")
    for raw, inner in [(ws_raw, ws), (st_raw, st)] + holds:
        lo = inner.ctypes.data - raw.ctypes.data
        if not ((raw[:lo] == 0xA5).all() and (raw[lo + inner.size:] == 0xA5).all()):
            raise AssertionError("pgdvs_png_decode_host wrote outside a buffer")
    at = -(-n * 16 // 256) * 256
    pad16 = lambda v: -(-v // 16) * 16  # noqa: E731
    for k, ((i, info), c, hold) in enumerate(zip(parsed, out_ch, holds)):
        nbytes, row = _png_inflated(info)
        results[i] = {"status": int(st.view(np.uint32)[k]), "image": hold[1].reshape(_png_shape(info, c)).copy(),
                      "inflated": ws[at:at + nbytes].copy(), "info": tuple(int(v) for v in ws[16 * k:16 * k + 16].view(np.uint32))}
        at += pad16(nbytes) + pad16(row)
    return results


MASK_PLACE_MODES = {"u8": 0, "bgr_f32": 1}  # PGDVS_MASK_PLACE_*
_nearest_maps = {}  # ((h, w), (H, W), device) -> int32 [H,W] on the device: Pillow's NEAREST picks


def nearest_map(src_hw, dst_hw, device):
    """int32 [H,W] on ``device``: the index y' * w + x' of the source pixel Pillow's NEAREST resize of an [h,w] image to [H,W]
    picks for every output pixel -- taken from Pillow itself, by resizing the indices (``_common.resize_nearest_f64``'s way),
    once per size pair and device"""
    import PIL.Image

    key = (tuple(int(v) for v in src_hw), tuple(int(v) for v in dst_hw), str(device))
    got = _nearest_maps.get(key)
    if got is None:
        (h, w), (H, W) = key[:2]
        idx = np.arange(h * w, dtype=np.int32).reshape(h, w)
        picks = np.array(PIL.Image.fromarray(idx).resize((W, H), resample=PIL.Image.Resampling.NEAREST))
        host = torch.empty(picks.shape, dtype=torch.int32, pin_memory=True)  # (pinned: the copy is asynchronous, nothing waits)
        host.copy_(torch.from_numpy(np.ascontiguousarray(picks, dtype=np.int32)))
        got = _nearest_maps[key] = host.to(device, non_blocking=True)
    return got


def mask_place(src, shape=None, mode: str = "u8", out=None):
    """A decoded mask into its place (``pgdvs_mask_place``; include/pgdvs_hip.h): ``src`` uint8 [h,w] or [h,w,C] on the GPU
    (pixels contiguous, the row stride free).  ``mode="u8"`` (C = 1): uint8 [H,W] = Pillow's NEAREST resize of ``src`` to
    ``shape`` (default: its own size), byte for byte, through ``nearest_map``; ``out``: a uint8 [H,W] tensor with a free row
    stride, e.g. a frame's slot of the resident store.  ``mode="bgr_f32"`` (C = 1 or 3): float32 [H,W,3] =
    ``np.float32(np.array(image.convert("RGB"))[..., ::-1] > 1e-3)`` of a grey or RGB mask file at its own size.  One launch
    on the current stream; does not synchronise (a size pair's map is uploaded once, without a wait)."""
    if mode not in MASK_PLACE_MODES:
        raise ValueError(f"mask_place: mode {mode!r}, expected one of {tuple(MASK_PLACE_MODES)}")
    ok = isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.ndim in (2, 3) and src.numel() > 0
    if ok:
        c = src.shape[2] if src.ndim == 3 else 1
        ok = (src.stride(-1) == 1 and (src.ndim == 2 or src.stride(1) == c) and (src.stride(0) >= src.shape[1] * c or src.shape[0] == 1) and
              (c == 1 or (c == 3 and mode == "bgr_f32")))
    if not ok:
        raise ValueError(f"mask_place: src must be a uint8 [h,w] or [h,w,C] GPU tensor with contiguous pixels (C = 3: mode 'bgr_f32' alone), got "
                         f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
    h, w = src.shape[:2]
    H, W = (h, w) if shape is None else (int(shape[0]), int(shape[1]))
    if mode == "bgr_f32" and (H, W) != (h, w):
        raise ValueError(f"mask_place: mode 'bgr_f32' keeps the size, got {(h, w)} -> {(H, W)}")
    index = None if (H, W) == (h, w) else nearest_map((h, w), (H, W), src.device)
    if mode == "u8":
        out = _png_out(out, (H, W), src.device, "mask_place: out")
        stride = out.stride(0) if H > 1 else W
    else:
        out = _out(out, (H, W, 3), torch.float32, src.device, "mask_place: out")
        stride = W * 12
    check(_lib.load().pgdvs_mask_place(_ptr(src), h, w, c, src.stride(0) if h > 1 else w * c, None if index is None else _ptr(index), H, W,
                                       MASK_PLACE_MODES[mode], _ptr(out), stride, _stream()), "pgdvs_mask_place")
    return out


DEPTH_OPS = {"copy": 0, "reciprocal": 1, "scale": 2}  # PGDVS_DEPTH_*
DEPTH_MAX_ENTRIES = 4096  # PGDVS_DEPTH_MAX_ENTRIES
# one depth payload of a ``depth_place`` batch: ``data`` (bytes-like) holds the little-endian float32 [h,w] array ``shape`` at
# byte ``offset`` (``datasets.npy_file`` finds it); ``op`` of DEPTH_OPS with its ``scale`` (a float32 value; used by "scale"
# alone); ``out``: the float32 [H,W] GPU tensor to fill, pixels contiguous, the row stride free
DepthRequest = namedtuple("DepthRequest", "data offset shape op scale out")


def depth_place(requests, device=None, align: int = 16):
    """The float32 payloads of depth files, as stored, into their places (``pgdvs_depth_place``; include/pgdvs_hip.h; DESIGN.md
    7l).  ``requests``: ``DepthRequest``s.  Every payload is copied once, as bytes, into ONE pinned buffer behind the entry
    table (each at a multiple of ``align`` bytes: 16, so the kernel loads 16 bytes per lane; the ABI asks for 4), one asynchronous
    copy takes the buffer to ``device`` (default: the outs') and ONE launch on the current stream writes every ``out``: "copy" the
    values themselves, "reciprocal" ``1 / (x + 1e-8)`` as NumPy 2 evaluates it on a float32 array, "scale" ``x * scale``, each
    bit for bit the numpy statement.  An ``out`` of another size than its source is filled through Pillow's own NEAREST
    picks (``nearest_map``).  Does not synchronise.  Returns the outs."""
    requests = list(requests)
    n = len(requests)
    if not 1 <= n <= DEPTH_MAX_ENTRIES:
        raise ValueError(f"depth_place: {n} requests (1 .. {DEPTH_MAX_ENTRIES})")
    if align < 4 or align % 4:
        raise ValueError(f"depth_place: align {align} (a multiple of 4)")
    device = _cuda_device(device, "depth_place: the payloads are placed", [r.out for r in requests])
    offsets, at = [], -(-n * C.sizeof(_lib.DepthEntry) // 16) * 16
    for i, r in enumerate(requests):
        h, w = (int(v) for v in r.shape)
        o = r.out
        ok = (isinstance(o, torch.Tensor) and o.is_cuda and o.device == device and o.dtype == torch.float32 and o.ndim == 2 and o.numel() > 0 and
              o.stride(1) == 1 and (o.stride(0) >= o.shape[1] or o.shape[0] == 1))
        if not ok:
            raise ValueError(f"depth_place: out of request {i} must be a float32 [H,W] tensor on {device} with contiguous rows, got "
                             f"{getattr(o, 'dtype', type(o))} {tuple(getattr(o, 'shape', ()))} on {getattr(o, 'device', None)}")
        if r.op not in DEPTH_OPS:
            raise ValueError(f"depth_place: request {i}: op {r.op!r}, expected one of {tuple(DEPTH_OPS)}")
        if h < 1 or w < 1 or r.offset < 0 or r.offset + h * w * 4 > len(r.data):
            raise ValueError(f"depth_place: request {i}: {h} x {w} floats at byte {r.offset} of {len(r.data)}")
        at = -(-at // align) * align
        offsets.append(at)
        at += h * w * 4
    buf = torch.empty(-(-at // 16) * 16, dtype=torch.uint8, pin_memory=True)
    view = buf.numpy()
    table = (_lib.DepthEntry * n).from_address(buf.data_ptr())
    for i, (r, off) in enumerate(zip(requests, offsets)):
        h, w = (int(v) for v in r.shape)
        H, W = (int(v) for v in r.out.shape)
        view[off:off + h * w * 4] = np.frombuffer(r.data, np.uint8, h * w * 4, r.offset)
        index = None if (H, W) == (h, w) else nearest_map((h, w), (H, W), device)
        e = table[i]
        e.offset, e.h, e.w, e.op, e.scale = off, h, w, DEPTH_OPS[r.op], float(np.float32(r.scale))
        e.map, e.out, e.out_row_stride, e.H, e.W = (None if index is None else index.data_ptr()), r.out.data_ptr(), (r.out.stride(0) if H > 1 else W) * 4, H, W
    with torch.cuda.device(device):
        dev = buf.to(device, non_blocking=True)
        check(_lib.load().pgdvs_depth_place(C.c_void_p(buf.data_ptr()), _ptr(dev), buf.numel(), n, _stream()), "pgdvs_depth_place")
    return [r.out for r in requests]


def percentile_f32(frames, q):
    """``np.percentile(frame, q)`` (NumPy 2, method "linear") of every frame of ``frames`` -- float32 GPU tensors of any shape, at
    least one value each -- as a float32 [len(frames)] tensor on their device, bit for bit (``pgdvs_percentile_f32``;
    include/pgdvs_hip.h): an exact radix select of the two neighbouring ranks and NumPy's ``_lerp``; any NaN in a frame gives NaN.
    Launches only: the caller's one ``.cpu()`` is the batch's one wait."""
    frames = [_req(f, torch.float32, "frames").reshape(-1) for f in frames]
    if not frames or any(f.numel() < 1 for f in frames) or any(f.device != frames[0].device for f in frames):
        raise ValueError("percentile_f32: at least one frame, each with at least one value, all on one GPU")
    if type(q) not in (int, float) or not 0 <= q <= 100:
        raise ValueError(f"percentile_f32: q must be a Python number in 0 .. 100 (NumPy forms q / 100 in the array's type then), got {q!r}")
    n, device = len(frames), frames[0].device
    lib = _lib.load()
    counts = (C.c_int64 * n)(*[f.numel() for f in frames])
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    with torch.cuda.device(device):
        ws = _ws(lib.pgdvs_percentile_f32_workspace_bytes(counts, n), device)
        out = torch.empty(n, dtype=torch.float32, device=device)
        check(lib.pgdvs_percentile_f32(ptrs, counts, n, float(q), _ptr(out), _ptr(ws), ws.numel(), _stream()), "pgdvs_percentile_f32")
    return out


def _flow_pair(a, b, names, what):
    """two float32 [H,W,2] GPU tensors of one shape, H, W >= 2 (the preprocessing ops' inputs)"""
    a, b = _req(a, torch.float32, names[0]), _req(b, torch.float32, names[1])
    if a.ndim != 3 or a.shape[2] != 2 or tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError(f"{what}: shapes {names[0]} {tuple(a.shape)}, {names[1]} {tuple(b.shape)} ([H,W,2] each, one device)")
    if a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError(f"{what}: H, W >= 2 expected, got {tuple(a.shape)}")
    return a, b


def flow_consistency(flow12, flow21):
    """Forward-backward flow consistency (``pgdvs_flow_consistency``; include/pgdvs_hip.h): flow12[H,W,2] and flow21[H,W,2]
    float32 on the GPU -> (coord_diff_1, coord_diff_2), float32 [H,W,2] on the GPU, the ``coord_diff`` entries of
    ``<a>_<b>.npz`` and ``<b>_<a>.npz``; both directions in one launch."""
    a, b = _flow_pair(flow12, flow21, ("flow12", "flow21"), "flow_consistency")
    H, W = int(a.shape[0]), int(a.shape[1])
    cd1, cd2 = torch.empty_like(a), torch.empty_like(a)
    check(_lib.load().pgdvs_flow_consistency(_ptr(a), _ptr(b), H, W, _ptr(cd1), _ptr(cd2), _stream()), "pgdvs_flow_consistency")
    return cd1, cd2


def flow_tile_blend(tiles, origins, weight, H, W):
    """FlowFormer's tiled inference after the network (``pgdvs_flow_tile_blend``; include/pgdvs_hip.h): tiles[n,2,ph,pw]
    float32 on the GPU, planar as the network returns them, ``origins`` the n host pairs (h, w) in upstream's order,
    weight[ph,pw] float32 on the GPU -> flow[H,W,2] float32 on the GPU: per pixel the weighted mean of the tiles that cover
    it, accumulated in tile order.  One launch."""
    t, w = _req(tiles, torch.float32, "tiles"), _req(weight, torch.float32, "weight")
    org = np.ascontiguousarray(np.asarray(origins), dtype=np.int32)
    if t.ndim != 4 or t.shape[1] != 2 or tuple(w.shape) != tuple(t.shape[2:]) or org.shape != (t.shape[0], 2) or t.device != w.device:
        raise ValueError(f"flow_tile_blend: shapes tiles {tuple(t.shape)}, weight {tuple(w.shape)}, origins {org.shape} "
                         "([n,2,ph,pw], [ph,pw] and [n,2], one device)")
    n, _, ph, pw = (int(v) for v in t.shape)
    H, W = int(H), int(W)
    out = torch.empty((max(H, 0), max(W, 0), 2), dtype=torch.float32, device=t.device)
    check(_lib.load().pgdvs_flow_tile_blend(_ptr(t), org.ctypes.data_as(C.c_void_p), n, ph, pw, _ptr(w), H, W, _ptr(out), _stream()),
          "pgdvs_flow_tile_blend")
    return out


def _flow_export(a, b, H, W, adaptive, cd1, cd2, out, what):
    shape = (1 if b is None else 2, H, 1 + 3 * W)
    out = _out(out, shape, torch.uint8, a.device, f"{what}: out", flat=True)
    lib = _lib.load()
    ws = _ws(lib.pgdvs_flow_pair_export_workspace_bytes(H, W), a.device)
    rad_max = torch.empty((shape[0],), dtype=torch.float32, device=a.device)
    check(lib.pgdvs_flow_pair_export(_ptr(a), _ptr(b), H, W, 1 if adaptive else 0, _ptr(cd1), _ptr(cd2), _ptr(rad_max), _ptr(out),
                                     _ptr(ws), ws.numel(), _stream()), "pgdvs_flow_pair_export")
    return rad_max, out.view(shape)


def flow_pair_export(flow12, flow21, adaptive=True, out=None):
    """Everything the flow stage derives from a pair's flows (``pgdvs_flow_pair_export``; include/pgdvs_hip.h): flow12[H,W,2]
    and flow21[H,W,2] float32 on the GPU -> (coord_diff_1, coord_diff_2, rad_max[2], scanlines[2,H,1+3W] uint8), all on the
    GPU: ``flow_consistency``'s values, the largest flow radius of each frame, and the PNG scanlines of the two colour-wheel
    pictures (``adaptive`` as in ``png_scanlines``), ready for ``png.PngWriter``.  Two launches.  ``out``: a contiguous uint8
    GPU tensor of 2 H (1 + 3 W) elements to fill in place (any alignment)."""
    a, b = _flow_pair(flow12, flow21, ("flow12", "flow21"), "flow_pair_export")
    H, W = int(a.shape[0]), int(a.shape[1])
    cd1, cd2 = torch.empty_like(a), torch.empty_like(a)
    rad_max, out = _flow_export(a, b, H, W, adaptive, cd1, cd2, out, "flow_pair_export")
    return cd1, cd2, rad_max, out


def flow_image(flow, adaptive=False):
    """The colour-wheel picture of one flow (the pictures-alone call of ``pgdvs_flow_pair_export``): flow[H,W,2] float32 on
    the GPU -> (rad_max[1], scanlines[H,1+3W] uint8) on the GPU; with ``adaptive=False`` ``scanlines[:, 1:]`` is the packed
    [H,W,3] picture."""
    f = _req(flow, torch.float32, "flow")
    if f.ndim != 3 or f.shape[2] != 2 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"flow_image: flow [H,W,2] expected, got {tuple(f.shape)}")
    H, W = int(f.shape[0]), int(f.shape[1])
    rad_max, out = _flow_export(f, None, H, W, adaptive, None, None, None, "flow_image")
    return rad_max, out[0]


def epipolar_mask(flow, coord_diff, F, consist_thres=1.0, threshold=1.0, want_dist=False):
    """The ``flow_epi`` motion mask of one direction (``pgdvs_epipolar_mask``; include/pgdvs_hip.h): flow[H,W,2] and
    coord_diff[H,W,2] float32 on the GPU, the numpy float64 fundamental matrix ``F[3,3]`` (l_2 = F p_1) -> mask[H,W] uint8
    on the GPU: (epipolar distance x consistency > threshold) opened with ``disk(1)``.  ``want_dist``: returns
    (mask, e_dist[H,W] float64 on the GPU), the distance already multiplied by the consistency mask."""
    f, cd = _flow_pair(flow, coord_diff, ("flow", "coord_diff"), "epipolar_mask")
    H, W = int(f.shape[0]), int(f.shape[1])
    mat = _mat64(F, 9)
    mask = torch.empty((H, W), dtype=torch.uint8, device=f.device)
    dist = torch.empty((H, W), dtype=torch.float64, device=f.device) if want_dist else None
    check(_lib.load().pgdvs_epipolar_mask(_ptr(f), _ptr(cd), H, W, mat, float(consist_thres), float(threshold), _ptr(mask),
                                          _ptr(dist), _stream()), "pgdvs_epipolar_mask")
    return (mask, dist) if want_dist else mask


def zoe_sample(pred_depth, mask, pts3d, w2c, K):
    """The ZoeDepth stage's look-ups for one frame (``pgdvs_zoe_sample``; include/pgdvs_hip.h): pred_depth[H,W], mask[H,W]
    and pts3d[P,3] float32 on the GPU, the numpy float64 ``w2c[4,4]`` and ``K[3,3]`` -> (proj_pcl[3,n] float64,
    pcl_depth_mvs[n] float64, pcl_depth_pred[n] float32, index[n] int64) on the GPU, the kept points in ascending order.
    Reads the count back (one synchronisation)."""
    d = _req(pred_depth, torch.float32, "pred_depth")
    m = _req(mask, torch.float32, "mask")
    p = _req(pts3d, torch.float32, "pts3d")
    if d.ndim != 2 or tuple(m.shape) != tuple(d.shape) or p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError(f"zoe_sample: shapes pred_depth {tuple(d.shape)}, mask {tuple(m.shape)}, pts3d {tuple(p.shape)}")
    if d.shape[0] < 2 or d.shape[1] < 2:
        raise ValueError(f"zoe_sample: H, W >= 2 expected, got {tuple(d.shape)}")
    H, W, P = int(d.shape[0]), int(d.shape[1]), int(p.shape[0])
    lib = _lib.load()
    ws = _ws(lib.pgdvs_zoe_sample_workspace_bytes(H, W, P), d.device)
    proj = torch.empty((3, P), dtype=torch.float64, device=d.device)
    mvs = torch.empty((P,), dtype=torch.float64, device=d.device)
    pred = torch.empty((P,), dtype=torch.float32, device=d.device)
    index = torch.empty((P,), dtype=torch.int64, device=d.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=d.device)
    check(lib.pgdvs_zoe_sample(_ptr(d), _ptr(m), H, W, _ptr(p), P, _mat64(w2c, 16), _mat64(K, 9), _ptr(proj), _ptr(mvs), _ptr(pred),
                               _ptr(index), _ptr(cnt), _ptr(ws), ws.numel(), _stream()), "pgdvs_zoe_sample")
    n = checked_count(cnt, "pgdvs_zoe_sample")
    return proj[:, :n], mvs[:n], pred[:n], index[:n]


def _zoe_samples(pcl_depth_pred, pcl_depth_mvs, what):
    a, b = _req(pcl_depth_pred, torch.float32, "pcl_depth_pred").reshape(-1), _req(pcl_depth_mvs, torch.float64, "pcl_depth_mvs").reshape(-1)
    if a.numel() != b.numel() or a.numel() < 1:
        raise ValueError(f"{what}: {a.numel()} predicted and {b.numel()} MVS depths (one each per sample, at least one)")
    return a, b


def zoe_fit(pcl_depth_pred, pcl_depth_mvs):
    """The disparity-domain scale and shift of one frame (``pgdvs_zoe_fit``; include/pgdvs_hip.h): pcl_depth_pred[n]
    float32 and pcl_depth_mvs[n] float64 on the GPU -> (fit[4] float64: scale_med, shift_med, scale_trim, shift_trim;
    flag_trim[n] bool; status[1] int32: bit 0 a negative prediction, bit 1 a negative MVS depth), all on the GPU."""
    a, b = _zoe_samples(pcl_depth_pred, pcl_depth_mvs, "zoe_fit")
    n = a.numel()
    lib = _lib.load()
    ws = _ws(lib.pgdvs_zoe_fit_workspace_bytes(n), a.device)
    fit = torch.empty((4,), dtype=torch.float64, device=a.device)
    flag = torch.empty((n,), dtype=torch.uint8, device=a.device)
    status = torch.empty((1,), dtype=torch.int32, device=a.device)
    check(lib.pgdvs_zoe_fit(_ptr(a), _ptr(b), n, _ptr(fit), _ptr(flag), _ptr(status), _ptr(ws), ws.numel(), _stream()), "pgdvs_zoe_fit")
    return fit, flag.view(torch.bool), status


def zoe_errors(pcl_depth_pred, pcl_depth_mvs, flag_trim, scale_shift):
    """The error table of one frame (``pgdvs_zoe_errors``; include/pgdvs_hip.h): the samples and flag_trim[n] (bool or
    uint8) on the GPU, the numpy float64 ``scale_shift[4,2]`` of med_share, med_indiv, trim_share, trim_indiv ->
    errors[8] float64 on the GPU: the four mean absolute errors, then the four mean errors."""
    a, b = _zoe_samples(pcl_depth_pred, pcl_depth_mvs, "zoe_errors")
    if not isinstance(flag_trim, torch.Tensor) or not flag_trim.is_cuda:
        raise PgdvsHipError("flag_trim: expected a GPU tensor (no CPU fallback)")
    f = flag_trim.reshape(-1).contiguous()
    f = f.view(torch.uint8) if f.dtype == torch.bool else _req(f, torch.uint8, "flag_trim")
    if f.numel() != a.numel():
        raise ValueError(f"zoe_errors: flag_trim has {f.numel()} entries for {a.numel()} samples")
    out = torch.empty((8,), dtype=torch.float64, device=a.device)
    check(_lib.load().pgdvs_zoe_errors(_ptr(a), _ptr(b), _ptr(f), a.numel(), _mat64(scale_shift, 8), _ptr(out), _stream()),
          "pgdvs_zoe_errors")
    return out


def _mask8(t, name):
    """a bool or uint8 GPU tensor as contiguous uint8 (bool reinterpreted, not copied)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PgdvsHipError(f"{name}: expected a GPU tensor (no CPU fallback)")
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else _req(t, torch.uint8, name)


def semantic_mask(sem_ade20k, sem_coco, ids_ade20k, ids_coco):
    """The semantic raw mask (``pgdvs_semantic_mask``; include/pgdvs_hip.h): the two int64 class-id maps [H,W] on the GPU
    (ids counted from 0, -1 for none) and the two Python lists of dynamic classes counted from 1 -> (ade20k, coco, sem)
    uint8 [H,W] on the GPU."""
    a, b = _req(sem_ade20k, torch.int64, "sem_ade20k"), _req(sem_coco, torch.int64, "sem_coco")
    if a.ndim != 2 or tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError(f"semantic_mask: shapes sem_ade20k {tuple(a.shape)}, sem_coco {tuple(b.shape)} ([H,W] each, one device)")
    H, W = int(a.shape[0]), int(a.shape[1])
    la, lb = [int(v) for v in ids_ade20k], [int(v) for v in ids_coco]
    out = [torch.empty((H, W), dtype=torch.uint8, device=a.device) for _ in range(3)]
    check(_lib.load().pgdvs_semantic_mask(_ptr(a), _ptr(b), H, W, (C.c_int32 * len(la))(*la), len(la), (C.c_int32 * len(lb))(*lb),
                                          len(lb), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()), "pgdvs_semantic_mask")
    return tuple(out)


def mask_combine(raw_no_warp, sam, prev_mask=None, prev_cnt=None, bwd_flow=None, bwd_coord_diff=None, *, img_idx,
                 dyn_track_thres=0.5, sam_overlap_thres=0.1, table=None, want_segments=False):
    """The final motion mask of one frame (``pgdvs_mask_combine``; include/pgdvs_hip.h): raw_no_warp[H,W] and
    sam[n_seg,H,W] (bool or uint8, n_seg >= 0) on the GPU and, from the second frame on, the previous call's ``next_prev``
    and ``dyn_cnt`` with bwd_flow[H,W,2] and bwd_coord_diff[H,W,2] float32 -> a dict of GPU tensors: warp_prev, dyn_track
    (None on the first frame), raw_no_warp, raw, raw_eroded, final_raw, final, next_prev as uint8 0 / 1 and dyn_cnt float32;
    with ``want_segments`` also seg_counts[n_seg,2] int32 (n_pix, n_overlap) and seg_selected[n_seg] uint8.  ``table``: the
    warp's float32 [32,4] weights, ``preprocess.final_mask.cubic_table()`` by default.  One C call, nothing read back."""
    r = _mask8(raw_no_warp, "raw_no_warp")
    s = _mask8(sam, "sam")
    if r.ndim != 2 or s.ndim != 3 or tuple(s.shape[1:]) != tuple(r.shape) or s.device != r.device:
        raise ValueError(f"mask_combine: shapes raw_no_warp {tuple(r.shape)}, sam {tuple(s.shape)} ([H,W] and [n_seg,H,W], one device)")
    H, W, n_seg = int(r.shape[0]), int(r.shape[1]), int(s.shape[0])
    prev = (prev_mask, prev_cnt, bwd_flow, bwd_coord_diff)
    has_prev = prev_mask is not None
    if any((t is not None) != has_prev for t in prev):
        raise ValueError("mask_combine: prev_mask, prev_cnt, bwd_flow and bwd_coord_diff go together")
    tab = None
    if has_prev:
        pm, pc = _mask8(prev_mask, "prev_mask"), _req(prev_cnt, torch.float32, "prev_cnt")
        fl, cd = _req(bwd_flow, torch.float32, "bwd_flow"), _req(bwd_coord_diff, torch.float32, "bwd_coord_diff")
        if tuple(pm.shape) != (H, W) or tuple(pc.shape) != (H, W) or tuple(fl.shape) != (H, W, 2) or tuple(cd.shape) != (H, W, 2):
            raise ValueError(f"mask_combine: shapes prev_mask {tuple(pm.shape)}, prev_cnt {tuple(pc.shape)}, bwd_flow {tuple(fl.shape)}, "
                             f"bwd_coord_diff {tuple(cd.shape)} for a {(H, W)} frame")
        if table is None:
            from .preprocess.final_mask import cubic_table

            table = cubic_table()
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.shape != (32, 4):
            raise ValueError(f"mask_combine: table {table.shape}, expected (32, 4)")
        tab = (C.c_float * 128)(*table.reshape(-1).tolist())
    else:
        pm = pc = fl = cd = None
    lib = _lib.load()
    ws = _ws(lib.pgdvs_mask_combine_workspace_bytes(H, W, n_seg), r.device)
    u8 = lambda: torch.empty((H, W), dtype=torch.uint8, device=r.device)  # noqa: E731
    out = dict(warp_prev=u8() if has_prev else None, dyn_track=u8() if has_prev else None,
               dyn_cnt=torch.empty((H, W), dtype=torch.float32, device=r.device), raw_no_warp=r, raw=u8(), raw_eroded=u8(),
               final_raw=u8(), final=u8(), next_prev=u8())
    counts = torch.empty((n_seg, 2), dtype=torch.int32, device=r.device) if want_segments else None
    selected = torch.empty((n_seg,), dtype=torch.uint8, device=r.device) if want_segments else None
    check(lib.pgdvs_mask_combine(_ptr(r), _ptr(s) if n_seg else None, n_seg, H, W, _ptr(pm), _ptr(pc), _ptr(fl), _ptr(cd), tab,
                                 int(img_idx), float(dyn_track_thres), float(sam_overlap_thres), _ptr(out["warp_prev"]),
                                 _ptr(out["dyn_track"]), _ptr(out["dyn_cnt"]), _ptr(out["raw"]), _ptr(out["raw_eroded"]),
                                 _ptr(out["final_raw"]), _ptr(out["final"]), _ptr(out["next_prev"]),
                                 _ptr(counts) if n_seg else None, _ptr(selected) if n_seg else None, _ptr(ws), ws.numel(), _stream()),
          "pgdvs_mask_combine")
    if want_segments:
        out.update(seg_counts=counts, seg_selected=selected)
    return out


PNG_QUANT = {"save_image": 0, "truncate": 1}


def png_scanlines(img, *, quant="save_image", adaptive=True, out=None):
    """The visualiser's image export up to the deflate (``pgdvs_png_scanlines``; include/pgdvs_hip.h): img[B,3,H,W] (or
    [3,H,W]) float32 on the GPU, unclamped -> uint8 [B,H,1+3W]: per row a PNG filter-type byte, then the row's R G B bytes
    quantised as ``quant`` says ("save_image": ``torchvision.utils.save_image``; "truncate": the ``*_gnt.png`` cast; both after
    ``clamp(0, 1)``, NaN -> 0) and filtered (``adaptive``: libpng's default per-row choice among the five filter types;
    otherwise type 0, so ``out[..., 1:]`` is the packed [H,W,3] image).  ``out``: a contiguous uint8 GPU tensor of
    B H (1 + 3 W) elements to fill in place (any alignment)."""
    if quant not in PNG_QUANT:
        raise ValueError(f"png_scanlines: quant {quant!r} (one of {sorted(PNG_QUANT)})")
    x, B, H, W = _planar_batch(img, "png_scanlines")
    shape = (B, H, 1 + 3 * W)
    out = _out(out, shape, torch.uint8, x.device, "png_scanlines: out", flat=True)
    check(_lib.load().pgdvs_png_scanlines(_ptr(x), B, H, W, PNG_QUANT[quant], 1 if adaptive else 0, _ptr(out), _stream()),
          "pgdvs_png_scanlines")
    return out.view(shape)


# the step of csrc/png_deflate.hip: a workgroup tokenises PNG_DEFLATE_PAYLOAD bytes at a time out of a window of
# PNG_DEFLATE_WINDOW (the rest is look-ahead), a thread owns PNG_DEFLATE_PER consecutive bytes, a wavefront 64 of those
PNG_DEFLATE_PER = 16
PNG_DEFLATE_WINDOW = 4096
PNG_DEFLATE_HALO = 272
PNG_DEFLATE_PAYLOAD = PNG_DEFLATE_WINDOW - PNG_DEFLATE_HALO


def png_deflate_capacity(img_bytes: int, seg_bytes=None) -> int:
    """The bytes an image's stream can take at most (an ``out_stride`` of ``pgdvs_png_deflate`` that always fits): 15 bits
    per input byte, 160 bytes of header and flush per segment, 8 for the stream's head and tail (``png.deflate_capacity``)."""
    from . import png

    return png.deflate_capacity(img_bytes, seg_bytes)


def png_deflate(scanlines, seg_bytes=None, out=None):
    """The deflate of the PNG export on the device (``pgdvs_png_deflate``; include/pgdvs_hip.h): scanlines uint8 [n,H,L] or
    [n,nbytes] on the GPU (any bytes) -> (data uint8 [n,stride], nbytes int32 [n]) on the GPU: ``data[i, :nbytes[i]]`` is image
    i's zlib stream, byte for byte ``png.deflate_rle``; the rest of a row is not written.  ``seg_bytes``: a power of two in
    4096 .. 65536, None for ``png.DEFLATE_SEG_DEFAULT``.  ``out``: a contiguous uint8 GPU tensor [n,stride] to fill in place;
    an image whose stream does not fit ``stride`` gets ``nbytes = -1`` and an untouched row (``png_deflate_capacity`` always
    fits).  Runs on the current stream; nothing synchronises."""
    from . import png

    if not isinstance(scanlines, torch.Tensor) or not scanlines.is_cuda:
        raise PgdvsHipError("png_deflate: scanlines must be a GPU tensor (the host path is png.deflate_rle)")
    if scanlines.dtype != torch.uint8 or scanlines.ndim not in (2, 3) or scanlines.shape[0] < 1 or scanlines[0].numel() < 1:
        raise ValueError(f"png_deflate: uint8 [n,H,L] or [n,nbytes] expected, got {scanlines.dtype} {tuple(scanlines.shape)}")
    x = scanlines.contiguous()
    n, img_bytes = int(x.shape[0]), int(x[0].numel())
    seg = png.check_seg_bytes(seg_bytes)
    out = _out(out, (n, png.deflate_capacity(img_bytes, seg)), torch.uint8, x.device, "png_deflate: out", at_least=1,
               shown=f"tensor [{n}, stride]")
    lib = _lib.load()
    ws = _ws(lib.pgdvs_png_deflate_workspace_bytes(n, img_bytes, seg), x.device)
    nbytes = torch.empty((n,), dtype=torch.int32, device=x.device)
    check(lib.pgdvs_png_deflate(_ptr(x), n, img_bytes, seg, _ptr(out), int(out.shape[1]), _ptr(nbytes), _ptr(ws), ws.numel(), _stream()),
          "pgdvs_png_deflate")
    return out, nbytes


def _quant_ptr(table, name):
    t = np.ascontiguousarray(np.asarray(table).reshape(-1), dtype=np.int64)
    if t.shape != (64,) or t.min() < 1 or t.max() > 255:
        raise ValueError(f"{name}: a quantisation table of 64 entries in 1 .. 255 expected")
    return (C.c_uint16 * 64)(*t.tolist())


def jpeg_coefficients(img, quality=90, out=None, subsampling="4:4:4"):
    """The first half of a video frame's compression (``pgdvs_jpeg_coefficients``; include/pgdvs_hip.h): img[B,3,H,W] (or
    [3,H,W]) float32 on the GPU, unclamped -> int16 [B,nby,nbx,3,64]: per 8 x 8 block the quantised DCT coefficients of Y, Cb
    and Cr in zigzag order, bit for bit ``video.jpeg_coefficients`` of the image quantised as ``*_combined.png`` is.
    ``quality``: libjpeg's 1 .. 100 (``video.quant_tables``), or a pair of tables in natural order.
    ``subsampling="4:2:0"`` (``pgdvs_jpeg_coefficients_420``): int16 [B,nmy,nmx,6,64] over 16 x 16 MCUs, blocks Y00, Y01, Y10,
    Y11, Cb, Cr, with libjpeg's chroma averaging, edge rules and dummy blocks."""
    from . import video

    video.check_subsampling(subsampling)
    x, B, H, W = _planar_batch(img, "jpeg_coefficients")
    if H < 1 or W < 1:
        raise ValueError(f"jpeg_coefficients: img [B,3,H,W] expected, got {tuple(x.shape)}")
    luma, chroma = video.quant_tables(quality) if np.isscalar(quality) else quality
    shape = (B, *video.mcu_grid(H, W, subsampling), video.BLOCKS_PER_MCU[subsampling], 64)
    out = _out(out, shape, torch.int16, x.device, "jpeg_coefficients: out")
    name = "pgdvs_jpeg_coefficients" if subsampling == "4:4:4" else "pgdvs_jpeg_coefficients_420"
    check(getattr(_lib.load(), name)(_ptr(x), B, H, W, _quant_ptr(luma, "jpeg_coefficients"), _quant_ptr(chroma, "jpeg_coefficients"),
                                     _ptr(out), _stream()), name)
    return out


def jpeg_scan_capacity(nby: int, nbx: int, restart_mcus: int, blocks_per_mcu: int = 3) -> int:
    """The bytes a frame's scan data can take at most (the least ``out_stride`` of ``pgdvs_jpeg_scan``): 1248 per MCU -- a
    block costs at most 1658 bits = 208 bytes, doubled by stuffing -- plus 2 per restart marker.  ``blocks_per_mcu=6``: the
    4:2:0 layout (``nby``, ``nbx`` its MCU grid), 2496 per MCU."""
    if blocks_per_mcu not in (3, 6):
        raise ValueError(f"jpeg_scan_capacity: blocks_per_mcu {blocks_per_mcu} (3 or 6)")
    n_mcu = int(nby) * int(nbx)
    seg = max(1, min(int(restart_mcus), n_mcu))
    return 416 * blocks_per_mcu * n_mcu + 2 * ((n_mcu + seg - 1) // seg - 1)


def jpeg_scan(coef, restart_mcus=None, out=None):
    """The second half (``pgdvs_jpeg_scan``; include/pgdvs_hip.h): coef[B,nby,nbx,3,64] (or [nby,nbx,3,64]) int16 on the GPU, or
    the 4:2:0 layout [B,nmy,nmx,6,64] (recognised by ``coef.shape[-2]``; ``pgdvs_jpeg_scan_420``, MCUs of 16 x 16 pixels) ->
    (data uint8 [B,stride], nbytes int32 [B]) on the GPU: ``data[b, :nbytes[b]]`` is frame b's entropy-coded scan, byte for
    byte ``video.encode_scan``; the rest of a row is not written.  ``restart_mcus``: MCUs per restart interval, None for one
    MCU row; 0 (no restart markers) is host-only and refused.  ``out``: a contiguous uint8 GPU tensor [B,stride] with
    stride >= ``jpeg_scan_capacity(nby, nbx, restart_mcus, coef.shape[-2])`` to fill in place.  Nothing synchronises."""
    if not isinstance(coef, torch.Tensor) or not coef.is_cuda:
        raise PgdvsHipError("jpeg_scan: coef must be a GPU tensor (the host path is video.encode_scan)")
    if coef.dtype != torch.int16:
        raise ValueError(f"jpeg_scan: int16 coefficients expected, got {coef.dtype}")
    c = coef.contiguous()
    if c.ndim == 4:
        c = c[None]
    if c.ndim != 5 or tuple(c.shape[3:]) not in ((3, 64), (6, 64)) or c.shape[0] < 1 or c.shape[1] < 1 or c.shape[2] < 1:
        raise ValueError(f"jpeg_scan: coef [B,nby,nbx,3,64] or [B,nmy,nmx,6,64] expected, got {tuple(coef.shape)}")
    B, nby, nbx, bpm = (int(v) for v in c.shape[:4])
    name = "pgdvs_jpeg_scan" if bpm == 3 else "pgdvs_jpeg_scan_420"
    R = nbx if restart_mcus is None else int(restart_mcus)
    if R == 0:
        raise PgdvsHipError("jpeg_scan: restart_mcus 0 (no restart markers) is host-only (video.encode_scan); the device pass "
                            "needs restart_mcus >= 1")
    if not 1 <= R <= 65535:
        raise ValueError(f"jpeg_scan: restart_mcus {restart_mcus} (1 .. 65535)")
    cap = jpeg_scan_capacity(nby, nbx, R, bpm)
    out = _out(out, (B, cap), torch.uint8, c.device, "jpeg_scan: out", at_least=cap)
    lib = _lib.load()
    ws = _ws(getattr(lib, name + "_workspace_bytes")(B, nby, nbx, R), c.device)
    nbytes = torch.empty((B,), dtype=torch.int32, device=c.device)
    check(getattr(lib, name)(_ptr(c), B, nby, nbx, R, _ptr(out), int(out.shape[1]), _ptr(nbytes), _ptr(ws), ws.numel(), _stream()), name)
    return out, nbytes


def jpeg_encode(img, quality=90, restart_mcus=None, subsampling="4:4:4"):
    """``jpeg_coefficients`` then ``jpeg_scan``: img[B,3,H,W] (or [3,H,W]) float32 on the GPU -> (data [B,stride], nbytes [B]);
    ``video.jpeg_frame(data[b, :nbytes[b]], H, W, quality, restart_mcus, subsampling)`` is frame b's JPEG file, the bytes of
    ``video.encode_jpeg`` on the same image."""
    return jpeg_scan(jpeg_coefficients(img, quality, subsampling=subsampling), restart_mcus)


def eval_export_scanlines(pred, gt_hwc, static=None, adaptive=True, out=None):
    """The evaluator's per-view image export up to the deflate in one launch (``pgdvs_eval_export_scanlines``;
    include/pgdvs_hip.h): pred[3,H,W] raw render, gt_hwc[H,W,3] raw ground truth and, given, static[3,H,W] (the renderer's
    ``static_coarse_rgb`` or ``geo_static_rgb``), float32 on the GPU -> uint8 [n,H,1+3W] with n = 2 or 3 in the order gt, pred,
    static: each image's PNG scanlines under the truncating cast (``png_scanlines(quant="truncate")``'s bytes).  ``out``: a
    contiguous uint8 GPU tensor of n H (1 + 3 W) elements to fill in place (any alignment)."""
    p = _req(pred, torch.float32, "pred")
    g = _req(gt_hwc, torch.float32, "gt")
    s_ = _req(static, torch.float32, "static") if static is not None else None
    if p.ndim != 3 or p.shape[0] != 3 or g.ndim != 3 or tuple(g.shape) != (p.shape[1], p.shape[2], 3) or (
            s_ is not None and tuple(s_.shape) != tuple(p.shape)):
        raise ValueError(f"eval_export_scanlines: pred [3,H,W], gt [H,W,3] and static [3,H,W] expected, got {tuple(p.shape)}, "
                         f"{tuple(g.shape)}, {tuple(s_.shape) if s_ is not None else None}")
    H, W = int(p.shape[1]), int(p.shape[2])
    shape = (3 if s_ is not None else 2, H, 1 + 3 * W)
    out = _out(out, shape, torch.uint8, p.device, "eval_export_scanlines: out", flat=True)
    check(_lib.load().pgdvs_eval_export_scanlines(_ptr(p), _ptr(g), _ptr(s_), H, W, 1 if adaptive else 0, _ptr(out), _stream()),
          "pgdvs_eval_export_scanlines")
    return out.view(shape)


class RowRing:
    """Pinned staging for metric rows (8 float64 each) read back behind the GPU: ``depth`` row blocks, each with its own event,
    so that up to ``depth`` steps' rows can be on their way at once.  ``enqueue(rows)`` copies [n] device rows
    asynchronously on the current stream into the next block and records its event -> a ticket; ``finish(ticket)`` waits
    for that block's event alone -> [n][8] Python floats.  Tickets are finished in the order they were taken, each before
    its block comes round again (``depth`` enqueues later)."""

    def __init__(self, depth: int = 1):
        self.depth = int(depth)
        self._blocks = [None] * self.depth
        self._next = 0

    def enqueue(self, rows):
        n = len(rows)
        slot = self._next
        self._next = (slot + 1) % self.depth
        ent = self._blocks[slot]
        if ent is None or ent[0].shape[0] < n:
            ent = self._blocks[slot] = (torch.empty((max(n, 8), 8), dtype=torch.float64).pin_memory(), torch.cuda.Event())
        host, ev = ent
        for i, r_ in enumerate(rows):
            host[i].copy_(r_, non_blocking=True)
        ev.record()
        return slot, n

    def finish(self, ticket):
        slot, n = ticket
        host, ev = self._blocks[slot]
        ev.synchronize()
        return host[:n].tolist()


_row_rings = {}


def row_ring(device, depth: int = 1) -> RowRing:
    """the cached ``RowRing`` of ``depth`` blocks for ``device`` (pinning host memory is slow; one ring per device and depth)"""
    key = (torch.device(device).index, int(depth))
    ring = _row_rings.get(key)
    if ring is None:
        ring = _row_rings[key] = RowRing(depth)
    return ring


def read_back_rows(rows):
    """[n] device tensors of 8 float64 each -> [n][8] Python floats, through the device's cached one-block ``RowRing``:
    asynchronous copies on the current stream and one event wait, instead of a pageable `.cpu()` per step (which stages
    through a fresh host block and synchronises the whole stream)."""
    ring = row_ring(rows[0].device, 1)
    return ring.finish(ring.enqueue(rows))


def checked_count(cnt, what: str) -> int:
    """Host read of a device-side count that doubles as a status word: negative = the kernel chain
    reported an internal error (e.g. ``agg_select``'s ordered-offset look-back gave up) and its
    output must not be used."""
    n = int(cnt.item())
    if n < 0:
        raise PgdvsHipError(f"{what}: device-side error flag set (count {n}); the output is not valid")
    return n


def combine(static_rgb, dyn_rgb, dyn_mask):
    """[B,3,H,W], [B,3,H,W], [B,1,H,W] -> combined, combined_static, combined_dyn."""
    st = _req(static_rgb, torch.float32, "static_rgb")
    dy = _req(dyn_rgb, torch.float32, "dyn_rgb")
    mk = _req(dyn_mask, torch.float32, "dyn_mask")
    B, _, H, W = st.shape
    outs = [torch.empty_like(st) for _ in range(3)]
    lib = _lib.load()
    for b in range(B):
        check(lib.pgdvs_combine(_ptr(st[b]), _ptr(dy[b]), _ptr(mk[b]), H * W, _ptr(outs[0][b]), _ptr(outs[1][b]),
                                _ptr(outs[2][b]), _stream()), "pgdvs_combine")
    return outs


def gnt_gather(ray_o, ray_d, depth_range, n_samples: int, inv_uniform: bool, cam_tgt, cams_src, src_rgbs, featmaps_cl,
               inv_masks=None, z_samples=None):
    """A13.  ray_o/ray_d[R,3], depth_range[1,2] or [R,2], cams_src[V,80], src_rgbs[V,H,W,3],
    featmaps_cl[V,hf,wf,C], inv_masks[V,H,W] or None -> dict of [R,S,V,*] tensors."""
    ro, rd = _req(ray_o, torch.float32, "ray_o"), _req(ray_d, torch.float32, "ray_d")
    dr = _req(depth_range, torch.float32, "depth_range").reshape(-1, 2)
    R, S = ro.shape[0], int(n_samples)
    zs = None
    if z_samples is not None:  # explicit sample depths [R,S] (fine pass)
        zs = _req(z_samples, torch.float32, "z_samples")
        assert tuple(zs.shape) == (R, S), (zs.shape, R, S)
    img = _req(src_rgbs, torch.float32, "src_rgbs")
    V, H, W, _ = img.shape
    fm = _req(featmaps_cl, torch.float32, "featmaps_cl")
    hf, wf, Cc = fm.shape[1], fm.shape[2], fm.shape[3]
    per_ray = dr.shape[0] != 1
    assert dr.shape[0] in (1, R), dr.shape
    im = _req(inv_masks, torch.float32, "inv_masks").reshape(V, H, W) if inv_masks is not None else None
    dev = ro.device
    e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    out = {"pts": e(R, S, 3), "z_vals": e(R, S), "rgb_feat": e(R, S, V, 3 + Cc), "ray_diff": e(R, S, V, 4),
           "mask_inbound": e(R, S, V, 1), "mask_invalid": e(R, S, V, 1), "mask": e(R, S, V, 1)}
    ct, cs = _req(cam_tgt, torch.float32, "cam_tgt"), _req(cams_src, torch.float32, "cams_src")
    check(_lib.load().pgdvs_gnt_gather(
        _ptr(ro), _ptr(rd), _ptr(dr), int(per_ray), _ptr(zs), R, S, int(bool(inv_uniform)), _ptr(ct), _ptr(cs), V, _ptr(img), H, W,
        _ptr(fm), hf, wf, Cc, _ptr(im), _ptr(out["pts"]), _ptr(out["z_vals"]), _ptr(out["rgb_feat"]), _ptr(out["ray_diff"]),
        _ptr(out["mask_inbound"]), _ptr(out["mask_invalid"]), _ptr(out["mask"]), _stream()), "pgdvs_gnt_gather")
    if im is None:
        out["mask_invalid"].zero_()
    return out


# ---- CoTracker's correlation step (csrc/cotracker.hip) ------------------------------------
class CotrackerPyramid:
    """The four channels-last levels of ``CorrBlock.__init__`` in one device buffer (``ops.cotracker_pyramid``)."""

    def __init__(self, buf, S, H, W):
        self.buf, self.S, self.H, self.W = buf, S, H, W

    def level(self, i):
        """level ``i`` as a [S, H >> i, W >> i, 128] view (tests, diagnostics)"""
        off = 0
        for k in range(i):
            n = self.S * (self.H >> k) * (self.W >> k) * 128 * 4
            off += (n + 255) // 256 * 256
        h, w = self.H >> i, self.W >> i
        return self.buf[off:off + self.S * h * w * 512].view(torch.float32).view(self.S, h, w, 128)


def cotracker_pyramid(fmaps, reject_ok: bool = False):
    """fmaps[S,128,H,W] -> the pyramid ``cotracker_corr_lookup`` reads.  A shape the kernels do not cover (C != 128, a level
    below 2 x 2) raises PgdvsHipError, or returns None with ``reject_ok`` (the caller then runs its torch statement)."""
    fm = _req(fmaps, torch.float32, "fmaps")
    assert fm.ndim == 4, fm.shape
    S, Cc, H, W = fm.shape
    lib = _lib.load()
    nbytes = lib.pgdvs_cotracker_pyramid_workspace_bytes(S, Cc, H, W)
    if nbytes < 0 and reject_ok:
        return None
    ws = _ws(nbytes, fm.device)
    check(lib.pgdvs_cotracker_pyramid(_ptr(fm), S, Cc, H, W, _ptr(ws), ws.numel(), _stream()), "pgdvs_cotracker_pyramid")
    return CotrackerPyramid(ws, S, H, W)


def cotracker_corr_lookup(pyramid: CotrackerPyramid, feats, coords, out=None, col_offset: int = 0):
    """``CorrBlock.corr(feats)`` + ``CorrBlock.sample(coords)``: feats[S,N,128], coords[S,N,2] (x, y) -> [S,N,196].  With
    ``out`` [S,N,width] (float32, contiguous) the 196 values of a row land at ``col_offset`` and the other columns stay."""
    ft, cd = _req(feats, torch.float32, "feats"), _req(coords, torch.float32, "coords")
    S, N = ft.shape[0], ft.shape[1]
    assert ft.shape == (S, N, 128) and cd.shape == (S, N, 2) and S == pyramid.S, (ft.shape, cd.shape, pyramid.S)
    if out is None:
        out = torch.empty((S, N, 196), dtype=torch.float32, device=ft.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape[:2] == (S, N), (out.shape, out.dtype)
    check(_lib.load().pgdvs_cotracker_corr_lookup(_ptr(pyramid.buf), S, pyramid.H, pyramid.W, _ptr(ft), _ptr(cd), N, _ptr(out),
                                                  out.shape[2], int(col_offset), _stream()), "pgdvs_cotracker_corr_lookup")
    return out


# ---- packed-weight caches of the fused GNT kernels ---------------------------------------
def _param_key(*modules):
    """(storage address, in-place version) of every parameter: changes on `.to(device)`, on
    `load_state_dict` (in-place copies bump `_version`) and on optimiser steps."""
    return tuple((p.data_ptr(), p._version) for m in modules for p in m.parameters())


def _packed(owner, build, *modules):
    """Packed copy of `modules`' parameters cached on `owner`, rebuilt whenever a parameter was moved or
    written since it was packed (a checkpoint loaded after a warm-up forward must not keep the old weights)."""
    key = _param_key(*(modules or (owner,)))
    hit = getattr(owner, "_pgdvs_packed", None)
    if hit is None or hit[0] != key:
        hit = (key, build())
        object.__setattr__(owner, "_pgdvs_packed", hit)  # plain attribute: never a submodule / buffer / state_dict entry
    return hit[1]


def needs_autograd(*modules_and_tensors) -> bool:
    """The fused kernels return tensors without autograd history: they may run only when nobody can ask
    for gradients through them (inference under no_grad, or nothing on the path requires grad)."""
    if not torch.is_grad_enabled():
        return False
    for x in modules_and_tensors:
        if isinstance(x, torch.Tensor):
            if x.requires_grad:
                return True
        elif x is not None and any(p.requires_grad for p in x.parameters()):
            return True
    return False


_fallback_seen = set()


# ---------------------------------------------------------------- library options (include/pgdvs_hip.h, "Options")
def set_option(name: str, value) -> None:
    """process-wide option of the library (read from the environment once, at load time; this is the only other way to
    change one).  Names: agg_ordered, agg_stage, gnt_fp32, raster_bound_density, knn_no_tpq, knn_stats."""
    check(_lib.load().pgdvs_option_set(name.encode(), float(value)), f"pgdvs_option_set({name})")


def get_option(name: str) -> float:
    v = _lib.load().pgdvs_option_get(name.encode())
    if v != v:
        raise PgdvsHipError(f"pgdvs_option_get: unknown option '{name}'")
    return v


class option:
    """``with ops.option("agg_ordered", 1): ...`` -- sets a library option for the block and restores it (tests, bench.py)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.prev)
        return False


def gnt_product_path(fp32: bool):
    """the GNT kernels' product path for a block of code: exact bf16x3 products on the bf16 matrix instructions (default) or
    every product on the fp32 matrix instruction (csrc/gnt_view.hip)"""
    return option("gnt_fp32", 1 if fp32 else 0)


def gnt_fallback(kernel: str, why: str) -> None:
    """A CUDA tensor is about to take the torch branch of a GNT stage because the fused kernel does not
    cover its shape: say so once per (kernel, reason); raise instead under PGDVS_GNT_STRICT=1."""
    import os
    import warnings

    if not _GNT_VIEW_ENABLED:  # the fused kernels are switched off on purpose (tests: the torch statement as the reference half)
        return
    msg = f"pgdvs_amd: {kernel} does not cover {why}; this stage runs on torch/rocBLAS (results identical, slower)"
    if os.environ.get("PGDVS_GNT_STRICT", "0") not in ("", "0"):
        raise PgdvsHipError(msg)
    if (kernel, why) not in _fallback_seen:
        _fallback_seen.add((kernel, why))
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


# ---- GNT view-transformer contraction on MFMA (csrc/gnt_view.hip) ------------------------
def gnt_view_available(dim: int, n_views: int) -> bool:
    """True when the fused MFMA view-layer kernel handles this shape (width 64)."""
    lib = _lib.load()
    return hasattr(lib, "pgdvs_gnt_view_layer") and dim == 64 and 1 <= n_views <= 64 and _GNT_VIEW_ENABLED


_GNT_VIEW_ENABLED = True


def _featc(t):
    """csrc/gnt_view.hip featc: feature index of register t of a 32-row tile's lane (+ 4 h for the lane's half)"""
    return (t & 3) + 8 * ((t & 15) >> 2) + 32 * (t >> 4)


_ff_img_index = None


def ff_bf16x3_images(w1_t: torch.Tensor, w2_t: torch.Tensor) -> torch.Tensor:
    """The feed-forward block's weights (input-major ``w1_t[64, 256]``, ``w2_t[256, 64]``) as the lane-major bf16x3 images of
    ``gnt_ff_bf16x3_kernel`` (csrc/gnt_view.hip): every weight split EXACTLY into three bf16 pieces (hi = w & 0xffff0000,
    mid = (w - hi) & 0xffff0000, lo = w - hi - mid), arranged [half of the hidden units][piece][W1 part | W2 part], a part
    being [chunk][lane][8 bf16] in the order the MFMA's A operand takes them (see the kernel).  Returns float32[49152] (the
    bit patterns, two bf16 per word)."""
    global _ff_img_index
    import numpy as np

    if _ff_img_index is None:
        lane = np.arange(64)
        m, kg = lane & 31, lane >> 5
        j = np.arange(8)
        idx1 = np.zeros((2, 4, 4, 64, 8), np.int64)      # [half][mtl][c][lane][j] -> flat index into w1_t (in * 256 + hid)
        idx2 = np.zeros((2, 4, 2, 2, 64, 8), np.int64)   # [half][mtl][c'][ot][lane][j] -> flat index into w2_t (hid * 64 + out)
        for hf in range(2):
            for mtl in range(4):
                mt = 4 * hf + mtl
                for c in range(4):
                    t = 8 * c + j                                        # [8]
                    fin = _featc(t)[None, :] + 4 * kg[:, None]           # [64, 8]
                    idx1[hf, mtl, c] = fin * 256 + (32 * mt + m)[:, None]
                for c2 in range(2):
                    r = 8 * c2 + j
                    hid = ((r & 3) + 8 * (r >> 2))[None, :] + 4 * kg[:, None] + 32 * mt
                    for ot in range(2):
                        idx2[hf, mtl, c2, ot] = hid * 64 + (32 * ot + m)[:, None]
        _ff_img_index = (torch.from_numpy(idx1.reshape(2, -1)), torch.from_numpy(idx2.reshape(2, -1)))
    i1, i2 = (x_.to(w1_t.device) for x_ in _ff_img_index)

    def pieces(w):  # float32 [n] -> three int32 [n] holding the bf16 bit patterns (upper halves)
        w = w.detach().float().contiguous().reshape(-1)
        mask = torch.tensor(-65536, dtype=torch.int32, device=w.device)
        hi = (w.view(torch.int32) & mask).view(torch.float32)
        r1 = w - hi
        mid = (r1.view(torch.int32) & mask).view(torch.float32)
        lo = r1 - mid
        return [((x_.view(torch.int32) >> 16) & 0xFFFF) for x_ in (hi, mid, lo)]

    p1, p2 = pieces(w1_t), pieces(w2_t)
    halves = []
    for hf in range(2):
        for p in range(3):
            halves.append(torch.cat([p1[p][i1[hf]], p2[p][i2[hf]]]))  # 8192 + 8192 bf16
    bits = torch.cat(halves).to(torch.int32)  # [98304] 16-bit patterns
    words = (bits[0::2] | (bits[1::2] << 16)).to(torch.int32)
    return words.view(torch.float32)


def pack_view_layer(layer) -> torch.Tensor:
    """Pack the parameters of one view-transformer layer (Transformer2D) into the input-major
    layout of csrc/gnt_view.hip (VW_* offsets)."""
    a = layer.attn
    dev = a.q_fc.weight.device

    def pad_cols(w_t, cols):  # [in][out] -> [in][cols]
        out = torch.zeros((w_t.shape[0], cols), dtype=torch.float32, device=dev)
        out[:, : w_t.shape[1]] = w_t
        return out

    def pad_vec(b, n):
        out = torch.zeros(n, dtype=torch.float32, device=dev)
        out[: b.numel()] = b
        return out

    parts = [
        layer.attn_norm.weight, layer.attn_norm.bias, a.q_fc.weight.t(), a.k_fc.weight.t(), a.v_fc.weight.t(),
        pad_cols(a.pos_fc[0].weight.t(), 32), pad_vec(a.pos_fc[0].bias, 32), a.pos_fc[2].weight.t(), a.pos_fc[2].bias,
        pad_cols(a.attn_fc[0].weight.t(), 32), pad_vec(a.attn_fc[0].bias, 32), a.attn_fc[2].weight.t(), a.attn_fc[2].bias,
        a.out_fc.weight.t(), a.out_fc.bias, layer.ff_norm.weight, layer.ff_norm.bias, layer.ff.fc1.weight.t(),
        layer.ff.fc1.bias, layer.ff.fc2.weight.t(), layer.ff.fc2.bias,
        ff_bf16x3_images(layer.ff.fc1.weight.t(), layer.ff.fc2.weight.t()),
    ]
    packed = torch.cat([p.detach().float().contiguous().reshape(-1) for p in parts])
    assert packed.numel() == _lib.load().pgdvs_gnt_view_weight_floats(), packed.numel()
    return packed


def gnt_view_layer(layer, q, feat, ray_diff, valid, want_stats):
    """q[R,S,64], feat[R,S,V,64], ray_diff[R,S,V,4], valid[R,S,V] bool -> (q_out, stats or None)."""
    packed = _packed(layer, lambda: pack_view_layer(layer))
    R, S, V = feat.shape[0], feat.shape[1], feat.shape[2]
    N = R * S
    qi = _req(q, torch.float32, "q")
    ft = _req(feat, torch.float32, "feat")
    rd = _req(ray_diff, torch.float32, "ray_diff")
    vd = _req(valid.view(torch.uint8) if valid.dtype == torch.bool else valid, torch.uint8, "valid")
    out = torch.empty_like(qi)
    stats = torch.empty((N, 3), dtype=torch.float32, device=q.device) if want_stats else None
    check(_lib.load().pgdvs_gnt_view_layer(_ptr(packed), _ptr(qi), _ptr(ft), _ptr(rd), _ptr(vd), N, V, _ptr(out), _ptr(stats),
                                           _stream()), "pgdvs_gnt_view_layer")
    if not want_stats:
        return out, None
    st = stats.reshape(R, S, 3)
    return out, (st[..., 0], st[..., 1], st[..., 2])


def gnt_embed_available(mlp, cin: int) -> bool:
    """True when the fused rgbfeat_fc kernel handles this network (3+32 channels -> 64 -> 64)."""
    return (_GNT_VIEW_ENABLED and 32 < cin <= 36 and mlp[0].out_features == 64 and mlp[2].out_features == 64
            and mlp[0].in_features == cin)


def pack_embed(mlp) -> torch.Tensor:
    """rgbfeat_fc (Linear -> ReLU -> Linear) in the input-major layout of csrc/gnt_embed.hip."""
    cin = mlp[0].in_features
    rows = (cin + 3) // 4 * 4
    w1 = torch.zeros((rows, 64), dtype=torch.float32, device=mlp[0].weight.device)
    w1[:cin] = mlp[0].weight.detach().float().t()
    parts = [w1, mlp[0].bias, mlp[2].weight.t(), mlp[2].bias]
    packed = torch.cat([p.detach().float().contiguous().reshape(-1) for p in parts])
    assert packed.numel() == _lib.load().pgdvs_gnt_embed_weight_floats(cin), packed.numel()
    return packed


def gnt_embed(mlp, rgb_feat, want_std: bool):
    """rgb_feat[R,S,V,Cin] -> feat[R,S,V,64], q0[R,S,64], (std[R,S], std_normalized[R,S]) or None."""
    packed = _packed(mlp, lambda: pack_embed(mlp))
    x = _req(rgb_feat, torch.float32, "rgb_feat")
    R, S, V, cin = x.shape
    N = R * S
    feat = torch.empty((R, S, V, 64), dtype=torch.float32, device=x.device)
    q0 = torch.empty((R, S, 64), dtype=torch.float32, device=x.device)
    stats = torch.empty((N, 2), dtype=torch.float32, device=x.device) if want_std else None
    check(_lib.load().pgdvs_gnt_embed(_ptr(packed), _ptr(x), N, V, cin, _ptr(feat), _ptr(q0), _ptr(stats), _stream()),
          "pgdvs_gnt_embed")
    if not want_std:
        return feat, q0, None
    st = stats.reshape(R, S, 2)
    return feat, q0, (st[..., 0], st[..., 1])


def gnt_posfc_available(q_fcs, dim: int) -> bool:
    mlps = [m for m in q_fcs if not isinstance(m, torch.nn.Identity)]
    return (_GNT_VIEW_ENABLED and dim == 64 and len(mlps) > 0
            and all(m[0].out_features == 64 and m[2].in_features == 64 and m[2].out_features == 64 for m in mlps))


class GntPosFc:
    """Per-forward state of the even layers' positional re-embedding (csrc/gnt_embed.hip,
    pgdvs_gnt_posfc): the position / direction parts of every q_fc's first layer come from one
    GEMM each, the per-row part runs in the MFMA kernel."""

    def __init__(self, q_fcs, pe_pts, pe_view):
        """pe_pts[R,S,P], pe_view[R,P']"""
        self.ids = [i for i, m in enumerate(q_fcs) if not isinstance(m, torch.nn.Identity)]
        mlps = [q_fcs[i] for i in self.ids]
        P, Pv = pe_pts.shape[-1], pe_view.shape[-1]
        def build():
            wp = torch.cat([m[0].weight.detach().float()[:, 64:64 + P] for m in mlps], 0).t().contiguous()  # [P, 64 L]
            wv = torch.cat([m[0].weight.detach().float()[:, 64 + P:64 + P + Pv] for m in mlps], 0).t().contiguous()
            b1 = torch.cat([m[0].bias.detach().float() for m in mlps], 0)
            packed = [torch.cat([m[0].weight.detach().float()[:, :64].t().contiguous().reshape(-1),
                                 m[2].weight.detach().float().t().contiguous().reshape(-1),
                                 m[2].bias.detach().float()]) for m in mlps]
            return (wp, wv, b1, packed)

        wp, wv, b1, self.packed = _packed(q_fcs, build)
        R, S = pe_pts.shape[0], pe_pts.shape[1]
        self.R, self.S = R, S
        self.T = pe_pts.reshape(R * S, P).float() @ wp        # [N, 64 L]
        self.tv = torch.addmm(b1, pe_view.float(), wv)        # [R, 64 L]

    def __call__(self, layer_index, q):
        k = self.ids.index(layer_index)
        qi = _req(q, torch.float32, "q")
        out = torch.empty_like(qi)
        N = self.R * self.S
        check(_lib.load().pgdvs_gnt_posfc(_ptr(self.packed[k]), _ptr(qi), self.T.data_ptr() + 256 * k, self.T.shape[1],
                                          self.tv.data_ptr() + 256 * k, self.tv.shape[1], N, self.S, _ptr(out), _stream()),
              "pgdvs_gnt_posfc")
        return out


def gnt_head_available(norm, rgb_fc) -> bool:
    return (_GNT_VIEW_ENABLED and tuple(norm.normalized_shape) == (64,) and abs(norm.eps - 1e-5) < 1e-12
            and rgb_fc.in_features == 64 and rgb_fc.out_features == 3)


def gnt_head(norm, rgb_fc, q):
    """rgb_fc(norm(q).mean(dim=1)): q[R,S,64] -> [R,3]"""
    packed = _packed(rgb_fc, lambda: torch.cat([p.detach().float().contiguous().reshape(-1)
                                                for p in (norm.weight, norm.bias, rgb_fc.weight, rgb_fc.bias)]), norm, rgb_fc)
    qi = _req(q, torch.float32, "q")
    R, S, _ = qi.shape
    out = torch.empty((R, 3), dtype=torch.float32, device=q.device)
    check(_lib.load().pgdvs_gnt_head(_ptr(packed), _ptr(qi), R, S, _ptr(out), _stream()), "pgdvs_gnt_head")
    return out


def pack_ray_layer(layer) -> torch.Tensor:
    """Ray-transformer layer (Transformer) in the same packed layout; view-only regions stay 0."""
    a = layer.attn
    dev = a.q_fc.weight.device
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    parts = [
        layer.attn_norm.weight, layer.attn_norm.bias, a.q_fc.weight.t(), a.k_fc.weight.t(), a.v_fc.weight.t(),
        z(128 + 32 + 512 + 64 + 2048 + 32 + 512 + 64),
        a.out_fc.weight.t(), a.out_fc.bias, layer.ff_norm.weight, layer.ff_norm.bias, layer.ff.fc1.weight.t(),
        layer.ff.fc1.bias, layer.ff.fc2.weight.t(), layer.ff.fc2.bias,
        ff_bf16x3_images(layer.ff.fc1.weight.t(), layer.ff.fc2.weight.t()),
    ]
    packed = torch.cat([p.detach().float().contiguous().reshape(-1) for p in parts])
    assert packed.numel() == _lib.load().pgdvs_gnt_view_weight_floats(), packed.numel()
    return packed


GNT_RAY_MAX_SAMPLES = 256  # K and V of one ray live in LDS (csrc/gnt_view.hip)


def gnt_ray_available(dim: int, n_samples: int, n_heads: int) -> bool:
    return _GNT_VIEW_ENABLED and dim == 64 and n_heads == 4 and 1 <= n_samples <= GNT_RAY_MAX_SAMPLES


def gnt_ray_layer(layer, q, want_attn: bool):
    """q[R,S,64] -> (q_out[R,S,64], weights[R,S] or None)."""
    packed = _packed(layer, lambda: pack_ray_layer(layer))
    qi = _req(q, torch.float32, "q")
    R, S, _ = qi.shape
    out = torch.empty_like(qi)
    w = torch.empty((R, S), dtype=torch.float32, device=q.device) if want_attn else None
    check(_lib.load().pgdvs_gnt_ray_layer(_ptr(packed), _ptr(qi), R, S, _ptr(out), _ptr(w), _stream()), "pgdvs_gnt_ray_layer")
    return out, w
