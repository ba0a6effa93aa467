"""What tests/test_resample_host.py and tests/test_gpu_resample.py share: the shapes, contents and filters of the resize
checks, Pillow's answer (the yardstick: ``Image.resize`` of the installed Pillow, called here), ``pgdvs_resample_table`` through
ctypes, and a numpy statement of the resampler's two integer passes over those tables."""
import ctypes as C

import numpy as np
import PIL.Image

FILTERS = {"box": (0, PIL.Image.Resampling.BOX), "lanczos": (1, PIL.Image.Resampling.LANCZOS)}
# (in H, in W) -> (out H, out W)
SHAPES = [
    ((1, 1), (1, 1)),  # copy
    ((1, 1), (3, 2)),  # upscale from one pixel, the filter scale clamped to 1
    ((7, 5), (3, 2)),  # small downscale
    ((5, 7), (11, 13)),  # upscale
    ((37, 53), (9, 13)),  # non-integer ratios
    ((45, 60), (12, 16)),  # ratio 3.75: 25 LANCZOS taps
    ((3, 1031), (2, 257)),  # a row wider than a block, output past 256
    ((64, 64), (64, 17)),  # horizontal pass only
    ((64, 64), (17, 64)),  # vertical pass only
    ((108, 206), (29, 55)),  # the workload's ratio (1080 x 2062 -> 288 x 550) at a tenth
]
CONTENTS = ("random", "checker", "white", "black")


def random_pairs(n=60, lo=1, hi=39, seed=20):
    """``n`` seeded ((in H, in W), (out H, out W)) with every size in lo .. hi"""
    r = np.random.default_rng(seed).integers(lo, hi + 1, (n, 4))
    return [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in r]


def content(kind, h, w, c, seed=0):
    """uint8 [h,w] (c == 1) or [h,w,3]: random bytes; a 0/255 checkerboard (LANCZOS's negative lobes overshoot both ways:
    the clamp decides); all 255 (the rounded coefficients need not sum to 2^22); all 0"""
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == "random":
        return np.random.default_rng(1000 * h + 10 * w + c + seed).integers(0, 256, shape, dtype=np.uint8)
    if kind == "checker":
        board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2) * 255).astype(np.uint8)
        return board if c == 1 else np.ascontiguousarray(np.repeat(board[..., None], c, axis=2))
    return np.full(shape, {"white": 255, "black": 0}[kind], dtype=np.uint8)


def pil_resize(a, out_hw, filter):
    """the yardstick"""
    return np.array(PIL.Image.fromarray(a).resize((out_hw[1], out_hw[0]), resample=FILTERS[filter][1]))


def table(n_in, n_out, filter):
    """``pgdvs_resample_table`` of one axis -> (bounds [out,2], kk [out,ksize]) int32, or (-1, message) when it refuses"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    fid = FILTERS[filter][0] if isinstance(filter, str) else filter
    ksize = lib.pgdvs_resample_table(n_in, n_out, fid, None, None)
    if ksize < 0:
        return ksize, lib.pgdvs_last_error().decode()
    bounds, kk = np.full((n_out, 2), -7, np.int32), np.full((n_out, ksize), -7, np.int32)
    rc = lib.pgdvs_resample_table(n_in, n_out, fid, C.c_void_p(bounds.ctypes.data), C.c_void_p(kk.ctypes.data))
    assert rc == ksize, (rc, ksize)
    return bounds, kk


def _pass(a, bounds, kk, first=0):
    """one pass along axis 0 of int32 ``a`` [n_in - first, ...]: acc = 2^21 + sum k * pixel in int32, clamp(acc >> 22, 0, 255)"""
    out = np.empty((len(bounds),) + a.shape[1:], np.int32)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, np.int32)
        for t in range(n):
            acc = acc + kk[i, t] * a[lo - first + t]
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def two_passes(a, out_hw, filter):
    """the resampler over ``pgdvs_resample_table``'s tables: horizontal first, over the rows the vertical pass reads, rounded
    to 8 bits in between; an axis that keeps its size is skipped"""
    x = a.astype(np.int32)
    (h_in, w_in), (h, w) = a.shape[:2], out_hw
    first = 0
    if h != h_in:
        bounds_v, kk_v = table(h_in, h, filter)
        first, last = bounds_v[0, 0], bounds_v[-1, 0] + bounds_v[-1, 1]
        if w != w_in:
            x = x[first:last]
        else:
            first = 0
    if w != w_in:
        bounds_h, kk_h = table(w_in, w, filter)
        x = np.moveaxis(_pass(np.moveaxis(x, 1, 0), bounds_h, kk_h), 0, 1)
    if h != h_in:
        x = _pass(x, bounds_v, kk_v, first)
    return x.astype(np.uint8)
