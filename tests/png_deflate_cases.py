"""Inputs shared by tests/test_png_deflate_host.py and tests/test_gpu_png_deflate.py: the crafted byte buffers at which the
run-length tokens, the segment cuts, the length-limited code and the Adler sums of ``png.deflate_rle`` / ``ops.png_deflate``
can go wrong, and scanlines of small images.  Everything is seeded; a buffer is built once per process."""
import functools

import numpy as np

SEGS = (4096, 32768)
RUN_LENGTHS = (1, 2, 3, 4, 5, 259, 260, 261, 262, 263, 517)  # the 3 / 4 threshold and (n - 1) % 258 in {0, 1, 2, 3, 4}


def _separated_runs():
    out = []
    for i, n in enumerate(RUN_LENGTHS):
        out += [10 + i] * n + [200 + i]  # (all values distinct: no run grows by its separator)
    return np.array(out, dtype=np.uint8)


def deep_tree():
    """19 distinct values with the counts 2^0 .. 2^18 (524 287 bytes), shuffled: the unlimited Huffman tree is deeper than 15"""
    vals = np.repeat((np.arange(19) * 13 + 1).astype(np.uint8), [1 << i for i in range(19)])
    np.random.default_rng(19).shuffle(vals)
    return vals


@functools.lru_cache(maxsize=None)
def buffers() -> dict:
    rng = np.random.default_rng(20)
    b = {
        "one": np.array([7], dtype=np.uint8),
        "seven": np.array([1, 2, 2, 2, 2, 2, 9], dtype=np.uint8),
        "runs": _separated_runs(),
        "zeros": np.zeros(100000, dtype=np.uint8),
        "ff": np.full(70001, 255, dtype=np.uint8),
        "noise": rng.integers(0, 256, 50000, dtype=np.uint8),
        "deep": deep_tree(),
    }
    for seg in SEGS:
        for n in (seg - 1, seg, seg + 1, 3 * seg + 1):  # (the last: a final segment of one byte)
            b[f"len{n}"] = rng.integers(0, 4, n, dtype=np.uint8)
        a = rng.integers(0, 256, 2 * seg, dtype=np.uint8)
        a[seg - 100:seg + 100] = 5
        b[f"straddle{seg}"] = a
        a = rng.integers(0, 256, 2 * seg, dtype=np.uint8)
        a[seg - 300:seg] = 5
        a[seg] = 6
        b[f"ends_on{seg}"] = a
    for v in b.values():
        v.setflags(write=False)
    return b


def render_image(H, W):
    """uint8 [H,W,3]: the project's synthetic render (smooth background, moving objects), quantised"""
    from pgdvs_amd import synth

    rgb = synth.make_video(1, max(H, 16), max(W, 16), seed=5)["rgbs"][0][:H, :W]
    return np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8)


def smooth_image(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([255 * x / max(W - 1, 1), 255 * y / max(H - 1, 1), 127 + 127 * np.sin((x + y) / 40.0)], axis=2).astype(np.uint8)


def noise_image(H, W):
    return np.random.default_rng(1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def scanlines(kind: str, H: int, W: int):
    """adaptive-filtered scanlines [H,1+3W] uint8 of one of the images above (or "zeros")"""
    from pgdvs_amd import png

    img = {"render": render_image, "smooth": smooth_image, "noise": noise_image, "zeros": lambda h, w: np.zeros((h, w, 3), np.uint8)}[kind](H, W)
    s = png.filter_scanlines(np.ascontiguousarray(img))
    s.setflags(write=False)
    return s


def zlib_rle_size(raw) -> int:
    """the bytes of zlib's own run-length strategy on the same input"""
    import zlib

    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(co.compress(np.ascontiguousarray(raw).tobytes()) + co.flush())


def boundary_buffers(boundary: int, length: int, seed: int):
    """For one boundary of the kernel's tiling: noise buffers of ``length`` bytes, each with one run that starts k bytes in
    front of the boundary and is n long, for every k and n below -- runs that end on, reach and cross the boundary, matches
    whose 258-byte groups are cut by it, and remainders of 0 .. 4 behind it."""
    rng = np.random.default_rng(seed)
    out = []
    for k in (0, 1, 2, 3, 7, 8, 9, 63, 64, 257, 258, 259, 300):
        for n in (3, 4, 5, 259, 262, 263, 520):
            a = rng.integers(0, 256, length, dtype=np.uint8)
            lo = max(boundary - k, 0)
            hi = min(lo + n, length)
            v = a[lo]
            a[lo:hi] = v
            if lo > 0 and a[lo - 1] == v:
                a[lo - 1] ^= 1
            if hi < length and a[hi] == v:
                a[hi] ^= 1
            out.append(a)
    return np.stack(out)
