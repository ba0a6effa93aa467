"""What tests/test_jpeg_decode_host.py and tests/test_gpu_jpeg_decode.py share: the stream matrix, the streams the reader
refuses, Pillow's answer (the yardstick: ``np.array(PIL.Image.open(...))`` of the installed Pillow, which must be built over
libjpeg-turbo), the two host entries through ctypes, and a numpy statement of the reconstruction (libjpeg's islow inverse
DCT, fancy upsampling and colour tables) over the coefficients the host entry decodes.  No tests in here."""
import ctypes as C
import functools
import io

import numpy as np
import PIL.features
import PIL.Image

# (H, W): one block; odd sizes; several MCUs; a last MCU of one column / row; chroma planes 1 and 2 samples wide (plain
# replication) and 3 wide (the shortest fancy row); one pixel; a width of whole MCUs; several workgroups of both kernels
SIZES = [(8, 8), (17, 23), (40, 56), (33, 49), (16, 2), (5, 3), (31, 64), (1, 1), (24, 33), (130, 270)]
SUBSAMPLINGS = (0, 1, 2)  # Pillow's: 4:4:4, 4:2:2, 4:2:0
QUALITIES = (30, 95, 100)
CONTENTS = ("noise", "smooth")
RESTARTS = (None, 3)


def require_turbo():
    import pytest

    if not PIL.features.check_feature("libjpeg_turbo"):
        pytest.skip("the installed Pillow is not built over libjpeg-turbo: its decoder is the yardstick of these tests")


def content(kind, h, w, seed=0):
    """uint8 [h,w,3]: seeded noise; or a smooth gradient with hard edges (a dark bar, a primary-coloured box) and a patch
    saturated at 255 / 0, whose ringing reaches the clamps"""
    if kind == "noise":
        return np.random.default_rng(100000 + 1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], axis=2).astype(np.uint8)
    a[h // 3: h // 3 + max(h // 8, 1)] = 10
    a[h // 2:, w // 2: w // 2 + max(w // 5, 1)] = (255, 0, 0)
    a[: max(h // 4, 1), : max(w // 4, 1)] = 255
    a[h - max(h // 5, 1):, : max(w // 6, 1)] = 0
    return a


def encode(a, subsampling, quality, restart=None, optimize=False):
    buf = io.BytesIO()
    kw = {} if restart is None else {"restart_marker_blocks": restart}
    PIL.Image.fromarray(a).save(buf, format="JPEG", subsampling=subsampling, quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def matrix(subsampling):
    """[(label, stream)] of one chroma subsampling: every size x quality x content x restart, then ``optimize=True`` (custom
    Huffman tables) for a subset, then (at 4:4:4 and 4:2:0) the project's own encoder's files"""
    out = []
    for h, w in SIZES:
        for q in QUALITIES:
            for kind in CONTENTS:
                for rst in RESTARTS:
                    out.append((f"{h}x{w} s{subsampling} q{q} {kind} rst{rst}", encode(content(kind, h, w), subsampling, q, rst)))
    for h, w in ((17, 23), (33, 49), (130, 270)):
        for q in (30, 75):  # (Pillow gives the optimising encoder one buffer of the image's size: noise at 95 overruns it)
            out.append((f"{h}x{w} s{subsampling} q{q} noise optimize", encode(content("noise", h, w, 1), subsampling, q, None, True)))
    if subsampling in (0, 2):
        from pgdvs_amd import video

        for h, w in ((17, 23), (40, 56), (130, 270)):
            for rst in (None, 0, 2):
                out.append((f"{h}x{w} s{subsampling} own encoder rst{rst}",
                            video.encode_jpeg(content("smooth", h, w, 2), 85, rst, "4:4:4" if subsampling == 0 else "4:2:0")))
    return out


def pillow(data):
    """the yardstick"""
    return np.array(PIL.Image.open(io.BytesIO(data)))


def _save(mode, a=None, **kw):
    buf = io.BytesIO()
    im = PIL.Image.fromarray(content("smooth", 24, 40)) if a is None else a
    im.convert(mode).save(buf, format=kw.pop("format", "JPEG"), **kw)
    return buf.getvalue()


def flipped_restart(data):
    """``data`` with the index of its second RSTn marker changed"""
    i = data.index(b"\xff\xd1", data.index(b"\xff\xda"))
    return data[:i + 1] + b"\xd5" + data[i + 2:]


@functools.lru_cache(maxsize=None)
def refusals():
    """[(label, stream)]: streams Pillow reads (but for the empty one) and this reader leaves to it"""
    with_rst = encode(content("noise", 24, 40), 0, 75, 1)
    return [("progressive", _save("RGB", progressive=True)), ("greyscale", _save("L")), ("cmyk", _save("CMYK")),
            ("keep_rgb", _save("RGB", keep_rgb=True)), ("4:1:1", _save("RGB", subsampling="4:1:1")),
            ("png", _save("RGB", format="PNG")), ("empty", b""), ("flipped RSTn", flipped_restart(with_rst))]


def small_stream():
    return encode(content("smooth", 9, 11), 2, 50)


# ---------------------------------------------------------------------------- the host entries
def parse(data):
    """``pgdvs_jpeg_parse`` -> (rc, JpegInfo as filled, message)"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    info = _lib.JpegInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    buf = np.frombuffer(data, np.uint8)
    rc = lib.pgdvs_jpeg_parse(C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, C.byref(info))
    return rc, info, lib.pgdvs_last_error().decode()


GUARD = 64  # int16 words of canary on either side of the coefficients


def entropy_decode(data, coef_bytes):
    """``pgdvs_jpeg_entropy_decode`` into a buffer of ``coef_bytes`` between canaries -> (rc, int16 array, message); the
    canaries are checked here"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    mem = np.full(GUARD + coef_bytes // 2 + GUARD, 0x5A5A, np.int16)
    coef = mem[GUARD:GUARD + coef_bytes // 2]
    rc = lib.pgdvs_jpeg_entropy_decode(C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, C.c_void_p(coef.ctypes.data), coef_bytes)
    assert (mem[:GUARD] == 0x5A5A).all() and (mem[GUARD + coef_bytes // 2:] == 0x5A5A).all(), "written outside coef"
    return rc, coef, lib.pgdvs_last_error().decode()


# ---------------------------------------------------------------------------- the reconstruction in numpy
def _idct_pass(x, shift):
    """jidctint.c's 8-point pass along the last axis of int32 ``x`` [..., 8]"""
    i = [x[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    tmp2, tmp3 = z1 + i[6] * -15137, z1 + i[2] * 6270
    tmp0, tmp1 = (i[0] + i[4]) * 8192, (i[0] - i[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + half) >> shift for o in out], axis=-1)


def planes(info, coef):
    """the three 8-bit component planes over the padded grids"""
    out, off = [], 0
    for c in range(3):
        bh, bw = info.blocks_h[c], info.blocks_w[c]
        q = np.ctypeslib.as_array(info.quant)[c].astype(np.int32).reshape(8, 8)
        blk = coef[off:off + bh * bw * 64].astype(np.int32).reshape(bh, bw, 8, 8) * q
        off += bh * bw * 64
        ws = np.swapaxes(_idct_pass(np.swapaxes(blk, -1, -2), 11), -1, -2)  # columns first
        px = np.clip(_idct_pass(ws, 18) + 128, 0, 255)
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _h2v1(p):
    """jdsample.c's h2v1_fancy_upsample of int32 rows [..., n], n > 2 -> [..., 2n]"""
    left, right = np.concatenate([p[..., :1], p[..., :-1]], -1), np.concatenate([p[..., 1:], p[..., -1:]], -1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[..., 0], odd[..., -1] = p[..., 0], p[..., -1]
    return np.stack([even, odd], -1).reshape(*p.shape[:-1], -1)


def _h2v2(p):
    """h2v2_fancy_upsample of an int32 plane [m, n], n > 2 -> [2m, 2n]; the rows beyond the ends repeat them"""
    above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    rows = np.stack([3 * p + above, 3 * p + below], 1).reshape(-1, p.shape[1])  # the column sums of output rows 2i, 2i + 1
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    even, odd = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], -1).reshape(rows.shape[0], -1)


def reconstruct(info, coef):
    """uint8 [H,W,3] from the parsed info and the decoded coefficients"""
    H, W = info.height, info.width
    y, cb, cr = (p.astype(np.int32) for p in planes(info, coef))
    if info.sampling != 0:
        cw, ch = (W + 1) // 2, (H + 1) // 2 if info.sampling == 2 else H
        up = []
        for p in (cb, cr):
            p = p[:ch, :cw]
            if cw <= 2:
                p = np.repeat(np.repeat(p, 2, 1), 2 if info.sampling == 2 else 1, 0)
            else:
                p = _h2v2(p) if info.sampling == 2 else _h2v1(p)
            up.append(p)
        cb, cr = up
    y, cb, cr = y[:H, :W], cb[:H, :W] - 128, cr[:H, :W] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)
