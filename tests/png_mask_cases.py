"""What tests/test_png_mask_host.py and tests/test_gpu_png_mask.py share: the mask files -- grey and palette PNGs of bit depth
1, 2, 4 and 8 -- written by Pillow where it writes them (1-bit, ``L``, ``P``) and assembled by hand over tests/png_decode_cases.py's
writer where it does not (depths 2 and 4, every filter type, padding bits that are not zero, several IDAT chunks, stored and
fixed blocks), the files that are refused, and Pillow's answer to a file.  No tests in here."""
import functools
import io
import struct
import zlib

import numpy as np
import PIL.Image

import png_decode_cases as PC

GREY, PALETTE = 0, 3
WIDTHS, HEIGHTS = (1, 7, 8, 9, 13, 71), (1, 63, 64, 65, 130)
MONO = (288, 550)  # the mono video's size
# every width and every height at least once per format; 64 rows are one row block of the unfilter, 65 and 130 cross it
SIZES = ((1, 1), (63, 7), (64, 8), (65, 9), (130, 13), (1, 71), (65, 71))


def samples(h, w, depth, seed):
    """[h,w] uint8 below 2^depth: stripes and blobs with a noisy patch, as a mask has them"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((yy // 5 + xx // 3 + (yy * xx) // 37) % (1 << depth)).astype(np.uint8)
    ph, pw = max(h // 3, 1), max(w // 2, 1)
    a[h // 4:h // 4 + ph, w // 5:w // 5 + pw] = rng.integers(0, 1 << depth, a[h // 4:h // 4 + ph, w // 5:w // 5 + pw].shape)
    return a


def pack(values, depth, seed):
    """the packed rows [h, ceil(w depth / 8)] of ``values`` [h,w], most significant bits first; the padding bits of each row's
    last byte are random, not zero"""
    h, w = values.shape
    per = 8 // depth
    r = -(-w // per)
    padded = np.random.default_rng(seed).integers(0, 1 << depth, (h, r * per), dtype=np.uint8)
    if r * per > w:
        padded[:, w] = (1 << depth) - 1  # (at least one padding sample is not zero)
    padded[:, :w] = values
    out = np.zeros((h, r), np.uint8)
    for j in range(per):
        out |= padded[:, j::per] << (8 - depth * (j + 1))
    return out


def wrap(h, w, depth, colour, z, idat_bytes=None, before=(), after=(), interlace=0):
    if colour == PALETTE:
        before = (PC.chunk(b"PLTE", bytes(k * 37 % 256 for k in range(3 * (1 << depth)))), *before)
    step = idat_bytes or max(len(z), 1)
    idat = b"".join(PC.chunk(b"IDAT", z[k:k + step]) for k in range(0, max(len(z), 1), step))
    return PC.SIGNATURE + PC.ihdr(h, w, 1, depth, interlace, colour) + b"".join(before) + idat + b"".join(after) + PC.chunk(b"IEND")


def scanlines(values, depth, ftypes, seed=0):
    """the filtered scanlines of a file of ``values``: packed, then filtered with the byte as the unit"""
    return PC.filter_rows(pack(values, depth, seed)[..., None], ftypes).tobytes()


def write(values, depth, colour, ftypes=(0, 1, 2, 3, 4), seed=0, idat_bytes=None, **kw):
    h, w = values.shape
    if "flush_rows" in kw:
        kw["row_bytes"] = 1 + -(-w * depth // 8)
    return wrap(h, w, depth, colour, PC.deflate(scanlines(values, depth, ftypes, seed), **kw), idat_bytes=idat_bytes)


def pillow_save(array, mode, **kw):
    b = io.BytesIO()
    PIL.Image.fromarray(array).convert(mode).save(b, format="png", **kw)
    return b.getvalue()


def pillow(data):
    """``np.array(PIL.Image.open(f)).astype(np.uint8)``: what a served mask file decodes to"""
    return np.array(PIL.Image.open(io.BytesIO(data))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, file)]: every one a file Pillow opens and ``kinds="mask"`` serves"""
    out, seed = [], 0
    for colour, name in ((GREY, "grey"), (PALETTE, "palette")):
        for depth in (1, 2, 4, 8):
            for h, w in SIZES:
                seed += 1
                out.append((f"{name} depth {depth} {h}x{w} rows cycling 0..4", write(samples(h, w, depth, seed), depth, colour, seed=seed)))
    for ft in range(5):  # Paeth included, on row 0 too
        out.append((f"filter {ft} on every row, grey depth 1, 9x13", write(samples(9, 13, 1, 50 + ft), 1, GREY, (ft,), seed=ft)))
        out.append((f"filter {ft} on every row, palette depth 2, 66x9", write(samples(66, 9, 2, 60 + ft), 2, PALETTE, (ft,), seed=ft)))
        out.append((f"filter {ft} on every row, grey depth 4 noise, 7x71", write(np.random.default_rng(ft).integers(0, 16, (7, 71), dtype=np.uint8), 4, GREY, (ft,))))
    v = samples(65, 71, 2, 70)
    out.append(("IDAT in 1-byte chunks", write(samples(9, 13, 4, 71), 4, GREY, idat_bytes=1)))
    out.append(("IDAT in 7-byte chunks", write(v, 2, PALETTE, idat_bytes=7)))
    out.append(("level 0: stored blocks", write(v, 2, GREY, level=0)))
    out.append(("Z_FIXED: fixed blocks", write(v, 2, GREY, strategy=zlib.Z_FIXED)))
    out.append(("level 9: dynamic blocks", write(v, 2, GREY, level=9)))
    out.append(("Z_SYNC_FLUSH after every row: short blocks", write(v, 2, PALETTE, (4, 1), flush_rows=zlib.Z_SYNC_FLUSH)))
    rng = np.random.default_rng(80)
    for h, w in ((1, 1), (63, 7), (65, 9), (130, 71)):
        blob = samples(h, w, 1, h + w).astype(bool)
        out.append((f"Pillow 1-bit {h}x{w}", pillow_save(blob, "1")))  # what preprocess/final_mask.py writes
        out.append((f"Pillow L {h}x{w}", pillow_save(rng.integers(0, 256, (h, w), dtype=np.uint8), "L")))
        out.append((f"Pillow P {h}x{w}", pillow_save(PC.content("smooth", h, w, 3, h), "P")))
    out.append(("Pillow L, compress_level 0", pillow_save(samples(64, 13, 8, 81), "L", compress_level=0)))
    out.append(("Pillow P, optimize", pillow_save(PC.content("smooth", 40, 33, 3, 3), "P", optimize=True)))
    out.append((f"Pillow 1-bit {MONO[0]}x{MONO[1]}", pillow_save(samples(*MONO, 1, 82).astype(bool), "1")))
    return out


def small_cases(n=12):
    """a spread of ``cases`` for the tests that repeat a run per file"""
    got = cases()
    return got[::max(len(got) // n, 1)]


def host_refusals():
    """[(label, file, word of the reason)]: refused on the host under ``kinds="mask"``, in front of any decode"""
    v = samples(6, 5, 8, 1)
    good = write(v, 8, GREY, (0, 1))
    z = PC.deflate(scanlines(v, 8, (0,)))
    deep = io.BytesIO()
    PIL.Image.fromarray(v.astype(np.uint16) * 257).save(deep, format="png")
    bad_crc = bytearray(good)
    bad_crc[len(good) - 14] ^= 1  # the IDAT chunk's CRC
    return [
        ("16 bits", deep.getvalue(), "colour type"), ("grey + alpha", pillow_save(np.dstack([v, v]), "LA"), "colour type"),
        ("interlaced", wrap(6, 5, 8, GREY, z, interlace=1), "interlaced"),
        ("tRNS", wrap(6, 5, 8, GREY, z, before=(PC.chunk(b"tRNS", bytes(2)),)), "tRNS"),
        ("APNG", wrap(6, 5, 8, PALETTE, z, before=(PC.chunk(b"acTL", struct.pack(">II", 1, 0)),)), "acTL"),
        ("truncated", good[:-9], "truncated"), ("bad CRC", bytes(bad_crc), "CRC"),
        ("RGB under kinds=mask alone", PC.write(PC.content("smooth", 6, 5, 3, 1), (0,)), "colour type"),
    ]


def device_refusals():
    """[(label, file, status bits of which at least one must be set)]: served by the host side, given up behind the inflate"""
    v = samples(6, 13, 2, 2)
    h, w = v.shape
    raw = scanlines(v, 2, (0, 1))
    pitch = 1 + -(-w * 2 // 8)
    z = PC.deflate(raw)
    five = bytearray(raw)
    five[2 * pitch] = 5
    return [
        ("a filter byte 5", wrap(h, w, 2, GREY, PC.deflate(bytes(five))), PC.FILTER),
        ("a flipped Adler byte", wrap(h, w, 2, GREY, z[:-2] + bytes([z[-2] ^ 0x10]) + z[-1:]), PC.ADLER),
        ("one row too few", wrap(h, w, 2, PALETTE, PC.deflate(raw[:-pitch])), PC.SIZE),
        ("the rows of the 8-bit file of this size", wrap(h, w, 2, GREY, PC.deflate(PC.filter_rows(v[..., None], (0,)).tobytes())), PC.SIZE),
        ("data running out", wrap(h, w, 2, GREY, z[:len(z) // 2]), PC.DATA_OUT | PC.CODE | PC.BLOCK | PC.DISTANCE | PC.STORED),
    ]


def fuzz_files():
    """the small files of tools/png_mask_fuzz.cpp's run: each format's unpack once, the carry row crossed"""
    return {"grey1.png": write(samples(9, 13, 1, 21), 1, GREY), "pal2.png": write(samples(66, 7, 2, 22), 2, PALETTE, strategy=zlib.Z_FIXED),
            "grey4.png": write(samples(5, 9, 4, 23), 4, GREY, (4, 3)), "pal8.png": write(samples(4, 6, 8, 24), 8, PALETTE, (2, 1))}
