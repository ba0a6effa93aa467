"""What tests/test_png_decode_host.py and tests/test_gpu_png_decode.py share: a small PNG writer (own row filtering, zlib
through ``zlib.compressobj``, or tokens written by hand in the fixed code) that builds what Pillow would never choose, the
streams where inflating in subsequences can go wrong, the damaged files, and Pillow's answer to a file.  No tests in here."""
import functools
import io
import struct
import zlib

import numpy as np
import PIL.Image

SUB = 64  # PGDVS_PNG_INFLATE_SUB_BYTES
TEAM = 256  # subsequences of a window
BLOCK, CODE, DISTANCE, STORED, DATA_OUT, SIZE, LEFT_OVER, ADLER, FILTER, NOT_SYNCHRONISED = (1 << k for k in range(10))
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---------------------------------------------------------------------------- the writer
def content(kind, h, w, c, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w, c), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(yy * 3 + xx * 2 + 40 * k) % 256 for k in range(c)], -1).astype(np.uint8)  # smooth, with a noisy patch
    a[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)] = rng.integers(0, 256, a[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)].shape)
    return a


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, ftypes):
    """the filtered scanlines of ``img`` [H,W,C] uint8, row y under filter ``ftypes[y % len(ftypes)]`` (the PNG specification's
    five, on row 0 and column 0 with zeros for what lies outside)"""
    h, w, c = img.shape
    flat = img.reshape(h, w * c).astype(np.int32)
    out = np.zeros((h, 1 + w * c), np.uint8)
    for y in range(h):
        ft = ftypes[y % len(ftypes)]
        row = flat[y]
        up = flat[y - 1] if y else np.zeros_like(row)
        left = np.concatenate([np.zeros(c, np.int32), row[:-c]])
        upleft = np.concatenate([np.zeros(c, np.int32), up[:-c]])
        pred = {0: 0, 1: left, 2: up, 3: (left + up) // 2, 4: _paeth(left, up, upleft)}[ft]
        out[y, 0], out[y, 1:] = ft, (row - pred) & 255
    return out


def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(h, w, c, depth=8, interlace=0, colour=None):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, {3: 2, 4: 6}[c] if colour is None else colour, 0, 0, interlace))


def wrap(h, w, c, zstream, idat_bytes=None, before=(), after=()):
    """a PNG file around a zlib stream: IHDR, ``before``, the stream in IDAT chunks of ``idat_bytes``, ``after``, IEND"""
    step = idat_bytes or max(len(zstream), 1)
    idat = b"".join(chunk(b"IDAT", zstream[k:k + step]) for k in range(0, max(len(zstream), 1), step))
    return SIGNATURE + ihdr(h, w, c) + b"".join(before) + idat + b"".join(after) + chunk(b"IEND")


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_rows=None, row_bytes=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_rows is None:
        return co.compress(raw) + co.flush()
    parts = [co.compress(raw[k:k + row_bytes]) + co.flush(flush_rows) for k in range(0, len(raw), row_bytes)]
    return b"".join(parts) + co.flush()


def write(img, ftypes=(0,), **kw):
    h, w, c = img.shape
    extra = {k: kw.pop(k) for k in ("idat_bytes", "before", "after") if k in kw}
    raw = filter_rows(img, ftypes).tobytes()
    if "flush_rows" in kw:
        kw["row_bytes"] = 1 + w * c
    return wrap(h, w, c, deflate(raw, **kw), **extra)


def pillow_save(img, **kw):
    b = io.BytesIO()
    PIL.Image.fromarray(img).save(b, format="png", **kw)
    return b.getvalue()


# ---------------------------------------------------------------------------- deflate by hand: the fixed code
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):  # least significant bit first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):  # a Huffman code: most significant bit first
        self.put(int(f"{value:0{nbits}b}"[::-1], 2), nbits)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def _fixed_litlen(b, sym):
    if sym < 144:
        b.code(0x30 + sym, 8)
    elif sym < 256:
        b.code(0x190 + sym - 144, 9)
    elif sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xC0 + sym - 280, 8)


def fixed_blocks(blocks, dist_symbol=None):
    """(zlib stream, the bytes it inflates to) of blocks in the fixed code; a block is a list of tokens: an int (a literal) or
    (length, distance).  ``dist_symbol``: write that distance symbol whatever the distance (30 and 31 are not codes)"""
    b, raw = Bits(), bytearray()
    b.put(0x78, 8), b.put(0x01, 8)
    for k, tokens in enumerate(blocks):
        b.put(1 if k == len(blocks) - 1 else 0, 1), b.put(1, 2)
        for tk in tokens:
            if isinstance(tk, int):
                _fixed_litlen(b, tk)
                raw.append(tk)
                continue
            length, dist = tk
            ls = max(k for k in range(29) if _LEN_BASE[k] <= length)
            _fixed_litlen(b, 257 + ls)
            b.put(length - _LEN_BASE[ls], _LEN_EXTRA[ls])
            ds = max(k for k in range(30) if _DIST_BASE[k] <= dist)
            b.code(ds if dist_symbol is None else dist_symbol, 5)
            b.put(dist - _DIST_BASE[ds], _DIST_EXTRA[ds])
            for _ in range(length):
                raw.append(raw[-dist] if dist <= len(raw) else 0)
        _fixed_litlen(b, 256)
    body = b.done()
    return body + struct.pack(">I", zlib.adler32(bytes(raw))), bytes(raw)


def _rows_of_literals(h, w, c, seed, below=144):
    """filter-0 scanlines of noise below ``below`` (8-bit codes in the fixed code): every byte a literal"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, below, (h, 1 + w * c), dtype=np.uint8)
    raw[:, 0] = 0
    return raw.tobytes()


def _literal_file(h, w, c, seed, splits=()):
    raw = _rows_of_literals(h, w, c, seed)
    cuts = [0, *splits, len(raw)]
    z, back = fixed_blocks([list(raw[a:b]) for a, b in zip(cuts, cuts[1:])])
    assert back == raw
    return wrap(h, w, c, z)


def long_matches():
    """a match of length 258 at distance 32768, then one at distance 1, in a 90 x 128 RGB image of filter-0 rows"""
    h, w, c = 90, 128, 3
    pitch = 1 + w * c
    lead = bytearray(_rows_of_literals(h, w, c, 5, 256)[:32768])
    lead[257] = 0  # the distance-1 run repeats this byte across a row's filter byte
    tokens = list(lead) + [(258, 32768), (258, 1)]
    have = 32768 + 516
    rest = bytearray(np.random.default_rng(6).integers(0, 256, h * pitch - have, dtype=np.uint8).tobytes())
    for p in range(0, h * pitch, pitch):
        if p >= have:
            rest[p - have] = 0
    z, raw = fixed_blocks([tokens + list(rest)])
    assert len(raw) == h * pitch and all(raw[p] == 0 for p in range(0, len(raw), pitch))
    return wrap(h, w, c, z)


# ---------------------------------------------------------------------------- the streams
@functools.lru_cache(maxsize=None)
def streams():
    """[(label, file)]: every one a file Pillow opens and the device path serves"""
    out = []
    for h, w in ((1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65), (65, 9), (130, 7)):
        for c in (3, 4):
            out.append((f"{h}x{w}x{c} rows cycling 0..4", write(content("smooth", h, w, c, h + w), (0, 1, 2, 3, 4))))
    for ft in range(5):
        out.append((f"filter {ft} on every row (row 0 included), RGB", write(content("smooth", 9, 11, 3, ft), (ft,))))
        out.append((f"filter {ft} on every row, RGBA noise", write(content("noise", 7, 13, 4, ft), (ft,))))
    noise = content("noise", 128, 128, 3, 1)
    out.append(("128x128 noise: several windows", write(noise, (0, 1, 2, 3, 4))))
    smooth = content("smooth", 66, 40, 3, 2)
    for level in (0, 1, 6, 9):
        out.append((f"Pillow compress_level {level}", pillow_save(smooth, compress_level=level)))
    out.append(("Pillow optimize", pillow_save(smooth, optimize=True)))
    out.append(("Pillow RGBA", pillow_save(content("smooth", 40, 33, 4, 3))))
    for name in ("Z_FIXED", "Z_HUFFMAN_ONLY", "Z_RLE", "Z_FILTERED"):
        out.append((f"strategy {name}", write(smooth, (0, 1, 2, 3, 4), strategy=getattr(zlib, name))))
    out.append(("Z_RLE over zeros: distance-1 chains across threads and windows", write(content("zeros", 100, 300, 3), (0,), strategy=zlib.Z_RLE)))
    out.append(("zeros at level 9: long matches", write(content("zeros", 100, 300, 4), (0,), level=9)))
    out.append(("level 0: stored blocks, more than 65535 bytes", write(content("smooth", 150, 146, 3, 4), (0, 4), level=0)))
    for name in ("Z_SYNC_FLUSH", "Z_FULL_FLUSH"):
        out.append((f"{name} after every row: short blocks, empty stored blocks", write(smooth, (4, 1), flush_rows=getattr(zlib, name))))
    out.append(("wbits 9", write(smooth, (0, 1, 2, 3, 4), wbits=9)))
    out.append(("wbits 15, level 9", write(smooth, (0, 1, 2, 3, 4), wbits=15, level=9)))
    out.append(("length 258 at distance 32768 and at distance 1", long_matches()))
    # fixed-code literals of 8 bits: n literals take 8 n + 10 bits = n + 2 bytes
    out.append(("deflate data of exactly one subsequence", _literal_file(2, 10, 3, 7)))          # 62 literals: 64 bytes
    out.append(("two subsequences less one byte", _literal_file(5, 8, 3, 8)))                  # 125: 127 bytes
    out.append(("two subsequences and one byte", _literal_file(1, 42, 3, 9)))                   # 127: 129 bytes
    # 4 x 2728 RGB = 32740 literals: a block of 16390 (its end-of-block falls into the second window's first subsequence), then
    # one of 16350 (8 * 16350 bits: into its window's last subsequence)
    out.append(("a block ends in a window's first and one in its last subsequence", _literal_file(4, 2728, 3, 10, splits=(16390,))))
    small = content("smooth", 5, 7, 3, 11)
    out.append(("IDAT in 1-byte chunks", write(small, (0, 1, 2, 3, 4), idat_bytes=1)))
    out.append(("ancillary chunks between the others", write(small, (4,), idat_bytes=7, before=(chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"k\0v")),
                                                              after=(chunk(b"tIME", bytes(7)), chunk(b"zzZz", b"private")))))
    return out


def pillow(data):
    """np.array(PIL.Image.open(...)) of the file, or the exception's type"""
    import warnings

    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.array(PIL.Image.open(io.BytesIO(data)))
    except Exception as e:  # noqa: BLE001 (whatever Pillow raises is the answer)
        return type(e)


# ---------------------------------------------------------------------------- what is refused
def host_refusals():
    """[(label, file, word of the reason)]: refused on the host, in front of any device work"""
    img = content("smooth", 6, 5, 3, 1)
    good = write(img, (0, 1))
    raw = filter_rows(img, (0,)).tobytes()
    z = deflate(raw)
    grey = pillow_save(img[..., 0])
    pal = io.BytesIO()
    PIL.Image.fromarray(img).convert("P").save(pal, format="png")
    deep = io.BytesIO()
    PIL.Image.fromarray(img[..., 0].astype(np.uint16) * 257).save(deep, format="png")
    bad_crc = bytearray(good)
    bad_crc[len(good) - 14] ^= 1  # the IDAT chunk's CRC
    dict_z = bytes([0x78, 0xBB]) + z[2:]  # FDICT set, FCHECK right
    assert (0x78 * 256 + 0xBB) % 31 == 0
    cz = zlib.compressobj(6, zlib.DEFLATED, 15)
    two = cz.compress(raw[:40]) + cz.flush(zlib.Z_FULL_FLUSH)
    return [
        ("grey", grey, "colour type"), ("palette", pal.getvalue(), "colour type"), ("16 bits", deep.getvalue(), "colour type"),
        ("interlaced", SIGNATURE + ihdr(6, 5, 3, interlace=1) + chunk(b"IDAT", z) + chunk(b"IEND"), "interlaced"),
        ("tRNS", wrap(6, 5, 3, z, before=(chunk(b"tRNS", bytes(6)),)), "tRNS"),
        ("APNG", wrap(6, 5, 3, z, before=(chunk(b"acTL", struct.pack(">II", 1, 0)),)), "acTL"),
        ("bad signature", b"\x89PNG\r\n\x1a\r" + good[8:], "signature"),
        ("bad CRC", bytes(bad_crc), "CRC"),
        ("IDAT chunks apart", SIGNATURE + ihdr(6, 5, 3) + chunk(b"IDAT", z[:9]) + chunk(b"tEXt", b"k\0v") + chunk(b"IDAT", z[9:]) + chunk(b"IEND"), "order"),
        ("no IHDR in front", SIGNATURE + chunk(b"gAMA", struct.pack(">I", 1)) + good[8:], "order"),
        ("truncated", good[:-9], "truncated"), ("no IEND", good[:-12], "truncated"),
        ("zlib method", wrap(6, 5, 3, bytes([0x79, 0x9B]) + z[2:]), "zlib header"), ("zlib check bits", wrap(6, 5, 3, bytes([0x78, 0x9D]) + z[2:]), "zlib header"),
        ("preset dictionary", wrap(6, 5, 3, dict_z), "dictionary"),
        ("zero width", SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 6, 8, 2, 0, 0, 0)) + chunk(b"IDAT", z) + chunk(b"IEND"), "pixels"),
        ("16385 wide", SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 16385, 1, 8, 2, 0, 0, 0)) + chunk(b"IDAT", two) + chunk(b"IEND"), "pixels"),
        ("inflated size above the cap", SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 16384, 16384, 8, 2, 0, 0, 0)) + chunk(b"IDAT", two) + chunk(b"IEND"), "above"),
    ]


def _dynamic_header(cl_lens_in_order):
    """a zlib stream whose one dynamic block states HLIT 257, HDIST 1 and these code-length-code lengths, then zeros"""
    b = Bits()
    b.put(0x78, 8), b.put(0x01, 8)
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(len(cl_lens_in_order) - 4, 4)
    for v in cl_lens_in_order:
        b.put(v, 3)
    return b.done() + bytes(12)


def device_refusals():
    """[(label, file, status bits of which at least one must be set)]: served by the host side, given up by the inflate"""
    img = content("smooth", 6, 5, 3, 1)
    h, w, c = img.shape
    raw = filter_rows(img, (0, 1)).tobytes()
    z = deflate(raw)
    flipped = z[:-2] + bytes([z[-2] ^ 0x10]) + z[-1:]
    five = bytearray(raw)
    five[2 * (1 + w * c)] = 5
    lits = list(_rows_of_literals(h, w, c, 3))
    far, _ = fixed_blocks([lits[:4] + [(len(lits) - 4, 5)]])
    sym30, _ = fixed_blocks([lits[:40] + [(len(lits) - 40, 3)]], dist_symbol=30)
    stored = bytearray(deflate(raw, level=0))
    stored[5] ^= 1  # NLEN
    b = Bits()
    b.put(0x78, 8), b.put(0x01, 8), b.put(1, 1), b.put(3, 2)
    return [
        ("a flipped Adler byte", wrap(h, w, c, flipped), ADLER),
        ("a distance in front of the output", wrap(h, w, c, far), DISTANCE),
        ("distance symbol 30", wrap(h, w, c, sym30), CODE),
        ("an over-subscribed code-length code", wrap(h, w, c, _dynamic_header([1, 1, 1, 1])), BLOCK),
        ("an incomplete code-length code", wrap(h, w, c, _dynamic_header([1, 0, 0, 0])), BLOCK),
        ("block type 3", wrap(h, w, c, b.done() + bytes(8)), BLOCK),
        ("LEN and NLEN disagree", wrap(h, w, c, bytes(stored)), STORED),
        ("a filter byte 5", wrap(h, w, c, deflate(bytes(five))), FILTER),
        ("one row too few", wrap(h, w, c, deflate(raw[:-(1 + w * c)])), SIZE),
        ("one row too many", wrap(h, w, c, deflate(raw + raw[-(1 + w * c):])), SIZE),
        ("data running out", wrap(h, w, c, z[:len(z) // 2]), DATA_OUT | CODE | BLOCK | DISTANCE | STORED),
        ("bytes behind the Adler-32", wrap(h, w, c, z + b"\0"), LEFT_OVER),
        ("the Adler-32 cut short", wrap(h, w, c, z[:-1]), DATA_OUT),
    ]


def fuzz_files():
    """the three small files of the truncation and mutation runs (and of tools/png_inflate_fuzz.cpp)"""
    a, b = content("smooth", 9, 11, 3, 21), content("noise", 4, 6, 4, 22)
    return {"rgb_cycle.png": write(a, (0, 1, 2, 3, 4)), "rgba_fixed.png": write(b, (4, 3), strategy=zlib.Z_FIXED),
            "rgb_flush.png": write(a[:5, :7], (2, 1), flush_rows=zlib.Z_SYNC_FLUSH, level=1)}


def split(data):
    """(h, w, c, zlib stream) of a file of this module's writer"""
    pos, z, dims = 8, b"", None
    while pos < len(data):
        (n,) = struct.unpack_from(">I", data, pos)
        kind = data[pos + 4:pos + 8]
        if kind == b"IHDR":
            w, h, _, colour = struct.unpack_from(">IIBB", data, pos + 8)
            dims = (h, w, 3 if colour == 2 else 4)
        elif kind == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return (*dims, z)


def stream_mutations(data, n, seed):
    """``n`` files whose zlib stream has one byte replaced, the chunks' CRCs right again: the damage reaches the inflate"""
    h, w, c, z = split(data)
    rng = np.random.default_rng(seed)
    at, val = rng.integers(0, len(z), n), rng.integers(0, 256, n)
    for a, v in zip(at.tolist(), val.tolist()):
        yield wrap(h, w, c, z[:a] + bytes([v]) + z[a + 1:])


def stream_truncations(data):
    h, w, c, z = split(data)
    for n in range(len(z)):
        yield wrap(h, w, c, z[:n])
