"""PNG export of rendered views without PIL on the write path (the visualiser's two writers,
pgdvs/engines/visualizer_pgdvs.py:118-139).

A PNG is filtered scanlines (per row one filter-type byte and the row's bytes, each predicted from its left / upper
neighbours) under one zlib stream.  On the GPU the quantisation and the filtering are one HIP pass
(``ops.png_scanlines``, csrc/png.hip); this module holds the same two steps in torch / numpy for host images, the
container (``encode``), and ``PngWriter``: a ring of pinned host buffers and a small thread pool that copies, deflates
and writes behind the thread that drives the GPU (zlib releases the GIL).  With ``deflate="device"`` the writer leaves the
deflate to the GPU as well (``ops.png_deflate``, csrc/png_deflate.hip); ``deflate_rle`` states that stream on the host."""
from __future__ import annotations

import os
import pathlib
import struct
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

QUANT_MODES = ("save_image", "truncate")
MAX_THREADS = 16


def quantize_save_image(x: torch.Tensor) -> torch.Tensor:
    """``torchvision.utils.save_image``'s quantisation of an image the visualiser clamped to [0, 1]:
    ``x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` in float32 (multiply and add rounded separately).  NaN -> 0."""
    x = torch.nan_to_num(x.float().clamp(0.0, 1.0), nan=0.0)
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def quantize_truncate(x: torch.Tensor) -> torch.Tensor:
    """The ``*_gnt.png`` writer's ``(clamp(x, 0, 1) * 255).astype(np.uint8)`` in float32.  NaN -> 0."""
    x = torch.nan_to_num(x.float().clamp(0.0, 1.0), nan=0.0)
    return (x * 255).to(torch.uint8)


QUANTIZERS = {"save_image": quantize_save_image, "truncate": quantize_truncate}


def filter_scanlines(q, adaptive: bool = True) -> np.ndarray:
    """q[H,W,3] (or [B,H,W,3]) uint8 -> scanlines [H,1+3W] ([B,H,1+3W]) uint8: per row the filter-type byte, then the
    filtered bytes.  ``adaptive``: per row the PNG filter (None, Sub, Up, Average, Paeth at 3 bytes per pixel) with the
    least sum of ``v if v < 128 else 256 - v`` over its bytes (libpng's default heuristic), the lowest type on a tie;
    otherwise type 0 on every row."""
    q = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
    if q.dtype != np.uint8 or q.ndim not in (3, 4) or q.shape[-1] != 3:
        raise ValueError(f"filter_scanlines: expected uint8 [H,W,3] or [B,H,W,3], got {q.dtype} {q.shape}")
    if q.ndim == 4:
        return np.stack([filter_scanlines(v, adaptive) for v in q])
    H, W, _ = q.shape
    x = q.reshape(H, 3 * W).astype(np.int32)
    out = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    if not adaptive:
        out[:, 1:] = x
        return out
    a = np.zeros_like(x)  # left
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)  # above
    b[1:] = x[:-1]
    c = np.zeros_like(x)  # above left
    c[1:, 3:] = x[:-1, :-3]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255  # [5,H,3W]
    cost = np.where(cands < 128, cands, 256 - cands).sum(axis=2, dtype=np.int64)  # [5,H]
    ftype = np.argmin(cost, axis=0)  # (the first of equal minima)
    out[:, 0] = ftype
    out[:, 1:] = np.take_along_axis(cands, ftype[None, :, None], axis=0)[0]
    return out


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)))


def encode(scanlines, H: int, W: int, level: int = 1) -> bytes:
    """Scanlines of one image ([H,1+3W] uint8, any buffer of H (1 + 3 W) bytes) -> the PNG file: signature, IHDR (8-bit
    truecolour, no interlace), one IDAT with ``zlib.compress(scanlines, level)``, IEND."""
    if isinstance(scanlines, torch.Tensor):
        scanlines = scanlines.cpu().numpy()
    raw = memoryview(np.ascontiguousarray(scanlines)).cast("B") if isinstance(scanlines, np.ndarray) else memoryview(scanlines)
    if raw.nbytes != H * (1 + 3 * W):
        raise ValueError(f"encode: {raw.nbytes} bytes of scanlines for {H} x {W} (expected {H * (1 + 3 * W)})")
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b"")


def write_file(path, scanlines, H: int, W: int, level: int = 1) -> int:
    """``encode`` to ``path`` through a temporary name and a rename (a reader never sees a partial file); returns the bytes
    written."""
    return atomic_write(path, encode(scanlines, H, W, level))


# ---- the device deflate's stream, restated ------------------------------------------------------------------------------------
# ``ops.png_deflate`` (csrc/png_deflate.hip) writes a zlib stream that is stated here in Python / numpy integers; the kernels
# follow this statement byte for byte.  The stream: 0x78 0x01; per segment of ``seg_bytes`` scanline bytes one non-final
# dynamic-Huffman block and an empty stored block (so every segment starts and ends on a byte); one final empty fixed block;
# the Adler-32.  Tokens are zlib's Z_RLE idea at distance 1 only, segments are independent, and ONE literal/length code per
# image is built from the image's token histogram and repeated in every segment's header.
DEFLATE_SEG_MIN, DEFLATE_SEG_MAX = 4096, 65536
DEFLATE_SEG_DEFAULT = 32768
DEFLATE_MAX_BITS = 15
DEFLATE_LITLEN = 286
DEFLATE_MAX_MATCH = 258
# header of a segment's block: BFINAL, BTYPE, HLIT = 29, HDIST = 0, HCLEN = 15 (17 bits); the 19 code-length-code lengths
# (3 bits each: 0 for the repeat codes 16 / 17 / 18, 4 for 0 .. 15 -- a complete code whose codeword IS the length, 4 bits);
# 286 literal/length lengths and the one distance length (1) at 4 bits each
DEFLATE_HEADER_BITS = 17 + 3 * 19 + 4 * DEFLATE_LITLEN + 4
# bytes a segment costs beyond its tokens, at most: the header, an end-of-block of up to 15 bits, the stored block's 3 bits,
# up to 7 bits of padding (ceil(1240 / 8) + 1 = 156) and 00 00 FF FF
DEFLATE_SEG_OVERHEAD = (DEFLATE_HEADER_BITS + DEFLATE_MAX_BITS + 3 + 7) // 8 + 1 + 4
DEFLATE_MODES = ("zlib", "device")
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _length_symbol(length: int):
    """match length 3 .. 258 -> (literal/length symbol, extra bits, extra value) (RFC 1951 3.2.5)"""
    if length == DEFLATE_MAX_MATCH:
        return 285, 0, 0
    x = length - 3
    e = max(x.bit_length() - 3, 0)
    return 257 + 4 * e + (x >> e), e, x & ((1 << e) - 1)


_LEN_SYM = np.zeros((DEFLATE_MAX_MATCH + 1, 3), dtype=np.int64)
for _n in range(3, DEFLATE_MAX_MATCH + 1):
    _LEN_SYM[_n] = _length_symbol(_n)


def check_seg_bytes(seg_bytes) -> int:
    seg = DEFLATE_SEG_DEFAULT if seg_bytes is None else int(seg_bytes)
    if not (DEFLATE_SEG_MIN <= seg <= DEFLATE_SEG_MAX and seg & (seg - 1) == 0):
        raise ValueError(f"seg_bytes {seg_bytes}: a power of two in {DEFLATE_SEG_MIN} .. {DEFLATE_SEG_MAX} expected")
    return seg


def deflate_capacity(img_bytes: int, seg_bytes=None) -> int:
    """The bytes ``deflate_rle`` can take at most for ``img_bytes`` of input: a token costs at most 15 bits per byte it
    covers (a literal 15; a match 15 + 5 extra + 1 distance bit for at least 3), every segment ``DEFLATE_SEG_OVERHEAD``,
    plus the two bytes in front and the six behind (the final block and the Adler-32)."""
    seg = check_seg_bytes(seg_bytes)
    n = int(img_bytes)
    if n < 1:
        raise ValueError(f"deflate_capacity: img_bytes {img_bytes}")
    return 8 + DEFLATE_SEG_OVERHEAD * ((n + seg - 1) // seg) + (15 * n + 7) // 8


def rle_tokens(raw, seg_bytes=None):
    """raw (uint8, any shape) -> (pos, sym, extra_bits, extra_value), int64 arrays with one entry per token in stream order:
    the position of the first byte it covers and its literal/length symbol.  Runs of equal bytes are cut at every multiple
    of ``seg_bytes``; a run of n gives a literal, then (n - 1) // 258 matches of 258 and, of the r bytes left, one match
    (r >= 3) or r literals.  Every match has distance 1."""
    seg = check_seg_bytes(seg_bytes)
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    if b.size < 1:
        raise ValueError("rle_tokens: at least one byte expected")
    first = np.ones(b.size, dtype=bool)
    first[1:] = b[1:] != b[:-1]
    first[::seg] = True
    s = np.flatnonzero(first)
    n = np.diff(np.append(s, b.size))
    q, r = (n - 1) // DEFLATE_MAX_MATCH, (n - 1) % DEFLATE_MAX_MATCH
    count = 1 + q + np.where(r >= 3, 1, r)
    run = np.repeat(np.arange(s.size), count)
    k = np.arange(run.size) - np.repeat(np.cumsum(count) - count, count)  # index of the token in its run
    qk, rk, sk = q[run], r[run], s[run]
    length = np.where(k == 0, 0, np.where(k <= qk, DEFLATE_MAX_MATCH, np.where(rk >= 3, rk, 0)))
    rest = sk + 1 + DEFLATE_MAX_MATCH * qk  # where the run's last, partial group begins
    pos = np.where(k == 0, sk, np.where(k <= qk, sk + 1 + DEFLATE_MAX_MATCH * (k - 1), rest + np.where(rk >= 3, 0, k - 1 - qk)))
    sym = np.where(length > 0, _LEN_SYM[length, 0], b[sk])
    return pos, sym, _LEN_SYM[length, 1], _LEN_SYM[length, 2]


def litlen_code_lengths(hist) -> list:
    """Histogram of the 286 literal/length symbols (at least two used) -> their code lengths: a Huffman code limited to 15
    bits, complete (Kraft sum exactly 1).  The used symbols are sorted by (count, symbol); the two-queue merge takes a leaf
    before an inner node of equal weight; leaves deeper than 15 are put at 15 and, while the Kraft sum exceeds 1, the
    deepest leaf above level 15 moves one level down with a level-15 leaf as its new sibling (zlib's repair); at last the
    levels are handed out along the sorted order, the longest to the rarest."""
    hist = [int(v) for v in hist]
    if len(hist) != DEFLATE_LITLEN or min(hist) < 0:
        raise ValueError("litlen_code_lengths: 286 counts >= 0 expected")
    used = sorted((s for s in range(DEFLATE_LITLEN) if hist[s] > 0), key=lambda s: (hist[s], s))
    n = len(used)
    if n < 2:
        raise ValueError("litlen_code_lengths: at least two used symbols expected")
    w = [hist[s] for s in used]
    inner, leaf_parent, inner_parent = [], [0] * n, [0] * (n - 1)
    li = ii = 0
    for k in range(n - 1):
        total = 0
        for _ in range(2):
            if li < n and (ii >= len(inner) or w[li] <= inner[ii]):
                total += w[li]
                leaf_parent[li] = k
                li += 1
            else:
                total += inner[ii]
                inner_parent[ii] = k
                ii += 1
        inner.append(total)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[inner_parent[k]] + 1
    count = [0] * (DEFLATE_MAX_BITS + 1)
    for i in range(n):
        count[min(depth[leaf_parent[i]] + 1, DEFLATE_MAX_BITS)] += 1
    excess = sum(c << (DEFLATE_MAX_BITS - l) for l, c in enumerate(count) if l) - (1 << DEFLATE_MAX_BITS)
    while excess > 0:
        bits = DEFLATE_MAX_BITS - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[DEFLATE_MAX_BITS] -= 1
        excess -= 1
    lengths, r = [0] * DEFLATE_LITLEN, 0
    for l in range(DEFLATE_MAX_BITS, 0, -1):
        for _ in range(count[l]):
            lengths[used[r]] = l
            r += 1
    return lengths


def canonical_codes(lengths) -> list:
    """code lengths -> the canonical codes (RFC 1951 3.2.2), bit-reversed: as the stream holds them, first bit lowest"""
    count = [0] * (DEFLATE_MAX_BITS + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (DEFLATE_MAX_BITS + 2), 0
    for l in range(1, DEFLATE_MAX_BITS + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        c = 0
        if l:
            c = int(format(nxt[l], f"0{l}b")[::-1], 2)
            nxt[l] += 1
        out.append(c)
    return out


def _rev4(v: int) -> int:
    return ((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3)


def deflate_header(lengths) -> int:
    """the ``DEFLATE_HEADER_BITS`` bits in front of every segment's tokens, as an integer whose bit k is bit k of the stream"""
    bits, at = 0, 0
    for value, n in ((0, 1), (2, 2), (DEFLATE_LITLEN - 257, 5), (0, 5), (19 - 4, 4)):
        bits |= value << at
        at += n
    for s in _CL_ORDER:
        bits |= (0 if s >= 16 else 4) << at
        at += 3
    for l in list(lengths) + [1]:
        bits |= _rev4(l) << at
        at += 4
    assert at == DEFLATE_HEADER_BITS
    return bits


def deflate_rle(raw, seg_bytes=None) -> bytes:
    """The zlib stream ``ops.png_deflate`` writes for the bytes ``raw`` (uint8, any shape, at least one byte), restated on
    the host: see the comment above.  ``zlib.decompress`` returns ``raw``."""
    seg = check_seg_bytes(seg_bytes)
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    pos, sym, ebits, evalue = rle_tokens(b, seg)
    n_seg = (b.size + seg - 1) // seg
    hist = np.bincount(sym, minlength=DEFLATE_LITLEN)
    hist[256] = n_seg
    lengths = litlen_code_lengths(hist)
    codes = canonical_codes(lengths)
    len_of, code_of = np.asarray(lengths, dtype=np.int64), np.asarray(codes, dtype=np.int64)
    header = deflate_header(lengths).to_bytes((DEFLATE_HEADER_BITS + 7) // 8, "little")
    is_match = (sym > 256).astype(np.int64)
    value = code_of[sym] | (evalue << len_of[sym])  # (the distance code is the one bit 0 behind them)
    nbits = len_of[sym] + ebits + is_match
    cut = np.searchsorted(pos, np.arange(n_seg + 1) * seg)
    out = [b"\x78\x01"]
    for g in range(n_seg):
        v = np.append(value[cut[g]:cut[g + 1]], codes[256])
        nb = np.append(nbits[cut[g]:cut[g + 1]], lengths[256])
        off = DEFLATE_HEADER_BITS + np.cumsum(nb) - nb
        end = int(off[-1] + nb[-1]) + 3  # the stored block's BFINAL = 0, BTYPE = 00
        n_bytes = (end + 7) // 8 + 4
        acc = np.zeros(n_bytes + 4, dtype=np.float64)  # (bits never overlap: sums of byte parts stay below 256)
        acc[:len(header)] += np.frombuffer(header, dtype=np.uint8)
        x, at = v << (off & 7), off >> 3
        for k in range(4):
            acc += np.bincount(at + k, weights=(x >> (8 * k)) & 255, minlength=acc.size)
        acc[n_bytes - 2:n_bytes] = 255
        out.append(acc[:n_bytes].astype(np.uint8).tobytes())
    out.append(b"\x03\x00" + struct.pack(">I", zlib.adler32(b)))
    return b"".join(out)


def png_from_zstream(zstream, H: int, W: int) -> bytes:
    """A ready zlib stream of the H (1 + 3 W) scanline bytes -> the PNG file ``encode`` builds round its own: signature,
    IHDR, one IDAT, IEND.  The stream itself is not checked."""
    return b"".join(_png_parts(zstream, H, W))


def _png_parts(zstream, H: int, W: int) -> list:
    """the file of ``png_from_zstream`` as three buffers, the middle one ``zstream`` itself (the writer's workers hand them to
    the file without joining them: no copy of the stream is made under the GIL)"""
    if H < 1 or W < 1:
        raise ValueError(f"png_from_zstream: {H} x {W}")
    z = memoryview(zstream).cast("B")
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    head = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + struct.pack(">I", z.nbytes) + b"IDAT"
    return [head, z, struct.pack(">I", zlib.crc32(z, zlib.crc32(b"IDAT"))) + _chunk(b"IEND", b"")]


def atomic_write(path, parts) -> int:
    """``parts`` (a buffer or a list of buffers) to ``path`` through a temporary name beside it and a rename, so that no reader
    meets half a file; the temporary file is removed on any failure.  Returns the bytes written."""
    path = pathlib.Path(path)
    parts = parts if isinstance(parts, list) else [parts]
    tmp = path.with_name(f".{path.name}.{os.getpid()}.{threading.get_ident()}.tmp")
    try:
        with open(tmp, "wb") as f:
            f.writelines(parts)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return sum(memoryview(x).nbytes for x in parts)


def _check_scanlines(what, x):
    if x.ndim != 2 or (x.shape[1] - 1) % 3 != 0 or x.shape[1] < 4:
        raise ValueError(f"{what}: scanlines [H,1+3W] expected, got {tuple(x.shape)}")
    if x.dtype not in (torch.uint8, np.dtype(np.uint8)):
        raise ValueError(f"{what}: uint8 expected, got {x.dtype}")


def _as_batch(items):
    """GPU scanlines of one shape -> one tensor [n,H,L]: the view over them where they lie back to back in one allocation
    (the evaluator's export), a stacked copy otherwise"""
    items = [x.contiguous() for x in items]
    first, step = items[0], items[0].numel()
    if all(x.data_ptr() == first.data_ptr() + i * step and x.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
           for i, x in enumerate(items)):
        return first.as_strided((len(items),) + tuple(first.shape), (step,) + tuple(first.stride()))
    return torch.stack(items)


class _DeviceSlot:
    """what one device-deflate call keeps until its files are written: the lengths' pinned landing place and the event"""

    def __init__(self, n: int):
        self.n_host = torch.empty(max(n, 4), dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.left = 0


class AsyncWriter:
    """What ``PngWriter`` and ``video.MjpegWriter`` share: a thread pool whose workers' first exception is kept and raised
    once, at ``close()`` (a second ``close()`` returns quietly), the refusal of work after ``close()``, the ``with`` protocol,
    one copy stream per device, and a worker's fetch of a device-counted run of bytes through pinned memory.  ``n_threads``
    is fixed by the caller (at most ``MAX_THREADS``) and never derived from the machine's CPU count."""

    def __init__(self, n_threads: int, thread_name_prefix: str):
        if not 1 <= int(n_threads) <= MAX_THREADS:
            raise ValueError(f"{type(self).__name__}: n_threads {n_threads} (1 .. {MAX_THREADS})")
        self.n_threads = int(n_threads)
        self._pool = ThreadPoolExecutor(max_workers=self.n_threads, thread_name_prefix=thread_name_prefix)
        self._lock = threading.Lock()
        self._futures = []
        self._error = None
        self._copy_stream = {}
        self._tls = threading.local()
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except BaseException:
            if exc_type is None:
                raise
        return False

    def _check_open(self, what: str) -> None:
        if self._closed:
            raise RuntimeError(f"{what} after close()")

    def _guard(self, fn, *args):
        try:
            fn(*args)
        except BaseException as e:  # kept for close()
            with self._lock:
                if self._error is None:
                    self._error = e

    def _run(self, fn, *args) -> None:
        """``fn(*args)`` on a worker thread; what it raises waits for ``close()``"""
        self._futures.append(self._pool.submit(self._guard, fn, *args))

    def copy_stream(self, device):
        cs = self._copy_stream.get(device.index)
        if cs is None:
            cs = self._copy_stream[device.index] = torch.cuda.Stream(device=device)
        return cs

    def _fetch(self, n, row, stream, refusal):
        """The first ``n`` bytes of the device buffer ``row`` on the host: ``n`` is a count the device wrote, already landed
        in pinned memory, and is refused (``RuntimeError(refusal(n, capacity))``) outside 0 .. ``row.numel()``; the copy runs
        on ``stream`` into this thread's pinned staging buffer, grown as needed, and the stream is synchronised.  The view
        returned is good until this thread's next fetch."""
        n = int(n)
        if not 0 <= n <= row.numel():
            raise RuntimeError(refusal(n, row.numel()))
        with torch.cuda.stream(stream):
            buf = getattr(self._tls, "buf", None)
            if buf is None or buf.numel() < n:
                buf = self._tls.buf = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
            host = buf[:n]
            host.copy_(row[:n], non_blocking=True)
        stream.synchronize()
        return host

    def _drained(self) -> None:
        """what ``close()`` does once every worker has finished (an exception raised here counts as a worker's)"""

    def close(self) -> None:
        """Wait for everything submitted, stop the workers and raise the first exception one of them met."""
        if not self._closed:
            self._closed = True
            for f in self._futures:
                f.result()
            self._futures = []
            self._pool.shutdown(wait=True)
            self._guard(self._drained)
        err, self._error = self._error, None
        if err is not None:
            raise err


class PngWriter(AsyncWriter):
    """Writes scanline buffers as PNG files behind the caller.

    ``submit(path, scanlines)`` takes one image's scanlines [H,1+3W] uint8.  For a GPU tensor it takes a free slot of the ring
    of pinned host buffers (blocking only when all ``n_slots`` are in use), enqueues the device-to-host copy on the writer's
    copy stream behind an event of the current (producing) stream -- or behind ``ready``, an event the producer recorded when
    the scanlines were enqueued, so that the copy does not wait for work enqueued since -- and returns; a worker thread waits for the copy's event,
    deflates, writes the file (temporary name, then rename) and frees the slot.  Host tensors / numpy arrays skip the copy
    stage.  ``close()`` (also on leaving a ``with`` block) drains the pool and re-raises the first worker exception.
    ``n_threads`` is fixed by the caller (default 8, at most ``MAX_THREADS``) and never derived from the machine's CPU
    count.  ``bytes_written`` / ``files_written`` count what reached the disk.

    ``deflate``: "zlib" (the default) is the above in every respect.  "device" applies to GPU scanlines only -- host tensors
    and numpy arrays still go through zlib, byte for byte as under "zlib": ``submit`` makes the copy stream wait as above,
    runs ``ops.png_deflate`` there (segments of ``seg_bytes``, None for ``DEFLATE_SEG_DEFAULT``) and returns; a worker waits
    for the event behind it, reads the stream's length through pinned memory, copies exactly that many bytes, wraps them
    (``png_from_zstream``; the IDAT's CRC-32 is ``zlib.crc32`` here) and writes the file.  The files are valid PNGs with the
    same pixels; their bytes are those of ``deflate_rle``, not zlib's.  A length below 0 or above the capacity raises in
    the worker and surfaces at ``close()``.  A slot then stands for one call's device buffer.
    ``submit_batch(paths, scanlines)``: n images of one size, a tensor [n,H,1+3W] or a sequence of [H,1+3W]; in device mode
    ONE deflate call for GPU scanlines (a view's two or three images), otherwise ``submit`` for each."""

    def __init__(self, n_threads: int = 8, n_slots: int = None, level: int = 1, deflate: str = "zlib", seg_bytes=None):
        if deflate not in DEFLATE_MODES:
            raise ValueError(f"PngWriter: deflate {deflate!r} (one of {DEFLATE_MODES})")
        self.deflate = deflate
        self.seg_bytes = check_seg_bytes(seg_bytes)
        super().__init__(n_threads, "png")
        self.n_slots = int(n_slots) if n_slots is not None else 2 * self.n_threads
        if self.n_slots < 1:
            raise ValueError(f"PngWriter: n_slots {n_slots}")
        self.level = int(level)
        self._free = threading.Semaphore(self.n_slots)
        self._slots = []  # free (pinned buffer, event) pairs
        self._device_slots = []  # free _DeviceSlot objects
        self.bytes_written = 0
        self.files_written = 0

    def _take_slot(self, nbytes: int):
        self._free.acquire()
        with self._lock:
            slot = self._slots.pop() if self._slots else None
        if slot is None or slot[0].numel() < nbytes:
            slot = (torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.cuda.Event())
        return slot

    def _release_slot(self, slot):
        with self._lock:
            self._slots.append(slot)
        self._free.release()

    def _count(self, n_file: int) -> None:
        with self._lock:
            self.bytes_written += n_file
            self.files_written += 1

    def _work(self, path, buf, H, W, slot):
        try:
            if slot is not None:
                slot[1].synchronize()
            self._count(write_file(path, buf, H, W, self.level))
        finally:
            if slot is not None:
                self._release_slot(slot)

    def _work_device(self, path, data, i, H, W, slot):
        try:
            slot.event.synchronize()
            fetch = getattr(self._tls, "fetch", None)  # this worker's own stream
            if fetch is None or fetch.device != data.device:
                fetch = self._tls.fetch = torch.cuda.Stream(device=data.device)
            host = self._fetch(slot.n_host[i], data[i], fetch, lambda n, capacity: (
                f"PngWriter: the device deflate of {path} reports {n} bytes (capacity {capacity})"))
            self._count(atomic_write(path, _png_parts(host.numpy(), H, W)))
        finally:
            with self._lock:
                slot.left -= 1
                done = slot.left == 0
                if done:
                    self._device_slots.append(slot)
            if done:
                self._free.release()

    def _submit_device(self, paths, items, ready) -> None:
        from . import ops

        n, dev = len(items), items[0].device
        H, W = int(items[0].shape[0]), (int(items[0].shape[1]) - 1) // 3
        self._free.acquire()
        with self._lock:
            slot = self._device_slots.pop() if self._device_slots else None
        if slot is None or slot.n_host.numel() < n:
            slot = _DeviceSlot(n)
        try:
            cs = self.copy_stream(dev)
            cs.wait_event(ready if ready is not None else torch.cuda.current_stream(dev).record_event())
            with torch.cuda.stream(cs):
                data, nbytes = ops.png_deflate(_as_batch(items), self.seg_bytes)
                slot.n_host[:n].copy_(nbytes, non_blocking=True)
                slot.event.record(cs)
            for x in items:
                x.record_stream(cs)  # (the allocator may not hand the block out again before the deflate has run)
        except BaseException:
            with self._lock:
                self._device_slots.append(slot)
            self._free.release()
            raise
        slot.left = n
        for i, path in enumerate(paths):
            self._run(self._work_device, path, data, i, H, W, slot)

    def submit_batch(self, paths, scanlines, ready=None) -> None:
        self._check_open("PngWriter.submit_batch")
        paths = list(paths)
        items = [scanlines[i] for i in range(scanlines.shape[0])] if hasattr(scanlines, "shape") else list(scanlines)
        if not paths or len(paths) != len(items):
            raise ValueError(f"PngWriter.submit_batch: {len(paths)} paths for {len(items)} images")
        on_gpu = all(isinstance(x, torch.Tensor) and x.is_cuda for x in items)
        if not (self.deflate == "device" and on_gpu and all(x.shape == items[0].shape and x.device == items[0].device for x in items)):
            for path, x in zip(paths, items):
                self.submit(path, x, ready)
            return
        for x in items:
            _check_scanlines("PngWriter.submit_batch", x)
        self._submit_device(paths, items, ready)

    def submit(self, path, scanlines, ready=None) -> None:
        self._check_open("PngWriter.submit")
        _check_scanlines("PngWriter.submit", scanlines)
        H, W = int(scanlines.shape[0]), (int(scanlines.shape[1]) - 1) // 3
        if isinstance(scanlines, torch.Tensor) and scanlines.is_cuda:
            if self.deflate == "device":
                self._submit_device([path], [scanlines], ready)
                return
            src = scanlines.contiguous().reshape(-1)
            slot = self._take_slot(src.numel())
            try:
                dev = src.device
                cs = self.copy_stream(dev)
                cs.wait_event(ready if ready is not None else torch.cuda.current_stream(dev).record_event())
                host = slot[0][:src.numel()]
                with torch.cuda.stream(cs):
                    host.copy_(src, non_blocking=True)
                    slot[1].record(cs)
                src.record_stream(cs)  # (the allocator may not hand the block out again before the copy has run)
            except BaseException:
                self._release_slot(slot)
                raise
            self._run(self._work, path, host.numpy(), H, W, slot)
            return
        buf = scanlines.numpy() if isinstance(scanlines, torch.Tensor) else np.asarray(scanlines)
        self._run(self._work, path, buf, H, W, None)

    def _drained(self) -> None:
        self._slots = []
        self._device_slots = []
