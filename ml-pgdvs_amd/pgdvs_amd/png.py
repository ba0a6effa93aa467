"""PNG export of rendered views without PIL on the write path (the visualiser's two writers,
pgdvs/engines/visualizer_pgdvs.py:118-139).

A PNG is filtered scanlines (per row one filter-type byte and the row's bytes, each predicted from its left / upper
neighbours) under one zlib stream.  On the GPU the quantisation and the filtering are one HIP pass
(``ops.png_scanlines``, csrc/png.hip); this module holds the same two steps in torch / numpy for host images, the
container (``encode``), and ``PngWriter``: a ring of pinned host buffers and a small thread pool that copies, deflates
and writes behind the thread that drives the GPU (zlib releases the GIL)."""
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
    path = pathlib.Path(path)
    data = encode(scanlines, H, W, level)
    tmp = path.with_name(f".{path.name}.{os.getpid()}.{threading.get_ident()}.tmp")
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return len(data)


class PngWriter:
    """Writes scanline buffers as PNG files behind the caller.

    ``submit(path, scanlines)`` takes one image's scanlines [H,1+3W] uint8.  For a GPU tensor it takes a free slot of the ring
    of pinned host buffers (blocking only when all ``n_slots`` are in use), enqueues the device-to-host copy on the writer's
    copy stream behind an event of the current (producing) stream -- or behind ``ready``, an event the producer recorded when
    the scanlines were enqueued, so that the copy does not wait for work enqueued since -- and returns; a worker thread waits for the copy's event,
    deflates, writes the file (temporary name, then rename) and frees the slot.  Host tensors / numpy arrays skip the copy
    stage.  ``close()`` (also on leaving a ``with`` block) drains the pool and re-raises the first worker exception.
    ``n_threads`` is fixed by the caller (default 8, at most ``MAX_THREADS``) and never derived from the machine's CPU
    count.  ``bytes_written`` / ``files_written`` count what reached the disk."""

    def __init__(self, n_threads: int = 8, n_slots: int = None, level: int = 1):
        if not 1 <= int(n_threads) <= MAX_THREADS:
            raise ValueError(f"PngWriter: n_threads {n_threads} (1 .. {MAX_THREADS})")
        self.n_threads = int(n_threads)
        self.n_slots = int(n_slots) if n_slots is not None else 2 * self.n_threads
        if self.n_slots < 1:
            raise ValueError(f"PngWriter: n_slots {n_slots}")
        self.level = int(level)
        self._pool = ThreadPoolExecutor(max_workers=self.n_threads, thread_name_prefix="png")
        self._free = threading.Semaphore(self.n_slots)
        self._lock = threading.Lock()
        self._slots = []  # free (pinned buffer, event) pairs
        self._futures = []
        self._error = None
        self._copy_stream = {}
        self._closed = False
        self.bytes_written = 0
        self.files_written = 0

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except BaseException:
            if exc_type is None:
                raise
        return False

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

    def _work(self, path, buf, H, W, slot):
        try:
            if slot is not None:
                slot[1].synchronize()
            n = write_file(path, buf, H, W, self.level)
            with self._lock:
                self.bytes_written += n
                self.files_written += 1
        except BaseException as e:  # kept for close()
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            if slot is not None:
                self._release_slot(slot)

    def submit(self, path, scanlines, ready=None) -> None:
        if self._closed:
            raise RuntimeError("PngWriter.submit after close()")
        if scanlines.ndim != 2 or (scanlines.shape[1] - 1) % 3 != 0 or scanlines.shape[1] < 4:
            raise ValueError(f"PngWriter.submit: scanlines [H,1+3W] expected, got {tuple(scanlines.shape)}")
        H, W = int(scanlines.shape[0]), (int(scanlines.shape[1]) - 1) // 3
        if isinstance(scanlines, torch.Tensor) and scanlines.is_cuda:
            if scanlines.dtype != torch.uint8:
                raise ValueError(f"PngWriter.submit: uint8 expected, got {scanlines.dtype}")
            src = scanlines.contiguous().reshape(-1)
            slot = self._take_slot(src.numel())
            try:
                dev = src.device
                cs = self._copy_stream.get(dev.index)
                if cs is None:
                    cs = self._copy_stream[dev.index] = torch.cuda.Stream(device=dev)
                cs.wait_event(ready if ready is not None else torch.cuda.current_stream(dev).record_event())
                host = slot[0][:src.numel()]
                with torch.cuda.stream(cs):
                    host.copy_(src, non_blocking=True)
                    slot[1].record(cs)
                src.record_stream(cs)  # (the allocator may not hand the block out again before the copy has run)
            except BaseException:
                self._release_slot(slot)
                raise
            self._futures.append(self._pool.submit(self._work, path, host.numpy(), H, W, slot))
            return
        buf = scanlines.numpy() if isinstance(scanlines, torch.Tensor) else np.asarray(scanlines)
        if buf.dtype != np.uint8:
            raise ValueError(f"PngWriter.submit: uint8 expected, got {buf.dtype}")
        self._futures.append(self._pool.submit(self._work, path, buf, H, W, None))

    def close(self) -> None:
        """Wait for every submitted file, stop the workers and raise the first exception one of them met."""
        if not self._closed:
            self._closed = True
            for f in self._futures:
                f.result()
            self._futures = []
            self._pool.shutdown(wait=True)
            self._slots = []
        err, self._error = self._error, None
        if err is not None:
            raise err
