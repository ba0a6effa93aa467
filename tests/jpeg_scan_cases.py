"""What tests/test_jpeg_scan_host.py and tests/test_gpu_jpeg_scan.py share: the streams added to tests/jpeg_decode_cases.py's
matrix for the scan decoded in subsequences (csrc/jpeg_scan_core.h), the damaged streams, and the two host entries
(``pgdvs_jpeg_scan_prepare``, ``pgdvs_jpeg_scan_decode_host``) through ctypes between guard words.  No tests in here."""
import ctypes as C
import functools

import numpy as np

import jpeg_decode_cases as JC

SUB = 64  # PGDVS_JPEG_SCAN_SUB_BYTES
GROUP = 256  # subsequences of one workgroup
CAP = 1 << 25  # PGDVS_JPEG_SCAN_MAX_BYTES
GUARD = JC.GUARD
SHORT, BAD_CODE, DC_RANGE, NOT_SYNCHRONISED, LEFT_OVER = 1, 2, 4, 8, 16


def scan_extent(data):
    """(first byte of the entropy-coded data, the EOI marker's FF) of a stream this project's parser serves"""
    sos = data.index(b"\xff\xda")
    begin = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    return begin, data.rindex(b"\xff\xd9")


def unstuffed_length(data):
    """bytes of the scan with FF 00 taken as one byte and the RSTn markers taken out: what the subsequences are cut from"""
    begin, end = scan_extent(data)
    scan = data[begin:end]
    n_rst = sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8))
    return len(scan) - scan.count(b"\xff\x00") - 2 * n_rst


def with_trailing(data, extra):
    """``data`` with ``extra`` between its last MCU and EOI (no FF in it: data the decoder never reaches)"""
    _, end = scan_extent(data)
    return data[:end] + extra + data[end:]


def _scan_of_length(want, subsampling=0):
    """a stream without restart markers whose unstuffed scan is exactly ``want`` bytes: the noise image whose scan comes
    nearest from below, then trailing bytes up to it"""
    best = None
    for side in (8, 16):
        for quality in (5, 10, 20, 30, 50, 75, 90):
            data = JC.encode(JC.content("noise", side, side, 7), subsampling, quality)
            n = unstuffed_length(data)
            if n <= want and (best is None or n > best[0]):
                best = (n, data)
    assert best is not None and best[0] > want // 2, (want, best and best[0])
    return with_trailing(best[1], b"\x00" * (want - best[0]))


@functools.lru_cache(maxsize=None)
def added():
    """[(label, stream)]: where reading a scan in subsequences can go wrong"""
    out = [("1x1", JC.encode(JC.content("noise", 1, 1), 2, 90)), ("8x8", JC.encode(JC.content("smooth", 8, 8), 0, 50))]
    for label, n in (("one subsequence", SUB), ("two subsequences less one byte", 2 * SUB - 1), ("two subsequences and one byte", 2 * SUB + 1)):
        out.append((f"scan of exactly {label}", _scan_of_length(n)))
    noise = JC.content("noise", 256, 384, 11)
    out.append(("256x384 noise q100 4:4:4: more than two workgroups", JC.encode(noise, 0, 100)))
    out.append(("96x128 noise q100 4:4:4 optimize: 16-bit codes", JC.encode(noise[:96, :128], 0, 100, None, True)))
    out.append(("restart interval 1", JC.encode(JC.content("noise", 40, 56, 3), 2, 90, 1)))
    out.append(("restart interval 1, smooth 4:4:4", JC.encode(JC.content("smooth", 33, 49, 3), 0, 75, 1)))
    out.append(("restart interval larger than the image", JC.encode(JC.content("noise", 24, 33, 4), 1, 90, 1000)))
    flat = np.full((200, 300, 3), 97, np.uint8)
    flat[50:60, 70:90] = 180
    out.append(("smooth: almost every block is EOB", JC.encode(flat, 2, 50)))
    out.append(("noise q100: blocks end on coefficient 63", JC.encode(JC.content("noise", 64, 64, 5), 0, 100)))
    out.append(("trailing bytes in front of EOI", with_trailing(JC.encode(JC.content("smooth", 40, 56, 6), 2, 80), bytes(range(1, 250)) * 3)))
    out.append(("trailing bytes, restart interval 3", with_trailing(JC.encode(JC.content("noise", 33, 49, 6), 0, 80, 3), b"\x12\x34" * 200)))
    return out


def fuzz_streams():
    """the three streams of the sanitizer run of tests/test_jpeg_decode_host.py"""
    return {"s420.jpg": JC.small_stream(), "s444_rst.jpg": JC.encode(JC.content("noise", 10, 19), 0, 60, 1),
            "s422_opt.jpg": JC.encode(JC.content("smooth", 17, 23), 1, 90, None, True)}


def mutations(data, n, seed):
    """``n`` copies of ``data`` with one byte replaced, seeded"""
    rng = np.random.default_rng(seed)
    at, val = rng.integers(0, len(data), n), rng.integers(0, 256, n)
    for a, v in zip(at.tolist(), val.tolist()):
        yield data[:a] + bytes([v]) + data[a + 1:]


def oversized():
    """a served stream whose scan is one byte above the cap: a small image, then zeros in front of EOI"""
    data = JC.small_stream()
    begin, end = scan_extent(data)
    return with_trailing(data, b"\x00" * (CAP + 1 - (end - begin)))


# ---------------------------------------------------------------------------- the host entries
def prepare(data, sub_bytes=0):
    """``pgdvs_jpeg_scan_prepare`` into a buffer of exactly the queried size between guard bytes -> (rc, uint8 array or None,
    JpegInfo, message); the guards are checked here"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    ptr = C.c_void_p(buf.ctypes.data if buf.size else 0)
    info = _lib.JpegInfo()
    need = lib.pgdvs_jpeg_scan_prepare_bytes(ptr, buf.size, sub_bytes)
    if need <= 0:
        return (1 if need == 0 else -1), None, info, lib.pgdvs_last_error().decode()
    assert need % 8 == 0
    mem = np.full(64 + need + 64, 0xA5, np.uint8)
    off = (-mem.ctypes.data) % 16 + 16
    prepared = mem[off:off + need]
    rc = lib.pgdvs_jpeg_scan_prepare(ptr, buf.size, sub_bytes, C.c_void_p(prepared.ctypes.data), need, C.byref(info))
    assert (mem[:off] == 0xA5).all() and (mem[off + need:] == 0xA5).all(), "written outside the prepared buffer"
    return rc, (prepared if rc == 0 else None), info, lib.pgdvs_last_error().decode()


def header(prepared):
    from pgdvs_amd import _lib

    return _lib.JpegScanHeader.from_buffer_copy(prepared[:C.sizeof(_lib.JpegScanHeader)].tobytes())


def decode_host(prepared, coef_bytes):
    """``pgdvs_jpeg_scan_decode_host`` with coef and the workspace between guard words -> (status, int16 array, (rounds of the
    first launch, fix-up launches that ran)); the guards are checked here"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    p = C.c_void_p(prepared.ctypes.data)
    need = lib.pgdvs_jpeg_scan_decode_workspace_bytes(p, prepared.size)
    assert need > 0, lib.pgdvs_last_error()
    mem = np.full(GUARD + coef_bytes // 2 + GUARD, 0x5A5A, np.int16)
    coef = mem[GUARD:GUARD + coef_bytes // 2]
    wmem = np.full(need // 8 + 2 * GUARD, 0x5A5A5A5A5A5A5A5A, np.uint64)
    ws = wmem[GUARD:GUARD + need // 8]
    status = np.full(3, 0x5A5A5A5A, np.uint32)
    rc = lib.pgdvs_jpeg_scan_decode_host(p, p, prepared.size, C.c_void_p(coef.ctypes.data), coef_bytes, C.c_void_p(status[1:].ctypes.data),
                                         C.c_void_p(ws.ctypes.data), need)
    assert rc == 0, (rc, lib.pgdvs_last_error())
    assert (mem[:GUARD] == 0x5A5A).all() and (mem[GUARD + coef_bytes // 2:] == 0x5A5A).all(), "written outside coef"
    assert (wmem[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (wmem[GUARD + need // 8:] == 0x5A5A5A5A5A5A5A5A).all(), "written outside the workspace"
    assert status[0] == status[2] == 0x5A5A5A5A, "written outside the status word"
    words = ws.view(np.uint32)  # (the workspace's first two words)
    return int(status[1]), coef, (int(words[0]), int(words[1]))


def check_against_host_decoder(label, data, sub_bytes=0, intact=True):
    """The emulation against ``pgdvs_jpeg_entropy_decode``.  ``intact``: status 0 and equal coefficients are demanded;
    otherwise a stream the host decoder refuses must give a non-zero status (or be refused by the preparation), and one it
    serves either equal coefficients or a non-zero status.  Returns (status or None, rounds)."""
    rc_p, info, msg = JC.parse(data)
    rc, prepared, info2, msg2 = prepare(data, sub_bytes)
    assert rc in (0, 1), (label, rc, msg2)
    if rc_p != 0:
        assert rc == 1 and msg2 == msg, (label, rc, msg, msg2)
        return None, None
    if rc == 1:
        assert not intact, (label, msg2)
        return None, None
    assert bytes(info2) == bytes(info), label
    rc_h, want, msg_h = JC.entropy_decode(data, info.coef_bytes)
    status, got, rounds = decode_host(prepared, info.coef_bytes)
    if intact:
        assert rc_h == 0, (label, msg_h)
        assert status == 0, (label, status, "not synchronised" if status & NOT_SYNCHRONISED else "")
    assert not status & NOT_SYNCHRONISED, (label, status)
    if rc_h != 0:
        assert status != 0, (label, msg_h, "the host decoder refuses this scan, the emulation serves it")
    elif status == 0:
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, bad.size, bad[:6].tolist())
    return status, rounds
