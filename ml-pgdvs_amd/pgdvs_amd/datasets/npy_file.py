"""Where a depth file keeps its floats: the one reader of ``.npy`` headers and of stored ``.npz`` members.

``device_depth`` sends a file's bytes across the bus as stored, so the host only has to find the payload: no array is made and
no pixel is touched here.  Both functions return ``(offset, shape, reason)``: the payload's byte offset in ``data`` and the
array's shape where the file is one the device path serves -- little-endian float32 in C order, the payload complete -- and
``(None, None, reason)`` for every other input.  They never raise for a file they do not serve: the caller then runs the
loader's own host statement (``np.load`` ...), and that statement decides what a bad file means."""
import ast
import io
import math
import struct
import zipfile

MAGIC = b"\x93NUMPY"
SERVED_DESCR = "<f4"


def npy_payload(data, start=0, end=None):
    """``(offset, shape, None)`` of the ``.npy`` file in ``data[start:end]`` (format 1.0, 2.0 or 3.0) whose ``descr`` is ``'<f4'``,
    whose ``fortran_order`` is False and whose payload of ``prod(shape) * 4`` bytes lies inside; else ``(None, None, reason)``"""
    try:
        end = len(data) if end is None else min(int(end), len(data))
        head = bytes(data[start:start + 12])
        if len(head) < 10 or head[:6] != MAGIC:
            return None, None, "not an .npy file (no magic string)"
        version = (head[6], head[7])
        if version == (1, 0):
            (hlen,), at = struct.unpack("<H", head[8:10]), start + 10
        elif version in ((2, 0), (3, 0)):
            if len(head) < 12:
                return None, None, "the header is cut short"
            (hlen,), at = struct.unpack("<I", head[8:12]), start + 12
        else:
            return None, None, f"format version {version[0]}.{version[1]} (1.0, 2.0 and 3.0 are read)"
        if at + hlen > end:
            return None, None, "the header is cut short"
        header = ast.literal_eval(bytes(data[at:at + hlen]).decode("utf-8" if version == (3, 0) else "latin1"))
        if not isinstance(header, dict) or set(header) != {"descr", "fortran_order", "shape"}:
            return None, None, "the header is no dict of descr, fortran_order and shape"
        descr, fortran, shape = header["descr"], header["fortran_order"], header["shape"]
        if descr != SERVED_DESCR:
            return None, None, f"descr {descr!r} ({SERVED_DESCR!r} is served)"
        if fortran is not False:
            return None, None, "Fortran order"
        if not isinstance(shape, tuple) or not all(type(s) is int and s >= 0 for s in shape):
            return None, None, f"shape {shape!r}"
        offset, nbytes = at + hlen, math.prod(shape) * 4
        if offset + nbytes > end:
            return None, None, f"the payload is cut short ({end - offset} of {nbytes} bytes)"
        return offset, shape, None
    except Exception as e:  # (a header that is no Python literal, no text ...)
        return None, None, f"unreadable header: {type(e).__name__}: {e}"


def npz_member(data, name):
    """``npy_payload`` of the member ``name + ".npy"`` of the ``.npz`` archive ``data``, where the member is stored (method 0)
    and not encrypted.  The payload's place follows from the LOCAL header's own name and extra lengths: ``np.savez`` writes a
    zip64 extra field there that the central directory does not show."""
    try:
        with zipfile.ZipFile(io.BytesIO(data)) as z:
            info = z.getinfo(name + ".npy")
        if info.compress_type != zipfile.ZIP_STORED:
            return None, None, f"member {name!r} is compressed (method {info.compress_type}; stored members are served)"
        if info.flag_bits & 1:
            return None, None, f"member {name!r} is encrypted"
        local = bytes(data[info.header_offset:info.header_offset + 30])
        if len(local) < 30 or local[:4] != b"PK\x03\x04":
            return None, None, f"member {name!r}: no local header where the directory points"
        n, m = struct.unpack("<HH", local[26:30])
        start = info.header_offset + 30 + n + m
        if start + info.file_size > len(data):
            return None, None, f"member {name!r} is cut short"
        return npy_payload(data, start, start + info.file_size)
    except KeyError:
        return None, None, f"no member {name!r}"
    except Exception as e:  # (BadZipFile, a damaged directory ...)
        return None, None, f"unreadable archive: {type(e).__name__}: {e}"
