"""Helpers of the video tests (test_video_host.py, test_video_420_host.py, test_gpu_video.py, test_gpu_video_420.py), written
out independently of pgdvs_amd.video and csrc/jpeg.hip: a RIFF walker, a parser of the DHT / DQT segments of a PIL-written
JPEG, the float64 decode model of a coefficient array, the crafted coefficient blocks and the inputs the test files share.
Not a test."""
import io
import pathlib
import struct

import numpy as np
import PIL.Image
from scipy.fft import idctn

# T.81 Figure A.6: NATURAL[i] = row-major index of the i-th coefficient of the zigzag sequence
NATURAL = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

SIZES = [(1, 1), (8, 8), (9, 17), (37, 53), (24, 40)]


# ---- RIFF ----------------------------------------------------------------------------------------------------------------------
class Chunk:
    def __init__(self, tag, offset, size, form=None, children=None, data=None):
        self.tag, self.offset, self.size, self.form, self.children, self.data = tag, offset, size, form, children, data

    def find(self, tag, form=None):
        return [c for c in self.children if c.tag == tag and (form is None or c.form == form)]


def _walk(raw, start, end):
    out, pos = [], start
    while pos < end:
        assert pos + 8 <= end, ("chunk header past its parent", pos, end)
        tag, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body, stop = pos + 8, pos + 8 + size
        assert stop <= end, ("chunk past its parent", tag, pos, size, end)
        if tag in (b"RIFF", b"LIST"):
            assert size >= 4
            out.append(Chunk(tag, pos, size, form=raw[body:body + 4], children=_walk(raw, body + 4, stop)))
        else:
            out.append(Chunk(tag, pos, size, data=raw[body:stop]))
        pos = stop + (size & 1)  # chunks start on even offsets
        if size & 1 and pos <= end:
            assert raw[stop] == 0, ("pad byte", tag, pos)
    assert pos == end, ("children do not fill their parent", pos, end)
    return out


def riff(raw: bytes) -> Chunk:
    """the whole file as one RIFF chunk; asserts that every size field is consistent and every odd chunk padded"""
    top = _walk(raw, 0, len(raw))
    assert len(top) == 1 and top[0].tag == b"RIFF", [c.tag for c in top]
    return top[0]


def avi_frames(raw: bytes):
    """the walker's view of a file: (top chunk, the payloads of movi's 00dc chunks)"""
    top = riff(raw)
    assert top.form == b"AVI " and top.size == len(raw) - 8
    movi = top.find(b"LIST", b"movi")[0]
    assert all(c.tag == b"00dc" for c in movi.children)
    return top, [c.data for c in movi.children]


def avi_file_frames(path) -> list:
    return avi_frames(pathlib.Path(path).read_bytes())[1]


# ---- PIL's tables ----------------------------------------------------------------------------------------------------------------
def pil_jpeg(q_hwc: np.ndarray, quality: int, **kw) -> bytes:
    b = io.BytesIO()
    PIL.Image.fromarray(q_hwc).save(b, "JPEG", quality=quality, subsampling=0, **kw)
    return b.getvalue()


def segments(data: bytes):
    """(marker, payload) of every segment in front of the scan data"""
    assert data[:2] == b"\xff\xd8"
    i, out = 2, []
    while True:
        assert data[i] == 0xFF, i
        m, L = data[i + 1], struct.unpack_from(">H", data, i + 2)[0]
        out.append((m, data[i + 4:i + 2 + L]))
        i += 2 + L
        if m == 0xDA:
            return out, i


def parse_dht(data: bytes) -> dict:
    """{class << 4 | id: (BITS[16], HUFFVAL)} of all DHT segments"""
    out = {}
    for m, seg in segments(data)[0]:
        if m != 0xC4:
            continue
        j = 0
        while j < len(seg):
            tc, bits = seg[j], list(seg[j + 1:j + 17])
            n = sum(bits)
            out[tc] = (bits, list(seg[j + 17:j + 17 + n]))
            j += 17 + n
    return out


def parse_dqt(data: bytes) -> dict:
    """{id: 64 entries in the order of the file (zigzag)} of all DQT segments (8-bit tables)"""
    out = {}
    for m, seg in segments(data)[0]:
        if m != 0xDB:
            continue
        j = 0
        while j < len(seg):
            assert seg[j] >> 4 == 0
            out[seg[j] & 15] = list(seg[j + 1:j + 65])
            j += 65
    return out


def decode_pil(data: bytes):
    with PIL.Image.open(io.BytesIO(data)) as im:
        im.load()
        return im.mode, im.size, np.asarray(im).copy()


# ---- the decode model ------------------------------------------------------------------------------------------------------------
def decode_model(coef, q_luma, q_chroma, H, W) -> np.ndarray:
    """coef[nby,nbx,3,64] (zigzag; DC within -1024 .. 1023, AC within +-1023: what the coder clamps to) -> float64 RGB
    [H,W,3], rounded and clamped: dequantise, exact inverse DCT, + 128, round, clamp per plane, JFIF inverse colour, round,
    clamp."""
    coef = np.asarray(coef).astype(np.int64)
    coef = np.concatenate([np.clip(coef[..., :1], -1024, 1023), np.clip(coef[..., 1:], -1023, 1023)], axis=-1)
    nby, nbx = coef.shape[:2]
    planes = []
    for c in range(3):
        Q = np.asarray(q_luma if c == 0 else q_chroma, dtype=np.float64).reshape(64)
        nat = np.zeros((nby, nbx, 64))
        nat[..., NATURAL] = coef[:, :, c, :]
        px = idctn((nat * Q).reshape(nby, nbx, 8, 8), axes=(-2, -1), norm="ortho")
        px = px.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)[:H, :W]
        planes.append(np.clip(np.rint(px + 128.0), 0, 255))
    Y, Cb, Cr = planes[0], planes[1] - 128.0, planes[2] - 128.0
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255)


def psnr(a, b) -> float:
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return 10.0 * np.log10(255.0 ** 2 / max(mse, 1e-12))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def contents(H, W):
    """name -> uint8 [H,W,3]: the synthetic render (cropped from a larger one: its generator needs room), byte noise, a
    constant and a one-pixel checkerboard"""
    from pgdvs_amd import synth

    big = synth.make_video(1, max(H, 48), max(W, 64), seed=5)["rgbs"][0]
    render = (np.clip(big[:H, :W], 0.0, 1.0).astype(np.float32) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    noise = np.random.default_rng(100 * H + W).integers(0, 256, (H, W, 3)).astype(np.uint8)
    const = np.empty((H, W, 3), np.uint8)
    const[...] = (200, 30, 120)
    checker = np.repeat((((np.add.outer(np.arange(H), np.arange(W)) % 2) * 255).astype(np.uint8))[..., None], 3, axis=2)
    return {"render": render, "noise": noise, "constant": const, "checker": checker}


def float_inputs(B, H, W):
    """(name, float32 [B,3,H,W]): seeded noise over [0, 1), a synthetic render (cropped from one with room for its objects),
    the value table tiled (values outside [0, 1], NaN, +-inf included)"""
    import torch
    import vis_reference as VR
    from pgdvs_amd import synth

    g = torch.Generator().manual_seed(1000 * H + W + B)
    yield "noise", torch.rand((B, 3, H, W), generator=g)
    video = synth.make_video(B, max(H, 48), max(W, 64), seed=5)
    yield "render", torch.from_numpy(np.ascontiguousarray(video["rgbs"][:, :H, :W])).permute(0, 3, 1, 2).contiguous()
    yield "table", VR.table_image(H, W).repeat(B, 1, 1, 1)


def host_coef(x, quality, subsampling="4:4:4"):
    """the host restatement's coefficients of the float batch x[B,3,H,W], quantised as ``*_combined.png`` is"""
    from pgdvs_amd import png, video

    q = png.quantize_save_image(x).permute(0, 2, 3, 1).contiguous().numpy()
    return np.stack([video.jpeg_coefficients(v, quality, subsampling=subsampling) for v in q])


def _block(entries):
    b = np.zeros(64, dtype=np.int16)
    for k, v in entries.items():
        b[k] = v
    return b


def crafted_blocks() -> dict:
    """name -> one block's 64 coefficients in zigzag order, each built round one edge of the entropy coder.  A zero run of n
    is n zeros between coefficient 1 and the next non-zero one."""
    out = {
        "zero": _block({}),
        "only63": _block({63: 5}),
        "last_nonzero_no_eob": _block({0: 40, 1: -3, 30: 7, 63: -1}),
        "ac_pm1": _block({0: -7, 1: 1, 2: -1, 5: 1, 6: -1}),
        "ac_p1023": _block({0: 10, 3: 1023}),
        "ac_m1023": _block({0: -10, 4: -1023}),
        "dense": _block({k: (k % 7) - 3 for k in range(64)}),
    }
    for n in (15, 16, 17, 32, 48):
        out[f"run{n}"] = _block({0: 3, 1: 2, 2 + n: -2, 63: 0})
    out["runs_to_the_end"] = _block({0: -100, 1: 9, 18: 1, 35: -1, 52: 1})  # ZRL, ZRL ..., then EOB after 52
    return out


def crafted_frame(name_or_block, n_mcu=2):
    """[1,n_mcu,3,64]: the block as Y, Cb and Cr of every MCU (the chroma planes keep the AC and a third of the DC)"""
    b = crafted_blocks()[name_or_block] if isinstance(name_or_block, str) else name_or_block
    coef = np.zeros((1, n_mcu, 3, 64), dtype=np.int16)
    coef[:, :, 0] = b
    coef[:, :, 1] = b
    coef[:, :, 1, 0] = b[0] // 3
    coef[:, :, 2, 0] = -(b[0] // 3)
    return coef


def dc_step_frame(n_mcu=6):
    """DC + 1020, - 1020, + 1020 ... from MCU to MCU in every component: differences of +-2040, size category 11"""
    coef = np.zeros((1, n_mcu, 3, 64), dtype=np.int16)
    sign = np.where(np.arange(n_mcu) % 2 == 0, 1, -1)
    for c in range(3):
        coef[0, :, c, 0] = 1020 * sign * (1 if c != 1 else -1)
    return coef


def crafted_grid(nby, nbx, seed=0):
    """[nby,nbx,3,64]: the crafted blocks, the DC steps, values beyond the coder's clamps and seeded sparse noise, dealt over
    the grid's blocks so that every component and every position in a restart segment meets several of them"""
    rng = np.random.default_rng(seed)
    pool = list(crafted_blocks().values())
    pool += [_block({0: 1020}), _block({0: -1020}), _block({0: 1023}), _block({0: -1024}), _block({0: 2000, 1: 5000, 63: -5000}),
             _block({0: -32768, 7: 32767, 8: -32768}), _block({k: 1023 if k % 2 else -1023 for k in range(64)})]
    for _ in range(6):
        sparse = rng.integers(-1023, 1024, 64) * (rng.random(64) < 0.15)
        sparse[0] = rng.integers(-1024, 1024)
        pool.append(sparse.astype(np.int16))
    n = nby * nbx * 3
    order = np.concatenate([rng.permutation(len(pool)) for _ in range(n // len(pool) + 1)])[:n]
    return np.stack([pool[i] for i in order]).reshape(nby, nbx, 3, 64).astype(np.int16)
