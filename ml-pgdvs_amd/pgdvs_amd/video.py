"""The visualiser's video without ffmpeg: a Motion-JPEG AVI in place of ``<scene_id>_combined.mp4``
(pgdvs/engines/visualizer_pgdvs.py:141-177, pgdvs/utils/rendering.py:79-116 ``images_to_video(..., fps=10, quality=9)``).

It is a substitute for the mp4, not an mp4: every frame is an independent baseline JPEG (8 bit, 4:4:4 or on request 4:2:0, one interleaved
scan, the four standard Huffman tables, IJG quality scaling of the Annex K tables) inside a RIFF AVI with an ``idx1``
index.  imageio's ``quality=9`` has no counterpart here; ``quality`` is libjpeg's 1..100.

The codec is defined in integers so that this module and csrc/jpeg.hip agree byte for byte:

  pixels    ``png.quantize_save_image`` (the 8-bit image of ``*_combined.png``), edges replicated to whole 8 x 8 blocks
  colour    JFIF's 16-bit fixed point as libjpeg computes it, then - 128
  DCT       the 13-bit integer DCT of Loeffler, Ligtenberg and Moschytz in the Independent JPEG Group's scaling (``fdct_int``):
            rows, then columns; the result is 8 x the coefficient
  quantise  one rounding: sign(c) ((|c| + 4 Q) // (8 Q)), int16 in zigzag order: coef[nby, nbx, 3, 64].  Colour, DCT and
            quantiser are libjpeg's: at the same tables and 4:4:4 PIL writes the same scan bytes
  entropy   per block: DC difference to the previous block of the component (0 after a restart), AC run / size symbols,
            ZRL, EOB; per restart segment: bits padded with ones, 0xFF -> 0xFF 0x00, RSTm between segments.  On read DC is
            clamped to -1024 .. 1023 and AC to +-1023, so that every symbol exists in the standard tables (a DC difference
            is then at most 2047, category 11).

``subsampling="4:2:0"`` (the default stays "4:4:4") is upstream's chroma format -- imageio's ffmpeg writer without a
``pixelformat`` writes yuv420p -- and the same codec with a 16 x 16 MCU of six blocks, Y00 Y01 Y10 Y11 Cb Cr:
coef[nmy, nmx, 6, 64] with nmy = ceil(H / 16), nmx = ceil(W / 16).  Its edges are libjpeg's, and PIL writes the same scan
bytes at ``subsampling=2`` (nby = ceil(H / 8), nbx = ceil(W / 8)):

  columns   beyond W - 1 replicate column W - 1 out to 16 nmx; quantisation and colour transform as at 4:4:4
  luma      a block with block column < nbx and block row < nby is coded as at 4:4:4 (rows beyond H - 1 replicate row H - 1).
            Every other luma block of the MCU is a dummy: 63 zero AC coefficients and a QUANTISED DC copied inside the MCU --
            a right-edge dummy (column >= nbx) takes its left neighbour's (Y01 from Y00, Y11 from Y10); a bottom dummy row
            (row >= nby) gives both its blocks the DC of Y01, the block in front of the row in MCU order, dummy or not, and
            wins over the right-edge rule.  Dummies are entropy-coded like any block: a DC difference, then EOB
  chroma    sample (j, i), j < ceil(H / 2): (a + b + c + d + bias) >> 2 over rows min(2j, H-1), min(2j+1, H-1) and columns
            2i, 2i+1 of the column-replicated Cb (Cr) plane, bias 1 for even i and 2 for odd i, then - 128.  Rows
            j >= ceil(H / 2) replicate the DOWNSAMPLED row ceil(H / 2) - 1.  No dummy blocks: ceil(ceil(W / 2) / 8) = nmx
  entropy   luma tables for blocks 0 .. 3, chroma tables for 4 and 5; DC prediction per component in stream order: Y from
            the previous Y block (across MCUs), Cb from the previous Cb, Cr from the previous Cr, all 0 at a restart.
            ``restart_mcus`` counts 16 x 16 MCUs
  header    SOF0 sampling 2x2 for Y, 1x1 for Cb and Cr; DRI in MCUs; the rest as at 4:4:4

``jpeg_coefficients`` / ``encode_scan`` are the host restatement (numpy integers; the fallback for host tensors, not
meant to be fast), ``ops.jpeg_coefficients`` / ``ops.jpeg_scan`` the HIP path.  ``jpeg_frame`` puts the headers round a
scan, ``write_avi`` the container round the frames, ``MjpegWriter`` does both behind the thread that drives the GPU.

The container is checked structurally and frame by frame with PIL; it has not been opened in a player."""
from __future__ import annotations

import pathlib
import struct

import numpy as np
import torch

from . import png

# ---- tables ----------------------------------------------------------------------------------------------------------------
# ITU-T T.81 Annex K.1, natural (row-major) order
QUANT_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], dtype=np.int64)
QUANT_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, dtype=np.int64)

# ITU-T T.81 Annex K.3: (class << 4 | id) -> (BITS[16], HUFFVAL); class 0 DC, 1 AC; id 0 luminance, 1 chrominance
_AC_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]  # only used to check the lists below are complete
HUFFMAN = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
        0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
        0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
        0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
        0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
        0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
        0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
        0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
        0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
        0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
        0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
        0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
        0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
}
assert all(sum(b) == len(v) for b, v in HUFFMAN.values()) and all(set(_AC_TAIL) <= set(HUFFMAN[t][1]) for t in (0x10, 0x11))

# ZIGZAG[i] = the natural (row-major) index of the i-th coefficient of the zigzag sequence
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8)), dtype=np.int64)

# the 13-bit constants of the forward DCT (Loeffler, Ligtenberg, Moschytz 1989, as the Independent JPEG Group's slow-but-
# accurate integer DCT scales them): rint(8192 x) of the named values
DCT_BITS, DCT_PASS1_BITS = 13, 2
DCT_FIX = {name: int(np.rint(float(name) * 8192)) for name in (
    "0.298631336", "0.390180644", "0.541196100", "0.765366865", "0.899976223", "1.175875602", "1.501321110", "1.847759065",
    "1.961570560", "2.053119869", "2.562915447", "3.072711026")}

DC_MIN, DC_MAX, AC_MAX = -1024, 1023, 1023
BLOCK_MAX_BYTES = 416  # 20 bits of DC + 63 x 26 bits of AC = 1658 bits -> 208 bytes, doubled by stuffing


def quant_tables(quality: int):
    """IJG's quality rule on the Annex K pair -> (luma[64], chroma[64]) int64 in natural order: scale = 5000 // q below 50,
    else 200 - 2 q; (base scale + 50) // 100 clamped to 1 .. 255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quant_tables: quality {quality} (1 .. 100)")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (QUANT_LUMA, QUANT_CHROMA))


SUBSAMPLINGS = ("4:4:4", "4:2:0")
BLOCKS_PER_MCU = {"4:4:4": 3, "4:2:0": 6}
MCU_SIZE = {"4:4:4": 8, "4:2:0": 16}


def check_subsampling(subsampling) -> str:
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r} ('4:4:4' or '4:2:0')")
    return subsampling


def mcu_grid(H: int, W: int, subsampling="4:4:4"):
    """(MCU rows, MCU columns) of an H x W frame: MCUs of 8 x 8 pixels at 4:4:4, of 16 x 16 at 4:2:0"""
    m = MCU_SIZE[check_subsampling(subsampling)]
    return (int(H) + m - 1) // m, (int(W) + m - 1) // m


def default_restart(nbx: int) -> int:
    """The default restart interval: one MCU row (``nbx``: the MCUs in a row of the layout at hand)."""
    return int(nbx)


def _resolve_restart(restart_mcus, nbx):
    r = default_restart(nbx) if restart_mcus is None else int(restart_mcus)
    if not 0 <= r <= 65535:
        raise ValueError(f"restart_mcus {restart_mcus} (0 .. 65535)")
    return r


# ---- colour, DCT, quantisation ---------------------------------------------------------------------------------------------
def rgb_to_ycc(rgb: np.ndarray) -> np.ndarray:
    """uint8 [...,3] -> int64 [...,3] Y, Cb, Cr in 0 .. 255 (JFIF, 16-bit fixed point)"""
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16
    return np.stack([Y, Cb, Cr], axis=-1)


def _fdct_1d(d, first: bool):
    """one pass of the DCT along the last axis of d[...,8] (int64).  The first pass leaves its results scaled up by
    2^DCT_PASS1_BITS, the second removes that scale again but for a factor of 8 overall."""
    F = DCT_FIX
    half = lambda x, n: (x + (1 << (n - 1))) >> n  # noqa: E731
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = DCT_BITS - DCT_PASS1_BITS if first else DCT_BITS + DCT_PASS1_BITS
    if first:
        o0, o4 = (t10 + t11) << DCT_PASS1_BITS, (t10 - t11) << DCT_PASS1_BITS
    else:
        o0, o4 = half(t10 + t11, DCT_PASS1_BITS), half(t10 - t11, DCT_PASS1_BITS)
    z1 = (t12 + t13) * F["0.541196100"]
    o2 = half(z1 + t13 * F["0.765366865"], n)
    o6 = half(z1 - t12 * F["1.847759065"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["1.175875602"]
    t4, t5, t6, t7 = t4 * F["0.298631336"], t5 * F["2.053119869"], t6 * F["3.072711026"], t7 * F["1.501321110"]
    z1, z2 = -z1 * F["0.899976223"], -z2 * F["2.562915447"]
    z3, z4 = z5 - z3 * F["1.961570560"], z5 - z4 * F["0.390180644"]
    o7, o5, o3, o1 = half(t4 + z1 + z3, n), half(t5 + z2 + z4, n), half(t6 + z2 + z3, n), half(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def fdct_int(s: np.ndarray) -> np.ndarray:
    """s[...,8,8] integer samples (row, column) -> 8 x the DCT, [...,8,8] (vertical, horizontal frequency), in integers:
    rows first, then columns"""
    t = _fdct_1d(s.astype(np.int64), True)
    return np.swapaxes(_fdct_1d(np.swapaxes(t, -1, -2), False), -1, -2)


def _quantised_blocks(plane, Q):
    """plane[8 r, 8 c] level-shifted samples -> [r, c, 64] int64 quantised coefficients in zigzag order"""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    co = fdct_int(plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3)).reshape(r, c, 64)
    return (np.sign(co) * ((np.abs(co) + 4 * Q) // (8 * Q)))[..., ZIGZAG]  # the DCT carries a factor of 8: ONE rounding


def _coefficients_420(q, quality) -> np.ndarray:
    """q[H,W,3] uint8 -> coef[nmy,nmx,6,64] int16: libjpeg's 4:2:0 (h2v2 downsampling, its edge expansion and its dummy
    blocks), see the module text"""
    H, W, _ = q.shape
    nmy, nmx = (H + 15) // 16, (W + 15) // 16
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    QL, QC = quant_tables(quality)
    ycc = rgb_to_ycc(q[:, np.minimum(np.arange(16 * nmx), W - 1)])  # columns replicated out to whole MCUs
    out = np.empty((nmy, nmx, 6, 64), dtype=np.int16)
    # luma: rows replicated; the blocks past nby / nbx are computed here and replaced below
    Y = _quantised_blocks(ycc[np.minimum(np.arange(16 * nmy), H - 1), :, 0] - 128, QL)
    out[:, :, :4] = Y.reshape(nmy, 2, nmx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(nmy, nmx, 4, 64)
    if nbx & 1:  # the dummy column: no AC, the quantised DC of the left neighbour
        out[:, -1, 1:4:2, 1:] = 0
        out[:, -1, 1:4:2, 0] = out[:, -1, 0:4:2, 0]
    if nby & 1:  # the dummy row: no AC, both blocks the quantised DC of Y01, the block before them in the MCU
        out[-1, :, 2:4, 1:] = 0
        out[-1, :, 2:4, 0] = out[-1, :, 1:2, 0]
    # chroma: the 2 x 2 mean with the alternating bias over the real rows, then the last DOWNSAMPLED row replicated
    hc = (H + 1) // 2
    r0, r1 = np.minimum(2 * np.arange(hc), H - 1), np.minimum(2 * np.arange(hc) + 1, H - 1)
    bias = 1 + (np.arange(8 * nmx) & 1)
    for c in (1, 2):
        p = ycc[..., c]
        down = (p[r0][:, 0::2] + p[r0][:, 1::2] + p[r1][:, 0::2] + p[r1][:, 1::2] + bias) >> 2
        out[:, :, 3 + c] = _quantised_blocks(down[np.minimum(np.arange(8 * nmy), hc - 1)] - 128, QC)
    return out


def jpeg_coefficients(q_uint8_hwc, quality: int = 90, subsampling="4:4:4") -> np.ndarray:
    """The quantised image q[H,W,3] uint8 -> coef[nby,nbx,3,64] int16, zigzag order (component order Y, Cb, Cr); at
    ``subsampling="4:2:0"`` coef[nmy,nmx,6,64] with nmy = ceil(H / 16), nmx = ceil(W / 16), block order Y00, Y01, Y10, Y11,
    Cb, Cr."""
    check_subsampling(subsampling)
    q = q_uint8_hwc.cpu().numpy() if isinstance(q_uint8_hwc, torch.Tensor) else np.asarray(q_uint8_hwc)
    if q.dtype != np.uint8 or q.ndim != 3 or q.shape[2] != 3 or q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"jpeg_coefficients: uint8 [H,W,3] expected, got {q.dtype} {q.shape}")
    if subsampling == "4:2:0":
        return _coefficients_420(q, quality)
    H, W, _ = q.shape
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    pad = q[np.minimum(np.arange(nby * 8), H - 1)][:, np.minimum(np.arange(nbx * 8), W - 1)]
    ycc = rgb_to_ycc(pad) - 128
    out = np.empty((nby, nbx, 3, 64), dtype=np.int16)
    for c, Q in enumerate((quant_tables(quality)[0], quant_tables(quality)[1], quant_tables(quality)[1])):
        out[:, :, c, :] = _quantised_blocks(ycc[..., c], Q)
    return out


# ---- entropy coding ----------------------------------------------------------------------------------------------------------
def huffman_codes(bits, vals):
    """(BITS, HUFFVAL) -> {symbol: (code, length)} (T.81 Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _code_arrays(tab, n):
    code, length = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    for sym, (c, ln) in huffman_codes(*HUFFMAN[tab]).items():
        code[sym], length[sym] = c, ln
    return code, length


_DC = [_code_arrays(0x00, 12), _code_arrays(0x01, 12)]
_AC = [_code_arrays(0x10, 256), _code_arrays(0x11, 256)]
_CAT = np.array([int(v).bit_length() for v in range(2048)], dtype=np.int64)


def _block_entries(zz, pred, tab):
    """zz[N,64] clamped coefficients, pred[N] DC predictions, tab[N] table id -> (value, length) [N,128]: entry 0 the DC
    symbol with its bits, 2k - 1 the ZRLs in front of AC k, 2k its run / size symbol with its bits, 127 EOB; length 0 = none."""
    N = zz.shape[0]
    val = np.zeros((N, 128), dtype=np.uint64)
    length = np.zeros((N, 128), dtype=np.int64)
    dc_code = np.stack([_DC[0][0], _DC[1][0]])
    dc_len = np.stack([_DC[0][1], _DC[1][1]])
    ac_code = np.stack([_AC[0][0], _AC[1][0]])
    ac_len = np.stack([_AC[0][1], _AC[1][1]])
    d = zz[:, 0] - pred
    c = _CAT[np.abs(d)]
    bits = np.where(d >= 0, d, d + (1 << c) - 1).astype(np.uint64)
    val[:, 0] = (dc_code[tab, c] << c.astype(np.uint64)) | bits
    length[:, 0] = dc_len[tab, c] + c
    ac = zz[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)  # position of the last non-zero at or before k
    prev = np.concatenate([np.zeros((N, 1), dtype=np.int64), last[:, :-1]], axis=1)
    run = pos - prev - 1  # zeros in front of AC k (meaningful where nz)
    c = _CAT[np.abs(ac)]
    bits = np.where(ac >= 0, ac, ac + (1 << c) - 1).astype(np.uint64)
    sym = ((run & 15) << 4) | c
    t2 = tab[:, None]
    val[:, 2:127:2] = np.where(nz, (ac_code[t2, sym] << c.astype(np.uint64)) | bits, 0)
    length[:, 2:127:2] = np.where(nz, ac_len[t2, sym] + c, 0)
    n_zrl = np.where(nz, run >> 4, 0)  # 0 .. 3
    zc, zl = ac_code[t2, 0xF0], ac_len[t2, 0xF0]
    zv = np.zeros_like(val[:, 1:126:2])
    for _ in range(3):
        more = n_zrl > 0
        zv = np.where(more, (zv << zl.astype(np.uint64)) | zc, zv)
        n_zrl = n_zrl - more
    val[:, 1:126:2] = zv
    length[:, 1:126:2] = np.where(nz, run >> 4, 0) * zl
    eob = ~nz[:, 62]
    val[:, 127] = np.where(eob, ac_code[tab, 0], 0)
    length[:, 127] = np.where(eob, ac_len[tab, 0], 0)
    return val, length


def encode_scan(coef, restart_mcus=None) -> bytes:
    """coef[nby,nbx,3,64] int16 (zigzag), or the 4:2:0 layout [nmy,nmx,6,64] (recognised by ``coef.shape[2]``) -> the
    entropy-coded data of the frame's one scan: everything between the SOS header
    and EOI, the RSTm markers included.  ``restart_mcus``: MCUs per restart interval, 0 for none, None for one MCU row.
    Structured as the device pass is: per block the (code, length) entries, a running sum of the lengths for the bit
    positions, the bits ORed together, then per segment the padding with ones and the byte stuffing."""
    coef = coef.cpu().numpy() if isinstance(coef, torch.Tensor) else np.asarray(coef)
    if coef.dtype != np.int16 or coef.ndim != 4 or coef.shape[2:] not in ((3, 64), (6, 64)) or coef.shape[0] < 1 or coef.shape[1] < 1:
        raise ValueError(f"encode_scan: int16 [nby,nbx,3,64] or [nmy,nmx,6,64] expected, got {coef.dtype} {coef.shape}")
    nby, nbx, bpm = coef.shape[:3]
    n_mcu = nby * nbx
    R = _resolve_restart(restart_mcus, nbx)
    seg_mcus = R if R > 0 else n_mcu
    zz = coef.reshape(n_mcu * bpm, 64).astype(np.int64)
    zz[:, 0] = np.clip(zz[:, 0], DC_MIN, DC_MAX)
    zz[:, 1:] = np.clip(zz[:, 1:], -AC_MAX, AC_MAX)
    blk = np.arange(n_mcu * bpm)
    pos = blk % bpm
    # the previous block of the component: 3 back at 4:4:4; at 4:2:0 Y00 follows the Y11 of the MCU before (3 back), Y01 ..
    # Y11 the block before, Cb and Cr the MCU before (6 back)
    back = np.array([3, 3, 3] if bpm == 3 else [3, 1, 1, 1, 6, 6])[pos]
    first = ((blk // bpm) % seg_mcus == 0) & (back >= 3)  # the first block of a component in a segment predicts from 0
    pred = np.where(first, 0, zz[np.maximum(blk - back, 0), 0])
    tab = (pos != 0).astype(np.int64) if bpm == 3 else (pos >= 4).astype(np.int64)
    out = bytearray()
    slab = max(1, 8192 // seg_mcus) * seg_mcus  # whole segments, a few thousand MCUs at a time
    for m0 in range(0, n_mcu, slab):
        m1 = min(n_mcu, m0 + slab)
        val, length = _block_entries(zz[bpm * m0:bpm * m1], pred[bpm * m0:bpm * m1], tab[bpm * m0:bpm * m1])
        block_bits = length.sum(axis=1)
        seg_first = np.arange(0, bpm * (m1 - m0), bpm * seg_mcus)
        seg_bits = np.add.reduceat(block_bits, seg_first)
        pad = (-seg_bits) % 8
        seg_bytes = (seg_bits + pad) // 8
        # one more entry behind each segment: the padding ones
        n_blk = bpm * (m1 - m0)
        seg_of = np.arange(n_blk) // (bpm * seg_mcus)
        is_last = np.concatenate([seg_of[1:] != seg_of[:-1], [True]])
        val = np.concatenate([val, np.where(is_last, (1 << pad[seg_of]) - 1, 0).astype(np.uint64)[:, None]], axis=1).reshape(-1)
        length = np.concatenate([length, np.where(is_last, pad[seg_of], 0)[:, None]], axis=1).reshape(-1)
        keep = length > 0
        val, length = val[keep], length[keep]
        start = np.cumsum(length) - length
        total = int(length.sum())
        owner = np.repeat(np.arange(length.size), length)
        j = np.arange(total) - start[owner]
        bitstream = ((val[owner] >> (length[owner] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        packed = np.packbits(bitstream)
        ends = np.cumsum(seg_bytes)
        for s, (a, b) in enumerate(zip(ends - seg_bytes, ends)):
            g = m0 // seg_mcus + s  # the segment's number in the frame
            if g > 0:
                out += bytes((0xFF, 0xD0 + ((g - 1) & 7)))
            out += packed[a:b].tobytes().replace(b"\xff", b"\xff\x00")
    return bytes(out)


def jpeg_frame(scan_bytes, H: int, W: int, quality: int = 90, restart_mcus=None, subsampling="4:4:4") -> bytes:
    """The JPEG file round one frame's scan data: SOI, JFIF APP0, two DQT, SOF0 (8 bit, three components, 1x1 sampling, or
    2x2 for Y at ``subsampling="4:2:0"``), the four DHT, DRI when ``restart_mcus`` (in MCUs of the sampling; None: one MCU
    row) is not 0, SOS, the data, EOI."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"jpeg_frame: H {H}, W {W} (1 .. 65535)")
    R = _resolve_restart(restart_mcus, mcu_grid(H, W, subsampling)[1])
    luma_sampling = 0x11 if subsampling == "4:4:4" else 0x22
    hd = bytearray(b"\xff\xd8\xff\xe0" + struct.pack(">H", 16) + b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for t, Q in enumerate(quant_tables(quality)):
        hd += b"\xff\xdb" + struct.pack(">HB", 67, t) + bytes(int(v) for v in Q[ZIGZAG])
    hd += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, luma_sampling, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc in (0x00, 0x10, 0x01, 0x11):
        bits, vals = HUFFMAN[tc]
        hd += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc) + bytes(bits) + bytes(vals)
    if R:
        hd += b"\xff\xdd" + struct.pack(">HH", 4, R)
    hd += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(hd) + bytes(scan_bytes) + b"\xff\xd9"


def encode_jpeg(img, quality: int = 90, restart_mcus=None, subsampling="4:4:4") -> bytes:
    """One image -> a JPEG file on the host.  ``img``: float [3,H,W] (quantised as ``*_combined.png`` is) or uint8 [H,W,3].
    ``subsampling``: "4:4:4", or "4:2:0" for chroma at half resolution in both directions (16 x 16 MCUs)."""
    check_subsampling(subsampling)
    if isinstance(img, torch.Tensor) and img.dtype != torch.uint8:
        if img.ndim != 3 or img.shape[0] != 3:
            raise ValueError(f"encode_jpeg: float [3,H,W] or uint8 [H,W,3] expected, got {tuple(img.shape)}")
        img = png.quantize_save_image(img.detach().cpu()).permute(1, 2, 0).contiguous()
    q = img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    H, W = int(q.shape[0]), int(q.shape[1])
    return jpeg_frame(encode_scan(jpeg_coefficients(q, quality, subsampling), restart_mcus), H, W, quality, restart_mcus, subsampling)


# ---- the container -----------------------------------------------------------------------------------------------------------
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
AVI_MAX_BYTES = 1 << 31


def write_avi(path, frames, W: int, H: int, fps: int = 10) -> int:
    """JPEG files (bytes, in play order) -> a Motion-JPEG AVI 1.0 at ``path``; returns the bytes written.

    RIFF 'AVI ' { LIST 'hdrl' { avih (56 bytes, AVIF_HASINDEX), LIST 'strl' { strh (56 bytes, vids / MJPG, scale 1, rate
    fps), strf (BITMAPINFOHEADER, 40 bytes, 24 bit, MJPG) } }, LIST 'movi' { 00dc chunks, padded to even length }, idx1 (16
    bytes per frame: 00dc, AVIIF_KEYFRAME, offset from the 'movi' fourcc, length) }.  Raises ``ValueError`` before anything
    is written if there is no frame or the file would reach 2^31 bytes (no OpenDML)."""
    path = pathlib.Path(path)
    frames = [bytes(f) for f in frames]
    fps = int(fps)
    if not frames or fps < 1 or not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"write_avi: {len(frames)} frames, fps {fps}, {W} x {H}")
    n = len(frames)
    movi_bytes = 4 + sum(8 + len(f) + (len(f) & 1) for f in frames)
    hdrl_bytes = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))
    total = 12 + (8 + hdrl_bytes) + (8 + movi_bytes) + (8 + 16 * n)
    if total >= AVI_MAX_BYTES:
        raise ValueError(f"write_avi: {total} bytes would reach 2^31 (AVI 1.0 without OpenDML); write fewer or smaller frames")
    biggest = max(len(f) for f in frames)
    avih = struct.pack("<14I", 1000000 // fps, biggest * fps, 0, AVIF_HASINDEX, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
        + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"LIST" + struct.pack("<I", hdrl_bytes) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
    assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40 and len(hdrl) == 8 + hdrl_bytes
    parts = [b"RIFF" + struct.pack("<I", total - 8) + b"AVI ", hdrl, b"LIST" + struct.pack("<I", movi_bytes) + b"movi"]
    idx = bytearray()
    off = 4
    for f in frames:
        parts.append(b"00dc" + struct.pack("<I", len(f)))
        parts.append(f)
        if len(f) & 1:
            parts.append(b"\0")
        idx += b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, len(f))
        off += 8 + len(f) + (len(f) & 1)
    parts.append(b"idx1" + struct.pack("<I", len(idx)) + bytes(idx))
    written = png.atomic_write(path, parts)
    assert written == total
    return written


# ---- per-rank part files -------------------------------------------------------------------------------------------------------
# <dir>/.<scene_id>_combined.part<rank>: b"PGDVSMJ1", then <IIII> W, H, fps, n, then per frame <iI> tgt_idx, length and the JPEG
PART_MAGIC = b"PGDVSMJ1"


def part_path(scene_dir, scene_id: str, rank: int) -> pathlib.Path:
    return pathlib.Path(scene_dir) / f".{scene_id}_combined.part{int(rank)}"


def video_path(scene_dir, scene_id: str) -> pathlib.Path:
    return pathlib.Path(scene_dir) / f"{scene_id}_combined.avi"


def _write_part(path, frames, W, H, fps) -> int:
    parts = [PART_MAGIC + struct.pack("<IIII", W, H, fps, len(frames))]
    for idx, data in frames:
        parts += [struct.pack("<iI", idx, len(data)), data]
    return png.atomic_write(path, parts)


def _read_part(path):
    raw = pathlib.Path(path).read_bytes()
    if raw[:8] != PART_MAGIC or len(raw) < 24:
        raise ValueError(f"{path}: not a video part file")
    W, H, fps, n = struct.unpack_from("<IIII", raw, 8)
    frames, off = [], 24
    for _ in range(n):
        idx, ln = struct.unpack_from("<iI", raw, off)
        frames.append((idx, raw[off + 8:off + 8 + ln]))
        off += 8 + ln
    if off != len(raw):
        raise ValueError(f"{path}: truncated video part file")
    return W, H, fps, frames


def _sorted_frames(frames):
    """(tgt_idx, data) pairs -> sorted by tgt_idx, one frame per index (the last submitted): upstream builds the video from
    the sorted ``*_combined.png`` of the scene, and a view rendered twice (the sampler's wrap-round) overwrites its file"""
    return sorted(dict(frames).items())


def assemble(vis_dir, world: int) -> list:
    """Merges the part files that the ranks of a ``world``-process run left under ``vis_dir`` (any depth) into one
    ``<scene_id>_combined.avi`` per scene, frames sorted by ``tgt_idx`` (one per index), and deletes the parts.  A rank writes a part for
    every scene it rendered a view of, so a scene may lack the part of a rank that had none of its views; a rank of
    0 .. world - 1 that left no part at all is missing: ``FileNotFoundError``, nothing written or deleted.  Returns the AVI
    paths."""
    vis_dir = pathlib.Path(vis_dir)
    scenes, ranks_seen = {}, set()
    for p in sorted(vis_dir.rglob(".*_combined.part*")):
        stem, _, rank = p.name[1:].rpartition("_combined.part")
        if not rank.isdigit() or int(rank) >= world:
            continue
        scenes.setdefault((p.parent, stem), {})[int(rank)] = p
        ranks_seen.add(int(rank))
    missing = sorted(set(range(world)) - ranks_seen)
    if missing:
        raise FileNotFoundError(f"assemble: no video part of rank(s) {missing} under {vis_dir} (world {world})")
    out = []
    for (scene_dir, scene_id), parts in sorted(scenes.items()):
        frames, geom = [], None
        for rank in sorted(parts):
            W, H, fps, fr = _read_part(parts[rank])
            if geom is not None and geom != (W, H, fps):
                raise ValueError(f"assemble: {parts[rank]} holds {W} x {H} at {fps} fps, another part {geom}")
            geom = (W, H, fps)
            frames += fr
        frames = _sorted_frames(frames)
        path = video_path(scene_dir, scene_id)
        write_avi(path, [f[1] for f in frames], geom[0], geom[1], geom[2])
        for p in parts.values():
            p.unlink()
        out.append(path)
    return out


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class DeviceScan:
    """One frame's scan data on the GPU, as ``ops.jpeg_encode`` leaves it: ``data`` uint8 [capacity] and ``nbytes`` int32 [1]
    device tensors (views of a batch's), the frame's H and W, ``ready``, an event recorded behind the kernels, and the
    ``subsampling`` the scan was made with, which the frame's header has to name."""

    def __init__(self, data, nbytes, H, W, ready=None, subsampling="4:4:4"):
        self.data, self.nbytes, self.H, self.W, self.ready = data, nbytes, int(H), int(W), ready
        self.subsampling = check_subsampling(subsampling)


class MjpegWriter(png.AsyncWriter):
    """Collects frames per scene and writes one Motion-JPEG AVI per scene at ``close()``; shaped like ``png.PngWriter``.

    ``submit(scene_key, tgt_idx, frame)`` returns at once.  ``scene_key`` is ``(directory, scene_id)``; ``frame`` is a float
    image [3,H,W] (a host tensor is encoded by a worker with the host path; a GPU tensor goes through ``ops.jpeg_encode``
    on the current stream) or a ``DeviceScan``.  For GPU frames a worker thread waits for the frame's event, reads the
    length, copies exactly that many bytes through pinned memory on the writer's copy stream and wraps them with
    ``jpeg_frame``; the submitting thread never synchronises.  ``close()`` drains the workers, writes every scene's file
    -- ``<directory>/<scene_id>_combined.avi`` with the frames sorted by ``tgt_idx``, or for ``world > 1`` this rank's
    hidden part file for ``assemble`` -- and re-raises the first worker error.  The frames of a scene must share H and W
    (``ValueError`` at ``submit``).  ``restart_mcus``: None = one MCU row; the GPU path needs >= 1.  A GPU frame's buffer
    has its worst-case capacity (``ops.jpeg_scan_capacity``: 40 MB at 1080p) and lives until a worker has fetched its bytes.
    ``subsampling``: "4:4:4", or "4:2:0" (upstream's chroma format) for every frame of the writer; a ``DeviceScan`` made
    with another one is refused at ``submit``."""

    def __init__(self, fps: int = 10, quality: int = 90, restart_mcus=None, n_threads: int = 4, rank: int = 0, world: int = 1,
                 subsampling="4:4:4"):
        super().__init__(n_threads, "mjpeg")
        if int(fps) < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"MjpegWriter: fps {fps}, rank {rank}, world {world}")
        quant_tables(quality)
        if restart_mcus is not None:
            _resolve_restart(restart_mcus, 1)
        self.fps, self.quality, self.restart_mcus = int(fps), int(quality), restart_mcus
        self.subsampling = check_subsampling(subsampling)
        self.rank, self.world = int(rank), int(world)
        self._scenes = {}  # scene_key -> {"hw": (H, W), "frames": [(tgt_idx, bytes)]}
        self.files = []
        self.bytes_written = 0

    def _keep(self, key, tgt_idx, data):
        with self._lock:
            self._scenes[key]["frames"].append((int(tgt_idx), data))

    def _work_host(self, key, tgt_idx, img):
        self._keep(key, tgt_idx, encode_jpeg(img, self.quality, self.restart_mcus, self.subsampling))

    def _work_device(self, key, tgt_idx, scan, cs):
        if scan.ready is not None:
            scan.ready.synchronize()
        with torch.cuda.stream(cs):
            n_host = getattr(self._tls, "n", None)
            if n_host is None:
                n_host = self._tls.n = torch.empty(1, dtype=torch.int32).pin_memory()
            n_host.copy_(scan.nbytes.reshape(1), non_blocking=True)
        cs.synchronize()
        host = self._fetch(n_host[0], scan.data, cs, lambda n, capacity: (
            f"MjpegWriter: a frame's scan length {n} exceeds its capacity {capacity}"))
        self._keep(key, tgt_idx, jpeg_frame(host.numpy().tobytes(), scan.H, scan.W, self.quality, self.restart_mcus, scan.subsampling))

    def submit(self, scene_key, tgt_idx, frame) -> None:
        self._check_open("MjpegWriter.submit")
        key = (pathlib.Path(scene_key[0]), str(scene_key[1]))
        if isinstance(frame, torch.Tensor) and frame.is_cuda:
            from . import ops

            if frame.ndim != 3:
                raise ValueError(f"MjpegWriter.submit: [3,H,W] expected, got {tuple(frame.shape)}")
            data, nbytes = ops.jpeg_encode(frame, quality=self.quality, restart_mcus=self.restart_mcus, subsampling=self.subsampling)
            frame = DeviceScan(data[0], nbytes[0:1], frame.shape[1], frame.shape[2], torch.cuda.current_stream(frame.device).record_event(),
                               self.subsampling)
        if isinstance(frame, DeviceScan):
            if frame.subsampling != self.subsampling:
                raise ValueError(f"MjpegWriter.submit: a {frame.subsampling} scan for a {self.subsampling} writer")
            H, W = frame.H, frame.W
        elif isinstance(frame, torch.Tensor) and frame.ndim == 3 and frame.shape[0] == 3:
            H, W = int(frame.shape[1]), int(frame.shape[2])
        else:
            raise ValueError("MjpegWriter.submit: a float image [3,H,W] or a DeviceScan expected")
        with self._lock:
            scene = self._scenes.setdefault(key, {"hw": (H, W), "frames": []})
        if scene["hw"] != (H, W):
            raise ValueError(f"MjpegWriter.submit: scene {key[1]} has {scene['hw']} frames, got {(H, W)}")
        if isinstance(frame, DeviceScan):
            dev = frame.data.device
            if frame.ready is None:
                frame.ready = torch.cuda.current_stream(dev).record_event()
            self._run(self._work_device, key, tgt_idx, frame, self.copy_stream(dev))
        else:
            self._run(self._work_host, key, tgt_idx, frame.detach())

    def _drained(self) -> None:
        """every frame is in: write each scene's file (or this rank's part), unless a worker failed"""
        scenes, self._scenes = self._scenes, {}
        if self._error is not None:
            return
        for (scene_dir, scene_id), scene in sorted(scenes.items()):
            frames = _sorted_frames(scene["frames"])
            H, W = scene["hw"]
            if self.world > 1:
                path = part_path(scene_dir, scene_id, self.rank)
                self.bytes_written += _write_part(path, frames, W, H, self.fps)
            else:
                path = video_path(scene_dir, scene_id)
                self.bytes_written += write_avi(path, [f[1] for f in frames], W, H, self.fps)
            self.files.append(path)
