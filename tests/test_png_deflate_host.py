"""The stream of the device deflate, restated on the host (png.deflate_rle; csrc/png_deflate.hip follows it byte for byte,
tests/test_gpu_png_deflate.py): zlib decodes it back to the input on crafted buffers, the literal/length code is limited to 15
bits and complete, the container round it opens in PIL with png.encode's pixels, its size stays within 3 % of zlib's own
run-length strategy, and the writer's option changes nothing for host arrays."""
import io
import pathlib
import re
import sys
import zlib

import numpy as np
import PIL.Image
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import png_deflate_cases as PC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("seg", PC.SEGS)
@pytest.mark.parametrize("name", sorted(PC.buffers()))
def test_zlib_decodes_the_restated_stream(name, seg):
    from pgdvs_amd import png

    raw = PC.buffers()[name]
    z = png.deflate_rle(raw, seg)
    assert z[:2] == b"\x78\x01"
    assert zlib.decompress(z) == raw.tobytes()  # (zlib checks the Adler-32 itself)
    assert len(z) <= png.deflate_capacity(raw.size, seg)


def test_tokens_follow_the_run_rule():
    from pgdvs_amd import png

    pos, sym, ebits, evalue = png.rle_tokens(PC.buffers()["seven"], 4096)
    assert pos.tolist() == [0, 1, 2, 6] and sym.tolist() == [1, 2, 258, 9] and ebits.tolist() == [0] * 4  # 2, then a match of 4
    pos, sym, ebits, evalue = png.rle_tokens(PC.buffers()["runs"], 4096)
    want, at = [], 0
    for i, n in enumerate(PC.RUN_LENGTHS):
        m = n - 1
        r = m % 258
        want += [10 + i] + [285] * (m // 258) + ([png._length_symbol(r)[0]] if r >= 3 else [10 + i] * r) + [200 + i]
        at += n + 1
    assert sym.tolist() == want
    # a run never continues across a segment start, and a segment's first byte is a literal
    raw = PC.buffers()["straddle4096"]
    pos, sym, _, _ = png.rle_tokens(raw, 4096)
    i = int(np.searchsorted(pos, 4096))
    assert pos[i] == 4096 and sym[i] == 5 and sym[i - 1] == png._length_symbol(99)[0] and sym[i + 1] == png._length_symbol(99)[0]


@pytest.mark.parametrize("seg", PC.SEGS)
@pytest.mark.parametrize("name", sorted(PC.buffers()))
def test_code_is_limited_to_15_bits_and_complete(name, seg):
    from pgdvs_amd import png

    raw = PC.buffers()[name]
    _, sym, _, _ = png.rle_tokens(raw, seg)
    hist = np.bincount(sym, minlength=286)
    hist[256] = -(-raw.size // seg)
    lengths = png.litlen_code_lengths(hist)
    assert max(lengths) <= 15
    assert sum(1 << (15 - n) for n in lengths if n) == 1 << 15  # Kraft sum exactly 1
    assert all((n > 0) == (h > 0) for n, h in zip(lengths, hist))
    if name == "deep":
        assert max(lengths) == 15
    codes = png.canonical_codes(lengths)
    assert len({(n, c) for n, c in zip(lengths, codes) if n}) == sum(1 for n in lengths if n)


@pytest.mark.parametrize("H,W", [(37, 53), (3, 2049)])
@pytest.mark.parametrize("kind", ["noise", "render", "zeros"])
def test_container_opens_with_the_pixels_of_encode(kind, H, W):
    from pgdvs_amd import png

    s = PC.scanlines(kind, H, W)
    ours = png.png_from_zstream(png.deflate_rle(s, 4096), H, W)
    with PIL.Image.open(io.BytesIO(ours)) as a, PIL.Image.open(io.BytesIO(png.encode(s, H, W))) as b:
        a.load()
        b.load()
        assert a.mode == b.mode == "RGB" and a.size == b.size == (W, H)
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("seg", PC.SEGS)
@pytest.mark.parametrize("name", ["render", "smooth", "noise", "deep"])
def test_size_within_3_percent_of_zlib_rle(name, seg):
    """bound from the issue: len(ours) <= 1.03 R + n_seg c + 16 with R zlib's Z_RLE stream and c = png.DEFLATE_SEG_OVERHEAD"""
    from pgdvs_amd import png

    raw = PC.buffers()["deep"] if name == "deep" else PC.scanlines(name, 135, 240).reshape(-1)
    ours, R = len(png.deflate_rle(raw, seg)), PC.zlib_rle_size(raw)
    n_seg = -(-raw.size // seg)
    print(f"{name} seg {seg}: {raw.size} bytes -> {ours} (zlib Z_RLE {R}, level 1 {len(zlib.compress(raw.tobytes(), 1))}), "
          f"{(ours - n_seg * png.DEFLATE_SEG_OVERHEAD) / R:.4f} R without the segments' overhead")
    assert ours <= 1.03 * R + n_seg * png.DEFLATE_SEG_OVERHEAD + 16


def test_kernel_constants_are_the_ones_python_states():
    from pgdvs_amd import ops, png

    text = (ROOT / "ml-pgdvs_amd" / "csrc" / "png_deflate.hip").read_text()
    const = {k: v for k, v in re.findall(r"constexpr int (k\w+) = ([^;]+);", text)}
    assert int(const["kPer"]) == ops.PNG_DEFLATE_PER and int(const["kHalo"]) == ops.PNG_DEFLATE_HALO
    assert const["kWindow"] == "kBlock * kPer" and int(const["kBlock"]) * ops.PNG_DEFLATE_PER == ops.PNG_DEFLATE_WINDOW
    assert const["kPayload"] == "kWindow - kHalo" and ops.PNG_DEFLATE_PAYLOAD == ops.PNG_DEFLATE_WINDOW - ops.PNG_DEFLATE_HALO
    assert ops.PNG_DEFLATE_HALO >= png.DEFLATE_MAX_MATCH == int(const["kMaxMatch"])
    assert (int(const["kSegMin"]), int(const["kSegMax"])) == (png.DEFLATE_SEG_MIN, png.DEFLATE_SEG_MAX)
    assert png.DEFLATE_HEADER_BITS == 1222 and png.DEFLATE_SEG_OVERHEAD == 160
    assert ops.png_deflate_capacity(97335, 32768) == 8 + 3 * 160 + (15 * 97335 + 7) // 8
    for bad in (0, 4095, 5000, 131072):
        with pytest.raises(ValueError):
            png.check_seg_bytes(bad)


def test_writer_option_leaves_host_arrays_to_zlib(tmp_path):
    from pgdvs_amd import png

    H, W = 37, 53
    s = np.array(PC.scanlines("render", H, W))
    files = {}
    for mode in ("zlib", "device"):
        with png.PngWriter(n_threads=2, deflate=mode) as w:
            w.submit(tmp_path / f"{mode}.png", s)
            w.submit_batch([tmp_path / f"{mode}_b{i}.png" for i in range(2)], np.stack([s, s]))
        assert w.files_written == 3
        files[mode] = [(tmp_path / f).read_bytes() for f in (f"{mode}.png", f"{mode}_b0.png", f"{mode}_b1.png")]
    assert files["device"] == files["zlib"] == [png.encode(s, H, W)] * 3
    with pytest.raises(ValueError):
        png.PngWriter(deflate="nonsense")
    with pytest.raises(ValueError):
        png.PngWriter(deflate="device", seg_bytes=1000)
