"""The visualiser's video on the host (pgdvs_amd/video.py, harness.vis_step / vis_run with ``video``): the tables are the
standard's as PIL writes them, the integer DCT and colour transform stay within their stated distance of the exact ones,
every stream decodes with PIL (libjpeg, independent of the writer) to the float64 decode model of its coefficients and loses
no quality against PIL's own encoder, the AVI container is consistent field by field, and the loop writes one file per
scene, on one rank or assembled from two.  No AVI reader exists on the build machine: the container is checked structurally,
frame by frame, and has not been opened in a player."""
import io
import pathlib
import re
import struct
import sys

import numpy as np
import pytest
import torch
from scipy.fft import dctn

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import video_reference as R  # noqa: E402
import vis_reference as VR  # noqa: E402

from pgdvs_amd import harness, png, video  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------- tables
def test_huffman_tables_are_the_ones_pil_writes():
    dht = R.parse_dht(R.pil_jpeg(np.zeros((8, 8, 3), np.uint8), 50, optimize=False))
    assert sorted(dht) == [0x00, 0x01, 0x10, 0x11]
    for tc, (bits, vals) in dht.items():
        assert (list(video.HUFFMAN[tc][0]), list(video.HUFFMAN[tc][1])) == (bits, vals), hex(tc)
    # and the frame header carries exactly these four
    ours = R.parse_dht(video.encode_jpeg(np.zeros((8, 8, 3), np.uint8)))
    assert ours == dht


@pytest.mark.parametrize("q", [1, 25, 50, 75, 90, 95, 100])
def test_quant_tables_are_libjpegs(q):
    import PIL.Image

    data = R.pil_jpeg(np.zeros((8, 8, 3), np.uint8), q)
    pil = PIL.Image.open(io.BytesIO(data)).quantization
    luma, chroma = video.quant_tables(q)
    assert luma.shape == (64,) and chroma.shape == (64,)
    # Image.quantization is in natural (row-major) order for this PIL: the table of the file, read raw, is its zigzag
    raw = R.parse_dqt(data)
    assert [raw[0][i] for i in np.argsort(R.NATURAL)] == list(pil[0])
    assert luma.tolist() == list(pil[0]) and chroma.tolist() == list(pil[1])
    ours = R.parse_dqt(video.encode_jpeg(np.zeros((8, 8, 3), np.uint8), quality=q))
    assert ours == raw
    for bad in (0, 101):
        with pytest.raises(ValueError):
            video.quant_tables(bad)


def test_zigzag_and_dct_constants():
    assert video.ZIGZAG.tolist() == R.NATURAL.tolist()
    # the twelve constants are rint(8192 x) of the values they are named after, and csrc/jpeg.hip holds the same ones (its
    # GPU test compares results; this compares the source)
    assert len(video.DCT_FIX) == 12 and (video.DCT_BITS, video.DCT_PASS1_BITS) == (13, 2)
    for name, v in video.DCT_FIX.items():
        assert v == int(np.rint(float(name) * 8192)), name
    text = (ROOT / "ml-pgdvs_amd" / "csrc" / "jpeg.hip").read_text()
    found = {f"{a}.{b}": int(v) for a, b, v in re.findall(r"kFix_(\d)_(\d{9}) = (\d+)", text)}
    assert found == video.DCT_FIX
    assert re.search(r"kDctBits = 13, kPass1Bits = 2;", text)
    # the values: sqrt(2) cos(k pi / 16) combinations of the Loeffler-Ligtenberg-Moschytz flow graph
    c = lambda k: np.sqrt(2.0) * np.cos(k * np.pi / 16.0)  # noqa: E731
    want = {"0.541196100": c(6), "1.175875602": c(3), "0.765366865": c(2) - c(6), "1.847759065": c(2) + c(6),
            "0.298631336": -c(1) + c(3) + c(5) - c(7), "2.053119869": c(1) + c(3) - c(5) + c(7),
            "3.072711026": c(1) + c(3) + c(5) - c(7), "1.501321110": c(1) + c(3) - c(5) - c(7),
            "0.899976223": c(7) - c(3), "2.562915447": -c(1) - c(3), "1.961570560": -c(3) - c(5), "0.390180644": c(5) - c(3)}
    assert sorted(want) == sorted(video.DCT_FIX)
    for name, v in want.items():
        assert abs(abs(v) - float(name)) < 1e-8, name
    body = re.search(r"kZigzagPos\[64\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", body)] == np.argsort(R.NATURAL).tolist()


def test_integer_dct_against_the_exact_one():
    """``fdct_int`` gives 8 x the coefficient.  Measured over these blocks: max |integer / 8 - exact| 0.180; quantised with
    Q = 1 the largest |AC| is 1020 and DC runs from -1024 to 1016."""
    rng = np.random.default_rng(0)
    blocks = [rng.integers(-128, 128, (20000, 8, 8))]
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(k == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * n + 1) * k * np.pi / 16.0)
    for a in range(8):  # the 128 sign patterns that drive one coefficient to its extremes
        for b in range(8):
            pattern = np.where(np.outer(c[a], c[b]) >= 0, 127, -128)
            blocks.append(np.stack([pattern, -pattern - 1]))
    s = np.concatenate(blocks)
    got = video.fdct_int(s)
    err = np.abs(got / 8.0 - dctn(s.astype(np.float64), axes=(-2, -1), norm="ortho")).max()
    q1 = np.sign(got) * ((np.abs(got) + 4) // 8)  # the quantiser at Q = 1
    ac = q1.reshape(-1, 64)[:, 1:]
    print(f"max |int dct / 8 - exact| {err:.3f}, max |AC| {np.abs(ac).max()}, DC {q1[:, 0, 0].min()} .. {q1[:, 0, 0].max()}")
    assert err <= 1.0
    assert np.abs(ac).max() <= 1023 and -1024 <= q1[:, 0, 0].min() and q1[:, 0, 0].max() <= 1023
    assert np.abs(got).max() * 25172 * 4 < 2 ** 31  # the largest constant times a sum of four outputs: the sums fit int32


def test_colour_lines():
    ramps = []
    for ch in range(3):
        for other in (0, 255):
            r = np.full((256, 3), other, np.uint8)
            r[:, ch] = np.arange(256)
            ramps.append(r)
    rgb = np.concatenate(ramps + [np.random.default_rng(1).integers(0, 256, (5000, 3)).astype(np.uint8)])
    assert rgb.shape[0] == 6 * 256 + 5000
    got = video.rgb_to_ycc(rgb)
    for i, (r, g, b) in enumerate(rgb.tolist()):
        want = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
                (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16)
        assert tuple(got[i].tolist()) == want, (r, g, b)
    assert got.min() >= 0 and got.max() <= 255
    exact = np.stack([0.299 * rgb[:, 0] + 0.587 * rgb[:, 1] + 0.114 * rgb[:, 2],
                      -0.168735892 * rgb[:, 0] - 0.331264108 * rgb[:, 1] + 0.5 * rgb[:, 2] + 128,
                      0.5 * rgb[:, 0] - 0.418687589 * rgb[:, 1] - 0.081312411 * rgb[:, 2] + 128], axis=1)
    assert np.abs(got - exact).max() <= 0.51  # round to nearest up to the 16-bit constants


# ---------------------------------------------------------------------------- whole frames
@pytest.mark.parametrize("H,W", R.SIZES)
@pytest.mark.parametrize("name", ["render", "noise", "constant", "checker"])
def test_encode_jpeg_decodes_with_pil(H, W, name):
    """(a) PIL's pixels within 3 levels of the float64 decode model: libjpeg's inverse DCT is within 1 per sample and its
    colour step within 1, times the largest inverse-colour weight 1.772, plus the model's own roundings.  (b) PSNR against
    the source no more than 0.1 dB below PIL's own encoder at the same quality and 4:4:4 (the two DCTs differ by under one
    coefficient LSB).

    Measured over the 60 (content, size, quality) cases: (a) at most 3 levels (render and noise 37 x 53 at quality 100; 2 elsewhere);
    (b) 0.000 dB in every case: colour, DCT and quantiser are libjpeg's, so the coefficients are PIL's own, and (c) without
    restart markers the scan data is byte for byte PIL's (``optimize=False``: the standard Huffman tables), which is
    asserted as well.  A first version of the codec (a matrix DCT rounded to whole coefficients before the division by Q)
    was beyond the margin in three cases: checker 37 x 53 at quality 90 by double rounding (-0.247 dB), noise 37 x 53 and
    24 x 40 at quality 100 (-0.306, -0.102 dB)."""
    im = R.contents(H, W)[name]
    nbx = (W + 7) // 8
    beyond = []
    for q in (50, 90, 100):
        coef = video.jpeg_coefficients(im, q)
        assert coef.shape == ((H + 7) // 8, nbx, 3, 64) and coef.dtype == np.int16
        model = R.decode_model(coef, *video.quant_tables(q), H, W)
        theirs = R.pil_jpeg(im, q, optimize=False)
        own = R.psnr(R.decode_pil(theirs)[2], im)
        plain = video.encode_jpeg(im, q, 0)
        assert plain[R.segments(plain)[1]:] == theirs[R.segments(theirs)[1]:], (q, "the scan differs from PIL's")
        pixels = None
        for restart in (0, 1, 3, nbx, None):
            data = video.encode_jpeg(im, q, restart)
            assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
            seg = dict(R.segments(data)[0])
            assert (0xDD in seg) == (restart != 0)
            if restart != 0:
                assert struct.unpack(">H", seg[0xDD])[0] == (nbx if restart is None else restart)
            assert struct.unpack(">BHHB", seg[0xC0][:6]) == (8, H, W, 3) and seg[0xC0][6:] == bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
            mode, size, pix = R.decode_pil(data)
            assert mode == "RGB" and size == (W, H)
            if pixels is None:
                pixels = pix
                d = np.abs(pix.astype(np.float64) - model).max()
                ours = R.psnr(pix, im)
                print(f"{name} {H}x{W} q{q}: |pil - model| max {d:.0f}, psnr {ours:.3f} against {own:.3f} ({ours - own:+.3f} dB), {len(data)} bytes")
                assert d <= 3, (q, d)
                if ours - own < -0.1:
                    beyond.append((q, round(ours, 3), round(own, 3)))
            else:  # restart markers change the bytes, never the picture
                assert np.array_equal(pix, pixels), (q, restart)
        assert video.encode_jpeg(im, q, None) == video.encode_jpeg(im, q, nbx)
    # the float [3,H,W] form quantises as *_combined.png does
    x = torch.from_numpy(im).permute(2, 0, 1).float().div(255.0)
    assert video.encode_jpeg(x, 90) == video.encode_jpeg(png.quantize_save_image(x).permute(1, 2, 0).numpy(), 90)
    assert not beyond, f"PSNR more than 0.1 dB below PIL's encoder at (quality, ours, PIL's): {beyond}"


def _frame_of(coef, restart, q=100):
    nby, nbx = coef.shape[:2]
    return video.jpeg_frame(video.encode_scan(coef, restart), 8 * nby, 8 * nbx, q, restart)


@pytest.mark.parametrize("name", sorted(R.crafted_blocks()))
def test_crafted_blocks_decode_to_the_model(name):
    """quality 100 (every divisor 1) keeps the dequantised samples inside the range libjpeg's range limiter covers"""
    q1 = video.quant_tables(100)
    assert q1[0].tolist() == [1] * 64
    coef = R.crafted_frame(name)
    for restart in (0, 1, None):
        mode, size, pix = R.decode_pil(_frame_of(coef, restart))
        assert size == (16, 8)
        assert np.abs(pix - R.decode_model(coef, *q1, 8, 16)).max() <= 3, (name, restart)


def test_crafted_dc_steps_markers_and_clamps():
    q1 = video.quant_tables(100)
    coef = R.dc_step_frame(6)
    assert set(np.abs(np.diff(coef[0, :, 0, 0].astype(int))).tolist()) == {2040}
    for restart in (0, 1, 4):
        pix = R.decode_pil(_frame_of(coef, restart))[2]
        assert np.abs(pix - R.decode_model(coef, *q1, 8, 48)).max() <= 3, restart
    # 15 MCUs, a restart after each: the marker number wraps past 7
    blocks = list(R.crafted_blocks().values())
    coef = np.zeros((3, 5, 3, 64), np.int16)
    for m in range(15):
        coef[m // 5, m % 5, 0] = blocks[m % len(blocks)]
        coef[m // 5, m % 5, 1 + m % 2] = blocks[(m + 3) % len(blocks)]
    scan = video.encode_scan(coef, 1)
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(14)]
    pix = R.decode_pil(_frame_of(coef, 1))[2]
    assert np.abs(pix - R.decode_model(coef, *q1, 24, 40)).max() <= 3
    # values beyond the tables are clamped on read: DC to -1024 .. 1023, AC to +-1023
    wild = np.zeros((1, 2, 3, 64), np.int16)
    wild[0, 0, 0, :3] = (32767, -32768, 5000)
    wild[0, 1, 0, :3] = (-32768, 32767, -5000)
    tame = np.zeros_like(wild)
    tame[0, 0, 0, :3] = (1023, -1023, 1023)
    tame[0, 1, 0, :3] = (-1024, 1023, -1023)
    assert video.encode_scan(wild, 0) == video.encode_scan(tame, 0)
    R.decode_pil(_frame_of(wild, 0))
    with pytest.raises(ValueError):
        video.encode_scan(coef.astype(np.int32), 1)
    with pytest.raises(ValueError):
        video.encode_scan(coef, 65536)


def test_noise_at_quality_100_is_byte_stuffed():
    im = R.contents(37, 53)["noise"]
    scan = video.encode_scan(video.jpeg_coefficients(im, 100), 0)
    assert scan.count(b"\xff\x00") > 0
    assert all(scan[i + 1] == 0 for i in range(len(scan) - 1) if scan[i] == 0xFF)  # no marker without restarts
    with_rst = video.encode_scan(video.jpeg_coefficients(im, 100), 1)
    after_ff = [with_rst[i + 1] for i in range(len(with_rst) - 1) if with_rst[i] == 0xFF]
    assert all(v == 0 or 0xD0 <= v <= 0xD7 for v in after_ff) and with_rst[-1] != 0xFF
    assert sum(v != 0 for v in after_ff) == 5 * 7 - 1


# ---------------------------------------------------------------------------- container
@pytest.mark.parametrize("lengths", [(101,), (100, 33, 7, 250)])
def test_write_avi_structure(tmp_path, lengths):
    rng = np.random.default_rng(len(lengths))
    frames = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lengths]
    path = tmp_path / "v.avi"
    n_bytes = video.write_avi(path, frames, 53, 37, fps=10)
    raw = path.read_bytes()
    assert n_bytes == len(raw) and sorted(p.name for p in tmp_path.iterdir()) == ["v.avi"]
    top, payloads = R.avi_frames(raw)
    assert payloads == frames
    assert [c.tag for c in top.children] == [b"LIST", b"LIST", b"idx1"]
    hdrl, movi, idx1 = top.children
    assert hdrl.form == b"hdrl" and [(c.tag, c.form) for c in hdrl.children] == [(b"avih", None), (b"LIST", b"strl")]
    avih = hdrl.children[0].data
    assert len(avih) == 56
    us, rate, pad, flags, total, initial, streams, bufsize, w, h = struct.unpack_from("<10I", avih)
    assert (us, flags, total, initial, streams, w, h) == (100000, 0x10, len(frames), 0, 1, 53, 37)
    assert bufsize >= max(lengths) and avih[40:] == bytes(16)
    strl = hdrl.children[1]
    assert [c.tag for c in strl.children] == [b"strh", b"strf"]
    strh, strf = strl.children[0].data, strl.children[1].data
    assert len(strh) == 56 and strh[:8] == b"vidsMJPG"
    scale, fps, start, length = struct.unpack_from("<4I", strh, 20)
    assert (scale, fps, start, length) == (1, 10, 0, len(frames))
    assert struct.unpack_from("<4h", strh, 48) == (0, 0, 53, 37)
    assert len(strf) == 40
    size, bw, bh, planes, bits, comp, image = struct.unpack_from("<IiiHH4sI", strf)
    assert (size, bw, bh, planes, bits, comp, image) == (40, 53, 37, 1, 24, b"MJPG", 53 * 37 * 3)
    # the index: 16 bytes per frame, offsets from the 'movi' fourcc to the chunk header
    assert idx1.size == 16 * len(frames)
    movi_fourcc = movi.offset + 8
    for i, f in enumerate(frames):
        tag, flags, off, ln = struct.unpack_from("<4sIII", idx1.data, 16 * i)
        assert (tag, flags, ln) == (b"00dc", 0x10, len(f))
        at = movi_fourcc + off
        assert raw[at:at + 4] == b"00dc" and struct.unpack_from("<I", raw, at + 4)[0] == len(f) and raw[at + 8:at + 8 + ln] == f
        assert at % 2 == 0


def test_write_avi_refuses_what_it_cannot_hold(tmp_path):
    with pytest.raises(ValueError):
        video.write_avi(tmp_path / "empty.avi", [], 8, 8)
    big = bytes(1 << 26)
    frames = [big] * 32  # 2^31 bytes of payload in 64 MiB of memory: one object, listed 32 times
    with pytest.raises(ValueError, match="2\\^31"):
        video.write_avi(tmp_path / "big.avi", frames, 8, 8)
    assert list(tmp_path.iterdir()) == []
    assert video.AVI_MAX_BYTES == 2 ** 31


# ---------------------------------------------------------------------------- the loop
def _all_files(root):
    return sorted(p.relative_to(root).as_posix() for p in pathlib.Path(root).rglob("*") if p.is_file())


def _expected_video(ds, indices, scene):
    """the frames of one scene in tgt_idx order, encoded on the host from what *_combined.png holds"""
    items = sorted((ds[i] for i in set(indices) if ds[i]["misc"]["scene_id"] == scene), key=lambda it: it["misc"]["tgt_idx"])
    return [video.encode_jpeg(VR.expected_save_image(it["img"]).permute(1, 2, 0).numpy(), 90) for it in items]


@pytest.mark.parametrize("split", [None, "val"])
def test_vis_run_video(tmp_path, split):
    ds = VR.StubDataset(7, 9, 14, split=split, gnt=True, scenes=("scene_a", "scene_b"))
    plain = harness.vis_run(VR.StubModel(), ds, None, tmp_path / "plain", batch_size=2)
    with_video = harness.vis_run(VR.StubModel(), ds, None, tmp_path / "video", batch_size=2, video=True)
    assert {k: v.relative_to(tmp_path / "plain") for k, v in plain.items()} == {
        k: v.relative_to(tmp_path / "video") for k, v in with_video.items()}
    base = f"{split}/" if split else ""
    before, after = _all_files(tmp_path / "plain"), _all_files(tmp_path / "video")
    assert all(name.endswith(".png") for name in before) and len(before) == 14  # the defaults: today's files, nothing else
    assert sorted(set(after) - set(before)) == [f"{base}scene_a_combined.avi", f"{base}scene_b_combined.avi"]
    assert set(before) <= set(after)
    for name in before:
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "video" / name).read_bytes(), name
    for scene in ("scene_a", "scene_b"):
        top, frames = R.avi_frames((tmp_path / "video" / f"{base}{scene}_combined.avi").read_bytes())
        assert frames == _expected_video(ds, range(7), scene)
        for f, it in zip(frames, sorted((it for it in ds.items if it["misc"]["scene_id"] == scene), key=lambda it: it["misc"]["tgt_idx"])):
            mode, size, pix = R.decode_pil(f)
            q8 = VR.expected_save_image(it["img"]).permute(1, 2, 0).numpy()  # the pixels of the view's *_combined.png
            assert size == (14, 9) and np.abs(pix - R.decode_model(video.jpeg_coefficients(q8, 90), *video.quant_tables(90), 9, 14)).max() <= 3


@pytest.mark.parametrize("n", [7, 8])
def test_vis_run_video_across_ranks(tmp_path, n):
    """7 items over 2 ranks: the sampler wraps item 0 round to rank 1, whose PNG upstream writes twice and whose frame the
    video holds once"""
    ds = VR.StubDataset(n, 9, 14, scenes=("scene_a", "scene_b", "scene_c"))
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "one", video=True, video_fps=5, video_quality=75)
    for rank in (1, 0):
        harness.vis_run(VR.StubModel(), ds, None, tmp_path / "two", rank=rank, world=2, video=True, video_fps=5, video_quality=75)
    parts = sorted(name for name in _all_files(tmp_path / "two") if ".part" in name)
    assert parts and all(re.fullmatch(r"\.scene_[abc]_combined\.part[01]", name) for name in parts)
    assert not any(name.endswith(".avi") for name in _all_files(tmp_path / "two"))
    with pytest.raises(FileNotFoundError):
        video.assemble(tmp_path / "two", 3)  # rank 2 left nothing
    assert sorted(name for name in _all_files(tmp_path / "two") if ".part" in name) == parts
    made = video.assemble(tmp_path / "two", 2)
    assert sorted(p.name for p in made) == ["scene_a_combined.avi", "scene_b_combined.avi", "scene_c_combined.avi"]
    assert _all_files(tmp_path / "one") == _all_files(tmp_path / "two")  # (no part is left behind)
    for name in _all_files(tmp_path / "one"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    top, frames = R.avi_frames((tmp_path / "one" / "scene_a_combined.avi").read_bytes())
    assert struct.unpack_from("<I", top.children[0].children[1].children[0].data, 24)[0] == 5  # strh's rate
    assert frames == [video.encode_jpeg(it["img"], 75) for it in ds.items if it["misc"]["scene_id"] == "scene_a"]


def test_writer_errors_and_arguments(tmp_path):
    ds = VR.StubDataset(3, 9, 14)
    w = video.MjpegWriter(n_threads=2)
    w.submit((tmp_path, "s"), 4, ds[0]["img"])
    with pytest.raises(ValueError):
        w.submit((tmp_path, "s"), 5, torch.zeros((3, 9, 15)))  # another size in the same scene
    with pytest.raises(ValueError):
        w.submit((tmp_path, "s"), 5, torch.zeros((9, 14)))
    w.submit((tmp_path, "s"), 1, ds[1]["img"])
    w.close()
    assert w.files == [tmp_path / "s_combined.avi"] and w.bytes_written == (tmp_path / "s_combined.avi").stat().st_size
    top, frames = R.avi_frames((tmp_path / "s_combined.avi").read_bytes())
    assert frames == [video.encode_jpeg(ds[1]["img"]), video.encode_jpeg(ds[0]["img"])]  # tgt_idx 1 before 4
    with pytest.raises(RuntimeError):
        w.submit((tmp_path, "s"), 9, ds[0]["img"])
    # a worker's failure (an empty frame, which the encoder refuses) surfaces at close(), once, and no file is written
    w = video.MjpegWriter(n_threads=1)
    w.submit((tmp_path, "t"), 0, ds[0]["img"])
    w.submit((tmp_path, "t2"), 1, torch.zeros((3, 0, 14)))
    with pytest.raises(ValueError):
        w.close()
    w.close()
    assert not (tmp_path / "t_combined.avi").exists()
    # a directory that is a regular file: the error of the file write surfaces at close() as well, through vis_run too
    blocker = tmp_path / "blocker"
    blocker.write_bytes(b"x")
    w = video.MjpegWriter()
    w.submit((blocker, "u"), 0, ds[0]["img"])
    with pytest.raises(OSError):
        w.close()
    for kw in (dict(n_threads=17), dict(fps=0), dict(quality=0), dict(restart_mcus=70000), dict(rank=2, world=2)):
        with pytest.raises(ValueError):
            video.MjpegWriter(**kw)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["blocker", "s_combined.avi"]


# ---------------------------------------------------------------------------- ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from pgdvs_amd import _lib

    head = (ROOT / "include" / "pgdvs_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name, nargs in (("pgdvs_jpeg_coefficients", 8), ("pgdvs_jpeg_scan", 11), ("pgdvs_jpeg_scan_workspace_bytes", 4)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert "visualizer_pgdvs.py:141-177" in head and "rendering.py:79-116" in head  # the reference lines they replace
    lib = _lib.load()
    assert lib.pgdvs_jpeg_scan_workspace_bytes(1, 135, 240, 240) >= 135 * 240 * 1248
    assert lib.pgdvs_jpeg_scan_workspace_bytes(1, 0, 240, 240) == -1       # H = 0
    assert lib.pgdvs_jpeg_scan_workspace_bytes(1, 135, 240, 0) == -1       # no restart markers: host-only
    assert lib.pgdvs_jpeg_scan_workspace_bytes(1, 8193, 240, 240) == -1    # H > 65535
    assert lib.pgdvs_jpeg_scan_workspace_bytes(64, 135, 240, 240) == -1    # 2^31


def test_ops_refuse_host_tensors_and_restart_zero():
    from pgdvs_amd import _lib, ops

    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8)))
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_scan(torch.zeros((1, 1, 1, 3, 64), dtype=torch.int16))
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_encode(torch.zeros((3, 8, 8)))
    assert ops.jpeg_scan_capacity(135, 240, 240) == 135 * 240 * 1248 + 2 * 134
    assert ops.jpeg_scan_capacity(1, 1, 5) == 1248
