"""The visualiser's video at 4:2:0 on the host (pgdvs_amd/video.py with ``subsampling="4:2:0"``, harness.vis_run with
``video_subsampling``): without restart markers the scan is byte for byte what PIL (libjpeg) writes at ``subsampling=2`` and
the standard Huffman tables, restart markers change bytes and not the picture, crafted edges show libjpeg's dummy blocks and
its replicated downsampled chroma row in the coefficient array itself, 4:4:4 keeps its bytes, and the writer, the loop and
the C ABI carry the option through.  The AVI is checked structurally; it has not been opened in a player."""
import io
import pathlib
import re
import struct
import sys

import numpy as np
import PIL.Image
import pytest
import torch
from scipy.fft import idctn

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import video_reference as R  # noqa: E402
import vis_reference as VR  # noqa: E402

from pgdvs_amd import harness, video  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
S420 = "4:2:0"
SIZES = [(1, 1), (2, 2), (8, 8), (24, 8), (8, 24), (9, 14), (10, 10), (16, 16), (7, 23), (17, 33), (33, 17), (31, 15), (18, 34),
         (40, 70), (64, 80), (37, 53), (288, 550)]
SOF_420 = bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])


def _pil_420(im, quality):
    b = io.BytesIO()
    PIL.Image.fromarray(im).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
    return b.getvalue()


def _images(H, W):
    """uniform noise, and a smooth ramp (another slope per channel) with small noise"""
    rng = np.random.default_rng(1000 * H + W)
    yield "noise", rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    ramp = np.add.outer(3.0 * np.arange(H), 2.0 * np.arange(W))[..., None] * np.array([1.0, 0.5, -0.7]) + np.array([10.0, 60.0, 250.0])
    yield "smooth", np.clip(ramp + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)


def _scan(data):
    """the bytes between the SOS header and EOI"""
    assert data[-2:] == b"\xff\xd9"
    return data[R.segments(data)[1]:-2]


# ---------------------------------------------------------------------------- against PIL
@pytest.mark.parametrize("H,W", SIZES)
def test_scan_bytes_are_pils_at_420(H, W):
    nmy, nmx = (H + 15) // 16, (W + 15) // 16
    for name, im in _images(H, W):
        for q in (50, 90, 100):
            coef = video.jpeg_coefficients(im, q, subsampling=S420)
            assert coef.shape == (nmy, nmx, 6, 64) and coef.dtype == np.int16
            ours, theirs = video.encode_jpeg(im, q, 0, subsampling=S420), _pil_420(im, q)
            assert _scan(ours) == _scan(theirs), (name, q, "the scan differs from PIL's")
            seg = dict(R.segments(ours)[0])
            assert struct.unpack(">BHHB", seg[0xC0][:6]) == (8, H, W, 3) and seg[0xC0][6:] == SOF_420
            assert seg[0xC0] == dict(R.segments(theirs)[0])[0xC0] and 0xDD not in seg
            mode, size, pix = R.decode_pil(ours)
            assert mode == "RGB" and size == (W, H) and np.array_equal(pix, R.decode_pil(theirs)[2])


# ---------------------------------------------------------------------------- restart markers
@pytest.mark.parametrize("H,W", [(9, 17), (37, 53), (40, 70)])
def test_restart_markers_change_bytes_not_the_picture(H, W):
    nmy, nmx = video.mcu_grid(H, W, S420)
    n_mcu = nmy * nmx
    for name, im in _images(H, W):
        plain = R.decode_pil(video.encode_jpeg(im, 90, 0, subsampling=S420))[2]
        for restart in (1, 4, nmx, None, n_mcu + 7):
            interval = nmx if restart is None else restart
            data = video.encode_jpeg(im, 90, restart, subsampling=S420)
            seg = dict(R.segments(data)[0])
            assert struct.unpack(">H", seg[0xDD])[0] == interval and seg[0xC0][6:] == SOF_420
            scan = _scan(data)
            after_ff = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF]
            assert [v for v in after_ff if v != 0] == [0xD0 + (i & 7) for i in range((n_mcu + interval - 1) // interval - 1)], (name, restart)
            mode, size, pix = R.decode_pil(data)
            assert size == (W, H) and np.array_equal(pix, plain), (name, restart)
        assert video.encode_jpeg(im, 90, None, subsampling=S420) == video.encode_jpeg(im, 90, nmx, subsampling=S420)


def test_dc_prediction_runs_per_component_and_restarts_at_zero():
    """two MCUs of DC-only blocks with a restart between them: each segment's bytes are those of a frame of its own, so Y, Cb
    and Cr all predict from 0 behind the marker (prediction across MCUs without restarts is in every PIL comparison above)"""
    coef = np.zeros((1, 2, 6, 64), np.int16)
    coef[0, 0, :, 0] = (5, 9, -3, 40, 100, -100)
    coef[0, 1, :, 0] = (41, 7, 7, -20, 90, -90)
    both = video.encode_scan(coef, 1)
    cut = both.index(b"\xff\xd0")
    assert both[:cut] == video.encode_scan(coef[:, :1], 0) and both[cut + 2:] == video.encode_scan(coef[:, 1:], 0)


# ---------------------------------------------------------------------------- crafted edges
def _edge_image(H, W):
    """mid grey with a little texture; the last row and the last column differ sharply from their neighbours"""
    rng = np.random.default_rng(H * 31 + W)
    im = (120 + rng.integers(-6, 7, (H, W, 3))).astype(np.uint8)
    im[-1, :] = (250, 20, 30)
    im[:, -1] = (10, 240, 200)
    return im


@pytest.mark.parametrize("H,W", [(8, 8), (9, 17), (24, 8)])
def test_crafted_edges_show_dummy_blocks_and_the_replicated_chroma_row(H, W):
    im = _edge_image(H, W)
    nmy, nmx = video.mcu_grid(H, W, S420)
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    coef = video.jpeg_coefficients(im, 100, subsampling=S420)  # every divisor 1: nothing hides in the quantiser
    assert coef.shape == (nmy, nmx, 6, 64)
    full = video.jpeg_coefficients(im, 100)  # the 4:4:4 luma blocks are the real 4:2:0 ones
    n_dummy = 0
    for my in range(nmy):
        for mx in range(nmx):
            for k in range(4):
                by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                blk = coef[my, mx, k]
                if by < nby and bx < nbx:
                    assert np.array_equal(blk, full[by, bx, 0]), (my, mx, k)
                    continue
                n_dummy += 1
                source = 1 if by >= nby else k - 1  # a bottom row: Y01, dummy or not; a right edge: the left neighbour
                assert not blk[1:].any(), (my, mx, k, "a dummy block has AC coefficients")
                assert blk[0] == coef[my, mx, source, 0], (my, mx, k, source)
    assert n_dummy == 4 * nmy * nmx - nby * nbx and n_dummy > 0
    # chroma, independently of PIL and of the forward DCT: the exact inverse DCT of the coefficients (Q = 1) gives the chroma
    # samples back to within 10 levels -- a coefficient is off by at most 0.5 + 0.18 (rounding, the integer DCT:
    # test_integer_dct_against_the_exact_one) and a sample sums 64 of them with weights whose magnitudes add up to at most
    # (sqrt(1/8) + 7 / 2)^2 = 14.9 -- and the edge rows differ from their neighbours by far more
    tol = 10.0
    hc = (H + 1) // 2
    ycc = video.rgb_to_ycc(im[:, np.minimum(np.arange(16 * nmx), W - 1)]).astype(np.float64)
    for comp in (0, 1):
        nat = np.zeros((nmy, nmx, 64))
        nat[..., R.NATURAL] = coef[:, :, 4 + comp]
        got = (idctn(nat.reshape(nmy, nmx, 8, 8), axes=(-2, -1), norm="ortho") + 128.0).transpose(0, 2, 1, 3).reshape(8 * nmy, 8 * nmx)
        p = ycc[..., 1 + comp]
        rows = [(p[min(2 * j, H - 1), 0::2] + p[min(2 * j, H - 1), 1::2] + p[min(2 * j + 1, H - 1), 0::2] + p[min(2 * j + 1, H - 1), 1::2]) / 4.0
                for j in range(hc)]
        assert np.abs(got[:hc] - np.stack(rows)).max() <= tol + 0.75, comp  # (the bias and the shift: at most 0.75)
        assert 8 * nmy > hc
        assert np.abs(got[hc:] - rows[-1]).max() <= tol + 0.75, (comp, "the rows past the last downsampled one do not repeat it")
        if H % 2 == 0 and comp == 1:  # the last pair is (H - 2, H - 1): input rows replicated BEFORE the average would give row H - 1
            naive = (p[H - 1, 0::2] + p[H - 1, 1::2]) / 2.0
            inside = (W - 1) // 2  # the chroma columns left of the sharp last column
            assert inside >= 3 and np.abs(naive - rows[-1])[:inside].min() > 4 * tol
            assert np.abs(got[hc:] - naive)[:, :inside].min() > tol
    # and PIL agrees with the whole
    assert _scan(video.encode_jpeg(im, 100, 0, subsampling=S420)) == _scan(_pil_420(im, 100))


def test_bottom_dummy_row_takes_y01_even_when_y01_is_a_dummy():
    """8 x 8: Y01 is a right-edge dummy (DC of Y00) and the bottom row copies it; 8 x 24's second MCU likewise, its first MCU
    has a real Y01 whose DC differs from Y00's"""
    im = _edge_image(8, 24)
    im[:, 8:16] = (30, 200, 90)
    coef = video.jpeg_coefficients(im, 100, subsampling=S420)
    assert coef.shape == (1, 2, 6, 64)
    assert coef[0, 0, 0, 0] != coef[0, 0, 1, 0]                               # a real Y01
    assert coef[0, 0, 2, 0] == coef[0, 0, 3, 0] == coef[0, 0, 1, 0]           # both of the row take Y01, not Y00 / Y10
    assert coef[0, 1, 1, 0] == coef[0, 1, 0, 0] and not coef[0, 1, 1, 1:].any()  # the dummy Y01 of the last MCU
    assert coef[0, 1, 2, 0] == coef[0, 1, 3, 0] == coef[0, 1, 1, 0]
    assert not coef[0, :, 2:4, 1:].any()


# ---------------------------------------------------------------------------- 4:4:4 untouched, arguments
def test_444_is_untouched():
    for H, W in ((9, 17), (37, 53)):
        for name, im in _images(H, W):
            for restart in (0, 3, None):
                assert video.encode_jpeg(im, 90, restart) == video.encode_jpeg(im, 90, restart, subsampling="4:4:4")
            assert np.array_equal(video.jpeg_coefficients(im, 50), video.jpeg_coefficients(im, 50, subsampling="4:4:4"))
            assert video.jpeg_coefficients(im, 50).shape == ((H + 7) // 8, (W + 7) // 8, 3, 64)
            scan = video.encode_scan(video.jpeg_coefficients(im, 50))
            assert video.jpeg_frame(scan, H, W, 50) == video.jpeg_frame(scan, H, W, 50, None, "4:4:4") == video.encode_jpeg(im, 50)
            assert _scan(video.encode_jpeg(im, 90, 0)) == _scan(R.pil_jpeg(im, 90, optimize=False))
    assert video.encode_jpeg(im, 90) != video.encode_jpeg(im, 90, subsampling=S420)


def test_bad_arguments():
    im = np.zeros((8, 8, 3), np.uint8)
    for bad in ("4:2:2", "420", 2, None, "4:1:1"):
        with pytest.raises(ValueError):
            video.jpeg_coefficients(im, 90, subsampling=bad)
        with pytest.raises(ValueError):
            video.jpeg_frame(b"", 8, 8, 90, None, subsampling=bad)
        with pytest.raises(ValueError):
            video.encode_jpeg(im, subsampling=bad)
        with pytest.raises(ValueError):
            video.MjpegWriter(subsampling=bad)
        with pytest.raises(ValueError):
            video.DeviceScan(None, None, 8, 8, subsampling=bad)
    with pytest.raises(ValueError):
        video.jpeg_coefficients(im.astype(np.int32), 90, subsampling=S420)
    with pytest.raises(ValueError):
        video.encode_scan(np.zeros((1, 1, 4, 64), np.int16))
    with pytest.raises(ValueError):
        video.encode_scan(np.zeros((1, 1, 6, 64), np.int16), 65536)
    with pytest.raises(ValueError):
        video.encode_jpeg(im, 0, subsampling=S420)
    with pytest.raises(ValueError):
        harness.vis_run(VR.StubModel(), VR.StubDataset(1, 9, 14), None, "unused", video=True, video_subsampling="4:2:2")


# ---------------------------------------------------------------------------- the writer and the loop
def _all_files(root):
    return sorted(p.relative_to(root).as_posix() for p in pathlib.Path(root).rglob("*") if p.is_file())


def test_writer_at_420(tmp_path):
    ds = VR.StubDataset(3, 9, 14)
    with video.MjpegWriter(n_threads=2, subsampling=S420) as w:
        assert w.subsampling == S420
        w.submit((tmp_path, "s"), 4, ds[0]["img"])
        w.submit((tmp_path, "s"), 1, ds[1]["img"])
        with pytest.raises(ValueError):  # a scan made at another sampling would get the wrong header
            w.submit((tmp_path, "s"), 2, video.DeviceScan(None, None, 9, 14))
    top, frames = R.avi_frames((tmp_path / "s_combined.avi").read_bytes())
    assert frames == [video.encode_jpeg(ds[1]["img"], subsampling=S420), video.encode_jpeg(ds[0]["img"], subsampling=S420)]
    assert video.MjpegWriter().subsampling == "4:4:4" and video.DeviceScan(None, None, 8, 8).subsampling == "4:4:4"
    # the container does not depend on the sampling: strf is the 4:4:4 writer's
    (tmp_path / "x").mkdir()
    with video.MjpegWriter(n_threads=2) as w4:
        w4.submit((tmp_path / "x", "s"), 4, ds[0]["img"])
        w4.submit((tmp_path / "x", "s"), 1, ds[1]["img"])
    strf = lambda t: t.children[0].children[1].children[1].data  # noqa: E731
    top4, frames4 = R.avi_frames((tmp_path / "x" / "s_combined.avi").read_bytes())
    assert strf(top) == strf(top4) and frames4 != frames


def test_vis_run_video_at_420(tmp_path):
    ds = VR.StubDataset(7, 9, 14, split="val", gnt=True, scenes=("scene_a", "scene_b"))
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "plain", batch_size=2)
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "video", batch_size=2, video=True, video_subsampling=S420)
    before, after = _all_files(tmp_path / "plain"), _all_files(tmp_path / "video")
    assert sorted(set(after) - set(before)) == ["val/scene_a_combined.avi", "val/scene_b_combined.avi"] and set(before) <= set(after)
    for name in before:  # the PNGs are the ones of a run without video
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "video" / name).read_bytes(), name
    for scene in ("scene_a", "scene_b"):
        top, frames = R.avi_frames((tmp_path / "video" / "val" / f"{scene}_combined.avi").read_bytes())
        items = sorted((it for it in ds.items if it["misc"]["scene_id"] == scene), key=lambda it: it["misc"]["tgt_idx"])
        assert frames == [video.encode_jpeg(VR.expected_save_image(it["img"]).permute(1, 2, 0).numpy(), 90, subsampling=S420) for it in items]
        for f in frames:
            assert dict(R.segments(f)[0])[0xC0][6:] == SOF_420 and R.decode_pil(f)[1] == (14, 9)
    # a writer handed in decides for itself
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "own", batch_size=2, video=video.MjpegWriter(subsampling=S420))
    assert (tmp_path / "own" / "val" / "scene_a_combined.avi").read_bytes() == (tmp_path / "video" / "val" / "scene_a_combined.avi").read_bytes()


def test_vis_run_video_at_420_across_ranks(tmp_path):
    ds = VR.StubDataset(7, 9, 14, scenes=("scene_a", "scene_b", "scene_c"))
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "one", video=True, video_subsampling=S420)
    for rank in (1, 0):
        harness.vis_run(VR.StubModel(), ds, None, tmp_path / "two", rank=rank, world=2, video=True, video_subsampling=S420)
    assert not any(name.endswith(".avi") for name in _all_files(tmp_path / "two"))
    video.assemble(tmp_path / "two", 2)
    assert _all_files(tmp_path / "one") == _all_files(tmp_path / "two")
    for name in _all_files(tmp_path / "one"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    top, frames = R.avi_frames((tmp_path / "one" / "scene_a_combined.avi").read_bytes())
    assert frames == [video.encode_jpeg(it["img"], 90, subsampling=S420) for it in ds.items if it["misc"]["scene_id"] == "scene_a"]


# ---------------------------------------------------------------------------- ABI
def test_header_declares_and_lib_binds_the_420_entry_points():
    from pgdvs_amd import _lib, ops

    head = (ROOT / "include" / "pgdvs_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name, sibling in (("pgdvs_jpeg_coefficients_420", "pgdvs_jpeg_coefficients"), ("pgdvs_jpeg_scan_420", "pgdvs_jpeg_scan"),
                          ("pgdvs_jpeg_scan_420_workspace_bytes", "pgdvs_jpeg_scan_workspace_bytes")):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[sibling][1]), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sibling]
    lib = _lib.load()
    assert lib.pgdvs_abi_version() == 1
    query = lib.pgdvs_jpeg_scan_420_workspace_bytes
    assert query(1, 68, 120, 120) >= 68 * 120 * 2496
    assert query(1, 0, 120, 120) == -1      # nmy = 0
    assert query(1, 68, 120, 0) == -1       # no restart markers: host-only
    assert query(1, 4097, 120, 120) == -1   # more than 65536 rows
    assert query(1, 4096, 1, 1) > 0
    assert query(128, 68, 120, 120) == -1   # 2^31
    assert ops.jpeg_scan_capacity(68, 120, 120, 6) == 68 * 120 * 2496 + 2 * 67
    assert ops.jpeg_scan_capacity(1, 1, 5, blocks_per_mcu=6) == 2496 and ops.jpeg_scan_capacity(1, 1, 5) == 1248
    with pytest.raises(ValueError):
        ops.jpeg_scan_capacity(1, 1, 1, 4)
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8)), subsampling=S420)
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_scan(torch.zeros((1, 1, 1, 6, 64), dtype=torch.int16))
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_encode(torch.zeros((3, 8, 8)), subsampling=S420)
    with pytest.raises(ValueError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8)), subsampling="4:2:2")
