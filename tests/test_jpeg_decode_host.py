"""The JPEG reader's host side (csrc/jpeg_entropy.cpp ``pgdvs_jpeg_parse`` / ``pgdvs_jpeg_entropy_decode``; the loaders'
``device_decode`` keyword): the parsed fields against Pillow's; the decoded coefficients, run through a numpy statement of the
reconstruction, give ``np.array(PIL.Image.open(...))`` byte for byte over the whole stream matrix; the streams the reader
leaves to Pillow are refused with 1 and a reason; the keyword is refused without ``device_resize=True``; and the decoder, built
alone with the host compiler's address and undefined-behaviour sanitizers, survives every truncation and 2000 single-byte
mutations of three streams."""
import ctypes as C
import io
import pathlib
import shutil
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import jpeg_decode_cases as JC  # noqa: E402
import resident_cases as RC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module", autouse=True)
def _turbo():
    JC.require_turbo()


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_parse_fields_equal_pillows(subsampling):
    for label, data in JC.matrix(subsampling):
        rc, info, msg = JC.parse(data)
        assert rc == 0, (label, rc, msg)
        im = PIL.Image.open(io.BytesIO(data))
        assert (info.width, info.height) == im.size, label
        h, v = im.layer[0][1], im.layer[0][2]
        assert im.layer[1][1:3] == im.layer[2][1:3] == (1, 1) and {(1, 1): 0, (2, 1): 1, (2, 2): 2}[h, v] == info.sampling == subsampling, label
        mw, mh = -(-info.width // (8 * h)), -(-info.height // (8 * v))
        assert list(info.blocks_w) == [mw * h, mw, mw] and list(info.blocks_h) == [mh * v, mh, mh], label
        assert info.coef_bytes == 128 * sum(a * b for a, b in zip(info.blocks_w, info.blocks_h)), label
        own = "own encoder" in label  # (video.encode_jpeg's default interval: one MCU row)
        want_rst = {"rst3": 3, "rst2": 2, "rst0": 0}.get(label.split()[-1], mw if own else 0)
        assert info.restart_interval == want_rst, (label, info.restart_interval)
        for c in range(3):  # Pillow gives the tables in natural order too
            assert np.array_equal(np.ctypeslib.as_array(info.quant)[c], np.array(im.quantization[im.layer[c][3]], np.uint16)), (label, c)


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_entropy_decode_and_the_numpy_reconstruction_equal_pillow(subsampling):
    n = 0
    for label, data in JC.matrix(subsampling):
        rc, info, msg = JC.parse(data)
        assert rc == 0, (label, rc, msg)
        rc, coef, msg = JC.entropy_decode(data, info.coef_bytes)
        assert rc == 0, (label, rc, msg)
        got, want = JC.reconstruct(info, coef), JC.pillow(data)
        assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape)
        assert np.array_equal(got, want), (label, int((got != want).sum()))
        n += 1
    assert n == len(JC.SIZES) * 12 + 6 + (9 if subsampling != 1 else 0)


def _refused(label, data):
    """parse, or the scan behind it, returns 1 with a reason; what a refusal must not write is checked"""
    rc, info, msg = JC.parse(data)
    assert rc in (0, 1), (label, rc, msg)
    if rc == 1:
        assert msg.startswith("jpeg: ") and len(msg) > 10, (label, msg)
        assert bytes(info) == b"\x5a" * C.sizeof(info), (label, "a refused parse wrote the info")
        rc2, coef, msg2 = JC.entropy_decode(data, 1024)  # the same refusal, in front of the size check and of any write
        assert rc2 == 1 and msg2 == msg and (coef == 0x5A5A).all(), (label, rc2, msg2)
        return msg
    rc, coef, msg = JC.entropy_decode(data, info.coef_bytes)  # (its canaries: nothing outside coef)
    assert rc == 1 and msg.startswith("jpeg: corrupt scan"), (label, rc, msg)
    return msg


def test_streams_left_to_pillow_are_refused_with_a_reason():
    words = {"progressive": "baseline", "greyscale": "three components", "cmyk": "three components", "keep_rgb": "Adobe", "png": "SOI",
             "empty": "SOI", "flipped RSTn": "restart marker"}
    for label, data in JC.refusals():
        if label == "4:1:1":
            continue
        assert words[label] in _refused(label, data), label
        if label == "flipped RSTn":  # (served by the markers: ops.jpeg_decode then takes pinned memory, tests/test_gpu_jpeg_decode.py)
            continue
        from pgdvs_amd import ops

        assert ops.jpeg_info(data) is None and ops.jpeg_decode(data, reject_ok=True) is None, label
        with pytest.raises(ValueError, match="not served"):
            ops.jpeg_decode(data)


def test_sampling_factors_other_than_the_three():
    """Pillow's ``subsampling="4:1:1"`` is its old name of 4:2:0 (JpegImagePlugin: "for compatibility"): the stream it writes
    has 2x2 luma and is served.  Real 4:1:1 (luma 4x1) and 4:4:0 (1x2) frame headers, and chroma factors other than 1x1, are
    refused by the markers alone."""
    data = dict(JC.refusals())["4:1:1"]
    assert PIL.Image.open(io.BytesIO(data)).layer[0][1:3] == (2, 2)
    rc, info, _ = JC.parse(data)
    assert rc == 0 and info.sampling == 2
    rc, coef, _ = JC.entropy_decode(data, info.coef_bytes)
    assert rc == 0 and np.array_equal(JC.reconstruct(info, coef), JC.pillow(data))
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x22 and data[sof + 14] == data[sof + 17] == 0x11
    for at, factor, word in ((11, 0x41, "luma"), (11, 0x12, "luma"), (11, 0x21, None), (14, 0x21, "chroma"), (17, 0x12, "chroma"), (11, 0x44, "luma")):
        bad = data[:sof + at] + bytes([factor]) + data[sof + at + 1:]
        if word is None:  # 4:2:2's factors over a 4:2:0 scan: served by the markers, the scan is then short or corrupt -- or decodes
            assert JC.parse(bad)[0] == 0
            continue
        assert word in _refused(f"factor {factor:#x} at {at}", bad)


def test_every_truncation_is_refused():
    data = JC.small_stream()
    assert JC.parse(data)[0] == 0 and len(data) < 2000
    for n in range(len(data)):
        msg = _refused(f"first {n} bytes", data[:n])
        assert "truncated" in msg or "SOI" in msg or "past the end" in msg, (n, msg)


def test_argument_errors_return_minus_one():
    from pgdvs_amd import _lib

    lib, data = _lib.load(), np.frombuffer(JC.small_stream(), np.uint8)
    info = _lib.JpegInfo()
    ptr = C.c_void_p(data.ctypes.data)
    assert lib.pgdvs_jpeg_parse(ptr, data.size, None) == -1 and b"null" in lib.pgdvs_last_error()
    assert lib.pgdvs_jpeg_parse(None, 5, C.byref(info)) == -1 and lib.pgdvs_jpeg_parse(ptr, -1, C.byref(info)) == -1
    assert lib.pgdvs_jpeg_parse(ptr, data.size, C.byref(info)) == 0
    coef = np.zeros(info.coef_bytes // 2 + 64, np.int16)
    assert lib.pgdvs_jpeg_entropy_decode(ptr, data.size, None, info.coef_bytes) == -1
    for wrong in (info.coef_bytes - 128, info.coef_bytes + 128, 0):
        assert lib.pgdvs_jpeg_entropy_decode(ptr, data.size, C.c_void_p(coef.ctypes.data), wrong) == -1 and b"coef_bytes" in lib.pgdvs_last_error()
    assert not coef.any()
    # the reconstruction's workspace query is host only: the planes over the padded grids, each rounded up to 256 bytes
    assert lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)) == 16 * 16 + 2 * 256  # 9 x 11 at 4:2:0: one MCU
    info.blocks_w[0] += 1
    assert lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)) == -1 and b"blocks" in lib.pgdvs_last_error()
    assert lib.pgdvs_jpeg_reconstruct_workspace_bytes(None) == -1


def test_sources_are_listed():
    make = (ROOT / "ml-pgdvs_amd" / "csrc" / "Makefile").read_text()
    assert "jpeg_entropy.cpp" in make and "jpeg_decode.hip" in make
    from pgdvs_amd import _lib, ops

    assert {"pgdvs_jpeg_parse", "pgdvs_jpeg_entropy_decode", "pgdvs_jpeg_reconstruct", "pgdvs_jpeg_reconstruct_workspace_bytes",
            "pgdvs_jpeg_info_size"} <= set(_lib.SIGNATURES)
    assert _lib.load().pgdvs_jpeg_info_size() == C.sizeof(_lib.JpegInfo) == 48 + 3 * 128
    data = JC.matrix(2)[0][1]
    info = ops.jpeg_info(data)
    assert (info["height"], info["width"], info["sampling"], info["blocks"]) == (8, 8, "4:2:0", [(2, 2), (1, 1), (1, 1)])
    assert info["quant"].shape == (3, 64) and info["quant"].dtype == np.uint16 and info["coef_bytes"] == 6 * 128
    with pytest.raises(ValueError, match="GPU"):
        ops.jpeg_decode(data, device="cpu")
    with pytest.raises(TypeError):
        ops.jpeg_info("a path is not a stream")


# ---------------------------------------------------------------------------- the sanitizers, on a stand-alone program
def test_the_decoder_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_entropy_fuzz"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tools" / "jpeg_entropy_fuzz.cpp"), str(ROOT / "ml-pgdvs_amd" / "csrc" / "jpeg_entropy.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("sanitize" in built.stderr or "asan" in built.stderr or "ubsan" in built.stderr):
        pytest.skip(f"{cxx} lacks the address / undefined sanitizers: {built.stderr.strip().splitlines()[-1]}")
    assert built.returncode == 0, built.stderr
    streams = {"s420.jpg": JC.small_stream(), "s444_rst.jpg": JC.encode(JC.content("noise", 10, 19), 0, 60, 1),
               "s422_opt.jpg": JC.encode(JC.content("smooth", 17, 23), 1, 90, None, True)}
    for name, data in streams.items():
        (tmp_path / name).write_bytes(data)
    run = subprocess.run([str(exe), "20261020", "2000", *(str(tmp_path / n) for n in streams)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 3 and all("other returns 0" in ln for ln in lines), run.stdout
    for ln, data in zip(lines, streams.values()):  # every truncation is refused; the mutations take all three exits
        served, by_markers, by_scan = (int(ln.split(w)[1].split(",")[0].split()[0]) for w in ("served", "by the markers", "by the scan"))
        assert served + by_markers + by_scan == 1 + len(data) + 2000 and by_markers >= len(data) and served > 1 and by_scan > 0, ln


# ---------------------------------------------------------------------------- the loaders' keyword
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("jpeg_host"))


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_decode_needs_device_resize(name, trees):
    """refused in the constructor, in front of everything else it does"""
    with pytest.raises(ValueError, match="device_resize=True"):
        RC.make(name, trees, device_decode=True)
    with pytest.raises(ValueError, match="device_resize=True"):
        RC.make(name, trees, device_decode=True, resident=True, device="cuda:0")
    with pytest.raises(ValueError, match="resident=True"):
        RC.make(name, trees, device_decode=True, device_resize=True)
    with pytest.raises(ValueError, match="GPU"):
        RC.make(name, trees, device_decode=True, device_resize=True, resident=True, device=None)
    if name != "nvidia_pure_geo":
        ds = RC.make(name, trees, resident=True, device=None)  # the default: off
        assert ds.store.device_decode is False and ds.store.stats["frames_decoded_on_device"] == 0 == ds.store.stats["jpeg_fallbacks"]


def test_device_decode_needs_device_resize_dycheck(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1,
              mode="eval", scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3,
              n_src_views_temporal_track_one_side=2)
    with pytest.raises(ValueError, match="device_resize=True"):
        DyCheckiPhoneEvaluationDataset(**kw, device_decode=True)
    with pytest.raises(ValueError, match="device_resize=True"):
        DyCheckiPhoneEvaluationDataset(**kw, device_decode=True, resident=True, device="cuda:0")
    assert DyCheckiPhoneEvaluationDataset(**kw, resident=True).store.device_decode is False
