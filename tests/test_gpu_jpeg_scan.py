"""The JPEG scan decoded on the MI355X (csrc/jpeg_scan_decode.hip over csrc/jpeg_scan_core.h; ``ops.jpeg_scan_decode``,
``ops.jpeg_decode(entropy="device")``, the loaders' ``device_entropy=True``): the kernels' coefficients against
``pgdvs_jpeg_entropy_decode``'s bit for bit over the stream matrix of tests/jpeg_decode_cases.py and the streams
tests/jpeg_scan_cases.py adds; the decoded image against Pillow and ``entropy="host"`` byte for byte, ``out=`` slots between
guard bytes included; damaged streams, each passed by the host emulation first, against what ``entropy="host"`` returns or
raises, with guard words round coef and the workspace; and the five loaders over trees of real JPEG files against the same
loaders with ``device_decode=True`` alone."""
import ctypes as C
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import jpeg_decode_cases as JC  # noqa: E402
import jpeg_scan_cases as SC  # noqa: E402
import resident_cases as RC  # noqa: E402
from resident_cases import NT  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    JC.require_turbo()
    from pgdvs_amd import _lib

    _lib.load()


def _want(label, data):
    rc, info, msg = JC.parse(data)
    assert rc == 0, (label, msg)
    rc, coef, msg = JC.entropy_decode(data, info.coef_bytes)
    assert rc == 0, (label, msg)
    return coef


def _check_scan(streams):
    from pgdvs_amd import ops

    for label, data in streams:
        coef, status = ops.jpeg_scan_decode(data, device=DEV)
        want = _want(label, data)
        assert status == 0, (label, status)
        assert coef.is_cuda and coef.dtype == torch.int16 and coef.numel() == want.size, (label, coef.shape)
        bad = np.flatnonzero(coef.cpu().numpy() != want)
        assert bad.size == 0, (label, bad.size, bad[:6].tolist())


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_scan_decode_equals_the_host_decoder_over_the_matrix(subsampling):
    streams = JC.matrix(subsampling)
    _check_scan(streams)
    assert len(streams) == len(JC.SIZES) * 12 + 6 + (9 if subsampling != 1 else 0)


def test_scan_decode_equals_the_host_decoder_on_the_added_streams():
    from pgdvs_amd import ops

    _check_scan(SC.added())
    big = dict(SC.added())["256x384 noise q100 4:4:4: more than two workgroups"]
    coef, status, (rounds, fixups) = ops.jpeg_scan_decode(big, device=DEV, return_rounds=True)
    assert status == 0 and 1 <= rounds <= SC.GROUP + 1 and fixups >= 1, (status, rounds, fixups)  # more than one workgroup: a fix-up ran
    for sub in (16, 64, 256, 4096):  # every size the entry takes gives the same coefficients
        coef, status = ops.jpeg_scan_decode(big, device=DEV, sub_bytes=sub)
        assert status == 0 and np.array_equal(coef.cpu().numpy(), _want("big", big)), sub


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_jpeg_decode_with_the_scan_on_the_device_equals_pillow_and_the_host_path(subsampling):
    from pgdvs_amd import ops

    streams = JC.matrix(subsampling) + (SC.added() if subsampling == 0 else [])
    for label, data in streams:
        got, on_device = ops.jpeg_decode_device(data, device=DEV)
        want = JC.pillow(data)
        assert on_device, label
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous(), (label, got.shape, want.shape)
        assert np.array_equal(got.cpu().numpy(), want), label
        assert torch.equal(ops.jpeg_decode(data, device=DEV, entropy="device"), ops.jpeg_decode(data, device=DEV, entropy="host")), label


def test_out_into_a_padded_slot_between_guard_bytes():
    from pgdvs_amd import ops

    for subsampling in JC.SUBSAMPLINGS:
        for h, w in ((5, 3), (17, 23), (33, 49)):
            data = JC.encode(JC.content("noise", h, w, 3), subsampling, 90)
            per = h * w * 3
            slot = -(-per // 16) * 16 + 16
            tab = torch.full((3, slot), CANARY, dtype=torch.uint8, device=DEV)
            out = tab[1, :per].view(h, w, 3)
            assert ops.jpeg_decode(data, out=out, entropy="device") is out
            got = tab.cpu().numpy()
            assert np.array_equal(got[1, :per].reshape(h, w, 3), JC.pillow(data)), (subsampling, h, w)
            assert (got[1, per:] == CANARY).all() and (got[[0, 2]] == CANARY).all(), (subsampling, h, w, "bytes outside the frame were written")
    with pytest.raises(ValueError, match="out"):
        ops.jpeg_decode(JC.encode(JC.content("noise", 17, 23), 2, 90), out=torch.zeros((17, 24, 3), dtype=torch.uint8, device=DEV), entropy="device")
    for label, data in JC.refusals():  # what the markers refuse never reaches the device: the host path's answer
        if label != "4:1:1":
            assert ops.jpeg_decode(data, reject_ok=True, entropy="device") is None, label
            with pytest.raises(ValueError, match="not served: jpeg: "):
                ops.jpeg_decode(data, entropy="device")


def _damaged():
    """three cuts inside the scan (EOI kept: the markers serve them), three truncations, the flipped RSTn and five mutations in
    the scan of a restart stream"""
    small = JC.small_stream()
    begin, end = SC.scan_extent(small)
    out = [(f"scan cut to {n} bytes", small[:begin + n] + small[end:]) for n in (1, (end - begin) // 2, end - begin - 1)]
    out += [(f"first {n} bytes", small[:n]) for n in (begin - 1, begin + 20, len(small) - 1)]
    out.append(("flipped RSTn", dict(JC.refusals())["flipped RSTn"]))
    data = JC.encode(JC.content("noise", 40, 56, 9), 0, 85, 2)
    begin, end = SC.scan_extent(data)
    rng = np.random.default_rng(20261021)
    for k in range(5):
        at = int(rng.integers(begin, end))
        out.append((f"mutation {k} at {at}", data[:at] + bytes([data[at] ^ (1 << int(rng.integers(0, 8)))]) + data[at + 1:]))
    return out


def test_damaged_streams_give_what_the_host_path_gives():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    for label, data in _damaged():
        SC.check_against_host_decoder(label, data, intact=False)  # the emulation first, on the CPU: its guards hold
        want = ops.jpeg_decode(data, device=DEV, reject_ok=True, entropy="host")
        got, on_device = ops.jpeg_decode_device(data, device=DEV, reject_ok=True)
        assert (got is None) == (want is None), label
        if want is None:
            assert not on_device, label
            with pytest.raises(ValueError, match="not served"):
                ops.jpeg_decode(data, device=DEV, entropy="device")
        else:
            assert torch.equal(got, want), label
        # the C entry itself, guard words round coef, the status word and the workspace
        prepared = ops.jpeg_scan_prepare(data)
        if prepared is None:
            continue
        prepared, info = prepared
        n, need = info.coef_bytes // 2, lib.pgdvs_jpeg_scan_decode_workspace_bytes(C.c_void_p(prepared.data_ptr()), prepared.numel())
        dev = prepared.to(DEV)
        mem = torch.full((128 + n + 128,), 0x5A5A, dtype=torch.int16, device=DEV)
        wmem = torch.full((256 + need + 256,), CANARY, dtype=torch.uint8, device=DEV)
        status = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        off = (-wmem.data_ptr()) % 256
        _lib.check(lib.pgdvs_jpeg_scan_decode(C.c_void_p(prepared.data_ptr()), C.c_void_p(dev.data_ptr()), prepared.numel(),
                                              C.c_void_p(mem.data_ptr() + 256), info.coef_bytes, C.c_void_p(status.data_ptr() + 16),
                                              C.c_void_p(wmem.data_ptr() + off), need, ops._stream()), "pgdvs_jpeg_scan_decode")
        m, wm, st = mem.cpu().numpy(), wmem.cpu().numpy(), status.cpu().numpy()
        assert (m[:128] == 0x5A5A).all() and (m[128 + n:] == 0x5A5A).all(), (label, "written outside coef")
        assert (wm[:off] == CANARY).all() and (wm[off + need:] == CANARY).all(), (label, "written outside the workspace")
        assert (np.delete(st, 4) == 0x5A5A5A5A).all() and (want is not None or st[4] != 0), (label, st)
        if st[4] == 0:
            assert np.array_equal(m[128:128 + n], _want(label, data)), label


# ---------------------------------------------------------------------------- the loaders
BIG = (701, 83)  # for the 288 x 36 frames
PROGRESSIVE, GREY, PNG_BYTES = (3, 3), (2, 7), ((5, 5), (6, 1))  # (time step, camera)


def _jpeg(path, hw, rng, **kw):
    base = JC.content("smooth", *hw).astype(np.int32) + rng.integers(-20, 21, (*hw, 3))
    PIL.Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).convert(kw.pop("mode", "RGB")).save(path, format="JPEG", quality=90, **kw)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the resident tests' trees with real JPEG files, as tests/test_gpu_jpeg_decode.py builds them: every mv_images file of the
    NVIDIA tree under its .jpg name alone, sampling (f + c) % 3, half of them at 701 x 83, every third with restart markers;
    source frame 3 progressive, the target (2, 7) greyscale, (5, 5) and (6, 1) PNG bytes under the .jpg name.  Monocular tree:
    JPEG bytes under the .png names but for frame 2."""
    t = RC.build_trees(tmp_path_factory.mktemp("jpeg_scan_gpu"))
    rng = np.random.default_rng(20261021)
    dense = pathlib.Path(t["nvidia"]) / "raw" / NT.SCENE / "dense"
    for f in range(NT.F):
        for c in range(NT.N_CAMS):
            png = dense / "mv_images" / f"{f:05d}" / f"cam{c + 1:02d}.png"
            jpg = png.with_suffix(".jpg")
            png.unlink()
            hw = BIG if ((f + c) // 2) % 2 else (NT.H, NT.W)
            if (f, c) == PROGRESSIVE:
                _jpeg(jpg, hw, rng, progressive=True)
            elif (f, c) == GREY:
                _jpeg(jpg, (NT.H, NT.W), rng, mode="L")
            elif (f, c) not in PNG_BYTES:
                _jpeg(jpg, hw, rng, subsampling=(f + c) % 3, **({"restart_marker_blocks": 2} if (f + 2 * c) % 3 == 0 else {}))
    mono = pathlib.Path(t["mono"]) / NT.MONO_SCENE / "rgbs"
    names = sorted(mono.iterdir())
    h, w = PIL.Image.open(names[0]).size[::-1]
    for f, name in enumerate(names):
        if f != 2:
            _jpeg(name, (h, w) if f % 3 == 0 else (97, 131), rng, subsampling=f % 3)
    return t


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_entropy_items_equal_the_device_decode_loaders(name, trees):
    kw = dict(device=DEV, resident=True, device_resize=True, device_decode=True)
    want, got = RC.make(name, trees, **kw), RC.make(name, trees, **kw, device_entropy=True)
    assert got.store.device_entropy and not want.store.device_entropy
    for i in range(len(want)):
        RC.assert_items_equal(got[i], want[i], (name, i))
    st, ref = got.store.stats, want.store.stats
    assert ref["scans_decoded_on_device"] == ref["entropy_fallbacks"] == 0
    for key in ("frames_decoded", "frames_decoded_on_device", "targets_decoded_on_device", "jpeg_fallbacks", "frames_resized_on_device"):
        assert st[key] == ref[key], (key, st[key], ref[key])
    # every file the device reconstructs had its scan decoded there too: the intact files never fall back
    assert st["entropy_fallbacks"] == 0 and st["scans_decoded_on_device"] == st["frames_decoded_on_device"] + st["targets_decoded_on_device"] > 0
    if name == "mono_vis":
        assert st["jpeg_fallbacks"] == 0
    elif name == "nvidia_vis":  # the progressive source frame reaches Pillow
        assert st["jpeg_fallbacks"] == 1
    else:  # the progressive file twice (source frame and target) and the greyscale target; the PNG bytes never count
        assert st["jpeg_fallbacks"] == 3
