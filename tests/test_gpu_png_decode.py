"""PNG frames decoded on the MI355X (csrc/png_inflate.hip and csrc/png_unfilter.hip over csrc/png_inflate_core.h;
``ops.png_decode``, ``ops.png_decode_batch``, the loaders' ``device_png=True``): the decoded image against Pillow byte for byte
over the streams of tests/png_decode_cases.py, one file at a time and in batches of mixed sizes, ``out=`` slots between guard
bytes at all four row alignments, ``channels="rgb"``; the damaged streams, each passed by the host emulation first, through
the op and through the C entry with guard words round output, status and workspace; and the five loaders over trees of
real PNG files against the same loaders with ``device_resize=True`` alone, with the fallbacks counted and one wait per item
fill."""
import ctypes as C
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import png_decode_cases as PC  # noqa: E402
import resident_cases as RC  # noqa: E402
from resident_cases import NT  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def wanted():
    """Pillow's array of every stream, computed once"""
    return {label: PC.pillow(data) for label, data in PC.streams()}


def test_png_decode_equals_pillow_over_the_streams(wanted):
    from pgdvs_amd import ops

    for label, data in PC.streams():
        got = ops.png_decode(data, device=DEV)
        want = wanted[label]
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (label, got.shape, want.shape)
        assert np.array_equal(got.cpu().numpy(), want), label


@pytest.mark.parametrize("sub_bytes", [8, 256])
def test_other_subsequence_sizes_give_the_same_images(wanted, sub_bytes):
    from pgdvs_amd import ops

    streams = PC.streams()
    for (label, _), got in zip(streams, ops.png_decode_batch([d for _, d in streams], device=DEV, sub_bytes=sub_bytes)):
        assert np.array_equal(got.cpu().numpy(), wanted[label]), (label, sub_bytes)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_batches_of_mixed_sizes(wanted, n):
    from pgdvs_amd import ops

    streams = PC.streams()
    picks = [streams[(5 * k + 3 * n) % len(streams)] for k in range(n)]  # sizes, channels and block kinds mixed
    stats = []
    got = ops.png_decode_batch([d for _, d in picks], device=DEV, stats=stats)
    assert len(got) == n and all(s is not None and s[3] >= 1 for s in stats)
    for (label, _), g in zip(picks, got):
        assert np.array_equal(g.cpu().numpy(), wanted[label]), (n, label)


def test_a_batch_with_unserved_files_serves_the_others(wanted):
    from pgdvs_amd import ops

    (label, good), bad_host, bad_stream = PC.streams()[12], PC.host_refusals()[0][1], PC.device_refusals()[0][1]
    reasons = []
    got = ops.png_decode_batch([bad_host, good, bad_stream, good], device=DEV, reject_ok=True, reasons=reasons)
    assert got[0] is None and got[2] is None and "colour type" in reasons[0] and "adler" in reasons[2] and reasons[1] is None
    assert np.array_equal(got[1].cpu().numpy(), wanted[label]) and np.array_equal(got[3].cpu().numpy(), wanted[label])
    with pytest.raises(ValueError, match="file 2 is not served.*adler"):
        ops.png_decode_batch([good, good, bad_stream], device=DEV)


def test_out_into_padded_slots_between_guard_bytes_at_all_row_alignments(wanted):
    from pgdvs_amd import ops

    streams = dict(PC.streams())
    for label in ("5x63x3 rows cycling 0..4", "65x9x4 rows cycling 0..4", "130x7x3 rows cycling 0..4", "1x70x4 rows cycling 0..4"):
        want = wanted[label]
        h, w, c = want.shape
        for shift in range(4):
            for pad in (0, 5):  # rows that follow each other, and rows with bytes between them
                pitch = w * c + pad
                mem = torch.full((64 + shift + h * pitch + 64,), CANARY, dtype=torch.uint8, device=DEV)
                out = mem[64 + shift:64 + shift + h * pitch].view(h, pitch)[:, :w * c].view(h, w, c) if pad else mem[64 + shift:64 + shift + h * pitch].view(h, w, c)
                assert out.data_ptr() % 4 == (mem.data_ptr() + 64 + shift) % 4
                assert ops.png_decode(streams[label], out=out) is out
                got = mem.cpu().numpy()
                body = got[64 + shift:64 + shift + h * pitch].reshape(h, pitch)
                assert np.array_equal(body[:, :w * c].reshape(h, w, c), want), (label, shift, pad)
                assert (body[:, w * c:] == CANARY).all() and (got[:64 + shift] == CANARY).all() and (got[64 + shift + h * pitch:] == CANARY).all(), (
                    label, shift, pad, "bytes outside the frame were written")
    with pytest.raises(ValueError, match="out"):
        ops.png_decode(streams["5x63x3 rows cycling 0..4"], out=torch.zeros((5, 64, 3), dtype=torch.uint8, device=DEV))


def test_rgb_of_rgba_files(wanted):
    from pgdvs_amd import ops

    picks = [(lb, d) for lb, d in PC.streams() if PC.split(d)[2] == 4]
    for (label, _), got in zip(picks, ops.png_decode_batch([d for _, d in picks], channels="rgb", device=DEV)):
        assert tuple(got.shape) == wanted[label].shape[:2] + (3,) and np.array_equal(got.cpu().numpy(), wanted[label][..., :3]), label
    rgb = dict(PC.streams())["5x64x3 rows cycling 0..4"]
    assert torch.equal(ops.png_decode(rgb, channels="rgb", device=DEV), ops.png_decode(rgb, device=DEV))


def test_the_projects_own_png_output_is_read_back():
    """what ``pgdvs_amd.png`` writes -- scanlines filtered in HIP, then stored (level 0), deflated by zlib, or deflated in HIP
    (run-length + Huffman, csrc/png_deflate.hip) -- decodes to what Pillow reads from the same file"""
    from pgdvs_amd import ops, png

    gen = torch.Generator().manual_seed(5)
    img = torch.rand((2, 3, 45, 70), generator=gen).to(DEV)
    img[1, :, 10:30, 20:50] = 0.25  # flat areas: runs
    lines = ops.png_scanlines(img)  # adaptive filters
    H, W = 45, 70
    data, nbytes = ops.png_deflate(lines)
    files = []
    for i in range(2):
        host = lines[i].cpu().numpy()
        files += [png.encode(host, H, W, level=0), png.encode(host, H, W, level=1),
                  png.png_from_zstream(data[i, :int(nbytes[i])].cpu().numpy().tobytes(), H, W)]
    for k, (got, f) in enumerate(zip(ops.png_decode_batch(files, device=DEV), files)):
        assert np.array_equal(got.cpu().numpy(), PC.pillow(f)), k


def _damaged():
    """the status-word refusals, three truncated streams and five mutated ones (the chunks whole: the damage reaches the kernels)"""
    out = [(label, data) for label, data, _ in PC.device_refusals()]
    small = PC.fuzz_files()["rgb_cycle.png"]
    cut = list(PC.stream_truncations(small))
    out += [(f"stream cut to {n} bytes", cut[n]) for n in (7, len(cut) // 2, len(cut) - 1)]
    out += [(f"mutation {k}", bad) for k, bad in enumerate(PC.stream_mutations(dict(PC.streams())["Pillow compress_level 6"], 5, 20261021))]
    return out


def test_damaged_streams_are_given_up_or_equal_pillow():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    for label, data in _damaged():
        (emu,) = ops.png_decode_host([data], guard=64)  # the emulation first, on the CPU: its guards hold
        assert emu is not None, label
        reasons = []
        (got,) = ops.png_decode_batch([data], device=DEV, reject_ok=True, reasons=reasons)
        assert (got is None) == (emu["status"] != 0), (label, reasons, hex(emu["status"]))
        if got is not None:
            assert np.array_equal(got.cpu().numpy(), PC.pillow(data)), label
        else:
            assert f"{emu['status']:#x}" in reasons[0], (label, reasons, hex(emu["status"]))
        # the C entry itself, guard bytes round the image, the status word and the workspace
        info = ops.png_parse(data)[0]
        h, w, c = info["height"], info["width"], info["channels"]
        img = torch.full((64 + h * w * c + 64,), CANARY, dtype=torch.uint8, device=DEV)
        batch = ops._png_batch([info], [c], [(img.data_ptr() + 64, w * c)], pin=False)
        need = lib.pgdvs_png_inflate_workspace_bytes(C.c_void_p(batch.data_ptr()), 1)
        wmem = torch.full((256 + need + 256,), CANARY, dtype=torch.uint8, device=DEV)
        status = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        off = (-wmem.data_ptr()) % 256
        dev = batch.to(DEV)
        _lib.check(lib.pgdvs_png_decode(C.c_void_p(batch.data_ptr()), C.c_void_p(dev.data_ptr()), batch.numel(), 1, 0, C.c_void_p(status.data_ptr() + 16),
                                        C.c_void_p(wmem.data_ptr() + off), need, ops._stream()), "pgdvs_png_decode")
        m, wm, st = img.cpu().numpy(), wmem.cpu().numpy(), status.cpu().numpy()
        assert (m[:64] == CANARY).all() and (m[64 + h * w * c:] == CANARY).all(), (label, "written outside the image")
        assert (wm[:off] == CANARY).all() and (wm[off + need:] == CANARY).all(), (label, "written outside the workspace")
        assert (np.delete(st, 4) == 0x5A5A5A5A).all() and int(st[4]) & 0xFFFFFFFF == emu["status"], (label, st, hex(emu["status"]))
        assert tuple(int(v) for v in wm[off:off + 16].view(np.uint32)) == emu["info"], (label, emu["info"])


# ---------------------------------------------------------------------------- the loaders
BIG = (701, 83)  # for the 288 x 36 frames


def _png(path, hw, rng, mode="RGB", **kw):
    base = PC.content("smooth", *hw, 3, int(rng.integers(1 << 30))).astype(np.int32) + rng.integers(-9, 10, (*hw, 3))
    PIL.Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).convert(mode).save(path, format="PNG", **kw)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the resident tests' trees, whose images are real PNG files already, with: half of the NVIDIA tree's frames at 701 x 83
    (the resize), every file's bytes also under its .jpg name (PNG bytes under .jpg names), frame 3's camera 3 interlaced,
    the target (2, 7) a palette file, (5, 5) a 16-bit RGB file, (6, 1) a JPEG under the .png name (RGBA files: the DyCheck tree below); the
    pure-geometry stack's frames 1 and 4 at other sizes and frame 2 interlaced; the monocular tree's frames behind frame 0
    larger, frame 2 a JPEG under its .png name and frame 5 interlaced"""
    t = RC.build_trees(tmp_path_factory.mktemp("png_gpu"))
    rng = np.random.default_rng(20261021)
    dense = pathlib.Path(t["nvidia"]) / "raw" / NT.SCENE / "dense"
    for f in range(NT.F):
        for c in range(NT.N_CAMS):
            png = dense / "mv_images" / f"{f:05d}" / f"cam{c + 1:02d}.png"
            hw = BIG if ((f + c) // 2) % 2 else (NT.H, NT.W)
            if (f, c) == (3, 3):
                png.write_bytes(_interlaced(hw))
            elif (f, c) == (2, 7):
                _png(png, (NT.H, NT.W), rng, mode="P")
            elif (f, c) == (5, 5):
                png.write_bytes(_sixteen_bits(hw))
            elif (f, c) == (6, 1):
                PIL.Image.fromarray(PC.content("smooth", *hw, 3, 6)).save(png, format="JPEG", quality=90)
            else:
                _png(png, hw, rng)
            png.with_suffix(".jpg").write_bytes(png.read_bytes())
    for f, hw in ((1, BIG), (4, (300, 40))):
        _png(dense / f"images_{NT.W}x{NT.H}" / f"{f:05d}.png", hw, rng)
    (dense / f"images_{NT.W}x{NT.H}" / "00002.png").write_bytes(_interlaced((NT.H, NT.W)))
    mono = pathlib.Path(t["mono"]) / NT.MONO_SCENE / "rgbs"
    for f in range(1, NT.MF):
        name = mono / f"{f:05d}.png"
        if f == 2:
            PIL.Image.fromarray(PC.content("smooth", 97, 131, 3, 2)).save(name, format="JPEG", quality=90)
        elif f == 5:
            name.write_bytes(_interlaced((97, 131)))
        else:
            _png(name, (97, 131) if f % 3 else (40, 57), rng)
    return t


def _interlaced(hw):
    """an Adam7 file: Pillow reads them and writes none, so the seven passes are filtered here (filter 0) by hand"""
    import zlib

    img = PC.content("smooth", *hw, 3, 33)
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            raw += b"".join(b"\0" + row.tobytes() for row in sub)
    return PC.SIGNATURE + PC.ihdr(*hw, 3, interlace=1) + PC.chunk(b"IDAT", zlib.compress(raw)) + PC.chunk(b"IEND")


def _sixteen_bits(hw):
    """a 16-bit RGB file (Pillow opens it as 8-bit RGB): filter-0 rows of big-endian samples"""
    import zlib

    img = PC.content("smooth", *hw, 3, 44).astype(">u2") * 257
    raw = b"".join(b"\0" + row.tobytes() for row in img)
    return PC.SIGNATURE + PC.ihdr(*hw, 3, depth=16) + PC.chunk(b"IDAT", zlib.compress(raw)) + PC.chunk(b"IEND")


def _logged(ds):
    """the loader with every ``decode_image`` path of its store recorded"""
    log, inner = [], ds.store.decode_image

    def decode_image(path, *a, **kw):
        log.append(pathlib.Path(path))
        return inner(path, *a, **kw)

    ds.store.decode_image = decode_image
    return log


def _expected_counts(log):
    from pgdvs_amd import ops

    served = unserved = 0
    for path in log:
        data = path.read_bytes()
        if data[:8] == PC.SIGNATURE:
            served, unserved = served + (ops.png_info(data) is not None), unserved + (ops.png_info(data) is None)
    return served, unserved


def _count_waits_per_fill(ds, monkeypatch):
    """[(missing frames of a fill, Event.synchronize calls inside it)]: counted as tests/test_gpu_resample.py's never-waits
    check intercepts them, by replacing the waiting call"""
    fills, inner_fill, inner_sync, state = [], ds.store._fill, torch.cuda.Event.synchronize, {"n": 0}

    def synchronize(self):
        state["n"] += 1
        return inner_sync(self)

    def fill(scene, frame_ids, decode, image_path=None):
        missing = [f for f in sorted(set(frame_ids)) if not scene.filled[f - scene.first_id]]
        before = state["n"]
        inner_fill(scene, frame_ids, decode, image_path)
        fills.append((len(missing), state["n"] - before))

    monkeypatch.setattr(torch.cuda.Event, "synchronize", synchronize)
    ds.store._fill = fill
    return fills


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_png_items_equal_the_device_resize_loaders(name, trees, monkeypatch):
    kw = dict(device=DEV, resident=True, device_resize=True)
    want, got = RC.make(name, trees, **kw), RC.make(name, trees, **kw, device_png=True)
    assert got.store.device_png and not want.store.device_png and not got.store.device_decode
    log = _logged(got)
    fills = _count_waits_per_fill(got, monkeypatch)
    if name == "nvidia_pure_geo":  # its stack was decoded while the loader was built: in one batch, counted then
        log_base = (got.store.stats["png_decoded_on_device"], got.store.stats["png_fallbacks"])
        assert log_base[0] > 1 and log_base[1] == 1, log_base  # (the interlaced frame 2)
    else:
        log_base = (0, 0)
    for i in range(len(want)):
        RC.assert_items_equal(got[i], want[i], (name, i))
    st, ref = got.store.stats, want.store.stats
    served, unserved = _expected_counts(log)
    assert st["png_decoded_on_device"] == served + log_base[0] > 0 and st["png_fallbacks"] == unserved + log_base[1], (st, served, unserved)
    assert ref["png_decoded_on_device"] == ref["png_fallbacks"] == 0
    for key in ("frames_decoded", "frames_resized_on_device", "targets_resized_on_device", "jpeg_fallbacks"):
        assert st[key] == ref[key], (key, st[key], ref[key])
    assert unserved > 0 or name == "nvidia_pure_geo"
    # one wait per item fill: the batch's; a fill with one missing frame waits for that file, one with none for nothing
    assert (fills or name == "nvidia_pure_geo") and all(waits <= 1 for _, waits in fills), fills
    assert any(missing > 1 and waits == 1 for missing, waits in fills) or name == "nvidia_pure_geo", fills
    assert all(waits == 0 for missing, waits in fills if missing == 0), fills


DYCHECK_KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DT.SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
                  flow_consist_thres=1.0, device=DEV, resident=True, device_resize=True)


def test_device_png_items_equal_the_device_resize_loader_dycheck(tmp_path_factory, monkeypatch):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    root = DT.build_tree(tmp_path_factory.mktemp("png_gpu_dycheck"))
    rng = np.random.default_rng(7)
    rgb = pathlib.Path(root) / "iphone" / DT.SCENE / f"rgb/{DT.FACTOR}x"
    for k, t in enumerate(DT.TRAIN_T[1:]):  # behind the first, which sets the scene's size: larger, every other one RGBA, one interlaced
        path = rgb / f"{DT.frame_name(0, t)}.png"
        if k == 2:
            path.write_bytes(_interlaced((117, 149)))
        else:
            _png(path, (117, 149), rng, mode="RGBA" if k % 2 else "RGB")
    want = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW)
    got = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW, device_png=True)
    log = _logged(got)
    fills = _count_waits_per_fill(got, monkeypatch)
    for i in range(len(want)):
        item, ref = got[i], want[i]
        assert list(item) == list(ref) and all(v.is_cuda for v in item.values() if isinstance(v, torch.Tensor))
        RC.assert_items_equal(item, ref, i)
    st = got.store.stats
    served, unserved = _expected_counts(log)
    assert st["png_decoded_on_device"] == served > 0 and st["png_fallbacks"] == unserved > 0, (st, served, unserved)
    assert st["targets_decoded_on_device"] == len(want) and st["frames_decoded"] == want.store.stats["frames_decoded"]
    assert all(waits <= 1 for _, waits in fills) and any(missing > 1 and waits == 1 for missing, waits in fills), fills
