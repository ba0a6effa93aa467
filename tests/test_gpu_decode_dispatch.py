"""The store's decode dispatch on the MI355X with the real ops (``SceneStore.decode_image`` and ``prefetch_images`` with all
four image-input options): slot-sized PNG and JPEG files are decoded straight into their slots, the others into fresh
tensors, all byte for byte Pillow's, the same with and without a prefetch; and the side-stream launch of ``ops.png_decode``
and ``ops.jpeg_decode(..., entropy="device")`` against work on the caller's stream in front of and behind the call, with the
stream operations each call issues, in their order."""
import numpy as np
import PIL.Image
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


def _content(h, w, c, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(37 * xx + 11 * yy + 60 * k + seed) % 256 for k in range(c)], -1)
    return (img ^ np.random.default_rng(seed).integers(0, 8, img.shape)).astype(np.uint8)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(path, channels, whether it has the slot's size, Pillow's array) of the four files; the scene's frames are 16 x 16"""
    d = tmp_path_factory.mktemp("dispatch")
    out = []
    for name, (h, w, c), channels, kw in (("a.png", (16, 16, 3), "file", {}),
                                          ("b.jpg", (16, 16, 3), "file", dict(quality=90, subsampling="4:2:0")),  # one MCU
                                          ("c.png", (9, 17, 4), "rgb", {}),  # not the slot's size; an odd last row
                                          ("d.jpg", (16, 24, 3), "file", dict(quality=90, subsampling="4:2:2"))):
        path = str(d / name)
        PIL.Image.fromarray(_content(h, w, c, len(out))).save(path, **kw)
        want = np.array(PIL.Image.open(path))
        out.append((path, channels, (h, w) == (16, 16), want[..., :3] if channels == "rgb" else want))
    return out


def _decode_all(files, prefetch):
    from pgdvs_amd.datasets.resident import SceneStore

    store = SceneStore(DEV, device_resize=True, device_decode=True, device_entropy=True, device_png=True)
    scene = store.scene("scene", 3, (16, 16))
    intos = [(scene, f) for f in (0, 1, 2, 2)]  # (the two files of another size never reach a slot)
    if prefetch:
        store.prefetch_images([(path, channels) for path, channels, _, _ in files], intos)
    images = [store.decode_image(path, into=into, channels=channels) for (path, channels, _, _), into in zip(files, intos)]
    torch.cuda.synchronize()
    return store, scene, images


def test_slot_sized_files_land_in_their_slots_and_all_equal_pillow(files):
    plain, with_prefetch = _decode_all(files, False), _decode_all(files, True)
    for store, scene, images in (plain, with_prefetch):
        for f, (image, (path, _, slot_sized, want)) in enumerate(zip(images, files)):
            assert isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8, path
            if slot_sized:
                assert image.data_ptr() == scene.rgb[f].data_ptr(), path
            else:
                assert all(image.data_ptr() != scene.rgb[s].data_ptr() for s in range(3)), path
                lo, hi = scene.rgb.data_ptr(), scene.rgb.data_ptr() + scene.rgb.stride(0) * 3
                assert not lo <= image.data_ptr() < hi, path  # a fresh tensor
            assert tuple(image.shape) == want.shape and np.array_equal(image.cpu().numpy(), want), path
        assert not store._prefetched
    assert plain[0].stats == with_prefetch[0].stats
    want = dict.fromkeys(plain[0].stats, 0)
    want.update(png_decoded_on_device=2, scans_decoded_on_device=2, frames_decoded_on_device=4)
    assert plain[0].stats == want


def _record_stream_operations(monkeypatch, main):
    """every stream operation and library launch of the decode ops from here on, as text, in order"""
    from pgdvs_amd import _lib

    log, lib, depth = [], _lib.load(), [0]
    name = lambda s: "main" if s == main else "side"  # noqa: E731

    def wrap(owner, attr, text):
        real = getattr(owner, attr)

        def wrapped(*a, **k):
            if not depth[0]:  # (torch's wait_stream is an event of its own, recorded and waited for: one operation here)
                log.append(text(*a, **k))
            depth[0] += 1
            try:
                return real(*a, **k)
            finally:
                depth[0] -= 1

        monkeypatch.setattr(owner, attr, wrapped)

    wrap(torch.cuda.Stream, "wait_stream", lambda self, other: f"{name(self)} waits for {name(other)}")
    wrap(torch.cuda.Event, "record", lambda self, stream=None: f"event recorded on {name(stream if stream is not None else torch.cuda.current_stream())}")
    wrap(torch.cuda.Event, "synchronize", lambda self: "host waits for the event")
    wrap(torch.cuda.Event, "wait", lambda self, stream=None: "a stream waits for the event")
    wrap(torch.cuda.Stream, "synchronize", lambda self: f"host waits for {name(self)}")
    wrap(torch.Tensor, "record_stream", lambda self, stream: f"record_stream({name(stream)})")
    wrap(torch.cuda, "synchronize", lambda *a: "host waits for the device")
    for fn in ("pgdvs_png_decode", "pgdvs_jpeg_scan_decode", "pgdvs_jpeg_reconstruct"):
        wrap(lib, fn, lambda *a, fn=fn: f"{fn} on {name(torch.cuda.current_stream())}")
    return log


def test_the_side_stream_is_ordered_against_the_callers_stream(tmp_path, monkeypatch):
    from pgdvs_amd import ops

    img = _content(48, 64, 3, 9)
    PIL.Image.fromarray(img).save(tmp_path / "x.png")
    PIL.Image.fromarray(img).save(tmp_path / "x.jpg", quality=90, subsampling="4:2:0")
    png, jpg = (tmp_path / "x.png").read_bytes(), (tmp_path / "x.jpg").read_bytes()
    want_png, want_jpg = np.array(PIL.Image.open(tmp_path / "x.png")), np.array(PIL.Image.open(tmp_path / "x.jpg"))
    ops.png_decode(png, device=DEV), ops.jpeg_decode(jpg, device=DEV, entropy="device")  # (warm-up: code objects, the side streams)
    torch.cuda.synchronize()
    dst_png, dst_jpg = (torch.empty((48, 64, 3), dtype=torch.uint8, device=DEV) for _ in range(2))
    log = _record_stream_operations(monkeypatch, torch.cuda.current_stream())

    dst_png.fill_(0x5A)
    assert ops.png_decode(png, out=dst_png) is dst_png
    dst_png.add_(1)
    png_log = log[:]
    del log[:]
    dst_jpg.fill_(0x5A)
    assert ops.jpeg_decode(jpg, out=dst_jpg, entropy="device") is dst_jpg
    dst_jpg.add_(1)
    jpg_log = log[:]
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert np.array_equal(dst_png.cpu().numpy(), want_png + np.uint8(1))  # (uint8: modulo 256)
    assert np.array_equal(dst_jpg.cpu().numpy(), want_jpg + np.uint8(1))
    assert png_log == ["side waits for main", "pgdvs_png_decode on side", "event recorded on side", "main waits for side", "record_stream(side)",
                       "host waits for the event"]
    assert jpg_log == ["side waits for main", "pgdvs_jpeg_scan_decode on side", "event recorded on side", "pgdvs_jpeg_reconstruct on side",
                       "main waits for side", "host waits for the event"]
