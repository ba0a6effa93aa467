"""The image-input options and the store's decode dispatch without a GPU (``datasets._common.device_input``,
``datasets.resident.SceneStore``): the truth table of the four options' rules, through the one function and through the
store's constructor, against this file's own statement of them in precedence order; and ``decode_image``,
``prefetch_images``, ``decode_stack`` and ``_fill`` with the three decode ops replaced by recorders -- which op is asked, in
which order and with which arguments (the ``kinds`` of a PNG call among them), what a give-up ends in, the complete ``stats`` after every call, that a prefetched file
is neither read nor walked again, and that the prefetch table is left empty."""
import builtins
import io
import itertools
import types

import numpy as np
import PIL.Image
import pytest
import torch

FLAGS = ("resize", "decode", "entropy", "png")
PNG_WALK = "png_parse"  # the public chunk walk of ops
MARK = 7  # what a recorder's image is filled with: not Pillow's


# ---------------------------------------------------------------------------- the option rules
def missing(resize, decode, entropy, png, resident, device):
    """what the first broken rule asks for, or None: the rules in their order of precedence"""
    rules = ((entropy and not decode, "device_decode=True"),
             (png and not resize, "device_resize=True"),
             (decode and not resize, "device_resize=True"),
             (resize and not resident, "resident=True"),
             (resize and (device is None or torch.device(device).type != "cuda"), "GPU"))
    return next((what for broken, what in rules if broken), None)


TABLE = [(flags, resident, device) for flags in itertools.product((False, True), repeat=4) for resident in (False, True)
         for device in (None, "cpu", "cuda:0")]


def test_the_truth_table_through_the_one_function():
    from pgdvs_amd.datasets._common import device_input

    for flags, resident, device in TABLE:
        kw = dict(resident=resident, device=device, **{f"device_{n}": v for n, v in zip(FLAGS, flags)})
        want = missing(*flags, resident, device)
        if want is None:
            got = device_input("Loader", **kw)
            assert (got.resize, got.decode, got.entropy, got.png) == flags, (flags, resident, device)
            assert all(type(getattr(got, n)) is bool for n in FLAGS)
        else:
            with pytest.raises(ValueError, match=want) as err:
                device_input("Loader", **kw)
            assert str(err.value).startswith("Loader(device_"), (flags, resident, device, str(err.value))
    got = device_input("Loader", resident=True, device="cuda", device_resize=1, device_decode=0, device_entropy=0, device_png=1)
    assert (got.resize, got.decode, got.entropy, got.png) == (True, False, False, True)  # (truthy values come back as booleans)
    with pytest.raises((AttributeError, TypeError)):
        got.png = False  # immutable


def test_the_truth_table_through_the_store():
    from pgdvs_amd.datasets.resident import SceneStore

    for flags, device in ((flags, device) for flags, resident, device in TABLE if resident):  # (a store is resident)
        kw ={f"device_{n}": v for n, v in zip(FLAGS, flags)}
        want = "GPU" if device == "cpu" else missing(*flags, True, device)  # (a store lives in host memory or on a GPU)
        if want is None:
            store = SceneStore(device, **kw)
            assert (store.device_resize, store.device_decode, store.device_entropy, store.device_png) == flags, (flags, device)
            assert not store.scenes and store.nbytes == 0  # nothing is allocated until scene() is called
        else:
            with pytest.raises(ValueError, match=want):
                SceneStore(device, **kw)


# ---------------------------------------------------------------------------- the dispatch
OPTION_SETS = {"resize": (True, False, False, False), "decode": (True, True, False, False), "entropy": (True, True, True, False),
               "png": (True, False, False, True), "all": (True, True, True, True)}
KINDS = ("rgb_png", "rgba_png", "png16", "jpeg", "progressive", "noise")
CHANNELS = {"rgba_png": "rgb"}  # (every other file is read with channels="file")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """kind -> path of a 16 x 16 file written by Pillow (noise: 32 random bytes)"""
    d = tmp_path_factory.mktemp("dispatch")
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    paths = {k: str(d / f"{k}.{'jpg' if k in ('jpeg', 'progressive') else 'png'}") for k in KINDS}
    PIL.Image.fromarray(rgb).save(paths["rgb_png"])
    PIL.Image.fromarray(np.dstack([rgb, rng.integers(0, 256, (16, 16, 1), dtype=np.uint8)])).save(paths["rgba_png"])
    PIL.Image.fromarray(rng.integers(0, 65536, (16, 16), dtype=np.uint16)).save(paths["png16"])
    PIL.Image.fromarray(rgb).save(paths["jpeg"], quality=90, subsampling="4:2:0")
    PIL.Image.fromarray(rgb).save(paths["progressive"], quality=90, subsampling="4:2:0", progressive=True)
    noise = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    assert noise[:2] != b"\xff\xd8" and noise[:4] != b"\x89PNG"
    with open(paths["noise"], "wb") as f:
        f.write(noise)
    return paths


def pillow(path, channels="file"):
    image = np.array(PIL.Image.open(path))
    return image[..., :3] if channels == "rgb" else image


class Recorders:
    """``ops.png_decode_batch``, ``ops.jpeg_decode`` and ``ops.jpeg_decode_device`` replaced: every call is written down and
    answered with an image of the file's size filled with MARK, or with a give-up (``serve`` False; ``scan`` False: the
    device's scan alone gave up and the host path served the file)"""

    def __init__(self, monkeypatch, serve=True, scan=True):
        from pgdvs_amd import ops

        self.calls, self.walks, self.walk_kinds, self.serve, self.scan = [], 0, [], serve, scan
        walk = getattr(ops, PNG_WALK)

        def counted_walk(data, kinds=("colour",)):
            self.walks += 1
            self.walk_kinds.append(tuple(kinds))
            return walk(data, kinds)

        monkeypatch.setattr(ops, PNG_WALK, counted_walk)
        monkeypatch.setattr(ops, "png_decode_batch", self.png_decode_batch)
        monkeypatch.setattr(ops, "jpeg_decode", self.jpeg_decode)
        monkeypatch.setattr(ops, "jpeg_decode_device", self.jpeg_decode_device)

    def image(self, data, channels="file"):
        if not self.serve:
            return None
        im = PIL.Image.open(io.BytesIO(bytes(data)))
        bands = len(im.getbands())  # (one band: a mask file, [H,W])
        return torch.full((im.size[1], im.size[0]) + ((3 if channels == "rgb" else bands,) if bands > 1 else ()), MARK, dtype=torch.uint8)

    def png_decode_batch(self, datas, outs=None, channels="file", device=None, reject_ok=False, sub_bytes=0, reasons=None, stats=None, parsed=None,
                         kinds=("colour",)):
        self.calls.append(("png", len(datas), channels, str(device), reject_ok, list(outs), parsed is not None and len(parsed) == len(datas), tuple(kinds)))
        return [self.image(d, channels) for d in datas]

    def jpeg_decode(self, data, out=None, device=None, reject_ok=False, entropy="host"):
        self.calls.append(("jpeg_host", str(device), reject_ok, out, entropy))
        return self.image(data)

    def jpeg_decode_device(self, data, out=None, device=None, reject_ok=False):
        self.calls.append(("jpeg_device", str(device), reject_ok, out))
        return self.image(data), self.serve and self.scan

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def expected(options, kind, target, serve, scan):
    """(the recorders' calls, the counters that go up by one, whether a recorder's image is the answer) of one
    ``decode_image(path, target=target, into=None)``"""
    _, decode, entropy, png = options
    calls, up, served = [], [], False
    if png and kind in ("rgb_png", "rgba_png", "png16"):
        if kind != "png16":  # (the host side refuses 16 bits: no launch)
            calls.append(("png", 1, CHANNELS.get(kind, "file"), "cuda:0", True, [None], True, ("colour",)))
            served = serve
        up.append("png_decoded_on_device" if served else "png_fallbacks")
    if not served and decode and kind in ("jpeg", "progressive"):
        if kind == "jpeg":  # (the host side refuses a progressive file: no launch)
            calls.append(("jpeg_device", "cuda:0", True, None) if entropy else ("jpeg_host", "cuda:0", True, None, "host"))
            if entropy:
                up.append("scans_decoded_on_device" if serve and scan else "entropy_fallbacks")
            served = serve
        if not served:
            up.append("jpeg_fallbacks")
    if served:
        up.append("targets_decoded_on_device" if target else "frames_decoded_on_device")
    return calls, up, served


@pytest.mark.parametrize("serve,scan", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_decode_image_asks_the_codecs_in_order_and_counts(files, monkeypatch, name, serve, scan):
    from pgdvs_amd.datasets.resident import SceneStore

    options = OPTION_SETS[name]
    rec = Recorders(monkeypatch, serve, scan)
    store = SceneStore("cuda:0", **{f"device_{n}": v for n, v in zip(FLAGS, options)})
    stats = dict.fromkeys(store.stats, 0)
    assert store.stats == stats and len(stats) == 13
    for kind, target in itertools.product(KINDS, (False, True)):
        channels = CHANNELS.get(kind, "file")
        calls, up, served = expected(options, kind, target, serve, scan)
        for key in up:
            stats[key] += 1
        if kind == "noise":
            with pytest.raises(PIL.UnidentifiedImageError):
                store.decode_image(files[kind], target=target, channels=channels)
        else:
            got = store.decode_image(files[kind], target=target, channels=channels)
            want = pillow(files[kind], channels)
            if served:
                assert isinstance(got, torch.Tensor) and tuple(got.shape) == want.shape and bool((got == MARK).all()), (name, kind)
            else:  # Pillow's array, whoever gave up
                assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), (name, kind)
        assert rec.take() == calls, (name, kind, target)
        assert store.stats == stats, (name, kind, target)


def count_opens(monkeypatch):
    opens, real = [], builtins.open

    def counting(file, *a, **k):
        opens.append(str(file))
        return real(file, *a, **k)

    monkeypatch.setattr(builtins, "open", counting)
    return opens


@pytest.mark.parametrize("name", ["png", "all"])
def test_a_prefetched_file_is_neither_read_nor_walked_again(files, monkeypatch, name):
    from pgdvs_amd.datasets.resident import SceneStore

    options = OPTION_SETS[name]
    rec = Recorders(monkeypatch)
    store = SceneStore("cuda:0", **{f"device_{n}": v for n, v in zip(FLAGS, options)})
    kinds = ("rgb_png", "rgba_png", "png16", "jpeg")
    paths = [(files[k], CHANNELS[k]) if k in CHANNELS else files[k] for k in kinds]
    opens = count_opens(monkeypatch)
    store.prefetch_images(paths)
    store.prefetch_images(paths[:2])  # (what is there already is not read again)
    assert sorted(opens) == sorted(files[k] for k in kinds) and rec.walks == 3  # every file read once, every PNG walked once
    assert rec.take() == [("png", 1, "file", "cuda:0", True, [None], True, ("colour",)),
                          ("png", 1, "rgb", "cuda:0", True, [None], True, ("colour",))]  # a launch per mode, image-only: the default kinds
    assert rec.walk_kinds == [("colour",)] * 3
    assert store.stats == dict.fromkeys(store.stats, 0)  # (counted when the image is handed out)
    stats = dict.fromkeys(store.stats, 0)
    for kind in kinds:
        del opens[:]
        got = store.decode_image(files[kind], channels=CHANNELS.get(kind, "file"))
        _, up, served = expected(options, kind, False, True, True)
        for key in up:
            stats[key] += 1
        assert served == isinstance(got, torch.Tensor) and store.stats == stats, kind
        # the store opens nothing; a file that falls back is opened by Pillow's statement, once
        assert opens == ([] if served else [files[kind]]) and rec.walks == 3, (kind, opens)
    assert rec.take() == ([("jpeg_device", "cuda:0", True, None)] if options[1] else [])  # (the JPEG's bytes came from the table too)
    assert not store._prefetched
    del opens[:]
    store.decode_image(files["rgb_png"])  # use once: the second call reads, walks and launches again
    assert opens == [files["rgb_png"]] and rec.walks == 4 and len(rec.take()) == 1


def test_fill_and_decode_stack_leave_the_prefetch_table_empty(files, monkeypatch):
    from pgdvs_amd.datasets.resident import SceneStore

    rec = Recorders(monkeypatch)
    store = SceneStore("cuda:0", device_resize=True, device_png=True)
    got = store.decode_stack([files["rgb_png"], files["png16"], files["jpeg"]])
    assert [type(g) for g in got] == [np.ndarray] * 3 and bool((got[0] == MARK).all()) and np.array_equal(got[2], pillow(files["jpeg"]))
    assert not store._prefetched and [c[:3] for c in rec.take()] == [("png", 1, "file")]
    with pytest.raises(PIL.UnidentifiedImageError):
        store.decode_stack([files["rgb_png"], files["noise"], files["rgba_png"]])
    assert not store._prefetched and [c[:3] for c in rec.take()] == [("png", 2, "file")]

    scene = types.SimpleNamespace(filled=np.zeros(3, dtype=bool), first_id=0, n_frames=3, h=8, w=8)  # (no slot of the files' size: no table is touched)
    frames = {0: files["rgb_png"], 1: files["png16"], 2: files["rgba_png"]}
    put = []
    monkeypatch.setattr(store, "put", lambda scene, f, *frame: put.append(f))
    opens = count_opens(monkeypatch)
    store._fill(scene, [2, 0, 1, 0], lambda f: (store.decode_image(frames[f], into=(scene, f)), None, None), frames.get)
    assert put == [0, 1, 2] and not store._prefetched and [c[:3] for c in rec.take()] == [("png", 2, "file")]
    assert sorted(opens) == sorted([*frames.values(), frames[1]])  # each once, and Pillow's statement for the one that fell back

    def reader(f):
        raise OSError(f"frame {f} has no depth file")

    with pytest.raises(OSError, match="frame 0"):
        store._fill(scene, [0, 1, 2], reader, frames.get)
    assert not store._prefetched and [c[:3] for c in rec.take()] == [("png", 2, "file")]  # (prefetched, then dropped)


def test_masks_ride_with_the_first_mode_and_the_batch_carries_both_kinds(files, monkeypatch, tmp_path):
    from pgdvs_amd.datasets.resident import SceneStore

    rec = Recorders(monkeypatch)
    masks = [str(tmp_path / f"mask{k}.png") for k in range(2)]
    for k, path in enumerate(masks):
        PIL.Image.fromarray(np.random.default_rng(k).integers(0, 2, (16, 16)).astype(bool)).save(path)
    paths = [files["rgb_png"], (files["rgba_png"], "rgb"), files["png16"], files["jpeg"]]
    store = SceneStore("cuda:0", device_resize=True, device_png=True, device_mask=True)
    assert len(store.stats) == 15
    opens = count_opens(monkeypatch)
    store.prefetch_images(paths, masks=[(m, None, None) for m in masks])
    assert sorted(opens) == sorted([files["rgb_png"], files["rgba_png"], files["png16"], files["jpeg"], *masks]) and rec.walks == 5
    assert rec.walk_kinds == [("colour",)] * 3 + [("mask",)] * 2
    # a launch per mode: the masks in the first one's batch, behind its images, which alone carries both kinds
    assert rec.take() == [("png", 3, "file", "cuda:0", True, [None] * 3, True, ("colour", "mask")), ("png", 1, "rgb", "cuda:0", True, [None], True, ("colour",))]
    assert store.stats == dict.fromkeys(store.stats, 0)  # (counted when the image or mask is handed out)
    del opens[:]
    for k, path in enumerate(masks):
        got = store.decode_mask(path)
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (16, 16) and store.stats["masks_decoded_on_device"] == k + 1
    assert isinstance(store.decode_image(files["rgb_png"]), torch.Tensor) and store.stats["png_decoded_on_device"] == 1
    assert opens == [] and rec.walks == 5 and rec.take() == []  # nothing is read, walked or launched again
    store._prefetched.clear()

    alone = SceneStore("cuda:0", device_resize=True, device_mask=True)  # without device_png: the images stay out, the masks are a batch of their own
    alone.prefetch_images(paths, masks=[(m, None, None) for m in masks])
    assert sorted(opens) == sorted(masks) and rec.take() == [("png", 2, "file", "cuda:0", True, [None] * 2, True, ("colour", "mask"))]
    assert sorted(alone._prefetched) == sorted((m, "mask") for m in masks)
    del opens[:]
    got = alone.decode_mask(masks[0])  # handed out: counted, not read again
    assert isinstance(got, torch.Tensor) and opens == [] and alone.stats["masks_decoded_on_device"] == 1 and alone.stats["mask_fallbacks"] == 0
    got = alone.decode_mask(files["png16"])  # not prefetched: read, walked, refused by the host side (16 bits), Pillow's statement
    assert isinstance(got, np.ndarray) and opens == [files["png16"]] * 2 and alone.stats["mask_fallbacks"] == 1 and rec.take() == []
