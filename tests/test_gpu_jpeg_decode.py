"""The JPEG reader on the MI355X (csrc/jpeg_entropy.cpp + csrc/jpeg_decode.hip, ``ops.jpeg_decode``, the loaders'
``device_decode=True``): ``ops.jpeg_decode`` against ``np.array(PIL.Image.open(...))`` byte for byte over the whole stream
matrix of tests/jpeg_decode_cases.py; ``out=`` into a padded slot between guard words, and the C entry with rows a stride
apart at every alignment; the refusals; the five loaders with ``device_decode=True`` over trees of real JPEG files (all three
samplings, files larger than the frames, one progressive, one greyscale, PNG bytes under a .jpg name and JPEG bytes under a
.png name) against the same loaders with ``device_resize=True`` alone; and a ``device_decode`` item never waits for the
device, on the first use of its frames too."""
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
import jpeg_decode_cases as JC  # noqa: E402
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


# ---------------------------------------------------------------------------- ops.jpeg_decode
@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_jpeg_decode_equals_pillow(subsampling):
    from pgdvs_amd import ops

    streams = JC.matrix(subsampling)
    got = [ops.jpeg_decode(data) for _, data in streams]  # (all enqueued before the first is read back)
    for (label, data), g in zip(streams, got):
        want = JC.pillow(data)
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == want.shape and g.is_contiguous(), (label, g.shape, want.shape)
        bad = np.argwhere(g.cpu().numpy() != want)
        assert bad.size == 0, (label, len(bad), bad[:4].tolist())
    assert len(streams) == len(JC.SIZES) * 12 + 6 + (9 if subsampling != 1 else 0)


def test_out_into_a_padded_slot_between_guard_words():
    """a frame's slot of the resident store: padded to 16 bytes, its neighbours' bytes and its own padding stay"""
    from pgdvs_amd import ops

    for subsampling in JC.SUBSAMPLINGS:
        for h, w in ((5, 3), (17, 23), (33, 49)):
            data = JC.encode(JC.content("noise", h, w, 3), subsampling, 90)
            per = h * w * 3
            slot = -(-per // 16) * 16 + 16
            tab = torch.full((3, slot), CANARY, dtype=torch.uint8, device=DEV)
            out = tab[1, :per].view(h, w, 3)
            assert ops.jpeg_decode(data, out=out) is out
            got = tab.cpu().numpy()
            assert np.array_equal(got[1, :per].reshape(h, w, 3), JC.pillow(data)), (subsampling, h, w)
            assert (got[1, per:] == CANARY).all() and (got[[0, 2]] == CANARY).all(), (subsampling, h, w, "bytes outside the frame were written")
    for bad in (torch.zeros((17, 23, 3), dtype=torch.float32, device=DEV), torch.zeros((17, 24, 3), dtype=torch.uint8, device=DEV),
                torch.zeros((17, 23, 3), dtype=torch.uint8), torch.zeros((17, 23, 6), dtype=torch.uint8, device=DEV)[..., ::2]):
        with pytest.raises(ValueError, match="out"):
            ops.jpeg_decode(JC.encode(JC.content("noise", 17, 23), 2, 90), out=bad)


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_rows_a_stride_apart_at_every_alignment(subsampling):
    """``pgdvs_jpeg_reconstruct`` itself: rows row_stride bytes apart from a base at each of the four alignments (dword stores
    only where a row's address allows), the bytes between rows and around the image untouched"""
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    h, w = 19, 45
    data = JC.encode(JC.content("smooth", h, w, 5), subsampling, 95)
    want = JC.pillow(data)
    rc, info, msg = JC.parse(data)
    assert rc == 0, msg
    rc, coef, msg = JC.entropy_decode(data, info.coef_bytes)
    assert rc == 0, msg
    buf = torch.from_numpy(np.concatenate([coef, np.ctypeslib.as_array(info.quant).reshape(-1).view(np.int16)])).to(DEV)
    ws = torch.empty(lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)), dtype=torch.uint8, device=DEV)
    for base in range(4):
        for stride in (w * 3, w * 3 + 1, w * 3 + 6, w * 3 + 13):
            mem = torch.full((64 + base + h * stride + 64,), CANARY, dtype=torch.uint8, device=DEV)
            _lib.check(lib.pgdvs_jpeg_reconstruct(buf.data_ptr(), buf.data_ptr() + info.coef_bytes, C.byref(info), mem.data_ptr() + 64 + base,
                                                  stride, ws.data_ptr(), ws.numel(), ops._stream()), "pgdvs_jpeg_reconstruct")
            got = mem.cpu().numpy()
            rows = got[64 + base:64 + base + h * stride].reshape(h, stride)
            assert np.array_equal(rows[:, :w * 3].reshape(h, w, 3), want), (base, stride)
            assert (rows[:, w * 3:] == CANARY).all() and (got[:64 + base] == CANARY).all() and (got[64 + base + h * stride:] == CANARY).all(), (base, stride)
    # what the entry refuses, in front of any launch
    for args, word in (((buf.data_ptr() + 2, buf.data_ptr() + info.coef_bytes, w * 3, ws.numel()), "aligned"),
                       ((buf.data_ptr(), buf.data_ptr() + info.coef_bytes, w * 3 - 1, ws.numel()), "apart"),
                       ((buf.data_ptr(), buf.data_ptr() + info.coef_bytes, w * 3, ws.numel() - 1), "workspace"),
                       ((0, buf.data_ptr() + info.coef_bytes, w * 3, ws.numel()), "null")):
        mem = torch.full((h * w * 3,), CANARY, dtype=torch.uint8, device=DEV)
        assert lib.pgdvs_jpeg_reconstruct(args[0], args[1], C.byref(info), mem.data_ptr(), args[2], ws.data_ptr(), args[3], ops._stream()) == -1
        assert word in lib.pgdvs_last_error().decode() and (mem == CANARY).all(), word


def test_refusals_raise_or_return_none():
    from pgdvs_amd import ops

    for label, data in JC.refusals():
        if label == "4:1:1":  # Pillow's old name of 4:2:0 (tests/test_jpeg_decode_host.py): served
            assert np.array_equal(ops.jpeg_decode(data).cpu().numpy(), JC.pillow(data))
            continue
        assert ops.jpeg_decode(data, reject_ok=True) is None and ops.jpeg_decode(data, reject_ok=True, device=DEV) is None, label
        with pytest.raises(ValueError, match="not served: jpeg: "):
            ops.jpeg_decode(data)
    small = JC.small_stream()
    for n in range(0, len(small), 7):
        assert ops.jpeg_decode(small[:n], reject_ok=True) is None, n
    out = torch.full((24, 40, 3), CANARY, dtype=torch.uint8, device=DEV)  # a scan found corrupt on the host: nothing reaches the device
    assert ops.jpeg_decode(dict(JC.refusals())["flipped RSTn"], out=out, reject_ok=True) is None and (out == CANARY).all()


# ---------------------------------------------------------------------------- the loaders
BIG = (701, 83)  # for the 288 x 36 frames, as tests/test_gpu_resample.py
PROGRESSIVE, GREY, PNG_BYTES = (3, 3), (2, 7), ((5, 5), (6, 1))  # (time step, camera): a source frame; a target; a source frame and a target


def _jpeg(path, hw, rng, **kw):
    """a real JPEG of seeded smooth-plus-noise content at ``path`` (PIL opens by content, whatever the name)"""
    base = JC.content("smooth", *hw).astype(np.int32) + rng.integers(-20, 21, (*hw, 3))
    PIL.Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).convert(kw.pop("mode", "RGB")).save(path, format="JPEG", quality=90, **kw)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the resident tests' trees with real JPEG files.  NVIDIA tree: every mv_images file under its .jpg name alone (the .png
    twins leave, so both evaluation loaders read the .jpg files), sampling (f + c) % 3, every second source frame and half of
    the other cameras at 701 x 83; source frame 3 progressive, the target (2, 7) greyscale, and (5, 5), (6, 1) keep PNG bytes
    under the .jpg name.  Monocular tree: the frames behind frame 0 as JPEG bytes under their .png names, two of three larger;
    frame 0, which sets the size, JPEG too; frame 2 stays a PNG."""
    t = RC.build_trees(tmp_path_factory.mktemp("jpeg_gpu"))
    rng = np.random.default_rng(20261020)
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
                _jpeg(jpg, hw, rng, subsampling=(f + c) % 3)
    mono = pathlib.Path(t["mono"]) / NT.MONO_SCENE / "rgbs"
    names = sorted(mono.iterdir())
    h, w = PIL.Image.open(names[0]).size[::-1]
    for f, name in enumerate(names):
        if f != 2:
            _jpeg(name, (h, w) if f % 3 == 0 else (97, 131), rng, subsampling=f % 3)
    return t


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_decode_items_equal_the_device_resize_loaders(name, trees):
    want = RC.make(name, trees, device=DEV, resident=True, device_resize=True)
    got = RC.make(name, trees, device=DEV, resident=True, device_resize=True, device_decode=True)
    assert got.store.device_decode and not want.store.device_decode
    for i in range(len(want)):
        item = got[i]
        assert all(v.is_cuda for v in item.values() if isinstance(v, torch.Tensor)), [k for k, v in item.items()
                                                                                      if isinstance(v, torch.Tensor) and not v.is_cuda]
        RC.assert_items_equal(item, want[i], (name, i))
    st, ref = got.store.stats, want.store.stats
    n_frames = NT.MF if name == "mono_vis" else NT.F
    assert st["frames_decoded"] == ref["frames_decoded"] == n_frames
    assert ref["frames_decoded_on_device"] == ref["targets_decoded_on_device"] == ref["jpeg_fallbacks"] == 0
    if name == "mono_vis":  # every frame but the PNG one; no JPEG is left to Pillow
        assert (st["frames_decoded_on_device"], st["jpeg_fallbacks"], st["targets_decoded_on_device"]) == (NT.MF - 1, 0, 0)
        assert st["frames_resized_on_device"] == ref["frames_resized_on_device"] == len([f for f in range(NT.MF) if f % 3 and f != 2])
        return
    assert st["frames_decoded_on_device"] == NT.F - 2 > 0  # all but the progressive frame and the PNG bytes of frame 5
    assert st["frames_resized_on_device"] == ref["frames_resized_on_device"] > 0
    if name == "nvidia_vis":  # source frames alone: the progressive one
        assert (st["jpeg_fallbacks"], st["targets_decoded_on_device"]) == (1, 0)
    else:  # every file is some item's target: the progressive file once more, the greyscale one, and not the two PNGs
        assert st["jpeg_fallbacks"] == 3 and st["targets_decoded_on_device"] == len(want) - 4 > 0
        assert st["targets_resized_on_device"] == ref["targets_resized_on_device"] > 0


DYCHECK_KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DT.SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
                  flow_consist_thres=1.0, device=DEV, resident=True, device_resize=True)


def test_device_decode_falls_back_entirely_for_dycheck(tmp_path):
    """the dataset's images are PNG: the keyword is taken, Pillow reads every file, the items are the same"""
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    root = DT.build_tree(tmp_path)
    want = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW)
    got = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW, device_decode=True)
    assert got.store.device_decode
    for i in range(0, len(want), 3):
        RC.assert_items_equal(got[i], want[i], i)
    st = got.store.stats
    assert st["frames_decoded"] > 0 and st["frames_decoded_on_device"] == st["targets_decoded_on_device"] == st["jpeg_fallbacks"] == 0


def _refuse(*a, **kw):
    raise AssertionError("a device_decode __getitem__ waited for the device")


WAITS = ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
         (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"))


@pytest.mark.parametrize("name", ["nvidia_vis", "mono_vis", "nvidia_eval"])
def test_a_device_decode_item_never_waits_for_the_device(name, trees, monkeypatch):
    """tests/test_gpu_resample.py's check for this path, from the FIRST use of every frame on: the waiting calls raise while the
    items are built, the loader's frames and targets are decoded under them, and the items equal the device_resize loader's"""
    make = lambda **kw: RC.make(name, trees, device=DEV, resident=True, device_resize=True, **kw)  # noqa: E731
    want, res = make(), make(device_decode=True)
    idx = range(0, len(res), 5 if name != "nvidia_eval" else 23)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        for owner, attr in WAITS:
            m.setattr(owner, attr, _refuse)
        first = [res[i] for i in idx]
        assert res.store.stats["frames_decoded_on_device"] > 0
        second = [res[i] for i in idx]
    if name == "nvidia_eval":
        assert res.store.stats["targets_decoded_on_device"] > 0
    for i, a, b in zip(idx, first, second):
        RC.assert_items_equal(a, want[i], (name, i, "first use"))
        RC.assert_items_equal(b, a, (name, i, "second use"))
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()) if isinstance(x, torch.Tensor))
