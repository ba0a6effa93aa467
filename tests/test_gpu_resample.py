"""The device resize on the MI355X (csrc/resample.hip, ``ops.resample_u8``, the loaders' ``device_resize=True``):
``ops.resample_u8`` against ``PIL.Image.resize`` byte for byte, both filters, one and three channels, one and three frames,
over shapes that take every path of the two passes and contents that reach the clamp; ``out=`` into a padded slot leaves the
padding alone; the refusals; the five loaders with ``device_resize=True`` over trees whose image files need the resize
against the same loaders with ``resident=True``; and a ``device_resize`` item never waits for the device, on the first use
of its frames too."""
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import resample_cases as RS  # noqa: E402
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


# ---------------------------------------------------------------------------- ops.resample_u8
def _frames(kind, n, in_hw, c):
    return np.stack([RS.content(kind, *in_hw, c, seed=7 * i) for i in range(n)])


@pytest.mark.parametrize("filter", sorted(RS.FILTERS))
@pytest.mark.parametrize("in_hw,out_hw", RS.SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in RS.SHAPES])
def test_resample_u8_equals_pillow(in_hw, out_hw, filter):
    from pgdvs_amd import ops

    for c in (1, 3):
        for kind in RS.CONTENTS:
            host = _frames(kind, 3, in_hw, c)  # [3,H,W] or [3,H,W,3]
            want = np.stack([RS.pil_resize(f, out_hw, filter) for f in host])
            dev = torch.from_numpy(host).to(DEV)
            # one frame in the layout it has on the host: [H,W] or [H,W,3]
            got = ops.resample_u8(dev[0], out_hw, filter)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want[0].shape
            bad = np.argwhere(got.cpu().numpy() != want[0])
            assert bad.size == 0, (c, kind, "one frame", len(bad), bad[:4].tolist())
            # three frames [N,H,W,C]
            got = ops.resample_u8(dev.reshape(3, *in_hw, c), out_hw, filter)
            assert tuple(got.shape) == (3, *out_hw, c)
            bad = np.argwhere(got.cpu().numpy() != want.reshape(3, *out_hw, c))
            assert bad.size == 0, (c, kind, "three frames", len(bad), bad[:4].tolist())


# paths of the two kernels that the shapes above do not take
OTHER_PATHS = [
    ((37, 53), (9, 53), "box"),  # vertical pass alone over rows of 53 and 159 bytes: one byte per lane
    ((37, 53), (9, 53), "lanczos"),
    ((1, 5120), (1, 21), "box"),  # 245 taps: the LDS stage holds the span of 20 output pixels, two tiles
    ((2, 4200), (1, 100), "lanczos"),  # 253 taps a pixel: tiles of 124 output pixels
    ((2, 700), (2, 600), "box"),  # three tiles of 256 output pixels, a ratio just above 1
]


@pytest.mark.parametrize("in_hw,out_hw,filter", OTHER_PATHS, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}-{f}" for a, b, f in OTHER_PATHS])
def test_long_filters_narrow_tiles_and_unaligned_rows_equal_pillow(in_hw, out_hw, filter):
    from pgdvs_amd import ops

    for c in (1, 3):
        for kind in ("random", "checker"):
            host = RS.content(kind, *in_hw, c)
            got, want = ops.resample_u8(torch.from_numpy(host).to(DEV), out_hw, filter).cpu().numpy(), RS.pil_resize(host, out_hw, filter)
            bad = np.argwhere(got != want)
            assert got.shape == want.shape and bad.size == 0, (c, kind, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("in_hw,out_hw", [((7, 5), (3, 2)), ((37, 53), (9, 13)), ((64, 64), (64, 17)), ((64, 64), (17, 64)), ((5, 7), (5, 7))])
def test_out_into_padded_slots_and_strided_frames(in_hw, out_hw):
    """frames and results in slots padded to 16 bytes, as the resident store keeps them: the bytes between frames stay"""
    from pgdvs_amd import ops

    def table(n, hw, fill):
        per = hw[0] * hw[1] * 3
        slot = -(-per // 16) * 16 + 16  # (a whole spare line, so that every case has padding)
        tab = torch.full((n, slot), fill, dtype=torch.uint8, device=DEV)
        return tab, tab[:, :per].view(n, *hw, 3)

    host = _frames("random", 3, in_hw, 3)
    _, src = table(3, in_hw, 0)
    src.copy_(torch.from_numpy(host))
    for filter in sorted(RS.FILTERS):
        want = np.stack([RS.pil_resize(f, out_hw, filter) for f in host])
        tab, out = table(3, out_hw, CANARY)
        assert ops.resample_u8(src, out_hw, filter, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), filter
        per = out_hw[0] * out_hw[1] * 3
        assert (tab[:, per:] == CANARY).all(), (filter, "the padding was written")
        tab, out = table(3, out_hw, CANARY)  # one frame into the middle slot
        ops.resample_u8(src[2], out_hw, filter, out=out[1])
        got = tab.cpu().numpy()
        assert np.array_equal(got[1, :per].reshape(*out_hw, 3), want[2]) and (got[1, per:] == CANARY).all() and (got[[0, 2]] == CANARY).all()


def test_resample_refusals():
    from pgdvs_amd import ops

    img = torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV)
    for bad in (img.float(), img.cpu(), img[..., :2], torch.zeros((8, 8, 4), dtype=torch.uint8, device=DEV), img[0, 0],
                torch.zeros((1, 1, 8, 8, 3), dtype=torch.uint8, device=DEV), img.cpu().numpy()):
        with pytest.raises(ValueError):
            ops.resample_u8(bad, (4, 4), "box")
    with pytest.raises(ValueError):
        ops.resample_u8(img, (4, 4), "nearest")
    for out in (torch.zeros((4, 4, 3), dtype=torch.float32, device=DEV), torch.zeros((4, 5, 3), dtype=torch.uint8, device=DEV),
                torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 4, 6), dtype=torch.uint8, device=DEV)[..., ::2]):
        with pytest.raises(ValueError):
            ops.resample_u8(img, (4, 4), "box", out=out)
    # sizes the table entry refuses: more than 256 taps, an empty output, an axis past 16384
    wide = torch.zeros((1, 5120, 3), dtype=torch.uint8, device=DEV)
    for hw, filter in (((1, 20), "box"), ((1, 100), "lanczos"), ((0, 4), "box"), ((1, 16385), "box")):
        with pytest.raises(ValueError):
            ops.resample_u8(wide, hw, filter)
        assert ops.resample_plan((1, 5120), hw, filter, DEV, reject_ok=True) is None
    assert tuple(ops.resample_u8(wide, (1, 21), "box").shape) == (1, 21, 3)  # 245 taps: served


def test_resample_plans_are_kept():
    from pgdvs_amd import ops

    a = ops.resample_plan((45, 60), (12, 16), "lanczos", DEV)
    assert ops.resample_plan((45, 60), (12, 16), "lanczos", DEV) is a and ops.resample_plan((45, 60), (12, 16), "box", DEV) is not a
    bounds_h, kk_h, bounds_v, kk_v = a.tables
    for got, want in zip((bounds_h, kk_h, bounds_v, kk_v), RS.table(60, 16, "lanczos") + RS.table(45, 12, "lanczos")):
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert ops.resample_plan((64, 64), (64, 17), "box", DEV).tables[2:] == (None, None)  # the axis that keeps its size has none
    for i in range(ops.RESAMPLE_PLANS):
        ops.resample_plan((100 + i, 9), (7, 5), "box", DEV)
    assert len(ops._resample_plans) == ops.RESAMPLE_PLANS and ops.resample_plan((45, 60), (12, 16), "lanczos", DEV) is not a


# ---------------------------------------------------------------------------- the loaders
BIG = (701, 83)  # for the 288 x 36 target: ratios 2.43 and 2.31


def _resave(path, hw, rng):
    """the image file at another size, seeded random bytes, under its name (PIL opens by content: a .jpg name keeps PNG bytes)"""
    PIL.Image.fromarray(rng.integers(0, 256, (*hw, 3), dtype=np.uint8)).save(path, format="PNG")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the resident tests' trees with image files that need the resize: every source frame of the NVIDIA tree (camera f % 12 of
    time step f) and every second other camera at 701 x 83, so that targets take both branches (a height that is not 288:
    the monocular video's size; 288: the file's own); some frames of the monocular video directory at two other sizes (the
    pure-geometry loader's LANCZOS stack); the monocular tree's frames behind frame 0, which sets the size, larger"""
    t = RC.build_trees(tmp_path_factory.mktemp("resample_gpu"))
    rng = np.random.default_rng(20261020)
    dense = pathlib.Path(t["nvidia"]) / "raw" / NT.SCENE / "dense"
    for f in range(NT.F):
        for c in range(NT.N_CAMS):
            if c == f % NT.N_CAMS or (f + c) % 2:
                png = dense / "mv_images" / f"{f:05d}" / f"cam{c + 1:02d}.png"
                _resave(png, BIG, rng)
                png.with_suffix(".jpg").write_bytes(png.read_bytes())
    for f, hw in ((1, BIG), (4, (300, 40)), (5, BIG), (9, (300, 40)), (13, (289, 36))):
        _resave(dense / f"images_{NT.W}x{NT.H}" / f"{f:05d}.png", hw, rng)
    for f in range(1, NT.MF):
        _resave(pathlib.Path(t["mono"]) / NT.MONO_SCENE / "rgbs" / f"{f:05d}.png", (97, 131) if f % 3 else (40, 57), rng)
    return t


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_resize_items_equal_the_resident_loaders(name, trees):
    want, got = RC.make(name, trees, device=DEV, resident=True), RC.make(name, trees, device=DEV, resident=True, device_resize=True)
    assert got.store.device_resize and not want.store.device_resize
    for i in range(len(want)):
        item = got[i]
        assert all(v.is_cuda for v in item.values() if isinstance(v, torch.Tensor)), [k for k, v in item.items()
                                                                                      if isinstance(v, torch.Tensor) and not v.is_cuda]
        RC.assert_items_equal(item, want[i], (name, i))
    st = got.store.stats
    assert st["frames_decoded"] == want.store.stats["frames_decoded"] == (NT.MF if name == "mono_vis" else NT.F)
    # the resize was taken: every source frame but the monocular tree's frame 0; the pure-geometry loader's five video frames
    assert st["frames_resized_on_device"] == {"mono_vis": NT.MF - 1, "nvidia_pure_geo": NT.F + 5}.get(name, NT.F)
    assert want.store.stats["frames_resized_on_device"] == 0
    if name in ("nvidia_eval", "nvidia_pure_geo"):  # targets of both branches
        assert 0 < st["targets_resized_on_device"] < len(want)


DYCHECK_KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DT.SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
                  flow_consist_thres=1.0, device=DEV, resident=True)


@pytest.fixture(scope="module")
def dycheck_tree(tmp_path_factory):
    """the DyCheck tree with every train frame behind the first, which sets the scene's size, stored larger"""
    root = DT.build_tree(tmp_path_factory.mktemp("resample_gpu_dycheck"))
    rng = np.random.default_rng(7)
    for t in DT.TRAIN_T[1:]:
        _resave(pathlib.Path(root) / "iphone" / DT.SCENE / f"rgb/{DT.FACTOR}x" / f"{DT.frame_name(0, t)}.png", (117, 149), rng)
    return root


def test_device_resize_items_equal_the_resident_loader_dycheck(dycheck_tree):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    want = DyCheckiPhoneEvaluationDataset(data_root=dycheck_tree, **DYCHECK_KW)
    got = DyCheckiPhoneEvaluationDataset(data_root=dycheck_tree, **DYCHECK_KW, device_resize=True)
    for i in range(len(want)):
        item, ref = got[i], want[i]
        assert list(item) == list(ref) and all(v.is_cuda for v in item.values() if isinstance(v, torch.Tensor))
        RC.assert_items_equal(item, ref, i)
    st = got.store.stats
    assert st["frames_decoded"] == want.store.stats["frames_decoded"] > 1
    assert 0 < st["frames_resized_on_device"] >= st["frames_decoded"] - 1  # (every decoded frame but, where it was used, the first)


def _refuse(*a, **kw):
    raise AssertionError("a device_resize __getitem__ waited for the device")


WAITS = ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
         (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"))


@pytest.mark.parametrize("name", ["nvidia_vis", "mono_vis", "nvidia_eval", "dycheck"])
def test_a_device_resize_item_never_waits_for_the_device(name, trees, dycheck_tree, monkeypatch):
    """tests/test_gpu_resident.py's check for this path, from the FIRST use of every frame on: the waiting calls raise while
    the items are built, the loader's frames are decoded and resized under them, and the items equal the resident loader's"""
    if name == "dycheck":
        from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

        make = lambda **kw: DyCheckiPhoneEvaluationDataset(data_root=dycheck_tree, **DYCHECK_KW, **kw)  # noqa: E731
    else:
        make = lambda **kw: RC.make(name, trees, device=DEV, resident=True, **kw)  # noqa: E731
    want, res = make(), make(device_resize=True)
    idx = range(0, len(res), 5 if name != "dycheck" else 3)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        for owner, attr in WAITS:
            m.setattr(owner, attr, _refuse)
        first = [res[i] for i in idx]
        assert res.store.stats["frames_resized_on_device"] > 0
        second = [res[i] for i in idx]
    for i, a, b in zip(idx, first, second):
        RC.assert_items_equal(a, want[i], (name, i, "first use"))
        RC.assert_items_equal(b, a, (name, i, "second use"))
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()) if isinstance(x, torch.Tensor))
