"""The mask PNG reader on the GPU (``pgdvs_png_decode``, ``pgdvs_mask_place``): every file of
tests/png_mask_cases.py byte for byte Pillow's through ``ops.png_decode_batch(kinds="mask")``, alone and in one mixed batch with
RGB and RGBA files that costs one call of the C entry (as the colour files alone do) and writes rows with a stride; ``ops.mask_place`` against Pillow's NEAREST
and against the evaluation mask's numpy expression; and the five loaders with ``device_mask`` on trees whose masks mix the
formats: items bit for bit the ``device_resize`` loaders', the counters the tree implies, one wait per item fill."""
import io
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import nvidia_tree as NT  # noqa: E402
import png_decode_cases as PC  # noqa: E402
import png_mask_cases as MC  # noqa: E402
import resident_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = 0x5A


# ---------------------------------------------------------------------------- the decode
def test_every_case_alone_is_pillows():
    from pgdvs_amd import ops

    for label, data in MC.cases():
        got = ops.png_decode(data, device=DEV, kinds="mask")
        want = MC.pillow(data)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), label
    with pytest.raises(ValueError, match="colour type"):
        ops.png_decode(MC.cases()[0][1], device=DEV)  # the default kinds refuse it, as before


def test_one_mixed_batch_is_one_call_and_writes_strided_rows(monkeypatch):
    from pgdvs_amd import _lib, ops

    colour = [d for _, d in PC.streams()[:8]]  # RGB and RGBA in turns
    assert {PC.split(d)[2] for d in colour} == {3, 4}
    masks = [d for _, d in MC.cases()]
    datas = masks[:len(masks) // 2] + colour + masks[len(masks) // 2:]
    wants = [np.array(PIL.Image.open(io.BytesIO(d))).astype(np.uint8) for d in datas]
    PAD = 5  # bytes between a row's end and the next row
    wide = [torch.full((w.shape[0], int(np.prod(w.shape[1:])) + PAD), CANARY, dtype=torch.uint8, device=DEV) for w in wants]
    outs = [b[:, :b.shape[1] - PAD].view(w.shape[0], w.shape[1], -1) if w.ndim == 3 else b[:, :w.shape[1]] for b, w in zip(wide, wants)]
    ops.png_decode(masks[0], device=DEV, kinds="mask")  # (warm-up: the code object, the side stream)
    lib, calls = _lib.load(), []
    real = lib.pgdvs_png_decode

    def counted(*a):
        calls.append(a[3])  # (nstreams)
        return real(*a)

    monkeypatch.setattr(lib, "pgdvs_png_decode", counted)
    got = ops.png_decode_batch(datas, outs=outs, device=DEV, kinds=("colour", "mask"))
    alone = ops.png_decode_batch(colour, device=DEV)  # the colour files alone: the same one entry, once
    monkeypatch.undo()
    assert calls == [len(datas), len(colour)]  # one call of the one entry per batch, masks or not
    for k, (g, d) in enumerate(zip(alone, colour)):
        want = PC.pillow(d)
        assert g.dtype == torch.uint8 and tuple(g.shape) == want.shape and np.array_equal(g.cpu().numpy(), want), k
    for k, (g, o, b, w) in enumerate(zip(got, outs, wide, wants)):
        assert g is o and tuple(g.shape) == w.shape and (g.stride(0) > int(np.prod(w.shape[1:])) or w.shape[0] == 1), k
        host = b.cpu().numpy()
        assert np.array_equal(host[:, :host.shape[1] - PAD].reshape(w.shape), w), k
        assert (host[:, host.shape[1] - PAD:] == CANARY).all(), (k, "written between the rows")


def test_damaged_mask_streams_are_given_up_with_the_emulations_status():
    from pgdvs_amd import ops

    cases = MC.device_refusals()
    emu = ops.png_decode_host([d for _, d, _ in cases], kinds="mask", guard=64)
    reasons = []
    got = ops.png_decode_batch([d for _, d, _ in cases] + [MC.cases()[3][1]], device=DEV, reject_ok=True, reasons=reasons, kinds="mask")
    for (label, _, bits), e, g, why in zip(cases, emu, got, reasons):
        assert g is None and e["status"] & bits and f"{e['status']:#x}" in why, (label, why, hex(e["status"]))
    assert got[-1] is not None and reasons[-1] is None and np.array_equal(got[-1].cpu().numpy(), MC.pillow(MC.cases()[3][1]))


# ---------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("src,dst", [((37, 53), (19, 29)), ((37, 53), (74, 106)), ((37, 53), (37, 53))])
def test_mask_place_is_pillows_nearest(src, dst):
    from pgdvs_amd import ops

    rng = np.random.default_rng(src[0] + dst[0])
    m = rng.integers(0, 256, src, dtype=np.uint8)
    want = np.array(PIL.Image.fromarray(m).resize((dst[1], dst[0]), resample=PIL.Image.Resampling.NEAREST))
    got = ops.mask_place(torch.from_numpy(m).to(DEV), dst)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    bits = m > 127  # a 1-bit mask resizes to the same picks
    want1 = np.array(PIL.Image.fromarray(bits).resize((dst[1], dst[0]), resample=PIL.Image.Resampling.NEAREST)).astype(np.uint8)
    table = torch.full((3, dst[0] * dst[1] + 7), CANARY, dtype=torch.uint8, device=DEV)  # a slot of a padded table, from rows with a stride
    slot = table[1, :dst[0] * dst[1]].view(dst)
    wide = torch.full((src[0], src[1] + 3), CANARY, dtype=torch.uint8, device=DEV)
    wide[:, :src[1]] = torch.from_numpy(bits.astype(np.uint8)).to(DEV)
    assert ops.mask_place(wide[:, :src[1]], dst, out=slot) is slot
    host = table.cpu().numpy()
    assert np.array_equal(host[1, :dst[0] * dst[1]].reshape(dst), want1) and (host[0] == CANARY).all() and (host[2] == CANARY).all()
    assert (host[1, dst[0] * dst[1]:] == CANARY).all()
    with pytest.raises(ValueError, match="mask_place"):
        ops.mask_place(torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV), (2, 2))


@pytest.mark.parametrize("channels", [1, 3])
def test_mask_place_expands_the_evaluation_mask(channels):
    from pgdvs_amd import ops

    rng = np.random.default_rng(channels)
    m = rng.integers(0, 3, (37, 53, channels), dtype=np.uint8) * rng.integers(0, 2, (37, 53, 1), dtype=np.uint8) * 127
    image = PIL.Image.fromarray(m[..., 0] if channels == 1 else m)
    want = np.float32(np.array(image.convert("RGB"))[..., ::-1] > 1e-3)
    src = torch.from_numpy(m[..., 0] if channels == 1 else m).to(DEV)
    got = ops.mask_place(src, mode="bgr_f32")
    assert got.dtype == torch.float32 and tuple(got.shape) == (37, 53, 3) and np.array_equal(got.cpu().numpy(), want)
    assert 0 < want.mean() < 1 and (channels == 1 or not np.array_equal(want, want[..., ::-1]))
    with pytest.raises(ValueError, match="keeps the size"):
        ops.mask_place(src, (19, 29), mode="bgr_f32")


# ---------------------------------------------------------------------------- the loaders
OTHER = (301, 47)  # a mask of another size than the 288 x 36 frames


def _blob(hw, k):
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    return (xx - hw[1] * (0.3 + 0.02 * k)) ** 2 + (yy - hw[0] * 0.5) ** 2 < (0.25 * hw[1]) ** 2


def _sixteen(hw, k):
    b = io.BytesIO()
    PIL.Image.fromarray(_blob(hw, k).astype(np.uint16) * 40000).save(b, format="png")
    return b.getvalue()


def _write_mask(path, hw, k, other):
    """frame k's mask in the format k names: 1-bit, ``L``, ``P``, 1-bit of another size, ``L`` of another size"""
    kind = k % 5
    blob = _blob(other if kind >= 3 else hw, k)
    if kind in (0, 3):
        PIL.Image.fromarray(blob).save(path)
    elif kind in (1, 4):
        PIL.Image.fromarray(blob.astype(np.uint8) * (255 if kind == 1 else 1)).save(path)
    else:
        PIL.Image.fromarray(np.dstack([blob * 255, blob * 0, blob * 255]).astype(np.uint8)).convert("P").save(path)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the resident tests' trees with the frames' masks in turns a 1-bit file, an ``L`` file, a ``P`` file and two of another
    size, and the NVIDIA tree's evaluation masks (RGB as built) in turns RGB, ``L``, 1-bit, ``P`` and 16-bit grey (one of
    another size has no host statement to fall back to: the loaders' resize refuses its float image)"""
    t = RC.build_trees(tmp_path_factory.mktemp("mask_gpu"))
    masks = pathlib.Path(t["nvidia"]) / "masks" / NT.SCENE / "dense" / "masks" / "final"
    for f in range(NT.F):
        _write_mask(masks / f"{f:05d}_final.png", (NT.H, NT.W), f, OTHER)
    mono = pathlib.Path(t["mono"]) / NT.MONO_SCENE / "masks" / "final"
    for f in range(NT.MF):
        _write_mask(mono / f"{f:05d}_final.png", (NT.MH, NT.MW), f + 1, (97, 131))
    dense = pathlib.Path(t["nvidia"]) / "raw" / NT.SCENE / "dense"
    for f in range(NT.F):
        for c in range(NT.N_CAMS):
            path, kind = dense / "mv_masks" / f"{f:05d}" / f"cam{c + 1:02d}.png", (f + c) % 5
            blob = _blob((NT.H, NT.W), f + c)
            if kind == 1:
                PIL.Image.fromarray(blob.astype(np.uint8) * 200).save(path)
            elif kind == 2:
                PIL.Image.fromarray(blob).save(path)
            elif kind == 3:
                PIL.Image.fromarray(np.dstack([blob * 255] * 3).astype(np.uint8)).convert("P").save(path)
            elif kind == 4:
                path.write_bytes(_sixteen((NT.H, NT.W), f + c))
    return t


def _served(path, shape=None):
    """whether the device path serves the file, from what Pillow says it is: a mask file (``shape`` None) is a grey or palette
    file of at most 8 bits; an evaluation mask a grey or 8-bit RGB file of the target's size"""
    with PIL.Image.open(path) as im:
        if shape is None:
            return im.mode in ("1", "L", "P")
        return im.mode in ("1", "L", "RGB") and (im.size[1], im.size[0]) == tuple(shape)


def _instrument(ds, monkeypatch):
    """(log of (path, served), fills = [(missing frames, waits inside the fill, prefetch table empty afterwards)])"""
    store, log, fills, state = ds.store, [], [], {"n": 0}
    inner_mask, inner_eval, inner_fill, inner_sync = store.decode_mask, store.decode_eval_mask, store._fill, torch.cuda.Event.synchronize

    def decode_mask(path, shape=None, into=None):
        log.append((pathlib.Path(path), _served(path)))
        return inner_mask(path, shape, into)

    def decode_eval_mask(path, shape):
        log.append((pathlib.Path(path), _served(path, shape)))
        return inner_eval(path, shape)

    def synchronize(self):
        state["n"] += 1
        return inner_sync(self)

    def fill(scene, frame_ids, decode, image_path=None, mask_path=None):
        missing = [f for f in sorted(set(frame_ids)) if not scene.filled[f - scene.first_id]]
        before = state["n"]
        inner_fill(scene, frame_ids, decode, image_path, mask_path)
        fills.append((len(missing), state["n"] - before, not store._prefetched))

    monkeypatch.setattr(torch.cuda.Event, "synchronize", synchronize)
    store.decode_mask, store.decode_eval_mask, store._fill = decode_mask, decode_eval_mask, fill
    return log, fills


def _check_counts_and_waits(got, want, log, fills, several=1):
    """``several``: some fill must have more missing frames than this (the pure-geometry items have two source frames, and one
    of them is there already)"""
    st, ref = got.store.stats, want.store.stats
    served, unserved = sum(s for _, s in log), sum(not s for _, s in log)
    assert st["masks_decoded_on_device"] == served > 0 and st["mask_fallbacks"] == unserved, (st, served, unserved)
    assert "masks_decoded_on_device" not in ref and len(ref) == 13
    for key in ref:
        if key not in ("png_decoded_on_device", "png_fallbacks", "frames_decoded_on_device", "targets_decoded_on_device"):
            assert st[key] == ref[key], (key, st[key], ref[key])
    # one wait per item fill, images and masks together; a fill with no missing frame waits for nothing
    assert fills and all(empty for *_, empty in fills), fills
    assert all(waits == (1 if missing else 0) for missing, waits, _ in fills), fills
    assert any(missing > several for missing, *_ in fills), fills


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_mask_items_equal_the_device_resize_loaders(name, trees, monkeypatch):
    kw = dict(device=DEV, resident=True, device_resize=True)
    want, got = RC.make(name, trees, **kw), RC.make(name, trees, **kw, device_png=True, device_mask=True)
    assert got.store.device_mask and not want.store.device_mask
    log, fills = _instrument(got, monkeypatch)
    for i in range(len(want)):
        RC.assert_items_equal(got[i], want[i], (name, i))
    _check_counts_and_waits(got, want, log, fills, several=0 if name == "nvidia_pure_geo" else 1)
    has_eval = name in ("nvidia_eval", "nvidia_pure_geo")  # the frames' masks fall back nowhere; palette and 16-bit evaluation masks do
    assert any(not s for _, s in log) == has_eval and {p.parent.name == "final" for p, _ in log} == ({True, False} if has_eval else {True})


def test_device_mask_alone_is_one_batch_of_masks_and_one_wait(trees, monkeypatch):
    kw = dict(device=DEV, resident=True, device_resize=True)
    want, got = RC.make("nvidia_vis", trees, **kw), RC.make("nvidia_vis", trees, **kw, device_mask=True)
    assert got.store.device_mask and not got.store.device_png
    log, fills = _instrument(got, monkeypatch)
    for i in range(0, len(want), 3):
        RC.assert_items_equal(got[i], want[i], i)
    st = got.store.stats
    assert st["masks_decoded_on_device"] == len(log) > 0 and st["mask_fallbacks"] == 0 and st["png_decoded_on_device"] == 0
    assert all(waits == (1 if missing else 0) and empty for missing, waits, empty in fills) and any(missing > 1 for missing, *_ in fills), fills


def test_a_mask_the_device_path_does_not_serve_is_the_host_statements(tmp_path):
    from pgdvs_amd.datasets.resident import SceneStore

    store = SceneStore(DEV, device_resize=True, device_mask=True)
    deep, rgb, noise = tmp_path / "deep.png", tmp_path / "rgb.png", tmp_path / "noise.png"
    deep.write_bytes(_sixteen((9, 13), 1))
    PIL.Image.fromarray(PC.content("smooth", 9, 13, 3, 1)).save(rgb)
    noise.write_bytes(bytes(range(40)))
    for path in (deep, rgb):
        want = np.array(PIL.Image.open(path))
        got = store.decode_mask(path)
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), path
    with pytest.raises(PIL.UnidentifiedImageError):
        store.decode_mask(noise)
    with pytest.raises(FileNotFoundError):
        store.decode_mask(tmp_path / "none.png")
    assert store.stats["mask_fallbacks"] == 3 and store.stats["masks_decoded_on_device"] == 0
    scene = store.scene("s", 2, (9, 13))
    one = tmp_path / "one.png"
    PIL.Image.fromarray(_blob((9, 13), 0)).save(one)
    got = store.decode_mask(one, (9, 13), into=(scene, 1))
    assert got.data_ptr() == scene.dyn_mask[1].data_ptr() and np.array_equal(got.cpu().numpy(), _blob((9, 13), 0).astype(np.uint8))
    big = tmp_path / "big.png"
    PIL.Image.fromarray(_blob((31, 20), 0)).save(big)
    got = store.decode_mask(big, (9, 13), into=(scene, 0))
    want = np.array(PIL.Image.fromarray(_blob((31, 20), 0)).resize((13, 9), resample=PIL.Image.Resampling.NEAREST)).astype(np.uint8)
    assert got.data_ptr() == scene.dyn_mask[0].data_ptr() and np.array_equal(got.cpu().numpy(), want)
    store.put(scene, 0, np.zeros((9, 13, 3), np.uint8), got, np.ones((9, 13), np.float32))  # the slot's own mask is recognised
    assert np.array_equal(scene.dyn_mask[0].cpu().numpy(), want) and store.stats["masks_decoded_on_device"] == 2


DYCHECK_KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DT.SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
                  flow_consist_thres=1.0, device=DEV, resident=True, device_resize=True)


def test_device_mask_items_equal_the_device_resize_loader_dycheck(tmp_path_factory, monkeypatch):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    root = DT.build_tree(tmp_path_factory.mktemp("mask_gpu_dycheck"))
    masks = pathlib.Path(root) / "flow_mask" / DT.SCENE / "masks" / "final"
    for k, t in enumerate(DT.TRAIN_T):
        _write_mask(masks / f"{DT.frame_name(0, t)}_final.png", (DT.H, DT.W), k, (117, 149))
    covis = pathlib.Path(root) / "iphone" / DT.SCENE / f"covisible/{DT.FACTOR}x/val"
    for k, (c, t) in enumerate(DT.VAL):  # ``L`` as built, then in turns 1-bit, 16-bit, palette
        path = covis / f"{DT.frame_name(c, t)}.png"
        if k % 4 == 1:
            PIL.Image.fromarray(_blob((DT.H, DT.W), k)).save(path)
        elif k % 4 == 2:
            path.write_bytes(_sixteen((DT.H, DT.W), k))
        elif k % 4 == 3:
            PIL.Image.fromarray(np.dstack([_blob((DT.H, DT.W), k) * 255] * 3).astype(np.uint8)).convert("P").save(path)
    want = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW)
    got = DyCheckiPhoneEvaluationDataset(data_root=root, **DYCHECK_KW, device_png=True, device_mask=True)
    log, fills = _instrument(got, monkeypatch)
    for i in range(len(want)):
        item, ref = got[i], want[i]
        assert list(item) == list(ref) and all(v.is_cuda for v in item.values() if isinstance(v, torch.Tensor))
        RC.assert_items_equal(item, ref, i)
    _check_counts_and_waits(got, want, log, fills)
    assert sum(p.parent.name == "val" for p, _ in log) == len(want) and sum(not s for p, s in log if p.parent.name == "val") == 2  # (the 16-bit files)
