"""``device_depth`` without a GPU: the reader of ``.npy`` headers and stored ``.npz`` members (``datasets/npy_file.py``) over files
it serves -- its offset and shape give ``np.load``'s array bit for bit -- and files it must leave to the host statement, which
it refuses with a reason and without raising; the sixth keyword's rule behind the five, through the check function, the store
and a loader; and the store's fill with ``ops.depth_place`` replaced by a recorder: one call per fill with each frame's op,
scale, source shape and slot, a refused file read by the host statement and counted, and nothing staged left behind."""
import io
import itertools
import pathlib
import sys
import zipfile

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import resident_cases as RC  # noqa: E402

from pgdvs_amd.datasets import npy_file  # noqa: E402  (the module this feature adds)


def _npy(array, version=None, fortran=False):
    """the bytes ``np.save`` (or ``np.lib.format.write_array`` at ``version``) writes"""
    out = io.BytesIO()
    if version is None:
        np.save(out, np.asfortranarray(array) if fortran else array)
    else:
        np.lib.format.write_array(out, np.asfortranarray(array) if fortran else array, version=version)
    return out.getvalue()


def _values(shape, seed=0):
    """float32 noise with the special values in front, as far as they fit"""
    x = np.random.default_rng(seed).normal(0, 3, shape).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)[:x.size]
    x.reshape(-1)[:special.size] = special
    return x


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _from_payload(data, offset, shape):
    return np.frombuffer(data, "<f4", int(np.prod(shape, dtype=np.int64)), offset).reshape(shape)


SERVED_NPY = [(f"v{v[0]}.{v[1]} {shape}", _npy(_values(shape, k), v)) for k, (v, shape) in
              enumerate(itertools.product(((1, 0), (2, 0), (3, 0)), ((7, 9), (7, 9, 1), (1, 1), (5,))))]


@pytest.mark.parametrize("label,data", SERVED_NPY, ids=[c[0] for c in SERVED_NPY])
def test_npy_payload_gives_np_load_bit_for_bit(label, data):
    offset, shape, reason = npy_file.npy_payload(data)
    want = np.load(io.BytesIO(data))
    assert reason is None and shape == want.shape and _same_bits(_from_payload(data, offset, shape), want), label
    assert data[6:8] == bytes(int(c) for c in label[1:4].split("."))  # (the version the label names)
    assert npy_file.npy_payload(data + b"trailing") == (offset, shape, None)  # bytes behind the payload are np.load's to ignore too
    assert npy_file.npy_payload(memoryview(data))[:2] == (offset, shape)


def _refused_npy():
    x = _values((6, 5), 3)
    good = _npy(x)
    return [("Fortran order", _npy(x, fortran=True), "Fortran"), ("big-endian", _npy(x.astype(">f4")), "descr"), ("float16", _npy(x.astype(np.float16)), "descr"),
            ("float64", _npy(x.astype(np.float64)), "descr"), ("int32", _npy(np.arange(30, dtype=np.int32).reshape(6, 5)), "descr"),
            ("object array", _npy(np.array([[1, "a"], [None, 2.5]], dtype=object)), "descr"), ("cut by one byte", good[:-1], "cut short"),
            ("random bytes", np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8).tobytes(), "magic"), ("empty", b"", "magic"),
            ("header cut", good[:40], "cut short"), ("version 4.0", good[:6] + b"\x04\x00" + good[8:], "version"),
            ("header no literal", good[:10] + b"{" * (len(good) - 10 - x.nbytes) + good[-x.nbytes:], "unreadable header")]


@pytest.mark.parametrize("label,data,word", _refused_npy(), ids=[c[0] for c in _refused_npy()])
def test_npy_payload_refuses_with_a_reason_and_raises_nothing(label, data, word):
    offset, shape, reason = npy_file.npy_payload(data)
    assert offset is None and shape is None and isinstance(reason, str) and word in reason, (label, reason)


def test_npz_member_honours_the_local_header_of_np_savez(tmp_path):
    arrays = {"depth": _values((9, 13), 1), "flow": _values((9, 13, 2), 2), "K": np.eye(4), "scale": np.float64(0.25), "pred": _values((4, 6, 1), 3)}
    path = tmp_path / "several.npz"
    np.savez(path, **arrays)
    data = path.read_bytes()
    loaded = np.load(path)
    with zipfile.ZipFile(path) as z:
        infos = {i.filename: i for i in z.infolist()}
    for name in ("depth", "flow", "pred"):
        offset, shape, reason = npy_file.npz_member(data, name)
        assert reason is None and shape == arrays[name].shape and _same_bits(_from_payload(data, offset, shape), loaded[name]), name
        info = infos[name + ".npy"]
        assert info.extra == b""  # the central directory shows no extra field ...
        member = info.header_offset + 30 + len(info.filename)
        n, m = np.frombuffer(data, "<u2", 2, info.header_offset + 26)
        assert n == len(info.filename) and m > 0  # ... and the local header has one (zip64): the payload lies behind it
        assert data[member:member + 6] != npy_file.MAGIC and data[member + m:member + m + 6] == npy_file.MAGIC
        assert offset != member and offset - (member + m) in range(64, 4096)  # (behind the extra field and the member's own .npy header)
        assert offset == npy_file.npy_payload(data, member + m, member + m + info.file_size)[0]
    for name, word in (("K", "descr"), ("scale", "descr"), ("missing", "no member")):
        assert npy_file.npz_member(data, name)[:2] == (None, None) and word in npy_file.npz_member(data, name)[2], name


def test_npz_member_refuses_compressed_missing_and_damaged_archives(tmp_path):
    x = _values((9, 13), 4)
    np.savez_compressed(tmp_path / "c.npz", depth=x)
    np.savez(tmp_path / "s.npz", depth=x)
    compressed, stored = (tmp_path / "c.npz").read_bytes(), (tmp_path / "s.npz").read_bytes()
    assert npy_file.npz_member(stored, "depth")[2] is None
    cases = [("compressed", compressed, "depth", "compressed"), ("missing member", stored, "depth_pred", "no member"),
             ("truncated archive", stored[:len(stored) // 2], "depth", "unreadable archive"), ("no archive", b"\x93NUMPY" + bytes(40), "depth", "unreadable archive"),
             ("directory only", stored[-120:], "depth", "")]
    for label, data, name, word in cases:
        offset, shape, reason = npy_file.npz_member(data, name)
        assert offset is None and shape is None and isinstance(reason, str) and word in reason, (label, reason)
    moved = bytearray(stored)  # a directory that points at no local header
    moved[0:4] = b"XXXX"
    assert npy_file.npz_member(bytes(moved), "depth")[0] is None
    encrypted = bytearray(stored)
    at = encrypted.rfind(b"PK\x01\x02")
    encrypted[at + 8] |= 1  # the central entry's flag bit 0
    assert "encrypted" in npy_file.npz_member(bytes(encrypted), "depth")[2]


# ---------------------------------------------------------------------------- the keyword
FLAGS = ("resize", "decode", "entropy", "png", "mask", "depth")


def missing(resize, decode, entropy, png, mask, depth, resident, device):
    """(the option refused, what the first broken rule asks for), or None: the rules in their order of precedence -- the five
    of the image input, then the sixth"""
    rules = ((entropy and not decode, "device_entropy", "device_decode=True"),
             (png and not resize, "device_png", "device_resize=True"),
             (mask and not resize, "device_mask", "device_resize=True"),
             (decode and not resize, "device_decode", "device_resize=True"),
             (resize and not resident, "device_resize", "resident=True"),
             (resize and (device is None or torch.device(device).type != "cuda"), "device_resize", "GPU"),
             (depth and not resize, "device_depth", "device_resize=True"))
    return next(((option, what) for broken, option, what in rules if broken), None)


def _checked(owner, resident, device, flags):
    from pgdvs_amd.datasets._common import device_depth, device_input

    options = device_input(owner, resident=resident, device=device, **{f"device_{n}": v for n, v in zip(FLAGS[:5], flags[:5])})
    return options, device_depth(owner, options, flags[5])


def test_the_truth_table_with_the_sixth_flag():
    from pgdvs_amd.datasets._common import DeviceInput
    from pgdvs_amd.datasets.resident import SceneStore

    assert DeviceInput._fields == FLAGS[:5]  # the record stays the five-field tuple
    for flags in itertools.product((False, True), repeat=6):
        for resident, device in itertools.product((False, True), (None, "cpu", "cuda:0")):
            want = missing(*flags, resident, device)
            if want is None:
                options, depth = _checked("Loader", resident, device, flags)
                assert tuple(options) == flags[:5] and depth is flags[5]
            else:
                with pytest.raises(ValueError, match=want[1]) as err:
                    _checked("Loader", resident, device, flags)
                text = str(err.value)  # the family's form: "<owner>(<option>=True) ...: it needs <what>"
                assert text.startswith(f"Loader({want[0]}=True) ") and ": it needs " in text and (want[1] == "GPU" or text.endswith(f": it needs {want[1]}")), text
        kw = {f"device_{n}": v for n, v in zip(FLAGS, flags)}
        want = missing(*flags, True, "cuda:0")
        if want is None:
            store = SceneStore("cuda:0", **kw)
            assert store.device_depth is flags[5] and (store.device_resize, store.device_mask) == (flags[0], flags[4])
            assert ("depths_placed_on_device" in store.stats) == ("depth_fallbacks" in store.stats) == flags[5]
            assert len(store.stats) == 13 + 2 * flags[4] + 2 * flags[5]  # (the record is the old one without the option)
        else:
            with pytest.raises(ValueError, match=f"SceneStore.{want[0]}=True.*{want[1]}"):
                SceneStore("cuda:0", **kw)
    with pytest.raises(ValueError, match="SceneStore.device_depth=True.*: it needs device_resize=True"):
        SceneStore(device="cuda:0", device_depth=True)  # (refused in front of any device work)
    with pytest.raises(ValueError, match="device_entropy=True"):
        SceneStore(device="cuda:0", device_depth=True, device_entropy=True)  # (the five come first)


@pytest.mark.parametrize("name", RC.LOADERS)
def test_loaders_refuse_the_keyword_without_device_resize(name, tmp_path):
    trees = RC.build_trees(tmp_path)
    with pytest.raises(ValueError, match=r"Dataset\(device_depth=True\).*: it needs device_resize=True"):
        RC.make(name, trees, resident=True, device_depth=True, **({} if name == "nvidia_pure_geo" else {"device": None}))
    with pytest.raises(ValueError, match="device_png=True.*device_resize=True"):
        RC.make(name, trees, resident=True, device_depth=True, device_png=True, **({} if name == "nvidia_pure_geo" else {"device": None}))
    if name != "nvidia_pure_geo":  # (builds its cloud on a GPU)
        got = RC.make(name, trees, resident=True)
        assert got.store.device_depth is False and len(got.store.stats) == 13


def test_dycheck_loader_refuses_the_keyword_without_device_resize(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
              scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
              flow_consist_thres=1.0)
    with pytest.raises(ValueError, match=r"DyCheckiPhoneEvaluationDataset\(device_depth=True\).*: it needs device_resize=True"):
        DyCheckiPhoneEvaluationDataset(**kw, resident=True, device_depth=True)
    ds = DyCheckiPhoneEvaluationDataset(**kw, resident=True)
    request = ds._depth_request(DT.SCENE, DT.TRAIN_T[0])  # depth * scale is float32 under a Python scale: the request names it as float32
    assert request[1:3] == (None, "scale") and type(request[3]) is np.float32 and request[3] == np.float32(DT.SCALE)
    assert npy_file.npy_payload(pathlib.Path(request[0]).read_bytes())[1] == (DT.H, DT.W, 1)
    ds.parser_dict[DT.SCENE]._scale = np.float64(DT.SCALE)  # a float64 product: no request, the loader's host statement refuses as before
    assert ds._depth_request(DT.SCENE, DT.TRAIN_T[0]) is None


# ---------------------------------------------------------------------------- the store's fill, ops.depth_place recorded
H, W = 6, 10


def _host_scene(store, n_frames, first_id=0):
    """a scene's tables in host memory under a store that believes itself on a GPU: no device is touched"""
    from pgdvs_amd.datasets.resident import _Scene

    return _Scene(n_frames, H, W, None, first_id)


@pytest.fixture
def recorded(monkeypatch):
    """``ops.depth_place`` replaced by a recorder that fills each out with the numpy statement (sizes equal) or marks it"""
    from pgdvs_amd import ops

    calls = []

    def depth_place(requests, device=None, align=16):
        calls.append([r._replace(data=None) for r in requests])
        for r in requests:
            x = np.frombuffer(r.data, "<f4", r.shape[0] * r.shape[1], r.offset).reshape(r.shape)
            if tuple(r.out.shape) == tuple(r.shape):
                with np.errstate(all="ignore"):
                    y = {"copy": x, "reciprocal": 1 / (x + 1e-8), "scale": x * r.scale}[r.op]
                assert y.dtype == np.float32
                r.out.copy_(torch.from_numpy(np.array(y)))
            else:
                r.out.fill_(-7.0)
        return [r.out for r in requests]

    monkeypatch.setattr(ops, "depth_place", depth_place)
    return calls


def _store():
    from pgdvs_amd.datasets.resident import SceneStore

    return SceneStore("cuda:0", device_resize=True, device_depth=True)


def test_fill_places_the_missing_frames_depths_in_one_call(tmp_path, recorded):
    store = _store()
    scene = _host_scene(store, 6, first_id=10)
    disp = {f: _values((H, W), f) for f in range(10, 16)}
    disp[12] = _values((9, 4), 12)  # another size: through the NEAREST picks, on the device
    scaled = _values((H, W, 1), 20)
    for f, x in disp.items():
        np.save(tmp_path / f"{f}.npy", x)
    np.save(tmp_path / "13.npy", disp[13].astype(np.float64))  # not served: the host statement
    np.savez(tmp_path / "14.npz", depth_pred=disp[14], scale=np.float64(2.0))
    np.save(tmp_path / "15.npy", scaled)
    blob = (tmp_path / "14.npz").read_bytes()
    requests = {10: (tmp_path / "10.npy", None, "reciprocal", 1.0), 11: (str(tmp_path / "11.npy"), None, "copy", 1.0),
                12: (tmp_path / "12.npy", None, "reciprocal", 1.0), 13: (tmp_path / "13.npy", None, "reciprocal", 1.0),
                14: (blob, "depth_pred", "copy", 1.0), 15: (tmp_path / "15.npy", None, "scale", np.float32(0.37))}
    seen = {}

    def decode(f):
        staged = store.staged_depth(scene, f)
        seen[f] = staged
        depth = staged.depth if staged.depth is not None else 1 / (np.load(tmp_path / f"{f}.npy") + 1e-8)
        return np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), depth

    scene.filled[1] = True  # frame 11 is there already: not asked for, not placed
    ids = [15, 10, 12, 11, 13, 14, 10]
    store._fill(scene, ids, decode, None, depth_request=requests.__getitem__)
    assert len(recorded) == 1 and store._staged_depths == {} and store._prefetched == {}
    call = {int((r.out.data_ptr() - scene.depth.data_ptr()) // (scene.depth.stride(0) * 4)) + 10: r for r in recorded[0]}
    assert sorted(call) == [10, 12, 14, 15]
    assert [(call[f].shape, call[f].op, float(call[f].scale)) for f in sorted(call)] == [
        ((H, W), "reciprocal", 1.0), ((9, 4), "reciprocal", 1.0), ((H, W), "copy", 1.0), ((H, W), "scale", float(np.float32(0.37)))]
    assert all(call[f].out.data_ptr() == scene.depth[f - 10].data_ptr() and tuple(call[f].out.shape) == (H, W) for f in call)
    assert store.stats["depths_placed_on_device"] == 4 and store.stats["depth_fallbacks"] == 1 and store.stats["frames_decoded"] == 5
    assert seen[13].depth is None and seen[13].data is None and seen[14].data == blob and seen[10].data is None and 11 not in seen
    with np.errstate(all="ignore"):
        assert _same_bits(scene.depth[0].numpy(), 1 / (disp[10] + 1e-8))
        assert _same_bits(scene.depth[3].numpy(), (1 / (disp[13].astype(np.float64) + 1e-8)).astype(np.float32))  # the host statement, then F32
        assert _same_bits(scene.depth[4].numpy(), disp[14]) and _same_bits(scene.depth[5].numpy(), scaled[..., 0] * np.float32(0.37))
    assert (scene.depth[2] == -7.0).all() and scene.filled[[0, 1, 2, 3, 4, 5]].all()
    store._fill(scene, ids, decode, None, depth_request=requests.__getitem__)  # nothing is missing: nothing is asked, read or placed
    assert len(recorded) == 1 and store.stats["depths_placed_on_device"] == 4


def test_fill_without_a_request_or_without_the_option_is_the_host_path(tmp_path, recorded):
    from pgdvs_amd.datasets.resident import SceneStore

    decode = lambda f: (np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 2.5, np.float32))  # noqa: E731
    store = _store()
    scene = _host_scene(store, 2)
    store._fill(scene, [0, 1], decode)  # positional, as the existing callers
    assert recorded == [] and store.stats["depths_placed_on_device"] == 0 and store.stats["depth_fallbacks"] == 0 and (scene.depth == 2.5).all()
    assert store.staged_depth(scene, 0) is None and store.staged_depth(None, 0) is None
    off = SceneStore("cuda:0", device_resize=True)
    scene = _host_scene(off, 2)
    off._fill(scene, [0, 1], decode, None, None, depth_request=lambda f: 1 / 0)  # off: the request is never asked
    assert recorded == [] and "depths_placed_on_device" not in off.stats and len(off.stats) == 13


def test_unserved_missing_and_unnamed_files_are_counted_and_left_to_the_host(tmp_path, recorded):
    store = _store()
    scene = _host_scene(store, 4)
    np.savez_compressed(tmp_path / "0.npz", depth=_values((H, W), 0))
    np.save(tmp_path / "1.npy", _values((H, W, 1), 1))  # a trailing axis belongs to the "scale" files alone
    requests = {0: (tmp_path / "0.npz", "depth", "copy", 1.0), 1: (tmp_path / "1.npy", None, "reciprocal", 1.0),
                2: (tmp_path / "none.npy", None, "copy", 1.0), 3: None}
    host = []

    def decode(f):
        assert store.staged_depth(scene, f).depth is None
        host.append(f)
        return np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), np.ones((H, W), np.float64)

    store._fill(scene, [0, 1, 2, 3], decode, depth_request=requests.__getitem__)
    assert recorded == [] and host == [0, 1, 2, 3] and store.stats["depth_fallbacks"] == 4 and store.stats["depths_placed_on_device"] == 0


def test_a_reader_that_raises_leaves_nothing_staged(tmp_path, recorded):
    store = _store()
    scene = _host_scene(store, 3)
    for f in range(3):
        np.save(tmp_path / f"{f}.npy", _values((H, W), f))

    def decode(f):
        if f == 1:
            raise OSError("the image reader fails")
        return np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), store.staged_depth(scene, f).depth

    with pytest.raises(OSError, match="the image reader fails"):
        store._fill(scene, [0, 1, 2], decode, depth_request=lambda f: (tmp_path / f"{f}.npy", None, "copy", 1.0))
    assert len(recorded) == 1 and len(recorded[0]) == 3 and store._staged_depths == {} and store._prefetched == {}
    assert scene.filled.tolist() == [True, False, False] and store.staged_depth(scene, 2) is None

    def request(f):
        raise KeyError("the request itself fails")

    with pytest.raises(KeyError):
        store._fill(scene, [1, 2], decode, depth_request=request)
    assert store._staged_depths == {} and len(recorded) == 1


def test_put_recognises_a_depth_that_is_its_slot_and_checks_a_tensor():
    store = _store()
    scene = _host_scene(store, 2)
    rgb, mask = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    scene.depth[1].fill_(4.0)
    store.put(scene, 1, rgb, mask, scene.depth[1])  # the slot itself: nothing is copied over it
    assert (scene.depth[1] == 4.0).all() and scene.filled[1]
    store.put(scene, 0, rgb, mask, torch.full((H, W), 3.0))  # another float32 tensor is copied
    assert (scene.depth[0] == 3.0).all()
    with pytest.raises(ValueError, match="depth"):
        store.put(scene, 0, rgb, mask, torch.zeros((H, W), dtype=torch.float64))
    with pytest.raises(ValueError, match="depth"):
        store.put(scene, 0, rgb, mask, torch.zeros((H, W + 1)))
