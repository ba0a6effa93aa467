"""``device_depth`` on the GPU (``pgdvs_depth_place``, ``pgdvs_percentile_f32``): ``ops.depth_place`` against the
loaders' numpy statements bit for bit (NaN compares as NaN) over the vector tail's widths, Pillow's NEAREST picks, the special
values, a mixed batch in one launch, a payload that is only 4-byte aligned, strided rows between guards and the C entry's
argument checks; ``ops.percentile_f32`` against ``np.percentile(x, 5)``; and the five loaders (the NVIDIA evaluation one in
prediction mode too) with every device option on against ``resident=True`` alone, on their fixture trees and on copies with
depth files of another size and files the device path does not serve."""
import ctypes as C
import pathlib
import shutil
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402
import resident_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -12345.5
SCALE = np.float32(0.37)
OPS = ("copy", "reciprocal", "scale")
# 0, -0, the sum x + 1e-8f is 0 (the division gives inf), 1e-8f, a denormal, a denormal quotient, the infinities, NaN
SPECIAL = np.array([0.0, -0.0, -np.float32(1e-8), np.float32(1e-8), 1e-40, 3e38, np.inf, -np.inf, np.nan, -3e38, 1.0, -2.5], np.float32)
ALL_ON = dict(device=DEV, resident=True, device_resize=True, device_decode=True, device_entropy=True, device_png=True, device_mask=True, device_depth=True)


def statement(x, op):
    """the loaders' numpy statements on a float32 array"""
    with np.errstate(all="ignore"):
        y = {"copy": x, "reciprocal": 1 / (x + 1e-8), "scale": x * SCALE}[op]
    assert y.dtype == np.float32  # (NumPy 2: the Python scalars are weak)
    return y


def nearest(y, shape):
    return y if y.shape == tuple(shape) else np.array(PIL.Image.fromarray(y).resize((shape[1], shape[0]), resample=PIL.Image.Resampling.NEAREST))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def values(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(0, 2, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.permutation(flat.size)[:min(flat.size, SPECIAL.size)]] = SPECIAL[:flat.size]
    return x


def request(x, op, out, lead=0):
    from pgdvs_amd import ops

    return ops.DepthRequest(bytes(lead) + x.tobytes(), lead, x.shape, op, SCALE, out)


def fresh(shape):
    return torch.full(shape, CANARY, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("op", OPS)
def test_same_size_over_the_vector_tail(op):
    from pgdvs_amd import ops

    assert statement(SPECIAL, "reciprocal")[2] == np.inf and 0 < statement(SPECIAL, "reciprocal")[5] < np.finfo(np.float32).tiny
    for W in (1, 3, 4, 5, 67):
        for H in (1, 3):
            x = values((H, W), 10 * W + H)
            (got,) = ops.depth_place([request(x, op, fresh((H, W)), lead=20)], device=DEV)
            assert same_bits(got.cpu().numpy(), statement(x, op)), (op, H, W)
    x = np.tile(SPECIAL, 11)[:128].reshape(8, 16)  # every special value through the 16-byte path
    assert same_bits(ops.depth_place([request(x, op, fresh((8, 16)))])[0].cpu().numpy(), statement(x, op))


@pytest.mark.parametrize("src,dst", [((7, 9), (3, 4)), ((5, 6), (11, 13)), ((1, 1), (4, 4))])
def test_another_size_goes_through_pillows_nearest_picks(src, dst):
    from pgdvs_amd import ops

    for op in OPS:
        x = values(src, src[0] * dst[1])
        (got,) = ops.depth_place([request(x, op, fresh(dst))])
        assert same_bits(got.cpu().numpy(), nearest(statement(x, op), dst)), (op, src, dst)


def test_five_entries_of_different_shapes_and_ops_are_one_launch(monkeypatch):
    from pgdvs_amd import _lib, ops

    shapes = [((3, 67), (3, 67), "reciprocal"), ((7, 9), (3, 4), "scale"), ((1, 5), (1, 5), "copy"), ((40, 33), (40, 33), "scale"), ((5, 6), (11, 13), "reciprocal")]
    xs = [values(s, k) for k, (s, _, _) in enumerate(shapes)]
    ops.depth_place([request(xs[0], "copy", fresh(shapes[0][1]))])  # (warm-up: the code object, the maps' uploads aside)
    lib, calls = _lib.load(), []
    real = lib.pgdvs_depth_place

    def counted(*a):
        calls.append(a[3])  # (n)
        return real(*a)

    monkeypatch.setattr(lib, "pgdvs_depth_place", counted)
    got = ops.depth_place([request(x, op, fresh(dst)) for x, (_, dst, op) in zip(xs, shapes)], device=DEV)
    assert calls == [5]
    for x, (src, dst, op), g in zip(xs, shapes, got):
        assert same_bits(g.cpu().numpy(), nearest(statement(x, op), dst)), (src, dst, op)


def test_a_payload_that_is_4_byte_but_not_16_byte_aligned():
    from pgdvs_amd import _lib, ops

    a, b = values((1, 3), 1), values((6, 67), 2)  # 12 bytes in front of the second payload: table 112, payloads at 112 and 124
    assert -(-2 * C.sizeof(_lib.DepthEntry) // 16) * 16 == 112 and C.sizeof(_lib.DepthEntry) == 56
    for op in OPS:
        got = ops.depth_place([request(a, op, fresh(a.shape)), request(b, op, fresh(b.shape))], align=4)
        assert same_bits(got[0].cpu().numpy(), statement(a, op)) and same_bits(got[1].cpu().numpy(), statement(b, op)), op
    with pytest.raises(ValueError, match="align"):
        ops.depth_place([request(a, "copy", fresh(a.shape))], align=2)


@pytest.mark.parametrize("W", [5, 64, 67])
def test_padded_rows_and_guards_stay_untouched(W):
    from pgdvs_amd import ops

    H, PAD = 9, 3
    for op in OPS:
        wide, x = fresh((H + 2, W + PAD)), values((H, W), W)
        out = wide[1:H + 1, :W]  # rows W + PAD floats apart, a guard row above and below
        ops.depth_place([request(x, op, out)])
        host = wide.cpu().numpy()
        assert same_bits(host[1:H + 1, :W], statement(x, op)), (op, W)
        host[1:H + 1, :W] = CANARY
        assert (host == CANARY).all(), (op, W)
        flat = fresh((H * W + 32,))  # contiguous rows between guards, off the 16-byte grid
        ops.depth_place([request(x, op, flat[15:15 + H * W].view(H, W))])
        host = flat.cpu().numpy()
        assert same_bits(host[15:15 + H * W].reshape(H, W), statement(x, op)) and (host[:15] == CANARY).all() and (host[15 + H * W:] == CANARY).all(), (op, W)
        mapped = fresh((H + 2, W + PAD))  # a mapped entry into strided rows
        small = values((4, 7), W + 1)
        ops.depth_place([request(small, op, mapped[1:H + 1, :W])])
        host = mapped.cpu().numpy()
        assert same_bits(host[1:H + 1, :W], nearest(statement(small, op), (H, W)))
        host[1:H + 1, :W] = CANARY
        assert (host == CANARY).all()


def test_argument_errors_return_minus_one_and_launch_nothing():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    x = values((4, 6), 3)
    out, index = fresh((4, 6)), ops.nearest_map((4, 6), (3, 5), DEV)
    buf = torch.zeros(64 + x.nbytes + 16, dtype=torch.uint8, pin_memory=True)
    table = (_lib.DepthEntry * 1).from_address(buf.data_ptr())
    buf.numpy()[64:64 + x.nbytes] = np.frombuffer(x.tobytes(), np.uint8)

    def call(nbytes=None, n=1, **fields):
        e = table[0]
        e.offset, e.h, e.w, e.op, e.scale, e.map, e.out, e.out_row_stride, e.H, e.W = 64, 4, 6, 1, 1.0, None, out.data_ptr(), 24, 4, 6
        for k, v in fields.items():
            setattr(e, k, v)
        dev = buf.to(DEV)
        rc = lib.pgdvs_depth_place(C.c_void_p(buf.data_ptr()), C.c_void_p(dev.data_ptr()), buf.numel() if nbytes is None else nbytes, n, ops._stream())
        torch.cuda.synchronize()
        return rc, lib.pgdvs_last_error().decode()

    bad = [dict(offset=66), dict(offset=buf.numel() - 8), dict(offset=48), dict(op=3), dict(op=-1), dict(H=3, W=5), dict(h=0), dict(W=16385, w=16385),
           dict(out_row_stride=20), dict(out_row_stride=26), dict(out=0), dict(out=out.data_ptr() + 2), dict(map=index.data_ptr() + 1, H=3, W=5)]
    for fields in bad:
        rc, text = call(**fields)
        assert rc == -1 and text.startswith("pgdvs_depth_place"), (fields, rc, text)
    assert call(nbytes=64 + x.nbytes - 4)[0] == -1 and call(nbytes=40)[0] == -1 and call(n=0)[0] == -1  # the payload / the table past the buffer
    assert (out == CANARY).all()  # nothing was launched
    assert call()[0] == 0 and same_bits(out.cpu().numpy(), statement(x, "reciprocal"))
    small = fresh((3, 5))
    assert call(map=index.data_ptr(), H=3, W=5, out=small.data_ptr(), out_row_stride=20)[0] == 0
    assert same_bits(small.cpu().numpy(), nearest(statement(x, "reciprocal"), (3, 5)))
    with pytest.raises(ValueError, match="float32"):
        ops.depth_place([request(x, "copy", torch.zeros((4, 6), dtype=torch.float64, device=DEV))])
    with pytest.raises(ValueError, match="op"):
        ops.depth_place([request(x, "square", out)])
    with pytest.raises(ValueError, match="floats at byte"):
        ops.depth_place([ops.DepthRequest(x.tobytes(), 8, x.shape, "copy", 1.0, out)])
    assert lib.pgdvs_abi_version() == 1


# ---------------------------------------------------------------------------- the percentile
def _percentile_cases():
    rng = np.random.default_rng(7)
    cases = {n: rng.normal(1.5, 2.0, n).astype(np.float32) for n in (1, 2, 20, 21, 4097)}
    cases["ties"] = np.repeat(np.float32([3.0, -1.0, 2.0, -1.0]), 25)
    cases["negatives"] = -rng.uniform(0.1, 9.0, 333).astype(np.float32)
    cases["infinities"] = np.concatenate([np.float32([np.inf, -np.inf, np.inf]), rng.normal(0, 1, 58).astype(np.float32)])
    cases["-inf at the rank"] = np.concatenate([np.full(5, -np.inf, np.float32), rng.normal(0, 1, 16).astype(np.float32)])
    cases["one NaN"] = np.concatenate([rng.normal(0, 1, 40).astype(np.float32), np.float32([np.nan])])
    cases["a frame"] = rng.uniform(0.5, 4.0, (40, 56)).astype(np.float32)
    return cases


def test_percentile_is_np_percentile_bit_for_bit():
    from pgdvs_amd import ops

    cases = _percentile_cases()
    assert (20 - 1) * 0.05 != int((20 - 1) * 0.05) and (21 - 1) * np.float32(0.05) == 1.0  # a fractional and a whole virtual index
    with np.errstate(all="ignore"):
        want = [np.percentile(x.reshape(-1), 5) for x in cases.values()]
    assert all(type(w) is np.float32 for w in want)
    got = ops.percentile_f32([torch.from_numpy(x).to(DEV) for x in cases.values()], 5)  # one batch
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (len(cases),)
    for label, g, w in zip(cases, got.cpu().numpy(), want):
        assert same_bits(np.float32([g]), np.float32([w])), (label, g, w)
    assert np.isnan(want[list(cases).index("one NaN")])
    for q in (0, 50, 100, 37.5):
        x = cases[4097]
        assert same_bits(ops.percentile_f32([torch.from_numpy(x).to(DEV)], q).cpu().numpy(), np.float32([np.percentile(x, q)])), q
    with pytest.raises(ValueError):
        ops.percentile_f32([], 5)
    with pytest.raises(ValueError):
        ops.percentile_f32([torch.zeros(4, device=DEV)], np.float64(5))


# ---------------------------------------------------------------------------- the loaders
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("depth_gpu"))


@pytest.fixture(scope="module")
def odd_trees(tmp_path_factory, trees):
    """copies of the trees with depth files the loaders must still read right: frame 2's of another size (the NEAREST picks, on
    the device), frame 4's float64 (the NVIDIA tree's frame 5 too: the host statement), and the monocular tree's frame 6
    ``np.savez_compressed`` (the same);
    "nvidia_one_size": the NVIDIA tree with the float64 file alone"""
    root = tmp_path_factory.mktemp("depth_gpu_odd")
    odd = {k: pathlib.Path(shutil.copytree(v, root / k)) for k, v in trees.items()}
    disp = odd["nvidia"] / "depths" / NT.SCENE / "disp"
    for f in (4, 5):
        np.save(disp / f"{f:05d}.npy", np.load(disp / f"{f:05d}.npy").astype(np.float64))
    odd["nvidia_one_size"] = pathlib.Path(shutil.copytree(odd["nvidia"], root / "nvidia_one_size"))  # (the pure-geometry loader stacks the video's depths)
    np.save(disp / "00002.npy", np.random.default_rng(2).uniform(0.2, 0.6, (100, 20)).astype(np.float32))
    depths = odd["mono"] / NT.MONO_SCENE / "depths"
    np.savez(depths / "00002.npz", depth=np.random.default_rng(3).uniform(0.9, 2.4, (25, 31)).astype(np.float32))
    np.savez(depths / "00004.npz", depth=np.load(depths / "00004.npz")["depth"].astype(np.float64))
    np.savez_compressed(depths / "00006.npz", depth=np.load(depths / "00006.npz")["depth"])
    np.savez(depths / "00000.npz", depth=np.random.default_rng(4).uniform(0.9, 2.4, (50, 70)).astype(np.float32))  # the frame _tgt_shape fills
    return odd


def _sample(n, k=6):
    return sorted({int(i) for i in np.linspace(0, n - 1, k)})


def _compare(got, want, what, unserved=()):
    """items equal on a first and a second pass; every filled frame's depth placed on the device but the ``unserved`` ones"""
    idx = _sample(len(want))
    for i in idx:
        RC.assert_items_equal(got[i], want[i], (what, i))
    st, ref = got.store.stats, want.store.stats
    (scene,) = got.store.scenes.values()
    filled = {int(s) + scene.first_id for s in np.flatnonzero(scene.filled)}
    fallbacks = len(filled & set(unserved))
    assert st["depth_fallbacks"] == fallbacks and st["depths_placed_on_device"] == len(filled) - fallbacks > 0, (what, st, sorted(filled))
    assert st["frames_decoded"] == len(filled) == ref["frames_decoded"] and "depths_placed_on_device" not in ref
    assert st["flow_files_read"] == ref["flow_files_read"] and st["zoe_files_read"] == ref["zoe_files_read"] and st["items_built"] == ref["items_built"]
    once = ("frames_decoded", "depths_placed_on_device", "depth_fallbacks", "flow_files_read", "zoe_files_read")
    before = {k: st[k] for k in once}
    for i in (idx[0], idx[-1]):
        RC.assert_items_equal(got[i], want[i], (what, i, "second pass"))
    assert {k: st[k] for k in once} == before  # nothing is read or placed twice
    assert got.store._staged_depths == {}
    return filled


def _same_valid_fs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(np.array_equal(np.asarray(u), np.asarray(v)) and type(u) is type(v) for u, v in zip(x, y)), (x, y)


@pytest.mark.parametrize("name", RC.LOADERS)
def test_items_equal_the_resident_loaders(name, trees):
    want, got = RC.make(name, trees, device=DEV, resident=True), RC.make(name, trees, **ALL_ON)
    assert got.store.device_depth and not want.store.device_depth
    _same_valid_fs(got.valid_fs, want.valid_fs)
    _compare(got, want, name)


@pytest.mark.parametrize("name", RC.LOADERS)
def test_items_equal_on_a_tree_with_odd_depth_files(name, odd_trees):
    geo = name == "nvidia_pure_geo"
    t = dict(odd_trees, nvidia=odd_trees["nvidia_one_size"]) if geo else odd_trees
    want, got = RC.make(name, t, device=DEV, resident=True), RC.make(name, t, **ALL_ON)
    _same_valid_fs(got.valid_fs, want.valid_fs)
    unserved = (4, 6) if name == "mono_vis" else (4, 5)
    filled = _compare(got, want, name, unserved=unserved)
    assert (geo or 2 in filled) and filled & set(unserved), (name, sorted(filled))  # the NEAREST picks and the host statement were both taken


@pytest.mark.parametrize("setting,container", [("k_me_med_share", "zip"), ("moe", "dir")])
def test_prediction_mode_items_equal(tmp_path_factory, setting, container):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    tree = ZT.build_tree(tmp_path_factory.mktemp("depth_gpu_zoe"))
    odd = tuple(range(1, NT.F, 2)) if container == "dir" else ()
    for f in odd:  # every other frame's files compressed: the host statement from the same bytes, and "moe" still picks its pair
        for t in ZT.TYPES:
            path = tree / ZT.ZOE_DIR / NT.SCENE / "dense" / f"zoe_depths_{t}" / f"{f:05d}.npz"
            np.savez_compressed(path, **dict(np.load(path)))
    kw = dict(data_root=tree, use_zoe_depth=setting, zoe_depth_data_path=ZT.CONTAINERS[container], **ZT.KW)
    want, got = NvidiaDynEvaluationDataset(device=DEV, resident=True, **kw), NvidiaDynEvaluationDataset(**ALL_ON, **kw)
    filled = _compare(got, want, (setting, container), unserved=odd)
    assert got.store.scenes[NT.SCENE].prediction and (not odd or filled & set(odd))


DYCHECK_KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DT.SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2, flow_consist_thres=1.0)


def test_dycheck_items_equal_and_a_float64_file_is_refused_as_before(tmp_path_factory):
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    root = DT.build_tree(tmp_path_factory.mktemp("depth_gpu_dycheck"))
    depth = pathlib.Path(root) / "iphone" / DT.SCENE / f"depth/{DT.FACTOR}x"
    for t in (9, 11):  # another size
        np.save(depth / f"{DT.frame_name(0, t)}.npy", np.random.default_rng(t).uniform(1.0, 3.0, (30, 41, 1)).astype(np.float32))
    want = DyCheckiPhoneEvaluationDataset(data_root=root, device=DEV, resident=True, **DYCHECK_KW)
    got = DyCheckiPhoneEvaluationDataset(data_root=root, **ALL_ON, **DYCHECK_KW)
    filled = _compare(got, want, "dycheck")
    assert filled & {9, 11}
    other = DT.build_tree(tmp_path_factory.mktemp("depth_gpu_dycheck64"))
    for t in DT.TRAIN_T:
        path = pathlib.Path(other) / "iphone" / DT.SCENE / f"depth/{DT.FACTOR}x" / f"{DT.frame_name(0, t)}.npy"
        np.save(path, np.load(path).astype(np.float64))
    for kw in (dict(device=DEV, resident=True), ALL_ON):
        ds = DyCheckiPhoneEvaluationDataset(data_root=other, **kw, **DYCHECK_KW)
        with pytest.raises(ValueError, match="float64"):
            ds[0]
    assert ds.store.stats["depth_fallbacks"] > 0 and ds.store.stats["depths_placed_on_device"] == 0 and ds.store._staged_depths == {}


def test_flow_pair_under_the_option_is_todays_pair(tmp_path):
    from pgdvs_amd.datasets.resident import SceneStore

    H, W = 9, 14
    rng = np.random.default_rng(11)
    flow, cd = rng.normal(0, 2, (H, W, 2)).astype(np.float32), rng.normal(0, 0.8, (H, W, 2)).astype(np.float32)
    cd[0, 0], cd[0, 1] = np.nan, (0.5, 0.5)  # a NaN, and a sum that equals the threshold
    np.savez(tmp_path / "stored.npz", flow=flow, coord_diff=cd)
    np.savez_compressed(tmp_path / "compressed.npz", flow=flow, coord_diff=cd)
    np.savez(tmp_path / "wide.npz", flow=flow.astype(np.float64), coord_diff=cd)
    np.savez(tmp_path / "cd64.npz", flow=flow, coord_diff=cd.astype(np.float64))
    today, store = SceneStore(DEV), SceneStore(DEV, device_resize=True, device_depth=True)
    scenes = [s.scene("s", 2, (H, W)) for s in (today, store)]
    for k, name in enumerate(("stored", "compressed", "wide")):
        want, got = (s.flow(scene, 0, k + 1, tmp_path / f"{name}.npz") for s, scene in zip((today, store), scenes))
        assert all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(RC.bits(g), RC.bits(w)) for g, w in zip(got, want)), name
    assert store.stats["flow_files_read"] == today.stats["flow_files_read"] == 3 and store.nbytes >= today.nbytes
    held = scenes[1].flows[0, 1][0]
    assert held.untyped_storage().nbytes() >= H * W * 16 and store._pair_bytes(scenes[1], scenes[1].flows[0, 1]) == H * W * 12 + held.untyped_storage().nbytes() - H * W * 8
    for s, scene in zip((today, store), scenes):
        with pytest.raises(ValueError, match="coord_diff is float64"):
            s.flow(scene, 1, 0, tmp_path / "cd64.npz")
