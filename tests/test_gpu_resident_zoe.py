"""ZoeDepth inputs from the resident store on the MI355X (csrc/depth_range.hip item_zoe_kernel, ``ops.item_zoe_depth``,
``NvidiaDynEvaluationDataset(resident=True, use_zoe_depth=..., device=...)``): the loader's items against the host disk path's and
the reference's fixture; the op against a numpy statement (``numpy_depth`` / ``numpy_range`` of tests/test_gpu_nvidia_zoe.py,
never against itself) over slots that are padded, views that are and are not 16-byte aligned, repeated ids out of order and
guard words around every output; the edge predictions; the limits, with buffers that a refused call must leave alone.

Bit identity is derived, not measured: every operation of the chain is one correctly rounded IEEE operation in a fixed
order and the order statistics are exact, so there is no tolerance anywhere in this file."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402
import resident_cases as RC  # noqa: E402
from test_gpu_nvidia_zoe import cameras, edge_view, numpy_depth, numpy_range, same_bits  # noqa: E402
from test_nvidia_zoe_host import assert_item_equals_fixture  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

DEV = "cuda:0"
CANARY = 0x5AA55AA5
GROUPS = [[2, 0, 2], [1], [0, 0]]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return ZT.build_tree(tmp_path_factory.mktemp("resident_zoe_gpu"))


# ---------------------------------------------------------------------------- loader
@pytest.mark.parametrize("setting,container", [("k_me_med_share", "zip"), ("moe", "dir")])
def test_device_store_items_equal_the_host_disk_items_and_the_fixture(tree, golden_dir, setting, container):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    g = dict(np.load(golden_dir / "nvidia_zoe_items.npz"))
    kw = dict(data_root=tree, use_zoe_depth=setting, zoe_depth_data_path=ZT.CONTAINERS[container], **ZT.KW)
    disk = NvidiaDynEvaluationDataset(**kw)
    want = [disk[f * NT.N_CAMS + c] for f, c in ZT.ITEMS]
    for device_resize in (False, True):
        res = NvidiaDynEvaluationDataset(device=DEV, resident=True, device_resize=device_resize, **kw)
        assert res.store.device == torch.device(DEV)
        for n, (f, c) in enumerate(ZT.ITEMS):
            got = res[f * NT.N_CAMS + c]
            off = [k for k, v in got.items() if isinstance(v, torch.Tensor) and not v.is_cuda]
            assert not off, (device_resize, n, off)
            RC.assert_items_equal(got, want[n], (setting, container, device_resize, n))
            host = {k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in got.items()}
            assert_item_equals_fixture(host, g, f"{setting}_{container}_i{n}_")
        scene = res.store.scenes[NT.SCENE]
        filled = set(np.flatnonzero(scene.filled).tolist())
        assert scene.prediction and ZT.ZERO_PRED_FRAME in filled and ZT.ZERO_SCALE_FRAME in filled and filled & set(ZT.TIE_FRAMES)
        stats = dict(res.store.stats)
        again = res[ZT.ITEMS[0][0] * NT.N_CAMS + ZT.ITEMS[0][1]]  # nothing is read or decoded twice
        RC.assert_items_equal(again, want[0], "second pass")
        assert res.store.stats["zoe_files_read"] == stats["zoe_files_read"] and res.store.stats["frames_decoded"] == stats["frames_decoded"]


# ---------------------------------------------------------------------------- the op
def _table(pred):
    """[F,H,W] host predictions -> the store's table on the device: every frame in a slot padded to 16 bytes, the padding
    holding NaN bits that no output may show"""
    F, n = pred.shape[0], pred[0].size
    slot = -(-n * 4 // 16) * 4
    tab = torch.full((F, slot), float("nan"), dtype=torch.float32, device=DEV)
    view = tab[:, :n].view(pred.shape)
    view.copy_(torch.from_numpy(pred))
    return view, slot * 4


def _carve(groups, H, W, gap):
    """one output [n,H,W,1] per group carved out of a canary-filled buffer, ``gap`` floats around each"""
    sizes = [len(g) * H * W for g in groups]
    buf = torch.full((sum(sizes) + gap * (len(sizes) + 1),), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    out, keep, off = [], np.ones(buf.numel(), bool), gap
    for g, s in zip(groups, sizes):
        out.append(buf[off:off + s].view(len(g), H, W, 1))
        keep[off:off + s] = False
        off += s + gap
    return buf, out, keep


def _case(F, H, W, seed):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.3, 6.0, (F, H, W)).astype(np.float32)
    n_views = sum(len(g) for g in GROUPS)
    ss = np.stack([rng.uniform(0.7, 1.4, n_views), rng.uniform(-0.03, 0.05, n_views)], 1)
    ss[1] = [0.0, 0.37]  # a scale the fit clamped to 0: a constant depth
    return pred, ss, cameras(len(GROUPS[0]), H, W, rng)


@pytest.mark.parametrize("F,H,W", [(3, 2, 3), (5, 7, 13), (4, 4, 8), (3, 33, 65)])
def test_op_equals_numpy(F, H, W):
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.nvidia_eval import ray_rows

    pred, ss, (Ks, c2ws, tgt) = _case(F, H, W, 100000 + 1000 * H + W)  # (seeds whose cameras look at the cloud: near is not clamped)
    table, slot = _table(pred)
    assert slot % 16 == 0 and (slot != 4 * H * W) == ((H * W) % 4 != 0) and ((F, H, W) != (5, 7, 13) or slot == 368)
    ids = [i for g in GROUPS for i in g]
    want64 = numpy_depth(pred[ids], ss)  # per VIEW: the same frame under two pairs gives two depths
    want = want64.astype(np.float32)
    want_nf = numpy_range(want64[:len(GROUPS[0])], Ks, c2ws, tgt)
    assert 1e-16 < want_nf[0] < want_nf[1] and np.all(want64[1] == want64[1, 0, 0])
    rays = torch.from_numpy(ray_rows(Ks, c2ws).astype(np.float32)).to(DEV)
    for gap in (4, 5):  # outputs at 16-byte boundaries (where H W allows) and off them
        buf, out, keep = _carve(GROUPS, H, W, gap)
        nf = torch.zeros(2, dtype=torch.float64, device=DEV)
        ret, rng32 = ops.item_zoe_depth(table, GROUPS, ss, rays, np.linalg.inv(tgt), near_far=nf, out=out)
        torch.cuda.synchronize()
        assert ret is out
        host = buf.cpu().view(torch.int32).numpy()
        assert (host[keep] == CANARY).all(), (gap, "a guard word was overwritten")
        got = np.concatenate([o.cpu().numpy()[..., 0] for o in out])
        assert same_bits(got, want), (gap, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
        assert same_bits(nf.cpu().numpy(), want_nf), (gap, nf.cpu().numpy(), want_nf)
        assert same_bits(rng32.cpu().numpy(), want_nf.astype(np.float32)), (gap, rng32, want_nf)
    # without a range: the same depths, in tensors the op allocates, and no range
    ret, none = ops.item_zoe_depth(table, GROUPS, ss)
    assert none is None and [tuple(o.shape) for o in ret] == [(len(g), H, W, 1) for g in GROUPS]
    assert same_bits(np.concatenate([o.cpu().numpy()[..., 0] for o in ret]), want)
    # a second witness: the stacked-prediction op on the gathered stack
    stack = torch.from_numpy(np.ascontiguousarray(pred[ids])).to(DEV)
    assert same_bits(ops.nvidia_zoe_depth(stack, ss).cpu().numpy(), want)
    d3, r3 = ops.nvidia_zoe_depth(stack[:3].contiguous(), ss[:3], rays, np.linalg.inv(tgt))
    assert same_bits(r3.cpu().numpy(), want_nf.astype(np.float32)) and same_bits(d3.cpu().numpy(), want[:3])


def test_edge_values_in_one_slot():
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.nvidia_eval import ray_rows

    pred, ss = edge_view()
    table, _ = _table(pred[None])
    for s in (ss, np.array([[-2.0, -1e-16]]), np.array([[0.0, np.nextafter(-1e-16, 0.0)]])):
        want = numpy_depth(pred[None], s)
        (got,), _ = ops.item_zoe_depth(table, [[0]], s)
        got = got.cpu().numpy()[..., 0]
        assert same_bits(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), (s, got, want)
    want_inf = numpy_depth(pred[None], np.array([[-2.0, -1e-16]]))[0]
    want_big = numpy_depth(pred[None], np.array([[0.0, np.nextafter(-1e-16, 0.0)]]))[0]
    assert np.isposinf(want_inf[0, 3]) and want_big[2, 2] == 2.0 ** 106  # the inf and the 2^106 cases were among them
    # on the range path the NaN pixel decides: (1e-16, 2e-16); without it, the clamped numpy pair
    K, c2w = np.eye(4)[None], np.eye(4)[None]
    rays = torch.from_numpy(ray_rows(K, c2w).astype(np.float32)).to(DEV)
    nf = torch.zeros(2, dtype=torch.float64, device=DEV)
    (got,), rng32 = ops.item_zoe_depth(table, [[0]], ss, rays, np.eye(4), near_far=nf)
    want = numpy_depth(pred[None], ss)
    assert same_bits(got.cpu().numpy()[..., 0].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert nf.cpu().numpy().tolist() == [1e-16, 2e-16] and same_bits(nf.cpu().numpy(), numpy_range(want, K, c2w, np.eye(4)))
    assert rng32.cpu().numpy().tolist() == [np.float32(1e-16), np.float32(2e-16)]
    clean = pred.copy()
    clean[0, 4] = 2.0
    table_c, _ = _table(clean[None])
    want_c = numpy_depth(clean[None], ss)
    want_nf = numpy_range(want_c, K, c2w, np.eye(4))
    (got,), rng32 = ops.item_zoe_depth(table_c, [[0]], ss, rays, np.eye(4), near_far=nf)
    assert want_nf[0] == 1e-16 < want_nf[1]
    assert same_bits(nf.cpu().numpy(), want_nf) and same_bits(rng32.cpu().numpy(), want_nf.astype(np.float32))
    assert same_bits(got.cpu().numpy()[..., 0], want_c.astype(np.float32))


def test_limits_and_refused_calls_write_nothing():
    from pgdvs_amd import _lib, ops

    C = _lib.C
    rng = np.random.default_rng(64)
    F, H, W = 6, 3, 5
    pred = rng.uniform(0.3, 6.0, (F, H, W)).astype(np.float32)
    table, slot = _table(pred)
    ids = rng.integers(0, F, 64).tolist()
    groups = [ids[:1], ids[1:31], ids[31:44], ids[44:]]  # 64 views in 4 groups
    ss = np.stack([rng.uniform(0.7, 1.4, 64), rng.uniform(-0.03, 0.05, 64)], 1)
    Ks, c2ws, tgt = cameras(1, H, W, rng)
    from pgdvs_amd.datasets.nvidia_eval import ray_rows

    rays = torch.from_numpy(ray_rows(Ks, c2ws).astype(np.float32)).to(DEV)
    nf = torch.zeros(2, dtype=torch.float64, device=DEV)
    out, _ = ops.item_zoe_depth(table, groups, ss, rays, np.linalg.inv(tgt), near_far=nf)
    want64 = numpy_depth(pred[ids], ss)
    assert same_bits(np.concatenate([o.cpu().numpy()[..., 0] for o in out]), want64.astype(np.float32))
    assert same_bits(nf.cpu().numpy(), numpy_range(want64[:1], Ks, c2ws, tgt))
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [ids + [0]], np.ones((65, 2)))  # 65 views
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[0]] * 5, np.ones((5, 2)))  # five groups
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[F]], np.ones((1, 2)))  # no such frame
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[0], []], np.ones((1, 2)))  # an empty group
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[0, 1]], np.ones((3, 2)))  # a scale and shift per view
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[0]], np.ones((1, 2)), rays)  # rays without the target's pose
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table, [[0, 1]], np.ones((2, 2)), rays, np.eye(4))  # rays of another group size
    with pytest.raises(ValueError):  # frames 60 bytes apart: the slots are not padded
        ops.item_zoe_depth(torch.from_numpy(pred).to(DEV), [[0]], np.ones((1, 2)))
    with pytest.raises(ValueError):
        ops.item_zoe_depth(table.double(), [[0]], np.ones((1, 2)))
    with pytest.raises(ops.PgdvsHipError):
        ops.item_zoe_depth(table.cpu(), [[0]], np.ones((1, 2)))
    one, _ = _table(np.ones((2, 1, 1), np.float32))
    with pytest.raises(ops.PgdvsHipError):  # H W == 1 with a range (the workspace query refuses it first)
        ops.item_zoe_depth(one, [[0, 1]], np.ones((2, 2)), torch.zeros(2, 12, device=DEV), np.eye(4))
    (d,), _ = ops.item_zoe_depth(one, [[1]], np.array([[2.0, -0.25]]))  # ... and without one it is served
    assert same_bits(d.cpu().numpy().reshape(1, 1, 1), numpy_depth(np.ones((1, 1, 1), np.float32), [[2.0, -0.25]]).astype(np.float32))
    # the entry point itself: buffers filled beforehand are untouched after every refused call
    lib = _lib.load()
    obuf = torch.full((4 * H * W + 8,), 3.5, device=DEV)
    ws = torch.zeros(lib.pgdvs_item_zoe_depths_workspace_bytes(2, H, W), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 2 * H * W * 8
    rbuf = torch.full((2,), 3.5, device=DEV)
    inv = (C.c_double * 16)(*np.linalg.inv(tgt).reshape(-1).tolist())
    rays2 = torch.from_numpy(ray_rows(np.stack([Ks[0]] * 2), np.stack([c2ws[0]] * 2)).astype(np.float32)).to(DEV)  # (n_range is 2 below)
    ssv = (C.c_double * 130)(*([1.0, 0.0] * 65))

    def call(F=F, H=H, W=W, slot=slot, ids=(0, 1, 2), sizes=(2, 1), n_views=None, n_groups=None, with_range=True, table=table, ws_bytes=ws.numel()):
        outs = (C.c_void_p * max(len(sizes), 1))(*[obuf.data_ptr() + 4 * (4 + sum(sizes[:k]) * H * W) for k in range(len(sizes))])
        r = (rays2.data_ptr(), inv, rbuf.data_ptr(), nf.data_ptr(), ws.data_ptr(), ws_bytes) if with_range else (None, None, None, None, None, 0)
        return lib.pgdvs_item_zoe_depths(table.data_ptr(), F, H, W, slot, (C.c_int32 * len(ids))(*ids), len(ids) if n_views is None else n_views,
                                         ssv, (C.c_int32 * max(len(sizes), 1))(*sizes), len(sizes) if n_groups is None else n_groups, outs, *r,
                                         ops._stream())

    nf.zero_()
    assert call(ids=tuple(range(6)) * 11, sizes=(65,), n_views=65) == -1            # 65 views
    assert call(ids=(0, 1, 2, 3, 4), sizes=(1, 1, 1, 1, 1)) == -1                    # five groups
    assert call(ids=(0, F, 1)) == -1                                                 # an id equal to F
    assert call(sizes=(3, 0)) == -1                                                  # an empty group
    assert call(sizes=(1, 1)) == -1                                                  # groups short of the ids
    assert call(slot=slot - 4) == -1                                                 # a slot off 16 bytes
    assert call(table=one, F=2, H=1, W=1, slot=16, ids=(0, 1), sizes=(2,)) == -1     # H W == 1 with a range
    assert call(ws_bytes=lib.pgdvs_item_zoe_depths_workspace_bytes(2, H, W) - 1) == -3   # a workspace one byte short
    assert b"pgdvs_item_zoe_depths" in lib.pgdvs_last_error()
    assert lib.pgdvs_item_zoe_depths_workspace_bytes(2, 1, 1) == lib.pgdvs_item_zoe_depths_workspace_bytes(0, 4, 4) == -1
    torch.cuda.synchronize()
    assert (obuf.cpu().numpy() == 3.5).all() and (rbuf.cpu().numpy() == 3.5).all() and not ws.any().item() and not nf.any().item()
    # ... and the same arguments unrefused write exactly the outputs
    assert call() == 0
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    assert (got[:4] == 3.5).all() and (got[4 + 3 * H * W:] == 3.5).all()
    assert same_bits(got[4:4 + 3 * H * W].reshape(3, H, W), numpy_depth(pred[:3], [[1.0, 0.0]] * 3).astype(np.float32))
    assert same_bits(nf.cpu().numpy(), numpy_range(numpy_depth(pred[:2], [[1.0, 0.0]] * 2), np.stack([Ks[0]] * 2), np.stack([c2ws[0]] * 2), tgt))
