"""The ZoeDepth alignment fused into the NVIDIA depth range on the MI355X (csrc/depth_range.hip, DESIGN.md 8f-3 NVIDIA):
bit-identical to a numpy statement written here (upstream's three lines, then the float64 unprojection and
depth_range_from_points) and to the reference's fixture, never compared with itself: the loader's device path item for
item, the op on shapes that are no multiple of the block and span several, edge values in one small view, the
conversion-only call between guard words, and the argument checks.

Bit identity is derived, not measured: every operation of the chain is one correctly rounded IEEE operation in a fixed
order and the order statistics are exact, so any mismatch is a contracted or approximated operation in the kernel."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402
from test_nvidia_zoe_host import assert_item_equals_fixture  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return ZT.build_tree(tmp_path_factory.mktemp("nvidia_zoe"))


def numpy_depth(pred, ss):
    """upstream's three lines per view, with the scale and shift as the 0-d float64 arrays an .npz gives"""
    out = []
    for p, (a, b) in zip(pred, ss):
        scale, shift = np.asarray(np.float64(a)), np.asarray(np.float64(b))
        raw_disp = 1.0 / (p + 1e-16)
        disp = scale * raw_disp + shift
        depth = 1 / (disp + 1e-16)
        assert raw_disp.dtype == np.float32 and depth.dtype == np.float64
        out.append(depth)
    return np.stack(out)


def numpy_range(depth64, Ks, c2ws, c2w_tgt):
    from pgdvs_amd.datasets.nvidia_eval import depth_range_from_points, ray_constants

    V, H, W = depth64.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    pix = np.stack([u.reshape(-1), v.reshape(-1), np.ones(H * W, np.float32)], 0)
    cloud = []
    for K, c2w, d in zip(Ks, c2ws, depth64):
        M, o = ray_constants(K, c2w)
        rays_d = (M @ pix).T
        assert rays_d.dtype == np.float32 and o.dtype == np.float32
        cloud.append(o[None, :] + rays_d * d.reshape(-1, 1))  # float32 rays, float64 depth: float64 points
    cloud = np.concatenate(cloud, axis=0)
    assert cloud.dtype == np.float64
    return depth_range_from_points(cloud, c2w_tgt)


def run_op(pred, ss, Ks=None, c2ws=None, c2w_tgt=None):
    """(depth float32 [V,H,W], depth_range float32[2] or None, near_far float64[2] or None) of the op"""
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.nvidia_eval import ray_rows

    p = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(DEV)
    if Ks is None:
        depth = ops.nvidia_zoe_depth(p, ss)
        torch.cuda.synchronize()
        return depth.cpu().numpy(), None, None
    nf = torch.zeros(2, dtype=torch.float64, device=DEV)
    rays = torch.from_numpy(ray_rows(Ks, c2ws).astype(np.float32)).to(DEV)
    depth, rng = ops.nvidia_zoe_depth(p, ss, rays, np.linalg.inv(c2w_tgt), near_far=nf)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), rng.cpu().numpy(), nf.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def cameras(V, H, W, rng):
    Ks, c2ws = [], []
    for v in range(V):
        K = np.eye(4)
        f = (0.8 + 0.4 * rng.random()) * max(H, W)
        K[:3, :3] = [[f, 0, W / 2.0 + rng.normal()], [0, f * (1 + 0.01 * rng.normal()), H / 2.0 + rng.normal()], [0, 0, 1]]
        c2w = np.eye(4)
        c2w[:3, :3] = np.linalg.qr(np.eye(3) + 0.1 * rng.normal(size=(3, 3)))[0]
        c2w[:3, 3] = 0.2 * rng.normal(size=3)
        Ks.append(K)
        c2ws.append(c2w)
    tgt = np.eye(4)
    tgt[:3, :3] = np.linalg.qr(np.eye(3) + 0.1 * rng.normal(size=(3, 3)))[0]
    tgt[:3, 3] = 0.2 * rng.normal(size=3)
    return np.stack(Ks), np.stack(c2ws), tgt


# ---------------------------------------------------------------------------- loader
@pytest.mark.parametrize("setting,container", [("k_me_med_share", "zip"), ("moe", "dir")])
def test_loader_device_items_equal_host_items_and_fixture(tree, golden_dir, setting, container):
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    g = dict(np.load(golden_dir / "nvidia_zoe_items.npz"))
    kw = dict(data_root=tree, use_zoe_depth=setting, zoe_depth_data_path=ZT.CONTAINERS[container], **ZT.KW)
    host, dev = NvidiaDynEvaluationDataset(**kw), NvidiaDynEvaluationDataset(device=DEV, **kw)
    for n, (f, c) in enumerate(g["items"]):
        idx = int(f) * NT.N_CAMS + int(c)
        a, b = host[idx], dev[idx]
        assert a.keys() == b.keys() and a["misc"] == b["misc"]
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert not b[k].is_cuda and same_bits(a[k].numpy(), b[k].numpy()), (n, k)
        assert_item_equals_fixture(b, g, f"{setting}_{container}_i{n}_")


# ---------------------------------------------------------------------------- direct op
@pytest.mark.parametrize("V,H,W", [(1, 2, 3), (3, 7, 13), (4, 33, 65)])
def test_range_path_vs_numpy(V, H, W):
    rng = np.random.default_rng(100 * V + H)
    pred = rng.uniform(0.3, 6.0, (V, H, W)).astype(np.float32)
    ss = np.stack([rng.uniform(0.7, 1.4, V), rng.uniform(-0.03, 0.05, V)], 1)
    if V > 1:
        ss[1] = [0.0, 0.37]  # a scale the fit clamped to 0: a constant depth
    Ks, c2ws, tgt = cameras(V, H, W, rng)
    want = numpy_depth(pred, ss)
    want_nf = numpy_range(want, Ks, c2ws, tgt)
    depth, rng32, nf = run_op(pred, ss, Ks, c2ws, tgt)
    assert same_bits(depth, want.astype(np.float32)), np.abs(depth - want).max()
    assert same_bits(nf, want_nf), (nf, want_nf)
    assert same_bits(rng32, want_nf.astype(np.float32)), (rng32, want_nf)
    assert 1e-16 < want_nf[0] < want_nf[1]
    if V > 1:
        assert np.all(want[1] == want[1, 0, 0])
    # the float64 cloud is not the float32 one: the disparity path's op gives another pair on the same depths
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.nvidia_eval import ray_rows

    nf32 = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.nvidia_depth_range(torch.from_numpy(depth).to(DEV), torch.from_numpy(ray_rows(Ks, c2ws).astype(np.float32)).to(DEV),
                           np.linalg.inv(tgt), near_far=nf32)
    if V * H * W > 100:
        assert not same_bits(nf32.cpu().numpy(), want_nf)


def edge_view():
    """one 4 x 5 view (scale 2, shift -0.5; other pixels 2.0) with the issue's edge predictions"""
    pred = np.full((4, 5), 2.0, np.float32)
    pred[0, 0] = 0.0              # raw_disp = 1 / float32(1e-16)
    pred[0, 1] = 1e-20            # beside the 1e-16: another float32 sum, nearly the same depth
    pred[0, 2] = 1e30             # raw_disp 1e-30: disp = shift, negative depth -2
    pred[0, 3] = np.inf           # raw_disp 0: the same depth
    pred[0, 4] = np.nan
    pred[1, 0] = 4.0              # disp = 2 * 0.25 - 0.5 = 0 exactly: depth 1 / 1e-16
    pred[1, 1] = 8.0              # disp = -0.25: depth about -4
    pred[1, 2] = 3.9999998        # just below 4: a tiny positive disp, a huge depth
    pred[1, 3] = 4.0000005        # just above 4: a tiny negative disp, a huge negative depth
    return pred, np.array([[2.0, -0.5]])


def test_edge_values_in_one_view():
    f32max = float(np.finfo(np.float32).max)
    pred, ss = edge_view()
    want = numpy_depth(pred[None], ss)[0]
    raw0 = np.float32(1.0) / np.float32(1e-16)
    assert want[0, 0] == 1 / ((2.0 * np.float64(raw0) - 0.5) + 1e-16) and 0 < want[0, 0] < want[0, 1] < 1e-16
    assert want[0, 2] == want[0, 3] == 1 / (-0.5 + 1e-16) and want[0, 2] < 0
    assert np.isnan(want[0, 4]) and want[1, 0] == 1 / 1e-16 and want[1, 1] < 0 and want[1, 2] > 1e6 and want[1, 3] < -1e6
    # a negative shift: disp + 1e-16 is negative where raw_disp > 0 (scale -2) and exactly 0 where it is 0 (the inf
    # prediction), which gives inf
    ss_inf = np.array([[-2.0, -1e-16]])
    want_inf = numpy_depth(pred[None], ss_inf)[0]
    assert np.isposinf(want_inf[0, 3]) and want_inf[2, 2] < 0 and want_inf[0, 2] < -1e29 and np.isinf(want_inf).sum() == 1
    # A depth above the float32 maximum.  No finite float64 depth is: disp + 1e-16 is a float64 sum, so when it is not 0
    # it is at least the spacing of the doubles around 1e-16 (2^-106 = 1.2e-32), and the depth at most 8.2e31 < 3.4e38.  The
    # only depth the cast turns into inf is the float64 inf above.  The largest finite depth, one spacing from -1e-16:
    ss_big = np.array([[0.0, np.nextafter(-1e-16, 0.0)]])
    want_big = numpy_depth(pred[None], ss_big)[0]
    assert want_big[2, 2] == 2.0 ** 106 < f32max and np.isfinite(want_big.astype(np.float32)[2, 2])
    assert np.isposinf(want_inf.astype(np.float32)[0, 3])
    for s, w in ((ss, want), (ss_inf, want_inf), (ss_big, want_big)):
        got, _, _ = run_op(pred[None], s)
        assert same_bits(got[0].view(np.uint32), w.astype(np.float32).view(np.uint32)), (s, got[0], w)
    # on the range path the NaN pixel decides: (1e-16, 2e-16); without it, the negative depths clamp near only
    K, c2w = np.eye(4)[None], np.eye(4)[None]
    depth, rng32, nf = run_op(pred[None], ss, K, c2w, np.eye(4))
    assert same_bits(depth[0].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert nf.tolist() == [1e-16, 2e-16] and same_bits(nf, numpy_range(want[None], K, c2w, np.eye(4)))
    assert rng32.tolist() == [np.float32(1e-16), np.float32(2e-16)]
    clean = pred.copy()
    clean[0, 4] = 2.0
    want_c = numpy_depth(clean[None], ss)
    want_nf = numpy_range(want_c, K, c2w, np.eye(4))
    depth, rng32, nf = run_op(clean[None], ss, K, c2w, np.eye(4))
    assert same_bits(nf, want_nf) and same_bits(rng32, want_nf.astype(np.float32)) and want_nf[0] == 1e-16 < want_nf[1]
    assert same_bits(depth, want_c.astype(np.float32))


def test_conversion_only_call_writes_the_depth_and_nothing_else():
    """the three range arguments null: the same depth bits as the range path, in a buffer between guard words; more views
    than one launch carries scales for (64), and a one-pixel view, which only the range path rejects"""
    from pgdvs_amd import _lib, ops

    rng = np.random.default_rng(9)
    V, H, W = 3, 7, 13
    pred = rng.uniform(0.3, 6.0, (V, H, W)).astype(np.float32)
    ss = np.stack([rng.uniform(0.7, 1.4, V), rng.uniform(-0.03, 0.05, V)], 1)
    want = numpy_depth(pred, ss).astype(np.float32)
    Ks, c2ws, tgt = cameras(V, H, W, rng)
    assert same_bits(run_op(pred, ss, Ks, c2ws, tgt)[0], want) and same_bits(run_op(pred, ss)[0], want)
    n, guard = V * H * W, 64
    buf = torch.full((n + 2 * guard,), -7.25, dtype=torch.float32, device=DEV)
    p = torch.from_numpy(pred).to(DEV)
    ssv = (_lib.C.c_double * (2 * V))(*ss.reshape(-1).tolist())
    lib = _lib.load()
    rc = lib.pgdvs_nvidia_zoe_depth_range(p.data_ptr(), ssv, None, V, H, W, None, buf.data_ptr() + 4 * guard, None, None, None, 0,
                                          ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    out = buf.cpu().numpy()
    assert same_bits(out[guard:guard + n].reshape(V, H, W), want)
    assert (out[:guard] == -7.25).all() and (out[guard + n:] == -7.25).all()
    V2 = 70
    pred2 = rng.uniform(0.3, 6.0, (V2, 3, 5)).astype(np.float32)
    ss2 = np.stack([rng.uniform(0.7, 1.4, V2), rng.uniform(-0.03, 0.05, V2)], 1)
    assert same_bits(run_op(pred2, ss2)[0], numpy_depth(pred2, ss2).astype(np.float32))
    Ks2, c2ws2, tgt2 = cameras(V2, 3, 5, rng)
    d2, r2, nf2 = run_op(pred2, ss2, Ks2, c2ws2, tgt2)
    assert same_bits(d2, numpy_depth(pred2, ss2).astype(np.float32))
    assert same_bits(nf2, numpy_range(numpy_depth(pred2, ss2), Ks2, c2ws2, tgt2))
    assert same_bits(run_op(pred[:, :1, :1], ss)[0], want[:, :1, :1])


def test_argument_checks_raise_and_launch_nothing():
    from pgdvs_amd import _lib, ops

    one = torch.ones((2, 1, 1), device=DEV)
    with pytest.raises(ops.PgdvsHipError):  # H W == 1 on the range path (the workspace query refuses it first)
        ops.nvidia_zoe_depth(one, np.ones((2, 2)), torch.zeros(2, 12, device=DEV), np.eye(4))
    with pytest.raises(ops.PgdvsHipError):  # V = 0
        ops.nvidia_zoe_depth(torch.ones((0, 4, 4), device=DEV), np.ones((0, 2)))
    with pytest.raises(ops.PgdvsHipError):
        ops.nvidia_zoe_depth(torch.ones((0, 4, 4), device=DEV), np.ones((0, 2)), torch.zeros(0, 12, device=DEV), np.eye(4))
    with pytest.raises(ValueError):
        ops.nvidia_zoe_depth(torch.ones((2, 4, 4), device=DEV), np.ones((3, 2)))
    with pytest.raises(ValueError):
        ops.nvidia_zoe_depth(torch.ones((2, 4, 4), device=DEV), np.ones((2, 2)), torch.zeros(2, 12, device=DEV))
    lib = _lib.load()
    ssv = (_lib.C.c_double * 4)(1.0, 0.0, 1.0, 0.0)
    inv = (_lib.C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
    out = torch.full((8,), 3.5, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    rays = torch.zeros(2, 12, device=DEV)
    args = (one.data_ptr(), ssv, rays.data_ptr(), 2, 1, 1, inv, out.data_ptr(), out.data_ptr() + 16, None, ws.data_ptr(),
            ws.numel(), ops._stream())
    assert lib.pgdvs_nvidia_zoe_depth_range(*args) == -1  # PGDVS_ERR_INVALID, straight from the entry point
    assert lib.pgdvs_nvidia_zoe_depth_range_workspace_bytes(2, 1, 1) == lib.pgdvs_nvidia_zoe_depth_range_workspace_bytes(0, 4, 4) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 3.5).all() and not ws.any().item()
