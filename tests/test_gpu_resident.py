"""The resident source frames on the MI355X (csrc/item_gather.hip, pgdvs_amd/datasets/resident.py): ``ops.item_views`` against
its statement bit for bit, over every byte value, special depths, repeated ids, groups without depth and odd sizes, with
canaries around every output; ``ops.flow_occ`` against numpy at the threshold's edges; the four loaders with
``resident=True`` on the device against their disk paths; ``harness.vis_run`` over resident items writes the disk items'
files."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import resident_cases as RC  # noqa: E402
from resident_cases import NT, VT  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0x5AA55AA5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("resident_gpu"))


# ---------------------------------------------------------------------------- ops.item_views
SPECIAL_DEPTHS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc12345, 0xffa00001,
                           0x3f800000, 0x7f7fffff], dtype=np.uint32).view(np.float32)


def _padded(frames):
    """[F, ...] host array -> the store's table on the device: every frame in a slot padded to 16 bytes"""
    t = torch.from_numpy(np.ascontiguousarray(frames))
    F, per = t.shape[0], t[0].numel()
    slot = -(-per * t.element_size() // 16) * 16 // t.element_size()
    tab = torch.zeros((F, slot), dtype=t.dtype, device=DEV)
    view = tab[:, :per].view(t.shape)
    view.copy_(t)
    return view


def _store(F, H, W, mask_kind, seed):
    rng = np.random.default_rng(seed)
    n = H * W
    # every byte value in every channel as far as the pixels reach: channel c of pixel i of frame f holds (i + 85 c + 37 f) % 256
    i = np.arange(n).reshape(H, W)
    rgb = np.stack([np.stack([(i + 85 * c + 37 * f) % 256 for c in range(3)], -1) for f in range(F)]).astype(np.uint8)
    if n >= 256:
        assert all(len(np.unique(rgb[f, ..., c])) == 256 for f in range(F) for c in range(3))
    mask = {"zeros": np.zeros((F, H, W), np.uint8), "ones": np.ones((F, H, W), np.uint8),
            "mixed": rng.integers(0, 2, (F, H, W)).astype(np.uint8)}[mask_kind]
    depth = rng.uniform(0.5, 9.0, (F, H, W)).astype(np.float32)
    flat = depth.reshape(-1)
    where = rng.permutation(flat.size)[:len(SPECIAL_DEPTHS)]
    flat[where] = SPECIAL_DEPTHS[:len(where)]
    return rgb, mask, depth


def _statement(rgb, mask, depth, ids, with_depth):
    """the loaders' statement on the host.  The division is numpy's: a true float32 division"""
    x = rgb[ids].astype(np.float32) / 255.0
    m = mask[ids].astype(np.float32)
    out = {"rgb": x, "dyn_mask": m[..., None], "dyn_rgb": x * m[..., None], "static_rgb": x * (1 - m[..., None])}
    if with_depth:
        out["depth"] = depth[ids][..., None]
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def _id_lists(F):
    rng = np.random.default_rng(F)
    many = rng.integers(0, F, 64).tolist()
    return {
        "one view": [([F - 1], True)],
        "reversed": [(list(range(F))[::-1], True)],
        "repeats": [([2, 2, 0, 2] if F > 2 else [0, 0, 0, 0], True)],
        "64 views in four groups": [(many[:1], True), (many[1:31], False), (many[31:44], True), (many[44:], True)],
        "a group without depth": [([0, F - 1], False), ([F - 1], True)],
    }


def _carve(groups, H, W, gap):
    """the groups' outputs carved out of one canary-filled buffer, ``gap`` floats between neighbours"""
    chans = {"rgb": 3, "dyn_mask": 1, "dyn_rgb": 3, "static_rgb": 3, "depth": 1}
    sizes = [(g, k, len(ids) * H * W * c) for g, (ids, with_depth) in enumerate(groups) for k, c in chans.items()
             if k != "depth" or with_depth]
    buf = torch.full((sum(s for _, _, s in sizes) + gap * (len(sizes) + 1),), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    out, spans, off = [dict() for _ in groups], [], gap
    for g, k, s in sizes:
        out[g][k] = buf[off:off + s].view(len(groups[g][0]), H, W, chans[k])
        spans.append((off, off + s))
        off += s + gap
    return buf, out, spans


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (3, 4), (17, 19), (288, 36)])  # 35 and 323 pixels: a tail of 3, unaligned views
def test_item_views_equal_the_statement(H, W, F):
    from pgdvs_amd import ops

    for mask_kind in ("zeros", "ones", "mixed"):
        rgb, mask, depth = _store(F, H, W, mask_kind, seed=1000 * H + 10 * W + F)
        tabs = _padded(rgb), _padded(mask), _padded(depth)
        for what, groups in _id_lists(F).items():
            for gap in (4, 5):  # outputs at 16-byte boundaries (where H W allows) and off them
                buf, out, spans = _carve(groups, H, W, gap)
                ret = ops.item_views(*tabs, groups, out=out)
                assert ret is out
                host = buf.cpu().view(torch.int32).numpy()
                keep = np.ones(host.size, bool)
                for a, b in spans:
                    keep[a:b] = False
                assert (host[keep] == CANARY).all(), (what, mask_kind, gap, "a canary was overwritten")
                for (ids, with_depth), o in zip(groups, out):
                    want = _statement(rgb, mask, depth, ids, with_depth)
                    assert set(o) == set(want), (what, sorted(o))
                    for k, w in want.items():
                        got = o[k].cpu()
                        assert got.shape == w.shape and got.dtype == torch.float32
                        bad = np.argwhere(got.numpy().view(np.int32) != w.numpy().view(np.int32))
                        assert bad.size == 0, (what, mask_kind, gap, k, len(bad), bad[:4].tolist())
    # outputs the op allocates itself
    groups = _id_lists(F)["64 views in four groups"]
    for (ids, with_depth), o in zip(groups, ops.item_views(*tabs, groups)):
        for k, w in _statement(rgb, mask, depth, ids, with_depth).items():
            assert o[k].is_cuda and np.array_equal(o[k].cpu().numpy().view(np.int32), w.numpy().view(np.int32)), k
        assert ("depth" in o) == with_depth


def test_the_division_is_not_a_multiplication():
    """the statement the kernel is held to differs from byte * (1 / 255) at 126 byte values: the all-values image pins it"""
    b = np.arange(256, dtype=np.float32)
    assert int((b / np.float32(255.0) != b * (np.float32(1.0) / np.float32(255.0))).sum()) == 126


def test_item_views_argument_checks():
    from pgdvs_amd import ops

    rgb, mask, depth = _store(3, 5, 7, "mixed", 1)
    tabs = _padded(rgb), _padded(mask), _padded(depth)
    with pytest.raises(ValueError):
        ops.item_views(*tabs, [([3], True)])  # no such frame
    with pytest.raises(ValueError):
        ops.item_views(*tabs, [([0], True)] * 5)  # five groups
    with pytest.raises(ValueError):
        ops.item_views(*tabs, [(list(range(3)) * 22, True)])  # 66 views
    with pytest.raises(ValueError):
        ops.item_views(*tabs, [([], True)])
    with pytest.raises(ValueError):  # frames 105 bytes apart: the slots are not padded
        ops.item_views(torch.from_numpy(rgb).to(DEV), tabs[1], tabs[2], [([0], True)])
    with pytest.raises(ValueError):
        ops.item_views(tabs[0], tabs[1], tabs[2].double(), [([0], True)])
    with pytest.raises(ops.PgdvsHipError):
        ops.item_views(tabs[0].cpu(), tabs[1], tabs[2], [([0], True)])


# ---------------------------------------------------------------------------- ops.flow_occ
@pytest.mark.parametrize("thres", [1.0, 0.0])
@pytest.mark.parametrize("H,W", [(5, 7), (288, 36)])
def test_flow_occ_equals_numpy(H, W, thres):
    from pgdvs_amd import ops

    rng = np.random.default_rng(H + W)
    cd = rng.normal(0, 0.6, (H, W, 2)).astype(np.float32)
    one, half = np.float32(1.0), np.float32(0.5)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    tiny = np.float32(1e-45)
    edges = [(0.25, 0.75), (1.0, 0.0), (-0.5, 0.5), (-1.0, -0.0), (up, 0.0), (down, 0.0), (0.0, -up), (-down, 0.0),
             (half, np.nextafter(half, one)), (half, np.nextafter(half, np.float32(0))), (-3.0, -4.0), (np.nan, 0.0), (0.0, np.nan),
             (np.nan, np.inf), (np.inf, 0.0), (-np.inf, 2.0), (0.0, 0.0), (-0.0, 0.0), (tiny, 0.0), (0.0, -tiny)]
    flat = cd.reshape(-1, 2)
    flat[rng.permutation(len(flat))[:len(edges)]] = np.array(edges, dtype=np.float32)
    want = (np.sum(np.abs(cd), axis=2) > thres).astype(np.float32)  # datasets._common.read_flow_npz
    assert 0 < want.sum() < want.size
    got = ops.flow_occ(torch.from_numpy(cd).to(DEV), thres)
    assert got.shape == (H, W) and got.dtype == torch.float32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), np.argwhere(got.cpu().numpy() != want)[:4].tolist()
    with pytest.raises(TypeError):
        ops.flow_occ(torch.from_numpy(cd).to(DEV), np.float64(thres))


# ---------------------------------------------------------------------------- the loaders
@pytest.mark.parametrize("name", RC.LOADERS)
def test_resident_loaders_on_the_device(name, trees):
    disk, res = RC.make(name, trees, device=DEV), RC.make(name, trees, device=DEV, resident=True)
    assert res.store.device == torch.device(DEV)
    for i in range(len(disk)):
        got = res[i]
        assert all(v.is_cuda for v in got.values() if isinstance(v, torch.Tensor)), [k for k, v in got.items()
                                                                                     if isinstance(v, torch.Tensor) and not v.is_cuda]
        RC.assert_items_equal(got, disk[i], (name, i))
    assert res.store.stats["frames_decoded"] == (NT.MF if name == "mono_vis" else NT.F)


@pytest.mark.parametrize("name", ["nvidia_vis", "mono_vis", "nvidia_eval"])
def test_a_resident_item_never_waits_for_the_device(name, trees, monkeypatch):
    res = RC.make(name, trees, device=DEV, resident=True)
    first = [res[i] for i in range(0, len(res), 5)]
    torch.cuda.synchronize()

    def refuse(*a, **kw):
        raise AssertionError("a resident __getitem__ waited for the device")

    with monkeypatch.context() as m:
        for owner, attr in ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
                            (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
            m.setattr(owner, attr, refuse)
        second = [res[i] for i in range(0, len(res), 5)]
    for a, b in zip(first, second):
        RC.assert_items_equal(b, a, name)
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()) if isinstance(x, torch.Tensor))


# ---------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["nvidia_vis", "mono_vis"])
def test_vis_run_writes_the_disk_items_files(name, trees, tmp_path):
    """harness.vis_run over four views, the renderer as tests/test_gpu_vis.py sets it up (the visualiser config, a seeded GNT
    of depth 2) but for the dynamic branch, which renders the mesh: the default splat accumulates with float atomics, so two
    forwards of ONE item differ in the last bits (tests/test_gpu_nvidia_vis.py) and could not be held to equal file bytes"""
    from pgdvs_amd import harness
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    torch.manual_seed(0)
    cfg = load_config(engine="visualizer_pgdvs")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    rc.dyn_render_type = "mesh"
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False

    class Four(torch.utils.data.Dataset):
        def __init__(self, ds):
            self.ds = ds

        def __len__(self):
            return len(VT.ITEMS)

        def __getitem__(self, i):
            return self.ds[VT.ITEMS[i]]

    files = {}
    for kind, resident in (("warm", False), ("disk", False), ("resident", True)):  # (the first run picks convolution algorithms)
        ds = RC.make(name, trees, device=DEV, resident=resident)
        dirs = harness.vis_run(model, Four(ds), rc, tmp_path / kind, device=DEV)
        files[kind] = {p.relative_to(tmp_path / kind): p.read_bytes() for d in dirs.values() for p in sorted(d.iterdir())}
    assert len(files["disk"]) == 2 * len(VT.ITEMS) and files["resident"].keys() == files["disk"].keys()
    for rel, data in files["disk"].items():
        assert files["resident"][rel] == data, rel
