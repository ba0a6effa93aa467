"""The DyCheck loader's resident source frames on the MI355X (csrc/item_gather.hip, pgdvs_amd/datasets/dycheck_iphone.py):
``ops.item_target`` against the loader's two numpy statements bit for bit, over every byte value, aligned and unaligned
outputs, with and without a covisible image, with guard words around every output; its argument checks; the loader with
``resident=True`` on the device against the host disk path; a resident ``__getitem__`` that never waits for the device;
``harness.eval_run`` over resident items gives the disk items' sums and records."""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import dycheck_tree as DT  # noqa: E402
import test_dycheck_resident_host as RH  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0x5AA55AA5
SIZES = [(1, 1), (5, 7), (3, 4), (16, 16), (17, 19), (48, 64)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DT.build_tree(tmp_path_factory.mktemp("dycheck_resident_gpu"))


# ---------------------------------------------------------------------------- ops.item_target
def _image(H, W, seed):
    """colour bytes: channel c of pixel i holds (i + 85 c) % 256, so 256 pixels carry every value in every channel position"""
    i = np.arange(H * W).reshape(H, W)
    rgb = np.stack([(i + 85 * c) % 256 for c in range(3)], -1).astype(np.uint8)
    if H * W >= 256:
        assert all(len(np.unique(rgb[..., c])) == 256 for c in range(3))
    rng = np.random.default_rng(seed)
    masks = {"drawn": rng.choice(np.array([0, 1, 2, 128, 255], np.uint8), (H, W)), "zeros": np.zeros((H, W), np.uint8),
             "all 255": np.full((H, W), 255, np.uint8), "none": None}
    return rgb, masks


def _statements(rgb, cov):
    """the loader's host statements (dycheck_iphone.py, _process_view and __getitem__)"""
    return rgb.astype(np.float32) / 255.0, None if cov is None else (cov > 0).astype(np.float32)[..., None]


def _guarded(H, W, with_mask, shift):
    """the outputs as views of one guard-filled buffer, 4 words between neighbours, each ``shift`` words past a 16-byte boundary"""
    sizes = [H * W * 3] + ([H * W] if with_mask else [])
    starts, off = [], 4
    for s in sizes:
        starts.append(off + shift)
        off = -(-(off + shift + s + 4) // 4) * 4
    buf = torch.full((off + 4,), GUARD, dtype=torch.int32, device=DEV).view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    outs = [buf[a:a + s] for a, s in zip(starts, sizes)]
    out = (outs[0].view(H, W, 3), outs[1].view(H, W, 1) if with_mask else None)
    assert all(o is None or o.data_ptr() % 16 == 4 * shift for o in out)
    return buf, out, [(a, a + s) for a, s in zip(starts, sizes)]


@pytest.mark.parametrize("H,W", SIZES)
def test_item_target_equals_the_numpy_statements(H, W):
    from pgdvs_amd import ops

    rgb, masks = _image(H, W, seed=100 * H + W)
    rgb_d = torch.from_numpy(rgb).to(DEV)
    for kind, cov in masks.items():
        cov_d = None if cov is None else torch.from_numpy(cov).to(DEV)
        want_rgb, want_mask = _statements(rgb, cov)
        for shift in (0, 1):  # outputs at 16-byte boundaries, and 4 bytes past them: one pixel per lane for the whole image
            buf, out, spans = _guarded(H, W, cov is not None, shift)
            got = ops.item_target(rgb_d, cov_d, out=out)
            assert got[0] is out[0] and got[1] is out[1]
            host = buf.cpu().view(torch.int32).numpy()
            keep = np.ones(host.size, bool)
            for a, b in spans:
                keep[a:b] = False
            assert keep.sum() >= 8 and (host[keep] == GUARD).all(), (kind, shift, "a guard word was overwritten")
            for g, w, name in ((got[0], want_rgb, "rgb"), (got[1], want_mask, "mask")):
                if w is None:
                    assert g is None
                    continue
                g = g.cpu().numpy()
                assert g.shape == w.shape and g.dtype == np.float32
                bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
                assert bad.size == 0, (kind, shift, name, len(bad), bad[:4].tolist())
        # outputs the op allocates itself, and inputs 4 bytes into a larger buffer
        pad = torch.zeros(4 + rgb.size + 4 + H * W, dtype=torch.uint8, device=DEV)
        rgb_off = pad[4:4 + rgb.size].view(H, W, 3).copy_(rgb_d)
        cov_off = None if cov is None else pad[8 + rgb.size:].view(H, W).copy_(cov_d)
        for a, b in ((rgb_d, cov_d), (rgb_off, cov_off)):
            g_rgb, g_mask = ops.item_target(a, b)
            assert g_rgb.is_cuda and np.array_equal(g_rgb.cpu().numpy().view(np.int32), want_rgb.view(np.int32)), kind
            assert (g_mask is None) == (cov is None)
            if cov is not None:
                assert g_mask.shape == (H, W, 1) and np.array_equal(g_mask.cpu().numpy().view(np.int32), want_mask.view(np.int32)), kind


def test_the_division_is_not_a_multiplication():
    """byte / 255 differs from byte * (1 / 255) at 126 byte values; the kernel gives the division's"""
    from pgdvs_amd import ops

    b = np.arange(256, dtype=np.uint8)
    div, mul = b.astype(np.float32) / np.float32(255.0), b.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    differ = np.flatnonzero(div != mul)
    assert len(differ) == 126
    img = np.repeat(b.reshape(16, 16, 1), 3, axis=2)
    got = ops.item_target(torch.from_numpy(np.ascontiguousarray(img)).to(DEV))[0].cpu().numpy()[..., 0].reshape(-1)
    assert np.array_equal(got.view(np.int32), div.view(np.int32))
    assert (got[differ] != mul[differ]).all()


def test_item_target_argument_checks():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    rgb = torch.zeros(5, 7, 3, dtype=torch.uint8, device=DEV)
    cov = torch.zeros(5, 7, dtype=torch.uint8, device=DEV)
    guard = torch.full((5 * 7 * 4,), GUARD, dtype=torch.int32, device=DEV)
    out_rgb, out_mask = guard[:105].view(torch.float32).view(5, 7, 3), guard[105:].view(torch.float32).view(5, 7, 1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for args, what in (((p(rgb), p(cov), 0, 7, p(out_rgb), p(out_mask), None), b"bad shape"),
                       ((p(rgb), p(cov), 5, 1 << 20, p(out_rgb), p(out_mask), None), b"bad shape"),
                       ((None, p(cov), 5, 7, p(out_rgb), p(out_mask), None), b"null pointer"),
                       ((p(rgb), p(cov), 5, 7, None, p(out_mask), None), b"null pointer"),
                       ((p(rgb), p(cov), 5, 7, p(out_rgb), None, None), b"mask_out"),
                       ((p(rgb), None, 5, 7, p(out_rgb), p(out_mask), None), b"covisible")):
        assert lib.pgdvs_item_target(*args) == -1, what
        assert what in lib.pgdvs_last_error(), (what, lib.pgdvs_last_error())
    with pytest.raises(ValueError):
        ops.item_target(rgb, cov, out=(out_rgb, None))  # covisible without its output
    with pytest.raises(ValueError):
        ops.item_target(rgb, cov, out=(out_rgb.view(7, 5, 3), out_mask))  # a misshapen out
    with pytest.raises(ValueError):
        ops.item_target(rgb, cov, out=(out_rgb, out_mask.view(5, 7)))
    with pytest.raises(ValueError):
        ops.item_target(rgb, cov.view(7, 5))
    with pytest.raises(ValueError):
        ops.item_target(rgb.float(), cov)
    with pytest.raises(ops.PgdvsHipError):
        ops.item_target(rgb.cpu(), None)
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == GUARD).all()  # nothing was launched


# ---------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("typ", RH.TYPES)
def test_device_store_equals_the_host_disk_path(tree, typ):
    disk, res = RH.make(tree, typ, device=None), RH.make(tree, typ, device=DEV, resident=True)
    assert res.store.device == torch.device(DEV)
    raised = RH.compare_all(res, disk, typ, on_device=True)
    assert (raised > 0) == (typ == "clustered")
    assert 0 < res.store.stats["frames_decoded"] <= len(DT.TRAIN_T)


def test_unusual_target_files_take_the_host_statements(tmp_path):
    """a covisible image with three channels is no [H,W] byte image: its float entry rides in the packed copy, the colour
    still crosses as bytes"""
    import PIL.Image

    root = DT.build_tree(tmp_path)
    sd = root / "iphone" / DT.SCENE
    cam, t = DT.VAL[0]
    f = sd / f"covisible/{DT.FACTOR}x/val" / f"{DT.frame_name(cam, t)}.png"
    PIL.Image.fromarray(np.repeat(np.array(PIL.Image.open(f))[..., None], 3, axis=2)).save(f)
    disk, res = RH.make(root, device=None), RH.make(root, device=DEV, resident=True)
    idx = [i for i, e in enumerate(res.valid_fs) if (int(e[3]), int(e[2])) == (cam, t)][0]
    want, got = disk[idx], res[idx]
    assert want["eval_mask"].shape == (DT.H, DT.W, 3, 1) and got["eval_mask"].is_cuda and got["rgb_tgt"].is_cuda
    RH.assert_items_identical(got, want, "three-channel covisible")


def test_a_resident_item_never_waits_for_the_device(tree, monkeypatch):
    res = RH.make(tree, device=DEV, resident=True)
    first = [res[i] for i in range(len(res))]
    torch.cuda.synchronize()

    def refuse(*a, **kw):
        raise AssertionError("a resident __getitem__ waited for the device")

    with monkeypatch.context() as m:
        for owner, attr in ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
                            (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
            m.setattr(owner, attr, refuse)
        second = [res[i] for i in range(len(res))]
    for a, b in zip(first, second):
        RH.assert_items_identical(b, a, "second pass")
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()) if isinstance(x, torch.Tensor))


# ---------------------------------------------------------------------------- end to end
def test_eval_run_over_resident_items_equals_the_disk_items(tree):
    """harness.eval_run(quant_type="dycheck_iphone", run_ahead=2) over the 8 closest_wo_temporal items with the small seeded GNT
    of tests/test_gpu_dycheck_dataset.py, one model object: count, sums and every record's values are equal bits.
    The dynamic branch renders the mesh, as in tests/test_gpu_resident.py: the default splat accumulates with float atomics,
    so two runs over the SAME disk loader differ (measured on this arrangement: eval/psnr_combined sums of 53.41043, 53.41250
    and 53.41042 from three disk runs, 53.41045 and 53.41090 from two resident ones), and no loader could be held to equal
    bits through it.  The convolutions of the GNT feature network run with ``cudnn.deterministic`` (and no benchmarking), as
    there: without it the records of views 0, 1 and 4 each moved between two values from one run to the next of either
    loader (psnr sums 53.092957, 53.092964, 53.092972).  With both, runs over disk and resident items in either order, with
    ``run_ahead`` 0 and 2, gave one set of bits."""
    from pgdvs_amd import harness
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    torch.manual_seed(0)
    cfg = load_config(static_renderer="gnt")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    rc.dyn_render_type = "mesh"
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    runs, flags = {}, (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for kind, resident in (("disk", False), ("resident", True)):
            ds = RH.make(tree, "closest_wo_temporal", device=DEV, resident=resident)
            assert len(ds) == 8
            runs[kind] = harness.eval_run(model, ds, rc, device=DEV, quant_type="dycheck_iphone", run_ahead=2)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    a, b = runs["disk"], runs["resident"]
    print({k: (a["sums"][k], b["sums"][k]) for k in a["sums"]})
    assert a["eval/count"] == b["eval/count"] == 8
    assert a["sums"].keys() == b["sums"].keys() and len(a["sums"]) > 1
    f64 = lambda x: np.float64(x).view(np.uint64)  # noqa: E731
    for k in a["sums"]:
        assert f64(a["sums"][k]) == f64(b["sums"][k]), (k, a["sums"][k], b["sums"][k])
    assert len(a["records"]) == len(b["records"]) == 8
    for ra, rb in zip(a["records"], b["records"]):
        assert ra["name"] == rb["name"] and list(ra["info"]) == list(rb["info"])
        for k, v in ra["info"].items():
            if isinstance(v, np.ndarray):
                assert v.dtype == rb["info"][k].dtype and np.array_equal(v, rb["info"][k]), (ra["name"], k)
            else:
                assert f64(v) == f64(rb["info"][k]), (ra["name"], k, v, rb["info"][k])
