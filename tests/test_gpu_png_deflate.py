"""The deflate of the PNG export on the MI355X (csrc/png_deflate.hip, ops.png_deflate, png.PngWriter(deflate="device")): the
stream equals png.deflate_rle byte for byte and decodes under zlib -- on the crafted buffers of the host test, with runs
across every boundary of the kernel's tiling, and for several images in one call; nothing is written past a stream's end, a
row that is too short stays untouched; the writer's and the loops' device mode leaves the same files with the same pixels,
and the defaults still leave today's bytes."""
import pathlib
import sys
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import eval_run_reference as ER  # noqa: E402
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402
import png_deflate_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


def _decode(path):
    with PIL.Image.open(path) as im:
        im.load()
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _check(raw, seg, slack=64):
    """raw [n,nbytes] uint8 -> every image's device stream equals the restatement, decodes, and nothing else of a pre-filled
    row is written"""
    from pgdvs_amd import ops, png

    raw = np.array(raw, dtype=np.uint8, order="C")  # (a writable copy: the shared buffers are read-only)
    n, size = raw.shape
    want = [png.deflate_rle(raw[i], seg) for i in range(n)]
    stride = ops.png_deflate_capacity(size, seg) + slack
    out = torch.full((n, stride), FILL, dtype=torch.uint8, device=DEV)
    data, nbytes = ops.png_deflate(torch.from_numpy(raw).to(DEV), seg, out=out)
    assert data.data_ptr() == out.data_ptr() and nbytes.dtype == torch.int32 and nbytes.is_cuda
    host, lens = data.cpu().numpy(), nbytes.cpu().tolist()
    for i in range(n):
        assert lens[i] == len(want[i]), (i, lens[i], len(want[i]))
        got = host[i, :lens[i]].tobytes()
        if got != want[i]:
            bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want[i], np.uint8))
            raise AssertionError((i, len(bad), bad[:8].tolist()))
        assert zlib.decompress(got) == raw[i].tobytes(), i
        assert (host[i, lens[i]:] == FILL).all(), (i, "bytes past the stream's end were written")
    return want


@pytest.mark.parametrize("seg", PC.SEGS)
@pytest.mark.parametrize("name", sorted(PC.buffers()))
def test_stream_equals_the_restatement(name, seg):
    _check(PC.buffers()[name][None], seg)


def _boundaries():
    from pgdvs_amd import ops

    P, per, window = ops.PNG_DEFLATE_PAYLOAD, ops.PNG_DEFLATE_PER, ops.PNG_DEFLATE_WINDOW
    wave = 64 * per
    # a thread's, a wavefront's and the step's edges in the first and the second step, the window's end, the segment's start
    return sorted({per, wave, 2 * wave, 3 * wave, P - per, P, P + per, P + wave, window, 2 * P, 4096, 4096 + P})


@pytest.mark.parametrize("boundary", _boundaries())
def test_runs_across_the_tiling(boundary):
    from pgdvs_amd import ops

    _check(PC.boundary_buffers(boundary, 4096 + 2 * ops.PNG_DEFLATE_PAYLOAD + 100, seed=boundary), 4096)


def test_three_images_of_different_content_in_one_call():
    size = 3 * 4096 + 1
    rng = np.random.default_rng(4)
    raw = np.stack([rng.integers(0, 256, size, dtype=np.uint8), np.zeros(size, np.uint8), np.repeat(rng.integers(0, 7, size // 5 + 1, dtype=np.uint8), 5)[:size]])
    want = _check(raw, 4096)
    assert len({len(w) for w in want}) == 3
    H, W = 37, 53  # [n,H,L] scanlines are the same call
    from pgdvs_amd import ops, png

    s = np.stack([PC.scanlines(k, H, W) for k in ("noise", "render", "zeros")])
    data, nbytes = ops.png_deflate(torch.from_numpy(s).to(DEV))
    for i in range(3):
        assert data[i, :int(nbytes[i])].cpu().numpy().tobytes() == png.deflate_rle(s[i], png.DEFLATE_SEG_DEFAULT)


def test_a_row_one_byte_too_short_stays_untouched():
    from pgdvs_amd import _lib, ops, png

    raw = np.stack([PC.buffers()["noise"][:20000], np.zeros(20000, np.uint8)])
    need = len(png.deflate_rle(raw[0], 4096))
    out = torch.full((2, need - 1), FILL, dtype=torch.uint8, device=DEV)
    data, nbytes = ops.png_deflate(torch.from_numpy(raw).to(DEV), 4096, out=out)
    host = data.cpu().numpy()
    assert nbytes.cpu().tolist() == [-1, len(png.deflate_rle(raw[1], 4096))]
    assert (host[0] == FILL).all()
    assert host[1, :int(nbytes[1])].tobytes() == png.deflate_rle(raw[1], 4096) and (host[1, int(nbytes[1]):] == FILL).all()
    out = torch.full((2, need), FILL, dtype=torch.uint8, device=DEV)  # exactly enough
    data, nbytes = ops.png_deflate(torch.from_numpy(raw).to(DEV), 4096, out=out)
    assert int(nbytes[0]) == need and data[0].cpu().numpy().tobytes() == png.deflate_rle(raw[0], 4096)
    # shapes outside the limits
    lib = _lib.load()
    for args in ((0, 100, 4096), (1, 0, 4096), (1, 100, 2048), (1, 100, 5000), (1, 100, 131072), (1, (1 << 30) + 1, 65536)):
        assert lib.pgdvs_png_deflate_workspace_bytes(*args) == -1, args
    with pytest.raises(ops.PgdvsHipError):
        ops.png_deflate(torch.from_numpy(raw))
    with pytest.raises(ValueError):
        ops.png_deflate(torch.from_numpy(raw).to(DEV), 1000)


@pytest.mark.parametrize("H,W", [(37, 53), (3, 2049), (288, 550)])
def test_device_writer_leaves_the_pixels_of_the_zlib_writer(tmp_path, H, W):
    from pgdvs_amd import ops, png

    x = torch.stack([torch.from_numpy(PC.render_image(H, W)), torch.from_numpy(PC.noise_image(H, W))]).permute(0, 3, 1, 2).float() / 255.0
    scan = ops.png_scanlines(x.to(DEV))
    for mode in ("zlib", "device"):
        with png.PngWriter(n_threads=2, deflate=mode, seg_bytes=4096) as w:
            w.submit(tmp_path / f"{mode}_0.png", scan[0])
            w.submit_batch([tmp_path / f"{mode}_b{i}.png" for i in range(2)], scan)
        assert w.files_written == 3
    host = scan.cpu().numpy()
    for i, name in ((0, "0"), (0, "b0"), (1, "b1")):
        assert (tmp_path / f"zlib_{name}.png").read_bytes() == png.encode(host[i], H, W)  # the default: today's bytes
        assert (tmp_path / f"device_{name}.png").read_bytes() == png.png_from_zstream(png.deflate_rle(host[i], 4096), H, W)
        assert np.array_equal(_decode(tmp_path / f"device_{name}.png"), _decode(tmp_path / f"zlib_{name}.png")), name
    assert png.PngWriter().deflate == "zlib"


def test_vis_loops_in_device_mode_write_the_same_files(tmp_path):
    """the nvidia_vis item of tests/test_gpu_vis.py"""
    from pgdvs_amd import harness, png
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    torch.manual_seed(0)
    cfg = load_config(engine="visualizer_pgdvs")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    real = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()

    class RenderedOnce:
        """the item goes through the renderer once; every loop below exports that one render (two forwards of the splatting
        path need not agree to the bit, and this test is about the export)"""
        training, ret = False, None

        def forward(self, data, **kw):
            if self.ret is None:
                RenderedOnce.ret = real.forward(data, **kw)
            return self.ret

    model = RenderedOnce()
    ds = NvidiaDynVisualizationDataset(data_root=VT.build_tree(tmp_path / "tree"), device=None, **VT.KW)
    batch = harness.collate([ds[10]])
    batch["static_noise"] = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, NT.H, NT.W)).astype(np.float32))
    files = {}
    for mode in ("zlib", "device"):
        with png.PngWriter(n_threads=2, deflate=mode) as w:
            files[mode] = harness.vis_step(model, batch, rc, tmp_path / mode, device=DEV, writer=w)
    assert "static_coarse_rgb" in model.ret and len(files["device"]) == 2
    assert [p.relative_to(tmp_path / "device") for p in files["device"]] == [p.relative_to(tmp_path / "zlib") for p in files["zlib"]]
    for a, b in zip(files["device"], files["zlib"]):
        pixels = _decode(b)
        assert np.array_equal(_decode(a), pixels), a
        H, W = pixels.shape[:2]
        assert b.read_bytes() == png.encode(png.filter_scanlines(pixels), H, W)  # the default: today's bytes
        assert a.read_bytes() == png.png_from_zstream(png.deflate_rle(png.filter_scanlines(pixels), png.DEFLATE_SEG_DEFAULT), H, W)

    class One:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {k: v[0] for k, v in batch.items()}

    for mode in ("zlib", "device"):
        dirs = harness.vis_run(model, One(), rc, tmp_path / f"run_{mode}", device=DEV, png_deflate=mode)
        assert sorted(p.name for d in dirs.values() for p in d.iterdir()) == sorted(p.name for p in files[mode])
        for a in files[mode]:
            assert (tmp_path / f"run_{mode}" / a.relative_to(tmp_path / mode)).read_bytes() == a.read_bytes(), (mode, a)
    with pytest.raises(ValueError):
        harness.vis_run(model, One(), rc, tmp_path / "bad", device=DEV, png_deflate="nonsense")


def test_eval_run_in_device_mode_gives_the_default_records_and_pixels(tmp_path):
    from pgdvs_amd import harness

    g = ER.load_fixture()
    res = {}
    for mode in ("zlib", "device"):
        res[mode] = harness.eval_run(ER.RecordedModel(with_geo=True, gnt=True), ER.Items(g), None, batch_size=2, device=DEV, save_individual=True,
                                     info_dir=tmp_path / mode / "info", vis_dir=tmp_path / mode / "vis", run_ahead=1, png_deflate=mode)
    assert res["device"]["records"] and len(res["device"]["records"]) == len(res["zlib"]["records"])
    for a, b in zip(res["device"]["records"], res["zlib"]["records"]):
        assert a["name"] == b["name"] and list(a["info"]) == list(b["info"])
        for k, v in a["info"].items():
            assert np.array_equal(np.asarray(v), np.asarray(b["info"][k])), (a["name"], k)
    names = ER.all_files(tmp_path / "zlib" / "vis")
    assert names and ER.all_files(tmp_path / "device" / "vis") == names
    for name in names:
        assert np.array_equal(_decode(tmp_path / "device" / "vis" / name), _decode(tmp_path / "zlib" / "vis" / name)), name
    with pytest.raises(ValueError):
        harness.eval_run(ER.RecordedModel(), ER.Items(g), None, png_deflate="nonsense")
