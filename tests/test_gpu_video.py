"""The visualiser's video on the MI355X (csrc/jpeg.hip, ops.jpeg_*, video.MjpegWriter, harness.vis_step with ``video``): the
HIP coefficients equal the host restatement bit for bit, the HIP entropy coder equals ``video.encode_scan`` byte for byte on
crafted coefficients and on noise at every position of a restart boundary against the 256-block groups, nothing past a
frame's length is written, whole frames equal the host's files and decode with PIL, and an nvidia_vis item goes through
PGDVSRenderer and vis_step to an AVI whose frame is the host encoding of ``ret["combined_rgb"]``."""
import pathlib
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402
import video_reference as R  # noqa: E402
import vis_reference as VR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


# (16, 520): 65 MCUs in a row, one more than a wavefront; (288, 550): the datasets' frame
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (8, 8), (9, 17), (37, 53), (16, 520), (288, 550)])
def test_jpeg_coefficients_equal_the_host_restatement(H, W, B):
    from pgdvs_amd import ops

    for name, x in R.float_inputs(B, H, W):
        xd = x.to(DEV)
        for quality in (50, 100):
            got = ops.jpeg_coefficients(xd, quality)
            assert got.shape == (B, (H + 7) // 8, (W + 7) // 8, 3, 64) and got.dtype == torch.int16 and got.is_cuda
            want = R.host_coef(x, quality)
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, (name, quality, len(bad), bad[:4].tolist())
    one = ops.jpeg_coefficients(xd[0], 50)  # [3,H,W] is a batch of one
    assert np.array_equal(one.cpu().numpy(), R.host_coef(x[:1], 50))


def _scan_cases(nby, nbx):
    from pgdvs_amd import video

    yield "crafted", R.crafted_grid(nby, nbx, seed=nby * 100 + nbx)
    noise = np.random.default_rng(nby + nbx).integers(0, 256, (8 * nby, 8 * nbx, 3)).astype(np.uint8)
    yield "noise_q100", video.jpeg_coefficients(noise, 100)


# restart intervals: every MCU, a partial last segment, 64 and 65 (segments of 192 and 195 blocks: under one group of 256
# blocks), one row, two rows of 65 (390 blocks: two groups, a carry of bits between them), more than the frame holds
@pytest.mark.parametrize("nby,nbx", [(1, 1), (3, 5), (2, 65)])
def test_jpeg_scan_equals_the_host_coder(nby, nbx):
    from pgdvs_amd import ops, video

    restarts = sorted({1, 4, 64, 65, nbx, 2 * nbx, nby * nbx + 7})
    for name, coef in _scan_cases(nby, nbx):
        batch = np.stack([coef, coef[::-1, ::-1].copy()])  # B = 2: frames of different lengths
        dev = torch.from_numpy(batch).to(DEV)
        for restart in restarts + [None]:
            cap = ops.jpeg_scan_capacity(nby, nbx, nbx if restart is None else restart)
            stride = cap + 13  # a stride above the capacity, and odd
            out = torch.full((2, stride), 0xA5, dtype=torch.uint8, device=DEV)
            ret, nbytes = ops.jpeg_scan(dev, restart, out=out)
            assert ret.data_ptr() == out.data_ptr() and nbytes.dtype == torch.int32 and nbytes.shape == (2,)
            host, n = out.cpu().numpy(), nbytes.cpu().tolist()
            for b in range(2):
                want = video.encode_scan(batch[b], restart)
                assert n[b] == len(want), (name, restart, b, n[b], len(want))
                got = host[b, :n[b]].tobytes()
                if got != want:
                    first = next(i for i in range(len(want)) if got[i] != want[i])
                    raise AssertionError((name, restart, b, "first difference at byte", first, got[first:first + 8].hex(), want[first:first + 8].hex()))
                assert (host[b, n[b]:] == 0xA5).all(), (name, restart, b, "bytes past the frame's length were written")
    fresh, nb = ops.jpeg_scan(dev[0], 4)  # [nby,nbx,3,64] is a batch of one; out allocated at the capacity
    assert fresh.shape == (1, ops.jpeg_scan_capacity(nby, nbx, 4)) and fresh[0, :int(nb[0])].cpu().numpy().tobytes() == video.encode_scan(batch[0], 4)


def test_jpeg_scan_arguments():
    from pgdvs_amd import _lib, ops

    coef = torch.zeros((1, 2, 3, 3, 64), dtype=torch.int16, device=DEV)
    with pytest.raises(_lib.PgdvsHipError, match="host-only"):
        ops.jpeg_scan(coef, 0)  # no restart markers: the device pass needs byte-aligned segments
    lib = _lib.load()
    ws = torch.empty(lib.pgdvs_jpeg_scan_workspace_bytes(1, 2, 3, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty(ops.jpeg_scan_capacity(2, 3, 3), dtype=torch.uint8, device=DEV)
    nb = torch.empty(1, dtype=torch.int32, device=DEV)

    def call(restart=3, stride=out.numel(), ws_bytes=ws.numel(), nby=2):
        return lib.pgdvs_jpeg_scan(coef.data_ptr(), 1, nby, 3, restart, out.data_ptr(), stride, nb.data_ptr(), ws.data_ptr(), ws_bytes, None)

    assert call() == 0
    assert call(restart=0) == -1 and b"host-only" in lib.pgdvs_last_error()
    assert call(restart=65536) == -1
    assert call(stride=out.numel() - 1) == -1 and b"out_stride" in lib.pgdvs_last_error()
    assert call(ws_bytes=ws.numel() - 1) == -1
    assert call(nby=0) == -1
    with pytest.raises(ValueError):
        ops.jpeg_scan(coef.float())
    with pytest.raises(ValueError):
        ops.jpeg_scan(coef, 3, out=torch.empty((1, 5), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.jpeg_coefficients(torch.zeros((1, 4, 8, 8), device=DEV))
    with pytest.raises(ValueError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8), device=DEV), quality=0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(37, 53), (288, 550)])
def test_jpeg_encode_gives_the_host_files(H, W):
    from pgdvs_amd import ops, video

    for name, x in R.float_inputs(2, H, W):
        if name == "table":
            continue
        for quality, restart in ((90, None), (50, 7)):
            data, nbytes = ops.jpeg_encode(x.to(DEV), quality, restart)
            host, n = data.cpu().numpy(), nbytes.cpu().tolist()
            for b in range(2):
                got = video.jpeg_frame(host[b, :n[b]].tobytes(), H, W, quality, restart)
                assert got == video.encode_jpeg(x[b], quality, restart), (name, quality, restart, b)
                mode, size, pix = R.decode_pil(got)
                assert mode == "RGB" and size == (W, H)


def test_vis_step_video_on_an_nvidia_vis_item(tmp_path):
    """set up as test_gpu_vis.test_vis_step_on_an_nvidia_vis_item: the visualiser config, a seeded GNT of depth 2"""
    from pgdvs_amd import harness, png, video
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    torch.manual_seed(0)
    cfg = load_config(engine="visualizer_pgdvs")
    cfg.static_renderer.model_cfg.transformer_depth = 2
    rc = cfg.engine.engine_cfg.render_cfg
    rc.n_coarse_samples_per_ray = 16
    rc.chunk_size = 1024
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    ds = NvidiaDynVisualizationDataset(data_root=VT.build_tree(tmp_path / "tree"), device=None, **VT.KW)
    item = ds[10]
    batch = harness.collate([item])
    batch["static_noise"] = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, NT.H, NT.W)).astype(np.float32))
    plain = harness.vis_step(model, batch, rc, tmp_path / "plain", device=DEV)
    with video.MjpegWriter(n_threads=2) as w:
        paths, ret = harness.vis_step(model, batch, rc, tmp_path / "video", device=DEV, video=w, return_ret=True)
    split_dir = tmp_path / "video" / item["misc"].get("split", "")
    avi = split_dir / f"{item['misc']['scene_id']}_combined.avi"
    assert w.files == [avi] and avi.exists()
    frames = R.avi_file_frames(avi)
    img = ret["combined_rgb"].cpu()
    assert frames == [video.encode_jpeg(img[0], 90)]
    # PIL decodes the frame to the decode model of the coefficients of the PNG's pixels, within the bound of the host tests
    mode, size, pix = R.decode_pil(frames[0])
    q8 = VR.expected_save_image(img[0]).permute(1, 2, 0).numpy()
    model = R.decode_model(video.jpeg_coefficients(q8, 90), *video.quant_tables(90), NT.H, NT.W)
    assert size == (NT.W, NT.H) and np.abs(pix - model).max() <= 3
    # the PNG beside it has the bytes it has without the video: the host path's file of the same ``ret`` (a second forward
    # is no yardstick: the GNT's sums are not ordered from run to run)
    assert [p.relative_to(tmp_path / "video") for p in paths] == [p.relative_to(tmp_path / "plain") for p in plain]
    assert paths[0].name.endswith("_combined.png")
    assert paths[0].read_bytes() == png.encode(png.filter_scanlines(q8), NT.H, NT.W)
    assert sorted(p.name for p in split_dir.iterdir()) == sorted([item["misc"]["scene_id"], avi.name])


def test_vis_step_video_with_three_views_in_a_step(tmp_path):
    from pgdvs_amd import harness, video

    ds = VR.StubDataset(3, 37, 53, scenes=("scene_a", "scene_b"))
    batch = harness.collate([ds[i] for i in (2, 1, 0)])  # tgt_idx 7, 4, 1: the file sorts them
    with video.MjpegWriter(quality=75, restart_mcus=3) as w:
        harness.vis_step(VR.StubModel(), batch, None, tmp_path, device=DEV, video=w)
    assert sorted(p.name for p in w.files) == ["scene_a_combined.avi", "scene_b_combined.avi"]
    assert R.avi_file_frames(tmp_path / "scene_a_combined.avi") == [video.encode_jpeg(ds[i]["img"], 75, 3) for i in (0, 2)]
    assert R.avi_file_frames(tmp_path / "scene_b_combined.avi") == [video.encode_jpeg(ds[1]["img"], 75, 3)]
    w = video.MjpegWriter(restart_mcus=0)  # host-only: the GPU path refuses it when the frame is submitted
    with pytest.raises(Exception, match="host-only"):
        harness.vis_step(VR.StubModel(), batch, None, tmp_path / "no", device=DEV, video=w)
    w.close()


def test_vis_run_video_on_the_gpu(tmp_path):
    """the loop end to end on the device path: every frame is the host encoding of its view and decodes, within the bound of
    the host tests, to the decode model of the pixels its *_combined.png holds"""
    import PIL.Image

    from pgdvs_amd import harness, video

    ds = VR.StubDataset(5, 37, 53, scenes=("scene_a", "scene_b"))
    dirs = harness.vis_run(VR.StubModel(), ds, None, tmp_path, batch_size=2, device=DEV, video=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["scene_a", "scene_a_combined.avi", "scene_b", "scene_b_combined.avi"]
    for scene in ("scene_a", "scene_b"):
        items = [it for it in ds.items if it["misc"]["scene_id"] == scene]
        frames = R.avi_file_frames(tmp_path / f"{scene}_combined.avi")
        assert frames == [video.encode_jpeg(it["img"], 90) for it in items]
        for f, it in zip(frames, items):
            with PIL.Image.open(dirs[scene] / f"{it['misc']['tgt_idx']:05d}_combined.png") as im:
                q8 = np.asarray(im).copy()
            model = R.decode_model(video.jpeg_coefficients(q8, 90), *video.quant_tables(90), 37, 53)
            assert np.abs(R.decode_pil(f)[2] - model).max() <= 3


def test_1080p_once():
    """coefficients against the host's for a noise and a render frame at quality 90; the device stream's length and CRC
    against the host coder's, which runs once, on the render frame (about a second); for noise its top 64 rows only"""
    from pgdvs_amd import ops, synth, video

    H, W = 1080, 1920
    noise = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(9))
    render = torch.from_numpy(np.ascontiguousarray(synth.make_video(1, H, W, seed=5)["rgbs"])).permute(0, 3, 1, 2).contiguous()
    x = torch.cat([noise, render])
    coef = ops.jpeg_coefficients(x.to(DEV), 90)
    want = R.host_coef(x, 90)
    assert np.array_equal(coef.cpu().numpy(), want)
    data, nbytes = ops.jpeg_scan(coef)
    n = nbytes.cpu().tolist()
    host_render = video.encode_scan(want[1])
    assert n[1] == len(host_render)
    assert zlib.crc32(data[1, :n[1]].cpu().numpy().tobytes()) == zlib.crc32(host_render)
    top, n_top = ops.jpeg_scan(coef[0, :8].contiguous())
    host_top = video.encode_scan(want[0, :8])
    assert int(n_top[0]) == len(host_top) and top[0, :len(host_top)].cpu().numpy().tobytes() == host_top
    # one row per restart: the top eight rows of the frame are the first bytes of its stream, up to the marker behind them
    assert data[0, :len(host_top)].cpu().numpy().tobytes() == host_top and n[0] > len(host_top)
    mode, size, pix = R.decode_pil(video.jpeg_frame(data[1, :n[1]].cpu().numpy().tobytes(), H, W, 90))
    assert size == (W, H)
