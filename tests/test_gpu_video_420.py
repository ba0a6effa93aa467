"""The visualiser's video at 4:2:0 on the MI355X (csrc/jpeg.hip's 4:2:0 coefficient kernel and six-block entropy coder,
ops.jpeg_* with ``subsampling="4:2:0"``, video.MjpegWriter and harness.vis_step with a 4:2:0 writer): the HIP coefficients
equal the host restatement bit for bit at every edge case of libjpeg's rules (dummy columns and rows, the replicated
downsampled chroma row), the entropy coder equals ``video.encode_scan`` byte for byte with restart boundaries either side
of a 256-block group, nothing past a frame's length is written, whole frames equal the host's files and decode with PIL,
and an nvidia_vis item goes through PGDVSRenderer and vis_step to an AVI whose frame is the host encoding of
``ret["combined_rgb"]``."""
import pathlib
import sys

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
S420 = "4:2:0"
SOF_420 = bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


# (8, 8): a dummy column and a dummy row at once; (8, 24) / (24, 8): a real Y01 over a dummy row / a dummy column beside a real
# row; (16, 1040): 65 MCUs in a row, one more than a wavefront; (288, 550): the datasets' frame, nbx = 69 is odd
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (8, 8), (8, 24), (24, 8), (9, 17), (16, 16), (17, 33), (37, 53), (16, 1040), (288, 550)])
def test_jpeg_coefficients_420_equal_the_host_restatement(H, W, B):
    from pgdvs_amd import ops

    for name, x in R.float_inputs(B, H, W):
        xd = x.to(DEV)
        for quality in (50, 100):
            got = ops.jpeg_coefficients(xd, quality, subsampling=S420)
            assert got.shape == (B, (H + 15) // 16, (W + 15) // 16, 6, 64) and got.dtype == torch.int16 and got.is_cuda
            want = R.host_coef(x, quality, S420)
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, (name, quality, len(bad), bad[:4].tolist())
    one = ops.jpeg_coefficients(xd[0], 50, subsampling=S420)  # [3,H,W] is a batch of one
    assert np.array_equal(one.cpu().numpy(), R.host_coef(x[:1], 50, S420))
    out = torch.empty_like(one)
    assert ops.jpeg_coefficients(xd[0], 50, out=out, subsampling=S420).data_ptr() == out.data_ptr() and torch.equal(out, one)


def _crafted_grid_420(nmy, nmx, seed):
    """the crafted blocks of the 4:4:4 tests dealt over six blocks per MCU: twice the MCU columns of a three-block grid"""
    return R.crafted_grid(nmy, 2 * nmx, seed=seed).reshape(nmy, nmx, 6, 64)


def _scan_cases(nmy, nmx):
    from pgdvs_amd import video

    yield "crafted", _crafted_grid_420(nmy, nmx, seed=nmy * 100 + nmx)
    noise = np.random.default_rng(nmy + nmx).integers(0, 256, (16 * nmy, 16 * nmx, 3)).astype(np.uint8)
    yield "noise_q100", video.jpeg_coefficients(noise, 100, subsampling=S420)


# restart intervals: every MCU, a partial last segment, 42 and 43 (segments of 252 and 258 blocks: either side of one group of
# 256 blocks, a carry of bits into the second group), one row, two rows, more than the frame holds
@pytest.mark.parametrize("nmy,nmx", [(1, 1), (3, 5), (2, 65)])
def test_jpeg_scan_420_equals_the_host_coder(nmy, nmx):
    from pgdvs_amd import ops, video

    restarts = sorted({1, 4, 42, 43, nmx, 2 * nmx, nmy * nmx + 7})
    for name, coef in _scan_cases(nmy, nmx):
        batch = np.stack([coef, coef[::-1, ::-1].copy()])  # B = 2: frames of different lengths
        dev = torch.from_numpy(batch).to(DEV)
        for restart in restarts + [None]:
            cap = ops.jpeg_scan_capacity(nmy, nmx, nmx if restart is None else restart, 6)
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
    fresh, nb = ops.jpeg_scan(dev[0], 4)  # [nmy,nmx,6,64] is a batch of one; out allocated at the capacity
    assert fresh.shape == (1, ops.jpeg_scan_capacity(nmy, nmx, 4, 6)) and fresh[0, :int(nb[0])].cpu().numpy().tobytes() == video.encode_scan(batch[0], 4)


def test_jpeg_420_arguments():
    from pgdvs_amd import _lib, ops

    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8)), subsampling=S420)  # a host tensor
    with pytest.raises(_lib.PgdvsHipError):
        ops.jpeg_scan(torch.zeros((1, 1, 1, 6, 64), dtype=torch.int16))
    coef = torch.zeros((1, 2, 3, 6, 64), dtype=torch.int16, device=DEV)
    with pytest.raises(_lib.PgdvsHipError, match="host-only"):
        ops.jpeg_scan(coef, 0)  # no restart markers: the device pass needs byte-aligned segments
    with pytest.raises(_lib.PgdvsHipError, match="host-only"):
        ops.jpeg_encode(torch.zeros((3, 8, 8), device=DEV), restart_mcus=0, subsampling=S420)
    lib = _lib.load()
    ws = torch.empty(lib.pgdvs_jpeg_scan_420_workspace_bytes(1, 2, 3, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty(ops.jpeg_scan_capacity(2, 3, 3, 6), dtype=torch.uint8, device=DEV)
    nb = torch.empty(1, dtype=torch.int32, device=DEV)

    def call(restart=3, stride=out.numel(), ws_bytes=ws.numel(), nmy=2):
        return lib.pgdvs_jpeg_scan_420(coef.data_ptr(), 1, nmy, 3, restart, out.data_ptr(), stride, nb.data_ptr(), ws.data_ptr(), ws_bytes, None)

    assert call() == 0
    assert call(restart=0) == -1 and b"host-only" in lib.pgdvs_last_error()
    assert call(restart=65536) == -1
    assert call(stride=out.numel() - 1) == -1 and b"out_stride" in lib.pgdvs_last_error()
    assert call(ws_bytes=ws.numel() - 1) == -1
    assert call(nmy=0) == -1 and call(nmy=4097) == -1
    with pytest.raises(ValueError):
        ops.jpeg_scan(coef.float())  # a wrong dtype
    with pytest.raises(ValueError):
        ops.jpeg_scan(coef, 3, out=torch.empty((1, ops.jpeg_scan_capacity(2, 3, 3, 6) - 1), dtype=torch.uint8, device=DEV))  # too small
    with pytest.raises(ValueError):
        ops.jpeg_scan(torch.zeros((1, 2, 3, 4, 64), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError):
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8), device=DEV), subsampling="4:2:2")
    with pytest.raises(ValueError):  # the 4:4:4 shape for a 4:2:0 call
        ops.jpeg_coefficients(torch.zeros((1, 3, 8, 8), device=DEV), subsampling=S420, out=torch.empty((1, 1, 1, 3, 64), dtype=torch.int16, device=DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(37, 53), (288, 550)])
def test_jpeg_encode_420_gives_the_host_files(H, W):
    from pgdvs_amd import ops, video

    for name, x in R.float_inputs(2, H, W):
        if name == "table":
            continue
        for quality, restart in ((90, None), (50, 7)):
            data, nbytes = ops.jpeg_encode(x.to(DEV), quality, restart, subsampling=S420)
            host, n = data.cpu().numpy(), nbytes.cpu().tolist()
            for b in range(2):
                got = video.jpeg_frame(host[b, :n[b]].tobytes(), H, W, quality, restart, S420)
                assert got == video.encode_jpeg(x[b], quality, restart, subsampling=S420), (name, quality, restart, b)
                mode, size, pix = R.decode_pil(got)
                assert mode == "RGB" and size == (W, H)
                assert dict(R.segments(got)[0])[0xC0][6:] == SOF_420


def _pil_420(im, quality):
    import io

    import PIL.Image

    b = io.BytesIO()
    PIL.Image.fromarray(im).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
    return b.getvalue()


def test_vis_step_video_420_on_an_nvidia_vis_item(tmp_path):
    """set up as test_gpu_video.test_vis_step_video_on_an_nvidia_vis_item, with a 4:2:0 writer"""
    from pgdvs_amd import harness, video
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
    with video.MjpegWriter(n_threads=2, subsampling=S420) as w:
        paths, ret = harness.vis_step(model, batch, rc, tmp_path / "video", device=DEV, video=w, return_ret=True)
    avi = tmp_path / "video" / item["misc"].get("split", "") / f"{item['misc']['scene_id']}_combined.avi"
    assert w.files == [avi] and avi.exists()
    frames = R.avi_file_frames(avi)
    img = ret["combined_rgb"].cpu()
    assert frames == [video.encode_jpeg(img[0], 90, subsampling=S420)]
    mode, size, pix = R.decode_pil(frames[0])
    assert size == (NT.W, NT.H) and dict(R.segments(frames[0])[0])[0xC0][6:] == SOF_420
    # and PIL's own encoder writes the same scan from the PNG's pixels
    q8 = VR.expected_save_image(img[0]).permute(1, 2, 0).numpy()
    ours, theirs = video.encode_jpeg(q8, 90, 0, subsampling=S420), _pil_420(q8, 90)
    assert ours[R.segments(ours)[1]:] == theirs[R.segments(theirs)[1]:]


def test_vis_step_video_420_with_three_views_in_a_step(tmp_path):
    from pgdvs_amd import harness, video

    ds = VR.StubDataset(3, 37, 53, scenes=("scene_a", "scene_b"))
    batch = harness.collate([ds[i] for i in (2, 1, 0)])  # tgt_idx 7, 4, 1: the file sorts them
    with video.MjpegWriter(quality=75, restart_mcus=3, subsampling=S420) as w:
        harness.vis_step(VR.StubModel(), batch, None, tmp_path, device=DEV, video=w)
    assert R.avi_file_frames(tmp_path / "scene_a_combined.avi") == [video.encode_jpeg(ds[i]["img"], 75, 3, subsampling=S420) for i in (0, 2)]
    assert R.avi_file_frames(tmp_path / "scene_b_combined.avi") == [video.encode_jpeg(ds[1]["img"], 75, 3, subsampling=S420)]
    # through vis_run's own writer, and a GPU frame submitted directly
    harness.vis_run(VR.StubModel(), ds, None, tmp_path / "run", device=DEV, video=True, video_subsampling=S420)
    assert R.avi_file_frames(tmp_path / "run" / "scene_b_combined.avi") == [video.encode_jpeg(ds[1]["img"], 90, subsampling=S420)]
    with video.MjpegWriter(subsampling=S420) as w:
        w.submit((tmp_path / "run", "direct"), 0, ds[1]["img"].to(DEV))
    assert R.avi_file_frames(tmp_path / "run" / "direct_combined.avi") == [video.encode_jpeg(ds[1]["img"], 90, subsampling=S420)]


def test_1080p_420_once():
    """one render frame at quality 90, one MCU row per restart: nby = 135 is odd, so the last MCU row's Y10 and Y11 are dummy
    blocks.  Device coefficients and device bytes against the host's, which runs once."""
    from pgdvs_amd import ops, synth, video

    H, W = 1080, 1920
    x = torch.from_numpy(np.ascontiguousarray(synth.make_video(1, H, W, seed=5)["rgbs"])).permute(0, 3, 1, 2).contiguous()
    coef = ops.jpeg_coefficients(x.to(DEV), 90, subsampling=S420)
    want = R.host_coef(x, 90, S420)
    assert want.shape == (1, 68, 120, 6, 64) and np.array_equal(coef.cpu().numpy(), want)
    assert not want[0, -1, :, 2:4, 1:].any() and np.array_equal(want[0, -1, :, 2, 0], want[0, -1, :, 1, 0])  # the dummy row
    data, nbytes = ops.jpeg_scan(coef)
    n = int(nbytes[0])
    host = video.encode_scan(want[0])
    assert n == len(host) and data[0, :n].cpu().numpy().tobytes() == host
    mode, size, pix = R.decode_pil(video.jpeg_frame(host, H, W, 90, None, S420))
    assert size == (W, H)
