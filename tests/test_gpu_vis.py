"""The visualiser's export on the MI355X (csrc/png.hip, harness.vis_step, png.PngWriter): the HIP scanlines are byte-identical
to the host path's quantise + filter, for both quantisations, adaptive and not, at every row alignment; an nvidia_vis item
goes through PGDVSRenderer and vis_step to files that decode (with PIL) to the quantised ``ret`` tensors and equal the host
path's file bytes; the writer's slot ring never hands a buffer out before its file is written."""
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import nvidia_tree as NT  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402
import vis_reference as VR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def _inputs(B, H, W):
    """seeded noise over [0, 1) (uniform bytes once quantised), a synthetic render (smooth background, moving objects), the
    value table tiled (values outside [0, 1], NaN, +-inf included)"""
    from pgdvs_amd import synth

    g = torch.Generator().manual_seed(1000 * H + W + B)
    yield "noise", torch.rand((B, 3, H, W), generator=g)
    if H >= 16 and W >= 16:
        video = synth.make_video(B, H, W, seed=5)
        yield "render", torch.from_numpy(np.ascontiguousarray(video["rgbs"])).permute(0, 3, 1, 2).contiguous()
    yield "table", VR.table_image(H, W).repeat(B, 1, 1, 1)


# frame sizes of the datasets and 1080p, and rows wider than the kernel's LDS chunk (2048 pixels), with and without the float4 loads
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (31, 45), (288, 550), (1080, 1920), (3, 4100), (2, 6145)])
def test_png_scanlines_equal_the_host_path(H, W, B):
    from pgdvs_amd import ops, png

    types = np.zeros(5, dtype=np.int64)
    for name, x in _inputs(B, H, W):
        xd = x.to(DEV)
        for quant, fn in (("save_image", png.quantize_save_image), ("truncate", png.quantize_truncate)):
            q = fn(x).permute(0, 2, 3, 1).contiguous()
            assert torch.equal(q, VR.EXPECTED[quant](x).permute(0, 2, 3, 1)), (name, quant)
            for adaptive in (False, True):
                want = png.filter_scanlines(q, adaptive=adaptive)
                got = ops.png_scanlines(xd, quant=quant, adaptive=adaptive)
                assert got.shape == (B, H, 1 + 3 * W) and got.dtype == torch.uint8 and got.is_cuda
                got = got.cpu().numpy()
                bad = np.argwhere(got != want)
                assert bad.size == 0, (name, quant, adaptive, len(bad), bad[:4].tolist(), np.bincount(got[..., 0].ravel(), minlength=5))
                if adaptive and name == "noise":
                    types += np.bincount(got[..., 0].ravel(), minlength=5)[:5]
    if H >= 288:  # (uniform byte noise of a few hundred rows takes every filter type; a handful of rows need not)
        assert (types > 0).all(), types


def test_png_scanlines_fill_out_in_place_and_nothing_else():
    from pgdvs_amd import ops, png

    B, H, W = 2, 37, 53
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(3)) * 1.2 - 0.1
    want = png.filter_scanlines(png.quantize_save_image(x).permute(0, 2, 3, 1).contiguous())
    n = B * H * (1 + 3 * W)
    for guard in (64, 61, 62, 63):  # the output at every alignment
        buf = torch.full((guard + n + 67,), 0xA5, dtype=torch.uint8, device=DEV)
        out = buf[guard:guard + n]
        ret = ops.png_scanlines(x.to(DEV), out=out)
        assert ret.data_ptr() == out.data_ptr() and ret.shape == (B, H, 1 + 3 * W)
        host = buf.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + n:] == 0xA5).all(), guard
        assert np.array_equal(host[guard:guard + n].reshape(want.shape), want), guard
    one = ops.png_scanlines(x[0].to(DEV), quant="truncate", adaptive=False)  # [3,H,W] is a batch of one
    assert np.array_equal(one.cpu().numpy()[0, :, 1:].reshape(H, W, 3), VR.expected_truncate(x[0]).permute(1, 2, 0).numpy())
    with pytest.raises(ops.PgdvsHipError):
        ops.png_scanlines(x)
    with pytest.raises(ValueError):
        ops.png_scanlines(x.to(DEV), quant="round")
    with pytest.raises(ValueError):
        ops.png_scanlines(x.to(DEV), out=torch.empty(n - 1, dtype=torch.uint8, device=DEV))


def test_vis_step_on_an_nvidia_vis_item(tmp_path):
    """set up as test_nvidia_vis_item_through_renderer: the visualiser config, a seeded GNT of depth 2"""
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
    model = PGDVSRenderer(cfg, render_cfg=rc).to(DEV).eval()
    ds = NvidiaDynVisualizationDataset(data_root=VT.build_tree(tmp_path / "tree"), device=None, **VT.KW)
    item = ds[10]
    batch = harness.collate([item])
    batch["static_noise"] = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, NT.H, NT.W)).astype(np.float32))
    with png.PngWriter(n_threads=2) as w:
        for out_dir, writer in ((tmp_path / "sync", None), (tmp_path / "async", w)):
            paths, ret = harness.vis_step(model, batch, rc, out_dir, device=DEV, writer=writer, return_ret=True)
            if writer is not None:
                writer.close()
            assert ret["combined_rgb"].is_cuda and "static_coarse_rgb" in ret
            scene_dir = out_dir / item["misc"].get("split", "") / item["misc"]["scene_id"]
            stem = f"{item['misc']['tgt_idx']:05d}"
            assert paths == [scene_dir / f"{stem}_combined.png", scene_dir / f"{stem}_gnt.png"]
            assert sorted(p.name for p in scene_dir.iterdir()) == [f"{stem}_combined.png", f"{stem}_gnt.png"]
            for path, key, quant in ((paths[0], "combined_rgb", "save_image"), (paths[1], "static_coarse_rgb", "truncate")):
                img = ret[key].cpu()
                want = VR.EXPECTED[quant](img)[0].permute(1, 2, 0).numpy()
                assert np.array_equal(_decode(path), want), (path, quant)
                host_q = png.QUANTIZERS[quant](img)[0].permute(1, 2, 0).contiguous()
                host_file = png.encode(png.filter_scanlines(host_q), want.shape[0], want.shape[1])
                assert path.read_bytes() == host_file, (path, "file bytes differ from the host path's")
    cpu = harness.vis_step(VR.StubModel(), {"img": ret["combined_rgb"].cpu(), "misc": batch["misc"]}, None, tmp_path / "cpu")
    assert cpu[0].read_bytes() == paths[0].read_bytes()


def test_writer_with_fewer_slots_than_views(tmp_path):
    from pgdvs_amd import ops, png

    H, W, n = 288, 550, 12
    x = torch.rand((n, 3, H, W), generator=torch.Generator().manual_seed(11))
    want = VR.expected_save_image(x).permute(0, 2, 3, 1).numpy()
    assert len({want[i].tobytes() for i in range(n)}) == n
    xd = x.to(DEV)
    with png.PngWriter(n_threads=3, n_slots=2) as w:
        for i in range(n):  # each view's scanlines in a fresh device buffer, submitted back to back
            w.submit(tmp_path / f"{i:02d}.png", ops.png_scanlines(xd[i:i + 1])[0])
    assert w.files_written == n
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"{i:02d}.png" for i in range(n)]
    for i in range(n):
        assert np.array_equal(_decode(tmp_path / f"{i:02d}.png"), want[i]), i
