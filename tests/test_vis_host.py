"""The visualiser's loop and its PNG export on the host (pgdvs_amd/png.py, harness.vis_step / vis_run): the container decodes
with PIL (independent of the writer) to the quantised pixels, the two quantisers match the reference writers' expressions
on a value table, the filter choice is libpng's under a per-row restatement kept in vis_reference.py, and the loop lays the
files out and selects the items as ``PGDVSVisualizer.vis_model`` does."""
import math
import os
import pathlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import vis_reference as VR  # noqa: E402

from pgdvs_amd import harness, png  # noqa: E402


def _decode(path_or_bytes):
    import io

    src = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    with PIL.Image.open(src) as im:
        im.load()
        return im.mode, im.size, np.asarray(im).copy()


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("H,W", VR.SIZES)
def test_encode_decodes_with_pil_to_the_same_pixels(H, W, adaptive):
    q = VR.noise_bytes(H, W, seed=H * 1000 + W)
    data = png.encode(png.filter_scanlines(q, adaptive=adaptive), H, W)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    mode, size, pix = _decode(data)
    assert mode == "RGB" and size == (W, H)
    assert np.array_equal(pix, q)
    with pytest.raises(ValueError):
        png.encode(png.filter_scanlines(q, adaptive=adaptive), H + 1, W)


def test_quantisers_on_the_value_table():
    t = VR.value_table()
    assert t.numel() > 2500 and torch.isnan(t).any() and torch.isinf(t).any() and (t < 0).any() and (t > 1).any()
    a, b = png.quantize_save_image(t), png.quantize_truncate(t)
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8
    assert torch.equal(a, VR.expected_save_image(t))
    assert torch.equal(b, VR.expected_truncate(t))
    assert not torch.equal(a, b)  # (a swap of the modes fails the two lines above)
    special = torch.tensor([float("nan"), float("inf"), float("-inf")])
    assert png.quantize_save_image(special).tolist() == [0, 255, 0]
    assert png.quantize_truncate(special).tolist() == [0, 255, 0]
    # every k + 0.5 boundary separates the modes: rounding gives k + 1, truncation k
    half = torch.from_numpy(((np.arange(255) + 0.75) / 255.0).astype(np.float32))
    assert png.quantize_save_image(half).tolist() == list(range(1, 256))
    assert png.quantize_truncate(half).tolist() == list(range(255))


def test_filter_choice_is_libpngs():
    seen = np.zeros(5, dtype=np.int64)
    for H, W in VR.SIZES:
        q = VR.noise_bytes(H, W, seed=H + W)
        got = png.filter_scanlines(q, adaptive=True)
        assert got.shape == (H, 1 + 3 * W) and got.dtype == np.uint8
        rows = q.reshape(H, 3 * W)
        for y in range(H):
            cands = VR.row_candidates(rows[y], rows[y - 1] if y > 0 else np.zeros(3 * W, np.uint8))
            costs = [VR.row_cost(f) for f in cands]
            t = int(got[y, 0])
            assert 0 <= t <= 4 and costs[t] == min(costs) and all(costs[j] > costs[t] for j in range(t)), (H, W, y, t, costs)
            assert got[y, 1:].tolist() == cands[t], (H, W, y, t)
        seen += np.bincount(got[:, 0], minlength=5)
        plain = png.filter_scanlines(q, adaptive=False)
        assert not plain[:, 0].any() and np.array_equal(plain[:, 1:].reshape(H, W, 3), q)
    assert (seen > 0).all(), seen  # the inputs exercise all five filter types
    const = np.full((6, 9, 3), 77, np.uint8)
    assert np.array_equal(VR.expected_scanlines(const)[:, 0], [1, 2, 2, 2, 2, 2])
    assert np.array_equal(png.filter_scanlines(const)[:, 0], [1, 2, 2, 2, 2, 2])
    thin = np.full((5, 1, 3), 77, np.uint8)
    assert np.array_equal(VR.expected_scanlines(thin)[:, 0], [0, 2, 2, 2, 2])
    assert np.array_equal(png.filter_scanlines(thin)[:, 0], [0, 2, 2, 2, 2])
    assert not png.filter_scanlines(np.zeros((4, 5, 3), np.uint8)).any()
    batch = np.stack([VR.noise_bytes(5, 6, seed=1), VR.noise_bytes(5, 6, seed=2)])
    assert np.array_equal(png.filter_scanlines(batch), np.stack([VR.expected_scanlines(v) for v in batch]))


def _expected_files(ds, indices, vis_dir):
    out = {}
    for i in indices:
        it = ds[i]
        d = pathlib.Path(vis_dir) / it["misc"].get("split", "") / it["misc"]["scene_id"]
        out[d / f"{it['misc']['tgt_idx']:05d}_combined.png"] = VR.expected_save_image(it["img"]).permute(1, 2, 0).numpy()
        if "gnt" in it:
            out[d / f"{it['misc']['tgt_idx']:05d}_gnt.png"] = VR.expected_truncate(it["gnt"]).permute(1, 2, 0).numpy()
    return out


def _all_files(root):
    return sorted(p for p in pathlib.Path(root).rglob("*") if p.is_file())


def _check_tree(root, expected):
    assert _all_files(root) == sorted(expected), (_all_files(root), sorted(expected))  # (also: no temporary file is left)
    for path, pix in expected.items():
        mode, size, got = _decode(path)
        assert mode == "RGB" and size == (pix.shape[1], pix.shape[0])
        assert np.array_equal(got, pix), path


@pytest.mark.parametrize("split,gnt", [(None, False), ("val", True)])
def test_vis_step_layout_and_pixels(tmp_path, split, gnt):
    ds = VR.StubDataset(3, 9, 14, split=split, gnt=gnt, scenes=("scene_a", "scene_b"))
    batch = harness.collate([ds[i] for i in range(3)])
    assert batch["img"].shape == (3, 3, 9, 14) and isinstance(batch["misc"], list) and batch["name"] == ["v0", "v1", "v2"]
    assert isinstance(batch["time"], torch.Tensor) and batch["time"].shape == (3,)
    model = VR.StubModel()
    paths, ret = harness.vis_step(model, batch, None, tmp_path, return_ret=True)
    assert not model.training and ret["combined_rgb"] is not None
    expected = _expected_files(ds, range(3), tmp_path)
    assert sorted(paths) == sorted(expected)
    assert all((p.name.endswith("_gnt.png") for p in paths[1::2])) if gnt else not any("_gnt" in p.name for p in paths)
    if split is None:
        assert {p.parent.parent for p in paths} == {tmp_path}
    else:
        assert {p.parent.parent for p in paths} == {tmp_path / "val"}
    _check_tree(tmp_path, expected)
    if gnt:  # the two quantisations differ on these images: a swap of the writers fails above
        it = ds[0]
        assert not np.array_equal(VR.expected_save_image(it["gnt"]).numpy(), VR.expected_truncate(it["gnt"]).numpy())


@pytest.mark.parametrize("n,batch_size,n_max_data,rank,world", [
    (7, 1, -1, 0, 1), (7, 2, -1, 0, 1), (7, 2, 5, 0, 1), (7, 1, 5, 1, 2), (7, 2, -1, 1, 3), (7, 3, 4, 0, 2), (5, 1, 100, 2, 4),
])
def test_vis_run_selects_the_reference_indices(tmp_path, n, batch_size, n_max_data, rank, world):
    ds = VR.StubDataset(n, 5, 6, gnt=True, scenes=("scene_a", "scene_b"))
    # DistributedSampler(shuffle=False, drop_last=False): pad by wrapping to a multiple of world, then rank::world; the
    # loader batches that list and the loop stops after ceil(min(len, n_max_data) / (batch_size world)) steps
    total = math.ceil(n / world) * world
    order = (list(range(n)) * 2)[:total][rank::world]
    n_all = min(n, n_max_data) if n_max_data > 0 else n
    steps = math.ceil(n_all / (batch_size * world))
    picked = [i for s in range(steps) for i in order[s * batch_size:(s + 1) * batch_size]]
    dirs = harness.vis_run(VR.StubModel(), ds, None, tmp_path, batch_size=batch_size, n_max_data=n_max_data, rank=rank, world=world)
    assert dirs == {ds[i]["misc"]["scene_id"]: tmp_path / ds[i]["misc"]["scene_id"] for i in picked}
    _check_tree(tmp_path, _expected_files(ds, picked, tmp_path))


def test_writer_reports_a_workers_failure_and_leaves_no_temporaries(tmp_path):
    ds = VR.StubDataset(4, 5, 6)
    q = [VR.expected_save_image(ds[i]["img"]).permute(1, 2, 0).numpy() for i in range(4)]
    with png.PngWriter(n_threads=2, n_slots=2) as w:
        for i in range(4):
            w.submit(tmp_path / f"{i}.png", png.filter_scanlines(q[i]))
    assert w.files_written == 4 and w.bytes_written == sum(p.stat().st_size for p in _all_files(tmp_path))
    _check_tree(tmp_path, {tmp_path / f"{i}.png": q[i] for i in range(4)})
    with pytest.raises(RuntimeError):
        w.submit(tmp_path / "late.png", png.filter_scanlines(q[0]))
    # a path whose directory is a regular file: unwritable for every user
    blocker = tmp_path / "blocker"
    blocker.write_bytes(b"x")
    w = png.PngWriter(n_threads=2)
    w.submit(tmp_path / "ok.png", torch.from_numpy(png.filter_scanlines(q[1])))
    w.submit(blocker / "no.png", png.filter_scanlines(q[0]))
    with pytest.raises(OSError):
        w.close()
    w.close()  # (the failure is reported once)
    assert sorted(os.listdir(tmp_path)) == ["0.png", "1.png", "2.png", "3.png", "blocker", "ok.png"]
    with pytest.raises(ValueError):
        png.PngWriter(n_threads=17)
    with pytest.raises(OSError):
        harness.vis_run(VR.StubModel(), ds, None, blocker)
