"""The evaluator's loop on the MI355X (harness.eval_run, csrc/png.hip's export pass): the one-launch export of a view's images
is byte-identical to the host path and to ``ops.png_scanlines(quant="truncate")``; the loop on the fused path leaves what the
reference's run left (tests/golden/eval_run_nvidia.npz); run-ahead changes no record and no file byte; a status error of a
view surfaces from the loop with the earlier views' files complete."""
import pathlib
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_run_reference as ER  # noqa: E402
import vis_reference as VR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


def _export_inputs(H, W):
    """three [3,H,W] images: the value table tiled (NaN, +-inf, values outside [0, 1], every k / 255 and its float32 neighbours
    on both sides), seeded noise stretched over [-0.1, 1.1), and the table rolled by one element"""
    g = torch.Generator().manual_seed(100 * H + W)
    table = VR.table_image(H, W)[0]
    noise = torch.rand((3, H, W), generator=g) * 1.2 - 0.1
    return table, noise, table.reshape(-1).roll(1).reshape(3, H, W).clone()


def _host_scanlines(x, adaptive):
    from pgdvs_amd import png

    q = png.QUANTIZERS["truncate"](x[None]).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(q, VR.expected_truncate(x[None]).permute(0, 2, 3, 1))
    return png.filter_scanlines(q, adaptive=adaptive)[0]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (24, 40), (67, 71), (288, 550), (1080, 1920)])
def test_export_scanlines_equal_the_host_path_and_png_scanlines(H, W):
    from pgdvs_amd import ops

    a, b, c = _export_inputs(H, W)
    if H * W >= 3 * 256 * 5:
        assert torch.isnan(a).any() and torch.isinf(a).any() and (a < 0).any() and (a > 1).any()
    for gt, pred, static in ((a, b, c), (b, c, a), (c, a, None), (b, a, None)):
        imgs = [gt, pred] + ([static] if static is not None else [])
        gt_hwc = gt.permute(1, 2, 0).contiguous().to(DEV)
        dev = [x.to(DEV) for x in imgs]
        for adaptive in (False, True):
            want = np.stack([_host_scanlines(x, adaptive) for x in imgs])
            got = ops.eval_export_scanlines(dev[1], gt_hwc, dev[2] if static is not None else None, adaptive=adaptive)
            assert got.shape == (len(imgs), H, 1 + 3 * W) and got.dtype == torch.uint8 and got.is_cuda
            planar = ops.png_scanlines(torch.stack(dev), quant="truncate", adaptive=adaptive)
            assert torch.equal(got, planar), (adaptive, "differs from png_scanlines(quant='truncate')")
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, (adaptive, len(bad), bad[:4].tolist())


def test_export_scanlines_alignments_out_in_place_and_errors():
    from pgdvs_amd import _lib, ops

    H, W = 37, 52  # (W % 4 == 0: the 16-byte loads when the pointers allow them)
    a, b, c = _export_inputs(H, W)
    want = np.stack([_host_scanlines(x, True) for x in (a, b, c)])
    n = 3 * H * (1 + 3 * W)
    for shift, guard in ((0, 64), (1, 61), (2, 62), (3, 63)):  # inputs off their 16-byte alignment, the output at every alignment
        def shifted(x):
            buf = torch.zeros(x.numel() + 4, device=DEV)
            buf[shift:shift + x.numel()] = x.reshape(-1).to(DEV)
            return buf[shift:shift + x.numel()].view(x.shape)

        buf = torch.full((guard + n + 67,), 0xA5, dtype=torch.uint8, device=DEV)
        out = buf[guard:guard + n]
        ret = ops.eval_export_scanlines(shifted(b), shifted(a.permute(1, 2, 0).contiguous()), shifted(c), out=out)
        assert ret.data_ptr() == out.data_ptr() and ret.shape == (3, H, 1 + 3 * W)
        host = buf.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + n:] == 0xA5).all(), guard
        assert np.array_equal(host[guard:guard + n].reshape(want.shape), want), (shift, guard)
    pd, gd = b.to(DEV), a.permute(1, 2, 0).contiguous().to(DEV)
    with pytest.raises(ops.PgdvsHipError):
        ops.eval_export_scanlines(b, a.permute(1, 2, 0).contiguous())  # host tensors: no fallback
    with pytest.raises(ValueError):
        ops.eval_export_scanlines(pd, a.to(DEV))  # a planar ground truth
    with pytest.raises(ValueError):
        ops.eval_export_scanlines(pd, gd, c[:, :-1].contiguous().to(DEV))
    with pytest.raises(ValueError):
        ops.eval_export_scanlines(pd, gd, out=torch.empty(n - 1, dtype=torch.uint8, device=DEV))
    # the C entry point's own checks: PGDVS_ERR_INVALID (-1) and a message, nothing launched
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    for args in ((pd.data_ptr(), gd.data_ptr(), None, 0, W, 1, out.data_ptr(), None), (pd.data_ptr(), gd.data_ptr(), None, H, 0, 1, out.data_ptr(), None),
                 (pd.data_ptr(), gd.data_ptr(), None, H, W, 2, out.data_ptr(), None), (None, gd.data_ptr(), None, H, W, 1, out.data_ptr(), None),
                 (pd.data_ptr(), gd.data_ptr(), None, H, W, 1, None, None), (pd.data_ptr(), gd.data_ptr(), None, 1 << 15, 1 << 15, 1, out.data_ptr(), None),
                 (pd.data_ptr() + 2, gd.data_ptr(), None, H, W, 1, out.data_ptr(), None)):
        assert lib.pgdvs_eval_export_scanlines(*args) == -1, args
        assert b"pgdvs_eval_export_scanlines" in lib.pgdvs_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("run", sorted(ER.RUNS))
def test_eval_run_on_the_gpu_leaves_what_the_reference_run_left(tmp_path, run):
    from pgdvs_amd import harness

    g = ER.load_fixture()
    with_geo, n_max = ER.RUNS[run]
    model = ER.RecordedModel(with_geo)
    res = harness.eval_run(model, ER.Items(g), "rc", batch_size=2, n_max_data=n_max, device=DEV, with_ssim=True, save_individual=True,
                           info_dir=tmp_path / "info", vis_dir=tmp_path / "vis", run_ahead=1)
    assert model.calls == (2 if run == "max3" else 3)
    ER.check_against_fixture(g, run, tmp_path, res, with_ssim=True)
    # the file bytes are the host path's
    host = tmp_path.parent / (tmp_path.name + "_host")
    harness.eval_run(ER.RecordedModel(with_geo), ER.Items(g), "rc", batch_size=2, n_max_data=n_max, with_ssim=True, save_individual=True,
                     info_dir=host / "info", vis_dir=host / "vis")
    for name in g[f"{run}_png_names"].tolist():
        assert (tmp_path / name).read_bytes() == (host / name).read_bytes(), name


class _Scene:
    """a 12-view synthetic scene through the real PGDVSRenderer (geometry path, the splat noise drawn by the kernel): the static
    cloud aggregated once and resident, added to every batch of one view"""
    H, W, S, N = 96, 160, 6, 12

    def __init__(self, mask_channels):
        from pgdvs_amd import ops, synth

        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        self.video = v = synth.make_video(self.S, self.H, self.W, seed=21)
        self.cloud, self.count, self.xyz = ops.static_aggregate(T(v["rgbs"]), T(v["depths"]), T(v["dyn_masks"]).view(torch.uint8), v["K3s"],
                                                                v["c2ws"], capacity=self.S * self.H * self.W, return_xyz=True)
        self.n_rows = ops.checked_count(self.count, "agg")
        g = torch.Generator().manual_seed(9)
        self.items = []
        for j in range(self.N):
            i = j % (self.S - 1)
            d = synth.to_torch(synth.make_view(v, i, frac=0.1 + 0.8 * j / (self.N - 1), seed=5), "cpu")
            d.pop("static_noise", None)
            item = {k: t[0] for k, t in d.items()}
            item["rgb_tgt"] = (item["rgb_src_temporal"][0] + 0.05 * torch.randn(self.H, self.W, 3, generator=g)).contiguous()
            item["eval_mask"] = (torch.rand(self.H, self.W, 1, generator=g) < 0.3).float().repeat(1, 1, mask_channels).contiguous()
            item["seq_ids"] = torch.tensor([j, i, i + 1])
            item["misc"] = {"scene_id": "synth", "tgt_frame_id": j, "tgt_cam_id": j % 3}
            self.items.append(item)

    def model(self, overflow_at=None):
        """a freshly seeded renderer (its splat noise state starts from the seed); ``overflow_at``: the view whose static cloud is
        aggregated inside the call into a buffer five rows too small (the construction of
        test_gpu_round4.py::test_native_view_call_aggregates_the_cloud_itself)"""
        from pgdvs_amd.instantiate import load_config
        from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

        torch.manual_seed(1234)
        cfg = load_config(static_renderer="geo")
        rc = cfg.engine.engine_cfg.render_cfg
        rc["dyn_pcl_remove_outlier"], rc["dyn_pcl_outlier_knn"], rc["st_render_pcl_pts_per_pixel"] = True, 16, 3
        inner = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(DEV).eval()
        scene = self

        class Resident:
            training = False
            forwards = []  # the views whose forward has been issued, in order

            def eval(self):
                return self

            def forward(self, data, **kw):
                v = scene.video
                self.forwards.append(data["misc"][0]["tgt_frame_id"])
                if overflow_at is not None and data["misc"][0]["tgt_frame_id"] == overflow_at:
                    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
                    extra = {"_st_pcl_video": {"rgbs": T(v["rgbs"]), "depths": T(v["depths"]), "dyn_masks": T(v["dyn_masks"]).view(torch.uint8),
                                               "K3s": v["K3s"], "c2ws": v["c2ws"], "capacity": scene.n_rows - 5},
                             "st_pcl_rgb_row_bound": scene.n_rows - 5}
                else:
                    extra = {"st_pcl_rgb": scene.cloud[None], "st_pcl_rgb_count": scene.count, "st_pcl_xyz": scene.xyz[None]}
                data.update(extra)  # (in place: the loop checks the status words against the batch it handed over)
                return inner.forward(data, **kw)

        model = Resident()
        model.forwards = []
        return model, rc


def _tree(root):
    return {name: (pathlib.Path(root) / name).read_bytes() for name in ER.all_files(root)}


@pytest.mark.parametrize("quant_type,with_ssim", [("nvidia", True), ("dycheck_iphone", False)])
def test_run_ahead_changes_no_record_and_no_file(tmp_path, quant_type, with_ssim):
    from pgdvs_amd import harness

    scene = _Scene(3 if quant_type == "nvidia" else 1)
    runs = {}
    for k in (0, 1, 2, 3):
        model, rc = scene.model()
        d = tmp_path / f"k{k}"
        res = harness.eval_run(model, scene.items, rc, device=DEV, quant_type=quant_type, with_ssim=with_ssim, save_individual=True,
                               info_dir=d / "info", vis_dir=d / "vis", run_ahead=k)
        runs[k] = (res, _tree(d))
    res0, tree0 = runs[0]
    assert res0["eval/count"] == scene.N and len(tree0) == scene.N * 4  # record, gt, combined, geo_static
    n_keys = 7 if quant_type == "nvidia" else 5
    assert all(len(r["info"]) == n_keys for r in res0["records"])
    for k in (1, 2, 3):
        res, tree = runs[k]
        assert sorted(tree) == sorted(tree0)
        for r0, r in zip(res0["records"], res["records"]):
            assert r["name"] == r0["name"] and list(r["info"]) == list(r0["info"])
            for key in r0["info"]:
                same = np.array_equal(r["info"][key], r0["info"][key])
                if not same:
                    print(f"run_ahead {k} {r['name']} {key}: {r['info'][key]!r} against {r0['info'][key]!r}")
                assert same, (k, r["name"], key, r["info"][key], r0["info"][key])
        assert res["sums"] == res0["sums"] and {kk: v for kk, v in res.items() if kk != "records"} == {kk: v for kk, v in res0.items() if kk != "records"}
        for name in tree0:
            assert tree[name] == tree0[name], (k, name)
    for name, data in tree0.items():
        if name.endswith(".pkl"):
            info = pickle.loads(data)
            assert list(info)[0] == "src_frame_ids" and all(type(v) is float for kk, v in info.items() if kk != "src_frame_ids")
    # k = 0 against a plain loop over eval_step, the sums accumulated as run_eval_single_ckpt accumulates them
    model, rc = scene.model()
    loss_sum = {}
    for item in scene.items:
        stats = harness.eval_step(model, harness.collate([item]), rc, device=DEV, quant_type=quant_type, with_ssim=with_ssim)
        for key, v in stats.items():
            loss_sum[key] = loss_sum.get(key, 0.0) + v.cpu()
    assert int(loss_sum["eval/count"]) == res0["eval/count"]
    for key, v in loss_sum.items():
        if key != "eval/count":
            print(f"{key}: plain loop {float(v)!r} eval_run {res0['sums'][key]!r}")
            assert float(v) == res0["sums"][key], key
            assert float(v / loss_sum["eval/count"]) == res0[key], key


@pytest.mark.parametrize("run_ahead", [0, 2])
def test_a_status_error_surfaces_late_and_earlier_files_are_complete(tmp_path, run_ahead):
    """view 5's static cloud overflows its capacity (the library's own status word, read back with the metric rows): the error
    is raised when view 5 is finished, by which time the loop has issued the forwards of run_ahead more views (with run_ahead
    2: views 0..7; with 0: views 0..5) -- the one place where the order of enqueue and finish shows without a clock; views
    0..4 are on disk, whole, and nothing of view 5 or later"""
    from pgdvs_amd import harness, ops

    scene = _Scene(3)
    model, rc = scene.model(overflow_at=5)
    with pytest.raises(ops.PgdvsHipError, match="filled its buffer"):
        harness.eval_run(model, scene.items, rc, device=DEV, save_individual=True, info_dir=tmp_path / "info", vis_dir=tmp_path / "vis",
                         run_ahead=run_ahead)
    assert model.forwards == list(range(5 + run_ahead + 1)), model.forwards
    torch.cuda.synchronize()
    files = ER.all_files(tmp_path)
    want = sorted([f"info/synth/{j:05d}_cam_{j % 3:03d}_rank_0.pkl" for j in range(5)]
                  + [f"vis/synth/{j:05d}_cam_{j % 3:03d}_{tag}.png" for j in range(5) for tag in ("gt", "combined", "geo_static")])
    assert files == want
    for name in want:
        if name.endswith(".png"):
            mode, size, pix = ER.decode(tmp_path / name)
            assert mode == "RGB" and size == (scene.W, scene.H)
        else:
            with open(tmp_path / name, "rb") as f:
                assert list(pickle.load(f)) == ["src_frame_ids", "psnr_full_combined", "psnr_dyn_combined", "psnr_static_combined"]


def test_both_static_images_on_the_gpu(tmp_path):
    """a renderer that returns static_coarse_rgb and geo_static_rgb: one rides in the view's export launch, the other takes a
    png_scanlines launch; both files hold the truncating cast, and every file's bytes are the host path's"""
    from pgdvs_amd import harness

    g = ER.load_fixture()
    res = harness.eval_run(ER.RecordedModel(with_geo=True, gnt=True), ER.Items(g), None, batch_size=2, device=DEV, save_individual=True,
                           info_dir=tmp_path / "gpu" / "info", vis_dir=tmp_path / "gpu" / "vis", run_ahead=1)
    ER.check_static_images(g, tmp_path / "gpu" / "vis", res, VR.expected_truncate)
    harness.eval_run(ER.RecordedModel(with_geo=True, gnt=True), ER.Items(g), None, batch_size=2, save_individual=True,
                     info_dir=tmp_path / "host" / "info", vis_dir=tmp_path / "host" / "vis")
    for name in ER.all_files(tmp_path / "host" / "vis"):
        assert (tmp_path / "gpu" / "vis" / name).read_bytes() == (tmp_path / "host" / "vis" / name).read_bytes(), name
