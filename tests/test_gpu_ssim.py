"""The evaluator's masked SSIM on the MI355X (csrc/eval_ssim.hip): ops.eval_ssim_sums against the numpy float64
restatement of calculate_ssim (tests/test_ssim_host.py), its determinism, harness.eval_step(with_ssim=True) on the
fused GPU path against the torch path, and around the real HIP renderer."""
import numpy as np
import pytest
import torch

import test_ssim_host as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


def _raw_inputs(H, W, seed, mask_kind):
    """raw (unquantised) render [3,H,W] and ground truth [H,W,3] with NaN, negative and > 1 values; mask [H,W,3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.4 * (np.sin(xx / 17.0) * np.cos(yy / 11.0))[..., None] * np.ones(3)
    gt = (base + 0.05 * rng.standard_normal((H, W, 3))).astype(np.float32)
    pred = (gt + 0.08 * rng.standard_normal((H, W, 3))).astype(np.float32)
    pred[rng.random((H, W, 3)) < 0.01] = np.nan
    pred[rng.random((H, W, 3)) < 0.01] = -0.3
    pred[rng.random((H, W, 3)) < 0.01] = 1.4
    gt[rng.random((H, W, 3)) < 0.005] = 1.2
    if mask_kind == "binary":
        mask = (rng.random((H, W, 1)) < 0.3).astype(np.float32).repeat(3, axis=-1)
    elif mask_kind == "soft":
        mask = rng.random((H, W, 3)).astype(np.float32)
    else:  # empty dynamic region
        mask = np.zeros((H, W, 3), np.float32)
    return np.ascontiguousarray(pred.transpose(2, 0, 1)), gt, mask


def _expected(pred_planar, gt, mask):
    pq, gq = R.quantise(pred_planar.transpose(1, 2, 0)), R.quantise(gt)
    S = R.ssim_map(gq, pq)
    m = mask.astype(np.float64)
    ms = (np.float32(1.0) - mask).astype(np.float64)
    vals = [float(np.sum(S * w) / (np.sum(w) + 1e-8)) for w in (np.ones_like(m), m, ms)]
    return vals, S


@pytest.mark.parametrize("H,W,mask_kind", [(256, 256, "binary"), (540, 960, "soft"), (1080, 1920, "binary"), (37, 1001, "empty"),
                                           (7, 7, "soft"), (7, 70, "empty")])
def test_eval_ssim_sums_vs_restatement(H, W, mask_kind):
    from pgdvs_amd import ops

    pred, gt, mask = _raw_inputs(H, W, H * 7 + W, mask_kind)
    sums, smap = ops.eval_ssim_sums(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(mask).to(DEV),
                                    want_map=True)
    s = sums.cpu().numpy()
    want, S = _expected(pred, gt, mask)
    assert s[3] == 3 * H * W and s[6] == 0 and s[7] == 0
    np.testing.assert_allclose(s[4], mask.astype(np.float64).sum(), rtol=1e-7)  # (eight values at a time in fp32)
    for j, name in enumerate(("full", "dyn", "static")):
        got = s[j] / (s[3 + j] + 1e-8)
        assert abs(got - want[j]) <= 1e-6, (name, got, want[j])
    if mask_kind == "empty":
        assert s[1] == 0 and s[4] == 0
    err = float(np.abs(smap.cpu().numpy().transpose(1, 2, 0) - S).max())
    assert err <= 1e-4, err


def test_eval_ssim_sums_deterministic_and_small_sizes_rejected():
    from pgdvs_amd import ops

    pred, gt, mask = (torch.from_numpy(a).to(DEV) for a in _raw_inputs(1080, 1920, 3, "soft"))
    a = ops.eval_ssim_sums(pred, gt, mask)[0].cpu().numpy()
    b = ops.eval_ssim_sums(pred, gt, mask)[0].cpu().numpy()
    assert a.tobytes() == b.tobytes()
    for H, W in ((6, 20), (20, 6)):
        p, g, m = (torch.from_numpy(x).to(DEV) for x in _raw_inputs(max(H, 7), max(W, 7), 1, "binary"))
        with pytest.raises(ValueError):
            ops.eval_ssim_sums(p[:, :H, :W], g[:H, :W], m[:H, :W])


def _fake_model(pred):
    class Fake(torch.nn.Module):
        def forward(self, data_gpu, render_cfg=None, disable_tqdm=True, for_debug=False):
            return {"combined_rgb": pred}

    return Fake()


def test_eval_step_fused_ssim_vs_torch_path():
    from pgdvs_amd.harness import METRIC_KEYS, SSIM_KEYS, eval_step

    B, H, W = 2, 120, 200
    ins = [_raw_inputs(H, W, 40 + b, "binary") for b in range(B)]
    pred = torch.from_numpy(np.stack([i[0] for i in ins]))
    data = {"rgb_src_temporal": torch.zeros(B, 2, H, W, 3), "rgb_tgt": torch.from_numpy(np.stack([i[1] for i in ins])),
            "eval_mask": torch.from_numpy(np.stack([i[2] for i in ins])), "misc": [{}] * B}
    data_gpu = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in data.items()}
    md_gpu0 = eval_step(_fake_model(pred.to(DEV)), data_gpu, "rc", device=DEV)
    md_gpu, ex = eval_step(_fake_model(pred.to(DEV)), data_gpu, "rc", device=DEV, with_ssim=True, return_images=True)
    md_cpu, ex_cpu = eval_step(_fake_model(pred), data, "rc", device="cpu", with_ssim=True, return_images=True)
    assert set(md_gpu) == set(md_cpu) == set(md_gpu0) | {f"eval/{k}" for k in SSIM_KEYS}
    assert int(md_gpu["eval/count"]) == B
    for k in METRIC_KEYS:
        assert md_gpu[f"eval/{k}"].numpy().tobytes() == md_gpu0[f"eval/{k}"].numpy().tobytes(), k
    for k in SSIM_KEYS:
        assert md_gpu[f"eval/{k}"].dtype == torch.float32 and md_gpu[f"eval/{k}"].device.type == "cpu"
        assert abs(float(md_gpu[f"eval/{k}"]) - float(md_cpu[f"eval/{k}"])) <= 1e-6 * B, k
        np.testing.assert_allclose(ex["per_view"][k], ex_cpu["per_view"][k], rtol=0, atol=1e-6, err_msg=k)


def test_eval_step_with_ssim_around_the_hip_renderer():
    from pgdvs_amd import synth
    from pgdvs_amd.datasets.static_aggregation import aggregate_static_pcl
    from pgdvs_amd.harness import SSIM_KEYS, eval_step
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    H, W, S = 256, 256, 4
    v = synth.make_video(S, H, W, seed=31)
    d = synth.make_view(v, 1, seed=5)
    cfg = load_config(static_renderer="geo")
    rc = cfg.engine.engine_cfg.render_cfg
    for k, x in dict(dyn_pcl_remove_outlier=True, dyn_pcl_outlier_knn=20, st_render_pcl_pts_per_pixel=3,
                     st_render_pcl_pt_radius=0.02).items():
        rc[k] = x
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(DEV).eval()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    cloud = aggregate_static_pcl(T(v["rgbs"]), T(v["depths"]), T(v["dyn_masks"]), v["K3s"], v["c2ws"])
    rng = np.random.default_rng(9)
    gt = np.clip(v["rgbs"][1][None] + 0.05 * rng.standard_normal((1, H, W, 3)), 0, 1).astype(np.float32)
    dyn = np.repeat(v["dyn_masks"][1][None, ..., None], 3, axis=-1).astype(np.float32)
    data = {k: torch.from_numpy(np.ascontiguousarray(x)) for k, x in d.items()}
    data["st_pcl_rgb"] = cloud[None].cpu()
    data["rgb_tgt"], data["eval_mask"] = torch.from_numpy(gt), torch.from_numpy(dyn)
    data["misc"] = [{"scene_id": "synthetic", "tgt_frame_id": 1, "tgt_cam_id": 0}]
    md, ex = eval_step(model, data, rc, device=DEV, return_images=True, with_ssim=True)
    # the restatement on the quantised images the step returns (as 8-bit codes, then / 255 in float32)
    codes = lambda t: np.rint(t[0].cpu().numpy().transpose(1, 2, 0) * 255.0).astype(np.float32) / np.float32(255)  # noqa: E731
    pq, gq = codes(ex["pred"]), codes(ex["gt"])
    m = dyn[0].astype(np.float64)
    for k, w in zip(SSIM_KEYS, (np.ones_like(m), m, 1.0 - m)):
        want = R.calculate_ssim(gq, pq, w)
        assert abs(ex["per_view"][k][0] - want) <= 1e-6, (k, ex["per_view"][k][0], want)
        assert abs(float(md[f"eval/{k}"]) - want) <= 1e-6, (k, float(md[f"eval/{k}"]), want)
    assert 0.0 < float(md["eval/ssim_full_combined"]) < 1.0
