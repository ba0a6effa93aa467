"""The DyCheck iPhone metric protocol (quant_type "dycheck_iphone") without a GPU: the float32 torch restatements
(harness.masked_{psnr,ssim,lpips}_dycheck) against the reference's own pgdvs/utils/dycheck/metrics.py (tests/golden/dycheck.npz,
made by tests/golden/make_golden_dycheck.py), the protocol's empty-mask and identical-image behaviours, the ScalingLayer,
eval_step(quant_type="dycheck_iphone") on CPU tensors, and quant_type_from_engine_cfg."""
import math
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import lpips_inputs as LI  # noqa: E402

CASES = ("a", "b", "c31", "ident", "empty", "dark", "wide")


def golden():
    return dict(np.load(GOLDEN / "dycheck.npz"))


def weights(g=None, device="cpu"):
    from pgdvs_amd.harness import LpipsAlex

    g = golden() if g is None else g
    bb = {k: torch.from_numpy(v) for k, v in LI.backbone_weights().items()}
    return LpipsAlex(bb, {f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]) for k in range(5)}, device)


def case(g, name):
    """quantised gt / pred [3,H,W] and the covisibility mask [1,H,W]"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)  # noqa: E731
    gt = T(g[f"{name}_gt"].astype(np.float32) / np.float32(255))
    pred = T(g[f"{name}_pred"].astype(np.float32) / np.float32(255))
    return gt, pred, torch.from_numpy(g[f"{name}_mask"].astype(np.float32))[None]


def close(got, want, atol):
    """equal infinities, else within atol"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=atol)


def test_fixture_matches_the_seeded_backbone():
    np.testing.assert_allclose(golden()["weights_checksum"], LI.checksum(LI.backbone_weights()), rtol=1e-12)


@pytest.mark.parametrize("name", CASES)
def test_psnr_ssim_vs_reference_golden(name):
    from pgdvs_amd.harness import masked_psnr_dycheck, masked_ssim_dycheck

    g = golden()
    gt, pred, m = case(g, name)
    ones = torch.ones_like(m)
    got = [masked_psnr_dycheck(gt, pred, ones), masked_ssim_dycheck(gt, pred, ones), masked_psnr_dycheck(gt, pred, m),
           masked_ssim_dycheck(gt, pred, m)]
    close(got, g[f"{name}_psnr_ssim"], 1e-5)


@pytest.mark.parametrize("name", CASES)
def test_lpips_vs_reference_golden(name):
    from pgdvs_amd.harness import masked_lpips_dycheck

    g = golden()
    gt, pred, m = case(g, name)
    w = weights(g)
    got = [masked_lpips_dycheck(gt, pred, torch.ones_like(m), w), masked_lpips_dycheck(gt, pred, m, w)]
    np.testing.assert_allclose(got, g[f"{name}_lpips"], rtol=0, atol=1e-5)


def test_upsample_forms_gap():
    """The reference's copy of PNetLin upsamples by scale_factor = out / in, lpips 0.1.4 by size.  Measured on every fixture
    case: the two give bit-identical values (gap 0)."""
    g = golden()
    for name in CASES:
        assert np.abs(g[f"{name}_lpips"] - g[f"{name}_lpips_sf"]).max() == 0.0, name


def test_empty_mask_and_identical_images():
    from pgdvs_amd.harness import masked_lpips_dycheck, masked_psnr_dycheck, masked_ssim_dycheck

    g = golden()
    gt, pred, m = case(g, "empty")
    assert float(m.sum()) == 0
    assert masked_psnr_dycheck(gt, pred, m) == math.inf
    assert masked_ssim_dycheck(gt, pred, m) == 1.0
    assert masked_lpips_dycheck(gt, pred, m, weights(g)) == 0.0
    gt, _, m = case(g, "ident")
    for mm in (m, torch.ones_like(m)):
        assert masked_psnr_dycheck(gt, gt, mm) == math.inf
        assert masked_ssim_dycheck(gt, gt, mm) == 1.0
        assert masked_lpips_dycheck(gt, gt, mm, weights(g)) == 0.0


def test_scaling_layer_applied_here_but_not_on_the_nvidia_path():
    """The DyCheck LPIPS applies the ScalingLayer; the NVIDIA one does not (harness.masked_lpips).  With the full mask the two
    protocols differ only by that layer (and the spatial vs. nearest-resized averaging, which agree for a full mask up to fp32
    rounding of the upsampling)."""
    from pgdvs_amd.harness import masked_lpips, masked_lpips_dycheck

    g = golden()
    gt, pred, _ = case(g, "a")
    w = weights(g)
    ones = torch.ones(1, *gt.shape[1:])
    dy = masked_lpips_dycheck(gt, pred, ones, w)
    nv_scaled = masked_lpips(gt, pred, ones.repeat(3, 1, 1), w, scaling_layer=True)
    nv_plain = masked_lpips(gt, pred, ones.repeat(3, 1, 1), w)
    assert abs(dy - nv_plain) > 1e-3
    assert abs(dy - nv_scaled) < 1e-2 * abs(dy - nv_plain)
    assert abs(dy - g["a_lpips"][0]) <= 1e-5


def test_small_images_rejected():
    from pgdvs_amd.harness import masked_lpips_dycheck, masked_ssim_dycheck

    x = torch.rand(3, 10, 40)
    with pytest.raises(ValueError):
        masked_ssim_dycheck(x, x, torch.ones(1, 10, 40))
    x = torch.rand(3, 30, 40)
    with pytest.raises(ValueError):
        masked_lpips_dycheck(x, x, torch.ones(1, 30, 40), weights())


def test_lpips_package_weight_file(tmp_path):
    """LpipsAlex takes the lpips package's own weight file (lpips/weights/v0.1/alex.pth: the five lin{k}.model.1.weight) and a
    full LPIPS state dict (scaling_layer buffers, net.slice*, lin*) as well."""
    from pgdvs_amd.harness import LpipsAlex

    g = golden()
    lin = {f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]) for k in range(5)}
    torch.save(lin, tmp_path / "alex.pth")
    bb = {k: torch.from_numpy(v) for k, v in LI.backbone_weights().items()}
    torch.save(bb, tmp_path / "alexnet.pth")
    w = LpipsAlex.from_files(tmp_path / "alexnet.pth", tmp_path / "alex.pth")
    slices = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
    full = {f"net.slice{slices[int(k.split('.')[1])]}.{k.split('.', 1)[1]}": v for k, v in bb.items()}
    full.update(lin)
    full["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188])[None, :, None, None]
    full["scaling_layer.scale"] = torch.tensor([.458, .448, .450])[None, :, None, None]
    w2 = LpipsAlex(full)
    for a, b in zip(w.convs + w.lins, w2.convs + w2.lins):
        assert torch.equal(a, b)
    gt, pred, m = case(g, "a")
    from pgdvs_amd.harness import masked_lpips_dycheck

    np.testing.assert_allclose(masked_lpips_dycheck(gt, pred, m, w), g["a_lpips"][1], rtol=0, atol=1e-5)


def test_quant_type_from_engine_cfg():
    from pgdvs_amd.harness import quant_type_from_engine_cfg
    from pgdvs_amd.instantiate import load_config

    cfg = load_config()
    assert quant_type_from_engine_cfg(cfg.engine.engine_cfg) == "nvidia"
    assert quant_type_from_engine_cfg({"quant_type": "dycheck_iphone"}) == "dycheck_iphone"
    assert quant_type_from_engine_cfg({}) == "nvidia"
    with pytest.raises(ValueError):
        quant_type_from_engine_cfg({"quant_type": "llff"})


# ---------------------------------------------------------------- eval_step(quant_type="dycheck_iphone") on CPU tensors
def _fake_model(pred):
    class Fake(torch.nn.Module):
        def forward(self, data_gpu, render_cfg=None, disable_tqdm=True, for_debug=False):
            return {"combined_rgb": pred}

    return Fake()


def _batch(strided=False, seed=8):
    rng = np.random.default_rng(seed)
    B, H, W = 2, 48, 72
    rh, rw = (40, 60) if strided else (H, W)
    pred = torch.from_numpy(rng.normal(0.5, 0.3, (B, 3, rh, rw)).astype(np.float32))
    pred[0, 1, 2, 3] = float("nan")
    gt = torch.from_numpy((0.2 + 0.6 * rng.random((B, H, W, 3))).astype(np.float32))
    mask = torch.from_numpy((rng.random((B, H, W, 1)) < 0.4).astype(np.float32))
    return pred, {"rgb_src_temporal": torch.zeros(B, 2, H, W, 3), "rgb_tgt": gt, "eval_mask": mask, "misc": [{}] * B}


@pytest.mark.parametrize("strided", [False, True])
def test_eval_step_dycheck_on_cpu(strided):
    from pgdvs_amd.harness import (DYCHECK_KEYS, DYCHECK_LPIPS_KEYS, eval_step, masked_lpips_dycheck, masked_psnr_dycheck,
                                   masked_ssim_dycheck)

    pred, data = _batch(strided)
    w = weights()
    md0 = eval_step(_fake_model(pred), data, "rc", device="cpu", quant_type="dycheck_iphone")
    assert set(md0) == {"eval/count"} | {f"eval/{k}" for k in DYCHECK_KEYS}
    md, ex = eval_step(_fake_model(pred), data, "rc", device="cpu", quant_type="dycheck_iphone", lpips=w, return_images=True)
    assert set(md) == set(md0) | {f"eval/{k}" for k in DYCHECK_LPIPS_KEYS}
    assert int(md["eval/count"]) == 2 and md["eval/count"].dtype == torch.int64
    for k in md0:
        assert md[k].numpy().tobytes() == md0[k].numpy().tobytes(), k
    for b in range(2):
        g, p, m = ex["gt"][b], ex["pred"][b], ex["eval_mask"][b]
        ones = torch.ones_like(m)
        want = {"psnr_combined": masked_psnr_dycheck(g, p, ones), "ssim_combined": masked_ssim_dycheck(g, p, ones),
                "mpsnr_combined": masked_psnr_dycheck(g, p, m), "mssim_combined": masked_ssim_dycheck(g, p, m),
                "lpips_combined": masked_lpips_dycheck(g, p, ones, w), "mlpips_combined": masked_lpips_dycheck(g, p, m, w)}
        for k, v in want.items():
            np.testing.assert_allclose(ex["per_view"][k][b], v, rtol=1e-6, atol=1e-7)
    for k in DYCHECK_KEYS + DYCHECK_LPIPS_KEYS:
        assert md[f"eval/{k}"].dtype == torch.float32 and md[f"eval/{k}"].device.type == "cpu"
        np.testing.assert_allclose(float(md[f"eval/{k}"]), float(np.float32(sum(np.float32(v) for v in ex["per_view"][k]))), rtol=1e-6)
    assert 5 < float(md["eval/psnr_combined"]) / 2 < 40 and 0 < float(md["eval/mssim_combined"]) / 2 < 1


def test_eval_step_dycheck_does_not_touch_the_default():
    from pgdvs_amd.harness import METRIC_KEYS, eval_step

    pred, data = _batch()
    d3 = dict(data, eval_mask=data["eval_mask"].repeat(1, 1, 1, 3))
    before = eval_step(_fake_model(pred), d3, "rc", device="cpu")
    eval_step(_fake_model(pred), data, "rc", device="cpu", quant_type="dycheck_iphone")
    after = eval_step(_fake_model(pred), d3, "rc", device="cpu", quant_type="nvidia")
    assert set(after) == {"eval/count"} | {f"eval/{k}" for k in METRIC_KEYS}
    for k in before:
        assert before[k].numpy().tobytes() == after[k].numpy().tobytes(), k


def test_eval_step_dycheck_errors():
    from pgdvs_amd.harness import eval_step

    pred, data = _batch()
    with pytest.raises(ValueError):
        eval_step(_fake_model(pred), data, "rc", device="cpu", quant_type="dycheck_iphone", with_ssim=True)
    with pytest.raises(ValueError):
        eval_step(_fake_model(pred), dict(data, eval_mask=data["eval_mask"].repeat(1, 1, 1, 3)), "rc", device="cpu",
                  quant_type="dycheck_iphone")
    with pytest.raises(ValueError):
        eval_step(_fake_model(pred), data, "rc", device="cpu", quant_type="llff")
