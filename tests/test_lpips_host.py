"""The evaluator's masked LPIPS without a GPU: harness.masked_lpips (the float32 torch restatement) against the reference's
own PerceptualLoss (tests/golden/lpips.npz, made by tests/golden/make_golden_lpips.py), the ScalingLayer quirk the fixture
pins, torch's nearest-resize index rule that the HIP head restates, weight loading, and eval_step(lpips=...) on CPU
tensors."""
import io
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import lpips_inputs as LI  # noqa: E402


def golden():
    return dict(np.load(GOLDEN / "lpips.npz"))


def lin_state(g):
    return {f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]) for k in range(5)}


def backbone_state():
    return {k: torch.from_numpy(v) for k, v in LI.backbone_weights().items()}


def weights(device="cpu"):
    from pgdvs_amd.harness import LpipsAlex

    return LpipsAlex(backbone_state(), lin_state(golden()), device)


def case(g, name):
    """quantised gt / pred [3,H,W] and the dynamic mask [3,H,W]"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)  # noqa: E731
    gt = T(g[f"{name}_gt"].astype(np.float32) / np.float32(255))
    pred = T(g[f"{name}_pred"].astype(np.float32) / np.float32(255))
    m = T(np.repeat(g[f"{name}_mask"][..., None], 3, axis=-1))
    return gt, pred, m


def test_fixture_matches_the_seeded_backbone():
    np.testing.assert_allclose(golden()["weights_checksum"], LI.checksum(LI.backbone_weights()), rtol=1e-12)


@pytest.mark.parametrize("name", list(LI.CASES))
def test_masked_lpips_vs_reference_golden(name):
    from pgdvs_amd.harness import masked_lpips

    g = golden()
    gt, pred, m = case(g, name)
    w = weights()
    got = [masked_lpips(gt, pred, torch.ones_like(gt), w), masked_lpips(gt, pred, m, w), masked_lpips(gt, pred, 1.0 - m, w)]
    np.testing.assert_allclose(got, g[f"{name}_lpips"], rtol=0, atol=1e-5)
    if name == "ident":
        assert got == [0.0, 0.0, 0.0]
    if LI.CASES[name][2] == "empty":
        assert got[1] == 0.0


def test_features_vs_reference_golden():
    from pgdvs_amd.harness import alex_features

    g = golden()
    gt, pred, _ = case(g, LI.FEATURE_CASE)
    feats = alex_features(2.0 * torch.stack([gt, pred]) - 1.0, weights())
    for k, f in enumerate(feats):
        want = g[f"{LI.FEATURE_CASE}_relu{k + 1}"]
        assert tuple(f.shape) == want.shape
        np.testing.assert_allclose(f.numpy(), want, rtol=0, atol=1e-5 * max(1.0, float(np.abs(want).max())))


def test_scaling_layer_quirk_is_pinned():
    """PNetLin compares version 0.1 (float) with "0.1": no ScalingLayer.  Applying it moves every value well past the
    tolerance, so the fixture tells the two apart."""
    from pgdvs_amd.harness import masked_lpips

    g = golden()
    for name in ("a", "b"):
        gt, pred, m = case(g, name)
        scaled = masked_lpips(gt, pred, m, weights(), scaling_layer=True)
        assert abs(scaled - g[f"{name}_lpips"][1]) > 1e-3, (name, scaled, g[f"{name}_lpips"][1])


@pytest.mark.parametrize("src,dst", [((1080, 1920), (269, 479)), ((1080, 1920), (66, 119)), ((67, 101), (15, 23)),
                                     ((31, 31), (1, 1)), ((135, 240), (7, 14)), ((40, 20), (80, 40)), ((64, 96), (64, 96)),
                                     ((1001, 37), (249, 8))])
def test_nearest_index_rule_matches_interpolate(src, dst):
    """the HIP head's index rule: src = min(floor(dst * (float)in / out), in - 1) with the product in float32"""
    (H, W), (h, w) = src, dst
    ref = F.interpolate(torch.arange(H * W, dtype=torch.float64).reshape(1, 1, H, W), size=[h, w]).reshape(h, w).numpy()

    def idx(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)

    rule = idx(H, h)[:, None] * W + idx(W, w)[None, :]
    np.testing.assert_array_equal(ref, rule.astype(np.float64))


def test_weight_loading_layouts():
    from pgdvs_amd.harness import LpipsAlex

    g = golden()
    tv = backbone_state()
    tv.update({"classifier.1.weight": torch.zeros(4096, 9216), "classifier.1.bias": torch.zeros(4096)})  # ignored
    a = LpipsAlex(tv, lin_state(g))
    # the reference's PNetLin state dict (DataParallel prefixes included): backbone and lin in one
    slices = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
    ref = {}
    for k, v in backbone_state().items():
        i, kind = int(k.split(".")[1]), k.split(".")[2]
        ref[f"module.net.slice{slices[i]}.{i}.{kind}"] = v
    ref.update({f"module.{k}": v for k, v in lin_state(g).items()})
    ref["module.scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    b = LpipsAlex(ref)
    for x, y in ((a.conv_weights, b.conv_weights), (a.conv_biases, b.conv_biases), (a.lin_weights, b.lin_weights)):
        assert torch.equal(x, y)
    assert a.conv_weights.numel() == 2468544 and a.conv_biases.numel() == 1152 and a.lin_weights.numel() == 1152
    bad = dict(tv)
    del bad["features.6.bias"]
    with pytest.raises(KeyError):
        LpipsAlex(bad, lin_state(g))
    bad = dict(tv)
    bad["features.8.weight"] = torch.zeros(256, 384, 5, 5)
    with pytest.raises(ValueError):
        LpipsAlex(bad, lin_state(g))


def test_from_files_with_a_cuda_saved_lin_file(tmp_path, monkeypatch):
    """the reference's alex.pth holds CUDA storages: from_files must load it with map_location="cpu" on a host without a
    GPU.  A file whose storages are tagged "cuda" is written by saving under a patched location tag."""
    from pgdvs_amd.harness import LpipsAlex

    g = golden()
    torch.save(backbone_state(), tmp_path / "alexnet.pth")
    buf = io.BytesIO()
    import torch.serialization as S

    orig = S.location_tag
    monkeypatch.setattr(S, "location_tag", lambda storage: "cuda:0")
    torch.save(lin_state(g), buf)
    monkeypatch.setattr(S, "location_tag", orig)
    (tmp_path / "alex.pth").write_bytes(buf.getvalue())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            torch.load(tmp_path / "alex.pth", weights_only=True)  # (what the file holds: CUDA storages)
    w = LpipsAlex.from_files(tmp_path / "alexnet.pth", tmp_path / "alex.pth")
    assert torch.equal(w.lin_weights, weights().lin_weights)
    assert torch.equal(w.conv_weights, weights().conv_weights)


def test_from_engine_cfg(tmp_path):
    from pgdvs_amd.harness import LpipsAlex
    from pgdvs_amd.instantiate import load_config

    ecfg = load_config(static_renderer="geo").engine.engine_cfg
    assert "lpips_weights" in ecfg and ecfg.lpips_weights is None
    assert LpipsAlex.from_engine_cfg(ecfg) is None
    torch.save(backbone_state(), tmp_path / "alexnet.pth")
    torch.save(lin_state(golden()), tmp_path / "alex.pth")
    w = LpipsAlex.from_engine_cfg({"lpips_weights": {"backbone": str(tmp_path / "alexnet.pth"), "lin": str(tmp_path / "alex.pth")}})
    assert torch.equal(w.conv_biases, weights().conv_biases)


def test_small_images_rejected():
    from pgdvs_amd.harness import masked_lpips

    for H, W in ((30, 64), (64, 30)):
        x = torch.rand(3, H, W)
        with pytest.raises(ValueError):
            masked_lpips(x, x, torch.ones_like(x), weights())


# ---------------------------------------------------------------- eval_step(lpips=...) on CPU tensors
def _fake_model(pred):
    class Fake(torch.nn.Module):
        def forward(self, data_gpu, render_cfg=None, disable_tqdm=True, for_debug=False):
            return {"combined_rgb": pred}

    return Fake()


@pytest.mark.parametrize("strided", [False, True])
def test_eval_step_with_lpips_on_cpu(strided):
    from pgdvs_amd.harness import LPIPS_KEYS, METRIC_KEYS, SSIM_KEYS, eval_step, masked_lpips

    rng = np.random.default_rng(8)
    B, H, W = 2, 48, 72
    rh, rw = (40, 60) if strided else (H, W)
    pred = torch.from_numpy(rng.normal(0.5, 0.3, (B, 3, rh, rw)).astype(np.float32))
    pred[0, 1, 2, 3] = float("nan")
    gt = torch.from_numpy((0.2 + 0.6 * rng.random((B, H, W, 3))).astype(np.float32))  # (no bicubic overshoot past [0, 1])
    mask = torch.from_numpy((rng.random((B, H, W, 1)) < 0.3).astype(np.float32).repeat(3, axis=-1))
    data = {"rgb_src_temporal": torch.zeros(B, 2, H, W, 3), "rgb_tgt": gt, "eval_mask": mask, "misc": [{}] * B}
    w = weights()
    md0 = eval_step(_fake_model(pred), data, "rc", device="cpu", with_ssim=True)
    md, ex = eval_step(_fake_model(pred), data, "rc", device="cpu", with_ssim=True, lpips=w, return_images=True)
    assert set(md) == set(md0) | {f"eval/{k}" for k in LPIPS_KEYS}
    for k in md0:
        assert md[k].numpy().tobytes() == md0[k].numpy().tobytes(), k
    for k in METRIC_KEYS + SSIM_KEYS:
        assert k in ex["per_view"]
    for b in range(B):
        g, p, m = ex["gt"][b], ex["pred"][b], ex["eval_mask"][b]
        want = [masked_lpips(g, p, torch.ones_like(g), w), masked_lpips(g, p, m, w), masked_lpips(g, p, 1.0 - m, w)]
        for k, v in zip(LPIPS_KEYS, want):
            assert ex["per_view"][k][b] == v, k
    for k in LPIPS_KEYS:
        assert md[f"eval/{k}"].dtype == torch.float32
        np.testing.assert_allclose(float(md[f"eval/{k}"]), float(np.float32(sum(np.float32(v) for v in ex["per_view"][k]))),
                                   rtol=1e-6)
    assert float(md["eval/lpips_full_combined"]) > 0
