"""The evaluator's masked LPIPS on the MI355X (csrc/lpips.hip): each backbone convolution against F.conv2d in float64, the
head against a float64 numpy restatement, the whole pass against the reference's own PerceptualLoss (tests/golden/lpips.npz)
and against harness.masked_lpips at 1080p, quantisation of NaN / out-of-range inputs, soft and empty masks, identical
images, determinism, the size limit, and harness.eval_step(with_ssim=True, lpips=...) around the real HIP renderer."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_lpips_host as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def W_():
    return R.weights(DEV)


def _raw_inputs(H, W, seed, mask_kind):
    """raw render [3,H,W] and ground truth [H,W,3] with NaN, negative and > 1 values; mask [H,W,3]"""
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
    else:
        mask = np.zeros((H, W, 3), np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return T(pred.transpose(2, 0, 1)), T(gt), T(mask)


def _quantised(pred, gt):
    from pgdvs_amd.harness import quantize_like_evaluator

    return quantize_like_evaluator(gt.permute(2, 0, 1)), quantize_like_evaluator(pred)


def _values(sums):
    return [float(v) for v in sums.cpu().numpy()[:3]]


@pytest.mark.parametrize("H,W", [(135, 240), (270, 481)])
def test_each_convolution_vs_conv2d_float64(H, W, W_):
    """relu_k from the kernel against relu(conv2d) in float64 on the kernel's own input to that layer.  Bound: a K-term fp32
    dot product (K = 363 .. 3456) plus the bias is within (K + 1) u sum |w x| + |b| of the exact value, in any order."""
    from pgdvs_amd import ops
    from pgdvs_amd.harness import _ALEX_CONVS

    pred, gt, mask = _raw_inputs(H, W, 3, "binary")
    _, feats = ops.lpips_sums(pred, gt, mask, W_, want_features=True)
    g, p = _quantised(pred, gt)
    x = (2.0 * torch.stack([g, p]) - 1.0).double()
    for j, (_, k, st, pd, pool) in enumerate(_ALEX_CONVS):
        inp = x if j == 0 else feats[j - 1].double()
        if pool:
            inp = F.max_pool2d(inp, kernel_size=3, stride=2)
        w, b = W_.convs[2 * j].double(), W_.convs[2 * j + 1].double()
        want = F.relu(F.conv2d(inp, w, b, stride=st, padding=pd))
        absc = F.conv2d(inp.abs(), w.abs(), b.abs(), stride=st, padding=pd)
        K = w[0].numel()
        got = feats[j].double()
        assert got.shape == want.shape, (j, got.shape, want.shape)
        err = (got - want).abs()
        bound = (K + 1) * U * absc + 1e-30
        worst = float((err / bound).max())
        assert worst <= 1.0, (j, K, worst, float(err.max()))


@pytest.mark.parametrize("mask_kind", ["binary", "soft", "empty"])
def test_head_vs_float64_restatement(mask_kind, W_):
    """the head and the final ratios from the kernel's own relu maps, restated in float64 numpy (normalise, subtract, square,
    weight; the mask's channel 0 resampled by torch's nearest rule)"""
    from pgdvs_amd import ops

    H, W = 135, 240
    pred, gt, mask = _raw_inputs(H, W, 5, mask_kind)
    sums, feats = ops.lpips_sums(pred, gt, mask, W_, want_features=True)
    got = _values(sums)
    m = mask[..., 0].double()[None, None]
    want = [0.0, 0.0, 0.0]
    for f, lin in zip(feats, W_.lins):
        f = f.double().cpu().numpy()
        n = f / (np.sqrt(np.sum(f ** 2, axis=1, keepdims=True)) + 1e-10)
        d = np.einsum("c,chw->hw", lin.double().cpu().numpy().reshape(-1), (n[0] - n[1]) ** 2)
        mr = F.interpolate(m, size=list(d.shape)).cpu().numpy()[0, 0]
        for j, w in enumerate((np.ones_like(mr), mr, 1.0 - mr)):
            want[j] += float(np.sum(d * w) / (np.sum(w) + 1e-8))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-9)
    s = sums.cpu().numpy()
    relu1 = feats[0].shape[2:]
    assert s[3] == relu1[0] * relu1[1] and s[6] == 0 and s[7] == 0
    if mask_kind == "empty":
        assert got[1] == 0.0 and s[4] == 0


@pytest.mark.parametrize("name", list(R.LI.CASES))
def test_full_pass_vs_reference_golden(name, W_):
    from pgdvs_amd import ops

    g = R.golden()
    gt, pred, m = (t.to(DEV) for t in R.case(g, name))
    sums, _ = ops.lpips_sums(pred.contiguous(), gt.permute(1, 2, 0).contiguous(), m.permute(1, 2, 0).contiguous(), W_)
    got = _values(sums)
    np.testing.assert_allclose(got, g[f"{name}_lpips"], rtol=0, atol=1e-4)
    if name == "ident":
        assert got == [0.0, 0.0, 0.0]


def test_1080p_vs_masked_lpips_on_the_gpu(W_):
    from pgdvs_amd import ops
    from pgdvs_amd.harness import masked_lpips

    pred, gt, mask = _raw_inputs(1080, 1920, 7, "binary")
    got = _values(ops.lpips_sums(pred, gt, mask, W_)[0])
    g, p = _quantised(pred, gt)
    m = mask.permute(2, 0, 1)
    want = [masked_lpips(g, p, torch.ones_like(g), W_), masked_lpips(g, p, m, W_), masked_lpips(g, p, 1.0 - m, W_)]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
    assert got[0] > 0


@pytest.mark.parametrize("mask_kind", ["soft", "empty"])
def test_quantisation_and_masks(mask_kind, W_):
    """raw inputs with NaN / negative / > 1 values give the values of their quantised images; soft and empty masks"""
    from pgdvs_amd import ops
    from pgdvs_amd.harness import masked_lpips

    pred, gt, mask = _raw_inputs(97, 203, 9, mask_kind)
    a = ops.lpips_sums(pred, gt, mask, W_)[0].cpu().numpy()
    g, p = _quantised(pred, gt)
    b = ops.lpips_sums(p.contiguous(), g.permute(1, 2, 0).contiguous(), mask, W_)[0].cpu().numpy()
    assert a.tobytes() == b.tobytes()
    m = mask.permute(2, 0, 1)
    want = [masked_lpips(g, p, torch.ones_like(g), W_), masked_lpips(g, p, m, W_), masked_lpips(g, p, 1.0 - m, W_)]
    np.testing.assert_allclose(a[:3], want, rtol=0, atol=1e-4)
    if mask_kind == "empty":
        assert a[1] == 0.0


def test_identical_images_give_zero_and_runs_are_bit_identical(W_):
    from pgdvs_amd import ops

    pred, gt, mask = _raw_inputs(1080, 1920, 13, "soft")
    same = ops.lpips_sums(gt.permute(2, 0, 1).contiguous(), gt, mask, W_)[0].cpu().numpy()
    assert list(same[:3]) == [0.0, 0.0, 0.0]
    a = ops.lpips_sums(pred, gt, mask, W_)[0].cpu().numpy()
    b = ops.lpips_sums(pred, gt, mask, W_)[0].cpu().numpy()
    assert a.tobytes() == b.tobytes() and a[0] > 0


def test_small_images_rejected_by_ops_and_the_c_abi(W_):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    pred, gt, mask = _raw_inputs(40, 40, 1, "binary")
    assert lib.pgdvs_lpips_workspace_bytes(31, 31) > 0
    for H, W in ((30, 40), (40, 30)):
        with pytest.raises(ValueError):
            ops.lpips_sums(pred[:, :H, :W].contiguous(), gt[:H, :W].contiguous(), mask[:H, :W].contiguous(), W_)
        assert lib.pgdvs_lpips_workspace_bytes(H, W) < 0
        sums = torch.zeros(8, dtype=torch.float64, device=DEV)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = lib.pgdvs_lpips_sums(ptr(pred), ptr(gt), ptr(mask), H, W, ptr(W_.conv_weights), ptr(W_.conv_biases), ptr(W_.lin_weights),
                                  ptr(sums), ptr(ws), ws.numel(), ops._stream())
        assert rc < 0 and b"31" in lib.pgdvs_last_error()
    torch.cuda.synchronize()


def _fake_model(pred):
    class Fake(torch.nn.Module):
        def forward(self, data_gpu, render_cfg=None, disable_tqdm=True, for_debug=False):
            return {"combined_rgb": pred}

    return Fake()


def test_eval_step_fused_lpips_vs_torch_path(W_):
    from pgdvs_amd.harness import LPIPS_KEYS, METRIC_KEYS, SSIM_KEYS, eval_step

    B, H, W = 2, 120, 200
    ins = [_raw_inputs(H, W, 40 + b, "binary") for b in range(B)]
    pred = torch.stack([i[0] for i in ins])
    data_gpu = {"rgb_src_temporal": torch.zeros(B, 2, H, W, 3, device=DEV), "rgb_tgt": torch.stack([i[1] for i in ins]),
                "eval_mask": torch.stack([i[2] for i in ins]), "misc": [{}] * B}
    data_cpu = {k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in data_gpu.items()}
    md0 = eval_step(_fake_model(pred), data_gpu, "rc", device=DEV, with_ssim=True)
    md, ex = eval_step(_fake_model(pred), data_gpu, "rc", device=DEV, with_ssim=True, lpips=W_, return_images=True)
    md_cpu, ex_cpu = eval_step(_fake_model(pred.cpu()), data_cpu, "rc", device="cpu", with_ssim=True, lpips=R.weights(),
                               return_images=True)
    assert set(md) == set(md_cpu) == set(md0) | {f"eval/{k}" for k in LPIPS_KEYS}
    for k in md0:
        assert md[k].numpy().tobytes() == md0[k].numpy().tobytes(), k
    for k in LPIPS_KEYS:
        assert md[f"eval/{k}"].dtype == torch.float32 and md[f"eval/{k}"].device.type == "cpu"
        np.testing.assert_allclose(ex["per_view"][k], ex_cpu["per_view"][k], rtol=0, atol=1e-4, err_msg=k)
    assert all(k in ex["per_view"] for k in METRIC_KEYS + SSIM_KEYS)


def test_eval_step_with_ssim_and_lpips_around_the_hip_renderer(W_):
    from pgdvs_amd import synth
    from pgdvs_amd.datasets.static_aggregation import aggregate_static_pcl
    from pgdvs_amd.harness import LPIPS_KEYS, eval_step, masked_lpips
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
    md0 = eval_step(model, data, rc, device=DEV, with_ssim=True)
    md, ex = eval_step(model, data, rc, device=DEV, return_images=True, with_ssim=True, lpips=W_)
    for k in md0:  # PSNR / SSIM (and the count) bit-identical with LPIPS on
        assert md[k].numpy().tobytes() == md0[k].numpy().tobytes(), k
    g, p, m = ex["gt"][0], ex["pred"][0], ex["eval_mask"][0]
    want = [masked_lpips(g, p, torch.ones_like(g), W_), masked_lpips(g, p, m, W_), masked_lpips(g, p, 1.0 - m, W_)]
    for k, w in zip(LPIPS_KEYS, want):
        assert abs(ex["per_view"][k][0] - w) <= 1e-4, (k, ex["per_view"][k][0], w)
        assert abs(float(md[f"eval/{k}"]) - w) <= 1e-4, k
    assert float(md["eval/lpips_full_combined"]) > 0
