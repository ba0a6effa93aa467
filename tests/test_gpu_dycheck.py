"""The DyCheck iPhone metric protocol on the MI355X (csrc/eval_dycheck.hip): the PSNR + SSIM pass against a float64 numpy
restatement from 11x11 to 1080p (NaN and out-of-range inputs; binary, soft, empty and full masks) and against the reference's
own metrics.py (tests/golden/dycheck.npz), the LPIPS pass against the golden and against harness.masked_lpips_dycheck at
720x960, determinism, the size limits in ops and the C ABI, and eval_step(quant_type="dycheck_iphone") around the real HIP
renderer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metric_cases as M
import test_dycheck_host as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def W_():
    return R.weights(device=DEV)


def _raw_inputs(H, W, seed, mask_kind):
    """raw render [3,H,W] and ground truth [H,W,3] with NaN, negative and > 1 values; mask [H,W,1]"""
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
        mask = ((rng.random((H, W, 1)) < 0.3) | (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.3 * min(H, W)) ** 2)[..., None])
        mask = mask.astype(np.float32)
    elif mask_kind == "soft":
        mask = rng.random((H, W, 1)).astype(np.float32)
    elif mask_kind == "full":
        mask = np.ones((H, W, 1), np.float32)
    else:
        mask = np.zeros((H, W, 1), np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return T(pred.transpose(2, 0, 1)), T(gt), T(mask)


def _q(x):
    """the evaluator's quantisation in numpy: clamp, NaN -> 0, 8-bit code / 255 (float32)"""
    x = np.nan_to_num(np.clip(np.asarray(x, np.float32), 0, 1), nan=0.0)
    return (x * np.float32(255)).astype(np.uint8).astype(np.float32) / np.float32(255)


def _np_reference(pred, gt, mask):
    """the float64 numpy restatement of metrics.py:63-186 (metric_cases.dycheck_reference) on the quantised images: psnr, ssim,
    mpsnr, mssim"""
    return M.dycheck_reference(_q(gt.cpu().numpy()), _q(pred.cpu().numpy().transpose(1, 2, 0)), mask.cpu().numpy()[..., 0])[0]


def _values(row, H, W):
    """the row of ops.dycheck_psnr_ssim_sums -> psnr, ssim, mpsnr, mssim (as harness.eval_step forms them)"""
    s = row.cpu().numpy()
    db = lambda n, d: math.inf if n / max(d, 1e-6) == 0 else -10.0 / math.log(10.0) * math.log(n / max(d, 1e-6))  # noqa: E731
    n_map = 3.0 * (H - 10) * (W - 10)
    return [db(s[0], s[3]), s[2] / n_map, db(s[1], s[4]), s[5] / n_map]


@pytest.mark.parametrize("name", R.CASES)
def test_psnr_ssim_vs_reference_golden(name):
    from pgdvs_amd import ops

    g = R.golden()
    gt, pred, m = R.case(g, name)  # already quantised: the kernel's quantisation leaves them unchanged
    H, W = gt.shape[1:]
    row = ops.dycheck_psnr_ssim_sums(pred.to(DEV).contiguous(), gt.permute(1, 2, 0).contiguous().to(DEV), m[0, ..., None].to(DEV))
    got = _values(row, H, W)
    R.close(got, g[f"{name}_psnr_ssim"], 1e-5)
    s = row.cpu().numpy()
    assert s[3] == 3 * H * W and s[6] == -1 and s[7] == 0


@pytest.mark.parametrize("H,W,kind", [(11, 11, "binary"), (11, 40, "soft"), (31, 31, "binary"), (45, 77, "empty"),
                                      (360, 480, "soft"), (720, 960, "binary"), (720, 960, "full"), (1080, 1920, "binary")])
def test_psnr_ssim_vs_numpy(H, W, kind):
    from pgdvs_amd import ops

    pred, gt, mask = _raw_inputs(H, W, H + W, kind)
    cnt = torch.tensor([1234], dtype=torch.int64, device=DEV)
    st = torch.tensor([7], dtype=torch.int32, device=DEV)
    row = ops.dycheck_psnr_ssim_sums(pred, gt, mask, count_dev=cnt, status_dev=st)
    got = _values(row, H, W)
    want = _np_reference(pred, gt, mask)
    R.close(got, want, 1e-5)
    s = row.cpu().numpy()
    assert s[6] == 1234 and s[7] == 7
    if kind == "empty":
        assert got[2] == math.inf and got[3] == 1.0


def test_identical_images_and_empty_mask_exact():
    from pgdvs_amd import ops

    pred, gt, mask = _raw_inputs(64, 80, 3, "empty")
    same = gt.permute(2, 0, 1).contiguous()
    got = _values(ops.dycheck_psnr_ssim_sums(same, gt, mask), 64, 80)
    assert got[0] == math.inf and got[1] == 1.0 and got[2] == math.inf and got[3] == 1.0


def test_determinism(W_):
    from pgdvs_amd import ops

    pred, gt, mask = _raw_inputs(720, 960, 5, "binary")
    a = ops.dycheck_psnr_ssim_sums(pred, gt, mask).cpu().numpy()
    b = ops.dycheck_psnr_ssim_sums(pred, gt, mask).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    a = ops.dycheck_lpips(pred, gt, mask, W_).cpu().numpy()
    b = ops.dycheck_lpips(pred, gt, mask, W_).cpu().numpy()
    assert a.tobytes() == b.tobytes() and a[0] > 0 and a[1] > 0


@pytest.mark.parametrize("name", [n for n in R.CASES])
def test_lpips_vs_reference_golden(name, W_):
    from pgdvs_amd import ops

    g = R.golden()
    gt, pred, m = R.case(g, name)
    s = ops.dycheck_lpips(pred.to(DEV).contiguous(), gt.permute(1, 2, 0).contiguous().to(DEV), m[0, ..., None].to(DEV), W_).cpu().numpy()
    np.testing.assert_allclose(s[:2], g[f"{name}_lpips"], rtol=0, atol=1e-4)
    if name in ("ident",):
        assert s[0] == 0.0 and s[1] == 0.0
    if name in ("empty", "dark"):
        assert s[1] == 0.0 and s[5] == 0.0


@pytest.mark.parametrize("H,W,kind", [(720, 960, "binary"), (200, 300, "soft"), (64, 64, "empty")])
def test_lpips_vs_torch(H, W, kind, W_):
    from pgdvs_amd import ops
    from pgdvs_amd.harness import masked_lpips_dycheck, quantize_like_evaluator

    pred, gt, mask = _raw_inputs(H, W, 77 + H, kind)
    s = ops.dycheck_lpips(pred, gt, mask, W_).cpu().numpy()
    g, p = quantize_like_evaluator(gt.permute(2, 0, 1)), quantize_like_evaluator(pred)
    m = mask[..., 0]
    want = [masked_lpips_dycheck(g, p, torch.ones_like(m), W_), masked_lpips_dycheck(g, p, m, W_)]
    np.testing.assert_allclose(s[:2], want, rtol=0, atol=1e-4)
    assert s[3] == H * W
    np.testing.assert_allclose(s[5], float(m.double().sum()), rtol=1e-12)


def test_small_images_rejected_by_ops_and_the_c_abi(W_):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    pred, gt, mask = _raw_inputs(40, 40, 1, "binary")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sums = torch.zeros(8, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    assert lib.pgdvs_dycheck_psnr_ssim_workspace_bytes(11, 11) > 0
    for H, W in ((10, 40), (40, 10)):
        with pytest.raises(ValueError):
            ops.dycheck_psnr_ssim_sums(pred[:, :H, :W].contiguous(), gt[:H, :W].contiguous(), mask[:H, :W].contiguous())
        assert lib.pgdvs_dycheck_psnr_ssim_workspace_bytes(H, W) < 0
        rc = lib.pgdvs_dycheck_psnr_ssim_sums(ptr(pred), ptr(gt), ptr(mask), H, W, None, None, ptr(sums), ptr(ws), ws.numel(), ops._stream())
        assert rc < 0 and b"11" in lib.pgdvs_last_error()
    assert lib.pgdvs_dycheck_lpips_workspace_bytes(31, 31) > 0
    for H, W in ((30, 40), (40, 30)):
        with pytest.raises(ValueError):
            ops.dycheck_lpips(pred[:, :H, :W].contiguous(), gt[:H, :W].contiguous(), mask[:H, :W].contiguous(), W_)
        assert lib.pgdvs_dycheck_lpips_workspace_bytes(H, W) < 0
        rc = lib.pgdvs_dycheck_lpips(ptr(pred), ptr(gt), ptr(mask), H, W, ptr(W_.conv_weights), ptr(W_.conv_biases),
                                     ptr(W_.lin_weights), ptr(sums), ptr(ws), ws.numel(), ops._stream())
        assert rc < 0 and b"31" in lib.pgdvs_last_error()
    with pytest.raises(ValueError):  # a three-channel mask is the NVIDIA protocol's
        ops.dycheck_psnr_ssim_sums(pred, gt, mask.repeat(1, 1, 3))
    torch.cuda.synchronize()


def test_eval_step_fused_vs_torch_path(W_):
    from pgdvs_amd.harness import DYCHECK_KEYS, DYCHECK_LPIPS_KEYS, eval_step

    B, H, W = 2, 120, 200
    ins = [_raw_inputs(H, W, 40 + b, "binary") for b in range(B)]
    pred = torch.stack([i[0] for i in ins])
    data_gpu = {"rgb_src_temporal": torch.zeros(B, 2, H, W, 3, device=DEV), "rgb_tgt": torch.stack([i[1] for i in ins]),
                "eval_mask": torch.stack([i[2] for i in ins]), "misc": [{}] * B}
    data_cpu = {k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in data_gpu.items()}
    md, ex = eval_step(R._fake_model(pred), data_gpu, "rc", device=DEV, quant_type="dycheck_iphone", lpips=W_, return_images=True)
    md_cpu, ex_cpu = eval_step(R._fake_model(pred.cpu()), data_cpu, "rc", device="cpu", quant_type="dycheck_iphone", lpips=R.weights(),
                               return_images=True)
    assert set(md) == set(md_cpu) == {"eval/count"} | {f"eval/{k}" for k in DYCHECK_KEYS + DYCHECK_LPIPS_KEYS}
    for k in DYCHECK_KEYS + DYCHECK_LPIPS_KEYS:
        assert md[f"eval/{k}"].dtype == torch.float32 and md[f"eval/{k}"].device.type == "cpu"
        np.testing.assert_allclose(ex["per_view"][k], ex_cpu["per_view"][k], rtol=0, atol=1e-4, err_msg=k)


def test_eval_step_dycheck_around_the_hip_renderer(W_):
    from pgdvs_amd import synth
    from pgdvs_amd.datasets.static_aggregation import aggregate_static_pcl
    from pgdvs_amd.harness import DYCHECK_KEYS, DYCHECK_LPIPS_KEYS, eval_step
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
    covis = (1.0 - v["dyn_masks"][1][None, ..., None]).astype(np.float32)
    data = {k: torch.from_numpy(np.ascontiguousarray(x)) for k, x in d.items()}
    data["st_pcl_rgb"] = cloud[None].cpu()
    data["rgb_tgt"] = torch.from_numpy(gt)
    data["misc"] = [{"scene_id": "synthetic", "tgt_frame_id": 1, "tgt_cam_id": 0}]
    nv = dict(data, eval_mask=torch.from_numpy(np.repeat(1.0 - covis, 3, axis=-1)))
    dy = dict(data, eval_mask=torch.from_numpy(covis))
    md_nv0 = eval_step(model, nv, rc, device=DEV, with_ssim=True, lpips=W_)
    md, ex = eval_step(model, dy, rc, device=DEV, quant_type="dycheck_iphone", lpips=W_, return_images=True)
    md_nv1 = eval_step(model, nv, rc, device=DEV, with_ssim=True, lpips=W_)
    for k in md_nv0:  # the default protocol is unchanged by a DyCheck step in between
        assert md_nv1[k].numpy().tobytes() == md_nv0[k].numpy().tobytes(), k
    g, p, m = ex["gt"][0].cpu(), ex["pred"][0].cpu(), ex["eval_mask"][0].cpu()
    md_t, ex_t = eval_step(R._fake_model(p[None]), {"rgb_src_temporal": torch.zeros(1, 2, H, W, 3), "rgb_tgt": g.permute(1, 2, 0)[None],
                                                    "eval_mask": m.permute(1, 2, 0)[None], "misc": [{}]},
                           "rc", device="cpu", quant_type="dycheck_iphone", lpips=R.weights(), return_images=True)
    for k in DYCHECK_KEYS + DYCHECK_LPIPS_KEYS:
        np.testing.assert_allclose(ex["per_view"][k], ex_t["per_view"][k], rtol=0, atol=1e-4, err_msg=k)
    assert math.isfinite(float(md["eval/psnr_combined"])) and float(md["eval/lpips_combined"]) > 0
