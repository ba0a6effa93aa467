#!/usr/bin/env python3
"""The DyCheck iPhone protocol's passes on the chip (csrc/eval_dycheck.hip) at 720x960 (the DyCheck iPhone size) and 1080p:
`pgdvs_dycheck_psnr_ssim_sums` and `pgdvs_dycheck_lpips` per view (HIP events, warm-up, median of --reps), each of their
kernels (the library's per-launch event brackets) with the convolutions' fraction of the fp32 matrix peak, the NVIDIA
protocol's SSIM and LPIPS passes on the same inputs for comparison, and `harness.eval_step` per view at bench.py's workload
(1080p x 24 source frames, the real renderer, one view in flight) with the default protocol and with quant_type
"dycheck_iphone" (without and with LPIPS), interleaved in blocks.  Seeded AlexNet weights (tests/golden/lpips_inputs.py).
Prints one JSON object.
Usage (GPU box): timeout -k 10 900 python tools/eval_dycheck_bench.py [--reps 30] [--views 20]"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tests" / "golden"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from eval_lpips_bench import FP32_MATRIX_PEAK, conv_flops, event_median, make_weights  # noqa: E402


def kernel_times(lib, run, n):
    """per kernel ms per call from the library's event brackets (pgdvs_prof_*)"""
    buf = C.create_string_buffer(1 << 16)
    lib.pgdvs_prof_enable(1)
    lib.pgdvs_prof_report(buf, len(buf))
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    lib.pgdvs_prof_report(buf, len(buf))
    lib.pgdvs_prof_enable(0)
    kern = {}
    for line in buf.value.decode().strip().splitlines():
        name, calls, total = line.split()
        kern[name] = {"ms_per_view": round(float(total) / n, 4)}
    return kern


def passes(dev, H, W, reps, w):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(3, H, W, device=dev, generator=g)
    gt = (pred.permute(1, 2, 0) + 0.05 * torch.randn(H, W, 3, device=dev, generator=g)).contiguous()
    m1 = (torch.rand(H, W, 1, device=dev, generator=g) < 0.7).float()
    m3 = m1.expand(H, W, 3).contiguous()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    out = {}

    def ws(n):
        return torch.empty(int(n), dtype=torch.uint8, device=dev)

    n_ps = lib.pgdvs_dycheck_psnr_ssim_workspace_bytes(H, W)
    w_ps = ws(n_ps)
    n_lp = lib.pgdvs_dycheck_lpips_workspace_bytes(H, W)
    w_lp = ws(n_lp)
    n_ss = lib.pgdvs_eval_ssim_workspace_bytes(H, W)
    w_ss = ws(n_ss)
    n_nl = lib.pgdvs_lpips_workspace_bytes(H, W)
    w_nl = ws(n_nl)
    calls = {
        "dycheck_psnr_ssim": lambda: lib.pgdvs_dycheck_psnr_ssim_sums(ptr(pred), ptr(gt), ptr(m1), H, W, None, None, ptr(sums), ptr(w_ps),
                                                                      n_ps, ops._stream()),
        "dycheck_lpips": lambda: lib.pgdvs_dycheck_lpips(ptr(pred), ptr(gt), ptr(m1), H, W, ptr(w.conv_weights), ptr(w.conv_biases),
                                                         ptr(w.lin_weights), ptr(sums), ptr(w_lp), n_lp, ops._stream()),
        "nvidia_ssim": lambda: lib.pgdvs_eval_ssim_sums(ptr(pred), ptr(gt), ptr(m3), H, W, None, ptr(sums), ptr(w_ss), n_ss, ops._stream()),
        "nvidia_lpips": lambda: lib.pgdvs_lpips_sums(ptr(pred), ptr(gt), ptr(m3), H, W, ptr(w.conv_weights), ptr(w.conv_biases),
                                                     ptr(w.lin_weights), ptr(sums), ptr(w_nl), n_nl, ops._stream()),
    }
    flops = conv_flops(H, W)  # (two images)
    for name, fn in calls.items():
        def run(fn=fn, name=name):
            rc = fn()
            assert rc == 0, (name, lib.pgdvs_last_error())

        med, mn = event_median(run, reps, 5)
        e = {"median_ms_per_view": round(med, 4), "min_ms_per_view": round(mn, 4)}
        if name.startswith("dycheck"):
            e["kernels"] = kernel_times(lib, run, max(10, reps // 2))
        if name.endswith("lpips"):
            n_img = 4 if name.startswith("dycheck") else 2
            gf = sum(flops) * n_img / 2
            e["backbone_gflop_per_view"] = round(gf / 1e9, 2)
            if "kernels" in e:
                conv_ms = sum(v["ms_per_view"] for k, v in e["kernels"].items() if k.startswith("lpips_conv"))
                e["conv_ms_per_view"] = round(conv_ms, 4)
                e["conv_fraction_of_fp32_matrix_peak"] = round(gf / (conv_ms * 1e-3) / FP32_MATRIX_PEAK, 3)
        else:
            e["ns_per_pixel"] = round(med * 1e6 / (H * W), 4)
        out[name] = e
    return out


def eval_step_times(dev, H, W, S, n_views, block, w):
    from pgdvs_amd import harness, synth
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer
    from pgdvs_amd.runtime import ResidentVideoRenderer

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cfg = load_config(static_renderer="geo", overrides={"engine.engine_cfg.render_cfg.dyn_pcl_remove_outlier": True,
                                                        "engine.engine_cfg.render_cfg.st_render_pcl_pts_per_pixel": 3})
    rc = cfg.engine.engine_cfg.render_cfg
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(dev).eval()
    video = synth.make_video(S, H, W, seed=1234, scene="nominal")
    rvr = ResidentVideoRenderer(model, rc, T(video["rgbs"]), T(video["depths"]), T(video["dyn_masks"]).view(torch.uint8),
                                video["K3s"], video["c2ws"], lanes=1)
    nv = max(1, min(4, S - 1))
    ids = [int(round(j * (S - 2) / max(nv - 1, 1))) for j in range(nv)]
    views = []
    for i in ids:
        d_ = synth.to_torch(synth.make_view(video, i, frac=0.4, seed=5), dev)
        d_.pop("static_noise", None)
        d_["_st_pcl_video"] = dict(rvr.video, capacity=rvr.row_bound or S * H * W)
        if rvr.row_bound is not None:
            d_["st_pcl_rgb_row_bound"] = rvr.row_bound
        d_["rgb_tgt"] = d_["rgb_src_temporal"][:, 0]
        m = d_["dyn_mask_src_temporal"][:, 0]
        d_["eval_mask"] = m.expand(-1, -1, -1, 3).contiguous()
        views.append((d_, dict(d_, eval_mask=(1.0 - m).contiguous())))
    arms = {"nvidia_default": lambda v: harness.eval_step(model, v[0], rc, device=dev),
            "dycheck": lambda v: harness.eval_step(model, v[1], rc, device=dev, quant_type="dycheck_iphone"),
            "dycheck_lpips": lambda v: harness.eval_step(model, v[1], rc, device=dev, quant_type="dycheck_iphone", lpips=w)}
    for j in range(4):
        for fn in arms.values():
            fn(views[j % nv])
    torch.cuda.synchronize()
    per = {k: [] for k in arms}
    j = 0
    while len(per["dycheck_lpips"]) < n_views:
        for k, fn in arms.items():
            for _ in range(block):
                t0 = time.perf_counter()
                md = fn(views[j % nv])
                per[k].append((time.perf_counter() - t0) * 1e3)
                j += 1
    res = {"size": [H, W, S], "views_each": n_views, "block": block}
    for k, v in per.items():
        res[f"{k}_ms_per_view"] = round(statistics.median(v), 3)
        res[f"{k}_views_per_s"] = round(1e3 / statistics.median(v), 1)
    res["mssim_last"] = round(float(md["eval/mssim_combined"]), 6)
    res["note"] = ("harness.eval_step per view (forward = one native call, metric passes, one host synchronisation), wall clock "
                   "per call, medians; nvidia_default = PSNR only, dycheck = PSNR + SSIM, dycheck_lpips = + LPIPS")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--views", type=int, default=20, help="timed eval_step views per arm")
    ap.add_argument("--block", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    from pgdvs_amd import _lib

    _lib.load()
    w = make_weights(dev)
    out = {"passes_720x960": passes(dev, 720, 960, args.reps, w), "passes_1080p": passes(dev, 1080, 1920, args.reps, w),
           "eval_step_1080p_x24": eval_step_times(dev, 1080, 1920, 24, args.views, args.block, w),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
