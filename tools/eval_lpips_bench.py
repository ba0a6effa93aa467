#!/usr/bin/env python3
"""The evaluator's masked LPIPS pass on the chip (csrc/lpips.hip) at 1080p: `pgdvs_lpips_sums` per view (HIP events,
warm-up, median of --reps), each of its kernels (the library's per-launch event brackets) with the convolutions' fraction of
the fp32 matrix peak, the float32 torch restatement on the same GPU (MIOpen convolutions; backbone alone and the whole
three-mask value), and `harness.eval_step` per view at bench.py's workload (1080p x 24 source frames, the real renderer, one
view in flight, SSIM on in both arms) with and without LPIPS, interleaved in blocks.  Seeded AlexNet weights
(tests/golden/lpips_inputs.py): the time does not depend on their values.  Prints one JSON object.
Usage (GPU box): timeout -k 10 900 python tools/eval_lpips_bench.py [--reps 30] [--views 30]"""
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
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tests" / "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

FP32_MATRIX_PEAK = 157.3e12  # MI355X dense fp32 matrix FLOP/s


def make_weights(dev):
    import lpips_inputs as LI

    from pgdvs_amd.harness import LpipsAlex

    rng = np.random.default_rng(3)
    lin = {f"lin{k}.model.1.weight": torch.from_numpy(np.abs(rng.standard_normal((1, c, 1, 1))).astype(np.float32) * 0.01)
           for k, c in enumerate((64, 192, 384, 256, 256))}
    return LpipsAlex({k: torch.from_numpy(v) for k, v in LI.backbone_weights().items()}, lin, dev)


def conv_flops(H, W):
    from pgdvs_amd import ops

    relu, pool = ops.lpips_map_sizes(H, W)
    shapes = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
    return [2.0 * 2 * co * ci * k * k * h * w for (co, ci, k), (h, w) in zip(shapes, relu)]


def event_median(fn, reps, calls):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / calls)
    return statistics.median(times), min(times)


def hip_pass(dev, H, W, reps, w):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(3, H, W, device=dev, generator=g)
    gt = (pred.permute(1, 2, 0) + 0.05 * torch.randn(H, W, 3, device=dev, generator=g)).contiguous()
    mask = (torch.rand(H, W, 1, device=dev, generator=g) < 0.3).float().expand(H, W, 3).contiguous()
    nws = int(lib.pgdvs_lpips_workspace_bytes(H, W))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = (ptr(pred), ptr(gt), ptr(mask), H, W, ptr(w.conv_weights), ptr(w.conv_biases), ptr(w.lin_weights), ptr(sums), ptr(ws), nws,
            ops._stream())

    def run():
        rc = lib.pgdvs_lpips_sums(*args)
        assert rc == 0, lib.pgdvs_last_error()

    med, mn = event_median(run, reps, 5)
    flops = conv_flops(H, W)
    # per kernel: the library's event brackets (pgdvs_prof_*), their fixed overhead subtracted
    buf = C.create_string_buffer(1 << 16)
    lib.pgdvs_prof_enable(1)
    lib.pgdvs_prof_report(buf, len(buf))
    n = max(10, reps // 2)
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    lib.pgdvs_prof_report(buf, len(buf))
    lib.pgdvs_prof_enable(0)
    kern = {}
    for line in buf.value.decode().strip().splitlines():
        name, calls, total = line.split()
        kern[name] = {"ms_per_view": round(float(total) / n, 4)}
    conv_ms = 0.0
    for k in range(5):
        e = kern.get(f"lpips_conv{k + 1}")
        if e:
            e["gflop"] = round(flops[k] / 1e9, 2)
            e["fraction_of_fp32_matrix_peak"] = round(flops[k] / (e["ms_per_view"] * 1e-3) / FP32_MATRIX_PEAK, 3)
            conv_ms += e["ms_per_view"]
    return {"median_ms_per_view": round(med, 4), "min_ms_per_view": round(mn, 4), "reps": reps, "workspace_mb": round(nws / 2 ** 20, 1),
            "backbone_gflop_per_view": round(sum(flops) / 1e9, 2),
            "conv_fraction_of_fp32_matrix_peak": round(sum(flops) / (conv_ms * 1e-3) / FP32_MATRIX_PEAK, 3) if conv_ms else None,
            "kernels": kern, "lpips_full": round(float(sums[0]), 6),
            "note": "pgdvs_lpips_sums called back to back between HIP events (launch gaps included); per kernel: HIP event "
                    "brackets around each launch (pgdvs_prof_*), bracket overhead subtracted"}


def torch_restatement(dev, H, W, reps, w):
    from pgdvs_amd.harness import _lpips_torch, alex_features

    torch.backends.cudnn.allow_tf32 = False
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.rand(3, H, W, device=dev, generator=g)
    b = (a + 0.05 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1)
    m = (torch.rand(3, H, W, device=dev, generator=g) < 0.3).float()
    x = 2.0 * torch.stack([a, b]) - 1.0
    bb_med, bb_min = event_median(lambda: alex_features(x, w), reps, 2)
    times = []
    _lpips_torch(a, b, [torch.ones_like(a), m, 1.0 - m], w)
    for _ in range(max(5, reps // 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lpips_torch(a, b, [torch.ones_like(a), m, 1.0 - m], w)  # (ends in host reads: synchronised)
        times.append((time.perf_counter() - t0) * 1e3)
    return {"backbone_median_ms": round(bb_med, 4), "backbone_min_ms": round(bb_min, 4),
            "backbone_fraction_of_fp32_matrix_peak": round(sum(conv_flops(H, W)) / (bb_med * 1e-3) / FP32_MATRIX_PEAK, 3),
            "three_values_median_ms_wall": round(statistics.median(times), 4),
            "note": "harness.alex_features (F.conv2d = MIOpen, F.max_pool2d) on both images, HIP events; three_values = "
                    "harness masked_lpips' body for the three masks, backbone once, host wall clock incl. its host reads"}


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
        d_["eval_mask"] = d_["dyn_mask_src_temporal"][:, 0].expand(-1, -1, -1, 3).contiguous()
        views.append(d_)
    for j in range(4):
        harness.eval_step(model, views[j % nv], rc, device=dev, with_ssim=True)
        harness.eval_step(model, views[j % nv], rc, device=dev, with_ssim=True, lpips=w)
    torch.cuda.synchronize()
    per = {False: [], True: []}
    j = 0
    while len(per[True]) < n_views:
        for on in (False, True):
            for _ in range(block):
                t0 = time.perf_counter()
                md = harness.eval_step(model, views[j % nv], rc, device=dev, with_ssim=True, lpips=w if on else None)
                per[on].append((time.perf_counter() - t0) * 1e3)
                j += 1
    off, on = statistics.median(per[False]), statistics.median(per[True])
    return {"size": [H, W, S], "views_each": len(per[True]), "block": block,
            "without_lpips_ms_per_view": round(off, 3), "with_lpips_ms_per_view": round(on, 3), "added_ms": round(on - off, 3),
            "lpips_full_last": round(float(md["eval/lpips_full_combined"]), 6),
            "note": "harness.eval_step per view with SSIM in both arms (forward = one native call, metric passes, one host "
                    "synchronisation), wall clock per call, medians"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--views", type=int, default=30, help="timed eval_step views per arm")
    ap.add_argument("--block", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    from pgdvs_amd import _lib

    _lib.load()
    w = make_weights(dev)
    out = {"hip_1080p": hip_pass(dev, 1080, 1920, args.reps, w),
           "torch_miopen_1080p": torch_restatement(dev, 1080, 1920, args.reps, w),
           "eval_step_1080p_x24": eval_step_times(dev, 1080, 1920, 24, args.views, args.block, w),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
