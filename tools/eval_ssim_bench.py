#!/usr/bin/env python3
"""The evaluator's masked SSIM pass on the chip (csrc/eval_ssim.hip): `pgdvs_eval_ssim_sums` alone at 1080p (HIP events,
warm-up, median of --reps), its bytes read per second against the 8 TB/s HBM peak, and `harness.eval_step` per view at
bench.py's workload (1080p x 24 source frames, the real renderer, one view in flight) with and without `with_ssim`,
interleaved in blocks so that clock drift hits both alike.  Prints one JSON object.
Usage (GPU box): timeout -k 10 900 python tools/eval_ssim_bench.py [--reps 200] [--views 40]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12


def kernel_time(dev, H, W, reps, calls=20):
    """`pgdvs_eval_ssim_sums` called through the C ABI with preallocated buffers, `calls` launches back to back between two
    HIP events (so the host's enqueue cost is not in the interval), per-call time = interval / calls; median over reps"""
    import ctypes as C

    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(3, H, W, device=dev, generator=g)
    gt = torch.rand(H, W, 3, device=dev, generator=g)
    mask = (torch.rand(H, W, 1, device=dev, generator=g) < 0.3).float().expand(H, W, 3).contiguous()
    nws = int(lib.pgdvs_eval_ssim_workspace_bytes(H, W))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    smap = torch.empty_like(pred)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    for want_map in (False, True):
        args = (ptr(pred), ptr(gt), ptr(mask), H, W, ptr(smap) if want_map else C.c_void_p(0), ptr(sums), ptr(ws), nws, ops._stream())

        def run(n):
            for _ in range(n):
                rc = lib.pgdvs_eval_ssim_sums(*args)
                assert rc == 0, lib.pgdvs_last_error()

        run(10)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(calls)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / calls)
        us = statistics.median(times)
        nbytes = 3 * H * W * 4 * 3 + (3 * H * W * 4 if want_map else 0)  # pred + gt + mask read (+ map written)
        out["with_map" if want_map else "sums_only"] = {
            "median_us": round(us, 2), "min_us": round(min(times), 2), "reps": reps, "calls_per_rep": calls, "bytes": nbytes,
            "bytes_per_s": round(nbytes / (us * 1e-6) / 1e9, 1), "fraction_of_8TBps": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}
    out["note"] = ("per view: the partials kernel and the fixed-order final sum, C entry point called back to back between "
                   "HIP events (launch gaps included, host enqueue cost not)")
    return out


def eval_step_times(dev, H, W, S, n_views, block):
    from pgdvs_amd import harness, synth
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer
    from pgdvs_amd.runtime import ResidentVideoRenderer

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cfg = load_config(static_renderer="geo", overrides={"engine.engine_cfg.render_cfg.dyn_pcl_remove_outlier": True,
                                                        "engine.engine_cfg.render_cfg.st_render_pcl_pts_per_pixel": 3})
    rc = cfg.engine.engine_cfg.render_cfg
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(dev).eval()
    # bench.py's scene and its eval_step inputs (ground truth = a source frame, mask = its dynamic mask)
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
        harness.eval_step(model, views[j % nv], rc, device=dev)
        harness.eval_step(model, views[j % nv], rc, device=dev, with_ssim=True)
    torch.cuda.synchronize()
    per = {False: [], True: []}
    j = 0
    while len(per[True]) < n_views:
        for ssim in (False, True):  # blocks of `block` views, alternating
            for _ in range(block):
                t0 = time.perf_counter()
                md = harness.eval_step(model, views[j % nv], rc, device=dev, with_ssim=ssim)
                per[ssim].append((time.perf_counter() - t0) * 1e3)
                j += 1
    off, on = statistics.median(per[False]), statistics.median(per[True])
    return {"size": [H, W, S], "views_each": len(per[True]), "block": block,
            "without_ssim_ms_per_view": round(off, 3), "with_ssim_ms_per_view": round(on, 3),
            "without_ssim_mean_ms": round(statistics.mean(per[False]), 3), "with_ssim_mean_ms": round(statistics.mean(per[True]), 3),
            "ratio_median": round(on / off, 4), "ssim_full_last": round(float(md["eval/ssim_full_combined"]), 5),
            "note": "harness.eval_step per view (forward = one native call incl. the static aggregation, metric passes, one host "
                    "synchronisation), wall clock per call, medians"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--views", type=int, default=40, help="timed eval_step views per arm")
    ap.add_argument("--block", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    from pgdvs_amd import _lib

    _lib.load()
    out = {"kernel_1080p": kernel_time(dev, 1080, 1920, max(50, args.reps)),
           "eval_step_1080p_x24": eval_step_times(dev, 1080, 1920, 24, args.views, args.block),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
