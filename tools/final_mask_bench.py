#!/usr/bin/env python3
"""Times one frame of the final motion mask (csrc/mask_combine.hip) against the host path (numpy and scipy.ndimage, as
upstream runs it) on the same box and inputs: ``--height`` x ``--width`` with ``--segments`` segments that already sit on
the device, as a SAM-style segmenter leaves them, and a previous state ("Preprocessing: the final motion mask").
The device call is timed with device events around ``--iters`` calls after ``--warmup``; its kernels one by one with the
library's own event brackets (pgdvs_prof_*), from which the count pass's bytes per second follow: it reads
n_seg H W bytes once.  Calls on ONE segment tensor find part of it in the 256 MB last-level cache, so the kernels are timed
a second time over ``--rotate`` copies of it used in turn (together well above that cache): the rate to quote for a video,
where every frame's segments are new.  The host path with a wall clock around ``--host-iters`` calls.  Prints one JSON
line."""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ml-pgdvs_amd"))


def scene(H, W, n_seg, seed=0):
    """a frame in the middle of a video: a few moving objects, segments that tile the image as blocks of varying size"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    raw = np.zeros((H, W), bool)
    for _ in range(6):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.03, 0.12) * H
        raw |= (xs - cx) ** 2 + (ys - cy) ** 2 < r * r
    raw |= rng.random((H, W)) < 0.01
    sam = np.zeros((n_seg, H, W), bool)
    for s in range(n_seg):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        rx, ry = rng.uniform(0.02, 0.2) * W, rng.uniform(0.02, 0.2) * H
        sam[s] = (np.abs(xs - cx) < rx) & (np.abs(ys - cy) < ry)
    flow = np.stack([3.3 + 2 * np.sin(ys / 90.0), -1.7 + np.cos(xs / 110.0)], -1).astype(np.float32)
    cd = (0.4 * rng.random((H, W, 2))).astype(np.float32)
    cd[:, : W // 8] += 1.0
    return raw, sam, flow, cd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--segments", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("final_mask_bench needs the GPU: a time taken elsewhere says nothing")
    from pgdvs_amd import _lib
    from pgdvs_amd.preprocess import combine_masks

    dev = "cuda:0"
    H, W, n_seg = args.height, args.width, args.segments
    raw, sam, flow, cd = scene(H, W, n_seg)
    first = combine_masks(mask_type="flow_epi", img_idx=6, mask_sam=sam, mask_flow_epi=raw)
    prev_mask, prev_cnt = first["next_prev"], first["dyn_cnt"] * np.float32(5)
    kw = dict(mask_type="flow_epi", img_idx=7, mask_flow_epi=raw, bwd_flow=flow, bwd_coord_diff=cd)
    on_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(kw, mask_sam=sam, prev_mask_final_raw=prev_mask,
                                                                                    prev_dyn_cnt=prev_cnt).items() if hasattr(v, "shape")}
    run = lambda: combine_masks(device=dev, **dict(kw, **on_dev))  # noqa: E731
    copies = [on_dev["mask_sam"]] + [on_dev["mask_sam"].clone() for _ in range(args.rotate - 1)]
    turn = [0]

    def run_rotating():
        turn[0] += 1
        return combine_masks(device=dev, **dict(kw, **dict(on_dev, mask_sam=copies[turn[0] % len(copies)])))

    t = time.perf_counter()
    for _ in range(args.host_iters):
        want = combine_masks(mask_sam=sam, prev_mask_final_raw=prev_mask, prev_dyn_cnt=prev_cnt, **kw)
    host_ms = (time.perf_counter() - t) * 1e3 / args.host_iters
    got = run()
    from pgdvs_amd.preprocess.final_mask import segment_counts, segments_selected

    selected = segments_selected(*segment_counts(sam, want["raw_eroded"])).sum()
    differing = {k: int((got[k].cpu().numpy().view(np.uint8) != want[k].view(np.uint8)).sum()) for k in want if want[k] is not None}

    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        run()
    t1.record()
    torch.cuda.synchronize()
    hip_ms = t0.elapsed_time(t1) / args.iters

    lib = _lib.load()

    def kernel_ms(fn):
        buf = C.create_string_buffer(1 << 16)
        lib.pgdvs_prof_enable(1)
        lib.pgdvs_prof_report(buf, len(buf))
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        lib.pgdvs_prof_report(buf, len(buf))
        lib.pgdvs_prof_enable(0)
        return {line.split()[0]: round(float(line.split()[2]) / args.iters, 4) for line in buf.value.decode().strip().splitlines()}

    rate = lambda k: round(n_seg * H * W / (k["mask_seg_count"] * 1e-3) / 1e9, 1)  # noqa: E731
    same, rotating = kernel_ms(run), kernel_ms(run_rotating)
    print(json.dumps({"H": H, "W": W, "segments": n_seg, "segments_selected": int(selected), "bytes_differing_from_host": differing,
                      "hip_ms_per_frame": round(hip_ms, 4), "host_numpy_ms_per_frame": round(host_ms, 1), "count_pass_bytes": n_seg * H * W,
                      "kernel_ms_one_tensor": same, "count_pass_GBps_one_tensor": rate(same), "rotate": len(copies),
                      "kernel_ms_rotating": rotating, "count_pass_GBps_rotating": rate(rotating)}))


if __name__ == "__main__":
    main()
