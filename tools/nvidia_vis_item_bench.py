#!/usr/bin/env python3
"""The NVIDIA-family loaders' per-item depth range (DESIGN.md 8f-3 NVIDIA) at 288 x 550 (the NVIDIA frames) with 10 and 24
spatial views: host time per item of the numpy path (compute_pcl of every spatial view + depth_range_from_points, what
device=None runs) against the device path as the loaders run it (ray constants, host-to-device copies of depth and rays,
ops.nvidia_depth_range, the copy back), the op's GPU time alone (HIP events, inputs resident, median of --reps) with each
kernel's share (the library's event brackets), and the host time of the temporal / tracker-window point clouds the loaders
used to compute and discard (2 + 2 x 5 views).  Checks bit-identity of the two paths on every scene.  Prints one JSON object.
Usage (GPU box): timeout -k 10 600 python tools/nvidia_vis_item_bench.py [--reps 50] [--out profiles/nvidia_vis_item_bench.json]"""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dycheck_item_bench import kernel_split, wall  # noqa: E402
from eval_lpips_bench import event_median  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pgdvs_amd import _lib, ops
    from pgdvs_amd.datasets.nvidia_eval import compute_pcl, ray_rows, spatial_depth_range
    from test_gpu_nvidia_vis import _scene

    dev = torch.device("cuda:0")
    lib = _lib.load()
    rec = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "cases": []}
    for V in (10, 24):
        H, W = 288, 550
        depths, Ks, c2ws, tgt = _scene(V, H, W, V)
        views = {"depth": depths, "K": Ks, "c2w": c2ws}
        want = spatial_depth_range(views, tgt).numpy()
        got = spatial_depth_range(views, tgt, dev).numpy()
        rays = ray_rows(Ks, c2ws)
        d, r = torch.from_numpy(depths).to(dev), torch.from_numpy(rays.astype(np.float32)).to(dev)
        inv = np.linalg.inv(tgt)
        run = lambda: ops.nvidia_depth_range(d, r, inv)  # noqa: E731
        k_med, k_min = event_median(run, args.reps, 1)
        h_np = wall(lambda: spatial_depth_range(views, tgt), args.host_reps)
        h_dev = wall(lambda: spatial_depth_range(views, tgt, dev), args.reps)
        h_discard = wall(lambda: [compute_pcl(H, W, Ks[v % V], c2ws[v % V], depths[v % V]) for v in range(12)], args.host_reps)
        n = V * H * W
        case = {"V": V, "H": H, "W": W, "points": n, "bit_identical": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))),
                "host_numpy_ms_median": h_np[0], "host_numpy_ms_min": h_np[1],
                "host_device_path_ms_median": h_dev[0], "host_device_path_ms_min": h_dev[1],
                "op_gpu_ms_median": k_med, "op_gpu_ms_min": k_min,
                "host_discarded_pcl_12_views_ms_median": h_discard[0],
                "bytes_depth_read": n * 4, "bytes_keys_written": n * 8,
                "kernels": kernel_split(lib, run, 20)}
        rec["cases"].append(case)
    js = json.dumps(rec, indent=1)
    if args.out:
        pathlib.Path(args.out).write_text(js + "\n")
    print(js)


if __name__ == "__main__":
    main()
