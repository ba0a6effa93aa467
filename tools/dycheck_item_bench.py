#!/usr/bin/env python3
"""The DyCheck loader's per-item depth range (DESIGN.md 8f-3 DyCheck) at 360 x 480 (the 2x iPhone frames) with 10 and 40
spatial views: host time per item of the numpy path (compute_pcl + depth_range_numpy, what device=None runs) against the
device path as the loader runs it (host-to-device copies of depth / mask / ray constants, ops.dycheck_depth_range, the copy
back), and the op's GPU time alone (HIP events, inputs resident, median of --reps), with each kernel's share (the library's
event brackets).  Checks bit-identity of the two paths on every scene.  Prints one JSON object.
Usage (GPU box): timeout -k 10 600 python tools/dycheck_item_bench.py [--reps 50] [--out profiles/dycheck_item_bench.json]"""
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
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from eval_lpips_bench import event_median  # noqa: E402
from pgdvs_amd.datasets._common import ray_rows  # noqa: E402


def scene(V, H, W, seed):
    from test_gpu_dycheck_dataset import _scene

    return _scene(V, H, W, seed)


def host_numpy(s, near, far):
    from pgdvs_amd.datasets.dycheck_iphone import compute_pcl, depth_range_numpy

    V, H, W = s["depth"].shape
    pcl = np.concatenate([compute_pcl(H, W, M, o, d) for (M, o), d in zip(s["rays"], s["depth"])], axis=0)
    return depth_range_numpy(pcl, s["dyn"], s["raw_c2w_tgt"], s["flat_cam_tgt"], near, far, H, W)


def host_device(s, near, far, dev):
    from pgdvs_amd import ops

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rays = ray_rows(s["rays"])
    out = ops.dycheck_depth_range(T(s["depth"]), T(s["dyn"]), T(rays), np.linalg.inv(s["raw_c2w_tgt"]),
                                  np.linalg.inv(s["flat_cam_tgt"][18:34].reshape(4, 4)), s["K3"], near, far)
    return out.cpu().numpy()


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def kernel_split(lib, run, n):
    buf = C.create_string_buffer(1 << 16)
    lib.pgdvs_prof_enable(1)
    lib.pgdvs_prof_report(buf, len(buf))
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    lib.pgdvs_prof_report(buf, len(buf))
    lib.pgdvs_prof_enable(0)
    return buf.value.decode().strip().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pgdvs_amd import _lib, ops

    dev = "cuda:0"
    lib = _lib.load()
    near, far = 0.5, 4.0
    rec = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "cases": []}
    for V in (10, 40):
        H, W = 360, 480
        s = scene(V, H, W, seed=1)
        want = host_numpy(s, near, far)
        got = host_device(s, near, far, dev)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        rays = T(ray_rows(s["rays"]))
        d, m = T(s["depth"]), T(s["dyn"])
        A, B = np.linalg.inv(s["raw_c2w_tgt"]), np.linalg.inv(s["flat_cam_tgt"][18:34].reshape(4, 4))
        run = lambda: ops.dycheck_depth_range(d, m, rays, A, B, s["K3"], near, far)  # noqa: E731
        k_med, k_min = event_median(run, args.reps, 1)
        h_np = wall(lambda: host_numpy(s, near, far), args.host_reps)
        h_dev = wall(lambda: host_device(s, near, far, dev), args.reps)
        n = V * H * W
        case = {"V": V, "H": H, "W": W, "points": n, "bit_identical": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))),
                "host_numpy_ms_median": h_np[0], "host_numpy_ms_min": h_np[1],
                "host_device_path_ms_median": h_dev[0], "host_device_path_ms_min": h_dev[1],
                "op_gpu_ms_median": k_med, "op_gpu_ms_min": k_min,
                "bytes_points_read": n * (4 + 4), "bytes_keys_written": n * 4,
                "kernels": kernel_split(lib, run, 20)}
        rec["cases"].append(case)
    js = json.dumps(rec, indent=1)
    if args.out:
        pathlib.Path(args.out).write_text(js + "\n")
    print(js)


if __name__ == "__main__":
    main()
