#!/usr/bin/env python3
"""Times the two preprocessing kernels (csrc/preprocess.hip) against the same computation written in torch-ROCm ops, on the
GPU, with device events around ``--iters`` back-to-back calls after ``--warmup`` ("Preprocessing").  Prints one
JSON line per (op, size).  The torch expressions are the comparison only; the package never calls them."""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ml-pgdvs_amd"))


def torch_flow_consistency(f12, f21):
    """both directions, upstream's own tensor ops (coords_grid, bilinear_sampler, compute_occlusion)"""
    H, W = f12.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, device=f12.device), torch.arange(W, device=f12.device), indexing="ij")
    c0 = torch.stack([xs, ys], -1).float()
    out = []
    for a, b in ((f12, f21), (f21, f12)):
        c1 = c0 + a
        g = torch.stack([2 * c1[..., 0] / (W - 1) - 1, 2 * c1[..., 1] / (H - 1) - 1], -1)
        s = F.grid_sample(b.permute(2, 0, 1)[None], g[None], align_corners=True)[0].permute(1, 2, 0)
        out.append(c0 - (c1 + s))
    return out


def torch_epipolar_mask(flow, cd, Fm, consist_thres=1.0, threshold=1.0):
    H, W = flow.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    p = torch.stack([xs, ys], -1).float()
    p2 = (p + flow).double()
    p1 = torch.stack([xs.double(), ys.double(), torch.ones_like(xs, dtype=torch.float64)], 0).reshape(3, -1)
    l = (Fm @ p1).reshape(3, H, W)
    d = torch.abs((p2[..., 0] * l[0] + p2[..., 1] * l[1] + l[2]) / (torch.sqrt(l[0] ** 2 + l[1] ** 2) + 1e-8))
    raw = (d * (cd.abs().sum(-1) <= consist_thres)) > threshold

    def cross(x, pad, fn):
        q = F.pad(x[None, None].float(), (1, 1, 1, 1), value=pad)[0, 0]
        return fn(fn(fn(q[1:-1, 1:-1], q[:-2, 1:-1]), fn(q[2:, 1:-1], q[1:-1, :-2])), q[1:-1, 2:])

    return cross(cross(raw, 1.0, torch.minimum), 0.0, torch.maximum) > 0


def time_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--iters", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs the GPU: a time taken elsewhere says nothing")
    from pgdvs_amd import ops

    dev = "cuda:0"
    Fm = np.array([[1e-6, 2e-5, -3e-3], [-2e-5, 1e-6, 2e-2], [3e-3, -2e-2, 1.0]])
    Ft = torch.from_numpy(Fm).to(dev)
    for H, W in ((288, 550), (1080, 1920)):
        g = torch.Generator(device="cpu").manual_seed(H)
        f12 = (torch.randn(H, W, 2, generator=g) * 3).to(dev)
        f21 = (-f12 + torch.randn(H, W, 2, generator=g) * 0.5).to(dev)
        cd = ops.flow_consistency(f12, f21)[0]
        # the comparison computes the same thing (the masks' pixels near a threshold aside)
        ref = torch_flow_consistency(f12, f21)[0]
        agree = float(((cd - ref).abs().amax(-1) < 1e-3).float().mean())
        same = float((ops.epipolar_mask(f12, cd, Fm).bool() == torch_epipolar_mask(f12, cd, Ft)).float().mean())
        rows = {
            "flow_consistency": (lambda: ops.flow_consistency(f12, f21), lambda: torch_flow_consistency(f12, f21),
                                 2 * H * W * 8 * 3, agree),  # per direction: own flow, the other flow once, the output
            "epipolar_mask": (lambda: ops.epipolar_mask(f12, cd, Fm), lambda: torch_epipolar_mask(f12, cd, Ft),
                              H * W * (8 + 8 + 1), same),
        }
        for name, (hip, ref_fn, nbytes, agreement) in rows.items():
            t_hip, t_ref = time_us(hip, args.warmup, args.iters), time_us(ref_fn, args.warmup, max(args.iters // 10, 10))
            print(json.dumps({"op": name, "H": H, "W": W, "hip_us_per_call": round(t_hip, 2), "torch_us_per_call": round(t_ref, 2),
                              "min_bytes": nbytes, "hip_gb_per_s_incl_launch": round(nbytes / t_hip / 1e3, 1),
                              "agreement_share": round(agreement, 6), "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
