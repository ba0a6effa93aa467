#!/usr/bin/env python3
"""Where the time of one flow pair goes after the network ("Preprocessing"): both ``.npz`` and both colour-wheel
``.png`` of a 1080p pair whose flows the model left on the GPU, by three routes, each split into GPU time (HIP events,
median of ``--reps`` after a warm-up), host-to-device and device-to-host copies, host arithmetic, ``np.savez`` and the
deflate (``zlib`` level 1, as ``png.PngWriter``):

  host     everything in numpy: the flows come down, coord_diff_numpy, flow_to_image, filter_scanlines
  device0  the device path before ``ops.flow_pair_export``: the flows come down and go up again for ``ops.flow_consistency``,
           the pictures through the host's flow_to_image and filter_scanlines
  device1  ``ops.flow_pair_export`` on the model's tensors; flows, coord_diff and scanlines come down once

Prints one JSON line per route.  Times in ms per pair, medians; the files go to a temporary directory."""
import argparse
import json
import pathlib
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ml-pgdvs_amd"))


class Split:
    def __init__(self):
        self.parts = {}

    def host(self, key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.parts[key] = self.parts.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    def gpu(self, key, fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        self.parts[key] = self.parts.get(key, 0.0) + t0.elapsed_time(t1)
        return out


def finish(s, tmp, flows, cds, lines):
    s.host("savez_ms", lambda: [np.savez(tmp / f"{k}.npz", flow=f, coord_diff=c) for k, (f, c) in enumerate(zip(flows, cds))])
    s.host("deflate_ms", lambda: [zlib.compress(np.ascontiguousarray(ln).tobytes(), 1) for ln in lines])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_export_bench needs the GPU: a time taken elsewhere says nothing")
    from pgdvs_amd import ops
    from pgdvs_amd.png import filter_scanlines
    from pgdvs_amd.preprocess.flow import coord_diff_numpy, flow_to_image

    dev = "cuda:0"
    H, W = args.height, args.width
    g = torch.Generator(device="cpu").manual_seed(H)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    smooth = torch.stack([8 * torch.sin(xs / 97.0) + 3 * torch.cos(ys / 53.0), 6 * torch.cos(xs / 71.0) - 4 * torch.sin(ys / 89.0)], -1)
    g12 = (smooth + torch.randn(H, W, 2, generator=g) * 0.3).to(dev)  # what the model returned, permuted: [H,W,2] on the GPU
    g21 = (-smooth + torch.randn(H, W, 2, generator=g) * 0.3).to(dev)

    def host_pictures(s, flows):
        return s.host("host_arithmetic_ms", lambda: [filter_scanlines(flow_to_image(f)) for f in flows])

    def route_host(s, tmp):
        flows = s.host("d2h_ms", lambda: [g12.cpu().numpy(), g21.cpu().numpy()])
        cds = s.host("host_arithmetic_ms", lambda: [coord_diff_numpy(flows[0], flows[1]), coord_diff_numpy(flows[1], flows[0])])
        finish(s, tmp, flows, cds, host_pictures(s, flows))

    def route_device0(s, tmp):
        flows = s.host("d2h_ms", lambda: [g12.cpu().numpy(), g21.cpu().numpy()])
        up = s.host("h2d_ms", lambda: [torch.from_numpy(f).to(dev) for f in flows])
        cd = s.gpu("gpu_ms", lambda: ops.flow_consistency(up[0], up[1]))
        cds = s.host("d2h_ms", lambda: [c.cpu().numpy() for c in cd])
        finish(s, tmp, flows, cds, host_pictures(s, flows))

    def route_device1(s, tmp):
        cd1, cd2, _, lines = s.gpu("gpu_ms", lambda: ops.flow_pair_export(g12, g21, adaptive=True))
        down = s.host("d2h_ms", lambda: [t.cpu().numpy() for t in (g12, g21, cd1, cd2, lines)])
        finish(s, tmp, down[:2], down[2:4], down[4])

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for name, route, reps in (("host", route_host, args.host_reps), ("device0", route_device0, args.reps), ("device1", route_device1, args.reps)):
            route(Split(), tmp)  # warm-up: allocator, code objects, page cache
            runs = []
            for _ in range(reps):
                s = Split()
                route(s, tmp)
                runs.append(s.parts)
            keys = ("gpu_ms", "h2d_ms", "d2h_ms", "host_arithmetic_ms", "savez_ms", "deflate_ms")
            med = {k: round(statistics.median(r.get(k, 0.0) for r in runs), 3) for k in keys}
            print(json.dumps({"route": name, "H": H, "W": W, "reps": reps, **med, "total_ms": round(sum(med.values()), 3)}), flush=True)


if __name__ == "__main__":
    main()
