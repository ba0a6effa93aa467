#!/usr/bin/env python3
"""CoTracker's correlation step at its working size: ops.cotracker_pyramid + ops.cotracker_corr_lookup (csrc/cotracker.hip)
against the torch statement (CorrBlock: avg_pool2d, matmul, grid_sample) on the same device, in the same run.

One refinement window: the pyramid is built once, the look-up runs `--iters` times (6 in the predictor).  Device events
around each leg, the two legs alternated `--repeats` times after a warm-up of both; medians are printed, and one JSON line.

  python tools/cotracker_lookup_bench.py [--S 8 --H 96 --W 128 --N 4132 --iters 6 --repeats 7]
"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ml-pgdvs_amd"))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("S", 8), ("H", 96), ("W", 128), ("N", 4132), ("iters", 6), ("repeats", 7)):
        ap.add_argument(f"--{name}", type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from pgdvs_amd import ops
    from pgdvs_amd.models.cotracker.blocks import CorrBlock

    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(0)
    fmaps = torch.randn((1, a.S, 128, a.H, a.W), generator=g).to(dev)
    feats = torch.randn((1, a.S, a.N, 128), generator=g).to(dev)
    coords = (torch.rand((1, a.S, a.N, 2), generator=g) * torch.tensor([a.W - 1.0, a.H - 1.0])).to(dev)
    tokens = torch.empty((a.S, a.N, 456), device=dev)

    def hip():
        pyr = ops.cotracker_pyramid(fmaps[0])
        for _ in range(a.iters):
            ops.cotracker_corr_lookup(pyr, feats[0], coords[0], out=tokens, col_offset=130)
        return tokens[:, :, 130:326]

    def hip_lookup_only(pyr):
        ops.cotracker_corr_lookup(pyr, feats[0], coords[0], out=tokens, col_offset=130)

    def torch_statement():
        blk = CorrBlock(fmaps, num_levels=4, radius=3)
        for _ in range(a.iters):
            blk.corr(feats)
            out = blk.sample(coords)
        return out[0]

    def timed(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        diff = float((hip() - torch_statement()).abs().max())  # also the warm-up of both
        torch.cuda.synchronize()
        peak0 = torch.cuda.max_memory_allocated()
        t_hip, t_torch, t_look = [], [], []
        pyr = ops.cotracker_pyramid(fmaps[0])
        for _ in range(a.repeats):
            t_hip.append(timed(hip))
            t_torch.append(timed(torch_statement))
            t_look.append(timed(hip_lookup_only, pyr))
        torch.cuda.reset_peak_memory_stats()
        hip()
        torch.cuda.synchronize()
        mem_hip = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch_statement()
        torch.cuda.synchronize()
        mem_torch = torch.cuda.max_memory_allocated()
    tap_bytes = a.S * a.N * 4 * 64 * 512  # 8 x 8 tap lines of 512 bytes per (s, n, level), before the level's borders
    rec = dict(S=a.S, H=a.H, W=a.W, N=a.N, iters=a.iters, repeats=a.repeats,
               hip_ms=statistics.median(t_hip), hip_ms_all=t_hip, torch_ms=statistics.median(t_torch), torch_ms_all=t_torch,
               hip_lookup_ms=statistics.median(t_look), gathered_GB_per_lookup=tap_bytes / 1e9,
               gathered_TB_per_s=tap_bytes / 1e12 / (statistics.median(t_look) / 1e3),
               peak_bytes_hip=mem_hip, peak_bytes_torch=mem_torch, peak_bytes_before=peak0, max_abs_diff=diff)
    print(f"pyramid + {a.iters} look-ups: HIP {rec['hip_ms']:.3f} ms, torch statement {rec['torch_ms']:.3f} ms "
          f"(one look-up {rec['hip_lookup_ms']:.3f} ms, {rec['gathered_TB_per_s']:.2f} TB/s of tap lines); peak memory "
          f"{mem_hip / 1e9:.2f} GB against {mem_torch / 1e9:.2f} GB; max |HIP - torch| {diff:.3g}", file=sys.stderr)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
