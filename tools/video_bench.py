#!/usr/bin/env python3
"""Times the video codec's two device calls (csrc/jpeg.hip) on one frame at 4:4:4 and at 4:2:0, in one process, alternated
call by call, so that both see the same box in the same state: ``--height`` x ``--width`` at ``--quality``,
a synthetic render and uniform noise, the restart interval one MCU row (``--segment-blocks N``: the MCUs that hold N blocks
instead, N / 3 at 4:4:4 and N / 6 at 4:2:0, so that both samplings give a workgroup the same number of blocks).  Per sampling and content: ``ops.jpeg_coefficients``,
``ops.jpeg_scan`` and the two together, device events round each call, Python wrapper included, outputs preallocated, the
median of ``--iters`` calls after ``--warmup`` with the minimum beside it; the bytes of the frame's JPEG file; and whether
the device stream equals the host coder's.  Prints one JSON line (``--out``: also written there)."""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ml-pgdvs_amd"))

SAMPLINGS = ("4:4:4", "4:2:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--segment-blocks", type=int, default=0)
    ap.add_argument("--out", type=pathlib.Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_bench needs the GPU: a time taken elsewhere says nothing")
    from pgdvs_amd import ops, png, synth, video

    dev = "cuda:0"
    H, W, q = args.height, args.width, args.quality
    contents = {
        "render": torch.from_numpy(np.ascontiguousarray(synth.make_video(1, H, W, seed=5)["rgbs"])).permute(0, 3, 1, 2).contiguous(),
        "noise": torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(9)),
    }
    result = {"H": H, "W": W, "quality": q, "warmup": args.warmup, "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "restart": f"{args.segment_blocks} blocks" if args.segment_blocks else "one MCU row", "ms": {}, "jpeg_bytes": {}, "scan_bytes": {}, "equals_host": {}}
    for name, x in contents.items():
        xd = x.to(dev)
        calls = {}
        for s in SAMPLINGS:
            nmy, nmx = video.mcu_grid(H, W, s)
            bpm = video.BLOCKS_PER_MCU[s]
            coef = torch.empty((1, nmy, nmx, bpm, 64), dtype=torch.int16, device=dev)
            restart = max(1, args.segment_blocks // bpm) if args.segment_blocks else nmx
            out = torch.empty((1, ops.jpeg_scan_capacity(nmy, nmx, restart, bpm)), dtype=torch.uint8, device=dev)
            ops.jpeg_coefficients(xd, q, out=coef, subsampling=s)
            data, nbytes = ops.jpeg_scan(coef, restart, out=out)
            n = int(nbytes[0])
            q8 = png.quantize_save_image(x[0]).permute(1, 2, 0).contiguous().numpy()
            host = video.encode_scan(video.jpeg_coefficients(q8, q, subsampling=s), restart)
            result["equals_host"][f"{name} {s}"] = data[0, :n].cpu().numpy().tobytes() == host
            result["scan_bytes"][f"{name} {s}"] = n
            result["jpeg_bytes"][f"{name} {s}"] = len(video.jpeg_frame(host, H, W, q, restart, s))
            calls[("coefficients", s)] = lambda s=s, coef=coef: ops.jpeg_coefficients(xd, q, out=coef, subsampling=s)
            calls[("scan", s)] = lambda coef=coef, out=out, restart=restart: ops.jpeg_scan(coef, restart, out=out)
            calls[("together", s)] = lambda s=s, coef=coef, out=out, restart=restart: ops.jpeg_scan(
                ops.jpeg_coefficients(xd, q, out=coef, subsampling=s), restart, out=out)
        for what in ("coefficients", "scan", "together"):
            times = {s: [] for s in SAMPLINGS}
            for it in range(args.warmup + args.iters):
                for s in SAMPLINGS:  # alternated: a drift of the box falls on both alike
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    calls[(what, s)]()
                    t1.record()
                    t1.synchronize()
                    if it >= args.warmup:
                        times[s].append(t0.elapsed_time(t1))
            for s in SAMPLINGS:
                result["ms"][f"{name} {s} {what}"] = {"median": round(float(np.median(times[s])), 4), "min": round(float(np.min(times[s])), 4)}
    line = json.dumps(result)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
