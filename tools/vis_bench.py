#!/usr/bin/env python3
"""The visualiser's export on a seeded synthetic video through the point-renderer path, at 1080p x 24 and
288 x 550 x 24 frames:
  kernel   GPU time of ops.png_scanlines alone on a rendered view (HIP events, median, input resident, warmed), adaptive and
           not, beside the least time for its bytes (12 H W read + H (1 + 3 W) written over the measured HBM rate of
           MI355X_MICROARCH.md, 6.29 TB/s), as a share of that bound
  loop     views/s of harness.vis_run over --views views (the static cloud aggregated once per scene and resident, as the
           reference's datasets do) with the PngWriter at 1, 8 and 16 threads, against a baseline measured in the same
           process and alternated with it: the reference's export restated (forward, .clamp(0, 1), save_image's expression,
           .cpu(), PIL.Image.save at its default level, synchronously per view); the forward-only rate (no export) as the
           ceiling; bytes written by each; the writer in device mode (deflate="device": ops.png_deflate on the copy stream,
           the workers fetch, wrap and write) at 8 and 16 threads in the same alternation
  deflate  GPU time of ops.png_deflate alone (HIP events, median, warmed, output preallocated) on the resident scanlines of a
           rendered view and of uniform noise, for segments of 8192, 16384 and 32768 bytes, with the stream's bytes beside
           zlib level 1's and zlib's Z_RLE strategy's on the same scanlines
Prints one JSON object.
Usage (GPU box): timeout -k 10 900 python tools/vis_bench.py [--views 64] [--rounds 2] [--out profiles/vis_bench.json]"""
import argparse
import json
import pathlib
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from eval_lpips_bench import event_median  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # MI355X_MICROARCH.md: measured float4 copy


class ResidentCloudRenderer:
    """the renderer with the scene's aggregated static cloud resident on the GPU: adds it to every batch (batch size 1)"""

    def __init__(self, model, cloud, count, xyz):
        self.model, self.extra = model, {"st_pcl_rgb": cloud[None], "st_pcl_rgb_count": count, "st_pcl_xyz": xyz[None]}
        self.training = False

    def eval(self):
        return self

    def forward(self, data, **kw):
        return self.model.forward(dict(data, **self.extra), **kw)


class Views:
    def __init__(self, views, n):
        self.views, self.n = views, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        item = {k: v[0] for k, v in self.views[i % len(self.views)].items()}
        item["misc"] = {"scene_id": "synth", "tgt_idx": i}
        return item


def tree_bytes(d):
    return sum(p.stat().st_size for p in pathlib.Path(d).rglob("*.png"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--baseline-views", type=int, default=16, help="views per round of the PIL baseline (about a second each at 1080p)")
    ap.add_argument("--distinct", type=int, default=16, help="distinct target views the loop cycles through")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="1080x1920,288x550")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import PIL.Image

    from pgdvs_amd import harness, ops, png, synth
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    assert torch.cuda.is_available(), "vis_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cfg = load_config(static_renderer="geo")
    rc = cfg.engine.engine_cfg.render_cfg
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(dev).eval()
    scratch = pathlib.Path(tempfile.mkdtemp(prefix="vis_bench_"))
    rec = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "views": args.views,
           "baseline_views": args.baseline_views, "rounds": args.rounds, "zlib_level": 1, "cases": []}
    try:
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            S = args.frames
            video = synth.make_video(S, H, W, seed=1234)
            cloud, count, xyz = ops.static_aggregate(T(video["rgbs"]), T(video["depths"]), T(video["dyn_masks"]).view(torch.uint8),
                                                     video["K3s"], video["c2ws"], capacity=S * H * W, return_xyz=True)
            ids = [int(round(j * (S - 2) / max(args.distinct - 1, 1))) for j in range(args.distinct)]
            views = []
            for j, i in enumerate(ids):
                d = synth.to_torch(synth.make_view(video, i, frac=0.1 + 0.8 * j / max(len(ids) - 1, 1), seed=5), dev)
                d.pop("static_noise", None)
                views.append(d)
            renderer = ResidentCloudRenderer(model, cloud, count, xyz)
            ds = Views(views, args.views)
            fwd = lambda i: renderer.forward(harness.collate([ds[i]]), render_cfg=rc, disable_tqdm=True, for_debug=False)  # noqa: E731

            with torch.no_grad():
                img = fwd(0)["combined_rgb"].clone()
            torch.cuda.synchronize()
            case = {"H": H, "W": W, "frames": S, "static_points": int(count.reshape(-1)[0].item()),
                    "bytes_read": 12 * H * W, "bytes_written": H * (1 + 3 * W)}
            bound_ms = (case["bytes_read"] + case["bytes_written"]) / HBM_BYTES_PER_S * 1e3
            case["streaming_bound_ms"] = bound_ms
            out = torch.empty((1, H, 1 + 3 * W), dtype=torch.uint8, device=dev)
            for name, adaptive in (("adaptive", True), ("plain", False)):
                med, mn = event_median(lambda: ops.png_scanlines(img, adaptive=adaptive, out=out), args.reps, 4)  # noqa: B023
                case[f"png_scanlines_{name}_ms_median"], case[f"png_scanlines_{name}_ms_min"] = med, mn
                case[f"png_scanlines_{name}_share_of_bound"] = bound_ms / med
            types = np.bincount(ops.png_scanlines(img)[0, :, 0].cpu().numpy(), minlength=5).tolist()
            case["filter_types_chosen"] = types
            import zlib

            case["png_deflate"] = {}
            noise = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
            for name, x in (("render", img), ("noise", noise)):
                scan = ops.png_scanlines(x)
                raw = scan.cpu().numpy().tobytes()
                co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
                entry = {"scanline_bytes": len(raw), "zlib_level_1_bytes": len(zlib.compress(raw, 1)),
                         "zlib_rle_bytes": len(co.compress(raw) + co.flush())}
                for seg in (8192, 16384, 32768):
                    buf = torch.empty((1, ops.png_deflate_capacity(len(raw), seg)), dtype=torch.uint8, device=dev)
                    med, mn = event_median(lambda: ops.png_deflate(scan, seg, out=buf), args.reps, 4)  # noqa: B023
                    n = int(ops.png_deflate(scan, seg, out=buf)[1][0])
                    assert zlib.decompress(buf[0, :n].cpu().numpy().tobytes()) == raw
                    entry[f"seg_{seg}"] = {"ms_median": med, "ms_min": mn, "bytes": n}
                case["png_deflate"][name] = entry
            del noise

            def forward_only(n):
                t0 = time.perf_counter()
                with torch.no_grad():
                    for i in range(n):
                        fwd(i)
                torch.cuda.synchronize()
                return n / (time.perf_counter() - t0), 0

            def baseline(n):
                d = scratch / f"base_{H}"
                shutil.rmtree(d, ignore_errors=True)
                d.mkdir(parents=True)
                t0 = time.perf_counter()
                with torch.no_grad():
                    for i in range(n):
                        rgb = fwd(i)["combined_rgb"].clamp(0.0, 1.0)
                        arr = rgb[0].mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
                        PIL.Image.fromarray(arr).save(d / f"{i:05d}_combined.png")
                dt = time.perf_counter() - t0
                return n / dt, tree_bytes(d)

            def ours(threads, deflate="zlib"):
                def run(n):
                    d = scratch / f"ours_{H}_{threads}_{deflate}"
                    shutil.rmtree(d, ignore_errors=True)
                    t0 = time.perf_counter()
                    with png.PngWriter(n_threads=threads, deflate=deflate) as w:
                        harness.vis_run(renderer, Views(views, n), rc, d, device=dev, writer=w)
                    dt = time.perf_counter() - t0
                    return n / dt, tree_bytes(d)
                return run

            forward_only(8)  # warm-up
            runs = [("forward_only", forward_only, args.views), ("baseline_pil_default", baseline, args.baseline_views),
                    ("writer_1_thread", ours(1), args.views), ("writer_8_threads", ours(8), args.views),
                    ("writer_16_threads", ours(16), args.views), ("device_writer_8_threads", ours(8, "device"), args.views),
                    ("device_writer_16_threads", ours(16, "device"), args.views)]
            rates = {k: [] for k, _, _ in runs}
            sizes = {}
            for _ in range(args.rounds):  # alternated: every round runs each variant once
                for k, fn, n in runs:
                    r, b = fn(n)
                    rates[k].append(r)
                    sizes[k] = (b, n)
            case["views_per_s"] = {k: {"rounds": v, "best": max(v)} for k, v in rates.items()}
            case["bytes_per_view"] = {k: b / n for k, (b, n) in sizes.items() if b}
            rec["cases"].append(case)
            del views, ds, renderer, cloud, xyz
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    js = json.dumps(rec, indent=1)
    if args.out:
        pathlib.Path(args.out).write_text(js + "\n")
    print(js)


if __name__ == "__main__":
    main()
