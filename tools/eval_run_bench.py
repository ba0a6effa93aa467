#!/usr/bin/env python3
"""The evaluator's loop on a seeded synthetic video through the point-renderer path at 1080p x 24 frames, the
static cloud aggregated once and resident.  One step per process, each writing its part of the result:
  --step loop     views/s of a plain loop over harness.eval_step (one view per step, collated as the loop collates), three
                  runs; with --tree DIR the package and library of another checkout (the parent commit's, built there) are
                  measured instead of this one's, on the same machine
  --step run      views/s of harness.eval_run with run_ahead 0, 1, 2, 3, three rounds alternated
  --step save     the same with save_individual=True and a PngWriter of 8 threads (--save-views views)
  --step export   GPU time (HIP events, median) of ops.eval_export_scanlines on a rendered view against its streaming bound
                  (the bytes of three float images read and three scanline images written over the measured HBM rate of
                  MI355X_MICROARCH.md, 6.29 TB/s) and against what it replaces: three ops.png_scanlines launches plus the
                  extra cost of eval_psnr_sums(want_images=True) over want_images=False
  --step merge    the parts -> one JSON object (--out)
Usage (GPU box), every GPU step under its own time limit and the chain stopping at the first failure:
  P=/tmp/eval_run_parts; timeout -k 10 300 python tools/eval_run_bench.py --step loop --tree ../parent --parts $P \\
  && timeout -k 10 300 python tools/eval_run_bench.py --step loop --parts $P \\
  && timeout -k 10 300 python tools/eval_run_bench.py --step run --parts $P \\
  && timeout -k 10 400 python tools/eval_run_bench.py --step save --parts $P \\
  && timeout -k 10 300 python tools/eval_run_bench.py --step export --parts $P \\
  && python tools/eval_run_bench.py --step merge --parts $P --out profiles/eval_run_bench.json"""
import argparse
import json
import pathlib
import shutil
import statistics
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
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
        item = dict(self.views[i % len(self.views)])
        item["misc"] = {"scene_id": "synth", "tgt_frame_id": i, "tgt_cam_id": 0}
        return item


def scene(args, dev):
    import numpy as np
    import torch

    from pgdvs_amd import ops, synth
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cfg = load_config(static_renderer="geo")
    rc = cfg.engine.engine_cfg.render_cfg
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(dev).eval()
    H, W, S = args.height, args.width, args.frames
    video = synth.make_video(S, H, W, seed=1234)
    cloud, count, xyz = ops.static_aggregate(T(video["rgbs"]), T(video["depths"]), T(video["dyn_masks"]).view(torch.uint8),
                                             video["K3s"], video["c2ws"], capacity=S * H * W, return_xyz=True)
    g = torch.Generator().manual_seed(7)
    views = []
    for j in range(args.distinct):
        i = int(round(j * (S - 2) / max(args.distinct - 1, 1)))
        d = synth.to_torch(synth.make_view(video, i, frac=0.1 + 0.8 * j / max(args.distinct - 1, 1), seed=5), dev)
        d.pop("static_noise", None)
        item = {k: v[0] for k, v in d.items()}
        item["rgb_tgt"] = item["rgb_src_temporal"][0].clone()
        item["eval_mask"] = (torch.rand((H, W, 1), generator=g) < 0.3).float().repeat(1, 1, 3).to(dev)
        item["seq_ids"] = torch.tensor([i, i, i + 1])
        views.append(item)
    return ResidentCloudRenderer(model, cloud, count, xyz), rc, views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["loop", "run", "save", "export", "merge"])
    ap.add_argument("--parts", required=True, help="directory the steps leave their parts in")
    ap.add_argument("--tree", default=None, help="--step loop: another checkout (built) to measure instead of this one")
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=512)
    ap.add_argument("--save-views", type=int, default=96)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=24)
    args = ap.parse_args()
    parts = pathlib.Path(args.parts)
    parts.mkdir(parents=True, exist_ok=True)
    if args.step == "merge":
        rec = {"hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "H": args.height, "W": args.width, "frames": args.frames}
        for p in sorted(parts.glob("*.json")):
            rec[p.stem] = json.loads(p.read_text())
        js = json.dumps(rec, indent=1)
        if args.out:
            pathlib.Path(args.out).write_text(js + "\n")
        print(js)
        return
    tree = pathlib.Path(args.tree).resolve() if args.tree else ROOT
    for p in (str(tree), str(tree / "ml-pgdvs_amd"), str(ROOT / "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    from pgdvs_amd import _lib, harness, ops, png

    assert torch.cuda.is_available(), "eval_run_bench.py measures on the GPU"
    assert pathlib.Path(_lib.LIB_PATH).resolve().is_relative_to(tree), (_lib.LIB_PATH, tree)
    dev = torch.device("cuda:0")
    model, rc, views = scene(args, dev)
    rec = {"device": torch.cuda.get_device_name(0), "library": str(pathlib.Path(_lib.LIB_PATH).resolve().relative_to(tree)),
           "checkout": "--tree (another checkout, built there)" if args.tree else "this one"}

    def spread(rates):
        return {"rounds": rates, "median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    def plain_loop(n):
        ds = Views(views, n)
        sums = {}
        t0 = time.perf_counter()
        for i in range(n):
            stats = harness.eval_step(model, harness.collate([ds[i]]), rc, device=dev)
            for k, v in stats.items():
                sums[k] = sums[k] + v.cpu() if k in sums else v.cpu()
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    if args.step == "loop":
        plain_loop(32)  # warm-up
        rec.update(views=args.views, views_per_s=spread([plain_loop(args.views) for _ in range(args.rounds)]))
        name = "eval_step_loop_other_tree" if args.tree else "eval_step_loop"
    elif args.step in ("run", "save"):
        save = args.step == "save"
        n = args.save_views if save else args.views
        scratch = pathlib.Path(tempfile.mkdtemp(prefix="eval_run_bench_"))

        def run(k):
            d = scratch / f"k{k}"
            shutil.rmtree(d, ignore_errors=True)
            t0 = time.perf_counter()
            if save:
                with png.PngWriter(n_threads=8) as w:
                    harness.eval_run(model, Views(views, n), rc, device=dev, run_ahead=k, save_individual=True, info_dir=d / "info",
                                     vis_dir=d / "vis", writer=w)
                nbytes = sum(p.stat().st_size for p in d.rglob("*.png"))
            else:
                harness.eval_run(model, Views(views, n), rc, device=dev, run_ahead=k)
                nbytes = 0
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0), nbytes

        try:
            plain_loop(32)  # warm-up
            run(1)
            rates, sizes = {k: [] for k in range(4)}, {}
            loop_rates = []
            for _ in range(args.rounds):  # alternated: every round runs each variant once
                if not save:
                    loop_rates.append(plain_loop(n))
                for k in range(4):
                    r, b = run(k)
                    rates[k].append(r)
                    sizes[k] = b
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        rec.update(views=n, views_per_s={f"run_ahead_{k}": spread(v) for k, v in rates.items()})
        if save:
            rec.update(writer_threads=8, files_per_view=3, png_bytes_per_view=sizes[0] / n)
        else:
            rec["views_per_s"]["eval_step_loop_same_process"] = spread(loop_rates)
        name = "eval_run_save_individual" if save else "eval_run"
    else:
        from eval_lpips_bench import event_median

        H, W = args.height, args.width
        batch = harness.collate([Views(views, 1)[0]])
        with torch.no_grad():
            ret = model.forward(batch, render_cfg=rc, disable_tqdm=True, for_debug=False)
        pred, static, gt, em = ret["combined_rgb"][0].clone(), ret["geo_static_rgb"][0].clone(), batch["rgb_tgt"][0], batch["eval_mask"][0]
        torch.cuda.synchronize()
        out = torch.empty((3, H, 1 + 3 * W), dtype=torch.uint8, device=dev)
        planar = torch.stack([gt.permute(2, 0, 1).contiguous(), pred, static])
        rec.update(bytes_read=3 * 12 * H * W, bytes_written=3 * H * (1 + 3 * W))
        bound_ms = (rec["bytes_read"] + rec["bytes_written"]) / HBM_BYTES_PER_S * 1e3
        rec["streaming_bound_ms"] = bound_ms
        cases = {
            "eval_export_scanlines_adaptive": lambda: ops.eval_export_scanlines(pred, gt, static, adaptive=True, out=out),
            "eval_export_scanlines_plain": lambda: ops.eval_export_scanlines(pred, gt, static, adaptive=False, out=out),
            "three_png_scanlines_adaptive": lambda: [ops.png_scanlines(planar[i], quant="truncate", out=out[i]) for i in range(3)],
            "one_png_scanlines_batch_of_three_adaptive": lambda: ops.png_scanlines(planar, quant="truncate", out=out),
            "eval_psnr_sums": lambda: ops.eval_psnr_sums(pred, gt, em),
            "eval_psnr_sums_want_images": lambda: ops.eval_psnr_sums(pred, gt, em, want_images=True),
        }
        for k, fn in cases.items():
            med, mn = event_median(fn, args.reps, 4)
            rec[f"{k}_ms_median"], rec[f"{k}_ms_min"] = med, mn
        rec["eval_export_scanlines_adaptive_share_of_bound"] = bound_ms / rec["eval_export_scanlines_adaptive_ms_median"]
        rec["eval_export_scanlines_plain_share_of_bound"] = bound_ms / rec["eval_export_scanlines_plain_ms_median"]
        rec["replaced_path_ms_median"] = (rec["three_png_scanlines_adaptive_ms_median"] + rec["eval_psnr_sums_want_images_ms_median"]
                                          - rec["eval_psnr_sums_ms_median"])
        same = torch.equal(ops.eval_export_scanlines(pred, gt, static), ops.png_scanlines(planar, quant="truncate"))
        assert same, "the export pass and png_scanlines(quant='truncate') disagree"
        name = "export_kernel"
    (parts / f"{name}.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
