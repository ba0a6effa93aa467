#!/usr/bin/env python3
"""The loaders with and without resident source frames, on a real ``--data_root`` (the NVIDIA tree of
INTEGRATION.md 2b, ``--scene``) or on a synthetic NVIDIA scene this tool writes into a temporary directory: 288 x 550, 48
frames, the monocular video's JPEG sources stored at 1080 x 2062 so that the BOX resize is taken, and the same video in the
monocular layout for ``mono_vis``:
  items    items/s of each loader's ``__getitem__`` with ``resident=False`` (the disk path), and with ``resident=True`` on
           the first pass (frames are decoded on the way) and on the second (nothing is opened), the same indices each
           time, the device drained at the end of each pass; every resident item is compared with the disk item, bit for bit
  vis_run  views/s of ``harness.vis_run`` over nvidia_vis items both ways, through the geometric renderer with the scene's
           static cloud resident (tools/vis_bench.py), PNGs written by an 8-thread writer
  gather   GPU time of the ``ops.item_views`` launch alone (HIP events, median, warmed) for an item of 22 views in four
           groups at 288 x 550, its algorithmic bytes, and its share of the 6.29 TB/s stream rate of MI355X_MICROARCH.md
  dycheck  the DyCheck iPhone loader on a synthetic scene of its own (360 x 480, 48 train frames, two val cameras; 10
           spatial views, tracker windows of 5, device cuda:0): items/s as under ``items``, every resident item compared with
           the disk item (keys in order, bits), the target's upload bytes, and the ``ops.item_target`` launch alone (events,
           bytes, achieved bandwidth, share of the stream rate)
  device_resize  under ``items``: the same indices once more through a loader with ``device_resize=True`` (the
           decoded frames are resized on the device), first and second pass, compared with the disk items bit for bit
  resample the ``ops.resample_u8`` launches alone (HIP events, median, warmed): one 1080 x 2062 x 3 frame to 288 x 550 with
           BOX and with LANCZOS, and the two passes' algorithmic bytes
  zoe      nvidia_eval with ZoeDepth inputs (``--zoe-setting``, default "moe"; on the synthetic tree the files are written as one
           zip in the released layout, on a real tree ``--zoe-path`` names them): items/s of today's device path (disk reads,
           ``device="cuda:0"``) and of ``resident=True`` on the first and second pass, every resident item compared with the
           disk item, the store's stats; and the ``ops.item_zoe_depth`` call alone as under ``gather``, with and without the
           range.  A package whose loader refuses the combination reports the disk figure alone
  decode   ``device_decode=True`` against ``device_resize=True`` alone: the synthetic scene's mv_images rewritten
           as 1080 x 2062 JPEGs (both cameras of a time step; Pillow, quality 90) at 4:2:0 and then at 4:4:4; nvidia_eval and
           nvidia_vis, first and second pass items/s of fresh loaders, the two variants alternating over ``--rounds`` rounds
           (median, min and max are reported: the spread is the yardstick of a difference), the items compared bit for bit.  A
           package without the keyword reports ``device_resize`` alone (the parent commit's figure).  Per frame: Pillow's
           full decode, the host entropy decode (one thread; 16 frames on 16 threads), the reconstruction's two launches by
           device events and each kernel's mean, with the bytes they move against the stream rate.  ``device_entropy=True``
            is a third variant beside the two where the package has the keyword, and per frame the scan on
           the device at the ``--scan-sizes`` subsequence sizes (eight by default): host preparation, bytes uploaded, the scan's launches by device events,
           each kernel's mean, the synchronisation rounds used, and the whole ``ops.jpeg_decode`` call both ways
  depth    ``device_depth=True`` against every other device option alone (``device_resize``, ``device_decode``,
           ``device_entropy``, ``device_png``, ``device_mask``): the five loaders (``--depth-parts``), first and second pass items/s of
           fresh loaders, the two variants alternating over ``--rounds`` rounds in one process (median, min and max: the spread
           between the "off" rounds is the yardstick of a difference), the items compared bit for bit, the construction time of
           each variant (``mono_vis`` takes its near depths there); and ``ops.depth_place`` alone for one 288 x 550 frame and a
           batch of 12: the kernel by the library's event brackets against its streaming bound (4 bytes in, 4 out per pixel at
           6.29 TB/s), and the whole call (staging, upload and launch) by device events and on the host's clock
``--legs nvidia,dycheck,resample,zoe,decode,png,depth`` picks what runs (nvidia: items, vis_run and gather).  Prints one JSON object.
Usage (GPU box): timeout -k 10 900 python tools/loader_bench.py [--data_root DIR --scene Balloon1] [--items 32] [--legs dycheck] [--out FILE]"""
import argparse
import json
import pathlib
import shutil
import sys
import tempfile
import time

import numpy as np
import PIL.Image
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ml-pgdvs_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 6.29e12
H, W, F, N_CAMS = 288, 550, 48, 12
SRC_H, SRC_W = 1080, 2062
SCENE, MONO_SCENE = "Balloon1", "synthetic_video"


def _pose(i):
    y = np.deg2rad(2.5 * (i % N_CAMS) - 12)
    c2w = np.eye(4)
    c2w[:3, :3] = [[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]]
    c2w[:3, 3] = [0.11 * (i % N_CAMS) + 0.003 * i, 0.02 * (i % 3), 0.01 * i]
    return c2w


def write_trees(root, frames=F):
    """the synthetic NVIDIA scene (two cameras per time step: the monocular video's, a JPEG at 1080 x 2062, and its
    neighbour's, a PNG at the target size) and the same video in the monocular layout"""
    root = pathlib.Path(root)
    rng = np.random.default_rng(7)
    dense, mono = root / "nvidia" / "raw" / SCENE / "dense", root / "mono" / MONO_SCENE
    for d in (dense / f"images_{W}x{H}", root / "nvidia" / "masks" / SCENE / "dense" / "masks" / "final",
              root / "nvidia" / "depths" / SCENE / "disp", mono / "rgbs", mono / "poses", mono / "depths", mono / "masks" / "final"):
        d.mkdir(parents=True)
    rows = []
    for i in range(frames):
        c2w = _pose(i)
        m = np.stack([c2w[:3, 1], c2w[:3, 0], -c2w[:3, 2], c2w[:3, 3], np.array([SRC_H, SRC_W, 0.9 * SRC_W])], 1)
        rows.append(np.concatenate([m.reshape(-1), [0.5 + 0.01 * i, 9.0]]))
    np.save(dense / "poses_bounds_cvd.npy", np.stack(rows))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for f in range(frames):
        img = np.stack([127 + 100 * np.sin(xx / 45 + f), 127 + 100 * np.cos(yy / 37 + 0.3 * f), 30.0 * ((xx + yy + f) % 8)], -1)
        img = np.clip(img + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
        big = PIL.Image.fromarray(img).resize((SRC_W, SRC_H), resample=PIL.Image.Resampling.BICUBIC)
        (dense / "mv_images" / f"{f:05d}").mkdir(parents=True)
        (dense / "mv_masks" / f"{f:05d}").mkdir(parents=True)
        c = f % N_CAMS
        big.save(dense / "mv_images" / f"{f:05d}" / f"cam{c + 1:02d}.jpg", quality=92)
        PIL.Image.fromarray(img).save(dense / "mv_images" / f"{f:05d}" / f"cam{(c + 1) % N_CAMS + 1:02d}.png")
        PIL.Image.fromarray(img).save(dense / f"images_{W}x{H}" / f"{f:05d}.png")
        PIL.Image.fromarray(img).save(mono / "rgbs" / f"{f:05d}.png")
        em = np.repeat(((((xx - W * 0.5) ** 2 + (yy - H * 0.4) ** 2) < (0.3 * H) ** 2) * 255).astype(np.uint8)[..., None], 3, -1)
        for cam in (c, (c + 1) % N_CAMS):
            PIL.Image.fromarray(em).save(dense / "mv_masks" / f"{f:05d}" / f"cam{cam + 1:02d}.png")
        dyn = ((xx - W * (0.3 + 0.005 * f)) ** 2 + (yy - H * 0.5) ** 2) < (0.2 * H) ** 2
        disp = (1.0 / (2.0 + 0.4 * np.sin(xx / W * 2 + f) + 0.2 * np.cos(yy / H * 5))).astype(np.float32)
        PIL.Image.fromarray(dyn).save(root / "nvidia" / "masks" / SCENE / "dense" / "masks" / "final" / f"{f:05d}_final.png")
        PIL.Image.fromarray(dyn).save(mono / "masks" / "final" / f"{f:05d}_final.png")
        np.save(root / "nvidia" / "depths" / SCENE / "disp" / f"{f:05d}.npy", disp)
        np.savez(mono / "depths" / f"{f:05d}.npz", depth=(1 / (disp + 1e-8)).astype(np.float32))
        K = np.eye(4)
        K[0, 0] = K[1, 1] = 0.9 * W
        K[0, 2], K[1, 2] = W / 2.0, H / 2.0
        np.savez(mono / "poses" / f"{f:05d}.npz", K=K, c2w=_pose(f))
    for k in (1, 2):
        a_dir, m_dir = root / "nvidia" / "flows" / SCENE / "dense" / "flows" / f"interval_{k}", mono / "flows" / f"interval_{k}"
        a_dir.mkdir(parents=True)
        m_dir.mkdir(parents=True)
        for a in range(frames):
            for b in (a - k, a + k):
                if 0 <= b < frames:
                    pair = dict(flow=rng.normal(0, 1.5, (H, W, 2)).astype(np.float32), coord_diff=rng.normal(0, 0.6, (H, W, 2)).astype(np.float32))
                    np.savez(a_dir / f"{a:05d}_{b:05d}.npz", **pair)
                    if k == 1:
                        np.savez(m_dir / f"{a:05d}_{b:05d}.npz", **pair)
    return root


def loaders(nvidia_root, mono_root, scene, mono_scene, center):
    """name -> factory(resident, device_resize=False, device_decode=False) of the four loaders, on cuda:0"""
    from pgdvs_amd.datasets.mono_vis import MonoVisualizationDataset
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset, NvidiaDynPureGeoEvaluationDataset
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    nv = dict(data_root=nvidia_root, raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows",
              max_hw=-1, scene_ids=[scene], device="cuda:0")
    vis = dict(vis_center_time=center, n_render_frames=200, vis_time_interval=10, vis_bt_max_disp=32)
    # j: False, True (device_decode) or "entropy" (device_entropy too); a package without a keyword still takes the rest
    jk = lambda j: ({"device_decode": True, "device_entropy": True} if j == "entropy" else {"device_decode": True}) if j else {}  # noqa: E731
    pk = lambda p: {"device_png": True} if p else {}  # noqa: E731  (the png leg's keyword)
    out = {"nvidia_eval": lambda r, d=False, j=False, p=False: NvidiaDynEvaluationDataset(mode="eval", resident=r, device_resize=d, **jk(j), **pk(p), **nv),
           "nvidia_pure_geo": lambda r, d=False: NvidiaDynPureGeoEvaluationDataset(mode="eval", resident=r, device_resize=d, **nv),
           "nvidia_vis": lambda r, d=False, j=False: NvidiaDynVisualizationDataset(mode="vis", resident=r, device_resize=d, **jk(j), **vis, **nv)}
    if mono_root is not None:
        out["mono_vis"] = lambda r, d=False, j=False, p=False: MonoVisualizationDataset(data_root=mono_root, max_hw=-1, mode="vis", scene_ids=[mono_scene],
                                                                                        device="cuda:0", resident=r, device_resize=d, **pk(p), **vis)
    return out


def timed_pass(ds, indices):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    items = [ds[i] for i in indices]
    torch.cuda.synchronize()
    return len(indices) / (time.perf_counter() - t0), items


def same_bits(a, b):
    return a.keys() == b.keys() and all(
        (v.dtype == b[k].dtype and v.shape == b[k].shape and torch.equal(v.cpu().contiguous().view(torch.uint8), b[k].cpu().contiguous().view(torch.uint8)))
        if isinstance(v, torch.Tensor) else v == b[k] for k, v in a.items())


def gather_case(reps):
    from eval_lpips_bench import event_median
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.resident import _Scene

    dev = torch.device("cuda:0")
    scene = _Scene(F, H, W, dev)
    scene.rgb.copy_(torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev))
    scene.dyn_mask.copy_(torch.randint(0, 2, (F, H, W), dtype=torch.uint8, device=dev))
    scene.depth.copy_(torch.rand((F, H, W), device=dev) + 0.5)
    groups = [(list(range(14, 24)), True), ([23, 24], True), (list(range(18, 23)), True), (list(range(25, 30)), True)]
    out = ops.item_views(scene.rgb, scene.dyn_mask, scene.depth, groups)
    med, mn = event_median(lambda: ops.item_views(scene.rgb, scene.dyn_mask, scene.depth, groups, out=out), reps, 4)
    views = sum(len(g) for g, _ in groups)
    read, written = views * H * W * 8, views * H * W * 44
    bound_ms = (read + written) / HBM_BYTES_PER_S * 1e3
    return {"views": views, "H": H, "W": W, "bytes_read": read, "bytes_written": written, "ms_median": med, "ms_min": mn,
            "streaming_bound_ms": bound_ms, "share_of_stream_rate": bound_ms / med,
            "distinct_frames_read": len({f for g, _ in groups for f in g})}


ZOE_ZIP = "nvidia_zoedepth"


def write_zoe_files(nvidia_root, frames=F):
    """ZoeDepth files for the synthetic NVIDIA scene in the released layout: one zip, ``<stem>/<scene>/dense/zoe_depths_{n,k,nk}/
    <frame>.npz`` with ``depth_pred`` float32 at the target size and the fits' 0-d float64 entries; the stored mean errors make
    "moe" move between the twelve pairs from frame to frame"""
    import io
    import zipfile

    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gain = {"n": 0.8, "k": 1.3, "nk": 1.05}
    with zipfile.ZipFile(pathlib.Path(nvidia_root) / f"{ZOE_ZIP}.zip", "w") as z:
        for f in range(frames):
            for ti, t in enumerate(gain):
                pred = (2.0 + 0.4 * np.sin(xx / W * 2 + f) + 0.2 * np.cos(yy / H * 5)) * gain[t]
                info = {"depth_pred": (pred + 0.05 * rng.random((H, W))).astype(np.float32)}
                for scope in ("share", "indiv"):
                    for fit in ("med", "trim"):
                        info[f"disp_{scope}_scale_{fit}"] = np.asarray(np.float64(gain[t] * rng.uniform(0.9, 1.1)))
                        info[f"disp_{scope}_shift_{fit}"] = np.asarray(np.float64(rng.uniform(-0.03, 0.03)))
                        j = ti * 4 + 2 * (fit == "trim") + (scope == "indiv")
                        me = (0.05 + 0.01 * ((5 * j + 7 * f) % 12)) * (1.0 if (j + f) % 2 == 0 else -1.0)
                        info[f"me_{fit}_{scope}"], info[f"mae_{fit}_{scope}"] = np.asarray(np.float64(me)), np.asarray(np.float64(abs(me) + 0.02))
                blob = io.BytesIO()
                np.savez(blob, **info)
                z.writestr(f"{ZOE_ZIP}/{SCENE}/dense/zoe_depths_{t}/{f:05d}.npz", blob.getvalue())


def zoe_case(nvidia_root, scene, zoe_path, setting, n_items):
    """nvidia_eval with ZoeDepth inputs: today's device path (disk reads, ``device="cuda:0"``) against ``resident=True`` on
    the device, first and second pass, every resident item compared with the disk item.  A package whose loader refuses the
    combination gives the disk figure alone (the baseline of the commit before this row existed)."""
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset

    kw = dict(data_root=nvidia_root, raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1,
              scene_ids=[scene], mode="eval", device="cuda:0", use_zoe_depth=setting, zoe_depth_data_path=zoe_path)
    disk = NvidiaDynEvaluationDataset(**kw)
    idx = [int(round(j * (len(disk) - 1) / max(n_items - 1, 1))) for j in range(n_items)]
    disk[idx[0]]  # (warm-up: the fused op's first call)
    r_disk, want = timed_pass(disk, idx)
    rec = {"use_zoe_depth": setting, "container": "zip" if disk.zoe_depth_data_path.is_file() else "dir", "len": len(disk),
           "disk_device_items_per_s": r_disk,
           "views_per_item": int(sum(v.shape[0] for k, v in want[0].items() if k.startswith("rgb_src_")))}
    try:
        res = NvidiaDynEvaluationDataset(resident=True, **kw)
    except ValueError as e:
        rec["resident"] = f"refused: {e}"
        return rec
    r_first, got1 = timed_pass(res, idx)
    r_second, got2 = timed_pass(res, idx)
    rec.update({"resident_first_pass_items_per_s": r_first, "resident_second_pass_items_per_s": r_second,
                "second_pass_over_disk": r_second / r_disk,
                "bit_identical": all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2)),
                "on_device": all(v.is_cuda for it in got2 for v in it.values() if isinstance(v, torch.Tensor)),
                "store_bytes": res.store.nbytes, "stats": dict(res.store.stats)})
    return rec


def zoe_gather_case(reps):
    """the ``ops.item_zoe_depth`` call alone (HIP events, median, warmed) for an item of 22 views in four groups at 288 x 550,
    the range over the 10 spatial views: the gather launch's algorithmic bytes and streaming bound, with and without the
    range (whose select passes read the 8-byte keys once per radix pass on top)"""
    from eval_lpips_bench import event_median
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.resident import _Scene

    dev = torch.device("cuda:0")
    scene = _Scene(F, H, W, dev, prediction=True)
    scene.depth.copy_(torch.rand((F, H, W), device=dev) * 4 + 0.5)
    groups = [list(range(14, 24)), [23, 24], list(range(18, 23)), list(range(25, 30))]
    views, n_range = sum(len(g) for g in groups), len(groups[0])
    rng = np.random.default_rng(5)
    ss = np.stack([rng.uniform(0.8, 1.2, views), rng.uniform(-0.02, 0.02, views)], 1)
    rays = torch.zeros((n_range, 12), device=dev)
    rays[:, 0], rays[:, 4], rays[:, 8] = 1.0 / (0.9 * W), 1.0 / (0.9 * W), 1.0  # (M = inv(K) without the principal point)
    out, _ = ops.item_zoe_depth(scene.depth, groups, ss, rays, np.eye(4))
    med, mn = event_median(lambda: ops.item_zoe_depth(scene.depth, groups, ss, rays, np.eye(4), out=out), reps, 4)
    med0, mn0 = event_median(lambda: ops.item_zoe_depth(scene.depth, groups, ss, out=out), reps, 4)
    n = H * W
    read, written, keys = views * n * 4, views * n * 4, n_range * n * 8
    bound0, bound = (read + written) / HBM_BYTES_PER_S * 1e3, (read + written + keys) / HBM_BYTES_PER_S * 1e3
    return {"views": views, "range_views": n_range, "H": H, "W": W, "bytes_read": read, "bytes_written": written, "key_bytes_written": keys,
            "select_passes": 6, "select_bytes_read": 6 * keys,
            "depths_only": {"ms_median": med0, "ms_min": mn0, "streaming_bound_ms": bound0, "share_of_stream_rate": bound0 / med0},
            "with_range": {"ms_median": med, "ms_min": mn, "gather_streaming_bound_ms": bound,
                           "streaming_bound_ms_with_select_reads": (read + written + 7 * keys) / HBM_BYTES_PER_S * 1e3},
            "distinct_frames_read": len({f for g in groups for f in g})}


def resample_case(reps):
    """the two launches of ``ops.resample_u8`` alone, one source frame of the synthetic scene's size to the target's"""
    from eval_lpips_bench import event_median
    from pgdvs_amd import _lib, ops

    dev = torch.device("cuda:0")
    src = torch.randint(0, 256, (SRC_H, SRC_W, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    rec = {"in": [SRC_H, SRC_W, 3], "out": [H, W, 3]}
    for filter in ("box", "lanczos"):
        plan = ops.resample_plan((SRC_H, SRC_W), (H, W), filter, dev)
        ops.resample_u8(src, (H, W), filter, out=out)
        med, mn = event_median(lambda: ops.resample_u8(src, (H, W), filter, out=out), reps, 4)
        tmp = _lib.load().pgdvs_resample_u8_workspace_bytes(1, SRC_H, SRC_W, 3, H, W, ops.RESAMPLE_FILTERS[filter])
        taps_v = int(plan.tables[3].shape[1])
        # the horizontal pass reads the frame and writes the intermediate image; the vertical pass reads it once per tap row
        # of every output row (from the L2) and writes the result
        rec[filter] = {"ms_median": med, "ms_min": mn, "taps": [int(plan.tables[1].shape[1]), taps_v], "frame_bytes": src.numel(),
                       "intermediate_bytes": int(tmp), "out_bytes": out.numel(),
                       "streaming_bound_ms": (src.numel() + 2 * int(tmp) + out.numel()) / HBM_BYTES_PER_S * 1e3}
    return rec


def rewrite_jpegs(nvidia_root, subsampling, frames=F):
    """every mv_images file of the synthetic scene -- both cameras of a time step, so that every evaluation target is one too --
    as a 1080 x 2062 JPEG written by Pillow at quality 90 with ``subsampling``, from the monocular video's frames"""
    dense = pathlib.Path(nvidia_root) / "raw" / SCENE / "dense"
    for f in range(frames):
        big = PIL.Image.open(dense / f"images_{W}x{H}" / f"{f:05d}.png").resize((SRC_W, SRC_H), resample=PIL.Image.Resampling.BICUBIC)
        d = dense / "mv_images" / f"{f:05d}"
        for old in d.iterdir():
            old.unlink()
        for cam in (f % N_CAMS, (f + 1) % N_CAMS):
            big.save(d / f"cam{cam + 1:02d}.jpg", quality=90, subsampling=subsampling)


def _spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), "min": xs[0], "max": xs[-1]}


def decode_loaders_case(make, n_items, rounds):
    """fresh loaders each round, ``device_resize`` alone, with ``device_decode`` and with ``device_entropy`` on top, alternating;
    items/s of both passes"""
    rec = {}
    for name in ("nvidia_eval", "nvidia_vis"):
        fn = make[name]
        try:
            fn(True, True, True)
            variants = (("device_resize", False), ("device_decode", True))
        except TypeError:
            variants = (("device_resize", False),)
        try:
            fn(True, True, "entropy")
            variants += (("device_entropy", "entropy"),)
        except TypeError:  # (a package without the keyword: the parent commit's columns alone)
            pass
        probe = fn(True, True)
        idx = [int(round(j * (len(probe) - 1) / max(n_items - 1, 1))) for j in range(n_items)]
        probe[idx[0]]  # (warm-up: code objects, the resize plans)
        del probe
        rates = {v: {"first": [], "second": []} for v, _ in variants}
        want, same, stats = None, True, {}
        for _ in range(rounds):
            for v, j in variants:
                ds = fn(True, True, j)
                r1, got1 = timed_pass(ds, idx)
                r2, got2 = timed_pass(ds, idx)
                rates[v]["first"].append(r1)
                rates[v]["second"].append(r2)
                if want is None:
                    want = got1
                same = same and all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2))
                stats[v] = dict(ds.store.stats)
                del ds, got1, got2
                torch.cuda.empty_cache()
        r = rec[name] = {"items": len(idx), "rounds": rounds, "bit_identical": same, "stats": stats}
        for v, _ in variants:
            r[f"{v}_first_pass_items_per_s"], r[f"{v}_second_pass_items_per_s"] = _spread(rates[v]["first"]), _spread(rates[v]["second"])
        print(f"decode {name}: {r}", file=sys.stderr, flush=True)
    return rec


def decode_frame_case(path, reps, scan_sizes=(64,)):
    """one file: Pillow's decode, the host entropy decode and the reconstruction on the device"""
    import ctypes as C
    import io
    from concurrent.futures import ThreadPoolExecutor

    from eval_lpips_bench import event_median
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    data = pathlib.Path(path).read_bytes()
    arr = np.frombuffer(data, np.uint8)
    ptr = C.c_void_p(arr.ctypes.data)

    def clock(fn, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _spread(ts)

    info = _lib.JpegInfo()
    assert lib.pgdvs_jpeg_parse(ptr, arr.size, C.byref(info)) == 0, lib.pgdvs_last_error()
    nq = C.sizeof(info.quant)
    bufs = [torch.empty((info.coef_bytes + nq) // 2, dtype=torch.int16, pin_memory=True) for _ in range(16)]
    entropy = lambda b: lib.pgdvs_jpeg_entropy_decode(ptr, arr.size, C.c_void_p(b.data_ptr()), info.coef_bytes)  # noqa: E731
    assert entropy(bufs[0]) == 0
    rec = {"file_bytes": arr.size, "sampling": ops.JPEG_SAMPLINGS[info.sampling], "coef_bytes": info.coef_bytes,
           "pillow_decode_ms": clock(lambda: np.array(PIL.Image.open(io.BytesIO(data))), 10),
           "parse_ms": clock(lambda: lib.pgdvs_jpeg_parse(ptr, arr.size, C.byref(info)), 10),
           "entropy_decode_ms_one_thread": clock(lambda: entropy(bufs[0]), 10)}
    with ThreadPoolExecutor(16) as pool:  # one frame per thread, 16 at once (ctypes drops the GIL for the call)
        list(pool.map(entropy, bufs))
        rec["entropy_decode_ms_16_frames_on_16_threads"] = clock(lambda: list(pool.map(entropy, bufs)), 5)
    C.memmove(bufs[0].data_ptr() + info.coef_bytes, info.quant, nq)
    dev = bufs[0].to("cuda:0")
    ws = torch.empty(lib.pgdvs_jpeg_reconstruct_workspace_bytes(C.byref(info)), dtype=torch.uint8, device="cuda:0")
    out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device="cuda:0")
    run = lambda: _lib.check(lib.pgdvs_jpeg_reconstruct(dev.data_ptr(), dev.data_ptr() + info.coef_bytes, C.byref(info), out.data_ptr(),  # noqa: E731
                                                        info.width * 3, ws.data_ptr(), ws.numel(), ops._stream()), "pgdvs_jpeg_reconstruct")
    med, mn = event_median(run, reps, 4)
    lib.pgdvs_prof_enable(1)
    for _ in range(reps):
        run()
    text = C.create_string_buffer(4096)
    lib.pgdvs_prof_report(text, 4096)
    lib.pgdvs_prof_enable(0)
    kernels = {ln.split()[0]: float(ln.split()[2]) / int(ln.split()[1]) for ln in text.value.decode().splitlines() if ln.startswith("jpeg_")}
    planes = sum(64 * info.blocks_w[c] * info.blocks_h[c] for c in range(3))
    moved = {"jpeg_idct": info.coef_bytes + planes, "jpeg_colour": planes + out.numel()}
    rec.update({"equals_pillow": bool(np.array_equal(out.cpu().numpy(), np.array(PIL.Image.open(io.BytesIO(data))))),
                "reconstruct_ms_median": med, "reconstruct_ms_min": mn, "plane_bytes": planes, "rgb_bytes": out.numel(),
                "kernels": {k: {"ms_mean": v, "bytes_moved": moved[k], "streaming_bound_ms": moved[k] / HBM_BYTES_PER_S * 1e3,
                                "share_of_stream_rate": moved[k] / HBM_BYTES_PER_S * 1e3 / v} for k, v in kernels.items()},
                "streaming_bound_ms": sum(moved.values()) / HBM_BYTES_PER_S * 1e3})
    if hasattr(ops, "jpeg_scan_decode"):
        rec["scan_on_device"] = scan_frame_case(data, info, reps, clock, event_median, scan_sizes)
    return rec


def scan_frame_case(data, info, reps, clock, event_median, sizes):
    """the scan of one file decoded on the device, per subsequence size: the host preparation, the bytes
    uploaded, the launches of ``pgdvs_jpeg_scan_decode`` together (device events, median) and each kernel's mean, the rounds
    the synchronisation used; and the whole ``ops.jpeg_decode`` call both ways, to its last byte (a host clock round a
    synchronise)"""
    import ctypes as C

    from pgdvs_amd import _lib, ops

    lib, dev = _lib.load(), torch.device("cuda:0")
    rec = {"default_sub_bytes": ops.JPEG_SCAN_SUB_BYTES, "sizes": {}}
    rc, want, _ = _host_coef(lib, data, info)
    for sub in sizes:
        prepared, _ = ops.jpeg_scan_prepare(data, sub)
        coef, status, (rounds, fixups) = ops.jpeg_scan_decode(data, dev, sub, return_rounds=True)
        hd = _lib.JpegScanHeader.from_address(prepared.data_ptr())
        r = rec["sizes"][sub] = {"status": status, "equals_host_decoder": bool(rc == 0 and np.array_equal(coef.cpu().numpy(), want)),
                                 "subsequences": hd.nsub, "workgroups": -(-hd.nsub // 256), "rounds_first_launch": rounds,
                                 "fixup_launches_that_ran": fixups, "bytes_uploaded": prepared.numel(), "coef_bytes": info.coef_bytes,
                                 "prepare_ms": clock(lambda: ops.jpeg_scan_prepare(data, sub), 10)}
        d = prepared.to(dev)
        out, st = torch.empty(info.coef_bytes // 2, dtype=torch.int16, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.pgdvs_jpeg_scan_decode_workspace_bytes(C.c_void_p(prepared.data_ptr()), prepared.numel()), dtype=torch.uint8, device=dev)
        run = lambda: _lib.check(lib.pgdvs_jpeg_scan_decode(C.c_void_p(prepared.data_ptr()), d.data_ptr(), prepared.numel(), out.data_ptr(),  # noqa: E731
                                                            info.coef_bytes, st.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "scan")
        r["scan_decode_ms_median"], r["scan_decode_ms_min"] = event_median(run, reps, 4)
        r["upload_ms_median"], _ = event_median(lambda: d.copy_(prepared, non_blocking=True), reps, 4)
        lib.pgdvs_prof_enable(1)
        for _ in range(reps):
            run()
        text = C.create_string_buffer(4096)
        lib.pgdvs_prof_report(text, 4096)
        lib.pgdvs_prof_enable(0)
        r["kernels_ms_per_call"] = {ln.split()[0]: float(ln.split()[2]) / reps for ln in text.value.decode().splitlines()
                                    if ln.startswith(("jpeg_scan", "jpeg_dc", "fill_bytes"))}

    def whole(mode):
        def fn():
            ops.jpeg_decode(data, device=dev, entropy=mode)
            torch.cuda.synchronize()
        fn()
        return clock(fn, 20)
    rec["jpeg_decode_call_ms"] = {"host": whole("host"), "device": whole("device")}
    return rec


def _host_coef(lib, data, info):
    import ctypes as C

    arr = np.frombuffer(data, np.uint8)
    coef = np.zeros(info.coef_bytes // 2, np.int16)
    rc = lib.pgdvs_jpeg_entropy_decode(C.c_void_p(arr.ctypes.data), arr.size, C.c_void_p(coef.ctypes.data), info.coef_bytes)
    return rc, coef, None


def decode_case(nvidia_root, scene, center, n_items, reps, rounds, synthetic, scan_sizes):
    rec = {}
    for sub in (("4:2:0", "4:4:4") if synthetic else (None,)):
        if sub is not None:
            rewrite_jpegs(nvidia_root, sub)
        r = rec[sub or "tree"] = {"loaders": decode_loaders_case(loaders(nvidia_root, None, scene, None, center), n_items, rounds)}
        first = sorted((pathlib.Path(nvidia_root) / "raw" / scene / "dense" / "mv_images").glob("*/*.jpg"))[0]
        try:
            r["frame"] = decode_frame_case(first, reps, scan_sizes)
        except AttributeError as e:  # (a package without the reader)
            r["frame"] = f"not in this package: {e}"
        print(f"decode frame {sub}: {r['frame']}", file=sys.stderr, flush=True)
    return rec


DY_H, DY_W, DY_F, DY_FACTOR, DY_SCENE = 360, 480, 48, 2, "synthetic-iphone"


def rewrite_pngs(nvidia_root, mono_root, frames=F):
    """every mv_images file of the synthetic scene (both cameras of a time step: every evaluation target too) and every
    frame of the monocular tree behind frame 0 as a 1080 x 2062 PNG written by Pillow at its default level"""
    dense = pathlib.Path(nvidia_root) / "raw" / SCENE / "dense"
    for f in range(frames):
        big = PIL.Image.open(dense / f"images_{W}x{H}" / f"{f:05d}.png").resize((SRC_W, SRC_H), resample=PIL.Image.Resampling.BICUBIC)
        d = dense / "mv_images" / f"{f:05d}"
        for old in d.iterdir():
            old.unlink()
        for cam in (f % N_CAMS, (f + 1) % N_CAMS):
            big.save(d / f"cam{cam + 1:02d}.png")
        if mono_root is not None and f:
            big.save(pathlib.Path(mono_root) / MONO_SCENE / "rgbs" / f"{f:05d}.png")


def png_loaders_case(factories, n_items, rounds):
    """fresh loaders each round, ``device_resize=True`` alone and with ``device_png=True``, alternating; items/s of both passes.
    ``factories``: name -> fn(device_png) -> loader (a package without the keyword: the first column alone)"""
    rec = {}
    for name, fn in factories.items():
        variants = ("device_resize",)
        try:
            fn(True)
            variants += ("device_png",)
        except TypeError:  # (the parent commit's checkout)
            pass
        probe = fn(False)
        idx = [int(round(j * (len(probe) - 1) / max(n_items - 1, 1))) for j in range(n_items)]
        probe[idx[0]]  # (warm-up: code objects, the resize plans)
        del probe
        rates = {v: {"first": [], "second": []} for v in variants}
        want, same, stats = None, True, {}
        for _ in range(rounds):
            for v in variants:
                ds = fn(v == "device_png")
                r1, got1 = timed_pass(ds, idx)
                r2, got2 = timed_pass(ds, idx)
                rates[v]["first"].append(r1)
                rates[v]["second"].append(r2)
                if want is None:
                    want = got1
                same = same and all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2))
                stats[v] = dict(ds.store.stats)
                del ds, got1, got2
                torch.cuda.empty_cache()
        r = rec[name] = {"items": len(idx), "rounds": rounds, "bit_identical": same, "stats": stats}
        for v in variants:
            r[f"{v}_first_pass_items_per_s"], r[f"{v}_second_pass_items_per_s"] = _spread(rates[v]["first"]), _spread(rates[v]["second"])
        print(f"png {name}: {r}", file=sys.stderr, flush=True)
    return rec


def png_frame_case(path, reps, sub_sizes):
    """one 1080 x 2062 file: Pillow's decode, ``zlib.decompress`` of its stream alone, and per subsequence size the call of
    ``ops.png_decode_batch`` by device events for one file and for a batch of 12, the two launches of ``pgdvs_png_decode``
    apart (the library's event brackets), and the windows, blocks and rounds the stream took"""
    import ctypes as C
    import io
    import zlib

    from eval_lpips_bench import event_median
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    data = pathlib.Path(path).read_bytes()
    info = ops.png_parse(data)[0]
    stream = b"".join(data[o:o + n] for o, n in info["idat"])

    def clock(fn, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[n // 2]

    rec = {"file_bytes": len(data), "stream_bytes": len(stream), "size": [info["height"], info["width"], info["channels"]],
           "pillow_decode_ms": clock(lambda: np.array(PIL.Image.open(io.BytesIO(data))), 10), "zlib_decompress_ms": clock(lambda: zlib.decompress(stream), 10),
           "host_chunk_walk_ms": clock(lambda: ops.png_info(data), 10)}
    want = np.array(PIL.Image.open(io.BytesIO(data)))
    for sub in sub_sizes:
        stats = []
        got = ops.png_decode_batch([data], device="cuda:0", sub_bytes=sub, stats=stats)[0]
        r = rec[f"sub_bytes_{sub}"] = {"equal_pillow": bool(np.array_equal(got.cpu().numpy(), want)), "windows": stats[0][0], "sync_rounds_max": stats[0][1],
                                       "resolve_rounds_max": stats[0][2], "blocks": stats[0][3]}
        lib.pgdvs_prof_enable(1)
        for _ in range(reps):
            ops.png_decode_batch([data], device="cuda:0", sub_bytes=sub)
        text = C.create_string_buffer(4096)
        lib.pgdvs_prof_report(text, 4096)
        lib.pgdvs_prof_enable(0)
        r["kernels_ms_per_call"] = {ln.split()[0]: float(ln.split()[2]) / reps for ln in text.value.decode().splitlines() if ln.startswith("png_")}
        for batch in (1, 12):
            med, mn = event_median(lambda: ops.png_decode_batch([data] * batch, device="cuda:0", sub_bytes=sub), reps, 1)
            r[f"batch_{batch}_call_ms"] = {"median": med, "min": mn, "per_file": med / batch}
        print(f"png frame sub {sub}: {r}", file=sys.stderr, flush=True)
    return rec


PNG_PARTS = ("nvidia_eval", "mono_vis", "dycheck", "frame")


def png_case(scratch, nvidia_root, mono_root, scene, center, n_items, reps, rounds, sub_sizes, parts):
    """the png leg: the synthetic scenes with frames and targets rewritten as PNG; ``parts`` of nvidia_eval, mono_vis, dycheck
    (the loaders, each on its own so that a run can be cut into calls) and frame (one file through the op)"""
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    factories = {}
    if set(parts) & {"nvidia_eval", "mono_vis", "frame"}:
        rewrite_pngs(nvidia_root, mono_root if "mono_vis" in parts else None)
        make = loaders(nvidia_root, mono_root, scene, MONO_SCENE, center)
        for name in ("nvidia_eval", "mono_vis"):
            if name in parts:
                factories[name] = lambda p, fn=make[name]: fn(True, True, False, **({"p": True} if p else {}))
    if "dycheck" in parts:
        root = write_dycheck_tree(scratch / "dycheck_png")
        kw = dict(data_root=root, raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DY_SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=10, n_src_views_temporal_track_one_side=5, device="cuda:0", resident=True,
                  device_resize=True)
        factories["dycheck"] = lambda p: DyCheckiPhoneEvaluationDataset(**kw, **({"device_png": True} if p else {}))
    rec = {"loaders": png_loaders_case(factories, n_items, rounds)}
    if "frame" in parts and hasattr(ops, "png_decode_batch"):
        dense = pathlib.Path(nvidia_root) / "raw" / scene / "dense" / "mv_images" / f"{center:05d}"
        rec["frame"] = png_frame_case(sorted(dense.iterdir())[0], reps, sub_sizes)
    return rec


DEPTH_PARTS = ("nvidia_eval", "nvidia_pure_geo", "nvidia_vis", "mono_vis", "dycheck", "op")
OTHER_DEVICE_OPTIONS = dict(device_resize=True, device_decode=True, device_entropy=True, device_png=True, device_mask=True)


def depth_loaders_case(factories, n_items, rounds):
    """fresh loaders each round, every other device option on, without and with ``device_depth=True``, alternating; items/s of both
    passes and the seconds each construction took.  ``factories``: name -> fn(device_depth) -> loader"""
    rec = {}
    for name, fn in factories.items():
        variants = ("off", "device_depth")
        probe = fn(True)
        idx = [int(round(j * (len(probe) - 1) / max(n_items - 1, 1))) for j in range(n_items)]
        probe[idx[0]]  # (warm-up: code objects, the resize plans, the side streams)
        del probe
        rates = {v: {"first": [], "second": [], "construct_s": []} for v in variants}
        want, same, stats = None, True, {}
        for _ in range(rounds):
            for v in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ds = fn(v == "device_depth")
                torch.cuda.synchronize()
                rates[v]["construct_s"].append(time.perf_counter() - t0)
                r1, got1 = timed_pass(ds, idx)
                r2, got2 = timed_pass(ds, idx)
                rates[v]["first"].append(r1)
                rates[v]["second"].append(r2)
                if want is None:
                    want = got1
                same = same and all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2))
                stats[v] = dict(ds.store.stats)
                del ds, got1, got2
                torch.cuda.empty_cache()
        r = rec[name] = {"items": len(idx), "rounds": rounds, "bit_identical": same, "stats": stats}
        for v in variants:
            r[f"{v}_first_pass_items_per_s"], r[f"{v}_second_pass_items_per_s"] = _spread(rates[v]["first"]), _spread(rates[v]["second"])
            r[f"{v}_construct_s"] = _spread(rates[v]["construct_s"])
        off, on = r["off_first_pass_items_per_s"], r["device_depth_first_pass_items_per_s"]
        r["first_pass_on_over_off"] = on["median"] / off["median"]
        r["faster_than_the_off_spread"] = bool(on["median"] > off["max"])
        print(f"depth {name}: {r}", file=sys.stderr, flush=True)
    return rec


def depth_op_case(reps):
    """``ops.depth_place`` of 288 x 550 frames ("reciprocal", straight into padded slots): the kernel alone and the whole call"""
    import ctypes as C

    from eval_lpips_bench import event_median
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    rng = np.random.default_rng(5)
    rec = {"size": [H, W]}
    for batch in (1, 12):
        datas = [rng.uniform(0.2, 0.6, (H, W)).astype(np.float32) for _ in range(batch)]
        slots = torch.empty((batch, -(-H * W // 4) * 4), dtype=torch.float32, device="cuda:0")
        outs = [slots[k, :H * W].view(H, W) for k in range(batch)]
        requests = [ops.DepthRequest(d.tobytes(), 0, d.shape, "reciprocal", 1.0, o) for d, o in zip(datas, outs)]
        call = lambda: ops.depth_place(requests, device="cuda:0")  # noqa: E731
        call()
        equal = all(np.array_equal(o.cpu().numpy(), 1 / (d + 1e-8)) for d, o in zip(datas, outs))
        lib.pgdvs_prof_enable(1)
        for _ in range(reps):
            call()
        text = C.create_string_buffer(4096)
        lib.pgdvs_prof_report(text, 4096)
        lib.pgdvs_prof_enable(0)
        kernel_ms = [float(ln.split()[2]) / reps for ln in text.value.decode().splitlines() if ln.startswith("depth_place")][0]
        med, mn = event_median(call, reps, 1)
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        host_ms = (time.perf_counter() - t0) * 1e3 / reps
        torch.cuda.synchronize()
        nbytes = batch * H * W * 8
        rec[f"batch_{batch}"] = {"equal_numpy": bool(equal), "bytes_in_and_out": nbytes, "streaming_bound_us": nbytes / HBM_BYTES_PER_S * 1e6,
                                 "kernel_us": kernel_ms * 1e3, "kernel_share_of_stream_rate": nbytes / HBM_BYTES_PER_S / (kernel_ms * 1e-3),
                                 "call_events_ms": {"median": med, "min": mn}, "call_host_ms": host_ms}
        print(f"depth op batch {batch}: {rec[f'batch_{batch}']}", file=sys.stderr, flush=True)
    return rec


def depth_case(scratch, nvidia_root, mono_root, scene, center, n_items, reps, rounds, parts):
    """the depth leg: the synthetic scenes as written; ``parts`` of the five loaders (each on its own, so that a run can be cut into
    calls) and op (``ops.depth_place`` alone)"""
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset
    from pgdvs_amd.datasets.mono_vis import MonoVisualizationDataset
    from pgdvs_amd.datasets.nvidia_eval import NvidiaDynEvaluationDataset, NvidiaDynPureGeoEvaluationDataset
    from pgdvs_amd.datasets.nvidia_vis import NvidiaDynVisualizationDataset

    on = dict(device="cuda:0", resident=True, **OTHER_DEVICE_OPTIONS)
    nv = dict(data_root=nvidia_root, raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1, scene_ids=[scene], **on)
    vis = dict(vis_center_time=center, n_render_frames=200, vis_time_interval=10, vis_bt_max_disp=32)
    factories = {"nvidia_eval": lambda d: NvidiaDynEvaluationDataset(mode="eval", device_depth=d, **nv),
                 "nvidia_pure_geo": lambda d: NvidiaDynPureGeoEvaluationDataset(mode="eval", device_depth=d, **nv),
                 "nvidia_vis": lambda d: NvidiaDynVisualizationDataset(mode="vis", device_depth=d, **vis, **nv),
                 "mono_vis": lambda d: MonoVisualizationDataset(data_root=mono_root, max_hw=-1, mode="vis", scene_ids=[MONO_SCENE], device_depth=d, **vis, **on)}
    if "dycheck" in parts:
        root = write_dycheck_tree(scratch / "dycheck_depth")
        kw = dict(data_root=root, raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval", scene_ids=[DY_SCENE],
                  spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=10, n_src_views_temporal_track_one_side=5, **on)
        factories["dycheck"] = lambda d: DyCheckiPhoneEvaluationDataset(device_depth=d, **kw)
    rec = {"loaders": depth_loaders_case({k: v for k, v in factories.items() if k in parts}, n_items, rounds)}
    if "op" in parts:
        rec["op"] = depth_op_case(reps)
    return rec


def write_dycheck_tree(root, frames=DY_F):
    """a synthetic DyCheck iPhone scene in the layout iPhoneParser reads: 360 x 480 (the 2x frames), ``frames`` train frames on
    camera 0 at time ids 0.., two val cameras at every second instant (val frames sit on train instants, as the dataset's do,
    so every item's temporal pair is the placeholder one and no flow file is read)"""
    root = pathlib.Path(root)
    rng = np.random.default_rng(11)
    sd, md = root / "iphone" / DY_SCENE, root / "flow_mask" / DY_SCENE / "masks" / "final"
    for d in (sd / "camera", sd / f"rgb/{DY_FACTOR}x", sd / f"depth/{DY_FACTOR}x", sd / f"covisible/{DY_FACTOR}x/val", md,
              root / "flow_mask" / DY_SCENE / "flows"):
        d.mkdir(parents=True)
    shots = [(0, t) for t in range(frames)] + [(c, t) for c in (1, 2) for t in range(0, frames, 2)]
    names = [f"{c}_{t:05d}" for c, t in shots]
    (sd / "scene.json").write_text(json.dumps({"center": [0.0, 0.0, 0.0], "scale": 0.5, "near": 0.2, "far": 6.0}))
    (sd / "dataset.json").write_text(json.dumps({"count": len(names), "num_exemplars": frames, "ids": names}))
    (sd / "metadata.json").write_text(json.dumps({n: {"warp_id": t, "appearance_id": t, "camera_id": c} for n, (c, t) in zip(names, shots)}))
    (sd / "extra.json").write_text(json.dumps({"factor": DY_FACTOR, "fps": 30.0, "bbox": [[-1, -1, -1], [1, 1, 1]], "lookat": [0, 0, 1],
                                               "up": [0, -1, 0]}))
    yy, xx = np.mgrid[0:DY_H, 0:DY_W].astype(np.float32)
    for n, (c, t) in zip(names, shots):
        a = 0.01 * t - 0.2 + 0.05 * c
        R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
        (sd / "camera" / f"{n}.json").write_text(json.dumps({
            "orientation": R.tolist(), "position": [-0.6 + 0.025 * t, 0.1 * c, 0.02 * c], "focal_length": 1.7 * DY_W,
            "principal_point": [DY_W * 1.0, DY_H * 1.0], "image_size": [DY_W * DY_FACTOR, DY_H * DY_FACTOR], "skew": 0.0,
            "pixel_aspect_ratio": 1.0, "radial_distortion": [0.0, 0.0, 0.0], "tangential_distortion": [0.0, 0.0]}))
        img = np.stack([127 + 100 * np.sin(xx / 45 + t), 127 + 100 * np.cos(yy / 37 + 0.3 * t + c), 30.0 * ((xx + yy + t) % 8)], -1)
        img = np.clip(img + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
        PIL.Image.fromarray(img).save(sd / f"rgb/{DY_FACTOR}x" / f"{n}.png")
        if c == 0:
            depth = (4.0 + 0.8 * np.sin(xx / DY_W * 3 + 0.1 * t) + 0.4 * np.cos(yy / DY_H * 5)).astype(np.float32)
            np.save(sd / f"depth/{DY_FACTOR}x" / f"{n}.npy", depth[..., None])
            dyn = ((xx - DY_W * (0.3 + 0.005 * t)) ** 2 + (yy - DY_H * 0.5) ** 2) < (0.2 * DY_H) ** 2
            PIL.Image.fromarray(dyn).save(md / f"{n}_final.png")
        else:
            PIL.Image.fromarray((((xx + yy + t) % 7 != 0) * 255).astype(np.uint8)).save(sd / f"covisible/{DY_FACTOR}x/val" / f"{n}.png")
    return root


def dycheck_case(scratch, n_items, reps):
    """the DyCheck loader, ``resident=False`` against ``resident=True`` on cuda:0 (10 spatial views by the closest_wo_temporal
    rule, tracker windows of 5), and the ``ops.item_target`` launch alone"""
    from eval_lpips_bench import event_median
    from pgdvs_amd import ops
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    t0 = time.perf_counter()
    root = write_dycheck_tree(scratch / "dycheck")
    rec = {"tree": {"synthetic": True, "H": DY_H, "W": DY_W, "train_frames": DY_F, "val_cameras": 2, "written_s": time.perf_counter() - t0}}
    kw = dict(data_root=root, raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
              scene_ids=[DY_SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=10,
              n_src_views_temporal_track_one_side=5, device="cuda:0")
    disk, res = DyCheckiPhoneEvaluationDataset(**kw), DyCheckiPhoneEvaluationDataset(resident=True, **kw)
    idx = [int(round(j * (len(disk) - 1) / max(n_items - 1, 1))) for j in range(n_items)]
    disk[idx[0]]  # (warm-up: the depth-range op's first call)
    r_disk, want = timed_pass(disk, idx)
    r_first, got1 = timed_pass(res, idx)
    r_second, got2 = timed_pass(res, idx)
    n = DY_H * DY_W
    rec["loader"] = {
        "len": len(disk), "items": n_items, "disk_items_per_s": r_disk, "resident_first_pass_items_per_s": r_first,
        "resident_second_pass_items_per_s": r_second, "second_pass_over_disk": r_second / r_disk,
        "bit_identical": all(list(a) == list(b) == list(c) and same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2)),
        "on_device": all(v.is_cuda for it in got2 for v in it.values() if isinstance(v, torch.Tensor)),
        "views_per_item": int(sum(v.shape[0] for k, v in want[0].items() if k.startswith("rgb_src_"))),
        "store_bytes": res.store.nbytes, "stats": dict(res.store.stats),
        "target_upload_bytes_per_item": {"as_bytes": n * 4, "as_float32": n * 16}}
    del want, got1, got2, disk, res
    torch.cuda.empty_cache()
    dev = torch.device("cuda:0")
    rgb = torch.randint(0, 256, (DY_H, DY_W, 3), dtype=torch.uint8, device=dev)
    cov = torch.randint(0, 2, (DY_H, DY_W), dtype=torch.uint8, device=dev) * 255
    out = ops.item_target(rgb, cov)
    med, mn = event_median(lambda: ops.item_target(rgb, cov, out=out), reps, 4)
    read, written = n * 4, n * 16
    bound_ms = (read + written) / HBM_BYTES_PER_S * 1e3
    rec["item_target"] = {"H": DY_H, "W": DY_W, "bytes_read": read, "bytes_written": written, "ms_median": med, "ms_min": mn,
                          "achieved_bytes_per_s": (read + written) / (med * 1e-3), "streaming_bound_ms": bound_ms,
                          "share_of_stream_rate": bound_ms / med}
    return rec


def vis_run_case(make, n_views, scratch):
    """views/s of harness.vis_run over nvidia_vis items, disk and resident (second pass), geometric renderer, resident cloud"""
    from pgdvs_amd import harness, ops, png
    from pgdvs_amd.datasets.static_aggregation import hwf_to_K
    from pgdvs_amd.instantiate import load_config
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer
    from vis_bench import ResidentCloudRenderer

    dev = torch.device("cuda:0")
    cfg = load_config(static_renderer="geo")
    rc = cfg.engine.engine_cfg.render_cfg
    model = PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(dev).eval()
    res = make(True)
    scene_id = res.valid_fs[0][0]
    n = res.c2w_dict[scene_id].shape[0]
    first = res[0]  # (gives the store its scene)
    scene = res.store.scenes[scene_id]
    shape = (scene.h, scene.w)
    for f in range(n):  # the whole video into the store: the static cloud is aggregated from it
        if not scene.filled[f]:
            res.store.put(scene, f, *res._decode_frame(scene_id, f, shape))
    del first
    K3s = np.stack([hwf_to_K(*res.hwf_dict[scene_id][f], tgt_shape=shape) for f in range(n)])
    cloud, count, xyz = ops.static_aggregate(scene.rgb.float() / 255.0, scene.depth.contiguous(), scene.dyn_mask.contiguous(), K3s,
                                             res.c2w_dict[scene_id], capacity=n * shape[0] * shape[1], return_xyz=True)
    renderer = ResidentCloudRenderer(model, cloud, count, xyz)
    indices = [int(round(j * (len(res) - 1) / max(n_views - 1, 1))) for j in range(n_views)]

    class Sub:
        def __init__(self, ds):
            self.ds = ds

        def __len__(self):
            return len(indices)

        def __getitem__(self, i):
            return self.ds[indices[i]]

    def run(ds, tag):
        d = scratch / f"vis_{tag}"
        shutil.rmtree(d, ignore_errors=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with png.PngWriter(n_threads=8) as w:
            harness.vis_run(renderer, Sub(ds), rc, d, device=dev, writer=w)
        torch.cuda.synchronize()
        return len(indices) / (time.perf_counter() - t0)

    run(res, "warm")
    return {"views": n_views, "disk_views_per_s": run(make(False), "disk"), "resident_views_per_s": run(res, "resident"),
            "static_points": int(count.reshape(-1)[0].item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_root", default=None, help="a real NVIDIA tree (raw/, depths/, masks/, flows/); default: a synthetic one")
    ap.add_argument("--scene", default=SCENE)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--vis-views", type=int, default=48)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--legs", default="nvidia,dycheck", help="comma-separated: nvidia (the four loaders, vis_run, gather), dycheck, resample, zoe, decode, png, depth")
    ap.add_argument("--rounds", type=int, default=3, help="decode leg: rounds of fresh loaders per variant")
    ap.add_argument("--scan-sizes", default="16,32,48,64,96,128,256,512", help="decode leg: subsequence sizes (bytes) of the per-frame scan figures")
    ap.add_argument("--png-sizes", default="16,32,64,128,256", help="png leg: subsequence sizes (bytes) of the per-frame figures")
    ap.add_argument("--png-parts", default=",".join(PNG_PARTS), help="png leg: which of its parts run (a long leg is cut into calls)")
    ap.add_argument("--depth-parts", default=",".join(DEPTH_PARTS), help="depth leg: which of its parts run (a long leg is cut into calls)")
    ap.add_argument("--zoe-setting", default="moe", help="use_zoe_depth of the zoe leg")
    ap.add_argument("--zoe-path", default=None, help="zoe_depth_data_path under a real --data_root (the synthetic tree brings its own)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loader_bench.py measures on the GPU"
    from pgdvs_amd import _lib

    _lib.load()
    scratch = pathlib.Path(tempfile.mkdtemp(prefix="loader_bench_"))
    rec = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "items": args.items, "loaders": {}}
    legs = set(args.legs.split(","))
    assert legs and legs <= {"nvidia", "dycheck", "resample", "zoe", "decode", "png", "depth"}, args.legs
    try:
        if "resample" in legs:
            rec["resample"] = resample_case(args.reps)
            print(f"resample: {rec['resample']}", file=sys.stderr, flush=True)
        if "dycheck" in legs:
            rec["dycheck"] = dycheck_case(scratch, args.items, args.reps)
            print(f"dycheck: {rec['dycheck']}", file=sys.stderr, flush=True)
        png_tree = "png" in legs and set(args.png_parts.split(",")) != {"dycheck"}  # (the DyCheck part writes a tree of its own)
        depth_parts = tuple(args.depth_parts.split(",")) if "depth" in legs else ()
        assert set(depth_parts) <= set(DEPTH_PARTS), args.depth_parts
        depth_tree = bool(set(depth_parts) - {"dycheck", "op"})  # (the DyCheck part writes a tree of its own, the op needs none)
        if not legs & {"nvidia", "zoe", "decode"} and not png_tree and not depth_tree:
            nvidia_root = mono_root = center = None
        elif args.data_root is None:
            t0 = time.perf_counter()
            write_trees(scratch / "tree")
            rec["tree"] = {"synthetic": True, "H": H, "W": W, "frames": F, "source_jpeg": [SRC_H, SRC_W], "written_s": time.perf_counter() - t0}
            nvidia_root, mono_root, center = scratch / "tree" / "nvidia", scratch / "tree" / "mono", F // 2
        else:
            nvidia_root, mono_root, center = pathlib.Path(args.data_root), None, 50
            rec["tree"] = {"synthetic": False, "scene": args.scene}
        make = loaders(nvidia_root, mono_root, args.scene, MONO_SCENE, center) if "nvidia" in legs else {}
        for name, fn in make.items():
            disk, res = fn(False), fn(True)
            idx = [int(round(j * (len(disk) - 1) / max(args.items - 1, 1))) for j in range(args.items)]
            disk[idx[0]]  # (warm-up: the depth-range op's first call)
            r_disk, want = timed_pass(disk, idx)
            r_first, got1 = timed_pass(res, idx)
            r_second, got2 = timed_pass(res, idx)
            dr = fn(True, True)  # device_resize: the same indices, both passes
            r_dr_first, got3 = timed_pass(dr, idx)
            r_dr_second, got4 = timed_pass(dr, idx)
            rec["loaders"][name] = {
                "len": len(disk), "disk_items_per_s": r_disk, "resident_first_pass_items_per_s": r_first,
                "resident_second_pass_items_per_s": r_second, "second_pass_over_disk": r_second / r_disk,
                "bit_identical": all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got1, want, got2)),
                "views_per_item": int(sum(v.shape[0] for k, v in want[0].items() if k.startswith("rgb_src_"))),
                "store_bytes": res.store.nbytes, "stats": dict(res.store.stats),
                "device_resize_first_pass_items_per_s": r_dr_first, "device_resize_second_pass_items_per_s": r_dr_second,
                "device_resize_first_pass_over_resident": r_dr_first / r_first,
                "device_resize_bit_identical": all(same_bits(a, b) and same_bits(c, b) for a, b, c in zip(got3, want, got4)),
                "device_resize_stats": dict(dr.store.stats)}
            print(f"{name}: {rec['loaders'][name]}", file=sys.stderr, flush=True)
            del want, got1, got2, got3, got4, disk, res, dr
            torch.cuda.empty_cache()
        if "zoe" in legs:
            zoe_path = args.zoe_path
            if args.data_root is None:
                write_zoe_files(nvidia_root)
                zoe_path = f"{ZOE_ZIP}.zip"
            assert zoe_path is not None, "--zoe-path: where the ZoeDepth files of --data_root are"
            rec["nvidia_eval_zoe"] = zoe_case(nvidia_root, args.scene, zoe_path, args.zoe_setting, args.items)
            print(f"nvidia_eval_zoe: {rec['nvidia_eval_zoe']}", file=sys.stderr, flush=True)
            if "resident" not in rec["nvidia_eval_zoe"]:
                rec["zoe_gather"] = zoe_gather_case(args.reps)
        if "nvidia" in legs:
            rec["vis_run"] = vis_run_case(make["nvidia_vis"], args.vis_views, scratch)
            rec["gather"] = gather_case(args.reps)
        if "depth" in legs:  # (in front of the legs that rewrite the synthetic tree's image files)
            assert args.data_root is None or not {"mono_vis"} & set(depth_parts), "mono_vis runs on the synthetic tree"
            rec["depth"] = depth_case(scratch, nvidia_root, mono_root, args.scene, center, args.items, args.reps, args.rounds, depth_parts)
        if "png" in legs:  # (it rewrites the synthetic tree's image files too)
            assert args.data_root is None and "decode" not in legs, "the png leg rewrites the synthetic tree: a run of its own"
            parts = tuple(args.png_parts.split(","))
            assert parts and set(parts) <= set(PNG_PARTS), args.png_parts
            rec["png"] = png_case(scratch, nvidia_root, mono_root, args.scene, center, args.items, args.reps, args.rounds,
                                  tuple(int(x) for x in args.png_sizes.split(",")), parts)
        if "decode" in legs:  # last: it rewrites the synthetic tree's image files
            rec["decode"] = decode_case(nvidia_root, args.scene, center, args.items, args.reps, args.rounds, args.data_root is None,
                                        tuple(int(x) for x in args.scan_sizes.split(",")))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    js = json.dumps(rec, indent=1)
    if args.out:
        pathlib.Path(args.out).write_text(js + "\n")
    print(js)


if __name__ == "__main__":
    main()
