#!/usr/bin/env python3
"""Golden vectors for the evaluator's loop (harness.eval_run) by RUNNING THE REFERENCE's own
``PGDVSEvaluator.run_eval_single_ckpt`` (pgdvs/engines/trainer_pgdvs.py:282-360) with ``save_individual=True`` in the build
container: its sampler, loader and ``default_collate_fn``, its ``eval_step`` / ``obtain_quantitative_nvidia`` /
``save_vis_for_eval`` (pgdvs/engines/evaluator_pgdvs.py:27-280, 417-465) and its averaging, around a stand-in model that
returns each item's recorded image.  The engine object is made with ``__new__`` (no Hydra, no checkpoints), the process
group is a single-rank gloo group, the third-party modules that are not installed are stubbed as in make_golden_harness.py;
SSIM and LPIPS (skimage / lpips: not installed) are stubbed to 0, so the fixture pins the PSNR values, the record's keys and
their order, the file names, the decoded pixels of every PNG (read back with PIL) and the logged averages.

Three runs over one list dataset of 5 items (two scene ids, one item with a ``split``, batch size 2 so that the last batch is
short, 24 x 40 images with values above 1 and below 0 and no NaN): "plain", "geo" (the model also returns
``geo_static_rgb``) and "max3" (``n_max_eval_data=3``).  Stores inputs + outputs in eval_run_nvidia.npz (data only).
Usage: python tests/golden/make_golden_eval_run.py"""
import pathlib
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as MG  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
N, H, W = 5, 24, 40
SCENES = ["scene_a", "scene_b", "scene_a", "scene_b", "scene_a"]
SPLIT_ITEM = 3  # the one item whose misc carries a split


def inputs():
    rng = np.random.default_rng(77)
    gt = rng.normal(0.5, 0.3, (N, H, W, 3)).astype(np.float32)
    pred = rng.normal(0.5, 0.35, (N, 3, H, W)).astype(np.float32)
    geo = rng.normal(0.5, 0.4, (N, 3, H, W)).astype(np.float32)
    pred[1, 0, 3, 4], pred[1, 2, 5, 6] = 1.75, -0.5  # (NaN-free values outside [0, 1] in one view, whatever the draw)
    # exact multiples of 1/255 and their float32 neighbours: where a quantiser that rounds differs from one that truncates
    k = np.arange(256, dtype=np.float64)
    levels = (k / 255.0).astype(np.float32)
    pred[2, 0].reshape(-1)[:256] = levels
    pred[2, 1].reshape(-1)[:256] = np.nextafter(levels, np.float32(-np.inf))
    pred[2, 2].reshape(-1)[:256] = np.nextafter(levels, np.float32(np.inf))
    gt[2].reshape(-1)[:256] = levels
    mask = (rng.random((N, H, W, 1)) < 0.3).astype(np.float32).repeat(3, axis=-1)
    seq_ids = (np.arange(N * 3).reshape(N, 3) * 7 % 23).astype(np.int64)
    frame_ids = np.array([3, 11, 4, 250, 17], dtype=np.int64)
    cam_ids = np.array([0, 5, 11, 2, 7], dtype=np.int64)
    return {"gt": gt, "pred": pred, "geo": geo, "mask": mask, "seq_ids": seq_ids, "frame_ids": frame_ids, "cam_ids": cam_ids,
            "scene_ids": np.array(SCENES), "splits": np.array(["val" if i == SPLIT_ITEM else "" for i in range(N)]),
            "has_split": np.array([i == SPLIT_ITEM for i in range(N)])}


class Items(torch.utils.data.Dataset):
    def __init__(self, x):
        self.x = x

    def __len__(self):
        return N

    def __getitem__(self, i):
        x = self.x
        misc = {"scene_id": str(x["scene_ids"][i]), "tgt_frame_id": int(x["frame_ids"][i]), "tgt_cam_id": int(x["cam_ids"][i])}
        if x["has_split"][i]:
            misc["split"] = str(x["splits"][i])
        return {"rgb_src_temporal": torch.zeros(2, H, W, 3), "rgb_tgt": torch.from_numpy(x["gt"][i]),
                "eval_mask": torch.from_numpy(x["mask"][i]), "seq_ids": torch.from_numpy(x["seq_ids"][i]),
                "pred": torch.from_numpy(x["pred"][i]), "geo": torch.from_numpy(x["geo"][i]), "misc": misc}


def main():
    MG._install_stubs()
    from unittest.mock import MagicMock

    import PIL.Image

    for m in ["tensorboard", "torch.utils.tensorboard", "jax", "jax.numpy"]:  # not installed here; unused by the loop
        sys.modules.setdefault(m, MagicMock())
    import pgdvs.engines.evaluator_pgdvs as EV

    EV.calculate_ssim = lambda *a, **k: 0.0
    torch.distributed.init_process_group("gloo", init_method="tcp://127.0.0.1:29673", rank=0, world_size=1)
    x = inputs()
    out = dict(x)
    for run, (with_geo, n_max) in {"plain": (False, -1), "geo": (True, -1), "max3": (False, 3)}.items():
        class Fake(torch.nn.Module):
            def forward(self, data_gpu, render_cfg=None, disable_tqdm=True, for_debug=False):
                ret = {"combined_rgb": data_gpu["pred"]}
                if with_geo:  # noqa: B023
                    ret["geo_static_rgb"] = data_gpu["geo"]
                return ret

        ev = EV.PGDVSEvaluator.__new__(EV.PGDVSEvaluator)
        tmp = pathlib.Path(tempfile.mkdtemp())
        ev.device = torch.device("cpu")
        ev.model = Fake()
        ev.engine_cfg = types.SimpleNamespace(render_cfg=None, quant_type="nvidia")
        ev.cfg = types.SimpleNamespace(rgb_range="0_1", eval_batch_size=2, n_dataloader_workers=0, n_max_eval_data=n_max,
                                       distributed=False)
        ev.verbose = False
        ev.local_rank = ev.global_rank = 0
        ev.world_size = 1
        ev.is_main_proc = True
        ev.datasets = {"eval": Items(x)}
        ev.INFO_DIR, ev.VIS_DIR = str(tmp / "info"), str(tmp / "vis")
        ev.lpips_fn = types.SimpleNamespace(forward=lambda *a, **k: torch.zeros(1))
        logged = []
        ev._write_log = lambda k, v, step: logged.append((k, np.asarray(v, dtype=np.float32).reshape(-1)[0]))  # noqa: B023
        ev.run_eval_single_ckpt(0, 0, save_individual=True)

        files = sorted(str(p.relative_to(tmp)) for p in tmp.rglob("*") if p.is_file())
        out[f"{run}_files"] = np.array(files)
        pngs = [f for f in files if f.endswith(".png")]
        out[f"{run}_png_names"] = np.array(pngs)
        pix = []
        for f in pngs:
            with PIL.Image.open(tmp / f) as im:
                assert im.mode == "RGB" and im.size == (W, H), (f, im.mode, im.size)
                pix.append(np.asarray(im).copy())
        out[f"{run}_png_pixels"] = np.stack(pix)
        pkls = [f for f in files if f.endswith(".pkl")]
        out[f"{run}_pkl_names"] = np.array(pkls)
        keys, vals, src = [], [], []
        for f in pkls:
            with open(tmp / f, "rb") as fh:
                info = pickle.load(fh)
            ks = list(info.keys())
            assert ks[0] == "src_frame_ids", ks
            keys.append(ks)
            src.append(np.asarray(info["src_frame_ids"], dtype=np.int64))
            vals.append([float(info[k]) for k in ks[1:]])
        out[f"{run}_pkl_keys"], out[f"{run}_pkl_values"], out[f"{run}_pkl_src"] = np.array(keys), np.array(vals, np.float64), np.stack(src)
        out[f"{run}_avg_keys"] = np.array([k for k, _ in logged])
        out[f"{run}_avg_values"] = np.array([v for _, v in logged], dtype=np.float32)
        print(run, len(files), "files;", {k: float(v) for k, v in logged})
    np.savez_compressed(OUT / "eval_run_nvidia.npz", **out)
    print((OUT / "eval_run_nvidia.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
