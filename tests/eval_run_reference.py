"""Shared by the evaluator-loop tests (test_eval_run_host.py, test_gpu_eval_run.py): the fixture's list dataset and stand-in
model (tests/golden/make_golden_eval_run.py ran the reference's own loop around the same), and the comparison of what
``harness.eval_run`` left on disk and returned with what the reference left and logged."""
import pathlib
import pickle

import numpy as np
import PIL.Image
import torch

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
RUNS = {"plain": (False, -1), "geo": (True, -1), "max3": (False, 3)}  # run -> (the model returns geo_static_rgb, n_max_data)
# The reference's PSNRs are numpy float32 / float64 arithmetic on the quantised images; ours are the same sums in another
# order.  1e-6 relative is the bound of test_host_cpu.py::test_harness_eval_step_vs_reference_eval_step.
RTOL = 1e-6


def load_fixture():
    return dict(np.load(GOLDEN / "eval_run_nvidia.npz"))


class Items:
    """the generator's dataset, rebuilt from the fixture's inputs"""

    def __init__(self, g):
        self.g = g

    def __len__(self):
        return int(self.g["gt"].shape[0])

    def __getitem__(self, i):
        g = self.g
        H, W = g["gt"].shape[1:3]
        misc = {"scene_id": str(g["scene_ids"][i]), "tgt_frame_id": int(g["frame_ids"][i]), "tgt_cam_id": int(g["cam_ids"][i])}
        if g["has_split"][i]:
            misc["split"] = str(g["splits"][i])
        return {"rgb_src_temporal": torch.zeros(2, H, W, 3), "rgb_tgt": torch.from_numpy(g["gt"][i]),
                "eval_mask": torch.from_numpy(g["mask"][i]), "seq_ids": torch.from_numpy(g["seq_ids"][i]),
                "pred": torch.from_numpy(g["pred"][i]), "geo": torch.from_numpy(g["geo"][i]), "misc": misc}


class RecordedModel:
    """the plugin contract's surface that the loop uses; returns each item's recorded images"""
    training = True

    def __init__(self, with_geo=False, gnt=False):
        self.with_geo, self.gnt, self.calls = with_geo, gnt, 0

    def eval(self):
        self.training = False
        return self

    def forward(self, data, render_cfg=None, disable_tqdm=True, for_debug=False):
        assert not self.training and not for_debug and not torch.is_grad_enabled()
        self.calls += 1
        ret = {"combined_rgb": data["pred"]}
        if self.with_geo:
            ret["geo_static_rgb"] = data["geo"]
        if self.gnt:
            ret["static_coarse_rgb"] = data["geo"]
        return ret


def all_files(root):
    root = pathlib.Path(root)
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def decode(path):
    with PIL.Image.open(path) as im:
        im.load()
        return im.mode, im.size, np.asarray(im).copy()


def expected_keys(g, run, i, with_ssim, with_lpips):
    """the reference record's keys in its order, without the metrics eval_run was not asked for (it leaves them out)"""
    drop = ([] if with_ssim else ["ssim_"]) + ([] if with_lpips else ["lpips_"])
    return [k for k in g[f"{run}_pkl_keys"][i].tolist() if not any(k.startswith(d) for d in drop)]


def check_against_fixture(g, run, root, result, *, with_ssim, rtol=RTOL):
    """root/info and root/vis as eval_run wrote them, and its return value, against the reference's run"""
    assert all_files(root) == g[f"{run}_files"].tolist()  # (also: no temporary file is left, no <fname>_rank_<r>.png)
    for name, pix in zip(g[f"{run}_png_names"].tolist(), g[f"{run}_png_pixels"]):
        mode, size, got = decode(pathlib.Path(root) / name)
        assert mode == "RGB" and size == (pix.shape[1], pix.shape[0]), name
        assert np.array_equal(got, pix), name
    by_name = {r["name"]: r["info"] for r in result["records"]}
    for i, name in enumerate(g[f"{run}_pkl_names"].tolist()):
        with open(pathlib.Path(root) / name, "rb") as f:
            info = pickle.load(f)
        keys = g[f"{run}_pkl_keys"][i].tolist()
        assert list(info.keys()) == expected_keys(g, run, i, with_ssim, False), name
        assert isinstance(info["src_frame_ids"], np.ndarray) and np.array_equal(info["src_frame_ids"], g[f"{run}_pkl_src"][i]), name
        for k, v in zip(keys[1:], g[f"{run}_pkl_values"][i]):
            if k.startswith("psnr_"):
                print(f"{run} {name} {k}: got {info[k]!r} reference {float(v)!r}")
                assert type(info[k]) is float and abs(info[k] - float(v)) <= rtol * abs(float(v)), (name, k, info[k], float(v))
        rel = name[len("info/"):-len("_rank_0.pkl")]
        assert list(by_name[rel].keys()) == list(info.keys()) and all(
            np.array_equal(by_name[rel][k], info[k]) for k in info), name  # the returned record is the written one
    assert len(result["records"]) == len(g[f"{run}_pkl_names"])
    avg = dict(zip(g[f"{run}_avg_keys"].tolist(), g[f"{run}_avg_values"].tolist()))
    assert result["eval/count"] == len(g[f"{run}_pkl_names"]) and avg["eval/count"] == 1.0
    for k, v in avg.items():
        if "psnr_" in k:
            print(f"{run} average {k}: got {result[k]!r} reference {v!r}")
            assert abs(result[k] - v) <= rtol * abs(v), (k, result[k], v)
            assert abs(result["sums"][k] / result["eval/count"] - v) <= 2 * rtol * abs(v), k


def check_static_images(g, vis_root, result, expected_truncate):
    """a run over the whole dataset whose model returned both static images (the fixture's ``geo`` under both keys): per view
    _gt, _combined, _gnt and _geo_static, the two static files holding the truncating cast of the clamped image"""
    names = [r["name"] for r in result["records"]]
    assert len(names) == len(g["gt"]) and all_files(vis_root) == sorted(f"{n}_{t}.png" for n in names for t in ("gt", "combined", "gnt", "geo_static"))
    for i, n in enumerate(names):  # (one rank, no limit: record i is item i)
        want = expected_truncate(torch.from_numpy(g["geo"][i])).permute(1, 2, 0).numpy()
        for tag in ("gnt", "geo_static"):
            mode, size, pix = decode(pathlib.Path(vis_root) / f"{n}_{tag}.png")
            assert mode == "RGB" and np.array_equal(pix, want), (n, tag)
        want = expected_truncate(torch.from_numpy(g["pred"][i])).permute(1, 2, 0).numpy()
        assert np.array_equal(decode(pathlib.Path(vis_root) / f"{n}_combined.png")[2], want), n
