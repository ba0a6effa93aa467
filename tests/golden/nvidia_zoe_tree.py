"""ZoeDepth files beside the synthetic NVIDIA tree of nvidia_tree.py, in the layout the reference's
NvidiaDynEvaluationDataset reads them (pgdvs/datasets/nvidia_eval.py:869-945), once as a directory and once as a zip:

  zoe_dir/<scene>/dense/zoe_depths_{n,k,nk}/<frame>.npz                 a directory tree
  zoe_zip.zip: zoe_zip/<scene>/dense/zoe_depths_{n,k,nk}/<frame>.npz    the same files as members of a zip

Each .npz holds what the reference's preprocessing stores: ``depth_pred`` [H,W] float32, the disparity-domain
``disp_{share,indiv}_{scale,shift}_{med,trim}`` as 0-d float64 and the fit's errors ``me_*`` / ``mae_*``.  The errors are
laid out so that "moe" (smallest |mean error| of the twelve (type, principle) pairs) picks a different pair from frame to
frame, and on the frames of TIE_FRAMES two pairs tie exactly in magnitude (opposite signs): the earlier one in the
reference's key order wins.  Frame ZERO_PRED_FRAME's predictions hold an exact 0, and frame ZERO_SCALE_FRAME's
``k`` / ``disp_share_scale_med`` is 0.0 (the reference's fit clamps negative scales to 0).  Used by the golden generator
(make_golden_nvidia_zoe.py, which points the REFERENCE loader at it) and by the tests (which point the mirror at a rebuilt
copy): the files are data."""
import pathlib
import zipfile

import numpy as np

import nvidia_tree as NT

ZOE_DIR, ZOE_ZIP = "zoe_dir", "zoe_zip"
TYPES = ("n", "k", "nk")
PRINCIPLES = ("me_med_share", "me_med_indiv", "me_trim_share", "me_trim_indiv")
PAIRS = [(t, k) for t in TYPES for k in PRINCIPLES]  # the reference's zoe_k_dict order
SETTINGS = ("k_me_med_share", "n_me_trim_indiv", "moe")
ZERO_PRED_FRAME, ZERO_PRED_PIXEL = 4, (10, 7)
ZERO_SCALE_FRAME = 3
TIE_FRAMES = (1, 5, 9, 13)
ITEMS = [(5, 5), (0, 0), (13, 1), (6, 2)]  # (frame, camera), as make_golden_nvidia.py's first four
KW = dict(raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1, mode="eval",
          scene_ids=[NT.SCENE], n_src_views_spatial=4, n_src_views_temporal_track_one_side=2, flow_consist_thres=1.0)
# what to pass as zoe_depth_data_path: each name exists only in its other form, so both fallbacks are taken
CONTAINERS = {"dir": f"{ZOE_DIR}.zip", "zip": ZOE_ZIP}


def mean_errors(frame):
    """the twelve pairs' stored mean errors of a frame, in PAIRS order, and the pair "moe" must pick"""
    mag = np.array([0.05 + 0.01 * ((5 * j + 7 * frame) % 12) for j in range(12)])
    sign = np.array([1.0 if (j + frame) % 2 == 0 else -1.0 for j in range(12)])
    me = mag * sign
    best = int(np.argmin(mag))
    if frame in TIE_FRAMES:
        other = (best + 6) % 12
        me[other] = -me[best]  # the same magnitude: a stable sort keeps the dict's order
        best = min(best, other)
    return me, PAIRS[best]


def build_zoe_tree(root, seed=20241017):
    """write both containers under ``root`` (beside raw/, depths/, ...); returns root"""
    root = pathlib.Path(root)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:NT.H, 0:NT.W].astype(np.float32)
    gain = {"n": 0.8, "k": 1.3, "nk": 1.05}  # metric predictions off by a per-model factor, which the scale undoes
    members = []
    for f in range(NT.F):
        me, _ = mean_errors(f)
        for ti, t in enumerate(TYPES):
            pred = (2.0 + 0.4 * np.sin(xx / NT.W * 2 + f) + 0.2 * np.cos(yy / NT.H * 5)) * gain[t]
            pred = (pred + 0.05 * rng.random((NT.H, NT.W))).astype(np.float32)
            if f == ZERO_PRED_FRAME:
                pred[ZERO_PRED_PIXEL] = 0.0
            info = {"depth_pred": pred}
            for scope in ("share", "indiv"):
                for fit in ("med", "trim"):
                    info[f"disp_{scope}_scale_{fit}"] = np.float64(gain[t] * rng.uniform(0.9, 1.1))
                    info[f"disp_{scope}_shift_{fit}"] = np.float64(rng.uniform(-0.03, 0.03))
            if f == ZERO_SCALE_FRAME and t == "k":
                info["disp_share_scale_med"], info["disp_share_shift_med"] = np.float64(0.0), np.float64(0.4)
            for pi, k in enumerate(PRINCIPLES):
                info[k] = np.float64(me[ti * 4 + pi])
                info["mae" + k[2:]] = np.float64(abs(me[ti * 4 + pi]) + 0.02)
            rel = pathlib.Path(NT.SCENE) / "dense" / f"zoe_depths_{t}" / f"{f:05d}.npz"
            (root / ZOE_DIR / rel).parent.mkdir(parents=True, exist_ok=True)
            np.savez(root / ZOE_DIR / rel, **{k: np.asarray(v) for k, v in info.items()})
            members.append(rel)
    with zipfile.ZipFile(root / f"{ZOE_ZIP}.zip", "w") as z:
        for rel in members:
            z.write(root / ZOE_DIR / rel, arcname=f"{ZOE_ZIP}/{rel.as_posix()}")
    return root


def build_tree(root):
    """nvidia_tree's scene with the ZoeDepth containers beside it"""
    return build_zoe_tree(NT.build_tree(root))
