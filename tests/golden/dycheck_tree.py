"""Synthetic DyCheck iPhone tree (the layout ``iPhoneParser`` reads, pgdvs/datasets/dycheck_utils.py:11-360), small
enough to build in a test: one scene, 48 x 64 frames under a ``2x`` factor directory.

  iphone/<scene>/scene.json, dataset.json, metadata.json, extra.json   (no splits/: the parser writes them)
  iphone/<scene>/camera/<name>.json                                    orientation, position, focal, principal point,
                                                                       skew != 0, pixel aspect != 1, distortion (unused)
  iphone/<scene>/rgb/2x/<name>.png, depth/2x/<name>.npy [H,W,1] fp32
  iphone/<scene>/covisible/2x/val/<name>.png                           val frames only
  flow_mask/<scene>/masks/final/<name>_final.png                       dynamic masks (1-bit), train frames
  flow_mask/<scene>/flows/interval_{1,2}/<a>_<b>.npz {flow, coord_diff}

Train: 16 frames on camera 0 at time ids 3..18 (the first is not 0, so the clustered selection's train-list indices differ
from time ids).  Val: cameras 1 and 2 at the first / last train instant, inside the range, and at instants outside it.
Camera 1 at time 10 is a copy of the train camera of that instant, so static points land on the last column and row
exactly; train frames 15..18 are all dynamic and camera 2 at time 21 sits at their end of the path, so with three
spatial sources its static set is empty."""
import json
import pathlib

import numpy as np
import PIL.Image

SCENE = "synth-iphone"
H, W, FACTOR = 48, 64, 2
TRAIN_T = list(range(3, 19))
VAL = [(1, 3), (1, 10), (1, 18), (1, 1), (2, 3), (2, 12), (2, 18), (2, 21)]  # (camera, time id)
ALL_DYNAMIC_T = (15, 16, 17, 18)
CENTER, SCALE, NEAR, FAR = [0.1, -0.2, 0.3], 0.8, 1.3, 2.6


def frame_name(cam, t):
    return f"{cam}_{t:05d}"


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])


def _train_pose(t):
    i = t - TRAIN_T[0]
    return _rot_y(0.03 * i - 0.2), np.array([-0.6 + 0.08 * i, 0.05 * np.sin(i), 0.0]) / SCALE + np.array(CENTER)


def _camera(cam, t):
    if cam == 0 or (cam, t) == (1, 10):
        R, pos = _train_pose(t)
    elif (cam, t) == (2, 21):
        R, pos = _train_pose(18)
        pos = pos + np.array([0.02, 0.01, -0.01])
    else:
        R, pos = _train_pose(min(max(t, 3), 18))
        R = _rot_y(0.1 * cam) @ R
        pos = pos + np.array([0.0, 0.1 * cam, 0.05])
    return {"orientation": R.tolist(), "position": pos.tolist(), "focal_length": 110.0 + 3 * cam,
            "principal_point": [64.3, 47.8], "image_size": [W * FACTOR, H * FACTOR], "skew": 0.8,
            "pixel_aspect_ratio": 1.03, "radial_distortion": [0.01, -0.002, 0.0], "tangential_distortion": [0.0005, -0.0003]}


def build_tree(root):
    root = pathlib.Path(root)
    sd = root / "iphone" / SCENE
    for d in ("camera", f"rgb/{FACTOR}x", f"depth/{FACTOR}x", f"covisible/{FACTOR}x/val"):
        (sd / d).mkdir(parents=True, exist_ok=True)
    md = root / "flow_mask" / SCENE / "masks" / "final"
    md.mkdir(parents=True, exist_ok=True)
    frames = [(0, t) for t in TRAIN_T] + VAL
    names = [frame_name(c, t) for c, t in frames]
    (sd / "scene.json").write_text(json.dumps({"center": CENTER, "scale": SCALE, "near": NEAR, "far": FAR}))
    (sd / "dataset.json").write_text(json.dumps({"count": len(names), "num_exemplars": len(TRAIN_T), "ids": names,
                                                 "train_ids": names[:len(TRAIN_T)], "val_ids": names[len(TRAIN_T):]}))
    (sd / "metadata.json").write_text(json.dumps({frame_name(c, t): {"warp_id": t, "appearance_id": t, "camera_id": c}
                                                  for c, t in frames}))
    (sd / "extra.json").write_text(json.dumps({"factor": FACTOR, "fps": 30.0, "bbox": [[-1, -1, -1], [1, 1, 1]],
                                               "lookat": [0, 0, 1], "up": [0, -1, 0]}))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for c, t in frames:
        n = frame_name(c, t)
        rng = np.random.default_rng(1000 * c + t)
        (sd / "camera" / f"{n}.json").write_text(json.dumps(_camera(c, t)))
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        PIL.Image.fromarray(rgb).save(sd / f"rgb/{FACTOR}x" / f"{n}.png")
        depth = (2.0 + 0.6 * np.sin(xx / 9.0 + t) * np.cos(yy / 7.0) + 0.3 * rng.random((H, W))) / SCALE
        np.save(sd / f"depth/{FACTOR}x" / f"{n}.npy", depth.astype(np.float32)[..., None])
        if c == 0:
            if t in ALL_DYNAMIC_T:
                dyn = np.ones((H, W), bool)
            else:
                dyn = (xx - (10 + 2 * t)) ** 2 + (yy - 20) ** 2 < 64
            PIL.Image.fromarray(dyn).save(md / f"{n}_final.png")
        else:
            cov = ((xx + yy + t) % 7 != 0).astype(np.uint8) * 255
            PIL.Image.fromarray(cov).save(sd / f"covisible/{FACTOR}x/val" / f"{n}.png")
    for k in (1, 2):
        fd = root / "flow_mask" / SCENE / "flows" / f"interval_{k}"
        fd.mkdir(parents=True, exist_ok=True)
        for a in TRAIN_T:
            for b in (a - k, a + k):
                if b in TRAIN_T:
                    rng = np.random.default_rng(7 * a + b)
                    np.savez(fd / f"{frame_name(0, a)}_{frame_name(0, b)}.npz",
                             flow=rng.normal(0, 2, (H, W, 2)).astype(np.float32),
                             coord_diff=rng.normal(0, 0.8, (H, W, 2)).astype(np.float32))
    return root
