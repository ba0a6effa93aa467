#!/usr/bin/env python3
"""Golden vectors of the ZoeDepth stage: the reference's own pgdvs/preprocess/compute_zoedepth.py, run end to end through
runpy with --save_space on seeded synthetic scenes; zoe_align.npz holds the inputs and what the script wrote, together.

What stands in for modules that are not installed here: trimesh, skimage.transform, cv2 and third_parties.ZoeDepth.* are
MagicMock stand-ins (nothing the script calls with --save_space touches them, bar the two below); ``build_model`` returns a
stub whose ``infer`` gives the scene's seeded depth of the frame, in call order; ``get_config`` returns None; tqdm, when
missing, is the identity.  The reference's pgdvs/preprocess directory is on sys.path for its bare ``import colmap_reader``.
The scene's files are written here: PNG images and masks, ``poses_bounds_cvd.npy``, a hand-packed ``sparse/points3D.bin``.

Per scene and frame the fixture holds the script's .npz entries and two things it keeps in its globals but does not save:
``flag_trim`` (its ``all_flag_trim``) and the kept points' indices, found by matching the columns of its ``proj_pcl``, bit
for bit and in order, in the projection of all points computed with its own expressions.

Scenes: the smallest at which each part of the device path can go wrong.
  A  23 x 37, 5 frames, 400 points, a mask rectangle that moves.
  B  70 x 130 (rows longer than a wavefront), 3 frames, about 3000 points; frame 0's camera is the identity with a
     power-of-two focal length, so points can be put exactly on integer pixels, in the last fractional row and column
     (scipy samples 0 there: static, predicted depth 0), behind the camera, under the mask and nearer than 1e-3.
  C  5 x 7, 2 frames: frame 0 keeps exactly one point (scale 0, quantile of one element), frame 1 two (even medians).
  D  3 x 300, one frame: a row longer than a workgroup, three window chunks of the row pass.

Guard bands, asserted here so that the consumers may demand bits (a point that lands in one is nudged by 1/64, an integer-pixel
point by one pixel, and the scene run again):
  * no projected coordinate within 1e-9 of 0, W-1, W, H-1, H, bar the deliberate integer-pixel points, strictly inside;
  * no mask sample within 1e-6 of 0.1, no depth within 1e-9 of 1e-3;
  * no float64 spline value (scipy, output=float64) of a kept point within 1e-9 relative of a float32 rounding midpoint;
  * no kept spline sample negative;
  * the projection of a kept point is well conditioned: sum |terms| / |result| < 100 for x, y and the depth, so that two
    float64 evaluations in different orders agree to 1e-12 relative;
  * the two order statistics around the 0.8 quantile differ by more than 1e-4 relative; adjacent sorted keys at every
    median differ; |nn_disp / nn_disp_shifted| < 1e3 at the elements that give each ratio median;
  * the med and trim fits differ by more than 1e-3 relative (scenes A, B);
  * every frame keeps between 20 % and 95 % of its points;
  * mean |diff| / |mean diff| < 1e3 for every error pair, so that summation order stays below 1e-12 of the mean error.
Scene C is exempt from the frame-level asserts: with n = 1 the shifted disparities are 0 and both fits have scale 0; with
n = 2 the two normalised differences are rounding residue of +-1 - +-1, and the 0.8 quantile lies between them whenever
they differ.  Nothing there depends on a summation order (a sum of two float32 values is the same in any width), so the
device path can still be asked for the same bits."""
import pathlib
import runpy
import struct
import sys
import tempfile
from types import ModuleType
from unittest.mock import MagicMock

import numpy as np
import PIL.Image
import torch
from scipy.ndimage import map_coordinates

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as MG  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
TINY = 1.0e-16
NUDGE = 1.0 / 64
SAVED = ("disp_indiv_scale_med", "disp_indiv_shift_med", "disp_share_scale_med", "disp_share_shift_med", "disp_indiv_scale_trim",
         "disp_indiv_shift_trim", "disp_share_scale_trim", "disp_share_shift_trim", "sparse_pcl", "proj_pcl", "pcl_depth_mvs",
         "pcl_depth_pred", "depth_pred", "depth_is_disp", "mae_med_share", "mae_med_indiv", "mae_trim_share", "mae_trim_indiv",
         "me_med_share", "me_med_indiv", "me_trim_share", "me_trim_indiv")
BULKY_SAME_AS_INPUT = ("sparse_pcl", "depth_pred")


class _StubModel:
    """stands in for ZoeDepth: ``infer`` returns the running scene's depth of the next frame"""
    depths = None

    def __init__(self):
        self.calls = 0

    def to(self, device):
        return self

    def eval(self):
        return self

    def infer(self, X):
        d = torch.from_numpy(_StubModel.depths[self.calls])[None, None]
        assert tuple(X.shape[2:]) == tuple(d.shape[2:])
        self.calls += 1
        return d


def _install_stubs():
    MG._install_stubs()
    for m in ["trimesh", "cv2", "skimage", "skimage.transform", "third_parties", "third_parties.ZoeDepth",
              "third_parties.ZoeDepth.zoedepth", "third_parties.ZoeDepth.zoedepth.models", "third_parties.ZoeDepth.zoedepth.utils"]:
        sys.modules[m] = MagicMock()
    builder = ModuleType("third_parties.ZoeDepth.zoedepth.models.builder")
    builder.build_model = lambda conf: _StubModel()
    config = ModuleType("third_parties.ZoeDepth.zoedepth.utils.config")
    config.get_config = lambda *a, **k: None
    sys.modules[builder.__name__], sys.modules[config.__name__] = builder, config
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = ModuleType("tqdm")
        t.tqdm = lambda it, **k: it
        sys.modules["tqdm"] = t
    sys.path.insert(0, str(MG.REF / "pgdvs" / "preprocess"))


# ---------------------------------------------------------------------------- scenes
def true_depth(xs, ys):
    return 3.0 + np.sin(xs / 9.0) + 0.5 * np.cos(ys / 5.0)


def predictions(F, H, W):
    """smooth and positive: the scene's disparity through an affine map, plus a small term of the frame's own"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    out = []
    for i in range(F):
        disp = (1.0 / true_depth(xs, ys) - 0.05) / 0.7 + 0.02 * np.sin(xs / 7.0 + i) * np.cos(ys / 6.0)
        out.append((1.0 / disp).astype(np.float32))
    return out


def cameras(F, H, W, focal, step):
    """poses_bounds rows of cameras that slide along x by ``step`` per frame (frame 0: the identity) -> [F,17]"""
    rows = []
    for i in range(F):
        right, down, fwd = np.eye(3)
        t = np.array([step * i, 0.015625 * (i % 2), 0.0])
        m = np.stack([down, right, -fwd, t, np.array([H, W, focal], np.float64)], axis=1)  # [3,5]: down, right, back | t | hwf
        rows.append(np.concatenate([m.reshape(-1), [0.1, 10.0]]))
    return np.array(rows)


def unproject(x, y, d, H, W, focal):
    """world points (frame 0 is the identity) of the pixels (x, y) at depth d, float32"""
    return np.stack([(x - W / 2.0) * d / focal, (y - H / 2.0) * d / focal, d], -1).astype(np.float32)


def cloud(rng, n, H, W, focal, outliers=0.25):
    x, y = rng.uniform(-3, W + 3, n), rng.uniform(-2, H + 2, n)
    d = true_depth(x, y) * (1.0 + 0.02 * rng.normal(size=n))
    bad = rng.random(n) < outliers
    d[bad] *= rng.uniform(0.5, 2.0, bad.sum())
    return unproject(x, y, d, H, W, focal)


def moving_mask(F, H, W, h, w, x0, dx, y0):
    masks = np.zeros((F, H, W), np.uint8)
    for i in range(F):
        masks[i, y0:y0 + h, x0 + dx * i:x0 + dx * i + w] = 255
    return masks


def scene_a():
    rng = np.random.default_rng(23037)
    F, H, W, focal = 5, 23, 37, 32.0
    return dict(H=H, W=W, focal=focal, poses=cameras(F, H, W, focal, 0.0625), pred=predictions(F, H, W),
                masks=moving_mask(F, H, W, 8, 9, 4, 5, 6), pts=cloud(rng, 400, H, W, focal), integer=np.zeros(400, bool))


def scene_b():
    rng = np.random.default_rng(70130)
    F, H, W, focal = 3, 70, 130, 64.0
    pts = [cloud(rng, 2900, H, W, focal)]
    special = []
    ix, iy = rng.integers(1, W - 1, 30).astype(np.float64), rng.integers(1, H - 1, 30).astype(np.float64)
    special.append(unproject(ix, iy, np.where(np.arange(30) % 2, 2.0, 4.0), H, W, focal))  # exactly on integer pixels
    n_int = 30
    lx, ly = rng.uniform(5, W - 5, 20), rng.uniform(5, H - 5, 20)
    special.append(unproject(np.full(20, W - 0.5), ly, true_depth(lx, ly), H, W, focal))  # the last fractional column
    special.append(unproject(lx, np.full(20, H - 0.25), true_depth(lx, ly), H, W, focal))  # the last fractional row
    special.append(unproject(lx, ly, -true_depth(lx, ly), H, W, focal))  # behind the camera, projecting into the image
    special.append(unproject(lx, ly, np.full(20, 0.0005), H, W, focal))  # nearer than 1e-3
    mx, my = rng.uniform(42, 58, 20), rng.uniform(22, 38, 20)
    special.append(unproject(mx, my, true_depth(mx, my), H, W, focal))  # under frame 0's mask
    pts = np.concatenate(pts + special)
    integer = np.zeros(len(pts), bool)
    integer[2900:2900 + n_int] = True
    perm = rng.permutation(len(pts))
    return dict(H=H, W=W, focal=focal, poses=cameras(F, H, W, focal, 0.03125), pred=predictions(F, H, W),
                masks=moving_mask(F, H, W, 20, 20, 40, 25, 20), pts=pts[perm], integer=integer[perm])


def scene_c():
    F, H, W, focal = 2, 5, 7, 8.0
    # frame 1's camera sits 1 to the right: a point at depth 2 moves 4 pixels to the left, one at 2.5 moves 3.2
    x = np.array([2.0, 8.4, 5.6, 3.3, -4.0, 2.2])
    y = np.array([-3.0, 1.7, 3.1, 2.2, 1.0, 9.0])
    d = np.array([2.0, 2.5, 2.0, -2.0, 2.0, 3.0])  # kept in frame 0: point 2 alone; in frame 1: points 1 and 2
    return dict(H=H, W=W, focal=focal, poses=cameras(F, H, W, focal, 1.0), pred=predictions(F, H, W),
                masks=np.zeros((F, H, W), np.uint8), pts=unproject(x, y, d, H, W, focal), integer=np.zeros(6, bool))


def scene_d():
    rng = np.random.default_rng(3300)
    F, H, W, focal = 1, 3, 300, 128.0
    n = 300
    x, y = rng.uniform(-20, W + 20, n), rng.uniform(-0.3, H - 0.85, n)
    d = true_depth(x, y) * (1.0 + 0.02 * rng.normal(size=n))
    bad = rng.random(n) < 0.25
    d[bad] *= rng.uniform(0.5, 2.0, bad.sum())
    masks = np.zeros((F, H, W), np.uint8)
    masks[0, :, 100:140] = 255
    return dict(H=H, W=W, focal=focal, poses=cameras(F, H, W, focal, 0.0), pred=predictions(F, H, W), masks=masks,
                pts=unproject(x, y, d, H, W, focal), integer=np.zeros(n, bool))


# ---------------------------------------------------------------------------- files and the run
def pack_points3d(path, pts):
    """COLMAP's points3D.bin: count, then per point id, xyz (double), rgb, error, track length and the track"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for i, p in enumerate(pts):
            track = i % 3
            f.write(struct.pack("<QdddBBBd", i + 1, float(p[0]), float(p[1]), float(p[2]), 10, 20, 30, 0.5))
            f.write(struct.pack("<Q", track))
            f.write(struct.pack("<" + "ii" * track, *range(2 * track)))


def write_tree(root, sc):
    """the scene's files under ``root`` (the layout tests/test_zoe_align_host.py writes again from the fixture)"""
    root = pathlib.Path(root)
    (root / "rgbs").mkdir(parents=True)
    (root / "masks" / "final").mkdir(parents=True)
    (root / "sparse").mkdir()
    for i, m in enumerate(sc["masks"]):
        rgb = np.full((sc["H"], sc["W"], 3), 16 * i, np.uint8)
        PIL.Image.fromarray(rgb).save(root / "rgbs" / f"{i:05d}.png")
        PIL.Image.fromarray(m).save(root / "masks" / "final" / f"{i:05d}_final.png")
    np.save(root / "poses_bounds_cvd.npy", sc["poses"])
    pack_points3d(root / "sparse" / "points3D.bin", sc["pts"])


def run_reference(sc):
    """-> (the script's globals, {frame: its .npz as a dict})"""
    with tempfile.TemporaryDirectory() as td:
        td = pathlib.Path(td)
        write_tree(td / "scene", sc)
        _StubModel.depths = sc["pred"]
        argv = sys.argv
        sys.argv = ["compute_zoedepth.py", "--root_dir", str(td / "scene"), "--save_dir", str(td / "out"), "--mask_dir",
                    str(td / "scene"), "--zoedepth_type", "NK", "--zoedepth_ckpt_dir", str(td), "--save_space"]
        try:
            g = runpy.run_path(str(MG.REF / "pgdvs" / "preprocess" / "compute_zoedepth.py"), run_name="__main__")
        finally:
            sys.argv = argv
        files = sorted((td / "out" / "zoe_depths_nk").glob("*.npz"))
        assert len(files) == len(sc["pred"]) and not list((td / "out").rglob("*.ply"))
        return g, {i: dict(np.load(f)) for i, f in enumerate(files)}


# ---------------------------------------------------------------------------- guards
def near_any(v, targets, tol):
    return np.any([np.abs(v - t) < tol for t in targets], axis=0)


def f32_midpoint_close(v64, rel):
    v32 = v64.astype(np.float32)
    close = np.zeros(v64.shape, bool)
    for side in (-np.inf, np.inf):
        mid = (v32.astype(np.float64) + np.nextafter(v32, np.float32(side)).astype(np.float64)) / 2.0
        close |= np.abs(v64 - mid) <= rel * np.abs(v64)
    return close & (v64 != 0.0)


def median_neighbours_differ(keys):
    s = np.sort(keys)
    n = len(s)
    lo, hi = (n - 1) // 2, n // 2
    idx = [i for i in (lo - 1, lo, hi, hi + 1) if 0 <= i < n]
    return all(s[a] != s[b] for a, b in zip(idx[:-1], idx[1:]) if a != b)


def point_guards(sc, g, frame):
    """indices of the points of ``frame`` inside a point-level guard band, and the kept points' indices"""
    H, W = sc["H"], sc["W"]
    w2c, K = g["all_w2c"][frame], g["all_K"][frame]
    h_pt = np.ones([len(sc["pts"]), 4])
    h_pt[:, :3] = sc["pts"]
    h_pt = h_pt.T
    out = w2c @ h_pt
    im = K @ out[:3, :]
    depth = im[2, :].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        im = im / im[2:, :]
    x, y = im[0], im[1]
    edge = near_any(x, (0, W - 1, W), 1e-9) | near_any(y, (0, H - 1, H), 1e-9)
    on_int = sc["integer"] & (frame == 0)
    assert np.all((x[on_int] == np.round(x[on_int])) & (y[on_int] == np.round(y[on_int])))
    assert np.all((x[on_int] >= 1) & (x[on_int] <= W - 2) & (y[on_int] >= 1) & (y[on_int] <= H - 2))
    bad = edge & ~on_int
    inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    mask = sc["masks"][frame].astype(np.float32)
    ms = np.full(len(x), np.nan)
    ms[inb] = map_coordinates(mask, [y[inb], x[inb]], output=np.float64)
    bad |= inb & (np.abs(ms - 0.1) < 1e-6)
    static = inb & (ms < 0.1)
    bad |= static & (np.abs(depth - 1e-3) < 1e-9)
    kept = static & (depth > 1e-3)
    v64 = np.zeros(len(x))
    v64[kept] = map_coordinates(sc["pred"][frame], [y[kept], x[kept]], output=np.float64)
    bad |= kept & (f32_midpoint_close(v64, 1e-9) | (v64 < 0))
    # conditioning of the kept points' projection
    A = np.abs(w2c[:3]) @ np.abs(h_pt)
    B = np.abs(K) @ A
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.maximum.reduce([B[0] / np.abs(K @ out[:3, :])[0], B[1] / np.abs(K @ out[:3, :])[1], B[2] / np.abs(depth)])
    bad |= kept & ~(cond < 100)
    # the kept indices from the reference's own columns
    ref = g["pts_list"][frame]
    idx, j = [], 0
    for k in range(ref.shape[1]):
        while not (np.array_equal(im[:, j], ref[:, k]) and depth[j] == g["mvs_depths"][frame][k]):
            j += 1
        idx.append(j)
        j += 1
    idx = np.array(idx, np.int64)
    assert np.array_equal(idx, np.where(kept)[0]), (frame, len(idx), kept.sum())
    return np.where(bad)[0], idx, int(((x > W - 1) & (x < W) & inb | (y > H - 1) & (y < H) & inb)[idx].sum())


def frame_guards(name, g, frame, n_points):
    pred, mvs = g["pred_depths"][frame], g["mvs_depths"][frame]
    n = len(pred)
    assert pred.dtype == np.float32 and mvs.dtype == np.float64
    assert 0.2 * n_points <= n <= 0.95 * n_points, (name, frame, n, n_points)
    nn_disp, mvs_disp = 1 / (pred + TINY), 1 / (mvs + TINY)
    assert nn_disp.dtype == np.float32
    nn_s, mvs_s = nn_disp - np.median(nn_disp), mvs_disp - np.median(mvs_disp)
    ratio = mvs_s / (nn_s + TINY)
    diff = np.abs(nn_s / (np.mean(np.abs(nn_s)) + TINY) - mvs_s / (np.mean(np.abs(mvs_s)) + TINY))
    flag = g["all_flag_trim"][frame]
    s = np.sort(diff)
    a = int(np.floor(0.8 * (n - 1)))
    assert s[a + 1] - s[a] > 1e-4 * s[a + 1], (name, frame, "quantile neighbours")
    assert np.array_equal(flag, diff <= np.quantile(diff, 0.8)) and flag.sum() == a + 1
    fits = [g[f"all_disp_indiv_{k}"][frame] for k in ("scales_med", "shifts_med", "scales_trim", "shifts_trim")]
    for keys, sub in ((nn_disp, None), (mvs_disp, None), (ratio, None), (mvs_disp - nn_disp * fits[0], None), (ratio, flag),
                      (mvs_disp - nn_disp * fits[2], flag)):
        assert median_neighbours_differ(keys if sub is None else keys[sub]), (name, frame, "median neighbours")
    for sub in (np.ones(n, bool), flag):
        r, ns, nd = ratio[sub], nn_s[sub], nn_disp[sub]
        order = np.argsort(r)
        for k in {(len(r) - 1) // 2, len(r) // 2}:
            assert abs(nd[order[k]] / ns[order[k]]) < 1e3, (name, frame, "conditioning of the ratio median")
    assert abs(fits[0] - fits[2]) > 1e-3 * abs(fits[0]) and abs(fits[1] - fits[3]) > 1e-3 * abs(fits[1]), (name, frame, fits)


def error_guards(name, files):
    for i, d in files.items():
        for p in ("med_share", "med_indiv", "trim_share", "trim_indiv"):
            assert d[f"mae_{p}"] < 1e3 * abs(d[f"me_{p}"]), (name, i, p, d[f"mae_{p}"], d[f"me_{p}"])


def settle(name, sc):
    for it in range(40):
        g, files = run_reference(sc)
        bad_all, idxs, quirks = set(), [], 0
        for frame in range(len(sc["pred"])):
            bad, idx, q = point_guards(sc, g, frame)
            bad_all |= set(bad.tolist())
            idxs.append(idx)
            quirks += q
        if not bad_all:
            return g, files, idxs, quirks
        print(f"    scene {name}: nudging {len(bad_all)} points (round {it})")
        sel = np.array(sorted(bad_all))
        on_int = sc["integer"][sel]
        sc["pts"][sel[~on_int], it % 2] += np.float32(NUDGE)
        sc["pts"][sel[on_int], 0] += sc["pts"][sel[on_int], 2] / np.float32(sc["focal"])  # one whole pixel to the right
    raise AssertionError("the guard bands did not clear")


def main():
    _install_stubs()
    torch.set_num_threads(1)
    out = {"numpy_version": np.array(np.__version__), "scenes": np.array(["A", "B", "C", "D"])}
    for name, build in (("A", scene_a), ("B", scene_b), ("C", scene_c), ("D", scene_d)):
        sc = build()
        g, files, idxs, quirks = settle(name, sc)
        F = len(sc["pred"])
        if name == "C":
            assert [len(i) for i in idxs] == [1, 2], [len(i) for i in idxs]
            assert files[0]["disp_indiv_scale_med"] == 0.0 and files[0]["disp_indiv_scale_trim"] == 0.0 and g["all_flag_trim"][0].all()
            assert files[1]["disp_indiv_scale_med"] > 0.0  # the two-point frame's fit is not the clamp
            print(f"    scene C frame 1: flag_trim {g['all_flag_trim'][1].tolist()}")
        else:
            for frame in range(F):
                frame_guards(name, g, frame, len(sc["pts"]))
            error_guards(name, files)
        if name == "B":
            assert quirks >= 10 and sc["integer"][idxs[0]].sum() >= 10, (quirks, sc["integer"][idxs[0]].sum())
            assert (files[0]["pcl_depth_pred"] == 0).sum() >= 10
        pre = f"{name}_"
        out[pre + "H"], out[pre + "W"], out[pre + "F"] = np.array(sc["H"]), np.array(sc["W"]), np.array(F)
        out[pre + "poses_bounds"], out[pre + "pts3d"] = sc["poses"], sc["pts"]
        out[pre + "masks"], out[pre + "pred"] = sc["masks"], np.stack(sc["pred"])
        out[pre + "w2c"], out[pre + "K"] = g["all_w2c"], g["all_K"]
        for i in range(F):
            d = files[i]
            assert sorted(d) == sorted(SAVED), sorted(d)
            assert np.array_equal(d["sparse_pcl"], sc["pts"]) and d["sparse_pcl"].dtype == np.float32
            assert np.array_equal(d["depth_pred"], sc["pred"][i]) and d["depth_pred"].dtype == np.float32
            assert d["proj_pcl"].dtype == np.float64 and d["pcl_depth_mvs"].dtype == np.float64
            assert d["pcl_depth_pred"].dtype == np.float32 and d["depth_is_disp"].dtype == bool and not d["depth_is_disp"]
            for k in SAVED:
                if k not in BULKY_SAME_AS_INPUT:
                    out[f"{pre}f{i}_{k}"] = d[k]
            out[f"{pre}f{i}_index"], out[f"{pre}f{i}_flag_trim"] = idxs[i], g["all_flag_trim"][i]
            print(f"    scene {name} frame {i}: kept {len(idxs[i])} of {len(sc['pts'])}, trimmed to {int(g['all_flag_trim'][i].sum())}, "
                  f"scale {float(d['disp_indiv_scale_med']):.4f} / {float(d['disp_indiv_scale_trim']):.4f}")
    np.savez_compressed(OUT / "zoe_align.npz", **out)
    print(f"  zoe_align.npz {(OUT / 'zoe_align.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


if __name__ == "__main__":
    main()
