"""The ZoeDepth stage's host path (pgdvs_amd/preprocess/zoedepth.py, device=None) against what the reference's own
compute_zoedepth.py wrote for the seeded scenes of tests/golden/make_golden_zoe_align.py (zoe_align.npz), and the plain
numpy statement of the spline the kernels compute against scipy.

sample_frame   kept indices equal, pcl_depth_pred bit for bit (the same scipy call), proj_pcl and pcl_depth_mvs to rtol
               1e-12: the reference's ``w2c @ h_pt`` goes through BLAS, whose operation order may differ by machine, and the
               generator asserts a conditioning below 100 for every kept point.
fit_frame      fed the fixture's stored samples: flag_trim equal, the four values bit for bit.
frame_errors   rtol 1e-12: the float64 summation-order bound n eps for n <= 1e5, with mean |diff| / |mean diff| < 1e3
               asserted by the generator.
run_zoedepth   writes upstream's tree for scene A; ``nvidia_eval.read_zoe_npz`` reads it back for a fixed key and for "moe".
               Fits to rtol 1e-8: the 1e-12 of the samples times the conditioning bound 1e3 the generator asserts at the
               medians, with one order of margin.

Shared with tests/test_gpu_zoe_align.py: the fixture access, the case list and the scene writer."""
import pathlib
import struct

import numpy as np
import PIL.Image
import pytest
import torch

SCENES = {"A": 5, "B": 3, "C": 2, "D": 1}
FRAMES = [(s, i) for s, n in SCENES.items() for i in range(n)]
FIT_KEYS = ("disp_indiv_scale_med", "disp_indiv_shift_med", "disp_indiv_scale_trim", "disp_indiv_shift_trim")
ERR_KEYS = tuple(f"{kind}_{fit}_{scope}" for kind in ("mae", "me") for fit in ("med", "trim") for scope in ("share", "indiv"))
ALL_KEYS = {"sparse_pcl", "proj_pcl", "pcl_depth_mvs", "pcl_depth_pred", "depth_pred", "depth_is_disp", *ERR_KEYS, *FIT_KEYS,
            *(k.replace("indiv", "share") for k in FIT_KEYS)}
RTOL_GEOMETRY, RTOL_ERRORS, RTOL_FIT_END_TO_END = 1e-12, 1e-12, 1e-8


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(golden_dir / "zoe_align.npz"))


def frame(fx, scene, i):
    """the fixture's inputs and the reference's outputs of one frame"""
    pre = f"{scene}_f{i}_"
    d = {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}
    d.update(pred=fx[f"{scene}_pred"][i], mask=fx[f"{scene}_masks"][i].astype(np.float32), pts3d=fx[f"{scene}_pts3d"],
             w2c=fx[f"{scene}_w2c"][i], K=fx[f"{scene}_K"][i])
    return d


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_samples(got, want, tag):
    pts, mvs, pred, idx = got
    assert idx.dtype == np.int64 and np.array_equal(idx, want["index"]), tag
    assert pred.dtype == np.float32 and np.array_equal(bits(pred), bits(want["pcl_depth_pred"])), tag
    assert pts.dtype == np.float64 and pts.shape == want["proj_pcl"].shape and mvs.dtype == np.float64
    np.testing.assert_allclose(pts, want["proj_pcl"], rtol=RTOL_GEOMETRY, atol=0, err_msg=tag)
    np.testing.assert_allclose(mvs, want["pcl_depth_mvs"], rtol=RTOL_GEOMETRY, atol=0, err_msg=tag)


def check_fit(fit, flag, want, tag):
    assert flag.dtype == bool and np.array_equal(flag, want["flag_trim"]), tag
    for k in FIT_KEYS:
        assert isinstance(fit[k], np.float64) and bits(fit[k]) == bits(np.float64(want[k])), (tag, k, fit[k], want[k])


def check_errors(err, want, tag):
    assert sorted(err) == sorted(ERR_KEYS)
    for k in ERR_KEYS:
        print(f"{tag} {k}: {err[k]!r} vs {float(want[k])!r}")
        np.testing.assert_allclose(err[k], want[k], rtol=RTOL_ERRORS, atol=0, err_msg=f"{tag} {k}")


def scales_shifts(want):
    return {k: want[k] for k in ALL_KEYS if k.startswith("disp_")}


def write_scene(root, fx, scene):
    """the scene's input files as run_zoedepth reads them"""
    root = pathlib.Path(root)
    for sub in ("rgbs", "masks/final", "sparse"):
        (root / sub).mkdir(parents=True)
    H, W = int(fx[f"{scene}_H"]), int(fx[f"{scene}_W"])
    for i, m in enumerate(fx[f"{scene}_masks"]):
        PIL.Image.fromarray(np.full((H, W, 3), 16 * i, np.uint8)).save(root / "rgbs" / f"{i:05d}.png")
        PIL.Image.fromarray(m).save(root / "masks/final" / f"{i:05d}_final.png")
    np.save(root / "poses_bounds_cvd.npy", fx[f"{scene}_poses_bounds"])
    with open(root / "sparse/points3D.bin", "wb") as f:
        pts = fx[f"{scene}_pts3d"]
        f.write(struct.pack("<Q", len(pts)))
        for i, p in enumerate(pts):
            f.write(struct.pack("<QdddBBBdQ", i + 1, float(p[0]), float(p[1]), float(p[2]), 1, 2, 3, 0.25, i % 3))
            f.write(struct.pack("<" + "ii" * (i % 3), *range(2 * (i % 3))))
    return root


class StoredDepth:
    """the plug-in model of the tests: the fixture's prediction of the frame, recognised by the image's grey level"""

    def __init__(self, fx, scene):
        self.pred = fx[f"{scene}_pred"]

    def __call__(self, X):
        assert X.ndim == 4 and X.shape[:2] == (1, 3) and X.dtype == torch.float32
        i = int(round(float(X[0, 0, 0, 0]) * 255 / 16))
        return torch.from_numpy(self.pred[i])[None, None].to(X.device)


def check_tree(files, fx, scene, rtol_fit):
    assert [f.name for f in files] == [f"{i:05d}.npz" for i in range(SCENES[scene])]
    for i, f in enumerate(files):
        got, want = dict(np.load(f)), frame(fx, scene, i)
        assert set(got) == ALL_KEYS and len(ALL_KEYS) == 22
        for k in ALL_KEYS - {"sparse_pcl", "depth_pred"}:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape)
        assert got["sparse_pcl"].dtype == np.float32 and np.array_equal(got["sparse_pcl"], want["pts3d"])
        assert got["depth_pred"].dtype == np.float32 and np.array_equal(got["depth_pred"], want["pred"])
        assert got["depth_is_disp"].dtype == bool and not got["depth_is_disp"]
        assert np.array_equal(bits(got["pcl_depth_pred"]), bits(want["pcl_depth_pred"]))
        np.testing.assert_allclose(got["proj_pcl"], want["proj_pcl"], rtol=RTOL_GEOMETRY, atol=0)
        for k in ALL_KEYS:
            if k.startswith("disp_"):
                np.testing.assert_allclose(got[k], want[k], rtol=rtol_fit, atol=0, err_msg=f"frame {i} {k}")
        for k in ERR_KEYS:  # the errors follow the fits they are made with: the fits' tolerance, one more order of margin
            np.testing.assert_allclose(got[k], want[k], rtol=10 * rtol_fit, atol=0, err_msg=f"frame {i} {k}")


# ---------------------------------------------------------------------------- against the fixture
def test_fixture_is_what_upstream_writes(fx):
    """22 entries per frame in upstream's file; the fixture leaves out the two that repeat its inputs"""
    assert len(ALL_KEYS) == 22 and list(fx["scenes"]) == list(SCENES)
    for scene, i in FRAMES:
        want = frame(fx, scene, i)
        assert ALL_KEYS - {"sparse_pcl", "depth_pred"} <= set(want)
        assert want["proj_pcl"].shape == (3, len(want["index"])) and want["flag_trim"].shape == want["index"].shape
    assert [len(frame(fx, "C", i)["index"]) for i in range(2)] == [1, 2]
    assert (frame(fx, "B", 0)["pcl_depth_pred"] == 0).sum() >= 10  # the zero-sample quirk is in the fixture


@pytest.mark.parametrize("scene,i", FRAMES)
def test_sample_frame_vs_fixture(fx, scene, i):
    from pgdvs_amd.preprocess import sample_frame

    want = frame(fx, scene, i)
    check_samples(sample_frame(want["pred"], want["mask"], want["pts3d"], want["w2c"], want["K"]), want, f"{scene}{i}")


@pytest.mark.parametrize("scene,i", FRAMES)
def test_fit_and_errors_vs_fixture(fx, scene, i):
    from pgdvs_amd.preprocess import fit_frame, frame_errors

    want = frame(fx, scene, i)
    fit, flag = fit_frame(want["pcl_depth_pred"], want["pcl_depth_mvs"])
    check_fit(fit, flag, want, f"{scene}{i}")
    check_errors(frame_errors(want["pcl_depth_pred"], want["pcl_depth_mvs"], want["flag_trim"], scales_shifts(want)), want, f"{scene}{i}")


def moe_choice(want):
    """the principle "moe" picks: the smallest |mean error|, the first of upstream's order among equals"""
    from pgdvs_amd.datasets.nvidia_eval import ZOE_PRINCIPLES

    return sorted(ZOE_PRINCIPLES, key=lambda k: abs(float(want[k])))[0]


def test_run_zoedepth_writes_upstreams_tree(fx, tmp_path):
    from pgdvs_amd.datasets.nvidia_eval import read_zoe_npz, select_zoe_pair, zoe_scale_shift_keys
    from pgdvs_amd.preprocess import run_zoedepth

    root = write_scene(tmp_path / "in" / "scene", fx, "A")
    dense = tmp_path / "zoe" / "scene" / "dense"
    for t in ("N", "K", "NK"):
        files = run_zoedepth(root, dense, root, StoredDepth(fx, "A"), t)
        assert files[0].parent == dense / f"zoe_depths_{t.lower()}"
    check_tree(files, fx, "A", RTOL_FIT_END_TO_END)
    assert not list(dense.rglob("*.ply"))
    for i in range(SCENES["A"]):
        want = frame(fx, "A", i)
        depth, scale, shift = read_zoe_npz(tmp_path / "zoe", None, "scene", i, "nk_me_trim_indiv")
        assert np.array_equal(depth, want["pred"])
        np.testing.assert_allclose([scale, shift], [want["disp_indiv_scale_trim"], want["disp_indiv_shift_trim"]], rtol=RTOL_FIT_END_TO_END)
        pair = select_zoe_pair(tmp_path / "zoe", None, "scene", i, "moe")
        assert pair == ("n", moe_choice(want)), (i, pair)  # three equal model types: the first wins
        depth, scale, shift = read_zoe_npz(tmp_path / "zoe", None, "scene", i, "moe")
        ks, kh = zoe_scale_shift_keys(pair[1])
        np.testing.assert_allclose([scale, shift], [want[ks], want[kh]], rtol=RTOL_FIT_END_TO_END)


def test_errors_raised(fx, tmp_path):
    from pgdvs_amd.preprocess import fit_frame, run_zoedepth, sample_frame

    with pytest.raises(ValueError, match="frame 7"):
        fit_frame(np.zeros(0, np.float32), np.zeros(0), frame=7)
    with pytest.raises(ValueError, match="frame 3.*negative"):
        fit_frame(np.array([1.0, -0.5], np.float32), np.array([1.0, 2.0]), frame=3)
    with pytest.raises(ValueError, match="negative"):
        fit_frame(np.array([1.0, 0.5], np.float32), np.array([1.0, -2.0]))
    with pytest.raises(ValueError, match="model"):
        run_zoedepth(tmp_path, tmp_path, tmp_path, None, "NK")
    with pytest.raises(ValueError, match="H, W >= 2"):
        sample_frame(np.ones((1, 5), np.float32), np.zeros((1, 5), np.float32), np.zeros((1, 3), np.float32), np.eye(4), np.eye(3))
    # a frame none of whose points is kept: every point behind the camera
    want = frame(fx, "C", 0)
    pts = want["pts3d"] * np.float32([1, 1, -1])
    pts[:, 2] = -np.abs(pts[:, 2])
    kept = sample_frame(want["pred"], want["mask"], pts, want["w2c"], want["K"])
    assert kept[0].shape == (3, 0) and kept[3].shape == (0,)
    with pytest.raises(ValueError, match="frame 0"):
        fit_frame(kept[2], kept[1], frame=0)


# ---------------------------------------------------------------------------- the spline, restated
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (23, 37), (70, 130)])
def test_numpy_spline_restatement_vs_scipy(H, W):
    """what csrc/zoe_align.hip computes, in plain numpy: coefficients to 1e-14 of the image's scale, 300 float32 samples
    per size bit for bit, coordinates from outside the image to the last fractional row and column and integer pixels"""
    from scipy.ndimage import map_coordinates, spline_filter

    from pgdvs_amd.preprocess.zoedepth import spline_coefficients_numpy, spline_sample_numpy

    rng = np.random.default_rng(100 * H + W)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    img = (2.0 + np.sin(xs / 3.0) * np.cos(ys / 2.0) + 0.1 * rng.random((H, W))).astype(np.float32)
    coef = spline_coefficients_numpy(img)
    ref = spline_filter(img, order=3, output=np.float64, mode="mirror")
    assert np.abs(coef - ref).max() <= 1e-14 * np.abs(ref).max()
    rows, cols = rng.uniform(-0.5, H + 0.5, 300), rng.uniform(-0.5, W + 0.5, 300)
    rows[:40], cols[20:60] = rng.integers(0, H, 40), rng.integers(0, W, 40)
    rows[60:70], cols[70:80] = rng.uniform(H - 1, H, 10), rng.uniform(W - 1, W, 10)
    want = map_coordinates(img, [rows, cols], order=3, mode="constant")
    got = spline_sample_numpy(coef, rows, cols)
    assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    outside = (rows < 0) | (rows > H - 1) | (cols < 0) | (cols > W - 1)
    assert outside.sum() >= 20 and not want[outside].any() and want[~outside].all()
