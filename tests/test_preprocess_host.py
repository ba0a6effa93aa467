"""pgdvs_amd.preprocess on the host (numpy / scipy.ndimage paths) against the reference's fixtures
(tests/golden/make_golden_preprocess.py -> preprocess_flow.npz, preprocess_epi.npz): coord_diff within a stated number of
float32 ulps and its thresholded mask bit for bit, the flow_epi mask and the fundamental matrix exactly, the tree run_flow
writes as read_flow_npz reads it, the three direction branches with the tie, and the C ABI's declarations."""
import pathlib
import re

import numpy as np
import PIL.Image
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CASES = ("zero", "int", "mix")

# coord_diff: the numpy restatement against torch's grid_sample (the fixture), in ulps of the largest coordinate,
# max(H, W) - 1.  Measured here on the fixture's twelve pairs: at most 1 ulp (3.8e-6 at 37x53, 7.6e-6 at 70x130), on 1-4 % of
# the pixels; torch's vectorised CPU kernel is free to fuse its products and sums.  The bound for anything that follows the
# same float32 recipe, the HIP kernel included, is four times that.  At the handful of pixels that hold the flow of 1e4 or
# sample it, the numbers rounded are of that size, not of the image's, and the same 1 ulp was measured in THEIR unit
# (4.9e-4 where a weight times 1e4 lands in [4096, 8192)): there the ulp is that of the largest magnitude the pixel's own
# arithmetic touches (ulp_unit below), everywhere else exactly that of max(H, W) - 1.
MEASURED_ULPS = 1
TOL_ULPS = 4 * MEASURED_ULPS


def ulp_unit(flow_a, flow_b, want):
    """per pixel the float32 spacing at max(max(H, W) - 1, |c1|, |want|, |flow_b| on the 4 x 4 texels around c1)"""
    H, W = flow_a.shape[:2]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    c1x, c1y = xs + flow_a[..., 0], ys + flow_a[..., 1]
    mag = np.maximum(np.float32(max(H, W) - 1), np.maximum(np.abs(c1x), np.abs(c1y)))
    mag = np.maximum(mag, np.abs(want).max(-1))
    big_b = np.abs(flow_b).max(-1)
    x0, y0 = np.floor(c1x), np.floor(c1y)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            cx, cy = x0 + dx, y0 + dy
            ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            near = big_b[np.where(ok, cy, 0).astype(np.int64), np.where(ok, cx, 0).astype(np.int64)]
            mag = np.maximum(mag, np.where(ok, near, 0))
    return np.spacing(mag.astype(np.float32)).astype(np.float64)


def coord_diff_ulps(got, want, flow_a, flow_b):
    """the largest deviation of got from want in the pixel's ulps, and the share of pixels whose unit is the image's"""
    H, W = want.shape[:2]
    unit = ulp_unit(flow_a, flow_b, want)
    plain = unit == float(np.spacing(np.float32(max(H, W) - 1)))
    return float((np.abs(got.astype(np.float64) - want).max(-1) / unit).max()), float(plain.mean())


@pytest.fixture(scope="module")
def flow_fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_flow.npz"))


@pytest.fixture(scope="module")
def epi_fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_epi.npz"))


def occ(cd):
    return (np.sum(np.abs(cd), axis=2) > 1.0).astype(np.float32)


def test_flow_consistency_numpy_vs_fixture(flow_fx):
    from pgdvs_amd.preprocess import flow_consistency

    worst = 0.0
    for H, W in flow_fx["sizes"]:
        for case in CASES:
            tag = f"{H}x{W}_{case}"
            cd1, cd2 = flow_consistency(flow_fx[f"{tag}_flow12"], flow_fx[f"{tag}_flow21"])
            f12, f21 = flow_fx[f"{tag}_flow12"], flow_fx[f"{tag}_flow21"]
            for got, want, a, b in ((cd1, flow_fx[f"{tag}_cd1"], f12, f21), (cd2, flow_fx[f"{tag}_cd2"], f21, f12)):
                assert got.dtype == np.float32 and got.shape == (H, W, 2)
                ulps, plain = coord_diff_ulps(got, want, a, b)
                worst = max(worst, ulps)
                assert ulps <= TOL_ULPS, (tag, ulps)
                assert plain > 0.9 or H * W < 100, (tag, plain)  # the wider unit is the exception
                assert np.array_equal(occ(got), occ(want)), tag
            if case == "zero":
                assert not cd1.any() and not cd2.any()
    print(f"worst deviation: {worst:.2f} ulp of max(H, W) - 1")
    assert worst <= MEASURED_ULPS  # the figure the tolerance is derived from still holds


def test_flow_consistency_argument_checks():
    from pgdvs_amd.preprocess import flow_consistency

    with pytest.raises(ValueError):
        flow_consistency(np.zeros((1, 5, 2), np.float32), np.zeros((1, 5, 2), np.float32))  # H = 1: upstream divides by H - 1
    with pytest.raises(ValueError):
        flow_consistency(np.zeros((4, 5, 2), np.float32), np.zeros((4, 6, 2), np.float32))
    with pytest.raises(ValueError):
        flow_consistency(np.zeros((4, 5, 3), np.float32), np.zeros((4, 5, 3), np.float32))


def test_run_flow_writes_the_interval_tree(flow_fx, tmp_path):
    """a stub model on five images: the file names per interval, and every .npz read back through read_flow_npz gives the
    fixture's flow and occlusion mask bit for bit"""
    from pgdvs_amd.datasets._common import read_flow_npz
    from pgdvs_amd.preprocess import run_flow

    H, W = 37, 53
    tag = f"{H}x{W}_mix"
    f12, f21 = flow_fx[f"{tag}_flow12"], flow_fx[f"{tag}_flow21"]
    img_dir = tmp_path / "rgbs"
    img_dir.mkdir()
    stems = [f"{i:05d}" for i in (3, 0, 4, 1, 2)]  # written out of order: the list is sorted
    for s in stems:
        PIL.Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(img_dir / f"{s}.png")
    (img_dir / "notes.txt").write_text("not an image")
    calls = []

    def model(img_f1, img_f2):
        calls.append((pathlib.Path(img_f1).stem, pathlib.Path(img_f2).stem))
        return f12.transpose(2, 0, 1)[None], f21.transpose(2, 0, 1)[None]  # [1,2,H,W] each

    out_dir = tmp_path / "flows"
    written = run_flow(img_dir, out_dir, model, img_pair_max_diff=3)
    want_calls = [(f"{i:05d}", f"{i + k:05d}") for k in (1, 2, 3) for i in range(5 - k)]
    assert calls == want_calls
    assert sorted(p.name for p in out_dir.iterdir()) == ["interval_1", "interval_2", "interval_3"]
    for k in (1, 2, 3):
        names = sorted(p.name for p in (out_dir / f"interval_{k}").iterdir())
        want = sorted([f"{i:05d}_{i + k:05d}.npz" for i in range(5 - k)] + [f"{i + k:05d}_{i:05d}.npz" for i in range(5 - k)])
        assert names == want  # and nothing else: no colour wheel, no debug collage
    assert len(written) == 2 * (4 + 3 + 2)
    for a, b in want_calls:
        k = int(b) - int(a)
        for path, flow, cd in ((out_dir / f"interval_{k}" / f"{a}_{b}.npz", f12, flow_fx[f"{tag}_cd1"]),
                               (out_dir / f"interval_{k}" / f"{b}_{a}.npz", f21, flow_fx[f"{tag}_cd2"])):
            raw = np.load(path)
            assert sorted(raw.files) == ["coord_diff", "flow"]
            assert raw["flow"].dtype == raw["coord_diff"].dtype == np.float32 and raw["coord_diff"].shape == (H, W, 2)
            got_flow, got_occ = read_flow_npz(path)
            assert np.array_equal(got_flow, flow) and np.array_equal(got_occ, occ(cd))
            assert 0.2 < got_occ.mean() < 0.8


def test_run_flow_without_a_model_raises(tmp_path):
    from pgdvs_amd.preprocess import run_flow

    with pytest.raises(RuntimeError, match="model"):
        run_flow(tmp_path, tmp_path / "flows", None)
    assert not (tmp_path / "flows").exists()


def test_run_flow_rejects_a_wrong_model_output(tmp_path):
    from pgdvs_amd.preprocess import run_flow

    for i in range(2):
        PIL.Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(tmp_path / f"{i}.png")
    with pytest.raises(ValueError, match=r"\[1,2,H,W\]"):
        run_flow(tmp_path, tmp_path / "flows", lambda a, b: (np.zeros((4, 5, 2)), np.zeros((4, 5, 2))), img_pair_max_diff=1)


def test_fundamental_matrix_vs_fixture(epi_fx):
    from pgdvs_amd.preprocess import fundamental_matrix

    w2c, K = epi_fx["w2c"], epi_fx["K"]
    for i in range(len(w2c)):
        j = int(epi_fx[f"f{i}_other"])
        F = fundamental_matrix(np.dot(w2c[j], np.linalg.inv(w2c[i])), K[i], K[j])
        assert F.dtype == np.float64 and np.array_equal(F, epi_fx[f"f{i}_F"]), i


def _write_epi_tree(epi_fx, flow_dir):
    names = [str(n) for n in epi_fx["names"]]
    for i in range(len(names)):
        j = int(epi_fx[f"f{i}_other"])
        np.savez(flow_dir / f"{names[i]}_{names[j]}.npz", flow=epi_fx[f"f{i}_flow"], coord_diff=epi_fx[f"f{i}_coord_diff"])
    return names


def test_epipolar_motion_mask_numpy_vs_fixture(epi_fx, tmp_path):
    """only the chosen direction's file exists: the other one is never read"""
    from pgdvs_amd.preprocess import epipolar_motion_mask
    from pgdvs_amd.preprocess.mask import masked_epipolar_distance_numpy

    names = _write_epi_tree(epi_fx, tmp_path)
    n = len(names)
    for i in range(n):
        mask = epipolar_motion_mask(i, n, epi_fx["w2c"], epi_fx["K"], tmp_path, names)
        assert mask.dtype == bool and np.array_equal(mask, epi_fx[f"f{i}_mask"]), i
        e = masked_epipolar_distance_numpy(epi_fx[f"f{i}_flow"], epi_fx[f"f{i}_coord_diff"], epi_fx[f"f{i}_F"])
        assert np.array_equal(e, epi_fx[f"f{i}_e_dist"]), i
        assert ((e > 1.0) != mask).any()  # the opening removed something
    # another threshold is another mask
    assert epipolar_motion_mask(0, n, epi_fx["w2c"], epi_fx["K"], tmp_path, names, threshold=3.3).sum() < epi_fx["f0_mask"].sum()


def test_direction_branches_and_the_tie(epi_fx):
    from pgdvs_amd.preprocess.mask import choose_direction

    w2c = epi_fx["w2c"]
    n = len(w2c)
    got = [choose_direction(i, n, w2c) for i in range(n)]
    assert got == [bool(epi_fx[f"f{i}_use_prev"]) for i in range(n)] == [False, True, False, False, True]
    c = [np.linalg.inv(w2c[j])[:3, 3] for j in (2, 3, 4)]
    assert np.sum(np.abs(c[0] - c[1])) == np.sum(np.abs(c[2] - c[1]))  # frame 3: a tie, forward
    # flow_interval 2: frames 0, 1 forward only, frames 3, 4 backward only, frame 2 by distance
    assert [choose_direction(i, n, w2c, 2) for i in (0, 1, 3, 4)] == [False, False, True, True]
    c = [np.linalg.inv(w2c[j])[:3, 3] for j in (0, 2, 4)]
    assert choose_direction(2, n, w2c, 2) == bool(np.sum(np.abs(c[0] - c[1])) < np.sum(np.abs(c[2] - c[1])))
    # moving the next camera a hair away turns the tie into "previous"
    far = w2c.copy()
    far[4, 0, 3] -= 2.0 ** -20
    assert choose_direction(3, n, far) is True


def test_opening_borders():
    """the scipy statement of skimage's opening: a corner pixel with its two in-image neighbours survives, a lone pixel goes"""
    from pgdvs_amd.preprocess.mask import binary_opening_disk1

    raw = np.zeros((6, 7), bool)
    raw[0, 0] = raw[0, 1] = raw[1, 0] = True
    raw[3, 3] = True
    raw[5, 4:7] = raw[4, 5] = True  # a T on the last row: the plus whose fifth pixel lies outside the image
    raw[2, 6] = raw[3, 6] = True    # a 2-pixel line on the last column goes: its ends have clear in-image neighbours
    got = binary_opening_disk1(raw)
    want = np.zeros_like(raw)
    want[0, 0] = want[0, 1] = want[1, 0] = True
    want[5, 4:7] = want[4, 5] = True
    assert np.array_equal(got, want)


def test_header_declares_and_binding_binds_both_entry_points():
    from pgdvs_amd import _lib

    text = (ROOT / "include" / "pgdvs_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("pgdvs_flow_consistency", 7), ("pgdvs_epipolar_mask", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    # each cites the reference lines it replaces
    assert "common.py:211-233" in text and ":314-325 compute_occlusion" in text and "compute_mask.py:164-181" in text


def test_ops_refuse_cpu_tensors():
    import torch

    from pgdvs_amd import ops

    z = torch.zeros(4, 5, 2)
    with pytest.raises(ops.PgdvsHipError):
        ops.flow_consistency(z, z)
    with pytest.raises(ops.PgdvsHipError):
        ops.epipolar_mask(z, z, np.eye(3))
