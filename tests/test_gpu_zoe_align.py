"""The ZoeDepth stage on the MI355X (csrc/zoe_align.hip) against what the reference's own compute_zoedepth.py wrote for
the seeded scenes of tests/golden/make_golden_zoe_align.py: never against the host path of this package.

ops.zoe_sample   kept indices equal; pcl_depth_pred bit for bit, which the generator's float32 guard band (no float64
                 spline value within 1e-9 relative of a rounding midpoint) makes a fair demand of any float64 evaluation
                 within 1e-9, and the kernel's chunked prefilter is within 1e-14; proj_pcl and pcl_depth_mvs to rtol 1e-12
                 (conditioning below 100 asserted by the generator).
ops.zoe_fit      fed the fixture's stored samples: flag_trim and the four values bit for bit (the 0.8 quantile's neighbours
                 differ by more than 1e-4 relative, so the float64-summed float32 mean cannot move the trim set, and every
                 median is an exact order statistic).
ops.zoe_errors   rtol 1e-12, the float64 summation-order bound.
run_zoedepth     device="cuda" end to end on scene A: the same files and keys, depth_pred equal, fits within rtol 1e-8 (the
                 1e-12 of the samples times the conditioning bound 1e3 asserted at the medians, one order of margin; a wrong
                 rank or trim set moves them by more than 1e-3).
Scene C's one-point and two-point frames and scene D's 300-column row (three chunks of the row pass, a row longer than a
workgroup) are cases of their own; scene B's rows are longer than a wavefront and hold the zero-sample quirk."""
import numpy as np
import pytest
import torch

from test_zoe_align_host import (FIT_KEYS, FRAMES, RTOL_FIT_END_TO_END, SCENES, StoredDepth, check_errors, check_fit, check_samples,
                                 check_tree, frame, scales_shifts, write_scene)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(golden_dir / "zoe_align.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("scene,i", FRAMES)
def test_zoe_sample_vs_fixture(fx, scene, i):
    from pgdvs_amd import ops

    want = frame(fx, scene, i)
    out = ops.zoe_sample(dev(want["pred"]), dev(want["mask"]), dev(want["pts3d"]), want["w2c"], want["K"])
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.float64, torch.float64, torch.float32, torch.int64]
    check_samples(tuple(t.cpu().numpy() for t in out), want, f"{scene}{i}")


@pytest.mark.parametrize("scene,i", FRAMES)
def test_zoe_fit_and_errors_vs_fixture(fx, scene, i):
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess.zoedepth import ERROR_PAIRS

    want = frame(fx, scene, i)
    pred, mvs = dev(want["pcl_depth_pred"]), dev(want["pcl_depth_mvs"])
    fit, flag, status = ops.zoe_fit(pred, mvs)
    torch.cuda.synchronize()
    assert fit.dtype == torch.float64 and flag.dtype == torch.bool and int(status.item()) == 0
    check_fit(dict(zip(FIT_KEYS, fit.cpu().numpy())), flag.cpu().numpy(), want, f"{scene}{i}")
    ss = scales_shifts(want)
    pairs = np.array([[ss[f"disp_{p.split('_')[1]}_{kind}_{p.split('_')[0]}"] for kind in ("scale", "shift")] for p in ERROR_PAIRS])
    err = ops.zoe_errors(pred, mvs, dev(want["flag_trim"]), pairs).cpu().numpy()
    check_errors({f"{kind}_{p}": err[4 * k + j] for k, kind in enumerate(("mae", "me")) for j, p in enumerate(ERROR_PAIRS)}, want,
                 f"{scene}{i}")


@pytest.mark.parametrize("scene", ["C", "D"])
def test_public_path_small_frames_and_long_row(fx, scene):
    """preprocess.sample_frame / fit_frame / frame_errors with a device are the ops"""
    from pgdvs_amd.preprocess import fit_frame, frame_errors, sample_frame

    for i in range(SCENES[scene]):
        want = frame(fx, scene, i)
        check_samples(sample_frame(want["pred"], want["mask"], want["pts3d"], want["w2c"], want["K"], device=DEV), want, f"{scene}{i}")
        fit, flag = fit_frame(want["pcl_depth_pred"], want["pcl_depth_mvs"], device=DEV, frame=i)
        check_fit(fit, flag, want, f"{scene}{i}")
        check_errors(frame_errors(want["pcl_depth_pred"], want["pcl_depth_mvs"], want["flag_trim"], scales_shifts(want), device=DEV), want,
                     f"{scene}{i}")


def test_run_zoedepth_on_device(fx, tmp_path):
    from pgdvs_amd.preprocess import run_zoedepth

    root = write_scene(tmp_path / "scene", fx, "A")
    files = run_zoedepth(root, tmp_path / "out", root, StoredDepth(fx, "A"), "NK", device=DEV)
    assert files[0].parent == tmp_path / "out" / "zoe_depths_nk"
    check_tree(files, fx, "A", RTOL_FIT_END_TO_END)


def test_errors_raised_on_device(fx):
    from pgdvs_amd import ops
    from pgdvs_amd._lib import PgdvsHipError
    from pgdvs_amd.preprocess import fit_frame

    want = frame(fx, "C", 1)
    cpu = [torch.from_numpy(np.ascontiguousarray(want[k])) for k in ("pred", "mask", "pts3d")]
    with pytest.raises(PgdvsHipError):
        ops.zoe_sample(*cpu, want["w2c"], want["K"])
    with pytest.raises(PgdvsHipError):
        ops.zoe_fit(torch.from_numpy(want["pcl_depth_pred"]), torch.from_numpy(want["pcl_depth_mvs"]))
    with pytest.raises(PgdvsHipError):
        ops.zoe_errors(dev(want["pcl_depth_pred"]), dev(want["pcl_depth_mvs"]), torch.from_numpy(want["flag_trim"]), np.ones((4, 2)))
    with pytest.raises(ValueError, match="frame 5.*negative"):
        fit_frame(np.array([1.0, -0.5, 2.0], np.float32), np.array([1.0, 2.0, 3.0]), device=DEV, frame=5)
    with pytest.raises(ValueError, match="frame 2"):
        fit_frame(np.zeros(0, np.float32), np.zeros(0), device=DEV, frame=2)
