"""CoTracker on the MI355X: the two ops of csrc/cotracker.hip and the model with its HIP correlation step against what the
reference's own classes computed on the CPU (tests/golden/cotracker_*.npz, see tests/test_cotracker_host.py for the cases
and the tolerance rule: |ours - reference float64| <= 4 x the reference's own float32-vs-float64 gap of that case).

ops.cotracker_pyramid       against F.avg_pool2d on the CPU, to 2 float32 spacings of the level's largest value (a mean of
                            four in one fixed order; the pooling of the CPU library may associate differently)
ops.cotracker_corr_lookup   the four look-up fixtures: values within tol, exact zeros where every tap of level 0 is outside
                            the level, a 456-wide destination whose other columns keep their sentinel, the same bits
                            from two calls, and the shapes the entry points reject
the model                   one refinement step (iters 1 and 2), fnet, both forward cases and the interface on the device,
                            the HIP statement asserted taken; the HIP statement against the torch statement on the device
run_track                   PGDVSDynamicTrackRenderer.run_track with the interface plugged in: shapes, and both halves run
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cotracker_cases as CC
from test_cotracker_host import (check_fnet, check_forward, check_interface, check_step, err, make_interface, run_step, step_model,
                                 tamed_model)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def fx_lookup(golden_dir):
    return dict(np.load(golden_dir / "cotracker_lookup.npz"))


@pytest.fixture(scope="module")
def fx_model(golden_dir):
    return dict(np.load(golden_dir / "cotracker_model.npz"))


@pytest.fixture(scope="module")
def full_gain_model():
    return step_model(DEV)


@pytest.fixture(scope="module")
def whole_model():
    return tamed_model(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- the ops
@pytest.mark.parametrize("name", ["even_n37", "odd_n37"])
def test_pyramid_vs_avg_pool(name):
    from pgdvs_amd import ops

    fmaps = torch.from_numpy(CC.lookup_inputs(name)[0])
    pyr = ops.cotracker_pyramid(fmaps.to(DEV))
    torch.cuda.synchronize()
    want = fmaps
    for lvl in range(4):
        got = pyr.level(lvl).cpu()
        assert got.shape == (want.shape[0], want.shape[2], want.shape[3], 128)
        e, bound = float((got - want.permute(0, 2, 3, 1)).abs().max()), 2.0 * float(np.spacing(np.float32(want.abs().max())))
        print(f"{name} level {lvl} {tuple(got.shape)}: max |d| = {e:.3g}, bound {bound:.3g}")
        assert e <= bound
        want = F.avg_pool2d(want, 2, stride=2)
    assert tuple(want.shape[-2:]) == (fmaps.shape[-2] >> 4, fmaps.shape[-1] >> 4)


@pytest.mark.parametrize("name", list(CC.LOOKUP_CASES))
def test_corr_lookup_vs_fixture(fx_lookup, name):
    from pgdvs_amd import ops

    fmaps, feats, coords, kind = CC.lookup_inputs(name)
    assert CC.checksum(fmaps, feats, coords) == fx_lookup[f"{name}__chk"]
    S, N = feats.shape[:2]
    pyr = ops.cotracker_pyramid(dev(fmaps))
    out = ops.cotracker_corr_lookup(pyr, dev(feats), dev(coords))
    wide = torch.full((S, N, 456), SENTINEL, dtype=torch.float32, device=DEV)
    assert ops.cotracker_corr_lookup(pyr, dev(feats), dev(coords), out=wide, col_offset=130) is wide
    torch.cuda.synchronize()
    got, wide = out.cpu().numpy(), wide.cpu().numpy()
    e, tol = err(got, fx_lookup[f"{name}__f64"]), float(fx_lookup[f"{name}__tol"])
    print(f"{name}: max |ours - float64 reference| = {e:.3g}, tol {tol:.3g}")
    assert got.shape == (S, N, 196) and np.isfinite(got).all() and e <= tol
    zero = (kind == 5) | (kind == 7)
    assert zero.any() and not got[zero][:, :49].any()  # every tap of level 0 outside the level: exact zeros
    assert np.array_equal(wide[:, :, 130:326], got)  # the same bits from a second call, at the offset
    assert (wide[:, :, :130] == SENTINEL).all() and (wide[:, :, 326:] == SENTINEL).all()


def test_rejects():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    ok = torch.zeros((2, 128, 16, 16), device=DEV)
    for bad in (torch.zeros((2, 64, 16, 16), device=DEV), torch.zeros((2, 128, 15, 16), device=DEV), torch.zeros((2, 128, 16, 15), device=DEV)):
        with pytest.raises(ops.PgdvsHipError):  # C != 128; a last level of 1 x 2, of 2 x 1
            ops.cotracker_pyramid(bad)
        assert ops.cotracker_pyramid(bad, reject_ok=True) is None
        assert lib.pgdvs_cotracker_pyramid_workspace_bytes(*bad.shape) < 0
    assert lib.pgdvs_cotracker_pyramid_workspace_bytes(0, 128, 16, 16) < 0  # S = 0
    pyr = ops.cotracker_pyramid(ok)
    feats, coords = torch.zeros((2, 3, 128), device=DEV), torch.zeros((2, 3, 2), device=DEV)
    out = torch.full((2, 3, 300), SENTINEL, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda S, H, W, N, stride, off: lib.pgdvs_cotracker_corr_lookup(p(pyr.buf), S, H, W, p(feats), p(coords), N, p(out), stride, off, None)
    assert call(2, 16, 16, 3, 300, 104) == 0  # the last offset that fits
    for args in ((2, 16, 16, 3, 300, 105), (2, 16, 16, 3, 195, 0), (2, 16, 16, 3, 300, -1), (2, 16, 16, 0, 300, 0), (0, 16, 16, 3, 300, 0),
                 (2, 15, 16, 3, 300, 0), (2, 16, 16, (1 << 31) // (2 * 196) + 1, 300, 0)):
        assert call(*args) != 0, args
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, :104] == SENTINEL).all() and not (got[:, :, 104:] == SENTINEL).any()  # only the accepted call wrote


# ---------------------------------------------------------------- the model with the HIP statement
@pytest.mark.parametrize("iters", [1, 2])
def test_forward_iteration_hip_vs_fixture(fx_model, full_gain_model, iters):
    check_step(full_gain_model, fx_model, iters, DEV)
    assert full_gain_model.last_corr_path == "hip"


def test_forward_iteration_hip_vs_torch_on_device(fx_model, full_gain_model):
    """the two statements on the same device, one step: apart by no more than the two float32 errors the fixture allows each"""
    hip = run_step(full_gain_model, fx_model, 1, DEV)
    assert full_gain_model.last_corr_path == "hip"
    full_gain_model.force_torch_corr = True
    try:
        ref = run_step(full_gain_model, fx_model, 1, DEV)
        assert full_gain_model.last_corr_path == "torch"
    finally:
        full_gain_model.force_torch_corr = False
    for a, b, key in ((hip[0], ref[0], "step1_coords"), (hip[1], ref[1], "step1_vis")):
        e, tol = err(a, b), 2.0 * float(fx_model[f"tol_{key}"])
        print(f"{key}: max |hip - torch| = {e:.3g}, bound {tol:.3g}")
        assert e <= tol


def test_autograd_keeps_the_torch_statement(full_gain_model):
    x = {k: dev(v) for k, v in CC.step_inputs().items()}
    preds, _, _ = full_gain_model.forward_iteration(iters=1, **x)  # gradients enabled, parameters require them
    assert full_gain_model.last_corr_path == "torch" and preds[-1].requires_grad


@pytest.mark.parametrize("size", CC.FNET_SIZES)
def test_fnet_vs_fixture(fx_model, full_gain_model, size):
    check_fnet(full_gain_model, fx_model, size, DEV)


@pytest.mark.parametrize("name", list(CC.FORWARD_CASES))
def test_forward_vs_fixture(fx_model, whole_model, name):
    whole_model.last_corr_path = None
    check_forward(whole_model, fx_model, name, DEV)
    assert whole_model.last_corr_path == "hip"


def test_interface_vs_fixture(fx_model):
    iface = make_interface(fx_model, DEV)
    check_interface(iface, fx_model, DEV)
    assert iface.model.model.last_corr_path == "hip"


# ---------------------------------------------------------------- plugged into the renderer
def test_run_track_with_interface(fx_model):
    """a window with one frame before and one after the target, padded to five as prepare_data pads for a tracker"""
    from pgdvs_amd.models.cotracker import CoTrackerInterface
    from pgdvs_amd.renderers.pgdvs_renderer_dyn_track import PGDVSDynamicTrackRenderer

    class Recording(CoTrackerInterface):
        def __call__(self, *, frames, query_points):
            self.seen.append((frames.clone(), query_points.clone()))
            return super().__call__(frames=frames, query_points=query_points)

    tracker = Recording(None, ori_rgb_range="0_1", query_chunk_size=16).to(DEV).eval()
    tracker.seen = []
    renderer = PGDVSDynamicTrackRenderer.__new__(PGDVSDynamicTrackRenderer)
    torch.nn.Module.__init__(renderer)
    renderer.tracker, renderer.track_chunk_size = tracker, tracker.query_chunk_size
    H, W, n_actual, n_views = 24, 32, 2, 5
    rgbs = dev(CC.moving_pattern(n_actual, H, W, 51, scale=1.0).transpose(0, 2, 3, 1)).repeat(3, 1, 1, 1)[:n_views]
    masks = torch.zeros((n_views, H, W, 1), device=DEV)
    masks[0, 3:6, 4:8] = 1.0   # 12 queries on the frame before the target
    masks[1, 10:12, 20:30] = 1.0  # 20 on the frame after it: two chunks of 16
    dft = dict(rgbs_for_track=rgbs, dyn_masks_for_track=masks, n_actual_frames=n_actual, idx_real_track=[0, 1],
               idx_real_track_fwd=[0], idx_real_track_bwd=[1])
    query_pts, tracks, visibles = renderer.run_track(dft)
    torch.cuda.synchronize()
    assert query_pts.shape == (32, 3) and tracks.shape == (32, n_actual, 2) and visibles.shape == (32, n_actual)
    assert tracks.dtype == torch.float32 and visibles.dtype == torch.bool and bool(torch.isfinite(tracks).all()) and bool((tracks >= 0).all())
    assert torch.equal(query_pts[:12, 0], torch.zeros(12, device=DEV)) and torch.equal(query_pts[12:, 0], torch.ones(20, device=DEV))
    assert [s[1].shape[0] for s in tracker.seen] == [16, 16, 16]  # forward half: one chunk; backward half: two
    fwd, bwd = tracker.seen[0][0], tracker.seen[1][0]
    assert torch.equal(fwd, rgbs) and torch.equal(bwd[:n_actual], torch.flip(rgbs[:n_actual], dims=[0]))  # the backward half runs reversed
    assert bool((tracker.seen[1][1][:, 0] == 0).all())  # its queries start on the reversed clip's first frame
    assert tracker.model.model.last_corr_path == "hip"
