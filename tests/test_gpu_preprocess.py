"""The preprocessing kernels on the MI355X (csrc/preprocess.hip) against the reference's fixtures and, for the opening, a
scipy statement computed here: never against themselves.

flow consistency  every fixture pair (2x2, 5x7, 37x53, 70x130; zero, even-integer and coherent flows with targets on the
                  last row / column, half outside on all four sides, wholly outside, and one flow of 1e4): coord_diff within
                  TOL_ULPS of the fixture (the unit and where the figure comes from: test_preprocess_host.py), the
                  thresholded masks bit for bit, zero flow exactly zero.
epipolar mask     the fixture's five frames: mask exactly, e_dist to a relative 1e-9 (well above the double rounding of a
                  ten-operation expression, far below anything a 1-pixel threshold sees).  Hand-made raw patterns through a
                  degenerate F (d = |flow_y| / (1 + 1e-8), so flow_y = 2 sets a pixel and 0.5 clears it): single pixels,
                  a lone plus, a 2-pixel line, borders and corners, the seams of the 64 x 16 tiles on both axes, H = 2 and
                  W = 3 with all 64 patterns."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from test_preprocess_host import CASES, TOL_ULPS, _write_epi_tree, coord_diff_ulps, occ

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
F_ROWS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # l = (0, 1, -y): d = |flow_y| / (1 + 1e-8)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def flow_fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_flow.npz"))


@pytest.fixture(scope="module")
def epi_fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_epi.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def opening(raw):
    return ndi.binary_dilation(ndi.binary_erosion(raw, structure=CROSS, border_value=True), structure=CROSS, border_value=0)


# ---------------------------------------------------------------------------- flow consistency
@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (37, 53), (70, 130)])
def test_flow_consistency_vs_fixture(flow_fx, H, W):
    from pgdvs_amd import ops

    for case in CASES:
        tag = f"{H}x{W}_{case}"
        f12, f21 = flow_fx[f"{tag}_flow12"], flow_fx[f"{tag}_flow21"]
        cd1, cd2 = ops.flow_consistency(dev(f12), dev(f21))
        torch.cuda.synchronize()
        assert cd1.dtype == torch.float32 and tuple(cd1.shape) == (H, W, 2) == tuple(cd2.shape)
        for got, want, a, b in ((cd1.cpu().numpy(), flow_fx[f"{tag}_cd1"], f12, f21), (cd2.cpu().numpy(), flow_fx[f"{tag}_cd2"], f21, f12)):
            ulps, _ = coord_diff_ulps(got, want, a, b)
            print(f"{tag}: {ulps:.2f} ulp")
            assert np.isfinite(got).all()
            assert ulps <= TOL_ULPS, (tag, ulps)
            assert np.array_equal(occ(got), occ(want)), tag
            if case == "zero":
                assert not got.any()
        if case == "mix":
            assert np.abs(f12).max() == 1e4  # the large flow is in the case


def test_flow_consistency_public_path_and_files(flow_fx, tmp_path):
    """preprocess.flow_consistency(device=...) is the op, and write_flow_pair's files read back as the fixture's masks"""
    from pgdvs_amd import ops
    from pgdvs_amd.datasets._common import read_flow_npz
    from pgdvs_amd.preprocess import flow_consistency, write_flow_pair

    tag = "37x53_mix"
    f12, f21 = flow_fx[f"{tag}_flow12"], flow_fx[f"{tag}_flow21"]
    cd1, cd2 = flow_consistency(f12, f21, device=DEV)
    o1, o2 = ops.flow_consistency(dev(f12), dev(f21))
    assert np.array_equal(cd1, o1.cpu().numpy()) and np.array_equal(cd2, o2.cpu().numpy())
    p12, p21 = write_flow_pair(tmp_path, "a", "b", f12, f21, device=DEV)
    assert p12.name == "a_b.npz" and p21.name == "b_a.npz"
    for path, flow, cd in ((p12, f12, flow_fx[f"{tag}_cd1"]), (p21, f21, flow_fx[f"{tag}_cd2"])):
        got_flow, got_occ = read_flow_npz(path)
        assert np.array_equal(got_flow, flow) and np.array_equal(got_occ, occ(cd))


def test_flow_consistency_writes_only_its_outputs():
    """both outputs between guard words, at a size that fills no block in either direction"""
    from pgdvs_amd import _lib, ops

    H, W, guard = 5, 67, 64
    rng = np.random.default_rng(3)
    f12 = dev((rng.normal(size=(H, W, 2)) * 40).astype(np.float32))  # most targets outside
    f21 = dev((rng.normal(size=(H, W, 2)) * 40).astype(np.float32))
    n = H * W * 2
    buf = torch.full((2 * n + 3 * guard,), -7.25, dtype=torch.float32, device=DEV)
    rc = _lib.load().pgdvs_flow_consistency(f12.data_ptr(), f21.data_ptr(), H, W, buf.data_ptr() + 4 * guard,
                                            buf.data_ptr() + 4 * (2 * guard + n), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    out = buf.cpu().numpy()
    for lo, hi in ((0, guard), (guard + n, 2 * guard + n), (2 * guard + 2 * n, 3 * guard + 2 * n)):
        assert (out[lo:hi] == -7.25).all()
    want1, want2 = ops.flow_consistency(f12, f21)
    assert np.array_equal(out[guard:guard + n], want1.cpu().numpy().reshape(-1))
    assert np.array_equal(out[2 * guard + n:2 * guard + 2 * n], want2.cpu().numpy().reshape(-1))


# ---------------------------------------------------------------------------- epipolar mask
def test_epipolar_mask_vs_fixture(epi_fx, tmp_path):
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess import epipolar_motion_mask

    names = _write_epi_tree(epi_fx, tmp_path)
    n = len(names)
    for i in range(n):
        mask, dist = ops.epipolar_mask(dev(epi_fx[f"f{i}_flow"]), dev(epi_fx[f"f{i}_coord_diff"]), epi_fx[f"f{i}_F"], want_dist=True)
        torch.cuda.synchronize()
        assert mask.dtype == torch.uint8 and dist.dtype == torch.float64
        got, e, want_e = mask.cpu().numpy(), dist.cpu().numpy(), epi_fx[f"f{i}_e_dist"]
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), epi_fx[f"f{i}_mask"]), i
        rel = np.abs(e - want_e) / np.maximum(np.abs(want_e), np.finfo(np.float64).tiny)
        print(f"frame {i}: e_dist relative deviation {rel.max():.3g}")
        assert np.array_equal(e == 0, want_e == 0) and rel.max() <= 1e-9, (i, rel.max())
        # without the distance output, and through the public function
        assert np.array_equal(ops.epipolar_mask(dev(epi_fx[f"f{i}_flow"]), dev(epi_fx[f"f{i}_coord_diff"]), epi_fx[f"f{i}_F"]).cpu().numpy(), got)
        pub = epipolar_motion_mask(i, n, epi_fx["w2c"], epi_fx["K"], tmp_path, names, device=DEV)
        assert pub.dtype == bool and np.array_equal(pub, epi_fx[f"f{i}_mask"]), i


def run_pattern(raw, inconsistent=None):
    """the kernel on a hand-made raw pattern: flow_y = 2 where raw is set, 0.5 elsewhere; ``inconsistent`` pixels fail the
    flow-consistency gate and count as clear.  Returns (mask, e_dist)."""
    from pgdvs_amd import ops

    H, W = raw.shape
    flow = np.zeros((H, W, 2), np.float32)
    flow[..., 0] = 3.0  # along the line: no effect on the distance
    flow[..., 1] = np.where(raw, 2.0, 0.5)
    cd = np.zeros((H, W, 2), np.float32)
    if inconsistent is not None:
        cd[inconsistent] = (0.75, -0.5)
    mask, dist = ops.epipolar_mask(dev(flow), dev(cd), F_ROWS, want_dist=True)
    torch.cuda.synchronize()
    return mask.cpu().numpy().astype(bool), dist.cpu().numpy(), flow, cd


def plus(raw, y, x):
    for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        if 0 <= y + dy < raw.shape[0] and 0 <= x + dx < raw.shape[1]:
            raw[y + dy, x + dx] = True


def test_opening_hand_made_patterns():
    from pgdvs_amd.preprocess.mask import masked_epipolar_distance_numpy

    H, W = 40, 150  # 3 x 3 tiles of 64 x 16, the last ones partial
    raw = np.zeros((H, W), bool)
    raw[5, 5] = raw[5, 20] = raw[20, 70] = True           # single pixels: removed
    plus(raw, 8, 30)                                       # a lone plus: survives exactly
    raw[12, 40:42] = True                                  # a 2-pixel line: removed
    raw[0, 0] = raw[0, 1] = raw[1, 0] = True               # each corner with its two in-image neighbours: survives
    raw[0, W - 1] = raw[0, W - 2] = raw[1, W - 1] = True
    raw[H - 1, 0] = raw[H - 1, 1] = raw[H - 2, 0] = True
    raw[H - 1, W - 1] = raw[H - 1, W - 2] = raw[H - 2, W - 1] = True
    plus(raw, 0, 50), plus(raw, H - 1, 90), plus(raw, 20, 0), plus(raw, 25, W - 1)  # pluses centred on each border
    raw[0, 100] = raw[30, 0] = True                        # single pixels on borders: removed
    for y, x in ((15, 63), (16, 64), (31, 128), (32, 127), (15, 10), (16, 100), (10, 64), (36, 63)):
        plus(raw, y, x)                                    # pluses across the tile seams on both axes
    raw[14:18, 126:130] = True                             # a block over a tile corner
    raw[15, 80] = raw[16, 80] = True                       # a 2-pixel line across a seam: removed
    want = opening(raw)
    single = np.zeros_like(raw)
    single[5, 5] = single[5, 20] = single[20, 70] = single[0, 100] = single[30, 0] = single[12, 40] = single[15, 80] = True
    assert not want[single].any() and want[8, 29:32].all() and want[0, 0] and want[H - 1, W - 1] and want[0, W - 1] and want[H - 1, 0]
    lone = np.zeros_like(raw)
    plus(lone, 8, 30)
    assert np.array_equal(want[6:11, 28:33], lone[6:11, 28:33])
    got, e, flow, cd = run_pattern(raw)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    want_e = masked_epipolar_distance_numpy(flow, cd, F_ROWS)
    assert np.abs(e / want_e - 1).max() <= 1e-9 and set(np.round(want_e, 3).ravel()) == {0.5, 2.0}
    # the consistency gate clears set pixels: a plus loses its centre and goes
    gate = np.zeros_like(raw)
    gate[8, 30] = gate[16, 64] = True
    got_g, e_g, _, _ = run_pattern(raw, gate)
    assert np.array_equal(got_g, opening(raw & ~gate)) and not got_g[8, 29:32].any()
    assert (e_g[gate] == 0).all() and np.array_equal(e_g[~gate], e[~gate])
    # a dense random pattern over the same tiling
    rnd = np.random.default_rng(5).random((H, W)) < 0.8
    assert np.array_equal(run_pattern(rnd)[0], opening(rnd)) and 0 < opening(rnd).mean() < 1


def test_opening_smallest_shapes():
    """H = 2 and W = 3: every one of the 64 patterns; and 2 x 2, 3 x 2 at a few"""
    for code in range(64):
        raw = np.array([(code >> k) & 1 for k in range(6)], bool).reshape(2, 3)
        got = run_pattern(raw)[0]
        assert np.array_equal(got, opening(raw)), (code, got, opening(raw))
    corner = np.array([[1, 1, 0], [1, 0, 0]], bool)
    assert np.array_equal(opening(corner), corner)  # the corner pixel survives the erosion and grows back to the three
    for shape in ((2, 2), (3, 2), (17, 2), (2, 65)):
        rnd = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape) < 0.75
        assert np.array_equal(run_pattern(rnd)[0], opening(rnd)), shape


def test_epipolar_mask_thresholds():
    """threshold and consist_thres reach the kernel: d = 2 / (1 + 1e-8) sits on either side of 1.9 and 2.1, sum|cd| = 1.25 on
    either side of 1.0 and 1.5"""
    from pgdvs_amd import ops

    H, W = 6, 9
    flow = np.zeros((H, W, 2), np.float32)
    flow[..., 1] = 2.0
    cd = np.zeros((H, W, 2), np.float32)
    cd[..., 0], cd[..., 1] = 0.75, -0.5
    f, c = dev(flow), dev(cd)
    assert not ops.epipolar_mask(f, c, F_ROWS).any().item()                                       # gated
    assert ops.epipolar_mask(f, c, F_ROWS, consist_thres=1.5).all().item()
    assert ops.epipolar_mask(f, c, F_ROWS, consist_thres=1.25, threshold=1.9).all().item()      # <= : 1.25 passes
    assert not ops.epipolar_mask(f, c, F_ROWS, consist_thres=1.5, threshold=2.1).any().item()


def test_argument_checks_raise_and_launch_nothing():
    from pgdvs_amd import _lib, ops

    z = torch.zeros((1, 5, 2), device=DEV)
    with pytest.raises(ValueError):
        ops.flow_consistency(z, z)
    with pytest.raises(ValueError):
        ops.epipolar_mask(z, z, np.eye(3))
    with pytest.raises(ValueError):
        ops.flow_consistency(torch.zeros((4, 5, 2), device=DEV), torch.zeros((4, 6, 2), device=DEV))
    lib = _lib.load()
    out = torch.full((64,), 3.5, device=DEV)
    m = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    F = (_lib.C.c_double * 9)(*np.eye(3).reshape(-1).tolist())
    assert lib.pgdvs_flow_consistency(z.data_ptr(), z.data_ptr(), 1, 5, out.data_ptr(), out.data_ptr() + 128, ops._stream()) == -1
    assert b"bad shape" in lib.pgdvs_last_error()
    assert lib.pgdvs_epipolar_mask(z.data_ptr(), z.data_ptr(), 5, 1, F, 1.0, 1.0, m.data_ptr(), None, ops._stream()) == -1
    assert b"bad shape" in lib.pgdvs_last_error()
    assert lib.pgdvs_epipolar_mask(z.data_ptr(), z.data_ptr(), 2, 2, None, 1.0, 1.0, m.data_ptr(), None, ops._stream()) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 3.5).all() and (m.cpu().numpy() == 7).all()
