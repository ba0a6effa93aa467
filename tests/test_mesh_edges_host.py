"""The mesh variant (row A10) without a GPU: the reference's own face lists (tests/golden/mesh_edges.npz) against the
explicit list of oracle/p3d_second.py and against the implicit (source pixel, kind) faces of orc_mesh_render; the
oracle's rasteriser -- candidate pixel range, z-buffer, face order -- against the naive every-pixel-against-every-face
statement on every case of tests/mesh_cases.py; the constructed cases against their integer-arithmetic expectations;
and float32 against float64.  What stays unpinned is said in oracle/p3d_second.py: the in-face formulas are one reading
of pytorch3d's CheckPixelInsideFace, shared by all statements here.  CPU only."""
import numpy as np
import pytest

import mesh_cases as mc
from mesh_cases import EXCLUDED_SHARE_CAP, RGB32_VS_64_MEASURED, RGB_VS_F64_ATOL  # the measured margins, stated there
from oracle import oracle as orc
from oracle import p3d_second as p3d


@pytest.fixture(scope="module")
def oracle_out():
    """orc.mesh_render on every case, once"""
    return {n: orc.mesh_render(c.keep, c.pcl, c.rgb, c.cam) for n, c in mc.cases().items()}


# ---------------------------------------------------------------- topology
@pytest.mark.parametrize("name", mc.topology_names())
def test_face_list_equals_reference(name):
    """mesh_faces_from_keep builds the reference's face list, row for row; no list at all where the reference took its
    ``torch.sum(flag_valid_v) == 0`` branch"""
    keep, faces, blank = mc.topology(name)
    mine = p3d.mesh_faces_from_keep(keep)
    assert mine.dtype == np.int64 and np.array_equal(mine, faces)
    assert blank == (faces.shape[0] == 0)
    if faces.shape[0]:
        assert faces.min() > 0  # vertex 0, the first kept pixel, is in no face


def test_fixture_cases_are_what_they_claim():
    first = lambda n: tuple(np.argwhere(mc.topology(n)[0])[0])
    for tag, (H, W) in (("a", (37, 61)), ("b", (61, 37))):
        assert mc.topology(f"all_{tag}")[0].shape == (H, W) and first(f"all_{tag}") == (0, 0)
        r, c = first(f"first_interior_{tag}")
        assert 0 < r < H - 1 and 0 < c < W - 1
        assert first(f"first_lastcol_{tag}")[1] == W - 1 and first(f"first_lastrow_{tag}")[0] == H - 1
        assert mc.topology(f"block_{tag}")[2] and mc.topology(f"block_lone_{tag}")[1].shape[0] == 2
        assert mc.topology(f"all_{tag}")[1].shape[0] == 2 * (H - 1) * (W - 1) - 2
        for n in ("first_lastrow", "empty", "single", "checker", "alt_rows", "last_row_col"):
            assert mc.topology(f"{n}_{tag}")[2], n
    assert [mc.topology(n)[0].shape for n in ("row_1x40", "col_40x1", "all_2x2")] == [(1, 40), (40, 1), (2, 2)]


def _pan_ids(keep):
    """every face id orc.mesh_render can produce for ``keep``: the flat source grid drawn four pixels to the cell at
    depth 1 (each face then holds several pixel centres strictly inside, at least an eighth of a pixel off its edges and
    its diagonal), the H x W window panned over the 4H x 4W sheet in steps that overlap by a cell"""
    H, W = keep.shape
    s = min(H, W) / 2.0
    cam = mc.flat_cam(H, W, s, s, W / 2.0, H / 2.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    seen = set()
    for oy in range(0, 4 * H, H - 4):
        for ox in range(0, 4 * W, W - 4):
            pcl = mc._unproject(cam, 4 * xx + 0.25 - ox, 4 * yy + 0.125 - oy, 1.0)
            face = orc.mesh_render(keep, pcl, np.zeros((H, W, 3), np.float32), cam)[2]
            seen.update(face[face >= 0].tolist())
    return np.array(sorted(seen), np.int64)


@pytest.mark.parametrize("name", mc.topology_names())
def test_oracle_face_ids_map_onto_reference_list(name):
    """the (kind, source pixel) ids the oracle draws, turned into vertex ranks, are the reference's faces -- the same set,
    and in the order of the ids the reference's order: all kind-1 rows, then all kind-2 rows, each in raster order"""
    keep, faces, _ = mc.topology(name)
    if min(keep.shape) < 6:  # 1 x 40, 40 x 1, 2 x 2: no room to pan, and no faces -- one render of the case's own sheet
        c = mc.cases()["topo_" + name]
        ids = np.unique(orc.mesh_render(c.keep, c.pcl, c.rgb, c.cam)[2])
        ids = ids[ids >= 0]
    else:
        ids = _pan_ids(keep)
    ranks = mc.ranks_of_ids(keep, ids)
    assert np.array_equal(ranks, faces)  # sorted ids <-> list order, row for row
    assert np.array_equal(mc.face_ids_of_list(keep, faces), ids)


# ---------------------------------------------------------------- rasteriser
@pytest.mark.parametrize("name", mc.names())
def test_oracle_equals_naive_float32(name, oracle_out):
    """no candidate range, explicit faces, min (z, index): winners and mask exact, colours bit for bit (same operation
    order).  This is the check that ndc_to_pix_range is a superset."""
    c = mc.cases()[name]
    img, mask, face = oracle_out[name]
    nv = mc.naive(name)
    assert np.array_equal(face, nv.face)
    assert np.array_equal(mask, nv.mask)
    assert np.array_equal(img.view(np.uint32), nv.img.view(np.uint32))
    if name.startswith("topo_"):
        _, faces, blank = mc.topology(name[5:])
        assert np.array_equal(nv.faces, faces) and (not blank or not mask.any())


def test_cases_do_what_they_claim(oracle_out):
    cov = lambda n: float(oracle_out[n][1].mean())
    assert cov("mirrored") > 0.5 and cov("magnified") > 0.9
    for n in mc.names("wild_") + mc.names("sheet_"):
        assert cov(n) > 0.2, n
    for n in mc.names("wild_"):
        c = mc.cases()[n]
        ndc = mc.ndc_verts(c)
        assert (ndc[:, 2] == 0).any() and (ndc[:, 2] < 0).any() and (~np.isfinite(ndc[:, :2])).any() and (ndc[:, 2] == np.float32(1e-30)).any()
    for n in mc.names("dyadic_"):  # every vertex of the dyadic cases is exact: float32 and float64 give the same NDC
        c = mc.cases()[n]
        K = c.cam[2:18].reshape(4, 4).astype(np.float64)
        s = min(c.H, c.W) / 2.0
        p = c.pcl.astype(np.float64)
        exact = np.stack([-(p[..., 0] * K[0, 0]) / s, -(p[..., 1] * K[1, 1]) / s, p[..., 2]], -1).reshape(-1, 3)
        assert np.array_equal(mc.ndc_verts(c).astype(np.float64), exact)


@pytest.mark.parametrize("name", [n for n in mc.names() if mc.cases()[n].expect is not None])
def test_constructed_cases_against_integer_arithmetic(name, oracle_out):
    """vertex / edge / diagonal holes, the lower id at equal depth, the kind bit in the order, the closed area band"""
    c = mc.cases()[name]
    img, mask, face = oracle_out[name]
    mc.check_expect(c, face, mask, img)
    nv = mc.naive(name)
    mc.check_expect(c, nv.face, nv.mask, nv.img)


# ---------------------------------------------------------------- precision
def test_float32_against_float64(oracle_out):
    """Winners: measured 0 differing pixels on every case but wild_40x24, which has 2 of 960 (0.21 %; both lie within
    1e-7 of a shared edge of the two faces, whose depths there differ by 6e-9 relative).  A differing pixel must be such
    a near-decision in float64 -- a smallest |barycentric| of one of the two faces below 1e-5, or a depth gap between
    them below 1e-6 relative -- and a case may have at most 0.5 % of them.
    Colours, where the winners agree: the float32 statement is within 1.94e-5 of float64 (RGB32_VS_64_MEASURED, the
    largest over all cases); the oracle, which runs the float32 arithmetic in the same order, must stay within 4 x that
    = 7.8e-5 (RGB_VS_F64_ATOL)."""
    worst, excluded = 0.0, {}
    for name, c in mc.cases().items():
        a, b = mc.naive(name), mc.naive(name, "f64")
        diff = np.argwhere(a.face != b.face)
        if diff.shape[0]:
            excluded[name] = diff.shape[0] / (c.H * c.W)
            ndc = mc.ndc_verts(c)
            for yi, xi in diff:
                tris = [r.faces[r.idx[yi, xi]] for r in (a, b) if r.idx[yi, xi] >= 0]
                at = [p3d.face_at_pixel(ndc, t, c.H, c.W, yi, xi) for t in tris]
                near_edge = min(m for m, _ in at) < 1e-5
                z_tie = len(at) == 2 and abs(at[0][1] - at[1][1]) < 1e-6 * max(abs(at[0][1]), abs(at[1][1]))
                assert near_edge or z_tie, (name, yi, xi, at)
        agree = a.face == b.face
        worst = max(worst, float(np.abs(a.img.astype(np.float64) - b.img)[agree].max(initial=0.0)))
        assert np.abs(oracle_out[name][0].astype(np.float64) - b.img)[agree].max(initial=0.0) <= RGB_VS_F64_ATOL, name
    print(f"mesh float32 vs float64: largest |rgb32 - rgb64| = {worst:.3e}; excluded pixel shares = {excluded}")
    assert all(v <= EXCLUDED_SHARE_CAP for v in excluded.values()), excluded
    assert worst <= RGB32_VS_64_MEASURED * 1.01  # the docstring's figure is the one this run gives


def test_backend_rounding_of_the_vertices_is_reported():
    """how many winners change when the vertex transform fuses its multiply-adds (pytorch3d's CUDA backend; "fma") -- a
    report, as for the points (test_p3d_second.py).  Asserted: the "seq" flavour gives the oracle's own vertices, so it changes no winner."""
    report = {}
    for name in [n for n in mc.names() if not n.startswith("topo_")]:
        c = mc.cases()[name]
        k = c.keep.reshape(-1) != 0
        # value for value, NaN for NaN (a zero's sign may differ: a vertex on the optical axis is -0 in the closed form)
        assert np.array_equal(mc.ndc_verts(c), orc.points_to_ndc(c.pcl.reshape(-1, 3)[k], c.cam, c.H, c.W), equal_nan=True)
        changed = int((mc.naive(name, "f32", "fma").face != mc.naive(name).face).sum())
        if changed:
            report[name] = changed
    print("mesh winners changed by the fma vertex flavour:", report or "none")
