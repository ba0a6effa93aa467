"""Cases for the mesh variant of the dynamic renderer (csrc/mesh.hip, ops.mesh_render, orc_mesh_render; render_dyn_mesh,
pgdvs_renderer_dyn.py:542-669 in the reference), the naive statement run over them (oracle/p3d_second.py) and, for the
constructed ones, the result worked out with integer arithmetic alone.

A case is (name, H, W, flat camera, keep[H,W], pcl[H,W,3], rgb[H,W,3], expect).  Face ids are the kernel's and the
oracle's: ``kind * H * W + source pixel``; ``face_ids_of_list`` maps the reference's explicit face list (vertex ranks)
onto them from the list's own geometry.

  topology   the keep masks of tests/golden/mesh_edges.npz (the reference's own face lists) over a noisy sheet.
  dyadic     identity pose, fx = fy = min(H,W)/2, centred principal point, depth 1: every vertex and every pixel centre
             is an exact float and point_to_ndc is exact.  The source grid is shifted by (dx, dy) pixels, so whether a
             centre lies on a vertex, on an edge, on the shared diagonal or strictly inside a face -- and inside which
             -- follows from the shift in eighths of a pixel (``_expect_grid``): strict ``bary > 0`` leaves a hole on
             every vertex, edge and diagonal, and the cell whose two faces touch vertex 0 is never drawn.
  tie        coincident sheets (the right half's vertices copied from the left half's: identical arithmetic, so
             identical z bits, and the lower id must win), two sheets at depths 2 and 1 with equal footprints (the
             nearer wins although its ids are higher), and a kind-1 face of a low pixel against the same triangle as
             the kind-0 face of a higher pixel (kind-0 ids are below every kind-1 id: the higher pixel must win).
  area       one 2 x 2 block and a lone first pixel; the block's vertices sit a few 2^-n around one pixel centre, which
             lies strictly inside the kind-0 face.  face_area = +-2^-2n against the closed +-1e-8 band: drawn for
             n <= 13, not for n >= 14.  ``area_edge``: face_area exactly float32(1e-8) (inside the closed band, not
             drawn) and one ulp above (drawn), both signs.
  shape      a sheet mirrored (every face clockwise) and one magnified 40 x (a few faces cover the image, vertices far
             outside it); sheets with noise 0, 0.3 and 2.0.
  wild       vertices in front of, on and behind the camera plane (5 % at z_view exactly 0: infinite or NaN NDC),
             3 % at x = 1e6, 2 % at z = 1e-30; 90 % of the pixels kept.  pytorch3d clips nothing here, so vertices behind
             the camera are part of the contract.  NaN / inf coordinates given directly in ``pcl`` are left out:
             their handling upstream cannot be read from anything available.

Test infrastructure only (tests/test_mesh_edges_host.py runs it without a GPU, tests/test_gpu_mesh_edges.py runs the
kernels over it): nothing here touches the GPU."""
import collections
import functools
import pathlib

import numpy as np

from oracle import p3d_second as p3d

F32 = np.float32
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
Case = collections.namedtuple("Case", "name H W cam keep pcl rgb expect")
Naive = collections.namedtuple("Naive", "face mask img z faces ids idx")

DYADIC_SIZES = ((16, 32), (32, 16), (16, 16))
DYADIC_SHIFTS = ((0, 0), (2, 2), (4, 4), (2, 4), (4, 2), (2, 1))  # (dx, dy) in eighths of a pixel
AREA_N = (12, 13, 14, 15)
WILD_SIZES = ((24, 40), (40, 24), (2, 512), (512, 2), (3, 300), (16, 16))
EPS_BITS = 0x322BCC77  # float32(1e-8) = 11258999 * 2^-50

# measured on the CPU over every case of mesh_cases.py, at the pixels where the float32 and float64 winners agree:
# the largest |rgb32 - rgb64| is 1.94e-5 (topo_all_a: sliver faces of the jittered sheet, whose barycentrics are
# quotients of small differences).  The oracle and the kernel run the float32 statement's arithmetic in its order;
# factor 4 -> 7.8e-5.
RGB32_VS_64_MEASURED = 1.94e-5
RGB_VS_F64_ATOL = 4 * RGB32_VS_64_MEASURED
EXCLUDED_SHARE_CAP = 0.005


# ---------------------------------------------------------------- cameras and clouds
def flat_cam(H, W, fx, fy, cx, cy, c2w=None):
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return np.concatenate(([H, W], K.flatten(), (np.eye(4) if c2w is None else np.asarray(c2w, np.float64)).flatten())).astype(F32)


def _dyadic_cam(H, W):
    s = min(H, W) / 2.0
    return flat_cam(H, W, s, s, W / 2.0, H / 2.0)


def _unproject(cam, u, v, z):
    """camera-space points of pixel coordinates (u, v) (a pixel's centre is at +0.5) at depth z -> world, float32"""
    K, c2w = cam[2:18].reshape(4, 4).astype(np.float64), cam[18:34].reshape(4, 4).astype(np.float64)
    pc = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z * np.ones_like(u)], -1)
    return (pc @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)


def _grid(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return xx + 0.5, yy + 0.5


def _pose(yaw_deg, pitch_deg, t):
    y, p = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    c2w = np.eye(4)
    c2w[:3, :3] = Ry @ Rx
    c2w[:3, 3] = t
    return c2w


def _sheet(H, W, seed, noise, mag=1.0, mirror=False):
    """a smooth depth sheet seen by a general camera a little off the source view, pixel positions jittered by ``noise``"""
    rng = np.random.default_rng(seed)
    src = flat_cam(H, W, 0.9 * W, 0.9 * W, W / 2.0, H / 2.0)
    tgt = flat_cam(H, W, 0.85 * W, 0.88 * W, W / 2.0 + 0.7, H / 2.0 - 0.4, _pose(2.0, -1.5, [0.03, -0.02, 0.05]))
    u, v = _grid(H, W)
    z = 2.0 + 0.5 * np.sin(u / W * 3) + 0.3 * np.cos(v / H * 2) + rng.normal(0, 1, (H, W)) * noise * 0.3
    u = (u - W / 2.0) * mag * (-1.0 if mirror else 1.0) + W / 2.0 + rng.normal(0, 1, (H, W)) * noise
    v = (v - H / 2.0) * mag + H / 2.0 + rng.normal(0, 1, (H, W)) * noise
    return tgt, _unproject(src, u, v, z), rng.random((H, W, 3), dtype=F32)


# ---------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN / "mesh_edges.npz"))


def topology_names():
    return [str(n) for n in fixture()["cases"]]


def topology(name):
    g = fixture()
    return g[name + "__keep"], g[name + "__faces"], bool(g[name + "__blank"])


# ---------------------------------------------------------------- face ids <-> the explicit list
def face_ids_of_list(keep, faces):
    """the (kind * P + source pixel) id of every row of ``faces`` (vertex ranks), from the row's own corners"""
    keep = np.asarray(keep) != 0
    H, W = keep.shape
    pix = np.flatnonzero(keep.reshape(-1))
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    q0, q1, q2 = pix[faces[:, 0]], pix[faces[:, 1]], pix[faces[:, 2]]
    kind0 = (q1 == q0 + W) & (q2 == q0 + W + 1)
    kind1 = (q1 == q0 + W + 1) & (q2 == q0 + 1)
    assert np.all(kind0 ^ kind1)
    return np.where(kind0, 0, H * W) + q0


def ranks_of_ids(keep, ids):
    """(kind, q0) -> the three vertex ranks, -1 for a corner that is not kept"""
    keep = np.asarray(keep) != 0
    H, W = keep.shape
    P = H * W
    rank = np.where(keep.reshape(-1), np.cumsum(keep.reshape(-1)) - 1, -1)
    ids = np.asarray(ids, np.int64)
    kind, q0 = ids // P, ids % P
    q1 = np.where(kind == 0, q0 + W, q0 + W + 1)
    q2 = np.where(kind == 0, q0 + W + 1, q0 + 1)
    return np.stack([rank[q0], rank[q1], rank[q2]], 1)


# ---------------------------------------------------------------- integer expectations
def _expect_grid(H, W, dx8, dy8, cols=None):
    """winner of every pixel for the unit grid shifted by (dx8, dy8) eighths of a pixel, every pixel kept: the centre of
    pixel (yi, xi) sits (8 xi - dx8, 8 yi - dy8) eighths from vertex (0, 0); on a vertex column, a vertex row or the
    diagonal (local x == local y) nothing is drawn; below the diagonal (local y > local x) face kind 0 of the cell,
    above it kind 1; the cell (0, 0) has both faces on vertex 0.  ``cols``: only cells whose left column is in it."""
    face = np.full((H, W), -1, np.int64)
    for yi in range(H):
        for xi in range(W):
            ax, ay = 8 * xi - dx8, 8 * yi - dy8
            c, lx, r, ly = ax // 8, ax % 8, ay // 8, ay % 8
            if lx == 0 or ly == 0 or lx == ly or not (0 <= c < W - 1 and 0 <= r < H - 1) or (r == 0 and c == 0):
                continue
            if cols is not None and c not in cols:
                continue
            face[yi, xi] = (0 if ly > lx else H * W) + r * W + c
    return face


def _inside_int(tri, H, W, unit):
    """pixel centres strictly inside the triangle ``tri`` = 3 x (u, v) in integer multiples of 1/unit pixel"""
    (ax, ay), (bx, by), (cx, cy) = tri
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx * unit + unit // 2, yy * unit + unit // 2
    e0 = (px - bx) * (cy - by) - (py - by) * (cx - bx)
    e1 = (px - cx) * (ay - cy) - (py - cy) * (ax - cx)
    e2 = (px - ax) * (by - ay) - (py - ay) * (bx - ax)
    return ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0))


# ---------------------------------------------------------------- constructed cases
def _rgb(H, W, seed):
    return np.random.default_rng(seed).random((H, W, 3), dtype=F32)


def _dyadic_pcl(H, W, dx8, dy8, depth=1.0):
    u, v = _grid(H, W)
    return _unproject(_dyadic_cam(H, W), u + dx8 / 8.0, v + dy8 / 8.0, depth)


def _dyadic_cases():
    out = []
    for H, W in DYADIC_SIZES:
        for dx8, dy8 in DYADIC_SHIFTS:
            face = _expect_grid(H, W, dx8, dy8)
            n = int((face >= 0).sum())
            assert n == (0 if dx8 == dy8 else (H - 1) * (W - 1) - 1)
            out.append(Case(f"dyadic_{H}x{W}_{dx8}_{dy8}", H, W, _dyadic_cam(H, W), np.ones((H, W), np.uint8),
                            _dyadic_pcl(H, W, dx8, dy8), _rgb(H, W, 11), {"face": face}))
    return out


def _tie_cases():
    H, W, P = 16, 32, 16 * 32
    cam, keep, rgb = _dyadic_cam(H, W), np.ones((H, W), np.uint8), _rgb(H, W, 12)
    out = []
    # the issue's pair: coincident sheets.  A left face and its copy run through identical arithmetic, so their z bits are
    # equal and the lower id (the left one) must win.  The seam cells (column 15 -> the copy of column 0) are stretched
    # faces at the same depth that cover the same 15 x 15 pixels; their z may differ from the sheets' in the last bit, so
    # which of a left face and a seam face wins is left open here -- both have their first corner in the left half.  The
    # left sheet's cell (0, 0) touches vertex 0: pixel (1, 1) goes to the seam's kind-1 face of row 0 (id P + 15), below
    # the copy's id P + 16.
    pcl = _dyadic_pcl(H, W, 2, 4)
    pcl[:, 16:] = pcl[:, :16]
    cov = np.zeros((H, W), bool)
    cov[1:16, 1:16] = True
    out.append(Case("tie_coincident", H, W, cam, keep, pcl, rgb, {"covered": cov, "q0_cols_below": 16}))
    # the same without the seam (column 15 not kept): every winner is known exactly -- the left sheet's face wherever
    # it has one, the copy's (higher id) only where the left sheet has none: cell (0, 0) and the left sheet's lost column 14
    k2 = keep.copy()
    k2[:, 15] = 0
    right = _expect_grid(H, W, 2, 4, cols=range(15))
    right = np.where(right >= 0, right + 16, -1)
    right[1, 1] = P + 16  # the copy's cell (0, 16) does not touch vertex 0
    l2 = _expect_grid(H, W, 2, 4, cols=range(14))
    out.append(Case("tie_coincident_noseam", H, W, cam, k2, pcl, rgb, {"face": np.where(l2 >= 0, l2, right)}))
    # depths 2 (left, low ids) and 1 (right, high ids), equal NDC footprints: the nearer sheet wins everywhere; the seam
    # faces run from depth 2 to depth 1 and stay behind depth 1 at every centre
    pcl = _dyadic_pcl(H, W, 2, 4, depth=2.0)
    pcl[:, 16:] = _dyadic_pcl(H, W, 2, 4, depth=1.0)[:, :16]
    near = _expect_grid(H, W, 2, 4, cols=range(15))
    near = np.where(near >= 0, near + 16, -1)
    near[1, 1] = P + 16
    out.append(Case("tie_depth_1_2", H, W, cam, keep, pcl, rgb, {"face": near}))
    # the key's kind bit: block A at (2..3, 2..3), magnified to 4 pixels; block B at (6..7, 6..7), whose kind-0 face is
    # the same vertex triple, in the same order, as A's kind-1 face (identical arithmetic: identical z bits).  B's
    # fourth vertex repeats its first, so B's kind-1 face has no area.  id(B, kind 0) = 6 W + 6 < P + 2 W + 2 = id(A, kind 1).
    keep = np.zeros((H, W), np.uint8)
    keep[0, 0] = 1
    keep[2:4, 2:4] = 1
    keep[6:8, 6:8] = 1
    pos = {(2, 2): (34, 36), (3, 2): (34, 68), (3, 3): (66, 68), (2, 3): (66, 36)}  # (u, v) in eighths of a pixel
    pos.update({(6, 6): pos[(2, 2)], (7, 6): pos[(3, 3)], (7, 7): pos[(2, 3)], (6, 7): pos[(2, 2)]})
    u, v = _grid(H, W)
    for (r, c), (pu, pv) in pos.items():
        u[r, c], v[r, c] = pu / 8.0, pv / 8.0
    pcl = _unproject(cam, u, v, 1.0)
    face = np.full((H, W), -1, np.int64)
    face[_inside_int((pos[(2, 2)], pos[(3, 2)], pos[(3, 3)]), H, W, 8)] = 2 * W + 2  # A, kind 0
    up = _inside_int((pos[(2, 2)], pos[(3, 3)], pos[(2, 3)]), H, W, 8)
    assert up.sum() >= 3 and (face >= 0).sum() >= 3
    face[up] = 6 * W + 6  # B's kind 0 beats A's kind 1
    out.append(Case("tie_kind_bit", H, W, cam, keep, pcl, _rgb(H, W, 13), {"face": face}))
    return out


def _block_case(name, H, W, centre, x_off, y_off, drawn):
    """lone first pixel (0, 0) and the block (2..3, 2..3) with NDC corners (x_off[j], y_off[i]) for block row i, column j;
    identity pose, depth 1 and fxn = fyn = 1, so a vertex's NDC position is minus its camera-space position, exactly"""
    keep = np.zeros((H, W), np.uint8)
    keep[0, 0] = 1
    keep[2:4, 2:4] = 1
    u, v = _grid(H, W)
    pcl = _unproject(_dyadic_cam(H, W), u, v, 1.0)
    for i in range(2):
        for j in range(2):
            pcl[2 + i, 2 + j] = (-F32(x_off[j]), -F32(y_off[i]), 1.0)
    face = np.full((H, W), -1, np.int64)
    if drawn:
        face[centre] = 2 * W + 2
    return Case(name, H, W, _dyadic_cam(H, W), keep, pcl, _rgb(H, W, 14), {"face": face})


def _area_cases():
    out = []
    for n in AREA_N:
        for mirror in (False, True):
            # 16 x 16: pixel (7, 7) has its centre at NDC (1/16, 1/16).  Legs L = 2^-n; the centre lies a quarter of a leg
            # from the block's first column and half a leg from its first row: strictly inside the kind-0 face.
            L, c = 2.0 ** -n, 1.0 / 16
            sx = -1.0 if mirror else 1.0
            x_off = (c + sx * L / 4, c + sx * (L / 4 - L))
            y_off = (c + L / 2, c + L / 2 - L)
            assert all(float(F32(t)) == t for t in x_off + y_off)
            out.append(_block_case(f"area_n{n}_{'neg' if mirror else 'pos'}", 16, 16, (7, 7), x_off, y_off, drawn=n <= 13))
    # 17 x 17: the centre of pixel (8, 8) is NDC (0, 0) exactly.  Legs 2^-13 (x) and m * 2^-37 (y) with m the mantissa of
    # float32(1e-8) = m * 2^-50, or m + 1: face_area is the band's edge exactly, or one ulp outside it
    m = (EPS_BITS & 0x7FFFFF) | 0x800000
    assert float(np.array(EPS_BITS, np.uint32).view(F32)) == m * 2.0 ** -50 == float(F32(1e-8))
    for tag, mm, drawn in (("eq", m, False), ("above", m + 1, True)):
        for mirror in (False, True):
            sx = -1.0 if mirror else 1.0
            Lx = 2.0 ** -13
            x_off = (sx * Lx / 4, sx * (Lx / 4 - Lx))
            y_off = ((mm - 2 ** 22) * 2.0 ** -37, -(2.0 ** -15))
            assert all(float(F32(t)) == t for t in x_off + y_off) and float(F32(y_off[0]) - F32(y_off[1])) == mm * 2.0 ** -37
            out.append(_block_case(f"area_edge_{tag}_{'neg' if mirror else 'pos'}", 17, 17, (8, 8), x_off, y_off, drawn))
    return out


def _shape_cases():
    out = []
    for name, (H, W), seed, kw in (("sheet_n0", (24, 40), 21, dict(noise=0.0)), ("sheet_n03", (40, 24), 22, dict(noise=0.3)),
                                   ("sheet_n2", (32, 32), 23, dict(noise=2.0)), ("mirrored", (24, 40), 24, dict(noise=0.1, mirror=True)),
                                   ("magnified", (24, 40), 25, dict(noise=0.1, mag=40.0))):
        cam, pcl, rgb = _sheet(H, W, seed, **kw)
        keep = np.random.default_rng(seed + 100).random((H, W)) < 0.9
        out.append(Case(name, H, W, cam, keep.astype(np.uint8), pcl, rgb, None))
    return out


def _wild_cases():
    out = []
    for i, (H, W) in enumerate(WILD_SIZES):
        rng = np.random.default_rng(300 + i)
        c2w = np.eye(4)
        c2w[:3, 3] = [0.25, -0.125, 0.0]  # no rotation and no z translation: z_view is the world z, exactly
        cam = flat_cam(H, W, 0.8 * max(H, W), 0.9 * max(H, W), W / 2.0 + 1.3, H / 2.0 - 0.6, c2w)
        u, v = _grid(H, W)
        z = rng.uniform(-2.0, 4.0, (H, W))
        pcl = _unproject(cam, u + rng.normal(0, 1.5, (H, W)), v + rng.normal(0, 1.5, (H, W)), z)
        sel = rng.random((H, W))
        pcl[sel < 0.05, 2] = 0.0
        pcl[(sel >= 0.05) & (sel < 0.08), 0] = 1e6
        pcl[(sel >= 0.08) & (sel < 0.10), 2] = 1e-30
        keep = rng.random((H, W)) < 0.9
        out.append(Case(f"wild_{H}x{W}", H, W, cam, keep.astype(np.uint8), pcl, rng.random((H, W, 3), dtype=F32), None))
    return out


def _topology_cases():
    out = []
    for i, name in enumerate(topology_names()):
        keep, _, _ = topology(name)
        H, W = keep.shape
        cam, pcl, rgb = _sheet(H, W, 500 + i, noise=0.2)
        out.append(Case("topo_" + name, H, W, cam, keep, pcl, rgb, None))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    cs = _dyadic_cases() + _tie_cases() + _area_cases() + _shape_cases() + _wild_cases() + _topology_cases()
    for c in cs:
        for a in (c.cam, c.keep, c.pcl, c.rgb):
            a.setflags(write=False)
    return collections.OrderedDict((c.name, c) for c in cs)


def names(prefix=""):
    return [n for n in cases() if n.startswith(prefix)]


# ---------------------------------------------------------------- the naive statement over a case
def ndc_verts(case, flavour="seq"):
    k = case.keep.reshape(-1) != 0
    with np.errstate(all="ignore"):  # vertices on the camera plane divide by zero, on purpose
        return p3d.points_to_ndc(case.cam, case.pcl.reshape(-1, 3)[k], flavour=flavour, inverse="f64")


@functools.lru_cache(maxsize=None)
def naive(name, dtype="f32", flavour="seq"):
    """the naive statement on a case (computed once per process): winners as face ids, mask, image, z"""
    c = cases()[name]
    dt = np.float32 if dtype == "f32" else np.float64
    faces = p3d.mesh_faces_from_keep(c.keep)
    ids = face_ids_of_list(c.keep, faces)
    k = c.keep.reshape(-1) != 0
    if faces.shape[0] == 0:  # the reference's blank branch: no mesh is built
        z = np.zeros((c.H, c.W), dt)
        return Naive(np.full((c.H, c.W), -1, np.int64), np.zeros((c.H, c.W), F32), np.zeros((c.H, c.W, 3), dt), z, faces, ids, None)
    img, mask, idx, z = p3d.render_mesh(ndc_verts(c, flavour), faces, c.rgb.reshape(-1, 3)[k], c.H, c.W, dt)
    face = np.where(idx >= 0, ids[np.maximum(idx, 0)], -1)
    for a in (face, mask, img, z):
        a.setflags(write=False)
    return Naive(face, mask, img, z, faces, ids, idx)


def check_expect(case, face, mask, img):
    """the integer-arithmetic expectation of a constructed case against a result: face[H,W] ids, mask[H,W], img[H,W,3]"""
    e = case.expect
    face = np.asarray(face).astype(np.int64)
    P = case.H * case.W
    if "face" in e:
        assert np.array_equal(face, e["face"]), (case.name, np.argwhere(face != e["face"])[:8])
        cov = e["face"] >= 0
    else:
        cov = e["covered"]
        assert np.array_equal(face >= 0, cov), case.name
        assert np.all((face[cov] % P) % case.W < e["q0_cols_below"]), case.name
    assert np.array_equal(np.asarray(mask) != 0, cov) and set(np.unique(mask)) <= {0.0, 1.0}, case.name
    assert np.all(np.asarray(img)[~cov] == 0.0), case.name  # a hole is mask 0 and colour exactly 0
