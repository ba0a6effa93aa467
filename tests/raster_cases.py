"""Cases for the point rasteriser and compositor (csrc/raster.hip, ops.points_raster; pytorch3d's PointsRasterizer with
bin_size = 0 and NormWeightedCompositor as StaticGeoPointRenderer.forward drives them, st_geo_renderer.py:77-120 in the
reference) at the inputs on which the kernel takes its own decisions, and the two CPU statements run over them
(oracle/pgdvs_oracle.c: pixel-major C loop; oracle/p3d_second.py: pytorch3d's object chain and priority queue).

A case is (name, H, W, flat camera, pts[n,3], feat[n,3], radius, K, claims).  ``claims`` says what the host test must
find in the oracle's result, so that a case cannot silently stop exercising its edge.  Cameras are built as in
tests/test_gpu_parity.py (synth.flat_cam).  The "dyadic" camera is that of tests/mesh_cases.py: identity pose,
fx = fy = min(H, W) / 2, centred principal point, so fxn = fyn = 1 and p0 = -0: at z = 1 a point's NDC position is minus
its world position, exactly; pixel centres are exact floats where H and W are powers of two (64 x 64), and rounded
quotients elsewhere (17 x 15, 33 x 47) -- which is why the grazing positions are searched, not written down.

  degenerate  300 ordinary points with the rows of ``SPECIAL`` spliced in at the first, the middle and the last indices:
              z_view = +0, -0, 1.4e-45, 1e-30, 3e38, +inf, -1, -inf (on the optical axis, and with x = 0.3, y = -0.2), NaN
              in each coordinate alone, +-inf in x, x = y = 3e38, and (1e30, 0, 1e30).  Dyadic camera (64 x 64: 16
              tiles, the direct binning pass's segments exist) and a rotated one (40 x 56), under which one non-finite
              world coordinate makes all three view coordinates non-finite.  With the dyadic camera the drawn rows follow
              from IEEE arithmetic: on the axis x_ndc = -0 / z is a zero for every z > 0 -- the subnormal 1.4e-45
              included -- and NaN for z = +-0 and +inf (0 x inf); off the axis 0.3 / 1.4e-45 overflows, 0.3 / 1e-30 =
              3e29 is finite and far outside, 0.3 / 3e38 is a subnormal at the centre; (1e30, 0, 1e30) lands on x_ndc = -1
              exactly, half a pixel beyond the last column's centres.  ``*_behind``: every undrawn special row replaced by
              a point behind the camera -- the fragments must not change.  ``degen_dense``: 1700 points at z in [1, 3]
              around the centre of an 80 x 128 image plus the rows at z = 1e-30 and z = 3e38: the sorted path's 1024
              buckets span the bit patterns of 1e-30 .. 3e38, the cluster falls into seven of them, far more than 64
              entries share a bucket, and the tile (list <= 2048) goes to the general path.
  grazing     for each target pixel -- the image corners, the centre, both sides of the tile borders (rows and columns
              15 | 16, 31 | 32, 47 | 48, over four ``phases`` every one of (15, 15), (15, 16), (16, 15), (16, 16)), the
              last row and column of a partial tile -- one direction, across the tile border where there is one (the
              point's own centre then lies in the neighbouring tile; at two corners outside the image), and along it at
              z = 1: the last float32 world position whose disc still covers the pixel centre (d2 < r2), the first with
              d2 >= r2, and where that one has d2 == r2 the first with d2 > r2.  The walk evaluates the oracle's own
              arithmetic (orc.points_to_ndc, dx dx + dy dy in float32).  Targets are at least 2 r + 1 pixels apart, so
              no other disc reaches a target: in the ``lone`` cases the grazing fragment is the pixel's only one, its
              weight 1 - d2 / r2 is a few 1e-6, and the compositor's clamp t = max(sum w, 1e-4) scales the colour down
              while the mask stays 1.  ``layer``: a centre hit (d2 = 0) at z = 2 on every target and 300 ordinary points
              at z = 4 behind; K = 1 keeps the grazing fragment alone, K = 3 puts it first.  d2 == r2 exactly exists
              along an axis wherever pixel centre +- radius is a float32 (a dyadic radius: at z = 1 the NDC position is
              the negated world coordinate, so dx = r exactly), and at 64 x 64 with radius 5/64 along a 3-4-5 direction.
  thresholds  layered random clouds (depths from six layers, 70 % jittered: exact depth ties across indices; two points
              in every pixel of one tile so that the depth bound is finite there) at radii one float32 step below and at:
              rpx = radius min(H, W) / 2 = 2.25 and 5.05 (block size of the depth bound), 2 (rpx' + 0.0625) + 2 = 16 (the
              tile_box_within_2x2 switch, rpx' = radius W / range_x in float32), rpx = 0.5 and sqrt(1/2) (discs that reach
              no pixel centre, one, or two).  K = 1..8 where rpx >= 5.05, 4 and 5 where 2.25 <= rpx < 5.05 (K <= b b on
              and off), 1 and 3 below.  Every threshold at every size: 64 x 64 (16 tiles: segments), 48 x 64 (12: none), 16 x 16, 15 x 17.
  shapes      1 x 1, 1 x 300, 300 x 1, 2 x 2, 4 x 2048, 2048 x 4, 4 x 8192; rpx 0.75 .. 2; points over and beyond the
              image, every twelfth at a distance of the radius (to float32 rounding) from a pixel centre: with
              range_x = 2 W / H the rounding of pix_to_ndc grows with the aspect ratio, and tile_box's 0.0625 px margin
              has to cover it.

Left out: nothing that the two statements disagree on was found -- on every case they agree bit for bit in idx, zbuf and
dist2 (the NDC of UNDRAWN rows differs in NaN payload and in NaN-versus-inf of z, so NDC equality is asserted on drawn
rows only, and there value for value: a zero's sign differs on the optical axis).  The kNN grid's handling of non-finite
rows is another subject.

Test infrastructure only (tests/test_raster_edges_host.py runs it without a GPU, tests/test_gpu_raster_edges.py runs the
kernels over it): nothing here touches the GPU."""
import collections
import functools

import numpy as np

from oracle import oracle as orc
from oracle import p3d_second as p3d
from pgdvs_amd import synth

F32 = np.float32
Case = collections.namedtuple("Case", "name H W cam pts feat radius K claims")

# measured on the CPU over the thresholds and shapes families, at the pixels whose every weight is >= 2^-10: the largest
# |orc.composite - float64 compositor on the same idx and float32 d2| is 6.03e-7 (thr_box_below_64x64_K2: a few float32
# roundings per fragment on values <= 1); factor 4 -> 2.4e-6.  A weight 1 - d2 / r2 carries the absolute rounding 2^-25 of
# the quotient: 3e-5 of a weight of 2^-10, several per cent of a grazing one -- the reference's conditioning, left out
# here and met head-on by the grazing family.  A fragment falls below 2^-10 with probability ~2^-10, at most 8 per pixel:
# the largest share of covered pixels left out is 1.2 % (thr_b4_below_16x16_K5), pooled over a family 0.40 % (thresholds)
# and 0.73 % (shapes), against the cap of 2 %.
COMPOSITE32_VS_64_MEASURED = 6.03e-7
COMPOSITE_VS_F64_ATOL = 4 * COMPOSITE32_VS_64_MEASURED
W_MIN_F64 = 2.0 ** -10
EXCLUDED_SHARE_CAP = 0.02

SPECIAL_Z = (("p0", 0.0), ("m0", -0.0), ("den", 1.4e-45), ("1e-30", 1e-30), ("3e38", 3e38), ("pinf", np.inf), ("m1", -1.0),
             ("minf", -np.inf))
SPECIAL = tuple([(f"z{n}_axis", (0.0, 0.0, z)) for n, z in SPECIAL_Z] + [(f"z{n}_off", (0.3, -0.2, z)) for n, z in SPECIAL_Z]
                + [("nan_x", (np.nan, 0.1, 2.0)), ("nan_y", (0.1, np.nan, 2.0)), ("nan_z", (0.1, 0.1, np.nan)),
                   ("x_pinf", (np.inf, 0.0, 2.0)), ("x_minf", (-np.inf, 0.0, 2.0)), ("xy_3e38", (3e38, 3e38, 2.0)),
                   ("far_diag", (1e30, 0.0, 1e30))])
# dyadic camera: see the docstring
DRAWN_DYADIC = ("zden_axis", "z1e-30_axis", "z3e38_axis", "z3e38_off", "far_diag")
# rotated camera (world rows as given; the camera stands 2.5 behind the world origin and looks along the world z axis to
# within a degree): the rows near the origin, (0.3, -0.2, -1) included, are ordinary points in front of it; the rows at
# z = 3e38 keep finite view coordinates (|R| <= 1) whose quotient is the direction of the world z axis, near the centre;
# every row with a non-finite coordinate is non-finite throughout; x = y = 3e38 and x = 1e30 land far outside
DRAWN_ROTATED = ("zp0_axis", "zm0_axis", "zden_axis", "z1e-30_axis", "z3e38_axis", "zm1_axis", "zp0_off", "zm0_off", "zden_off",
                 "z1e-30_off", "z3e38_off", "zm1_off")

GRAZE_GEOMS = (("64x64_r5", 64, 64, 5.0 / 64), ("64x64_r4", 64, 64, 1.0 / 16), ("17x15", 17, 15, 1.0 / 4), ("33x47", 33, 47, 1.0 / 8))
THRESH_SIZES = ((64, 64), (48, 64), (16, 16), (15, 17))
SHAPE_SIZES = (((1, 1), 0.75, 40), ((1, 300), 1.0, 300), ((300, 1), 1.25, 300), ((2, 2), 2.0, 60), ((4, 2048), 1.5, 200),
               ((2048, 4), 1.5, 2000), ((4, 8192), 1.75, 3000))
WINDOWS_4x8192 = (0, 2040, 4090, 6143, 8192 - 64)  # column windows of 64 checked with the pixel-major loop


# ---------------------------------------------------------------- cameras, pixel centres, coverage
def dyadic_cam(H, W):
    s = min(H, W) / 2.0
    return synth.flat_cam(H, W, np.array([[s, 0, W / 2.0], [0, s, H / 2.0], [0, 0, 1.0]]), np.eye(4))


def rotated_cam(H, W):
    K3, c2w = synth.frame_camera(1, 4, H, W)
    c2w = np.array(c2w, np.float64)
    c2w[:3, 3] += c2w[:3, :3] @ np.array([0.0, 0.0, -2.5])  # step back: the world origin is 2.5 in front
    return synth.flat_cam(H, W, K3, c2w)


def pixel_centres(H, W):
    """(xf[W], yf[H]): NDC of the pixel centres as both statements compute them (PixToNonSquareNdc, reversed index)"""
    xf = np.array([p3d.pix_to_non_square_ndc(W - 1 - xi, W, H) for xi in range(W)], F32)
    yf = np.array([p3d.pix_to_non_square_ndc(H - 1 - yi, H, W) for yi in range(H)], F32)
    return xf, yf


def ndc_of(case_or_cam, pts=None, H=None, W=None):
    if pts is None:
        c = case_or_cam
        return orc.points_to_ndc(c.pts, c.cam, c.H, c.W)
    return orc.points_to_ndc(pts, case_or_cam, H, W)


def d2_f32(ndc, xf, yf):
    """dist2 of rows ndc[m,3] to every pixel centre, in the statements' float32 order: [m, H, W]"""
    with np.errstate(all="ignore"):
        dx = (ndc[:, 0, None] - xf[None, :]).astype(F32)
        dy = (ndc[:, 1, None] - yf[None, :]).astype(F32)
        return ((dx * dx).astype(F32)[:, None, :] + (dy * dy).astype(F32)[:, :, None]).astype(F32)


def rows_drawn(ndc, H, W, radius, rows):
    """which of ``rows`` pass the naive loop's two tests (not z < 0; d2 < r2) at one pixel or more"""
    xf, yf = pixel_centres(H, W)
    r2 = F32(F32(radius) * F32(radius))
    sub = ndc[np.asarray(rows, np.int64)]
    with np.errstate(all="ignore"):
        return (~(sub[:, 2] < 0)) & (d2_f32(sub, xf, yf) < r2).any((1, 2))


def _world(cam, u, v, z):
    """view-space points at pixel coordinates (u, v) (a pixel's centre is at +0.5) and depth z -> world, float32"""
    K, c2w = cam[2:18].reshape(4, 4).astype(np.float64), cam[18:34].reshape(4, 4).astype(np.float64)
    pc = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z * np.ones_like(u)], -1)
    return (pc @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)


# ---------------------------------------------------------------- degenerate
def _splice(bg, special):
    """the special rows in three groups at the first, the middle and the last indices -> (pts, {name: row})"""
    n3 = len(special) // 3
    groups = (special[:n3], special[n3:2 * n3], special[2 * n3:])
    half = bg.shape[0] // 2
    parts = [np.array([p for _, p in groups[0]], F32), bg[:half], np.array([p for _, p in groups[1]], F32), bg[half:],
             np.array([p for _, p in groups[2]], F32)]
    starts = np.cumsum([0] + [p.shape[0] for p in parts])
    where = {}
    for g, s in zip(groups, (starts[0], starts[2], starts[4])):
        for i, (name, _) in enumerate(g):
            where[name] = int(s + i)
    return np.concatenate(parts, 0), where


def _background(cam, H, W, n, rng, zs=(1.0, 3.0)):
    u, v = rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)
    z = np.round(rng.uniform(zs[0], zs[1], n), 1)  # coarse depths: exact ties broken by index
    return _world(cam, u, v, z)


def _degenerate_cases():
    out = []
    for tag, (H, W), cam_of, drawn in (("dyadic", (64, 64), dyadic_cam, DRAWN_DYADIC),
                                       ("rotated", (40, 56), rotated_cam, DRAWN_ROTATED)):
        rng = np.random.default_rng(7100 + H)
        cam = cam_of(H, W)
        pts, where = _splice(_background(cam, H, W, 300, rng), list(SPECIAL))
        feat = rng.random((pts.shape[0], 3), dtype=F32)
        radius, K = 0.05, 3
        claims = {"special": where, "drawn": drawn}
        out.append(Case(f"degen_{tag}", H, W, cam, pts, feat, radius, K, claims))
        with np.errstate(all="ignore"):
            drawn_now = rows_drawn(ndc_of(cam, pts, H, W), H, W, radius, list(where.values()))
        undrawn = [r for r, d in zip(where.values(), drawn_now) if not d]
        behind = pts.copy()
        c2w = cam[18:34].reshape(4, 4).astype(np.float64)
        behind[undrawn] = (c2w[:3, :3] @ np.array([0.0, 0.0, -1.0]) + c2w[:3, 3]).astype(F32)
        out.append(Case(f"degen_{tag}_behind", H, W, cam, behind, feat, radius, K,
                        {"same_as": f"degen_{tag}", "replaced": undrawn}))
    # the dense variant
    H, W = 80, 128
    rng = np.random.default_rng(7200)
    cam = dyadic_cam(H, W)
    n = 1700
    dense = _world(cam, W / 2.0 + rng.uniform(-4, 4, n), H / 2.0 + rng.uniform(-4, 4, n), rng.uniform(1.0, 3.0, n))
    extremes = [("z1e-30_axis", (0.0, 0.0, 1e-30)), ("z3e38_axis", (0.0, 0.0, 3e38)), ("zden_axis", (0.0, 0.0, 1.4e-45))]
    pts, where = _splice(np.concatenate([dense, _background(cam, H, W, 200, rng)], 0), extremes)
    out.append(Case("degen_dense", H, W, cam, pts, rng.random((pts.shape[0], 3), dtype=F32), 0.05, 3,
                    {"special": where, "drawn": tuple(n for n, _ in extremes)}))
    return out


def tile_lists(case):
    """per tile, the rows whose disc covers a pixel centre of the tile (what any correct binning must at least hold)"""
    ndc = ndc_of(case)
    xf, yf = pixel_centres(case.H, case.W)
    r2 = F32(F32(case.radius) * F32(case.radius))
    lists = collections.defaultdict(list)
    with np.errstate(all="ignore"):
        for lo in range(0, ndc.shape[0], 256):
            hit = (d2_f32(ndc[lo:lo + 256], xf, yf) < r2) & ~(ndc[lo:lo + 256, 2] < 0)[:, None, None]
            for m, yi, xi in zip(*np.nonzero(hit)):
                lists[(yi // 16, xi // 16)].append(lo + m)
    return {t: np.unique(v) for t, v in lists.items()}, ndc


# ---------------------------------------------------------------- grazing
def _neighbours(v, steps):
    a = np.empty(2 * steps + 1, F32)
    a[steps] = v
    for i in range(1, steps + 1):
        a[steps + i] = np.nextafter(a[steps + i - 1], F32(np.inf))
        a[steps - i] = np.nextafter(a[steps - i + 1], F32(-np.inf))
    return a


def _walk(cam, H, W, xf_t, yf_t, r2, base, axis, sign, steps=256):
    """float32 neighbours of world coordinate ``axis`` of ``base``, ordered outwards (``sign``): the last with d2 < r2 to
    the pixel centre (xf_t, yf_t), the first with d2 >= r2, the first with d2 > r2 -- as rows, with their d2"""
    pts = np.tile(np.asarray(base, F32), (2 * steps + 1, 1))
    pts[:, axis] = _neighbours(F32(base[axis]), steps)[::sign]
    ndc = orc.points_to_ndc(pts, cam, H, W)
    dx, dy = (ndc[:, 0] - xf_t).astype(F32), (ndc[:, 1] - yf_t).astype(F32)
    d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
    assert np.all(np.diff(d2) >= 0) and d2[0] < r2 < d2[-1], "the walk does not bracket the disc edge"
    i_ge = int(np.argmax(d2 >= r2))
    i_gt = int(np.argmax(d2 > r2))
    return (pts[i_ge - 1], d2[i_ge - 1]), (pts[i_ge], d2[i_ge]), (pts[i_gt], d2[i_gt])


def _graze_targets(H, W, phase, sep):
    """[((yi, xi), (dx, dy))] -- direction in pixel units (x right, y down), unit length; at least ``sep`` pixels apart"""
    d345, cand = (3.0 / 5, 4.0 / 5), []
    cand += [((0, 0), (-1.0, 0.0)), ((0, W - 1), (0.0, -1.0)), ((H - 1, 0), (1.0, 0.0)), ((H - 1, W - 1), (-d345[0], -d345[1])),
             ((H // 2, W // 2), d345)]
    rows = [(16 * k - 1 + ((k + phase) & 1), k) for k in range(1, (H - 1) // 16 + 1)]
    cols = [(16 * m - 1 + ((m + (phase >> 1)) & 1), m) for m in range(1, (W - 1) // 16 + 1)]
    ydir = lambda yi: (0.0, 1.0 if yi % 16 == 15 else -1.0)   # across the border, into the neighbouring tile
    xdir = lambda xi: (1.0 if xi % 16 == 15 else -1.0, 0.0)
    for yi, k in rows:
        for xi, m in cols:
            if yi < H and xi < W:
                cand.append(((yi, xi), xdir(xi) if (k + m) & 1 else ydir(yi)))
    for yi, _ in rows:
        cand += [((yi, x), ydir(yi)) for x in (W // 4, (3 * W) // 4, W // 2) if yi < H]
    for xi, _ in cols:
        cand += [((y, xi), xdir(xi)) for y in (H // 4, (3 * H) // 4, H // 2) if xi < W]
    cand += [((H - 1, W // 2), (d345[1], -d345[0])), ((H // 2, W - 1), (1.0, 0.0)), ((0, W // 2), (0.0, 1.0)),
             ((H // 2, 0), (0.0, 1.0))]
    kept = []
    for (yi, xi), d in cand:
        if all((yi - y) ** 2 + (xi - x) ** 2 >= sep * sep for (y, x), _ in kept):
            kept.append(((yi, xi), d))
    return kept


def _grazing_cases():
    out = []
    for gi, (tag, H, W, radius) in enumerate(GRAZE_GEOMS):
        cam = dyadic_cam(H, W)
        s = min(H, W) / 2.0
        xf, yf = pixel_centres(H, W)
        r2 = F32(F32(radius) * F32(radius))
        rpx = radius * s
        for li, layered in enumerate((False, True)):
            phase = (2 * gi + li) % 4
            rows, graze = [], []  # graze: (row, yi, xi, kind)
            targets = _graze_targets(H, W, phase, 2 * rpx + 1.0)
            for (yi, xi), (dx, dy) in targets:
                base = _world(cam, np.float64(xi + 0.5 + rpx * dx), np.float64(yi + 0.5 + rpx * dy), 1.0)
                axis = 1 if dx == 0 else 0  # (a 3-4-5 direction: y fixed, x walked)
                sign = 1 if (dx if axis == 0 else dy) > 0 else -1
                last_in, first_ge, first_gt = _walk(cam, H, W, xf[xi], yf[yi], r2, base, axis, sign)
                found = [(last_in, "in"), (first_ge, "eq" if first_ge[1] == r2 else "gt")] + ([(first_gt, "gt")] if first_ge[1] == r2 else [])
                for (row, _), kind in found:
                    graze.append((len(rows), yi, xi, kind))
                    rows.append(row)
            rng = np.random.default_rng(7300 + 10 * gi + li)
            pts = np.array(rows, F32)
            if layered:
                # (z = 2, world = -2 x the centre's NDC: the NDC position is the pixel centre, exactly)
                on = np.array([(-2.0 * float(xf[xi]), -2.0 * float(yf[yi]), 2.0) for (yi, xi), _ in targets], F32)
                graze += [(pts.shape[0] + i, yi, xi, "on") for i, ((yi, xi), _) in enumerate(targets)]
                far = _world(cam, rng.uniform(-2, W + 2, 300), rng.uniform(-2, H + 2, 300), 4.0)
                pts = np.concatenate([pts, on, far], 0)
            feat = rng.random((pts.shape[0], 3), dtype=F32) * F32(0.5) + F32(0.5)  # away from 0: a scaled colour is visible
            n_eq = sum(1 for g in graze if g[3] == "eq")
            for K in (1, 3):
                claims = {"graze": tuple(graze), "targets": tuple(t for t, _ in targets), "layered": layered, "cloud": f"graze_{tag}_{li}",
                          "lone_min": 8 if (not layered or K == 1) else 0, "front_min": 8,
                          "exact_min": 4, "exact_found": n_eq}
                out.append(Case(f"graze_{tag}_{'layer' if layered else 'lone'}_K{K}", H, W, cam, pts, feat, radius, K, claims))
    return out


# ---------------------------------------------------------------- thresholds
def _f32_from_bits(b):
    return np.array(b, np.uint32).view(F32)[()]


def smallest_radius(pred):
    """the smallest positive float32 radius with ``pred`` true (pred monotone), by bisection on the bit pattern"""
    lo, hi = int(F32(1e-6).view(np.uint32)), int(F32(64.0).view(np.uint32))
    assert not pred(_f32_from_bits(lo)) and pred(_f32_from_bits(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(_f32_from_bits(mid)):
            hi = mid
        else:
            lo = mid
    return _f32_from_bits(hi), _f32_from_bits(lo)


def host_rpx(radius, H, W):
    """rpx as points_raster_impl computes it (float32): the depth bound's block size switches on it"""
    return F32(F32(radius) * F32(F32(min(H, W)) / F32(2.0)))


def box_within_2x2(radius, H, W):
    """tile_box_within_2x2 in its float32 arithmetic"""
    rx = F32(2.0) * F32(W) / F32(H) if W > H else F32(2.0)
    ry = F32(2.0) * F32(H) / F32(W) if H > W else F32(2.0)
    rpx = F32(F32(F32(radius) * F32(W)) / rx) + F32(0.0625)
    rpy = F32(F32(F32(radius) * F32(H)) / ry) + F32(0.0625)
    return bool(F32(F32(2.0) * rpx + F32(2.0)) < F32(16.0) and F32(F32(2.0) * rpy + F32(2.0)) < F32(16.0))


def depth_bound_block(radius, H, W):
    rpx = host_rpx(radius, H, W)
    return 4 if rpx >= F32(5.05) else (2 if rpx >= F32(2.25) else 0)


THRESHOLDS = {
    "b2": lambda H, W: (lambda r: host_rpx(r, H, W) >= F32(2.25)),
    "b4": lambda H, W: (lambda r: host_rpx(r, H, W) >= F32(5.05)),
    "box": lambda H, W: (lambda r: not box_within_2x2(r, H, W)),
    "c05": lambda H, W: (lambda r: float(r) * (min(H, W) / 2.0) >= 0.5),
    "c07": lambda H, W: (lambda r: float(r) * (min(H, W) / 2.0) >= np.sqrt(0.5)),
}


def bound_tile(H, W):
    """the tile of the threshold clouds that holds the dense cluster (the only tile of the small images)"""
    return (1, 1) if H * W > 1024 else (0, 0)


def _layered_cloud(H, W, seed):
    rng = np.random.default_rng(seed)
    # the dense tile (``bound_tile``): two points inside every pixel's cell, so that every b x b block of it holds b b points'
    # nearest pixels -- the depth bound is finite there for every K <= b b
    n_all, m = (260, 8) if H * W > 1024 else (400, 4)
    cam = synth.flat_cam(H, W, np.array([[0.8 * H, 0, W / 2.0], [0, 0.8 * H, H / 2.0], [0, 0, 1.0]]), np.eye(4))
    ty, tx = bound_tile(H, W)
    yy, xx = np.mgrid[16 * ty:min(16 * ty + 16, H), 16 * tx:min(16 * tx + 16, W)]
    n_tile = 2 * yy.size
    u = np.concatenate([rng.uniform(-m, W + m, n_all), np.tile(xx.reshape(-1), 2) + 0.5 + rng.uniform(-0.4, 0.4, n_tile)])
    v = np.concatenate([rng.uniform(-m, H + m, n_all), np.tile(yy.reshape(-1), 2) + 0.5 + rng.uniform(-0.4, 0.4, n_tile)])
    n = n_all + n_tile
    z = rng.choice([1.5, 1.5, 1.7, 2.0, 2.5, 3.0], n) + rng.normal(0, 0.05, n) * (rng.random(n) < 0.7)
    pts = _world(cam, u, v, z)  # (identity pose: z_view is z, and the layers' depths tie exactly)
    pts[5:15, 2] = -1.0
    return cam, pts[rng.permutation(n)], rng.random((n, 3), dtype=F32)


def depth_bound_of_tile(case, ty, tx):
    """What the depth bound of tile (ty, tx) is when computed as csrc/raster.hip describes it, in float64: per pixel the
    smallest depth among the points whose centre is nearest to it, per b x b block the K-th smallest of those, per tile
    the largest over its blocks (inf: a block holds fewer than K such points) -> (bound, rows of the tile's list behind it)"""
    b, K, H, W = case.claims["block"], case.K, case.H, case.W
    ndc = ndc_of(case).astype(np.float64)
    s = min(H, W) / 2.0
    px, py = W / 2.0 - ndc[:, 0] * s - 0.5, H / 2.0 - ndc[:, 1] * s - 0.5  # pixel-index units
    zmin = np.full((H + 16, W + 16), np.inf)
    for x, y, z in zip(np.rint(px), np.rint(py), ndc[:, 2]):
        if z >= 0 and 0 <= x < W and 0 <= y < H:
            zmin[int(y), int(x)] = min(zmin[int(y), int(x)], z)
    bound = 0.0
    for by in range(16 * ty, min(16 * ty + 16, H), b):
        for bx in range(16 * tx, min(16 * tx + 16, W), b):
            blk = np.sort(zmin[by:by + b, bx:bx + b].reshape(-1))
            bound = max(bound, blk[K - 1])
    lists, _ = tile_lists(case)
    rows = lists.get((ty, tx), np.zeros(0, np.int64))
    return bound, rows[ndc[rows, 2] > bound]


def _threshold_cases():
    out = []
    for si, (H, W) in enumerate(THRESH_SIZES):
        cam, pts, feat = _layered_cloud(H, W, 7400 + si)
        for kind in THRESHOLDS:
            at, below = smallest_radius(THRESHOLDS[kind](H, W))
            for side, radius in (("below", below), ("at", at)):
                b = depth_bound_block(radius, H, W)
                Ks = range(1, 9) if b == 4 else ((4, 5) if b == 2 else (1, 3))
                for K in Ks:
                    claims = {"cloud": f"thr_{H}x{W}", "kind": kind, "side": side, "block": b, "bound_runs": b != 0 and K <= b * b,
                              "box2": box_within_2x2(radius, H, W), "segments": (-(-H // 16)) * (-(-W // 16)) >= 16}
                    out.append(Case(f"thr_{kind}_{side}_{H}x{W}_K{K}", H, W, cam, pts, feat, float(radius), K, claims))
    return out


# ---------------------------------------------------------------- shapes
def _shape_cases():
    out = []
    for i, ((H, W), rpx, n) in enumerate(SHAPE_SIZES):
        rng = np.random.default_rng(7500 + i)
        s = min(H, W) / 2.0
        radius = float(F32(rpx / s))
        cam = synth.flat_cam(H, W, np.array([[0.9 * s, 0, W / 2.0 + 0.3], [0, 0.95 * s, H / 2.0 - 0.2], [0, 0, 1.0]]), np.eye(4))
        u, v = rng.uniform(-4, W + 4, n), rng.uniform(-4, H + 4, n)
        e = np.arange(n) % 12 == 0  # edge-grazing: at the radius (in pixels, through this camera) from a pixel centre
        ang = rng.uniform(0, 2 * np.pi, n)
        u[e] = np.floor(u[e]) + 0.5 + rpx * np.cos(ang[e])
        v[e] = np.floor(v[e]) + 0.5 + rpx * np.sin(ang[e])
        z = np.round(rng.uniform(1.0, 2.0, n), 1)
        z[rng.integers(0, n, max(n // 20, 1))] = -0.5
        # (x_ndc = -(u - W / 2) / s whatever the focal length and the principal point: the camera's pixels are the raster's)
        pts = _world(cam, u, v, z)
        out.append(Case(f"shape_{H}x{W}", H, W, cam, pts, rng.random((n, 3), dtype=F32), radius, 3, {"cloud": f"shape_{H}x{W}"}))
    return out


# ---------------------------------------------------------------- all of them, and the statements over them
@functools.lru_cache(maxsize=None)
def cases():
    cs = _degenerate_cases() + _grazing_cases() + _threshold_cases() + _shape_cases()
    for c in cs:
        for a in (c.cam, c.pts, c.feat):
            a.setflags(write=False)
    return collections.OrderedDict((c.name, c) for c in cs)


def names(prefix=""):
    return [n for n in cases() if n.startswith(prefix)]


def families(*prefixes):
    return [n for n in cases() if n.startswith(tuple(prefixes))]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(idx, zbuf, d2, img, mask) of the oracle on a case, computed once per process and read-only"""
    c = cases()[name]
    if c.H * c.W * c.pts.shape[0] > 5e7:  # 4 x 8192: the point-major sweep (held to the pixel-major loop on windows by the host test)
        idx, zbuf, d2 = orc.rasterize_points_pointmajor(ndc_of(c), c.H, c.W, c.radius, c.K)
    else:
        idx, zbuf, d2 = orc.rasterize_points(c.pts, c.cam, c.H, c.W, c.radius, c.K)
    img = orc.composite(idx, d2, c.radius, c.feat)
    mask = (orc.composite(idx, d2, c.radius, None)[..., 0] > 0).astype(F32)
    for a in (idx, zbuf, d2, img, mask):
        a.setflags(write=False)
    return idx, zbuf, d2, img, mask


def _cloud_key(c):
    return (c.claims["cloud"], c.radius) if c.name.startswith("thr_") else (c.name, c.radius)


@functools.lru_cache(maxsize=None)
def _second_cloud(key):
    c = next(c for c in cases().values() if _cloud_key(c) == key)
    with np.errstate(all="ignore"):  # rows on the camera plane divide by zero, on purpose
        ndc = p3d.points_to_ndc(c.cam, c.pts, flavour="seq", inverse="f64")
        K = 8 if c.name.startswith("thr_") else c.K
        return (ndc,) + tuple(p3d.rasterize_points_naive(ndc, c.H, c.W, c.radius, K))


def second(name):
    """(ndc, idx, zbuf, d2) of the second statement (pytorch3d's chain and priority queue).  Cases that share a cloud and
    a radius share its K = 8 run: a pixel's K nearest under (z, id) are the first K of its 8 nearest."""
    c = cases()[name]
    ndc, idx, zbuf, d2 = _second_cloud(_cloud_key(c))
    return ndc, idx[..., :c.K], zbuf[..., :c.K], d2[..., :c.K]


def composite_f64(idx, d2, radius, feat):
    """NormWeightedCompositor in float64 on the float32 d2 and r2: (img[H,W,3], smallest weight per pixel (inf: no fragment))"""
    r2 = np.float64(F32(F32(radius) * F32(radius)))
    has = idx >= 0
    w = np.where(has, 1.0 - d2.astype(np.float64) / r2, 0.0)
    t = np.maximum(w.sum(-1), np.float64(F32(1e-4)))
    f = np.asarray(feat, np.float64)[np.maximum(idx, 0)]
    img = (w[..., None] * f).sum(-2) / t[..., None]
    return img, np.where(has, w, np.inf).min(-1)
