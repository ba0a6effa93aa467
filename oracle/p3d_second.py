"""SECOND, independent restatement of the pytorch3d 0.7.4 boundary of rows A9 (points; below) and A10 (mesh; the last
section of this file, which says what it pins and what it cannot) -- test infrastructure only.

pytorch3d is an un-vendored dependency of the reference (README.md:38, `conda install pytorch3d=0.7.4`)
and cannot be obtained in the build container (no wheel, no source, no network), so neither
`rasterize_points_cpu.cpp` nor the camera classes can be compiled or imported: **parity of A9 stays
unpinned**.  What can be bounded is how much the unknowable part matters.  oracle/pgdvs_oracle.c
restates the pipeline in pixel-friendly closed form; this file restates it the way pytorch3d itself
computes it, object by object, so that the two can be compared:

    cameras_from_opencv_projection   (pgdvs/utils/pytorch3d_utils.py:5-47 is a copy of it;
                                      call sites st_geo_renderer.py:86-88, pgdvs_renderer_dyn.py:685-690)
      R' = R^T with x,y columns negated, T' = t with x,y negated, f' = f / s, p0' = -(pp - wh/2) / s
    PointsRasterizer.transform
      pts_view = (Rotate(R').compose(Translate(T'))).transform_points(pts_world)
      pts_ndc  = (K'^T composed with the identity NDC transform).transform_points(pts_view)
      pts_ndc[..., 2] = pts_view[..., 2]
    Transform3d.transform_points: [x y z 1] @ M (one 4-term dot product per output, `torch.bmm`),
      then division by the 4th component
    RasterizePointsNaiveCpu: pixel centres from PixToNonSquareNdc with reversed indices, skip z < 0,
      strict dist2 < r^2, a max-heap of (z, idx, dist2) tuples trimmed to K
    NormWeightedCompositor: w = 1 - dist2 / r^2, out = sum w f / max(sum w, 1e-4)

The one thing reading cannot settle is the float32 rounding inside `torch.bmm` and `torch.inverse`:
BLAS kernels accumulate the 4 products in index order but may or may not fuse multiply and add, and
differ between the CPU (MKL / OpenBLAS) and the GPU (cuBLAS, FMA; nvcc also contracts
`dx*dx + dy*dy` in the CUDA rasteriser).  `flavour` selects the accumulation: "seq" rounds every
product and every sum (what pgdvs_oracle.c does), "fma" fuses each multiply-add (emulated through
float64: the product of two float32 is exact there).  tests/test_p3d_second.py measures how often
the two flavours -- i.e. the reference's own backends -- disagree on the z-buffer index.
"""
from __future__ import annotations

import heapq

import numpy as np

F = np.float32


def _dot4(rows, M, flavour):
    """rows[N,4] @ M[4,4] in float32, accumulating k = 0..3 in order."""
    rows = np.asarray(rows, F)
    M = np.asarray(M, F)
    out = np.empty((rows.shape[0], 4), F)
    for j in range(4):
        if flavour == "seq":
            acc = rows[:, 0] * M[0, j]
            for k in (1, 2, 3):
                acc = (acc + rows[:, k] * M[k, j]).astype(F)
        elif flavour == "fma":
            acc = (rows[:, 0].astype(np.float64) * np.float64(M[0, j])).astype(F)
            for k in (1, 2, 3):
                acc = (rows[:, k].astype(np.float64) * np.float64(M[k, j]) + acc.astype(np.float64)).astype(F)
        else:
            raise ValueError(flavour)
        out[:, j] = acc
    return out


class Transform3d:
    """row-vector convention, matrices composed left to right (pytorch3d/transforms/transform3d.py)"""

    def __init__(self, matrix=None):
        self._matrix = np.eye(4, dtype=F) if matrix is None else np.asarray(matrix, F).reshape(4, 4)
        self._transforms = []

    def compose(self, *others):
        out = Transform3d(self._matrix.copy())
        out._transforms = self._transforms + list(others)
        return out

    def get_matrix(self, flavour="seq"):
        m = self._matrix.copy()
        for other in self._transforms:
            m = _dot4(m, other.get_matrix(flavour), flavour)
        return m

    def transform_points(self, points, flavour="seq"):
        pts = np.asarray(points, F).reshape(-1, 3)
        hom = np.concatenate([pts, np.ones((pts.shape[0], 1), F)], axis=1)
        out = _dot4(hom, self.get_matrix(flavour), flavour)
        return (out[:, :3] / out[:, 3:]).astype(F)


class Rotate(Transform3d):
    def __init__(self, R):
        m = np.eye(4, dtype=F)
        m[:3, :3] = np.asarray(R, F)
        super().__init__(m)


class Translate(Transform3d):
    def __init__(self, T):
        m = np.eye(4, dtype=F)
        m[3, :3] = np.asarray(T, F)
        super().__init__(m)


class PerspectiveCameras:
    """in_ndc=True cameras as cameras_from_opencv_projection builds them"""

    def __init__(self, R, T, focal_length, principal_point):
        self.R, self.T = np.asarray(R, F), np.asarray(T, F)
        self.focal_length, self.principal_point = np.asarray(focal_length, F), np.asarray(principal_point, F)

    def get_world_to_view_transform(self):
        return Rotate(self.R).compose(Translate(self.T))

    def get_projection_transform(self):
        fx, fy = self.focal_length
        px, py = self.principal_point
        K = np.array([[fx, 0, px, 0], [0, fy, py, 0], [0, 0, 0, 1], [0, 0, 1, 0]], F)  # _get_sfm_calibration_matrix
        return Transform3d(K.T.copy())

    def get_ndc_camera_transform(self):
        return Transform3d()  # already in NDC


def cameras_from_opencv_projection(R, tvec, camera_matrix, image_size_hw):
    """R[3,3], tvec[3] = world-to-camera (OpenCV), camera_matrix[3,3], image_size (h, w)"""
    R, tvec, cm = np.asarray(R, F), np.asarray(tvec, F), np.asarray(camera_matrix, F)
    focal = np.array([cm[0, 0], cm[1, 1]], F)
    pp = cm[:2, 2].copy()
    wh = np.array([image_size_hw[1], image_size_hw[0]], F)
    scale = F(wh.min() / F(2.0))
    c0 = wh / F(2.0)
    focal_p3d = (focal / scale).astype(F)
    p0_p3d = (-(pp - c0) / scale).astype(F)
    R_p3d = R.T.copy()
    T_p3d = tvec.copy()
    R_p3d[:, :2] *= F(-1)
    T_p3d[:2] *= F(-1)
    return PerspectiveCameras(R_p3d, T_p3d, focal_p3d, p0_p3d)


def inverse_f32(c2w):
    """`torch.inverse(c2w)` on a float32 4x4: LAPACK single precision (getrf + getri), as torch's CPU path"""
    return np.linalg.inv(np.asarray(c2w, F)).astype(F)


def points_to_ndc(flat_cam_tgt, pts_world, flavour="seq", inverse="f32"):
    """st_geo_renderer.py:77-88 + PointsRasterizer.transform -> ndc[N,3] (x, y in NDC, z in view space)"""
    fc = np.asarray(flat_cam_tgt, F).reshape(-1)
    H, W = int(fc[0]), int(fc[1])
    K4, c2w = fc[2:18].reshape(4, 4), fc[18:34].reshape(4, 4)
    if inverse == "f32":
        w2c = inverse_f32(c2w)
    else:  # the closed-form oracle's choice: fp64 inverse rounded once
        w2c = np.linalg.inv(c2w.astype(np.float64)).astype(F)
    cams = cameras_from_opencv_projection(w2c[:3, :3], w2c[:3, 3], K4[:3, :3], (H, W))
    pts_view = cams.get_world_to_view_transform().transform_points(pts_world, flavour)
    proj = cams.get_projection_transform().compose(cams.get_ndc_camera_transform())
    ndc = proj.transform_points(pts_view, flavour)
    ndc[:, 2] = pts_view[:, 2]
    return ndc


def non_square_ndc_range(S1, S2):
    rng = F(2.0)
    if S1 > S2:
        rng = F(F(S1) * rng) / F(S2)  # "(S1 * range) / S2" of rasterization_utils
    return F(rng)


def pix_to_non_square_ndc(i, S1, S2):
    rng = non_square_ndc_range(S1, S2)
    offset = F(rng / F(2.0))
    return F(-offset + F(F(rng * F(i)) + offset) / F(S1))


def rasterize_points_naive(ndc, H, W, radius, K, fma_dist=False):
    """RasterizePointsNaiveCpu with its std::priority_queue of (z, idx, dist2) tuples (pure Python: small
    inputs only).  `fma_dist` = the CUDA flavour of dist2 (nvcc contracts dx*dx + dy*dy into one FMA)."""
    ndc = np.asarray(ndc, F)
    r2 = F(F(radius) * F(radius))
    idx = np.full((H, W, K), -1, np.int64)
    zbuf = np.full((H, W, K), -1, F)
    dist = np.full((H, W, K), -1, F)
    front = np.nonzero(~(ndc[:, 2] < 0))[0]
    for yi in range(H):
        yf = pix_to_non_square_ndc(H - 1 - yi, H, W)
        dy = (ndc[front, 1] - yf).astype(F)
        near_row = front[np.abs(dy) < np.sqrt(r2) * F(1.01) + F(1e-6)]
        for xi in range(W):
            xf = pix_to_non_square_ndc(W - 1 - xi, W, H)
            heap = []  # max-heap through negated keys
            for p in near_row:
                dx, dyy = F(ndc[p, 0] - xf), F(ndc[p, 1] - yf)
                if fma_dist:
                    d2 = F(np.float64(dx) * np.float64(dx) + np.float64(F(dyy * dyy)))
                else:
                    d2 = F(F(dx * dx) + F(dyy * dyy))
                if d2 < r2:
                    heapq.heappush(heap, (-float(ndc[p, 2]), -int(p), -float(d2)))
                    if len(heap) > K:
                        heapq.heappop(heap)  # drops the largest (z, idx, dist2)
            while heap:
                nz, nidx, nd = heapq.heappop(heap)
                i = len(heap)
                zbuf[yi, xi, i], idx[yi, xi, i], dist[yi, xi, i] = -nz, -nidx, -nd
    return idx, zbuf, dist


def norm_weighted_composite(idx, dist, radius, feat):
    """points/renderer.py: weights = 1 - dists2 / r^2; norm_weighted_sum_cpu.cpp"""
    H, W, K = idx.shape
    r2 = F(F(radius) * F(radius))
    out = np.zeros((H, W, feat.shape[1]), F)
    for yi in range(H):
        for xi in range(W):
            t = F(0)
            for k in range(K):
                if idx[yi, xi, k] < 0:
                    continue
                t = F(t + F(F(1) - F(dist[yi, xi, k] / r2)))
            t = max(t, F(1e-4))
            for k in range(K):
                n = idx[yi, xi, k]
                if n < 0:
                    continue
                w = F(F(1) - F(dist[yi, xi, k] / r2))
                out[yi, xi] = (out[yi, xi] + (w * feat[n]).astype(F) / t).astype(F)
    return out


# ---------------------------------------------------------------------------------------------------
# Row A10 (dyn_render_type = "mesh"): the second statement of the mesh path.
#
# pytorch3d's source cannot be obtained here, so the in-face formulas below (the bounding-box test, the
# +-1e-8 zero-area band, the 1e-8 added to the area, the perspective correction with its 1e-8 clamp and the
# strict ``bary > 0`` test) necessarily come from the same reading of ``CheckPixelInsideFace``
# (rasterize_meshes.cu) and geometry_utils.cuh as oracle/pgdvs_oracle.c's: if that reading is wrong, both
# are wrong, and **parity of the in-face arithmetic with pytorch3d stays UNPINNED**.  What is independent of
# the oracle and of csrc/mesh.hip is everything around those formulas:
#   * structure -- every pixel is tested against every face, in face order, as the naive rasteriser does;
#     there is no candidate pixel range (``ndc_to_pix_range`` is this project's invention) and no packed
#     64-bit key: the winner is the minimum of (z, face index);
#   * the explicit face list -- faces are rows of vertex ranks built the way render_dyn_mesh builds them
#     (pgdvs_renderer_dyn.py:550-604: two stacks of candidates concatenated, the in-bounds filter, then the
#     ``> 0`` filter), pinned to the reference's own output by tests/golden/mesh_edges.npz; the oracle and the
#     kernel derive faces implicitly as (source pixel, kind);
#   * the precision -- ``dtype=np.float32`` rounds every operation on its own (the "seq" flavour above, the
#     oracle's operation order), ``dtype=np.float64`` is the high-precision reference on the same float32
#     vertices.
# ---------------------------------------------------------------------------------------------------
MESH_EPS = 1e-8


def mesh_faces_from_keep(keep):
    """keep[H,W] (non-zero = a vertex) -> faces[#face,3] int64 of vertex ranks, in the reference's order."""
    keep = np.asarray(keep) != 0
    h, w = keep.shape
    rows, cols = np.nonzero(keep)  # row-major, as torch.nonzero
    vert_idxs_img = np.full((h, w), -1, np.int64)
    vert_idxs_img[rows, cols] = np.arange(rows.shape[0])
    # (row, col) -> (row, col), (row + 1, col), (row + 1, col + 1)  and  (row, col), (row + 1, col + 1), (row, col + 1)
    cand_1 = np.stack([np.stack([rows, cols], 1), np.stack([rows + 1, cols], 1), np.stack([rows + 1, cols + 1], 1)], 1)
    cand_2 = np.stack([np.stack([rows, cols], 1), np.stack([rows + 1, cols + 1], 1), np.stack([rows, cols + 1], 1)], 1)
    cand = np.concatenate([cand_1, cand_2], 0).reshape(-1, 3, 2)  # [#cand, 3, 2]
    in_bound = np.all((cand[..., 0] >= 0) & (cand[..., 0] < h) & (cand[..., 1] >= 0) & (cand[..., 1] < w), axis=1)
    cand = cand[in_bound]
    face_v = vert_idxs_img[cand[..., 0], cand[..., 1]].reshape(-1, 3)
    return face_v[np.all(face_v > 0, axis=1)].astype(np.int64)  # sic: vertex 0 counts as "no vertex"


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _pixel_centres(H, W, dtype):
    """pixel centres in NDC, [H*W] each (PixToNonSquareNdc with reversed indices)"""
    if dtype == np.float32:
        xs = np.array([pix_to_non_square_ndc(W - 1 - xi, W, H) for xi in range(W)], F)
        ys = np.array([pix_to_non_square_ndc(H - 1 - yi, H, W) for yi in range(H)], F)
    else:
        def centre(i, S1, S2):
            rng = 2.0 * S1 / S2 if S1 > S2 else 2.0
            return -rng / 2.0 + (rng * i + rng / 2.0) / S1

        xs = np.array([centre(W - 1 - xi, W, H) for xi in range(W)], np.float64)
        ys = np.array([centre(H - 1 - yi, H, W) for yi in range(H)], np.float64)
    return np.tile(xs, H), np.repeat(ys, W)


def _face_terms(px, py, v0, v1, v2, eps):
    """CheckPixelInsideFace's arithmetic for one face at the pixel centres (px, py): the bounding-box flag, the
    perspective-corrected barycentrics and z, unfiltered"""
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = v0, v1, v2
    xmin, xmax = np.fmin(np.fmin(x0, x1), x2), np.fmax(np.fmax(x0, x1), x2)
    ymin, ymax = np.fmin(np.fmin(y0, y1), y2), np.fmax(np.fmax(y0, y1), y2)
    outside = (px > xmax) | (px < xmin) | (py > ymax) | (py < ymin)
    area = _edge(x2, y2, x0, y0, x1, y1) + eps
    b0 = _edge(px, py, x1, y1, x2, y2) / area
    b1 = _edge(px, py, x2, y2, x0, y0) / area
    b2 = _edge(px, py, x0, y0, x1, y1) / area
    t0 = b0 * z1 * z2
    t1 = z0 * b1 * z2
    t2 = z0 * z1 * b2
    den = np.fmax(t0 + t1 + t2, eps)
    w0, w1, w2 = t0 / den, t1 / den, t2 / den
    z = w0 * z0 + w1 * z1 + w2 * z2
    return outside, w0, w1, w2, z


def rasterize_meshes_naive(ndc, faces, H, W, dtype=np.float32):
    """RasterizeMeshesNaive for blur_radius 0, faces_per_pixel 1, perspective-correct, no clipping, no culling:
    every pixel against every face of ``faces[#face,3]`` (indices into ``ndc[#vert,3]``), in face order.
    -> face index [H,W] int64 (-1 = none), z [H,W], barycentrics [H,W,3], all in ``dtype``."""
    dt = np.dtype(dtype).type
    v = np.asarray(ndc, F).astype(dt)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    px, py = _pixel_centres(H, W, dt)
    eps, zero = dt(F(MESH_EPS)), dt(0)
    P = H * W
    best = np.full(P, -1, np.int64)
    zbuf = np.zeros(P, dt)
    bary = np.zeros((P, 3), dt)
    with np.errstate(all="ignore"):
        for f, (i0, i1, i2) in enumerate(faces):
            v0, v1, v2 = v[i0], v[i1], v[i2]
            zmax = np.fmax(np.fmax(v0[2], v1[2]), v2[2])
            face_area = _edge(v0[0], v0[1], v1[0], v1[1], v2[0], v2[1])
            if zmax < zero or (face_area <= eps and face_area >= -eps):
                continue
            outside, w0, w1, w2, z = _face_terms(px, py, v0, v1, v2, eps)
            inside = ~outside & ~(z < zero) & (w0 > zero) & (w1 > zero) & (w2 > zero)
            win = inside & ((best < 0) | (z < zbuf))  # strict: among equal z the earlier face stays
            best[win], zbuf[win] = f, z[win]
            bary[win, 0], bary[win, 1], bary[win, 2] = w0[win], w1[win], w2[win]
    return best.reshape(H, W), zbuf.reshape(H, W), bary.reshape(H, W, 3)


def face_at_pixel(ndc, tri, H, W, yi, xi, dtype=np.float64):
    """one face at one pixel, unfiltered: (smallest |barycentric|, z) -- how close the pixel is to the face's border"""
    dt = np.dtype(dtype).type
    v = np.asarray(ndc, F).astype(dt)
    px, py = _pixel_centres(H, W, dt)
    k = yi * W + xi
    with np.errstate(all="ignore"):
        _, w0, w1, w2, z = _face_terms(px[k:k + 1], py[k:k + 1], v[tri[0]], v[tri[1]], v[tri[2]], dt(F(MESH_EPS)))
    return float(min(abs(w0[0]), abs(w1[0]), abs(w2[0]))), float(z[0])


def interpolate_vertex_colors(face_idx, bary, faces, feat):
    """TexturesVertex.sample_textures (interpolate_face_attributes: sum over the three corners in order) followed
    by hard_rgb_blend on a black background -> img[H,W,C] in bary's dtype"""
    dt = bary.dtype.type
    feat = np.asarray(feat, F).astype(dt)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    H, W = face_idx.shape
    img = np.zeros((H, W, feat.shape[1]), dt)
    hit = face_idx >= 0
    if hit.any():
        fv = faces[face_idx[hit]]  # [n, 3]
        b = bary[hit]
        a = b[:, 0:1] * feat[fv[:, 0]]
        a = a + b[:, 1:2] * feat[fv[:, 1]]
        a = a + b[:, 2:3] * feat[fv[:, 2]]
        img[hit] = a
    return img


def render_mesh(ndc, faces, feat, H, W, dtype=np.float32):
    """render_dyn_mesh's two renders (pgdvs_renderer_dyn.py:646-658): the colour image, and the mask as
    ``(render of ones) > 0`` -> img[H,W,3], mask[H,W] (float32 0/1), face index[H,W], z[H,W]"""
    idx, z, bary = rasterize_meshes_naive(ndc, faces, H, W, dtype)
    img = interpolate_vertex_colors(idx, bary, faces, feat)
    ones = interpolate_vertex_colors(idx, bary, faces, np.ones((np.asarray(ndc).shape[0], 1), F))
    return img, (ones[..., 0] > 0).astype(F), idx, z
