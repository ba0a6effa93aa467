"""Cases for the splat kernels (csrc/softsplat.hip: pgdvs_softsplat_fwd, pgdvs_softsplat_bwd, pgdvs_dyn_splat_composite and
its _rng twin) at the inputs on which the kernels take their own decisions -- the 40 x 40 LDS window of a 16 x 16 source
tile, the flag pre-pass, the static-pixel skip, the zero-weight skip, ragged last tiles, image borders, signed and zero
normalisers, integer positions -- with float64 restatements of the upstream formulas the kernel header cites
(pgdvs/utils/softsplat.py:280-617, pgdvs_renderer_base.py:59-138, pgdvs_renderer_dyn.py:177-202, pgdvs_renderer.py:169-178)
and an error bound derived from the operation sequence, not fitted to any result.

Positions.  Upstream forms two positions in float32 and so does every statement here, operation by operation, one
rounding each: the backwarp coordinate (linspace(-1, 1, steps) as ATen computes it, + flow / ((W - 1) / 2), + 1, / 2,
* (W - 1)) and the splat position x + flow.  A float64 position would differ by ~u W pixels, which at alpha = 100 moves
exp(-alpha l1) by more than every later rounding together.  Everything after the positions (bilinear weights, sums, exp,
ratios) is float64 in the reference statement (D = float64) and float32 in the plain numpy version (D = float32).

Every restatement returns, per output element, ``n`` (the number of non-zero-weight contributions summed into it) and
``A`` (the same expression with the absolute value of every term); the bound is built from them (see BOUND below).

Composite families (``composite_cases()``; layouts are the C ABI's: rgb1 / rgb2 [H,W,3], flow12 [H,W,2], flow_1_to_tgt
[2,H,W], mask [H,W], noise / static_rgb [3,H,W]).  Unless stated: colours uniform in [0,1), flow12 ~ N(0, 0.7^2), noise
N(0,1), static pixels drift by a quarter pixel, alpha = 100, static_rgb given.

  border_37x53    ragged last tiles both ways; 5 x 5 dynamic blocks with constant flows whose first pixel lands, in x and
                  likewise in y, at -0.5 (x0 = -1), 0.0, W - 1, W - 0.5, W, W + 3.25, -1.5 and -6.5, and one block whose 25
                  pixels all land on the bottom-right corner pixel.  Blocks wholly outside flag nothing.
  window_48x112   tile-aligned 16 x 16 blocks stretched so that the farthest in-image corner is window column 39 (A), 40
                  (B), row 39 (C), row 40 (D); one block x 3 both ways (E); one mirrored both ways so the origin comes from
                  lane 255 (F); one tile half dynamic moving +60.5 px, half static but flagged by E's content, so the origin
                  comes from a static lane and every dynamic corner takes the global path (G).  Also at alpha = 0 and 3.
  lone_33x33      one dynamic pixel at (15,15) with flow (+1.5,+1.5); static pixels of four tiles reach its four targets;
                  single dynamic pixels with flow NaN, +inf, -inf, 1e9 and +40 px (outside) flag nothing, change nothing.
  collide_*_32x48 a 16 x 32 block (two tiles) all onto one target: at (40,20) (weights exactly 1,0,0,0: the skip rule), at
                  (40.5,20.5) and at (40.3,20.6); 512 contributions per accumulator.
  empty_18x20     mask all zero.           full_16x16, full_2x2   mask all one, zero flow, alpha = 0.
  soft_24x40      mask values in {0, 0.25, 0.5, 1}.
  range_24x40     colours in [0,3) at alpha = 1 and 3: the metric's clamp [-alpha, alpha] is active.
  thin_2x70, thin_70x2   2 is the smallest extent at which the backwarp's normalisation is defined.

Generic families (``generic_cases()``): shapes (1,1,1,1) with flow 0, +0.5, -0.5; (3,5,1,300); (2,8,17,16); (1,2,16,17); the
rows of ``_specials`` spliced in: integer flows, flows onto the last row / column, +-0.0, NaN, +-inf, +-1e9, floor equal
to -2, -1, W-1, W (and H); a NaN input value at a source with integer flow (upstream's NaN * 0).  Two flow fields per
shape: ``flow`` (real offsets) for sum / avg / soft*, ``flow_q`` (quarter-pixel offsets: every weight is a multiple of
1/16) for linear*, whose metric is signed: with real offsets a weight of 1e-4 alone would put a normaliser next to its
pole.  ``zero_t``: two sources with metrics +0.875 and -0.875 land on that target at integer flows and no other source
touches it: its float32 normaliser is exactly 0 in any order.

Test infrastructure only: tests/test_splat_edges_host.py runs it without a GPU, tests/test_gpu_splat_edges.py runs the
kernels over it.  Nothing here touches the GPU."""
import functools
import types

import numpy as np

from oracle import oracle as orc

F32, F64 = np.float32, np.float64
U = 2.0 ** -24       # float32 unit roundoff: one rounding moves a value by at most u |value|
TINY = 2.0 ** -126   # smallest normal float32: below it a term's error is absolute (or the term is flushed)
TILE, WIN = 16, 40   # kSplatTile, kSplatWin (csrc/softsplat.hip, above dyn_splat_scatter_kernel)
THR = float(F32(1e-3))  # (.) > 1e-3 on a float32 tensor compares with the float32 nearest 1e-3
EPS = 1e-7

# BOUND.  A sum of n float32 terms t_i, each carrying c roundings on its way from the inputs, differs from the exact sum
# by at most (c + n) u sum |t_i| to first order, in any order of summation (n - 1 adds; adding onto a zero is exact).  A
# ratio num / den of two such sums adds the relative errors of both and two roundings of its own (den + 1e-7 with the
# float32 1e-7, and the division):
#     |got - want| <= (c + n) u (A_num / |den| + |num| A_den / den^2) + 2 u |num / den|  =:  2 (c + 1 + n) u A
# with A = (A_num / |den| + |num| A_den / den^2) / 2 >= |num / den| -- for non-negative terms A = A_num / den, the
# expression with absolute values.  Plain sums (mode "sum", the backward) have no factor 2 and no + 1.
#
# Roundings of one term, read off the operation sequence (softsplat.py:365-401 and the kernel alike):
#   bilinear weight  (sex - X) (sey - Y): each difference rounds once (only in the cells next to 0, where
#                    |X| < 1 has a finer grid than 1 - X), the product once                                         3
#   generic sum      v w                                                                          C_SUM    = 3 + 1 = 4
#   avg              as sum; the ratio's own two roundings                                         C_AVG    = 4 + 1 = 5
#   linear           (v m) w                                                                       C_LINEAR = 5 + 1 = 6
#   soft             (v exp(m)) w, exp within 1 ulp = 2 u                                           C_SOFT   = 7 + 1 = 8
#   composite        (c1 e) w with e = exp(.) within 1 ulp                                         C_0      = 7 + 1 = 8
#   backward         ingrad: g w  -> 4;  flowgrad: (g v) d with d one difference  -> 3
# The composite's e = exp(clip(-alpha l1)) also carries the error of its argument: an absolute error d of the argument
# is a relative error d of e.  With colours of magnitude <= L:
#   warp_k = sum of <= 4 terms rgb2 w: 3 (weight) + 1 (product) + 3 (adds) = 7 roundings on terms summing to <= L    7 u L
#   d_k = c1_k - warp_k: one rounding on |d_k|; sabs = (|d_0| + |d_1|) + |d_2|: two; / 3: one -> 4 u l1 <= 4 u L      4 u L
#   -alpha l1: one rounding                                                                                 alpha u L
# -> C_E = 7 + 4 + 1 = 12: the argument is within 12 alpha L u, and so is e relatively.  c1 = rgb1 m + nz (1 - m) is
# exact for m in {0, 1}; a soft mask adds 1 - m, two products and a sum, <= 3 u L on c1: C_SOFTMASK = 3 more in both.
# (Read at a glance the kernel gives ~9 and ~6; the counts here are worst cases per operation.)
# Terms below TINY are outside the relative model: (n + 1) TINY / |den| is added -- at most ~1e-29, nothing a wrong
# kernel could hide behind.
C_SUM, C_AVG, C_LINEAR, C_SOFT = 4, 5, 6, 8
C_E, C_0, C_SOFTMASK = 12, 8, 3
C_INGRAD, C_FLOWGRAD = 4, 3

UNSURE_SHARE_CAP, UNSURE_PIXEL_CAP = 0.01, 4
POLE_DISTANCE = 1e-3

# worst |float32 numpy - float64| / bound per case, measured on the CPU (tests/test_splat_edges_host.py asserts that
# these are what it finds, to 5 % + 0.001, and that each is <= 1)
COMPOSITE32_MEASURED = {
    "border_37x53": 0.023, "window_48x112": 0.034, "window_48x112_a0": 0.165, "window_48x112_a3": 0.068,
    "lone_33x33": 0.003, "collide_int_32x48": 0.001, "collide_half_32x48": 0.001, "collide_frac_32x48": 0.001,
    "empty_18x20": 0.000, "full_16x16": 0.055, "full_2x2": 0.053, "soft_24x40": 0.027,
    "range_24x40_a1": 0.052, "range_24x40_a3": 0.032, "thin_2x70": 0.028, "thin_70x2": 0.012,
}
FORWARD32_MEASURED = {
    "one_zero:sum": 0.000, "one_zero:avg": 0.024, "one_zero:linear": 0.019,
    "one_zero:linear-addeps": 0.019, "one_zero:linear-zeroeps": 0.000, "one_zero:linear-clipeps": 0.121,
    "one_zero:soft": 0.057, "one_zero:soft-zeroeps": 0.000, "one_zero:soft-clipeps": 0.000,
    "one_plus:sum": 0.000, "one_plus:avg": 0.082, "one_plus:linear": 0.016,
    "one_plus:linear-addeps": 0.016, "one_plus:linear-zeroeps": 0.000, "one_plus:linear-clipeps": 0.120,
    "one_plus:soft": 0.008, "one_plus:soft-zeroeps": 0.000, "one_plus:soft-clipeps": 0.000,
    "one_minus:sum": 0.000, "one_minus:avg": 0.107, "one_minus:linear": 0.033,
    "one_minus:linear-addeps": 0.033, "one_minus:linear-zeroeps": 0.000, "one_minus:linear-clipeps": 0.045,
    "one_minus:soft": 0.041, "one_minus:soft-zeroeps": 0.000, "one_minus:soft-clipeps": 0.000,
    "row_3x5x1x300:sum": 0.450, "row_3x5x1x300:avg": 0.221, "row_3x5x1x300:linear": 0.232,
    "row_3x5x1x300:linear-addeps": 0.232, "row_3x5x1x300:linear-zeroeps": 0.181, "row_3x5x1x300:linear-clipeps": 0.285,
    "row_3x5x1x300:soft": 0.222, "row_3x5x1x300:soft-zeroeps": 0.188, "row_3x5x1x300:soft-clipeps": 0.188,
    "tall_2x8x17x16:sum": 0.373, "tall_2x8x17x16:avg": 0.230, "tall_2x8x17x16:linear": 0.231,
    "tall_2x8x17x16:linear-addeps": 0.231, "tall_2x8x17x16:linear-zeroeps": 0.194, "tall_2x8x17x16:linear-clipeps": 0.305,
    "tall_2x8x17x16:soft": 0.189, "tall_2x8x17x16:soft-zeroeps": 0.181, "tall_2x8x17x16:soft-clipeps": 0.181,
    "wide_1x2x16x17:sum": 0.317, "wide_1x2x16x17:avg": 0.211, "wide_1x2x16x17:linear": 0.203,
    "wide_1x2x16x17:linear-addeps": 0.203, "wide_1x2x16x17:linear-zeroeps": 0.201, "wide_1x2x16x17:linear-clipeps": 0.258,
    "wide_1x2x16x17:soft": 0.224, "wide_1x2x16x17:soft-zeroeps": 0.168, "wide_1x2x16x17:soft-clipeps": 0.168,
}
BACKWARD32_MEASURED = {
    "one_zero": 0.025, "one_plus": 0.033, "one_minus": 0.004,
    "row_3x5x1x300": 0.463, "tall_2x8x17x16": 0.404, "wide_1x2x16x17": 0.315,
}


# ---------------------------------------------------------------- float32 positions (upstream's operation sequence)
def splat_positions(flow):
    """flow[2,H,W] float32 -> X, Y float32: x + flow, one rounding"""
    H, W = flow.shape[-2:]
    xs = np.arange(W, dtype=F32)[None, :]
    ys = np.arange(H, dtype=F32)[:, None]
    with np.errstate(all="ignore"):
        return (xs + flow[0]).astype(F32), (ys + flow[1]).astype(F32)


def linspace_pm1(steps):
    """torch.linspace(-1, 1, steps) as ATen computes it, float32"""
    i = np.arange(steps)
    step = F32(2.0) / F32(steps - 1)
    lo = F32(-1.0) + step * i.astype(F32)
    hi = F32(1.0) - step * (steps - 1 - i).astype(F32)
    return np.where(i < steps // 2, lo, hi).astype(F32)


def backwarp_positions(flow12):
    """flow12[H,W,2] float32 -> ix, iy float32 (pgdvs_renderer_base.py:91-138, grid_sample's unnormalise, align_corners)"""
    H, W = flow12.shape[:2]
    hw_x, hw_y = (F32(W) - F32(1.0)) / F32(2.0), (F32(H) - F32(1.0)) / F32(2.0)
    with np.errstate(all="ignore"):
        gx = linspace_pm1(W)[None, :] + flow12[..., 0] / hw_x
        gy = linspace_pm1(H)[:, None] + flow12[..., 1] / hw_y
        ix = ((gx + F32(1.0)) / F32(2.0)) * F32(W - 1)
        iy = ((gy + F32(1.0)) / F32(2.0)) * F32(H - 1)
    assert ix.dtype == F32 and iy.dtype == F32
    return ix, iy


def corners(X, Y, H, W):
    """idx[4,H,W]: flat index of the nw, ne, sw, se corner or -1 if dropped; x0, y0 (int64, -8 where the position is not
    finite or so far outside that no corner can pass its bounds test); ok"""
    ok = np.isfinite(X) & np.isfinite(Y)
    x0 = np.floor(np.where(ok, X, 0).astype(F64))
    y0 = np.floor(np.where(ok, Y, 0).astype(F64))
    ok = ok & (x0 >= -2) & (x0 <= W) & (y0 >= -2) & (y0 <= H)
    x0 = np.where(ok, x0, -8).astype(np.int64)
    y0 = np.where(ok, y0, -8).astype(np.int64)
    idx = []
    for k in range(4):
        cx, cy = x0 + (k & 1), y0 + (k >> 1)
        inb = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        idx.append(np.where(inb, cy * W + cx, -1))
    return np.stack(idx), x0, y0, ok


def weights(X, Y, x0, y0, ok, D):
    """the four bilinear weights in D from the float32 position (softsplat.py:376-379)"""
    Xd, Yd = np.where(ok, X, 0).astype(D), np.where(ok, Y, 0).astype(D)
    wx, wy = x0.astype(D), y0.astype(D)
    ex, ey = (x0 + 1).astype(D), (y0 + 1).astype(D)
    return np.stack([(ex - Xd) * (ey - Yd), (Xd - wx) * (ey - Yd), (ex - Xd) * (Yd - wy), (Xd - wx) * (Yd - wy)])


def exp_(x, D):
    """exp in D, correctly rounded for float32 (numpy's SIMD float32 exp is allowed 2.5 ulp; the bound counts 1)"""
    with np.errstate(all="ignore"):
        return np.exp(x.astype(F64)).astype(D)


def splat_raw(vals, X, Y, D, keep=None):
    """softsplat_out (softsplat.py:352-402): vals[C,H,W] in D summed at the corners of (X, Y).  Sequential sums in D, corner
    by corner and in raster order of the sources within a corner.  -> out[C,H,W], n[H,W], A[C,H,W]"""
    C, H, W = vals.shape
    idx, x0, y0, ok = corners(X, Y, H, W)
    w = weights(X, Y, x0, y0, ok, D)
    out, A, n = np.zeros((C, H * W), D), np.zeros((C, H * W), D), np.zeros(H * W, np.int64)
    with np.errstate(all="ignore"):
        for k in range(4):
            sel = idx[k] >= 0
            if keep is not None:
                sel = sel & keep[k]
            t, wk = idx[k][sel], w[k][sel]
            np.add.at(n, t[wk != 0], 1)
            for c in range(C):
                term = (vals[c][sel] * wk).astype(D)
                np.add.at(out[c], t, term)
                np.add.at(A[c], t, np.abs(term))
    return out.reshape(C, H, W), n.reshape(H, W), A.reshape(C, H, W)


def _ratio_A(num, A_num, den, A_den):
    with np.errstate(all="ignore"):
        return 0.5 * (A_num / np.abs(den) + np.abs(num) * A_den / (den * den))


def worst_ratio(got, want, bound, where=None):
    """max |got - want| / bound over ``where``; a NaN must meet a NaN, and where the bound is 0 the values must be equal
    (inf otherwise)"""
    got, want, bound = np.asarray(got, F64), np.asarray(want, F64), np.asarray(bound, F64)
    sel = np.ones(want.shape, bool) if where is None else np.broadcast_to(where, want.shape)
    got, want, bound = got[sel], want[sel], np.broadcast_to(bound, sel.shape)[sel]
    if got.size == 0:
        return 0.0
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    fin = ~np.isnan(want)
    with np.errstate(all="ignore"):
        err = np.abs(got[fin] - want[fin])
        b = bound[fin]
        r = np.where(err == 0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------- the composite
def backwarp(rgb2, ix, iy, D):
    """grid_sample(bilinear, zeros, align_corners=True) of rgb2[H,W,3] at (ix, iy) -> [3,H,W] in D; corners nw, ne, sw, se"""
    H, W = ix.shape
    fin = np.isfinite(ix) & np.isfinite(iy) & (np.abs(ix) < 1e9) & (np.abs(iy) < 1e9)
    x0 = np.where(fin, np.floor(np.where(fin, ix, 0).astype(F64)), -10).astype(np.int64)
    y0 = np.where(fin, np.floor(np.where(fin, iy, 0).astype(F64)), -10).astype(np.int64)
    w = weights(ix, iy, x0, y0, fin, D)
    img = rgb2.astype(D)
    out = np.zeros((3, H, W), D)
    for k in range(4):
        cx, cy = x0 + (k & 1), y0 + (k >> 1)
        inb = fin & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        v = img[np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]  # [H,W,3]
        for c in range(3):
            out[c] = np.where(inb, out[c] + v[..., c] * w[k], out[c])
    return out


def flagged(c):
    """the target pixels a corner of a source pixel with non-zero mask reaches (the flag pre-pass; 'live' pixels)"""
    X, Y = splat_positions(c.f1t)
    idx = corners(X, Y, c.H, c.W)[0]
    fl = np.zeros(c.H * c.W, bool)
    src = c.mask != 0
    for k in range(4):
        t = idx[k][src]
        fl[t[t >= 0]] = True
    return fl.reshape(c.H, c.W)


def composite(c, D=F64, keep=None, thr=THR, drop_static=False, noise=None):
    """pgdvs_renderer_dyn.py:177-202 + pgdvs_renderer.py:169-178 in D (positions float32).  ``keep`` [4,H,W], ``thr`` and
    ``drop_static`` exist for the deliberately wrong variants of the host test."""
    H, W = c.H, c.W
    m = c.mask.astype(D)
    nz = np.clip(c.noise if noise is None else noise, 0.0, 1.0).astype(D)
    with np.errstate(all="ignore"):
        c1 = c.rgb1.transpose(2, 0, 1).astype(D) * m + nz * (D(1.0) - m)
        ix, iy = backwarp_positions(c.flow12)
        d = np.abs(c1 - backwarp(c.rgb2, ix, iy, D))
        l1 = ((d[0] + d[1]) + d[2]) / D(3.0)
        a = D(c.alpha)
        arg = np.clip(-a * l1, -a, a)
        e = exp_(arg, D)
        vals = np.stack([c1[0] * e, c1[1] * e, c1[2] * e, e, m * e]).astype(D)
        X, Y = splat_positions(c.f1t)
        if drop_static:
            keep = np.broadcast_to(c.mask != 0, (4, H, W)) & (True if keep is None else keep)
        acc, n, A = splat_raw(vals, X, Y, D, keep)
        den = acc[3] + D(EPS)
        r = acc / den
        dm = (r[4] > D(thr)).astype(D)
        dyn_rgb = r[:3] * dm
        st = c.static.astype(D)
        comb_st = (D(1.0) - dm) * st
        comb_dy = dm * dyn_rgb
    assert r.dtype == D and comb_dy.dtype == D
    return types.SimpleNamespace(dyn_rgb=dyn_rgb, dyn_mask=dm, comb=comb_st + comb_dy, comb_st=comb_st, comb_dy=comb_dy, r=r,
                                 acc=acc, den=den, n=n, A=A, l1=l1, clamped=(-a * l1) < -a, live=flagged(c))


def composite_bound(c, ref):
    """bound on r (rows 0..2 colour, 4 mask) from a float64 ``composite`` result, and the pixels unsure about the threshold"""
    cc = (C_E + (C_SOFTMASK if c.soft else 0)) * c.alpha * c.L + C_0 + (C_SOFTMASK if c.soft else 0)
    A = _ratio_A(ref.acc, ref.A, ref.den, ref.A[3] + EPS)
    bound = 2.0 * (cc + ref.n) * U * A + (ref.n + 1) * TINY / ref.den
    unsure = ref.live & (np.abs(ref.r[4] - THR) <= bound[4])
    return bound, unsure


def composite_ratio(got, c, ref, scale=1.0):
    """worst err / bound of the five images in ``got`` (an object with dyn_rgb, dyn_mask, comb, comb_st, comb_dy) against
    the float64 result; -> (ratio, number of unsure pixels).  Outside the unsure pixels the mask is equal, not close; so is
    the static share of the composite; where the mask is 0 every colour is the exact 0 or the exact static colour."""
    bound, unsure = composite_bound(c, ref)
    sure = ~unsure
    if not np.array_equal(np.asarray(got.dyn_mask, F64)[sure], ref.dyn_mask[sure]):
        return np.inf, int(unsure.sum())
    if not np.array_equal(np.asarray(got.comb_st, F64)[:, sure], ref.comb_st[:, sure]):
        return np.inf, int(unsure.sum())
    b = scale * bound[:3] * ref.dyn_mask
    worst = max(worst_ratio(getattr(got, k), getattr(ref, k), b, sure[None]) for k in ("dyn_rgb", "comb_dy", "comb"))
    return worst, int(unsure.sum())


def oracle_composite(c):
    """the same five images from the C oracle (float32), as tests/test_gpu_round3.py composes them"""
    m4 = c.mask[None, None]
    c1 = (np.transpose(c.rgb1, (2, 0, 1))[None] * m4 + np.clip(c.noise, 0.0, 1.0)[None] * (F32(1.0) - m4)).astype(F32)
    c2 = np.ascontiguousarray(np.transpose(c.rgb2, (2, 0, 1))[None])
    f12 = np.ascontiguousarray(np.transpose(c.flow12, (2, 0, 1))[None])
    splat_full, metric = orc.softsplat_img(c1, c.f1t[None], c2, f12, c.alpha)
    splat_mask, _ = orc.softsplat_img(m4.astype(F32), c.f1t[None], c2, f12, c.alpha, metric=metric)
    dm = (splat_mask[0, 0] > F32(1e-3)).astype(F32)
    dyn_rgb = splat_full[0] * dm[None]
    comb_st = (F32(1.0) - dm)[None] * c.static
    comb_dy = dm[None] * dyn_rgb
    return types.SimpleNamespace(dyn_rgb=dyn_rgb, dyn_mask=dm, comb=comb_st + comb_dy, comb_st=comb_st, comb_dy=comb_dy)


def tile_geometry(c):
    """The scatter's tile rule restated from the kernel's comments: a lane takes part if one of its corners is in the image
    and it is dynamic (mask != 0) or one of its in-image corners is flagged; the window origin of a 16 x 16 source tile is
    the smallest max(x0, 0) / max(y0, 0) over its lanes that take part; a corner is inside the window if its offset from
    the origin is in [0, 40) both ways.  -> part[H,W], in_win[4,H,W] (of in-image corners of lanes taking part), idx, and
    per tile (ty, tx): dict(ox, oy, lane_x, lane_y (lanes giving the origin), n_in, n_out, dyn_in, dyn_out)"""
    H, W = c.H, c.W
    X, Y = splat_positions(c.f1t)
    idx, x0, y0, ok = corners(X, Y, H, W)
    fl = flagged(c).reshape(-1)
    hit = np.zeros((H, W), bool)
    for k in range(4):
        hit |= (idx[k] >= 0) & fl[np.clip(idx[k], 0, None)]
    part = (idx >= 0).any(0) & ((c.mask != 0) | hit)
    in_win = np.zeros((4, H, W), bool)
    tiles = {}
    for ty in range(-(-H // TILE)):
        for tx in range(-(-W // TILE)):
            sl = (slice(ty * TILE, min(H, ty * TILE + TILE)), slice(tx * TILE, min(W, tx * TILE + TILE)))
            p = part[sl]
            if not p.any():
                continue
            cx, cy = np.maximum(x0[sl], 0), np.maximum(y0[sl], 0)
            ox, oy = int(cx[p].min()), int(cy[p].min())
            lx = np.argwhere(p & (cx == ox))
            ly = np.argwhere(p & (cy == oy))
            t = dict(ox=ox, oy=oy, lane_x=[int(a * TILE + b) for a, b in lx], lane_y=[int(a * TILE + b) for a, b in ly],
                     n_in=0, n_out=0, dyn_in=0, dyn_out=0, max_wx=-1, max_wy=-1)
            for k in range(4):
                wx, wy = x0[sl] + (k & 1) - ox, y0[sl] + (k >> 1) - oy
                live = p & (idx[k][sl] >= 0)
                inside = live & (wx >= 0) & (wx < WIN) & (wy >= 0) & (wy < WIN)
                in_win[k][sl] = inside
                dyn = c.mask[sl] != 0
                t["n_in"] += int(inside.sum())
                t["n_out"] += int((live & ~inside).sum())
                t["dyn_in"] += int((inside & dyn).sum())
                t["dyn_out"] += int((live & ~inside & dyn).sum())
                if live.any():
                    t["max_wx"] = max(t["max_wx"], int(wx[live].max()))
                    t["max_wy"] = max(t["max_wy"], int(wy[live].max()))
            tiles[(ty, tx)] = t
    return types.SimpleNamespace(part=part, in_win=in_win, idx=idx, tiles=tiles)


# ---------------------------------------------------------------- composite cases
def _base(name, H, W, seed, alpha=100.0, L=1.0, soft=False):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(F32)
    f1t = np.zeros((2, H, W), F32)
    f1t[0] = F32(0.25) * np.sin(ys / F32(5.0))  # the static pixels drift a little
    f1t[1] = F32(0.25) * np.cos(xs / F32(7.0))
    return types.SimpleNamespace(
        name=name, H=H, W=W, alpha=float(alpha), L=float(L), soft=soft,
        rgb1=rng.random((H, W, 3), dtype=F32) * F32(L), rgb2=rng.random((H, W, 3), dtype=F32) * F32(L),
        flow12=(rng.standard_normal((H, W, 2)) * 0.7).astype(F32), noise=rng.standard_normal((3, H, W)).astype(F32),
        f1t=f1t, mask=np.zeros((H, W), F32), static=rng.random((3, H, W), dtype=F32), claims={}, rng=rng, xs=xs, ys=ys)


def _block(c, sy, sx, h, w, X, Y):
    """make source block [sy:sy+h, sx:sx+w] dynamic and send its pixels to the positions X, Y (arrays over the block)"""
    sl = (slice(sy, sy + h), slice(sx, sx + w))
    c.f1t[0][sl] = (np.asarray(X, F64) - c.xs[sl]).astype(F32)
    c.f1t[1][sl] = (np.asarray(Y, F64) - c.ys[sl]).astype(F32)
    c.mask[sl] = 1.0
    return sl


def _edge_positions(n):
    """(first-pixel position of a 5-pixel run along an axis of extent n, whether any of its corners is in the image)"""
    return [(-0.5, True), (0.0, True), (n - 1.0, True), (n - 0.5, True), (float(n), False), (n + 3.25, False), (-1.5, True),
            (-6.5, False)]


def _border():
    H, W = 37, 53
    c = _base("border_37x53", H, W, 11)
    slots_x, slots_y = [1, 8, 15, 22, 29, 36, 43, 48], [1, 8, 15, 22, 32]
    inside, outside = [], []
    i5 = np.arange(5, dtype=F64)
    for i, (t, vis) in enumerate(_edge_positions(W)):  # edges in x; sources in the first row of slots, the last one ragged
        sy, sx = slots_y[0], slots_x[i]
        _block(c, sy, sx, 5, 5, (t + i5)[None, :] + 0 * i5[:, None], (sy + 0.3 + i5)[:, None] + 0 * i5[None, :])
        (inside if vis else outside).append((sy, sx))
    for i, (t, vis) in enumerate(_edge_positions(H)):  # edges in y; sources in the ragged last row of tiles
        sy, sx = slots_y[4], slots_x[i]
        _block(c, sy, sx, 5, 5, (sx + 0.3 + i5)[None, :] + 0 * i5[:, None], (t + i5)[:, None] + 0 * i5[None, :])
        (inside if vis else outside).append((sy, sx))
    sy, sx = slots_y[2], slots_x[3]  # all 25 pixels onto the bottom-right corner pixel
    _block(c, sy, sx, 5, 5, np.full((5, 5), W - 1.0), np.full((5, 5), H - 1.0))
    inside.append((sy, sx))
    c.claims.update(inside_blocks=inside, outside_blocks=outside, both_sides=True,
                    ragged_sources=[b for b in inside + outside if b[0] >= 32 or b[1] >= 48])
    return c


def _window(alpha=100.0):
    H, W = 48, 112
    c = _base("window_48x112" + ("" if alpha == 100.0 else f"_a{alpha:g}"), H, W, 12, alpha=alpha)
    i16 = np.arange(16, dtype=F64)
    row, col = i16[None, :] + 0 * i16[:, None], i16[:, None] + 0 * i16[None, :]
    _block(c, 0, 0, 16, 16, 2.25 + (38.5 / 15) * row, 0.4 + col)                 # A: last corner on window column 39
    _block(c, 0, 48, 16, 16, 50.25 + (39.5 / 15) * row, 0.4 + col)               # B: ... on column 40
    _block(c, 0, 96, 16, 16, 96.3 + row, 1.25 + (38.5 / 15) * col)               # C: row 39
    _block(c, 16, 0, 16, 16, 0.3 + row, 2.25 + (39.5 / 15) * col)                # D: row 40
    _block(c, 16, 32, 16, 16, 20.3 + 3 * row, 0.6 + 3 * col)                     # E: x 3 both ways
    _block(c, 16, 64, 16, 16, 100.4 - 2 * row, 45.3 - 2 * col)                   # F: mirrored, origin from lane 255
    _block(c, 32, 16, 16, 8, 16 + 60.5 + row[:, :8], 32 + 0.25 + col[:, :8])     # G: left half dynamic, +60.5 px
    c.claims.update(both_sides=alpha == 100.0,
                    tiles=dict(A=(0, 0), B=(0, 3), C=(0, 6), D=(1, 0), E=(1, 2), F=(1, 4), G=(2, 1)))
    return c


def _lone():
    H = W = 33
    c = _base("lone_33x33", H, W, 13)
    _block(c, 15, 15, 1, 1, [[16.5]], [[16.5]])
    # static pixels of four tiles reach its targets (16,16), (17,16), (16,17), (17,17)
    for (y, x), (X, Y) in {(14, 14): (15.6, 15.7), (14, 17): (16.6, 15.6), (17, 14): (15.7, 16.7), (18, 18): (16.6, 16.6)}.items():
        c.f1t[0, y, x], c.f1t[1, y, x] = F32(X - x), F32(Y - y)
    dead = {(5, 5): (np.nan, 0.3), (5, 20): (0.2, np.inf), (20, 5): (-np.inf, 0.1), (25, 25): (1e9, 0.0), (8, 30): (40.0, 0.0),
            (28, 3): (0.0, -1e9)}
    for (y, x), (fx, fy) in dead.items():
        c.f1t[0, y, x], c.f1t[1, y, x], c.mask[y, x] = F32(fx), F32(fy), 1.0
    c.claims.update(dead=list(dead), reachers=[(14, 14), (14, 17), (17, 14), (18, 18)])
    return c


def _collide(tag, X, Y):
    c = _base(f"collide_{tag}_32x48", 32, 48, 14)
    _block(c, 0, 0, 16, 32, np.full((16, 32), X), np.full((16, 32), Y))
    c.claims.update(target=(int(np.floor(Y)), int(np.floor(X))), exact=float(X).is_integer())
    return c


def _random_dynamic(c, share, sigma):
    dyn = c.rng.random((c.H, c.W)) < share
    f = (c.rng.standard_normal((2, c.H, c.W)) * sigma).astype(F32)
    c.f1t[:, dyn] = f[:, dyn]
    return dyn


def _soft():
    c = _base("soft_24x40", 24, 40, 15, soft=True)
    dyn = _random_dynamic(c, 0.5, 1.5)
    c.mask[dyn] = c.rng.choice(np.array([0.25, 0.5, 1.0], F32), size=int(dyn.sum()))
    c.claims.update(both_sides=True)
    return c


def _range(alpha):
    c = _base(f"range_24x40_a{alpha:g}", 24, 40, 16, alpha=alpha, L=3.0)
    c.mask[_random_dynamic(c, 0.3, 1.5)] = 1.0
    return c


def _thin(H, W):
    c = _base(f"thin_{H}x{W}", H, W, 17)
    c.mask[_random_dynamic(c, 0.3, 0.8)] = 1.0
    return c


def _empty():
    return _base("empty_18x20", 18, 20, 18)


def _full(n):
    c = _base(f"full_{n}x{n}", n, n, 19, alpha=0.0)
    c.mask[:] = 1.0
    c.f1t[:] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def composite_cases():
    cs = [_border(), _window(), _window(0.0), _window(3.0), _lone(), _collide("int", 40.0, 20.0), _collide("half", 40.5, 20.5),
          _collide("frac", 40.3, 20.6), _empty(), _full(16), _full(2), _soft(), _range(1.0), _range(3.0), _thin(2, 70),
          _thin(70, 2)]
    for c in cs:
        for k in ("rgb1", "rgb2", "flow12", "noise", "f1t", "mask", "static"):
            a = np.ascontiguousarray(getattr(c, k), F32)
            a.setflags(write=False)
            setattr(c, k, a)
    return {c.name: c for c in cs}


@functools.lru_cache(maxsize=None)
def composite_ref(name):
    """the float64 result of a case, computed once and shared"""
    return composite(composite_cases()[name], F64)


# ---------------------------------------------------------------- generic forward / backward
MODES = ("sum", "avg", "linear", "linear-addeps", "linear-zeroeps", "linear-clipeps", "soft", "soft-zeroeps", "soft-clipeps")


def forward(g, mode, D=F64):
    """softsplat() (softsplat.py:280-333) in D -> out[B,C,H,W], bound[B,C,H,W] (meaningful for D = float64), nrm[B,H,W] or
    None, n[B,H,W]"""
    parts = mode.split("-")
    x = g.x.astype(D)
    flow = g.flow_q if parts[0] == "linear" else g.flow
    B, C, H, W = x.shape
    outs, bounds, nrms, ns = [], [], [], []
    for b in range(B):
        X, Y = splat_positions(flow[b])
        with np.errstate(all="ignore"):
            if parts[0] == "sum":
                vals, cc = x[b], C_SUM
            elif parts[0] == "avg":
                vals, cc = np.concatenate([x[b], np.ones((1, H, W), D)]), C_AVG
            elif parts[0] == "linear":
                m = g.metric_lin[b].astype(D)
                vals, cc = np.concatenate([x[b] * m, m]), C_LINEAR
            else:
                e = exp_(g.metric[b].astype(D), D)
                vals, cc = np.concatenate([x[b] * e, e]), C_SOFT
            acc, n, A = splat_raw(vals.astype(D), X, Y, D)
            if parts[0] == "sum":
                outs.append(acc), bounds.append((cc + n) * U * A + (n + 1) * TINY), nrms.append(None), ns.append(n)
                continue
            nrm, A_den = acc[-1], A[-1]
            if len(parts) == 1 or parts[1] == "addeps":
                den, A_den = nrm + D(EPS), A_den + EPS
            elif parts[1] == "zeroeps":
                den, A_den = np.where(nrm == 0, D(1.0), nrm), np.where(nrm == 0, 0.0, A_den)
            else:
                den, A_den = np.where(nrm < D(EPS), D(EPS), nrm), np.where(nrm < D(EPS), 0.0, A_den)
            out = acc[:-1] / den
            bound = 2.0 * (cc + n) * U * _ratio_A(acc[:-1], A[:-1], den, A_den) + (n + 1) * TINY / np.abs(den)
        outs.append(out), bounds.append(bound), nrms.append(nrm), ns.append(n)
    return (np.stack(outs), np.stack(bounds), None if nrms[0] is None else np.stack(nrms), np.stack(ns))


def backward(g, D=F64):
    """softsplat_ingrad / softsplat_flowgrad (softsplat.py:459-617) in D on (x_fin, flow, og): at an integer position the
    derivative is the one-sided one of the cell floor selects.  -> gi, gf, bound_gi, bound_gf, read[B,H,W] (outgrad pixels
    some corner reads)"""
    x, og = g.x_fin.astype(D), g.og.astype(D)
    B, C, H, W = x.shape
    gi, gf = np.zeros((B, C, H, W), D), np.zeros((B, 2, H, W), D)
    Ai, Af = np.zeros((B, C, H, W), D), np.zeros((B, 2, H, W), D)
    ni, read = np.zeros((B, H, W), np.int64), np.zeros((B, H * W), bool)
    for b in range(B):
        X, Y = splat_positions(g.flow[b])
        idx, x0, y0, ok = corners(X, Y, H, W)
        w = weights(X, Y, x0, y0, ok, D)
        Xd, Yd = np.where(ok, X, 0).astype(D), np.where(ok, Y, 0).astype(D)
        ex, ey, wx, wy = (x0 + 1).astype(D), (y0 + 1).astype(D), x0.astype(D), y0.astype(D)
        dx = [-(ey - Yd), ey - Yd, -(Yd - wy), Yd - wy]
        dy = [-(ex - Xd), -(Xd - wx), ex - Xd, Xd - wx]
        with np.errstate(all="ignore"):
            for c in range(C):
                flat = og[b, c].reshape(-1)
                for k in range(4):
                    inb = idx[k] >= 0
                    if c == 0:
                        read[b][idx[k][inb]] = True
                        ni[b] += inb
                    gk = flat[np.clip(idx[k], 0, None)]
                    t = np.where(inb, gk * w[k], 0).astype(D)
                    gi[b, c] = gi[b, c] + t
                    Ai[b, c] = Ai[b, c] + np.abs(t)
                    for j, d in ((0, dx[k]), (1, dy[k])):
                        t = np.where(inb, gk * x[b, c] * d, 0).astype(D)
                        gf[b, j] = gf[b, j] + t
                        Af[b, j] = Af[b, j] + np.abs(t)
    bi = (C_INGRAD + ni[:, None]) * U * Ai + 5 * TINY
    bf = (C_FLOWGRAD + C * ni[:, None]) * U * Af + (4 * C + 1) * TINY
    return gi, gf, bi, bf, read.reshape(B, H, W)


def _specials(H, W):
    """(fx or None, X or None, fy or None, Y or None): a flow component given directly, or through the position it must
    produce; None leaves the base flow"""
    rows = [(1.0, None, 0.0, None), (-1.0, None, 2.0, None), (0.0, None, -0.0, None), (-0.0, None, 0.0, None),
            (None, W - 1.0, None, None), (None, None, None, H - 1.0), (None, W - 1.0, None, H - 1.0),
            (np.nan, None, None, None), (None, None, np.nan, None), (np.inf, None, None, None), (None, None, -np.inf, None),
            (-np.inf, None, np.inf, None), (1e9, None, None, None), (None, None, -1e9, None), (-1e9, None, 1e9, None)]
    for t in (-1.75, -0.75, W - 0.75, W + 0.25):
        rows.append((None, t, None, None))
    for t in (-1.75, -0.75, H - 0.75, H + 0.25):
        rows.append((None, None, None, t))
    return rows


def _generic(name, B, C, H, W, seed, flow0=None, zero=None):
    rng = np.random.default_rng(seed)
    P = H * W
    x = rng.standard_normal((B, C, H, W)).astype(F32)
    sy = 0.4 if H == 1 else 1.5
    flow = (rng.standard_normal((B, 2, H, W)) * np.array([1.5, sy])[None, :, None, None]).astype(F32)
    flow_q = (rng.integers(-10, 11, (B, 2, H, W)) * np.array([0.25, 0.25 if H > 1 else 0.0])[None, :, None, None]).astype(F32)
    metric = rng.standard_normal((B, 1, H, W)).astype(F32)
    metric_lin = (rng.uniform(0.5, 1.5, (B, 1, H, W)) * rng.choice([-1.0, 1.0], (B, 1, H, W))).astype(F32)
    nan_src = None
    if flow0 is not None:
        flow[:] = F32(flow0)
        flow_q[:] = F32(flow0)
    else:
        for f in (flow, flow_q):
            for i, (fx, X, fy, Y) in enumerate(_specials(H, W)):
                p = 7 * i + 3
                assert p < P
                y, xx = divmod(p, W)
                for b in range(B):
                    if fx is not None:
                        f[b, 0, y, xx] = F32(fx)
                    if X is not None:
                        f[b, 0, y, xx] = F32(X - xx)
                    if fy is not None:
                        f[b, 1, y, xx] = F32(fy)
                    if Y is not None:
                        f[b, 1, y, xx] = F32(Y - y)
        nan_src = divmod(3, W)  # the first special: flow (1, 0), weights exactly 1, 0, 0, 0
        x[0, 0][nan_src] = np.nan
    zero_t = None
    if zero is not None:
        (ya, xa), (yb, xb), (yt, xt) = zero
        for (ys_, xs_), s in (((ya, xa), 1.0), ((yb, xb), -1.0)):
            flow_q[:, 0, ys_, xs_], flow_q[:, 1, ys_, xs_] = F32(xt - xs_), F32(yt - ys_)
            metric_lin[:, 0, ys_, xs_] = F32(0.875 * s)
        for b in range(B):  # nobody else may touch the target
            idx = corners(*splat_positions(flow_q[b]), H, W)[0]
            touch = (idx == yt * W + xt).any(0)
            touch[ya, xa] = touch[yb, xb] = False
            flow_q[b, 0][touch] = np.nan
        zero_t = (yt, xt)
    og = rng.standard_normal((B, C, H, W)).astype(F32)
    g = types.SimpleNamespace(name=name, B=B, C=C, H=H, W=W, x=x, x_fin=np.nan_to_num(x), flow=flow, flow_q=flow_q, metric=metric,
                              metric_lin=metric_lin, og=og, nan_src=nan_src, zero_t=zero_t, zero_src=zero, og_nan=None)
    read = backward(g)[4]
    free = np.argwhere(~read[0])
    if len(free):  # a NaN in outgrad where no corner reads it
        g.og_nan = tuple(int(v) for v in free[len(free) // 2])
        og[0, :, g.og_nan[0], g.og_nan[1]] = np.nan
    for k in ("x", "x_fin", "flow", "flow_q", "metric", "metric_lin", "og"):
        getattr(g, k).setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def generic_cases():
    # (seeds: the first from 21 on at which no signed normaliser of flow_q lies within 5e-3 of its pole -- found on the CPU,
    # asserted at 1e-3 by the host test)
    gs = [_generic("one_zero", 1, 1, 1, 1, 21, flow0=0.0), _generic("one_plus", 1, 1, 1, 1, 22, flow0=0.5),
          _generic("one_minus", 1, 1, 1, 1, 23, flow0=-0.5),
          _generic("row_3x5x1x300", 3, 5, 1, 300, 33, zero=((0, 200), (0, 201), (0, 250))),
          _generic("tall_2x8x17x16", 2, 8, 17, 16, 25, zero=((8, 5), (8, 6), (10, 9))),
          _generic("wide_1x2x16x17", 1, 2, 16, 17, 26, zero=((8, 5), (8, 6), (10, 9)))]
    return {g.name: g for g in gs}


@functools.lru_cache(maxsize=None)
def forward_ref(name, mode):
    return forward(generic_cases()[name], mode, F64)


@functools.lru_cache(maxsize=None)
def backward_ref(name):
    return backward(generic_cases()[name], F64)
