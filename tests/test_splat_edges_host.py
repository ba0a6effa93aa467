"""CPU only: the cases of tests/splat_cases.py checked against themselves before any kernel sees them.  On every case the
float64 restatement agrees with the C oracle (orc.softsplat_img, orc.softsplat, orc.softsplat_bwd_raw) within the derived
bound; a plain float32 numpy version of the same formulas stays within it too, with its worst err / bound recorded in the
*_MEASURED tables; each case exercises what it claims (window columns 39 / 40, origins, flags, clamps, exact zeros); the
pixels unsure about the 1e-3 threshold are few; no signed normaliser sits next to its pole; and three deliberately wrong
variants of the restatement each leave the bound on a named case -- otherwise the cases would not see such a kernel."""
import numpy as np
import pytest

import splat_cases as S
from oracle import oracle as orc

F32, F64 = S.F32, S.F64
COMPOSITE = list(S.composite_cases())
GENERIC = list(S.generic_cases())


def _recorded(table, key, value):
    assert value <= 1.0, (key, value)
    assert key in table, f"record {key!r}: {value:.3g} in splat_cases.py"
    assert abs(table[key] - value) <= 0.05 * table[key] + 1e-3, (key, table[key], value)


# ---------------------------------------------------------------- composite
@pytest.mark.parametrize("name", COMPOSITE)
def test_composite_float64_vs_oracle_and_float32(name):
    c, ref = S.composite_cases()[name], S.composite_ref(name)
    bound, unsure = S.composite_bound(c, ref)
    live = int(ref.live.sum())
    # the unsure cap, from the restatement alone
    assert unsure.sum() <= min(S.UNSURE_PIXEL_CAP, S.UNSURE_SHARE_CAP * live), (int(unsure.sum()), live)
    assert not ref.dyn_mask[~ref.live].any()  # a pixel no dynamic source reaches is below the threshold: splatted mask 0
    assert np.isfinite(ref.r).all() and (ref.den > 0).all()
    if c.claims.get("both_sides"):
        assert c.alpha == 100.0 and 0 < ref.dyn_mask.sum() < live, (ref.dyn_mask.sum(), live)
    r_orc, _ = S.composite_ratio(S.oracle_composite(c), c, ref)
    assert r_orc <= 1.0, r_orc
    r32, _ = S.composite_ratio(S.composite(c, F32), c, ref)
    _recorded(S.COMPOSITE32_MEASURED, name, r32)


def test_border_claims():
    c = S.composite_cases()["border_37x53"]
    assert c.W % S.TILE == 5 and c.H % S.TILE == 5
    idx, x0, y0, _ = S.corners(*S.splat_positions(c.f1t), c.H, c.W)
    for sy, sx in c.claims["outside_blocks"]:
        assert (idx[:, sy:sy + 5, sx:sx + 5] < 0).all(), (sy, sx)  # blocks wholly outside flag nothing
    for sy, sx in c.claims["inside_blocks"]:
        assert (idx[:, sy:sy + 5, sx:sx + 5] >= 0).any(), (sy, sx)
    assert len(c.claims["outside_blocks"]) == 6 and len(c.claims["ragged_sources"]) >= 2
    dyn = c.mask != 0
    # every listed landing: x0 = -1 with a target in (-1, 0), exactly 0, exactly W - 1, (W - 1, W), W, beyond, below -1
    X, Y = S.splat_positions(c.f1t)
    for P, n in ((X, c.W), (Y, c.H)):
        p = P[dyn]
        assert ((p > -1) & (p < 0)).any() and (p == 0).any() and (p == n - 1).any() and ((p > n - 1) & (p < n)).any()
        assert (p == n).any() and (p > n + 1).any() and (p < -1).any() and (np.floor(p) == -2).any()
    fl = S.flagged(c)
    assert fl[c.H - 1, c.W - 1] and fl[:, 0].any() and fl[0].any() and fl[:, c.W - 1].sum() > 1 and fl[c.H - 1].sum() > 1
    ref = S.composite_ref("border_37x53")
    assert ref.n[c.H - 1, c.W - 1] >= 25


def test_window_claims():
    c = S.composite_cases()["window_48x112"]
    geo = S.tile_geometry(c)
    t = {k: geo.tiles[v] for k, v in c.claims["tiles"].items()}
    # the count of corners inside and outside the window, per tile (16 lanes x 2 corners on the column / row past it)
    assert (t["A"]["max_wx"], t["A"]["n_in"], t["A"]["n_out"]) == (S.WIN - 1, 1024, 0)
    assert (t["B"]["max_wx"], t["B"]["n_in"], t["B"]["n_out"]) == (S.WIN, 992, 32)
    assert (t["C"]["max_wy"], t["C"]["n_in"], t["C"]["n_out"]) == (S.WIN - 1, 992, 0)  # (its last column leaves the image)
    assert (t["D"]["max_wy"], t["D"]["n_in"], t["D"]["n_out"]) == (S.WIN, 992, 32)
    assert (t["E"]["n_in"], t["E"]["n_out"]) == (729, 295) and t["E"]["max_wx"] == t["E"]["max_wy"] == 46
    assert 255 in t["F"]["lane_x"] and 255 in t["F"]["lane_y"] and 0 not in t["F"]["lane_x"] + t["F"]["lane_y"]
    assert t["F"]["n_out"] == 0
    g = t["G"]  # the origin comes from static lanes (lx >= 8), every dynamic corner is outside the window
    assert all(lane % 16 >= 8 for lane in g["lane_x"] + g["lane_y"])
    assert (g["dyn_in"], g["dyn_out"], g["n_in"]) == (0, 496, 512)
    ty, tx = c.claims["tiles"]["G"]
    assert geo.part[ty * 16:ty * 16 + 15, tx * 16 + 8:tx * 16 + 16].all()  # static, but flagged by E's content
    for name in ("window_48x112_a0", "window_48x112_a3"):
        o = S.composite_cases()[name]
        assert np.array_equal(o.f1t, c.f1t) and np.array_equal(o.mask, c.mask) and o.alpha != c.alpha


def test_lone_claims():
    c = S.composite_cases()["lone_33x33"]
    fl = S.flagged(c)
    assert sorted(map(tuple, np.argwhere(fl))) == [(16, 16), (16, 17), (17, 16), (17, 17)]  # the dead pixels flag nothing
    assert c.mask[15, 15] == 1 and 15 % S.TILE == S.TILE - 1  # the last lane of the first tile
    idx = S.corners(*S.splat_positions(c.f1t), c.H, c.W)[0]
    targets = {16 * 33 + 16, 16 * 33 + 17, 17 * 33 + 16, 17 * 33 + 17}
    tiles = {(y // S.TILE, x // S.TILE) for y, x in c.claims["reachers"] if c.mask[y, x] == 0 and targets & set(idx[:, y, x])}
    assert tiles == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for y, x in c.claims["dead"]:
        assert c.mask[y, x] == 1 and (idx[:, y, x] < 0).all()
    # ... and change no output: the same scene without them
    import types
    mask = c.mask.copy()
    for y, x in c.claims["dead"]:
        mask[y, x] = 0.0
    other = S.composite(types.SimpleNamespace(**{**vars(c), "mask": mask}), F64)
    ref = S.composite_ref("lone_33x33")
    for k in ("dyn_rgb", "dyn_mask", "comb", "comb_st", "comb_dy"):
        assert np.array_equal(getattr(other, k), getattr(ref, k)), k


@pytest.mark.parametrize("tag", ["int", "half", "frac"])
def test_collide_claims(tag):
    name = f"collide_{tag}_32x48"
    c, ref = S.composite_cases()[name], S.composite_ref(name)
    ty, tx = c.claims["target"]
    assert ref.n[ty, tx] >= 512
    X, Y = S.splat_positions(c.f1t)
    idx, x0, y0, ok = S.corners(X, Y, c.H, c.W)
    w = S.weights(X, Y, x0, y0, ok, F32)[:, :16, :32]
    if c.claims["exact"]:  # one corner has weight exactly 1 and three exactly 0: the skip rule
        assert (w[0] == 1).all() and (w[1:] == 0).all() and (ref.n[ty, tx + 1], ref.dyn_mask.sum()) == (ref.n[ty + 1, tx + 1], 1)
    else:
        assert (w > 0).all() and (ref.n[ty:ty + 2, tx:tx + 2] >= 512).all()
    assert len({(y // 16, x // 16) for y in range(16) for x in range(32)}) == 2  # the block spans two tiles


def test_empty_full_and_range_claims():
    c, ref = S.composite_cases()["empty_18x20"], S.composite_ref("empty_18x20")
    assert not c.mask.any() and not ref.live.any()
    assert not ref.dyn_mask.any() and not ref.dyn_rgb.any() and not ref.comb_dy.any() and np.array_equal(ref.comb, c.static)
    for name in ("full_16x16", "full_2x2"):
        c, ref = S.composite_cases()[name], S.composite_ref(name)
        want = c.rgb1.transpose(2, 0, 1).astype(F64) / (1.0 + 1e-7)
        assert np.abs(ref.dyn_rgb - want).max() <= 1e-15 and ref.dyn_mask.all() and c.alpha == 0
    c = S.composite_cases()["soft_24x40"]
    assert set(np.unique(c.mask)) == {0.0, 0.25, 0.5, 1.0}
    for name in ("range_24x40_a1", "range_24x40_a3"):
        c, ref = S.composite_cases()[name], S.composite_ref(name)
        part = S.tile_geometry(c).part
        assert c.rgb1.max() > 2.9 and ref.clamped[part].mean() >= 0.10  # alpha l1 > alpha: the clamp is active
    for name, ext in (("thin_2x70", 0), ("thin_70x2", 1)):
        c = S.composite_cases()[name]
        assert (c.H, c.W)[ext] == 2 and c.mask.any()


def test_wrong_variants_leave_the_bound():
    """a restatement that drops what lies more than 40 columns from the tile's origin, one that skips static sources
    unconditionally, one that reads the threshold as 2e-3: the oracle is outside each one's bound on the named case"""
    for name, kind in (("window_48x112", "window"), ("window_48x112_a0", "window"), ("lone_33x33", "static"),
                       ("soft_24x40", "static"), ("window_48x112", "threshold"), ("border_37x53", "threshold")):
        c = S.composite_cases()[name]
        got = S.oracle_composite(c)
        assert S.composite_ratio(got, c, S.composite_ref(name))[0] <= 1.0
        if kind == "window":
            geo = S.tile_geometry(c)
            wrong = S.composite(c, F64, keep=geo.in_win | (geo.idx < 0))
        elif kind == "static":
            wrong = S.composite(c, F64, drop_static=True)
        else:
            wrong = S.composite(c, F64, thr=2e-3)
        assert S.composite_ratio(got, c, wrong)[0] > 1.0, (name, kind)


# ---------------------------------------------------------------- generic forward and backward
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", GENERIC)
def test_forward_float64_vs_oracle_and_float32(name, mode):
    g = S.generic_cases()[name]
    want, bound, nrm, n = S.forward_ref(name, mode)
    parts = mode.split("-")
    metric = None if parts[0] in ("sum", "avg") else (g.metric_lin if parts[0] == "linear" else g.metric)
    flow = g.flow_q if parts[0] == "linear" else g.flow
    assert S.worst_ratio(orc.softsplat(g.x, flow, metric, mode), want, bound) <= 1.0
    _recorded(S.FORWARD32_MEASURED, f"{name}:{mode}", S.worst_ratio(S.forward(g, mode, F32)[0], want, bound))
    if g.nan_src is not None:  # NaN * 0 at the zero-weight corners of a source with integer flow
        y, x = g.nan_src
        f = flow[0, :, y, x]
        assert tuple(f) == (1.0, 0.0) and np.isnan(g.x[0, 0, y, x])
        lit = np.argwhere(np.isnan(want[0, 0]))
        assert {tuple(p) for p in lit} == {(yy, xx) for yy in (y, y + 1) for xx in (x + 1, x + 2) if yy < g.H and xx < g.W}
        assert not np.isnan(want[0, 1:]).any() and not np.isnan(want[1:]).any()
    if parts[0] == "linear":
        # no comparison on a pole: every normaliser is an exact zero by construction or >= 1e-3 away from -1e-7
        zero = np.zeros(nrm.shape, bool)
        if g.zero_t is not None:
            zero[(slice(None),) + g.zero_t] = True
            assert (nrm[zero] == 0).all() and (n[zero] == 2).all()
            assert (orc.softsplat_raw(g.metric_lin, flow)[:, 0][zero] == 0).all()  # ... in float32 too: +m and -m
            (ya, xa), (yb, xb), (yt, xt) = g.zero_src
            assert (g.metric_lin[:, 0, ya, xa] == 0.875).all() and (g.metric_lin[:, 0, yb, xb] == -0.875).all()
            num = g.x[:, :, ya, xa].astype(F64) * 0.875 + g.x[:, :, yb, xb].astype(F64) * -0.875
            div = {"zeroeps": 1.0}.get(parts[-1], 1e-7)  # addeps divides by 1e-7, zeroeps by 1, clipeps by 1e-7
            assert np.array_equal(want[:, :, yt, xt], num / div)
            assert (nrm < -0.1).any()  # ... and normalisers well below zero
        rest = (n > 0) & ~zero
        assert (np.abs(nrm[rest] + S.EPS) >= S.POLE_DISTANCE).all(), np.abs(nrm[rest] + S.EPS).min()


def test_generic_flows_hold_every_listed_edge():
    for name in GENERIC[3:]:
        g = S.generic_cases()[name]
        for flow in (g.flow, g.flow_q):
            f = flow[0]
            X, Y = S.splat_positions(f)
            assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and (np.abs(f) == 1e9).any()
            assert ((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any()
            for P, nn in ((X, g.W), (Y, g.H)):
                fl = np.floor(P[np.isfinite(P)])
                assert {-2.0, -1.0, nn - 1.0, float(nn)} <= set(fl) and (P == nn - 1).any()
            assert ((f[0] == np.round(f[0])) & (f[1] == np.round(f[1])) & np.isfinite(f).all(0)).sum() >= 2
    assert [(g.B, g.C, g.H, g.W) for g in S.generic_cases().values()] == [(1, 1, 1, 1)] * 3 + [(3, 5, 1, 300), (2, 8, 17, 16),
                                                                                               (1, 2, 16, 17)]
    assert [float(g.flow[0, 0, 0, 0]) for g in list(S.generic_cases().values())[:3]] == [0.0, 0.5, -0.5]


@pytest.mark.parametrize("name", GENERIC)
def test_backward_float64_vs_oracle_and_float32(name):
    g = S.generic_cases()[name]
    gi, gf, bi, bf, read = S.backward_ref(name)
    oi, of = orc.softsplat_bwd_raw(g.x_fin, g.flow, g.og)
    assert S.worst_ratio(oi, gi, bi) <= 1.0 and S.worst_ratio(of, gf, bf) <= 1.0
    gi32, gf32 = S.backward(g, F32)[:2]
    _recorded(S.BACKWARD32_MEASURED, name, max(S.worst_ratio(gi32, gi, bi), S.worst_ratio(gf32, gf, bf)))
    # the plain float32 version shares the oracle's operation order
    assert np.array_equal(gi32, oi) and np.array_equal(gf32, of)
    assert np.isfinite(gi).all() and np.isfinite(gf).all()  # the NaN in outgrad sits where no corner reads
    if g.og_nan is not None:
        assert np.isnan(g.og[0, :, g.og_nan[0], g.og_nan[1]]).all() and not read[0][g.og_nan]
    dead = ~np.isfinite(g.flow).all(1) | (np.abs(g.flow) >= 1e9).any(1)  # non-finite or far outside: zero gradients
    if g.H * g.W > 1:
        assert dead.any()
    assert not gi[np.broadcast_to(dead[:, None], gi.shape)].any() and not gf[np.broadcast_to(dead[:, None], gf.shape)].any()
    # at an integer position: the one-sided derivative of the cell floor selects (weights 1, 0, 0, 0)
    X, Y = S.splat_positions(g.flow[0])
    at = np.argwhere((X == np.floor(X)) & (Y == np.floor(Y)) & (X >= 0) & (X < g.W - 1) & (Y >= 0) & (Y < g.H - 1))
    for y, x in at[:3]:
        tx, ty = int(X[y, x]), int(Y[y, x])
        o = g.og[0].astype(F64)
        want = sum((o[c, ty, tx + 1] - o[c, ty, tx]) * float(g.x_fin[0, c, y, x]) for c in range(g.C))
        assert abs(gf[0, 0, y, x] - want) <= 1e-12 * (1 + abs(want))
        assert np.array_equal(gi[0, :, y, x], o[:, ty, tx])
