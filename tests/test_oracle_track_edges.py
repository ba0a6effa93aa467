"""CPU: the oracle (oracle/) against the tracker-window edge fixtures, made by the reference itself
(tests/golden/make_golden_track_edges.py): ties for first and second place in time, extrapolation, a target on
a real frame's time, two frames with one time stamp, offset raw times; one closest frame, one-sided windows, two
real frames, 64 frames; tracks on integers, half-integers, the borders and one float32 spacing either side of
them, negative and far outside, over zero and negative depths; no, one and a few valid tracks, clouds smaller
than K + 1, a base threshold that rejects every track.

Exact: ``valid``, the row counts after every stage, prepare_data's index lists and shifted times.

Floats against the reference.  Colours 1e-6 everywhere.  Points 2e-6 (test_oracle_golden.py's bound) where the
coordinates are of order 1 to 10, which is every item but three.  The point is ``X0 + (X1 - X0) * ratio``; in
``time/before`` and ``time/after`` (extrapolation, ratios down to -8 and -13) and in ``time/equal_stamps`` (two frames with
one time stamp: ratio 0.25 / 1e-8 = 2.5e7) the terms are far larger than the frames' points, and a last-bit
difference of X0 or X1 comes out multiplied by the ratio.  There the bound is a number of float32 ulps of S, the
largest magnitude in the expression: S = max |ratio| x 2.594, the ratios recomputed here from the fixture's times
and visibilities (``chosen_frames``) and 2.594 the largest coordinate of the same tracks interpolated inside the
window (item ``time/tie``).  Measured on the CPU, oracle against the reference fixture (this test prints every
item's figures, ``pytest -s``):
    time/before        S = 20.8     ulp(S) = 1.9e-6   max |d| = 1.91e-6 = 1.0 ulp(S)    bound 2 ulp(S) = 3.8e-6
    time/after         S = 33.7     ulp(S) = 3.8e-6   max |d| = 1.67e-6 = 0.4 ulp(S)    bound 1 ulp(S) = 3.8e-6
    time/equal_stamps  S = 6.5e7    ulp(S) = 4        max |d| = 6       = 1.5 ulp(S)    bound 3 ulp(S) = 12
Every other item: points at most 2.4e-7 (most are bit-identical), colours at most 1.2e-7.  The bounds leave room
for another summation order and nothing more; they are not tuned to any GPU output."""
import numpy as np
import pytest

from oracle import oracle as orc

FAMILIES = {
    "time": ["tie", "before", "after", "on_real", "equal_stamps", "offset"],
    "window": ["one_closest", "fwd_only", "bwd_only", "two_real", "n64"],
    "sample": ["p257", "p256", "p1"],
    "counts": [n + s for n in ("none_valid", "one_valid", "three_valid", "small_track", "small_track_k20", "small_base",
                               "reject_all", "keep_some", "keep_most") for s in ("", "_nb")],
}
ITEMS = [(f, i) for f, items in FAMILIES.items() for i in items]
IDS = [f"{f}-{i}" for f, i in ITEMS]
ATOL_PCL, ATOL_RGB = 2e-6, 1e-6
ULPS = {("time", "before"): 2, ("time", "after"): 1, ("time", "equal_stamps"): 3}  # of S, the expression's largest magnitude


def load_item(golden_dir, family, item):
    """an item's arrays; those it shares with the family's first item are stored once, under the first"""
    g = np.load(golden_dir / f"track_edges_{family}.npz")
    first = str(g["items"][0])
    assert item in g["items"].tolist()
    d = {k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(first + "__")}
    d.update({k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(item + "__")})
    return d


def chosen_frames(g):
    """per track: the two visible frames nearest in time to the target (lower index first among equals), the time
    ratio, and whether first / second place was tied -- from the fixture's shifted times, in float32"""
    t, tt = g["dfk_times"].astype(np.float32), np.float32(g["dfk_time_tgt"][0])
    d = np.where(g["vis"], np.abs(t - tt)[None, :], np.float32(np.inf))
    order = np.argsort(d, axis=1, kind="stable")
    f0, f1 = order[:, 0], order[:, 1]
    ds = np.take_along_axis(d, order, 1)
    ratio = (tt - t[f0]) / ((t[f1] - t[f0]) + np.float32(1e-8))
    tie_first = ds[:, 0] == ds[:, 1]
    tie_second = (ds[:, 1] == ds[:, 2]) & np.isfinite(ds[:, 2]) if d.shape[1] > 2 else np.zeros_like(tie_first)
    return f0, f1, ratio.astype(np.float32), tie_first, tie_second


def pcl_atol(golden_dir, family, item, g):
    """the bound on a point coordinate of this item (module docstring)"""
    if (family, item) not in ULPS:
        return ATOL_PCL
    x = np.abs(load_item(golden_dir, family, "tie")["ref_pcl_all"]).max()
    ratio = chosen_frames(g)[2][g["ref_valid"]]
    s = np.float32(np.abs(ratio).max() * x)
    return max(ATOL_PCL, ULPS[(family, item)] * float(np.spacing(s)))


def base_of(g):
    wb = bool(g["with_base"])
    return (g["base_pts"] if wb else None, g["base_rgb"] if wb else None, None if np.isnan(g["base_thres"]) else float(g["base_thres"]))


def _max(a, b):
    return float(np.abs(a - b).max()) if a.size else 0.0


def test_every_item_is_listed(golden_dir):
    for family, items in FAMILIES.items():
        assert np.load(golden_dir / f"track_edges_{family}.npz")["items"].tolist() == items


@pytest.mark.parametrize("family,item", ITEMS, ids=IDS)
def test_prepare_data(golden_dir, family, item):
    g = load_item(golden_dir, family, item)
    dft = orc.track_prepare_data({k[5:]: v for k, v in g.items() if k.startswith("data_")}, 0)
    assert np.array_equal(dft["times"], g["dfk_times"]) and np.array_equal(dft["time_tgt"], g["dfk_time_tgt"][0])
    closest, real = np.flatnonzero(dft["kind"] == 1), np.flatnonzero(dft["kind"] == 2)
    assert closest.tolist() == g["dfk_idx_closest"].tolist() and real.tolist() == g["dfk_idx_real"].tolist()
    assert real[real < closest[0]].tolist() == g["dfk_idx_real_fwd"].tolist()
    assert real[real > closest[-1]].tolist() == g["dfk_idx_real_bwd"].tolist()
    assert dft["rgbs"].shape[0] == dft["depths"].shape[0] == dft["flat_cams"].shape[0] == dft["times"].shape[0]


@pytest.mark.parametrize("family,item", ITEMS, ids=IDS)
def test_track_points_and_filters(golden_dir, family, item):
    g = load_item(golden_dir, family, item)
    dft = orc.track_prepare_data({k[5:]: v for k, v in g.items() if k.startswith("data_")}, 0)
    atol = pcl_atol(golden_dir, family, item, g)
    # per-track stage against the reference's unfiltered cloud and colours
    valid, pcl, rgb = orc.track_points(dft, g["tracks"], g["vis"])
    assert np.array_equal(valid, g["ref_valid"]) and int(valid.sum()) == int(g["n_valid"])
    assert pcl[valid].shape == g["ref_pcl_all"].shape == g["ref_rgb_all"].shape
    d_pcl, d_rgb = _max(pcl[valid], g["ref_pcl_all"]), _max(rgb[valid], g["ref_rgb_all"])
    print(f"\n{family}/{item}: max|d pcl| = {d_pcl:.3g}  max|d rgb| = {d_rgb:.3g}  bound {atol:.3g}")
    assert not np.any(pcl[~valid]) and not np.any(rgb[~valid])
    np.testing.assert_allclose(pcl[valid], g["ref_pcl_all"], rtol=0, atol=atol)
    np.testing.assert_allclose(rgb[valid], g["ref_rgb_all"], rtol=0, atol=ATOL_RGB)
    # the whole row: the same filter decisions at every stage, the same cloud
    bp, br, th = base_of(g)
    rc = dict(dyn_pcl_outlier_knn=int(g["knn"]), dyn_pcl_track_track2base_thres_mult=int(g["mult"]),
              dyn_pcl_outlier_std_thres=float(g["std_thres"]))
    o_pcl, o_rgb, info = orc.track_compute_pcl_for_tgt(dft, g["tracks"], g["vis"], rc, bp, br, th)
    n_t2b = info["avg_self"].shape[0] if "avg_self" in info else 0
    assert (int(info["valid"].sum()), n_t2b, info.get("n_track", 0)) == (int(g["n_valid"]), int(g["n_after_t2b"]), int(g["n_after_self"]))
    assert o_pcl.shape == g["out_pcl"].shape and o_rgb.shape == g["out_rgb"].shape
    np.testing.assert_allclose(o_pcl, g["out_pcl"], rtol=0, atol=atol)
    np.testing.assert_allclose(o_rgb, g["out_rgb"], rtol=0, atol=ATOL_RGB)


def nearest_depth(g):
    """per track and frame: the depth under the nearest sample (0 outside the frame), the kernel's formula"""
    n_fwd, n_close = int(g["data_n_actual_temporal_track_fwd2tgt"][0, 0]), int(g["data_n_actual_temporal"][0, 0])
    n_bwd = int(g["data_n_actual_temporal_track_bwd2tgt"][0, 0])
    depth = np.concatenate([g["data_depth_src_temporal_track_fwd2tgt"][0, :n_fwd], g["data_depth_src_temporal"][0, :n_close],
                            g["data_depth_src_temporal_track_bwd2tgt"][0, :n_bwd]])[..., 0]
    N, H, W = depth.shape
    f32 = np.float32
    u, v = g["tracks"][..., 0], g["tracks"][..., 1]
    nx = np.rint(((((f32(2) * u / f32(W) - f32(1)) + f32(1)) * f32(W) - f32(1)) / f32(2)))
    ny = np.rint(((((f32(2) * v / f32(H) - f32(1)) + f32(1)) * f32(H) - f32(1)) / f32(2)))
    inside = (nx >= 0) & (nx <= W - 1) & (ny >= 0) & (ny <= H - 1)
    xi, yi = np.where(inside, nx, 0).astype(int), np.where(inside, ny, 0).astype(int)
    return np.where(inside, depth[np.arange(N)[None, :], yi, xi], f32(0)), inside


def branch_counts(g):
    """how many valid tracks of an item take each branch (the figures of the pull request's description)"""
    f0, f1, ratio, tie1, tie2 = chosen_frames(g)
    v = g["ref_valid"]
    dep, inside = nearest_depth(g)
    rows = np.arange(v.size)
    d0, d1 = dep[rows, f0], dep[rows, f1]
    in0, in1 = inside[rows, f0], inside[rows, f1]
    return dict(valid=int(v.sum()), tie_first=int((v & tie1).sum()), tie_second=int((v & tie2).sum()),
                extrapolated=int((v & ((ratio < 0) | (ratio > 1))).sum()), ratio_zero=int((v & (ratio == 0)).sum()),
                zero_depth=int((v & (((d0 == 0) & in0) | ((d1 == 0) & in1))).sum()),
                negative_depth=int((v & ((d0 < 0) | (d1 < 0))).sum()), outside=int((v & (~in0 | ~in1)).sum()),
                after_t2b=int(g["n_after_t2b"]), after_self=int(g["n_after_self"]), out=int(g["out_pcl"].shape[0]))


def test_items_reach_their_edges(golden_dir):
    """the fixtures do what they claim (and the figures of every item, ``pytest -s``)"""
    c = {}
    for family, item in ITEMS:
        c[family, item] = branch_counts(load_item(golden_dir, family, item))
        print(f"\n{family}/{item}: {c[family, item]}")
    tie = c["time", "tie"]
    assert tie["tie_first"] >= 10 and tie["tie_second"] >= 10 and tie["extrapolated"] >= 10
    assert c["time", "before"]["extrapolated"] == c["time", "before"]["valid"] > 0
    assert c["time", "after"]["extrapolated"] == c["time", "after"]["valid"] > 0
    assert c["time", "on_real"]["ratio_zero"] >= 10
    g = load_item(golden_dir, "time", "equal_stamps")
    assert np.sum(np.abs(chosen_frames(g)[2][g["ref_valid"]]) > 1e7) >= 10 and np.abs(g["ref_pcl_all"]).max() > 1e6
    assert load_item(golden_dir, "time", "offset")["data_time_src_temporal"].min() > 1000
    for item in FAMILIES["sample"][:2]:
        s = c["sample", item]
        assert s["zero_depth"] >= 10 and s["negative_depth"] >= 10 and s["outside"] >= 30
    g = load_item(golden_dir, "sample", "p257")
    H, W = g["data_rgb_src_temporal"].shape[2:4]
    u, v = g["tracks"][..., 0], g["tracks"][..., 1]
    up, dn = (lambda x: np.nextafter(np.float32(x), np.float32(np.inf))), (lambda x: np.nextafter(np.float32(x), np.float32(-np.inf)))
    for x, arr in [(b, u) for b in (0, 0.5, W - 1, W, 7.5, -1)] + [(b, v) for b in (0, 0.5, H - 1, H, 7.5, -1)]:
        assert np.any(arr == np.float32(x)) and np.any(arr == up(x)) and np.any(arr == dn(x)), x
    assert np.any(np.abs(u) == 1e6) and np.any(np.abs(v) == 1e6) and np.all(np.abs(g["tracks"]) <= 1e6 + 1)
    assert [c["sample", i]["valid"] > 0 for i in FAMILIES["sample"]] == [True] * 3
    assert load_item(golden_dir, "window", "n64")["tracks"].shape[1] == 64
    assert c["counts", "none_valid"]["valid"] == 0 and c["counts", "one_valid"]["valid"] == 1
    assert (c["counts", "one_valid"]["out"], c["counts", "one_valid_nb"]["out"]) == (121, 0)  # NaN std drops the single point
    assert c["counts", "reject_all"]["after_t2b"] == 0 == c["counts", "reject_all"]["out"]
    ks = c["counts", "keep_some"]
    assert 0 < ks["after_self"] < ks["after_t2b"] < ks["valid"]
