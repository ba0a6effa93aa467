#!/usr/bin/env python3
"""Edge fixtures of the tracker-window branch, made by RUNNING THE REFERENCE ITSELF.

make_golden_track.py builds one window (2 + 2 + 1 frames, times 3..7, target 5.4) of smooth tracks that almost
all lie inside the image, with clouds of hundreds of points.  This generator runs the same two reference
functions, PGDVSDynamicTrackRenderer.prepare_data and .compute_pcl_for_tgt
(pgdvs/renderers/pgdvs_renderer_dyn_track.py:599-764, :98-396), on the CPU, on constructed inputs that meet the
branch's time, window, sampling and count edges, and writes ``track_edges_*.npz`` next to this script.  Like
make_golden_track.py it runs only in the build container, where the upstream tree is mounted read-only, under the
``sys.modules`` stubs of make_golden.py and with the tracker networks mocked; ``_save`` and the nearest-sample
flavour check (``_checked_grid_sample``: the CPU sampler and both CUDA flavours must pick the same depth pixel at
every track position, or the generator stops) come from make_golden_dyn_edges.py.  The fixtures are data only:
tests/test_oracle_track_edges.py replays them against oracle/ (CPU) and tests/test_gpu_track_edges.py against
the HIP path.

How the reference's intermediate values are reached without touching its code:
  * ``valid``: compute_pcl_for_tgt indexes its ``query_pts`` argument with the validity flags
    (``query_pts[flag_valid, :]``); the generator passes an object whose ``__getitem__`` records that key.
    (With no valid track the reference returns before it gets there: all flags are False.)
  * the unfiltered cloud: the ``knn_points`` stub records its arguments; the first call's first argument is
    ``pcl_track`` before any filter (``ref_pcl_all``).  ``torch.mean / median / std`` are wrapped while the
    reference runs, so the average distances and the statistics are the reference's own values
    (``ref_avg_t2b``, ``ref_avg_self``, ``ref_thres_*``), and the row counts after each stage follow from the
    later calls' arguments (``n_valid``, ``n_after_t2b``, ``n_after_self``).
  * the unfiltered colours: a second run of the same tracks against a one-point base cloud with threshold 1e30
    keeps every valid track through both filters (even a single one, whose unbiased std is NaN); its output
    without the appended base row is the per-track cloud and colour in track order (``ref_rgb_all``; the cloud
    must equal the recorded ``ref_pcl_all`` bit for bit).

Every filter decision is kept away from its threshold: the generator asserts that no recorded average distance
lies within a relative 1e-4 of the threshold it is compared with, so the tests may demand identical decisions.
Non-finite tracks and magnitudes beyond 1e6 are not here (their integer conversion is undefined in the
reference's sampler); tests/test_gpu_track_edges.py holds those against the oracle.

One file per family; an item holds the batch dict of prepare_data (``data_*``), what prepare_data returned
(``dfk_*``), the arguments of compute_pcl_for_tgt and the recorded values under ``<item>__<key>``; an item after
the first omits the arrays equal to the first item's.  Frames are 24 x 32 (8 x 12 for the 64-frame window);
colours are multiples of 1/256 so that the files stay small.
  track_edges_time     3 + 2 + 3 frames.  ``tie``: target on a time stamp (5.0) with real frames at 2,3,4 and 6,7,8:
                       ties for first and for second place; ``before`` / ``after``: target outside every time
                       stamp (extrapolation); ``on_real``: target on a visible real frame's time (ratio 0);
                       ``equal_stamps``: two real frames with one time stamp (ratio = (tt - t0) / 1e-8);
                       ``offset``: raw times 1000 + k.
  track_edges_window   ``one_closest`` (2 + 1 + 2), ``fwd_only`` (3 + 2 + 0), ``bwd_only`` (0 + 2 + 3), ``two_real``
                       (1 + 2 + 1), ``n64`` (31 + 2 + 31 at 8 x 12).  Each starts with rows visible in exactly two
                       real frames, in one real frame, in a closest frame only, in a closest frame and all real
                       ones, and nowhere.
  track_edges_sample   2 + 2 + 1 frames, P = 1, 256, 257: positions on integers and half-integers, at 0, W-1, H-1,
                       W, H and one float32 spacing either side of each, negative, up to +-1e6; depth maps with
                       zeros and negative values.
  track_edges_counts   no valid track, one valid track, track clouds and base clouds smaller than K + 1, a base
                       threshold that rejects every track, one that keeps some; every item with a base cloud
                       has a twin ``<item>_nb`` with base None and threshold None.

Two runs write byte-identical files (fixed seeds, one torch thread, fixed zip timestamps).

Usage:  python tests/golden/make_golden_track_edges.py
"""
import pathlib
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden_dyn_edges as DE  # noqa: E402
from make_golden import OUT, _flat_cam, _install_stubs, _pose  # noqa: E402

F32 = np.float32
T = torch.from_numpy
MULT, STD_THRES = 50, 0.1
KEYS = ("rgb", "dyn_mask", "depth", "flat_cam", "time")


# ---------------------------------------------------------------- windows
def _frames(rng, N, H, W, yaw_step=1.5, zero_depth=0.0, neg_depth=0.0):
    cams = np.stack([_flat_cam(H, W, 0.9 * W * (1 + 0.01 * (i % 7)), _pose(yaw_step * i - 3, 0.4 * (i % 9), [0.03 * (i % 11), 0.01 * (i % 5), 0.0]))
                     for i in range(N)]).astype(F32)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    depths = np.stack([(2.0 + 0.4 * np.sin(xx / W * 3 + i) + 0.2 * np.cos(yy / H * 2)).astype(F32) for i in range(N)])
    u = rng.random((N, H, W))
    depths[u < zero_depth] = 0.0
    neg = (u >= zero_depth) & (u < zero_depth + neg_depth)
    depths[neg] = -depths[neg]
    rgbs = (rng.integers(0, 256, (N, H, W, 3)) / 256.0).astype(F32)
    masks = (rng.random((N, H, W, 1)) < 0.2).astype(F32)
    return dict(rgb=rgbs, dyn_mask=masks, depth=depths[..., None], flat_cam=cams)


def _batch(frames, counts, times, time_tgt, pad_side):
    """the batch dict PGDVSDynamicTrackRenderer.prepare_data consumes (B = 1, each side padded to pad_side)"""
    n_fwd, n_close, n_bwd = counts

    def pad(a, n):
        return np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:], a.dtype)], 0)[None]

    arrs = dict(frames, time=np.asarray(times, F32))
    data = {"n_actual_temporal_track_fwd2tgt": np.array([[n_fwd]]), "n_actual_temporal": np.array([[n_close]]),
            "n_actual_temporal_track_bwd2tgt": np.array([[n_bwd]]), "time_tgt": np.array([[time_tgt]], F32)}
    for key in KEYS:
        a = arrs[key]
        data[f"{key}_src_temporal_track_fwd2tgt"] = pad(a[:n_fwd], pad_side)
        data[f"{key}_src_temporal"] = pad(a[n_fwd:n_fwd + n_close], 2)
        data[f"{key}_src_temporal_track_bwd2tgt"] = pad(a[n_fwd + n_close:], pad_side)
    return data


def _smooth_tracks(rng, n_pt, N, H, W, drift=0.6):
    start = np.stack([rng.uniform(1.0, W - 6.0, n_pt), rng.uniform(1.0, H - 4.0, n_pt)], -1)
    d = rng.normal(size=(n_pt, 1, 2)) * 0.25 * drift + np.array([drift, drift / 2])
    return (start[:, None] + d * np.arange(N)[None, :, None] + rng.normal(size=(n_pt, N, 2)) * 0.2).astype(F32)


def _vis(rng, n_pt, counts, p_real=0.7, p_close=0.15):
    n_fwd, n_close, n_bwd = counts
    N = sum(counts)
    vis = rng.random((n_pt, N)) < p_real
    vis[:, n_fwd:n_fwd + n_close] = rng.random((n_pt, n_close)) < p_close
    return vis


def _base(rng, n):
    pts = (rng.normal(size=(n, 3)) * np.array([0.6, 0.4, 0.3]) + np.array([0.0, 0.0, 2.2])).astype(F32)
    return pts, rng.random((n, 3), dtype=F32)


# ---------------------------------------------------------------- reference calls
class _QueryProbe:
    """stands in for ``query_pts``: records the boolean key the reference indexes it with (its ``flag_valid``)"""

    def __init__(self, q):
        self.q, self.key = q, None

    def __getitem__(self, key):
        self.key = key[0].clone()
        return self.q[key]


class Ref:
    def __init__(self):
        for m in ("pgdvs.models.tapnet", "pgdvs.models.tapnet.interface", "pgdvs.models.cotracker", "pgdvs.models.cotracker.interface"):
            sys.modules[m] = MagicMock()
        import pgdvs.renderers.pgdvs_renderer_dyn_track as RT

        self.RT = RT
        self.renderer = RT.PGDVSDynamicTrackRenderer.__new__(RT.PGDVSDynamicTrackRenderer)
        torch.nn.Module.__init__(self.renderer)

    def prepare(self, data, n_views):
        return self.renderer.prepare_data(0, {k: T(np.asarray(v)) for k, v in data.items()}, n_views, "cpu")

    def _run(self, dfk, tracks, vis, query, knn, std_thres, base_pts, base_rgb, base_thres):
        """compute_pcl_for_tgt with knn_points, torch.mean / median / std recording what they return"""
        ev = []
        ops_mod = self.RT.p3d_ops
        real = dict(knn=ops_mod.knn_points, mean=torch.mean, median=torch.median, std=torch.std)

        def knn_points(p1, p2, K, **kw):
            r = real["knn"](p1, p2, K, **kw)
            ev.append(("knn", p1[0].clone(), p2[0].clone(), r[0][0].clone()))
            return r

        def wrap(name):
            def f(x, *a, **k):
                r = real[name](x, *a, **k)
                ev.append((name, tuple(x.shape), r.clone()))
                return r
            return f

        probe = _QueryProbe(T(query))
        base = {"pcl": None if base_pts is None else T(base_pts), "pcl_rgbs": None if base_rgb is None else T(base_rgb),
                "pcl_nn_dist_thres": None if base_thres is None else torch.tensor(base_thres, dtype=torch.float32)}
        rc = types.SimpleNamespace(dyn_pcl_outlier_knn=knn, dyn_pcl_track_track2base_thres_mult=MULT, dyn_pcl_outlier_std_thres=std_thres)
        ops_mod.knn_points, torch.mean, torch.median, torch.std = knn_points, wrap("mean"), wrap("median"), wrap("std")
        try:
            pcl, rgb = self.renderer.compute_pcl_for_tgt(data_for_track=dfk, query_pts=probe, tracks=T(tracks), track_visibles=T(vis),
                                                         render_cfg=rc, base_pcl_info=base, device="cpu")
        finally:
            ops_mod.knn_points, torch.mean, torch.median, torch.std = real["knn"], real["mean"], real["median"], real["std"]
        valid = np.zeros(tracks.shape[0], bool) if probe.key is None else probe.key.numpy().astype(bool)
        return pcl.numpy(), rgb.numpy(), valid, ev

    def item(self, data, dfk, tracks, vis, knn, *, std_thres=STD_THRES, base=None, base_thres=None, rng=None):
        P, N = tracks.shape[:2]
        query = np.concatenate([rng.integers(0, N, (P, 1)), tracks[:, 0, ::-1]], 1).astype(F32)
        base_pts, base_rgb = base if base is not None else (None, None)
        with_base = base_pts is not None
        pcl, rgb, valid, ev = self._run(dfk, tracks, vis, query, knn, std_thres, base_pts, base_rgb, base_thres)
        n_valid = int(valid.sum())
        knns = [i for i, e in enumerate(ev) if e[0] == "knn"]

        def avg_after(i):  # the reference's mean over the distances of knn call i
            e = next(e for e in ev[i + 1:] if e[0] == "mean" and len(e[1]) == 2)
            return e[2].numpy()

        def far_enough(avg, thres):
            if np.isfinite(thres):
                assert np.all(np.abs(avg - thres) > 1e-4 * abs(thres)), "a filter decision within 1e-4 of its threshold"

        rec = dict(ref_valid=valid, n_valid=n_valid, n_after_t2b=n_valid, n_after_self=n_valid if n_valid else 0,
                   ref_pcl_all=np.zeros((0, 3), F32), ref_avg_t2b=np.zeros(0, F32), ref_thres_t2b=F32(np.nan),
                   ref_avg_self=np.zeros(0, F32), ref_thres_self=F32(np.nan))
        if n_valid:
            assert knns, "a non-empty track cloud meets a filter"
            rec["ref_pcl_all"] = ev[knns[0]][1].numpy()
            assert rec["ref_pcl_all"].shape[0] == n_valid
            k_self = 0
            if with_base:
                rec["ref_avg_t2b"] = avg_after(knns[0])
                rec["ref_thres_t2b"] = (torch.tensor(base_thres, dtype=torch.float32) * MULT).numpy()
                far_enough(rec["ref_avg_t2b"], float(rec["ref_thres_t2b"]))
                k_self = 1
                rec["n_after_t2b"] = ev[knns[1]][1].shape[0] if len(knns) > 1 else 0
            if len(knns) > k_self:
                i = knns[k_self]
                rec["ref_avg_self"] = avg_after(i)
                med = next(e for e in ev[i + 1:] if e[0] == "median")[2]
                std = next(e for e in ev[i + 1:] if e[0] == "std")[2]
                th = torch.tensor(base_thres, dtype=torch.float32) if base_thres is not None else med + std * std_thres
                rec["ref_thres_self"] = th.numpy()
                far_enough(rec["ref_avg_self"], float(th))
        else:
            assert not ev and pcl.shape[0] == 0
        n_app = base_pts.shape[0] if with_base and pcl.shape[0] > 0 else 0
        rec["n_after_self"] = pcl.shape[0] - n_app
        # the unfiltered colours: the same tracks against a one-point base with a threshold nothing reaches
        rgb_all = np.zeros((0, 3), F32)
        if n_valid:
            far = (np.array([[0.0, 0.0, 2.0]], F32), np.array([[0.5, 0.5, 0.5]], F32))
            k_pcl, k_rgb, k_valid, _ = self._run(dfk, tracks, vis, query, knn, std_thres, far[0], far[1], 1e30)
            assert np.array_equal(k_valid, valid) and k_pcl.shape[0] == n_valid + 1, "the keep-all run dropped a track"
            assert np.array_equal(k_pcl[:-1].view(np.uint32), rec["ref_pcl_all"].view(np.uint32))
            rgb_all = k_rgb[:-1]
        out = {"data_" + k: np.asarray(v) for k, v in data.items()}
        out.update(
            dfk_times=dfk["time_for_track"].numpy(), dfk_time_tgt=dfk["time_tgt"].numpy(),
            dfk_idx_closest=np.array(dfk["idx_temporal_closest"], np.int64), dfk_idx_real=np.array(dfk["idx_real_track"], np.int64),
            dfk_idx_real_fwd=np.array(dfk["idx_real_track_fwd"], np.int64), dfk_idx_real_bwd=np.array(dfk["idx_real_track_bwd"], np.int64),
            tracks=tracks, vis=vis, query=query, knn=knn, std_thres=F32(std_thres), mult=MULT, with_base=with_base,
            base_thres=F32(np.nan if base_thres is None else base_thres),
            base_pts=np.zeros((0, 3), F32) if base_pts is None else base_pts,
            base_rgb=np.zeros((0, 3), F32) if base_rgb is None else base_rgb,
            ref_rgb_all=rgb_all, out_pcl=pcl, out_rgb=rgb, **rec)
        return out


def _write_family(name, items):
    """an item stores only the arrays that differ from the first item's (the tests merge them back)"""
    arrays = {"items": np.array(list(items))}
    first = next(iter(items.values()))
    for j, (item, d) in enumerate(items.items()):
        for k, v in d.items():
            v, f = np.asarray(v), np.asarray(first[k])
            if j == 0 or not (v.dtype == f.dtype and v.shape == f.shape and np.array_equal(v, f, equal_nan=v.dtype.kind == "f")):
                arrays[f"{item}__{k}"] = v
    DE._save(OUT / f"track_edges_{name}.npz", arrays)


def _show(name, items):
    for item, d in items.items():
        print(f"  {name:7s}{item:22s} P {d['tracks'].shape[0]:4d}  valid {d['n_valid']:4d}  after track-to-base {d['n_after_t2b']:4d}"
              f"  after filter {d['n_after_self']:4d}  out {d['out_pcl'].shape[0]:4d}")


# ---------------------------------------------------------------- families
def family_time(ref):
    rng = np.random.default_rng(1701)
    H, W, counts = 24, 32, (3, 2, 3)
    frames = _frames(rng, 8, H, W)
    tracks = _smooth_tracks(rng, 220, 8, H, W, drift=0.4)
    vis = _vis(rng, 220, counts, p_real=0.55, p_close=0.08)
    stamps = np.array([2, 3, 4, 5, 6, 6, 7, 8], F32)  # closest frames at 5 and 6; the real frame at 6 is another frame
    items = {}
    for name, times, tt in (("tie", stamps, 5.0), ("before", stamps, -6.0), ("after", stamps, 20.0), ("on_real", stamps, 3.0),
                            ("equal_stamps", np.array([2, 3, 3, 5, 6, 6, 7, 7], F32), 3.25),
                            ("offset", stamps + F32(1000), 1005.4)):
        data = _batch(frames, counts, times, tt, 3)
        dfk = ref.prepare(data, 8)
        assert dfk["idx_temporal_closest"] == [3, 4] and dfk["idx_real_track"] == [0, 1, 2, 5, 6, 7]
        items[name] = ref.item(data, dfk, tracks, vis, 5, std_thres=1e6, rng=np.random.default_rng(5))
        assert items[name]["n_after_self"] == items[name]["n_valid"] > 60
    _show("time", items)
    _write_family("time", items)


def _crafted_vis(vis, counts):
    """rows 0..: visible in exactly two real frames (first two, first and last, last two), in one real frame, in a
    closest frame only, in a closest frame and every real one, nowhere"""
    n_fwd, n_close, n_bwd = counts
    real = [i for i in range(sum(counts)) if not n_fwd <= i < n_fwd + n_close]
    rows = [[real[0], real[1]], [real[0], real[-1]], [real[-2], real[-1]], [real[0]], [real[-1]], [n_fwd], [n_fwd] + real, []]
    for r, on in enumerate(rows):
        vis[r] = False
        vis[r, on] = True
    return len(rows)


def family_window(ref):
    rng = np.random.default_rng(1702)
    items = {}
    for name, counts, (H, W), n_pt, pad_side in (("one_closest", (2, 1, 2), (24, 32), 150, 3), ("fwd_only", (3, 2, 0), (24, 32), 150, 3),
                                                 ("bwd_only", (0, 2, 3), (24, 32), 150, 3), ("two_real", (1, 2, 1), (24, 32), 150, 3),
                                                 ("n64", (31, 2, 31), (8, 12), 150, 31)):
        N = sum(counts)
        frames = _frames(rng, N, H, W, yaw_step=1.5 if N < 10 else 0.1)
        times = (3.0 + np.arange(N)).astype(F32)
        tt = float(times[counts[0]]) + 0.4  # between the closest frames (past the only one)
        data = _batch(frames, counts, times, tt, pad_side)
        dfk = ref.prepare(data, 2 * pad_side + 2)
        assert len(dfk["idx_temporal_closest"]) == counts[1] and len(dfk["idx_real_track"]) == counts[0] + counts[2]
        tracks = _smooth_tracks(rng, n_pt, N, H, W, drift=0.6 if N < 10 else 0.03)
        vis = _vis(rng, n_pt, counts, p_real=0.7 if N < 10 else 0.12, p_close=0.1)
        n_crafted = _crafted_vis(vis, counts)
        items[name] = it = ref.item(data, dfk, tracks, vis, 5, std_thres=1e6, rng=np.random.default_rng(6))
        assert it["ref_valid"][:n_crafted].tolist() == [True, True, True, False, False, False, False, False]
        assert it["n_after_self"] == it["n_valid"] > 30
    _show("window", items)
    _write_family("window", items)


def _edge_values(size):
    """coordinates along an axis of ``size`` pixels: integers, halves, the borders, one float32 spacing either side
    of each, negatives and magnitudes up to 1e6"""
    base = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 7.0, 7.5, size / 2.0, size / 2.0 - 0.5, size - 2.0, size - 1.5, size - 1.0, size - 0.5,
            float(size), size + 0.5, size + 1.0, -0.5, -1.0, -1.5, -3.25, 1e3, -1e3, 65536.0, 1e6, -1e6]
    vals = []
    for b in base:
        b = F32(b)
        vals += [b, np.nextafter(b, F32(np.inf)), np.nextafter(b, F32(-np.inf))]
    return np.array(vals, F32)


def family_sample(ref):
    rng = np.random.default_rng(1703)
    H, W, counts = 24, 32, (2, 2, 1)
    frames = _frames(rng, 5, H, W, zero_depth=0.15, neg_depth=0.1)
    data = _batch(frames, counts, [3, 4, 5, 6, 7], 5.4, 3)
    dfk = ref.prepare(data, 8)
    xs, ys = _edge_values(W), _edge_values(H)
    items = {}
    for name, P in (("p257", 257), ("p256", 256), ("p1", 1)):
        # every x edge value at least once per frame; two thirds of the positions pair an edge with an interior
        # coordinate (so that the other axis decides), the rest pair two edges
        tr = np.empty((P, 5, 2), F32)
        for f in range(5):
            ix = (np.arange(P) * 7 + 11 * f) % xs.size
            iy = (np.arange(P) * 5 + 3 * f) % ys.size
            tr[:, f, 0], tr[:, f, 1] = xs[ix], ys[iy]
            inner = rng.random(P)
            rx, ry = rng.uniform(0, W - 1, P).astype(F32), rng.uniform(0, H - 1, P).astype(F32)
            tr[:, f, 0] = np.where(inner < 1 / 3, rx, tr[:, f, 0])
            tr[:, f, 1] = np.where((inner >= 1 / 3) & (inner < 2 / 3), ry, tr[:, f, 1])
        vis = _vis(rng, P, counts, p_real=0.9, p_close=0.0)
        if P == 1:
            tr[0, :, 0], tr[0, :, 1] = [W - 1, 0.5, 3, 4, np.nextafter(F32(W - 1), F32(np.inf))], [H - 1, 11.5, 2, 2, 7.5]
            vis[0] = [True, True, False, False, True]
        items[name] = it = ref.item(data, dfk, tr, vis, 5, std_thres=1e6, rng=np.random.default_rng(7))
        # (a single point has no unbiased std: the filter of the main run drops it, the keep-all run records it)
        assert it["n_valid"] >= min(P, 200) and it["n_after_self"] == (it["n_valid"] if P > 1 else 0)
    _show("sample", items)
    _write_family("sample", items)


def family_counts(ref):
    rng = np.random.default_rng(1704)
    H, W, counts = 24, 32, (2, 2, 1)
    frames = _frames(rng, 5, H, W)
    data = _batch(frames, counts, [3, 4, 5, 6, 7], 5.4, 3)
    dfk = ref.prepare(data, 8)
    assert dfk["idx_temporal_closest"] == [2, 3] and dfk["idx_real_track"] == [0, 1, 4]
    tracks = _smooth_tracks(rng, 400, 5, H, W)
    vis = _vis(rng, 400, counts)
    n_ok = np.flatnonzero(~vis[:, 2:4].any(1) & (vis[:, [0, 1, 4]].sum(1) >= 2))
    assert n_ok.size > 40

    def only(n):  # the same tracks with all but n valid ones made visible in a closest frame
        v = vis.copy()
        v[n_ok[n:], 2] = True
        return v

    base120, base3 = _base(rng, 120), _base(rng, 3)
    # a base cloud around one corner of the track cloud (the reference's own unfiltered points): the tracks of the
    # opposite corner are further from it than 50 thresholds
    cloud = ref.item(data, dfk, tracks, vis, 6, rng=np.random.default_rng(8))["ref_pcl_all"]
    corner = cloud[np.argmin(cloud[:, 0] + cloud[:, 1])]
    base_corner = ((corner + rng.normal(size=(120, 3)) * 0.1).astype(F32), rng.random((120, 3), dtype=F32))
    plan = {  # item: (vis, K, base, base threshold)
        "none_valid": (only(0), 6, base120, 0.03),
        "one_valid": (only(1), 6, base120, 0.03),
        "three_valid": (only(3), 6, base120, 0.03),
        "small_track": (only(4), 6, base120, 0.03),       # fewer than K + 1 track points
        "small_track_k20": (only(17), 20, base120, 0.03),
        "small_base": (vis, 6, base3, 0.03),              # fewer than K + 1 base points
        "reject_all": (vis, 6, base120, 1e-7),            # no track within 50 x 1e-7 of the base
        "keep_some": (vis, 4, base_corner, 0.05),
        "keep_most": (vis, 6, base120, 0.03),
    }
    items = {}
    for name, (v, K, base, th) in plan.items():
        items[name] = ref.item(data, dfk, tracks, v, K, base=base, base_thres=th, rng=np.random.default_rng(8))
        items[name + "_nb"] = ref.item(data, dfk, tracks, v, K, rng=np.random.default_rng(8))
    _show("counts", items)
    assert items["none_valid"]["out_pcl"].shape[0] == 0 and items["one_valid_nb"]["out_pcl"].shape[0] == 0
    assert items["reject_all"]["n_after_t2b"] == 0 and items["reject_all"]["out_pcl"].shape[0] == 0
    assert 0 < items["keep_some"]["n_after_t2b"] < items["keep_some"]["n_valid"]
    assert 0 < items["keep_some"]["n_after_self"] < items["keep_some"]["n_after_t2b"]
    _write_family("counts", items)


def main():
    torch.set_num_threads(1)
    _install_stubs()
    torch.nn.functional.grid_sample = DE._checked_grid_sample
    ref = Ref()
    for family in (family_time, family_window, family_sample, family_counts):
        family(ref)
    print(f"nearest samples checked against both CUDA flavours: {DE._nearest_checked[0]}")
    total = 0
    for f in sorted(OUT.glob("track_edges_*.npz")):
        total += f.stat().st_size
        print(f"  {f.name:28s} {f.stat().st_size / 1024:8.1f} KiB")
    print(f"  {'total':28s} {total / 1024:8.1f} KiB")


if __name__ == "__main__":
    main()
