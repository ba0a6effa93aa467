"""GPU (MI355X): the tracker-window branch at its time, window, sampling and count edges -- ``track_points_kernel``
and the chain compaction -> gather_rows -> knn_cross_mean_dist -> threshold_flags -> knn_mean_dist -> outlier_flags ->
threshold_flags -> concat_rows -- against the reference's fixtures (tests/golden/make_golden_track_edges.py) and the
oracle.  Per-track outputs are bit-exact against the oracle (same operation order) and within the bounds of
tests/test_oracle_track_edges.py against the reference; the filters must take the reference's decisions at every
item (no decision of a fixture is within 1e-4 of its threshold).  ``threshold_flags``, ``concat_rows`` and
``gather_rows`` are also held directly against numpy, once past their grid caps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402  (checker only)
from pgdvs_amd import _lib, ops  # noqa: E402
from pgdvs_amd.instantiate import load_config  # noqa: E402
from test_oracle_track_edges import ATOL_RGB, IDS, ITEMS, base_of, load_item, pcl_atol  # noqa: E402

DEV = "cuda:0"
BASE_ITEMS = [(f, i) for f, i in ITEMS if f == "counts" and not i.endswith("_nb")]
GUARD = 12345.5


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def I32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()  # fails loudly if the HIP extension is missing


def _renderer(g):
    from pgdvs_amd.renderers.pgdvs_renderer_dyn_track import PGDVSDynamicTrackRenderer

    cfg = load_config(static_renderer="gnt")
    rc = cfg.engine.engine_cfg.render_cfg
    rc["dyn_pcl_outlier_knn"], rc["dyn_pcl_track_track2base_thres_mult"] = int(g["knn"]), int(g["mult"])
    rc["dyn_pcl_outlier_std_thres"] = float(g["std_thres"])
    return PGDVSDynamicTrackRenderer(cfg=cfg, use_tracker=True).to(DEV), rc


def _window(g):
    raw = {k[5:]: v for k, v in g.items() if k.startswith("data_")}
    rend, rc = _renderer(g)
    n_views = 2 * raw["rgb_src_temporal_track_fwd2tgt"].shape[1] + 2
    return rend, rc, rend.prepare_data(0, {k: T(v) for k, v in raw.items()}, n_views, DEV), orc.track_prepare_data(raw, 0)


def _track_points(dft, tracks, vis):
    return ops.track_points(T(tracks), T(vis), dft["frame_kind"], dft["time_for_track_raw"], dft["time_tgt_raw"],
                            dft["rgbs_for_track"][: dft["n_actual_frames"]], dft["depths_for_track"][..., 0], dft["cams_for_track"])


def _base(g, pad=0, count=None, fill=1.5):
    """base_pcl_info of an item; ``pad`` junk rows after the cloud and a device count make it a capacity-sized buffer"""
    bp, br, th = base_of(g)
    info = {"pcl": None, "pcl_rgbs": None, "pcl_nn_dist_thres": None if th is None else T(np.array([th], np.float32))}
    if bp is not None:
        junk = np.full((pad, 3), fill, np.float32)
        info["pcl"], info["pcl_rgbs"] = T(np.concatenate([bp, junk])), T(np.concatenate([br, junk * 0.5]))
        if pad or count is not None:
            info["n_pts"] = I32(bp.shape[0] if count is None else count)
    return info


def _compute(rend, rc, dft, g, base, **kw):
    return rend.compute_pcl_for_tgt(data_for_track=dft, query_pts=T(g["query"]), tracks=T(g["tracks"]), track_visibles=T(g["vis"]),
                                    render_cfg=rc, base_pcl_info=base, device=DEV, **kw)


# ---------------------------------------------------------------- the fixture items
@pytest.mark.parametrize("family,item", ITEMS, ids=IDS)
def test_track_points_items(golden_dir, family, item):
    g = load_item(golden_dir, family, item)
    rend, rc, dft, odft = _window(g)
    assert dft["idx_temporal_closest"] == g["dfk_idx_closest"].tolist() and dft["idx_real_track"] == g["dfk_idx_real"].tolist()
    assert dft["idx_real_track_fwd"] == g["dfk_idx_real_fwd"].tolist() and dft["idx_real_track_bwd"] == g["dfk_idx_real_bwd"].tolist()
    assert np.array_equal(N(dft["time_for_track"]), g["dfk_times"]) and np.array_equal(N(dft["time_tgt"]), g["dfk_time_tgt"])
    valid, pcl, rgb = (N(t) for t in _track_points(dft, g["tracks"], g["vis"]))
    valid = valid.astype(bool)
    assert np.array_equal(valid, g["ref_valid"])
    o_valid, o_pcl, o_rgb = orc.track_points(odft, g["tracks"], g["vis"])
    assert np.array_equal(valid, o_valid)
    assert np.array_equal(bits(pcl), bits(o_pcl)) and np.array_equal(bits(rgb), bits(o_rgb))  # same operation order
    np.testing.assert_allclose(pcl[valid], g["ref_pcl_all"], rtol=0, atol=pcl_atol(golden_dir, family, item, g))
    np.testing.assert_allclose(rgb[valid], g["ref_rgb_all"], rtol=0, atol=ATOL_RGB)


@pytest.mark.parametrize("family,item", ITEMS, ids=IDS)
def test_compute_pcl_for_tgt_items(golden_dir, family, item):
    g = load_item(golden_dir, family, item)
    rend, rc, dft, _ = _window(g)
    atol = pcl_atol(golden_dir, family, item, g)
    pcl, rgb = _compute(rend, rc, dft, g, _base(g))
    assert tuple(pcl.shape) == g["out_pcl"].shape and tuple(rgb.shape) == g["out_rgb"].shape  # the reference's decisions
    np.testing.assert_allclose(N(pcl), g["out_pcl"], rtol=0, atol=atol)
    np.testing.assert_allclose(N(rgb), g["out_rgb"], rtol=0, atol=ATOL_RGB)
    pcl_c, rgb_c, n = _compute(rend, rc, dft, g, _base(g), return_count=True)
    n = int(n.item())
    assert n == g["out_pcl"].shape[0] and pcl_c.shape[0] >= n and rgb_c.shape[0] >= n
    assert torch.equal(pcl_c[:n], pcl) and torch.equal(rgb_c[:n], rgb)


@pytest.mark.parametrize("family,item", BASE_ITEMS, ids=[f"{f}-{i}" for f, i in BASE_ITEMS])
def test_base_cloud_as_capacity_buffer(golden_dir, family, item):
    g = load_item(golden_dir, family, item)
    twin = load_item(golden_dir, family, item + "_nb")
    assert np.array_equal(twin["tracks"], g["tracks"]) and np.array_equal(twin["vis"], g["vis"]) and not bool(twin["with_base"])
    rend, rc, dft, _ = _window(g)
    pcl, rgb = _compute(rend, rc, dft, g, _base(g))
    # junk rows beyond the device count change nothing
    pcl2, rgb2 = _compute(rend, rc, dft, g, _base(g, pad=50))
    assert torch.equal(pcl2, pcl) and torch.equal(rgb2, rgb)
    # a device count of 0: no base cloud at all -- the twin item's result, not an appended base, whatever the buffer holds
    outs = []
    for fill in (1.5, -7.25):
        p0, r0, n0 = _compute(rend, rc, dft, g, _base(g, pad=9, count=0, fill=fill), return_count=True)
        n0 = int(n0.item())
        assert n0 == twin["out_pcl"].shape[0]
        outs.append((p0[:n0], r0[:n0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    np.testing.assert_allclose(N(outs[0][0]), twin["out_pcl"], rtol=0, atol=pcl_atol(golden_dir, family, item + "_nb", twin))
    np.testing.assert_allclose(N(outs[0][1]), twin["out_rgb"], rtol=0, atol=ATOL_RGB)
    pcl_nb, rgb_nb = _compute(rend, rc, dft, twin, _base(twin))
    assert torch.equal(outs[0][0], pcl_nb) and torch.equal(outs[0][1], rgb_nb)


# ---------------------------------------------------------------- outside the fixtures
@pytest.mark.parametrize("with_base", [False, True])
def test_no_tracks_gives_empty_clouds(golden_dir, with_base):
    g = load_item(golden_dir, "counts", "keep_most" if with_base else "keep_most_nb")
    rend, rc, dft, _ = _window(g)
    g0 = dict(g, tracks=g["tracks"][:0], vis=g["vis"][:0], query=g["query"][:0])
    valid, pcl_all, rgb_all = _track_points(dft, g0["tracks"], g0["vis"])
    assert valid.shape == (0,) and pcl_all.shape == (0, 3) and rgb_all.shape == (0, 3)
    pcl, rgb = _compute(rend, rc, dft, g0, _base(g))
    assert pcl.shape == (0, 3) and rgb.shape == (0, 3)
    _, _, n = _compute(rend, rc, dft, g0, _base(g), return_count=True)
    assert int(n.item()) == 0


def test_65_frames_raise_and_launch_nothing():
    P, NF, H, W = 4, 65, 8, 12
    tracks, vis = torch.zeros((P, NF, 2), device=DEV), torch.ones((P, NF), dtype=torch.bool, device=DEV)
    times, rgbs = torch.arange(NF, dtype=torch.float32, device=DEV), torch.zeros((NF, H, W, 3), device=DEV)
    with pytest.raises(_lib.PgdvsHipError, match="at most 64 frames"):
        ops.track_points(tracks, vis, [2] * NF, times, times[:1], rgbs, rgbs[..., 0], torch.zeros((NF, _lib.CAM_BLOCK), device=DEV))
    lib = _lib.load()
    valid = torch.full((P + 16,), 7, dtype=torch.uint8, device=DEV)
    out = torch.full((2, P + 8, 3), GUARD, device=DEV)
    kind = (_lib.C.c_uint8 * NF)(*([2] * NF))
    cams = torch.zeros((NF, _lib.CAM_BLOCK), device=DEV)
    rc = lib.pgdvs_track_points(tracks.data_ptr(), vis.view(torch.uint8).data_ptr(), P, NF, _lib.C.cast(kind, _lib.C.c_void_p),
                                times.data_ptr(), times.data_ptr(), rgbs.data_ptr(), rgbs.data_ptr(), H, W, cams.data_ptr(),
                                valid.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), ops._stream())
    assert rc == -1 and b"bad shape" in lib.pgdvs_last_error()
    torch.cuda.synchronize()
    assert (N(valid) == 7).all() and (N(out) == GUARD).all()


def test_non_finite_and_huge_tracks(golden_dir):
    """NaN, +-inf and 1e30 positions scattered through an item: those rows equal the oracle's, every other row is
    untouched, and nothing is written outside the outputs (guard words on both sides)"""
    g = load_item(golden_dir, "sample", "p257")
    rend, rc, dft, odft = _window(g)
    clean = [N(t) for t in _track_points(dft, g["tracks"], g["vis"])]
    tracks = g["tracks"].copy()
    bad = [(3, 1, 0, np.nan), (18, 1, 1, np.nan), (40, 4, 0, np.inf), (41, 1, 1, -np.inf), (99, 1, 0, 1e30), (100, 4, 1, -1e30),
           (200, 4, 0, np.inf), (200, 4, 1, np.nan), (255, 1, 0, 3e38), (256, 4, 0, -np.inf)]  # (track, frame, axis, value)
    for p, f, c, val in bad:
        tracks[p, f, c] = val
    rows = sorted({p for p, *_ in bad})
    P, NF = tracks.shape[:2]
    H, W = dft["rgbs_for_track"].shape[1:3]
    lib = _lib.load()
    G = 64  # guard words on both sides of every output
    valid = torch.full((P + 2 * G,), 7, dtype=torch.uint8, device=DEV)
    pcl = torch.full((P * 3 + 2 * G,), GUARD, device=DEV)
    rgb = torch.full((P * 3 + 2 * G,), GUARD, device=DEV)
    t_tracks, t_vis = T(tracks), T(g["vis"]).view(torch.uint8)
    kind = (_lib.C.c_uint8 * NF)(*[int(k) for k in dft["frame_kind"]])
    rgbs, depths = dft["rgbs_for_track"][:NF].contiguous(), dft["depths_for_track"][..., 0].contiguous()
    rc_ = lib.pgdvs_track_points(t_tracks.data_ptr(), t_vis.data_ptr(), P, NF, _lib.C.cast(kind, _lib.C.c_void_p),
                                 dft["time_for_track_raw"].data_ptr(), dft["time_tgt_raw"].data_ptr(), rgbs.data_ptr(), depths.data_ptr(),
                                 H, W, dft["cams_for_track"].data_ptr(), valid.data_ptr() + G, pcl.data_ptr() + 4 * G,
                                 rgb.data_ptr() + 4 * G, ops._stream())
    assert rc_ == 0
    torch.cuda.synchronize()
    valid, pcl, rgb = N(valid), N(pcl), N(rgb)
    for buf, guard in ((valid, 7), (pcl, GUARD), (rgb, GUARD)):
        assert (buf[:G] == guard).all() and (buf[-G:] == guard).all()
    valid, pcl, rgb = valid[G:-G], pcl[G:-G].reshape(P, 3), rgb[G:-G].reshape(P, 3)
    o_valid, o_pcl, o_rgb = orc.track_points(odft, tracks, g["vis"])
    assert np.array_equal(valid.astype(bool), o_valid)
    for got, want in ((pcl[rows], o_pcl[rows]), (rgb[rows], o_rgb[rows])):  # bit for bit; a NaN's sign and payload are not pinned
        assert np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    # the altered positions are sampled: most of these rows are valid tracks that chose the altered frame
    assert np.sum((bits(o_pcl[rows]) != bits(clean[1][rows])).any(1) | (bits(o_rgb[rows]) != bits(clean[2][rows])).any(1)) >= 6
    others = np.setdiff1d(np.arange(P), rows)
    assert np.array_equal(valid[others], clean[0][others])
    assert np.array_equal(bits(pcl[others]), bits(clean[1][others])) and np.array_equal(bits(rgb[others]), bits(clean[2][others]))


# ---------------------------------------------------------------- the small ops, directly
def _guarded(n, dtype, guard):
    buf = torch.full((n + 64,), guard, dtype=dtype, device=DEV)
    return buf, buf[:n]


@pytest.mark.parametrize("cap", [1, 300, 262145 + 300])
def test_threshold_flags_direct(cap):
    """flag[i] = avg[i] < thres * mult for i < count, 0 beyond; a gate count of 0 switches to the alternative threshold,
    or to "keep all" without one.  262145 + 300 is past the grid cap (1024 workgroups of 256): the stride loop runs twice."""
    rng = np.random.default_rng(cap)
    avg = rng.random(cap).astype(np.float32)
    avg[:: 7] = np.float32(0.25)  # exactly on thres * mult: strict <
    avg[min(3, cap - 1)] = np.nan
    lib = _lib.load()
    d_avg = T(avg)
    thres, alt, nan = T(np.array([0.125], np.float32)), T(np.array([0.6], np.float32)), T(np.array([np.nan], np.float32))
    with np.errstate(invalid="ignore"):
        by_t = {"main": avg < np.float32(0.125) * np.float32(2.0), "alt": avg < np.float32(0.6), "all": np.ones(cap, bool), "nan": np.zeros(cap, bool)}
    for count in sorted({0, 1, cap - 1, cap}):
        for name, th, a, gate, expect in (("no gate", thres, None, None, "main"), ("gate > 0", thres, alt, I32(5), "main"),
                                          ("gate 0, alt", thres, alt, I32(0), "alt"), ("gate 0, no alt", thres, None, I32(0), "all"),
                                          ("thres nan", nan, None, None, "nan"), ("gate 0, alt nan", thres, nan, I32(0), "nan")):
            buf, flag = _guarded(cap, torch.uint8, 9)
            assert lib.pgdvs_threshold_flags(d_avg.data_ptr(), I32(count).data_ptr(), cap, th.data_ptr(), 2.0,
                                             None if a is None else a.data_ptr(), None if gate is None else gate.data_ptr(),
                                             flag.data_ptr(), ops._stream()) == 0
            torch.cuda.synchronize()
            want = by_t[expect].astype(np.uint8)
            want[count:] = 0
            assert np.array_equal(N(flag), want), (name, count)
            assert (N(buf)[cap:] == 9).all(), (name, count)
    # the front end allocates and returns the same flags
    got = ops.threshold_flags(d_avg, I32(cap), thres, 2.0, alt, I32(0))
    assert np.array_equal(N(got), by_t["alt"].astype(np.uint8))


@pytest.mark.parametrize("width,cap_a,cap_b", [(1, 5, 4), (3, 300, 120), (3, 1, 1), (1, 400000, 200000), (3, 100000, 80000)])
def test_concat_rows_direct(width, cap_a, cap_b):
    """out = [a[:count_a], b[:count_b]]; nothing of b when b is absent or when require_a and count_a == 0.  The last two
    sizes hold more than 524288 floats (2048 workgroups of 256): the stride loop runs a second round."""
    rng = np.random.default_rng(cap_a + width)
    a, b = rng.random((cap_a, width)).astype(np.float32), rng.random((cap_b, width)).astype(np.float32) + 2
    d_a, d_b = T(a), T(b)
    lib = _lib.load()
    big = (cap_a + cap_b) * width > 524288
    counts_a = [0, cap_a] if big else sorted({0, 1, cap_a - 1, cap_a})
    counts_b = [cap_b] if big else sorted({0, 1, cap_b - 1, cap_b})
    for ca in counts_a:
        for cb in counts_b:
            for with_b in (True, False):
                for require_a in (0, 1):
                    buf, out = _guarded((cap_a + cap_b) * width, torch.float32, GUARD)
                    cnt = torch.full((3,), -77, dtype=torch.int32, device=DEV)
                    assert lib.pgdvs_concat_rows(d_a.data_ptr(), I32(ca).data_ptr(), cap_a, d_b.data_ptr() if with_b else None,
                                                 I32(cb).data_ptr() if with_b else None, cap_b if with_b else 0, width, require_a,
                                                 out.data_ptr(), cnt[1:].data_ptr(), ops._stream()) == 0
                    torch.cuda.synchronize()
                    nb = cb if with_b and not (require_a and ca == 0) else 0
                    want = np.concatenate([a[:ca], b[:nb]]).reshape(-1)
                    assert N(cnt).tolist() == [-77, ca + nb, -77], (ca, cb, with_b, require_a)
                    got = N(buf)
                    assert np.array_equal(got[: want.size], want), (ca, cb, with_b, require_a)
                    assert (got[want.size:] == GUARD).all(), (ca, cb, with_b, require_a)  # rows beyond the count stay untouched
    rows, n = ops.concat_rows(d_a, I32(cap_a), d_b, I32(cap_b), require_a=True)
    assert int(n.item()) == cap_a + cap_b and np.array_equal(N(rows), np.concatenate([a, b]))
    rows, n = ops.concat_rows(d_a, I32(0), d_b, I32(cap_b), require_a=True)
    assert int(n.item()) == 0
    rows, n = ops.concat_rows(d_a, I32(min(2, cap_a)))
    assert int(n.item()) == min(2, cap_a) and np.array_equal(N(rows)[: min(2, cap_a)], a[: min(2, cap_a)])


@pytest.mark.parametrize("width,cap,n_src", [(1, 1, 1), (3, 300, 77), (1, 524288 + 300, 1000), (3, 1000, 100000)])
def test_gather_rows_direct(width, cap, n_src):
    """dst[i] = src[idx[i]] for i < count, nothing beyond.  524288 + 300 rows are past the grid cap (2048 workgroups of
    256): the stride loop runs a second round."""
    rng = np.random.default_rng(cap + width)
    src = rng.random((n_src, width)).astype(np.float32)
    idx = rng.integers(0, n_src, cap).astype(np.int32)
    idx[0], idx[-1] = n_src - 1, 0
    d_src, d_idx = T(src), T(idx)
    lib = _lib.load()
    for count in sorted({0, 1, cap - 1, cap}):
        buf, dst = _guarded(cap * width, torch.float32, GUARD)
        assert lib.pgdvs_gather_rows(d_src.data_ptr(), d_idx.data_ptr(), I32(count).data_ptr(), cap, width, dst.data_ptr(), ops._stream()) == 0
        torch.cuda.synchronize()
        got = N(buf)
        assert np.array_equal(got[: count * width], src[idx[:count]].reshape(-1)), count
        assert (got[count * width:] == GUARD).all(), count
    got = ops.gather_rows(d_src, d_idx, I32(cap))
    assert np.array_equal(N(got), src[idx])
    # an empty source: nothing to gather, no launch
    assert ops.gather_rows(d_src[:0], d_idx, I32(0)).shape == (cap, width)
