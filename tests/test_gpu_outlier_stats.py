"""GPU (MI355X): the outlier filter's threshold -- the three-pass radix select and the fp64 sums of csrc/knn.hip -- over
the selection edges of tests/outlier_cases.py, against its float64 reference and derived bound (validated on the host by
tests/test_outlier_stats_host.py); the tracker's ``threshold_flags`` (csrc/track.hip) at elements on and one ulp beside its
threshold; and the fused per-view form (``outlier_keep_fused``) at 1..22 dynamic points through PGDVSRenderer.forward,
against the per-op path and the oracle."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import outlier_cases as oc  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (checker only)
from pgdvs_amd import ops, synth  # noqa: E402

DEV = "cuda:0"
CASES = oc.cases()
IDS = oc.case_ids()
BY_NAME = {c[0]: c for c in CASES}


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cases are read-only arrays)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()  # fails loudly if the HIP extension is missing


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def _outlier_flags(avg, n, std_thres, remove_outlier):
    thres, flag = ops.outlier_flags(T(avg), _count(n), std_thres, remove_outlier)
    assert thres.shape == (1,) and flag.shape == (avg.size,) and flag.dtype == torch.uint8
    return N(thres)[0], N(flag)


# ---------------------------------------------------------------- ops.outlier_flags (per-op form)
@pytest.mark.parametrize("name,avg,n,std_thres", CASES, ids=IDS)
def test_outlier_flags_threshold_and_flags(name, avg, n, std_thres):
    ref = oc.reference(avg[:n], std_thres)
    thres, flag = _outlier_flags(avg, n, std_thres, True)
    print(f"{name}: thres={thres!r} T={ref.T!r} |d|={abs(float(thres) - ref.T)!r} B={ref.B!r} med={ref.med!r}")
    if np.isnan(ref.T):
        assert np.isnan(thres)
    elif oc.exact(ref, std_thres):
        assert float(thres) == ref.med  # (as a value: the sign of a zero is not compared)
    else:
        assert abs(float(thres) - ref.T) <= ref.B
    # the flags are those of the threshold that came out, and -- no element lies within B of T -- those of T itself
    assert np.array_equal(flag[:n], (avg[:n] < thres).astype(np.uint8))
    assert not flag[n:].any()
    want = np.zeros(n, np.uint8) if np.isnan(ref.T) else (avg[:n].astype(np.float64) < ref.T).astype(np.uint8)
    assert np.array_equal(flag[:n], want)
    # once more on the same workspace: the histograms start from zero again
    thres2, flag2 = _outlier_flags(avg, n, std_thres, True)
    assert thres2.view(np.uint32) == thres.view(np.uint32) and np.array_equal(flag2, flag)


@pytest.mark.parametrize("name,avg,n,std_thres", CASES, ids=IDS)
def test_outlier_flags_without_removal_keeps_all_and_still_gives_the_threshold(name, avg, n, std_thres):
    thres, _ = _outlier_flags(avg, n, std_thres, True)
    thres0, flag0 = _outlier_flags(avg, n, std_thres, False)
    assert thres0.view(np.uint32) == thres.view(np.uint32)
    assert np.isnan(thres0) == bool(np.isnan(oc.reference(avg[:n], std_thres).T))
    assert (flag0[:n] == 1).all() and not flag0[n:].any()


@pytest.mark.parametrize("std_thres", oc.STD_THRES)
@pytest.mark.parametrize("n", oc.COUNTS)
def test_outlier_threshold_does_not_depend_on_the_order(n, std_thres):
    """sorted input sends whole waves into one bin (the ballot shortcut), shuffled input every lane to its own"""
    got = {}
    for order in ("sorted", "shuffled"):
        _, avg, n_, s = BY_NAME[f"counts-{n}-{order}-s{std_thres}"]
        got[order] = _outlier_flags(avg, n_, s, True)[0]
    print(n, std_thres, got)
    assert got["sorted"].view(np.uint32) == got["shuffled"].view(np.uint32)


# ---------------------------------------------------------------- ops.threshold_flags (tracker)
THRES, ALT = np.float32(0.7431), np.float32(0.2113)
MULTS = (1.0, 0.5, 3.0)


@functools.lru_cache(maxsize=None)
def _threshold_avg():
    """more than one workgroup of elements, among them every threshold used below and its two neighbours; n < capacity"""
    rng = np.random.default_rng(5)
    edges = []
    for t in [THRES * np.float32(m) for m in MULTS] + [ALT]:
        edges += [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]
    special = np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], np.float32)
    n = 300
    body = rng.uniform(0.0, 3.0, n - len(edges) - special.size).astype(np.float32)
    avg = np.concatenate([rng.permutation(np.concatenate([body, np.array(edges, np.float32), special])),
                          np.resize(np.array([0.0, np.nan, -np.inf], np.float32), 37)])
    avg.setflags(write=False)
    return avg, n


@pytest.mark.parametrize("mult", MULTS)
@pytest.mark.parametrize("gate", ["none", "nonzero"])
def test_threshold_flags_at_the_threshold(mult, gate):
    avg, n = _threshold_avg()
    t = THRES * np.float32(mult)
    assert (avg[:n] == t).any() and (avg[:n] == np.nextafter(t, np.float32(0))).any() and (avg[:n] == np.nextafter(t, np.float32(9))).any()
    gate_count = None if gate == "none" else torch.tensor([3], dtype=torch.int32, device=DEV)
    alt = None if gate == "none" else T(np.array([ALT]))  # (not looked at: the gate is open)
    flag = N(ops.threshold_flags(T(avg), _count(n), T(np.array([THRES])), mult, alt, gate_count))
    assert flag.shape == (avg.size,)
    assert np.array_equal(flag[:n], (avg[:n] < t).astype(np.uint8)) and not flag[n:].any()


def test_threshold_flags_nan_threshold_flags_nothing():
    avg, n = _threshold_avg()
    flag = N(ops.threshold_flags(T(avg), _count(n), T(np.array([np.nan], np.float32)), 3.0))
    assert not flag.any()


def test_threshold_flags_zero_gate_uses_the_alternative_or_passes_all():
    avg, n = _threshold_avg()
    zero = torch.tensor([0], dtype=torch.int32, device=DEV)
    flag = N(ops.threshold_flags(T(avg), _count(n), T(np.array([THRES])), 3.0, T(np.array([ALT])), zero))
    assert np.array_equal(flag[:n], (avg[:n] < ALT).astype(np.uint8)) and not flag[n:].any()
    assert 0 < flag[:n].sum() < ((avg[:n] < THRES * np.float32(3.0)).sum())  # (told from the gated-off threshold)
    flag = N(ops.threshold_flags(T(avg), _count(n), T(np.array([THRES])), 3.0, None, zero))
    assert (flag[:n] == 1).all() and not flag[n:].any()


# ---------------------------------------------------------------- the fused form at small counts, through the renderer
H, W, KNN = 48, 64, 20
SMALL_COUNTS = (1, 2, 3, 20, 21, 22)


def _config(**over):
    from pgdvs_amd.instantiate import load_config

    cfg = load_config(static_renderer="geo")
    rc = cfg.engine.engine_cfg.render_cfg
    for k, v in over.items():
        rc[k] = v
    return cfg, rc


def _renderer(**over):
    from pgdvs_amd.renderers.pgdvs_renderer import PGDVSRenderer

    cfg, rc = _config(**over)
    return PGDVSRenderer(cfg, render_cfg=rc, softsplat_metric_abs_alpha=100.0).to(DEV).eval(), rc


def _footprint(p, flow):
    """the (up to four) target pixels a source pixel is splatted onto"""
    y, x = divmod(int(p), W)
    tx, ty = x + float(flow[0, y, x]), y + float(flow[1, y, x])
    x0, y0 = int(np.floor(tx)), int(np.floor(ty))
    return {(yy, xx) for yy in (y0, y0 + 1) for xx in (x0, x0 + 1) if 0 <= yy < H and 0 <= xx < W}


def _kept(mask, prints):
    """the kept set read off a rendered dynamic mask: the pixels whose footprint is lit"""
    return {p for p, fp in prints.items() if any(mask[yy, xx] > 0 for yy, xx in fp)}


@functools.lru_cache(maxsize=None)
def _scene():
    """one tiny view, a small static cloud, and lattice pixels (8 apart) that are valid dynamic points whose splat lands
    inside the frame -- by the oracle, on the CPU"""
    v = synth.make_video(3, H, W, seed=7)
    d = synth.make_view(v, 1, frac=0.4, seed=2)
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.normal(size=(64, 3)) * 0.5 + np.array([0.0, 0.0, 2.5]), rng.random((64, 3))], 1).astype(np.float32)
    d["st_pcl_rgb"] = cloud[None]
    _, rc = _config(dyn_pcl_remove_outlier=False, dyn_pcl_outlier_knn=KNN)
    lattice = [y * W + x for y in range(4, H, 8) for x in range(4, W, 8)]
    o = orc.render_view(_with_mask(d, lattice), dict(rc), static_noise=d["static_noise"], alpha=100.0)
    flow, valid = o["_info"]["flow_1_to_tgt"][0], o["_info"]["infos"][0]["valid"].reshape(-1)
    good = [p for p in lattice if valid[p] and len(_footprint(p, flow)) == 4 and _kept(o["render_dyn_mask"][0, 0], {p: _footprint(p, flow)})]
    return d, [int(p) for p in np.random.default_rng(11).permutation(good)]


def _with_mask(d, pixels):
    d = dict(d)
    m = np.zeros((1, 2, H, W, 1), np.float32)
    m[0, 1] = d["dyn_mask_src_temporal"][0, 1]
    m[0, 0].reshape(-1)[list(pixels)] = 1.0
    d["dyn_mask_src_temporal"] = m
    return d


@pytest.mark.parametrize("m", SMALL_COUNTS)
def test_fused_filter_at_small_counts_through_the_renderer(m, monkeypatch):
    """m valid dynamic points around outlier_knn + 1 = 21 (fewer neighbours than asked for below it; std of one element is
    NaN, of two equal means zero): the one native call per view (stat_pass_kernel<true> + outlier_keep_kernel) and the per-op
    path (pgdvs_outlier_flags) keep the same points as the oracle.  The native call hands out no keep map: the kept set is
    read off render_dyn_mask, which determines it here (checked on the oracle first: footprints apart, each lit when kept)."""
    base, good = _scene()
    assert len(good) >= m
    pixels = sorted(good[:m])
    d = _with_mask(base, pixels)
    model, rc = _renderer(dyn_pcl_remove_outlier=True, dyn_pcl_outlier_knn=KNN)
    rc_all = dict(rc, dyn_pcl_remove_outlier=False)
    o = orc.render_view(d, dict(rc), static_noise=d["static_noise"], alpha=100.0)
    o_all = orc.render_view(d, rc_all, static_noise=d["static_noise"], alpha=100.0)
    info = o["_info"]["infos"][0]
    # ---- on the CPU: exactly m valid points, and a dynamic mask that tells which of them were kept
    direct = orc.compute_dyn_pcl(
        dyn_mask_1=d["dyn_mask_src_temporal"][0, 0], rgb_1=d["rgb_src_temporal"][0, 0], depth_1=d["depth_src_temporal"][0, 0],
        flow_12=d["flow_fwd"][0], flow_12_occ_mask=d["flow_fwd_occ_mask"][0], rgb_2=d["rgb_src_temporal"][0, 1],
        depth_2=d["depth_src_temporal"][0, 1], flat_cam_1=d["flat_cam_src_temporal"][0, 0],
        flat_cam_2=d["flat_cam_src_temporal"][0, 1], flat_cam_tgt=d["flat_cam_tgt"][0], time_1=float(d["time_src_temporal"][0, 0]),
        time_2=float(d["time_src_temporal"][0, 1]), time_tgt=float(d["time_tgt"][0, 0]),
        dyn_render_use_flow_consistency=rc.dyn_render_use_flow_consistency, dyn_pcl_remove_outlier=True,
        dyn_pcl_outlier_knn=KNN, dyn_pcl_outlier_std_thres=rc.dyn_pcl_outlier_std_thres)
    assert int(direct["valid"].sum()) == m and sorted(np.flatnonzero(direct["valid"].reshape(-1)).tolist()) == pixels
    o_keep = set(np.flatnonzero(info["keep"].reshape(-1)).tolist())
    assert o_keep == set(np.flatnonzero(direct["keep"].reshape(-1)).tolist()) and o_keep <= set(pixels)
    prints = {p: _footprint(p, o_all["_info"]["flow_1_to_tgt"][0]) for p in pixels}
    cells = [c for fp in prints.values() for c in fp]
    assert len(cells) == len(set(cells)) == 4 * m
    assert _kept(o_all["render_dyn_mask"][0, 0], prints) == set(pixels)
    assert _kept(o["render_dyn_mask"][0, 0], prints) == o_keep
    print(f"m={m}: oracle keeps {len(o_keep)}, threshold {info['pcl_nn_dist_thres']!r}")
    if m == 1:
        assert np.isnan(info["pcl_nn_dist_thres"]) and not o_keep
    # ---- on the GPU: the native call, then the per-op path
    data = synth.to_torch(d, DEV)
    assert model._native_view_ok(data, rc)  # no silent fallback to the per-op path
    with torch.no_grad():
        rn = model.forward(dict(data), render_cfg=rc)
        monkeypatch.setenv("PGDVS_NATIVE_VIEW", "0")
        assert not model._native_view_ok(data, rc)
        rp = model.forward(dict(data), render_cfg=rc)
    torch.cuda.synchronize()
    assert torch.equal(rn["render_dyn_mask"], rp["render_dyn_mask"])
    assert np.array_equal(N(rn["render_dyn_mask"]), o["render_dyn_mask"])
    assert _kept(N(rn["render_dyn_mask"])[0, 0], prints) == _kept(N(rp["render_dyn_mask"])[0, 0], prints) == o_keep
    assert torch.allclose(rn["render_dyn_rgb"], rp["render_dyn_rgb"], rtol=0, atol=1e-6)
    for r in (rn, rp):
        np.testing.assert_allclose(N(r["render_dyn_rgb"]), o["render_dyn_rgb"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(N(r["combined_rgb"]), o["combined_rgb"], rtol=0, atol=1e-4)
    if m == 1:  # std of one element is NaN: nothing is below the threshold, the view is the static composite
        for r in (rn, rp):
            assert not N(r["render_dyn_mask"]).any()
            assert np.array_equal(N(r["combined_rgb"]), N(r["combined_rgb_static"]))
            assert np.array_equal(N(r["combined_rgb"]), N(r["geo_static_rgb"]))
