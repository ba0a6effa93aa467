"""The metric edge cases without a GPU (tests/metric_cases.py): the float64 references against the reference's own code on
structured images (tests/golden/metric_edges.npz, made by tests/golden/make_golden_metric_edges.py), the conditions the GPU
test's bounds rest on (the NVIDIA SSIM bound is at most 1e-5 on 99 % of every case's pixels and holds a float32 numpy
emulation of the kernel's expression; the recorded float32 deviations are current), and discrimination: each rule the cases
were built for, broken on purpose in the float64 reference, moves the designed case by at least ten times the tolerance the
GPU test uses there."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metric_cases as M
import test_dycheck_host as DH
from conftest import GOLDEN


@pytest.fixture(scope="module")
def W_():
    return DH.weights()


def golden():
    return dict(np.load(GOLDEN / "metric_edges.npz"))


# ---------------------------------------------------------------- the references against the reference's own code
def test_fixture_matches_the_generators_and_both_lin_fixtures():
    import lpips_inputs as LI
    import test_lpips_host as LH

    g = golden()
    np.testing.assert_allclose(g["weights_checksum"], LI.checksum(LI.backbone_weights()), rtol=1e-12)
    for a, b in zip(DH.weights().lins, LH.weights().lins):
        assert torch.equal(a, b)
    for name in M.FIXTURE_CASES:
        gt, pred, m = M.fixture_inputs(name)
        assert np.array_equal(g[f"{name}_gt"], gt) and np.array_equal(g[f"{name}_pred"], pred)
        assert np.array_equal(g[f"{name}_mask"].astype(np.float32), m)


@pytest.mark.parametrize("name", list(M.FIXTURE_CASES))
def test_references_vs_reference_golden(name, W_):
    """at the tolerances test_dycheck_host.py and test_lpips_host.py use for the float32 restatements"""
    g = golden()
    gt, pred, m = g[f"{name}_gt"], g[f"{name}_pred"], g[f"{name}_mask"].astype(np.float32)
    DH.close(M.dycheck_reference(M.values(gt), M.values(pred), m)[0], g[f"{name}_psnr_ssim"], 1e-5)
    np.testing.assert_allclose(M.lpips_dycheck64(gt, pred, m, W_)[0], g[f"{name}_dlpips"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(M.lpips_nvidia64(gt, pred, m, W_)[0], g[f"{name}_lpips"], rtol=0, atol=1e-5)


def test_psnr_reference_is_the_harness_statement():
    from pgdvs_amd.harness import masked_psnr

    gt, pred = M.images("noise", 37, 53)
    m3 = np.random.default_rng(1).random((37, 53, 3)).astype(np.float32)
    s = M.psnr_sums(gt, pred, m3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)  # noqa: E731
    for j, mm in enumerate((np.ones_like(m3), m3, np.float32(1) - m3)):
        want = masked_psnr(T(M.values(gt)), T(M.values(pred)), T(mm))
        assert abs(10 * math.log10(1.0 / (s[j] / (s[3 + j] + 1e-8))) - want) <= 1e-9


# ---------------------------------------------------------------- quantisation
def test_quantisation_probe_holds_every_boundary_and_tells_rounding_from_truncation():
    gt, pred = M.quantisation_probe()
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    need = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                           np.array([-0.0, 1e-45, 1.0 + 2.0 ** -23, np.inf, -np.inf, 1e30], np.float32)]).view(np.uint32)
    for img in (gt, pred.transpose(1, 2, 0)):
        for c in range(3):
            assert np.isin(need, img[..., c].view(np.uint32)).all() and np.isnan(img[..., c]).any()
    q = M.quantise_codes(gt)
    assert q.dtype == np.uint8 and q.min() == 0 and q.max() == 255
    assert M.quantise_codes(np.float32([np.nan, -np.inf, np.inf, 1e30, -0.0, 1e-45])).tolist() == [0, 0, 255, 255, 0, 0]
    with np.errstate(invalid="ignore"):
        rounded = np.rint(np.nan_to_num(np.clip(gt, 0, 1), nan=0.0) * np.float32(255)).astype(np.uint8)
    # (the GPU test is bit for bit: any code that differs is past its tolerance)
    assert int((rounded != q).sum()) >= 100, int((rounded != q).sum())
    assert not np.array_equal(M.quantise_codes(gt), M.quantise_codes(pred.transpose(1, 2, 0)))


# ---------------------------------------------------------------- NVIDIA SSIM: the bound's conditions
def _ssim_inputs(case):
    H, W, kind, pn = case
    return M.images(kind, H, W, M.positions(H, W, 32, 64)[pn] if pn else None)


def test_ssim_bound_is_tight_enough_and_holds_a_float32_emulation():
    """per case: the bound is at most 1e-5 on at least 99 % of the pixels; the kernel's expression in numpy float32 stays
    within it (worst ratio measured here: 0.27); and the float64 map on float32(code / 255) is within 5e-7 of the one on exact
    codes (3.3e-7 on the ramp, whose covariance is large and negative), below the 1e-6 of the ratios"""
    import test_ssim_host as SH

    worst = 0.0
    for case in M.ssim_cases():
        gt, pred = _ssim_inputs(case)
        S, bound = M.ssim_reference(gt, pred), M.ssim_bound(gt, pred)
        assert float((bound <= 1e-5).mean()) >= 0.99, (case, float((bound <= 1e-5).mean()))
        x1, x2, y1, y2, c1, c2 = M.ssim_terms(gt, pred)
        np.testing.assert_allclose(S, ((x1 + c1) * (x2 + c2)) / ((y1 + c1) * (y2 + c2)), rtol=0, atol=1e-13)
        ratio = float((np.abs(M.ssim_fp32_emulation(gt, pred) - S) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
        assert float(np.abs(SH.ssim_map(M.values(gt), M.values(pred)) - S).max()) <= 5e-7, case
    assert 12 <= M.SSIM_K <= 16 and worst >= 0.1  # (the bound is not slack by orders of magnitude)


def test_ssim_sizes_reach_every_tile_edge():
    assert {(31, 63), (32, 64), (33, 65), (38, 70), (39, 71)} <= set(M.SSIM_SIZES)  # tile 32 x 64, haloed tile 38 x 70
    for H, W in M.SSIM_KIND_SIZES:
        kinds = {c[2] for c in M.ssim_cases() if c[:2] == (H, W)}
        assert kinds >= {"noise", *M.FLATS, "checker", "ramp", "one_pixel", "halo_only"}


# ---------------------------------------------------------------- measured tolerances
def test_recorded_deviations_are_current(W_):
    """every recorded deviation within a factor of 2 of what this CPU gives.  A deviation below MEASURED_FLOOR / MEASURED_FACTOR
    has no say in the tolerance (the floor holds), so both sides are raised to that before they are compared."""
    keys = [M.dycheck_tag(c) for c in M.dycheck_cases()] + [M.dlpips_tag(c) for c in M.dlpips_cases()]
    assert set(keys) == set(M.MEASURED) and len(set(keys)) == len(keys)
    small = M.MEASURED_FLOOR / M.MEASURED_FACTOR
    now = {M.dycheck_tag(c): M.measure_dycheck_ssim(c) for c in M.dycheck_cases()}
    now.update({M.dlpips_tag(c): M.measure_dlpips(c, W_) for c in M.dlpips_cases()})
    for key, devs in now.items():
        for j in (0, 1):
            a, b = max(devs[j], small), max(M.MEASURED[key][j], small)
            assert 0.5 <= a / b <= 2.0, (key, j, devs[j], M.MEASURED[key][j])
            assert M.tolerance(key, j) >= M.MEASURED_FLOOR


def test_two_float32_orders_lie_further_apart_than_the_measured_tolerance():
    """What the measured tolerances of the DyCheck SSIM can and cannot carry.  On a flat image the map is constant, nothing
    averages out, and mu[2] - mu00 is pure rounding: the same expression with the kernel's tap order lands 2.3e-8 from
    float64 when product and sum round separately and 6.6e-5 away when every tap is one fused multiply-add (flat 128/131,
    full mask).  The recorded deviation of torch's evaluation (and four times it) lies between the two, so a correct float32
    kernel can miss it, and the fp32 kernel did on the 11 x 12 ramp; eval_dycheck.hip forms the moments and the map in float64
    for that reason.  (The kernels are built without contraction: the unfused figures were the fp32 kernel's.)"""
    case = (43, 43, "flat_128_131", None, "half32", None)
    gt, pred, m = M.dycheck_inputs(case)
    want = M.dycheck_reference(M.values(gt), M.values(pred), m)[0][1]
    ones = np.ones_like(m)
    plain = abs(M.dycheck_ssim_fp32_emulation(gt, pred, ones, fused=False) - want)
    fused = abs(M.dycheck_ssim_fp32_emulation(gt, pred, ones, fused=True) - want)
    tol = M.tolerance(M.dycheck_tag(case), 0)
    assert plain <= 1e-7 and 1e-5 <= fused <= 1e-4 and plain < tol < fused, (plain, fused, tol)
    case = (11, 12, "ramp", None, "soft", None)  # the fp32 kernel's own figure on the MI355X was 4.465e-6, this one
    gt, pred, m = M.dycheck_inputs(case)
    want = M.dycheck_reference(M.values(gt), M.values(pred), m)[0][1]
    plain = abs(M.dycheck_ssim_fp32_emulation(gt, pred, np.ones_like(m), fused=False) - want)
    assert 2e-6 <= plain <= 8e-6 and plain > M.tolerance(M.dycheck_tag(case), 0), plain
    case = (43, 43, "noise", None, "soft", None)  # (and on noise both orders sit inside the tolerance)
    gt, pred, m = M.dycheck_inputs(case)
    want = M.dycheck_reference(M.values(gt), M.values(pred), m)[0]
    for fu in (False, True):
        assert abs(M.dycheck_ssim_fp32_emulation(gt, pred, m, fused=fu) - want[3]) <= M.tolerance(M.dycheck_tag(case), 1)


def test_float32_sum_of_a_threads_twelve_entries_on_a_constant_map():
    """What the flat cases caught in eval_dycheck.hip: a thread used to add its 12 map entries (4 rows x 3 channels) in float32
    before it widened.  On a flat image all entries are one float32 value, every add rounds the same way in every thread, and
    the mean is off by 1.8e-7 (flat 128/131) and 1.1e-7 (flat 255/250) -- the kernel's figures on the MI355X to the last digit,
    past the 1e-7 tolerance -- while the entry itself is within 2.4e-8.  The kernel now works in float64 throughout."""
    for kind, was in (("flat_128_131", 1.8230207987635083e-07), ("flat_255_250", 1.0904475011841441e-07)):
        case = (42, 74, kind, None, "half32", None)
        gt, pred, m = M.dycheck_inputs(case)
        want = M.dycheck_reference(M.values(gt), M.values(pred), m)[0][1]
        entry = np.float32(M.dycheck_ssim_fp32_emulation(gt, pred, np.ones_like(m), fused=False))  # (a constant map: mean = entry)
        acc = np.float32(0)
        for _ in range(12):
            acc = np.float32(acc + entry)
        tol = M.tolerance(M.dycheck_tag(case), 0)
        assert abs(float(entry) - want) <= 2.4e-8 < tol
        assert abs(float(acc) / 12 - want) == pytest.approx(was, rel=1e-6) and was > tol


# ---------------------------------------------------------------- discrimination
def test_wrong_box_border_mirror():
    """numpy "reflect" (mirror without the edge sample) in place of "symmetric" in the 7 x 7 box"""
    for H, W in ((7, 7), (33, 65)):
        gt, pred = M.images("noise", H, W)
        x1, x2, y1, y2, c1, c2 = M.ssim_terms(gt, pred, mode="reflect")
        wrong = ((x1 + c1) * (x2 + c2)) / ((y1 + c1) * (y2 + c2))
        ratio = np.abs(wrong - M.ssim_reference(gt, pred)) / M.ssim_bound(gt, pred)
        assert float(ratio.max()) >= 10, float(ratio.max())
        assert float(ratio[3:-3, 3:-3].max(initial=0.0)) <= 1e-3  # (only the border can tell)


def test_wrong_nearest_index_by_rounding():
    from pgdvs_amd.ops import lpips_map_sizes

    for H, W in M.LPIPS_SIZES:
        (h1, w1) = lpips_map_sizes(H, W)[0][0]
        rule = M.nearest_rule_mask(H, W, h1, w1)
        count = lambda m: float(F.interpolate(torch.from_numpy(m)[None, None], size=[h1, w1]).sum())  # noqa: E731
        assert count(rule) == h1 * w1 and rule.sum() == h1 * w1
        assert count(M.nearest_rule_mask(H, W, h1, w1, 0, 1)) < h1 * w1 and count(M.nearest_rule_mask(H, W, h1, w1, 1, 0)) < h1 * w1
        iy, ix = M.nearest_index(H, h1, np.rint), M.nearest_index(W, w1, np.rint)
        assert float(rule[np.ix_(iy, ix)].sum()) <= h1 * w1 - 1  # (the GPU test's count is exact: one pixel off is past it)


def _upsample64(d, H, W, clamp=True):
    """bilinear, align_corners=False, by size, in float64 numpy; without ``clamp`` the source index is not clamped at 0"""
    d = d.numpy()

    def axis(n_in, n_out):
        src = (n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5
        if clamp:
            src = np.maximum(src, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)  # (truncation, as a C cast)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0

    y0, y1, ly = axis(d.shape[-2], H)
    x0, x1, lx = axis(d.shape[-1], W)
    rows = d[..., y0, :] * (1 - ly)[:, None] + d[..., y1, :] * ly[:, None]
    return torch.from_numpy(rows[..., x0] * (1 - lx) + rows[..., x1] * lx)


def test_wrong_bilinear_source_index(W_):
    for case, variants in (((46, 47, "band_top", None), ("noclamp", "corners")), ((46, 47, "band_left", None), ("noclamp", "corners")),
                           ((46, 47, "pixel", (0, 0)), ("noclamp",))):  # (align_corners=True keeps the corner pixel)
        H, W = case[:2]
        gt, pred, m = M.dlpips_inputs(case)
        right = M.lpips_dycheck64(gt, pred, m, W_)[0][1]
        np.testing.assert_allclose(M.lpips_dycheck64(gt, pred, m, W_, upsample=lambda d: _upsample64(d, H, W))[0][1], right, rtol=1e-12)
        wrong = {"noclamp": lambda d: _upsample64(d, H, W, clamp=False),
                 "corners": lambda d: F.interpolate(d, size=(H, W), mode="bilinear", align_corners=True)}
        for v in variants:
            diff = abs(M.lpips_dycheck64(gt, pred, m, W_, upsample=wrong[v])[0][1] - right)
            assert diff >= 10 * M.tolerance(M.dlpips_tag(case), 1), (case, v, diff, M.tolerance(M.dlpips_tag(case), 1))


def test_wrong_partial_convolution_mask_threshold():
    """conv(m, 1) > 0.5 in place of != 0.  The uniform soft mask never reaches the difference (eleven values sum to about 5.5):
    the soft stripes do, each window holding one value in (0, 1) or none."""
    for case in [c for c in M.dycheck_cases() if c[4] == "soft_stripes12"]:
        gt, pred, m = M.dycheck_inputs(case)
        right = M.dycheck_reference(M.values(gt), M.values(pred), m)[0][3]
        wrong = M.dycheck_reference(M.values(gt), M.values(pred), m, nonzero=lambda mw: mw > 0.5)[0][3]
        assert abs(wrong - right) >= 10 * M.tolerance(M.dycheck_tag(case), 1), (case, wrong, right)
    gt, pred, m = M.dycheck_inputs((43, 43, "noise", None, "soft", None))
    assert M.dycheck_reference(M.values(gt), M.values(pred), m, nonzero=lambda mw: mw > 0.5)[0][3] == \
        M.dycheck_reference(M.values(gt), M.values(pred), m)[0][3]


def test_wrong_scaling_layer(W_):
    """applied on the NVIDIA protocol: relu1 leaves the layer bound of the GPU test; omitted on DyCheck's: past the tolerance"""
    gt, pred = M.images("noise", 35, 35)
    m = M.mask("soft", 35, 35)
    _, right, _ = M.lpips_nvidia64(gt, pred, m, W_)
    vals_wrong, wrong, _ = M.lpips_nvidia64(gt, pred, m, W_, scaling_layer=True)
    w64 = M.Weights64(W_)
    x = 2.0 * torch.stack([M.chw(gt), M.chw(pred)]).double() - 1.0
    bound = (363 + 1) * M.U * F.conv2d(x.abs(), w64.convs[0].abs(), w64.convs[1].abs(), stride=4, padding=2)
    assert float(((wrong[0] - right[0]).abs() / bound).max()) >= 10
    case = (35, 35, "soft", None)
    gt, pred, m = M.dlpips_inputs(case)
    for j in (0, 1):
        diff = abs(M.lpips_dycheck64(gt, pred, m, W_, scaling_layer=False)[0][j] - M.lpips_dycheck64(gt, pred, m, W_)[0][j])
        assert diff >= 10 * M.tolerance(M.dlpips_tag(case), j), (j, diff)


def test_one_dropped_halo_pixel_in_the_dycheck_psnr_sums():
    """for halo_only and one_pixel a pixel of the last row / column dropped (or counted twice) is a whole term of s[0]: more
    than 100 times the tolerance"""
    for case in [c for c in M.dycheck_cases() if c[2] == "halo_only" or (c[2] == "one_pixel" and c[3] in ("c11", "c01", "c10", "right", "bottom"))]:
        H, W = case[:2]
        gt, pred, m = M.dycheck_inputs(case)
        d2 = (M.values(gt).astype(np.float64) - M.values(pred).astype(np.float64)) ** 2
        s0 = M.dycheck_psnr_sums(gt, pred, m)[0]
        pos = M.positions(H, W, 32, 32)[case[3]] if case[3] else (H - 1, W - 1)
        term = float(d2[pos].sum())
        assert term > 100 * M.DYCHECK_PSNR_RTOL * s0, (case, term, s0)


def test_dycheck_sizes_reach_every_tile_edge_and_the_uncovered_pixel(W_):
    assert {(42, 42), (43, 43), (42, 74), (75, 43)} <= set(M.DYCHECK_SIZES)  # 32 / 33 map entries; one and two haloed tiles
    kinds = {c[2] for c in M.dycheck_cases()}
    masks = {c[4] for c in M.dycheck_cases()}
    assert kinds >= {"noise", *M.FLATS, "checker", "ramp", "one_pixel", "halo_only"}
    assert masks >= {"full", "empty", "pixel", "band_top", "band_bottom", "band_left", "band_right", "stripes12", "stripes11", "half32", "soft"}
    gt, pred, m = M.dlpips_inputs((46, 47, "pixel", (45, 23)))
    assert M.lpips_dycheck64(gt, pred, m, W_)[0][1] == 0.0  # row 45 of 46 reaches no conv1 window
    gt, pred, m = M.dlpips_inputs((46, 47, "pixel", (23, 23)))
    assert M.lpips_dycheck64(gt, pred, m, W_)[0][1] > 0.0
