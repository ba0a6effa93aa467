"""The image-metric kernels on the MI355X at their size, window, mask and code edges (csrc/eval.hip, eval_ssim.hip,
eval_dycheck.hip, lpips.hip) against the float64 references of tests/metric_cases.py: the shared quantisation bit for bit next
to every code boundary; the PSNR sums at the grid-stride period; the NVIDIA SSIM map per pixel within the derived bound at
the 32 x 64 tile's edges; the DyCheck PSNR sums (every halo pixel once) and SSIM means at 32 / 33 map entries per axis; every
backbone layer, the head and the nearest-resampled mask at 1 x 1 tail maps and whole GEMM tiles; the DyCheck LPIPS with the
border rows and columns of its bilinear upsampling singled out by band and one-pixel masks.  Every test prints its figures
before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metric_cases as M
import test_dycheck_host as DH
import test_lpips_host as LH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def W_nv():
    return LH.weights(DEV)


@pytest.fixture(scope="module")
def W_dy():
    return DH.weights(device=DEV)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _feed(gt_codes, pred_codes):
    """pred [3,H,W] and gt [H,W,3] on the GPU, raw float32 code / 255"""
    return T(M.values(pred_codes).transpose(2, 0, 1)), T(M.values(gt_codes))


def _m3(m):
    return np.ascontiguousarray(np.repeat(np.asarray(m, np.float32)[..., None], 3, axis=-1))


def _close(got, want, rtol, what):
    print(f"{what}: got {got!r} want {want!r} err {abs(got - want):.3e} tol {rtol * abs(want):.3e}")
    if want == 0:
        assert got == 0, what
    else:
        assert abs(got - want) <= rtol * abs(want), (what, got, want)


# ---------------------------------------------------------------- 1. quantisation
def test_quantisation_bit_for_bit(W_nv, W_dy):
    """the quantised images are the numpy float32 statement's bit for bit, and every metric row from the raw input equals
    the row from the pre-quantised input byte for byte"""
    from pgdvs_amd import ops

    gt, pred = M.quantisation_probe()
    H, W = gt.shape[:2]
    m1 = M.mask("soft", H, W)
    m3 = np.ascontiguousarray(np.random.default_rng(5).random((H, W, 3)).astype(np.float32))
    gq = M.quantise_codes(gt).astype(np.float32) / np.float32(255)
    pq = M.quantise_codes(pred).astype(np.float32) / np.float32(255)
    _, got_p, got_g = ops.eval_psnr_sums(T(pred), T(gt), T(m3), want_images=True)
    bad_g = int((got_g.cpu().numpy().view(np.uint32) != gq.transpose(2, 0, 1).view(np.uint32)).sum())
    bad_p = int((got_p.cpu().numpy().view(np.uint32) != pq.view(np.uint32)).sum())
    print("quantised values that differ: gt", bad_g, "pred", bad_p)
    assert bad_g == 0 and bad_p == 0
    rows = {"eval_psnr_sums": lambda p, g: ops.eval_psnr_sums(p, g, T(m3))[0],
            "eval_ssim_sums": lambda p, g: ops.eval_ssim_sums(p, g, T(m3))[0],
            "dycheck_psnr_ssim_sums": lambda p, g: ops.dycheck_psnr_ssim_sums(p, g, T(m1[..., None])),
            "lpips_sums": lambda p, g: ops.lpips_sums(p, g, T(m3), W_nv)[0],
            "dycheck_lpips": lambda p, g: ops.dycheck_lpips(p, g, T(m1[..., None]), W_dy)}
    for name, fn in rows.items():
        raw, pre = fn(T(pred), T(gt)).cpu().numpy(), fn(T(pq), T(gq)).cpu().numpy()
        print(name, raw, pre)
        assert raw.tobytes() == pre.tobytes(), name
        assert np.isfinite(raw).all(), name


# ---------------------------------------------------------------- 2. PSNR sums
@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (37, 53), (255, 257), (256, 256), (1, 65537)])
def test_psnr_sums(H, W):
    """sums[0..2] and sums[5] to rtol 1e-12 (float64 summation order: 3 P 2^-53 is far below it), sums[3] = 3HW exactly,
    sums[4] exactly for binary masks, and exactly 0 for identical images"""
    from pgdvs_amd import ops

    last = (H - 1, W - 1)
    masks = {"full": M.mask("full", H, W), "empty": M.mask("empty", H, W), "pixel": M.mask("pixel", H, W, last)}
    masks = {k: _m3(v) for k, v in masks.items()}
    masks["soft"] = np.random.default_rng(H * 1000 + W).random((H, W, 3)).astype(np.float32)
    for kind in ("noise", *M.FLATS, "one_pixel", "ident"):
        gt, pred = M.images(kind, H, W, last)
        p, g = _feed(gt, pred)
        for mk, m3 in masks.items():
            s = ops.eval_psnr_sums(p, g, T(m3))[0].cpu().numpy()
            want = M.psnr_sums(gt, pred, m3)
            for j in (0, 1, 2, 5):
                _close(s[j], want[j], M.PSNR_RTOL, f"{H}x{W}/{kind}/{mk} sums[{j}]")
            assert s[3] == 3 * H * W and s[6] == -1 and s[7] == 0
            if mk != "soft":
                assert s[4] == want[4] and s[5] == want[5], (kind, mk, s[4], want[4])
            else:
                _close(s[4], want[4], M.PSNR_RTOL, "sums[4]")
            if kind in ("ident", "flat_0_0"):
                assert s[0] == 0 and s[1] == 0 and s[2] == 0


# ---------------------------------------------------------------- 3. NVIDIA SSIM
def _ssim_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}" + (f"@{c[3]}" if c[3] else "")


def _ssim_inputs(case):
    H, W, kind, pn = case
    return M.images(kind, H, W, M.positions(H, W, 32, 64)[pn] if pn else None)


@pytest.mark.parametrize("case", M.ssim_cases(), ids=_ssim_id)
def test_ssim_map_within_the_derived_bound(case):
    """every pixel of the map within metric_cases.ssim_bound of the float64 map, the three ratios to 1e-6"""
    from pgdvs_amd import ops

    H, W, kind, _ = case
    gt, pred = _ssim_inputs(case)
    m3 = np.random.default_rng(H * 131 + W).random((H, W, 3)).astype(np.float32)
    p, g = _feed(gt, pred)
    sums, smap = ops.eval_ssim_sums(p, g, T(m3), want_map=True)
    s, got = sums.cpu().numpy(), smap.cpu().numpy().transpose(1, 2, 0).astype(np.float64)
    S, bound = M.ssim_reference(gt, pred), M.ssim_bound(gt, pred)
    err = np.abs(got - S)
    worst = float((err / bound).max())
    print(f"{_ssim_id(case)}: worst err/bound {worst:.3f}, max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert (err <= bound).all(), (float((err / bound).max()), np.unravel_index((err / bound).argmax(), err.shape))
    assert s[3] == 3 * H * W and s[6] == 0 and s[7] == 0
    m = m3.astype(np.float64)
    ms = (np.float32(1) - m3).astype(np.float64)
    for j, w in enumerate((np.ones_like(m), m, ms)):
        want = float(np.sum(S * w) / (np.sum(w) + 1e-8))
        got_j = s[j] / (s[3 + j] + 1e-8)
        print(f"  ratio {j}: got {got_j!r} want {want!r}")
        assert abs(got_j - want) <= 1e-6, (j, got_j, want)
    if kind in ("ident", "flat_0_0"):  # equal images: numerator = denominator, the reciprocal is within 1 ulp
        assert float(np.abs(got - 1.0).max()) <= 2 * 2.0 ** -23, float(np.abs(got - 1.0).max())


@pytest.mark.parametrize("H,W", [(33, 65), (39, 71)])
def test_ssim_single_pixel_masks(H, W):
    """a one-pixel mask (all three channels): sums[1] is the map's value there, to the per-pixel bound, and sums[4] = 3"""
    from pgdvs_amd import ops

    gt, pred = M.images("noise", H, W)
    p, g = _feed(gt, pred)
    S, bound = M.ssim_reference(gt, pred), M.ssim_bound(gt, pred)
    for name, pos in M.positions(H, W, 32, 64).items():
        s = ops.eval_ssim_sums(p, g, T(_m3(M.mask("pixel", H, W, pos))))[0].cpu().numpy()
        want, tol = float(S[pos].sum()), float(bound[pos].sum())
        print(f"{H}x{W} mask@{name}: sums[1] {s[1]!r} want {want!r} err {abs(s[1] - want):.3e} tol {tol:.3e}")
        assert abs(s[1] - want) <= tol and s[4] == 3.0 and s[5] == 3.0 * (H * W - 1)


# ---------------------------------------------------------------- 4. DyCheck PSNR + SSIM
@pytest.mark.parametrize("case", M.dycheck_cases(), ids=M.dycheck_tag)
def test_dycheck_psnr_ssim(case):
    """s[3] = 3HW and, for binary masks, s[4] = 3 sum(m) exactly; s[0], s[1] to rtol 8 * 2^-24 (every halo pixel once: one
    dropped or doubled is a whole term); the SSIM means to the measured tolerance (a single entry per channel at 11 x 11).

    Found with these cases and settled in eval_dycheck.hip, whose moments, map entries and sums are float64 since: in fp32 a
    thread's sum of its 12 entries was off by 1.82e-7 (flat 128/131) and 1.09e-7 (flat 255/250) on a constant map, eight cases;
    and the eleven sequential fp32 taps lost 4.465e-6 on the 11 x 12 ramp (tolerance 1.884e-6), whose two entries per channel
    cancel four to one in mu[2] - mu00.  The host test reproduces all three figures in numpy float32
    (metric_cases.dycheck_ssim_fp32_emulation).  The kernel now agrees with the float64 reference to 4e-16 on every case."""
    from pgdvs_amd import ops

    H, W = case[:2]
    key = M.dycheck_tag(case)
    gt, pred, m = M.dycheck_inputs(case)
    p, g = _feed(gt, pred)
    s = ops.dycheck_psnr_ssim_sums(p, g, T(m[..., None])).cpu().numpy()
    d2, d2m, cnt, m3sum = M.dycheck_psnr_sums(gt, pred, m)
    _close(s[0], d2, M.DYCHECK_PSNR_RTOL, key + " s[0]")
    _close(s[1], d2m, M.DYCHECK_PSNR_RTOL, key + " s[1]")
    assert s[3] == cnt and s[6] == -1 and s[7] == 0
    if np.isin(m, (0.0, 1.0)).all():
        assert s[4] == m3sum, (s[4], m3sum)
    else:
        _close(s[4], m3sum, M.DYCHECK_PSNR_RTOL, key + " s[4]")
    want = M.dycheck_reference(M.values(gt), M.values(pred), m)[0]
    n_map = 3.0 * (H - 10) * (W - 10)
    for j, (got, w) in enumerate(((s[2] / n_map, want[1]), (s[5] / n_map, want[3]))):
        tol = M.tolerance(key, j)
        print(f"{key} ssim[{j}]: got {got!r} want {w!r} err {abs(got - w):.3e} tol {tol:.3e}")
        assert abs(got - w) <= tol, (key, j, got, w, tol)


# ---------------------------------------------------------------- 5. LPIPS backbone and head
_LP_KINDS = [("noise", None), ("flat_0_255", None), ("one_pixel", "c00"), ("one_pixel", "c11")]


@pytest.mark.parametrize("kind,pn", _LP_KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", M.LPIPS_SIZES)
def test_lpips_layers_head_and_mask(H, W, kind, pn, W_nv):
    """every layer against float64 conv2d on the kernel's own input to it, within (K + 1) u conv(|x|, |w|, |b|); the head and
    the three ratios against the float64 head on the kernel's own features (rtol 1e-5, atol 1e-9); s[3] = h1 w1; with the mask
    that is 1 exactly where the nearest rule looks, s[4] = h1 w1, and with its shifted copies what F.interpolate counts"""
    from pgdvs_amd import ops
    from pgdvs_amd.harness import _ALEX_CONVS

    gt, pred = M.images(kind, H, W, M.positions(H, W, 32, 32)[pn] if pn else None)
    p, g = _feed(gt, pred)
    sizes, _ = ops.lpips_map_sizes(H, W)
    h1, w1 = sizes[0]
    masks = {"soft": M.mask("soft", H, W), "rule": M.nearest_rule_mask(H, W, h1, w1),
             "rule_right": M.nearest_rule_mask(H, W, h1, w1, 0, 1), "rule_down": M.nearest_rule_mask(H, W, h1, w1, 1, 0),
             "stripes11": M.mask("stripes11", H, W)}
    w64 = M.Weights64(W_nv)
    feats64 = None
    for mk, m in masks.items():
        sums, feats = ops.lpips_sums(p, g, T(_m3(m)), W_nv, want_features=True)
        s = sums.cpu().numpy()
        if feats64 is None:
            feats64 = [f.double().cpu() for f in feats]
            assert [tuple(f.shape[2:]) for f in feats64] == [tuple(x) for x in sizes]
            x = 2.0 * torch.stack([M.chw(gt), M.chw(pred)]).double() - 1.0
            for j, (_, k, st, pd, pool) in enumerate(_ALEX_CONVS):
                inp = x if j == 0 else feats64[j - 1]
                if pool:
                    inp = F.max_pool2d(inp, kernel_size=3, stride=2)
                w, b = w64.convs[2 * j], w64.convs[2 * j + 1]
                want = F.relu(F.conv2d(inp, w, b, stride=st, padding=pd))
                absc = F.conv2d(inp.abs(), w.abs(), b.abs(), stride=st, padding=pd)
                K = w[0].numel()
                err = (feats64[j] - want).abs()
                worst = float((err / ((K + 1) * M.U * absc + 1e-30)).max())
                print(f"{H}x{W}/{kind} relu{j + 1} {tuple(want.shape)}: worst err/bound {worst:.3f}, max err {float(err.max()):.3e}")
                assert worst <= 1.0, (j, K, worst)
        want, _, cnt = M.lpips_head64(feats64, w64.lins, m)
        print(f"{H}x{W}/{kind}/{mk}: got {s[:3]} want {want} s[3..5] {s[3:6]} count {cnt}")
        np.testing.assert_allclose(s[:3], want, rtol=1e-5, atol=1e-9)
        assert s[3] == h1 * w1 and s[6] == 0 and s[7] == 0
        if mk != "soft":
            assert s[4] == cnt and s[5] == h1 * w1 - cnt, (mk, s[4], cnt)
        if mk == "rule":
            assert s[4] == h1 * w1
    same = ops.lpips_sums(T(M.values(gt).transpose(2, 0, 1)), g, T(_m3(masks["soft"])), W_nv)[0].cpu().numpy()
    assert list(same[:3]) == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------- 6. DyCheck LPIPS
@pytest.mark.parametrize("case", M.dlpips_cases(), ids=M.dlpips_tag)
def test_dycheck_lpips(case, W_dy):
    """s[0], s[1] against the float64 statement to the measured tolerance; s[3] = HW exactly, s[5] exactly for binary masks; a
    one-pixel mask on a pixel that no conv1 window reaches gives exactly 0"""
    from pgdvs_amd import ops

    H, W, mk, pos = case
    key = M.dlpips_tag(case)
    gt, pred, m = M.dlpips_inputs(case)
    p, g = _feed(gt, pred)
    s = ops.dycheck_lpips(p, g, T(m[..., None]), W_dy).cpu().numpy()
    want = M.lpips_dycheck64(gt, pred, m, W_dy)[0]
    for j in (0, 1):
        tol = M.tolerance(key, j)
        print(f"{key} lpips[{j}]: got {s[j]!r} want {want[j]!r} err {abs(s[j] - want[j]):.3e} tol {tol:.3e}")
        assert abs(s[j] - want[j]) <= tol, (key, j, s[j], want[j], tol)
    assert s[3] == H * W and s[6] == 0 and s[7] == 0
    if mk != "soft":
        assert s[5] == float(m.astype(np.float64).sum())
    if pos == (45, 23):
        assert want[1] == 0.0 and s[1] == 0.0 and s[4] == 0.0
    elif mk != "empty":
        assert want[1] > 0.0
