"""Cases, float64 references and tolerances for the image-metric kernels at their size, window, mask and code edges
(csrc/eval.hip, eval_ssim.hip, eval_dycheck.hip, lpips.hip).  No GPU code: tests/test_metric_edges_host.py checks the
references against the reference's own code (tests/golden/metric_edges.npz) and against deliberately wrong variants,
tests/test_gpu_metric_edges.py checks the kernels against the references.

Images are 8-bit codes [H,W,3] (uint8) and are fed to the kernels raw, as float32 code / 255; every reference is float64 on
those float32 values -- except the NVIDIA SSIM's, which is float64 on the exact codes, as eval_ssim.hip works on integers
(ssim_reference).  Masks are float32 [H,W].

Tolerances.  Derived: the PSNR sums (float64 summation order, rtol 1e-12), the DyCheck PSNR sums (rtol 8 * 2^-24: a thread adds
at most 42 * 42 / 256 -> 7 squared differences in fp32 before it widens), the NVIDIA SSIM map (ssim_bound).  Measured: the
DyCheck SSIM means and the DyCheck LPIPS values, for which no tight bound can be derived: MEASURED holds, per case, the
deviation of the project's float32 torch restatement (harness.masked_ssim_dycheck / masked_lpips_dycheck) from the float64
reference on the CPU; the kernel gets MEASURED_FACTOR times that, with the floor MEASURED_FLOOR.  The kernel adds its taps and
K terms in another order than torch (sequential taps, K in blocks of 16 on the matrix instruction); both orders obey the same
first-order bound, so agreement to a small multiple of one fp32 evaluation's own error is all that may be demanded."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # fp32 unit roundoff
PSNR_RTOL = 1e-12
DYCHECK_PSNR_RTOL = 8 * U
MEASURED_FACTOR, MEASURED_FLOOR = 4.0, 1e-7
SSIM_K = 16  # see ssim_bound

FLATS = {"flat_255_250": (255, 250), "flat_128_131": (128, 131), "flat_0_0": (0, 0), "flat_0_255": (0, 255)}


# ---------------------------------------------------------------- positions, images, masks
def positions(H, W, tile_h, tile_w):
    """name -> (y, x): the corners, the middle of each edge, and the first pixel past each tile boundary that the image has"""
    out = {"c00": (0, 0), "c01": (0, W - 1), "c10": (H - 1, 0), "c11": (H - 1, W - 1), "top": (0, W // 2), "bottom": (H - 1, W // 2),
           "left": (H // 2, 0), "right": (H // 2, W - 1)}
    if tile_w < W:
        out["past_x"] = (0, tile_w)
    if tile_h < H:
        out["past_y"] = (tile_h, 0)
    if tile_h < H and tile_w < W:
        out["past_xy"] = (tile_h, tile_w)
    seen, uniq = set(), {}
    for k, v in out.items():  # (tiny images: no position twice)
        if v not in seen:
            uniq[k] = v
            seen.add(v)
    return uniq


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def images(kind, H, W, pos=None):
    """(ground truth, prediction) as uint8 codes [H,W,3]"""
    rng = np.random.default_rng(_seed("img", kind, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    noise = rng.integers(0, 256, (H, W, 3))
    if kind == "noise":
        gt, pred = noise, np.clip(np.rint(noise + 20.0 * rng.standard_normal((H, W, 3))), 0, 255)
    elif kind == "ident":
        gt, pred = noise, noise
    elif kind in FLATS:
        gt, pred = (np.full((H, W, 3), v) for v in FLATS[kind])
    elif kind == "checker":  # period 1, the prediction shifted by one pixel
        gt = 255 * ((yy + xx) & 1)[..., None].repeat(3, axis=-1)
        pred = 255 - gt
    elif kind == "ramp":  # horizontal 0..255 against its mirror image
        gt = np.rint(xx * 255.0 / max(W - 1, 1))[..., None].repeat(3, axis=-1)
        pred = gt[:, ::-1]
    elif kind == "one_pixel":  # identical except one code (channel 1)
        gt, pred = noise, noise.copy()
        y, x = pos
        pred[y, x, 1] = (int(pred[y, x, 1]) + 128) % 256
    elif kind == "halo_only":  # identical except in the last 10 rows and the last 10 columns
        gt, pred = noise, noise.copy()
        other = rng.integers(0, 256, (H, W, 3))
        edge = (yy >= H - 10) | (xx >= W - 10)
        pred[edge] = other[edge]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(gt, dtype=np.uint8), np.ascontiguousarray(pred, dtype=np.uint8)


def mask(kind, H, W, pos=None):
    """float32 [H,W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "full":
        m = np.ones((H, W))
    elif kind == "empty":
        m = np.zeros((H, W))
    elif kind == "pixel":
        m = np.zeros((H, W))
        m[pos] = 1.0
    elif kind.startswith("band_"):  # 8 wide along one border
        m = {"band_top": yy < 8, "band_bottom": yy >= H - 8, "band_left": xx < 8, "band_right": xx >= W - 8}[kind]
    elif kind in ("stripes12", "stripes11"):  # vertical, width 1
        m = xx % int(kind[-2:]) == 0
    elif kind == "half32":  # a half plane cut at column 32
        m = xx < 32
    elif kind == "soft":
        m = np.random.default_rng(_seed("mask", H, W)).random((H, W))
    elif kind == "soft_stripes12":  # uniform values on width-1 stripes: an 11-tap window sums to 0 or to one value in (0, 1)
        m = np.random.default_rng(_seed("mask", H, W)).random((H, W)) * (xx % 12 == 0)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(m, dtype=np.float32)


def values(codes):
    """the float32 values code / 255 the kernels see"""
    return codes.astype(np.float32) / np.float32(255)


# ---------------------------------------------------------------- 1. quantisation
def quantise_codes(x):
    """the evaluator's quantisation as a numpy float32 statement -> uint8"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.nan_to_num(np.clip(x, 0, 1), nan=0.0) * np.float32(255)).astype(np.uint8)


def quantisation_probe():
    """(gt [32,64,3], pred [3,32,64]) float32: every channel of both arrangements holds, for every k in 0..255, float32(k/255)
    and its two fp32 neighbours, plus -0.0, the smallest denormal, 1 + 2^-23, +inf, -inf, NaN and 1e30 (each channel in another
    rotation, so that the two images differ).  The 775 values fill 16 x 64; the image is 32 rows high because the LPIPS passes
    take no image below 31 x 31."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    specials = np.array([-0.0, 1e-45, 1.0 + 2.0 ** -23, np.inf, -np.inf, np.nan, 1e30], np.float32)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), specials]).astype(np.float32)
    chan = lambda j: np.resize(np.roll(v, 97 * j), 32 * 64).reshape(32, 64)  # noqa: E731
    return np.ascontiguousarray(np.stack([chan(j) for j in range(3)], -1)), np.ascontiguousarray(np.stack([chan(j) for j in (5, 3, 4)]))


# ---------------------------------------------------------------- 2. PSNR sums (csrc/eval.hip)
def psnr_sums(gt_codes, pred_codes, mask3):
    """the six sums of ops.eval_psnr_sums in float64; mask3 float32 [H,W,3], ms = float32(1) - m formed in fp32"""
    a, b = values(gt_codes).astype(np.float64), values(pred_codes).astype(np.float64)
    m = np.asarray(mask3, np.float32)
    ms = (np.float32(1) - m).astype(np.float64)
    m = m.astype(np.float64)
    d2 = (a - b) ** 2
    return np.array([math.fsum(d2.ravel()), math.fsum((d2 * m).ravel()), math.fsum((d2 * ms).ravel()), float(d2.size),
                     math.fsum(m.ravel()), math.fsum(ms.ravel())])


# ---------------------------------------------------------------- 3. NVIDIA SSIM (csrc/eval_ssim.hip)
def ssim_reference(gt_codes, pred_codes):
    """S[H,W,3] in float64: test_ssim_host.ssim_map on code / 255 formed in float64.  eval_ssim.hip works on the integer codes
    and never forms float32(code / 255); that rounding moves a window's covariance by up to u rms(x) sd(y), which is relative
    to the variances and not to |2 Dab| + c2, so a reference on the float32 values would sit up to 1.05 ssim_bound away from the
    exact value where the covariance nearly vanishes (measured on halo_only 33 x 65; 3.3e-7 absolute at most, on the ramp)"""
    import test_ssim_host as SH

    return SH.ssim_map(gt_codes / 255.0, pred_codes / 255.0)


def ssim_fp32_emulation(gt_codes, pred_codes):
    """the kernel's expression in numpy float32 (an exact reciprocal in place of the 1-ulp one) -> float64"""
    f = np.float32
    x1, x2, y1, y2, c1, c2 = ssim_terms(gt_codes, pred_codes)
    num = (x1.astype(f) + f(c1)) * (x2.astype(f) + f(c2))
    den = (y1.astype(f) + f(c1)) * (y2.astype(f) + f(c2))
    return (num * (f(1) / den)).astype(np.float64)


def _box7_int(x, mode):
    H, W = x.shape[:2]
    xp = np.pad(x, ((3, 3), (3, 3), (0, 0)), mode=mode)
    c = sum(xp[:, k:k + W] for k in range(7))
    return sum(c[k:k + H] for k in range(7))


def ssim_terms(gt_codes, pred_codes, mode="symmetric"):
    """the kernel's exact integer terms (int64 [H,W,3]): 2 Sa Sb, 2 Dab, Sa^2 + Sb^2, Daa + Dbb, and c1, c2"""
    a, b = gt_codes.astype(np.int64), pred_codes.astype(np.int64)
    sa, sb, saa, sbb, sab = (_box7_int(z, mode) for z in (a, b, a * a, b * b, a * b))
    c1 = 0.02 ** 2 * (49.0 * 255.0) ** 2
    c2 = 0.06 ** 2 * (48.0 * 49.0 * 255.0 * 255.0)
    return 2 * sa * sb, 2 * (49 * sab - sa * sb), sa * sa + sb * sb, 49 * (saa + sbb) - sa * sa - sb * sb, c1, c2


def ssim_bound(gt_codes, pred_codes):
    """Per-pixel bound on |S_kernel - S_float64|.  The kernel forms, from exact integers X1 = 2 Sa Sb, X2 = 2 Dab,
    Y1 = Sa^2 + Sb^2, Y2 = Daa + Dbb (up to 3.1e8, so their conversion rounds), S = ((X1 + c1)(X2 + c2)) * rcp((Y1 + c1)(Y2 + c2))
    in fp32.  Roundings, each at most u = 2^-24 relative to the magnitude of what it rounds: four int-to-float conversions,
    four adds of a constant, one product per side (2), the reciprocal at 1 ulp = 2 u, the final product (1): 13; the fp32
    constants c1 and c2 themselves: c1 enters X1 + c1 and Y1 + c1 with the same sign and 0 <= X1 <= Y1, so both together move the
    ratio by at most 1 u; c2 enters X2 + c2 with X2 of either sign: 1 u on each side (2).  k = 16.  A rounding of the
    numerator's terms is relative to |X| + c, not to |X + c|: with X2 < 0 the sum cancels against c2, so the bound is
    k u (|X1| + c1)(|X2| + c2) / ((Y1 + c1)(Y2 + c2)), which is k u |S| where nothing cancels."""
    x1, x2, y1, y2, c1, c2 = ssim_terms(gt_codes, pred_codes)
    return SSIM_K * U * (np.abs(x1) + c1) * (np.abs(x2) + c2) / ((y1 + c1) * (y2 + c2))


SSIM_SIZES = [(7, 7), (7, 8), (8, 7), (9, 9), (31, 63), (32, 64), (33, 65), (38, 70), (39, 71), (65, 129)]
SSIM_KIND_SIZES = [(7, 7), (33, 65), (39, 71)]
SSIM_KINDS = ["noise", *FLATS, "checker", "ramp", "halo_only", "ident"]


def ssim_cases():
    """(H, W, image kind, position or None): every size with noise, every kind on three sizes, one_pixel at every position"""
    out = [(H, W, "noise", None) for H, W in SSIM_SIZES]
    out += [(H, W, k, None) for H, W in SSIM_KIND_SIZES for k in SSIM_KINDS if k != "noise"]
    out += [(H, W, "one_pixel", p) for H, W in SSIM_KIND_SIZES for p in positions(H, W, 32, 64)]
    return out


# ---------------------------------------------------------------- 4. DyCheck PSNR + SSIM (csrc/eval_dycheck.hip)
def dycheck_reference(a, b, m, nonzero=lambda mw: mw != 0):
    """float64 numpy restatement of metrics.py:63-186 on quantised images a, b [H,W,3] (ground truth, prediction) and the mask
    m [H,W]: ([psnr, ssim, mpsnr, mssim], [S map full, S map covisible] each [H-10,W-10,3])"""
    a, b, m = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(m, np.float64)
    f = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    f /= f.sum()

    def psnr(mm):
        mse = ((a - b) ** 2 * mm[..., None]).sum() / max(3 * mm.sum(), 1e-6)
        return math.inf if mse == 0 else -10.0 / math.log(10.0) * math.log(mse)

    def pconv(z, mm, axis):  # z[H,W,3], mm[H,W]; "valid" along axis (0 = H, 1 = W)
        n = z.shape[axis] - 10
        zm = z * mm[..., None]
        zc = sum(f[k] * np.take(zm, np.arange(k, k + n), axis=axis) for k in range(11))
        mw = sum(np.take(mm, np.arange(k, k + n), axis=axis) for k in range(11))
        ok = nonzero(mw)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(ok[..., None], zc * 11 / mw[..., None], 0.0)
        return out, ok.astype(np.float64)

    def filt(z, mm):
        z1, m1 = pconv(z, mm, 1)
        return pconv(z1, m1, 0)[0]

    def ssim(mm):
        mu0, mu1 = filt(a, mm), filt(b, mm)
        s00 = np.maximum(0, filt(a * a, mm) - mu0 * mu0)
        s11 = np.maximum(0, filt(b * b, mm) - mu1 * mu1)
        s01 = filt(a * b, mm) - mu0 * mu1
        s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        return ((2 * mu0 * mu1 + c1) * (2 * s01 + c2)) / ((mu0 ** 2 + mu1 ** 2 + c1) * (s00 + s11 + c2))

    ones = np.ones_like(m)
    maps = [ssim(ones), ssim(m)]
    return [psnr(ones), float(maps[0].mean()), psnr(m), float(maps[1].mean())], maps


def dycheck_psnr_sums(gt_codes, pred_codes, m):
    """s[0], s[1], s[3], s[4] of ops.dycheck_psnr_ssim_sums in float64"""
    d2 = (values(gt_codes).astype(np.float64) - values(pred_codes).astype(np.float64)) ** 2
    m = np.asarray(m, np.float64)
    return math.fsum(d2.ravel()), math.fsum((d2 * m[..., None]).ravel()), float(d2.size), 3.0 * math.fsum(m.ravel())


def dycheck_ssim_fp32_emulation(gt_codes, pred_codes, m, fused):
    """the mean of the kernel's SSIM map in numpy float32, taps added one after the other as eval_dycheck.hip adds them; with
    ``fused`` every tap is one fused multiply-add (the product exact in float64, rounded once), else product and sum round
    separately.  Not a reference: it shows how far two float32 orders of the same expression lie apart."""
    f32 = np.float32
    a, b, m = values(gt_codes), values(pred_codes), np.asarray(m, f32)
    g = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    filt = (g / g.sum()).astype(f32)
    H, W = m.shape
    Ho, Wo = H - 10, W - 10

    def tap(s, f, v):
        return (np.float64(f) * v.astype(np.float64) + s.astype(np.float64)).astype(f32) if fused else (s + f * v).astype(f32)

    def pconv(z, mm, axis, n):
        cut = (lambda x, k: x[:, k:k + n]) if axis == 1 else (lambda x, k: x[k:k + n])
        s, ms = np.zeros_like(cut(z, 0)), np.zeros_like(cut(z, 0))
        for k in range(11):
            s, ms = tap(s, filt[k], (cut(z, k) * cut(mm, k)).astype(f32)), ms + cut(mm, k)
        with np.errstate(all="ignore"):
            return np.where(ms != 0, (s * f32(11)) / ms, f32(0)).astype(f32), (ms != 0).astype(f32)

    maps = []
    for c in range(3):
        A, B = a[..., c], b[..., c]
        mu = []
        for z in (A, B, A * A, B * B, A * B):
            z1, m1 = pconv(z, m, 1, Wo)
            mu.append(pconv(z1, m1, 0, Ho)[0])
        mu00, mu11, mu01 = mu[0] * mu[0], mu[1] * mu[1], mu[0] * mu[1]
        s00, s11, s01 = np.maximum(f32(0), mu[2] - mu00), np.maximum(f32(0), mu[3] - mu11), mu[4] - mu01
        s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
        c1, c2 = f32(0.01 * 0.01), f32(0.03 * 0.03)
        maps.append((((f32(2) * mu01 + c1) * (f32(2) * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))).astype(np.float64))
    return float(np.mean(maps))


DYCHECK_SIZES = [(11, 11), (11, 12), (12, 11), (42, 42), (43, 43), (42, 74), (75, 43)]
DYCHECK_KINDS = ["noise", *FLATS, "checker", "ramp", "halo_only"]


def dycheck_cases():
    """(H, W, image kind, image position, mask kind, mask position)"""
    out = []
    for H, W in DYCHECK_SIZES:
        out += [(H, W, "noise", None, mk, None) for mk in ("full", "soft", "stripes12")]
    for H, W in ((43, 43), (42, 74)):
        out += [(H, W, ik, None, mk, None) for ik in DYCHECK_KINDS[1:] for mk in ("stripes11", "half32")]
    out += [(75, 43, "noise", None, mk, None) for mk in ("empty", "band_top", "band_bottom", "band_left", "band_right", "stripes11")]
    out += [(H, W, "noise", None, "soft_stripes12", None) for H, W in ((11, 11), (43, 43), (42, 74))]
    out += [(11, 11, "flat_255_250", None, "full", None), (11, 11, "checker", None, "soft", None), (11, 12, "ramp", None, "soft", None),
            (12, 11, "halo_only", None, "stripes12", None), (42, 42, "halo_only", None, "soft", None), (75, 43, "halo_only", None, "full", None)]
    for p in positions(43, 43, 32, 32):
        out += [(43, 43, "one_pixel", p, "full", None), (43, 43, "noise", None, "pixel", p)]
    for p in ("c11", "past_xy"):
        out += [(75, 43, "one_pixel", p, "soft", None), (42, 74, "one_pixel", {"c11": "c11", "past_xy": "past_x"}[p], "stripes12", None)]
    return out


def dycheck_inputs(case):
    H, W, ik, ip, mk, mp = case
    P = positions(H, W, 32, 32)
    gt, pred = images(ik, H, W, P[ip] if ip else None)
    return gt, pred, mask(mk, H, W, P[mp] if mp else None)


def dycheck_tag(case):
    H, W, ik, ip, mk, mp = case
    return f"{H}x{W}/{ik}{'@' + ip if ip else ''}/{mk}{'@' + mp if mp else ''}"


# ---------------------------------------------------------------- 5 / 6. LPIPS in float64 torch
class Weights64:
    """a harness.LpipsAlex's tensors cast to double, with the interface harness.alex_features / _lpips_layers use"""

    def __init__(self, w):
        self.convs = [t.detach().double().cpu() for t in w.convs]
        self.lins = [t.detach().double().cpu() for t in w.lins]

    def on(self, device):
        return self


def chw(codes):
    return torch.from_numpy(values(codes)).permute(2, 0, 1)


def nearest_index(n_in, n_out, rule=np.floor):
    """torch's nearest rule (the HIP head's): min(floor(dst * (float)in / out), in - 1), the product in float32"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(rule(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def nearest_rule_mask(H, W, h, w, dy=0, dx=0):
    """the float32 [H,W] mask that is 1 exactly on the pixels the nearest rule picks for an h x w map, shifted by (dy, dx)"""
    m = np.zeros((H, W), np.float32)
    m[np.ix_(nearest_index(H, h), nearest_index(W, w))] = 1.0
    out = np.zeros_like(m)
    out[dy:, dx:] = m[:H - dy, :W - dx]
    return out


def lpips_head64(feats, lins, m_hw, resize=None):
    """the NVIDIA head in float64: feats relu1..5 as [2,C,h,w] double, lins [1,C,1,1] double, m_hw float32 [H,W] ->
    ([full, dyn, static], per-layer distance maps, sum of the resized mask at relu1)"""
    resize = resize or (lambda m, size: F.interpolate(m, size=size))
    m = torch.as_tensor(m_hw, dtype=torch.float32)
    masks = [torch.ones_like(m).double(), m.double(), (1.0 - m).double()]  # (1 - m in fp32, as upstream)
    vals, maps, cnt = [0.0, 0.0, 0.0], [], None
    for f, lin in zip(feats, lins):
        n = f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((n[0:1] - n[1:2]) ** 2, lin)
        maps.append(d[0, 0])
        for j, mm in enumerate(masks):
            mr = resize(mm[None, None], list(d.shape[2:]))
            vals[j] += float(torch.sum(d * mr) / (torch.sum(mr) + 1e-8))
            if j == 1 and cnt is None:
                cnt = float(mr.sum())
    return vals, maps, cnt


def lpips_nvidia64(gt_codes, pred_codes, m_hw, weights, scaling_layer=False, resize=None):
    """harness._lpips_layers / _lpips_torch with the weights and images cast to double -> (values, features, maps)"""
    from pgdvs_amd.harness import _LPIPS_SCALE, _LPIPS_SHIFT, alex_features

    w = Weights64(weights)
    x = 2.0 * torch.stack([chw(gt_codes), chw(pred_codes)]).double() - 1.0
    if scaling_layer:
        shift, scale = (torch.tensor(v, dtype=torch.float32)[None, :, None, None] for v in (_LPIPS_SHIFT, _LPIPS_SCALE))
        x = (x - shift) / scale
    feats = alex_features(x, w)
    vals, maps, _ = lpips_head64(feats, w.lins, m_hw, resize)
    return vals, feats, maps


def lpips_dycheck64(gt_codes, pred_codes, m_hw, weights, scaling_layer=True, upsample=None):
    """harness._lpips_dycheck_torch with the weights, images and upsample cast to double: [lpips, mlpips], the summed map of
    the unmasked pair, the summed map of the masked pair"""
    from pgdvs_amd.harness import _lpips_layers

    g, p = chw(gt_codes), chw(pred_codes)
    H, W = g.shape[-2:]
    m = torch.as_tensor(m_hw, dtype=torch.float32)
    x = torch.stack([g, p, g * m, p * m]).double()  # (the mask product in fp32, as upstream forms it)
    upsample = upsample or (lambda d: F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False))
    val = sum(upsample(d) for d in _lpips_layers(x, Weights64(weights), scaling_layer))
    md = m.double()
    return [float(val[0, 0].sum() / max(float(H * W), 1e-6)), float((val[1, 0] * md).sum() / max(float(md.sum()), 1e-6))], val[0, 0], val[1, 0]


LPIPS_SIZES = [(31, 31), (35, 35), (46, 47), (47, 46), (47, 31), (67, 67), (71, 67)]
LPIPS_KINDS = ["noise", "flat_0_255", "one_pixel"]
DLPIPS_SIZES = [(31, 31), (35, 35), (46, 47), (47, 31), (63, 70)]
DLPIPS_MASKS = ["full", "band_top", "band_bottom", "band_left", "band_right", "half32", "soft"]
DLPIPS_STRIDE_SIZES = [(256, 512), (256, 513)]  # 131072 pixels: one grid-stride period of the upsampling pass, and one past it


def dlpips_cases():
    """(H, W, mask kind, mask position (y, x) or None).  46 x 47: conv1 (11 / 4, pad 2, floor) reaches no window past row 44,
    so a one-pixel mask at (45, 23) gives exactly 0 in float64 -- kept as the exact-zero case ("uncovered")."""
    out = [(H, W, mk, None) for H, W in DLPIPS_SIZES for mk in DLPIPS_MASKS]
    out += [(H, W, "pixel", p) for H, W in DLPIPS_SIZES for p in ((0, 0), (H // 2, W // 2))]
    out += [(46, 47, "pixel", (45, 23))]
    out += [(256, 512, "half32", None), (256, 513, "soft", None)]
    return out


def dlpips_tag(case):
    H, W, mk, p = case
    return f"{H}x{W}/noise/{mk}" + (f"@{p[0]},{p[1]}" if p else "")


def dlpips_inputs(case):
    H, W, mk, p = case
    gt, pred = images("noise", H, W)
    return gt, pred, mask(mk, H, W, p)


# ---------------------------------------------------------------- the fixture's cases (tests/golden/metric_edges.npz)
# name -> (H, W, image kind, image position name (32 x 32 tiles), mask kind)
FIXTURE_CASES = {
    "flat_hi": (42, 42, "flat_255_250", None, "stripes12"), "flat_mid": (43, 43, "flat_128_131", None, "half32"),
    "black": (31, 31, "flat_0_0", None, "full"), "bw": (35, 35, "flat_0_255", None, "band_left"),
    "checker": (43, 43, "checker", None, "soft"), "ramp": (42, 74, "ramp", None, "stripes11"),
    "one_c11": (47, 31, "one_pixel", "c11", "band_bottom"), "one_past": (46, 47, "one_pixel", "past_xy", "band_right"),
    "halo": (63, 70, "halo_only", None, "band_top"), "noise_a": (46, 47, "noise", None, "stripes12"),
    "noise_b": (74, 43, "noise", None, "empty"),
}


def fixture_inputs(name):
    H, W, ik, ip, mk = FIXTURE_CASES[name]
    gt, pred = images(ik, H, W, positions(H, W, 32, 32)[ip] if ip else None)
    return gt, pred, mask(mk, H, W)


# ---------------------------------------------------------------- measured deviations of the float32 torch restatements
def measure_dycheck_ssim(case):
    """|harness.masked_ssim_dycheck (fp32 torch) - float64 reference| for the full and the covisibility mask"""
    from pgdvs_amd.harness import masked_ssim_dycheck

    gt, pred, m = dycheck_inputs(case)
    want = dycheck_reference(values(gt), values(pred), m)[0]
    g, p, mm = chw(gt), chw(pred), torch.from_numpy(m)[None]
    return (abs(masked_ssim_dycheck(g, p, torch.ones_like(mm)) - want[1]), abs(masked_ssim_dycheck(g, p, mm) - want[3]))


def measure_dlpips(case, weights):
    """|harness.masked_lpips_dycheck (fp32 torch) - float64 reference| for the full and the covisibility mask"""
    from pgdvs_amd.harness import masked_lpips_dycheck

    gt, pred, m = dlpips_inputs(case)
    want = lpips_dycheck64(gt, pred, m, weights)[0]
    g, p, mm = chw(gt), chw(pred), torch.from_numpy(m)[None]
    return (abs(masked_lpips_dycheck(g, p, torch.ones_like(mm), weights) - want[0]), abs(masked_lpips_dycheck(g, p, mm, weights) - want[1]))


def tolerance(key, j):
    """the kernel's tolerance for value j (0 full, 1 covisible) of the measured case ``key``"""
    return max(MEASURED_FACTOR * MEASURED[key][j], MEASURED_FLOOR)


# key -> (deviation with the full mask, deviation with the case's mask); written by ``python tests/metric_cases.py``
MEASURED = {
    "11x11/noise/full": (2.96e-07, 2.96e-07),
    "11x11/noise/soft": (2.96e-07, 7.39e-08),
    "11x11/noise/stripes12": (2.96e-07, 3.41e-08),
    "11x12/noise/full": (7.01e-08, 7.01e-08),
    "11x12/noise/soft": (7.01e-08, 5.85e-08),
    "11x12/noise/stripes12": (7.01e-08, 1.03e-08),
    "12x11/noise/full": (4.42e-08, 4.42e-08),
    "12x11/noise/soft": (4.42e-08, 4.67e-08),
    "12x11/noise/stripes12": (4.42e-08, 3.90e-08),
    "42x42/noise/full": (2.15e-09, 2.15e-09),
    "42x42/noise/soft": (2.15e-09, 1.59e-08),
    "42x42/noise/stripes12": (2.15e-09, 4.21e-08),
    "43x43/noise/full": (1.31e-08, 1.31e-08),
    "43x43/noise/soft": (1.31e-08, 1.40e-09),
    "43x43/noise/stripes12": (1.31e-08, 2.33e-08),
    "42x74/noise/full": (1.80e-09, 1.80e-09),
    "42x74/noise/soft": (1.80e-09, 7.30e-09),
    "42x74/noise/stripes12": (1.80e-09, 2.29e-08),
    "75x43/noise/full": (6.63e-09, 6.63e-09),
    "75x43/noise/soft": (6.63e-09, 1.64e-08),
    "75x43/noise/stripes12": (6.63e-09, 5.54e-09),
    "43x43/flat_255_250/stripes11": (9.70e-09, 3.14e-08),
    "43x43/flat_255_250/half32": (9.70e-09, 2.71e-08),
    "43x43/flat_128_131/stripes11": (9.79e-07, 3.44e-08),
    "43x43/flat_128_131/half32": (9.79e-07, 2.64e-08),
    "43x43/flat_0_0/stripes11": (0.00e+00, 0.00e+00),
    "43x43/flat_0_0/half32": (0.00e+00, 0.00e+00),
    "43x43/flat_0_255/stripes11": (7.97e-12, 1.10e-09),
    "43x43/flat_0_255/half32": (7.97e-12, 2.00e-10),
    "43x43/checker/stripes11": (8.68e-08, 1.92e-08),
    "43x43/checker/half32": (8.68e-08, 5.19e-08),
    "43x43/ramp/stripes11": (2.93e-06, 6.68e-09),
    "43x43/ramp/half32": (2.93e-06, 2.27e-07),
    "43x43/halo_only/stripes11": (4.97e-09, 8.10e-09),
    "43x43/halo_only/half32": (4.97e-09, 6.38e-09),
    "42x74/flat_255_250/stripes11": (9.70e-09, 3.23e-08),
    "42x74/flat_255_250/half32": (9.70e-09, 1.40e-08),
    "42x74/flat_128_131/stripes11": (2.34e-08, 3.85e-08),
    "42x74/flat_128_131/half32": (2.34e-08, 1.36e-08),
    "42x74/flat_0_0/stripes11": (0.00e+00, 0.00e+00),
    "42x74/flat_0_0/half32": (0.00e+00, 0.00e+00),
    "42x74/flat_0_255/stripes11": (7.97e-12, 1.13e-09),
    "42x74/flat_0_255/half32": (7.97e-12, 1.03e-10),
    "42x74/checker/stripes11": (8.68e-08, 1.96e-08),
    "42x74/checker/half32": (8.68e-08, 2.68e-08),
    "42x74/ramp/stripes11": (2.14e-05, 5.65e-09),
    "42x74/ramp/half32": (2.14e-05, 5.68e-06),
    "42x74/halo_only/stripes11": (2.96e-09, 1.98e-09),
    "42x74/halo_only/half32": (2.96e-09, 1.25e-08),
    "75x43/noise/empty": (6.63e-09, 0.00e+00),
    "75x43/noise/band_top": (6.63e-09, 6.40e-09),
    "75x43/noise/band_bottom": (6.63e-09, 2.51e-08),
    "75x43/noise/band_left": (6.63e-09, 8.05e-09),
    "75x43/noise/band_right": (6.63e-09, 4.10e-09),
    "75x43/noise/stripes11": (6.63e-09, 2.46e-09),
    "11x11/noise/soft_stripes12": (2.96e-07, 1.05e-07),
    "43x43/noise/soft_stripes12": (1.31e-08, 4.26e-09),
    "42x74/noise/soft_stripes12": (1.80e-09, 2.17e-08),
    "11x11/flat_255_250/full": (9.70e-09, 9.70e-09),
    "11x11/checker/soft": (8.68e-08, 5.37e-08),
    "11x12/ramp/soft": (4.71e-07, 6.31e-08),
    "12x11/halo_only/stripes12": (1.14e-07, 1.54e-08),
    "42x42/halo_only/soft": (5.14e-09, 2.90e-08),
    "75x43/halo_only/full": (2.61e-09, 2.61e-09),
    "43x43/one_pixel@c00/full": (3.89e-12, 3.89e-12),
    "43x43/noise/pixel@c00": (1.31e-08, 3.59e-11),
    "43x43/one_pixel@c01/full": (3.17e-11, 3.17e-11),
    "43x43/noise/pixel@c01": (1.31e-08, 3.28e-11),
    "43x43/one_pixel@c10/full": (7.23e-12, 7.23e-12),
    "43x43/noise/pixel@c10": (1.31e-08, 2.89e-11),
    "43x43/one_pixel@c11/full": (2.20e-11, 2.20e-11),
    "43x43/noise/pixel@c11": (1.31e-08, 2.13e-11),
    "43x43/one_pixel@top/full": (5.41e-11, 5.41e-11),
    "43x43/noise/pixel@top": (1.31e-08, 2.13e-10),
    "43x43/one_pixel@bottom/full": (5.00e-10, 5.00e-10),
    "43x43/noise/pixel@bottom": (1.31e-08, 2.60e-10),
    "43x43/one_pixel@left/full": (3.60e-10, 3.60e-10),
    "43x43/noise/pixel@left": (1.31e-08, 2.44e-10),
    "43x43/one_pixel@right/full": (5.90e-11, 5.90e-11),
    "43x43/noise/pixel@right": (1.31e-08, 4.22e-11),
    "43x43/one_pixel@past_x/full": (6.16e-11, 6.16e-11),
    "43x43/noise/pixel@past_x": (1.31e-08, 4.38e-11),
    "43x43/one_pixel@past_y/full": (3.69e-11, 3.69e-11),
    "43x43/noise/pixel@past_y": (1.31e-08, 2.20e-12),
    "43x43/one_pixel@past_xy/full": (3.32e-10, 3.32e-10),
    "43x43/noise/pixel@past_xy": (1.31e-08, 2.49e-09),
    "75x43/one_pixel@c11/soft": (1.16e-12, 1.12e-11),
    "42x74/one_pixel@c11/stripes12": (8.40e-11, 0.00e+00),
    "75x43/one_pixel@past_xy/soft": (3.21e-10, 5.79e-12),
    "42x74/one_pixel@past_x/stripes12": (1.09e-10, 0.00e+00),
    "31x31/noise/full": (2.04e-09, 2.04e-09),
    "31x31/noise/band_top": (2.04e-09, 3.18e-09),
    "31x31/noise/band_bottom": (2.04e-09, 6.24e-10),
    "31x31/noise/band_left": (2.04e-09, 1.55e-09),
    "31x31/noise/band_right": (2.04e-09, 3.98e-09),
    "31x31/noise/half32": (2.04e-09, 2.04e-09),
    "31x31/noise/soft": (2.04e-09, 1.01e-09),
    "35x35/noise/full": (4.05e-10, 4.05e-10),
    "35x35/noise/band_top": (4.05e-10, 1.91e-09),
    "35x35/noise/band_bottom": (4.05e-10, 2.58e-09),
    "35x35/noise/band_left": (4.05e-10, 1.97e-09),
    "35x35/noise/band_right": (4.05e-10, 2.01e-09),
    "35x35/noise/half32": (4.05e-10, 1.47e-09),
    "35x35/noise/soft": (4.05e-10, 2.21e-10),
    "46x47/noise/full": (1.87e-09, 1.87e-09),
    "46x47/noise/band_top": (1.87e-09, 3.07e-09),
    "46x47/noise/band_bottom": (1.87e-09, 2.14e-09),
    "46x47/noise/band_left": (1.87e-09, 2.04e-09),
    "46x47/noise/band_right": (1.87e-09, 1.74e-10),
    "46x47/noise/half32": (1.87e-09, 2.88e-10),
    "46x47/noise/soft": (1.87e-09, 3.45e-11),
    "47x31/noise/full": (1.24e-09, 1.24e-09),
    "47x31/noise/band_top": (1.24e-09, 8.25e-10),
    "47x31/noise/band_bottom": (1.24e-09, 2.13e-09),
    "47x31/noise/band_left": (1.24e-09, 4.03e-10),
    "47x31/noise/band_right": (1.24e-09, 2.30e-09),
    "47x31/noise/half32": (1.24e-09, 1.24e-09),
    "47x31/noise/soft": (1.24e-09, 6.97e-11),
    "63x70/noise/full": (3.43e-09, 3.43e-09),
    "63x70/noise/band_top": (3.43e-09, 8.64e-10),
    "63x70/noise/band_bottom": (3.43e-09, 1.16e-09),
    "63x70/noise/band_left": (3.43e-09, 1.70e-09),
    "63x70/noise/band_right": (3.43e-09, 7.57e-10),
    "63x70/noise/half32": (3.43e-09, 3.06e-09),
    "63x70/noise/soft": (3.43e-09, 1.97e-09),
    "31x31/noise/pixel@0,0": (2.04e-09, 1.30e-11),
    "31x31/noise/pixel@15,15": (2.04e-09, 1.01e-10),
    "35x35/noise/pixel@0,0": (4.05e-10, 2.09e-11),
    "35x35/noise/pixel@17,17": (4.05e-10, 5.13e-11),
    "46x47/noise/pixel@0,0": (1.87e-09, 7.63e-11),
    "46x47/noise/pixel@23,23": (1.87e-09, 1.05e-10),
    "47x31/noise/pixel@0,0": (1.24e-09, 1.76e-10),
    "47x31/noise/pixel@23,15": (1.24e-09, 1.31e-10),
    "63x70/noise/pixel@0,0": (3.43e-09, 1.06e-10),
    "63x70/noise/pixel@31,35": (3.43e-09, 4.50e-12),
    "46x47/noise/pixel@45,23": (1.87e-09, 0.00e+00),
    "256x512/noise/half32": (2.42e-10, 4.12e-10),
    "256x513/noise/soft": (3.86e-10, 1.06e-11),
}


if __name__ == "__main__":
    import sys

    sys.path.insert(0, __file__.rsplit("/", 1)[0])
    import test_dycheck_host as DH

    w = DH.weights()
    rows = [(dycheck_tag(c), measure_dycheck_ssim(c)) for c in dycheck_cases()] + [(dlpips_tag(c), measure_dlpips(c, w)) for c in dlpips_cases()]
    print("MEASURED = {")
    for k, (a, b) in rows:
        print(f'    "{k}": ({a:.2e}, {b:.2e}),')
    print("}")
