"""Caller-side harness that makes end-to-end numbers comparable with the reference's evaluator
(SURVEY.md 8f-1): ``eval_step`` reproduces ``PGDVSEvaluator.eval_step``
(pgdvs/engines/evaluator_pgdvs.py:26-188) around any renderer with the plugin contract -- to-device,
``forward`` under no_grad, clamp -> NaN to 0 -> quantise, ground truth resized to the render size,
the evaluator's three masked PSNRs (``obtain_quantitative_nvidia`` :190-283 with
``calculate_psnr`` pgdvs/utils/training.py:281-313), on request its three masked SSIMs (``calculate_ssim``
training.py:316-346, skimage 0.20 ``structural_similarity``) and its three masked LPIPS values (``PerceptualLoss(
model="net-lin", net="alex", version=0.1)``, trainer_pgdvs.py:132-137, given the AlexNet and lin weights as an
``LpipsAlex``), and ONE packed reduce of the metric sums to rank 0 (the reference issues one
``torch.distributed.reduce`` per key, :183-186).  On the GPU at render size the metrics are HIP passes (csrc/eval.hip,
csrc/eval_ssim.hip, csrc/lpips.hip); otherwise a few torch ops on final images.  SSIM's window sums are exact integers
here, where skimage 0.20 filters in float32: the two differ by about 1e-7 on a masked mean.
``eval_run`` is the loop around it (``run_eval_single_ckpt``, trainer_pgdvs.py:282-360, with what ``save_individual`` leaves:
per-view records and images), able to run ahead of the GPU by up to three steps; ``vis_step`` / ``vis_run`` are the
visualiser's."""
import math
import time
from collections import OrderedDict

import torch
import torch.nn.functional as F

from . import dist as pdist


def quantize_like_evaluator(x: torch.Tensor) -> torch.Tensor:
    """clamp(0,1) -> NaN to 0 -> (x*255).byte().float()/255 (evaluator_pgdvs.py:52-77)."""
    x = torch.nan_to_num(x.clamp(0.0, 1.0), nan=0.0)
    return (x * 255).byte().float() / 255.0


def masked_psnr(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor) -> float:
    """calculate_psnr (training.py:281-313): float64, mse normalised by sum(mask)+1e-8 (the mask
    broadcasts over channels exactly as given), and the reference's quirk of returning 0 when
    the images are identical."""
    assert img1.ndim == 3 and img2.ndim == 3
    a, b, m = img1.double(), img2.double(), mask.double()
    assert float(a.min()) >= 0 and float(a.max()) <= 1 and float(b.min()) >= 0 and float(b.max()) <= 1
    mse = float((((a - b) ** 2) * m).sum() / (m.sum() + 1e-8))
    if mse == 0:
        return 0
    return 10 * math.log10(1.0 / mse)


def _box7_sym(x: torch.Tensor) -> torch.Tensor:
    """7x7 box mean over the last two axes with scipy.ndimage's "reflect" border (half-sample symmetric: -1 -> 0, -2 -> 1;
    numpy's "symmetric", not torch's "reflect") -- ``uniform_filter(size=7)``."""
    H, W = x.shape[-2:]

    def sym(n):
        i = torch.arange(-3, n + 3, device=x.device)
        return torch.where(i < 0, -1 - i, torch.where(i >= n, 2 * n - 1 - i, i))

    x = x.index_select(-2, sym(H)).index_select(-1, sym(W))
    x = sum(x[..., k:k + H, :] for k in range(7))
    return sum(x[..., k:k + W] for k in range(7)) / 49.0


def masked_ssim(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor) -> float:
    """calculate_ssim (training.py:316-346) on [3,H,W] images: skimage 0.20 ``structural_similarity(full=True,
    channel_axis=2, data_range=2.0)`` restated in float64 -- per channel 7x7 box means with the symmetric border, sample
    covariance 49/48, C1 = (0.01*2)^2, C2 = (0.03*2)^2, the full map without a border crop -- then
    sum(S * mask) / (sum(mask) + 1e-8).  H or W below 7 raises ValueError, as skimage does."""
    assert img1.ndim == 3 and img2.ndim == 3 and img1.shape == img2.shape
    H, W = img1.shape[-2:]
    if H < 7 or W < 7:
        raise ValueError(f"masked_ssim: the image ({H} x {W}) is smaller than SSIM's 7 x 7 window")
    a, b, m = img1.double(), img2.double(), mask.double()
    assert float(a.min()) >= 0 and float(a.max()) <= 1 and float(b.min()) >= 0 and float(b.max()) <= 1
    ux, uy = _box7_sym(a), _box7_sym(b)
    uxx, uyy, uxy = _box7_sym(a * a), _box7_sym(b * b), _box7_sym(a * b)
    cov_norm = 49.0 / 48.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float((S * m).sum() / (m.sum() + 1e-8))


# ---------------------------------------------------------------- LPIPS (nsff_lpips, the NVIDIA protocol)
# AlexNet features[0:12] as pretrained_networks.py:63-105 slices them: (features index, kernel, stride, padding, pool before)
_ALEX_CONVS = ((0, 11, 4, 2, False), (3, 5, 1, 2, True), (6, 3, 1, 1, True), (8, 3, 1, 1, False), (10, 3, 1, 1, False))
_ALEX_SHAPES = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
# the ScalingLayer (networks_basic.py:145-157) the NVIDIA protocol never applies (see masked_lpips)
_LPIPS_SHIFT = (-0.030, -0.088, -0.188)
_LPIPS_SCALE = (0.458, 0.448, 0.450)


def _strip_module(sd: dict) -> dict:
    return {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}


class LpipsAlex:
    """The weights of LPIPS v0.1 with the AlexNet backbone, on one device: ``features.{0,3,6,8,10}.{weight,bias}`` of
    torchvision's ``alexnet`` and the five ``lin{k}.model.1.weight`` of ``nsff_lpips/weights/v0.1/alex.pth``.  Only the keys
    it uses are read, and each must be present with its exact shape (other keys, e.g. the classifier's, are ignored).
    ``backbone`` may also be in the reference's layout (a ``PNetLin`` state dict: ``net.slice{s}.{i}.*``, optionally with
    ``module.`` prefixes), which then may carry the lin weights too.  Also holds the three packed buffers the C ABI takes."""

    def __init__(self, backbone: dict, lin: dict = None, device="cpu"):
        bb, ln = _strip_module(dict(backbone)), _strip_module(dict(lin)) if lin is not None else {}
        slices = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}  # features index -> PNetLin slice

        def pick(sd, names, what):
            for n in names:
                if n in sd:
                    return torch.as_tensor(sd[n]).detach().to("cpu", torch.float32)
            raise KeyError(f"LpipsAlex: {what} not found (looked for {', '.join(names)})")

        self.convs, self.lins = [], []
        for (i, *_), (co, ci, k) in zip(_ALEX_CONVS, _ALEX_SHAPES):
            for kind, shape in (("weight", (co, ci, k, k)), ("bias", (co,))):
                t = pick(bb, (f"features.{i}.{kind}", f"net.slice{slices[i]}.{i}.{kind}"), f"backbone {kind} of features.{i}")
                if tuple(t.shape) != shape:
                    raise ValueError(f"LpipsAlex: features.{i}.{kind} has shape {tuple(t.shape)}, expected {shape}")
                self.convs.append(t)
        for k, (co, _, _) in enumerate(_ALEX_SHAPES):
            t = pick(ln if ln else bb, (f"lin{k}.model.1.weight",), f"lin{k}.model.1.weight")
            if tuple(t.shape) != (1, co, 1, 1):
                raise ValueError(f"LpipsAlex: lin{k}.model.1.weight has shape {tuple(t.shape)}, expected {(1, co, 1, 1)}")
            self.lins.append(t)
        d = torch.device(device)
        self._move(torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d)

    def _pack(self):
        self.conv_weights = torch.cat([w.reshape(-1) for w in self.convs[0::2]])
        self.conv_biases = torch.cat(self.convs[1::2])
        self.lin_weights = torch.cat([w.reshape(-1) for w in self.lins])

    def _move(self, device):
        self.convs = [t.to(device) for t in self.convs]
        self.lins = [t.to(device) for t in self.lins]
        self._pack()
        self.device = device
        self._copies = {device: self}

    def on(self, device) -> "LpipsAlex":
        """these weights on ``device``: self, or a copy made once and kept"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        c = self._copies.get(device)
        if c is None:
            c = LpipsAlex.__new__(LpipsAlex)
            c.convs, c.lins = self.convs, self.lins
            c._move(device)
            self._copies[device] = c
        return c

    @classmethod
    def from_files(cls, backbone_path, lin_path, device="cpu"):
        """torchvision's AlexNet checkpoint (``alexnet-owt-*.pth``) and the reference's ``weights/v0.1/alex.pth`` (saved
        with CUDA storages: loaded with ``map_location="cpu"``)."""
        bb = torch.load(str(backbone_path), map_location="cpu", weights_only=True)
        ln = torch.load(str(lin_path), map_location="cpu", weights_only=True) if lin_path is not None else None
        return cls(bb, ln, device)

    @classmethod
    def from_engine_cfg(cls, engine_cfg, device="cpu"):
        """``engine_cfg.lpips_weights: {backbone: <path>, lin: <path>}`` (configs/engine/evaluator_pgdvs.yaml) -> an
        ``LpipsAlex``, or None when the key is absent or null (LPIPS then stays off)."""
        spec = engine_cfg.get("lpips_weights", None) if hasattr(engine_cfg, "get") else getattr(engine_cfg, "lpips_weights", None)
        if not spec:
            return None
        return cls.from_files(spec["backbone"], spec["lin"], device)


def alex_features(x: torch.Tensor, weights: LpipsAlex):
    """relu1..relu5 of AlexNet ``features[0:12]`` for a batch x[N,3,H,W] (float32 torch; pretrained_networks.py:63-105)."""
    w = weights.on(x.device)
    feats, h = [], x
    for j, (_, k, st, pd, pool) in enumerate(_ALEX_CONVS):
        if pool:
            h = F.max_pool2d(h, kernel_size=3, stride=2)
        h = F.relu(F.conv2d(h, w.convs[2 * j], w.convs[2 * j + 1], stride=st, padding=pd))
        feats.append(h)
    return feats


def _lpips_layers(x, weights, scaling_layer):
    """LPIPS's per-layer distance maps of image pairs x[2n,3,H,W] in [0,1] (pair i = x[2i] vs x[2i+1]): 2 x - 1 (modify_rgb_range
    "0_1" -> "-1_1", utils/rendering.py:26-77; im2tensor's x / 0.5 - 1 is the same exact map), optionally the ScalingLayer,
    AlexNet relu1..5, normalize_tensor, the squared difference and the 1x1 lin_k -> one [n,1,h,w] map per layer"""
    x = 2.0 * x - 1.0
    if scaling_layer:
        shift = torch.tensor(_LPIPS_SHIFT, dtype=torch.float32, device=x.device)[None, :, None, None]
        scale = torch.tensor(_LPIPS_SCALE, dtype=torch.float32, device=x.device)[None, :, None, None]
        x = (x - shift) / scale
    diffs = []
    for f, lin in zip(alex_features(x, weights), weights.on(x.device).lins):
        f = f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)  # normalize_tensor
        diffs.append(F.conv2d((f[0::2] - f[1::2]) ** 2, lin))
    return diffs


def _lpips_torch(img1, img2, masks, weights, scaling_layer=False):
    """LPIPS of [3,H,W] images in [0,1] for each of ``masks`` ([C,H,W], channel 0 used), the backbone run once."""
    H, W = img1.shape[-2:]
    if H < 31 or W < 31:
        raise ValueError(f"masked_lpips: the image ({H} x {W}) is smaller than AlexNet's 31 x 31 minimum (relu5 would be empty)")
    diffs = _lpips_layers(torch.stack([img1, img2]).float(), weights, scaling_layer)
    out = []
    for m in masks:
        m = m[None, 0:1].float().to(img1.device)
        val = None
        for d in diffs:  # spatial_average (networks_basic.py:15-25), then the sum over layers (:134-136)
            mr = F.interpolate(m, size=[d.shape[2], d.shape[3]])
            r = torch.sum(d * mr) / (torch.sum(mr) + 1e-8)
            val = r if val is None else val + r
        out.append(float(val))
    return out


def masked_lpips(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor, weights: LpipsAlex, *, scaling_layer: bool = False) -> float:
    """The evaluator's ``lpips_fn.forward(gt, pred, mask)`` (evaluator_pgdvs.py:190-283 with trainer_pgdvs.py:132-137) on
    [3,H,W] images in [0,1] (already quantised) restated in float32 torch: 2 x - 1, AlexNet relu1..5 (``F.conv2d``,
    ``F.max_pool2d``), normalize_tensor, squared difference, the 1x1 lin_k, then sum(x m) / (sum(m) + 1e-8) per layer with
    the mask's channel 0 ``F.interpolate``d (nearest) to the layer, summed over the layers.  The reference never applies its
    ScalingLayer on this protocol: ``PNetLin.forward`` tests ``self.version == "0.1"`` (a string) while the evaluator passes
    ``version=0.1`` (a float), networks_basic.py:94-99 -- kept here as the ``masked_psnr`` quirk is; ``scaling_layer=True``
    applies it (only to show that the difference is visible).  H or W below 31 raises ValueError (relu5 would be empty)."""
    assert img1.ndim == 3 and img2.ndim == 3 and img1.shape == img2.shape
    return _lpips_torch(img1, img2, [mask], weights, scaling_layer=scaling_layer)[0]


# ---------------------------------------------------------------- the DyCheck iPhone protocol (quant_type "dycheck_iphone")
# obtain_quantitative_dycheck_iphone (evaluator_pgdvs.py:282-409) through pgdvs/utils/dycheck/metrics.py:63-230: PSNR, SSIM and
# LPIPS per view with a full mask and with the covisibility mask eval_mask[H,W,1].  The restatements below take [3,H,W] images
# in [0,1] (already quantised) and a [1,H,W] (or [H,W]) mask, work in float32 torch elementwise and reduce in float64.
QUANT_TYPES = ("nvidia", "dycheck_iphone")


def _mask_hw(mask: torch.Tensor) -> torch.Tensor:
    return (mask[0] if mask.ndim == 3 else mask).float()


def masked_psnr_dycheck(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor) -> float:
    """compute_psnr (metrics.py:63-90): -10/ln 10 ln(masked_mean(d^2, m)), masked_mean = sum(x m) / max(sum(m broadcast to the
    three channels), 1e-6).  An exact match -- or an empty mask, 0 / 1e-6 -- gives +inf, as upstream."""
    a, b, m = img1.float(), img2.float(), _mask_hw(mask).to(img1.device)
    d2 = (a - b) ** 2
    num = float((d2 * m).double().sum())
    den = max(3.0 * float(m.double().sum()), 1e-6)
    mse = num / den
    return math.inf if mse == 0 else -10.0 / math.log(10.0) * math.log(mse)


def dycheck_filter(device="cpu") -> torch.Tensor:
    """metrics.py:148-153: the 11-tap Gaussian, sigma 1.5, normalised to sum 1 (float64, rounded once to float32)"""
    f = torch.exp(-0.5 * ((torch.arange(11, dtype=torch.float64) - 5) / 1.5) ** 2)
    return (f / f.sum()).float().to(device)


def _partial_conv(z: torch.Tensor, m: torch.Tensor, f: torch.Tensor, dim: int):
    """one pass of metrics.py:155-168 along ``dim`` (-1 = W, -2 = H) of z[C,H,W] with the shared mask m[H,W], mode "valid":
    z' = conv(z m, f) 11 / conv(m, 1) where conv(m, 1) != 0, else 0; returns (z', conv(m, 1) != 0)"""
    zu = (z * m).unfold(dim, 11, 1)  # [..., 11] windows
    mu = m.unfold(dim, 11, 1)
    zc = (zu * f).sum(-1)
    mc = mu.sum(-1)
    return torch.where(mc != 0, zc * 11.0 / mc, torch.zeros_like(zc)), (mc != 0).float()


def masked_ssim_dycheck(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor) -> float:
    """compute_ssim (metrics.py:93-186, modelled on tf.image.ssim): the five moments through the separable partial convolution
    (W pass, then H pass), variances clamped at 0, the covariance clipped to sign(s01) min(sqrt(s00 s11), |s01|), k1 = 0.01,
    k2 = 0.03, max_val 1, then the mean over ALL (H-10)(W-10) 3 entries of the map (a window without mask contributes 1:
    an empty mask gives 1).  H or W below 11 raises ValueError (upstream's mean of an empty map is NaN)."""
    H, W = img1.shape[-2:]
    if H < 11 or W < 11:
        raise ValueError(f"masked_ssim_dycheck: the image ({H} x {W}) is smaller than SSIM's 11 x 11 window")
    a, b, m = img1.float(), img2.float(), _mask_hw(mask).to(img1.device)
    f = dycheck_filter(a.device)

    def filt(z):
        z1, m1 = _partial_conv(z, m, f, -1)
        return _partial_conv(z1, m1, f, -2)[0]

    mu0, mu1 = filt(a), filt(b)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = torch.clamp(filt(a * a) - mu00, min=0.0)
    s11 = torch.clamp(filt(b * b) - mu11, min=0.0)
    s01 = filt(a * b) - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), torch.abs(s01))
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return float(S.double().mean())


def _lpips_dycheck_torch(img1, img2, masks, weights):
    """lpips 0.1.4 LPIPS(net="alex", spatial=True) as compute_lpips (metrics.py:189-230) calls it, for each of ``masks``
    ([H,W] each): the pair (img1 m, img2 m) -> im2tensor(factor=1/2) -> ScalingLayer -> AlexNet -> per layer normalize_tensor,
    squared difference, lin_k, bilinear upsampling to H x W (align_corners=False, by size), summed; then masked_mean with m."""
    H, W = img1.shape[-2:]
    if H < 31 or W < 31:
        raise ValueError(f"masked_lpips_dycheck: the image ({H} x {W}) is smaller than AlexNet's 31 x 31 minimum (relu5 would be empty)")
    ms = [m.float().to(img1.device) for m in masks]
    val = None
    for d in _lpips_layers(torch.stack([t for m in ms for t in (img1.float() * m, img2.float() * m)]), weights, True):
        up = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
        val = up if val is None else val + up
    return [float((val[i, 0] * m).double().sum() / max(float(m.double().sum()), 1e-6)) for i, m in enumerate(ms)]


def masked_lpips_dycheck(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor, weights: LpipsAlex) -> float:
    """compute_lpips (metrics.py:189-230) on [3,H,W] images in [0,1] (already quantised) and a [1,H,W] mask, restated in float32
    torch: the images are multiplied by the mask BEFORE the network, mapped by 2 x - 1 and the ScalingLayer (applied here:
    LPIPS's version is the string "0.1"), AlexNet relu1..5, normalize_tensor, squared difference, lin_k, each layer's map
    upsampled bilinearly to H x W and summed, then sum(v m) / max(sum(m), 1e-6).  The full-mask value is this with m = 1.
    H or W below 31 raises ValueError."""
    assert img1.ndim == 3 and img2.ndim == 3 and img1.shape == img2.shape
    return _lpips_dycheck_torch(img1, img2, [_mask_hw(mask)], weights)[0]


def quant_type_from_engine_cfg(engine_cfg) -> str:
    """``engine_cfg.quant_type`` (configs/engine/evaluator_pgdvs.yaml; "nvidia" when absent) -> the ``quant_type`` of
    ``eval_step``.  An unknown value raises ValueError, as trainer_pgdvs.py:86-91 does."""
    q = engine_cfg.get("quant_type", "nvidia") if hasattr(engine_cfg, "get") else getattr(engine_cfg, "quant_type", "nvidia")
    if q not in QUANT_TYPES:
        raise ValueError(q)
    return q


def to_device(batch: dict, device) -> dict:
    """``_to_gpu_func`` (pgdvs/engines/abstract.py:153-157): tensors move, everything else passes through"""
    return {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}


METRIC_KEYS = ("psnr_full_combined", "psnr_dyn_combined", "psnr_static_combined")
SSIM_KEYS = ("ssim_full_combined", "ssim_dyn_combined", "ssim_static_combined")  # eval_step(..., with_ssim=True)
LPIPS_KEYS = ("lpips_full_combined", "lpips_dyn_combined", "lpips_static_combined")  # eval_step(..., lpips=LpipsAlex(...))

DYCHECK_KEYS = ("psnr_combined", "ssim_combined", "mpsnr_combined", "mssim_combined")  # eval_step(..., quant_type="dycheck_iphone")
DYCHECK_LPIPS_KEYS = ("lpips_combined", "mlpips_combined")  # ... and lpips=LpipsAlex(...)

# measurement hook (bench.py): a dict set here accumulates the host wall time of eval_step's stages in seconds
# ("to_device", "forward" = enqueue of the renderer, "metric_enqueue", "sync_read" = the step's one wait for the GPU,
# "post"); None = no timing
STAGE_SECONDS = None


def _check_geo_status(ret, data_gpu, host_counts=None, host_status=None):
    """Device-side status words of the geometry path (eval_step and vis_step wait for the GPU anyway): a static cloud whose
    aggregation reported an error (count -1), filled its buffer (rows may have been dropped: the aggregation clamps at its
    capacity) or outgrew the rasteriser's row bound would otherwise show up as a silently blank or truncated static image.
    host_counts / host_status: the words as eval_step already read them back with its metric sums."""
    from . import ops

    cnts = ret.get("st_pcl_rgb_count", data_gpu.get("st_pcl_rgb_count", None))
    if isinstance(cnts, torch.Tensor):
        cloud = ret.get("st_pcl_rgb", None)
        values = host_counts if host_counts is not None else [int(c.item()) for c in cnts.reshape(-1)]
        for n in values:
            if n < 0:
                raise ops.PgdvsHipError(f"st_pcl_rgb_count: device-side error flag set (count {n}); the output is not valid")
            limited = cloud is not None and "_st_pcl_video" in data_gpu and cloud.shape[1] < data_gpu["_st_pcl_video"]["depths"].numel()
            if limited and n >= cloud.shape[1]:
                raise ops.PgdvsHipError(f"the aggregated static cloud filled its buffer of {cloud.shape[1]} rows (capacity-limited): "
                                        "rows may have been dropped -- pass a larger capacity")
    if host_status is not None:
        ops.check_raster_status(torch.tensor(host_status, dtype=torch.int32))
    else:
        ops.check_raster_status(ret.get("geo_static_raster_status", None))


class _Laps:
    """STAGE_SECONDS bookkeeping shared by the two halves of a step: ``lap(name)`` adds the host wall time since the last lap"""

    def __init__(self):
        self.stages, self.t_prev = STAGE_SECONDS, time.perf_counter()

    def __call__(self, name):
        if self.stages is not None:
            now = time.perf_counter()
            self.stages[name] = self.stages.get(name, 0.0) + (now - self.t_prev)
            self.t_prev = now


def _check_protocol(what, quant_type, with_ssim):
    if quant_type not in QUANT_TYPES:
        raise ValueError(quant_type)
    if quant_type == "dycheck_iphone" and with_ssim:
        raise ValueError(f"{what}: with_ssim does not apply to quant_type 'dycheck_iphone' (its SSIM is always computed)")


class _LazyRing:
    """the cached ``ops.RowRing`` of ``depth`` blocks for the device of the first rows enqueued (``eval_step``: depth 1, the
    staging of ``ops.read_back_rows``; ``eval_run``: run_ahead + 1)"""

    def __init__(self, depth=1):
        self.depth, self.ring = depth, None

    def enqueue(self, rows):
        if self.ring is None:
            from . import ops

            self.ring = ops.row_ring(rows[0].device, self.depth)
        return self.ring.enqueue(rows)

    def finish(self, ticket):
        return self.ring.finish(ticket)


class _PendingStep:
    """What ``_eval_enqueue`` leaves for ``_eval_finish``: on the fused path the enqueued rows' ticket in the row ring, on the
    torch path the finished per-view values"""
    __slots__ = ("fused", "n_batch", "keys", "device", "ret", "data", "data_gpu", "groups", "ticket", "ring", "images", "has_cnts",
                 "has_stat", "per_view", "pred", "gt", "eval_mask", "exports")


def _eval_enqueue(what, model, data, render_cfg, *, device, disable_tqdm, with_ssim, lpips, quant_type, want_images, ring, lap,
                  export=False):
    """The first half of an evaluator step: to-device, ``forward`` and, on the fused GPU path, the protocol's HIP passes per
    view and the asynchronous copy of their rows into ``ring`` (``ops.RowRing``) -- nothing here waits for the GPU.  On the
    torch path (CPU tensors, render size != ground-truth size) the whole step is computed here.  ``export``: also the
    scanlines of the view's images (``save_individual``), on the fused path one ``ops.eval_export_scanlines`` launch per view
    behind the metric passes, each with an event a ``PngWriter`` can wait for."""
    from . import ops

    _check_protocol(what, quant_type, with_ssim)
    if quant_type == "dycheck_iphone" and data["eval_mask"].shape[-1] != 1:
        raise ValueError(f"{what}: quant_type 'dycheck_iphone' takes eval_mask[B,H,W,1], got {tuple(data['eval_mask'].shape)}")
    device = device if device is not None else next(iter(v for v in data.values() if isinstance(v, torch.Tensor))).device
    data_gpu = to_device(data, device)
    lap("to_device")
    if model.training:
        model.eval()
    n_batch = data["rgb_src_temporal"].shape[0]
    ret = model.forward(data_gpu, render_cfg=render_cfg, disable_tqdm=disable_tqdm, for_debug=False)
    lap("forward")
    comb, gt, em = ret["combined_rgb"], data_gpu["rgb_tgt"], data_gpu["eval_mask"]
    if quant_type == "dycheck_iphone":
        keys, fused_rows, view_values = DYCHECK_KEYS + (DYCHECK_LPIPS_KEYS if lpips is not None else ()), _dycheck_rows, _dycheck_view
    else:
        keys = METRIC_KEYS + (SSIM_KEYS if with_ssim else ()) + (LPIPS_KEYS if lpips is not None else ())
        fused_rows, view_values = _nvidia_rows, _nvidia_view
    pend = _PendingStep()
    pend.n_batch, pend.keys, pend.ret, pend.data, pend.data_gpu, pend.exports = n_batch, keys, ret, data, data_gpu, None
    statics = [(tag, ret[k]) for tag, k in (("gnt", "static_coarse_rgb"), ("geo_static", "geo_static_rgb")) if k in ret]
    pend.fused = bool(comb.is_cuda and comb.dtype == torch.float32 and tuple(comb.shape[2:]) == tuple(gt.shape[1:3])
                      and gt.dtype == torch.float32 and em.dtype == torch.float32)
    if pend.fused:
        # GPU, render size == ground-truth size (render_stride 1): the protocol's HIP passes per view, the first of which
        # quantises and carries the geometry path's device-side status words, and ONE host read for the batch
        cnts = ret.get("st_pcl_rgb_count", data_gpu.get("st_pcl_rgb_count", None))
        cnts = cnts.reshape(-1) if isinstance(cnts, torch.Tensor) and cnts.is_cuda and cnts.dtype == torch.int64 else None
        stat = ret.get("geo_static_raster_status", None)
        stat = stat.reshape(-1) if isinstance(stat, torch.Tensor) and stat.is_cuda and stat.dtype == torch.int32 else None
        cd = [cnts[i_b:i_b + 1] if (cnts is not None and i_b < cnts.numel()) else None for i_b in range(n_batch)]
        sd = [stat[i_b:i_b + 1] if (stat is not None and i_b < stat.numel()) else None for i_b in range(n_batch)]
        pend.groups, pend.images = fused_rows(comb, gt, em, cd, sd, with_ssim, lpips, want_images)
        pend.has_cnts, pend.has_stat, pend.device, pend.eval_mask = cnts is not None, stat is not None, comb.device, em
        lap("metric_enqueue")
        pend.ring = ring
        pend.ticket = ring.enqueue([r_ for rows, _ in pend.groups for r_ in rows])
        if export:
            pend.exports = []
            # the first static image that fits rides in the view's export launch; another one (a renderer that returns both)
            # takes a png_scanlines launch of its own
            fast = [(tag, img) for tag, img in statics if img.is_cuda and img.dtype == torch.float32 and img.shape == comb.shape][:1]
            for i_b in range(n_batch):
                scan = ops.eval_export_scanlines(comb[i_b], gt[i_b], fast[0][1][i_b] if fast else None)
                views = [("gt", scan[0]), ("combined", scan[1])] + ([(fast[0][0], scan[2])] if fast else [])
                views += [(tag, _view_scanlines(img[i_b:i_b + 1], "truncate")[0]) for tag, img in statics if not fast or tag != fast[0][0]]
                pend.exports.append((views, torch.cuda.current_stream(comb.device).record_event()))
        return pend
    _check_geo_status(ret, data_gpu)
    # quantise first, as if the images had been written to disk and read back (:70-77)
    pred = quantize_like_evaluator(comb)
    rgb_gt = quantize_like_evaluator(gt.permute(0, 3, 1, 2))
    eval_mask = em.permute(0, 3, 1, 2)
    _, _, rh, rw = pred.shape
    if rgb_gt.shape[2] != rh or rgb_gt.shape[3] != rw:  # render_stride != 1 (:80-92)
        rgb_gt = torch.nn.functional.interpolate(rgb_gt, size=(rh, rw), mode="bicubic", antialias=True, align_corners=True)
        eval_mask = torch.nn.functional.interpolate(eval_mask, size=(rh, rw), mode="nearest")
        eval_mask = (eval_mask > 0).float()
    vals = [view_values(rgb_gt[i_b], pred[i_b].to(rgb_gt.device), eval_mask[i_b], with_ssim, lpips) for i_b in range(n_batch)]
    pend.per_view = {k: [v[j] for v in vals] for j, k in enumerate(keys)}
    pend.pred, pend.gt, pend.eval_mask, pend.device = pred, rgb_gt, eval_mask, rgb_gt.device
    if export:  # the evaluator's own images, quantised (and, with render_stride != 1, the resized ground truth) (:432-465)
        outs = [("gt", rgb_gt), ("combined", pred)] + statics
        lines = [(tag, _view_scanlines(img.float().cpu(), "truncate")) for tag, img in outs]
        pend.exports = [([(tag, scan[i_b]) for tag, scan in lines], None) for i_b in range(n_batch)]
    return pend


def _eval_finish(pend, lap):
    """The second half: the step's one wait for the GPU (its own block of the row ring), the status words, the per-view
    values in key order -> ``{key: [value per view]}``.  Raises ``PgdvsHipError`` on a device-side status error."""
    if not pend.fused:
        return pend.per_view
    n_batch = pend.n_batch
    host = pend.ring.finish(pend.ticket)  # (the step's synchronisation)
    lap("sync_read")
    _check_geo_status(pend.ret, pend.data_gpu, host_counts=[int(s_[6]) for s_ in host[:n_batch]] if pend.has_cnts else None,
                      host_status=[int(s_[7]) for s_ in host[:n_batch]] if pend.has_stat else None)
    vals = [[v for j, (_, values) in enumerate(pend.groups) for v in values(host[j * n_batch + i_b])] for i_b in range(n_batch)]
    pend.per_view = {k: [v[j] for v in vals] for j, k in enumerate(pend.keys)}
    return pend.per_view


def _multi_process():
    return torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1


@torch.no_grad()
def eval_step(model, data: dict, render_cfg, *, device=None, disable_tqdm=True, return_images=False, with_ssim=False,
              lpips=None, quant_type="nvidia"):
    """One evaluator step on a batch of target views.  ``data`` is the reference's data dict (row A0) plus
    ``rgb_tgt[B,H,W,3]`` and ``eval_mask[B,H,W,3]`` (1 = dynamic region).  Returns the reference's
    ``metric_dict`` restricted to the in-scope keys: ``eval/count`` (int64) and the per-key SUMS over the
    batch (float32), reduced to rank 0 when a process group is up (device tensors then, as upstream; in a single process
    HOST tensors on both the fused GPU path and the torch path, so that a caller who accumulates them over steps never
    mixes devices).  ``with_ssim`` adds the three masked SSIM sums (``SSIM_KEYS``, float32, reduced in the same packed
    block).  ``lpips`` (an ``LpipsAlex``) adds the three masked LPIPS values (``LPIPS_KEYS``, float32, in the same block).
    With ``return_images`` also the quantised prediction / ground truth and the per-view values.
    ``quant_type`` selects the evaluator's metric protocol (evaluator_pgdvs.py:137-143; ``quant_type_from_engine_cfg``): the
    default "nvidia" is all of the above; "dycheck_iphone" returns ``eval/count`` and ``DYCHECK_KEYS`` instead -- plus
    ``DYCHECK_LPIPS_KEYS`` with ``lpips`` -- for an ``eval_mask[B,H,W,1]`` (csrc/eval_dycheck.hip on the fused path).  There
    SSIM is always on, so ``with_ssim=True`` raises ValueError, as does an eval_mask whose last dimension is not 1.
    The step is ``_eval_enqueue`` followed at once by ``_eval_finish``; ``eval_run`` drives the same two halves with the
    second up to three steps behind the first."""
    lap = _Laps()
    pend = _eval_enqueue("eval_step", model, data, render_cfg, device=device, disable_tqdm=disable_tqdm, with_ssim=with_ssim,
                         lpips=lpips, quant_type=quant_type, want_images=return_images, ring=_LazyRing(1), lap=lap)
    per_view = _eval_finish(pend, lap)
    # (a single process keeps the metric tensors on the host: no upload and no one-element kernels per step)
    metric = _metric_dict(pend.n_batch, pend.keys, per_view, pend.device, _multi_process())
    if not pend.fused:
        if return_images:
            return metric, {"pred": pend.pred, "gt": pend.gt, "eval_mask": pend.eval_mask, "per_view": per_view, "ret": pend.ret}
        return metric
    lap("post")
    if return_images:
        pred, gtq = pend.images()
        return metric, {"pred": pred, "gt": gtq, "eval_mask": pend.eval_mask.permute(0, 3, 1, 2), "per_view": per_view, "ret": pend.ret}
    return metric


def _metric_dict(n_batch, keys, per_view, device, multi):
    """eval/count and the per-key float32 sums: host tensors in a single process, one packed reduce to rank 0 otherwise"""
    if not multi:
        metric = {"eval/count": torch.tensor([n_batch], dtype=torch.int64)}
        for k in keys:
            metric[f"eval/{k}"] = torch.tensor(per_view[k], dtype=torch.float32).sum()
        return metric
    # one packed reduce instead of one collective per key: [count, sums...] in float64 on the device
    packed = torch.tensor([float(n_batch)] + [float(torch.tensor(per_view[k], dtype=torch.float32).sum()) for k in keys],
                          dtype=torch.float64, device=device)
    packed = pdist.reduce_metrics(packed, dst=0)
    metric = {"eval/count": packed[:1].round().to(torch.int64)}
    for j, k in enumerate(keys):
        metric[f"eval/{k}"] = packed[1 + j].to(torch.float32)
    return metric


# Each protocol's part of eval_step.  *_rows (the fused path) enqueues the protocol's rows for every view -> ([(the views' rows,
# host row -> that row's values in key order)], () -> the quantised pred / gt [B,3,H,W] for return_images); *_view (the torch
# path) is one view's values in key order from quantised gt / pred [3,H,W] and eval_mask [C,H,W].
def _nvidia_rows(comb, gt, em, cd, sd, with_ssim, lpips, want_images):
    """csrc/eval.hip: quantisation and the three masked PSNR sums of a view in one pass; then SSIM (csrc/eval_ssim.hip) and
    LPIPS (csrc/lpips.hip: the backbone runs once per image per view, for all three masks) on request"""
    from . import ops

    n = comb.shape[0]
    psnr = [ops.eval_psnr_sums(comb[i], gt[i], em[i], want_images=want_images, count_dev=cd[i], status_dev=sd[i]) for i in range(n)]

    def psnr_values(s_):
        mses = [s_[j] / (s_[3 + j] + 1e-8) for j in range(3)]
        return [0 if mse == 0 else 10 * math.log10(1.0 / mse) for mse in mses]

    groups = [([r_[0] for r_ in psnr], psnr_values)]
    if with_ssim:
        groups.append(([ops.eval_ssim_sums(comb[i], gt[i], em[i])[0] for i in range(n)],
                       lambda s_: [s_[j] / (s_[3 + j] + 1e-8) for j in range(3)]))
    if lpips is not None:  # (the LPIPS row carries the finished values: include/pgdvs_hip.h)
        w = lpips.on(comb.device)
        groups.append(([ops.lpips_sums(comb[i], gt[i], em[i], w)[0] for i in range(n)], lambda s_: s_[:3]))
    return groups, lambda: (torch.stack([r_[1] for r_ in psnr]), torch.stack([r_[2] for r_ in psnr]))


def _nvidia_view(g, p, m_dyn, with_ssim, lpips):
    # calculate_psnr asserts on [0,1] inputs; a bicubically resized ground truth can overshoot, as upstream
    masks = [torch.ones_like(g), m_dyn, 1.0 - m_dyn]
    vals = [masked_psnr(g, p, m) for m in masks]
    if with_ssim:
        vals += [masked_ssim(g, p, m) for m in masks]
    if lpips is not None:
        vals += _lpips_torch(g, p, masks, lpips)
    return vals


def _dycheck_rows(comb, gt, em, cd, sd, with_ssim, lpips, want_images):
    """obtain_quantitative_dycheck_iphone (evaluator_pgdvs.py:282-409): one PSNR + SSIM pass per view (csrc/eval_dycheck.hip),
    the LPIPS pass on request"""
    from . import ops

    n = comb.shape[0]
    n_map = 3.0 * (comb.shape[2] - 10) * (comb.shape[3] - 10)
    to_db = lambda s_, n_: math.inf if s_ / max(n_, 1e-6) == 0 else -10.0 / math.log(10.0) * math.log(s_ / max(n_, 1e-6))  # noqa: E731
    groups = [([ops.dycheck_psnr_ssim_sums(comb[i], gt[i], em[i], count_dev=cd[i], status_dev=sd[i]) for i in range(n)],
               lambda s_: [to_db(s_[0], s_[3]), s_[2] / n_map, to_db(s_[1], s_[4]), s_[5] / n_map])]
    if lpips is not None:
        w = lpips.on(comb.device)
        groups.append(([ops.dycheck_lpips(comb[i], gt[i], em[i], w) for i in range(n)], lambda s_: s_[:2]))
    return groups, lambda: (quantize_like_evaluator(comb), quantize_like_evaluator(gt.permute(0, 3, 1, 2)))


def _dycheck_view(g, p, mask, with_ssim, lpips):
    m = mask[0]
    ones = torch.ones_like(m)
    vals = [masked_psnr_dycheck(g, p, ones), masked_ssim_dycheck(g, p, ones), masked_psnr_dycheck(g, p, m), masked_ssim_dycheck(g, p, m)]
    if lpips is not None:
        vals += _lpips_dycheck_torch(g, p, [ones, m], lpips)
    return vals


# ---- the visualiser's loop (pgdvs/engines/visualizer_pgdvs.py:29-152) ----------------------------------------------------
def _view_scanlines(img: torch.Tensor, quant: str):
    """img[B,3,H,W] -> scanlines [B,H,1+3W] uint8: one HIP pass on a GPU float32 image (csrc/png.hip), png.py's torch / numpy
    path otherwise"""
    from . import png

    if img.is_cuda and img.dtype == torch.float32:
        from . import ops

        return ops.png_scanlines(img, quant=quant, adaptive=True)
    return png.filter_scanlines(png.QUANTIZERS[quant](img).permute(0, 2, 3, 1).contiguous().cpu(), adaptive=True)


def _video_frames(img: torch.Tensor, writer):
    """img[B,3,H,W] -> what ``MjpegWriter.submit`` takes per view: for a GPU float32 batch the ``DeviceScan`` views of ONE
    ``ops.jpeg_encode`` (csrc/jpeg.hip) behind one event, the host images otherwise"""
    if not (img.is_cuda and img.dtype == torch.float32):
        return list(img.float().cpu())
    from . import ops, video

    data, nbytes = ops.jpeg_encode(img, quality=writer.quality, restart_mcus=writer.restart_mcus, subsampling=writer.subsampling)
    ready = torch.cuda.current_stream(img.device).record_event()
    return [video.DeviceScan(data[i], nbytes[i:i + 1], img.shape[2], img.shape[3], ready, writer.subsampling) for i in range(img.shape[0])]


@torch.no_grad()
def vis_step(model, data: dict, render_cfg, vis_dir, *, device=None, writer=None, disable_tqdm=True, return_ret=False, video=None):
    """The body of ``PGDVSVisualizer.vis_model``'s loop for one batch: to-device, ``forward`` under no_grad, the geometry
    path's status words checked as ``eval_step`` checks them, then per view ``vis_dir / split / scene_id /
    {tgt_idx:05d}_combined.png`` from ``combined_rgb`` (``torchvision.utils.save_image``'s quantisation) and, when the
    renderer returns ``static_coarse_rgb``, ``{tgt_idx:05d}_gnt.png`` from it (the truncating cast).  ``writer``: a
    ``png.PngWriter`` that copies, deflates and writes behind this thread (the files are complete once it is closed; one
    in device mode gets the view's images in one ``submit_batch``);
    without one the step writes each file before it returns.  ``video``: a ``video.MjpegWriter``; each view's ``combined_rgb``
    also becomes a frame of ``vis_dir / split / {scene_id}_combined.avi`` (upstream's ``_combined.mp4``, :141-177, as
    Motion-JPEG), written when that writer is closed: a GPU batch is compressed by one ``ops.jpeg_encode`` and the frames
    are fetched behind this thread, host images are encoded by the writer's workers.  Returns the paths of the PNGs (and
    ``ret`` with ``return_ret``)."""
    import pathlib

    from . import png

    device = device if device is not None else next(iter(v for v in data.values() if isinstance(v, torch.Tensor))).device
    data_gpu = to_device(data, device)
    if model.training:
        model.eval()
    ret = model.forward(data_gpu, render_cfg=render_cfg, disable_tqdm=disable_tqdm, for_debug=False)
    outputs = [("combined", ret["combined_rgb"], "save_image")]
    if "static_coarse_rgb" in ret:  # the pure GNT result (:127-139)
        outputs.append(("gnt", ret["static_coarse_rgb"], "truncate"))
    lines = [(tag, _view_scanlines(img, quant), int(img.shape[2]), int(img.shape[3])) for tag, img, quant in outputs]
    frames = _video_frames(ret["combined_rgb"], video) if video is not None else None
    _check_geo_status(ret, data_gpu)
    paths = []
    misc = data["misc"]
    for i_b in range(ret["combined_rgb"].shape[0]):
        scene_dir = pathlib.Path(vis_dir) / misc[i_b].get("split", "") / misc[i_b]["scene_id"]
        scene_dir.mkdir(parents=True, exist_ok=True)
        if frames is not None:
            video.submit((scene_dir.parent, misc[i_b]["scene_id"]), misc[i_b]["tgt_idx"], frames[i_b])
        view_paths = [scene_dir / f"{misc[i_b]['tgt_idx']:05d}_{tag}.png" for tag, _, _, _ in lines]
        if writer is not None and getattr(writer, "deflate", "zlib") == "device":
            writer.submit_batch(view_paths, [scan[i_b] for _, scan, _, _ in lines])  # one deflate call for the view's images
        else:
            for path, (tag, scan, h, w) in zip(view_paths, lines):
                if writer is not None:
                    writer.submit(path, scan[i_b])
                else:
                    png.write_file(path, scan[i_b].cpu().numpy() if isinstance(scan, torch.Tensor) else scan[i_b], h, w)
        paths += view_paths
    return (paths, ret) if return_ret else paths


def collate(batch: list) -> dict:
    """``default_collate_fn`` (pgdvs/engines/abstract.py:18-30): tensors stacked, floats and lists of floats to a tensor,
    everything else a list"""
    def combine(values):
        if isinstance(values[0], torch.Tensor):
            return torch.stack(values, dim=0)
        if isinstance(values[0], float) or (isinstance(values[0], list) and len(values[0]) > 0 and isinstance(values[0][0], float)):
            return torch.Tensor(values)
        return values

    return {k: combine([x[k] for x in batch]) for k in batch[0].keys()}


def _run_batches(what, dataset, batch_size, n_max_data, rank, world):
    """The item selection shared by ``vis_run`` and ``eval_run`` (run_eval_single_ckpt :290-331, vis_model): checks the
    arguments now, then yields this rank's collated batches: its items in ``DistributedSampler(shuffle=False)`` order
    (``dist.shard_indices``), ``batch_size`` per step, at most ``ceil(min(len(dataset), n_max_data) / (batch_size * world))``
    steps (``n_max_data <= 0``: all)."""
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"{what}: batch_size {batch_size}, rank {rank}, world {world}")
    n_all = min(len(dataset), n_max_data) if n_max_data > 0 else len(dataset)
    n_batches = int(math.ceil(n_all / (batch_size * world)))
    indices = pdist.shard_indices(len(dataset), rank, world)

    def batches():
        for step in range(min(n_batches, int(math.ceil(len(indices) / batch_size)))):
            yield collate([dataset[i] for i in indices[step * batch_size:(step + 1) * batch_size]])

    return batches()


def vis_run(model, dataset, render_cfg, vis_dir, *, batch_size=1, n_max_data=-1, rank=0, world=1, device=None, writer=None,
            video=False, video_fps=10, video_quality=90, png_deflate="zlib", video_subsampling="4:4:4"):
    """``vis_model``'s outer loop without Hydra: this rank's items in ``DistributedSampler(shuffle=False)`` order
    (``dist.shard_indices``), ``batch_size`` of them per step (the per-process batch size), collated as upstream collates
    them, at most ``ceil(min(len(dataset), n_max_data) / (batch_size * world))`` steps (``n_max_data <= 0``: all), each
    through ``vis_step``.  The files go through one ``png.PngWriter``: the given one, which stays open for its owner to
    close, or one made here -- ``png.PngWriter(deflate=png_deflate)``: "zlib", or "device" for the deflate in HIP
    (``ops.png_deflate``: the same pixels in files of other bytes); a given writer decides for itself -- and closed (every
    file complete) before the function returns.  Returns ``{scene_id: directory}``.

    ``video=True`` (or a ``video.MjpegWriter``, which is closed here): every view's ``combined_rgb`` also becomes a frame of
    ``<vis_dir>/<split or "">/<scene_id>_combined.avi`` at ``video_fps`` frames per second and libjpeg quality
    ``video_quality``, frames in ``tgt_idx`` order: upstream's ``_combined.mp4`` (:141-177) as Motion-JPEG, see
    ``pgdvs_amd/video.py``.  With ``world > 1`` each rank leaves hidden part files instead; under an initialised process
    group of that size the ranks then meet at a barrier and rank 0 merges them (``video.assemble``), without one call
    ``video.assemble(vis_dir, world)`` once every rank has returned.  ``video_subsampling``: "4:4:4", or "4:2:0" for chroma
    at half resolution in both directions, upstream's chroma format (its ffmpeg writer's yuv420p); a given writer decides for
    itself.  The default writes no video and nothing else changes."""
    from . import png
    from . import video as vid

    batches = _run_batches("vis_run", dataset, batch_size, n_max_data, rank, world)
    own = writer is None
    w = png.PngWriter(deflate=png_deflate) if own else writer
    mj = None
    if video is not None and video is not False:
        mj = vid.MjpegWriter(fps=video_fps, quality=video_quality, rank=rank, world=world,
                             subsampling=video_subsampling) if video is True else video
    dirs = {}
    try:
        for batch in batches:
            for path in vis_step(model, batch, render_cfg, vis_dir, device=device, writer=w, video=mj):
                dirs[path.parent.name] = path.parent
    finally:
        try:
            if own:
                w.close()
        finally:
            if mj is not None:
                mj.close()
    if mj is not None and mj.world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized() and (
            torch.distributed.get_world_size() == mj.world):
        torch.distributed.barrier()
        if mj.rank == 0:
            vid.assemble(vis_dir, mj.world)
        torch.distributed.barrier()
    return dirs


# ---- the evaluator's loop (pgdvs/engines/trainer_pgdvs.py:282-360, evaluator_pgdvs.py:115-175, 411-465) ------------------
# upstream's key order in a view's record (obtain_quantitative_nvidia :259-274, obtain_quantitative_dycheck_iphone :398-409)
RECORD_KEYS = {
    "nvidia": tuple(f"{m}_{r}_combined" for r in ("full", "dyn", "static") for m in ("psnr", "ssim", "lpips")),
    "dycheck_iphone": ("psnr_combined", "ssim_combined", "lpips_combined", "mpsnr_combined", "mssim_combined", "mlpips_combined"),
}
MAX_RUN_AHEAD = 3


def _write_record(path, info):
    import pickle

    from . import png

    png.atomic_write(path, pickle.dumps(info))


@torch.no_grad()
def eval_run(model, dataset, render_cfg, *, batch_size=1, n_max_data=-1, rank=0, world=1, device=None, quant_type="nvidia",
             with_ssim=False, lpips=None, save_individual=False, info_dir=None, vis_dir=None, writer=None, run_ahead=0, png_deflate="zlib") -> dict:
    """``run_eval_single_ckpt`` without Hydra: the items and steps of ``vis_run`` (``_run_batches``), each step the work of
    ``eval_step`` (same keys, protocols and errors), the per-step float32 sums accumulated as upstream accumulates them.
    Returns ``{"eval/count": int, "eval/<key>": the average (sum / count) as a float, ..., "sums": {"eval/count": int,
    "eval/<key>": float}, "records": [{"name": "<split>/<scene_id>/<fname>" (None without the ids), "info": the view's
    record}, ...]}``.  With ``world > 1`` the sums are reduced to rank 0 ONCE, at the end (``dist.reduce_metrics``; upstream
    reduces every step); the other ranks return their own partial sums and averages.
    ``save_individual`` (needs ``info_dir`` and ``vis_dir``) writes per view, with ``fname =
    f"{tgt_frame_id:05d}_cam_{tgt_cam_id:03d}"``, ``<info_dir>/<split>/<scene_id>/<fname>_rank_<rank>.pkl`` -- the pickled
    record: ``src_frame_ids``, then the view's values as Python floats under upstream's names in upstream's order, the
    metrics not asked for left out -- and ``<vis_dir>/<split>/<scene_id>/<fname>_gt.png``, ``_combined.png``, ``_gnt.png``
    (``static_coarse_rgb``) and ``_geo_static.png`` (``geo_static_rgb``) with upstream's pixels (NaN as 0), through ``writer``
    (a ``png.PngWriter``, left open) or one made and closed here (``png.PngWriter(deflate=png_deflate)``: "zlib", or
    "device" for the deflate in HIP, one ``ops.png_deflate`` call per view; a given writer decides for itself).  On the fused GPU path the scanlines are one
    ``ops.eval_export_scanlines`` launch per view, on the torch path ``png.py``'s.
    ``run_ahead`` = k (0..3): step j + k is enqueued before step j is finished; everything stays on the caller's stream in
    the same order, so every result is that of k = 0 and only the waiting moves.  (``STAGE_SECONDS``, when set, gets the loop's
    host time under ``eval_step``'s names, "post" including the records and the writer's submits.)  A status error of a view surfaces when the
    view is finished, up to k steps after it was enqueued: nothing later is finished or written, an owned writer is closed
    (the files of earlier views are complete) and the error is raised.  The torch path runs as k = 0."""
    import collections
    import pathlib

    from . import png

    _check_protocol("eval_run", quant_type, with_ssim)
    if not (isinstance(run_ahead, int) and 0 <= run_ahead <= MAX_RUN_AHEAD):
        raise ValueError(f"eval_run: run_ahead {run_ahead!r} (0 .. {MAX_RUN_AHEAD})")
    if save_individual and (info_dir is None or vis_dir is None):
        raise ValueError("eval_run: save_individual needs info_dir and vis_dir")
    batches = _run_batches("eval_run", dataset, batch_size, n_max_data, rank, world)
    if world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized() and (
            torch.distributed.get_world_size() != world or torch.distributed.get_rank() != rank):
        raise ValueError(f"eval_run: rank {rank} of world {world}, but the process group says rank {torch.distributed.get_rank()} of "
                         f"{torch.distributed.get_world_size()}")
    lap = _Laps()
    ring = _LazyRing(run_ahead + 1)
    if png_deflate not in png.DEFLATE_MODES:
        raise ValueError(f"eval_run: png_deflate {png_deflate!r} (one of {png.DEFLATE_MODES})")
    own = save_individual and writer is None
    w = png.PngWriter(deflate=png_deflate) if own else writer
    record_keys = RECORD_KEYS[quant_type]
    sums, records, pending = {}, [], collections.deque()
    out_device = [torch.device("cpu")]

    def finish(pend):
        per_view = _eval_finish(pend, lap)
        out_device[0] = pend.device
        step = _metric_dict(pend.n_batch, pend.keys, per_view, pend.device, False)
        for k_, v in step.items():  # (loss_sum[k] = loss_sum[k] + stats[k].cpu(), :341-343)
            sums[k_] = sums[k_] + v if k_ in sums else v
        misc = pend.data.get("misc", None)
        for i_b in range(pend.n_batch):
            info = {}
            if "seq_ids" in pend.data:
                info["src_frame_ids"] = pend.data["seq_ids"][i_b, 1:].cpu().numpy()
            info.update({k_: float(per_view[k_][i_b]) for k_ in record_keys if k_ in per_view})
            m = misc[i_b] if misc is not None else {}
            named = all(k_ in m for k_ in ("scene_id", "tgt_frame_id", "tgt_cam_id"))
            fname = f"{m['tgt_frame_id']:05d}_cam_{m['tgt_cam_id']:03d}" if named else None
            rel = pathlib.PurePosixPath(m.get("split", "")) / m["scene_id"] / fname if named else None
            records.append({"name": str(rel) if named else None, "info": info})
            if not save_individual:
                continue
            if not named:
                raise ValueError("eval_run: save_individual needs misc[i]['scene_id'], ['tgt_frame_id'] and ['tgt_cam_id']")
            scene_info = pathlib.Path(info_dir) / m.get("split", "") / m["scene_id"]
            scene_vis = pathlib.Path(vis_dir) / m.get("split", "") / m["scene_id"]
            scene_info.mkdir(parents=True, exist_ok=True)
            scene_vis.mkdir(parents=True, exist_ok=True)
            _write_record(scene_info / f"{fname}_rank_{rank}.pkl", info)
            views, ready = pend.exports[i_b]
            if getattr(w, "deflate", "zlib") == "device":
                w.submit_batch([scene_vis / f"{fname}_{tag}.png" for tag, _ in views], [scan for _, scan in views], ready=ready)
            else:
                for tag, scan in views:
                    w.submit(scene_vis / f"{fname}_{tag}.png", scan, ready=ready)
        lap("post")

    failed = False
    try:
        for batch in batches:
            pending.append(_eval_enqueue("eval_run", model, batch, render_cfg, device=device, disable_tqdm=True, with_ssim=with_ssim,
                                         lpips=lpips, quant_type=quant_type, want_images=False, ring=ring, lap=lap,
                                         export=save_individual))
            depth = run_ahead if pending[-1].fused else 0
            while len(pending) > depth:
                finish(pending.popleft())
        while pending:
            finish(pending.popleft())
    except BaseException:
        failed = True
        raise
    finally:
        pending.clear()
        if own:
            try:
                w.close()
            except BaseException:
                if not failed:  # (the loop's own error comes first)
                    raise
    count = int(sums["eval/count"].item()) if sums else 0
    totals = {k_: float(v) for k_, v in sums.items() if k_ != "eval/count"}
    if world > 1 and sums:  # ONE packed reduce for the run: [count, sums...] in float64
        names = sorted(totals)
        packed = torch.tensor([float(count)] + [totals[k_] for k_ in names], dtype=torch.float64, device=out_device[0])
        reduced = pdist.reduce_metrics(packed.clone(), dst=0)
        if rank == 0:
            count = int(reduced[0].round().item())
            totals = {k_: float(reduced[1 + j].to(torch.float32)) for j, k_ in enumerate(names)}
    result = {"eval/count": count}
    for k_, v in totals.items():  # (loss_sum[k] / loss_sum["eval/count"] in float32, :347)
        result[k_] = float(torch.tensor(v, dtype=torch.float32) / torch.tensor([count], dtype=torch.int64))
    result["sums"] = dict({"eval/count": count}, **totals)
    result["records"] = records
    return result
