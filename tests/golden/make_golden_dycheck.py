#!/usr/bin/env python3
"""Golden vectors for the evaluator's DyCheck iPhone protocol (quant_type "dycheck_iphone") by RUNNING THE
REFERENCE's own ``pgdvs/utils/dycheck/metrics.py`` (compute_psnr, compute_ssim, compute_lpips), called as
``obtain_quantitative_dycheck_iphone`` (evaluator_pgdvs.py:282-409) calls it: ground truth first, a full mask ones[H,W,1] and the
covisibility mask eval_mask[H,W,1].

jax and lpips are not installed here, so the module runs under a shim: ``jax.numpy`` is numpy, ``jax.scipy.signal.convolve2d``
is ``scipy.signal.convolve2d``, ``jax.vmap`` loops over the channel axis, ``jax.devices`` / ``jax.default_device`` do nothing,
``torch.cuda.is_available`` returns True (so that upstream's ``tmp_deivce`` typo on its CPU branch is not reached), and the
``lpips`` module provides the reference's ``nsff_lpips.im2tensor``.  The LPIPS network is the reference's
``nsff_lpips.PNetLin(pnet_type="alex", spatial=True, version="0.1")`` -- lpips 0.1.4's LPIPS(net="alex", spatial=True) -- with
the reference's v0.1 lin weights and the seeded backbone of lpips_inputs.py.  Its ``upsample`` passes ``scale_factor=out/in``
where lpips 0.1.4 passes ``size``; both forms are stored (``*_lpips`` = size, ``*_lpips_sf`` = scale_factor).
Usage: python tests/golden/make_golden_dycheck.py"""
import contextlib
import pathlib
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import scipy.signal
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import lpips_inputs as LI  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_lpips as MGL  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent

# name -> (H, W, mask kind, seed, brightness); "ident" compares an image with itself
CASES = {"a": (64, 96, "binary", 21, 1.0), "b": (45, 70, "binary", 22, 1.0), "c31": (31, 31, "binary", 23, 1.0),
         "ident": (48, 64, "binary", 24, 1.0), "empty": (40, 52, "empty", 25, 1.0), "dark": (37, 50, "empty", 26, 0.08),
         "wide": (33, 120, "binary", 27, 1.0)}


def case_images(name):
    """quantised ground truth / prediction [H,W,3] in [0,1] (8-bit codes / 255, float32) and the covisibility mask [H,W,1]"""
    H, W, kind, seed, bright = CASES[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.35 * (np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0))[..., None] * np.array([1.0, 0.8, 0.6])
    gt = np.clip(bright * (base + 0.08 * rng.standard_normal((H, W, 3))), 0, 1)
    pred = gt if name == "ident" else np.clip(gt + bright * 0.1 * rng.standard_normal((H, W, 3)), 0, 1)
    q = lambda x: (np.asarray(x, np.float32) * np.float32(255)).astype(np.uint8).astype(np.float32) / np.float32(255)  # noqa: E731
    if kind == "binary":  # a covisible blob plus scattered pixels, as a DyCheck covisibility mask looks
        blob = ((yy - H / 2) ** 2 / (0.3 * H) ** 2 + (xx - W / 3) ** 2 / (0.3 * W) ** 2) < 1.0
        mask = (blob | (rng.random((H, W)) < 0.2)).astype(np.float32)[..., None]
    else:
        mask = np.zeros((H, W, 1), np.float32)
    return q(gt), q(pred), mask


def _install_jax_shim(nsff_lpips):
    jax = types.ModuleType("jax")
    jsp = types.ModuleType("jax.scipy")
    jsp.signal = types.SimpleNamespace(convolve2d=lambda z, f, mode="full", precision=None: scipy.signal.convolve2d(z, f, mode=mode))

    def vmap(fn, in_axes, out_axes):
        assert in_axes == (2, None) and out_axes == (2, None)

        def g(z, m):
            outs = [fn(z[..., c], m) for c in range(z.shape[2])]
            return np.stack([o[0] for o in outs], axis=2), outs[0][1]

        return g

    jax.numpy, jax.scipy, jax.vmap = np, jsp, vmap
    jax.lax = types.SimpleNamespace(Precision=types.SimpleNamespace(HIGHEST=None))
    jax.devices = lambda *a: [None, None]
    jax.default_device = lambda d: contextlib.nullcontext()
    sys.modules.update({"jax": jax, "jax.numpy": np, "jax.scipy": jsp})
    sys.modules["lpips"] = types.SimpleNamespace(im2tensor=nsff_lpips.im2tensor)
    torch.cuda.is_available = lambda: True


def main():
    MGL_main_stubs()
    import pgdvs.utils.nsff_lpips as nsff_lpips
    import pgdvs.utils.nsff_lpips.networks_basic as NB

    net = NB.PNetLin(pnet_type="alex", spatial=True, version="0.1").eval()
    lin_path = pathlib.Path(nsff_lpips.__file__).resolve().parent / "weights" / "v0.1" / "alex.pth"
    missing = net.load_state_dict(torch.load(str(lin_path), map_location="cpu"), strict=False)
    assert not [k for k in missing.missing_keys if k.startswith("lin")], missing
    assert net.version == "0.1"  # the ScalingLayer applies on this protocol
    _install_jax_shim(nsff_lpips)
    sys.modules.pop("pgdvs.utils.dycheck.metrics", None)
    import pgdvs.utils.dycheck.metrics as DM

    size_upsample = lambda t, out_HW=(64, 64): torch.nn.functional.interpolate(  # noqa: E731  (lpips 0.1.4)
        t, size=tuple(out_HW), mode="bilinear", align_corners=False)
    sf_upsample = NB.upsample
    out = {"weights_checksum": LI.checksum(LI.backbone_weights())}
    for k in range(5):
        out[f"lin{k}"] = getattr(net, f"lin{k}").model[1].weight.detach().numpy().copy()
    for name in CASES:
        gt, pred, mask = case_images(name)
        full = np.ones_like(gt)[..., :1]
        vals = [float(DM.compute_psnr(gt, pred, full).item()), float(DM.compute_ssim(gt, pred, full).item()),
                float(DM.compute_psnr(gt, pred, mask).item()), float(DM.compute_ssim(gt, pred, mask).item())]
        lp = {}
        for tag, up in (("", size_upsample), ("_sf", sf_upsample)):
            NB.upsample = up
            lp[tag] = [float(DM.compute_lpips(net, gt, pred, full).item()), float(DM.compute_lpips(net, gt, pred, mask).item())]
        NB.upsample = sf_upsample
        out[f"{name}_gt"] = (gt * 255).round().astype(np.uint8)
        out[f"{name}_pred"] = (pred * 255).round().astype(np.uint8)
        out[f"{name}_mask"] = mask[..., 0].astype(np.uint8)
        out[f"{name}_psnr_ssim"] = np.array(vals, np.float64)  # psnr, ssim, mpsnr, mssim
        out[f"{name}_lpips"] = np.array(lp[""], np.float64)  # lpips, mlpips (lpips 0.1.4: upsample by size)
        out[f"{name}_lpips_sf"] = np.array(lp["_sf"], np.float64)  # (the reference's copy: upsample by scale_factor)
        print(name, vals, lp)
    np.savez_compressed(OUT / "dycheck.npz", **out)


def MGL_main_stubs():
    """the stubs of make_golden_lpips.main: the reference's imports, and torchvision's AlexNet with the seeded weights"""
    MG._install_stubs()
    for m in ["skimage.transform", "skimage.color", "IPython"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["torchvision"].models = types.SimpleNamespace(alexnet=MGL._alexnet_stub)
    sys.modules["torchvision.models"] = sys.modules["torchvision"].models
    torch.backends.cudnn.allow_tf32 = False


if __name__ == "__main__":
    main()
