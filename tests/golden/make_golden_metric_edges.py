#!/usr/bin/env python3
"""Golden vectors for the structured metric cases of tests/metric_cases.py (FIXTURE_CASES: flat, black against white,
checkerboard, ramp, single differing pixel, halo-only difference; 31 to 74 pixels a side; stripe, band, half-plane, soft and
empty masks) by RUNNING THE REFERENCE's own code: ``pgdvs/utils/dycheck/metrics.py`` (compute_psnr, compute_ssim, compute_lpips)
under the jax shim of make_golden_dycheck.py, and ``PerceptualLoss(model="net-lin", net="alex", version=0.1)`` as
make_golden_lpips.py sets it up.  Stores the 8-bit codes, the 8-bit masks (soft masks as float32) and the reference's scalars in
metric_edges.npz; the lin weights are those of dycheck.npz / lpips.npz and are not stored again.
Usage: python tests/golden/make_golden_metric_edges.py"""
import pathlib
import sys

import numpy as np
import torch

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "ml-pgdvs_amd"))
import lpips_inputs as LI  # noqa: E402
import make_golden_dycheck as MGD  # noqa: E402
import metric_cases as MC  # noqa: E402


def main():
    MGD.MGL_main_stubs()
    import pgdvs.utils.nsff_lpips as nsff_lpips
    import pgdvs.utils.nsff_lpips.networks_basic as NB
    from pgdvs.utils.rendering import modify_rgb_range

    nv = nsff_lpips.PerceptualLoss(model="net-lin", net="alex", use_gpu=False, version=0.1)
    assert nv.model.net.version == 0.1 and nv.model.net.version != "0.1"  # no ScalingLayer on the NVIDIA protocol
    dy = NB.PNetLin(pnet_type="alex", spatial=True, version="0.1").eval()
    lin_path = pathlib.Path(nsff_lpips.__file__).resolve().parent / "weights" / "v0.1" / "alex.pth"
    missing = dy.load_state_dict(torch.load(str(lin_path), map_location="cpu"), strict=False)
    assert not [k for k in missing.missing_keys if k.startswith("lin")], missing
    MGD._install_jax_shim(nsff_lpips)
    sys.modules.pop("pgdvs.utils.dycheck.metrics", None)
    import pgdvs.utils.dycheck.metrics as DM

    NB.upsample = lambda t, out_HW=(64, 64): torch.nn.functional.interpolate(  # noqa: E731  (lpips 0.1.4: by size)
        t, size=tuple(out_HW), mode="bilinear", align_corners=False)
    out = {"weights_checksum": LI.checksum(LI.backbone_weights())}
    with torch.no_grad():
        for name in MC.FIXTURE_CASES:
            gt_c, pred_c, m = MC.fixture_inputs(name)
            gt, pred, mask = MC.values(gt_c), MC.values(pred_c), m[..., None]
            full = np.ones_like(mask)
            ps = [float(DM.compute_psnr(gt, pred, full).item()), float(DM.compute_ssim(gt, pred, full).item()),
                  float(DM.compute_psnr(gt, pred, mask).item()), float(DM.compute_ssim(gt, pred, mask).item())]
            dl = [float(DM.compute_lpips(dy, gt, pred, full).item()), float(DM.compute_lpips(dy, gt, pred, mask).item())]
            T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)[None]  # noqa: E731
            g_l, p_l = (modify_rgb_range(T(x), src_range="0_1", tgt_range="-1_1", check_range=False) for x in (gt, pred))
            m3 = T(np.repeat(mask, 3, axis=-1))
            nl = [nv.forward(g_l, p_l, torch.ones_like(m3)).item(), nv.forward(g_l, p_l, m3).item(), nv.forward(g_l, p_l, 1.0 - m3).item()]
            binary = bool(np.isin(m, (0.0, 1.0)).all())
            out[f"{name}_gt"], out[f"{name}_pred"] = gt_c, pred_c
            out[f"{name}_mask"] = m.astype(np.uint8) if binary else m
            out[f"{name}_psnr_ssim"] = np.array(ps, np.float64)  # psnr, ssim, mpsnr, mssim
            out[f"{name}_dlpips"] = np.array(dl, np.float64)  # lpips, mlpips (DyCheck protocol)
            out[f"{name}_lpips"] = np.array(nl, np.float64)  # full, dyn, static (NVIDIA protocol)
            print(name, ps, dl, nl)
    np.savez_compressed(HERE / "metric_edges.npz", **out)


if __name__ == "__main__":
    main()
