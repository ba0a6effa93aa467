#!/usr/bin/env python3
"""Golden vectors for the evaluator's masked LPIPS by RUNNING THE REFERENCE's own
``PerceptualLoss(model="net-lin", net="alex", use_gpu=False, version=0.1)``, constructed exactly as
pgdvs/engines/trainer_pgdvs.py:132-137 does and called as ``obtain_quantitative_nvidia`` calls it
(evaluator_pgdvs.py:190-283: ``forward(gt, pred, mask)`` on images mapped to [-1, 1] by ``modify_rgb_range``, the
masks ones / eval_mask / 1 - eval_mask in [1,3,H,W]).  torchvision is not installed here: a stub
``torchvision.models.alexnet`` returns torchvision's ``features`` layout with the seeded weights of lpips_inputs.py.  The lin
weights are the reference's own ``weights/v0.1/alex.pth`` (loaded by the reference's DistModel) and are stored in the
fixture.  Stores the quantised inputs, the three values per case and relu1..relu5 of one case in lpips.npz.
Usage: python tests/golden/make_golden_lpips.py"""
import pathlib
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import lpips_inputs as LI  # noqa: E402
import make_golden as MG  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent


def _alexnet_stub(pretrained=True):
    nn = torch.nn
    features = nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
    sd = {k[len("features."):]: torch.from_numpy(v) for k, v in LI.backbone_weights().items()}
    features.load_state_dict(sd, strict=True)
    return types.SimpleNamespace(features=features)


def main():
    MG._install_stubs()
    for m in ["skimage.transform", "skimage.color", "scipy", "scipy.ndimage", "IPython"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["torchvision"].models = types.SimpleNamespace(alexnet=_alexnet_stub)
    sys.modules["torchvision.models"] = sys.modules["torchvision"].models
    torch.backends.cudnn.allow_tf32 = False  # (run.py:21-24; CPU here anyway)
    import pgdvs.utils.nsff_lpips as lpips
    from pgdvs.utils.rendering import modify_rgb_range

    lpips_fn = lpips.PerceptualLoss(model="net-lin", net="alex", use_gpu=False, version=0.1)
    net = lpips_fn.model.net
    assert net.version == 0.1 and net.version != "0.1"  # the ScalingLayer is skipped (networks_basic.py:94-99)
    out = {"weights_checksum": LI.checksum(LI.backbone_weights())}
    for k in range(5):
        out[f"lin{k}"] = getattr(net, f"lin{k}").model[1].weight.detach().numpy().copy()
    with torch.no_grad():
        for name in LI.CASES:
            gt, pred, mask = LI.case_images(name)
            T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)[None]  # noqa: E731
            g, p, m = T(gt), T(pred), T(mask)
            g_l = modify_rgb_range(g, src_range="0_1", tgt_range="-1_1", check_range=False)
            p_l = modify_rgb_range(p, src_range="0_1", tgt_range="-1_1", check_range=False)
            vals = [lpips_fn.forward(g_l, p_l, torch.ones_like(g)).item(), lpips_fn.forward(g_l, p_l, m).item(),
                    lpips_fn.forward(g_l, p_l, 1.0 - m).item()]
            out[f"{name}_gt"] = (gt * 255).round().astype(np.uint8)
            out[f"{name}_pred"] = (pred * 255).round().astype(np.uint8)
            out[f"{name}_mask"] = mask[..., 0].copy()
            out[f"{name}_lpips"] = np.array(vals, np.float64)
            if name == LI.FEATURE_CASE:
                feats = net.net.forward(torch.cat([g_l, p_l]))
                for k, f in enumerate(feats):
                    out[f"{name}_relu{k + 1}"] = f.numpy().astype(np.float32)
            print(name, vals)
    np.savez_compressed(OUT / "lpips.npz", **out)


if __name__ == "__main__":
    main()
