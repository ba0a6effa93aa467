"""Seeded AlexNet backbone weights and the cases of the LPIPS fixture (lpips.npz): pure numpy, imported by the generator
(make_golden_lpips.py, which runs the REFERENCE's PerceptualLoss with these weights in place of torchvision's pretrained
ones) and by the tests (tests/test_lpips_host.py, tests/test_gpu_lpips.py).  The 10 MB backbone is regenerated here rather
than committed; the fixture carries its checksum so that a generator that drifts fails loudly.  The lin weights are the
reference's real ``weights/v0.1/alex.pth`` (data, 6 KB) and ride in the fixture."""
import numpy as np

WEIGHT_SEED = 4711
# torchvision alexnet().features: index -> (Cout, Cin, k)
ALEX_CONVS = {0: (64, 3, 11), 3: (192, 64, 5), 6: (384, 192, 3), 8: (256, 384, 3), 10: (256, 256, 3)}
# name -> (H, W, mask kind, seed); "ident" compares an image with itself.  The features of FEATURE_CASE are stored too.
CASES = {"a": (64, 96, "binary", 11), "b": (135, 240, "soft", 12), "c": (67, 101, "empty", 13), "ident": (48, 64, "binary", 14)}
FEATURE_CASE = "a"


def backbone_weights():
    """features.{i}.{weight,bias} in torchvision's layout: He-scaled normal weights (ReLU maps neither vanish nor explode
    through five layers) and small non-zero biases."""
    rng = np.random.default_rng(WEIGHT_SEED)
    out = {}
    for i, (co, ci, k) in ALEX_CONVS.items():
        out[f"features.{i}.weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        out[f"features.{i}.bias"] = (0.05 * rng.standard_normal(co)).astype(np.float32)
    return out


def checksum(weights):
    return np.array([float(np.sum(weights[k].astype(np.float64) * (1 + j % 7))) for j, k in enumerate(sorted(weights))])


def case_images(name):
    """quantised ground truth / prediction [H,W,3] in [0,1] (8-bit codes / 255, float32, as the evaluator leaves them) and the
    dynamic mask [H,W,3]"""
    H, W, kind, seed = CASES[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.35 * (np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0))[..., None] * np.array([1.0, 0.8, 0.6])
    gt = np.clip(base + 0.08 * rng.standard_normal((H, W, 3)), 0, 1)
    pred = gt if name == "ident" else np.clip(gt + 0.1 * rng.standard_normal((H, W, 3)), 0, 1)
    q = lambda x: (np.asarray(x, np.float32) * np.float32(255)).astype(np.uint8).astype(np.float32) / np.float32(255)  # noqa: E731
    if kind == "binary":
        mask = (rng.random((H, W, 1)) < 0.35).astype(np.float32).repeat(3, axis=-1)
    elif kind == "soft":
        mask = rng.random((H, W, 3)).astype(np.float32)
    else:
        mask = np.zeros((H, W, 3), np.float32)
    return q(gt), q(pred), mask
