"""Expected values for the visualiser-export tests (test_vis_host.py, test_gpu_vis.py), written out independently of
pgdvs_amd.png and csrc/png.hip: the two quantisations as the torch expressions of the reference's writers, the PNG filters
and libpng's row heuristic as a plain per-row restatement, the value table, and stub model / dataset for the loop tests."""
import numpy as np
import torch

SIZES = [(1, 1), (1, 7), (7, 1), (31, 45), (288, 550)]


def expected_save_image(x: torch.Tensor) -> torch.Tensor:
    """visualizer_pgdvs.py:103-121 + torchvision.utils.save_image, NaN -> 0"""
    x = x.float().cpu().clamp(0.0, 1.0)
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def expected_truncate(x: torch.Tensor) -> torch.Tensor:
    """visualizer_pgdvs.py:127-136: (clamp(x, 0, 1).numpy() * 255).astype(np.uint8), NaN -> 0"""
    x = x.float().cpu().clamp(0.0, 1.0)
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return torch.from_numpy((x.numpy() * 255).astype(np.uint8))


EXPECTED = {"save_image": expected_save_image, "truncate": expected_truncate}


def value_table() -> torch.Tensor:
    """k/255 and (k + 0.5)/255 with their float32 neighbours on both sides for every k, values outside [0, 1], NaN, +-inf"""
    k = np.arange(256, dtype=np.float64)
    base = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(np.float32)
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    vals = [base, np.nextafter(base, lo), np.nextafter(base, hi), np.nextafter(np.nextafter(base, lo), lo),
            np.nextafter(np.nextafter(base, hi), hi),
            np.array([-1.0, -0.25, -1e-8, -0.0, 1.0 + 1e-6, 1.5, 2.0, 255.0, 1e30, -1e30, np.nan, np.inf, -np.inf], dtype=np.float32)]
    return torch.from_numpy(np.concatenate(vals).astype(np.float32))


def table_image(H: int, W: int) -> torch.Tensor:
    """the value table tiled into a [1,3,H,W] image (every entry appears when 3 H W >= its length)"""
    t = value_table()
    n = 3 * H * W
    return t.repeat((n + t.numel() - 1) // t.numel())[:n].reshape(1, 3, H, W).clone()


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def row_candidates(row: np.ndarray, above: np.ndarray):
    """one scanline's five filtered versions (PNG specification 9.2, bytes per pixel 3) as lists of ints.  row / above: the
    3 W raw bytes of the row and of the row above it (zeros above row 0)."""
    x, b = [int(v) for v in row], [int(v) for v in above]
    n = len(x)
    a = [0, 0, 0] + x[:n - 3] if n > 3 else [0] * n
    c = [0, 0, 0] + b[:n - 3] if n > 3 else [0] * n
    a, c = a[:n], c[:n]
    return [
        [x[i] for i in range(n)],
        [(x[i] - a[i]) % 256 for i in range(n)],
        [(x[i] - b[i]) % 256 for i in range(n)],
        [(x[i] - (a[i] + b[i]) // 2) % 256 for i in range(n)],
        [(x[i] - _paeth(a[i], b[i], c[i])) % 256 for i in range(n)],
    ]


def row_cost(filtered) -> int:
    """libpng's default heuristic: the sum of v < 128 ? v : 256 - v"""
    return sum(v if v < 128 else 256 - v for v in filtered)


def expected_scanlines(q: np.ndarray, adaptive: bool = True) -> np.ndarray:
    """q[H,W,3] uint8 -> [H,1+3W] uint8 by the per-row restatement"""
    H, W, _ = q.shape
    rows = q.reshape(H, 3 * W)
    out = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    for y in range(H):
        cands = row_candidates(rows[y], rows[y - 1] if y > 0 else np.zeros(3 * W, dtype=np.uint8))
        t = 0
        if adaptive:
            costs = [row_cost(f) for f in cands]
            t = costs.index(min(costs))  # (the first = lowest type among equal minima)
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out


def noise_bytes(H: int, W: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


class StubModel:
    """the plugin contract's surface that vis_step uses; renders the batch's own ``img`` (and ``gnt`` when present)"""
    training = True

    def eval(self):
        self.training = False
        return self

    def forward(self, data, render_cfg=None, disable_tqdm=True, for_debug=False):
        assert not self.training and not for_debug and not torch.is_grad_enabled()
        ret = {"combined_rgb": data["img"]}
        if "gnt" in data:
            ret["static_coarse_rgb"] = data["gnt"]
        return ret


class StubDataset:
    def __init__(self, n, H, W, *, split=None, gnt=False, scenes=("scene_a",), seed=0):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for i in range(n):
            misc = {"scene_id": scenes[i % len(scenes)], "tgt_idx": 3 * i + 1}
            if split is not None:
                misc["split"] = split
            item = {"img": torch.rand((3, H, W), generator=g) * 1.2 - 0.1, "misc": misc, "time": 0.5, "name": f"v{i}"}
            if gnt:
                item["gnt"] = torch.rand((3, H, W), generator=g) * 1.2 - 0.1
            self.items.append(item)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]
