#!/usr/bin/env python3
"""Golden vectors of the two preprocessing stages that are the reference's own arithmetic: its
pgdvs/preprocess/common.py compute_occlusion(return_raw=True) on seeded flow pairs (preprocess_flow.npz) and its
pgdvs/preprocess/compute_mask.py compute_epipolar_distance / read_optical_flow / compute_mask_epipolar_flow on a five-frame
synthetic scene (preprocess_epi.npz), inputs and outputs together.

What stands in for modules that are not installed here: cv2, detectron2.*, oneformer, third_parties.* and imageio_ffmpeg
are plain MagicMock stand-ins (nothing called here touches them).  ``skimage.morphology`` is a scipy-backed stand-in written
below: ``disk``, ``binary_erosion`` with border_value=True, ``binary_dilation`` with border_value=0 and ``binary_opening``
as the dilation of the erosion.  It RESTATES skimage (whose functions are these scipy.ndimage calls) and is not skimage
itself: the fixture's masks pin the opening to that restatement.

preprocess_flow.npz, per size 2x2, 5x7, 37x53, 70x130 and case:
  zero  both flows zero.
  int   even-integer flows: bilinear weights 0 and 1 up to the round trip through the normalised grid, sum|coord_diff| even.
  mix   a coherent pair (a smooth forward flow; the backward flow its negation resampled, plus noise on part of the
        image) with edge targets written over scattered pixels of both flows: exactly on the last column / row / corner,
        in (-1, 0) and (W-1, W) on all four sides, wholly outside on each side, and one flow of 1e4.
preprocess_epi.npz: cameras, the five .npz pairs the chosen directions read, the reference's F, masked distance and motion
mask per frame.  Frames 0 / 4 have one neighbour; frame 1's previous camera is nearer, frame 2's next one, frame 3's two
neighbours are exactly as far (pure translations by dyadic numbers): a tie, which goes forward.

Guard bands, asserted here so that the consumers may demand masks bit for bit: no pixel with | sum|coord_diff| - 1 | < 1e-3,
no pixel with a masked epipolar distance within 1e-6 of the threshold; pixels that land there get their own flow nudged
by 1/64 pixel and everything is recomputed.  On the 37x53 and 70x130 mix cases between 20 % and 80 % of the pixels pass
sum|coord_diff| <= 1 (purely random pairs fail it nearly everywhere)."""
import pathlib
import sys
import tempfile
from types import ModuleType
from unittest.mock import MagicMock

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as MG  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
SIZES = ((2, 2), (5, 7), (37, 53), (70, 130))
EPI_H, EPI_W, EPI_FRAMES = 23, 71, 5
GUARD_CONSIST, GUARD_DIST, NUDGE = 1e-3, 1e-6, 1.0 / 64


def _install_stubs():
    from scipy import ndimage as ndi

    MG._install_stubs()
    for m in ["cv2", "detectron2", "detectron2.config", "detectron2.data", "detectron2.data.detection_utils",
              "detectron2.projects", "detectron2.projects.deeplab", "detectron2.utils", "detectron2.utils.logger", "oneformer",
              "third_parties", "third_parties.OneFormer", "third_parties.OneFormer.demo", "third_parties.OneFormer.demo.predictor",
              "imageio_ffmpeg"]:
        sys.modules[m] = MagicMock()
    for m in ["tqdm", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.axes_grid1"]:  # unused by the three functions
        try:
            __import__(m)
        except ImportError:
            sys.modules[m] = MagicMock()

    def disk(radius):
        assert radius == 1
        return np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)

    def binary_erosion(image, footprint):
        return ndi.binary_erosion(image, structure=footprint, border_value=True)

    def binary_dilation(image, footprint):
        return ndi.binary_dilation(image, structure=footprint, border_value=0)

    def binary_opening(image, footprint):
        return binary_dilation(binary_erosion(image, footprint), footprint)

    morph = ModuleType("skimage.morphology")
    morph.disk, morph.binary_erosion, morph.binary_dilation, morph.binary_opening = disk, binary_erosion, binary_dilation, binary_opening
    sk = ModuleType("skimage")
    sk.morphology = morph
    sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, morph


def _chw(flow):
    return torch.from_numpy(np.ascontiguousarray(flow)).permute(2, 0, 1)[None]


def coord_diffs(PC, f12, f21):
    """the reference's two calls (compute_flow.py:335-346) -> coord_diff_1, coord_diff_2 as [H,W,2] float32"""
    H, W = f12.shape[:2]
    img = torch.zeros(1, 3, H, W)
    out = []
    for a, b in ((f12, f21), (f21, f12)):
        cd, _ = PC.compute_occlusion(img, _chw(a), _chw(b), return_raw=True)
        out.append(cd.permute(0, 2, 3, 1)[0].numpy())
        assert out[-1].dtype == np.float32
    return out


def sample(img, x, y):
    """plain float64 bilinear look-up with clamped coordinates: only shapes the INPUT flows"""
    H, W = img.shape[:2]
    x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    x0, y0 = np.minimum(np.floor(x), W - 2).astype(int), np.minimum(np.floor(y), H - 2).astype(int)
    wx, wy = (x - x0)[..., None], (y - y0)[..., None]
    return ((img[y0, x0] * (1 - wx) + img[y0, x0 + 1] * wx) * (1 - wy) + (img[y0 + 1, x0] * (1 - wx) + img[y0 + 1, x0 + 1] * wx) * wy)


def coherent_pair(H, W, rng, noise_cols=0.45):
    """a smooth forward flow, the backward flow its negation resampled where it lands, noise on the left part"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ph = rng.uniform(0, 2 * np.pi, 4)
    amp = min(3.0, 0.25 * min(H, W))
    f12 = np.stack([amp * np.sin(2 * np.pi * xs / (1.7 * W) + ph[0]) * np.cos(2 * np.pi * ys / (1.3 * H) + ph[1]),
                    amp * np.cos(2 * np.pi * xs / (1.1 * W) + ph[2]) * np.sin(2 * np.pi * ys / (1.9 * H) + ph[3])], -1)
    guess = -sample(f12, xs, ys)
    f21 = -sample(f12, xs + guess[..., 0], ys + guess[..., 1])
    noisy = xs < noise_cols * W
    f21 = f21 + noisy[..., None] * rng.normal(size=(H, W, 2)) * 2.0
    return f12.astype(np.float32), f21.astype(np.float32)


def edge_targets(H, W):
    """(target x, target y) of the edge pixels; None keeps a random in-image coordinate"""
    return [("big", "big"), (W - 1, None), (None, H - 1), (W - 1, H - 1), (-0.4, None), (W - 1 + 0.3, None), (None, -0.7),
            (None, H - 1 + 0.6), (-0.25, -0.5), (W - 1 + 0.75, H - 1 + 0.5), (-0.5, H - 1 + 0.25), (W - 1 + 0.5, -0.75),
            (-3.5, None), (W + 2.25, None), (None, -7.0), (None, H + 1.5), (-2.0, H + 3.0), (0, 0), (0.5, 0), (W - 1.5, H - 1)]


def write_edges(flow, rng, reps):
    H, W = flow.shape[:2]
    targets = edge_targets(H, W)
    n = min(len(targets) * reps, H * W)
    for k, pix in enumerate(rng.permutation(H * W)[:n]):
        y, x = divmod(int(pix), W)
        tx, ty = targets[k % len(targets)]
        if tx == "big":
            flow[y, x] = (1e4, -37.0)
            continue
        tx = rng.integers(0, W) + rng.choice([0.0, 0.25, 0.5]) if tx is None else tx
        ty = rng.integers(0, H) + rng.choice([0.0, 0.25, 0.5]) if ty is None else ty
        flow[y, x] = (np.float32(tx) - np.float32(x), np.float32(ty) - np.float32(y))


def settle(PC, f12, f21):
    """nudge the own flow of every pixel inside the consistency guard band until none is left"""
    for it in range(50):
        cd1, cd2 = coord_diffs(PC, f12, f21)
        bad = [np.abs(np.abs(cd).sum(-1, dtype=np.float64) - 1.0) < 2 * GUARD_CONSIST for cd in (cd1, cd2)]
        if not bad[0].any() and not bad[1].any():
            return cd1, cd2
        f12[bad[0], it % 2] += np.float32(NUDGE)  # x and y in turn: where the other flow has slope -1 along one axis,
        f21[bad[1], it % 2] += np.float32(NUDGE)  # the residual does not depend on that component
    raise AssertionError("the guard band did not clear")


def flow_fixture(PC):
    out = {"sizes": np.array(SIZES)}
    for H, W in SIZES:
        rng = np.random.default_rng(1000 * H + W)
        cases = {"zero": (np.zeros((H, W, 2), np.float32), np.zeros((H, W, 2), np.float32)),
                 "int": tuple((2 * rng.integers(-2, 3, (H, W, 2))).astype(np.float32) for _ in range(2))}
        f12, f21 = coherent_pair(H, W, rng)
        reps = 1 if H * W < 100 else 3
        write_edges(f12, rng, reps)
        write_edges(f21, rng, reps)
        cases["mix"] = (f12, f21)
        for name, (a, b) in cases.items():
            cd1, cd2 = settle(PC, a, b)
            for cd in (cd1, cd2):
                s = np.abs(cd).sum(-1)
                assert not (np.abs(s.astype(np.float64) - 1.0) < GUARD_CONSIST).any(), (H, W, name)
                assert np.isfinite(cd).all()
            if name == "zero":
                assert not cd1.any() and not cd2.any()
            if name == "int":
                assert np.all(a == np.round(a)) and np.all(b == np.round(b))  # no nudge was needed
            if name == "mix" and H * W > 1000:
                for cd in (cd1, cd2):
                    share = (np.abs(cd).sum(-1) <= 1.0).mean()
                    assert 0.2 < share < 0.8, (H, W, share)
                    print(f"    {H}x{W} mix: {100 * share:.1f} % consistent")
            tag = f"{H}x{W}_{name}"
            out[f"{tag}_flow12"], out[f"{tag}_flow21"], out[f"{tag}_cd1"], out[f"{tag}_cd2"] = a, b, cd1, cd2
    np.savez_compressed(OUT / "preprocess_flow.npz", **out)
    print(f"  preprocess_flow.npz {(OUT / 'preprocess_flow.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


class _Recorder:
    """numpy, with every 3 x 3 result of np.dot kept: compute_epipolar_distance's last one is its F_mat"""

    def __init__(self):
        self.dots = []

    def __getattr__(self, name):
        return getattr(np, name)

    def dot(self, a, b):
        r = np.dot(a, b)
        if r.shape == (3, 3):
            self.dots.append(r)
        return r


def epi_scene(rng):
    """cameras (w2c, K) and per directed pair of neighbours a flow: the rigid flow of a smooth depth, an object moving
    across the epipolar lines in a blob, speckles, and a band where the backward flow disagrees"""
    H, W, n = EPI_H, EPI_W, EPI_FRAMES
    K = np.array([[60.0, 0, W / 2.0], [0, 62.0, H / 2.0], [0, 0, 1]])
    centres = np.array([[0.0, 0.0, 0.0], [0.25, 0.03125, 0.0], [0.75, 0.0, 0.0625], [1.0, 0.125, 0.0], [1.25, 0.0, 0.0625]])
    # frame 3: |c2 - c3| = 0.25 + 0.125 + 0.0625 = |c4 - c3| exactly
    w2c = np.stack([np.eye(4)] * n)
    for i in range(n):
        if i < 2:  # a small rotation where no tie depends on it
            a = 0.03 * (i + 1)
            w2c[i, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        w2c[i, :3, 3] = -w2c[i, :3, :3] @ centres[i]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    flows = {}
    for a in range(n):
        for b in (a - 1, a + 1):
            if not 0 <= b < n:
                continue
            depth = 3.0 + np.sin(xs / 9.0 + a) + 0.5 * np.cos(ys / 5.0 + b)
            cam = (pix @ np.linalg.inv(K).T) * depth[..., None]
            T = w2c[b] @ np.linalg.inv(w2c[a])
            q = (cam @ T[:3, :3].T + T[:3, 3]) @ K.T
            flow = q[..., :2] / q[..., 2:] - pix[..., :2]
            blob = ((xs - (20 + 9 * a)) ** 2 / 60.0 + (ys - 11) ** 2 / 30.0) < 1.0
            flow[blob] += (0.5, 3.0 + 0.5 * a)  # across the (mostly horizontal) epipolar lines
            blob2 = (np.abs(xs - 64) < 4) & (np.abs(ys - 16) < 3)  # over the seams of a 64 x 16 tiling
            flow[blob2] += (0.0, -2.5)
            speck = rng.random((H, W)) < 0.03
            flow[speck] += (0.0, 4.0)
            flow[0, :5] += (0.0, 3.0)   # features on the border and in the corners
            flow[:3, 0] += (0.0, 3.0)
            flow[-1, -4:] += (0.0, -3.0)
            flow[-3:, -1] += (0.0, -3.0)
            flows[(a, b)] = flow.astype(np.float32)
    return w2c, np.stack([K] * n), flows


def epi_fixture(PC, CM):
    rng = np.random.default_rng(77)
    H, W, n = EPI_H, EPI_W, EPI_FRAMES
    w2c, Ks, flows = epi_scene(rng)
    names = [f"{i:05d}" for i in range(n)]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    # the opposite flow of every pair: the negation resampled where it lands, noise in a band (inconsistent there)
    back = {}
    for key, f in flows.items():
        f64 = f.astype(np.float64)
        guess = -sample(f64, xs, ys)
        g = -sample(f64, xs + guess[..., 0], ys + guess[..., 1])
        band = (ys >= 5) & (ys < 9)
        back[key] = (g + band[..., None] * rng.normal(size=(H, W, 2)) * 2.0).astype(np.float32)
    rec = _Recorder()
    CM.np = rec
    out = {"w2c": w2c, "K": Ks, "names": np.array(names), "H": np.array(H), "W": np.array(W)}
    with tempfile.TemporaryDirectory() as td:
        td = pathlib.Path(td)
        for _ in range(50):
            cds = {}
            for (a, b), f in flows.items():
                cds[(a, b)] = settle(PC, f, back[(a, b)])[0]  # nudges f in place
                np.savez(td / f"{names[a]}_{names[b]}.npz", flow=f, coord_diff=cds[(a, b)])
            close = False
            per_frame = []
            for i in range(n):
                fwd_ok, bwd_ok = i + 1 < n, i - 1 >= 0
                mask = CM.compute_mask_epipolar_flow(img_ref=np.zeros((H, W, 3)), idx_ref=i, n_all_frames=n, all_w2c=w2c, all_K=Ks,
                                                     flow_dir=td, flow_interval=1, threshold=1.0, all_img_names=names)
                # the direction the reference chose, from its own branches: one neighbour, or the nearer camera
                if not bwd_ok:
                    use_prev = False
                elif not fwd_ok:
                    use_prev = True
                else:
                    c = [np.linalg.inv(w2c[j])[:3, 3] for j in (i - 1, i, i + 1)]
                    use_prev = bool(np.sum(np.abs(c[0] - c[1])) < np.sum(np.abs(c[2] - c[1])))
                j = i - 1 if use_prev else i + 1
                flow, consist = CM.read_optical_flow(td, names, i, flow_interval=1, read_fwd=not use_prev)
                p_ref = np.float32(np.stack((xs, ys), axis=-1))
                ones = np.ones((H * W, 1))
                p1 = np.concatenate((np.reshape(p_ref, (-1, 2)), ones), axis=-1).T
                p2 = np.concatenate((np.reshape(p_ref + flow, (-1, 2)), ones), axis=-1).T
                rec.dots.clear()
                T = np.dot(w2c[j], np.linalg.inv(w2c[i]))
                e = CM.compute_epipolar_distance(T_12=T, K_1=Ks[i], K_2=Ks[j], p_1=p1, p_2=p2)
                F = rec.dots[-1]
                e = np.reshape(e, (H, W)) * consist
                # the mask of the chosen direction alone IS the reference's mask
                assert np.array_equal(CM.skimage.morphology.binary_opening(e > 1.0, CM.skimage.morphology.disk(1)), mask)
                near = np.abs(e - 1.0) < 2 * GUARD_DIST
                if near.any():
                    close = True
                    flows[(i, j)][near, 1] += np.float32(NUDGE)
                per_frame.append((i, j, use_prev, F, e, mask))
            if not close:
                break
        else:
            raise AssertionError("the distance guard band did not clear")
    assert [p[2] for p in per_frame] == [False, True, False, False, True], [p[2] for p in per_frame]
    c = [np.linalg.inv(w2c[j])[:3, 3] for j in (2, 3, 4)]
    assert np.sum(np.abs(c[0] - c[1])) == np.sum(np.abs(c[2] - c[1]))  # frame 3 is the tie
    for i, j, use_prev, F, e, mask in per_frame:
        cd = cds[(i, j)]
        assert not (np.abs(np.abs(cd).sum(-1, dtype=np.float64) - 1.0) < GUARD_CONSIST).any()
        assert not (np.abs(e - 1.0) < GUARD_DIST).any()
        consist = np.abs(cd).sum(-1) <= 1.0
        assert 0.2 < consist.mean() < 0.95 and 0 < mask.mean() < 0.5 and ((e > 1.0) != mask).any(), (i, consist.mean(), mask.mean())
        print(f"    frame {i} -> {j}: {100 * consist.mean():.0f} % consistent, raw {int((e > 1.0).sum())} px, mask {int(mask.sum())} px")
        out[f"f{i}_other"], out[f"f{i}_use_prev"], out[f"f{i}_F"] = np.array(j), np.array(use_prev), F
        out[f"f{i}_flow"], out[f"f{i}_coord_diff"], out[f"f{i}_e_dist"], out[f"f{i}_mask"] = flows[(i, j)], cd, e, mask
    np.savez_compressed(OUT / "preprocess_epi.npz", **out)
    print(f"  preprocess_epi.npz {(OUT / 'preprocess_epi.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


def main():
    _install_stubs()
    import pgdvs.preprocess.common as PC
    import pgdvs.preprocess.compute_mask as CM

    torch.manual_seed(0)
    torch.set_num_threads(1)
    flow_fixture(PC)
    epi_fixture(PC, CM)


if __name__ == "__main__":
    main()
