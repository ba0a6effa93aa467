#!/usr/bin/env python3
"""Golden vectors of what the reference's flow stage computes from flows besides running its networks
(preprocess_flow_export.npz), produced by RUNNING THE REFERENCE: its pgdvs/preprocess/compute_flow.py compute_grid_indices,
compute_weight and the tile branch of compute_flow_flowformer around a stub tile model that returns recorded flows, and its
pgdvs/preprocess/common.py flow_to_image.  compute_flow.py imports cv2 and (in its __main__ part) the two flow networks;
it is imported under the stand-ins of make_golden_preprocess._install_stubs(), none of which the functions here touch.

Blend (``blend_cases``): FLOWFORMER_TRAIN_SIZE is set to [48, 64] (in place: the functions bound the list as a default
argument) and the overlap left at 20.  48x64 one tile, the result is (f w) / w; 53x70 two tiles per axis that overlap almost
entirely; 76x108 with the origin lists [0, 28, 28] and [0, 44, 44], nine tiles of which pairs and one foursome coincide;
106x154 sixteen tiles, origins [0, 28, 56, 58] and [0, 44, 88, 90].  57x109 and 100x150 are stored as ORIGINS ONLY
(``origins_57x109``, ``origins_100x150``): upstream's lists there are [0, 28, 9] x [0, 44, 45], not monotonic, and
[0, 28, 56, 52] x [0, 44, 88, 86], and its own compute_weight raises on both, because the tile at 28 ends at row 76 of 57 and
the tile at 88 at column 152 of 150 -- a list of upstream's that is not monotonic always holds such an origin (the last
entry H - ph lies before its predecessor k (ph - 20) exactly when that predecessor's tile ends past H), so 76x108, where
the two are equal, and 106x154 are the nearest sizes that upstream can blend.  Each at
sigma 0.05 (denormal weights at the rim of a tile) and sigma 1.0.  Tile flows are quarter-pixel integers (int16, exact in
float32), stored in two parts: a base vector per tile and one per-pixel pattern that a case's tiles share (``tiles_of``
puts them together), which keeps the file small; tile 0 holds -0.0 at (component 0, row 0, column 0), a pixel that no other
tile covers (int16 has no -0: ``negzero`` lists the flat indices to overwrite).
Stored: origins, the two weight tables, the blended flows as float32 bits.

Picture (``picture_cases``): the 37x53 mixed flow12 of preprocess_flow.npz (read there, not stored again); an all-zero flow;
the eight axis and diagonal directions with both signs of zero on the axes (u > 0 with v = -0.0 gives a = +1, fk = 54 and
k1 wraps to 0; u > 0 with v = +0.0 gives a = -1, fk = 0); a frame with one vector 1000 times the rest; rows of 2048 and 2049
pixels, 3 rows high, drawn from a palette of 61 vectors so that they deflate well.  Stored per case: the flow, rad_max as
float32 bits, the normalised u and v the reference hands to flow_uv_to_colors (captured there) and the picture.  Two 3x5
frames with a NaN and an inf pixel are stored as inputs only: the reference casts NaN to an index there and raises.

The file must stay under 512 KiB."""
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden_preprocess as MGP  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
PATCH = (48, 64)
SIGMAS = (0.05, 1.0)
BLEND_SIZES = ((48, 64), (53, 70), (76, 108), (106, 154))
ORIGINS_ONLY = ((57, 109), (100, 150))  # upstream lists origins there that its own blend cannot take
LIMIT = 512 * 1024


def sigma_tag(sigma):
    return f"s{sigma:g}".replace(".", "p")


def tile_flows(n, rng):
    """(base[n,2], pattern[2,ph,pw]) quarter-pixel int16: tile t is base[t] + pattern, a vector per tile within +-40 pixels
    plus one per-pixel pattern within +-2 that the tiles of a case share; stored as the two parts, which is what keeps the
    file small"""
    base = rng.integers(-160, 161, (n, 2)).astype(np.int16)
    pattern = rng.integers(-8, 9, (2,) + PATCH).astype(np.int16)
    pattern[0, 0, 0] = -base[0, 0]  # tile 0 is zero there: the -0.0 of the case
    return base, pattern


def tiles_of(base, pattern, negzero):
    """the float32 tiles [n,2,ph,pw] of a case from its stored parts (the tests build them the same way)"""
    tiles = (base[:, :, None, None].astype(np.int32) + pattern[None]).astype(np.float32) / np.float32(4.0)
    tiles.reshape(-1)[negzero] = -0.0
    return tiles


def blend_fixture(CF, out):
    CF.FLOWFORMER_TRAIN_SIZE[:] = list(PATCH)
    for sigma in SIGMAS:
        w = CF.compute_weight("cpu", [(0, 0)], PATCH, CF.FLOWFORMER_TRAIN_SIZE, sigma)[0][0, 0].numpy()
        assert w.dtype == np.float32 and w.shape == PATCH and (w > 0).all()
        if sigma == 0.05:
            tiny = np.finfo(np.float32).tiny
            assert ((w < tiny) & (w > 0)).any(), "no denormal weight at sigma 0.05"
        out[f"weight_{sigma_tag(sigma)}"] = w
    out["blend_cases"] = np.array([f"{H}x{W}" for H, W in BLEND_SIZES])
    out["patch"], out["sigmas"] = np.array(PATCH), np.array(SIGMAS)
    for H, W in BLEND_SIZES:
        tag = f"blend_{H}x{W}"
        hws = CF.compute_grid_indices((H, W))
        rng = np.random.default_rng(7000 * H + W)
        base, pattern = tile_flows(len(hws), rng)
        negzero = np.array([0], np.int64)  # flat indices into tiles[n,2,ph,pw]
        tiles = tiles_of(base, pattern, negzero)
        assert tiles[0, 0, 0, 0] == 0 and np.signbit(tiles[0, 0, 0, 0]) and sum(1 for h, w in hws if h == 0 and w == 0) == 1
        out[f"{tag}_origins"], out[f"{tag}_base_q"], out[f"{tag}_pattern_q"] = np.array(hws, np.int32), base, pattern
        out[f"{tag}_negzero"] = negzero
        image = torch.zeros(1, 3, H, W)
        for sigma in SIGMAS:
            calls = iter(range(len(hws)))

            def model(t1, t2, calls=calls, tiles=tiles):
                assert tuple(t1.shape) == (1, 3) + PATCH == tuple(t2.shape)
                return torch.from_numpy(tiles[next(calls)][None]), None

            flow = CF.compute_flow_flowformer(model, image, image, sigma, flowformer_use_tile=True)
            assert next(calls, None) is None and tuple(flow.shape) == (1, 2, H, W) and flow.dtype == torch.float32
            flow = np.ascontiguousarray(flow[0].permute(1, 2, 0).numpy())
            assert np.isfinite(flow).all()
            out[f"{tag}_{sigma_tag(sigma)}_flow_bits"] = flow.view(np.uint32)
        print(f"    {tag}: {len(hws)} tiles")
    for H, W in ORIGINS_ONLY:
        odd = CF.compute_grid_indices((H, W))
        out[f"origins_{H}x{W}"] = np.array(odd, np.int32)
        try:
            CF.compute_weight("cpu", odd, (H, W), CF.FLOWFORMER_TRAIN_SIZE, 1.0)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"upstream blends {H}x{W} after all: make it a blend case")
    odd = CF.compute_grid_indices((57, 109))
    assert [h for h, w in odd if w == 0] == [0, 28, 9] and [w for h, w in odd if h == 0] == [0, 44, 45]
    assert [h for h, w in CF.compute_grid_indices((76, 108)) if w == 0] == [0, 28, 28]
    assert [w for h, w in CF.compute_grid_indices((76, 108)) if h == 0] == [0, 44, 44]


def picture_inputs():
    rng = np.random.default_rng(20240)
    flows = {"zero": np.zeros((4, 6, 2), np.float32)}
    z, nz = np.float32(0.0), np.float32(-0.0)
    axis = [(1, z), (1, nz), (-1, z), (-1, nz), (z, 1), (nz, 1), (z, -1), (nz, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]
    flows["axis"] = np.array(axis, np.float32).reshape(3, 4, 2) * np.float32(3.0)
    big = (rng.integers(-12, 13, (5, 7, 2)) / 4).astype(np.float32)
    big[2, 3] = big[1, 1] * np.float32(1000.0) + np.float32(250.0)
    flows["big"] = big
    palette = (rng.integers(-200, 201, (61, 2)) / 4).astype(np.float32)
    for W in (2048, 2049):
        flows[f"wide{W}"] = palette[rng.integers(0, 61, (3, W))]
    return flows


def picture_fixture(PC, out):
    flows = picture_inputs()
    mix = np.load(OUT / "preprocess_flow.npz")["37x53_mix_flow12"]
    cases = ["mix"] + list(flows)
    out["picture_cases"] = np.array(cases)
    seen = []
    inner = PC.flow_uv_to_colors

    def recorder(u, v, convert_to_bgr=False):
        seen.append((np.array(u), np.array(v)))
        return inner(u, v, convert_to_bgr)

    PC.flow_uv_to_colors = recorder
    try:
        for name in cases:
            flow = mix if name == "mix" else flows[name]
            del seen[:]
            img = PC.flow_to_image(flow)
            (u, v), = seen
            rad_max = np.max(np.sqrt(np.square(flow[..., 0]) + np.square(flow[..., 1])))
            assert img.dtype == np.uint8 and img.shape == flow.shape[:2] + (3,)
            assert u.dtype == np.float32 and rad_max.dtype == np.float32, "upstream's rad_max + epsilon left float32 (NumPy 2 expected)"
            assert np.array_equal(u.view(np.uint32), (flow[..., 0] / (rad_max + np.float32(1e-5))).view(np.uint32))
            if name != "mix":
                out[f"pic_{name}_flow"] = flow
            out[f"pic_{name}_rad_max_bits"] = np.array(rad_max).view(np.uint32)
            out[f"pic_{name}_u"], out[f"pic_{name}_v"], out[f"pic_{name}_img"] = u, v, img
            print(f"    picture {name}: {flow.shape[0]}x{flow.shape[1]}, rad_max {float(rad_max):g}")
    finally:
        PC.flow_uv_to_colors = inner
    assert (out["pic_zero_img"] == 255).all()
    nan = (np.arange(30).reshape(3, 5, 2) / 4 - 3).astype(np.float32)
    inf = nan.copy()
    nan[1, 2, 0] = np.nan
    inf[1, 2, 1] = np.inf
    out["pic_nan_flow"], out["pic_inf_flow"] = nan, inf


def main():
    MGP._install_stubs()
    import pgdvs.preprocess.common as PC
    import pgdvs.preprocess.compute_flow as CF

    torch.manual_seed(0)
    torch.set_num_threads(1)
    assert int(np.__version__.split(".")[0]) >= 2
    out = {}
    blend_fixture(CF, out)
    picture_fixture(PC, out)
    path = OUT / "preprocess_flow_export.npz"
    np.savez_compressed(path, **out)
    size = path.stat().st_size
    print(f"  {path.name} {size / 1024:.1f} KiB, keys {len(out)}")
    assert size < LIMIT, f"{path.name} is {size} bytes, the limit is {LIMIT}"


if __name__ == "__main__":
    main()
