"""The rest of the flow stage on the host (pgdvs_amd/preprocess/flow.py) against the reference's own results
(tests/golden/preprocess_flow_export.npz, written by make_golden_flow_export.py): FlowFormer's tile origins, Gaussian
weight and blend, and the colour-wheel picture with its PNG files.  Also the helpers the GPU tests share.

Colour criterion (host and device alike, against the fixture's picture; ``check_colour``): every byte within 1 level of the
fixture; a byte may differ only where 255 col, recomputed here in float64 from the bit-exact normalised u, v, lies within
0.01 of an integer; at most 1e-3 of a case's bytes differ.  The only step that cannot match is atan2: 6 ulp in atan2f near
pi is 1.4e-6, times 27 / pi that is 1.2e-5 in fk, times the steepest wheel step (0.25, the 4-entry green-to-cyan segment)
and 255 below 1e-3 of a level, a tenth of the window.  A wrong table entry, a swapped channel or a missing wrap moves bytes
by whole levels far from integers.  The reference against a correctly rounded float32 atan2 differs on 5.1e-6 of the bytes of
a 270 x 480 frame, against one pushed 4 ulp on 2.1e-5: fifty times inside the cap.

Weight table: within WEIGHT_ULPS = 2 float32 spacings of the fixture (torch's vectorised exp may differ between CPUs); the
blend itself is fed the fixture's table and must then equal the fixture bit for bit."""
import pathlib
import re

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
WEIGHT_ULPS = 2
COLOUR_WINDOW, COLOUR_SHARE = 0.01, 1e-3


def sigma_tag(sigma):
    return f"s{float(sigma):g}".replace(".", "p")


def load_export_fixture(golden_dir):
    fx = dict(np.load(golden_dir / "preprocess_flow_export.npz"))
    fx["pic_mix_flow"] = np.load(golden_dir / "preprocess_flow.npz")["37x53_mix_flow12"]
    return fx


@pytest.fixture(scope="module")
def fx(golden_dir):
    return load_export_fixture(golden_dir)


def blend_cases(fx):
    return [str(c) for c in fx["blend_cases"]]


def picture_cases(fx):
    return [str(c) for c in fx["picture_cases"]]


def case_tiles(fx, case):
    """the float32 tiles [n,2,ph,pw] of a blend case from the fixture's base vectors and shared pattern"""
    base, pattern = fx[f"blend_{case}_base_q"], fx[f"blend_{case}_pattern_q"]
    tiles = (base[:, :, None, None].astype(np.int32) + pattern[None]).astype(np.float32) / np.float32(4.0)
    tiles.reshape(-1)[fx[f"blend_{case}_negzero"]] = -0.0
    return tiles


def case_shape(case):
    H, W = case.split("x")
    return int(H), int(W)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def levels_f64(u, v):
    """255 col per channel in float64 from the normalised float32 u, v: the colour rule restated with a float64 angle"""
    from pgdvs_amd.preprocess.flow import colour_wheel

    wheel = colour_wheel()
    rad = np.sqrt(u * u + v * v).astype(np.float64)
    u, v = u.astype(np.float64), v.astype(np.float64)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
    k0 = np.clip(np.floor(fk), 0, 54).astype(np.int64)
    k1 = (k0 + 1) % 55
    f = fk - k0
    col = (1 - f)[..., None] * wheel[k0] / 255.0 + f[..., None] * wheel[k1] / 255.0
    col = np.where((rad <= 1)[..., None], 1 - rad[..., None] * (1 - col), col * 0.75)
    return 255 * col


def check_colour(got, want, u, v, what):
    """the colour criterion; returns the share of differing bytes"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape)
    diff = got != want
    share = float(diff.mean())
    print(f"{what}: {int(diff.sum())} of {diff.size} bytes differ ({share:.2e})")
    assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1, what
    lv = levels_f64(u, v)
    near = np.abs(lv - np.round(lv)) < COLOUR_WINDOW
    assert not (diff & ~near).any(), (what, "a byte differs away from an integer level")
    assert share <= COLOUR_SHARE, (what, share)
    return share


def expected_nonfinite(flow):
    """what is defined for a frame with a NaN or an inf: (is rad_max NaN / inf, mask of the pixels that must be 0 0 0, mask
    of those that must be white)"""
    u, v = flow[..., 0], flow[..., 1]
    if np.isnan(flow).any():
        return "nan", np.ones(u.shape, bool), np.zeros(u.shape, bool)
    bad = np.isinf(u) | np.isinf(v)
    return "inf", bad, ~bad


# ---------------------------------------------------------------------------- tiles
def test_tile_origins_equal_upstreams_lists(fx):
    from pgdvs_amd.preprocess import tile_origins

    patch = tuple(int(x) for x in fx["patch"])
    for case in blend_cases(fx):
        assert tile_origins(case_shape(case), patch) == [tuple(o) for o in fx[f"blend_{case}_origins"].tolist()], case
    for case in ("57x109", "100x150"):  # lists upstream gives and cannot blend itself
        assert tile_origins(case_shape(case), patch) == [tuple(o) for o in fx[f"origins_{case}"].tolist()], case
    odd = tile_origins((57, 109), patch)
    assert [h for h, w in odd if w == 0] == [0, 28, 9] and [w for h, w in odd if h == 0] == [0, 44, 45]  # not monotonic
    assert tile_origins((432, 960)) == [(0, 0)]  # a dimension equal to the patch
    assert tile_origins((1080, 1920)) == [(h, w) for h in (0, 412, 648) for w in (0, 940, 960)]
    with pytest.raises(ValueError, match="smaller than the patch"):
        tile_origins((47, 64), patch)
    with pytest.raises(ValueError, match="smaller than the patch"):
        tile_origins((48, 63), patch)
    with pytest.raises(ValueError, match="min_overlap"):
        tile_origins((100, 150), patch, min_overlap=48)


def test_tile_weight_vs_fixture(fx):
    from pgdvs_amd.preprocess import tile_weight

    patch = tuple(int(x) for x in fx["patch"])
    for sigma in fx["sigmas"]:
        w = tile_weight(patch, float(sigma))
        assert isinstance(w, torch.Tensor) and w.dtype == torch.float32 and not w.is_cuda and tuple(w.shape) == patch
        got, want = w.numpy(), fx[f"weight_{sigma_tag(sigma)}"]
        ulps = float((np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)).max())
        print(f"sigma {sigma}: {ulps:.2f} float32 spacings from the fixture")
        assert ulps <= WEIGHT_ULPS, (sigma, ulps)
    w = tile_weight(patch, 0.05).numpy()
    tiny = np.finfo(np.float32).tiny
    assert (w > 0).all() and ((w < tiny) & (w > 0)).any()  # denormals at the rim, no zero
    assert 2e-43 < w[0, 0] < 4e-43


def test_blend_tiles_equals_the_fixture_bit_for_bit(fx):
    from pgdvs_amd.preprocess import blend_tiles

    for case in blend_cases(fx):
        tiles, origins = case_tiles(fx, case), fx[f"blend_{case}_origins"]
        for sigma in fx["sigmas"]:
            got = blend_tiles(tiles, origins, case_shape(case), fx[f"weight_{sigma_tag(sigma)}"])
            assert got.dtype == np.float32 and got.shape == case_shape(case) + (2,)
            assert np.array_equal(bits(got), fx[f"blend_{case}_{sigma_tag(sigma)}_flow_bits"]), (case, sigma)
    # one tile, one pixel: (f w) / w, and the -0.0 of tile 0 comes out as +0 (0 + -0 = +0)
    one = blend_tiles(case_tiles(fx, "48x64"), [(0, 0)], (48, 64), fx["weight_s0p05"])
    t, w = case_tiles(fx, "48x64")[0], fx["weight_s0p05"]
    assert np.array_equal(bits(one), bits((t * w / w).transpose(1, 2, 0) + np.float32(0.0)))
    assert one[0, 0, 0] == 0 and not np.signbit(one[0, 0, 0])
    assert np.abs(one - t.transpose(1, 2, 0)).max() > 0  # the denormal weights do cost bits: (f w) / w is not f
    with pytest.raises(ValueError, match="outside"):  # upstream's own 57x109 list: the tile at row 28 ends at 76
        blend_tiles(np.zeros((9, 2, 48, 64), np.float32), fx["origins_57x109"], (57, 109), fx["weight_s1"])
    with pytest.raises(ValueError, match="uncovered"):
        blend_tiles(np.zeros((1, 2, 48, 64), np.float32), [(0, 0)], (48, 65), fx["weight_s1"])


def test_tiled_flow_reproduces_the_fixture(fx):
    from pgdvs_amd.preprocess import blend_tiles, tile_weight, tiled_flow

    patch = tuple(int(x) for x in fx["patch"])
    for case in blend_cases(fx):
        H, W = case_shape(case)
        tiles, origins = case_tiles(fx, case), [tuple(o) for o in fx[f"blend_{case}_origins"].tolist()]
        seen = []

        def model(t1, t2, tiles=tiles, seen=seen):
            assert tuple(t1.shape) == (1, 3) + patch == tuple(t2.shape)
            seen.append((int(t1[0, 0, 0, 0]), int(t1[0, 1, 0, 0])))
            return torch.from_numpy(tiles[len(seen) - 1][None]), None  # FlowFormer's (flow_pre, _)

        rows = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
        cols = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
        image = torch.stack([rows, cols, rows])[None]  # a tile's first pixel names its origin
        for sigma in fx["sigmas"]:
            del seen[:]
            got = tiled_flow(model, image, image, sigma=float(sigma), patch_size=patch, weight=fx[f"weight_{sigma_tag(sigma)}"])
            assert seen == origins, case
            assert isinstance(got, torch.Tensor) and tuple(got.shape) == (1, 2, H, W) and got.dtype == torch.float32
            hw2 = np.ascontiguousarray(got[0].permute(1, 2, 0).numpy())
            assert np.array_equal(bits(hw2), fx[f"blend_{case}_{sigma_tag(sigma)}_flow_bits"]), (case, sigma)
        del seen[:]
        own = tiled_flow(lambda a, b, tiles=tiles, seen=seen: (seen.append(0), torch.from_numpy(tiles[len(seen) - 1][None]))[1],
                         image, image, sigma=0.05, patch_size=patch)  # a bare tensor, this package's own weight
        want = blend_tiles(tiles, origins, (H, W), tile_weight(patch, 0.05))
        assert np.array_equal(bits(own[0].permute(1, 2, 0).numpy()), bits(want)), case


# ---------------------------------------------------------------------------- picture
def test_flow_to_image_vs_fixture(fx):
    from pgdvs_amd.preprocess import flow_to_image
    from pgdvs_amd.preprocess.flow import flow_normalised

    for name in picture_cases(fx):
        flow = fx[f"pic_{name}_flow"]
        rad_max, u, v = flow_normalised(flow)
        assert rad_max.dtype == np.float32 and u.dtype == np.float32
        assert int(bits(rad_max)[0]) == int(fx[f"pic_{name}_rad_max_bits"]), name
        assert np.array_equal(bits(u), bits(fx[f"pic_{name}_u"])) and np.array_equal(bits(v), bits(fx[f"pic_{name}_v"])), name
        img = flow_to_image(flow)
        assert img.shape == flow.shape[:2] + (3,)
        check_colour(img, fx[f"pic_{name}_img"], fx[f"pic_{name}_u"], fx[f"pic_{name}_v"], f"host {name}")
    assert (flow_to_image(fx["pic_zero_flow"]) == 255).all()
    # the axes: a = +1 / fk = 54 / k1 wraps for (u > 0, v = -0.0); a = -1 / fk = 0 for (u > 0, v = +0.0): different colours
    axis = flow_to_image(fx["pic_axis_flow"]).reshape(-1, 3)
    flat = fx["pic_axis_flow"].reshape(-1, 2)
    assert flat[0, 0] > 0 and not np.signbit(flat[0, 1]) and flat[1, 0] > 0 and np.signbit(flat[1, 1])
    assert tuple(axis[0]) != tuple(axis[1])


def test_flow_to_image_non_finite_frames(fx):
    from pgdvs_amd.preprocess import flow_to_image
    from pgdvs_amd.preprocess.flow import flow_normalised

    for name in ("nan", "inf"):
        flow = fx[f"pic_{name}_flow"]
        kind, black, white = expected_nonfinite(flow)
        rad_max = flow_normalised(flow)[0]
        assert np.isnan(rad_max) if kind == "nan" else np.isposinf(rad_max)
        img = flow_to_image(flow)
        assert (img[black] == 0).all() and (img[white] == 255).all() and black.any()


def test_flow_to_image_argument_checks():
    from pgdvs_amd.preprocess import flow_to_image

    with pytest.raises(ValueError):
        flow_to_image(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError):
        flow_to_image(np.zeros((4, 5), np.float32))


# ---------------------------------------------------------------------------- the tree
def _frames(tmp_path, H, W, n):
    img_dir = tmp_path / "rgbs"
    img_dir.mkdir()
    for i in range(n):
        PIL.Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(img_dir / f"{i:05d}.png")
    return img_dir


def test_run_flow_writes_the_pictures_beside_the_npz(fx, golden_dir, tmp_path):
    from pgdvs_amd.preprocess import flow_to_image, run_flow

    pair = np.load(golden_dir / "preprocess_flow.npz")
    f12, f21 = pair["37x53_mix_flow12"], pair["37x53_mix_flow21"]
    img_dir = _frames(tmp_path, 37, 53, 3)

    def model(img_f1, img_f2):
        return f12.transpose(2, 0, 1)[None], torch.from_numpy(f21.transpose(2, 0, 1)[None].copy())

    out_dir = tmp_path / "flows"
    written = run_flow(img_dir, out_dir, model, img_pair_max_diff=2, flow_png=True)
    assert [p.suffix for p in written] == [".npz"] * 6  # the return value stays the .npz paths
    for k, pairs in ((1, [(0, 1), (1, 2)]), (2, [(0, 2)])):
        want = sorted(f"{a:05d}_{b:05d}{ext}" for i, j in pairs for a, b in ((i, j), (j, i)) for ext in (".npz", ".png"))
        assert sorted(p.name for p in (out_dir / f"interval_{k}").iterdir()) == want
    for path in written:
        flow = np.load(path)["flow"]
        png = np.array(PIL.Image.open(path.with_suffix(".png")))
        assert png.dtype == np.uint8 and np.array_equal(png, flow_to_image(flow)), path.name
    first = np.array(PIL.Image.open(written[0].with_suffix(".png")))
    check_colour(first, fx["pic_mix_img"], fx["pic_mix_u"], fx["pic_mix_v"], "file mix")

    plain = tmp_path / "plain"
    run_flow(img_dir, plain, model, img_pair_max_diff=1)
    assert not [p for p in plain.rglob("*") if p.suffix == ".png"]
    assert sorted(p.name for p in (plain / "interval_1").iterdir()) == sorted(
        f"{a:05d}_{b:05d}.npz" for i in (0, 1) for a, b in ((i, i + 1), (i + 1, i)))


def test_write_flow_pair_leaves_a_given_writer_open(golden_dir, tmp_path):
    from pgdvs_amd.png import PngWriter
    from pgdvs_amd.preprocess import write_flow_pair

    pair = np.load(golden_dir / "preprocess_flow.npz")
    f12, f21 = pair["5x7_mix_flow12"], pair["5x7_mix_flow21"]
    with PngWriter(n_threads=1) as writer:
        write_flow_pair(tmp_path, "a", "b", f12, f21, flow_png=True, writer=writer)
        write_flow_pair(tmp_path, "c", "d", f12, f21, flow_png=True, writer=writer)  # still open
    assert writer.files_written == 4
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_b.npz", "a_b.png", "b_a.npz", "b_a.png", "c_d.npz", "c_d.png", "d_c.npz",
                                                          "d_c.png"]
    write_flow_pair(tmp_path / "", "e", "f", f12, f21, flow_png=True)  # a writer of its own, closed on return
    assert PIL.Image.open(tmp_path / "e_f.png").size == (7, 5)


# ---------------------------------------------------------------------------- ABI
def test_header_declares_and_lib_binds_the_entry_points():
    from pgdvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pgdvs_hip.h").read_text(), flags=re.S)
    for name, nargs in (("pgdvs_flow_tile_blend", 10), ("pgdvs_flow_pair_export", 12), ("pgdvs_flow_pair_export_workspace_bytes", 2)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    head = (ROOT / "include" / "pgdvs_hip.h").read_text()
    assert "compute_flow.py:138-165" in head and "common.py:93-205" in head  # each cites the reference lines it replaces
    lib = _lib.load()
    assert lib.pgdvs_flow_pair_export_workspace_bytes(1080, 1920) >= 8192
    assert lib.pgdvs_flow_pair_export_workspace_bytes(0, 5) == -1


def test_ops_refuse_host_tensors():
    from pgdvs_amd import _lib, ops

    z = torch.zeros((4, 5, 2))
    with pytest.raises(_lib.PgdvsHipError):
        ops.flow_pair_export(z, z)
    with pytest.raises(_lib.PgdvsHipError):
        ops.flow_image(z)
    with pytest.raises(_lib.PgdvsHipError):
        ops.flow_tile_blend(torch.zeros((1, 2, 4, 5)), [(0, 0)], torch.ones((4, 5)), 4, 5)
