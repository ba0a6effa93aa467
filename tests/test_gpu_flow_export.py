"""The flow stage's kernels on the MI355X (csrc/flow_export.hip, the flow staging of csrc/png.hip) against the reference's
fixture (tests/golden/preprocess_flow_export.npz) and, beyond the fixture's sizes, this package's host path, which
test_flow_export_host.py holds to the same fixture.

tile blend    bit for bit on every fixture case and both sigmas; one 540 x 960 frame at the real 432 x 960 patch; tiles in
              a shuffled order (the accumulation follows the list, not the position); the validation rules.
pair export   coord_diff bit-identical to ops.flow_consistency, rad_max bit for bit, the pictures under the colour criterion
              of test_flow_export_host.py, the adaptive scanlines exactly png.filter_scanlines of the device's own picture;
              the axis directions bit for bit; NaN / inf frames; a frame of more than one grid round of the first pass
              (1024 workgroups of 256 pixels); guard words around every output at out offsets 0..3.
public path   write_flow_pair(device=...) and tiled_flow(device=...) against the host path, bit for bit."""
import numpy as np
import PIL.Image
import pytest
import torch

from test_flow_export_host import (bits, blend_cases, case_shape, case_tiles, check_colour, expected_nonfinite, load_export_fixture,
                                   picture_cases, sigma_tag)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLEND = ("48x64", "53x70", "76x108", "106x154")
PICTURES = ("mix", "zero", "axis", "big", "wide2048", "wide2049")
ROUND = 1024 * 256  # pixels of one grid round of the first pass (csrc/flow_export.hip kP1Blocks kP1Block)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def fx(golden_dir):
    fx = load_export_fixture(golden_dir)
    assert tuple(blend_cases(fx)) == BLEND and tuple(picture_cases(fx)) == PICTURES
    return fx


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def partner(flow):
    """a second flow of the same shape for the pair: the first one mirrored and negated (finite wherever the first is)"""
    return np.ascontiguousarray(-flow[::-1, ::-1])


def picture_of(lines):
    """unfiltered scanlines [H,1+3W] (adaptive off) -> uint8 [H,W,3]"""
    lines = lines.cpu().numpy()
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(lines.shape[0], -1, 3)


def host_uv(flow):
    from pgdvs_amd.preprocess.flow import flow_normalised

    return flow_normalised(flow)


# ---------------------------------------------------------------------------- tile blend
@pytest.mark.parametrize("case", BLEND)
def test_tile_blend_vs_fixture(fx, case):
    from pgdvs_amd import ops

    H, W = case_shape(case)
    tiles, origins = dev(case_tiles(fx, case)), fx[f"blend_{case}_origins"]
    for sigma in fx["sigmas"]:
        got = ops.flow_tile_blend(tiles, origins, dev(fx[f"weight_{sigma_tag(sigma)}"]), H, W)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (H, W, 2)
        assert np.array_equal(bits(got.cpu().numpy()), fx[f"blend_{case}_{sigma_tag(sigma)}_flow_bits"]), (case, sigma)


def test_tile_blend_real_patch_and_shuffled_order(fx):
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess import blend_tiles, tile_origins, tile_weight

    rng = np.random.default_rng(11)
    H, W = 540, 960
    origins = tile_origins((H, W))
    assert origins == [(0, 0), (108, 0)]
    weight = tile_weight((432, 960), 0.05)
    tiny = np.finfo(np.float32).tiny
    assert int(((weight.numpy() < tiny) & (weight.numpy() > 0)).sum()) > 2000  # the denormal rim is in the case
    tiles = (rng.normal(size=(2, 2, 432, 960)) * 30).astype(np.float32)
    want = blend_tiles(tiles, origins, (H, W), weight)
    got = ops.flow_tile_blend(dev(tiles), origins, weight.to(DEV), H, W)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(blend_tiles(tiles, origins, (H, W), weight, device=DEV).cpu().numpy(), want)

    case = "106x154"
    order = rng.permutation(16)
    tiles, origins = case_tiles(fx, case)[order], fx[f"blend_{case}_origins"][order]
    assert not np.array_equal(order, np.arange(16))
    want = blend_tiles(tiles, origins, case_shape(case), fx["weight_s1"])
    got = ops.flow_tile_blend(dev(tiles), origins, dev(fx["weight_s1"]), *case_shape(case))
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert not np.array_equal(bits(want), fx[f"blend_{case}_s1_flow_bits"])  # the order does reach the bits


def test_tile_blend_validation_and_guards(fx):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    H, W, ph, pw, guard = 53, 70, 48, 64, 64
    tiles = dev(np.tile(case_tiles(fx, "53x70"), (33, 1, 1, 1)))  # 132 tiles to draw from
    weight = dev(fx["weight_s1"])
    n_out = H * W * 2
    buf = torch.full((n_out + 2 * guard,), -7.25, dtype=torch.float32, device=DEV)

    def call(origins, n, H=H, W=W):
        org = np.ascontiguousarray(origins, dtype=np.int32)
        return lib.pgdvs_flow_tile_blend(tiles.data_ptr(), org.ctypes.data, n, ph, pw, weight.data_ptr(), H, W,
                                         buf.data_ptr() + 4 * guard, ops._stream())

    good = fx["blend_53x70_origins"]
    assert call(good[:3], 3) == -1 and b"uncovered" in lib.pgdvs_last_error()           # a corner is left out
    assert call(np.tile(good, (33, 1))[:129], 129) == -1 and b"129 tiles" in lib.pgdvs_last_error()
    assert call(np.tile(good, (32, 1)), 128) == 0                                        # 128 are allowed
    assert call([(0, 0), (0, 6), (5, 0), (6, 6)], 4) == -1 and b"outside" in lib.pgdvs_last_error()   # h = 6 > H - ph
    assert call([(0, 0), (0, 6), (5, 0), (5, -1)], 4) == -1 and b"outside" in lib.pgdvs_last_error()
    assert call(fx["origins_57x109"], 9, 57, 109) == -1 and b"outside" in lib.pgdvs_last_error()  # upstream's own 57 x 109 list
    assert call(good, 0) == -1
    torch.cuda.synchronize()
    buf.fill_(-7.25)
    assert call(good, 4) == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:guard] == -7.25).all() and (out[guard + n_out:] == -7.25).all()
    assert np.array_equal(out[guard:guard + n_out].view(np.uint32), fx["blend_53x70_s1_flow_bits"].reshape(-1))
    with pytest.raises(_lib.PgdvsHipError, match="uncovered"):
        ops.flow_tile_blend(tiles[:3], good[:3], weight, H, W)


# ---------------------------------------------------------------------------- pair export
@pytest.mark.parametrize("name", PICTURES)
def test_pair_export_vs_fixture(fx, name):
    from pgdvs_amd import ops, png

    f12 = fx[f"pic_{name}_flow"]
    f21 = partner(f12)
    H, W = f12.shape[:2]
    d12, d21 = dev(f12), dev(f21)
    want_cd = ops.flow_consistency(d12, d21)
    cd1, cd2, rad_max, lines = ops.flow_pair_export(d12, d21, adaptive=False)
    torch.cuda.synchronize()
    assert tuple(lines.shape) == (2, H, 1 + 3 * W) and lines.dtype == torch.uint8 and tuple(rad_max.shape) == (2,)
    assert torch.equal(cd1.view(torch.int32), want_cd[0].view(torch.int32)) and torch.equal(cd2.view(torch.int32), want_cd[1].view(torch.int32))
    rad = bits(rad_max.cpu().numpy())
    assert int(rad[0]) == int(fx[f"pic_{name}_rad_max_bits"]) and int(rad[1]) == int(bits(host_uv(f21)[0])[0]), name
    pic12, pic21 = picture_of(lines[0]), picture_of(lines[1])
    check_colour(pic12, fx[f"pic_{name}_img"], fx[f"pic_{name}_u"], fx[f"pic_{name}_v"], f"MI355X {name}")
    # the partner is the same picture turned round: every vector negated is the opposite hue, so only its own host path can judge it
    from pgdvs_amd.preprocess import flow_to_image

    _, u21, v21 = host_uv(f21)
    check_colour(pic21, flow_to_image(f21), u21, v21, f"MI355X {name} partner (against the host path)")
    # adaptive: the filter choice and the filtered bytes are integer arithmetic on the device's own picture
    cd1b, cd2b, rad_b, filtered = ops.flow_pair_export(d12, d21, adaptive=True)
    torch.cuda.synchronize()
    assert torch.equal(cd1b, cd1) and torch.equal(cd2b, cd2) and torch.equal(rad_b.view(torch.int32), rad_max.view(torch.int32))
    for got, pic in zip(filtered.cpu().numpy(), (pic12, pic21)):
        assert np.array_equal(got, png.filter_scanlines(pic, adaptive=True)), name
    # one picture alone
    rad1, alone = ops.flow_image(d12)
    assert torch.equal(alone, lines[0]) and torch.equal(rad1.view(torch.int32), rad_max[:1].view(torch.int32))
    assert torch.equal(ops.flow_image(d21, adaptive=True)[1], filtered[1])


def test_axis_directions_bit_for_bit(fx):
    """the device atan2f returns the correctly rounded 0, +-pi/2, +-pi and the diagonals' +-pi/4, +-3pi/4 on the axis case"""
    from pgdvs_amd import ops

    _, lines = ops.flow_image(dev(fx["pic_axis_flow"]))
    pic = picture_of(lines)
    assert np.array_equal(pic, fx["pic_axis_img"]), (pic.reshape(-1, 3).tolist(), fx["pic_axis_img"].reshape(-1, 3).tolist())
    flat = pic.reshape(-1, 3)
    assert tuple(flat[0]) != tuple(flat[1])  # (u > 0, v = +0.0): fk = 0; (u > 0, v = -0.0): fk = 54 and k1 wraps
    assert (picture_of(ops.flow_image(dev(fx["pic_zero_flow"]))[1]) == 255).all()


@pytest.mark.parametrize("name", ("nan", "inf"))
def test_non_finite_frames(fx, name):
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess import flow_to_image

    flow = fx[f"pic_{name}_flow"]
    kind, black, white = expected_nonfinite(flow)
    cd1, cd2, rad_max, lines = ops.flow_pair_export(dev(flow), dev(np.zeros_like(flow)), adaptive=False)
    torch.cuda.synchronize()
    rad = rad_max.cpu().numpy()
    assert np.isnan(rad[0]) if kind == "nan" else np.isposinf(rad[0])
    assert rad[1] == 0
    pic = picture_of(lines[0])
    assert black.any() and (pic[black] == 0).all() and (pic[white] == 255).all()
    assert (picture_of(lines[1]) == 255).all()
    assert np.array_equal(flow_to_image(flow, device=DEV), pic)


@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_pair_export_writes_only_its_outputs(off):
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    H, W, guard = 5, 67, 64
    rng = np.random.default_rng(5 + off)
    f12, f21 = (dev((rng.normal(size=(H, W, 2)) * 40).astype(np.float32)) for _ in range(2))
    n = H * W * 2
    fbuf = torch.full((2 * n + 2 + 4 * guard,), -7.25, dtype=torch.float32, device=DEV)  # guard cd1 guard cd2 guard rad_max guard
    n_lines = 2 * H * (1 + 3 * W)
    bbuf = torch.full((n_lines + 2 * guard + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.empty(lib.pgdvs_flow_pair_export_workspace_bytes(H, W), dtype=torch.uint8, device=DEV)
    at = lambda k: fbuf.data_ptr() + 4 * k  # noqa: E731
    for adaptive in (0, 1):
        fbuf.fill_(-7.25)
        bbuf.fill_(0xA5)
        rc = lib.pgdvs_flow_pair_export(f12.data_ptr(), f21.data_ptr(), H, W, adaptive, at(guard), at(2 * guard + n), at(3 * guard + 2 * n),
                                        bbuf.data_ptr() + guard + off, ws.data_ptr(), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        out, lines = fbuf.cpu().numpy(), bbuf.cpu().numpy()
        for lo, hi in ((0, guard), (guard + n, 2 * guard + n), (2 * guard + 2 * n, 3 * guard + 2 * n), (3 * guard + 2 * n + 2, 4 * guard + 2 * n + 2)):
            assert (out[lo:hi] == -7.25).all(), (adaptive, lo)
        assert (lines[:guard + off] == 0xA5).all() and (lines[guard + off + n_lines:] == 0xA5).all(), adaptive
        cd1, cd2, rad_max, want = ops.flow_pair_export(f12, f21, adaptive=bool(adaptive))
        assert np.array_equal(out[guard:guard + n], cd1.cpu().numpy().reshape(-1))
        assert np.array_equal(out[2 * guard + n:2 * guard + 2 * n], cd2.cpu().numpy().reshape(-1))
        assert np.array_equal(out[3 * guard + 2 * n:3 * guard + 2 * n + 2], rad_max.cpu().numpy())
        assert np.array_equal(lines[guard + off:guard + off + n_lines], want.cpu().numpy().reshape(-1)), (adaptive, off)


def test_pair_export_beyond_one_grid_round():
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess import flow_to_image

    H, W = 520, 512
    assert ROUND < H * W < 2 * ROUND
    rng = np.random.default_rng(17)
    f12 = (rng.integers(-64, 65, (H, W, 2)) / 4).astype(np.float32)
    f21 = (rng.integers(-64, 65, (H, W, 2)) / 4).astype(np.float32)
    f12[H - 1, W - 3] = (40.0, -30.25)   # the maxima lie in the second round of either direction
    f21[H - 2, 5] = (-33.5, 41.0)
    d12, d21 = dev(f12), dev(f21)
    cd1, cd2, rad_max, lines = ops.flow_pair_export(d12, d21, adaptive=False)
    want = ops.flow_consistency(d12, d21)
    torch.cuda.synchronize()
    assert torch.equal(cd1.view(torch.int32), want[0].view(torch.int32)) and torch.equal(cd2.view(torch.int32), want[1].view(torch.int32))
    for k, f in enumerate((f12, f21)):
        r, u, v = host_uv(f)
        assert int(bits(rad_max[k:k + 1].cpu().numpy())[0]) == int(bits(r)[0])
        assert float(r) == float(np.sqrt(np.float32(f[..., 0] ** 2 + f[..., 1] ** 2)).reshape(-1)[ROUND:].max())
        check_colour(picture_of(lines[k]), flow_to_image(f), u, v, f"MI355X 520x512 flow {k + 1} (against the host path)")


def test_pair_export_argument_checks():
    from pgdvs_amd import _lib, ops

    lib = _lib.load()
    z = torch.zeros((4, 5, 2), device=DEV)
    with pytest.raises(ValueError):
        ops.flow_pair_export(z, torch.zeros((4, 6, 2), device=DEV))
    with pytest.raises(ValueError):
        ops.flow_pair_export(z, z, out=torch.empty(7, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.flow_image(torch.zeros((4, 5, 3), device=DEV))
    out = torch.empty(4096, dtype=torch.uint8, device=DEV)
    ws = torch.empty(8192, dtype=torch.uint8, device=DEV)
    rad = torch.empty(2, device=DEV)
    cd = torch.empty((2, 4, 5, 2), device=DEV)
    args = lambda H, W, adaptive, c1, c2, nbytes: (z.data_ptr(), z.data_ptr(), H, W, adaptive, c1, c2, rad.data_ptr(), out.data_ptr(),  # noqa: E731
                                                   ws.data_ptr(), nbytes, ops._stream())
    assert lib.pgdvs_flow_pair_export(*args(1, 5, 0, cd[0].data_ptr(), cd[1].data_ptr(), 8192)) == -1   # H = 1 with coord_diff
    assert lib.pgdvs_flow_pair_export(*args(4, 5, 2, cd[0].data_ptr(), cd[1].data_ptr(), 8192)) == -1   # adaptive
    assert lib.pgdvs_flow_pair_export(*args(4, 5, 0, cd[0].data_ptr(), None, 8192)) == -1               # one coord_diff
    assert lib.pgdvs_flow_pair_export(*args(4, 5, 0, cd[0].data_ptr(), cd[1].data_ptr(), 0)) == -1      # workspace
    assert lib.pgdvs_flow_pair_export(*args(4, 5, 0, cd[0].data_ptr(), cd[1].data_ptr(), 8192)) == 0
    torch.cuda.synchronize()
    one_row = ops.flow_image(torch.ones((1, 3, 2), device=DEV))[1]  # the pictures alone take H = 1
    assert tuple(one_row.shape) == (1, 10)


# ---------------------------------------------------------------------------- public path
def test_write_flow_pair_device_equals_host(fx, golden_dir, tmp_path):
    from pgdvs_amd.preprocess import flow_to_image, run_flow, write_flow_pair

    pair = np.load(golden_dir / "preprocess_flow.npz")
    f12, f21 = pair["37x53_mix_flow12"], pair["37x53_mix_flow21"]
    host, device = tmp_path / "host", tmp_path / "device"
    host.mkdir()
    device.mkdir()
    ph = write_flow_pair(host, "a", "b", f12, f21, flow_png=True)
    pd = write_flow_pair(device, "a", "b", f12, f21, device=DEV, flow_png=True)
    assert sorted(p.name for p in device.iterdir()) == ["a_b.npz", "a_b.png", "b_a.npz", "b_a.png"] == sorted(p.name for p in host.iterdir())
    for a, b in zip(ph, pd):
        za, zb = np.load(a), np.load(b)
        for key in ("flow", "coord_diff"):
            assert za[key].dtype == np.float32 and np.array_equal(bits(za[key]), bits(zb[key])), (a.name, key)
        flow = za["flow"]
        _, u, v = host_uv(flow)
        got = np.array(PIL.Image.open(b.with_suffix(".png")))
        assert np.array_equal(got, flow_to_image(flow, device=DEV))
        check_colour(got, np.array(PIL.Image.open(a.with_suffix(".png"))), u, v, f"file {b.name} (against the host path)")
    check_colour(np.array(PIL.Image.open(pd[0].with_suffix(".png"))), fx["pic_mix_img"], fx["pic_mix_u"], fx["pic_mix_v"], "file a_b.png")

    # run_flow around a model that answers on the GPU: the same tree, the same arrays
    img_dir = tmp_path / "rgbs"
    img_dir.mkdir()
    for i in range(2):
        PIL.Image.fromarray(np.zeros((37, 53, 3), np.uint8)).save(img_dir / f"{i:05d}.png")
    g12, g21 = dev(f12.transpose(2, 0, 1)[None]), dev(f21.transpose(2, 0, 1)[None])
    written = run_flow(img_dir, tmp_path / "flows", lambda a, b: (g12, g21), img_pair_max_diff=1, device=DEV, flow_png=True)
    assert sorted(p.name for p in (tmp_path / "flows" / "interval_1").iterdir()) == ["00000_00001.npz", "00000_00001.png", "00001_00000.npz",
                                                                                   "00001_00000.png"]
    for a, b in zip(ph, written):
        za, zb = np.load(a), np.load(b)
        assert np.array_equal(bits(za["flow"]), bits(zb["flow"])) and np.array_equal(bits(za["coord_diff"]), bits(zb["coord_diff"]))


def test_tiled_flow_device_equals_host(fx):
    from pgdvs_amd.preprocess import tiled_flow

    patch = tuple(int(x) for x in fx["patch"])
    case = "76x108"
    H, W = case_shape(case)
    tiles = case_tiles(fx, case)
    image = torch.zeros((1, 3, H, W))
    for where in (None, DEV):
        count = []

        def model(t1, t2, where=where, count=count):
            assert (t1.is_cuda, tuple(t1.shape)) == (where is not None, (1, 3) + patch)
            count.append(0)
            return torch.from_numpy(tiles[len(count) - 1][None]).to(t1.device), None

        got = tiled_flow(model, image, image, sigma=0.05, patch_size=patch, device=where)
        assert tuple(got.shape) == (1, 2, H, W) and got.is_cuda == (where is not None)
        hw2 = np.ascontiguousarray(got[0].permute(1, 2, 0).cpu().numpy())
        if where is None:
            host = hw2
        else:
            assert np.array_equal(bits(hw2), bits(host))
