"""GPU (MI355X): csrc/mesh.hip through ops.mesh_render and PGDVSDynamicRenderer on the cases of tests/mesh_cases.py --
the reference's own topologies (tests/golden/mesh_edges.npz), pixel centres exactly on vertices, edges and diagonals,
exact depth ties, the closed zero-area band, mirrored and magnified sheets, vertices on and behind the camera plane --
against the naive every-pixel-against-every-face statement of oracle/p3d_second.py (no candidate range, explicit face
list, min (z, index)), the oracle, and the integer-arithmetic expectations; the whole path on the reference's recorded
mesh; the vertex kernel's grid-stride rounds; and the entry point's writes and argument checks.
tests/test_mesh_edges_host.py checks the statements against each other and against float64 without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mesh_cases as mc  # noqa: E402
from mesh_cases import RGB_VS_F64_ATOL  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (checker only)
from oracle import p3d_second as p3d  # noqa: E402
from pgdvs_amd import _lib, ops  # noqa: E402
from pgdvs_amd.instantiate import AttrDict  # noqa: E402
from pgdvs_amd.renderers.pgdvs_renderer_dyn import PGDVSDynamicRenderer  # noqa: E402

DEV = "cuda:0"
ERR_INVALID, ERR_WORKSPACE = -1, -3  # include/pgdvs_hip.h


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()  # fails loudly if the HIP extension is missing


def _render(c):
    r = ops.mesh_render(ops.cam_prep(T(c.cam)), T(c.keep), T(c.pcl), T(c.rgb), c.H, c.W, want_faces=True)
    return N(r["face"]).astype(np.int64), N(r["mask"]), N(r["rgb"]).transpose(1, 2, 0)


# ---------------------------------------------------------------- every case
@pytest.mark.parametrize("name", mc.names())
def test_mesh_render_case(name):
    """winners and mask equal to the float32 naive statement and to the oracle; colours to 1e-6 (and within the host
    test's float64 margin where the float64 winner is the same); the constructed cases' integer expectations directly on
    the GPU result; two runs byte-identical"""
    c = mc.cases()[name]
    face, mask, img = _render(c)
    nv = mc.naive(name)
    o_img, o_mask, o_face = orc.mesh_render(c.keep, c.pcl, c.rgb, c.cam)
    assert np.array_equal(face, nv.face)
    assert np.array_equal(face, o_face)
    assert np.array_equal(mask, nv.mask) and np.array_equal(mask, o_mask)
    np.testing.assert_allclose(img, nv.img, rtol=0, atol=1e-6)
    np.testing.assert_allclose(img, o_img, rtol=0, atol=1e-6)
    if c.expect is not None:
        mc.check_expect(c, face, mask, img)
    hi = mc.naive(name, "f64")
    agree = hi.face == face
    assert np.abs(img.astype(np.float64) - hi.img)[agree].max(initial=0.0) <= RGB_VS_F64_ATOL
    face2, mask2, img2 = _render(c)
    assert np.array_equal(face2, face) and mask2.tobytes() == mask.tobytes() and img2.tobytes() == img.tobytes()


# ---------------------------------------------------------------- the whole path on the reference's recorded mesh
@pytest.mark.parametrize("rm", [0, 1])
def test_renderer_mesh_path_on_reference_record(golden_dir, rm, monkeypatch):
    """compute_dyn_pcl + render_dyn_mesh on dyn_edges_integer's first item, outlier removal off and on: the keep mask
    handed to ops.mesh_render gives the face list the reference handed to Meshes; the vertices and colours at those
    pixels are the recorded ones (tolerances of test_gpu_dyn_edges.py for out_pcl); the image is the naive statement's
    on that face list -- exactly (1e-6) with the path's own vertices and colours, and on the recorded mesh itself up to
    what vertices 1e-5 apart allow: such a vertex moves by up to 1e-5 f / z ~ 4e-4 pixels, a barycentric of a
    pixel-sized face and with it a colour in [0, 1] by about as much (bound 1e-3), and a winner only at a centre that
    close to an edge (at most 0.5 % of the pixels; measured on the CPU stand-in: none, and 3e-7)."""
    g = dict(np.load(golden_dir / "dyn_edges_integer.npz"))
    g = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith("rm0__")}
    fx = {k.split("__", 1)[1]: v for k, v in mc.fixture().items() if k.startswith(f"path_rm{rm}__")}
    H, W = g["dyn_mask_1"].shape[:2]
    cams = ops.cam_prep(T(np.stack([g["flat_cam_1"], g["flat_cam_2"], g["flat_cam_tgt"]])))
    times = T(np.array([g["time_1"], g["time_2"], g["time_tgt"]], np.float32))
    rc = AttrDict(dyn_render_use_flow_consistency=False, dyn_pcl_remove_outlier=bool(rm), dyn_pcl_outlier_knn=int(g["outlier_knn"]),
                  dyn_pcl_outlier_std_thres=float(g["outlier_std_thres"]), dyn_render_type="mesh")
    seen = {}
    real = ops.mesh_render

    def recording(cam_tgt, keep, pcl, rgb, H, W, want_faces=False):
        seen.update(keep=N(keep).reshape(H, W), pcl=N(pcl).reshape(H, W, 3), rgb=N(rgb).reshape(H, W, 3))
        r = real(cam_tgt, keep, pcl, rgb, H, W, want_faces=True)
        seen["face"] = N(r["face"]).astype(np.int64)
        return r

    monkeypatch.setattr(ops, "mesh_render", recording)
    dyn = PGDVSDynamicRenderer(cfg=AttrDict(rgb_range="0_1"), proj_func=None)
    _, _, info = dyn.compute_dyn_pcl(
        dyn_mask_1=T(g["dyn_mask_1"][..., 0]), rgb_1=T(g["rgb_1"]), depth_1=T(g["depth_1"][..., 0]), flow_12=T(g["flow_12"]),
        flow_12_occ_mask=T(g["flow_12_occ_mask"][..., 0]), rgb_2=T(g["rgb_2"]), depth_2=T(g["depth_2"][..., 0]), cam_1=cams[0],
        cam_2=cams[1], cam_tgt=cams[2], times=times, render_cfg=rc)
    rgb, mask = dyn.render_dyn_mesh(keep=info["keep"], pcl_dense=info["pcl_dense"], rgb_dense=info["rgb_dense"], cam_tgt=cams[2],
                                    H=H, W=W)
    img, mask = N(rgb).transpose(1, 2, 0), N(mask)
    keep = seen["keep"] != 0
    assert np.array_equal(keep, fx["keep"] != 0)
    faces = p3d.mesh_faces_from_keep(keep)
    assert np.array_equal(faces, fx["faces"])
    np.testing.assert_allclose(seen["pcl"][keep], fx["verts"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(seen["rgb"][keep], fx["rgbs"], rtol=1e-5, atol=1e-5)
    ids = mc.face_ids_of_list(keep, faces)
    # the naive statement on the reference's faces with the path's own vertices and colours
    own = p3d.render_mesh(p3d.points_to_ndc(g["flat_cam_tgt"], seen["pcl"][keep], "seq", inverse="f64"), faces, seen["rgb"][keep], H, W)
    assert mask.sum() > 100
    assert np.array_equal(seen["face"], np.where(own[2] >= 0, ids[np.maximum(own[2], 0)], -1))
    assert np.array_equal(mask, own[1])
    np.testing.assert_allclose(img, own[0], rtol=0, atol=1e-6)
    # ... and on the recorded mesh
    rec = p3d.render_mesh(p3d.points_to_ndc(g["flat_cam_tgt"], fx["verts"], "seq", inverse="f64"), faces, fx["rgbs"], H, W)
    agree = seen["face"] == np.where(rec[2] >= 0, ids[np.maximum(rec[2], 0)], -1)
    assert (~agree).sum() <= 0.005 * H * W
    assert np.array_equal(mask[agree], rec[1][agree])
    assert np.abs(img - rec[0])[agree].max() <= 1e-3


# ---------------------------------------------------------------- grid stride
@pytest.mark.parametrize("mask_kind", ["tail", "whole"])
def test_mesh_verts_grid_stride_rounds(mask_kind):
    """mesh_verts_kernel runs at most 2048 blocks of 256 threads, so only a frame above 524 288 pixels makes a thread
    take a second round -- this test cannot be small.  724 x 726 = 525 624.  ``tail``: nothing kept below linear index
    524 288 and 80 % above it, so the first kept pixel is found in the second round and every vertex that matters is
    written there; ``whole``: a blob and 30 % of the frame.  Against the oracle (which the host tests hold to the naive
    statement): winners and mask exact."""
    H, W = 724, 726
    assert H * W > 2048 * 256
    cam, pcl, rgb = mc._sheet(H, W, 901, noise=0.2)
    rng = np.random.default_rng(902)
    if mask_kind == "tail":
        keep = (rng.random(H * W) < 0.8) & (np.arange(H * W) >= 2048 * 256)
        keep = keep.reshape(H, W)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        keep = (rng.random((H, W)) < 0.3) | (((xx - 300) ** 2 + (yy - 400) ** 2) < 150 ** 2)
    c = mc.Case(mask_kind, H, W, cam, keep.astype(np.uint8), pcl, rgb, None)
    face, mask, img = _render(c)
    o_img, o_mask, o_face = orc.mesh_render(c.keep, c.pcl, c.rgb, c.cam)
    assert o_mask.sum() > (200 if mask_kind == "tail" else 0.1 * H * W)
    assert np.array_equal(face, o_face)
    assert np.array_equal(mask, o_mask)
    np.testing.assert_allclose(img, o_img, rtol=0, atol=1e-6)


# ---------------------------------------------------------------- the entry point's writes and argument checks
GUARD = 256  # bytes on either side of a buffer (keeps the 256-byte alignment of what lies between)


class _Guarded:
    """``nbytes`` of device memory between two guard blocks, everything filled with 0xA5"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD)

    def body(self, dtype):
        return N(self.buf[GUARD:GUARD + self.nbytes]).view(dtype)

    def guards_intact(self):
        b = N(self.buf)
        return bool(np.all(b[:GUARD] == 0xA5) and np.all(b[GUARD + self.nbytes:] == 0xA5))

    def untouched(self):
        return bool(np.all(N(self.buf) == 0xA5))


def _abi_case():
    H, W = 5, 67  # 335 pixels: the second block of every launch is part empty
    cam, pcl, rgb = mc._sheet(H, W, 911, noise=0.2)
    keep = (np.random.default_rng(912).random((H, W)) < 0.9).astype(np.uint8)
    return H, W, cam, keep, pcl, rgb


@pytest.mark.parametrize("with_faces", [True, False])
def test_mesh_render_writes_only_its_outputs(with_faces):
    H, W, cam, keep, pcl, rgb = _abi_case()
    lib = _lib.load()
    P = H * W
    ws_bytes = int(lib.pgdvs_mesh_render_workspace_bytes(H, W))
    assert ws_bytes >= 256 + 24 * P
    g_img, g_mask, g_face, g_ws = _Guarded(12 * P), _Guarded(4 * P), _Guarded(4 * P), _Guarded(ws_bytes)
    camb, k, p, r = ops.cam_prep(T(cam)), T(keep), T(pcl), T(rgb)
    rc = lib.pgdvs_mesh_render(C.c_void_p(camb.data_ptr()), H, W, C.c_void_p(k.data_ptr()), C.c_void_p(p.data_ptr()),
                               C.c_void_p(r.data_ptr()), g_img.ptr, g_mask.ptr, g_face.ptr if with_faces else C.c_void_p(0),
                               g_ws.ptr, ws_bytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for g in (g_img, g_mask, g_face, g_ws):
        assert g.guards_intact()
    o_img, o_mask, o_face = orc.mesh_render(keep, pcl, rgb, cam)
    assert o_mask.sum() > 50
    assert np.array_equal(g_mask.body(np.float32).reshape(H, W), o_mask)
    np.testing.assert_allclose(g_img.body(np.float32).reshape(3, H, W).transpose(1, 2, 0), o_img, rtol=0, atol=1e-6)
    if with_faces:
        assert np.array_equal(g_face.body(np.int32).reshape(H, W).astype(np.int64), o_face)
    else:
        assert g_face.untouched()


def test_mesh_render_rejects_bad_arguments_and_launches_nothing():
    """a null pointer in any required slot, H = 0 and W = 0 return PGDVS_ERR_INVALID; a workspace one byte short (or null)
    returns PGDVS_ERR_WORKSPACE; in every case outputs and workspace keep their fill"""
    H, W, cam, keep, pcl, rgb = _abi_case()
    lib = _lib.load()
    P = H * W
    ws_bytes = int(lib.pgdvs_mesh_render_workspace_bytes(H, W))
    g_img, g_mask, g_face, g_ws = _Guarded(12 * P), _Guarded(4 * P), _Guarded(4 * P), _Guarded(ws_bytes)
    camb, k, p, r = ops.cam_prep(T(cam)), T(keep), T(pcl), T(rgb)
    good = [C.c_void_p(camb.data_ptr()), H, W, C.c_void_p(k.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(r.data_ptr()),
            g_img.ptr, g_mask.ptr, g_face.ptr, g_ws.ptr, ws_bytes, ops._stream()]

    def call(**changes):
        a = list(good)
        for i, v in changes.items():
            a[int(i[1:])] = v
        rc = lib.pgdvs_mesh_render(*a)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in (g_img, g_mask, g_face, g_ws)), changes
        return rc

    null = C.c_void_p(0)
    for slot in (0, 3, 4, 5, 6, 7):  # cam, keep, pcl, rgb, img, mask
        assert call(**{f"a{slot}": null}) == ERR_INVALID, slot
        assert b"null pointer" in lib.pgdvs_last_error()
    assert call(a1=0) == ERR_INVALID and call(a2=0) == ERR_INVALID and call(a1=-3) == ERR_INVALID
    assert call(a10=ws_bytes - 1) == ERR_WORKSPACE
    assert b"workspace" in lib.pgdvs_last_error()
    assert call(a9=null) == ERR_WORKSPACE
    # and the same buffers with nothing wrong: the call goes through
    assert lib.pgdvs_mesh_render(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(g_mask.body(np.float32).reshape(H, W), orc.mesh_render(keep, pcl, rgb, cam)[1])
