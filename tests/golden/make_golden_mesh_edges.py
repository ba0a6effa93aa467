#!/usr/bin/env python3
"""Topology fixture of the mesh variant, made by RUNNING THE REFERENCE ITSELF.

``render_dyn_mesh`` (pgdvs_renderer_dyn.py:550-604) is plain torch up to the point where it hands vertices and
faces to ``pytorch3d.structures.Meshes``: the vertex ranks of the kept pixels, the two stacks of face candidates,
their concatenation, the in-bounds filter and the ``face_v_idxs > 0`` filter that drops every face touching the
first kept pixel.  This generator runs that function on constructed keep masks and records the face list it
builds, and runs ``compute_dyn_pcl`` with ``dyn_render_type = "mesh"`` on the inputs of dyn_edges_integer's
first item (read from that fixture, not duplicated) to record the mesh the whole path hands over.  Like
make_golden_dyn_edges.py it runs only in the build container, where the upstream tree is mounted read-only,
and imports the reference's modules under the ``sys.modules`` stubs of make_golden.py.  The fixture is data
only (masks, index lists, arrays): tests/mesh_cases.py reads it, tests/test_mesh_edges_host.py replays it against
oracle/ (CPU) and tests/test_gpu_mesh_edges.py against the HIP path.

What the stubs stand in for (and therefore what is NOT pinned by this file), beyond those of make_golden.py
(exact brute-force kNN for pytorch3d.ops.knn_points, the torch scatter for the cupy softsplat kernel):
  * pytorch3d.structures.Meshes -> a recorder that stores ``verts`` and ``faces``;
  * pytorch3d.renderer.MeshRenderer -> a recorder whose call returns zeros [1,H,W,4];
  * cameras_from_opencv_projection, RasterizationSettings, MeshRasterizer, TexturesVertex and the shader stay
    mocks.  pytorch3d's camera, rasteriser and shader are therefore NOT executed: the rasterisation itself
    stays restated (oracle/pgdvs_oracle.c, oracle/p3d_second.py), only the topology and the vertices /
    colours handed to it are the reference's own.

Per topology case ``<case>__keep`` (uint8 [H,W]), ``<case>__faces`` (int64 [#face,3], vertex ranks as the reference
produced them; [0,3] where it built no mesh) and ``<case>__blank`` (whether it took its
``torch.sum(flag_valid_v) == 0`` branch).  The whole-path records ``path_rm0`` / ``path_rm1`` (outlier removal
off / on) hold ``keep`` (= valid_dyn_mask_1), ``verts``, ``faces`` and ``rgbs``.

Two runs write byte-identical files (fixed seeds, one torch thread, fixed zip timestamps).

Usage:  python tests/golden/make_golden_mesh_edges.py
"""
import pathlib
import sys
import types

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_golden import OUT, _install_stubs  # noqa: E402
from make_golden_dyn_edges import KNN, STD_THRES, Ref, _save  # noqa: E402

T = torch.from_numpy


class _Recorder:
    """the two recording stand-ins, installed on the reference module's ``pytorch3d`` name"""

    def __init__(self, RD):
        self.meshes = []
        rec = self

        class Meshes:
            def __init__(self, verts, faces=None, textures=None):
                self.verts, self.faces, self.textures = verts, faces, textures
                rec.meshes.append(self)

        class MeshRenderer:
            def __init__(self, rasterizer=None, shader=None):
                pass

            def __call__(self, mesh):
                h, w = rec.hw
                return torch.zeros((1, h, w, 4))

        RD.pytorch3d.structures.Meshes = Meshes
        RD.pytorch3d.renderer.MeshRenderer = MeshRenderer

    def start(self, h, w):
        self.meshes.clear()
        self.hw = (h, w)


def _topology(ref, rec, keep):
    keep = np.ascontiguousarray(keep, dtype=bool)
    h, w = keep.shape
    rows, cols = torch.nonzero(T(keep), as_tuple=True)
    n = rows.shape[0]
    rec.start(h, w)
    flat_cam = torch.cat([torch.tensor([float(h), float(w)]), torch.eye(4).flatten(), torch.eye(4).flatten()])
    img, msk = ref.dyn.render_dyn_mesh(rows=rows, cols=cols, dyn_mask=T(keep.astype(np.float32))[..., None],
                                       dyn_pcl=torch.zeros((n, 3)), rgbs=torch.zeros((n, 3)), flat_cam=flat_cam)
    assert tuple(img.shape) == (h, w, 3) and tuple(msk.shape) == (h, w, 1)
    blank = len(rec.meshes) == 0
    faces = np.zeros((0, 3), np.int64) if blank else rec.meshes[0].faces[0].numpy().astype(np.int64)
    return dict(keep=keep.astype(np.uint8), faces=faces, blank=np.bool_(blank))


def _masks():
    rng = np.random.default_rng(808)
    out = {}
    for tag, (H, W) in (("a", (37, 61)), ("b", (61, 37))):
        full = np.ones((H, W), bool)
        out[f"all_{tag}"] = full
        m = np.zeros((H, W), bool)
        m[H // 3:, :] = True
        m[H // 3, : W // 2] = False  # the first kept pixel is (H/3, W/2)
        out[f"first_interior_{tag}"] = m
        m = np.zeros((H, W), bool)
        m[5:, :] = True
        m[5, : W - 1] = False  # the first kept pixel is (5, W-1)
        out[f"first_lastcol_{tag}"] = m
        m = np.zeros((H, W), bool)
        m[H - 1, W // 4:] = True  # the first kept pixel is in the last row: no faces at all
        out[f"first_lastrow_{tag}"] = m
        out[f"empty_{tag}"] = np.zeros((H, W), bool)
        m = np.zeros((H, W), bool)
        m[H // 2, W // 2] = True
        out[f"single_{tag}"] = m
        m = np.zeros((H, W), bool)
        m[10:12, 20:22] = True  # both faces of the block touch vertex 0: the blank branch
        out[f"block_{tag}"] = m
        m = m.copy()
        m[3, 7] = True  # a lone earlier pixel takes rank 0: the block keeps its two faces
        out[f"block_lone_{tag}"] = m
        yy, xx = np.mgrid[0:H, 0:W]
        out[f"checker_{tag}"] = (yy + xx) % 2 == 0
        out[f"alt_rows_{tag}"] = yy % 2 == 0
        m = np.zeros((H, W), bool)
        m[H - 1, :] = True
        m[:, W - 1] = True
        out[f"last_row_col_{tag}"] = m
        out[f"random80_{tag}"] = rng.random((H, W)) < 0.8
    out["row_1x40"] = np.ones((1, 40), bool)
    out["col_40x1"] = np.ones((40, 1), bool)
    out["all_2x2"] = np.ones((2, 2), bool)
    return out


def _whole_path(ref, rec, inp, rm):
    """compute_dyn_pcl with dyn_render_type = "mesh": what the reference hands to Meshes"""
    H, W = inp["dyn_mask_1"].shape[:2]
    rc = types.SimpleNamespace(dyn_render_use_flow_consistency=False, dyn_pcl_remove_outlier=rm, dyn_pcl_outlier_knn=KNN,
                               dyn_pcl_outlier_std_thres=STD_THRES, dyn_render_type="mesh")
    fc1, fc2 = T(inp["flat_cam_1"]), T(inp["flat_cam_2"])
    ro, rd, uvs, _, _ = ref.dyn.get_batched_rays(device="cpu", batch_size=1, H=H, W=W, render_stride=1,
                                                 intrinsics=fc1[2:18].reshape(1, 4, 4), c2w=fc1[18:34].reshape(1, 4, 4))
    rec.start(H, W)
    _, valid, info = ref.dyn.compute_dyn_pcl(
        dyn_mask_1=T(inp["dyn_mask_1"]), rgb_1=T(inp["rgb_1"]), uvs_1=uvs, ray_o_1=ro, ray_d_1=rd,
        depth_1=T(inp["depth_1"]), flow_12=T(inp["flow_12"]), flow_12_occ_mask=T(inp["flow_12_occ_mask"]),
        rgb_2=T(inp["rgb_2"]), depth_2=T(inp["depth_2"]), K_2=fc2[2:18].reshape(4, 4), c2w_2=fc2[18:34].reshape(4, 4),
        flat_cam_tgt=T(inp["flat_cam_tgt"]), time_1=torch.tensor(inp["time_1"]), time_2=torch.tensor(inp["time_2"]),
        time_tgt=torch.tensor(inp["time_tgt"]), render_cfg=rc)
    assert len(rec.meshes) == 1
    mesh = rec.meshes[0]
    verts = mesh.verts[0].numpy()
    assert np.array_equal(verts, info["pcl"].numpy())
    return dict(keep=(valid.numpy()[..., 0] != 0).astype(np.uint8), verts=verts.astype(np.float32),
                faces=mesh.faces[0].numpy().astype(np.int64), rgbs=info["pcl_rgbs"].numpy().astype(np.float32))


def main():
    torch.set_num_threads(1)
    _install_stubs()
    ref = Ref()
    rec = _Recorder(ref.RD)
    arrays = {}
    names = []
    for name, keep in _masks().items():
        names.append(name)
        arrays.update({f"{name}__{k}": v for k, v in _topology(ref, rec, keep).items()})
    arrays["cases"] = np.array(names)
    g = dict(np.load(OUT / "dyn_edges_integer.npz"))
    inp = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith("rm0__") and not k.startswith("rm0__out_")}
    for rm in (False, True):
        arrays.update({f"path_rm{int(rm)}__{k}": v for k, v in _whole_path(ref, rec, inp, rm).items()})
    _save(OUT / "mesh_edges.npz", arrays)
    for name in names:
        print(f"  {name:22s} faces {arrays[name + '__faces'].shape[0]:5d}  blank {bool(arrays[name + '__blank'])}")
    for rm in (0, 1):
        print(f"  path_rm{rm}: verts {arrays[f'path_rm{rm}__verts'].shape[0]}, faces {arrays[f'path_rm{rm}__faces'].shape[0]}")
    print(f"  mesh_edges.npz {(OUT / 'mesh_edges.npz').stat().st_size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
