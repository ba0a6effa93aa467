#!/usr/bin/env python3
"""Golden vectors of the NVIDIA visualisation loader: the reference's own
pgdvs/datasets/nvidia_vis.py NvidiaDynVisualizationDataset pointed at the synthetic tree of nvidia_vis_tree.py, with the
stubs of make_golden_nvidia.py.  Writes nvidia_vis_items.npz in the mono_items.npz style: the whole camera path, then
every key of a few items (digests for bulky arrays)."""
import pathlib
import sys
import tempfile

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as MG  # noqa: E402
import make_golden_nvidia as MN  # noqa: E402
import nvidia_vis_tree as VT  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent


def main():
    MG._install_stubs()
    sys.modules["cv2"] = MN._cv2_stub()
    if not hasattr(np, "mat"):  # the reference's quaternion helper predates NumPy 2 (geometry.py:123)
        np.mat = np.asmatrix
    import pgdvs.datasets.nvidia_vis as NV

    out = {}
    with tempfile.TemporaryDirectory() as td:
        VT.build_tree(td)
        ds = NV.NvidiaDynVisualizationDataset(data_root=td, **VT.KW)
        out["n_items"] = len(ds)
        out["all_tgt_c2w"] = np.stack([e[4] for e in ds.valid_fs])
        out["all_tgt_time"] = np.array([e[2] for e in ds.valid_fs])
        out["all_tgt_idx"] = np.array([e[3] for e in ds.valid_fs])
        for n, idx in enumerate(VT.ITEMS):
            item = ds[idx]
            out[f"i{n}_keys"] = np.array(sorted(item.keys()))
            out[f"i{n}_misc"] = np.array([item["misc"]["tgt_time"], item["misc"]["tgt_idx"]], np.float64)
            assert item["misc"]["scene_id"] == item["scene_id"] == VT.SCENE
            for k, v in item.items():
                if k in ("scene_id", "misc"):
                    continue
                v = MN._to_np(v)
                if k.startswith("dyn_rgb") or k.startswith("static_rgb"):
                    continue  # = rgb * mask / rgb * (1 - mask): checked from those in the test
                if k.startswith("rgb_"):
                    q = np.round(v * 255.0)
                    assert np.abs(q / 255.0 - v).max() < 1e-6
                    v = q.astype(np.uint8)
                elif "mask" in k:
                    assert set(np.unique(v)) <= {0.0, 1.0}
                    v = v.astype(np.uint8)
                if v.size > 2048:
                    out[f"i{n}_{k}__shape"], out[f"i{n}_{k}__digest"] = np.array(v.shape), MN.digest(v)
                else:
                    out[f"i{n}_{k}"] = v
    np.savez_compressed(OUT / "nvidia_vis_items.npz", items=np.array(VT.ITEMS), **out)
    print(f"  nvidia_vis_items.npz {(OUT / 'nvidia_vis_items.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


if __name__ == "__main__":
    main()
