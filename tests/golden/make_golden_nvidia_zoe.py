#!/usr/bin/env python3
"""Golden vectors of the NVIDIA evaluation loader's ZoeDepth branch: the reference's own
pgdvs/datasets/nvidia_eval.py NvidiaDynEvaluationDataset pointed at the synthetic tree of nvidia_zoe_tree.py, with the
stubs of make_golden_nvidia.py, for a fixed share key, a fixed trim / indiv key and "moe", each read from the directory
and from the zip.  Writes nvidia_zoe_items.npz: per setting, container and item the ``depth_range``, the ``depth_src_*``
(bulky ones as shape + digest, plus the SHA-256 of their little-endian bytes for the bit-for-bit comparison), the
``flat_cam_*`` and the ``seq_ids``; and per frame the (type, principle) pair "moe" chose, found from the reference's outputs alone: its ``_read_depth`` under "moe" equals its ``_read_depth`` under exactly
one of the twelve fixed keys (the tree gives every pair its own scale and shift).

The values are those of the NumPy that runs the reference (2.x: the stored 0-d float64 scale and shift promote the aligned
depth and the spatial cloud to float64); ``numpy_version`` records it."""
import hashlib
import pathlib
import sys
import tempfile
import warnings

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as MG  # noqa: E402
import make_golden_nvidia as MN  # noqa: E402
import nvidia_tree as NT  # noqa: E402
import nvidia_zoe_tree as ZT  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
KEEP = ("depth_range", "depth_src_", "flat_cam_", "seq_ids")


def sha256(a):
    """SHA-256 of an array's C-order little-endian bytes, as uint8[32]"""
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).digest(), np.uint8)


def main():
    MG._install_stubs()
    sys.modules["cv2"] = MN._cv2_stub()
    import pgdvs.datasets.nvidia_eval as NE

    warnings.simplefilter("ignore", RuntimeWarning)  # the exact-0 prediction: overflow on the way to float32
    out = {"numpy_version": np.array(np.__version__)}
    with tempfile.TemporaryDirectory() as td:
        ZT.build_tree(td)
        for tag, path in ZT.CONTAINERS.items():
            for setting in ZT.SETTINGS:
                ds = NE.NvidiaDynEvaluationDataset(data_root=td, use_zoe_depth=setting, zoe_depth_data_path=path, **ZT.KW)
                assert ds.zoe_depth_data_path.is_file() == (tag == "zip")
                for n, (f, c) in enumerate(ZT.ITEMS):
                    item = ds[f * NT.N_CAMS + c]
                    assert (ds.zoe_depth_zip_obj is not None) == (tag == "zip")
                    assert item["misc"]["tgt_frame_id"] == f and item["misc"]["tgt_cam_id"] == c
                    for k, v in item.items():
                        if not k.startswith(KEEP):
                            continue
                        v = MN._to_np(v)
                        if k.startswith("depth"):
                            assert v.dtype == np.float32, (k, v.dtype)
                        name = f"{setting}_{tag}_i{n}_{k}"
                        if v.size > 2048:
                            out[f"{name}__shape"], out[f"{name}__digest"] = np.array(v.shape), MN.digest(v)
                            out[f"{name}__sha256"] = sha256(v)  # the digest's sums depend on the CPU's summation order
                        else:
                            out[name] = v
            # the pair "moe" picked on every frame
            moe = NE.NvidiaDynEvaluationDataset(data_root=td, use_zoe_depth="moe", zoe_depth_data_path=path, **ZT.KW)
            moe._get_zip_obj()
            fixed = {}
            for key in moe.zoe_k_dict:
                fixed[key] = NE.NvidiaDynEvaluationDataset(data_root=td, use_zoe_depth=key, zoe_depth_data_path=path, **ZT.KW)
                fixed[key]._get_zip_obj()
            assert [moe.zoe_k_dict[k] for k in moe.zoe_k_dict] == ZT.PAIRS
            choice = []
            for f in range(NT.F):
                d = moe._read_depth(NT.SCENE, f)
                assert d.dtype == np.float64, d.dtype  # NumPy 2 promotion; see the module docstring
                hit = [k for k, ds in fixed.items() if np.array_equal(ds._read_depth(NT.SCENE, f), d, equal_nan=True)]
                assert len(hit) == 1, (f, hit)
                assert moe.zoe_k_dict[hit[0]] == ZT.mean_errors(f)[1], (f, hit)  # the tree's design, ties included
                choice.append(list(moe.zoe_k_dict[hit[0]]))
            out[f"moe_choice_{tag}"] = np.array(choice)
    np.savez_compressed(OUT / "nvidia_zoe_items.npz", items=np.array(ZT.ITEMS), **out)
    print(f"  nvidia_zoe_items.npz {(OUT / 'nvidia_zoe_items.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


if __name__ == "__main__":
    main()
