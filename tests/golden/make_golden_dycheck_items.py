#!/usr/bin/env python3
"""Golden vectors for the DyCheck iPhone loader (DESIGN.md 8f-3 DyCheck): the reference's own
``pgdvs.datasets.dycheck_iphone_eval.DyCheckiPhoneEvaluationDataset`` pointed at the synthetic tree of dycheck_tree.py, for
the three ``spatial_src_view_type``s.  Stubs: make_golden's module stand-ins, the cv2 stand-in of make_golden_nvidia.py
(the tree only exercises equal-size resizes), the real sklearn KMeans, and a ``dump_json`` that creates the ``splits``
directory first (DyCheck's own io.dump does; upstream's ``open`` fails on a missing directory).  Writes
tests/golden/dycheck_items.npz: exact arrays for cameras, selections, times and depth_range, ``digest`` fingerprints for
images, and the indices of items on which the reference raises (the clustered rule's train-list-index quirk)."""
import os
import pathlib
import sys
import tempfile

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import dycheck_tree as DT  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_nvidia as MN  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
TYPES = ["closest_wo_temporal", "closest_with_temporal", "clustered"]
KW = dict(raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
          scene_ids=[DT.SCENE], n_src_views_spatial=3, n_src_views_spatial_cluster=4, n_src_views_temporal_track_one_side=2,
          flow_consist_thres=1.0)


def main():
    MG._install_stubs()
    sys.modules["cv2"] = MN._cv2_stub()
    del sys.modules["sklearn.cluster"]
    import sklearn.cluster

    sys.modules["sklearn.cluster"] = sklearn.cluster
    import pgdvs.datasets.dycheck_iphone_eval as DI
    import pgdvs.datasets.dycheck_utils as DU

    dump = DU.iPhoneParser.dump_json

    def dump_json(self, filename, obj, **kw):
        os.makedirs(os.path.dirname(filename), exist_ok=True)
        return dump(self, filename, obj, **kw)

    DU.iPhoneParser.dump_json = dump_json
    out = {}
    with tempfile.TemporaryDirectory() as td:
        DT.build_tree(td)
        for ti, typ in enumerate(TYPES):
            ds = DI.DyCheckiPhoneEvaluationDataset(data_root=td, spatial_src_view_type=typ, **KW)
            if ti == 0:
                out["valid_fs_names"] = np.array([str(e[1]) for e in ds.valid_fs])
                out["valid_fs_ids"] = np.array([[int(e[2]), int(e[3])] for e in ds.valid_fs])
                out["train_c2w"] = ds.train_info_dict[DT.SCENE]["train_c2w"]
                p = ds.parser_dict[DT.SCENE]
                out["train_time_ids"] = p.load_split("train")[1]
                cam = p.load_camera(10, 1)
                out["cam_1_10_intrin"], out["cam_1_10_extrin"] = cam.intrin, cam.extrin
                out["cam_1_10_image_size"] = np.asarray(cam.image_size)
            raising = []
            for i in range(len(ds)):
                try:
                    item = ds[i]
                except ValueError:
                    raising.append(i)
                    continue
                for k, v in item.items():
                    if k == "scene_id" or k.startswith("dyn_rgb") or k.startswith("static_rgb"):
                        continue
                    if k == "misc":
                        assert v["tgt_frame_id"] == ds.valid_fs[i][2] and v["tgt_cam_id"] == ds.valid_fs[i][3]
                        continue
                    v = v.numpy()
                    if k.startswith("rgb_"):
                        v = np.round(v * 255.0).astype(np.uint8)
                    elif "mask" in k:
                        assert set(np.unique(v)) <= {0.0, 1.0}
                        v = v.astype(np.uint8)
                    if v.size > 2048 and k != "depth_range":
                        out[f"{typ}_i{i}_{k}__shape"] = np.array(v.shape)
                        out[f"{typ}_i{i}_{k}__digest"] = MN.digest(v)
                    else:
                        out[f"{typ}_i{i}_{k}"] = v
            out[f"{typ}_raising"] = np.array(raising, np.int64)
            print(f"  {typ}: {len(ds) - len(raising)} items, raising {raising}")
    np.savez_compressed(OUT / "dycheck_items.npz", **out)
    print(f"  dycheck_items.npz {(OUT / 'dycheck_items.npz').stat().st_size / 1024:.1f} KiB, keys {len(out)}")


if __name__ == "__main__":
    main()
