"""The synthetic NVIDIA tree of nvidia_tree.py in the layout the reference's NvidiaDynVisualizationDataset reads
(pgdvs/datasets/nvidia_vis.py:640-653): it opens source images as ``mv_images/<frame>/camXX.jpg``.  Each camXX.png of
the tree is copied to camXX.jpg byte for byte: PIL opens by content, so the .jpg names decode losslessly to the same
pixels.  Used by the golden generator (make_golden_nvidia_vis.py) and by the tests."""
import pathlib
import shutil

import nvidia_tree as NT

SCENE, F = NT.SCENE, NT.F
KW = dict(raw_data_dir="raw", depth_data_dir="depths", mask_data_dir="masks", flow_data_dir="flows", max_hw=-1, mode="vis",
          scene_ids=[NT.SCENE], n_src_views_spatial=4, n_src_views_temporal_track_one_side=2, flow_consist_thres=1.0,
          vis_center_time=6, n_render_frames=16, vis_time_interval=8, vis_bt_max_disp=8)
ITEMS = [0, 3, 10, 15]  # t = 0 (the first time), 2.4, 8.0, 12 = F - 2 (the last)


def build_tree(root):
    root = NT.build_tree(root)
    for png in sorted((pathlib.Path(root) / "raw" / NT.SCENE / "dense" / "mv_images").glob("*/cam*.png")):
        shutil.copyfile(png, png.with_suffix(".jpg"))
    return root
