"""The four stages of upstream's ``pgdvs/preprocess/`` that are its own arithmetic, not a third-party network:

``flow``      forward-backward flow consistency (``coord_diff``), the ``flows/interval_<k>/<a>_<b>.npz`` files every
              loader reads (``datasets._common.read_flow_npz``) and their colour-wheel ``.png`` pictures, around a plug-in
              optical-flow model; FlowFormer's tiled inference (origins, Gaussian weight, blend) around a tile-sized one.
``mask``      the ``flow_epi`` motion mask: epipolar distance of the flow correspondence, gated by flow consistency,
              thresholded and opened with ``disk(1)``.
``zoedepth``  the alignment of a monocular depth prediction with the COLMAP points: their projection, the cubic-spline
              look-ups of the motion mask and the prediction, the median and trimmed-median scale and shift in disparity,
              the error table, and the ``zoe_depths_<type>/<frame>.npz`` files ``datasets.nvidia_eval`` reads, around a
              plug-in depth model.
``final_mask`` upstream's ``combine_masks``: the ``flow_epi`` (or semantic) mask of a frame, the previous frame's result and
              a "how often dynamic" count warped along the backward flow, eroded, grown to whole segments of a plug-in
              segmenter and dilated; and ``run_masks``, the writer of the ``masks/final/<frame>_final.png`` files the
              loaders and ``run_zoedepth`` read.

Each runs in numpy (and scipy) on the host (``device=None``) or in HIP (csrc/preprocess.hip, csrc/flow_export.hip,
csrc/png.hip, csrc/zoe_align.hip, csrc/mask_combine.hip).  ``run_flow`` -> ``run_masks`` -> ``run_zoedepth`` takes a directory
of frames to the tree the loaders read.  Every network (RAFT, FlowFormer, OneFormer, SAM, ZoeDepth) is outside this package."""
from .final_mask import (DYNAMIC_IDS_ADE20K, DYNAMIC_IDS_COCO, combine_masks, cubic_table, run_masks, semantic_mask,  # noqa: F401
                         warp_flow_numpy)
from .flow import (blend_tiles, flow_consistency, flow_to_image, run_flow, tile_origins, tile_weight, tiled_flow,  # noqa: F401
                   write_flow_pair)
from .mask import epipolar_motion_mask, fundamental_matrix  # noqa: F401
from .zoedepth import fit_frame, frame_errors, run_zoedepth, sample_frame  # noqa: F401
