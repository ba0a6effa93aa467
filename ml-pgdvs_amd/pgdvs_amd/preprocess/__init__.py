"""The three stages of upstream's ``pgdvs/preprocess/`` that are its own arithmetic, not a third-party network:

``flow``      forward-backward flow consistency (``coord_diff``) and the ``flows/interval_<k>/<a>_<b>.npz`` files every
              loader reads (``datasets._common.read_flow_npz``), around a plug-in optical-flow model.
``mask``      the ``flow_epi`` motion mask: epipolar distance of the flow correspondence, gated by flow consistency,
              thresholded and opened with ``disk(1)``.
``zoedepth``  the alignment of a monocular depth prediction with the COLMAP points: their projection, the cubic-spline
              look-ups of the motion mask and the prediction, the median and trimmed-median scale and shift in disparity,
              the error table, and the ``zoe_depths_<type>/<frame>.npz`` files ``datasets.nvidia_eval`` reads, around a
              plug-in depth model.

Each runs in numpy (and scipy) on the host (``device=None``) or in HIP (csrc/preprocess.hip, csrc/zoe_align.hip).  The
``flow_epi`` mask is an INPUT of upstream's ``combine_masks`` (compute_mask.py:341-471), which merges it with the semantic
segmentations and propagates it in time; it is not the ``masks/final`` mask the loaders and ``run_zoedepth`` read.
``combine_masks``, the ``masks/final`` writer and every network (RAFT, FlowFormer, OneFormer, SAM, ZoeDepth) are outside
this package."""
from .flow import flow_consistency, run_flow, write_flow_pair  # noqa: F401
from .mask import epipolar_motion_mask, fundamental_matrix  # noqa: F401
from .zoedepth import fit_frame, frame_errors, run_zoedepth, sample_frame  # noqa: F401
