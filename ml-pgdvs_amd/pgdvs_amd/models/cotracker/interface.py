"""``CoTrackerInterface`` (pgdvs/models/cotracker/interface.py:14-82): the tracker contract of the renderers,
``tracker(frames=[N,H,W,3], query_points=[#pt,3] (t,row,col)) -> (tracks [#pt,N,2] (x,y) >= 0, visibles [#pt,N] bool)``.

``separate_fwd_bwd = True`` makes ``PGDVSDynamicTrackRenderer.run_track`` track the frames before and after the target in
two passes, as the reference does for this tracker (pgdvs_renderer_dyn_track.py:419-459).

``ckpt_path=None`` builds the stride-4, window-8 model with freshly initialised weights: for tests and timing only."""
import logging

import torch

from .predictor import CoTrackerPredictor

LOGGER = logging.getLogger(__name__)

_RANGES = {"0_1": (0.0, 1.0), "0_255": (0.0, 255.0), "-1_1": (-1.0, 1.0)}


class CoTrackerInterface(torch.nn.Module):
    separate_fwd_bwd = True

    def __init__(self, ckpt_path, ori_rgb_range="0_1", query_chunk_size=4096, local_rank=0):
        super().__init__()
        assert ori_rgb_range in _RANGES, ori_rgb_range
        self.ori_rgb_range = ori_rgb_range
        self.query_chunk_size = query_chunk_size
        self.model = CoTrackerPredictor(checkpoint=ckpt_path)
        if ckpt_path is None:
            LOGGER.warning("[CoTracker] no checkpoint given: the weights are freshly initialised")
        else:
            LOGGER.info(f"[CoTracker] Done loading checkpoint from {ckpt_path}")

    def __call__(self, *, frames, query_points):
        frames = frames.permute(0, 3, 1, 2)[None, ...].float()  # [1,N,3,H,W]
        lo, hi = _RANGES[self.ori_rgb_range]
        if self.ori_rgb_range != "0_255":  # modify_rgb_range(src, "0_255", check_range=False, enforce_range=True)
            frames = ((frames - lo) / (hi - lo) if lo != 0.0 else frames).clamp(0.0, 1.0) * 255.0
        query_points = query_points[None, :, [0, 2, 1]]  # (t, row, col) -> (t, x, y)
        tracks, visibles = [], []
        for start in range(0, query_points.shape[1], self.query_chunk_size):
            t, v = self.model(frames, queries=query_points[:, start:start + self.query_chunk_size, :])
            tracks.append(t)
            visibles.append(v)
        tracks = torch.cat(tracks, dim=2)[0].permute(1, 0, 2)  # [#pt,N,2]
        visibles = torch.cat(visibles, dim=2)[0].permute(1, 0)  # [#pt,N]
        return torch.clip(tracks, 0.0), visibles  # positions left of or above the image are clipped, as upstream
