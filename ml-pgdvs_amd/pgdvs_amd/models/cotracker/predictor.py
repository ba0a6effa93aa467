"""``CoTrackerPredictor`` (pgdvs/models/cotracker/predictor.py:20-180): the sparse-query path the renderer uses.  The clip is
resized to 384 x 512, the queries are scaled with it, a 6 x 6 support grid on frame 0 is tracked along and dropped again,
visibility is thresholded at 0.9, and the tracks are scaled back to the clip's size."""
import torch
import torch.nn.functional as F

from .model import build_cotracker, get_points_on_a_grid


class CoTrackerPredictor(torch.nn.Module):
    def __init__(self, checkpoint="cotracker/checkpoints/cotracker_stride_4_wind_8.pth"):
        super().__init__()
        self.interp_shape = (384, 512)
        self.support_grid_size = 6
        self.model = build_cotracker(checkpoint)
        self.model.eval()

    @torch.no_grad()
    def forward(self, video, queries=None, segm_mask=None, grid_size=0, grid_query_frame=0, backward_tracking=False):
        """video [1,T,3,H,W] in 0..255, queries [1,N,3] (t, x, y) -> tracks [1,T,N,2] (x, y), visibilities [1,T,N] bool.
        Only upstream's sparse-query call is built (queries given, no mask, no grid, forward in time): the renderer makes
        no other."""
        if queries is None or segm_mask is not None or grid_size != 0 or backward_tracking:
            raise NotImplementedError("CoTrackerPredictor: only sparse queries without mask, grid or backward tracking")
        return self._compute_sparse_tracks(video, queries, add_support_grid=True)

    def _compute_sparse_tracks(self, video, queries, add_support_grid=False):
        """:96-162"""
        B, T, C, H, W = video.shape
        assert B == 1
        ih, iw = self.interp_shape
        video = F.interpolate(video.reshape(B * T, C, H, W), (ih, iw), mode="bilinear").reshape(B, T, 3, ih, iw)
        queries = queries.clone()
        assert queries.shape[2] == 3, queries.shape
        queries[:, :, 1] *= iw / W
        queries[:, :, 2] *= ih / H
        n_support = self.support_grid_size**2
        if add_support_grid:
            grid_pts = get_points_on_a_grid(self.support_grid_size, self.interp_shape, device=video.device)
            grid_pts = torch.cat([torch.zeros_like(grid_pts[:, :, :1]), grid_pts], dim=2)
            queries = torch.cat([queries, grid_pts], dim=1)
        tracks, _, visibilities, _ = self.model(rgbs=video, queries=queries, iters=6)
        if add_support_grid:
            tracks = tracks[:, :, :-n_support]
            visibilities = visibilities[:, :, :-n_support]
        visibilities = visibilities > 0.9
        tracks[:, :, :, 0] *= W / float(iw)
        tracks[:, :, :, 1] *= H / float(ih)
        return tracks, visibilities
