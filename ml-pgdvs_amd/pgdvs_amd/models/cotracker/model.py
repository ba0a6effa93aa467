"""``CoTracker`` (pgdvs/models/cotracker/models/core/cotracker/cotracker.py:73-355), its embeddings (core/embeddings.py),
``bilinear_sample2d`` (core/model_utils.py:75-169) and ``build_cotracker`` (models/build_cotracker.py).

The correlation step of ``forward_iteration`` has two statements.  torch: upstream's ``CorrBlock`` (blocks.py), on the CPU,
when gradients may be asked for (``ops.needs_autograd``), or when the kernels reject the shape.  HIP otherwise:
``ops.cotracker_pyramid`` once per window and ``ops.cotracker_corr_lookup`` per iteration, which writes its 196 columns
straight into the 456-wide token buffer, so neither the correlation volume nor the ``cat`` exists.  ``last_corr_path``
says which one the last call took.
"""
import numpy as np
import torch
import torch.nn as nn

from .blocks import BasicEncoder, CorrBlock, UpdateFormer


# ---------------------------------------------------------------- embeddings (core/embeddings.py)
def get_1d_sincos_pos_embed_from_grid(embed_dim, pos):
    """:46-64: pos (M,) -> (M, embed_dim) float64, sines then cosines of pos / 10000^(2 k / embed_dim)"""
    assert embed_dim % 2 == 0
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0))
    out = np.einsum("m,d->md", np.asarray(pos).reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def get_2d_sincos_pos_embed(embed_dim, grid_size):
    """:11-43: (H W, embed_dim); the first half of the channels encodes the column, the second the row"""
    gh, gw = grid_size if isinstance(grid_size, tuple) else (grid_size, grid_size)
    grid = np.stack(np.meshgrid(np.arange(gw, dtype=np.float32), np.arange(gh, dtype=np.float32)), axis=0)
    assert embed_dim % 2 == 0
    return np.concatenate([get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[0]),
                           get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[1])], axis=1)


def get_2d_embedding(xy, C, cat_coords=True):
    """:67-89: [B,N,2] -> [B,N,2 C (+ 2)]: per coordinate sin / cos interleaved over C / 2 frequencies k 1000 / C"""
    B, N, D = xy.shape
    assert D == 2
    div_term = (torch.arange(0, C, 2, device=xy.device, dtype=torch.float32) * (1000.0 / C)).reshape(1, 1, C // 2)
    pes = []
    for k in range(2):
        pe = torch.zeros(B, N, C, device=xy.device, dtype=torch.float32)
        pe[:, :, 0::2] = torch.sin(xy[:, :, k:k + 1] * div_term)
        pe[:, :, 1::2] = torch.cos(xy[:, :, k:k + 1] * div_term)
        pes.append(pe)
    pe = torch.cat(pes, dim=2)
    return torch.cat([xy, pe], dim=2) if cat_coords else pe


# ---------------------------------------------------------------- core/model_utils.py
def bilinear_sample2d(im, x, y):
    """:75-169: im [B,C,H,W] (or [B,N,C,H,W]: map n for point n), x, y [B,N] -> [B,C,N].  Corner indices are clamped to
    the image, the weights are not: outside the image it extrapolates from the border pixels, as upstream."""
    per_point = im.ndim == 5
    B, C, H, W = (im.shape[0],) + tuple(im.shape[-3:])
    N = x.shape[1]
    x, y = x.float(), y.float()
    x0, y0 = torch.floor(x).int(), torch.floor(y).int()
    x1, y1 = x0 + 1, y0 + 1
    xc0, xc1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1)
    yc0, yc1 = y0.clamp(0, H - 1), y1.clamp(0, H - 1)
    base = (torch.arange(B, dtype=torch.int64, device=x.device) * (W * H)).reshape(B, 1)

    def take(yc, xc):
        idx = (base + yc * W + xc).long()  # [B,N]
        if per_point:
            flat = im.permute(0, 3, 4, 1, 2).reshape(B * H * W, N, C)
            return flat[idx.reshape(-1), torch.arange(N, device=x.device).repeat(B)].reshape(B, N, C)
        return im.permute(0, 2, 3, 1).reshape(B * H * W, C)[idx]

    x0f, x1f, y0f, y1f = x0.float(), x1.float(), y0.float(), y1.float()
    out = (((x1f - x) * (y1f - y)).unsqueeze(2) * take(yc0, xc0) + ((x - x0f) * (y1f - y)).unsqueeze(2) * take(yc0, xc1)
           + ((x1f - x) * (y - y0f)).unsqueeze(2) * take(yc1, xc0) + ((x - x0f) * (y - y0f)).unsqueeze(2) * take(yc1, xc1))
    return out.view(B, -1, C).permute(0, 2, 1)


def meshgrid2d(B, Y, X, device="cpu"):
    gy = torch.linspace(0.0, Y - 1, Y, device=device).reshape(1, Y, 1).repeat(B, 1, X)
    gx = torch.linspace(0.0, X - 1, X, device=device).reshape(1, 1, X).repeat(B, Y, 1)
    return gy, gx


def get_points_on_a_grid(grid_size, interp_shape, grid_center=(0, 0), device="cpu"):
    """cotracker.py:32-55: [1, grid_size^2, 2] (x, y), a margin of W // 64 pixels on every side"""
    if grid_size == 1:
        return torch.tensor([interp_shape[1] / 2, interp_shape[0] / 2], device=device)[None, None]
    gy, gx = meshgrid2d(1, grid_size, grid_size, device=device)
    step = interp_shape[1] // 64
    if grid_center[0] != 0 or grid_center[1] != 0:
        gy, gx = gy - grid_size / 2.0, gx - grid_size / 2.0
    gy = step + gy.reshape(1, -1) / float(grid_size - 1) * (interp_shape[0] - step * 2) + grid_center[0]
    gx = step + gx.reshape(1, -1) / float(grid_size - 1) * (interp_shape[1] - step * 2) + grid_center[1]
    return torch.stack([gx, gy], dim=-1).to(device)


def sample_pos_embed(grid_size, embed_dim, coords):
    """cotracker.py:58-70: the 2-D sin-cos embedding of the feature grid, sampled at the tracks' first-frame positions"""
    pe = torch.from_numpy(get_2d_sincos_pos_embed(embed_dim, grid_size)).reshape(grid_size[0], grid_size[1], embed_dim)
    pe = pe.float().unsqueeze(0).to(coords.device)
    return bilinear_sample2d(pe.permute(0, 3, 1, 2), coords[:, 0, :, 0], coords[:, 0, :, 1])


# ---------------------------------------------------------------- the model
class CoTracker(nn.Module):
    def __init__(self, S=8, stride=8, add_space_attn=True, num_heads=8, hidden_size=384, space_depth=12, time_depth=12):
        super().__init__()
        self.S = S
        self.stride = stride
        self.hidden_dim = 256
        self.latent_dim = latent_dim = 128
        self.corr_levels = 4
        self.corr_radius = 3
        self.add_space_attn = add_space_attn
        self.fnet = BasicEncoder(output_dim=latent_dim, stride=stride)
        self.updateformer = UpdateFormer(space_depth=space_depth, time_depth=time_depth, input_dim=456, hidden_size=hidden_size,
                                         num_heads=num_heads, output_dim=latent_dim + 2, mlp_ratio=4.0, add_space_attn=add_space_attn)
        self.norm = nn.GroupNorm(1, latent_dim)
        self.ffeat_updater = nn.Sequential(nn.Linear(latent_dim, latent_dim), nn.GELU())
        self.vis_predictor = nn.Sequential(nn.Linear(latent_dim, 1))
        self.force_torch_corr = False  # tests: the torch statement on the device
        self.last_corr_path = None     # "hip" or "torch", set by forward_iteration

    def _hip_pyramid(self, fmaps, *others):
        """the HIP statement's pyramid, or None where the torch statement has to run"""
        from ... import ops

        if self.force_torch_corr or not fmaps.is_cuda or fmaps.dtype != torch.float32 or ops.needs_autograd(self, fmaps, *others):
            return None
        return ops.cotracker_pyramid(fmaps[0], reject_ok=True)  # None: a shape the kernels reject (a level below 2 x 2)

    def forward_iteration(self, fmaps, coords_init, feat_init=None, vis_init=None, track_mask=None, iters=4):
        """:116-221.  fmaps [1,S,128,H8,W8], coords_init [1,S_init,N,2] in feature pixels, feat_init [1,S,N,128],
        vis_init [1,S_init,N,1], track_mask [1,<=S,N,1] -> (coordinates x stride after every iteration, visibility logits
        [1,S,N], feat_init)."""
        from ... import ops

        B, S_init, N, D = coords_init.shape
        assert D == 2 and B == 1
        S, H8, W8 = fmaps.shape[1], fmaps.shape[3], fmaps.shape[4]
        device = fmaps.device
        if S_init < S:
            coords = torch.cat([coords_init, coords_init[:, -1].repeat(1, S - S_init, 1, 1)], dim=1)
            vis_init = torch.cat([vis_init, vis_init[:, -1].repeat(1, S - S_init, 1, 1)], dim=1)
        else:
            coords = coords_init.clone()

        pyramid = self._hip_pyramid(fmaps, coords_init, feat_init)
        self.last_corr_path = "torch" if pyramid is None else "hip"
        fcorr_fn = CorrBlock(fmaps, num_levels=self.corr_levels, radius=self.corr_radius) if pyramid is None else None

        ffeats = feat_init.clone()
        pos_embed = sample_pos_embed(grid_size=(H8, W8), embed_dim=456, coords=coords)  # [1,456,N]
        pos_embed = pos_embed.permute(0, 2, 1).reshape(B * N, 456).unsqueeze(1)
        times = torch.linspace(0, S - 1, S).numpy()
        times_embed = torch.from_numpy(get_1d_sincos_pos_embed_from_grid(456, times))[None].repeat(B, 1, 1).float().to(device)

        if track_mask.shape[1] < vis_init.shape[1]:
            track_mask = torch.cat(
                [track_mask, torch.zeros_like(track_mask[:, 0]).repeat(1, vis_init.shape[1] - track_mask.shape[1], 1, 1)], dim=1)
        # upstream joins the two along the TRACK axis and then reads the result as [N,S,2]: a token's two flags come from
        # wherever that reshape finds them.  The weights were trained on it; kept.
        concat = torch.cat([track_mask, vis_init], dim=2).permute(0, 2, 1, 3).reshape(B * N, S, 2)

        coord_predictions = []
        for _ in range(iters):
            coords = coords.detach()
            flows_ = (coords - coords[:, 0:1]).permute(0, 2, 1, 3).reshape(B * N, S, 2)
            flows_cat = get_2d_embedding(flows_, 64, cat_coords=True)  # [N,S,130]
            if pyramid is None:
                fcorr_fn.corr(ffeats)
                fcorrs_ = fcorr_fn.sample(coords).permute(0, 2, 1, 3).reshape(B * N, S, -1)  # [N,S,196]
                ffeats_ = ffeats.permute(0, 2, 1, 3).reshape(B * N, S, self.latent_dim)
                transformer_input = torch.cat([flows_cat, fcorrs_, ffeats_, concat], dim=2)
            else:
                tokens = torch.empty((S, N, 456), dtype=torch.float32, device=device)  # frame-major, as ffeats and coords are
                tokens[:, :, :130] = flows_cat.permute(1, 0, 2)
                ops.cotracker_corr_lookup(pyramid, ffeats[0], coords[0], out=tokens, col_offset=130)
                tokens[:, :, 326:454] = ffeats[0]
                tokens[:, :, 454:] = concat.permute(1, 0, 2)
                transformer_input = tokens.permute(1, 0, 2)
            x = (transformer_input + pos_embed + times_embed).reshape(B, N, S, 456)

            delta = self.updateformer(x).reshape(B * N, S, self.latent_dim + 2)
            delta_coords_ = delta[:, :, :2]
            delta_feats_ = delta[:, :, 2:].reshape(B * N * S, self.latent_dim)
            ffeats_ = ffeats.permute(0, 2, 1, 3).reshape(B * N * S, self.latent_dim)
            ffeats_ = self.ffeat_updater(self.norm(delta_feats_)) + ffeats_
            ffeats = ffeats_.reshape(B, N, S, self.latent_dim).permute(0, 2, 1, 3)  # [B,S,N,C]
            coords = coords + delta_coords_.reshape(B, N, S, 2).permute(0, 2, 1, 3)
            coord_predictions.append(coords * self.stride)

        vis_e = self.vis_predictor(ffeats.reshape(B * S * N, self.latent_dim)).reshape(B, S, N)
        return coord_predictions, vis_e, feat_init

    def forward(self, rgbs, queries, iters=4, feat_init=None, is_train=False):
        """:223-355.  rgbs [1,T,3,H,W] in 0..255, queries [1,N,3] (t, x, y) -> (tracks [1,T,N,2], feat_init, visibility
        [1,T,N] after the sigmoid, training records or None).  Windows of S frames every S / 2; a short last window repeats
        its last frame; a query joins at the first window that reaches its frame."""
        B, T, C, H, W = rgbs.shape
        N = queries.shape[1]
        device = rgbs.device
        assert B == 1
        half = self.S // 2
        first_inds = queries[:, :, 0].long()
        # upstream's sort leaves the order of queries that start on the same frame to the backend, and its flag reshape in
        # forward_iteration makes the result depend on that order (0.02 px on the fixtures; a stable sort moves them as well).
        # The sort runs on the host, so that every device computes what the reference computes on the CPU (N indices, once
        # per call).
        _, sort_inds = torch.sort(first_inds[0].cpu(), dim=0, descending=False)
        sort_inds = sort_inds.to(device)
        inv_sort_inds = torch.argsort(sort_inds, dim=0)
        first_sorted = first_inds[0][sort_inds]

        coords_init = queries[:, :, 1:].reshape(B, 1, N, 2).repeat(1, self.S, 1, 1) / float(self.stride)
        rgbs = 2 * (rgbs / 255.0) - 1.0
        traj_e = torch.zeros((B, T, N, 2), device=device)
        vis_e = torch.zeros((B, T, N), device=device)
        ind_array = torch.arange(T, device=device)[None, :, None].repeat(B, 1, N)
        track_mask = (ind_array >= first_inds[:, None, :]).unsqueeze(-1)
        vis_init = torch.ones((B, self.S, N, 1), device=device).float() * 10  # logits: close to 1 after the sigmoid

        track_mask_ = track_mask[:, :, sort_inds].clone()
        coords_init_ = coords_init[:, :, sort_inds].clone()
        vis_init_ = vis_init[:, :, sort_inds].clone()

        ind, prev_wind_idx, fmaps_ = 0, 0, None
        vis_predictions, coord_predictions, wind_inds = [], [], []
        coords = vis = None
        while ind < T - half:
            rgbs_seq = rgbs[:, ind:ind + self.S]
            S_local = rgbs_seq.shape[1]
            if S_local < self.S:
                rgbs_seq = torch.cat([rgbs_seq, rgbs_seq[:, -1, None].repeat(1, self.S - S_local, 1, 1, 1)], dim=1)
            S = rgbs_seq.shape[1]
            rgbs_ = rgbs_seq.reshape(B * S, C, H, W)
            if fmaps_ is None:
                fmaps_ = self.fnet(rgbs_)
            else:  # the first half of this window is the second half of the one before
                fmaps_ = torch.cat([fmaps_[half:], self.fnet(rgbs_[half:])], dim=0)
            fmaps = fmaps_.reshape(B, S, self.latent_dim, H // self.stride, W // self.stride)

            curr_wind_points = torch.nonzero(first_sorted < ind + self.S)
            if curr_wind_points.shape[0] == 0:
                ind = ind + half
                continue
            wind_idx = int(curr_wind_points[-1]) + 1

            if wind_idx - prev_wind_idx > 0:
                fmaps_sample = fmaps[:, first_sorted[prev_wind_idx:wind_idx] - ind]
                feat_init_ = bilinear_sample2d(fmaps_sample, coords_init_[:, 0, prev_wind_idx:wind_idx, 0],
                                               coords_init_[:, 0, prev_wind_idx:wind_idx, 1]).permute(0, 2, 1)
                feat_init_ = feat_init_.unsqueeze(1).repeat(1, self.S, 1, 1)
                feat_init = feat_init_ if feat_init is None else torch.cat([feat_init, feat_init_], dim=2)

            if prev_wind_idx > 0:  # tracks of the window before start from its second half, held at its last frame
                new_coords = coords[-1][:, half:] / float(self.stride)
                coords_init_[:, :half, :prev_wind_idx] = new_coords
                coords_init_[:, half:, :prev_wind_idx] = new_coords[:, -1].repeat(1, half, 1, 1)
                new_vis = vis[:, half:].unsqueeze(-1)
                vis_init_[:, :half, :prev_wind_idx] = new_vis
                vis_init_[:, half:, :prev_wind_idx] = new_vis[:, -1].repeat(1, half, 1, 1)

            coords, vis, _ = self.forward_iteration(
                fmaps=fmaps, coords_init=coords_init_[:, :, :wind_idx], feat_init=feat_init[:, :, :wind_idx],
                vis_init=vis_init_[:, :, :wind_idx], track_mask=track_mask_[:, ind:ind + self.S, :wind_idx], iters=iters)
            if is_train:
                vis_predictions.append(torch.sigmoid(vis[:, :S_local]))
                coord_predictions.append([coord[:, :S_local] for coord in coords])
                wind_inds.append(wind_idx)

            traj_e[:, ind:ind + self.S, :wind_idx] = coords[-1][:, :S_local]
            vis_e[:, ind:ind + self.S, :wind_idx] = vis[:, :S_local]
            track_mask_[:, :ind + self.S, :wind_idx] = 0.0
            ind = ind + half
            prev_wind_idx = wind_idx

        traj_e = traj_e[:, :, inv_sort_inds]
        vis_e = torch.sigmoid(vis_e[:, :, inv_sort_inds])
        train_data = (vis_predictions, coord_predictions, wind_inds, sort_inds) if is_train else None
        return traj_e, feat_init, vis_e, train_data


# ---------------------------------------------------------------- models/build_cotracker.py
_CONFIGS = {"cotracker_stride_4_wind_8": (4, 8), "cotracker_stride_4_wind_12": (4, 12), "cotracker_stride_8_wind_16": (8, 16)}


def build_cotracker(checkpoint=None):
    """The model a checkpoint's file name asks for (``cotracker_stride_<stride>_wind_<S>.pth``; None: stride 4, window 8,
    freshly initialised), with the checkpoint loaded strictly."""
    name = "cotracker_stride_4_wind_8" if checkpoint is None else str(checkpoint).split("/")[-1].split(".")[0]
    if name not in _CONFIGS:
        raise ValueError(f"Unknown model name {name}")
    stride, window = _CONFIGS[name]
    model = CoTracker(stride=stride, S=window, add_space_attn=True, space_depth=6, time_depth=6)
    if checkpoint is not None:
        with open(checkpoint, "rb") as f:
            state_dict = torch.load(f, map_location="cpu")
        if "model" in state_dict:
            state_dict = state_dict["model"]
        model.load_state_dict(state_dict)
    return model
