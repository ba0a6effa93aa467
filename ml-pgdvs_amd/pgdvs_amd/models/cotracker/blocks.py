"""The networks of CoTracker (pgdvs/models/cotracker/models/core/cotracker/blocks.py) in plain torch: ``BasicEncoder`` with
its ``ResidualBlock`` (instance norm, the only flavour CoTracker builds), ``UpdateFormer`` with ``AttnBlock``, and
``CorrBlock``, the torch statement of the correlation step that csrc/cotracker.hip fuses.

Upstream takes ``Attention`` and ``Mlp`` from timm and reshapes with einops; neither is a dependency here.  ``Attention``
and ``Mlp`` below carry timm's parameter names (``qkv``, ``proj``, ``fc1``, ``fc2``), so ``state_dict()`` has upstream's keys
and shapes and an upstream checkpoint loads with ``strict=True``.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


class ResidualBlock(nn.Module):
    """:15-74 with norm_fn="instance": InstanceNorm2d without affine parameters or running statistics, so the norms
    contribute nothing to the state dict."""

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = nn.InstanceNorm2d(planes)
        self.norm2 = nn.InstanceNorm2d(planes)
        self.downsample = None
        if stride != 1:
            self.norm3 = nn.InstanceNorm2d(planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class BasicEncoder(nn.Module):
    """:77-220, the deep variant with instance norm: a 7 x 7 stem at stride 2, four two-block stages (64, 96, 128, 128
    channels at strides 1, 2, 2, 2), every stage resampled to H / stride x W / stride (bilinear, align_corners=True),
    concatenated and mixed by a 3 x 3 and a 1 x 1 convolution."""

    def __init__(self, input_dim=3, output_dim=128, stride=8):
        super().__init__()
        self.stride = stride
        self.norm1 = nn.InstanceNorm2d(64)
        self.norm2 = nn.InstanceNorm2d(output_dim * 2)
        self.conv1 = nn.Conv2d(input_dim, 64, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.layer1 = self._stage(64, 64, 1)
        self.layer2 = self._stage(64, 96, 2)
        self.layer3 = self._stage(96, 128, 2)
        self.layer4 = self._stage(128, 128, 2)
        self.conv2 = nn.Conv2d(128 + 128 + 96 + 64, output_dim * 2, kernel_size=3, padding=1)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(output_dim * 2, output_dim, kernel_size=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    @staticmethod
    def _stage(in_planes, planes, stride):
        return nn.Sequential(ResidualBlock(in_planes, planes, stride=stride), ResidualBlock(planes, planes, stride=1))

    def forward(self, x):
        size = (x.shape[-2] // self.stride, x.shape[-1] // self.stride)
        x = self.relu1(self.norm1(self.conv1(x)))
        stages = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = layer(x)
            stages.append(F.interpolate(x, size, mode="bilinear", align_corners=True))
        x = self.conv2(torch.cat(stages, dim=1))
        return self.conv3(self.relu2(self.norm2(x)))


class Attention(nn.Module):
    """timm.models.vision_transformer.Attention as CoTracker uses it (qkv_bias=True, no dropout, no q/k norm): one ``qkv``
    projection, softmax(q k^T / sqrt(head_dim)) v per head, ``proj``."""

    def __init__(self, dim, num_heads=8, qkv_bias=False):
        super().__init__()
        assert dim % num_heads == 0, (dim, num_heads)
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        x = F.scaled_dot_product_attention(q, k, v)  # scale 1 / sqrt(head_dim), timm's
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    """timm.layers.Mlp without dropout: ``fc1``, activation, ``fc2``."""

    def __init__(self, in_features, hidden_features, act_layer=nn.GELU):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, in_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class AttnBlock(nn.Module):
    """:223-248: pre-norm attention and MLP (tanh GELU), LayerNorm without affine parameters, eps 1e-6."""

    def __init__(self, hidden_size, num_heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.attn = Attention(hidden_size, num_heads=num_heads, qkv_bias=True)
        self.norm2 = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.mlp = Mlp(hidden_size, int(hidden_size * mlp_ratio), act_layer=lambda: nn.GELU(approximate="tanh"))

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class UpdateFormer(nn.Module):
    """:331-400: tokens [B, N, T, C]; every time block attends over a track's T frames, and after time block i (i a
    multiple of time_depth / space_depth) a space block attends over a frame's N tracks."""

    def __init__(self, space_depth=12, time_depth=12, input_dim=320, hidden_size=384, num_heads=8, output_dim=130, mlp_ratio=4.0,
                 add_space_attn=True):
        super().__init__()
        self.out_channels = 2
        self.num_heads = num_heads
        self.hidden_size = hidden_size
        self.add_space_attn = add_space_attn
        self.input_transform = nn.Linear(input_dim, hidden_size, bias=True)
        self.flow_head = nn.Linear(hidden_size, output_dim, bias=True)
        self.time_blocks = nn.ModuleList([AttnBlock(hidden_size, num_heads, mlp_ratio=mlp_ratio) for _ in range(time_depth)])
        if add_space_attn:
            self.space_blocks = nn.ModuleList([AttnBlock(hidden_size, num_heads, mlp_ratio=mlp_ratio) for _ in range(space_depth)])
            assert len(self.time_blocks) >= len(self.space_blocks)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)

    def forward(self, input_tensor):
        x = self.input_transform(input_tensor)
        B, N, T, C = x.shape
        every = len(self.time_blocks) // len(self.space_blocks) if self.add_space_attn else 0
        j = 0
        for i, block in enumerate(self.time_blocks):
            x = block(x.reshape(B * N, T, C)).reshape(B, N, T, C)
            if self.add_space_attn and i % every == 0:
                x_space = self.space_blocks[j](x.permute(0, 2, 1, 3).reshape(B * T, N, C))
                x = x_space.reshape(B, T, N, C).permute(0, 2, 1, 3)
                j += 1
        return self.flow_head(x)


def bilinear_sampler(img, coords):
    """:251-266: grid_sample in pixel coordinates (align_corners=True, zero padding)"""
    H, W = img.shape[-2:]
    xgrid, ygrid = coords.split([1, 1], dim=-1)
    xgrid = 2 * xgrid / (W - 1) - 1
    ygrid = 2 * ygrid / (H - 1) - 1
    return F.grid_sample(img, torch.cat([xgrid, ygrid], dim=-1), align_corners=True)


class CorrBlock:
    """:269-328, the torch statement of the correlation step: ``corr`` materialises <track feature, feature map> for
    every track, frame and pixel on every level, ``sample`` reads (2 r + 1)^2 bilinear samples per level around each
    track.  ``ops.cotracker_pyramid`` + ``ops.cotracker_corr_lookup`` compute the same values without the volume."""

    def __init__(self, fmaps, num_levels=4, radius=4):
        B, S, C, H, W = fmaps.shape
        self.S, self.C, self.H, self.W = S, C, H, W
        self.num_levels = num_levels
        self.radius = radius
        self.fmaps_pyramid = [fmaps]
        for _ in range(num_levels - 1):
            pooled = F.avg_pool2d(fmaps.reshape(B * S, C, H, W), 2, stride=2)
            H, W = pooled.shape[-2:]
            fmaps = pooled.reshape(B, S, C, H, W)
            self.fmaps_pyramid.append(fmaps)

    def corr(self, targets):
        B, S, N, C = targets.shape
        assert C == self.C and S == self.S
        self.corrs_pyramid = []
        for fmaps in self.fmaps_pyramid:
            H, W = fmaps.shape[-2:]
            corrs = torch.matmul(targets, fmaps.view(B, S, C, H * W)).view(B, S, N, H, W)
            self.corrs_pyramid.append(corrs / torch.sqrt(torch.tensor(C).float()))

    def sample(self, coords):
        r = self.radius
        B, S, N, D = coords.shape
        assert D == 2
        d = torch.linspace(-r, r, 2 * r + 1)
        # (dy, dx) added to (x, y): the slow index of the (2 r + 1)^2 samples moves x.  Upstream's quirk, kept.
        delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).to(coords.device).view(1, 2 * r + 1, 2 * r + 1, 2)
        out = []
        for i, corrs in enumerate(self.corrs_pyramid):
            H, W = corrs.shape[-2:]
            coords_lvl = coords.reshape(B * S * N, 1, 1, 2) / 2**i + delta
            out.append(bilinear_sampler(corrs.reshape(B * S * N, 1, H, W), coords_lvl).view(B, S, N, -1))
        return torch.cat(out, dim=-1).contiguous().float()
