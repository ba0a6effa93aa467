"""Seeded weights and inputs of the CoTracker fixtures, shared by tests/golden/make_golden_cotracker.py (which feeds them to
the reference's classes) and the tests (which feed them to pgdvs_amd.models.cotracker and to the HIP ops).  Nothing here is
stored: the fixture holds a float64 checksum of what these functions return, which the tests assert before anything else.

Every value comes from ``numpy.random.default_rng(seed).random()``.  ``fill`` walks a module's ``state_dict()`` in its own
order, so the two sides get equal weights exactly when their key lists are equal (asserted by the tests).
"""
import numpy as np
import torch

F32 = np.float32


def _uniform(rng, shape, half_width=1.0):
    return (2.0 * rng.random(int(np.prod(shape))) - 1.0).reshape(shape) * half_width


def fill(module, seed, gain=None):
    """every tensor of ``module.state_dict()``, in its order: uniform +-sqrt(3 / fan_in) (unit-variance-preserving) times
    ``gain(key)`` (default 1).  fan_in of a weight is its element count per output row, of a 1-D tensor its length; a norm's
    ``weight`` (1-D, no matching ``bias``-less linear layer) is 1 + that."""
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for key, t in sd.items():
            fan_in = t[0].numel() if t.ndim > 1 else t.numel()
            v = _uniform(rng, tuple(t.shape), np.sqrt(3.0 / fan_in)) * (1.0 if gain is None else gain(key))
            if key == "norm.weight":
                v = 1.0 + v
            t.copy_(torch.from_numpy(v).to(t.dtype))
    return module


def tamed_gain(key):
    """the whole-model cases: six refinement iterations of plain random weights are chaotic, these gains keep the updates
    small enough for float32 and float64 to stay together"""
    if key.startswith("updateformer.flow_head"):
        return 0.003
    if ".attn.proj." in key or ".mlp.fc2." in key:
        return 0.3
    return 1.0


def checksum(*arrays_or_modules):
    """float64: the sum of every value plus half the sum of every magnitude (numpy's pairwise sums over the flat arrays:
    the same bits on every machine and thread count)"""
    total = np.float64(0.0)
    for a in arrays_or_modules:
        parts = a.state_dict().values() if isinstance(a, torch.nn.Module) else [a]
        for p in parts:
            v = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
            v = np.ascontiguousarray(v, dtype=np.float64).ravel()
            total = total + v.sum() + 0.5 * np.abs(v).sum()
    return np.float64(total)


# ---------------------------------------------------------------- look-up
# name -> (S, H, W, N, seed).  16 x 24: the last level is 2 x 3, so its 8 x 8 taps pad on every side; 17 x 27: odd sizes on
# levels 0 and 1, pooling drops a row and a column
LOOKUP_CASES = {"even_n37": (3, 16, 24, 37, 11), "even_n1": (3, 16, 24, 1, 12), "odd_n37": (3, 17, 27, 37, 13), "odd_n1": (3, 17, 27, 1, 14)}
N_KINDS = 8


def lookup_inputs(name):
    """fmaps [S,128,H,W], feats [S,N,128] (unit variance), coords [S,N,2] (x, y) and kind [S,N]: 0 interior, 1 exactly
    integral, 2 exactly on 0 / W-1 / H-1, 3 half-pixel, 4 down to -5, 5 x = W + 5 (every tap of level 0 outside: zeros),
    6 anywhere in [-5, extent + 5], 7 y = H + 5 (zeros on level 0 as well)"""
    S, H, W, N, seed = LOOKUP_CASES[name]
    rng = np.random.default_rng(seed)
    fmaps = _uniform(rng, (S, 128, H, W), np.sqrt(3.0)).astype(F32)
    feats = _uniform(rng, (S, N, 128), np.sqrt(3.0)).astype(F32)
    u = rng.random((S, N, 2))
    idx = np.arange(S * N).reshape(S, N)
    kind = ((idx if N > 1 else idx * 3 + 2) % N_KINDS).astype(np.int64)  # N = 1: kinds 2, 5, 0
    ext = np.array([W, H], dtype=np.float64)
    inner = 1.0 + u * (ext - 3.0)
    coords = inner.copy()
    coords[kind == 1] = np.floor(inner[kind == 1])
    corner = np.where(u < 0.5, 0.0, ext - 1.0)
    coords[kind == 2] = corner[kind == 2]
    coords[kind == 3] = np.floor(inner[kind == 3]) + 0.5
    coords[kind == 4] = -5.0 + u[kind == 4] * 6.0
    coords[kind == 5] = np.stack([np.full(u.shape[:2], W + 5.0), inner[..., 1]], -1)[kind == 5]
    coords[kind == 6] = (-5.0 + u * (ext + 10.0))[kind == 6]
    coords[kind == 7] = np.stack([inner[..., 0], np.full(u.shape[:2], H + 5.0)], -1)[kind == 7]
    return fmaps, feats, coords.astype(F32), kind


# ---------------------------------------------------------------- one refinement step, fnet
STEP = dict(S=8, N=24, H=16, W=24, seed_w=21, seed_x=22)
FNET_SIZES = ((32, 48), (36, 52))  # stride 4; 36 x 52 makes the inner maps 18 x 26, 9 x 13, 5 x 7
FNET_SEED = 23


def step_inputs():
    """forward_iteration's arguments as numpy: fmaps [1,S,128,H,W], coords_init [1,S,N,2], feat_init [1,S,N,128], vis_init
    [1,S,N,1], track_mask [1,S,N,1] (0 / 1)"""
    S, N, H, W = STEP["S"], STEP["N"], STEP["H"], STEP["W"]
    rng = np.random.default_rng(STEP["seed_x"])
    fmaps = _uniform(rng, (1, S, 128, H, W), np.sqrt(3.0)).astype(F32)
    start = 1.0 + rng.random((1, 1, N, 2)) * (np.array([W, H]) - 3.0)
    coords = (start + _uniform(rng, (1, S, N, 2), 1.5)).astype(F32)
    feat = _uniform(rng, (1, 1, N, 128), np.sqrt(3.0)).repeat(S, axis=1).astype(F32)
    vis = _uniform(rng, (1, S, N, 1), 10.0).astype(F32)
    mask = (rng.random((1, S, N, 1)) < 0.6).astype(F32)
    return dict(fmaps=fmaps, coords_init=coords, feat_init=feat, vis_init=vis, track_mask=mask)


def fnet_input(size):
    H, W = size
    rng = np.random.default_rng(FNET_SEED + H)
    return _uniform(rng, (2, 3, H, W), 1.0).astype(F32)


# ---------------------------------------------------------------- the whole model
MODEL_SEED = 31
FORWARD_HW = (64, 96)
FORWARD_ITERS = 6
QUERY_FRAMES = (0, 0, 0, 2, 3, 5, 8, 9)
FORWARD_CASES = {"t10": 10, "t5": 5}  # two windows, the second padded; one padded window


def moving_pattern(T, H, W, seed, scale=255.0):
    """[T,3,H,W] in 0 .. scale: a sum of smooth waves that drifts by (1.5, 0.75) pixels per frame"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((T, 3, H, W))
    waves = rng.random((6, 5))
    for t in range(T):
        x, y = xx - 1.5 * t, yy - 0.75 * t
        for c in range(3):
            acc = 0.0
            for a, b, ph, kx, ky in waves:
                acc = acc + (0.5 + a) * np.sin(2 * np.pi * ((0.02 + 0.1 * kx) * x + (0.02 + 0.1 * ky) * y + ph + 0.3 * c * b))
            out[t, c] = acc
    out = (out - out.min()) / (out.max() - out.min())
    return (out * scale).astype(F32)


def forward_inputs(name):
    """video [1,T,3,H,W] in 0..255 and queries [1,8,3] (t, x, y): the first three on image corners.  With T = 5 the start
    frames are QUERY_FRAMES modulo 5 (0, 0, 0, 2, 3, 0, 3, 4): a query cannot start behind the clip."""
    T = FORWARD_CASES[name]
    H, W = FORWARD_HW
    video = moving_pattern(T, H, W, MODEL_SEED + T)[None]
    rng = np.random.default_rng(MODEL_SEED + 100 + T)
    xy = 4.0 + rng.random((8, 2)) * (np.array([W, H]) - 9.0)
    xy[0], xy[1], xy[2] = (0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0, 0.0)
    t = np.array(QUERY_FRAMES, dtype=np.float64) % T
    return video, np.concatenate([t[:, None], xy], axis=1)[None].astype(F32)


# ---------------------------------------------------------------- predictor and interface
CLIP = dict(T=5, H=40, W=56, seed=41)
LOGIT_09 = float(np.log(0.9 / 0.1))  # the visibility threshold 0.9 as a logit


def clip_inputs():
    """frames [T,H,W,3] in 0..1 and query_points [12,3] (t, row, col)"""
    T, H, W = CLIP["T"], CLIP["H"], CLIP["W"]
    frames = np.ascontiguousarray(moving_pattern(T, H, W, CLIP["seed"], scale=1.0).transpose(0, 2, 3, 1))
    rng = np.random.default_rng(CLIP["seed"] + 1)
    q = np.stack([rng.integers(0, T, 12), rng.integers(0, H, 12), rng.integers(0, W, 12)], axis=1).astype(F32)
    q[0] = (0, 0, 0)
    q[1] = (T - 1, H - 1, W - 1)
    return frames, q
