#!/usr/bin/env python3
"""Fixtures of the CoTracker point tracker, made by RUNNING THE REFERENCE'S OWN CLASSES
(pgdvs/models/cotracker/: CorrBlock, BasicEncoder, CoTracker, CoTrackerPredictor, CoTrackerInterface) on the CPU, in
float32 and, after ``model.double()``, in float64.  Like the other generators it runs only in the build container, where
the upstream tree is mounted read-only, under the ``sys.modules`` stubs of make_golden.py.

timm is not installed there.  The reference imports ``timm.models.vision_transformer.{Attention, Mlp}``; this generator
puts ``_TimmStandIn`` in their place: ``Attention`` (qkv, softmax(q k^T / sqrt(head_dim)) v, proj) and ``Mlp`` (fc1,
activation, fc2) with timm's constructor arguments and parameter names.  The stand-in is a RESTATEMENT of those two small
classes: the fixtures pin the reference's code around them, not timm itself.  No trained checkpoint exists there either:
weights are seeded random numbers (tests/cotracker_cases.py), and nothing below says anything about trained weights.

Weights and inputs are not stored: tests/cotracker_cases.py regenerates them from seeds, and the fixture holds a float64
checksum of them (``chk_*``), the reference's float32 outputs (``f32_*``), its float64 outputs (``f64_*``), the measured
tolerances ``tol_*`` = 4 x max |f32 - f64| of that case (both errors are maxima of round-off over sums of the same length
in a different association; a wrong tap, weight, level or window is orders of magnitude above), and the state-dict key and
shape lists of the three builders.

  cotracker_lookup   CorrBlock.corr + .sample: the four cases of cotracker_cases.LOOKUP_CASES
  cotracker_model    one refinement step (forward_iteration, iters = 1 and 2, full-gain weights), fnet at 32 x 48 and
                     36 x 52, CoTracker.forward at 64 x 96 with T = 10 and T = 5 (tamed gains; the generator asserts that
                     the float32/float64 gap is at most 1/50 of the median track displacement), and one
                     CoTrackerInterface call on a 5-frame clip with vis_predictor's bias set to put the median visibility
                     logit on the 0.9 threshold; entries within 4 x the visibility gap of 0.9 are excluded (at most 10 %,
                     asserted here and in the tests; each side of the threshold holds at least 20 %)

Two runs write byte-identical files (fixed seeds, one torch thread, fixed zip timestamps).

Usage:  python tests/golden/make_golden_cotracker.py
"""
import pathlib
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import cotracker_cases as CC  # noqa: E402
from make_golden import OUT, _install_stubs  # noqa: E402
from make_golden_dyn_edges import _save  # noqa: E402

T = torch.from_numpy


class _TimmStandIn:
    class Attention(nn.Module):
        def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0.0, proj_drop=0.0):
            super().__init__()
            self.num_heads = num_heads
            self.scale = (dim // num_heads) ** -0.5
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
            self.attn_drop = nn.Dropout(attn_drop)
            self.proj = nn.Linear(dim, dim)
            self.proj_drop = nn.Dropout(proj_drop)

        def forward(self, x):
            B, N, C = x.shape
            q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
            attn = self.attn_drop(((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1))
            return self.proj_drop(self.proj((attn @ v).transpose(1, 2).reshape(B, N, C)))

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
            super().__init__()
            self.fc1 = nn.Linear(in_features, hidden_features or in_features)
            self.act = act_layer()
            self.drop1 = nn.Dropout(drop)
            self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
            self.drop2 = nn.Dropout(drop)

        def forward(self, x):
            return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


def _reference():
    _install_stubs()
    timm, models, vit = types.ModuleType("timm"), types.ModuleType("timm.models"), types.ModuleType("timm.models.vision_transformer")
    vit.Attention, vit.Mlp = _TimmStandIn.Attention, _TimmStandIn.Mlp
    timm.models, models.vision_transformer = models, vit
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.vision_transformer": vit})
    import pgdvs.models.cotracker.interface as RI
    import pgdvs.models.cotracker.models.build_cotracker as RB
    import pgdvs.models.cotracker.models.core.cotracker.blocks as RK

    sys.modules.pop("cupy", None)  # make_golden's stub: einops asks every module named cupy for its ndarray type
    return RI, RB, RK


def _gap(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def make_lookup(RK):
    out = {}
    for name in CC.LOOKUP_CASES:
        fmaps, feats, coords, kind = CC.lookup_inputs(name)
        res = {}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            blk = RK.CorrBlock(T(fmaps)[None].to(dt), num_levels=4, radius=3)
            blk.corr(T(feats)[None].to(dt))
            res[tag] = blk.sample(T(coords)[None].to(dt))[0].numpy()  # .float() upstream: float32 either way
        zero = (kind == 5) | (kind == 7)
        assert zero.any() and not res["f32"][zero][:, :49].any(), name
        out[f"{name}__f32"], out[f"{name}__f64"] = res["f32"], res["f64"]
        out[f"{name}__tol"] = np.float64(4.0 * _gap(res["f32"], res["f64"]))
        out[f"{name}__chk"] = CC.checksum(fmaps, feats, coords)
        print(f"lookup {name}: gap {_gap(res['f32'], res['f64']):.3g} at magnitude {np.abs(res['f64']).max():.3g}")
    _save(OUT / "cotracker_lookup.npz", out)


def _both(model, run):
    """run(model, dtype) in float32, then in float64 after model.double()"""
    with torch.no_grad():
        a = run(model.float(), torch.float32)
        b = run(model.double(), torch.float64)
    model.float()
    return a, b


def make_model(RI, RB, RK):
    out = {}
    for name in ("cotracker_stride_4_wind_8", "cotracker_stride_4_wind_12", "cotracker_stride_8_wind_16"):
        sd = getattr(RB, "build_" + name)().state_dict()
        out[f"keys__{name}"] = np.array(list(sd.keys()))
        out[f"shapes__{name}"] = np.array([" ".join(map(str, v.shape)) for v in sd.values()])

    # ---- one refinement step, fnet: full-gain weights
    model = CC.fill(RB.build_cotracker(None).eval(), CC.STEP["seed_w"])
    x = CC.step_inputs()
    out["chk_step"] = CC.checksum(model, *x.values())
    for iters in (1, 2):
        def run(m, dt):
            a = {k: T(v).to(dt) for k, v in x.items()}
            preds, vis, _ = m.forward_iteration(iters=iters, **a)
            return torch.stack(preds).numpy(), vis.numpy()
        (c32, v32), (c64, v64) = _both(model, run)
        out[f"f32_step{iters}_coords"], out[f"f64_step{iters}_coords"] = c32, c64
        out[f"f32_step{iters}_vis"], out[f"f64_step{iters}_vis"] = v32, v64
        out[f"tol_step{iters}_coords"], out[f"tol_step{iters}_vis"] = np.float64(4 * _gap(c32, c64)), np.float64(4 * _gap(v32, v64))
        upd = np.abs(c64[-1] - 4.0 * x["coords_init"]).max()
        print(f"step iters={iters}: coords gap {_gap(c32, c64):.3g} px on updates of up to {upd:.3g} px, vis gap {_gap(v32, v64):.3g}")
    for size in CC.FNET_SIZES:
        img = CC.fnet_input(size)
        a, b = _both(model, lambda m, dt: m.fnet(T(img).to(dt)).numpy())
        tag = f"fnet_{size[0]}x{size[1]}"
        out[f"f32_{tag}"], out[f"f64_{tag}"], out[f"tol_{tag}"] = a, b, np.float64(4 * _gap(a, b))
        out[f"chk_{tag}"] = CC.checksum(img)
        print(f"{tag}: gap {_gap(a, b):.3g} at magnitude {np.abs(b).max():.3g}")

    # ---- CoTracker.forward: tamed gains
    model = CC.fill(RB.build_cotracker(None).eval(), CC.MODEL_SEED, CC.tamed_gain)
    out["chk_model"] = CC.checksum(model)
    for name in CC.FORWARD_CASES:
        video, queries = CC.forward_inputs(name)

        def run(m, dt):
            traj, _, vis, _ = m(rgbs=T(video).to(dt), queries=T(queries).to(dt), iters=CC.FORWARD_ITERS)
            return traj.numpy(), vis.numpy()
        (t32, v32), (t64, v64) = _both(model, run)
        started = np.arange(video.shape[1])[None, :, None] >= queries[:, None, :, 0]
        disp = np.linalg.norm(t64 - queries[:, None, :, 1:], axis=-1)[started]
        med, gap = float(np.median(disp)), _gap(t32, t64)
        print(f"forward {name}: tracks gap {gap:.3g} px, median displacement {med:.3g} px, vis gap {_gap(v32, v64):.3g}")
        assert gap <= med / 50.0, "the case cannot tell tracking from not tracking"
        out[f"f32_{name}_tracks"], out[f"f64_{name}_tracks"], out[f"tol_{name}_tracks"] = t32, t64, np.float64(4 * gap)
        out[f"f32_{name}_vis"], out[f"f64_{name}_vis"], out[f"tol_{name}_vis"] = v32, v64, np.float64(4 * _gap(v32, v64))
        out[f"chk_{name}"] = CC.checksum(video, queries)

    # ---- the interface on a clip
    frames, qpts = CC.clip_inputs()
    iface = RI.CoTrackerInterface(None, ori_rgb_range="0_1", query_chunk_size=4096)
    net = CC.fill(iface.model.model, CC.MODEL_SEED, CC.tamed_gain)
    seen = {}
    net.vis_predictor.register_forward_hook(lambda m, i, o: seen.__setitem__("logit", o.detach().double().numpy().copy()))
    net.register_forward_hook(lambda m, i, o: seen.__setitem__("vis", o[2].detach().double().numpy().copy()))
    with torch.no_grad():
        iface(frames=T(frames), query_points=T(qpts))
        bias = np.float32(CC.LOGIT_09 - np.median(seen["logit"]) + float(net.vis_predictor[0].bias))
        net.vis_predictor[0].bias.fill_(float(bias))
        tr32, vb32 = iface(frames=T(frames), query_points=T(qpts))
        vis32 = seen["vis"][0, :, :len(qpts)].T  # [#pt,T]
        # float64: the interface casts the frames to float32 itself, so the predictor is called as the interface calls it
        iface.model.double()
        video = (T(frames).permute(0, 3, 1, 2)[None].double().clamp(0.0, 1.0) * 255.0)
        tr64, vb64 = iface.model(video, queries=T(qpts)[None, :, [0, 2, 1]].double())
        tr64 = torch.clip(tr64[0].permute(1, 0, 2), 0.0)
        vis64 = seen["vis"][0, :, :len(qpts)].T
    tr32, tr64 = tr32.numpy(), tr64.numpy()
    gap_vis = _gap(vis32, vis64)
    excluded = np.abs(vis64 - 0.9) < 4.0 * gap_vis
    share, above = float(excluded.mean()), float((vis64 > 0.9).mean())
    print(f"interface: tracks gap {_gap(tr32, tr64):.3g} px, vis gap {gap_vis:.3g}, excluded {share:.3f}, above 0.9: {above:.3f}")
    assert share <= 0.10 and 0.2 <= above <= 0.8
    assert np.array_equal(vb32.numpy()[~excluded], (vis64 > 0.9)[~excluded])
    out.update(iface_vis_bias=bias, f32_iface_tracks=tr32, f64_iface_tracks=tr64, tol_iface_tracks=np.float64(4 * _gap(tr32, tr64)),
               f32_iface_visibles=vb32.numpy(), f64_iface_vis=vis64, iface_excluded=excluded, chk_iface=CC.checksum(frames, qpts))
    _save(OUT / "cotracker_model.npz", out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    RI, RB, RK = _reference()
    make_lookup(RK)
    make_model(RI, RB, RK)
    for f in ("cotracker_lookup.npz", "cotracker_model.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")
