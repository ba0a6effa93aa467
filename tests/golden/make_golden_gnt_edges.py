#!/usr/bin/env python3
"""Edge fixtures of the static GNT branch's first stage, made by RUNNING THE REFERENCE ITSELF.

gnt_small.npz holds 40 random rays of one benign rig; none of its 1 440 items meets a decision of the gather
(a projection on a border, p.z at or below 0, a mask sample at the 1e-3 threshold, coinciding cameras), it
samples in inverse depth only, with one depth range, one channel count and images of the cameras' own size.
This generator runs the reference's ``Projector``, ``sample_along_camera_ray`` and ``sample_fine_pts`` on
constructed inputs that do meet them and writes ``gnt_edges_*.npz`` next to this script.  Like
make_golden_gnt.py it runs only where the upstream tree is mounted, imports the reference under the stubs of
make_golden.py and copies none of its text; the fixtures are data (inputs, settings, outputs).
tests/test_oracle_gnt_edges.py replays them against oracle/gnt_oracle.py (CPU), tests/test_gpu_gnt_edges.py
against ``ops.gnt_gather`` and ``sample_fine_z`` (HIP path).

Every record runs the reference twice, in float32 and in float64 on the same inputs cast up.  Stored per
gather record ``<item>__<key>`` (an item after the first omits the arrays equal to the first item's):
  inputs   ray_o, ray_d, cam_tgt, cams_src, src_rgbs, featmaps, inv_masks, and V, C (the record uses
           cams_src[:V], featmaps[:V, :C], ...), use_mask, route ("z_in": explicit depths z_in[R,S], the route of
           the fine pass, with the depth_range the kernel is handed next to them (unused by the reference); "range": depth_range ([1,2] or
           [R,2]), S, inv_uniform)
  out_*    the float32 outputs: pts, z_vals, rgb_feat, ray_diff, mask_inbound, mask_invalid, mask
  out64_*  the float64 outputs pts, z_vals, rgb_feat, ray_diff
  err_*    max |float32 - float64| of the reference itself per float output, mag_* the largest magnitude
  m_pix64, m_pz64, m_mval64   pixel location, p.z and bilinear mask value of every (view, ray, sample), float64
  m_same   [V,R,S,4] whether u, v, p.z and the mask value are bit-identical in float32 and float64
  diff_pix, diff_pz, diff_mval   largest float32-to-float64 difference of the case (pixels inside a window of
           one image size around the image, p.z in front of the camera); margin = 64; n_border, n_items

Decision margins (a condition on the inputs).  The five conditions of an item are u >= 0, u <= w-1, v >= 0,
v <= h-1 and p.z > 0; a sixth is mask value > 1e-3.  A condition is settled when its quantity is bit-identical
in float32 and float64 (it sits on the decision by construction: dyadic cameras and points) or when its
distance from the decision is at least 64 x the case's float32-to-float64 difference.  ``mask_inbound`` is the
AND of the first five: where it is 1 all five must be settled, where it is 0 one violated condition must be.
Where that fails in a general (non-dyadic) case the source views' principal points move by a hundredth of a
pixel and the case is run again, a few times at most.  The reference's own decisions must also be the same in
both precisions.  Conditioning rule: the reference's own float32 error of an output may be at most half of the
tolerance the tests use for it (1e-6 relative + absolute for pts and z_vals, 5e-5 for rgb_feat and ray_diff).

Cases (dyadic: view 0 has f = 16, principal point (0, 0), identity pose, (h, w) = (17, 33), so the point
(u, v, 16) projects to exactly (u, v); rays start at the origin, which is the target's and view 0's centre, and are
sampled at power-of-two depths, so every sample of a ray keeps its pixel of view 0; image 17 x 33, feature map 9 x 17):
  gnt_edges_bounds   dyadic.  u in {0, w-1, one ulp beyond each (below 0: the smallest subnormal, the smallest
                     normal and 2^-23), pixel centres of the last column, halves} x v likewise: the four borders,
                     the four corners and one ulp beyond; exact 0 / 1 corner weights.  With and without masks.
  gnt_edges_depth    dyadic.  Samples on view 0's z = 0 plane, behind it, at +-2^-26, +-2^-27, +-2^-30 (both
                     sides of the 1e-8 clamp), +-2^-149; a ray through view 1's centre with a sample on it.
                     Reaches the +-1e6 pixel clamp.
  gnt_edges_angle    general.  View 0 bit-identical to the target camera, view 1 the same centre rotated,
                     views 2-3 general (centres at O(1) from the target's).
  gnt_edges_mask     dyadic.  Masks of isolated pixels and half-planes; samples with mask value exactly 0,
                     2^-10, 2^-9, 1, on the first / last row and column of the masked regions; three pixels holding
                     float32(1e-3) and its neighbours, sampled on their centres.
  gnt_edges_sizes    general.  Cameras at twice the image tensor's size, (h, w) differing between views,
                     feature map 7 x 11; C in {32, 64, 30, 68}, V in {3, 7, 1, 3}, 13 rays (R S V never a multiple
                     of 8); uniform and inverse sampling, per-ray and per-view ranges, one record whose depths come
                     from sample_fine_pts on per-ray ranges (z_in).
  gnt_edges_sampling sample_along_camera_ray (det) for both inv_uniform, per-view and per-ray ranges (two
                     orders of magnitude, some far barely above near), S in {2, 3, 64}; sample_fine_pts (det) for
                     both inv_uniform with all-zero, one-hot and single-dominant-bin weight rows (conditioned, see
                     case_sampling).
  gnt_edges_render   BaseRenderer.forward end to end with the small seeded network of make_golden_gnt.py (rebuilt,
                     its state_dict asserted equal to the w_* arrays of gnt_small.npz): B = 2, render_stride 2,
                     per-ray ranges [B rh rw, 2] cut from a 4-d range map, dynamic masks on.  Records: ``uni``
                     inv_uniform=False with 6 fine samples, chunks of 100 rays; ``inv`` inv_uniform=True without
                     a fine pass, chunks of 37 (384 rays per view: a chunk straddles the two batch items).  The
                     reference's feature maps are stored for the oracle replay.

Numbers of the committed files (printed by a run; diff = largest float32-to-float64 difference of the reference):
  gnt_edges_angle.npz     241.0 KiB  items   640  border    82  diff pix 6.2e-06 pz 4.5e-07 mval 3.0e-06
  gnt_edges_bounds.npz    140.5 KiB  items  1584  border   610  diff pix 2.4e-06 pz 0.0e+00 mval 9.0e-07
  gnt_edges_depth.npz     112.5 KiB  items   810  border    62  diff pix 1.7e-06 pz 6.0e-08 mval 1.2e-07
  gnt_edges_mask.npz      177.6 KiB  items  1296  border   200  diff pix 1.8e-06 pz 0.0e+00 mval 0.0e+00
  gnt_edges_render.npz    625.4 KiB  reference float32 vs float64: coarse 1.3e-05, fine 1.3e-05
  gnt_edges_sampling.npz  310.4 KiB  special weight rows kept: 0-5, 8-10 (all)
  gnt_edges_sizes.npz     576.3 KiB  items   975  border    42  diff pix 1.3e-05 pz 1.2e-06 mval 6.4e-06
  margin 64 everywhere.  (border = items in front of the camera within one pixel of a border of view 0's (h, w).)

Two runs write byte-identical files (fixed seeds, one torch thread, fixed zip timestamps).

Usage:  python tests/golden/make_golden_gnt_edges.py
"""
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_golden import OUT, _flat_cam, _install_stubs, _pose  # noqa: E402
from make_golden_dyn_edges import _save  # noqa: E402

F32, F64 = np.float32, np.float64
MARGIN = 64.0
TOL = {"pts": (1e-6, 1e-6), "z_vals": (1e-6, 1e-6), "rgb_feat": (0.0, 5e-5), "ray_diff": (0.0, 5e-5)}  # (rtol, atol) of the tests
FLOATS = ("pts", "z_vals", "rgb_feat", "ray_diff")
MASKS = ("mask_inbound", "mask_invalid", "mask")
INPUTS = ("ray_o", "ray_d", "cam_tgt", "cams_src", "src_rgbs", "featmaps", "inv_masks", "V", "C", "use_mask", "route", "z_in",
          "depth_range", "S", "inv_uniform")


class Ref:
    def __init__(self):
        from pgdvs.models.gnt.projector import Projector
        from pgdvs.models.gnt.ray_sampler import sample_along_camera_ray, sample_fine_pts

        self.proj = Projector()
        self.sample_along_camera_ray = sample_along_camera_ray
        self.sample_fine_pts = sample_fine_pts

    def sample(self, inp, dt):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
        ro, rd = t(inp["ray_o"]), t(inp["ray_d"])
        if str(inp["route"]) == "z_in":
            z = t(inp["z_in"])
            return z[..., None] * rd[:, None, :] + ro[:, None, :], z
        dr = t(inp["depth_range"])
        if dr.shape[0] == 1:
            dr = dr[torch.zeros(ro.shape[0], dtype=torch.long)]
        return self.sample_along_camera_ray(ro, rd, dr, int(inp["S"]), inv_uniform=bool(inp["inv_uniform"]), det=True)

    def gather(self, inp, dt):
        """one run of the reference in precision dt -> outputs and the decision quantities"""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
        V, C = int(inp["V"]), int(inp["C"])
        pts, z = self.sample(inp, dt)
        cams = t(inp["cams_src"][:V])
        masks = t(inp["inv_masks"][:V])
        with torch.no_grad():
            pr = self.proj.compute(xyz=pts, query_camera=t(inp["cam_tgt"])[None], train_imgs=t(inp["src_rgbs"][:V])[None],
                                   train_cameras=cams[None], featmaps=t(inp["featmaps"][:V, :C]),
                                   train_invalid_masks=masks[None] if bool(inp["use_mask"]) else None)
            pix, infront = self.proj.compute_projections(pts, cams)  # [V,R,S,2], [V,R,S]
            h, w = cams[0][:2]
            mval = torch.nn.functional.grid_sample(masks.permute(0, 3, 1, 2), self.proj.normalize(pix, h, w),
                                                   align_corners=True)[:, 0]  # [V,R,S]
            xyz_h = torch.cat([pts.reshape(-1, 3), torch.ones_like(pts.reshape(-1, 3)[:, :1])], -1)
            P = cams[:, 2:18].reshape(-1, 4, 4) @ torch.inverse(cams[:, 18:34].reshape(-1, 4, 4))
            pz = (P @ xyz_h.t()[None])[:, 2].reshape(infront.shape)
        assert torch.equal(pz > 0, infront)
        r = {"pts": pts, "z_vals": z, "rgb_feat": pr["rgb_feat"], "ray_diff": pr["ray_diff"], "mask_inbound": pr["mask_inbound"],
             "mask": pr["mask"], "mask_invalid": pr.get("mask_invalid", torch.zeros_like(pr["mask"])),
             "pix": pix, "pz": pz, "mval": mval}
        return {k: v.numpy() for k, v in r.items()}


def _window(pix, pz, h, w):
    """items whose projection is in play: in front of the camera and within one image size of the image"""
    return (pz > 1e-3) & (pix[..., 0] > -w) & (pix[..., 0] < 2 * w) & (pix[..., 1] > -h) & (pix[..., 1] < 2 * h)


def _records(ref, items):
    """both runs of every item, the case's float32-to-float64 differences, and whether every decision is settled"""
    runs = {k: (ref.gather(inp, torch.float32), ref.gather(inp, torch.float64)) for k, inp in items.items()}
    diff = {"pix": 0.0, "pz": 0.0, "mval": 0.0}
    for k, (a, b) in runs.items():
        h, w = items[k]["cams_src"][0][:2]
        win = _window(b["pix"], b["pz"], h, w)
        if win.any():
            diff["pix"] = max(diff["pix"], float(np.abs(a["pix"].astype(F64) - b["pix"])[win].max()))
        diff["pz"] = max(diff["pz"], float(np.abs(a["pz"].astype(F64) - b["pz"])[b["pz"] > -1e3].max()))
        diff["mval"] = max(diff["mval"], float(np.abs(a["mval"].astype(F64) - b["mval"]).max()))
    out, bad = {}, 0
    for k, (a, b) in runs.items():
        inp = items[k]
        h, w = (float(x) for x in inp["cams_src"][0][:2])
        u, v, pz, mv = b["pix"][..., 0], b["pix"][..., 1], b["pz"], b["mval"]
        same = np.stack([a["pix"][..., 0].astype(F64) == u, a["pix"][..., 1].astype(F64) == v, a["pz"].astype(F64) == pz,
                         a["mval"].astype(F64) == mv], -1)
        # signed distances (>= 0: condition holds), quantity index and difference of each of the five conditions
        conds = [(u, 0, diff["pix"]), (w - 1.0 - u, 0, diff["pix"]), (v, 1, diff["pix"]), (h - 1.0 - v, 1, diff["pix"])]
        holds = [c >= 0 for c, _, _ in conds] + [pz > 0]
        settled = [same[..., q] | (np.abs(c) >= MARGIN * d) for c, q, d in conds] + [same[..., 2] | (np.abs(pz) >= MARGIN * diff["pz"])]
        inb = np.all(holds, 0)
        ok_in = np.where(inb, np.all(settled, 0), np.any([~hh & ss for hh, ss in zip(holds, settled)], 0))
        ok_mv = same[..., 3] | (np.abs(mv - 1e-3) >= MARGIN * diff["mval"]) | (not bool(inp["use_mask"]))
        bad += int((~ok_in).sum() + (~ok_mv).sum())
        if (~ok_in).any() or (~ok_mv).any():
            ii = np.argwhere(~ok_in | ~ok_mv)[:6]
            print(f"  {k}: unsettled", [(tuple(i), u[tuple(i)], v[tuple(i)], pz[tuple(i)], mv[tuple(i)]) for i in ii], diff)
        # the reference's own decisions are the same in both precisions
        at_thr = (a["mval"] == F32(1e-3)).transpose(1, 2, 0)[..., None]  # the threshold is a float32 constant in that run
        for m in MASKS:
            bad += int(((a[m] != b[m]) & ~(at_thr & (m != "mask_inbound"))).sum())
        assert np.array_equal(b["mask_inbound"][..., 0].transpose(2, 0, 1) > 0, inb)
        near = (pz > 0) & (u >= -1) & (u <= w) & (v >= -1) & (v <= h) & (
            (np.abs(u) <= 1) | (np.abs(u - (w - 1)) <= 1) | (np.abs(v) <= 1) | (np.abs(v - (h - 1)) <= 1))
        rec = {kk: inp[kk] for kk in INPUTS if kk in inp}
        rec.update({"out_" + kk: a[kk] for kk in FLOATS + MASKS})
        rec.update({"out64_" + kk: b[kk] for kk in FLOATS})
        for kk in FLOATS:
            err = np.abs(a[kk].astype(F64) - b[kk])
            rtol, atol = TOL[kk]
            if np.any(err > 0.5 * (atol + rtol * np.abs(b[kk]))):
                raise RuntimeError(f"{k}: the reference's own float32 error of {kk} ({err.max():.2e}) exceeds half the tolerance: "
                                   "ill-conditioned inputs")
            rec["err_" + kk], rec["mag_" + kk] = F64(err.max()), F64(np.abs(b[kk]).max())
        rec.update(m_pix64=b["pix"], m_pz64=pz, m_mval64=mv, m_same=same, n_border=np.int64(near.sum()), n_items=np.int64(near.size))
        out[k] = rec
    for rec in out.values():
        rec.update(diff_pix=F64(diff["pix"]), diff_pz=F64(diff["pz"]), diff_mval=F64(diff["mval"]), margin=F64(MARGIN))
    return out, bad


def _write_case(name, items):
    """an item stores only the arrays that differ from the first item's (the tests merge them back)"""
    arrays = {"items": np.array(list(items))}
    first = next(iter(items.values()))
    for j, (item, d) in enumerate(items.items()):
        for k, v in d.items():
            same = j > 0 and k in first and np.asarray(v).dtype == np.asarray(first[k]).dtype and np.array_equal(v, first[k])
            if not same:
                arrays[f"{item}__{k}"] = v
    _save(OUT / f"{name}.npz", arrays)


def _case(ref, name, items, movable):
    for attempt in range(6):
        recs, bad = _records(ref, items)
        if bad == 0:
            break
        if not movable:
            raise RuntimeError(f"{name}: {bad} decisions are not settled in a dyadic case")
        for inp in items.values():  # move every view's principal point by a hundredth of a pixel
            c = inp["cams_src"].copy()
            c[:, 2 + 2] += F32(0.01)
            c[:, 2 + 6] += F32(0.01)
            inp["cams_src"] = c
    else:
        raise RuntimeError(f"{name}: no admissible inputs after {attempt + 1} attempts ({bad} unsettled decisions)")
    _write_case(f"gnt_edges_{name}", recs)
    return recs


# ---------------------------------------------------------------- scenes
def _dyadic_cam(h, w, f, cx, cy, t):
    c2w = np.eye(4)
    c2w[:3, 3] = t
    return _flat_cam(h, w, f, c2w, cx=cx, cy=cy)


H0, W0 = 17, 33


def _dyadic_rig():
    cams = np.stack([_dyadic_cam(H0, W0, 16.0, 0.0, 0.0, [0, 0, 0]),
                     _dyadic_cam(H0, W0, 16.0, 16.0, 8.0, [4.0, -2.0, 0.0]),
                     _dyadic_cam(H0, W0, 32.0, 16.0, 8.0, [-8.0, 4.0, -1.0])])
    return cams, _dyadic_cam(H0, W0, 16.0, 16.0, 8.0, [0, 0, 0])


def _dyadic_inputs(rng, X, zs, C=32, hf=9, wf=17, masks=None):
    """rays from the target's centre (the origin, which is view 0's centre too) through the points X[R,3], sampled at
    the depths zs (powers of two; 1 = the point itself): every sample z * X is exact in float32, and all samples of
    a ray share their pixel of view 0"""
    cams, cam_tgt = _dyadic_rig()
    d = np.asarray(X, F64).astype(F32)
    assert np.array_equal(d.astype(F64), np.asarray(X, F64))
    if masks is None:
        masks = (rng.random((3, H0, W0, 1)) < 0.3).astype(F32)
    return dict(ray_o=np.zeros((len(d), 3), F32), ray_d=d, z_in=np.tile(np.asarray(zs, F32), (len(d), 1)),
                cam_tgt=cam_tgt, cams_src=cams, src_rgbs=rng.random((3, H0, W0, 3), dtype=F32),
                featmaps=rng.normal(size=(3, C, hf, wf)).astype(F32), inv_masks=masks, V=np.int64(3), C=np.int64(C),
                use_mask=np.int64(1), route=np.array("z_in"), depth_range=np.array([[0.5, 5.0]], F32))


def case_bounds(ref):
    rng = np.random.default_rng(1101)
    up, dn = lambda x: np.nextafter(F32(x), F32(np.inf)), lambda x: np.nextafter(F32(x), F32(-np.inf))  # noqa: E731
    sub, nrm = np.nextafter(F32(0), F32(1)), F32(2.0 ** -126)
    us = [F32(0), -sub, -nrm, F32(-2.0 ** -23), sub, F32(W0 - 1), up(W0 - 1), dn(W0 - 1), F32(W0 - 2), F32(16), F32(0.5), F32(W0 - 1.5)]
    vs = [F32(0), -sub, F32(-2.0 ** -23), sub, F32(H0 - 1), up(H0 - 1), dn(H0 - 1), F32(H0 - 2), F32(8), F32(0.5), F32(H0 - 1.5)]
    X = [(F64(u), F64(v), 16.0) for u in us for v in vs]
    inp = _dyadic_inputs(rng, X, [1.0, 2.0])
    recs = _case(ref, "bounds", {"mask1": inp, "mask0": dict(inp, use_mask=np.int64(0))}, movable=False)
    r = recs["mask1"]
    u, v = r["m_pix64"][0, :, 0, 0], r["m_pix64"][0, :, 0, 1]  # view 0, the sample at the point
    assert np.array_equal(u, np.repeat(np.array(us, F64), len(vs))) and np.array_equal(v, np.tile(np.array(vs, F64), len(us)))
    assert r["m_same"][0, :, :, :3].all()
    mi = r["out_mask_inbound"][:, 0, 0, 0]
    assert np.array_equal(mi > 0, (u >= 0) & (u <= W0 - 1) & (v >= 0) & (v <= H0 - 1)) and 20 < mi.sum() < mi.size - 20
    return recs


def case_depth(ref):
    rng = np.random.default_rng(1202)
    zs = [0.0, 2.0 ** -26, 2.0 ** -27, 2.0 ** -30, 2.0 ** -149, -2.0 ** -26, -2.0 ** -27, -2.0 ** -30, -2.0 ** -149, -1.0, -0.25, 0.125]
    xy = [(0.0, 0.0), (2.0 ** -30, 2.0 ** -31), (2.0 ** -27, 0.0), (1.0, 0.5), (-1.0, 0.25), (2.0 ** -24, -2.0 ** -24), (0.0, 2.0 ** -29)]
    X = [(x, y, z) for z in zs for x, y in xy]
    # rays through the centres of views 1 and 2, the last sample (z = 4) exactly on the centre (beyond a centre the two
    # directions of compute_angle are parallel and their difference is rounding noise: not an edge of the kernel)
    X += [(1.0, -0.5, 0.0), (-2.0, 1.0, -0.25)]
    X += [(0.0, 0.0, 2.0 ** -25), (16.0, 8.0, 16.0), (3.0, 2.0, 4.0), (-1.0, 0.5, 1.0)]
    inp = _dyadic_inputs(rng, X, [1.0, 2.0, 4.0])
    recs = _case(ref, "depth", {"mask1": inp}, movable=False)
    r = recs["mask1"]
    pz0 = r["m_pz64"][0, :, 0]
    assert r["m_same"][0, :, 0, 2].all() and np.array_equal(pz0[:len(zs) * len(xy)], np.repeat(np.array(zs, F64), len(xy)))
    assert np.sum(np.abs(r["m_pix64"]) == 1e6) > 20, "the +-1e6 clamp is not reached"
    n = len(zs) * len(xy)
    assert r["m_pz64"][1, n, 2] == 0 and np.all(r["m_pix64"][1, n, 2] == 0) and r["m_pz64"][2, n + 1, 2] == 0  # on a centre
    inb0 = r["out_mask_inbound"][:, 0, 0, 0]
    assert inb0[:len(zs) * len(xy)].sum() >= 4  # tiny positive z with tiny x, y: inside the image
    return recs


def case_mask(ref):
    rng = np.random.default_rng(1303)
    m = np.zeros((3, H0, W0, 1), F32)
    m[0, 5, 7] = m[0, 0, 0] = m[0, H0 - 1, W0 - 1] = m[0, 11, 3] = 1.0  # isolated pixels, two of them in corners
    m[0, :, 20:28] = 1.0  # a band: columns 20..27
    # pixels whose value is the float32 threshold itself and its two neighbours: on their centres the sampled value is
    # exactly float32(1e-3), which is not above it (in float64 the same value lies above the double 1e-3: these items'
    # decision is the float32 run's, see _records)
    m[0, 13, 15], m[0, 13, 11], m[0, 13, 13] = F32(1e-3), np.nextafter(F32(1e-3), F32(1)), np.nextafter(F32(1e-3), F32(0))
    m[1, 9:, :] = 1.0  # half-planes in the other views
    m[2, :, :12] = 1.0
    e10, e9 = 2.0 ** -10, 2.0 ** -9
    pts = []
    for x0, y0 in ((7, 5), (3, 11)):  # around an isolated pixel: value = (1 - |du|) (1 - |dv|)
        for du in (0.0, 1 - e10, 1 - e9, -(1 - e10), -(1 - e9), 1.0, 0.5, 1 - 2.0 ** -11):
            for dv in (0.0, 1 - e10, -(1 - e9), 0.5):
                pts.append((x0 + du, y0 + dv))
    for u in (19.0, 19 + e10, 19 + e9, 19 + 2.0 ** -11, 20.0, 23.5, 27.0, 27 + (1 - e10), 27 + (1 - e9), 28.0, 28.5):  # the band's edges
        for v in (0.0, 4.25, 16.0):
            pts.append((u, v))
    pts += [(15.0, 13.0), (11.0, 13.0), (13.0, 13.0)]
    pts += [(0.0, 0.0), (1 - e10, 0.0), (0.0, 1 - e9), (1 - e9, 1 - e9), (32.0, 16.0), (31 + e10, 16.0), (31 + e9, 16.0), (32.0, 15 + e10)]
    X = [(u, v, 16.0) for u, v in pts]
    inp = _dyadic_inputs(rng, X, [1.0, 2.0], masks=m)
    recs = _case(ref, "mask", {"mask1": inp, "mask0": dict(inp, use_mask=np.int64(0))}, movable=False)
    r = recs["mask1"]
    mv = r["m_mval64"][0, :, 0]
    assert r["m_same"][0, :, 0, 3].all()
    for val, n in ((0.0, 5), (e10, 8), (e9, 8), (1.0, 8)):
        assert np.sum(mv == val) >= n, (val, np.sum(mv == val))
    assert np.array_equal(r["out_mask_invalid"][:, 0, 0, 0] > 0, mv > float(F32(1e-3)))
    on = mv == float(F32(1e-3))
    assert on.sum() == 1 and not r["out_mask_invalid"][:, 0, 0, 0][on].any()
    return recs


def _rays(rng, cam_tgt, n, H, W):
    """n rays of the target camera through random (fractional) pixels, direction with z_cam = 1"""
    K = cam_tgt[2:18].reshape(4, 4).astype(F64)
    c2w = cam_tgt[18:34].reshape(4, 4).astype(F64)
    uv = rng.random((n, 2)) * [W - 1, H - 1]
    d_cam = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(n)], -1)
    return np.tile(c2w[:3, 3], (n, 1)).astype(F32), (d_cam @ c2w[:3, :3].T).astype(F32)


def case_angle(ref):
    rng = np.random.default_rng(1404)
    H, W, V, C = 19, 27, 4, 32
    f = 0.9 * W
    tgt_pose = _pose(0.5, -0.4, [0.03, -0.02, 0.0])
    cam_tgt = _flat_cam(H, W, f, tgt_pose)
    rot = _pose(4.0, 2.5, [0, 0, 0])
    rot[:3, 3] = tgt_pose[:3, 3]  # the same centre, another orientation
    cams = np.stack([cam_tgt.copy(), _flat_cam(H, W, f * 1.05, rot, cx=W / 2 + 0.4),
                     _flat_cam(H, W, f, _pose(-6.0, 2.0, [0.7, 0.1, 0.05])), _flat_cam(H, W, f * 0.95, _pose(5.0, -3.0, [-0.6, -0.2, 0.1]))])
    assert np.array_equal(cams[0], cam_tgt) and np.array_equal(cams[1][[21, 25, 29]], cam_tgt[[21, 25, 29]])
    ro, rd = _rays(rng, cam_tgt, 40, H, W)
    inp = dict(ray_o=ro, ray_d=rd, depth_range=np.array([[0.8, 4.0]], F32), S=np.int64(4), inv_uniform=np.int64(1), cam_tgt=cam_tgt,
               cams_src=cams, src_rgbs=rng.random((V, H, W, 3), dtype=F32), featmaps=rng.normal(size=(V, C, 5, 7)).astype(F32),
               inv_masks=(rng.random((V, H, W, 1)) < 0.25).astype(F32), V=np.int64(V), C=np.int64(C), use_mask=np.int64(1),
               route=np.array("range"))
    recs = _case(ref, "angle", {"mask1": inp}, movable=True)
    rdiff = recs["mask1"]["out_ray_diff"]
    assert np.all(rdiff[:, :, :2, :3] == 0) and np.all(np.abs(rdiff[:, :, :2, 3] - 1) < 1e-5) and np.all(np.abs(rdiff[:, :, 2:, :3]).max(-1) > 0.1)
    return recs


def case_sizes(ref):
    rng = np.random.default_rng(1505)
    H, W, V, C, R = 17, 23, 7, 68, 13
    h, w = 2 * H, 2 * W
    f = 0.9 * w
    hw = [(h, w), (30, 50), (40, 40), (h, w), (36, 44), (34, 48), (28, 60)]
    cams = np.stack([_flat_cam(hw[i][0], hw[i][1], f * (1 + 0.03 * i), _pose(4.0 * i - 10, 1.5 * i - 4, [0.25 * i - 0.7, 0.05 * i - 0.1, 0.02 * i]),
                               cx=w / 2 + 0.3 * i, cy=h / 2 - 0.2 * i) for i in range(V)])
    cam_tgt = _flat_cam(h, w, f, _pose(0.5, -0.4, [0.03, -0.02, 0.0]))
    ro, rd = _rays(rng, cam_tgt, R, h, w)
    near = (0.3 * 10 ** (rng.random(R) * 1.2)).astype(F32)
    per_ray = np.stack([near, near * (1.5 + 3 * rng.random(R)).astype(F32)], 1).astype(F32)
    base = dict(ray_o=ro, ray_d=rd, cam_tgt=cam_tgt, cams_src=cams, src_rgbs=rng.random((V, H, W, 3), dtype=F32),
                featmaps=rng.normal(size=(V, C, 7, 11)).astype(F32), inv_masks=(rng.random((V, H, W, 1)) < 0.25).astype(F32),
                use_mask=np.int64(1), route=np.array("range"))
    one = np.array([[0.8, 4.0]], F32)
    # the fine record: depths from the reference's own importance re-sampling of a coarse pass with per-ray ranges
    T = torch.from_numpy
    w_c = rng.random((R, 5)).astype(F32)
    w_c[3] = 0
    w_c[5] = [0, 0, 1, 0, 0]
    _, z_c = ref.sample_along_camera_ray(T(ro), T(rd), T(per_ray), 5, inv_uniform=False, det=True)
    _, z_f = ref.sample_fine_pts(False, 4, True, 5, {"ray_o": T(ro), "ray_d": T(rd)}, T(w_c.copy()), z_c)
    items = {
        "c32_v3_perray_uniform": dict(base, V=np.int64(3), C=np.int64(32), depth_range=per_ray, S=np.int64(5), inv_uniform=np.int64(0)),
        "c64_v7_perview_inverse": dict(base, V=np.int64(7), C=np.int64(64), depth_range=one, S=np.int64(3), inv_uniform=np.int64(1)),
        # (the fine pass hands the kernel its depths together with the rays' own ranges)
        "c30_v1_fine": dict(base, V=np.int64(1), C=np.int64(30), z_in=z_f.numpy(), route=np.array("z_in"), depth_range=per_ray),
        "c68_v3_perray_inverse": dict(base, V=np.int64(3), C=np.int64(68), depth_range=per_ray, S=np.int64(5), inv_uniform=np.int64(1)),
        "c32_v3_perview_uniform_nomask": dict(base, V=np.int64(3), C=np.int64(32), depth_range=one, S=np.int64(5), inv_uniform=np.int64(0),
                                              use_mask=np.int64(0)),
    }
    recs = _case(ref, "sizes", items, movable=True)
    for k, r in recs.items():
        assert (r["out_mask"].size % 8) != 0, k
    return recs


def case_sampling(ref):
    rng = np.random.default_rng(1606)
    T = torch.from_numpy
    R = 24
    ro = (rng.normal(size=(R, 3)) * 0.1).astype(F32)
    rd = (rng.normal(size=(R, 3)) * 0.3 + [0, 0, 1]).astype(F32)
    near = (0.05 * 10 ** (rng.random(R) * 2)).astype(F32)
    far = (near * (1.5 + 4 * rng.random(R))).astype(F32)
    far[::5] = near[::5] * F32(1.001)  # far barely above near
    ranges = {"perview": np.array([[0.8, 4.0]], F32), "perray": np.stack([near, far], 1)}
    out = {"ray_o": ro, "ray_d": rd, "range_perview": ranges["perview"], "range_perray": ranges["perray"]}
    names = []

    def conditioned(name, a, b, key):
        err = np.abs(a.astype(F64) - b)
        assert np.all(err <= 0.5 * (1e-6 + 1e-6 * np.abs(b))), (name, key, err.max())
        return err.max()

    for rk, dr in ranges.items():
        drr = dr if dr.shape[0] == R else np.tile(dr, (R, 1))
        for iu in (0, 1):
            for S in (2, 3, 64):
                name = f"coarse_{rk}_iu{iu}_s{S}"
                p32, z32 = ref.sample_along_camera_ray(T(ro), T(rd), T(drr), S, inv_uniform=bool(iu), det=True)
                p64, z64 = ref.sample_along_camera_ray(T(ro).double(), T(rd).double(), T(drr).double(), S, inv_uniform=bool(iu), det=True)
                out.update({name + "__pts": p32.numpy(), name + "__z_vals": z32.numpy(), name + "__pts64": p64.numpy(), name + "__z_vals64": z64.numpy(),
                            name + "__err_z_vals": F64(conditioned(name, z32.numpy(), z64.numpy(), "z")),
                            name + "__err_pts": F64(conditioned(name, p32.numpy(), p64.numpy(), "pts"))})
                names.append(name)
    # importance re-sampling: weights with all-zero, one-hot and single-dominant-bin rows.  One set of weights per value of
    # inv_uniform: a one-hot row's hot bin is the last one of the CDF (after the flip of the inverse branch), see below
    S, N = 12, 6
    ws = {}
    for iu in (0, 1):
        w = rng.random((R, S)).astype(F32)
        w[0:3] = 0
        for r, mag in ((3, 1.0), (4, 0.5), (5, 3.0)):
            w[r] = 0
            w[r, 1 if iu else S - 2] = mag
        for r, j in ((8, 2), (9, 6), (10, 9)):
            w[r] *= F32(0.1)
            w[r, j] = 0.9
        ws[iu] = w

    def fine(rk, iu, wts):
        dr = ranges[rk]
        drr = dr if dr.shape[0] == R else np.tile(dr, (R, 1))
        _, zc = ref.sample_along_camera_ray(T(ro), T(rd), T(drr), S, inv_uniform=bool(iu), det=True)
        p32, za32 = ref.sample_fine_pts(bool(iu), N, True, S, {"ray_o": T(ro), "ray_d": T(rd)}, T(wts.copy()), zc)
        _, za64 = ref.sample_fine_pts(bool(iu), N, True, S, {"ray_o": T(ro).double(), "ray_d": T(rd).double()},
                                      T(wts.copy()).double(), zc.double())  # the same coarse depths cast up
        return zc.numpy(), p32.numpy(), za32.numpy(), za64.numpy()

    # Conditioning.  With det=True the last draw is u = 1, the end of the CDF.  Where a row's last bins hold only the
    # 1e-5 floor, whether a float32 cumsum reaches 1 one knot early decides the bin, and the denom < 1e-5 branch makes
    # the sample jump to that bin's edge: the reference's own float32 and float64 runs then differ by a bin width.  So
    # a one-hot row has its hot bin last; its empty bins still drive the denom < 1e-5 branch at u = 0.
    # The same holds where a bin's share of the CDF is close to 1e-5 itself.  Such a row is ill-conditioned in the
    # reference's arithmetic (another float32 summation order moves the sample by a bin): rows whose float32 and float64
    # results differ, or that move under a perturbation of the weights by a few ulps, are replaced by random rows.
    special = np.array([0, 1, 2, 3, 4, 5, 8, 9, 10])
    combos = [(rk, iu) for rk in ("perview", "perray") for iu in (0, 1)]
    replaced = np.zeros(R, bool)
    jitter = rng.random((R, S))
    for _ in range(6):
        ok = np.ones(R, bool)
        for rk, iu in combos:
            w = ws[iu]
            _, _, za32, za64 = fine(rk, iu, w)
            ok &= np.all(np.abs(za32.astype(F64) - za64) <= 0.4e-6 * (1 + np.abs(za64)), 1)
            for sgn in (1.0, -1.0):  # and under a relative perturbation of the weights of a few float32 ulps
                wp = (w.astype(F64) * (1.0 + sgn * 2.0 ** -20 * jitter)).astype(F32)
                zp = fine(rk, iu, wp)[2]
                ok &= np.all(np.abs(zp.astype(F64) - za64) <= 2e-6 * (1 + np.abs(za64)), 1)
        if ok.all():
            break
        for iu in (0, 1):
            ws[iu][~ok] = rng.random((int((~ok).sum()), S)).astype(F32)
        replaced |= ~ok
    kept = special[~replaced[special]]
    assert np.all(np.isin(np.arange(6), kept)) and len(kept) >= 8, kept  # (nearly) every constructed row is well-conditioned
    out["fine_weights_iu0"], out["fine_weights_iu1"], out["fine_special_rows"] = ws[0], ws[1], kept
    for rk, iu in combos:
        name = f"fine_{rk}_iu{iu}"
        zc, p32, za32, za64 = fine(rk, iu, ws[iu])
        conditioned(name, za32, za64, "z_all")
        # sorting is 1-Lipschitz in the maximum norm, so depths that swap order between the two precisions are closer
        # than the bound just asserted: the union taken in the float32 run's order is ascending in float64 up to it
        out.update({name + "__z_coarse": zc, name + "__z_all": za32, name + "__z_all64": za64, name + "__pts": p32,
                    name + "__inv_uniform": np.int64(iu), name + "__n_fine": np.int64(N), name + "__range": np.array(rk)})
        names.append(name)
    print("  sampling: special weight rows kept", kept.tolist())
    out["items"] = np.array(names)
    _save(OUT / "gnt_edges_sampling.npz", out)


def case_render(ref):
    import copy

    from pgdvs.models.gnt.model import GNTModel
    from pgdvs.models.gnt.renderer import BaseRenderer
    import pgdvs.renderers.pgdvs_renderer_base as RB

    T = torch.from_numpy
    rng = np.random.default_rng(1707)
    B, H, W, V, Ss, stride = 2, 32, 48, 3, 12, 2
    torch.manual_seed(123)  # the network of make_golden_gnt.py, rebuilt
    model = GNTModel(netwidth=64, transformer_depth=2, coarse_feat_dim=32, fine_feat_dim=32, single_net=True,
                     posenc_max_freq_log2=9, pos_enc_n_freqs=10, view_enc_n_freqs=10).eval()
    with torch.no_grad():
        for n, p in model.net_coarse.named_parameters():
            if p.ndim == 1:
                p.add_(torch.randn_like(p) * 0.1)
    small = np.load(OUT / "gnt_small.npz")
    sd = model.net_coarse.state_dict()
    assert {"w_" + k for k in sd} == {k for k in small.files if k.startswith("w_")}
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), small["w_" + k]), k
    f = 0.9 * W
    cams_src = np.stack([np.stack([_flat_cam(H, W, f * (1 + 0.03 * i), _pose(3.0 * i - 3 + b, 1.0 * i - 0.5 * b, [0.15 * i - 0.15, 0.02 * i + 0.05 * b, 0.01 * i]),
                                             cx=W / 2 + 0.3 * i) for i in range(V)]) for b in range(B)])
    cam_tgt = np.stack([_flat_cam(H, W, f, _pose(0.5, -0.4, [0.03, -0.02, 0.0])), _flat_cam(H, W, f * 1.02, _pose(-0.8, 0.6, [-0.05, 0.04, 0.02]))])
    src_rgbs = rng.random((B, V, H, W, 3), dtype=F32)
    inv_masks = (rng.random((B, V, H, W, 1)) < 0.25).astype(F32)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    near = np.stack([0.6 + 0.3 * np.sin(xx / W * 3 + b) + 0.1 * yy / H for b in range(B)]).astype(F32)
    range_map = np.stack([near, near * (3.0 + np.cos(yy / H * 2)[None] + 0.5 * rng.random((B, H, W)))], -1).astype(F32)  # [B,H,W,2]
    per_ray = np.ascontiguousarray(range_map[:, ::stride, ::stride].reshape(-1, 2))
    base = RB.PGDVSBaseRenderer()
    ro, rd, uvs, brefs, shape = base.get_batched_rays(device="cpu", batch_size=B, H=H, W=W, render_stride=stride,
                                                      intrinsics=T(cam_tgt[:, 2:18].reshape(B, 4, 4)), c2w=T(cam_tgt[:, 18:34].reshape(B, 4, 4)))
    assert ro.shape[0] == per_ray.shape[0] == B * shape[0] * shape[1]
    out = dict(B=B, H=H, W=W, V=V, Ss=Ss, render_stride=stride, cams_src=cams_src, cam_tgt=cam_tgt, src_rgbs=src_rgbs, inv_masks=inv_masks,
               depth_range_map=range_map, ray_o=ro.numpy(), ray_d=rd.numpy())
    runs = {}
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(model).to(dt)
        br = BaseRenderer.__new__(BaseRenderer)
        torch.nn.Module.__init__(br)
        br.projector, br.model = ref.proj, m
        c = lambda a: T(np.ascontiguousarray(a)).to(dt)  # noqa: E731
        ray_batch = {"ray_o": ro.to(dt), "ray_d": rd.to(dt), "camera": c(cam_tgt), "rgb": None, "batch_refs": brefs, "view_uv": uvs, "raw_h": H,
                     "raw_w": W, "render_h": shape[0], "render_w": shape[1], "depth_range": c(per_ray), "depth_range_per_ray": True,
                     "src_rgbs": c(src_rgbs), "src_invalid_masks": c(inv_masks), "src_cameras": c(cams_src)}
        with torch.no_grad():
            if dt == torch.float32:
                fc, ff = m.feature_net(c(src_rgbs).permute(0, 1, 4, 2, 3).reshape(B * V, 3, H, W))
                out["featmaps"] = fc.numpy().reshape((B, V) + tuple(fc.shape[1:]))
                assert torch.equal(fc, ff)  # single_net: one feature map for both passes
            for tag, iu, nf, chunk in (("uni", False, 6, 100), ("inv", True, 0, 37)):
                assert (shape[0] * shape[1]) % chunk != 0
                runs[tag, dt] = br.forward(ray_batch=ray_batch, chunk_size=chunk, inv_uniform=iu, n_coarse_samples_per_ray=Ss,
                                           n_fine_samples_per_ray=nf, use_dyn_mask=True, flag_deterministic=True, render_stride=stride,
                                           ret_view_entropy=True, ret_view_std=True, disable_tqdm=True)
                out.update({f"{tag}__inv_uniform": np.int64(iu), f"{tag}__n_fine": np.int64(nf), f"{tag}__chunk_size": np.int64(chunk)})
    worst = {}
    for tag in ("uni", "inv"):
        for grp, atol in (("outputs_coarse", 2e-4), ("outputs_fine", 3e-4)):
            a, b = runs[tag, torch.float32][grp], runs[tag, torch.float64][grp]
            if a is None:
                continue
            for k in a:
                err = float((a[k].double() - b[k]).abs().max())
                worst[grp] = max(worst.get(grp, 0.0), err)
                if err > 0.5 * atol:  # conditioning rule, at the tolerances of test_gnt_renderer_end_to_end_vs_reference
                    raise RuntimeError(f"render {tag} {grp} {k}: the reference's own float32 error {err:.2e} exceeds half the tolerance")
                pre = "out_" if grp == "outputs_coarse" else "fine_"
                out[f"{tag}__{pre}{k}"] = a[k].numpy()
                out[f"{tag}__{pre}{k}_64"] = b[k].numpy().astype(F32)  # the float64 result, rounded once
    out["err_coarse"], out["err_fine"] = F64(worst["outputs_coarse"]), F64(worst["outputs_fine"])
    _save(OUT / "gnt_edges_render.npz", out)
    print(f"  render: reference float32 vs float64, coarse {worst['outputs_coarse']:.1e} fine {worst['outputs_fine']:.1e}")


def main():
    torch.set_num_threads(1)
    _install_stubs()
    ref = Ref()
    stats = {}
    for case in (case_bounds, case_depth, case_angle, case_mask, case_sizes):
        recs = case(ref)
        r0 = next(iter(recs.values()))
        stats[case.__name__[5:]] = (sum(int(r["n_items"]) for r in recs.values()), sum(int(r["n_border"]) for r in recs.values()),
                                    float(r0["diff_pix"]), float(r0["diff_pz"]), float(r0["diff_mval"]))
    case_sampling(ref)
    case_render(ref)
    for f in sorted(OUT.glob("gnt_edges_*.npz")):
        s = stats.get(f.stem[len("gnt_edges_"):])
        extra = "" if s is None else f"  items {s[0]:5d}  border {s[1]:5d}  diff pix {s[2]:.1e} pz {s[3]:.1e} mval {s[4]:.1e}"
        print(f"  {f.name:22s} {f.stat().st_size / 1024:6.1f} KiB{extra}")
    print(f"  margin {MARGIN:g} everywhere.")


if __name__ == "__main__":
    main()
