"""GPU (MI355X): the splat kernels of csrc/softsplat.hip over tests/splat_cases.py -- pgdvs_dyn_splat_composite and its _rng
twin through the C ABI with a workspace the test owns and fills with 0xFF (every accumulator a NaN, every flag byte set:
accumulators of unflagged pixels must never be read, the flags must be rebuilt by the call) and outputs between guard
regions; pgdvs_softsplat_fwd in every mode and pgdvs_softsplat_bwd through their wrappers.  Each result is compared with
the float64 restatement under the bound derived in splat_cases.py; the mask is equal, not close, outside the few pixels
within their own bound of the 1e-3 threshold.  Every test prints its worst err / bound (``pytest -s``)."""
import types

import numpy as np
import pytest
import torch

import splat_cases as S

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402  (checker only)
from pgdvs_amd import ops  # noqa: E402
from pgdvs_amd.utils.softsplat import softsplat  # noqa: E402

DEV = "cuda:0"
GUARD = 64          # floats on either side of every output
SENTINEL = -777.25
F64 = np.float64
IMAGES = (("dyn_rgb", 3), ("dyn_mask", 1), ("comb", 3), ("comb_st", 3), ("comb_dy", 3))


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cases are read-only)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()  # fails loudly if the HIP extension is missing


def _composite(c, noise="case", rng_state=None, static=True, null=()):
    """one call through the C ABI.  -> the five images as numpy (None where the pointer was NULL or must stay untouched:
    then the buffer is checked to hold the sentinel), the flag bytes the call left in the workspace"""
    from pgdvs_amd import _lib

    lib = _lib.load()
    H, W = c.H, c.W
    P = H * W
    t = {k: T(getattr(c, k)) for k in ("rgb1", "rgb2", "flow12", "f1t", "mask", "static")}
    nz = T(c.noise) if isinstance(noise, str) else noise
    nbytes = int(lib.pgdvs_dyn_splat_workspace_bytes(H, W))
    assert nbytes >= 5 * 4 * P + P
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    bufs = {k: torch.full((GUARD + ch * P + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for k, ch in IMAGES}
    ptr = {k: (None if k in null else bufs[k][GUARD:GUARD + ch * P]) for k, ch in IMAGES}
    head = (H, W, ops._ptr(t["rgb1"]), ops._ptr(t["rgb2"]), ops._ptr(t["flow12"]), ops._ptr(t["f1t"]), ops._ptr(t["mask"]))
    tail = (float(c.alpha), ops._ptr(t["static"] if static else None), ops._ptr(ptr["dyn_rgb"]), ops._ptr(ptr["dyn_mask"]),
            ops._ptr(ptr["comb"]), ops._ptr(ptr["comb_st"]), ops._ptr(ptr["comb_dy"]), ops._ptr(ws), nbytes, ops._stream())
    if rng_state is None:
        rc = lib.pgdvs_dyn_splat_composite(*head, ops._ptr(nz), *tail)
    else:
        rc = lib.pgdvs_dyn_splat_composite_rng(*head, ops._ptr(rng_state), *tail)
    assert rc == 0, lib.pgdvs_last_error()
    torch.cuda.synchronize()
    out = {}
    for k, ch in IMAGES:
        b = N(bufs[k])
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), f"{k}: guard overwritten"
        body = b[GUARD:-GUARD]
        if k in null or (not static and k.startswith("comb")):
            assert (body == SENTINEL).all(), f"{k}: written although it must stay untouched"
            out[k] = None
        else:
            assert np.isfinite(body).all() and not (body == SENTINEL).any(), f"{k}: not finite / not written everywhere"
            out[k] = body.reshape((ch, H, W) if ch == 3 else (H, W))
    flags = N(ws)[5 * 4 * P:5 * 4 * P + P].reshape(H, W)
    return types.SimpleNamespace(**out), flags


def _ratio(got, c, ref, scale=1.0):
    """S.composite_ratio over the images that are there"""
    full = types.SimpleNamespace(**{k: (getattr(ref, k) if getattr(got, k) is None else getattr(got, k)) for k, _ in IMAGES})
    return S.composite_ratio(full, c, ref, scale)


# ---------------------------------------------------------------- composite
@pytest.mark.parametrize("name", list(S.composite_cases()))
def test_composite_vs_float64(name):
    c, ref = S.composite_cases()[name], S.composite_ref(name)
    got, flags = _composite(c)
    assert np.array_equal(flags != 0, ref.live) and set(np.unique(flags)) <= {0, 1}  # rebuilt from all-ones
    ratio, unsure = _ratio(got, c, ref)
    print(f"\nSPLAT composite {name}: worst err/bound {ratio:.3f}, unsure {unsure}, live {int(ref.live.sum())}")
    assert ratio <= 1.0, ratio
    if name.startswith("empty"):
        assert not got.dyn_mask.any() and not got.dyn_rgb.any() and not got.comb_dy.any()
        assert got.comb.tobytes() == c.static.tobytes() and got.comb_st.tobytes() == c.static.tobytes()
    if name.startswith("full"):
        want = c.rgb1.transpose(2, 0, 1).astype(F64) / (1.0 + 1e-7)
        assert (np.abs(got.dyn_rgb - want) <= 2 * S.U * np.abs(want)).all() and (got.dyn_mask == 1).all()
    if name.startswith("collide"):  # the compare-and-swap add loses nothing under contention: a second run agrees
        again, _ = _composite(c)
        bound, unsure_px = S.composite_bound(c, ref)
        sure = ~unsure_px
        assert np.array_equal(again.dyn_mask[sure], got.dyn_mask[sure])
        r2 = S.worst_ratio(again.dyn_rgb, got.dyn_rgb, 2 * bound[:3] * ref.dyn_mask, sure[None])
        print(f"SPLAT composite {name}: second run vs first {r2:.3f} of twice the bound")
        assert r2 <= 1.0, r2
    if name.startswith("lone"):  # the dead pixels change no output
        mask = c.mask.copy()
        for y, x in c.claims["dead"]:
            mask[y, x] = 0.0
        other, oflags = _composite(types.SimpleNamespace(**{**vars(c), "mask": mask}))
        assert np.array_equal(oflags, flags) and _ratio(other, c, ref)[0] <= 1.0
        assert np.array_equal(other.dyn_mask, got.dyn_mask)


def test_composite_nullable_outputs():
    """static_rgb = NULL leaves the three combined buffers untouched, and so does each combined pointer that alone is NULL
    (_composite asserts the sentinel); what is written is still right"""
    c, ref = S.composite_cases()["border_37x53"], S.composite_ref("border_37x53")
    got, _ = _composite(c, static=False)
    assert got.comb is None and got.comb_st is None and got.comb_dy is None and _ratio(got, c, ref)[0] <= 1.0
    for k in ("comb", "comb_st", "comb_dy"):
        got, _ = _composite(c, null=(k,))
        assert getattr(got, k) is None and all(getattr(got, o) is not None for o, _ in IMAGES if o != k)
        assert _ratio(got, c, ref)[0] <= 1.0, k


@pytest.mark.parametrize("name", ["lone_33x33", "window_48x112", "empty_18x20"])
def test_composite_rng_entry_point(name):
    """the kernel's own noise: its images equal, within twice the bound, those of the injected-noise entry point fed
    ops.splat_noise_field of the same state, and the draw number advances by exactly 1 per call (also where every tile
    exits early)"""
    c = S.composite_cases()[name]
    seed = 20240607
    state = ops.splat_rng_state(DEV, seed=seed)
    field = ops.splat_noise_field(state, c.H, c.W)
    assert N(state).tolist() == [seed, 0]
    ref = S.composite(c, F64, noise=N(field))
    injected, _ = _composite(c, noise=field)
    r_inj, unsure = _ratio(injected, c, ref)
    drawn, _ = _composite(c, noise=None, rng_state=state)
    assert N(state).tolist() == [seed, 1]
    r_drawn, _ = _ratio(drawn, c, ref)
    bound, unsure_px = S.composite_bound(c, ref)
    sure = ~unsure_px
    assert np.array_equal(drawn.dyn_mask[sure], injected.dyn_mask[sure])
    r_pair = max(S.worst_ratio(getattr(drawn, k), getattr(injected, k), 2 * bound[:3] * ref.dyn_mask, sure[None])
                 for k in ("dyn_rgb", "comb", "comb_dy"))
    print(f"\nSPLAT rng {name}: injected {r_inj:.3f}, drawn {r_drawn:.3f}, drawn vs injected {r_pair:.3f} of twice the bound, "
          f"unsure {unsure}")
    assert r_inj <= 1.0 and r_drawn <= 1.0 and r_pair <= 1.0
    _composite(c, noise=None, rng_state=state)
    assert N(state).tolist() == [seed, 2]
    if name != "empty_18x20":
        assert not np.array_equal(N(ops.splat_noise_field(state, c.H, c.W)), N(field))  # the next draw is a fresh field


# ---------------------------------------------------------------- generic forward and backward
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", list(S.generic_cases()))
def test_forward_vs_float64(name, mode):
    g = S.generic_cases()[name]
    want, bound, nrm, n = S.forward_ref(name, mode)
    kind = mode.split("-")[0]
    metric = None if kind in ("sum", "avg") else (g.metric_lin if kind == "linear" else g.metric)
    flow = g.flow_q if kind == "linear" else g.flow
    with torch.no_grad():
        got = N(softsplat(T(g.x), T(flow), None if metric is None else T(metric), mode))
    ratio = S.worst_ratio(got, want, bound)
    print(f"\nSPLAT forward {name} {mode}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    if kind == "linear" and g.zero_t is not None:  # the exact-zero normaliser: addeps and clipeps divide by 1e-7, zeroeps by 1
        (ya, xa), (yb, xb), (yt, xt) = g.zero_src
        num = g.x[:, :, ya, xa].astype(F64) * 0.875 + g.x[:, :, yb, xb].astype(F64) * -0.875
        div = 1.0 if mode.endswith("zeroeps") else 1e-7
        assert (nrm[:, yt, xt] == 0).all() and (np.abs(got[:, :, yt, xt] - num / div) <= bound[:, :, yt, xt]).all()
    if mode == "sum":  # ... and the oracle, at the tolerances of tests/test_gpu_dyn_edges.py
        np.testing.assert_allclose(got, orc.softsplat(g.x, flow, None, "sum"), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("name", list(S.generic_cases()))
def test_backward_vs_oracle_and_float64(name):
    g = S.generic_cases()[name]
    gi, gf, bi, bf, _ = S.backward_ref(name)
    x, flow, og = T(g.x_fin), T(g.flow), T(g.og)
    di, df = ops.softsplat_bwd(x, flow, og)
    oi, of = orc.softsplat_bwd_raw(g.x_fin, g.flow, g.og)
    # the gather shares the oracle's operation order: bit for bit (a NaN in outgrad where no corner reads stays out)
    assert N(di).tobytes() == oi.tobytes() and N(df).tobytes() == of.tobytes()
    ri, rf = S.worst_ratio(N(di), gi, bi), S.worst_ratio(N(df), gf, bf)
    print(f"\nSPLAT backward {name}: worst err/bound ingrad {ri:.3f}, flowgrad {rf:.3f}")
    assert ri <= 1.0 and rf <= 1.0
    dead = ~np.isfinite(g.flow).all(1) | (np.abs(g.flow) >= 1e9).any(1)  # non-finite or far outside: zero gradients
    assert not N(di)[np.broadcast_to(dead[:, None], gi.shape)].any() and not N(df)[np.broadcast_to(dead[:, None], gf.shape)].any()
    assert np.isfinite(N(di)).all() and np.isfinite(N(df)).all()
    only_i, none_f = ops.softsplat_bwd(x, flow, og, True, False)
    none_i, only_f = ops.softsplat_bwd(x, flow, og, False, True)
    assert none_f is None and none_i is None
    assert N(only_i).tobytes() == N(di).tobytes() and N(only_f).tobytes() == N(df).tobytes()
