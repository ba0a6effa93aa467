"""GPU (MI355X): the fused GNT layer kernels (csrc/gnt_view.hip, csrc/gnt_embed.hip) against a float64 statement of the same
stage, past one round of their persistent grids and at the edges of their statistics.

Every layer kernel launches a capped grid and walks the remaining tiles in a grid-stride loop: the view layer 256 blocks x
8 waves x 16 groups (32 768 groups per round), the feed-forward block behind every view and ray layer 256 x 8 x 32 rows
(65 536), embed and posfc 512 x 4 x 16 (32 768), the ray attention 1024 rays.  The cases here are the smallest that reach
exactly one round, one row more, a partial tile in a later round, a third round, and -- for the bf16x3 feed-forward -- a
prefetch one grid ahead that points past N or onto a partial tile.  The stat cases (N = 703) give the view layer groups
with one valid view, with none (promoted), a dominant logit, identical views, and embed identical views, a mean 32 times
the spread and a single view (NaN statistics, like torch.std).

Yardstick: tests/gnt_layer_cases.py ref_* in float64 on the device (pinned against the .double() modules by
test_gnt_layers_host.py) and torch's own float32 statement of the stage -- the same call with ops._GNT_VIEW_ENABLED =
False.  For every output, over all elements, and again over the rows of the last grid round and of the last partial tile:

    max |kernel - ref64|  <=  4.0 * max |torch_fp32 - ref64| + 1e-5

the bound and floor of test_gpu_round5.py's float64 comparison.  The profiler's labels show that the fused kernel ran on
the kernel half and did not on the torch half.

Measured on an MI355X (worst case per stage and quantity: max|d| of the kernel, of torch fp32, and the kernel's error as a
fraction of the bound 4 x torch + 1e-5; "last round" / "last tile" rows never came out worse than "all" except where noted):

    stage                path        quantity   kernel    torch     of the bound
    view layer, rounds   bf16x3      x          1.5e-06   8.0e-07   0.12
                                     entropy    2.0e-07   2.2e-07   0.02
                                     std        1.4e-07   9.6e-08   0.01
                                     std_norm   2.4e-06   3.9e-06   0.15
                         fp32_mfma   x          1.4e-06   8.0e-07   0.10
                                     entropy    2.5e-07   2.2e-07   0.02
                                     std        1.1e-07   9.6e-08   0.01
                                     std_norm   1.1e-06   3.9e-06   0.08
    view layer, stats    bf16x3      x          4.2e-06   2.7e-06   0.28  (dominant logit, last tile: torch 1.3e-06 there)
                                     entropy    4.6e-07   2.6e-07   0.04  (dominant logit)
                                     std        1.8e-07   1.7e-07   0.02
                                     std_norm   2.5e-07   1.7e-07   0.02
                         fp32_mfma   x          4.4e-06   2.7e-06   0.29
                                     entropy    4.3e-07   2.6e-07   0.04
                                     std        2.0e-07   1.7e-07   0.02
                                     std_norm   2.0e-07   1.7e-07   0.02
      identical views    both        std        4.8e-17   1.6e-08   0.00  (the kernel's std is exactly 0)
    feed-forward         bf16x3      x          4.0e-06   4.0e-06   0.16
                         fp32_mfma   x          4.1e-06   4.0e-06   0.16
                         both        weights    1.8e-07   0         0.02  (one sample: the row is 1)
    ray layer            bf16x3      x          1.3e-06   9.2e-07   0.09
                         fp32_mfma   x          1.1e-06   9.2e-07   0.08
                         both        weights    8.9e-08   7.2e-08   0.01
    embed, rounds                    feat       1.1e-06   1.1e-06   0.08
                                     q0         9.9e-07   8.5e-07   0.07
                                     std        1.1e-07   1.0e-07   0.01
                                     std_norm   3.8e-06   3.3e-06   0.16
    embed, stats                     feat       8.2e-06   7.7e-06   0.20  (mean 32 x spread: values near 40)
                                     q0         7.4e-06   6.7e-06   0.20
                                     std        2.3e-07   2.8e-07   0.02
                                     std_norm   2.1e-07   2.8e-07   0.02
    posfc                            layer 0/2  5.5e-07   5.0e-07   0.05
    head                             rgb        5.6e-07   3.0e-07   0.05

Every quantity meets the bound with the one floor: none needed a floor of its own.  The view layer's std and std_norm
did not at first: the kernel formed the variance as sum k^2 - n mean^2, which left 6e-6 .. 1e-5 on the std of ordinary
inputs (0.6 .. 1.0 of the bound, against torch's 9e-8) and 8e-5 / 1.6e-4 on std / std_norm of identical views (8 and 16
times the bound).  It now keeps a running mean and the sum of squares about it (csrc/gnt_view.hip), which is what the
figures above show.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import gnt_layer_cases as C  # noqa: E402
from pgdvs_amd import ops  # noqa: E402
from pgdvs_amd.models.gnt.models.transformer_network import GNT  # noqa: E402

DEV = "cuda:0"
BOTH = (("bf16x3", False), ("fp32_mfma", True))
ONE = (("single", False),)  # embed, posfc and head have one product path: the option plays no part
FACTOR, FLOOR = 4.0, 1e-5  # test_gpu_round5.py: 4.0 * worst_t + 1e-5
VIEW_TILE, VIEW_ROUND = 16, 256 * 8 * 16
FF_TILE, FF_ROUND = 32, 256 * 8 * 32
EMB_TILE, EMB_ROUND = 16, 512 * 4 * 16
RAY_ROUND = 1024


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()  # fails loudly if the HIP extension is missing


class _Labels:
    """the kernel labels the library's profiler saw inside the block"""

    def __enter__(self):
        from pgdvs_amd import _lib

        self.lib = _lib.load()
        self.buf = ctypes.create_string_buffer(4096)
        self.lib.pgdvs_prof_report(self.buf, len(self.buf))  # clears earlier records
        self.lib.pgdvs_prof_enable(1)
        return self

    def __exit__(self, *exc):
        self.lib.pgdvs_prof_enable(0)
        self.lib.pgdvs_prof_report(self.buf, len(self.buf))
        self.seen = self.buf.value
        return False


def _err(a, ref, rows=None):
    """max |a - ref| over all elements (of the rows, given as (units, slice): the tensor as [units, -1]); the NaN pattern
    is compared by the caller, NaN == NaN counts as no error here"""
    a = a.double()
    if rows is not None:
        units, sl = rows
        a, ref = a.reshape(units, -1)[sl], ref.reshape(units, -1)[sl]
    d = (a - ref).abs()
    d = d[~torch.isnan(ref)]
    return float(d.max()) if d.numel() else 0.0


def _compare(case, run, ref, labels, paths=BOTH, rows=None):
    """run() -> {quantity: float32 tensor}, on the fused kernels as called and on torch with the kernels switched off;
    ref: {quantity: float64 tensor}; rows: {quantity: [(name, units, slice)]}.  Asserts the NaN pattern, finiteness and the
    bound on every quantity and row range; returns the table rows."""
    table = []
    with _Labels() as lab:
        ops._GNT_VIEW_ENABLED = False
        try:
            with torch.no_grad():
                out_t = run()
        finally:
            ops._GNT_VIEW_ENABLED = True
    assert not any(lb in lab.seen for lb in labels), (case, "the torch half ran a fused kernel", lab.seen)
    assert set(out_t) == set(ref), (case, sorted(out_t), sorted(ref))
    failures = []
    for path, fp32 in paths:
        with ops.gnt_product_path(fp32=fp32), _Labels() as lab, torch.no_grad():
            out_k = run()
        assert all(lb in lab.seen for lb in labels), (case, path, "the fused kernel did not run", lab.seen)
        assert set(out_k) == set(ref)
        for name, r in ref.items():
            k, t = out_k[name], out_t[name]
            assert k.dtype == torch.float32 and t.dtype == torch.float32 and r.dtype == torch.float64
            assert k.shape == r.shape == t.shape, (case, name, k.shape, r.shape)
            nan = torch.isnan(r)
            assert torch.equal(torch.isnan(k), nan), (case, path, name, "NaN pattern", int(torch.isnan(k).sum()), int(nan.sum()))
            assert bool(torch.isfinite(k[~nan]).all()) and bool(torch.isfinite(r[~nan]).all()), (case, path, name, "not finite")
            for rname, units, sl in [("all", None, None)] + list((rows or {}).get(name, [])):
                sel = None if units is None else (units, sl)
                ek, et = _err(k, r, sel), _err(t, r, sel)
                table.append((case, path, name, rname, ek, et))
                if not ek <= FACTOR * et + FLOOR:
                    failures.append((path, name, rname, ek, et))
    print(f"\n{case}: max|d| against float64 (kernel, torch fp32, ratio to the bound)")
    for _, path, name, rname, ek, et in table:
        print(f"  {path:9s} {name:9s} {rname:14s} {ek:.2e} {et:.2e} {ek / (FACTOR * et + FLOOR):.3f}")
    assert not failures, (case, failures)
    return table


def _unit_rows(n, tile, rnd, tag=""):
    return [(tag + name, n, sl) for name, sl in C.round_slices(n, tile, rnd).items()]


# ---------------------------------------------------------------- view layer
def _view_compare(case, net, layer, q, feat, rd, valid, cnt, want_stats):
    q, feat, rd, valid, cnt = (t.to(DEV) for t in (q, feat, rd, valid, cnt))
    n = q.shape[0] * q.shape[1]
    names = ("entropy", "std", "std_norm")

    def run():
        x, st = net._view_layer(layer, q, feat, rd, valid, cnt, want_stats)
        out = {"x": x.reshape(n, 64)}
        if want_stats:
            out.update({k: v.reshape(n) for k, v in zip(names, st)})
        else:
            assert st is None
        return out

    x64, st64 = C.ref_view_layer(C.weights64(layer), q, feat, rd, valid, want_stats)
    ref = {"x": x64.reshape(n, 64)}
    if want_stats:
        ref.update({k: v.reshape(n) for k, v in zip(names, st64)})
    view_rows = _unit_rows(n, VIEW_TILE, VIEW_ROUND, "view ")
    rows = {k: view_rows for k in names}
    rows["x"] = view_rows + _unit_rows(n, FF_TILE, FF_ROUND, "ff ")
    return _compare(case, run, ref, (b"gnt_view_layer", b"gnt_ff"), rows=rows), ref


@pytest.mark.parametrize("R,S,V,want_stats", [(128, 256, 2, True), (32769, 1, 2, True), (1725, 19, 3, True),
                                              (1725, 19, 3, False), (65569, 1, 1, True)])
def test_view_layer_grid_rounds(R, S, V, want_stats):
    """N = 32 768 (exactly one round: no block takes a second trip), 32 769 (round 2 = one tile with one live lane),
    32 775 (a partial tile in round 2, S > 1; also without the statistics), 65 569 (a third round of the view kernel, the
    feed-forward block's second round = one full and one 1-row tile; V = 1)."""
    n = R * S
    slices = C.round_slices(n, VIEW_TILE, VIEW_ROUND)
    assert ("last round" in slices) == (n > VIEW_ROUND) and ("last tile" in slices) == (n % 16 != 0)
    net = C.make_net(40 + V).to(DEV)
    q, feat, rd, valid, cnt = C.view_case(1000 + n, R, S, V)
    assert int(cnt.min()) >= 1
    _view_compare(f"view layer ({R}, {S}, V={V}{'' if want_stats else ', no stats'})", net, net.view_crosstrans[0], q, feat, rd,
                  valid, cnt, want_stats)


@pytest.mark.parametrize("edge", ["masks", "dominant_logit", "identical_views"])
def test_view_layer_stat_edges(edge):
    """R = 37, S = 19 (N = 703: 43 tiles of 16 groups and one of 15), V = 6.
    masks: groups 160..223 (four whole tiles) keep exactly one view, a different one from group to group in the first three
    tiles and view 2 throughout the fourth -- softmax over one entry, entropy 0, the output is that view's value path;
    groups 48..63 (a whole tile) and group 100 (alone in an ordinary tile) have no valid view and are promoted to all
    views, as GNT.forward promotes them.
    dominant_logit: attn_fc[2] scaled by 120, the largest logit of a group leads the second by more than 80: every other
    view's weight underflows, the entropy goes towards 0.
    identical_views: every view a copy of view 0: the std is 0 (float64: to rounding), the kernel's 0 or at rounding level,
    never NaN."""
    R, S, V = 37, 19, 6
    net = C.make_net(50).to(DEV)
    layer = net.view_crosstrans[0]
    q, feat, rd, valid, cnt = C.view_case(2000, R, S, V, p_valid=0.7 if edge == "dominant_logit" else 0.6)
    one = torch.zeros(R * S, dtype=torch.bool)
    only = torch.arange(R * S) % V  # the view a single-view group keeps ...
    only[208:224] = 2  # ... the same for a whole tile: the kernel skips the five views that no group of a tile sees
    if edge == "masks":
        v = valid.reshape(R * S, V).clone()
        one[160:224] = True
        v[160:224] = False
        v[torch.arange(160, 224), only[160:224]] = True
        v[48:64] = False
        v[100] = False
        valid, cnt = C.promote(v.reshape(R, S, V))
        c = cnt.reshape(-1)
        assert bool((c[160:224] == 1).all()) and bool((c[48:64] == V).all()) and int(c[100]) == V
        assert bool(valid.reshape(-1, V)[48:64].all()) and bool(valid.reshape(-1, V)[100].all())
    elif edge == "dominant_logit":
        feat = feat * 2.0
        with torch.no_grad():
            layer.attn.attn_fc[2].weight.mul_(120.0)
        lg = C.ref_view_logits(C.weights64(layer), q.to(DEV), feat.to(DEV), rd.to(DEV))
        top = torch.where(valid.to(DEV)[..., None], lg, torch.full_like(lg, -float("inf"))).topk(2, dim=2).values
        lead = top[:, :, 0] - top[:, :, 1]
        lead = lead[torch.isfinite(lead)]  # (groups with one valid view: no second logit)
        assert float(lead.max()) > 80.0 and float((lead > 80.0).double().mean()) > 0.01, (float(lead.max()),)
    else:
        feat = feat[:, :, :1].expand(R, S, V, 64).contiguous()
        rd = rd[:, :, :1].expand(R, S, V, 4).contiguous()
    table, ref = _view_compare(f"view layer stats, {edge}", net, layer, q, feat, rd, valid, cnt, True)
    if edge == "masks":
        # the yardstick itself has the property: one entry -> entropy -log(1 + 1e-8), output = that view's value path alone
        assert float(ref["entropy"][one.to(DEV)].abs().max()) <= 2e-8
        pick = only.reshape(R, S)[..., None, None]
        f1 = torch.gather(feat, 2, pick.expand(R, S, 1, 64)).to(DEV)
        d1 = torch.gather(rd, 2, pick.expand(R, S, 1, 4)).to(DEV)
        x1, _ = C.ref_view_layer(C.weights64(layer), q.to(DEV), f1, d1, torch.ones(R, S, 1, dtype=torch.bool, device=DEV), False)
        assert float((x1.reshape(-1, 64) - ref["x"])[one.to(DEV)].abs().max()) <= 1e-12
    if edge == "identical_views":
        assert float(ref["std"].abs().max()) <= 1e-12 and float(ref["std_norm"].abs().max()) <= 1e-9


# ---------------------------------------------------------------- feed-forward block and ray layer
def _ray_compare(case, layer, q):
    q = q.to(DEV)
    R, S = q.shape[:2]
    n = R * S

    def run():
        x, w = GNT._ray_layer(layer, q, True)
        return {"x": x, "weights": w}

    x64, w64 = C.ref_ray_layer(C.weights64(layer), q)
    ray_rows = [("ray last round", R, slice((R - 1) // RAY_ROUND * RAY_ROUND, R))] if R > RAY_ROUND else []
    rows = {"x": ray_rows + _unit_rows(n, FF_TILE, FF_ROUND, "ff "), "weights": ray_rows}
    return _compare(case, run, {"x": x64, "weights": w64}, (b"gnt_ray_attn", b"gnt_ff"), rows=rows)


@pytest.mark.parametrize("n", [65536, 65537, 65536 + 8 * 32 + 5, 2 * 65536 + 31])
def test_feed_forward_grid_rounds(n):
    """the feed-forward block through the ray layer (n rays of one sample: the attention is the identity on v) at
    n = 65 536 (one round exactly: every prefetch of the bf16x3 kernel points past N), 65 537 (round 2 = one row),
    65 536 + 8 x 32 + 5 (round 2 = one workgroup's eight full tiles and a 5-row tile in the next: its prefetch from round 1
    lands on the partial tile) and 2 x 65 536 + 31 (a third round of 31 rows); rows spanning 0.1 .. 10 in magnitude and the
    first layer scaled as in test_gnt_feed_forward_both_product_paths."""
    net = C.make_net(60).to(DEV)
    layer = net.view_selftrans[0]
    with torch.no_grad():
        layer.ff.fc1.weight.mul_(2.0)
    _ray_compare(f"feed-forward n={n}", layer, C.rows_case(3000 + n, n, 1, decades=True))


@pytest.mark.parametrize("R,S", [(1024, 3), (1025, 3), (2049, 5), (1025, 256)])
def test_ray_layer_grid_rounds(R, S):
    """one ray per workgroup, 1024 workgroups: R = 1024 (no wrap), 1025 and 2049 (one ray in the second / third trip);
    (1025, 256): the wrap with the LDS-filling S, and 262 400 feed-forward rows (five rounds) behind it."""
    net = C.make_net(61).to(DEV)
    _ray_compare(f"ray layer ({R}, {S})", net.view_selftrans[0], C.rows_case(4000 + R * S, R, S))


# ---------------------------------------------------------------- embed, posfc, head
def _embed_compare(case, net, x):
    x = x.to(DEV)
    R, S, V, cin = x.shape
    n = R * S

    def run():  # GNT.forward's dispatch
        if ops.gnt_embed_available(net.rgbfeat_fc, cin):
            feat, q0, st = ops.gnt_embed(net.rgbfeat_fc, x, True)
        else:
            feat, q0, st = C.stmt_embed(net, x)
        return {"feat": feat.reshape(n, V * 64), "q0": q0.reshape(n, 64), "std": st[0].reshape(n), "std_norm": st[1].reshape(n)}

    f64, q64, st64 = C.ref_embed(C.weights64(net.rgbfeat_fc), x)
    ref = {"feat": f64.reshape(n, V * 64), "q0": q64.reshape(n, 64), "std": st64[0].reshape(n), "std_norm": st64[1].reshape(n)}
    rows = {k: _unit_rows(n, EMB_TILE, EMB_ROUND) for k in ref}
    return _compare(case, run, ref, (b"gnt_embed",), paths=ONE, rows=rows), ref


@pytest.mark.parametrize("R,S,V", [(1725, 19, 3), (32769, 1, 2)])
def test_embed_grid_rounds(R, S, V):
    """N = 32 775 and 32 769: a partial tile in the second round; Cin = 35 is no multiple of 4 (last_ok)"""
    net = C.make_net(70).to(DEV)
    assert net.rgbfeat_fc[0].in_features == 35
    _embed_compare(f"embed ({R}, {S}, V={V})", net, C.embed_case(5000 + R, R, S, V))


@pytest.mark.parametrize("edge", ["identical_views", "spread", "single_view"])
def test_embed_stat_edges(edge):
    """R = 37, S = 19.  identical_views (V = 6): s2 - s1^2 / n must not go negative into a NaN (the kernel's fmaxf(var, 0));
    spread (V = 6): features whose mean is 32 times their view-to-view spread -- the kernel takes its moments about the
    first view's value for exactly this; single_view (V = 1): torch.std of one view is NaN, so are the kernel's two
    statistics, and nothing else is."""
    R, S = 37, 19
    net = C.make_net(71).to(DEV)
    if edge == "identical_views":
        x = C.embed_case(5100, R, S, 6)
        x = x[:, :, :1].expand(R, S, 6, 35).contiguous()
    elif edge == "spread":
        x = C.embed_case(5101, R, S, 6, offset=32.0)
    else:
        x = C.embed_case(5102, R, S, 1)
    table, ref = _embed_compare(f"embed stats, {edge}", net, x)
    if edge == "identical_views":
        assert float(ref["std"].abs().max()) <= 1e-12
    if edge == "single_view":
        assert bool(torch.isnan(ref["std"]).all()) and bool(torch.isnan(ref["std_norm"]).all())
        assert not bool(torch.isnan(ref["feat"]).any()) and not bool(torch.isnan(ref["q0"]).any())


def test_posfc_grid_rounds():
    """(1725, 19): N = 32 775, a partial tile in the second round whose clamped lanes read the per-ray operand through
    g / S; both even layers of a depth-4 network (they share one position GEMM, 256 bytes apart)"""
    R, S = 1725, 19
    n = R * S
    net = C.make_net(80, depth=4).to(DEV)
    q, pe_p, pe_v = (t.to(DEV) for t in C.posfc_case(6000, net, R, S))

    def run():  # GNT.forward's dispatch
        if ops.gnt_posfc_available(net.q_fcs, 64):
            fused = ops.GntPosFc(net.q_fcs, pe_p, pe_v)
            return {f"layer {i}": fused(i, q).reshape(n, 64) for i in (0, 2)}
        return {f"layer {i}": C.stmt_posfc(net, i, q, pe_p, pe_v).reshape(n, 64) for i in (0, 2)}

    ref = {f"layer {i}": C.ref_posfc(C.weights64(net.q_fcs[i]), q, pe_p, pe_v).reshape(n, 64) for i in (0, 2)}
    _compare(f"posfc ({R}, {S})", run, ref, (b"gnt_posfc",), paths=ONE, rows={k: _unit_rows(n, EMB_TILE, EMB_ROUND) for k in ref})


@pytest.mark.parametrize("R,S", [(1025, 1), (3, 257)])
def test_head_edges(R, S):
    """one workgroup per ray (no wrap in R: 1025 workgroups); S = 257: the 256-thread sample loop's second trip with one
    live thread"""
    net = C.make_net(90).to(DEV)
    q = (C.rows_case(7000 + S, R, S) + 0.5).to(DEV)

    def run():  # GNT.forward's dispatch
        if ops.gnt_head_available(net.norm, net.rgb_fc):
            return {"rgb": ops.gnt_head(net.norm, net.rgb_fc, q)}
        return {"rgb": C.stmt_head(net, q)}

    W = {k: v for k, v in C.weights64(net).items() if k.startswith(("norm.", "rgb_fc."))}
    _compare(f"head ({R}, {S})", run, {"rgb": C.ref_head(W, q)}, (b"gnt_head",), paths=ONE)
