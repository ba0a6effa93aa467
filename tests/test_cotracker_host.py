"""pgdvs_amd.models.cotracker on the CPU (the torch statement of the correlation step) against what the reference's own
classes computed for the seeded cases of tests/cotracker_cases.py (tests/golden/make_golden_cotracker.py wrote the
fixtures; it ran the reference around a stand-in for timm's Attention and Mlp, and with seeded random weights: nothing here
pins timm itself or says anything about a trained checkpoint).

Every comparison is |ours - reference float64| <= tol, tol = 4 x the reference's own float32-vs-float64 gap of that case
(stored in the fixture).  Weights and inputs are regenerated from seeds; their float64 checksum is asserted first.
tests/test_gpu_cotracker.py imports the helpers below and runs the same cases through the HIP statement.
"""
import numpy as np
import pytest
import torch

import cotracker_cases as CC

BUILDERS = ("cotracker_stride_4_wind_8", "cotracker_stride_4_wind_12", "cotracker_stride_8_wind_16")
T = torch.from_numpy


@pytest.fixture(scope="module")
def fx_lookup(golden_dir):
    return dict(np.load(golden_dir / "cotracker_lookup.npz"))


@pytest.fixture(scope="module")
def fx_model(golden_dir):
    return dict(np.load(golden_dir / "cotracker_model.npz"))


def err(ours, ref64):
    return float(np.abs(np.asarray(ours, np.float64) - np.asarray(ref64, np.float64)).max())


def assert_close(ours, fx, key, what):
    """|ours - f64_<key>| <= tol_<key>; the figure is printed before it is asserted"""
    e, tol = err(ours, fx[f"f64_{key}"]), float(fx[f"tol_{key}"])
    print(f"{what}: max |ours - float64 reference| = {e:.3g}, tol {tol:.3g}")
    assert np.asarray(ours).shape == fx[f"f64_{key}"].shape and np.isfinite(np.asarray(ours)).all()
    assert e <= tol, (what, e, tol)


def step_model(device="cpu"):
    from pgdvs_amd.models.cotracker import build_cotracker

    return CC.fill(build_cotracker(None).eval(), CC.STEP["seed_w"]).to(device)


def tamed_model(device="cpu"):
    from pgdvs_amd.models.cotracker import build_cotracker

    return CC.fill(build_cotracker(None).eval(), CC.MODEL_SEED, CC.tamed_gain).to(device)


def run_step(model, fx, iters, device="cpu"):
    x = CC.step_inputs()
    assert CC.checksum(model, *x.values()) == fx["chk_step"]
    with torch.no_grad():
        preds, vis, _ = model.forward_iteration(iters=iters, **{k: T(v).to(device) for k, v in x.items()})
    return torch.stack(preds).cpu().numpy(), vis.cpu().numpy()


def check_step(model, fx, iters, device="cpu"):
    coords, vis = run_step(model, fx, iters, device)
    assert_close(coords, fx, f"step{iters}_coords", f"step iters={iters} coords [px]")
    assert_close(vis, fx, f"step{iters}_vis", f"step iters={iters} visibility logits")


def check_fnet(model, fx, size, device="cpu"):
    img = CC.fnet_input(size)
    tag = f"fnet_{size[0]}x{size[1]}"
    assert CC.checksum(img) == fx[f"chk_{tag}"]
    with torch.no_grad():
        out = model.fnet(T(img).to(device)).cpu().numpy()
    assert_close(out, fx, tag, tag)


def check_forward(model, fx, name, device="cpu"):
    video, queries = CC.forward_inputs(name)
    assert CC.checksum(model) == fx["chk_model"] and CC.checksum(video, queries) == fx[f"chk_{name}"]
    with torch.no_grad():
        traj, _, vis, _ = model(rgbs=T(video).to(device), queries=T(queries).to(device), iters=CC.FORWARD_ITERS)
    assert_close(traj.cpu().numpy(), fx, f"{name}_tracks", f"forward {name} tracks [px]")
    assert_close(vis.cpu().numpy(), fx, f"{name}_vis", f"forward {name} visibility")


def make_interface(fx, device="cpu"):
    from pgdvs_amd.models.cotracker import CoTrackerInterface

    iface = CoTrackerInterface(None, ori_rgb_range="0_1", query_chunk_size=4096)
    net = CC.fill(iface.model.model, CC.MODEL_SEED, CC.tamed_gain)
    assert CC.checksum(net) == fx["chk_model"]
    with torch.no_grad():
        net.vis_predictor[0].bias.fill_(float(fx["iface_vis_bias"]))
    return iface.to(device).eval()


def check_interface(iface, fx, device="cpu"):
    frames, qpts = CC.clip_inputs()
    assert CC.checksum(frames, qpts) == fx["chk_iface"]
    tracks, visibles = iface(frames=T(frames).to(device), query_points=T(qpts).to(device))
    assert tracks.shape == (len(qpts), len(frames), 2) and tracks.dtype == torch.float32
    assert visibles.shape == (len(qpts), len(frames)) and visibles.dtype == torch.bool
    assert_close(tracks.cpu().numpy(), fx, "iface_tracks", "interface tracks [px]")
    excluded, want = fx["iface_excluded"], fx["f64_iface_vis"] > 0.9
    assert excluded.mean() <= 0.10 and 0.2 <= want.mean() <= 0.8  # the generator's own assertions, again
    assert np.array_equal(visibles.cpu().numpy()[~excluded], want[~excluded])
    assert np.array_equal(fx["f32_iface_visibles"][~excluded], want[~excluded])


# ---------------------------------------------------------------- the torch statement against every fixture
@pytest.mark.parametrize("name", list(CC.LOOKUP_CASES))
def test_corr_block_vs_fixture(fx_lookup, name):
    from pgdvs_amd.models.cotracker.blocks import CorrBlock

    fmaps, feats, coords, kind = CC.lookup_inputs(name)
    assert CC.checksum(fmaps, feats, coords) == fx_lookup[f"{name}__chk"]
    blk = CorrBlock(T(fmaps)[None], num_levels=4, radius=3)
    blk.corr(T(feats)[None])
    out = blk.sample(T(coords)[None])[0].numpy()
    e, tol = err(out, fx_lookup[f"{name}__f64"]), float(fx_lookup[f"{name}__tol"])
    print(f"{name}: max |ours - float64 reference| = {e:.3g}, tol {tol:.3g}")
    assert out.shape == fx_lookup[f"{name}__f64"].shape and e <= tol
    zero = (kind == 5) | (kind == 7)
    assert zero.any() and not out[zero][:, :49].any()  # every tap of level 0 outside the level


@pytest.fixture(scope="module")
def full_gain_model():
    return step_model()


@pytest.fixture(scope="module")
def whole_model():
    return tamed_model()


@pytest.mark.parametrize("iters", [1, 2])
def test_forward_iteration_vs_fixture(fx_model, full_gain_model, iters):
    check_step(full_gain_model, fx_model, iters)
    assert full_gain_model.last_corr_path == "torch"


@pytest.mark.parametrize("size", CC.FNET_SIZES)
def test_fnet_vs_fixture(fx_model, full_gain_model, size):
    check_fnet(full_gain_model, fx_model, size)


@pytest.mark.parametrize("name", list(CC.FORWARD_CASES))
def test_forward_vs_fixture(fx_model, whole_model, name):
    check_forward(whole_model, fx_model, name)


def test_interface_vs_fixture(fx_model):
    check_interface(make_interface(fx_model), fx_model)


def test_torch_statement_keeps_autograd(fx_model, full_gain_model):
    """with gradients enabled the correlation step stays on torch and a loss on the coordinates reaches fnet's features"""
    x = {k: T(v) for k, v in CC.step_inputs().items()}
    x["fmaps"].requires_grad_(True)
    preds, _, _ = full_gain_model.forward_iteration(iters=1, **x)
    preds[-1].sum().backward()
    assert full_gain_model.last_corr_path == "torch" and x["fmaps"].grad is not None and bool(x["fmaps"].grad.abs().sum() > 0)
    full_gain_model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------- state dict
@pytest.mark.parametrize("name", BUILDERS)
def test_state_dict_keys_and_shapes_equal_upstream(fx_model, name):
    from pgdvs_amd.models.cotracker import build_cotracker

    from pgdvs_amd.models.cotracker.model import _CONFIGS, CoTracker

    stride, window = _CONFIGS[name]
    assert (stride, window) == tuple(int(v) for v in name.replace("cotracker_stride_", "").split("_wind_"))
    model = build_cotracker(None) if name == BUILDERS[0] else CoTracker(stride=stride, S=window, space_depth=6, time_depth=6)
    assert (model.stride, model.S) == (stride, window)
    sd = model.state_dict()
    assert list(sd.keys()) == list(fx_model[f"keys__{name}"])
    assert [" ".join(map(str, v.shape)) for v in sd.values()] == list(fx_model[f"shapes__{name}"])


def test_checkpoint_loads_strictly(tmp_path, whole_model):
    """a state dict saved under an upstream checkpoint name, bare or under "model", loads strictly into the model the name asks for"""
    from pgdvs_amd.models.cotracker import build_cotracker

    for k, payload in enumerate((whole_model.state_dict(), {"model": whole_model.state_dict()})):
        path = tmp_path / str(k) / "cotracker_stride_4_wind_8.pth"
        path.parent.mkdir()
        torch.save(payload, path)
        loaded = build_cotracker(str(path))
        assert (loaded.stride, loaded.S) == (4, 8) and CC.checksum(loaded) == CC.checksum(whole_model)
    with pytest.raises(ValueError):
        build_cotracker("cotracker_stride_2_wind_4.pth")


# ---------------------------------------------------------------- interface contract
class _RecordingPredictor(torch.nn.Module):
    """stands in for CoTrackerPredictor: records its arguments, returns tracks = the query's (x, y) - 3 in every frame"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, video, queries=None):
        self.calls.append((video.clone(), queries.clone()))
        n_frames = video.shape[1]
        tracks = (queries[:, None, :, 1:] - 3.0).repeat(1, n_frames, 1, 1)
        return tracks, (queries[:, None, :, 0] <= torch.arange(n_frames)[None, :, None])


def test_interface_contract():
    from pgdvs_amd.models.cotracker import CoTrackerInterface

    iface = CoTrackerInterface(None, ori_rgb_range="0_1", query_chunk_size=4, local_rank=0)
    assert iface.separate_fwd_bwd is True and iface.query_chunk_size == 4
    iface.model = rec = _RecordingPredictor()
    frames = torch.linspace(-0.2, 1.2, 3 * 6 * 8 * 3).reshape(3, 6, 8, 3)
    q = torch.tensor([[0, 1, 2], [1, 5, 7], [2, 0, 0], [0, 4, 6], [1, 2, 1], [2, 3, 3], [0, 5, 0], [1, 0, 7], [2, 2, 2], [0, 1, 1]]).float()
    tracks, visibles = iface(frames=frames, query_points=q)
    assert tracks.shape == (10, 3, 2) and tracks.dtype == torch.float32 and visibles.shape == (10, 3) and visibles.dtype == torch.bool
    assert [c[1].shape[1] for c in rec.calls] == [4, 4, 2]  # chunks of query_chunk_size
    video = rec.calls[0][0]
    assert video.shape == (1, 3, 3, 6, 8) and float(video.min()) == 0.0 and float(video.max()) == 255.0  # 0_1 -> 0_255, clamped
    assert torch.equal(video[0, :, :, 2, 3], (frames[:, 2, 3, :].clamp(0, 1) * 255.0))
    sent = torch.cat([c[1] for c in rec.calls], dim=1)[0]
    assert torch.equal(sent, q[:, [0, 2, 1]])  # (t, row, col) -> (t, x, y)
    assert torch.equal(tracks[:, 0, :], (q[:, [2, 1]] - 3.0).clamp(min=0.0)) and bool((q[:, [2, 1]] - 3.0).min() < 0)  # the clip at 0
    assert torch.equal(visibles, q[:, 0:1] <= torch.arange(3)[None, :])
    iface255 = CoTrackerInterface(None, ori_rgb_range="0_255")
    iface255.model = rec255 = _RecordingPredictor()
    iface255(frames=frames * 100.0, query_points=q[:2])
    assert torch.equal(rec255.calls[0][0][0, :, :, 2, 3], frames[:, 2, 3, :] * 100.0)  # same range: passed through


def test_predictor_builds_only_the_sparse_call():
    from pgdvs_amd.models.cotracker import CoTrackerPredictor

    pred = CoTrackerPredictor(checkpoint=None)
    assert pred.interp_shape == (384, 512) and pred.support_grid_size == 6 and not pred.model.training
    with pytest.raises(NotImplementedError):
        pred(torch.zeros(1, 2, 3, 32, 32), queries=None)


def test_config_instantiates():
    from pgdvs_amd.instantiate import instantiate, load_config
    from pgdvs_amd.models.cotracker import CoTrackerInterface

    cfg = load_config(tracker="cotracker_hip")
    assert cfg.tracker._target_ == "pgdvs_amd.models.cotracker.interface.CoTrackerInterface"
    assert cfg.tracker.ckpt_path == "cotracker_stride_4_wind_8.pth" and cfg.tracker.query_chunk_size == 4096
    # no checkpoint exists where the tests run: the configured file name selects the model, the weights stay fresh
    tracker = instantiate(cfg.tracker, ckpt_path=None, ori_rgb_range="0_1", local_rank=0)
    assert isinstance(tracker, CoTrackerInterface) and tracker.query_chunk_size == 4096 and tracker.separate_fwd_bwd
    assert (tracker.model.model.stride, tracker.model.model.S) == (4, 8)
    assert load_config(tracker="cotracker").tracker._target_ == "pgdvs.models.cotracker.interface.CoTrackerInterface"  # unchanged
