"""pgdvs_amd.preprocess.final_mask on the host (numpy / scipy.ndimage) against the reference's fixture
(tests/golden/make_golden_final_mask.py -> preprocess_final_mask.npz): every key of every frame of the four sequences bit
for bit (dyn_cnt as float32 bits), each frame once from the previous state the fixture stored and once in a chain that
carries its own state; the warp against the stored warped count; the class-id masks; the error cases; and ``run_masks`` on
a tree built from sequence A, whose files must read back as the fixture's ``final`` and be found by ``run_zoedepth``."""
import pathlib

import numpy as np
import PIL.Image
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SEQUENCES = ("A", "B", "C", "D")
MASK_KEYS = ("ade20k", "coco", "sem", "warp_prev", "dyn_track", "raw_no_warp", "raw", "raw_eroded", "final_raw", "final", "next_prev")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_final_mask.npz"))


def frames(fx, seq):
    return range(int(fx[f"{seq}_n_frames"]))


def sam_of(fx, seq, t):
    W = fx[f"{seq}_f{t}_raw"].shape[1]
    return np.unpackbits(fx[f"{seq}_f{t}_sam"], axis=2, count=W).astype(bool)


def frame_inputs(fx, seq, t, stored_state=True):
    """the keywords of combine_masks for frame t; ``stored_state``: with the previous state the fixture recorded"""
    p = f"{seq}_f{t}_"
    kw = dict(mask_type="semantic" if seq == "D" else "flow_epi", img_idx=t, mask_sam=sam_of(fx, seq, t))
    if seq == "D":
        kw.update(sem_seg_ade20k=fx[p + "sem_ade20k"], sem_seg_coco=fx[p + "sem_coco"])
    else:
        kw.update(mask_flow_epi=fx[p + "raw_no_warp"])
    if t > 0:
        kw.update(bwd_flow=fx[p + "bwd_flow"], bwd_coord_diff=fx[p + "bwd_coord_diff"])
        if stored_state:
            kw.update(prev_mask_final_raw=fx[p + "prev_mask"], prev_dyn_cnt=fx[p + "prev_cnt"])
    return kw


def assert_frame(got, fx, seq, t, to_numpy=np.asarray):
    """every key of the returned dict against the fixture; a key the fixture lacks is one upstream returns as None"""
    p = f"{seq}_f{t}_"
    for k in MASK_KEYS:
        if p + k not in fx:
            assert got[k] is None, (seq, t, k)
            continue
        g = to_numpy(got[k])
        assert g.dtype == bool and np.array_equal(g, fx[p + k]), (seq, t, k, int((g != fx[p + k]).sum()))
    cnt = to_numpy(got["dyn_cnt"])
    assert cnt.dtype == np.float32 and np.array_equal(cnt.view(np.uint32), fx[p + "dyn_cnt"].view(np.uint32)), (seq, t, "dyn_cnt")


def segment_reference(fx, seq, t):
    """(n_pix, n_overlap, selected) from the fixture's own arrays"""
    sam, eroded = sam_of(fx, seq, t), fx[f"{seq}_f{t}_raw_eroded"]
    n_pix = sam.reshape(len(sam), eroded.size).sum(1)
    n_overlap = (sam & eroded[None]).reshape(len(sam), eroded.size).sum(1)
    return n_pix, n_overlap, (n_overlap > 0) & (n_overlap.astype(np.float64) > 0.1 * n_pix.astype(np.float64))


# ---------------------------------------------------------------------------- combine_masks
@pytest.mark.parametrize("seq", SEQUENCES)
def test_combine_masks_numpy_per_frame(fx, seq):
    from pgdvs_amd.preprocess import combine_masks

    for t in frames(fx, seq):
        assert_frame(combine_masks(**frame_inputs(fx, seq, t)), fx, seq, t)


@pytest.mark.parametrize("seq", SEQUENCES)
def test_combine_masks_numpy_as_sequence(fx, seq):
    from pgdvs_amd.preprocess import combine_masks

    prev_mask = prev_cnt = None
    for t in frames(fx, seq):
        res = combine_masks(prev_mask_final_raw=prev_mask, prev_dyn_cnt=prev_cnt, **frame_inputs(fx, seq, t, stored_state=False))
        assert_frame(res, fx, seq, t)
        prev_mask, prev_cnt = res["next_prev"], res["dyn_cnt"]


def test_fixture_holds_what_the_tests_rely_on(fx):
    """the ties of the selection and of the dynamic track are in the fixture, and so are n_seg 0 and 1"""
    for seq in "AB":
        for t in frames(fx, seq):
            n_pix, n_overlap, selected = segment_reference(fx, seq, t)
            for n_o, n_p in ((5, 50), (3, 30), (7, 70)):
                assert ((n_pix == n_p) & (n_overlap == n_o) & ~selected).any(), (seq, t, n_o)
            assert ((n_pix == 50) & (n_overlap == 6) & selected).any()
            assert (n_pix == 0).any() and (n_pix == 1).any() and (n_pix == fx[f"{seq}_f{t}_raw"].size).any()
    assert max(int(fx[f"A_f{t}_n_ties"]) for t in (1, 3)) >= 20
    assert [len(sam_of(fx, "C", t)) for t in frames(fx, "C")] == [0, 1] and len(sam_of(fx, "A", 0)) == 70
    assert np.abs(fx["B_f1_bwd_flow"]).max() == 1e4


def test_segment_selection_is_a_strict_float64_comparison():
    from pgdvs_amd.preprocess.final_mask import segments_selected

    n_pix, n_overlap = np.array([50, 30, 70, 50, 10, 10, 7]), np.array([5, 3, 7, 6, 1, 2, 0])
    assert segments_selected(n_pix, n_overlap).tolist() == [False, False, False, True, False, True, False]


# ---------------------------------------------------------------------------- the warp
def test_cubic_table(fx):
    from pgdvs_amd.preprocess import cubic_table

    tab = cubic_table()
    assert tab.dtype == np.float32 and tab.shape == (32, 4) and np.array_equal(tab, fx["table"])
    assert np.array_equal(tab[0], [0, 1, 0, 0]) and np.array_equal(tab[16], [-0.09375, 0.59375, 0.59375, -0.09375])


def test_warp_flow_numpy_vs_fixture(fx):
    from pgdvs_amd.preprocess import warp_flow_numpy

    n = 0
    for seq in "ABC":
        for t in list(frames(fx, seq))[1:]:
            p = f"{seq}_f{t}_"
            got = warp_flow_numpy(fx[p + "prev_cnt"], fx[p + "bwd_flow"])
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fx[p + "cnt_warp"].view(np.uint32)), (seq, t)
            n += 1
    assert n == 7


def test_warp_flow_numpy_by_hand():
    from pgdvs_amd.preprocess import warp_flow_numpy

    img = np.arange(30, dtype=np.float32).reshape(5, 6)
    flow = np.zeros((5, 6, 2), np.float32)
    assert np.array_equal(warp_flow_numpy(img, flow), img)
    flow[..., 0] = 1.0  # one pixel to the right; the last column reads outside: zero
    assert np.array_equal(warp_flow_numpy(img, flow)[:, :5], img[:, 1:]) and not warp_flow_numpy(img, flow)[:, 5].any()
    flow[..., 0] = np.nan  # a NaN coordinate clamps to -8: wholly outside
    flow[..., 1] = 1e30
    assert not warp_flow_numpy(img, flow).any()
    flow[:] = (0.5, 0)  # the half-pixel weights on a row 0 1 2 3: -0.09375 * 0 + 0.59375 * 1 + 0.59375 * 2 - 0.09375 * 3
    assert warp_flow_numpy(img, flow)[0, 1] == np.float32(1.5)


# ---------------------------------------------------------------------------- class ids
def test_semantic_mask(fx):
    from pgdvs_amd.preprocess import DYNAMIC_IDS_ADE20K, DYNAMIC_IDS_COCO, semantic_mask

    ade, coco, sem = semantic_mask(fx["D_f0_sem_ade20k"], fx["D_f0_sem_coco"])
    for got, key in ((ade, "ade20k"), (coco, "coco"), (sem, "sem")):
        assert got.dtype == bool and np.array_equal(got, fx[f"D_f0_{key}"]), key
    assert len(DYNAMIC_IDS_ADE20K) == 18 and len(DYNAMIC_IDS_COCO) == 25 and max(DYNAMIC_IDS_ADE20K) == 150
    ids = np.array([[-1, 0, 12, 13, 11, 149, 150]])
    assert semantic_mask(ids, ids)[0].tolist() == [[False, False, True, False, False, True, False]]  # id + 1 is listed
    assert semantic_mask(ids, ids)[1].tolist() == [[False, True, False, False, False, False, False]]


# ---------------------------------------------------------------------------- errors
def test_error_cases(fx, tmp_path):
    from pgdvs_amd.preprocess import combine_masks, run_masks

    kw = frame_inputs(fx, "C", 0)
    with pytest.raises(NotImplementedError):
        combine_masks(**dict(kw, mask_type="flow_depth"))
    with pytest.raises(ValueError, match="bogus"):
        combine_masks(**dict(kw, mask_type="bogus"))
    with pytest.raises(NotImplementedError):
        run_masks(root_dir=tmp_path, save_dir=tmp_path, segmenter=lambda img: None, mask_type="flow_depth")
    with pytest.raises(ValueError, match="bogus"):
        run_masks(root_dir=tmp_path, save_dir=tmp_path, segmenter=lambda img: None, mask_type="bogus")
    with pytest.raises(ValueError, match="segmenter"):
        run_masks(root_dir=tmp_path, save_dir=tmp_path, segmenter=None)
    with pytest.raises(ValueError, match="semantic"):
        run_masks(root_dir=tmp_path, save_dir=tmp_path, segmenter=lambda img: None, mask_type="semantic")


# ---------------------------------------------------------------------------- run_masks
def write_llff_cameras(root, all_w2c, all_K, H, W):
    """poses_bounds_cvd.npy, one row per camera: [down, right, back | t | (h, w, f)] and two bounds"""
    rows = []
    for w2c, K in zip(all_w2c, all_K):
        c2w = np.linalg.inv(w2c)
        m = np.stack([c2w[:3, 1], c2w[:3, 0], -c2w[:3, 2], c2w[:3, 3], np.array([2.0 * H, 2.0 * W, K[0, 0]])], 1)
        rows.append(np.concatenate([m.reshape(-1), [0.5, 9.0]]))
    np.save(root / "poses_bounds_cvd.npy", np.stack(rows))


def build_tree(fx, root, cameras, flow_dirname="flows"):
    """sequence A as a scene directory: six images (pixel (0, 0) carries the frame number in R, and B = 100), the stored
    forward files, the backward files the warp reads, a zero backward file for the sixth image, cameras in either format"""
    names = [str(n) for n in fx["A_names"]]
    H, W = fx["A_f0_raw"].shape
    (root / "rgbs").mkdir(parents=True)
    flow_dir = root / flow_dirname / "interval_1"
    flow_dir.mkdir(parents=True)
    for t, name in enumerate(names):
        img = np.zeros((H, W, 3), np.uint8)
        img[..., 0], img[..., 2] = t, 100
        PIL.Image.fromarray(img).save(root / "rgbs" / f"{name}.png")
    for t in range(len(names) - 1):
        np.savez(flow_dir / f"{names[t]}_{names[t + 1]}.npz", flow=fx[f"A_f{t}_epi_flow"], coord_diff=fx[f"A_f{t}_epi_coord_diff"])
        if t > 0:
            np.savez(flow_dir / f"{names[t]}_{names[t - 1]}.npz", flow=fx[f"A_f{t}_bwd_flow"], coord_diff=fx[f"A_f{t}_bwd_coord_diff"])
    zeros = np.zeros((H, W, 2), np.float32)
    np.savez(flow_dir / f"{names[-1]}_{names[-2]}.npz", flow=zeros, coord_diff=zeros)
    if cameras == "dycheck":
        np.savez(root / "camera.npz", all_K=fx["A_K"], all_w2c=fx["A_w2c"])
    else:
        write_llff_cameras(root, fx["A_w2c"], fx["A_K"], H, W)
    return names


def stub_segmenter(fx, as_tensor=None):
    """the fixture's segments of the frame whose number the image carries; checks that the image arrives as BGR uint8"""
    def segmenter(img):
        assert img.dtype == np.uint8 and img.ndim == 3 and img[0, 0, 0] == 100 and img[0, 0, 1] == 0
        t = int(img[0, 0, 2])
        sam = sam_of(fx, "A", min(t, 4))
        return sam if as_tensor is None else as_tensor(sam)
    return segmenter


def read_mask(path):
    return np.array(PIL.Image.open(path))


@pytest.mark.parametrize("cameras", ["llff", "dycheck"])
def test_run_masks_numpy_writes_the_fixtures_final(fx, tmp_path, cameras):
    from pgdvs_amd.preprocess import run_masks

    names = build_tree(fx, tmp_path / "scene", cameras)
    written = run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "out", segmenter=stub_segmenter(fx),
                        flag_dycheck_format=cameras == "dycheck")
    assert len(written) == 2 * len(names)
    for t in range(5):
        f = tmp_path / "out/masks/final" / f"{names[t]}_final.png"
        assert f in written and PIL.Image.open(f).mode == "1"
        assert np.array_equal(read_mask(f), fx[f"A_f{t}_final"]), t
        epi = read_mask(tmp_path / "out/masks/flow_epi" / f"{names[t]}.png")
        assert epi.dtype == np.uint8 and np.array_equal(epi, fx[f"A_f{t}_raw_no_warp"] * np.uint8(255)), t


def test_run_masks_for_colmap(fx, tmp_path):
    from pgdvs_amd.preprocess import run_masks

    names = build_tree(fx, tmp_path / "scene", "llff", flow_dirname="flows_for_colmap")
    written = run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "out", segmenter=stub_segmenter(fx), for_colmap=True)
    assert not list((tmp_path / "out").rglob("*_final.png")) and not (tmp_path / "out/masks").exists()
    for t in range(5):
        f = tmp_path / "out/masks_for_colmap" / f"{names[t]}.png.png"
        assert f in written and np.array_equal(read_mask(f), ~fx[f"A_f{t}_final"]), t


def test_run_zoedepth_finds_the_masks_run_masks_wrote(fx, tmp_path):
    """run_zoedepth checks its mask paths before anything else: with the masks in place it gets past that check and stops
    at the next file it needs"""
    from pgdvs_amd.preprocess import run_masks, run_zoedepth

    build_tree(fx, tmp_path / "scene", "llff")
    model = lambda x: x[:, :1]  # noqa: E731
    with pytest.raises(FileNotFoundError, match="_final.png"):
        run_zoedepth(tmp_path / "scene", tmp_path / "out", tmp_path / "out", model, "N")
    run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "out", segmenter=stub_segmenter(fx))
    with pytest.raises(FileNotFoundError, match="points3D.bin"):
        run_zoedepth(tmp_path / "scene", tmp_path / "out", tmp_path / "out", model, "N")


def test_run_masks_semantic_with_stub_networks(fx, tmp_path):
    """the semantic branch: the plug-in's class ids of sequence D, one frame, no flow and no cameras read"""
    from pgdvs_amd.preprocess import run_masks

    H, W = fx["D_f0_raw"].shape
    (tmp_path / "scene/rgbs").mkdir(parents=True)
    PIL.Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(tmp_path / "scene/rgbs/00000.png")
    written = run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "out", segmenter=lambda img: sam_of(fx, "D", 0),
                        semantic=lambda img: (fx["D_f0_sem_ade20k"], fx["D_f0_sem_coco"]), mask_type="semantic")
    assert [f.name for f in written] == ["00000_final.png"] and np.array_equal(read_mask(written[0]), fx["D_f0_final"])


def test_frames_to_aligned_depths_with_stub_models(tmp_path):
    """run_flow -> run_masks -> run_zoedepth on one synthetic scene: no mask file is written by hand"""
    import struct

    import torch

    from pgdvs_amd.preprocess import run_flow, run_masks, run_zoedepth

    H, W, n = 24, 32, 4
    root = tmp_path / "scene"
    (root / "rgbs").mkdir(parents=True)
    (root / "sparse").mkdir()
    for i in range(n):
        PIL.Image.fromarray(np.full((H, W, 3), 40 * i, np.uint8)).save(root / "rgbs" / f"{i:05d}.png")
    w2c = np.stack([np.eye(4)] * n)
    w2c[:, 0, 3] = -0.5 * np.arange(n)  # translation along x: the epipolar distance is |flow_y|
    K = np.array([[30.0, 0, W / 2.0], [0, 30.0, H / 2.0], [0, 0, 1]])
    write_llff_cameras(root, w2c, np.stack([K] * n), H, W)
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(-1.2, 2.5, 60), rng.uniform(-1, 1, 60), rng.uniform(3, 5, 60)], -1)
    with open(root / "sparse/points3D.bin", "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for i, q in enumerate(pts):
            f.write(struct.pack("<QdddBBBdQ", i + 1, *map(float, q), 1, 2, 3, 0.25, 0))

    def flow_model(fn1, fn2):
        """an object of 9 x 8 pixels that moves across the rows, consistently in both directions"""
        flow = torch.zeros((1, 2, H, W))
        flow[0, 1, 6:15, 10:18] = 4.0
        back = torch.zeros((1, 2, H, W))
        back[0, 1, 10:19, 10:18] = -4.0
        return flow, back

    def segmenter(img):
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        sam = np.zeros((2, H, W), bool)
        sam[0, 4:17, 8:20] = True
        sam[1, :, 24:] = True
        return sam

    def depth_model(X):
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        return (3.0 + 0.05 * xs + 0.02 * ys)[None, None]

    run_flow(root / "rgbs", root / "flows", flow_model, img_pair_max_diff=1)
    masks = run_masks(root_dir=root, save_dir=root, segmenter=segmenter)
    finals = [np.array(PIL.Image.open(f)) for f in masks if f.name.endswith("_final.png")]
    assert len(finals) == n and all(m.dtype == bool and m.any() and not m.all() for m in finals)
    assert finals[0][4:17, 8:20].all() and not finals[0][:, 26:].any()  # grown to the overlapping segment, not to the other
    depths = run_zoedepth(root, root, root, depth_model, "N")
    assert [f.name for f in depths] == [f"{i:05d}.npz" for i in range(n)]
    assert all(np.isfinite(np.load(f)["disp_indiv_scale_med"]) for f in depths)


# ---------------------------------------------------------------------------- the C ABI's declarations
def test_abi_declares_the_mask_entry_points():
    import re

    from pgdvs_amd import _lib

    header = (ROOT / "include/pgdvs_hip.h").read_text()
    for name in ("pgdvs_mask_combine_workspace_bytes", "pgdvs_mask_combine", "pgdvs_semantic_mask"):
        m = re.search(r"^\w+ " + name + r"\(([^;]*)\);", header, re.MULTILINE)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_ops_refuse_cpu_tensors():
    import torch

    from pgdvs_amd import ops
    from pgdvs_amd._lib import PgdvsHipError

    with pytest.raises(PgdvsHipError):
        ops.mask_combine(torch.zeros((4, 5), dtype=torch.bool), torch.zeros((1, 4, 5), dtype=torch.bool), img_idx=0)
    with pytest.raises(PgdvsHipError):
        ops.semantic_mask(torch.zeros((4, 5), dtype=torch.int64), torch.zeros((4, 5), dtype=torch.int64), [1], [1])
