"""The final motion mask on the MI355X (csrc/mask_combine.hip) against the reference's fixture (preprocess_final_mask.npz;
the helpers and what the fixture holds: test_final_mask_host.py), bit for bit, dyn_cnt as float32 bits.

per frame        ``combine_masks(device=...)`` from the previous state the fixture stored, numpy in: a failure names its frame.
as sequences     the state (``next_prev``, ``dyn_cnt``) and the segments stay on the device from frame to frame.
segments         ``ops.mask_combine``'s seg_counts / seg_selected against counts made from the fixture's arrays in numpy: 70
                 segments of 1961 pixels start at every 16-byte phase; bytes of 200 instead of 1 count as set.
larger frames    131 x 257 (more than one workgroup of the count pass per segment, odd) and 64 x 128 (every segment
                 16-byte aligned, whole tiles), three frames each, against the host path, which the fixture pins.
invalid shapes   the library's error, nothing launched.
run_masks        ``device="cuda"`` writes the bytes ``device=None`` writes."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_final_mask_host import SEQUENCES, assert_frame, build_tree, frame_inputs, frames, sam_of, segment_reference, stub_segmenter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(golden_dir / "preprocess_final_mask.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    assert t.is_cuda
    return t.cpu().numpy()


@pytest.mark.parametrize("seq", SEQUENCES)
def test_combine_masks_device_per_frame(fx, seq):
    from pgdvs_amd.preprocess import combine_masks

    for t in frames(fx, seq):
        assert_frame(combine_masks(device=DEV, **frame_inputs(fx, seq, t)), fx, seq, t, to_numpy=host)


@pytest.mark.parametrize("seq", SEQUENCES)
def test_combine_masks_device_as_sequence(fx, seq):
    """segments as GPU bool tensors, the state never leaves the device"""
    from pgdvs_amd.preprocess import combine_masks

    prev_mask = prev_cnt = None
    for t in frames(fx, seq):
        kw = frame_inputs(fx, seq, t, stored_state=False)
        kw["mask_sam"] = dev(kw["mask_sam"])
        assert kw["mask_sam"].dtype == torch.bool
        res = combine_masks(device=DEV, prev_mask_final_raw=prev_mask, prev_dyn_cnt=prev_cnt, **kw)
        assert_frame(res, fx, seq, t, to_numpy=host)
        prev_mask, prev_cnt = res["next_prev"], res["dyn_cnt"]


def op_inputs(fx, seq, t):
    p = f"{seq}_f{t}_"
    prev = {}
    if t > 0:
        prev = dict(prev_mask=dev(fx[p + "prev_mask"]), prev_cnt=dev(fx[p + "prev_cnt"]), bwd_flow=dev(fx[p + "bwd_flow"]),
                    bwd_coord_diff=dev(fx[p + "bwd_coord_diff"]))
    return dev(fx[p + "raw_no_warp"]), prev


@pytest.mark.parametrize("seq", "ABC")
def test_segment_counts_and_selection(fx, seq):
    from pgdvs_amd import ops

    for t in frames(fx, seq):
        raw_no_warp, prev = op_inputs(fx, seq, t)
        sam = sam_of(fx, seq, t)
        n_pix, n_overlap, selected = segment_reference(fx, seq, t)
        for scale in (1, 200):  # any non-zero byte is a set pixel
            out = ops.mask_combine(raw_no_warp, dev(sam.astype(np.uint8) * np.uint8(scale)), img_idx=t, want_segments=True, **prev)
            counts = host(out["seg_counts"])
            assert counts.dtype == np.int32 and counts.shape == (len(sam), 2)
            assert np.array_equal(counts[:, 0], n_pix) and np.array_equal(counts[:, 1], n_overlap), (seq, t, scale)
            assert np.array_equal(host(out["seg_selected"]).astype(bool), selected), (seq, t, scale)
            assert np.array_equal(host(out["final"]).astype(bool), fx[f"{seq}_f{t}_final"]), (seq, t, scale)


def test_thresholds_are_arguments(fx):
    """another overlap threshold selects the tie segments; the float32 just below 0.5 as dyn_track threshold takes the
    pixels that sit on the 0.5 tie and no others"""
    from pgdvs_amd import ops

    raw_no_warp, prev = op_inputs(fx, "A", 3)
    n_pix, n_overlap, selected = segment_reference(fx, "A", 3)
    out = ops.mask_combine(raw_no_warp, dev(sam_of(fx, "A", 3)), img_idx=3, want_segments=True, sam_overlap_thres=0.09,
                           dyn_track_thres=float(np.nextafter(np.float32(0.5), np.float32(0))), **prev)
    assert np.array_equal(host(out["seg_counts"])[:, 0], n_pix)
    want = (n_overlap > 0) & (n_overlap > 0.09 * n_pix)
    assert (want != selected).sum() >= 3
    ties = (np.abs(fx["A_f3_bwd_coord_diff"]).sum(-1) <= 1.0) & (fx["A_f3_cnt_warp"] / np.float32(4) == np.float32(0.5))
    got = host(out["dyn_track"]).astype(bool)
    assert ties.sum() >= 20 and got[ties].all() and not fx["A_f3_dyn_track"][ties].any()
    assert np.array_equal(got[~ties], fx["A_f3_dyn_track"][~ties])


def synthetic_frames(H, W, n_seg, seed):
    """three frames' inputs: blobs, random rectangles as segments, a smooth flow with an inconsistent band"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for t in range(3):
        raw = ((xs - W * 0.4 - 3 * t) ** 2 + (ys - H * 0.5) ** 2 < (min(H, W) * 0.3) ** 2) | (rng.random((H, W)) < 0.02)
        raw[:, W - 3:] = True
        sam = np.zeros((n_seg, H, W), bool)
        for s in range(n_seg):
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            sam[s, y0:y0 + rng.integers(4, H // 2), x0:x0 + rng.integers(4, W // 2)] = True
        flow = np.stack([2.25 + np.sin(ys / 9.0), -1.5 + np.cos(xs / 11.0)], -1).astype(np.float32)
        cd = np.zeros((H, W, 2), np.float32)
        cd[H // 3:H // 3 + 5] = 0.75
        out.append(dict(mask_flow_epi=raw, mask_sam=sam, bwd_flow=flow, bwd_coord_diff=cd))
    return out


@pytest.mark.parametrize("H,W,n_seg", [(131, 257, 5), (64, 128, 3)])
def test_larger_frames_against_the_host_path(H, W, n_seg):
    from pgdvs_amd.preprocess import combine_masks

    state = {None: (None, None), DEV: (None, None)}
    for t, kw in enumerate(synthetic_frames(H, W, n_seg, seed=H)):
        if t == 0:
            kw = {k: v for k, v in kw.items() if not k.startswith("bwd_")}
        res = {}
        for device in (None, DEV):
            res[device] = combine_masks(mask_type="flow_epi", img_idx=t, device=device, prev_mask_final_raw=state[device][0],
                                        prev_dyn_cnt=state[device][1], **kw)
            state[device] = (res[device]["next_prev"], res[device]["dyn_cnt"])
        for k, want in res[None].items():
            if want is None:
                assert res[DEV][k] is None, (t, k)
            else:
                got = host(res[DEV][k])
                assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (t, k)
        assert res[None]["final"].any() and not res[None]["final"].all()
    assert res[None]["warp_prev"].any() and res[None]["dyn_track"].any()


def test_semantic_mask_op(fx):
    from pgdvs_amd import ops
    from pgdvs_amd.preprocess import DYNAMIC_IDS_ADE20K, DYNAMIC_IDS_COCO

    got = ops.semantic_mask(dev(fx["D_f0_sem_ade20k"]), dev(fx["D_f0_sem_coco"]), DYNAMIC_IDS_ADE20K, DYNAMIC_IDS_COCO)
    for g, key in zip(got, ("ade20k", "coco", "sem")):
        assert g.dtype == torch.uint8 and np.array_equal(host(g).astype(bool), fx[f"D_f0_{key}"]), key


def test_invalid_arguments_return_the_library_error():
    from pgdvs_amd import _lib, ops
    from pgdvs_amd._lib import PgdvsHipError

    lib = _lib.load()
    H, W = 4, 5
    m = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    outs = [torch.zeros((H, W), dtype=torch.uint8, device=DEV).data_ptr() for _ in range(7)]
    cnt, cnt_out = (torch.zeros((H, W), dtype=torch.float32, device=DEV) for _ in range(2))
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    tab = (C.c_float * 128)()

    def call(H=H, W=W, n_seg=0, sam=None, prev=(None, None, None, None), img_idx=0, ws_bytes=4096):
        return lib.pgdvs_mask_combine(m.data_ptr(), sam, n_seg, H, W, *prev, tab, img_idx, 0.5, 0.1, outs[0], outs[1], cnt_out.data_ptr(),
                                      *outs[2:], None, None, ws.data_ptr(), ws_bytes, ops._stream())

    assert call() == 0
    for bad in (dict(H=0), dict(W=0), dict(H=1 << 20), dict(H=1 << 16, W=1 << 16), dict(n_seg=-1), dict(n_seg=65536, sam=m.data_ptr()),
                dict(n_seg=1), dict(img_idx=-1), dict(img_idx=1 << 24), dict(ws_bytes=16),
                dict(prev=(m.data_ptr(), None, None, None)), dict(prev=(m.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 4, cnt.data_ptr()))):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert lib.pgdvs_mask_combine_workspace_bytes(0, 5, 1) == -1 and lib.pgdvs_mask_combine_workspace_bytes(4, 5, 65536) == -1
    assert lib.pgdvs_mask_combine_workspace_bytes(4, 5, 0) > 0
    assert lib.pgdvs_semantic_mask(None, None, 4, 5, None, 0, None, 0, m.data_ptr(), m.data_ptr(), m.data_ptr(), ops._stream()) == -1
    with pytest.raises(PgdvsHipError):
        ops.mask_combine(m, torch.zeros((65536, H, W), dtype=torch.uint8, device=DEV), img_idx=0)
    with pytest.raises(ValueError):
        ops.mask_combine(m, torch.zeros((1, H, W + 1), dtype=torch.uint8, device=DEV), img_idx=0)
    with pytest.raises(ValueError):
        ops.mask_combine(m, torch.zeros((1, H, W), dtype=torch.uint8, device=DEV), prev_mask=m, img_idx=1)


def test_run_masks_device_writes_the_hosts_bytes(fx, tmp_path):
    from pgdvs_amd.preprocess import run_masks

    names = build_tree(fx, tmp_path / "scene", "llff")
    on_host = run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "host", segmenter=stub_segmenter(fx))
    on_dev = run_masks(root_dir=tmp_path / "scene", save_dir=tmp_path / "dev", segmenter=stub_segmenter(fx, as_tensor=dev), device=DEV)
    assert len(on_dev) == len(on_host) == 2 * len(names)
    for a, b in zip(on_host, on_dev):
        assert a.relative_to(tmp_path / "host") == b.relative_to(tmp_path / "dev") and a.read_bytes() == b.read_bytes(), a.name
