"""The device resize's host side (csrc/resample.hip ``pgdvs_resample_table``; the loaders' ``device_resize`` keyword): the
coefficient tables, run through a numpy statement of the two integer passes, give Pillow's BOX and LANCZOS resize byte for
byte; sizes and filters outside the limits are refused with -1 and a message; the keyword is refused without
``resident=True`` and with a host store."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import resample_cases as RS  # noqa: E402
import resident_cases as RC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("filter", sorted(RS.FILTERS))
def test_tables_and_two_integer_passes_equal_pillow(filter):
    n = 0
    for in_hw, out_hw in RS.SHAPES + RS.random_pairs():
        for c in (1, 3):
            for kind in ("random", "checker", "white"):
                a = RS.content(kind, *in_hw, c)
                got, want = RS.two_passes(a, out_hw, filter), RS.pil_resize(a, out_hw, filter)
                assert got.shape == want.shape and got.dtype == want.dtype
                assert np.array_equal(got, want), (in_hw, out_hw, c, kind, int((got != want).sum()))
                n += 1
    assert n == (len(RS.SHAPES) + 60) * 6


def test_the_table_of_the_workload():
    """1080 -> 288: ratio 3.75, 5 BOX taps and 25 LANCZOS taps; every row's coefficients sum to 2^22 within the rounding of its
    taps, zero past the row's count, and nothing outside the arrays is written"""
    for filter, ksize in (("box", 5), ("lanczos", 25)):
        bounds, kk = RS.table(1080, 288, filter)
        assert bounds.shape == (288, 2) and kk.shape == (288, ksize) and kk.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 1080).all() and (bounds[:, 1] >= 1).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()
        for row, (_, n) in zip(kk, bounds):
            assert (row[n:] == 0).all() and abs(int(row.sum()) - (1 << 22)) <= n
    bounds, kk = RS.table(288, 288, "lanczos")  # an axis that keeps its size still has its (identity) table
    assert kk.shape == (288, 7) and (kk[np.arange(288), np.argmax(kk, 1)] == 1 << 22).all()


def test_the_table_entry_refuses_with_a_message():
    for n_in, n_out, filter, word in ((0, 4, "box", "pixels"), (4, 0, "box", "pixels"), (16385, 4, "box", "16384"), (4, 16385, "lanczos", "16384"),
                                      (-3, 4, "box", "pixels"), (8, 4, 2, "filter"), (8, 4, -1, "filter"),
                                      (16384, 1, "box", "taps"), (4300, 100, "lanczos", "taps"), (5120, 20, "box", "taps")):
        rc, msg = RS.table(n_in, n_out, filter)
        assert rc == -1 and word in msg, (n_in, n_out, filter, rc, msg)
    # the last sizes inside the limit of 256 taps: a lanczos reduction of 42 : 1, a box reduction of 254 : 1
    assert RS.table(4200, 100, "lanczos")[1].shape == (100, 253) and RS.table(5080, 20, "box")[1].shape == (20, 255)
    from pgdvs_amd import _lib

    lib = _lib.load()
    assert lib.pgdvs_resample_table(8, 4, 0, np.zeros(8, np.int32).ctypes.data, None) == -1  # one array without the other
    assert b"go together" in lib.pgdvs_last_error()
    # the op's workspace query: host only
    assert lib.pgdvs_resample_u8_workspace_bytes(1, 1080, 2062, 3, 288, 550, 0) == 1080 * 1652
    assert lib.pgdvs_resample_u8_workspace_bytes(3, 64, 64, 1, 64, 17, 1) == 0 and lib.pgdvs_resample_u8_workspace_bytes(1, 8, 8, 3, 8, 8, 0) == 0
    for bad in ((0, 8, 8, 3, 4, 4, 0), (1, 8, 8, 2, 4, 4, 0), (1, 8, 8, 4, 4, 4, 0), (1, 8, 20000, 3, 4, 4, 0), (1, 8, 8, 3, 4, 4, 5),
                (70000, 8, 8, 3, 4, 4, 0), (1, 16384, 8, 3, 1, 4, 1)):
        assert lib.pgdvs_resample_u8_workspace_bytes(*bad) == -1 and lib.pgdvs_last_error(), bad


def test_sources_are_listed():
    assert "resample.hip" in (ROOT / "ml-pgdvs_amd" / "csrc" / "Makefile").read_text()
    from pgdvs_amd import _lib, ops

    assert {"pgdvs_resample_table", "pgdvs_resample_u8", "pgdvs_resample_u8_workspace_bytes"} <= set(_lib.SIGNATURES)
    with pytest.raises(ValueError):
        ops.resample_plan((8, 8), (4, 4), "box", "cpu")  # the tables live on a GPU
    with pytest.raises(ValueError):
        ops.resample_plan((8, 8), (4, 4), "nearest", "cuda:0")
    import torch

    with pytest.raises(ValueError):
        ops.resample_u8(torch.zeros((8, 8, 3), dtype=torch.uint8), (4, 4), "box")  # a CPU tensor


# ---------------------------------------------------------------------------- the loaders' keyword
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("resample_host"))


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_resize_needs_a_resident_gpu_store(name, trees):
    """refused in the constructor, in front of everything else it does (the pure-geometry loader's aggregation needs a GPU)"""
    with pytest.raises(ValueError, match="resident=True"):
        RC.make(name, trees, device_resize=True)
    with pytest.raises(ValueError, match="resident=True"):
        RC.make(name, trees, device_resize=True, device="cuda:0")
    with pytest.raises(ValueError, match="GPU"):
        RC.make(name, trees, device_resize=True, resident=True, device=None)
    if name != "nvidia_pure_geo":
        ds = RC.make(name, trees, resident=True, device=None)  # the default: off, and the store counts no device resize
        assert ds.store.device_resize is False and ds.store.stats["frames_resized_on_device"] == 0


def test_device_resize_needs_a_resident_gpu_store_dycheck(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1,
              mode="eval", scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3,
              n_src_views_temporal_track_one_side=2)
    with pytest.raises(ValueError, match="resident=True"):
        DyCheckiPhoneEvaluationDataset(**kw, device_resize=True)
    with pytest.raises(ValueError, match="GPU"):
        DyCheckiPhoneEvaluationDataset(**kw, device_resize=True, resident=True)
    assert DyCheckiPhoneEvaluationDataset(**kw, resident=True).store.device_resize is False
