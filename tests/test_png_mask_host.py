"""The mask PNG reader without a GPU (``pgdvs_png_decode_host``: the kernels' host emulation, which runs their inflate
core, their byte-unit row filters and their unpack; ``ops.png_parse(kinds=...)``): over the files of tests/png_mask_cases.py the
emulation's image equals ``np.array(PIL.Image.open(f)).astype(np.uint8)``, between guard bytes, at three subsequence sizes,
alone and in one table with RGB and RGBA streams; the refusals on the host side and by the status word; the default ``kinds``,
which refuses every mask file as before; the unpack under the host compiler's address and undefined-behaviour sanitizers, in
a stand-alone program; the fifth image-input keyword's rules; and the loaders on a host store, which are unchanged."""
import io
import itertools
import pathlib
import shutil
import subprocess
import sys
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import png_decode_cases as PC  # noqa: E402
import png_mask_cases as MC  # noqa: E402
import resident_cases as RC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
GUARD = 64


@pytest.mark.parametrize("sub_bytes", [PC.SUB, 8, 256])
def test_emulation_equals_pillow_over_the_cases(sub_bytes):
    from pgdvs_amd import ops

    cases = MC.cases()
    assert len({(MC.pillow(d).shape) for _, d in cases} & {(h, w) for h in MC.HEIGHTS for w in MC.WIDTHS}) >= 8
    results = ops.png_decode_host([d for _, d in cases], sub_bytes=sub_bytes, guard=GUARD, kinds="mask")  # one batch: the table's offsets too
    for (label, data), r in zip(cases, results):
        assert r is not None, (label, ops.png_refusal(data, kinds="mask"))
        assert r["status"] == 0, (label, hex(r["status"]), r["info"])
        want = MC.pillow(data)
        assert r["image"].dtype == np.uint8 and r["image"].shape == want.shape and np.array_equal(r["image"], want), label
        info = ops.png_info(data, kinds="mask")
        assert r["inflated"].size == info["height"] * (1 + -(-info["width"] * info["bit_depth"] // 8)), label


def test_the_cases_are_what_their_labels_say():
    from pgdvs_amd import ops

    cases = dict(MC.cases())
    formats = {(i["palette"], i["bit_depth"]) for i in (ops.png_info(d, kinds="mask") for d in cases.values())}
    assert formats == set(itertools.product((False, True), (1, 2, 4, 8)))
    assert {ops.png_info(d, kinds="mask")["scale"] for lb, d in cases.items() if lb.startswith("grey depth")} == {1, 85, 17}
    assert len(ops.png_info(cases["IDAT in 1-byte chunks"], kinds="mask")["idat"]) > 20
    (stored, fixed, dynamic) = ops.png_decode_host([cases[k] for k in ("level 0: stored blocks", "Z_FIXED: fixed blocks", "level 9: dynamic blocks")], kinds="mask")
    assert all(r["status"] == 0 for r in (stored, fixed, dynamic))
    for r, btype in ((stored, 0), (fixed, 1), (dynamic, 2)):  # the first block's BTYPE, behind the two zlib header bytes
        data = cases[{0: "level 0: stored blocks", 1: "Z_FIXED: fixed blocks", 2: "level 9: dynamic blocks"}[btype]]
        info = ops.png_info(data, kinds="mask")
        z = b"".join(data[o:o + n] for o, n in info["idat"])
        assert (z[2] >> 1) & 3 == btype and zlib.decompress(z) == r["inflated"].tobytes()
    # padding bits that are not zero, every filter type in use
    raw = zlib.decompress(b"".join(cases["grey depth 1 63x7 rows cycling 0..4"][o:o + n] for o, n in
                                   ops.png_info(cases["grey depth 1 63x7 rows cycling 0..4"], kinds="mask")["idat"]))
    assert len(raw) == 63 * 2 and {raw[2 * y] for y in range(63)} == {0, 1, 2, 3, 4} and raw[1] & 1  # (filter 0 on row 0: the byte as packed)
    mono = ops.png_info(cases[f"Pillow 1-bit {MC.MONO[0]}x{MC.MONO[1]}"], kinds="mask")
    assert (mono["height"], mono["width"], mono["bit_depth"]) == (*MC.MONO, 1)


def test_mask_and_colour_streams_share_a_table():
    from pgdvs_amd import ops

    masks, colour = MC.small_cases(), [d for _, d in PC.streams()[:6]]
    datas = [d for pair in itertools.zip_longest([d for _, d in masks], colour) for d in pair if d is not None]
    results = ops.png_decode_host(datas, guard=GUARD, kinds=("colour", "mask"))
    for data, r in zip(datas, results):
        want = np.array(PIL.Image.open(io.BytesIO(data))).astype(np.uint8)
        assert r is not None and r["status"] == 0 and r["image"].shape == want.shape and np.array_equal(r["image"], want)
    assert {r["image"].ndim for r in results} == {2, 3}
    rgb = ops.png_decode_host(datas, channels="rgb", guard=GUARD, kinds=("mask", "colour"))  # (masks keep their one channel)
    assert all(r["status"] == 0 and r["image"].shape[2:] in ((), (3,)) for r in rgb)


def test_host_refusals_come_before_any_decode():
    from pgdvs_amd import ops

    for label, data, word in MC.host_refusals():
        assert ops.png_info(data, kinds="mask") is None, label
        assert word in ops.png_refusal(data, kinds="mask"), (label, ops.png_refusal(data, kinds="mask"))
        assert ops.png_decode_host([data], kinds="mask") == [None], label
        reasons = []
        assert ops.png_decode_batch([data], reject_ok=True, reasons=reasons, kinds="mask") == [None] and word in reasons[0], label  # (no GPU here: none is touched)
        with pytest.raises(ValueError, match="not served"):
            ops.png_decode(data, kinds="mask")
    with pytest.raises(ValueError, match="kinds"):
        ops.png_parse(MC.cases()[0][1], kinds="grey")
    with pytest.raises(ValueError, match="kinds"):
        ops.png_decode_host([MC.cases()[0][1]], kinds=())


def test_status_word_refusals_return_none_under_reject_ok():
    from pgdvs_amd import ops

    cases = MC.device_refusals()
    for sub_bytes in (0, 8):
        for (label, data, bits), r in zip(cases, ops.png_decode_host([d for _, d, _ in cases], sub_bytes=sub_bytes, guard=GUARD, kinds="mask")):
            assert r is not None, (label, ops.png_refusal(data, kinds="mask"))  # the host side serves it: the damage is the stream's
            assert r["status"] & bits and not r["status"] & PC.NOT_SYNCHRONISED, (label, hex(r["status"]))


def test_the_default_kinds_still_refuse_every_mask_file():
    from pgdvs_amd import ops

    for label, data in MC.cases():
        assert ops.png_info(data) is None and "colour type" in ops.png_refusal(data) and "8-bit RGB and RGBA are served" in ops.png_refusal(data), label
        assert ops.png_decode_host([data]) == [None] == ops.png_decode_host([data], kinds="colour"), label
        assert ops.png_decode_batch([data], reject_ok=True) == [None], label
    rgb = PC.streams()[0][1]
    assert ops.png_info(rgb, kinds=("colour", "mask")) == ops.png_info(rgb) and "bit_depth" not in ops.png_info(rgb)  # a colour file's info is what it was


def test_c_entry_argument_checks():
    import ctypes as C

    from pgdvs_amd import _lib

    lib = _lib.load()
    assert C.sizeof(_lib.PngImage) == 56
    table = (_lib.PngImage * 1)()
    t = table[0]
    t.offset, t.size, t.height, t.width, t.channels, t.out_channels, t.bit_depth, t.scale = 64, 12, 3, 9, 1, 1, 2, 85
    need = lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1)
    assert need == 512  # the head of 256, 3 rows of 1 + 3 bytes and the carry row of 3, each padded to 16: 288, to a multiple of 256
    t.height = 64  # 64 * 4 = 256 bytes of rows: 256 + 256 + 16
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == 768
    t.height = 3
    for field, value in (("bit_depth", 3), ("bit_depth", 16), ("scale", 86), ("scale", 0), ("channels", 2), ("width", 16385)):
        keep = getattr(t, field)
        setattr(t, field, value)
        assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == -1, (field, value)
        assert b"pgdvs_png_inflate_workspace_bytes" in lib.pgdvs_last_error()
        setattr(t, field, keep)
    t.channels, t.out_channels, t.bit_depth, t.scale = 3, 3, 4, 1  # colour streams are 8-bit
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == -1
    for gone in ("images_workspace_bytes", "decode_images", "decode_images_host"):  # the second table's entry points went with it
        assert not hasattr(lib, f"pgdvs_png_{gone}") and f"pgdvs_png_{gone}" not in _lib.SIGNATURES, gone
    assert {n for n in _lib.SIGNATURES if n.startswith("pgdvs_png_") and ("inflate" in n or "decode" in n)} == {
        "pgdvs_png_inflate_workspace_bytes", "pgdvs_png_decode", "pgdvs_png_decode_host"}
    buf = np.zeros(64, np.uint64)
    st = np.zeros(2, np.uint32)
    ptr = C.c_void_p(buf.ctypes.data)
    assert lib.pgdvs_png_decode_host(ptr, ptr, 512, 1, 0, C.c_void_p(st.ctypes.data), ptr, 512) == -1
    assert b"pgdvs_png_decode_host" in lib.pgdvs_last_error()


# ---------------------------------------------------------------------------- the sanitizers, on a stand-alone program
def test_the_unpack_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "png_mask_fuzz"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")  # does this compiler have the sanitizers at all?
    probe = subprocess.run([cxx, *flags, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} lacks the address / undefined sanitizers: {(probe.stderr.strip().splitlines() or ['the probe does not run'])[-1]}")
    built = subprocess.run([cxx, *flags, str(ROOT / "tools" / "png_mask_fuzz.cpp"), str(ROOT / "ml-pgdvs_amd" / "csrc" / "png_decode_host.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr  # (with the sanitizers there, a failure here is the driver's or the source's)
    files = {**MC.fuzz_files(), **{f"case{k}.png": d for k, (_, d) in enumerate(MC.small_cases())}}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    mutations = 60  # per file: some hundreds in all
    run = subprocess.run([str(exe), "20261021", str(mutations), *(str(tmp_path / n) for n in files)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(files) and all("failures 0" in ln for ln in lines), run.stdout
    total = 0
    for ln in lines:
        decoded, given_up = (int(ln.split(word)[1].split(",")[0]) for word in ("decoded ", "given up "))
        assert decoded + given_up == 1 + mutations and decoded >= 1, ln
        total += given_up
    assert total > len(files) * mutations // 2 and (1 + mutations) * len(files) > 300  # the damage reaches the decode


# ---------------------------------------------------------------------------- the keyword
FLAGS = ("resize", "decode", "entropy", "png", "mask")


def missing(resize, decode, entropy, png, mask, resident, device):
    """what the first broken rule asks for, or None: the rules in their order of precedence"""
    rules = ((entropy and not decode, "device_decode=True"),
             (png and not resize, "device_resize=True"),
             (mask and not resize, "device_resize=True"),
             (decode and not resize, "device_resize=True"),
             (resize and not resident, "resident=True"),
             (resize and (device is None or torch.device(device).type != "cuda"), "GPU"))
    return next((what for broken, what in rules if broken), None)


def test_the_truth_table_with_the_fifth_flag():
    from pgdvs_amd.datasets._common import device_input
    from pgdvs_amd.datasets.resident import SceneStore

    for flags in itertools.product((False, True), repeat=5):
        for resident, device in itertools.product((False, True), (None, "cpu", "cuda:0")):
            kw = dict(resident=resident, device=device, **{f"device_{n}": v for n, v in zip(FLAGS, flags)})
            want = missing(*flags, resident, device)
            if want is None:
                got = device_input("Loader", **kw)
                assert tuple(got) == flags and got.mask is flags[4] and all(type(v) is bool for v in got), (flags, resident, device)
            else:
                with pytest.raises(ValueError, match=want) as err:
                    device_input("Loader", **kw)
                assert str(err.value).startswith("Loader(device_"), (flags, resident, device, str(err.value))
        if missing(*flags, True, "cuda:0") is None:
            store = SceneStore("cuda:0", **{f"device_{n}": v for n, v in zip(FLAGS, flags)})
            assert (store.device_resize, store.device_decode, store.device_entropy, store.device_png, store.device_mask) == flags
            assert ("masks_decoded_on_device" in store.stats) == ("mask_fallbacks" in store.stats) == flags[4]  # (the record is the old one without it)
    with pytest.raises(ValueError, match="device_mask=True.*device_resize=True"):
        SceneStore(device="cuda:0", device_mask=True)  # (refused in front of any device work)
    with pytest.raises(ValueError, match="device_mask=True.*device_resize=True"):
        device_input("Loader", resident=True, device="cuda:0", device_mask=True, device_decode=True)  # (in front of device_decode's rule)


def test_a_host_store_reads_masks_with_the_host_statement(tmp_path):
    from pgdvs_amd.datasets.resident import SceneStore

    store = SceneStore()
    assert not store.device_mask and "mask_fallbacks" not in store.stats
    store.prefetch_images([], masks=[("/nonexistent.png", (4, 4), None)])  # off: nothing is opened
    for k, (label, data) in enumerate(MC.small_cases(5)):
        path = tmp_path / f"{k}.png"
        path.write_bytes(data)
        want = np.array(PIL.Image.open(path))
        got = store.decode_mask(path)
        assert got.dtype == want.dtype and np.array_equal(got, want), label
        small = store.decode_mask(path, (3, 5))
        assert np.array_equal(small, np.array(PIL.Image.fromarray(want).resize((5, 3), resample=PIL.Image.Resampling.NEAREST))), label


@pytest.mark.parametrize("name", RC.LOADERS)
def test_loaders_refuse_the_keyword_without_device_resize_and_are_unchanged_on_a_host_store(name, tmp_path):
    trees = RC.build_trees(tmp_path)
    with pytest.raises(ValueError, match="device_mask=True.*device_resize=True"):
        RC.make(name, trees, resident=True, device_mask=True, **({} if name == "nvidia_pure_geo" else {"device": None}))
    if name == "nvidia_pure_geo":
        return  # (builds its cloud on a GPU)
    want, got = RC.make(name, trees), RC.make(name, trees, resident=True)
    for i in (0, len(want) - 1):
        RC.assert_items_equal(got[i], want[i], (name, i))
    assert not got.store.device_mask and len(got.store.stats) == 13


def test_dycheck_loader_refuses_the_keyword_and_is_unchanged_on_a_host_store(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
              scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
              flow_consist_thres=1.0)
    with pytest.raises(ValueError, match="device_mask=True.*device_resize=True"):
        DyCheckiPhoneEvaluationDataset(**kw, resident=True, device_mask=True)
    want, got = DyCheckiPhoneEvaluationDataset(**kw), DyCheckiPhoneEvaluationDataset(**kw, resident=True)
    for i in (0, len(want) - 1):
        RC.assert_items_equal(got[i], want[i], i)
    p = got.parser_dict[DT.SCENE]
    t, c = int(got.valid_fs[0][2]), int(got.valid_fs[0][3])
    assert np.array_equal(p.load_covisible(t, c, "val"), np.array(PIL.Image.open(p.covisible_path(t, c, "val"))))
    pathlib.Path(p.covisible_path(t, c, "val")).unlink()
    with pytest.raises(ValueError, match="Covisible image not found"):
        p.load_covisible(t, c, "val")
