"""The PNG reader without a GPU (csrc/png_inflate_core.h through ``pgdvs_png_decode_host``, the kernels' host emulation;
``ops.png_info``): over the streams of tests/png_decode_cases.py the emulation's inflated bytes equal ``zlib.decompress`` and its
image Pillow's array, between guard bytes, at three subsequence sizes; every refusal of the contract, on the host side and by
the status word, and every damaged file gives what Pillow gives because the file falls back; the same under the host
compiler's address and undefined-behaviour sanitizers, in a stand-alone program; the keyword rules; and the loaders on a host
store, which are unchanged."""
import pathlib
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import png_decode_cases as PC  # noqa: E402
import resident_cases as RC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
GUARD = 64


def _same_as_pillow(got, want, label):
    if isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want), label
    else:
        assert got is want, (label, got, want)


def served_or_pillow(data, sub_bytes=0, channels="file"):
    """what a caller of the device path ends with, on the emulation: its image at status 0, else Pillow's answer"""
    from pgdvs_amd import ops

    (r,) = ops.png_decode_host([data], channels=channels, sub_bytes=sub_bytes, guard=GUARD)
    if r is not None and r["status"] == 0:
        return r["image"], True
    want = PC.pillow(data)
    return (want[..., :3] if channels == "rgb" and isinstance(want, np.ndarray) and want.ndim == 3 else want), False


@pytest.mark.parametrize("sub_bytes", [PC.SUB, 8, 256])
def test_emulation_equals_zlib_and_pillow_over_the_streams(sub_bytes):
    from pgdvs_amd import ops

    streams = PC.streams()
    results = ops.png_decode_host([d for _, d in streams], sub_bytes=sub_bytes, guard=GUARD)  # one batch: the table's offsets too
    for (label, data), r in zip(streams, results):
        assert r is not None, (label, ops.png_refusal(data))
        assert r["status"] == 0, (label, hex(r["status"]), r["info"])
        h, w, c, z = PC.split(data)
        assert r["inflated"].tobytes() == zlib.decompress(z), label
        _same_as_pillow(r["image"], PC.pillow(data), label)
    by_label = dict(zip((lb for lb, _ in streams), results))
    if sub_bytes == PC.SUB:  # the cases are what their labels say
        assert by_label["128x128 noise: several windows"]["info"][3] >= 2  # stored blocks: zlib gives noise up
        assert by_label["length 258 at distance 32768 and at distance 1"]["info"][0] >= 2
        assert by_label["a block ends in a window's first and one in its last subsequence"]["info"] == (3, 4, 1, 2)
        assert by_label["Z_SYNC_FLUSH after every row: short blocks, empty stored blocks"]["info"][3] > 100
        assert max(r["info"][1] for r in results) <= PC.TEAM and max(r["info"][2] for r in results) <= PC.TEAM


def test_rgb_of_rgba_files():
    from pgdvs_amd import ops

    streams = [(lb, d) for lb, d in PC.streams() if PC.split(d)[2] == 4]
    assert len(streams) > 8
    for (label, data), r in zip(streams, ops.png_decode_host([d for _, d in streams], channels="rgb", guard=GUARD)):
        assert r["status"] == 0 and np.array_equal(r["image"], PC.pillow(data)[..., :3]), label


def test_host_refusals_come_before_any_device_work():
    from pgdvs_amd import ops

    for label, data, word in PC.host_refusals():
        assert ops.png_info(data) is None, label
        assert word in ops.png_refusal(data), (label, ops.png_refusal(data))
        reasons = []
        assert ops.png_decode_batch([data], reject_ok=True, reasons=reasons) == [None] and word in reasons[0], label  # (no GPU here: none is touched)
        with pytest.raises(ValueError, match="not served"):
            ops.png_decode(data)
        got, served = served_or_pillow(data)
        assert not served
        _same_as_pillow(got, PC.pillow(data), label)
    info = ops.png_info(PC.streams()[0][1])
    assert (info["width"], info["height"], info["channels"]) == (1, 1, 3) and info["stream_bytes"] == sum(n for _, n in info["idat"])
    with pytest.raises(ValueError, match="channels"):
        ops.png_decode(PC.streams()[0][1], channels="rgba")


def test_status_word_refusals_fall_back_to_pillow():
    from pgdvs_amd import ops

    cases = PC.device_refusals()
    for sub_bytes in (0, 8):
        for (label, data, bits), r in zip(cases, ops.png_decode_host([d for _, d, _ in cases], sub_bytes=sub_bytes, guard=GUARD)):
            assert r is not None, (label, ops.png_refusal(data))  # the host side serves it: the damage is the stream's
            assert r["status"] & bits and not r["status"] & PC.NOT_SYNCHRONISED, (label, hex(r["status"]))
            got, served = served_or_pillow(data, sub_bytes)
            assert not served
            _same_as_pillow(got, PC.pillow(data), label)


def test_every_truncation_gives_what_pillow_gives():
    from pgdvs_amd import ops

    for name, data in PC.fuzz_files().items():
        for n in range(len(data)):  # of the file: the chunk walk refuses every one, and the caller ends with Pillow's answer
            assert ops.png_info(data[:n]) is None, (name, n)
            got, served = served_or_pillow(data[:n])
            assert not served
            _same_as_pillow(got, PC.pillow(data[:n]), (name, n))
        cut = list(PC.stream_truncations(data))  # of the stream, the chunks whole again: the inflate runs out of data
        for n, (bad, r) in enumerate(zip(cut, ops.png_decode_host(cut, guard=GUARD))):
            assert r is None or (r["status"] != 0 and not r["status"] & PC.NOT_SYNCHRONISED), (name, n, r and hex(r["status"]))
            _same_as_pillow(served_or_pillow(bad)[0], PC.pillow(bad), (name, n))


def test_4000_mutations_give_what_pillow_gives():
    from pgdvs_amd import ops

    seen = {"served": 0, "refused on the host": 0, "given up": 0}
    files = list(PC.fuzz_files().items())
    for k, (name, data) in enumerate(files):
        rng = np.random.default_rng(20261021 + k)
        whole = [data[:a] + bytes([v]) + data[a + 1:] for a, v in zip(rng.integers(0, len(data), 667).tolist(), rng.integers(0, 256, 667).tolist())]
        variants = whole + list(PC.stream_mutations(data, 667, 20261021 + k))
        for m, (bad, sub_bytes) in enumerate(zip(variants, (0, 8) * len(variants))):
            (r,) = ops.png_decode_host([bad], sub_bytes=sub_bytes, guard=GUARD)
            if r is None:
                seen["refused on the host"] += 1
            elif r["status"]:
                assert not r["status"] & PC.NOT_SYNCHRONISED, (name, m, hex(r["status"]))
                seen["given up"] += 1
            else:  # served: Pillow must open it, to the same bytes
                seen["served"] += 1
                _same_as_pillow(r["image"], PC.pillow(bad), (name, m))
    assert sum(seen.values()) == 4002 and seen["served"] > 20 and seen["refused on the host"] > 1500 and seen["given up"] > 1500, seen


def test_c_entry_argument_checks():
    import ctypes as C

    from pgdvs_amd import _lib

    lib = _lib.load()
    table = (_lib.PngImage * 1)()
    table[0].offset, table[0].size, table[0].height, table[0].width, table[0].channels, table[0].out_channels = 64, 12, 1, 1, 3, 3
    table[0].bit_depth, table[0].scale = 8, 1
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) > 0
    for field in ("bit_depth", "scale"):  # a colour entry states its depth and scale
        keep = getattr(table[0], field)
        setattr(table[0], field, 0)
        assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == -1, field
        assert b"colour streams have bit depth 8 and scale 1" in lib.pgdvs_last_error(), field
        setattr(table[0], field, keep)
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) > 0
    table[0].channels = 2
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == -1
    table[0].channels, table[0].width = 3, 16385
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 1) == -1
    assert lib.pgdvs_png_inflate_workspace_bytes(C.byref(table), 0) == -1
    buf = np.zeros(64, np.uint64)
    st = np.zeros(2, np.uint32)
    ptr = C.c_void_p(buf.ctypes.data)
    # an empty table, a stream outside the buffer, a subsequence size out of range: -1, nothing decoded
    assert lib.pgdvs_png_decode_host(ptr, ptr, 512, 1, 0, C.c_void_p(st.ctypes.data), ptr, 512) == -1
    assert b"pgdvs_png_decode_host" in lib.pgdvs_last_error()


# ---------------------------------------------------------------------------- the sanitizers, on a stand-alone program
def test_the_inflate_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "png_inflate_fuzz"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")  # does this compiler have the sanitizers at all?
    probe = subprocess.run([cxx, *flags, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} lacks the address / undefined sanitizers: {(probe.stderr.strip().splitlines() or ['the probe does not run'])[-1]}")
    built = subprocess.run([cxx, *flags, str(ROOT / "tools" / "png_inflate_fuzz.cpp"), str(ROOT / "ml-pgdvs_amd" / "csrc" / "png_decode_host.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr  # (with the sanitizers there, a failure here is the driver's or the source's)
    files = PC.fuzz_files()
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    run = subprocess.run([str(exe), "20261021", "1334", *(str(tmp_path / n) for n in files)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 3 and all("failures 0" in ln for ln in lines), run.stdout
    for ln, data in zip(lines, files.values()):  # the stream, its truncations from 6 bytes on, the mutations
        n = len(PC.split(data)[3])
        decoded, given_up = (int(ln.split(word)[1].split(",")[0]) for word in ("decoded ", "given up "))
        assert decoded + given_up == 1 + (n - 6) + 1334 and decoded >= 1 and given_up >= n - 6, ln


# ---------------------------------------------------------------------------- the keyword
def test_device_png_needs_device_resize():
    from pgdvs_amd.datasets._common import device_input
    from pgdvs_amd.datasets.resident import SceneStore

    def png_option(device_png, device_resize, owner):
        return device_input(owner, resident=True, device="cuda:0", device_resize=device_resize, device_png=device_png).png

    with pytest.raises(ValueError, match="device_png=True.*device_resize=True"):
        SceneStore(device="cuda:0", device_png=True)  # (refused in front of any device work)
    with pytest.raises(ValueError, match="device_png=True.*device_resize=True"):
        png_option(True, False, "Loader")
    assert png_option(False, False, "Loader") is False and png_option(True, True, "Loader") is True
    store = SceneStore()
    assert not store.device_png and store.stats["png_decoded_on_device"] == store.stats["png_fallbacks"] == 0
    store.prefetch_images(["/nonexistent.png"])  # off: nothing is opened


@pytest.mark.parametrize("name", RC.LOADERS)
def test_loaders_refuse_the_keyword_without_device_resize_and_are_unchanged_on_a_host_store(name, tmp_path):
    trees = RC.build_trees(tmp_path)
    with pytest.raises(ValueError, match="device_png=True.*device_resize=True"):
        RC.make(name, trees, resident=True, device_png=True, **({} if name == "nvidia_pure_geo" else {"device": None}))
    if name == "nvidia_pure_geo":
        return  # (builds its cloud on a GPU)
    want, got = RC.make(name, trees), RC.make(name, trees, resident=True)
    for i in (0, len(want) - 1):
        RC.assert_items_equal(got[i], want[i], (name, i))
    assert got.store.stats["png_decoded_on_device"] == got.store.stats["png_fallbacks"] == 0


def test_dycheck_loader_refuses_the_keyword_and_is_unchanged_on_a_host_store(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1, mode="eval",
              scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3, n_src_views_temporal_track_one_side=2,
              flow_consist_thres=1.0)
    with pytest.raises(ValueError, match="device_png=True.*device_resize=True"):
        DyCheckiPhoneEvaluationDataset(**kw, resident=True, device_png=True)
    want, got = DyCheckiPhoneEvaluationDataset(**kw), DyCheckiPhoneEvaluationDataset(**kw, resident=True)
    for i in (0, len(want) - 1):
        RC.assert_items_equal(got[i], want[i], i)
    p = got.parser_dict[DT.SCENE]
    t, c = int(got.train_info_dict[DT.SCENE]["time_ids"][0]), got.get_train_cam_id(DT.SCENE)
    assert np.array_equal(got.store.decode_image(p.rgb_path(t, c), channels="rgb"), p.load_rgba(t, c)[..., :3])
