"""The JPEG scan read in subsequences, on the host (csrc/jpeg_scan_core.h through ``pgdvs_jpeg_scan_prepare`` and the kernels'
emulation ``pgdvs_jpeg_scan_decode_host`` of csrc/jpeg_entropy.cpp; the loaders' ``device_entropy`` keyword): the emulation
gives ``pgdvs_jpeg_entropy_decode``'s coefficients bit for bit, with status 0, over the whole stream matrix of
tests/jpeg_decode_cases.py and the streams tests/jpeg_scan_cases.py adds -- none falls back, none reports "not synchronised";
damaged streams (every truncation, a flipped RSTn, 2000 seeded mutations of three streams) are refused wherever the host
decoder refuses them and nothing is written outside the buffers; the preparation refuses what the parser refuses and a scan
above the cap; the same under the host compiler's address and undefined-behaviour sanitizers, in a stand-alone program; and
the keyword is refused without ``device_decode=True``."""
import ctypes as C
import pathlib
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
import jpeg_decode_cases as JC  # noqa: E402
import jpeg_scan_cases as SC  # noqa: E402
import resident_cases as RC  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module", autouse=True)
def _turbo():
    JC.require_turbo()


def test_constants_are_the_headers():
    from pgdvs_amd import _lib, ops

    text = (ROOT / "include" / "pgdvs_hip.h").read_text()
    assert f"#define PGDVS_JPEG_SCAN_SUB_BYTES {SC.SUB}\n" in text and "#define PGDVS_JPEG_SCAN_MAX_BYTES (1 << 25)\n" in text
    assert (ops.JPEG_SCAN_SUB_BYTES, ops.JPEG_SCAN_MAX_BYTES) == (SC.SUB, SC.CAP)
    for name, bit in (("SHORT", SC.SHORT), ("BAD_CODE", SC.BAD_CODE), ("DC_RANGE", SC.DC_RANGE), ("NOT_SYNCHRONISED", SC.NOT_SYNCHRONISED),
                      ("LEFT_OVER", SC.LEFT_OVER)):
        assert f"#define PGDVS_JPEG_SCAN_{name} {bit}\n" in text
    make = (ROOT / "ml-pgdvs_amd" / "csrc" / "Makefile").read_text()
    assert "jpeg_scan_decode.hip" in make and "jpeg_scan_core.h" in make
    assert {"pgdvs_jpeg_scan_prepare_bytes", "pgdvs_jpeg_scan_prepare", "pgdvs_jpeg_scan_decode_workspace_bytes", "pgdvs_jpeg_scan_decode",
            "pgdvs_jpeg_scan_decode_host"} <= set(_lib.SIGNATURES)
    rc, prepared, info, msg = SC.prepare(JC.small_stream())
    assert rc == 0, msg
    hd = SC.header(prepared)
    assert hd.magic == 0x314E4353 and hd.total_bytes == prepared.size and hd.sub_bytes == SC.SUB and hd.coef_bytes == info.coef_bytes
    assert hd.off_quant % 16 == 0 and np.array_equal(prepared[hd.off_quant:hd.off_quant + 384].view(np.uint16).reshape(3, 64),
                                                     np.ctypeslib.as_array(info.quant))


@pytest.mark.parametrize("subsampling", JC.SUBSAMPLINGS)
def test_emulation_equals_the_host_decoder_over_the_matrix(subsampling):
    """status 0 and the same int16 array for every stream: the share of intact streams that falls back is zero"""
    n = 0
    for label, data in JC.matrix(subsampling):
        status, rounds = SC.check_against_host_decoder(label, data)
        assert status == 0 and 1 <= rounds[0] <= SC.GROUP + 1, (label, status, rounds)
        n += 1
    assert n == len(JC.SIZES) * 12 + 6 + (9 if subsampling != 1 else 0)


def test_emulation_equals_the_host_decoder_on_the_added_streams():
    seen = {}
    for label, data in SC.added():
        status, rounds = SC.check_against_host_decoder(label, data)
        assert status == 0, (label, status)
        rc, prepared, info, _ = SC.prepare(data)
        seen[label] = (SC.header(prepared), info, rounds)
    assert seen["1x1"][0].nsub == seen["8x8"][0].nsub == 1 and seen["8x8"][0].stream_bytes < SC.SUB
    for label, n, subs in (("one subsequence", SC.SUB, 1), ("two subsequences less one byte", 2 * SC.SUB - 1, 2),
                           ("two subsequences and one byte", 2 * SC.SUB + 1, 3)):
        hd = seen[f"scan of exactly {label}"][0]
        assert (hd.stream_bytes, hd.nsub, hd.nseg) == (n, subs, 1), (label, hd.stream_bytes, hd.nsub)
    hd, info, rounds = seen["256x384 noise q100 4:4:4: more than two workgroups"]
    assert hd.nsub > 2 * SC.GROUP and (info.width, info.height, info.sampling) == (384, 256, 0) and rounds[1] >= 1  # a fix-up launch ran
    hd, info, _ = seen["restart interval 1"]
    assert info.restart_interval == 1 and hd.nseg == hd.mcus_w * hd.mcus_h == 12 and hd.nsub >= hd.nseg
    hd, info, _ = seen["restart interval larger than the image"]
    assert info.restart_interval == 1000 > hd.mcus_w * hd.mcus_h and hd.nseg == 1
    hd, info, _ = seen["smooth: almost every block is EOB"]
    assert info.coef_bytes // 128 > 50 * hd.nsub  # many blocks fall in each subsequence


def test_every_subsequence_size_gives_the_same_coefficients():
    """the sizes the entry takes, from the smallest (a symbol with its extra bits spans a quarter of it) to the largest"""
    add = dict(SC.added())
    picks = [JC.matrix(0)[-1], JC.matrix(2)[50], ("noise", add["noise q100: blocks end on coefficient 63"]), ("rst 1", add["restart interval 1"])]
    for label, data in picks:
        for sub in (16, 20, 64, 256, 4096):
            status, _ = SC.check_against_host_decoder(f"{label} @ {sub}", data, sub)
            assert status == 0
    from pgdvs_amd import _lib

    lib, buf = _lib.load(), np.frombuffer(JC.small_stream(), np.uint8)
    for bad in (8, 18, 4100, -4):
        assert lib.pgdvs_jpeg_scan_prepare_bytes(C.c_void_p(buf.ctypes.data), buf.size, bad) == -1 and b"sub_bytes" in lib.pgdvs_last_error()


# ---------------------------------------------------------------------------- damaged streams
def test_every_truncation_is_refused_by_the_preparation():
    data = JC.small_stream()
    for n in range(len(data)):
        assert SC.check_against_host_decoder(f"first {n} bytes", data[:n], intact=False) == (None, None)


def test_a_flipped_restart_marker_is_refused_by_the_preparation():
    data = dict(JC.refusals())["flipped RSTn"]
    assert JC.parse(data)[0] == 0
    rc, prepared, _, msg = SC.prepare(data)
    assert rc == 1 and prepared is None and "restart marker" in msg


def test_mutations_never_pass_where_the_host_decoder_refuses():
    """2000 single-byte mutations of three streams: the emulation is non-zero wherever the host decoder returns 1, equal to it
    wherever both serve, and writes nothing outside its buffers (the guard words of tests/jpeg_scan_cases.py)"""
    seen = {"decoded": 0, "refused": 0, "corrupt": 0}
    for k, (name, data) in enumerate(SC.fuzz_streams().items()):
        for m, bad in enumerate(SC.mutations(data, 2000, 20261021 + k)):
            status, _ = SC.check_against_host_decoder(f"{name} mutation {m}", bad, sub_bytes=(0, 16)[m & 1], intact=False)
            seen["refused" if status is None else ("decoded" if status == 0 else "corrupt")] += 1
    assert seen["decoded"] > 500 and seen["refused"] > 500 and seen["corrupt"] > 100, seen


def test_preparation_refuses_what_the_parser_refuses_and_an_oversized_scan():
    for label, data in JC.refusals():
        if label == "4:1:1":  # Pillow's old name of 4:2:0: served
            assert SC.check_against_host_decoder(label, data)[0] == 0
            continue
        rc_p, _, msg_p = JC.parse(data)
        rc, prepared, info, msg = SC.prepare(data)
        assert rc == 1 and prepared is None and msg.startswith("jpeg: "), (label, rc, msg)
        assert (rc_p == 1 and msg == msg_p) or label == "flipped RSTn", (label, msg, msg_p)
    big = SC.oversized()
    rc_p, info, _ = JC.parse(big)
    assert rc_p == 0  # the parser and the host decoder serve it
    rc, prepared, _, msg = SC.prepare(big)
    assert rc == 1 and prepared is None and "PGDVS_JPEG_SCAN_MAX_BYTES" in msg
    at_cap = big[:-3] + big[-2:]  # one byte less: served
    from pgdvs_amd import _lib

    buf = np.frombuffer(at_cap, np.uint8)
    assert 0 < _lib.load().pgdvs_jpeg_scan_prepare_bytes(C.c_void_p(buf.ctypes.data), buf.size, 0) < 1 << 31


def test_argument_errors_return_minus_one():
    from pgdvs_amd import _lib

    lib, data = _lib.load(), np.frombuffer(JC.small_stream(), np.uint8)
    ptr, info = C.c_void_p(data.ctypes.data), _lib.JpegInfo()
    need = lib.pgdvs_jpeg_scan_prepare_bytes(ptr, data.size, 0)
    mem = np.zeros(need + 16, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 8
    assert lib.pgdvs_jpeg_scan_prepare_bytes(None, 5, 0) == -1 and lib.pgdvs_jpeg_scan_prepare_bytes(ptr, -1, 0) == -1
    assert lib.pgdvs_jpeg_scan_prepare(ptr, data.size, 0, None, need, C.byref(info)) == -1
    assert lib.pgdvs_jpeg_scan_prepare(ptr, data.size, 0, C.c_void_p(base), need, None) == -1
    assert lib.pgdvs_jpeg_scan_prepare(ptr, data.size, 0, C.c_void_p(base + 1), need, C.byref(info)) == -1
    assert lib.pgdvs_jpeg_scan_prepare(ptr, data.size, 0, C.c_void_p(base), need - 8, C.byref(info)) == -1 and b"takes" in lib.pgdvs_last_error()
    assert not mem.any()
    assert lib.pgdvs_jpeg_scan_prepare(ptr, data.size, 0, C.c_void_p(base), need, C.byref(info)) == 0
    p = C.c_void_p(base)
    ws_need = lib.pgdvs_jpeg_scan_decode_workspace_bytes(p, need)
    assert ws_need > 0 and ws_need % 256 == 0 and lib.pgdvs_jpeg_scan_decode_workspace_bytes(p, need - 8) == -1
    assert lib.pgdvs_jpeg_scan_decode_workspace_bytes(None, need) == -1
    coef, ws, status = np.zeros(info.coef_bytes // 2, np.int16), np.zeros(ws_need // 8, np.uint64), np.zeros(1, np.uint32)
    args = lambda **kw: [kw.get("p", p), kw.get("p", p), kw.get("n", need), C.c_void_p(coef.ctypes.data), kw.get("cb", info.coef_bytes),  # noqa: E731
                         C.c_void_p(status.ctypes.data), C.c_void_p(ws.ctypes.data), kw.get("wb", ws_need)]
    for kw, word in (({"cb": info.coef_bytes - 128}, "coef_bytes"), ({"wb": ws_need - 256}, "workspace"), ({"n": need - 8}, "shorter")):
        assert lib.pgdvs_jpeg_scan_decode_host(*args(**kw)) == -1 and word.encode() in lib.pgdvs_last_error(), word
    mem[base - mem.ctypes.data] ^= 0xFF  # the magic
    assert lib.pgdvs_jpeg_scan_decode_host(*args()) == -1 and b"pgdvs_jpeg_scan_prepare" in lib.pgdvs_last_error()
    assert not coef.any() and not ws.any()


# ---------------------------------------------------------------------------- the sanitizers, on a stand-alone program
def test_the_scan_reader_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_scan_fuzz"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")  # does this compiler have the sanitizers at all?
    probe = subprocess.run([cxx, *flags, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} lacks the address / undefined sanitizers: {(probe.stderr.strip().splitlines() or ['the probe does not run'])[-1]}")
    built = subprocess.run([cxx, *flags, str(ROOT / "tools" / "jpeg_scan_fuzz.cpp"), str(ROOT / "ml-pgdvs_amd" / "csrc" / "jpeg_entropy.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr  # (with the sanitizers there, a failure here is the driver's or the source's)
    streams = SC.fuzz_streams()
    for name, data in streams.items():
        (tmp_path / name).write_bytes(data)
    run = subprocess.run([str(exe), "20261021", "2000", *(str(tmp_path / n) for n in streams)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 3 and all("failures 0" in ln for ln in lines), run.stdout
    for ln, data in zip(lines, streams.values()):  # both sizes: the stream and its truncations; then the mutations
        decoded, refused, corrupt, fell_back = (int(ln.split(w)[1].split(",")[0].split()[0]) for w in
                                                ("decoded", "by the preparation", "corrupt for both", "fell back"))
        assert decoded + refused + corrupt + fell_back == 2 * (1 + len(data)) + 2000 and refused >= 2 * len(data) and decoded > 2 and corrupt > 0, ln


# ---------------------------------------------------------------------------- the loaders' keyword
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return RC.build_trees(tmp_path_factory.mktemp("jpeg_scan_host"))


@pytest.mark.parametrize("name", RC.LOADERS)
def test_device_entropy_needs_device_decode(name, trees):
    """refused in the constructor, in front of everything else it does"""
    with pytest.raises(ValueError, match="device_decode=True"):
        RC.make(name, trees, device_entropy=True)
    with pytest.raises(ValueError, match="device_decode=True"):
        RC.make(name, trees, device_entropy=True, device_resize=True, resident=True, device="cuda:0")
    with pytest.raises(ValueError, match="device_resize=True"):
        RC.make(name, trees, device_entropy=True, device_decode=True)
    if name != "nvidia_pure_geo":
        ds = RC.make(name, trees, resident=True, device=None)  # the default: off
        assert ds.store.device_entropy is False and ds.store.stats["scans_decoded_on_device"] == 0 == ds.store.stats["entropy_fallbacks"]


def test_device_entropy_needs_device_decode_dycheck_and_store(tmp_path):
    import dycheck_tree as DT
    from pgdvs_amd.datasets.dycheck_iphone import DyCheckiPhoneEvaluationDataset
    from pgdvs_amd.datasets.resident import SceneStore

    kw = dict(data_root=DT.build_tree(tmp_path), raw_data_dir="iphone", mask_data_dir="flow_mask", flow_data_dir="flow_mask", max_hw=-1,
              mode="eval", scene_ids=[DT.SCENE], spatial_src_view_type="closest_wo_temporal", n_src_views_spatial=3,
              n_src_views_temporal_track_one_side=2)
    with pytest.raises(ValueError, match="device_decode=True"):
        DyCheckiPhoneEvaluationDataset(**kw, device_entropy=True)
    assert DyCheckiPhoneEvaluationDataset(**kw, resident=True).store.device_entropy is False
    with pytest.raises(ValueError, match="device_decode=True"):
        SceneStore("cuda:0", device_resize=True, device_entropy=True)
    with pytest.raises(ValueError, match="entropy"):
        from pgdvs_amd import ops

        ops.jpeg_decode(JC.small_stream(), entropy="gpu")
