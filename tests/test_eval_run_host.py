"""The evaluator's loop on the host / torch path (harness.eval_run): against what the reference's own
``run_eval_single_ckpt(save_individual=True)`` left behind on the same inputs (tests/golden/eval_run_nvidia.npz, made by
tests/golden/make_golden_eval_run.py) -- file names, decoded pixels, the records' keys / order / values, the averages --
plus the sharding over ranks, the argument errors and the identity the HIP export pass rests on."""
import os
import pathlib
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_run_reference as ER  # noqa: E402
import vis_reference as VR  # noqa: E402

from pgdvs_amd import harness, png  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return ER.load_fixture()


@pytest.mark.parametrize("run", sorted(ER.RUNS))
def test_eval_run_leaves_what_the_reference_run_left(tmp_path, g, run):
    with_geo, n_max = ER.RUNS[run]
    model = ER.RecordedModel(with_geo)
    other, tmp_path = tmp_path / "other", tmp_path / "main"
    res = harness.eval_run(model, ER.Items(g), "rc", batch_size=2, n_max_data=n_max, with_ssim=True, save_individual=True,
                           info_dir=tmp_path / "info", vis_dir=tmp_path / "vis")
    assert not model.training and model.calls == (2 if run == "max3" else 3)
    ER.check_against_fixture(g, run, tmp_path, res, with_ssim=True)
    assert all(f"eval/{k}" in res for k in harness.METRIC_KEYS + harness.SSIM_KEYS) and not any("lpips" in k for k in res)
    # without SSIM the record holds the PSNRs alone, in upstream's order; run_ahead is accepted on the torch path (as k = 0)
    res2 = harness.eval_run(ER.RecordedModel(with_geo), ER.Items(g), "rc", batch_size=2, n_max_data=n_max, save_individual=True,
                            info_dir=other / "info", vis_dir=other / "vis", run_ahead=2)
    assert ER.all_files(other) == ER.all_files(tmp_path)
    assert all(list(r["info"]) == ["src_frame_ids", "psnr_full_combined", "psnr_dyn_combined", "psnr_static_combined"]
               for r in res2["records"])
    assert all(res2[f"eval/{k}"] == res[f"eval/{k}"] for k in harness.METRIC_KEYS)
    for name in ER.all_files(other):
        if name.endswith(".png"):
            assert (other / name).read_bytes() == (tmp_path / name).read_bytes(), name
    # no files without save_individual, same numbers
    res3 = harness.eval_run(ER.RecordedModel(with_geo), ER.Items(g), "rc", batch_size=2, n_max_data=n_max)
    assert {k: v for k, v in res3.items() if k != "records"} == {k: v for k, v in res2.items() if k != "records"}
    assert [r["name"] for r in res3["records"]] == [r["name"] for r in res2["records"]]


def test_eval_run_shards_over_ranks(tmp_path, g):
    """world 2: the two ranks' files together are the single-rank set, names differing only in _rank_<r>; each rank's sums are
    its own (no process group here: nothing to reduce into)"""
    single = tmp_path / "single"
    one = harness.eval_run(ER.RecordedModel(True), ER.Items(g), None, save_individual=True, info_dir=single / "info", vis_dir=single / "vis")
    union, count, total = [], 0, 0.0
    for r in range(2):
        d = tmp_path / f"r{r}"
        res = harness.eval_run(ER.RecordedModel(True), ER.Items(g), None, rank=r, world=2, save_individual=True, info_dir=d / "info",
                               vis_dir=d / "vis")
        files = ER.all_files(d)
        assert all(f.endswith(f"_rank_{r}.pkl") for f in files if f.endswith(".pkl"))
        union += [f.replace(f"_rank_{r}.pkl", "_rank_0.pkl") for f in files]
        count += res["eval/count"]
        total += res["sums"]["eval/psnr_full_combined"]
    # 5 items over 2 ranks: DistributedSampler pads by wrapping, so item 0 is evaluated by rank 1 as well
    assert count == 6 and sorted(set(union)) == ER.all_files(single) and len(union) == len(set(union)) + 4
    first = one["records"][0]["info"]["psnr_full_combined"]
    assert abs(total - first - one["sums"]["eval/psnr_full_combined"]) < 1e-4


def test_the_256_levels_survive_the_quantise_divide_multiply_cast_chain():
    """upstream writes _gt.png / _combined.png from the evaluator's quantised images, (q / 255 * 255).astype(uint8) in float32;
    for every level that is q again under truncation, so the export may cast the clamped raw image once"""
    q = np.arange(256, dtype=np.uint8)
    chain = (torch.from_numpy(q).float() / 255.0).numpy()
    assert chain.dtype == np.float32 and np.array_equal((chain * 255).astype(np.uint8), q)
    x = torch.linspace(-0.2, 1.2, 100001)
    x = torch.cat([x, torch.from_numpy(chain), torch.from_numpy(np.nextafter(chain, np.float32(2))), torch.from_numpy(np.nextafter(chain, np.float32(-1)))])
    upstream = ((x.clamp(0.0, 1.0) * 255).byte().float() / 255.0).numpy()
    assert np.array_equal((upstream * 255).astype(np.uint8), png.quantize_truncate(x).numpy())


def test_eval_run_argument_errors_and_a_failing_writer(tmp_path, g, monkeypatch):
    ds, m = ER.Items(g), ER.RecordedModel()
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, save_individual=True)
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, save_individual=True, info_dir=tmp_path)
    for bad in (4, -1, 1.0):
        with pytest.raises(ValueError):
            harness.eval_run(m, ds, None, run_ahead=bad)
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, batch_size=0)
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, rank=2, world=2)
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, quant_type="other")
    with pytest.raises(ValueError):
        harness.eval_run(m, ds, None, quant_type="dycheck_iphone", with_ssim=True)
    with pytest.raises(ValueError):  # (the nvidia fixture's mask has three channels)
        harness.eval_run(m, ds, None, quant_type="dycheck_iphone")
    assert m.calls == 0
    # a directory that is a regular file: unwritable for every user; the error comes out of eval_run
    blocker = tmp_path / "blocker"
    blocker.write_bytes(b"x")
    with pytest.raises(OSError):
        harness.eval_run(m, ds, None, save_individual=True, info_dir=tmp_path / "info", vis_dir=blocker)

    class FailingWriter(png.PngWriter):
        def _work(self, path, buf, H, W, slot):
            if path.name.endswith("00011_cam_005_combined.png"):
                path = blocker / "no.png"
            return super()._work(path, buf, H, W, slot)

    # a worker's failure surfaces when its owner closes the writer; eval_run leaves a given writer open
    w = FailingWriter(n_threads=2)
    harness.eval_run(ER.RecordedModel(), ds, None, save_individual=True, info_dir=tmp_path / "i2", vis_dir=tmp_path / "v2", writer=w)
    with pytest.raises(OSError):
        w.close()
    assert len(ER.all_files(tmp_path / "v2")) == 9 and len(ER.all_files(tmp_path / "i2")) == 5
    with open(tmp_path / "i2" / "scene_a" / "00003_cam_000_rank_0.pkl", "rb") as f:
        assert list(pickle.load(f)) == ["src_frame_ids", "psnr_full_combined", "psnr_dyn_combined", "psnr_static_combined"]
    # the writer eval_run makes itself: a worker's failure comes out of eval_run, which closes the writer before it returns
    monkeypatch.setattr(png, "PngWriter", FailingWriter)
    with pytest.raises(OSError):
        harness.eval_run(ER.RecordedModel(), ds, None, save_individual=True, info_dir=tmp_path / "i3", vis_dir=tmp_path / "v3")
    assert len(ER.all_files(tmp_path / "v3")) == 9 and len(ER.all_files(tmp_path / "i3")) == 5  # (every other file is whole)
    assert not [t._name for t in __import__("threading").enumerate() if t._name.startswith("png")]  # the pool is shut down

    # when the loop fails as well, its error is the one raised (the writer is still closed; its error is dropped)
    class Boom(RuntimeError):
        pass

    class FailsAtThirdStep(ER.RecordedModel):
        def forward(self, data, **kw):
            if self.calls == 2:
                raise Boom("forward")
            return super().forward(data, **kw)

    with pytest.raises(Boom):
        harness.eval_run(FailsAtThirdStep(), ds, None, batch_size=2, save_individual=True, info_dir=tmp_path / "i4", vis_dir=tmp_path / "v4")
    # views 0..3 were finished before the third forward; the failing file of view 1 (00011_cam_005) is the one missing
    assert len(ER.all_files(tmp_path / "i4")) == 4 and len(ER.all_files(tmp_path / "v4")) == 7
    assert not [t._name for t in __import__("threading").enumerate() if t._name.startswith("png")]


def test_dycheck_protocol_records(tmp_path):
    """the other protocol through the loop: upstream's key order (psnr, ssim, [lpips,] mpsnr, mssim) and eval_step's values"""
    gen = torch.Generator().manual_seed(3)
    H, W = 36, 44
    items = [{"rgb_src_temporal": torch.zeros(2, H, W, 3), "rgb_tgt": torch.rand(H, W, 3, generator=gen),
              "eval_mask": (torch.rand(H, W, 1, generator=gen) < 0.6).float(), "seq_ids": torch.tensor([i, i + 1, i + 2]),
              "pred": torch.rand(3, H, W, generator=gen), "geo": torch.zeros(3, H, W),
              "misc": {"scene_id": "s", "tgt_frame_id": i, "tgt_cam_id": 1}} for i in range(3)]
    res = harness.eval_run(ER.RecordedModel(), items, None, batch_size=2, quant_type="dycheck_iphone", save_individual=True,
                           info_dir=tmp_path / "info", vis_dir=tmp_path / "vis")
    assert [list(r["info"]) for r in res["records"]] == [["src_frame_ids", "psnr_combined", "ssim_combined", "mpsnr_combined", "mssim_combined"]] * 3
    sums = {}
    for batch in (items[:2], items[2:]):
        md = harness.eval_step(ER.RecordedModel(), harness.collate(batch), None, quant_type="dycheck_iphone")
        for k, v in md.items():
            sums[k] = sums[k] + v if k in sums else v
    assert res["eval/count"] == int(sums["eval/count"]) == 3
    for k in harness.DYCHECK_KEYS:
        assert res["sums"][f"eval/{k}"] == float(sums[f"eval/{k}"]), k
        assert res[f"eval/{k}"] == float(sums[f"eval/{k}"] / sums["eval/count"]), k
    assert len(ER.all_files(tmp_path)) == 9


def test_both_static_images_are_written(tmp_path, g):
    """a renderer that returns static_coarse_rgb and geo_static_rgb: upstream writes both (evaluator_pgdvs.py:442-465), each the
    truncating cast of the clamped image"""
    res = harness.eval_run(ER.RecordedModel(with_geo=True, gnt=True), ER.Items(g), None, batch_size=2, save_individual=True,
                           info_dir=tmp_path / "info", vis_dir=tmp_path / "vis")
    ER.check_static_images(g, tmp_path / "vis", res, VR.expected_truncate)


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "ml-pgdvs_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import eval_run_reference as ER
from pgdvs_amd import harness
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g = ER.load_fixture()
calls = []
real = dist.reduce
dist.reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
res = harness.eval_run(ER.RecordedModel(), ER.Items(g), None, rank=rank, world=world)
assert len(calls) == 1, calls  # ONE collective for the run (three steps on each rank)
try:
    harness.eval_run(ER.RecordedModel(), ER.Items(g), None, rank=rank, world=world + 1)
    raise SystemExit("a world that is not the group's was accepted")
except ValueError:
    pass
dist.reduce = real
parts = [None] * world
dist.all_gather_object(parts, {k: v for k, v in res["sums"].items()} if rank else None)
if rank == 0:
    import numpy as np
    single = harness.eval_run(ER.RecordedModel(), ER.Items(g), None)
    first = single["records"][0]["info"]  # 5 items over 2 ranks: the sampler wraps, item 0 is evaluated twice
    assert res["eval/count"] == 6 and res["sums"]["eval/count"] == 6
    for k in harness.METRIC_KEYS:
        want = single["sums"][f"eval/{k}"] + first[k]
        assert abs(res["sums"][f"eval/{k}"] - want) <= 1e-5 * abs(want), (k, res["sums"], want)
        assert res[f"eval/{k}"] == float(torch.tensor(res["sums"][f"eval/{k}"], dtype=torch.float32) / torch.tensor([6]))
    assert parts[1]["eval/count"] == 3  # the other rank returned its own partial sums
    print("REDUCE_OK")
else:
    assert res["eval/count"] == 3 and len(res["records"]) == 3
dist.destroy_process_group()
"""


def test_eval_run_reduces_once_over_a_two_rank_group(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29717", str(script), str(root)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REDUCE_OK" in r.stdout
