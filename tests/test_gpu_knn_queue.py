"""GPU tests of the thread-per-query kNN pass's candidate queue (MI355X): one insertion chain per trigger on every
lane's newest entry, two candidates of a run per step.  Every case compares the grid search (`algo=2`) with the
brute-force kernel (`algo=1`, itself pinned on the oracle) bit for bit, for every K + 1 the pass is instantiated for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pgdvs_amd import ops  # noqa: E402

DEV = "cuda:0"
KS = [4, 8, 16, 20, 50]  # K + 1 = 5, 9, 17, 21, 51


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pgdvs_amd import _lib

    _lib.load()


def _both(pts, K):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n = len(pts)
    assert n <= 40_000
    t = torch.from_numpy(pts).to(DEV)
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    grid = ops.knn_mean_dist(t, cnt, K, algo=2).cpu().numpy()[:n]
    brute = ops.knn_mean_dist(t, cnt, K, algo=1).cpu().numpy()[:n]
    return grid.view(np.uint32), brute.view(np.uint32)


def _check(pts, K):
    grid, brute = _both(pts, K)
    bad = np.flatnonzero(grid != brute)
    assert bad.size == 0, f"K={K}, n={len(pts)}: {bad.size} results differ, first at {bad[:8]}"


def _sheet(rng, n):
    u = rng.uniform(-1, 1, (n, 2))
    return np.stack([u[:, 0], u[:, 1], 0.1 * np.sin(3 * u[:, 0]) * np.cos(2 * u[:, 1])], 1)


@pytest.mark.parametrize("K", KS)
def test_one_lane_under_queue_pressure(K):
    """A thin sheet in which one cell holds several hundred nearly coincident points and its neighbours a handful: the
    lanes of the sheet's queries next to the cluster accept on consecutive steps while their wavefront's other lanes
    accept nothing, so the trigger fires on back-to-back steps and lanes with empty queues take the chain."""
    rng = np.random.default_rng(100 + K)
    sheet = _sheet(rng, 8000)
    centre = sheet[17]
    cluster = centre + 1e-4 * rng.normal(size=(400, 3))
    _check(np.concatenate([sheet, cluster]), K)


@pytest.mark.parametrize("K", KS)
def test_queues_exactly_full_and_exactly_empty_at_the_end_of_the_walk(K):
    """Few points, all in one cell: n just above K + 1 (every lane accepts everything it sees; the walk ends with
    queues at every fill level), n = K + 1 (lists that are exactly full), n = K (too few points: the other search),
    n = 1, and n = 257 (one live lane in the last workgroup, the rest dead with empty queues)."""
    rng = np.random.default_rng(200 + K)
    for n in (K + 4, K + 2, K + 1, K, 1, 257):
        _check(rng.uniform(0.0, 1e-3, (n, 3)) + 0.5, K)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ["lattice", "duplicates"])
def test_ties(kind, K):
    """Equal and zero distances everywhere: a regular lattice whose points lie ON cell and quarter-cell boundaries, and
    a cloud with every point twice."""
    rng = np.random.default_rng(300 + K)
    if kind == "lattice":
        g = np.arange(16, dtype=np.float64) / 8.0
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        pts = pts[rng.permutation(len(pts))]
    else:
        half = _sheet(rng, 3000)
        pts = np.concatenate([half, half])[rng.permutation(6000)]
    _check(pts, K)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ["sparse_volume", "sheet_thin_x"])
def test_short_runs_and_odd_tails(kind, K):
    """Runs of one, two and three candidates and odd tails for the two-candidate step: a sparse volume (every point
    nearly alone in its cell) and a sheet that is thin along x (every row of a block is one or two cells long)."""
    rng = np.random.default_rng(400 + K)
    n = 5000
    if kind == "sparse_volume":
        pts = rng.uniform(-1, 1, (n, 3))
    else:
        u = rng.uniform(-1, 1, (n, 2))
        pts = np.stack([1e-3 * np.sin(7 * u[:, 0]), u[:, 0], u[:, 1]], 1)
    _check(pts, K)


def test_second_attempt_of_a_wavefront():
    """A slab several cells thick: the surface density estimate behind the starting threshold is too tight for most
    queries, more than a quarter of a wavefront's lists come out short and the wavefront walks its blocks again with
    the wider threshold -- queues, counts and buffers start over."""
    rng = np.random.default_rng(500)
    n = 20_000
    pts = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-0.15, 0.15, n)], 1)
    _check(pts, 50)
