"""Cases and a float64 reference for the outlier filter's scalar, ``median + std * std_thres`` (csrc/knn.hip: the three-pass
radix select of ``stat_select_block`` and the fp64 sums of ``stat_pass_kernel``; pgdvs_renderer_dyn.py:419-427,
st_geo_renderer.py:51-59, pgdvs_renderer_dyn_track.py:359-371 in the reference).

The select orders floats by the key ``u | 0x80000000`` (non-negative) / ``~u`` (negative) of their bit pattern ``u`` and
looks at key bits [31:21] in pass 0, [20:10] in pass 1 and [9:0] in pass 2; one grid round of a pass is 120 x 256 = 30720
elements.  The cases put the median where that machinery can go wrong: in the first and last bin of each pass, on either side
of a pass boundary and of zero, inside runs of equal values, at counts around a wave, a workgroup and a grid round, behind
a count smaller than the capacity, next to non-finite entries and among denormals.

Test infrastructure only (tests/test_outlier_stats_host.py validates it without a GPU, tests/test_gpu_outlier_stats.py
runs the kernels over it): no fixtures, nothing here touches the GPU."""
import collections
import functools

import numpy as np

STD_THRES = (0.0, 0.1)  # every family: the median alone, and the config's value (dyn_pcl_outlier_std_thres)
ONE = 0x3F800000
COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 30719, 30720, 30721, 61441)
GARBAGE = 37  # entries behind the count in the capacity > n case

Ref = collections.namedtuple("Ref", "T B med sd")


def f32_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def key(x):
    """the select's order-preserving key of float32 values (stat_key)"""
    u = np.asarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def reference(x, std_thres):
    """float64: lower median (torch.median), unbiased std (torch.std), T = med + sd * std_thres with ``std_thres`` as the
    float32 the entry point receives, and the bound B on |thres - T| for a float32 evaluation of that expression:
    rounding sd to float, the product and the final add (fused or not) each cost at most 2^-24 relative to their operand,
    i.e. together less than 2^-22 * (|med| + |sd * std_thres|); 2^-149 covers results among the denormals.  The fp64
    accumulation error of the sums (n <= 61441) is orders of magnitude below that.
    T is NaN for n == 0, for n == 1 (std of one element) and when any element is non-finite."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.size
    nan = float("nan")
    if n == 0:
        return Ref(nan, nan, nan, nan)
    med = float(np.sort(x)[(n - 1) // 2])
    if n == 1 or not np.isfinite(x).all():
        return Ref(nan, nan, med, nan)
    mean = x.sum() / n
    sd = float(np.sqrt(((x - mean) ** 2).sum() / (n - 1)))
    prod = sd * float(np.float32(std_thres))
    return Ref(med + prod, 2.0 ** -22 * (abs(med) + abs(prod)) + 2.0 ** -149, med, sd)


def exact(ref, std_thres):
    """the threshold is the median itself, in any arithmetic: std_thres == 0, or all elements equal (sd == 0 exactly)"""
    return not np.isnan(ref.T) and (std_thres == 0.0 or ref.sd == 0.0)


def clear_of_threshold(x, std_thres):
    """the precondition of the flag comparison: no element within B of T (so ``x < thres`` is the same for every thres
    within B of T) -- not needed where the threshold is exact or NaN"""
    ref = reference(x, std_thres)
    if np.isnan(ref.T) or exact(ref, std_thres):
        return True
    return bool(np.abs(np.asarray(x, np.float32).astype(np.float64) - ref.T).min() > ref.B)


# ---------------------------------------------------------------- families: rng -> avg[capacity] (float32), n = capacity unless said
def _majority(rng, major, others):
    """more than half of the elements equal ``major`` (so it is the median), the rest drawn from ``others``"""
    rest = rng.choice(others, size=40, replace=False)
    return rng.permutation(np.concatenate([np.full(47, major, np.uint32), rest.astype(np.uint32)]))


def _low(rng, which):
    """values that differ only in key bits [9:0]: pass 2 decides"""
    if which == "spread":
        return f32_bits(ONE + rng.choice(1024, size=62, replace=False).astype(np.uint32))
    major = {"bin0": 0, "bin1023": 1023}[which]
    return f32_bits(_majority(rng, ONE + major, ONE + np.setdiff1d(np.arange(1024), [major])))


def _mid(rng, which):
    """values that differ only in key bits [20:10]: pass 1 decides"""
    if which == "spread":
        return f32_bits(ONE + (rng.choice(2048, size=62, replace=False).astype(np.uint32) << 10))
    major = {"bin0": 0, "bin2047": 2047}[which]
    return f32_bits(_majority(rng, ONE + (major << 10), ONE + (np.setdiff1d(np.arange(2048), [major]) << 10)))


def _top_values():
    """both signs, exponents 2^-60 .. 2^40, the two mantissa bits pass 0 sees: only key bits [31:21] differ"""
    e = np.arange(127 - 60, 127 + 40 + 1, dtype=np.uint32)
    pos = ((e[:, None] << 23) | (np.arange(4, dtype=np.uint32)[None] << 21)).ravel()
    pos = pos[f32_bits(pos) <= np.float32(2.0 ** 40)]
    return np.concatenate([pos | np.uint32(0x80000000), pos])


def _top(rng, which):
    vals = _top_values()
    if which == "spread":
        return f32_bits(rng.choice(vals, size=202, replace=False))
    order = vals[np.argsort(key(f32_bits(vals)))]
    major = order[0] if which == "first" else order[-1]  # -2^40 / +2^40: the first / last occupied bin of pass 0
    return f32_bits(_majority(rng, major, order[1:-1]))


def _around(rng, lo_bits, hi_bits, below, above, half=50):
    """even n whose two middle elements are ``lo_bits`` | ``hi_bits``, neighbours in key order (but for the zeros between the
    two denormals)"""
    a, b = f32_bits([lo_bits])[0], f32_bits([hi_bits])[0]
    assert 1 <= int(key(b)) - int(key(a)) <= 3
    lo, hi = below(rng, half - 1).astype(np.float32), above(rng, half - 1).astype(np.float32)
    assert (key(lo) < key(a)).all() and (key(hi) > key(b)).all()
    return rng.permutation(np.concatenate([lo, [a, b], hi]).astype(np.float32))


def _boundary(rng, which):
    if which == "pass0":
        return _around(rng, 0x3FDFFFFF, 0x3FE00000, lambda r, k: r.uniform(0.5, 1.7, k), lambda r, k: r.uniform(1.8, 3.0, k))
    if which == "pass1":
        return _around(rng, 0x3F8003FF, 0x3F800400, lambda r, k: r.uniform(0.5, 0.99, k), lambda r, k: r.uniform(1.01, 2.0, k))

    def mag(r, k):
        return np.exp2(r.uniform(-60, 0, k))
    if which == "denormal-sign":  # largest negative denormal | smallest positive denormal
        return _around(rng, 0x80000001, 0x00000001, lambda r, k: -mag(r, k), mag)
    return _around(rng, 0x80000000, 0x00000000, lambda r, k: -mag(r, k), mag)  # -0.0 | +0.0


def _ties(rng, which):
    if which == "all-equal":
        return np.full(100, 0.37, np.float32)
    below, above = {"first": (40, 34), "last": (34, 40)}[which]  # n = 81, rank 40: the run's first / last element
    lo = ONE + rng.choice(500, size=below, replace=False).astype(np.uint32)
    hi = ONE + 501 + rng.choice(523, size=above, replace=False).astype(np.uint32)
    return f32_bits(rng.permutation(np.concatenate([lo, np.full(7, ONE + 500, np.uint32), hi])))


def _lognormal(rng, n):
    return rng.lognormal(0.0, 1.0, n).astype(np.float32)


def _families():
    """name -> (builder(rng) -> (avg, n) or {variant: (avg, n)}, std_thres values)"""
    fam = {}

    def add(name, fn, stds=STD_THRES):
        fam[name] = (fn, stds)

    def whole(fn, *a):
        def build(rng):
            x = fn(rng, *a)
            return x, x.size
        return build

    for w in ("spread", "bin0", "bin1023"):
        add(f"low-{w}", whole(_low, w))
    for w in ("spread", "bin0", "bin2047"):
        add(f"mid-{w}", whole(_mid, w))
    for w in ("spread", "first", "last"):
        add(f"top-{w}", whole(_top, w))
    for w in ("pass0", "pass1", "denormal-sign", "zero-sign"):
        add(f"boundary-{w}", whole(_boundary, w))
    for w in ("first", "last", "all-equal"):
        add(f"ties-{w}", whole(_ties, w))

    def counts(n):
        def build(rng):
            x = _lognormal(rng, n)
            if n == 0:  # (nothing to read: the capacity holds what a previous view left)
                x = np.full(64, 1e30, np.float32)
                return {"sorted": (x, 0), "shuffled": (x, 0)}
            return {"sorted": (np.sort(x), n), "shuffled": (rng.permutation(x), n)}
        return build
    for n in COUNTS:
        add(f"counts-{n}", counts(n))

    def capacity(rng):
        x = _lognormal(rng, 200)
        tail = np.resize(np.array([np.nan, np.inf, 1e30], np.float32), GARBAGE)
        return np.concatenate([x, tail]), 200
    add("capacity", capacity, STD_THRES + (2.0,))

    def nonfinite(v):
        def build(rng):
            x = _lognormal(rng, 200)
            x[77] = v
            return x, 200
        return build
    add("nonfinite-inf", nonfinite(np.inf))
    add("nonfinite-nan", nonfinite(np.nan))

    def denormals(rng):
        x = f32_bits(rng.choice(np.arange(1, 1001), size=60, replace=False).astype(np.uint32))  # k * 2^-149
        return x, 60
    add("denormals", denormals)
    return fam


@functools.lru_cache(maxsize=None)
def _built():
    """every family from the first seed at which no element lies within B of a threshold (searched here, on the CPU;
    tests/test_outlier_stats_host.py asserts the property itself)"""
    out = []
    for i, (name, (fn, stds)) in enumerate(_families().items()):
        for attempt in range(64):
            made = fn(np.random.default_rng(1000 * i + attempt))
            variants = made if isinstance(made, dict) else {None: made}
            if all(clear_of_threshold(x[:n], s) for x, n in variants.values() for s in stds):
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the elements clear of the threshold")
        for v, (x, n) in variants.items():
            x = np.ascontiguousarray(x, dtype=np.float32)
            x.setflags(write=False)
            for s in stds:
                out.append((f"{name}{'-' + v if v else ''}-s{s}", x, n, s))
    return tuple(out)


def cases():
    """(name, avg float32[capacity] (read-only), n, std_thres)"""
    return list(_built())


def case_ids():
    return [c[0] for c in _built()]
