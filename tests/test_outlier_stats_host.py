"""Host (no GPU): the cases and the float64 reference of tests/outlier_cases.py, checked before any kernel is compared
with them -- the reference's own expression ``torch.median(t) + torch.std(t) * std_thres`` in float32 on the CPU
(pgdvs_renderer_dyn.py:419-427) and ``oracle.outlier_threshold`` must agree with ``reference`` within its derived bound,
and no element of a case may lie within that bound of the threshold, so that tests/test_gpu_outlier_stats.py can compare
the flags of every element."""
import warnings

import numpy as np
import pytest
import torch

import outlier_cases as oc
from oracle import oracle as orc  # noqa: E402  (checker only)

CASES = oc.cases()
IDS = oc.case_ids()


def _agrees(got, ref, std_thres, what):
    got = float(got)
    if np.isnan(ref.T):
        assert np.isnan(got), (what, got)
    elif oc.exact(ref, std_thres):
        assert got == ref.med, (what, got, ref.med)
    else:
        assert abs(got - ref.T) <= ref.B, (what, got, ref.T, abs(got - ref.T), ref.B)


def test_the_families_are_all_there():
    names = set(IDS)
    assert len(names) == len(IDS)
    for s in oc.STD_THRES:
        for fam in ["low-spread", "low-bin0", "low-bin1023", "mid-spread", "mid-bin0", "mid-bin2047", "top-spread", "top-first",
                    "top-last", "boundary-pass0", "boundary-pass1", "boundary-denormal-sign", "boundary-zero-sign", "ties-first",
                    "ties-last", "ties-all-equal", "capacity", "nonfinite-inf", "nonfinite-nan", "denormals"]:
            assert f"{fam}-s{s}" in names, fam
        for n in oc.COUNTS:
            assert {f"counts-{n}-sorted-s{s}", f"counts-{n}-shuffled-s{s}"} <= names, n
    assert "capacity-s2.0" in names


@pytest.mark.parametrize("name,avg,n,std_thres", CASES, ids=IDS)
def test_reference_agrees_with_torch_and_oracle(name, avg, n, std_thres):
    x = avg[:n]
    ref = oc.reference(x, std_thres)
    t = torch.from_numpy(x.copy())
    assert t.dtype == torch.float32
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # (std of one element, inf - inf)
        if n > 0:  # (torch.median of an empty tensor raises or gives NaN, by version: the contract is NaN, pinned on the GPU)
            med_t = torch.median(t)
            if not np.isnan(x).any():
                assert float(med_t) == ref.med
            _agrees(med_t + torch.std(t) * std_thres, ref, std_thres, "torch")
        _agrees(orc.outlier_threshold(x, std_thres), ref, std_thres, "oracle")


@pytest.mark.parametrize("name,avg,n,std_thres", CASES, ids=IDS)
def test_no_element_within_the_bound_of_the_threshold(name, avg, n, std_thres):
    x = avg[:n].astype(np.float64)
    ref = oc.reference(avg[:n], std_thres)
    if np.isnan(ref.T):
        assert n <= 1 or not np.isfinite(x).all()
    elif oc.exact(ref, std_thres):
        assert ref.T == ref.med and (x == ref.med).any()
    else:
        assert ref.B < abs(ref.sd * std_thres)  # (the threshold is told from the median)
        assert np.abs(x - ref.T).min() > ref.B
    assert oc.clear_of_threshold(avg[:n], std_thres)


@pytest.mark.parametrize("name,lo,hi", [("boundary-pass0", 0x3FDFFFFF, 0x3FE00000), ("boundary-pass1", 0x3F8003FF, 0x3F800400),
                                        ("boundary-denormal-sign", 0x80000001, 0x00000001),
                                        ("boundary-zero-sign", 0x80000000, 0x00000000)])
def test_boundary_cases_straddle_their_boundary(name, lo, hi):
    """even n, the two middle elements of the key order are the pair: the lower one is the median"""
    avg, n = next((a, n) for c, a, n, s in CASES if c == f"{name}-s0.0")
    assert n % 2 == 0 and n == avg.size
    k = np.sort(oc.key(avg))
    assert [int(k[n // 2 - 1]), int(k[n // 2])] == [int(oc.key(oc.f32_bits([lo]))[0]), int(oc.key(oc.f32_bits([hi]))[0])]
    assert np.float32(oc.reference(avg, 0.0).med).view(np.uint32) == lo or name == "boundary-zero-sign"


def test_bit_families_use_the_bins_they_name():
    by = {c: (a[:n], n) for c, a, n, s in CASES if s == 0.0}

    def med_key(name):
        x, n = by[name + "-s0.0"]
        return int(np.sort(oc.key(x))[(n - 1) // 2]), oc.key(x)

    for name, shift, mask, want in [("low-bin0", 0, 0x3FF, 0), ("low-bin1023", 0, 0x3FF, 1023), ("mid-bin0", 10, 0x7FF, 0),
                                    ("mid-bin2047", 10, 0x7FF, 2047)]:
        m, k = med_key(name)
        assert (m >> shift) & mask == want and (k == m).sum() * 2 > k.size
        assert len(set((k >> (shift + (10 if shift == 0 else 11))).tolist())) == 1  # one bin in the passes before
    for name, pick in [("top-first", min), ("top-last", max)]:
        m, k = med_key(name)
        assert m >> 21 == pick((k >> 21).tolist()) and (k == m).sum() * 2 > k.size
        assert (by[name + "-s0.0"][0].view(np.uint32) & 0x1FFFFF == 0).all()  # only the bits pass 0 sees
    for name, first in [("ties-first", True), ("ties-last", False)]:
        x, n = by[name + "-s0.0"]
        s = np.sort(x)
        r = (n - 1) // 2
        assert s[r - 1] != s[r] if first else s[r + 1] != s[r]
        assert (s == s[r]).sum() > 1
    x, n = by["denormals-s0.0"]
    assert (x > 0).all() and (x <= np.float32(1000 * 2.0 ** -149)).all()
    for name in ("low-spread", "mid-spread", "top-spread"):
        x = by[name + "-s0.0"][0]
        assert x.size % 2 == 0 and np.abs(x).min() >= 2.0 ** -60 and np.abs(x).max() <= 2.0 ** 40
