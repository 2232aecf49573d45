"""Packed label codes on the device (12 / 14 bits per cached code in 1024-row
tiles): the three-call protocol of tests/test_label_cache_gpu.py (first
sight / emit / hit) with label_code_pack_min_rows lowered to 1, every result
compared with the oracle in the tolerance classes of tests/test_hip_parity.py
(arg-like funcs exactly), the third call a hit, and label_cache_stats()
showing the packed size ceil(n/1024) * 128 * W."""

import functools
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi
from oracle import groupby_reduce as oracle_reduce
from tests.test_label_cache_gpu import (
    TWO_PASS, _check, _delta, _labels, _max_lds_groups, _values,
)

pytestmark = pytest.mark.gpu

# one grid-stride iteration of the packed kernel: 2 resident blocks on each of
# 256 CUs x 16 waves x one 1024-row tile = 8 388 608 rows; this size runs a
# second iteration and ends in a partial tile
N_PAST_GRID = 8_500_005


def _width(ng):
    return 12 if ng <= 4094 else 14 if ng <= 16382 else 16


def _nbytes(n, width):
    return 2 * n if width == 16 else -(-n // 1024) * 128 * width


def _three_calls(vals_t, by_ts, func, expected, want, width, min_rows=1):
    """three calls, each checked; the third is served from the cache, which
    holds the codes at `width` bits"""
    n = by_ts[0].numel()
    passes = 2 if func in TWO_PASS else 1
    with flox_amd.set_options(label_code_pack_min_rows=min_rows):
        flox_amd.clear_label_cache()
        s = [flox_amd.label_cache_stats()]
        for _ in range(3):
            got, *_g = flox_amd.groupby_reduce(vals_t, *by_ts, func=func, expected_groups=expected)
            _check(got, want, func)
            s.append(flox_amd.label_cache_stats())
    total, third = _delta(s[0], s[3]), _delta(s[2], s[3])
    assert third == {"hits": passes, "emits": 0, "misses": 0}, (third, total)
    assert total["misses"] == 1 and total["emits"] == 1, total
    assert s[3]["bytes"] == _nbytes(n, width), (s[3]["bytes"], n, width)


def _run(n, ng, func, vdtype, ldtype="int64", bad=True, width=None, min_rows=1):
    rng = np.random.default_rng(zlib.crc32(f"packed-{n}-{ng}-{func}-{vdtype}-{ldtype}".encode()))
    vals = _values(rng, n, vdtype, func)
    lab = _labels(rng, n, ng, ldtype, bad)
    want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(ng))
    _three_calls(torch.as_tensor(vals).cuda(), (torch.as_tensor(lab).cuda(),),
                 func, np.arange(ng), want, _width(ng) if width is None else width,
                 min_rows=min_rows)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385])
@pytest.mark.parametrize("func,vdtype", [("mean", "float32"), ("first", "int32")])
def test_row_counts(n, func, vdtype):
    # lane (16 rows), tile (1024) and block-iteration (16 tiles) boundaries
    _run(n, 255, func, vdtype)


@functools.lru_cache(maxsize=None)
def _big():
    """one shared data set past a full grid-stride iteration (read-only)"""
    rng = np.random.default_rng(199)
    n = N_PAST_GRID
    vals = (rng.standard_normal(n) * 100).astype("float32")
    vals[::97] = np.nan
    lab = _labels(rng, n, 255)
    return vals, lab, torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()


@pytest.mark.parametrize("func", ["nanmean", "first"])
def test_past_one_grid_stride_iteration(func):
    vals, lab, vals_t, lab_t = _big()
    want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(255))
    _three_calls(vals_t, (lab_t,), func, np.arange(255), want, 12)


@pytest.mark.parametrize("ng", [1, 4094, 4095, 10_000])
def test_group_counts(ng):
    # 4094 is the last 12-bit count, 4095 the first 14-bit one
    _run(20_001, ng, "mean", "float32")


def test_largest_lds_group_count():
    ng = _max_lds_groups(_ffi.SET_SUM_COUNT, _ffi.F32)
    assert 4095 <= ng <= 16382  # 14-bit
    _run(100_003, ng, "mean", "float32", width=14)


def test_last_14_bit_count_and_first_uint16_one():
    assert _max_lds_groups(_ffi.SET_COUNT, _ffi.F64) >= 16383
    _run(100_003, 16382, "count", "float64", width=14)
    _run(100_003, 16383, "count", "float64", width=16)  # bytes == 2n


@pytest.mark.parametrize("vdtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("func", ["sum", "nanmean", "min", "argmax"])
def test_funcs_and_dtypes(func, vdtype):
    # NaNs in float values; labels of -1, ng and ng + 70000 (_labels)
    _run(16385, 257, func, vdtype)


def test_two_by():
    rng = np.random.default_rng(zlib.crc32(b"packed-2by"))
    n = 100_003
    vals = _values(rng, n, "float64", "nanmean")
    a = rng.integers(0, 12, n).astype("int64")
    b = rng.integers(0, 180, n).astype("int64")
    k = rng.random(n)
    a[k < 0.01] = -1
    a[(k >= 0.01) & (k < 0.02)] = 12       # out of range in the first key only
    b[(k >= 0.02) & (k < 0.03)] = 180      # ... in the second key only
    b[(k >= 0.03) & (k < 0.04)] = -5
    a[(k >= 0.04) & (k < 0.05)] = 13       # ... in both
    b[(k >= 0.04) & (k < 0.05)] = 70_000
    expected = (np.arange(12), np.arange(180))
    want, *_ = oracle_reduce(vals, a, b, func="nanmean", expected_groups=expected)
    assert want.shape == (12, 180)
    _three_calls(torch.as_tensor(vals).cuda(),
                 (torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()),
                 "nanmean", expected, want, 12)  # 2160 groups


def test_offset_view_values():
    # values that start 4 bytes into an allocation
    vals, lab, vals_t, lab_t = _big()
    n = 100_001
    want, *_ = oracle_reduce(vals[1:n + 1], lab[:n], func="nanmean", expected_groups=np.arange(255))
    by = lab_t[:n].clone()
    _three_calls(vals_t[1:n + 1], (by,), "nanmean", np.arange(255), want, 12)


def test_every_row_out_of_range():
    rng = np.random.default_rng(5)
    n, ng = 10_007, 300
    vals = _values(rng, n, "float32", "mean")
    lab = np.where(rng.random(n) < 0.5, -1, ng + rng.integers(0, 1 << 20, n)).astype("int64")
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    for func in ("mean", "sum", "count", "first"):
        want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(ng))
        _three_calls(vals_t, (lab_t,), func, np.arange(ng), want, 12)


def test_second_stream_consumes_codes_packed_on_the_first():
    rng = np.random.default_rng(24)
    n, ng = 1_000_003, 500
    vals = _values(rng, n, "float32", "mean")
    lab = _labels(rng, n, ng)
    want, *_ = oracle_reduce(vals, lab, func="nanmean", expected_groups=np.arange(ng))
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    with flox_amd.set_options(label_code_pack_min_rows=1):
        flox_amd.clear_label_cache()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s0 = flox_amd.label_cache_stats()
        with torch.cuda.stream(s1):
            for _ in range(2):  # first sight, then the emitting and packing call
                r1, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="nanmean", expected_groups=range(ng))
        with torch.cuda.stream(s2):  # no host sync in between
            r2, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="nanmean", expected_groups=range(ng))
        torch.cuda.synchronize()
    stats = flox_amd.label_cache_stats()
    assert _delta(s0, stats) == {"hits": 1, "emits": 1, "misses": 1}
    assert stats["bytes"] == _nbytes(n, 12)
    _check(r1, want, "nanmean")
    _check(r2, want, "nanmean")


def test_var_hits_twice():
    assert "var" in TWO_PASS
    _run(30_001, 300, "var", "float64")


def test_default_threshold_keeps_uint16():
    # the option left alone (None): a call this small keeps the 2 B/row form
    _run(30_001, 300, "mean", "float32", width=16, min_rows=None)
