"""The tree combine and its fused finish (mean / sum / count written by the
combine kernel itself): every case is compared with the oracle in the
tolerance classes of tests/test_hip_parity.py and with the same call under
set_options(fused_finalize=False) — bit-for-bit for integer inputs and for
count, within the same tolerance for floats (the fold order differs)."""

import contextlib
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from flox_amd import core as fa_core
from oracle import groupby_reduce as oracle_reduce
from tests.test_hip_parity import _tol

pytestmark = pytest.mark.gpu

FUNCS = ["mean", "nanmean", "sum", "nansum", "count"]
VDTYPES = ["float32", "float64", "int32", "int64"]
LDS_MAX = 160 * 1024 - 512  # csrc/floxhip.hip
N_PAST_GRID = 5_200_005     # past one grid stride of the u16 kernel
OP_SET_OF = {"mean": _ffi.SET_SUM_COUNT, "nanmean": _ffi.SET_SUM_COUNT,
             "sum": _ffi.SET_SUM_COUNT_PRESENT, "nansum": _ffi.SET_SUM_COUNT_PRESENT,
             "count": _ffi.SET_COUNT}


@contextlib.contextmanager
def _spy():
    """records, per grouped_partials call made by core, whether the combine
    kernel finished the result"""
    seen = []
    orig = fa_core.grouped_partials

    def wrapper(*a, **kw):
        out = orig(*a, **kw)
        seen.append("result" in out)
        return out

    fa_core.grouped_partials = wrapper
    try:
        yield seen
    finally:
        fa_core.grouped_partials = orig


def _values(rng, n, dtype, nan_group_rows=None):
    if np.dtype(dtype).kind == "f":
        v = (rng.standard_normal(n) * 100).astype(dtype)
        if n:
            v[rng.random(n) < 0.03] = np.nan
        if nan_group_rows is not None:
            v[nan_group_rows] = np.nan
    else:
        v = rng.integers(-1000, 1000, n).astype(dtype)
    return v


def _labels(rng, n, ng, ldtype="int64", bad=True, empty=()):
    lab = rng.integers(0, ng, n).astype(ldtype)
    if bad and n:
        k = rng.random(n)
        lab[k < 0.02] = -1
        lab[(k >= 0.02) & (k < 0.04)] = ng
        lab[(k >= 0.04) & (k < 0.05)] = ng + 70_000
    for g in empty:  # groups that receive no row
        lab[lab == g] = -1
    return lab


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _compare(fused, unfused, want, func, exact):
    fused, unfused = _np(fused), _np(unfused)
    assert fused.shape == want.shape and fused.dtype == unfused.dtype, (
        fused.shape, want.shape, fused.dtype, unfused.dtype)
    tol = _tol(func, want.dtype)
    np.testing.assert_allclose(fused, want, equal_nan=True, err_msg=f"{func} vs oracle", **tol)
    if exact:
        np.testing.assert_array_equal(fused, unfused, err_msg=f"{func} vs unfused")
    else:
        np.testing.assert_allclose(fused, unfused, equal_nan=True,
                                   err_msg=f"{func} vs unfused", **tol)


def _both(vals, bys, func, expected, calls=1, expect_fused=True, **kw):
    """oracle, then `calls` fused calls (each checked), then the unfused call"""
    want, *_ = oracle_reduce(vals, *bys, func=func, expected_groups=expected, **kw)
    vals_t = torch.as_tensor(vals).cuda()
    by_ts = tuple(torch.as_tensor(b).cuda() for b in bys)
    with flox_amd.set_options(fused_finalize=False), _spy() as seen_off:
        unfused, *_ = flox_amd.groupby_reduce(vals_t, *by_ts, func=func,
                                              expected_groups=expected, **kw)
    assert not any(seen_off)
    exact = func == "count" or np.dtype(vals.dtype).kind in "iu"
    flox_amd.clear_label_cache()
    for _ in range(calls):
        with _spy() as seen:
            fused, *_ = flox_amd.groupby_reduce(vals_t, *by_ts, func=func,
                                                expected_groups=expected, **kw)
        assert seen == [expect_fused], seen
        _compare(fused, unfused, want, func, exact)
    return fused


def _run(n, ng, func, vdtype, ldtype="int64", calls=1, expect_fused=True, **kw):
    rng = np.random.default_rng(zlib.crc32(f"ff-{n}-{ng}-{func}-{vdtype}-{ldtype}".encode()))
    lab = _labels(rng, n, ng, ldtype, empty=(0, ng // 2) if ng > 2 else ())
    # one all-NaN group (group 1) for the nan* functions
    vals = _values(rng, n, vdtype, nan_group_rows=(lab == 1) if ng > 2 else None)
    return _both(vals, (lab,), func, np.arange(ng), calls=calls,
                 expect_fused=expect_fused, **kw)


def _layout_bytes(op_set, vbytes, ng):
    """bin_layout of csrc/floxhip.hip for the three finished op sets"""
    sec = lambda elem: (ng * elem + 255) // 256 * 256  # noqa: E731
    b = sec(4)  # count
    if op_set != _ffi.SET_COUNT:
        b += sec(8)
    if op_set == _ffi.SET_SUM_COUNT_PRESENT:
        b += sec(4)
    return b


def _largest(pred):
    lo, hi = 1, 1 << 17
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def _max_lds_groups(op_set, ffi_dt):
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.op_set, c.vdtype = op_set, ffi_dt

    def lds(ng):
        c.ngroups = ng
        return lib.fh_query_path(ctypes.byref(c)) == 1

    return _largest(lds)


# ---- group counts --------------------------------------------------------

@pytest.mark.parametrize("ng", [1, 31, 32, 33, 257, 5000, 10_000, 30_000])
@pytest.mark.parametrize("func,vdtype", [("mean", "float32"), ("nansum", "float64"),
                                         ("count", "int32")])
def test_group_counts(ng, func, vdtype):
    # 30 000 groups of nansum bins (16 B each) exceed LDS: that one falls
    # back to partials + torch finalize and must still agree
    fits = _layout_bytes(OP_SET_OF[func], 0, ng) <= LDS_MAX
    _run(40_009, ng, func, vdtype, expect_fused=fits)


@pytest.mark.parametrize("func,vdtype,ffi_dt", [("mean", "float32", _ffi.F32),
                                                ("sum", "int64", _ffi.I64)])
def test_both_sides_of_the_two_blocks_per_cu_switch(func, vdtype, ffi_dt):
    op_set = OP_SET_OF[func]
    ng2 = _largest(lambda ng: 2 * _layout_bytes(op_set, 0, ng) <= LDS_MAX)
    # 600 011 rows are more than 512 blocks' worth, so nblocks is 512 below
    # the switch and 256 above it
    for ng in (ng2, ng2 + 1):
        _run(600_011, ng, func, vdtype)


@pytest.mark.parametrize("func,vdtype,ffi_dt", [("mean", "float32", _ffi.F32),
                                                ("sum", "float64", _ffi.F64),
                                                ("count", "int64", _ffi.I64)])
def test_largest_lds_group_count_and_one_more(func, vdtype, ffi_dt):
    ng = _max_lds_groups(OP_SET_OF[func], ffi_dt)
    assert _layout_bytes(OP_SET_OF[func], 0, ng) <= LDS_MAX < _layout_bytes(
        OP_SET_OF[func], 0, ng + 64)
    _run(100_003, ng, func, vdtype)
    _run(100_003, ng + 1, func, vdtype, expect_fused=False)


# ---- row counts ----------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 8 * 1024 - 1, 8 * 1024, 8 * 1024 + 1,
                               20 * 1024 + 5, 20 * 8 * 1024 + 5])
@pytest.mark.parametrize("func,vdtype", [("mean", "float32"), ("sum", "int64")])
def test_row_counts(n, func, vdtype):
    # three calls: the int64-label form (nblocks = ceil(n/1024)), the
    # emitting form and the u16 form (nblocks = ceil(n/8192)); 20 and 21
    # blocks are no multiple of the 32 slab lanes of the combine
    _run(n, 255, func, vdtype, calls=3)


@functools.lru_cache(maxsize=None)
def _big():
    rng = np.random.default_rng(99)
    n = N_PAST_GRID
    vals = (rng.standard_normal(n) * 100).astype("float32")
    vals[::97] = np.nan
    lab = _labels(rng, n, 10_000, empty=(17,))
    return vals, lab


@pytest.mark.parametrize("func", ["nanmean", "sum"])
def test_past_one_grid_stride(func):
    vals, lab = _big()
    _both(vals, (lab,), func, np.arange(10_000), calls=3)


# ---- functions, dtypes, labels -------------------------------------------

@pytest.mark.parametrize("ldtype", ["int64", "int32"])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("func", FUNCS)
def test_funcs_and_dtypes(func, vdtype, ldtype):
    _run(8 * 1024 + 1, 257, func, vdtype, ldtype, calls=3)


@pytest.mark.parametrize("func", ["mean", "nansum"])
def test_label_cache_off(func):
    with flox_amd.set_options(label_cache=False):
        _run(8 * 1024 + 1, 257, func, "float32", calls=3)


@pytest.mark.parametrize("func,vdtype,ldtype", [("nanmean", "float64", "int64"),
                                                ("sum", "float32", "int32"),
                                                ("count", "int64", "int64")])
def test_two_by(func, vdtype, ldtype):
    rng = np.random.default_rng(zlib.crc32(f"ff-2by-{func}".encode()))
    n = 100_003
    vals = _values(rng, n, vdtype)
    a = rng.integers(0, 12, n).astype(ldtype)
    b = rng.integers(0, 180, n).astype(ldtype)
    k = rng.random(n)
    a[k < 0.01] = -1
    a[(k >= 0.01) & (k < 0.02)] = 12
    b[(k >= 0.02) & (k < 0.03)] = 180
    b[(k >= 0.03) & (k < 0.04)] = -5
    a[(k >= 0.04) & (k < 0.05)] = 13
    b[(k >= 0.04) & (k < 0.05)] = 70_000
    b[(a == 3) & (b == 7)] = -1  # an empty cell
    got = _both(vals, (a, b), func, (np.arange(12), np.arange(180)), calls=3)
    assert got.shape == (12, 180)


def test_every_row_out_of_range():
    rng = np.random.default_rng(5)
    n, ng = 10_007, 300
    vals = _values(rng, n, "float32")
    lab = np.where(rng.random(n) < 0.5, -1, ng + rng.integers(0, 1 << 20, n)).astype("int64")
    for func in FUNCS:
        _both(vals, (lab,), func, np.arange(ng), calls=3)


# ---- dtype= and fills ------------------------------------------------------

@pytest.mark.parametrize("func", ["mean", "nansum", "sum"])
def test_dtype_f64_for_f32_input(func):
    got = _run(8 * 1024 + 1, 257, func, "float32", dtype=np.float64)
    assert got.dtype == torch.float64


@pytest.mark.parametrize("kw", [
    dict(fill_value=-7.5), dict(fill_value=-7.5, min_count=1),
    dict(fill_value=123.0, min_count=3), dict(fill_value=float("nan"), min_count=3),
])
@pytest.mark.parametrize("func,vdtype", [("mean", "float32"), ("nanmean", "float64"),
                                         ("sum", "float32"), ("nansum", "float64"),
                                         ("mean", "int64")])
def test_float_fills(func, vdtype, kw):
    # 257 groups over 600 rows: counts of 0, 1, 2, 3 all occur
    _run(600, 257, func, vdtype, **kw)


@pytest.mark.parametrize("kw", [dict(fill_value=-7), dict(fill_value=-7, min_count=1),
                                dict(fill_value=99, min_count=3)])
@pytest.mark.parametrize("func,vdtype", [("sum", "int64"), ("nansum", "int32"),
                                         ("count", "float32"), ("count", "int64")])
def test_integer_fills(func, vdtype, kw):
    got = _run(600, 257, func, vdtype, **kw)
    assert got.dtype == torch.int64


def test_no_fill_with_min_count_stays_on_the_host_checked_path():
    rng = np.random.default_rng(8)
    vals = _values(rng, 600, "float32")
    lab = _labels(rng, 600, 257)
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    for fused in (None, False):
        with flox_amd.set_options(fused_finalize=fused), _spy() as seen:
            with pytest.raises(ValueError, match="fill_value is None"):
                flox_amd.groupby_reduce(vals_t, lab_t, func="mean", min_count=3,
                                        expected_groups=np.arange(257))
        assert seen == [False]


def test_nan_fill_on_integer_sum_promotes_to_f64():
    got = _run(600, 257, "sum", "int64", expect_fused=False,
               fill_value=float("nan"), min_count=2)
    assert got.dtype == torch.float64 and bool(torch.isnan(got).any())


# ---- partials unchanged -----------------------------------------------------

def _oracle_for(vals, lab, ng, func):
    want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(ng))
    return np.asarray(want)


@pytest.mark.parametrize("n", [1000, 300_007])  # nblocks 1 and many
@pytest.mark.parametrize("ng", [33, 10_000])
@pytest.mark.parametrize("vdtype", ["float32", "int32"])  # 16-20 B bins: 1e4 groups fit LDS
def test_partials_unchanged(vdtype, ng, n):
    rng = np.random.default_rng(zlib.crc32(f"ff-part-{vdtype}-{ng}-{n}".encode()))
    lab = _labels(rng, n, ng, empty=(0, ng // 2))
    isf = np.dtype(vdtype).kind == "f"
    vals = _values(rng, n, vdtype)
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    inr = (lab >= 0) & (lab < ng)
    valid = inr & ~np.isnan(vals) if isf else inr

    def part(op_set, skipnan=False, v=vals_t, **kw):
        p = aggregate_hip.grouped_partials(op_set, v, lab_t, ng, skipnan=skipnan, **kw)
        assert p["_path"] == 1 and "result" not in p
        return {k: _np(t) for k, t in p.items() if k != "_path"}

    count = np.bincount(lab[valid], minlength=ng)
    present = (np.bincount(lab[inr], minlength=ng) > 0).astype(np.int32)
    nanflag = (np.bincount(lab[inr & ~valid], minlength=ng) > 0).astype(np.int32)
    tol = _tol("sum", np.dtype("float64" if isf else "int64"))

    acc = np.float64 if isf else np.int64
    for skip in (False, True):
        rows_in = valid if skip else inr  # a NaN row poisons its group's plain sum
        want = np.zeros(ng, dtype=acc)
        np.add.at(want, lab[rows_in], vals[rows_in].astype(acc))
        p = part(_ffi.SET_SUM_COUNT_PRESENT, skip)
        np.testing.assert_allclose(p["sum"], want, equal_nan=True, **tol)
        np.testing.assert_array_equal(p["count"], count)
        np.testing.assert_array_equal(p["present"], present)
    np.testing.assert_array_equal(part(_ffi.SET_SUM_COUNT)["count"], count)
    np.testing.assert_array_equal(part(_ffi.SET_COUNT)["count"], count)

    # min / max: empty groups hold +inf / -inf (INT_MAX / -INT_MAX)
    hi = np.inf if isf else np.iinfo(vdtype).max
    lo = -np.inf if isf else -np.iinfo(vdtype).max  # the kernels' -pos_inf()
    for op_full, op_cnt, key, ofunc, ident in (
        (_ffi.SET_MIN_FULL, _ffi.SET_MIN_COUNT, "min", "nanmin", hi),
        (_ffi.SET_MAX_FULL, _ffi.SET_MAX_COUNT, "max", "nanmax", lo),
    ):
        want = _oracle_for(vals, lab, ng, ofunc).astype(np.float64)
        want = np.where(count == 0, ident, want).astype(vdtype)
        pf = part(op_full)
        ok = (count > 0) | (present == 0)  # all-NaN groups: the nanflag decides
        np.testing.assert_array_equal(pf[key][ok], want[ok])
        np.testing.assert_array_equal(pf["count"], count)
        np.testing.assert_array_equal(pf["present"], present)
        np.testing.assert_array_equal(pf["nanflag"], nanflag)
        pc = part(op_cnt, True)
        np.testing.assert_array_equal(pc[key], want)
        np.testing.assert_array_equal(pc["count"], count)

    # idxmin / idxmax over all in-range rows: first / last row of each group
    rows = np.arange(n)
    first = np.full(ng, (1 << 63) - 1, dtype=np.int64)
    np.minimum.at(first, lab[inr], rows[inr])
    last = np.full(ng, -1, dtype=np.int64)
    np.maximum.at(last, lab[inr], rows[inr])
    np.testing.assert_array_equal(part(_ffi.SET_IDXMIN)["idx"], first)
    np.testing.assert_array_equal(part(_ffi.SET_IDXMAX)["idx"], last)

    # prod over {-1, 1, 2}: exact in both accumulators
    pv = rng.choice(np.array([-1, 1]), n).astype(vdtype)
    pv[rng.random(n) < 0.001] = 2  # a few doublings per group: no overflow
    pp = part(_ffi.SET_PROD, v=torch.as_tensor(pv).cuda())
    want = np.ones(ng, dtype=np.float64 if isf else np.int64)
    np.multiply.at(want, lab[inr], pv[inr].astype(want.dtype))
    np.testing.assert_array_equal(pp["sum"], want)

    # ssd about the per-group means
    cnt_all = np.maximum(count, 1)
    sums = np.zeros(ng)
    np.add.at(sums, lab[valid], vals[valid].astype(np.float64))
    means = sums / cnt_all
    ps = part(_ffi.SET_SSD, True, means=torch.as_tensor(means).cuda())
    want = np.zeros(ng)
    np.add.at(want, lab[valid], (vals[valid].astype(np.float64) - means[lab[valid]]) ** 2)
    np.testing.assert_allclose(ps["sum"], want, rtol=1e-12, atol=1e-9)


# ---- fold order ---------------------------------------------------------------

def test_fold_order_is_fixed():
    # integer-valued f64 inputs (|sum| < 2^30 * n < 2^50): the LDS atomics are exact in
    # any order, so the slab is the same on every run and any difference
    # between runs would come from the cross-block fold
    rng = np.random.default_rng(3)
    n, ng = 600_011, 33
    vals = torch.as_tensor(rng.integers(-(1 << 30), 1 << 30, n).astype("float64")).cuda()
    lab = torch.as_tensor(rng.integers(0, ng, n)).cuda()
    runs = [aggregate_hip.grouped_partials(_ffi.SET_SUM_COUNT, vals, lab, ng)["sum"].clone()
            for _ in range(2)]
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        other.wait_stream(torch.cuda.default_stream())
        runs.append(aggregate_hip.grouped_partials(_ffi.SET_SUM_COUNT, vals, lab, ng)["sum"].clone())
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    want = np.zeros(ng)
    np.add.at(want, _np(lab), _np(vals))
    np.testing.assert_array_equal(_np(runs[0]), want)


# ---- capture ------------------------------------------------------------------

def test_fused_step_under_graph_capture():
    rng = np.random.default_rng(4)
    n, ng = 100_000, 10_000
    vals = torch.as_tensor(rng.standard_normal(n).astype("float32")).cuda()
    lab = torch.as_tensor(rng.integers(0, ng, n)).cuda()
    expected = np.arange(ng)
    with _spy() as seen:
        eager, *_ = flox_amd.groupby_reduce(vals, lab, func="mean", expected_groups=expected)
    assert seen == [True]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g), _spy() as seen:
            res, *_ = flox_amd.groupby_reduce(vals, lab, func="mean", expected_groups=expected)
    assert seen == [True]
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_allclose(_np(res), _np(eager), equal_nan=True, **_tol("mean", np.float32))


# ---- the C boundary refuses what it cannot finish --------------------------------

def test_finish_off_the_lds_path_is_an_error():
    n, ng = 1000, 33
    vals = torch.zeros(n, dtype=torch.float32, device="cuda")
    lab = torch.zeros(n, dtype=torch.int64, device="cuda")
    # forced global-atomic path: grouped_partials returns partials instead
    p = aggregate_hip.grouped_partials(
        _ffi.SET_SUM_COUNT, vals, lab, ng, force_path=2,
        finish=(_ffi.FINISH_MEAN, torch.float32, 0, None))
    assert "result" not in p and p["_path"] == 2
    # a finish mode that does not belong to the op set: error 14
    with pytest.raises(RuntimeError, match="floxhip error 14"):
        aggregate_hip.grouped_partials(
            _ffi.SET_COUNT, vals, lab, ng,
            finish=(_ffi.FINISH_MEAN, torch.float32, 0, None))
