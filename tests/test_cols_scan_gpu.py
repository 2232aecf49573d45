"""Grouped scans over leading dims in the column kernel (fh_grouped_scan_cols).

Raw kernel results against plain numpy (per group, rows ascending, np.cumsum /
np.nancumsum, a row loop for the fills) and API results against the oracle are
EXACT, f32 sums included: kernel, numpy and oracle all add sequentially in the
value dtype in the same order. Against the fold (cols_scan=False), whose tree
scan associates differently, sums use the tolerances of
tests/test_hip_parity.py::test_scan_vs_oracle; fills are exact everywhere.
"""

import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from oracle import groupby_scan as oracle_scan

pytestmark = pytest.mark.gpu

OPS = {"cumsum": 0, "nancumsum": 1, "ffill": 2, "bfill": 3}
SUMS = ("cumsum", "nancumsum")
FILLS = ("ffill", "bfill")
# (func, dtype) the kernel is instantiated for
KERNEL_CASES = [(f, d) for f in SUMS for d in ("float32", "float64", "int64")] + [
    (f, d) for f in FILLS for d in ("float32", "float64")
]
TTILE = 2048  # rows per staged tile of k_scan_cols
NG = 7


# ---- inputs and the numpy reference ---------------------------------------------------------------------


def _codes(rng, n_t, ng=NG):
    """codes in [1, ng - 1): groups 0 and ng - 1 stay empty, about 5 % of rows
    at -1. Past one staging tile the last non-empty group takes about 60 % of
    the rows: sorted, its run ends at n_t and starts below 2048, so it spans
    one (2049 rows) or two (4101 rows) tile boundaries where one workgroup
    walks all rows."""
    lab = rng.integers(1, max(ng - 1, 2), n_t)
    if n_t > TTILE:
        lab[rng.random(n_t) < 0.6] = ng - 2
    lab[rng.random(n_t) < 0.05] = -1
    return lab.astype(np.int64)


def _values(rng, shape, dtype, codes=None, scale=100):
    """about 10 % NaN in float values; with codes (and enough rows) the planted
    cases: group 1 starts with NaN, group 2 has a NaN in its middle, group 3
    is all NaN, group 4 starts with -0.0 and goes on with +inf, -inf"""
    if np.dtype(dtype).kind != "f":
        return rng.integers(-1000, 1000, shape).astype(dtype)
    v = (rng.standard_normal(shape) * scale).astype(dtype)
    v[rng.random(shape) < 0.10] = np.nan
    if codes is not None and shape[0] >= 257:
        r1, r2, r3, r4 = (np.flatnonzero(codes == g) for g in (1, 2, 3, 4))
        v[r1[0]] = np.nan
        v[r2[0]], v[r2[len(r2) // 2]], v[r2[-1]] = 1.5, np.nan, 2.5
        v[r3] = np.nan
        v[r4[0]], v[r4[1]], v[r4[2]] = -0.0, np.inf, -np.inf
    return v


def _ffill_rows(seg):
    out = seg.copy()
    for i in range(1, len(out)):
        gap = np.isnan(out[i])
        out[i][gap] = out[i - 1][gap]
    return out


def _ref_scan(v, codes, func):
    """per group (the -1 rows are one), rows ascending, column by column"""
    out = np.empty_like(v)
    order = np.argsort(codes, kind="stable")
    sc = codes[order]
    starts = np.flatnonzero(np.concatenate(([True], sc[1:] != sc[:-1])))
    for s0, s1 in zip(starts, np.append(starts[1:], len(sc))):
        rows = order[s0:s1]
        seg = v[rows]
        with np.errstate(all="ignore"):
            if func == "cumsum":
                out[rows] = np.cumsum(seg, axis=0, dtype=v.dtype)
            elif func == "nancumsum":
                out[rows] = np.nancumsum(seg, axis=0, dtype=v.dtype)
            elif func == "ffill":
                out[rows] = _ffill_rows(seg)
            else:
                out[rows] = _ffill_rows(seg[::-1])[::-1]
    return out


def _sorted(codes_np):
    codes = torch.as_tensor(codes_np, dtype=torch.int64).cuda()
    sc, perm = torch.sort(codes, stable=True)
    return sc.to(torch.int32), perm.to(torch.int32)


def _raw(v_t, codes_np, func, out=None):
    sc, perm = _sorted(codes_np)
    return aggregate_hip.grouped_scan_cols(v_t, sc, perm, func, out=out)


def _ffi_call(v_t, sc, perm, op, out_t, *, chunks=None):
    """fh_grouped_scan_cols called directly; chunks None = chunk_offsets NULL.
    Returns the entry's code."""
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.vdtype = aggregate_hip._TORCH_VDTYPE[v_t.dtype]
    c.ldtype = _ffi.L_I32
    c.n, c.m = v_t.shape
    c.ldm = v_t.stride(0)
    c.values = v_t.data_ptr()
    c.labels = sc.data_ptr()
    c.perm = perm.data_ptr()
    c.out_sum = out_t.data_ptr()
    if chunks is not None:
        c.chunk_offsets = chunks.data_ptr()
        c.nchunks = chunks.numel() - 1
    c.stream = torch.cuda.current_stream().cuda_stream
    code = lib.fh_grouped_scan_cols(ctypes.byref(c), op, out_t.stride(0))
    torch.cuda.synchronize()
    if code == 0:
        assert c.path_used == 3
    return code


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ---- the raw kernel -------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (257, 5), (2048, 64), (2049, 65), (4101, 12)])
@pytest.mark.parametrize("func,dtype", KERNEL_CASES)
def test_raw_kernel_equals_numpy(func, dtype, shape):
    rng = np.random.default_rng(zlib.crc32(f"raw-{func}-{dtype}-{shape}".encode()))
    n_t, m = shape
    codes = _codes(rng, n_t)
    v = _values(rng, shape, dtype, codes)
    want = _ref_scan(v, codes, func)
    v_t = torch.as_tensor(v).cuda()
    got = _np(_raw(v_t, codes, func))  # the host's group-aligned chunk plan
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_np(v_t), v)  # the input is read only
    # one workgroup per column tile walks all rows: segments cross the tiles
    sc, perm = _sorted(codes)
    whole = torch.full_like(v_t, 99)
    assert _ffi_call(v_t, sc, perm, OPS[func], whole) == 0
    np.testing.assert_array_equal(_np(whole), want)
    if np.dtype(dtype).kind == "f" and n_t >= 257 and func in SUMS:
        r4 = np.flatnonzero(codes == 4)
        assert np.signbit(got[r4[0]]).all()  # -0.0 as a group's first row survives
        assert np.isnan(got[r4[2]]).all()    # +inf then -inf


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("m", [1, 7, 64, 130])
@pytest.mark.parametrize("func,dtype", [("cumsum", "float32"), ("nancumsum", "int64"),
                                        ("ffill", "float64"), ("bfill", "float32")])
def test_strided_views_and_untouched_padding(func, dtype, m, off):
    """values and output are column slices of wider storage, ldo != ldm, the
    slices start `off` elements in (0: the aligned 16-B vector form with a
    partial last vector; 1, 3: the one-column form)"""
    rng = np.random.default_rng(1000 + 10 * m + off)
    n_t = 300
    ldm = (m + 3 + 3) // 4 * 4 + 4
    ldo = ldm + 4
    codes = _codes(rng, n_t)
    store = _values(rng, (n_t, ldm), dtype)
    store_t = torch.as_tensor(store).cuda()
    v_t = store_t[:, off:off + m]
    assert v_t.stride(0) == ldm
    out_store = torch.full((n_t, ldo), 777, dtype=v_t.dtype, device="cuda")
    out_t = out_store[:, off:off + m]
    res = _raw(v_t, codes, func, out=out_t)
    assert res.data_ptr() == out_t.data_ptr()
    torch.cuda.synchronize()
    want = _ref_scan(store[:, off:off + m], codes, func)
    np.testing.assert_array_equal(_np(out_t), want)
    np.testing.assert_array_equal(_np(store_t), store)
    pad = _np(out_store).copy()
    pad[:, off:off + m] = 777
    assert (pad == 777).all()


@pytest.mark.parametrize("func,dtype", KERNEL_CASES)
def test_one_group_and_no_group(func, dtype):
    rng = np.random.default_rng(7)
    n_t, m = 4101, 12
    v = _values(rng, (n_t, m), dtype)
    v_t = torch.as_tensor(v).cuda()
    for codes in (np.zeros(n_t, dtype=np.int64), np.full(n_t, -1, dtype=np.int64)):
        want = _ref_scan(v, codes, func)  # every row at -1 is one group too
        np.testing.assert_array_equal(_np(_raw(v_t, codes, func)), want)


@pytest.mark.parametrize("func,dtype", [("cumsum", "float32"), ("nancumsum", "float64"),
                                        ("cumsum", "int64"), ("ffill", "float32"),
                                        ("bfill", "float64")])
def test_every_row_its_own_group(func, dtype):
    rng = np.random.default_rng(8)
    n_t, m = 6000, 5  # 6000 groups: no cap on the group count
    codes = rng.permutation(n_t).astype(np.int64)
    v = _values(rng, (n_t, m), dtype)
    want = np.where(np.isnan(v), 0, v) if func == "nancumsum" else v
    np.testing.assert_array_equal(_np(_raw(torch.as_tensor(v).cuda(), codes, func)), want)


def test_int64_sums_wrap():
    rng = np.random.default_rng(9)
    n_t, m = 300, 7
    codes = _codes(rng, n_t)
    v = rng.integers(2**62 - 1000, 2**62, (n_t, m)).astype(np.int64)
    want = _ref_scan(v, codes, "cumsum")
    assert (want < 0).any()  # positive terms: a negative sum has wrapped
    for func in SUMS:
        np.testing.assert_array_equal(_np(_raw(torch.as_tensor(v).cuda(), codes, func)), want)


@pytest.mark.parametrize("func,dtype", KERNEL_CASES)
def test_chunk_plan_and_single_walk_agree_bit_for_bit(func, dtype):
    rng = np.random.default_rng(10)
    n_t, m = 4101, 12
    codes = _codes(rng, n_t, ng=40)
    v = _values(rng, (n_t, m), dtype)
    v_t = torch.as_tensor(v).cuda()
    planned = _raw(v_t, codes, func)
    sc, perm = _sorted(codes)
    whole = torch.empty_like(v_t)
    assert _ffi_call(v_t, sc, perm, OPS[func], whole) == 0
    # explicit group-aligned chunks through the entry as well
    edges = np.flatnonzero(np.diff(_np(sc))) + 1
    chunks = torch.as_tensor(np.concatenate(([0], edges[::3], [n_t])), dtype=torch.int64).cuda()
    mine = torch.empty_like(v_t)
    assert _ffi_call(v_t, sc, perm, OPS[func], mine, chunks=chunks) == 0
    bits = np.int32 if v.itemsize == 4 else np.int64
    for other in (whole, mine):
        np.testing.assert_array_equal(_np(other).view(bits), _np(planned).view(bits))


# ---- ABI refusals ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,code", [
    ("no_out", 22), ("no_perm", 22), ("no_values", 22),
    ("op4", 24), ("i32", 24), ("ffill_i64", 24), ("rows_beyond_int32", 23),
])
def test_refusals_leave_the_output_untouched(case, code):
    rng = np.random.default_rng(11)
    n_t, m = 64, 5
    codes = _codes(rng, n_t)
    sc, perm = _sorted(codes)
    dt = {"i32": torch.int32, "ffill_i64": torch.int64}.get(case, torch.float32)
    v_t = torch.ones((n_t, m), dtype=dt, device="cuda")
    out_t = torch.full((n_t, m), 55, dtype=dt, device="cuda")
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.vdtype = aggregate_hip._TORCH_VDTYPE[dt]
    c.ldtype = _ffi.L_I32
    c.n, c.m, c.ldm = n_t, m, m
    c.values, c.labels, c.perm = v_t.data_ptr(), sc.data_ptr(), perm.data_ptr()
    c.out_sum = out_t.data_ptr()
    c.stream = torch.cuda.current_stream().cuda_stream
    op = 0
    if case == "no_out":
        c.out_sum = None
    elif case == "no_perm":
        c.perm = None
    elif case == "no_values":
        c.values = None
    elif case == "op4":
        op = 4
    elif case == "ffill_i64":
        op = 2
    elif case == "rows_beyond_int32":
        c.n = 2**31
    assert lib.fh_grouped_scan_cols(ctypes.byref(c), op, m) == code
    torch.cuda.synchronize()
    assert (out_t == 55).all()
    with pytest.raises(RuntimeError, match=f"floxhip error {code}: fh_grouped_scan_cols"):
        _ffi.check(code)


# ---- the API ----------------------------------------------------------------------------------------------


@contextlib.contextmanager
def _spy():
    """records ("cols", values data_ptr, row stride) for every
    grouped_scan_cols call and ("1d",) for every fh_grouped_scan call"""
    seen = []
    lib = _ffi.load_library()
    orig_cols = aggregate_hip.grouped_scan_cols
    orig_1d = lib.fh_grouped_scan

    def cols(values2d, *a, **kw):
        seen.append(("cols", values2d.data_ptr(), values2d.stride(0)))
        return orig_cols(values2d, *a, **kw)

    def one_d(*a):
        seen.append(("1d",))
        return orig_1d(*a)

    aggregate_hip.grouped_scan_cols = cols
    lib.fh_grouped_scan = one_d
    try:
        yield seen
    finally:
        aggregate_hip.grouped_scan_cols = orig_cols
        lib.fh_grouped_scan = orig_1d


def _kinds(seen):
    return [s[0] for s in seen]


def _fold_tol(dtype):
    # tests/test_hip_parity.py::test_scan_vs_oracle
    dt = np.dtype(dtype)  # of the input: dtype= casts a result computed in it
    if dt.kind != "f":
        return dict(rtol=0, atol=0)
    return dict(rtol=1e-4, atol=1e-4) if dt.itemsize == 4 else dict(rtol=1e-12, atol=1e-10)


def _api_values(rng, shape, dtype):
    if dtype == "bool":
        return rng.random(shape) < 0.4
    if dtype == "uint8":
        return rng.integers(0, 255, shape).astype(np.uint8)
    # unit scale, as test_scan_vs_oracle draws them: the fold's tolerances
    # (atol 1e-4 for f32) are stated for running sums of that size
    return _values(rng, shape, dtype, scale=1)


def _layouts(rng, dtype):
    """(storage, array view) pairs: storage is time-major, the array is its
    permute view with the grouped axis last"""
    a = _api_values(rng, (4101, 12), dtype)        # (12, 4101).T-style
    b = _api_values(rng, (300, 3, 4), dtype)       # three leading dims
    return [(a, (1, 0)), (b, (1, 2, 0))]


# bool and uint8 for the sums only
API_CASES = [(f, d) for f in OPS for d in ("float32", "float64", "int32", "int64")] + [
    (f, d) for f in SUMS for d in ("bool", "uint8")
]


@pytest.mark.parametrize("func,dtype", API_CASES)
def test_api_parity(func, dtype):
    rng = np.random.default_rng(zlib.crc32(f"api-{func}-{dtype}".encode()))
    as_tensor = dtype != "uint8"  # torch uint8 values are not a scan dtype; numpy ones promote
    # the kernel's dtypes after promotion: these calls must take the column form
    # (integer fills keep the fold)
    served = as_tensor and (dtype in ("float32", "float64") or func in SUMS)
    for store, perm_dims in _layouts(rng, dtype):
        n = store.shape[0]
        arr_np = np.transpose(store, perm_dims)
        by1 = rng.integers(0, NG + 2, n)  # NG, NG + 1 fall outside expected_groups
        by2a, by2b = rng.integers(0, 4, n), rng.integers(0, 3, n)
        variants = [
            ((by1,), dict(expected_groups=np.arange(NG))),
            ((by1,), dict()),
            ((by2a, by2b), dict(expected_groups=(np.arange(3), np.arange(3)))),
            ((by2a, by2b), dict()),
        ]
        if np.dtype(dtype).kind == "f":
            variants.append(((by1,), dict(expected_groups=np.arange(NG), dtype=np.float64)))
        for bys, kw in variants:
            want = oracle_scan(arr_np, *bys, func=func, **kw)
            inputs = [(arr_np, bys)]
            if as_tensor:
                arr_t = torch.as_tensor(store).cuda().permute(*perm_dims)
                inputs.append((arr_t, tuple(torch.as_tensor(b).cuda() for b in bys)))
            for arr, bb in inputs:
                with flox_amd.set_options(cols_scan_min_cols=1), _spy() as seen:
                    got = flox_amd.groupby_scan(arr, *bb, func=func, **kw)
                if isinstance(arr, torch.Tensor) and served:
                    assert _kinds(seen) == ["cols"], (_kinds(seen), kw)
                with flox_amd.set_options(cols_scan=False), _spy() as seen_off:
                    fold = flox_amd.groupby_scan(arr, *bb, func=func, **kw)
                assert _kinds(seen_off) == ["1d"]
                assert isinstance(got, type(fold))
                got, fold = _np(got), _np(fold)
                assert got.shape == want.shape == fold.shape
                assert got.dtype == want.dtype == fold.dtype, (got.dtype, want.dtype, fold.dtype)
                if "cols" in _kinds(seen):
                    np.testing.assert_array_equal(got, want)  # exact, f32 sums included
                else:
                    np.testing.assert_allclose(got, want, equal_nan=True, **_fold_tol(dtype))
                if func in FILLS:
                    np.testing.assert_array_equal(got, fold)
                else:
                    np.testing.assert_allclose(got, fold, equal_nan=True, **_fold_tol(dtype))


def test_spy_column_entry_runs_once_on_the_callers_view():
    rng = np.random.default_rng(21)
    store = torch.as_tensor(_values(rng, (4101, 12), "float32")).cuda()
    arr = store.permute(1, 0)
    lab = torch.as_tensor(rng.integers(0, NG, 4101)).cuda()
    with flox_amd.set_options(cols_scan_min_cols=1), _spy() as seen:
        got = flox_amd.groupby_scan(arr, lab, func="cumsum", expected_groups=np.arange(NG))
    assert seen == [("cols", store.data_ptr(), 12)]
    assert got.shape == arr.shape and got.dtype == arr.dtype
    want = oracle_scan(_np(arr), _np(lab), func="cumsum", expected_groups=np.arange(NG))
    np.testing.assert_array_equal(_np(got), want)


@pytest.mark.parametrize("func", list(OPS))
def test_stable_order_interleaved_labels(func):
    """a scan depends on the row order inside a group: interleaved labels
    against a per-column Python loop; bfill = ffill of the reversed rows"""
    rng = np.random.default_rng(22)
    n_t, m = 600, 6
    v = _values(rng, (n_t, m), "float64")
    lab = np.arange(n_t) % 3  # rows of the three groups interleave
    arr = torch.as_tensor(v).cuda().permute(1, 0)
    with flox_amd.set_options(cols_scan_min_cols=1), _spy() as seen:
        got = _np(flox_amd.groupby_scan(arr, torch.as_tensor(lab).cuda(), func=func))
    assert _kinds(seen) == ["cols"]
    want = np.empty_like(v)
    for col in range(m):
        for g in range(3):
            rows = range(g, n_t, 3) if func != "bfill" else range(n_t - 3 + g, -1, -3)
            acc, first = None, True
            for r in rows:
                x = v[r, col]
                if func in FILLS:
                    acc = x if (first or not np.isnan(x)) else acc
                else:
                    x = 0.0 if (func == "nancumsum" and np.isnan(x)) else x
                    acc = x if first else acc + x
                first = False
                want[r, col] = acc
    np.testing.assert_array_equal(got.T, want)
    if func == "bfill":
        rev = torch.as_tensor(v[::-1].copy()).cuda().permute(1, 0)
        with flox_amd.set_options(cols_scan_min_cols=1):
            ff = _np(flox_amd.groupby_scan(rev, torch.as_tensor(lab[::-1].copy()).cuda(), func="ffill"))
        np.testing.assert_array_equal(got, ff[:, ::-1])


# ---- what keeps the fold --------------------------------------------------------------------------------


def _fold_only(arr, lab, func, opts, **kw):
    """the call under `opts` launches only the fold and equals the
    cols_scan=False result exactly"""
    with flox_amd.set_options(**opts), _spy() as seen:
        got = flox_amd.groupby_scan(arr, lab, func=func, **kw)
    assert _kinds(seen) == ["1d"], _kinds(seen)
    with flox_amd.set_options(cols_scan=False):
        off = flox_amd.groupby_scan(arr, lab, func=func, **kw)
    got, off = _np(got), _np(off)
    assert got.dtype == off.dtype and got.shape == off.shape
    np.testing.assert_array_equal(got, off)


def _whole_floats(rng, shape):
    # whole-number f32: every partial sum is exact under any association
    return rng.integers(-50, 50, shape).astype(np.float32)


def test_fallback_c_contiguous_lead_layout():
    rng = np.random.default_rng(31)
    arr = torch.as_tensor(_whole_floats(rng, (5, 300))).cuda()
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    for func in OPS:
        _fold_only(arr, lab, func, dict(cols_scan_min_cols=1), expected_groups=np.arange(NG))


def test_fallback_datetime_values():
    rng = np.random.default_rng(32)
    v = rng.integers(0, 10**6, (300, 5)).astype("timedelta64[s]")
    lab = rng.integers(0, NG, 300)
    for func in ("cumsum", "ffill"):
        _fold_only(v.T, lab, func, dict(cols_scan_min_cols=1), expected_groups=np.arange(NG))


def test_fallback_integer_fill():
    rng = np.random.default_rng(33)
    arr = torch.as_tensor(rng.integers(-9, 9, (300, 5))).cuda().permute(1, 0)
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    for func in FILLS:
        _fold_only(arr, lab, func, dict(cols_scan_min_cols=1), expected_groups=np.arange(NG))


def test_fallback_option_off_and_narrow_arrays():
    rng = np.random.default_rng(34)
    arr = torch.as_tensor(_whole_floats(rng, (300, 5))).cuda().permute(1, 0)
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    for func in OPS:
        _fold_only(arr, lab, func, dict(cols_scan=False, cols_scan_min_cols=1))
        _fold_only(arr, lab, func, dict(cols_scan_min_cols=6))  # lead_M = 5
        with flox_amd.set_options(cols_scan_min_cols=5), _spy() as seen:
            flox_amd.groupby_scan(arr, lab, func=func)
        assert _kinds(seen) == ["cols"]


@pytest.mark.parametrize("func", ["cumsum", "ffill"])
def test_fallback_capture_replays_the_eager_result(func):
    # the chunk plan reads the sorted codes on the host, which a capturing
    # stream cannot: the fold runs
    rng = np.random.default_rng(35)
    v = _whole_floats(rng, (4101, 12))
    v[rng.random(v.shape) < 0.05] = np.nan
    arr = torch.as_tensor(v).cuda().permute(1, 0)
    lab = torch.as_tensor(rng.integers(0, NG, 4101)).cuda()
    kw = dict(func=func, expected_groups=np.arange(NG))
    with flox_amd.set_options(cols_scan_min_cols=1):
        with _spy() as seen:
            eager = flox_amd.groupby_scan(arr, lab, **kw)
        assert _kinds(seen) == ["cols"]
        with flox_amd.set_options(cols_scan=False):
            off = flox_amd.groupby_scan(arr, lab, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g), _spy() as seen:
                res = flox_amd.groupby_scan(arr, lab, **kw)
        assert _kinds(seen) == ["1d"]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(res), _np(eager))
        np.testing.assert_array_equal(_np(res), _np(off))


# ---- beyond 2^32 elements -------------------------------------------------------------------------------


def test_beyond_2_32_elements():
    n_t, m = 2**11, 2**21 + 64
    assert n_t * m > 2**32
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 48 * 2**30:
        pytest.skip("needs 48 GiB of free device memory")
    g0 = torch.Generator(device="cuda").manual_seed(5)
    vt = torch.empty((n_t, m), dtype=torch.float32, device="cuda")
    step = 256  # fill in row blocks: the int8 draw never holds more than 0.5 GiB
    for r in range(0, n_t, step):
        vt[r:r + step] = torch.randint(0, 7, (step, m), dtype=torch.int8, device="cuda", generator=g0)
    lab = torch.arange(n_t, device="cuda") % 3
    with _spy() as seen:  # the default gate: this width is far above any minimum
        got = flox_amd.groupby_scan(vt.permute(1, 0), lab, func="cumsum")
    assert seen == [("cols", vt.data_ptr(), m)]
    assert got.shape == (m, n_t) and got.dtype == torch.float32
    res = got.permute(1, 0)
    # every partial sum is a whole number below 2^24: exact in f32
    for c0 in (0, m // 2 - 2048, m - 4096):
        for g in range(3):
            want = torch.cumsum(vt[g::3, c0:c0 + 4096], 0)
            assert torch.equal(res[g::3, c0:c0 + 4096], want), (c0, g)
    del got, res, vt
    torch.cuda.empty_cache()
