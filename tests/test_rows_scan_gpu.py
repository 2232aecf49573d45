"""Grouped scans over leading dims in the row kernel (fh_grouped_scan_rows):
the C-contiguous (lead..., N) layout, grouped axis last.

Raw kernel results against plain numpy (tests/test_cols_scan_gpu.py::_ref_scan
applied per lead row: per group, time ascending, np.cumsum / np.nancumsum in
the value dtype, a row loop for the fills) and API results against the oracle
are EXACT, f32 sums included: kernel, numpy and oracle all add sequentially in
the value dtype in the same order. Against the fold (rows_scan=False), whose
tree scan associates differently, sums use the tolerances of
tests/test_hip_parity.py::test_scan_vs_oracle; fills are exact everywhere.
Tile extents come from fh_scan_rows_plan.
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
from tests.test_cols_scan_gpu import _api_values, _fold_tol, _np, _ref_scan, _whole_floats

pytestmark = pytest.mark.gpu

OPS = {"cumsum": 0, "nancumsum": 1, "ffill": 2, "bfill": 3}
SUMS = ("cumsum", "nancumsum")
FILLS = ("ffill", "bfill")
# (func, dtype) the kernel is instantiated for
KERNEL_CASES = [(f, d) for f in SUMS for d in ("float32", "float64", "int64")] + [
    (f, d) for f in FILLS for d in ("float32", "float64")
]
NG = 7
PLANT_MIN = 24  # time steps from which groups 1..4 have three steps each
VD = {"float32": _ffi.F32, "float64": _ffi.F64, "int64": _ffi.I64}


def _plan(dtype, ng=NG):
    """(R, T): lead rows per workgroup and time steps per tile for the case"""
    return _ffi.scan_rows_plan(VD[str(dtype)], ng)


def _shapes(dtype, ng=NG):
    R, T = _plan(dtype, ng)
    return [(1, 1), (2, 3), (R - 1, T - 1), (R, T), (R + 1, T + 1), (5, 2 * T + 5),
            (2 * R + 3, 7)]


# ---- inputs and the numpy reference ---------------------------------------------------------------------


def _codes(rng, n, T, ng=NG):
    """codes in [1, ng - 1): groups 0 and ng - 1 stay empty, about 5 % of steps
    at -1. Past one time tile the last non-empty group takes about 60 % of the
    steps, so its carry crosses tile boundaries (and is parked and fetched
    again wherever another group's step interrupts it). From PLANT_MIN steps
    groups 1..4 have at least three steps each."""
    lab = rng.integers(1, max(ng - 1, 2), n)
    if n > T:
        lab[rng.random(n) < 0.6] = ng - 2
    lab[rng.random(n) < 0.05] = -1
    if n >= PLANT_MIN and ng >= 6:
        lab[rng.permutation(n)[:12]] = np.repeat([1, 2, 3, 4], 3)  # _values plants in these
    return lab.astype(np.int64)


def _values(rng, shape, dtype, codes=None):
    """(m, n) values, about 10 % NaN in floats; with codes whose groups 1..4
    have three steps each, the planted cases in every row: group 1 starts with
    NaN, group 2 has a NaN in its middle, group 3 is all NaN, group 4 starts
    with -0.0 and goes on with +inf, -inf"""
    if np.dtype(dtype).kind != "f":
        return rng.integers(-1000, 1000, shape).astype(dtype)
    v = (rng.standard_normal(shape) * 100).astype(dtype)
    v[rng.random(shape) < 0.10] = np.nan
    if codes is not None:
        t1, t2, t3, t4 = (np.flatnonzero(codes == g) for g in (1, 2, 3, 4))
        if min(len(t1), len(t2), len(t3), len(t4)) >= 3:
            v[:, t1[0]] = np.nan
            v[:, t2[0]], v[:, t2[len(t2) // 2]], v[:, t2[-1]] = 1.5, np.nan, 2.5
            v[:, t3] = np.nan
            v[:, t4[0]], v[:, t4[1]], v[:, t4[2]] = -0.0, np.inf, -np.inf
    return v


def _ref_rows(v, codes, func):
    """_ref_scan takes (time, columns): every lead row is a column of v.T"""
    return np.ascontiguousarray(_ref_scan(np.ascontiguousarray(v.T), codes, func).T)


def _codes_t(codes_np):
    return torch.as_tensor(codes_np, dtype=torch.int32).cuda()


def _raw(v_t, codes_np, func, ng=NG, out=None):
    return aggregate_hip.grouped_scan_rows(v_t, _codes_t(codes_np), ng, func, out=out)


def _ffi_call(v_t, codes_t, ng, op, out_t, **over):
    """fh_grouped_scan_rows called directly; `over` overrides fh_call fields
    (and `ldo`). Returns the entry's code."""
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.vdtype = aggregate_hip._TORCH_VDTYPE[v_t.dtype]
    c.ldtype = _ffi.L_I32
    c.m, c.n = v_t.shape
    c.ngroups = ng
    c.ldm = v_t.stride(0)
    c.values = v_t.data_ptr()
    c.labels = codes_t.data_ptr()
    c.out_sum = out_t.data_ptr()
    c.stream = torch.cuda.current_stream().cuda_stream
    ldo = over.pop("ldo", out_t.stride(0))
    for k, val in over.items():
        setattr(c, k, val)
    code = lib.fh_grouped_scan_rows(ctypes.byref(c), op, ldo)
    torch.cuda.synchronize()
    if code == 0:
        assert c.path_used == 3
    return code


# ---- the raw kernel -------------------------------------------------------------------------------------


@pytest.mark.parametrize("si", range(7))
@pytest.mark.parametrize("func,dtype", KERNEL_CASES)
def test_raw_kernel_equals_numpy(func, dtype, si):
    R, T = _plan(dtype)
    m, n = _shapes(dtype)[si]
    rng = np.random.default_rng(zlib.crc32(f"rows-raw-{func}-{dtype}-{si}".encode()))
    codes = _codes(rng, n, T)
    v = _values(rng, (m, n), dtype, codes)
    want = _ref_rows(v, codes, func)
    v_t = torch.as_tensor(v).cuda()
    got = _np(_raw(v_t, codes, func))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_np(v_t), v)  # the input is read only
    t4 = np.flatnonzero(codes == 4)
    if np.dtype(dtype).kind == "f" and func in SUMS and n >= PLANT_MIN:
        assert np.signbit(got[:, t4[0]]).all()  # -0.0 as a group's first step survives
        assert np.isnan(got[:, t4[2]]).all()    # +inf then -inf


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("func,dtype", [("cumsum", "float32"), ("nancumsum", "int64"),
                                        ("ffill", "float64"), ("bfill", "float32")])
def test_strided_views_and_untouched_padding(func, dtype, off):
    """values and output are slices of wider rows with different row strides.
    off = 1: row stride n + 3 and a base one element in, so no 16-byte
    alignment holds (the element-wise form). off = 0: strides that are whole
    vectors on an aligned base with n no multiple of the vector (the 16-B form
    with a partial last vector)."""
    R, T = _plan(dtype)
    m, n = R + 1, 2 * T + 5
    rng = np.random.default_rng(2000 + off)
    codes = _codes(rng, n, T)
    ldm = n + 3 if off else (n + 3 + 7) // 8 * 8
    ldo = ldm + (2 if off else 8)
    store = _values(rng, (m * ldm + off,), dtype)
    store_t = torch.as_tensor(store).cuda()
    v_t = store_t[off:].view(m, ldm)[:, :n]
    assert v_t.stride() == (ldm, 1)
    assert (v_t.data_ptr() % 16 != 0) == bool(off)
    out_store = torch.full((m * ldo + off,), 777, dtype=v_t.dtype, device="cuda")
    out_t = out_store[off:].view(m, ldo)[:, :n]
    res = _raw(v_t, codes, func, out=out_t)
    assert res.data_ptr() == out_t.data_ptr()
    torch.cuda.synchronize()
    v = store[off:].reshape(m, ldm)[:, :n]
    np.testing.assert_array_equal(_np(out_t), _ref_rows(v, codes, func))
    np.testing.assert_array_equal(_np(store_t), store)
    pad = _np(out_store).copy()
    pad[off:].reshape(m, ldo)[:, :n] = 777
    assert (pad == 777).all()


@pytest.mark.parametrize("func,dtype", KERNEL_CASES)
def test_one_group_all_sentinel_and_every_step_its_own_group(func, dtype):
    R, T = _plan(dtype)
    rng = np.random.default_rng(7)
    m, n = 5, 2 * T + 5
    v = _values(rng, (m, n), dtype)
    v_t = torch.as_tensor(v).cuda()
    for codes in (np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)):
        want = _ref_rows(v, codes, func)  # every step at -1 is one group too
        np.testing.assert_array_equal(_np(_raw(v_t, codes, func, ng=1)), want)
    codes = rng.permutation(n).astype(np.int64)
    assert n <= _ffi.scan_rows_max_groups(VD[dtype])
    want = np.where(np.isnan(v), 0, v) if func == "nancumsum" else v
    np.testing.assert_array_equal(_np(_raw(v_t, codes, func, ng=n)), want)


@pytest.mark.parametrize("func,dtype", [("cumsum", "float32"), ("bfill", "float32"),
                                        ("nancumsum", "float64"), ("ffill", "float64")])
def test_group_count_at_capacity_and_one_beyond(func, dtype):
    mg = _ffi.scan_rows_max_groups(VD[dtype])
    R, T = _plan(dtype, mg)
    assert R < _plan(dtype)[0]  # the row tile has shrunk
    rng = np.random.default_rng(8)
    m, n = R + 1, 2 * T + 5
    codes = rng.integers(0, mg, n).astype(np.int64)
    codes[:6] = [mg - 1, 0, mg - 1, -1, 0, mg - 1]  # the last slot's carry is used
    v = _values(rng, (m, n), dtype)
    v_t = torch.as_tensor(v).cuda()
    np.testing.assert_array_equal(_np(_raw(v_t, codes, func, ng=mg)), _ref_rows(v, codes, func))
    out_t = torch.full_like(v_t, 55)
    assert _ffi_call(v_t, _codes_t(codes), mg + 1, OPS[func], out_t) == 25
    assert (out_t == 55).all()
    with pytest.raises(RuntimeError, match="floxhip error 25: fh_grouped_scan_rows"):
        _raw(v_t, codes, func, ng=mg + 1)


def test_max_groups_by_dtype():
    mg = {d: _ffi.scan_rows_max_groups(v) for d, v in VD.items()}
    assert mg["float64"] == mg["int64"] <= mg["float32"]
    assert _ffi.scan_rows_max_groups(_ffi.I32) == 0


def test_int64_sums_wrap():
    R, T = _plan("int64")
    rng = np.random.default_rng(9)
    m, n = 7, 2 * T + 5
    codes = _codes(rng, n, T)
    v = rng.integers(2**62 - 1000, 2**62, (m, n)).astype(np.int64)
    want = _ref_rows(v, codes, "cumsum")
    assert (want < 0).any()  # positive terms: a negative sum has wrapped
    for func in SUMS:
        np.testing.assert_array_equal(_np(_raw(torch.as_tensor(v).cuda(), codes, func)), want)


# ---- ABI refusals ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,code", [
    ("no_out", 22), ("no_labels", 22), ("no_values", 22),
    ("steps_beyond_int32", 23), ("negative_rows", 23), ("ldm_below_n", 23), ("ldo_below_n", 23),
    ("op4", 24), ("op_neg", 24), ("i32", 24), ("ffill_i64", 24),
])
def test_refusals_leave_the_output_untouched(case, code):
    rng = np.random.default_rng(11)
    m, n = 5, 64
    codes_t = _codes_t(_codes(rng, n, 64))
    dt = {"i32": torch.int32, "ffill_i64": torch.int64}.get(case, torch.float32)
    v_t = torch.ones((m, n), dtype=dt, device="cuda")
    out_t = torch.full((m, n), 55, dtype=dt, device="cuda")
    op, over = 0, {}
    if case == "no_out":
        over["out_sum"] = None
    elif case == "no_labels":
        over["labels"] = None
    elif case == "no_values":
        over["values"] = None
    elif case == "steps_beyond_int32":
        over.update(n=2**31, ldm=2**31, ldo=2**31)
    elif case == "negative_rows":
        over["m"] = -1
    elif case == "ldm_below_n":
        over["ldm"] = n - 1
    elif case == "ldo_below_n":
        over["ldo"] = n - 1
    elif case == "op4":
        op = 4
    elif case == "op_neg":
        op = -1
    elif case == "ffill_i64":
        op = 2
    assert _ffi_call(v_t, codes_t, NG, op, out_t, **over) == code
    assert (out_t == 55).all()
    with pytest.raises(RuntimeError, match=f"floxhip error {code}: fh_grouped_scan_rows"):
        _ffi.check(code, _ffi._SCAN_ROWS_ERRORS)


# ---- the API ----------------------------------------------------------------------------------------------


@contextlib.contextmanager
def _spy():
    """records ("rows", values data_ptr, row stride) for every
    grouped_scan_rows call, ("cols",) for every grouped_scan_cols call and
    ("1d",) for every fh_grouped_scan call"""
    seen = []
    lib = _ffi.load_library()
    orig_rows = aggregate_hip.grouped_scan_rows
    orig_cols = aggregate_hip.grouped_scan_cols
    orig_1d = lib.fh_grouped_scan

    def rows(values2d, *a, **kw):
        seen.append(("rows", values2d.data_ptr(), values2d.stride(0)))
        return orig_rows(values2d, *a, **kw)

    def cols(*a, **kw):
        seen.append(("cols",))
        return orig_cols(*a, **kw)

    def one_d(*a):
        seen.append(("1d",))
        return orig_1d(*a)

    aggregate_hip.grouped_scan_rows = rows
    aggregate_hip.grouped_scan_cols = cols
    lib.fh_grouped_scan = one_d
    try:
        yield seen
    finally:
        aggregate_hip.grouped_scan_rows = orig_rows
        aggregate_hip.grouped_scan_cols = orig_cols
        lib.fh_grouped_scan = orig_1d


def _kinds(seen):
    return [s[0] for s in seen]


# bool and uint8 for the sums only
API_CASES = [(f, d) for f in OPS for d in ("float32", "float64", "int32", "int64")] + [
    (f, d) for f in SUMS for d in ("bool", "uint8")
]


@pytest.mark.parametrize("func,dtype", API_CASES)
def test_api_parity(func, dtype):
    rng = np.random.default_rng(zlib.crc32(f"rows-api-{func}-{dtype}".encode()))
    as_tensor = dtype != "uint8"  # torch uint8 values are not a scan dtype; numpy ones promote
    # the kernel's dtypes after promotion: these calls must take the row form
    # (integer fills keep the fold)
    served = dtype in ("float32", "float64") or func in SUMS
    same_storage = dtype in ("float32", "float64", "int64")  # no promoted copy
    for shape in ((12, 4101), (3, 4, 300)):
        arr_np = _api_values(rng, shape, dtype)
        n = shape[-1]
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
                inputs.append((torch.as_tensor(arr_np).cuda(),
                               tuple(torch.as_tensor(b).cuda() for b in bys)))
            for arr, bb in inputs:
                with flox_amd.set_options(rows_scan_min_rows=1), _spy() as seen:
                    got = flox_amd.groupby_scan(arr, *bb, func=func, **kw)
                if served:
                    assert _kinds(seen) == ["rows"], (_kinds(seen), kw)
                    if isinstance(arr, torch.Tensor) and same_storage:
                        assert seen[0][1:] == (arr.data_ptr(), n)
                else:
                    assert _kinds(seen) == ["1d"], (_kinds(seen), kw)
                with flox_amd.set_options(rows_scan=False), _spy() as seen_off:
                    fold = flox_amd.groupby_scan(arr, *bb, func=func, **kw)
                assert _kinds(seen_off) == ["1d"]
                assert isinstance(got, type(fold))
                got, fold = _np(got), _np(fold)
                assert got.shape == want.shape == fold.shape
                assert got.dtype == want.dtype == fold.dtype, (got.dtype, want.dtype, fold.dtype)
                if served:
                    np.testing.assert_array_equal(got, want)  # exact, f32 sums included
                else:
                    np.testing.assert_allclose(got, want, equal_nan=True, **_fold_tol(dtype))
                if func in FILLS:
                    np.testing.assert_array_equal(got, fold)
                else:
                    np.testing.assert_allclose(got, fold, equal_nan=True, **_fold_tol(dtype))


def test_sliced_row_stride_is_read_in_place():
    rng = np.random.default_rng(21)
    wide = torch.as_tensor(_values(rng, (3, 4, 333), "float32")).cuda()
    arr = wide[:, :, :300]  # row stride 333 > N
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    with flox_amd.set_options(rows_scan_min_rows=1), _spy() as seen:
        got = flox_amd.groupby_scan(arr, lab, func="cumsum", expected_groups=np.arange(NG))
    assert seen == [("rows", wide.data_ptr(), 333)]
    assert got.shape == arr.shape and got.dtype == arr.dtype
    want = oracle_scan(_np(arr), _np(lab), func="cumsum", expected_groups=np.arange(NG))
    np.testing.assert_array_equal(_np(got), want)


@pytest.mark.parametrize("func", list(OPS))
def test_stable_order_interleaved_labels(func):
    """a scan depends on the time order inside a group: cyclic labels against
    a scalar Python loop; bfill = ffill of the reversed array, reversed"""
    rng = np.random.default_rng(22)
    m, n = 6, 600
    v = _values(rng, (m, n), "float64")
    lab = np.arange(n) % 3  # steps of the three groups interleave
    with flox_amd.set_options(rows_scan_min_rows=1), _spy() as seen:
        got = _np(flox_amd.groupby_scan(torch.as_tensor(v).cuda(), torch.as_tensor(lab).cuda(),
                                        func=func))
    assert _kinds(seen) == ["rows"]
    want = np.empty_like(v)
    for r in range(m):
        for g in range(3):
            steps = range(g, n, 3) if func != "bfill" else range(n - 3 + g, -1, -3)
            acc, first = None, True
            for t in steps:
                x = v[r, t]
                if func in FILLS:
                    acc = x if (first or not np.isnan(x)) else acc
                else:
                    x = 0.0 if (func == "nancumsum" and np.isnan(x)) else x
                    acc = x if first else acc + x
                first = False
                want[r, t] = acc
    np.testing.assert_array_equal(got, want)
    if func == "bfill":
        with flox_amd.set_options(rows_scan_min_rows=1):
            ff = _np(flox_amd.groupby_scan(torch.as_tensor(v[:, ::-1].copy()).cuda(),
                                           torch.as_tensor(lab[::-1].copy()).cuda(), func="ffill"))
        np.testing.assert_array_equal(got, ff[:, ::-1])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("func", list(OPS))
def test_same_bits_as_the_column_form(func, dtype):
    rng = np.random.default_rng(23)
    n, m = 4101, 12
    store = _values(rng, (n, m), dtype)  # time-major
    lab = torch.as_tensor(rng.integers(0, NG + 2, n)).cuda()
    kw = dict(func=func, expected_groups=np.arange(NG))
    view = torch.as_tensor(store).cuda().permute(1, 0)
    with flox_amd.set_options(cols_scan_min_cols=1), _spy() as seen:
        by_cols = flox_amd.groupby_scan(view, lab, **kw)
    assert _kinds(seen) == ["cols"]
    contig = torch.as_tensor(np.ascontiguousarray(store.T)).cuda()
    with flox_amd.set_options(rows_scan_min_rows=1), _spy() as seen:
        by_rows = flox_amd.groupby_scan(contig, lab, **kw)
    assert _kinds(seen) == ["rows"]
    bits = np.int32 if store.itemsize == 4 else np.int64
    np.testing.assert_array_equal(_np(by_rows.contiguous()).view(bits),
                                  _np(by_cols.contiguous()).view(bits))


def test_no_copy_no_scratch():
    """a condition, not a measurement: the fold on this shape needs hundreds of
    MiB, and a transposed copy would double the array"""
    m, n = 4096, 2048
    g0 = torch.Generator(device="cuda").manual_seed(4)
    # whole numbers: torch.cumsum, which associates differently, is exact on them
    arr = torch.randint(0, 7, (m, n), device="cuda", generator=g0).to(torch.float32)
    lab = torch.arange(n, device="cuda") % 24
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with _spy() as seen:
        got = flox_amd.groupby_scan(arr, lab, func="cumsum", expected_groups=np.arange(24))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert seen == [("rows", arr.data_ptr(), n)]
    assert peak - before <= got.numel() * got.element_size() + 64 * n + 2**20, peak - before
    for g in (0, 23):
        assert torch.equal(got[:8, g::24], torch.cumsum(arr[:8, g::24], 1))


# ---- what keeps the fold --------------------------------------------------------------------------------


def _fold_only(arr, lab, func, opts, **kw):
    """the call under `opts` launches only the fold and equals the
    rows_scan=False result exactly"""
    with flox_amd.set_options(**opts), _spy() as seen:
        got = flox_amd.groupby_scan(arr, lab, func=func, **kw)
    assert _kinds(seen) == ["1d"], _kinds(seen)
    with flox_amd.set_options(rows_scan=False):
        off = flox_amd.groupby_scan(arr, lab, func=func, **kw)
    got, off = _np(got), _np(off)
    assert got.dtype == off.dtype and got.shape == off.shape
    np.testing.assert_array_equal(got, off)


def test_fallback_datetime_values():
    rng = np.random.default_rng(32)
    v = rng.integers(0, 10**6, (5, 300)).astype("timedelta64[s]")
    lab = rng.integers(0, NG, 300)
    for func in ("cumsum", "ffill"):
        _fold_only(v, lab, func, dict(rows_scan_min_rows=1), expected_groups=np.arange(NG))


def test_fallback_integer_fill():
    rng = np.random.default_rng(33)
    arr = torch.as_tensor(rng.integers(-9, 9, (5, 300))).cuda()
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    for func in FILLS:
        _fold_only(arr, lab, func, dict(rows_scan_min_rows=1), expected_groups=np.arange(NG))


def test_fallback_option_off_and_few_rows():
    rng = np.random.default_rng(34)
    arr = torch.as_tensor(_whole_floats(rng, (5, 300))).cuda()
    lab = torch.as_tensor(rng.integers(0, NG, 300)).cuda()
    for func in OPS:
        _fold_only(arr, lab, func, dict(rows_scan=False, rows_scan_min_rows=1))
        _fold_only(arr, lab, func, dict(rows_scan_min_rows=6))  # lead_M = 5
        _fold_only(arr, lab, func, dict())  # the default gate is above 5 rows
        with flox_amd.set_options(rows_scan_min_rows=5), _spy() as seen:
            flox_amd.groupby_scan(arr, lab, func=func)
        assert _kinds(seen) == ["rows"]


def test_fallback_group_count_above_capacity():
    rng = np.random.default_rng(35)
    mg = _ffi.scan_rows_max_groups(_ffi.F32)
    n = mg + 40
    arr = torch.as_tensor(_whole_floats(rng, (5, n))).cuda()
    lab = torch.as_tensor(rng.integers(0, mg + 1, n)).cuda()
    _fold_only(arr, lab, "cumsum", dict(rows_scan_min_rows=1), expected_groups=np.arange(mg + 1))
    with flox_amd.set_options(rows_scan_min_rows=1), _spy() as seen:
        flox_amd.groupby_scan(arr, lab, func="cumsum", expected_groups=np.arange(mg))
    assert _kinds(seen) == ["rows"]


# ---- capture ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("func", ["cumsum", "ffill"])
def test_capture_launches_the_row_form(func):
    rng = np.random.default_rng(36)
    v = _whole_floats(rng, (12, 4101))
    v[rng.random(v.shape) < 0.05] = np.nan
    arr = torch.as_tensor(v).cuda()
    lab = torch.as_tensor(rng.integers(0, NG, 4101)).cuda()
    kw = dict(func=func, expected_groups=np.arange(NG))
    with flox_amd.set_options(rows_scan_min_rows=1):
        with _spy() as seen:
            eager = flox_amd.groupby_scan(arr, lab, **kw)
        assert _kinds(seen) == ["rows"]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g), _spy() as seen:
                res = flox_amd.groupby_scan(arr, lab, **kw)
        assert _kinds(seen) == ["rows"]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(res), _np(eager))


# ---- beyond 2^32 elements -------------------------------------------------------------------------------


def test_beyond_2_32_elements():
    m, n = 2**21 + 64, 2**11
    assert m * n > 2**32
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 48 * 2**30:
        pytest.skip("needs 48 GiB of free device memory")
    g0 = torch.Generator(device="cuda").manual_seed(5)
    arr = torch.empty((m, n), dtype=torch.float32, device="cuda")
    step = 2**18  # fill in row blocks: the int8 draw never holds more than 0.5 GiB
    for r in range(0, m, step):
        k = min(step, m - r)
        arr[r:r + k] = torch.randint(0, 7, (k, n), dtype=torch.int8, device="cuda", generator=g0)
    lab = torch.arange(n, device="cuda") % 3
    with _spy() as seen:  # the default gate: this many rows are far above any minimum
        got = flox_amd.groupby_scan(arr, lab, func="cumsum")
    assert seen == [("rows", arr.data_ptr(), n)]
    assert got.shape == (m, n) and got.dtype == torch.float32
    # every partial sum is a whole number below 2^24: exact in f32
    for r0 in (0, m // 2 - 2048, m - 4096):
        for g in range(3):
            want = torch.cumsum(arr[r0:r0 + 4096, g::3], 1)
            assert torch.equal(got[r0:r0 + 4096, g::3], want), (r0, g)
    del got, arr
    torch.cuda.empty_cache()
