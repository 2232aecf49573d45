"""groupby_reduce_many over leading dims: one SET_SUMMARY pass of the column
kernel. Every result against the oracle and the single-func call on the
shapes where the fused column form can go wrong, the raw partials against
numpy (direct and slab flush), no group cap, capture, the variance numerics
and the API corners that go through the unchanged finalize."""

import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from flox_amd import core as fa_core
from oracle import groupby_reduce as oracle_reduce
from tests.test_hip_parity import _tol
from tests.test_reduce_many_gpu import (ALL13, EXACT, FFI_DT, FIVE, _compare, _kw_for,
                                        _max_summary_groups, _np, _spy)

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "int32", "int64"]
COLS_TTILE = 2048  # rows per staged tile of k_reduce_cols


@contextlib.contextmanager
def _spy_cols():
    """records (op set, values data_ptr, row stride) of every
    grouped_partials_cols call core makes"""
    seen = []
    orig = fa_core.grouped_partials_cols

    def wrapper(op_set, values2d, *a, **kw):
        seen.append((op_set, values2d.data_ptr(), values2d.stride(0)))
        return orig(op_set, values2d, *a, **kw)

    fa_core.grouped_partials_cols = wrapper
    try:
        yield seen
    finally:
        fa_core.grouped_partials_cols = orig


def _sets(seen):
    return [s[0] for s in seen]


def _time_major(rng, n_t, m, dtype, ldm=None, nan=0.03):
    """(n_t, ldm) values, time-major"""
    ldm = m if ldm is None else ldm
    if np.dtype(dtype).kind == "f":
        v = (rng.standard_normal((n_t, ldm)) * 100).astype(dtype)
        if nan:
            v[rng.random((n_t, ldm)) < nan] = np.nan
    else:
        v = rng.integers(-1000, 1000, (n_t, ldm)).astype(dtype)
    return v


def _codes(rng, n_t, ng):
    """labels in [1, ng - 1): groups 0 and ng - 1 stay empty; some rows in no group"""
    lab = rng.integers(1, max(ng - 1, 2), n_t)
    lab[rng.random(n_t) < 0.05] = -1
    return lab


def _check_api(arr_t, arr_np, bys, funcs, summary=True, **kw):
    """groupby_reduce_many(arr_t, ...) func by func against the oracle (on
    arr_np) and the single-func call; summary=True: exactly one column pass,
    carrying SET_SUMMARY, serves the fused names."""
    vkind = arr_np.dtype.kind
    as_numpy = not isinstance(arr_t, torch.Tensor)
    bin_ = bys if as_numpy else tuple(torch.as_tensor(b).cuda() for b in bys)
    with _spy_cols() as seen:
        results, *groups = flox_amd.groupby_reduce_many(arr_t, *bin_, funcs=funcs, **kw)
    fused = [f for f in funcs if f in fa_core.FUSED_MANY_FUNCS]
    if summary:
        assert _sets(seen).count(_ffi.SET_SUMMARY) == 1, seen
        if len(fused) == len(funcs):
            assert len(seen) == 1, seen
    else:
        assert _ffi.SET_SUMMARY not in _sets(seen), seen
    assert list(results) == list(funcs)
    for f in funcs:
        kwf = _kw_for(kw, f)
        want, *wg = oracle_reduce(arr_np, *bys, func=f, **kwf)
        single, *sg = flox_amd.groupby_reduce(arr_t, *bin_, func=f, **kwf)
        _compare(results[f], single, want, f, vkind)
        assert len(groups) == len(sg) == len(wg)
        for a, b, c in zip(groups, sg, wg):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    return results, seen


def _np_members(v, codes, ng):
    """numpy reference of the seven SET_SUMMARY members, (ng, m)"""
    n_t, m = v.shape
    isf = v.dtype.kind == "f"
    out = {
        "sum": np.zeros((ng, m), np.float64 if isf else np.int64),
        "count": np.zeros((ng, m), np.int64),
        "present": np.zeros((ng, m), np.int32),
        "nanflag": np.zeros((ng, m), np.int32),
        "min": np.full((ng, m), np.inf if isf else np.iinfo(v.dtype).max, v.dtype),
        "max": np.full((ng, m), -np.inf if isf else -np.iinfo(v.dtype).max, v.dtype),
        "ssd": np.zeros((ng, m), np.float64),
    }
    for g in range(ng):
        rows = v[codes == g]
        for c in range(m):
            col = rows[:, c]
            ok = col[~np.isnan(col)] if isf else col
            out["count"][g, c] = len(ok)
            out["nanflag"][g, c] = int(len(ok) < len(col))
            out["present"][g, c] = int(len(col) > 0)
            if len(ok):
                out["sum"][g, c] = ok.sum(dtype=out["sum"].dtype)
                out["min"][g, c], out["max"][g, c] = ok.min(), ok.max()
                x = ok.astype(np.float64)
                out["ssd"][g, c] = ((x - x.mean()) ** 2).sum()
    return out


def _assert_members(got, want, isf):
    for k in ("count", "nanflag", "present", "min", "max"):
        np.testing.assert_array_equal(_np(got[k]), want[k], err_msg=k)
    if isf:
        np.testing.assert_allclose(_np(got["sum"]), want["sum"], rtol=1e-12, atol=1e-9)
    else:
        np.testing.assert_array_equal(_np(got["sum"]), want["sum"])
    np.testing.assert_allclose(_np(got["ssd"]), want["ssd"], rtol=1e-11, atol=1e-7)
    assert bool((got["ssd"] >= 0).all())


def _check_partials(vt, v_np, codes, ng):
    """aggregate_hip.grouped_partials_cols(SET_SUMMARY) on the (n_t, m) view
    vt against numpy, member by member"""
    sc, perm = torch.sort(torch.as_tensor(codes).cuda(), stable=True)
    got = aggregate_hip.grouped_partials_cols(
        _ffi.SET_SUMMARY, vt, sc.to(torch.int32), perm.to(torch.int32), ng, skipnan=True)
    assert got["_path"] == 3
    _assert_members(got, _np_members(v_np, codes, ng), v_np.dtype.kind == "f")


# ---- one pass ------------------------------------------------------------------

def _lead4():
    rng = np.random.default_rng(61)
    arr = _time_major(rng, 25_000, 4, "float32").T.copy()  # (4, 25_000)
    lab = rng.integers(0, 257, 25_000)
    return torch.as_tensor(arr).cuda(), torch.as_tensor(lab).cuda(), np.arange(257)


@pytest.mark.parametrize("funcs", [FIVE, ALL13], ids=["five", "all13"])
def test_one_column_pass_serves_the_call(funcs):
    arr, lab, expected = _lead4()
    with _spy_cols() as seen, _spy() as seen1d:
        flox_amd.groupby_reduce_many(arr, lab, funcs=funcs, expected_groups=expected)
    assert _sets(seen) == [_ffi.SET_SUMMARY]
    assert _ffi.SET_SUMMARY not in seen1d


def test_no_column_summary_when_it_does_not_apply():
    arr, lab, expected = _lead4()
    kw = dict(expected_groups=expected)
    with flox_amd.set_options(fused_many=False), _spy_cols() as seen:
        flox_amd.groupby_reduce_many(arr, lab, funcs=FIVE, **kw)
    assert _ffi.SET_SUMMARY not in _sets(seen) and len(seen) >= 5
    with _spy_cols() as seen:
        flox_amd.groupby_reduce_many(arr, lab, funcs=("mean",), **kw)
    assert _sets(seen) == [_ffi.SET_SUM_COUNT]
    with _spy_cols() as seen:
        flox_amd.groupby_reduce_many(arr, lab, funcs=("std", "median"), **kw)
    assert _ffi.SET_SUMMARY not in _sets(seen)


# ---- column shapes ---------------------------------------------------------------

N_T = 301
NG = 9


def _col_case(n_t, m, dtype, ldm=None, offset=0, seed=""):
    """time-major (n_t, ldm) tensor `offset` elements into its allocation, its
    first m columns as the (n_t, m) view the kernel reads, the (m, n_t)
    permute view the API takes, and the numpy twins"""
    rng = np.random.default_rng(zlib.crc32(f"cols-{n_t}-{m}-{dtype}-{ldm}-{offset}-{seed}".encode()))
    ldm = m if ldm is None else ldm
    v = _time_major(rng, n_t, m, dtype, ldm)
    flat = torch.empty(n_t * ldm + offset, dtype=getattr(torch, dtype), device="cuda")
    base = flat[offset:].view(n_t, ldm)
    base.copy_(torch.as_tensor(v))
    vt = base[:, :m]
    return vt, v[:, :m], _codes(rng, n_t, NG)


COL_SHAPES = [
    # m, ldm, offset
    (1, None, 0), (3, None, 0),          # VC = 1
    (8, None, 0),
    (2056, None, 0),                     # a second, partly empty column block
    (10, 16, 0),                         # partial lanes: full == false
    (12, None, 1),                       # base pointer off 16-B alignment
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,ldm,offset", COL_SHAPES)
def test_column_shapes(m, ldm, offset, dtype):
    vt, v_np, codes = _col_case(N_T, m, dtype, ldm, offset)
    if offset:
        assert vt.data_ptr() % 16 != 0
    _check_partials(vt, v_np, codes, NG)
    if m > 1:
        # the permute view of time-major data reaches the kernel without a copy
        funcs = ALL13 if m <= 12 else FIVE + ("nanvar", "sum")
        _, seen = _check_api(vt.permute(1, 0), v_np.T, (codes,), funcs,
                             expected_groups=np.arange(NG))
        assert seen[0][1:] == (vt.data_ptr(), vt.stride(0))


def test_ldm_not_a_multiple_of_eight_f32():
    vt, v_np, codes = _col_case(N_T, 12, "float32")
    _check_partials(vt, v_np, codes, NG)
    _check_api(vt.permute(1, 0), v_np.T, (codes,), ALL13, expected_groups=np.arange(NG))


def test_contiguous_lead_major_input_is_transposed_once():
    vt, v_np, codes = _col_case(N_T, 12, "float64")
    arr = vt.permute(1, 0).contiguous()  # (12, n_t) C-order: needs the copy
    _check_api(arr, v_np.T, (codes,), FIVE, expected_groups=np.arange(NG))


# ---- row shapes -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float32", "int64"])
@pytest.mark.parametrize("n_t", [1, 2, 3, 2047, 2048, 2049, 4101])
def test_row_counts(n_t, dtype):
    vt, v_np, codes = _col_case(n_t, 12, dtype)
    _check_partials(vt, v_np, codes, NG)
    _check_api(vt.permute(1, 0), v_np.T, (codes,), ALL13, expected_groups=np.arange(NG))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32"])
def test_group_straddles_a_tile_boundary(dtype):
    # group 1 holds 3000 rows: its chunk stages COLS_TTILE rows, then the rest
    vt, v_np, _ = _col_case(4101, 12, dtype)
    codes = np.full(4101, 2)
    codes[np.random.default_rng(5).permutation(4101)[:3000]] = 1
    assert (codes == 1).sum() > COLS_TTILE
    _check_partials(vt, v_np, codes, 4)
    _check_api(vt.permute(1, 0), v_np.T, (codes,), ALL13, expected_groups=np.arange(4))


@pytest.mark.parametrize("dtype", ["float64", "int32"])
def test_single_row_groups(dtype):
    vt, v_np, _ = _col_case(7, 12, dtype)
    codes = np.array([3, 0, 6, 1, 5, 2, 4])
    _check_partials(vt, v_np, codes, 7)
    _check_api(vt.permute(1, 0), v_np.T, (codes,), ALL13, expected_groups=np.arange(7))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nan_placement(dtype):
    n_t, m = 401, 12
    rng = np.random.default_rng(71)
    v = _time_major(rng, n_t, m, dtype, nan=0.0)
    codes = rng.integers(0, 5, n_t)
    codes[:3] = -1                       # out of range, sorted first
    v[codes == 1, 4] = np.nan            # group 1 all NaN in column 4 only
    first2 = np.flatnonzero(codes == 2)[0]
    v[first2, :] = np.nan                # NaN is the first value of group 2's segment
    first3 = np.flatnonzero(codes == 3)[:2]
    v[first3, 7] = np.nan
    vt = torch.as_tensor(v).cuda()
    # expected groups 5 and 6 receive no row; labels -1 fall in no group
    _check_partials(vt, v, codes, 7)
    res, _ = _check_api(vt.permute(1, 0), v.T, (codes,), ALL13, expected_groups=np.arange(7))
    assert np.isnan(_np(res["var"])[4, 1]) and np.isnan(_np(res["nanmax"])[4, 1])
    assert np.isfinite(_np(res["nanvar"])[:, 2]).all() and np.isnan(_np(res["var"])[:, 2]).all()
    assert (_np(res["count"])[:, 5:] == 0).all()


# ---- no group cap ------------------------------------------------------------------

def test_group_count_beyond_the_lds_summary():
    ng = _max_summary_groups("float64") + 1
    n_t, m = 6000, 8
    rng = np.random.default_rng(81)
    v = _time_major(rng, n_t, m, "float64")
    codes = rng.integers(0, ng, n_t)
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (codes,), FIVE + ("nanvar", "sum"),
               expected_groups=np.arange(ng))
    with _spy() as seen1d:  # the same count without leading dims still is not fused
        flox_amd.groupby_reduce_many(vt[:, 0].contiguous(), torch.as_tensor(codes).cuda(),
                                     funcs=FIVE, expected_groups=np.arange(ng))
    assert _ffi.SET_SUMMARY not in seen1d


# ---- slab mode: the raw ABI and capture -----------------------------------------------

TORCH_ACC = {"float32": torch.float64, "float64": torch.float64,
             "int32": torch.int64, "int64": torch.int64}


def _raw_cols_call(vt, sc, perm, ng, outs, scratch=None):
    c = _ffi.FhCall()
    c.op_set, c.vdtype, c.ldtype = _ffi.SET_SUMMARY, FFI_DT[str(vt.dtype)[6:]], _ffi.L_I32
    c.flags = _ffi.FLAG_SKIPNAN
    c.n, c.m, c.ldm, c.ngroups = vt.shape[0], vt.shape[1], vt.stride(0), ng
    c.values, c.labels, c.perm = vt.data_ptr(), sc.data_ptr(), perm.data_ptr()
    c.out_sum, c.out_count = outs["sum"].data_ptr(), outs["count"].data_ptr()
    c.out_present, c.out_nanflag = outs["present"].data_ptr(), outs["nanflag"].data_ptr()
    c.out_min, c.out_max = outs["min"].data_ptr(), outs["max"].data_ptr()
    c.out_ssd = outs["ssd"].data_ptr()
    if scratch is not None:
        c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel()
    c.stream = torch.cuda.current_stream().cuda_stream
    return c


def _slab_case(dtype, values=None, codes=None, ng=3):
    """4101 rows x 24 columns in 3 groups (or the caller's), chunk_offsets
    NULL: row chunks whose boundaries fall inside segments"""
    rng = np.random.default_rng(zlib.crc32(f"slab-{dtype}".encode()))
    v = _time_major(rng, 4101, 24, dtype) if values is None else values
    n_t, m = v.shape
    codes = rng.integers(-1, ng, n_t) if codes is None else codes
    vt = torch.as_tensor(v).cuda()
    sc, perm = torch.sort(torch.as_tensor(codes).cuda(), stable=True)
    outs = {
        "sum": torch.full((ng, m), -77, dtype=TORCH_ACC[dtype], device="cuda"),
        "count": torch.full((ng, m), -77, dtype=torch.int64, device="cuda"),
        "present": torch.full((ng, m), -77, dtype=torch.int32, device="cuda"),
        "nanflag": torch.full((ng, m), -77, dtype=torch.int32, device="cuda"),
        "min": torch.full((ng, m), -77, dtype=vt.dtype, device="cuda"),
        "max": torch.full((ng, m), -77, dtype=vt.dtype, device="cuda"),
        "ssd": torch.full((ng, m), -77, dtype=torch.float64, device="cuda"),
    }
    return v, codes, vt, sc.to(torch.int32), perm.to(torch.int32), ng, outs


def _run_slab(dtype, values=None, codes=None, ng=3):
    lib = _ffi.load_library()
    v, codes, vt, sc, perm, ng, outs = _slab_case(dtype, values, codes, ng)
    c = _raw_cols_call(vt, sc, perm, ng, outs)
    nscratch = lib.fh_scratch_bytes(ctypes.byref(c))
    assert nscratch > 0
    scratch = torch.empty(nscratch, dtype=torch.uint8, device="cuda")
    c = _raw_cols_call(vt, sc, perm, ng, outs, scratch)
    assert lib.fh_grouped_reduce_cols(ctypes.byref(c)) == 0
    torch.cuda.synchronize()
    assert c.path_used == 3
    return v, codes, ng, outs, c


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_abi_slab_mode_against_numpy(dtype):
    lib = _ffi.load_library()
    assert lib.fh_abi_revision() == 6
    v, codes, ng, outs, c = _run_slab(dtype)
    _assert_members(outs, _np_members(v, codes, ng), v.dtype.kind == "f")
    # no finish mode applies to the set
    c.finish, c.result_dtype, c.result = _ffi.FINISH_MEAN, _ffi.F64, outs["sum"].data_ptr()
    assert lib.fh_grouped_reduce_cols(ctypes.byref(c)) == 14
    c.finish = _ffi.FINISH_NONE
    c.out_ssd = None
    assert lib.fh_grouped_reduce_cols(ctypes.byref(c)) == 16
    c.out_ssd, c.out_nanflag = outs["ssd"].data_ptr(), None
    assert lib.fh_grouped_reduce_cols(ctypes.byref(c)) == 6
    assert b"LDS-binned path only" in lib.fh_error_string(15)


def test_capture_over_leading_dims_replays_the_eager_result():
    rng = np.random.default_rng(91)
    n_t, m, ng = 4101, 12, 3
    vt = torch.as_tensor(_time_major(rng, n_t, m, "float32")).cuda()
    arr = vt.permute(1, 0)
    lab = torch.as_tensor(rng.integers(0, ng, n_t)).cuda()
    expected = np.arange(ng)
    eager, _ = flox_amd.groupby_reduce_many(arr, lab, funcs=FIVE, expected_groups=expected)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g), _spy_cols() as seen:
            res, _ = flox_amd.groupby_reduce_many(arr, lab, funcs=FIVE, expected_groups=expected)
    assert _sets(seen) == [_ffi.SET_SUMMARY]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for f in FIVE:
            if f in EXACT:
                np.testing.assert_array_equal(_np(res[f]), _np(eager[f]), err_msg=f)
            else:
                np.testing.assert_allclose(_np(res[f]), _np(eager[f]), equal_nan=True,
                                           err_msg=f, **_tol(f, np.float32))


# ---- variance numerics ---------------------------------------------------------------

# max relative error over (group, column) of groupby_reduce(func="var") and
# (func="std") over leading dims, the single-pass FH_SET_WELFORD column form,
# against the oracle on the inputs of _var_case, measured on an MI355X
# (profiles/r07_cols_summary.md; five runs each, the largest kept). The fused
# column form is allowed VAR_SLACK times these, the margin
# tests/test_reduce_many_gpu.py gives a one-pass form over a reference form:
# 3.08e-13 / 1.54e-13, 0 / 0, 2.88e-13 / 1.44e-13. With group-aligned chunks
# (direct flush) it is the same arithmetic and measured the same figures. The
# slab flush is checked on the same inputs and against the same bounds through
# the raw ABI (chunk_offsets NULL), where the chunks' triples are merged: it
# measured 7.712e-14 / 3.854e-14 (f64), 0 / 0 (f32), 7.199e-14 / 3.587e-14 (i64).
WELFORD_ERR = {
    "float64": {"var": 7.690e-14, "std": 3.844e-14},
    "float32": {"var": 0.0, "std": 0.0},
    "int64": {"var": 7.199e-14, "std": 3.588e-14},
}
VAR_SLACK = 4.0
VAR_NT, VAR_M, VAR_NG = 20_003, 8, 7


def _var_case(vdtype):
    rng = np.random.default_rng(zlib.crc32(f"colvar-{vdtype}".encode()))
    shape = (VAR_NT, VAR_M)
    if vdtype == "float64":
        v = 1e8 + rng.standard_normal(shape)
    elif vdtype == "float32":
        v = (1e3 + rng.standard_normal(shape)).astype(np.float32)
    else:
        v = 10**6 + rng.integers(-10, 11, shape)
    return v, rng.integers(0, VAR_NG, VAR_NT)


def _relerr(got, want):
    got, want = _np(got).astype(np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _splits_rows(arr, n_t, m, ng):
    """whether a column call of this shape without chunk_offsets takes the slab"""
    c = _ffi.FhCall()
    c.op_set, c.vdtype = _ffi.SET_SUMMARY, FFI_DT[str(arr.dtype)[6:]]
    c.n, c.ngroups, c.m, c.ldm = n_t, ng, m, m
    c.values = c.out_ssd = arr.data_ptr()  # read for alignment / presence only
    return _ffi.load_library().fh_scratch_bytes(ctypes.byref(c)) > 0


@pytest.mark.parametrize("vdtype", ["float64", "float32", "int64"])
def test_variance_numerics_direct(vdtype):
    v, lab = _var_case(vdtype)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(expected_groups=np.arange(VAR_NG))
    with _spy_cols() as seen:
        res, _ = flox_amd.groupby_reduce_many(arr, lt, funcs=("var", "nanvar", "std", "mean"), **kw)
    assert _sets(seen) == [_ffi.SET_SUMMARY]
    for f in ("var", "nanvar", "std"):
        bound = VAR_SLACK * WELFORD_ERR[vdtype]["std" if f == "std" else "var"]
        want, _ = oracle_reduce(v.T, lab, func=f, **kw)
        single, _ = flox_amd.groupby_reduce(arr, lt, func=f, **kw)
        got = _np(res[f])
        print(f"direct {vdtype} {f}: welford err {_relerr(single, want):.3e} "
              f"fused err {_relerr(got, want):.3e} bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and np.all(got >= 0), (f, got)
        assert _relerr(got, want) <= bound, (f, _relerr(got, want), bound)


@pytest.mark.parametrize("vdtype", ["float64", "float32", "int64"])
def test_variance_numerics_slab(vdtype):
    # the inputs of the direct test with the row range split without group
    # alignment: ten chunks per (group, column), merged by k_combine
    v, lab = _var_case(vdtype)
    _, _, ng, outs, _ = _run_slab(vdtype, v, lab, VAR_NG)
    kw = dict(expected_groups=np.arange(ng))
    var = (outs["ssd"] / outs["count"]).t()
    for f, got in (("var", _np(var)), ("std", _np(torch.sqrt(var)))):
        bound = VAR_SLACK * WELFORD_ERR[vdtype][f]
        want, _ = oracle_reduce(v.T, lab, func=f, **kw)
        got = got.astype(want.dtype)  # the finalize's cast: f32 in, f32 out
        print(f"slab {vdtype} {f}: fused err {_relerr(got, want):.3e} bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and np.all(got >= 0), (f, got)
        assert _relerr(got, want) <= bound, (f, _relerr(got, want), bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_group_splits_rows_eagerly(dtype):
    # one group leaves nothing to align chunks to: the eager call takes the slab
    vt, v_np, _ = _col_case(4101, 12, dtype)
    codes = np.zeros(4101, dtype=np.int64)
    assert _splits_rows(vt, 4101, 12, 1)
    _check_partials(vt, v_np, codes, 1)
    _check_api(vt.permute(1, 0), v_np.T, (codes,), ALL13, expected_groups=np.arange(1))


@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
def test_no_negative_variance_on_constant_groups(slab):
    n_t, m, ng = 6001, 8, 1 if slab else 5
    rng = np.random.default_rng(31)
    lab = rng.integers(0, ng, n_t)
    v = (1e8 + lab[:, None] * 0.1 + np.arange(m)[None, :] * 0.3).astype(np.float64)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    assert _splits_rows(arr, n_t, m, ng) or not slab
    res, _ = flox_amd.groupby_reduce_many(arr, lt, funcs=("var", "std"),
                                          expected_groups=np.arange(ng))
    assert np.array_equal(_np(res["var"]), np.zeros((m, ng)))
    assert np.array_equal(_np(res["std"]), np.zeros((m, ng)))


# ---- API corners (the unchanged finalize) ---------------------------------------------

def _sparse_cols(dtype="float64", n_t=803, m=6, ng=9):
    """group 0 empty, group 1 all NaN (floats), group 2 with two rows"""
    rng = np.random.default_rng(41)
    lab = rng.integers(3, ng, n_t)
    lab[:2] = 2
    lab[2:6] = 1
    v = _time_major(rng, n_t, m, dtype)
    if np.dtype(dtype).kind == "f":
        v[:2] = 1.5
        v[2:6] = np.nan
    return v, lab, ng


@pytest.mark.parametrize("dtype", ["float64", "int32"])
@pytest.mark.parametrize("kw", [
    dict(fill_value=-7.0),
    dict(min_count=3, fill_value=-9.0),
    dict(min_count={"sum": 3, "nanmin": 5}, fill_value={"mean": 0.5, "sum": 1.0, "nanmin": 2.0,
                                                        "count": 3, "var": 5.0, "min": 6.0}),
])
def test_fill_value_and_min_count(dtype, kw):
    v, lab, ng = _sparse_cols(dtype)
    _check_api(torch.as_tensor(v).cuda().permute(1, 0), v.T, (lab,),
               ("mean", "sum", "nanmin", "count", "var", "min"), expected_groups=np.arange(ng), **kw)


def test_sort_false_keeps_first_appearance_order():
    rng = np.random.default_rng(13)
    n_t, m = 1007, 5
    by = rng.choice([30, 5, 17, 2, 44, 9], n_t)
    v = _time_major(rng, n_t, m, "float32")
    _check_api(torch.as_tensor(v).cuda().permute(1, 0), v.T, (by,), FIVE + ("nanmax",), sort=False)


def test_axis_subset_with_leading_dims():
    rng = np.random.default_rng(14)
    v = (rng.standard_normal((3, 4, 50)) * 10).astype(np.float64)
    v[rng.random(v.shape) < 0.05] = np.nan
    by = rng.integers(0, 4, (4, 50))
    res, _ = _check_api(torch.as_tensor(v).cuda(), v, (by,), FIVE + ("nansum",), axis=(2,),
                        expected_groups=np.arange(4), fill_value=-9.0)
    assert _np(res["mean"]).shape == (3, 4, 4)


def test_two_by():
    rng = np.random.default_rng(15)
    n_t, m = 2003, 6
    b0, b1 = rng.integers(-1, 5, n_t), rng.integers(-1, 8, n_t)
    v = _time_major(rng, n_t, m, "float32")
    res, _ = _check_api(torch.as_tensor(v).cuda().permute(1, 0), v.T, (b0, b1), FIVE + ("nansum",),
                        expected_groups=(np.arange(4), np.arange(7)))
    assert _np(res["mean"]).shape == (m, 4, 7)


def test_numpy_in_numpy_out():
    v, lab, ng = _sparse_cols("float32")
    res, _ = _check_api(np.ascontiguousarray(v.T), v.T, (lab,), FIVE, expected_groups=np.arange(ng))
    assert all(isinstance(r, np.ndarray) for r in res.values())


def test_mixed_funcs_equal_their_singles():
    v, lab, ng = _sparse_cols("float64")
    funcs = ("mean", "max", "median", "argmax")
    _, seen = _check_api(torch.as_tensor(v).cuda().permute(1, 0), v.T, (lab,), funcs,
                         expected_groups=np.arange(ng))
    # mean and max shared the summary pass; median and argmax took their own paths
    assert _sets(seen).count(_ffi.SET_SUMMARY) == 1
    assert _ffi.SET_SUM_COUNT not in _sets(seen) and _ffi.SET_MAX_FULL not in _sets(seen)
