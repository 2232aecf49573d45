"""quantile / median over leading dims with groups longer than the sort-in-LDS
capacity, on the radix-select column kernel (fh_grouped_quantile_select_cols):
the raw entry against numpy, digit hazards, more q than one batch of slots,
the ABI corners, the four API functions against the oracle and against the
lead fold (set_options(cols_select_funcs=False)) bit for bit, dispatch, what
keeps today's paths, groupby_reduce_many, and the 2**31-element array the fold
refuses.

The raw reference and its tolerance are those of tests/test_cols_sorted_gpu.py
(its docstring): np.quantile / np.nanquantile of the float64 view, the
documented rule where numpy's interpolation pair is infinite, 2**-50 relative
plus 2**-50 of the largest finite magnitude for a possible fused multiply-add.

Capture: the quantile names copy q from host memory on either path and cannot
be captured at all, so the capture case runs the names that can be captured
(mode / nanmode) with a long group: they keep the fold and the replay equals
the eager result. The select path's own capture condition is the one
_cols_sorted_ok already applies before it looks at the group lengths.
"""

import contextlib
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from flox_amd import core as fa_core
from oracle import groupby_reduce as oracle_reduce
from tests.test_cols_order_gpu import DTYPES, NG, _device_case, _same_bits, _tied_values
from tests.test_cols_sorted_gpu import (CAP, Q4, _api_values, _kinds, _np_sorted, _q_tol,
                                        _scale, _sorted_codes, _spy_sorted)
from tests.test_reduce_many_cols_gpu import _spy_cols
from tests.test_reduce_many_gpu import FFI_DT, _np, _spy

pytestmark = pytest.mark.gpu


def _define(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                        "floxhip_selcols.h")
    with open(path) as f:
        return int(next(ln for ln in f if ln.startswith(f"#define {name} ")).split()[2])


TILE = _define("FH_SELCOLS_MAX_COLS")    # columns of the one-slot plan's tile
SLOTS = _define("FH_SELCOLS_MAX_SLOTS")  # q served by one launch
FOUR = ("quantile", "nanquantile", "median", "nanmedian")


def _lib():
    lib = _ffi.load_library()
    assert _ffi.has_select_cols(), "library lacks the radix-select column entry"
    return lib


# ---- the raw entry ----------------------------------------------------------------------

def _raw(vt, sc, perm, ng, q, skipnan, want_count=True, drop=None, **override):
    """fh_grouped_quantile_select_cols through the raw ABI. Outputs are
    pre-filled with -77. `drop` names a buffer left NULL, `override` sets call
    fields (or nq) after everything else. Returns (rc, out, count)."""
    lib = _lib()
    n_t, m = vt.shape
    nq = len(q)
    out = torch.full((nq, ng, m), -77.0, dtype=torch.float64, device="cuda")
    count = torch.full((ng, m), -77, dtype=torch.int64, device="cuda")
    q_t = torch.tensor(q, dtype=torch.float64, device="cuda")
    c = _ffi.FhCall()
    c.vdtype, c.ldtype = FFI_DT[str(vt.dtype)[6:]], _ffi.L_I32
    c.flags = _ffi.FLAG_SKIPNAN if skipnan else 0
    c.n, c.m, c.ldm, c.ngroups = n_t, m, vt.stride(0), ng
    c.values, c.labels, c.perm = vt.data_ptr(), sc.data_ptr(), perm.data_ptr()
    c.out_sum = out.data_ptr()
    c.means = q_t.data_ptr()
    if want_count:
        c.out_count = count.data_ptr()
    if drop is not None:
        setattr(c, drop, None)
    nq = override.pop("nq", nq)
    for k, val in override.items():
        setattr(c, k, val)
    c.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.fh_grouped_quantile_select_cols(ctypes.byref(c), nq)
    torch.cuda.synchronize()
    if rc == 0:
        assert c.path_used == 3
    return rc, out, count


def _check_raw(vt, v_np, codes, ng, qs=(Q4,)):
    sc, perm = _sorted_codes(codes)
    tol = dict(rtol=2.0**-50, atol=2.0**-50 * _scale(v_np), equal_nan=True)
    outs = {}
    for skipnan in (False, True):
        for q in qs:
            wq, _, wcount = _np_sorted(v_np, codes, ng, q, skipnan)
            rc, got, cnt = _raw(vt, sc, perm, ng, q, skipnan)
            assert rc == 0
            with np.errstate(invalid="ignore"):
                np.testing.assert_allclose(_np(got), wq, err_msg=f"q={q} skipnan={skipnan}", **tol)
            np.testing.assert_array_equal(_np(cnt), wcount)
            outs[(skipnan, tuple(q))] = got
    return outs


def _wide_values(rng, n_t, m, dtype):
    """every other column from the tied pool (+-inf, +-0.0, extremes, NaN), the
    rest spread over the dtype so that every digit of the key matters"""
    v = _tied_values(rng, n_t, m, dtype)
    d = np.dtype(dtype)
    if d.kind == "f":
        w = (rng.standard_normal((n_t, m)) * 10.0 ** rng.integers(-3, 4, (n_t, m))).astype(d)
        w[rng.random((n_t, m)) < 0.05] = np.nan
    else:
        ii = np.iinfo(d)
        w = rng.integers(ii.min, ii.max, (n_t, m), dtype=d, endpoint=True)
    v[:, ::2] = w[:, ::2]
    return v


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_against_numpy(dtype):
    # groups: 0 = 2049 rows (one over the LDS capacity), 1 = 2303 rows (no
    # multiple of the row stride of 8, 16 or 32), 2 = one row, 3 = empty,
    # 4 = 41 rows that are all NaN for floats; 47 rows in no group
    sizes = {0: CAP + 1, 1: 2303, 2: 1, 4: 41, -1: 47}
    rng = np.random.default_rng(zlib.crc32(f"select-raw-{dtype}".encode()))
    codes = rng.permutation(np.concatenate([np.full(s, g) for g, s in sizes.items()]))
    n_t, m, ng = len(codes), TILE + 3, 5
    v = _wide_values(rng, n_t, m + 2, dtype)
    if v.dtype.kind == "f":
        v[codes == 4, :] = np.nan     # an all-NaN group
        v[codes == 0, 5] = np.nan     # an all-NaN column of a long group
        v[np.flatnonzero(codes == 1)[:3], 6] = np.nan  # exactly three NaN
        v[np.flatnonzero(codes == 1)[7], 8] = -0.0
    # ldm > m, the base one element off its allocation
    vt = _device_case(v, m, 1)
    assert vt.stride(0) == m + 2
    _check_raw(vt, v[:, :m], codes, ng, qs=(Q4, [0.5]))


def _bits(dtype, pattern):
    d = np.dtype(dtype)
    u = np.asarray(pattern, dtype=np.uint64).astype(f"u{d.itemsize}")
    return u.view(d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_digit_hazards(dtype):
    d = np.dtype(dtype)
    bits = d.itemsize * 8
    n = 300
    k = np.arange(n, dtype=np.uint64)
    base = 0x40490F0000000000 >> (64 - bits)  # a finite positive float / a positive int
    cols = [
        # keys that differ only in the lowest byte
        _bits(d, base + (k * 7) % 256),
        # keys that differ only in the highest byte (finite as floats: the
        # exponent's lower bits are clear)
        _bits(d, (((k * 11) % 256) << np.uint64(bits - 8)) | np.uint64(0x0012345678ABCD >> (64 - bits))),
        # an all-equal segment
        np.full(n, 3, d),
        # two distinct values in different bins of the first digit, split in
        # halves: q = 0.5 has vi = 149.5, floor in one half, ceil in the other
        np.where(k < n // 2, -7, 9).astype(d),
        # the same with a key in between that occurs once
        np.where(k < n // 2, -7, np.where(k == n // 2, 2, 9)).astype(d),
    ]
    if d.kind == "i":
        ii = np.iinfo(d)
        cols.append(np.where(k % 2 == 0, ii.min, ii.max).astype(d))     # min and max
        cols.append(np.where(k % 3 == 0, ii.min, np.where(k % 3 == 1, ii.max, -1)).astype(d))
    else:
        rng = np.random.default_rng(5)
        cols.append((-np.abs(rng.standard_normal(n)) - 0.5).astype(d))  # all negative
        cols.append((rng.standard_normal(n) * 3).astype(d))             # mixed sign
        cols.append(np.where(k % 2 == 0, -0.0, 0.0).astype(d))          # zeros of both signs
        cols.append(np.where(k < 100, -np.inf, np.where(k < 200, 1.0, np.inf)).astype(d))
    v = np.stack(cols, axis=1)
    assert np.isfinite(v[:, :5].astype(np.float64)).all()
    perm = np.random.default_rng(6).permutation(n)
    v = np.ascontiguousarray(v[perm])
    codes = np.zeros(n, dtype=np.int64)
    vt = torch.as_tensor(v).cuda()
    # dyadic q: vi = q * 299 and vi - floor(vi) are exact, fused or not. (The
    # reference's tolerance covers a fused `a + diff * t`, not a fused
    # `q * (actual - 1) - floor(vi)`, which the shared rule may also form and
    # which shows once `diff` spans the float range, as in column 1.)
    outs = _check_raw(vt, v, codes, 1, qs=(Q4, [0.5], [0.375, 0.875]))
    med = _np(outs[(True, (0.5,))])[0, 0]
    # positions 149 and 150: (-7, 9) and, with the single 2 between, (-7, 2)
    assert med[2] == 3.0 and med[3] == 1.0 and med[4] == -2.5
    if d.kind == "i":
        # (min + max) / 2; int64's max rounds to 2**63 as a double
        assert med[5] == (-0.5 if d.itemsize == 4 else 0.0)
    else:
        assert med[7] == 0.0


@pytest.mark.parametrize("dtype", ["float32", "int64"])
def test_more_q_than_one_batch_of_slots(dtype):
    rng = np.random.default_rng(8)
    n_t, m, ng = 700, TILE + 3, 3
    v = _wide_values(rng, n_t, m, dtype)
    codes = rng.integers(-1, ng, n_t)
    vt = torch.as_tensor(v).cuda()
    nq = SLOTS * 2 + 1
    q = [0.9, 0.1, 0.5, 0.5, 1.0, 0.0, 0.333, 0.9, 0.75, 0.25, 0.6, 0.01][:nq]
    q += [0.42] * (nq - len(q))
    assert len(q) == nq and len(set(q)) < nq and q != sorted(q)
    outs = _check_raw(vt, v, codes, ng, qs=(q,))
    sc, perm = _sorted_codes(codes)
    for skipnan in (False, True):
        for i, qq in enumerate(q):
            rc, one, _ = _raw(vt, sc, perm, ng, [qq], skipnan)
            assert rc == 0
            _same_bits(outs[(skipnan, tuple(q))][i], one[0], f"q[{i}]={qq} alone")


# ---- ABI ------------------------------------------------------------------------------------

def test_abi_corners():
    lib = _lib()
    assert lib.fh_abi_revision() == 6
    rng = np.random.default_rng(9)
    v = _wide_values(rng, 301, 4, "float64")
    codes = rng.integers(-1, NG, 301)
    vt = torch.as_tensor(v).cuda()
    sc, perm = _sorted_codes(codes)

    def untouched(rc, out, cnt, code):
        assert rc == code
        assert bool((out == -77).all()) and bool((cnt == -77).all())

    for drop in ("values", "labels", "perm", "out_sum", "means"):
        untouched(*_raw(vt, sc, perm, NG, [0.5], False, drop=drop), 22)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, nq=0), 22)    # mode is not served
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, nq=-1), 22)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, n=2**31), 22)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, n=-1), 22)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, vdtype=99), 9)
    # nothing to do: validated, no launch
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, ngroups=0), 0)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, m=0), 0)
    # the counts are optional
    rc, out, cnt = _raw(vt, sc, perm, NG, [0.5], True, want_count=False)
    assert rc == 0 and bool((cnt == -77).all()) and not bool((out == -77).any())
    # the wrapper names the entry in its message for code 22
    with pytest.raises(RuntimeError, match="floxhip error 22: fh_grouped_quantile_select_cols"):
        _ffi.check(22, _ffi._SELECT_COLS_ERRORS)


# ---- API parity ---------------------------------------------------------------------------------

@contextlib.contextmanager
def _spy_select():
    """_spy_sorted plus the select entry: ("select", values data_ptr, row stride)"""
    orig = aggregate_hip.grouped_quantile_select_cols
    with _spy_sorted() as seen:
        def w(values, *a, **kw):
            seen.append(("select", values.data_ptr(), values.stride(0)))
            return orig(values, *a, **kw)

        aggregate_hip.grouped_quantile_select_cols = w
        try:
            yield seen
        finally:
            aggregate_hip.grouped_quantile_select_cols = orig


def _long_labels(rng, n_t, long, ng=NG):
    """group 1 has `long` rows, the rest spread over groups 2..ng-2 and a few
    in no group; groups 0 and ng - 1 stay empty"""
    lab = rng.integers(2, ng - 1, n_t)
    lab[rng.random(n_t) < 0.05] = -1
    lab[rng.permutation(n_t)[:long]] = 1
    assert (lab == 1).sum() == long and np.bincount(lab[lab >= 0]).max() == long
    return lab


def _api_case(dtype, n_t=CAP + 500, m=7, long=CAP + 1):
    rng = np.random.default_rng(zlib.crc32(f"select-api-{dtype}-{n_t}-{m}-{long}".encode()))
    v = _api_values(rng, n_t, m, dtype)
    lab = _long_labels(rng, n_t, long)
    if v.dtype.kind == "f":
        v[lab == 3, 0] = np.nan  # an all-NaN (group, column)
    return v, lab


def _check_api(arr, arr_np, bys, func, vt=None, oracle=True, tol_dtype=None, **kw):
    """groupby_reduce on the select entry against the same call through the
    lead fold (bit for bit) and against the oracle"""
    as_numpy = not isinstance(arr, torch.Tensor)
    bin_ = bys if as_numpy else tuple(torch.as_tensor(b).cuda() for b in bys)
    if "quantile" in func and "finalize_kwargs" not in kw:
        kw["finalize_kwargs"] = {"q": Q4}
    with flox_amd.set_options(cols_select_min_cols=1), _spy_select() as seen:
        got, *groups = flox_amd.groupby_reduce(arr, *bin_, func=func, **kw)
    assert _kinds(seen) == ["select"], (func, seen)  # no fold, no 1-D sort
    if vt is not None:
        assert seen[0][1:] == (vt.data_ptr(), vt.stride(0))  # zero copy
    with flox_amd.set_options(cols_select_min_cols=1, cols_select_funcs=False), \
            _spy_select() as seen_off:
        off, *goff = flox_amd.groupby_reduce(arr, *bin_, func=func, **kw)
    assert _kinds(seen_off) == ["fold", "1d"], (func, seen_off)
    assert type(got) is type(off)
    _same_bits(got, off, f"{func} vs the fold")
    for a, b in zip(groups, goff):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    if not oracle:
        return got
    want, *wg = oracle_reduce(arr_np, *bys, func=func, **kw)
    g = _np(got)
    assert g.shape == want.shape and g.dtype == want.dtype, (func, g.shape, want.shape, g.dtype, want.dtype)
    np.testing.assert_allclose(g, want, equal_nan=True, err_msg=f"{func} vs oracle",
                               **_q_tol(tol_dtype or arr_np.dtype))
    for a, c in zip(groups, wg):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("func", FOUR)
def test_api_parity(func, dtype):
    v, lab = _api_case(dtype)
    vt = torch.as_tensor(v).cuda()
    got = _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, expected_groups=np.arange(NG))
    assert isinstance(got, torch.Tensor)
    assert got.shape == ((4, 7, NG) if "quantile" in func else (7, NG))


@pytest.mark.parametrize("func", ("quantile", "nanquantile"))
def test_api_scalar_and_vector_q(func):
    v, lab = _api_case("float64")
    vt = torch.as_tensor(v).cuda()
    kw = dict(expected_groups=np.arange(NG))
    s = _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, finalize_kwargs={"q": 0.3}, **kw)
    assert s.shape == (7, NG)
    one = _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, finalize_kwargs={"q": [0.3]}, **kw)
    assert one.shape == (1, 7, NG)
    _same_bits(one[0], s, "q=[0.3] vs q=0.3")


@pytest.mark.parametrize("dtype", ["float64", "int32"])
@pytest.mark.parametrize("func", ("median", "nanquantile"))
@pytest.mark.parametrize("kw", [
    dict(min_count=3, fill_value=-9),
    dict(min_count=1, fill_value=-5),  # all-NaN groups count 0 and fill
], ids=["min_count3", "min_count1"])
def test_api_min_count_takes_the_kernel_s_counts(kw, func, dtype):
    v, lab = _api_case(dtype)
    lab[np.flatnonzero(lab == 7)] = 6
    lab[np.flatnonzero(lab != 1)[:2]] = 7  # a group of two rows: below min_count=3
    vt = torch.as_tensor(v).cuda()
    with _spy() as seen1d, _spy_cols() as seen_cols:
        _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, oracle=False,
                   expected_groups=np.arange(NG), **kw)
    # the select call made no SET_COUNT pass; the fold's one 1-D count pass is
    # the only other kernel pass the two calls made
    assert seen_cols == [] and seen1d == [_ffi.SET_COUNT]
    _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, expected_groups=np.arange(NG), **kw)


def test_api_sort_false():
    rng = np.random.default_rng(13)
    n_t, m = CAP + 400, 5
    by = rng.choice([30, 5, 17, 2, 44, 9], n_t)
    by[rng.permutation(n_t)[:CAP + 1]] = 17
    v = _api_values(rng, n_t, m, "float32")
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (by,), "nanmedian", vt=vt, sort=False)


def test_api_two_by():
    rng = np.random.default_rng(15)
    n_t, m = CAP + 900, 6
    b0, b1 = rng.integers(-1, 5, n_t), rng.integers(-1, 8, n_t)
    rows = rng.permutation(n_t)[:CAP + 1]
    b0[rows], b1[rows] = 2, 3
    v = _api_values(rng, n_t, m, "float64")
    vt = torch.as_tensor(v).cuda()
    got = _check_api(vt.permute(1, 0), v.T, (b0, b1), "nanquantile", vt=vt,
                     expected_groups=(np.arange(4), np.arange(7)))
    assert got.shape == (4, m, 4, 7)


def test_api_three_leading_dims():
    rng = np.random.default_rng(18)
    n_t = CAP + 300
    v = _api_values(rng, 3 * 4, n_t, "float32").reshape(3, 4, n_t)
    lab = _long_labels(rng, n_t, CAP + 1, ng=5)
    for func in ("nanmedian", "quantile"):
        got = _check_api(torch.as_tensor(v).cuda(), v, (lab,), func, expected_groups=np.arange(5))
        assert got.shape == ((4, 3, 4, 5) if func == "quantile" else (3, 4, 5))


@pytest.mark.parametrize("dtype", ["uint8", "int16"])
def test_api_numpy_input_of_a_small_dtype(dtype):
    rng = np.random.default_rng(16)
    n_t, m = CAP + 300, 5
    v = rng.integers(0, 5, (m, n_t)).astype(dtype)
    lab = _long_labels(rng, n_t, CAP + 1)
    got = _check_api(v, v, (lab,), "median", expected_groups=np.arange(NG), tol_dtype="int64")
    assert isinstance(got, np.ndarray)


@pytest.mark.parametrize("func", ("nanmedian", "quantile"))
def test_the_boundary_is_the_lds_capacity(func):
    kw = dict(func=func, expected_groups=np.arange(NG))
    if func == "quantile":
        kw["finalize_kwargs"] = {"q": Q4}
    for long, kind in ((CAP, "cols"), (CAP + 1, "select")):
        v, lab = _api_case("float32", long=long)
        arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
        with flox_amd.set_options(cols_select_min_cols=1), _spy_select() as seen:
            on, _ = flox_amd.groupby_reduce(arr, lt, **kw)
        assert _kinds(seen) == [kind]
        with flox_amd.set_options(cols_sorted_funcs=False):
            off, _ = flox_amd.groupby_reduce(arr, lt, **kw)
        _same_bits(on, off, f"{func} at {long} rows")


# ---- what keeps today's paths ------------------------------------------------------------------------

def _both_ways(arr, by, off=None, **kw):
    """the call with the gate open, and with `off` (default: the select switch off)"""
    with flox_amd.set_options(cols_select_min_cols=1), _spy_select() as seen:
        on = flox_amd.groupby_reduce(arr, by, **kw)
    with flox_amd.set_options(**(off or dict(cols_select_funcs=False))), _spy_select() as seen_off:
        other = flox_amd.groupby_reduce(arr, by, **kw)
    return on, other, _kinds(seen), _kinds(seen_off)


@pytest.mark.parametrize("func", ("mode", "nanmode"))
def test_mode_with_a_long_group_keeps_the_fold(func):
    v, lab = _api_case("float32")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    on, other, kinds, kinds_off = _both_ways(arr, lt, off=dict(cols_sorted_funcs=False),
                                             func=func, expected_groups=np.arange(NG))
    assert kinds == kinds_off == ["fold", "1d"]
    _same_bits(on[0], other[0], func)


def test_datetime_values_keep_the_fold():
    rng = np.random.default_rng(19)
    n_t = CAP + 200
    v = rng.integers(0, 5, (4, n_t)).astype("datetime64[ns]")
    lab = _long_labels(rng, n_t, CAP + 1)
    on, other, kinds, kinds_off = _both_ways(v, lab, func="median", expected_groups=np.arange(NG))
    assert kinds == kinds_off == ["fold", "1d"]
    _same_bits(on[0], other[0], "median")


def test_axis_subset_keeps_the_fold():
    rng = np.random.default_rng(20)
    n_t = CAP + 200
    v = _api_values(rng, 6, n_t, "float64").reshape(3, 2, n_t)
    by = np.stack([_long_labels(rng, n_t, CAP + 1, ng=5) for _ in range(2)])
    kw = dict(func="nanmedian", axis=(2,), expected_groups=np.arange(5), fill_value=-9.0)
    on, other, kinds, kinds_off = _both_ways(
        torch.as_tensor(v).cuda(), torch.as_tensor(by).cuda(), **kw)
    assert kinds == kinds_off == ["fold", "1d"]
    assert on[0].shape == (3, 2, 5)
    _same_bits(on[0], other[0], "nanmedian")


@pytest.mark.parametrize("func", ("mode", "nanmode"))
def test_capture_keeps_the_fold_and_replays_the_eager_result(func):
    # see the module docstring: the names a stream can capture at all
    v, lab = _api_case("float32", n_t=CAP + 300, m=12)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(func=func, expected_groups=np.arange(NG))
    with flox_amd.set_options(cols_select_min_cols=1):
        eager, _ = flox_amd.groupby_reduce(arr, lt, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g), _spy_select() as seen:
                res, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    assert _kinds(seen) == ["fold", "1d"]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _same_bits(res, eager, func)


def test_a_narrow_array_keeps_the_fold_at_the_shipped_gate():
    assert fa_core.COLS_SELECT_MIN_COLS >= TILE
    v, lab = _api_case("float32", m=3)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(func="nanmedian", expected_groups=np.arange(NG))
    with _spy_select() as seen:
        narrow, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    assert _kinds(seen) == ["fold", "1d"]
    with flox_amd.set_options(cols_select_min_cols=1), _spy_select() as seen:
        sel, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    assert _kinds(seen) == ["select"]
    _same_bits(narrow, sel, "nanmedian on 3 columns")
    # at the gate itself the shipped default selects
    v, lab = _api_case("float32", n_t=CAP + 100, m=fa_core.COLS_SELECT_MIN_COLS)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    with _spy_select() as seen:
        wide, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    assert _kinds(seen) == ["select"]
    with flox_amd.set_options(cols_select_funcs=False):
        off, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    _same_bits(wide, off, "nanmedian at the gate")


def test_the_sorted_switch_turns_the_select_path_off_too():
    v, lab = _api_case("float64")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    on, other, kinds, kinds_off = _both_ways(
        arr, lt, off=dict(cols_sorted_funcs=False, cols_select_funcs=True, cols_select_min_cols=1),
        func="median", expected_groups=np.arange(NG))
    assert kinds == ["select"] and kinds_off == ["fold", "1d"]
    _same_bits(on[0], other[0], "median")


def test_many_mean_median():
    v, lab = _api_case("float64")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(expected_groups=np.arange(NG))
    funcs = ("mean", "median")
    with flox_amd.set_options(cols_select_min_cols=1):
        with _spy_select() as seen:
            res, _ = flox_amd.groupby_reduce_many(arr, lt, funcs=funcs, **kw)
        assert _kinds(seen) == ["select"]
        for f in funcs:
            single, _ = flox_amd.groupby_reduce(arr, lt, func=f, **kw)
            _same_bits(res[f], single, f)


# ---- the size limit -------------------------------------------------------------------------------------

def test_two_to_the_31_elements():
    n_t, m, ng = 2**12, 2**19, 2
    torch.cuda.empty_cache()  # blocks cached by earlier tests are not "free"
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2**30:
        pytest.skip("needs 24 GiB of free device memory")
    gen = torch.Generator(device="cuda").manual_seed(3)
    vt = torch.empty((n_t, m), dtype=torch.float32, device="cuda")
    # few distinct values: ties in every column; one of them becomes NaN
    vt.copy_(torch.randint(0, 7, (n_t, m), generator=gen, device="cuda", dtype=torch.int8))
    vt.masked_fill_(vt == 6, float("nan"))
    assert vt.numel() == 2**31
    # 7 is coprime to 2**12: exactly 2500 rows in group 0, 1596 in group 1
    lab = ((torch.arange(n_t, device="cuda") * 7) % n_t >= 2500).to(torch.int64)
    assert int((lab == 0).sum()) == 2500 > CAP
    arr = vt.permute(1, 0)
    kw = dict(func="nanmedian", expected_groups=np.arange(ng))
    with _spy_select() as seen:
        med, _ = flox_amd.groupby_reduce(arr, lab, **kw)
    assert seen == [("select", vt.data_ptr(), vt.stride(0))]
    assert med.shape == (m, ng) and med.dtype == torch.float32
    with flox_amd.set_options(cols_select_funcs=False):
        with pytest.raises(NotImplementedError, match="with leading dims at this size"):
            flox_amd.groupby_reduce(arr, lab, **kw)
    cols = torch.as_tensor(np.random.default_rng(4).choice(m, 4096, replace=False)).cuda()
    sample = vt[:, cols].cpu().numpy().astype(np.float64)
    got = med[cols].cpu().numpy()
    lab_np = lab.cpu().numpy()
    for g in range(ng):
        want = np.nanquantile(sample[lab_np == g], 0.5, axis=0, method="linear")
        np.testing.assert_array_equal(got[:, g], want.astype(np.float32))
