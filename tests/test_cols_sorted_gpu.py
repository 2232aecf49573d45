"""quantile / median / mode over leading dims on the sort-in-LDS column kernel
(fh_grouped_quantile_cols): the raw entry against numpy, the ABI corners, the
six API functions against the oracle and against the lead fold
(set_options(cols_sorted_funcs=False)) bit for bit, dispatch, the fallbacks,
groupby_reduce_many, and the 2**31-element array the fold refuses.

The raw reference is np.quantile / np.nanquantile (method="linear") of the
float64 view of each (group, column). Two remarks on it:

* np.quantile interpolates between positions floor(vi) and floor(vi) + 1 with
  weight 0 where vi is whole, the kernel (like k_quantile) between floor(vi)
  and ceil(vi). In finite arithmetic both give the value at vi; where one of
  numpy's pair is infinite, numpy's `inf * 0` turns the result into NaN. The
  rule the kernel documents is restated in numpy below (_rule_quantile),
  checked to agree with np.quantile wherever numpy's pair is finite, and is
  the reference for the remaining (infinite-neighbour) entries.
* the kernel may contract `a + diff * t` into one fused multiply-add: one
  rounding instead of two, so a result may differ from numpy's by one unit in
  the last place of the larger operand. The tolerance is 2**-50 relative plus
  2**-50 of the largest finite magnitude in the case (it matters only for the
  int64 extremes, whose difference is 2**64).
"""

import contextlib
import ctypes
import warnings
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from flox_amd import core as fa_core
from oracle import groupby_reduce as oracle_reduce
from tests.test_cols_order_gpu import (DTYPES, NG, _codes, _device_case, _plant_nans,
                                       _same_bits, _tied_values)
from tests.test_reduce_many_cols_gpu import _sets, _spy_cols
from tests.test_reduce_many_gpu import FFI_DT, _np, _spy

pytestmark = pytest.mark.gpu

CAP = 2048
Q4 = [0.0, 0.25, 0.5, 1.0]
SIX = ("quantile", "nanquantile", "median", "nanmedian", "mode", "nanmode")


def _lib():
    lib = _ffi.load_library()
    assert hasattr(lib, "fh_grouped_quantile_cols"), "library lacks the column quantile entry"
    return lib


# ---- numpy references -----------------------------------------------------------------

def _segments(codes, ng):
    order = np.argsort(codes, kind="stable")
    sc = codes[order]
    lo = np.searchsorted(sc, np.arange(ng), "left")
    hi = np.searchsorted(sc, np.arange(ng), "right")
    return [order[lo[g]:hi[g]] for g in range(ng)]


def _rule_quantile(sub, q, skipnan):
    """the documented rule on a (rows, m) float64 block: (nq, m), and whether
    numpy's interpolation pair (floor(vi), floor(vi) + 1) is finite"""
    r, m = sub.shape
    s = np.sort(sub, axis=0)  # NaN last
    actual = (~np.isnan(s)).sum(0)
    out = np.full((len(q), m), np.nan)
    finite = np.ones((len(q), m), bool)
    ok = (actual > 0) & (skipnan | (actual == r))
    for qi, qq in enumerate(q):
        vi = qq * (actual - 1).astype(np.float64)
        lo = np.clip(np.floor(vi), 0, None).astype(np.int64)
        hi = np.minimum(np.ceil(vi).astype(np.int64), actual - 1)
        lo, hi = np.clip(lo, 0, r - 1), np.clip(hi, 0, r - 1)
        a = np.take_along_axis(s, lo[None], 0)[0]
        b = np.take_along_axis(s, hi[None], 0)[0]
        nxt = np.take_along_axis(s, np.clip(np.minimum(lo + 1, actual - 1), 0, r - 1)[None], 0)[0]
        t = vi - lo
        diff = b - a
        res = np.where(t >= 0.5, b - diff * (1.0 - t), a + diff * t)
        out[qi] = np.where(ok, res, np.nan)
        finite[qi] = np.isfinite(a) & np.isfinite(nxt)
    return out, finite


def _np_sorted(v, codes, ng, q, skipnan):
    """(quantiles (nq, ng, m) f64, mode (ng, m) v.dtype, count (ng, m))"""
    n_t, m = v.shape
    isf = v.dtype.kind == "f"
    quant = np.full((len(q), ng, m), np.nan)
    mode = np.full((ng, m), np.nan if isf else 0, v.dtype)
    count = np.zeros((ng, m), np.int64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN slices
        for g, rows in enumerate(_segments(codes, ng)):
            if len(rows) == 0:
                continue
            sub = v[rows]
            sub64 = sub.astype(np.float64)
            isn = np.isnan(sub64)
            count[g] = (~isn).sum(0)
            rule, finite = _rule_quantile(sub64, q, skipnan)
            ref = (np.nanquantile if skipnan else np.quantile)(sub64, q, axis=0, method="linear")
            np.testing.assert_allclose(
                np.where(finite, rule, 0), np.where(finite, ref, 0), rtol=1e-15, atol=0,
                equal_nan=True, err_msg="the restated rule is np.quantile on finite pairs")
            quant[:, g] = np.where(finite, ref, rule)
            for c in range(m):
                col = sub[:, c]
                if isf:
                    col = np.where(col == 0, 0.0, col).astype(v.dtype)  # -0.0 is +0.0
                nn = col[~isn[:, c]]
                if nn.size == 0:
                    continue  # NaN / 0
                u, cnt = np.unique(nn, return_counts=True)
                best = np.argmax(cnt)  # ties to the smallest value
                if not skipnan and isn[:, c].sum() > cnt[best]:
                    continue  # a strictly longer NaN run wins
                mode[g, c] = u[best]
    return quant, mode, count


def _scale(v):
    f = np.abs(v.astype(np.float64))
    f = f[np.isfinite(f)]
    return float(f.max()) if f.size else 1.0


# ---- the raw entry ----------------------------------------------------------------------

def _raw(vt, sc, perm, ng, q, skipnan, max_seg_rows, want_count=True, drop=None):
    """fh_grouped_quantile_cols through the raw ABI; q None = mode. Outputs are
    pre-filled with -77. `drop` names a buffer left NULL. Returns (rc, out, count)."""
    lib = _lib()
    n_t, m = vt.shape
    nq = 0 if q is None else len(q)
    out = (torch.full((ng, m), -77, dtype=vt.dtype, device="cuda") if q is None
           else torch.full((nq, ng, m), -77.0, dtype=torch.float64, device="cuda"))
    count = torch.full((ng, m), -77, dtype=torch.int64, device="cuda")
    q_t = None if q is None else torch.tensor(q, dtype=torch.float64, device="cuda")
    c = _ffi.FhCall()
    c.vdtype, c.ldtype = FFI_DT[str(vt.dtype)[6:]], _ffi.L_I32
    c.flags = _ffi.FLAG_SKIPNAN if skipnan else 0
    c.n, c.m, c.ldm, c.ngroups = n_t, m, vt.stride(0), ng
    c.values, c.labels, c.perm = vt.data_ptr(), sc.data_ptr(), perm.data_ptr()
    c.out_sum = out.data_ptr()
    if q_t is not None:
        c.means = q_t.data_ptr()
    if want_count:
        c.out_count = count.data_ptr()
    if drop is not None:
        setattr(c, drop, None)
    c.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.fh_grouped_quantile_cols(ctypes.byref(c), nq, max_seg_rows)
    torch.cuda.synchronize()
    if rc == 0:
        assert c.path_used == 3
    return rc, out, count


def _sorted_codes(codes, perm_np=None):
    codes_t = torch.as_tensor(codes).cuda()
    if perm_np is None:
        sc, perm = torch.sort(codes_t, stable=True)
    else:
        perm = torch.as_tensor(perm_np).cuda()
        sc = codes_t[perm]
    return sc.to(torch.int32).contiguous(), perm.to(torch.int32).contiguous()


def _check_raw(vt, v_np, codes, ng, max_seg_rows, qs=(Q4,), perm_np=None):
    sc, perm = _sorted_codes(codes, perm_np)
    tol = dict(rtol=2.0**-50, atol=2.0**-50 * _scale(v_np), equal_nan=True)
    outs = {}
    for skipnan in (False, True):
        for q in qs:
            wq, wmode, wcount = _np_sorted(v_np, codes, ng, q, skipnan)
            rc, got, cnt = _raw(vt, sc, perm, ng, q, skipnan, max_seg_rows)
            assert rc == 0
            with np.errstate(invalid="ignore"):
                np.testing.assert_allclose(_np(got), wq, err_msg=f"q={q} skipnan={skipnan}", **tol)
            np.testing.assert_array_equal(_np(cnt), wcount)
            outs[("q", skipnan, tuple(q))] = got
        rc, got, cnt = _raw(vt, sc, perm, ng, None, skipnan, max_seg_rows)
        assert rc == 0
        g = _np(got)
        np.testing.assert_array_equal(g, wmode, err_msg=f"mode skipnan={skipnan}")
        if g.dtype.kind == "f":  # the merged zero run reports +0.0
            assert not np.signbit(g[g == 0]).any()
        np.testing.assert_array_equal(_np(cnt), wcount)
        outs[("mode", skipnan)] = got
    return outs


def _case(n_t, m, dtype, ldm=None, offset=0, ng=NG, seed="", codes=None):
    rng = np.random.default_rng(zlib.crc32(f"sorted-{n_t}-{m}-{dtype}-{ldm}-{offset}-{seed}".encode()))
    v = _tied_values(rng, n_t, m if ldm is None else ldm, dtype)
    if codes is None:
        codes = _codes(rng, n_t, ng)
    _plant_nans(v, codes)
    return _device_case(v, m, offset), v[:, :m], codes


def _length_codes(sizes, seed):
    """groups 1..len(sizes) of the given sizes, shuffled among 5 % rows in no
    group; groups 0 and len(sizes) + 1 stay empty"""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.full(s, g + 1) for g, s in enumerate(sizes)])
    lab = np.concatenate([lab, np.full(len(lab) // 19, -1)])
    return rng.permutation(lab), len(sizes) + 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sizes,max_seg_rows", [
    ((1, 2, 3, 63, 64, 65, 1023, 1024, 1025, CAP), CAP),  # n_t ~ 5600, exact bound
    ((1, 2, 3, 63, 64, 65, 1023, 1024, 1025), 1025),      # exact bound
    ((1, 2, 3, 63, 64, 65, 1023, 1024, 1025), 2048),      # rounded up to the power of two
    ((1, 2, 3, 63, 64, 65), 65),
    ((1, 2, 3, 63, 64, 65), 128),
], ids=["cap", "1025", "1025up", "65", "65up"])
def test_raw_segment_lengths(sizes, max_seg_rows, dtype):
    codes, ng = _length_codes(sizes, 7)
    vt, v_np, codes = _case(len(codes), 20, dtype, ng=ng, codes=codes, seed=str(max_seg_rows))
    _check_raw(vt, v_np, codes, ng, max_seg_rows, qs=(Q4, [0.5]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 3, 15, 16, 17, 63, 64, 65, 130])
def test_raw_columns_and_layout(m, dtype):
    # ldm > m, the base one element off its allocation: no vector alignment
    vt, v_np, codes = _case(300, m, dtype, ldm=m + 3, offset=1)
    assert vt.data_ptr() % 16 != 0 and vt.stride(0) == m + 3
    longest = int(np.bincount(codes[codes >= 0]).max())
    _check_raw(vt, v_np, codes, NG, longest)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_mode_zero_signs_and_nan_runs(dtype):
    nan = np.nan
    cols = np.array([
        # -0.0 and +0.0 make one run of 3, longer than the run of two 1.0
        [-0.0, 1.0, 0.0, 1.0, -0.0, 5.0, 7.0],
        # NaN run of 3 against a best run of 2: wins only without skipnan
        [nan, 2.0, nan, 2.0, nan, 3.0, 4.0],
        # NaN run of 2 ties the best run of 2: the value wins either way
        [nan, 2.0, nan, 2.0, 9.0, 3.0, 4.0],
    ], dtype=dtype).T.copy()
    codes = np.zeros(7, dtype=np.int64)
    vt = torch.as_tensor(cols).cuda()
    sc, perm = _sorted_codes(codes)
    _, keep, cnt = _raw(vt, sc, perm, 1, None, False, 7)
    _, skip, _ = _raw(vt, sc, perm, 1, None, True, 7)
    keep, skip = _np(keep)[0], _np(skip)[0]
    assert keep[0] == 0 and not np.signbit(keep[0]) and skip[0] == 0
    assert np.isnan(keep[1]) and skip[1] == 2.0
    assert keep[2] == 2.0 and skip[2] == 2.0
    assert _np(cnt)[0].tolist() == [7, 4, 5]
    _check_raw(vt, cols, codes, 1, 7)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32"])
def test_any_sorting_perm_gives_the_same_output(dtype):
    vt, v_np, codes = _case(1500, 12, dtype, seed="rev")
    longest = int(np.bincount(codes[codes >= 0]).max())
    fwd = _check_raw(vt, v_np, codes, NG, longest)
    perm_rev = np.lexsort((-np.arange(len(codes)), codes))
    assert (np.diff(codes[perm_rev]) >= 0).all()
    rev = _check_raw(vt, v_np, codes, NG, longest, perm_np=perm_rev)
    for k in fwd:
        _same_bits(fwd[k], rev[k], k)


def test_no_group_count_cap():
    # more (tile, group) workgroups than a grid dimension of 65535 would hold.
    # No NaN here, so NaN-padding every group to the longest one lets numpy
    # answer all 50 000 groups at once; the mode is checked on a sample
    n_t, ng, m = 60_000, 50_000, 4
    rng = np.random.default_rng(17)
    v = _tied_values(rng, n_t, m, "float32", nan=0)
    v[np.isinf(v)] = 7.0  # finite: np.nanquantile is the reference everywhere
    codes = rng.integers(0, ng, n_t)
    sizes = np.bincount(codes, minlength=ng)
    longest = int(sizes.max())
    order = np.argsort(codes, kind="stable")
    start = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    pad = np.full((ng, longest, m), np.nan)
    pad[codes[order], np.arange(n_t) - start[codes[order]]] = v[order]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # empty groups
        want = np.nanquantile(pad, Q4, axis=1, method="linear")
    vt = torch.as_tensor(v).cuda()
    sc, perm = _sorted_codes(codes)
    rc, got, cnt = _raw(vt, sc, perm, ng, Q4, False, longest)
    assert rc == 0
    np.testing.assert_allclose(_np(got), want, rtol=2.0**-50, atol=2.0**-50 * 7, equal_nan=True)
    np.testing.assert_array_equal(_np(cnt), np.broadcast_to(sizes[:, None], (ng, m)))
    rc, got, cnt = _raw(vt, sc, perm, ng, None, True, longest)
    assert rc == 0
    np.testing.assert_array_equal(_np(cnt), np.broadcast_to(sizes[:, None], (ng, m)))
    g = _np(got)
    assert np.isnan(g[sizes == 0]).all() and not np.isnan(g[sizes > 0]).any()
    for grp in np.concatenate((rng.choice(ng, 300, replace=False), [0, ng - 1])):
        sub = v[codes == grp]
        for c in range(m):
            if len(sub):
                u, n_u = np.unique(np.where(sub[:, c] == 0, 0.0, sub[:, c]), return_counts=True)
                assert g[grp, c] == u[np.argmax(n_u)]


# ---- ABI ------------------------------------------------------------------------------------

def test_abi_capacity_and_refusals():
    lib = _lib()
    assert lib.fh_abi_revision() == 6
    for dt in (_ffi.F32, _ffi.F64, _ffi.I32, _ffi.I64):
        assert lib.fh_quantile_cols_max_rows(dt) == CAP == _ffi.quantile_cols_max_rows(dt)
    assert lib.fh_quantile_cols_max_rows(99) == 0
    vt, v_np, codes = _case(301, 4, "float64")
    sc, perm = _sorted_codes(codes)

    def untouched(rc, out, cnt, code):
        assert rc == code
        assert bool((out == -77).all()) and bool((cnt == -77).all())

    for q in (None, [0.5]):
        untouched(*_raw(vt, sc, perm, NG, q, False, CAP + 1), 20)
        untouched(*_raw(vt, sc, perm, NG, q, False, 1 << 40), 20)
        for drop in ("values", "labels", "perm", "out_sum"):
            untouched(*_raw(vt, sc, perm, NG, q, False, 301, drop=drop), 21)
    untouched(*_raw(vt, sc, perm, NG, [0.5], False, 301, drop="means"), 21)
    # the counts are optional
    rc, out, cnt = _raw(vt, sc, perm, NG, [0.5], True, 301, want_count=False)
    assert rc == 0 and bool((cnt == -77).all()) and not bool((out == -77).any())
    with pytest.raises(RuntimeError, match="floxhip error 20"):
        aggregate_hip.grouped_mode_cols(vt, sc, perm, NG, max_seg_rows=CAP + 1)


# ---- API parity ---------------------------------------------------------------------------------

def _api_values(rng, n_t, m, dtype):
    """finite values with ties (so modes exist), 5 % NaN for floats"""
    v = np.round(rng.standard_normal((n_t, m)) * 3)
    if np.dtype(dtype).kind == "f":
        v = (v / 2).astype(dtype)
        v[rng.random((n_t, m)) < 0.05] = np.nan
        return v
    return v.astype(dtype)


def _api_case(dtype, n_t=1003, m=7, ng=NG):
    rng = np.random.default_rng(zlib.crc32(f"sorted-api-{dtype}-{n_t}-{m}".encode()))
    v = _api_values(rng, n_t, m, dtype)
    lab = _codes(rng, n_t, ng)
    _plant_nans(v, lab)
    return v, lab


@contextlib.contextmanager
def _spy_sorted():
    """records the calls core makes to the column entry ("cols", values
    data_ptr, row stride), to the 1-D sorted entries ("1d") and to the lead
    fold ("fold")"""
    seen = []
    names = ("grouped_quantile_cols", "grouped_mode_cols", "grouped_quantile", "grouped_mode")
    orig = {k: getattr(aggregate_hip, k) for k in names}
    orig_fold = fa_core._fold_lead

    def wrap(name):
        def w(values, *a, **kw):
            seen.append(("cols", values.data_ptr(), values.stride(0)) if name.endswith("_cols")
                        else ("1d",))
            return orig[name](values, *a, **kw)
        return w

    def fold(*a, **kw):
        seen.append(("fold",))
        return orig_fold(*a, **kw)

    for k in names:
        setattr(aggregate_hip, k, wrap(k))
    fa_core._fold_lead = fold
    try:
        yield seen
    finally:
        for k in names:
            setattr(aggregate_hip, k, orig[k])
        fa_core._fold_lead = orig_fold


def _kinds(seen):
    return [s[0] for s in seen]


def _q_tol(dtype):
    # the tolerances of tests/test_hip_parity.py::test_quantile_family_vs_oracle
    d = np.dtype(dtype)
    return dict(rtol=3e-6, atol=1e-5) if d.itemsize == 4 and d.kind == "f" else dict(rtol=1e-12, atol=1e-12)


def _check_api(arr, arr_np, bys, func, vt=None, oracle=True, tol_dtype=None, **kw):
    """groupby_reduce on the column entry against the same call through the
    lead fold (bit for bit) and against the oracle"""
    as_numpy = not isinstance(arr, torch.Tensor)
    bin_ = bys if as_numpy else tuple(torch.as_tensor(b).cuda() for b in bys)
    if "quantile" in func and "finalize_kwargs" not in kw:
        kw["finalize_kwargs"] = {"q": Q4}
    with _spy_sorted() as seen:
        got, *groups = flox_amd.groupby_reduce(arr, *bin_, func=func, **kw)
    assert _kinds(seen) == ["cols"], (func, seen)
    if vt is not None:
        assert seen[0][1:] == (vt.data_ptr(), vt.stride(0))  # zero copy
    with flox_amd.set_options(cols_sorted_funcs=False), _spy_sorted() as seen_off:
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
    if "mode" in func:
        np.testing.assert_array_equal(g, want, err_msg=f"{func} vs oracle")
    else:
        np.testing.assert_allclose(g, want, equal_nan=True, err_msg=f"{func} vs oracle",
                                   **_q_tol(tol_dtype or arr_np.dtype))
    for a, c in zip(groups, wg):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("func", SIX)
def test_api_parity(func, dtype):
    v, lab = _api_case(dtype)
    vt = torch.as_tensor(v).cuda()
    kw = dict(expected_groups=np.arange(NG))
    got = _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, **kw)
    assert isinstance(got, torch.Tensor)
    assert got.shape == ((4, 7, NG) if "quantile" in func else (7, NG))
    got_np = _check_api(np.ascontiguousarray(v.T), v.T, (lab,), func, **kw)
    assert isinstance(got_np, np.ndarray)


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
@pytest.mark.parametrize("func", ("median", "nanquantile", "mode", "nanmode"))
@pytest.mark.parametrize("kw", [
    dict(fill_value=-7),
    dict(min_count=3, fill_value=-9),
    dict(min_count=1, fill_value=-5),  # all-NaN groups count 0 and fill
], ids=["fill", "min_count3", "min_count1"])
def test_api_fill_value_and_min_count(kw, func, dtype):
    v, lab = _api_case(dtype)
    lab[lab == 7] = 6
    lab[:2] = 7  # a group of two rows: below min_count=3
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, expected_groups=np.arange(NG), **kw)


@pytest.mark.parametrize("func", ("nanmedian", "quantile", "mode"))
def test_api_sort_false(func):
    rng = np.random.default_rng(13)
    n_t, m = 1007, 5
    by = rng.choice([30, 5, 17, 2, 44, 9], n_t)
    v = _api_values(rng, n_t, m, "float32")
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (by,), func, vt=vt, sort=False)


@pytest.mark.parametrize("func", ("median", "nanquantile", "nanmode"))
def test_api_two_by(func):
    rng = np.random.default_rng(15)
    n_t, m = 2003, 6
    b0, b1 = rng.integers(-1, 5, n_t), rng.integers(-1, 8, n_t)
    v = _api_values(rng, n_t, m, "float64")
    vt = torch.as_tensor(v).cuda()
    got = _check_api(vt.permute(1, 0), v.T, (b0, b1), func, vt=vt,
                     expected_groups=(np.arange(4), np.arange(7)))
    assert got.shape == ((4, m, 4, 7) if "quantile" in func else (m, 4, 7))


@pytest.mark.parametrize("func", ("median", "quantile", "mode"))
@pytest.mark.parametrize("dtype", ["bool", "int8", "uint8", "int16"])
def test_api_bool_and_small_dtypes(dtype, func):
    rng = np.random.default_rng(16)
    n_t, m = 611, 5
    v = rng.integers(0, 2 if dtype == "bool" else 5, (m, n_t)).astype(dtype)
    lab = _codes(rng, n_t, NG)
    _check_api(v, v, (lab,), func, expected_groups=np.arange(NG), tol_dtype="int64")
    # a torch tensor of a small dtype comes back in torch's dtype, where the
    # empty-group fill is not numpy's: the fold is the reference there
    _check_api(torch.as_tensor(v).cuda(), v, (lab,), func, oracle=False,
               expected_groups=np.arange(NG))


def test_api_three_leading_dims():
    rng = np.random.default_rng(18)
    v = _api_values(rng, 3 * 4, 50, "float32").reshape(3, 4, 50)
    lab = rng.integers(0, 4, 50)
    for func in ("nanmedian", "quantile", "mode"):
        got = _check_api(torch.as_tensor(v).cuda(), v, (lab,), func, expected_groups=np.arange(4))
        assert got.shape == ((4, 3, 4, 4) if func == "quantile" else (3, 4, 4))


# ---- dispatch and the fallbacks --------------------------------------------------------------------

def _both_ways(arr, by, **kw):
    with _spy_sorted() as seen:
        on = flox_amd.groupby_reduce(arr, by, **kw)
    with flox_amd.set_options(cols_sorted_funcs=False):
        off = flox_amd.groupby_reduce(arr, by, **kw)
    return on, off, _kinds(seen)


def test_eligible_calls_build_no_composite_labels():
    v, lab = _api_case("float32")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    for func in ("nanmedian", "mode"):
        with _spy_sorted() as seen, _spy() as seen1d, _spy_cols() as seen_cols:
            flox_amd.groupby_reduce(arr, lt, func=func, expected_groups=np.arange(NG))
        # one column call: no fold, no 1-D sort, and no SET_COUNT pass either
        assert _kinds(seen) == ["cols"] and seen1d == [] and seen_cols == []


@pytest.mark.parametrize("func", ("median", "mode"))
def test_datetime_values_keep_the_fold(func):
    rng = np.random.default_rng(19)
    v = rng.integers(0, 5, (4, 300)).astype("datetime64[ns]")
    lab = rng.integers(0, 5, 300)
    on, off, kinds = _both_ways(v, lab, func=func, expected_groups=np.arange(6))
    assert kinds == ["fold", "1d"]
    _same_bits(on[0], off[0], func)


@pytest.mark.parametrize("func", ("nanmedian", "nanmode"))
def test_axis_subset_keeps_the_fold(func):
    rng = np.random.default_rng(20)
    v = _api_values(rng, 12, 50, "float64").reshape(3, 4, 50)
    by = rng.integers(0, 4, (4, 50))
    kw = dict(func=func, axis=(2,), expected_groups=np.arange(4), fill_value=-9.0)
    on, off, kinds = _both_ways(torch.as_tensor(v).cuda(), torch.as_tensor(by).cuda(), **kw)
    assert kinds == ["fold", "1d"]
    assert on[0].shape == (3, 4, 4)
    _same_bits(on[0], off[0], func)


@pytest.mark.parametrize("func", ("nanmedian", "mode"))
def test_a_group_over_capacity_keeps_the_fold(func):
    rng = np.random.default_rng(21)
    n_t, m = CAP + 40, 3
    v = _api_values(rng, n_t, m, "float32")
    arr = torch.as_tensor(v).cuda().permute(1, 0)
    lab = np.zeros(n_t, dtype=np.int64)
    lab[CAP + 1:] = 1  # group 0 has CAP + 1 rows
    lt = torch.as_tensor(lab).cuda()
    on, off, kinds = _both_ways(arr, lt, func=func, expected_groups=np.arange(2))
    assert kinds == ["fold", "1d"]
    _same_bits(on[0], off[0], func)
    lab[CAP] = 1  # exactly the capacity: the column entry
    on, off, kinds = _both_ways(arr, torch.as_tensor(lab).cuda(), func=func, expected_groups=np.arange(2))
    assert kinds == ["cols"]
    _same_bits(on[0], off[0], func)


@pytest.mark.parametrize("func", ("mode", "nanmode"))
def test_capture_keeps_the_fold_and_replays_the_eager_result(func):
    # the column form reads the sorted codes on the host to bound the longest
    # group, which a capturing stream cannot: the fold runs. (The quantile
    # names copy q from host memory on either path and cannot be captured.)
    v, lab = _api_case("float32", n_t=1101, m=12)
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(func=func, expected_groups=np.arange(NG))
    eager, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g), _spy_sorted() as seen:
            res, _ = flox_amd.groupby_reduce(arr, lt, **kw)
    assert _kinds(seen) == ["fold", "1d"]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _same_bits(res, eager, func)


def test_many_mean_median_mode():
    v, lab = _api_case("float64")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(expected_groups=np.arange(NG))
    funcs = ("mean", "median", "mode")
    with _spy_sorted() as seen:
        res, _ = flox_amd.groupby_reduce_many(arr, lt, funcs=funcs, **kw)
    assert _kinds(seen) == ["cols", "cols"]
    for f in funcs:
        single, _ = flox_amd.groupby_reduce(arr, lt, func=f, **kw)
        _same_bits(res[f], single, f)


# ---- the size limit -------------------------------------------------------------------------------------

def test_two_to_the_31_elements():
    n_t, m, ng = 2**11, 2**20, 3
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
    lab = torch.arange(n_t, device="cuda") % ng
    arr = vt.permute(1, 0)
    with _spy_sorted() as seen:
        med, _ = flox_amd.groupby_reduce(arr, lab, func="nanmedian", expected_groups=np.arange(ng))
    assert seen == [("cols", vt.data_ptr(), vt.stride(0))]
    assert med.shape == (m, ng) and med.dtype == torch.float32
    cols = torch.as_tensor(np.random.default_rng(4).choice(m, 4096, replace=False)).cuda()
    sample = vt[:, cols].cpu().numpy().astype(np.float64)
    got = med[cols].cpu().numpy()
    for g in range(ng):
        want = np.nanquantile(sample[g::ng], 0.5, axis=0, method="linear")
        np.testing.assert_array_equal(got[:, g], want.astype(np.float32))
