"""groupby_reduce_many and FH_SET_SUMMARY on the GPU: every result against the
oracle and against the single-func call, on the shapes where the fused kernel
can go wrong; one pass; the label cache; the variance numerics; capture; and
the C boundary."""

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

FIVE = ("mean", "std", "min", "max", "count")
ALL13 = ("count", "sum", "nansum", "mean", "nanmean", "var", "nanvar", "std",
         "nanstd", "min", "nanmin", "max", "nanmax")
# bit-identical to the single-func call, whatever the dtype
EXACT = ("count", "min", "nanmin", "max", "nanmax")
N_PAST_GRID = 5_200_005  # past one grid stride of the u16-code kernel
FFI_DT = {"float32": _ffi.F32, "float64": _ffi.F64, "int32": _ffi.I32, "int64": _ffi.I64}


@contextlib.contextmanager
def _spy():
    """records the op set of every grouped_partials call core makes"""
    seen = []
    orig = fa_core.grouped_partials

    def wrapper(op_set, *a, **kw):
        seen.append(op_set)
        return orig(op_set, *a, **kw)

    fa_core.grouped_partials = wrapper
    try:
        yield seen
    finally:
        fa_core.grouped_partials = orig


def _values(rng, n, dtype, nan_rows=None):
    if np.dtype(dtype).kind == "f":
        v = (rng.standard_normal(n) * 100).astype(dtype)
        if n:
            v[rng.random(n) < 0.03] = np.nan
        if nan_rows is not None:
            v[nan_rows] = np.nan
    else:
        v = rng.integers(-1000, 1000, n).astype(dtype)
    return v


def _labels(rng, n, ng, ldtype="int64", empty=()):
    lab = rng.integers(0, ng, n).astype(ldtype)
    if n:
        k = rng.random(n)
        lab[k < 0.02] = -1
        lab[(k >= 0.02) & (k < 0.04)] = ng
        lab[(k >= 0.04) & (k < 0.05)] = ng + 70_000
    for g in empty:  # groups that receive no row
        lab[lab == g] = -1
    return lab


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _kw_for(kw, f):
    """the single-func keywords of func f, by the rules of groupby_reduce_many"""
    out = {}
    for k, v in kw.items():
        keyed = k in ("fill_value", "dtype", "min_count", "finalize_kwargs") and isinstance(v, dict)
        if keyed and k == "finalize_kwargs":  # a dict of dicts is keyed by func
            keyed = bool(v) and all(isinstance(x, dict) for x in v.values())
        out[k] = v.get(f) if keyed else v
    return out


def _compare(got, single, want, func, vkind):
    g, s = _np(got), _np(single)
    assert type(got) is type(single), (func, type(got), type(single))
    assert g.shape == s.shape == want.shape, (func, g.shape, s.shape, want.shape)
    assert g.dtype == s.dtype, (func, g.dtype, s.dtype)
    exact = func in EXACT or (vkind in "iu" and func in ("sum", "nansum"))
    if g.dtype.kind in "Mm":
        np.testing.assert_array_equal(g, s, err_msg=f"{func} vs single")
        np.testing.assert_array_equal(g, want, err_msg=f"{func} vs oracle")
        return
    tol = _tol(func, want.dtype)
    np.testing.assert_allclose(g, want, equal_nan=True, err_msg=f"{func} vs oracle", **tol)
    if exact:
        np.testing.assert_array_equal(g, s, err_msg=f"{func} vs single")
    else:
        np.testing.assert_allclose(g, s, equal_nan=True, err_msg=f"{func} vs single", **tol)


def _check(vals, bys, funcs, summary, calls=1, as_numpy=False, **kw):
    """`calls` groupby_reduce_many calls, each checked func by func against the
    oracle and the single-func call. summary: whether exactly one SET_SUMMARY
    pass must serve the call (True), none may (False), or either (None)."""
    vkind = np.dtype(vals.dtype).kind
    if as_numpy:
        vin, bin_ = vals, bys
    else:
        vin = torch.as_tensor(vals).cuda()
        bin_ = tuple(torch.as_tensor(b).cuda() for b in bys)
    ref = {}
    for f in funcs:
        kwf = _kw_for(kw, f)
        want, *wg = oracle_reduce(vals, *bys, func=f, **kwf)
        single, *sg = flox_amd.groupby_reduce(vin, *bin_, func=f, **kwf)
        ref[f] = (want, single, wg, sg)
    flox_amd.clear_label_cache()
    out = None
    for _ in range(calls):
        with _spy() as seen:
            results, *groups = flox_amd.groupby_reduce_many(vin, *bin_, funcs=funcs, **kw)
        if summary is not None:
            assert seen.count(_ffi.SET_SUMMARY) == (1 if summary else 0), seen
        assert list(results) == list(funcs)
        for f in funcs:
            want, single, wg, sg = ref[f]
            _compare(results[f], single, want, f, vkind)
            assert len(groups) == len(sg) == len(wg)
            for a, b, c in zip(groups, sg, wg):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
                np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
        out = results
    return out


def _run(n, ng, vdtype, funcs=ALL13, ldtype="int64", summary=True, calls=1, **kw):
    rng = np.random.default_rng(zlib.crc32(f"many-{n}-{ng}-{vdtype}-{ldtype}".encode()))
    lab = _labels(rng, n, ng, ldtype, empty=(0, ng // 2) if ng > 2 else ())
    # group 1 is all NaN (float dtypes)
    vals = _values(rng, n, vdtype, nan_rows=(lab == 1) if ng > 2 else None)
    return _check(vals, (lab,), funcs, summary, calls=calls,
                  expected_groups=np.arange(ng), **kw)


# ---- shapes --------------------------------------------------------------------

@pytest.mark.parametrize("vdtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("n", [1, 7, 8 * 3072 + 3, 200_003])
def test_row_counts(n, vdtype):
    # three calls: plain labels, the emitting form, then the u16 codes
    _run(n, 7, vdtype, calls=3)


@pytest.mark.parametrize("vdtype", ["float32", "int64"])
def test_no_rows_falls_back(vdtype):
    _run(0, 7, vdtype, summary=False)


@pytest.mark.parametrize("vdtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("ng", [1, 7, 1000])
def test_group_counts(ng, vdtype):
    _run(20_011, ng, vdtype, calls=3)


def test_past_one_grid_stride():
    _run(N_PAST_GRID, 7, "float32", funcs=FIVE, calls=3)


@pytest.mark.parametrize("ldtype", ["int64", "int32"])
@pytest.mark.parametrize("vdtype", ["float32", "float64", "int32", "int64"])
def test_label_dtypes(vdtype, ldtype):
    _run(30_003, 257, vdtype, ldtype=ldtype, calls=3)


# ---- LDS capacity edge ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _max_summary_groups(vdtype):
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.op_set, c.vdtype = _ffi.SET_SUMMARY, FFI_DT[vdtype]

    def fits(ng):
        c.ngroups = ng
        return lib.fh_query_path(ctypes.byref(c)) == 1

    lo, hi = 1, 1 << 17
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("vdtype", ["float32", "float64", "int32", "int64"])
def test_largest_lds_group_count_and_one_more(vdtype):
    ng = _max_summary_groups(vdtype)
    # 44 B (4-byte dtypes) and 56 B (8-byte) per group, in 256-B sections
    assert 2500 < ng < 4000
    assert aggregate_hip.summary_fits(getattr(torch, vdtype), ng)
    assert not aggregate_hip.summary_fits(getattr(torch, vdtype), ng + 1)
    _run(60_007, ng, vdtype, funcs=FIVE + ("nanvar", "sum"), summary=True)
    _run(60_007, ng + 1, vdtype, funcs=FIVE + ("nanvar", "sum"), summary=False)


# ---- several by, bins, order -----------------------------------------------------

@pytest.mark.parametrize("vdtype,ldtype", [("float32", "int64"), ("float64", "int32")])
def test_two_by_reindexes_to_expected_groups(vdtype, ldtype):
    rng = np.random.default_rng(11)
    n = 50_003
    # labels beyond the expected 12 x 180 grid fall in no group
    b0 = rng.integers(-1, 14, n).astype(ldtype)
    b1 = rng.integers(-1, 183, n).astype(ldtype)
    vals = _values(rng, n, vdtype)
    res = _check(vals, (b0, b1), FIVE + ("nansum",), True, calls=3,
                 expected_groups=(np.arange(12), np.arange(180)))
    assert _np(res["mean"]).shape == (12, 180)


def test_isbin():
    rng = np.random.default_rng(12)
    n = 20_003
    by = rng.standard_normal(n) * 2
    vals = _values(rng, n, "float64")
    edges = np.array([-3.0, -1.0, 0.0, 1.0, 3.0])
    _check(vals, (by,), FIVE + ("var",), True, expected_groups=edges, isbin=True)


def test_sort_false_keeps_first_appearance_order():
    rng = np.random.default_rng(13)
    n = 10_007
    by = rng.choice([30, 5, 17, 2, 44, 9], n)
    vals = _values(rng, n, "float32")
    _check(vals, (by,), FIVE + ("nanmax",), None, sort=False)


# ---- one pass ------------------------------------------------------------------

SEVEN = ("mean", "std", "min", "max", "count", "nanvar", "sum")


def _resident(n=100_003, ng=257, vdtype="float32", seed=21):
    rng = np.random.default_rng(seed)
    vals = torch.as_tensor(_values(rng, n, vdtype)).cuda()
    lab = torch.as_tensor(_labels(rng, n, ng)).cuda()
    return vals, lab, np.arange(ng)


def test_one_summary_pass_serves_seven_funcs():
    vals, lab, expected = _resident()
    flox_amd.clear_label_cache()
    with _spy() as seen:
        flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN, expected_groups=expected)
    assert seen == [_ffi.SET_SUMMARY]
    # the cache's policy: the second sighting of a `by` tensor emits the codes
    # (through the fused kernel), every later call reads them back
    s0 = flox_amd.label_cache_stats()
    flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN, expected_groups=expected)
    s1 = flox_amd.label_cache_stats()
    assert (s1["emits"], s1["hits"]) == (s0["emits"] + 1, s0["hits"])
    with _spy() as seen:
        flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN, expected_groups=expected)
    assert seen == [_ffi.SET_SUMMARY]
    assert flox_amd.label_cache_stats()["hits"] == s1["hits"] + 1


def test_factorization_runs_once_per_call(monkeypatch):
    vals, lab, _ = _resident()
    calls = []
    orig = fa_core._factorize_device
    monkeypatch.setattr(fa_core, "_factorize_device",
                        lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN + ("median",))
    assert len(calls) == 1
    calls.clear()
    flox_amd.groupby_reduce_many(vals, lab, funcs=("mean", "median"))
    assert len(calls) == 2  # nothing to share: the plain per-func calls


def test_no_summary_pass_when_it_does_not_apply():
    vals, lab, expected = _resident()
    kw = dict(expected_groups=expected)
    with flox_amd.set_options(fused_many=False), _spy() as seen:
        flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN, **kw)
    assert _ffi.SET_SUMMARY not in seen and len(seen) >= len(SEVEN)
    with _spy() as seen:  # one fused-set name among others
        flox_amd.groupby_reduce_many(vals, lab, funcs=("std", "median", "argmax"), **kw)
    assert _ffi.SET_SUMMARY not in seen
    with _spy() as seen:  # a single name
        flox_amd.groupby_reduce_many(vals, lab, funcs=("mean",), **kw)
    assert seen == [_ffi.SET_SUM_COUNT]
    with _spy() as seen:  # too many groups for the LDS bins
        big = _max_summary_groups("float32") + 1
        flox_amd.groupby_reduce_many(vals, lab, funcs=SEVEN, expected_groups=np.arange(big))
    assert _ffi.SET_SUMMARY not in seen
    with _spy() as seen:  # leading dims: the column path
        flox_amd.groupby_reduce_many(vals[:100_000].reshape(4, 25_000), lab[:25_000],
                                     funcs=("mean", "max"), **kw)
    assert _ffi.SET_SUMMARY not in seen


def test_column_path_and_complex_fall_back():
    rng = np.random.default_rng(23)
    arr = rng.standard_normal((3, 500))
    by = rng.integers(0, 6, 500)
    _check(arr, (by,), FIVE, False, as_numpy=True, expected_groups=np.arange(6))
    z = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex128)
    zb = rng.integers(0, 5, 300)
    with _spy() as seen:
        res, _ = flox_amd.groupby_reduce_many(z, zb, funcs=("mean", "sum", "count"))
    assert _ffi.SET_SUMMARY not in seen
    for f in res:
        single, _ = flox_amd.groupby_reduce(z, zb, func=f)
        np.testing.assert_array_equal(res[f], single)


# ---- variance numerics -----------------------------------------------------------

# max relative error over the groups of groupby_reduce(func="var") and
# (func="std"), the two-pass path, against the oracle on the inputs of
# _var_case, measured on an MI355X (profiles/r05_fused_many.md; five runs each,
# the largest kept): f64 5.754e-13 / 2.878e-13, f32 0 / 0 (the f32 results are
# identical), int64 6.131e-13 / 3.065e-13. The fused path, one pass over
# per-block pivots plus a Chan merge where that path makes two passes, is
# allowed VAR_SLACK times these: 2.30e-12 / 1.15e-12, 0 / 0, 2.45e-12 /
# 1.23e-12. It measured 5.754e-13 / 2.877e-13, 0 / 0 and 5.971e-13 / 2.986e-13.
TWO_PASS_ERR = {
    "float64": {"var": 5.754e-13, "std": 2.878e-13},
    "float32": {"var": 0.0, "std": 0.0},
    "int64": {"var": 6.131e-13, "std": 3.065e-13},
}
VAR_SLACK = 4.0


def _var_case(vdtype):
    rng = np.random.default_rng(zlib.crc32(f"var-{vdtype}".encode()))
    n, ng = 200_003, 7
    lab = rng.integers(0, ng, n)
    if vdtype == "float64":
        vals = 1e8 + rng.standard_normal(n)
    elif vdtype == "float32":
        vals = (1e3 + rng.standard_normal(n)).astype(np.float32)
    else:
        vals = 10**6 + rng.integers(-10, 11, n)
    return vals, lab, ng


def _relerr(got, want):
    got, want = _np(got).astype(np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("vdtype", ["float64", "float32", "int64"])
def test_variance_numerics(vdtype):
    vals, lab, ng = _var_case(vdtype)
    vt, lt = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    funcs = ("var", "nanvar", "std", "mean", "count")
    with _spy() as seen:
        res, _ = flox_amd.groupby_reduce_many(vt, lt, funcs=funcs, expected_groups=np.arange(ng))
    assert seen == [_ffi.SET_SUMMARY]
    for f in ("var", "nanvar", "std"):
        bound = VAR_SLACK * TWO_PASS_ERR[vdtype]["std" if f == "std" else "var"]
        want, _ = oracle_reduce(vals, lab, func=f, expected_groups=np.arange(ng))
        two_pass, _ = flox_amd.groupby_reduce(vt, lt, func=f, expected_groups=np.arange(ng))
        got = _np(res[f])
        print(f"{vdtype} {f}: two-pass err {_relerr(two_pass, want):.3e} "
              f"fused err {_relerr(got, want):.3e} bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and np.all(got >= 0), (f, got)
        assert _relerr(got, want) <= bound, (f, _relerr(got, want), bound)


def test_no_negative_variance_on_constant_groups():
    # zero spread far from zero: s2 - s1^2/n and the merges must not dip below 0
    n, ng = 100_003, 5
    rng = np.random.default_rng(31)
    lab = rng.integers(0, ng, n)
    vals = (1e8 + lab * 0.1).astype(np.float64)
    vt, lt = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    res, _ = flox_amd.groupby_reduce_many(vt, lt, funcs=("var", "std"),
                                          expected_groups=np.arange(ng))
    assert np.array_equal(_np(res["var"]), np.zeros(ng))
    assert np.array_equal(_np(res["std"]), np.zeros(ng))


# ---- NaN derivation ----------------------------------------------------------------

@pytest.mark.parametrize("vdtype", ["float32", "float64"])
def test_one_nan_among_finite_rows(vdtype):
    vals = np.array([1.0, 2.0, np.nan, 4.0, 5.0, 7.0], dtype=vdtype)
    lab = np.array([0, 0, 0, 0, 1, 1])
    res = _check(vals, (lab,), ALL13, True, expected_groups=np.arange(2))
    for f in ("sum", "mean", "var", "std", "min", "max"):
        r = _np(res[f])
        assert np.isnan(r[0]) and np.isfinite(r[1]), (f, r)
        assert np.all(np.isfinite(_np(res["nan" + f]))), f
    assert _np(res["count"]).tolist() == [3, 2]
    assert _np(res["nansum"])[0] == 7 and _np(res["nanmin"])[0] == 1 and _np(res["nanmax"])[0] == 4


# ---- argument forms --------------------------------------------------------------------

def _sparse_case(vdtype="float64", n=4003, ng=9):
    """group 0 empty, group 1 all NaN, group 2 with two rows"""
    rng = np.random.default_rng(41)
    lab = rng.integers(3, ng, n)
    lab[:2] = 2
    lab[2:6] = 1
    vals = _values(rng, n, vdtype)
    if np.dtype(vdtype).kind == "f":
        vals[:2] = [1.5, 2.5]
        vals[2:6] = np.nan
    return vals, lab, ng


@pytest.mark.parametrize("vdtype", ["float64", "int32"])
@pytest.mark.parametrize("kw", [
    dict(fill_value=-7.0),
    dict(fill_value={"mean": -1.0, "count": -2, "nanmax": 123.0}),
    dict(min_count=3, fill_value=-9.0),
    dict(min_count={"sum": 3, "nanmin": 5}, fill_value=-9.0),
    dict(min_count=3, fill_value={"mean": 0.5, "sum": 1.0, "nanmin": 2.0, "count": 3,
                                  "nanmax": 4.0, "var": 5.0, "min": 6.0}),
])
def test_fill_value_and_min_count_forms(vdtype, kw):
    vals, lab, ng = _sparse_case(vdtype)
    _check(vals, (lab,), ("mean", "sum", "nanmin", "count", "nanmax", "var", "min"), True,
           expected_groups=np.arange(ng), **kw)


def test_dtype_and_finalize_kwargs_per_func():
    vals, lab, ng = _sparse_case()
    res = _check(vals, (lab,), ("mean", "var", "nanstd", "sum"), True,
                 expected_groups=np.arange(ng), dtype={"mean": np.float32},
                 finalize_kwargs={"var": {"ddof": 1}})
    assert _np(res["mean"]).dtype == np.float32 and _np(res["var"]).dtype == np.float64
    ddof0, _ = flox_amd.groupby_reduce(torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda(),
                                       func="var", expected_groups=np.arange(ng))
    assert not np.allclose(_np(res["var"])[3:], _np(ddof0)[3:], rtol=1e-9)
    # one finalize_kwargs for every func
    _check(vals, (lab,), ("var", "nanstd", "mean"), True, expected_groups=np.arange(ng),
           finalize_kwargs={"ddof": 2})


@pytest.mark.parametrize("as_numpy", [True, False])
def test_container_type_follows_the_input(as_numpy):
    vals, lab, ng = _sparse_case("float32")
    res = _check(vals, (lab,), FIVE, True, as_numpy=as_numpy, expected_groups=np.arange(ng))
    want_type = np.ndarray if as_numpy else torch.Tensor
    assert all(isinstance(r, want_type) for r in res.values())


def test_results_do_not_share_storage():
    vals, lab, expected = _resident(vdtype="int64")
    res, _ = flox_amd.groupby_reduce_many(
        vals, lab, funcs=("min", "nanmin", "max", "count", "sum", "nansum"),
        expected_groups=expected)
    ptrs = [r.data_ptr() for r in res.values()]
    assert len(set(ptrs)) == len(ptrs)


def test_datetime_by():
    rng = np.random.default_rng(43)
    n = 5003
    by = np.datetime64("2022-03-01") + rng.integers(0, 12, n).astype("timedelta64[D]")
    vals = _values(rng, n, "float64")
    _check(vals, (by,), FIVE + ("nansum",), True, as_numpy=True)


def test_datetime_values_fall_back():
    rng = np.random.default_rng(44)
    n = 2003
    tv = np.datetime64("2022-03-01") + rng.integers(0, 9000, n).astype("timedelta64[m]")
    tv[rng.random(n) < 0.2] = np.datetime64("NaT")
    by = rng.integers(0, 6, n)
    _check(tv, (by,), ("min", "max", "count"), False, as_numpy=True,
           expected_groups=np.arange(6))


def test_mixed_funcs_come_from_their_own_paths():
    rng = np.random.default_rng(45)
    n, ng = 20_003, 33
    lab = _labels(rng, n, ng, empty=(0,))
    vals = _values(rng, n, "float64", nan_rows=lab == 1)
    funcs = ("mean", "median", "argmax", "std")
    _check(vals, (lab,), funcs, True, expected_groups=np.arange(ng))
    with _spy() as seen:
        flox_amd.groupby_reduce_many(torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda(),
                                     funcs=funcs, expected_groups=np.arange(ng))
    # mean and std shared the summary pass; argmax made its own two
    assert seen.count(_ffi.SET_SUMMARY) == 1 and _ffi.SET_IDXMIN in seen
    assert _ffi.SET_SUM_COUNT not in seen and _ffi.SET_SSD not in seen


# ---- capture ----------------------------------------------------------------------------

def test_many_under_graph_capture():
    vals, lab, expected = _resident(n=100_000, ng=1000, seed=5)
    eager, _ = flox_amd.groupby_reduce_many(vals, lab, funcs=FIVE, expected_groups=expected)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g), _spy() as seen:
            res, _ = flox_amd.groupby_reduce_many(vals, lab, funcs=FIVE, expected_groups=expected)
    assert seen == [_ffi.SET_SUMMARY]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for f in FIVE:
            if f in EXACT:
                np.testing.assert_array_equal(_np(res[f]), _np(eager[f]), err_msg=f)
            else:
                np.testing.assert_allclose(_np(res[f]), _np(eager[f]), equal_nan=True,
                                           err_msg=f, **_tol(f, np.float32))


# ---- the C boundary ------------------------------------------------------------------------

def _raw_summary_call(vals, lab, ng, outs, scratch):
    c = _ffi.FhCall()
    c.op_set, c.vdtype, c.ldtype = _ffi.SET_SUMMARY, _ffi.F64, _ffi.L_I64
    c.flags = _ffi.FLAG_SKIPNAN
    c.n, c.ngroups = vals.numel(), ng
    c.values, c.labels = vals.data_ptr(), lab.data_ptr()
    c.out_sum, c.out_count = outs["sum"].data_ptr(), outs["count"].data_ptr()
    c.out_present, c.out_nanflag = outs["present"].data_ptr(), outs["nanflag"].data_ptr()
    c.out_min, c.out_max = outs["min"].data_ptr(), outs["max"].data_ptr()
    c.out_ssd = outs["ssd"].data_ptr()
    if scratch is not None:
        c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel()
    c.stream = torch.cuda.current_stream().cuda_stream
    return c


def _raw_outs(ng, mark):
    dev = "cuda"
    return {
        "sum": torch.full((ng,), mark, dtype=torch.float64, device=dev),
        "count": torch.full((ng,), mark, dtype=torch.int64, device=dev),
        "present": torch.full((ng,), mark, dtype=torch.int32, device=dev),
        "nanflag": torch.full((ng,), mark, dtype=torch.int32, device=dev),
        "min": torch.full((ng,), mark, dtype=torch.float64, device=dev),
        "max": torch.full((ng,), mark, dtype=torch.float64, device=dev),
        "ssd": torch.full((ng,), mark, dtype=torch.float64, device=dev),
    }


def test_raw_abi_summary_against_numpy():
    lib = _ffi.load_library()
    assert lib.fh_abi_revision() >= 4
    rng = np.random.default_rng(51)
    n, ng = 30_011, 6
    lab_np = rng.integers(-1, ng + 1, n)  # -1 and ng: in no group
    lab_np[lab_np == 4] = -1              # group 4 empty
    vals_np = 50.0 + rng.standard_normal(n) * 3
    vals_np[rng.random(n) < 0.05] = np.nan
    vals_np[lab_np == 5] = np.nan         # group 5 all NaN
    vals, lab = torch.as_tensor(vals_np).cuda(), torch.as_tensor(lab_np).cuda()
    outs = _raw_outs(ng, -77)
    c = _raw_summary_call(vals, lab, ng, outs, None)
    assert lib.fh_query_path(ctypes.byref(c)) == 1
    nscratch = lib.fh_scratch_bytes(ctypes.byref(c))
    assert nscratch > 0
    scratch = torch.empty(nscratch, dtype=torch.uint8, device="cuda")
    c = _raw_summary_call(vals, lab, ng, outs, scratch)
    assert lib.fh_grouped_reduce(ctypes.byref(c)) == 0
    torch.cuda.synchronize()
    assert c.path_used == 1
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    for g in range(ng):
        rows = vals_np[lab_np == g]
        ok = rows[~np.isnan(rows)]
        assert got["count"][g] == len(ok)
        assert got["nanflag"][g] == int(np.isnan(rows).any())
        assert got["present"][g] == int(len(rows) > 0)
        np.testing.assert_allclose(got["sum"][g], ok.sum(), rtol=1e-12, atol=1e-9)
        assert got["min"][g] == (ok.min() if len(ok) else np.inf)
        assert got["max"][g] == (ok.max() if len(ok) else -np.inf)
        ssd = ((ok - ok.mean()) ** 2).sum() if len(ok) else 0.0
        np.testing.assert_allclose(got["ssd"][g], ssd, rtol=1e-12, atol=1e-9)
    # no finish mode applies to the set
    c.finish, c.result_dtype, c.result = _ffi.FINISH_MEAN, _ffi.F64, outs["sum"].data_ptr()
    assert lib.fh_grouped_reduce(ctypes.byref(c)) == 14


def test_raw_abi_refuses_summary_off_the_lds_path():
    lib = _ffi.load_library()
    ng = _max_summary_groups("float64") + 1
    n = 1000
    vals = torch.ones(n, dtype=torch.float64, device="cuda")
    lab = torch.zeros(n, dtype=torch.int64, device="cuda")
    outs = _raw_outs(ng, -77)
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    c = _raw_summary_call(vals, lab, ng, outs, scratch)
    assert lib.fh_query_path(ctypes.byref(c)) == 0
    assert lib.fh_grouped_reduce(ctypes.byref(c)) == 15
    assert b"LDS-binned path only" in lib.fh_error_string(15)
    outs7 = _raw_outs(7, -77)
    c = _raw_summary_call(vals, lab, 7, outs7, scratch)
    c.flags |= _ffi.FLAG_FORCE_ATOMIC
    assert lib.fh_grouped_reduce(ctypes.byref(c)) == 15
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its marker
    for k in outs:
        assert bool((outs[k] == -77).all()) and bool((outs7[k] == -77).all()), k
    # the engine layer raises instead of falling back
    with pytest.raises(RuntimeError, match="floxhip error 15"):
        aggregate_hip.grouped_partials(_ffi.SET_SUMMARY, vals, lab, ng, skipnan=True)
