"""Label-code cache on the device: every reduction is called three times on
the same tensors (first sight / emit / hit), every result is compared with
the oracle in the tolerance classes of tests/test_hip_parity.py, and
label_cache_stats() must show that the third call really was a hit."""

import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi
from oracle import groupby_reduce as oracle_reduce
from tests.test_hip_parity import _tol

pytestmark = pytest.mark.gpu

ARG_LIKE = ("argmax", "argmin", "first", "last", "any")
TWO_PASS = ("var", "argmax")  # two kernel passes over the same labels per call
FUNCS = ["sum", "nansum", "mean", "nanmean", "count", "min", "nanmax", "prod",
         "var", "argmax", "first", "any"]
VDTYPES = ["float32", "float64", "int32", "int64"]

# one grid-stride iteration of the u16 kernel: 2 resident blocks on each of
# 256 CUs x 1024 lanes x 8 rows = 4 194 304 rows; this size runs a second
# iteration and a 5-row tail
N_PAST_GRID = 5_200_005


def _values(rng, n, dtype, func):
    if func == "any":
        return rng.random(n) < 0.02
    if func == "prod":
        v = rng.choice(np.array([-1, 1, 2]), n).astype(dtype)
    elif np.dtype(dtype).kind == "f":
        v = (rng.standard_normal(n) * 100).astype(dtype)
    else:
        v = rng.integers(-1000, 1000, n).astype(dtype)
    if np.dtype(dtype).kind == "f" and n:
        v[rng.random(n) < 0.03] = np.nan
    return v


def _labels(rng, n, ng, ldtype="int64", bad=True):
    lab = rng.integers(0, ng, n).astype(ldtype)
    if bad and n:
        k = rng.random(n)
        lab[k < 0.02] = -1
        lab[(k >= 0.02) & (k < 0.04)] = ng
        lab[(k >= 0.04) & (k < 0.05)] = ng + 70_000  # past the u16 range too
    return lab


def _check(got, want, func):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    tol = dict(rtol=0, atol=0) if func in ARG_LIKE else _tol(func, want.dtype)
    np.testing.assert_allclose(got, want, equal_nan=True, err_msg=func, **tol)


def _delta(a, b):
    return {k: b[k] - a[k] for k in ("hits", "emits", "misses")}


def _three_calls(vals_t, by_ts, func, expected, want, cached=True):
    """the protocol: three calls, each checked; the third must be served
    from the cache (or, cached=False, none may be)"""
    flox_amd.clear_label_cache()
    passes = 2 if func in TWO_PASS else 1
    s = [flox_amd.label_cache_stats()]
    for _ in range(3):
        got, *_g = flox_amd.groupby_reduce(vals_t, *by_ts, func=func, expected_groups=expected)
        _check(got, want, func)
        s.append(flox_amd.label_cache_stats())
    total, third = _delta(s[0], s[3]), _delta(s[2], s[3])
    if not cached:
        assert total == {"hits": 0, "emits": 0, "misses": 0}, total
        return
    assert third == {"hits": passes, "emits": 0, "misses": 0}, (third, total)
    assert total["misses"] == 1 and total["emits"] == 1, total
    assert s[3]["bytes"] == 2 * by_ts[0].numel()


def _run(n, ng, func, vdtype, ldtype="int64", seed=None, bad=True, cached=True):
    rng = np.random.default_rng(zlib.crc32(f"{n}-{ng}-{func}-{vdtype}-{ldtype}-{seed}".encode()))
    vals = _values(rng, n, vdtype, func)
    lab = _labels(rng, n, ng, ldtype, bad)
    want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(ng))
    _three_calls(torch.as_tensor(vals).cuda(), (torch.as_tensor(lab).cuda(),),
                 func, np.arange(ng), want, cached=cached)


@pytest.mark.parametrize("ldtype", ["int64", "int32"])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("func", FUNCS)
def test_funcs_and_dtypes(func, vdtype, ldtype):
    # NaNs in float values, negative and >= ngroups labels; 8*1024+1 rows is
    # past one vector iteration of a block and leaves a tail
    _run(8 * 1024 + 1, 257, func, vdtype, ldtype)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 8 * 1024 - 1, 8 * 1024, 8 * 1024 + 1])
@pytest.mark.parametrize("func,vdtype", [("mean", "float32"), ("nansum", "float64"),
                                         ("first", "int32"), ("argmax", "int64")])
def test_row_counts(n, func, vdtype):
    if n == 0:
        # no rows: nothing to cache, results are the empty-group fills
        _run(0, 255, func, vdtype, cached=False)
    else:
        _run(n, 255, func, vdtype)


@functools.lru_cache(maxsize=None)
def _big():
    """one shared data set past a full grid-stride iteration (read-only)"""
    rng = np.random.default_rng(99)
    n = N_PAST_GRID
    vals = (rng.standard_normal(n) * 100).astype("float32")
    vals[::97] = np.nan
    lab = _labels(rng, n, 255)
    return vals, lab, torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()


@pytest.mark.parametrize("func", ["nanmean", "first"])
def test_past_one_grid_stride_iteration(func):
    vals, lab, vals_t, lab_t = _big()
    want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(255))
    _three_calls(vals_t, (lab_t,), func, np.arange(255), want)


def test_offset_view_values():
    # values that start 4 bytes into an allocation (vals_big[1:])
    vals, lab, vals_t, lab_t = _big()
    n = 100_001
    want, *_ = oracle_reduce(vals[1:n + 1], lab[:n], func="nanmean", expected_groups=np.arange(255))
    by = lab_t[:n].clone()
    _three_calls(vals_t[1:n + 1], (by,), "nanmean", np.arange(255), want)
    # and labels that are themselves an offset view
    want, *_ = oracle_reduce(vals[:n], lab[3:n + 3], func="nanmean", expected_groups=np.arange(255))
    _three_calls(vals_t[:n], (lab_t[3:n + 3],), "nanmean", np.arange(255), want)


def _max_lds_groups(op_set, vdtype):
    """largest group count whose bins still fit LDS for the op set"""
    lib = _ffi.load_library()
    c = _ffi.FhCall()
    c.op_set, c.vdtype = op_set, vdtype

    def lds(ng):
        c.ngroups = ng
        return lib.fh_query_path(ctypes.byref(c)) == 1

    lo, hi = 1, 1 << 17
    assert lds(lo) and not lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lds(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("ng", [1, 2, 255, 256, 257])
def test_small_group_counts(ng):
    _run(20_001, ng, "mean", "float32")


@pytest.mark.parametrize("func,op_set,vdtype,ffi_dt", [
    ("mean", _ffi.SET_SUM_COUNT, "float32", _ffi.F32),
    ("count", _ffi.SET_COUNT, "float64", _ffi.F64),
    ("min", _ffi.SET_MIN_FULL, "int64", _ffi.I64),
])
def test_largest_lds_group_count_and_one_more(func, op_set, vdtype, ffi_dt):
    ng = _max_lds_groups(op_set, ffi_dt)
    assert ng < 0xFFFF  # the u16 sentinel stays out of range
    _run(100_003, ng, func, vdtype)
    # one more group: the bins leave LDS, the call runs uncached, still right
    _run(100_003, ng + 1, func, vdtype, cached=False)


def test_every_row_out_of_range():
    rng = np.random.default_rng(5)
    n, ng = 10_007, 300
    vals = _values(rng, n, "float32", "mean")
    lab = np.where(rng.random(n) < 0.5, -1, ng + rng.integers(0, 1 << 20, n)).astype("int64")
    for func in ("mean", "sum", "count", "first"):
        want, *_ = oracle_reduce(vals, lab, func=func, expected_groups=np.arange(ng))
        _three_calls(torch.as_tensor(vals).cuda(), (torch.as_tensor(lab).cuda(),),
                     func, np.arange(ng), want)


@pytest.mark.parametrize("func,vdtype,ldtype", [
    ("nanmean", "float64", "int64"), ("sum", "float32", "int32"),
    ("var", "float64", "int64"), ("first", "int32", "int64"),
])
def test_two_by(func, vdtype, ldtype):
    rng = np.random.default_rng(zlib.crc32(f"2by-{func}".encode()))
    n = 100_003
    vals = _values(rng, n, vdtype, func)
    a = rng.integers(0, 12, n).astype(ldtype)
    b = rng.integers(0, 180, n).astype(ldtype)
    k = rng.random(n)
    a[k < 0.01] = -1
    a[(k >= 0.01) & (k < 0.02)] = 12       # out of range in the first key only
    b[(k >= 0.02) & (k < 0.03)] = 180      # ... in the second key only
    b[(k >= 0.03) & (k < 0.04)] = -5
    a[(k >= 0.04) & (k < 0.05)] = 13       # ... in both
    b[(k >= 0.04) & (k < 0.05)] = 70_000
    expected = (np.arange(12), np.arange(180))
    want, *_ = oracle_reduce(vals, a, b, func=func, expected_groups=expected)
    assert want.shape == (12, 180)
    _three_calls(torch.as_tensor(vals).cuda(),
                 (torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()),
                 func, expected, want)


def test_inplace_write_invalidates():
    rng = np.random.default_rng(21)
    n, ng = 50_001, 100
    vals = _values(rng, n, "float32", "mean")
    lab = _labels(rng, n, ng)
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    want, *_ = oracle_reduce(vals, lab, func="sum", expected_groups=np.arange(ng))
    _three_calls(vals_t, (lab_t,), "sum", np.arange(ng), want)
    new0 = (int(lab[0]) + 1) % ng if 0 <= lab[0] < ng else 0
    lab[0] = new0
    lab_t[0] = new0
    want, *_ = oracle_reduce(vals, lab, func="sum", expected_groups=np.arange(ng))
    s0 = flox_amd.label_cache_stats()
    got, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="sum", expected_groups=np.arange(ng))
    _check(got, want, "sum")
    assert _delta(s0, flox_amd.label_cache_stats()) == {"hits": 0, "emits": 0, "misses": 1}
    # count is exact: the moved row shows in both groups
    wantc, *_ = oracle_reduce(vals, lab, func="count", expected_groups=np.arange(ng))
    for _ in range(2):  # emit, then hit on the NEW labels
        got, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="count", expected_groups=np.arange(ng))
        _check(got, wantc, "count")
    assert _delta(s0, flox_amd.label_cache_stats()) == {"hits": 1, "emits": 1, "misses": 1}


def test_free_and_reallocate_is_a_miss():
    rng = np.random.default_rng(22)
    n, ng = 50_001, 100
    vals = _values(rng, n, "float64", "mean")
    vals_t = torch.as_tensor(vals).cuda()
    lab = _labels(rng, n, ng)
    lab_t = torch.as_tensor(lab).cuda()
    want, *_ = oracle_reduce(vals, lab, func="mean", expected_groups=np.arange(ng))
    _three_calls(vals_t, (lab_t,), "mean", np.arange(ng), want)
    ptr = lab_t.data_ptr()
    del lab_t
    assert flox_amd.label_cache_stats()["bytes"] == 0  # dropped with the tensor
    lab2 = _labels(rng, n, ng)
    lab2_t = torch.as_tensor(lab2).cuda()  # equal size: the allocator reuses the block
    reused = lab2_t.data_ptr() == ptr
    want2, *_ = oracle_reduce(vals, lab2, func="mean", expected_groups=np.arange(ng))
    s0 = flox_amd.label_cache_stats()
    got, *_ = flox_amd.groupby_reduce(vals_t, lab2_t, func="mean", expected_groups=np.arange(ng))
    _check(got, want2, "mean")
    assert _delta(s0, flox_amd.label_cache_stats()) == {"hits": 0, "emits": 0, "misses": 1}, reused


def test_inference_mode_labels_run_uncached():
    # tensors made under inference_mode have no version counter: they must
    # work as before the cache existed, and never be cached
    rng = np.random.default_rng(25)
    n, ng = 30_001, 300
    vals = _values(rng, n, "float32", "mean")
    lab = _labels(rng, n, ng)
    want, *_ = oracle_reduce(vals, lab, func="mean", expected_groups=np.arange(ng))
    with torch.inference_mode():
        vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
        assert lab_t.is_inference()
        _three_calls(vals_t, (lab_t,), "mean", np.arange(ng), want, cached=False)
    _three_calls(vals_t, (lab_t,), "mean", np.arange(ng), want, cached=False)


def test_storage_swap_invalidates():
    # by.data = other changes neither the object nor its _version
    rng = np.random.default_rng(26)
    n, ng = 30_001, 300
    vals = _values(rng, n, "float64", "mean")
    lab, other = _labels(rng, n, ng), _labels(rng, n, ng)
    vals_t = torch.as_tensor(vals).cuda()
    lab_t, other_t = torch.as_tensor(lab).cuda(), torch.as_tensor(other).cuda()
    want, *_ = oracle_reduce(vals, lab, func="count", expected_groups=np.arange(ng))
    _three_calls(vals_t, (lab_t,), "count", np.arange(ng), want)
    lab_t.data = other_t
    want2, *_ = oracle_reduce(vals, other, func="count", expected_groups=np.arange(ng))
    s0 = flox_amd.label_cache_stats()
    got, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="count", expected_groups=np.arange(ng))
    _check(got, want2, "count")
    assert _delta(s0, flox_amd.label_cache_stats()) == {"hits": 0, "emits": 0, "misses": 1}


def test_capture_bypasses_the_cache():
    rng = np.random.default_rng(23)
    n, ng = 200_003, 1000
    vals = _values(rng, n, "float32", "mean")
    lab, new = _labels(rng, n, ng), _labels(rng, n, ng)
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    new_t = torch.as_tensor(new).cuda()
    want, *_ = oracle_reduce(vals, lab, func="mean", expected_groups=np.arange(ng))
    _three_calls(vals_t, (lab_t,), "mean", range(ng), want)  # warm: codes are held

    def step():
        return flox_amd.groupby_reduce(vals_t, lab_t, func="mean", expected_groups=range(ng))

    torch.cuda.synchronize()
    s0 = flox_amd.label_cache_stats()
    g = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    with torch.cuda.stream(cap):
        with torch.cuda.graph(g):
            res = step()
    assert flox_amd.label_cache_stats() == s0  # neither read nor written
    lab_t.copy_(new_t)
    g.replay()
    torch.cuda.synchronize()
    want_new, *_ = oracle_reduce(vals, new, func="mean", expected_groups=np.arange(ng))
    _check(res[0], want_new, "mean")


def test_option_off_never_hits():
    with flox_amd.set_options(label_cache=False):
        _run(30_001, 300, "mean", "float32", cached=False)
        _run(30_001, 300, "var", "float64", cached=False)


def test_second_stream_consumes_codes_emitted_on_the_first():
    rng = np.random.default_rng(24)
    n, ng = 1_000_003, 500
    vals = _values(rng, n, "float32", "mean")
    lab = _labels(rng, n, ng)
    want, *_ = oracle_reduce(vals, lab, func="nanmean", expected_groups=np.arange(ng))
    vals_t, lab_t = torch.as_tensor(vals).cuda(), torch.as_tensor(lab).cuda()
    flox_amd.clear_label_cache()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s0 = flox_amd.label_cache_stats()
    with torch.cuda.stream(s1):
        for _ in range(2):  # first sight, then the emitting call
            r1, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="nanmean", expected_groups=range(ng))
    with torch.cuda.stream(s2):  # no host sync in between
        r2, *_ = flox_amd.groupby_reduce(vals_t, lab_t, func="nanmean", expected_groups=range(ng))
    torch.cuda.synchronize()
    assert _delta(s0, flox_amd.label_cache_stats()) == {"hits": 1, "emits": 1, "misses": 1}
    _check(r1, want, "nanmean")
    _check(r2, want, "nanmean")
