"""The order-dependent functions over leading dims on the column path: the
column forms of SET_IDXMIN / SET_IDXMAX and the single-pass SET_ARGMIN_COLS /
SET_ARGMAX_COLS. Raw partials against numpy in the three flush modes, the ABI
corners, the eight API functions against the oracle and against the lead fold
(set_options(cols_order_funcs=False)) bit for bit, groupby_reduce_many,
capture, the fallbacks, and the 2**31-element array the fold refuses."""

import ctypes
import zlib

import numpy as np
import pytest
import torch

import flox_amd
from flox_amd import _ffi, aggregate_hip
from oracle import groupby_reduce as oracle_reduce
from tests.test_reduce_many_cols_gpu import _sets, _spy_cols
from tests.test_reduce_many_gpu import FFI_DT, _np, _spy

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "int32", "int64"]
I64_MAX = np.iinfo(np.int64).max
SETS = {
    "idxmin": _ffi.SET_IDXMIN, "idxmax": _ffi.SET_IDXMAX,
    "argmin": _ffi.SET_ARGMIN_COLS, "argmax": _ffi.SET_ARGMAX_COLS,
}
ARG_FUNCS = ("argmax", "argmin", "nanargmax", "nanargmin")
FL_FUNCS = ("first", "last", "nanfirst", "nanlast")
SET_OF_FUNC = {
    "argmax": _ffi.SET_ARGMAX_COLS, "nanargmax": _ffi.SET_ARGMAX_COLS,
    "argmin": _ffi.SET_ARGMIN_COLS, "nanargmin": _ffi.SET_ARGMIN_COLS,
    "first": _ffi.SET_IDXMIN, "nanfirst": _ffi.SET_IDXMIN,
    "last": _ffi.SET_IDXMAX, "nanlast": _ffi.SET_IDXMAX,
}
NG = 9


# ---- inputs and the numpy reference -------------------------------------------------

def _pool(dtype):
    """about five distinct values, so ties are everywhere: +-0.0 and +-inf for
    floats, the dtype's own extremes (the running extremum's identities) for
    ints"""
    if np.dtype(dtype).kind == "f":
        return np.array([-np.inf, -2.5, -0.0, 0.0, 1.5, np.inf], dtype=dtype)
    ii = np.iinfo(dtype)
    return np.array([ii.min, -1, 0, 3, ii.max], dtype=dtype)


def _tied_values(rng, n_t, ldm, dtype, nan=0.1):
    v = rng.choice(_pool(dtype), size=(n_t, ldm))
    if np.dtype(dtype).kind == "f" and nan:
        v[rng.random((n_t, ldm)) < nan] = np.nan
    return v


def _codes(rng, n_t, ng):
    """labels in [1, ng - 1): groups 0 and ng - 1 stay empty; some rows in no group"""
    lab = rng.integers(1, max(ng - 1, 2), n_t)
    lab[rng.random(n_t) < 0.05] = -1
    return lab


def _plant_nans(v, codes):
    """group 1 starts with a NaN row, group 2 has one later, group 3 is all NaN"""
    if v.dtype.kind != "f":
        return
    r1, r2 = np.flatnonzero(codes == 1), np.flatnonzero(codes == 2)
    if len(r1):
        v[r1[0], :] = np.nan
    if len(r2) > 2:
        v[r2[2], :] = np.nan
    v[codes == 3, :] = np.nan


def _np_order(v, codes, ng, skipnan, row_offset=0):
    """numpy reference of the four sets' members, each (ng, m); np.argmax /
    np.argmin give the tie and NaN rules of the non-skipping arg sets"""
    n_t, m = v.shape
    isf = v.dtype.kind == "f"
    out = {k: {"idx": np.full((ng, m), -1 if k == "idxmax" else I64_MAX, np.int64)} for k in SETS}
    count = np.zeros((ng, m), np.int64)
    present = np.zeros((ng, m), np.int32)
    nanflag = np.zeros((ng, m), np.int32)
    order = np.argsort(codes, kind="stable")
    sc = codes[order]
    lo = np.searchsorted(sc, np.arange(ng), "left")
    hi = np.searchsorted(sc, np.arange(ng), "right")
    for g in np.flatnonzero(hi > lo):
        r = order[lo[g]:hi[g]]  # ascending rows of the group
        sub = v[r]
        isn = np.isnan(sub) if isf else np.zeros(sub.shape, bool)
        ok = ~isn
        count[g] = ok.sum(0)
        present[g] = 1
        nanflag[g] = isn.any(0)
        cand = ok if skipnan else np.ones_like(ok)
        has = cand.any(0)
        rows = r + row_offset
        out["idxmin"]["idx"][g] = np.where(has, rows[np.argmax(cand, 0)], I64_MAX)
        out["idxmax"]["idx"][g] = np.where(has, rows[len(r) - 1 - np.argmax(cand[::-1], 0)], -1)
        for name, arg, ext, worst in (("argmax", np.argmax, np.max, -np.inf),
                                      ("argmin", np.argmin, np.min, np.inf)):
            if skipnan and isf:
                e = ext(np.where(isn, worst, sub), 0)
                at = np.argmax(ok & (sub == e[None, :]), 0)
                out[name]["idx"][g] = np.where(ok.any(0), rows[at], I64_MAX)
            else:
                out[name]["idx"][g] = rows[arg(sub, 0)]
    for k in SETS:
        out[k].update(count=count, present=present)
    for k in ("argmin", "argmax"):
        out[k]["nanflag"] = nanflag
    return out


def _chunk_bounds(sc_np, parts=8):
    """group-aligned row chunks, as grouped_partials_cols plans them"""
    n_t = len(sc_np)
    seg = np.flatnonzero(np.diff(sc_np)) + 1
    target = max(1, -(-n_t // parts))
    bounds = [0]
    for b in seg:
        if b - bounds[-1] >= target:
            bounds.append(int(b))
    bounds.append(n_t)
    return bounds


def _raw(op_set, vt, sc, perm, ng, skipnan, mode, row_offset=0, target=None):
    """fh_grouped_reduce_cols through the raw ABI. mode: "chunks" (group-aligned
    chunk_offsets), "slab" (chunk_offsets NULL: the launcher splits the rows
    and k_combine merges) or "single" (one chunk). Returns (rc, outs)."""
    lib = _ffi.load_library()
    m = vt.shape[1]
    outs = {
        "idx": torch.full((ng, m), -77, dtype=torch.int64, device="cuda"),
        "count": torch.full((ng, m), -77, dtype=torch.int64, device="cuda"),
        "present": torch.full((ng, m), -77, dtype=torch.int32, device="cuda"),
        "nanflag": torch.full((ng, m), -77, dtype=torch.int32, device="cuda"),
    }
    c = _ffi.FhCall()
    c.op_set, c.vdtype, c.ldtype = op_set, FFI_DT[str(vt.dtype)[6:]], _ffi.L_I32
    c.flags = _ffi.FLAG_SKIPNAN if skipnan else 0
    c.n, c.m, c.ldm, c.ngroups = vt.shape[0], m, vt.stride(0), ng
    c.values, c.labels, c.perm = vt.data_ptr(), sc.data_ptr(), perm.data_ptr()
    c.out_sum, c.out_count = outs["idx"].data_ptr(), outs["count"].data_ptr()
    c.out_present, c.out_nanflag = outs["present"].data_ptr(), outs["nanflag"].data_ptr()
    c.row_offset = row_offset
    if target is not None:
        c.target = target.data_ptr()
    keep = []
    if mode != "slab":
        bounds = _chunk_bounds(sc.cpu().numpy()) if mode == "chunks" else [0, vt.shape[0]]
        offs = torch.tensor(bounds, dtype=torch.int64, device="cuda")
        keep.append(offs)
        c.chunk_offsets, c.nchunks = offs.data_ptr(), len(bounds) - 1
    nscratch = lib.fh_scratch_bytes(ctypes.byref(c))
    assert nscratch >= 0
    if nscratch:
        assert mode == "slab"
        scratch = torch.empty(nscratch, dtype=torch.uint8, device="cuda")
        keep.append(scratch)
        c.scratch, c.scratch_bytes = scratch.data_ptr(), nscratch
    c.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.fh_grouped_reduce_cols(ctypes.byref(c))
    torch.cuda.synchronize()
    if rc == 0:
        assert c.path_used == 3
    return rc, outs


def _device_case(v, m, offset=0):
    """v (n_t, ldm) on the device `offset` elements into its allocation; the
    (n_t, m) view of its first m columns"""
    n_t, ldm = v.shape
    flat = torch.empty(n_t * ldm + offset, dtype=getattr(torch, str(v.dtype)), device="cuda")
    base = flat[offset:].view(n_t, ldm)
    base.copy_(torch.as_tensor(v))
    return base[:, :m]


def _check_raw(vt, v_np, codes, ng, sets=tuple(SETS), modes=("chunks", "slab", "single"),
               perm_np=None, row_offset=0):
    """every set, skipping and not, in every mode, against numpy: exact"""
    codes_t = torch.as_tensor(codes).cuda()
    if perm_np is None:
        sc, perm = torch.sort(codes_t, stable=True)
    else:
        perm = torch.as_tensor(perm_np).cuda()
        sc = codes_t[perm]
    sc, perm = sc.to(torch.int32).contiguous(), perm.to(torch.int32).contiguous()
    for skipnan in (False, True):
        want = _np_order(v_np, codes, ng, skipnan, row_offset)
        for name in sets:
            for mode in modes:
                rc, got = _raw(SETS[name], vt, sc, perm, ng, skipnan, mode, row_offset)
                assert rc == 0, (name, mode, rc)
                for k, w in want[name].items():
                    np.testing.assert_array_equal(
                        _np(got[k]), w, err_msg=f"{name} skipnan={skipnan} {mode}: {k}")


def _case(n_t, m, dtype, ldm=None, offset=0, ng=NG, seed=""):
    rng = np.random.default_rng(zlib.crc32(f"order-{n_t}-{m}-{dtype}-{ldm}-{offset}-{seed}".encode()))
    v = _tied_values(rng, n_t, m if ldm is None else ldm, dtype)
    codes = _codes(rng, n_t, ng)
    _plant_nans(v, codes)
    return _device_case(v, m, offset), v[:, :m], codes


# ---- raw partials against numpy -------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 3, 4, 1023, 1024, 1025])
@pytest.mark.parametrize("n_t", [1, 2047, 2048, 2049, 4097])
def test_raw_partials_rows_and_columns(n_t, m, dtype):
    # n_t around COLS_TTILE; 4097 rows in slab mode: chunks that cut segments,
    # a segment across a staged tile; n_t = 1: more groups than rows
    vt, v_np, codes = _case(n_t, m, dtype)
    _check_raw(vt, v_np, codes, NG)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,ldm,offset", [
    (10, 16, 0),   # ldm a multiple of every vector width, partial lanes
    (10, 13, 0),   # ldm no multiple of any: one column per thread
    (16, 24, 0),   # f32/i32: 16-B rows but not 32-B ones
    (12, None, 1),  # base pointer off 16-B alignment: one column per thread
])
def test_raw_partials_strides_and_alignment(m, ldm, offset, dtype):
    vt, v_np, codes = _case(4097, m, dtype, ldm, offset)
    if offset:
        assert vt.data_ptr() % 16 != 0
    _check_raw(vt, v_np, codes, NG)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_long_group_and_row_offset(dtype):
    # one group of 3000 rows among 4097: a segment longer than a staged tile
    vt, v_np, _ = _case(4097, 12, dtype, seed="long")
    codes = np.full(4097, 2)
    codes[np.random.default_rng(5).permutation(4097)[:3000]] = 1
    _check_raw(vt, v_np, codes, 4, row_offset=1_000_000_007)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32"])
def test_any_sorting_perm_gives_the_same_rows(dtype):
    # a perm that sorts the codes but walks each group's rows backwards: ties
    # must still go to the smallest row, the first NaN must still win
    vt, v_np, codes = _case(4097, 12, dtype, seed="rev")
    perm_rev = np.lexsort((-np.arange(len(codes)), codes))
    assert (np.diff(codes[perm_rev]) >= 0).all()
    _check_raw(vt, v_np, codes, NG, perm_np=perm_rev)


def test_signed_zeros_tie():
    # -0.0 and +0.0 are equal values: the smaller row wins whichever comes first
    v = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, -0.0]], dtype=np.float32)
    codes = np.zeros(3, dtype=np.int64)
    vt = torch.as_tensor(v).cuda()
    _check_raw(vt, v, codes, 1, sets=("argmin", "argmax"))
    sc = torch.zeros(3, dtype=torch.int32, device="cuda")
    perm = torch.arange(3, dtype=torch.int32, device="cuda")
    for name in ("argmin", "argmax"):
        _, got = _raw(SETS[name], vt, sc, perm, 1, False, "single")
        assert _np(got["idx"]).tolist() == [[0, 0]]


def test_no_group_count_cap():
    n_t, ng, m = 60_000, 50_000, 4
    rng = np.random.default_rng(17)
    v = _tied_values(rng, n_t, m, "float32")
    codes = rng.integers(0, ng, n_t)
    _check_raw(torch.as_tensor(v).cuda(), v, codes, ng)


# ---- ABI ---------------------------------------------------------------------------------

def test_abi_supports_and_refusals():
    lib = _ffi.load_library()
    assert lib.fh_abi_revision() == 6
    for s in list(SETS.values()) + [_ffi.SET_SUMMARY]:
        assert lib.fh_cols_supports(s) == 1 and _ffi.cols_supports(s)
    assert lib.fh_cols_supports(_ffi.SET_ARGMIN_PAIR) == 0
    assert lib.fh_cols_supports(99) == 0
    assert (_ffi.SET_ARGMIN_COLS, _ffi.SET_ARGMAX_COLS) == (15, 16)

    vt, v_np, codes = _case(301, 4, "float64")
    sc, perm = torch.sort(torch.as_tensor(codes).cuda(), stable=True)
    sc, perm = sc.to(torch.int32), perm.to(torch.int32)
    # a target on the column path stays refused, and nothing is written
    target = torch.zeros((NG, 4), dtype=torch.float64, device="cuda")
    for s in (_ffi.SET_IDXMIN, _ffi.SET_IDXMAX, _ffi.SET_ARGMAX_COLS):
        rc, outs = _raw(s, vt, sc, perm, NG, False, "single", target=target)
        assert rc != 0
        assert bool((outs["idx"] == -77).all())
    # the 1-D entry point refuses the column-only sets without launching
    vals = vt[:, 0].contiguous()
    lab = torch.as_tensor(codes).cuda()
    out = torch.full((NG,), -77, dtype=torch.int64, device="cuda")
    for s in (_ffi.SET_ARGMIN_COLS, _ffi.SET_ARGMAX_COLS):
        c = _ffi.FhCall()
        c.op_set, c.vdtype, c.ldtype = s, _ffi.F64, _ffi.L_I64
        c.n, c.ngroups = vals.numel(), NG
        c.values, c.labels = vals.data_ptr(), lab.data_ptr()
        c.out_sum = c.out_count = out.data_ptr()
        c.stream = torch.cuda.current_stream().cuda_stream
        assert lib.fh_grouped_reduce(ctypes.byref(c)) == 18
    torch.cuda.synchronize()
    assert bool((out == -77).all())
    assert b"column path only" in lib.fh_error_string(18)
    with pytest.raises(RuntimeError, match="floxhip error 18"):
        aggregate_hip.grouped_partials(_ffi.SET_ARGMAX_COLS, vals, lab, NG)


# ---- API parity ----------------------------------------------------------------------------

def _api_case(dtype, n_t=803, m=6, ng=NG):
    """time-major (n_t, m) values with ties and the planted NaN groups; labels
    leave groups 0 and ng - 1 empty"""
    rng = np.random.default_rng(zlib.crc32(f"api-{dtype}-{n_t}-{m}".encode()))
    v = _tied_values(rng, n_t, m, dtype)
    lab = _codes(rng, n_t, ng)
    _plant_nans(v, lab)
    return v, lab


def _same_bits(a, b, msg):
    a, b = _np(a), _np(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), msg


def _check_api(arr, arr_np, bys, func, vt=None, oracle=True, **kw):
    """groupby_reduce(arr, ...) on the column path against the oracle (exact)
    and against the same call through the lead fold (bit for bit); exactly one
    column call, of the func's set, on the caller's storage when vt is given"""
    as_numpy = not isinstance(arr, torch.Tensor)
    bin_ = bys if as_numpy else tuple(torch.as_tensor(b).cuda() for b in bys)
    with _spy_cols() as seen:
        got, *groups = flox_amd.groupby_reduce(arr, *bin_, func=func, **kw)
    assert _sets(seen) == [SET_OF_FUNC[func]], (func, seen)
    if vt is not None:
        assert seen[0][1:] == (vt.data_ptr(), vt.stride(0))  # zero copy
    with flox_amd.set_options(cols_order_funcs=False), _spy_cols() as seen_off:
        off, *goff = flox_amd.groupby_reduce(arr, *bin_, func=func, **kw)
    assert seen_off == []
    assert type(got) is type(off)
    _same_bits(got, off, f"{func} vs the fold")
    for a, b in zip(groups, goff):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    if not oracle:
        return got
    want, *wg = oracle_reduce(arr_np, *bys, func=func, **kw)
    g = _np(got)
    assert g.shape == want.shape, (func, g.shape, want.shape)
    np.testing.assert_array_equal(g, want, err_msg=f"{func} vs oracle")
    for a, b, c in zip(groups, goff, wg):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("func", ARG_FUNCS + FL_FUNCS)
def test_api_parity(func, dtype):
    v, lab = _api_case(dtype)
    vt = torch.as_tensor(v).cuda()
    kw = dict(expected_groups=np.arange(NG))
    got = _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, **kw)
    assert isinstance(got, torch.Tensor) and got.shape == (6, NG)
    got_np = _check_api(np.ascontiguousarray(v.T), v.T, (lab,), func, **kw)
    assert isinstance(got_np, np.ndarray)


CORNER_FUNCS = ("argmin", "nanargmax", "first", "nanlast")


@pytest.mark.parametrize("dtype", ["float64", "int32"])
@pytest.mark.parametrize("func", CORNER_FUNCS)
@pytest.mark.parametrize("kw", [
    dict(fill_value=-7),
    dict(min_count=3, fill_value=-9),
    dict(min_count=1, fill_value=-5),  # nanarg*: all-NaN groups count 0 and fill
], ids=["fill", "min_count3", "min_count1"])
def test_api_fill_value_and_min_count(kw, func, dtype):
    v, lab = _api_case(dtype)
    lab[lab == 7] = 6
    lab[:2] = 7  # a group of two rows: below min_count=3
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (lab,), func, vt=vt, expected_groups=np.arange(NG), **kw)


@pytest.mark.parametrize("func", CORNER_FUNCS)
def test_api_sort_false(func):
    rng = np.random.default_rng(13)
    n_t, m = 1007, 5
    by = rng.choice([30, 5, 17, 2, 44, 9], n_t)
    v = _tied_values(rng, n_t, m, "float32")
    vt = torch.as_tensor(v).cuda()
    _check_api(vt.permute(1, 0), v.T, (by,), func, vt=vt, sort=False)


@pytest.mark.parametrize("func", CORNER_FUNCS)
def test_api_two_by(func):
    rng = np.random.default_rng(15)
    n_t, m = 2003, 6
    b0, b1 = rng.integers(-1, 5, n_t), rng.integers(-1, 8, n_t)
    v = _tied_values(rng, n_t, m, "float64")
    vt = torch.as_tensor(v).cuda()
    got = _check_api(vt.permute(1, 0), v.T, (b0, b1), func, vt=vt,
                     expected_groups=(np.arange(4), np.arange(7)))
    assert got.shape == (m, 4, 7)


@pytest.mark.parametrize("func", ("argmax", "first", "nanlast"))
@pytest.mark.parametrize("dtype", ["bool", "int8", "uint8", "int16"])
def test_api_bool_and_small_dtypes(dtype, func):
    rng = np.random.default_rng(16)
    n_t, m = 611, 5
    v = rng.integers(0, 2 if dtype == "bool" else 5, (m, n_t)).astype(dtype)
    lab = _codes(rng, n_t, NG)
    _check_api(v, v, (lab,), func, expected_groups=np.arange(NG))
    # a torch tensor of a small dtype comes back in torch's dtype, where the
    # empty-group fill is not numpy's: the fold is the reference there
    _check_api(torch.as_tensor(v).cuda(), v, (lab,), func, oracle=False,
               expected_groups=np.arange(NG))


def test_api_three_leading_dims():
    rng = np.random.default_rng(18)
    v = _tied_values(rng, 3 * 4, 50, "float32").reshape(3, 4, 50)
    lab = rng.integers(0, 4, 50)
    for func in ("nanargmin", "last"):
        got = _check_api(torch.as_tensor(v).cuda(), v, (lab,), func, expected_groups=np.arange(4))
        assert got.shape == (3, 4, 4)


# ---- groupby_reduce_many -----------------------------------------------------------------------

def _check_many(funcs):
    v, lab = _api_case("float64")
    arr, lt = torch.as_tensor(v).cuda().permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(expected_groups=np.arange(NG))
    with _spy_cols() as seen:
        res, _ = flox_amd.groupby_reduce_many(arr, lt, funcs=funcs, **kw)
    for f in funcs:
        single, _ = flox_amd.groupby_reduce(arr, lt, func=f, **kw)
        if f == "mean":
            np.testing.assert_allclose(_np(res[f]), _np(single), rtol=1e-12, equal_nan=True)
        else:
            _same_bits(res[f], single, f)
    return _sets(seen)


def test_many_shares_the_factorization_only():
    # mean and max share the summary pass; argmax and first keep their own
    sets = _check_many(("mean", "max", "argmax", "first"))
    assert sorted(sets) == sorted([_ffi.SET_SUMMARY, _ffi.SET_ARGMAX_COLS, _ffi.SET_IDXMIN]), sets


def test_many_mean_argmax_first():
    # one name of the fused family is not enough to share a pass (as before
    # this form existed): mean takes the pass it takes alone
    sets = _check_many(("mean", "argmax", "first"))
    assert sets.count(_ffi.SET_ARGMAX_COLS) == 1 and sets.count(_ffi.SET_IDXMIN) == 1, sets
    assert len(sets) == 3 and sets.count(_ffi.SET_SUMMARY) + sets.count(_ffi.SET_SUM_COUNT) == 1, sets


# ---- capture --------------------------------------------------------------------------------------

@pytest.mark.parametrize("func", ("nanargmax", "argmin", "first", "nanlast"))
def test_capture_replays_the_eager_result(func):
    # under capture no chunk planning may sync: the slab form runs
    v, lab = _api_case("float32", n_t=4101, m=12)
    vt = torch.as_tensor(v).cuda()
    arr, lt = vt.permute(1, 0), torch.as_tensor(lab).cuda()
    kw = dict(expected_groups=np.arange(NG))
    eager, _ = flox_amd.groupby_reduce(arr, lt, func=func, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g), _spy_cols() as seen:
            res, _ = flox_amd.groupby_reduce(arr, lt, func=func, **kw)
    assert _sets(seen) == [SET_OF_FUNC[func]]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _same_bits(res, eager, func)


# ---- fallbacks ---------------------------------------------------------------------------------------

def _both_ways(arr, by, **kw):
    with _spy_cols() as seen:
        on = flox_amd.groupby_reduce(arr, by, **kw)
    with flox_amd.set_options(cols_order_funcs=False):
        off = flox_amd.groupby_reduce(arr, by, **kw)
    return on, off, _sets(seen)


@pytest.mark.parametrize("func", ("argmax", "nanfirst", "last"))
def test_datetime_values_keep_the_fold(func):
    rng = np.random.default_rng(19)
    v = rng.integers(0, 5, (4, 300)).astype("datetime64[ns]")
    v[rng.random(v.shape) < 0.1] = np.datetime64("NaT")
    lab = rng.integers(0, 5, 300)
    on, off, sets = _both_ways(v, lab, func=func, expected_groups=np.arange(6))
    assert not set(sets) & set(SET_OF_FUNC.values())
    _same_bits(on[0], off[0], func)


@pytest.mark.parametrize("func", ("first", "nanlast"))
def test_axis_subset_keeps_the_fold(func):
    rng = np.random.default_rng(20)
    v = _tied_values(rng, 12, 50, "float64").reshape(3, 4, 50)
    by = rng.integers(0, 4, (4, 50))
    kw = dict(func=func, axis=(2,), expected_groups=np.arange(4), fill_value=-9.0)
    on, off, sets = _both_ways(torch.as_tensor(v).cuda(), torch.as_tensor(by).cuda(), **kw)
    assert not set(sets) & set(SET_OF_FUNC.values())
    assert on[0].shape == (3, 4, 4)
    _same_bits(on[0], off[0], func)


def test_arg_with_axis_subset_still_raises():
    v = torch.zeros((3, 4, 50), device="cuda")
    by = torch.zeros((4, 50), dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="axis subset"):
        flox_amd.groupby_reduce(v, by, func="argmax", axis=(2,), expected_groups=np.arange(2))


# ---- the size limit -----------------------------------------------------------------------------------

def test_two_to_the_31_elements():
    n_t, m, ng = 2**11, 2**20, 3
    torch.cuda.empty_cache()  # blocks cached by earlier tests are not "free"
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2**30:
        pytest.skip("needs 24 GiB of free device memory")
    gen = torch.Generator(device="cuda").manual_seed(3)
    vt = torch.empty((n_t, m), dtype=torch.float32, device="cuda")
    # few distinct values: ties in every column
    vt.copy_(torch.randint(0, 7, (n_t, m), generator=gen, device="cuda", dtype=torch.int8))
    assert vt.numel() == 2**31
    lab = torch.arange(n_t, device="cuda") % ng
    arr = vt.permute(1, 0)
    kw = dict(expected_groups=np.arange(ng))
    with _spy_cols() as seen, _spy() as seen1d:
        amax, _ = flox_amd.groupby_reduce(arr, lab, func="argmax", **kw)
        last, _ = flox_amd.groupby_reduce(arr, lab, func="last", **kw)
    assert _sets(seen) == [_ffi.SET_ARGMAX_COLS, _ffi.SET_IDXMAX] and seen1d == []
    assert all(s[1:] == (vt.data_ptr(), vt.stride(0)) for s in seen)
    assert amax.shape == last.shape == (m, ng)
    for g in range(ng):
        rows = torch.arange(g, n_t, ng, device="cuda")
        sub = vt[g::ng]  # the group's rows, ascending: a strided view
        # torch.argmax does not promise the first maximum: take the smallest
        # position among the rows equal to the column maximum instead
        pos = torch.arange(sub.shape[0], device="cuda", dtype=torch.int32)[:, None]
        first_max = torch.where(sub == sub.amax(0, keepdim=True), pos, sub.shape[0]).amin(0)
        assert torch.equal(amax[:, g], rows[first_max.long()])
        assert torch.equal(last[:, g], vt[rows[-1]])
        del first_max, pos
