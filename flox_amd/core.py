"""groupby_reduce: the flox-shaped top-level API on MI355X.

Mirrors the reference's eager path (flox/core.py:739-1222 groupby_reduce ->
_reduce_blockwise -> chunk_reduce -> _finalize_results) with the per-block
kernel layer replaced by fused HIP passes (aggregate_hip.grouped_partials)
and the dask combine tree replaced by RCCL all-reduces of the per-group
partial bins (distributed.py).

Scope: every reduction/scan the reference registers, over any mix of
leading array dims, axis subsets of ``by``'s dims, 1+ ``by`` arrays
(multi-dim groupby), isbin/IntervalIndex binning, sort=False
first-appearance ordering, expected_groups/fill_value/min_count/dtype
rules, custom Aggregation(chunk/combine/finalize) instances; dtypes
f32/f64/i32/i64/bool/datetime64/timedelta64 (NaT as int64-min, like the
reference) plus u8/u16/u32/u64/i8/i16/f16 via promote-compute-cast
following the reference's own promotion rules (see _SMALL_PROMOTE; uint64
computes on the int64 view). Grouping BY datetime labels works on the
int64 view (NaT rows drop; expected groups unit-align), including datetime
bin edges (isbin). Multi-GPU: every op combines across ranks (partial-bin
all-reduce / scan carries / quantile radix selection / mode run merge).
"""

from __future__ import annotations

import math
from collections import namedtuple
from typing import Any

import numpy as np
import torch

from . import _ffi, distributed, xrdtypes
from .aggregate_hip import _TORCH_VDTYPE, grouped_partials, grouped_partials_cols, summary_fits
from .aggregations import REDUCTIONS, Aggregation, CustomAggregation

# arg-reductions switch from the two-pass (extremum, then index-match) form to
# the packed-key single-pass form above this group count: the IDX bins cost
# 20 B/group in LDS, so past ~8e3 groups the second pass falls to the
# global-atomic path. Measured crossover (tools/arg_threshold_prof.py,
# 2e8 rows): two-pass wins to ~4e3 groups (0.94 vs 1.14 ms), packed wins
# from ~8e3 (1.09 vs 1.35; 2.6 vs 10.0 ms at 16e3). Tests lower this to
# exercise the packed form at small n.
PACKED_ARG_THRESHOLD = 6000
# options.fused_finalize: mean/sum/count finished inside the combine kernel
FUSED_FINALIZE = True
# options.fused_many: groupby_reduce_many serves these names from one
# SET_SUMMARY pass where the call is eligible (see _ManyCall)
FUSED_MANY = True
FUSED_MANY_FUNCS = frozenset((
    "count", "sum", "nansum", "mean", "nanmean", "var", "nanvar", "std",
    "nanstd", "min", "nanmin", "max", "nanmax",
))

# order-dependent reductions that run with leading array dims by folding the
# lead index into the group codes (see _fold_lead)
_QUANTILE_FUNCS = ("quantile", "nanquantile", "median", "nanmedian")
_ARG_FUNCS = ("argmax", "argmin", "nanargmax", "nanargmin")
_FIRST_LAST_FUNCS = ("first", "last", "nanfirst", "nanlast")
_VAR_FUNCS = ("var", "nanvar", "std", "nanstd")
_LEAD_FOLD_FUNCS = _QUANTILE_FUNCS + ("mode", "nanmode") + _ARG_FUNCS + _FIRST_LAST_FUNCS
# options.cols_order_funcs: the arg-reductions and first/last over leading
# dims take the column kernel's row-valued sets where the call is eligible
# (_cols_order_ok) instead of the lead fold
COLS_ORDER_FUNCS = True
_COLS_ORDER = _ARG_FUNCS + _FIRST_LAST_FUNCS
# options.cols_sorted_funcs: the quantile family and mode over leading dims
# sort each group's rows in LDS (fh_grouped_quantile_cols) where the call is
# eligible (_cols_sorted_ok) instead of the lead fold
COLS_SORTED_FUNCS = True
_COLS_SORTED = _QUANTILE_FUNCS + ("mode", "nanmode")
# options.cols_select_funcs: where a group is longer than the sort-in-LDS
# capacity, the quantile family takes the radix-select column kernel
# (fh_grouped_quantile_select_cols) instead of the lead fold. It extends the
# sorted form: cols_sorted_funcs=False turns both off.
COLS_SELECT_FUNCS = True
_COLS_SELECT = _QUANTILE_FUNCS
# options.cols_select_min_cols: the narrowest lead_M that takes it. The grid
# is column tiles x groups, so a narrow array with few long groups leaves
# most of the chip idle and the fold wins. Measured on MI355X at 2**26
# elements, nanmedian, 1 and 4 groups (profiles/r11_cols_select.md): f32 wins
# from 8192 columns with one group (3.35 vs 4.39 ms) and from 2048 with four;
# f64 loses at 8192 with one group (9.05 vs 7.97 ms) and wins from 16384
# (4.67 vs 8.07 ms). Never below one column tile of the kernel's plan (64).
COLS_SELECT_MIN_COLS = 16384

_TORCH_TO_NP = {
    torch.float32: np.dtype("float32"),
    torch.float64: np.dtype("float64"),
    torch.int64: np.dtype("int64"),
    torch.int32: np.dtype("int32"),
    torch.bool: np.dtype(bool),
}


def _np_dtype(t: torch.dtype) -> np.dtype:
    try:
        return _TORCH_TO_NP[t]
    except KeyError:
        raise NotImplementedError(
            f"engine='hip' does not support torch dtype {t} (numpy inputs "
            "of small/unsigned dtypes promote automatically)"
        ) from None


def _torch_dtype(d: np.dtype) -> torch.dtype:
    for k, v in _TORCH_TO_NP.items():
        if v == np.dtype(d):
            return k
    raise NotImplementedError(f"unsupported dtype {d}")


# small / unsigned / half value dtypes compute on a promoted dtype and cast
# back per the reference's own promotion rules (it casts BEFORE reducing:
# _initialize_aggregation + xrdtypes - u* sums land in uint64, i8/i16 in
# int64, min/max/first/last/mode preserve the input dtype, mean/var/std and
# the quantile family preserve a floating input dtype)
_SMALL_PROMOTE = {
    np.dtype("uint8"): np.dtype("int32"),
    np.dtype("uint16"): np.dtype("int32"),
    np.dtype("int8"): np.dtype("int32"),
    np.dtype("int16"): np.dtype("int32"),
    np.dtype("uint32"): np.dtype("int64"),
    np.dtype("float16"): np.dtype("float32"),
}
# the small dtypes torch itself has: tensor inputs promote through this table
# and dtype-preserving tensor results cast back through its inverse
_TORCH_SMALL = {
    torch.uint8: np.dtype("uint8"), torch.int8: np.dtype("int8"),
    torch.int16: np.dtype("int16"), torch.float16: np.dtype("float16"),
}
_TORCH_SMALL_BACK = {v: k for k, v in _TORCH_SMALL.items()}
_PRESERVE_SMALL = (
    "min", "nanmin", "max", "nanmax", "first", "last", "nanfirst", "nanlast",
    "mode", "nanmode",
)


def _cast_back_small(out_np: np.ndarray, func: str, small, fill_value=None) -> np.ndarray:
    # final cast from the promoted compute dtype back to the reference's
    # output dtype for a small input dtype (see _SMALL_PROMOTE)
    if small is None:
        return out_np
    small = np.dtype(small)
    if fill_value is not None:
        # a user fill promotes the output dtype unconditionally (reference
        # xrdtypes.py:170-171) — core already computed in the promoted
        # result dtype, so no cast-back applies
        try:
            tgt = small if func in _PRESERVE_SMALL else (
                np.dtype(np.uint64) if small.kind == "u"
                else np.dtype(np.int64) if small.kind == "i" else small)
            if np.result_type(tgt, fill_value) != tgt:
                return out_np
        except TypeError:
            return out_np
    if small == np.dtype(np.uint64):
        if func in _PRESERVE_SMALL:
            # values < 2**63 (guarded at entry); NA fill int64-min maps to
            # uint64 NA = 0
            return np.where(
                out_np == np.iinfo(np.int64).min, 0, out_np
            ).astype(np.uint64)
        if func in ("sum", "nansum", "prod", "nanprod", "cumsum", "nancumsum"):
            out_np = np.where(out_np == np.iinfo(np.int64).min, 0, out_np) \
                if func in ("sum", "nansum", "prod", "nanprod") else out_np
            return out_np.astype(np.int64).view(np.uint64)  # wrap-exact
        if func in ("ffill", "bfill"):
            return out_np.view(np.uint64)  # identity carry
        return out_np
    if func in _PRESERVE_SMALL:
        if small.kind in "iu" and out_np.dtype.kind == "i":
            # the promoted NA fill (iinfo(promoted).min) maps to the small
            # dtype's NA (iinfo(small).min); real data never hits it
            out_np = np.where(
                out_np == np.iinfo(out_np.dtype).min, np.iinfo(small).min, out_np
            )
        return out_np.astype(small)
    if func in ("ffill", "bfill"):
        # identity-carry preserves the input dtype for every kind
        return out_np.astype(small)
    if func in ("sum", "nansum", "prod", "nanprod", "cumsum", "nancumsum"):
        if small.kind == "u":
            if out_np.dtype.kind == "i":
                # empty-group NA fill: iinfo(int64).min on the promoted
                # dtype maps to iinfo(uint64).min == 0 on the true output
                out_np = np.where(
                    out_np == np.iinfo(np.int64).min, 0, out_np
                )
            return out_np.astype(np.uint64)
        if small.kind == "i":
            return out_np.astype(np.int64)
        return out_np.astype(small)  # float16 sums stay float16
    if small.kind == "f" and func in (
        "mean", "nanmean", "var", "nanvar", "std", "nanstd",
        "median", "nanmedian", "ffill", "bfill",
    ):
        # NOT quantile/nanquantile: their final dtype is ALWAYS float64
        # (reference aggregations.py:695-710); median preserves floating
        return out_np.astype(small)
    return out_np


_FUSED_FUNCS = {
    "mean": (_ffi.FINISH_MEAN, _ffi.SET_SUM_COUNT),
    "nanmean": (_ffi.FINISH_MEAN, _ffi.SET_SUM_COUNT),
    "sum": (_ffi.FINISH_SUM, _ffi.SET_SUM_COUNT_PRESENT),
    "nansum": (_ffi.FINISH_SUM, _ffi.SET_SUM_COUNT_PRESENT),
    "count": (_ffi.FINISH_COUNT, _ffi.SET_COUNT),
}


def _fused_finish(func, op_set, val_dtype, out_dtype, min_count_, fill_value):
    """The `finish=` request that makes the combine kernel reproduce this
    call's finalize (division, mask, fill, cast), or None where the torch
    finalize must run: the two fill cases that inspect the mask on the host
    (no fill with min_count > 0; a NaN fill into an integer result, which
    promotes the dtype) and dtype pairs the kernel does not convert."""
    if func not in _FUSED_FUNCS or _FUSED_FUNCS[func][1] != op_set:
        return None
    mode = _FUSED_FUNCS[func][0]
    try:
        t_out = _torch_dtype(out_dtype)
    except Exception:
        return None
    float_out = t_out in (torch.float32, torch.float64)
    if not float_out and (t_out != torch.int64 or mode == _ffi.FINISH_MEAN):
        return None
    if val_dtype not in (torch.float32, torch.float64, torch.int32, torch.int64):
        return None
    if val_dtype.is_floating_point and mode == _ffi.FINISH_SUM and not float_out:
        return None  # f64 sums to an integer dtype: torch's cast rules apply
    if min_count_ > 0:
        fv = fill_value
        if fv is None:
            return None
    else:
        fv = fill_value if fill_value is not None else xrdtypes.fill_default(func, out_dtype)
    if isinstance(fv, (bool, np.bool_)) or not isinstance(
        fv, (int, float, np.integer, np.floating)
    ):
        return None
    nan_fv = isinstance(fv, (float, np.floating)) and math.isnan(fv)
    if nan_fv and not float_out:
        return None
    if nan_fv and mode != _ffi.FINISH_MEAN and not val_dtype.is_floating_point:
        return None  # NaN into an integer sum/count promotes: torch finalize
    # the kernel carries the fill as a double: it must survive the round trip
    if not float_out and not (
        float(fv) == int(fv) and int(float(fv)) == int(fv) and -(2**63) <= int(fv) < 2**63
    ):
        return None
    if float_out and isinstance(fv, (int, np.integer)) and int(float(fv)) != int(fv):
        return None
    if min_count_ == 0 and nan_fv and mode == _ffi.FINISH_MEAN:
        fv = None  # 0/0 already is the NaN the fill would write
    return (mode, t_out, int(min_count_), None if fv is None else float(fv))


class _ManyCall:
    """What the groupby_reduce calls made by one groupby_reduce_many share:
    the factorization, the SET_SUMMARY partials (gathered by the first func
    that needs a kernel pass) and the sort=False group order. `eligible` is
    decided once, by the first call that reaches the 1-D or the column
    engine (every call of one groupby_reduce_many has the same leading
    dims)."""

    def __init__(self):
        self.facs = None
        self.eligible = None
        self.partials = None
        self.orders = {}


def _from_summary(S, op_set, skipnan):
    """The partials `op_set` would have produced, derived from the
    NaN-skipping SET_SUMMARY partials S. Without skipnan a NaN row poisons
    the sums (as it does in the kernels); min/max carry nanflag and the
    finalize applies it."""
    poison = None
    if not skipnan and S["sum"].dtype.is_floating_point:
        poison = S["nanflag"] != 0

    def nanned(t):
        return t if poison is None else torch.where(poison, torch.full_like(t, float("nan")), t)

    if op_set == _ffi.SET_SSD:
        return {"sum": nanned(S["ssd"])}
    if op_set == _ffi.SET_WELFORD:  # the column path's var_chunk triple
        return {"wssd": nanned(S["ssd"]), "wsum": nanned(S["sum"].to(torch.float64)),
                "count": S["count"]}
    if op_set == _ffi.SET_SUM_COUNT:
        return {"sum": nanned(S["sum"]), "count": S["count"]}
    if op_set == _ffi.SET_SUM_COUNT_PRESENT:
        return {"sum": nanned(S["sum"]), "count": S["count"], "present": S["present"]}
    if op_set == _ffi.SET_COUNT:
        return {"count": S["count"]}
    if op_set in (_ffi.SET_MIN_FULL, _ffi.SET_MAX_FULL):
        k = "min" if op_set == _ffi.SET_MIN_FULL else "max"
        return {k: S[k], "count": S["count"], "present": S["present"],
                "nanflag": S["nanflag"]}
    if op_set in (_ffi.SET_MIN_COUNT, _ffi.SET_MAX_COUNT):
        k = "min" if op_set == _ffi.SET_MIN_COUNT else "max"
        return {k: S[k], "count": S["count"]}
    raise NotImplementedError(f"op set {op_set} from summary partials")  # pragma: no cover


def _coerce_by(b):
    # by / expected arrays in dtypes torch cannot ingest (u16/u32/i8/f16...)
    # carry the same information as int64/f32 - convert before the device
    if isinstance(b, torch.Tensor):
        return b
    b = np.asarray(b)
    if b.dtype.kind in "iub" and b.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        return b.astype(np.int64)
    if b.dtype == np.float16:
        return b.astype(np.float32)
    return b


# host staging buffers whose H2D copies get captured into a hipGraph must
# outlive every replay (the graph re-executes the copy from the same host
# address) — pin them here while capturing
_CAPTURE_KEEPALIVE: list = []


def _fill_scalar(fv, dtype, device, like: torch.Tensor) -> torch.Tensor:
    """0-dim fill tensor for a where() over `like`. torch.tensor copies from
    host memory, which a stream under hipGraph capture cannot do: there the
    value is written by a fill kernel instead."""
    if like.is_cuda and torch.cuda.is_current_stream_capturing():
        return torch.full((), fv, dtype=dtype, device=device)
    return torch.tensor(fv, dtype=dtype, device=device)


def _keepalive_if_capturing(t: torch.Tensor) -> torch.Tensor:
    if torch.cuda.is_current_stream_capturing():
        _CAPTURE_KEEPALIVE.append(t)
    return t


def _as_device_tensor(x, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = _keepalive_if_capturing(torch.from_numpy(np.ascontiguousarray(x)))
    if t.device != device:
        t = t.to(device, non_blocking=True)
    return t


class _FactorizedBy:
    """One by-array turned into dense integer codes on device.

    direct=True: codes ARE the raw labels (expected_groups is 0..n-1), so the
    kernel's bounds check is the whole factorize step (the GPU analogue of
    the reference's RangeIndex fast path, factorize.py:44-53)."""

    def __init__(self, codes: torch.Tensor, groups: np.ndarray, direct: bool):
        self.codes = codes
        self.groups = groups
        self.ngroups = len(groups)
        self.direct = direct


def _factorize_bins(flat: torch.Tensor, edges: np.ndarray, dt_by=None) -> _FactorizedBy:
    """Bin-edge grouping (isbin=True): right-closed intervals (edges[i-1],
    edges[i]], values outside every interval -> invalid (restates reference
    factorize.py:55-82: np.digitize(right=True) - 1). Groups are the
    pandas IntervalIndex the reference returns. Datetime edges bin the
    int64-viewed by on unit-aligned views (dt_by = the by dtype)."""
    import pandas as pd

    edges = np.asarray(edges)
    assert edges.ndim == 1 and len(edges) >= 2, "bin edges need >= 2 values"
    iv_groups = pd.IntervalIndex.from_breaks(edges)
    if edges.dtype.kind in "Mm":
        assert dt_by is not None, "datetime bin edges need a datetime by"
        edges = edges.astype(dt_by).view("i8")
    nbins = len(edges) - 1
    fl = flat
    edges_t = _keepalive_if_capturing(
        torch.from_numpy(np.ascontiguousarray(edges))
    ).to(flat.device)
    if edges_t.dtype != fl.dtype:
        common = torch.promote_types(edges_t.dtype, fl.dtype)
        edges_t = edges_t.to(common)
        fl = fl.to(common)
    codes = torch.searchsorted(edges_t, fl, right=False) - 1
    bad = (codes < 0) | (codes >= nbins)
    if fl.dtype.is_floating_point:
        bad |= torch.isnan(fl)
    codes = torch.where(bad, torch.full_like(codes, -1), codes)
    return _FactorizedBy(codes, iv_groups, direct=False)


def _factorize_device(flat: torch.Tensor, expect, sort: bool, dt_by=None) -> _FactorizedBy:
    """labels -> codes in [0, ngroups), invalid/NaN -> out-of-range
    (restates reference _factorize_single, factorize.py:42-99).

    dt_by: original numpy datetime64/timedelta64 dtype when the by array was
    viewed as int64 — NaT (int64 min) rows are missing (pd.factorize drops
    NaT) and found/expected groups convert back to dt_by."""
    if dt_by is not None:
        nat = torch.iinfo(torch.int64).min
        if expect is None:
            fl = flat[flat != nat]
            uniq = torch.unique(fl)  # sorted; NaT excluded
            codes = torch.searchsorted(uniq, flat)
            codes = torch.where(flat == nat, torch.full_like(codes, -1), codes)
            codes = torch.clamp(codes, max=max(uniq.numel() - 1, 0))
            return _FactorizedBy(codes, uniq.cpu().numpy().view(dt_by), direct=False)
        expect_np = np.asarray(expect)
        assert expect_np.dtype.kind in "Mm", "datetime by needs datetime expected_groups"
        # align to the by array's unit (the reference returns groups in the
        # by's unit, e.g. expected [D] against a [s] by -> groups [s])
        sorted_expect = (np.sort(expect_np) if sort else expect_np).astype(dt_by)
        exp_t = _keepalive_if_capturing(
            torch.from_numpy(sorted_expect.view("i8").copy())
        ).to(flat.device)
        n = exp_t.numel()
        codes = torch.searchsorted(exp_t, flat)
        clipped = torch.clamp(codes, max=n - 1)
        bad = (codes == n) | (exp_t[clipped] != flat) | (flat == nat)
        codes = torch.where(bad, torch.full_like(codes, -1), clipped)
        return _FactorizedBy(codes, sorted_expect, direct=False)
    if expect is None:
        fl = flat
        if fl.dtype.is_floating_point:
            fl = fl[~torch.isnan(fl)]
        uniq = torch.unique(fl)  # sorted
        codes = torch.searchsorted(uniq, flat)
        if flat.dtype.is_floating_point:
            codes = torch.where(torch.isnan(flat), torch.full_like(codes, -1), codes)
        return _FactorizedBy(codes, uniq.cpu().numpy(), direct=False)

    if isinstance(expect, range):
        # O(1) RangeIndex-style fast path (reference factorize.py:44-53)
        if expect.step != 1 or expect.start != 0:
            expect = np.asarray(expect)
        elif flat.dtype.is_floating_point:
            expect = np.asarray(expect)
        else:
            # groups echo the caller's range (materializing np.arange(1e7)
            # costs ~10 ms per call)
            return _FactorizedBy(flat, expect, direct=True)
    expect_np = np.asarray(expect)
    n = len(expect_np)
    if (
        expect_np.dtype.kind in "iu"
        and not flat.dtype.is_floating_point
        and n > 0
        and expect_np[0] == 0
        and expect_np[-1] == n - 1
        and np.array_equal(expect_np, np.arange(n))
    ):
        # direct path: labels are already the codes; the kernel's unsigned
        # bounds check drops anything outside [0, n)
        return _FactorizedBy(flat, expect_np, direct=True)

    sorted_expect = np.sort(expect_np) if sort else expect_np
    if sort is False and not np.all(np.diff(expect_np) >= 0):
        raise NotImplementedError("unsorted expected_groups with sort=False")
    exp_t = _keepalive_if_capturing(
        torch.from_numpy(np.ascontiguousarray(_coerce_by(sorted_expect)))
    ).to(flat.device)
    if exp_t.dtype != flat.dtype:
        common = torch.promote_types(exp_t.dtype, flat.dtype)
        exp_t = exp_t.to(common)
        flat = flat.to(common)
    codes = torch.searchsorted(exp_t, flat)
    clipped = torch.clamp(codes, max=n - 1)
    bad = (codes == n) | (exp_t[clipped] != flat)
    if flat.dtype.is_floating_point:
        bad |= torch.isnan(flat)
    codes = torch.where(bad, torch.full_like(codes, -1), codes)
    return _FactorizedBy(codes, sorted_expect, direct=False)


def _factorize_strings_host(flat_np: np.ndarray, expect, sort: bool, device) -> _FactorizedBy:
    """String/object labels: the reference's pd.factorize hash path runs on
    the HOST (strings have no device representation); the dense int64 codes
    ship to the GPU (reference factorize.py:96)."""
    if expect is None:
        uniq, inv = np.unique(flat_np, return_inverse=True)  # sorted
        codes = inv.astype(np.int64)
        groups = uniq
    else:
        expect_np = np.asarray(expect)
        sorted_expect = np.sort(expect_np) if sort else expect_np
        if not sort and len(sorted_expect) > 1 and not np.all(
            sorted_expect[:-1] <= sorted_expect[1:]
        ):
            raise NotImplementedError("unsorted expected_groups with sort=False")
        idx = np.searchsorted(sorted_expect, flat_np).astype(np.int64)
        n = len(sorted_expect)
        clip = np.clip(idx, 0, max(n - 1, 0))
        bad = (idx == n) | (sorted_expect[clip] != flat_np)
        codes = np.where(bad, -1, clip)
        groups = sorted_expect
    t = torch.from_numpy(np.ascontiguousarray(codes)).to(device)
    return _FactorizedBy(t, groups, direct=False)


def _combined_codes(facs: list[_FactorizedBy]):
    """Combine multiple factorized by-arrays into one code stream.

    Returns (labels, labels2, grp_pair): when exactly two direct int code
    arrays, the ravel is fused into the kernel (labels2 path, mirroring
    reference _ravel_factorized factorize.py:102-108); otherwise codes are
    raveled here with invalid propagation."""
    if len(facs) == 1:
        return facs[0].codes, None, None
    if len(facs) == 2 and all(f.direct for f in facs):
        return facs[0].codes, facs[1].codes, (facs[0].ngroups, facs[1].ngroups)
    code = facs[0].codes.to(torch.int64)
    bad = code < 0
    for f in facs[1:]:
        c = f.codes.to(torch.int64)
        bad = bad | (c < 0) | (code < 0)
        code = code * f.ngroups + c
    code = torch.where(bad, torch.full_like(code, -1), code)
    return code, None, None


def _bounded_codes(labels, labels2, grp_pair, ngroups, check_single=True):
    """One int64 code stream in [-1, ngroups) from what _combined_codes
    returned: two direct code arrays ravel as c0 * g1 + c1, and whatever the
    kernel's own bounds check would have dropped becomes -1. The cross-rank
    selections bound-check a single label array themselves
    (check_single=False)."""
    c0 = labels.to(torch.int64)
    if labels2 is None:
        if not check_single:
            return c0
        return torch.where((c0 < 0) | (c0 >= ngroups), torch.full_like(c0, -1), c0)
    g0, g1 = grp_pair
    c1 = labels2.to(torch.int64)
    bad = (c0 < 0) | (c0 >= g0) | (c1 < 0) | (c1 >= g1)
    return torch.where(bad, torch.full_like(c0, -1), c0 * g1 + c1)


_CUSTOM_CHUNK_OK = frozenset(
    "sum nansum count nanlen min nanmin max nanmax prod nanprod".split()
)
_COMPLEX_OK = ("sum", "nansum", "mean", "nanmean", "count", "first", "last", "nanfirst", "nanlast")


def _reduce_custom(array, by, func, kw):
    """Reference-style custom aggregation (docs "Custom Aggregations"): run
    each chunk reduction through the full machinery, then apply the user's
    finalize and the final fill for empty groups."""
    inner = {k: v for k, v in kw.items() if k not in _PER_FUNC_ARGS}
    inters, groups_c, counts_c = [], None, None
    for cn in func.chunk:
        cn2 = "count" if cn == "nanlen" else cn
        if cn2 not in _CUSTOM_CHUNK_OK:
            raise NotImplementedError(f"custom aggregation chunk {cn!r}")
        r, *g = groupby_reduce(array, *by, func=cn2, **inner)
        inters.append(r)
        groups_c = g
        if cn2 == "count":
            counts_c = r
    if counts_c is None:
        counts_c, *_ = groupby_reduce(array, *by, func="count", **inner)
    res = func.finalize(*inters) if func.finalize is not None else inters[0]
    fill_value = kw["fill_value"]
    ffv = fill_value if fill_value is not None else func.final_fill_value
    mask = counts_c == 0
    if isinstance(res, torch.Tensor):
        if not isinstance(mask, torch.Tensor):
            mask = torch.as_tensor(np.asarray(mask), device=res.device)
        if ffv is not None and bool(mask.any().item()):
            nan_on_int = (
                isinstance(ffv, float) and math.isnan(ffv)
                and not res.dtype.is_floating_point
            )
            if nan_on_int:
                res = res.to(torch.float64)
            res = torch.where(mask, torch.tensor(ffv, dtype=res.dtype, device=res.device), res)
        if func.final_dtype is not None:
            res = res.to(_torch_dtype(np.dtype(func.final_dtype)))
    else:
        res = np.asarray(res)
        if ffv is not None and bool(np.any(mask)):
            res = np.where(mask, ffv, res)
        if func.final_dtype is not None:
            res = res.astype(func.final_dtype)
    return (res, *groups_c)


def _reduce_complex(arr_np, by, func, kw):
    """Complex input: the linear set computes on a (2, ...) re/im component
    view (components are independent for sums/means/first/last and scans);
    whole-value nulls (either component NaN — the reference's isnull) premask
    BOTH components for skipna funcs. Order/product/var families have no
    componentwise form: raise."""
    if func not in _COMPLEX_OK:
        raise NotImplementedError(f"complex input for {func!r} (supported: {_COMPLEX_OK})")
    fill_value, dtype, axis = kw["fill_value"], kw["dtype"], kw["axis"]
    if fill_value is not None and not (
        isinstance(fill_value, (float, complex)) and np.isnan(np.asarray(fill_value).real)
    ):
        raise NotImplementedError("complex input with a non-NaN fill_value")
    comp_dt = arr_np.dtype
    if func == "count":
        # count ignores magnitudes: a real view with whole-value nulls
        # mapped to NaN is exact
        real = arr_np.real.astype(np.float64)
        real[np.isnan(arr_np)] = np.nan
        return groupby_reduce(real, *by, func=func, **kw)
    fwidth = np.float64 if comp_dt == np.dtype(np.complex128) else np.float32
    fv2 = arr_np.view(fwidth).reshape(arr_np.shape + (2,)).copy()
    if REDUCTIONS[func].skipnan:
        fv2[np.isnan(arr_np)] = np.nan  # both components
    comps = np.moveaxis(fv2, -1, 0)  # (2, ...original dims)
    ax2 = axis
    if axis is not None:
        axl = axis if isinstance(axis, (tuple, list)) else (axis,)
        ax2 = tuple((a % arr_np.ndim) + 1 for a in axl)
    r, *grps = groupby_reduce(
        np.ascontiguousarray(comps), *by, func=func, **{**kw, "axis": ax2, "dtype": None}
    )
    out = np.asarray(r)
    res = (out[0] + 1j * out[1]).astype(comp_dt if dtype is None else np.dtype(dtype))
    return (res, *grps)


# what _normalize_input learned about the caller's array; fill_value is the
# user's, defaulted for datetimes, and user_fill_value the user's untouched
# (internal defaults must not trigger _cast_back_small's promotion rule)
_Input = namedtuple(
    "_Input",
    "return_numpy small_dtype dt_dtype was_bool in_np_dtype fill_value user_fill_value",
)


def _normalize_input(array, func, fill_value, device):
    """The values as a device tensor of a compute dtype (f32/f64/i32/i64),
    and the _Input record of what was coerced on the way. Complex input
    never gets here (_reduce_complex)."""
    return_numpy = not isinstance(array, torch.Tensor)
    user_fill_value = fill_value
    dt_dtype = small_dtype = None
    if return_numpy:
        arr_np = np.asarray(array)
        if arr_np.dtype in _SMALL_PROMOTE:
            small_dtype = arr_np.dtype
            array = arr_np = arr_np.astype(_SMALL_PROMOTE[arr_np.dtype])
        elif arr_np.dtype == np.uint64:
            # uint64 computes on its int64 VIEW: sums/prods/counts are
            # wrap-exact mod 2^64; order-dependent funcs are only correct
            # below 2^63, so values with the high bit set are rejected there
            small_dtype = arr_np.dtype
            array = arr_np = arr_np.view(np.int64)
            if func not in (
                "sum", "nansum", "count", "prod", "nanprod", "any", "all",
            ) and bool((arr_np < 0).any()):
                raise NotImplementedError(
                    f"{func} on uint64 values >= 2**63 (int64-view order breaks)"
                )
        if arr_np.dtype.kind in "Mm":
            # datetime64/timedelta64 values compute on their int64 view and
            # dtype-preserving results view back (reference core.py:985-1001)
            dt_dtype = arr_np.dtype
            array = arr_np.view("i8")
            # NaT (= INT64_MIN) passes through the int64 view untouched, as
            # in the reference (core.py:994-997): it wins min and loses max;
            # count and nanfirst/nanlast skip NaT rows (_build_codes); empty
            # groups fill with NaT (xrdtypes.py:54-61)
            if func in xrdtypes.PRESERVES_DTYPE and fill_value is None:
                fill_value = np.iinfo(np.int64).min
    arr = _as_device_tensor(array, device)
    if arr.dtype in _TORCH_SMALL:
        small_dtype = _TORCH_SMALL[arr.dtype]
        arr = arr.to(_torch_dtype(_SMALL_PROMOTE[small_dtype]))
    was_bool = arr.dtype == torch.bool
    if was_bool:
        arr = arr.to(torch.int64)  # reference core.py:916-917
    return arr, _Input(return_numpy, small_dtype, dt_dtype, was_bool,
                       _np_dtype(arr.dtype), fill_value, user_fill_value)


def _align_by(arr, by, axis, device):
    """Coerce the by arrays, check them against the array's trailing dims
    (size-1 dims broadcast) and, for an axis subset of by's dims, move the
    reduced dims last. Returns (bys, by_dts, by_shape, arr, subset_keep_shape,
    subset_by_inv, lead_shape, lead_M)."""
    if len(by) == 0:
        raise ValueError("need at least one by array")
    by_dts, bys = [], []
    for b in by:
        dtb, host = None, False
        if not isinstance(b, torch.Tensor):
            b = np.asarray(b)
            # string/object labels factorize on the host
            # (_factorize_strings_host); the array stays numpy until then
            host = b.dtype.kind in "US" or b.dtype == object
            if b.dtype.kind in "Mm":
                # group BY datetimes on the int64 view; NaT rows are missing
                dtb = b.dtype
                b = b.view("i8")
            elif not host:
                b = _coerce_by(b)
        by_dts.append(dtb)
        bys.append(b if host else _as_device_tensor(b, device))
    bys = tuple(bys)
    # size-1 by dims broadcast against the array's trailing dims (the
    # dim=... case, reference core.py:300-309); multiple by arrays must
    # share a shape, as in the reference
    by_shape = bys[0].shape
    for b in bys:
        if b.shape != by_shape:
            raise ValueError("by arrays must have the same shape")
    if len(by_shape) <= arr.ndim:
        trail = tuple(arr.shape[arr.ndim - len(by_shape):])
        if trail != tuple(by_shape) and all(
            bs in (1, ts) for bs, ts in zip(by_shape, trail)
        ):
            bys = tuple(
                np.ascontiguousarray(np.broadcast_to(b, trail))
                if isinstance(b, np.ndarray)
                else b.broadcast_to(trail).contiguous()
                for b in bys
            )
            by_shape = bys[0].shape
    if tuple(arr.shape[arr.ndim - len(by_shape) :]) != tuple(by_shape):
        raise ValueError(f"by {tuple(by_shape)} must align with trailing dims of array {tuple(arr.shape)}")
    subset_keep_shape = subset_by_inv = None
    if axis is not None:
        ax = axis if isinstance(axis, (tuple, list)) else (axis,)
        ax = tuple(a % arr.ndim for a in ax)
        trailing = tuple(range(arr.ndim - len(by_shape), arr.ndim))
        if tuple(sorted(ax)) != trailing:
            # axis subset of by's dims (reference offset-labels case,
            # factorize.py:24-39): move reduced dims last and fold the kept
            # by-dims into the group codes (_build_codes)
            if not set(ax) <= set(trailing):
                raise ValueError(f"axis {axis} must address dims of by")
            nlead_s = arr.ndim - len(by_shape)
            keep = [d for d in range(arr.ndim) if d not in ax]  # lead + kept by dims
            perm = keep + sorted(ax)
            arr = arr.permute(perm).contiguous()
            by_perm = [d - nlead_s for d in perm if d >= nlead_s]
            bys = tuple(
                np.ascontiguousarray(np.transpose(b, by_perm))
                if isinstance(b, np.ndarray)
                else b.permute(by_perm).contiguous()
                for b in bys
            )
            by_shape = bys[0].shape  # (kept by dims..., reduced dims...)
            subset_keep_shape = tuple(arr.shape[nlead_s : len(keep)])
            # for sort=False: first-appearance order is defined on the
            # ORIGINAL by layout — keep the inverse permutation
            subset_by_inv = tuple(int(i) for i in np.argsort(by_perm))
    lead_shape = tuple(arr.shape[: arr.ndim - len(by_shape)])
    lead_M = math.prod(lead_shape) if lead_shape else 1
    return bys, by_dts, by_shape, arr, subset_keep_shape, subset_by_inv, lead_shape, lead_M


def _group_spec(expected_groups, isbin, nby):
    """expected_groups and isbin as one entry per by array. Returns
    (expected_groups, isbins, provided_expected)."""
    if expected_groups is not None and not isinstance(expected_groups, tuple):
        expected_groups = (expected_groups,)
    if expected_groups is None:
        expected_groups = (None,) * nby
    # pd.IntervalIndex expected groups imply binning (reference
    # _convert_expected_groups_to_index, core.py:931-933)
    try:
        import pandas as pd

        isbins0 = isbin if isinstance(isbin, (tuple, list)) else (isbin,) * nby
        if any(isinstance(e, pd.IntervalIndex) for e in expected_groups):
            new_eg, new_isbin = [], []
            for e, ib in zip(expected_groups, isbins0):
                if isinstance(e, pd.IntervalIndex):
                    assert (e.left.to_numpy()[1:] == e.right.to_numpy()[:-1]).all(), (
                        "IntervalIndex bins must be contiguous"
                    )
                    e, ib = np.append(e.left.to_numpy(), e.right.to_numpy()[-1]), True
                new_eg.append(e)
                new_isbin.append(ib)
            expected_groups = tuple(new_eg)
            isbin = tuple(new_isbin)
    except ImportError:
        pass
    provided_expected = any(e is not None for e in expected_groups)
    if isbin and not provided_expected:
        raise ValueError("isbin=True requires expected_groups (the bin edges)")
    isbins = isbin if isinstance(isbin, (tuple, list)) else (isbin,) * nby
    return expected_groups, isbins, provided_expected


def _factorize(bys, expected_groups, isbins, by_dts, sort, device):
    """One _FactorizedBy per by array. groupby_reduce_many runs this once
    and hands the list to every func of the call."""
    return [
        _factorize_strings_host(b.reshape(-1), e, sort, device)
        if isinstance(b, np.ndarray)
        else _factorize_bins(b.reshape(-1), e, dt_by=dtb)
        if ib
        else _factorize_device(b.reshape(-1), e, sort, dt_by=dtb)
        for b, e, ib, dtb in zip(bys, expected_groups, isbins, by_dts)
    ]


class _Plan:
    """What the stages of one reduction share; engines and families read it.
    `ngroups` counts the bins the engine reduces into (grp_shape times the
    subset and lead folds); `out_prefix` holds result dims in front of the
    lead dims (quantile's q)."""

    __slots__ = (
        # _reduce: the call
        "func", "agg", "inp", "device", "sort", "finalize_kwargs", "ddof",
        "shard_row_offset", "dist_on", "provided_expected", "many", "out_prefix",
        # _align_by
        "arr", "bys", "by_shape", "lead_shape", "lead_M", "subset_keep_shape", "subset_by_inv",
        # _factorize, _build_codes
        "facs", "grp_shape", "labels", "labels2", "grp_pair", "ngroups", "vals",
        "nat_skip_after_fold",
        # _resolve_fill
        "min_count_", "fill_value", "out_dtype",
        # _select_engine, _fold_lead
        "label_src", "row_offset", "cols", "many_served", "lead_folded",
        "arg_localize_N", "base_ngroups", "cols_order", "cols_sorted_rows",
        "cols_select",
    )


def _build_codes(p):
    """facs -> the code stream the engine reduces over: the combined codes,
    minus NaT rows where they count as missing, offset per kept slice under
    an axis subset."""
    func, device = p.func, p.device
    p.nat_skip_after_fold = False
    p.grp_shape = tuple(f.ngroups for f in p.facs)
    p.ngroups = math.prod(p.grp_shape)
    p.labels, p.labels2, p.grp_pair = _combined_codes(p.facs)

    if p.inp.dt_dtype is not None and func in ("count", "nanfirst", "nanlast"):
        # NaT rows are missing for count (verified reference behavior) and
        # for nanfirst/nanlast (xrutils.nanfirst's isnull, xrutils.py:389-397):
        # drop them by invalidating their codes; with leading dims NaT-ness
        # is per (lead, row), so count recounts on a float view instead
        # (NaT -> NaN; exact, count ignores magnitudes) and nanfirst/nanlast
        # invalidate the per-(lead, row) composite codes after the lead fold
        if p.lead_M != 1:
            if func == "count":
                p.arr = torch.where(
                    p.arr == torch.iinfo(torch.int64).min,
                    torch.tensor(float("nan"), dtype=torch.float64, device=device),
                    p.arr.to(torch.float64),
                )
            else:
                p.nat_skip_after_fold = True
        else:
            natm = p.arr.reshape(-1) == torch.iinfo(torch.int64).min
            p.labels = torch.where(natm, torch.full_like(p.labels, -1), p.labels)

    if p.subset_keep_shape is not None:
        # offset the codes by the kept-dims slice index (reference
        # offset_labels, factorize.py:24-39): slice s's groups become bins
        # [s*ngroups, (s+1)*ngroups)
        base_codes = _bounded_codes(p.labels, p.labels2, p.grp_pair, p.ngroups)
        inner_n = math.prod(p.by_shape[len(p.subset_keep_shape):])
        lead_idx = torch.arange(base_codes.numel(), device=device) // inner_n
        offset = lead_idx * p.ngroups + base_codes
        p.labels = torch.where(base_codes < 0, torch.full_like(base_codes, -1), offset)
        p.labels2, p.grp_pair = None, None
        p.ngroups = int(math.prod(p.subset_keep_shape)) * p.ngroups
    # only the 1-D path flattens the values (a no-op for contiguous input);
    # the column path reads the caller's strided view directly
    p.vals = p.arr.reshape(-1) if p.lead_M == 1 else None


def _resolve_fill(p, dtype, min_count):
    """min_count, fill_value and output dtype defaulting (reference
    core.py:1026-1038 + aggregations.py:997-1003)."""
    func, fill_value = p.func, p.inp.fill_value
    min_count_ = min_count
    if min_count is None:
        needs_one = (fill_value is not None and p.provided_expected) or p.subset_keep_shape is not None
        min_count_ = 1 if needs_one else 0
    out_dtype = xrdtypes.final_dtype(func, p.inp.in_np_dtype, dtype)
    if func in ("nanmin", "nanmax") and min_count_ == 0:
        min_count_ = 1
        if fill_value is None:
            fill_value = xrdtypes.fill_default(func, out_dtype)
    if min_count_ > 0 and func in ("nansum", "nanprod") and fill_value is None:
        fill_value = float("nan")
    if fill_value is not None:
        # user fill promotes the output dtype (reference xrdtypes.py:170-171)
        out_dtype = np.result_type(out_dtype, fill_value)
    p.min_count_, p.fill_value, p.out_dtype = min_count_, fill_value, out_dtype


class _Engine:
    """How a family asks for kernel passes over the plan's rows:
    run(op_set, skipnan, means=None, target=None, finish=None) -> partials.
    _select_engine picks the subclass once per call."""

    def __init__(self, plan):
        self.p = plan

    def count(self, skipnan=True):
        # a SET_COUNT pass of its own, summed across ranks when distributed
        p = self.p
        pc = grouped_partials(
            _ffi.SET_COUNT, p.vals, p.labels, p.ngroups, skipnan=skipnan,
            labels2=p.labels2, grp_shape=p.grp_pair,
        )
        if p.dist_on:
            distributed.all_reduce_(pc["count"], "sum")
        return pc["count"]


class _Engine1D(_Engine):
    """grouped_partials over the flattened values: no leading dims, or
    leading dims folded into the group codes (_fold_lead)."""

    def run(self, op_set, skipnan, means=None, target=None, finish=None):
        p = self.p
        # these keywords travel only when set: stand-ins for grouped_partials
        # with the older signature keep working
        opt_kw = {} if p.label_src is None else {"label_src": p.label_src}
        if finish is not None:
            opt_kw["finish"] = finish
        return grouped_partials(
            op_set, p.vals, p.labels, p.ngroups, skipnan=skipnan,
            labels2=p.labels2, grp_shape=p.grp_pair, means=means,
            target=target, row_offset=p.row_offset, **opt_kw,
        )


class _EngineSummary(_Engine1D):
    """A fused-set func of an eligible groupby_reduce_many call: every pass
    it asks for is answered from the call's one SET_SUMMARY pass, and the
    finalize runs unchanged."""

    def run(self, op_set, skipnan, means=None, target=None, finish=None):
        many = self.p.many
        if many.partials is None:
            many.partials = super().run(_ffi.SET_SUMMARY, True)
        return _from_summary(many.partials, op_set, skipnan)


class _EngineCols(_Engine):
    """Leading dims as columns: rows sorted by code, one contiguous segment
    per group (grouped_partials_cols)."""

    def run(self, op_set, skipnan, means=None, target=None, finish=None):
        vt, scodes, perm = self.p.cols
        return grouped_partials_cols(
            op_set, vt, scodes, perm, self.p.ngroups, skipnan=skipnan, means=means
        )


class _EngineColsSummary(_EngineCols):
    """A fused-set func of an eligible groupby_reduce_many call over leading
    dims: one SET_SUMMARY column pass serves every pass the call's fused
    funcs ask for, as _EngineSummary does without leading dims. The column
    kernel keeps its state in registers, so no group-count limit applies."""

    def run(self, op_set, skipnan, means=None, target=None, finish=None):
        many = self.p.many
        if many.partials is None:
            many.partials = super().run(_ffi.SET_SUMMARY, True)
        return _from_summary(many.partials, op_set, skipnan)


def _fold_lead(p, codes_full, N):
    """Order-dependent reductions with leading dims: fold the lead index
    into the group codes (lead*ngroups + code) and run the 1-D machinery
    over the C-order flattened stream — the offset-labels trick of reference
    factorize.py:24-39. With an axis subset the two folds COMPOSE: labels
    already carry the kept-by-dims offset (ngroups = keep*base), and the
    extra leading array dims fold on top of that."""
    func, lead_M, ngroups = p.func, p.lead_M, p.ngroups
    if p.subset_keep_shape is not None and func in _ARG_FUNCS:
        raise NotImplementedError(f"{func} with an axis subset and extra leading array dims: next row")
    if p.dist_on:
        raise NotImplementedError(f"distributed {func} with leading dims: next row")
    if N * lead_M >= (1 << 31) or ngroups * lead_M >= (1 << 31):
        raise NotImplementedError(f"{func} with leading dims at this size: next row")
    p.vals = p.arr.reshape(-1)
    lead_i = torch.arange(lead_M, device=p.device, dtype=torch.int64)
    comp = lead_i[:, None] * ngroups + codes_full[None, :]
    comp = torch.where((codes_full < 0)[None, :].expand_as(comp), torch.full_like(comp, -1), comp)
    p.labels = comp.reshape(-1)
    p.labels2, p.grp_pair = None, None
    p.arg_localize_N = N
    p.base_ngroups = ngroups
    p.ngroups = lead_M * ngroups
    p.lead_folded = True
    if p.nat_skip_after_fold:
        # exact NaT skipping per (lead, row): the folded composite codes
        # are per flattened element, so invalidating them IS the
        # int64-sentinel skip (no lossy float view)
        natm = p.vals == torch.iinfo(torch.int64).min
        p.labels = torch.where(natm, torch.full_like(p.labels, -1), p.labels)


def _cols_order_ok(p, vt):
    """Whether an arg-reduction or first/last over leading dims takes the
    column form. Everything else in _LEAD_FOLD_FUNCS, and these where a
    condition fails, keeps the lead fold with its results and exceptions."""
    return (
        COLS_ORDER_FUNCS
        and p.func in _COLS_ORDER
        and vt.dtype in _TORCH_VDTYPE
        and not p.dist_on
        and p.inp.dt_dtype is None
        and p.subset_keep_shape is None
        and vt.numel() > 0 and p.ngroups > 0
        and _ffi.cols_supports(_ffi.SET_ARGMAX_COLS)
    )


def _cols_sorted_ok(p, vt):
    """Whether a quantile-family or mode call over leading dims takes the
    sort-in-LDS column form; sets p.cols_sorted_rows (the largest group's row
    count) when it does. Where a condition fails the call keeps the lead fold
    with its results and exceptions. The largest group is read from the
    sorted codes on the host, the copy grouped_partials_cols also makes for
    its chunk plan: a stream under capture cannot, and keeps the fold. A group
    over the capacity sends the quantile family to the radix-select kernel
    (p.cols_select) where that is on, present and the array wide enough."""
    if not (
        COLS_SORTED_FUNCS
        and p.func in _COLS_SORTED
        and vt.dtype in _TORCH_VDTYPE
        and not p.dist_on
        and p.inp.dt_dtype is None
        and p.subset_keep_shape is None
        and vt.numel() > 0 and p.ngroups > 0
        and not (vt.is_cuda and torch.cuda.is_current_stream_capturing())
    ):
        return False
    cap = _ffi.quantile_cols_max_rows(_TORCH_VDTYPE[vt.dtype])
    if cap <= 0:
        return False
    sc = p.cols[1].cpu().numpy()
    sc = sc[np.searchsorted(sc, 0):]  # rows of code -1 sort first
    edges = np.flatnonzero(np.diff(sc)) + 1
    longest = int(np.diff(np.concatenate(([0], edges, [sc.size]))).max()) if sc.size else 1
    if longest > cap:
        if not (
            COLS_SELECT_FUNCS
            and p.func in _COLS_SELECT
            and p.lead_M >= COLS_SELECT_MIN_COLS
            and _ffi.has_select_cols()
        ):
            return False
        p.cols_select = True
    p.cols_sorted_rows = longest
    return True


def _select_engine(p, by):
    """1-D, column (either summary-served inside an eligible
    groupby_reduce_many), or lead-folded. Fills in the plan's engine fields;
    the lead fold (_fold_lead) also rewrites its vals, labels and ngroups."""
    p.label_src, p.row_offset, p.cols = None, p.shard_row_offset, None
    p.many_served = p.lead_folded = p.cols_order = False
    p.cols_sorted_rows, p.cols_select = None, False
    many, facs = p.many, p.facs
    if p.lead_M == 1:
        # label-code cache key: the CALLER's by object(s) — `labels` is a
        # fresh view on every call. Only direct codes that reach the kernel
        # untouched qualify (searchsorted / bins / string factorizations are
        # the follow-up: DESIGN.md)
        if (
            len(facs) <= 2
            and all(f.direct for f in facs)
            and all(isinstance(b, torch.Tensor) and bb is b for b, bb in zip(by, p.bys))
            and p.labels is facs[0].codes
            and (p.labels2 is facs[1].codes if len(facs) == 2 else p.labels2 is None)
        ):
            p.label_src = tuple(by)
        if many is not None:
            if many.eligible is None:
                many.eligible = (
                    not p.dist_on and p.inp.dt_dtype is None
                    and p.vals.numel() > 0 and summary_fits(p.vals.dtype, p.ngroups)
                )
            p.many_served = many.eligible and p.func in FUSED_MANY_FUNCS
        return _EngineSummary(p) if p.many_served else _Engine1D(p)
    # column path: grouped dims to the front, lead dims flattened as
    # columns (a zero-copy view when the caller's layout is
    # grouped-axis-major, e.g. time-major climatology read through a
    # .permute view; otherwise one transpose copy)
    arr, nbydims = p.arr, len(p.by_shape)
    N = math.prod(p.by_shape)
    arr_t = arr.movedim(tuple(range(arr.ndim - nbydims, arr.ndim)), tuple(range(nbydims)))
    vt = arr_t.reshape((N, p.lead_M))
    if vt.stride(1) != 1:
        vt = vt.contiguous()
    if N >= 2**31 or p.ngroups * p.lead_M >= 2**62:
        raise NotImplementedError("column path: axis length must fit int32")
    # bound codes here (the column kernel trusts codes in [-1, ngroups))
    codes_full = _bounded_codes(p.labels, p.labels2, p.grp_pair, p.ngroups)
    # stable sort of the (small) per-row code vector: rows are then
    # walked in group order, one contiguous segment per group (the GPU
    # analogue of _prepare_for_flox, reference aggregate_flox.py:9-23)
    scodes64, perm64 = torch.sort(codes_full, stable=True)
    p.cols = (vt, scodes64.to(torch.int32), perm64.to(torch.int32))
    if p.func not in _LEAD_FOLD_FUNCS:
        if many is not None:
            if many.eligible is None:
                # no summary_fits here: the column kernel has no LDS bins
                many.eligible = (
                    not p.dist_on and p.inp.dt_dtype is None
                    and vt.numel() > 0 and p.ngroups > 0
                    and vt.dtype in _TORCH_VDTYPE
                )
            p.many_served = many.eligible and p.func in FUSED_MANY_FUNCS
        return _EngineColsSummary(p) if p.many_served else _EngineCols(p)
    if _cols_order_ok(p, vt):
        # the row-valued column sets: no composite labels, no flattened copy,
        # one read of the values, no limit on N * lead_M. Inside
        # groupby_reduce_many these names share the factorization only.
        p.cols_order = True
        return _EngineCols(p)
    if _cols_sorted_ok(p, vt):
        # each group's rows sorted in LDS, or its order statistics selected
        # by radix passes where it is too long for that: no composite labels,
        # no flattened copy, no device-wide sort, no limit on N * lead_M. Inside
        # groupby_reduce_many these names share the factorization only.
        return _EngineCols(p)
    # (the column view and the sort above go unused here: kept, since
    # dropping them would change which kernels these calls launch)
    _fold_lead(p, codes_full, N)
    p.row_offset = 0
    return _Engine1D(p)


# families: (plan, engine) -> (result, empty_mask, counts_for_mask).
# empty_mask None means "count == 0, built only if a fill needs it";
# empty_mask _FINISHED means fill, mask and dtype are already applied.
_FINISHED = object()
_I64_MAX = (1 << 63) - 1


def _quantile_q(p):
    """(q as f64[nq], whether the caller's q was a scalar)."""
    if p.func in ("quantile", "nanquantile"):
        if not p.finalize_kwargs or "q" not in p.finalize_kwargs:
            raise ValueError("Please pass `q` for quantile calculations.")
        q = p.finalize_kwargs["q"]
    else:
        q = 0.5
    return np.atleast_1d(np.asarray(q, dtype=np.float64)), np.isscalar(q) or np.ndim(q) == 0


def _quantile_finish(p, resq, scalar_q, nq, counts):
    """The quantile family's own fill rule: NaN already marks empty groups,
    so only an explicit fill under min_count writes anything. counts is a
    callable: the pass is made only where the rule needs it."""
    result = resq[0] if scalar_q else resq
    if p.min_count_ > 0:
        counts = counts()
        if p.fill_value is not None:
            mask = counts < p.min_count_
            fv = torch.tensor(float(p.fill_value), dtype=result.dtype, device=p.device)
            result = torch.where(mask, fv, result)
    if not scalar_q:
        p.out_prefix = (nq,)
    return result.to(_torch_dtype(p.out_dtype)), _FINISHED, None


def _family_quantile_cols(p, eng):
    """Quantiles over leading dims, sorted in LDS: (nq, ngroups, M) from one
    read of the (N, lead_M) view; the kernel's non-NaN counts stand in for
    the SET_COUNT pass of the min_count rule. With a group too long to sort
    in LDS (p.cols_select) the radix-select kernel gives the same."""
    from .aggregate_hip import grouped_quantile_cols, grouped_quantile_select_cols

    q_arr, scalar_q = _quantile_q(p)
    vt, scodes, perm = p.cols
    want = p.min_count_ > 0
    if p.cols_select:
        r = grouped_quantile_select_cols(
            vt, scodes, perm, p.ngroups, q_arr, skipnan=p.agg.skipnan, want_count=want,
        )
    else:
        r = grouped_quantile_cols(
            vt, scodes, perm, p.ngroups, q_arr, skipnan=p.agg.skipnan,
            max_seg_rows=p.cols_sorted_rows, want_count=want,
        )
    resq, counts = r if want else (r, None)
    return _quantile_finish(p, resq, scalar_q, len(q_arr), lambda: counts)


def _family_mode_cols(p, eng):
    """Mode over leading dims, sorted in LDS; the counts _family_mode takes
    from a SET_COUNT pass come from the same kernel."""
    from .aggregate_hip import grouped_mode_cols

    vt, scodes, perm = p.cols
    result, counts = grouped_mode_cols(
        vt, scodes, perm, p.ngroups, skipnan=p.agg.skipnan,
        max_seg_rows=p.cols_sorted_rows, want_count=True,
    )
    empty_mask = (
        torch.zeros_like(counts, dtype=torch.bool)
        if p.arr.dtype.is_floating_point
        else counts == 0
    )
    return result, empty_mask, counts


def _family_quantile(p, eng):
    from .aggregate_hip import grouped_quantile

    vals, ngroups = p.vals, p.ngroups
    q_arr, scalar_q = _quantile_q(p)
    if vals.numel() == 0 and not p.dist_on:
        resq = torch.full((len(q_arr), ngroups), float("nan"), dtype=torch.float64, device=p.device)
    elif p.dist_on:
        # exact cross-rank quantiles by radix selection over grouped
        # counts — histograms cross the wire, values never do
        from .dist_quantile import distributed_grouped_quantile

        codes = _bounded_codes(p.labels, p.labels2, p.grp_pair, ngroups, check_single=False)
        resq = distributed_grouped_quantile(vals, codes, ngroups, q_arr, skipnan=p.agg.skipnan)
    else:
        resq = grouped_quantile(
            vals, p.labels, ngroups, q_arr, skipnan=p.agg.skipnan,
            labels2=p.labels2, grp_shape=p.grp_pair,
        )
    return _quantile_finish(p, resq, scalar_q, len(q_arr), eng.count)


def _family_mode(p, eng):
    from .aggregate_hip import grouped_mode

    vals, ngroups = p.vals, p.ngroups
    if p.dist_on:
        # exact cross-rank mode: run-length-encoded (group, value, count)
        # runs are all_gathered and merged on every rank
        from .dist_quantile import distributed_grouped_mode

        codes = _bounded_codes(p.labels, p.labels2, p.grp_pair, ngroups, check_single=False)
        result = distributed_grouped_mode(vals, codes, ngroups, p.agg.skipnan)
    elif vals.numel() == 0:
        empty = float("nan") if vals.is_floating_point() else 0
        result = torch.full((ngroups,), empty, dtype=vals.dtype, device=p.device)
    else:
        result = grouped_mode(
            vals, p.labels, ngroups, skipnan=p.agg.skipnan,
            labels2=p.labels2, grp_shape=p.grp_pair,
        )
    counts = eng.count()
    # float results carry NaN for empty/propagated groups already;
    # integer results need the empty fill
    empty_mask = (
        torch.zeros_like(counts, dtype=torch.bool)
        if p.arr.dtype.is_floating_point
        else counts == 0
    )
    return result, empty_mask, counts


def _family_arg(p, eng):
    func, vals, labels, ngroups = p.func, p.vals, p.labels, p.ngroups
    device, dist_on, shard_row_offset = p.device, p.dist_on, p.shard_row_offset
    skip = p.agg.skipnan
    ismax = "max" in func
    base_ok = (
        ngroups > PACKED_ARG_THRESHOLD
        and shard_row_offset + vals.numel() < (1 << 32)
    )
    # huge group counts, 4-byte dtypes: pack (order-preserving 32-bit
    # value encoding, row index) into one int64 key and take a single
    # grouped MIN — the partition path then handles what the 20 B/group
    # IDX bins cannot (LDS holds ~8e3 of them). Ties break to the
    # smaller row, which is exactly np.argmin/argmax's first-occurrence
    # rule. Distributed: the packed key is lexicographic (value, row),
    # so ONE min all-reduce of the key bins is the exact global answer.
    packed_ok = (
        base_ok
        and vals.dtype in (torch.float32, torch.int32)
        and (0 < vals.numel() or dist_on)
    )
    # 8-byte dtypes: no room to pack — the partition pairs carry the
    # row in their spare pad word and a second bucket pass takes the
    # min row among rows matching the group extremum (FH_SET_ARG*_PAIR)
    pair_ok = (
        base_ok
        and not dist_on
        and vals.dtype in (torch.float64, torch.int64)
        and 0 < vals.numel() < (1 << 31)
        and ngroups <= (1 << 24)
        # pair-arg rides the partition path, whose overflow check
        # host-syncs: under hipGraph capture use the two-pass form
        and not (vals.is_cuda and torch.cuda.is_current_stream_capturing())
    )
    if dist_on and distributed.is_active():
        # the branch choice must agree across ranks (shard sizes differ)
        okt = torch.tensor([1 if packed_ok else 0], dtype=torch.int32, device=device)
        distributed.all_reduce_(okt, "min")
        packed_ok = bool(okt.item())
    if packed_ok:
        lib = _ffi.load_library()
        key = torch.empty(vals.numel(), dtype=torch.int64, device=device)
        vc = vals.contiguous()
        if vc.numel():  # a zero-row dist rank still joins the collectives
            _ffi.check(lib.fh_pack_argkeys(
                vc.data_ptr(),
                _ffi.F32 if vals.dtype == torch.float32 else _ffi.I32,
                vc.numel(), shard_row_offset, int(ismax), int(skip),
                key.data_ptr(),
                torch.cuda.current_stream(device).cuda_stream,
            ))
            vc.record_stream(torch.cuda.current_stream(device))
        pk = grouped_partials(
            _ffi.SET_MIN_COUNT, key, labels, ngroups,
            skipnan=False, labels2=p.labels2, grp_shape=p.grp_pair,
        )
        if dist_on:
            distributed.all_reduce_(pk["min"], "min")
            distributed.all_reduce_(pk["count"], "sum")
        kmin = pk["min"]
        empty_mask = kmin == _I64_MAX
        result = (kmin ^ (-(1 << 63))) & 0xFFFFFFFF
        counts_for_mask = pk["count"]
        if p.min_count_ > 0 and skip:
            # the packed keys are always-valid ints, so pk["count"]
            # counts NaN rows too; nanarg min_count masks on the
            # NaN-aware count
            counts_for_mask = eng.count()
    elif pair_ok:
        pp = grouped_partials(
            _ffi.SET_ARGMAX_PAIR if ismax else _ffi.SET_ARGMIN_PAIR,
            vals, labels, ngroups, skipnan=skip,
            labels2=p.labels2, grp_shape=p.grp_pair,
            row_offset=shard_row_offset,
        )
        result = pp["idx"]
        empty_mask = result == _I64_MAX
        counts_for_mask = pp["count"]
    else:
        # pass 1: the per-group extremum; pass 2: the smallest row index
        # whose value matches it (ties -> first occurrence, like
        # np.argmax; a NaN target matches NaN rows, so non-skip arg*
        # land on the first NaN)
        ext = "max" if ismax else "min"
        if skip:
            p1 = eng.run(_ffi.SET_MAX_COUNT if ismax else _ffi.SET_MIN_COUNT, True)
        else:
            p1 = eng.run(_ffi.SET_MAX_FULL if ismax else _ffi.SET_MIN_FULL, False)
        if dist_on:
            distributed.all_reduce_(p1[ext], ext)
            distributed.all_reduce_(p1["count"], "sum")
            if "nanflag" in p1:
                distributed.all_reduce_(p1["nanflag"], "max")
        target = p1[ext]
        if "nanflag" in p1 and p.arr.dtype.is_floating_point:
            target = torch.where(p1["nanflag"] != 0, torch.full_like(target, float("nan")), target)
        p2 = eng.run(_ffi.SET_IDXMIN, skip, target=target)
        if dist_on:
            # present/count are rank-local (the kernel marks presence
            # only for rows this rank holds): combine them too, or a
            # rank with no rows of a group would fill -1 while others
            # return the index
            distributed.all_reduce_(p2["idx"], "min")
            distributed.all_reduce_(p2["present"], "max")
            distributed.all_reduce_(p2["count"], "sum")
        result = p2["idx"]
        empty_mask = (p2["present"] == 0) | (result == _I64_MAX)
        counts_for_mask = p2["count"]
    if p.lead_folded:
        # composite-group indices are flat (lead*N + t); the API returns the
        # index within the reduced trailing axes (t), like np.argmax(axis=-1)
        offs = (
            torch.arange(p.lead_M, device=device, dtype=torch.int64) * p.arg_localize_N
        ).repeat_interleave(p.base_ngroups)
        result = result - offs  # empty slots are overwritten by the fill
    return result, empty_mask, counts_for_mask


def _family_first_last_packed(p, eng):
    """Huge group counts: first/last is a grouped MIN/MAX over the row
    indices themselves (any value dtype), so the partition path applies
    where the 20 B/group IDX bins cannot; NaN rows take the opposite extreme
    under nan* so all-NaN groups land on the empty sentinel."""
    vals = p.vals
    isfirst = p.func in ("first", "nanfirst")
    rows_key = torch.arange(vals.numel(), device=p.device, dtype=torch.int64) + p.shard_row_offset
    if p.agg.skipnan and vals.is_floating_point():
        bad_v = _I64_MAX if isfirst else -1
        rows_key = torch.where(torch.isnan(vals), torch.full_like(rows_key, bad_v), rows_key)
    pk = grouped_partials(
        _ffi.SET_MIN_COUNT if isfirst else _ffi.SET_MAX_COUNT,
        rows_key, p.labels, p.ngroups,
        skipnan=False, labels2=p.labels2, grp_shape=p.grp_pair,
    )
    idx = pk["min"] if isfirst else pk["max"]
    valid = (idx != _I64_MAX) if isfirst else (idx >= 0)
    local = idx - p.shard_row_offset
    safe = torch.clamp(local, 0, max(vals.numel() - 1, 0))
    result = vals[safe]
    empty_mask = ~valid
    if p.min_count_ > 0:
        counts_for_mask = eng.count(skipnan=p.agg.skipnan)
    else:
        counts_for_mask = torch.where(valid, torch.ones_like(idx), torch.zeros_like(idx))
    return result, empty_mask, counts_for_mask


def _family_first_last(p, eng):
    vals, device = p.vals, p.device
    pp = eng.run(p.agg.op_set, p.agg.skipnan)
    if p.dist_on:
        distributed.combine_partials(pp, p.agg.combine)
    idx = pp["idx"]
    sentinel = _I64_MAX if p.func in ("first", "nanfirst") else -1
    valid = idx != sentinel
    local = idx - p.shard_row_offset
    n_local = vals.numel()
    safe = torch.clamp(local, 0, max(n_local - 1, 0))
    if p.dist_on:
        # the owning rank contributes the value; others contribute exact 0
        owner = valid & (local >= 0) & (local < n_local)
        gathered = torch.where(owner, vals[safe], torch.zeros((), dtype=vals.dtype, device=device))
        distributed.all_reduce_(gathered, "sum")
    elif n_local == 0:
        # no rows: every group is empty and takes the fill
        gathered = torch.zeros(idx.shape, dtype=vals.dtype, device=device)
    else:
        gathered = vals[safe]
    return gathered, ~valid, pp["count"]


def _family_arg_cols(p, eng):
    """Arg-reductions over leading dims: one SET_ARG*_COLS pass keeps the
    running extremum and its row per (group, column). The row is already the
    index within the reduced axes, so nothing is subtracted; the triple is
    the one _family_arg's two-pass form hands the finalize."""
    op_set = _ffi.SET_ARGMAX_COLS if "max" in p.func else _ffi.SET_ARGMIN_COLS
    pp = eng.run(op_set, p.agg.skipnan)
    result = pp["idx"]
    empty_mask = (pp["present"] == 0) | (result == _I64_MAX)
    return result, empty_mask, pp["count"]


def _family_first_last_cols(p, eng):
    """first/last over leading dims: the column form of the func's index set,
    then a gather from the (N, lead_M) view the kernel read."""
    vt = p.cols[0]
    pp = eng.run(p.agg.op_set, p.agg.skipnan)
    idx = pp["idx"]
    sentinel = _I64_MAX if p.func in ("first", "nanfirst") else -1
    valid = idx != sentinel
    safe = torch.clamp(idx, 0, vt.shape[0] - 1)
    return torch.gather(vt, 0, safe), ~valid, pp["count"]


def _var_from_ssd(p, ssd, counts):
    den = counts.to(torch.float64) - p.ddof
    result = ssd / den
    nan_t = torch.full_like(result, float("nan"))
    result = torch.where((den < 0) | (counts == 0), nan_t, result)
    if p.func in ("std", "nanstd"):
        result = torch.sqrt(result)
    return result


def _family_var_cols(p, eng):
    """Single fused pass on the column path: the kernel accumulates
    mean-shifted sums per (group, column) segment and emits the var_chunk
    triple (ssd, sum, count); cross-rank combine closes the reference's
    _var_combine adjustment in one formula."""
    pw = eng.run(_ffi.SET_WELFORD, p.agg.skipnan)
    ssd, sums, counts = pw["wssd"], pw["wsum"], pw["count"]
    if p.dist_on:
        t = torch.where(counts > 0, sums * sums / counts, torch.zeros_like(sums))
        a = ssd + t
        distributed.all_reduce_sum_many([a, sums, counts])
        ssd = a - torch.where(counts > 0, sums * sums / counts, torch.zeros_like(sums))
    return _var_from_ssd(p, ssd, counts), counts == 0, counts


def _family_var(p, eng):
    skip = p.agg.skipnan
    p1 = eng.run(_ffi.SET_SUM_COUNT, skip)
    if p.dist_on:
        distributed.all_reduce_sum_many([p1["sum"], p1["count"]])
    counts = p1["count"]
    # deviations about the (global) per-group mean: the cross-rank ssd
    # combine is then a plain sum (the reference's _var_combine,
    # aggregations.py:392-451, with zero adjustment terms)
    means = (p1["sum"].to(torch.float64) / counts).contiguous()
    p2 = eng.run(_ffi.SET_SSD, skip, means=means)
    if p.dist_on:
        distributed.all_reduce_(p2["sum"], "sum")
    return _var_from_ssd(p, p2["sum"], counts), None, counts


def _family_simple(p, eng):
    """count, sum/prod, mean, min/max, any/all: one pass of the func's own
    op set; mean/sum/count ask the combine kernel to finish where it can."""
    func, agg = p.func, p.agg
    fin = None
    if FUSED_FINALIZE and p.lead_M == 1 and not p.dist_on and p.ngroups > 0 and not p.many_served:
        fin = _fused_finish(func, agg.op_set, p.vals.dtype, p.out_dtype, p.min_count_, p.fill_value)
    pp = eng.run(agg.op_set, agg.skipnan, finish=fin)
    if p.dist_on:
        distributed.combine_partials(pp, agg.combine)
    if "result" in pp:
        # the combine kernel already divided, masked, filled and cast
        return pp["result"], _FINISHED, None
    counts = pp["count"]
    if func == "count":
        return counts, counts == 0, counts
    if func in ("sum", "nansum", "prod", "nanprod"):
        return pp["sum"], pp["present"] == 0, counts
    if func in ("mean", "nanmean"):
        return pp["sum"].to(torch.float64) / counts, None, counts
    if func in ("min", "nanmin", "max", "nanmax"):
        result = pp["min" if "min" in pp else "max"]
        if "nanflag" in pp and p.arr.dtype.is_floating_point:
            nan_t = torch.full_like(result, float("nan"))
            result = torch.where(pp["nanflag"] != 0, nan_t, result)
        empty_mask = (pp["present"] == 0) if "present" in pp else (counts == 0)
        return result, empty_mask, counts
    if func in ("any", "all"):
        if not p.inp.was_bool:
            raise NotImplementedError("any/all support bool input only")
        return pp["max" if func == "any" else "min"] == 1, counts == 0, counts
    raise NotImplementedError(func)  # pragma: no cover


def _select_family(p):
    func = p.func
    if func in _QUANTILE_FUNCS:
        return _family_quantile if p.cols_sorted_rows is None else _family_quantile_cols
    if func in ("mode", "nanmode"):
        return _family_mode if p.cols_sorted_rows is None else _family_mode_cols
    if p.cols_order:
        return _family_arg_cols if func in _ARG_FUNCS else _family_first_last_cols
    if func in _ARG_FUNCS:
        return _family_arg
    if func in _FIRST_LAST_FUNCS:
        packed_ok = (
            p.ngroups > PACKED_ARG_THRESHOLD
            and not p.dist_on
            and 0 < p.vals.numel()
            and p.shard_row_offset + p.vals.numel() < (1 << 32)
        )
        return _family_first_last_packed if packed_ok else _family_first_last
    if func in _VAR_FUNCS:
        return _family_var_cols if p.lead_M > 1 else _family_var
    return _family_simple


def _finalize_fill(p, result, empty_mask, counts_for_mask):
    """Masking + fills + final dtype (reference core.py:410-475). Fills are
    applied with an unconditional where (no host sync); the one case that
    must inspect the mask on the host is a NaN fill on an integer result,
    which promotes the output dtype (reference core.py:446-449
    maybe_promote)."""
    func, fill_value, device = p.func, p.fill_value, p.device
    t_out_dtype = _torch_dtype(p.out_dtype)
    is_float_out = torch.empty(0, dtype=t_out_dtype).is_floating_point()
    if p.min_count_ > 0:
        fv, mask = fill_value, counts_for_mask < p.min_count_
    else:
        fv = fill_value if fill_value is not None else xrdtypes.fill_default(func, p.out_dtype)
        if isinstance(fv, float) and math.isnan(fv) and func in ("mean", "nanmean") + _VAR_FUNCS:
            # 0/0 division already produced NaN exactly where the fill goes
            return result.to(t_out_dtype)
        mask = empty_mask if empty_mask is not None else counts_for_mask == 0
    nan_fv = isinstance(fv, float) and math.isnan(fv)
    if fv is None or (nan_fv and not is_float_out):
        if bool(mask.any().item()):
            if fv is None:
                raise ValueError("Filling is required but fill_value is None.")
            t_out_dtype = torch.float64
            result = result.to(t_out_dtype)
            result = torch.where(mask, torch.tensor(fv, dtype=t_out_dtype, device=device), result)
    else:
        result = result.to(t_out_dtype)
        result = torch.where(mask, _fill_scalar(fv, t_out_dtype, device, result), result)
    return result.to(t_out_dtype)


def _shape_and_order(p, result):
    """Flat bins -> (q..., lead..., kept by dims..., group dims...), and the
    groups; under sort=False without expected_groups both in
    first-appearance order."""
    many = p.many
    if p.lead_M > 1 and not p.lead_folded:
        # column partials are (q..., ngroups, M) group-major; the API result
        # puts the group dims last
        result = result.reshape(
            p.out_prefix + (p.ngroups, p.lead_M)
        ).transpose(-1, -2).contiguous()
    result = result.reshape(
        p.out_prefix + p.lead_shape + (p.subset_keep_shape or ()) + p.grp_shape
    )
    groups_list = [f.groups for f in p.facs]
    if not p.sort and not p.provided_expected:
        # groups in first-appearance order (reference pd.factorize(sort=False),
        # factorize.py:96): find each group's first row with an index-min pass
        # and permute the result bins — rows need no relabeling; the group
        # dims are always the trailing len(facs) axes of the result
        for ax_i, f in enumerate(p.facs):
            if many is not None and ax_i in many.orders:
                order, order_np = many.orders[ax_i]
            else:
                fcodes = f.codes
                if p.subset_keep_shape is not None:
                    # restore the original by layout before taking first rows
                    fcodes = fcodes.reshape(p.by_shape).permute(p.subset_by_inv).reshape(-1).contiguous()
                pidx = grouped_partials(_ffi.SET_IDXMIN, fcodes.to(torch.int64), fcodes, f.ngroups)
                order = torch.argsort(pidx["idx"], stable=True)
                order_np = order.cpu().numpy()
                if many is not None:
                    many.orders[ax_i] = (order, order_np)
            result = torch.index_select(result, result.dim() - len(p.facs) + ax_i, order)
            groups_list[ax_i] = np.asarray(groups_list[ax_i])[order_np]
    return result, tuple(groups_list)


def _to_caller(p, result):
    """The result in the caller's array type and, where the func preserves
    it, the caller's dtype."""
    func, inp = p.func, p.inp
    if inp.return_numpy:
        out_np = result.cpu().numpy()
        if inp.dt_dtype is not None and func not in ("count", "any", "all"):
            # the reference casts every non-count result back to the datetime
            # dtype (core.py:1209-1211): int64 counts reinterpret, float
            # results truncate, NaN -> NaT
            out_np = out_np.astype(inp.dt_dtype)
        return _cast_back_small(out_np, func, inp.small_dtype, inp.user_fill_value)
    if inp.small_dtype is not None and func in _PRESERVE_SMALL:
        # torch outputs for torch small-dtype inputs: preserve-funcs cast
        # back (torch has these dtypes); sums stay in the promoted
        # accumulator dtype (torch has no uint64) - documented
        back = _TORCH_SMALL_BACK.get(np.dtype(inp.small_dtype))
        if back is not None:
            result = result.to(back)
    return result


def _reduce(many, array, by, func, kw):
    """One grouped reduction, stage by stage. `many` is the _ManyCall of the
    enclosing groupby_reduce_many (shared factorization, summary partials
    and group order), or None; `kw` holds groupby_reduce's keywords."""
    if isinstance(func, Aggregation):
        func = func.name  # reference accepts Aggregation instances (core.py:934-948)
    if kw["engine"] != "hip":
        raise ValueError(f"flox_amd implements engine='hip' only (got {kw['engine']!r})")
    if func not in REDUCTIONS:
        raise NotImplementedError(f"reduction {func!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("flox_amd.groupby_reduce requires a GPU (engine='hip')")
    device = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(array, torch.Tensor):
        array = np.asarray(array)
        if array.dtype.kind == "c":
            return _reduce_complex(array, by, func, kw)

    p = _Plan()
    p.func, p.agg, p.device, p.sort = func, REDUCTIONS[func], device, kw["sort"]
    p.many, p.out_prefix = many, ()
    p.finalize_kwargs = kw["finalize_kwargs"]
    p.ddof = (p.finalize_kwargs or {}).get("ddof", 0)
    p.shard_row_offset = kw["shard_row_offset"]

    arr, p.inp = _normalize_input(array, func, kw["fill_value"], device)
    (p.bys, by_dts, p.by_shape, p.arr, p.subset_keep_shape, p.subset_by_inv,
     p.lead_shape, p.lead_M) = _align_by(arr, by, kw["axis"], device)
    expected_groups, isbins, p.provided_expected = _group_spec(
        kw["expected_groups"], kw["isbin"], len(p.bys)
    )
    p.facs = many.facs if many is not None else None
    if p.facs is None:
        p.facs = _factorize(p.bys, expected_groups, isbins, by_dts, p.sort, device)
        if many is not None:
            many.facs = p.facs
    _build_codes(p)
    _resolve_fill(p, kw["dtype"], kw["min_count"])

    dc = kw["distributed_combine"]
    p.dist_on = distributed.is_active() if dc is None else dc
    if p.dist_on and any(e is None for e in expected_groups):
        # rank-local factorization (torch.unique of the local shard) yields
        # per-rank code spaces: the all-reduced bins would be misaligned.
        # The reference's dask path has the same constraint (its combine
        # tree reindexes every block to the full expected_groups vector,
        # dask.py:90-144); discovering groups globally needs a set-union
        # collective that is not built — require expected_groups instead.
        raise NotImplementedError(
            "distributed_combine requires expected_groups for every `by` "
            "(rank-local group discovery would misalign the combined bins)"
        )

    eng = _select_engine(p, by)
    result, empty_mask, counts_for_mask = _select_family(p)(p, eng)
    if empty_mask is not _FINISHED:
        result = _finalize_fill(p, result, empty_mask, counts_for_mask)
    result, groups = _shape_and_order(p, result)
    return (_to_caller(p, result), *groups)


def groupby_reduce(
    array, *by, func: str, expected_groups=None, sort: bool = True, isbin=False,
    axis=None, fill_value=None, dtype=None, min_count: int | None = None,
    method: str | None = None, engine: str = "hip", reindex=None,
    finalize_kwargs: dict[str, Any] | None = None,
    distributed_combine: bool | None = None, shard_row_offset: int = 0,
):
    """Grouped reduction with flox semantics on MI355X. Returns (result, *groups).

    ``array``/``by``: numpy arrays or torch tensors (numpy is moved to the
    GPU; note the PCIe cost — keep tensors resident for performance).
    ``distributed_combine``: all-reduce the per-group partials across the
    initialized torch.distributed world (default: auto when initialized).
    Each rank passes its own row shard; results are full-group on every rank.
    """
    kw = dict(
        expected_groups=expected_groups, sort=sort, isbin=isbin, axis=axis,
        fill_value=fill_value, dtype=dtype, min_count=min_count, method=method,
        engine=engine, reindex=reindex, finalize_kwargs=finalize_kwargs,
        distributed_combine=distributed_combine, shard_row_offset=shard_row_offset,
    )
    if isinstance(func, CustomAggregation):
        return _reduce_custom(array, by, func, kw)
    return _reduce(None, array, by, func, kw)


_PER_FUNC_ARGS = ("fill_value", "dtype", "min_count", "finalize_kwargs")


def _per_func(name, value, funcs):
    """Resolve one of the per-func arguments of groupby_reduce_many: a dict
    keyed by func name (missing key = the argument's default, None), or one
    value for every func. finalize_kwargs is itself a dict, so it counts as
    keyed by func only when all its values are dicts (or None)."""
    keyed = isinstance(value, dict)
    if keyed and name == "finalize_kwargs":
        keyed = len(value) > 0 and all(v is None or isinstance(v, dict) for v in value.values())
    if not keyed:
        return {f: value for f in funcs}
    extra = [k for k in value if k not in funcs]
    if extra:
        raise ValueError(f"{name} has keys that are not in funcs: {extra}")
    return {f: value.get(f) for f in funcs}


def groupby_reduce_many(
    array, *by, funcs, expected_groups=None, sort: bool = True, isbin=False,
    axis=None, fill_value=None, dtype=None, min_count=None,
    method: str | None = None, engine: str = "hip", reindex=None,
    finalize_kwargs=None, distributed_combine: bool | None = None,
    shard_row_offset: int = 0,
):
    """Several grouped reductions of one array over the same labels.
    Returns (results, *groups): results maps each name in ``funcs`` (in that
    order) to what ``groupby_reduce(array, *by, func=name, ...)`` returns.

    ``fill_value``, ``dtype``, ``min_count`` and ``finalize_kwargs`` take one
    value for all funcs or a dict keyed by func name (see _per_func).

    The labels are factorized once. When at least two names belong to
    FUSED_MANY_FUNCS (the sum/mean/var/std/min/max/count family and its nan*
    twins) and the call is a non-distributed 1-D reduction of real
    f32/f64/i32/i64 values whose bins fit LDS, those names share ONE pass
    over the rows (SET_SUMMARY); every other name, and every name of a call
    that is not eligible, runs its usual passes. ``set_options(fused_many=
    False)`` turns the sharing off. Results do not depend on which way a
    name was served beyond float rounding of sum/mean/var/std.
    """
    if isinstance(funcs, str):
        funcs = (funcs,) if funcs else ()
    funcs = tuple(funcs)
    if not funcs:
        raise ValueError("funcs must name at least one reduction")
    for f in funcs:
        if not isinstance(f, str) or f not in REDUCTIONS:
            raise NotImplementedError(f"reduction {f!r}")
    if len(set(funcs)) != len(funcs):
        dup = sorted({f for f in funcs if funcs.count(f) > 1})
        raise ValueError(f"funcs lists a reduction more than once: {dup}")
    per = {
        k: _per_func(k, v, funcs)
        for k, v in zip(_PER_FUNC_ARGS, (fill_value, dtype, min_count, finalize_kwargs))
    }

    is_complex = (
        array.is_complex() if isinstance(array, torch.Tensor)
        else np.asarray(array).dtype.kind == "c"
    )
    # complex input re-enters groupby_reduce on views: nothing to share
    share = FUSED_MANY and not is_complex and sum(f in FUSED_MANY_FUNCS for f in funcs) >= 2
    results, groups = {}, ()
    state = _ManyCall() if share else None
    common = dict(
        expected_groups=expected_groups, sort=sort, isbin=isbin, axis=axis,
        method=method, engine=engine, reindex=reindex,
        distributed_combine=distributed_combine, shard_row_offset=shard_row_offset,
    )
    for f in funcs:
        kw = {**common, **{k: per[k][f] for k in _PER_FUNC_ARGS}}
        results[f], *groups = _reduce(state, array, by, f, kw)
    if state is not None and state.partials is not None:
        # a result that needed no fill and no cast can be a partial
        # itself: hand out copies, so no two results share storage
        shared = {t.data_ptr() for t in state.partials.values()
                  if isinstance(t, torch.Tensor)}
        for f, r in results.items():
            if isinstance(r, torch.Tensor) and r.data_ptr() in shared:
                results[f] = r.clone()
    return (results, *groups)
