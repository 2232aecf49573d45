"""groupby_scan: grouped scans with flox semantics on MI355X.

Mirrors the reference's eager scan path (flox/scan.py:101-352 groupby_scan
-> chunk_scan -> aggregate_flox._np_grouped_scan / ffill,
aggregate_flox.py:269-325): cumulative sums and forward/backward fills
within each group, in the original row order, over the trailing axis.
"""

from __future__ import annotations

import builtins
import ctypes

import numpy as np
import torch

from . import _ffi, distributed
from ._ffi import FhCall
from .core import _as_device_tensor, _combined_codes, _factorize_device

SCAN_OPS = {"cumsum": 0, "nancumsum": 1, "ffill": 2, "bfill": 3}


def groupby_scan(
    array, *by, func: str, expected_groups=None, axis=None, dtype=None,
    distributed_combine: bool | None = None,
):
    """Grouped scan. Returns an array shaped like ``array``.

    cumsum/nancumsum: per-group running sum in row order (np.cumsum /
    np.nancumsum semantics, incl. integer promotion to the platform int).
    ffill/bfill: carry the last/next non-NaN value within the group.
    Rows with labels outside ``expected_groups`` scan as their own group
    (the reference's NaN-sentinel group, factorize.py:201-210).
    """
    if func not in SCAN_OPS:
        raise NotImplementedError(f"scan {func!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("flox_amd.groupby_scan requires a GPU (engine='hip')")
    # reference scan.py:286-291 ("avoid some roundoff error when we can"):
    # a length-1 trailing axis, or a 1-D by where every observed row is its
    # own group, returns the INPUT unchanged cast to the scan output dtype.
    # Semantically this differs from the computed scan only for nancumsum of
    # NaN rows (NaN stays NaN instead of the identity 0), so only that func
    # needs the quirk mirrored; mirrored only under the reference's own
    # precondition (its scans reject expected_groups). Found by the
    # oracle-vs-reference fuzz, seed 606162.
    if func == "nancumsum" and expected_groups is None and len(by) == 1:
        b0 = by[0]
        bt = b0 if isinstance(b0, torch.Tensor) else None
        bn = None if bt is not None else np.asarray(b0)
        shape = tuple(bt.shape) if bt is not None else bn.shape
        hit = len(shape) >= 1 and shape[-1] == 1
        if not hit and len(shape) == 1:
            # all-distinct, non-null labels <=> n == observed group count
            n_rows = shape[0]
            if bt is not None:
                bb = bt[~torch.isnan(bt)] if bt.is_floating_point() else bt
                hit = int(torch.unique(bb).numel()) == n_rows
            else:
                if bn.dtype.kind == "f":
                    bb = bn[~np.isnan(bn)]
                elif bn.dtype.kind in "Mm":
                    bb = bn[~np.isnat(bn)]
                else:
                    bb = bn
                hit = np.unique(bb).size == n_rows
        if hit:
            if isinstance(array, torch.Tensor):
                out_t = array.clone()
                if out_t.dtype == torch.bool:
                    out_t = out_t.to(torch.int64)
                elif out_t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32):
                    out_t = out_t.to(torch.int64)
                if dtype is not None:
                    out_t = out_t.to(dtype)
                return out_t
            out_n = np.asarray(array).copy()
            if out_n.dtype.kind == "b":
                out_n = out_n.astype(np.int64)
            elif out_n.dtype.kind in "iu" and out_n.dtype.itemsize < 8:
                out_n = out_n.astype(np.uint64 if out_n.dtype.kind == "u" else np.int64)
            if dtype is not None:
                out_n = out_n.astype(dtype)
            return out_n
    device = torch.device("cuda", torch.cuda.current_device())
    return_numpy = not isinstance(array, torch.Tensor)
    # datetime64/timedelta64 scan on the int64 view, NaT (= int64 min)
    # passing through as a plain value — the reference's behavior (its ffill
    # isnull sees no missing values on the int64 view)
    dt_dtype = None
    small_dtype = None
    if return_numpy:
        arr_np0 = np.asarray(array)
        from .core import _SMALL_PROMOTE, _cast_back_small, _coerce_by

        if arr_np0.dtype.kind == "c":
            # complex scans: componentwise on the (2, ...) re/im view;
            # skipna whole-value nulls premask both components (either
            # component NaN is null per the reference's isnull)
            comp_dt = arr_np0.dtype
            if func in ("ffill", "bfill"):
                # reference quirk: its dtype gate (scan.py:199) routes
                # non-float kinds to the identity scan — complex ffill is
                # a no-op
                return arr_np0.copy()
            fwidth = np.float64 if comp_dt == np.dtype(np.complex128) else np.float32
            fv2 = arr_np0.view(fwidth).reshape(arr_np0.shape + (2,)).copy()
            if func == "nancumsum":
                fv2[np.isnan(arr_np0)] = np.nan
            comps = np.moveaxis(fv2, -1, 0)
            r = groupby_scan(
                np.ascontiguousarray(comps), *by, func=func,
                expected_groups=expected_groups, axis=None, dtype=None,
                distributed_combine=distributed_combine,
            )
            out = np.asarray(r)
            return (out[0] + 1j * out[1]).astype(
                comp_dt if dtype is None else np.dtype(dtype)
            )
        if arr_np0.dtype in _SMALL_PROMOTE:
            small_dtype = arr_np0.dtype
            array = arr_np0.astype(_SMALL_PROMOTE[arr_np0.dtype])
            arr_np0 = np.asarray(array)
        elif arr_np0.dtype == np.uint64:
            # int64 view: cumsum wrap-exact mod 2^64; ffill/bfill identity
            small_dtype = arr_np0.dtype
            array = arr_np0.view(np.int64)
            arr_np0 = np.asarray(array)
        if arr_np0.dtype.kind in "Mm":
            dt_dtype = arr_np0.dtype
            array = arr_np0.view("i8")
    else:
        from .core import _cast_back_small, _coerce_by
    arr = _as_device_tensor(array, device)
    by_dts = []
    _coerced = []
    for b in by:
        if not isinstance(b, torch.Tensor):
            bn = np.asarray(b)
            if bn.dtype.kind in "Mm":
                by_dts.append(bn.dtype)
                _coerced.append(bn.view("i8"))
                continue
            if bn.dtype.kind in "US" or bn.dtype == object:
                by_dts.append(None)
                _coerced.append(bn)  # host-factorized at the facs stage
                continue
        by_dts.append(None)
        _coerced.append(_coerce_by(b))
    bys = tuple(
        b if isinstance(b, np.ndarray) and (b.dtype.kind in "US" or b.dtype == object)
        else _as_device_tensor(b, device)
        for b in _coerced
    )
    if len(bys) == 0:
        raise ValueError("need at least one by array")
    by_shape = bys[0].shape
    if tuple(arr.shape[arr.ndim - len(by_shape):]) != tuple(by_shape):
        raise ValueError("by must align with trailing dims of array")
    lead_M = 1
    for d in arr.shape[: arr.ndim - len(by_shape)]:
        lead_M *= d
    if axis is not None:
        ax = axis if isinstance(axis, (tuple, list)) else (axis,)
        ax = tuple(a % arr.ndim for a in ax)
        if tuple(sorted(ax)) != tuple(range(arr.ndim - len(by_shape), arr.ndim)):
            raise NotImplementedError("scan over an axis subset: next row")

    orig_shape = arr.shape
    if arr.numel() == 0:
        out0 = torch.empty_like(arr.reshape(-1)).reshape(orig_shape)
        if return_numpy:
            o = out0.cpu().numpy()
            return o.astype(dt_dtype) if dt_dtype is not None else o
        return out0
    # integer promotion like np.cumsum (sub-platform ints accumulate in intp);
    # done on the array as laid out (.to keeps a permute view's strides), the
    # flattening is left to whichever path runs
    if func in ("cumsum", "nancumsum") and arr.dtype in (torch.int32, torch.bool):
        arr = arr.to(torch.int64)
    if arr.dtype == torch.bool:
        arr = arr.to(torch.int64)

    if expected_groups is not None and not isinstance(expected_groups, tuple):
        expected_groups = (expected_groups,)
    if expected_groups is None:
        expected_groups = (None,) * len(bys)
    from .core import _factorize_strings_host

    facs = [
        _factorize_strings_host(b.reshape(-1), e, True, device)
        if isinstance(b, np.ndarray)
        else _factorize_device(b.reshape(-1), e, True, dt_by=dtb)
        for b, e, dtb in zip(bys, expected_groups, by_dts)
    ]
    ngroups = 1
    for f in facs:
        ngroups *= f.ngroups
    labels, labels2, grp_pair = _combined_codes(facs)

    if distributed_combine is None:
        distributed_combine = distributed.is_active()
    out = None
    if lead_M > 1:
        vt = _cols_view(arr, len(by_shape), lead_M)
        if _cols_scan_ok(func, vt, lead_M, dt_dtype,
                         distributed_combine and distributed.is_active()):
            # the column form: no flattened copy, no composite labels, no
            # device-wide sort, no scratch, no limit on N * lead_M. The
            # output takes the view's own strides, so reads and writes are
            # both coalesced.
            from .aggregate_hip import grouped_scan_cols
            from .core import _bounded_codes

            codes_full = _bounded_codes(labels, labels2, grp_pair, ngroups)
            scodes64, perm64 = torch.sort(codes_full, stable=True)
            out_full = torch.empty_like(arr)  # preserve_format: arr's strides
            out_vt = _cols_view(out_full, len(by_shape), lead_M)
            if out_vt is None:
                out_full = None  # a sliced layout, which empty_like densified
            res = grouped_scan_cols(
                vt, scodes64.to(torch.int32), perm64.to(torch.int32), func, out=out_vt
            )
            out = out_full if out_full is not None else (
                res.reshape(tuple(by_shape) + tuple(orig_shape[: arr.ndim - len(by_shape)]))
                .movedim(tuple(range(len(by_shape))),
                         tuple(range(arr.ndim - len(by_shape), arr.ndim)))
            )
    if out is None and lead_M > 1:
        rv = _rows_view(arr, len(by_shape), lead_M)
        if _rows_scan_ok(func, rv, lead_M, ngroups, dt_dtype,
                         distributed_combine and distributed.is_active()):
            # the row form, for the grouped axis last and contiguous: tiles
            # staged through LDS, one lane per lead row, codes in the caller's
            # time order. No copy, no composite labels, no sort, no scratch,
            # no host sync, no limit on N * lead_M.
            from .aggregate_hip import grouped_scan_rows
            from .core import _bounded_codes

            codes = _bounded_codes(labels, labels2, grp_pair, ngroups).to(torch.int32)
            out_full = torch.empty_like(arr)
            out_rv = _rows_view(out_full, len(by_shape), lead_M)
            res = grouped_scan_rows(rv, codes, ngroups, func, out=out_rv)
            out = out_full if out_rv is not None else res.reshape(orig_shape)
    if out is None:
        out = _scan_fold(arr, func, lead_M, labels, labels2, grp_pair, ngroups,
                         distributed_combine, device).reshape(orig_shape)

    if dtype is not None:
        td = torch.from_numpy(np.empty(0, dtype=np.dtype(dtype))).dtype
        out = out.to(td)
    if return_numpy:
        out_np = out.cpu().numpy()
        if dt_dtype is not None:
            out_np = out_np.astype(dt_dtype)  # int64 counts reinterpret
        if small_dtype is not None and dtype is None:
            out_np = _cast_back_small(out_np, func, small_dtype)
        return out_np
    return out


# options.cols_scan: scans over leading dims take the column kernel
# (fh_grouped_scan_cols) where the call is eligible (_cols_scan_ok) instead of
# the lead fold
COLS_SCAN = True
# options.cols_scan_min_cols: the narrowest lead_M that takes it. The grid is
# column tiles x group-aligned chunks, so a narrow array with few long groups
# leaves most of the chip idle and the fold wins there. Measured at 2^26
# elements (profiles/r10_cols_scan.md): with 24 groups the column form wins
# from 1024 columns, with 2 groups it is still 3 % behind at 4096 and 3.3x
# ahead at 16384, the smallest width of the sweep where it loses in neither.
COLS_SCAN_MIN_COLS = 16384


def _cols_view(arr, nbydims, lead_M):
    """The (N, lead_M) view of arr with the grouped dims in front, as
    core._select_engine builds it, or None where it has no unit column stride
    without a copy."""
    N = arr.numel() // lead_M
    arr_t = arr.movedim(tuple(range(arr.ndim - nbydims, arr.ndim)), tuple(range(nbydims)))
    try:
        vt = arr_t.view((N, lead_M))
    except RuntimeError:
        return None
    return vt if vt.stride(1) == 1 else None


def _cols_scan_ok(func, vt, lead_M, dt_dtype, dist_on):
    """Whether a scan over leading dims takes the column form; vt is
    _cols_view's answer. Everything else keeps the lead fold with its results
    and exceptions. The chunk plan reads the sorted codes on the host, which a
    stream under capture cannot."""
    return (
        COLS_SCAN
        and vt is not None
        and lead_M >= COLS_SCAN_MIN_COLS
        and vt.dtype in (
            (torch.float32, torch.float64, torch.int64)
            if func in ("cumsum", "nancumsum") else (torch.float32, torch.float64)
        )
        and not dist_on
        and dt_dtype is None
        and vt.shape[0] > 0
        and vt.shape[0] < 2**31
        and not torch.cuda.is_current_stream_capturing()
        and _ffi.has_scan_cols()
    )


# options.rows_scan: scans over leading dims of an array whose grouped axis is
# last and contiguous (the C-contiguous (lead..., N) layout) take the row
# kernel (fh_grouped_scan_rows) where the call is eligible (_rows_scan_ok)
# instead of the lead fold. The column form is tried first.
ROWS_SCAN = True
# options.rows_scan_min_rows: the fewest lead rows that take it. A workgroup is
# one wave that walks a tile of up to 64 rows, so a short array leaves most of
# the chip idle. Measured at 2^26 elements, f32 and f64, cumsum and ffill, 2
# groups in long runs and 24 cyclic groups (profiles/r12_rows_scan.md): at
# 1024 rows the row form loses everywhere (1.6x to 2.5x the fold's time), at
# 4096 it wins everywhere (0.41 to 0.64 of it), the smallest width of the
# sweep where it loses in neither pattern for either dtype. Never below the
# plan's largest row tile (64).
ROWS_SCAN_MIN_ROWS = 4096


def _rows_view(arr, nbydims, lead_M):
    """The (lead_M, N) view of arr with the grouped dims last, or None where it
    has no unit stride along N and one uniform row stride without a copy. A
    row stride above N (a slice of wider storage) is fine."""
    N = arr.numel() // lead_M
    try:
        rv = arr.view((lead_M, N))
    except RuntimeError:
        return None
    if N > 1 and rv.stride(1) != 1:
        return None
    if lead_M > 1 and rv.stride(0) < N:
        return None
    return rv


def _rows_scan_ok(func, rv, lead_M, ngroups, dt_dtype, dist_on):
    """Whether a scan over leading dims takes the row form; rv is _rows_view's
    answer. The entry makes no host sync, so a capturing stream is no
    obstacle. Everything else keeps the lead fold with its results and
    exceptions."""
    if not (
        ROWS_SCAN
        and rv is not None
        and lead_M > 1
        and lead_M >= ROWS_SCAN_MIN_ROWS
        and rv.dtype in (
            (torch.float32, torch.float64, torch.int64)
            if func in ("cumsum", "nancumsum") else (torch.float32, torch.float64)
        )
        and not dist_on
        and dt_dtype is None
        and 1 <= rv.shape[1] < 2**31
        and _ffi.has_scan_rows()
    ):
        return False
    vd = {torch.float32: _ffi.F32, torch.float64: _ffi.F64, torch.int64: _ffi.I64}[rv.dtype]
    return ngroups <= _ffi.scan_rows_max_groups(vd)


def _scan_fold(arr, func, lead_M, labels, labels2, grp_pair, ngroups,
               distributed_combine, device):
    """The 1-D scan (fh_grouped_scan) over the C-order flattened array, leading
    dims folded into the group codes. Returns the flat result."""
    vals = arr.reshape(-1)
    if lead_M > 1:
        # leading array dims: fold the lead index into the group codes
        # (lead*(ngroups+1) + code, +1 so every column keeps its own
        # NaN-sentinel group) and scan the C-order flattened stream — the
        # offset-labels trick of reference factorize.py:24-39 applied to scans
        if labels2 is not None:
            g0, g1 = grp_pair
            c0, c1 = labels.to(torch.int64), labels2.to(torch.int64)
            bad = (c0 < 0) | (c0 >= g0) | (c1 < 0) | (c1 >= g1)
            base = torch.where(bad, torch.full_like(c0, -1), c0 * g1 + c1)
        else:
            base = labels.to(torch.int64)
        ngs = ngroups + 1
        valid = (base >= 0) & (base < ngroups)
        col = torch.where(valid, base, torch.full_like(base, ngroups))
        lead_idx = torch.arange(lead_M, device=device, dtype=torch.int64)
        labels = (lead_idx[:, None] * ngs + col[None, :]).reshape(-1)
        labels2, grp_pair = None, None
        ngroups = lead_M * ngs

    lib = _ffi.load_library()
    vals = vals.contiguous()
    labels = labels.contiguous()
    if labels.dtype not in (torch.int64, torch.int32):
        labels = labels.to(torch.int64)
    out = torch.empty_like(vals)
    c = FhCall()
    c.vdtype = {torch.float32: _ffi.F32, torch.float64: _ffi.F64,
                torch.int64: _ffi.I64, torch.int32: _ffi.I32}[vals.dtype]
    c.ldtype = _ffi.L_I64 if labels.dtype == torch.int64 else _ffi.L_I32
    c.n = vals.numel()
    c.ngroups = ngroups
    c.values = vals.data_ptr()
    c.labels = labels.data_ptr()
    if labels2 is not None:
        labels2 = labels2.contiguous()
        if labels2.dtype != labels.dtype:
            labels2 = labels2.to(labels.dtype)
        c.labels2 = labels2.data_ptr()
        c.g0, c.g1 = grp_pair
    c.out_sum = out.data_ptr()
    nscratch = lib.fh_scan_scratch_bytes(ctypes.byref(c))
    scratch = torch.empty(builtins.max(int(nscratch), 1), dtype=torch.uint8, device=device)
    c.scratch = scratch.data_ptr()
    c.scratch_bytes = nscratch
    c.stream = torch.cuda.current_stream(device).cuda_stream
    # sorted-labels fast path (the reference's issorted check,
    # aggregate_flox.py:9-23): nondecreasing in-range codes skip the
    # device radix sort entirely — the common time-ordered layout. The probe
    # reads back to the host, which a stream under capture cannot: there the
    # radix sort runs (stable, so the result is the same)
    if labels.numel() > 1 and not torch.cuda.is_current_stream_capturing():
        in_range = bool(
            ((labels >= 0) & (labels < ngroups)).all().item()
        ) if labels2 is None else False
        if in_range and bool((labels[1:] >= labels[:-1]).all().item()):
            c.flags |= _ffi.FLAG_SORTED_LABELS
    _ffi.check(lib.fh_grouped_scan(ctypes.byref(c), SCAN_OPS[func]))
    from .aggregate_hip import _record

    for t in (vals, labels, labels2, scratch, out):
        _record(t, torch.cuda.current_stream(device))

    if distributed_combine and distributed.is_active():
        if labels2 is not None:
            codes = labels.to(torch.int64) * grp_pair[1] + labels2.to(torch.int64)
            codes = torch.where((labels < 0) | (labels2 < 0), torch.full_like(codes, -1), codes)
        else:
            codes = labels.to(torch.int64)
        # rows outside [0, ngroups) are the reference's NaN-sentinel group
        # (factorize.py:201-210) — the kernel scans them as one group, so
        # their carry must cross ranks too: give them a dedicated slot
        # ngroups (every rank gathers ngroups+1 slots so the collective
        # shapes agree even when only some ranks hold sentinel rows).
        # The lead_M>1 layout already folded sentinels in-range; its codes
        # pass through unchanged and the extra slot stays empty.
        codes = torch.where(
            (codes >= 0) & (codes < ngroups), codes, torch.full_like(codes, ngroups)
        )
        out = distributed.scan_carry_exchange(out, vals, codes, ngroups + 1, func)
    return out
