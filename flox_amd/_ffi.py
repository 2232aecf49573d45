"""ctypes binding to the in-tree HIP library (flox_amd/libfloxhip.so).

The library implements the C ABI declared in include/floxhip.h — the drop-in
boundary for the reference's engine seam (flox/aggregations.py:60-133).
This module FAILS LOUDLY if the extension or a GPU is missing: the product
path has no CPU fallback (parity claims depend on the HIP kernels being the
code that runs).
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfloxhip.so")

# fh_dtype / fh_ldtype / fh_opset / fh_flags — mirror include/floxhip.h
F32, F64, I64, I32 = 0, 1, 2, 3
L_I64, L_I32, L_U16, L_P12, L_P14 = 0, 1, 2, 3, 4
# cached label codes by bits per code (label_cache.py)
L_CODES = {16: L_U16, 14: L_P14, 12: L_P12}
SET_SUM_COUNT = 0
SET_SUM_COUNT_PRESENT = 1
SET_COUNT = 2
SET_MIN_FULL = 3
SET_MIN_COUNT = 4
SET_MAX_FULL = 5
SET_MAX_COUNT = 6
SET_SSD = 7
SET_PROD = 8
SET_IDXMIN = 9
SET_IDXMAX = 10
SET_WELFORD = 11
SET_ARGMIN_PAIR = 12
SET_ARGMAX_PAIR = 13
SET_SUMMARY = 14
SET_ARGMIN_COLS = 15  # column path only (fh_grouped_reduce_cols)
SET_ARGMAX_COLS = 16
FLAG_SKIPNAN = 1
FLAG_FORCE_LDS = 2
FLAG_FORCE_ATOMIC = 4
FLAG_SORTED_LABELS = 8
FLAG_NO_HOST_SYNC = 16
FINISH_NONE, FINISH_MEAN, FINISH_SUM, FINISH_COUNT = 0, 1, 2, 3

VDTYPE_OF = {
    np.dtype("float32"): F32,
    np.dtype("float64"): F64,
    np.dtype("int64"): I64,
    np.dtype("int32"): I32,
}
LDTYPE_OF = {np.dtype("int64"): L_I64, np.dtype("int32"): L_I32}


class FhCall(ctypes.Structure):
    _fields_ = [
        ("op_set", ctypes.c_int),
        ("vdtype", ctypes.c_int),
        ("ldtype", ctypes.c_int),
        ("flags", ctypes.c_int),
        ("n", ctypes.c_int64),
        ("ngroups", ctypes.c_int64),
        ("values", ctypes.c_void_p),
        ("labels", ctypes.c_void_p),
        ("labels2", ctypes.c_void_p),
        ("g0", ctypes.c_int64),
        ("g1", ctypes.c_int64),
        ("means", ctypes.c_void_p),
        ("out_sum", ctypes.c_void_p),
        ("out_count", ctypes.c_void_p),
        ("out_present", ctypes.c_void_p),
        ("out_min", ctypes.c_void_p),
        ("out_max", ctypes.c_void_p),
        ("out_nanflag", ctypes.c_void_p),
        ("scratch", ctypes.c_void_p),
        ("scratch_bytes", ctypes.c_int64),
        ("stream", ctypes.c_void_p),
        ("path_used", ctypes.c_int),
        # column path (fh_grouped_reduce_cols)
        ("perm", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("ldm", ctypes.c_int64),
        ("chunk_offsets", ctypes.c_void_p),
        ("nchunks", ctypes.c_int64),
        ("target", ctypes.c_void_p),
        ("row_offset", ctypes.c_int64),
        # label-code cache: uint16[n] output of an emitting LDS-path call
    # (repacked by fh_pack_codes where a narrower width applies)
        ("emit_codes", ctypes.c_void_p),
        # fused finish (fh_finish): result buffer instead of partials
        ("finish", ctypes.c_int),
        ("result_dtype", ctypes.c_int),
        ("result", ctypes.c_void_p),
        ("min_count", ctypes.c_int64),
        ("has_fill", ctypes.c_int),
        ("fill", ctypes.c_double),
        # SET_SUMMARY: f64[ngroups] sum of squared deviations about the mean
        ("out_ssd", ctypes.c_void_p),
    ]


_lib = None


def load_library():
    """Load libfloxhip.so; raise (never fall back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"flox_amd HIP extension not built: {_LIB_PATH} missing. "
            "Run __graft_entry__.build() (hipcc --offload-arch=gfx950)."
        )
    lib = ctypes.CDLL(_LIB_PATH)
    lib.fh_grouped_reduce.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_grouped_reduce.restype = ctypes.c_int
    lib.fh_grouped_reduce_cols.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_grouped_reduce_cols.restype = ctypes.c_int
    lib.fh_scratch_bytes.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_scratch_bytes.restype = ctypes.c_int64
    lib.fh_quantile_scratch_bytes.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_quantile_scratch_bytes.restype = ctypes.c_int64
    lib.fh_grouped_quantile.argtypes = [ctypes.POINTER(FhCall), ctypes.c_int]
    lib.fh_grouped_quantile.restype = ctypes.c_int
    lib.fh_scan_scratch_bytes.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_scan_scratch_bytes.restype = ctypes.c_int64
    lib.fh_grouped_scan.argtypes = [ctypes.POINTER(FhCall), ctypes.c_int]
    lib.fh_grouped_scan.restype = ctypes.c_int
    lib.fh_pack_argkeys.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fh_pack_argkeys.restype = ctypes.c_int
    lib.fh_packed_code_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.fh_packed_code_bytes.restype = ctypes.c_int64
    lib.fh_pack_codes.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fh_pack_codes.restype = ctypes.c_int
    lib.fh_error_string.argtypes = [ctypes.c_int]
    lib.fh_error_string.restype = ctypes.c_char_p
    lib.fh_version.argtypes = []
    lib.fh_version.restype = ctypes.c_int
    lib.fh_query_path.argtypes = [ctypes.POINTER(FhCall)]
    lib.fh_query_path.restype = ctypes.c_int
    lib.fh_abi_revision.argtypes = []
    lib.fh_abi_revision.restype = ctypes.c_int
    if lib.fh_version() != 1 or lib.fh_abi_revision() < 6:
        raise RuntimeError("libfloxhip.so ABI version mismatch")
    # the column forms of the row-valued sets came without a new revision:
    # the symbol is how a caller detects them (cols_supports below)
    if hasattr(lib, "fh_cols_supports"):
        lib.fh_cols_supports.argtypes = [ctypes.c_int]
        lib.fh_cols_supports.restype = ctypes.c_int
    # likewise the sort-in-LDS column form of the quantile family
    if hasattr(lib, "fh_grouped_quantile_cols"):
        lib.fh_grouped_quantile_cols.argtypes = [
            ctypes.POINTER(FhCall), ctypes.c_int, ctypes.c_int64,
        ]
        lib.fh_grouped_quantile_cols.restype = ctypes.c_int
        lib.fh_quantile_cols_max_rows.argtypes = [ctypes.c_int]
        lib.fh_quantile_cols_max_rows.restype = ctypes.c_int64
    # and the column form of the grouped scans
    if hasattr(lib, "fh_grouped_scan_cols"):
        lib.fh_grouped_scan_cols.argtypes = [
            ctypes.POINTER(FhCall), ctypes.c_int, ctypes.c_int64,
        ]
        lib.fh_grouped_scan_cols.restype = ctypes.c_int
    # and the radix-select column form of the quantile family
    if hasattr(lib, "fh_grouped_quantile_select_cols"):
        lib.fh_grouped_quantile_select_cols.argtypes = [
            ctypes.POINTER(FhCall), ctypes.c_int,
        ]
        lib.fh_grouped_quantile_select_cols.restype = ctypes.c_int
    # and the row form of the grouped scans
    if hasattr(lib, "fh_grouped_scan_rows"):
        lib.fh_grouped_scan_rows.argtypes = [
            ctypes.POINTER(FhCall), ctypes.c_int, ctypes.c_int64,
        ]
        lib.fh_grouped_scan_rows.restype = ctypes.c_int
        lib.fh_scan_rows_max_groups.argtypes = [ctypes.c_int]
        lib.fh_scan_rows_max_groups.restype = ctypes.c_int64
        lib.fh_scan_rows_plan.argtypes = [
            ctypes.c_int, ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ]
        lib.fh_scan_rows_plan.restype = ctypes.c_int
    _lib = lib
    return lib


def has_select_cols() -> bool:
    """Whether the loaded library has fh_grouped_quantile_select_cols."""
    return hasattr(load_library(), "fh_grouped_quantile_select_cols")


def has_scan_cols() -> bool:
    """Whether the loaded library has fh_grouped_scan_cols."""
    return hasattr(load_library(), "fh_grouped_scan_cols")


def has_scan_rows() -> bool:
    """Whether the loaded library has fh_grouped_scan_rows."""
    return hasattr(load_library(), "fh_grouped_scan_rows")


def scan_rows_max_groups(vdtype: int) -> int:
    """The largest group count fh_grouped_scan_rows serves for this value
    dtype; 0 where the loaded library predates the entry."""
    lib = load_library()
    if not hasattr(lib, "fh_grouped_scan_rows"):
        return 0
    return int(lib.fh_scan_rows_max_groups(vdtype))


def scan_rows_plan(vdtype: int, ngroups: int) -> tuple[int, int]:
    """(lead rows per workgroup, time steps per tile) of fh_grouped_scan_rows
    for this value dtype and group count."""
    lib = load_library()
    r, t = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.fh_scan_rows_plan(vdtype, ngroups, ctypes.byref(r), ctypes.byref(t)),
          _SCAN_ROWS_ERRORS)
    return r.value, t.value


def quantile_cols_max_rows(vdtype: int) -> int:
    """The longest group fh_grouped_quantile_cols can stage for this value
    dtype; 0 where the loaded library predates the entry."""
    lib = load_library()
    if not hasattr(lib, "fh_grouped_quantile_cols"):
        return 0
    return int(lib.fh_quantile_cols_max_rows(vdtype))


def cols_supports(op_set: int) -> bool:
    """Whether fh_grouped_reduce_cols of the loaded library serves op_set. A
    library without fh_cols_supports predates the row-valued column forms
    and serves the sets that had one before: all but the index and arg sets."""
    lib = load_library()
    if hasattr(lib, "fh_cols_supports"):
        return lib.fh_cols_supports(op_set) == 1
    return op_set in (
        SET_SUM_COUNT, SET_SUM_COUNT_PRESENT, SET_COUNT, SET_MIN_FULL, SET_MIN_COUNT,
        SET_MAX_FULL, SET_MAX_COUNT, SET_SSD, SET_PROD, SET_WELFORD, SET_SUMMARY,
    )


# codes of fh_grouped_quantile_cols, which fh_error_string predates
_QCOLS_ERRORS = {
    20: "max_seg_rows exceeds fh_quantile_cols_max_rows for the value dtype",
    21: "fh_grouped_quantile_cols: missing values/labels/perm/out_sum buffer, "
        "missing q array, or an extent that is negative or beyond int32 rows",
    # fh_grouped_scan_cols
    22: "fh_grouped_scan_cols: missing values/labels/perm/out_sum buffer",
    23: "fh_grouped_scan_cols: an extent that is negative, beyond int32 rows, "
        "a row stride below the column count, or nchunks out of range",
    24: "fh_grouped_scan_cols: unknown op, or a value dtype the op is not "
        "served for (sums: f32/f64/i64, fills: f32/f64)",
}


# fh_grouped_quantile_select_cols gives code 22 its own meaning
_SELECT_COLS_ERRORS = {
    22: "fh_grouped_quantile_select_cols: missing values/labels/perm/out_sum/q "
        "buffer, nq below 1, or an extent that is negative or beyond int32 rows",
}


# fh_grouped_scan_rows numbers its refusals as fh_grouped_scan_cols does
_SCAN_ROWS_ERRORS = {
    22: "fh_grouped_scan_rows: missing values/labels/out_sum buffer",
    23: "fh_grouped_scan_rows: an extent that is negative, beyond int32 time "
        "steps, or a row stride below the number of time steps",
    24: "fh_grouped_scan_rows: unknown op, or a value dtype the op is not "
        "served for (sums: f32/f64/i64, fills: f32/f64)",
    25: "fh_grouped_scan_rows: ngroups exceeds fh_scan_rows_max_groups for the "
        "value dtype",
}


def check(code: int, errors=_QCOLS_ERRORS) -> None:
    if code != 0:
        msg = errors.get(code) or load_library().fh_error_string(code).decode()
        raise RuntimeError(f"floxhip error {code}: {msg}")
