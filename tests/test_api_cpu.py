"""CPU-runnable checks: package import, the C-ABI surface, and that the
product NEVER silently falls back to CPU compute."""

import ctypes
import os

import numpy as np
import pytest

import flox_amd
from flox_amd import REDUCTIONS, generic_aggregate

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flox_amd", "libfloxhip.so")


def test_registry_covers_reference_reduction_core():
    # the reduction families of the reference registry this tier implements
    # (reference flox/aggregations.py:881-913)
    for f in [
        "count", "sum", "nansum", "prod", "nanprod", "mean", "nanmean",
        "var", "nanvar", "std", "nanstd", "min", "nanmin", "max", "nanmax",
    ]:
        assert f in REDUCTIONS


def test_cabi_library_loads_and_exports_declared_symbols():
    """include/floxhip.h declares the boundary; the built .so must export it."""
    assert os.path.exists(LIB), "libfloxhip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    for sym in [
        "fh_grouped_reduce", "fh_grouped_reduce_cols", "fh_scratch_bytes",
        "fh_grouped_quantile", "fh_quantile_scratch_bytes", "fh_grouped_scan",
        "fh_scan_scratch_bytes", "fh_pack_argkeys", "fh_error_string",
        "fh_version",
    ]:
        assert hasattr(lib, sym), sym
    lib.fh_version.restype = ctypes.c_int
    assert lib.fh_version() == 1
    lib.fh_error_string.restype = ctypes.c_char_p
    assert lib.fh_error_string(0) == b"ok"
    assert b"op_set" in lib.fh_error_string(4)


def test_scratch_bytes_no_gpu_needed():
    from flox_amd._ffi import FhCall, load_library

    lib = load_library()
    c = FhCall()
    c.op_set = 0  # SUM_COUNT
    c.vdtype = 0  # f32
    c.ngroups = 10_000
    n = lib.fh_scratch_bytes(ctypes.byref(c))
    # 1e4 groups: sum 8B + count 4B per group per block-copy, 256-B aligned,
    # one block per CU (bins > 78 KiB)
    assert n > 0
    assert n % 256 == 0
    per_block = 80128 + 40192  # carve-aligned sections
    assert n == 256 * per_block, n


# fh_scratch_bytes / fh_query_path pinned on values recorded from the build
# before the host launch layer was restructured (quirks included: e.g. the
# summary set reports path 0 and no scratch once its bins outgrow LDS).
# n = 1_000_000, m = 0. Key: (op_set, value dtypes sharing the row). Each
# list runs over ngroups (outer) x flags (inner, none/FORCE_LDS/FORCE_ATOMIC).
_F32, _F64, _I64, _I32 = 0, 1, 2, 3
SIZING_NGROUPS = [100, 8000, 13000, 14000, 2_000_000, 20_000_000, 40_000_000]
SIZING_FLAGS = [0, 2, 4]
_P_NONE = [0] * 21
_P_8000 = [1, 1, 0, 1, 1, 0] + [0] * 15
_P_13000 = [1, 1, 0] * 3 + [0] * 12
_P_14000 = [1, 1, 0] * 4 + [0] * 9
SIZING = {
    (0, (_F32, _I32)): ([786432, 786432, 786432, 24576000, 24576000, 24576000, 40042496, 40042496, 40042496, 10132736, 43057152, 0, 36357632, 6144000000, 0, 182631680, 61440000000, 0, 0, 122880000000, 0],
                        _P_13000),
    (0, (_F64, _I64)): ([786432, 786432, 786432, 24576000, 24576000, 24576000, 40042496, 40042496, 40042496, 20264192, 43057152, 0, 72711680, 6144000000, 0, 365232896, 61440000000, 0, 0, 122880000000, 0],
                        _P_13000),
    (1, (_F32, _I32)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 10263808, 53411840, 0, 10263808, 57409536, 0, 52595200, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                        _P_8000),
    (1, (_F64, _I64)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 20526336, 53411840, 0, 20526336, 57409536, 0, 105183744, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                        _P_8000),
    (2, (_F32, _I32)): ([262144, 262144, 262144, 16384000, 16384000, 16384000, 26738688, 26738688, 26738688, 28704768, 28704768, 28704768, 36357632, 2048000000, 0, 182631680, 20480000000, 0, 0, 40960000000, 0],
                        _P_14000),
    (2, (_F64, _I64)): ([262144, 262144, 262144, 16384000, 16384000, 16384000, 26738688, 26738688, 26738688, 28704768, 28704768, 28704768, 72711680, 2048000000, 0, 365232896, 20480000000, 0, 0, 40960000000, 0],
                        _P_14000),
    (3, (_F32, _I32)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 10263808, 53477376, 0, 10263808, 57409536, 0, 52595200, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                        _P_8000),
    (3, (_F64, _I64)): ([1310720, 1310720, 1310720, 40960000, 40960000, 40960000, 20526336, 66781184, 0, 20526336, 71761920, 0, 105183744, 10240000000, 0, 0, 102400000000, 0, 0, 204800000000, 0],
                        _P_8000),
    (7, (_F32, _I32)): ([524288, 524288, 524288, 32768000, 32768000, 32768000, 26673152, 26673152, 26673152, 28704768, 28704768, 28704768, 36357632, 4096000000, 0, 182631680, 40960000000, 0, 0, 81920000000, 0],
                        _P_14000),
    (7, (_F64, _I64)): ([524288, 524288, 524288, 32768000, 32768000, 32768000, 26673152, 26673152, 26673152, 28704768, 28704768, 28704768, 72711680, 4096000000, 0, 365232896, 40960000000, 0, 0, 81920000000, 0],
                        _P_14000),
    (8, (_F32, _I32)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 10263808, 53411840, 0, 10263808, 57409536, 0, 52595200, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                        _P_8000),
    (8, (_F64, _I64)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 20526336, 53411840, 0, 20526336, 57409536, 0, 105183744, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                        _P_8000),
    (9, (_F32, _F64, _I64, _I32)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 0, 53411840, 0, 0, 57409536, 0, 0, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                                    _P_8000),
    (12, (_F32, _I32)): ([1048576, 1048576, 1048576, 32768000, 32768000, 32768000, 0, 53477376, 0, 0, 57409536, 0, 0, 8192000000, 0, 0, 81920000000, 0, 0, 163840000000, 0],
                         _P_NONE),
    (12, (_F64, _I64)): ([1310720, 1310720, 1310720, 40960000, 40960000, 40960000, 20526336, 66781184, 0, 20526336, 71761920, 0, 105183744, 10240000000, 0, 0, 102400000000, 0, 0, 204800000000, 0],
                         _P_NONE),
    (14, (_F32, _I32)): ([2883584, 2883584, 2883584] + [0] * 18, [1, 1, 0] + [0] * 18),
    (14, (_F64, _I64)): ([3670016, 3670016, 3670016] + [0] * 18, [1, 1, 0] + [0] * 18),
}
SIZING_CASES = [(op, vd, want) for (op, vds), want in SIZING.items() for vd in vds]


@pytest.mark.parametrize("op_set,vdtype,want", SIZING_CASES,
                         ids=[f"op{op}-vd{vd}" for op, vd, _ in SIZING_CASES])
def test_scratch_bytes_and_query_path_pinned(op_set, vdtype, want):
    from flox_amd._ffi import FhCall, load_library

    lib = load_library()
    want_bytes, want_path = want
    assert len(want_bytes) == len(want_path) == len(SIZING_NGROUPS) * len(SIZING_FLAGS)
    i = 0
    for ngroups in SIZING_NGROUPS:
        for flags in SIZING_FLAGS:
            c = FhCall()
            c.op_set, c.vdtype, c.flags = op_set, vdtype, flags
            c.n, c.ngroups = 1_000_000, ngroups
            got = (lib.fh_scratch_bytes(ctypes.byref(c)), lib.fh_query_path(ctypes.byref(c)))
            assert got == (want_bytes[i], want_path[i]), (ngroups, flags)
            i += 1


def test_sizing_table_is_the_full_cross():
    assert sorted({op for op, _, _ in SIZING_CASES}) == [0, 1, 2, 3, 7, 8, 9, 12, 14]
    assert len(SIZING_CASES) == 9 * 4


# column path (ngroups = 24, ldm = m, 32-byte aligned values):
# (op_set, vdtype, m, n, group-aligned chunk_offsets given, scratch bytes, path)
COLS_SIZING = [
    (0, _F32, 3, 100, False, 0, 1),
    (0, _F32, 3, 100, True, 0, 1),
    (0, _F32, 3, 1_000_000, False, 81920, 1),
    (0, _F32, 3, 1_000_000, True, 0, 1),
    (0, _F32, 64, 100, False, 0, 1),
    (0, _F32, 64, 1_000_000, False, 1179648, 1),
    (0, _F32, 64, 1_000_000, True, 0, 1),
    (3, _F64, 3, 1_000_000, False, 147456, 1),
    (3, _F64, 64, 100, False, 0, 1),
    (3, _F64, 64, 1_000_000, False, 1966080, 1),
    (3, _F64, 64, 1_000_000, True, 0, 1),
    (8, _I64, 3, 1_000_000, False, 114688, 1),
    (8, _I64, 64, 1_000_000, False, 1572864, 1),
    (11, _F32, 3, 1_000_000, False, 131072, 1),
    (11, _F32, 64, 1_000_000, False, 1966080, 1),
    (11, _F32, 64, 1_000_000, True, 0, 1),
    (14, _F32, 3, 1_000_000, False, 0, 1),
    (14, _F32, 64, 1_000_000, False, 0, 1),
]


@pytest.mark.parametrize("op_set,vdtype,m,n,chunks,want_bytes,want_path", COLS_SIZING)
def test_cols_scratch_bytes_pinned(op_set, vdtype, m, n, chunks, want_bytes, want_path):
    from flox_amd._ffi import FhCall, load_library

    lib = load_library()
    offsets = (ctypes.c_int64 * 3)(0, n // 2, n)
    c = FhCall()
    c.op_set, c.vdtype, c.n, c.ngroups, c.m, c.ldm = op_set, vdtype, n, 24, m, m
    if chunks:
        c.chunk_offsets = ctypes.addressof(offsets)
        c.nchunks = 2
    assert lib.fh_scratch_bytes(ctypes.byref(c)) == want_bytes
    assert lib.fh_query_path(ctypes.byref(c)) == want_path


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="requires a GPU"):
        flox_amd.groupby_reduce(np.ones(10), np.zeros(10, dtype=np.int64), func="sum")
    with pytest.raises(RuntimeError, match="requires a GPU"):
        generic_aggregate(np.zeros(4, dtype=np.int64), np.ones(4), engine="hip", func="sum", size=1)


def test_wrong_engine_rejected():
    with pytest.raises(ValueError, match="engine='hip' only"):
        generic_aggregate(np.zeros(4, dtype=np.int64), np.ones(4), engine="numpy", func="sum")


def test_unknown_func_rejected():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(NotImplementedError):
        flox_amd.groupby_reduce(np.ones(4), np.zeros(4, dtype=np.int64), func="cumsum")


def test_set_options_roundtrip():
    """flox_amd.set_options mirrors the reference's options context
    (reference options.py:9-64), re-keyed to this engine's knobs."""
    import flox_amd
    from flox_amd import core, distributed

    old_thr = core.PACKED_ARG_THRESHOLD
    old_ng = distributed.SPARSE_NGROUPS
    with flox_amd.set_options(packed_arg_threshold=123,
                              sparse_combine_ngroups=456,
                              sparse_combine_fraction=0.5):
        assert core.PACKED_ARG_THRESHOLD == 123
        assert distributed.SPARSE_NGROUPS == 456
        assert distributed.SPARSE_FRACTION == 0.5
    assert core.PACKED_ARG_THRESHOLD == old_thr
    assert distributed.SPARSE_NGROUPS == old_ng
    import pytest

    with pytest.raises(ValueError):
        with flox_amd.set_options(nonsense=1):
            pass
