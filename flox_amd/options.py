"""Runtime options (the reference's flox.set_options surface, options.py:9-64,
re-keyed to this engine's knobs).

Supported options:
  packed_arg_threshold: group count above which arg-reductions leave the
      LDS two-pass form for the packed/pair partition paths (core.py).
  sparse_combine_ngroups: group count from which the distributed combine
      tries the shard-aware sparse (touched-bin) exchange (distributed.py).
  sparse_combine_fraction: gathered-traffic fraction under which the sparse
      exchange engages (vs the dense all-reduce).
  label_cache: False turns the label-code cache off (label_cache.py): every
      call reads the caller's labels, as if each were a first sighting.
  label_cache_entries: how many label tensors the cache tracks (LRU).
  label_cache_bytes: byte budget for the cached codes (2 B/row as uint16;
      1.5 / 1.75 B/row where they are packed to 12 / 14 bits).
  label_code_pack_min_rows: row count from which cached codes are packed to
      the width the group count needs (12 bits up to 4094 groups, 14 bits up
      to 16382); smaller calls keep the uint16 form (label_cache.py).
  fused_finalize: False makes mean/sum/count return to per-group partials
      finished by torch ops; on (the default) the combine kernel writes the
      finished result where the LDS-binned path serves the call (core.py).
  fused_many: False makes groupby_reduce_many run every func through its own
      groupby_reduce passes; on (the default) the sum/mean/var/std/min/max/
      count family shares one SET_SUMMARY pass on eligible calls: on the
      LDS-binned path without leading dims, on the column path (any group
      count) with them (core.py).
  cols_order_funcs: False sends argmax/argmin/nanargmax/nanargmin and
      first/last/nanfirst/nanlast over leading dims through the lead fold
      (composite int64 labels over the flattened array, limited to
      N * lead_M < 2**31); on (the default) they take the column kernel's
      row-valued sets, which read the caller's strided view in place, once,
      at any size, where the call is eligible: f32/f64/i32/i64 values after
      normalisation, not distributed, no datetime values, no axis subset,
      at least one row and one group (core.py).
  cols_sorted_funcs: False sends quantile/nanquantile/median/nanmedian and
      mode/nanmode over leading dims through the lead fold (a device-wide
      radix sort of N * lead_M composite keys, limited to N * lead_M <
      2**31); on (the default) each group's rows are sorted in LDS by the
      column kernel, which reads the caller's strided view in place, once,
      at any size, where the call is eligible: the conditions of
      cols_order_funcs, no hipGraph capture, and no group longer than the
      kernel's capacity (2048 rows) (core.py).
  cols_select_funcs: False sends quantile/nanquantile/median/nanmedian over
      leading dims through the lead fold as soon as one group is longer than
      the sort-in-LDS capacity, with the fold's limit of N * lead_M < 2**31;
      on (the default) such calls take the radix-select column kernel, which
      finds each (group, column)'s order statistics in per-tile LDS digit
      histograms: the caller's strided view is read in place (5 times for
      4-byte values, 9 for 8-byte ones, one less where no column needs a
      second key), at any size and any group length, where the call meets
      the conditions of cols_sorted_funcs and lead_M >= cols_select_min_cols.
      It extends cols_sorted_funcs and is off where that is off; mode and
      nanmode keep the fold for long groups (core.py).
  cols_select_min_cols: the narrowest lead_M that takes the radix-select
      kernel. Its grid is column tiles x groups, so a narrow array with few
      long groups is left to the fold; None = the measured default, 16384
      (profiles/r11_cols_select.md). One column tile (64) is the least
      useful value.
  cols_scan: False sends cumsum/nancumsum/ffill/bfill over leading dims
      through the lead fold (a flattened copy, composite int64 labels and a
      device-wide radix sort of N * lead_M pairs with about 70 B of scratch
      per element, limited to N * lead_M < 2**32); on (the default) the
      column kernel walks each group's rows with one running value per
      column, reading the caller's strided view in place and writing the
      result once, at any size, where the call is eligible: the (N, lead_M)
      view has unit column stride without a copy (time-major storage read
      through a permute view), f32/f64/i64 values after promotion for the
      sums and f32/f64 for the fills, not distributed, no datetime values,
      at least one row, N < 2**31, no hipGraph capture, and lead_M >=
      cols_scan_min_cols (scan.py).
  cols_scan_min_cols: the narrowest lead_M that takes the column form. Its
      parallelism is column tiles times group-aligned row chunks, so a
      narrow array with few long groups is left to the fold; None = the
      measured default (profiles/r10_cols_scan.md).
  rows_scan: False sends the same four scans over leading dims through the
      lead fold also where the grouped axis is the last, contiguous one (the
      C-contiguous (lead..., N) layout every numpy input has on the device),
      with the fold's sort, scratch and N * lead_M < 2**32 limit; on (the
      default) the row kernel stages tiles of the caller's rows through LDS,
      one lane per lead row walking the time steps in order with the other
      groups' running values parked in LDS, reading the array in place and
      writing the result once, at any size, where the call is eligible: the
      column form does not apply, the (lead_M, N) view has unit stride along
      N and one row stride without a copy, f32/f64/i64 values after promotion
      for the sums and f32/f64 for the fills, not distributed, no datetime
      values, 1 <= N < 2**31, no more groups than the kernel has LDS for
      (2333 for 4-byte values, 1202 for 8-byte ones), and lead_M >=
      rows_scan_min_rows. hipGraph capture does not exclude it (scan.py).
  rows_scan_min_rows: the fewest lead rows that take the row form. Its
      parallelism is lead rows alone, one wave per tile of up to 64 rows, so
      an array with few rows is left to the fold; None = the measured
      default (profiles/r12_rows_scan.md).
"""

from __future__ import annotations

from contextlib import contextmanager

OPTIONS = {
    "packed_arg_threshold": None,     # None = the measured default
    "sparse_combine_ngroups": None,
    "sparse_combine_fraction": None,
    "label_cache": None,              # None = on
    "label_cache_entries": None,
    "label_cache_bytes": None,
    "label_code_pack_min_rows": None,  # None = the measured default
    "fused_finalize": None,           # None = on
    "fused_many": None,               # None = on
    "cols_order_funcs": None,         # None = on
    "cols_sorted_funcs": None,        # None = on
    "cols_select_funcs": None,        # None = on
    "cols_select_min_cols": None,     # None = the measured default
    "cols_scan": None,                # None = on
    "cols_scan_min_cols": None,       # None = the measured default
    "rows_scan": None,                # None = on
    "rows_scan_min_rows": None,       # None = the measured default
}

_CACHE_FIELDS = {
    "label_cache": "enabled",
    "label_cache_entries": "max_entries",
    "label_cache_bytes": "max_bytes",
}


def _apply(name, value):
    from . import core, distributed, label_cache, scan

    if name in _CACHE_FIELDS:
        field = _CACHE_FIELDS[name]
        old = getattr(label_cache.CACHE, field)
        if value is not None:
            label_cache.CACHE.configure(**{field: value})
        return (name, old)
    if name == "label_code_pack_min_rows":
        old = label_cache.PACK_MIN_ROWS
        if value is not None:
            label_cache.PACK_MIN_ROWS = int(value)
        return (name, old)
    if name == "packed_arg_threshold":
        old = core.PACKED_ARG_THRESHOLD
        if value is not None:
            core.PACKED_ARG_THRESHOLD = int(value)
        return ("packed_arg_threshold", old)
    if name == "fused_finalize":
        old = core.FUSED_FINALIZE
        if value is not None:
            core.FUSED_FINALIZE = bool(value)
        return ("fused_finalize", old)
    if name == "fused_many":
        old = core.FUSED_MANY
        if value is not None:
            core.FUSED_MANY = bool(value)
        return ("fused_many", old)
    if name == "cols_order_funcs":
        old = core.COLS_ORDER_FUNCS
        if value is not None:
            core.COLS_ORDER_FUNCS = bool(value)
        return ("cols_order_funcs", old)
    if name == "cols_sorted_funcs":
        old = core.COLS_SORTED_FUNCS
        if value is not None:
            core.COLS_SORTED_FUNCS = bool(value)
        return ("cols_sorted_funcs", old)
    if name == "cols_select_funcs":
        old = core.COLS_SELECT_FUNCS
        if value is not None:
            core.COLS_SELECT_FUNCS = bool(value)
        return ("cols_select_funcs", old)
    if name == "cols_select_min_cols":
        old = core.COLS_SELECT_MIN_COLS
        if value is not None:
            core.COLS_SELECT_MIN_COLS = int(value)
        return ("cols_select_min_cols", old)
    if name == "cols_scan":
        old = scan.COLS_SCAN
        if value is not None:
            scan.COLS_SCAN = bool(value)
        return ("cols_scan", old)
    if name == "cols_scan_min_cols":
        old = scan.COLS_SCAN_MIN_COLS
        if value is not None:
            scan.COLS_SCAN_MIN_COLS = int(value)
        return ("cols_scan_min_cols", old)
    if name == "rows_scan":
        old = scan.ROWS_SCAN
        if value is not None:
            scan.ROWS_SCAN = bool(value)
        return ("rows_scan", old)
    if name == "rows_scan_min_rows":
        old = scan.ROWS_SCAN_MIN_ROWS
        if value is not None:
            scan.ROWS_SCAN_MIN_ROWS = int(value)
        return ("rows_scan_min_rows", old)
    if name == "sparse_combine_ngroups":
        old = distributed.SPARSE_NGROUPS
        if value is not None:
            distributed.SPARSE_NGROUPS = int(value)
        return ("sparse_combine_ngroups", old)
    if name == "sparse_combine_fraction":
        old = distributed.SPARSE_FRACTION
        if value is not None:
            distributed.SPARSE_FRACTION = float(value)
        return ("sparse_combine_fraction", old)
    raise ValueError(
        f"unknown option {name!r}; supported: {sorted(OPTIONS)}"
    )


def _restore(name, old):
    from . import core, distributed, label_cache, scan

    if name in _CACHE_FIELDS:
        label_cache.CACHE.configure(**{_CACHE_FIELDS[name]: old})
    elif name == "label_code_pack_min_rows":
        label_cache.PACK_MIN_ROWS = old
    elif name == "packed_arg_threshold":
        core.PACKED_ARG_THRESHOLD = old
    elif name == "fused_finalize":
        core.FUSED_FINALIZE = old
    elif name == "fused_many":
        core.FUSED_MANY = old
    elif name == "cols_order_funcs":
        core.COLS_ORDER_FUNCS = old
    elif name == "cols_sorted_funcs":
        core.COLS_SORTED_FUNCS = old
    elif name == "cols_select_funcs":
        core.COLS_SELECT_FUNCS = old
    elif name == "cols_select_min_cols":
        core.COLS_SELECT_MIN_COLS = old
    elif name == "cols_scan":
        scan.COLS_SCAN = old
    elif name == "cols_scan_min_cols":
        scan.COLS_SCAN_MIN_COLS = old
    elif name == "rows_scan":
        scan.ROWS_SCAN = old
    elif name == "rows_scan_min_rows":
        scan.ROWS_SCAN_MIN_ROWS = old
    elif name == "sparse_combine_ngroups":
        distributed.SPARSE_NGROUPS = old
    elif name == "sparse_combine_fraction":
        distributed.SPARSE_FRACTION = old


@contextmanager
def set_options(**kwargs):
    """Context manager over the engine's runtime knobs (the reference's
    flox.set_options shape: `with flox_amd.set_options(x=...): ...`)."""
    saved = [_apply(k, v) for k, v in kwargs.items()]
    try:
        yield
    finally:
        for name, old in reversed(saved):
            _restore(name, old)
