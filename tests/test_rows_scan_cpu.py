"""The row form of the grouped scans without a GPU: the tile plan header, built
as a stand-alone host program under AddressSanitizer and UBSan and run
directly, and the rows_scan / rows_scan_min_rows options."""

import os
import subprocess

import pytest

import flox_amd
from flox_amd import scan
from tests.test_cols_sorted_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scanrows_plan_host")
    subprocess.run(
        [_host_compiler(), "-std=c++17", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "scanrows_plan_host.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scanrows plan host checks OK" in r.stdout


def test_option_round_trip():
    assert scan.ROWS_SCAN is True
    default_rows = scan.ROWS_SCAN_MIN_ROWS
    with flox_amd.set_options(rows_scan=False):
        assert scan.ROWS_SCAN is False
        with flox_amd.set_options(rows_scan=True):
            assert scan.ROWS_SCAN is True
        assert scan.ROWS_SCAN is False
        with flox_amd.set_options(rows_scan=None):  # None = leave as is
            assert scan.ROWS_SCAN is False
        assert scan.ROWS_SCAN_MIN_ROWS == default_rows  # the gate is its own option
    assert scan.ROWS_SCAN is True
    with flox_amd.set_options(rows_scan_min_rows=1):
        assert scan.ROWS_SCAN_MIN_ROWS == 1 and scan.ROWS_SCAN is True
        with flox_amd.set_options(rows_scan_min_rows=None):
            assert scan.ROWS_SCAN_MIN_ROWS == 1
        with flox_amd.set_options(rows_scan_min_rows=4096, rows_scan=False):
            assert scan.ROWS_SCAN_MIN_ROWS == 4096 and scan.ROWS_SCAN is False
        assert scan.ROWS_SCAN_MIN_ROWS == 1 and scan.ROWS_SCAN is True
    assert scan.ROWS_SCAN_MIN_ROWS == default_rows


def test_each_switch_is_independent_of_cols_scan():
    default_rows, default_cols = scan.ROWS_SCAN_MIN_ROWS, scan.COLS_SCAN_MIN_COLS
    with flox_amd.set_options(cols_scan=False):
        assert scan.ROWS_SCAN is True and scan.COLS_SCAN is False
    with flox_amd.set_options(rows_scan=False):
        assert scan.COLS_SCAN is True and scan.ROWS_SCAN is False
    with flox_amd.set_options(cols_scan_min_cols=7):
        assert scan.ROWS_SCAN_MIN_ROWS == default_rows and scan.COLS_SCAN_MIN_COLS == 7
    with flox_amd.set_options(rows_scan_min_rows=7):
        assert scan.COLS_SCAN_MIN_COLS == default_cols and scan.ROWS_SCAN_MIN_ROWS == 7
    assert (scan.ROWS_SCAN, scan.COLS_SCAN) == (True, True)
    assert (scan.ROWS_SCAN_MIN_ROWS, scan.COLS_SCAN_MIN_COLS) == (default_rows, default_cols)


def test_near_miss_names_are_unknown_options():
    for wrong in ("row_scan", "rows_scans", "rows_scan_min_row", "rows_scan_min_cols",
                  "scan_rows"):
        with pytest.raises(ValueError, match="unknown option"):
            with flox_amd.set_options(**{wrong: False}):
                pass
    assert scan.ROWS_SCAN is True


def test_the_default_gate_is_at_least_the_largest_row_tile():
    # include/floxhip_scanrows.h: FH_SCANROWS_MAX_ROWS, the few-groups plan's tile
    with open(os.path.join(HERE, "..", "include", "floxhip_scanrows.h")) as f:
        line = next(ln for ln in f if ln.startswith("#define FH_SCANROWS_MAX_ROWS"))
    assert scan.ROWS_SCAN_MIN_ROWS >= int(line.split()[2])
