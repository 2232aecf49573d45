"""The radix-select column form without a GPU: the tile plan header, built as
a stand-alone host program under AddressSanitizer and UBSan and run directly,
and the cols_select_funcs / cols_select_min_cols options."""

import os
import subprocess

import pytest

import flox_amd
from flox_amd import core
from tests.test_cols_sorted_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "selcols_plan_host")
    subprocess.run(
        [_host_compiler(), "-std=c++17", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "selcols_plan_host.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selcols plan host checks OK" in r.stdout


def test_option_round_trip():
    assert core.COLS_SELECT_FUNCS is True
    default_cols = core.COLS_SELECT_MIN_COLS
    with flox_amd.set_options(cols_select_funcs=False):
        assert core.COLS_SELECT_FUNCS is False
        with flox_amd.set_options(cols_select_funcs=True):
            assert core.COLS_SELECT_FUNCS is True
        assert core.COLS_SELECT_FUNCS is False
        with flox_amd.set_options(cols_select_funcs=None):  # None = leave as is
            assert core.COLS_SELECT_FUNCS is False
        # the width gate is its own option
        assert core.COLS_SELECT_MIN_COLS == default_cols
    assert core.COLS_SELECT_FUNCS is True
    with flox_amd.set_options(cols_select_min_cols=1):
        assert core.COLS_SELECT_MIN_COLS == 1 and core.COLS_SELECT_FUNCS is True
        with flox_amd.set_options(cols_select_min_cols=None):
            assert core.COLS_SELECT_MIN_COLS == 1
        with flox_amd.set_options(cols_select_min_cols=4096, cols_select_funcs=False):
            assert core.COLS_SELECT_MIN_COLS == 4096 and core.COLS_SELECT_FUNCS is False
        assert core.COLS_SELECT_MIN_COLS == 1 and core.COLS_SELECT_FUNCS is True
    assert core.COLS_SELECT_MIN_COLS == default_cols
    # neither switch moves the other
    with flox_amd.set_options(cols_sorted_funcs=False):
        assert core.COLS_SELECT_FUNCS is True and core.COLS_SORTED_FUNCS is False
    with flox_amd.set_options(cols_select_funcs=False):
        assert core.COLS_SORTED_FUNCS is True and core.COLS_SELECT_FUNCS is False
    for wrong in ("cols_select", "cols_select_func", "cols_select_min_col"):
        with pytest.raises(ValueError, match="unknown option"):
            with flox_amd.set_options(**{wrong: False}):
                pass
    assert core.COLS_SELECT_FUNCS is True and core.COLS_SELECT_MIN_COLS == default_cols


def test_the_default_gate_is_at_least_one_column_tile():
    # include/floxhip_selcols.h: FH_SELCOLS_MAX_COLS, the one-slot plan's tile
    with open(os.path.join(HERE, "..", "include", "floxhip_selcols.h")) as f:
        line = next(ln for ln in f if ln.startswith("#define FH_SELCOLS_MAX_COLS"))
    assert core.COLS_SELECT_MIN_COLS >= int(line.split()[2])


def test_the_four_quantile_names_are_the_switch_s_scope():
    assert set(core._COLS_SELECT) == {"quantile", "nanquantile", "median", "nanmedian"}
    assert not {"mode", "nanmode"} & set(core._COLS_SELECT)
    assert set(core._COLS_SELECT) <= set(core._COLS_SORTED)
