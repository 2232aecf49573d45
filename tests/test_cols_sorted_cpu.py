"""The sort-in-LDS column form without a GPU: the tile plan header, built as
a stand-alone host program under AddressSanitizer and UBSan and run directly,
and the cols_sorted_funcs option."""

import os
import shutil
import subprocess

import pytest

import flox_amd
from flox_amd import core

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def test_tile_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "qcols_plan_host")
    subprocess.run(
        [_host_compiler(), "-std=c++17", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "qcols_plan_host.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qcols plan host checks OK" in r.stdout


def test_option_round_trip():
    assert core.COLS_SORTED_FUNCS is True
    with flox_amd.set_options(cols_sorted_funcs=False):
        assert core.COLS_SORTED_FUNCS is False
        with flox_amd.set_options(cols_sorted_funcs=True):
            assert core.COLS_SORTED_FUNCS is True
        assert core.COLS_SORTED_FUNCS is False
        with flox_amd.set_options(cols_sorted_funcs=None):  # None = leave as is
            assert core.COLS_SORTED_FUNCS is False
    assert core.COLS_SORTED_FUNCS is True
    # the neighbouring switch is its own
    with flox_amd.set_options(cols_order_funcs=False):
        assert core.COLS_SORTED_FUNCS is True and core.COLS_ORDER_FUNCS is False
    with pytest.raises(ValueError, match="unknown option"):
        with flox_amd.set_options(cols_sorted=False):
            pass


def test_the_six_functions_are_the_switch_s_scope():
    assert set(core._COLS_SORTED) == {
        "quantile", "nanquantile", "median", "nanmedian", "mode", "nanmode"}
    assert not set(core._COLS_SORTED) & set(core._COLS_ORDER)
    assert set(core._COLS_SORTED) <= set(core._LEAD_FOLD_FUNCS)
