"""The cols_scan / cols_scan_min_cols options (no GPU): present in OPTIONS,
applied, nested and restored by set_options, untouched by None."""

import pytest

import flox_amd
from flox_amd import scan as fa_scan


def test_both_options_are_registered():
    assert "cols_scan" in flox_amd.OPTIONS
    assert "cols_scan_min_cols" in flox_amd.OPTIONS
    assert flox_amd.OPTIONS["cols_scan"] is None            # None = on
    assert flox_amd.OPTIONS["cols_scan_min_cols"] is None   # None = the measured default
    assert fa_scan.COLS_SCAN is True
    assert isinstance(fa_scan.COLS_SCAN_MIN_COLS, int) and fa_scan.COLS_SCAN_MIN_COLS >= 1


def test_set_options_applies_nests_and_restores():
    on0, min0 = fa_scan.COLS_SCAN, fa_scan.COLS_SCAN_MIN_COLS
    with flox_amd.set_options(cols_scan=False, cols_scan_min_cols=7):
        assert fa_scan.COLS_SCAN is False
        assert fa_scan.COLS_SCAN_MIN_COLS == 7
        with flox_amd.set_options(cols_scan=True):
            assert fa_scan.COLS_SCAN is True
            assert fa_scan.COLS_SCAN_MIN_COLS == 7
            with flox_amd.set_options(cols_scan_min_cols=1):
                assert fa_scan.COLS_SCAN_MIN_COLS == 1
            assert fa_scan.COLS_SCAN_MIN_COLS == 7
        assert fa_scan.COLS_SCAN is False
    assert (fa_scan.COLS_SCAN, fa_scan.COLS_SCAN_MIN_COLS) == (on0, min0)


def test_restores_after_an_exception():
    on0, min0 = fa_scan.COLS_SCAN, fa_scan.COLS_SCAN_MIN_COLS
    with pytest.raises(KeyError):
        with flox_amd.set_options(cols_scan=False, cols_scan_min_cols=3):
            raise KeyError("boom")
    assert (fa_scan.COLS_SCAN, fa_scan.COLS_SCAN_MIN_COLS) == (on0, min0)


def test_none_leaves_them_as_they_are():
    with flox_amd.set_options(cols_scan=False, cols_scan_min_cols=5):
        with flox_amd.set_options(cols_scan=None, cols_scan_min_cols=None):
            assert fa_scan.COLS_SCAN is False
            assert fa_scan.COLS_SCAN_MIN_COLS == 5
        assert fa_scan.COLS_SCAN is False
        assert fa_scan.COLS_SCAN_MIN_COLS == 5


def test_an_unknown_name_still_raises():
    with pytest.raises(ValueError, match="unknown option"):
        with flox_amd.set_options(cols_scan_bogus=True):
            pass
