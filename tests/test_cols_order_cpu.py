"""set_options(cols_order_funcs=...): the switch between the column forms of
the arg-reductions / first / last over leading dims and the lead fold."""

import pytest

import flox_amd
from flox_amd import _ffi
from flox_amd import core as fa_core


def test_cols_order_funcs_option_is_accepted_and_restored():
    assert "cols_order_funcs" in flox_amd.OPTIONS
    assert fa_core.COLS_ORDER_FUNCS is True  # the default is on
    with flox_amd.set_options(cols_order_funcs=False):
        assert fa_core.COLS_ORDER_FUNCS is False
        with flox_amd.set_options(cols_order_funcs=True):
            assert fa_core.COLS_ORDER_FUNCS is True
        assert fa_core.COLS_ORDER_FUNCS is False
        with flox_amd.set_options(cols_order_funcs=None):  # None = leave as it is
            assert fa_core.COLS_ORDER_FUNCS is False
    assert fa_core.COLS_ORDER_FUNCS is True
    with pytest.raises(RuntimeError):
        with flox_amd.set_options(cols_order_funcs=False):
            raise RuntimeError("restored on the way out of an exception too")
    assert fa_core.COLS_ORDER_FUNCS is True


def test_unknown_option_still_raises():
    with pytest.raises(ValueError, match="unknown option"):
        with flox_amd.set_options(cols_order_func=True):
            pass
    assert fa_core.COLS_ORDER_FUNCS is True


def test_new_set_numbers_mirror_the_header():
    assert (_ffi.SET_ARGMIN_COLS, _ffi.SET_ARGMAX_COLS) == (15, 16)
