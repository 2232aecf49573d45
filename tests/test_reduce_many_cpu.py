"""groupby_reduce_many: what can be checked without a GPU — argument
validation (it runs before any device work), the export and the option."""

import numpy as np
import pytest

import flox_amd
from flox_amd import core as fa_core

VALS = np.arange(6, dtype=np.float64)
LAB = np.array([0, 1, 0, 1, 2, 2])


def test_symbol_is_exported():
    assert flox_amd.groupby_reduce_many is fa_core.groupby_reduce_many
    assert fa_core.FUSED_MANY_FUNCS == {
        "count", "sum", "nansum", "mean", "nanmean", "var", "nanvar", "std",
        "nanstd", "min", "nanmin", "max", "nanmax"}
    assert fa_core.FUSED_MANY_FUNCS <= set(flox_amd.REDUCTIONS)


@pytest.mark.parametrize("funcs", [(), [], ""])
def test_empty_funcs(funcs):
    with pytest.raises(ValueError, match="at least one"):
        flox_amd.groupby_reduce_many(VALS, LAB, funcs=funcs)


def test_duplicate_funcs():
    with pytest.raises(ValueError, match="more than once.*mean"):
        flox_amd.groupby_reduce_many(VALS, LAB, funcs=("mean", "std", "mean"))


def test_unknown_func():
    # the same error the single-func call raises for that name
    with pytest.raises(NotImplementedError, match="nope"):
        flox_amd.groupby_reduce_many(VALS, LAB, funcs=("mean", "nope"))
    with pytest.raises(NotImplementedError):
        flox_amd.groupby_reduce_many(VALS, LAB, funcs=("mean", 3))


@pytest.mark.parametrize("arg,value", [
    ("fill_value", {"max": 0.0}),
    ("dtype", {"mean": np.float32, "var": np.float64}),
    ("min_count", {"count": 1, "sum": 1}),
    ("finalize_kwargs", {"var": {"ddof": 1}}),
])
def test_dict_key_not_in_funcs(arg, value):
    with pytest.raises(ValueError, match=f"{arg} has keys that are not in funcs"):
        flox_amd.groupby_reduce_many(VALS, LAB, funcs=("mean", "std", "count"), **{arg: value})


def test_per_func_resolution():
    funcs = ("mean", "var")
    assert fa_core._per_func("fill_value", -1.0, funcs) == {"mean": -1.0, "var": -1.0}
    assert fa_core._per_func("fill_value", {"var": 2}, funcs) == {"mean": None, "var": 2}
    assert fa_core._per_func("min_count", None, funcs) == {"mean": None, "var": None}
    # finalize_kwargs is a dict either way: keyed by func only when nested
    assert fa_core._per_func("finalize_kwargs", {"ddof": 1}, funcs) == {
        "mean": {"ddof": 1}, "var": {"ddof": 1}}
    assert fa_core._per_func("finalize_kwargs", {"var": {"ddof": 1}}, funcs) == {
        "mean": None, "var": {"ddof": 1}}


def test_fused_many_option_round_trips():
    assert "fused_many" in flox_amd.OPTIONS
    assert fa_core.FUSED_MANY is True
    with flox_amd.set_options(fused_many=False):
        assert fa_core.FUSED_MANY is False
        with flox_amd.set_options(fused_many=True):
            assert fa_core.FUSED_MANY is True
        assert fa_core.FUSED_MANY is False
        with flox_amd.set_options(fused_many=None):  # None = leave as it is
            assert fa_core.FUSED_MANY is False
    assert fa_core.FUSED_MANY is True
    # it sits beside the other options and disturbs none of them
    with flox_amd.set_options(fused_many=False, fused_finalize=False):
        assert (fa_core.FUSED_MANY, fa_core.FUSED_FINALIZE) == (False, False)
    assert (fa_core.FUSED_MANY, fa_core.FUSED_FINALIZE) == (True, True)
    with pytest.raises(ValueError, match="unknown option"):
        with flox_amd.set_options(fused_lots=True):
            pass
