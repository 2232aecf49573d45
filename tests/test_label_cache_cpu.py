"""Label-code cache policy on CPU tensors with a stub code builder (no GPU):
the sighting sequence, invalidation, eviction, the off switch and clear."""

import gc

import pytest
import torch

import flox_amd
from flox_amd import label_cache
from flox_amd.label_cache import EMIT, FIRST, HIT, LabelCodeCache

N = 1000
NG = 10


def _labels(seed=0, n=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, NG, (n,), generator=g, dtype=torch.int64)


def _build(lab):
    """what the emitting kernel writes: the code, 0xFFFF when out of range"""
    bad = (lab < 0) | (lab >= NG)
    return torch.where(bad, torch.full_like(lab, 0xFFFF), lab).to(torch.int32)


def _call(cache, *labs, groups=NG):
    """one reduction's worth of cache traffic; returns (action, codes used)"""
    plan = cache.acquire(labs, groups, labs[0].numel())
    if plan is None:
        return None, None
    if plan.action == EMIT:
        cache.publish(plan, _build(labs[0]))
        return EMIT, None
    return plan.action, plan.codes


def test_first_second_third_sight():
    c = LabelCodeCache()
    lab = _labels()
    assert _call(c, lab) == (FIRST, None)
    assert c.stats() == {"hits": 0, "emits": 0, "misses": 1, "bytes": 0, "entries": 1}
    assert _call(c, lab) == (EMIT, None)
    assert c.stats()["emits"] == 1 and c.stats()["bytes"] == 2 * N
    for k in range(3):
        action, codes = _call(c, lab)
        assert action == HIT
        assert torch.equal(codes, _build(lab))
        assert c.stats()["hits"] == k + 1
    assert c.stats()["misses"] == 1 and c.stats()["emits"] == 1


def test_fresh_view_of_the_same_tensor_is_the_callers_business():
    # the key is the OBJECT: core passes the caller's tensor, not its views
    c = LabelCodeCache()
    lab = _labels()
    _call(c, lab), _call(c, lab)
    assert _call(c, lab)[0] == HIT
    assert _call(c, lab.reshape(-1))[0] == FIRST


def test_inplace_write_is_a_miss():
    c = LabelCodeCache()
    lab = _labels()
    _call(c, lab), _call(c, lab)
    assert _call(c, lab)[0] == HIT
    lab[0] = (int(lab[0]) + 1) % NG  # bumps _version
    assert _call(c, lab) == (FIRST, None)
    assert c.stats()["misses"] == 2 and c.stats()["bytes"] == 0
    assert _call(c, lab)[0] == EMIT
    action, codes = _call(c, lab)
    assert action == HIT and torch.equal(codes, _build(lab))


def test_write_through_a_view_is_a_miss():
    c = LabelCodeCache()
    lab = _labels()
    _call(c, lab), _call(c, lab)
    lab.reshape(-1)[3:5] = 0  # views share the version counter
    assert _call(c, lab)[0] == FIRST


def test_inference_tensor_is_never_cached():
    # no version counter: reading _version raises, writes could not be seen
    c = LabelCodeCache()
    with torch.inference_mode():
        lab = _labels()
    assert lab.is_inference()
    before = c.stats()
    for _ in range(4):
        assert _call(c, lab) == (None, None)
    assert c.stats() == before
    # also as one of two keys
    assert _call(c, _labels(seed=1), lab, groups=(NG, NG)) == (None, None)


def test_storage_swap_is_a_miss():
    # by.data = other keeps the object, _version, shape, strides and dtype
    c = LabelCodeCache()
    lab, other = _labels(seed=10), _labels(seed=11)
    _call(c, lab), _call(c, lab)
    assert _call(c, lab)[0] == HIT
    v = lab._version
    lab.data = other
    assert lab._version == v
    assert _call(c, lab) == (FIRST, None)
    assert c.stats()["bytes"] == 0
    assert _call(c, lab)[0] == EMIT
    action, codes = _call(c, lab)
    assert action == HIT and torch.equal(codes, _build(other))


def test_eviction_survives_a_reentrant_drop():
    # a weak-reference callback may drop entries while _evict walks them
    c = LabelCodeCache(max_entries=2)
    labs = [_labels(seed=s) for s in range(3)]
    for lab in labs[:2]:
        _call(c, lab)
    real_drop = c._drop

    def drop_two(key):  # as if GC killed another entry mid-eviction
        real_drop(key)
        for k in list(c._entries)[:1]:
            real_drop(k)

    c._drop = drop_two
    assert _call(c, labs[2])[0] == FIRST
    c._drop = real_drop
    assert c.stats()["entries"] <= 2


def test_del_and_reallocate_equal_shape_is_a_miss():
    c = LabelCodeCache()
    lab = _labels(seed=1)
    _call(c, lab), _call(c, lab)
    assert c.stats()["entries"] == 1
    del lab
    gc.collect()
    # the weak-reference callback dropped the entry and its codes
    assert c.stats()["entries"] == 0 and c.stats()["bytes"] == 0
    lab2 = _labels(seed=2)  # may well reuse the id / the address
    assert _call(c, lab2) == (FIRST, None)
    assert c.stats()["misses"] == 2


def test_same_id_other_object_never_hits():
    # even with the callback suppressed, identity is checked on lookup
    c = LabelCodeCache()
    lab = _labels(seed=1)
    _call(c, lab), _call(c, lab)
    (key,) = list(c._entries)
    other = _labels(seed=3)
    e = c._entries.pop(key)
    forged = ((id(other),), key[1])
    e.key = forged
    c._entries[forged] = e  # as if `other` had inherited lab's id
    assert _call(c, other)[0] == FIRST


def test_groups_are_part_of_the_key():
    c = LabelCodeCache()
    lab = _labels()
    _call(c, lab), _call(c, lab)
    assert _call(c, lab)[0] == HIT
    assert _call(c, lab, groups=NG + 1)[0] == FIRST


def test_two_by_key():
    c = LabelCodeCache()
    a, b = _labels(seed=4), _labels(seed=5)
    assert _call(c, a, b, groups=(NG, NG))[0] == FIRST
    assert _call(c, a, b, groups=(NG, NG))[0] == EMIT
    assert _call(c, a, b, groups=(NG, NG))[0] == HIT
    assert _call(c, b, a, groups=(NG, NG))[0] == FIRST  # order matters
    b[0] = (int(b[0]) + 1) % NG
    assert _call(c, a, b, groups=(NG, NG))[0] == FIRST  # either tensor invalidates


def test_lru_entry_limit():
    c = LabelCodeCache(max_entries=2)
    labs = [_labels(seed=s) for s in range(3)]
    for lab in labs[:2]:
        _call(c, lab), _call(c, lab)
    assert _call(c, labs[0])[0] == HIT       # 0 is now the most recent
    assert _call(c, labs[2])[0] == FIRST     # evicts 1, the least recent
    assert c.stats()["entries"] == 2
    assert _call(c, labs[0])[0] == HIT
    assert _call(c, labs[1])[0] == FIRST     # was evicted: starts over


def test_byte_budget():
    c = LabelCodeCache(max_entries=8, max_bytes=2 * N + 100)  # room for one
    a, b = _labels(seed=6), _labels(seed=7)
    _call(c, a), _call(c, a)
    assert c.stats()["bytes"] == 2 * N
    _call(c, b), _call(c, b)               # publishing b evicts a's codes
    assert c.stats()["bytes"] == 2 * N
    assert _call(c, b)[0] == HIT
    assert _call(c, a)[0] == FIRST
    # a stream that could never fit is not tracked at all
    big = _labels(seed=8, n=4 * N)
    assert _call(c, big)[0] == FIRST
    assert _call(c, big)[0] == FIRST
    assert c.stats()["bytes"] <= 2 * N + 100


def test_option_off_and_clear():
    lab = _labels(seed=9)
    cache = label_cache.CACHE
    flox_amd.clear_label_cache()
    before = flox_amd.label_cache_stats()
    with flox_amd.set_options(label_cache=False):
        for _ in range(4):
            assert _call(cache, lab) == (None, None)
        assert flox_amd.label_cache_stats() == before
    assert cache.enabled  # restored
    _call(cache, lab), _call(cache, lab)
    assert _call(cache, lab)[0] == HIT
    assert flox_amd.label_cache_stats()["bytes"] == 2 * N
    flox_amd.clear_label_cache()
    st = flox_amd.label_cache_stats()
    assert st["bytes"] == 0 and st["entries"] == 0
    assert _call(cache, lab)[0] == FIRST
    flox_amd.clear_label_cache()


def test_limit_options_apply_and_restore():
    cache = label_cache.CACHE
    e0, b0 = cache.max_entries, cache.max_bytes
    with flox_amd.set_options(label_cache_entries=1, label_cache_bytes=123):
        assert (cache.max_entries, cache.max_bytes) == (1, 123)
    assert (cache.max_entries, cache.max_bytes) == (e0, b0)
    with pytest.raises(ValueError):
        with flox_amd.set_options(label_cache_nope=1):
            pass
