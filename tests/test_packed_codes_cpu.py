"""Packed label codes without a GPU: the shared pack/unpack header, built as
a stand-alone host program under AddressSanitizer and UBSan and run directly,
and the cache's width selection and byte accounting."""

import os
import shutil
import subprocess

import pytest
import torch

import flox_amd
from flox_amd import label_cache
from flox_amd.label_cache import EMIT, FIRST, HIT, LabelCodeCache

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def test_header_round_trip_under_sanitizers(tmp_path):
    exe = str(tmp_path / "packed_codes_host")
    subprocess.run(
        [_host_compiler(), "-std=c++17", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "packed_codes_host.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed codes host checks OK" in r.stdout


@pytest.mark.parametrize("ngroups,width", [
    (1, 12), (4094, 12), (4095, 14), (10_000, 14), (16382, 14), (16383, 16), (40_000, 16),
])
def test_width_selection(ngroups, width):
    with flox_amd.set_options(label_code_pack_min_rows=1):
        assert label_cache.code_width(ngroups, 1) == width
        assert label_cache.code_width(ngroups, 10**9) == width


def test_width_is_16_below_the_row_threshold():
    # the default threshold stays above the sizes at which the uint16 form's
    # 2 B/row is pinned by tests/test_label_cache_gpu.py
    assert label_cache.PACK_MIN_ROWS > 5_200_005
    t = label_cache.PACK_MIN_ROWS
    assert label_cache.code_width(100, t - 1) == 16
    assert label_cache.code_width(100, t) == 12
    assert label_cache.code_width(10_000, t) == 14
    with flox_amd.set_options(label_code_pack_min_rows=1000):
        assert label_cache.PACK_MIN_ROWS == 1000
        assert label_cache.code_width(100, 999) == 16
        assert label_cache.code_width(100, 1000) == 12
    assert label_cache.PACK_MIN_ROWS == t  # restored


@pytest.mark.parametrize("n,tiles", [(0, 0), (1, 1), (1023, 1), (1024, 1), (1025, 2),
                                     (10**9, 976_563)])
def test_code_bytes(n, tiles):
    assert label_cache.code_bytes(n, 12) == tiles * 128 * 12
    assert label_cache.code_bytes(n, 14) == tiles * 128 * 14
    assert label_cache.code_bytes(n, 16) == 2 * n


def _labels(n=5000, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)


def test_acquire_accounts_the_bytes_it_is_given():
    c = LabelCodeCache()
    lab = _labels()
    n = lab.numel()
    nb = label_cache.code_bytes(n, 14)
    assert nb == 5 * 1792 and nb != 2 * n
    assert c.acquire((lab,), 10_000, n, nbytes=nb, width=14).action == FIRST
    plan = c.acquire((lab,), 10_000, n, nbytes=nb, width=14)
    assert plan.action == EMIT and plan.width == 14
    codes = torch.zeros(nb, dtype=torch.uint8)
    c.publish(plan, codes)
    assert c.stats()["bytes"] == nb
    plan = c.acquire((lab,), 10_000, n, nbytes=nb, width=14)
    assert plan.action == HIT and plan.width == 14 and plan.codes is codes
    c.clear()
    assert c.stats()["bytes"] == 0


def test_default_accounting_is_uint16():
    c = LabelCodeCache()
    lab = _labels()
    c.acquire((lab,), 10, lab.numel())
    plan = c.acquire((lab,), 10, lab.numel())
    assert plan.action == EMIT and plan.width == 16
    c.publish(plan, torch.zeros(lab.numel(), dtype=torch.int32))
    assert c.stats()["bytes"] == 2 * lab.numel()
    assert c.acquire((lab,), 10, lab.numel()).width == 16


def test_packed_bytes_count_against_the_budget():
    n = 4096
    nb12 = label_cache.code_bytes(n, 12)  # 6144 against 8192 as uint16
    a, b = _labels(n, 1), _labels(n, 2)
    # room for two packed streams, but not for two uint16 ones
    c = LabelCodeCache(max_bytes=2 * nb12)
    for lab in (a, b):
        c.acquire((lab,), 10, n, nbytes=nb12, width=12)
        c.publish(c.acquire((lab,), 10, n, nbytes=nb12, width=12), torch.zeros(nb12, dtype=torch.uint8))
    assert c.stats()["bytes"] == 2 * nb12 and c.stats()["entries"] == 2
    assert c.acquire((a,), 10, n, nbytes=nb12, width=12).action == HIT
    # a third evicts the least recently used (b)
    d = _labels(n, 3)
    c.acquire((d,), 10, n, nbytes=nb12, width=12)
    c.publish(c.acquire((d,), 10, n, nbytes=nb12, width=12), torch.zeros(nb12, dtype=torch.uint8))
    assert c.stats()["bytes"] == 2 * nb12
    assert c.acquire((a,), 10, n, nbytes=nb12, width=12).action == HIT
    assert c.acquire((b,), 10, n, nbytes=nb12, width=12).action == FIRST
    # a stream larger than the whole budget is never tracked
    small = LabelCodeCache(max_bytes=nb12 - 1)
    assert small.acquire((a,), 10, n, nbytes=nb12, width=12).action == FIRST
    assert small.stats()["entries"] == 0


def test_another_width_starts_over():
    # the packing threshold moved between two sightings: codes of the old
    # width must not be served as the new one
    c = LabelCodeCache()
    lab = _labels()
    n = lab.numel()
    c.acquire((lab,), 10, n)
    c.publish(c.acquire((lab,), 10, n), torch.zeros(n, dtype=torch.int32))
    assert c.acquire((lab,), 10, n).action == HIT
    nb = label_cache.code_bytes(n, 12)
    assert c.acquire((lab,), 10, n, nbytes=nb, width=12).action == FIRST
    assert c.stats()["bytes"] == 0
    plan = c.acquire((lab,), 10, n, nbytes=nb, width=12)
    assert plan.action == EMIT and plan.width == 12
