"""Exercise the REAL RCCL backend: every prior
distributed test ran gloo on CPU; these run `init_process_group("nccl")`
(= RCCL on ROCm) on actual hardware.

world-size 1 always runs (RCCL init + the coalesced all-reduce + the
inf-filled min/max bin conventions execute on the real backend). The
world-size-2-on-one-GPU variant runs when RCCL permits two ranks on one
device (it typically refuses duplicate GPUs, in which case it SKIPs with
the refusal recorded); the real multi-device scaling run is the driver's.
"""

import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _seed_data(n=2_000_000, ng=10_000):
    rng = np.random.default_rng(77)
    vals = rng.standard_normal(n).astype(np.float32)
    vals[rng.random(n) < 0.03] = np.nan
    labels = rng.integers(0, ng, n)
    return vals, labels, ng


def test_nccl_world1_combine():
    """world=1 over the real RCCL: distributed_combine=True executes the
    collectives (self-reduction) — results must equal the plain path."""
    import torch.distributed as dist

    import flox_amd

    assert torch.cuda.is_available()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29611")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        # real RCCL collectives (identity at world 1): the sum/min/max ops
        # and the inf-filled bin convention execute on the actual backend
        t = torch.arange(1000, dtype=torch.float64, device="cuda")
        dist.all_reduce(t)
        np.testing.assert_allclose(t.cpu().numpy(), np.arange(1000.0))
        t_inf = torch.full((64,), float("inf"), device="cuda")
        dist.all_reduce(t_inf, op=dist.ReduceOp.MIN)
        assert bool(torch.isinf(t_inf).all().item())
        t_key = torch.full((64,), (1 << 63) - 1, dtype=torch.int64, device="cuda")
        dist.all_reduce(t_key, op=dist.ReduceOp.MIN)  # packed-arg sentinel bins
        assert int(t_key.max().item()) == (1 << 63) - 1
        if hasattr(dist, "all_reduce_coalesced"):
            a = torch.ones(128, dtype=torch.float64, device="cuda")
            b = torch.full((64,), 2.0, dtype=torch.float64, device="cuda")
            dist.all_reduce_coalesced([a, b])
            assert float(a.sum().item()) == 128.0 and float(b.sum().item()) == 128.0
        torch.cuda.synchronize()

        vals, labels, ng = _seed_data()
        eg = np.arange(ng)
        for func in ["nanmean", "sum", "min", "var", "count", "argmin",
                     "nanargmax", "first", "nanlast"]:
            plain, *_ = flox_amd.groupby_reduce(
                vals, labels, func=func, expected_groups=eg,
                distributed_combine=False)
            comb, *_ = flox_amd.groupby_reduce(
                vals, labels, func=func, expected_groups=eg,
                distributed_combine=True)
            np.testing.assert_array_equal(
                np.asarray(plain), np.asarray(comb), err_msg=func)
        # grouped scan carry exchange over RCCL (self)
        s_plain = flox_amd.groupby_scan(vals, labels, func="cumsum",
                                        expected_groups=eg,
                                        distributed_combine=False)
        s_comb = flox_amd.groupby_scan(vals, labels, func="cumsum",
                                       expected_groups=eg,
                                       distributed_combine=True)
        np.testing.assert_allclose(s_plain, s_comb, equal_nan=True,
                                   rtol=1e-12, atol=1e-12)
    finally:
        dist.destroy_process_group()


def _worker2(rank, world, port, fail_q, ok_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(0)  # both ranks share the single device
        try:
            dist.init_process_group("nccl", rank=rank, world_size=world)
            t = torch.ones(8, device="cuda")
            dist.all_reduce(t)  # RCCL may only object at first collective
            torch.cuda.synchronize()
        except Exception as e:
            ok_q.put(("refused", f"{type(e).__name__}: {e}"))
            return
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import flox_amd
        from oracle import groupby_reduce as oracle_reduce

        vals, labels, ng = _seed_data()
        eg = np.arange(ng)
        n = len(vals)
        sl = slice(rank * n // world, (rank + 1) * n // world)
        for func in ["nanmean", "sum", "min", "count", "argmin", "nanargmax"]:
            got, *_ = flox_amd.groupby_reduce(
                vals[sl], labels[sl], func=func, expected_groups=eg,
                shard_row_offset=sl.start)
            want, *_ = oracle_reduce(vals, labels, func=func, expected_groups=eg)
            np.testing.assert_allclose(
                np.asarray(got), want, equal_nan=True, rtol=1e-6, atol=1e-6,
                err_msg=func)
        dist.destroy_process_group()
        ok_q.put(("ok", rank))
    except Exception as e:  # pragma: no cover
        import traceback

        fail_q.put(f"rank {rank}: {type(e).__name__}: {e}\n{traceback.format_exc()}")
        raise


def test_nccl_world2_single_device():
    """Two ranks on one MI355X over RCCL: the full distributed combine
    (coalesced all-reduce, packed-arg key min) against the whole-data
    oracle. SKIPs if RCCL refuses duplicate devices."""
    ctx = mp.get_context("spawn")
    fail_q, ok_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_worker2, args=(r, 2, 29613, fail_q, ok_q))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    for p in procs:
        if p.is_alive():  # pragma: no cover
            p.terminate()
            pytest.skip("RCCL world-2-on-one-device hung (rendezvous refused)")
    outcomes = []
    while not ok_q.empty():
        outcomes.append(ok_q.get())
    errs = []
    while not fail_q.empty():
        errs.append(fail_q.get())
    if any(o[0] == "refused" for o in outcomes):
        pytest.skip(f"RCCL refuses 2 ranks on one device: {outcomes}")
    assert not errs, errs[0]
    assert sum(1 for o in outcomes if o[0] == "ok") == 2, outcomes
