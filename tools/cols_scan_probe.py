"""Timing probe: cumsum / nancumsum / ffill / bfill over leading dims, the
column form (set_options(cols_scan=True), the default) against the lead fold
(False), on time-major climatology shapes read through a permute view; cumsum
against mean on the (8760, 720, 1440) hour-of-day shape only the column form
can run; and the gate sweep: about 2^26 elements, lead_M from 4 to 16384, 24
and 2 groups, both paths. Each figure is a host clock around a call that ends
in a device synchronise (the whole API call: factorize, sort, kernel): warm-up
runs, then `--runs` timed runs one by one, the two paths alternating; median,
min and max are reported, so the spread is on the page. `frac_copy` is read +
write bytes over the median against the 6.29 TB/s copy ceiling.

    python tools/cols_scan_probe.py [--runs 7] [--part shapes|big|gate|all] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import flox_amd  # noqa: E402

FUNCS = ("cumsum", "nancumsum", "ffill", "bfill")
COPY_CEILING_GBS = 6290.0


def timed_pair(fns, runs, warm=2):
    """times each callable of `fns` `runs` times, alternating between them; one
    that runs out of device memory in its first warm-up is reported as such"""
    failed = {}
    for k in list(fns):
        try:
            fns[k]()
        except torch.cuda.OutOfMemoryError:
            failed[k] = {"error": "out of device memory", "runs": 0, "median_ms": None}
            del fns[k]
            torch.cuda.empty_cache()
    for _ in range(warm - 1):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
               "max_ms": round(max(v), 3), "runs": runs} for k, v in ms.items()}
    out.update(failed)
    return out


def make(shape, dtype, nan, gen):
    """time-major storage (time, ...), filled plane by plane: no full-size
    temporary beside the array"""
    store = torch.empty(shape, dtype=dtype, device="cuda")
    for i in range(shape[0]):
        store[i].copy_(torch.rand(shape[1:], generator=gen, device="cuda", dtype=torch.float32))
        if nan:
            store[i][torch.rand(shape[1:], generator=gen, device="cuda") < nan] = float("nan")
    return store


def scan_call(view, lab, func, ng, on):
    def run():
        with flox_amd.set_options(cols_scan=on, cols_scan_min_cols=1):
            return flox_amd.groupby_scan(view, lab, func=func, expected_groups=range(ng))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--part", default="all", choices=("shapes", "big", "gate", "all"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(3)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
        if args.out:  # rewritten after every figure: a cut-short run keeps its rows
            with open(args.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")

    def frac(nbytes_rw, ms):
        return None if ms is None else round(nbytes_rw / ms / 1e6 / COPY_CEILING_GBS, 3)

    if args.part in ("shapes", "all"):
        cases = [
            ((2000, 512, 512), torch.float32, 0.05, 24),
            ((2000, 512, 512), torch.float64, 0.05, 24),
            ((1440, 720, 2000), torch.float32, 0.0, 24),
        ]
        for shape, dtype, nan, ng in cases:
            store = make(shape, dtype, nan, gen)
            view = store.permute(1, 2, 0)
            lab = torch.arange(shape[0], device="cuda") % ng
            rw = 2 * store.numel() * store.element_size()
            for func in FUNCS:
                r = timed_pair({"cols": scan_call(view, lab, func, ng, True),
                                "fold": scan_call(view, lab, func, ng, False)}, args.runs)
                for path in ("cols", "fold"):
                    emit(part="shapes", shape=shape, dtype=str(dtype)[6:], nan=nan, groups=ng,
                         func=func, path=path, **r[path],
                         frac_copy=frac(rw, r[path]["median_ms"]))
            del store, view
            torch.cuda.empty_cache()

    if args.part in ("big", "all"):
        shape = (8760, 720, 1440)
        store = make(shape, torch.float32, 0.0, gen)
        view = store.permute(1, 2, 0)
        lab = torch.arange(shape[0], device="cuda") % 24
        nbytes = store.numel() * store.element_size()
        r = timed_pair({
            "mean": lambda: flox_amd.groupby_reduce(view, lab, func="mean", expected_groups=range(24)),
            "cumsum": lambda: flox_amd.groupby_scan(view, lab, func="cumsum", expected_groups=range(24)),
        }, args.runs)
        emit(part="big", shape=shape, dtype="float32", groups=24, func="mean", path="cols",
             **r["mean"], frac_copy=frac(nbytes, r["mean"]["median_ms"]))
        emit(part="big", shape=shape, dtype="float32", groups=24, func="cumsum", path="cols",
             **r["cumsum"], frac_copy=frac(2 * nbytes, r["cumsum"]["median_ms"]),
             over_mean=round(r["cumsum"]["median_ms"] / r["mean"]["median_ms"], 2))
        del store, view
        torch.cuda.empty_cache()

    if args.part in ("gate", "all"):
        total = 2**26
        for ng in (24, 2):
            for lead_m in (4, 16, 64, 256, 1024, 4096, 16384):
                n = total // lead_m
                store = make((n, lead_m), torch.float32, 0.0, gen) if n <= 2**16 else (
                    torch.rand((n, lead_m), generator=gen, device="cuda", dtype=torch.float32))
                view = store.permute(1, 0)
                lab = torch.arange(n, device="cuda") % ng
                r = timed_pair({"cols": scan_call(view, lab, "cumsum", ng, True),
                                "fold": scan_call(view, lab, "cumsum", ng, False)}, args.runs)
                for path in ("cols", "fold"):
                    emit(part="gate", elements=total, lead_M=lead_m, rows=n, groups=ng,
                         func="cumsum", path=path, **r[path])
                del store, view
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
