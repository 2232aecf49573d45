"""Timing probe: quantile / median / mode over leading dims, the sort-in-LDS
column form (set_options(cols_sorted_funcs=True), the default) against the
lead fold (False), on time-major climatology shapes read through a permute
view; and nanmedian against mean on the (8760, 720, 1440) hour-of-day shape
only the column form can run. Each figure: warm-up runs, then `--runs` timed
runs one by one; median, min and max are reported, so the spread is on the
page.

    python tools/cols_sorted_probe.py [--runs 7] [--skip-big] [--out FILE]
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

FUNCS = (
    ("nanmedian", None),
    ("nanquantile", {"q": [0.1, 0.5, 0.9]}),
    ("mode", None),
)


def timed(fn, runs, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "runs": runs}


def make(shape, dtype, nan, gen, ngroups):
    """(time, lat, lon) storage; the (lat, lon, time) permute view and labels.
    Values are rounded to 1/64 so that modes exist."""
    n_t = shape[0]
    store = torch.empty(shape, dtype=dtype, device="cuda")
    # filled plane by plane: no full-size temporary beside the array
    for i in range(n_t):
        plane = torch.rand(shape[1:], generator=gen, device="cuda", dtype=torch.float32)
        store[i].copy_(torch.round(plane * 64) / 64)
        if nan:
            store[i][torch.rand(shape[1:], generator=gen, device="cuda") < nan] = float("nan")
    lab = torch.arange(n_t, device="cuda") % ngroups
    return store, store.permute(1, 2, 0), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--skip-big", action="store_true")
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

    # (shape, dtype, NaN fraction, groups): segments of 84, 84 and 60 rows,
    # then the same arrays in 2 groups (1000 / 720 rows per segment)
    cases = [
        ((2000, 512, 512), torch.float32, 0.05, 24),
        ((2000, 512, 512), torch.float64, 0.05, 24),
        ((1440, 720, 2000), torch.float32, 0.0, 24),
        ((2000, 512, 512), torch.float32, 0.05, 2),
        ((2000, 512, 512), torch.float64, 0.05, 2),
    ]
    for shape, dtype, nan, ng in cases:
        store, view, lab = make(shape, dtype, nan, gen, ng)
        nbytes = store.numel() * store.element_size()
        for func, fk in FUNCS:
            kw = dict(expected_groups=range(ng), finalize_kwargs=fk)
            for on in (True, False):
                with flox_amd.set_options(cols_sorted_funcs=on):
                    r = timed(lambda: flox_amd.groupby_reduce(view, lab, func=func, **kw), args.runs)
                emit(shape=shape, dtype=str(dtype)[6:], nan=nan, groups=ng,
                     seg_rows=-(-shape[0] // ng), func=func,
                     path="cols" if on else "fold", **r,
                     read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))
        del store, view
        torch.cuda.empty_cache()

    if not args.skip_big:
        shape = (8760, 720, 1440)
        store, view, lab = make(shape, torch.float32, 0.0, gen, 24)
        nbytes = store.numel() * store.element_size()
        for func in ("mean", "nanmedian"):
            r = timed(lambda: flox_amd.groupby_reduce(view, lab, func=func, expected_groups=range(24)),
                      args.runs)
            emit(shape=shape, dtype="float32", nan=0.0, groups=24, seg_rows=365, func=func,
                 path="cols", **r, read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))


if __name__ == "__main__":
    main()
