"""Timing probe: the arg-reductions and first/last over leading dims, the
column forms (set_options(cols_order_funcs=True), the default) against the
lead fold (False), on time-major climatology shapes read through a permute
view; and argmax against mean on the (8760, 720, 1440) shape only the column
form can run. Each figure: warm-up runs, then `--runs` timed runs one by one;
median, min and max are reported, so the spread is on the page.

    python tools/cols_order_probe.py [--runs 7] [--skip-big] [--out FILE]
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

FUNCS = ("argmax", "nanargmin", "first", "nanlast")


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


def make(shape, dtype, nan, gen):
    """(time, lat, lon) storage; the (lat, lon, time) permute view and labels"""
    n_t = shape[0]
    store = torch.empty(shape, dtype=dtype, device="cuda")
    # filled plane by plane: no full-size temporary beside the array
    for i in range(n_t):
        store[i].copy_(torch.rand(shape[1:], generator=gen, device="cuda", dtype=torch.float32))
        if nan:
            store[i][torch.rand(shape[1:], generator=gen, device="cuda") < nan] = float("nan")
    lab = torch.arange(n_t, device="cuda") % 24
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

    cases = [
        ((2000, 512, 512), torch.float32, 0.05),
        ((2000, 512, 512), torch.float64, 0.05),
        ((1440, 720, 2000), torch.float32, 0.0),
    ]
    kw = dict(expected_groups=range(24))
    for shape, dtype, nan in cases:
        store, view, lab = make(shape, dtype, nan, gen)
        nbytes = store.numel() * store.element_size()
        for func in FUNCS:
            for on in (True, False):
                with flox_amd.set_options(cols_order_funcs=on):
                    r = timed(lambda: flox_amd.groupby_reduce(view, lab, func=func, **kw), args.runs)
                emit(shape=shape, dtype=str(dtype)[6:], nan=nan, func=func,
                     path="cols" if on else "fold", **r,
                     read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))
        del store, view
        torch.cuda.empty_cache()

    if not args.skip_big:
        shape = (8760, 720, 1440)
        store, view, lab = make(shape, torch.float32, 0.0, gen)
        nbytes = store.numel() * store.element_size()
        for func in ("mean", "argmax"):
            r = timed(lambda: flox_amd.groupby_reduce(view, lab, func=func, **kw), args.runs)
            emit(shape=shape, dtype="float32", nan=0.0, func=func, path="cols", **r,
                 read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
