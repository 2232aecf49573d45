"""Timing probe: quantile / median over leading dims with groups longer than
the sort-in-LDS capacity, the radix-select column form
(set_options(cols_select_funcs=True), the default) against the lead fold
(False), on time-major climatology shapes read through a permute view; a
width sweep at a fixed element count for the cols_select_min_cols gate; the
select entry against the LDS sort at a 2048-row group; and nanmedian against
mean on the (14600, 720, 1440) shape only the column forms can run. Each
figure: warm-up runs, then `--runs` timed runs one by one; median, min and
max are reported, so the spread is on the page. `reads` is how often the
kernel reads the segment (digit passes plus the successor pass);
`read_gbs` is array bytes x reads / median time.

    python tools/cols_select_probe.py [--runs 7] [--skip-big] [--out FILE]
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
from flox_amd import aggregate_hip  # noqa: E402

CAP = 2048
FUNCS = (
    ("nanmedian", None),
    ("nanquantile", {"q": [0.1, 0.5, 0.9]}),
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
    """(time, ...) storage; the (..., time) permute view and labels: `ngroups`
    groups of equal length, interleaved"""
    n_t = shape[0]
    store = torch.empty(shape, dtype=dtype, device="cuda")
    # filled in slabs of rows: no full-size temporary beside the array
    step = max(1, (1 << 26) // max(1, store[0].numel()))
    for i in range(0, n_t, step):
        slab = store[i:i + step]
        slab.copy_(torch.randn(slab.shape, generator=gen, device="cuda", dtype=torch.float32))
        if nan:
            slab[torch.rand(slab.shape, generator=gen, device="cuda") < nan] = float("nan")
    lab = torch.arange(n_t, device="cuda") % ngroups
    dims = tuple(range(1, len(shape))) + (0,)
    return store, store.permute(dims), lab


def reads(dtype):
    return {torch.float32: 5, torch.float64: 9}[dtype]


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

    def both(part, store, view, lab, ng, funcs, paths=(True, False)):
        nbytes = store.numel() * store.element_size()
        for func, fk in funcs:
            kw = dict(expected_groups=range(ng), finalize_kwargs=fk)
            for on in paths:
                with flox_amd.set_options(cols_select_funcs=on, cols_select_min_cols=1):
                    r = timed(lambda: flox_amd.groupby_reduce(view, lab, func=func, **kw), args.runs)
                extra = {}
                if on:
                    extra = dict(reads=reads(store.dtype),
                                 read_gbs=round(nbytes * reads(store.dtype) / r["median_ms"] / 1e6, 1))
                emit(part=part, shape=tuple(store.shape), dtype=str(store.dtype)[6:], groups=ng,
                     seg_rows=-(-store.shape[0] // ng), func=func,
                     path="select" if on else "fold", **r, **extra)

    # width sweep at 2**26 elements: 1 and 4 long groups. A width whose groups
    # fit the LDS sort (<= 2048 rows) never reaches the select kernel: skipped
    for dtype in (torch.float32, torch.float64):
        for width in (64, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            n_t = (1 << 26) // width
            for ng in (1, 4):
                if n_t // ng <= CAP:
                    continue
                store, view, lab = make((n_t, width), dtype, 0.05, gen, ng)
                both("sweep", store, view, lab, ng, FUNCS[:1])
                del store, view
    torch.cuda.empty_cache()

    # the select entry against the LDS sort at a 2048-row group (4 groups)
    for dtype in (torch.float32, torch.float64):
        store, view, lab = make((4 * CAP, 65536), dtype, 0.05, gen, 4)
        sc, perm = torch.sort(lab, stable=True)
        sc, perm = sc.to(torch.int32), perm.to(torch.int32)
        nbytes = store.numel() * store.element_size()
        for name, fn in (
            ("select", lambda: aggregate_hip.grouped_quantile_select_cols(
                store, sc, perm, 4, [0.5], skipnan=True)),
            ("lds_sort", lambda: aggregate_hip.grouped_quantile_cols(
                store, sc, perm, 4, [0.5], skipnan=True, max_seg_rows=CAP)),
        ):
            r = timed(fn, args.runs)
            emit(part="vs_lds_sort", shape=tuple(store.shape), dtype=str(dtype)[6:], groups=4,
                 seg_rows=CAP, func="nanmedian (raw entry)", path=name, **r,
                 read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))
        del store, view
    torch.cuda.empty_cache()

    # climatology shapes: 2 groups of 3000 rows, then the same rows in 1 group
    for dtype in (torch.float32, torch.float64):
        store, view, _ = make((6000, 512, 512), dtype, 0.05, gen, 2)
        for ng in (2, 1):
            lab = torch.arange(6000, device="cuda") % ng
            both("climatology", store, view, lab, ng, FUNCS)
        del store, view
        torch.cuda.empty_cache()

    if not args.skip_big:
        store, view, lab = make((14600, 720, 1440), torch.float32, 0.0, gen, 4)
        nbytes = store.numel() * store.element_size()
        r = timed(lambda: flox_amd.groupby_reduce(view, lab, func="mean", expected_groups=range(4)),
                  args.runs)
        emit(part="big", shape=tuple(store.shape), dtype="float32", groups=4, seg_rows=3650,
             func="mean", path="cols", **r, read_once_gbs=round(nbytes / r["median_ms"] / 1e6, 1))
        both("big", store, view, lab, 4, FUNCS[:1], paths=(True,))


if __name__ == "__main__":
    main()
