"""Timing probe: cumsum / ffill over leading dims of C-contiguous (lead..., N)
arrays, the row form (set_options(rows_scan=True), the default) against the
lead fold (False) and against the column form on the permuted copy of the same
data; cumsum on the (720, 1440, 8760) hour-of-day shape only the row form can
run; and the gate sweep: 2^26 elements, f32 and f64, lead_M over powers of two,
2 groups in long runs and 24 cyclic groups, both paths. Each figure is a host
clock around a call that ends in a device synchronise (the whole API call:
factorize, kernel): warm-up runs, then `--runs` timed runs one by one, the
paths alternating; median, min and max are reported, so the spread is on the
page. `frac_copy` is read + write bytes over the median against the 6.29 TB/s
copy ceiling.

    python tools/rows_scan_probe.py [--runs 7] [--part shapes|big|gate|all] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import flox_amd  # noqa: E402
from tools.cols_scan_probe import COPY_CEILING_GBS, timed_pair  # noqa: E402

FUNCS = ("cumsum", "ffill")
GATE_ROWS = (64, 256, 1024, 4096, 16384, 65536)


def make(shape, dtype, nan, gen):
    """C-contiguous (lead..., N), filled block by block: no full-size temporary
    beside the array"""
    arr = torch.empty(shape, dtype=dtype, device="cuda")
    flat = arr.view(-1, shape[-1])
    step = max(1, 2**26 // shape[-1])
    for r in range(0, flat.shape[0], step):
        blk = flat[r:r + step]
        blk.copy_(torch.rand(blk.shape, generator=gen, device="cuda", dtype=torch.float32))
        if nan:
            blk[torch.rand(blk.shape, generator=gen, device="cuda") < nan] = float("nan")
    return arr


def scan_call(arr, lab, func, ng, **opts):
    def run():
        with flox_amd.set_options(**opts):
            return flox_amd.groupby_scan(arr, lab, func=func, expected_groups=range(ng))
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

    if args.part in ("gate", "all"):
        total = 2**26
        for dtype in (torch.float32, torch.float64):
            for pattern, ng in (("runs", 2), ("cyclic", 24)):
                for lead_m in GATE_ROWS:
                    n = total // lead_m
                    arr = make((lead_m, n), dtype, 0.0, gen)
                    t = torch.arange(n, device="cuda")
                    # 2 groups in long runs (eight runs over the axis) / t % 24
                    lab = (t * 8 // n) % 2 if pattern == "runs" else t % ng
                    for func in FUNCS:
                        r = timed_pair({
                            "rows": scan_call(arr, lab, func, ng, rows_scan=True, rows_scan_min_rows=1),
                            "fold": scan_call(arr, lab, func, ng, rows_scan=False),
                        }, args.runs)
                        for path in ("rows", "fold"):
                            emit(part="gate", elements=total, dtype=str(dtype)[6:], lead_M=lead_m,
                                 steps=n, pattern=pattern, groups=ng, func=func, path=path,
                                 **r[path])
                    del arr
                    torch.cuda.empty_cache()

    if args.part in ("shapes", "all"):
        for dtype in (torch.float32, torch.float64):
            shape, ng = (512, 512, 2000), 24
            arr = make(shape, dtype, 0.05, gen)
            store = arr.permute(2, 0, 1).contiguous()  # the same data, time-major
            view = store.permute(1, 2, 0)
            lab = torch.arange(shape[-1], device="cuda") % ng
            rw = 2 * arr.numel() * arr.element_size()
            for func in FUNCS:
                r = timed_pair({
                    "rows": scan_call(arr, lab, func, ng, rows_scan=True),
                    "fold": scan_call(arr, lab, func, ng, rows_scan=False),
                    "cols": scan_call(view, lab, func, ng, cols_scan=True),
                }, args.runs)
                for path in ("rows", "fold", "cols"):
                    emit(part="shapes", shape=shape, dtype=str(dtype)[6:], nan=0.05, groups=ng,
                         func=func, path=path, **r[path],
                         frac_copy=frac(rw, r[path]["median_ms"]))
            del arr, store, view
            torch.cuda.empty_cache()

    if args.part in ("big", "all"):
        shape = (720, 1440, 8760)
        arr = make(shape, torch.float32, 0.0, gen)
        lab = torch.arange(shape[-1], device="cuda") % 24
        nbytes = arr.numel() * arr.element_size()
        r = timed_pair({"cumsum": scan_call(arr, lab, "cumsum", 24, rows_scan=True)}, args.runs)
        emit(part="big", shape=shape, dtype="float32", groups=24, func="cumsum", path="rows",
             **r["cumsum"], frac_copy=frac(2 * nbytes, r["cumsum"]["median_ms"]))
        del arr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
