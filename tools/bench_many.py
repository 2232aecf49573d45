"""Probe: five statistics of one array over one set of labels, three ways.

Times, on resident tensors, funcs=("mean","std","min","max","count") as
  singles    five groupby_reduce calls
  many_off   groupby_reduce_many with fused_many=False
  many_fused groupby_reduce_many (one SET_SUMMARY pass)
with the label-code cache warm (same `by` tensor, codes held) and cold
(cleared before every timed repetition), plus the fused kernel pair
(k_reduce_lds + k_combine_tree) on its own with its bytes per row and share
of the measured 6.29 TB/s copy ceiling. Prints one JSON line per workload.

The column workloads (COLS_WORKLOADS: time-major data grouped over axis 0
through a permute view, so the leading dims become the column path's columns)
are timed the same three ways, cache state aside (the column path has no
label-code cache), plus the fused SET_SUMMARY column pass on its own.

--root DIR imports flox_amd from DIR instead of this checkout (a build of
another commit, which may lack groupby_reduce_many: those forms are then
reported as null). Not part of the test suite; bench.py is untouched.
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

COPY_CEILING = 6.29e12  # B/s, measured float4 copy (profiles/r01_rocprof_summary.md)
FUNCS = ("mean", "std", "min", "max", "count")
WORKLOADS = {
    "f32_1e8_1000g": dict(n=100_000_000, dtype="float32", groups=(1000,), nan=0.0),
    "f64_1e8_12x180g_nan5": dict(n=100_000_000, dtype="float64", groups=(12, 180), nan=0.05),
}


# time-major (n_t, *lead) arrays grouped over axis 0: BASELINE config 4's
# hour-of-day climatology, and an f64 shape with NaNs and 12 groups
COLS_WORKLOADS = {
    "cols_f32_8760x720x1440_24g": dict(shape=(8760, 720, 1440), dtype="float32", groups=24, nan=0.0),
    "cols_f64_2000x512x512_12g_nan5": dict(shape=(2000, 512, 512), dtype="float64", groups=12, nan=0.05),
}


def bench_cols(args, torch, flox_amd, name, w):
    from flox_amd import _ffi, aggregate_hip

    many = getattr(flox_amd, "groupby_reduce_many", None)
    n_t = max(int(w["shape"][0] * args.scale), 1)
    shape = (n_t,) + tuple(w["shape"][1:])
    dt = getattr(torch, w["dtype"])
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = torch.empty(shape, dtype=dt, device="cuda")
    for t0 in range(0, n_t, 256):  # in slabs: no second full-size temporary
        blk = base[t0:t0 + 256]
        blk.normal_(generator=gen)
        if w["nan"]:
            blk[torch.rand(blk.shape, device="cuda", generator=gen) < w["nan"]] = float("nan")
    arr = base.permute(*range(1, len(shape)), 0)  # (*lead, n_t): zero copy
    by = (torch.arange(n_t, device="cuda") % w["groups"])
    kw = dict(expected_groups=np.arange(w["groups"]))

    def singles():
        return [flox_amd.groupby_reduce(arr, by, func=f, **kw)[0] for f in FUNCS]

    def many_off():
        with flox_amd.set_options(fused_many=False):
            return flox_amd.groupby_reduce_many(arr, by, funcs=FUNCS, **kw)[0]

    def many_fused():
        return flox_amd.groupby_reduce_many(arr, by, funcs=FUNCS, **kw)[0]

    forms = {"singles": singles}
    if many is not None:
        forms["many_off"] = many_off
        forms["many_fused"] = many_fused
    out = {"workload": name, "shape": list(shape), "root": args.root, "reps": args.reps}

    def timed(fn):
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    meds = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(2):
            fn()
    for _ in range(args.rounds):  # rounds alternate the forms
        for k, fn in forms.items():
            meds[k].append(timed(fn))
    for k in ("singles", "many_off", "many_fused"):
        m = meds.get(k)
        out[f"{k}_ms"] = None if m is None else round(statistics.median(m), 4)
        out[f"{k}_range_ms"] = None if m is None else [round(min(m), 4), round(max(m), 4)]

    # one column pass on its own, device events: the fused set where this
    # build has it, and the mean's SET_SUM_COUNT for scale
    m_cols = base[0].numel()
    vt = base.reshape(n_t, m_cols)
    sc, perm = torch.sort(by, stable=True)
    sc, perm = sc.to(torch.int32), perm.to(torch.int32)
    for label, op in (("summary", _ffi.SET_SUMMARY), ("sum_count", _ffi.SET_SUM_COUNT)):
        def kern():
            return aggregate_hip.grouped_partials_cols(op, vt, sc, perm, w["groups"], skipnan=True)
        try:
            for _ in range(2):
                kern()
        except RuntimeError:  # a build whose column path lacks the set
            out[f"kernel_{label}_ms"] = None
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            kern()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        out[f"kernel_{label}_ms"] = round(ms, 4)
        out[f"kernel_{label}_B_per_element"] = vt.element_size()
        out[f"kernel_{label}_frac_copy_ceiling"] = round(
            vt.numel() * vt.element_size() / (ms * 1e-3) / COPY_CEILING, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink n (rehearsal)")
    ap.add_argument("--only", default=None)
    ap.add_argument("--cols", action="store_true", help="the column workloads only")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch

    import flox_amd
    from flox_amd import _ffi, aggregate_hip

    assert torch.cuda.is_available(), "bench_many needs a GPU"
    many = getattr(flox_amd, "groupby_reduce_many", None)
    gen = torch.Generator(device="cuda").manual_seed(0)

    def sync_time(fn, reps, before=None):
        ts = []
        for _ in range(reps):
            if before is not None:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    for name, w in COLS_WORKLOADS.items():
        if args.only == name or (args.only is None and args.cols):
            bench_cols(args, torch, flox_amd, name, w)

    for name, w in WORKLOADS.items():
        if (args.only and args.only != name) or (args.only is None and args.cols):
            continue
        n = int(w["n"] * args.scale)
        dt = getattr(torch, w["dtype"])
        vals = torch.randn(n, dtype=dt, device="cuda", generator=gen)
        if w["nan"]:
            vals[torch.rand(n, device="cuda", generator=gen) < w["nan"]] = float("nan")
        bys = tuple(torch.randint(0, g, (n,), device="cuda", generator=gen) for g in w["groups"])
        expected = tuple(np.arange(g) for g in w["groups"])
        expected = expected if len(expected) > 1 else expected[0]
        kw = dict(expected_groups=expected)

        def singles():
            return [flox_amd.groupby_reduce(vals, *bys, func=f, **kw)[0] for f in FUNCS]

        def many_off():
            with flox_amd.set_options(fused_many=False):
                return flox_amd.groupby_reduce_many(vals, *bys, funcs=FUNCS, **kw)[0]

        def many_fused():
            return flox_amd.groupby_reduce_many(vals, *bys, funcs=FUNCS, **kw)[0]

        forms = {"singles": singles}
        if many is not None:
            forms["many_off"] = many_off
            forms["many_fused"] = many_fused
        out = {"workload": name, "n": n, "root": args.root, "reps": args.reps}
        for state in ("warm", "cold"):
            before = flox_amd.clear_label_cache if state == "cold" else None
            # rounds alternate the forms, so drift hits all of them alike
            meds = {k: [] for k in forms}
            for k, fn in forms.items():  # warm-up: code objects, cache, allocator
                for _ in range(4):
                    fn()
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    meds[k].append(sync_time(fn, args.reps, before))
            for k in ("singles", "many_off", "many_fused"):
                m = meds.get(k)
                out[f"{state}_{k}_ms"] = None if m is None else round(statistics.median(m), 4)
                out[f"{state}_{k}_range_ms"] = None if m is None else [round(min(m), 4), round(max(m), 4)]

        if many is not None:
            # the fused kernel pair on its own, device events, u16 codes (warm)
            # and the caller's int64 labels (no cache key given)
            ng = int(np.prod(w["groups"]))
            two = len(bys) == 2
            pk = dict(labels2=bys[1] if two else None, grp_shape=tuple(w["groups"]) if two else None)
            for label, src in (("codes", tuple(bys)), ("labels", None)):
                def kern():
                    return aggregate_hip.grouped_partials(
                        _ffi.SET_SUMMARY, vals, bys[0], ng, skipnan=True, label_src=src, **pk)
                for _ in range(4):
                    kern()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    kern()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / args.reps
                brow = vals.element_size() + (2 if label == "codes" else 8 * len(bys))
                out[f"kernel_{label}_ms"] = round(ms, 4)
                out[f"kernel_{label}_B_per_row"] = brow
                out[f"kernel_{label}_frac_copy_ceiling"] = round(n * brow / (ms * 1e-3) / COPY_CEILING, 3)
        print(json.dumps(out), flush=True)
        del vals, bys


if __name__ == "__main__":
    main()
