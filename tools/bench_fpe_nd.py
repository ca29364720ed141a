#!/usr/bin/env python3
"""Time per Horner pass of the grid-resident Fokker-Planck propagator (blindno_fp_propagate_nd).

    python tools/bench_fpe_nd.py [--iters 10] [--warmup 3] [--out profiles/fpe_nd_bench.json]

One call with nout = 2 enqueues substeps x degree passes (plus one copy of p0); the call is timed
with a pair of events (min / median / max) and divided by the pass count.  Reported per grid: ms
per pass and the achieved bytes/s, counting per cell the 7 coefficients, p, the cell's own w and
the result (10 doubles = 80 B -- the six neighbour values are re-reads of lines another cell
streams).  Grids: 40^3 with B = 8 (the figure blindno.fpe.MAX_TOTAL_PASSES_ND is derived from, see
DESIGN 4c), 128^2 with B = 32, and 80^2 with B = 32 on both kernels: there the LDS-resident
blindno_fp_propagate runs the same substeps in one launch.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))

import torch

DEGREE = 18
BYTES_PER_CELL = 80


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def problem(B, dims, rows):
    """Random in-rates below 1 with diag their sum bound (||M||_1 <= 2 x 6), a normalised p0."""
    N = dims[0] * dims[1] * dims[2]
    g = torch.Generator(device="cuda").manual_seed(0)
    coef = torch.zeros(B, rows, N, dtype=torch.float64, device="cuda")
    live = 1 + 2 * sum(1 for n in dims if n > 1)
    coef[:, 1:live] = torch.rand(B, live - 1, N, dtype=torch.float64, device="cuda", generator=g)
    coef[:, 0] = coef[:, 1:].sum(1)
    p0 = torch.rand(B, N, dtype=torch.float64, device="cuda", generator=g)
    return coef, p0 / p0.sum(1, keepdim=True)


def bench(B, dims, substeps, iters, warmup, lds=False):
    from blindno._lib import call, ptr, query, stream_ptr
    N = dims[0] * dims[1] * dims[2]
    coef, p0 = problem(B, dims, 5 if lds else 7)
    out = torch.empty(B, 2, N, dtype=torch.float64, device="cuda")
    dt_out = substeps * 0.5 / 24.0
    if lds:
        def run():
            call("blindno_fp_propagate", ptr(p0), ptr(coef), ptr(out), B, dims[0], dims[1], 2, substeps, DEGREE,
                 dt_out, stream_ptr())
    else:
        scratch = torch.empty(query("blindno_fp_propagate_nd_scratch_doubles", B, *dims), dtype=torch.float64,
                              device="cuda")

        def run():
            call("blindno_fp_propagate_nd", ptr(p0), ptr(coef), ptr(out), ptr(scratch), B, *dims, 2, substeps,
                 DEGREE, dt_out, stream_ptr())
    ms = timed(run, iters, warmup)
    assert bool(torch.isfinite(out).all())
    passes = substeps * DEGREE
    med = statistics.median(ms)
    return {"B": B, "grid": list(dims), "cells": N, "passes_per_call": passes,
            "call_ms": {"min": round(min(ms), 4), "median": round(med, 4), "max": round(max(ms), 4), "iters": len(ms)},
            "ms_per_pass": round(med / passes, 6),
            "bytes_per_s": round(B * N * BYTES_PER_CELL / (med / passes * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpe_nd_bench.json"))
    a = ap.parse_args()

    import blindno
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    res = {"device": torch.cuda.get_device_name(0), "degree": DEGREE, "bytes_counted_per_cell": BYTES_PER_CELL,
           "nd_40x40x40_B8": bench(8, (40, 40, 40), a.substeps, a.iters, a.warmup),
           "nd_128x128_B32": bench(32, (128, 128, 1), a.substeps, a.iters, a.warmup),
           "nd_80x80_B32": bench(32, (80, 80, 1), a.substeps, a.iters, a.warmup),
           "lds_80x80_B32": bench(32, (80, 80, 1), a.substeps, a.iters, a.warmup, lds=True)}
    res["nd_over_lds_80x80"] = round(res["nd_80x80_B32"]["ms_per_pass"] / res["lds_80x80_B32"]["ms_per_pass"], 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
            f.write("\n")


if __name__ == "__main__":
    main()
