#!/usr/bin/env python3
"""The record-free Fokker-Planck error path (blindno_fp_error_nd) at the 3D dataset's shape, beside
what an evaluator would otherwise do with blindno_fp_propagate_nd's record.

    python tools/bench_fpe_err.py [--iters 10] [--warmup 3] [--out profiles/fpe_err_bench.json]

40^3 cells, B = 6 trajectories in groups of 3 (two test indices, two models), degree 18.
  * per pass: one call with nout = 2 enqueues substeps x degree Horner passes, the copy of p0 and two
    reductions (4 launches); timed with a pair of events as tools/bench_fpe_nd.py does and divided
    by the pass count.  The same for blindno_fp_propagate_nd at the same B, and one reduction alone
    (nout = 1: the copy and the two reduction launches).
  * a short run, both compositions, host wall time from the call to the numbers on the host:
      error   blindno_fp_error_nd, err (B, nout, 2) copied to the host, the metric from the sums
      record  blindno_fp_propagate_nd, the (B, nout, N) record copied to the host, the metric with
              numpy norms (timeerror.time_averaged_relative_l2)
    with the peak device memory of each (torch's allocator, inputs included).
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))

import numpy as np
import torch

from bench_fpe_nd import DEGREE, problem, timed

B, GROUP, DIMS = 6, 3, (40, 40, 40)
N = DIMS[0] * DIMS[1] * DIMS[2]


def _stats(ms, passes=None):
    med = statistics.median(ms)
    r = {"min": round(min(ms), 4), "median": round(med, 4), "max": round(max(ms), 4), "iters": len(ms)}
    return (r, round(med / passes, 6)) if passes else r


def per_pass(substeps, iters, warmup):
    from blindno._lib import call, ptr, query, stream_ptr
    coef, p0 = problem(B, DIMS, 7)
    dt_out = substeps * 0.5 / 24.0
    err = torch.empty(B, 2, 2, dtype=torch.float64, device="cuda")
    s_err = torch.empty(query("blindno_fp_error_nd_scratch_doubles", B, *DIMS), dtype=torch.float64, device="cuda")
    out = torch.empty(B, 2, N, dtype=torch.float64, device="cuda")
    s_rec = torch.empty(query("blindno_fp_propagate_nd_scratch_doubles", B, *DIMS), dtype=torch.float64, device="cuda")

    def run_err(nout=2):
        call("blindno_fp_error_nd", ptr(p0), ptr(coef), ptr(err), ptr(s_err), B, GROUP, *DIMS, nout, substeps, DEGREE,
             dt_out, stream_ptr())

    def run_rec():
        call("blindno_fp_propagate_nd", ptr(p0), ptr(coef), ptr(out), ptr(s_rec), B, *DIMS, 2, substeps, DEGREE,
             dt_out, stream_ptr())
    passes = substeps * DEGREE
    e_call, e_pass = _stats(timed(run_err, iters, warmup), passes)
    assert bool(torch.isfinite(err).all()) and bool((err[::GROUP, :, 0] == 0).all())
    r_call, r_pass = _stats(timed(run_rec, iters, warmup), passes)
    red = _stats(timed(lambda: run_err(1), iters, warmup))
    return {"B": B, "group": GROUP, "grid": list(DIMS), "cells": N, "passes_per_call": passes,
            "error_nd": {"call_ms": e_call, "ms_per_pass": e_pass},
            "propagate_nd_same_B": {"call_ms": r_call, "ms_per_pass": r_pass},
            "copy_and_one_reduction_ms": red}


def short_run(nout, substeps, iters, warmup):
    from blindno import timeerror
    from blindno._lib import call, ptr, query, stream_ptr
    coef, p0 = problem(B, DIMS, 7)
    dt_out = substeps * 0.5 / 24.0

    def error_path():
        err = torch.empty(B, nout, 2, dtype=torch.float64, device="cuda")
        scratch = torch.empty(query("blindno_fp_error_nd_scratch_doubles", B, *DIMS), dtype=torch.float64,
                              device="cuda")
        call("blindno_fp_error_nd", ptr(p0), ptr(coef), ptr(err), ptr(scratch), B, GROUP, *DIMS, nout, substeps,
             DEGREE, dt_out, stream_ptr())
        e = err.cpu().numpy()
        return [float(np.mean(np.sqrt(e[b, :, 0]) / (np.sqrt(e[b, :, 1]) + 1e-12))) for b in range(B)]

    def record_path():
        out = torch.empty(B, nout, N, dtype=torch.float64, device="cuda")
        scratch = torch.empty(query("blindno_fp_propagate_nd_scratch_doubles", B, *DIMS), dtype=torch.float64,
                              device="cuda")
        call("blindno_fp_propagate_nd", ptr(p0), ptr(coef), ptr(out), ptr(scratch), B, *DIMS, nout, substeps, DEGREE,
             dt_out, stream_ptr())
        rec = out.cpu().numpy()
        return [timeerror.time_averaged_relative_l2(rec[b], rec[b // GROUP * GROUP]) for b in range(B)]

    res = {"nout": nout, "substeps": substeps, "passes": (nout - 1) * substeps * DEGREE}
    vals = {}
    for name, fn in (("error", error_path), ("record", record_path)):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(iters):
            t0 = time.perf_counter()
            vals[name] = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"wall_ms": _stats(ms), "peak_device_bytes": int(torch.cuda.max_memory_allocated())}
    res["max_metric_difference"] = max(abs(a - b) for a, b in zip(vals["error"], vals["record"]))
    res["record_bytes"] = B * nout * N * 8
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--nout", type=int, default=41, help="frames of the short run")
    ap.add_argument("--run-substeps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpe_err_bench.json"))
    a = ap.parse_args()

    import blindno
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    res = {"device": torch.cuda.get_device_name(0), "degree": DEGREE,
           "per_pass_40x40x40_B6": per_pass(a.substeps, a.iters, a.warmup),
           "short_run_40x40x40_B6": short_run(a.nout, a.run_substeps, a.iters, a.warmup)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
            f.write("\n")


if __name__ == "__main__":
    main()
