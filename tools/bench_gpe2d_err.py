#!/usr/bin/env python3
"""The record-free 2D GPE error path (gpe.solve_error_batch_2d, blindno_gpe2d_error) beside the
recorded path it replaces, at the evaluator's defaults on the dataset's grid.

    python tools/bench_gpe2d_err.py [--iters 5] [--warmup 2] [--out profiles/gpe2d_err_bench.json]

256^2 cells, 1000 Strang steps of dt = 0.005, every 10th step (101 frames), B = 6 trajectories in two
groups of three (two test indices, two models).  Both compositions end with the four errors of the
non-reference trajectories on the host:
  error   solve_error_batch_2d, then time_averaged_L2_error_from_sums per trajectory
  record  solve_batch_2d (the fp64 |psi| record), then time_averaged_L2_error_2d per trajectory
          against its group's first
Each is timed with a pair of events around the whole composition (uploads, allocations and the
final copies included), after warm-up calls, and the median of the repeats is reported; the peak
device memory of each is torch's allocator's (inputs included).  No threshold: whatever is measured
goes into the file.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from bench_fpe_err import _stats
from bench_fpe_nd import timed

B, GROUP = 6, 3


def run(n, nsteps, rec_every, iters, warmup):
    from blindno import gpe
    from blindno._lib import query
    x = np.linspace(-10, 10, n)
    V = gpe.training_potentials_2d(B, x, x, np.random.RandomState(0))
    f = gpe.initial_condition
    psi0 = f(2, x)[:, None] * f(2, x)[None, :]
    dt = 0.005
    args = (psi0, x, x, dt, dt * (nsteps + 0.5), 2, 2.0, 2.0, V)
    pairs = [b for b in range(B) if b % GROUP]
    vals = {}

    def error_path():
        r = gpe.solve_error_batch_2d(*args, group=GROUP, rec_every=rec_every)
        vals["error"] = [gpe.time_averaged_L2_error_from_sums(r["t"], r["num"][b], r["den"][b]) for b in pairs]

    def record_path():
        r = gpe.solve_batch_2d(*args, rec_every=rec_every)
        vals["record"] = [gpe.time_averaged_L2_error_2d(r["t"], r["abs"][b // GROUP * GROUP], r["t"], r["abs"][b],
                                                        (x, x)) for b in pairs]

    nrec = nsteps // rec_every + 1
    res = {"B": B, "group": GROUP, "grid": [n, n], "steps": nsteps, "order": 2, "rec_every": rec_every,
           "frames": nrec, "launches": {"error": query("blindno_gpe2d_error_launches", nsteps, 2, rec_every),
                                        "record": query("blindno_gpe2d_launches", nsteps, 2) + len(pairs)},
           "record_bytes": B * nrec * n ** 2 * 8,
           "scratch_bytes": {"error": 8 * query("blindno_gpe2d_error_scratch_doubles", B, n, n),
                             "record": 8 * query("blindno_gpe2d_scratch_doubles", B, n, n)}}
    for name, fn in (("error", error_path), ("record", record_path)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        ms = timed(fn, iters, warmup)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res[name] = {"wall_ms": _stats(ms), "peak_device_bytes": int(torch.cuda.max_memory_allocated())}
    res["errors"] = vals
    res["max_relative_difference"] = max(abs(a - b) / b for a, b in zip(vals["error"], vals["record"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rec-every", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpe2d_err_bench.json"))
    a = ap.parse_args()

    import blindno
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    res = {"device": torch.cuda.get_device_name(0),
           f"evaluator_{a.n}x{a.n}_B{B}": run(a.n, a.steps, a.rec_every, a.iters, a.warmup)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
            f.write("\n")


if __name__ == "__main__":
    main()
