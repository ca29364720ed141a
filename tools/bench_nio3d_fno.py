#!/usr/bin/env python3
"""Training-step time of NIOFP3D_FNO at the 40^3 grid with the bag-level 3D projection
(csrc/bagproj3d.hip, ops.BagEncoder3dFn) and with the forced fallback (ops.BAG3D_STATS = False:
FNO3dFn on the distinct snapshots + BagMeanFn, the composition the ops allowed before).

    python tools/bench_nio3d_fno.py [--iters 10] [--warmup 3] [--out profiles/nio3d_fno_bench.json]

Model: NIOFP3D_FNO(2, 8, 4, 2, input_modes=4) in train mode on x (4, 100, 40, 40, 40) with a fixed
bag of L = 75 snapshots drawn with replacement (deduplicated to its distinct snapshots, as every
step is).  One step = forward, MSE loss, backward, timed with a pair of events (min / median /
max).  After the step timing, a few more steps run with events around the projection launches
alone: blindno_project_bag3d_fwd / _bwd, or the encoder's blindno_project3d_fwd / _bwd launches
(the largest launch of each entry per step; the head's 4-sample launches are the small ones).
Peak memory is torch's max_memory_allocated over the timed steps of each mode.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))

import numpy as np
import torch

CTOR = (2, 8, 4, 2)
INPUT_MODES = 4
B, T, N, L = 4, 100, 40, 75
KERNELS = {True: ("blindno_project_bag3d_fwd", "blindno_project_bag3d_bwd"),
           False: ("blindno_project3d_fwd", "blindno_project3d_bwd")}


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


def summary(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4),
            "max_ms": round(max(ms), 4), "iters": len(ms)}


class _LaunchEvents:
    """A blindno._lib hook: an event pair around every launch of one entry point."""

    def __init__(self):
        self.pairs = []

    def before(self, args):
        self._e0 = torch.cuda.Event(enable_timing=True)
        self._e0.record()

    def after(self, args):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.pairs.append((self._e0, e1))


def kernel_times(step, names, iters):
    """Per entry point, the largest launch of each step: min / median / max over ``iters`` steps."""
    from blindno import _lib
    out = {}
    per_step = {n: [] for n in names}
    for _ in range(iters):
        hooks = {n: _LaunchEvents() for n in names}
        _lib._HOOKS.update(hooks)
        try:
            step()
        finally:
            for n in names:
                _lib._HOOKS.pop(n, None)
        torch.cuda.synchronize()
        for n, h in hooks.items():
            per_step[n].append(max(a.elapsed_time(b) for a, b in h.pairs))
    for n, ms in per_step.items():
        out[n] = summary(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nio3d_fno_bench.json"))
    a = ap.parse_args()

    import blindno
    from blindno import ops
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    m = blindno.NIOFP3D_FNO(*CTOR, "cuda", input_modes=INPUT_MODES).cuda().train()
    x = torch.randn(B, T, N, N, N, device="cuda")
    ax = torch.linspace(-1, 1, N, device="cuda")
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).contiguous()
    idx = np.random.RandomState(0).choice(T, L)
    y = torch.randn(B, N, N, N, CTOR[3], device="cuda")

    def step():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(m(x, grid, bag_idx=idx), y, None).backward()

    res = {"model": f"NIOFP3D_FNO{CTOR} input_modes={INPUT_MODES}", "x": [B, T, N, N, N], "bag": L,
           "distinct_snapshots": int(len(np.unique(idx))), "device": torch.cuda.get_device_name(0)}
    for key, bag_level in (("bag_level", True), ("fallback", False)):
        ops.BAG3D_STATS = bag_level
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        r = {"step": summary(timed(step, a.iters, a.warmup)),
             "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
        r["projection_kernels"] = kernel_times(step, KERNELS[bag_level], max(3, a.iters // 2))
        res[key] = r
    ops.BAG3D_STATS = True
    res["stats_mib"] = round(4 * blindno._lib.query("blindno_project_bag3d_stats_floats", B, N, N, N) / 2 ** 20, 1)
    res["bag_level_is_faster"] = res["bag_level"]["step"]["min_ms"] < res["fallback"]["step"]["min_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
