#!/usr/bin/env python3
"""Forward + backward time and peak memory of NIOFP2D_attn's bag attention in coefficient space
(csrc/nioattn.hip, ops.NIOAttnFn) against the composition the ops allowed before it: the DeepONet
field materialised with torch, (w @ basis^T + b0) / sqrt(P), then ops.BagAttnFn (csrc/attn.hip).

    python tools/bench_nio2d_attn.py [--iters 50] [--rounds 10] [--out profiles/nio2d_attn_bench.json]

Shape: config D's (128^2 grid, B = 4, L = 75 snapshots drawn with replacement, P = 25, width 12).
``op``: the attention alone, forward + backward from a fixed cotangent, inputs w (B, L, P), basis
(S, P), b0 requiring gradients.  ``model_step``: the whole NIOFP2D_attn(2, 3, 100, 25, 3, 12, 32, 2)
eager training step (forward, MSE loss, backward) on x (4, 100, 128, 128), once with the model as it
is and once with its attention swapped for the materialised composition.  The two variants are
timed in alternating blocks (--rounds blocks of --iters calls each for the op, a tenth as many calls
for the model step; one event pair per block; min / median / max of the block means), and a
speed-up is reported only where the two ranges do not overlap.  Peak memory is torch's
max_memory_allocated over one call above what was allocated before it: the allocator's view, not
the kernels' private scratch (csrc/nioattn.hip's kernels use none).  One JSON line on stdout, the
same object in --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))

import numpy as np
import torch

CTOR = (2, 3, 100, 25, 3, 12, 32, 2)
B, T, N, L, P, WIDTH = 4, 100, 128, 75, 25, 12


def timed_pair(fns, iters, warmup, rounds):
    """Time the variants of ``fns`` (name -> callable) in alternating blocks: ``rounds`` times, one
    block of ``iters`` calls of each variant in turn, one event pair per block, so that drift of the
    device's clocks falls on every variant alike.  Per variant: min / median / max of the block
    means, and the peak memory of one more call on its own, above what was allocated before it."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    out = {}
    for k, fn in fns.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[k] = {"min_ms": round(min(ms[k]), 4), "median_ms": round(statistics.median(ms[k]), 4),
                  "max_ms": round(max(ms[k]), 4), "blocks": rounds, "calls_per_block": iters,
                  "peak_bytes": int(torch.cuda.max_memory_allocated() - base)}
    return out


def compare(r):
    """Speed-up of the coefficient path, or none where the two ranges of block means overlap."""
    c, d = r["coefficient"], r["materialised"]
    r["peak_bytes_saved"] = d["peak_bytes"] - c["peak_bytes"]
    r["ranges_overlap"] = not (c["max_ms"] < d["min_ms"] or d["max_ms"] < c["min_ms"])
    r["speedup_median"] = None if r["ranges_overlap"] else round(d["median_ms"] / c["median_ms"], 3)
    r["verdict"] = ("no measurable difference" if r["ranges_overlap"] else
                    "coefficient path faster" if c["max_ms"] < d["min_ms"] else "coefficient path slower")


def materialised(ops, w, basis, b0, grid, fw, fb):
    """The parent composition: the (B, L, S) field, then the bag attention on it."""
    u = (w @ basis.t() + b0) / math.sqrt(w.shape[-1])
    return ops.BagAttnFn.apply(u, grid, fw, fb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls per timed block of the op")
    ap.add_argument("--rounds", type=int, default=10, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nio2d_attn_bench.json"))
    a = ap.parse_args()

    import blindno
    from blindno import ops
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    S = N * N
    ax = torch.linspace(-1, 1, N, device="cuda")
    grid = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).contiguous()
    g2 = grid.reshape(S, 2)
    w = (0.3 * torch.randn(B, L, P, device="cuda")).requires_grad_(True)
    basis = torch.randn(S, P, device="cuda").requires_grad_(True)
    b0 = torch.zeros((), device="cuda").requires_grad_(True)
    fw, fb = torch.randn(WIDTH, 1, device="cuda"), torch.randn(WIDTH, device="cuda")
    dy = torch.randn(B, S, WIDTH, device="cuda")

    def op(fn):
        def run():
            w.grad = basis.grad = b0.grad = None
            fn(w, basis, b0, g2, fw, fb).backward(dy)
        return run

    res = {"shape": {"B": B, "L": L, "S": S, "P": P, "width": WIDTH},
           "device": torch.cuda.get_device_name(0),
           "op": timed_pair({"coefficient": op(ops.NIOAttnFn.apply),
                             "materialised": op(lambda *t: materialised(ops, *t))},
                            a.iters, a.warmup, a.rounds)}
    y0 = ops.NIOAttnFn.apply(w, basis, b0, g2, fw, fb)
    y1 = materialised(ops, w, basis, b0, g2, fw, fb)
    res["op"]["rel_l2_between_them"] = float((y0.detach() - y1.detach()).norm() / y1.detach().norm())
    del y0, y1

    m = blindno.NIOFP2D_attn(*CTOR, branch_last_kernel=blindno.Encoder2D.kernel_for_grid(N)).cuda().train()
    x = torch.randn(B, T, N, N, device="cuda")
    idx = np.random.RandomState(0).choice(T, L)
    target = torch.randn(B, N, N, 2, device="cuda")

    def step():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(m(x, grid, bag_idx=idx), target, None).backward()

    res["model"] = f"NIOFP2D_attn{CTOR}"
    real = ops.NIOAttnFn.apply
    swapped = staticmethod(lambda *t: materialised(ops, *t))

    def step_materialised():
        ops.NIOAttnFn.apply = swapped
        try:
            step()
        finally:
            ops.NIOAttnFn.apply = real

    res["model_step"] = timed_pair({"coefficient": step, "materialised": step_materialised},
                                   max(2, a.iters // 10), max(2, a.warmup // 2), a.rounds)
    compare(res["op"])
    compare(res["model_step"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
