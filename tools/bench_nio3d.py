#!/usr/bin/env python3
"""Forward + backward time of NIOFP3D at the reference's 40^3 grid, and each Conv3d layer's share.

    python tools/bench_nio3d.py [--iters 10] [--warmup 3] [--out profiles/nio3d_bench.json]

Model: NIOFP3D(3, 3, 100, 25, 2, 8, 4, 1) in train mode on x (4, 100, 40, 40, 40) with a fixed bag
of L = 75 snapshots (2d_FPE/NIOModules.py:720-788: B L = 300 volumes through Encoder3D).  The
step is timed with a pair of events around forward + backward (min / median / max).  Then every
ConvBlock3D convolution is timed on its own at the shape it has inside that step -- forward,
input gradient and weight gradient through ops.conv3d -- and reported with its dense FLOP count
(2 N Co Do Ho Wo Ci KD KH KW per pass), the TFLOP/s that gives, the fraction of the 157.3 TFLOP/s
fp32 matrix peak and its share of the step's median.
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

FP32_PEAK_TFLOPS = 157.3
CTOR = (3, 3, 100, 25, 2, 8, 4, 1, "cuda")
B, T, N, L = 4, 100, 40, 75
BLOCKS = ("convblock1", "convblock2_1", "convblock2_2", "convblock3_1", "convblock3_2", "convblock4_1",
          "convblock4_2", "convblock7_1", "convblock7_2", "convblock7_3")


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


def conv_layers(m, step_ms, iters, warmup):
    """Each block's convolution alone (forward + both gradients) at its in-step shape."""
    from blindno import ops
    rows = []
    shape = (B * L, 1, N, N, N)
    for name in BLOCKS:
        conv = getattr(m.branch, name).layers[0]
        # the snapshots need no gradient: the first block runs no input-gradient pass in the step
        passes = 2 if name == BLOCKS[0] else 3
        x = torch.randn(*shape, device="cuda", requires_grad=passes == 3)
        w, b = conv.weight.detach().requires_grad_(True), conv.bias.detach().requires_grad_(True)
        y = ops.conv3d(x, w, b, conv.stride, conv.padding)
        dy = torch.randn_like(y)

        def run():
            x.grad = w.grad = b.grad = None
            ops.conv3d(x, w, b, conv.stride, conv.padding).backward(dy)

        ms = statistics.median(timed(run, iters, warmup))
        flop = passes * 2.0 * y.numel() * conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1] * conv.kernel_size[2]
        tf = flop / (ms * 1e-3) / 1e12
        rows.append({"layer": name, "in": list(shape), "out": list(y.shape), "kernel": list(conv.kernel_size),
                     "stride": list(conv.stride), "fwd_bwd_ms": round(ms, 4), "gflop": round(flop / 1e9, 2),
                     "tflops": round(tf, 2), "frac_fp32_peak": round(tf / FP32_PEAK_TFLOPS, 3),
                     "share_of_step": round(ms / step_ms, 4)})
        shape = tuple(y.shape)
        del x, y, dy
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nio3d_bench.json"))
    a = ap.parse_args()

    import blindno
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    m = blindno.NIOFP3D(*CTOR).cuda().train()
    x = torch.randn(B, T, N, N, N, device="cuda")
    ax = torch.linspace(-1, 1, N, device="cuda")
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).contiguous()
    idx = torch.as_tensor(np.random.RandomState(0).choice(T, L), device="cuda")
    cot = torch.randn(B, N, N, N, CTOR[7], device="cuda")

    def step():
        for p in m.parameters():
            p.grad = None
        (m(x, grid, bag_idx=idx) * cot).sum().backward()

    res = {"model": f"NIOFP3D{CTOR[:8]}", "x": [B, T, N, N, N], "bag": L,
           "device": torch.cuda.get_device_name(0), "step": summary(timed(step, a.iters, a.warmup))}
    res["conv_layers"] = conv_layers(m, res["step"]["median_ms"], max(3, a.iters // 2), 2)
    res["conv_share_of_step"] = round(sum(r["share_of_step"] for r in res["conv_layers"]), 4)
    big = sorted(res["conv_layers"], key=lambda r: -r["gflop"])[:3]
    res["largest_three"] = {r["layer"]: r["frac_fp32_peak"] for r in big}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
