#!/usr/bin/env python3
"""The fused plane MLP and the NIOFP3D_Trans training step on the native kernels (csrc/planemlp.hip,
csrc/physattn.hip, csrc/conv3d.hip) beside the same computation composed from torch on the same GPU.

    python tools/bench_trans3d.py [--grid auto|40|32|20] [--rounds 4] [--block 3] [--warmup 2]
                                  [--out profiles/trans3d_bench.json]

B = 4, a fixed recorded bag of L = 75 snapshots drawn with replacement from T = 100, on a cubic grid:
the largest of 40^3, 32^3 and 20^3 whose torch-composed step is estimated (POINT_FLOATS floats kept
per point and snapshot) to fit into half the free device memory; a side that still runs out of memory
sends the tool to the next smaller grid.

1. ``ops.PlaneMLPFn`` alone, forward + backward, on S = B L = 300 snapshots of 32 channel planes
   (LayerNorm, Linear, GELU, Linear, residual: one launch each way plus the partial sum) beside the
   five launches it replaces: ``ops.LayerNormPlanesFn``, a 1x1x1 ``ops.conv3d``, torch's GELU,
   another 1x1x1 ``ops.conv3d`` and torch's add.
2. The whole NIOFP3D_Trans(3, 12, 8, 2) step (forward, MSE, backward) beside the model composed
   from torch.nn.functional (linear, gelu, layer_norm, conv3d and the reference's attention
   sequence, activations (S, N, C) as in the reference).  Both sides encode the distinct snapshots
   of the bag once and weight them by multiplicity; the bag mean and the FNO3d head are the native
   ones in both.

Timing as in tools/bench_trans2d.py: alternating blocks, an event pair per step, medians over all
steps of a side and the spread of the per-block medians; peak memory is torch's
max_memory_allocated over one further step.
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
import torch.nn.functional as F

from bench_trans2d import alternate, kernel_times, torch_phys_attn

B, T, L = 4, 100, 75
GRIDS = (40, 32, 20)
POINT_FLOATS = 2000      # floats the torch-composed step keeps per point and snapshot (three blocks)
ENTRIES = ("blindno_plane_mlp_fwd", "blindno_plane_mlp_bwd", "blindno_physattn_fwd", "blindno_physattn_bwd",
           "blindno_ln_planes_fwd", "blindno_ln_planes_bwd", "blindno_conv3d_fwd", "blindno_conv3d_bwd_data",
           "blindno_conv3d_bwd_weight")


def torch_encoder3d(t, inp):
    """Transolver3D's forward on its parameters from torch.nn.functional: inp (S, N, 4) -> (S, N, 1)."""
    def mlp(mm, h):
        return F.linear(F.gelu(F.linear(h, mm.linear_pre[0].weight, mm.linear_pre[0].bias)),
                        mm.linear_post.weight, mm.linear_post.bias)
    S = inp.shape[0]
    fx = mlp(t.preprocess, inp)
    for blk in t.blocks:
        a = blk.Attn
        h = F.layer_norm(fx, (32,), blk.ln_1.weight, blk.ln_1.bias, blk.ln_1.eps)
        img = h.reshape(S, t.H, t.W, t.D, 32).permute(0, 4, 1, 2, 3).contiguous()
        xf = torch.cat((F.conv3d(img, a.in_project_x.weight, a.in_project_x.bias, padding=1),
                        F.conv3d(img, a.in_project_fx.weight, a.in_project_fx.bias, padding=1)), 1)
        fx = torch_phys_attn(xf.view(S, 64, t.H, t.W * t.D), a.temperature, a.in_project_slice.weight,
                             a.in_project_slice.bias, a.to_q.weight, a.to_k.weight, a.to_v.weight,
                             a.to_out[0].weight, a.to_out[0].bias) + fx
        fx = mlp(blk.mlp, F.layer_norm(fx, (32,), blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps)) + fx
        if blk.last_layer:
            fx = F.linear(F.layer_norm(fx, (32,), blk.ln_3.weight, blk.ln_3.bias, blk.ln_3.eps),
                          blk.mlp2.weight, blk.mlp2.bias)
    return fx


def run(n, a):
    import blindno
    from blindno import nio, ops
    dev = "cuda"
    torch.manual_seed(0)
    res = {"grid": [n, n, n], "B": B, "bag": L, "device": torch.cuda.get_device_name(0),
           "blocks": {"rounds": a.rounds, "steps_per_block": a.block}}
    P = n ** 3

    # ---- 1. the op alone
    S = B * L
    g = torch.Generator(device="cpu").manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x = r(S, 32, n, n, n).requires_grad_(True)
    prm = [p.requires_grad_(True) for p in (r(32, 32) / 32 ** 0.5, 0.1 * r(32), r(32, 32) / 32 ** 0.5, 0.1 * r(32),
                                            1.0 + 0.3 * r(32), 0.1 * r(32))]
    W1, b1, W2, b2, gamma, beta = prm
    dy = r(S, 32, n, n, n)
    leaves = [x] + prm

    def op_fused():
        for t in leaves:
            t.grad = None
        ops.PlaneMLPFn.apply(x, W1, b1, W2, b2, x, gamma, beta, 1e-5).backward(dy)

    def five(xx):
        h = ops.LayerNormPlanesFn.apply(xx, gamma, beta, 1e-5)
        h = ops.conv3d(h, W1.view(32, 32, 1, 1, 1), b1, 1, 0)
        return ops.conv3d(F.gelu(h), W2.view(32, 32, 1, 1, 1), b2, 1, 0) + xx

    def op_five():
        for t in leaves:
            t.grad = None
        five(x).backward(dy)

    op_fused()
    gn = [t.grad.clone() for t in leaves]
    op_five()
    agree = max(float((a_ - t.grad).norm() / t.grad.norm()) for a_, t in zip(gn, leaves))
    with torch.no_grad():
        yn = ops.PlaneMLPFn.apply(x, W1, b1, W2, b2, x, gamma, beta, 1e-5)
        agree_f = float((yn - five(x)).norm() / yn.norm())
    del gn, yn
    op = alternate({"fused": op_fused, "five_launches": op_five}, a.rounds, a.block, a.warmup)
    spread = max(op["fused"]["block_spread_ms"], op["five_launches"]["block_spread_ms"])
    plane_mib = S * 32 * P * 4 / 2 ** 20
    op.update({"snapshots": S, "plane_tensor_mib": round(plane_mib, 1),
               "forward_rel_l2_fused_vs_five": agree_f, "worst_gradient_rel_l2_fused_vs_five": agree,
               "fused_faster_beyond_block_spread":
                   op["fused"]["step"]["median_ms"] + spread < op["five_launches"]["step"]["median_ms"],
               "fused_peaks_lower": op["fused"]["peak_memory_mib"] < op["five_launches"]["peak_memory_mib"]})
    res["plane_mlp_fwd_bwd"] = op
    del x, dy, leaves, prm, W1, b1, W2, b2, gamma, beta
    torch.cuda.empty_cache()

    # ---- 2. the whole step
    m = blindno.NIOFP3D_Trans(3, 12, 8, 2, dev, (n, n, n)).to(dev).train()
    xb = torch.randn(B, T, n, n, n, device=dev)
    ax = np.linspace(-1, 1, n, dtype=np.float32)
    grid = torch.from_numpy(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), 3)).to(dev)
    y = torch.randn(B, n, n, n, 2, device=dev)
    idx = np.random.RandomState(0).choice(T, L)
    uniq, lw = nio.dedup_bag(idx)
    bag = (torch.as_tensor(uniq, device=dev), torch.as_tensor(lw, device=dev))
    Lu = len(uniq)

    def composed_forward():
        xs = xb.index_select(1, bag[0]).reshape(B * Lu, P, 1)
        pts = torch.cat((xs, grid.reshape(1, P, 3).expand(B * Lu, P, 3)), -1)
        u = torch_encoder3d(m.trans_input, pts)
        h = ops.BagMeanFn.apply(u.reshape(B, Lu, P), grid.reshape(P, 3), m.fc0.weight.data, m.fc0.bias.data,
                                bag[1])
        return m.fno(h.view(B, n, n, n, -1))

    def native():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(m(xb, grid, bag_idx=bag), y, None).backward()

    def composed():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(composed_forward(), y, None).backward()

    with torch.no_grad():
        o_n, o_t = m(xb, grid, bag_idx=bag), composed_forward()
    fwd_agree = float((o_n - o_t).norm() / o_t.norm())
    del o_n, o_t
    step = alternate({"native": native, "torch_functional": composed}, a.rounds, a.block, a.warmup)
    step.update({"model": f"NIOFP3D_Trans(3, 12, 8, 2, grid_shape=({n}, {n}, {n}))", "x": [B, T, n, n, n],
                 "distinct_snapshots": Lu, "bag_idx": [int(i) for i in idx],
                 "block_plane_tensor_mib": round(B * Lu * 32 * P * 4 / 2 ** 20, 1),
                 "forward_rel_l2_native_vs_torch": fwd_agree})
    res["step"] = step
    res["native_entry_points"] = kernel_times(native, ENTRIES, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="auto")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans3d_bench.json"))
    a = ap.parse_args()

    import blindno
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    free = torch.cuda.mem_get_info()[0]
    choice = []
    grids = GRIDS if a.grid == "auto" else (int(a.grid),)
    res = None
    for n in grids:
        est = B * L * n ** 3 * POINT_FLOATS * 4           # an upper bound: the bag's distinct snapshots are fewer
        rec = {"grid": n, "estimated_torch_step_gib": round(est / 2 ** 30, 1), "free_gib": round(free / 2 ** 30, 1)}
        choice.append(rec)
        if a.grid == "auto" and est > free / 2:
            rec["verdict"] = "estimate above half the free memory"
            continue
        try:
            res = run(n, a)
            rec["verdict"] = "ran"
            break
        except torch.cuda.OutOfMemoryError:
            rec["verdict"] = "out of memory"
            torch.cuda.empty_cache()
    assert res is not None, choice
    res["shape_choice"] = choice
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
