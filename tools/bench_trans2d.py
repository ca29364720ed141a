#!/usr/bin/env python3
"""Physics attention and the NIOFP2D_Trans training step at the reference grid on the native kernels
(csrc/physattn.hip) beside the same computation composed from torch on the same GPU.

    python tools/bench_trans2d.py [--rounds 4] [--block 3] [--warmup 2] [--out profiles/trans2d_bench.json]

61 x 61 grid, B = 4, a fixed recorded bag of L = 75 snapshots drawn with replacement from T = 100.

1. ``ops.PhysAttnFn`` alone, forward + backward, on S = B L = 300 snapshots: input the 64-channel
   output of the two 3x3 convolutions as planes, gradients for it and for all eight parameters.
   The torch side is the reference's own sequence from the same planes (permute to (S, heads, N, 8),
   softmax, einsum, matmul, rearrange, to_out), its output left in the reference's (S, N, 32)
   layout.
2. The whole NIOFP2D_Trans(2, 3, 100, 25, 3, 12, 32, 2) step (forward, MSE, backward) beside the
   model composed from torch.nn.functional (linear, gelu, layer_norm, conv2d and the sequence
   above, activations (S, N, C) as in the reference).  Both sides encode the distinct snapshots of
   the bag once and weight them by multiplicity; the bag mean and the FNO heads are the native
   ones in both.

The two sides are timed in alternating blocks of ``block`` steps, ``rounds`` times, each step with
a pair of events; medians over all steps of a side, and the spread of the per-block medians of a
side.  Peak memory is torch's max_memory_allocated over one further step.  A few native steps then
run with events around every launch of the entry points the encoder uses, summed per entry and step.
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
import torch.nn.functional as F

B, T, N, L = 4, 100, 61, 75
HEADS, D, G = 4, 8, 16
ENTRIES = ("blindno_physattn_fwd", "blindno_physattn_bwd", "blindno_ln_planes_fwd", "blindno_ln_planes_bwd",
           "blindno_conv2d_fwd_split", "blindno_conv2d_bwd_data_split", "blindno_conv2d_bwd_weight")


def summary(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4),
            "max_ms": round(max(ms), 4), "iters": len(ms)}


def time_block(fn, n):
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def alternate(steps, rounds, block, warmup):
    for fn in steps.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    blocks = {k: [] for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            b = time_block(fn, block)
            ms[k] += b
            blocks[k].append(statistics.median(b))
    out = {}
    for k, fn in steps.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[k] = {"step": summary(ms[k]), "block_medians_ms": [round(v, 4) for v in blocks[k]],
                  "block_spread_ms": round(max(blocks[k]) - min(blocks[k]), 4),
                  "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    return out


def torch_phys_attn(xf, temperature, Ws, bs, Wq, Wk, Wv, Wo, bo):
    """Physics_Attention_Structured_Mesh_2D.forward after its convolutions: xf (S, 64, H, W) ->
    (S, N, 32)."""
    S, _, H, W = xf.shape
    n = H * W

    def mid(t):
        return t.permute(0, 2, 3, 1).contiguous().reshape(S, n, HEADS, D).permute(0, 2, 1, 3).contiguous()
    x_mid, fx_mid = mid(xf[:, :HEADS * D]), mid(xf[:, HEADS * D:])
    sw = torch.softmax(F.linear(x_mid, Ws, bs) / torch.clamp(temperature, min=0.1, max=5), dim=-1)
    norm = sw.sum(2)
    tok = torch.einsum("bhnc,bhng->bhgc", fx_mid, sw)
    tok = tok / ((norm + 1e-5)[:, :, :, None].repeat(1, 1, 1, D))
    q, k, v = F.linear(tok, Wq), F.linear(tok, Wk), F.linear(tok, Wv)
    attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * D ** -0.5, dim=-1)
    out = torch.einsum("bhgc,bhng->bhnc", torch.matmul(attn, v), sw)
    return F.linear(out.permute(0, 2, 1, 3).reshape(S, n, HEADS * D), Wo, bo)


def torch_encoder(t, inp):
    """Transolver2D's forward on its parameters from torch.nn.functional: inp (S, N, 3) -> (S, N, 1)."""
    def mlp(mm, h):
        return F.linear(F.gelu(F.linear(h, mm.linear_pre[0].weight, mm.linear_pre[0].bias)),
                        mm.linear_post.weight, mm.linear_post.bias)
    S = inp.shape[0]
    fx = mlp(t.preprocess, inp)
    for blk in t.blocks:
        a = blk.Attn
        h = F.layer_norm(fx, (32,), blk.ln_1.weight, blk.ln_1.bias, blk.ln_1.eps)
        img = h.reshape(S, t.H, t.W, 32).permute(0, 3, 1, 2).contiguous()
        xf = torch.cat((F.conv2d(img, a.in_project_x.weight, a.in_project_x.bias, padding=1),
                        F.conv2d(img, a.in_project_fx.weight, a.in_project_fx.bias, padding=1)), 1)
        fx = torch_phys_attn(xf, a.temperature, a.in_project_slice.weight, a.in_project_slice.bias,
                             a.to_q.weight, a.to_k.weight, a.to_v.weight, a.to_out[0].weight,
                             a.to_out[0].bias) + fx
        fx = mlp(blk.mlp, F.layer_norm(fx, (32,), blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps)) + fx
        if blk.last_layer:
            fx = F.linear(F.layer_norm(fx, (32,), blk.ln_3.weight, blk.ln_3.bias, blk.ln_3.eps),
                          blk.mlp2.weight, blk.mlp2.bias)
    return fx


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
    from blindno import _lib
    per_step = {n: [] for n in names}
    calls = {}
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
            per_step[n].append(sum(a.elapsed_time(b) for a, b in h.pairs))
            calls[n] = len(h.pairs)
    return {n: {"calls_per_step": calls[n], "sum_ms_per_step": round(statistics.median(ms), 4)}
            for n, ms in per_step.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans2d_bench.json"))
    a = ap.parse_args()

    import blindno
    from blindno import nio, ops
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    dev = "cuda"
    res = {"grid": [N, N], "B": B, "bag": L, "device": torch.cuda.get_device_name(0),
           "blocks": {"rounds": a.rounds, "steps_per_block": a.block}}

    # ---- 1. the op alone
    S = B * L
    g = torch.Generator(device="cpu").manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    xf = r(S, 64, N, N).requires_grad_(True)
    prm = [p.requires_grad_(True) for p in (torch.tensor([0.5, 0.3, 0.8, 1.2]).view(1, 4, 1, 1).to(dev), 0.5 * r(G, D),
                                            0.1 * r(G), 0.6 * r(D, D), 0.6 * r(D, D), 0.6 * r(D, D),
                                            0.3 * r(32, 32), 0.1 * r(32))]
    dy = r(S, 32, N, N)
    dy_pts = dy.reshape(S, 32, N * N).transpose(1, 2).contiguous()
    leaves = [xf] + prm

    def op_native():
        for t in leaves:
            t.grad = None
        ops.PhysAttnFn.apply(xf, *prm).backward(dy)

    def op_torch():
        for t in leaves:
            t.grad = None
        torch_phys_attn(xf, *prm).backward(dy_pts)

    op_native()
    gn = [t.grad.clone() for t in leaves]
    op_torch()
    agree = max(float((a_ - t.grad).norm() / t.grad.norm()) for a_, t in zip(gn, leaves))
    with torch.no_grad():
        yn = ops.PhysAttnFn.apply(xf, *prm).reshape(S, 32, N * N).transpose(1, 2)
        agree_f = float((yn - torch_phys_attn(xf, *prm)).norm() / yn.norm())
    op = alternate({"native": op_native, "torch": op_torch}, a.rounds, a.block, a.warmup)
    spread = max(op["native"]["block_spread_ms"], op["torch"]["block_spread_ms"])
    op.update({"snapshots": S, "forward_rel_l2_native_vs_torch": agree_f, "worst_gradient_rel_l2_native_vs_torch": agree,
               "native_not_slower_beyond_block_spread":
                   op["native"]["step"]["median_ms"] <= op["torch"]["step"]["median_ms"] + spread,
               "native_peaks_lower": op["native"]["peak_memory_mib"] < op["torch"]["peak_memory_mib"]})
    res["phys_attn_fwd_bwd"] = op
    del xf, dy, dy_pts, leaves, gn, yn
    torch.cuda.empty_cache()

    # ---- 2. the whole step
    m = blindno.NIOFP2D_Trans(2, 3, 100, 25, 3, 12, 32, 2).to(dev).train()
    x = torch.randn(B, T, N, N, device=dev)
    ax = np.linspace(-1, 1, N, dtype=np.float32)
    grid = torch.from_numpy(np.stack(np.meshgrid(ax, ax, indexing="ij"), 2)).to(dev)
    y = torch.randn(B, N, N, 2, device=dev)
    idx = np.random.RandomState(0).choice(T, L)
    uniq, lw = nio.dedup_bag(idx)
    bag = (torch.as_tensor(uniq, device=dev), torch.as_tensor(lw, device=dev))
    Lu = len(uniq)

    def composed_forward():
        xs = x.index_select(1, bag[0]).reshape(B * Lu, N * N, 1)
        pts = torch.cat((xs, grid.reshape(1, N * N, 2).expand(B * Lu, N * N, 2)), -1)
        u = torch_encoder(m.trans_input, pts)
        return nio._run_heads(m, nio._bag_mean_2d(m, u, grid, B, Lu, N, N, bag[1]))

    def native():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(m(x, grid, bag_idx=bag), y, None).backward()

    def composed():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(composed_forward(), y, None).backward()

    with torch.no_grad():
        o_n, o_t = m(x, grid, bag_idx=bag), composed_forward()
    step = alternate({"native": native, "torch_functional": composed}, a.rounds, a.block, a.warmup)
    step.update({"model": "NIOFP2D_Trans(2, 3, 100, 25, 3, 12, 32, 2)", "x": [B, T, N, N], "distinct_snapshots": Lu,
                 "bag_idx": [int(i) for i in idx],
                 "forward_rel_l2_native_vs_torch": float((o_n - o_t).norm() / o_t.norm())})
    res["step"] = step
    res["native_entry_points"] = kernel_times(native, ENTRIES, 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
