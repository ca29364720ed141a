#!/usr/bin/env python3
"""The multiplicity-weighted bag attention (csrc/bagattn_mix.hip) and the NIOFP2D_Trans_attn training
step at the reference grid.

    python tools/bench_trans_attn.py [--rounds 4] [--block 3] [--warmup 2] [--out profiles/trans_attn_bench.json]

61 x 61 grid, B = 4, T = 100, one recorded bag of L = 75 draws with replacement (U distinct).

(a) ``ops.BagAttnMixFn`` forward + backward on the U distinct tokens with their counts, beside the
    reference's own torch sequence (cat, matmul, softmax, matmul, the fusion matrix, autograd) on
    the L + 2 materialised tokens.  Both return y (B, S, width) and the gradient of the snapshot
    tokens; time and peak memory of both.
(b) The whole eager NIOFP2D_Trans_attn(2, 3, 100, 25, 3, 12, 32, 2, 61, 61) step (forward, MSE,
    backward) beside the same model with ``nio.DEDUP_BAGS = False`` (every duplicate encoded and
    attended to as a token of its own).
(c) The same eager step beside NIOFP2D_Trans' step on the same bag.

The sides of each comparison are timed in alternating blocks of ``block`` steps, ``rounds`` times,
each step with a pair of events; medians over all steps of a side, and the spread of the per-block
medians of a side.  Peak memory is torch's max_memory_allocated over one further step.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from bench_trans2d import alternate, kernel_times

B, T, N, L = 4, 100, 61, 75
WIDTH = 12
ENTRIES = ("blindno_bagattn_mix_fwd", "blindno_bagattn_mix_bwd")


def torch_sequence(x, grid, W, bias):
    """2d_FPE/NIOModules.py:243-278 on the materialised tokens: x (B, L, S), grid (S, 2) -> (B, S, width)."""
    Bn, Ln, S = x.shape
    x_flat = torch.cat((grid.t().unsqueeze(0).expand(Bn, 2, S), x), dim=1)
    scores = torch.matmul(x_flat, x_flat.transpose(1, 2)) / math.sqrt(S)
    Z = torch.matmul(torch.softmax(scores, dim=-1), x_flat)
    Wn = torch.cat([W[:, :2], W[:, 2].view(-1, 1).repeat(1, Ln) / Ln], dim=1)
    return torch.matmul(Z.permute(0, 2, 1), Wn.t()) + bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans_attn_bench.json"))
    a = ap.parse_args()

    import blindno
    from blindno import nio, ops
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    dev = "cuda"
    idx = np.random.RandomState(0).choice(T, L)
    uniq, lw_np = nio.dedup_bag(idx)
    U = len(uniq)
    res = {"grid": [N, N], "B": B, "T": T, "bag": L, "distinct_snapshots": U,
           "bag_idx": [int(i) for i in idx], "device": torch.cuda.get_device_name(0),
           "blocks": {"rounds": a.rounds, "steps_per_block": a.block}}

    # ---- (a) the op alone: structured tokens (neither a uniform nor an identity attention)
    S = N * N
    g = torch.Generator(device="cpu").manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    amp = torch.linspace(0.05, 0.35, U)[torch.randperm(U, generator=g)]
    u = (1.5 * (amp.view(1, U, 1) * r(B, 1, S) + 0.02 * r(B, U, S))).to(dev).requires_grad_(True)
    sel = torch.as_tensor(np.searchsorted(uniq, idx), device=dev)          # bag position -> distinct
    ax = np.linspace(-1, 1, N, dtype=np.float32)
    grid = torch.from_numpy(np.stack(np.meshgrid(ax, ax, indexing="ij"), 2)).to(dev)
    gflat = grid.reshape(S, 2)
    W, bias, dy = r(WIDTH, 3).to(dev), r(WIDTH).to(dev), r(B, S, WIDTH).to(dev)
    lw = torch.as_tensor(lw_np, device=dev)

    def op_native():
        u.grad = None
        ops.BagAttnMixFn.apply(u, gflat, W, bias, lw, L).backward(dy)

    def op_torch():
        u.grad = None
        torch_sequence(u.index_select(1, sel), gflat, W, bias).backward(dy)

    op_native()
    gn = u.grad.clone()
    op_torch()
    with torch.no_grad():
        yn = ops.BagAttnMixFn.apply(u, gflat, W, bias, lw, L)
        yt = torch_sequence(u.index_select(1, sel), gflat, W, bias)
    op = alternate({"native_distinct_tokens": op_native, "torch_materialised_tokens": op_torch},
                   a.rounds, a.block, a.warmup)
    nat, tor = op["native_distinct_tokens"], op["torch_materialised_tokens"]
    op.update({"tokens_native": U + 2, "tokens_torch": L + 2, "width": WIDTH,
               "forward_rel_l2_native_vs_torch": float((yn - yt).norm() / yt.norm()),
               "du_rel_l2_native_vs_torch": float((gn - u.grad).norm() / u.grad.norm()),
               "native_over_torch_time": round(nat["step"]["median_ms"] / tor["step"]["median_ms"], 3),
               "native_entry_points": kernel_times(op_native, ENTRIES, 3)})
    res["a_bag_attention_fwd_bwd"] = op
    del u, gn, yn, yt
    torch.cuda.empty_cache()

    # ---- (b), (c) the whole eager step
    m = blindno.NIOFP2D_Trans_attn(2, 3, 100, 25, 3, 12, 32, 2, N, N).to(dev).train()
    mt = blindno.NIOFP2D_Trans(2, 3, 100, 25, 3, 12, 32, 2).to(dev).train()
    x = torch.randn(B, T, N, N, device=dev)
    y = torch.randn(B, N, N, 2, device=dev)

    def step_of(model, dedup):
        def step():
            nio.DEDUP_BAGS = dedup
            try:
                for p in model.parameters():
                    p.grad = None
                ops.MSEFn.apply(model(x, grid, bag_idx=idx), y, None).backward()
            finally:
                nio.DEDUP_BAGS = True
        return step

    with torch.no_grad():
        o_d = m(x, grid, bag_idx=idx)
        nio.DEDUP_BAGS = False
        try:
            o_k = m(x, grid, bag_idx=idx)
        finally:
            nio.DEDUP_BAGS = True
    b = alternate({"dedup": step_of(m, True), "duplicates_kept": step_of(m, False)}, a.rounds, a.block, a.warmup)
    b.update({"model": f"NIOFP2D_Trans_attn(2, 3, 100, 25, 3, 12, 32, 2, {N}, {N})", "x": [B, T, N, N],
              "forward_rel_l2_dedup_vs_kept": float((o_d - o_k).norm() / o_k.norm()),
              "dedup_over_kept_time": round(b["dedup"]["step"]["median_ms"] /
                                            b["duplicates_kept"]["step"]["median_ms"], 3)})
    res["b_step_dedup_vs_duplicates_kept"] = b
    c = alternate({"trans_attn": step_of(m, True), "trans": step_of(mt, True)}, a.rounds, a.block, a.warmup)
    c.update({"trans_attn_over_trans_time": round(c["trans_attn"]["step"]["median_ms"] /
                                                  c["trans"]["step"]["median_ms"], 3),
              "native_entry_points": kernel_times(step_of(m, True), ENTRIES, 3)})
    res["c_step_vs_NIOFP2D_Trans"] = c
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
