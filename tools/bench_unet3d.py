#!/usr/bin/env python3
"""Training-step time of PermInvUNet_attn3D at the 40^3 grid on the native kernels
(csrc/unet3d.hip with conv3d / cnx_pw / bn_act / tok_attn) and of the same model composed from
torch.nn.functional on the same GPU (conv3d with groups, layer_norm, max_pool3d, conv_transpose3d,
batch_norm and the materialised temporal attention; the FNO3d head is the native one in both).

    python tools/bench_unet3d.py [--rounds 4] [--block 3] [--warmup 2] [--out profiles/unet3d_bench.json]

Model: PermInvUNet_attn3D(1, 2, 1, 3, (40, 40, 40)) in train mode on x (4, 100, 40, 40, 40) with a
fixed recorded bag of L = 75 snapshots drawn with replacement.  One step = forward, MSE loss,
backward, timed with a pair of events.  The two steps are timed in alternating blocks of ``block``
steps, ``rounds`` times; medians over all steps of a mode.  Peak memory is torch's
max_memory_allocated over one further step of each mode.  After that, a few native steps run with
events around the launches of csrc/unet3d.hip alone (the largest launch of each entry per step: the
level-0 one), and dwconv3d_fwd's level-0 launch is set against the fp32 vector peak
(2 x 343 x N C D H W flop over 157.3 TFLOP/s).
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

B, T, N, L = 4, 100, 40, 75
PEAK_FP32_VECTOR = 157.3e12
ENTRIES = ("blindno_dwconv3d_fwd", "blindno_dwconv3d_bwd_data", "blindno_dwconv3d_bwd_weight",
           "blindno_maxpool3d_fwd", "blindno_maxpool3d_bwd", "blindno_convt3d_fwd",
           "blindno_convt3d_bwd_data", "blindno_convt3d_bwd_weight")


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
    return {n: summary(ms) for n, ms in per_step.items()}


def torch_forward(m, x, idx):
    """The forward of blindno.unet3d.PermInvUNet_attn3D on m's parameters, composed from
    torch.nn.functional; the head is m.fno."""
    def cnx(blk, h):
        C = h.shape[1]
        z = F.conv3d(h, blk.dwconv.weight, blk.dwconv.bias, padding=3, groups=C).permute(0, 2, 3, 4, 1)
        z = F.layer_norm(z, (C,), blk.norm.weight, blk.norm.bias, 1e-6)
        z = F.linear(F.gelu(F.linear(z, blk.pwconv1.weight, blk.pwconv1.bias)), blk.pwconv2.weight, blk.pwconv2.bias)
        return z.permute(0, 4, 1, 2, 3) + h

    x = x.index_select(1, idx)
    Bn, Ln = x.shape[:2]
    h = x.reshape(Bn * Ln, 1, *x.shape[2:])
    feats = []
    for i in range(m.depth + 1):
        seq = m.down_convs[i]
        h = cnx(seq[1], F.conv3d(h, seq[0].weight, seq[0].bias, padding=1))
        feats.append(h)
        if i < m.depth:
            h = F.max_pool3d(h, 2)

    def agg(lv):
        f = feats[lv]
        X = f.reshape(Bn, Ln, -1)
        A = torch.softmax(X @ X.transpose(1, 2) / X.shape[-1] ** 0.5, dim=-1)
        nrm = m.temp_atts[lv].norm
        return F.layer_norm(A @ X + X, (X.shape[-1],), nrm.weight, nrm.bias, nrm.eps).mean(1).view(Bn, *f.shape[1:])

    h = agg(m.depth)
    for i in range(m.depth):
        lv = m.depth - 1 - i
        up = m.up_transposes[i]
        h = F.conv_transpose3d(h, up.weight, up.bias, stride=2, output_padding=up.output_padding)
        bn = m.skip_norms[lv]
        s = F.batch_norm(agg(lv), None, None, bn.weight, bn.bias, training=True, eps=bn.eps)
        seq = m.up_convs[i]
        h = cnx(seq[1], F.conv3d(torch.cat([h, s], 1), seq[0].weight, seq[0].bias, padding=1))
    fused = F.conv3d(h, m.final_conv.weight, m.final_conv.bias)
    return m.fno(fused.permute(0, 2, 3, 4, 1).contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet3d_bench.json"))
    a = ap.parse_args()

    import blindno
    from blindno import ops
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    m = blindno.PermInvUNet_attn3D(1, 2, 1, 3, (N, N, N), device="cuda").cuda().train()
    x = torch.randn(B, T, N, N, N, device="cuda")
    idx = np.random.RandomState(0).choice(T, L)
    idx_t = torch.as_tensor(idx, device="cuda")
    y = torch.randn(B, N, N, N, 2, device="cuda")

    def native():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(m(x, bag_idx=idx_t), y, None).backward()

    def composed():
        for p in m.parameters():
            p.grad = None
        ops.MSEFn.apply(torch_forward(m, x, idx_t), y, None).backward()

    steps = {"native": native, "torch_functional": composed}
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    with torch.no_grad():
        o_n, o_t = m(x, bag_idx=idx_t), torch_forward(m, x, idx_t)
        agree = float((o_n - o_t).norm() / o_t.norm())
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ms[k] += time_block(fn, a.block)
    res = {"model": "PermInvUNet_attn3D(1, 2, 1, 3, (40, 40, 40))", "x": [B, T, N, N, N], "bag": L,
           "bag_idx": [int(i) for i in idx], "device": torch.cuda.get_device_name(0),
           "forward_rel_l2_native_vs_torch": agree, "blocks": {"rounds": a.rounds, "steps_per_block": a.block}}
    for k, fn in steps.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res[k] = {"step": summary(ms[k]), "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    res["native_kernels"] = kernel_times(native, ENTRIES, 3)
    t = res["native_kernels"]["blindno_dwconv3d_fwd"]["median_ms"] * 1e-3
    flop = 2.0 * 343 * B * L * 1 * N ** 3
    res["dwconv3d_fwd_level0"] = {"flop": flop, "tflops": round(flop / t / 1e12, 2),
                                  "fraction_of_fp32_vector_peak": round(flop / t / PEAK_FP32_VECTOR, 4)}
    res["native_is_faster"] = res["native"]["step"]["median_ms"] < res["torch_functional"]["step"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
