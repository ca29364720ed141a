#!/usr/bin/env python3
"""Forward + backward time of the native FNO3d against the same math on torch.fft.

    python tools/bench_fno3d.py [--iters 50] [--warmup 10] [--out profiles/fno3d_bench.json]
    python tools/bench_fno3d.py --breakdown      # + per-kernel share from one rocprofv3 run

Shape: FNO3d(8, 20, 4, 4, 1) on a (4, 40, 40, 40, 4) input (NIOFP3D's 40^3 grid, 2d_FPE/
NIOModules.py:720-788).  Baseline: TorchFNO3d below, the tool's own fp32 restatement of the layer
on torch.fft.rfftn / irfftn and torch.nn.functional, on the same GPU with the same parameters.
Each iteration is timed with a pair of events around forward + backward; min / median / max over
the timed iterations are reported.  blindno_colpass3d is timed on its own in a separate pass
(blindno.timing.KernelTimer) against its algorithmic bytes and the 8 TB/s HBM peak.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd"))

import torch
import torch.nn as nn
import torch.nn.functional as F

HBM_PEAK_GBS = 8000.0
FP32_PEAK_TFLOPS = 157.3
CTOR = (8, 20, 4, 4, 1)
SHAPE = (4, 40, 40, 40, 4)


class TorchFNO3d(nn.Module):
    """The same math as blindno.FNO3d in eager PyTorch (fp32, torch.fft); takes its parameters
    from a blindno.FNO3d so that both run the same numbers."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def spectral(self, s, x):
        B, _, P1, P2, P3 = x.shape
        m1, m2, m3 = s.modes1, s.modes2, s.modes3
        xf = torch.fft.rfftn(x, dim=[-3, -2, -1])
        of = torch.zeros(B, s.out_channels, P1, P2, P3 // 2 + 1, dtype=torch.cfloat, device=x.device)
        lo1, hi1, lo2, hi2 = slice(None, m1), slice(-m1, None), slice(None, m2), slice(-m2, None)
        for (a, b), w in zip([(lo1, lo2), (hi1, lo2), (lo1, hi2), (hi1, hi2)],
                             [s.weights1, s.weights2, s.weights3, s.weights4]):
            of[:, :, a, b, :m3] = torch.einsum("bixyz,ioxyz->boxyz", xf[:, :, a, b, :m3], w)
        return torch.fft.irfftn(of, s=(P1, P2, P3))

    def forward(self, x):
        m, p = self.m, self.m.padding
        h = F.pad(m.fc0(x).permute(0, 4, 1, 2, 3), [0, p, 0, p, 0, p])
        for k in range(4):
            h = self.spectral(getattr(m, f"conv{k}"), h) + getattr(m, f"w{k}")(h)
            if k < 3:
                h = F.gelu(h)
        h = h[..., :-p, :-p, :-p].permute(0, 2, 3, 4, 1)
        return m.fc2(F.gelu(m.fc1(h)))


def time_step(model, x, cot, iters, warmup):
    def step():
        for p in model.parameters():
            p.grad = None
        x.grad = None
        (model(x) * cot).sum().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4),
            "max_ms": round(max(ms), 4), "iters": iters, "warmup": warmup}


def breakdown(iters):
    """Per-kernel share of the native step from one rocprofv3 --kernel-trace --stats run of this
    tool (a child process; nothing else is traced in it)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", "2",
               "--native-only", "--out", ""]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv written"}
        rows = list(csv.DictReader(open(files[0])))
        tot = sum(float(r_["TotalDurationNs"]) for r_ in rows) or 1.0
        return [{"kernel": r_["Name"][:80], "calls": int(r_["Calls"]),
                 "share": round(float(r_["TotalDurationNs"]) / tot, 4),
                 "avg_us": round(float(r_["AverageNs"]) / 1e3, 2)} for r_ in rows[:16]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fno3d_bench.json"))
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--native-only", action="store_true")
    a = ap.parse_args()

    import blindno
    from blindno import timing
    assert torch.cuda.is_available(), "needs a HIP device"
    blindno.load_library()
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    m = blindno.FNO3d(*CTOR).to(dev)
    x = torch.randn(*SHAPE, device=dev, requires_grad=True)
    cot = torch.randn(*SHAPE[:4], CTOR[4], device=dev)
    res = {"model": f"FNO3d{CTOR}", "input": list(SHAPE), "device": torch.cuda.get_device_name(0),
           "native": time_step(m, x, cot, a.iters, a.warmup)}
    if not a.native_only:
        ref = TorchFNO3d(m)
        res["torch_fft"] = time_step(ref, x, cot, a.iters, a.warmup)
        res["speedup_median"] = round(res["torch_fft"]["median_ms"] / res["native"]["median_ms"], 3)
        out_n, out_r = m(x).detach(), ref(x).detach()
        res["native_vs_torch_fft_rel_l2"] = float((out_n - out_r).norm() / out_r.norm())
        # blindno_colpass3d on its own (events around every launch: a separate pass)
        kt = timing.KernelTimer("blindno_colpass3d")
        kt.start()
        for _ in range(10):
            (m(x) * cot).sum().backward()
        kt.stop()
        res["colpass3d"] = kt.roofline(HBM_PEAK_GBS, FP32_PEAK_TFLOPS, bound="hbm")
        if a.breakdown:
            res["kernel_share"] = breakdown(5)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
