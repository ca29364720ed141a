"""Float64 restatement of the reference's 3D Fourier layer and FNO3d, written from the reference's
definitions (yl602019618/Reconstruction-of-PDE-without-Time-Label, 2d_FPE/FNOModules.py) on
torch.fft in complex128.  Test infrastructure: the checker of tests/test_fno3d_golden.py (pinned
there to the reference's own outputs) and of tests/test_gpu_fno3d.py.

Parameters come as a dict of float64 / complex128 tensors keyed like the reference's state_dict.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

F64, C128 = torch.float64, torch.complex128


def to64(t):
    """fp32 / cfloat tensor or numpy array -> float64 / complex128 leaf tensor."""
    t = torch.as_tensor(t)
    return t.detach().cpu().to(C128 if t.is_complex() else F64)


def corner_slices(m1, m2):
    """The four corner blocks in assignment order (FNOModules.py:277-284)."""
    lo1, hi1, lo2, hi2 = slice(None, m1), slice(-m1, None), slice(None, m2), slice(-m2, None)
    return [(lo1, lo2), (hi1, lo2), (lo1, hi2), (hi1, hi2)]


def spectral_conv3d(x, ws):
    """SpectralConv3d.forward (FNOModules.py:270-288): x (B, Ci, P1, P2, P3) float64, ws the four
    complex128 weights (Ci, Co, m1, m2, m3).  Later assignments overwrite earlier ones."""
    B, Ci, P1, P2, P3 = x.shape
    Co, m1, m2, m3 = ws[0].shape[1:]
    x_ft = torch.fft.rfftn(x, dim=[-3, -2, -1])                                    # :273
    out_ft = torch.zeros(B, Co, P1, P2, P3 // 2 + 1, dtype=C128)                   # :276
    for (s1, s2), w in zip(corner_slices(m1, m2), ws):                             # :277-284
        out_ft[:, :, s1, s2, :m3] = torch.einsum("bixyz,ioxyz->boxyz", x_ft[:, :, s1, s2, :m3], w)
    return torch.fft.irfftn(out_ft, s=(P1, P2, P3))                                # :287


def mixed_spectrum_planes(At, ws, P, direction=0):
    """What the middle of the layer does to the last-axis spectrum, in float64: At (B, m3, C, P1,
    P2) complex128, the rfft over z of the field (direction 0) or of the output gradient
    (direction 1).  Returns Z (B, P1, P2, m3, C'), the coefficients whose last-axis inverse
    sum_k Re(Z_k e^{2 pi i k z / P3}) is the layer's output (direction 0), or the adjoint map
    (direction 1: conjugate-transposed weights, same transforms)."""
    P1, P2, P3 = P
    Ci, Co, m1, m2, m3 = ws[0].shape
    B = At.shape[0]
    X = torch.fft.fftn(At, dim=[-2, -1])                          # (B, m3, C, P1, P2)
    cout = Co if direction == 0 else Ci
    Y = torch.zeros(B, m3, cout, P1, P2, dtype=C128)
    ck = torch.tensor([1.0 if (k == 0 or 2 * k == P3) else 2.0 for k in range(m3)], dtype=F64)
    for (s1, s2), w in zip(corner_slices(m1, m2), ws):
        wk = w.permute(4, 0, 1, 2, 3) * (ck / (P1 * P2 * P3))[:, None, None, None, None]
        if direction == 0:
            Y[:, :, :, s1, s2] = torch.einsum("bkixy,kioxy->bkoxy", X[:, :, :, s1, s2], wk)
        else:
            Y[:, :, :, s1, s2] = torch.einsum("bkoxy,kioxy->bkixy", X[:, :, :, s1, s2], wk.conj())
    # unnormalised inverse over x and y (the 1/(P1 P2 P3) sits in the weights)
    Z = torch.fft.ifftn(Y, dim=[-2, -1], norm="forward")
    return Z.permute(0, 3, 4, 1, 2)


def winners(m1, m2, P1, P2):
    """mask[q] (m1, m2) bool: the entries of weights(q+1) whose frequency no later corner
    overwrites (only these receive gradient)."""
    owner = torch.full((P1, P2), -1, dtype=torch.int64)
    idx = []
    for q, (s1, s2) in enumerate(corner_slices(m1, m2)):
        owner[s1, s2] = q
        r1 = torch.arange(P1)[s1]
        r2 = torch.arange(P2)[s2]
        idx.append((r1, r2))
    return [owner[r1][:, r2] == q for q, (r1, r2) in enumerate(idx)]


def fno3d(p, x, padding=2):
    """FNO3d.forward (FNOModules.py:334-366) on a state_dict-keyed float64 parameter dict."""
    h = F.linear(x, p["fc0.weight"], p["fc0.bias"])                                # :336
    h = h.permute(0, 4, 1, 2, 3)                                                   # :337
    h = F.pad(h, [0, padding, 0, padding, 0, padding])                             # :339
    for k in range(4):                                                             # :341-358
        ws = [p[f"conv{k}.weights{q}"] for q in range(1, 5)]
        h = spectral_conv3d(h, ws) + F.conv3d(h, p[f"w{k}.weight"], p[f"w{k}.bias"])
        if k < 3:
            h = F.gelu(h)
    h = h[..., :-padding, :-padding, :-padding]                                    # :360
    h = h.permute(0, 2, 3, 4, 1)                                                   # :361
    h = F.gelu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))                        # :362-363
    return F.linear(h, p["fc2.weight"], p["fc2.bias"])                             # :364


def run(kind, p, x, cot):
    """Forward + backward of a golden case in float64: returns (out, {name: grad}, gin)."""
    p = {k: to64(v).requires_grad_(True) for k, v in p.items()}
    x = to64(x).requires_grad_(True)
    if kind == "sc3d":
        out = spectral_conv3d(x, [p[f"weights{q}"] for q in range(1, 5)])
    else:
        out = fno3d(p, x)
    (out * to64(cot)).sum().backward()
    return out.detach(), {k: v.grad for k, v in p.items()}, x.grad
