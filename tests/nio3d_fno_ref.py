"""Float64 restatement of the 3D FNO-NIO model NIOFP3D_FNO: the reference's 2D composite
(yl602019618/Reconstruction-of-PDE-without-Time-Label, 2d_FPE/NIOModules.py:543-581) on three
axes, composed from its FNO3d (2d_FPE/FNOModules.py:290-366, restated in tests/fno3d_ref.py) and
its bag-mean expression (NIOModules.py:565-575) with one more grid channel.  Test infrastructure:
the checker of tests/test_nio3d_fno_golden.py (pinned there to that composition run in the
reference's own fp32 code) and of tests/test_gpu_nio3d_fno.py.

The bag is taken literally: every drawn snapshot is encoded, repeats included, and the mean is
the matmul of cat[grid, u_1..u_L] with W' -- no deduplication, no bag-level statistics.

Parameters come as a dict of float64 / complex128 tensors keyed like the model's state_dict
(``FNO_input.*``, ``fc0.*``, ``fno.*``).
"""
from __future__ import annotations

import torch

import fno3d_ref
from nio3d_ref import leaves, make_state3d, sub  # noqa: F401  (re-exported for the tests)

F64 = torch.float64


def niofp3d_fno(p, x, grid, idx=None):
    """x (B, T, Nx, Ny, Nz), grid (Nx, Ny, Nz, 3) -> (B, Nx, Ny, Nz, output_dim).  ``idx``: the
    train-mode bag (x[:, idx], repeats kept); None: every snapshot."""
    x = x.to(F64)
    if idx is not None:
        x = x[:, list(idx)]                                                    # :551
    B, L, nx, ny, nz = x.shape
    g = grid.to(F64)
    x_input = x.reshape(B * L, 1, nx, ny, nz)                                  # :555
    grid_r = g.permute(3, 0, 1, 2).unsqueeze(0).repeat(B * L, 1, 1, 1, 1)      # :558
    inp = torch.cat((x_input, grid_r), dim=1).permute(0, 2, 3, 4, 1)           # :560
    u = fno3d_ref.fno3d(sub(p, "FNO_input"), inp)                              # :562
    u = u.view(B, L, nx, ny, nz)                                               # :564
    gcf = g.unsqueeze(0).repeat(B, 1, 1, 1, 1).permute(0, 4, 1, 2, 3)          # :565
    h = torch.cat((gcf, u), 1)                                                 # :567
    W, b = p["fc0.weight"].detach(), p["fc0.bias"].detach()                    # :569-570 (.data)
    Wt = torch.cat([W[:, :3], W[:, 3].view(-1, 1).repeat(1, L) / L], dim=1)    # :572
    h = torch.matmul(h.permute(0, 2, 3, 4, 1), Wt.T) + b                       # :573-575
    return fno3d_ref.fno3d(sub(p, "fno"), h)                                   # :577
