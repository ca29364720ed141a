"""Float64 restatement of the reference's 3D snapshot encoders and NIOFP3D, written from the
reference's definitions (yl602019618/Reconstruction-of-PDE-without-Time-Label,
2d_FPE/Baselines.py:26-38,322-429 and 2d_FPE/NIOModules.py:720-788) on torch's float64 CPU
operators.  Test infrastructure: the checker of tests/test_nio3d_golden.py (pinned there to the
reference's own outputs) and of tests/test_gpu_nio3d.py.

Parameters come as a dict of float64 tensors keyed like the reference's state_dict.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import fno3d_ref
from oracle import fno_ref

F64 = torch.float64

# (block, stride, padding) of Encoder3D / Encoder3D_down in forward order; the kernels are the
# weights' own shapes ((1, 7, 7), 3^3 ..., and (2, 1, 1) or (1, 1, 1) for the last block)
ENC3D_BLOCKS = [
    ("convblock1", (1, 2, 2), (0, 3, 3)),
    ("convblock2_1", (2, 2, 2), (1, 1, 1)),
    ("convblock2_2", (1, 1, 1), (1, 1, 1)),
    ("convblock3_1", (2, 2, 2), (1, 1, 1)),
    ("convblock3_2", (1, 1, 1), (1, 1, 1)),
    ("convblock4_1", (2, 2, 2), (1, 1, 1)),
    ("convblock4_2", (1, 1, 1), (1, 1, 1)),
    ("convblock7_1", (2, 2, 2), (1, 1, 1)),
    ("convblock7_2", (2, 2, 2), (1, 1, 1)),
    ("convblock7_3", (1, 1, 1), (0, 0, 0)),
]


def sub(p, prefix):
    prefix += "."
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def encoder3d(p, x, masks=None, record=None, stats=None):
    """Encoder3D(_down).forward with train-mode BatchNorm3d (Baselines.py:339-374): x (B, L, 1, D,
    H, W) -> (B, L, n_out).  ConvBlock3D = Conv3d -> BatchNorm3d (batch statistics over N D H W)
    -> LeakyReLU(0.2).  ``masks`` / ``record``: the LeakyReLU branches taken from / handed to
    another evaluation (see oracle.fno_ref.encoder2d).  ``stats`` (optional list) receives each
    block's (batch mean, unbiased batch variance), what the running statistics are updated with."""
    B, L = x.shape[:2]
    h = x.reshape(B * L, *x.shape[2:]).to(F64)
    for k, (name, stride, pad) in enumerate(ENC3D_BLOCKS):
        h = F.conv3d(h, p[f"{name}.layers.0.weight"], p[f"{name}.layers.0.bias"], stride=stride,
                     padding=pad)
        if stats is not None:
            hd = h.detach()
            stats.append((hd.mean(dim=(0, 2, 3, 4)), hd.var(dim=(0, 2, 3, 4), unbiased=True)))
        h = F.batch_norm(h, None, None, p[f"{name}.layers.1.weight"], p[f"{name}.layers.1.bias"],
                         training=True, eps=1e-5)
        if record is not None:
            record.append(h.detach() > 0)
        h = F.leaky_relu(h, 0.2) if masks is None else torch.where(masks[k], h, 0.2 * h)
    h = h.flatten(1).view(B, L, -1)
    return F.linear(h, p["linear.weight"], p["linear.bias"])


def niofp3d(p, x, grid, idx=None, n_hidden_layers=3, branch_masks=None):
    """NIOFP3D.forward (NIOModules.py:755-788): x (B, T, Nx, Ny, Nz), grid (Nx, Ny, Nz, 3) ->
    (B, Nx, Ny, Nz, output_dim).  ``idx``: the train-mode bag (x[:, idx]); None: every snapshot."""
    x = x.to(F64)
    if idx is not None:
        x = x[:, list(idx)]
    B, L, nx, ny, nz = x.shape
    g = grid.to(F64)
    w = encoder3d(sub(p, "branch"), x.unsqueeze(2), branch_masks)              # :772 branch
    basis = fno_ref.ffn(sub(p, "trunk"), g.reshape(-1, 3), n_hidden_layers)    # :771-772 trunk
    u = fno_ref.deeponet_nobias(w, basis, p["deeponet.b0"]).view(B, L, nx, ny, nz)   # :774
    gcf = g.unsqueeze(0).repeat(B, 1, 1, 1, 1).permute(0, 4, 1, 2, 3)          # :775
    h = torch.cat((gcf, u), 1)                                                 # :777
    W, b = p["fc0.weight"].detach(), p["fc0.bias"].detach()                    # :778-779 (.data)
    Wt = torch.cat([W[:, :3], W[:, 3].view(-1, 1).repeat(1, L) / L], dim=1)    # :781
    h = torch.matmul(h.permute(0, 2, 3, 4, 1), Wt.T) + b                       # :782-784
    return fno3d_ref.fno3d(sub(p, "fno"), h)                                   # :786


def leaves(state):
    """numpy state -> float64 / complex128 leaves (requires_grad except on integer buffers)."""
    out = {}
    for k, v in state.items():
        t = torch.from_numpy(v)
        if v.dtype.kind in "fc":
            t = t.to(torch.complex128 if v.dtype.kind == "c" else F64).requires_grad_(True)
        out[k] = t
    return out


def make_state3d(named_shapes, seed, complex_names=()):
    """recipe.make_state with complex values for FNO3d's cfloat weights (the recipe's own complex
    branch serves the 2D ``spectral_list`` names only): real and imaginary parts are two recipe
    parameters named ``<key>.re`` / ``<key>.im``."""
    import numpy as np
    from recipe import make_param, make_state
    st = make_state([(k, s) for k, s in named_shapes if k not in complex_names], seed)
    for k, s in named_shapes:
        if k in complex_names:
            st[k] = (make_param(k + ".re", s, seed) + 1j * make_param(k + ".im", s, seed)).astype(np.complex64)
    return {k: st[k] for k, _ in named_shapes}
