"""Float64 restatements, on the CPU in plain torch, of what csrc/unet3d.hip and blindno/unet3d.py
compute: the depthwise convolution, the max pool and the transposed convolution (their gradients
by autograd), ConvNeXtBlock3D, the materialised temporal attention + bag mean and the whole
PermInvUNet_attn3D (tests/fno3d_ref.py is the head).  Test infrastructure: the checker of
tests/test_gpu_unet3d.py, itself pinned to torch.nn.functional by tests/test_unet3d_ref.py.  Also
the case tables both test files use.

Every function works in the dtype of its inputs, so the model can also be run in float32 (the
conditioning yardstick of the gradient bars).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import fno3d_ref

F64 = torch.float64

# the depthwise kernels' output tile (D, H, W); blindno.unet3d.DW3D_TILE must agree
TILE = (5, 10, 40)

# name -> (N, C, D, H, W, (KD, KH, KW), bias)
DW_CASES = {
    "all_padding": (2, 3, 5, 9, 11, (7, 7, 7), True),      # D below the kernel: every voxel touches padding
    "tile_edges": (1, 1, 6, 11, 41, (7, 7, 7), True),      # each extent = tile + 1: halos cross tile edges
    "k117": (2, 2, 4, 5, 13, (1, 1, 7), True),
    "k357": (1, 2, 6, 7, 9, (3, 5, 7), True),
    "no_bias": (1, 2, 4, 6, 10, (7, 7, 7), False),
}
# weight gradient at forced split counts: 2 x 2 x 2 tiles x N = 2 -> 16 work items per channel
DW_WGRAD_CASE = (2, 2, 6, 11, 41, (7, 7, 7), True)
DW_WGRAD_SPLITS = (1, 3)

# name -> (N, C, D, H, W, window)
POOL_CASES = {
    "floor": (2, 3, 5, 7, 9, (2, 2, 2)),                   # -> (2, 3, 4): a plane dropped on every axis
    "w122": (2, 2, 3, 6, 8, (1, 2, 2)),
}

# (N, Ci, Co, (Di, Hi, Wi), (Do, Ho, Wo)): output_padding (1, 0, 1)
CONVT_CASE = (2, 4, 2, (2, 3, 4), (5, 6, 9))

# the model case: three distinct extents (one odd) that FNO3d takes at modes 2
MODEL = dict(input_size=(9, 12, 10), depth=2, base_ch=2, width=4, modes=2, B=2, T=6, bag=[0, 3, 3, 5, 1])


def dw_tiles(D, H, W):
    return tuple(-(-n // t) for n, t in zip((D, H, W), TILE))


# ------------------------------------------------------------------------------------- ops

def dwconv3d(x, w, b=None):
    """y[n][c][d][h][w] = b[c] + sum_{i,j,k} W[c][i][j][k] x[n][c][d+i-KD/2][h+j-KH/2][w+k-KW/2],
    zero padding, written out tap by tap.  x (N, C, D, H, W), w (C, KD, KH, KW)."""
    N, C, D, H, W = x.shape
    KD, KH, KW = w.shape[-3:]
    w = w.reshape(C, KD, KH, KW)
    xp = F.pad(x, [KW // 2, KW // 2, KH // 2, KH // 2, KD // 2, KD // 2])
    y = torch.zeros_like(x)
    for i in range(KD):
        for j in range(KH):
            for k in range(KW):
                y = y + w[:, i, j, k].view(1, C, 1, 1, 1) * xp[:, :, i:i + D, j:j + H, k:k + W]
    return y if b is None else y + b.view(1, C, 1, 1, 1)


def dwconv3d_bwd_data(g, w):
    """The input gradient as the kernel forms it: the same convolution on the point-reflected taps."""
    return dwconv3d(g, w.reshape(w.shape[0], *w.shape[-3:]).flip(1, 2, 3))


def maxpool3d(x, k):
    """Window = stride = k, floor; the first maximum in (d, h, w) scan order wins, a NaN wins.
    Returns (y, tap index)."""
    N, C, D, H, W = x.shape
    Do, Ho, Wo = D // k[0], H // k[1], W // k[2]
    v = x[:, :, :Do * k[0], :Ho * k[1], :Wo * k[2]].reshape(N, C, Do, k[0], Ho, k[1], Wo, k[2])
    v = v.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, Do, Ho, Wo, -1)
    return v.max(-1)


def convt3d(x, w, b, out):
    """ConvTranspose3d(kernel = stride = 2): y[n][o][2d+a][2h+e][2w+f] = b[o] + sum_i x[n][i][d][h][w]
    W[i][o][a][e][f]; the planes past 2 Di (output_padding) hold the bias only."""
    N, Ci, Di, Hi, Wi = x.shape
    Co = w.shape[1]
    y = torch.zeros(N, Co, *out, dtype=x.dtype)
    for a in range(2):
        for e in range(2):
            for f in range(2):
                y[:, :, a:2 * Di:2, e:2 * Hi:2, f:2 * Wi:2] = torch.einsum("nidhw,io->nodhw", x, w[:, :, a, e, f])
    return y if b is None else y + b.view(1, Co, 1, 1, 1)


def convnext_block3d(p, pre, x):
    """ConvNeXtBlock3D: dwconv 7^3 -> LayerNorm over C (eps 1e-6) -> Linear(C, 4C) -> exact GELU ->
    Linear(4C, C) -> + x."""
    C = x.shape[1]
    h = dwconv3d(x, p[pre + "dwconv.weight"], p[pre + "dwconv.bias"]).permute(0, 2, 3, 4, 1)
    h = F.layer_norm(h, (C,), p[pre + "norm.weight"], p[pre + "norm.bias"], 1e-6)
    h = F.linear(F.gelu(F.linear(h, p[pre + "pwconv1.weight"], p[pre + "pwconv1.bias"])),
                 p[pre + "pwconv2.weight"], p[pre + "pwconv2.bias"])
    return h.permute(0, 4, 1, 2, 3) + x


def attention_bag_mean(X, lw, lb, eps=1e-5):
    """mean_l LayerNorm_D(softmax(X X^T / sqrt D) X + X)_l, materialised.  X (B, L, D) -> (B, D)."""
    D = X.shape[-1]
    A = torch.softmax(X @ X.transpose(1, 2) / D ** 0.5, dim=-1)
    return F.layer_norm(A @ X + X, (D,), lw, lb, eps).mean(1)


def unet_body(p, x, depth, idx=None, train=True):
    """PermInvUNet_attn3D up to final_conv: x (B, T, Nx, Ny, Nz) -> (B, Nx, Ny, Nz, width)."""
    if idx is not None:
        x = x[:, torch.as_tensor(np.asarray(idx), dtype=torch.long)]
    B, L = x.shape[:2]
    h = x.reshape(B * L, 1, *x.shape[2:])
    feats = []
    for i in range(depth + 1):
        h = F.conv3d(h, p[f"down_convs.{i}.0.weight"], p[f"down_convs.{i}.0.bias"], padding=1)
        h = convnext_block3d(p, f"down_convs.{i}.1.", h)
        feats.append(h)
        if i < depth:
            h = maxpool3d(h, (2, 2, 2))[0]

    def agg(lv):
        f = feats[lv]
        y = attention_bag_mean(f.reshape(B, L, -1), p[f"temp_atts.{lv}.norm.weight"], p[f"temp_atts.{lv}.norm.bias"])
        return y.view(B, *f.shape[1:])

    h = agg(depth)
    for i in range(depth):
        lv = depth - 1 - i
        h = convt3d(h, p[f"up_transposes.{i}.weight"], p[f"up_transposes.{i}.bias"], tuple(feats[lv].shape[2:]))
        pre = f"skip_norms.{lv}."
        s = F.batch_norm(agg(lv), None if train else p[pre + "running_mean"], None if train else p[pre + "running_var"],
                         p[pre + "weight"], p[pre + "bias"], training=train, eps=1e-5)
        h = F.conv3d(torch.cat([h, s], 1), p[f"up_convs.{i}.0.weight"], p[f"up_convs.{i}.0.bias"], padding=1)
        h = convnext_block3d(p, f"up_convs.{i}.1.", h)
    return F.conv3d(h, p["final_conv.weight"], p["final_conv.bias"]).permute(0, 2, 3, 4, 1)


def unet3d(p, x, depth, idx=None, train=True):
    """The whole model; the head (p["fno.*"]) always runs in float64."""
    fused = unet_body(p, x, depth, idx, train)
    head = {k[4:]: (v.to(torch.complex128) if v.is_complex() else v.to(F64)) for k, v in p.items()
            if k.startswith("fno.")}
    return fno3d_ref.fno3d(head, fused.to(F64))


def leaves(state, dtype=F64):
    """state_dict -> leaf tensors of ``dtype`` (complex ones of the matching complex dtype)."""
    cd = torch.complex128 if dtype == F64 else torch.complex64
    out = {}
    for k, v in state.items():
        v = torch.as_tensor(v).detach().cpu()
        if v.is_complex():
            out[k] = v.to(cd).requires_grad_(True)
        elif v.is_floating_point():
            out[k] = v.to(dtype).requires_grad_(True)
        else:
            out[k] = v
    return out


def run_model(state, x, cot, depth, idx, dtype=F64, perturb=None, train=True):
    """Forward + backward: (out float64, {name: gradient float64 / complex128})."""
    p = leaves(state, dtype)
    x = torch.as_tensor(x).to(dtype)
    if perturb is not None:       # an input change of the size of one float32 rounding
        gen = torch.Generator().manual_seed(perturb)
        x = x * (1 + float(np.finfo(np.float32).eps) * torch.randn(x.shape, generator=gen, dtype=dtype))
    out = unet3d(p, x, depth, idx, train)
    (out * torch.as_tensor(cot).to(out.dtype)).sum().backward()
    grads = {}
    for k, v in p.items():
        if torch.is_tensor(v) and v.requires_grad and v.grad is not None:
            grads[k] = v.grad.to(torch.complex128 if v.is_complex() else F64)
    return out.detach().to(F64), grads
