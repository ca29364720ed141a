"""The permutation-invariant attention UNet on 3D bags, ``PermInvUNet_attn3D``: the 2D class of
blindno/unet.py (2d_FPE/NIOModules.py:1086-1181, "BlinDNO") carried to three axes.

The reference has no 3D UNet; like ``NIOFP3D_FNO`` this model is the project's own, so no
checkpoint layout has to be kept -- the 2D attribute names and creation order are kept anyway, so
that the family reads alike.  One multi-channel head ``fno = FNO3d(modes, width, 2, width,
out_ch)`` (NIOFP3D_FNO's convention) replaces the 2D class's two one-channel heads.

Per-snapshot layers run on the B*L snapshots of a bag: the 3x3x3 and 1x1x1 convolutions on the
conv3d op (csrc/conv3d.hip), the 7x7x7 depthwise convolution, MaxPool3d(2) and
ConvTranspose3d(kernel = stride = 2) on csrc/unet3d.hip, and what is per voxel or per flattened
token on the 2D model's kernels unchanged: the ConvNeXt pointwise MLP (``CnxPwFn``, HW = D H W),
the skip BatchNorm (``ops.BNActFn``) and the collapsed temporal attention + bag mean
(``TokAttnMeanFn``, D = C D H W).  There is no CPU path and no graph capture.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import call, ptr, query, stream_ptr
from .fno import FNO3d
from .unet import CnxPwFn, TokAttnMeanFn, _UNetBase, _bn, _c, _e, _sizes_and_pads

DW3D_TILE = (5, 10, 40)     # the depthwise kernels' output tile (D, H, W), csrc/unet3d.hip


# ---------------------------------------------------------------------------- kernel launchers

def dwconv3d_fwd(x, w, b):
    """Depthwise KDxKHxKW convolution, same padding, with bias: ConvNeXtBlock3D.dwconv.
    x (N, C, D, H, W); w (C, 1, KD, KH, KW)."""
    ops.require_device(x, w)
    x, w = _c(x), _c(w)
    b = _c(b) if b is not None else None
    y = torch.empty_like(x)
    call("blindno_dwconv3d_fwd", ptr(x), ptr(w), ptr(b), ptr(y), *x.shape, *w.shape[-3:], stream_ptr())
    return y


def dwconv3d_bwd(dy, x, w, need_dx=True, need_w=True, nsplit=None):
    g = (*x.shape, *w.shape[-3:])
    C, T = x.shape[1], w[0].numel()
    dy = _c(dy)
    dx = dw = db = None
    if need_dx:
        dx = torch.empty_like(x)
        call("blindno_dwconv3d_bwd_data", ptr(dy), ptr(w), ptr(dx), *g, stream_ptr())
    if need_w:
        ns = nsplit or query("blindno_dwconv3d_wgrad_nsplit", *g)
        dwb = _e(C, T + 1, like=dy)
        part = _e(ns * C * (T + 1), like=dy) if ns > 1 else None
        call("blindno_dwconv3d_bwd_weight", ptr(dy), ptr(x), ptr(dwb), ptr(part), ns, *g, stream_ptr())
        dw = dwb[:, :-1].reshape(w.shape)
        db = dwb[:, -1].contiguous()
    return dx, dw, db


def maxpool3d_fwd(x, k):
    """MaxPool3d(k) (window = stride, floor) on (N, C, D, H, W) -> (y, arg uint8)."""
    ops.require_device(x)
    x = _c(x)
    N, C, D, H, W = x.shape
    out = (N, C, D // k[0], H // k[1], W // k[2])
    y = _e(*out, like=x)
    arg = torch.empty(out, device=x.device, dtype=torch.uint8)
    call("blindno_maxpool3d_fwd", ptr(x), ptr(y), ptr(arg), N * C, D, H, W, *k, stream_ptr())
    return y, arg


def maxpool3d_bwd(dy, arg, shape, k):
    N, C, D, H, W = shape
    dy = _c(dy)
    dx = _e(*shape, like=dy)
    call("blindno_maxpool3d_bwd", ptr(dy), ptr(_c(arg)), ptr(dx), N * C, D, H, W, *k, stream_ptr())
    return dx


def convt3d_fwd(x, w, b, out):
    """ConvTranspose3d(Ci, Co, kernel = stride = 2, output_padding): x (N, Ci, Di, Hi, Wi),
    w (Ci, Co, 2, 2, 2) -> (N, Co, *out)."""
    ops.require_device(x, w)
    x, w = _c(x), _c(w)
    b = _c(b) if b is not None else None
    if tuple(w.shape[2:]) != (2, 2, 2) or w.shape[0] != x.shape[1]:
        raise ValueError(f"convt3d: weight {tuple(w.shape)} is not (Ci = {x.shape[1]}, Co, 2, 2, 2)")
    y = _e(x.shape[0], w.shape[1], *out, like=x)
    call("blindno_convt3d_fwd", ptr(x), ptr(w), ptr(b), ptr(y), *x.shape, w.shape[1], *out, stream_ptr())
    return y


def convt3d_bwd(dy, x, w, need_dx=True, need_w=True):
    N, Ci, Di, Hi, Wi = x.shape
    Co = w.shape[1]
    g = (N, Ci, Di, Hi, Wi, Co, *dy.shape[2:])
    dy = _c(dy)
    dx = dw = db = None
    if need_dx:
        dx = torch.empty_like(x)
        call("blindno_convt3d_bwd_data", ptr(dy), ptr(w), ptr(dx), *g, stream_ptr())
    if need_w:
        E = Ci * Co * 8 + Co
        dwb = _e(E, like=dy)
        part = _e(query("blindno_convt3d_wgrad_nparts", N, Di, Hi, Wi) * E, like=dy)
        call("blindno_convt3d_bwd_weight", ptr(dy), ptr(x), ptr(dwb), ptr(part), *g, stream_ptr())
        dw = dwb[:E - Co].view(w.shape)
        db = dwb[E - Co:]
    return dx, dw, db


# ---------------------------------------------------------------------------- autograd ops

class DWConv3dFn(torch.autograd.Function):
    """``dwconv3d_fwd`` with its adjoint."""

    @staticmethod
    def forward(ctx, x, w, b):
        y = dwconv3d_fwd(x, w, b)
        ctx.save_for_backward(_c(x), _c(w))
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        n = ctx.needs_input_grad
        dx, dw, db = dwconv3d_bwd(dy, x, w, n[0], n[1] or (ctx.has_bias and n[2]))
        return dx, dw, db if ctx.has_bias else None


class MaxPool3dFn(torch.autograd.Function):
    """``maxpool3d_fwd`` with its adjoint."""

    @staticmethod
    def forward(ctx, x, k):
        y, arg = maxpool3d_fwd(x, k)
        ctx.save_for_backward(arg)
        ctx.geom = (tuple(x.shape), tuple(k))
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        return maxpool3d_bwd(dy, arg, *ctx.geom), None


class ConvT3dFn(torch.autograd.Function):
    """``convt3d_fwd`` with its adjoint."""

    @staticmethod
    def forward(ctx, x, w, b, out):
        y = convt3d_fwd(x, w, b, tuple(out))
        ctx.save_for_backward(_c(x), _c(w))
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        n = ctx.needs_input_grad
        dx, dw, db = convt3d_bwd(dy, x, w, n[0], n[1] or (ctx.has_bias and n[2]))
        return dx, dw, db if ctx.has_bias else None, None


# ---------------------------------------------------------------------------- building blocks

def _conv(conv: nn.Conv3d, x):
    """nn.Conv3d (kernel 3 padding 1, or final_conv's kernel 1) on the HIP implicit-GEMM op."""
    return ops.conv3d(x, conv.weight, conv.bias, conv.stride, conv.padding)


class ConvNeXtBlock3D(nn.Module):
    """ConvNeXtBlock (2d_FPE/NIOModules.py:1044-1062) with a 7x7x7 depthwise convolution."""

    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv3d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        N, C = x.shape[:2]
        xd = DWConv3dFn.apply(x, self.dwconv.weight, self.dwconv.bias)
        y = CnxPwFn.apply(xd.view(N, C, 1, -1), _c(x).view(N, C, 1, -1), self.norm.weight, self.norm.bias,
                          self.pwconv1.weight, self.pwconv1.bias, self.pwconv2.weight, self.pwconv2.bias)
        return y.view(x.shape)


class TemporalSelfAttention3D(nn.Module):
    """TemporalSelfAttention (2d_FPE/NIOModules.py:1065-1083) over tokens of D = C D H W values;
    the UNet only ever uses the bag mean of it, ``bag_mean`` (the collapsed HIP op)."""

    def __init__(self, C, D, H, W):
        super().__init__()
        self.C, self.Dz, self.H, self.W = C, D, H, W
        self.D = C * D * H * W
        self.norm = nn.LayerNorm(self.D)

    def bag_mean(self, x):
        """x (B, L, *feat) -> mean over the bag of the attention output: (B, *feat)."""
        B, L = x.shape[:2]
        y = TokAttnMeanFn.apply(x.reshape(B, L, -1), self.norm.weight, self.norm.bias, self.norm.eps)
        return y.view(B, *x.shape[2:])


class PermInvUNet_attn3D(_UNetBase):
    """PermInvUNet_attn on (B, T, Nx, Ny, Nz) bags.  ``depth`` pool levels with channels
    base_ch 2^i (each a power of two <= 64: the ConvNeXt pointwise kernel), ``width`` and
    ``modes`` those of the single FNO3d head."""

    dim = 3
    _heads = ("fno",)

    def __init__(self, in_ch=1, out_ch=2, base_ch=1, depth=3, input_size=(40, 40, 40), width=8, modes=4,
                 device=None):
        super().__init__()
        self.device = device
        self.depth = depth
        self.width = width
        self.input_size = tuple(int(n) for n in input_size)
        if len(self.input_size) != 3:
            raise ValueError(f"PermInvUNet_attn3D: input_size must have three extents, got {input_size}")
        self.chs = [base_ch * (2 ** i) for i in range(depth + 1)]
        sizes, pads = zip(*(_sizes_and_pads(n, depth) for n in self.input_size))
        self.down_convs = nn.ModuleList()
        self.pools = nn.ModuleList()
        self.down_convs.append(nn.Sequential(nn.Conv3d(in_ch, self.chs[0], kernel_size=3, padding=1),
                                             ConvNeXtBlock3D(self.chs[0])))
        for i in range(depth):
            self.pools.append(nn.MaxPool3d(2))
            self.down_convs.append(nn.Sequential(
                nn.Conv3d(self.chs[i], self.chs[i + 1], kernel_size=3, padding=1),
                ConvNeXtBlock3D(self.chs[i + 1])))
        self.skip_norms = nn.ModuleList([nn.BatchNorm3d(ch) for ch in self.chs])
        self.temp_atts = nn.ModuleList([TemporalSelfAttention3D(self.chs[i], *(s[i] for s in sizes))
                                        for i in range(depth + 1)])
        self.up_transposes = nn.ModuleList()
        self.up_convs = nn.ModuleList()
        for pad, i in zip(zip(*pads), reversed(range(depth))):
            self.up_transposes.append(nn.ConvTranspose3d(self.chs[i + 1], self.chs[i], kernel_size=2,
                                                         stride=2, output_padding=pad))
            self.up_convs.append(nn.Sequential(
                nn.Conv3d(self.chs[i] * 2, self.chs[i], kernel_size=3, padding=1),
                ConvNeXtBlock3D(self.chs[i])))
        self.final_conv = nn.Conv3d(self.chs[0], self.width, kernel_size=1)
        self.fno = FNO3d(modes=modes, width=self.width, n_layers=2, input_dim=self.width, output_dim=out_ch,
                         device=device)

    @property
    def unused_prefixes(self):
        """Registered parameters the forward never uses: the bottom level's skip BatchNorm."""
        return (f"skip_norms.{self.depth}.",)

    def forward(self, x, grid=None, bag_idx=None):
        """x (B, T, Nx, Ny, Nz) -> (B, Nx, Ny, Nz, out_ch).  ``grid`` is accepted and ignored;
        train mode draws the bag as the reference does (draw_bag), eval mode uses all T snapshots,
        ``bag_idx`` (host or device indices) overrides the draw."""
        if x.dim() != 5 or tuple(x.shape[2:]) != self.input_size:
            raise ValueError(f"PermInvUNet_attn3D: expected x (B, T, {', '.join(map(str, self.input_size))}), "
                             f"got {tuple(x.shape)}")
        ops.require_device(x)
        x = self._bag_of(x, bag_idx)
        B, L = x.shape[:2]
        h = x.reshape(B * L, 1, *x.shape[2:])
        feats = []
        for i in range(self.depth + 1):
            seq = self.down_convs[i]
            h = self._tap(f"feat{i}", seq[1](_conv(seq[0], h)))
            feats.append(h)
            if i < self.depth:
                h = MaxPool3dFn.apply(h, (2, 2, 2))

        def agg(level):
            f = feats[level]
            return self._tap(f"agg{level}", self.temp_atts[level].bag_mean(f.view(B, L, *f.shape[1:])))

        h = agg(self.depth)
        for i in range(self.depth):
            lv = self.depth - 1 - i
            up = self.up_transposes[i]
            h = ConvT3dFn.apply(h, up.weight, up.bias, tuple(feats[lv].shape[2:]))
            s = _bn(self.skip_norms[lv], agg(lv), 1.0)
            seq = self.up_convs[i]
            h = self._tap(f"up{i}", seq[1](_conv(seq[0], torch.cat([h, s], dim=1))))
        fused = self._tap("fused", _conv(self.final_conv, h))
        return self.fno(fused.permute(0, 2, 3, 4, 1).contiguous())
