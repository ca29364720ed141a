"""Snapshot-bag (time-label-free) models: NIOFP2D_FNO, NIOFP_FNO, NIOFP2D, NIOFP2D_attn,
NIOFP2D_Trans, NIOFP2D_Trans_attn, NIOFP, NIOFP_schrodinger, NIOFP3D -- drop-in for the reference's
NIOModules -- and NIOFP3D_FNO and
NIOFP3D_Trans, the project's own 3D FNO-NIO and 3D Transolver-NIO (the reference has no such
classes).

Same constructor signatures, attribute names and initialisation order as
2d_FPE/NIOModules.py:14-83,508-581, 2d_Non_conservative_FPE/NIOModules.py:13-82,503-577,
1d_FPE/NIOModules.py:15-155, 1d_GPE/NIOModules.py:160-289 and (NIOFP3D)
2d_FPE/NIOModules.py:720-788.

Train mode draws the bag exactly like the reference -- ``L = np.random.randint(50, T)``,
``idx = np.random.choice(T, L)`` (with replacement) from numpy's global RNG -- so a
seeded run sees the same bags.  ``bag_idx=`` overrides the draw (parity harness).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .deeponet import FFN, DeepOnetNoBiasOrg
from .encoders import Encoder, Encoder2D, Encoder3D, Encoder3D_down
from .fno import FNO1d, FNO2d, FNO3d, fno_params
from .transolver import Transolver2D
from .transolver3d import Transolver3D


def draw_bag(T: int):
    """The reference's train-mode bag draw (2d_FPE/NIOModules.py:548-553)."""
    L = np.random.randint(50, T)
    idx = np.random.choice(T, L)
    return L, idx


def _select(module, x, bag_idx, dedup=False):
    """The bag of this step: (x[:, idx], L, lw).  With ``dedup`` (models whose per-snapshot
    encoder output does not depend on the rest of the batch -- not the BatchNorm'd NIO branch)
    the bag is reduced to its distinct snapshots and lw holds multiplicity / L."""
    if isinstance(bag_idx, tuple):
        idx_t, lw = bag_idx                       # device-resident deduplicated bag
        return x.index_select(1, idx_t), idx_t.numel(), lw
    if torch.is_tensor(bag_idx) and bag_idx.is_cuda:
        # device-resident index list (graph replays): gather on the device
        return x.index_select(1, bag_idx), bag_idx.numel(), None
    if bag_idx is not None:
        idx = np.asarray(bag_idx)
    elif module.training:
        _, idx = draw_bag(x.shape[1])
    else:
        return x, x.shape[1], None
    lw = None
    if dedup:
        idx, w = dedup_bag(idx)
        if w is not None:
            lw = torch.as_tensor(w, device=x.device)
    return x[:, torch.as_tensor(idx, device=x.device)], len(idx), lw


_SIDE = {}


HEAD_STREAMS = True     # fork the two heads over two streams (ops.HeadPairFn)
# the encoder hands the grouped heads the bag mean ubar, the heads' lift forms their input
# (False, tests only: the (B, N, N, width) field between them and two bag-mean launches)
BAG_INPUT_HEADS = True
DEDUP_BAGS = True       # run the snapshot encoder once per distinct snapshot of a bag


def dedup_bag(idx):
    """(unique indices int32, multiplicity / L float32) of a with-replacement bag draw, or
    (idx, None) when every index is distinct (or DEDUP_BAGS is off).  The encoder output of a
    repeated snapshot is identical, so the bag mean sum_l u_l = sum_u count_u u_u."""
    idx = np.asarray(idx, dtype=np.int32)
    if not DEDUP_BAGS:
        return idx, None
    uniq, counts = np.unique(idx, return_counts=True)
    if len(uniq) == len(idx):
        return idx, None
    return uniq.astype(np.int32), (counts / float(len(idx))).astype(np.float32)


def _run_heads(module, h):
    """The FNO heads on h, concatenated (2d_FPE/NIOModules.py:577-581).  On the GPU two heads run
    concurrently, forward and backward (ops.HeadPairFn: the second on a side stream forked from
    and joined back into the current one; inside a graph capture, two parallel branches).  The
    heads are small (B samples), latency-bound launches, which is why overlapping them pays."""
    heads = [getattr(module, n) for n in module._heads]
    if len(heads) != 2 or not h.is_cuda or not HEAD_STREAMS:
        return torch.cat([f(h) for f in heads], dim=-1)
    side = _SIDE.get(h.device)
    if side is None:
        side = _SIDE[h.device] = torch.cuda.Stream(h.device)
    dim = 2 if isinstance(heads[0], FNO2d) else 1
    p0, p1 = fno_params(heads[0], dim), fno_params(heads[1], dim)
    return ops.HeadPairFn.apply(heads[0].meta(h.shape[-1]), heads[1].meta(h.shape[-1]), len(p0), side,
                                h, *p0, *p1)


def _bag_mean_2d(module, u, grid, B, L, nx, ny, lw=None):
    g = grid.reshape(nx * ny, 2)
    h = ops.BagMeanFn.apply(u.reshape(B, L, nx * ny), g, module.fc0.weight.data,
                            module.fc0.bias.data, lw)
    return h.view(B, nx, ny, -1)


def _bag_mean_1d(module, u, grid, B, L, nx, lw=None):
    h = ops.BagMeanFn.apply(u.reshape(B, L, nx), grid.reshape(nx, 1), module.fc0.weight.data,
                            module.fc0.bias.data, lw)
    return h


class NIOFP2D_FNO(nn.Module):
    """FNO-NIO, 2d_FPE/NIOModules.py:508-581.  ``heads`` selects the head attribute names
    (("fno_drift", "fno_diffusion") for 2d_FPE, ("fno_Fx", "fno_Fy") for the
    non-conservative copy); ``branch_last_kernel`` is the unused Encoder2D's final kernel
    (part of the checkpoint layout)."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, heads: Sequence[str] = ("fno_drift", "fno_diffusion"),
                 branch_last_kernel=(2, 1)):
        super().__init__()
        output_dimensions = n_basis
        self.fno_layers = fno_layers
        self.branch = Encoder2D(output_dimensions, last_kernel=branch_last_kernel)
        self.fc0 = nn.Linear(3, width)
        self.FNO_input = FNO2d(modes=12, width=4, n_layers=2, input_dim=3, output_dim=1)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))

    accepts_dedup_bag = True    # forward(bag_idx=(unique idx, weights)) on the fused path

    def _fused_ok(self, x, grid):
        return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and
                grid.dtype == torch.float32 and tuple(grid.shape) == (x.shape[2], x.shape[3], 2) and
                self.FNO_input.width <= 4 and
                not (torch.is_grad_enabled() and (x.requires_grad or grid.requires_grad)))

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, Nx, Ny) standardised snapshots, grid (Nx, Ny, 2) -> (B, Nx, Ny, 2).

        Without input gradients the snapshot encoder + bag mean run as the fused HIP path
        (ops.BagEncoderFn: snapshots read from x through the bag's indices); otherwise as the
        generic composition below (same numerics, gradients for x and grid)."""
        # the grouped heads' spectral weights are packed by the encoder's pack launch
        if x.is_cuda and HEAD_STREAMS and len(self._heads) == 2 and x.dim() == 4:
            hs = [getattr(self, nm) for nm in self._heads]
            w = self.fc0.out_features
            if all(isinstance(hd, FNO2d) for hd in hs) and hs[0].meta(w).__dict__ == hs[1].meta(w).__dict__:
                ops.pack_heads_ahead(hs[0].meta(w), (x.shape[0], x.shape[2], x.shape[3], w),
                                     [fno_params(hd, 2) for hd in hs], x.device)
        try:
            out = self._encoder_heads_fused(x, grid, bag_idx)
            if out is not None:
                return out
            return self.forward_heads(self.forward_encoder(x, grid, bag_idx))
        finally:
            ops.drop_pack_ahead()

    def _encoder_heads_fused(self, x, grid, bag_idx):
        """Encoder -> grouped heads with the bag mean handed over as ubar (B, Nx, Ny): the heads'
        lift forms fc0([grid, ubar]) itself and its adjoint returns d ubar (ops.BagHeadsIn), so
        the (B, Nx, Ny, width) field and the two bag-mean launches do not exist.  None where it
        does not apply (the composition forward_heads(forward_encoder(...)) then runs)."""
        if not (BAG_INPUT_HEADS and HEAD_STREAMS and len(self._heads) == 2 and self._fused_ok(x, grid)):
            return None
        hs = [getattr(self, nm) for nm in self._heads]
        if not all(isinstance(hd, FNO2d) for hd in hs):
            return None
        w = self.fc0.out_features
        m0, m1 = hs[0].meta(w), hs[1].meta(w)
        p0, p1 = fno_params(hs[0], 2), fno_params(hs[1], 2)
        if m0.__dict__ != m1.__dict__ or not ops.GROUPED_HEADS or \
                not ops.grouped_ok(m0, (x.shape[0], x.shape[2], x.shape[3], w), [p0, p1]):
            return None
        fno = self.FNO_input
        fp = fno_params(fno, 2)
        n = len(fno.spectral_list)
        idx_t, lw = self._encoder_bag(x, bag_idx)
        if not ops.bag_ubar_ok(fno.meta(3), x.shape[0], idx_t.numel(), x.shape[2], x.shape[3],
                               fp[2 + 4 * n], fp[4 + 4 * n], m0, 2, w):
            return None
        ubar = ops.BagEncoderFn.apply(fno.meta(3), True, x, idx_t, lw, grid, self.fc0.weight.data,
                                      self.fc0.bias.data, *fp)
        side = _SIDE.get(x.device)
        if side is None:
            side = _SIDE[x.device] = torch.cuda.Stream(x.device)
        bag = ops.BagHeadsIn(grid, self.fc0.weight.data, self.fc0.bias.data)
        return ops.HeadPairFn.apply((m0, bag), m1, len(p0), side, ubar, *p0, *p1)

    def _encoder_bag(self, x, bag_idx):
        """(device bag indices, multiplicity weights or None) of the fused encoder."""
        lw = None
        if isinstance(bag_idx, tuple):
            # device-resident deduplicated bag (train.GraphedBagStep): unique indices and
            # multiplicity weights
            idx_t, lw = bag_idx
        elif torch.is_tensor(bag_idx) and bag_idx.is_cuda and bag_idx.dtype == torch.int32:
            idx_t = bag_idx                  # device-resident bag indices
        else:
            if bag_idx is not None:
                idx = np.asarray(bag_idx)
            elif self.training:
                _, idx = draw_bag(x.shape[1])
            else:
                idx = np.arange(x.shape[1])
            idx, w = dedup_bag(idx)
            idx_t = torch.as_tensor(idx, device=x.device)
            if w is not None:
                lw = torch.as_tensor(w, device=x.device)
        return idx_t, lw

    def forward_heads(self, h):
        """The two FNO heads on the bag-mean field h (B, Nx, Ny, width) (:577-581)."""
        return _run_heads(self, h)

    def forward_encoder(self, x, grid, bag_idx=None):
        """FNO_input on the bag + the fixed-weight bag mean (:548-575) -> h (B, Nx, Ny, width).
        Split from the heads so a training step can be replayed as two graphs and the heads'
        gradient all-reduce overlap the encoder's backward (train.GraphedBagStep, overlap)."""
        if self._fused_ok(x, grid):
            fno = self.FNO_input
            idx_t, lw = self._encoder_bag(x, bag_idx)
            return ops.BagEncoderFn.apply(fno.meta(3), False, x, idx_t, lw, grid, self.fc0.weight.data,
                                          self.fc0.bias.data, *fno_params(fno, 2))
        x, L, lw = _select(self, x, bag_idx, dedup=True)
        B, _, nx, ny = x.shape
        x_in = x.reshape(B * L, 1, nx, ny)
        grid_r = grid.permute(2, 0, 1).unsqueeze(0).expand(B * L, 2, nx, ny)
        inp = torch.cat((x_in, grid_r), dim=1).permute(0, 2, 3, 1).contiguous()
        u = self.FNO_input(inp)                       # (B*L, nx, ny, 1)
        return _bag_mean_2d(self, u, grid, B, L, nx, ny, lw)


def draw_bag_distinct(T: int):
    """Train-mode draw of the attention variant: WITHOUT replacement
    (2d_FPE/NIOModules.py:344-345)."""
    L = np.random.randint(50, T)
    idx = np.random.choice(T, L, replace=False)
    return L, idx


class NIOFP2D_FNO_attn(nn.Module):
    """FNO-NIO with token self-attention over the bag, 2d_FPE/NIOModules.py:300-408
    (NC copy with heads fno_Fx/fno_Fy: 2d_Non_conservative_FPE/NIOModules.py:299-407).

    The snapshot encoder FNO_input runs on every snapshot of the bag (HIP FNO2d), then
    ops.BagAttnFn forms the tokens [gx, gy, u_1..u_L], their softmax(X X^T / sqrt(nx ny))
    attention and the fc0-weighted token mean (fc0 = Linear(1, width), ``.data``), and the
    two FNO heads run as in NIOFP2D_FNO.  Registration order (FNO_input, heads, fc0) follows
    the reference, so a seeded construction gives the reference's initial weights."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, nx, ny,
                 heads: Sequence[str] = ("fno_drift", "fno_diffusion")):
        super().__init__()
        self.fno_layers = fno_layers
        self.FNO_input = FNO2d(modes=12, width=4, n_layers=2, input_dim=3, output_dim=1)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))
        self.fc0 = nn.Linear(1, width)
        self.nx = nx
        self.ny = ny

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, nx, ny), grid (nx, ny, 2) -> (B, nx, ny, 2).  ``bag_idx`` overrides the
        train-mode draw (a host index list or a device int tensor)."""
        ops.require_device(x, grid)
        if torch.is_tensor(bag_idx) and bag_idx.is_cuda:
            x = x.index_select(1, bag_idx)
        elif bag_idx is not None:
            x = x[:, torch.as_tensor(np.asarray(bag_idx), device=x.device)]
        elif self.training:
            _, idx = draw_bag_distinct(x.shape[1])
            x = x[:, torch.as_tensor(idx, device=x.device)]
        B, L, nx, ny = x.shape
        x_in = x.reshape(B * L, 1, nx, ny)
        grid_r = grid.permute(2, 0, 1).unsqueeze(0).expand(B * L, 2, nx, ny)
        inp = torch.cat((x_in, grid_r), dim=1).permute(0, 2, 3, 1).contiguous()
        u = self.FNO_input(inp)                                      # (B*L, nx, ny, 1)
        h = ops.BagAttnFn.apply(u.reshape(B, L, nx * ny), grid.reshape(nx * ny, 2),
                                self.fc0.weight.data, self.fc0.bias.data)
        return _run_heads(self, h.view(B, nx, ny, -1))


class NIOFP_FNO(nn.Module):
    """1D FNO-NIO: 1d_FPE/NIOModules.py:87-155 (heads fno_drift/fno_diffusion) or
    1d_GPE/NIOModules.py:228-289 (single head ``fno_V``: ``heads=("fno_V",)``)."""

    accepts_dedup_bag = True    # forward(bag_idx=(unique idx, weights)): deduplicated bag

    def __init__(self, fno_layers, width, modes, output_dim, device,
                 heads: Sequence[str] = ("fno_drift", "fno_diffusion")):
        super().__init__()
        self.device = device
        self.fno_layers = fno_layers
        self.FNO_input = FNO1d(modes=12, width=4, n_layers=2, input_dim=2, output_dim=1,
                               device=self.device)
        self.fc0 = nn.Linear(2, width)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO1d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1, device=self.device))

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, Nx), grid (Nx, 1) -> (B, Nx, n_heads)."""
        x, L, lw = _select(self, x, bag_idx, dedup=True)
        B, _, nx = x.shape
        x_in = x.reshape(B * L, nx, 1)
        grid_r = grid.unsqueeze(0).expand(B * L, nx, 1)
        inp = torch.cat((x_in, grid_r), dim=2).contiguous()
        u = self.FNO_input(inp)                       # (B*L, nx, 1)
        h = _bag_mean_1d(self, u, grid, B, L, nx, lw)
        outs = [getattr(self, n)(h) for n in self._heads]
        return torch.cat(outs, dim=-1) if len(outs) > 1 else outs[0]


class NIOFP2D(nn.Module):
    """NIO (DeepONet branch/trunk + FNO heads), 2d_FPE/NIOModules.py:14-83 and
    2d_Non_conservative_FPE/NIOModules.py:13-82 (heads fno_Fx/fno_Fy)."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, heads: Sequence[str] = ("fno_drift", "fno_diffusion"),
                 branch_last_kernel=(2, 1)):
        super().__init__()
        output_dimensions = n_basis
        self.trunk = FFN(input_dimensions_trunk, output_dimensions, n_hidden_layers, neurons,
                         "leaky_relu", 0.0)
        self.fno_layers = fno_layers
        self.branch = Encoder2D(output_dimensions, last_kernel=branch_last_kernel)
        self.deeponet = DeepOnetNoBiasOrg(self.branch, self.trunk)
        self.fc0 = nn.Linear(3, width)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, nx, ny), grid (nx, ny, 2) -> (B, nx, ny, 2).  The DeepONet combiner and the
        bag mean run fused (ops.DeepONetBagFn: the bag mean commutes with w basis^T + b0, so
        the (B, L, nx ny) field of DeepOnetNoBiasOrg.forward is never formed)."""
        ops.require_device(x, grid)
        x, L, _ = _select(self, x, bag_idx)
        B, _, nx, ny = x.shape
        w = self.deeponet.branch(x.unsqueeze(2))                   # (B, L, n_basis)
        basis = self.deeponet.trunk(grid.reshape(-1, 2))           # (nx ny, n_basis)
        ubar = ops.DeepONetBagFn.apply(w, basis, self.deeponet.b0)
        h = _bag_mean_2d(self, ubar.view(B, 1, nx * ny), grid, B, 1, nx, ny)
        return _run_heads(self, h)          # the two FNO heads as one grouped launch chain


class NIOFP2D_attn(nn.Module):
    """NIO branch/trunk with the bag token attention, 2d_FPE/NIOModules.py:410-504 (NC copy with
    heads fno_Fx/fno_Fy: 2d_Non_conservative_FPE/NIOModules.py:406-).

    The DeepONet branch and trunk of NIOFP2D, then the attention of NIOFP2D_FNO_attn over the
    tokens [gx, gy, u_1..u_L] with u_l = (w_l . basis + b0) / sqrt(n_basis), fused with fc0 =
    Linear(1, width) (``.data``), then the two FNO heads.  ops.NIOAttnFn runs the attention on the
    tokens' coefficients (they have rank <= n_basis + 3), so the (B, L, nx ny) field is never
    formed.  Registration order (trunk, branch, deeponet, fc0, heads) follows the reference.

    The train-mode draw is WITH replacement (:449-450, unlike NIOFP2D_FNO_attn) and duplicates stay
    duplicate tokens: the branch's BatchNorm statistics and the softmax normaliser count them."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, heads: Sequence[str] = ("fno_drift", "fno_diffusion"),
                 branch_last_kernel=(2, 1)):
        super().__init__()
        output_dimensions = n_basis
        self.trunk = FFN(input_dimensions_trunk, output_dimensions, n_hidden_layers, neurons,
                         "leaky_relu", 0.0)
        self.fno_layers = fno_layers
        self.branch = Encoder2D(output_dimensions, last_kernel=branch_last_kernel)
        self.deeponet = DeepOnetNoBiasOrg(self.branch, self.trunk)
        self.fc0 = nn.Linear(1, width)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, nx, ny), grid (nx, ny, 2) -> (B, nx, ny, 2).  ``bag_idx`` overrides the
        train-mode draw (a host index list or a device int tensor); eval mode uses all T."""
        ops.require_device(x, grid)
        x, L, _ = _select(self, x, bag_idx)        # no dedup: duplicates are tokens of their own
        B, _, nx, ny = x.shape
        w = self.deeponet.branch(x.unsqueeze(2))                   # (B, L, n_basis)
        g = grid.reshape(-1, 2)
        basis = self.deeponet.trunk(g)                             # (nx ny, n_basis)
        h = ops.NIOAttnFn.apply(w, basis, self.deeponet.b0, g, self.fc0.weight.data,
                                self.fc0.bias.data)
        return _run_heads(self, h.view(B, nx, ny, -1))


class NIOFP2D_Trans(nn.Module):
    """Transolver snapshot encoder + FNO heads, 2d_FPE/NIOModules.py:85-166 and
    2d_Non_conservative_FPE/NIOModules.py:84-165 (both name the heads fno_drift / fno_diffusion).

    Every drawn snapshot goes through ``trans_input`` = Transolver2D(space_dim=2, n_layers=3,
    n_hidden=32, n_head=4, mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=16, H=W=61) as the point
    features [rho, gx, gy] (the reference calls ``trans_input(x_input, grid_r)``, whose forward
    concatenates ``(x, fx)``); the bag mean with fc0 (read through ``.data``, never trained) and
    the two FNO heads follow as in NIOFP2D_FNO.  ``branch`` = Encoder2D(n_basis) and the
    Transolver's ``placeholder`` are built and never used: they are part of the checkpoint layout.
    Registration order (branch, fc0, trans_input, heads) follows the reference.

    The Transolver has LayerNorm and no BatchNorm, so a snapshot's encoding does not depend on the
    rest of the bag: it runs once per distinct snapshot of the with-replacement draw, and the bag
    mean (and its adjoint) weights each by multiplicity / L."""

    GRID = 61      # the reference hard-codes H = W = 61 in the Transolver's reshape

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, heads: Sequence[str] = ("fno_drift", "fno_diffusion"),
                 branch_last_kernel=(2, 1)):
        super().__init__()
        output_dimensions = n_basis
        self.fno_layers = fno_layers
        self.branch = Encoder2D(output_dimensions, last_kernel=branch_last_kernel)
        self.fc0 = nn.Linear(3, width)
        self.trans_input = Transolver2D(space_dim=2, n_layers=3, n_hidden=32, dropout=0.0, n_head=4,
                                        Time_Input=False, mlp_ratio=1, fun_dim=1, out_dim=1,
                                        slice_num=16, ref=8, unified_pos=False, H=self.GRID,
                                        W=self.GRID)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))

    # parameters that never receive a gradient (the reference's Adam leaves them unchanged)
    unused_prefixes = ("branch.", "trans_input.placeholder", "fc0.")

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, 61, 61), grid (61, 61, 2) -> (B, 61, 61, 2).  ``bag_idx`` overrides the
        train-mode draw (draw_bag: with replacement); eval mode uses all T snapshots."""
        ops.require_device(x, grid)
        n = self.GRID
        if x.dim() != 4 or tuple(x.shape[2:]) != (n, n) or tuple(grid.shape) != (n, n, 2):
            raise ValueError(f"NIOFP2D_Trans: the reference's Transolver is built for a {n} x {n} grid; "
                             f"got x {tuple(x.shape)} and grid {tuple(grid.shape)}")
        x, L, lw = _select(self, x, bag_idx, dedup=True)
        B = x.shape[0]
        g = grid.permute(2, 0, 1).unsqueeze(0).expand(B * L, 2, n, n)
        inp = torch.cat((x.reshape(B * L, 1, n, n), g), dim=1)        # [rho, gx, gy] planes
        u = self.trans_input.forward_planes(inp)                      # (B L, 1, n, n)
        h = _bag_mean_2d(self, u, grid, B, L, n, n, lw)
        return _run_heads(self, h)


class NIOFP2D_Trans_attn(nn.Module):
    """Transolver snapshot encoder + bag token attention + FNO heads, 2d_FPE/NIOModules.py:169-296
    and 2d_Non_conservative_FPE/NIOModules.py:168-295 (both name the heads fno_drift /
    fno_diffusion).

    Every drawn snapshot goes through ``trans_input`` as in NIOFP2D_Trans; the tokens [gx, gy,
    u_1..u_L] then attend to each other (softmax(X X^T / sqrt(nx ny)) X) and the token outputs are
    fused with fc0 = Linear(3, width) read through ``.data``: the grid tokens' outputs with
    fc0.weight[:, 0] and [:, 1], the snapshot tokens' mean output with [:, 2].

    The reference assigns ``self.fc0`` twice: the second Linear(3, width) is created after the
    heads (it draws from the RNG there) and keeps the first one's slot in the module order.  The
    construction below does the same, so a seeded construction gives the reference's weights.

    The draw is with replacement.  The Transolver runs once per distinct snapshot, and
    ops.BagAttnMixFn runs the attention on the distinct tokens with their multiplicities: a
    duplicate's row and column of the attention matrix are copies of its original's, so the
    softmax normaliser counts each distinct token multiplicity times and nothing of the size of
    the drawn bag is formed."""

    GRID = NIOFP2D_Trans.GRID

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, nx, ny,
                 heads: Sequence[str] = ("fno_drift", "fno_diffusion"), branch_last_kernel=(2, 1)):
        super().__init__()
        output_dimensions = n_basis
        self.fno_layers = fno_layers
        self.branch = Encoder2D(output_dimensions, last_kernel=branch_last_kernel)
        self.fc0 = nn.Linear(3, width)
        self.trans_input = Transolver2D(space_dim=2, n_layers=3, n_hidden=32, dropout=0.0, n_head=4,
                                        Time_Input=False, mlp_ratio=1, fun_dim=1, out_dim=1,
                                        slice_num=16, ref=8, unified_pos=False, H=self.GRID,
                                        W=self.GRID)
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO2d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1))
        self.fc0 = nn.Linear(3, width)      # the reference's second assignment: drawn last
        self.nx = nx
        self.ny = ny

    unused_prefixes = NIOFP2D_Trans.unused_prefixes

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, 61, 61), grid (61, 61, 2) -> (B, 61, 61, 2).  ``bag_idx`` (a host index list)
        overrides the train-mode draw (draw_bag: with replacement); eval mode uses all T."""
        ops.require_device(x, grid)
        n = self.GRID
        if x.dim() != 4 or tuple(x.shape[2:]) != (n, n) or tuple(grid.shape) != (n, n, 2):
            raise ValueError(f"NIOFP2D_Trans_attn: the reference's Transolver is built for a {n} x {n} "
                             f"grid; got x {tuple(x.shape)} and grid {tuple(grid.shape)}")
        if isinstance(bag_idx, tuple) or (torch.is_tensor(bag_idx) and bag_idx.is_cuda):
            raise ValueError("NIOFP2D_Trans_attn: bag_idx must be a host index list (the attention "
                             "needs the number of draws; graph capture is not supported)")
        if bag_idx is None and self.training:
            _, bag_idx = draw_bag(x.shape[1])
        drawn = x.shape[1] if bag_idx is None else len(bag_idx)
        x, U, lw = _select(self, x, bag_idx, dedup=True)
        B = x.shape[0]
        g = grid.permute(2, 0, 1).unsqueeze(0).expand(B * U, 2, n, n)
        inp = torch.cat((x.reshape(B * U, 1, n, n), g), dim=1)        # [rho, gx, gy] planes
        u = self.trans_input.forward_planes(inp)                      # (B U, 1, n, n)
        h = ops.BagAttnMixFn.apply(u.reshape(B, U, n * n), grid.reshape(n * n, 2),
                                   self.fc0.weight.data, self.fc0.bias.data, lw, drawn)
        return _run_heads(self, h.view(B, n, n, -1))


class NIOFP3D(nn.Module):
    """3D NIO (DeepONet branch/trunk + one FNO3d), 2d_FPE/NIOModules.py:720-788 and
    2d_Non_conservative_FPE/NIOModules.py:716-784.  ``down`` selects Encoder3D_down (depth <= 32)
    instead of Encoder3D (33 <= depth <= 64)."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, device, down=False):
        super().__init__()
        output_dimensions = n_basis
        self.trunk = FFN(input_dimensions_trunk, output_dimensions, n_hidden_layers, neurons,
                         "leaky_relu", 0.0)
        self.fno_layers = fno_layers
        self.branch = (Encoder3D_down if down else Encoder3D)(output_dimensions)
        self.deeponet = DeepOnetNoBiasOrg(self.branch, self.trunk)
        self.fc0 = nn.Linear(4, width)
        self.device = device
        self.fno = FNO3d(modes=modes, width=width, n_layers=self.fno_layers, input_dim=width,
                         output_dim=output_dim, device=self.device)

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, Nx, Ny, Nz), grid (Nx, Ny, Nz, 3) -> (B, Nx, Ny, Nz, output_dim).  Composed as
        NIOFP2D: the DeepONet combiner fused with the bag mean (ops.DeepONetBagFn), the
        fixed-weight fc0 on [grid, ubar] (ops.BagMeanFn with d = 3), then FNO3d."""
        ops.require_device(x, grid)
        if x.dim() != 5 or tuple(grid.shape) != (*x.shape[2:], 3):
            raise ValueError(f"NIOFP3D: expected x (B, T, Nx, Ny, Nz) and grid (Nx, Ny, Nz, 3), got "
                             f"{tuple(x.shape)} and {tuple(grid.shape)}")
        x, L, _ = _select(self, x, bag_idx)        # no dedup: the branch is BatchNorm'd
        B, _, nx, ny, nz = x.shape
        S = nx * ny * nz
        w = self.deeponet.branch(x.unsqueeze(2))                   # (B, L, n_basis)
        basis = self.deeponet.trunk(grid.reshape(-1, 3))           # (S, n_basis)
        ubar = ops.DeepONetBagFn.apply(w, basis, self.deeponet.b0)
        h = ops.BagMeanFn.apply(ubar.view(B, 1, S), grid.reshape(S, 3), self.fc0.weight.data,
                                self.fc0.bias.data, None)
        return self.fno(h.view(B, nx, ny, nz, -1))


class NIOFP3D_FNO(nn.Module):
    """3D FNO-NIO: the composite of NIOFP2D_FNO (2d_FPE/NIOModules.py:508-581) on three axes,
    built from the reference's FNO3d (2d_FPE/FNOModules.py:290-366).  The reference has no such
    class; this is the project's own, so there is no ``branch`` to keep a checkpoint layout for.

    ``FNO_input`` = FNO3d(input_modes or modes, 4, 2, 4, 1) encodes every snapshot of the bag from
    [u, gx, gy, gz]; ``fc0`` = Linear(4, width), read through ``.data`` and never trained, maps
    [gx, gy, gz, bag mean] to the head's width (the bag-mean expression of NIOModules.py:565-575
    with one more grid channel); ``fno`` = FNO3d(modes, width, fno_layers, width, output_dim) is
    the single head (FNO3d.fc2 honours output_dim).  Train with
    ``train.trained_parameters(model, exclude_prefixes=("fc0.",))``."""

    accepts_dedup_bag = True    # forward(bag_idx=(unique idx, weights)): deduplicated bag

    def __init__(self, fno_layers, width, modes, output_dim, device, input_modes=None):
        super().__init__()
        self.device = device
        self.fno_layers = fno_layers
        self.FNO_input = FNO3d(modes=input_modes or modes, width=4, n_layers=2, input_dim=4,
                               output_dim=1, device=self.device)
        self.fc0 = nn.Linear(4, width)
        self.fno = FNO3d(modes=modes, width=width, n_layers=self.fno_layers, input_dim=width,
                         output_dim=output_dim, device=self.device)

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, Nx, Ny, Nz), grid (Nx, Ny, Nz, 3) -> (B, Nx, Ny, Nz, output_dim).  Train mode
        draws the bag as the reference does (draw_bag: with replacement) and runs the encoder
        once per distinct snapshot, weighted by multiplicity / L; eval mode uses all T snapshots;
        ``bag_idx=`` overrides the draw.  The encoder, its projection and the bag mean are
        ops.bag_encoder3d."""
        ops.require_device(x, grid)
        if x.dim() != 5 or tuple(grid.shape) != (*x.shape[2:], 3):
            raise ValueError(f"NIOFP3D_FNO: expected x (B, T, Nx, Ny, Nz) and grid (Nx, Ny, Nz, 3), got "
                             f"{tuple(x.shape)} and {tuple(grid.shape)}")
        lw = None
        if isinstance(bag_idx, tuple):
            idx_t, lw = bag_idx                       # device-resident deduplicated bag
        else:
            if torch.is_tensor(bag_idx):
                bag_idx = bag_idx.detach().cpu().numpy()
            if bag_idx is not None:
                idx = np.asarray(bag_idx)
            elif self.training:
                _, idx = draw_bag(x.shape[1])
            else:
                idx = np.arange(x.shape[1])
            idx, w = dedup_bag(idx)
            idx_t = torch.as_tensor(idx, device=x.device)
            if w is not None:
                lw = torch.as_tensor(w, device=x.device)
        h = ops.bag_encoder3d(self.FNO_input.padding, x, idx_t, lw, grid, self.fc0.weight.data,
                              self.fc0.bias.data, self.FNO_input.params())
        return self.fno(h)


class NIOFP3D_Trans(nn.Module):
    """3D Transolver-NIO: NIOFP2D_Trans on three axes, ending as NIOFP3D_FNO does.  The reference
    has the 3D Transolver (model/Transolver_Structured_Mesh_3D.py) and no composite around it;
    this is the project's own, so there is no ``branch`` to keep a checkpoint layout for.

    ``trans_input`` = Transolver3D(space_dim=3, n_layers=3, n_hidden=32, n_head=4, mlp_ratio=1,
    fun_dim=1, out_dim=1, slice_num=16, H, W, D = grid_shape) encodes every distinct snapshot of
    the bag from the point features [rho, gx, gy, gz] (it has LayerNorm and no BatchNorm, so a
    snapshot's encoding does not depend on the rest of the bag); ``fc0`` = Linear(4, width), read
    through ``.data`` and never trained, maps [gx, gy, gz, bag mean] to the head's width, the bag
    mean weighted by multiplicity / L; ``fno`` = FNO3d(modes, width, fno_layers, width,
    output_dim) is the single head."""

    def __init__(self, fno_layers, width, modes, output_dim, device, grid_shape):
        super().__init__()
        self.device = device
        self.fno_layers = fno_layers
        self.grid_shape = tuple(int(n) for n in grid_shape)
        if len(self.grid_shape) != 3:
            raise ValueError(f"NIOFP3D_Trans: grid_shape must be (Nx, Ny, Nz), got {grid_shape}")
        H, W, D = self.grid_shape
        self.trans_input = Transolver3D(space_dim=3, n_layers=3, n_hidden=32, dropout=0.0, n_head=4,
                                        Time_Input=False, mlp_ratio=1, fun_dim=1, out_dim=1,
                                        slice_num=16, ref=8, unified_pos=False, H=H, W=W, D=D)
        self.fc0 = nn.Linear(4, width)
        self.fno = FNO3d(modes=modes, width=width, n_layers=self.fno_layers, input_dim=width,
                         output_dim=output_dim, device=self.device)

    # parameters that never receive a gradient
    unused_prefixes = ("trans_input.placeholder", "fc0.")

    def forward(self, x, grid, bag_idx=None):
        """x (B, T, Nx, Ny, Nz), grid (Nx, Ny, Nz, 3) -> (B, Nx, Ny, Nz, output_dim).  ``bag_idx``
        overrides the train-mode draw (draw_bag: with replacement); eval mode uses all T
        snapshots."""
        ops.require_device(x, grid)
        n = self.grid_shape
        if x.dim() != 5 or tuple(x.shape[2:]) != n or tuple(grid.shape) != (*n, 3):
            raise ValueError(f"NIOFP3D_Trans: built for a {n[0]} x {n[1]} x {n[2]} grid; got x "
                             f"{tuple(x.shape)} and grid {tuple(grid.shape)}")
        x, L, lw = _select(self, x, bag_idx, dedup=True)
        B, P = x.shape[0], n[0] * n[1] * n[2]
        g = grid.permute(3, 0, 1, 2).unsqueeze(0).expand(B * L, 3, *n)
        inp = torch.cat((x.reshape(B * L, 1, *n), g), dim=1)          # [rho, gx, gy, gz] planes
        u = self.trans_input.forward_planes(inp)                      # (B L, 1, Nx, Ny, Nz)
        h = ops.BagMeanFn.apply(u.reshape(B, L, P), grid.reshape(P, 3), self.fc0.weight.data,
                                self.fc0.bias.data, lw)
        return self.fno(h.view(B, *n, -1))


class NIOFP(nn.Module):
    """1D NIO, 1d_FPE/NIOModules.py:15-84 (``heads=("fno_V",)`` + GPE encoder kernels
    give NIOFP_schrodinger, 1d_GPE/NIOModules.py:160-223)."""

    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, device,
                 heads: Sequence[str] = ("fno_drift", "fno_diffusion"),
                 encoder_kernels=(5, 4, 15), encoder_conv4=False):
        super().__init__()
        output_dimensions = n_basis
        self.trunk = FFN(input_dimensions_trunk, output_dimensions, n_hidden_layers, neurons,
                         "leaky_relu", 0.0)
        self.fno_layers = fno_layers
        self.branch = Encoder(output_dimensions, final_kernels=encoder_kernels,
                              apply_conv4=encoder_conv4)
        self.deeponet = DeepOnetNoBiasOrg(self.branch, self.trunk)
        self.fc0 = nn.Linear(2, width)
        self.device = device
        self._heads = tuple(heads)
        for name in self._heads:
            setattr(self, name, FNO1d(modes=modes, width=width, n_layers=self.fno_layers,
                                      input_dim=width, output_dim=1, device=self.device))

    @property
    def unused_prefixes(self):
        """Parameters that never receive a gradient: the 1d_FPE encoder builds final_conv4 but
        does not apply it (1d_FPE/Baselines.py:254-287); the reference's Adam skips them."""
        return () if self.branch.apply_conv4 else ("branch.final_conv4.",)

    def forward(self, x, grid, bag_idx=None):
        ops.require_device(x, grid)
        x, L, _ = _select(self, x, bag_idx)
        B, _, nx = x.shape
        w = self.deeponet.branch(x)                                  # (B, L, n_basis)
        basis = self.deeponet.trunk(grid)                            # (nx, n_basis)
        ubar = ops.DeepONetBagFn.apply(w, basis, self.deeponet.b0)  # fused combiner + bag mean
        h = _bag_mean_1d(self, ubar.view(B, 1, nx), grid, B, 1, nx)
        outs = [getattr(self, n)(h) for n in self._heads]
        return torch.cat(outs, dim=-1) if len(outs) > 1 else outs[0]


class NIOFP_schrodinger(NIOFP):
    def __init__(self, input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                 width, modes, output_dim, device):
        super().__init__(input_dimensions_trunk, n_hidden_layers, neurons, n_basis, fno_layers,
                         width, modes, output_dim, device, heads=("fno_V",),
                         encoder_kernels=(5, 7, 4), encoder_conv4=True)
