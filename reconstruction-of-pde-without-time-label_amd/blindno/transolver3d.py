"""Structured-mesh 3D Transolver (model/Transolver_Structured_Mesh_3D.py with
Physics_Attention_Structured_Mesh_3D, model/Physics_Attention.py:119-175) on the HIP kernels.

Activations stay channel planes (S, C, H, W, D) from the first layer to the last.  Per block: the
two 3x3x3 convolutions of the attention run as one 64-channel ``ops.Conv3dFn``; physics attention
is ``ops.PhysAttnFn`` on the (S, 64, H, W D) view (the kernels read H W D points and never the
mesh's shape), with the residual in its deslice store; ``ln_1`` is ``ops.LayerNormPlanesFn``;
``ln_2`` + ``mlp`` + the residual are one ``ops.PlaneMLPFn`` (csrc/planemlp.hip), which keeps the
hidden layer in registers and recomputes it in the backward; ``preprocess`` is one ``PlaneMLPFn``
as well.  The last block's ``ln_3`` + ``mlp2`` (32 -> 1) are ``LayerNormPlanesFn`` and a 1x1x1
convolution.

Module and parameter names, shapes and registration order equal the reference ``Model``'s, so its
``state_dict`` loads with ``strict=True``; initialisation draws in the reference's order, as
described in ``transolver.py``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class _MLP3D(nn.Module):
    """The reference's MLP with n_layers = 0, res = False (Linear, GELU, Linear) as one fused
    launch, with the LayerNorm in front of it and the residual behind it where the block has them."""

    def __init__(self, n_input, n_hidden, n_output):
        super().__init__()
        self.linear_pre = nn.Sequential(nn.Linear(n_input, n_hidden), nn.GELU())
        self.linear_post = nn.Linear(n_hidden, n_output)
        self.linears = nn.ModuleList()

    def forward(self, x, res=None, ln=None):
        pre, post = self.linear_pre[0], self.linear_post
        if ln is None:
            return ops.PlaneMLPFn.apply(x, pre.weight, pre.bias, post.weight, post.bias, res)
        return ops.PlaneMLPFn.apply(x, pre.weight, pre.bias, post.weight, post.bias, res, ln.weight,
                                    ln.bias, ln.eps)


class PhysicsAttention3D(nn.Module):
    """Physics_Attention_Structured_Mesh_3D (model/Physics_Attention.py:119-175) on planes."""

    def __init__(self, dim, heads=4, dim_head=8, dropout=0.0, slice_num=16, H=32, W=32, D=32, kernel=3):
        super().__init__()
        if dropout != 0.0:
            raise ValueError("PhysicsAttention3D: dropout must be 0 (the reference's setting)")
        if (heads, dim_head, slice_num) != (4, 8, 16) or dim != 32:
            raise ValueError("PhysicsAttention3D: the HIP kernels take heads = 4, dim_head = 8, "
                             f"slice_num = 16, dim = 32; got heads = {heads}, dim_head = {dim_head}, "
                             f"slice_num = {slice_num}, dim = {dim}")
        inner = dim_head * heads
        self.dim_head, self.heads, self.H, self.W, self.D = dim_head, heads, H, W, D
        self.scale = dim_head ** -0.5
        self.temperature = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.in_project_x = nn.Conv3d(dim, inner, kernel, 1, kernel // 2)
        self.in_project_fx = nn.Conv3d(dim, inner, kernel, 1, kernel // 2)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))

    def forward(self, x, res=None):
        """x (S, 32, H, W, D) -> to_out(attention) (+ res), planes."""
        mesh = (self.H, self.W, self.D)
        if x.dim() != 5 or tuple(x.shape[2:]) != mesh:
            raise ValueError(f"PhysicsAttention3D: built for {mesh}, got {tuple(x.shape)}")
        S = x.shape[0]
        k = self.in_project_x.kernel_size[0]
        wcat = torch.cat((self.in_project_x.weight, self.in_project_fx.weight), 0)
        bcat = torch.cat((self.in_project_x.bias, self.in_project_fx.bias), 0)
        xf = ops.conv3d(x, wcat, bcat, 1, k // 2)
        flat = (self.H, self.W * self.D)
        y = ops.PhysAttnFn.apply(xf.view(S, xf.shape[1], *flat), self.temperature,
                                 self.in_project_slice.weight, self.in_project_slice.bias,
                                 self.to_q.weight, self.to_k.weight, self.to_v.weight,
                                 self.to_out[0].weight, self.to_out[0].bias,
                                 None if res is None else res.reshape(S, -1, *flat))
        return y.view(S, -1, *mesh)


class TransolverBlock3D(nn.Module):
    """Transolver_block (model/Transolver_Structured_Mesh_3D.py:41-76) on planes."""

    def __init__(self, num_heads, hidden_dim, dropout=0.0, act="gelu", mlp_ratio=1, last_layer=False,
                 out_dim=1, slice_num=16, H=32, W=32, D=32):
        super().__init__()
        if act != "gelu":
            raise ValueError("TransolverBlock3D: act must be 'gelu'")
        if mlp_ratio != 1:
            raise ValueError("TransolverBlock3D: the fused MLP kernel takes mlp_ratio = 1")
        self.last_layer = last_layer
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.Attn = PhysicsAttention3D(hidden_dim, heads=num_heads, dim_head=hidden_dim // num_heads,
                                       dropout=dropout, slice_num=slice_num, H=H, W=W, D=D)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = _MLP3D(hidden_dim, hidden_dim * mlp_ratio, hidden_dim)
        if self.last_layer:
            self.ln_3 = nn.LayerNorm(hidden_dim)
            self.mlp2 = nn.Linear(hidden_dim, out_dim)

    @staticmethod
    def _ln(ln, x):
        return ops.LayerNormPlanesFn.apply(x, ln.weight, ln.bias, ln.eps)

    def forward(self, fx):
        fx = self.Attn(self._ln(self.ln_1, fx), res=fx)       # the residual rides the deslice store
        fx = self.mlp(fx, res=fx, ln=self.ln_2)               # ln_2, mlp and the residual: one launch
        if self.last_layer:
            w = self.mlp2.weight
            return ops.conv3d(self._ln(self.ln_3, fx), w.view(*w.shape, 1, 1, 1), self.mlp2.bias, 1, 0)
        return fx


class Transolver3D(nn.Module):
    """Model (model/Transolver_Structured_Mesh_3D.py:79-191) without Time_Input / unified_pos."""

    def __init__(self, space_dim=3, n_layers=3, n_hidden=32, n_head=4, mlp_ratio=1, fun_dim=1,
                 out_dim=1, slice_num=16, H=32, W=32, D=32, dropout=0.0, Time_Input=False, act="gelu",
                 ref=8, unified_pos=False):
        super().__init__()
        if Time_Input or unified_pos:
            raise ValueError("Transolver3D: Time_Input and unified_pos are not supported")
        if fun_dim + space_dim != 4:
            raise ValueError("Transolver3D: the fused preprocess kernel takes space_dim + fun_dim = 4; "
                             f"got {space_dim} + {fun_dim}")
        self.__name__ = "Transolver_3D"
        self.H, self.W, self.D, self.ref, self.unified_pos = H, W, D, ref, unified_pos
        self.Time_Input, self.n_hidden, self.space_dim = Time_Input, n_hidden, space_dim
        self.preprocess = _MLP3D(fun_dim + space_dim, n_hidden * 2, n_hidden)
        self.blocks = nn.ModuleList([
            TransolverBlock3D(num_heads=n_head, hidden_dim=n_hidden, dropout=dropout, act=act,
                              mlp_ratio=mlp_ratio, out_dim=out_dim, slice_num=slice_num, H=H, W=W, D=D,
                              last_layer=(i == n_layers - 1)) for i in range(n_layers)])
        self.apply(self._init_weights)
        self.placeholder = nn.Parameter((1 / n_hidden) * torch.rand(n_hidden, dtype=torch.float))

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward_planes(self, inp):
        """inp (S, space_dim + fun_dim, H, W, D), channels in the order of ``cat((x, fx), -1)`` ->
        (S, out_dim, H, W, D)."""
        ops.require_device(inp)
        mesh = (self.H, self.W, self.D)
        if inp.dim() != 5 or tuple(inp.shape[2:]) != mesh:
            raise ValueError(f"Transolver3D: built for {mesh} planes, got {tuple(inp.shape)}")
        fx = self.preprocess(inp)
        for block in self.blocks:
            fx = block(fx)
        return fx

    def forward(self, x, fx, T=None):
        """The reference's signature: x (S, N, a), fx (S, N, b), concatenated as cat((x, fx), -1)
        -> (S, N, out_dim)."""
        if fx is None:
            raise ValueError("Transolver3D: fx is required (the placeholder path is not supported)")
        if T is not None:
            raise ValueError("Transolver3D: Time_Input is not supported")
        S = x.shape[0]
        inp = torch.cat((x, fx), -1).reshape(S, self.H, self.W, self.D, -1).permute(0, 4, 1, 2, 3)
        out = self.forward_planes(inp.contiguous())
        return out.permute(0, 2, 3, 4, 1).reshape(S, self.H * self.W * self.D, -1)
