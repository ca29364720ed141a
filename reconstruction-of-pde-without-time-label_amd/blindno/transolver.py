"""Structured-mesh 2D Transolver (model/Transolver_Structured_Mesh_2D.py, model/Physics_Attention.py
of the two 2D experiments; the copies are identical) on the HIP kernels.

Activations stay channel planes (S, C, H, W) from the first layer to the last: the two 3x3
convolutions of the attention run as one 64-channel ``ops.conv2d``, physics attention is
``ops.PhysAttnFn`` (csrc/physattn.hip), the LayerNorms are ``ops.LayerNormPlanesFn`` and every
pointwise ``nn.Linear`` is a 1x1 ``ops.conv2d`` on the planes, so the reference's (S, N, C) <->
(S, C, H, W) permutes do not exist.  GELU (exact erf form, ``nn.GELU``) is a torch elementwise op.

Module and parameter names, shapes and registration order equal the reference ``Model``'s, so its
``state_dict`` loads with ``strict=True``; initialisation draws in the reference's order
(``orthogonal_`` on in_project_slice inside the attention's constructor, then ``Model.apply``'s
truncated normal over every Linear -- in_project_slice included, as in the reference -- zero
biases, temperature 0.5, ``placeholder`` uniform / n_hidden).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def _pointwise(x, lin: nn.Linear):
    """nn.Linear over the channel planes of x (S, Ci, H, W)."""
    return ops.conv2d(x, lin.weight.view(lin.out_features, lin.in_features, 1, 1), lin.bias,
                      (1, 1), (0, 0))


class _MLP(nn.Module):
    """The reference's MLP with n_layers = 0, res = False: Linear, GELU, Linear."""

    def __init__(self, n_input, n_hidden, n_output):
        super().__init__()
        self.linear_pre = nn.Sequential(nn.Linear(n_input, n_hidden), nn.GELU())
        self.linear_post = nn.Linear(n_hidden, n_output)
        self.linears = nn.ModuleList()

    def forward(self, x, res=None):
        y = _pointwise(F.gelu(_pointwise(x, self.linear_pre[0])), self.linear_post)
        return y if res is None else y + res


class PhysicsAttention2D(nn.Module):
    """Physics_Attention_Structured_Mesh_2D (model/Physics_Attention.py:60-116) on planes."""

    def __init__(self, dim, heads=4, dim_head=8, dropout=0.0, slice_num=16, H=61, W=61, kernel=3):
        super().__init__()
        if dropout != 0.0:
            raise ValueError("PhysicsAttention2D: dropout must be 0 (the reference's setting)")
        if (heads, dim_head, slice_num) != (4, 8, 16) or dim != 32:
            raise ValueError("PhysicsAttention2D: the HIP kernels take heads = 4, dim_head = 8, "
                             f"slice_num = 16, dim = 32 (NIOFP2D_Trans); got heads = {heads}, "
                             f"dim_head = {dim_head}, slice_num = {slice_num}, dim = {dim}")
        inner = dim_head * heads
        self.dim_head, self.heads, self.H, self.W = dim_head, heads, H, W
        self.scale = dim_head ** -0.5
        self.temperature = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.in_project_x = nn.Conv2d(dim, inner, kernel, 1, kernel // 2)
        self.in_project_fx = nn.Conv2d(dim, inner, kernel, 1, kernel // 2)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))

    def forward(self, x, res=None):
        """x (S, 32, H, W) -> to_out(attention) (+ res), planes."""
        if tuple(x.shape[2:]) != (self.H, self.W):
            raise ValueError(f"PhysicsAttention2D: built for {self.H} x {self.W}, got {tuple(x.shape)}")
        k = self.in_project_x.kernel_size[0]
        wcat = torch.cat((self.in_project_x.weight, self.in_project_fx.weight), 0)
        bcat = torch.cat((self.in_project_x.bias, self.in_project_fx.bias), 0)
        xf = ops.conv2d(x, wcat, bcat, (1, 1), (k // 2, k // 2))
        return ops.PhysAttnFn.apply(xf, self.temperature, self.in_project_slice.weight,
                                    self.in_project_slice.bias, self.to_q.weight, self.to_k.weight,
                                    self.to_v.weight, self.to_out[0].weight, self.to_out[0].bias, res)


class TransolverBlock2D(nn.Module):
    """Transolver_block (model/Transolver_Structured_Mesh_2D.py:40-74) on planes."""

    def __init__(self, num_heads, hidden_dim, dropout=0.0, act="gelu", mlp_ratio=1, last_layer=False,
                 out_dim=1, slice_num=16, H=61, W=61):
        super().__init__()
        if act != "gelu":
            raise ValueError("TransolverBlock2D: act must be 'gelu'")
        self.last_layer = last_layer
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.Attn = PhysicsAttention2D(hidden_dim, heads=num_heads, dim_head=hidden_dim // num_heads,
                                       dropout=dropout, slice_num=slice_num, H=H, W=W)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = _MLP(hidden_dim, hidden_dim * mlp_ratio, hidden_dim)
        if self.last_layer:
            self.ln_3 = nn.LayerNorm(hidden_dim)
            self.mlp2 = nn.Linear(hidden_dim, out_dim)

    @staticmethod
    def _ln(ln, x):
        return ops.LayerNormPlanesFn.apply(x, ln.weight, ln.bias, ln.eps)

    def forward(self, fx):
        fx = self.Attn(self._ln(self.ln_1, fx), res=fx)       # the residual rides the deslice store
        fx = self.mlp(self._ln(self.ln_2, fx), res=fx)
        if self.last_layer:
            return _pointwise(self._ln(self.ln_3, fx), self.mlp2)
        return fx


class Transolver2D(nn.Module):
    """Model (model/Transolver_Structured_Mesh_2D.py:77-174) without Time_Input / unified_pos."""

    def __init__(self, space_dim=2, n_layers=3, n_hidden=32, n_head=4, mlp_ratio=1, fun_dim=1,
                 out_dim=1, slice_num=16, H=61, W=61, dropout=0.0, Time_Input=False, act="gelu",
                 ref=8, unified_pos=False):
        super().__init__()
        if Time_Input or unified_pos:
            raise ValueError("Transolver2D: Time_Input and unified_pos are not supported "
                             "(NIOFP2D_Trans uses neither)")
        self.__name__ = "Transolver_2D"
        self.H, self.W, self.ref, self.unified_pos = H, W, ref, unified_pos
        self.Time_Input, self.n_hidden, self.space_dim = Time_Input, n_hidden, space_dim
        self.preprocess = _MLP(fun_dim + space_dim, n_hidden * 2, n_hidden)
        self.blocks = nn.ModuleList([
            TransolverBlock2D(num_heads=n_head, hidden_dim=n_hidden, dropout=dropout, act=act,
                              mlp_ratio=mlp_ratio, out_dim=out_dim, slice_num=slice_num, H=H, W=W,
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
        """inp (S, space_dim + fun_dim, H, W), channels in the order of ``cat((x, fx), -1)`` ->
        (S, out_dim, H, W)."""
        ops.require_device(inp)
        if inp.dim() != 4 or tuple(inp.shape[2:]) != (self.H, self.W):
            raise ValueError(f"Transolver2D: built for {self.H} x {self.W} planes, got {tuple(inp.shape)}")
        fx = self.preprocess(inp)
        for block in self.blocks:
            fx = block(fx)
        return fx

    def forward(self, x, fx, T=None):
        """The reference's signature: x (S, N, a), fx (S, N, b), concatenated as cat((x, fx), -1)
        -> (S, N, out_dim)."""
        if fx is None:
            raise ValueError("Transolver2D: fx is required (the placeholder path is not supported)")
        if T is not None:
            raise ValueError("Transolver2D: Time_Input is not supported")
        S = x.shape[0]
        inp = torch.cat((x, fx), -1).reshape(S, self.H, self.W, -1).permute(0, 3, 1, 2).contiguous()
        out = self.forward_planes(inp)
        return out.permute(0, 2, 3, 1).reshape(S, self.H * self.W, -1)
