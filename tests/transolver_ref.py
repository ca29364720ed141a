"""Restatements, in plain torch and any precision (float64 as the checker, float32 for the error
floor), of the structured-mesh Transolver (model/Transolver_Structured_Mesh_2D.py,
model/Physics_Attention.py) and of NIOFP2D_Trans (2d_FPE/NIOModules.py:85-166), written from the
formulas of include/blindno_physattn.h for tests/test_transolver_ref.py, tests/test_gpu_physattn.py
and tests/test_gpu_trans.py.

  phys_attn      physics attention on planes xm, fm (S, 32, N): every intermediate by name
  layer_norm     LayerNorm over the channel planes
  transolver     the three-block model on point features (S, N, 3) -> (S, N, 1)
  niofp2d_trans  the whole model: Transolver per snapshot, bag mean with fc0, the two FNO heads
"""
import math

import torch
import torch.nn.functional as F

import oracle.fno_ref as ref

HEADS, D, G = 4, 8, 16
NORM_EPS = 1e-5


def rescaled_state(shapes, seed, rescale):
    """recipe.make_state(shapes, seed) with every parameter whose name ends in a key of ``rescale``
    multiplied by that key's factor (the golden generator's parameter choice: the recipe's scales
    leave the attention branch negligible; tests/golden/make_golden_trans.py)."""
    import numpy as np
    from recipe import make_state
    st = make_state(shapes, seed=seed)
    for name in st:
        for suffix, f in rescale.items():
            if name.endswith(suffix):
                st[name] = (st[name] * np.float32(f)).astype(st[name].dtype)
    return st


def phys_attn(xm, fm, temperature, Ws, bs, Wq, Wk, Wv, Wo, bo, res=None, uniform=False):
    """xm, fm (S, 32, N) planes -> dict with y (S, 32, N) = to_out(deslice) (+ res) and w (S, 4,
    16, N), norm (S, 4, 16), tok, otok (S, 4, 16, 8), A (S, 4, 16, 16).  ``uniform`` replaces w by
    1/16 (the generator's proof that the attention matters)."""
    S, C, N = xm.shape
    xh = xm.reshape(S, HEADS, D, N)
    fh = fm.reshape(S, HEADS, D, N)
    T = temperature.reshape(1, HEADS, 1, 1).clamp(0.1, 5.0)
    logits = (torch.einsum("gc,shcn->shgn", Ws, xh) + bs.view(1, 1, G, 1)) / T
    w = torch.softmax(logits, dim=2)
    if uniform:
        w = torch.full_like(w, 1.0 / G)
    norm = w.sum(-1)                                                  # (S, 4, 16)
    tok = torch.einsum("shgn,shcn->shgc", w, fh) / (norm + NORM_EPS).unsqueeze(-1)
    q, k, v = tok @ Wq.t(), tok @ Wk.t(), tok @ Wv.t()
    A = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)
    otok = A @ v
    ox = torch.einsum("shgn,shgc->shcn", w, otok).reshape(S, C, N)
    y = torch.einsum("oi,sin->son", Wo, ox) + bo.view(1, C, 1)
    if res is not None:
        y = y + res
    return {"y": y, "w": w, "norm": norm, "tok": tok, "A": A, "otok": otok}


def layer_norm(x, gamma, beta, eps=1e-5):
    """x (S, C, N): LayerNorm over C (biased variance)."""
    m = x.mean(1, keepdim=True)
    v = ((x - m) ** 2).mean(1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)


def _lin(x, p, name):
    """Linear over the channel planes of x (S, Ci, N)."""
    y = torch.einsum("oi,sin->son", p[name + ".weight"], x)
    return y + p[name + ".bias"].view(1, -1, 1) if name + ".bias" in p else y


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(p, fx, H, W, last, uniform=False, record=None):
    """Transolver_block on planes fx (S, 32, N)."""
    S, C, N = fx.shape
    x = layer_norm(fx, p["ln_1.weight"], p["ln_1.bias"]).reshape(S, C, H, W)
    xm = F.conv2d(x, p["Attn.in_project_x.weight"], p["Attn.in_project_x.bias"], padding=1).reshape(S, C, N)
    fm = F.conv2d(x, p["Attn.in_project_fx.weight"], p["Attn.in_project_fx.bias"], padding=1).reshape(S, C, N)
    a = phys_attn(xm, fm, p["Attn.temperature"], p["Attn.in_project_slice.weight"],
                  p["Attn.in_project_slice.bias"], p["Attn.to_q.weight"], p["Attn.to_k.weight"],
                  p["Attn.to_v.weight"], p["Attn.to_out.0.weight"], p["Attn.to_out.0.bias"], res=fx,
                  uniform=uniform)
    if record is not None:
        record.append(a["w"].detach())
    fx = a["y"]
    h = layer_norm(fx, p["ln_2.weight"], p["ln_2.bias"])
    fx = _lin(_gelu(_lin(h, p, "mlp.linear_pre.0")), p, "mlp.linear_post") + fx
    if last:
        return _lin(layer_norm(fx, p["ln_3.weight"], p["ln_3.bias"]), p, "mlp2")
    return fx


def transolver(p, inp, H, W, n_layers=3, uniform=False, record=None):
    """Model.forward on planes: inp (S, 3, N) = cat((x, fx), -1) transposed -> (S, 1, N).  ``p``
    holds the Model's state_dict (any dtype; the computation runs in inp's)."""
    fx = _lin(_gelu(_lin(inp, p, "preprocess.linear_pre.0")), p, "preprocess.linear_post")
    for i in range(n_layers):
        fx = block(ref.sub_params(p, f"blocks.{i}"), fx, H, W, i == n_layers - 1, uniform, record)
    return fx


def trans_bag_field(p, x, grid, idx=None, uniform=False, record=None, dt=torch.float64):
    """The field the heads read: fc0([grid, mean_l Transolver(snapshot l)]) (B, nx, ny, width)."""
    x = x.to(dt)
    if idx is not None:
        x = x[:, list(idx)]
    B, L, nx, ny = x.shape
    g = grid.to(dt)
    gp = g.permute(2, 0, 1).reshape(1, 2, nx * ny).expand(B * L, 2, nx * ny)
    inp = torch.cat((x.reshape(B * L, 1, nx * ny), gp), 1)           # [rho, gx, gy]
    tp = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in ref.sub_params(p, "trans_input").items()}
    u = transolver(tp, inp, nx, ny, uniform=uniform, record=record).reshape(B, L, nx, ny)
    w0, b0 = p["fc0.weight"].detach().to(dt), p["fc0.bias"].detach().to(dt)
    return (g @ w0[:, :2].t()).unsqueeze(0) + u.mean(1).unsqueeze(-1) * w0[:, 2] + b0


def niofp2d_trans(p, x, grid, idx=None, heads=("fno_drift", "fno_diffusion"), uniform=False, record=None):
    """NIOFP2D_Trans.forward in float64 (``idx`` replaces the train-mode draw; None = eval)."""
    h = trans_bag_field(p, x, grid, idx, uniform, record, ref.DT)
    return torch.cat([ref.fno2d(ref.sub_params(p, hd), h) for hd in heads], dim=-1)
