"""Float64 (or any precision) restatements of NIOFP2D_attn's bag attention
(2d_FPE/NIOModules.py:410-504) for tests/test_nio2d_attn.py and tests/test_gpu_nioattn.py.

  attn_math     the coefficient-space formulas of include/blindno_nioattn.h, term by term, in the
                precision asked for (forward and the hand-derived backward)
  attn_direct   the tokens materialised, oracle.fno_ref.bag_attention on them, float64 autograd:
                shares neither the low-rank rewriting nor the hand-derived backward
  niofp2d_attn  the whole model from oracle.fno_ref's pieces (encoder2d, ffn, deeponet_nobias,
                bag_attention, fno2d)
"""
import math

import torch

import oracle.fno_ref as ref


def attn_math(w, basis, b0, grid, fc0w, fc0b, dy, dt):
    """w (B, L, P), basis (S, P), b0 scalar, grid (S, 2), fc0w / fc0b (width), dy (B, S, width)."""
    w, basis, b0, grid, fc0w, fc0b, dy = (t.to(dt) for t in (w, basis, b0, grid, fc0w, fc0b, dy))
    B, L, P = w.shape
    S = basis.shape[0]
    T, Q = L + 2, P + 3
    scale = 1.0 / math.sqrt(P)
    rs = math.sqrt(S)
    Phi = torch.cat((grid, scale * basis, scale * torch.ones(S, 1, dtype=dt)), 1)      # (S, Q)
    C = torch.zeros(B, T, Q, dtype=dt)
    C[:, 0, 0] = 1
    C[:, 1, 1] = 1
    C[:, 2:, 2:2 + P] = w
    C[:, 2:, Q - 1] = b0.reshape(())
    Ct = C.transpose(1, 2)
    M = Phi.t() @ Phi                                                      # (Q, Q)
    logits = C @ M @ Ct / rs
    A = torch.softmax(logits, -1)                                          # row maximum subtracted
    cs = A.sum(1)                                                          # cs_s = sum_t A[t, s]
    v = (Ct @ cs.unsqueeze(-1)).squeeze(-1) / T                            # (B, Q)
    m = v @ Phi.t()                                                        # (B, S)
    y = m.unsqueeze(-1) * fc0w + fc0b
    dm = dy @ fc0w                                                         # (B, S)
    dv = dm @ Phi                                                          # (B, Q)
    dcs = (C @ dv.unsqueeze(-1)).squeeze(-1) / T                           # (B, T)
    r = (A @ dcs.unsqueeze(-1)).squeeze(-1)
    dS = A * (dcs.unsqueeze(1) - r.unsqueeze(2))
    soft = (dS + dS.transpose(1, 2)) @ C @ M / rs                          # the softmax path of dC
    dC = cs.unsqueeze(2) * dv.unsqueeze(1) / T + soft
    dM = (Ct @ dS @ C).sum(0) / rs
    dPhi = Phi @ (dM + dM.t()) + dm.t() @ v
    return {"M": M, "logits": logits, "A": A, "cs": cs, "v": v, "y": y,
            "dw": dC[:, 2:, 2:2 + P], "db0": dC[:, 2:, Q - 1].sum().reshape(1),
            "dbasis": scale * dPhi[:, 2:2 + P], "soft_w": soft[:, 2:, 2:2 + P]}


def tokens(w, basis, b0):
    """DeepOnetNoBiasOrg.forward: (B, L, S)."""
    return ref.deeponet_nobias(w, basis, b0)


def attn_direct(w, basis, b0, grid, fc0w, fc0b, dy):
    """y, dw, dbasis, db0 by float64 autograd of the reference's own composition."""
    wd, bd, b0d = (t.detach().double().clone().requires_grad_(True) for t in (w, basis, b0))
    B, L, _ = wd.shape
    S = bd.shape[0]
    u = tokens(wd, bd, b0d)
    gcf = grid.double().t().unsqueeze(0).expand(B, 2, S).reshape(B, 2, S, 1)
    y = ref.bag_attention(u.view(B, L, S, 1), gcf, fc0w.double().view(-1, 1), fc0b.double()).view(B, S, -1)
    (y * dy.double()).sum().backward()
    return {"y": y.detach(), "dw": wd.grad, "dbasis": bd.grad, "db0": b0d.grad.reshape(1)}


def uniform_attention_output(w, basis, b0, grid, fc0w, fc0b):
    """The model's fused field with A replaced by the uniform matrix 1/T (float64)."""
    B, L, _ = w.shape
    S = basis.shape[0]
    X = torch.cat((grid.double().t().unsqueeze(0).expand(B, 2, S), tokens(w.double(), basis.double(), b0.double())), 1)
    m = X.mean(1)                                                          # (1/T) sum_t (1/T) sum_s X_s T
    return m.unsqueeze(-1) * fc0w.double() + fc0b.double()


def niofp2d_attn(p, x, grid, idx=None, n_hidden_layers=3, heads=("fno_drift", "fno_diffusion"),
                 branch_masks=None, record=None):
    """NIOFP2D_attn.forward, 2d_FPE/NIOModules.py:443-504 (NC: heads fno_Fx/fno_Fy).  ``idx``
    replaces the train-mode draw (:449-450, WITH replacement); None = eval.  ``record`` (optional
    dict) receives the tokens' attention matrix, the fused field, and the fused field and the model
    output under a uniform attention matrix."""
    DT = ref.DT
    x = x.to(DT)
    if idx is not None:
        x = x[:, list(idx)]
    B, L, nx, ny = x.shape
    g = grid.to(DT)
    w = ref.encoder2d(ref.sub_params(p, "branch"), x.unsqueeze(2), branch_masks)
    basis = ref.ffn(ref.sub_params(p, "trunk"), g.reshape(-1, 2), n_hidden_layers)
    u = ref.deeponet_nobias(w, basis, p["deeponet.b0"]).view(B, L, nx, ny)
    gcf = g.unsqueeze(0).repeat(B, 1, 1, 1).permute(0, 3, 1, 2)
    h = ref.bag_attention(u, gcf, p["fc0.weight"], p["fc0.bias"])
    if record is not None:
        xt = torch.cat((gcf, u), 1).reshape(B, L + 2, nx * ny)
        record["A"] = torch.softmax(xt @ xt.transpose(1, 2) / math.sqrt(nx * ny), -1).detach()
        record["h"] = h.detach()
        record["h_uniform"] = (xt.mean(1).view(B, nx, ny, 1) * p["fc0.weight"].detach().to(DT)[:, 0]
                               + p["fc0.bias"].detach().to(DT)).detach()
    if record is not None:      # the model's output had its attention matrix been uniform
        record["y_uniform"] = torch.cat([ref.fno2d(ref.sub_params(p, hd), record["h_uniform"]) for hd in heads],
                                        dim=-1).detach()
    return torch.cat([ref.fno2d(ref.sub_params(p, hd), h) for hd in heads], dim=-1)
