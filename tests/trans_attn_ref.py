"""Restatement, in plain torch (float64 as the checker), of the bag token attention of
NIOFP2D_Trans_attn (2d_FPE/NIOModules.py:241-278) on a deduplicated bag, in two forms, and of the
whole model on top of tests/transolver_ref.py.  Written from the formulas of
include/blindno_bagattn_mix.h for tests/test_trans_attn_ref.py, tests/test_gpu_bagattn_mix.py and
tests/test_gpu_trans_attn.py.

A bag of L draws has U distinct snapshots u (B, U, S) with counts nu (sum L).

  literal              the reference's own sequence on the L + 2 materialised tokens (index_select
                       from the distinct snapshots, matmul, softmax, matmul, the fusion matrix)
  reduced, reduced_bwd the formulas the kernels implement: V = U + 2 distinct tokens with masses
                       [1, 1, nu], forward and hand-written backward
  niofp2d_trans_attn   the whole model: Transolver per distinct snapshot, literal attention, heads
"""
import math

import numpy as np
import torch

import oracle.fno_ref as ref
import transolver_ref as tr


def _counts(counts, U):
    c = [1] * U if counts is None else [int(n) for n in counts]
    assert len(c) == U and min(c) >= 1
    return c


def expand_index(counts, U):
    """Bag positions -> distinct snapshot: snapshot v repeated counts[v] times."""
    return torch.as_tensor(np.repeat(np.arange(U), _counts(counts, U)))


def literal(u, grid, W, bias, counts=None, attn=None):
    """u (B, U, S), grid (S, 2), W (width, 3), bias (width) -> (y (B, S, width), A (B, T, T)) by
    the reference's sequence on the T = L + 2 materialised tokens.  ``attn`` replaces the attention
    matrix: "identity" or "uniform" (the tests' proof that the attention matters)."""
    B, U, S = u.shape
    x = u.index_select(1, expand_index(counts, U))
    L = x.shape[1]
    x_flat = torch.cat((grid.t().unsqueeze(0).expand(B, 2, S), x), dim=1)        # (B, T, S)
    T = L + 2
    scores = torch.matmul(x_flat, x_flat.transpose(1, 2)) / math.sqrt(S)
    A = torch.softmax(scores, dim=-1)
    if attn == "identity":
        A = torch.eye(T, dtype=u.dtype).expand(B, T, T)
    elif attn == "uniform":
        A = torch.full((B, T, T), 1.0 / T, dtype=u.dtype)
    else:
        assert attn is None
    Z = torch.matmul(A, x_flat)
    Wn = torch.cat([W[:, :2], W[:, 2].view(-1, 1).repeat(1, L) / L], dim=1)      # (width, T)
    return torch.matmul(Z.permute(0, 2, 1), Wn.t()) + bias, A


def _reduced_parts(u, grid, counts):
    B, U, S = u.shape
    c = _counts(counts, U)
    L = sum(c)
    mass = torch.tensor([1, 1] + c, dtype=u.dtype)
    X = torch.cat((grid.t().unsqueeze(0).expand(B, 2, S), u), dim=1)             # (B, V, S)
    G = torch.matmul(X, X.transpose(1, 2)) / math.sqrt(S)
    E = mass * torch.exp(G - G.max(dim=-1, keepdim=True).values)
    P = E / E.sum(dim=-1, keepdim=True)
    lw = mass[2:] / L                                                             # nu / L
    r = torch.stack((P[:, 0], P[:, 1], (lw.view(1, U, 1) * P[:, 2:]).sum(1)), dim=1)   # (B, 3, V)
    return X, P, r, lw


def reduced(u, grid, W, bias, counts=None):
    """The same function on the V = U + 2 distinct tokens: (y, P (B, V, V), r (B, 3, V))."""
    X, P, r, _ = _reduced_parts(u, grid, counts)
    m = torch.matmul(r, X)                                                        # (B, 3, S)
    return torch.matmul(m.transpose(1, 2), W.t()) + bias, P, r


def reduced_bwd(u, grid, W, dy, counts=None):
    """(du (B, U, S), dgrid (S, 2)) from dy (B, S, width), by the hand-written backward."""
    S = u.shape[2]
    X, P, r, lw = _reduced_parts(u, grid, counts)
    dm = torch.matmul(dy, W).transpose(1, 2)                                      # (B, 3, S)
    dr = torch.matmul(dm, X.transpose(1, 2))                                      # (B, 3, V)
    dP = torch.cat((dr[:, 0:1], dr[:, 1:2], lw.view(1, -1, 1) * dr[:, 2:3]), dim=1)
    dG = P * (dP - (P * dP).sum(-1, keepdim=True))
    M = (dG + dG.transpose(1, 2)) / math.sqrt(S)
    dX = torch.matmul(r.transpose(1, 2), dm) + torch.matmul(M, X)
    return dX[:, 2:], dX[:, :2].sum(0).t()


def dedup(idx):
    """(distinct indices, counts) of a bag draw, in np.unique's order."""
    uniq, counts = np.unique(np.asarray(idx), return_counts=True)
    return uniq.tolist(), counts.tolist()


def niofp2d_trans_attn(p, x, grid, idx=None, heads=("fno_drift", "fno_diffusion"), attn=None,
                       record=None):
    """NIOFP2D_Trans_attn.forward in float64 (``idx`` replaces the train-mode draw; None = eval):
    the Transolver on the distinct snapshots, the literal attention on the L + 2 tokens taken from
    them by index_select, the two FNO heads.  ``record`` receives the attention matrix."""
    dt = ref.DT
    x = x.to(dt)
    counts = None
    if idx is not None:
        uniq, counts = dedup(idx)
        x = x[:, uniq]
    B, U, nx, ny = x.shape
    g = grid.to(dt)
    gp = g.permute(2, 0, 1).reshape(1, 2, nx * ny).expand(B * U, 2, nx * ny)
    inp = torch.cat((x.reshape(B * U, 1, nx * ny), gp), 1)                        # [rho, gx, gy]
    tp = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in ref.sub_params(p, "trans_input").items()}
    u = tr.transolver(tp, inp, nx, ny).reshape(B, U, nx * ny)
    w0, b0 = p["fc0.weight"].detach().to(dt), p["fc0.bias"].detach().to(dt)
    h, A = literal(u, g.reshape(nx * ny, 2), w0, b0, counts, attn)
    if record is not None:
        record.append(A.detach())
    h = h.view(B, nx, ny, -1)
    return torch.cat([ref.fno2d(ref.sub_params(p, hd), h) for hd in heads], dim=-1)
