"""Inputs of the BagAttnMixFn tests (tests/test_gpu_bagattn_mix.py, checked without a GPU by
tests/test_trans_attn_ref.py).

With unstructured inputs the bag attention is near-uniform or near-identity and hides errors, so
the snapshot tokens are u_l = amp (a_l f + 0.02 eps) with f, eps ~ N(0, 1) fixed per sample and a_l
a shuffled linspace(0.05, 0.35, U).  ``amp`` is chosen per shape (the score of two tokens grows
with S) so that, on the float64 reference alone, replacing the attention matrix by the identity or
by the uniform matrix moves y by >= 100 x FWD_TOL and the mean row maximum of P over the snapshot
rows lies strictly between 2 / V and 0.9 (``hiding_figures``).
"""
import numpy as np
import torch

import trans_attn_ref as R

FWD_TOL = 1e-5          # tests/test_gpu_parity.py

_C75 = [1] * 30 + [2] * 14 + [3] * 3 + [4] * 2          # 49 distinct snapshots, 75 draws

# name: (B, U, S, width, counts, amp, seed)
CASES = {
    "workload": (2, 49, 3721, 12, _C75, 1.5, 1),        # the workload's ragged S
    "cap": (1, 254, 400, 4, None, 2.0, 2),              # V = 256, the cap
    "one_snapshot": (2, 1, 1089, 12, [3], 3.0, 3),      # one snapshot drawn three times
    "small_S": (2, 5, 37, 3, [1, 2, 1, 1, 3], 2.0, 4),  # S below one tile
    "S1": (1, 3, 1, 2, None, 12.0, 5),                   # S = 1
}


def make_case(name):
    """float64 CPU tensors: dict(u (B, U, S), grid (S, 2), W (width, 3), bias (width),
    dy (B, S, width), counts)."""
    B, U, S, width, counts, amp, seed = CASES[name]
    rs = np.random.RandomState(seed)
    f = rs.standard_normal((B, 1, S))
    eps = rs.standard_normal((B, U, S))
    a = np.linspace(0.05, 0.35, U)
    rs.shuffle(a)
    u = amp * (a[None, :, None] * f + 0.02 * eps)
    c = {"u": u, "grid": rs.uniform(-1, 1, (S, 2)), "W": rs.standard_normal((width, 3)),
         "bias": rs.standard_normal(width), "dy": rs.standard_normal((B, S, width))}
    c = {k: torch.from_numpy(v) for k, v in c.items()}
    c["counts"] = counts
    assert counts is None or (len(counts) == U and sum(counts) >= U)
    return c


def hiding_figures(c):
    """(identity move, uniform move, mean row max of P over the snapshot rows, V) in float64."""
    y, _ = R.literal(c["u"], c["grid"], c["W"], c["bias"], c["counts"])
    moves = []
    for mode in ("identity", "uniform"):
        ym, _ = R.literal(c["u"], c["grid"], c["W"], c["bias"], c["counts"], attn=mode)
        moves.append(float((ym - y).norm() / y.norm()))
    _, P, _ = R.reduced(c["u"], c["grid"], c["W"], c["bias"], c["counts"])
    return moves[0], moves[1], float(P[:, 2:].max(-1).values.mean()), P.shape[-1]


def assert_not_hidden(c):
    ident, unif, rowmax, V = hiding_figures(c)
    assert ident >= 100 * FWD_TOL, ident
    assert unif >= 100 * FWD_TOL, unif
    assert 2.0 / V < rowmax < 0.9, (rowmax, V)
