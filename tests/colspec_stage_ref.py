"""Float64 numpy restatements of the folded column pass (csrc/colspec.h, csrc/colspec.hip and the
ZY / CD modes behind the *_zc entries of csrc/rowinv.hip), one function per operation, written
from the entries' definitions in include/blindno.h and the layout comments of colspec.h -- not
from the kernels' arithmetic:

  spectrum          blindno_rowdft_cd + blindno_colmix(Wt NULL)   X[n,k,c,j] = sum_{h<N1v, w<N2v}
                                                     f(x[n,c,h,w]) e^{-2 pi i (k w / P2 + r_j h / P1)}
  bag_fields        the zero-padded snapshots X[b][idx[l]] (n = b L + l); spectrum of them: Usave
  grid_planes       gx, gy and the ones plane on the crop; their spectrum: Dg2, row_dft: Dg
  lift_spectrum     Xs[c] = w0[c,0] U + w0[c,1] Dg2[0] + w0[c,2] Dg2[1] + b0[c] Dg2[2]
  mix               blindno_colmix dir 0 / 1: (Xsave, Y)
  z_from_y          Z[n,h,k,c] = sum_j Y[n,k,c,j] e^{+2 pi i r_j h / P1}, then the row-inverse
                    references of spectral_stage_ref (row_inv, row_inv_adj, conv_wgrad)
  lift_field        x0 = pad(fc0(u, gx, gy))
  bwd_lift_rows     [dWc | dbc | dW0 (C x 3) | db0] of blindno_rowidft_bwd_lift(_zc)
  bag_lift_at       At of blindno_rowdft_bag_lift(_dg), blindno_rowdft's layout

Complex tensors are complex128.  Each reference has an `*_abs` twin: the same formula with every
operand replaced by its modulus (|twiddle| = 1), the S_abs of the per-element bound
|got - ref| <= (n + c) 2^-24 S_abs; where GELU / GELU' is evaluated on load the twin also returns
the summed weight of the GELU-evaluated operands (spectral_stage_ref's convention).  The kept rows
are the K1 = 24 of m1 = 12 (the only ones the folded pass has).
"""
import numpy as np

import spectral_stage_ref as sr
from spectral_stage_ref import (GELU_ABS, U24, Guarded, _phase, cplx, kept_rows, ri, row_inv_adj,  # noqa: F401
                                row_inv_adj_abs, row_inv_bare_abs, worst)

M1 = 12
K1 = 24
GELU_LIP = 1.13          # >= max |GELU'| = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 1.1290


def col_phase(P1):
    """F[h][j] = e^{-2 pi i r_j h / P1} at the K1 kept rows."""
    assert len(kept_rows(M1, P1)) == K1
    return _phase(np.arange(P1), kept_rows(M1, P1), P1, -1.0)


# ------------------------------------------------------------------------------- spectra
def spectrum(x, m2, act=0, valid=None):
    """x (Bn, C, P1, P2) -> X (Bn, m2, C, K1): the 2D spectrum of f(x) on the valid region."""
    return np.einsum("nkch,hj->nkcj", sr.row_dft(x, m2, act, valid), col_phase(x.shape[2]), optimize=True)


def spectrum_abs(x, m2, act=0, valid=None):
    """(S_abs, gelu weight), each (Bn, 1, C, 1): sum |f(x)| over the region / operands read."""
    S, cnt = sr.row_dft_abs(x, m2, act, valid)                 # (Bn, 1, C, P1)
    return S.sum(-1, keepdims=True), cnt.sum(-1, keepdims=True)


def bag_fields(X, idx, P1, P2):
    """X (B, T, N1, N2), idx (L) -> u (B L, 1, P1, P2), zero past N1 x N2."""
    B, T, N1, N2 = X.shape
    u = np.zeros((B, len(idx), 1, P1, P2))
    u[:, :, 0, :N1, :N2] = np.asarray(X, np.float64)[:, np.asarray(idx)]
    return u.reshape(B * len(idx), 1, P1, P2)


def grid_planes(grid, P1, P2):
    """grid (N1, N2, 2) -> (1, 3, P1, P2): gx, gy and 1 on the crop, zero on the padding."""
    N1, N2, _ = grid.shape
    g = np.zeros((1, 3, P1, P2))
    g[0, 0, :N1, :N2] = grid[..., 0]
    g[0, 1, :N1, :N2] = grid[..., 1]
    g[0, 2, :N1, :N2] = 1.0
    return g


def lift_spectrum(U, Dg2, w0, b0):
    """U (Bn, m2, K1), Dg2 (m2, 3, K1), w0 (C, 3), b0 (C) -> Xs (Bn, m2, C, K1)."""
    A = np.concatenate([np.asarray(w0, np.float64)[:, 1:], np.asarray(b0, np.float64)[:, None]], 1)   # (C, 3)
    return np.einsum("c,nkj->nkcj", np.asarray(w0, np.float64)[:, 0], U) + np.einsum("cp,kpj->kcj", A, Dg2)[None]


def lift_spectrum_abs(SU, Dg2, w0, b0):
    """SU: S_abs of U, one value per sample."""
    SU = np.asarray(SU, np.float64).reshape(-1, 1, 1)
    return lift_spectrum(np.broadcast_to(SU, (SU.shape[0], Dg2.shape[0], Dg2.shape[2])), np.abs(Dg2),
                         np.abs(w0), np.abs(b0))


def mix(X, Wt, P1, P2, direction):
    """X (Bn, m2, cin, K1), Wt (m2, K1, C, C) -> (Xsave, Y).
    dir 0: Xsave = X, Y[n,k,o,j] = c_k/(P1 P2) sum_c X[n,k,c,j] Wt[k,j,c,o];
    dir 1: Xsave = G = c_k/(P1 P2) X, Y[n,k,c,j] = sum_o conj(Wt[k,j,c,o]) G[n,k,o,j]."""
    sc = (sr.c2r(X.shape[1], P2) / (P1 * P2))[None, :, None, None]
    if direction == 0:
        return X, np.einsum("nkcj,kjco->nkoj", X, Wt) * sc
    G = X * sc
    return G, np.einsum("nkoj,kjco->nkcj", G, np.conj(Wt))


def mix_abs(SX, Wt, P1, P2, direction):
    return mix(np.asarray(SX, np.float64), np.abs(Wt), P1, P2, direction)


# ------------------------------------------------------------------------------- row inverses
def z_from_y(Y, P1):
    """Y (Bn, m2, C, K1) -> Z (Bn, P1, m2, C)."""
    return np.einsum("nkcj,hj->nhkc", Y, np.conj(col_phase(P1)), optimize=True)


def z_from_y_abs(Y, P1):
    return np.repeat(np.abs(Y).sum(-1)[:, None], P1, 1)


def lift_field(X, idx, grid, w0, b0, P1, P2):
    """x0 (B L, C, P1, P2) = fc0(u, gx, gy) on the N1 x N2 crop, zero on the padding."""
    u, g = bag_fields(X, idx, P1, P2), grid_planes(grid, P1, P2)
    w0, b0 = np.asarray(w0, np.float64), np.asarray(b0, np.float64)
    return (w0[None, :, 0, None, None] * u + np.einsum("cp,phw->chw", w0[:, 1:], g[0, :2])[None]
            + b0[None, :, None, None] * g[:, 2:3])


def lift_field_abs(X, idx, grid, w0, b0, P1, P2):
    return lift_field(np.abs(X), idx, np.abs(grid), np.abs(w0), np.abs(b0), P1, P2)


def lift_inputs(X, idx, grid, P1, P2):
    """in = (u, gx, gy, 1) on the crop: (B L, 4, P1, P2)."""
    u, g = bag_fields(X, idx, P1, P2), grid_planes(grid, P1, P2)
    return np.concatenate([u, np.broadcast_to(g, (u.shape[0],) + g.shape[1:])], 1)


def bwd_lift_rows(Z, P2, dz, wc, X, idx, grid, w0, b0):
    """[dWc[o][i] = sum dz_o x0_i | dbc[o] = sum dz_o | dW0[c][j] = sum_crop dx0_c (u, gx, gy)_j |
    db0[c] = sum_crop dx0_c], dx0 = irow^H(Z) + Wc^T dz (no activation)."""
    P1 = Z.shape[1]
    x0 = lift_field(X, idx, grid, w0, b0, P1, P2)
    dx0 = row_inv_adj(Z, P2, dz, wc, None, 0)
    M = np.einsum("nchw,njhw->cj", dx0, lift_inputs(X, idx, grid, P1, P2))
    d = np.asarray(dz, np.float64)
    return np.concatenate([np.einsum("nohw,nihw->oi", d, x0).ravel(), d.sum((0, 2, 3)), M[:, :3].ravel(), M[:, 3]])


def bwd_lift_rows_abs(Zabs, P2, dz, wc, X, idx, grid, w0, b0):
    P1 = Zabs.shape[1]
    x0 = lift_field_abs(X, idx, grid, w0, b0, P1, P2)
    s, _ = row_inv_adj_abs(None, P2, dz, wc, None, 0, bare=row_inv_bare_abs(Zabs, P2))
    M = np.einsum("nchw,njhw->cj", s, np.abs(lift_inputs(X, idx, grid, P1, P2)))
    d = np.abs(dz)
    return np.concatenate([np.einsum("nohw,nihw->oi", d, x0).ravel(), d.sum((0, 2, 3)), M[:, :3].ravel(), M[:, 3]])


# ------------------------------------------------------------------------------- unfolded lift
def bag_lift_at(X, idx, w0, m2, P1, P2, Gt=None, b0=None, Dg=None):
    """At[n,k,c,h] = w0[c,0] rowDFT(u)[n,k,h] + Gt[k,c,h]; Gt given, or formed from Dg (m2, 3, P1)
    as w0[c,1] Dg[.,0] + w0[c,2] Dg[.,1] + b0[c] Dg[.,2]."""
    Ur = sr.row_dft(bag_fields(X, idx, P1, P2), m2)[:, :, 0]          # (Bn, m2, P1)
    w0 = np.asarray(w0, np.float64)
    if Gt is None:
        A = np.concatenate([w0[:, 1:], np.asarray(b0, np.float64)[:, None]], 1)
        Gt = np.einsum("cp,kph->kch", A, Dg)
    return np.einsum("c,nkh->nkch", w0[:, 0], Ur) + Gt[None]


def bag_lift_at_abs(X, idx, w0, m2, P1, P2, Gt=None, b0=None, Dg=None):
    Su = np.abs(bag_fields(X, idx, P1, P2)).sum(-1)                   # (Bn, 1, P1) per row
    Su = np.broadcast_to(Su, (Su.shape[0], m2, P1))
    w0 = np.abs(w0)
    if Gt is None:
        A = np.concatenate([w0[:, 1:], np.abs(b0)[:, None]], 1)
        Gt = np.einsum("cp,kph->kch", A, np.abs(Dg))
    return np.einsum("c,nkh->nkch", w0[:, 0], Su) + np.abs(Gt)[None]
