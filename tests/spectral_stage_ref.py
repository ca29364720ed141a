"""Float64 numpy restatements of the 2D / 1D spectral stages declared in include/blindno.h, one
function per stage, written from the header's formulas (not from the kernels):

  row_dft        blindno_rowdft(_crop)          At[n,k,c,h] = sum_w f(x[n,c,h,w]) e^{-2 pi i k w / P2}
  col_pass       blindno_colpass(_g), dir 0 / 1 (Xs, Z) at the kept rows r_j
  mix1d          blindno_mix1d, dir 0 / 1
  row_inv        blindno_rowidft_epi(_g)        z = sum_k Re(Z e^{+2 pi i k w / P2}) + Wc f(x) + bc
  row_inv_adj    blindno_rowidft_bwd(_crop/_g)  dx = (sum_k Re(G e^{+...}) + Wc^T dz) GELU'(xsrc)
  conv_wgrad     the in-pass dWc | dbc sums of blindno_rowidft_bwd (C <= 4)
  tile_encode / tile_decode                     blindno_spectrum_tile_layout's A-tile order of Z

Complex tensors are numpy complex128 here; `cplx` / `ri` convert from / to the interleaved
(re, im) float pairs of the ABI.  Every stage has an `*_abs` twin: the same formula with every
operand replaced by its modulus (|twiddle| = 1), the per-element magnitude S_abs of the
rounding-error bound  |got - ref| <= (n + c) 2^-24 S_abs  of a length-n fp32 accumulation.  Where
GELU / GELU' is evaluated on load the twin also returns the summed weight of the GELU-evaluated
operands (for the 5e-7 absolute term of csrc/common.h's measured GELU error).

`Guarded` and `worst` are the sentinel-margin output buffer and the err / bound ratio of
test_gpu_finalise.py (copied: test modules do not import each other).
"""
import math

import numpy as np

U24 = 2.0 ** -24
GELU_ABS = 5e-7          # >= the 4.2e-7 (GELU) / 3.2e-7 (GELU') measured in csrc/common.h, |z| <= 12
SENT = -12345.678        # the sentinel (random data never takes this value)
MARGIN = 64              # sentinel floats on both sides of every output


# ------------------------------------------------------------------------------- helpers
def cplx(a):
    """(..., 2) interleaved float pairs -> complex128."""
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def ri(z):
    """complex -> (..., 2) float64 pairs."""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], -1)


def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    x = np.asarray(x, np.float64)
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def kept_rows(m1, P1):
    """K1 = min(2 m1, P1) kept rows; row j -> frequency r_j = j (j < m1 or K1 == P1), else
    P1 - 2 m1 + j."""
    K1 = min(2 * m1, P1)
    return np.array([j if (K1 == P1 or j < m1) else P1 - 2 * m1 + j for j in range(K1)], np.int64)


def c2r(m, P):
    """c_k: bin 0 and the Nyquist bin of an even P count once, every other bin twice."""
    c = np.full(m, 2.0)
    c[0] = 1.0
    if P % 2 == 0 and m > P // 2:
        c[P // 2] = 1.0
    return c


def _phase(a, b, P, sign):
    """e^{sign 2 pi i a_i b_j / P} with exact integer phases."""
    ph = (np.outer(a, b) % P).astype(np.float64) * (2.0 * math.pi / P)
    return np.cos(ph) + sign * 1j * np.sin(ph)


def pack_w2d(w1, w2, P1):
    """Reference-layout complex weights (Ci, Co, m1, m2) x 2 -> Wt[k][j][ci][co] (m2, K1, Ci, Co):
    kept row j uses weights1[:, :, r_j] for r_j < P1 - m1 and weights2[:, :, r_j - (P1 - m1)]
    otherwise (weights2 wins on overlap)."""
    m1 = w1.shape[2]
    cols = []
    for r in kept_rows(m1, P1):
        cols.append(w2[:, :, r - (P1 - m1), :] if r >= P1 - m1 else w1[:, :, r, :])
    return np.ascontiguousarray(np.stack(cols, 0).transpose(3, 0, 1, 2))      # (K1,Ci,Co,m2) -> (m2,K1,Ci,Co)


def pack_w1d(w):
    """(Ci, Co, m) complex -> Wt[k][ci][co]."""
    return np.ascontiguousarray(w.transpose(2, 0, 1))


# ------------------------------------------------------------------------------- row DFT
def _valid(x, valid):
    """x with everything outside h < N1v, w < N2v replaced by zero (never read)."""
    if valid is None:
        return np.asarray(x, np.float64)
    v = np.zeros(x.shape, np.float64)
    v[..., :valid[0], :valid[1]] = x[..., :valid[0], :valid[1]]
    return v


def row_dft(x, m2, act=0, valid=None):
    """x (Bn, C, P1, P2) -> At (Bn, m2, C, P1) complex."""
    P2 = x.shape[-1]
    xv = _valid(x, valid)
    f = _valid(gelu(xv), valid) if act else xv
    return np.einsum("nchw,wk->nkch", f, _phase(np.arange(P2), np.arange(m2), P2, -1.0))


def row_dft_abs(x, m2, act=0, valid=None):
    """(S_abs, gelu weight), each (Bn, 1, C, P1): sum_w |f(x)| and the number of operands read."""
    xv = _valid(x, valid)
    f = np.abs(_valid(gelu(xv), valid) if act else xv)
    cnt = _valid(np.ones(x.shape), valid).sum(-1) if act else np.zeros(x.shape[:-1])
    return f.sum(-1)[:, None], cnt[:, None]


# ------------------------------------------------------------------------------- column pass
def col_pass(At, Wt, P1, P2, m1, direction):
    """At (Bn, m2, cin, P1), Wt (m2, K1, Ci, Co) [or (Bn, m2, K1, Ci, Co): per-sample weights of a
    grouped launch] -> (Xs (Bn, m2, cin, K1), Z (Bn, P1, m2, cout)).
    dir 0: Xs = colDFT(At);  Z = c_k/(P1 P2) colIDFT(sum_i Xs W).
    dir 1: Xs = c_k/(P1 P2) colDFT(At);  Z = colIDFT(sum_o conj(W) Xs)."""
    m2 = At.shape[1]
    F = _phase(np.arange(P1), kept_rows(m1, P1), P1, -1.0)            # F[h][j] = e^{-2 pi i r_j h / P1}
    sc = (c2r(m2, P2) / (P1 * P2))[None, :, None, None]
    W = Wt if Wt.ndim == 5 else Wt[None]
    X = np.einsum("nkch,hj->nkcj", At, F, optimize=True)
    if direction == 0:
        Y = np.einsum("nkij,nkjio->nkoj", X, np.broadcast_to(W, (At.shape[0],) + W.shape[1:])) * sc
    else:
        X = X * sc
        Y = np.einsum("nkoj,nkjio->nkij", X, np.broadcast_to(np.conj(W), (At.shape[0],) + W.shape[1:]))
    Z = np.einsum("nkcj,hj->nhkc", Y, np.conj(F), optimize=True)
    return X, Z


def col_pass_abs(At, Wt, P1, P2, m1, direction):
    """S_abs of (Xs, Z): moduli everywhere, |F| = 1."""
    m2 = At.shape[1]
    K1 = len(kept_rows(m1, P1))
    sc = (c2r(m2, P2) / (P1 * P2))[None, :, None, None]
    W = np.abs(Wt if Wt.ndim == 5 else Wt[None])
    W = np.broadcast_to(W, (At.shape[0],) + W.shape[1:])
    X = np.repeat(np.abs(At).sum(-1, keepdims=True), K1, -1)
    if direction == 0:
        Y = np.einsum("nkij,nkjio->nkoj", X, W) * sc
    else:
        X = X * sc
        Y = np.einsum("nkoj,nkjio->nkij", X, W)
    Z = np.repeat(Y.sum(-1)[:, None], P1, 1)                           # (Bn, P1, m2, cout)
    return X, Z


# ------------------------------------------------------------------------------- 1D mix
def mix1d(At, Wt, P2, direction):
    """At (Bn, m, cin), Wt (m, Ci, Co) -> (Xs (Bn, m, cin), Z (Bn, m, cout)).
    dir 0: Xs = At with the DC bin halved;  Z = c_k/P2 sum_i Xs W  (the Nyquist bin of an even P2
    is not doubled).  dir 1: Xs = c_k/P2 At;  Z = h_k sum_o conj(W) Xs, h_0 = 0.5, h_k = 1."""
    m = At.shape[1]
    half = np.ones(m)
    half[0] = 0.5
    sc = (c2r(m, P2) / P2)[None, :, None]
    if direction == 0:
        X = At * half[None, :, None]
        return X, np.einsum("nki,kio->nko", X, Wt) * sc
    X = At * sc
    return X, np.einsum("nko,kio->nki", X, np.conj(Wt)) * half[None, :, None]


def mix1d_abs(At, Wt, P2, direction):
    return mix1d(np.abs(At), np.abs(Wt), P2, direction)


# ------------------------------------------------------------------------------- row inverse
def _crop(dz, crop):
    return _valid(dz, crop)


def row_inv_bare(Z, P2):
    """Z (Bn, P1, m2, C) complex -> sum_k Re(Z e^{+2 pi i k w / P2}) as (Bn, C, P1, P2)."""
    m2 = Z.shape[2]
    return np.real(np.einsum("nhkc,kw->nchw", Z, _phase(np.arange(m2), np.arange(P2), P2, +1.0)))


def row_inv_bare_abs(Z, P2):
    return np.repeat(np.abs(Z).sum(2).transpose(0, 2, 1)[..., None], P2, -1)


def row_inv(Z, P2, x=None, wc=None, bc=None, act=0, bare=None):
    """z = sum_k Re(Z e^{+...}) + sum_i Wc[o,i] f(x_i) + bc[o]; wc None drops the conv / bias term.
    wc (C, C) or (Bn, C, C) / bc (C) or (Bn, C): per-sample weights of a grouped launch.
    bare: row_inv_bare(Z, P2) when the caller already has it (here and below)."""
    z = row_inv_bare(Z, P2) if bare is None else bare
    if wc is not None:
        f = gelu(x) if act else np.asarray(x, np.float64)
        w = np.broadcast_to(wc, (z.shape[0],) + wc.shape[-2:])
        b = np.broadcast_to(bc, (z.shape[0],) + bc.shape[-1:])
        z = z + np.einsum("noi,nihw->nohw", w, f) + b[:, :, None, None]
    return z


def row_inv_abs(Z, P2, x=None, wc=None, bc=None, act=0, bare=None):
    """(S_abs, gelu weight sum_i |Wc[o,i]|); bare: row_inv_bare_abs(Z, P2)."""
    s = row_inv_bare_abs(Z, P2) if bare is None else bare
    gw = np.zeros_like(s)
    if wc is not None:
        f = np.abs(gelu(x) if act else np.asarray(x, np.float64))
        w = np.abs(np.broadcast_to(wc, (s.shape[0],) + wc.shape[-2:]))
        b = np.abs(np.broadcast_to(bc, (s.shape[0],) + bc.shape[-1:]))
        s = s + np.einsum("noi,nihw->nohw", w, f) + b[:, :, None, None]
        if act:
            gw = gw + w.sum(-1)[:, :, None, None]
    return s, gw


def row_inv_adj(G, P2, dz=None, wc=None, xsrc=None, act=0, crop=None, bare=None):
    """dx = sum_k Re(G e^{+...}) + sum_o Wc[o,i] dz_o, times GELU'(xsrc) when act; dz counts as
    zero outside h < dN1, w < dN2 (crop); wc None: the bare transform."""
    dx = row_inv_bare(G, P2) if bare is None else bare
    if wc is not None:
        w = np.broadcast_to(wc, (dx.shape[0],) + wc.shape[-2:])
        dx = dx + np.einsum("noi,nohw->nihw", w, _crop(dz, crop))
        if act:
            dx = dx * gelu_grad(xsrc)
    return dx


def row_inv_adj_abs(G, P2, dz=None, wc=None, xsrc=None, act=0, crop=None, bare=None):
    """(S_abs, gelu weight): with act the GELU-evaluated operand is GELU'(xsrc), weighted by the
    modulus sum it multiplies."""
    s = row_inv_bare_abs(G, P2) if bare is None else bare
    gw = np.zeros_like(s)
    if wc is not None:
        w = np.abs(np.broadcast_to(wc, (s.shape[0],) + wc.shape[-2:]))
        s = s + np.einsum("noi,nohw->nihw", w, np.abs(_crop(dz, crop)))
        if act:
            gw = s
            s = s * np.abs(gelu_grad(xsrc))
    return s, gw


def conv_wgrad(dz, xsrc, act=0, crop=None):
    """[dWc[o][i] = sum dz_o f(xsrc_i) | dbc[o] = sum dz_o] (C*C + C), sums over every point."""
    d = _crop(dz, crop)
    f = gelu(xsrc) if act else np.asarray(xsrc, np.float64)
    return np.concatenate([np.einsum("nohw,nihw->oi", d, f).ravel(), d.sum((0, 2, 3))])


def conv_wgrad_abs(dz, xsrc, act=0, crop=None):
    """(S_abs, gelu weight sum |dz_o| for the dWc entries, 0 for dbc)."""
    d = np.abs(_crop(dz, crop))
    C = d.shape[1]
    f = np.abs(gelu(xsrc) if act else np.asarray(xsrc, np.float64))
    s = np.concatenate([np.einsum("nohw,nihw->oi", d, f).ravel(), d.sum((0, 2, 3))])
    gw = np.concatenate([np.repeat(d.sum((0, 2, 3)), C) if act else np.zeros(C * C), np.zeros(C)])
    return s, gw


# ------------------------------------------------------------------------------- A-tile layout
def _tile_index(nrows, m2, C):
    """Index arrays of Zt[((q C/4 + g) m2/2 + s) 64 + l] = Re (kk even) / Im (kk odd) of
    Z[row 4q + (l&15)/4][kk/2][4g + (l&3)], kk = 4s + l/16."""
    assert nrows % 4 == 0 and C % 4 == 0 and m2 % 2 == 0
    q, g, s, l = np.indices((nrows // 4, C // 4, m2 // 2, 64))
    kk = 4 * s + l // 16
    return 4 * q + (l & 15) // 4, kk // 2, 4 * g + (l & 3), kk & 1


def tile_encode(Zr):
    """Z as (Bn, P1, m2, C, 2) float pairs (rows n P1 + h) -> flat Zt in A-tile order."""
    Bn, P1, m2, C, _ = Zr.shape
    row, k, c, part = _tile_index(Bn * P1, m2, C)
    return np.ascontiguousarray(Zr.reshape(Bn * P1, m2, C, 2)[row, k, c, part]).ravel()


def tile_decode(Zt, Bn, P1, m2, C):
    """Flat Zt -> (Bn, P1, m2, C, 2)."""
    row, k, c, part = _tile_index(Bn * P1, m2, C)
    Zr = np.full((Bn * P1, m2, C, 2), np.nan, np.asarray(Zt).dtype)
    Zr[row, k, c, part] = np.asarray(Zt).reshape(row.shape)
    return Zr.reshape(Bn, P1, m2, C, 2)


def tile_layout(Bn, C, P1, P2, m2):
    """The header's rule for blindno_spectrum_tile_layout."""
    return int(C in (8, 12, 16) and m2 > 0 and m2 % 2 == 0 and m2 // 2 <= (24 if C == 8 else 16)
               and P1 % 4 == 0 and P1 >= 16 and Bn * C * P1 * P2 < 2 ** 31 - 1
               and Bn * P1 * m2 * C * 2 < 2 ** 31 - 1)


# ------------------------------------------------------------------------------- buffers / ratio
class Guarded:
    """n elements between two sentinel margins, all sentinel-filled (device tensor)."""

    def __init__(self, n, dtype=None):
        import torch
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * MARGIN,), SENT, device="cuda", dtype=dtype or torch.float32)
        self.t = self.buf[MARGIN:MARGIN + self.n]

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == SENT).all() and (self.buf[MARGIN + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def cpu(self):
        return self.t.cpu()


def worst(err, bound):
    """max err / bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
