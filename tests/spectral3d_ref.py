"""Float64 numpy restatements of the 3D Fourier layer's entry points (csrc/spectral3d.hip), written
from the formulas of include/blindno.h (not from the kernels), with their rounding bounds and the
case tables of tests/test_gpu_spectral3d.py:

  colpass3d      blindno_colpass3d, dir 0 / 1   Xs = DFT_y,x(At) at the kept frequencies, Y the channel
                                                mix, Z = the two conjugate inverses of Y
  pack_w3d       blindno_pack_w3d               Wt[k3][jx K2 + jy][ci][co] = c_k3 / (P1 P2 P3) w_q[...]
  unpack_w3d     blindno_unpack_w3d             the adjoint: s dWt where corner q owns the frequency, else 0
  lift3d_fwd     blindno_lift3d_fwd             fc0 + permute + right pad of three axes
  lift3d_bwd     blindno_lift3d_bwd             d_in and [dW0 | db0]
  project3d_*    blindno_project3d_fwd / _bwd   projection_ref's references on the host-cropped field:
                                                the op is pointwise, so z[..., :N1, :N2, :N3] viewed as
                                                (Bn, C, N1 N2, N3) with a full crop is the same map

Every reference has an `*_abs` twin (moduli everywhere, |twiddle| = 1): the S_abs of the project's
bound  |got - ref| <= (n + c) 2^-24 S_abs,  n the number of accumulated terms along the chain (the
f32 matrix-core steps are exact f32 and add nothing beyond n) and c the single roundings outside
the accumulations, counted here rounding by rounding:

  colpass3d   Z:  n = P2 + P1 + cin + K1 + K2 (y DFT, x DFT, mix, x inverse, y inverse);
                  c = C_Z = 7: the four twiddle-table applications Ty, Tx, conj Tx, conj Ty (each
                  entry rounded once to fp32), the stored result, and two for the fused multiply-add /
                  summation-order differences.  The 2D column pass counts 8 with two tables and the
                  three roundings of its scale c_k / (P1 P2); here the scale is not applied by this
                  entry (it lives in Wt, tested at the pack), so two more tables and three fewer
                  scale roundings give 7.
              Y:  n = P2 + P1 + cin, c = C_XS = 5 (two tables, the result, two for order).
              Xs: n = P2 + P1,       c = C_XS.
  pack / unpack   3 2^-24 |value|: the reciprocal 1 / (P1 P2 P3), its product with c_k3 and the
                  application; the unpack's zeros are exact.
  lift3d_fwd      n = Cin + 1 (bias and Cin products), c = C_LIFT = 1: nothing is rounded outside the
                  chain; the one stands for the second-order term of (1 + u)^n - 1 over n u.  The pad
                  is exactly 0.
  lift3d_bwd      d_in: n = C.  [dW0 | db0], the device's per-workgroup rows summed in float64 on the
                  host: n = 256 x the largest number of tiles one workgroup visits (lift_chain).
                  c = C_LIFT.
  project3d       projection_ref's bounds (c = its C_EXTRA = 8, GELU term 5e-7 x weight).  Its
                  parameter sums use the number of crop points as the chain; project3d_bwd_bound
                  passes them this kernel's chain, 32 points x the tiles one workgroup visits.
                  dz off the crop is exactly 0 (the entry clears the field).

Inputs come from seeded numpy generators at O(1) amplitude, fp32-representable.

Case tables: each id names the path it is there for (DESIGN.md "3D Fourier layer launch paths").
They are the smallest shapes at which each path exists, with three remarks.  `workload_tiles` has 3 x 2 = 6 output
tiles in the y DFT and the x inverse and 3 x 3 = 9 in the y inverse, but its x DFT writes K1 x K2 =
24 x 24, 2 x 2 = 4 tiles: one per wave, no second trip.  `xs_second_trip` is added for that stage
(K1 = P1 = 34, K2 = P2 = 18: six tiles in every stage, every K = 2 mod 4).  `cout1_hd1_c32` has
np = Hd C + Hd + Cout Hd + Cout = 35 parameters (< 256: most threads own none).  The pack-only
`nyquist_m3` keeps every last-axis bin of an even P3 (m3 = P3/2 + 1): the only case whose scale
has c_k3 = 1 at the Nyquist bin.
"""
import numpy as np

import projection_ref as pr
from spectral_stage_ref import (GELU_ABS, SENT, U24, Guarded, _phase, c2r, cplx, gelu, gelu_grad,  # noqa: F401
                                kept_rows, ri, tile_decode, tile_layout, worst)

C_Z = 7                  # module docstring
C_XS = 5
C_LIFT = 1
PACK_ROUNDINGS = 3
LDS_LIMIT = 64 * 1024    # dynamic LDS a kernel of csrc/spectral3d.hip may ask for
LIFT_STRIDE = 257
LIFT_TILE = 256
PROJ_TILE = 32
MAX_CHUNKS = 1024


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _c64(rng, *shape, scale=1.0):
    """fp32-representable complex values as complex128."""
    return _f32(rng, *shape, scale=scale).astype(np.float64) + 1j * _f32(rng, *shape, scale=scale).astype(np.float64)


# ------------------------------------------------------------------------------- shape rules
def spectral3d_ok(Bn, Ci, Co, P, m):
    """The limits include/blindno.h states for blindno_spectral3d_ok."""
    (P1, P2, P3), (m1, m2, m3) = P, m
    if min(Bn, Ci, Co, P1, P2, P3, m1, m2, m3) <= 0 or Ci > 32 or Co > 32:
        return False
    if m1 > P1 or m2 > P2 or m3 > P3 // 2 + 1 or m3 > 48:
        return False
    K1, K2, Cm = min(2 * m1, P1), min(2 * m2, P2), max(Ci, Co)
    if colpass_lds_bytes(P, m) > LDS_LIMIT:
        return False
    big = 2 ** 31 - 1
    return (P1 * P2 < 2 ** 24 and K1 * K2 * Cm * Cm * m3 < big // 2 and Bn * m3 * Cm < big
            and Bn * P1 * P2 * m3 * Cm * 2 < big and Bn * Cm * P1 * P2 < big)


def colpass_lds_bytes(P, m):
    """The P1 x K2 complex plane both transform kernels keep in LDS."""
    return 8 * P[0] * min(2 * m[1], P[1])


def stage_tiles(P, m):
    """Output tiles (16 x 16, one wave each, four waves per workgroup) and accumulation length K
    of the four complex GEMMs: y DFT (P1 x K2 over P2), x DFT (K1 x K2 over P1), x inverse (P1 x K2
    over K1), y inverse (P1 x P2 over K2)."""
    (P1, P2, _), (m1, m2, _) = P, m
    K1, K2 = min(2 * m1, P1), min(2 * m2, P2)
    t = lambda a, b: -(-a // 16) * -(-b // 16)
    return {"dft_y": (t(P1, K2), P2), "dft_x": (t(K1, K2), P1), "idft_x": (t(P1, K2), K1), "idft_y": (t(P1, P2), K2)}


def lift3d_ok(Bn, N, P, Cin, C):
    return (min(Bn, *N, Cin, C) > 0 and Cin <= 32 and C <= 32 and all(p >= n for p, n in zip(P, N))
            and C * Cin + C <= 1024)


def lift_lds_bytes(Cin, C):
    return 4 * (C + Cin) * LIFT_STRIDE


def _chunks(npts, tile):
    tiles = -(-npts // tile)
    nchunk = max(1, min(tiles, MAX_CHUNKS))
    return tiles, nchunk


def lift_tiles(Bn, N):
    """(tiles of 256 points, workgroups = blindno_lift3d_bwd_nchunk)."""
    return _chunks(Bn * N[0] * N[1] * N[2], LIFT_TILE)


def lift_chain(Bn, N):
    tiles, nchunk = lift_tiles(Bn, N)
    return LIFT_TILE * -(-tiles // nchunk)


def project3d_ok(Bn, C, P, N, Hd, Cout):
    return (min(Bn, C, *N, Hd, Cout) > 0 and C <= 32 and all(p >= n for p, n in zip(P, N)) and Hd <= 128
            and Cout <= 8)


def project_tiles(Bn, N):
    """(tiles of 32 points, workgroups = blindno_project3d_bwd_nchunk)."""
    return _chunks(Bn * N[0] * N[1] * N[2], PROJ_TILE)


def project_chain(Bn, N):
    tiles, nchunk = project_tiles(Bn, N)
    return PROJ_TILE * -(-tiles // nchunk)


def project_lds_bytes(C, Hd, Cout):
    return 4 * (2 * Hd + C + Cout) * 33


# ------------------------------------------------------------------------------- colpass3d
def _axes(P, m):
    (P1, P2, _), (m1, m2, _) = P, m
    Fx = _phase(np.arange(P1), kept_rows(m1, P1), P1, -1.0)            # Fx[x][jx] = e^{-2 pi i r_jx x / P1}
    Fy = _phase(np.arange(P2), kept_rows(m2, P2), P2, -1.0)
    return Fx, Fy


def _mix(X, W, direction):
    if direction == 0:
        return np.einsum("nkiab,kabio->nkoab", X, W, optimize=True)
    return np.einsum("nkoab,kabio->nkiab", X, np.conj(W), optimize=True)


def colpass3d_all(At, Wt, P, m, direction):
    """At (Bn, m3, cin, P1, P2), Wt (m3, K1 K2, Ci, Co) -> (Xs (Bn, m3, cin, K1 K2), Y (Bn, m3, cout,
    K1 K2), Z (Bn, P1 P2, m3, cout))."""
    Fx, Fy = _axes(P, m)
    K1, K2 = Fx.shape[1], Fy.shape[1]
    Bn, m3, cin = At.shape[:3]
    X = np.einsum("nkcxy,yb,xa->nkcab", At, Fy, Fx, optimize=True)
    Y = _mix(X, Wt.reshape(m3, K1, K2, *Wt.shape[-2:]), direction)
    Z = np.einsum("nkcab,xa,yb->nxykc", Y, np.conj(Fx), np.conj(Fy), optimize=True)
    cout = Y.shape[2]
    return X.reshape(Bn, m3, cin, K1 * K2), Y.reshape(Bn, m3, cout, K1 * K2), Z.reshape(Bn, P[0] * P[1], m3, cout)


def colpass3d(At, Wt, P, m, direction):
    """(Xs, Z): Xs[b][c][jx K2 + jy] the y-then-x DFT at the kept frequencies, Z[n][x P2 + y][k3][c']
    after the mix (direction 1: conj(Wt) transposed) and the two conjugate inverses."""
    X, _, Z = colpass3d_all(At, Wt, P, m, direction)
    return X, Z


def colpass3d_all_abs(At, Wt, P, m, direction):
    """S_abs of (Xs, Y, Z)."""
    (P1, P2, _), (m1, m2, _) = P, m
    K1, K2 = min(2 * m1, P1), min(2 * m2, P2)
    Bn, m3, cin = At.shape[:3]
    X = np.broadcast_to(np.abs(At).sum((-2, -1))[..., None, None], (Bn, m3, cin, K1, K2))
    Y = _mix(X, np.abs(Wt).reshape(m3, K1, K2, *Wt.shape[-2:]), direction)
    cout = Y.shape[2]
    Z = np.broadcast_to(Y.sum((-2, -1))[:, None], (Bn, P1 * P2, m3, cout))
    return X.reshape(Bn, m3, cin, K1 * K2), Y.reshape(Bn, m3, cout, K1 * K2), Z


def colpass3d_abs(At, Wt, P, m, direction):
    X, _, Z = colpass3d_all_abs(At, Wt, P, m, direction)
    return X, Z


def colpass_chains(P, m, cin):
    """n of (Xs, Y, Z)."""
    (P1, P2, _), (m1, m2, _) = P, m
    K1, K2 = min(2 * m1, P1), min(2 * m2, P2)
    return P2 + P1, P2 + P1 + cin, P2 + P1 + cin + K1 + K2


def colpass3d_bounds(At, Wt, P, m, direction):
    """Per-element bounds of (Xs, Y, Z), each applied to the real and the imaginary part."""
    Xa, Ya, Za = colpass3d_all_abs(At, Wt, P, m, direction)
    nx, ny, nz = colpass_chains(P, m, At.shape[2])
    return (nx + C_XS) * U24 * Xa, (ny + C_XS) * U24 * Ya, (nz + C_Z) * U24 * Za


# ------------------------------------------------------------------------------- weight pack
def corner_owner(m, P):
    """(owner (K1, K2), ix (K1, K2), iy (K1, K2)): the last of weights1..4 (0..3: low/low, high/low,
    low/high, high/high in x/y) whose block contains kept frequency (r_jx, r_jy), and the index of
    that frequency inside the block."""
    (m1, m2, _), (P1, P2, _) = m, P
    r1, r2 = kept_rows(m1, P1)[:, None], kept_rows(m2, P2)[None, :]
    lo1, hi1, lo2, hi2 = r1 < m1, r1 >= P1 - m1, r2 < m2, r2 >= P2 - m2
    owner = np.full((r1.size, r2.size), -1)
    for q, inside in enumerate((lo1 & lo2, hi1 & lo2, lo1 & hi2, hi1 & hi2)):
        owner[inside] = q                                             # later corners overwrite earlier ones
    assert (owner >= 0).all()
    return owner, np.where(owner & 1, r1 - (P1 - m1), r1), np.where(owner & 2, r2 - (P2 - m2), r2)


def pack_scale(m, P):
    return c2r(m[2], P[2]) / (P[0] * P[1] * P[2])


def pack_w3d(ws, m, P):
    """ws: four (Ci, Co, m1, m2, m3) complex -> Wt (m3, K1 K2, Ci, Co)."""
    owner, ix, iy = corner_owner(m, P)
    w = np.stack(ws)                                                  # (4, Ci, Co, m1, m2, m3)
    Wt = w[owner, :, :, ix, iy, :]                                    # (K1, K2, Ci, Co, m3)
    Wt = Wt.transpose(4, 0, 1, 2, 3) * pack_scale(m, P)[:, None, None, None, None]
    return np.ascontiguousarray(Wt.reshape(m[2], -1, *w.shape[1:3]))


def unpack_w3d(dWt, m, P):
    """dWt (m3, K1 K2, Ci, Co) -> four (Ci, Co, m1, m2, m3): s_k3 dWt at the entries whose corner owns
    their frequency, exactly 0 at the others."""
    owner, ix, iy = corner_owner(m, P)
    K1, K2 = owner.shape
    Ci, Co = dWt.shape[-2:]
    g = (dWt.reshape(m[2], K1, K2, Ci, Co) * pack_scale(m, P)[:, None, None, None, None]).transpose(1, 2, 3, 4, 0)
    out = np.zeros((4, Ci, Co, m[0], m[1], m[2]), g.dtype)
    for jx in range(K1):
        for jy in range(K2):
            out[owner[jx, jy], :, :, ix[jx, jy], iy[jx, jy], :] = g[jx, jy]
    return list(out)


def losers(m, P):
    """mask[q] (m1, m2): the entries of weights(q+1) whose frequency a later corner owns."""
    owner, ix, iy = corner_owner(m, P)
    won = np.zeros((4, m[0], m[1]), bool)
    won[owner, ix, iy] = True
    return list(~won)


# ------------------------------------------------------------------------------- lift
def lift3d_fwd(inp, w0, b0, P):
    """inp (Bn, N1, N2, N3, Cin) -> x0 (Bn, C, P1, P2, P3), 0 on the right pad of the three axes."""
    inp, w0, b0 = (np.asarray(a, np.float64) for a in (inp, w0, b0))
    Bn, N1, N2, N3, _ = inp.shape
    x0 = np.zeros((Bn, w0.shape[0], *P))
    x0[:, :, :N1, :N2, :N3] = (inp @ w0.T + b0).transpose(0, 4, 1, 2, 3)
    return x0


def lift3d_fwd_abs(inp, w0, b0, P):
    return lift3d_fwd(np.abs(inp), np.abs(w0), np.abs(b0), P)


def lift3d_fwd_bound(inp, w0, b0, P):
    return (np.shape(inp)[-1] + 1 + C_LIFT) * U24 * lift3d_fwd_abs(inp, w0, b0, P)


def lift3d_bwd(dx0, inp, w0):
    """(d_in (Bn, N1, N2, N3, Cin), [dW0 (C Cin) | db0 (C)]); dx0 is read on the grid only."""
    dx0, inp, w0 = (np.asarray(a, np.float64) for a in (dx0, inp, w0))
    _, N1, N2, N3, _ = inp.shape
    d = dx0[:, :, :N1, :N2, :N3].transpose(0, 2, 3, 4, 1)              # (Bn, N1, N2, N3, C)
    return d @ w0, np.concatenate([np.einsum("nxyzc,nxyzi->ci", d, inp).ravel(), d.sum((0, 1, 2, 3))])


def lift3d_bwd_abs(dx0, inp, w0):
    return lift3d_bwd(np.abs(dx0), np.abs(inp), np.abs(w0))


def lift3d_bwd_bound(dx0, inp, w0):
    da, ga = lift3d_bwd_abs(dx0, inp, w0)
    Bn, N = np.shape(inp)[0], np.shape(inp)[1:4]
    return (np.shape(w0)[0] + C_LIFT) * U24 * da, (lift_chain(Bn, N) + C_LIFT) * U24 * ga


# ------------------------------------------------------------------------------- projection
def _view(z, N):
    """The crop of z (Bn, C, P1, P2, P3) as the 2D field (Bn, C, N1 N2, N3)."""
    z = np.asarray(z, np.float64)
    return np.ascontiguousarray(z[:, :, :N[0], :N[1], :N[2]]).reshape(z.shape[0], z.shape[1], N[0] * N[1], N[2])


def _args2d(z, N):
    return _view(z, N), N[0] * N[1], N[2]


def project3d_max_abs_h(z, w1, b1, N):
    zv, Ho, Wo = _args2d(z, N)
    return pr.max_abs_h(zv, w1, b1, Ho, Wo)


def project3d_fwd(z, w1, b1, w2, b2, N):
    """(Bn, N1, N2, N3, Cout)."""
    zv, Ho, Wo = _args2d(z, N)
    return pr.project_fwd(zv, w1, b1, w2, b2, Ho, Wo).reshape(zv.shape[0], *N, -1)


def project3d_fwd_abs(z, w1, b1, w2, b2, N):
    zv, Ho, Wo = _args2d(z, N)
    return pr.project_fwd_abs(zv, w1, b1, w2, b2, Ho, Wo).reshape(zv.shape[0], *N, -1)


def project3d_fwd_bound(z, w1, b1, w2, b2, N):
    zv, Ho, Wo = _args2d(z, N)
    return pr.project_fwd_bound(zv, w1, b1, w2, b2, Ho, Wo).reshape(zv.shape[0], *N, -1)


def _field(dzc, shape, N):
    """dz on the crop (Bn, C, N1 N2, N3) -> the whole field, 0 outside the crop."""
    dz = np.zeros(shape)
    dz[:, :, :N[0], :N[1], :N[2]] = dzc.reshape(shape[0], shape[1], *N)
    return dz


def project3d_bwd(z, w1, b1, w2, dout, N):
    """(dz (Bn, C, P1, P2, P3), 0 off the crop; [dW1 (Hd C) | db1 (Hd) | dW2 (Cout Hd) | db2 (Cout)])."""
    zv, Ho, Wo = _args2d(z, N)
    dzc, grads = pr.project_bwd(zv, w1, b1, w2, np.asarray(dout).reshape(zv.shape[0], Ho, Wo, -1), Ho, Wo)
    return _field(dzc, np.shape(z), N), grads


def project3d_bwd_abs(z, w1, b1, w2, dout, N):
    zv, Ho, Wo = _args2d(z, N)
    dzc, grads = pr.project_bwd_abs(zv, w1, b1, w2, np.asarray(dout).reshape(zv.shape[0], Ho, Wo, -1), Ho, Wo)
    return _field(dzc, np.shape(z), N), grads


def project3d_bwd_bound(z, w1, b1, w2, dout, N, chain=None):
    """The bounds of project3d_bwd's results: projection_ref's, the parameter sums with the
    accumulation length `chain` (default project_chain: 32 points x the tiles one workgroup visits;
    the rows of `partial` are added in float64 on the host) in place of the number of crop points."""
    zv, Ho, Wo = _args2d(z, N)
    if chain is None:
        chain = project_chain(zv.shape[0], N)
    dzc, grads = pr.project_bwd_bound(zv, w1, b1, w2, np.asarray(dout).reshape(zv.shape[0], Ho, Wo, -1), Ho, Wo,
                                      chain=chain)
    return _field(dzc, np.shape(z), N), grads


# ------------------------------------------------------------------------------- the GPU cases
# id -> (Bn, Ci, Co, (P1, P2, P3), (m1, m2, m3), (TILE at dir 0, TILE at dir 1))
COLPASS_CASES = {
    "tile_c8": (2, 8, 8, (6, 6, 8), (2, 2, 4), (1, 1)),                   # TILE both directions, 36 rows per sample
    "tile_c12_dir0_only": (1, 5, 12, (10, 6, 10), (3, 3, 2), (1, 0)),     # dir 0 TILE (cout 12), dir 1 plain (cout 5)
    "tile_c16_allkept": (3, 16, 16, (5, 4, 6), (3, 2, 2), (1, 1)),        # K1 = P1, K2 = P2: overlapping corners, odd P1
    "plain_odd_m3": (2, 8, 8, (6, 6, 8), (2, 2, 3), (0, 0)),              # width 8 but odd m3
    "plain_rows_mod4": (1, 8, 8, (7, 9, 6), (2, 3, 2), (0, 0)),           # 63 rows; every edge tile partial
    "workload_tiles": (1, 12, 12, (42, 42, 10), (12, 12, 4), (1, 1)),     # 6 / 4 / 6 / 9 tiles; K 42, 42, 24, 24
    "lds_limit": (1, 1, 1, (128, 64, 4), (1, 32, 1), (0, 0)),             # P1 K2 8 = 65 536 bytes exactly; m3 = 1
    "degenerate": (1, 2, 3, (1, 3, 4), (1, 1, 2), (0, 0)),                # P1 = K1 = 1
    "xs_second_trip": (1, 3, 2, (34, 18, 4), (17, 9, 2), (0, 0)),         # 6 tiles in every stage, every K = 2 mod 4
}
# the pack / unpack shapes: every colpass shape and the admitted channel maximum
PACK_CASES = {k: v[1:5] for k, v in COLPASS_CASES.items()}
PACK_CASES["c32_allkept"] = (32, 32, (5, 4, 6), (3, 2, 2))
PACK_CASES["nyquist_m3"] = (3, 2, (5, 4, 6), (3, 2, 4))                    # m3 = P3/2 + 1, even P3: c_k3 = 1 at k3 = 3

# id -> (Bn, (N1, N2, N3), (P1, P2, P3), Cin, C)
LIFT_CASES = {
    "small": (2, (6, 5, 7), (8, 7, 9), 4, 5),
    "nopad": (2, (4, 4, 4), (4, 4, 4), 3, 2),
    "np1023": (1, (3, 3, 30), (4, 5, 32), 32, 31),                        # accumulator slot q = 3, 64 764 bytes of LDS
    "np1024": (1, (3, 3, 30), (4, 5, 32), 31, 32),
    "stride_1045_tiles": (3, (45, 45, 44), (46, 46, 45), 2, 3),           # 1045 tiles on 1024 workgroups, last tile 36 points
    "one_point": (1, (1, 1, 1), (2, 2, 2), 1, 1),
}
LIFT_NULL_DIN = ("small", "stride_1045_tiles")                             # run again with d_in = NULL

# id -> (Bn, C, (P1, P2, P3), (N1, N2, N3), Hd, Cout)
PROJECT_CASES = {
    "base": (2, 5, (8, 7, 9), (6, 5, 7), 128, 2),
    "cout8_hd37": (1, 3, (5, 6, 7), (4, 5, 6), 37, 8),
    "cout1_hd1_c32": (2, 32, (4, 4, 9), (3, 3, 7), 1, 1),
    "hd128_c32_cout8": (1, 32, (5, 5, 5), (4, 4, 4), 128, 8),             # the largest LDS request
    "stride_1055_tiles": (1, 5, (35, 34, 33), (33, 33, 31), 128, 2),      # 1055 tiles, 31 workgroups take a second one
}


def _seed(table, cid, salt):
    return 31000 + 1000 * salt + list(table).index(cid)


def colpass_inputs(cid, direction):
    """(At (Bn, m3, cin, P1, P2), Wt (m3, K1 K2, Ci, Co)): complex128, fp32-representable.  Wt is an
    arbitrary packed operand (random, not the output of the pack)."""
    Bn, Ci, Co, P, m, _ = COLPASS_CASES[cid]
    rng = np.random.default_rng(_seed(COLPASS_CASES, cid, direction))
    cin = Co if direction else Ci
    K = min(2 * m[0], P[0]) * min(2 * m[1], P[1])
    return _c64(rng, Bn, m[2], cin, P[0], P[1]), _c64(rng, m[2], K, Ci, Co, scale=1.0 / np.sqrt(cin))


def pack_inputs(cid):
    """(ws: four (Ci, Co, m1, m2, m3), G (m3, K1 K2, Ci, Co)) complex128, fp32-representable."""
    Ci, Co, P, m = PACK_CASES[cid]
    rng = np.random.default_rng(_seed(PACK_CASES, cid, 2))
    K = min(2 * m[0], P[0]) * min(2 * m[1], P[1])
    return [_c64(rng, Ci, Co, *m) for _ in range(4)], _c64(rng, m[2], K, Ci, Co)


def lift_inputs(cid):
    Bn, N, P, Cin, C = LIFT_CASES[cid]
    rng = np.random.default_rng(_seed(LIFT_CASES, cid, 3))
    return {"in": _f32(rng, Bn, *N, Cin), "w0": _f32(rng, C, Cin, scale=1.0 / np.sqrt(Cin)), "b0": _f32(rng, C),
            "dx0": _f32(rng, Bn, C, *P)}


def project_inputs(cid):
    """z, w1, b1, w2, b2, dout in fp32, scaled as projection_ref.proj_inputs (|h| stays far below 12)."""
    Bn, C, P, N, Hd, Cout = PROJECT_CASES[cid]
    rng = np.random.default_rng(_seed(PROJECT_CASES, cid, 4))
    return {"z": _f32(rng, Bn, C, *P), "w1": _f32(rng, Hd, C, scale=0.6 / np.sqrt(C)), "b1": _f32(rng, Hd, scale=0.2),
            "w2": _f32(rng, Cout, Hd, scale=0.2), "b2": _f32(rng, Cout), "dout": _f32(rng, Bn, *N, Cout)}
