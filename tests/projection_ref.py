"""Float64 numpy restatements of the projection MLP (crop -> fc1 -> GELU -> fc2) and of the 2D
bag-level projection, written from the formulas of include/blindno.h and the header comment of
csrc/bagproj.h (not from the kernels):

  project_fwd    blindno_project_fwd(_g)       out[n,h,w,o] = b2_o + sum_k w2_ok GELU(b1_k + sum_c w1_kc z[n,c,h,w])
  project_bwd    blindno_project_bwd(_g / _w)  dz on the crop and [dW1 | db1 | dW2 | db2]; sample n reads
                                               dout[n // dout_div] * lscale[n % dout_div]
  bag_fwd        blindno_project_bag_fwd       ubar[b,p] = sum_l lw_l (w2 . GELU(h_l) + b2),  v = W1^T (w2 GELU'(h))
  bag_bwd        blindno_project_bag_bwd       dz = lw_l ghat v and the gradients from the statistics A, S, Q

Every stage has an `*_abs` twin, the same formula with every operand replaced by its modulus,
and a `*_bound` function, the per-element acceptance bound of the GPU tests.  The bound is derived,
not measured; u = 2^-24, GELU_ABS = 5e-7 (>= the 4.2e-7 / 3.2e-7 GELU / GELU' errors csrc/common.h
states for |h| <= 12), c = C_EXTRA = 8 single roundings outside an accumulation (the scalings of
W1 and b1, the dout * lscale product, folded weight products, the final scale and the result):

  habs_k  = |b1_k| + sum_c |w1_kc| |z_c|
  dh_k    = (C + 1 + c) u habs_k                         the rounding error of the pre-activation h_k
                                                         (the f32 matrix cores accumulate in exact f32 steps)
  forward |out_o - ref| <= sum_k |w2_ok| (GELU_ABS + 1.13 dh_k)
                           + (Hd + c) u (|b2_o| + sum_k |w2_ok| |GELU(h_k)|)
          1.13 >= sup |GELU'| (GELU' peaks at 1.129 near h = 1.41): an error dh of h moves GELU(h) by
          at most 1.13 dh.
  backward, with g_o the upstream gradient, da_k = sum_o w2_ok g_o and dH_k = da_k GELU'(h_k):
          e_k  = |da_k| (GELU_ABS + 0.8 dh_k)            the error of dH_k from the GELU' evaluation;
                                                         0.8 >= sup |GELU''| (GELU''(0) = 2 phi(0) = 0.798)
          dHa_k = (sum_o |w2_ok| |g_o|) |GELU'(h_k)|     the modulus twin of dH_k
          dz_c   <= sum_k |w1_kc| e_k + (Hd + c) u sum_k |w1_kc| dHa_k
          dW1_kc <= sum_p |z_pc| e_kp + (N + c) u sum_p |z_pc| dHa_kp      N = the number of crop points
          db1_k  <= sum_p e_kp + (N + c) u sum_p dHa_kp
          dW2_ok <= sum_p |g_op| (GELU_ABS + 1.13 dh_kp) + (N + c) u sum_p |g_op| |GELU(h_kp)|
          db2_o  <= (N + c) u sum_p |g_op|
  bag     the weighted sum over the U snapshots adds U terms to every accumulation length.  The modulus
          twin of GELU(h) is GELU(habs): GELU(h) = h (Phi(h) - 1/2) + h / 2 is a legitimate fp32
          evaluation order whose two parts have moduli summing to GELU(|h|) <= GELU(habs) (GELU increases
          on h >= 0), which |GELU(h)| alone would not cover for h < 0.  The twin of GELU' is its
          supremum 1.13.

Where a bound is 0 the error must be 0 (`worst`).  The GPU cases and their inputs live here too
(`MFMA_CASES`, ..., `proj_inputs`, `bag_inputs`): tests/test_projection_ref.py checks on the host
that a plain fp32 evaluation of the same formulas stays inside the bounds on exactly the inputs
the GPU tests use, and that max |h| <= 12 there.
"""
import numpy as np

from spectral_stage_ref import GELU_ABS, U24, Guarded, gelu, gelu_grad, worst  # noqa: F401 (re-exported)

C_EXTRA = 8
GP_SUP = 1.13            # >= sup |GELU'|
GPP_SUP = 0.8            # >= sup |GELU''|


def _f64(*a):
    return [None if x is None else np.asarray(x, np.float64) for x in a]


def crop(z, Ho, Wo):
    """z (Bn, C, P1, P2) -> the crop as points (Bn, Ho, Wo, C), float64."""
    return np.ascontiguousarray(np.asarray(z, np.float64)[:, :, :Ho, :Wo].transpose(0, 2, 3, 1))


def hidden(zc, w1, b1):
    return zc @ w1.T + b1


def _dh(zc, w1, b1):
    """(habs, dh): the modulus twin of h and the rounding error of h."""
    habs = np.abs(zc) @ np.abs(w1).T + np.abs(b1)
    return habs, (w1.shape[1] + 1 + C_EXTRA) * U24 * habs


def upstream(dout, Bn, dout_div=1, lscale=None):
    """dout (Bn / dout_div, Ho, Wo, Cout) -> the gradient sample n reads, (Bn, Ho, Wo, Cout)."""
    n = np.arange(Bn)
    g = np.asarray(dout, np.float64)[n // dout_div]
    if lscale is not None:
        g = g * np.asarray(lscale, np.float64)[n % dout_div][:, None, None, None]
    return g


# ------------------------------------------------------------------------------- projection
def project_fwd(z, w1, b1, w2, b2, Ho, Wo):
    """(Bn, Ho, Wo, Cout)."""
    z, w1, b1, w2, b2 = _f64(z, w1, b1, w2, b2)
    return gelu(hidden(crop(z, Ho, Wo), w1, b1)) @ w2.T + b2


def project_fwd_abs(z, w1, b1, w2, b2, Ho, Wo):
    return project_fwd(*[np.abs(a) for a in _f64(z, w1, b1, w2, b2)], Ho, Wo)


def project_fwd_bound(z, w1, b1, w2, b2, Ho, Wo):
    z, w1, b1, w2, b2 = _f64(z, w1, b1, w2, b2)
    zc = crop(z, Ho, Wo)
    _, dh = _dh(zc, w1, b1)
    a = np.abs(gelu(hidden(zc, w1, b1)))
    return (GELU_ABS + GP_SUP * dh) @ np.abs(w2).T + (w1.shape[0] + C_EXTRA) * U24 * (a @ np.abs(w2).T + np.abs(b2))


def max_abs_h(z, w1, b1, Ho, Wo):
    z, w1, b1 = _f64(z, w1, b1)
    return float(np.abs(hidden(crop(z, Ho, Wo), w1, b1)).max())


def project_bwd(z, w1, b1, w2, dout, Ho, Wo, dout_div=1, lscale=None):
    """(dz on the crop (Bn, C, Ho, Wo), [dW1 (Hd C) | db1 (Hd) | dW2 (Cout Hd) | db2 (Cout)])."""
    z, w1, b1, w2 = _f64(z, w1, b1, w2)
    zc = crop(z, Ho, Wo)
    h = hidden(zc, w1, b1)
    g = upstream(dout, z.shape[0], dout_div, lscale)
    dH = (g @ w2) * gelu_grad(h)
    dz = (dH @ w1).transpose(0, 3, 1, 2)
    grads = np.concatenate([np.einsum("nhwk,nhwc->kc", dH, zc).ravel(), dH.sum((0, 1, 2)),
                            np.einsum("nhwo,nhwk->ok", g, gelu(h)).ravel(), g.sum((0, 1, 2))])
    return dz, grads


def project_bwd_abs(z, w1, b1, w2, dout, Ho, Wo, dout_div=1, lscale=None):
    z, w1, b1, w2, dout, lscale = _f64(z, w1, b1, w2, dout, lscale)
    return project_bwd(np.abs(z), np.abs(w1), np.abs(b1), np.abs(w2), np.abs(dout), Ho, Wo, dout_div,
                       None if lscale is None else np.abs(lscale))


def project_bwd_bound(z, w1, b1, w2, dout, Ho, Wo, dout_div=1, lscale=None, chain=None):
    """The bounds of (dz, grads), shaped like project_bwd's results.  chain: the accumulation length of
    the parameter sums where it is not the number of crop points (partial rows added in float64)."""
    z, w1, b1, w2 = _f64(z, w1, b1, w2)
    zc = crop(z, Ho, Wo)
    h = hidden(zc, w1, b1)
    _, dh = _dh(zc, w1, b1)
    g = upstream(dout, z.shape[0], dout_div, lscale)
    e = np.abs(g @ w2) * (GELU_ABS + GPP_SUP * dh)
    dHa = (np.abs(g) @ np.abs(w2)) * np.abs(gelu_grad(h))
    Hd, N = w1.shape[0], zc.shape[0] * Ho * Wo
    dz = (e @ np.abs(w1) + (Hd + C_EXTRA) * U24 * (dHa @ np.abs(w1))).transpose(0, 3, 1, 2)
    nu = ((N if chain is None else chain) + C_EXTRA) * U24
    az, ag = np.abs(zc), np.abs(g)
    grads = np.concatenate([
        (np.einsum("nhwk,nhwc->kc", e, az) + nu * np.einsum("nhwk,nhwc->kc", dHa, az)).ravel(),
        e.sum((0, 1, 2)) + nu * dHa.sum((0, 1, 2)),
        (np.einsum("nhwo,nhwk->ok", ag, GELU_ABS + GP_SUP * dh) +
         nu * np.einsum("nhwo,nhwk->ok", ag, np.abs(gelu(h)))).ravel(),
        nu * ag.sum((0, 1, 2))])
    return dz, grads


# ------------------------------------------------------------------------------- bag-level projection
def _lw(lw, U):
    return np.full(U, 1.0 / U) if lw is None else np.asarray(lw, np.float64)


def _bag_points(z, U, Ho, Wo):
    zc = crop(z, Ho, Wo)
    return zc.reshape(zc.shape[0] // U, U, Ho * Wo, zc.shape[-1])          # (B, U, S, C)


def _bag_field(x, Ho, Wo):
    """(B, U, S, C) -> (B U, C, Ho, Wo)."""
    B, U, S, C = x.shape
    return np.ascontiguousarray(x.reshape(B * U, Ho, Wo, C).transpose(0, 3, 1, 2))


def bag_fwd(z, w1, b1, w2, b2, lw, U, Ho, Wo):
    """(ubar (B, Ho Wo), v on the crop (B U, C, Ho, Wo)); lw None: 1 / U."""
    z, w1, b1, w2, b2 = _f64(z, w1, b1, w2, b2)
    w2, lw = w2.reshape(-1), _lw(lw, U)
    h = hidden(_bag_points(z, U, Ho, Wo), w1, b1)
    ubar = np.einsum("l,blp->bp", lw, gelu(h) @ w2 + b2.reshape(()))
    return ubar, _bag_field((gelu_grad(h) * w2) @ w1, Ho, Wo)


def bag_fwd_abs(z, w1, b1, w2, b2, lw, U, Ho, Wo):
    """The twins: GELU(habs) for GELU, 1.13 for GELU' (module docstring)."""
    z, w1, b1, w2, b2 = [np.abs(a) for a in _f64(z, w1, b1, w2, b2)]
    w2, lw = w2.reshape(-1), np.abs(_lw(lw, U))
    zc = _bag_points(z, U, Ho, Wo)
    ubar = np.einsum("l,blp->bp", lw, gelu(hidden(zc, w1, b1)) @ w2 + b2.reshape(()))
    v = np.broadcast_to(GP_SUP * (w2 @ w1), zc.shape)
    return ubar, _bag_field(v, Ho, Wo)


def bag_fwd_bound(z, w1, b1, w2, b2, lw, U, Ho, Wo):
    z, w1, b1, w2, b2 = _f64(z, w1, b1, w2, b2)
    aw2, lwa, Hd = np.abs(w2.reshape(-1)), np.abs(_lw(lw, U)), w1.shape[0]
    _, dh = _dh(_bag_points(z, U, Ho, Wo), w1, b1)
    ua, va = bag_fwd_abs(z, w1, b1, w2, b2, lw, U, Ho, Wo)
    ubar = np.einsum("l,blp->bp", lwa, (GELU_ABS + GP_SUP * dh) @ aw2) + (U + Hd + C_EXTRA) * U24 * ua
    v = _bag_field((GELU_ABS + GPP_SUP * dh) @ (aw2[:, None] * np.abs(w1)), Ho, Wo) + (Hd + C_EXTRA) * U24 * va
    return ubar, v


def bag_bwd(z, w1, b1, w2, lw, U, ghat, Ho, Wo):
    """(dz = lw_l ghat v on the crop (B U, C, Ho, Wo), [dW1 | db1 | dW2 | db2]) from the bag-level
    statistics A = sum_l lw a, S = sum_l lw g, Q = sum_l lw g z^T."""
    z, w1, b1, w2, ghat = _f64(z, w1, b1, w2, ghat)
    w2, lw = w2.reshape(-1), _lw(lw, U)
    zc = _bag_points(z, U, Ho, Wo)
    h = hidden(zc, w1, b1)
    gp = gelu_grad(h)
    A = np.einsum("l,blpk->bpk", lw, gelu(h))
    S = np.einsum("l,blpk->bpk", lw, gp)
    Q = np.einsum("l,blpk,blpc->bpkc", lw, gp, zc)
    gh = ghat.reshape(ghat.shape[0], -1)
    v = (gp * w2) @ w1
    dz = lw[None, :, None, None] * gh[:, None, :, None] * v
    grads = np.concatenate([(w2[:, None] * np.einsum("bp,bpkc->kc", gh, Q)).ravel(),
                            w2 * np.einsum("bp,bpk->k", gh, S), np.einsum("bp,bpk->k", gh, A),
                            [gh.sum() * lw.sum()]])
    return _bag_field(dz, Ho, Wo), grads


def bag_bwd_abs(z, w1, b1, w2, lw, U, ghat, Ho, Wo):
    z, w1, b1, w2, ghat = [np.abs(a) for a in _f64(z, w1, b1, w2, ghat)]
    w2, lw = w2.reshape(-1), np.abs(_lw(lw, U))
    zc = _bag_points(z, U, Ho, Wo)
    gh = ghat.reshape(ghat.shape[0], -1)
    A = np.einsum("l,blpk->bpk", lw, gelu(hidden(zc, w1, b1)))
    zbar = np.einsum("l,blpc->bpc", lw, zc)
    gs = gh.sum() * lw.sum()
    dz = lw[None, :, None, None] * gh[:, None, :, None] * np.broadcast_to(GP_SUP * (w2 @ w1), zc.shape)
    grads = np.concatenate([(GP_SUP * w2[:, None] * np.einsum("bp,bpc->c", gh, zbar)[None, :]).ravel(),
                            GP_SUP * w2 * gs, np.einsum("bp,bpk->k", gh, A), [gs]])
    return _bag_field(dz, Ho, Wo), grads


def bag_bwd_bound(z, w1, b1, w2, lw, U, ghat, Ho, Wo):
    z, w1, b1, w2, ghat = _f64(z, w1, b1, w2, ghat)
    aw2, lwa, Hd = np.abs(w2.reshape(-1)), np.abs(_lw(lw, U)), w1.shape[0]
    zc = _bag_points(z, U, Ho, Wo)
    _, dh = _dh(zc, w1, b1)
    gh = np.abs(ghat.reshape(ghat.shape[0], -1))
    dza, ga = bag_bwd_abs(z, w1, b1, w2, lw, U, ghat, Ho, Wo)
    wgt = lwa[None, :, None] * gh[:, None, :]                                  # |lw_l ghat| (B, U, S)
    e1 = GELU_ABS + GPP_SUP * dh                                               # GELU' evaluations
    dz = _bag_field(wgt[..., None] * (e1 @ (aw2[:, None] * np.abs(w1))), Ho, Wo) + (Hd + C_EXTRA) * U24 * dza
    nu = (U + gh.size + C_EXTRA) * U24
    grads = np.concatenate([
        (aw2[:, None] * np.einsum("blp,blpk,blpc->kc", wgt, e1, np.abs(zc))).ravel(),
        aw2 * np.einsum("blp,blpk->k", wgt, e1),
        np.einsum("blp,blpk->k", wgt, GELU_ABS + GP_SUP * dh), [0.0]]) + nu * ga
    return dz, grads


# ------------------------------------------------------------------------------- the GPU cases
# crop geometries of the matrix-core path: name -> (Bn, (P1, P2), (Ho, Wo), (ostride, ooff) or None
# for ostride = Cout, ooff = 0)
GEOMS = {
    "t16_9tiles": (3, (5, 19), (3, 16), (5, 2)),      # Wo % 16 == 0: T16; 9 tiles, the last step has a dead tile
    "row4": (3, (6, 14), (5, 12), (5, 2)),            # not T16, Wo % 4 == 0: row4 true
    "ragged": (3, (6, 14), (5, 11), (5, 2)),          # row4 false; points straddle rows and samples; 165 = 10 * 16 + 5
    "head1d": (3, (1, 40), (1, 37), (5, 2)),          # the 1D heads: Ho = P1 = 1
    "nocrop": (2, (4, 16), (4, 16), None),            # Ho == P1, Wo == P2 (T16), plain output addressing
}
CHANNELS = [1, 3, 4, 5, 8, 9, 12, 13, 15]             # CK 4: 1 3 4; CK 8: 5 8; CK 12: 9 12; CK 16: 13 15


def ck_of(C):
    return (C + 3) // 4 * 4


def proj_inputs(C, Cout, Bn, P, N, Hd=128, dout_div=1, seed=0):
    """fp32 inputs of one projection case (numpy): z, w1, b1, w2, b2, dout, lscale."""
    rng = np.random.default_rng(7000 + 131 * C + 17 * Cout + 5 * Bn + 3 * N[1] + N[0] + Hd + seed)
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)
    return {"z": f(Bn, C, *P), "w1": f(Hd, C, scale=0.6 / np.sqrt(C)), "b1": f(Hd, scale=0.2),
            "w2": f(Cout, Hd, scale=0.2), "b2": f(Cout), "dout": f(Bn // dout_div, *N, Cout),
            "lscale": (rng.integers(1, 5, dout_div) / 7.0).astype(np.float32)}


# the 2D bag projection: (B, U, C, (P1, P2), (Ho, Wo)); the first four are the original square cases
BAG_CASES = [
    (2, 1, 4, (40, 40), (30, 30)), (3, 37, 4, (40, 40), (30, 30)), (2, 300, 4, (24, 24), (18, 18)),
    (2, 19, 3, (40, 40), (30, 30)),
    (2, 5, 4, (20, 36), (13, 29)), (2, 5, 2, (33, 12), (30, 7)),           # rectangular
    (3, 9, 1, (12, 12), (9, 9)),                                           # C = 1
    (2, 8, 4, (12, 12), (7, 7)), (2, 9, 4, (12, 12), (7, 7)),              # the 8-snapshot chunk edges
    (2, 16, 4, (12, 12), (7, 7)), (2, 17, 4, (12, 12), (7, 7)),
    (1, 1024, 2, (6, 6), (4, 4)),                                          # four staging rounds of the weights
]


def bag_id(case):
    B, U, C, P, N = case
    return f"B{B}_U{U}_C{C}_P{P[0]}x{P[1]}_N{N[0]}x{N[1]}"


def bag_inputs(case, weighted):
    B, U, C, P, N = case
    rng = np.random.default_rng(9000 + 7 * U + C + P[1] + 2 * int(weighted))
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)
    t = {"z": f(B * U, C, *P), "w1": f(128, C, scale=0.4), "b1": f(128, scale=0.1), "w2": f(1, 128, scale=0.1),
         "b2": f(1), "gs": f(B, N[0] * N[1]), "lw": None}
    if weighted:
        counts = rng.integers(1, 4, U).astype(np.float32)
        t["lw"] = (counts / counts.sum()).astype(np.float32)          # multiplicity / L
    return t


def _case(cid, C, Cout, Bn, P, N, Hd=128, dout_div=1, addr=None, kinds=("fwd", "bwd")):
    return {"id": cid, "C": C, "Cout": Cout, "Bn": Bn, "P": P, "N": N, "Hd": Hd, "dout_div": dout_div,
            "addr": addr or (Cout, 0), "kinds": kinds}


def case_inputs(c, seed=0):
    return proj_inputs(c["C"], c["Cout"], c["Bn"], c["P"], c["N"], c["Hd"], c["dout_div"], seed)


# project_{fwd,bwd}_mfma_kernel<CK, COM, NP, T16>: every channel class x Cout x crop geometry
MFMA_CASES = [_case(f"{g}_c{C}_o{Co}_ck{ck_of(C)}_com{Co}_{'t16' if N[1] % 16 == 0 else 'pt'}", C, Co, Bn, P, N,
                    addr=addr)
              for g, (Bn, P, N, addr) in GEOMS.items() for C in CHANNELS for Co in (1, 2)]
# dout_div = 3 broadcast (Bn = 6), T16 and not: blindno_project_bwd and blindno_project_bwd_w (lscale)
BCAST_CASES = [_case(f"div3_{g}_c{C}_o{Co}", C, Co, 6, GEOMS[g][1], GEOMS[g][2], dout_div=3, addr=(5, 2),
                     kinds=("bwd",))
               for g in ("t16_9tiles", "ragged") for C in (4, 12) for Co in (1, 2)]
# one weight group of the grouped launches (G = 2; group g: seed g): gpts = 64 = 16 NP for NP 2 / 4
GROUP_CASES = [_case(f"g2_c{C}_np{2 if C == 12 else 4}_o{Co}_{tag}", C, Co, 2, P, N)
               for C in (12, 4) for Co in (1, 2)
               for tag, P, N in (("pt", (6, 18), (4, 8)), ("t16", (3, 18), (2, 16)))]
# project_fwd_kernel<CM, COM> (fields.hip): C > 15, Cout in {3, 4} or Hd != 128
FALLBACK_FWD_CASES = [_case(f"fwd_c{C}_o{Co}_hd{Hd}_cm{cm}_com{1 if Co == 1 else 4}", C, Co, 3, (6, 14), (5, 11),
                            Hd=Hd, addr=(5, 1), kinds=("fwd",))
                      for C, Co, Hd, cm in ((16, 1, 128, 16), (16, 3, 128, 16), (20, 1, 128, 32), (20, 3, 128, 32),
                                            (32, 1, 128, 32), (32, 3, 128, 32), (4, 4, 128, 4), (4, 1, 64, 4),
                                            (6, 3, 128, 8), (8, 1, 64, 8))]
# project_bwd_wsum_kernel<CM, 8, COM> (Hd = 128): <8, 8, 1> needs C <= 8, Cout = 1 off the matrix cores,
# i.e. a field of >= 2^31 elements, and is not covered
FALLBACK_BWD_CASES = [_case(f"bwd_c{C}_o{Co}_div{dv}_cm{cm}_jw8_com{1 if Co == 1 else 4}", C, Co, 4, (6, 14), (5, 11),
                            dout_div=dv, addr=(5, 1), kinds=("bwd",))
                      for C, Co, cm in ((16, 1, 16), (32, 3, 32), (6, 3, 8), (16, 3, 16), (20, 1, 32))
                      for dv in (1, 2)]
# the forward's grid cap: 9 * 256 * 256 / 16 tiles / (4 waves * 2) = 4608 -> 2048 workgroups, stride loop
GRIDCAP_CASE = _case("gridcap_c4_o1_blocks2048", 4, 1, 9, (258, 258), (256, 256), kinds=("fwd",))
ALL_CASES = MFMA_CASES + BCAST_CASES + GROUP_CASES + FALLBACK_FWD_CASES + FALLBACK_BWD_CASES
