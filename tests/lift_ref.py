"""Float64 numpy restatements of the lift (fc0 + permute + pad), its adjoint and the 1x1-conv
weight gradient, written from the formulas of include/blindno.h and the header comments of
csrc/fields.hip, csrc/liftw.h and csrc/wgrad.h (not from the kernel bodies):

  lift_fwd      blindno_lift_fwd(_g / _bag_g)   x0[g Bg + n, c, h, w] = b_g[c] + sum_j W_g[c, j] in[n, h, w, j]
                                                on h < N1, w < N2, exactly 0 on the padding
  bag_h         the bag-mean input              h[p, j] = bb[j] + bw[j, 0] gx + bw[j, 1] gy + bw[j, 2] invL ubar[p]
  lift_bwd_in   blindno_lift_bwd(_g / _mix_g)   d_in[n, h, w, j] = sum_g sum_c W_g[c, j] dx0[g Bg + n, c, h, w]
  bag_dubar     the bag adjoint                 d_ubar[p] = invLb sum_j bw[j, 2] d_h[p, j]   (invLb, not invL)
  lift_bwd_w    the partial sums, reduced       [dW0[c, j] = sum_p dx0[c, p] in[p, j] | db0[c] = sum_p dx0[c, p]]
                                                per group over the N1 x N2 crop
  conv_wgrad_g  blindno_conv_wgrad(_g)          [dWc[o, i] = sum_p dz[o, p] f(x)[i, p] | dbc[o]] per group
  mix_wgrad     the hosted spectral gradient    dWt[g][k, j, i, o] = sum_n conj(X[n, k, i, j]) G[n, k, o, j]

Every stage has an `*_abs` twin, the same formula with every operand replaced by its modulus,
and a `*_bound` function, the per-element acceptance bound of the GPU tests.  The bounds are
derived, not measured; u = 2^-24, c = C_EXTRA = 8 single roundings outside an accumulation (a
rounded product ahead of an fma, the final rounding, the slack between gamma_n and n u),
GELU_ABS = 5e-7 the absolute GELU error csrc/common.h states for |x| <= 12:

  a sum of n fp32 products, in any order      |got - ref| <= (n + c) u S_abs
  lift forward      n = Cin + 1 (the bias is one term).  With the bag input the operand h carries
                    its own error dh[p, j] = (3 + c) u habs[p, j] (habs = the twin of h), which the
                    lift passes on as sum_j |W[c, j]| dh[p, j].
  input gradient    n = G C.  The bag adjoint sums Cin more terms of an operand d_h that is itself
                    off by (G C + c) u of its twin: (G C + Cin + 2 c) u  invLb sum_j |bw[j, 2]| dha[p, j].
  weight gradients  n = the number of crop points of one group, Bg N1 N2 (conv: Bg P1 P2), whatever
                    the split into workgroup partials (a split only shortens the chains).  The bag
                    input adds sum_p |dx0[c, p]| dh[p, j] to dW0; the conv's GELU adds
                    GELU_ABS sum_p |dz[o, p]| to dWc.
  hosted mix        the kernel accumulates in float64, so a slice's sum is one fp32 rounding of an
                    (almost) exact value; s non-empty slices are then added in fp32:
                    (s + c) u S_abs with s = min(mnsplit, Bg).

Where a bound is 0 (the padding, a weight column that meets no input) the error must be 0
(`worst`).  The GPU cases and their seeded inputs live here too: tests/test_lift_ref.py checks on
the host that a plain fp32 evaluation of the same formulas, in sequential and in pairwise order,
stays inside every bound on exactly the inputs the GPU tests use.

Each case id ends in the kernel instantiation the dispatcher selects, restated here from
blindno_lift_fwd_bag_g, blindno_lift_bwd_bag_mix_g and blindno_conv_wgrad_g (`fwd_path`,
`bwd_path`, `conv_path`; DESIGN.md "Lift and conv weight-gradient launch paths" has the table).
"""
import numpy as np

import spectral_stage_ref as ssr
from spectral_stage_ref import GELU_ABS, U24, Guarded, worst  # noqa: F401 (re-exported)

C_EXTRA = 8
K_LIFT_MAX_G, K_LIFT_MAX_C = 4, 16        # liftw.h
TP = 256                                  # points per tile of the nchunk rule
NCHUNK_CAP = 1024


def _f64(*a):
    return [None if x is None else np.asarray(x, np.float64) for x in a]


# ------------------------------------------------------------------------------- lift forward
def lift_fwd(inp, w0, b0, N, P, G):
    """inp (Bg, N1, N2, Cin), w0 (G, C, Cin), b0 (G, C) -> x0 (G Bg, C, P1, P2)."""
    inp, w0, b0 = _f64(inp, w0, b0)
    Bg, C = inp.shape[0], w0.shape[1]
    x0 = np.zeros((G * Bg, C, *P))
    for g in range(G):
        x0[g * Bg:(g + 1) * Bg, :, :N[0], :N[1]] = (np.einsum("nhwj,cj->nchw", inp, w0[g])
                                                    + b0[g][None, :, None, None])
    return x0


def lift_fwd_abs(inp, w0, b0, N, P, G):
    return lift_fwd(*[np.abs(a) for a in _f64(inp, w0, b0)], N, P, G)


def lift_fwd_bound(inp, w0, b0, N, P, G, dh=None):
    """dh: the per-element error of inp (the bag input), or None."""
    Cin = np.shape(w0)[2]
    b = (Cin + 1 + C_EXTRA) * U24 * lift_fwd_abs(inp, w0, b0, N, P, G)
    if dh is not None:
        b = b + lift_fwd(dh, np.abs(np.asarray(w0, np.float64)), np.zeros(np.shape(b0)), N, P, G)
    return b


# ------------------------------------------------------------------------------- bag input
def bag_h(ubar, grid, bw, bb, invL, N):
    """ubar (B, N1 N2), grid (N1 N2, 2), bw (Cin, 3), bb (Cin) -> h (B, N1, N2, Cin)."""
    ubar, grid, bw, bb = _f64(ubar, grid, bw, bb)
    h = (bb[None, None, :] + grid[None, :, 0, None] * bw[None, None, :, 0]
         + grid[None, :, 1, None] * bw[None, None, :, 1]
         + (ubar * float(invL))[:, :, None] * bw[None, None, :, 2])
    return h.reshape(ubar.shape[0], N[0], N[1], bw.shape[0])


def bag_h_abs(ubar, grid, bw, bb, invL, N):
    return bag_h(*[np.abs(a) for a in _f64(ubar, grid, bw, bb)], abs(float(invL)), N)


def bag_h_bound(ubar, grid, bw, bb, invL, N):
    return (3 + C_EXTRA) * U24 * bag_h_abs(ubar, grid, bw, bb, invL, N)


# ------------------------------------------------------------------------------- input gradient
def lift_bwd_in(dx0, w0, N, G):
    """dx0 (G Bg, C, P1, P2), w0 (G, C, Cin) -> d_in (Bg, N1, N2, Cin)."""
    dx0, w0 = _f64(dx0, w0)
    Bg = dx0.shape[0] // G
    d = dx0[:, :, :N[0], :N[1]].reshape(G, Bg, dx0.shape[1], N[0], N[1])
    return np.einsum("gnchw,gcj->nhwj", d, w0)


def lift_bwd_in_abs(dx0, w0, N, G):
    return lift_bwd_in(*[np.abs(a) for a in _f64(dx0, w0)], N, G)


def lift_bwd_in_bound(dx0, w0, N, G):
    C = np.shape(w0)[1]
    return (G * C + C_EXTRA) * U24 * lift_bwd_in_abs(dx0, w0, N, G)


def bag_dubar(d_h, bw, invLb):
    """d_h (B, N1, N2, Cin) -> d_ubar (B, N1 N2)."""
    d_h, bw = _f64(d_h, bw)
    return float(invLb) * (d_h @ bw[:, 2]).reshape(d_h.shape[0], -1)


def bag_dubar_abs(dx0, w0, N, G, bw, invLb):
    return bag_dubar(lift_bwd_in_abs(dx0, w0, N, G), np.abs(np.asarray(bw, np.float64)), abs(float(invLb)))


def bag_dubar_bound(dx0, w0, N, G, bw, invLb):
    C, Cin = np.shape(w0)[1:]
    return (G * C + Cin + 2 * C_EXTRA) * U24 * bag_dubar_abs(dx0, w0, N, G, bw, invLb)


# ------------------------------------------------------------------------------- weight gradients
def lift_bwd_w(dx0, inp, N, G):
    """dx0 (G Bg, C, P1, P2), inp (Bg, N1, N2, Cin) -> (G, C Cin + C): [dW0 | db0] per group."""
    dx0, inp = _f64(dx0, inp)
    Bg = dx0.shape[0] // G
    d = dx0[:, :, :N[0], :N[1]].reshape(G, Bg, dx0.shape[1], N[0], N[1])
    dw = np.einsum("gnchw,nhwj->gcj", d, inp, optimize=True)
    return np.concatenate([dw.reshape(G, -1), d.sum((1, 3, 4))], 1)


def lift_bwd_w_abs(dx0, inp, N, G):
    return lift_bwd_w(*[np.abs(a) for a in _f64(dx0, inp)], N, G)


def lift_bwd_w_bound(dx0, inp, N, G, dh=None):
    Bg = np.shape(inp)[0]
    b = (Bg * N[0] * N[1] + C_EXTRA) * U24 * lift_bwd_w_abs(dx0, inp, N, G)
    if dh is not None:
        e = lift_bwd_w(np.abs(np.asarray(dx0, np.float64)), dh, N, G)
        e[:, np.shape(dx0)[1] * np.shape(inp)[3]:] = 0.0          # db0 does not read the input
        b = b + e
    return b


def conv_wgrad_g(dz, x, act, G):
    """dz, x (G Bg, C, P1, P2) -> (G, C C + C) per group (spectral_stage_ref.conv_wgrad)."""
    Bg = np.shape(dz)[0] // G
    return np.stack([ssr.conv_wgrad(dz[g * Bg:(g + 1) * Bg], x[g * Bg:(g + 1) * Bg], act) for g in range(G)])


def conv_wgrad_g_abs(dz, x, act, G):
    """(S_abs, gelu weight), each (G, C C + C)."""
    Bg = np.shape(dz)[0] // G
    r = [ssr.conv_wgrad_abs(dz[g * Bg:(g + 1) * Bg], x[g * Bg:(g + 1) * Bg], act) for g in range(G)]
    return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


def conv_wgrad_g_bound(dz, x, act, G):
    n = np.shape(dz)[0] // G * np.shape(dz)[2] * np.shape(dz)[3]
    s, gw = conv_wgrad_g_abs(dz, x, act, G)
    return (n + C_EXTRA) * U24 * s + GELU_ABS * gw


# ------------------------------------------------------------------------------- hosted mix gradient
def mix_wgrad(Xs, Gs, G):
    """Xs (G Bg, m2, Ci, K1) complex, Gs (G Bg, m2, Co, K1) complex -> dWt (G, m2, K1, Ci, Co)."""
    Bg = Xs.shape[0] // G
    X = Xs.reshape(G, Bg, *Xs.shape[1:])
    Y = Gs.reshape(G, Bg, *Gs.shape[1:])
    return np.einsum("gnkij,gnkoj->gkjio", np.conj(X), Y, optimize=True)


def mix_wgrad_abs(Xs, Gs, G):
    """The twin of either component: sum_n (|Re X| + |Im X|)(|Re G| + |Im G|) covers both."""
    a = np.abs(Xs.real) + np.abs(Xs.imag)
    b = np.abs(Gs.real) + np.abs(Gs.imag)
    return mix_wgrad(a.astype(np.complex128), b.astype(np.complex128), G).real


def mix_wgrad_bound(Xs, Gs, G, mnsplit):
    s = min(int(mnsplit), Xs.shape[0] // G)
    return (s + C_EXTRA) * U24 * mix_wgrad_abs(Xs, Gs, G)


# ------------------------------------------------------------------------------- the dispatch rules
def lift_bwd_nchunk(Bg, N):
    return min(-(-Bg * N[0] * N[1] // TP), NCHUNK_CAP)


def conv_wgrad_nchunk(Bg, P):
    return min(Bg * -(-P[0] * P[1] // TP), NCHUNK_CAP)


def fwd_path(c):
    """blindno_lift_fwd_bag_g: the kernel a valid forward case runs."""
    wide = c["Cin"] == 12 and 4 < c["C"] <= K_LIFT_MAX_C and c["G"] <= K_LIFT_MAX_G
    if wide and (c["bag"] or not c["mis_in"]):
        return "wide12x16"
    return "pt16" if 4 < c["C"] <= 16 else "generic"


def bwd_path(c):
    """blindno_lift_bwd_bag_mix_g: both1 = lift_bwd_both_kernel<1>; otherwise the launches in
    order (in_wide / in_generic, then mfma1 / mfma2 / lds)."""
    Cin, C, G = c["Cin"], c["C"], c["G"]
    wide_in = (c["want_in"] and Cin == 12 and C <= K_LIFT_MAX_C and G <= K_LIFT_MAX_G
               and (c["bag"] or not c["mis_din"]))
    mf = 5 <= C <= 16 and Cin + 1 <= 32 and c["N"][1] % 16 == 0 and c["P"][1] % 4 == 0 and not c["mis_dx0"]
    if wide_in and c["want_w"] and mf:
        return "both1" if Cin + 1 <= 16 else "both2"      # both2 is unreachable: Cin == 12
    parts = []
    if c["want_in"]:
        parts.append("in_wide" if wide_in else "in_generic")
    if c["want_w"]:
        parts.append(("mfma1" if Cin + 1 <= 16 else "mfma2") if mf else "lds")
    return "+".join(parts)


def conv_path(c):
    """blindno_conv_wgrad_g: conv_wgrad_mfma_ok(C, HW) = 5 <= C <= 15."""
    if 5 <= c["C"] <= 15:
        return f"mfma_act{c['act']}_" + ("vec" if c["P"][0] * c["P"][1] % 4 == 0 else "scalar")
    return f"lds_act{c['act']}"


# ------------------------------------------------------------------------------- the GPU cases
DEF_N, DEF_P, DEF_BG = (5, 16), (7, 20), 3


def _lcase(tag, Cin, C, G=1, N=DEF_N, P=DEF_P, Bg=DEF_BG, bag=None, mis_in=False, mis_din=False,
           mis_dx0=False, want_in=True, want_w=True, mix=None, identity=False, reduce=False):
    """bag: None or (invL, invLb); mix: None or (K1, m2, mnsplit) with mnsplit 0 = the library's
    blindno_mix_wgrad_nsplit(Bg, ...); reduce: also through blindno_reduce_partials."""
    return {"tag": tag, "Cin": Cin, "C": C, "G": G, "N": N, "P": P, "Bg": Bg, "bag": bag, "mis_in": mis_in,
            "mis_din": mis_din, "mis_dx0": mis_dx0, "want_in": want_in, "want_w": want_w, "mix": mix,
            "identity": identity, "reduce": reduce}


def fwd_id(c):
    return f"{c['tag']}_{fwd_path(c)}"


def bwd_id(c):
    return f"{c['tag']}_{bwd_path(c)}"


def conv_id(c):
    return f"{c['tag']}_{conv_path(c)}"


def lift_inputs(c):
    """Seeded fp32 inputs of one lift case: inp, w0, b0, dx0 and, as the case asks, the bag input
    (ubar, grid, bw, bb; inp then is None) and the hosted mix operands (Xs, Gs as float pairs)."""
    Cin, C, G, N, P, Bg = c["Cin"], c["C"], c["G"], c["N"], c["P"], c["Bg"]
    rng = np.random.default_rng(4000 + 131 * Cin + 17 * C + 5 * G + 3 * N[1] + N[0] + 7 * P[1] + Bg)
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)
    t = {"inp": f(Bg, *N, Cin), "w0": f(G, C, Cin, scale=1.0 / np.sqrt(Cin)), "b0": f(G, C, scale=0.3),
         "dx0": f(G * Bg, C, *P)}
    if c["identity"]:
        # _grid_planes: the planes gx, gy and 1 through the lift
        assert (Cin, C, G) == (2, 3, 1)
        t["w0"] = np.array([[[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]], np.float32)
        t["b0"] = np.array([[0.0, 0.0, 1.0]], np.float32)
    if c["bag"]:
        gy, gx = np.meshgrid(np.linspace(0, 1, N[1]), np.linspace(-1, 1, N[0]))
        t.update(ubar=f(Bg, N[0] * N[1]), grid=np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32),
                 bw=f(Cin, 3, scale=0.6), bb=f(Cin, scale=0.3), inp=None)
    if c["mix"]:
        K1, m2, _ = c["mix"]
        t.update(Xs=f(G * Bg, m2, C, K1, 2), Gs=f(G * Bg, m2, C, K1, 2))
    return t


def case_input64(c, t):
    """(the lift's input in float64, its error or None): the materialised field or the bag's h."""
    if not c["bag"]:
        return np.asarray(t["inp"], np.float64), None
    a = (t["ubar"], t["grid"], t["bw"], t["bb"], c["bag"][0], c["N"])
    return bag_h(*a), bag_h_bound(*a)


FWD_CASES = (
    # lift_fwd_wide_kernel<12, 16>: Cin 12, 5 <= C <= 16, G <= 4, in 16-B aligned (or the bag input)
    [_lcase(f"c{C}_g{G}", 12, C, G) for C in (5, 12, 16) for G in (1, 2, 4)]
    + [_lcase("nopad_c12_g2", 12, 12, 2, P=DEF_N), _lcase("line_c12_g1", 12, 12, 1, N=(1, 16), P=(1, 20)),
       _lcase("bag_invL1_c12_g2", 12, 12, 2, bag=(1.0, 1.0)),
       _lcase("bag_invL3_c5_g4", 12, 5, 4, bag=(1.0 / 3.0, 1.0)),
       _lcase("bag_invL3_c16_g1", 12, 16, 1, bag=(1.0 / 3.0, 1.0))]
    # the wide kernel's fall-backs to the lane-quad kernel
    + [_lcase("misaligned_c12_g2", 12, 12, 2, mis_in=True), _lcase("c12_g5", 12, 12, 5)]
    # lift_fwd_pt_kernel<16>: 5 <= C <= 16
    + [_lcase(f"cin3_c{C}_g{G}", 3, C, G) for C, G in ((5, 1), (6, 2), (7, 1), (8, 2), (16, 1))]
    + [_lcase("cin25_c12_g2", 25, 12, 2)]
    # lift_fwd_kernel: C <= 4 or C > 16
    + [_lcase("gridplanes_cin2_c3", 2, 3, 1, Bg=1, identity=True)]
    + [_lcase(f"cin3_c{C}_g{G}", 3, C, G) for C, G in ((4, 1), (17, 2), (32, 1))])

_MIX = (4, 3)            # K1, m2
BWD_CASES = (
    # lift_bwd_both_kernel<1>: d_in and partial, Cin 12, N2 % 16 == 0, P2 % 4 == 0
    [_lcase(f"c{C}_g{G}", 12, C, G) for C in (5, 12, 16) for G in (1, 2, 4)]
    + [_lcase(f"mix_ns{ns if ns else 'lib'}_c12_g2", 12, 12, 2, mix=(*_MIX, ns)) for ns in (1, 2, 0, 5)]
    + [_lcase("bag_c12_g2", 12, 12, 2, bag=(1.0 / 3.0, 0.25)), _lcase("bag_mix_c5_g4", 12, 5, 4, bag=(1.0 / 3.0, 0.25),
                                                                      mix=(*_MIX, 2)),
       _lcase("reduce_c12_g2", 12, 12, 2, N=(20, 16), P=(22, 20), reduce=True)]
    # two launches
    + [_lcase("in_only_c12_g2", 12, 12, 2, want_w=False), _lcase("in_only_cin3_c8_g2", 3, 8, 2, want_w=False),
       _lcase("in_only_c12_g5", 12, 12, 5, want_w=False),
       _lcase("in_only_misaligned_c12_g2", 12, 12, 2, want_w=False, mis_din=True),
       _lcase("n13_c12_g2", 12, 12, 2, N=(5, 13))]
    + [_lcase(f"w_only_cin{Cin}_c{C}_g{G}", Cin, C, G, want_in=False)
       for Cin, C, G in ((3, 5, 1), (12, 12, 2), (15, 16, 1), (16, 5, 2), (25, 12, 1), (31, 16, 2))]
    + [_lcase("w_only_cin32_c12_g1", 32, 12, 1, want_in=False), _lcase("w_only_cin12_c4_g2", 12, 4, 2, want_in=False),
       _lcase("w_only_cin12_c17_g1", 12, 17, 1, want_in=False),
       _lcase("w_only_n13_c12_g2", 12, 12, 2, N=(5, 13), want_in=False),
       _lcase("w_only_p18_c12_g1", 12, 12, 1, P=(7, 18), want_in=False),
       _lcase("w_only_dx0_misaligned_c12_g2", 12, 12, 2, want_in=False, mis_dx0=True),
       _lcase("w_only_reduce_cin3_c8_g2", 3, 8, 2, N=(20, 13), P=(22, 20), want_in=False, reduce=True)])


def _ccase(tag, C, P, act, G=1, Bg=DEF_BG, reduce=False):
    return {"tag": tag, "C": C, "P": P, "act": act, "G": G, "Bg": Bg, "reduce": reduce}


def conv_inputs(c):
    rng = np.random.default_rng(6000 + 131 * c["C"] + 17 * c["G"] + 3 * c["P"][1] + c["P"][0] + c["act"] + c["Bg"])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"dz": f(c["G"] * c["Bg"], c["C"], *c["P"]), "x": f(c["G"] * c["Bg"], c["C"], *c["P"])}


CONV_CASES = (
    # conv_wgrad_mfma_kernel<ACT>: 5 <= C <= 15; 7 x 20: float4 loads and a ragged last chunk (140 = 8 * 16 + 12),
    # 7 x 19: HW % 4 != 0, the scalar loader; 1 x 16: one chunk
    [_ccase(f"c{C}_{P[0]}x{P[1]}_g{G}", C, P, act, G)
     for C in (5, 12, 15) for P, G in (((7, 20), 1), ((7, 19), 2), ((1, 16), 4)) for act in (0, 1)]
    + [_ccase("reduce_c12_20x20_g2", 12, (20, 20), 1, 2, reduce=True)]
    # conv_wgrad_kernel<ACT>: C <= 4 or C >= 16; 13 x 23 = 299: two tiles per sample, the second ragged
    + [_ccase(f"c{C}_{P[0]}x{P[1]}_g{G}", C, P, act, G)
       for C, P, G in ((1, (7, 20), 1), (4, (13, 23), 2), (16, (7, 20), 2), (31, (13, 23), 1)) for act in (0, 1)]
    + [_ccase("reduce_c16_13x23_g2", 16, (13, 23), 0, 2, reduce=True)])

# the nchunk cap of 1024: the smallest shapes with more than 1024 tiles of 256 points, so that the
# workgroups' grid-stride tile loops run a second round
CAP_LIFT_LDS = _lcase("cap_1052tiles_cin3_c5", 3, 5, 1, N=(232, 232), P=(232, 232), Bg=5, want_in=False)
CAP_LIFT_MFMA = _lcase("cap_1050tiles_cin12_c5", 12, 5, 1, N=(224, 240), P=(224, 240), Bg=5, want_in=False)
CAP_CONV = _ccase("cap_1055tiles_c5_232x232", 5, (232, 232), 0, 1, Bg=5)
