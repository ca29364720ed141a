"""Plain-torch CPU restatement of every entry point of csrc/unet.hip (include/blindno.h,
"permutation-invariant attention UNet"), one function per entry family, in float64 or float32
(``dtype``).  TEST INFRASTRUCTURE: tests/test_unet_stage_ref.py pins it on the host,
tests/test_gpu_unet_kernels.py compares the kernels with it.

Every function returns a dict of the tensors the family's entries write, in the entries' own
layouts.  Forwards are written from the formulas in the kernels' comments, backwards come from
autograd of those forwards (``dy`` is the incoming gradient).  ``mutant`` selects a deliberately
wrong variant; the tests use them to show that their comparisons discriminate.

The module also holds the case lists and the seeded inputs that both test files use.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


# ------------------------------------------------------------------------------ dwconv
def dwconv(x, w, b, dy, dtype=F64):
    """y[n][c][h][w] = b[c] + sum_ij W[c][i][j] x[n][c][h + i - KH/2][w + j - KW/2]: padding K/2
    before and K - 1 - K/2 after (equal for odd K).  x (N, C, H, W), w (C, KH, KW), b (C) or
    None.  dwb (C, KH KW + 1) = [dW | db]; db is formed whether or not a bias is given."""
    C, KH, KW = w.shape
    xl, wl = _leaf(x, dtype), _leaf(w, dtype)
    bl = _leaf(b if b is not None else torch.zeros(C), dtype)
    ph, pw = KH // 2, KW // 2
    xp = F.pad(xl, (pw, KW - 1 - pw, ph, KH - 1 - ph))
    y = F.conv2d(xp, wl.view(C, 1, KH, KW), bl, groups=C)
    (y * dy.to(dtype)).sum().backward()
    yo = y.detach() if b is not None else (y - bl.view(1, C, 1, 1)).detach()
    return {"y": yo, "dx": xl.grad, "dwb": torch.cat((wl.grad.reshape(C, KH * KW), bl.grad.view(C, 1)), 1)}


# ------------------------------------------------------------------------------ cnx_pw
CNX_PIECES = ("dW1", "db1", "dW2", "db2", "dgamma", "dbeta")


def cnx_pieces(dparams, C):
    """Split the entry's dparams vector [dW1 | db1 | dW2 | db2 | dgamma | dbeta]."""
    sizes = (4 * C * C, 4 * C, 4 * C * C, C, C, C)
    return dict(zip(CNX_PIECES, torch.split(dparams.reshape(-1), sizes)))


def cnx_pw(xd, sc, lw, lb, w1, b1, w2, b2, dy, dtype=F64, mutant=None):
    """y = Linear2(GELU(Linear1(LayerNorm_C(xd)))) + sc per pixel; xd, sc, dy (N, C, HW);
    LayerNorm with biased variance and eps 1e-6 inside the root.  dxd is the gradient at xd
    alone (the shortcut's is dy itself).  Mutants: "eps_outside" (1 / (sqrt(var) + eps)),
    "swap_affine_grads" (dgamma and dbeta exchanged in dparams)."""
    t = [_leaf(v, dtype) for v in (xd, sc, lw, lb, w1, b1, w2, b2)]
    xdl, scl, lwl, lbl, w1l, b1l, w2l, b2l = t
    h = xdl.permute(0, 2, 1)                                            # (N, HW, C)
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    r = 1.0 / (torch.sqrt(var) + 1e-6) if mutant == "eps_outside" else 1.0 / torch.sqrt(var + 1e-6)
    ln = (h - mu) * r * lwl + lbl
    z = ln @ w1l.T + b1l
    g = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    y = (g @ w2l.T + b2l).permute(0, 2, 1) + scl
    (y * dy.to(dtype)).sum().backward()
    order = (w1l, b1l, w2l, b2l, lbl, lwl) if mutant == "swap_affine_grads" else (w1l, b1l, w2l, b2l, lwl, lbl)
    return {"y": y.detach(), "dxd": xdl.grad, "dparams": torch.cat([v.grad.reshape(-1) for v in order])}


# ------------------------------------------------------------------------------ maxpool
def maxpool(x, k, dy, mutant=None):
    """Window = stride = (KH, KW), floor.  x (NC, H, W) in any float dtype, evaluated as given:
    the operation is exact.  Scan order i (rows) then j; a tap replaces the running maximum if it
    is greater or a NaN (so the first maximum wins and a NaN wins over everything before it).
    arg (NC, Ho, Wo) uint8 = i KW + j.  dx: dy at the chosen tap, 0 elsewhere and on the
    dropped rows / columns.  Mutant "last_max": >= instead of >."""
    KH, KW = k
    NC, H, W = x.shape
    Ho, Wo = H // KH, W // KW
    win = x[:, :Ho * KH, :Wo * KW].reshape(NC, Ho, KH, Wo, KW).permute(0, 1, 3, 2, 4).reshape(NC, Ho, Wo, KH * KW)
    m, a = win[..., 0].clone(), torch.zeros(NC, Ho, Wo, dtype=torch.int64)
    for t in range(KH * KW):
        v = win[..., t]
        upd = ((v >= m) if mutant == "last_max" else (v > m)) | torch.isnan(v)
        m = torch.where(upd, v, m)
        a = torch.where(upd, torch.full_like(a, t), a)
    dwin = torch.zeros(NC, Ho, Wo, KH * KW, dtype=dy.dtype)
    dwin.scatter_(3, a.unsqueeze(-1), dy.reshape(NC, Ho, Wo, 1))
    dx = torch.zeros(NC, H, W, dtype=dy.dtype)
    dx[:, :Ho * KH, :Wo * KW] = dwin.reshape(NC, Ho, Wo, KH, KW).permute(0, 1, 3, 2, 4).reshape(NC, Ho * KH, Wo * KW)
    return {"y": m, "arg": a.to(torch.uint8), "dx": dx}


# ------------------------------------------------------------------------------ convt
def convt(x, w, b, Ho, Wo, dy, dtype=F64, mutant=None):
    """ConvTranspose2d with kernel = stride = (KH, KW) and output_padding (Ho - KH Hi,
    Wo - KW Wi): those rows / columns hold the bias only.  x (N, Ci, Hi, Wi), w (Ci, Co, KH, KW),
    b (Co) or None.  dwb = [dW | db].  Mutant "pad_row_gets_xw": the output_padding rows (or,
    without any, columns) also receive the products of the last input row (column)."""
    Ci, Co, KH, KW = w.shape
    Hi, Wi = x.shape[2:]
    xl, wl = _leaf(x, dtype), _leaf(w, dtype)
    bl = _leaf(b if b is not None else torch.zeros(Co), dtype)
    opH, opW = Ho - KH * Hi, Wo - KW * Wi
    y = F.conv_transpose2d(xl, wl, bl, stride=(KH, KW), output_padding=(opH, opW))
    if mutant == "pad_row_gets_xw":
        nb = y - bl.view(1, Co, 1, 1)
        if opH:
            y = torch.cat((y[:, :, :KH * Hi], y[:, :, KH * Hi:] + nb[:, :, KH * (Hi - 1):KH * (Hi - 1) + opH]), 2)
        elif opW:
            y = torch.cat((y[..., :KW * Wi], y[..., KW * Wi:] + nb[..., KW * (Wi - 1):KW * (Wi - 1) + opW]), 3)
    (y * dy.to(dtype)).sum().backward()
    yo = y.detach() if b is not None else (y - bl.view(1, Co, 1, 1)).detach()
    return {"y": yo, "dx": xl.grad, "dwb": torch.cat((wl.grad.reshape(-1), bl.grad))}


# ------------------------------------------------------------------------------ tok_attn
def tok_attn(X, lw, lb, eps, dY, dtype=F64):
    """The literal form: Ybar = mean_l LayerNorm_D(softmax(X X^T / sqrt D) X + X)_l, X (B, L, D),
    with dX, dlw, dlb by autograd."""
    Xl, lwl, lbl = _leaf(X, dtype), _leaf(lw, dtype), _leaf(lb, dtype)
    D = X.shape[-1]
    A = torch.softmax(Xl @ Xl.transpose(1, 2) / math.sqrt(D), -1)
    o = A @ Xl + Xl
    mu = o.mean(-1, keepdim=True)
    var = ((o - mu) ** 2).mean(-1, keepdim=True)
    Y = ((o - mu) / torch.sqrt(var + eps) * lwl + lbl).mean(1)
    (Y * dY.to(dtype)).sum().backward()
    return {"Ybar": Y.detach(), "dX": Xl.grad, "dlw": lwl.grad, "dlb": lbl.grad}


SAVE_PIECES = ("mu", "r", "c", "xbar", "A", "P", "kappa", "U")


def tok_attn_collapsed(X, lw, lb, eps, dtype=F64, mutant=None):
    """The collapsed form of the comment at the top of csrc/unet.hip: token means xbar, centred
    Gram Gc, A = softmax((Gc + D xbar xbar^T) / sqrt D), M = A + I, P = M Gc, mu = M xbar,
    var_l = (1/D) sum_s P_ls M_ls, r = (var + eps)^-1/2, c_t = (1/L) sum_l r_l M_lt,
    kappa = (1/L) sum_l r_l mu_l, U = sum_t c_t (X_t - xbar_t), Ybar = gamma U + beta.
    Returns the pieces and ``save`` in the layout of blindno_tok_attn_save_floats:
    st (B, L, 4) = (mu, r, c, 0) | xbar | A | P | kappa | U.
    Mutants: "no_identity" (M = A), "uncentred_P" (P from the raw Gram X X^T)."""
    X, lw, lb = X.to(dtype), lw.to(dtype), lb.to(dtype)
    B, L, D = X.shape
    xbar = X.mean(-1)
    Xc = X - xbar.unsqueeze(-1)
    Gc = Xc @ Xc.transpose(1, 2)
    A = torch.softmax((Gc + D * xbar.unsqueeze(2) * xbar.unsqueeze(1)) / math.sqrt(D), -1)
    M = A if mutant == "no_identity" else A + torch.eye(L, dtype=dtype)
    P = M @ ((X @ X.transpose(1, 2)) if mutant == "uncentred_P" else Gc)
    mu = (M @ xbar.unsqueeze(-1)).squeeze(-1)
    var = ((P * M).sum(-1) / D).clamp_min(0.0)
    r = 1.0 / torch.sqrt(var + eps)
    c = (r.unsqueeze(-1) * M).sum(1) / L
    kappa = (r * mu).sum(1) / L
    U = (c.unsqueeze(-1) * Xc).sum(1)
    st = torch.stack((mu, r, c, torch.zeros_like(mu)), -1)
    save = torch.cat([t.reshape(-1) for t in (st, xbar, A, P, kappa, U)])
    return {"Ybar": lw * U + lb, "mu": mu, "r": r, "c": c, "xbar": xbar, "A": A, "P": P, "kappa": kappa,
            "U": U, "save": save}


def split_save(save, B, L, D):
    """The pieces of a save buffer (blindno_tok_attn_save_floats layout); "w" is st's fourth lane: 0
    in the reference, the low part of the float32 token mean (mean = xbar + w) on the device."""
    BL = B * L
    sizes = (4 * BL, BL, BL * L, BL * L, B, B * D)
    st, xbar, A, P, kappa, U = torch.split(save.reshape(-1)[:sum(sizes)], sizes)
    st = st.view(B, L, 4)
    return {"mu": st[..., 0], "r": st[..., 1], "c": st[..., 2], "w": st[..., 3], "xbar": xbar.view(B, L),
            "A": A.view(B, L, L), "P": P.view(B, L, L), "kappa": kappa, "U": U.view(B, D)}


# ============================================================================== cases and inputs
DWCONV_CASES = [(1, 1, 1, 1, 7, 7), (2, 3, 5, 4, 7, 7), (3, 2, 1, 9, 1, 7), (2, 5, 13, 11, 7, 7),
                (1, 2, 6, 7, 5, 3), (1, 2, 6, 6, 2, 4)]

CNX_CS = (1, 2, 4, 8, 16, 32, 64)
# cnx_pb(C), the backward's pixels per workgroup: 12 C floats per pixel next to the staged weights
# in 64 KiB of LDS.  C = 32 has 16 (32 pixels would need 82 KB), checked against
# blindno_cnx_pw_bwd_nblk by the GPU test
CNX_PB = {1: 256, 2: 256, 4: 256, 8: 128, 16: 64, 32: 16, 64: 16}


def cnx_sizes(C):
    """(N, HW) with N HW = 1, pb, pb + 1, 2 pb + 3, and three samples over three blocks: 2 pb + 3 is
    never a multiple of 3 (pb is a power of two), so the three-sample case takes the smallest HW
    with 3 HW >= 2 pb + 3; block 0 then straddles samples 0 and 1 and the last block is ragged."""
    pb = CNX_PB[C]
    return [(1, 1), (1, pb), (1, pb + 1), (1, 2 * pb + 3), (3, (2 * pb + 3 + 2) // 3)]


CNX_CASES = [(C, N, HW, "random") for C in CNX_CS for (N, HW) in cnx_sizes(C)] + \
            [(C, *cnx_sizes(C)[-1], "offset") for C in CNX_CS] + \
            [(C, *cnx_sizes(C)[-1], "constant_pixel") for C in CNX_CS if C >= 2]

MAXPOOL_CASES = [(3, 7, 6, 2, 2), (2, 1, 9, 1, 2), (1, 2, 2, 2, 2), (2, 5, 5, 1, 1), (1, 16, 15, 3, 5),
                 (1, 15, 17, 15, 17)]
MAXPOOL_VARIANTS = ("ties", "constant", "nan", "neginf", "max_last")

CONVT_CASES = [(2, 3, 2, 1, 1, 2, 2, 0, 0), (1, 4, 4, 3, 5, 2, 2, 1, 1), (3, 2, 1, 1, 7, 1, 2, 0, 1),
               (2, 2, 3, 8, 8, 2, 2, 0, 0), (2, 8, 4, 9, 8, 2, 2, 1, 0), (1, 32, 33, 2, 3, 2, 2, 0, 1)]

TOK_SHAPES = [(2, 1, 5), (2, 3, 32), (1, 5, 128), (2, 7, 129), (1, 9, 70), (2, 90, 40), (1, 130, 33),
              (1, 480, 16), (3, 6, 1)]
TOK_SPECIAL = [(2, 7, 129), (2, 90, 40)]
TOK_CASES = [(s, "random") for s in TOK_SHAPES] + \
            [(s, r) for r in ("sharp", "offset", "duplicates") for s in TOK_SPECIAL]
TOK_EPS = 1e-5
# "sharp": X = scale x randn.  The diagonal score |X_l|^2 / sqrt D ~ scale^2 sqrt D stands
# scale^2 (sqrt D - O(1)) above the others at D = 129; at L = 90, D = 40 some other token can win
# a row, and the scale keeps the two largest scores of nearly every row more than ln(1e7) apart
TOK_SHARP_SCALE = {(2, 7, 129): 3.0, (2, 90, 40): 100.0}


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1009 + (k if isinstance(k, int) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def dwconv_inputs(N, C, H, W, KH, KW):
    g = _gen("dw", N, C, H, W, KH, KW)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"x": r(N, C, H, W), "w": 0.2 * r(C, KH, KW), "b": r(C), "dy": r(N, C, H, W)}


def cnx_inputs(C, N, HW, regime):
    g = _gen("cnx", C, N, HW, regime)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = {"xd": 1.5 * r(N, C, HW) + 0.3, "sc": r(N, C, HW), "lw": 1 + 0.2 * r(C), "lb": 0.1 * r(C),
           "w1": r(4 * C, C) / C ** 0.5, "b1": 0.1 * r(4 * C), "w2": r(C, 4 * C) / (4 * C) ** 0.5,
           "b2": 0.1 * r(C), "dy": r(N, C, HW)}
    if regime == "offset":
        inp["xd"] = 100.0 + 0.01 * r(N, C, HW)
    elif regime == "constant_pixel":
        for n in range(N):
            inp["xd"][n, :, (7 * n + 1) % HW] = 0.75 + n
    return inp


def maxpool_inputs(NC, H, W, KH, KW, variant):
    """Small integers (ties everywhere) plus: "constant" plane 0 all equal; "nan" one NaN at the
    last tap of window (0, 0) of the last plane; "neginf" that window all -inf; "max_last" the
    strict maximum of that window planted at its last tap (arg = KH KW - 1)."""
    g = _gen("mp", NC, H, W, KH, KW, variant)
    x = torch.randint(-3, 4, (NC, H, W), generator=g).float()
    dy = torch.randn(NC, H // KH, W // KW, generator=g)
    if variant == "constant":
        x[0] = 1.5
    elif variant == "nan":
        x[-1, KH - 1, KW - 1] = float("nan")
    elif variant == "neginf":
        x[-1, :KH, :KW] = float("-inf")
    elif variant == "max_last":
        x[-1, KH - 1, KW - 1] = 9.0
    return {"x": x, "dy": dy}


def convt_inputs(N, Ci, Co, Hi, Wi, KH, KW, opH, opW):
    g = _gen("ct", N, Ci, Co, Hi, Wi, KH, KW, opH, opW)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Ho, Wo = KH * Hi + opH, KW * Wi + opW
    return {"x": r(N, Ci, Hi, Wi), "w": r(Ci, Co, KH, KW) / Ci ** 0.5, "b": r(Co), "dy": r(N, Co, Ho, Wo),
            "Ho": Ho, "Wo": Wo}


def tok_inputs(shape, regime):
    B, L, D = shape
    g = _gen("tok", B, L, D, regime)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    X = r(B, L, D) + 0.5 * r(B, L, 1)                   # per-token offsets
    if regime == "sharp":
        X = TOK_SHARP_SCALE[shape] * r(B, L, D)
    elif regime == "offset":
        X = 50.0 + 0.1 * r(B, L, D)
    elif regime == "duplicates":
        X[:, 1] = X[:, 0]
        X[:, L - 1] = 0.625
    return {"X": X, "lw": 1 + 0.2 * r(D), "lb": 0.1 * r(D), "dY": r(B, D)}


# ============================================================================== one call per family
FAMILIES = {"dwconv": (DWCONV_CASES, dwconv_inputs), "cnx_pw": (CNX_CASES, cnx_inputs),
            "convt": (CONVT_CASES, convt_inputs), "tok_attn": (TOK_CASES, tok_inputs)}


def run(family, inp, dtype=F64, mutant=None):
    """Every tensor the GPU test compares for one case of a family (maxpool is exact and has its
    own path), evaluated in ``dtype``."""
    kw = {"mutant": mutant} if mutant else {}
    if family == "dwconv":
        o = dwconv(inp["x"], inp["w"], inp["b"], inp["dy"], dtype)
        o["y_nobias"] = dwconv(inp["x"], inp["w"], None, inp["dy"], dtype)["y"]
        return o
    if family == "cnx_pw":
        o = cnx_pw(*[inp[k] for k in ("xd", "sc", "lw", "lb", "w1", "b1", "w2", "b2", "dy")], dtype, **kw)
        o.update(cnx_pieces(o.pop("dparams"), inp["lw"].numel()))
        return o
    if family == "convt":
        o = convt(inp["x"], inp["w"], inp["b"], inp["Ho"], inp["Wo"], inp["dy"], dtype, **kw)
        o["y_nobias"] = convt(inp["x"], inp["w"], None, inp["Ho"], inp["Wo"], inp["dy"], dtype, **kw)["y"]
        return o
    if family == "tok_attn":
        o = tok_attn(inp["X"], inp["lw"], inp["lb"], TOK_EPS, inp["dY"], dtype)
        col = tok_attn_collapsed(inp["X"], inp["lw"], inp["lb"], TOK_EPS, dtype, **kw)
        o.update({k: col[k] for k in SAVE_PIECES})
        o["Ybar_collapsed"] = col["Ybar"]
        return o
    raise KeyError(family)


_REF = {}


def reference(family, case):
    """(inputs, float64 reference, e32 per tensor) of a listed case, computed once and shared.
    e32 is the rel-L2 distance of the same reference run in float32 from the float64 one."""
    key = (family, case)
    if key not in _REF:
        inp = FAMILIES[family][1](*case)
        r64, r32 = run(family, inp, F64), run(family, inp, torch.float32)
        _REF[key] = (inp, r64, {k: rel(r32[k], r64[k]) for k in r64})
    return _REF[key]


def bar(e32):
    """The project's bar per compared tensor: rel-L2 <= max(1e-5, 3 x e32)."""
    return max(1e-5, 3.0 * e32)
