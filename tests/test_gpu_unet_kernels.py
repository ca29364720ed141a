"""The entry points of csrc/unet.hip (include/blindno.h: dwconv, cnx_pw, maxpool, convt, tok_attn)
called through the C ABI on sentinel-guarded buffers, against tests/unet_stage_ref.py in float64.

Bar, per compared tensor: rel-L2 <= max(1e-5, 3 x e32), e32 the rel-L2 distance of the same
reference run in float32 on the CPU from float64 on the same inputs; maxpool is exact.  Every
output, partial and scratch buffer has 64 sentinel elements on each side and a NaN interior (255
for the uint8 arg), checked after the call: a write outside the buffer or an element left unwritten
shows.  Each case runs twice and the two results must be equal to the bit.  Where a case is listed
for a launch path, the path is asserted from the size queries, so a retuned constant fails the
test instead of silently moving the case to another path.  Refused calls must return non-zero
and leave every buffer untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import unet_stage_ref as ur

pytestmark = pytest.mark.gpu

M = 64
SENT = 77777.0
SENT8 = 171


class Guarded:
    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.n, self.u8 = shape, int(np.prod(shape)), dtype == torch.uint8
        self.sent, self.fill = (SENT8, 255) if self.u8 else (SENT, float("nan"))
        self.buf = torch.full((self.n + 2 * M,), self.sent, device="cuda", dtype=dtype)
        self.buf[M:M + self.n] = self.fill
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.buf.element_size() * M)

    def off(self, nbytes):
        return ctypes.c_void_p(self.ptr.value + nbytes)

    def raw(self):
        assert bool((self.buf[:M] == self.sent).all()) and bool((self.buf[M + self.n:] == self.sent).all()), \
            "a kernel wrote outside its buffer"
        return self.buf[M:M + self.n].view(*self.shape)

    def get(self):
        """The interior, every element written (float buffers: no NaN left)."""
        t = self.raw()
        if not self.u8:
            assert not bool(torch.isnan(t).any()), "an element was left unwritten"
        return t

    def untouched(self):
        t = self.raw()
        return bool((t == 255).all()) if self.u8 else bool(torch.isnan(t).all())


def _cuda(inp):
    return {k: v.cuda().contiguous() for k, v in inp.items() if torch.is_tensor(v)}


def _abi():
    from blindno import _lib
    return _lib.call, _lib.ptr, _lib.query, _lib.stream_ptr()


def _compare(tag, got, again, r64, e32, keys):
    bad, worst = [], 0.0
    for k in keys:
        assert torch.equal(got[k], again[k]), f"{tag} {k}: two calls differ"
        e, b = ur.rel(got[k], r64[k]), ur.bar(e32[k])
        worst = max(worst, e / b)
        print(f"{tag} {k:9s} rel-L2 {e:.2e}  e32 {e32[k]:.2e}  bar {b:.2e}")
        if not e <= b:
            bad.append((k, e, b))
    print(f"{tag} worst e/bar {worst:.3f}")
    assert not bad, bad


# ------------------------------------------------------------------------------------ dwconv
@pytest.mark.parametrize("case", ur.DWCONV_CASES)
def test_dwconv_against_float64(case):
    N, C, H, W, KH, KW = case
    call, ptr, query, st = _abi()
    inp, r64, e32 = ur.reference("dwconv", case)
    d = _cuda(inp)
    T, P = KH * KW, N * H * W
    default = query("blindno_dwconv_wgrad_nsplit", N, C, H, W)
    assert default == max(1, (P + 1023) // 1024) == 1          # ~1024 output pixels per split
    splits = sorted({1, 2, 3, default, P + 5})

    def run():
        o = {"y": Guarded(N, C, H, W), "y_nobias": Guarded(N, C, H, W), "dx": Guarded(N, C, H, W)}
        call("blindno_dwconv_fwd", ptr(d["x"]), ptr(d["w"]), ptr(d["b"]), o["y"].ptr, N, C, H, W, KH, KW, st)
        call("blindno_dwconv_fwd", ptr(d["x"]), ptr(d["w"]), None, o["y_nobias"].ptr, N, C, H, W, KH, KW, st)
        call("blindno_dwconv_bwd_data", ptr(d["dy"]), ptr(d["w"]), o["dx"].ptr, N, C, H, W, KH, KW, st)
        for ns in splits:
            o[f"dwb{ns}"] = Guarded(C, T + 1)
            part = Guarded(ns, C, T + 1) if ns > 1 else None
            call("blindno_dwconv_bwd_weight", ptr(d["dy"]), ptr(d["x"]), o[f"dwb{ns}"].ptr,
                 part.ptr if part else None, ns, N, C, H, W, KH, KW, st)
            if part:
                o[f"partial{ns}"] = part
        torch.cuda.synchronize()
        return {k: v.get().clone() for k, v in o.items()}
    got, again = run(), run()
    ref = dict(r64, **{f"dwb{ns}": r64["dwb"] for ns in splits})
    err = dict(e32, **{f"dwb{ns}": e32["dwb"] for ns in splits})
    _compare(f"dwconv {case}", got, again, ref, err, ["y", "y_nobias", "dx"] + [f"dwb{ns}" for ns in splits])
    big = got[f"partial{P + 5}"]                               # more splits than pixels: the empty ones are +0
    per = (P + P + 5 - 1) // (P + 5)
    first_empty = (P + per - 1) // per
    assert first_empty < P + 5 and float(big[first_empty:].abs().max()) == 0.0
    assert torch.equal(got[f"partial{P + 5}"], again[f"partial{P + 5}"])


# ------------------------------------------------------------------------------------ cnx_pw
@pytest.mark.parametrize("C,N,HW,regime", ur.CNX_CASES)
def test_cnx_pw_against_float64(C, N, HW, regime):
    call, ptr, query, st = _abi()
    inp, r64, e32 = ur.reference("cnx_pw", (C, N, HW, regime))
    d = _cuda(inp)
    pb = ur.CNX_PB[C]
    nblk = query("blindno_cnx_pw_bwd_nblk", N, C, HW)
    assert nblk == (N * HW + pb - 1) // pb                     # pb = cnx_pb(C) pixels per backward block
    assert nblk == {1: 1, pb: 1, pb + 1: 2, 2 * pb + 3: 3}.get(N * HW, 3)
    E = 8 * C * C + 7 * C
    if regime == "constant_pixel":
        assert bool(((inp["xd"].var(1, unbiased=False) == 0).sum(1) >= 1).all())
    prm = [ptr(d[k]) for k in ("lw", "lb", "w1", "b1", "w2")]

    def run():
        o = {"y": Guarded(N, C, HW), "dxd": Guarded(N, C, HW), "dparams": Guarded(E), "partial": Guarded(nblk, E)}
        call("blindno_cnx_pw_fwd", ptr(d["xd"]), ptr(d["sc"]), *prm, ptr(d["b2"]), o["y"].ptr, N, C, HW, st)
        call("blindno_cnx_pw_bwd", ptr(d["dy"]), ptr(d["xd"]), *prm, o["dxd"].ptr, o["dparams"].ptr,
             o["partial"].ptr, nblk, N, C, HW, st)
        torch.cuda.synchronize()
        r = {k: v.get().clone() for k, v in o.items()}
        r.update(ur.cnx_pieces(r["dparams"], C))
        return r
    got, again = run(), run()
    assert torch.equal(got["partial"], again["partial"])
    _compare(f"cnx_pw C={C} N={N} HW={HW} {regime}", got, again, r64, e32, ["y", "dxd"] + list(ur.CNX_PIECES))


# ------------------------------------------------------------------------------------ maxpool
@pytest.mark.parametrize("case", ur.MAXPOOL_CASES)
def test_maxpool_exact(case):
    NC, H, W, KH, KW = case
    call, ptr, query, st = _abi()
    Ho, Wo = H // KH, W // KW
    for variant in ur.MAXPOOL_VARIANTS:
        inp = ur.maxpool_inputs(*case, variant)
        ref = ur.maxpool(inp["x"], (KH, KW), inp["dy"])
        d = _cuda(inp)

        def run():
            o = {"y": Guarded(NC, Ho, Wo), "arg": Guarded(NC, Ho, Wo, dtype=torch.uint8), "dx": Guarded(NC, H, W)}
            call("blindno_maxpool_fwd", ptr(d["x"]), o["y"].ptr, o["arg"].ptr, NC, H, W, KH, KW, st)
            call("blindno_maxpool_bwd", ptr(d["dy"]), o["arg"].ptr, o["dx"].ptr, NC, H, W, KH, KW, st)
            torch.cuda.synchronize()
            return {k: v.raw().clone().cpu() for k, v in o.items()}
        got, again = run(), run()
        for k in ("y", "arg", "dx"):
            # y holds a NaN exactly where the reference does (the window with the NaN): equal_nan
            # on the values, so a NaN left from the prefill anywhere else fails
            same = torch.allclose(got[k], ref[k], rtol=0, atol=0, equal_nan=True) if k == "y" else torch.equal(got[k], ref[k])
            assert same, (variant, k)
            assert torch.allclose(got[k].float(), again[k].float(), rtol=0, atol=0, equal_nan=True), (variant, k)
        assert not bool(torch.isnan(got["dx"]).any())
        assert int(torch.isnan(got["y"]).sum()) == (1 if variant == "nan" else 0)
        if variant == "max_last":
            assert int(got["arg"][-1, 0, 0]) == KH * KW - 1
        if H % KH:
            assert float(got["dx"][:, Ho * KH:].abs().max()) == 0.0
        if W % KW:
            assert float(got["dx"][:, :, Wo * KW:].abs().max()) == 0.0
    if KH * KW == 255:
        assert int(got["arg"].max()) == 254


# ------------------------------------------------------------------------------------ convt
@pytest.mark.parametrize("case", ur.CONVT_CASES)
def test_convt_against_float64(case):
    N, Ci, Co, Hi, Wi, KH, KW, opH, opW = case
    call, ptr, query, st = _abi()
    inp, r64, e32 = ur.reference("convt", case)
    d = _cuda(inp)
    Ho, Wo = inp["Ho"], inp["Wo"]
    E = Ci * Co * KH * KW + Co
    nparts = query("blindno_convt_wgrad_nparts", N, Hi, Wi)
    chunks = {1: 1, 15: 1, 7: 1, 64: 1, 72: 2, 6: 1}[Hi * Wi]   # 64 input pixels per chunk
    assert nparts == N * chunks
    # 16 x 256 entries per (chunk, sample): past that the grid's z extent is capped and threads loop
    assert (E > 4096) == (case == (1, 32, 33, 2, 3, 2, 2, 0, 1)) and (E != 4257 or case[1] == 32)
    geo = (N, Ci, Hi, Wi, Co, KH, KW, Ho, Wo)

    def run():
        o = {"y": Guarded(N, Co, Ho, Wo), "y_nobias": Guarded(N, Co, Ho, Wo), "dx": Guarded(N, Ci, Hi, Wi),
             "dwb": Guarded(E), "partial": Guarded(nparts, E)}
        call("blindno_convt_fwd", ptr(d["x"]), ptr(d["w"]), ptr(d["b"]), o["y"].ptr, *geo, st)
        call("blindno_convt_fwd", ptr(d["x"]), ptr(d["w"]), None, o["y_nobias"].ptr, *geo, st)
        call("blindno_convt_bwd_data", ptr(d["dy"]), ptr(d["w"]), o["dx"].ptr, *geo, st)
        call("blindno_convt_bwd_weight", ptr(d["dy"]), ptr(d["x"]), o["dwb"].ptr, o["partial"].ptr, *geo, st)
        torch.cuda.synchronize()
        return {k: v.get().clone() for k, v in o.items()}
    got, again = run(), run()
    assert torch.equal(got["partial"], again["partial"])
    _compare(f"convt {case}", got, again, r64, e32, ["y", "y_nobias", "dx", "dwb"])
    yn = got["y_nobias"]
    assert float(yn[:, :, KH * Hi:].abs().max() if opH else 0.0) == 0.0      # output_padding: bias only
    assert float(yn[..., KW * Wi:].abs().max() if opW else 0.0) == 0.0


# ------------------------------------------------------------------------------------ tok_attn
def _tok_pad(B, L):
    """Index of the one float of the backward scratch that no kernel writes: the pad that brings
    the float2 tail ab to 8 bytes (before ab if B L + B is odd, else the last float)."""
    BL = B * L
    end = 3 * BL + B + 2 * BL * L
    return end if (BL + B) & 1 else end + 2 * BL


@pytest.mark.parametrize("shape,regime", ur.TOK_CASES)
def test_tok_attn_against_float64(shape, regime):
    B, L, D = shape
    call, ptr, query, st = _abi()
    inp, r64, e32 = ur.reference("tok_attn", (shape, regime))
    d = _cuda(inp)
    nch = query("blindno_tok_gram_nchunk", D)
    assert nch == {5: 1, 32: 1, 128: 1, 129: 2, 70: 1, 40: 1, 33: 1, 16: 1, 1: 1}[D]    # 128 points per chunk
    nsave = query("blindno_tok_attn_save_floats", B, L, D)
    assert nsave == 5 * B * L + 2 * B * L * L + B + B * D
    nscr = query("blindno_tok_attn_bwd_scratch_floats", B, L)
    assert nscr == 5 * B * L + B + 2 * B * L * L + 1
    if shape == (2, 90, 40):
        assert (L + 3) // 4 * ((L + 3) // 4 + 1) // 2 == 276            # a second round of 256 Gram blocks
    if regime == "sharp":
        assert float((r64["A"].max(-1).values >= 1 - 1e-7).double().mean()) >= 0.9
    X, lw, lb, dY = (ptr(d[k]) for k in ("X", "lw", "lb", "dY"))

    def run():
        o = {"Ybar": Guarded(B, D), "save": Guarded(nsave), "gram": Guarded(B, L, L),
             "dX": Guarded(B, L, D), "dlw": Guarded(D), "dlb": Guarded(D), "scratch": Guarded(nscr)}
        gp = None                                                  # one chunk: gram_partial = NULL
        if nch > 1:
            o["gram_partial"] = Guarded(nch, B, L, L)
            gp = o["gram_partial"].ptr
        call("blindno_tok_attn_fwd", X, lw, lb, o["Ybar"].ptr, o["save"].ptr, gp, o["gram"].ptr, B, L, D,
             ur.TOK_EPS, st)
        sv = o["save"].ptr
        call("blindno_tok_attn_bwd", dY, X, lw, sv, o["dX"].ptr, o["dlw"].ptr, o["dlb"].ptr, o["scratch"].ptr,
             B, L, D, st)
        # the optional outputs, one run each; what is not asked for stays untouched
        e = {k: Guarded(*o[k.split("_")[0]].shape) for k in ("dX_a", "dlw_a", "dlb_a", "scratch_a", "dX_b", "dlw_b",
                                                             "dlb_b", "scratch_b", "dlw_c", "dlb_c", "dlw_d",
                                                             "dlb_d", "scratch_c", "scratch_d")}
        call("blindno_tok_attn_bwd", dY, X, lw, sv, None, e["dlw_a"].ptr, e["dlb_a"].ptr, e["scratch_a"].ptr, B, L, D, st)
        call("blindno_tok_attn_bwd", dY, X, lw, sv, e["dX_b"].ptr, None, None, e["scratch_b"].ptr, B, L, D, st)
        call("blindno_tok_attn_bwd", dY, X, lw, sv, None, e["dlw_c"].ptr, None, e["scratch_c"].ptr, B, L, D, st)
        call("blindno_tok_attn_bwd", dY, X, lw, sv, None, None, e["dlb_d"].ptr, e["scratch_d"].ptr, B, L, D, st)
        torch.cuda.synchronize()
        for k in ("dX_a", "scratch_a", "dlw_b", "dlb_b", "dlb_c", "scratch_c", "dlw_d", "scratch_d"):
            assert e[k].untouched(), k
        r = {k: v.get().clone() for k, v in o.items() if k != "scratch"}
        for k in ("scratch", "scratch_b"):
            s = (o[k] if k == "scratch" else e[k]).raw()
            nan = torch.isnan(s).nonzero().flatten().tolist()
            assert nan == [_tok_pad(B, L)], (k, nan[:8])
        assert torch.equal(e["dlw_a"].get(), r["dlw"]) and torch.equal(e["dlb_a"].get(), r["dlb"])
        assert torch.equal(e["dX_b"].get(), r["dX"])
        assert torch.equal(e["dlw_c"].get(), r["dlw"]) and torch.equal(e["dlb_d"].get(), r["dlb"])
        r.update(ur.split_save(r["save"], B, L, D))
        return r
    got, again = run(), run()
    assert torch.equal(got["save"], again["save"]) and torch.equal(got["gram"], again["gram"])
    # st's fourth lane is the low part of the token mean: xbar + w is the mean to well below an
    # ulp of xbar (the float32 sum of D residuals of size std: <= D 2^-24 std / D per token)
    mean2 = got["xbar"].double().cpu() + got["w"].double().cpu()
    err = (mean2 - r64["xbar"]).abs()
    std = inp["X"].double().std(-1) if D > 1 else torch.zeros(B, L, dtype=torch.float64)
    assert bool((err <= 2.0 ** -22 * std + 2.0 ** -40 * r64["xbar"].abs()).all()), float(err.max())
    assert torch.equal(got["gram"], got["gram"].transpose(1, 2)), "the mirrored Gram blocks differ"
    _compare(f"tok_attn {shape} {regime}", got, again, r64, e32,
             ["Ybar", "dX", "dlw", "dlb"] + list(ur.SAVE_PIECES))
    if L == 1:
        assert torch.equal(got["A"].cpu(), torch.ones(B, 1, 1))
    if D == 1:
        assert torch.equal(got["Ybar"].cpu(), inp["lb"].expand(B, D))


# ------------------------------------------------------------------------------------ refusals
def test_invalid_arguments_are_refused():
    """Each call returns non-zero before any launch and leaves every buffer untouched.  The three
    entries of convt (and of dwconv, of maxpool) apply one rule: what the forward refuses, the
    backward entries refuse."""
    from blindno import _lib
    _, ptr, query, st = _abi()
    z = torch.zeros(1 << 16, device="cuda")
    g = [Guarded(1 << 16) for _ in range(4)]
    g8 = Guarded(1 << 12, dtype=torch.uint8)
    big = [Guarded(2 * 481 * 481 + 8 * 481 + 64) for _ in range(2)]
    a, b, c, e = (x.ptr for x in g)
    zp = ptr(z)
    bad = []

    def refuse(name, *args):
        rc = query(name, *args)
        torch.cuda.synchronize()
        if rc == 0 or not all(x.untouched() for x in g + [g8] + big):
            bad.append((name, [v for v in args if isinstance(v, (int, float))], rc))

    def vary(name, head, geo, variants, tail=()):
        for i, v in variants:
            gg = list(geo)
            gg[i] = v
            refuse(name, *head, *tail, *gg, st)

    # dwconv: (N, C, H, W, KH, KW)
    geo = (1, 2, 3, 3, 7, 7)
    sizes = [(i, 0) for i in range(6)] + [(i, -1) for i in range(6)]
    for name, head, tail in (("blindno_dwconv_fwd", (zp, zp, zp, a), ()),
                             ("blindno_dwconv_bwd_data", (zp, zp, a), ()),
                             ("blindno_dwconv_bwd_weight", (zp, zp, a, b), (1,))):
        vary(name, head, geo, sizes, tail)
        vary(name, head, (1, 2, 3, 3, 5, 10), [(0, 1)], tail)            # 50 taps
        vary(name, head, (1, 2, 3, 3, 7, 8), [(0, 1)], tail)             # 56 taps
    refuse("blindno_dwconv_bwd_weight", zp, zp, a, b, 0, *geo, st)                     # nsplit = 0
    refuse("blindno_dwconv_bwd_weight", zp, zp, a, None, 2, *geo, st)                  # partial = NULL
    # cnx_pw: (N, C, HW)
    w = (zp,) * 6
    for N, C, HW in ((0, 4, 5), (2, 4, 0), (2, 3, 5), (2, 128, 5), (-1, 4, 5)):
        refuse("blindno_cnx_pw_fwd", zp, zp, *w, a, N, C, HW, st)
        refuse("blindno_cnx_pw_bwd", zp, zp, *w[:5], a, b, c, 1, N, C, HW, st)
    nblk = query("blindno_cnx_pw_bwd_nblk", 2, 4, 300)
    assert nblk == 3
    for nb in (nblk - 1, nblk + 1):
        refuse("blindno_cnx_pw_bwd", zp, zp, *w[:5], a, b, c, nb, 2, 4, 300, st)
    refuse("blindno_cnx_pw_bwd", zp, zp, *w[:5], a, b, None, nblk, 2, 4, 300, st)
    # maxpool: (NC, H, W, KH, KW)
    for geo in ((0, 4, 4, 2, 2), (2, 1, 4, 2, 2), (2, 4, 1, 2, 2), (2, 4, 4, 0, 2), (2, 4, 4, 2, 0),
                (1, 16, 16, 16, 16)):                                            # 256 taps
        refuse("blindno_maxpool_fwd", zp, a, g8.ptr, *geo, st)
        refuse("blindno_maxpool_bwd", zp, g8.ptr, a, *geo, st)
    # convt: (N, Ci, Hi, Wi, Co, KH, KW, Ho, Wo), valid (2, 3, 4, 5, 2, 2, 2, 8..9, 10..11)
    geo = (2, 3, 4, 5, 2, 2, 2, 8, 10)
    variants = [(i, 0) for i in range(7)] + [(7, 7), (7, 10), (8, 9), (8, 12), (7, 0), (8, 0), (0, -1)]
    vary("blindno_convt_fwd", (zp, zp, zp, a), geo, variants)
    vary("blindno_convt_bwd_data", (zp, zp, a), geo, variants)
    vary("blindno_convt_bwd_weight", (zp, zp, a, b), geo, variants)
    refuse("blindno_convt_bwd_weight", zp, zp, a, None, *geo, st)
    # tok_attn: (B, L, D)
    s, gr = big
    for B, L, D in ((0, 3, 8), (1, 0, 8), (1, 3, 0), (1, 481, 4), (-1, 3, 8)):
        refuse("blindno_tok_attn_fwd", zp, zp, zp, a, s.ptr, b, gr.ptr, B, L, D, 1e-5, st)
        refuse("blindno_tok_attn_bwd", zp, zp, zp, zp, a, b, c, s.ptr, B, L, D, st)
    refuse("blindno_tok_attn_fwd", zp, zp, zp, a, s.off(4), b, gr.ptr, 1, 3, 8, 1e-5, st)      # save + 4 bytes
    refuse("blindno_tok_attn_fwd", zp, zp, zp, a, None, b, gr.ptr, 1, 3, 8, 1e-5, st)
    refuse("blindno_tok_attn_fwd", zp, zp, zp, a, s.ptr, b, None, 1, 3, 8, 1e-5, st)
    refuse("blindno_tok_attn_fwd", zp, zp, zp, a, s.ptr, None, gr.ptr, 1, 3, 129, 1e-5, st)   # two chunks
    refuse("blindno_tok_attn_bwd", zp, zp, zp, ctypes.c_void_p(z.data_ptr() + 4), a, b, c, s.ptr, 1, 3, 8, st)
    refuse("blindno_tok_attn_bwd", zp, zp, zp, zp, a, b, c, s.off(4), 1, 3, 8, st)            # scratch + 4 bytes
    refuse("blindno_tok_attn_bwd", zp, zp, zp, zp, a, b, c, None, 1, 3, 8, st)
    assert not bad, bad
    # a valid call still succeeds afterwards
    _lib.call("blindno_dwconv_fwd", zp, zp, zp, a, 1, 2, 3, 3, 7, 7, st)
    torch.cuda.synchronize()
    assert float(g[0].raw()[:18].abs().max()) == 0.0
