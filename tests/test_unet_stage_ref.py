"""Pins tests/unet_stage_ref.py, the float64 reference of the attention-UNet kernels, on the host:
its forms agree with each other and with oracle.unet_ref to 1e-12, the special input regimes of
tests/test_gpu_unet_kernels.py have the property they are named for (on the float64 reference
alone), and every seeded mutant of the reference, evaluated in float32, exceeds that file's bar
max(1e-5, 3 x e32) on at least one compared tensor of one listed case.
"""
import pytest
import torch
import torch.nn.functional as F

import oracle.unet_ref as ou
import unet_stage_ref as ur

F64 = torch.float64
TOL = 1e-12


@pytest.mark.parametrize("shape,regime", ur.TOK_CASES)
def test_tok_attn_forms_agree(shape, regime):
    inp, r64, _ = ur.reference("tok_attn", (shape, regime))
    B, L, D = shape
    p = {"norm.weight": inp["lw"].double(), "norm.bias": inp["lb"].double()}
    assert ur.TOK_EPS == 1e-5                                   # the eps oracle.unet_ref hard-codes
    orc = ou.temporal_attention(p, inp["X"].double().view(B, L, D, 1)).mean(1).view(B, D)
    # 1e-12 presumes tokens whose mean is of the order of their spread.  The literal form subtracts
    # mean_d(A X + X) from A X + X, so its own float64 rounding grows in proportion to
    # |xbar| / std(X_t); the collapsed form never forms that difference.  "offset" is the regime
    # with that ratio >= 100 (500 here), and there the tolerance is scaled by ratio / 100.
    ratio = float((r64["xbar"].abs() / inp["X"].double().std(-1).clamp_min(1e-300)).max()) if D > 1 else 1.0
    tol = TOL * max(1.0, ratio / 100.0) if regime == "offset" else TOL
    assert ur.rel(r64["Ybar"], orc) <= TOL
    assert ur.rel(r64["Ybar_collapsed"], r64["Ybar"]) <= tol, ur.rel(r64["Ybar_collapsed"], r64["Ybar"])
    col = ur.tok_attn_collapsed(inp["X"], inp["lw"], inp["lb"], ur.TOK_EPS)
    assert col["save"].numel() == B * L + 2 * B * L * L + 4 * B * L + B + B * D
    pieces = ur.split_save(col["save"], B, L, D)
    for k in ur.SAVE_PIECES:
        assert torch.equal(pieces[k], col[k]), k
    assert float(pieces["w"].abs().max()) == 0.0
    if D == 1:
        assert torch.equal(col["Ybar"], inp["lb"].double().expand(B, D))


@pytest.mark.parametrize("C", ur.CNX_CS)
def test_cnx_pw_equals_oracle_convnext(C):
    N, HW = ur.cnx_sizes(C)[-1]
    inp, r64, _ = ur.reference("cnx_pw", (C, N, HW, "random"))
    delta = torch.zeros(C, 1, 7, 7, dtype=F64)
    delta[:, 0, 3, 3] = 1.0                                     # the depthwise part as the identity
    p = {"dwconv.weight": delta, "dwconv.bias": torch.zeros(C, dtype=F64), "norm.weight": inp["lw"].double(),
         "norm.bias": inp["lb"].double(), "pwconv1.weight": inp["w1"].double(), "pwconv1.bias": inp["b1"].double(),
         "pwconv2.weight": inp["w2"].double(), "pwconv2.bias": inp["b2"].double()}
    x = inp["xd"].double().view(N, C, 1, HW)
    orc = ou.convnext(p, x, 2).view(N, C, HW)
    mine = r64["y"] - inp["sc"].double() + inp["xd"].double()   # convnext's shortcut is its own input
    assert ur.rel(mine, orc) <= TOL


@pytest.mark.parametrize("case", ur.MAXPOOL_CASES)
def test_maxpool_equals_torch_on_tie_free_inputs(case):
    NC, H, W, KH, KW = case
    g = torch.Generator().manual_seed(5)
    x = torch.randperm(NC * H * W, generator=g).double().view(NC, H, W)      # tie-free
    dy = torch.randn(NC, H // KH, W // KW, generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr.unsqueeze(0), (KH, KW), return_indices=True)
    (y[0] * dy).sum().backward()
    ih, iw = idx[0] // W, idx[0] % W
    arg = (ih % KH) * KW + (iw % KW)
    got = ur.maxpool(x, (KH, KW), dy)
    assert torch.equal(got["y"], y[0].detach()) and torch.equal(got["arg"].long(), arg)
    assert torch.equal(got["dx"], xr.grad)


@pytest.mark.parametrize("case", ur.DWCONV_CASES)
def test_dwconv_formula(case):
    """The reference against the kernel comment's sum written as loops over the taps."""
    N, C, H, W, KH, KW = case
    inp, r64, _ = ur.reference("dwconv", case)
    x, w = inp["x"].double(), inp["w"].double()
    y = torch.zeros(N, C, H, W, dtype=F64)
    for i in range(KH):
        for j in range(KW):
            for h in range(H):
                hi = h + i - KH // 2
                if not 0 <= hi < H:
                    continue
                for q in range(W):
                    wi = q + j - KW // 2
                    if 0 <= wi < W:
                        y[:, :, h, q] += w[:, i, j] * x[:, :, hi, wi]
    assert ur.rel(r64["y_nobias"], y) <= TOL
    assert ur.rel(r64["y"], y + inp["b"].double().view(1, C, 1, 1)) <= TOL
    assert r64["dwb"].shape == (C, KH * KW + 1)
    assert ur.rel(r64["dwb"][:, -1], inp["dy"].double().sum((0, 2, 3))) <= TOL


@pytest.mark.parametrize("case", ur.CONVT_CASES)
def test_convt_padding_is_bias_only(case):
    N, Ci, Co, Hi, Wi, KH, KW, opH, opW = case
    inp, r64, _ = ur.reference("convt", case)
    y, yn = r64["y"], r64["y_nobias"]
    assert y.shape == (N, Co, KH * Hi + opH, KW * Wi + opW)
    assert float(yn[:, :, KH * Hi:].abs().max() if opH else 0.0) == 0.0
    assert float(yn[..., KW * Wi:].abs().max() if opW else 0.0) == 0.0
    x, w = inp["x"].double(), inp["w"].double()
    blocks = torch.einsum("nihw,ioab->nohawb", x, w).reshape(N, Co, KH * Hi, KW * Wi)
    assert ur.rel(yn[:, :, :KH * Hi, :KW * Wi], blocks) <= TOL
    assert r64["dwb"].numel() == Ci * Co * KH * KW + Co


# ------------------------------------------------------------------------------------ regimes
@pytest.mark.parametrize("shape", ur.TOK_SPECIAL)
def test_tok_regimes_hold(shape):
    _, sharp, _ = ur.reference("tok_attn", (shape, "sharp"))
    frac = float((sharp["A"].max(-1).values >= 1 - 1e-7).double().mean())
    assert frac >= 0.9, frac
    inp, off, _ = ur.reference("tok_attn", (shape, "offset"))
    ratio = off["xbar"].abs() / inp["X"].double().std(-1)
    assert float(ratio.min()) >= 100.0, float(ratio.min())
    inp, _, _ = ur.reference("tok_attn", (shape, "duplicates"))
    assert torch.equal(inp["X"][:, 0], inp["X"][:, 1])
    assert float(inp["X"][:, -1].max() - inp["X"][:, -1].min()) == 0.0


@pytest.mark.parametrize("C", ur.CNX_CS)
def test_cnx_regimes_hold(C):
    N, HW = ur.cnx_sizes(C)[-1]
    pb = ur.CNX_PB[C]
    assert N == 3 and 2 * pb + 3 <= N * HW <= 2 * pb + 5 and HW < pb < 2 * HW    # block 0 straddles samples 0 and 1
    inp = ur.cnx_inputs(C, N, HW, "offset")
    assert float((inp["xd"].double().mean(1).abs() / inp["xd"].double().std(1, unbiased=False).clamp_min(1e-300)).min()) >= 100 or C == 1
    if C >= 2:
        inp = ur.cnx_inputs(C, N, HW, "constant_pixel")
        var = inp["xd"].double().var(1, unbiased=False)                      # (N, HW), over C
        assert bool(((var == 0.0).sum(1) >= 1).all())


def test_maxpool_variants_hold():
    for case in ur.MAXPOOL_CASES:
        NC, H, W, KH, KW = case
        T = KH * KW
        ref = {v: ur.maxpool(ur.maxpool_inputs(*case, v)["x"], (KH, KW), ur.maxpool_inputs(*case, v)["dy"])
               for v in ur.MAXPOOL_VARIANTS}
        assert bool(torch.isnan(ref["nan"]["y"][-1, 0, 0])) and int(ref["nan"]["arg"][-1, 0, 0]) == T - 1
        assert float(ref["neginf"]["y"][-1, 0, 0]) == float("-inf") and int(ref["neginf"]["arg"][-1, 0, 0]) == 0
        assert int(ref["max_last"]["arg"][-1, 0, 0]) == T - 1
        assert bool((ref["constant"]["arg"][0] == 0).all())
        x = ur.maxpool_inputs(*case, "ties")["x"]
        assert x.unique().numel() <= 7
        dx = ref["ties"]["dx"]
        assert float(dx[:, (H // KH) * KH:].abs().max() if H % KH else 0.0) == 0.0
    assert int(ur.maxpool(ur.maxpool_inputs(1, 15, 17, 15, 17, "max_last")["x"], (15, 17),
                          torch.ones(1, 1, 1))["arg"].max()) == 254


# ------------------------------------------------------------------------------------ mutants
def _caught(family, mutant, cases=None):
    """Largest e / bar of the float32 mutant over the family's listed cases and compared tensors."""
    worst = 0.0
    for case in cases or ur.FAMILIES[family][0]:
        inp, r64, e32 = ur.reference(family, case)
        m = ur.run(family, inp, torch.float32, mutant)
        for k in r64:
            if k != "Ybar_collapsed":
                worst = max(worst, ur.rel(m[k], r64[k]) / ur.bar(e32[k]))
    return worst


@pytest.mark.parametrize("family,mutant", [("tok_attn", "no_identity"), ("tok_attn", "uncentred_P"),
                                           ("convt", "pad_row_gets_xw"), ("cnx_pw", "swap_affine_grads"),
                                           ("cnx_pw", "eps_outside")])
def test_mutants_are_caught(family, mutant):
    cases = [c for c in ur.CNX_CASES if c[0] in (2, 8)] if family == "cnx_pw" else None
    worst = _caught(family, mutant, cases)
    print(f"{family} {mutant}: worst e / bar {worst:.3g}")
    assert worst > 1.0, worst


def test_unmutated_float32_reference_passes_its_own_bar():
    """e32 / bar <= 1/3 by construction; a mutant's excess is therefore the mutation's."""
    for family in ur.FAMILIES:
        case = ur.FAMILIES[family][0][1]
        inp, r64, e32 = ur.reference(family, case)
        m = ur.run(family, inp, torch.float32)
        assert all(ur.rel(m[k], r64[k]) <= ur.bar(e32[k]) for k in r64)


def test_maxpool_mutant_is_caught():
    hit = 0
    for case in ur.MAXPOOL_CASES:
        for v in ur.MAXPOOL_VARIANTS:
            inp = ur.maxpool_inputs(*case, v)
            good, bad = (ur.maxpool(inp["x"], case[3:], inp["dy"], m) for m in (None, "last_max"))
            hit += not (torch.equal(good["arg"], bad["arg"]) and torch.equal(good["dx"], bad["dx"]))
    assert hit >= 1
