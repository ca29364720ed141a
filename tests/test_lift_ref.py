"""The float64 lift / conv weight-gradient references of tests/lift_ref.py checked on the host,
without a GPU:

* they equal float64 torch autograd of F.linear + permute + F.pad (the lift, grouped: the input
  gradient sums over the groups), of fc0([grid, ubar]) (the bag input and d ubar), of F.conv2d with
  a 1x1 kernel on GELU^act(x) (the conv weight gradient) and of the complex mix einsum (the hosted
  spectral weight gradient), to 1e-12 rel-L2;
* a plain fp32 numpy evaluation of the same formulas stays inside every derived bound of lift_ref
  (module docstring there) on exactly the inputs of every GPU case, with the sums taken in
  sequential and in pairwise order; the worst err / bound ratio of each case is printed and must
  leave room (<= 0.5);
* with act the inputs stay in |x| <= 12, the range for which GELU_ABS is stated;
* every case id ends in the path lift_ref's restatement of the dispatchers selects, every path
  has a case, and the cap cases have more than 1024 tiles.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lift_ref as lr
from conftest import rel_l2
from spectral_stage_ref import cplx, gelu

ROOM = 0.5
ORDERS = ("seq", "pair")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _sum32(terms, order):
    """Sum of fp32 terms over axis 0, every addition rounded to fp32, in the given order."""
    a = np.asarray(terms, np.float32)
    if order == "seq":
        return np.cumsum(a, axis=0, dtype=np.float32)[-1]
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros_like(a[:1])])
        a = a[0::2] + a[1::2]
    return a[0]


def _f32(a):
    return np.asarray(a, np.float32)


# ------------------------------------------------------------------------------- fp32 evaluations
def _h32(c, t, order):
    """The lift's input in fp32: the field, or the bag's h with the u weight scaled first."""
    if not c["bag"]:
        return t["inp"]
    bw, g, N = t["bw"], t["grid"], c["N"]
    wu = bw[:, 2] * np.float32(c["bag"][0])
    terms = np.stack([np.broadcast_to(t["bb"], (c["Bg"], g.shape[0], c["Cin"])),
                      np.broadcast_to(g[None, :, 0, None] * bw[None, None, :, 0], (c["Bg"], g.shape[0], c["Cin"])),
                      np.broadcast_to(g[None, :, 1, None] * bw[None, None, :, 1], (c["Bg"], g.shape[0], c["Cin"])),
                      t["ubar"][:, :, None] * wu[None, None, :]])
    return _sum32(terms, order).reshape(c["Bg"], N[0], N[1], c["Cin"])


def _fwd32(c, t, order):
    h, (N1, N2) = _h32(c, t, order), c["N"]
    x0 = np.zeros((c["G"] * c["Bg"], c["C"], *c["P"]), np.float32)
    for g in range(c["G"]):
        w, b = t["w0"][g], t["b0"][g]
        terms = np.concatenate([np.broadcast_to(b, h.shape[:3] + (c["C"],))[None],
                                np.moveaxis(h[..., None, :] * w[None, None, None], -1, 0)])
        x0[g * c["Bg"]:(g + 1) * c["Bg"], :, :N1, :N2] = _sum32(terms, order).transpose(0, 3, 1, 2)
    return x0


def _din32(c, t, order):
    N1, N2 = c["N"]
    d = t["dx0"][:, :, :N1, :N2].reshape(c["G"], c["Bg"], c["C"], N1, N2)
    terms = d.transpose(0, 2, 1, 3, 4)[..., None] * t["w0"][:, :, None, None, None, :]     # (G, C, Bg, N1, N2, Cin)
    d_h = _sum32(terms.reshape(c["G"] * c["C"], c["Bg"], N1, N2, c["Cin"]), order)
    if not c["bag"]:
        return d_h
    wu = t["bw"][:, 2] * np.float32(c["bag"][1])
    return _sum32(np.moveaxis(d_h * wu, -1, 0), order).reshape(c["Bg"], N1 * N2)


def _w32(c, t, order):
    h, (N1, N2) = _h32(c, t, order), c["N"]
    out = []
    for g in range(c["G"]):
        d = t["dx0"][g * c["Bg"]:(g + 1) * c["Bg"], :, :N1, :N2].transpose(0, 2, 3, 1).reshape(-1, c["C"])
        hp = np.asarray(h).reshape(-1, c["Cin"])
        dw = _sum32(d[:, :, None] * hp[:, None, :], order)
        out.append(np.concatenate([dw.ravel(), _sum32(d, order)]))
    return np.stack(out)


def _conv32(c, t, order):
    Bg, C = c["Bg"], c["C"]
    f = _f32(gelu(t["x"])) if c["act"] else t["x"]
    out = []
    for g in range(c["G"]):
        d = t["dz"][g * Bg:(g + 1) * Bg].transpose(0, 2, 3, 1).reshape(-1, C)
        fp = f[g * Bg:(g + 1) * Bg].transpose(0, 2, 3, 1).reshape(-1, C)
        out.append(np.concatenate([_sum32(d[:, :, None] * fp[:, None, :], order).ravel(), _sum32(d, order)]))
    return np.stack(out)


def _mix32(c, t, mnsplit, order):
    """Float64 sums of each sample slice rounded to fp32, the slices then added in fp32."""
    G, Bg = c["G"], c["Bg"]
    X, Y = cplx(t["Xs"]), cplx(t["Gs"])
    ns = -(-Bg // mnsplit)
    parts = []
    for y in range(mnsplit):
        sel = np.concatenate([np.arange(g * Bg + y * ns, min(g * Bg + Bg, g * Bg + (y + 1) * ns)) for g in range(G)])
        if sel.size:
            p = lr.mix_wgrad(X[sel], Y[sel], G)
        else:
            p = np.zeros((G, X.shape[1], X.shape[3], X.shape[2], Y.shape[2]), np.complex128)
        parts.append(np.stack([_f32(p.real), _f32(p.imag)], -1))
    return _sum32(np.stack(parts), order)


def _report(label, ratios):
    print(label + ": fp32 worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= ROOM, (label, ratios)


# ------------------------------------------------------------------------------- float64 autograd
def _torch_lift(c, t):
    """(x0, d_in or d_ubar, [dW0 | db0] per group) by float64 torch autograd."""
    (N1, N2), (P1, P2), G, Bg = c["N"], c["P"], c["G"], c["Bg"]
    w0, b0 = _t(t["w0"]).requires_grad_(True), _t(t["b0"]).requires_grad_(True)
    if c["bag"]:
        # the adjoint's u scale is invLb: d ubar is the adjoint of fc0([grid, invLb ubar])
        ubar = _t(t["ubar"]).requires_grad_(True)
        grid, bw, bb = _t(t["grid"]), _t(t["bw"]), _t(t["bb"])
        feat = lambda s: torch.cat([grid[None].expand(Bg, -1, -1), (ubar * s)[..., None]], -1)
        inp = F.linear(feat(c["bag"][0]), bw, bb).view(Bg, N1, N2, -1)
        inp_b = F.linear(feat(c["bag"][1]), bw, bb).view(Bg, N1, N2, -1)
        leaf = ubar
    else:
        inp = inp_b = leaf = _t(t["inp"]).requires_grad_(True)
    pad = lambda h: torch.cat([F.pad(F.linear(h, w0[g], b0[g]).permute(0, 3, 1, 2), [0, P2 - N2, 0, P1 - N1])
                               for g in range(G)])
    x0, dx0 = pad(inp), _t(t["dx0"])
    gw, gb = torch.autograd.grad(x0, (w0, b0), dx0, retain_graph=True)
    gin, = torch.autograd.grad(pad(inp_b), leaf, dx0)
    return x0.detach().numpy(), gin.numpy(), torch.cat([gw.reshape(G, -1), gb], 1).numpy()


_AUTOGRAD = [c for c in lr.BWD_CASES if c["want_in"] and c["want_w"]][::3] + \
    [c for c in lr.BWD_CASES if c["bag"]] + [lr.BWD_CASES[-2], lr.BWD_CASES[-8]]


@pytest.mark.parametrize("c", _AUTOGRAD, ids=lr.bwd_id)
def test_lift_reference_equals_fp64_autograd(c):
    t = lr.lift_inputs(c)
    x0, gin, gw = _torch_lift(c, t)
    h, _ = lr.case_input64(c, t)
    N, P, G = c["N"], c["P"], c["G"]
    assert rel_l2(lr.lift_fwd(h, t["w0"], t["b0"], N, P, G), x0) <= 1e-12
    assert np.all(lr.lift_fwd(h, t["w0"], t["b0"], N, P, G)[:, :, N[0]:, :] == 0)
    d = lr.lift_bwd_in(t["dx0"], t["w0"], N, G)
    if c["bag"]:
        d = lr.bag_dubar(d, t["bw"], c["bag"][1])
    assert rel_l2(d, gin) <= 1e-12
    assert rel_l2(lr.lift_bwd_w(t["dx0"], h, N, G), gw) <= 1e-12


@pytest.mark.parametrize("c", lr.CONV_CASES[::5], ids=lr.conv_id)
def test_conv_reference_equals_fp64_autograd(c):
    t = lr.conv_inputs(c)
    C, G, Bg = c["C"], c["G"], c["Bg"]
    x, dz = _t(t["x"]), _t(t["dz"])
    f = F.gelu(x) if c["act"] else x
    ref = []
    for g in range(G):
        w = torch.zeros(C, C, 1, 1, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        gw, gb = torch.autograd.grad(F.conv2d(f[g * Bg:(g + 1) * Bg], w, b), (w, b), dz[g * Bg:(g + 1) * Bg])
        ref.append(torch.cat([gw.reshape(-1), gb]).numpy())
    assert rel_l2(lr.conv_wgrad_g(t["dz"], t["x"], c["act"], G), np.stack(ref)) <= 1e-12


def test_mix_reference_equals_fp64_autograd():
    c = next(c for c in lr.BWD_CASES if c["mix"])
    t = lr.lift_inputs(c)
    X, Y, G, Bg = cplx(t["Xs"]), cplx(t["Gs"]), c["G"], c["Bg"]
    K1, m2, C = c["mix"][0], c["mix"][1], c["C"]
    for g in range(G):
        W = torch.zeros(m2, K1, C, C, dtype=torch.complex128, requires_grad=True)
        out = torch.einsum("nkij,kjio->nkoj", torch.from_numpy(X[g * Bg:(g + 1) * Bg]), W)
        gW, = torch.autograd.grad(out, W, torch.from_numpy(Y[g * Bg:(g + 1) * Bg]))
        assert rel_l2(lr.mix_wgrad(X, Y, G)[g], gW.numpy()) <= 1e-12


# ------------------------------------------------------------------------------- fp32 inside the bounds
@pytest.mark.parametrize("c", lr.FWD_CASES, ids=lr.fwd_id)
def test_fp32_lift_forward_is_inside_the_bound(c):
    t = lr.lift_inputs(c)
    h, dh = lr.case_input64(c, t)
    a = (h, t["w0"], t["b0"], c["N"], c["P"], c["G"])
    ref, bound = lr.lift_fwd(*a), lr.lift_fwd_bound(*a, dh=dh)
    r = {}
    for order in ORDERS:
        if c["bag"]:
            r["h " + order] = lr.worst(np.abs(_h32(c, t, order) - h), dh)
        got = _fwd32(c, t, order)
        r["x0 " + order] = lr.worst(np.abs(got - ref), bound)
        if c["identity"]:
            assert np.array_equal(got[0, :2, :c["N"][0], :c["N"][1]], t["inp"][0].transpose(2, 0, 1))
    _report(lr.fwd_id(c), r)


@pytest.mark.parametrize("c", lr.BWD_CASES + [lr.CAP_LIFT_LDS, lr.CAP_LIFT_MFMA], ids=lr.bwd_id)
def test_fp32_lift_backward_is_inside_the_bound(c):
    t = lr.lift_inputs(c)
    h, dh = lr.case_input64(c, t)
    N, G = c["N"], c["G"]
    r = {}
    for order in ORDERS:
        if c["want_in"]:
            if c["bag"]:
                ref = lr.bag_dubar(lr.lift_bwd_in(t["dx0"], t["w0"], N, G), t["bw"], c["bag"][1])
                bound = lr.bag_dubar_bound(t["dx0"], t["w0"], N, G, t["bw"], c["bag"][1])
            else:
                ref, bound = lr.lift_bwd_in(t["dx0"], t["w0"], N, G), lr.lift_bwd_in_bound(t["dx0"], t["w0"], N, G)
            r["d_in " + order] = lr.worst(np.abs(_din32(c, t, order) - ref), bound)
        if c["want_w"]:
            r["dW0|db0 " + order] = lr.worst(np.abs(_w32(c, t, order) - lr.lift_bwd_w(t["dx0"], h, N, G)),
                                             lr.lift_bwd_w_bound(t["dx0"], h, N, G, dh=dh))
        if c["mix"]:
            X, Y = cplx(t["Xs"]), cplx(t["Gs"])
            ref = lr.mix_wgrad(X, Y, G)
            for ns in (1, 2, 5):
                b = lr.mix_wgrad_bound(X, Y, G, ns)[..., None]
                r[f"dWt ns{ns} " + order] = lr.worst(np.abs(_mix32(c, t, ns, order) - np.stack([ref.real, ref.imag], -1)),
                                                     np.broadcast_to(b, b.shape[:-1] + (2,)))
    _report(lr.bwd_id(c), r)


@pytest.mark.parametrize("c", lr.CONV_CASES + [lr.CAP_CONV], ids=lr.conv_id)
def test_fp32_conv_wgrad_is_inside_the_bound(c):
    t = lr.conv_inputs(c)
    if c["act"]:
        assert np.abs(t["x"]).max() <= 12.0
    ref, bound = lr.conv_wgrad_g(t["dz"], t["x"], c["act"], c["G"]), lr.conv_wgrad_g_bound(t["dz"], t["x"], c["act"], c["G"])
    _report(lr.conv_id(c), {order: lr.worst(np.abs(_conv32(c, t, order) - ref), bound) for order in ORDERS})


def test_bounds_are_zero_exactly_where_nothing_is_summed():
    """The padding of x0 and the gradient of a weight column whose input is identically zero."""
    c = lr.FWD_CASES[1]
    t = lr.lift_inputs(c)
    b = lr.lift_fwd_bound(t["inp"], t["w0"], t["b0"], c["N"], c["P"], c["G"])
    assert np.all(b[:, :, c["N"][0]:, :] == 0) and np.all(b[:, :, :, c["N"][1]:] == 0)
    assert np.all(b[:, :, :c["N"][0], :c["N"][1]] > 0)
    inp = t["inp"].copy()
    inp[..., 3] = 0
    bw = lr.lift_bwd_w_bound(t["dx0"], inp, c["N"], c["G"])[:, :c["C"] * c["Cin"]].reshape(c["G"], c["C"], c["Cin"])
    assert np.all(bw[:, :, 3] == 0) and np.all(np.delete(bw, 3, 2) > 0)


# ------------------------------------------------------------------------------- the case tables
def test_case_ids_cover_every_dispatch_branch():
    fwd = {lr.fwd_path(c) for c in lr.FWD_CASES}
    assert fwd == {"wide12x16", "pt16", "generic"}
    bwd = {lr.bwd_path(c) for c in lr.BWD_CASES}
    assert bwd == {"both1", "in_wide", "in_generic", "in_wide+lds", "mfma1", "mfma2", "lds"}
    conv = {lr.conv_path(c) for c in lr.CONV_CASES}
    assert conv == {f"mfma_act{a}_{v}" for a in (0, 1) for v in ("vec", "scalar")} | {"lds_act0", "lds_act1"}
    for ids in ([lr.fwd_id(c) for c in lr.FWD_CASES], [lr.bwd_id(c) for c in lr.BWD_CASES],
                [lr.conv_id(c) for c in lr.CONV_CASES]):
        assert len(set(ids)) == len(ids)
    # the fall-backs fall back for the reason their tag gives
    by = {c["tag"]: c for c in lr.FWD_CASES}
    assert lr.fwd_path(by["misaligned_c12_g2"]) == lr.fwd_path(by["c12_g5"]) == "pt16"
    assert lr.fwd_path(dict(by["misaligned_c12_g2"], mis_in=False)) == "wide12x16"


def test_merged_instantiation_2_is_unreachable():
    """lift_bwd_both_kernel<2> needs Cin + 1 > 16 and the wide input gradient, which needs Cin == 12."""
    for Cin in range(1, 40):
        for C in range(1, 20):
            c = lr._lcase("x", Cin, C, 2)
            assert lr.bwd_path(c) != "both2"
            assert (lr.bwd_path(c) == "both1") == (Cin == 12 and 5 <= C <= 16)


def test_cap_cases_exceed_the_nchunk_cap_by_little():
    for c, tiles in ((lr.CAP_LIFT_LDS, 1052), (lr.CAP_LIFT_MFMA, 1050)):
        assert -(-c["Bg"] * c["N"][0] * c["N"][1] // lr.TP) == tiles > lr.NCHUNK_CAP == lr.lift_bwd_nchunk(c["Bg"], c["N"])
    c = lr.CAP_CONV
    assert c["Bg"] * -(-c["P"][0] * c["P"][1] // lr.TP) == 1055 > lr.NCHUNK_CAP == lr.conv_wgrad_nchunk(c["Bg"], c["P"])
    assert lr.bwd_path(lr.CAP_LIFT_LDS) == "lds" and lr.bwd_path(lr.CAP_LIFT_MFMA) == "mfma1"
    assert lr.conv_path(lr.CAP_CONV) == "mfma_act0_vec"
