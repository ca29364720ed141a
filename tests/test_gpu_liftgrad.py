"""The bag encoder's first-layer gradients from spectra and moments (ops.LIFTGRAD_SPEC; DESIGN
section 4; the identity itself: tests/test_liftgrad_identity.py) on the 128^2 grid (P = 160, the
geometry the encoder runs at; C 4, modes 12) with B = 1 bag of U = 3 and B = 2 bags of U = 5
distinct snapshots, unequal multiplicity weights.

Bars: per-tensor rel-L2 <= 1e-4 for gradients against float64; the path
against path comparison under tests/test_gpu_colspec.py's fp32 rounding bars (1e-6 output, 1e-5
gradients).
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

C, M12, N, P = 4, 12, 128, 160
CASES = [(1, 3, (1.0, 2.0, 4.0)), (2, 5, (1.0, 2.0, 4.0, 1.0, 3.0))]
NP = C * C + C + 4 * C


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import blindno
    blindno.load_library()


def _grid():
    gx, gy = np.meshgrid(np.linspace(-1, 1, N, dtype=np.float32),
                         np.linspace(-1, 1, N, dtype=np.float32), indexing="ij")
    return torch.tensor(np.stack([gx, gy], 2), device="cuda")


def _inputs(X, idx, grid, B, U):
    """in = (u, gx, gy, 1) on the crop, float64 (Bn, 4, N, N)."""
    u = X[:, idx.long()].reshape(B * U, N, N).double().cpu()
    g = grid.double().cpu()
    one = torch.ones(N, N, dtype=torch.float64)
    return torch.stack([u, g[..., 0].expand_as(u), g[..., 1].expand_as(u), one.expand_as(u)], 1)


@pytest.mark.parametrize("bag", [True, False], ids=["zc_bag_m", "zc_m"])
@pytest.mark.parametrize("B,U,mult", CASES, ids=["B1U3", "B2U5"])
def test_adjoint_moments_and_optional_dx(B, U, mult, bag):
    """(a) blindno_rowidft_bwd_zc_bag_m (dz = lw ghat v formed on load) and blindno_rowidft_bwd_zc_m
    (dz read as a field on its crop): the moments M and dx against float64 on the same inputs;
    (b) dx == NULL leaves every partial column (and the column-DFT partials) bit-identical."""
    import spectral_stage_ref as sr
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    Bn, T = B * U, 7
    g = torch.Generator(device="cuda").manual_seed(40 + U)
    r = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale
    v, ghat = r(Bn, C, P, P), r(B, N * N)
    lw = torch.tensor(mult, device="cuda") / sum(mult)
    Yb, cw, xsrc = r(Bn, M12, C, 24, 2, scale=0.1), r(C, C) / C, r(Bn, C, P, P)
    X, grid = r(B, T, N, N), _grid()
    idx = torch.tensor([5, 0, 3, 6, 2][:U], device="cuda", dtype=torch.int32)
    cs = ops._ColSpec(Bn, C, P, P, M12, M12, v.device)
    nchunk = query("blindno_colspec_bwd_nchunk", Bn, P)
    # the field form reads dz = fl(fl(lw ghat) v) on the crop only (NaN elsewhere: never read)
    sc32 = (lw.repeat(B)[:, None] * ghat.repeat_interleave(U, 0)).view(Bn, 1, N, N)
    dzf = torch.full((Bn, C, P, P), float("nan"), device="cuda")
    dzf[:, :, :N, :N] = sc32 * v[:, :, :N, :N]
    res = []
    for with_dx in (True, False):
        dx = torch.full((Bn, C, P, P), float("nan"), device="cuda") if with_dx else None
        part = torch.zeros_like(cs.part(C, v))
        pw = torch.full((nchunk, NP), float("nan"), device="cuda")
        tail = (ptr(cs.tb), ptr(cs.tab), ptr(part), ptr(cs.Tp), ptr(pw), ptr(X), ptr(idx), ptr(grid), B, T, U, N, N, C,
                P, P, M12, M12, 1, N, N, stream_ptr())
        if bag:
            call("blindno_rowidft_bwd_zc_bag_m", ptr(Yb), ptr(v), ptr(ghat), ptr(lw), ptr(cw), ptr(xsrc), ptr(dx), *tail)
        else:
            call("blindno_rowidft_bwd_zc_m", ptr(Yb), ptr(dzf), ptr(cw), ptr(xsrc), ptr(dx), *tail)
        torch.cuda.synchronize()
        res.append((dx, part, pw))
    (dx, part1, pw1), (_, part0, pw0) = res
    assert torch.isfinite(pw1).all() and torch.isfinite(dx).all()
    assert torch.equal(pw1, pw0) and torch.equal(part1, part0)
    # float64: dz = lw ghat v on the crop, dx = GELU'(xsrc) (row inverse adjoint + Wc^T dz)
    dz = torch.zeros(Bn, C, P, P, dtype=torch.float64)
    sc = (lw.double().cpu().repeat(B)[:, None] * ghat.double().cpu().repeat_interleave(U, 0)).view(Bn, 1, N, N)
    dz[:, :, :N, :N] = sc * v.double().cpu()[:, :, :N, :N]
    Y = sr.cplx(Yb.cpu().numpy())
    F = sr._phase(np.arange(P), sr.kept_rows(M12, P), P, -1.0)
    G = np.einsum("nkcj,hj->nhkc", Y, np.conj(F), optimize=True)
    ref = sr.row_inv_adj(G, P, dz.numpy(), cw.cpu().numpy().astype(np.float64), xsrc.cpu().numpy(), 1, (N, N))
    Mref = np.einsum("nohw,njhw->oj", ref[:, :, :N, :N], _inputs(X, idx, grid, B, U).numpy())
    Mgot = pw1[:, C * C + C:].double().sum(0).view(C, 4).cpu().numpy()
    e_dx, e_m = rel_l2(dx.cpu().numpy(), ref), rel_l2(Mgot, Mref)
    print(f"B={B} U={U} bag={bag}: dx vs float64 {e_dx:.2e}, M vs float64 {e_m:.2e}")
    assert e_dx <= 1e-4 and e_m <= 1e-4, (e_dx, e_m)
    # the 1x1-conv gradient columns are those of the entry without the moments
    pw2 = torch.empty(nchunk, C * C + C, device="cuda")
    call("blindno_rowidft_bwd_zc_bag", ptr(Yb), ptr(v), ptr(ghat), ptr(lw), U, ptr(cw), ptr(xsrc), ptr(dx),
         ptr(cs.tb), ptr(cs.tab), ptr(torch.zeros_like(part1)), ptr(cs.Tp), ptr(pw2), Bn, C, P, P, M12, M12, 1, N, N,
         stream_ptr())
    torch.cuda.synchronize()
    e_w = rel_l2(pw1[:, :C * C + C].double().sum(0).cpu().numpy(), pw2.double().sum(0).cpu().numpy())
    assert e_w <= 1e-5, e_w


def _layer0_fp64(inp, A, w1, w2, wc, bc):
    """Layer 0 restated with torch.fft (float64): z0 (Bn, C, P, P) from in (Bn, 4, N, N)."""
    pad = (0, P - N, 0, P - N)
    x0 = torch.nn.functional.pad(torch.einsum("cj,njhw->nchw", A, inp), pad)
    xf = torch.fft.rfft2(x0)
    of = torch.zeros(x0.shape[0], C, P, P // 2 + 1, dtype=torch.complex128)
    of[:, :, :M12, :M12] = torch.einsum("nckl,cokl->nokl", xf[:, :, :M12, :M12], w1)
    of[:, :, -M12:, :M12] = torch.einsum("nckl,cokl->nokl", xf[:, :, -M12:, :M12], w2)
    return torch.fft.irfft2(of, s=(P, P)) + torch.einsum("oc,nchw->nohw", wc, x0) + bc[None, :, None, None]


@pytest.mark.parametrize("hosted", [False, True], ids=["alone", "hosting"])
@pytest.mark.parametrize("B,U,mult", CASES, ids=["B1U3", "B2U5"])
def test_liftgrad_spec_matches_fp64_autograd(B, U, mult, hosted):
    """(c) blindno_liftgrad_spec's five outputs -- the spectral weights' gradient (both halves),
    the 1x1 conv's weight and bias, fc0's weight and bias -- against float64 autograd of the
    restated layer, for a random dz0 whose spectrum and moments the project's kernels form.
    ``hosted``: the launch also hosts one spectral weight-gradient job (the second layer's in the
    encoder), whose partials must equal blindno_mix_wgrad_part's (blindno_mix_wgrad's when the samples are
    not split) bit for bit."""
    import ctypes
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    Bn, T = B * U, 7
    g = torch.Generator(device="cuda").manual_seed(60 + U)
    r = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale
    lw = torch.tensor(mult, device="cuda").repeat(B) / sum(mult)
    dz0 = r(Bn, C, P, P) * lw[:, None, None, None]
    X, grid = r(B, T, N, N), _grid()
    idx = torch.tensor([5, 0, 3, 6, 2][:U], device="cuda", dtype=torch.int32)
    fc0w, fc0b, cw, cb = r(C, 3), r(C), r(C, C) / C, r(C)
    w1, w2 = r(C, C, M12, M12, 2, scale=0.25), r(C, C, M12, M12, 2, scale=0.25)
    cs = ops._ColSpec(Bn, C, P, P, M12, M12, X.device)
    Wt = ops.k_pack_w2d(w1, w2, P)
    Dg2 = ops._grid_spec2(grid, N, N, P, P, M12, M12)
    # U: the forward's first stage; G: the adjoint spectrum of dz0
    part = cs.part(1, X)
    call("blindno_rowdft_bag_lift_cd", ptr(X), ptr(idx), ptr(part), ptr(cs.Tp), ptr(cs.tab), B, T, U, N, N, P, P,
         M12, stream_ptr())
    U0 = torch.empty(Bn, M12, cs.K1, 2, device="cuda")
    cs.mix(part, (N + 15) // 16, Wt, 0, Cp=1, lift=(fc0w, fc0b, Dg2), usave=U0)
    part = cs.part(C, X)
    call("blindno_rowdft_cd", ptr(dz0), ptr(part), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, M12, 0, P, P, stream_ptr())
    G, _ = cs.mix(part, P // 16, Wt, 1)
    inp = _inputs(X, idx, grid, B, U)
    Mm = torch.einsum("nohw,njhw->oj", dz0.double().cpu()[:, :, :N, :N], inp)
    pw = torch.zeros(2, NP, device="cuda")                      # two partial rows of moments
    pw[0, C * C + C:] = (0.25 * Mm).reshape(-1).float().cuda()
    pw[1, C * C + C:] = (0.75 * Mm).reshape(-1).float().cuda()
    ns = query("blindno_mix_wgrad_nsplit", Bn, C, C, cs.K1, M12)
    nel = M12 * cs.K1 * C * C * 2
    rows = query("blindno_liftgrad_rows", C, M12, ns, 2)
    dWp = torch.full((ns, nel), float("nan"), device="cuda")
    pl = torch.full((rows, NP), float("nan"), device="cuda")
    jobs = (None, None, None, None, 0)
    if hosted:
        hX, hG = r(Bn, M12, C, cs.K1, 2), r(Bn, M12, C, cs.K1, 2)
        hout = torch.full((ns, nel), float("nan"), device="cuda")
        href = torch.full((ns, nel), float("nan"), device="cuda")
        if ns > 1:
            call("blindno_mix_wgrad_part", ptr(hX), ptr(hG), ptr(href), ns, 1, Bn, C, C, cs.K1, M12, stream_ptr())
        else:           # no sample split: the partial is the gradient itself
            call("blindno_mix_wgrad", ptr(hX), ptr(hG), ptr(href), None, 1, Bn, C, C, cs.K1, M12, stream_ptr())
        jobs = ((ctypes.c_void_p * 1)(hX.data_ptr()), (ctypes.c_void_p * 1)(hG.data_ptr()),
                (ctypes.c_void_p * 1)(hout.data_ptr()), (ctypes.c_int * 7)(Bn, C, C, cs.K1, M12, ns, 1), 1)
    call("blindno_liftgrad_spec", ptr(G), ptr(U0), ptr(Wt), ptr(Dg2), ptr(fc0w), ptr(fc0b), ptr(cw), ptr(pw), 2, NP,
         C * C + C, ptr(dWp), ptr(pl), Bn, C, P, P, M12, M12, ns, *jobs, stream_ptr())
    if hosted:
        torch.cuda.synchronize()
        assert torch.isfinite(hout).all() and torch.equal(hout, href)
    dWt = ops.reduce_partials(dWp, ns, nel).view(M12, cs.K1, C, C, 2)
    d1, d2 = ops.unpack_weights(dWt, (w1, w2), P, 2)
    gsm = ops.reduce_partials(pl, rows, NP)
    torch.cuda.synchronize()
    got = {"weights1": d1, "weights2": d2, "conv.weight": gsm[:C * C].view(C, C), "conv.bias": gsm[C * C:C * C + C],
           "fc0.weight": gsm[C * C + C:C * C + 4 * C].view(C, 3), "fc0.bias": gsm[C * C + 4 * C:]}
    # float64 autograd of L = <z0, dz0>
    leaf = lambda t: t.detach().double().cpu().requires_grad_(True)
    pf, pb, pc, pcb = leaf(fc0w), leaf(fc0b), leaf(cw), leaf(cb)
    p1 = torch.view_as_complex(w1.double().cpu().contiguous()).requires_grad_(True)
    p2 = torch.view_as_complex(w2.double().cpu().contiguous()).requires_grad_(True)
    z0 = _layer0_fp64(inp, torch.cat([pf, pb[:, None]], 1), p1, p2, pc, pcb)
    (z0 * dz0.double().cpu()).sum().backward()
    ref = {"weights1": torch.view_as_real(p1.grad), "weights2": torch.view_as_real(p2.grad), "conv.weight": pc.grad,
           "conv.bias": pcb.grad, "fc0.weight": pf.grad, "fc0.bias": pb.grad}
    errs = {k: rel_l2(got[k].cpu().numpy(), ref[k].numpy()) for k in ref}
    print(f"B={B} U={U}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(np.isfinite(got[k].cpu().numpy()).all() for k in got)
    assert max(errs.values()) <= 1e-4, errs


def _encoder_case(B, U, mult):
    idx = np.concatenate([np.full(int(c), s) for s, c in zip([11, 3, 40, 7, 25][:U], mult)]).astype(np.int64)
    return idx


class _Count:
    def __init__(self):
        self.n = 0

    def before(self, args):
        self.n += 1

    def after(self, args):
        pass


@pytest.mark.parametrize("bag_stats", [True, False], ids=["bag_level", "per_snapshot"])
@pytest.mark.parametrize("B,U,mult", CASES, ids=["B1U3", "B2U5"])
def test_encoder_backward_flag_on_off_and_fp64(B, U, mult, bag_stats, monkeypatch):
    """(d) NIOFP2D_FNO's step with ops.LIFTGRAD_SPEC on against off (output bit-identical,
    every FNO_input gradient to 1e-5), and both against the float64 oracle (1e-4); with the
    bag-level projection (dz formed on load: blindno_rowidft_bwd_zc_bag_m) and with the per-snapshot
    one (ops.BAG_STATS off: dz a field, blindno_rowidft_bwd_zc_m).  The launches are counted, so a
    flag that silently took the other path fails."""
    import blindno
    import oracle
    from blindno import NIOFP2D_FNO, _lib, ops
    monkeypatch.setattr(ops, "BAG_STATS", bag_stats)
    adj = "blindno_rowidft_bwd_zc_bag_m" if bag_stats else "blindno_rowidft_bwd_zc_m"
    counts = {k: _Count() for k in ("blindno_liftgrad_spec", adj, "blindno_rowidft_bwd_lift_zc_mix")}
    for k, h in counts.items():
        monkeypatch.setitem(_lib._HOOKS, k, h)
    torch.manual_seed(33)
    m = NIOFP2D_FNO(2, 3, 100, 25, 2, 8, 6, 2).cuda().train()
    T = 48
    x = torch.randn(B, T, N, N, device="cuda")
    y = torch.randn(B, N, N, 2, device="cuda")
    grid = _grid()
    idx = _encoder_case(B, U, mult)
    assert ops.colspec_ok(B * U, C, P, P, M12, M12)
    res = []
    for on in (True, False):
        ops.LIFTGRAD_SPEC = on
        try:
            m.zero_grad()
            out = m(x, grid, bag_idx=idx)
            blindno.mse_loss(out, y).backward()
            torch.cuda.synchronize()
            res.append((out.detach().cpu().numpy(),
                        {k: p.grad.cpu().numpy() for k, p in m.FNO_input.named_parameters()}))
            if on:      # the new launches ran, the old one did not
                assert [counts[k].n for k in ("blindno_liftgrad_spec", adj, "blindno_rowidft_bwd_lift_zc_mix")] \
                    == [1, 1, 0]
        finally:
            ops.LIFTGRAD_SPEC = True
    assert [c.n for c in counts.values()] == [1, 1, 1]
    with torch.no_grad():       # no backward follows: the spectrum is not saved, the output is the same
        assert np.array_equal(m(x, grid, bag_idx=idx).cpu().numpy(), res[0][0])
    assert np.array_equal(res[0][0], res[1][0])
    e_g = {k: rel_l2(res[0][1][k], res[1][1][k]) for k in res[1][1]}
    worst = max(e_g, key=e_g.get)
    print(f"B={B} U={U}: on vs off, worst grad {worst} {e_g[worst]:.2e}")
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()
         if not k.startswith("branch.")}
    ref = oracle.niofp2d_fno(p, x.cpu(), grid.cpu(), idx=idx.tolist())
    oracle.mse(ref, y.cpu()).backward()
    e_o = {k: rel_l2(res[0][1][k], p["FNO_input." + k].grad.numpy()) for k in res[0][1]}
    wo = max(e_o, key=e_o.get)
    print(f"B={B} U={U}: on vs float64, worst grad {wo} {e_o[wo]:.2e}")
    assert e_g[worst] <= 1e-5, (worst, e_g[worst])
    assert e_o[wo] <= 1e-4, (wo, e_o[wo])


def test_graph_replays_bit_identical():
    """(e) two consecutive replays of the graphed step on the same inputs: bit-identical flat
    gradient (the moments and the spectral sums are reduced in fixed order, no float atomics)."""
    import blindno
    from blindno import NIOFP2D_FNO
    from blindno.train import DataParallel, FlatAdam, GraphedBagStep, trained_parameters
    torch.manual_seed(34)
    m = NIOFP2D_FNO(2, 3, 100, 25, 2, 8, 6, 2).cuda().train()
    B, T = 2, 48
    x = torch.randn(B, T, N, N, device="cuda")
    y = torch.randn(B, N, N, 2, device="cuda")
    opt = FlatAdam(trained_parameters(m, exclude_prefixes=("branch.", "fc0.")), lr=1e-3)
    gs = GraphedBagStep(m, blindno.mse_loss, opt, DataParallel(opt), x, y, _grid())
    idx = _encoder_case(2, 5, CASES[1][2])
    gs.replay(idx)
    torch.cuda.synchronize()
    g0 = opt.grad.clone()
    gs.replay(idx)
    torch.cuda.synchronize()
    assert torch.isfinite(g0).all() and bool(g0.any())
    assert torch.equal(g0, opt.grad)
