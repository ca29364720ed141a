"""The column pass folded into the row kernels (csrc/colspec.h; ops.COLSPEC) against the fused
column pass it replaces (blindno_colpass between the row kernels) on the same inputs, and the
snapshot encoder through it against the one through the column pass.  The folded path forms the
same sums in a different order, so the bars are fp32-rounding ones: 1e-6 on spectra and fields,
1e-5 on parameter gradients (SURVEY 8c's 1e-5 / 1e-4 against fp64 are checked by the config
tests, which take this path by default)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _grid(N):
    gx, gy = np.meshgrid(np.linspace(-1, 1, N, dtype=np.float32), np.linspace(-1, 1, N, dtype=np.float32),
                         indexing="ij")
    return torch.tensor(np.stack([gx, gy], 2)).cuda()


def _layer(Bn, N, seed):
    from blindno import ops
    C, m = 4, 12
    P = N + ops.pad_amount(N)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(Bn, C, P, P, device="cuda", generator=g)
    w1 = torch.randn(C, C, m, m, 2, device="cuda", generator=g) / (C * C)
    w2 = torch.randn(C, C, m, m, 2, device="cuda", generator=g) / (C * C)
    cw = torch.randn(C, C, device="cuda", generator=g) / C
    cb = torch.randn(C, device="cuda", generator=g)
    Wt = ops.pack_weights((w1, w2), P, 2)
    return x, Wt, cw, cb, C, m, P


@pytest.mark.parametrize("Bn,N,act", [(6, 128, 1), (3, 128, 0), (2, 256, 1)])
def test_rowdft_cd_colmix_matches_colpass(Bn, N, act):
    """blindno_rowdft_cd (row DFT + per-block column-DFT partials) + blindno_colmix (block sum,
    Xs, mix) vs blindno_rowdft + blindno_colpass: the saved spectrum Xs in both directions, and
    the forward row inverse from the mixed spectrum (ZY) vs from the column pass's Z."""
    from blindno import ops
    from blindno._lib import call, ptr, stream_ptr
    x, Wt, cw, cb, C, m, P = _layer(Bn, N, 11 + N)
    assert ops.colspec_ok(Bn, C, P, P, m, m)
    cs = ops._ColSpec(Bn, C, P, P, m, m, x.device)
    part = cs.part(C, x)
    call("blindno_rowdft_cd", ptr(x), ptr(part), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, m, act, P, P, stream_ptr())
    At = ops.k_rowdft(x, Bn, C, P, P, m, act)
    for direction in (0, 1):
        Xs_cs, Y = cs.mix(part, cs.nb, Wt, direction)
        Xs_ref, Z = ops.k_colpass(At, Wt, Bn, C, C, P, m, m, P, direction)
        torch.cuda.synchronize()
        e = rel_l2(Xs_cs.cpu().numpy(), Xs_ref.cpu().numpy())
        print(f"Bn={Bn} N={N} act={act} dir={direction}: Xs {e:.2e}")
        assert e <= 1e-6, e
        if direction == 0:
            z_cs = torch.empty_like(x)
            call("blindno_rowidft_epi_zc", ptr(Y), ptr(x), ptr(cw), ptr(cb), ptr(z_cs), ptr(cs.tb), ptr(cs.tab),
                 None, None, Bn, C, P, P, m, m, act, 0, P, P, stream_ptr())
            z_ref = ops.k_rowidft_epi(Z, x, cw, cb, Bn, C, P, P, m, act)
            torch.cuda.synchronize()
            ez = rel_l2(z_cs.cpu().numpy(), z_ref.cpu().numpy())
            print(f"   row inverse from Y vs from Z: {ez:.2e}")
            assert ez <= 1e-6, ez


@pytest.mark.parametrize("Bn,N", [(5, 128), (2, 256)])
def test_chained_layer_cd_matches_rowdft(Bn, N):
    """The chained layer as bench.py's roofline_spectral times it: row inverse from Y with the
    next row DFT's column-DFT partials in the same pass (blindno_rowidft_epi_zc with part) vs the
    separate row DFT of the field it wrote (blindno_rowdft_cd of GELU(z)); fields identical."""
    from blindno import ops
    from blindno._lib import call, ptr, stream_ptr
    x, Wt, cw, cb, C, m, P = _layer(Bn, N, 5 + N)
    cs = ops._ColSpec(Bn, C, P, P, m, m, x.device)
    p0 = cs.part(C, x)
    call("blindno_rowdft_cd", ptr(x), ptr(p0), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, m, 1, P, P, stream_ptr())
    _, Y = cs.mix(p0, cs.nb, Wt, 0)
    z = torch.empty_like(x)
    p1 = cs.part(C, x)
    call("blindno_rowidft_epi_zc", ptr(Y), ptr(x), ptr(cw), ptr(cb), ptr(z), ptr(cs.tb), ptr(cs.tab), ptr(p1),
         ptr(cs.Tp), Bn, C, P, P, m, m, 1, 1, P, P, stream_ptr())
    z2 = torch.empty_like(x)
    call("blindno_rowidft_epi_zc", ptr(Y), ptr(x), ptr(cw), ptr(cb), ptr(z2), ptr(cs.tb), ptr(cs.tab), None,
         None, Bn, C, P, P, m, m, 1, 0, P, P, stream_ptr())
    p2 = cs.part(C, x)
    call("blindno_rowdft_cd", ptr(z), ptr(p2), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, m, 1, P, P, stream_ptr())
    X1, _ = cs.mix(p1, cs.nb, Wt, 0)
    X2, _ = cs.mix(p2, cs.nb, Wt, 0)
    torch.cuda.synchronize()
    assert torch.equal(z, z2)
    e = rel_l2(X1.cpu().numpy(), X2.cpu().numpy())
    print(f"Bn={Bn} N={N}: next layer's spectrum in-pass vs separate {e:.2e}")
    assert e <= 1e-6, e


# ------------------------------------------------------------------ dz = lw_l ghat v formed on load
def _bag_dz_setup(crop, weighted):
    """The smallest folded-pass geometry (C 4, m 12, P 32; B 2 bags of U 3 snapshots): v from
    blindno_project_bag_fwd, dz = lw ghat v written by blindno_project_bag_bwd."""
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    B, U, C, m, P = 2, 3, 4, 12, 32
    Ho, Wo = crop
    Bn = B * U
    assert query("blindno_colspec_ok", Bn, C, P, P, m, m) == 1
    assert query("blindno_colspec_ok", Bn, C, 16, 32, m, m) == 0          # nothing smaller is accepted
    g = torch.Generator(device="cuda").manual_seed(300 + Wo)
    r = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale
    z, w1, b1, w2, b2 = r(Bn, C, P, P), r(128, C, scale=0.4), r(128, scale=0.1), r(1, 128, scale=0.1), r(1)
    ghat = r(B, Ho * Wo)
    lw = None
    if weighted:
        lw = torch.tensor([2.0, 1.0, 3.0], device="cuda") / 6.0
    ubar = torch.empty(B, Ho * Wo, device="cuda")
    stats = torch.empty(query("blindno_project_bag_stats_floats", B, Ho, Wo), device="cuda")
    v = torch.full_like(z, float("nan"))
    call("blindno_project_bag_fwd", ptr(z), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(lw), ptr(ubar), ptr(stats),
         ptr(v), B, U, C, P, P, Ho, Wo, 128, stream_ptr())
    dz = torch.full_like(z, float("nan"))                                 # never read outside the crop
    partial = torch.empty(3, 128 * C + 257, device="cuda")
    call("blindno_project_bag_bwd", ptr(stats), ptr(ghat), ptr(w2), ptr(lw), ptr(v), ptr(dz), ptr(partial), 3, B, U,
         C, P, P, Ho, Wo, 128, stream_ptr())
    cs = ops._ColSpec(Bn, C, P, P, m, m, z.device)
    return cs, v, dz, ghat, lw, (B, U, C, m, P, Bn)


@pytest.mark.parametrize("weighted", [False, True], ids=["lw_null", "lw_given"])
@pytest.mark.parametrize("crop", [(23, 29), (23, 28)], ids=["wo29", "wo28_float4"])
def test_rowdft_cd_bag_matches_rowdft_cd_of_dz(crop, weighted):
    """blindno_rowdft_cd_bag(v, ghat, lw) vs blindno_rowdft_cd(dz, act 0, Ho, Wo): both form
    fl(fl(lw ghat) v) before the same accumulation, so the partials are bit-identical."""
    from blindno._lib import call, ptr, stream_ptr
    cs, v, dz, ghat, lw, (B, U, C, m, P, Bn) = _bag_dz_setup(crop, weighted)
    pa, pb = (torch.full_like(cs.part(C, v), -12345.678) for _ in range(2))
    call("blindno_rowdft_cd", ptr(dz), ptr(pa), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, m, 0, crop[0], crop[1],
         stream_ptr())
    call("blindno_rowdft_cd_bag", ptr(v), ptr(ghat), ptr(lw), U, ptr(pb), ptr(cs.Tp), ptr(cs.tab), Bn, C, P, P, m,
         crop[0], crop[1], stream_ptr())
    torch.cuda.synchronize()
    assert torch.isfinite(pa).all() and bool((pa != -12345.678).any())
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("weighted", [False, True], ids=["lw_null", "lw_given"])
@pytest.mark.parametrize("crop", [(23, 29), (23, 28)], ids=["wo29", "wo28_float4"])
def test_rowidft_bwd_zc_bag_matches_rowidft_bwd_zc_of_dz(crop, weighted):
    """blindno_rowidft_bwd_zc_bag(Yb, v, ghat, lw) vs blindno_rowidft_bwd_zc(Yb, dz, act 1, Ho, Wo)
    (they may take different instantiations): dx and the column-DFT partials to 1e-6 rel-L2, the
    reduced dWc | dbc to 1e-5; dx also per element against spectral_stage_ref.row_inv_adj on
    Z[n,h,k,c] = sum_j Yb[n,k,c,j] e^{+2 pi i r_j h / P1} under that file's bound with the chain
    n = K1 (column inverse) + 2 m2 (row inverse) + C (conv) + 1 (the GELU' product)."""
    import spectral_stage_ref as sr
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    cs, v, dz, ghat, lw, (B, U, C, m, P, Bn) = _bag_dz_setup(crop, weighted)
    g = torch.Generator(device="cuda").manual_seed(17)
    Yb = torch.randn(Bn, m, C, cs.K1, 2, device="cuda", generator=g) * 0.1
    cw = torch.randn(C, C, device="cuda", generator=g) / C
    xsrc = torch.randn(Bn, C, P, P, device="cuda", generator=g)
    nchunk = query("blindno_colspec_bwd_nchunk", Bn, P)
    if crop[1] % 4:
        # the folded adjoint runs in the transposed kernel only, whose field accesses are whole
        # float4s: both entries refuse the width on the host and write nothing (before the refusal
        # blindno_rowidft_bwd_zc went on to the general row inverse with Z == NULL)
        from blindno._lib import load
        dx = torch.full((Bn * C * P * P + 128,), -12345.678, device="cuda")
        part = torch.zeros_like(cs.part(C, v))
        pw = torch.zeros(nchunk, C * C + C, device="cuda")
        tail = (ptr(cw), ptr(xsrc), ptr(dx[64:]), ptr(cs.tb), ptr(cs.tab), ptr(part), ptr(cs.Tp), ptr(pw), Bn, C, P, P,
                m, m, 1, crop[0], crop[1], stream_ptr())
        assert int(load().blindno_rowidft_bwd_zc(ptr(Yb), ptr(dz), *tail)) == 1
        assert int(load().blindno_rowidft_bwd_zc_bag(ptr(Yb), ptr(v), ptr(ghat), ptr(lw), U, *tail)) == 1
        torch.cuda.synchronize()
        assert bool((dx == -12345.678).all()) and not part.any() and not pw.any()
        return
    res = []
    for bag in (False, True):
        dx = torch.full((Bn, C, P, P), float("nan"), device="cuda")
        part = torch.zeros_like(cs.part(C, v))
        pw = torch.full((nchunk, C * C + C), float("nan"), device="cuda")
        tail = (ptr(cw), ptr(xsrc), ptr(dx), ptr(cs.tb), ptr(cs.tab), ptr(part), ptr(cs.Tp), ptr(pw), Bn, C, P, P, m,
                m, 1, crop[0], crop[1], stream_ptr())
        if bag:
            call("blindno_rowidft_bwd_zc_bag", ptr(Yb), ptr(v), ptr(ghat), ptr(lw), U, *tail)
        else:
            call("blindno_rowidft_bwd_zc", ptr(Yb), ptr(dz), *tail)
        gw = ops.reduce_partials(pw, nchunk, C * C + C)
        torch.cuda.synchronize()
        res.append((dx.cpu().numpy(), part.cpu().numpy(), gw.cpu().numpy()))
    (dx0, p0, g0), (dx1, p1, g1) = res
    e = (rel_l2(dx1, dx0), rel_l2(p1, p0), rel_l2(g1, g0))
    print(f"crop={crop} weighted={weighted}: dx {e[0]:.2e}, partials {e[1]:.2e}, dWc|dbc {e[2]:.2e}")
    assert np.isfinite(dx1).all() and e[0] <= 1e-6 and e[1] <= 1e-6 and e[2] <= 1e-5, e
    # per element against float64
    Y = sr.cplx(Yb.cpu().numpy())
    F = sr._phase(np.arange(P), sr.kept_rows(m, P), P, -1.0)
    G = np.einsum("nkcj,hj->nhkc", Y, np.conj(F), optimize=True)
    Gabs = np.repeat(np.abs(Y).sum(-1).transpose(0, 1, 2)[:, None], P, 1)            # (Bn, P1, m2, C)
    dzn, wc, xs = dz.cpu().numpy().astype(np.float64), cw.cpu().numpy().astype(np.float64), xsrc.cpu().numpy()
    ref = sr.row_inv_adj(G, P, dzn, wc, xs, 1, crop)
    S, gwt = sr.row_inv_adj_abs(None, P, dzn, wc, xs, 1, crop, bare=sr.row_inv_bare_abs(Gabs, P))
    bound = (cs.K1 + 2 * m + C + 1 + 8) * sr.U24 * S + sr.GELU_ABS * gwt
    for name, dx in (("zc", dx0), ("zc_bag", dx1)):
        r = sr.worst(np.abs(dx.astype(np.float64) - ref), bound)
        print(f"   dx ({name}) vs float64: worst err/bound {r:.3f}")
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize("N,B,dedup", [(128, 2, True), (128, 3, False), (256, 1, True)])
def test_encoder_colspec_matches_colpass(N, B, dedup):
    """NIOFP2D_FNO's snapshot encoder (ops.BagEncoderFn, 2 layers, modes 12, width 4) with the
    folded column pass vs with the column pass: output and every FNO_input gradient."""
    from blindno import NIOFP2D_FNO, nio, ops
    torch.manual_seed(21)
    m = NIOFP2D_FNO(2, 3, 100, 25, 2, 8, 6, 2).cuda().train()
    x = torch.randn(B, 80, N, N, device="cuda")
    grid = _grid(N)
    idx = np.random.RandomState(4).choice(80, 61)
    P = N + ops.pad_amount(N)
    assert ops.colspec_ok(B * 61, 4, P, P, 12, 12)
    res = []
    for on in (True, False):
        ops.COLSPEC = on
        nio.DEDUP_BAGS = dedup
        try:
            m.zero_grad()
            out = m(x, grid, bag_idx=idx)
            (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
            torch.cuda.synchronize()
            res.append((out.detach().cpu().numpy(),
                        {k: p.grad.cpu().numpy() for k, p in m.FNO_input.named_parameters()}))
        finally:
            ops.COLSPEC = True
            nio.DEDUP_BAGS = True
    e_out = rel_l2(res[0][0], res[1][0])
    e_g = {k: rel_l2(res[0][1][k], res[1][1][k]) for k in res[1][1]}
    worst = max(e_g, key=e_g.get)
    print(f"N={N} B={B} dedup={dedup}: out {e_out:.2e}, worst grad {worst} {e_g[worst]:.2e}")
    assert e_out <= 1e-6, e_out
    assert e_g[worst] <= 1e-5, (worst, e_g[worst])
