"""The 3D Fourier layer on the HIP device: SpectralConv3d / FNO3d against the reference's golden
vectors, blindno_colpass3d / lift3d / project3d on their own against float64, determinism, and the
NIOFP3D grid (40^3 padded to 42^3: 1764 flattened rows through the reused row kernels).

Bars (DESIGN.md section 2 / SURVEY.md 8c): forward rel-L2 <= 1e-5, gradients rel-L2 <= 1e-4.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

import fno3d_ref
from test_fno3d_golden import CASES, load3d

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _load(module, g, strict=True):
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")}
    missing, unexpected = module.load_state_dict(sd, strict=strict)
    assert not unexpected
    return module


def _run(module, g, fwd, inputs):
    module.cuda()
    ins = {k: torch.from_numpy(g["in." + k]).cuda().requires_grad_(("gin." + k) in g) for k in inputs}
    out = fwd(module, ins)
    torch.cuda.synchronize()
    e = rel_l2(out.detach().cpu().numpy(), g["out"])
    print(f"fwd rel-L2 {e:.2e}")
    assert e <= FWD_TOL, e
    (out * torch.from_numpy(g["cot"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    named = dict(module.named_parameters())
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            p = named[k[2:]]
            assert p.grad is not None, k
            e = rel_l2(p.grad.detach().cpu().numpy(), v)
            print(f"{k} rel-L2 {e:.2e}")
            assert e <= GRAD_TOL, (k, e)
            n += 1
        elif k.startswith("gin."):
            e = rel_l2(ins[k[4:]].grad.detach().cpu().numpy(), v)
            print(f"{k} rel-L2 {e:.2e}")
            assert e <= GRAD_TOL, (k, e)
            n += 1
    assert n > 0
    return out, named, ins


@pytest.mark.parametrize("case", list(CASES))
def test_golden(case):
    import blindno
    kind, args = CASES[case]
    g = load3d(case)
    cls = blindno.SpectralConv3d if kind == "sc3d" else blindno.FNO3d
    m = _load(cls(*args), g)
    _, named, _ = _run(m, g, lambda m, i: m(i["x"]), ["x"])
    if case == "sc3d_overlap":
        # an entry that lost an overlap gets exactly 0
        for q, mask in enumerate(fno3d_ref.winners(3, 3, 5, 5)):
            gw = named[f"weights{q + 1}"].grad.cpu()
            if (~mask).any():
                assert float(gw[:, :, ~mask].abs().max()) == 0.0


def _cplx(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(shape, generator=gen), torch.randn(shape, generator=gen))


@pytest.mark.parametrize("case", ["sc3d_overlap", "sc3d_tiles"])
def test_colpass3d_alone(case):
    from blindno import ops
    from blindno._lib import query
    g = load3d(case)
    Bn, Ci, P1, P2, P3 = g["in.x"].shape
    ws = [torch.from_numpy(g[f"p.weights{q}"]) for q in range(1, 5)]
    Co, m1, m2, m3 = ws[0].shape[1:]
    sh = ops.Spec3Shape(Bn, Ci, Co, P1, P2, P3, m1, m2, m3)
    assert query("blindno_spectrum_tile_layout", Bn, Co, P1 * P2, P3, m3) == 0
    assert query("blindno_spectrum_tile_layout", Bn, Ci, P1 * P2, P3, m3) == 0
    Wt = ops.k_pack_w3d([w.cuda() for w in ws], sh)
    ws64 = [fno3d_ref.to64(w) for w in ws]
    jx = torch.tensor(ops.kept_rows(m1, P1))
    jy = torch.tensor(ops.kept_rows(m2, P2))
    outs = []
    for direction, cin, cout, tol in ((0, Ci, Co, FWD_TOL), (1, Co, Ci, GRAD_TOL)):
        a = _cplx((Bn, m3, cin, P1, P2), 7 + direction)
        At = torch.view_as_real(a).contiguous().cuda()
        Xs, Z = ops.k_colpass3d(At, Wt, sh, direction)
        torch.cuda.synchronize()
        a64 = a.to(torch.complex128)
        want_x = torch.fft.fftn(a64, dim=[-2, -1])[:, :, :, jx][:, :, :, :, jy]
        got_x = torch.view_as_complex(Xs.cpu()).view(Bn, m3, cin, sh.K1, sh.K2)
        e = rel_l2(got_x.numpy(), want_x.numpy())
        print(f"{case} dir {direction}: spectrum {e:.2e}")
        assert e <= tol, e
        want = fno3d_ref.mixed_spectrum_planes(a64, ws64, (P1, P2, P3), direction)
        got = torch.view_as_complex(Z.cpu()).view(Bn, P1, P2, m3, cout)
        e = rel_l2(got.numpy(), want.numpy())
        print(f"{case} dir {direction}: Z {e:.2e}")
        assert e <= tol, e
        outs.append((a64, got.to(torch.complex128)))
    # <colpass(a), b> = <a, colpass_adj(b)> in float64 on the host
    (a, La), (b, Lb) = outs
    lhs = torch.sum(La.conj() * b.permute(0, 3, 4, 1, 2)).real
    rhs = torch.sum(a.permute(0, 3, 4, 1, 2).conj() * Lb).real
    print(f"{case}: <La, b> {float(lhs):.9e}  <a, L^H b> {float(rhs):.9e}")
    assert abs(float(lhs - rhs)) <= 1e-5 * abs(float(lhs))


def test_deterministic():
    import blindno
    g = load3d("fno3d_b")
    res = []
    for _ in range(2):
        m = _load(blindno.FNO3d(*CASES["fno3d_b"][1]), g).cuda()
        x = torch.from_numpy(g["in.x"]).cuda().requires_grad_(True)
        out = m(x)
        (out * torch.from_numpy(g["cot"]).cuda()).sum().backward()
        torch.cuda.synchronize()
        res.append([out.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in m.parameters()])
    for a, b in zip(*res):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a,
                           torch.view_as_real(b) if b.is_complex() else b)


def test_workload_shape():
    """FNO3d(8, 12, 4, 4, 1) on NIOFP3D's 40^3 grid (padded 42^3: 1764 flattened rows, not a
    multiple of 16; width 12 with even modes takes the row inverse's A-tile spectrum order)."""
    import blindno
    torch.manual_seed(11)
    m = blindno.FNO3d(8, 12, 4, 4, 1)
    x = torch.randn(1, 40, 40, 40, 4)
    cot = torch.randn(1, 40, 40, 40, 1)
    want, grads, gin = fno3d_ref.run("fno3d", dict(m.state_dict()), x, cot)
    m.cuda()
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    (out * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    e = rel_l2(out.detach().cpu().numpy(), want.numpy())
    print(f"fwd rel-L2 {e:.2e}")
    assert e <= FWD_TOL, e
    e = rel_l2(xg.grad.cpu().numpy(), gin.numpy())
    print(f"gin rel-L2 {e:.2e}")
    assert e <= GRAD_TOL, e
    for k, p in m.named_parameters():
        e = rel_l2(p.grad.cpu().numpy(), grads[k].numpy())
        print(f"g.{k} rel-L2 {e:.2e}")
        assert e <= GRAD_TOL, (k, e)


def test_lift3d_project3d_alone():
    from blindno import ops
    N, P, Cin, C, Hd, Cout, Bn = (6, 5, 7), (8, 7, 9), 4, 5, 128, 2, 2
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen)
    inp, w0, b0 = r(Bn, *N, Cin), r(C, Cin) * 0.5, r(C) * 0.1
    dx0 = r(Bn, C, *P)
    # lift
    x0 = ops.lift3d(inp.cuda(), w0.cuda(), b0.cuda(), P)
    d_in, gw0, gb0 = ops.lift3d_backward(dx0.cuda(), inp.cuda(), w0.cuda(), P)
    torch.cuda.synchronize()
    i64, w64, b64 = (t.double().requires_grad_(True) for t in (inp, w0, b0))
    ref = F.pad(F.linear(i64, w64, b64).permute(0, 4, 1, 2, 3), [0, P[2] - N[2], 0, P[1] - N[1], 0, P[0] - N[0]])
    (ref * dx0.double()).sum().backward()
    assert rel_l2(x0.cpu().numpy(), ref.detach().numpy()) <= FWD_TOL
    pad = torch.ones(P, dtype=torch.bool)
    pad[:N[0], :N[1], :N[2]] = False
    assert float(x0.cpu()[:, :, pad].abs().max()) == 0.0
    for got, want in ((d_in, i64.grad), (gw0, w64.grad), (gb0, b64.grad)):
        assert rel_l2(got.cpu().numpy(), want.numpy()) <= GRAD_TOL
    # projection
    z, w1, b1, w2, b2 = r(Bn, C, *P), r(Hd, C) * 0.4, r(Hd) * 0.1, r(Cout, Hd) * 0.1, r(Cout) * 0.1
    gout = r(Bn, *N, Cout)
    out = ops.project3d(z.cuda(), w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), N)
    dz, gw1, gb1, gw2, gb2 = ops.project3d_backward(z.cuda(), w1.cuda(), b1.cuda(), w2.cuda(), gout.cuda(), N)
    torch.cuda.synchronize()
    z64, w164, b164, w264, b264 = (t.double().requires_grad_(True) for t in (z, w1, b1, w2, b2))
    h = z64[..., :N[0], :N[1], :N[2]].permute(0, 2, 3, 4, 1)
    ref = F.linear(F.gelu(F.linear(h, w164, b164)), w264, b264)
    (ref * gout.double()).sum().backward()
    e = rel_l2(out.cpu().numpy(), ref.detach().numpy())
    print(f"project3d fwd {e:.2e}")
    assert e <= FWD_TOL, e
    for name, got, want in (("dz", dz, z64.grad), ("dW1", gw1, w164.grad), ("db1", gb1, b164.grad),
                            ("dW2", gw2, w264.grad), ("db2", gb2, b264.grad)):
        e = rel_l2(got.cpu().numpy(), want.numpy())
        print(f"project3d {name} {e:.2e}")
        assert e <= GRAD_TOL, (name, e)
    assert float(dz.cpu()[:, :, pad].abs().max()) == 0.0


def test_rejected_on_device():
    import blindno
    from blindno._lib import BlindnoError
    with pytest.raises(BlindnoError):
        blindno.SpectralConv3d(2, 2, 2, 2, 5).cuda()(torch.randn(1, 2, 6, 6, 6).cuda())
