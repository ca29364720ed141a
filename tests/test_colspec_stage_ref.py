"""tests/colspec_stage_ref.py against an independent float64 restatement with torch.fft (rfft2 /
irfft2 on the zero-padded field, float64 autograd for the adjoints and the gradient rows; the
style of test_gpu_liftgrad._layer0_fp64), at P1 != P2 and with a crop: the references, not the
kernels, define the operations the GPU tests of test_gpu_colspec_stages.py check.  Agreement is
float64 rounding: <= 1e-12 of the largest magnitude."""
import numpy as np
import pytest
import torch

import colspec_stage_ref as cr
import spectral_stage_ref as sr

C, M2 = 4, 12
GEOMS = [pytest.param((48, 32, 37, 28), id="P48x32"), pytest.param((32, 64, 23, 52), id="P32x64")]
B, T, IDX = 2, 5, [4, 0, 2, 0]


def _close(label, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{label}: {e:.2e}")
    assert e <= 1e-12, (label, e)


def _gelu(t):
    return torch.nn.functional.gelu(t)


def _rows(P1):
    return torch.tensor(sr.kept_rows(cr.M1, P1))


def _fft_spectrum(f):
    """f (Bn, C, P1, P2) float64 tensor -> (Bn, m2, C, K1) complex numpy."""
    return torch.fft.rfft2(f)[:, :, _rows(f.shape[2]), :M2].permute(0, 3, 1, 2).numpy()


def _layer(f, w1, w2, wc, bc):
    """SpectralConv2d (two kept corner blocks) + 1x1 conv + bias on the layer input f."""
    Bn, _, P1, P2 = f.shape
    xf = torch.fft.rfft2(f)
    of = torch.zeros(Bn, C, P1, P2 // 2 + 1, dtype=torch.complex128)
    of[:, :, :cr.M1, :M2] = torch.einsum("nckl,cokl->nokl", xf[:, :, :cr.M1, :M2], w1)
    of[:, :, -cr.M1:, :M2] = torch.einsum("nckl,cokl->nokl", xf[:, :, -cr.M1:, :M2], w2)
    return torch.fft.irfft2(of, s=(P1, P2)) + torch.einsum("oc,nchw->nohw", wc, f) + bc[None, :, None, None]


def _data(geom, seed):
    P1, P2, N1, N2 = geom
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s)
    d = dict(x=r(3, C, P1, P2), dz=r(3, C, P1, P2), w1=r(C, C, cr.M1, M2) + 1j * r(C, C, cr.M1, M2),
             w2=r(C, C, cr.M1, M2) + 1j * r(C, C, cr.M1, M2), wc=r(C, C), bc=r(C), X=r(B, T, N1, N2),
             grid=r(N1, N2, 2), w0=r(C, 3), b0=r(C), dzl=r(B * len(IDX), C, P1, P2))
    d["Wt"] = sr.pack_w2d(d["w1"], d["w2"], P1)
    return d


def _pad(t, P1, P2):
    return torch.nn.functional.pad(t, (0, P2 - t.shape[-1], 0, P1 - t.shape[-2]))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom", GEOMS)
def test_spectrum_mix_and_row_inverse_match_fft(geom, act):
    """spectrum (with a valid region), mix dir 0 with pack_w2d's order, z_from_y and the epilogue:
    the whole layer z = irfft2(W rfft2(f(x))) + Wc f(x) + bc."""
    P1, P2, N1, N2 = geom
    d = _data(geom, 1)
    xt = torch.from_numpy(d["x"])
    xv = torch.zeros_like(xt)
    xv[:, :, :N1, :N2] = (_gelu(xt) if act else xt)[:, :, :N1, :N2]
    _close("spectrum on the valid region", cr.spectrum(d["x"], M2, act, (N1, N2)), _fft_spectrum(xv))
    f = _gelu(xt) if act else xt
    Xs = cr.spectrum(d["x"], M2, act)
    _close("spectrum", Xs, _fft_spectrum(f))
    Xsave, Y = cr.mix(Xs, d["Wt"], P1, P2, 0)
    assert Xsave is Xs
    z = sr.row_inv(cr.z_from_y(Y, P1), P2, d["x"], d["wc"], d["bc"], act)
    ref = _layer(f, *(torch.from_numpy(d[k]) for k in ("w1", "w2", "wc", "bc")))
    _close("layer output", z, ref.numpy())


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom", GEOMS)
def test_adjoint_and_conv_gradient_rows_match_autograd(geom, act):
    """mix dir 1 (G = c_k/(P1 P2) X of the cropped dz, Y = conj(W) G), z_from_y, row_inv_adj and
    conv_wgrad: float64 autograd of <layer(x), dz> with dz zero outside its crop."""
    P1, P2, N1, N2 = geom
    d = _data(geom, 2)
    xt = torch.from_numpy(d["x"]).requires_grad_(True)
    wc, bc = (torch.from_numpy(d[k]).requires_grad_(True) for k in ("wc", "bc"))
    dzc = torch.zeros(d["dz"].shape, dtype=torch.float64)
    dzc[:, :, :N1, :N2] = torch.from_numpy(d["dz"])[:, :, :N1, :N2]
    z = _layer(_gelu(xt) if act else xt, torch.from_numpy(d["w1"]), torch.from_numpy(d["w2"]), wc, bc)
    (z * dzc).sum().backward()
    G, Y = cr.mix(cr.spectrum(d["dz"], M2, 0, (N1, N2)), d["Wt"], P1, P2, 1)
    _close("G", G, _fft_spectrum(dzc) * (sr.c2r(M2, P2) / (P1 * P2))[None, :, None, None])
    dx = sr.row_inv_adj(cr.z_from_y(Y, P1), P2, d["dz"], d["wc"], d["x"], act, (N1, N2))
    _close("dx", dx, xt.grad.numpy())
    _close("dWc | dbc", sr.conv_wgrad(d["dz"], d["x"], act, (N1, N2)),
           np.concatenate([wc.grad.numpy().ravel(), bc.grad.numpy()]))


@pytest.mark.parametrize("geom", GEOMS)
def test_lift_references_match_fft_and_autograd(geom):
    """bag_fields / grid_planes / lift_spectrum / lift_field / bag_lift_at against rfft2 / rfft of
    x0 = pad(fc0(u, gx, gy)); bwd_lift_rows against autograd of <layer0, dz> in wc, bc, w0, b0."""
    P1, P2, N1, N2 = geom
    d = _data(geom, 3)
    Xt, gt = torch.from_numpy(d["X"]), torch.from_numpy(d["grid"])
    w0, b0, wc, bc = (torch.from_numpy(d[k]).requires_grad_(True) for k in ("w0", "b0", "wc", "bc"))
    u = Xt[:, IDX].reshape(B * len(IDX), N1, N2)
    inp = torch.stack([u, gt[..., 0].expand_as(u), gt[..., 1].expand_as(u), torch.ones_like(u)], 1)
    x0 = _pad(torch.einsum("cj,njhw->nchw", torch.cat([w0, b0[:, None]], 1), inp), P1, P2)
    _close("x0", cr.lift_field(d["X"], IDX, d["grid"], d["w0"], d["b0"], P1, P2), x0.detach().numpy())
    _close("in", cr.lift_inputs(d["X"], IDX, d["grid"], P1, P2), _pad(inp, P1, P2).numpy())
    U = cr.spectrum(cr.bag_fields(d["X"], IDX, P1, P2), M2)[:, :, 0]
    _close("U", U, _fft_spectrum(_pad(u[:, None], P1, P2))[:, :, 0])
    Dg2 = cr.spectrum(cr.grid_planes(d["grid"], P1, P2), M2)[0]
    _close("Dg2", Dg2, _fft_spectrum(_pad(inp[:1, 1:], P1, P2))[0])
    _close("lifted spectrum", cr.lift_spectrum(U, Dg2, d["w0"], d["b0"]), _fft_spectrum(x0.detach()))
    At = torch.fft.rfft(x0.detach())[..., :M2].permute(0, 3, 1, 2).numpy()
    Dg = sr.row_dft(cr.grid_planes(d["grid"], P1, P2), M2)[0]
    _close("At (Dg)", cr.bag_lift_at(d["X"], IDX, d["w0"], M2, P1, P2, b0=d["b0"], Dg=Dg), At)
    Gt = torch.fft.rfft(_pad(torch.einsum("cj,njhw->nchw", torch.cat([w0, b0[:, None]], 1).detach()[:, 1:],
                                          inp[:1, 1:]), P1, P2))[0, ..., :M2].permute(2, 0, 1).numpy()
    _close("At (Gt)", cr.bag_lift_at(d["X"], IDX, d["w0"], M2, P1, P2, Gt=Gt), At)
    z = _layer(x0, torch.from_numpy(d["w1"]), torch.from_numpy(d["w2"]), wc, bc)
    (z * torch.from_numpy(d["dzl"])).sum().backward()
    _, Y = cr.mix(cr.spectrum(d["dzl"], M2), d["Wt"], P1, P2, 1)
    rows = cr.bwd_lift_rows(cr.z_from_y(Y, P1), P2, d["dzl"], d["wc"], d["X"], IDX, d["grid"], d["w0"], d["b0"])
    ref = np.concatenate([t.grad.numpy().ravel() for t in (wc, bc, w0, b0)])
    _close("dWc | dbc | dW0 | db0", rows, ref)


def test_abs_twins_dominate():
    """Each *_abs twin bounds the modulus of its reference element by element (it is the same sum
    with every term replaced by its modulus)."""
    geom = (48, 32, 37, 28)
    P1, P2, N1, N2 = geom
    d = _data(geom, 4)
    X = cr.spectrum(d["x"], M2, 1, (N1, N2))
    S, cnt = cr.spectrum_abs(d["x"], M2, 1, (N1, N2))
    assert S.shape == (3, 1, C, 1) and np.all(cnt == N1 * N2) and np.all(np.abs(X) <= S * (1 + 1e-12))
    _, Y = cr.mix(X, d["Wt"], P1, P2, 0)
    _, Ya = cr.mix_abs(np.broadcast_to(S, X.shape), d["Wt"], P1, P2, 0)
    assert np.all(np.abs(Y) <= Ya * (1 + 1e-12))
    assert np.all(np.abs(cr.z_from_y(Y, P1)) <= cr.z_from_y_abs(Y, P1) * (1 + 1e-12))
    a = cr.lift_field(d["X"], IDX, d["grid"], d["w0"], d["b0"], P1, P2)
    assert np.all(np.abs(a) <= cr.lift_field_abs(d["X"], IDX, d["grid"], d["w0"], d["b0"], P1, P2) * (1 + 1e-12))
    Dg = sr.row_dft(cr.grid_planes(d["grid"], P1, P2), M2)[0]
    At = cr.bag_lift_at(d["X"], IDX, d["w0"], M2, P1, P2, b0=d["b0"], Dg=Dg)
    Ata = cr.bag_lift_at_abs(d["X"], IDX, d["w0"], M2, P1, P2, b0=d["b0"], Dg=Dg)
    assert Ata.shape == At.shape and np.all(np.abs(At) <= Ata * (1 + 1e-12))
    U = cr.spectrum(cr.bag_fields(d["X"], IDX, P1, P2), M2)[:, :, 0]
    Dg2 = cr.spectrum(cr.grid_planes(d["grid"], P1, P2), M2)[0]
    SU, _ = cr.spectrum_abs(cr.bag_fields(d["X"], IDX, P1, P2), M2)
    Xl, Xla = cr.lift_spectrum(U, Dg2, d["w0"], d["b0"]), cr.lift_spectrum_abs(SU, Dg2, d["w0"], d["b0"])
    assert Xla.shape == Xl.shape and np.all(np.abs(Xl) <= Xla * (1 + 1e-12))
    Z = cr.z_from_y(Y[:1].repeat(B * len(IDX), 0), P1)
    r = cr.bwd_lift_rows(Z, P2, d["dzl"], d["wc"], d["X"], IDX, d["grid"], d["w0"], d["b0"])
    ra = cr.bwd_lift_rows_abs(np.abs(Z), P2, d["dzl"], d["wc"], d["X"], IDX, d["grid"], d["w0"], d["b0"])
    assert np.all(np.abs(r) <= ra * (1 + 1e-12))
