"""The first encoder layer's gradients without the row inverse of dz0: the
identity behind blindno_liftgrad_spec, restated with torch.fft in float64 on the CPU.

Layer 0 of FNO_input (2d_FPE/FNOModules.py:156-178, 226-232; the lift of NIOFP2D_FNO):
    in = (u, gx, gy) on the N x N crop,  x0 = pad(fc0(in)) to P x P,
    z0 = irfft2(W . rfft2(x0) on the kept modes) + Wc x0 + bc.
x0 is linear in the single snapshot channel, x0[c] = sum_j A[c][j] in_j with in = (u, gx, gy, 1 on
the crop) and A = [fc0.weight | fc0.bias], so for any dz0 = dL/dz0 every parameter gradient of
the layer is a function of
    M[o][j] = sum_{n, p in crop} dz0[n][o][p] in_j[n][p]                       (16 moments)
    Ru[o][k] = sum_n conj(U[n][k]) G[n][o][k],   R1[o][k] = sum_n G[n][o][k]   (kept modes k)
where G is the adjoint spectrum of dz0 (the gradient of L with respect to the mixed kept modes)
and U the kept-mode spectrum of the zero-padded snapshot.  The test pins the conjugations:
    dW[c][o][k] = A[c][0] Ru[o][k] + conj(Gam_c[k]) R1[o][k],  Gam_c = sum_{j>=1} A[c][j] In_j
    dA[c][0]    = sum_o Wc[o][c] M[o][0] + sum_{o,k} Re(conj(Ru[o][k]) W[c][o][k])
    dA[c][j]    = sum_o Wc[o][c] M[o][j] + sum_{o,k} Re(In_j[k] conj(R1[o][k]) W[c][o][k])
    dWc[o][c]   = sum_j A[c][j] M[o][j]
    dbc[o]      = P P Re R1[o][DC]     (the bias acts on the whole padded field, not the crop)
against autograd, to float64 rounding (1e-12 relative).
"""
import pytest
import torch

C = 4


def _kept(xf, m1, m2):
    return torch.cat([xf[..., :m1, :m2], xf[..., -m1:, :m2]], dim=-2)


def _embed(Y, P, m1, m2):
    out = torch.zeros(*Y.shape[:-2], P, P // 2 + 1, dtype=Y.dtype)
    out[..., :m1, :m2] = Y[..., :m1, :]
    out[..., -m1:, :m2] = Y[..., m1:, :]
    return out


# (N, P, m1, m2): the tiny 12 -> 16 grid; a crop that is no multiple of the 16-row pad block
# inside two blocks; the Nyquist column kept (m2 = P / 2 + 1); every row kept and the Nyquist
# column at once
CASES = [(12, 16, 3, 3), (21, 32, 3, 5), (6, 8, 3, 5), (5, 8, 4, 5)]


@pytest.mark.parametrize("N,P,m1,m2", CASES)
def test_first_layer_gradients_from_moments_and_spectra(N, P, m1, m2):
    torch.manual_seed(N * 100 + P)
    f64, c128 = torch.float64, torch.complex128
    Bn = 3
    u = torch.randn(Bn, N, N, dtype=f64)
    lin = torch.linspace(-1, 1, N, dtype=f64)
    gx, gy = torch.meshgrid(lin, lin, indexing="ij")
    gx = gx + 0.1 * torch.randn(N, N, dtype=f64)         # a non-separable grid
    fc0w = torch.randn(C, 3, dtype=f64, requires_grad=True)
    fc0b = torch.randn(C, dtype=f64, requires_grad=True)
    w1 = torch.randn(C, C, m1, m2, dtype=c128, requires_grad=True)
    w2 = torch.randn(C, C, m1, m2, dtype=c128, requires_grad=True)
    wc = torch.randn(C, C, dtype=f64, requires_grad=True)
    bc = torch.randn(C, dtype=f64, requires_grad=True)
    lw = torch.tensor([1.0, 2.0, 4.0], dtype=f64) / 7.0   # unequal snapshot weights
    R = torch.randn(Bn, C, P, P, dtype=f64) * lw[:, None, None, None]

    ones = torch.ones(N, N, dtype=f64)
    inp = torch.stack([u, gx.expand(Bn, N, N), gy.expand(Bn, N, N), ones.expand(Bn, N, N)], 1)
    pad = (0, P - N, 0, P - N)
    A = torch.cat([fc0w, fc0b[:, None]], 1)                               # (C, 4)
    x0 = torch.nn.functional.pad(torch.einsum("cj,njhw->nchw", A, inp), pad)
    W = torch.cat([w1, w2], dim=2)                                        # (C, C, 2 m1, m2)
    Y = torch.einsum("nckl,cokl->nokl", _kept(torch.fft.rfft2(x0), m1, m2), W)
    Y.retain_grad()
    z0 = torch.fft.irfft2(_embed(Y, P, m1, m2), s=(P, P)) + torch.einsum("oc,nchw->nohw", wc, x0) \
        + bc[None, :, None, None]
    z0.retain_grad()
    (z0 * R).sum().backward()

    # what the closed forms may use: dz0 on the field only through M, its spectrum only through
    # Ru and R1
    dz0, G = z0.grad, Y.grad
    M = torch.einsum("nohw,njhw->oj", dz0[:, :, :N, :N], inp)
    Inh = _kept(torch.fft.rfft2(torch.nn.functional.pad(inp, pad)), m1, m2)   # (Bn, 4, 2 m1, m2)
    U, Ig = Inh[:, 0], Inh[0, 1:]                                         # (Bn, K1, m2), (3, K1, m2)
    Ru = torch.einsum("nkl,nokl->okl", U.conj(), G)
    R1 = G.sum(0)
    Ad, Wd, wcd = A.detach(), W.detach(), wc.detach()

    Gam = torch.einsum("cj,jkl->ckl", Ad[:, 1:].to(c128), Ig)
    dW = Ad[:, 0, None, None, None] * Ru[None] + Gam.conj()[:, None] * R1[None]
    dA = torch.einsum("oc,oj->cj", wcd, M)
    dA[:, 0] += torch.einsum("okl,cokl->c", Ru.conj(), Wd).real
    dA[:, 1:] += torch.einsum("jkl,okl,cokl->cj", Ig, R1.conj(), Wd).real
    dWc = torch.einsum("cj,oj->oc", Ad, M)
    dbc = P * P * R1[:, 0, 0].real

    def close(got, ref, name):
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err <= 1e-12, (name, err)

    close(dW[:, :, :m1], w1.grad, "weights1")
    close(dW[:, :, m1:], w2.grad, "weights2")
    close(dA[:, :3], fc0w.grad, "fc0.weight")
    close(dA[:, 3], fc0b.grad, "fc0.bias")
    close(dWc, wc.grad, "conv.weight")
    close(dbc, bc.grad, "conv.bias")
