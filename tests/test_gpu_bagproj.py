"""The bag-level projection entry point (csrc/bagproj.hip, blindno_project_bag_fwd) called through
the C ABI against a float64 torch restatement of what it replaces: the FNO_input projection
(crop -> fc1 -> GELU -> fc2, 2d_FPE/FNOModules.py:234-239) of every snapshot of a bag and the
weighted bag mean over the snapshots (2d_FPE/NIOModules.py:569-575).  The statistics it leaves are
then fed to blindno_project_bag_bwd, whose fc1 / fc2 gradients are compared with float64 autograd.

The shapes reach the workgroup set-up's edge cases: one snapshot per bag, a bag size that is not
a multiple of the 8-snapshot chunk, more snapshots than the 256 threads that stage the bag
weights (two staging rounds), 3 channels (the clamped channel of the first chunk's loads), and
a crop whose 16-point tiles straddle bags."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gelu(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def _gelu_grad(h):
    cdf = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return cdf + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def _rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


@pytest.mark.parametrize("B,U,C,P,N", [(2, 1, 4, 40, 30), (3, 37, 4, 40, 30), (2, 300, 4, 24, 18),
                                       (2, 19, 3, 40, 30)])
def test_project_bag_fwd_matches_fp64(B, U, C, P, N):
    import blindno
    from blindno._lib import call, ptr, query, stream_ptr
    blindno.load_library()
    g = torch.Generator(device="cuda").manual_seed(100 + U)
    dev = torch.device("cuda")
    z = torch.randn(B * U, C, P, P, device=dev, generator=g)
    w1 = torch.randn(128, C, device=dev, generator=g) * 0.4
    b1 = torch.randn(128, device=dev, generator=g) * 0.1
    w2 = torch.randn(1, 128, device=dev, generator=g) * 0.1
    b2 = torch.randn(1, device=dev, generator=g)
    lw = torch.rand(U, device=dev, generator=g) + 0.5
    lw = lw / lw.sum()
    ubar = torch.full((B, N * N), float("nan"), device=dev)
    stats = torch.empty(query("blindno_project_bag_stats_floats", B, N, N), device=dev)
    v = torch.full_like(z, float("nan"))
    call("blindno_project_bag_fwd", ptr(z), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(lw), ptr(ubar),
         ptr(stats), ptr(v), B, U, C, P, P, N, N, 128, stream_ptr())
    torch.cuda.synchronize()

    zc = z[:, :, :N, :N].double().permute(0, 2, 3, 1).reshape(B, U, N * N, C)
    h = zc @ w1.double().t() + b1.double()                      # (B, U, pts, 128)
    proj = _gelu(h) @ w2.double().t() + b2.double()             # (B, U, pts, 1)
    ubar_ref = (lw.double().view(1, U, 1) * proj[..., 0]).sum(1)
    v_ref = (_gelu_grad(h) * w2.double().view(1, 1, 1, 128)) @ w1.double()   # (B, U, pts, C)
    v_gpu = v[:, :, :N, :N].double().permute(0, 2, 3, 1).reshape(B, U, N * N, C)
    e_u, e_v = _rel(ubar.double(), ubar_ref), _rel(v_gpu, v_ref)
    print(f"B={B} U={U} C={C} N={N}: ubar {e_u:.2e}, v {e_v:.2e}")
    assert torch.isfinite(ubar).all() and torch.isfinite(v_gpu).all()
    # fp32 fc1 / fc2 and the A&S erf (|err| <= 4.2e-7) against float64 (measured <= 2e-7)
    assert e_u <= 2e-6
    assert e_v <= 2e-6

    # the backward entry point on the statistics just produced: the fc1 / fc2 gradients, reduced
    # from the per-workgroup partials [dW1 (Hd C) | db1 (Hd) | dW2 (Hd) | db2], against float64
    # autograd of the same restatement (dz = NULL: its consumers form it on load)
    from blindno import ops
    ghat = torch.randn(B, N * N, device=dev, generator=g)
    nchunk = query("blindno_project_bag_bwd_nchunk", B, N, N)
    np_ = 128 * C + 2 * 128 + 1
    partial = torch.full((nchunk, np_), float("nan"), device=dev)
    call("blindno_project_bag_bwd", ptr(stats), ptr(ghat), ptr(w2), ptr(lw), None, None, ptr(partial),
         nchunk, B, U, C, P, P, N, N, 128, stream_ptr())
    gp = ops.reduce_partials(partial, nchunk, np_)
    torch.cuda.synchronize()
    leaves = [t.double().cpu().requires_grad_(True) for t in (w1, b1, w2, b2)]
    w1d, b1d, w2d, b2d = leaves
    pr = _gelu(zc.cpu() @ w1d.t() + b1d) @ w2d.t() + b2d
    ub = (lw.double().cpu().view(1, U, 1) * pr[..., 0]).sum(1)
    (ub * ghat.double().cpu()).sum().backward()
    gp = gp.double().cpu()
    got = (gp[:128 * C].view(128, C), gp[128 * C:128 * C + 128], gp[128 * C + 128:128 * C + 256].view(1, 128),
           gp[128 * C + 256:])
    assert torch.isfinite(gp).all()
    for name, a, leaf in zip(("dw1", "db1", "dw2", "db2"), got, leaves):
        e = _rel(a, leaf.grad)
        print(f"B={B} U={U} C={C} N={N}: {name} {e:.2e}")
        assert e <= 2e-6, (name, e)
