"""The bag-level projection entry point (csrc/bagproj.hip, blindno_project_bag_fwd) called through
the C ABI against a float64 torch restatement of what it replaces: the FNO_input projection
(crop -> fc1 -> GELU -> fc2, 2d_FPE/FNOModules.py:234-239) of every snapshot of a bag and the
weighted bag mean over the snapshots (2d_FPE/NIOModules.py:569-575).  The statistics it leaves are
then fed to blindno_project_bag_bwd, whose fc1 / fc2 gradients are compared with float64 autograd.

The shapes reach the workgroup set-up's edge cases: one snapshot per bag, a bag size that is not
a multiple of the 8-snapshot chunk, more snapshots than the 256 threads that stage the bag
weights (two staging rounds), 3 channels (the clamped channel of the first chunk's loads), and
a crop whose 16-point tiles straddle bags.

The second half calls both entry points on projection_ref.BAG_CASES (those four shapes, rectangular
grids with P1 != P2 and Ho != Wo, C = 1 and 2, bag sizes at the edges of the 8-snapshot double
buffer, U = 1024) with lw = NULL and with multiplicities / L, against the float64 bag reference
under the per-element bound derived in tests/projection_ref.py (the sum over the snapshots adds U
terms): ubar, v, dz = lw ghat v on the crop (dz and v pre-filled with the sentinel and untouched
outside it) and the gradients, summed on the host in float64 from the per-workgroup partials, at
nchunk 1, 3 (the backward's stride loop tg += gridDim.x iterates) and the default."""
import math

import numpy as np
import pytest
import torch

import projection_ref as pr
from projection_ref import Guarded, worst
from spectral_stage_ref import SENT

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


# ================================================================================ per-element bound
INVALID = 1              # hipErrorInvalidValue
SENT32 = np.float32(SENT)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _ratio(label, got, ref, bound):
    r = worst(np.abs(np.asarray(got, np.float64) - ref), np.broadcast_to(bound, np.shape(ref)))
    print(f"{label}: worst err/bound {r:.3f}")
    assert r <= 1.0, (label, r)


def _on_crop(label, buf, case):
    """A guarded (B U, C, P1, P2) field: untouched outside the crop; returns the crop."""
    B, U, C, P, N = case
    assert buf.margins_intact()
    d = buf.cpu().numpy().reshape(B * U, C, *P)
    outside = np.ones(d.shape, bool)
    outside[:, :, :N[0], :N[1]] = False
    assert np.all(d[outside] == SENT32), label + " written outside the crop"
    return d[:, :, :N[0], :N[1]]


def _bag_fwd(case, d):
    from blindno._lib import load, ptr, query, stream_ptr
    B, U, C, P, N = case
    ubar, v = Guarded(B * N[0] * N[1]), Guarded(B * U * C * P[0] * P[1])
    stats = torch.full((query("blindno_project_bag_stats_floats", B, *N),), float("nan"), device="cuda")
    rc = load().blindno_project_bag_fwd(*[ptr(d[k]) for k in ("z", "w1", "b1", "w2", "b2", "lw")], ptr(ubar.t),
                                        ptr(stats), ptr(v.t), B, U, C, *P, *N, 128, stream_ptr())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return ubar, stats, v


def _bag_bwd(case, d, stats, v, nchunk, want_dz=True):
    from blindno._lib import load, ptr, stream_ptr
    B, U, C, P, N = case
    dz = Guarded(B * U * C * P[0] * P[1])
    part = Guarded(nchunk * (128 * C + 257))
    rc = load().blindno_project_bag_bwd(ptr(stats), ptr(d["gs"]), ptr(d["w2"]), ptr(d["lw"]),
                                        ptr(v.t) if want_dz else None, ptr(dz.t) if want_dz else None, ptr(part.t),
                                        nchunk, B, U, C, *P, *N, 128, stream_ptr())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return dz, part


def _bag_nchunks(case):
    from blindno._lib import query
    return sorted({1, 3, query("blindno_project_bag_bwd_nchunk", case[0], *case[4])})


@pytest.mark.parametrize("weighted", [False, True], ids=["lw_null", "lw_counts"])
@pytest.mark.parametrize("case", pr.BAG_CASES, ids=pr.bag_id)
def test_project_bag_vs_fp64_bound(case, weighted):
    import blindno
    blindno.load_library()
    B, U, C, P, N = case
    t = pr.bag_inputs(case, weighted)
    d = {k: _dev(a) for k, a in t.items()}
    a = (t["z"], t["w1"], t["b1"], t["w2"])
    label = f"bag {pr.bag_id(case)} weighted={weighted}"
    ubar, stats, v = _bag_fwd(case, d)
    (ur, vr), (bu, bv) = pr.bag_fwd(*a, t["b2"], t["lw"], U, *N), pr.bag_fwd_bound(*a, t["b2"], t["lw"], U, *N)
    assert ubar.margins_intact()
    _ratio(label + " ubar", ubar.cpu().numpy().reshape(B, -1), ur, bu)
    _ratio(label + " v", _on_crop(label + " v", v, case), vr, bv)
    (dzr, gr), (bz, bg) = pr.bag_bwd(*a, t["lw"], U, t["gs"], *N), pr.bag_bwd_bound(*a, t["lw"], U, t["gs"], *N)
    for nchunk in _bag_nchunks(case):
        dz, part = _bag_bwd(case, d, stats, v, nchunk)
        _ratio(f"{label} nchunk={nchunk} dz", _on_crop(label + " dz", dz, case), dzr, bz)
        assert part.margins_intact()
        _ratio(f"{label} nchunk={nchunk} dW1|db1|dW2|db2", part.cpu().double().numpy().reshape(nchunk, -1).sum(0), gr, bg)
    # dz = NULL: the gradients alone, dz and v not touched / read
    dz, part = _bag_bwd(case, d, stats, v, 3, want_dz=False)
    assert dz.untouched()
    _ratio(f"{label} dz=NULL dW1|db1|dW2|db2", part.cpu().double().numpy().reshape(3, -1).sum(0), gr, bg)


@pytest.mark.parametrize("case", [pr.BAG_CASES[4], pr.BAG_CASES[10]], ids=pr.bag_id)
def test_project_bag_is_bit_reproducible(case):
    import blindno
    blindno.load_library()
    d = {k: _dev(a) for k, a in pr.bag_inputs(case, True).items()}
    runs = []
    for _ in range(2):
        ubar, stats, v = _bag_fwd(case, d)
        dz, part = _bag_bwd(case, d, stats, v, 3)
        runs.append((ubar.buf, stats, v.buf, dz.buf, part.buf))
    for name, x, y in zip(("ubar", "stats", "v", "dz", "partial"), *runs):
        assert torch.equal(x, y), name


def test_invalid_bag_projection_calls_are_refused_on_the_host():
    from blindno._lib import load, ptr, stream_ptr
    import blindno
    blindno.load_library()
    lib, sp = load(), stream_ptr
    n = 1 << 16
    src = torch.zeros(n, device="cuda")
    o1, o2, o3 = Guarded(n), Guarded(n), Guarded(n)
    p, q1, q2, q3 = ptr(src), ptr(o1.t), ptr(o2.t), ptr(o3.t)

    def fwd(U=2, C=4, P1=8, Ho=6, Hd=128, stats=q2):
        return int(lib.blindno_project_bag_fwd(p, p, p, p, p, None, q1, stats, q3, 1, U, C, P1, 8, Ho, 6, Hd, sp()))

    def bwd(U=2, C=4, P1=8, Ho=6, Hd=128, stats=p, v=p, dz=q1, nchunk=2):
        return int(lib.blindno_project_bag_bwd(stats, p, p, None, v, dz, q2, nchunk, 1, U, C, P1, 8, Ho, 6, Hd, sp()))

    assert fwd(U=1025) == INVALID and bwd(U=1025) == INVALID
    assert fwd(C=5) == INVALID and bwd(C=5) == INVALID
    assert fwd(Hd=64) == INVALID and bwd(Hd=64) == INVALID
    assert fwd(Ho=9) == INVALID and bwd(Ho=9) == INVALID                 # Ho > P1
    assert bwd(v=None) == INVALID                                        # dz given with v = NULL
    assert bwd(nchunk=0) == INVALID
    assert fwd(stats=None) == INVALID and bwd(stats=None) == INVALID     # NULL stats
    torch.cuda.synchronize()
    assert o1.untouched() and o2.untouched() and o3.untouched()
