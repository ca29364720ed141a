"""The 3D bag-level projection entry points (csrc/bagproj3d.hip, include/blindno_bag3d.h) called
through the C ABI against a float64 restatement of what they replace: FNO3d's projection (crop ->
fc1 -> GELU -> fc2, 2d_FPE/FNOModules.py:360-364) of every snapshot of a bag and the weighted bag
mean over the snapshots, with the gradients from float64 autograd of that restatement.

Bars, those of tests/test_gpu_bagproj.py (fp32 fc1 / fc2 and the A&S erf, |err| <= 4.2e-7, against
float64): ubar, v, every parameter gradient and dz <= 2e-6 rel-L2; dz exactly 0 on the padding.

Shapes (B, U, C, P, N): a one-snapshot bag with 210 points per bag (a 16-point tile straddles the
bag boundary, the last tile is ragged); U no multiple of the 8-snapshot staged chunk; a long bag
(more snapshots than the 256 threads that stage the weights) with C < 4; C = 1 with a long last
axis and a padding other than 2 on every axis.  Each with lw = NULL (1 / U) and with integer
multiplicities / L.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 4, (9, 8, 7), (7, 6, 5)), (3, 37, 4, (12, 10, 9), (10, 8, 7)),
          (2, 300, 3, (8, 8, 8), (6, 6, 6)), (1, 9, 1, (6, 5, 20), (4, 3, 18))]
BAR = 2e-6


def _gelu(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def _rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


def _inputs(B, U, C, P, N, weighted):
    g = torch.Generator(device="cuda").manual_seed(1000 + 7 * U + C)
    dev = torch.device("cuda")
    t = {"z": torch.randn(B * U, C, *P, device=dev, generator=g),
         "w1": torch.randn(128, C, device=dev, generator=g) * 0.4,
         "b1": torch.randn(128, device=dev, generator=g) * 0.1,
         "w2": torch.randn(1, 128, device=dev, generator=g) * 0.1,
         "b2": torch.randn(1, device=dev, generator=g),
         "gs": torch.randn(B, N[0] * N[1] * N[2], device=dev, generator=g), "lw": None}
    if weighted:
        counts = torch.randint(1, 4, (U,), device=dev, generator=g).float()
        t["lw"] = counts / counts.sum()                 # multiplicity / L
    return t


def _run(B, U, C, P, N, t):
    """Forward + backward through the C ABI; every output starts as NaN."""
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    dev = t["z"].device
    S = N[0] * N[1] * N[2]
    nan = float("nan")
    ubar = torch.full((B, S), nan, device=dev)
    stats = torch.full((query("blindno_project_bag3d_stats_floats", B, *N),), nan, device=dev)
    v = torch.full_like(t["z"], nan)
    call("blindno_project_bag3d_fwd", ptr(t["z"]), ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]),
         ptr(t["lw"]), ptr(ubar), ptr(stats), ptr(v), B, U, C, *P, *N, 128, stream_ptr())
    nchunk = query("blindno_project_bag3d_bwd_nchunk", B, *N)
    np_ = 128 * C + 2 * 128 + 1
    partial = torch.full((nchunk, np_), nan, device=dev)
    dz = torch.full_like(t["z"], nan)
    call("blindno_project_bag3d_bwd", ptr(stats), ptr(t["gs"]), ptr(t["w2"]), ptr(t["lw"]), ptr(v), ptr(dz),
         ptr(partial), nchunk, B, U, C, *P, *N, 128, stream_ptr())
    gp = ops.reduce_partials(partial, nchunk, np_)
    torch.cuda.synchronize()
    return ubar, v, dz, gp


@pytest.mark.parametrize("weighted", [False, True], ids=["lw_null", "lw_counts"])
@pytest.mark.parametrize("B,U,C,P,N", SHAPES)
def test_project_bag3d_matches_fp64(B, U, C, P, N, weighted):
    import blindno
    blindno.load_library()
    t = _inputs(B, U, C, P, N, weighted)
    ubar, v, dz, gp = _run(B, U, C, P, N, t)
    S = N[0] * N[1] * N[2]
    crop = (slice(None), slice(None), slice(0, N[0]), slice(0, N[1]), slice(0, N[2]))

    # float64 definition with autograd: z on the crop is the leaf whose gradient dz is
    z64 = t["z"].double().cpu()[crop].clone().requires_grad_(True)
    w1, b1, w2, b2 = [t[k].double().cpu().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")]
    lw = (t["lw"].double().cpu() if weighted else torch.full((U,), 1.0 / U, dtype=torch.float64))
    zc = z64.permute(0, 2, 3, 4, 1).reshape(B, U, S, C)
    h = zc @ w1.t() + b1                                        # (B, U, S, 128)
    proj = _gelu(h) @ w2.t() + b2                               # (B, U, S, 1)
    ubar_ref = (lw.view(1, U, 1) * proj[..., 0]).sum(1)         # (B, S)
    (ubar_ref * t["gs"].double().cpu()).sum().backward()
    # v = d proj / d z per snapshot point = W1^T (w2 * GELU'(h))
    hd = h.detach()
    cdf = 0.5 * (1.0 + torch.erf(hd / math.sqrt(2.0)))
    gd = cdf + hd * torch.exp(-0.5 * hd * hd) / math.sqrt(2.0 * math.pi)
    v_ref = (gd * w2.detach().view(1, 1, 1, 128)) @ w1.detach()              # (B, U, S, C)

    v_gpu = v[crop].double().cpu().permute(0, 2, 3, 4, 1).reshape(B, U, S, C)
    errs = {"ubar": _rel(ubar.double().cpu(), ubar_ref.detach()), "v": _rel(v_gpu, v_ref),
            "dz": _rel(dz[crop].double().cpu(), z64.grad)}
    gp = gp.double().cpu()
    assert torch.isfinite(gp).all() and torch.isfinite(ubar).all() and torch.isfinite(dz).all()
    o1, o2, o3 = 128 * C, 128 * C + 128, 128 * C + 256
    for name, a, leaf in (("dw1", gp[:o1].view(128, C), w1), ("db1", gp[o1:o2], b1),
                          ("dw2", gp[o2:o3].view(1, 128), w2), ("db2", gp[o3:], b2)):
        errs[name] = _rel(a, leaf.grad)
    print(f"B={B} U={U} C={C} P={P} N={N} weighted={weighted}: " +
          ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= BAR, (k, e)
    # dz is exactly zero on the padding (every element outside the crop)
    pad = torch.ones_like(dz, dtype=torch.bool)
    pad[crop] = False
    assert pad.any() and bool((dz[pad] == 0).all())


@pytest.mark.parametrize("B,U,C,P,N", SHAPES[1:3])
def test_project_bag3d_is_bit_reproducible(B, U, C, P, N):
    import blindno
    blindno.load_library()
    t = _inputs(B, U, C, P, N, True)
    a = _run(B, U, C, P, N, t)
    b = _run(B, U, C, P, N, t)
    crop = (slice(None), slice(None), slice(0, N[0]), slice(0, N[1]), slice(0, N[2]))
    for name, x, y in zip(("ubar", "v", "dz", "grads"), a, b):
        if name == "v":
            x, y = x[crop], y[crop]             # v is written on the crop only
        assert torch.equal(x, y), name
