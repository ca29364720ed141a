"""The float64 projection references of tests/projection_ref.py checked on the host, without a GPU:

* they equal float64 torch autograd of F.linear / F.gelu / F.linear on the cropped, permuted field
  (dout_div broadcast and lscale included), and the bag reference equals the per-snapshot
  projection followed by the weighted mean, to 1e-12 rel-L2;
* a plain fp32 torch evaluation of the same formulas on the CPU stays inside the derived bounds of
  projection_ref (module docstring there) on the inputs of every GPU case -- the bounds are loose
  enough for a correct fp32 implementation; the worst err / bound ratio of each case is printed;
* those inputs give max |h| <= 12 in float64, the range of csrc/common.h's GELU error;
* the modulus twins dominate.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import projection_ref as pr
from conftest import rel_l2


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _torch_project(t, c, dtype, lscale):
    """(out, dz on the crop, flat grads) by torch autograd in `dtype`."""
    Ho, Wo = c["N"]
    z = _t(t["z"], dtype)[:, :, :Ho, :Wo].clone().requires_grad_(True)
    w1, b1, w2, b2 = (_t(t[k], dtype).requires_grad_(True) for k in ("w1", "b1", "w2", "b2"))
    out = F.linear(F.gelu(F.linear(z.permute(0, 2, 3, 1), w1, b1)), w2, b2)
    n = torch.arange(c["Bn"])
    g = _t(t["dout"], dtype)[n // c["dout_div"]]
    if lscale is not None:
        g = g * _t(lscale, dtype)[n % c["dout_div"]].view(-1, 1, 1, 1)
    gz, g1, gb1, g2, gb2 = torch.autograd.grad(out, (z, w1, b1, w2, b2), g)
    grads = torch.cat([g1.reshape(-1), gb1, g2.reshape(-1), gb2])
    return out.detach().double().numpy(), gz.double().numpy(), grads.double().numpy()


def _variants(c):
    """lscale settings of a case: the broadcast cases run with and without the weights."""
    return (False, True) if c["id"].startswith("div3") else (False,)


@pytest.mark.parametrize("c", pr.MFMA_CASES[::7] + pr.BCAST_CASES[::3] + pr.FALLBACK_BWD_CASES[1::4],
                         ids=lambda c: c["id"])
def test_reference_equals_fp64_autograd(c):
    t = pr.case_inputs(c)
    for use_ls in (False, True):
        ls = t["lscale"] if use_ls else None
        out, gz, grads = _torch_project(t, c, torch.float64, ls)
        assert rel_l2(pr.project_fwd(t["z"], t["w1"], t["b1"], t["w2"], t["b2"], *c["N"]), out) <= 1e-12
        dz, gr = pr.project_bwd(t["z"], t["w1"], t["b1"], t["w2"], t["dout"], *c["N"], c["dout_div"], ls)
        assert rel_l2(dz, gz) <= 1e-12 and rel_l2(gr, grads) <= 1e-12


@pytest.mark.parametrize("c", pr.ALL_CASES, ids=lambda c: c["id"])
def test_fp32_evaluation_is_inside_the_bound(c):
    for seed in ((0, 1) if c["id"].startswith("g2") else (0,)):
        t = pr.case_inputs(c, seed)
        a = (t["z"], t["w1"], t["b1"], t["w2"])
        hmax = pr.max_abs_h(t["z"], t["w1"], t["b1"], *c["N"])
        assert hmax <= 12.0
        for use_ls in _variants(c):
            ls = t["lscale"] if use_ls else None
            out, gz, grads = _torch_project(t, c, torch.float32, ls)
            r = {}
            if "fwd" in c["kinds"]:
                r["out"] = pr.worst(np.abs(out - pr.project_fwd(*a, t["b2"], *c["N"])),
                                    pr.project_fwd_bound(*a, t["b2"], *c["N"]))
            if "bwd" in c["kinds"]:
                k = (t["dout"], *c["N"], c["dout_div"], ls)
                (dz, gr), (bz, bg) = pr.project_bwd(*a, *k), pr.project_bwd_bound(*a, *k)
                r["dz"], r["grads"] = pr.worst(np.abs(gz - dz), bz), pr.worst(np.abs(grads - gr), bg)
            print(f"{c['id']} seed={seed} lscale={use_ls}: max|h| {hmax:.2f}, CPU fp32 worst err/bound " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert max(r.values()) < 1.0, r


def test_gridcap_case_fp32_and_range():
    """The forward grid-cap case, one sample at a time (its float64 hidden layer is 67 MB a sample)."""
    c = pr.GRIDCAP_CASE
    t = pr.case_inputs(c)
    worst, hmax = 0.0, 0.0
    for n in range(0, c["Bn"], 4):                       # every fourth sample: same weights, same law
        z = t["z"][n:n + 1]
        a = (z, t["w1"], t["b1"], t["w2"], t["b2"], *c["N"])
        o32 = F.linear(F.gelu(F.linear(_t(z, torch.float32)[:, :, :256, :256].permute(0, 2, 3, 1), _t(t["w1"], torch.float32),
                                       _t(t["b1"], torch.float32))), _t(t["w2"], torch.float32), _t(t["b2"], torch.float32))
        worst = max(worst, pr.worst(np.abs(o32.double().numpy() - pr.project_fwd(*a)), pr.project_fwd_bound(*a)))
        hmax = max(hmax, pr.max_abs_h(z, t["w1"], t["b1"], *c["N"]))
    print(f"{c['id']}: max|h| {hmax:.2f}, CPU fp32 worst err/bound out {worst:.3f}")
    assert worst < 1.0 and hmax <= 12.0


def _torch_bag(t, case, dtype):
    """(ubar, v, dz, grads): the per-snapshot projection, the weighted mean and autograd in `dtype`."""
    B, U, C, P, N = case
    z = _t(t["z"], dtype)[:, :, :N[0], :N[1]].clone().requires_grad_(True)
    w1, b1, w2, b2 = (_t(t[k], dtype).requires_grad_(True) for k in ("w1", "b1", "w2", "b2"))
    lw = torch.full((U,), 1.0 / U, dtype=dtype) if t["lw"] is None else _t(t["lw"], dtype)
    h = F.linear(z.permute(0, 2, 3, 1), w1, b1)
    proj = F.linear(F.gelu(h), w2, b2).reshape(B, U, N[0] * N[1])
    ubar = (lw.view(1, U, 1) * proj).sum(1)
    gz, g1, gb1, g2, gb2 = torch.autograd.grad(ubar, (z, w1, b1, w2, b2), _t(t["gs"], dtype))
    hd = h.detach()
    gd = 0.5 * (1.0 + torch.erf(hd * 0.7071067811865476)) + hd * torch.exp(-0.5 * hd * hd) * 0.3989422804014327
    v = ((gd * w2.detach().view(-1)) @ w1.detach()).permute(0, 3, 1, 2)
    grads = torch.cat([g1.reshape(-1), gb1, g2.reshape(-1), gb2])
    return [x.detach().double().numpy() for x in (ubar, v, gz, grads)]


@pytest.mark.parametrize("weighted", [False, True], ids=["lw_null", "lw_counts"])
@pytest.mark.parametrize("case", pr.BAG_CASES, ids=pr.bag_id)
def test_bag_reference_and_fp32_bound(case, weighted):
    B, U, C, P, N = case
    t = pr.bag_inputs(case, weighted)
    a = (t["z"], t["w1"], t["b1"], t["w2"])
    ubar, v = pr.bag_fwd(*a, t["b2"], t["lw"], U, *N)
    dz, gr = pr.bag_bwd(*a, t["lw"], U, t["gs"], *N)
    for got, ref in zip(_torch_bag(t, case, torch.float64), (ubar, v, dz, gr)):
        assert rel_l2(ref, got) <= 1e-12
    # the bag backward is the projection backward with the broadcast dout_div = U and lscale = lw
    lw = np.full(U, 1.0 / U) if t["lw"] is None else t["lw"]
    dz2, gr2 = pr.project_bwd(*a, t["gs"].reshape(B, *N, 1), *N, U, lw)
    assert rel_l2(dz, dz2) <= 1e-12 and rel_l2(gr, gr2) <= 1e-12
    hmax = pr.max_abs_h(t["z"], t["w1"], t["b1"], *N)
    bu, bv = pr.bag_fwd_bound(*a, t["b2"], t["lw"], U, *N)
    bz, bg = pr.bag_bwd_bound(*a, t["lw"], U, t["gs"], *N)
    r = {k: pr.worst(np.abs(g - ref), b)
         for k, g, ref, b in zip(("ubar", "v", "dz", "grads"), _torch_bag(t, case, torch.float32), (ubar, v, dz, gr),
                                 (bu, bv, bz, bg))}
    print(f"bag {pr.bag_id(case)} weighted={weighted}: max|h| {hmax:.2f}, CPU fp32 worst err/bound " +
          ", ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert max(r.values()) < 1.0 and hmax <= 12.0
    # the twins dominate
    ua, va = pr.bag_fwd_abs(*a, t["b2"], t["lw"], U, *N)
    dza, ga = pr.bag_bwd_abs(*a, t["lw"], U, t["gs"], *N)
    for x, xa in ((ubar, ua), (v, va), (dz, dza), (gr, ga)):
        assert np.all(np.abs(x) <= xa * (1 + 1e-12))


def test_abs_twins_dominate():
    c = pr.BCAST_CASES[-1]
    t = pr.case_inputs(c)
    a = (t["z"], t["w1"], t["b1"], t["w2"])
    assert np.all(np.abs(pr.project_fwd(*a, t["b2"], *c["N"])) <= pr.project_fwd_abs(*a, t["b2"], *c["N"]) * (1 + 1e-12))
    k = (t["dout"], *c["N"], 3, t["lscale"])
    for x, xa in zip(pr.project_bwd(*a, *k), pr.project_bwd_abs(*a, *k)):
        assert np.all(np.abs(x) <= xa * (1 + 1e-12))


def test_case_tables_name_every_instantiation():
    """Every matrix-core instantiation CK x COM x T16 (16 forward, 16 backward) and every reachable
    fall-back instantiation is named by a case id."""
    ids = [c["id"] for c in pr.MFMA_CASES]
    for ck in (4, 8, 12, 16):
        for com in (1, 2):
            for t in ("t16", "pt"):
                assert any(f"_ck{ck}_com{com}_{t}" in i for i in ids), (ck, com, t)
    fwd = {i.split("_cm")[1] for i in (c["id"] for c in pr.FALLBACK_FWD_CASES)}
    assert fwd == {f"{cm}_com{co}" for cm in (4, 8, 16, 32) for co in (1, 4)}
    bwd = {i.split("_cm")[1] for i in (c["id"] for c in pr.FALLBACK_BWD_CASES)}
    assert bwd == {f"{cm}_jw8_com{co}" for cm in (8, 16, 32) for co in (1, 4)} - {"8_jw8_com1"}
