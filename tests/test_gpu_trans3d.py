"""Transolver3D and NIOFP3D_Trans on the GPU: the fused plane MLP against the five-launch path it
replaces inside one block, the model against the float64 restatement tests/transolver3d_ref.py
with the golden's weights on three meshes, and the train step against the reference's own fp32
run (tests/golden/nio3d_trans_train.npz), deduplicated and with the duplicates kept.

Bar of the comparisons with float64: rel-L2 <= max(1e-5, 3 x e32), e32 the error of the same
restatement run in fp32 on the CPU against float64 on the same inputs and parameters.
"""
import pytest
import torch
import torch.nn.functional as F

import transolver3d_ref as t3

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def _golden_weights():
    from test_transolver3d_ref import model_case
    _, st = model_case()
    return {k: torch.from_numpy(v) for k, v in st.items()}


def _five_launch_mlp(block):
    """The block's ln_2 + mlp + residual as TransolverBlock2D composes it: LayerNormPlanesFn, a
    1x1x1 convolution, torch's GELU, another 1x1x1 convolution and torch's add."""
    from blindno import ops
    pre, post, ln = block.mlp.linear_pre[0], block.mlp.linear_post, block.ln_2

    def forward(x, res=None, ln=ln):
        h = ops.LayerNormPlanesFn.apply(x, ln.weight, ln.bias, ln.eps)
        h = ops.conv3d(h, pre.weight.view(32, 32, 1, 1, 1), pre.bias, 1, 0)
        return ops.conv3d(F.gelu(h), post.weight.view(32, 32, 1, 1, 1), post.bias, 1, 0) + res
    return forward


def test_fused_mlp_against_five_launches_in_a_block(monkeypatch):
    import blindno
    mesh, S = (6, 7, 7), 2
    N = mesh[0] * mesh[1] * mesh[2]
    sd = {k[len("blocks.1."):]: v for k, v in _golden_weights().items() if k.startswith("blocks.1.")}
    g = torch.Generator().manual_seed(31)
    fx, dy = torch.randn(S, 32, N, generator=g), torch.randn(S, 32, N, generator=g)

    def reference(dt):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        y = t3.block3d(p, fx.to(dt), mesh, last=False)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), {k: v.grad for k, v in p.items()}
    y64, g64 = reference(torch.float64)
    y32, g32 = reference(torch.float32)
    block = blindno.TransolverBlock3D(4, 32, H=mesh[0], W=mesh[1], D=mesh[2])
    block.load_state_dict(sd, strict=True)
    block = block.cuda()

    def run():
        block.zero_grad(set_to_none=True)
        y = block(fx.view(S, 32, *mesh).cuda())
        (y * dy.view(S, 32, *mesh).cuda()).sum().backward()
        return y.detach().reshape(S, 32, N), {k: p.grad.clone() for k, p in block.named_parameters()}
    yf, gf = run()
    monkeypatch.setattr(block.mlp, "forward", _five_launch_mlp(block))
    y5, g5 = run()
    bad = []
    for name, fused, five, want, fp32 in [("y", yf, y5, y64, y32)] + [(k, gf[k], g5[k], g64[k], g32[k]) for k in sorted(gf)]:
        bar = max(1e-5, 3 * rel(fp32, want))
        ef, e5, d = rel(fused, want), rel(five, want), rel(fused, five)
        print(f"{name:34s} fused {ef:.2e}  five launches {e5:.2e}  fused vs five {d:.2e}  bar {bar:.2e}")
        if ef > bar or d > bar:
            bad.append((name, ef, d, bar))
    assert len(gf) == len(g64) == 20 and not bad, bad


@pytest.mark.parametrize("mesh", [(5, 6, 7), (6, 7, 7), (8, 8, 8)])
def test_transolver3d_against_float64(mesh):
    """210 points (below one workgroup, unequal axes), 294 and 512 points, S = 3."""
    import blindno
    S, N = 3, mesh[0] * mesh[1] * mesh[2]
    sd = _golden_weights()
    g = torch.Generator().manual_seed(N)
    inp, dy = torch.randn(S, 4, N, generator=g), torch.randn(S, 1, N, generator=g)

    def reference(dt):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        y = t3.transolver3d(p, inp.to(dt), mesh)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}
    y64, g64 = reference(torch.float64)
    y32, g32 = reference(torch.float32)
    assert "placeholder" not in g64 and len(g64) == 68
    m = blindno.Transolver3D(H=mesh[0], W=mesh[1], D=mesh[2])
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    y = m.forward_planes(inp.view(S, 4, *mesh).cuda())
    (y * dy.view(S, 1, *mesh).cuda()).sum().backward()
    e, bar = rel(y.reshape(S, 1, N), y64), max(1e-5, 3 * rel(y32, y64))
    print(f"{mesh} forward rel-L2 {e:.2e} bar {bar:.2e}")
    bad = [("y", e, bar)] if e > bar else []
    for k, p in m.named_parameters():
        if k == "placeholder":
            assert p.grad is None
            continue
        e, bar = rel(p.grad, g64[k]), max(1e-5, 3 * rel(g32[k], g64[k]))
        print(f"{mesh} {k:40s} rel-L2 {e:.2e} bar {bar:.2e}")
        if e > bar:
            bad.append((k, e, bar))
    assert not bad, bad
    # the reference's (S, N, C) signature gives the same numbers
    pts = inp.transpose(1, 2).cuda()
    with torch.no_grad():
        y2 = m(pts[..., :3], pts[..., 3:])
    assert torch.equal(y2.reshape(-1), y.detach().reshape(-1))


def test_train_step_against_reference_golden():
    """NIOFP3D_Trans against the reference composition's fp32 run: output, loss, the gradient of
    every trained parameter (bars of tests/test_transolver3d_ref.py), none for fc0 and the
    placeholder; and the deduplicated bag against the same bag with its duplicates kept."""
    import blindno
    from blindno import nio
    from conftest import rel_l2
    from test_transolver3d_ref import G_TOL, OUT_TOL, nio_case
    g, st, x = nio_case()
    m = blindno.NIOFP3D_Trans(*[int(v) for v in g["ctor"]], "cuda", tuple(int(v) for v in g["x_shape"][2:]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m = m.cuda().train()
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g["in.grid"]).cuda()
    target = torch.from_numpy(g["target"]).cuda()
    idx = g["idx"]

    def step(dedup):
        nio.DEDUP_BAGS = dedup
        try:
            m.zero_grad(set_to_none=True)
            xs, L, lw = nio._select(m, xd, idx, dedup=True)
            assert (L, lw is not None) == ((3, True) if dedup else (8, False))
            out = m(xd, gd, bag_idx=idx)
            loss = F.mse_loss(out, target)
            loss.backward()
            return out.detach(), loss.item(), {k: p.grad for k, p in m.named_parameters()}
        finally:
            nio.DEDUP_BAGS = True
    out, loss, grads = step(True)
    e = rel_l2(out.cpu().numpy(), g["out"])
    print(f"output rel-L2 {e:.2e} (bar {OUT_TOL}); loss {loss:.8e} against {float(g['loss']):.8e}")
    assert e <= OUT_TOL and abs(loss - float(g["loss"])) <= OUT_TOL * float(g["loss"])
    worst = (None, 0.0)
    for k, v in g.items():
        if k.startswith("g."):
            gr = grads[k[2:]]
            assert gr is not None, k
            gr = (torch.view_as_real(gr) if gr.is_complex() else gr).cpu().numpy()
            e = rel_l2(gr, v)
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e <= G_TOL, (k, e)
    print(f"worst gradient {worst[0]} rel-L2 {worst[1]:.2e} (bar {G_TOL})")
    for k, gr in grads.items():
        unused = k.startswith("fc0.") or k == "trans_input.placeholder"
        assert (gr is None) == unused and unused == ("g." + k not in g), k
    assert float(grads["trans_input.blocks.2.Attn.temperature"].abs().max()) == 0.0   # all four clamped
    grads = {k: v.clone() for k, v in grads.items() if v is not None}
    out_k, loss_k, grads_k = step(False)
    e = rel_l2(out_k.cpu().numpy(), out.cpu().numpy())
    print(f"dedup vs kept: out rel-L2 {e:.2e}")
    assert e <= OUT_TOL
    for k, v in grads.items():
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (v, grads_k[k]))
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= G_TOL, k
    with pytest.raises(ValueError, match="7 x 6 x 5"):
        m(torch.zeros(1, 6, 5, 6, 7, device="cuda"), torch.zeros(5, 6, 7, 3, device="cuda"))
