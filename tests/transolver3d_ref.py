"""Restatements, in plain torch and any precision (float64 as the checker, float32 for the error
floor), of the fused plane MLP (include/blindno_planemlp.h), of the structured-mesh 3D Transolver
(model/Transolver_Structured_Mesh_3D.py, Physics_Attention_Structured_Mesh_3D of
model/Physics_Attention.py:119-175) and of NIOFP3D_Trans, for tests/test_transolver3d_ref.py,
tests/test_gpu_planemlp.py and tests/test_gpu_trans3d.py.  The attention after its convolutions,
the LayerNorm, the Linear and the GELU are tests/transolver_ref.py's: they see N points and no
mesh.

  plane_mlp      W2 gelu(W1 u + b1) + b2 (+ res) on planes, u = LayerNorm(x) or x
  block3d        Transolver_block on planes (S, 32, N) of an (H, W, D) mesh
  transolver3d   the model on point features (S, 4, N) -> (S, 1, N)
  niofp3d_trans  the whole model: Transolver per snapshot, bag mean with fc0, the FNO3d head
"""
import torch
import torch.nn.functional as F

import fno3d_ref
import oracle.fno_ref as ref
import transolver_ref as tr


def plane_mlp(x, W1, b1, W2, b2, res=None, gamma=None, beta=None, eps=1e-5):
    """x (S, Cin, N) -> (S, Cout, N)."""
    u = x if gamma is None else tr.layer_norm(x, gamma, beta, eps)
    z = torch.einsum("ji,sin->sjn", W1, u) + b1.view(1, -1, 1)
    y = torch.einsum("oj,sjn->son", W2, tr._gelu(z)) + b2.view(1, -1, 1)
    return y if res is None else y + res


def block3d(p, fx, mesh, last, uniform=False, record=None):
    """Transolver_block on planes fx (S, 32, N), N = H W D in the mesh's row-major order."""
    S, C, N = fx.shape
    x = tr.layer_norm(fx, p["ln_1.weight"], p["ln_1.bias"]).reshape(S, C, *mesh)
    xm = F.conv3d(x, p["Attn.in_project_x.weight"], p["Attn.in_project_x.bias"], padding=1).reshape(S, C, N)
    fm = F.conv3d(x, p["Attn.in_project_fx.weight"], p["Attn.in_project_fx.bias"], padding=1).reshape(S, C, N)
    a = tr.phys_attn(xm, fm, p["Attn.temperature"], p["Attn.in_project_slice.weight"],
                     p["Attn.in_project_slice.bias"], p["Attn.to_q.weight"], p["Attn.to_k.weight"],
                     p["Attn.to_v.weight"], p["Attn.to_out.0.weight"], p["Attn.to_out.0.bias"], res=fx,
                     uniform=uniform)
    if record is not None:
        record.append(a["w"].detach())
    fx = a["y"]
    fx = plane_mlp(fx, p["mlp.linear_pre.0.weight"], p["mlp.linear_pre.0.bias"], p["mlp.linear_post.weight"],
                   p["mlp.linear_post.bias"], res=fx, gamma=p["ln_2.weight"], beta=p["ln_2.bias"])
    if last:
        return tr._lin(tr.layer_norm(fx, p["ln_3.weight"], p["ln_3.bias"]), p, "mlp2")
    return fx


def transolver3d(p, inp, mesh, n_layers=3, uniform=False, record=None):
    """Model.forward on planes: inp (S, 4, N) = cat((x, fx), -1) transposed -> (S, 1, N).  ``p``
    holds the Model's state_dict (any dtype; the computation runs in inp's)."""
    fx = plane_mlp(inp, p["preprocess.linear_pre.0.weight"], p["preprocess.linear_pre.0.bias"],
                   p["preprocess.linear_post.weight"], p["preprocess.linear_post.bias"])
    for i in range(n_layers):
        fx = block3d(ref.sub_params(p, f"blocks.{i}"), fx, mesh, i == n_layers - 1, uniform, record)
    return fx


def trans3d_bag_field(p, x, grid, idx=None, uniform=False, record=None, dt=torch.float64):
    """The field the head reads: fc0([grid, mean_l Transolver(snapshot l)]) (B, nx, ny, nz, width).
    The bag is taken literally: every drawn snapshot is encoded, repeats included."""
    x = x.to(dt)
    if idx is not None:
        x = x[:, list(idx)]
    B, L = x.shape[:2]
    mesh = tuple(x.shape[2:])
    P = mesh[0] * mesh[1] * mesh[2]
    g = grid.to(dt)
    gp = g.permute(3, 0, 1, 2).reshape(1, 3, P).expand(B * L, 3, P)
    inp = torch.cat((x.reshape(B * L, 1, P), gp), 1)                 # [rho, gx, gy, gz]
    tp = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in ref.sub_params(p, "trans_input").items()}
    u = transolver3d(tp, inp, mesh, uniform=uniform, record=record).reshape(B, L, *mesh)
    w0, b0 = p["fc0.weight"].detach().to(dt), p["fc0.bias"].detach().to(dt)
    return (g @ w0[:, :3].t()).unsqueeze(0) + u.mean(1).unsqueeze(-1) * w0[:, 3] + b0


def niofp3d_trans(p, x, grid, idx=None, uniform=False, record=None):
    """NIOFP3D_Trans.forward in float64 (``idx`` replaces the train-mode draw; None = eval)."""
    h = trans3d_bag_field(p, x, grid, idx, uniform, record, torch.float64)
    return fno3d_ref.fno3d(ref.sub_params(p, "fno"), h)
