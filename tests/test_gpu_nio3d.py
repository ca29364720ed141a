"""Encoder3D / Encoder3D_down / NIOFP3D on the HIP device (needs a GPU).

The encoders run against tests/nio3d_ref.encoder3d in fp64 on the CPU with every LeakyReLU branch
taken from the HIP forward, exactly as test_encoder2d_matches_fp64 does (the model is piecewise
linear; a pre-activation within fp32 rounding of 0 may take either branch in two correct
evaluations).  Bars: output <= 1e-5, every gradient <= 1e-4 (conv biases ahead of a
batch-statistics BatchNorm skipped: their true gradient is exactly 0), running statistics <= 1e-5.
NIOFP3D runs against the reference's golden (tests/golden/nio3d_train*.npz) with the bars of
tests/test_nio3d_golden.py: out <= 1e-4, g.* <= 1e-3, gnorm.* within 1e-3 |v| + 1e-5 gmax.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2

import nio3d_ref
from test_nio3d_golden import CTOR, check_grads, golden_state, load_nio3d

pytestmark = pytest.mark.gpu

BLOCKS = [b[0] for b in nio3d_ref.ENC3D_BLOCKS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


@pytest.mark.parametrize("cls,depth", [("Encoder3D", 33), ("Encoder3D_down", 17)])
def test_encoder3d_matches_fp64(cls, depth):
    import blindno
    torch.manual_seed(3)
    enc = getattr(blindno, cls)(25).cuda().train()
    x = torch.randn(2, 5, 1, depth, 9, 10, device="cuda")
    masks, hooks = [], []
    for name in BLOCKS:
        hooks.append(getattr(enc, name).register_forward_hook(lambda mod, i, o: masks.append(o.detach().cpu() > 0)))
    out = enc(x)
    for h in hooks:
        h.remove()
    assert len(masks) == 10 and out.shape == (2, 5, 25)

    p64 = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point)
           for k, v in enc.state_dict().items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    stats = []
    out64 = nio3d_ref.encoder3d(p64, x.cpu().double(), masks=masks, stats=stats)
    e_out = rel_l2(out.detach().cpu().numpy(), out64.detach().numpy())
    print(f"{cls}: fwd {e_out:.2e}")
    assert e_out <= 1e-5, e_out
    cot = torch.randn(out64.shape, dtype=torch.float64)
    (out * cot.float().cuda()).sum().backward()
    (out64 * cot).sum().backward()
    worst = []
    for k, p in enc.named_parameters():
        if k.endswith("layers.0.bias"):
            continue    # conv bias ahead of a batch-statistics BatchNorm: true gradient is exactly 0
        e = rel_l2(p.grad.cpu().numpy(), p64[k].grad.numpy())
        worst.append((e, k))
        assert e <= 1e-4, (k, e)
    print(f"{cls}: worst grads {sorted(worst)[-3:]}")
    # running statistics after one step from (0, 1) with momentum 0.1, as nn.BatchNorm3d keeps them
    bufs = dict(enc.named_buffers())
    for name, (mean, var) in zip(BLOCKS, stats):
        assert rel_l2(bufs[f"{name}.layers.1.running_mean"].cpu().numpy(), (0.1 * mean).numpy()) <= 1e-5, name
        assert rel_l2(bufs[f"{name}.layers.1.running_var"].cpu().numpy(), (0.9 + 0.1 * var).numpy()) <= 1e-5, name
        assert int(bufs[f"{name}.layers.1.num_batches_tracked"]) == 1


@pytest.fixture(scope="module")
def golden_run():
    """NIOFP3D on the golden case, forward + backward on the device, once for the module."""
    import blindno
    g = load_nio3d()
    st, x = golden_state(g)
    m = blindno.NIOFP3D(*CTOR)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m = m.cuda().train()
    xd = torch.from_numpy(x).cuda()
    grid = torch.from_numpy(g["in.grid"]).cuda().requires_grad_(True)
    out = m(xd, grid, bag_idx=g["idx"])
    (out * torch.from_numpy(g["cot"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    return g, m, xd, grid, out


def test_niofp3d_matches_reference_golden(golden_run):
    g, m, xd, grid, out = golden_run
    assert tuple(out.shape) == tuple(g["out"].shape)
    e = rel_l2(out.detach().cpu().numpy(), g["out"])
    print(f"nio3d_train on the device: fwd {e:.2e}")
    assert e <= 1e-4, e
    grads = dict(m.named_parameters())
    check_grads(g, lambda k: grads[k].grad, grid.grad)
    assert m.fc0.weight.grad is None and m.fc0.bias.grad is None      # fc0 enters as .data


def test_niofp3d_train_draw_is_the_references(golden_run):
    """Without bag_idx, train mode draws the bag from numpy's global RNG as the reference does:
    seeded as the golden was, the draw is the golden's idx."""
    g, m, xd, grid, _ = golden_run
    import blindno
    m2 = blindno.NIOFP3D(*CTOR)
    m2.load_state_dict(m.state_dict())      # round trip into a fresh module
    m2 = m2.cuda().train()
    # the running statistics moved in golden_run's step; compare both modules on the same state
    m.load_state_dict(m2.state_dict())
    np.random.seed(17)
    with torch.no_grad():
        a = m2(xd, grid.detach())
        b = m(xd, grid.detach(), bag_idx=g["idx"])
    assert torch.equal(a, b)
    for (k, v), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k


def test_niofp3d_eval_uses_every_snapshot(golden_run):
    g, m, xd, grid, _ = golden_run
    m.eval()
    try:
        with torch.no_grad():
            a = m(xd, grid.detach())
            b = m(xd, grid.detach(), bag_idx=np.arange(xd.shape[1]))
        assert a.shape == (1, 33, 9, 10, 1) and torch.isfinite(a).all()
        assert torch.equal(a, b)                  # L = T
    finally:
        m.train()


def test_dropin_niofp3d_constructs_and_runs():
    code = ("import numpy as np, torch\n"
            "from NIOModules import NIOFP3D\nfrom Baselines import Encoder3D, Encoder3D_down, ConvBlock3D\n"
            "torch.manual_seed(0)\n"
            "m = NIOFP3D(3, 2, 32, 25, 2, 4, 3, 1, 'cuda', down=True).cuda().train()\n"
            "x = torch.randn(2, 60, 8, 6, 5, device='cuda')\n"
            "ax = [torch.linspace(-1, 1, n, device='cuda') for n in (8, 6, 5)]\n"
            "grid = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1).contiguous()\n"
            "np.random.seed(3)\n"
            "out = m(x, grid)\nout.square().mean().backward()\n"
            "ok = all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in m.named_parameters()"
            " if not k.startswith('fc0.'))\n"
            "print(type(m.branch).__name__, tuple(out.shape), bool(torch.isfinite(out).all()), ok)\n")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    d = os.path.join(ROOT, "dropin", "2d_FPE")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {d!r})\n" + code],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "Encoder3D_down (2, 8, 6, 5, 1) True True", r.stdout + r.stderr
