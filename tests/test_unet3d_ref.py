"""PermInvUNet_attn3D without a GPU: the float64 restatements of tests/unet3d_ref.py pinned to
torch.nn.functional, the properties the device tests rely on (adjoint identity, bag-order
invariance, per-axis sizes and pads), the model's state_dict layout, the trainer entry and the
case tables' placement on the kernel paths they name.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2

import unet3d_ref as R

F64 = torch.float64


@pytest.mark.parametrize("name", list(R.DW_CASES))
def test_depthwise_formula_is_grouped_conv3d(name):
    N, C, D, H, W, k, bias = R.DW_CASES[name]
    torch.manual_seed(1)
    x = torch.randn(N, C, D, H, W, dtype=F64)
    w = torch.randn(C, 1, *k, dtype=F64)
    b = torch.randn(C, dtype=F64) if bias else None
    ref = F.conv3d(x, w, b, padding=tuple(e // 2 for e in k), groups=C)
    assert rel_l2(R.dwconv3d(x, w, b), ref) <= 1e-13


@pytest.mark.parametrize("name", list(R.DW_CASES))
def test_depthwise_adjoint_identity(name):
    """<dwconv(x), g> = <x, bwd_data(g)> with bwd_data the convolution on the reflected taps."""
    N, C, D, H, W, k, _ = R.DW_CASES[name]
    torch.manual_seed(2)
    x, g = torch.randn(2, N, C, D, H, W, dtype=F64)
    w = torch.randn(C, 1, *k, dtype=F64)
    lhs = float((R.dwconv3d(x, w) * g).sum())
    rhs = float((x * R.dwconv3d_bwd_data(g, w)).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))
    xr = x.clone().requires_grad_(True)
    (R.dwconv3d(xr, w) * g).sum().backward()
    assert rel_l2(R.dwconv3d_bwd_data(g, w), xr.grad) <= 1e-13


@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool_is_max_pool3d(name):
    N, C, D, H, W, k = R.POOL_CASES[name]
    torch.manual_seed(3)
    x = torch.randn(N, C, D, H, W, dtype=F64)
    x[0, 0, :2, :2, :2] = 1.5                        # a tie: the first maximum in scan order wins
    x[1, 1, 0, 1, 1] = float("nan")                  # a NaN wins
    xr, xt = (x.clone().requires_grad_(True) for _ in range(2))
    y, arg = R.maxpool3d(xr, k)
    yt = F.max_pool3d(xt, k)
    assert torch.equal(torch.nan_to_num(y.detach(), nan=7e7), torch.nan_to_num(yt.detach(), nan=7e7))
    assert torch.isnan(y[1, 1, 0, 0, 0]) and int(arg[0, 0, 0, 0, 0]) == 0
    g = torch.randn(y.shape, dtype=F64)
    (y * g).sum().backward()
    (yt * g).sum().backward()
    assert torch.equal(xr.grad, xt.grad)
    if name == "floor":
        assert tuple(y.shape[2:]) == (2, 3, 4)
        assert float(xr.grad[:, :, 4].abs().max()) == 0 and float(xr.grad[..., 8].abs().max()) == 0


def test_convt_is_conv_transpose3d():
    N, Ci, Co, di, do = R.CONVT_CASE
    op = tuple(o - 2 * i for o, i in zip(do, di))
    assert op == (1, 0, 1)
    torch.manual_seed(4)
    x = torch.randn(N, Ci, *di, dtype=F64)
    w = torch.randn(Ci, Co, 2, 2, 2, dtype=F64)
    b = torch.randn(Co, dtype=F64)
    y = R.convt3d(x, w, b, do)
    assert rel_l2(y, F.conv_transpose3d(x, w, b, stride=2, output_padding=op)) <= 1e-14
    assert torch.equal(y[:, :, 4], b.view(1, Co, 1, 1).expand(N, Co, do[1], do[2]))   # padded planes: the bias
    assert torch.equal(y[..., 8], b.view(1, Co, 1, 1).expand(N, Co, do[0], do[1]))


def _ref_model():
    import blindno
    c = R.MODEL
    torch.manual_seed(7)
    m = blindno.PermInvUNet_attn3D(1, 2, c["base_ch"], c["depth"], c["input_size"], width=c["width"],
                                   modes=c["modes"])
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_reference_model_is_invariant_under_a_bag_permutation():
    c = R.MODEL
    _, st = _ref_model()
    torch.manual_seed(8)
    x = torch.randn(c["B"], c["T"], *c["input_size"], dtype=F64)
    p = {k: (v.to(torch.complex128) if v.is_complex() else v.to(F64)) if v.is_floating_point() or v.is_complex()
         else v for k, v in st.items()}
    with torch.no_grad():
        a = R.unet3d(p, x, c["depth"], idx=c["bag"])
        b = R.unet3d(p, x, c["depth"], idx=c["bag"][::-1])
        e = R.unet3d(p, x, c["depth"], idx=[0, 3, 5, 1])        # the duplicate counts
    assert tuple(a.shape) == (c["B"], *c["input_size"], 2)
    assert rel_l2(b, a) <= 1e-12
    assert rel_l2(e, a) > 1e-6


def test_sizes_and_pads_per_axis():
    from blindno.unet3d import _sizes_and_pads
    assert _sizes_and_pads(40, 3) == ([40, 20, 10, 5], [0, 0, 0])
    assert _sizes_and_pads(37, 3) == ([37, 18, 9, 4], [1, 0, 1])
    import blindno
    m = blindno.PermInvUNet_attn3D(1, 2, 1, 3, (37, 40, 37))
    assert [u.output_padding for u in m.up_transposes] == [(1, 0, 1), (0, 0, 0), (1, 0, 1)]
    assert [t.D for t in m.temp_atts] == [37 * 40 * 37, 2 * 18 * 20 * 18, 4 * 9 * 10 * 9, 8 * 4 * 5 * 4]


def test_layout_matches_fixture_and_module_imports_without_a_gpu():
    import blindno
    import blindno.unet3d as u3
    lay = json.load(open(os.path.join(GOLDEN, "layouts_unet3d.json")))

    def layout(m):
        return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]

    assert layout(blindno.PermInvUNet_attn3D()) == lay["PermInvUNet_attn3D(1,2,1,3,(40,40,40))"]
    m, _ = _ref_model()
    assert layout(m) == lay["PermInvUNet_attn3D(1,2,2,2,(9,12,10),width=4,modes=2)"]
    assert m.unused_prefixes == ("skip_norms.2.",)
    assert [n for n, _ in m.named_children()] == ["down_convs", "pools", "skip_norms", "temp_atts", "up_transposes",
                                                  "up_convs", "final_conv", "fno"]
    assert u3.DW3D_TILE == R.TILE
    for bad in (torch.zeros(2, 6, 9, 12), torch.zeros(2, 6, 9, 12, 11)):
        with pytest.raises(ValueError, match="expected x"):
            m(bad)


def test_unet3d_queries_without_a_device():
    from blindno import _lib
    q = _lib.query
    assert q("blindno_dwconv3d_wgrad_nsplit", 1, 1, 6, 11, 41, 7, 7, 7) == 8      # capped by the 8 work items
    assert q("blindno_dwconv3d_wgrad_nsplit", 400, 1, 40, 40, 40, 7, 7, 7) == 147  # ceil(1024 / 7)
    assert q("blindno_dwconv3d_wgrad_nsplit", 2, 2, 6, 11, 41, 7, 4, 7) == -1
    assert q("blindno_dwconv3d_wgrad_nsplit", 2, 2, 6, 11, 41, 9, 7, 7) == -1
    assert q("blindno_convt3d_wgrad_nparts", 4, 20, 20, 20) == 4 * 125


def test_trainer_has_the_3d_unet_experiment():
    from blindno import data, trainer, unet3d
    e = trainer.experiments_for("unet")["3d_FPE"]
    assert (e.dim, e.dataset, e.lr, e.batch, e.save_interval, e.result_dir, e.eager) == \
        (3, data.TrajectoryDataset3D, 5e-4, 4, 5, "results_3d_FPE_unet", True)
    two_d = trainer.experiments_for("unet")["2d_FPE"]
    assert (e.lr, e.batch, e.save_interval) == (two_d.lr, two_d.batch, two_d.save_interval)
    m = e.model(16, "cpu")
    assert isinstance(m, unet3d.PermInvUNet_attn3D) and m.input_size == (16, 16, 16) and m.depth == 3
    assert "3d_FPE" not in trainer.experiments_for("nio")


def test_cases_sit_on_the_paths_they_name():
    t = R.TILE
    N, C, D, H, W, k, _ = R.DW_CASES["tile_edges"]
    assert C == 1 and (D, H, W) == tuple(e + 1 for e in t) and R.dw_tiles(D, H, W) == (2, 2, 2)
    N, C, D, H, W, k, _ = R.DW_CASES["all_padding"]
    assert (N, C, D, H, W) == (2, 3, 5, 9, 11) and D < k[0]
    assert {R.DW_CASES["k117"][5], R.DW_CASES["k357"][5]} == {(1, 1, 7), (3, 5, 7)}
    assert R.DW_CASES["no_bias"][6] is False
    N, C, D, H, W, k, _ = R.DW_WGRAD_CASE
    items = N * int(np.prod(R.dw_tiles(D, H, W)))
    for ns in R.DW_WGRAD_SPLITS:
        per = -(-items // ns)
        assert all(min(items, (s + 1) * per) > s * per for s in range(ns))     # no empty range
    assert max(R.DW_WGRAD_SPLITS) > 1
    N, C, D, H, W, kp = R.POOL_CASES["floor"]
    assert (D, H, W) == (5, 7, 9) and all(n % 2 for n in (D, H, W))
    assert R.POOL_CASES["w122"][5] == (1, 2, 2)
    c = R.MODEL
    assert len(set(c["input_size"])) == 3 and any(n % 2 for n in c["input_size"])
    assert len(set(c["bag"])) < len(c["bag"])
