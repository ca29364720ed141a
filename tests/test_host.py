"""CPU-only checks: the C-ABI library loads (its binding is tests/test_abi.py's), module
layouts / initialisation match the reference, the product path refuses CPU tensors, and
the host-side training logic (bag draw, StepLR, data-parallel averaging) behaves like
the reference's."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

def test_error_string():
    import blindno
    lib = blindno.load_library()
    assert b"invalid" in lib.blindno_error_string(1).lower()


def test_state_dict_layouts_match_reference():
    import blindno
    lay = json.load(open(os.path.join(GOLDEN, "layouts.json")))

    def got(m):
        return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]

    assert got(blindno.NIOFP2D_FNO(2, 3, 100, 25, 3, 12, 32, 2)) == lay["2d_FPE.NIOFP2D_FNO(2,3,100,25,3,12,32,2)"]
    assert got(blindno.NIOFP2D(2, 3, 100, 25, 3, 12, 32, 2)) == lay["2d_FPE.NIOFP2D(2,3,100,25,3,12,32,2)"]
    nc = dict(heads=("fno_Fx", "fno_Fy"), branch_last_kernel=(3, 2))
    assert got(blindno.NIOFP2D_FNO(2, 3, 100, 25, 3, 12, 32, 2, **nc)) == lay["2d_NC.NIOFP2D_FNO(2,3,100,25,3,12,32,2)"]
    assert got(blindno.NIOFP2D(2, 3, 100, 25, 3, 12, 32, 2, **nc)) == lay["2d_NC.NIOFP2D(2,3,100,25,3,12,32,2)"]
    assert got(blindno.NIOFP_FNO(3, 30, 15, 2, "cpu")) == lay["1d_FPE.NIOFP_FNO(3,30,15,2)"]
    assert got(blindno.NIOFP_FNO(3, 20, 40, 1, "cpu", heads=("fno_V",))) == lay["1d_GPE.NIOFP_FNO(3,20,40,1)"]
    assert (got(blindno.NIOFP2D_FNO_attn(2, 3, 100, 25, 3, 12, 32, 2, 128, 128))
            == lay["2d.NIOFP2D_FNO_attn(2,3,100,25,3,12,32,2,128,128)"])
    assert (got(blindno.NIOFP2D_FNO_attn(2, 3, 100, 25, 3, 12, 32, 2, 128, 128, heads=("fno_Fx", "fno_Fy")))
            == lay["2d_NC.NIOFP2D_FNO_attn(2,3,100,25,3,12,32,2,128,128)"])


@pytest.mark.parametrize("case,seed,ctor", [
    ("fno2d", 304, lambda b: b.FNO2d(4, 5, 3, 3, 1)),
    ("fno2d_input61", 305, lambda b: b.FNO2d(12, 4, 2, 3, 1)),
    ("sc2d_a", 301, lambda b: b.SpectralConv2d(3, 4, 4, 3)),
    ("sc1d", 101, lambda b: b.SpectralConv1d(3, 4, 5)),
    ("fno1d", 103, lambda b: b.FNO1d(5, 6, 3, 2, 2)),
    ("nio1d_fno_train", 105, lambda b: b.NIOFP_FNO(3, 6, 5, 2, "cpu")),
    ("gpe_nio_fno_train", 201, lambda b: b.NIOFP_FNO(3, 5, 8, 1, "cpu", heads=("fno_V",))),
    ("nio2d_fno_attn_train", 401, lambda b: b.NIOFP2D_FNO_attn(2, 3, 100, 25, 2, 6, 5, 2, 20, 20)),
    ("nc_nio2d_fno_attn_train", 402,
     lambda b: b.NIOFP2D_FNO_attn(2, 3, 100, 25, 2, 6, 5, 2, 20, 20, heads=("fno_Fx", "fno_Fy"))),
])
def test_same_seed_same_initial_weights(case, seed, ctor):
    """Parameters are created in the reference's order with the reference's init, so a
    seeded construction reproduces the reference's initial weights bit for bit."""
    import blindno
    g = load_golden(case)
    torch.manual_seed(seed)
    m = ctor(blindno)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), g["p." + k]), k


def test_niofp2d_fno_init_matches_reference_with_branch():
    # the 2D model's unused Encoder2D is built first and consumes the RNG like the reference
    import blindno
    g = load_golden("nio2d_fno_train")
    torch.manual_seed(307)
    m = blindno.NIOFP2D_FNO(2, 3, 100, 25, 2, 6, 5, 2)
    for k, v in m.state_dict().items():
        if not k.startswith("branch."):
            assert np.array_equal(v.numpy(), g["p." + k]), k


def test_cpu_tensors_raise():
    import blindno
    m = blindno.FNO2d(4, 5, 2, 3, 1)
    with pytest.raises(blindno.BlindnoError):
        m(torch.randn(1, 8, 8, 3))
    nio = blindno.NIOFP2D_FNO(2, 3, 100, 25, 2, 6, 5, 2).eval()
    grid = torch.zeros(16, 16, 2)
    with pytest.raises(blindno.BlindnoError):
        nio(torch.randn(1, 60, 16, 16), grid)


def test_bag_draw_matches_reference_semantics():
    import blindno
    np.random.seed(13)
    L, idx = blindno.draw_bag(60)
    np.random.seed(13)
    L2 = np.random.randint(50, 60)
    idx2 = np.random.choice(60, L2)
    assert L == L2 and np.array_equal(idx, idx2)
    g = load_golden("nio2d_fno_train")   # the draw the reference made under seed 13
    assert L == int(g["L"]) and np.array_equal(idx, g["idx"])


def test_attn_bag_draw_is_without_replacement():
    """NIOFP2D_FNO_attn draws its bag WITHOUT replacement (2d_FPE/NIOModules.py:344-345);
    the recorded reference draw of the golden fixture is reproduced from the same seed."""
    from blindno.nio import draw_bag_distinct
    g = load_golden("nio2d_fno_attn_train")
    np.random.seed(19)
    L, idx = draw_bag_distinct(60)
    assert L == int(g["L"]) and np.array_equal(idx, g["idx"])
    assert len(set(idx.tolist())) == L
    import blindno
    m = blindno.NIOFP2D_FNO_attn(2, 3, 100, 25, 2, 6, 5, 2, 16, 16).eval()
    with pytest.raises(blindno.BlindnoError):
        m(torch.randn(1, 60, 16, 16), torch.zeros(16, 16, 2))


def test_steplr_and_accelerate_quirk():
    from blindno.train import StepLR

    class Opt:
        lr = 5e-4

    o = Opt()
    s = StepLR(o, 100, 0.5)
    for _ in range(99):
        s.step()
    assert o.lr == 5e-4
    s.step()
    assert o.lr == 2.5e-4
    o2 = Opt()
    s2 = StepLR(o2, 100, 0.5, world_steps=8)     # accelerate steps once per process
    for _ in range(13):
        s2.step()
    assert o2.lr == 5e-4 * 0.5 ** (13 * 8 // 100)


def test_pad_and_crop_geometry():
    from blindno import ops
    assert [ops.pad_amount(n) for n in (128, 61, 80, 64, 256, 18, 10)] == [32, 15, 20, 16, 64, 4, 2]
    meta = ops.FNOMeta(2, 3, 12, 32, 32, 128, 1, 12)
    g = ops._fno_geometry(torch.empty(4, 128, 128, 12), meta)
    assert g[4:] == (160, 160, 128, 128)


def test_trainer_split_is_random_split():
    """blindno.trainer's 80/20 split = torch's random_split (2d_FPE/train_fno.py:67-69) with a
    seeded generator (the reference's own split is unseeded: it differs run to run)."""
    import torch
    from torch.utils.data import random_split
    from blindno import trainer
    for seed in (0, 5):
        a, b = random_split(range(37), [29, 8], generator=torch.Generator().manual_seed(seed))
        tr, te = trainer.split_indices(37, seed)
        assert list(a) == tr and list(b) == te


# ---------------------------------------------------------------- PermInvUNet_attn
def _unet_ctors():
    from blindno import unet
    return {
        "2d.PermInvUNet_attn(1,2,1,4,(61,61))": ("unet2d", 531, lambda: unet.PermInvUNet_attn(1, 2, 1, 4, (61, 61))),
        "2d_NC.PermInvUNet_attn(1,2,1,4,(61,61))": ("nc_unet2d", 531,
                                                    lambda: unet.PermInvUNet_attn_NC(1, 2, 1, 4, (61, 61))),
        "1d.PermInvUNet_attn1D_bag(1,2,1,5,80)": ("unet1d_bag", 532,
                                                  lambda: unet.PermInvUNet_attn1D_bag(1, 2, 1, 5, 80, device="cpu")),
        "1d.PermInvUNet_attn1D(1,2,1,6,80)": ("unet1d", 533,
                                              lambda: unet.PermInvUNet_attn1D(1, 2, 1, 6, 80, device="cpu")),
        "1d_GPE.PermInvUNet_attn1D_bag(1,2,1,4,128)": (
            "unet1d_gpe_bag", 534, lambda: unet.PermInvUNet_attn1D_bag_V(1, 2, 1, 4, 128, device="cpu")),
        "1d_GPE.PermInvUNet_attn1D_bag_GPE(1,2,1,4,128,20,40)": (
            "unet1d_gpe", 535, lambda: unet.PermInvUNet_attn1D_bag_GPE(1, 2, 1, 4, 128, device="cpu", width=20,
                                                                       modes=40)),
    }


@pytest.mark.parametrize("key", list(_unet_ctors()))
def test_unet_layout_and_seeded_init_match_reference(key):
    """The UNet drop-ins (blindno.unet) have the reference's state_dict layout and, seeded, its
    initial weights (fingerprints captured by tests/golden/make_golden_unet.py)."""
    lay = json.load(open(os.path.join(GOLDEN, "layouts.json")))
    tag, seed, ctor = _unet_ctors()[key]
    torch.manual_seed(seed)
    m = ctor()
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    assert got == lay[key]
    fname = "unet1d_gpe" if tag.startswith("unet1d_gpe") else ("unet1d" if tag.startswith("unet1d") else tag)
    fp = np.load(os.path.join(GOLDEN, fname + "_init.npz"))
    for k, v in m.state_dict().items():
        a = (torch.view_as_real(v) if v.is_complex() else v).double().reshape(-1).numpy()
        ref = fp[f"{tag}|{k}"]
        head = np.zeros(4)
        head[:min(4, a.size)] = a[:4]
        np.testing.assert_array_equal(head, ref[2:], err_msg=k)
        np.testing.assert_allclose([a.sum(), (a * a).sum()], ref[:2], rtol=1e-12, atol=1e-12, err_msg=k)
