"""NIOFP2D_Trans_attn (2d_FPE/NIOModules.py:169-296) without a GPU: the identities the kernels rest
on (the reduced form on the distinct tokens against the literal form on the materialised bag, in
float64), the golden against the restatement, the state_dict layout against the reference's
(tests/golden/layouts_trans_attn.json, written by make_golden_trans_attn.py), the seeded
construction order, the trainer's table and the C ABI binding of include/blindno_bagattn_mix.h.

The kernels themselves are compared with the restatement on the GPU (tests/test_gpu_bagattn_mix.py,
tests/test_gpu_trans_attn.py).
"""
import json
import os

import numpy as np
import pytest
import torch

import bagattn_mix_cases as C
import trans_attn_ref as R
import transolver_ref as tr
from conftest import GOLDEN, load_golden, rel_l2
from recipe import make_array

OUT_TOL, G_TOL = 1e-4, 1e-3          # the bars of tests/test_transolver_ref.py

CTOR = (2, 3, 100, 25, 3, 12, 32, 2, 61, 61)


def golden_case():
    """(golden arrays, recipe state with the generator's rescaling, x) of nio2d_trans_attn_train."""
    g = load_golden("nio2d_trans_attn_train")
    shapes = [(k, tuple(sh)) for k, sh in json.loads(str(g["layout_json"]))]
    st = tr.rescaled_state(shapes, int(g["recipe_seed"]), json.loads(str(g["rescale_json"])))
    x = make_array(tuple(int(n) for n in g["x_shape"]), int(g["recipe_seed"]), "nio2d_trans_attn.x")
    return g, st, x


@pytest.mark.parametrize("counts", [[3, 1, 1, 2, 1, 1, 4], None])
def test_reduced_form_equals_literal_form(counts):
    """The formulas of include/blindno_bagattn_mix.h against the reference's sequence on the
    materialised L + 2 tokens, float64: forward and all gradients to 1e-11."""
    gen = torch.Generator().manual_seed(5)
    B, U, S, width = 2, 7, 50, 5
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    u, grid = (0.5 * r(B, U, S)).requires_grad_(True), r(S, 2).requires_grad_(True)
    W, bias, dy = r(width, 3), r(width), r(B, S, width)
    y, A = R.literal(u, grid, W, bias, counts)
    du, dg = torch.autograd.grad((y * dy).sum(), (u, grid))
    y2, P, rk = R.reduced(u, grid, W, bias, counts)
    du2, dg2 = torch.autograd.grad((y2 * dy).sum(), (u, grid))
    du3, dg3 = R.reduced_bwd(u.detach(), grid.detach(), W, dy, counts)
    assert float((y - y2).detach().abs().max()) < 1e-11
    for a, b in ((du, du2), (du, du3), (dg, dg2), (dg, dg3)):
        assert float((a - b).abs().max()) < 1e-11
    # the attention is neither uniform nor the identity here, and P's rows are distributions
    L = U if counts is None else sum(counts)
    assert A.shape[-1] == L + 2 and float((P.sum(-1) - 1).abs().max()) < 1e-13
    assert 1.5 / (L + 2) < float(A.max(-1).values.mean()) < 0.9
    # a duplicate's row of A is a copy of its original's, and P's column carries the multiplicity
    if counts is not None:
        assert torch.equal(A[:, 2], A[:, 3]) and torch.equal(A[:, 2], A[:, 4])
        assert float((P[:, :, 2] - A[:, [0, 1, 2, 5, 6, 7, 9, 10, 11], 2:5].sum(-1)).abs().max()) < 1e-13


@pytest.mark.parametrize("name", list(C.CASES))
def test_op_test_inputs_do_not_hide_the_attention(name):
    C.assert_not_hidden(C.make_case(name))


def test_golden_model_restatement():
    """trans_attn_ref.niofp2d_trans_attn against the reference's own fp32 run (61^2, one bag, 51
    recorded draws with replacement from 52 snapshots): output, every stored gradient, and both
    anti-hiding conditions on the float64 restatement."""
    g, st, x = golden_case()
    idx = g["idx"].tolist()
    assert tuple(g["x_shape"]) == (1, 52, 61, 61) and len(idx) == int(g["L"]) == 51
    assert len(set(idx)) < len(idx)                       # the draw holds a duplicate
    assert os.path.getsize(os.path.join(GOLDEN, "nio2d_trans_attn_train.npz")) <= \
        os.path.getsize(os.path.join(GOLDEN, "nio2d_fno_attn_train.npz"))
    p = {k: torch.from_numpy(v).double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    grid = torch.from_numpy(g["in.grid"]).double()
    y = R.niofp2d_trans_attn(p, torch.from_numpy(x), grid, idx=idx)
    e = rel_l2(y.detach().numpy(), g["out"])
    print(f"output rel-L2 {e:.2e}")
    assert e <= OUT_TOL
    (y * torch.from_numpy(g["cot"]).double()).sum().backward()
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            assert p[k[2:]].grad is not None, k
            assert rel_l2(p[k[2:]].grad.numpy(), v) <= G_TOL, k
            n += 1
    assert n == 96 and sum(k.startswith("g.trans_input.") for k in g) == 68
    assert not any(k.startswith(("g.branch.", "g.fc0.")) or k == "g.trans_input.placeholder" for k in g)
    for k, q in p.items():                                # and nothing else has a gradient
        if k.startswith(("branch.", "fc0.")) or k == "trans_input.placeholder":
            assert q.grad is None, k
    with torch.no_grad():
        for mode in ("identity", "uniform"):
            ym = R.niofp2d_trans_attn(p, torch.from_numpy(x), grid, idx=idx, attn=mode)
            move = rel_l2(ym.numpy(), y.detach().numpy())
            print(f"{mode} attention moves the output by {move:.2e}")
            assert move >= 10 * OUT_TOL, mode
            assert float(g[mode + "_move_out"]) >= 10 * OUT_TOL


def test_state_dict_layout_matches_reference():
    import blindno
    lay = json.load(open(os.path.join(GOLDEN, "layouts_trans_attn.json")))
    trans = json.load(open(os.path.join(GOLDEN, "layouts_trans.json")))
    for key, kernel in (("2d_FPE", (2, 1)), ("2d_NC", (3, 2))):
        m = blindno.NIOFP2D_Trans_attn(*CTOR, branch_last_kernel=kernel)
        got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
        want = lay[f"{key}.NIOFP2D_Trans_attn(2,3,100,25,3,12,32,2,61,61)"]
        assert got == want
        # fc0 keeps its slot between branch and trans_input; the layout is NIOFP2D_Trans'
        assert want == trans[f"{key}.NIOFP2D_Trans(2,3,100,25,3,12,32,2)"]
        names = [k for k, _, _ in want]
        assert names.index("fc0.weight") < names.index("trans_input.placeholder")
        assert m.unused_prefixes == blindno.NIOFP2D_Trans.unused_prefixes
        assert (m.nx, m.ny) == (61, 61)


def test_seeded_construction_draws_fc0_last():
    """The reference assigns fc0 twice; the surviving Linear(3, width) is drawn after the heads."""
    import blindno
    torch.manual_seed(7)
    m = blindno.NIOFP2D_Trans_attn(2, 2, 8, 3, 1, 4, 2, 2, 61, 61)
    fc0_after = torch.nn.Linear(3, 4)                     # the RNG's next Linear
    torch.manual_seed(7)
    t = blindno.NIOFP2D_Trans(2, 2, 8, 3, 1, 4, 2, 2)
    fc0_last = torch.nn.Linear(3, 4)                      # what the second assignment draws
    # everything drawn before the second fc0 is NIOFP2D_Trans' construction
    for (k, a), (k2, b) in zip(m.state_dict().items(), t.state_dict().items()):
        assert k == k2
        if not k.startswith("fc0."):
            assert torch.equal(a, b), k
    assert torch.equal(m.fc0.weight, fc0_last.weight) and torch.equal(m.fc0.bias, fc0_last.bias)
    assert not torch.equal(m.fc0.weight, t.fc0.weight)
    assert not torch.equal(fc0_after.weight, fc0_last.weight)   # and the RNG moved on past it


def test_grid_other_than_61_and_device_bags_are_refused(monkeypatch):
    import blindno
    from blindno import ops
    monkeypatch.setattr(ops, "require_device", lambda *a: None)
    m = blindno.NIOFP2D_Trans_attn(2, 2, 8, 3, 1, 2, 2, 2, 24, 24)
    with pytest.raises(ValueError, match="61 x 61"):
        m(torch.zeros(1, 60, 24, 24), torch.zeros(24, 24, 2))
    with pytest.raises(ValueError, match="host index list"):
        m(torch.zeros(1, 60, 61, 61), torch.zeros(61, 61, 2),
          bag_idx=(torch.zeros(3, dtype=torch.int32), torch.ones(3) / 3))


def test_bagattn_mix_queries_and_refusals_without_a_device():
    import blindno
    from blindno import _lib
    lib = blindno.load_library()
    q = _lib.query
    assert q("blindno_bagattn_mix_ok", 4, 53, 3721, 12) == 1
    assert q("blindno_bagattn_mix_ok", 1, 254, 1, 1) == 1 and q("blindno_bagattn_mix_ok", 1, 255, 1, 1) == 0
    assert q("blindno_bagattn_mix_ok", 0, 3, 9, 1) == 0 and q("blindno_bagattn_mix_ok", 1, 3, 0, 1) == 0
    assert q("blindno_bagattn_mix_nchunk", 3721) == 8 == q("blindno_bagattn_nchunk", 3721)
    assert q("blindno_bagattn_mix_bwd_nchunk", 3721) == 30 and q("blindno_bagattn_mix_nchunk", 1) == 1
    assert q("blindno_bagattn_mix_fwd_scratch_floats", 4, 53, 3721) == 4 * 8 * 55 * 55
    assert q("blindno_bagattn_mix_bwd_scratch_floats", 4, 53, 3721) == \
        4 * 3 * 3721 + 4 * 30 * 3 * 55 + 4 * 55 * 55
    assert q("blindno_bagattn_mix_fwd_scratch_floats", 0, 53, 3721) == -1
    assert q("blindno_bagattn_mix_bwd_scratch_floats", 1, 255, 10) == -1
    # the entry points refuse bad arguments with a code and launch nothing (NULL pointers, V = 257)
    assert lib.blindno_bagattn_mix_fwd(None, None, None, None, None, None, None, None, None,
                                       1, 3, 9, 2, 3, None) != 0
    assert lib.blindno_bagattn_mix_bwd(None, None, None, None, None, None, None, None, None, None,
                                       1, 255, 9, 2, 255, None) != 0


def test_trainer_lists_the_experiment():
    from blindno import trainer
    exps = trainer.experiments_for("trans_attn")
    e, t = exps["2d_FPE"], trainer.experiments_for("trans")["2d_FPE"]
    assert e.eager and (e.lr, e.batch, e.save_interval) == (t.lr, t.batch, t.save_interval)
    assert e.result_dir == "results_2d_FPE_trans_attn"
    assert sorted(trainer._own_experiments("trans_attn")) == ["2d_FPE"]
    # _experiments keeps its tables: an unknown model name falls through to the NIO-FNO table
    assert trainer._experiments("trans_attn")["2d_FPE"].result_dir == "result_2d_fno"
    assert sorted(trainer._own_experiments("trans")) == ["2d_FPE"] and trainer._own_experiments("fno") == {}
    m = e.model(61, "cpu")
    assert type(m).__name__ == "NIOFP2D_Trans_attn" and (m.nx, m.ny) == (61, 61)
