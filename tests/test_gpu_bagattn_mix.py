"""ops.BagAttnMixFn (csrc/bagattn_mix.hip, include/blindno_bagattn_mix.h) against the literal
float64 form of tests/trans_attn_ref.py: the reference's own matmul / softmax / matmul / fusion
sequence on the L + 2 materialised tokens (needs a GPU).

Tolerances as SURVEY.md 8c (tests/test_gpu_parity.py): forward rel-L2 <= 1e-5, gradients <= 1e-4.
The inputs (tests/bagattn_mix_cases.py) are structured so that the attention is neither
near-uniform nor near-identity; that is asserted on the float64 reference alone.
"""
import numpy as np
import pytest
import torch

import bagattn_mix_cases as C
import trans_attn_ref as R
from conftest import rel_l2
from test_gpu_parity import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


_REF = {}


def reference(name):
    """(case, y, du, dgrid) of the literal float64 form, computed once per case."""
    if name not in _REF:
        c = C.make_case(name)
        C.assert_not_hidden(c)
        u = c["u"].clone().requires_grad_(True)
        g = c["grid"].clone().requires_grad_(True)
        y, _ = R.literal(u, g, c["W"], c["bias"], c["counts"])
        du, dg = torch.autograd.grad((y * c["dy"]).sum(), (u, g))
        _REF[name] = (c, y.detach().numpy(), du.numpy(), dg.numpy())
    return _REF[name]


def lw_of(counts, dev="cuda"):
    """(lw, L) as blindno.nio.dedup_bag forms them: multiplicity / L in float32."""
    if counts is None:
        return None, None
    L = int(sum(counts))
    return torch.as_tensor((np.asarray(counts) / float(L)).astype(np.float32), device=dev), L


def run(c, counts="case", need_grid=True):
    """The op on the GPU: (y, du, dgrid) as numpy."""
    from blindno import ops
    counts = c["counts"] if counts == "case" else counts
    u = c["u"].float().cuda().requires_grad_(True)
    g = c["grid"].float().cuda().requires_grad_(need_grid)
    lw, L = lw_of(counts)
    y = ops.BagAttnMixFn.apply(u, g, c["W"].float().cuda(), c["bias"].float().cuda(), lw, L)
    (y * c["dy"].float().cuda()).sum().backward()
    torch.cuda.synchronize()
    return (y.detach().cpu().numpy(), u.grad.cpu().numpy(),
            g.grad.cpu().numpy() if need_grid else None)


@pytest.mark.parametrize("name", list(C.CASES))
def test_op_against_literal_float64(name):
    c, y_ref, du_ref, dg_ref = reference(name)
    y, du, dg = run(c)
    e = (rel_l2(y, y_ref), rel_l2(du, du_ref), rel_l2(dg, dg_ref))
    print(f"{name}: y {e[0]:.2e}, du {e[1]:.2e}, dgrid {e[2]:.2e}")
    assert e[0] <= FWD_TOL, e
    assert e[1] <= GRAD_TOL, e
    assert e[2] <= GRAD_TOL, e


def test_du_without_grid_gradient():
    """The grid tokens' rows are skipped when the grid asks for no gradient; du is unchanged."""
    c, _, _, _ = reference("small_S")
    _, du, _ = run(c)
    _, du2, none = run(c, need_grid=False)
    assert none is None and np.array_equal(du, du2)


@pytest.mark.parametrize("name", ["workload", "small_S"])
def test_no_counts_is_all_ones_bitwise(name):
    c, _, _, _ = reference(name)
    U = c["u"].shape[1]
    a = run(c, counts=None)
    b = run(c, counts=[1] * U)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("name", ["workload", "one_snapshot", "small_S"])
def test_counts_agree_with_expanded_bag(name):
    """Distinct tokens with counts against the same op on the index_select-expanded bag."""
    c, _, _, _ = reference(name)
    U = c["u"].shape[1]
    sel = R.expand_index(c["counts"], U)
    e = dict(c, u=c["u"].index_select(1, sel), counts=None)
    y, du, dg = run(c)
    ye, due, dge = run(e)
    due_sum = np.zeros_like(du)
    np.add.at(due_sum, (slice(None), sel.numpy()), due)
    assert rel_l2(y, ye) <= FWD_TOL
    assert rel_l2(du, due_sum) <= GRAD_TOL
    assert rel_l2(dg, dge) <= GRAD_TOL


def test_against_bagattn_fn():
    """With W = [w/T, w/T, w L/T] and no counts this op and ops.BagAttnFn are one function."""
    from blindno import ops
    c, _, _, _ = reference("workload")
    B, L, S = c["u"].shape
    T = L + 2
    w = c["W"][:, 2:3].float()
    W3 = torch.cat([w / T, w / T, w * L / T], dim=1)
    bias, dy = c["bias"].float().cuda(), c["dy"].float().cuda()
    outs = []
    for fn, wt in ((ops.BagAttnFn, w), (ops.BagAttnMixFn, W3)):
        u = c["u"].float().cuda().requires_grad_(True)
        g = c["grid"].float().cuda().requires_grad_(True)
        y = fn.apply(u, g, wt.cuda(), bias)
        (y * dy).sum().backward()
        outs.append([t.detach().cpu().numpy() for t in (y, u.grad, g.grad)])
    assert rel_l2(outs[1][0], outs[0][0]) <= FWD_TOL
    assert rel_l2(outs[1][1], outs[0][1]) <= GRAD_TOL
    assert rel_l2(outs[1][2], outs[0][2]) <= GRAD_TOL


@pytest.mark.parametrize("name", ["workload", "cap"])
def test_two_runs_are_bit_identical(name):
    c, _, _, _ = reference(name)
    a, b = run(c), run(c)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_errors():
    from blindno import BlindnoError, ops
    dev = "cuda"
    g, W, b = torch.zeros(10, 2, device=dev), torch.zeros(4, 3, device=dev), torch.zeros(4, device=dev)
    with pytest.raises(BlindnoError, match="256 tokens"):
        ops.BagAttnMixFn.apply(torch.zeros(1, 255, 10, device=dev), g, W, b)
    u = torch.zeros(1, 3, 10, device=dev)
    with pytest.raises(BlindnoError, match="number of draws"):
        ops.BagAttnMixFn.apply(u, g, W, b, torch.full((3,), 1 / 3, device=dev))
    with pytest.raises(BlindnoError):
        ops.BagAttnMixFn.apply(u, g, W, b, torch.full((2,), 0.5, device=dev), 4)
    with pytest.raises(BlindnoError):
        ops.BagAttnMixFn.apply(u, torch.zeros(9, 2, device=dev), W, b)
    with pytest.raises(BlindnoError):
        ops.BagAttnMixFn.apply(u, g, torch.zeros(4, 1, device=dev), b)
    with pytest.raises(BlindnoError, match="device"):
        ops.BagAttnMixFn.apply(u.cpu(), g.cpu(), W.cpu(), b.cpu())
