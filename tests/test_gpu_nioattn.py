"""The coefficient-space bag attention of NIOFP2D_attn called directly through the C ABI
(csrc/nioattn.hip, include/blindno_nioattn.h: blindno_nioattn_moments / _fwd / _bwd) against the
float64 restatements of tests/nio2d_attn_ref.py, and the model on its golden.

Two references.  attn_math restates the header's formulas term by term (M, A, cs, v, y, dw, dbasis,
db0); attn_direct materialises the tokens and differentiates oracle.fno_ref.bag_attention in float64
(y, dw, dbasis, db0), sharing neither the low-rank rewriting nor the hand-derived backward; the two
agree to 1e-11 (tests/test_nio2d_attn.py).  Every shape runs in three logit regimes set by the
amplitude of w and asserted on the float64 reference before the device is touched
(tests/nioattn_cases.py): diffuse (max |logit| <= 1), mixed (mean row maximum of A in [0.2, 0.8] and
a softmax-path share of dw of at least 2 %) and sharp (max logit >= 150, beyond fp32 exp's overflow
at 88.7).  No pair is skipped.

Tolerances.  Each compared array is held to rel-L2 <= max(2e-6, 3 x envelope), the rule of
tests/test_gpu_bagagg.py: 2e-6 is what a single fp32 kernel is held to against float64, and the
envelope is measured on the reference, never on the kernels: the largest rel-L2 distance from the
float64 result among fp32 host evaluations of attn_math on the same inputs, unperturbed and under
three fp32-rounding-sized input perturbations (x (1 + 2^-24 N(0, 1))).

Every output and scratch buffer is a NaN-prefilled view with 256 sentinel floats on both sides: the
margins must come back untouched and the view without a NaN.  Each check prints its worst error /
bar.  (The guarded buffers, the envelope and the check are those of tests/test_gpu_bagagg.py.)
"""
import functools
import json
import math

import numpy as np
import pytest
import torch

import nio2d_attn_ref
from conftest import load_golden, rel_l2
from nioattn_cases import REGIMES, SHAPES, make_case

pytestmark = pytest.mark.gpu

SENT = -12345.678        # the sentinel (random data never takes this value)
MARGIN = 256             # sentinel floats on both sides of every output / scratch buffer
FLOOR = 2e-6             # one fp32 kernel against float64 (tests/test_gpu_bagproj.py)
MATH_NAMES = ("M", "A", "cs", "v", "y", "dw", "dbasis", "db0")
DIRECT_NAMES = ("y", "dw", "dbasis", "db0")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _api():
    from blindno._lib import call, ptr, query, stream_ptr
    return call, ptr, query, stream_ptr


def _rel(a, b):
    a, b = a.double(), b.double()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-300))


class Guarded:
    """A NaN-prefilled view of the given shape between two sentinel margins."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * MARGIN,), SENT, device="cuda")
        self.t = self.buf[MARGIN:MARGIN + self.n].view(*shape)
        self.t.fill_(float("nan"))

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == SENT).all() and (self.buf[MARGIN + self.n:] == SENT).all())

    def no_nan(self):
        return not bool(torch.isnan(self.t).any())

    def untouched(self):
        return self.margins_intact() and bool(torch.isnan(self.t).all())


def _jitter(t, gen):
    """One fp32 rounding's worth of input perturbation."""
    return (t.double() * (1 + 2.0 ** -24 * torch.randn(t.shape, generator=gen, dtype=torch.float64))).float()


def _envelope(math_fn, inputs, ref, names):
    """Largest rel-L2 distance from the float64 result among fp32 evaluations of ``math_fn``:
    the inputs as they are, and three times under an fp32-rounding-sized perturbation."""
    env = dict.fromkeys(names, 0.0)
    for seed in (None, 1, 2, 3):
        ins = inputs
        if seed is not None:
            gen = torch.Generator().manual_seed(seed)
            ins = [None if t is None else _jitter(t, gen) for t in inputs]
        got = math_fn(*ins, torch.float32)
        for k in names:
            env[k] = max(env[k], _rel(got[k], ref[k]))
    return env


def _check(tag, got, ref, env, names, ref_name="fp64"):
    worst = {}
    for k in names:
        bar = max(FLOOR, 3.0 * env[k])
        worst[k] = (_rel(got[k].cpu(), ref[k]), bar)
    print(f"{tag} vs {ref_name}: "
          + ", ".join(f"{k} {e:.2e}/{b:.2e} ({e / b:.2f})" for k, (e, b) in worst.items()))
    for k, (e, b) in worst.items():
        assert e <= b, (tag, ref_name, k, e, b, env[k])


@functools.lru_cache(maxsize=None)
def _case(B, L, S, P, width, regime):
    """Inputs, float64 attn_math, float64 autograd of the materialised composition and the fp32
    envelope of one case (the regime is asserted in make_case, on the float64 reference)."""
    inputs, ref = make_case(B, L, S, P, width, regime)
    direct = nio2d_attn_ref.attn_direct(*inputs)
    for k in DIRECT_NAMES:      # two float64 statements of the same function
        assert _rel(ref[k], direct[k]) <= 1e-11, (k, _rel(ref[k], direct[k]))
    env = _envelope(nio2d_attn_ref.attn_math, inputs, ref, MATH_NAMES)
    return inputs, ref, direct, env


class _Run:
    """blindno_nioattn_moments, _fwd and _bwd once each on guarded buffers."""

    def __init__(self, dev_inputs):
        call, ptr, query, sp = _api()
        w, basis, b0, grid, fw, fb, dy = dev_inputs
        B, L, P = w.shape
        S, width = basis.shape[0], fw.numel()
        T, Q = L + 2, P + 3
        nbm, nbb = query("blindno_nioattn_moments_nblk", S), query("blindno_nioattn_bwd_nblk", S)
        assert nbm == (S + 127) // 128 and nbb == (S + 127) // 128
        nm = query("blindno_nioattn_moments_scratch_floats", S, P)
        ns = query("blindno_nioattn_bwd_scratch_floats", B, S, P)
        assert nm == nbm * Q * Q and ns == B * S + nbb * B * Q + B * Q * Q + Q * Q + B
        self.g = {"partial": Guarded(nm), "M": Guarded(Q, Q), "A": Guarded(B, T, T), "cs": Guarded(B, T),
                  "v": Guarded(B, Q), "y": Guarded(B, S, width), "scratch": Guarded(ns),
                  "dw": Guarded(B, L, P), "dbasis": Guarded(S, P), "db0": Guarded(1)}
        g = self.g
        b0 = b0.reshape(1)
        call("blindno_nioattn_moments", ptr(grid), ptr(basis), ptr(g["partial"].t), ptr(g["M"].t), nbm, S, P,
             sp())
        call("blindno_nioattn_fwd", ptr(w), ptr(b0), ptr(basis), ptr(grid), ptr(g["M"].t), ptr(fw), ptr(fb),
             ptr(g["A"].t), ptr(g["cs"].t), ptr(g["v"].t), ptr(g["y"].t), B, L, S, P, width, sp())
        call("blindno_nioattn_bwd", ptr(dy), ptr(w), ptr(b0), ptr(basis), ptr(grid), ptr(g["M"].t), ptr(fw),
             ptr(g["A"].t), ptr(g["cs"].t), ptr(g["v"].t), ptr(g["scratch"].t), ptr(g["dw"].t),
             ptr(g["dbasis"].t), ptr(g["db0"].t), nbb, B, L, S, P, width, sp())
        torch.cuda.synchronize()

    def __getitem__(self, k):
        return self.g[k].t


@functools.lru_cache(maxsize=None)
def _runs(B, L, S, P, width, regime):
    """The device results of one case, shared by the tests below: two runs."""
    inputs = _case(B, L, S, P, width, regime)[0]
    dev = tuple(t.cuda() for t in inputs)
    return _Run(dev), _Run(dev)


def _params(f):
    f = pytest.mark.parametrize("B,L,S,P,width", SHAPES)(f)
    return pytest.mark.parametrize("regime", REGIMES)(f)


@_params
def test_nioattn_matches_fp64(B, L, S, P, width, regime):
    _, ref, direct, env = _case(B, L, S, P, width, regime)
    run = _runs(B, L, S, P, width, regime)[0]
    tag = f"nioattn B={B} L={L} S={S} P={P} width={width} {regime}"
    for k in run.g:
        assert torch.isfinite(run[k]).all(), k
    assert torch.equal(run["M"], run["M"].t())            # the moments are symmetric bit for bit
    _check(tag, run, ref, env, MATH_NAMES)
    _check(tag, run, direct, env, DIRECT_NAMES, "materialised autograd")


@_params
def test_nioattn_is_deterministic(B, L, S, P, width, regime):
    first, second = _runs(B, L, S, P, width, regime)
    for k in first.g:
        assert torch.equal(first[k], second[k]), k


@_params
def test_nioattn_writes_all_of_its_buffers_and_nothing_else(B, L, S, P, width, regime):
    for run in _runs(B, L, S, P, width, regime):
        for k, gb in run.g.items():
            assert gb.margins_intact(), k
            assert gb.no_nan(), k


@pytest.mark.parametrize("regime", REGIMES)
def test_a_bag_does_not_depend_on_the_rest_of_the_batch(regime):
    """Bag 0's A, cs, v at B = 1 are bit-identical to the same bag inside B = 3."""
    B, L, S, P, width = 3, 5, 63, 25, 5
    inputs = _case(B, L, S, P, width, regime)[0]
    full = _runs(B, L, S, P, width, regime)[0]
    w, basis, b0, grid, fw, fb, dy = (t.cuda() for t in inputs)
    one = _Run((w[:1].contiguous(), basis, b0, grid, fw, fb, dy[:1].contiguous()))
    assert torch.equal(one["M"], full["M"])
    for k in ("A", "cs", "v", "y"):
        assert torch.equal(one[k][0], full[k][0]), k


def test_nioattn_entry_points_refuse_invalid_arguments():
    """hipErrorInvalidValue with the guarded outputs untouched for B <= 0, L < 1, T > 256, P < 1,
    P > 64, S < 1, width < 1 and a NULL required pointer."""
    from blindno import BlindnoError
    call, ptr, query, sp = _api()
    B, L, S, P, width = 1, 2, 64, 3, 2
    z = torch.zeros(300 * 70, device="cuda")
    outs = [Guarded(300 * 300) for _ in range(5)]
    o = [ptr(g.t) for g in outs]

    def moments(S_, P_, grid=ptr(z), basis=ptr(z), partial=o[0], M=o[1], nblk=None):
        nb = max(1, query("blindno_nioattn_moments_nblk", S_)) if nblk is None else nblk
        call("blindno_nioattn_moments", grid, basis, partial, M, nb, S_, P_, sp())

    def fwd(B_, L_, S_, P_, width_, **kw):
        a = dict(w=ptr(z), b0=ptr(z), basis=ptr(z), grid=ptr(z), M=ptr(z), fw=ptr(z), fb=ptr(z), A=o[0],
                 cs=o[1], v=o[2], y=o[3])
        a.update(kw)
        call("blindno_nioattn_fwd", a["w"], a["b0"], a["basis"], a["grid"], a["M"], a["fw"], a["fb"], a["A"],
             a["cs"], a["v"], a["y"], B_, L_, S_, P_, width_, sp())

    def bwd(B_, L_, S_, P_, width_, nblk=None, **kw):
        a = dict(dy=ptr(z), w=ptr(z), b0=ptr(z), basis=ptr(z), grid=ptr(z), M=ptr(z), fw=ptr(z), A=ptr(z),
                 cs=ptr(z), v=ptr(z), scratch=o[0], dw=o[1], dbasis=o[2], db0=o[3])
        a.update(kw)
        nb = max(1, query("blindno_nioattn_bwd_nblk", S_)) if nblk is None else nblk
        call("blindno_nioattn_bwd", a["dy"], a["w"], a["b0"], a["basis"], a["grid"], a["M"], a["fw"], a["A"],
             a["cs"], a["v"], a["scratch"], a["dw"], a["dbasis"], a["db0"], nb, B_, L_, S_, P_, width_, sp())

    bad = [lambda: moments(0, P), lambda: moments(S, 0), lambda: moments(S, 65), lambda: moments(S, P, nblk=2)]
    bad += [lambda k=k: moments(S, P, **{k: None}) for k in ("grid", "basis", "partial", "M")]
    for f in (fwd, bwd):
        bad += [lambda f=f: f(0, L, S, P, width), lambda f=f: f(-1, L, S, P, width),
                lambda f=f: f(B, 0, S, P, width), lambda f=f: f(B, 255, S, P, width),
                lambda f=f: f(B, L, S, 0, width), lambda f=f: f(B, L, S, 65, width),
                lambda f=f: f(B, L, 0, P, width), lambda f=f: f(B, L, S, P, 0)]
    bad += [lambda k=k: fwd(B, L, S, P, width, **{k: None})
            for k in ("w", "b0", "basis", "grid", "M", "fw", "fb", "A", "cs", "v", "y")]
    bad += [lambda k=k: bwd(B, L, S, P, width, **{k: None})
            for k in ("dy", "w", "b0", "basis", "grid", "M", "fw", "A", "cs", "v", "scratch", "dw", "dbasis",
                      "db0")]
    bad.append(lambda: bwd(B, L, S, P, width, nblk=2))
    assert len(bad) == 50
    for f in bad:
        with pytest.raises(BlindnoError):
            f()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
    # the same sizes are accepted once they are valid (the refusals above are about the arguments)
    moments(S, P)
    fwd(B, L, S, P, width)
    torch.cuda.synchronize()
    assert all(g.margins_intact() for g in outs)


def test_nio_attn_fn_wrapper():
    """ops.NIOAttnFn: non-contiguous w and basis (the _c path), gradients against the materialised
    float64 autograd, and the grid that asks for a gradient."""
    from blindno import BlindnoError, ops
    B, L, S, P, width = 3, 5, 63, 25, 5
    (w, basis, b0, grid, fw, fb, dy), ref, direct, env = _case(B, L, S, P, width, "mixed")
    w_nc = w.cuda().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    basis_nc = basis.cuda().t().contiguous().t().requires_grad_(True)
    assert not w_nc.is_contiguous() and not basis_nc.is_contiguous()
    b0d = b0.cuda().requires_grad_(True)
    y = ops.NIOAttnFn.apply(w_nc, basis_nc, b0d, grid.cuda(), fw.cuda().view(width, 1), fb.cuda())
    y.backward(dy.cuda())
    got = {"y": y.detach(), "dw": w_nc.grad, "dbasis": basis_nc.grad, "db0": b0d.grad.reshape(1)}
    assert tuple(b0d.grad.shape) == ()
    _check("NIOAttnFn", got, direct, env, DIRECT_NAMES, "materialised autograd")
    with pytest.raises(BlindnoError):
        ops.NIOAttnFn.apply(w_nc, basis_nc, b0d, grid.cuda().requires_grad_(True), fw.cuda().view(width, 1),
                            fb.cuda())
    # b0 of shape (1,): its gradient comes back in that shape, the same bits
    b1 = b0.cuda().reshape(1).requires_grad_(True)
    w2, basis2 = w_nc.detach().requires_grad_(True), basis_nc.detach().requires_grad_(True)
    y2 = ops.NIOAttnFn.apply(w2, basis2, b1, grid.cuda(), fw.cuda().view(width, 1), fb.cuda())
    y2.backward(dy.cuda())
    assert tuple(b1.grad.shape) == (1,) and torch.equal(b1.grad.reshape(()), b0d.grad)
    assert torch.equal(y2, y) and torch.equal(w2.grad, w_nc.grad) and torch.equal(basis2.grad, basis_nc.grad)
    # only w asks for a gradient
    w3 = w_nc.detach().requires_grad_(True)
    ops.NIOAttnFn.apply(w3, basis_nc.detach(), b0.cuda(), grid.cuda(), fw.cuda().view(width, 1),
                        fb.cuda()).backward(dy.cuda())
    assert torch.equal(w3.grad, w_nc.grad)


# ------------------------------------------------------------------------------------ the model
def _golden_model():
    from blindno import NIOFP2D_attn
    from recipe import make_array, make_state
    g = load_golden("nio2d_attn_train")
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g["layout_json"]))]
    st = make_state(shapes, seed=int(g["recipe_seed"]))
    m = NIOFP2D_attn(2, 3, 100, 25, 2, 6, 8, 2, heads=("fno_Fx", "fno_Fy"), branch_last_kernel=(3, 2))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    x = float(g["amp"]) * make_array(tuple(int(n) for n in g["x_shape"]), int(g["recipe_seed"]), "nio2d_attn.x")
    return g, st, m.cuda().train(), torch.from_numpy(x).cuda(), torch.from_numpy(g["in.grid"]).cuda()


def test_niofp2d_attn_on_its_golden():
    """NIOFP2D_attn at 80^2 with recipe parameters and the recorded draw (with replacement) against
    the float64 restatement (nio2d_attn_ref.niofp2d_attn, itself pinned to the reference's golden on
    the CPU), by the NIO rule of tests/test_gpu_evaluators.py: the HIP output and gradients must be
    as close to float64 as the reference's own fp32 golden is, within 2x, or within forward 1e-5 /
    gradients 1e-4.  Then one torch.optim.Adam step: trunk and branch move, fc0 does not."""
    g, st, m, x, grid = _golden_model()
    idx = g["idx"]
    assert len(set(idx.tolist())) < len(idx)
    out = m(x, grid, bag_idx=idx)
    cot = torch.from_numpy(g["cot"]).cuda()
    (out * cot).sum().backward()
    p64 = {k: torch.from_numpy(v).cuda().double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    ref = nio2d_attn_ref.niofp2d_attn(p64, x.double(), grid.double(), idx=idx.tolist(), heads=("fno_Fx", "fno_Fy"))
    (ref * cot.double()).sum().backward()
    e = rel_l2(out.detach().cpu().numpy(), ref.detach().cpu().numpy())
    e_ref = rel_l2(g["out"], ref.detach().cpu().numpy())
    print(f"NIOFP2D_attn out: HIP {e:.2e}, reference fp32 {e_ref:.2e}")
    assert e <= max(1e-5, 2 * e_ref), (e, e_ref)
    named = dict(m.named_parameters())
    rows = []                                   # (name, gpu error, reference fp32 error)
    gmax = max(float(p64[k[6:]].grad.norm()) for k in g if k.startswith("gnorm."))
    for k, v in g.items():
        if k.startswith("g."):
            ref_g = p64[k[2:]].grad.cpu().numpy()
            rows.append((k, rel_l2(named[k[2:]].grad.cpu().numpy(), ref_g), rel_l2(v, ref_g)))
        elif k.startswith("gnorm."):
            want = float(p64[k[6:]].grad.norm())
            got = float(named[k[6:]].grad.double().norm())
            assert abs(got - want) <= max(2 * abs(float(v) - want), 1e-4 * want) + 1e-5 * gmax, k
    med = float(np.median([r[2] for r in rows]))
    print("NIOFP2D_attn grads: worst HIP %.2e, worst reference fp32 %.2e, median reference %.2e"
          % (max(r[1] for r in rows), max(r[2] for r in rows), med))
    for k, eg, er in rows:
        assert eg <= max(1e-4, 2 * er, 2 * med), (k, eg, er, med)
    assert len(rows) > 30
    assert m.fc0.weight.grad is None and m.fc0.bias.grad is None

    before = {k: v.detach().clone() for k, v in named.items()}
    torch.optim.Adam(m.parameters(), lr=1e-3).step()
    assert torch.equal(m.fc0.weight, before["fc0.weight"]) and torch.equal(m.fc0.bias, before["fc0.bias"])
    for k in ("trunk.input_layer.weight", "trunk.output_layer.weight", "branch.convblock1.layers.0.weight",
              "branch.linear.weight", "deeponet.b0"):
        assert not torch.equal(named[k], before[k]), k


def test_train_mode_bag_idx_equals_eval_on_the_gathered_bag():
    """forward(x, grid, bag_idx=idx) in train mode against an eval-mode call (all T snapshots) on
    x[:, idx].  The model's own mode decides only how the bag is chosen; the BatchNorm layers of the
    branch and the trunk are kept on batch statistics in both calls, so the two calls run the same
    kernels on the same values: fp32 rounding (1e-6) is all that may separate them."""
    g, st, m, x, grid = _golden_model()
    idx = g["idx"]
    with torch.no_grad():
        a = m(x, grid, bag_idx=idx)
        m.eval()
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.train()
        assert not m.training
        b = m(x[:, torch.as_tensor(idx, device="cuda")].contiguous(), grid)
    e = rel_l2(a.cpu().numpy(), b.cpu().numpy())
    print(f"train(bag_idx) vs eval(gathered): {e:.2e}")
    assert e <= 1e-6, e
