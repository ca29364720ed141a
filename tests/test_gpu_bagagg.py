"""The two snapshot-bag aggregations called directly through the C ABI: the token self-attention
over the bag (csrc/attn.hip, blindno_bagattn_fwd / _bwd: six kernels) and the fixed-weight bag
mean (csrc/fields.hip, blindno_bagmean_fwd_w / _bwd), each against a float64 restatement on the
host, with their autograd wrappers (ops.BagAttnFn, ops.BagMeanFn) checked where the wrapper itself
is the subject.

Bag attention.  The reference restates attn.hip's header comment literally (G = X X^T,
A = softmax(G / sqrt S), c = colsum A, y; dm, dc, dS, M = (dS + dS^T) / sqrt S, dX); y, du and the
grid gradient have a second reference that does not share the hand-derived backward: float64
autograd of oracle.fno_ref.bag_attention (pinned to the reference by the goldens).  Every shape
runs in three logit regimes set by the input amplitude and asserted on the float64 reference before
the device is touched: diffuse (max |logit| <= 1), mixed (mean row maximum of A in [0.2, 0.8] and
the softmax-path term sum_t M[s,t] X[t,p] at least 2 % of ||du||) and sharp (max logit >= 150,
beyond fp32 exp's overflow at 88.7: inf / NaN without the row-maximum subtraction).

Tolerances.  Each compared array is held to rel-L2 <= max(2e-6, 3 x envelope).  2e-6 is what a
single fp32 kernel is held to against float64 in test_gpu_bagproj.py; the envelope is measured on
the reference, never on the kernels: the largest rel-L2 distance from the float64 result among fp32
host evaluations of the same restatement on the same inputs, unperturbed and under three
fp32-rounding-sized input perturbations (x (1 + 2^-24 N(0, 1))), the rule of test_gpu_unet.py.
No array needed an allowance beyond that.

Every output and scratch buffer is a NaN-prefilled view with 256 sentinel floats on both sides:
the margins must come back untouched and the view without a NaN.  Each check prints its worst
error / bar.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -12345.678        # the sentinel (random data never takes this value)
MARGIN = 256             # sentinel floats on both sides of every output / scratch buffer
FLOOR = 2e-6             # one fp32 kernel against float64 (tests/test_gpu_bagproj.py)


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


# ============================================================================ bag attention
def _attn_math(grid, u, w, bias, dy, dt):
    """attn.hip's header comment, term by term, in the precision ``dt``."""
    grid, u, w, bias, dy = (t.to(dt) for t in (grid, u, w, bias, dy))
    B, L, S = u.shape
    T = L + 2
    X = torch.cat((grid.t().unsqueeze(0).expand(B, 2, S), u), 1)          # (B, T, S)
    logits = X @ X.transpose(1, 2) / math.sqrt(S)
    A = torch.softmax(logits, -1)
    cs = A.sum(1)                                                         # c_s = sum_t A[t,s]
    y = ((cs.unsqueeze(1) @ X).squeeze(1) / T).unsqueeze(-1) * w + bias   # (B, S, width)
    dm = dy @ w                                                           # (B, S)
    dc = (X @ dm.unsqueeze(-1)).squeeze(-1) / T                           # (B, T)
    r = (A @ dc.unsqueeze(-1)).squeeze(-1)
    dS = A * (dc.unsqueeze(1) - r.unsqueeze(2))
    M = (dS + dS.transpose(1, 2)) / math.sqrt(S)
    soft = M @ X                                                          # the softmax path of dX
    dX = (cs / T).unsqueeze(2) * dm.unsqueeze(1) + soft
    return {"logits": logits, "A": A, "cs": cs, "y": y, "dm": dm, "M": M, "du": dX[:, 2:],
            "dgt": dX[:, :2], "soft_u": soft[:, 2:]}


def _attn_oracle(grid, u, w, bias, dy):
    """y, du and the per-sample grid gradient by float64 autograd of the oracle's forward."""
    import oracle.fno_ref as ref
    B, L, S = u.shape
    ud = u.double().view(B, L, S, 1).requires_grad_(True)
    gcf = grid.double().t().unsqueeze(0).expand(B, 2, S).reshape(B, 2, S, 1).clone().requires_grad_(True)
    y = ref.bag_attention(ud, gcf, w.double().view(-1, 1), bias.double()).view(B, S, -1)
    (y * dy.double()).sum().backward()
    return {"y": y.detach(), "du": ud.grad.view(B, L, S), "dgt": gcf.grad.view(B, 2, S)}


# B, L, S, width
ATTN_SHAPES = [
    (2, 1, 25, 1),       # T = 3, S below one 32-point sub-tile, width 1
    (3, 5, 63, 5),       # T = 7 (not a multiple of 4: clamped rows, guarded mirror writes), S < 64
    (2, 12, 1023, 3),    # two chunks, ragged 511-point tail, S no multiple of 32 or 64
    (2, 30, 513, 4),     # one-point tail chunk; T = 32 is one dx_kernel pass with dgt, 30 rows without
    (1, 87, 64, 2),      # T = 89: 276 triangle blocks, a second Gram round with 20 live threads
    (1, 254, 64, 2),     # T = 256 (the cap): 9 Gram rounds, largest LDS of Gram and dx_kernel
    (2, 53, 512, 20),    # S exactly one chunk, wide output
]
REGIMES = ("diffuse", "mixed", "sharp")
ATTN_NAMES = ("A", "cs", "y", "dm", "M", "du", "dgt")


def _amplitude(regime, L, S):
    """Token standard deviation a: the diagonal logits are ~ a^2 sqrt(S), the others ~ a^2 N(0, 1).
    diffuse: diagonal 0.4; sharp: diagonal 220; mixed: diagonal ~ log T, where the diagonal entry
    weighs about as much as the T - 1 others together."""
    T = L + 2
    diag = {"diffuse": 0.4, "mixed": math.log(T), "sharp": 220.0}[regime]
    return math.sqrt(diag / math.sqrt(S))


@functools.lru_cache(maxsize=None)
def _attn_case(B, L, S, width, regime):
    """Inputs (fp32, host), the float64 restatement, the oracle's autograd and the fp32 envelope of
    one case; the regime is asserted here, on the float64 reference."""
    gen = torch.Generator().manual_seed(1000 * S + 10 * L + REGIMES.index(regime))
    a = _amplitude(regime, L, S)
    grid = a * torch.randn(S, 2, generator=gen)      # any (S, 2) values will do for the kernels
    u = a * torch.randn(B, L, S, generator=gen)
    w = torch.randn(width, generator=gen)
    bias = torch.randn(width, generator=gen)
    dy = torch.randn(B, S, width, generator=gen)
    inputs = (grid, u, w, bias, dy)
    ref = _attn_math(*inputs, torch.float64)
    logits, rowmax = ref["logits"], float(ref["A"].max(-1).values.mean())
    share = float(torch.linalg.vector_norm(ref["soft_u"]) / torch.linalg.vector_norm(ref["du"]))
    print(f"attn B={B} L={L} S={S} width={width} {regime}: amplitude {a:.3f}, max |logit| "
          f"{float(logits.abs().max()):.3g}, mean row max of A {rowmax:.3f}, softmax share of du {share:.3%}")
    if regime == "diffuse":
        assert float(logits.abs().max()) <= 1.0
    elif regime == "mixed":
        assert 0.2 <= rowmax <= 0.8
        assert share >= 0.02
    else:
        assert float(logits.max()) >= 150.0
    orc = _attn_oracle(*inputs)
    for k in orc:       # two float64 statements of the same function
        assert _rel(ref[k], orc[k]) <= 1e-11, (k, _rel(ref[k], orc[k]))
    env = _envelope(_attn_math, inputs, ref, ATTN_NAMES)
    return inputs, ref, orc, env


class _AttnRun:
    """blindno_bagattn_fwd once and blindno_bagattn_bwd once on guarded buffers."""

    def __init__(self, dev_inputs, with_dgt=True):
        call, ptr, query, sp = _api()
        grid, u, w, bias, dy = dev_inputs
        B, L, S = u.shape
        T, width = L + 2, w.numel()
        nch = query("blindno_bagattn_nchunk", S)
        assert nch == (S + 511) // 512
        self.g = {"partial_fwd": Guarded(B, nch, T, T), "A": Guarded(B, T, T), "cs": Guarded(B, T),
                  "y": Guarded(B, S, width), "partial_bwd": Guarded(B, nch, T), "dm": Guarded(B, S),
                  "M": Guarded(B, T, T), "du": Guarded(B, L, S)}
        if with_dgt:
            self.g["dgt"] = Guarded(B, 2, S)
        g = self.g
        call("blindno_bagattn_fwd", ptr(grid), ptr(u), ptr(w), ptr(bias), ptr(g["partial_fwd"].t),
             ptr(g["A"].t), ptr(g["cs"].t), ptr(g["y"].t), B, L, S, width, sp())
        call("blindno_bagattn_bwd", ptr(grid), ptr(u), ptr(dy), ptr(w), ptr(g["A"].t), ptr(g["cs"].t),
             ptr(g["partial_bwd"].t), ptr(g["dm"].t), ptr(g["M"].t), ptr(g["du"].t),
             ptr(g["dgt"].t) if with_dgt else None, B, L, S, width, sp())
        torch.cuda.synchronize()

    def __getitem__(self, k):
        return self.g[k].t


@functools.lru_cache(maxsize=None)
def _attn_runs(B, L, S, width, regime):
    """The device results of one case, shared by the tests below: two runs with the grid
    gradient and one without."""
    inputs = _attn_case(B, L, S, width, regime)[0]
    dev = tuple(t.cuda() for t in inputs)
    return _AttnRun(dev), _AttnRun(dev), _AttnRun(dev, with_dgt=False)


def _attn_params(f):
    f = pytest.mark.parametrize("B,L,S,width", ATTN_SHAPES)(f)
    return pytest.mark.parametrize("regime", REGIMES)(f)


@_attn_params
def test_bagattn_matches_fp64(B, L, S, width, regime):
    _, ref, orc, env = _attn_case(B, L, S, width, regime)
    run = _attn_runs(B, L, S, width, regime)[0]
    tag = f"attn B={B} L={L} S={S} width={width} {regime}"
    for k in run.g:
        assert torch.isfinite(run[k]).all(), k
    # sharp: A is one-hot to fp32 and M ~ 0 (its entries are products with A's vanished tail)
    names = [k for k in ATTN_NAMES if not (regime == "sharp" and k == "M")]
    _check(tag, run, ref, env, names)
    _check(tag, run, orc, env, ("y", "du", "dgt"), "oracle autograd")


@_attn_params
def test_bagattn_null_grid_grad_gives_the_same_du(B, L, S, width, regime):
    """Training passes dgt = NULL (the grid needs no gradient): dx_kernel then groups its rows
    from row 2 on.  Each row's sum runs in the same order either way."""
    full, _, nogrid = _attn_runs(B, L, S, width, regime)
    assert nogrid.g["du"].no_nan()
    assert torch.equal(full["du"], nogrid["du"])
    for k in ("A", "cs", "y", "dm", "M"):
        assert torch.equal(full[k], nogrid[k]), k


@_attn_params
def test_bagattn_is_deterministic(B, L, S, width, regime):
    first, second, _ = _attn_runs(B, L, S, width, regime)
    for k in first.g:
        assert torch.equal(first[k], second[k]), k


@_attn_params
def test_bagattn_writes_all_of_its_buffers_and_nothing_else(B, L, S, width, regime):
    for run in _attn_runs(B, L, S, width, regime):
        for k, gb in run.g.items():
            assert gb.margins_intact(), k
            assert gb.no_nan(), k


def test_bagattn_entry_points_reject_more_than_256_tokens():
    from blindno import BlindnoError
    call, ptr, _, sp = _api()
    B, L, S, width = 1, 255, 64, 2
    T = L + 2
    z = torch.zeros(B * L * S, device="cuda")
    outs = [Guarded(B, T, T) for _ in range(4)]
    with pytest.raises(BlindnoError):
        call("blindno_bagattn_fwd", ptr(z), ptr(z), ptr(z), ptr(z), ptr(outs[0].t), ptr(outs[1].t),
             ptr(outs[2].t), ptr(outs[3].t), B, L, S, width, sp())
    with pytest.raises(BlindnoError):
        call("blindno_bagattn_bwd", ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(outs[0].t),
             ptr(outs[1].t), ptr(outs[2].t), ptr(outs[3].t), None, B, L, S, width, sp())
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


def test_bag_attn_fn_wrapper():
    """ops.BagAttnFn: a non-contiguous u (the _c path), the grid gradient dgt.sum(0).t() against
    the oracle, and needs_input_grad with a grid that asks for none."""
    from blindno import ops
    B, L, S, width = 3, 5, 63, 5
    (grid, u, w, bias, dy), ref, orc, env = _attn_case(B, L, S, width, "mixed")
    u_nc = u.cuda().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    assert not u_nc.is_contiguous()
    gd = grid.cuda().requires_grad_(True)
    wd, bd, dyd = w.cuda().view(width, 1), bias.cuda(), dy.cuda()
    y = ops.BagAttnFn.apply(u_nc, gd, wd, bd)
    y.backward(dyd)
    got = {"y": y.detach(), "du": u_nc.grad, "ggrid": gd.grad}
    want = {"y": orc["y"], "du": orc["du"], "ggrid": orc["dgt"].sum(0).t()}
    # the batch sum of dgt is a torch fp32 sum of B = 3 terms: its envelope is that of the same
    # sum over the restatement's fp32 dgt

    def math_fn(*args):
        out = _attn_math(*args)
        out["ggrid"] = out["dgt"].sum(0).t()
        return out
    want64 = dict(ref, ggrid=ref["dgt"].sum(0).t())
    env = _envelope(math_fn, (grid, u, w, bias, dy), want64, ("y", "du", "ggrid"))
    assert tuple(gd.grad.shape) == (S, 2)
    _check("BagAttnFn", got, want, env, ("y", "du", "ggrid"), "oracle autograd")

    u2 = u_nc.detach().requires_grad_(True)
    g2 = grid.cuda()
    y2 = ops.BagAttnFn.apply(u2, g2, wd, bd)
    y2.backward(dyd)
    assert g2.grad is None
    assert torch.equal(y2, y) and torch.equal(u2.grad, u_nc.grad)
    # neither u nor the grid: nothing to differentiate
    assert not ops.BagAttnFn.apply(u_nc.detach(), g2, wd, bd).requires_grad


# ================================================================================= bag mean
def _bagmean_math(u, grid, w, bias, lw, dy, dt):
    """y = [grid, sum_l lw_l u_l] @ w.T + b (lw_l = 1 / L without weights) and its adjoints."""
    u, grid, w, bias, dy = (t.to(dt) for t in (u, grid, w, bias, dy))
    B, L, S = u.shape
    d = grid.shape[1]
    lwv = torch.full((L,), 1.0 / L, dtype=dt) if lw is None else lw.to(dt)
    ubar = (lwv.view(1, L, 1) * u).sum(1)                                  # (B, S)
    y = torch.cat((grid.unsqueeze(0).expand(B, S, d), ubar.unsqueeze(-1)), -1) @ w.t() + bias
    dubar = dy @ w[:, d]                                                   # (B, S)
    # blindno_bagmean_bwd's output: d ubar / L without weights, d ubar with (the wrapper scales)
    s = dubar / L if lw is None else dubar
    gu = lwv.view(1, L, 1) * dubar.unsqueeze(1)
    ggrid = torch.einsum("bsc,ce->se", dy, w[:, :d])
    return {"y": y, "s": s, "gu": gu, "ggrid": ggrid}


# B, L, S, d, width, weighted.  B * S is never a multiple of 16: the last wave holds idle quads.
BAGMEAN_CASES = [
    (2, 1, 37, 2, 1, False),
    (2, 3, 61, 1, 5, True),      # L < 4 with weights, d = 1 (the 1D models)
    (2, 4, 64, 2, 4, True),      # exactly one snapshot and one channel per quad lane
    (2, 7, 129, 1, 3, False),    # width < 4
    (1, 54, 4099, 2, 20, True),  # the flagship bag
]
BAGMEAN_NAMES = ("y", "s", "gu", "ggrid")


@functools.lru_cache(maxsize=None)
def _bagmean_case(B, L, S, d, width, weighted):
    gen = torch.Generator().manual_seed(7000 + 10 * S + L)
    u = torch.randn(B, L, S, generator=gen)
    grid = torch.rand(S, d, generator=gen) * 2 - 1
    w = torch.randn(width, d + 1, generator=gen)
    bias = torch.randn(width, generator=gen)
    dy = torch.randn(B, S, width, generator=gen)
    lw = None
    if weighted:                 # positive, unequal, summing to 1
        lw = torch.rand(L, generator=gen) + 0.25
        lw = lw / lw.sum()
        assert L == 1 or float(lw.max() / lw.min()) > 1.05
    inputs = (u, grid, w, bias, lw, dy)
    ref = _bagmean_math(*inputs, torch.float64)
    # the adjoints once more, by float64 autograd of the forward formula alone
    ud, gd = u.double().requires_grad_(True), grid.double().requires_grad_(True)
    lwv = torch.full((L,), 1.0 / L, dtype=torch.float64) if lw is None else lw.double()
    ubar = (lwv.view(1, L, 1) * ud).sum(1)
    feat = torch.cat((gd.unsqueeze(0).expand(B, S, d), ubar.unsqueeze(-1)), -1)
    ((feat @ w.double().t() + bias.double()) * dy.double()).sum().backward()
    assert _rel(ref["gu"], ud.grad) <= 1e-12 and _rel(ref["ggrid"], gd.grad) <= 1e-12
    env = _envelope(_bagmean_math, inputs, ref, BAGMEAN_NAMES)
    return inputs, ref, env


def _bagmean_direct(dev):
    call, ptr, _, sp = _api()
    u, grid, w, bias, lw, dy = dev
    B, L, S = u.shape
    d, width = grid.shape[1], w.shape[0]
    y, s = Guarded(B, S, width), Guarded(B, S)
    call("blindno_bagmean_fwd_w", ptr(u), ptr(grid), ptr(w), ptr(bias), ptr(lw), ptr(y.t), B, L, S, d,
         width, sp())
    call("blindno_bagmean_bwd", ptr(dy), ptr(w), ptr(s.t), B, S, d, width, 1 if lw is not None else L,
         sp())
    torch.cuda.synchronize()
    return {"y": y, "s": s}


@pytest.mark.parametrize("B,L,S,d,width,weighted", BAGMEAN_CASES)
def test_bagmean_kernels_match_fp64(B, L, S, d, width, weighted):
    inputs, ref, env = _bagmean_case(B, L, S, d, width, weighted)
    dev = tuple(None if t is None else t.cuda() for t in inputs)
    first, second = _bagmean_direct(dev), _bagmean_direct(dev)
    for k in ("y", "s"):
        assert first[k].margins_intact() and second[k].margins_intact(), k
        assert first[k].no_nan(), k
        assert torch.equal(first[k].t, second[k].t), k          # deterministic: a fixed quad order
    tag = f"bagmean B={B} L={L} S={S} d={d} width={width} lw={'yes' if weighted else 'no'}"
    _check(tag, {k: v.t for k, v in first.items()}, ref, env, ("y", "s"))
    if not weighted:             # the unweighted entry point is the weighted one with lw = NULL
        call, ptr, _, sp = _api()
        y0 = Guarded(B, S, width)
        call("blindno_bagmean_fwd", ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(y0.t), B, L,
             S, d, width, sp())
        torch.cuda.synchronize()
        assert y0.margins_intact() and torch.equal(y0.t, first["y"].t)


@pytest.mark.parametrize("B,L,S,d,width,weighted", BAGMEAN_CASES)
def test_bag_mean_fn_gradients(B, L, S, d, width, weighted):
    """ops.BagMeanFn: gu in its expand form (no weights) and its lw-scaled form, and the grid
    gradient's einsum."""
    from blindno import ops
    inputs, ref, env = _bagmean_case(B, L, S, d, width, weighted)
    u, grid, w, bias, lw, dy = (None if t is None else t.cuda() for t in inputs)
    u.requires_grad_(True)
    grid.requires_grad_(True)
    y = ops.BagMeanFn.apply(u, grid, w, bias, lw)
    y.backward(dy)
    assert tuple(u.grad.shape) == (B, L, S) and tuple(grid.grad.shape) == (S, d)
    tag = f"BagMeanFn B={B} L={L} S={S} d={d} width={width} lw={'yes' if weighted else 'no'}"
    _check(tag, {"y": y.detach(), "gu": u.grad, "ggrid": grid.grad}, ref, env, ("y", "gu", "ggrid"))
    # u alone: the grid's einsum is skipped, gu is the same bits
    u2 = u.detach().requires_grad_(True)
    y2 = ops.BagMeanFn.apply(u2, grid.detach(), w, bias, lw)
    y2.backward(dy)
    assert torch.equal(y2, y) and torch.equal(u2.grad, u.grad)
