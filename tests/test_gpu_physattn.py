"""The physics-attention and plane-LayerNorm entry points (csrc/physattn.hip,
include/blindno_physattn.h) called through the C ABI on sentinel-guarded buffers, against the
float64 restatement tests/transolver_ref.py (forward by formula, backward by float64 autograd).

Bar, per compared tensor: rel-L2 <= max(1e-5, 3 x e32), e32 the rel-L2 error of the same
computation done by torch in fp32 on the CPU against float64 on the same inputs.  Every output and
scratch buffer has 64 sentinel elements on each side, checked after the call; the interior starts
as NaN, so an element a kernel leaves unwritten shows.  Each case runs the forward and the backward
twice and requires the two results to be equal to the bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import transolver_ref as tr

pytestmark = pytest.mark.gpu

M = 64
SENT = 77777.0
HEADS, D, G, C = 4, 8, 16, 32

# S, H, W: fewer points than a wave; exactly 64; a ragged tail inside one workgroup; the
# reference grid (3721 = 14 x 256 + 137: several workgroups, ragged last); many snapshots
SHAPES = [(1, 5, 7), (3, 8, 8), (2, 9, 13), (2, 61, 61), (5, 24, 40)]
SPECIAL_SHAPES = [(2, 9, 13), (2, 61, 61)]
CASES = [(s, "random") for s in SHAPES] + [(s, r) for r in ("clamp", "onehot", "starve") for s in SPECIAL_SHAPES]
PARAMS = ("temperature", "Ws", "bs", "Wq", "Wk", "Wv", "Wo", "bo")


class Guarded:
    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * M,), SENT, device="cuda", dtype=torch.float32)
        self.buf[M:M + self.n] = float("nan")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * M)

    def get(self):
        assert bool((self.buf[:M] == SENT).all()) and bool((self.buf[M + self.n:] == SENT).all()), \
            "a kernel wrote outside its buffer"
        return self.buf[M:M + self.n].view(*self.shape)


def make_inputs(S, H, W, regime):
    g = torch.Generator().manual_seed(1000 * S + 10 * H + W + len(regime))
    N = H * W
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = {"xm": r(S, C, N), "fm": r(S, C, N), "dy": r(S, C, N), "res": r(S, C, N),
           "temperature": torch.tensor([0.5, 0.4, 0.7, 1.0]), "Ws": 0.5 * r(G, D), "bs": 0.1 * r(G),
           "Wq": 0.6 * r(D, D), "Wk": 0.6 * r(D, D), "Wv": 0.6 * r(D, D), "Wo": 0.3 * r(C, C), "bo": 0.1 * r(C)}
    if regime == "clamp":
        inp["temperature"] = torch.tensor([0.05, 0.1, 3.0, 7.0])
    elif regime == "onehot":
        inp["Ws"] = 400.0 * inp["Ws"]
    elif regime == "starve":
        inp["bs"][3] = -30.0
    return inp


def run_ref(inp, dt):
    t = {k: v.to(dt).clone().requires_grad_(k not in ("dy", "res")) for k, v in inp.items()}
    out = tr.phys_attn(t["xm"], t["fm"], *[t[k] for k in PARAMS], res=t["res"])
    (out["y"] * t["dy"]).sum().backward()
    res = {k: v.detach() for k, v in out.items()}
    res["w"] = res["w"].contiguous()
    res.update({"d" + k: t[k].grad for k in ("xm", "fm") + PARAMS})
    return res


_REF = {}


def reference(S, H, W, regime):
    key = (S, H, W, regime)
    if key not in _REF:
        inp = make_inputs(S, H, W, regime)
        r64, r32 = run_ref(inp, torch.float64), run_ref(inp, torch.float32)
        _REF[key] = (inp, r64, {k: rel(r32[k], r64[k]) for k in r64})
    return _REF[key]


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def run_gpu(inp, S, H, W):
    from blindno import _lib
    from blindno._lib import call, ptr, query
    N = H * W
    d = {k: v.cuda().contiguous() for k, v in inp.items()}
    xf = torch.cat((d["xm"], d["fm"]), 1).contiguous()               # the 64-channel layout
    st = _lib.stream_ptr()
    prm = [ptr(d[k]) for k in PARAMS]
    o = {"w": Guarded(S, HEADS, G, N), "tok": Guarded(S, HEADS, G, D), "norm": Guarded(S, HEADS, G),
         "A": Guarded(S, HEADS, G, G), "otok": Guarded(S, HEADS, G, D), "y": Guarded(S, C, N),
         "fscratch": Guarded(query("blindno_physattn_fwd_scratch_floats", S, H, W))}
    call("blindno_physattn_fwd", ptr(xf), ptr(xf[:, C:]), 2 * C * N, *prm, ptr(d["res"]), o["w"].ptr,
         o["tok"].ptr, o["norm"].ptr, o["A"].ptr, o["otok"].ptr, o["fscratch"].ptr, o["y"].ptr, S, H, W, st)
    b = {"dxf": Guarded(S, 2 * C, N), "bscratch": Guarded(query("blindno_physattn_bwd_scratch_floats", S, H, W)),
         "dtemperature": Guarded(HEADS), "dWs": Guarded(G, D), "dbs": Guarded(G), "dWq": Guarded(D, D),
         "dWk": Guarded(D, D), "dWv": Guarded(D, D), "dWo": Guarded(C, C), "dbo": Guarded(C)}
    dxf_fm = ctypes.c_void_p(b["dxf"].ptr.value + 4 * C * N)
    call("blindno_physattn_bwd", ptr(d["dy"]), ptr(xf), ptr(xf[:, C:]), 2 * C * N, *prm[:7], o["w"].ptr,
         o["tok"].ptr, o["norm"].ptr, o["A"].ptr, o["otok"].ptr, b["bscratch"].ptr, b["dxf"].ptr, dxf_fm,
         2 * C * N, b["dtemperature"].ptr, b["dWs"].ptr, b["dbs"].ptr, b["dWq"].ptr, b["dWk"].ptr,
         b["dWv"].ptr, b["dWo"].ptr, b["dbo"].ptr, S, H, W, st)
    torch.cuda.synchronize()
    got = {k: v.get().clone() for k, v in {**o, **b}.items() if not k.endswith("scratch")}
    for k in ("fscratch", "bscratch"):
        {**o, **b}[k].get()
    dxf = got.pop("dxf")
    got["dxm"], got["dfm"] = dxf[:, :C], dxf[:, C:]
    return got


@pytest.mark.parametrize("shape,regime", CASES)
def test_physattn_against_float64(shape, regime):
    S, H, W = shape
    inp, r64, e32 = reference(S, H, W, regime)
    if regime == "onehot":       # the slice weights are one-hot to fp32 almost everywhere
        assert float((r64["w"].float().max(2).values == 1.0).float().mean()) > 0.9
    if regime == "starve":       # norm[3] far below the 1e-5 that then decides the token
        assert float(r64["norm"][..., 3].max()) < 1e-6
    got = run_gpu(inp, S, H, W)
    again = run_gpu(inp, S, H, W)
    worst = []
    for k in sorted(got):
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
        e, bar = rel(got[k], r64[k]), max(1e-5, 3 * e32[k])
        print(f"{S}x{H}x{W} {regime:7s} {k:13s} rel-L2 {e:.2e}  bar {bar:.2e}  (fp32 torch {e32[k]:.2e})")
        if e > bar:
            worst.append((k, e, bar))
    if regime == "clamp":        # heads 0 and 3 sit outside [0.1, 5]; 0.1 itself passes
        dt = got["dtemperature"].cpu()
        assert float(dt[0]) == 0.0 and float(dt[3]) == 0.0 and float(dt[1]) != 0.0 and float(dt[2]) != 0.0
        assert float(r64["dtemperature"][0]) == 0.0 and float(r64["dtemperature"][3]) == 0.0
    assert not worst, worst


def _ln_case(S, H, W):
    g = torch.Generator().manual_seed(7 * S + H + W)
    N = H * W
    x = torch.randn(S, C, N, generator=g) * 2.0 + 0.5
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(S, C, N, generator=g)

    def run(dt):
        t = [v.to(dt).clone().requires_grad_(True) for v in (x, gamma, beta)]
        y = tr.layer_norm(*t, eps=1e-5)
        (y * dy.to(dt)).sum().backward()
        return {"y": y.detach(), "dx": t[0].grad, "dgamma": t[1].grad, "dbeta": t[2].grad}
    r64, r32 = run(torch.float64), run(torch.float32)
    return (x, gamma, beta, dy), r64, {k: rel(r32[k], r64[k]) for k in r64}


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_ln_planes_against_float64(S, H, W):
    from blindno import _lib
    from blindno._lib import call, ptr, query
    (x, gamma, beta, dy), r64, e32 = _ln_case(S, H, W)
    N = H * W
    xd, gd, bd, dyd = (t.cuda().contiguous() for t in (x, gamma, beta, dy))
    st = _lib.stream_ptr()

    def run():
        o = {"y": Guarded(S, C, N), "mean": Guarded(S, N), "rstd": Guarded(S, N), "dx": Guarded(S, C, N),
             "dgamma": Guarded(C), "dbeta": Guarded(C),
             "partial": Guarded(S * query("blindno_ln_planes_nblk", N) * 2 * C)}
        call("blindno_ln_planes_fwd", ptr(xd), ptr(gd), ptr(bd), o["y"].ptr, o["mean"].ptr, o["rstd"].ptr,
             S, C, N, 1e-5, st)
        call("blindno_ln_planes_bwd", ptr(dyd), ptr(xd), ptr(gd), o["mean"].ptr, o["rstd"].ptr, o["dx"].ptr,
             o["dgamma"].ptr, o["dbeta"].ptr, o["partial"].ptr, S, C, N, st)
        torch.cuda.synchronize()
        return {k: v.get().clone() for k, v in o.items()}
    got, again = run(), run()
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(got[k], again[k]), k
        e, bar = rel(got[k], r64[k]), max(1e-5, 3 * e32[k])
        print(f"ln {S}x{H}x{W} {k:7s} rel-L2 {e:.2e}  bar {bar:.2e}")
        assert e <= bar, (k, e, bar)
    assert torch.isfinite(got["mean"]).all() and torch.isfinite(got["rstd"]).all()


def test_unsupported_configurations_are_refused():
    from blindno import ops
    from blindno._lib import query
    assert query("blindno_physattn_ok", 2, 61, 61, 4, 8, 16) == 1
    for bad in [(2, 61, 61, 8, 8, 16), (2, 61, 61, 4, 16, 16), (2, 61, 61, 4, 8, 32), (0, 61, 61, 4, 8, 16),
                (2, 0, 61, 4, 8, 16)]:
        assert query("blindno_physattn_ok", *bad) == 0, bad
    assert query("blindno_physattn_fwd_scratch_floats", 2, 61, 61) == 2 * 4 * 15 * 144
    assert query("blindno_physattn_nblk", 61, 61) == 15 and query("blindno_physattn_nblk", 0, 3) == -1
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    ok = dict(xf=z(1, 64, 4, 4), t=z(1, 4, 1, 1) + 0.5, Ws=z(16, 8), bs=z(16), Wq=z(8, 8), Wo=z(32, 32), bo=z(32))

    def apply(**kw):
        a = {**ok, **kw}
        return ops.PhysAttnFn.apply(a["xf"], a["t"], a["Ws"], a["bs"], a["Wq"], a["Wq"], a["Wq"], a["Wo"], a["bo"])
    assert tuple(apply().shape) == (1, 32, 4, 4)
    with pytest.raises(ValueError, match="heads = 4"):
        apply(t=z(1, 8, 1, 1) + 0.5, xf=z(1, 128, 4, 4))
    with pytest.raises(ValueError, match="heads = 4"):
        apply(Ws=z(32, 8), bs=z(32))
    with pytest.raises(ValueError, match="heads = 4"):
        apply(Ws=z(16, 16), xf=z(1, 128, 4, 4))
    with pytest.raises(ValueError):
        ops.LayerNormPlanesFn.apply(z(1, 16, 4, 4), z(16), z(16), 1e-5)
