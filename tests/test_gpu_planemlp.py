"""The fused plane-MLP entry points (csrc/planemlp.hip, include/blindno_planemlp.h) called through
the C ABI on sentinel-guarded buffers, against the float64 restatement
tests/transolver3d_ref.plane_mlp (forward by formula, backward by float64 autograd).

Bar, per compared tensor, as in tests/test_gpu_physattn.py: rel-L2 <= max(1e-5, 3 x e32), e32 the
rel-L2 error of the same computation composed by torch in fp32 on the CPU (LayerNorm, Linear, GELU,
Linear, add) against float64 on the same inputs.  Every output and the scratch have 64 sentinel
elements on each side, checked after the call; the interior starts as NaN, so an element a kernel
leaves unwritten shows.  Each case runs twice and requires the two results to be equal to the bit.
Weights, gains and biases are O(1), so a transposed weight moves every result by O(1).
"""
import ctypes

import numpy as np
import pytest
import torch

import transolver3d_ref as t3

pytestmark = pytest.mark.gpu

M = 64
SENT = 77777.0
CONFIGS = {"block": (32, 32, 32, True), "preprocess": (4, 64, 32, False)}
# one partial workgroup, an exact one, a one-point tail, three workgroups
NS = (1, 255, 256, 257, 513)
CASES = [(c, S, N, res, False) for c in CONFIGS for S in (1, 3) for N in NS for res in (True, False)]
# activations that are channel slices of tensors twice as wide (the 64-channel-tensor case)
CASES += [(c, 3, 257, True, True) for c in CONFIGS] + [(c, 1, 256, False, True) for c in CONFIGS]


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


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def make_inputs(cfg, S, N):
    Cin, Chid, Cout, ln = CONFIGS[cfg]
    g = torch.Generator().manual_seed(1000 * S + N + Cin)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = {"x": 2.0 * r(S, Cin, N) + 0.5, "dy": r(S, Cout, N), "res": r(S, Cout, N),
           "W1": r(Chid, Cin) / Cin ** 0.5, "b1": 0.5 * r(Chid), "W2": r(Cout, Chid) / Chid ** 0.5 * 2.0,
           "b2": 0.5 * r(Cout)}
    if ln:
        inp.update(gamma=1.0 + 0.5 * r(Cin), beta=0.5 * r(Cin))
    return inp


PARAMS = ("W1", "b1", "W2", "b2", "gamma", "beta")


def run_ref(inp, dt, with_res):
    t = {k: v.to(dt).clone().requires_grad_(k not in ("dy", "res")) for k, v in inp.items()}
    y = t3.plane_mlp(t["x"], t["W1"], t["b1"], t["W2"], t["b2"], t["res"] if with_res else None,
                     t.get("gamma"), t.get("beta"))
    (y * t["dy"]).sum().backward()
    out = {"y": y.detach(), "dx": t["x"].grad}
    out.update({"d" + k: t[k].grad for k in PARAMS if k in t})
    return out


_REF = {}


def reference(cfg, S, N, with_res):
    key = (cfg, S, N, with_res)
    if key not in _REF:
        inp = make_inputs(cfg, S, N)
        r64, r32 = run_ref(inp, torch.float64, with_res), run_ref(inp, torch.float32, with_res)
        _REF[key] = (inp, r64, {k: rel(r32[k], r64[k]) for k in r64})
    return _REF[key]


def run_gpu(cfg, inp, S, N, with_res, wide):
    from blindno import _lib
    from blindno._lib import call, ptr, query
    Cin, Chid, Cout, ln = CONFIGS[cfg]
    d = {k: v.cuda().contiguous() for k, v in inp.items()}
    k = 2 if wide else 1                       # channel slices [C, 2 C) of tensors k times as wide

    def widen(t):
        if not wide:
            return t, t
        w = torch.full((S, 2 * t.shape[1], N), 3.0e4, device="cuda")
        w[:, t.shape[1]:] = t
        return w, w[:, t.shape[1]:]
    xw, x = widen(d["x"])
    rw, res = widen(d["res"])
    dyw, dy = widen(d["dy"])
    st = _lib.stream_ptr()
    o = {"y": Guarded(S, k * Cout, N), "dx": Guarded(S, k * Cin, N), "dW1": Guarded(Chid, Cin), "db1": Guarded(Chid),
         "dW2": Guarded(Cout, Chid), "db2": Guarded(Cout),
         "scratch": Guarded(query("blindno_plane_mlp_bwd_scratch_floats", S, N, Cin, Chid, Cout))}
    if ln:
        o.update(mean=Guarded(S, N), rstd=Guarded(S, N), dgamma=Guarded(Cin), dbeta=Guarded(Cin))
    op = lambda n: o[n].ptr if n in o else None  # noqa: E731
    off = lambda n, c: ctypes.c_void_p(o[n].ptr.value + (4 * c * N if wide else 0))  # noqa: E731
    call("blindno_plane_mlp_fwd", ptr(x), k * Cin * N, ptr(d.get("gamma")), ptr(d.get("beta")), ptr(d["W1"]),
         ptr(d["b1"]), ptr(d["W2"]), ptr(d["b2"]), ptr(res) if with_res else None, k * Cout * N, off("y", Cout),
         k * Cout * N, op("mean"), op("rstd"), S, N, Cin, Chid, Cout, 1e-5, st)
    call("blindno_plane_mlp_bwd", ptr(dy), k * Cout * N, ptr(x), k * Cin * N, ptr(d.get("gamma")),
         ptr(d.get("beta")), ptr(d["W1"]), ptr(d["b1"]), ptr(d["W2"]), op("mean"), op("rstd"), o["scratch"].ptr,
         off("dx", Cin), k * Cin * N, o["dW1"].ptr, o["db1"].ptr, o["dW2"].ptr, o["db2"].ptr, op("dgamma"),
         op("dbeta"), S, N, Cin, Chid, Cout, st)
    torch.cuda.synchronize()
    got = {n: v.get().clone() for n, v in o.items()}
    got.pop("scratch")
    if wide:                                   # the other half of the wide outputs is untouched
        for n, c in (("y", Cout), ("dx", Cin)):
            assert bool(torch.isnan(got[n][:, :c]).all()), n
            got[n] = got[n][:, c:]
    del xw, rw, dyw
    return got


@pytest.mark.parametrize("cfg,S,N,with_res,wide", CASES)
def test_plane_mlp_against_float64(cfg, S, N, with_res, wide):
    inp, r64, e32 = reference(cfg, S, N, with_res)
    got = run_gpu(cfg, inp, S, N, with_res, wide)
    again = run_gpu(cfg, inp, S, N, with_res, wide)
    bad = []
    for k in sorted(got):
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
        if k in ("mean", "rstd"):
            continue
        e, bar = rel(got[k], r64[k]), max(1e-5, 3 * e32[k])
        print(f"{cfg} S={S} N={N} res={with_res} wide={wide} {k:7s} rel-L2 {e:.2e}  bar {bar:.2e}  "
              f"(fp32 torch {e32[k]:.2e})")
        if e > bar:
            bad.append((k, e, bar))
    if "mean" in got:
        x = inp["x"].double()
        m, v = x.mean(1), x.var(1, unbiased=False)
        assert rel(got["mean"], m) <= 1e-5 and rel(got["rstd"], (v + 1e-5).rsqrt()) <= 1e-5
    assert not bad, bad


def test_transposed_weights_move_the_result():
    """The inputs tell W from its transpose: the float64 result with W1 and W2 transposed is O(1)
    away, so the bars above cannot pass a wrong index order."""
    inp, r64, _ = reference("block", 1, 255, True)
    t = dict(inp, W1=inp["W1"].t().contiguous(), W2=inp["W2"].t().contiguous())
    wrong = run_ref(t, torch.float64, True)
    assert rel(wrong["y"], r64["y"]) > 0.3 and rel(wrong["dx"], r64["dx"]) > 0.3


def test_refusals_launch_nothing():
    from blindno import BlindnoError, _lib, ops
    from blindno._lib import call, ptr, query
    S, N = 2, 300
    inp = make_inputs("block", S, N)
    d = {k: v.cuda().contiguous() for k, v in inp.items()}
    st = _lib.stream_ptr()
    o = {n: Guarded(*s) for n, s in dict(y=(S, 32, N), mean=(S, N), rstd=(S, N), dx=(S, 32, N), dW1=(32, 32),
                                         db1=(32,), dW2=(32, 32), db2=(32,), dgamma=(32,), dbeta=(32,)).items()}
    o["scratch"] = Guarded(query("blindno_plane_mlp_bwd_scratch_floats", S, N, 32, 32, 32))

    def fwd(**kw):
        a = dict(x=ptr(d["x"]), xs=32 * N, gamma=ptr(d["gamma"]), beta=ptr(d["beta"]), W1=ptr(d["W1"]), b1=ptr(d["b1"]),
                 W2=ptr(d["W2"]), b2=ptr(d["b2"]), res=ptr(d["res"]), rs=32 * N, y=o["y"].ptr, ys=32 * N,
                 mean=o["mean"].ptr, rstd=o["rstd"].ptr, S=S, N=N, Cin=32, Chid=32, Cout=32)
        a.update(kw)
        call("blindno_plane_mlp_fwd", a["x"], a["xs"], a["gamma"], a["beta"], a["W1"], a["b1"], a["W2"], a["b2"],
             a["res"], a["rs"], a["y"], a["ys"], a["mean"], a["rstd"], a["S"], a["N"], a["Cin"], a["Chid"],
             a["Cout"], 1e-5, st)

    def bwd(**kw):
        a = dict(dy=ptr(d["dy"]), dys=32 * N, x=ptr(d["x"]), xs=32 * N, gamma=ptr(d["gamma"]), beta=ptr(d["beta"]),
                 W1=ptr(d["W1"]), b1=ptr(d["b1"]), W2=ptr(d["W2"]), mean=o["mean"].ptr, rstd=o["rstd"].ptr,
                 scratch=o["scratch"].ptr, dx=o["dx"].ptr, dxs=32 * N, dW1=o["dW1"].ptr, db1=o["db1"].ptr,
                 dW2=o["dW2"].ptr, db2=o["db2"].ptr, dgamma=o["dgamma"].ptr, dbeta=o["dbeta"].ptr, S=S, N=N, Cin=32,
                 Chid=32, Cout=32)
        a.update(kw)
        call("blindno_plane_mlp_bwd", a["dy"], a["dys"], a["x"], a["xs"], a["gamma"], a["beta"], a["W1"], a["b1"],
             a["W2"], a["mean"], a["rstd"], a["scratch"], a["dx"], a["dxs"], a["dW1"], a["db1"], a["dW2"], a["db2"],
             a["dgamma"], a["dbeta"], a["S"], a["N"], a["Cin"], a["Chid"], a["Cout"], st)

    both = [dict(S=0), dict(S=65536), dict(N=0), dict(N=(1 << 24) + 1), dict(xs=32 * N - 1), dict(Cin=16),
            dict(Chid=64), dict(Cout=1), dict(Cin=4, Chid=64), dict(x=None), dict(W1=None), dict(b1=None),
            dict(W2=None), dict(gamma=None), dict(beta=None), dict(mean=None), dict(rstd=None)]
    for kw in both + [dict(ys=32 * N - 1), dict(rs=32 * N - 1), dict(y=None), dict(b2=None)]:
        with pytest.raises(BlindnoError, match="blindno_plane_mlp_fwd"):
            fwd(**kw)
    for kw in both + [dict(dys=32 * N - 1), dict(dxs=32 * N - 1), dict(dy=None), dict(scratch=None), dict(dx=None),
                      dict(dW1=None), dict(db1=None), dict(dW2=None), dict(db2=None), dict(dgamma=None),
                      dict(dbeta=None)]:
        with pytest.raises(BlindnoError, match="blindno_plane_mlp_bwd"):
            bwd(**kw)
    torch.cuda.synchronize()
    for n, v in o.items():                     # nothing was launched: every buffer is as it was made
        assert bool(torch.isnan(v.get()).all()), n
    # a valid call on the same stream is still right afterwards
    fwd()
    bwd()
    torch.cuda.synchronize()
    r = run_ref(inp, torch.float64, True)
    r32 = run_ref(inp, torch.float32, True)
    for n in ("y", "dx", "dW1", "db1", "dW2", "db2", "dgamma", "dbeta"):
        assert rel(o[n].get(), r[n]) <= max(1e-5, 3 * rel(r32[n], r[n])), n
    # the autograd op: unsupported triples are ValueErrors, CPU tensors BlindnoErrors
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match=r"\(32, 32, 32\)"):
        ops.PlaneMLPFn.apply(z(1, 16, 8), z(16, 16), z(16), z(16, 16), z(16))
    with pytest.raises(ValueError, match=r"\(32, 32, 32\)"):
        ops.PlaneMLPFn.apply(z(1, 32, 8), z(32, 32), z(32), z(32, 32), z(32))
    with pytest.raises(BlindnoError):
        ops.PlaneMLPFn.apply(torch.zeros(1, 4, 8), z(64, 4), z(64), z(32, 64), z(32))
    assert tuple(ops.PlaneMLPFn.apply(z(1, 4, 2, 2, 2), z(64, 4), z(64), z(32, 64), z(32)).shape) == (1, 32, 2, 2, 2)
