"""The lift kernels (csrc/fields.hip, csrc/liftw.h), the lift's adjoint with its hosted weight
gradients, and the 1x1-conv weight gradient (csrc/fields.hip, conv_wgrad_mfma_block of
csrc/wgrad.h) called through the C ABI against the float64 references of tests/lift_ref.py, on
every launch path the host code selects.  The case tables live in lift_ref (the host test checks
the same inputs); each id ends in the instantiation the dispatcher selects (lift_ref.fwd_path /
bwd_path / conv_path; DESIGN.md "Lift and conv weight-gradient launch paths" has the table):

  forward   wide12x16 = lift_fwd_wide_kernel<12, 16>, pt16 = lift_fwd_pt_kernel<16>,
            generic = lift_fwd_kernel
  backward  both1 = lift_bwd_both_kernel<1> (input gradient, matrix-core weight gradient and the
            hosted spectral weight gradient in one launch); otherwise in_wide =
            lift_bwd_in_wide_kernel<12, 16> or in_generic = lift_bwd_in_kernel, then mfma1 / mfma2 =
            lift_bwd_w_mfma_kernel<1 / 2> or lds = lift_bwd_w_kernel
  conv      mfma_act{0,1}_{vec,scalar} = conv_wgrad_mfma_kernel<ACT> with float4 or scalar loads,
            lds_act{0,1} = conv_wgrad_kernel<ACT>

The acceptance bound is per element and derived (lift_ref's docstring).  Every output and scratch
buffer lies between sentinel margins, which are checked after each call; the interior is
pre-filled with NaN where the kernel must write every element (x0 with its padding, d_in, the
partial rows, dWt and its slice partials) and with the sentinel where it must write nothing (the
refusals).  Weights of grouped launches are packed [W0 | b0 | NaN gap] per group, so a read past a
group's block shows.  The per-workgroup partial rows are summed on the host in float64; one case
per family also goes through blindno_reduce_partials.  Every call runs twice and must agree to
the bit, and every check prints its worst err / bound ratio.
"""
import numpy as np
import pytest
import torch

import lift_ref as lr
from lift_ref import Guarded, worst
from spectral_stage_ref import SENT, cplx

pytestmark = pytest.mark.gpu

INVALID = 1              # hipErrorInvalidValue
SENT32 = np.float32(SENT)
GAP = 37                 # NaN floats between the groups' weight blocks


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _api():
    from blindno._lib import load, ptr, query, stream_ptr
    return load(), ptr, query, stream_ptr


def _dev(a, misalign=False):
    """A flat device copy; misalign: offset by one float from the allocation (not 16-B aligned)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if not misalign:
        return torch.from_numpy(a).cuda()
    d = torch.from_numpy(np.concatenate([np.full(1, np.nan, np.float32), a])).cuda()[1:]
    assert d.data_ptr() % 16 == 4
    return d


def _nan(n, lead=0):
    """A Guarded of lead + n floats whose last n are NaN (the lead floats stay sentinels)."""
    g = Guarded(lead + n)
    g.t[lead:].fill_(float("nan"))
    g.view = g.t[lead:]
    g.lead = lead
    return g


def _intact(g):
    return g.margins_intact() and bool((g.t[:g.lead] == SENT).all())


def _ratio(label, got, ref, bound):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    assert np.isfinite(got).all(), label + ": an element was never written"
    r = worst(np.abs(got - ref), np.broadcast_to(bound, np.shape(ref)))
    print(f"{label}: worst err/bound {r:.3f}")
    assert r <= 1.0, (label, r)
    return r


def _pack_w(t, c):
    """-> (device buffer, wgs): group g's [W0 (C Cin) | b0 (C)] at g wgs, NaN between the blocks."""
    G, C, Cin = c["G"], c["C"], c["Cin"]
    wgs = C * Cin + C + GAP
    w = np.full(G * wgs, np.nan, np.float32)
    for g in range(G):
        w[g * wgs:g * wgs + C * Cin] = t["w0"][g].ravel()
        w[g * wgs + C * Cin:g * wgs + C * Cin + C] = t["b0"][g]
    return _dev(w), wgs


def _bag_args(c, t, ptr, both):
    if not c["bag"]:
        return (None, None, None, None, 1.0) + ((1.0,) if both else ())
    d = [_dev(t[k]) for k in ("ubar", "grid", "bw", "bb")]
    t.setdefault("_keep", []).extend(d)
    return tuple(ptr(x) for x in d) + ((c["bag"][0], c["bag"][1]) if both else (c["bag"][0],))


# ================================================================================ forward
def _fwd(c, t):
    lib, ptr, _, sp = _api()
    G, Bg, C, Cin = c["G"], c["Bg"], c["C"], c["Cin"]
    w, wgs = _pack_w(t, c)
    x0 = _nan(G * Bg * C * c["P"][0] * c["P"][1])
    inp = None if c["bag"] else _dev(t["inp"], c["mis_in"])
    rc = lib.blindno_lift_fwd_bag_g(ptr(inp), ptr(w), ptr(w[C * Cin:]), ptr(x0.view), G, wgs, G * Bg, *c["N"], Cin, C,
                                    *c["P"], *_bag_args(c, t, ptr, False), sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    assert _intact(x0)
    return x0


@pytest.mark.parametrize("c", lr.FWD_CASES, ids=lr.fwd_id)
def test_lift_fwd_vs_fp64(c):
    t = lr.lift_inputs(c)
    h, dh = lr.case_input64(c, t)
    a = (h, t["w0"], t["b0"], c["N"], c["P"], c["G"])
    x0, again = _fwd(c, t), _fwd(c, t)
    got = x0.cpu().numpy().reshape(c["G"] * c["Bg"], c["C"], *c["P"])
    assert np.all(got[:, :, c["N"][0]:, :] == 0) and np.all(got[:, :, :, c["N"][1]:] == 0), "the padding is not 0"
    _ratio(lr.fwd_id(c) + " x0", got, lr.lift_fwd(*a), lr.lift_fwd_bound(*a, dh=dh))
    if c["identity"]:
        # _grid_planes: the lift with unit weights reproduces its input and the constant plane exactly
        N1, N2 = c["N"]
        assert np.array_equal(got[0, :2, :N1, :N2], t["inp"][0].transpose(2, 0, 1))
        assert np.all(got[0, 2, :N1, :N2] == 1.0)
    assert torch.equal(x0.buf, again.buf), "not bit-reproducible"


def test_invalid_lift_fwd_calls_are_refused_on_the_host():
    lib, ptr, _, sp = _api()
    src = torch.zeros(1 << 15, device="cuda")
    out = Guarded(1 << 15)
    p, q = ptr(src), ptr(out.t)

    def fwd(G=1, Bn=2, N=(5, 16), Cin=12, C=12, P=(7, 20), bag=(None, None, None, None)):
        return int(lib.blindno_lift_fwd_bag_g(p, p, p, q, G, 512, Bn, *N, Cin, C, *P, *bag, 1.0, sp()))

    assert fwd() == 0                                                             # the valid neighbour
    assert fwd(N=(8, 16)) == INVALID and fwd(N=(5, 21)) == INVALID                # N > P
    assert fwd(G=2, Bn=3) == INVALID and fwd(G=0) == INVALID                      # Bn % G != 0
    out.buf.fill_(SENT)
    torch.cuda.synchronize()
    assert fwd(bag=(p, p, p, p)) == 0                                             # the valid bag neighbour
    out.buf.fill_(SENT)
    for bag in ((p, None, p, p), (p, p, None, p), (p, p, p, None)):               # ubar without grid / bw / bb
        assert fwd(bag=bag) == INVALID
    assert fwd(Cin=8, bag=(p, p, p, p)) == INVALID                                # ubar with Cin != 12
    assert fwd(C=4, bag=(p, p, p, p)) == INVALID and fwd(C=17, bag=(p, p, p, p)) == INVALID
    assert fwd(G=5, Bn=5, bag=(p, p, p, p)) == INVALID                            # ubar with G > kLiftMaxG
    assert fwd(N=(8, 16), bag=(p, p, p, p)) == INVALID
    torch.cuda.synchronize()
    assert out.untouched()


# ================================================================================ backward
def _bwd(c, t, want_in, want_w, mix, nchunk=None):
    """One backward call -> dict of Guarded buffers (d_in, part, dWt, mpart as asked) and nchunk."""
    lib, ptr, query, sp = _api()
    G, Bg, C, Cin, (N1, N2) = c["G"], c["Bg"], c["C"], c["Cin"], c["N"]
    w, wgs = _pack_w(t, c)
    dx0 = _dev(t["dx0"], c["mis_dx0"])
    inp = None if c["bag"] else _dev(t["inp"])
    nch = query("blindno_lift_bwd_nchunk", Bg, N1, N2) if nchunk is None else nchunk
    assert nchunk is not None or nch == lr.lift_bwd_nchunk(Bg, c["N"])
    r = {"nchunk": nch}
    if want_in:
        r["d_in"] = _nan(Bg * N1 * N2 * (1 if c["bag"] else Cin), lead=1 if c["mis_din"] else 0)
        assert not c["mis_din"] or r["d_in"].view.data_ptr() % 16 == 4
    if want_w:
        r["part"] = _nan(nch * G * (C * Cin + C))
    margs = (None, None, None, None, 1, 0, 0)
    if mix:
        K1, m2, ns = c["mix"]
        ns = ns or query("blindno_mix_wgrad_nsplit", Bg, C, C, K1, m2)
        xs, gs = _dev(t["Xs"]), _dev(t["Gs"])
        r["dWt"] = _nan(2 * m2 * K1 * C * C * G)
        r["mpart"] = _nan(ns * 2 * m2 * K1 * C * C * G) if ns > 1 else None
        r["ns"] = ns
        margs = (ptr(xs), ptr(gs), ptr(r["dWt"].view), ptr(r["mpart"].view) if ns > 1 else None, ns, K1, m2)
    head = (ptr(dx0), ptr(inp), ptr(w), ptr(r["d_in"].view) if want_in else None,
            ptr(r["part"].view) if want_w else None, nch if want_w else 0)
    dims = (G * Bg, N1, N2, Cin, C, *c["P"])
    if c["bag"]:
        rc = lib.blindno_lift_bwd_bag_mix_g(*head, G, wgs, *dims, *margs, *_bag_args(c, t, ptr, True), sp())
    elif mix:
        rc = lib.blindno_lift_bwd_mix_g(*head, G, wgs, *dims, *margs, sp())
    elif G == 1:
        rc = lib.blindno_lift_bwd(*head, *dims, sp())
    else:
        rc = lib.blindno_lift_bwd_g(*head, G, wgs, *dims, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    for k in ("d_in", "part", "dWt", "mpart"):
        assert r.get(k) is None or _intact(r[k]), k + ": written outside the buffer"
    return r


def _same(a, b):
    return all(a.get(k) is None or torch.equal(a[k].view, b[k].view) for k in ("d_in", "part", "dWt"))


def _rows(part, nchunk, G):
    p = part.view.cpu().double().numpy().reshape(nchunk, G, -1)
    assert np.isfinite(p).all(), "a partial row was never written"
    return p.sum(0)


def _reduced(part, nchunk, n):
    lib, ptr, _, sp = _api()
    out = _nan(n)
    assert lib.blindno_reduce_partials(ptr(part.view), ptr(out.view), nchunk, n, sp()) == 0
    torch.cuda.synchronize()
    assert _intact(out)
    return out.view.cpu().numpy()


def _check_bwd(c, t, r, label):
    N, G = c["N"], c["G"]
    h, dh = lr.case_input64(c, t)
    if "d_in" in r:
        got = r["d_in"].view.cpu().numpy()
        if c["bag"]:
            _ratio(label + " d_ubar", got, lr.bag_dubar(lr.lift_bwd_in(t["dx0"], t["w0"], N, G), t["bw"], c["bag"][1]),
                   lr.bag_dubar_bound(t["dx0"], t["w0"], N, G, t["bw"], c["bag"][1]))
        else:
            _ratio(label + " d_in", got, lr.lift_bwd_in(t["dx0"], t["w0"], N, G),
                   lr.lift_bwd_in_bound(t["dx0"], t["w0"], N, G))
    if "part" in r:
        ref, bound = lr.lift_bwd_w(t["dx0"], h, N, G), lr.lift_bwd_w_bound(t["dx0"], h, N, G, dh=dh)
        _ratio(label + " dW0|db0", _rows(r["part"], r["nchunk"], G), ref, bound)
        if c["reduce"]:
            assert r["nchunk"] > 1
            _ratio(label + " dW0|db0 reduce_partials", _reduced(r["part"], r["nchunk"], ref.size), ref, bound)
    if "dWt" in r:
        X, Y = cplx(t["Xs"]), cplx(t["Gs"])
        ref = lr.mix_wgrad(X, Y, G)
        b = lr.mix_wgrad_bound(X, Y, G, r["ns"])[..., None]
        _ratio(f"{label} dWt mnsplit={r['ns']}", r["dWt"].view.cpu().numpy(), np.stack([ref.real, ref.imag], -1),
               np.broadcast_to(b, b.shape[:-1] + (2,)))
        if r["mpart"] is not None:
            assert bool(torch.isfinite(r["mpart"].view).all()), "a slice partial was never written"


@pytest.mark.parametrize("c", lr.BWD_CASES, ids=lr.bwd_id)
def test_lift_bwd_vs_fp64(c):
    t = lr.lift_inputs(c)
    a = (c["want_in"], c["want_w"], bool(c["mix"]))
    r = _bwd(c, t, *a)
    _check_bwd(c, t, r, lr.bwd_id(c))
    assert _same(r, _bwd(c, t, *a)), "not bit-reproducible"
    if lr.bwd_path(c) == "both1" and not c["bag"]:
        # the merged launch keeps the grid of each part's own launch: bit-identical to the separate calls
        lib, ptr, _, sp = _api()
        sep = {"d_in": _bwd(c, t, True, False, False)["d_in"], "part": _bwd(c, t, False, True, False)["part"]}
        if c["mix"]:
            K1, m2, _ = c["mix"]
            C, G, ns = c["C"], c["G"], r["ns"]
            xs, gs = _dev(t["Xs"]), _dev(t["Gs"])
            sep["dWt"] = _nan(2 * m2 * K1 * C * C * G)
            mp = _nan(ns * 2 * m2 * K1 * C * C * G)
            rc = lib.blindno_mix_wgrad_g(ptr(xs), ptr(gs), ptr(sep["dWt"].view), ptr(mp.view) if ns > 1 else None, ns, G,
                                         G * c["Bg"], C, C, K1, m2, sp())
            assert rc == 0
            torch.cuda.synchronize()
            assert _intact(sep["dWt"]) and _intact(mp)
        assert _same(sep, r), "the merged launch differs from the separate launches"


def test_mix_nsplit_cases_include_empty_slices():
    """One mnsplit of the hosted mix cases exceeds Bg: its last slices hold no sample and must write 0."""
    _, _, query, _ = _api()
    cs = [c for c in lr.BWD_CASES if c["mix"]]
    ns = {c["mix"][2] or query("blindno_mix_wgrad_nsplit", c["Bg"], c["C"], c["C"], *c["mix"][:2]) for c in cs}
    assert {1, 2} <= ns and max(ns) > max(c["Bg"] for c in cs)


def test_invalid_lift_bwd_calls_are_refused_on_the_host():
    """Every refusal comes before the first launch: d_in, partial, dWt and mpartial keep the sentinel."""
    lib, ptr, _, sp = _api()
    src = torch.zeros(1 << 15, device="cuda")
    outs = [Guarded(1 << 15) for _ in range(4)]
    p = ptr(src)
    qi, qp, qw, qm = (ptr(o.t) for o in outs)
    bagp = (p, p, p, p)

    def bwd(G=2, Bn=4, N=(5, 16), Cin=12, C=12, P=(7, 20), d_in=qi, part=qp, nchunk=1, mix=(None, None, None, None, 1, 0, 0),
            bag=(None, None, None, None)):
        return int(lib.blindno_lift_bwd_bag_mix_g(p, p, p, d_in, part, nchunk, G, 512, Bn, *N, Cin, C, *P, *mix, *bag,
                                                  1.0, 1.0, sp()))

    mixok = (p, p, qw, qm, 2, 4, 3)
    assert bwd() == 0 and bwd(bag=bagp) == 0 and bwd(mix=mixok) == 0              # the valid neighbours
    torch.cuda.synchronize()
    for o in outs:
        o.buf.fill_(SENT)
    assert bwd(G=3) == INVALID and bwd(G=0) == INVALID                            # Bn % G != 0
    assert bwd(N=(8, 16)) == INVALID and bwd(N=(5, 32)) == INVALID                # N > P
    assert bwd(N=(5, 13), bag=bagp) == INVALID                                    # ubar off the merged path
    assert bwd(P=(7, 18), bag=bagp) == INVALID
    assert bwd(part=None, nchunk=0, bag=bagp) == INVALID and bwd(d_in=None, bag=bagp) == INVALID
    assert bwd(bag=(p, None, p, p)) == INVALID
    assert bwd(nchunk=2) == INVALID and bwd(nchunk=0) == INVALID                  # merged path
    assert bwd(N=(5, 13), nchunk=2) == INVALID                                    # in_wide + lds: d_in must stay
    assert bwd(Cin=3, C=8, nchunk=3) == INVALID                                   # in_generic + mfma1
    assert bwd(N=(5, 13), nchunk=2, mix=mixok) == INVALID                         # ... and the mix must not run
    assert bwd(Cin=40, C=32, N=(5, 13)) == INVALID                                # C Cin + C > 1024
    assert bwd(mix=(p, None, qw, qm, 2, 4, 3)) == INVALID and bwd(mix=(p, p, None, qm, 2, 4, 3)) == INVALID
    assert bwd(mix=(p, p, qw, None, 2, 4, 3)) == INVALID                          # mnsplit > 1 without mpartial
    assert bwd(mix=(p, p, qw, qm, 0, 4, 3)) == INVALID and bwd(mix=(p, p, qw, qm, 2, 0, 3)) == INVALID
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


def test_lift_bag_ok_agrees_with_the_bag_entries():
    """blindno_lift_bag_ok == (the forward and the adjoint both accept ubar), around every boundary
    of (G, C, N2, P2, Cin); N1 = 5, P1 = 7, Bg = 2."""
    lib, ptr, query, sp = _api()
    src = torch.zeros(1 << 15, device="cuda")
    x0, d_in, part = Guarded(1 << 15), Guarded(1 << 12), Guarded(1 << 12)
    p = ptr(src)
    seen = set()
    for G in (1, 4, 5):
        for C in (4, 5, 16, 17):
            for N2 in (13, 16):
                for P2 in (12, 18, 20):
                    for Cin in (11, 12, 13):
                        Bn, nch = 2 * G, query("blindno_lift_bwd_nchunk", 2, 5, N2)
                        assert Bn * C * 7 * P2 <= x0.n and 2 * 5 * N2 <= d_in.n and nch * G * (C * Cin + C) <= part.n
                        f = lib.blindno_lift_fwd_bag_g(None, p, p, ptr(x0.t), G, 512, Bn, 5, N2, Cin, C, 7, P2, p, p, p, p,
                                                       1.0, sp())
                        b = lib.blindno_lift_bwd_bag_mix_g(p, None, p, ptr(d_in.t), ptr(part.t), nch, G, 512, Bn, 5, N2,
                                                           Cin, C, 7, P2, None, None, None, None, 1, 0, 0, p, p, p, p,
                                                           1.0, 1.0, sp())
                        assert f in (0, INVALID) and b in (0, INVALID)
                        ok = query("blindno_lift_bag_ok", G, Bn, 5, N2, Cin, C, 7, P2)
                        assert ok == int(f == 0 and b == 0), (G, C, N2, P2, Cin, f, b, ok)
                        seen.add(ok)
    assert query("blindno_lift_bag_ok", 2, 3, 5, 16, 12, 12, 7, 20) == 0          # Bn % G != 0
    torch.cuda.synchronize()
    assert seen == {0, 1} and x0.margins_intact() and d_in.margins_intact() and part.margins_intact()


# ================================================================================ 1x1-conv weight gradient
def _conv(c, t, nchunk=None):
    lib, ptr, query, sp = _api()
    G, Bg, C, P = c["G"], c["Bg"], c["C"], c["P"]
    nch = query("blindno_conv_wgrad_nchunk", Bg, *P) if nchunk is None else nchunk
    assert nch == lr.conv_wgrad_nchunk(Bg, P)
    part = _nan(nch * G * (C * C + C))
    dz, x = _dev(t["dz"]), _dev(t["x"])
    if G == 1:
        rc = lib.blindno_conv_wgrad(ptr(dz), ptr(x), ptr(part.view), nch, Bg, C, *P, c["act"], sp())
    else:
        rc = lib.blindno_conv_wgrad_g(ptr(dz), ptr(x), ptr(part.view), nch, G, G * Bg, C, *P, c["act"], sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    assert _intact(part)
    return part, nch


@pytest.mark.parametrize("c", lr.CONV_CASES, ids=lr.conv_id)
def test_conv_wgrad_vs_fp64(c):
    t = lr.conv_inputs(c)
    a = (t["dz"], t["x"], c["act"], c["G"])
    ref, bound = lr.conv_wgrad_g(*a), lr.conv_wgrad_g_bound(*a)
    part, nch = _conv(c, t)
    _ratio(lr.conv_id(c) + " dWc|dbc", _rows(part, nch, c["G"]), ref, bound)
    if c["reduce"]:
        assert nch > 1
        _ratio(lr.conv_id(c) + " dWc|dbc reduce_partials", _reduced(part, nch, ref.size), ref, bound)
    assert torch.equal(part.buf, _conv(c, t)[0].buf), "not bit-reproducible"


def test_conv_wgrad_refusals():
    """C = 32 (C C + C > 1024 parameters per workgroup), a wrong nchunk and Bn % G != 0: partial untouched."""
    lib, ptr, query, sp = _api()
    src = torch.zeros(1 << 15, device="cuda")
    part = Guarded(1 << 15)
    p, q = ptr(src), ptr(part.t)
    nch = query("blindno_conv_wgrad_nchunk", 2, 7, 20)
    assert lib.blindno_conv_wgrad_g(p, p, q, nch, 1, 2, 31, 7, 20, 0, sp()) == 0  # the valid neighbour
    torch.cuda.synchronize()
    part.buf.fill_(SENT)
    for act in (0, 1):
        assert lib.blindno_conv_wgrad_g(p, p, q, nch, 1, 2, 32, 7, 20, act, sp()) == INVALID
        assert lib.blindno_conv_wgrad(p, p, q, nch, 2, 32, 7, 20, act, sp()) == INVALID
    assert lib.blindno_conv_wgrad_g(p, p, q, nch + 1, 1, 2, 12, 7, 20, 0, sp()) == INVALID
    assert lib.blindno_conv_wgrad_g(p, p, q, nch, 2, 3, 12, 7, 20, 0, sp()) == INVALID
    assert lib.blindno_conv_wgrad_g(p, p, q, nch, 0, 2, 12, 7, 20, 0, sp()) == INVALID
    torch.cuda.synchronize()
    assert part.untouched()


# ================================================================================ the nchunk cap
def _ones_like_case(t):
    """Unit operands: every sum is the exact integer point count (< 2^24), whatever the order, so a
    tile that the grid-stride loop skips or visits twice shows as a wrong count."""
    return {k: (None if v is None else np.ones_like(v)) for k, v in t.items()}


@pytest.mark.parametrize("c", [lr.CAP_LIFT_LDS, lr.CAP_LIFT_MFMA], ids=lr.bwd_id)
def test_lift_bwd_w_nchunk_cap(c):
    """More than 1024 tiles: nchunk is capped and the workgroups' tile loops run a second round."""
    t = lr.lift_inputs(c)
    r = _bwd(c, t, False, True, False)
    assert r["nchunk"] == lr.NCHUNK_CAP
    _check_bwd(c, t, r, lr.bwd_id(c))
    assert _same(r, _bwd(c, t, False, True, False)), "not bit-reproducible"
    r1 = _bwd(c, _ones_like_case(t), False, True, False)
    assert np.all(_rows(r1["part"], r1["nchunk"], 1) == c["Bg"] * c["N"][0] * c["N"][1])


def test_conv_wgrad_nchunk_cap():
    c = lr.CAP_CONV
    t = lr.conv_inputs(c)
    a = (t["dz"], t["x"], c["act"], c["G"])
    part, nch = _conv(c, t)
    assert nch == lr.NCHUNK_CAP
    _ratio(lr.conv_id(c) + " dWc|dbc", _rows(part, nch, 1), lr.conv_wgrad_g(*a), lr.conv_wgrad_g_bound(*a))
    assert torch.equal(part.buf, _conv(c, t)[0].buf), "not bit-reproducible"
    p1, _ = _conv(c, _ones_like_case(t))
    assert np.all(_rows(p1, nch, 1) == c["Bg"] * c["P"][0] * c["P"][1])
