"""The gradient finalisation and optimiser kernels called directly: the partial-sum reductions
(csrc/fields.hip), the spectral weight gradient (csrc/wgrad.h), the spectral weight packing and
unpacking (csrc/packw.h, csrc/spectral.hip), the deferred finalisation's bookkeeping
(blindno.ops._Deferred), the fused MSE, rowsq and Adam.

Every reference is float64 on the host, written from the operation's formula; every bound is
derived (stated at its check), not measured.  Outputs live inside sentinel-filled buffers with a
sentinel margin on both sides: each test also asserts that nothing outside the intended range
was written.  Each check prints its worst error / bound ratio.
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SENT = -12345.678        # the sentinel (random data never takes this value)
MARGIN = 64              # sentinel floats on both sides of every output


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _api():
    from blindno import ops
    from blindno._lib import BlindnoError, call, ptr, query, stream_ptr
    return ops, BlindnoError, call, ptr, query, stream_ptr


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """n elements between two sentinel margins, all sentinel-filled."""

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * MARGIN,), SENT, device="cuda", dtype=dtype)
        self.t = self.buf[MARGIN:MARGIN + self.n]

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == SENT).all() and (self.buf[MARGIN + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def cpu(self):
        return self.t.cpu()


def _dev(x):
    """A host tensor (complex: its real view) as a flat float32 device tensor."""
    x = torch.view_as_real(x) if x.is_complex() else x
    return x.to(torch.float32).reshape(-1).contiguous().cuda()


def _cplx(flat, *shape):
    return torch.view_as_complex(flat.cpu().reshape(*shape, 2).contiguous())


def _vp(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[None if t is None else t.data_ptr() for t in ts])


def _ia(vs):
    return (ctypes.c_int * max(1, len(vs)))(*[int(v) for v in vs])


def _worst(err, bound):
    """max err / bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# =========================================================================== 1. reductions
def _partials(nchunk, np_, seed, cancel=False):
    g = _gen(seed)
    p = torch.randn(nchunk, np_, generator=g)
    if cancel and nchunk > 1:
        # heavy cancellation: terms ~1e3 x the result
        p = p * 1e3
        p[-1] = (torch.randn(np_, generator=g).double() - p[:-1].double().sum(0)).float()
    return p


def _reduce_plain(part_dev, nchunk, np_):
    _, _, call, ptr, _, sp = _api()
    out = Guarded(np_)
    call("blindno_reduce_partials", ptr(part_dev), ptr(out.t), nchunk, np_, sp())
    return out


def _reduce_ratio(got, part):
    """|got - ref| <= nchunk 2^-24 sum_c |partial[c][p]| against the fp64 sum of the same fp32
    partials: nchunk - 1 fp32 additions in any order lose at most (nchunk - 1) u of the terms'
    absolute sum (first order), u = 2^-24."""
    pd = part.double()
    ref, bound = pd.sum(0), part.shape[0] * U24 * pd.abs().sum(0)
    return _worst((got.double() - ref).abs().numpy(), bound.numpy())


@pytest.mark.parametrize("np_", [1, 20, 63, 64, 65, 156, 1000])
def test_reduce_partials_vs_fp64(np_):
    PB = min(np_, 64)
    S = 1024 // PB
    worst = 0.0
    cases = [(nc, False) for nc in sorted({1, 3, S - 1, S, S + 1, 4 * S, 4 * S + 1, 5 * S + 3})]
    cases += [(4 * S + 1, True), (5 * S + 3, True)]
    for nchunk, cancel in cases:
        part = _partials(nchunk, np_, 1000 * np_ + nchunk, cancel)
        out = _reduce_plain(part.cuda(), nchunk, np_)
        torch.cuda.synchronize()
        assert out.margins_intact(), (np_, nchunk)
        r = _reduce_ratio(out.cpu(), part)
        worst = max(worst, r)
        assert r <= 1.0, (np_, nchunk, cancel, r)
        if cancel:
            ref = part.double().sum(0)
            assert float(part.abs().max()) > 100 * float(ref.abs().max())
    print(f"reduce_partials np={np_} S={S}: worst err/bound {worst:.3f}")


def _pieces_call(name, parts, outs, ncs, nps, e0s, e1s, extra=()):
    _, _, call, _, _, sp = _api()
    call(name, _vp(parts), _vp(outs), _ia(ncs), _ia(nps), _ia(e0s), _ia(e1s), *extra, len(parts), sp())


@pytest.mark.parametrize("np_,nchunk,pieces", [
    (300, 37, [(0, 7), (7, 64), (64, 65), (65, 130), (130, 300)]),   # (65, 130): the gap flush emits
    (20, 37, [(0, 1), (1, 13), (13, 20)]),                           # one block: e0 / pb = 0
    (20, 3, [(5, 6)]),
])
def test_reduce_partials_pieces_bit_identical(np_, nchunk, pieces):
    part = _partials(nchunk, np_, 77 + np_)
    pd = part.cuda()
    plain = _reduce_plain(pd, nchunk, np_)
    outs = [Guarded(e1 - e0) for e0, e1 in pieces]
    _pieces_call("blindno_reduce_partials_pieces", [pd] * len(pieces), [o.t for o in outs],
                 [nchunk] * len(pieces), [np_] * len(pieces), [p[0] for p in pieces],
                 [p[1] for p in pieces])
    torch.cuda.synchronize()
    ref = plain.cpu()
    assert _reduce_ratio(ref, part) <= 1.0
    for (e0, e1), o in zip(pieces, outs):
        assert o.margins_intact(), (e0, e1)
        assert torch.equal(o.cpu(), ref[e0:e1]), (e0, e1)


_SEG_NPS = [1, 20, 63, 64, 65, 156, 300]
_SEG_NCS = [1, 3, 17, 37, 70]


def _fifty_segments():
    segs = []
    for i in range(50):
        np_, nc = _SEG_NPS[i % 7], _SEG_NCS[i % 5]
        segs.append((nc, np_, _partials(nc, np_, 5000 + i)))
    return segs


def test_reduce_partials_multi_crosses_the_segment_group():
    """50 segments (two launch groups of the 48-segment table), whole (_multi) and with a piece
    in the second group (_pieces): each bit-identical to its own plain launch."""
    _, _, call, _, _, sp = _api()
    segs = _fifty_segments()
    segs[49] = (37, 300, _partials(37, 300, 5049))
    devs = [s[2].cuda() for s in segs]
    plains = [_reduce_plain(d, nc, np_) for d, (nc, np_, _) in zip(devs, segs)]
    outs = [Guarded(np_) for _, np_, _ in segs]
    call("blindno_reduce_partials_multi", _vp(devs), _vp([o.t for o in outs]), _ia([s[0] for s in segs]),
         _ia([s[1] for s in segs]), 50, sp())
    # segment 49 (np = 300 -> 5 blocks) as the piece [70, 140): blocks 1 .. 2 of its grid
    assert segs[49][1] == 300
    e0s, e1s = [0] * 50, [s[1] for s in segs]
    e0s[49], e1s[49] = 70, 140
    outs2 = [Guarded(e1 - e0) for e0, e1 in zip(e0s, e1s)]
    _pieces_call("blindno_reduce_partials_pieces", devs, [o.t for o in outs2], [s[0] for s in segs],
                 [s[1] for s in segs], e0s, e1s)
    torch.cuda.synchronize()
    worst = 0.0
    for i, (nc, np_, part) in enumerate(segs):
        ref = plains[i].cpu()
        worst = max(worst, _reduce_ratio(ref, part))
        assert outs[i].margins_intact() and outs2[i].margins_intact(), i
        assert torch.equal(outs[i].cpu(), ref), i
        assert torch.equal(outs2[i].cpu(), ref[e0s[i]:e1s[i]]), i
    assert worst <= 1.0
    print(f"reduce_partials_multi: worst err/bound {worst:.3f}")


def _unpack_plain(dWt_dev, Ci, Co, m1, m2, P1):
    _, _, call, ptr, _, sp = _api()
    d1, d2 = Guarded(2 * Ci * Co * m1 * m2), Guarded(2 * Ci * Co * m1 * m2)
    call("blindno_unpack_w2d", ptr(dWt_dev), ptr(d1.t), ptr(d2.t), Ci, Co, m1, m2, P1, sp())
    return d1, d2


def test_reduce_partials_pieces_u_descriptors_across_groups():
    """50 segments, 3 of the first launch group and 2 of the second stored unpacked; the
    descriptors are listed in another order than their segments, so descriptor uq (not the
    group-local count) must select the destination."""
    shapes = [(2, 3, 2, 3), (1, 1, 1, 1), (3, 2, 1, 5), (4, 4, 2, 2), (2, 2, 3, 3)]   # (Ci, Co, m1, m2)
    where = {2: 3, 10: 0, 30: 4, 48: 1, 49: 2}                                      # segment -> uq
    segs = _fifty_segments()
    for s, uq in where.items():
        Ci, Co, m1, m2 = shapes[uq]
        np_ = 4 * Ci * Co * m1 * m2
        segs[s] = (segs[s][0], np_, _partials(segs[s][0], np_, 6000 + s))
    devs = [s[2].cuda() for s in segs]
    plains = [_reduce_plain(d, nc, np_) for d, (nc, np_, _) in zip(devs, segs)]
    outs = [Guarded(np_) for _, np_, _ in segs]
    d1s = [Guarded(2 * a * b * c * d) for a, b, c, d in shapes]
    d2s = [Guarded(2 * a * b * c * d) for a, b, c, d in shapes]
    upks = [where.get(i, -1) for i in range(50)]
    ud = [t for a, b in zip(d1s, d2s) for t in (a.t, b.t)]
    ushp = [v for sh in shapes for v in sh]
    _pieces_call("blindno_reduce_partials_pieces_u", devs, [o.t for o in outs], [s[0] for s in segs],
                 [s[1] for s in segs], [0] * 50, [s[1] for s in segs], (_ia(upks), _vp(ud), _ia(ushp)))
    refs = {}
    for s, uq in where.items():
        Ci, Co, m1, m2 = shapes[uq]
        refs[uq] = _unpack_plain(plains[s].t, Ci, Co, m1, m2, 2 * m1 + 3)
    torch.cuda.synchronize()
    for i in range(50):
        if i in where:
            uq = where[i]
            assert outs[i].untouched(), i                 # stored through the descriptor only
            assert d1s[uq].margins_intact() and d2s[uq].margins_intact(), i
            assert torch.equal(d1s[uq].cpu(), refs[uq][0].cpu()), i
            assert torch.equal(d2s[uq].cpu(), refs[uq][1].cpu()), i
            # and against the formula: weights1 rows j < m1, weights2 rows m1 + j of dWt
            Ci, Co, m1, m2 = shapes[uq]
            dWt = _cplx(plains[i].t, m2, 2 * m1, Ci, Co)
            r1, r2 = _unpack_ref(dWt, m1, 2 * m1 + 3)
            assert torch.equal(_cplx(d1s[uq].t, Ci, Co, m1, m2), r1), i
            assert torch.equal(_cplx(d2s[uq].t, Ci, Co, m1, m2), r2), i
        else:
            assert outs[i].margins_intact(), i
            assert torch.equal(outs[i].cpu(), plains[i].cpu()), i


@pytest.mark.parametrize("bad", ["e0>=e1", "e1>np", "unpack on a piece", "shape product != np"])
def test_reduce_partials_pieces_u_rejects(bad):
    _, BlindnoError, _, _, _, _ = _api()
    np_ = 144                                       # 4 * 2 * 3 * 2 * 3
    part = _partials(5, np_, 9).cuda()
    outs = [Guarded(np_), Guarded(np_)]
    d1, d2 = Guarded(np_ // 2), Guarded(np_ // 2)
    e0s, e1s, upks, ushp = [0, 0], [np_, np_], [-1, -1], [2, 3, 2, 3]
    if bad == "e0>=e1":
        e0s[1], e1s[1] = 5, 5
    elif bad == "e1>np":
        e1s[1] = np_ + 1
    elif bad == "unpack on a piece":
        e0s[1], upks[1] = 64, 0
    else:
        upks[1], ushp = 0, [2, 3, 2, 4]
    with pytest.raises(BlindnoError):
        _pieces_call("blindno_reduce_partials_pieces_u", [part, part], [o.t for o in outs], [5, 5],
                     [np_, np_], e0s, e1s, (_ia(upks), _vp([d1.t, d2.t]), _ia(ushp)))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs + [d1, d2])


# =========================================================================== 2. spectral weight gradient
def _mix_inputs(Bn, Ci, Co, K1, m2, seed):
    g = _gen(seed)
    X = torch.complex(torch.randn(Bn, m2, Ci, K1, generator=g), torch.randn(Bn, m2, Ci, K1, generator=g))
    G = torch.complex(torch.randn(Bn, m2, Co, K1, generator=g), torch.randn(Bn, m2, Co, K1, generator=g))
    return X, G


def _mix_ref(X, G, n0=0, n1=None):
    """dWt[k,j,i,o] = sum_n conj(X[n,k,i,j]) G[n,k,o,j] over samples [n0, n1) in complex128, and
    per component the sum of the absolute values of its real products."""
    X, G = X[n0:n1].to(torch.complex128), G[n0:n1].to(torch.complex128)
    ref = torch.einsum("nkij,nkoj->kjio", X.conj(), G)
    e = lambda a, b: torch.einsum("nkij,nkoj->kjio", a.abs(), b.abs())   # noqa: E731
    t_re = e(X.real, G.real) + e(X.imag, G.imag)
    t_im = e(X.real, G.imag) + e(X.imag, G.real)
    return ref, torch.complex(t_re, t_im)


def _f64_ratio(got, ref, terms):
    """nsplit = 1: fp64 accumulation (2 Bn fused multiply-adds, each <= 2^-53 of the running
    absolute sum: 2 Bn 2^-53 <= 2^-45 for Bn <= 128) and one rounding to fp32 (2^-24 |ref|, the
    bound allows 2^-23): per component |got - ref| <= 2^-23 |ref| + 2^-45 sum |terms|."""
    got = got.to(torch.complex128)
    r = 0.0
    for c in ("real", "imag"):
        err = (getattr(got, c) - getattr(ref, c)).abs()
        bound = 2.0 ** -23 * getattr(ref, c).abs() + 2.0 ** -45 * getattr(terms, c)
        r = max(r, _worst(err.numpy(), bound.numpy()))
    return r


def _mix_g(Xd, Gd, nsplit, Gw, Bn, Ci, Co, K1, m2):
    _, _, call, ptr, _, sp = _api()
    tot = 2 * m2 * K1 * Ci * Co
    dWt = Guarded(Gw * tot)
    part = Guarded(nsplit * Gw * tot) if nsplit > 1 else None
    call("blindno_mix_wgrad_g", ptr(Xd), ptr(Gd), ptr(dWt.t), ptr(part.t) if part else None, nsplit, Gw,
         Bn, Ci, Co, K1, m2, sp())
    return dWt, part


def _check_split(dWt, part, X, G, nsplit, Gw, Bn, Ci, Co, K1, m2):
    """The partials of every (slice, group) against their own samples (nsplit = 1 bound; empty
    slices exactly 0), dWt bit-identical to the plain reduction of those partials and within the
    reduction's bound of their fp64 sum; together the bound of the split gradient."""
    tot = 2 * m2 * K1 * Ci * Co
    Bg = Bn // Gw
    ns = -(-Bg // nsplit)
    p = part.cpu().reshape(nsplit, Gw, tot)
    worst = 0.0
    for y in range(nsplit):
        for g in range(Gw):
            n0, n1 = g * Bg + y * ns, min(g * Bg + Bg, g * Bg + (y + 1) * ns)
            got = _cplx(p[y, g], m2, K1, Ci, Co)
            if n0 >= n1:
                assert not p[y, g].any(), (y, g)
                continue
            ref, terms = _mix_ref(X, G, n0, n1)
            r = _f64_ratio(got, ref, terms)
            worst = max(worst, r)
            assert r <= 1.0, (y, g, r)
    flat = p.reshape(nsplit, Gw * tot)
    r = _reduce_ratio(dWt.cpu(), flat)
    assert r <= 1.0, r
    plain = _reduce_plain(part.t, nsplit, Gw * tot)
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu(), dWt.cpu())
    return max(worst, r)


@pytest.mark.parametrize("shape", [(5, 3, 4, 6, 5), (17, 12, 12, 8, 3), (64, 4, 4, 24, 12)])
def test_mix_wgrad_vs_fp64(shape):
    _, _, call, ptr, query, sp = _api()
    Bn, Ci, Co, K1, m2 = shape
    X, G = _mix_inputs(Bn, Ci, Co, K1, m2, sum(shape))
    Xd, Gd = _dev(X), _dev(G)
    ref, terms = _mix_ref(X, G)
    tot = 2 * m2 * K1 * Ci * Co
    for nsplit in sorted({1, 2, 3, 7, query("blindno_mix_wgrad_nsplit", Bn, Ci, Co, K1, m2)}):
        dWt = Guarded(tot)
        part = Guarded(nsplit * tot) if nsplit > 1 else None
        call("blindno_mix_wgrad", ptr(Xd), ptr(Gd), ptr(dWt.t), ptr(part.t) if part else None, nsplit,
             Bn, Ci, Co, K1, m2, sp())
        torch.cuda.synchronize()
        assert dWt.margins_intact() and (part is None or part.margins_intact()), nsplit
        if nsplit == 1:
            r = _f64_ratio(_cplx(dWt.t, m2, K1, Ci, Co), ref, terms)
            assert r <= 1.0, r
        else:
            r = _check_split(dWt, part, X, G, nsplit, 1, Bn, Ci, Co, K1, m2)
            # the split gradient itself: the unsplit bound plus the reduction's bound on the fp32
            # partials (whose factor nsplit, one more than the additions, covers the slices' roundings)
            p64 = part.cpu().double().reshape(nsplit, tot)
            got = _cplx(dWt.t, m2, K1, Ci, Co).to(torch.complex128)
            b = torch.view_as_complex((nsplit * U24 * p64.abs().sum(0)).reshape(m2, K1, Ci, Co, 2).contiguous())
            for c in ("real", "imag"):
                bound = getattr(b, c) + 2.0 ** -23 * getattr(ref, c).abs() + 2.0 ** -45 * getattr(terms, c)
                assert _worst((getattr(got, c) - getattr(ref, c)).abs().numpy(), bound.numpy()) <= 1.0
            # blindno_mix_wgrad_part: the same partials
            part2 = Guarded(nsplit * tot)
            call("blindno_mix_wgrad_part", ptr(Xd), ptr(Gd), ptr(part2.t), nsplit, 1, Bn, Ci, Co, K1, m2, sp())
            torch.cuda.synchronize()
            assert part2.margins_intact() and torch.equal(part2.cpu(), part.cpu()), nsplit
        print(f"mix_wgrad {shape} nsplit={nsplit}: worst err/bound {r:.3f}")


@pytest.mark.parametrize("Bn", [4, 10])
def test_mix_wgrad_groups(Bn):
    """Gw = 2: each weight group sums its own samples only."""
    _, _, call, ptr, _, sp = _api()
    Ci, Co, K1, m2, Gw = 3, 4, 6, 5, 2
    X, G = _mix_inputs(Bn, Ci, Co, K1, m2, 40 + Bn)
    Xd, Gd = _dev(X), _dev(G)
    tot = 2 * m2 * K1 * Ci * Co
    Bg = Bn // Gw
    for nsplit in (1, 2, 3):
        dWt, part = _mix_g(Xd, Gd, nsplit, Gw, Bn, Ci, Co, K1, m2)
        torch.cuda.synchronize()
        assert dWt.margins_intact()
        if nsplit == 1:
            r = 0.0
            for g in range(Gw):
                ref, terms = _mix_ref(X, G, g * Bg, (g + 1) * Bg)
                r = max(r, _f64_ratio(_cplx(dWt.t[g * tot:(g + 1) * tot], m2, K1, Ci, Co), ref, terms))
            assert r <= 1.0, r
        else:
            assert part.margins_intact()
            r = _check_split(dWt, part, X, G, nsplit, Gw, Bn, Ci, Co, K1, m2)
            part2 = Guarded(nsplit * Gw * tot)
            call("blindno_mix_wgrad_part", ptr(Xd), ptr(Gd), ptr(part2.t), nsplit, Gw, Bn, Ci, Co, K1, m2, sp())
            torch.cuda.synchronize()
            assert part2.margins_intact() and torch.equal(part2.cpu(), part.cpu())
        print(f"mix_wgrad_g Bn={Bn} nsplit={nsplit}: worst err/bound {r:.3f}")


# jobs (Bn, Ci, Co, K1, m2, nsplit, Gw)
_MIX_JOBS = [(5, 3, 4, 6, 5, 1, 1), (17, 12, 12, 8, 3, 3, 1), (4, 3, 4, 6, 5, 1, 2), (10, 2, 3, 4, 3, 2, 2),
             (8, 4, 4, 24, 12, 1, 1), (9, 1, 1, 2, 1, 1, 1), (16, 2, 5, 4, 7, 7, 1), (12, 3, 3, 6, 2, 1, 4),
             (6, 5, 2, 2, 9, 2, 1), (7, 2, 2, 4, 4, 1, 1)]


def _own_launch(Xd, Gd, job):
    """The job through its own launch: dWt (nsplit = 1) or the partials."""
    _, _, call, ptr, _, sp = _api()
    Bn, Ci, Co, K1, m2, ns, Gw = job
    tot = 2 * m2 * K1 * Ci * Co
    if ns == 1:
        return _mix_g(Xd, Gd, 1, Gw, Bn, Ci, Co, K1, m2)[0]
    part = Guarded(ns * Gw * tot)
    call("blindno_mix_wgrad_part", ptr(Xd), ptr(Gd), ptr(part.t), ns, Gw, Bn, Ci, Co, K1, m2, sp())
    return part


def test_mix_wgrad_multi_crosses_the_job_group():
    """9 jobs (the job table holds 8): each bit-identical to its own launch."""
    _, _, call, _, _, sp = _api()
    jobs = _MIX_JOBS[:9]
    ins = [_mix_inputs(*j[:5], seed=300 + q) for q, j in enumerate(jobs)]
    Xd, Gd = [_dev(x) for x, _ in ins], [_dev(g) for _, g in ins]
    outs = [Guarded(j[5] * j[6] * 2 * j[4] * j[3] * j[1] * j[2]) for j in jobs]
    call("blindno_mix_wgrad_multi", _vp(Xd), _vp(Gd), _vp([o.t for o in outs]),
         _ia([v for j in jobs for v in j]), len(jobs), sp())
    own = [_own_launch(x, g, j) for x, g, j in zip(Xd, Gd, jobs)]
    torch.cuda.synchronize()
    for q, j in enumerate(jobs):
        assert outs[q].margins_intact(), q
        assert torch.equal(outs[q].cpu(), own[q].cpu()), (q, j)
    # one unsplit job against the formula (the own launches are checked above)
    ref, terms = _mix_ref(*ins[4])
    assert _f64_ratio(_cplx(outs[4].t, 12, 24, 4, 4), ref, terms) <= 1.0


def test_mix_wgrad_multi_u_stores_unpacked():
    """10 jobs, four of them (Gw = 1, 2, 4; one in the second launch group) stored unpacked into
    (dw1, dw2): bit-identical to the mix followed by blindno_unpack_w2d."""
    _, _, call, _, _, sp = _api()
    jobs = _MIX_JOBS
    unp = {0: 1, 2: 2, 7: 4, 9: 1}                             # job -> Gw
    ins = [_mix_inputs(*j[:5], seed=400 + q) for q, j in enumerate(jobs)]
    Xd, Gd = [_dev(x) for x, _ in ins], [_dev(g) for _, g in ins]
    outs = [Guarded(j[5] * j[6] * 2 * j[4] * j[3] * j[1] * j[2]) for j in jobs]
    ud, um1, dst = [None] * (8 * len(jobs)), [0] * len(jobs), {}
    for q, Gw in unp.items():
        Bn, Ci, Co, K1, m2, ns, gw = jobs[q]
        assert (ns, gw) == (1, Gw)
        um1[q] = K1 // 2
        for g in range(Gw):
            dst[q, g] = (Guarded(Ci * Co * K1 * m2), Guarded(Ci * Co * K1 * m2))    # 2 Ci Co m1 m2 floats
            ud[8 * q + 2 * g], ud[8 * q + 2 * g + 1] = dst[q, g][0].t, dst[q, g][1].t
    call("blindno_mix_wgrad_multi_u", _vp(Xd), _vp(Gd), _vp([o.t for o in outs]),
         _ia([v for j in jobs for v in j]), _vp(ud), _ia(um1), len(jobs), sp())
    own = [_own_launch(x, g, j) for x, g, j in zip(Xd, Gd, jobs)]
    refs = {}
    for q, Gw in unp.items():
        Bn, Ci, Co, K1, m2, _, _ = jobs[q]
        tot = 2 * m2 * K1 * Ci * Co
        for g in range(Gw):
            refs[q, g] = _unpack_plain(own[q].t[g * tot:(g + 1) * tot], Ci, Co, K1 // 2, m2, K1 + 1)
    torch.cuda.synchronize()
    for q, j in enumerate(jobs):
        if q not in unp:
            assert outs[q].margins_intact() and torch.equal(outs[q].cpu(), own[q].cpu()), q
            continue
        assert outs[q].untouched(), q
        for g in range(unp[q]):
            for k in (0, 1):
                assert dst[q, g][k].margins_intact(), (q, g, k)
                assert torch.equal(dst[q, g][k].cpu(), refs[q, g][k].cpu()), (q, g, k)


@pytest.mark.parametrize("bad", ["ns != 1", "K1 != 2 um1", "Gw = 5"])
def test_mix_wgrad_multi_u_rejects(bad):
    _, BlindnoError, call, _, _, sp = _api()
    job = {"ns != 1": (10, 2, 3, 4, 3, 2, 1), "K1 != 2 um1": (10, 2, 3, 4, 3, 1, 1),
           "Gw = 5": (10, 2, 3, 4, 3, 1, 5)}[bad]
    um1 = 3 if bad == "K1 != 2 um1" else 2
    X, G = _mix_inputs(*job[:5], seed=5)
    Xd, Gd = _dev(X), _dev(G)
    out = Guarded(job[5] * job[6] * 2 * 3 * 4 * 2 * 3)
    ds = [Guarded(2 * 3 * 4 * 3) for _ in range(8)]
    with pytest.raises(BlindnoError):
        call("blindno_mix_wgrad_multi_u", _vp([Xd]), _vp([Gd]), _vp([out.t]), _ia(job),
             _vp([d.t for d in ds]), _ia([um1]), 1, sp())
    torch.cuda.synchronize()
    assert out.untouched() and all(d.untouched() for d in ds)


# =========================================================================== 3. packing and unpacking
W2D_SHAPES = [(3, 5, 2, 5, 8),       # Ci Co = 15 < 32
              (12, 12, 4, 33, 20),   # ragged k tile
              (4, 4, 16, 12, 40),
              (2, 3, 4, 4, 8),       # 2 m1 == P1
              (2, 3, 5, 4, 8),       # overlapping kept rows
              (2, 2, 3, 3, 3)]       # m1 == P1
TILED = W2D_SHAPES[:3]


def _rows(m1, P1):
    return sorted(set(range(m1)) | set(range(P1 - m1, P1)))


def _pack_ref(w1, w2, P1):
    Ci, Co, m1, m2 = w1.shape
    full = torch.zeros(Ci, Co, P1, m2, dtype=w1.dtype)
    full[:, :, :m1] = w1
    full[:, :, P1 - m1:] = w2                      # weights2 wins on overlap (the assignment order)
    return full[:, :, _rows(m1, P1)].permute(3, 2, 0, 1).contiguous()


def _unpack_ref(dWt, m1, P1):
    """The adjoint of _pack_ref: rows of dw1 that weights2 shadows are exactly 0."""
    m2, K1, Ci, Co = dWt.shape
    gfull = torch.zeros(Ci, Co, P1, m2, dtype=dWt.dtype)
    gfull[:, :, _rows(m1, P1)] = dWt.permute(2, 3, 1, 0)
    dw1, dw2 = gfull[:, :, :m1].clone(), gfull[:, :, P1 - m1:].clone()
    if P1 - m1 < m1:
        dw1[:, :, P1 - m1:] = 0
    return dw1.contiguous(), dw2.contiguous()


def _crand(seed, *shape):
    g = _gen(seed)
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def _w_pair(shape, seed):
    Ci, Co, m1, m2, _ = shape
    return _crand(seed, Ci, Co, m1, m2), _crand(seed + 1, Ci, Co, m1, m2)


def _nK1(shape):
    return len(_rows(shape[2], shape[4]))


@pytest.mark.parametrize("shape", W2D_SHAPES)
def test_pack_w2d_entries(shape):
    ops, _, call, ptr, _, sp = _api()
    Ci, Co, m1, m2, P1 = shape
    K1 = _nK1(shape)
    n = 2 * m2 * K1 * Ci * Co
    (w1, w2), (w1b, w2b) = _w_pair(shape, 10), _w_pair(shape, 20)
    ref, refb = _pack_ref(w1, w2, P1), _pack_ref(w1b, w2b, P1)
    d = [_dev(t) for t in (w1, w2, w1b, w2b)]
    a = Guarded(n)
    call("blindno_pack_w2d", ptr(d[0]), ptr(d[1]), ptr(a.t), Ci, Co, m1, m2, P1, sp())
    b = Guarded(2 * n)
    call("blindno_pack_w2d_2", ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(b.t), Ci, Co, m1, m2, P1, sp())
    c = [Guarded(n), Guarded(n)]
    call("blindno_pack_w2d_multi", _vp([d[0], d[2]]), _vp([d[1], d[3]]), _vp([c[0].t, c[1].t]),
         _ia(list(shape) * 2), 2, sp())
    pairs = [(d[0].view(Ci, Co, m1, m2, 2), d[1].view(Ci, Co, m1, m2, 2)),
             (d[2].view(Ci, Co, m1, m2, 2), d[3].view(Ci, Co, m1, m2, 2))]
    many = ops.pack_w2d_many(pairs, P1)
    one = ops.k_pack_w2d(*pairs[0], P1)
    torch.cuda.synchronize()
    assert all(g.margins_intact() for g in [a, b] + c)
    assert torch.equal(_cplx(a.t, m2, K1, Ci, Co), ref)
    assert torch.equal(_cplx(b.t, 2, m2, K1, Ci, Co), torch.stack([ref, refb]))
    assert torch.equal(_cplx(c[0].t, m2, K1, Ci, Co), ref) and torch.equal(_cplx(c[1].t, m2, K1, Ci, Co), refb)
    assert many[0].shape == (m2, K1, Ci, Co, 2) and one.shape == (m2, K1, Ci, Co, 2)
    assert torch.equal(torch.view_as_complex(many[0].cpu()), ref)
    assert torch.equal(torch.view_as_complex(many[1].cpu()), refb)
    assert torch.equal(torch.view_as_complex(one.cpu()), ref)


@pytest.mark.parametrize("shape", W2D_SHAPES)
def test_unpack_w2d_entries(shape):
    _, _, call, ptr, _, sp = _api()
    Ci, Co, m1, m2, P1 = shape
    K1 = _nK1(shape)
    nw = 2 * Ci * Co * m1 * m2
    dWt, dWtb = _crand(30, m2, K1, Ci, Co), _crand(31, m2, K1, Ci, Co)
    (r1, r2), (r1b, r2b) = _unpack_ref(dWt, m1, P1), _unpack_ref(dWtb, m1, P1)
    if P1 - m1 < m1:
        assert not r1[:, :, P1 - m1:].any() and r1.shape[2] == m1
    both = _dev(torch.stack([dWt, dWtb]))
    da, db = both[:both.numel() // 2], both[both.numel() // 2:]
    a = _unpack_plain(da, Ci, Co, m1, m2, P1)
    b = [Guarded(nw) for _ in range(4)]
    call("blindno_unpack_w2d_2", ptr(both), *[ptr(g.t) for g in b], Ci, Co, m1, m2, P1, sp())
    c = [Guarded(nw) for _ in range(4)]
    call("blindno_unpack_w2d_multi", _vp([da, db]), _vp([c[0].t, c[2].t]), _vp([c[1].t, c[3].t]),
         _ia(list(shape) * 2), 2, sp())
    torch.cuda.synchronize()
    assert all(g.margins_intact() for g in list(a) + b + c)
    cp = lambda g: _cplx(g.t, Ci, Co, m1, m2)    # noqa: E731
    assert torch.equal(cp(a[0]), r1) and torch.equal(cp(a[1]), r2)
    for got in (b, c):
        assert torch.equal(cp(got[0]), r1) and torch.equal(cp(got[1]), r2)
        assert torch.equal(cp(got[2]), r1b) and torch.equal(cp(got[3]), r2b)


@pytest.mark.parametrize("overlap", [False, True])
def test_pack_unpack_w2d_multi_crosses_the_segment_group(overlap):
    """18 segments (the table holds 16): all tiled, or with an overlapping segment in the first
    group (that group then takes the element-wise kernel, the second stays tiled)."""
    _, _, call, _, _, sp = _api()
    shapes = [TILED[i % 3] for i in range(18)]
    if overlap:
        shapes[3] = W2D_SHAPES[4]
    ws = [_w_pair(s, 100 + 2 * i) for i, s in enumerate(shapes)]
    w1d, w2d = [_dev(w[0]) for w in ws], [_dev(w[1]) for w in ws]
    Wts = [Guarded(2 * s[3] * _nK1(s) * s[0] * s[1]) for s in shapes]
    flat = [v for s in shapes for v in s]
    call("blindno_pack_w2d_multi", _vp(w1d), _vp(w2d), _vp([W.t for W in Wts]), _ia(flat), 18, sp())
    dWs = [_crand(200 + i, s[3], _nK1(s), s[0], s[1]) for i, s in enumerate(shapes)]
    dWd = [_dev(x) for x in dWs]
    d1 = [Guarded(2 * s[0] * s[1] * s[2] * s[3]) for s in shapes]
    d2 = [Guarded(2 * s[0] * s[1] * s[2] * s[3]) for s in shapes]
    call("blindno_unpack_w2d_multi", _vp(dWd), _vp([g.t for g in d1]), _vp([g.t for g in d2]), _ia(flat), 18, sp())
    torch.cuda.synchronize()
    for i, (Ci, Co, m1, m2, P1) in enumerate(shapes):
        K1 = _nK1(shapes[i])
        assert Wts[i].margins_intact() and d1[i].margins_intact() and d2[i].margins_intact(), i
        assert torch.equal(_cplx(Wts[i].t, m2, K1, Ci, Co), _pack_ref(*ws[i], P1)), i
        r1, r2 = _unpack_ref(dWs[i], m1, P1)
        assert torch.equal(_cplx(d1[i].t, Ci, Co, m1, m2), r1), i
        assert torch.equal(_cplx(d2[i].t, Ci, Co, m1, m2), r2), i


@pytest.mark.parametrize("Ci,Co,m", [(3, 4, 5), (12, 12, 15)])
def test_pack_w1d_both_directions(Ci, Co, m):
    """(Ci, Co, m) complex <-> (m, Ci, Co) complex; the round trip is exact."""
    ops, _, call, ptr, _, sp = _api()
    w = _crand(50 + m, Ci, Co, m)
    wd = _dev(w)
    Wt, back = Guarded(2 * Ci * Co * m), Guarded(2 * Ci * Co * m)
    call("blindno_pack_w1d", ptr(wd), ptr(Wt.t), Ci, Co, m, 0, sp())
    call("blindno_pack_w1d", ptr(Wt.t), ptr(back.t), Ci, Co, m, 1, sp())
    kw = ops.k_pack_w1d(torch.view_as_complex(wd.view(Ci, Co, m, 2)))
    torch.cuda.synchronize()
    assert Wt.margins_intact() and back.margins_intact()
    assert torch.equal(_cplx(Wt.t, m, Ci, Co), w.permute(2, 0, 1).contiguous())
    assert torch.equal(back.cpu(), wd.cpu())
    assert kw.shape == (m, 1, Ci, Co, 2)
    assert torch.equal(torch.view_as_complex(kw.cpu()).reshape(m, Ci, Co), w.permute(2, 0, 1).contiguous())
    # the unpack direction on its own data
    dW = _crand(60 + m, m, Ci, Co)
    dw = Guarded(2 * Ci * Co * m)
    call("blindno_pack_w1d", ptr(_dev(dW)), ptr(dw.t), Ci, Co, m, 1, sp())
    torch.cuda.synchronize()
    assert dw.margins_intact() and torch.equal(_cplx(dw.t, Ci, Co, m), dW.permute(1, 2, 0).contiguous())


@pytest.mark.parametrize("case", ["one launch", "one launch, ragged teams", "17 unpacks", "overlap"])
def test_finish_multi_matches_separate_launches(case):
    """blindno_finish_multi: (a) the one-launch path with an unpack of 2 tiles (two of a
    workgroup's four teams idle), also with 6 tiles over two workgroups and a reduction stored
    unpacked; (b) 17 unpacks and (c) an overlapping unpack: the two-launch fallback."""
    _, _, call, _, _, sp = _api()
    ushapes = {"one launch": [(1, 1, 1, 1, 4)],
               "one launch, ragged teams": [(1, 1, 1, 1, 4), (3, 5, 2, 5, 8)],
               "17 unpacks": [TILED[i % 2] if i else (1, 1, 1, 1, 4) for i in range(17)],
               "overlap": [W2D_SHAPES[4]]}[case]
    reds = [(37, 300), (3, 20), (70, 144)]                      # (nchunk, np)
    parts = [_partials(nc, np_, 700 + i) for i, (nc, np_) in enumerate(reds)]
    pd = [p.cuda() for p in parts]
    plains = [_reduce_plain(d, nc, np_) for d, (nc, np_) in zip(pd, reds)]
    outs = [Guarded(np_) for _, np_ in reds]
    upks, ud, ushp, fold = [-1, -1, -1], [None, None], [1, 1, 1, 1], None
    if case == "one launch, ragged teams":                      # reduction 2 (np = 144) stored unpacked
        fold = (Guarded(72), Guarded(72))
        upks, ud, ushp = [-1, -1, 0], [fold[0].t, fold[1].t], [2, 3, 2, 3]
    dWs = [_crand(800 + i, s[3], _nK1(s), s[0], s[1]) for i, s in enumerate(ushapes)]
    dWd = [_dev(x) for x in dWs]
    d1 = [Guarded(2 * s[0] * s[1] * s[2] * s[3]) for s in ushapes]
    d2 = [Guarded(2 * s[0] * s[1] * s[2] * s[3]) for s in ushapes]
    call("blindno_finish_multi", _vp(pd), _vp([o.t for o in outs]), _ia([r[0] for r in reds]),
         _ia([r[1] for r in reds]), _ia([0, 0, 0]), _ia([r[1] for r in reds]), _ia(upks), _vp(ud), _ia(ushp),
         3, _vp(dWd), _vp([g.t for g in d1]), _vp([g.t for g in d2]), _ia([v for s in ushapes for v in s]),
         len(ushapes), sp())
    sep = [_unpack_plain(x, *s) for x, s in zip(dWd, ushapes)]
    foldref = _unpack_plain(plains[2].t, 2, 3, 2, 3, 7) if fold else None
    torch.cuda.synchronize()
    for i, part in enumerate(parts):
        if fold and i == 2:
            assert outs[i].untouched()
            for k in (0, 1):
                assert fold[k].margins_intact() and torch.equal(fold[k].cpu(), foldref[k].cpu())
            continue
        assert outs[i].margins_intact(), i
        assert torch.equal(outs[i].cpu(), plains[i].cpu()), i
        assert _reduce_ratio(outs[i].cpu(), part) <= 1.0
    for i, (Ci, Co, m1, m2, P1) in enumerate(ushapes):
        assert d1[i].margins_intact() and d2[i].margins_intact(), i
        assert torch.equal(d1[i].cpu(), sep[i][0].cpu()) and torch.equal(d2[i].cpu(), sep[i][1].cpu()), i
        r1, r2 = _unpack_ref(dWs[i], m1, P1)
        assert torch.equal(_cplx(d1[i].t, Ci, Co, m1, m2), r1), i
        assert torch.equal(_cplx(d2[i].t, Ci, Co, m1, m2), r2), i


# =========================================================================== 4. _Deferred bookkeeping
def _spec_job(Bn, Ci, Co, m1, m2, P1, seed):
    X, G = _mix_inputs(Bn, Ci, Co, 2 * m1, m2, seed)
    like = torch.empty(Ci, Co, m1, m2, 2, device="cuda")
    return dict(X=X, G=G, Xd=_dev(X), Gd=_dev(G), like=like, sh=(Bn, Ci, Co, 2 * m1, m2), P1=P1, m1=m1)


def _spec_grad(ops, j):
    dWt = ops.k_mix_wgrad(j["Xd"], j["Gd"], *j["sh"], deferrable=True)
    return ops.unpack_w2d(dWt, j["like"], j["P1"])


def _spec_check(j, d1, d2, split):
    """(dw1, dw2) against the unpack formula of the fp64 gradient.  Unsplit: the fp64 bound of
    section 2.  Split (ns slices): each slice's partial within that bound of its own sum, then
    ns fp32 additions: |err| <= 2^-23 T + 2^-45 T + ns 2^-24 (1 + 2^-22) T with T the sum of the
    terms' absolute values (every slice's |partial| and |ref| are below its terms' sum)."""
    ref, terms = _mix_ref(j["X"], j["G"])
    Bn, Ci, Co, K1, m2 = j["sh"]
    r1, r2 = _unpack_ref(ref, j["m1"], j["P1"])
    t1, t2 = _unpack_ref(terms, j["m1"], j["P1"])
    worst = 0.0
    for got, r, t in ((d1, r1, t1), (d2, r2, t2)):
        got = torch.view_as_complex(got.cpu().contiguous()).to(torch.complex128)
        for c in ("real", "imag"):
            T = getattr(t, c)
            bound = 2.0 ** -23 * (T if split else getattr(r, c).abs()) + 2.0 ** -45 * T
            if split:
                bound = bound + split * U24 * (1 + 2.0 ** -22) * T
            worst = max(worst, _worst((getattr(got, c) - getattr(r, c)).abs().numpy(), bound.numpy()))
    assert worst <= 1.0, worst
    return worst


def _deferred_scenario(ops, deferred, fold, redirect, monkeypatch):
    """Jobs A (unsplit mix + unpack), B (split mix + unpack), C (an unpack of a tensor no
    recorded kernel writes), E (a plain reduction, slices of it redirected).  Returns the results
    and, deferred, the guarded redirect targets."""
    monkeypatch.setattr(ops, "UNPACK_FOLD", fold)
    A = _spec_job(5, 3, 4, 3, 5, 8, 900)
    B = _spec_job(17, 2, 3, 2, 3, 7, 901)
    assert ops.query("blindno_mix_wgrad_nsplit", *A["sh"]) == 1
    nsB = ops.query("blindno_mix_wgrad_nsplit", *B["sh"])
    assert nsB > 1
    dWtC = _crand(902, 4, 4, 2, 3)                       # (m2, K1, Ci, Co), m1 = 2, P1 = 9
    dWtCd = _dev(dWtC).view(4, 4, 2, 3, 2)
    likeC = torch.empty(2, 3, 2, 4, 2, device="cuda")
    partE = _partials(37, 300, 903)
    partEd = partE.cuda()
    res, flat = {}, None

    def record():
        res["A"] = _spec_grad(ops, A)
        res["B"] = _spec_grad(ops, B)
        res["C"] = ops.unpack_w2d(dWtCd, likeC, 9)
        res["E"] = ops.reduce_partials(partEd, 37, 300)

    if not deferred:
        record()
    else:
        with ops.deferred_reductions() as d:
            record()
            assert len(d.mix) == 2 and len(d.red) == 2 and len(d.unp) == 3
            if redirect:
                res["E"].fill_(SENT)
                flat = Guarded(700)
                E = res["E"]
                params = [types.SimpleNamespace(grad=E[7:64].view(19, 3)),      # a slice of a reduction
                          types.SimpleNamespace(grad=E[130:201]),               # not adjacent, offsets
                          types.SimpleNamespace(grad=res["A"][0]),              # an unpack output
                          types.SimpleNamespace(grad=res["C"][1])]
                offs = [3, 101, 200, 600]
                pairs = [(p, flat.t[o:o + p.grad.numel()]) for p, o in zip(params, offs)]
                done = d.redirect(pairs)
                assert len(done) == 4
                for p, (_, dst) in zip(params, pairs):
                    assert p.grad.data_ptr() == dst.data_ptr()
                res["redir"] = (params, offs)
            mixu, redu, rest = d._fold_unpacks()
            if fold:
                # A's unpack rides its unsplit mix job, B's the reduction of its partials, C's is
                # left for the finish launch
                assert list(mixu) == [0] and list(redu) == [0] and len(rest) == 1
                assert rest[0][0].data_ptr() == dWtCd.data_ptr()
            else:
                assert not mixu and not redu and len(rest) == 3
    torch.cuda.synchronize()
    res["jobs"] = (A, B, nsB, dWtC, partE)
    return res, flat


@pytest.mark.parametrize("fold", [True, False])
def test_deferred_matches_immediate(fold, monkeypatch):
    ops = _api()[0]
    eager, _ = _deferred_scenario(ops, False, fold, False, monkeypatch)
    A, B, nsB, dWtC, partE = eager["jobs"]
    # the immediate results against the formulas
    ra = _spec_check(A, *eager["A"], 0)
    rb = _spec_check(B, *eager["B"], nsB)
    r1, r2 = _unpack_ref(dWtC, 2, 9)
    assert torch.equal(torch.view_as_complex(eager["C"][0].cpu()), r1)
    assert torch.equal(torch.view_as_complex(eager["C"][1].cpu()), r2)
    re = _reduce_ratio(eager["E"].cpu(), partE)
    assert re <= 1.0
    print(f"deferred fold={fold}: worst err/bound unsplit {ra:.3f}, split {rb:.3f}, reduction {re:.3f}")
    for redirect in (False, True):
        got, flat = _deferred_scenario(ops, True, fold, redirect, monkeypatch)
        for k in ("A", "B", "C"):
            for i in (0, 1):
                if redirect and (k, i) in (("A", 0), ("C", 1)):
                    continue
                assert torch.equal(got[k][i], eager[k][i]), (k, i, redirect)
        E, Eref = got["E"].cpu(), eager["E"].cpu()
        if not redirect:
            assert torch.equal(E, Eref)
            continue
        assert flat.margins_intact()
        f = flat.cpu()
        params, offs = got["redir"]
        # the redirected slices landed in the flat buffer, the gaps in the original one
        assert torch.equal(f[3:3 + 57], Eref[7:64]) and torch.equal(f[101:101 + 71], Eref[130:201])
        assert torch.equal(E[0:7], Eref[0:7]) and torch.equal(E[64:130], Eref[64:130])
        assert torch.equal(E[201:300], Eref[201:300])
        assert bool((E[7:64] == SENT).all()) and bool((E[130:201] == SENT).all())
        assert torch.equal(f[200:200 + 360], eager["A"][0].reshape(-1).cpu())
        assert torch.equal(f[600:600 + 96], eager["C"][1].reshape(-1).cpu())
        used = torch.zeros(700, dtype=torch.bool)
        for p, o in zip(params, offs):
            used[o:o + p.grad.numel()] = True
        assert bool((f[~used] == SENT).all())


@pytest.mark.parametrize("fold", [True, False])
def test_deferred_unpack_reading_a_reduction_is_ordered(fold, monkeypatch):
    """Unpacks of the slices dWt[g] of one grouped reduction's output (the heads' layout):
    _unpacks_read_reductions is true and the reductions run before the unpacks."""
    ops = _api()[0]
    monkeypatch.setattr(ops, "UNPACK_FOLD", fold)
    Ci, Co, m1, m2, P1, Gw, nc = 3, 2, 2, 5, 9, 2, 19
    tot = 2 * m2 * 2 * m1 * Ci * Co
    part = _partials(nc, Gw * tot, 950)
    pd = part.cuda()
    like = torch.empty(Ci, Co, m1, m2, 2, device="cuda")

    def record():
        dWt = ops.reduce_partials(pd, nc, Gw * tot).view(Gw, m2, 2 * m1, Ci, Co, 2)
        return dWt, [ops.unpack_w2d(dWt[g], like, P1) for g in range(Gw)]

    dWt0, eager = record()
    with ops.deferred_reductions() as d:
        dWt1, got = record()
        mixu, redu, rest = d._fold_unpacks()
        assert not mixu and not redu and len(rest) == Gw
        assert d._unpacks_read_reductions(rest)
    torch.cuda.synchronize()
    assert torch.equal(dWt1, dWt0)
    assert _reduce_ratio(dWt0.reshape(-1).cpu(), part) <= 1.0
    for g in range(Gw):
        r1, r2 = _unpack_ref(torch.view_as_complex(dWt0[g].cpu()), m1, P1)
        assert torch.equal(got[g][0], eager[g][0]) and torch.equal(got[g][1], eager[g][1]), g
        assert torch.equal(torch.view_as_complex(got[g][0].cpu()), r1), g
        assert torch.equal(torch.view_as_complex(got[g][1].cpu()), r2), g


@pytest.mark.parametrize("fold", [True, False])
def test_deferred_nine_split_spectral_gradients(fold, monkeypatch):
    """Nine split spectral weight gradients, each with its unpack, in one context: one launch
    group of the reductions stores at most blindno_reduce_segs_limit(1) = 8 of them unpacked, so
    the flush folds eight and leaves the ninth to the unpack launch.  Bit-identical to the
    unfolded and to the immediate results."""
    ops = _api()[0]
    monkeypatch.setattr(ops, "UNPACK_FOLD", fold)
    assert ops.query("blindno_reduce_segs_limit", 0) == 48 and ops.query("blindno_reduce_segs_limit", 1) == 8
    shapes = [(17, 2, 3, 2, 3, 7), (24, 3, 3, 1, 4, 5), (17, 1, 2, 3, 2, 8)]    # Bn Ci Co m1 m2 P1
    jobs = [_spec_job(*shapes[i % 3], seed=960 + i) for i in range(9)]
    for j in jobs:
        assert ops.query("blindno_mix_wgrad_nsplit", *j["sh"]) > 1
    eager = [_spec_grad(ops, j) for j in jobs]
    with ops.deferred_reductions() as d:
        got = [_spec_grad(ops, j) for j in jobs]
        mixu, redu, rest = d._fold_unpacks()
        assert not mixu
        assert (len(redu), len(rest)) == ((8, 1) if fold else (0, 9))
    torch.cuda.synchronize()
    worst = 0.0
    for i, j in enumerate(jobs):
        assert torch.equal(got[i][0], eager[i][0]) and torch.equal(got[i][1], eager[i][1]), i
        worst = max(worst, _spec_check(j, *got[i], ops.query("blindno_mix_wgrad_nsplit", *j["sh"])))
    print(f"nine split gradients fold={fold}: worst err/bound {worst:.3f}")


# =========================================================================== 5. loss, metric, Adam
def _adam64(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    step_size = lr / (1 - b1 ** t)
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
    return p - step_size * m / denom, m, v


def _adam_refs(p0, grads, lrs):
    """(p, m, v) after the steps in float64, and by torch.optim.Adam in fp32 on the CPU."""
    p, m, v = p0.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double()
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=lrs[0], foreach=False)
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        p, m, v = _adam64(p, m, v, g.double(), t, lr)
        opt.param_groups[0]["lr"] = lr
        q.grad = g.clone()
        opt.step()
    st = opt.state[q]
    return (p, m, v), (q.detach(), st["exp_avg"], st["exp_avg_sq"])


def _adam_bar(tag, got, ref64, ref32):
    for name, a, r, c in zip("pmv", got, ref64, ref32):
        e_gpu, e_ref = rel_l2(a.numpy(), r.numpy()), rel_l2(c.numpy(), r.numpy())
        print(f"adam {tag} {name}: GPU rel-L2 {e_gpu:.2e}, CPU fp32 torch.optim.Adam {e_ref:.2e}")
        assert e_gpu <= max(2 * e_ref, 1e-6), (tag, name, e_gpu, e_ref)


LRS = [5e-4, 5e-4, 5e-4, 2.5e-4, 2.5e-4]           # one StepLR change between the steps


@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("n", [1, 255, 257, 16384 * 256 + 3])
def test_adam_kernel_five_steps(n, gscale):
    _, _, call, ptr, _, sp = _api()
    g = _gen(n % 1000 + int(gscale * 8))
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 + k) for k in range(5)]
    P, M, V, Gb = Guarded(n), Guarded(n), Guarded(n), Guarded(n)
    P.t.copy_(p0)
    M.t.zero_()
    V.t.zero_()
    b1, b2 = 0.9, 0.999
    for t, (gr, lr) in enumerate(zip(grads, LRS), 1):
        Gb.t.copy_(gr)
        # as FlatAdam.step computes them
        step_size = lr / (1.0 - b1 ** t)
        bc2s = math.sqrt(1.0 - b2 ** t)
        call("blindno_adam", ptr(P.t), ptr(Gb.t), ptr(M.t), ptr(V.t), n, b1, b2, 1e-8, step_size, bc2s,
             gscale, sp())
    torch.cuda.synchronize()
    assert all(x.margins_intact() for x in (P, M, V, Gb))
    assert torch.equal(Gb.cpu(), grads[-1])
    ref64, ref32 = _adam_refs(p0, [gr * gscale for gr in grads], LRS)      # 0.25 g is exact in fp32
    _adam_bar(f"n={n} gscale={gscale}", (P.cpu(), M.cpu(), V.cpu()), ref64, ref32)


@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_flat_adam_three_parameters(gscale):
    from blindno.train import FlatAdam
    g = _gen(31)
    sizes = [(1,), (2049,), (50, 100)]
    p0 = [torch.randn(*s, generator=g) for s in sizes]
    grads = [[torch.randn(*s, generator=g) * (0.1 + k) for s in sizes] for k in range(5)]
    params = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
    opt = FlatAdam(params, lr=LRS[0])
    assert opt.n == 1 + 2049 + 5000
    for gr, lr in zip(grads, LRS):
        opt.lr = lr                                   # what StepLR.step sets
        for p, x in zip(params, gr):
            p.grad = x.cuda()
        opt.step(grad_scale=gscale)
    torch.cuda.synchronize()
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])    # noqa: E731
    ref64, ref32 = _adam_refs(cat(p0), [cat(gr) * gscale for gr in grads], LRS)
    got = cat([p.detach().cpu() for p in params])
    assert torch.equal(got, opt.flat.cpu())
    _adam_bar(f"FlatAdam gscale={gscale}", (got, opt.m.cpu(), opt.v.cpu()), ref64, ref32)


def _mse_cases():
    from blindno.ops import _mse_blocks
    ns = [1, 255, 257, 1025, 5000, 300001]
    cases = {(n, 1) for n in ns[:4]} | {(n, _mse_blocks(n)) for n in ns} | {(1025, 4)}
    return sorted(cases)


def test_mse_fused_matches_two_launches_and_fp64():
    """blindno_mse_fwd (partials + finish in one launch, on one completion counter) three times
    in a row against blindno_mse + blindno_mse_finish and float64.  n = 256 nblk + 1 at the nblk
    ops._mse_blocks gives is n = 257 only; 1025 (nblk = 2, 4), 5000 and 300001 (293 workgroups:
    the finish's strided loop) add the multi-workgroup geometries.
    Bound (the terms are non-negative): |got - ref| <= depth 2^-24 ref with depth =
    ceil(n / (256 nblk)) + ceil(nblk / 256) + 18: the per-thread chains of the two stages, two
    8-level trees, the division and the difference's rounding."""
    _, _, call, ptr, _, sp = _api()
    worst = 0.0
    for n, nblk in _mse_cases():
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        acc = Guarded(1)
        acc.t.zero_()
        losses, counters, run = [], [], np.float32(0.0)
        for k in range(3):
            g = _gen(7 * n + k)
            p, t = torch.randn(n, generator=g), torch.randn(n, generator=g) * (k + 1)
            pd, td = p.cuda(), t.cuda()
            part, loss, grad = Guarded(nblk), Guarded(1), Guarded(n)
            call("blindno_mse_fwd", ptr(pd), ptr(td), ptr(part.t), n, nblk, ptr(loss.t), ptr(acc.t),
                 ptr(counter), ptr(grad.t), sp())
            counters.append(counter.clone())
            part2, loss2, grad2 = Guarded(nblk), Guarded(1), Guarded(n)
            call("blindno_mse", ptr(pd), ptr(td), ptr(part2.t), ptr(grad2.t), n, nblk, None, sp())
            call("blindno_mse_finish", ptr(part2.t), nblk, n, ptr(loss2.t), sp())
            one = torch.ones(1, device="cuda")
            part3, grad3 = Guarded(nblk), Guarded(n)
            call("blindno_mse", ptr(pd), ptr(td), ptr(part3.t), ptr(grad3.t), n, nblk, ptr(one), sp())
            losses.append((p, t, part, loss, grad, part2, loss2, grad2, grad3))
        torch.cuda.synchronize()
        for k, (p, t, part, loss, grad, part2, loss2, grad2, grad3) in enumerate(losses):
            assert all(x.margins_intact() for x in (part, loss, grad, part2, loss2, grad2, grad3)), (n, nblk, k)
            assert int(counters[k]) == 0, (n, nblk, k)
            assert torch.equal(loss.cpu(), loss2.cpu()) and torch.equal(part.cpu(), part2.cpu()), (n, nblk, k)
            assert torch.equal(grad.cpu(), grad2.cpu()) and torch.equal(grad.cpu(), grad3.cpu()), (n, nblk, k)
            d = p.double() - t.double()
            ref = float((d * d).sum() / n)
            depth = -(-n // (256 * nblk)) + -(-nblk // 256) + 18
            r = abs(float(loss.cpu()) - ref) / (depth * U24 * ref)
            worst = max(worst, r)
            assert r <= 1.0, (n, nblk, k, r)
            # the gradient 2 (p - t) / n: three fp32 roundings, (1 + u)^3 - 1 < 4 u
            gerr = (grad.cpu().double() - 2 * d / n).abs()
            assert bool((gerr <= 4 * U24 * (2 * d / n).abs()).all()), (n, nblk, k)
            run = np.float32(run + np.float32(float(loss.cpu())))
        assert acc.margins_intact() and float(acc.cpu()) == float(run), (n, nblk)
    print(f"mse fused: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("den_all", [0, 1])
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("rows", [1, 3])
def test_rowsq_vs_fp64(rows, n, stride, den_all):
    """fp64 accumulation of exact fp64 products of fp32 data: relative error <= n stride 2^-52."""
    ops = _api()[0]
    off_a, off_b = (0, 0) if stride == 1 else ((1, stride - 1) if stride == 3 else (1, 1))
    g = _gen(rows * 1000 + n * 10 + stride)
    a, b = torch.randn(rows, n, stride, generator=g), torch.randn(rows, n, stride, generator=g)
    out = ops.rowsq(a.cuda(), b.cuda(), rows, n, stride, off_a, off_b, den_all)
    torch.cuda.synchronize()
    assert out.shape == (rows, 2) and out.dtype == torch.float64
    ad, bd = a.double(), b.double()
    num = ((ad[:, :, off_a] - bd[:, :, off_b]) ** 2).sum(1)
    den = (bd ** 2).sum((1, 2)) if den_all else (bd[:, :, off_b] ** 2).sum(1)
    ref = torch.stack([num, den], 1)
    r = _worst((out.cpu() - ref).abs().numpy(), (n * stride * 2.0 ** -52 * ref).numpy())
    assert r <= 1.0, r
    print(f"rowsq rows={rows} n={n} stride={stride} den_all={den_all}: worst err/bound {r:.3f}")
