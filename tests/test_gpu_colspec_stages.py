"""The folded column pass (csrc/colspec.h, csrc/colspec.hip, the ZY / CD modes of rowfuse_kernel
behind the *_zc entries of csrc/rowinv.hip) and the lift entries around it, called through the C
ABI one stage at a time against the float64 references of tests/colspec_stage_ref.py -- on every
launch path the host code selects (DESIGN.md "Folded column pass launch paths" tabulates the
predicates; each case names the instantiation it reaches and the predicate values that send it
there, worked out from rowdft_cd_launch, blindno_colmix_u, rowinv_launch, zc_w3 and zc_blocks).

The bound is test_gpu_spectral_stages.py's, per element and derived:
|got - ref| <= (n + c) 2^-24 S_abs (+ 5e-7 x the GELU weight where GELU / GELU' is evaluated), n
the accumulated terms along the chain observed, c = 8 (that file's single roundings: two twiddle
tables, the scale, the result, two for FMA / summation order) + 1 for each further table whose
entries are rounded once on the chain: Tab (ZY) and TabT (CD) of ops.twiddle_colspec.  The links:

  row DFT                    P2 terms
  column DFT partials        16 nbv: 16 rows per block, the Re / Im combination, the block sum
  lift (4 terms)             4
  mix                        C
  ZY (Z from Y)              K1 = 24
  row inverse + epilogue     2 m2 + C + 1 (bias / the GELU' product)
  reduced gradient rows      + the number of summed elements

Two terms beyond the issue's list, both for the next spectrum taken in the same pass (CD of f(z)
or dx), whose reference is the spectrum of the float64 field: (1) the field's own error reaches
the spectrum through f, so S_abs = L sum_{h,w} S_abs(field) with L = 1, or L = 1.13 >= max |GELU'|
= 1.1290 when f = GELU (mean value theorem), and n counts the field's chain too; (2) the field's
GELU weight is carried the same way, plus one GELU evaluation per point when f = GELU.

part is opaque (colspec.h): it is observed through blindno_colmix with Wt = NULL.  Outputs and
scratch are NaN-filled between sentinel margins; every case runs twice and must repeat bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import colspec_stage_ref as cr
import spectral_stage_ref as sr
from colspec_stage_ref import GELU_LIP, K1
from spectral_stage_ref import GELU_ABS, U24, Guarded, worst

pytestmark = pytest.mark.gpu

C_EXTRA = 8              # c of test_gpu_spectral_stages.py
INVALID = 1              # hipErrorInvalidValue
M1 = M2 = 12
C4 = 4
IDX = [4, 0, 2, 0]       # unsorted, a repeat, 0 and T - 1
B, T = 2, 5
GEOMS = [pytest.param((32, 32), id="P32x32"), pytest.param((48, 32), id="P48x32"),
         pytest.param((32, 64), id="P32x64")]
CROP = {(32, 32): (23, 28), (48, 32): (37, 28), (32, 64): (23, 52)}     # whole float4s


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


@pytest.fixture()
def fuse():
    """blindno_set_rowfuse for the test, the previous setting restored after."""
    from blindno._lib import query
    prev = query("blindno_set_rowfuse", 1)
    yield query
    query("blindno_set_rowfuse", prev)


def _api():
    from blindno import ops
    from blindno._lib import call, ptr, query, stream_ptr
    return ops, call, ptr, query, stream_ptr


def _rc(name, *args):
    from blindno._lib import load
    return int(getattr(load(), name)(*args))


class NanGuarded(Guarded):
    """Guarded with a NaN interior: an element the kernel leaves unwritten stays NaN."""

    def __init__(self, n):
        super().__init__(n)
        self.t.fill_(float("nan"))

    def untouched(self):
        return self.margins_intact() and bool(torch.isnan(self.t).all())

    def np(self, *shape):
        return self.t.cpu().numpy().reshape(shape)


def _twice(launch):
    """Run a case twice on fresh buffers: guards intact, results bit-identical."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is None:
            continue
        assert x.margins_intact() and y.margins_intact()
        assert torch.equal(x.t.view(torch.int32), y.t.view(torch.int32))
    return a


def _randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _crandn(rng, *shape, scale=1.0):
    return _randn(rng, *shape, scale=scale).astype(np.float64) + 1j * _randn(rng, *shape, scale=scale).astype(np.float64)


def _dev(a, dtype=np.float32):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = sr.ri(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1)).cuda()


def _nan_outside(a, crop):
    a = a.copy()
    if crop is not None:
        a[..., crop[0]:, :] = np.nan
        a[..., :, crop[1]:] = np.nan
    return a


def _ratio(label, got, ref, S, n, gw=None, c=C_EXTRA):
    bound = (n + c) * U24 * np.asarray(S, np.float64)
    if gw is not None:
        bound = bound + GELU_ABS * np.asarray(gw, np.float64)
    bound = np.broadcast_to(bound, np.shape(ref))
    got = np.asarray(got)
    assert np.isfinite(got.view(np.float64) if np.iscomplexobj(got) else got).all(), label
    if np.iscomplexobj(ref):
        d = got - ref
        r = max(worst(np.abs(d.real), bound), worst(np.abs(d.imag), bound))
    else:
        r = worst(np.abs(got.astype(np.float64) - ref), bound)
    print(f"{label}: worst err/bound {r:.3g}")
    assert r <= 1.0, (label, r)
    return r


class Tables:
    def __init__(self, P1, P2, m2=M2):
        ops = _api()[0]
        self.tab = ops.twiddle_colspec(P1, M1, "cuda")
        self.Tp = ops.twiddle_mfma(P2, m2, "cuda")
        self.tb = ops.twiddle_rowinv(P2, m2, "cuda")


def _psize(Bn, P1, Cp, m2):
    return Bn * (P1 // 16) * _api()[3]("blindno_colspec_nchunk", Cp, m2) * 128


def _spec_of(part, nbv, Bn, C, P1, P2, m2=M2):
    """The spectrum a partial buffer holds: blindno_colmix with Wt = NULL (Xsave only)."""
    _, call, ptr, _, sp = _api()
    Xs = NanGuarded(Bn * m2 * C * K1 * 2)
    call("blindno_colmix", ptr(part.t), nbv, None, ptr(Xs.t), None, Bn, C, C, P1, P2, M1, m2, 0, None, None, None, sp())
    return Xs


def _cx(g, *shape):
    return sr.cplx(g.np(*shape, 2))


def _dg2(grid, P1, P2):
    """Dg2 (m2, 3, K1) of the reference, rounded to fp32 (an input of the kernels under test)."""
    d = cr.spectrum(cr.grid_planes(grid, P1, P2), M2)[0]
    return d.real.astype(np.float32).astype(np.float64) + 1j * d.imag.astype(np.float32).astype(np.float64)


def test_nchunk_and_ok_follow_the_layout():
    """blindno_colspec_nchunk against colspec.h's chunk count; blindno_colspec_ok's geometry rule."""
    q = _api()[3]
    for C in (1, 3, 4):
        for m2 in (4, 8, 12, 16):
            nnt, half = (2 * m2 + 15) // 16, 1 if (2 * m2) % 16 == 8 else 0
            assert q("blindno_colspec_nchunk", C, m2) == (C * (nnt - half) + half * ((C + 1) // 2)) * 3
    assert q("blindno_colspec_nchunk", 4, 12) == 18 and q("blindno_colspec_nchunk", 1, 12) == 6
    for P1, P2 in ((32, 32), (48, 32), (32, 64)):
        assert q("blindno_colspec_ok", 3, 4, P1, P2, 12, 12) == 1
    for bad in ((3, 3, 32, 32, 12, 12), (3, 4, 32, 32, 12, 8), (3, 4, 32, 32, 8, 12), (3, 4, 16, 32, 12, 12),
                (3, 4, 40, 32, 12, 12), (3, 4, 32, 40, 12, 12)):
        assert q("blindno_colspec_ok", *bad) == 0


# ================================================================================ rowdft_cd
# (Bn, C, P1, P2, m2), valid region, input offset in floats.  rowdft_cd_kernel<NNT, ALIGNED, LIFT 0>
CD_CASES = [
    # NNT 2 (m2 12), aligned (N2v % 4 == 0, P2 % 4 == 0, base 16-B): 16 items over 4 workgroups
    pytest.param((2, 4, 32, 32, 12), (32, 32), 0, id="nnt2_aligned"),
    # NNT 1 (m2 8), aligned, C 3 (the _grid_spec2 use)
    pytest.param((2, 3, 32, 32, 8), (32, 32), 0, id="nnt1_aligned_c3"),
    # NNT 2, not aligned: N2v 29; N1v 37 of 48 -> nbv 3 = P1 / 16, rows 37..47 zero
    pytest.param((2, 4, 48, 32, 12), (37, 29), 0, id="nnt2_n2v29"),
    # NNT 2, not aligned: the base pointer 4 bytes past 16-B alignment at N2v % 4 == 0
    pytest.param((2, 4, 32, 64, 12), (32, 64), 1, id="nnt2_base_offset"),
    # NNT 1, not aligned, C 3, a partial last K block (N2v 29 of 64)
    pytest.param((2, 3, 32, 64, 8), (20, 29), 0, id="nnt1_n2v29_c3"),
    # N1v 10 -> nbv 1 < P1 / 16 = 2: block 1 is not written, colmix(nbv 1) does not read it
    pytest.param((2, 4, 32, 32, 12), (10, 32), 0, id="nbv1_of_2"),
    # Bn 1, C 3, nbv 1: 3 items < the 4 waves of the one workgroup; C 3 with the half tile
    pytest.param((1, 3, 32, 32, 12), (16, 32), 0, id="fewer_items_than_waves"),
    # 513 * 4 * 2 = 4104 items > 4 * COLSPEC_RD_BLOCKS = 4096: waves 0..7 take a second item
    pytest.param((513, 4, 32, 32, 12), (32, 32), 0, id="persistent_second_item"),
]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom,valid,off", CD_CASES)
def test_rowdft_cd_vs_fp64(geom, valid, off, act):
    """X = spectrum of f(x) on the valid region.  n = P2 (row DFT) + 16 nbv (column partials and
    their block sum); c = 8 + 1 (TabT)."""
    _, call, ptr, _, sp = _api()
    Bn, C, P1, P2, m2 = geom
    rng = np.random.default_rng(100 + sum(geom) + act)
    x = _randn(rng, Bn, C, P1, P2)
    buf = torch.zeros(x.size + 4, device="cuda")
    xt = buf[off:off + x.size]
    xt.copy_(torch.from_numpy(_nan_outside(x, valid).reshape(-1)))
    assert xt.data_ptr() % 16 == 4 * off
    tb = Tables(P1, P2, m2)
    nb, nbv = P1 // 16, (valid[0] + 15) // 16

    def launch():
        part = NanGuarded(_psize(Bn, P1, C, m2))
        call("blindno_rowdft_cd", ptr(xt), ptr(part.t), ptr(tb.Tp), ptr(tb.tab), Bn, C, P1, P2, m2, act, valid[0],
             valid[1], sp())
        return part, _spec_of(part, nbv, Bn, C, P1, P2, m2)

    part, Xs = _twice(launch)
    assert np.isnan(part.np(Bn, nb, -1)[:, nbv:]).all()              # blocks past the valid rows: unwritten
    S, cnt = cr.spectrum_abs(x, m2, act, valid)
    _ratio(f"rowdft_cd {geom} valid={valid} off={off} act={act}", _cx(Xs, Bn, m2, C, K1),
           cr.spectrum(x, m2, act, valid), S, P2 + 16 * nbv, cnt if act else None, C_EXTRA + 1)


def test_rowdft_cd_bag_vs_fp64_nonsquare():
    """blindno_rowdft_cd_bag (rowdft_cd_kernel<2, aligned, LIFT 0, BDZ 1>) at P1 48, P2 32, crop
    37 x 28: the spectrum of dz = lw_l ghat v.  n = P2 + 16 nbv + 2 (the two products forming dz);
    c = 9."""
    _, call, ptr, _, sp = _api()
    U, P1, P2, (Ho, Wo) = 3, 48, 32, (37, 28)
    Bn = B * U
    rng = np.random.default_rng(7)
    v, ghat = _randn(rng, Bn, C4, P1, P2), _randn(rng, B, Ho, Wo)
    lw = (np.array([2.0, 1.0, 5.0]) / 8.0).astype(np.float32)
    tb = Tables(P1, P2)
    vd, gd, ld = _dev(_nan_outside(v, (Ho, Wo))), _dev(ghat), _dev(lw)
    for lwd, lwn in ((ld, lw.astype(np.float64)), (None, np.full(U, 1.0 / U))):
        def launch():
            part = NanGuarded(_psize(Bn, P1, C4, M2))
            call("blindno_rowdft_cd_bag", ptr(vd), ptr(gd), ptr(lwd), U, ptr(part.t), ptr(tb.Tp), ptr(tb.tab), Bn, C4,
                 P1, P2, M2, Ho, Wo, sp())
            return part, _spec_of(part, 3, Bn, C4, P1, P2)

        _, Xs = _twice(launch)
        dz = np.zeros((Bn, C4, P1, P2))
        sc = np.float32(1.0 / U) if lwd is None else None
        w = np.tile(lwn, B) if sc is None else np.full(Bn, float(sc))
        dz[:, :, :Ho, :Wo] = (w[:, None, None] * np.repeat(ghat.astype(np.float64), U, 0))[:, None] * v[:, :, :Ho, :Wo]
        S, _ = cr.spectrum_abs(dz, M2)
        _ratio(f"rowdft_cd_bag lw={'given' if lwd is not None else 'NULL'}", _cx(Xs, Bn, M2, C4, K1),
               cr.spectrum(dz, M2), S, P2 + 16 * 3 + 2, None, C_EXTRA + 1)


# ================================================================================ bag lift + colmix (lift)
# (P1, P2, N1, N2).  rowdft_cd_kernel<2, ALIGNED, LIFT 1>
LIFT_CASES = [
    pytest.param((32, 32, 23, 28), id="aligned"),                  # N2 % 4 == 0
    pytest.param((48, 32, 37, 29), id="unaligned_n2_29"),          # N2 % 4 != 0 -> scalar reads
    pytest.param((32, 64, 16, 52), id="n1_16_nbv1"),               # N1 <= 16: nbv 1 of 2
    pytest.param((32, 32, 32, 32), id="n1_eq_p1"),
]


def _lift_inputs(rng, N1, N2, C):
    X = _randn(rng, B, T, N1, N2)
    grid = _randn(rng, N1, N2, 2)
    return X, grid, _randn(rng, C, 3, scale=0.6), _randn(rng, C, scale=0.6)


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("geom", LIFT_CASES)
def test_bag_lift_cd_and_lift_colmix_vs_fp64(geom, C):
    """blindno_rowdft_bag_lift_cd + colmix_kernel<0, LIFT> (w0 != NULL, Cp 1): Usave (n = P2 +
    16 nbv, c = 9), the lifted spectrum Xsave (+ 4 lift terms) and Y (+ C); with and without
    Usave, with and without Wt, Xsave NULL -- the common outputs bit-identical."""
    _, call, ptr, _, sp = _api()
    P1, P2, N1, N2 = geom
    L, Bn = len(IDX), B * len(IDX)
    rng = np.random.default_rng(200 + sum(geom) + C)
    X, grid, w0, b0 = _lift_inputs(rng, N1, N2, C)
    Wt = _crandn(rng, M2, K1, C, C, scale=0.5)
    Dg2 = _dg2(grid, P1, P2)
    tb = Tables(P1, P2)
    Xd, idx, w0d, b0d, Dd, Wd = _dev(X), _dev(IDX, np.int32), _dev(w0), _dev(b0), _dev(Dg2), _dev(Wt)
    nbv = (N1 + 15) // 16

    def launch():
        part = NanGuarded(_psize(Bn, P1, 1, M2))
        call("blindno_rowdft_bag_lift_cd", ptr(Xd), ptr(idx), ptr(part.t), ptr(tb.Tp), ptr(tb.tab), B, T, L, N1, N2, P1,
             P2, M2, sp())
        n = Bn * M2 * C * K1 * 2
        Xa, Ya, Xb, Yb, Ub, Xc, Uc, Ye = (NanGuarded(n), NanGuarded(n), NanGuarded(n), NanGuarded(n),
                                          NanGuarded(n // C), NanGuarded(n), NanGuarded(n // C), NanGuarded(n))
        tail = (Bn, C, 1, P1, P2, M1, M2, 0, ptr(w0d), ptr(b0d), ptr(Dd))
        call("blindno_colmix", ptr(part.t), nbv, ptr(Wd), ptr(Xa.t), ptr(Ya.t), *tail, sp())
        call("blindno_colmix_u", ptr(part.t), nbv, ptr(Wd), ptr(Xb.t), ptr(Yb.t), *tail, ptr(Ub.t), sp())
        call("blindno_colmix_u", ptr(part.t), nbv, None, ptr(Xc.t), None, *tail, ptr(Uc.t), sp())
        call("blindno_colmix", ptr(part.t), nbv, ptr(Wd), None, ptr(Ye.t), *tail, sp())
        return part, Xa, Ya, Xb, Yb, Ub, Xc, Uc, Ye

    part, Xa, Ya, Xb, Yb, Ub, Xc, Uc, Ye = _twice(launch)
    eq = lambda p, q: torch.equal(p.t.view(torch.int32), q.t.view(torch.int32))
    assert eq(Xa, Xb) and eq(Xa, Xc) and eq(Ya, Yb) and eq(Ya, Ye) and eq(Ub, Uc)
    assert np.isnan(part.np(Bn, P1 // 16, -1)[:, nbv:]).all()
    u = cr.bag_fields(X, IDX, P1, P2)
    U = cr.spectrum(u, M2)[:, :, 0]
    SU, _ = cr.spectrum_abs(u, M2)
    label = f"bag_lift_cd {geom} C={C}"
    n = P2 + 16 * nbv
    _ratio(label + " Usave", _cx(Ub, Bn, M2, K1), U, SU.reshape(Bn, 1, 1), n, None, C_EXTRA + 1)
    Xr, Sx = cr.lift_spectrum(U, Dg2, w0, b0), cr.lift_spectrum_abs(SU, Dg2, w0, b0)
    _ratio(label + " Xsave", _cx(Xa, Bn, M2, C, K1), Xr, Sx, n + 4, None, C_EXTRA + 1)
    _ratio(label + " Y", _cx(Ya, Bn, M2, C, K1), cr.mix(Xr, Wt, P1, P2, 0)[1], cr.mix_abs(Sx, Wt, P1, P2, 0)[1],
           n + 4 + C, None, C_EXTRA + 1)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# hosted: npk <= kPackSegs = 16 and every segment 2 m1 < P1 (w2d_tiled_segs) -> rowdft_cd_pack_kernel;
# fallback: one segment with 2 m1 >= P1 -> blindno_pack_w2d_multi + rowdft_cd_kernel, two launches
@pytest.mark.parametrize("shapes,hosted", [
    pytest.param([(4, 4, 12, 12, 32), (4, 4, 12, 12, 32)], True, id="hosted"),
    pytest.param([(4, 4, 12, 12, 32), (2, 3, 4, 5, 8)], False, id="fallback_overlapping_rows"),
    pytest.param([(2, 2, 2, 3, 8)] * 17, False, id="fallback_17_segments"),
])
def test_bag_lift_cd_pack_bit_identical(shapes, hosted):
    """blindno_rowdft_bag_lift_cd_pack: part and every packed Wts bit-identical to the separate
    blindno_rowdft_bag_lift_cd and blindno_pack_w2d_multi launches; Wts also equal to the
    reference pack order (a copy: exact)."""
    _, call, ptr, _, sp = _api()
    P1, P2, N1, N2 = 32, 32, 23, 28
    L, Bn = len(IDX), B * len(IDX)
    assert hosted == (len(shapes) <= 16 and all(2 * s[2] < s[4] for s in shapes))
    rng = np.random.default_rng(11)
    X = _randn(rng, B, T, N1, N2)
    tb = Tables(P1, P2)
    Xd, idx = _dev(X), _dev(IDX, np.int32)
    ws = [(_crandn(rng, ci, co, m1, m2), _crandn(rng, ci, co, m1, m2)) for ci, co, m1, m2, _ in shapes]
    w1d, w2d = [_dev(a) for a, _ in ws], [_dev(b) for _, b in ws]
    shp = (ctypes.c_int * (5 * len(shapes)))(*[v for s in shapes for v in s])
    nel = [m2 * min(2 * m1, p1) * ci * co * 2 for ci, co, m1, m2, p1 in shapes]

    def launch(fused):
        part = NanGuarded(_psize(Bn, P1, 1, M2))
        Wts = [NanGuarded(n) for n in nel]
        wp = _ptrs([w.t for w in Wts])
        head = (ptr(Xd), ptr(idx), ptr(part.t), ptr(tb.Tp), ptr(tb.tab), B, T, L, N1, N2, P1, P2, M2)
        if fused:
            call("blindno_rowdft_bag_lift_cd_pack", *head, _ptrs(w1d), _ptrs(w2d), wp, shp, len(shapes), sp())
        else:
            call("blindno_rowdft_bag_lift_cd", *head, sp())
            call("blindno_pack_w2d_multi", _ptrs(w1d), _ptrs(w2d), wp, shp, len(shapes), sp())
        return [part] + Wts

    a = _twice(lambda: launch(True))
    b = _twice(lambda: launch(False))
    for x, y in zip(a, b):
        assert torch.equal(x.t.view(torch.int32), y.t.view(torch.int32))
    for (w1, w2), s, g in zip(ws, shapes, a[1:]):
        ref = sr.pack_w2d(w1, w2, s[4])
        assert np.array_equal(sr.cplx(g.np(*ref.shape, 2)), ref)


# ================================================================================ colmix
@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("N1v", [37, 20], ids=["nbv3_of_3", "nbv2_of_3"])
def test_colmix_vs_fp64(N1v, C):
    """colmix_kernel<0, false> (dir 0) and <1, false> (dir 1) at P1 48, P2 32 from rowdft_cd's
    partials: Xsave (dir 0: X, n = P2 + 16 nbv; dir 1: G, the scale is among the c roundings) and
    Y (n + C); c = 9.  Xsave == NULL with Wt given is admitted: Y bit-identical."""
    _, call, ptr, _, sp = _api()
    Bn, P1, P2 = 2, 48, 32
    nbv = (N1v + 15) // 16
    rng = np.random.default_rng(300 + N1v + C)
    x = _randn(rng, Bn, C, P1, P2)
    Wt = _crandn(rng, M2, K1, C, C, scale=0.5)
    tb = Tables(P1, P2)
    xd, Wd = _dev(_nan_outside(x, (N1v, P2))), _dev(Wt)
    part = NanGuarded(_psize(Bn, P1, C, M2))
    call("blindno_rowdft_cd", ptr(xd), ptr(part.t), ptr(tb.Tp), ptr(tb.tab), Bn, C, P1, P2, M2, 0, N1v, P2, sp())
    Xr = cr.spectrum(x, M2, 0, (N1v, P2))
    Sx = np.broadcast_to(cr.spectrum_abs(x, M2, 0, (N1v, P2))[0], Xr.shape)
    n = P2 + 16 * nbv
    for direction in (0, 1):
        def launch():
            Xs, Y, Y2 = (NanGuarded(Bn * M2 * C * K1 * 2) for _ in range(3))
            tail = (Bn, C, C, P1, P2, M1, M2, direction, None, None, None, sp())
            call("blindno_colmix", ptr(part.t), nbv, ptr(Wd), ptr(Xs.t), ptr(Y.t), *tail)
            call("blindno_colmix", ptr(part.t), nbv, ptr(Wd), None, ptr(Y2.t), *tail)
            return Xs, Y, Y2

        Xs, Y, Y2 = _twice(launch)
        assert torch.equal(Y.t.view(torch.int32), Y2.t.view(torch.int32))
        (Xref, Yref), (Xa, Ya) = cr.mix(Xr, Wt, P1, P2, direction), cr.mix_abs(Sx, Wt, P1, P2, direction)
        label = f"colmix N1v={N1v} C={C} dir={direction}"
        _ratio(label + " Xsave", _cx(Xs, Bn, M2, C, K1), Xref, Xa, n, None, C_EXTRA + 1)
        _ratio(label + " Y", _cx(Y, Bn, M2, C, K1), Yref, Ya, n + C, None, C_EXTRA + 1)
    assert part.margins_intact()


def test_colmix_refusals_write_nothing():
    """Host-side argument checks of blindno_colmix(_u): hipErrorInvalidValue, nothing launched."""
    _, _, ptr, _, sp = _api()
    src = torch.zeros(1 << 16, device="cuda")
    p = ptr(src)
    o = [NanGuarded(1 << 14) for _ in range(3)]
    Xs, Y, Us = (ptr(g.t) for g in o)

    def mix(nbv=2, C=4, Cp=4, P1=32, m1=12, m2=12, direction=0, w0=None, usave=None, Wt=p, xs=Xs, y=Y):
        return _rc("blindno_colmix_u", p, nbv, Wt, xs, y, 2, C, Cp, P1, 32, m1, m2, direction, w0, w0, w0, usave, sp())

    assert mix(usave=Us) == INVALID                                  # Usave without lift
    assert mix(Cp=1, w0=p, direction=1) == INVALID                   # lift with dir 1
    assert mix(Cp=4, w0=p) == INVALID                                # lift with Cp != 1
    assert mix(Cp=3) == INVALID                                      # Cp != C
    assert mix(m1=8) == INVALID                                      # m1 != 12
    assert mix(nbv=0) == INVALID and mix(nbv=3) == INVALID           # nbv outside 1 .. P1 / 16
    assert mix(P1=24) == INVALID and mix(P1=40) == INVALID           # K1 != 24 / P1 % 16
    assert mix(m2=17) == INVALID and mix(C=17, Cp=17) == INVALID
    assert mix(y=None) == INVALID and mix(Wt=None, xs=None) == INVALID
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o)


# ================================================================================ epi_zc
def _layer_inputs(rng, Bn, P1, P2):
    Y = _crandn(rng, Bn, M2, C4, K1, scale=0.1)
    x = _randn(rng, Bn, C4, P1, P2)
    wc, bc = _randn(rng, C4, C4, scale=0.4), _randn(rng, C4, scale=0.4)
    return Y, x, wc, bc


N_Z = K1 + 2 * M2 + C4 + 1      # ZY + row inverse + conv + bias / GELU' product


def _next_spec_check(label, part, field_ref, S_field, gw_field, act_next, Bn, P1, P2, n_field):
    """The CD partials of f(field) against the spectrum of f(field_ref) (module docstring):
    n = the field's chain + P2 + 16 nb, c = 8 + 2 (Tab, TabT), S_abs = L sum S_abs(field)."""
    nb = P1 // 16
    Xs = _spec_of(part, nb, Bn, C4, P1, P2)
    torch.cuda.synchronize()
    assert Xs.margins_intact()
    lip = GELU_LIP if act_next else 1.0
    S = lip * S_field.sum((2, 3))[:, None, :, None]
    gw = lip * gw_field.sum((2, 3))[:, None, :, None] + (P1 * P2 if act_next else 0)
    return _ratio(label, _cx(Xs, Bn, M2, C4, K1), cr.spectrum(field_ref, M2, act_next), S, n_field + P2 + 16 * nb,
                  gw, C_EXTRA + 2)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom", GEOMS)
def test_rowidft_epi_zc_vs_fp64(geom, act):
    """rowinv_launch<0, act, 0, 0, ZC>: items = Bn ceil(rows / 16) <= 2600 -> zc_w3, the 3-wave
    kernels rowfuse_kernel<0, act, 0, 0, RD, 6, NH, true, 0, ZY, CD, 3>: part NULL -> RD 0 (ZY only;
    full field, and the crop 23 x 28: whole row blocks and 32-column steps past it skipped);
    part given -> RD 1 (act_next 0) / RD 2 (act_next 1) with CD.
    z: n = K1 + 2 m2 + C + 1, c = 8 + 1 (Tab)."""
    _, call, ptr, _, sp = _api()
    P1, P2 = geom
    Bn = 3
    rng = np.random.default_rng(400 + P1 + 2 * P2 + act)
    Y, x, wc, bc = _layer_inputs(rng, Bn, P1, P2)
    tb = Tables(P1, P2)
    Yd, xd, wd, bd = _dev(Y), _dev(x), _dev(wc), _dev(bc)
    Z, Za = cr.z_from_y(Y, P1), cr.z_from_y_abs(Y, P1)
    ref = sr.row_inv(Z, P2, x, wc.astype(np.float64), bc.astype(np.float64), act)
    S, gw = sr.row_inv_abs(Za, P2, x, wc.astype(np.float64), bc.astype(np.float64), act)
    for crop, with_part, act_next in ((None, False, 0), ((23, 28), False, 0), (None, True, 0), (None, True, 1)):
        oN1, oN2 = crop or (P1, P2)

        def launch():
            z = NanGuarded(Bn * C4 * P1 * P2)
            part = NanGuarded(_psize(Bn, P1, C4, M2)) if with_part else None
            call("blindno_rowidft_epi_zc", ptr(Yd), ptr(xd), ptr(wd), ptr(bd), ptr(z.t), ptr(tb.tb), ptr(tb.tab),
                 ptr(part.t) if with_part else None, ptr(tb.Tp) if with_part else None, Bn, C4, P1, P2, M1, M2, act,
                 act_next, oN1, oN2, sp())
            return z, part

        z, part = _twice(launch)
        label = f"epi_zc {geom} act={act} crop={crop} part={with_part} act_next={act_next}"
        sl = (slice(None), slice(None), slice(0, oN1), slice(0, oN2))
        _ratio(label + " z", z.np(Bn, C4, P1, P2)[sl], ref[sl], S[sl], N_Z, gw[sl], C_EXTRA + 1)
        if with_part:
            _next_spec_check(label + " next spectrum", part, ref, S, gw, act_next, Bn, P1, P2, N_Z)


# ================================================================================ epi_lift_zc
@pytest.mark.parametrize("geom", GEOMS)
def test_rowidft_epi_lift_zc_vs_fp64(geom):
    """rowinv_launch<0, 0, 0, LIFT 1, ZC> (zc_w3: items = 8 P1 / 16 <= 2600; N2 % 4 == 0): part NULL
    -> RD 0; part given -> RD 1 / 2 with CD.  z with x = x0 = pad(fc0(u, gx, gy)):
    n = K1 + 2 m2 + C + 1 + 4 (x0's terms), c = 9.  N2 % 4 != 0: rowinv_launch's float4 gate
    (bl.N2 % 4) fails and the ZC form has no general kernel behind it -> hipErrorInvalidValue,
    nothing written."""
    _, call, ptr, _, sp = _api()
    P1, P2 = geom
    N1, N2 = CROP[geom]
    L, Bn = len(IDX), B * len(IDX)
    rng = np.random.default_rng(500 + P1 + 2 * P2)
    Y, _, wc, bc = _layer_inputs(rng, Bn, P1, P2)
    X, grid, w0, b0 = _lift_inputs(rng, N1, N2, C4)
    tb = Tables(P1, P2)
    Yd, wd, bd, Xd, gd, w0d, b0d, idx = (_dev(Y), _dev(wc), _dev(bc), _dev(X), _dev(grid), _dev(w0), _dev(b0),
                                         _dev(IDX, np.int32))
    Z, Za = cr.z_from_y(Y, P1), cr.z_from_y_abs(Y, P1)
    x0, x0a = cr.lift_field(X, IDX, grid, w0, b0, P1, P2), cr.lift_field_abs(X, IDX, grid, w0, b0, P1, P2)
    ref = sr.row_inv(Z, P2, x0, wc.astype(np.float64), bc.astype(np.float64), 0)
    S, gw = sr.row_inv_abs(Za, P2, x0a, wc.astype(np.float64), bc.astype(np.float64), 0)
    for with_part, act_next in ((False, 0), (True, 0), (True, 1)):
        def launch():
            z = NanGuarded(Bn * C4 * P1 * P2)
            part = NanGuarded(_psize(Bn, P1, C4, M2)) if with_part else None
            call("blindno_rowidft_epi_lift_zc", ptr(Yd), ptr(Xd), ptr(idx), ptr(gd), ptr(w0d), ptr(b0d), ptr(wd),
                 ptr(bd), ptr(z.t), ptr(tb.tb), ptr(tb.tab), ptr(part.t) if with_part else None,
                 ptr(tb.Tp) if with_part else None, B, T, L, N1, N2, C4, P1, P2, M1, M2, act_next, sp())
            return z, part

        z, part = _twice(launch)
        label = f"epi_lift_zc {geom} part={with_part} act_next={act_next}"
        _ratio(label + " z", z.np(Bn, C4, P1, P2), ref, S, N_Z + 4, gw, C_EXTRA + 1)
        if with_part:
            _next_spec_check(label + " next spectrum", part, ref, S, gw, act_next, Bn, P1, P2, N_Z + 4)
    # N2 = 29: refused on the host
    X29, g29 = _dev(_randn(rng, B, T, N1, 29)), _dev(_randn(rng, N1, 29, 2))
    z, part = NanGuarded(Bn * C4 * P1 * P2), NanGuarded(_psize(Bn, P1, C4, M2))
    for pp, tp in ((None, None), (ptr(part.t), ptr(tb.Tp))):
        assert _rc("blindno_rowidft_epi_lift_zc", ptr(Yd), ptr(X29), ptr(idx), ptr(g29), ptr(w0d), ptr(b0d), ptr(wd),
                   ptr(bd), ptr(z.t), ptr(tb.tb), ptr(tb.tab), pp, tp, B, T, L, N1, 29, C4, P1, P2, M1, M2, 0,
                   sp()) == INVALID
    torch.cuda.synchronize()
    assert z.untouched() and part.untouched()


# ================================================================================ bwd_zc
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom", GEOMS)
def test_rowidft_bwd_zc_vs_fp64(geom, act):
    """rowinv_launch<1, act, WG, 0, ZC> on zc_blocks1 (the 2-wave budget only):
    rowfuse_kernel<1, act, WG, 0, RD, 6, 1, true, 0, ZY, CD>: partial NULL / given -> WG 0 / 1;
    part NULL / given -> RD 0 / RD 1 + CD; dz full and cropped (whole float4s).
    dx: n = K1 + 2 m2 + C + 1, c = 9.  dWc | dbc reduced over the partial rows: one product per
    point of the crop summed per lane, wave, workgroup and row: n = Bn dN1 dN2, c = 8.  The CD
    spectrum of dx: _next_spec_check."""
    _, call, ptr, query, sp = _api()
    P1, P2 = geom
    Bn = 3
    rng = np.random.default_rng(600 + P1 + 2 * P2 + act)
    Y, xs, wc, _ = _layer_inputs(rng, Bn, P1, P2)
    dz = _randn(rng, Bn, C4, P1, P2)
    tb = Tables(P1, P2)
    Yd, xd, wd = _dev(Y), _dev(xs), _dev(wc)
    Z, Za = cr.z_from_y(Y, P1), cr.z_from_y_abs(Y, P1)
    bare, bare_abs = sr.row_inv_bare(Z, P2), sr.row_inv_bare_abs(Za, P2)
    nchunk = query("blindno_colspec_bwd_nchunk", Bn, P1)
    assert nchunk == (Bn * (P1 // 16) + 3) // 4                        # zc_blocks1 below the 512 cap
    wc64 = wc.astype(np.float64)
    for crop in (None, CROP[geom]):
        dN1, dN2 = crop or (P1, P2)
        dzd = _dev(_nan_outside(dz, crop))
        ref = sr.row_inv_adj(Z, P2, dz, wc64, xs, act, crop, bare=bare)
        S, gw = sr.row_inv_adj_abs(Za, P2, dz, wc64, xs, act, crop, bare=bare_abs)
        gref, (Sw, gww) = sr.conv_wgrad(dz, xs, act, crop), sr.conv_wgrad_abs(dz, xs, act, crop)
        for with_partial in (False, True):
            for with_part in (False, True):
                def launch():
                    dx = NanGuarded(Bn * C4 * P1 * P2)
                    part = NanGuarded(_psize(Bn, P1, C4, M2)) if with_part else None
                    pw = NanGuarded(nchunk * (C4 * C4 + C4)) if with_partial else None
                    call("blindno_rowidft_bwd_zc", ptr(Yd), ptr(dzd), ptr(wd), ptr(xd), ptr(dx.t), ptr(tb.tb),
                         ptr(tb.tab), ptr(part.t) if with_part else None, ptr(tb.Tp) if with_part else None,
                         ptr(pw.t) if with_partial else None, Bn, C4, P1, P2, M1, M2, act, dN1, dN2, sp())
                    return dx, part, pw

                dx, part, pw = _twice(launch)
                label = f"bwd_zc {geom} act={act} crop={crop} partial={with_partial} part={with_part}"
                _ratio(label + " dx", dx.np(Bn, C4, P1, P2), ref, S, N_Z, gw, C_EXTRA + 1)
                if with_partial:
                    got = pw.np(nchunk, C4 * C4 + C4).astype(np.float64).sum(0)
                    _ratio(label + " dWc|dbc", got, gref, Sw, Bn * dN1 * dN2, gww)
                if with_part:
                    _next_spec_check(label + " spectrum of dx", part, ref, S, gw, 0, Bn, P1, P2, N_Z)


# ================================================================================ bwd_lift_zc
@pytest.mark.parametrize("geom", GEOMS)
def test_rowidft_bwd_lift_zc_vs_fp64(geom):
    """rowinv_launch<1, 0, 1, LIFT 1, ZC> (rowfuse_kernel<1, 0, 1, 1, 0, 6, 1, true, 0, ZY>; dx0 is
    not written): the reduced rows [dWc | dbc | dW0 | db0].  n = K1 + 2 m2 + C (dx0's chain) + 4
    (x0's terms) + Bn P1 P2 (the summed elements, an upper count for the crop sums); c = 9.
    nmj = 0 of blindno_rowidft_bwd_lift_zc_mix is the same launch: bit-identical rows."""
    _, call, ptr, query, sp = _api()
    P1, P2 = geom
    N1, N2 = CROP[geom]
    L, Bn = len(IDX), B * len(IDX)
    NP = C4 * C4 + C4 + 4 * C4
    rng = np.random.default_rng(700 + P1 + 2 * P2)
    Y, _, wc, _ = _layer_inputs(rng, Bn, P1, P2)
    dz = _randn(rng, Bn, C4, P1, P2)
    X, grid, w0, b0 = _lift_inputs(rng, N1, N2, C4)
    tb = Tables(P1, P2)
    Yd, dzd, wd, Xd, gd, w0d, b0d, idx = (_dev(Y), _dev(dz), _dev(wc), _dev(X), _dev(grid), _dev(w0), _dev(b0),
                                          _dev(IDX, np.int32))
    nchunk = query("blindno_colspec_bwd_nchunk", Bn, P1)

    def launch(mixed):
        pw = NanGuarded(nchunk * NP)
        head = (ptr(Yd), ptr(dzd), ptr(Xd), ptr(idx), ptr(gd), ptr(w0d), ptr(b0d), ptr(wd), ptr(tb.tb), ptr(tb.tab),
                ptr(pw.t), B, T, L, N1, N2, C4, P1, P2, M1, M2)
        if mixed:
            call("blindno_rowidft_bwd_lift_zc_mix", *head, None, None, None, None, 0, sp())
        else:
            call("blindno_rowidft_bwd_lift_zc", *head, sp())
        return (pw,)

    (pw,) = _twice(lambda: launch(False))
    (pm,) = _twice(lambda: launch(True))
    assert torch.equal(pw.t.view(torch.int32), pm.t.view(torch.int32))
    wc64 = wc.astype(np.float64)
    ref = cr.bwd_lift_rows(cr.z_from_y(Y, P1), P2, dz, wc64, X, IDX, grid, w0, b0)
    Sa = cr.bwd_lift_rows_abs(cr.z_from_y_abs(Y, P1), P2, dz, wc64, X, IDX, grid, w0, b0)
    got = pw.np(nchunk, NP).astype(np.float64).sum(0)
    n = K1 + 2 * M2 + C4 + 4 + Bn * P1 * P2
    for name, sl in (("dWc", slice(0, 16)), ("dbc", slice(16, 20)), ("dW0", slice(20, 32)), ("db0", slice(32, 36))):
        _ratio(f"bwd_lift_zc {geom} {name}", got[sl], ref[sl], Sa[sl], n, None, C_EXTRA + 1)


# ================================================================================ the wave-budget switch
NT7 = 7                                   # distinct samples, tiled
BN_CASES = [
    # P1 = P2 = 32: items = 2 Bn.  2600 <= ROWFUSE_ZC3_MAX -> zc_w3: ZW 3 on 650 of 768 workgroups
    pytest.param(1300, True, id="bn1300_w3"),
    # 2602 items: the 2-wave kernel on ROWFUSE_BLOCKS = 512 workgroups = 2048 waves; items 2048 ..
    # 2601 (samples 1024 ..) are second items of the persistent loop
    pytest.param(1301, False, id="bn1301_w2_persistent"),
]


def _switch_check(label, z, Bn, ref7, S7, gw7, n, P=32):
    """Finite everywhere; fp64 on the first, the last, sample 1024 (the first second item at Bn
    1301) and two in between; every tiled copy of sample 3 equal to its first occurrence."""
    zt = z.t.view(Bn, C4, P, P)
    assert bool(torch.isfinite(zt).all())
    for s in (0, 517, 1024, 1100, Bn - 1):
        r = s % NT7
        _ratio(f"{label} sample {s}", zt[s].cpu().numpy()[None], ref7[r:r + 1], S7[r:r + 1], n, gw7[r:r + 1], C_EXTRA + 1)
    cp = zt[3::NT7].view(torch.int32)
    assert bool((cp == cp[:1]).all())


@pytest.mark.parametrize("Bn,w3", BN_CASES)
def test_wave_budget_switch_epi_zc(Bn, w3):
    """blindno_rowidft_epi_zc (act 1) across zc_w3's threshold, part NULL (RD 0) and part given
    with act_next 1 (RD 2 + CD, the encoder's chained layer)."""
    _, call, ptr, _, sp = _api()
    P = 32
    assert w3 == (0 < 2 * Bn <= 2600) and (w3 or 2 * Bn > 4 * 512)
    rng = np.random.default_rng(800)
    Y, x, wc, bc = _layer_inputs(rng, NT7, P, P)
    rep = (Bn + NT7 - 1) // NT7
    tile = lambda a: np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:Bn]
    tb = Tables(P, P)
    Yd, xd, wd, bd = _dev(tile(Y)), _dev(tile(x)), _dev(wc), _dev(bc)
    wc64, bc64 = wc.astype(np.float64), bc.astype(np.float64)
    ref = sr.row_inv(cr.z_from_y(Y, P), P, x, wc64, bc64, 1)
    S, gw = sr.row_inv_abs(cr.z_from_y_abs(Y, P), P, x, wc64, bc64, 1)
    for with_part in (False, True):
        def launch():
            z = NanGuarded(Bn * C4 * P * P)
            part = NanGuarded(_psize(Bn, P, C4, M2)) if with_part else None
            call("blindno_rowidft_epi_zc", ptr(Yd), ptr(xd), ptr(wd), ptr(bd), ptr(z.t), ptr(tb.tb), ptr(tb.tab),
                 ptr(part.t) if with_part else None, ptr(tb.Tp) if with_part else None, Bn, C4, P, P, M1, M2, 1, 1, P,
                 P, sp())
            return z, part

        z, part = _twice(launch)
        _switch_check(f"epi_zc Bn={Bn} part={with_part}", z, Bn, ref, S, gw, N_Z)
        if with_part:
            assert bool(torch.isfinite(part.t).all())


@pytest.mark.parametrize("Bn,w3", BN_CASES)
def test_wave_budget_switch_epi_lift_zc(Bn, w3):
    """blindno_rowidft_epi_lift_zc across the threshold: one bag of L = Bn snapshots drawn from
    T = 7 (idx = l mod 7), part given with act_next 1 (the encoder's first layer)."""
    _, call, ptr, _, sp = _api()
    P, N1, N2 = 32, 23, 28
    rng = np.random.default_rng(801)
    Y, _, wc, bc = _layer_inputs(rng, NT7, P, P)
    X = _randn(rng, 1, NT7, N1, N2)
    grid, w0, b0 = _randn(rng, N1, N2, 2), _randn(rng, C4, 3, scale=0.6), _randn(rng, C4, scale=0.6)
    rep = (Bn + NT7 - 1) // NT7
    idx = np.arange(Bn) % NT7
    tb = Tables(P, P)
    Yd = _dev(np.tile(Y, (rep, 1, 1, 1))[:Bn])
    wd, bd, Xd, gd, w0d, b0d, idd = _dev(wc), _dev(bc), _dev(X), _dev(grid), _dev(w0), _dev(b0), _dev(idx, np.int32)
    wc64, bc64 = wc.astype(np.float64), bc.astype(np.float64)
    i7 = list(range(NT7))
    x0, x0a = cr.lift_field(X, i7, grid, w0, b0, P, P), cr.lift_field_abs(X, i7, grid, w0, b0, P, P)
    ref = sr.row_inv(cr.z_from_y(Y, P), P, x0, wc64, bc64, 0)
    S, gw = sr.row_inv_abs(cr.z_from_y_abs(Y, P), P, x0a, wc64, bc64, 0)

    def launch():
        z, part = NanGuarded(Bn * C4 * P * P), NanGuarded(_psize(Bn, P, C4, M2))
        call("blindno_rowidft_epi_lift_zc", ptr(Yd), ptr(Xd), ptr(idd), ptr(gd), ptr(w0d), ptr(b0d), ptr(wd), ptr(bd),
             ptr(z.t), ptr(tb.tb), ptr(tb.tab), ptr(part.t), ptr(tb.Tp), 1, NT7, Bn, N1, N2, C4, P, P, M1, M2, 1, sp())
        return z, part

    z, part = _twice(launch)
    _switch_check(f"epi_lift_zc Bn={Bn}", z, Bn, ref, S, gw, N_Z + 4)
    assert bool(torch.isfinite(part.t).all())


def test_persistent_loop_bwd_zc():
    """blindno_rowidft_bwd_zc at Bn 1301 (2602 items on zc_blocks1's 512 workgroups: the persistent
    loop), act 1 with the weight-gradient and column-DFT partials (the encoder's adjoint)."""
    _, call, ptr, query, sp = _api()
    P, Bn = 32, 1301
    rng = np.random.default_rng(802)
    Y, xs, wc, _ = _layer_inputs(rng, NT7, P, P)
    dz = _randn(rng, NT7, C4, P, P)
    rep = (Bn + NT7 - 1) // NT7
    tile = lambda a: np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:Bn]
    tb = Tables(P, P)
    Yd, xd, dzd, wd = _dev(tile(Y)), _dev(tile(xs)), _dev(tile(dz)), _dev(wc)
    nchunk = query("blindno_colspec_bwd_nchunk", Bn, P)
    assert nchunk == 512
    wc64 = wc.astype(np.float64)
    Z, Za = cr.z_from_y(Y, P), cr.z_from_y_abs(Y, P)
    ref = sr.row_inv_adj(Z, P, dz, wc64, xs, 1)
    S, gw = sr.row_inv_adj_abs(Za, P, dz, wc64, xs, 1)

    def launch():
        dx, part, pw = NanGuarded(Bn * C4 * P * P), NanGuarded(_psize(Bn, P, C4, M2)), NanGuarded(nchunk * 20)
        call("blindno_rowidft_bwd_zc", ptr(Yd), ptr(dzd), ptr(wd), ptr(xd), ptr(dx.t), ptr(tb.tb), ptr(tb.tab),
             ptr(part.t), ptr(tb.Tp), ptr(pw.t), Bn, C4, P, P, M1, M2, 1, P, P, sp())
        return dx, part, pw

    dx, part, pw = _twice(launch)
    _switch_check("bwd_zc Bn=1301", dx, Bn, ref, S, gw, N_Z)
    assert bool(torch.isfinite(part.t).all())
    cnt = np.bincount(np.arange(Bn) % NT7, minlength=NT7).astype(np.float64)
    gref = sum(cnt[r] * sr.conv_wgrad(dz[r:r + 1], xs[r:r + 1], 1) for r in range(NT7))
    Sw, gww = zip(*(sr.conv_wgrad_abs(dz[r:r + 1], xs[r:r + 1], 1) for r in range(NT7)))
    _ratio("bwd_zc Bn=1301 dWc|dbc", pw.np(nchunk, 20).astype(np.float64).sum(0), gref,
           sum(c * s for c, s in zip(cnt, Sw)), Bn * P * P, sum(c * g for c, g in zip(cnt, gww)))


# ================================================================================ the unfolded lift entries
# blindno_colspec_ok == 0: P2 40 (no rowfuse shape either: rowinv_mfma_kernel<4, 8, 0, 0, 0, 0, LIFT>)
# and m2 8 at P2 32 (rowfuse_shape: rowfuse_kernel<0, 0, 0, LIFT 1, 0, S 4> unless rowfuse is off)
@pytest.mark.parametrize("rowfuse", [1, 0])
@pytest.mark.parametrize("geom", [pytest.param((32, 40, 12, 23, 28), id="P2_40"),
                                  pytest.param((32, 32, 8, 23, 28), id="m2_8"),
                                  pytest.param((48, 40, 12, 37, 29), id="n2_29")])
def test_unfolded_lift_entries_vs_fp64(fuse, geom, rowfuse):
    """blindno_rowdft_bag_lift (Gt given: n = P2 + 1), blindno_rowdft_bag_lift_dg (Gt formed from
    Dg and fc0: n = P2 + 4) -- At against the reference, and against each other when Gt is built
    from Dg and fc0 (the sum of the two bounds plus Gt's own rounding) -- and
    blindno_rowidft_epi_lift (n = 2 m2 + C + 1 + 4); c = 8."""
    _, call, ptr, query, sp = _api()
    P1, P2, m2, N1, N2 = geom
    L, Bn = len(IDX), B * len(IDX)
    assert query("blindno_colspec_ok", Bn, C4, P1, P2, M1, m2) == 0
    fuse("blindno_set_rowfuse", rowfuse)
    rng = np.random.default_rng(900 + sum(geom))
    X, grid, w0, b0 = _lift_inputs(rng, N1, N2, C4)
    wc, bc = _randn(rng, C4, C4, scale=0.4), _randn(rng, C4, scale=0.4)
    Zs = _crandn(rng, Bn, P1, m2, C4, scale=0.3)
    f32 = lambda z: z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)
    Dg = f32(sr.row_dft(cr.grid_planes(grid, P1, P2), m2)[0])                       # (m2, 3, P1)
    A = np.concatenate([w0[:, 1:], b0[:, None]], 1).astype(np.float64)
    Gt = f32(np.einsum("cp,kph->kch", A, Dg))
    tb = Tables(P1, P2, m2)
    Xd, gd, w0d, b0d, idx, Dd, Gd, wd, bd, Zd = (_dev(X), _dev(grid), _dev(w0), _dev(b0), _dev(IDX, np.int32), _dev(Dg),
                                                 _dev(Gt), _dev(wc), _dev(bc), _dev(Zs))

    def launch():
        A1, A2, z = NanGuarded(Bn * m2 * C4 * P1 * 2), NanGuarded(Bn * m2 * C4 * P1 * 2), NanGuarded(Bn * C4 * P1 * P2)
        dims = (B, T, L, N1, N2, C4, P1, P2, m2, sp())
        call("blindno_rowdft_bag_lift", ptr(Xd), ptr(idx), ptr(w0d), ptr(Gd), ptr(A1.t), ptr(tb.Tp), *dims)
        call("blindno_rowdft_bag_lift_dg", ptr(Xd), ptr(idx), ptr(w0d), ptr(b0d), ptr(Dd), ptr(A2.t), ptr(tb.Tp), *dims)
        call("blindno_rowidft_epi_lift", ptr(Zd), ptr(Xd), ptr(idx), ptr(gd), ptr(w0d), ptr(b0d), ptr(wd), ptr(bd),
             ptr(z.t), ptr(tb.tb), *dims)
        return A1, A2, z

    A1, A2, z = _twice(launch)
    label = f"unfolded lift {geom} rowfuse={rowfuse}"
    a1, a2 = _cx(A1, Bn, m2, C4, P1), _cx(A2, Bn, m2, C4, P1)
    r1, s1 = cr.bag_lift_at(X, IDX, w0, m2, P1, P2, Gt=Gt), cr.bag_lift_at_abs(X, IDX, w0, m2, P1, P2, Gt=Gt)
    r2, s2 = (cr.bag_lift_at(X, IDX, w0, m2, P1, P2, b0=b0, Dg=Dg), cr.bag_lift_at_abs(X, IDX, w0, m2, P1, P2, b0=b0, Dg=Dg))
    _ratio(label + " At (Gt)", a1, r1, s1, P2 + 1)
    _ratio(label + " At (Dg)", a2, r2, s2, P2 + 4)
    both = ((P2 + 1 + C_EXTRA) * s1 + (P2 + 4 + C_EXTRA) * s2 + np.abs(Gt)[None]) * U24
    d = a1 - a2
    r = max(worst(np.abs(d.real), both), worst(np.abs(d.imag), both))
    print(f"{label} At (Gt) vs At (Dg): worst err/bound {r:.3g}")
    assert r <= 1.0, r
    x0, x0a = cr.lift_field(X, IDX, grid, w0, b0, P1, P2), cr.lift_field_abs(X, IDX, grid, w0, b0, P1, P2)
    wc64, bc64 = wc.astype(np.float64), bc.astype(np.float64)
    S, gw = sr.row_inv_abs(Zs, P2, x0a, wc64, bc64, 0)
    _ratio(label + " epi_lift z", z.np(Bn, C4, P1, P2), sr.row_inv(Zs, P2, x0, wc64, bc64, 0), S, 2 * m2 + C4 + 1 + 4, gw)


# ================================================================================ the grid spectra of ops
@pytest.mark.parametrize("geom", GEOMS)
def test_ops_grid_spectra_vs_fp64(geom):
    """ops._grid_spec2 (blindno_lift_fwd with unit weights: exact planes; rowdft_cd C 3 + colmix
    Wt NULL: n = P2 + 16 nb, c = 9) and ops._grid_planes (blindno_rowdft: n = P2, c = 8)."""
    ops = _api()[0]
    P1, P2 = geom
    N1, N2 = CROP[geom]
    rng = np.random.default_rng(1000 + P1 + P2)
    grid = _randn(rng, N1, N2, 2)
    gt = torch.from_numpy(grid).cuda()
    Dg2 = ops._grid_spec2(gt, N1, N2, P1, P2, M1, M2)
    Dg = ops._grid_planes(gt, N1, N2, P1, P2, M2)
    torch.cuda.synchronize()
    pl = cr.grid_planes(grid, P1, P2)
    S, _ = cr.spectrum_abs(pl, M2)
    _ratio(f"_grid_spec2 {geom}", sr.cplx(Dg2.cpu().numpy().reshape(1, M2, 3, K1, 2)), cr.spectrum(pl, M2), S,
           P2 + 16 * (P1 // 16), None, C_EXTRA + 1)
    Sr, _ = sr.row_dft_abs(pl, M2)
    _ratio(f"_grid_planes {geom}", sr.cplx(Dg.cpu().numpy().reshape(1, M2, 3, P1, 2)), sr.row_dft(pl, M2), Sr, P2)
