"""The kernels of the 3D Fourier layer (csrc/spectral3d.hip) called through the C ABI, one entry at a
time, against the float64 references of tests/spectral3d_ref.py, on every launch path the host code
selects (DESIGN.md "3D Fourier layer launch paths" maps case ids to kernel instantiations and
branches; the case tables live in spectral3d_ref, whose host test asserts that each id sits on the
path it names).

The acceptance bound is per element and derived (spectral3d_ref's docstring): (n + c) 2^-24 S_abs
with the chain n and the counted c of each output, 3 2^-24 |value| for the weight pack, and
projection_ref's bound for the projection.  Complex outputs are checked per component.  Where the
bound is 0 (the lift's pad, dz off the crop, the unpack's overlap losers) the value must be 0.
Every output (Xs, Y, Z, Wt, the four dw, x0, d_in, partial, out, dz) lives in a sentinel-guarded
buffer pre-filled with the sentinel: after each call the margins are intact and no sentinel is left
inside.  The inputs the header says are not read (dx0 on the pad, z off the crop) are NaN.  The
per-workgroup partial rows are summed on the host in float64.  Every check prints its worst
err / bound ratio.
"""
import numpy as np
import pytest
import torch

import spectral3d_ref as s3
from spectral3d_ref import SENT, U24, Guarded, ri, tile_decode, worst

pytestmark = pytest.mark.gpu

INVALID = 1              # hipErrorInvalidValue
SENT32 = np.float32(SENT)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _api():
    from blindno._lib import load, ptr, query, stream_ptr
    return load(), ptr, query, stream_ptr


def _dev(a):
    """A host array (complex: interleaved pairs) as a flat float32 device tensor."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = ri(a)
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _host(g, *shape):
    """A Guarded output on the host: margins intact, every element written."""
    assert g.margins_intact(), "written outside the output"
    a = g.cpu().numpy()
    assert not np.any(a == SENT32), "sentinel left inside the output"
    assert np.isfinite(a).all()
    return a.reshape(shape)


def _ratio(label, got, ref, bound):
    """got: float32 values (complex: (..., 2) pairs); ref complex or real float64."""
    if np.iscomplexobj(ref):
        ref, bound = ri(ref), np.repeat(np.asarray(bound)[..., None], 2, -1)
    r = worst(np.abs(np.asarray(got, np.float64).reshape(np.shape(ref)) - ref), np.broadcast_to(bound, np.shape(ref)))
    print(f"{label}: worst err/bound {r:.3f}")
    assert r <= 1.0, (label, r)
    return r


# ================================================================================ colpass3d
def _colpass(cid, direction, At, Wt):
    """One call; returns the Guarded (Xs, Y, Z)."""
    from blindno import ops
    lib, ptr, _, sp = _api()
    Bn, Ci, Co, P, m, _ = s3.COLPASS_CASES[cid]
    cin, cout = (Co, Ci) if direction else (Ci, Co)
    K = min(2 * m[0], P[0]) * min(2 * m[1], P[1])
    at, wt = _dev(At), _dev(Wt)
    assert at.numel() == Bn * m[2] * cin * P[0] * P[1] * 2 and wt.numel() == m[2] * K * Ci * Co * 2
    Xs, Y = Guarded(Bn * m[2] * cin * K * 2), Guarded(Bn * m[2] * cout * K * 2)
    Z = Guarded(Bn * P[0] * P[1] * m[2] * cout * 2)
    Tx, Ty = ops.twiddle_axis(P[0], m[0], "cuda"), ops.twiddle_axis(P[1], m[1], "cuda")
    assert Tx.numel() == P[0] * min(2 * m[0], P[0]) * 2 and Ty.numel() == P[1] * min(2 * m[1], P[1]) * 2
    rc = lib.blindno_colpass3d(ptr(at), ptr(wt), ptr(Xs.t), ptr(Y.t), ptr(Z.t), ptr(Tx), ptr(Ty), Bn, Ci, Co, *P, *m,
                               direction, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return Xs, Y, Z


def _decode_z(cid, direction, Z):
    """Z on the host as (Bn, P1 P2, m3, cout, 2), out of the A-tile order where the case is TILE."""
    Bn, Ci, Co, P, m, tile = s3.COLPASS_CASES[cid]
    cout, rows = (Ci if direction else Co), P[0] * P[1]
    flat = _host(Z, -1)
    if not tile[direction]:
        return flat.reshape(Bn, rows, m[2], cout, 2)
    z = tile_decode(flat, Bn, rows, m[2], cout)
    assert not np.isnan(z).any(), "the A-tile scatter left holes"
    return z


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("cid", list(s3.COLPASS_CASES))
def test_colpass3d_vs_fp64(cid, direction):
    _, _, query, _ = _api()
    Bn, Ci, Co, P, m, tile = s3.COLPASS_CASES[cid]
    cin, cout = (Co, Ci) if direction else (Ci, Co)
    assert query("blindno_spectral3d_ok", Bn, Ci, Co, *P, *m) == 1
    assert query("blindno_spectrum_tile_layout", Bn, cout, P[0] * P[1], P[2], m[2]) == tile[direction]
    At, Wt = s3.colpass_inputs(cid, direction)
    refs = s3.colpass3d_all(At, Wt, P, m, direction)
    bounds = s3.colpass3d_bounds(At, Wt, P, m, direction)
    Xs, Y, Z = _colpass(cid, direction, At, Wt)
    K = refs[0].shape[-1]
    label = f"{cid} dir {direction}"
    _ratio(label + " Xs", _host(Xs, Bn, m[2], cin, K, 2), refs[0], bounds[0])
    _ratio(label + " Y", _host(Y, Bn, m[2], cout, K, 2), refs[1], bounds[1])
    _ratio(label + (" Z (A-tile order)" if tile[direction] else " Z"), _decode_z(cid, direction, Z), refs[2], bounds[2])


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("cid", ["tile_c8", "workload_tiles"])
def test_colpass3d_is_deterministic(cid, direction):
    At, Wt = s3.colpass_inputs(cid, direction)
    a, b = _colpass(cid, direction, At, Wt), _colpass(cid, direction, At, Wt)
    for x, y in zip(a, b):
        assert torch.equal(x.buf, y.buf)


@pytest.mark.parametrize("direction", [0, 1])
def test_colpass3d_batch_independence(direction):
    """Sample 0's Xs, Y and Z rows are unchanged bit for bit when sample 1's input is replaced (the
    A-tile order packs four consecutive rows of the flattened batch into one tile)."""
    cid = "tile_c8"
    At, Wt = s3.colpass_inputs(cid, direction)
    other = At.copy()
    other[1] = s3._c64(np.random.default_rng(5), *At.shape[1:])
    a, b = _colpass(cid, direction, At, Wt), _colpass(cid, direction, other, Wt)
    Bn = At.shape[0]
    for x, y in zip(a[:2], b[:2]):
        hx, hy = _host(x, Bn, -1), _host(y, Bn, -1)
        assert np.array_equal(hx[0].view(np.int32), hy[0].view(np.int32)) and not np.array_equal(hx[1], hy[1])
    za, zb = _decode_z(cid, direction, a[2]), _decode_z(cid, direction, b[2])
    assert np.array_equal(za[0].view(np.int32), zb[0].view(np.int32)) and not np.array_equal(za[1], zb[1])


# ================================================================================ weight pack
@pytest.mark.parametrize("cid", list(s3.PACK_CASES))
def test_pack_unpack_w3d_vs_fp64(cid):
    lib, ptr, _, sp = _api()
    Ci, Co, P, m = s3.PACK_CASES[cid]
    ws, G = s3.pack_inputs(cid)
    K = min(2 * m[0], P[0]) * min(2 * m[1], P[1])
    wd = [_dev(w) for w in ws]
    Wt = Guarded(m[2] * K * Ci * Co * 2)
    rc = lib.blindno_pack_w3d(*[ptr(w) for w in wd], ptr(Wt.t), Ci, Co, *m, *P, sp())
    assert rc == 0, f"hip error {rc}"
    dws = [Guarded(Ci * Co * m[0] * m[1] * m[2] * 2) for _ in range(4)]
    gd = _dev(G)
    rc = lib.blindno_unpack_w3d(ptr(gd), *[ptr(d.t) for d in dws], Ci, Co, *m, *P, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    u3 = s3.PACK_ROUNDINGS * U24
    ref = ri(s3.pack_w3d(ws, m, P))
    got = _host(Wt, *ref.shape)
    _ratio(f"{cid} Wt", got, ref, u3 * np.abs(ref))
    lose = s3.losers(m, P)
    tol = float((u3 * np.abs(ref) * np.abs(ri(G))).sum())
    lhs = float((got.astype(np.float64) * ri(G)).sum())
    rhs = 0.0
    for q, (d, r) in enumerate(zip(dws, s3.unpack_w3d(G, m, P))):
        r = ri(r)
        g = _host(d, *r.shape)
        _ratio(f"{cid} dw{q + 1}", g, r, u3 * np.abs(r))
        assert np.all(g[:, :, lose[q]].view(np.int32) == 0), f"dw{q + 1}: an overlap loser is not +0"
        rhs += float((ri(ws[q]) * g.astype(np.float64)).sum())
        tol += float((u3 * np.abs(ri(ws[q])) * np.abs(r)).sum())
    print(f"{cid}: <pack(w), G> {lhs:.9e}  <w, unpack(G)> {rhs:.9e}  |diff| / tol {abs(lhs - rhs) / tol:.3f}")
    assert abs(lhs - rhs) <= tol


# ================================================================================ lift
def _lift_bwd(cid, t, with_din):
    lib, ptr, query, sp = _api()
    Bn, N, P, Cin, C = s3.LIFT_CASES[cid]
    nchunk = query("blindno_lift3d_bwd_nchunk", Bn, *N)
    assert nchunk == s3.lift_tiles(Bn, N)[1]
    dx0 = np.full((Bn, C, *P), np.nan, np.float32)                    # the pad is not read
    dx0[:, :, :N[0], :N[1], :N[2]] = t["dx0"][:, :, :N[0], :N[1], :N[2]]
    d = [_dev(dx0), _dev(t["in"]), _dev(t["w0"])]
    d_in = Guarded(Bn * N[0] * N[1] * N[2] * Cin) if with_din else None
    part = Guarded(nchunk * (C * Cin + C))
    rc = lib.blindno_lift3d_bwd(*[ptr(x) for x in d], ptr(d_in.t) if with_din else None, ptr(part.t), nchunk, Bn, *N,
                                Cin, C, *P, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return d_in, part, nchunk


@pytest.mark.parametrize("cid", list(s3.LIFT_CASES))
def test_lift3d_vs_fp64(cid):
    lib, ptr, _, sp = _api()
    Bn, N, P, Cin, C = s3.LIFT_CASES[cid]
    t = s3.lift_inputs(cid)
    d = [_dev(t[k]) for k in ("in", "w0", "b0")]
    x0 = Guarded(Bn * C * P[0] * P[1] * P[2])
    rc = lib.blindno_lift3d_fwd(*[ptr(x) for x in d], ptr(x0.t), Bn, *N, Cin, C, *P, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    ref = s3.lift3d_fwd(t["in"], t["w0"], t["b0"], P)
    got = _host(x0, *ref.shape)
    _ratio(f"{cid} x0", got, ref, s3.lift3d_fwd_bound(t["in"], t["w0"], t["b0"], P))
    pad = np.ones(ref.shape, bool)
    pad[:, :, :N[0], :N[1], :N[2]] = False
    assert np.all(got[pad].view(np.int32) == 0), "the pad is not +0"

    (rin, rg), (bin_, bg) = s3.lift3d_bwd(t["dx0"], t["in"], t["w0"]), s3.lift3d_bwd_bound(t["dx0"], t["in"], t["w0"])
    d_in, part, nchunk = _lift_bwd(cid, t, True)
    _ratio(f"{cid} d_in", _host(d_in, *rin.shape), rin, bin_)
    rows = _host(part, nchunk, -1)
    _ratio(f"{cid} dW0|db0 ({nchunk} rows, chain {s3.lift_chain(Bn, N)})", rows.astype(np.float64).sum(0), rg, bg)
    if cid in s3.LIFT_NULL_DIN:
        _, part0, _ = _lift_bwd(cid, t, False)
        assert torch.equal(part.buf, part0.buf), "partial rows differ with d_in = NULL"


# ================================================================================ projection
def _nan_off_crop(z, N):
    zz = np.full(z.shape, np.nan, np.float32)
    zz[:, :, :N[0], :N[1], :N[2]] = z[:, :, :N[0], :N[1], :N[2]]
    return zz


@pytest.mark.parametrize("cid", list(s3.PROJECT_CASES))
def test_project3d_vs_fp64(cid):
    lib, ptr, query, sp = _api()
    Bn, C, P, N, Hd, Cout = s3.PROJECT_CASES[cid]
    t = s3.project_inputs(cid)
    a = (t["z"], t["w1"], t["b1"], t["w2"])
    assert s3.project3d_max_abs_h(*a[:3], N) <= 12.0
    ref, bound = s3.project3d_fwd(*a, t["b2"], N), s3.project3d_fwd_bound(*a, t["b2"], N)
    (rz, rg), (bz, bg) = s3.project3d_bwd(*a, t["dout"], N), s3.project3d_bwd_bound(*a, t["dout"], N)

    d = [_dev(_nan_off_crop(t["z"], N))] + [_dev(t[k]) for k in ("w1", "b1", "w2", "b2")]
    out = Guarded(Bn * N[0] * N[1] * N[2] * Cout)
    rc = lib.blindno_project3d_fwd(*[ptr(x) for x in d], ptr(out.t), Bn, C, *P, *N, Hd, Cout, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    _ratio(f"{cid} out", _host(out, *ref.shape), ref, bound)

    nchunk = query("blindno_project3d_bwd_nchunk", Bn, *N)
    assert nchunk == s3.project_tiles(Bn, N)[1]
    dz, part = Guarded(Bn * C * P[0] * P[1] * P[2]), Guarded(nchunk * rg.size)
    dout = _dev(t["dout"])
    rc = lib.blindno_project3d_bwd(*[ptr(x) for x in d[:4]], ptr(dout), ptr(dz.t), ptr(part.t), nchunk, Bn, C, *P, *N,
                                   Hd, Cout, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    gz = _host(dz, *rz.shape)
    off = np.ones(rz.shape, bool)
    off[:, :, :N[0], :N[1], :N[2]] = False
    assert np.all(gz[off].view(np.int32) == 0), "dz off the crop is not +0"
    _ratio(f"{cid} dz", gz, rz, bz)
    rows = _host(part, nchunk, -1)
    _ratio(f"{cid} dW1|db1|dW2|db2 ({nchunk} rows, chain {s3.project_chain(Bn, N)})", rows.astype(np.float64).sum(0),
           rg, bg)


# ================================================================================ refusals
def test_3d_entries_refuse():
    """hipErrorInvalidValue from the host-side argument checks, nothing launched: every guarded output
    stays untouched, and a small valid call of each entry on the same stream succeeds afterwards.
    (Buffers hold 2^16 floats, more than any shape here would address, and are never read.)"""
    lib, ptr, query, sp = _api()
    n = 1 << 16
    src = torch.zeros(n, device="cuda")
    outs = [Guarded(n) for _ in range(5)]
    p = ptr(src)
    o = [ptr(g.t) for g in outs]

    def nulls(fn, ptrs, skip=()):
        """fn(list of pointers) with each pointer in turn replaced by NULL."""
        for i in range(len(ptrs)):
            if i not in skip:
                assert int(fn(ptrs[:i] + [None] + ptrs[i + 1:])) == INVALID, (fn.__name__, i)

    def colpass(ptrs=None, Bn=1, Ci=2, Co=2, P=(4, 4, 4), m=(2, 2, 2), direction=0):
        return int(lib.blindno_colpass3d(*(ptrs or [p, p, o[0], o[1], o[2], p, p]), Bn, Ci, Co, *P, *m, direction, sp()))

    def pack(ptrs=None, Ci=2, Co=2, P=(4, 4, 4), m=(2, 2, 2)):
        return int(lib.blindno_pack_w3d(*(ptrs or [p, p, p, p, o[0]]), Ci, Co, *m, *P, sp()))

    def unpack(ptrs=None, Ci=2, Co=2, P=(4, 4, 4), m=(2, 2, 2)):
        return int(lib.blindno_unpack_w3d(*(ptrs or [p, o[0], o[1], o[2], o[3]]), Ci, Co, *m, *P, sp()))

    def lift_fwd(ptrs=None, Bn=1, N=(2, 2, 2), P=(3, 3, 3), Cin=2, C=2):
        return int(lib.blindno_lift3d_fwd(*(ptrs or [p, p, p, o[0]]), Bn, *N, Cin, C, *P, sp()))

    def lift_bwd(ptrs=None, Bn=1, N=(2, 2, 2), P=(3, 3, 3), Cin=2, C=2, dn=0):
        nchunk = query("blindno_lift3d_bwd_nchunk", Bn, *N) + dn
        return int(lib.blindno_lift3d_bwd(*(ptrs or [p, p, p, o[0], o[1]]), nchunk, Bn, *N, Cin, C, *P, sp()))

    def proj_fwd(ptrs=None, Bn=1, C=2, P=(3, 3, 3), N=(2, 2, 2), Hd=4, Cout=2):
        return int(lib.blindno_project3d_fwd(*(ptrs or [p, p, p, p, p, o[0]]), Bn, C, *P, *N, Hd, Cout, sp()))

    def proj_bwd(ptrs=None, Bn=1, C=2, P=(3, 3, 3), N=(2, 2, 2), Hd=4, Cout=2, dn=0):
        nchunk = query("blindno_project3d_bwd_nchunk", Bn, *N) + dn
        return int(lib.blindno_project3d_bwd(*(ptrs or [p, p, p, p, p, o[0], o[1]]), nchunk, Bn, C, *P, *N, Hd, Cout,
                                             sp()))

    assert colpass(direction=2) == INVALID and colpass(direction=-1) == INVALID
    nulls(lambda q: colpass(q), [p, p, o[0], o[1], o[2], p, p])
    nulls(lambda q: pack(q), [p, p, p, p, o[0]])
    nulls(lambda q: unpack(q), [p, o[0], o[1], o[2], o[3]])
    nulls(lambda q: lift_fwd(q), [p, p, p, o[0]])
    nulls(lambda q: lift_bwd(q), [p, p, p, o[0], o[1]], skip=(3,))      # d_in may be NULL
    nulls(lambda q: proj_fwd(q), [p, p, p, p, p, o[0]])
    nulls(lambda q: proj_bwd(q), [p, p, p, p, p, o[0], o[1]])
    for fn in (colpass, pack, unpack):
        assert fn(m=(5, 2, 2)) == INVALID                                # m1 > P1
        assert fn(m=(2, 5, 2)) == INVALID                                # m2 > P2
        assert fn(m=(2, 2, 4)) == INVALID                                # m3 > P3/2 + 1
        assert fn(P=(4, 4, 96), m=(2, 2, 49)) == INVALID                 # m3 = 49 (<= P3/2 + 1 = 49)
        assert fn(Ci=33) == INVALID and fn(Co=33) == INVALID
        assert fn(Ci=1, Co=1, P=(129, 64, 4), m=(1, 32, 1)) == INVALID   # 66 048 bytes of LDS
        assert fn(Ci=0) == INVALID and fn(m=(2, 2, 0)) == INVALID
    for fn in (lift_fwd, lift_bwd):
        assert fn(N=(1, 1, 1), P=(1, 1, 1), Cin=32, C=32) == INVALID     # C Cin + C = 1056
        assert fn(C=33) == INVALID and fn(Cin=33) == INVALID
        for ax in range(3):
            assert fn(P=tuple(1 if i == ax else 3 for i in range(3))) == INVALID      # P < N on one axis
    assert lift_bwd(dn=1) == INVALID and lift_bwd(dn=-1) == INVALID
    for fn in (proj_fwd, proj_bwd):
        assert fn(Hd=129) == INVALID and fn(Cout=9) == INVALID and fn(C=33) == INVALID
        for ax in range(3):
            assert fn(P=tuple(1 if i == ax else 3 for i in range(3))) == INVALID
    assert proj_bwd(dn=1) == INVALID and proj_bwd(dn=-1) == INVALID
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
    for fn in (colpass, lambda: colpass(direction=1), pack, unpack, lift_fwd, lift_bwd, proj_fwd, proj_bwd):
        assert fn() == 0
    torch.cuda.synchronize()
    assert all(g.margins_intact() for g in outs)
