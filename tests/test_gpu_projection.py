"""The projection MLP kernels (csrc/project.hip on the matrix cores, the VALU fall-backs of
csrc/fields.hip) called through the C ABI against the float64 references of
tests/projection_ref.py, on every launch path the host code selects (DESIGN.md "Projection launch
paths" maps case ids to instantiations).  The case tables live in projection_ref (the host test
checks the same inputs); each id names the instantiation: `ck` / `cm` = the padded channel count,
`com` = the Cout template value, `t16` (Wo % 16 == 0) or `pt`, worked out from project_fwd_mfma,
project_bwd_mfma and the dispatchers of blindno_project_fwd / _bwd:

  matrix cores: Hd == 128, 1 <= C <= 15, Cout <= 2: <CK = 4 ceil(C/4), COM = Cout, NP, T16>, NP
      (forward) 4 for CK <= 8, else 2; NP (backward) 2 for CK 4, else 1.  CK 4: kGW44 (4x4x1 MFMA for
      dW1, db1 summed apart); CK >= 8 with T16: kDzM (dz on the matrix cores); COM 1: kFoldW2;
      row4 = Wo % 4 == 0 in the non-T16 branch.
  fall-backs: forward <CM, COM> with CM = 4 / 8 / 16 / 32 the channel class and COM = 1 or 4;
      backward (Hd 128 only) <CM = 8 / 16 / 32, 8, COM>.

The acceptance bound is per element and derived (projection_ref's docstring).  out and dz live in
sentinel-guarded buffers pre-filled with the sentinel: dz outside the crop and the slots of out
outside [ooff, ooff + Cout) of each ostride run must still hold it bit for bit.  The per-workgroup
partial rows are summed on the host in float64.  Every check prints its worst err / bound ratio.
"""
import numpy as np
import pytest
import torch

import projection_ref as pr
from projection_ref import Guarded, worst
from spectral_stage_ref import SENT

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
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _ratio(label, got, ref, bound):
    r = worst(np.abs(np.asarray(got, np.float64) - ref), np.broadcast_to(bound, np.shape(ref)))
    print(f"{label}: worst err/bound {r:.3f}")
    assert r <= 1.0, (label, r)
    return r


def _np_total(c):
    return c["Hd"] * c["C"] + c["Hd"] + c["Cout"] * c["Hd"] + c["Cout"]


def _embed(vals, ostride, ooff, fill=np.nan):
    """(..., Cout) values -> the interleaved (..., ostride) buffer the kernels address."""
    buf = np.full(vals.shape[:-1] + (ostride,), fill, np.float32)
    buf[..., ooff:ooff + vals.shape[-1]] = vals
    return buf


def _out_slots(out, c):
    """out: a Guarded of Bn Ho Wo ostride floats -> (its Cout slots, whether the rest is untouched)."""
    ostride, off = c["addr"]
    assert out.margins_intact()
    o = out.cpu().numpy().reshape(c["Bn"], *c["N"], ostride)
    keep = np.ones(ostride, bool)
    keep[off:off + c["Cout"]] = False
    return o[..., ~keep], bool(np.all(o[..., keep] == SENT32))


def _check_dz(label, dz, c, ref, bound):
    Ho, Wo = c["N"]
    assert dz.margins_intact()
    d = dz.cpu().numpy().reshape(c["Bn"], c["C"], *c["P"])
    outside = np.ones(d.shape, bool)
    outside[:, :, :Ho, :Wo] = False
    assert np.all(d[outside] == SENT32), label + ": dz written outside the crop"
    return _ratio(label + " dz", d[:, :, :Ho, :Wo], ref, bound)


def _fwd(c, t, G=1, wbuf=None):
    """One forward call; returns the Guarded output.  G = 2: t is a pair of inputs, wbuf the packed weights."""
    lib, ptr, _, sp = _api()
    ostride, ooff = c["addr"]
    dims = (c["C"], *c["P"], *c["N"], c["Hd"], c["Cout"], ostride, ooff)
    if G == 1:
        out = Guarded(c["Bn"] * c["N"][0] * c["N"][1] * ostride)
        d = [_dev(t[k]) for k in ("z", "w1", "b1", "w2", "b2")]
        rc = lib.blindno_project_fwd(*[ptr(x) for x in d], ptr(out.t), c["Bn"], *dims, sp())
    else:
        out = Guarded(c["Bn"] * c["N"][0] * c["N"][1] * ostride)
        z = _dev(np.concatenate([t[0]["z"], t[1]["z"]]))
        w, wgs, offs = wbuf
        rc = lib.blindno_project_fwd_g(ptr(z), *[ptr(w[o:]) for o in offs], ptr(out.t), 2, wgs, 2 * c["Bn"], *dims, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return out


def _bwd(c, t, nchunk, entry="blindno_project_bwd", lscale=None):
    """One backward call; returns (Guarded dz, Guarded partial)."""
    lib, ptr, _, sp = _api()
    ostride, ooff = c["addr"]
    dz = Guarded(c["Bn"] * c["C"] * c["P"][0] * c["P"][1])
    part = Guarded(nchunk * _np_total(c))
    d = [_dev(t[k]) for k in ("z", "w1", "b1", "w2")]
    dout = _dev(_embed(t["dout"], ostride, ooff))
    dims = (c["Bn"], c["C"], *c["P"], *c["N"], c["Hd"], c["Cout"], ostride, ooff, c["dout_div"])
    if entry == "blindno_project_bwd":
        rc = lib.blindno_project_bwd(*[ptr(x) for x in d], ptr(dout), ptr(dz.t), ptr(part.t), nchunk, *dims, sp())
    else:
        ls = _dev(lscale)
        rc = lib.blindno_project_bwd_w(*[ptr(x) for x in d], ptr(dout), ptr(ls), ptr(dz.t), ptr(part.t), nchunk,
                                       *dims, sp())
    assert rc == 0, f"hip error {rc}"
    torch.cuda.synchronize()
    return dz, part


def _grads(part, nchunk):
    assert part.margins_intact()
    p = part.cpu().double().numpy().reshape(nchunk, -1)
    assert np.isfinite(p).all()
    return p.sum(0)


def _nchunks(c):
    _, _, query, _ = _api()
    d = query("blindno_project_bwd_nchunk", c["Bn"], *c["N"])
    assert d >= 1
    return sorted({1, 3, d})


def _forward_case(c, t):
    a = (t["z"], t["w1"], t["b1"], t["w2"], t["b2"], *c["N"])
    out = _fwd(c, t)
    got, clean = _out_slots(out, c)
    assert clean, c["id"] + ": out written outside its channel slots"
    _ratio(c["id"] + " out", got, pr.project_fwd(*a), pr.project_fwd_bound(*a))
    return out


def _backward_case(c, t, entry="blindno_project_bwd", lscale=None):
    k = (t["z"], t["w1"], t["b1"], t["w2"], t["dout"], *c["N"], c["dout_div"], lscale)
    (dzr, gr), (bz, bg) = pr.project_bwd(*k), pr.project_bwd_bound(*k)
    for nchunk in _nchunks(c):
        dz, part = _bwd(c, t, nchunk, entry, lscale)
        label = f"{c['id']} {entry[8:]} nchunk={nchunk}"
        _check_dz(label, dz, c, dzr, bz)
        _ratio(label + " dW1|db1|dW2|db2", _grads(part, nchunk), gr, bg)


# ================================================================================ matrix cores
@pytest.mark.parametrize("c", pr.MFMA_CASES, ids=lambda c: c["id"])
def test_project_fwd_mfma_vs_fp64(c):
    _forward_case(c, pr.case_inputs(c))


@pytest.mark.parametrize("c", pr.MFMA_CASES, ids=lambda c: c["id"])
def test_project_bwd_mfma_vs_fp64(c):
    _backward_case(c, pr.case_inputs(c))


@pytest.mark.parametrize("c", pr.BCAST_CASES, ids=lambda c: c["id"])
def test_project_bwd_broadcast_and_weights(c):
    """dout_div = 3: sample n reads dout[n // 3]; blindno_project_bwd_w scales it by lscale[n % 3]."""
    t = pr.case_inputs(c)
    _backward_case(c, t)
    _backward_case(c, t, "blindno_project_bwd_w", t["lscale"])


@pytest.mark.parametrize("c", pr.GROUP_CASES, ids=lambda c: c["id"])
def test_project_grouped_vs_fp64(c):
    """G = 2: group g owns samples [g Bg, (g + 1) Bg), reads its weights at + g wgs (NaN between the
    groups) and addresses channel ooff + g Cout of the shared output sample; partial[nchunk][G][np].
    Each group must match the ungrouped reference on its samples with its own weights."""
    lib, ptr, query, sp = _api()
    ts = [pr.case_inputs(c, g) for g in (0, 1)]
    Cout, Hd, C, Bg = c["Cout"], c["Hd"], c["C"], c["Bn"]
    np_ = _np_total(c)
    wgs = np_ + 37
    offs = (0, Hd * C, Hd * C + Hd, Hd * C + Hd + Cout * Hd)             # w1 | b1 | w2 | b2 of a group
    w = np.full(2 * wgs, np.nan, np.float32)
    for g, t in enumerate(ts):
        w[g * wgs:g * wgs + np_] = np.concatenate([t[k].ravel() for k in ("w1", "b1", "w2", "b2")])
    w = _dev(w)
    ostride, ooff = 2 * Cout + 1, 1
    cg = dict(c, addr=(ostride, ooff))
    assert (Bg * c["N"][0] * c["N"][1]) % (16 * (2 if C == 12 else 4)) == 0
    out = _fwd(cg, ts, G=2, wbuf=(w, wgs, offs))
    assert out.margins_intact()
    o = out.cpu().numpy().reshape(Bg, *c["N"], ostride)
    assert np.all(o[..., 0] == SENT32), "out written outside the groups' channels"
    for g, t in enumerate(ts):
        a = (t["z"], t["w1"], t["b1"], t["w2"], t["b2"], *c["N"])
        _ratio(f"{c['id']} fwd group {g}", o[..., ooff + g * Cout:ooff + (g + 1) * Cout], pr.project_fwd(*a),
               pr.project_fwd_bound(*a))
    # backward: dout addressed like the forward's output
    dout = np.full((Bg, *c["N"], ostride), np.nan, np.float32)
    for g, t in enumerate(ts):
        dout[..., ooff + g * Cout:ooff + (g + 1) * Cout] = t["dout"]
    z, doutd = _dev(np.concatenate([ts[0]["z"], ts[1]["z"]])), _dev(dout)
    call_c = dict(c, Bn=2 * Bg)
    for nchunk in sorted({1, 3, query("blindno_project_bwd_nchunk_heads", Bg, *c["N"])}):
        dz = Guarded(2 * Bg * C * c["P"][0] * c["P"][1])
        part = Guarded(nchunk * 2 * np_)
        rc = lib.blindno_project_bwd_g(ptr(z), ptr(w), ptr(w[offs[1]:]), ptr(w[offs[2]:]), ptr(doutd), ptr(dz.t),
                                       ptr(part.t), nchunk, 2, wgs, 2 * Bg, C, *c["P"], *c["N"], Hd, Cout, ostride,
                                       ooff, sp())
        assert rc == 0, f"hip error {rc}"
        torch.cuda.synchronize()
        assert part.margins_intact()
        p = part.cpu().double().numpy().reshape(nchunk, 2, np_).sum(0)
        refs = [(pr.project_bwd(*k), pr.project_bwd_bound(*k))
                for k in ((t["z"], t["w1"], t["b1"], t["w2"], t["dout"], *c["N"]) for t in ts)]
        label = f"{c['id']} bwd_g nchunk={nchunk}"
        _check_dz(label, dz, call_c, np.concatenate([r[0][0] for r in refs]), np.concatenate([r[1][0] for r in refs]))
        for g, ((_, gr), (_, bg)) in enumerate(refs):
            _ratio(f"{label} group {g} dW1|db1|dW2|db2", p[g], gr, bg)


def test_project_fwd_grid_cap():
    """project_fwd_mfma_kernel<4, 1, 4, T16>: 36864 tiles / 8 = 4608 > 2048 workgroups -> the forward's
    stride loop (grp += gridDim.x * kWaves) runs; float64 reference by torch on the device."""
    lib, ptr, _, sp = _api()
    c = pr.GRIDCAP_CASE
    t = pr.case_inputs(c)
    Ho, Wo = c["N"]
    d = {k: torch.from_numpy(t[k]).cuda() for k in ("z", "w1", "b1", "w2", "b2")}
    out = Guarded(c["Bn"] * Ho * Wo)
    rc = lib.blindno_project_fwd(*[ptr(d[k]) for k in ("z", "w1", "b1", "w2", "b2")], ptr(out.t), c["Bn"], c["C"],
                                 *c["P"], Ho, Wo, 128, 1, 1, 0, sp())
    assert rc == 0
    torch.cuda.synchronize()
    assert out.margins_intact()
    z, w1, b1, w2, b2 = (d[k].double() for k in ("z", "w1", "b1", "w2", "b2"))
    zc = z[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    h = zc @ w1.t() + b1
    a = 0.5 * h * (1.0 + torch.erf(h * 0.7071067811865476))
    ref = a @ w2.t() + b2
    u = pr.U24
    dh = (c["C"] + 1 + pr.C_EXTRA) * u * (zc.abs() @ w1.abs().t() + b1.abs())
    bound = (pr.GELU_ABS + pr.GP_SUP * dh) @ w2.abs().t() + (128 + pr.C_EXTRA) * u * (a.abs() @ w2.abs().t() + b2.abs())
    err = (out.t.double().view_as(ref) - ref).abs()
    assert bool((bound > 0).all())
    r = float((err / bound).max())
    print(f"{c['id']} out: worst err/bound {r:.3f}")
    assert r <= 1.0


# ================================================================================ VALU fall-backs
@pytest.mark.parametrize("c", pr.FALLBACK_FWD_CASES, ids=lambda c: c["id"])
def test_project_fwd_fallback_vs_fp64(c):
    _forward_case(c, pr.case_inputs(c))


@pytest.mark.parametrize("c", pr.FALLBACK_BWD_CASES, ids=lambda c: c["id"])
def test_project_bwd_fallback_vs_fp64(c):
    """1024 threads and up to 113 KB of dynamic LDS: the launch's return code is checked first."""
    _backward_case(c, pr.case_inputs(c))


# ================================================================================ determinism
@pytest.mark.parametrize("c", [pr.MFMA_CASES[pr.CHANNELS.index(12) * 2 + 1], pr.FALLBACK_BWD_CASES[2],
                               pr.FALLBACK_FWD_CASES[1]], ids=lambda c: c["id"])
def test_project_is_bit_reproducible(c):
    t = pr.case_inputs(c)
    if "fwd" in c["kinds"]:
        assert torch.equal(_fwd(c, t).buf, _fwd(c, t).buf)
    if "bwd" in c["kinds"]:
        for nchunk in (1, 3):
            (dz1, p1), (dz2, p2) = _bwd(c, t, nchunk), _bwd(c, t, nchunk)
            assert torch.equal(dz1.buf, dz2.buf) and torch.equal(p1.buf, p2.buf)


# ================================================================================ refusals
def test_invalid_projection_calls_are_refused_on_the_host():
    """hipErrorInvalidValue from the host-side checks, nothing launched: the guarded outputs stay
    untouched.  (Buffers are sized for the nearest valid shape and never read.)"""
    lib, ptr, _, sp = _api()
    n = 1 << 16
    src = torch.zeros(n, device="cuda")
    o1, o2 = Guarded(n), Guarded(n)
    p, q1, q2 = ptr(src), ptr(o1.t), ptr(o2.t)

    def fwd(Bn=2, C=4, P1=4, P2=16, Ho=4, Wo=16, Hd=128, Cout=1):
        return int(lib.blindno_project_fwd(p, p, p, p, p, q1, Bn, C, P1, P2, Ho, Wo, Hd, Cout, Cout, 0, sp()))

    def fwd_g(G=2, Bn=2, C=4, Ho=4, Wo=16):
        return int(lib.blindno_project_fwd_g(p, p, p, p, p, q1, G, 1024, Bn, C, 4, 16, Ho, Wo, 128, 1, 2, 0, sp()))

    def bwd(Bn=2, C=4, P1=4, P2=16, Ho=4, Wo=16, Hd=128, Cout=1, nchunk=2, div=1, dz=q1):
        return int(lib.blindno_project_bwd(p, p, p, p, p, dz, q2, nchunk, Bn, C, P1, P2, Ho, Wo, Hd, Cout, Cout, 0,
                                           div, sp()))

    def bwd_g(G=2, Bn=2, C=4, nchunk=2, dz=q1):
        return int(lib.blindno_project_bwd_g(p, p, p, p, p, dz, q2, nchunk, G, 1024, Bn, C, 4, 16, 4, 16, 128, 1, 2,
                                             0, sp()))

    def bwd_w(C=4, div=1, nchunk=2, dz=q1):
        return int(lib.blindno_project_bwd_w(p, p, p, p, p, p, dz, q2, nchunk, 2, C, 4, 16, 4, 16, 128, 1, 1, 0, div,
                                             sp()))

    assert fwd_g(G=3, Bn=3) == INVALID and bwd_g(G=3, Bn=3) == INVALID          # G = 3
    assert fwd_g(Bn=3) == INVALID and bwd_g(Bn=3) == INVALID                    # G does not divide Bn
    assert bwd(div=0) == INVALID and bwd_w(div=0) == INVALID                    # dout_div = 0
    assert fwd(Ho=5) == INVALID and bwd(Ho=5) == INVALID                        # Ho > P1
    assert fwd(Wo=17) == INVALID and bwd(Wo=17) == INVALID                      # Wo > P2
    assert fwd(C=33) == INVALID and bwd(C=33) == INVALID                        # C = 33
    assert fwd(Cout=5) == INVALID and bwd(Cout=5) == INVALID                    # Cout = 5
    assert bwd(nchunk=0) == INVALID and bwd_g(nchunk=0) == INVALID and bwd_w(nchunk=0) == INVALID
    assert bwd(dz=None) == INVALID and bwd_g(dz=None) == INVALID and bwd_w(dz=None) == INVALID
    assert fwd_g(Ho=3, Wo=8) == INVALID                                         # gpts = 24, not a multiple of 16 * 4
    assert fwd_g(C=16) == INVALID and bwd_g(C=16) == INVALID and bwd_w(C=16) == INVALID   # no matrix-core path
    assert bwd(C=16, Hd=64) == INVALID                                          # the fall-back backward: Hd 128 only
    torch.cuda.synchronize()
    assert o1.untouched() and o2.untouched()
