"""The float64 references of tests/spectral3d_ref.py checked on the host, without a GPU:

* colpass3d fed pack_w3d's output equals fno3d_ref.mixed_spectrum_planes (pinned to the reference's
  goldens by tests/test_fno3d_golden.py) fed the unpacked weights, at every case and both
  directions, to 1e-12; its Xs is the 2D FFT at the kept frequencies;
* pack_w3d and unpack_w3d are adjoint to 1e-13, and the unpack's zeros are fno3d_ref.winners' losers;
* the lift and projection references equal float64 torch autograd of F.linear / F.pad / F.gelu / crop;
* a plain complex64 / fp32 evaluation on the CPU stays inside the derived bounds on the GPU cases'
  inputs (the bounds admit a correct fp32 implementation), max |h| <= 12, the twins dominate;
* the case tables sit on the paths their ids name.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fno3d_ref
import spectral3d_ref as s3
from conftest import rel_l2
from spectral3d_ref import U24, kept_rows, tile_layout, worst


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ================================================================================ colpass3d
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("cid", list(s3.COLPASS_CASES))
def test_colpass3d_equals_mixed_spectrum_planes(cid, direction):
    Bn, Ci, Co, P, m, _ = s3.COLPASS_CASES[cid]
    ws, _ = s3.pack_inputs(cid)
    At, _ = s3.colpass_inputs(cid, direction)
    Xs, Z = s3.colpass3d(At, s3.pack_w3d(ws, m, P), P, m, direction)
    want = fno3d_ref.mixed_spectrum_planes(_t(At), [_t(w) for w in ws], P, direction).numpy()
    cout = Ci if direction else Co
    assert Z.shape == (Bn, P[0] * P[1], m[2], cout)
    assert rel_l2(Z.reshape(want.shape), want) <= 1e-12
    jx, jy = kept_rows(m[0], P[0]), kept_rows(m[1], P[1])
    fx = np.fft.fft2(At)[..., jx, :][..., jy]
    assert rel_l2(Xs.reshape(fx.shape), fx) <= 1e-12


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("cid", list(s3.COLPASS_CASES))
def test_colpass3d_complex64_evaluation_is_inside_the_bound(cid, direction):
    """The same GEMM chain in complex64 with fp32-rounded twiddle tables; the twins dominate."""
    _, _, _, P, m, _ = s3.COLPASS_CASES[cid]
    At, Wt = s3.colpass_inputs(cid, direction)
    refs = s3.colpass3d_all(At, Wt, P, m, direction)
    bounds = s3.colpass3d_bounds(At, Wt, P, m, direction)
    Fx, Fy = (f.astype(np.complex64) for f in s3._axes(P, m))
    K1, K2 = Fx.shape[1], Fy.shape[1]
    a = At.astype(np.complex64)
    T1 = np.einsum("nkcxy,yb->nkcxb", a, Fy)
    X = np.einsum("nkcxb,xa->nkcab", T1, Fx)
    Y = s3._mix(X, Wt.astype(np.complex64).reshape(m[2], K1, K2, *Wt.shape[-2:]), direction)
    U = np.einsum("nkcab,xa->nkcxb", Y, np.conj(Fx))
    Z = np.einsum("nkcxb,yb->nxykc", U, np.conj(Fy))
    for name, got, ref, b, ab in zip(("Xs", "Y", "Z"), (X, Y, Z), refs, bounds, s3.colpass3d_all_abs(At, Wt, P, m, direction)):
        assert np.all(np.abs(ref) <= ab * (1 + 1e-12))
        d = got.reshape(ref.shape).astype(np.complex128) - ref
        r = max(worst(np.abs(d.real), b), worst(np.abs(d.imag), b))
        print(f"{cid} dir {direction} {name}: complex64 err/bound {r:.3f}")
        assert r <= 1.0


# ================================================================================ pack / unpack
@pytest.mark.parametrize("cid", list(s3.PACK_CASES))
def test_pack_unpack_are_adjoint_and_losers_match(cid):
    Ci, Co, P, m = s3.PACK_CASES[cid]
    ws, G = s3.pack_inputs(cid)
    Wt, dws = s3.pack_w3d(ws, m, P), s3.unpack_w3d(G, m, P)
    K1, K2 = min(2 * m[0], P[0]), min(2 * m[1], P[1])
    assert Wt.shape == (m[2], K1 * K2, Ci, Co) and all(d.shape == (Ci, Co, *m) for d in dws)
    lhs = np.vdot(Wt, G).real
    rhs = sum(np.vdot(w, d).real for w, d in zip(ws, dws))
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1e-30)
    lose = s3.losers(m, P)
    for q, win in enumerate(fno3d_ref.winners(m[0], m[1], P[0], P[1])):
        assert np.array_equal(lose[q], ~win.numpy())
        assert np.all(dws[q][:, :, lose[q], :] == 0)
        assert np.all(dws[q][:, :, ~lose[q], :] != 0)
    if cid in ("tile_c16_allkept", "c32_allkept"):
        assert sum(int(l.sum()) for l in lose) > 0                     # corners do overlap here


# ================================================================================ lift
@pytest.mark.parametrize("cid", list(s3.LIFT_CASES))
def test_lift3d_reference_equals_fp64_autograd(cid):
    Bn, N, P, Cin, C = s3.LIFT_CASES[cid]
    t = s3.lift_inputs(cid)
    pad = [0, P[2] - N[2], 0, P[1] - N[1], 0, P[0] - N[0]]
    for dtype in (torch.float64, torch.float32):
        inp, w0, b0 = (_t(t[k]).to(dtype).requires_grad_(True) for k in ("in", "w0", "b0"))
        x0 = F.pad(F.linear(inp, w0, b0).permute(0, 4, 1, 2, 3), pad)
        gi, gw, gb = torch.autograd.grad(x0, (inp, w0, b0), _t(t["dx0"]).to(dtype))
        grads = torch.cat([gw.reshape(-1), gb]).double().numpy()
        ref = s3.lift3d_fwd(t["in"], t["w0"], t["b0"], P)
        d_in, g = s3.lift3d_bwd(t["dx0"], t["in"], t["w0"])
        if dtype == torch.float64:
            assert ref.shape == (Bn, C, *P) and d_in.shape == (Bn, *N, Cin) and g.shape == (C * Cin + C,)
            assert rel_l2(ref, x0.detach().numpy()) <= 1e-12
            assert rel_l2(d_in, gi.numpy()) <= 1e-12 and rel_l2(g, grads) <= 1e-12
            off = np.ones(ref.shape, bool)
            off[:, :, :N[0], :N[1], :N[2]] = False
            assert np.all(ref[off] == 0)
        else:                                                          # fp32 on the CPU against the bounds
            bi, bg = s3.lift3d_bwd_bound(t["dx0"], t["in"], t["w0"])
            r = (worst(np.abs(x0.detach().double().numpy() - ref), s3.lift3d_fwd_bound(t["in"], t["w0"], t["b0"], P)),
                 worst(np.abs(gi.double().numpy() - d_in), bi))
            print(f"{cid}: fp32 err/bound x0 {r[0]:.3f} d_in {r[1]:.3f}")
            assert max(r) <= 1.0
            # the whole-grid fp32 sum is a longer chain than one workgroup's: bound it by the point count
            npts = Bn * N[0] * N[1] * N[2]
            full = bg * (npts + s3.C_LIFT) / (s3.lift_chain(Bn, N) + s3.C_LIFT)
            assert worst(np.abs(grads - g), np.maximum(full, bg)) <= 1.0


# ================================================================================ projection
@pytest.mark.parametrize("cid", list(s3.PROJECT_CASES))
def test_project3d_reference_equals_fp64_autograd(cid):
    Bn, C, P, N, Hd, Cout = s3.PROJECT_CASES[cid]
    t = s3.project_inputs(cid)
    assert s3.project3d_max_abs_h(t["z"], t["w1"], t["b1"], N) <= 12.0
    z, w1, b1, w2, b2 = (_t(t[k]).double().requires_grad_(True) for k in ("z", "w1", "b1", "w2", "b2"))
    zc = z[:, :, :N[0], :N[1], :N[2]].permute(0, 2, 3, 4, 1)
    out = F.linear(F.gelu(F.linear(zc, w1, b1)), w2, b2)
    gz, g1, gb1, g2, gb2 = torch.autograd.grad(out, (z, w1, b1, w2, b2), _t(t["dout"]).double())
    grads = torch.cat([g1.reshape(-1), gb1, g2.reshape(-1), gb2]).numpy()
    a = (t["z"], t["w1"], t["b1"], t["w2"])
    ref = s3.project3d_fwd(*a, t["b2"], N)
    assert ref.shape == (Bn, *N, Cout) and rel_l2(ref, out.detach().numpy()) <= 1e-12
    dz, g = s3.project3d_bwd(*a, t["dout"], N)
    assert dz.shape == (Bn, C, *P) and g.shape == (Hd * C + Hd + Cout * Hd + Cout,)
    assert rel_l2(dz, gz.numpy()) <= 1e-12 and rel_l2(g, grads) <= 1e-12
    bz, bg = s3.project3d_bwd_bound(*a, t["dout"], N)
    off = np.ones(dz.shape, bool)
    off[:, :, :N[0], :N[1], :N[2]] = False
    assert np.all(dz[off] == 0) and np.all(bz[off] == 0) and np.all(bz[~off] > 0) and np.all(bg > 0)
    # with the point count as the chain the restated bound is projection_ref's own
    zv, Ho, Wo = s3._args2d(t["z"], N)
    _, bg2d = s3.pr.project_bwd_bound(zv, t["w1"], t["b1"], t["w2"], t["dout"].reshape(Bn, Ho, Wo, Cout), Ho, Wo)
    _, bgn = s3.project3d_bwd_bound(*a, t["dout"], N, chain=Bn * Ho * Wo)
    assert np.allclose(bgn, bg2d, rtol=1e-12, atol=0) and np.all(bg <= bg2d * (1 + 1e-12))
    assert np.all(np.abs(ref) <= s3.project3d_fwd_abs(*a, t["b2"], N) * (1 + 1e-12))


# ================================================================================ the case tables
@pytest.mark.parametrize("cid", list(s3.COLPASS_CASES))
def test_colpass_case_is_on_its_path(cid):
    Bn, Ci, Co, P, m, tile = s3.COLPASS_CASES[cid]
    assert s3.spectral3d_ok(Bn, Ci, Co, P, m)
    rows = P[0] * P[1]
    got = (tile_layout(Bn, Co, rows, P[2], m[2]), tile_layout(Bn, Ci, rows, P[2], m[2]))
    assert got == tile, (cid, got)
    assert (got[0] == 1) == (cid.startswith("tile_") or cid == "workload_tiles")
    if cid.startswith("plain_"):
        assert got == (0, 0)
    if cid == "tile_c12_dir0_only":
        assert got == (1, 0) and Ci != Co
    if cid == "tile_c16_allkept":
        assert min(2 * m[0], P[0]) == P[0] and min(2 * m[1], P[1]) == P[1] and P[0] % 2 == 1
    if cid == "plain_rows_mod4":
        assert rows % 4 and P[0] % 16 and P[1] % 16
    if cid == "degenerate":
        assert P[0] == 1


def test_pack_cases_pass_the_shape_rule_and_reach_the_nyquist_bin():
    for cid, (Ci, Co, P, m) in s3.PACK_CASES.items():
        assert s3.spectral3d_ok(1, Ci, Co, P, m), cid
    assert s3.PACK_CASES["c32_allkept"][:2] == (32, 32)
    nyq = [cid for cid, (_, _, P, m) in s3.PACK_CASES.items() if P[2] % 2 == 0 and m[2] == P[2] // 2 + 1]
    assert nyq == ["nyquist_m3"]
    _, _, P, m = s3.PACK_CASES["nyquist_m3"]
    vol = P[0] * P[1] * P[2]
    assert np.array_equal(s3.pack_scale(m, P) * vol, [1.0, 2.0, 2.0, 1.0]) and m[2] - 1 == P[2] // 2


def test_second_wave_trip_and_ragged_k():
    st = s3.stage_tiles(*s3.COLPASS_CASES["workload_tiles"][3:5])
    assert {k: v[0] for k, v in st.items()} == {"dft_y": 6, "dft_x": 4, "idft_x": 6, "idft_y": 9}
    assert st["dft_y"][1] % 4 == 2 and st["dft_x"][1] % 4 == 2
    st = s3.stage_tiles(*s3.COLPASS_CASES["xs_second_trip"][3:5])
    assert all(n > 4 and k % 4 == 2 for n, k in st.values())
    assert s3.COLPASS_CASES["workload_tiles"][5] == (1, 1) and 42 * 42 == 1764


def test_lds_limit_case_is_exactly_at_the_limit():
    Bn, Ci, Co, P, m, _ = s3.COLPASS_CASES["lds_limit"]
    assert s3.colpass_lds_bytes(P, m) == 65536 == s3.LDS_LIMIT
    assert s3.colpass_lds_bytes((129, 64, 4), m) > s3.LDS_LIMIT
    assert not s3.spectral3d_ok(Bn, Ci, Co, (129, 64, 4), m)
    assert max(s3.colpass_lds_bytes(c[3], c[4]) for c in s3.COLPASS_CASES.values()) == 65536


def test_lift_cases_are_on_their_paths():
    for cid, (Bn, N, P, Cin, C) in s3.LIFT_CASES.items():
        assert s3.lift3d_ok(Bn, N, P, Cin, C), cid
        assert s3.lift_lds_bytes(Cin, C) <= s3.LDS_LIMIT
    np_ = {cid: c[4] * c[3] + c[4] for cid, c in s3.LIFT_CASES.items()}
    assert np_["np1023"] == 1023 and np_["np1024"] == 1024 and np_["np1023"] > 768     # accumulator slot q = 3
    assert s3.lift_lds_bytes(32, 31) == s3.lift_lds_bytes(31, 32) == 64764
    Bn, N = s3.LIFT_CASES["stride_1045_tiles"][:2]
    npts = Bn * N[0] * N[1] * N[2]
    assert npts == 267300 and s3.lift_tiles(Bn, N) == (1045, 1024) and npts - 1044 * 256 == 36
    assert s3.lift_chain(Bn, N) == 512
    assert s3.lift_tiles(*s3.LIFT_CASES["one_point"][:2]) == (1, 1)
    assert s3.LIFT_CASES["nopad"][1] == s3.LIFT_CASES["nopad"][2]
    assert all(p > n for n, p in zip(*s3.LIFT_CASES["small"][1:3]))
    assert not s3.lift3d_ok(1, (1, 1, 1), (1, 1, 1), 32, 32)                           # 1056 parameters
    assert max(Bn * C * P[0] * P[1] * P[2] for Bn, _, P, _, C in s3.LIFT_CASES.values()) * 4 < 4 * 2 ** 20


def test_project_cases_are_on_their_paths():
    for cid, (Bn, C, P, N, Hd, Cout) in s3.PROJECT_CASES.items():
        assert s3.project3d_ok(Bn, C, P, N, Hd, Cout), cid
        assert any(p > n for p, n in zip(P, N))
    Bn, _, _, N, _, _ = s3.PROJECT_CASES["stride_1055_tiles"]
    npts = Bn * N[0] * N[1] * N[2]
    assert npts == 33759 and s3.project_tiles(Bn, N) == (1055, 1024) and npts - 1054 * 32 == 31
    assert s3.project_chain(Bn, N) == 64
    lds = {cid: s3.project_lds_bytes(c[1], c[4], c[5]) for cid, c in s3.PROJECT_CASES.items()}
    assert max(lds, key=lds.get) == "hd128_c32_cout8" and lds["hd128_c32_cout8"] == s3.project_lds_bytes(32, 128, 8)
    assert {c[5] for c in s3.PROJECT_CASES.values()} >= {1, 2, 8}
    assert {c[4] for c in s3.PROJECT_CASES.values()} >= {1, 37, 128}
    assert not s3.project3d_ok(1, 4, (2, 2, 2), (2, 2, 2), 129, 1)
    assert not s3.project3d_ok(1, 4, (2, 2, 2), (2, 2, 2), 128, 9)
    assert not s3.project3d_ok(1, 33, (2, 2, 2), (2, 2, 2), 128, 1)
    assert U24 == 2.0 ** -24
