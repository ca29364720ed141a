"""The 2D / 1D spectral stage kernels (csrc/spectral.hip, csrc/rowinv.hip) called through the C
ABI, one stage at a time, against the float64 stage references of tests/spectral_stage_ref.py --
on every launch path the host code selects (DESIGN.md "Spectral stage launch paths" tabulates the
predicates and the case that covers each branch; each case below names the kernel instantiation
it is meant to reach and the predicate values that send it there, worked out from rowdft_plan,
blindno_colpass_g, rowinv_launch, rowinv_geom_general, rowfuse_shape and rowinv_tile_layout).

The acceptance bound is per element and derived, not measured: an output that is a sum of n fp32
products of fp32 operands satisfies |got - ref| <= (n + c) 2^-24 S_abs, S_abs the same formula
with every operand replaced by its modulus, n the number of accumulated terms along the stage's
chain, and c = C_EXTRA = 8 for the single roundings outside the accumulation: the two twiddle
tables (each entry rounded once), the scale c_k / (P1 P2) (its reciprocal, its product with c_k,
its application), the result, and two for the fused multiply-add / split-accumulator differences
between summation orders.  The f32 matrix-core instructions accumulate in exact f32 steps
(MI355X: v_mfma_f32_16x16x4_f32, "f32 in/acc, exact f32"), so they add nothing beyond n.  Where
GELU / GELU' is evaluated on load, 5e-7 (>= the 4.2e-7 / 3.2e-7 of csrc/common.h, |z| <= 12)
times the summed weight of the GELU-evaluated operands is added.  Complex outputs are checked
per component.  Where the bound is 0 the error must be 0.  Outputs live in sentinel-guarded
buffers; the scratch Y is NaN-filled.  Every check prints its worst err / bound ratio.
"""
import numpy as np
import pytest
import torch

import spectral_stage_ref as sr
from conftest import rel_l2
from spectral_stage_ref import GELU_ABS, U24, Guarded, worst

pytestmark = pytest.mark.gpu

C_EXTRA = 8              # c of the bound (module docstring)
INVALID = 1              # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


@pytest.fixture()
def switches():
    """Both kernel-selection switches on for the test, the previous settings restored after."""
    from blindno._lib import query
    prev_r, prev_c = query("blindno_set_rowfuse", 1), query("blindno_set_colfuse", 1)
    yield query
    query("blindno_set_rowfuse", prev_r)
    query("blindno_set_colfuse", prev_c)


def _api():
    from blindno import ops
    from blindno._lib import call, load, ptr, query, stream_ptr
    return ops, call, load, ptr, query, stream_ptr


def _randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _crandn(rng, *shape, scale=1.0):
    """fp32-representable complex values (as complex128)."""
    return _randn(rng, *shape, scale=scale).astype(np.float64) + 1j * _randn(rng, *shape, scale=scale).astype(np.float64)


def _dev(a):
    """A host array (complex: interleaved pairs) as a flat float32 device tensor."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = sr.ri(a)
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _ratio(label, got, ref, S, n, gw=None):
    """Worst err / bound of one output; bound = (n + c) 2^-24 S_abs + 5e-7 gelu-weight."""
    bound = (n + C_EXTRA) * U24 * np.asarray(S, np.float64)
    if gw is not None:
        bound = bound + GELU_ABS * np.asarray(gw, np.float64)
    bound = np.broadcast_to(bound, np.shape(ref))
    if np.iscomplexobj(ref):
        d = np.asarray(got) - ref
        r = max(worst(np.abs(d.real), bound), worst(np.abs(d.imag), bound))
    else:
        r = worst(np.abs(np.asarray(got, np.float64) - ref), bound)
    print(f"{label}: worst err/bound {r:.3f}")
    assert r <= 1.0, (label, r)
    return r


# ================================================================================ row DFT
# (Bn, C, P1, P2, m2), input offset in floats, valid region
ROWDFT_CASES = [
    # rowdft_mfma_kernel<1, unaligned, no stage>: Npad 16 -> 1 tile; P2 % 4 = 2; 30 rows = one
    # full + one partial 16-row tile; nwork 2 < 4 blocks -> twiddles not staged
    pytest.param((2, 3, 5, 18, 4), 0, None, id="nt1_unaligned_partial_row_tile"),
    # m2 = P2/2 + 1 = 10 (Nyquist kept): Npad 32 -> 2 tiles, nrt 2 < 512 -> NT 1, 2 groups
    pytest.param((2, 3, 5, 18, 10), 0, None, id="nt1_all_modes"),
    # <1, aligned>: 128 rows, nrt 8; Npad 32 -> 2 tiles; 8 < 512 -> NT 1 x 2 groups
    pytest.param((2, 4, 16, 40, 12), 0, None, id="nt1_two_groups_aligned"),
    # the same shape from a base one float past 16-B alignment: <1, unaligned> at P2 % 4 == 0
    pytest.param((2, 4, 16, 40, 12), 1, None, id="unaligned_base_pointer"),
    # <2, aligned, stage>: 8192 rows, nrt 512; Npad 32 -> 2 tiles; 512 * 1 >= 512 -> NT 2
    pytest.param((8, 16, 64, 64, 12), 0, None, id="nt2"),
    # <3, aligned, stage>: Npad 48 -> 3 tiles; 512 * 1 >= 512 -> NT 3
    pytest.param((8, 16, 64, 64, 24), 0, None, id="nt3"),
    # <4, aligned, stage>: Npad 64 -> 4 tiles -> NT 4
    pytest.param((8, 16, 64, 64, 32), 0, None, id="nt4"),
    # the header's limits C 32, m2 48: Npad 96 -> 6 tiles, nrt 256: NT 4 keeps 256 * 2 >= 512,
    # 6 % 4 -> NT 3 x 2 groups; nwork 512 >= 4 * 128 blocks -> staged
    pytest.param((4, 32, 32, 96, 48), 0, None, id="nt3_two_groups_limits"),
    # blindno_rowdft_crop: KB = ceil(17/16) = 2 K blocks, rows h >= 13 and columns w >= 17 NaN
    pytest.param((3, 4, 20, 36, 8), 0, (13, 17), id="valid_region"),
]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("geom,off,valid", ROWDFT_CASES)
def test_rowdft_vs_fp64(geom, off, valid, act):
    ops, call, _, ptr, _, sp = _api()
    Bn, C, P1, P2, m2 = geom
    rng = np.random.default_rng(100 + sum(geom) + act)
    x = _randn(rng, Bn, C, P1, P2)
    xd = x.copy()
    if valid is not None:                                   # never read outside the valid region
        xd[:, :, valid[0]:, :] = np.nan
        xd[:, :, :, valid[1]:] = np.nan
    buf = torch.zeros(x.size + 4, device="cuda")
    xt = buf[off:off + x.size]
    xt.copy_(torch.from_numpy(xd.reshape(-1)))
    assert xt.data_ptr() % 16 == 4 * off
    At = Guarded(Bn * m2 * C * P1 * 2)
    Tp = ops.twiddle_mfma(P2, m2, "cuda")
    if valid is None:
        call("blindno_rowdft", ptr(xt), ptr(At.t), ptr(Tp), Bn, C, P1, P2, m2, act, sp())
    else:
        call("blindno_rowdft_crop", ptr(xt), ptr(At.t), ptr(Tp), Bn, C, P1, P2, m2, act, valid[0], valid[1], sp())
    torch.cuda.synchronize()
    assert At.margins_intact()
    got = sr.cplx(At.cpu().numpy().reshape(Bn, m2, C, P1, 2))
    S, cnt = sr.row_dft_abs(x, m2, act, valid)
    # n = P2 products per component
    _ratio(f"rowdft {geom} act={act} off={off} valid={valid}", got, sr.row_dft(x, m2, act, valid), S, P2,
           cnt if act else None)


# ================================================================================ column pass
# (Bn, Ci, Co, P1, P2, m1, m2), weight groups Gw, colfuse setting, tile layout of Z (dir 0, dir 1)
COLPASS_CASES = [
    # colfuse_kernel<dir, 3, 8>: Ci == Co = 4, K1 8 -> K1p 16, 12 pairs / G 4 = 3 workgroups < 512
    # -> 8 waves, KS 8, HB 2 -> HBc 1; plain Z
    pytest.param((2, 4, 4, 24, 24, 4, 6), 1, 1, (0, 0), id="fused_plain"),
    # K1 = min(12, 10) = P1: the identity row map; G = 16/3 = 5; <3, 8>
    pytest.param((2, 3, 3, 10, 16, 6, 5), 1, 1, (0, 0), id="fused_identity_row_map"),
    # odd P1 -> vec 0 (scalar At reads); G = 3; <3, 8>
    pytest.param((2, 5, 5, 21, 20, 4, 4), 1, 1, (0, 0), id="fused_odd_P1_nonvector"),
    # C 12 (the unrolled mix), m2 8 even, P1 32 -> tile layout; <3, 8>
    pytest.param((2, 12, 12, 32, 32, 8, 8), 1, 1, (1, 1), id="fused_tiled_c12"),
    # C 8, m2 48 (m2/2 = 24 <= 24), P1 16 -> tile layout; <3, 8>
    pytest.param((2, 8, 8, 16, 100, 4, 48), 1, 1, (1, 1), id="fused_tiled_c8_m48"),
    # C 16, m2 10, P1 20 -> tile layout; <3, 8>
    pytest.param((2, 16, 16, 20, 36, 4, 10), 1, 1, (1, 1), id="fused_tiled_c16"),
    # 171 * 12 = 2052 pairs / G 4 = 513 workgroups >= 512 -> 4 waves (170 gives 510); K1 24 ->
    # Jt 2, KS 2, HBc 1: <3, 4>
    pytest.param((171, 4, 4, 32, 24, 12, 12), 1, 1, (0, 0), id="fused_w4_many_workgroups"),
    # K1 64 -> Jt 4 < 8 waves -> KS 2; HB 8 -> HBc 4: <5, 8>
    pytest.param((1, 4, 4, 128, 8, 32, 2), 1, 1, (0, 0), id="fused_h5"),
    # HB 11, KS 2 -> HBc 6: <10, 8>
    pytest.param((1, 4, 4, 176, 8, 32, 2), 1, 1, (0, 0), id="fused_h10_w8"),
    # C 12: G 1, 16 * 32 = 512 pairs -> 512 workgroups -> 4 waves; Jt 4 -> KS 1; HB = HBc = 10:
    # <10, 4>; tile layout (m2/2 = 16)
    pytest.param((16, 12, 12, 160, 64, 32, 32), 1, 1, (1, 1), id="fused_h10_w4_c12_many_pairs"),
    # Ci != Co -> coldft_mix_kernel<dir, full> + colidft_kernel; HB 2 <= 10, one workgroup
    pytest.param((2, 3, 5, 20, 18, 4, 5), 1, 1, (0, 0), id="split_ci_ne_co"),
    # Ci != Co, more than 16 channels (cout 24 / 20: no tile layout)
    pytest.param((2, 20, 24, 18, 34, 5, 17), 1, 1, (0, 0), id="split_ci_ne_co_wide"),
    # Ci == Co = 32 > 16 -> split
    pytest.param((2, 32, 32, 16, 16, 4, 4), 1, 1, (0, 0), id="split_c32"),
    # K1 = K1p = 80 > 64 -> split, full (HB 6)
    pytest.param((1, 4, 4, 96, 16, 40, 4), 1, 1, (0, 0), id="split_k1p_80"),
    # HB 11 > 10 -> coldft_mix_kernel<dir, not full>
    pytest.param((1, 2, 3, 176, 8, 3, 2), 1, 1, (0, 0), id="split_not_full"),
    # blindno_set_colfuse(0): the split kernels on the C 12 tiled shape (colidft writes the tiles)
    pytest.param((2, 12, 12, 32, 32, 8, 8), 1, 0, (1, 1), id="split_tiled_c12_colfuse_off"),
    # blindno_colpass_g, two weight groups at stride wtgs: fused + tiled, and split
    pytest.param((4, 12, 12, 32, 32, 8, 8), 2, 1, (1, 1), id="grouped_fused_tiled"),
    pytest.param((4, 3, 5, 20, 18, 4, 5), 2, 1, (0, 0), id="grouped_split"),
]


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("geom,Gw,colfuse,tiled", COLPASS_CASES)
def test_colpass_vs_fp64(switches, geom, Gw, colfuse, tiled, direction):
    ops, call, _, ptr, query, sp = _api()
    Bn, Ci, Co, P1, P2, m1, m2 = geom
    cin, cout = (Ci, Co) if direction == 0 else (Co, Ci)
    K1 = min(2 * m1, P1)
    K1p = 16 * ((K1 + 15) // 16)
    rng = np.random.default_rng(200 + sum(geom) + direction)
    At = _crandn(rng, Bn, m2, cin, P1)
    Wt = _crandn(rng, Gw, m2, K1, Ci, Co, scale=0.5)            # the groups get different weights
    # the layout contract (include/blindno.h blindno_spectrum_tile_layout)
    lay = query("blindno_spectrum_tile_layout", Bn, cout, P1, P2, m2)
    assert lay == tiled[direction] == sr.tile_layout(Bn, cout, P1, P2, m2)
    FB, GB = ops.twiddle_cols(P1, m1, "cuda")
    Xs, Z = Guarded(Bn * m2 * cin * K1 * 2), Guarded(Bn * P1 * m2 * cout * 2)
    Y = torch.full((Bn * m2 * cout * K1p * 2,), float("nan"), device="cuda")
    Atd, Wtd = _dev(At), _dev(Wt)
    switches("blindno_set_colfuse", colfuse)
    if Gw == 1:
        call("blindno_colpass", ptr(Atd), ptr(Wtd), ptr(Xs.t), ptr(Y), ptr(Z.t), ptr(FB), ptr(GB), Bn, Ci, Co,
             P1, m1, m2, P2, direction, sp())
    else:
        call("blindno_colpass_g", ptr(Atd), ptr(Wtd), ptr(Xs.t), ptr(Y), ptr(Z.t), ptr(FB), ptr(GB), Gw,
             m2 * K1 * Ci * Co * 2, Bn, Ci, Co, P1, m1, m2, P2, direction, sp())
    torch.cuda.synchronize()
    assert Xs.margins_intact() and Z.margins_intact()
    Wn = Wt[np.arange(Bn) // (Bn // Gw)] if Gw > 1 else Wt[0]
    Xr, Zr = sr.col_pass(At, Wn, P1, P2, m1, direction)
    Xa, Za = sr.col_pass_abs(At, Wn, P1, P2, m1, direction)
    Zg = Z.cpu().numpy()
    Zg = sr.tile_decode(Zg, Bn, P1, m2, cout) if lay else Zg.reshape(Bn, P1, m2, cout, 2)
    label = f"colpass {geom} dir={direction} Gw={Gw} colfuse={colfuse}"
    # Xs: P1 terms; Z: the chain P1 (column DFT) + cin (mix) + K1 (column inverse)
    _ratio(label + " Xs", sr.cplx(Xs.cpu().numpy().reshape(Bn, m2, cin, K1, 2)), Xr, Xa, P1)
    _ratio(label + " Z", sr.cplx(Zg), Zr, Za, P1 + cin + K1)


# ================================================================================ 1D mix
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("geom", [
    pytest.param((3, 4, 5, 11, 20), id="nyquist_bin"),       # m = P2/2 + 1: c_10 = 1
    pytest.param((2, 3, 2, 8, 15), id="odd_P2"),
    pytest.param((5, 1, 1, 1, 8), id="dc_only"),
    pytest.param((2, 32, 32, 48, 96), id="limits"),
])
def test_mix1d_vs_fp64(geom, direction):
    _, call, _, ptr, _, sp = _api()
    Bn, Ci, Co, m, P2 = geom
    cin, cout = (Ci, Co) if direction == 0 else (Co, Ci)
    rng = np.random.default_rng(300 + sum(geom) + direction)
    At, Wt = _crandn(rng, Bn, m, cin), _crandn(rng, m, Ci, Co, scale=0.5)
    Xs, Z = Guarded(Bn * m * cin * 2), Guarded(Bn * m * cout * 2)
    call("blindno_mix1d", ptr(_dev(At)), ptr(_dev(Wt)), ptr(Xs.t), ptr(Z.t), Bn, Ci, Co, m, P2, direction, sp())
    torch.cuda.synchronize()
    assert Xs.margins_intact() and Z.margins_intact()
    Xr, Zr = sr.mix1d(At, Wt, P2, direction)
    Xa, Za = sr.mix1d_abs(At, Wt, P2, direction)
    label = f"mix1d {geom} dir={direction}"
    _ratio(label + " Xs", sr.cplx(Xs.cpu().numpy().reshape(Bn, m, cin, 2)), Xr, Xa, 1)
    _ratio(label + " Z", sr.cplx(Z.cpu().numpy().reshape(Bn, m, cout, 2)), Zr, Za, cin)


# ================================================================================ row inverse
# (Bn, C, P1, P2, m2), weight groups G, rowfuse setting, tile layout of Z
ROWINV_CASES = [
    # rowfuse_kernel<S>: C 4, m2 % 4 == 0, P1 % 16 == 0, P2 % 32 == 0, 2 m2 <= P2 (a crop with
    # dN2 % 4 != 0 sends the adjoint to rowinv_mfma_kernel<4, 8>)
    pytest.param((2, 4, 16, 32, 4), 1, 1, 0, id="rowfuse_s2"),
    pytest.param((2, 4, 16, 32, 8), 1, 1, 0, id="rowfuse_s4"),
    pytest.param((2, 4, 32, 64, 12), 1, 1, 0, id="rowfuse_s6"),
    pytest.param((2, 4, 16, 32, 16), 1, 1, 0, id="rowfuse_s8"),
    # blindno_set_rowfuse(0): rowinv_mfma_kernel<CM 4, KS 8> on the S = 4 shape
    pytest.param((2, 4, 16, 32, 8), 1, 0, 0, id="general_cm4_rowfuse_off"),
    # <CM 4, KS 8>: 10 rows -> a partial quad, C 3 a partial channel group, odd m2
    pytest.param((2, 3, 5, 18, 5), 1, 1, 0, id="general_cm4_tails"),
    # <CM 8, KS 8>: C 6 = 1.5 groups
    pytest.param((2, 6, 10, 20, 7), 1, 1, 0, id="general_cm8"),
    # C 8 with odd m2: no tile layout -> <CM 8, KS 8>
    pytest.param((2, 8, 16, 32, 9), 1, 1, 0, id="general_c8_odd_m2"),
    # C 12, P1 % 4 != 0: no tile layout -> <CM 16, KS 16> (ks 10)
    pytest.param((2, 12, 18, 40, 20), 1, 1, 0, id="general_cm16_ks16"),
    # <CM 32, KS 16>: C 20 = 5 groups of the 8 (ks 9)
    pytest.param((2, 20, 6, 34, 17), 1, 1, 0, id="general_cm32_channel_tail"),
    # the header's limits: <CM 32, KS 24>
    pytest.param((1, 32, 8, 96, 48), 1, 1, 0, id="general_cm32_ks24_limits"),
    # ldsb: m2 6 -> no rowfuse; base = 64 * 256 / 4 = 4096 items >= ROWINV_MIN_ITEMS -> TPW = NT
    # = 3; 4096 >= ROWINV_LDSB_ITEMS, 4 items per block * 3 >= 2 * 3 -> <CM 4, KS 8, ldsb 1>
    pytest.param((64, 4, 256, 48, 6), 1, 1, 0, id="general_ldsb_c4"),
    # ldsb with C > 4: C 6 (NG 2) -> base = 32 * 256 / 4 * 2 = 4096, NT = TPW = 2, 4 * 2 >= 4;
    # C 6 has no tile layout -> <CM 8, KS 8, ldsb 1>
    pytest.param((32, 6, 256, 18, 5), 1, 1, 0, id="general_ldsb_c6"),
    # rowinv_wide_kernel<C, KS, full>: tile layout, full-field dz (a crop: rowinv_mfma_kernel
    # reading the tile order)
    pytest.param((2, 8, 16, 32, 16), 1, 1, 1, id="wide_c8_ks8_full"),
    pytest.param((2, 8, 16, 48, 20), 1, 1, 1, id="wide_c8_ks16"),
    pytest.param((2, 8, 16, 100, 48), 1, 1, 1, id="wide_c8_ks24_full"),
    pytest.param((2, 12, 16, 40, 12), 1, 1, 1, id="wide_c12_ks8"),
    pytest.param((2, 12, 32, 64, 32), 1, 1, 1, id="wide_c12_ks16_full"),
    pytest.param((2, 16, 20, 36, 10), 1, 1, 1, id="wide_c16_ks8"),
    pytest.param((2, 16, 16, 64, 32), 1, 1, 1, id="wide_c16_ks16_full"),
    # blindno_rowidft_epi_g / _bwd_g: two weight groups at stride wgs, wide C 12
    pytest.param((4, 12, 16, 40, 12), 2, 1, 1, id="grouped_wide_c12"),
]


def _rowinv_inputs(geom, G, seed):
    Bn, C, P1, P2, m2 = geom
    rng = np.random.default_rng(seed + sum(geom))
    Z = _crandn(rng, Bn, P1, m2, C, scale=0.3)
    x = _randn(rng, Bn, C, P1, P2)
    dz = _randn(rng, Bn, C, P1, P2)
    wb = _randn(rng, G, C * C + C, scale=0.4)                  # per group [wc (C x C) | bc (C)]
    wc = wb[:, :C * C].reshape(G, C, C).astype(np.float64)
    bc = wb[:, C * C:].astype(np.float64)
    idx = np.arange(Bn) // (Bn // G)
    return Z, x, dz, wb, wc[idx], bc[idx]                      # per-sample weights for the reference


def _zdev(Z, tiled):
    Zr = sr.ri(Z).astype(np.float32)
    return _dev(sr.tile_encode(Zr) if tiled else Zr)


@pytest.mark.parametrize("geom,G,rowfuse,tiled", ROWINV_CASES)
def test_rowinv_forward_vs_fp64(switches, geom, G, rowfuse, tiled):
    ops, call, _, ptr, query, sp = _api()
    Bn, C, P1, P2, m2 = geom
    Z, x, _, wb, wcn, bcn = _rowinv_inputs(geom, G, 400)
    assert query("blindno_spectrum_tile_layout", Bn, C, P1, P2, m2) == tiled == sr.tile_layout(Bn, C, P1, P2, m2)
    switches("blindno_set_rowfuse", rowfuse)
    Zd, xd, wd = _zdev(Z, tiled), _dev(x), _dev(wb)
    tb = ops.twiddle_rowinv(P2, m2, "cuda")
    bare, bare_abs = sr.row_inv_bare(Z, P2), sr.row_inv_bare_abs(Z, P2)
    for act in (0, 1):
        for has_wc in (True, False):
            out = Guarded(Bn * C * P1 * P2)
            a = (ptr(Zd), ptr(xd) if has_wc else None, ptr(wd) if has_wc else None,
                 ptr(wd[C * C:]) if has_wc else None, ptr(out.t), ptr(tb))
            if G == 1:
                call("blindno_rowidft_epi", *a, Bn, C, P1, P2, m2, act, sp())
            else:
                call("blindno_rowidft_epi_g", *a, G, C * C + C, Bn, C, P1, P2, m2, act, sp())
            torch.cuda.synchronize()
            assert out.margins_intact()
            kw = dict(x=x, wc=wcn, bc=bcn, act=act) if has_wc else {}
            ref = sr.row_inv(Z, P2, bare=bare, **kw)
            S, gw = sr.row_inv_abs(Z, P2, bare=bare_abs, **kw)
            # n = 2 m2 real products of the transform + C of the conv + the bias
            _ratio(f"rowidft_epi {geom} G={G} rowfuse={rowfuse} act={act} wc={has_wc}",
                   out.cpu().numpy().reshape(Bn, C, P1, P2), ref, S, 2 * m2 + C + 1, gw)


@pytest.mark.parametrize("geom,G,rowfuse,tiled", ROWINV_CASES)
def test_rowinv_adjoint_vs_fp64(switches, geom, G, rowfuse, tiled):
    ops, call, _, ptr, query, sp = _api()
    Bn, C, P1, P2, m2 = geom
    Gs, xs, dz, wb, wcn, _ = _rowinv_inputs(geom, G, 500)
    switches("blindno_set_rowfuse", rowfuse)
    Gd, xd, wd = _zdev(Gs, tiled), _dev(xs), _dev(wb)
    tb = ops.twiddle_rowinv(P2, m2, "cuda")
    bare, bare_abs = sr.row_inv_bare(Gs, P2), sr.row_inv_bare_abs(Gs, P2)
    n = 2 * m2 + C + 1                                         # transform + conv + the GELU' product
    label = f"rowidft_bwd {geom} G={G} rowfuse={rowfuse}"
    if G > 1:                                                  # the grouped entry: full fields only
        dzd = _dev(dz)
        for act in (0, 1):
            dx = Guarded(Bn * C * P1 * P2)
            call("blindno_rowidft_bwd_g", ptr(Gd), ptr(dzd), ptr(wd), ptr(xd), ptr(dx.t), ptr(tb), G,
                 C * C + C, Bn, C, P1, P2, m2, act, sp())
            torch.cuda.synchronize()
            assert dx.margins_intact()
            S, gw = sr.row_inv_adj_abs(Gs, P2, dz, wcn, xs, act, bare=bare_abs)
            _ratio(f"{label} act={act}", dx.cpu().numpy().reshape(Bn, C, P1, P2),
                   sr.row_inv_adj(Gs, P2, dz, wcn, xs, act, bare=bare), S, n, gw)
        return
    # dz crops: none; dN1 < P1 with dN2 % 4 != 0; on the rowfuse shapes also one in whole float4s
    crops = [None, (P1 - 3, P2 - 5 if (P2 - 5) % 4 else P2 - 6)]
    if rowfuse and C == 4 and m2 % 4 == 0 and P1 % 16 == 0 and P2 % 32 == 0:
        crops.append((P1 - 5, P2 - 8))
    assert crops[1][1] % 4 != 0
    for crop in crops:
        dN1, dN2 = crop if crop else (P1, P2)
        dzn = dz.copy()
        dzn[:, :, dN1:, :] = np.nan                            # never read outside the crop
        dzn[:, :, :, dN2:] = np.nan
        dzd = _dev(dzn)
        for act in (0, 1):
            for want_partial in ((False, True) if C <= 4 else (False,)):
                dx = Guarded(Bn * C * P1 * P2)
                nch = query("blindno_rowidft_bwd_nchunk", Bn, C, P1, P2, m2) if want_partial else 0
                part = Guarded(nch * (C * C + C)) if want_partial else None
                call("blindno_rowidft_bwd_crop", ptr(Gd), ptr(dzd), ptr(wd), ptr(xd), ptr(dx.t), ptr(tb),
                     ptr(part.t) if want_partial else None, Bn, C, P1, P2, m2, act, dN1, dN2, sp())
                torch.cuda.synchronize()
                assert dx.margins_intact()
                S, gw = sr.row_inv_adj_abs(Gs, P2, dz, wcn, xs, act, crop, bare=bare_abs)
                tag = f"{label} act={act} crop={crop} partial={want_partial}"
                _ratio(tag, dx.cpu().numpy().reshape(Bn, C, P1, P2),
                       sr.row_inv_adj(Gs, P2, dz, wcn, xs, act, crop, bare=bare), S, n, gw)
                if want_partial:
                    assert nch >= 1 and part.margins_intact()
                    got = part.cpu().double().numpy().reshape(nch, C * C + C).sum(0)
                    Sw, gww = sr.conv_wgrad_abs(dz, xs, act, crop)
                    # one product per point of the crop, summed per lane, wave, block and chunk
                    _ratio(tag + " dWc|dbc", got, sr.conv_wgrad(dz, xs, act, crop), Sw, Bn * dN1 * dN2, gww)
    # wc == NULL: the bare transform's adjoint (dz, xsrc unused)
    dx = Guarded(Bn * C * P1 * P2)
    call("blindno_rowidft_bwd", ptr(Gd), None, None, None, ptr(dx.t), ptr(tb), None, Bn, C, P1, P2, m2, 0, sp())
    torch.cuda.synchronize()
    assert dx.margins_intact()
    _ratio(f"{label} wc=NULL", dx.cpu().numpy().reshape(Bn, C, P1, P2), bare, bare_abs, 2 * m2)


# ================================================================================ whole layer
@pytest.mark.parametrize("geom", [(1, 32, 32, 24, 96, 12, 48), (2, 20, 24, 18, 34, 5, 17)])
def test_spectral_conv2d_op_at_the_limits(geom):
    """torch.ops.blindno.spectral_conv2d at the header's limits (C 32, m2 48) and with Ci != Co
    beyond 16 channels, forward and autograd, as test_gpu_torch_ops.test_spectral_conv2d_op:
    fp32 HIP vs the fp64 oracle, forward rel-L2 <= 1e-5, gradients <= 1e-4."""
    from blindno import torch_ops  # noqa: F401
    import oracle.fno_ref as ref
    Bn, Ci, Co, P1, P2, m1, m2 = geom
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(Bn, Ci, P1, P2, device="cuda", generator=g, requires_grad=True)
    w1 = (0.3 * torch.randn(Ci, Co, m1, m2, 2, device="cuda", generator=g)).requires_grad_(True)
    w2 = (0.3 * torch.randn(Ci, Co, m1, m2, 2, device="cuda", generator=g)).requires_grad_(True)
    y, _ = torch.ops.blindno.spectral_conv2d(x, w1, w2)
    xd, w1d, w2d = (t.detach().double().requires_grad_(True) for t in (x, w1, w2))
    yr = ref.spectral_conv2d(xd, w1d, w2d)
    err = lambda a, b: rel_l2(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    e = err(y, yr)
    cot = torch.randn_like(y)
    eg = [err(a, b) for a, b in zip(torch.autograd.grad(y, (x, w1, w2), cot),
                                    torch.autograd.grad(yr, (xd, w1d, w2d), cot.double()))]
    print(f"spectral_conv2d {geom}: fwd {e:.2e} grads {[f'{v:.2e}' for v in eg]}")
    assert e <= 1e-5
    assert max(eg) <= 1e-4


# ================================================================================ refusals
def _rc(name, *args):
    """The entry point's return code (no exception)."""
    from blindno._lib import load
    return int(getattr(load(), name)(*args))


def test_invalid_shapes_are_refused_on_the_host():
    """hipErrorInvalidValue from the host-side checks, nothing launched: every guarded output stays
    untouched.  (Buffers are sized for the nearest valid shape and never read.)"""
    ops, _, _, ptr, _, sp = _api()
    n = 1 << 16
    src = torch.zeros(n, device="cuda")
    o1, o2, o3 = Guarded(n), Guarded(n), Guarded(n)
    p = ptr(src)

    def epi(Bn, C, P1, P2, m2):
        return _rc("blindno_rowidft_epi", p, p, p, p, ptr(o1.t), p, Bn, C, P1, P2, m2, 0, sp())

    def bwd(Bn, C, P1, P2, m2, dN1, dN2, partial=None, act=0, wc=p):
        return _rc("blindno_rowidft_bwd_crop", p, p, wc, p, ptr(o1.t), p, partial, Bn, C, P1, P2, m2, act,
                   dN1, dN2, sp())

    def colpass(G, Bn, Ci, Co, P1, m1, m2, P2):
        return _rc("blindno_colpass_g", p, p, ptr(o1.t), ptr(o2.t), ptr(o3.t), p, p, G, 64, Bn, Ci, Co, P1, m1,
                   m2, P2, 0, sp())

    assert epi(1, 33, 4, 16, 4) == INVALID                          # C = 33
    assert bwd(1, 33, 4, 16, 4, 4, 16) == INVALID
    assert epi(1, 4, 4, 96, 49) == INVALID                          # m2 = 49
    assert bwd(1, 4, 4, 96, 49, 4, 96) == INVALID
    # m2 > P2/2 + 1: the row DFT, the column pass and the 1D mix
    assert _rc("blindno_rowdft", p, ptr(o1.t), p, 1, 4, 4, 16, 10, 0, sp()) == INVALID
    assert _rc("blindno_rowdft_crop", p, ptr(o1.t), p, 1, 4, 4, 16, 4, 0, 5, 16, sp()) == INVALID   # N1v > P1
    assert colpass(1, 2, 4, 4, 8, 2, 10, 16) == INVALID
    assert _rc("blindno_mix1d", p, p, ptr(o1.t), ptr(o2.t), 2, 4, 4, 10, 16, 0, sp()) == INVALID
    assert colpass(1, 2, 4, 4, 8, 9, 4, 16) == INVALID              # m1 > P1
    assert bwd(1, 4, 4, 16, 4, 4, 17) == INVALID                    # dN2 > P2
    assert bwd(1, 4, 4, 16, 4, 5, 16) == INVALID                    # dN1 > P1
    assert bwd(1, 5, 4, 16, 4, 4, 16, partial=ptr(o2.t)) == INVALID  # in-pass weight gradient, C > 4
    assert bwd(1, 4, 4, 16, 4, 4, 16, act=1, wc=None) == INVALID    # GELU' without the conv epilogue
    # G not dividing Bn
    assert colpass(2, 3, 4, 4, 8, 2, 4, 16) == INVALID
    assert _rc("blindno_rowidft_epi_g", p, p, p, p, ptr(o1.t), p, 2, 20, 3, 4, 4, 16, 4, 0, sp()) == INVALID
    assert _rc("blindno_rowidft_bwd_g", p, p, p, p, ptr(o1.t), p, 2, 20, 3, 4, 4, 16, 4, 0, sp()) == INVALID
    torch.cuda.synchronize()
    assert o1.untouched() and o2.untouched() and o3.untouched()
