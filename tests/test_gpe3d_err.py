"""The record-free 3D GPE error path without a GPU: the two host-only queries of
include/blindno_gpe3d_err.h, gpe.time_averaged_L2_error_from_sums against the numpy checker, and the
request guards of gpe.solve_error_batch_3d.
"""
import os
import re

import numpy as np
import pytest
import torch

import gpe3d_ref
from conftest import ROOT

HDR = os.path.join(ROOT, "include", "blindno_gpe3d_err.h")
NAMES = ["blindno_gpe3d_error", "blindno_gpe3d_error_launches", "blindno_gpe3d_error_scratch_doubles"]


def _tile():
    m = re.search(r"^#define BLINDNO_GPE3D_ERR_TILE (\d+)\s*$", open(HDR).read(), re.M)
    return int(m.group(1))


def test_gpe3d_err_table_is_disjoint_from_every_other_table():
    from blindno import _lib
    own = _lib.ABI["blindno_gpe3d_err.h"]
    assert sorted(own) == NAMES and len(_lib.ABI) >= 8
    for k, v in _lib.ABI.items():
        if k != "blindno_gpe3d_err.h":
            assert not set(v) & set(own), k
    assert len(_lib.exported_symbols()) == len(set(_lib.exported_symbols()))


def test_tile_macro_is_a_power_of_two_in_range():
    T = _tile()
    assert 256 <= T <= 4096 and T & (T - 1) == 0


def test_host_only_queries():
    from blindno import _lib
    T = _tile()
    q = lambda *a: _lib.query("blindno_gpe3d_error_scratch_doubles", *a)   # noqa: E731
    assert q(6, 64, 64, 64) == 3 * 6 * 64 ** 3 + 2 * 6 * (64 ** 3 // T)
    assert q(1, 4, 4, 4) == 3 * 64 + 2                             # N below one tile: one tile
    assert q(2, 4, 8, 16) == 2 * (3 * 512 + 2 * max(1, 512 // T))
    assert q(1024, 256, 256, 256) == 1024 * (3 * 256 ** 3 + 2 * 256 ** 3 // T) > 2 ** 35
    for bad in [(0, 8, 8, 8), (1, 2, 8, 8), (1, 8, 2, 8), (1, 8, 8, 2), (1, 12, 8, 8), (1, 8, 12, 8), (1, 8, 8, 12),
                (1, 8, 8, 2048), (1, 2048, 4, 4), (1, 0, 8, 8), (1, 8, 8, -4), (1, 1024, 128, 256), (1, 512, 256, 256)]:
        assert q(*bad) == -1, bad
    n = lambda *a: _lib.query("blindno_gpe3d_error_launches", *a)          # noqa: E731
    assert n(1000, 2, 10) == 3000 + 202
    assert n(7, 4, 3) == 84 + 6
    assert n(0, 2, 1) == 3 and n(0, 4, 5) == 3
    assert n(1000, 2, 1) == 3000 + 2002 and n(7, 2, 100) == 21 + 2
    for bad in [(5, 3, 1), (5, 1, 1), (-1, 2, 1), (5, 2, 0), (5, 4, -3)]:
        assert n(*bad) == -1, bad
    for ns, order, re_ in [(1000, 2, 10), (7, 4, 3), (0, 2, 1)]:
        assert n(ns, order, re_) == _lib.query("blindno_gpe3d_launches", ns, order) + 2 * (ns // re_ + 1)


def test_time_averaged_L2_error_from_sums_matches_the_checker():
    """Seeded sums, and fields whose numpy.trapz integrals are those sums exactly: on the grid
    {0, 1}^3 the triple trapezoid of a constant c^2 is c^2 (every step is (c^2 + c^2) / 2 * 1), and
    with c and the offset d multiples of 2^-10 below 2^10 the squares, c + d and (c + d) - c are all
    exact.  Both sides then form sqrt(num) / (sqrt(den) + eps) from the same numbers with the same
    correctly rounded operations, and 0.5 (r_i + r_{i+1}) (t_{i+1} - t_i) likewise (the halving is
    exact).  What may differ is the order of the sum of the nt - 1 = 3 terms.  Each side's result is
    the exact value of sum / (t_end - t_0) on those terms after three roundings (two additions, one
    division), so each is within 3 * 2^-53 of it, relative, and the two within 3 * 2^-52 of each
    other."""
    from blindno import gpe
    rs = np.random.RandomState(17)
    g = np.array([0.0, 1.0])
    for trial in range(20):
        nt = 4
        c = rs.randint(1, 1 << 20, nt) / 1024.0
        d = rs.randint(0, 1 << 20, nt) / 1024.0
        d[rs.randint(nt)] = 0.0                                   # a frame with no error at all
        num, den = d * d, c * c
        t = np.cumsum(rs.randint(1, 1 << 10, nt) / 256.0)
        ref = np.broadcast_to(c[:, None, None, None], (nt, 2, 2, 2))
        pred = np.broadcast_to((c + d)[:, None, None, None], (nt, 2, 2, 2))
        trapz = getattr(np, "trapezoid", None) or np.trapz
        i3 = lambda f: trapz(trapz(trapz(f, g, axis=1), g, axis=1), g, axis=1)   # noqa: E731
        assert np.array_equal(i3((pred - ref) ** 2), num) and np.array_equal(i3(ref ** 2), den)
        want = gpe3d_ref.time_averaged_L2_error(t, ref, pred, g, g, g)
        got = gpe.time_averaged_L2_error_from_sums(t, torch.from_numpy(num), torch.from_numpy(den))
        assert isinstance(got, float) and abs(got - want) <= 3 * 2.0 ** -52 * abs(want), (trial, got, want)
        assert gpe.time_averaged_L2_error_from_sums(t, num, den) == got       # arrays as well as tensors
    # a sum that rounding pushed below zero counts as zero
    assert gpe.time_averaged_L2_error_from_sums(t, -num, den) == 0.0
    # eps enters the denominator
    assert gpe.time_averaged_L2_error_from_sums(t, num, 0 * den, eps=2.0) == \
        gpe.time_averaged_L2_error_from_sums(t, num, 0 * den + 1.0, eps=1.0)


def test_solve_error_batch_3d_refusals_come_before_the_device(monkeypatch):
    """Over-budget launches, over-budget scratch and a batch that is not whole groups are refused
    before anything touches the device (device='cpu' raises the no-CPU-path error next)."""
    from blindno import gpe
    from blindno._lib import BlindnoError, query
    x = np.linspace(-10, 10, 8)
    V = np.zeros((4, 8, 8, 8))
    p = np.ones((8, 8, 8), complex)
    # one frame (rec_every above nsteps): 3 nsteps + 2 launches
    steps = (gpe.MAX_LAUNCHES_3D - 2) // 3
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_3d(p, x, x, x, 1.0, steps + 0.5, 2, 1, 1, V, rec_every=1 << 30, device="cpu")
    with pytest.raises(BlindnoError, match=r"MAX_LAUNCHES_3D.*refusing to launch"):
        gpe.solve_error_batch_3d(p, x, x, x, 1.0, steps + 1.5, 2, 1, 1, V, rec_every=1 << 30, device="cpu")
    # the reductions count: 250000 Strang steps are 750000 launches of the solver, inside its limit, and
    # 1250002 with every step reduced
    assert query("blindno_gpe3d_launches", 250000, 2) < gpe.MAX_LAUNCHES_3D
    with pytest.raises(BlindnoError, match=r"MAX_LAUNCHES_3D.*refusing to launch"):
        gpe.solve_error_batch_3d(p, x, x, x, 1.0, 250000.5, 2, 1, 1, V, device="cpu")
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_3d(p, x, x, x, 1.0, 250000.5, 2, 1, 1, V, rec_every=10, device="cpu")
    # scratch: 3 B N + 2 B tiles doubles
    need = 8 * query("blindno_gpe3d_error_scratch_doubles", 4, 8, 8, 8)
    assert need == 8 * 4 * (3 * 512 + 2)
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", need - 1)
    with pytest.raises(BlindnoError, match=r"MAX_RECORD_BYTES.*refusing to launch"):
        gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, 2, 1, 1, V, device="cpu")
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", need)
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, 2, 1, 1, V, device="cpu")
    # the scratch does not grow with the number of frames
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_3d(p, x, x, x, 0.001, 100.0, 2, 1, 1, V, device="cpu")
    for group in (3, 0, -1, 8):
        with pytest.raises(BlindnoError, match="whole groups"):
            gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, 2, 1, 1, V, group=group, device="cpu")
    for group in (None, 1, 2, 4):
        with pytest.raises(BlindnoError, match="no CPU path"):
            gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, 2, 1, 1, V, group=group, device="cpu")
    # solve_batch_3d's own argument checks
    for kw, pat in [(dict(order=3), "order"), (dict(rec_every=0), "rec_every")]:
        a = dict(order=2, rec_every=1)
        a.update(kw)
        with pytest.raises(BlindnoError, match=pat):
            gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, a["order"], 1, 1, V, rec_every=a["rec_every"], device="cpu")
    with pytest.raises(BlindnoError, match="power of two"):
        xs = np.linspace(-1, 1, 12)
        gpe.solve_error_batch_3d(np.ones((12, 8, 8), complex), xs, x, x, 0.1, 1.0, 2, 1, 1, np.zeros((12, 8, 8)),
                                 device="cpu")
    with pytest.raises(BlindnoError, match="V has shape"):
        gpe.solve_error_batch_3d(p, x, x, x, 0.1, 1.0, 2, 1, 1, np.zeros((8, 8)), device="cpu")
