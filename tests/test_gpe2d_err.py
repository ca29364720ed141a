"""The record-free 2D GPE error path without a GPU: the two host-only queries of
include/blindno_gpe2d_err.h, and the request guards of gpe.solve_error_batch_2d.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "blindno_gpe2d_err.h")
NAMES = ["blindno_gpe2d_error", "blindno_gpe2d_error_launches", "blindno_gpe2d_error_scratch_doubles"]


def _tile():
    m = re.search(r"^#define BLINDNO_GPE2D_ERR_TILE (\d+)\s*$", open(HDR).read(), re.M)
    return int(m.group(1))


def test_gpe2d_header_still_declares_four_entries():
    """The new entries live in their own header: blindno_gpe2d.h keeps its four."""
    from blindno import _lib
    hdr = open(os.path.join(ROOT, "include", "blindno_gpe2d.h")).read()
    decl = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(blindno_\w+)\(", hdr, re.M)))
    assert decl == sorted(_lib.ABI["blindno_gpe2d.h"]) and len(decl) == 4
    assert not re.findall(r"blindno_gpe2d_error", hdr)


def test_gpe2d_err_table_is_disjoint_from_every_other_table():
    from blindno import _lib
    own = _lib.ABI["blindno_gpe2d_err.h"]
    assert sorted(own) == NAMES and len(_lib.ABI) >= 9
    for k, v in _lib.ABI.items():
        if k != "blindno_gpe2d_err.h":
            assert not set(v) & set(own), k
    assert len(_lib.exported_symbols()) == len(set(_lib.exported_symbols()))
    assert set(own) <= set(_lib.exported_symbols())


def test_tile_macro_is_a_power_of_two_in_range():
    T = _tile()
    assert 256 <= T <= 4096 and T & (T - 1) == 0 and T == 1024


def test_host_only_queries():
    from blindno import _lib
    q = lambda *a: _lib.query("blindno_gpe2d_error_scratch_doubles", *a)   # noqa: E731
    for B in (1, 6):
        for nx, ny in [(4, 4), (32, 32), (64, 32), (1024, 512)]:
            N = nx * ny
            assert q(B, nx, ny) == 3 * B * N + 2 * B * max(1, N // 1024), (B, nx, ny)
    assert q(1, 4, 4) == 3 * 16 + 2                                # N below one tile: one tile
    assert q(4096, 1024, 1024) == 4096 * (3 * 1024 * 1024 + 2 * 1024) > 2 ** 33
    for bad in [(1, 12, 8), (1, 4, 2), (1, 2048, 4), (0, 8, 8), (1, 2, 8), (1, 8, 12), (1, 8, 2048), (1, 0, 8),
                (1, 8, -4), (-1, 8, 8)]:
        assert q(*bad) == -1, bad
    n = lambda *a: _lib.query("blindno_gpe2d_error_launches", *a)          # noqa: E731
    for ns, order, re_ in [(1000, 2, 10), (7, 4, 3), (0, 2, 1), (0, 4, 5), (1000, 2, 1), (7, 2, 100), (6, 4, 3)]:
        assert n(ns, order, re_) == _lib.query("blindno_gpe2d_launches", ns, order) + 2 * (ns // re_ + 1)
    assert n(1000, 2, 10) == 2000 + 202
    assert n(7, 4, 3) == 56 + 6
    assert n(0, 2, 1) == 3 and n(0, 4, 5) == 3
    for bad in [(5, 3, 1), (5, 1, 1), (5, 2, 0), (-1, 2, 1), (5, 4, -3)]:
        assert n(*bad) == -1, bad


def test_solve_error_batch_2d_refusals_come_before_the_device(monkeypatch):
    """Over-budget launches, over-budget scratch and a batch that is not whole groups are refused
    before anything touches the device (device='cpu' raises the no-CPU-path error next)."""
    from blindno import gpe
    from blindno._lib import BlindnoError, query
    x = np.linspace(-10, 10, 8)
    V = np.zeros((4, 8, 8))
    p = np.ones((8, 8), complex)
    # one frame (rec_every above nsteps): 2 nsteps + 2 launches
    steps = (gpe.MAX_LAUNCHES_2D - 2) // 2
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_2d(p, x, x, 1.0, steps + 0.5, 2, 1, 1, V, rec_every=1 << 30, device="cpu")
    with pytest.raises(BlindnoError, match=r"MAX_LAUNCHES_2D.*refusing to launch"):
        gpe.solve_error_batch_2d(p, x, x, 1.0, steps + 1.5, 2, 1, 1, V, rec_every=1 << 30, device="cpu")
    # the reductions count: 600000 Strang steps are 1200000 launches of the solver, inside its limit, and
    # 2400002 with every step reduced
    assert query("blindno_gpe2d_launches", 600000, 2) < gpe.MAX_LAUNCHES_2D
    with pytest.raises(BlindnoError, match=r"MAX_LAUNCHES_2D.*refusing to launch"):
        gpe.solve_error_batch_2d(p, x, x, 1.0, 600000.5, 2, 1, 1, V, device="cpu")
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_2d(p, x, x, 1.0, 600000.5, 2, 1, 1, V, rec_every=10, device="cpu")
    # scratch: 3 B N + 2 B tiles doubles; the message names the grid and the limit
    need = 8 * query("blindno_gpe2d_error_scratch_doubles", 4, 8, 8)
    assert need == 8 * 4 * (3 * 64 + 2)
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", need - 1)
    with pytest.raises(BlindnoError, match=rf"8 x 8 .*MAX_RECORD_BYTES = {need - 1}\b.*refusing to launch"):
        gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, 2, 1, 1, V, device="cpu")
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", need)
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, 2, 1, 1, V, device="cpu")
    # the scratch does not grow with the number of frames
    with pytest.raises(BlindnoError, match="no CPU path"):
        gpe.solve_error_batch_2d(p, x, x, 0.001, 100.0, 2, 1, 1, V, device="cpu")
    for group in (3, 0, -1, 8):
        with pytest.raises(BlindnoError, match="whole groups"):
            gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, 2, 1, 1, V, group=group, device="cpu")
    for group in (None, 1, 2, 4):
        with pytest.raises(BlindnoError, match="no CPU path"):
            gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, 2, 1, 1, V, group=group, device="cpu")
    # solve_batch_2d's own argument checks
    for kw, pat in [(dict(order=3), "order"), (dict(rec_every=0), "rec_every")]:
        a = dict(order=2, rec_every=1)
        a.update(kw)
        with pytest.raises(BlindnoError, match=pat):
            gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, a["order"], 1, 1, V, rec_every=a["rec_every"], device="cpu")
    with pytest.raises(BlindnoError, match="power of two"):
        xs = np.linspace(-1, 1, 12)
        gpe.solve_error_batch_2d(np.ones((12, 8), complex), xs, x, 0.1, 1.0, 2, 1, 1, np.zeros((12, 8)), device="cpu")
    with pytest.raises(BlindnoError, match="V has shape"):
        gpe.solve_error_batch_2d(p, x, x, 0.1, 1.0, 2, 1, 1, np.zeros((8,)), device="cpu")
    with pytest.raises(BlindnoError, match="batch sizes differ"):
        gpe.solve_error_batch_2d(np.ones((3, 8, 8), complex), x, x, 0.1, 1.0, 2, 1, 1, V, device="cpu")


def test_compute_time_error_gpe_2d_takes_record_free_and_defaults_to_the_record():
    import inspect
    from blindno import timeerror
    p = inspect.signature(timeerror.compute_time_error_gpe_2d).parameters
    assert p["record_free"].default is False and list(p)[-1] == "record_free"
