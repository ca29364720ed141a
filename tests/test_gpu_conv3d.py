"""The 3D convolution kernels (csrc/conv3d.hip) against F.conv3d in fp64 (needs a GPU).

blindno_conv3d_{fwd,bwd_data,bwd_weight} replace nn.Conv3d in the NIOFP3D encoders' ConvBlock3D
(2d_FPE/Baselines.py:26-38).  The fp64 side runs on the CPU.  Bar (as
test_conv2d_matches_fp64): one convolution of fp32 data, rel-L2 <= 1e-5 for the output and for
dx, dW, db.  Outputs and split-K partials are prefilled with NaN, every split count in {1, 2, 3,
default} is checked against fp64, and a second call must be bit-identical.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


K3, S1, S2, P0, P1 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (0, 0, 0), (1, 1, 1)
# (N, Ci, D, H, W, Co, kernel, stride, pad)
CASES = [
    (5, 1, 33, 12, 12, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)),    # first block, Ci = 1
    (3, 64, 9, 6, 5, 128, K3, S2, P1),                          # odd extents
    (3, 128, 5, 3, 3, 128, K3, S1, P1),                         # stride 1
    (7, 512, 3, 1, 1, 512, K3, S2, P1),      # 7_1 / 7_2 shape: most taps in padding, split-K default
    (7, 512, 2, 1, 1, 512, (2, 1, 1), S1, P0),                  # 7_3: dense, 1-voxel output
    (7, 512, 1, 1, 1, 512, (1, 1, 1), S1, P0),                  # the _down variant's last block
    (3, 5, 7, 6, 5, 7, (3, 2, 3), (2, 3, 1), (1, 0, 2)),  # odd channels, mixed strides, stride > kernel
    (2, 16, 4, 4, 4, 200, K3, S1, P1),       # Co = 200: ragged last M tile and a ragged bias column
]


def _geom(case):
    N, Ci, D, H, W, Co, k, s, p = case
    return (N, Ci, D, H, W, Co, *k, *s, *p)


def _data(case, seed_off=0):
    N, Ci, D, H, W, Co, k, s, p = case
    torch.manual_seed(sum(_geom(case)) + seed_off)
    x = torch.randn(N, Ci, D, H, W, dtype=torch.float64)
    w = torch.randn(Co, Ci, *k, dtype=torch.float64) / (Ci * k[0] * k[1] * k[2]) ** 0.5
    b = torch.randn(Co, dtype=torch.float64)
    x64, w64, b64 = (t.clone().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv3d(x64, w64, b64, stride=s, padding=p)
    dy = torch.randn_like(y64)
    y64.backward(dy)
    return x, w, b, dy, y64.detach(), x64.grad, w64.grad, b64.grad


def _err(got, ref):
    return rel_l2(got.cpu().numpy(), ref.numpy())


@pytest.mark.parametrize("case", CASES)
def test_conv3d_matches_fp64(case):
    """ops.conv3d (autograd.Function over the default split counts): y, dx, dW, db vs fp64; a
    second forward + backward is bit-identical."""
    from blindno import ops
    N, Ci, D, H, W, Co, k, s, p = case
    x, w, b, dy, y64, dx64, dw64, db64 = _data(case)
    runs = []
    for _ in range(2):
        xs, ws, bs = (t.float().cuda().requires_grad_(True) for t in (x, w, b))
        y = ops.conv3d(xs, ws, bs, s, p)
        assert y.shape == y64.shape
        (y * dy.float().cuda()).sum().backward()
        runs.append((y.detach(), xs.grad, ws.grad, bs.grad))
    errs = [_err(g, r) for g, r in zip(runs[0], (y64, dx64, dw64, db64))]
    print(f"{case}: y {errs[0]:.2e} dx {errs[1]:.2e} dW {errs[2]:.2e} db {errs[3]:.2e}")
    for e in errs:
        assert e <= TOL, errs
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    if case[7] == (2, 3, 1):
        # stride 3 over a 2-tap kernel axis: input rows h = 2, 5 meet no tap, their dx is exactly 0
        assert torch.count_nonzero(dx64[:, :, :, 2::3]) == 0
        assert torch.count_nonzero(runs[0][1][:, :, :, 2::3]) == 0


@pytest.mark.parametrize("case", CASES)
def test_conv3d_split_k(case):
    """The three entries at explicit split counts (1, 2, 3 and each entry's default) with
    NaN-prefilled outputs and partials: each against fp64, each deterministic."""
    from blindno._lib import call, ptr, query, stream_ptr
    N, Ci, D, H, W, Co, k, s, p = case
    g = _geom(case)
    x, w, b, dy, y64, dx64, dw64, db64 = _data(case, 1)
    xs, ws, bs, dys = (t.float().cuda().contiguous() for t in (x, w, b, dy))
    ncol = Ci * k[0] * k[1] * k[2] + 1
    ref_wb = torch.cat([dw64.reshape(Co, -1), db64[:, None]], 1)
    defaults = [query(f"blindno_conv3d_{n}_nsplit", *g) for n in ("fwd", "bwd_data", "wgrad")]
    assert all(d >= 1 for d in defaults), defaults
    if case[1] == 512 and k == K3:
        assert defaults[0] > 1 and defaults[1] > 1, defaults   # the deep layers split by default
    for ns in sorted({1, 2, 3, *defaults}):
        outs = []
        for _ in range(2):
            y = torch.full(y64.shape, NAN, device="cuda")
            part = torch.full((ns, y.numel()), NAN, device="cuda")
            call("blindno_conv3d_fwd", ptr(xs), ptr(ws), ptr(bs), ptr(y), ptr(part), ns, *g, stream_ptr())
            dx = torch.full(x.shape, NAN, device="cuda")
            partd = torch.full((ns, dx.numel()), NAN, device="cuda")
            call("blindno_conv3d_bwd_data", ptr(dys), ptr(ws), ptr(dx), ptr(partd), ns, *g, stream_ptr())
            dwb = torch.full((Co, ncol), NAN, device="cuda")
            partw = torch.full((ns, dwb.numel()), NAN, device="cuda")
            call("blindno_conv3d_bwd_weight", ptr(dys), ptr(xs), ptr(dwb), ptr(partw), ns, *g, stream_ptr())
            outs.append((y, dx, dwb))
        torch.cuda.synchronize()
        y, dx, dwb = outs[0]
        errs = (_err(y, y64), _err(dx, dx64), _err(dwb[:, :-1], ref_wb[:, :-1]), _err(dwb[:, -1], ref_wb[:, -1]))
        print(f"{case} nsplit {ns}: y {errs[0]:.2e} dx {errs[1]:.2e} dW {errs[2]:.2e} db {errs[3]:.2e}")
        for t in (y, dx, dwb):
            assert torch.isfinite(t).all(), ns
        for e in errs:
            assert e <= TOL, (ns, errs)
        for a, c in zip(*outs):
            assert torch.equal(a, c), ns
    # no bias: b = NULL
    y = torch.full(y64.shape, NAN, device="cuda")
    call("blindno_conv3d_fwd", ptr(xs), ptr(ws), None, ptr(y), None, 1, *g, stream_ptr())
    assert _err(y, y64 - b.view(1, -1, 1, 1, 1)) <= TOL


def test_conv3d_rejects_bad_arguments():
    """NULL tensors, a zero size, an output extent of 0, a non-positive split count and (for the
    input gradient) more stride-phase classes than the table holds return an error and launch
    nothing: the sentinel-filled outputs, their margins included, stay untouched."""
    from blindno._lib import load, ptr, query, stream_ptr
    lib = load()
    case = (2, 3, 5, 4, 4, 6, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    N, Ci, D, H, W, Co, k, s, p = case
    g = list(_geom(case))
    M = 64                                     # margin floats on each side
    SENT = 777.0
    ny, nx, nw = N * Co * 3 * 2 * 2, N * Ci * D * H * W, Co * (Ci * 27 + 1)
    bufs = {n: torch.full((sz + 2 * M,), SENT, device="cuda") for n, sz in (("y", ny), ("dx", nx), ("dwb", nw))}
    part = torch.full((3 * max(ny, nx, nw),), SENT, device="cuda")
    x = torch.randn(nx, device="cuda")
    w = torch.randn(Co * Ci * 27, device="cuda")
    b = torch.randn(Co, device="cuda")
    dy = torch.randn(ny, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)   # noqa: E731
    st = stream_ptr()

    def with_(i, v):
        h = list(g)
        h[i] = v
        return h

    bad_geoms = [with_(0, 0), with_(1, 0), with_(5, 0), with_(2, 0), with_(6, 0), with_(9, 0), with_(12, -1),
                 with_(6, 9),                                     # KD = 9 > D + 2 pd: output depth 0
                 with_(8, 7)]                                     # KW = 7 > W + 2 pw: output width 0
    calls = []
    for h in bad_geoms:
        calls.append(("blindno_conv3d_fwd", (P(x), P(w), P(b), P(bufs["y"], M), P(part), 1, *h, st)))
        calls.append(("blindno_conv3d_bwd_data", (P(dy), P(w), P(bufs["dx"], M), P(part), 1, *h, st)))
        calls.append(("blindno_conv3d_bwd_weight", (P(dy), P(x), P(bufs["dwb"], M), P(part), 1, *h, st)))
        for q in ("fwd", "bwd_data", "wgrad"):
            assert query(f"blindno_conv3d_{q}_nsplit", *h) == -1, (q, h)
    # NULL tensors
    calls += [("blindno_conv3d_fwd", (None, P(w), P(b), P(bufs["y"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_fwd", (P(x), None, P(b), P(bufs["y"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_fwd", (P(x), P(w), P(b), None, P(part), 1, *g, st)),
              ("blindno_conv3d_fwd", (P(x), P(w), P(b), P(bufs["y"], M), None, 2, *g, st)),
              ("blindno_conv3d_bwd_data", (None, P(w), P(bufs["dx"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_data", (P(dy), None, P(bufs["dx"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_data", (P(dy), P(w), None, P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_data", (P(dy), P(w), P(bufs["dx"], M), None, 3, *g, st)),
              ("blindno_conv3d_bwd_weight", (None, P(x), P(bufs["dwb"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_weight", (P(dy), None, P(bufs["dwb"], M), P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_weight", (P(dy), P(x), None, P(part), 1, *g, st)),
              ("blindno_conv3d_bwd_weight", (P(dy), P(x), P(bufs["dwb"], M), None, 2, *g, st))]
    # non-positive split counts
    calls += [("blindno_conv3d_fwd", (P(x), P(w), P(b), P(bufs["y"], M), P(part), 0, *g, st)),
              ("blindno_conv3d_bwd_data", (P(dy), P(w), P(bufs["dx"], M), P(part), -1, *g, st)),
              ("blindno_conv3d_bwd_weight", (P(dy), P(x), P(bufs["dwb"], M), P(part), 0, *g, st))]
    # strides (3, 3, 1): 9 stride-phase classes, one more than the input gradient's table holds
    h = with_(9, 3)
    h[10] = 3
    h[11] = 1
    calls.append(("blindno_conv3d_bwd_data", (P(dy), P(w), P(bufs["dx"], M), P(part), 1, *h, st)))
    assert query("blindno_conv3d_bwd_data_nsplit", *h) == -1
    for name, args in calls:
        rc = getattr(lib, name)(*args)
        assert rc != 0, (name, args[4:])
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert bool((t == SENT).all()), n
    assert bool((part == SENT).all())
    # and the valid geometry still runs, leaving the margins alone
    rc = lib.blindno_conv3d_fwd(P(x), P(w), P(b), P(bufs["y"], M), P(part), 1, *g, st)
    assert rc == 0
    torch.cuda.synchronize()
    y = bufs["y"]
    assert bool((y[:M] == SENT).all()) and bool((y[-M:] == SENT).all())
    ref = F.conv3d(x.view(N, Ci, D, H, W).double().cpu(), w.view(Co, Ci, 3, 3, 3).double().cpu(), b.double().cpu(),
                   stride=s, padding=p)
    assert _err(y[M:-M].view(ref.shape), ref) <= TOL
