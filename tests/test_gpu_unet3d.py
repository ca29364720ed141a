"""PermInvUNet_attn3D on the HIP device (needs a GPU): the kernels of csrc/unet3d.hip through the
C ABI on sentinel-guarded buffers, the model, and the trainer's 3d_FPE unet experiment, against the
float64 restatements of tests/unet3d_ref.py (pinned to torch.nn.functional by
tests/test_unet3d_ref.py).

Bars, those of tests/test_gpu_unet.py: one fp32 kernel, rel-L2 <= 1e-5 against fp64; gradients
max(1e-5, 3 x fp32 torch's own distance from fp64); the model's forward max(1e-5, 3 x the fp32
envelope) and its gradients unet_grad_bar of the envelope (the float64 model in fp32, unperturbed
and under three float32-rounding-sized input perturbations).
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

import unet3d_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENT = 777.0
M = 64                      # guard elements on each side of an output
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


class Guarded:
    """An output of n elements between two sentinel margins; the interior starts as NaN (uint8:
    255), so an element the kernel leaves unwritten shows."""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, n = shape, int(np.prod(shape))
        fill = SENT if dtype.is_floating_point else 99
        self.buf = torch.full((n + 2 * M,), fill, device="cuda", dtype=dtype)
        self.buf[M:M + n] = float("nan") if dtype.is_floating_point else 255
        self.fill, self.n = fill, n
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + M * self.buf.element_size())

    def sentinel(self):
        self.buf[:] = self.fill
        return self

    def get(self):
        assert bool((self.buf[:M] == self.fill).all()) and bool((self.buf[M + self.n:] == self.fill).all())
        return self.buf[M:M + self.n].view(*self.shape)

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _dev(t):
    return t.float().cuda().contiguous()


def _err(got, ref):
    return rel_l2(got.detach().double().cpu().numpy(), ref.detach().numpy())


def _api():
    from blindno._lib import load, ptr, query, stream_ptr
    return load(), ptr, query, stream_ptr()


# ---------------------------------------------------------------------------------- dwconv3d

_DW = {}


def _dw_data(key, case):
    """(x, w, b, g, y64, dx64, dwb64, fp32 torch's distances from fp64) -- computed once per case."""
    if key not in _DW:
        N, C, D, H, W, k, bias = case
        torch.manual_seed(sum(case[:5]) + sum(k))
        x = torch.randn(N, C, D, H, W, dtype=F64)
        w = torch.randn(C, 1, *k, dtype=F64) / math.sqrt(k[0] * k[1] * k[2])
        b = torch.randn(C, dtype=F64) if bias else None
        g = torch.randn(N, C, D, H, W, dtype=F64)
        x, w, g = (t.float().double() for t in (x, w, g))
        b = b.float().double() if bias else None
        leaf = [t.clone().requires_grad_(True) for t in (x, w)] + ([b.clone().requires_grad_(True)] if bias else [])
        y = R.dwconv3d(*leaf)
        (y * g).sum().backward()
        db = leaf[2].grad if bias else g.sum((0, 2, 3, 4))
        dwb = torch.cat([leaf[1].grad.reshape(C, -1), db[:, None]], 1)
        l32 = [t.float().requires_grad_(True) for t in (x, w)] + ([b.float().requires_grad_(True)] if bias else [])
        y32 = F.conv3d(*l32, *([] if bias else [None]), padding=tuple(e // 2 for e in k), groups=C)
        (y32 * g.float()).sum().backward()
        db32 = l32[2].grad if bias else g.float().sum((0, 2, 3, 4))
        dwb32 = torch.cat([l32[1].grad.reshape(C, -1), db32[:, None]], 1)
        e32 = (_err(l32[0].grad, leaf[0].grad), _err(dwb32, dwb))
        _DW[key] = (x, w, b, g, y.detach(), leaf[0].grad, dwb, e32)
    return _DW[key]


def _dw_calls(case, data, nsplit=None):
    lib, ptr, query, st = _api()
    N, C, D, H, W, k, bias = case
    x, w, b, g = data[:4]
    geom = (N, C, D, H, W, *k)
    T = k[0] * k[1] * k[2]
    xs, ws, gs = _dev(x), _dev(w), _dev(g)
    bs = _dev(b) if bias else None
    ns = nsplit or query("blindno_dwconv3d_wgrad_nsplit", *geom)
    assert ns >= 1
    y, dx, dwb = Guarded(N, C, D, H, W), Guarded(N, C, D, H, W), Guarded(C, T + 1)
    part = Guarded(ns, C, T + 1)
    assert lib.blindno_dwconv3d_fwd(ptr(xs), ptr(ws), ptr(bs), y.ptr, *geom, st) == 0
    assert lib.blindno_dwconv3d_bwd_data(ptr(gs), ptr(ws), dx.ptr, *geom, st) == 0
    assert lib.blindno_dwconv3d_bwd_weight(ptr(gs), ptr(xs), dwb.ptr, part.ptr if ns > 1 else None, ns, *geom, st) == 0
    torch.cuda.synchronize()
    if ns > 1:
        assert torch.isfinite(part.get()).all()
    else:
        part.get()                                   # margins; the interior is not used
    return y.get(), dx.get(), dwb.get(), ns


@pytest.mark.parametrize("name", list(R.DW_CASES))
def test_dwconv3d(name):
    case = R.DW_CASES[name]
    data = _dw_data(name, case)
    y64, dx64, dwb64, e32 = data[4:]
    y, dx, dwb, ns = _dw_calls(case, data)
    errs = (_err(y, y64), _err(dx, dx64), _err(dwb, dwb64))
    bars = (TOL, max(TOL, 3 * e32[0]), max(TOL, 3 * e32[1]))
    print(f"dwconv3d {name} nsplit {ns}: y {errs[0]:.2e} dx {errs[1]:.2e} dwb {errs[2]:.2e} (bars {bars})")
    for t in (y, dx, dwb):
        assert torch.isfinite(t).all()
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    again = _dw_calls(case, data)
    assert all(torch.equal(a, c) for a, c in zip((y, dx, dwb), again[:3]))


def test_dwconv3d_wgrad_forced_splits():
    case = R.DW_WGRAD_CASE
    data = _dw_data("wgrad", case)
    dwb64, e32 = data[6], data[7]
    bar = max(TOL, 3 * e32[1])
    for ns in R.DW_WGRAD_SPLITS:
        a = _dw_calls(case, data, nsplit=ns)
        c = _dw_calls(case, data, nsplit=ns)
        e = _err(a[2], dwb64)
        print(f"dwconv3d wgrad nsplit {ns}: dwb {e:.2e} (bar {bar:.2e})")
        assert a[3] == ns and torch.isfinite(a[2]).all() and e <= bar, (ns, e, bar)
        assert torch.equal(a[2], c[2]), ns


# ---------------------------------------------------------------------------------- maxpool3d

def _pool_calls(x, k):
    lib, ptr, query, st = _api()
    N, C, D, H, W = x.shape
    out = (N, C, D // k[0], H // k[1], W // k[2])
    xs = _dev(x)
    y, arg = Guarded(*out), Guarded(*out, dtype=torch.uint8)
    assert lib.blindno_maxpool3d_fwd(ptr(xs), y.ptr, arg.ptr, N * C, D, H, W, *k, st) == 0
    torch.cuda.synchronize()
    return y.get(), arg.get()


def _pool_bwd(g, arg, shape, k):
    lib, ptr, query, st = _api()
    N, C, D, H, W = shape
    gs = _dev(g)
    dx = Guarded(*shape)
    assert lib.blindno_maxpool3d_bwd(ptr(gs), ptr(arg.contiguous()), dx.ptr, N * C, D, H, W, *k, st) == 0
    torch.cuda.synchronize()
    return dx.get()


@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_maxpool3d(name):
    N, C, D, H, W, k = R.POOL_CASES[name]
    torch.manual_seed(3)
    x = torch.randn(N, C, D, H, W, dtype=F64).float().double()
    x[0, 0, :2, :2, :2] = 1.5                       # a tie inside one window
    xr = x.clone().requires_grad_(True)
    yr, ar = R.maxpool3d(xr, k)
    g = torch.randn(yr.shape, dtype=F64).float().double()
    (yr * g).sum().backward()
    y, arg = _pool_calls(x, k)
    assert torch.equal(y.double().cpu(), yr.detach())
    assert torch.equal(arg.cpu().long(), ar)
    dx = _pool_bwd(g, arg, x.shape, k)
    assert torch.equal(dx.double().cpu(), xr.grad)
    # every dy lands on exactly one voxel: the sums agree to the rounding of an fp64 sum of fp32 values
    assert abs(float(dx.double().sum()) - float(g.sum())) <= 1e-12 * float(g.abs().sum())
    if name == "floor":
        assert tuple(y.shape[2:]) == (2, 3, 4)
        assert float(dx[:, :, 4].abs().max()) == 0 and float(dx[:, :, :, 6].abs().max()) == 0 and \
            float(dx[..., 8].abs().max()) == 0


def test_maxpool3d_constant_input_and_nan():
    k = (2, 2, 2)
    x = torch.full((1, 2, 4, 4, 5), 0.25, dtype=F64)
    y, arg = _pool_calls(x, k)
    assert bool((arg == 0).all()) and bool((y == 0.25).all())
    g = torch.randn(1, 2, 2, 2, 2, dtype=F64).float().double()
    dx = _pool_bwd(g, arg, x.shape, k).double().cpu()
    want = torch.zeros_like(x)
    want[:, :, 0:4:2, 0:4:2, 0:4:2] = g             # tap 0 of every window, nothing elsewhere
    assert torch.equal(dx, want)
    x = torch.randn(1, 1, 2, 4, 4, dtype=F64).float().double()
    x[0, 0, 1, 0, 1] = float("nan")                 # window (0, 0, 0), tap (1, 0, 1) = 5; a larger value follows
    x[0, 0, 1, 1, 1] = 50.0
    y, arg = _pool_calls(x, k)
    assert math.isnan(float(y[0, 0, 0, 0, 0])) and int(arg[0, 0, 0, 0, 0]) == 5
    yr, ar = R.maxpool3d(x, k)
    assert torch.equal(arg.cpu().long(), ar)
    assert torch.equal(torch.nan_to_num(y.double().cpu(), nan=7e7), torch.nan_to_num(yr, nan=7e7))


# ---------------------------------------------------------------------------------- convt3d

def test_convt3d():
    lib, ptr, query, st = _api()
    N, Ci, Co, di, do = R.CONVT_CASE
    torch.manual_seed(4)
    x = torch.randn(N, Ci, *di, dtype=F64).float().double()
    w = (torch.randn(Ci, Co, 2, 2, 2, dtype=F64) * 0.3).float().double()
    b = torch.randn(Co, dtype=F64).float().double()
    leaf = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = R.convt3d(*leaf, do)
    g = torch.randn(yr.shape, dtype=F64).float().double()
    (yr * g).sum().backward()
    l32 = [t.float().requires_grad_(True) for t in (x, w, b)]
    y32 = F.conv_transpose3d(*l32, stride=2, output_padding=tuple(o - 2 * i for o, i in zip(do, di)))
    (y32 * g.float()).sum().backward()
    geom = (N, Ci, *di, Co, *do)
    E = Ci * Co * 8 + Co
    nparts = query("blindno_convt3d_wgrad_nparts", N, *di)
    assert nparts == N * 1
    xs, ws, bs, gs = _dev(x), _dev(w), _dev(b), _dev(g)
    runs = []
    for _ in range(2):
        y, dx, dwb, part = Guarded(N, Co, *do), Guarded(N, Ci, *di), Guarded(E), Guarded(nparts, E)
        assert lib.blindno_convt3d_fwd(ptr(xs), ptr(ws), ptr(bs), y.ptr, *geom, st) == 0
        assert lib.blindno_convt3d_bwd_data(ptr(gs), ptr(ws), dx.ptr, *geom, st) == 0
        assert lib.blindno_convt3d_bwd_weight(ptr(gs), ptr(xs), dwb.ptr, part.ptr, *geom, st) == 0
        torch.cuda.synchronize()
        part.get()
        runs.append((y.get(), dx.get(), dwb.get()))
    y, dx, dwb = runs[0]
    assert all(torch.equal(a, c) for a, c in zip(*runs))
    # the output_padding planes hold the bias exactly
    assert torch.equal(y[:, :, 4], bs.view(1, Co, 1, 1).expand(N, Co, do[1], do[2]))
    assert torch.equal(y[..., 8], bs.view(1, Co, 1, 1).expand(N, Co, do[0], do[1]))
    ref = (yr.detach(), leaf[0].grad, leaf[1].grad.reshape(-1), leaf[2].grad)
    got = (y, dx, dwb[:E - Co], dwb[E - Co:])
    r32 = (None, l32[0].grad, l32[1].grad.reshape(-1), l32[2].grad)
    for i, (a, r, s) in enumerate(zip(got, ref, r32)):
        bar = TOL if s is None else max(TOL, 3 * _err(s, r))
        assert torch.isfinite(a).all() and _err(a, r) <= bar, (i, _err(a, r), bar)


# ---------------------------------------------------------------------------------- refusals

def test_bad_arguments_are_refused_and_nothing_is_written():
    lib, ptr, query, st = _api()
    N, C, D, H, W = 2, 2, 4, 5, 6
    n = N * C * D * H * W
    x = torch.randn(n, device="cuda")
    w = torch.randn(C * 9 * 9 * 9, device="cuda")
    b = torch.randn(C, device="cuda")
    out = Guarded(8 * n).sentinel()
    arg = Guarded(n, dtype=torch.uint8).sentinel()
    part = Guarded(8 * n).sentinel()
    P = ptr
    g = (N, C, D, H, W)
    calls = []
    for k in [(7, 7, 4), (2, 7, 7), (7, 9, 7), (9, 9, 9), (7, 0, 7)]:          # even, 9, < 1
        calls += [("blindno_dwconv3d_fwd", (P(x), P(w), P(b), out.ptr, *g, *k, st)),
                  ("blindno_dwconv3d_bwd_data", (P(x), P(w), out.ptr, *g, *k, st)),
                  ("blindno_dwconv3d_bwd_weight", (P(x), P(x), out.ptr, part.ptr, 2, *g, *k, st))]
        assert query("blindno_dwconv3d_wgrad_nsplit", *g, *k) == -1
    k = (7, 7, 7)
    calls += [("blindno_dwconv3d_fwd", (None, P(w), P(b), out.ptr, *g, *k, st)),                  # NULL x
              ("blindno_dwconv3d_fwd", (P(x), None, P(b), out.ptr, *g, *k, st)),
              ("blindno_dwconv3d_fwd", (P(x), P(w), P(b), out.ptr, 0, C, D, H, W, *k, st)),
              ("blindno_dwconv3d_fwd", (P(x), P(w), P(b), out.ptr, N, C, D, 0, W, *k, st)),
              ("blindno_dwconv3d_bwd_data", (None, P(w), out.ptr, *g, *k, st)),
              ("blindno_dwconv3d_bwd_weight", (None, P(x), out.ptr, part.ptr, 2, *g, *k, st)),
              ("blindno_dwconv3d_bwd_weight", (P(x), P(x), out.ptr, None, 2, *g, *k, st)),       # split, no partials
              ("blindno_dwconv3d_bwd_weight", (P(x), P(x), out.ptr, part.ptr, 0, *g, *k, st)),
              ("blindno_maxpool3d_fwd", (None, out.ptr, arg.ptr, N * C, D, H, W, 2, 2, 2, st)),
              ("blindno_maxpool3d_fwd", (P(x), out.ptr, arg.ptr, N * C, D, H, W, 2, 3, 2, st)),
              ("blindno_maxpool3d_fwd", (P(x), out.ptr, arg.ptr, N * C, 1, H, W, 2, 2, 2, st)),
              ("blindno_maxpool3d_bwd", (P(x), None, out.ptr, N * C, D, H, W, 2, 2, 2, st)),
              ("blindno_maxpool3d_bwd", (P(x), arg.ptr, out.ptr, N * C, D, H, W, 0, 2, 2, st))]
    # transposed convolution: Do outside [2 Di, 2 Di + 2), likewise Ho, Wo; NULL x
    ci, co, di = 2, 2, (2, 3, 2)
    for do in [(3, 6, 4), (6, 6, 4), (4, 5, 4), (4, 6, 6)]:
        cg = (N, ci, *di, co, *do)
        calls += [("blindno_convt3d_fwd", (P(x), P(w), P(b), out.ptr, *cg, st)),
                  ("blindno_convt3d_bwd_data", (P(x), P(w), out.ptr, *cg, st)),
                  ("blindno_convt3d_bwd_weight", (P(x), P(x), out.ptr, part.ptr, *cg, st))]
    cg = (N, ci, *di, co, 5, 6, 4)
    calls += [("blindno_convt3d_fwd", (None, P(w), P(b), out.ptr, *cg, st)),
              ("blindno_convt3d_bwd_data", (P(x), None, out.ptr, *cg, st)),
              ("blindno_convt3d_bwd_weight", (P(x), P(x), out.ptr, None, *cg, st))]
    for name, args in calls:
        assert getattr(lib, name)(*args) != 0, (name, args[3:])
    torch.cuda.synchronize()
    assert out.untouched() and arg.untouched() and part.untouched()
    # the valid geometry still runs and stays inside its buffer
    y = Guarded(N, co, 5, 6, 4)
    assert lib.blindno_convt3d_fwd(P(x), P(w), P(b), y.ptr, *cg, st) == 0
    torch.cuda.synchronize()
    ref = R.convt3d(x[:N * ci * 12].view(N, ci, *di).double().cpu(), w[:ci * co * 8].view(ci, co, 2, 2, 2).double().cpu(),
                    b.double().cpu(), (5, 6, 4))
    assert _err(y.get(), ref) <= TOL


# ---------------------------------------------------------------------------------- model

_MODEL = {}


def _model_case():
    """The model case with its float64 reference and fp32 envelope -- computed once."""
    if not _MODEL:
        import blindno
        c = R.MODEL
        torch.manual_seed(7)
        m = blindno.PermInvUNet_attn3D(1, 2, c["base_ch"], c["depth"], c["input_size"], width=c["width"],
                                       modes=c["modes"])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        x = torch.randn(c["B"], c["T"], *c["input_size"])
        cot = torch.randn(c["B"], *c["input_size"], 2)
        o64, g64 = R.run_model(state, x, cot, c["depth"], c["bag"])
        env_o, env_g = 0.0, {}
        for seed in (None, 1, 2, 3):
            o32, g32 = R.run_model(state, x, cot, c["depth"], c["bag"], dtype=torch.float32, perturb=seed)
            env_o = max(env_o, rel_l2(o32.numpy(), o64.numpy()))
            for k in g64:
                env_g[k] = max(env_g.get(k, 0.0), rel_l2(g32[k].numpy(), g64[k].numpy()))
        _MODEL.update(state=state, x=x, cot=cot, o64=o64, g64=g64, env_o=env_o, env_g=env_g)
    return _MODEL


def _device_model(train=True):
    import blindno
    c, mc = R.MODEL, _model_case()
    m = blindno.PermInvUNet_attn3D(1, 2, c["base_ch"], c["depth"], c["input_size"], width=c["width"],
                                   modes=c["modes"])
    m.load_state_dict(mc["state"], strict=True)
    return m.cuda().train(train)


def _step(m, bag):
    mc = _model_case()
    m.zero_grad(set_to_none=True)
    out = m(mc["x"].cuda(), bag_idx=bag)
    (out * mc["cot"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_model_matches_fp64():
    from test_oracle_golden import unet_grad_bar
    c, mc = R.MODEL, _model_case()
    m = _device_model()
    out, grads = _step(m, c["bag"])
    assert tuple(out.shape) == (c["B"], *c["input_size"], 2)
    e = rel_l2(out.double().cpu().numpy(), mc["o64"].numpy())
    bar = max(1e-5, 3 * mc["env_o"])
    print(f"model fwd {e:.2e} (bar {bar:.2e})")
    assert e <= bar, (e, bar)
    g64 = mc["g64"]
    scale = max(float(v.abs().pow(2).sum().sqrt()) for v in g64.values())
    worst = (0.0, None)
    for k, p in m.named_parameters():
        if k.startswith(m.unused_prefixes):
            assert p.grad is None and k not in g64, k
            continue
        a = grads[k].cpu()
        a = a.to(torch.complex128) if a.is_complex() else a.double()
        r = g64[k]
        if float(r.abs().pow(2).sum().sqrt()) <= 1e-10 * scale:
            assert float(a.abs().pow(2).sum().sqrt()) <= 1e-5 * scale, k
            continue
        ek, bk = rel_l2(a.numpy(), r.numpy()), unet_grad_bar(mc["env_g"][k])
        assert ek <= bk, (k, ek, bk)
        worst = max(worst, (ek / bk, k))
    print(f"model worst gradient / bar {worst[0]:.2f} ({worst[1]})")
    again, grads2 = _step(m, c["bag"])                        # a second forward + backward: bit-identical
    assert torch.equal(out, again)
    assert grads.keys() == grads2.keys() and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_model_bag_order_eval_and_shapes():
    c, mc = R.MODEL, _model_case()
    m = _device_model()
    x = mc["x"].cuda()
    with torch.no_grad():
        a = m(x, bag_idx=c["bag"])
        b = m(x, bag_idx=c["bag"][::-1])
        d = m(x, bag_idx=torch.as_tensor(c["bag"], device="cuda"))       # device-resident indices
        assert rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= 1e-6
        assert torch.equal(a, d)
        m.eval()
        T = c["T"]
        full, same, part = m(x, grid=None), m(x, bag_idx=np.arange(T)), m(x, bag_idx=np.arange(T - 1))
        assert torch.equal(full, same) and not torch.equal(full, part)
        ref = R.unet3d(R.leaves(m.state_dict()), mc["x"].double(), c["depth"], idx=None, train=False)
        assert rel_l2(full.double().cpu().numpy(), ref.detach().numpy()) <= max(1e-5, 3 * mc["env_o"])
    for bad in (x[:, :, 0], x[:, :, :, :, :-1]):
        with pytest.raises(ValueError, match="expected x"):
            m(bad)


# ---------------------------------------------------------------------------------- trainer

def test_trainer_3d_fpe_unet_two_eager_steps(tmp_path):
    """Four 8^3 training samples of T = 52 snapshots at batch 2: one epoch = two eager steps of the
    3d_FPE unet experiment, then its evaluation; compute_time_error_3d takes the model as it is."""
    from blindno import datagen, timeerror, trainer, unet3d
    from blindno.train import trained_parameters
    rs = np.random.RandomState(8)
    Mn, T, n = 5, 52, 8
    traj = rs.rand(Mn, T, n, n, n)
    traj /= traj.sum(axis=(2, 3, 4), keepdims=True)
    d = dict(trajectories=traj, potential=-1e-20 * rs.rand(Mn, n, n, n),
             drag=datagen.DRAG * (1 + rs.rand(Mn, n, n, n)))
    path = str(tmp_path / "fpe3d.npz")
    np.savez(path, **d)
    exp = trainer.experiments_for("unet")["3d_FPE"]
    t = trainer.Trainer(exp, path, str(tmp_path / exp.result_dir), torch.device("cuda"), epochs=1, save_interval=1,
                        batch=2, log=lambda s: None)
    assert t.graphed is None and isinstance(t.model, unet3d.PermInvUNet_attn3D) and t.model.input_size == (8, 8, 8)
    assert len(t.train_idx) == 4
    names = {id(p): k for k, p in t.model.named_parameters()}
    trained = [names[id(p)] for p in trained_parameters(t.model, exclude_prefixes=exp.exclude_prefixes)]
    assert not any(k.startswith("skip_norms.3.") for k in trained) and "fno.fc0.weight" in trained
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    hist = t.fit()
    assert [len(hist[k]) for k in exp.loss_files] == [1, 1, 1, 1]
    assert all(math.isfinite(v) for k in exp.loss_files for v in hist[k]) and hist["train_losses"][0] > 0
    after = t.model.state_dict()
    moved = [k for k in trained if not torch.equal(before[k], after[k])]
    # (at base_ch = 1 the level-0 LayerNorm over one channel passes no gradient to what feeds it)
    assert {k.split(".")[0] for k in moved} == {"down_convs", "skip_norms", "temp_atts", "up_transposes", "up_convs",
                                                "final_conv", "fno"}
    assert len(moved) > len(trained) // 2
    rows = timeerror.compute_time_error_3d({"unet": t.model.eval()}, d, d, [0], nsteps=3, tf=2e-5, batch=1,
                                           extent_nm=80, resolution_nm=10)
    assert len(rows) == 1 and rows[0][1] == "unet" and all(math.isfinite(v) for v in rows[0][2:4])
