"""The filter gradient of fftconv on the device (plan_fftconv_grad, fftconv_filter_grad; TileCfg::WGRAD) and the autograd of
mf.fftconv: the kernel against the fp64 model of test_fftconv_grad_host.py in every length class, impulses index by index on
both paths, channel separation, the reduction over partials, overlap-save, the dot-product identity, and the gradients of
x, k, pregate, postgate and skip against torch CPU autograd of the composition.  Outputs lie between canaries; inputs are
compared bitwise before and after."""
import ctypes

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_grad_host import gk_of, reference_grads, wgrad_model, worst_row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
GUARD = 64
CANARY = -7.25


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _data(seed, B, D, L, Lo, dtype):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B * D, L)).astype(NP[dtype]), rng.standard_normal((B * D, Lo)).astype(NP[dtype])


def _run(plan, x, gy):
    """plan.run into a buffer with canaries on both sides; x and gy must come back bit for bit.  -> (P, D, h) complex128"""
    xd, gd = torch.from_numpy(x).to(DEV).reshape(plan.in_shape), torch.from_numpy(gy).to(DEV).reshape(plan.grad_shape)
    kx, kg = _bits(xd).clone(), _bits(gd).clone()
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    plan.run(out, xd, gd)
    torch.cuda.synchronize()
    assert (flat[:GUARD] == CANARY).all() and (flat[GUARD + numel:] == CANARY).all()
    assert torch.equal(_bits(xd), kx) and torch.equal(_bits(gd), kg)
    o = out.cpu().numpy().astype(np.float64)
    return o[..., 0] + 1j * o[..., 1]


def _facts(plan, n, t, ols):
    name = plan.kernel_name(1)
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert plan.kernel_name(0) == "none" and name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "") + "r2c_"), name
    assert name.endswith("_wgrad_ols_jit" if ols else "_wgrad_jit"), name
    tile, threads, n_tiles, grid = plan.pass_geometry(1)
    assert grid == plan.channels * plan.partials and tuple(plan.out_shape) == (plan.partials, plan.channels, n // 2 + 1, 2)
    assert plan.out_bytes == int(np.prod(plan.out_shape)) * (8 if t == "f64" else 4)
    return tile, grid


# the (n, L, K, D, B, dtype) list of test_gpu_fftconv.py: even half lengths, most of them powers of two.  Every length class
# of the packed rows (odd half lengths, tiles of 62, 42, 3 and 1 rows, one to four passes) runs in test_gpu_packed_families.py
LENGTHS = [(16, 8, 5, 1, 3, "f32"), (64, 37, 28, 3, 5, "f32"), (96, 50, 40, 2, 4, "f32"), (1000, 600, 300, 4, 2, "f32"),
           (2048, 1024, 1024, 3, 2, "f32"), (16384, 8192, 8192, 2, 2, "f32"), (12288, 6000, 6000, 2, 1, "f64"),
           (64, 37, 28, 3, 5, "f64"), (2048, 1024, 1024, 3, 2, "f64")]


@pytest.mark.parametrize("n,L,K,D,B,t", LENGTHS, ids=lambda v: str(v))
def test_lengths_against_the_model(n, L, K, D, B, t):
    dtype = DT[t]
    x, gy = _data(n + L, B, D, L, L, dtype)
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n)
    _facts(plan, n, t, False)
    assert (plan.blocks, plan.step) == (1, None) and 1 <= plan.partials <= B
    A = _run(plan, x, gy)
    want = wgrad_model(x, gy, n, D, 0, L, 0, 1, L, P=plan.partials)
    assert worst_row(A, want) <= TOL[dtype], worst_row(A, want)  # every partial row of bins
    gk = plan.filter_grad(torch.from_numpy(x).to(DEV).reshape(plan.in_shape), torch.from_numpy(gy).to(DEV).reshape(plan.grad_shape), K)
    assert tuple(gk.shape) == (D, K) and gk.dtype == dtype
    err = worst_row(gk.cpu().numpy(), gk_of(want, n, K))
    print(f"gk rel l2 {err:.3e}")
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("correlate", [False, True])
def test_impulses_index_by_index_single_block(correlate):
    n, L, K = 64, 37, 28
    plan = mf.plan_fftconv_grad(torch.float64, 1, 1, L, n, correlate=correlate)
    for s, t0 in ((0, 0), (0, 27), (5, 4), (5, 5), (9, 36), (36, 36), (36, 0), (20, 10)):
        x, gy = np.zeros((1, L)), np.zeros((1, L))
        x[0, s], gy[0, t0] = 1, 1
        gk = np.fft.irfft(_run(plan, x, gy).sum(0), n, axis=-1)[0, :K]
        want = np.zeros(K)
        lag = s - t0 if correlate else t0 - s
        if 0 <= lag < K:
            want[lag] = 1
        assert np.abs(gk - want).max() <= 1e-13, (s, t0, correlate)


def test_impulses_across_the_seams_of_overlap_save():
    n, K, T = 64, 20, 300
    S = n - K + 1
    plan = mf.plan_fftconv_grad(torch.float64, 1, 1, T, n, taps=K)
    assert plan.blocks == -(-T // S) and plan.step == S
    for s, t0 in ((S - 1, S - 1), (S - 1, S), (S, S), (S - 3, S + 2), (S, S - 1), (2 * S - 1, 2 * S + 5), (0, K - 1), (T - 1, T - 1),
                  (T - K, T - 1), (3 * S - 19, 3 * S), (3 * S - 20, 3 * S)):
        x, gy = np.zeros((1, T)), np.zeros((1, T))
        x[0, s], gy[0, t0] = 1, 1
        gk = np.fft.irfft(_run(plan, x, gy).sum(0), n, axis=-1)[0, :K]
        want = np.zeros(K)
        if 0 <= t0 - s < K:
            want[t0 - s] = 1
        assert np.abs(gk - want).max() <= 1e-13, (s, t0)


def test_channels_are_separate():
    n, L, D, B = 64, 37, 3, 4
    x, gy = _data(7, B, D, L, L, torch.float32)
    keep = np.zeros((B, D, 1), dtype=np.float32)
    keep[:, 1] = 1
    x, gy = (x.reshape(B, D, L) * keep).reshape(B * D, L), (gy.reshape(B, D, L) * keep).reshape(B * D, L)
    for P in (1, 2):
        A = _run(mf.plan_fftconv_grad(torch.float32, B, D, L, n, partials=P), x, gy)
        assert (A[:, 0] == 0).all() and (A[:, 2] == 0).all() and np.abs(A[:, 1]).max() > 1


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_the_reduction_over_partials(t):
    dtype = DT[t]
    n, L, D, B, K = 64, 37, 2, 11, 28
    x, gy = _data(11, B, D, L, L, dtype)
    p1 = mf.plan_fftconv_grad(dtype, B, D, L, n, partials=1)
    tile, _ = _facts(p1, n, t, False)
    A1 = _run(p1, x, gy)
    assert worst_row(A1, wgrad_model(x, gy, n, D, 0, L, 0, 1, L)) <= TOL[dtype]
    for P in (2, 3, 4, 11):  # (11 pairs per channel: no multiple of TILE * P)
        plan = mf.plan_fftconv_grad(dtype, B, D, L, n, partials=P)
        assert plan.partials == P
        A = _run(plan, x, gy)
        assert worst_row(A, wgrad_model(x, gy, n, D, 0, L, 0, 1, L, P=P)) <= TOL[dtype], P
        assert worst_row(A.sum(0), A1[0]) <= TOL[dtype], P
        assert np.array_equal(A, _run(plan, x, gy)), "two runs of one plan are bit-identical"
    # more partials asked for than there are pairs: capped
    few = mf.plan_fftconv_grad(dtype, 2, D, L, n, partials=5)
    assert few.partials == 2
    A = _run(few, x[:2 * D], gy[:2 * D])
    assert worst_row(A, wgrad_model(x[:2 * D], gy[:2 * D], n, D, 0, L, 0, 1, L, P=2)) <= TOL[dtype]


def test_a_workgroup_walks_three_tiles():
    n, L, D = 64, 37, 2
    probe = mf.plan_fftconv_grad(torch.float32, 1, D, L, n, partials=1)
    tile = probe.pass_geometry(1)[0]
    B = 2 * (3 * tile) + tile // 2 + 1  # two slices of more than three full steps each, the last step ragged
    plan = mf.plan_fftconv_grad(torch.float32, B, D, L, n, partials=2)
    tile2, threads, n_tiles, grid = plan.pass_geometry(1)
    assert tile2 == tile and grid == 2 * D and n_tiles // grid >= 3
    x, gy = _data(13, B, D, L, L, torch.float32)
    A = _run(plan, x, gy)
    assert worst_row(A, wgrad_model(x, gy, n, D, 0, L, 0, 1, L, P=2)) <= REL_L2_TOL_F32
    assert np.array_equal(A, _run(plan, x, gy))


@pytest.mark.parametrize("n,K,T,D,B,t", [(64, 20, 300, 2, 3, "f32"), (64, 20, 300, 2, 3, "f64"), (4096, 257, 20000, 1, 2, "f32")],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("correlate", [False, True])
def test_overlap_save_against_the_model(n, K, T, D, B, t, correlate):
    dtype = DT[t]
    x, gy = _data(n + T, B, D, T, T, dtype)
    plan = mf.plan_fftconv_grad(dtype, B, D, T, n, taps=K, correlate=correlate)
    _facts(plan, n, t, True)
    c, S, s0, F = mf.api._fftconv_ols_geometry(n, K, 0, T, correlate)
    assert (plan.blocks, plan.step) == (F, S)
    A = _run(plan, x, gy)
    want = wgrad_model(x, gy, n, D, c, S, s0, F, T, correlate, P=plan.partials)
    assert worst_row(A.sum(0), want.sum(0)) <= TOL[dtype]
    assert worst_row(np.fft.irfft(A.sum(0), n, axis=-1)[:, :K], gk_of(want, n, K)) <= TOL[dtype]


def test_overlap_save_agrees_with_the_single_block():
    T, K, D, B = 100, 20, 2, 3
    x, gy = _data(17, B, D, T, T, torch.float64)
    xd, gd = torch.from_numpy(x).to(DEV).reshape(B, D, T), torch.from_numpy(gy).to(DEV).reshape(B, D, T)
    one = mf.fftconv_filter_grad(xd, gd, K, n=128)
    many = mf.fftconv_filter_grad(xd, gd, K, block=64)
    assert worst_row(many.cpu().numpy(), one.cpu().numpy()) <= REL_L2_TOL_F64


def test_the_dot_product_identity():
    B, D, L, K = 4, 16, 1024, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    x, gy = (torch.randn(B, D, L, generator=g, device=DEV) for _ in range(2))
    k = torch.randn(D, K, generator=g, device=DEV)
    y = mf.fftconv(x, k)
    gk = mf.fftconv_filter_grad(x, gy, K)
    lhs, rhs = float((gy.double() * y.double()).sum()), float((k.double() * gk.double()).sum())
    scale = float(gy.double().norm() * y.double().norm())
    print(f"dot-product identity: {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= REL_L2_TOL_F32 * scale


def test_the_exec_refuses_what_it_must():
    plan = mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64)
    lib = _lib.lib()
    x = torch.zeros(plan.in_shape, device=DEV)
    gy = torch.zeros(plan.grad_shape, device=DEV)
    out = torch.full(plan.out_shape, CANARY, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    good = mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, x.data_ptr(), gy.data_ptr())
    for args, first, count, status, word in (
            (good, 1, 5, -8, "whole batch"), (good, 0, 5, -8, "whole batch"), (good, 0, 0, -8, "whole batch"),
            (mf.ConvGradArgs(0, x.data_ptr(), gy.data_ptr()), 0, 6, -15, "mifft_conv_grad_args"),
            (mf.ConvGradArgs(mf.GATED_ARGS_MAGIC, x.data_ptr(), gy.data_ptr()), 0, 6, -15, "magic"),
            (mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, None, gy.data_ptr()), 0, 6, -12, "x is NULL"),
            (mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, x.data_ptr(), None), 0, 6, -12, "gy is NULL"),
            (mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, out.data_ptr(), gy.data_ptr()), 0, 6, -13, "overlap"),
            (mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, x.data_ptr(), out.data_ptr()), 0, 6, -13, "overlap")):
        rc = lib.mifft_exec_batch(plan._h, ctypes.addressof(args), out.data_ptr(), first, count, stream)
        assert rc == status and word in lib.mifft_last_error().decode(), (first, count, rc, lib.mifft_last_error().decode())
    rc = lib.mifft_exec_batch(plan._h, x.data_ptr(), out.data_ptr(), 0, 6, stream)  # (a device address in the place of the block)
    assert rc == -15 and "device address" in lib.mifft_last_error().decode()
    torch.cuda.synchronize()
    assert (out == CANARY).all(), "nothing was launched"


# ---- autograd of mf.fftconv against torch CPU autograd of the composition ---------------------------------------------------
def _autograd_case(B, D, L, K, n, mode, correlate, dtype, gates, skip, block=None, k1d=False, seed=0):
    rng = np.random.default_rng(seed + L + K)
    o, Lo = mf.api._fftconv_window(mode, L, K)
    shape_x, shape_y = ((B, D, L), (B, D, Lo)) if not k1d else ((B, L), (B, Lo))
    x, gy = rng.standard_normal(shape_x), rng.standard_normal(shape_y)
    k = rng.standard_normal((K,) if k1d else (D, K))
    a = rng.standard_normal(shape_x) if gates & 1 else None
    b = rng.standard_normal(shape_y) if gates & 2 else None
    d = {None: None, "float": 0.75, "tensor": rng.standard_normal(1 if k1d else D)}[skip]
    cast = lambda v: v if v is None or isinstance(v, float) else v.astype(NP[dtype]).astype(np.float64)
    x, gy, k, a, b, d = (cast(v) for v in (x, gy, k, a, b, d))
    # the reference: fp64, CPU; the linear convolution is the composition at a length that does not wrap
    nref = n if block is None else 1 << int(np.ceil(np.log2(L + K)))
    yref, *gref = reference_grads(x, k, a, b, d, gy, nref, o, Lo, correlate)
    dev = lambda v: v if v is None or isinstance(v, float) else torch.from_numpy(v.astype(NP[dtype])).to(DEV).requires_grad_(True)
    xs, ks, as_, bs, ds = (dev(v) for v in (x, k, a, b, d))
    y = mf.fftconv(xs, ks, mode=mode, correlate=correlate, pregate=as_, postgate=bs, skip=ds,
                   **({"block": block} if block is not None else {"n": n}))
    assert y.grad_fn is not None and y.dtype == dtype
    y.backward(torch.from_numpy(gy.astype(NP[dtype])).to(DEV))
    tol = TOL[dtype]
    assert worst_row(y.detach().cpu().numpy(), yref) <= tol
    for name, t, ref in zip(("x", "k", "pregate", "postgate", "skip"), (xs, ks, as_, bs, ds), gref):
        if ref is None:
            continue
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == dtype, name
        err = worst_row(t.grad.cpu().numpy(), ref)
        print(f"{name}: rel l2 {err:.3e}")
        assert err <= tol, (name, err)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("mode,correlate", [("causal", False), ("full", False), ("same", False), ("valid", False), ("causal", True)])
def test_autograd_modes(mode, correlate, t):
    _autograd_case(3, 2, 50, 40, 128 if mode == "valid" else 96, mode, correlate, DT[t], 3, "tensor")


@pytest.mark.parametrize("gates,skip", [(0, None), (1, None), (2, None), (3, None), (0, "tensor"), (1, "float"), (2, "tensor")])
def test_autograd_gates_and_skip(gates, skip):
    _autograd_case(3, 2, 50, 40, 96, "causal", False, torch.float64, gates, skip, seed=3)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_autograd_circular_n(t):
    _autograd_case(3, 2, 50, 40, 64, "causal", False, DT[t], 3, "tensor", seed=5)


@pytest.mark.parametrize("mode,correlate", [("causal", False), ("same", False), ("full", False), ("valid", False), ("causal", True)])
def test_autograd_overlap_save(mode, correlate):
    _autograd_case(2, 2, 150, 20, None, mode, correlate, torch.float64, 3, "tensor", block=64, seed=7)
    _autograd_case(2, 2, 150, 20, None, mode, correlate, torch.float32, 1, None, block=64, seed=8)


def test_autograd_1d_filter():
    _autograd_case(5, 1, 50, 40, 96, "causal", False, torch.float64, 3, "tensor", k1d=True, seed=9)
    _autograd_case(5, 1, 50, 40, 96, "full", False, torch.float32, 0, None, k1d=True, seed=10)


def test_autograd_n_2048():
    _autograd_case(2, 3, 1024, 1024, 2048, "causal", False, torch.float32, 3, "tensor", seed=11)


@pytest.mark.parametrize("block", [None, 16])
def test_gradcheck(block):
    g = torch.Generator(device=DEV).manual_seed(21)
    B, D, L, K = 1, 2, 8, 5
    mk = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float64).requires_grad_(True)
    x, k, a, b, d = mk(B, D, L), mk(D, K), mk(B, D, L), mk(B, D, L), mk(D)
    sel = {"block": block} if block is not None else {"n": 16}
    fn = lambda x, k, a, b, d: mf.fftconv(x, k, pregate=a, postgate=b, skip=d, **sel)
    assert torch.autograd.gradcheck(fn, (x, k, a, b, d), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


def test_two_layers_of_one_shape():
    """both forwards first, then both backwards: the cached plans share one filter_spectrum per key, which the second
    forward overwrites; each layer's gradients still match its own reference"""
    rng = np.random.default_rng(33)
    B, D, L, K, n = 3, 2, 50, 40, 96
    layers = []
    for _ in range(2):
        x, a, b, gy = (rng.standard_normal((B, D, L)) for _ in range(4))
        k, d = rng.standard_normal((D, K)), rng.standard_normal(D)
        layers.append((x, k, a, b, d, gy))
    dev = lambda v: torch.from_numpy(v).to(DEV).requires_grad_(True)
    ts = [tuple(dev(v) for v in lay[:5]) for lay in layers]
    ys = [mf.fftconv(x, k, n=n, pregate=a, postgate=b, skip=d) for x, k, a, b, d in ts]
    for y, lay in zip(ys, layers):
        y.backward(torch.from_numpy(lay[5]).to(DEV))
    for t, lay in zip(ts, layers):
        _, *gref = reference_grads(*lay[:5], lay[5], n, 0, L, False)
        for name, v, ref in zip(("x", "k", "pregate", "postgate", "skip"), t, gref):
            assert worst_row(v.grad.cpu().numpy(), ref) <= REL_L2_TOL_F64, name


def test_only_what_is_asked():
    g = torch.Generator(device=DEV).manual_seed(41)
    B, D, L, K = 3, 2, 50, 40
    x, k = torch.randn(B, D, L, generator=g, device=DEV), torch.randn(D, K, generator=g, device=DEV)
    a = torch.randn(B, D, L, generator=g, device=DEV)
    plain = mf.fftconv(x, k, pregate=a)
    assert plain.grad_fn is None
    xs = x.clone().requires_grad_(True)
    y = mf.fftconv(xs, k, pregate=a)
    assert y.grad_fn is not None
    assert torch.equal(_bits(y.detach()), _bits(plain)), "the differentiable path's forward is today's, bit for bit"
    y.sum().backward()  # (an expanded, non-contiguous gradient)
    assert xs.grad is not None and k.grad is None and a.grad is None
    ref = reference_grads(x.cpu().numpy().astype(np.float64), k.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64),
                          None, None, np.ones((B, D, L)), mf.fftconv_length(L + K - 1), 0, L, False)[1]
    assert worst_row(xs.grad.cpu().numpy(), ref) <= REL_L2_TOL_F32
    with torch.no_grad():
        quiet = mf.fftconv(xs, k, pregate=a)
    assert quiet.grad_fn is None and torch.equal(_bits(quiet), _bits(plain))
    # only k: no gradient of x is computed or returned
    ks = k.clone().requires_grad_(True)
    mf.fftconv(x, ks, pregate=a).sum().backward()
    assert ks.grad is not None and x.grad is None
    # a float16 input is converted to the working dtype and gets its gradient back through the conversion
    xh = x.half().requires_grad_(True)
    yh = mf.fftconv(xh, k)
    assert yh.dtype == torch.float64
    yh.sum().backward()
    assert xh.grad is not None and xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape
