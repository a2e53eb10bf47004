"""Gates fused into the filter gradient of fftconv on the device (plan_fftconv_grad(pregate=, postgate=); TileCfg::WGRAD with
TileCfg::GATE).  The main check is bit equality: the gated kernel on (x, gy, a, b) against the ungated kernel of the same
arguments and partials on the torch products a * x and b * gy (16-bit rows: the float32 kernel on the float32 products of the
widened tensors), in every length class, on overlap-save blocks, through more than one tile per workgroup and through the
reduction over partials.  Impulses under gates that differ everywhere identify the index a gate is read at; gates between
rows of NaN show that a zero-extended position reads none; filter_grad / fftconv_filter_grad are compared with the fp64 model
of test_fftconv_grad_host.py; the autograd of mf.fftconv keeps its bits; the exec refuses what it must."""
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
# key -> (the plan's dtype, io_dtype, what the tensors are in memory, the kernel's suffix before `_jit`)
KINDS = {"f32": (torch.float32, None, torch.float32, ""), "f64": (torch.float64, None, torch.float64, ""),
         "bf16": (torch.float32, torch.bfloat16, torch.bfloat16, "_b16"), "h16": (torch.float32, torch.float16, torch.float16, "_h16")}
GUARD = 64
CANARY = -7.25
UNSUPPORTED = -15


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _rand(seed, shape, sdt):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(sdt).to(DEV)


def _run(plan, x, gy, a=None, b=None):
    """plan.run into a buffer with canaries on both sides; every input must come back bit for bit.  -> the result's bits"""
    ins = [t for t in (x, gy, a, b) if t is not None]
    keep = [_bits(t).clone() for t in ins]
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    kw = {k: v for k, v in (("pregate", a), ("postgate", b)) if v is not None}
    plan.run(out, x, gy, **kw)
    torch.cuda.synchronize()
    assert (flat[:GUARD] == CANARY).all() and (flat[GUARD + numel:] == CANARY).all()
    for t, k in zip(ins, keep):
        assert torch.equal(_bits(t), k), "an input was written"
    return _bits(out).cpu()


def _products(x, gy, a, b, wide):
    """what the ungated plan reads in the place of (x, gy): torch's products, of the widened tensors on 16-bit rows"""
    w = (lambda t: t.float()) if wide else (lambda t: t)
    return (w(x) if a is None else w(a) * w(x)), (w(gy) if b is None else w(b) * w(gy))


def _gated_against_products(kind, B, D, L, n, g, *, taps=None, correlate=False, partials=None, seed=0):
    """-> (gated plan, its result's bits); asserts the facts of the plan and the bit equality"""
    dtype, io, sdt, suffix = KINDS[kind]
    kw = dict(taps=taps, correlate=correlate)
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n, partials=partials, io_dtype=io, pregate=bool(g & 1), postgate=bool(g & 2), **kw)
    ref = mf.plan_fftconv_grad(dtype, B, D, L, n, partials=plan.partials, **kw)
    assert (plan.pregate, plan.postgate) == (bool(g & 1), bool(g & 2)) and plan.io_dtype == io
    name = plan.kernel_name(1)
    assert name.startswith(f"rows{n}_" + ("f64_" if kind == "f64" else "") + "r2c_"), name
    assert name.endswith(("_wgrad_ols" if taps is not None else "_wgrad") + f"_g{g}{suffix}_jit"), name
    assert ref.kernel_name(1).endswith("_wgrad_ols_jit" if taps is not None else "_wgrad_jit"), ref.kernel_name(1)
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert plan.pass_geometry(1) == ref.pass_geometry(1) and tuple(plan.out_shape) == tuple(ref.out_shape)
    assert plan.partials == ref.partials and (plan.blocks, plan.step) == (ref.blocks, ref.step)
    x, a = (_rand(seed + i, plan.in_shape, sdt) for i in (1, 2))
    gy, b = (_rand(seed + i, plan.grad_shape, sdt) for i in (3, 4))
    a, b = (a if g & 1 else None), (b if g & 2 else None)
    got = _run(plan, x, gy, a, b)
    u, gv = _products(x, gy, a, b, io is not None)
    want = _run(ref, u, gv)
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} words differ from the ungated kernel on the products"
    return plan, got


# ---- 1. bit for bit, the main check -------------------------------------------------------------------------------------------
# (n, L, K, D, B) with the storage types: every length class of the packed rows; odd L puts single loads at the row ends and
# every other row of 16-bit samples 2 bytes off a 4-byte boundary; n = 16384 fp32 and n = 12288 fp64 are the spilling kernels
LENGTHS = [(16, 8, 5, 1, 3, "f32"), (64, 37, 28, 3, 5, "f32"), (64, 37, 28, 3, 5, "f64"), (64, 37, 28, 3, 5, "bf16"),
           (64, 37, 28, 3, 5, "h16"), (96, 50, 40, 2, 4, "f32"), (1000, 600, 300, 4, 2, "f32"), (2048, 1024, 1024, 3, 2, "f32"),
           (16384, 8192, 8192, 2, 2, "f32"), (16384, 8192, 8192, 2, 2, "bf16"), (12288, 6000, 6000, 2, 1, "f64")]


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("n,L,K,D,B,kind", LENGTHS, ids=lambda v: str(v))
def test_single_block_equals_the_ungated_kernel_on_the_products(n, L, K, D, B, kind, g):
    plan, _ = _gated_against_products(kind, B, D, L, n, g, seed=n + L)
    assert (plan.blocks, plan.step) == (1, None)


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("kind", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("correlate", [False, True])
def test_overlap_save_equals_the_ungated_kernel_on_the_products(correlate, kind, g):
    n, K, T, D, B = 64, 20, 300, 2, 3  # (S = 45 is odd; tiles straddle signal rows)
    plan, _ = _gated_against_products(kind, B, D, T, n, g, taps=K, correlate=correlate, seed=T)
    assert plan.step == 45 and plan.blocks == 7


# ---- 2. impulses identify the index a gate is read at -------------------------------------------------------------------------
def _impulse(plan, rows, L, Lo, r, s, t0, n, K):
    """x = e_s and gy = e_t0 in row r under gates that differ everywhere -> (gk (D, K), a[r, s] * b[r, t0])"""
    x, gy = torch.zeros(rows, L, dtype=torch.float64), torch.zeros(rows, Lo, dtype=torch.float64)
    x[r, s], gy[r, t0] = 1, 1
    a = 1 + torch.arange(rows, dtype=torch.float64).reshape(rows, 1) + torch.arange(L, dtype=torch.float64) / 1024
    b = 2 + torch.arange(rows, dtype=torch.float64).reshape(rows, 1) + torch.arange(Lo, dtype=torch.float64) / 1024
    dev = lambda t, shape: t.to(DEV).reshape(shape)
    out = torch.empty(plan.out_shape, dtype=torch.float64, device=DEV)
    plan.run(out, dev(x, plan.in_shape), dev(gy, plan.grad_shape), pregate=dev(a, plan.in_shape), postgate=dev(b, plan.grad_shape))
    o = out.cpu().numpy()
    A = o[..., 0] + 1j * o[..., 1]
    return np.fft.irfft(A.sum(0), n, axis=-1)[:, :K], float(a[r, s] * b[r, t0])


def _check_impulse(gk, value, d, lag, K, what):
    """gk[d, lag] is the product of the two gate elements within 1e-13 relative; every other lag, of every channel, within
    1e-13 of zero"""
    rest = gk.copy()
    if 0 <= lag < K:
        assert abs(gk[d, lag] - value) <= 1e-13 * value, (what, gk[d, lag], value)
        rest[d, lag] = 0
    assert np.abs(rest).max() <= 1e-13, (what, np.abs(rest).max())


def test_impulses_identify_the_gate_index_single_block():
    n, L, K, D, B = 64, 37, 28, 3, 2
    plan = mf.plan_fftconv_grad(torch.float64, B, D, L, n, partials=1, pregate=True, postgate=True)
    for r in (0, B * D - 1):
        for s, t0 in ((0, 0), (0, 27), (5, 5), (9, 36), (36, 36), (18, 20), (20, 10), (36, 0)):
            gk, value = _impulse(plan, B * D, L, L, r, s, t0, n, K)
            _check_impulse(gk, value, r % D, t0 - s, K, (r, s, t0))


def test_impulses_identify_the_gate_index_across_the_seams_of_overlap_save():
    n, K, T, D, B = 64, 20, 300, 3, 2
    S = n - K + 1
    plan = mf.plan_fftconv_grad(torch.float64, B, D, T, n, taps=K, partials=1, pregate=True, postgate=True)
    assert plan.blocks == -(-T // S) and plan.step == S
    for r in (0, 5):  # (the tile's steps wrap from one signal into the next)
        for s, t0 in ((S - 1, S - 1), (S - 1, S), (S, S), (S - 3, S + 2), (S, S - 1), (2 * S - 1, 2 * S + 5), (0, K - 1),
                      (T - 1, T - 1), (T - K, T - 1), (3 * S - 19, 3 * S), (3 * S - 20, 3 * S)):
            gk, value = _impulse(plan, B * D, T, T, r, s, t0, n, K)
            _check_impulse(gk, value, r % D, t0 - s, K, (r, s, t0))


# ---- 3. positions that are zero-extended read no gate --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("taps", [None, 20], ids=["single", "ols"])
def test_zero_extended_positions_read_no_gate(taps, kind):
    """the gates are the middle of buffers whose first and last row are NaN (run() wants contiguous tensors, so the guards
    are rows before and after): a single block of L < n reads beyond the end of every row, the causal overlap-save plan
    (s0 = -19) before its beginning as well; a gate read there would reach the neighbouring row, at the ends a NaN"""
    dtype, io, sdt, _ = KINDS[kind]
    n, D, B = 64, 2, 3
    L = 37 if taps is None else 300
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=taps, partials=1, io_dtype=io, pregate=True, postgate=True)
    ref = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=taps, partials=1)
    rows = B * D
    x, gy = _rand(1, plan.in_shape, sdt), _rand(2, plan.grad_shape, sdt)
    bufs = []
    for i, shape in ((3, plan.in_shape), (4, plan.grad_shape)):
        buf = torch.full((rows + 2,) + tuple(shape[1:]), float("nan"), dtype=sdt, device=DEV)
        buf[1:-1] = _rand(i, shape, sdt)
        bufs.append(buf)
    a, b = bufs[0][1:-1], bufs[1][1:-1]
    assert a.is_contiguous() and b.is_contiguous() and torch.isnan(bufs[0][0]).all() and torch.isnan(bufs[1][-1]).all()
    got = _run(plan, x, gy, a, b)
    out = got.view(torch.float32)
    assert torch.isfinite(out).all()
    want = _run(ref, *_products(x, gy, a, b, io is not None))
    assert torch.equal(got, want)


# ---- 4. a workgroup walks three tiles, and the reduction over partials ---------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 5])
def test_three_tiles_per_workgroup_and_the_partials(P):
    n, L, D = 64, 37, 2
    probe = mf.plan_fftconv_grad(torch.float32, 1, D, L, n, partials=1, pregate=True, postgate=True)
    tile = probe.pass_geometry(1)[0]
    B = 2 * (3 * tile) + tile // 2 + 1  # (test_a_workgroup_walks_three_tiles: two slices of more than three steps, ragged)
    plan, got = _gated_against_products("f32", B, D, L, n, 3, partials=P, seed=13)
    tile2, threads, n_tiles, grid = plan.pass_geometry(1)
    assert plan.partials == P and tile2 == tile and grid == P * D and (P > 2 or n_tiles // grid >= 3)
    x, a = (_rand(13 + i, plan.in_shape, torch.float32) for i in (1, 2))
    gy, b = (_rand(13 + i, plan.grad_shape, torch.float32) for i in (3, 4))
    assert torch.equal(_run(plan, x, gy, a, b), got), "two runs of one plan are bit-identical"


# ---- 5. filter_grad / fftconv_filter_grad with gates ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("block", [None, 64], ids=["single", "ols"])
@pytest.mark.parametrize("mode,correlate", [("causal", False), ("full", False), ("same", False), ("valid", False), ("causal", True)])
def test_fftconv_filter_grad_with_gates_against_the_model(mode, correlate, block, kind):
    dtype = KINDS[kind][0]
    B, D = 3, 2
    L, K = (50, 40) if block is None else (150, 20)
    n = block if block is not None else 128 if mode == "valid" else 96
    o, Lo = mf.api._fftconv_window(mode, L, K)
    x, a = (_rand(L + i, (B, D, L), dtype) for i in (1, 2))
    gy, b = (_rand(L + i, (B, D, Lo), dtype) for i in (3, 4))
    gk = mf.fftconv_filter_grad(x, gy, K, mode=mode, correlate=correlate, pregate=a, postgate=b,
                                **({"block": block} if block is not None else {"n": n}))
    assert tuple(gk.shape) == (D, K) and gk.dtype == dtype
    c, S, s0, F = (o, Lo, 0, 1) if block is None else mf.api._fftconv_ols_geometry(n, K, o, Lo, correlate)
    u, gv = (a * x).cpu().numpy().reshape(B * D, L), (b * gy).cpu().numpy().reshape(B * D, Lo)
    want = gk_of(wgrad_model(u, gv, n, D, c, S, s0, F, Lo, correlate), n, K)
    err = worst_row(gk.cpu().numpy(), want)
    print(f"gk rel l2 {err:.3e}")
    assert err <= TOL[dtype], err
    # one gate alone, and the plan's own filter_grad
    for kw, (u1, g1) in ((dict(pregate=a), (a * x, gy)), (dict(postgate=b), (x, b * gy))):
        one = mf.fftconv_filter_grad(x, gy, K, mode=mode, correlate=correlate, **kw, **({"block": block} if block is not None else {"n": n}))
        w1 = gk_of(wgrad_model(u1.cpu().numpy().reshape(B * D, L), g1.cpu().numpy().reshape(B * D, Lo), n, D, c, S, s0, F, Lo, correlate), n, K)
        assert worst_row(one.cpu().numpy(), w1) <= TOL[dtype], kw.keys()
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K if block is not None else None, offset=o, out_length=Lo, correlate=correlate,
                                pregate=True, postgate=True)
    sh = lambda t, s: t.reshape(s)
    own = plan.filter_grad(sh(x, plan.in_shape), sh(gy, plan.grad_shape), K, pregate=sh(a, plan.in_shape), postgate=sh(b, plan.grad_shape))
    assert torch.equal(_bits(own), _bits(gk))
    with pytest.raises(mf.MifftError) as e:
        plan.filter_grad(sh(x, plan.in_shape), sh(gy, plan.grad_shape), K, pregate=sh(a, plan.in_shape))
    assert e.value.status == -12
    ungated = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K if block is not None else None, offset=o, out_length=Lo, correlate=correlate)
    with pytest.raises(mf.MifftError) as e:
        ungated.filter_grad(sh(x, plan.in_shape), sh(gy, plan.grad_shape), K, postgate=sh(b, plan.grad_shape))
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("kind", ["f32", "f64", "bf16"])
def test_the_partitioned_gradient_passes_the_gates_to_its_partitions(kind):
    dtype, io, sdt, _ = KINDS[kind]
    B, D, T, K = 2, 2, 100, 150
    x, a, gy, b = (_rand(70 + i, (B, D, T), sdt) for i in range(4))
    sel = dict(block=16, partition=9)
    got = mf.fftconv_filter_grad(x, gy, K, pregate=a, postgate=b, io_dtype=io, **sel)
    u, gv = _products(x, gy, a, b, io is not None)
    want = mf.fftconv_filter_grad(u, gv, K, **sel)
    assert tuple(got.shape) == (D, K) and got.dtype == dtype and torch.equal(_bits(got), _bits(want))
    plan = mf.plan_fftconv_grad(dtype, B, D, T, 16, taps=K, partition=9, io_dtype=io, pregate=True, postgate=True)
    assert plan.pregate and plan.postgate and plan.num_launches == sum(p is not None for p in plan.plans) > 1
    assert all(p.kernel_name(1).endswith("_wgrad_ols_g3" + KINDS[kind][3] + "_jit") for p in plan.plans if p is not None)


# ---- 6. autograd keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("kind", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("block", [None, 64], ids=["single", "ols"])
def test_autograd_takes_the_gated_plan_and_keeps_its_bits(block, kind, g):
    dtype, io, sdt, _ = KINDS[kind]
    B, D = 3, 2
    L, K = (50, 40) if block is None else (150, 20)
    sel = {"block": block} if block is not None else {"n": 96}
    x, a, gy, b = (_rand(90 + i, (B, D, L), sdt) for i in range(4))
    a, b = (a if g & 1 else None), (b if g & 2 else None)
    k = _rand(95, (D, K), dtype).requires_grad_(True)
    d = _rand(96, (D,), dtype).requires_grad_(True)
    y = mf.fftconv(x, k, pregate=a, postgate=b, skip=d, io_dtype=io, **sel)
    assert y.grad_fn is not None and y.dtype == sdt
    y.backward(gy)
    fused = mf.fftconv_filter_grad(x, gy, K, pregate=a, postgate=b, io_dtype=io, **sel)
    assert k.grad.dtype == dtype and torch.equal(_bits(k.grad), _bits(fused.reshape(k.shape).to(k.dtype)))
    assert torch.equal(_bits(d.grad), _bits(fused[:, 0].to(d.dtype)))
    u, gv = _products(x, gy, a, b, io is not None)
    on_products = mf.fftconv_filter_grad(u, gv, K, **sel)  # (16-bit rows: the float32 call on the widened products)
    assert on_products.dtype == dtype and torch.equal(_bits(k.grad), _bits(on_products))


def test_autograd_with_gates_against_the_reference():
    from test_gpu_fftconv_grad import _autograd_case
    _autograd_case(3, 2, 50, 40, 96, "causal", False, torch.float32, 3, "tensor", seed=51)
    _autograd_case(2, 2, 150, 20, None, "same", False, torch.float64, 3, "tensor", block=64, seed=52)


# ---- 7. the exec refuses what it must ------------------------------------------------------------------------------------------
def test_the_gated_exec_refuses_what_it_must():
    plan = mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64, pregate=True)
    lib = _lib.lib()
    x, a = torch.zeros(plan.in_shape, device=DEV), torch.ones(plan.in_shape, device=DEV)
    gy, b = torch.zeros(plan.grad_shape, device=DEV), torch.ones(plan.grad_shape, device=DEV)
    out = torch.full(plan.out_shape, CANARY, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    M = mf.CONV_GRAD_GATED_ARGS_MAGIC
    p = lambda t: t.data_ptr()
    good = mf.ConvGradGatedArgs(M, p(x), p(gy), p(a), None)
    for args, first, count, status, word in (
            (mf.ConvGradArgs(mf.CONV_GRAD_ARGS_MAGIC, p(x), p(gy)), 0, 6, -15, "mifft_conv_grad_gated_args"),  # the old block
            (mf.ConvGradGatedArgs(0, p(x), p(gy), p(a), None), 0, 6, -15, "mifft_conv_grad_gated_args"),
            (mf.ConvGradGatedArgs(mf.GATED_ARGS_MAGIC, p(x), p(gy), p(a), None), 0, 6, -15, "magic"),
            (mf.ConvGradGatedArgs(M, p(x), p(gy), None, None), 0, 6, -12, "pregate is NULL"),
            (mf.ConvGradGatedArgs(M, None, p(gy), p(a), None), 0, 6, -12, "x is NULL"),
            (mf.ConvGradGatedArgs(M, p(x), None, p(a), None), 0, 6, -12, "gy is NULL"),
            (mf.ConvGradGatedArgs(M, p(x), p(gy), p(a), p(b)), 0, 6, -15, "no postgate"),
            (mf.ConvGradGatedArgs(M, p(x), p(gy), p(out), None), 0, 6, -13, "pregate and out"),
            (mf.ConvGradGatedArgs(M, p(out), p(gy), p(a), None), 0, 6, -13, "overlap"),
            (good, 1, 5, -8, "whole batch"), (good, 0, 5, -8, "whole batch"), (good, 0, 0, -8, "whole batch")):
        rc = lib.mifft_exec_batch(plan._h, ctypes.addressof(args), p(out), first, count, stream)
        assert rc == status and word in lib.mifft_last_error().decode(), (first, count, rc, lib.mifft_last_error().decode())
    rc = lib.mifft_exec_batch(plan._h, p(x), p(out), 0, 6, stream)  # (a device address in the place of the block)
    assert rc == -15 and "mifft_conv_grad_gated_args" in lib.mifft_last_error().decode()
    # run(): a gate exactly where the plan has one, before any library call
    for kw, status in ((dict(), -12), (dict(pregate=a, postgate=b), UNSUPPORTED)):
        with pytest.raises(mf.MifftError) as e:
            plan.run(out, x, gy, **kw)
        assert e.value.status == status
    torch.cuda.synchronize()
    assert (out == CANARY).all(), "nothing was launched"
    # the gates may alias x, gy or each other: x as its own pregate squares it
    both = mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64, pregate=True, postgate=True, partials=1)
    xs, gs = _rand(5, both.in_shape, torch.float32), _rand(6, both.grad_shape, torch.float32)
    ref = mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64, partials=1)
    assert torch.equal(_run(both, xs, gs, xs, gs), _run(ref, xs * xs, gs * gs))
