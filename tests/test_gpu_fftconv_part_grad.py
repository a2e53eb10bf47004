"""The fused partitioned filter gradient on the device (plan_fftconv_grad(partition=, fused=True): FusedPartConvGradPlan; stage 1
TileCfg::WSPEC, stage 2 lag_corr.hip).  Every call names ``fused=True``.  The reference is the direct fp64 double sum on the
CPU (direct_gk of test_fftconv_part_grad_host.py), computed once per shape; the bounds are the project's REL_L2_TOL_F32 /
REL_L2_TOL_F64 per filter row, the ones the composed plan is held to.  Impulses name taps index by index across the seams of
the lag groups; slabs, dead frames, every compile-time class of the lag-group kernel, gates and 16-bit storage bit for bit
against the torch products, the autograd of mf.fftconv, and the layout of the spectra in scratch."""
import functools

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import api
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_grad_host import worst_row
from test_fftconv_part_grad_host import direct_gk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
# key -> (the plan's dtype, io_dtype, what the tensors are in memory, the kernel's suffix before `_jit`)
KINDS = {"f32": (torch.float32, None, torch.float32, ""), "f64": (torch.float64, None, torch.float64, ""),
         "bf16": (torch.float32, torch.bfloat16, torch.bfloat16, "_b16"), "h16": (torch.float32, torch.float16, torch.float16, "_h16")}
GUARD = 64
CANARY = -7.25


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _case(seed, B, D, L, Lo, K, o, correlate, t):
    """(x, gy) of the type's precision and the direct fp64 sum over them, once per shape"""
    rng = np.random.default_rng(seed)
    x, gy = rng.standard_normal((B * D, L)).astype(NP[DT[t]]), rng.standard_normal((B * D, Lo)).astype(NP[DT[t]])
    want = direct_gk(x, gy, D, K, o, correlate)
    for a in (x, gy, want):
        a.setflags(write=False)
    return x, gy, want


def _dev(a, B, D):
    return torch.tensor(a).to(DEV).reshape(B, D, a.shape[-1])  # (a copy: the shared arrays stay as they are)


# ---- against the model ----------------------------------------------------------------------------------------------------------
MODEL = [(8, 37, 29, 1, 3, "f32"), (16, 101, 101, 2, 2, "f32"), (96, 777, 300, 2, 3, "f32"), (1000, 5000, 2500, 2, 1, "f32"),
         (2048, 20000, 20000, 3, 1, "f32"), (16384, 40000, 40000, 1, 1, "f32"), (64, 1000, 1000, 3, 2, "f64"),
         (12288, 30000, 20000, 1, 1, "f64")]
# (both correlate values at the four smallest of either reading: the first four of the list, and the n = 64 one in fp64)
MODEL_CASES = [c + (False,) for c in MODEL] + [c + (True,) for c in MODEL[:4] + MODEL[6:7]]


@pytest.mark.parametrize("n,L,K,D,B,t,correlate", MODEL_CASES, ids=lambda v: str(v))
def test_against_the_model(n, L, K, D, B, t, correlate):
    dtype = DT[t]
    x, gy, want = _case(n + L + K, B, D, L, L, K, 0, correlate, t)
    got = mf.fftconv_filter_grad(_dev(x, B, D), _dev(gy, B, D), K, block=n, partition=n // 2 + 1, correlate=correlate, fused=True)
    assert tuple(got.shape) == (D, K) and got.dtype == dtype
    err = worst_row(got.cpu().numpy(), want)
    print(f"fused partitioned filter gradient n={n} L={L} K={K} {t} correlate={correlate}: rel l2 {err:.3e}")
    assert err <= TOL[dtype], err


def test_the_plan_and_its_kernels():
    n, L, K, D, B, Q = 64, 1000, 1000, 3, 2, 33
    plan = mf.plan_fftconv_grad(torch.float64, B, D, L, n, taps=K, partition=Q, fused=True)
    assert isinstance(plan, mf.FusedPartConvGradPlan)
    assert (plan.partition, plan.partitions, plan.step, plan.taps) == (Q, -(-K // Q), n - Q + 1, K)
    assert (plan.hop, plan.lag_groups, plan.slabs) == (32, 32, [(0, B)])
    assert plan.in_shape == (B * D, L, 1) and plan.grad_shape == (B * D, L, 1) and plan.io_dtype is None
    assert not plan.pregate and not plan.postgate and plan.num_launches == 3
    g = plan.geometry
    assert plan.scratch_bytes == B * D * (g.Fu + g.Fg) * (n // 2 + 1) * 16 == B * plan.entry_bytes
    up, gp, lp = plan.plans[0]
    for pl, tail in ((up, "_wspecu_ols_jit"), (gp, "_wspecg_ols_jit")):
        assert pl.kernel_name(0) == "none" and pl.kernel_name(1).startswith("rows64_f64_r2c_") and pl.kernel_name(1).endswith(tail)
    assert lp.kernel_name(1) == "lag_corr_f64_p32", lp.kernel_name(1)
    assert up.out_bytes == B * D * g.Fu * 33 * 16 and gp.out_bytes == B * D * g.Fg * 33 * 16
    assert lp.out_bytes == lp.partials * D * 32 * 33 * 16 and 1 <= lp.partials <= B
    # fused=False is today's composed plan
    composed = mf.plan_fftconv_grad(torch.float64, B, D, L, n, taps=K, partition=Q)
    assert isinstance(composed, mf.PartConvGradPlan) and len(composed.plans) == composed.partitions
    plan.close()
    composed.close()


# ---- every mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["causal", "full", "same", "valid"])
@pytest.mark.parametrize("L,K,n", [(333, 200, 16), (37, 90, 64)])
def test_every_mode(L, K, n, mode):
    B, D = 2, 2
    o, Lo = api._fftconv_window(mode, L, K)
    x, gy, want = _case(L + K + n + o, B, D, L, Lo, K, o, False, "f64")
    got = mf.fftconv_filter_grad(_dev(x, B, D), _dev(gy, B, D), K, block=n, partition=n // 2 + 1, mode=mode, fused=True)
    err = worst_row(got.cpu().numpy(), want)
    assert err <= REL_L2_TOL_F64, (mode, o, Lo, err)


# ---- impulses across lag-group seams ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("correlate", [False, True])
def test_impulses_across_lag_group_seams(correlate):
    n, T, K = 64, 200, 100  # (H = 32: lag groups 0 .. 3, the last of 4 lags)
    plan = mf.plan_fftconv_grad(torch.float64, 1, 1, T, n, taps=K, partition=33, correlate=correlate, fused=True)
    assert (plan.hop, plan.lag_groups) == (32, 4)
    for lag in (0, 31, 32, 33, 63, 64, 65, 99, 100):
        # gy[t0] meets x[s] at tap t0 - s (correlating: s - t0), once at the start of the rows and once at their end
        for s, t0 in ((0, lag), (T - 1 - lag, T - 1)):
            if correlate:
                s, t0 = t0, s
            x, gy = torch.zeros(1, T, 1, dtype=torch.float64, device=DEV), torch.zeros(1, T, 1, dtype=torch.float64, device=DEV)
            x[0, s], gy[0, t0] = 1, 1
            gk = plan.filter_grad(x, gy, K).cpu().numpy()[0]
            want = np.zeros(K)
            if lag < K:
                want[lag] = 1
            assert np.abs(gk - want).max() <= 1e-13, (lag, s, t0, correlate, np.abs(gk - want).max())


# ---- the composed plan computes the same ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,K,D,B,t", [(16, 101, 101, 2, 2, "f32"), (96, 777, 300, 2, 3, "f32"), (64, 1000, 1000, 3, 2, "f64")])
def test_agreement_with_the_composed_plan(n, L, K, D, B, t):
    x, gy, want = _case(n + L + K, B, D, L, L, K, 0, False, t)
    xd, gd = _dev(x, B, D), _dev(gy, B, D)
    kw = dict(block=n, partition=n // 2 + 1)
    fused, composed = mf.fftconv_filter_grad(xd, gd, K, fused=True, **kw), mf.fftconv_filter_grad(xd, gd, K, fused=False, **kw)
    assert torch.equal(_bits(composed), _bits(mf.fftconv_filter_grad(xd, gd, K, **kw))), "the default route is the composed plan here"
    for got in (fused, composed):
        assert worst_row(got.cpu().numpy(), want) <= TOL[DT[t]]


def test_two_runs_and_two_plans_give_the_same_bits():
    n, L, K, D, B = 96, 777, 300, 2, 3
    x, gy, _ = _case(n + L + K, B, D, L, L, K, 0, False, "f32")
    xd, gd = _dev(x, B, D).reshape(B * D, L, 1), _dev(gy, B, D).reshape(B * D, L, 1)
    make = lambda: mf.plan_fftconv_grad(torch.float32, B, D, L, n, taps=K, partition=49, fused=True)
    plan = make()
    first = _bits(plan.filter_grad(xd, gd, K)).clone()
    assert torch.equal(_bits(plan.filter_grad(xd, gd, K)), first)
    plan.close()
    again = make()
    assert torch.equal(_bits(again.filter_grad(xd, gd, K)), first)
    again.close()


# ---- slabs ------------------------------------------------------------------------------------------------------------------------
def test_slabs():
    n, L, K, D, B = 64, 300, 150, 2, 5
    x, gy, want = _case(5, B, D, L, L, K, 0, False, "f32")
    xd, gd = _dev(x, B, D).reshape(B * D, L, 1), _dev(gy, B, D).reshape(B * D, L, 1)
    g = api._fftconv_fused_grad_geometry(n, L, L, K, 0, False)
    entry = api._fftconv_fused_grad_entry_bytes(g, D, torch.float32)
    for limit, count in ((5 * entry, 1), (3 * entry + 1, 2), (2 * entry, 3), (entry, 5)):
        plan = mf.plan_fftconv_grad(torch.float32, B, D, L, n, taps=K, partition=33, fused=True, scratch_bytes=limit)
        assert plan.slabs == api._fftconv_fused_grad_slabs(B, entry, limit) and len(plan.slabs) == count
        assert plan.scratch_bytes == max(b1 - b0 for b0, b1 in plan.slabs) * entry <= limit
        assert plan.num_launches == 3 * count and plan.partials >= count
        err = worst_row(plan.filter_grad(xd, gd, K).cpu().numpy(), want)
        assert err <= REL_L2_TOL_F32, (count, err)
        plan.close()


# ---- guards -----------------------------------------------------------------------------------------------------------------------
def _between_nans(t):
    """a contiguous copy of (rows, L, 1) ``t`` that lies between two rows of NaN"""
    rows, L, _ = t.shape
    buf = torch.full((rows + 2, L, 1), float("nan"), dtype=t.dtype, device=t.device)
    buf[1:-1] = t
    return buf, buf[1:-1]


def _canaried(shape, dtype):
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + numel].view(shape)


@pytest.mark.parametrize("correlate", [False, True])
def test_guards(correlate):
    n, L, K, D, B = 64, 301, 150, 2, 3
    dtype = torch.float32
    gen = torch.Generator().manual_seed(9)
    mk = lambda: torch.randn((B * D, L, 1), generator=gen, dtype=torch.float64).to(dtype).to(DEV)
    bufs, views = zip(*(_between_nans(mk()) for _ in range(4)))
    x, gy, a, b = views
    keep = [_bits(t).clone() for t in bufs]
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K, partition=33, correlate=correlate, pregate=True, postgate=True, fused=True)
    gk = plan.filter_grad(x, gy, K, pregate=a, postgate=b)
    torch.cuda.synchronize()
    assert torch.isfinite(gk).all(), "a zero-extended position read the NaN beside its row"
    want = direct_gk((a * x).cpu().numpy()[..., 0], (b * gy).cpu().numpy()[..., 0], D, K, 0, correlate)
    assert worst_row(gk.cpu().numpy(), want) <= REL_L2_TOL_F32
    # each of the three launches into a buffer of its own between canaries
    g = plan.geometry
    up, gp, lp = plan.plans[0]
    bins = n // 2 + 1
    fu, U = _canaried((B * D, g.Fu, bins, 2), dtype)
    fg, G = _canaried((B * D, g.Fg, bins, 2), dtype)
    fo, out = _canaried((lp.partials, D, g.Pg, bins, 2), dtype)
    up.launch(U, x.data_ptr(), None, a.data_ptr(), None)
    gp.launch(G, None, gy.data_ptr(), None, b.data_ptr())
    lp.launch(out, U.data_ptr(), G.data_ptr())
    torch.cuda.synchronize()
    for flat, body in ((fu, U), (fg, G), (fo, out)):
        assert (flat[:GUARD] == CANARY).all() and (flat[-GUARD:] == CANARY).all(), "a store left its tensor"
        assert torch.isfinite(body).all() and not (body == CANARY).any(), "a value was left unwritten"
    A = out.sum(0)
    again = mf.irfftn(A.reshape(D * g.Pg, bins, 2), n).reshape(D, g.Pg, n)[:, :, :g.H].reshape(D, -1)[:, :K]
    assert torch.equal(_bits(again), _bits(gk))
    for buf, k in zip(bufs, keep):
        assert torch.equal(_bits(buf), k), "an input, or the rows beside it, changed"
    plan.close()


# ---- dead frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,Lo,correlate", [(5, 10, False), (60, 10, False), (95, 14, False), (3, 10, True), (0, 20, True)])
def test_dead_frames(o, Lo, correlate):
    n, L, K, D, B = 64, 20, 90, 2, 2  # (K > L and Lo < H = 32)
    x, gy, want = _case(o + Lo, B, D, L, Lo, K, o, correlate, "f64")
    plan = mf.plan_fftconv_grad(torch.float64, B, D, L, n, taps=K, partition=33, offset=o, out_length=Lo, correlate=correlate, fused=True)
    g = plan.geometry
    assert 0 < g.Fu < g.m_hi - g.m_lo + 1, "the case has dead frames"
    assert plan.plans[0][0].out_bytes == B * D * g.Fu * 33 * 16  # (only the live ones are stored)
    gk = plan.filter_grad(_dev(x, B, D).reshape(B * D, L, 1), _dev(gy, B, D).reshape(B * D, Lo, 1), K).cpu().numpy()
    assert worst_row(gk, want) <= REL_L2_TOL_F64
    j0, j1 = g.reachable
    assert j1 - j0 < K and (gk[:, :j0] == 0).all() and (gk[:, j1:] == 0).all(), "unreachable taps are exact zeros"
    assert (want[:, :j0] == 0).all() and (want[:, j1:] == 0).all()
    plan.close()


# ---- gates and storage ------------------------------------------------------------------------------------------------------------
def _odd_start(t):
    """a contiguous copy of a 16-bit tensor that starts 2 bytes off a 4-byte boundary"""
    flat = torch.empty(t.numel() + 3, dtype=t.dtype, device=t.device)
    k = 1 if flat.data_ptr() % 4 == 0 else 2
    v = flat[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("kind", ["f32", "f64", "bf16", "h16"])
def test_gates_equal_the_plan_on_the_torch_products(kind, g):
    dtype, io, sdt, suffix = KINDS[kind]
    n, L, K, D, B = 64, 151, 100, 2, 2  # (odd rows: every other row of 16-bit samples is 2 bytes off as well)
    gen = torch.Generator().manual_seed(g + len(kind))
    mk = lambda: torch.randn((B * D, L, 1), generator=gen, dtype=torch.float64).to(sdt).to(DEV)
    x, gy, a, b = mk(), mk(), mk(), mk()
    if io is not None:
        x, gy, a, b = (_odd_start(t) for t in (x, gy, a, b))
    a, b = (a if g & 1 else None), (b if g & 2 else None)
    plan = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K, partition=33, io_dtype=io, pregate=a is not None, postgate=b is not None,
                                fused=True)
    up, gp, _ = plan.plans[0]
    assert up.kernel_name(1).endswith("_wspecu_ols" + ("_g1" if g & 1 else "") + suffix + "_jit"), up.kernel_name(1)
    assert gp.kernel_name(1).endswith("_wspecg_ols" + ("_g2" if g & 2 else "") + suffix + "_jit"), gp.kernel_name(1)
    got = plan.filter_grad(x, gy, K, pregate=a, postgate=b)
    # the ungated plan on torch's products: of the widened tensors, in float32, on 16-bit rows
    w = (lambda t: t.float()) if io is not None else (lambda t: t)
    u, gv = (w(x) if a is None else w(a) * w(x)), (w(gy) if b is None else w(b) * w(gy))
    ref = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K, partition=33, fused=True)
    want = ref.filter_grad(u, gv, K)
    assert got.dtype == want.dtype == dtype
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} of {got.numel()} words differ"
    # and through the functional surface
    shape = lambda t: None if t is None else t.reshape(B, D, L)
    fn = mf.fftconv_filter_grad(shape(x), shape(gy), K, block=n, partition=33, io_dtype=io, pregate=shape(a), postgate=shape(b), fused=True)
    assert torch.equal(_bits(fn), _bits(got))
    plan.close()
    ref.close()


# ---- the accumulator classes of the lag-group kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("Pg", [1, 2, 3, 5, 9, 17, 32])
def test_the_bound_of_the_accumulator_classes(Pg):
    n, L, D, B = 16, 70, 2, 3  # (H = 8)
    K = 8 * Pg - 3 if Pg > 1 else 8
    x, gy, want = _case(Pg, B, D, L, L, K, 0, False, "f64")
    plan = mf.plan_fftconv_grad(torch.float64, B, D, L, n, taps=K, partition=9, fused=True)
    bound = next(b for b in (2, 4, 8, 16, 32) if Pg <= b)
    assert plan.lag_groups == Pg and plan.plans[0][2].kernel_name(1) == f"lag_corr_f64_p{bound}"
    gk = plan.filter_grad(_dev(x, B, D).reshape(B * D, L, 1), _dev(gy, B, D).reshape(B * D, L, 1), K).cpu().numpy()
    assert worst_row(gk, want) <= REL_L2_TOL_F64, worst_row(gk, want)
    plan.close()


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
def _torch_conv(x, k, mode):
    """the direct convolution on the CPU, differentiable: y[t] = sum_j k[j] x[t - j] of the full length, cropped as ``mode``"""
    D, K = k.shape
    L = x.shape[-1]
    full = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (K - 1, K - 1)), k.flip(-1)[:, None, :], groups=D)
    o, Lo = api._fftconv_window(mode, L, K)
    return full[..., o:o + Lo]


@pytest.mark.parametrize("mode", ["causal", "full", "same", "valid"])
def test_autograd_with_the_selector_forced(mode):
    n, Q, L, K, D, B = 64, 33, 150, 100, 2, 2
    gen = torch.Generator().manual_seed(len(mode))
    x0, k0 = torch.randn((B, D, L), generator=gen, dtype=torch.float64), torch.randn((D, K), generator=gen, dtype=torch.float64)
    o, Lo = api._fftconv_window(mode, L, K)
    gy0 = torch.randn((B, D, Lo), generator=gen, dtype=torch.float64)
    xc, kc = x0.clone().requires_grad_(), k0.clone().requires_grad_()
    (_torch_conv(xc, kc, mode) * gy0).sum().backward()
    x, k = x0.to(DEV).requires_grad_(), k0.to(DEV).requires_grad_()
    mf.clear_plan_cache()
    with mf.fftconv_fused_filter_grad(True):
        y = mf.fftconv(x, k, block=n, partition=Q, mode=mode)
        (y * gy0.to(DEV)).sum().backward()
    with api._PLAN_CACHE_LOCK:
        kinds = {type(p) for p in api._PLAN_CACHE.values()}
    assert mf.FusedPartConvGradPlan in kinds and mf.PartConvGradPlan not in kinds, "the backward took the fused plan"
    assert worst_row(y.detach().cpu().numpy().reshape(B * D, Lo), _torch_conv(x0, k0, mode).numpy().reshape(B * D, Lo)) <= REL_L2_TOL_F64
    assert worst_row(x.grad.cpu().numpy().reshape(B * D, L), xc.grad.numpy().reshape(B * D, L)) <= REL_L2_TOL_F64
    assert worst_row(k.grad.cpu().numpy(), kc.grad.numpy()) <= REL_L2_TOL_F64
    direct = mf.fftconv_filter_grad(x.detach(), gy0.to(DEV), K, block=n, partition=Q, mode=mode, fused=True)
    assert torch.equal(_bits(k.grad), _bits(direct)), "k.grad is fftconv_filter_grad(fused=True), bit for bit"


def test_gradcheck():
    n, Q, L, K, D, B = 16, 9, 23, 21, 2, 2
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((B, D, L), generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    k = torch.randn((D, K), generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    a = torch.randn((B, D, L), generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    with mf.fftconv_fused_filter_grad(True):
        assert torch.autograd.gradcheck(lambda x, k, a: mf.fftconv(x, k, block=n, partition=Q, pregate=a), (x, k, a), eps=1e-6,
                                        atol=1e-7, rtol=1e-6, nondet_tol=0.0)


# ---- the spectra in scratch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("correlate", [False, True])
def test_spectra_in_scratch(correlate):
    n, L, K, D, B = 16, 37, 29, 2, 2
    o, Lo = (0, L) if correlate else (6, 30)
    gen = torch.Generator().manual_seed(3)
    x, gy = torch.randn((B * D, L, 1), generator=gen, dtype=torch.float64), torch.randn((B * D, Lo, 1), generator=gen, dtype=torch.float64)
    plan = mf.plan_fftconv_grad(torch.float64, B, D, L, n, taps=K, partition=9, offset=o, out_length=Lo, correlate=correlate, fused=True)
    g = plan.geometry
    U, G = plan.spectra(x.to(DEV), gy.to(DEV))
    assert tuple(U.shape) == (B * D, g.Fu, n // 2 + 1) and tuple(G.shape) == (B * D, g.Fg, n // 2 + 1)
    # the frames, built on the CPU as the table of the geometry says
    xp = torch.nn.functional.pad(x[..., 0], (2 * n, 2 * n))
    frames = torch.stack([xp[:, 2 * n + g.frame_start(g.u_first + j):2 * n + g.frame_start(g.u_first + j) + n] for j in range(g.Fu)], 1)
    blocks = torch.zeros((B * D, g.Fg, n), dtype=torch.float64)
    for f in range(g.Fg):
        seg = gy[:, f * g.H:min(Lo, (f + 1) * g.H), 0]
        blocks[:, f, g.c:g.c + seg.shape[1]] = seg
    for got, ref in ((U, torch.fft.rfft(frames)), (G, torch.fft.rfft(blocks))):
        got = got.cpu()
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), float((got - ref).abs().max())
    plan.close()
