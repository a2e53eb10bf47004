"""Partitioned fftconv on the device (plan_fftconv(taps=, partition=), fftconv(partition=); TileCfg::PART, the 20-word
payload): every length class of the packed rows against the fp64 model of test_fftconv_part_host.py, the crops of every mode,
correlation and its adjointness, impulses index by index across partition and block seams, agreement across partition sizes
and with the overlap-save kernel, NaN guards around a row, slabs and batches bit for bit, three rounds of the persistent grid,
gates and skip, autograd against torch CPU autograd over a direct convolution, and partition="auto".  Outputs lie between
canaries; inputs are compared bitwise before and after.  The n = 16384 / 12288 cases have one signal row."""
import numpy as np
import pytest
import scipy.signal
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_part_host import model, part_geometry

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 64  # canary elements on both sides of an output
CANARY = -7.25


def _worst(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max())


def _data(seed, B, D, T, K, dtype):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, D, T)).astype(NP[dtype]), rng.standard_normal((D, K)).astype(NP[dtype])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_canaried(plan, x, first=None, count=None, pregate=None, postgate=None):
    """exec into the middle of a larger buffer of canaries (a value no result has), which must stay what they were"""
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    kw = {} if first is None else dict(first=first, count=count)
    if plan.conv_gates:
        plan.run(out, x, pregate=pregate, postgate=postgate, **kw)
    else:
        mf.fft(out, x, plan=plan, **kw)
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == CANARY).all()) and bool((flat[GUARD + numel:] == CANARY).all()), "a canary was written"
    return out


LENGTHS = [(16, 100, 40, 5, 1, 3, "f32"), (16, 101, 101, 9, 2, 2, "f32"), (64, 1000, 1000, 33, 3, 2, "f32"),
           (96, 777, 300, 40, 2, 3, "f32"), (1000, 5000, 2500, 300, 2, 1, "f32"), (2048, 20000, 20000, 1025, 3, 1, "f32"),
           (16384, 40000, 40000, 8193, 1, 1, "f32"), (64, 1000, 1000, 33, 3, 2, "f64"), (12288, 30000, 20000, 6145, 1, 1, "f64")]


@pytest.mark.parametrize("n,T,K,Q,D,B,t", LENGTHS, ids=lambda v: str(v))
def test_lengths_against_the_model(n, T, K, Q, D, B, t):
    dtype = DT[t]
    x, k = _data(n + T, B, D, T, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=Q)
    S, P = n - Q + 1, -(-K // Q)
    assert (plan.taps, plan.partition, plan.partitions, plan.step, plan.blocks) == (K, Q, P, S, -(-T // S))
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    name = plan.kernel_name(1)
    assert plan.kernel_name(0) == "none" and name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "") + "r2c_"), name
    assert name.endswith("_conv_pols_jit"), name
    assert tuple(plan.filter_spectrum.shape) == (D, P, n // 2 + 1, 2)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    keep = xd.clone()
    out = _exec_canaried(plan, xd)
    assert torch.equal(_bits(xd), _bits(keep)), "x was written"
    err = _worst(out.cpu().numpy()[..., 0], model(x.reshape(B * D, T), k, n, Q, 0, T))
    print(f"fftconv pols n={n} T={T} K={K} Q={Q} D={D} B={B} {t} {name} blocks {plan.blocks} partitions {P} worst rel-L2 {err:.3e}")
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("T,K,n,Q", [(333, 200, 16, 15), (37, 90, 64, 28)])
@pytest.mark.parametrize("mode", ["causal", "full", "same", "valid"])
def test_modes_against_scipy(T, K, n, Q, mode):
    dtype = torch.float64
    B, D = 2, 3
    x, k = _data(T + K, B, D, T, K, dtype)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), mode=mode, block=n, partition=Q).cpu().numpy()
    full = np.stack([np.stack([np.convolve(x[b, d], k[d]) for d in range(D)]) for b in range(B)])
    if mode == "causal":
        want = full[..., :T]
    else:
        want = np.stack([np.stack([scipy.signal.fftconvolve(x[b, d], k[d], mode=mode) for d in range(D)]) for b in range(B)])
    assert y.shape == want.shape, (y.shape, want.shape)
    # (a crop is compared on the scale of its whole row: "valid" keeps a few samples of it)
    err = np.linalg.norm((y - want).reshape(B * D, -1), axis=1) / np.linalg.norm(full.reshape(B * D, -1), axis=1)
    assert err.max() <= REL_L2_TOL_F64, err.max()


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("T,K,n,Q", [(333, 200, 16, 15), (37, 90, 64, 28)])
def test_correlation_and_adjointness(T, K, n, Q, t):
    dtype = DT[t]
    D, B = 2, 3
    x, k = _data(31 + T, B, D, T, K, dtype)
    g = np.random.default_rng(32).standard_normal((B, D, T)).astype(NP[dtype])
    xd, kd, gd = (torch.from_numpy(a).to(DEV) for a in (x, k, g))
    c = mf.fftconv(gd, kd, block=n, partition=Q, correlate=True)
    gp = np.concatenate([g.astype(np.float64), np.zeros((B, D, K))], axis=-1)
    want = np.stack([np.stack([np.array([np.dot(k[d].astype(np.float64), gp[b, d, u:u + K]) for u in range(T)])
                               for d in range(D)]) for b in range(B)])
    assert _worst(c.cpu().numpy(), want) <= TOL[dtype]
    assert _worst(c.cpu().numpy().reshape(B * D, T), model(g.reshape(B * D, T), k, n, Q, 0, T, correlate=True)) <= TOL[dtype]
    y = mf.fftconv(xd, kd, block=n, partition=Q)
    lhs = float((y.double() * gd.double()).sum())
    rhs = float((xd.double() * c.double()).sum())
    scale = float(y.double().norm() * gd.double().norm())
    assert abs(lhs - rhs) <= TOL[dtype] * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_impulses_index_by_index(t):
    """x a unit impulse at a block seam and at both ends, k a unit impulse on either side of every partition seam: one sample
    of the full convolution is 1, at t0 + j0, and every other one 0 to tolerance -- what a partition shifted by one breaks"""
    dtype = DT[t]
    n, T, K, Q = 64, 200, 100, 33
    S = n - Q + 1
    for t0 in (0, S - 1, S, 3 * S + 1, T - 1):
        for j0 in (0, Q - 1, Q, 2 * Q - 1, 2 * Q, K - 1):
            x = np.zeros((1, 1, T), dtype=NP[dtype])
            x[..., t0] = 1
            k = np.zeros((1, K), dtype=NP[dtype])
            k[0, j0] = 1
            y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), block=n, partition=Q,
                           mode="full").cpu().numpy()[0, 0]
            want = np.zeros(T + K - 1)
            want[t0 + j0] = 1
            assert int(np.abs(y).argmax()) == t0 + j0, (t0, j0, int(np.abs(y).argmax()))
            assert np.linalg.norm(y - want) <= TOL[dtype], (t0, j0, np.linalg.norm(y - want))


def test_agreement_across_partition_sizes_and_with_overlap_save():
    T, K, D, B = 600, 33, 3, 2
    x, k = _data(71, B, D, T, K, torch.float32)
    xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV)
    for mode in ("causal", "full"):
        ols = mf.fftconv(xd, kd, mode=mode, block=64).cpu().numpy()  # (K <= n / 2 + 1: the plain overlap-save plan exists)
        a = mf.fftconv(xd, kd, mode=mode, block=64, partition=9).cpu().numpy()
        b = mf.fftconv(xd, kd, mode=mode, block=64, partition=20).cpu().numpy()
        assert a.shape == b.shape == ols.shape
        assert _worst(a, b) <= REL_L2_TOL_F32 and _worst(a, ols) <= REL_L2_TOL_F32 and _worst(b, ols) <= REL_L2_TOL_F32, mode


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_a_single_partition_against_the_overlap_save_plan(t):
    dtype = DT[t]
    n, T, K, D, B = 64, 333, 28, 3, 2
    x, k = _data(73, B, D, T, K, dtype)
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    ols = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
    one = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=K)
    assert one.partitions == 1 and (one.step, one.blocks) == (ols.step, ols.blocks)
    for p in (ols, one):
        p.set_filter(torch.from_numpy(k).to(DEV))
    assert _worst(_exec_canaried(one, xd).cpu().numpy()[..., 0], _exec_canaried(ols, xd).cpu().numpy()[..., 0]) <= TOL[dtype]


@pytest.mark.parametrize("correlate", [False, True])
def test_a_row_between_nan_guards(correlate):
    """one signal row in the middle of a buffer of NaN: an empty or partial block that loaded anything outside [0, T) would
    carry a NaN into the result"""
    dtype = torch.float32
    n, T, K, Q = 64, 150, 170, 33
    x, k = _data(75, 1, 1, T, K, dtype)
    pad = 4 * n
    flat = torch.full((T + 2 * pad,), float("nan"), dtype=dtype, device=DEV)
    flat[pad:pad + T] = torch.from_numpy(x.reshape(T)).to(DEV)
    xd = flat[pad:pad + T].view(1, T, 1)
    plan = mf.plan_fftconv(dtype, 1, 1, T, n, taps=K, partition=Q, correlate=correlate)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    out = _exec_canaried(plan, xd).cpu().numpy()[..., 0]
    assert not np.isnan(out).any()
    assert _worst(out, model(x.reshape(1, T), k, n, Q, 0, T, correlate=correlate)) <= REL_L2_TOL_F32


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_slabs_batches_and_runs_equal_bit_for_bit(t):
    dtype = DT[t]
    n, T, K, Q, D, B = 64, 333, 200, 28, 3, 7
    x, k = _data(41, B, D, T, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=Q)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    whole = _exec_canaried(plan, xd)
    assert torch.equal(_bits(_exec_canaried(plan, xd)), _bits(whole)), "two runs of one plan"
    for first, count in ((1, 5), (4, 10), (11, 1), (20, 1), (2, 19)):  # first is no multiple of D = 3
        assert first % D != 0
        part = _exec_canaried(plan, xd, first=first, count=count)
        assert torch.equal(_bits(part[first:first + count]), _bits(whole[first:first + count])), (first, count)
        assert bool((part[:first] == CANARY).all()) and bool((part[first + count:] == CANARY).all()), (first, count)
    assert _worst(whole.cpu().numpy()[..., 0], model(x.reshape(B * D, T), k, n, Q, 0, T)) <= TOL[dtype]
    # the same signals in a batch of another size: the same bits
    small = mf.plan_fftconv(dtype, 2, D, T, n, taps=K, partition=Q)
    small.set_filter(torch.from_numpy(k).to(DEV))
    part = _exec_canaried(small, xd[3:9].contiguous())
    assert torch.equal(_bits(part), _bits(whole[3:9]))


def test_three_rounds_of_the_persistent_grid():
    """a batch sized by Plan.pass_geometry: two full rounds and a partial one with a ragged last tile; the blocks per signal
    do not divide the tile, so tiles straddle signal rows; every row checked"""
    dtype = torch.float32
    n, Q, D = 64, 33, 3
    S = n - Q + 1
    probe = mf.plan_fftconv(dtype, 2, D, 7 * S - 5, n, taps=2 * Q + 5, partition=Q)
    tile, threads, _, G = probe.pass_geometry(1, 1 << 40)
    F = next(f for f in (7, 5, 3, 11) if tile % f != 0 and f % tile != 0) if tile > 1 else 7
    T = F * S - 5
    K = 2 * Q + 5  # three partitions, the last one short
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    rows = -(-((n_tiles - 1) * tile + max(1, tile // 3)) // F)  # signal rows
    rows += (-rows) % D
    while (tile > 1 and (rows * F) % tile == 0) or -(-rows * F // tile) % G == 0:
        rows += D
    B = rows // D
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=Q)
    assert plan.blocks == F and plan.partitions == 3
    geo = plan.pass_geometry(1)
    assert geo[:2] == (tile, threads) and geo[2] == -(-rows * F // tile), (geo, rows, F)
    assert geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0, geo
    x, k = _data(51, B, D, T, K, dtype)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    out = _exec_canaried(plan, torch.from_numpy(x).to(DEV).reshape(rows, T, 1))
    got, ref = out.cpu().numpy()[..., 0], model(x.reshape(rows, T), k, n, Q, 0, T)
    e = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    r = int(e.argmax())
    print(f"fftconv pols rounds: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows} x {F} blocks "
          f"worst rel-L2 {e[r]:.3e}")
    assert e[r] <= REL_L2_TOL_F32, (f"signal row {r}", e[r])


@pytest.mark.parametrize("gates", [1, 2, 3])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_gates_equal_the_ungated_kernel_bit_for_bit(gates, t):
    dtype = DT[t]
    n, T, K, Q, D, B = 64, 333, 200, 28, 3, 2  # (odd S = 37: unaligned pairs of x and gate alike)
    x, k = _data(91, B, D, T, K, dtype)
    rng = np.random.default_rng(92)
    a, b = (rng.standard_normal((B * D, T, 1)).astype(NP[dtype]) for _ in range(2))
    xd, ad, bd = (torch.from_numpy(v).to(DEV).reshape(B * D, T, 1) for v in (x, a, b))
    plain = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=Q)
    gated = mf.plan_fftconv(dtype, B, D, T, n, taps=K, partition=Q, pregate=bool(gates & 1), postgate=bool(gates & 2))
    assert gated.kernel_name(1).endswith(f"_conv_pols_g{gates}_jit") and gated.num_launches == 1 and gated.scratch_bytes == 0
    for p in (plain, gated):
        p.set_filter(torch.from_numpy(k).to(DEV))
    want = _exec_canaried(plain, ad * xd if gates & 1 else xd)
    if gates & 2:
        want = bd * want
    keep = [_bits(v).clone() for v in (xd, ad, bd)]
    got = _exec_canaried(gated, xd, pregate=ad if gates & 1 else None, postgate=bd if gates & 2 else None)
    assert torch.equal(_bits(got), _bits(want))
    assert all(torch.equal(_bits(v), w) for v, w in zip((xd, ad, bd), keep)), "an input was written"


def test_skip_is_d_times_the_gated_input():
    dtype = torch.float64
    T, K, Q, D, B = 333, 200, 28, 3, 2
    x, k = _data(95, B, D, T, K, dtype)
    rng = np.random.default_rng(96)
    a, d = rng.standard_normal((B, D, T)), rng.standard_normal(D)
    xd, kd, ad, dd = (torch.from_numpy(v).to(DEV) for v in (x, k, a, d))
    got = mf.fftconv(xd, kd, block=64, partition=Q, pregate=ad, skip=dd).cpu().numpy()
    want = mf.fftconv(xd, kd, block=64, partition=Q, pregate=ad).cpu().numpy() + d[None, :, None] * (a * x)
    assert _worst(got, want) <= REL_L2_TOL_F64


# ---- autograd against torch CPU fp64 autograd over a direct convolution ----------------------------------------------------------
def _direct(x, k, a, b, d, o, Lo, correlate):
    """b * (crop(conv(a x, k)) + d * crop(a x)) with torch's direct conv1d, fp64 on the CPU; x (B, D, L), k (D, K)"""
    D, K = k.shape
    L = x.shape[-1]
    u = x if a is None else a * x
    if correlate:  # y[t] = sum_j k[j] u[t + j]
        full = torch.nn.functional.conv1d(torch.nn.functional.pad(u, (0, K - 1)), k.reshape(D, 1, K), groups=D)
        up = u
    else:
        full = torch.nn.functional.conv1d(torch.nn.functional.pad(u, (K - 1, K - 1)), k.flip(-1).reshape(D, 1, K), groups=D)
        up = torch.nn.functional.pad(u, (0, K - 1))
    y = full[..., o:o + Lo]
    if d is not None:
        y = y + d.reshape(1, D, 1) * up[..., o:o + Lo]
    return y if b is None else b * y


@pytest.mark.parametrize("T,K,n,Q", [(100, 150, 16, 9), (333, 200, 64, 33)])
@pytest.mark.parametrize("mode,correlate", [("causal", False), ("full", False), ("same", False), ("valid", False), ("causal", True)])
def test_autograd_against_a_direct_convolution(T, K, n, Q, mode, correlate):
    dtype = torch.float64
    rng = np.random.default_rng(T + K + len(mode))
    B, D = 2, 2
    o, Lo = mf.api._fftconv_window(mode, T, K)
    x, a = rng.standard_normal((B, D, T)), rng.standard_normal((B, D, T))
    b, gy = rng.standard_normal((B, D, Lo)), rng.standard_normal((B, D, Lo))
    k, d = rng.standard_normal((D, K)), rng.standard_normal(D)
    cpu = [torch.from_numpy(v).requires_grad_(True) for v in (x, k, a, b, d)]
    yref = _direct(cpu[0], cpu[1], cpu[2], cpu[3], cpu[4], o, Lo, correlate)
    yref.backward(torch.from_numpy(gy))
    dev = [torch.from_numpy(v).to(DEV).requires_grad_(True) for v in (x, k, a, b, d)]
    y = mf.fftconv(dev[0], dev[1], mode=mode, correlate=correlate, block=n, partition=Q, pregate=dev[2], postgate=dev[3], skip=dev[4])
    assert y.grad_fn is not None and y.dtype == dtype
    y.backward(torch.from_numpy(gy).to(DEV))
    full = _direct(cpu[0].detach(), cpu[1].detach(), cpu[2].detach(), None, cpu[4].detach(), 0, T if correlate else T + K - 1, correlate)
    err = (y.detach().cpu() - yref.detach()).reshape(B * D, -1).norm(dim=1) / (cpu[3].detach().abs().max() * full.reshape(B * D, -1).norm(dim=1))
    assert float(err.max()) <= TOL[dtype], float(err.max())  # (a crop on the scale of its whole row)
    for name, tdev, tcpu in zip(("x", "k", "pregate", "postgate", "skip"), dev, cpu):
        assert tdev.grad is not None and tdev.grad.shape == tdev.shape and tdev.grad.dtype == dtype, name
        got, ref = tdev.grad.cpu().numpy(), tcpu.grad.numpy()
        err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print(f"{mode} {name}: rel l2 {err:.3e}")
        assert err <= TOL[dtype], (name, err)


def test_gradcheck():
    g = torch.Generator(device=DEV).manual_seed(21)
    B, D, L, K = 1, 2, 20, 30
    mk = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float64).requires_grad_(True)
    x, k, a, b, d = mk(B, D, L), mk(D, K), mk(B, D, L), mk(B, D, L), mk(D)
    fn = lambda x, k, a, b, d: mf.fftconv(x, k, pregate=a, postgate=b, skip=d, block=16, partition=5)
    assert torch.autograd.gradcheck(fn, (x, k, a, b, d), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("correlate", [False, True])
def test_the_filter_gradient_against_the_model(correlate, t):
    """gk[d, j] = sum over b and t of gy[b, d, t] u[b, d, t - j] (correlation: t + j): the fp64 model is the adjoint of the
    forward model, column by column of the filter: <gy, conv(u, e_j)>"""
    dtype = DT[t]
    T, K, n, Q, D, B = 100, 150, 16, 9, 2, 3
    rng = np.random.default_rng(3)
    x, gy = rng.standard_normal((B, D, T)).astype(NP[dtype]), rng.standard_normal((B, D, T)).astype(NP[dtype])
    xl, gl = x.astype(np.float64), gy.astype(np.float64)
    xp = np.concatenate([np.zeros((B, D, K)), xl, np.zeros((B, D, K))], axis=-1)
    want = np.array([[sum(np.dot(gl[b, d], xp[b, d, K + j:K + j + T] if correlate else xp[b, d, K - j:K - j + T]) for b in range(B))
                      for j in range(K)] for d in range(D)])
    got = mf.fftconv_filter_grad(torch.from_numpy(x).to(DEV), torch.from_numpy(gy).to(DEV), K, block=n, partition=Q, correlate=correlate)
    assert tuple(got.shape) == (D, K) and got.dtype == dtype
    # (the model's own forward is its adjoint: <gy, model(x, e_j)> for a few taps across partition seams)
    for j in (0, Q - 1, Q, 5 * Q, K - 1):
        e = np.zeros((D, K))
        e[:, j] = 1
        y = model(xl.reshape(B * D, T), e, n, Q, 0, T, correlate=correlate).reshape(B, D, T)
        assert np.abs((gl * y).sum(axis=(0, 2)) - want[:, j]).max() <= 1e-12 * np.abs(want).max(), j
    err = _worst(got.cpu().numpy(), want)
    print(f"partitioned filter gradient correlate={correlate} {t}: rel l2 {err:.3e}")
    assert err <= TOL[dtype], err
    plan = mf.plan_fftconv_grad(dtype, B, D, T, n, taps=K, partition=Q, correlate=correlate)
    assert (plan.partition, plan.partitions, plan.step) == (Q, -(-K // Q), n - Q + 1)
    again = plan.filter_grad(torch.from_numpy(x).to(DEV).reshape(B * D, T, 1), torch.from_numpy(gy).to(DEV).reshape(B * D, T, 1), K)
    assert torch.equal(_bits(again), _bits(got)), "two runs give the same bits"


def test_the_filter_gradient_of_an_impulse_pair_across_a_partition_seam():
    n, T, K, Q = 64, 200, 100, 33
    for s, t0 in ((0, Q - 1), (0, Q), (5, Q + 5), (5, Q + 4), (50, 50 + 2 * Q), (50, 50 + 2 * Q - 1), (100, 199), (0, 0), (199, 199)):
        x, gy = torch.zeros(1, 1, T, dtype=torch.float64, device=DEV), torch.zeros(1, 1, T, dtype=torch.float64, device=DEV)
        x[..., s], gy[..., t0] = 1, 1
        gk = mf.fftconv_filter_grad(x, gy, K, block=n, partition=Q).cpu().numpy()[0]
        want = np.zeros(K)
        if 0 <= t0 - s < K:
            want[t0 - s] = 1
        assert np.abs(gk - want).max() <= 1e-13, (s, t0)


# ---- partition="auto" ------------------------------------------------------------------------------------------------------------
def test_auto_is_the_existing_path_where_there_is_one():
    for T, K, kw in ((600, 33, {}), (600, 33, dict(block=64)), (20000, 257, {}), (20000, 257, dict(mode="full"))):
        x, k = _data(T + K, 2, 2, T, K, torch.float32)
        xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV)
        assert torch.equal(_bits(mf.fftconv(xd, kd, partition="auto", **kw)), _bits(mf.fftconv(xd, kd, **kw))), (T, K, kw)


def test_auto_runs_a_filter_as_long_as_the_row():
    T = K = 20000
    x, k = _data(83, 1, 2, T, K, torch.float32)
    xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV)
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(xd, kd)
    assert e.value.status == -15 and "partition=" in str(e.value)
    y = mf.fftconv(xd, kd, partition="auto")
    assert tuple(y.shape) == (1, 2, T)
    want = np.stack([scipy.signal.fftconvolve(x[0, d].astype(np.float64), k[d].astype(np.float64))[:T] for d in range(2)])[None]
    err = _worst(y.cpu().numpy(), want)
    print(f"fftconv auto T = K = {T}: worst rel-L2 {err:.3e}")
    assert err <= REL_L2_TOL_F32, err
