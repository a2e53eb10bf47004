"""Overlap-save fftconv on the device (plan_fftconv(taps=), fftconv(block=), long rows through fftconv; TileCfg::OLS): every
length class of the packed rows, odd steps (unaligned loads and stores), the crops of every mode, correlation and its
adjointness, impulses and seams index by index, agreement with the single-block kernel, slabs, three rounds of the persistent
grid with tiles that straddle signal rows, and the binding of the filter tensor.  The tolerance is the worst row's relative
l2 against the fp64 model of test_fftconv_long_host.py."""
import numpy as np
import pytest
import scipy.signal
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_long_host import geometry, ols_model

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


def _exec_canaried(plan, x, first=None, count=None):
    """exec into the middle of a larger buffer of canaries (a value no result has), which must stay what they were"""
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    if first is None:
        mf.fft(out, x, plan=plan)
    else:
        mf.fft(out, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == CANARY).all()) and bool((flat[GUARD + numel:] == CANARY).all()), "a canary was written"
    return out


def _model(x2d, k, n, offset, out_length, correlate=False):
    K = np.atleast_2d(k).shape[-1]
    c, S, s0, F = geometry(n, K, offset, out_length, correlate)
    return ols_model(x2d, k, n, c, S, s0, F, out_length, correlate)


LENGTHS = [(16, 100, 5, 1, 3, "f32"), (16, 101, 9, 2, 2, "f32"), (64, 1000, 33, 3, 2, "f32"), (96, 777, 40, 2, 3, "f32"),
           (1000, 5000, 300, 2, 1, "f32"), (2048, 20000, 1024, 3, 1, "f32"), (16384, 70000, 4097, 1, 2, "f32"),
           (64, 1000, 33, 3, 2, "f64"), (12288, 40000, 3000, 1, 1, "f64")]


@pytest.mark.parametrize("n,T,K,D,B,t", LENGTHS, ids=lambda v: str(v))
def test_lengths_against_the_model(n, T, K, D, B, t):
    dtype = DT[t]
    x, k = _data(n + T, B, D, T, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
    S = n - K + 1
    assert (plan.taps, plan.step, plan.blocks) == (K, S, -(-T // S))
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    name = plan.kernel_name(1)
    assert plan.kernel_name(0) == "none" and name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "") + "r2c_"), name
    assert name.endswith("_conv_ols_jit"), name
    assert plan.in_bytes == B * D * T * x.itemsize and plan.out_bytes == B * D * T * x.itemsize
    assert tuple(plan.filter_spectrum.shape) == (D, n // 2 + 1, 2)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    keep = xd.clone()
    out = _exec_canaried(plan, xd)
    assert torch.equal(_bits(xd), _bits(keep)), "x was written"
    err = _worst(out.cpu().numpy()[..., 0], _model(x.reshape(B * D, T), k, n, 0, T))
    print(f"fftconv ols n={n} T={T} K={K} D={D} B={B} {t} {name} blocks {plan.blocks} worst rel-L2 {err:.3e}")
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("T,K,n", [(333, 15, 16), (37, 28, 64)])
@pytest.mark.parametrize("mode", ["causal", "full", "same", "valid"])
def test_modes_against_scipy(T, K, n, mode):
    dtype = torch.float64
    B, D = 2, 3
    x, k = _data(T + K, B, D, T, K, dtype)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), mode=mode, block=n).cpu().numpy()
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
@pytest.mark.parametrize("T,K,n", [(333, 15, 16), (37, 28, 64)])
def test_correlation_and_adjointness(T, K, n, t):
    dtype = DT[t]
    D, B = 2, 3
    x, k = _data(31 + T, B, D, T, K, dtype)
    g = np.random.default_rng(32).standard_normal((B, D, T)).astype(NP[dtype])
    xd, kd, gd = (torch.from_numpy(a).to(DEV) for a in (x, k, g))
    c = mf.fftconv(gd, kd, block=n, correlate=True)
    gp = np.concatenate([g.astype(np.float64), np.zeros((B, D, K))], axis=-1)
    want = np.stack([np.stack([np.array([np.dot(k[d].astype(np.float64), gp[b, d, u:u + K]) for u in range(T)])
                               for d in range(D)]) for b in range(B)])
    assert _worst(c.cpu().numpy(), want) <= TOL[dtype]
    assert _worst(c.cpu().numpy().reshape(B * D, T), _model(g.reshape(B * D, T), k, n, 0, T, correlate=True)) <= TOL[dtype]
    y = mf.fftconv(xd, kd, block=n)
    lhs = float((y.double() * gd.double()).sum())
    rhs = float((xd.double() * c.double()).sum())
    scale = float(y.double().norm() * gd.double().norm())
    assert abs(lhs - rhs) <= TOL[dtype] * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_impulses_index_by_index(t):
    """x a unit impulse around a block seam and at both ends, k a unit impulse at its first and last tap: one sample of the
    full convolution is 1, at t0 + j0, and every other one 0 to tolerance"""
    dtype = DT[t]
    n, T, K = 64, 200, 33
    S = n - K + 1
    for t0 in (0, S - 1, S, S + 1, T - 1):
        for j0 in (0, K - 1):
            x = np.zeros((1, 1, T), dtype=NP[dtype])
            x[..., t0] = 1
            k = np.zeros((1, K), dtype=NP[dtype])
            k[0, j0] = 1
            y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), block=n, mode="full").cpu().numpy()[0, 0]
            want = np.zeros(T + K - 1)
            want[t0 + j0] = 1
            assert int(np.abs(y).argmax()) == t0 + j0, (t0, j0, int(np.abs(y).argmax()))
            assert np.linalg.norm(y - want) <= TOL[dtype], (t0, j0, np.linalg.norm(y - want))


@pytest.mark.parametrize("n,K", [(64, 33), (96, 40), (16, 9)])
def test_seams_of_a_constant_signal(n, K):
    """a constant signal against an all-ones filter: every output far from the ends is K; a sample dropped, doubled or
    shifted at a block seam is not.  (The bound per sample: a block's relative l2 within the tolerance is an absolute l2
    of at most tol * max|y| * sqrt(n), which bounds every one of its samples.)"""
    T = 20 * n + 3
    x = np.ones((2, 1, T), dtype=np.float32)
    k = np.ones((1, K), dtype=np.float32)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), block=n).cpu().numpy().reshape(2, T)
    mid = y[:, K - 1:]
    assert np.abs(mid - K).max() <= REL_L2_TOL_F32 * K * np.sqrt(n), np.abs(mid - K).max()
    # ... and a ramp, which a shifted block would break: y[t] = sum_j (t - j) = K t - K (K - 1) / 2 from t = K - 1 on
    x = np.broadcast_to(np.arange(T, dtype=np.float64), (2, 1, T)).copy()
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k.astype(np.float64)).to(DEV), block=n).cpu().numpy().reshape(2, T)
    u = np.arange(K - 1, T)
    want = K * u - K * (K - 1) / 2
    assert np.abs(y[:, K - 1:] - want).max() <= REL_L2_TOL_F64 * np.abs(want).max() * np.sqrt(n)


def test_agreement_with_the_single_block_kernel():
    T, K, D, B = 600, 33, 3, 2
    x, k = _data(71, B, D, T, K, torch.float32)
    xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV)
    one = mf.fftconv(xd, kd)
    for mode in ("causal", "full"):
        a, b = mf.fftconv(xd, kd, mode=mode), mf.fftconv(xd, kd, mode=mode, block=64)
        assert a.shape == b.shape
        assert _worst(b.cpu().numpy(), a.cpu().numpy()) <= REL_L2_TOL_F32
    assert _worst(mf.fftconv(xd, kd, block=64).cpu().numpy().reshape(B * D, T), _model(x.reshape(B * D, T), k, 64, 0, T)) <= REL_L2_TOL_F32
    assert tuple(one.shape) == (B, D, T)


def test_rows_beyond_one_fft_no_longer_raise():
    """T + K - 1 > 16384: overlap-save at fftconv_block(K), where the single-block path had to refuse"""
    T, K, D, B = 20000, 257, 2, 2
    x, k = _data(81, B, D, T, K, torch.float32)
    with pytest.raises(mf.MifftError):
        mf.fftconv_length(T + K - 1)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV))
    assert tuple(y.shape) == (B, D, T)
    want = np.stack([np.stack([scipy.signal.fftconvolve(x[b, d].astype(np.float64), k[d].astype(np.float64))[:T]
                               for d in range(D)]) for b in range(B)])
    assert _worst(y.cpu().numpy(), want) <= REL_L2_TOL_F32
    for mode in ("full", "same", "valid"):
        y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), mode=mode).cpu().numpy()
        want = np.stack([np.stack([scipy.signal.fftconvolve(x[b, d].astype(np.float64), k[d].astype(np.float64), mode=mode)
                                   for d in range(D)]) for b in range(B)])
        assert y.shape == want.shape and _worst(y, want) <= REL_L2_TOL_F32, mode


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_slabs_equal_the_whole_batch_bit_for_bit(t):
    dtype = DT[t]
    n, T, K, D, B = 64, 333, 28, 3, 7
    x, k = _data(41, B, D, T, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    whole = _exec_canaried(plan, xd)
    for first, count in ((1, 5), (4, 10), (11, 1), (20, 1), (2, 19)):  # first is no multiple of D = 3
        assert first % D != 0
        part = _exec_canaried(plan, xd, first=first, count=count)
        assert torch.equal(_bits(part[first:first + count]), _bits(whole[first:first + count])), (first, count)
        assert bool((part[:first] == CANARY).all()) and bool((part[first + count:] == CANARY).all()), (first, count)
    assert _worst(whole.cpu().numpy()[..., 0], _model(x.reshape(B * D, T), k, n, 0, T)) <= TOL[dtype]
    # the same signals in a batch of another size: the same bits
    small = mf.plan_fftconv(dtype, 2, D, T, n, taps=K)
    small.set_filter(torch.from_numpy(k).to(DEV))
    part = _exec_canaried(small, xd[3:9].contiguous())
    assert torch.equal(_bits(part), _bits(whole[3:9]))


def test_three_rounds_of_the_persistent_grid():
    """a batch sized by Plan.pass_geometry: two full rounds and a partial one with a ragged last tile; the blocks per signal
    do not divide the tile, so tiles straddle signal rows; every row checked"""
    dtype = torch.float32
    n, K, D = 64, 33, 3
    S = n - K + 1
    probe = mf.plan_fftconv(dtype, 2, D, 7 * S - 5, n, taps=K)
    tile, threads, _, G = probe.pass_geometry(1, 1 << 40)
    F = next(f for f in (7, 5, 3, 11) if tile % f != 0 and f % tile != 0) if tile > 1 else 7
    T = F * S - 5
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    rows = -(-((n_tiles - 1) * tile + max(1, tile // 3)) // F)  # signal rows
    rows += (-rows) % D
    while (tile > 1 and (rows * F) % tile == 0) or -(-rows * F // tile) % G == 0:
        rows += D
    B = rows // D
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
    assert plan.blocks == F
    geo = plan.pass_geometry(1)
    assert geo[:2] == (tile, threads) and geo[2] == -(-rows * F // tile), (geo, rows, F)
    assert geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0, geo
    x, k = _data(51, B, D, T, K, dtype)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    out = _exec_canaried(plan, torch.from_numpy(x).to(DEV).reshape(rows, T, 1))
    got, ref = out.cpu().numpy()[..., 0], _model(x.reshape(rows, T), k, n, 0, T)
    e = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    r = int(e.argmax())
    print(f"fftconv ols rounds: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows} x {F} blocks "
          f"worst rel-L2 {e[r]:.3e}")
    assert e[r] <= REL_L2_TOL_F32, (f"signal row {r}", e[r])


def test_the_filter_is_bound_by_address_and_limited_to_taps():
    dtype = torch.float32
    n, T, K, D, B = 96, 777, 40, 2, 3
    x, k1 = _data(61, B, D, T, K, dtype)
    k2 = np.random.default_rng(62).standard_normal((D, 7)).astype(np.float32)
    plan = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
    ptr = plan.filter_spectrum.data_ptr()
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, T, 1)
    xr = x.reshape(B * D, T)
    plan.set_filter(torch.from_numpy(k1).to(DEV))
    assert _worst(_exec_canaried(plan, xd).cpu().numpy()[..., 0], _model(xr, k1, n, 0, T)) <= REL_L2_TOL_F32
    plan.set_filter(torch.from_numpy(k2).to(DEV))  # (fewer taps than the plan's: the same blocks, zero-extended filter)
    k2p = np.concatenate([k2, np.zeros((D, K - 7), dtype=np.float32)], axis=1)
    assert _worst(_exec_canaried(plan, xd).cpu().numpy()[..., 0], _model(xr, k2p, n, 0, T)) <= REL_L2_TOL_F32
    assert plan.filter_spectrum.data_ptr() == ptr
    with pytest.raises(mf.MifftError) as e:
        plan.set_filter(torch.zeros(D, K + 1, device=DEV))
    assert "taps" in str(e.value)
    assert plan.filter_spectrum.data_ptr() == ptr
