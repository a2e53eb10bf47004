"""The fused FFT convolution on the device (mf.fftconv, mf.plan_fftconv; TileCfg::CONV): every length class of the packed
rows, odd and circular lengths, impulses index by index, the crops of every mode, the unaligned store, correlation and its
adjointness, slabs, three rounds of the persistent grid, and the binding of the filter tensor.  The tolerance is the worst
row's relative l2 against the fp64 reference of test_fftconv_host.py."""
import numpy as np
import pytest
import scipy.signal
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_host import ref_fftconv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 64  # canary elements on both sides of an output


def _worst(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max())


def _data(seed, B, D, L, K, dtype):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, D, L)).astype(NP[dtype]), rng.standard_normal((D, K)).astype(NP[dtype])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_canaried(plan, x, first=None, count=None):
    """exec into the middle of a larger buffer of canaries (a value no result has), which must stay what they were"""
    numel = int(np.prod(plan.out_shape))
    canary = -7.25
    flat = torch.full((numel + 2 * GUARD,), canary, dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    if first is None:
        mf.fft(out, x, plan=plan)
    else:
        mf.fft(out, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == canary).all()) and bool((flat[GUARD + numel:] == canary).all()), "a canary was written"
    return out


LENGTHS = [(16, 8, 5, 1, 3, "f32"), (64, 37, 28, 3, 5, "f32"), (96, 50, 40, 2, 4, "f32"), (1000, 600, 300, 4, 2, "f32"),
           (2048, 1024, 1024, 3, 2, "f32"), (16384, 8192, 8192, 2, 2, "f32"), (12288, 6000, 6000, 2, 1, "f64"),
           (64, 37, 28, 3, 5, "f64"), (2048, 1024, 1024, 3, 2, "f64")]


@pytest.mark.parametrize("n,L,K,D,B,t", LENGTHS, ids=lambda v: str(v))
def test_lengths_against_the_reference(n, L, K, D, B, t):
    dtype = DT[t]
    x, k = _data(n + L, B, D, L, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, L, n)
    assert plan.num_launches == 1 and plan.scratch_bytes == 0 and "_conv" in plan.kernel_name(1), plan.kernel_name(1)
    assert plan.kernel_name(0) == "none" and plan.kernel_name(1).startswith(f"rows{n}_" + ("f64_" if t == "f64" else "") + "r2c_")
    assert plan.in_bytes == B * D * L * x.itemsize and plan.out_bytes == B * D * L * x.itemsize
    assert tuple(plan.filter_spectrum.shape) == (D, n // 2 + 1, 2) and not bool(plan.filter_spectrum.any())
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, L, 1)
    keep = xd.clone()
    out = _exec_canaried(plan, xd)
    assert torch.equal(_bits(xd), _bits(keep)), "x was written"
    err = _worst(out.cpu().numpy()[..., 0], ref_fftconv(x.reshape(B * D, L), k, n))
    print(f"fftconv n={n} L={L} K={K} D={D} B={B} {t} {plan.kernel_name(1)} worst rel-L2 {err:.3e}")
    assert err <= TOL[dtype], err
    # the one-call wrapper: the same kernel through the plan cache
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), n=n)
    assert tuple(y.shape) == (B, D, L)
    assert _worst(y.cpu().numpy(), ref_fftconv(x.reshape(B * D, L), k, n).reshape(B, D, L)) <= TOL[dtype]


def test_circular_when_n_is_short():
    n, L, K, D, B = 1024, 1024, 1024, 2, 2
    x, k = _data(7, B, D, L, K, torch.float32)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), n=n)
    assert _worst(y.cpu().numpy().reshape(B * D, L), ref_fftconv(x.reshape(B * D, L), k, n)) <= REL_L2_TOL_F32


def test_default_length_and_1d_filter():
    x = np.random.default_rng(11).standard_normal((5, 100)).astype(np.float32)
    k = np.random.default_rng(12).standard_normal(31).astype(np.float32)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV))
    want = np.stack([np.convolve(r.astype(np.float64), k.astype(np.float64))[:100] for r in x])
    assert _worst(y.cpu().numpy(), want) <= REL_L2_TOL_F32


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_impulses_index_by_index(t):
    dtype = DT[t]
    n, L, K, D = 64, 37, 20, 3
    tol = TOL[dtype]
    k = np.random.default_rng(21).standard_normal((D, K)).astype(NP[dtype])
    kd = torch.from_numpy(k).to(DEV)
    for p in (0, 1, L - 1):  # a unit impulse at p returns k shifted by p
        x = np.zeros((2, D, L), dtype=NP[dtype])
        x[:, :, p] = 1
        y = mf.fftconv(torch.from_numpy(x).to(DEV), kd, n=n, mode="full").cpu().numpy()
        want = np.zeros((2, D, L + K - 1))
        want[:, :, p:p + K] = k
        assert np.abs(y - want).max() <= tol * np.abs(k).max() * np.sqrt(K), (p, np.abs(y - want).max())
    # k[d] a unit impulse at lag d + 1: every row shifted by its own channel's lag (the r % D mapping)
    x = np.random.default_rng(22).standard_normal((3, D, L)).astype(NP[dtype])
    k = np.zeros((D, D + 1), dtype=NP[dtype])
    for d in range(D):
        k[d, d + 1] = 1
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), n=n).cpu().numpy()
    for d in range(D):
        want = np.zeros((3, L))
        want[:, d + 1:] = x[:, d, :L - d - 1]
        assert np.abs(y[:, d] - want).max() <= tol * np.abs(x).max() * np.sqrt(L), (d, np.abs(y[:, d] - want).max())


@pytest.mark.parametrize("L,K", [(37, 28), (50, 40)])
@pytest.mark.parametrize("mode", ["full", "same", "valid"])
def test_modes_against_scipy(L, K, mode):
    dtype = torch.float64
    B, D = 2, 3
    x, k = _data(L + K, B, D, L, K, dtype)
    y = mf.fftconv(torch.from_numpy(x).to(DEV), torch.from_numpy(k).to(DEV), mode=mode).cpu().numpy()
    want = np.stack([np.stack([scipy.signal.fftconvolve(x[b, d], k[d], mode=mode) for d in range(D)]) for b in range(B)])
    assert y.shape == want.shape, (y.shape, want.shape)
    full = np.stack([np.stack([np.convolve(x[b, d], k[d]) for d in range(D)]) for b in range(B)])
    # (a crop is compared on the scale of its whole row: "valid" keeps a few samples of it)
    err = np.linalg.norm((y - want).reshape(B * D, -1), axis=1) / np.linalg.norm(full.reshape(B * D, -1), axis=1)
    assert err.max() <= REL_L2_TOL_F64, err.max()


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("o,Lo", [(3, 17), (0, 63), (5, 32), (1, 1), (63, 1), (0, 64)])
def test_crops_and_the_unaligned_store(o, Lo, t):
    """odd offsets and odd lengths take the real-by-real store; canaries around the output stay untouched"""
    dtype = DT[t]
    n, L, K, D, B = 64, 37, 28, 3, 5
    x, k = _data(o * 64 + Lo, B, D, L, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, L, n, offset=o, out_length=Lo)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    out = _exec_canaried(plan, torch.from_numpy(x).to(DEV).reshape(B * D, L, 1))
    got = out.cpu().numpy()[..., 0]
    whole = ref_fftconv(x.reshape(B * D, L), k, n, 0, n)
    err = np.linalg.norm(got - whole[:, o:o + Lo], axis=1) / np.linalg.norm(whole, axis=1)
    assert err.max() <= TOL[dtype], err.max()


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_correlation_and_adjointness(t):
    dtype = DT[t]
    n, L, K, D, B = 96, 50, 40, 2, 4
    x, k = _data(31, B, D, L, K, dtype)
    g = np.random.default_rng(32).standard_normal((B, D, L)).astype(NP[dtype])
    xd, kd, gd = (torch.from_numpy(a).to(DEV) for a in (x, k, g))
    c = mf.fftconv(gd, kd, n=n, correlate=True)
    assert _worst(c.cpu().numpy().reshape(B * D, L), ref_fftconv(g.reshape(B * D, L), k, n, correlate=True)) <= TOL[dtype]
    y = mf.fftconv(xd, kd, n=n)
    lhs = float((y.double() * gd.double()).sum())
    rhs = float((xd.double() * c.double()).sum())
    scale = float(y.double().norm() * gd.double().norm())
    assert abs(lhs - rhs) <= TOL[dtype] * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_slabs_equal_the_whole_batch_bit_for_bit(t):
    dtype = DT[t]
    n, L, K, D, B = 64, 37, 28, 3, 7
    x, k = _data(41, B, D, L, K, dtype)
    plan = mf.plan_fftconv(dtype, B, D, L, n)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, L, 1)
    whole = _exec_canaried(plan, xd)
    for first, count in ((1, 5), (4, 10), (11, 1), (20, 1), (2, 19)):  # first is no multiple of D = 3
        assert first % D != 0
        part = _exec_canaried(plan, xd, first=first, count=count)
        assert torch.equal(_bits(part[first:first + count]), _bits(whole[first:first + count])), (first, count)
        assert bool((part[:first] == -7.25).all()) and bool((part[first + count:] == -7.25).all()), (first, count)
    assert _worst(whole.cpu().numpy()[..., 0], ref_fftconv(x.reshape(B * D, L), k, n)) <= TOL[dtype]


def test_three_rounds_of_the_persistent_grid():
    """a batch sized by Plan.pass_geometry: two full rounds and a partial one with a ragged last tile, every row checked"""
    dtype = torch.float32
    n, L, K, D = 64, 37, 28, 3
    probe = mf.plan_fftconv(dtype, 2, D, L, n)
    tile, threads, _, G = probe.pass_geometry(1, 1 << 40)
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    rows = (n_tiles - 1) * tile + max(1, tile // 3)
    rows += (-rows) % D
    while tile > 1 and rows % tile == 0:
        rows += D
    B = rows // D
    plan = mf.plan_fftconv(dtype, B, D, L, n)
    geo = plan.pass_geometry(1)
    assert geo[:2] == (tile, threads) and geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0, geo
    x, k = _data(51, B, D, L, K, dtype)
    plan.set_filter(torch.from_numpy(k).to(DEV))
    out = _exec_canaried(plan, torch.from_numpy(x).to(DEV).reshape(rows, L, 1))
    got, ref = out.cpu().numpy()[..., 0], ref_fftconv(x.reshape(rows, L), k, n)
    e = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    r = int(e.argmax())
    print(f"fftconv rounds: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows} worst rel-L2 {e[r]:.3e}")
    assert e[r] <= REL_L2_TOL_F32, (f"row {r} tile {r // tile} round {r // tile // geo[3]}", e[r])


def test_the_filter_is_bound_by_address_not_by_value():
    dtype = torch.float32
    n, L, K, D, B = 96, 50, 40, 2, 4
    x, k1 = _data(61, B, D, L, K, dtype)
    k2 = np.random.default_rng(62).standard_normal((D, 7)).astype(np.float32)
    plan = mf.plan_fftconv(dtype, B, D, L, n)
    ptr = plan.filter_spectrum.data_ptr()
    xd = torch.from_numpy(x).to(DEV).reshape(B * D, L, 1)
    xr = x.reshape(B * D, L)
    zero = _exec_canaried(plan, xd)
    assert not bool(zero.any())  # (the spectrum starts zero-filled)
    plan.set_filter(torch.from_numpy(k1).to(DEV))
    assert _worst(_exec_canaried(plan, xd).cpu().numpy()[..., 0], ref_fftconv(xr, k1, n)) <= REL_L2_TOL_F32
    plan.set_filter(torch.from_numpy(k2).to(DEV))
    assert _worst(_exec_canaried(plan, xd).cpu().numpy()[..., 0], ref_fftconv(xr, k2, n)) <= REL_L2_TOL_F32
    # a spectrum the caller already holds, here that of the first filter computed in fp64
    H = np.fft.rfft(k1.astype(np.float64), n, axis=-1)
    plan.set_filter_spectrum(torch.from_numpy(H).to(DEV))
    assert _worst(_exec_canaried(plan, xd).cpu().numpy()[..., 0], ref_fftconv(xr, k1, n)) <= REL_L2_TOL_F32
    assert plan.filter_spectrum.data_ptr() == ptr
    with pytest.raises(mf.MifftError):
        plan.set_filter(torch.zeros(D, n + 1, device=DEV))
    with pytest.raises(mf.MifftError):
        plan.set_filter(torch.zeros(D + 1, 4, device=DEV))
