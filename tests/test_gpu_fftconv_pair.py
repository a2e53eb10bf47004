"""The convolution / correlation of two signal batches on the device (plan_fftconv_pair, fftconv_pair; TileCfg::PAIR): one FFT
length per configuration class of the packed rows, impulses index by index, the modes, the separation of rows, slabs and
rounds of the persistent grid, adjointness of the plans the backward builds, and autograd against torch on the host.

Every output lies between guards of NaN and starts as NaN; every input comes back bit for bit (the helpers' pattern of
tests/test_gpu_packed_families.py).  The reference is the fp64 model of tests/test_fftconv_pair_host.py; errors are the worst
row's relative l2 against conftest's REL_L2_TOL_F32 / REL_L2_TOL_F64 and nothing else, the impulses |diff| <= 1e-13."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_pair_host import MODES, adjoints_of, ref_pair, window_of
from test_gpu_packed_lengths import CLASSES, _ids, _radices
from test_packed_families_host import full_and_ragged, single_shape

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}
TOL = {"f32": REL_L2_TOL_F32, "f64": REL_L2_TOL_F64}
FAR = 1 << 40  # a count at which no grid is clamped by the tile count
GUARD = 64     # NaN elements on both sides of every output

# one FFT length per configuration class (tests/test_gpu_packed_lengths.py), and the longest fp32 row, which that table lacks
PAIR_CLASSES = {k: CLASSES[k] for k in (("f32", 14), ("f32", 50), ("f32", 192), ("f32", 2058), ("f32", 4802), ("f32", 12288),
                                        ("f64", 14), ("f64", 66), ("f64", 2058), ("f64", 12288))}
PAIR_CLASSES[("f32", 16384)] = ((16, 8, 8, 8), 1, 1024)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _between(shape, dtype):
    """a NaN-prefilled tensor of `shape` in the middle of a buffer of NaN: (whole, view)"""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def _run(plan, x, v, slabs=None, written=True):
    """the exec of a pair plan (whole, or the (first, count) slabs) -> out (rows, Lo), between guards, the inputs untouched"""
    flat, out = _between(plan.out_shape, x.dtype)
    ins = [x] if v is x else [x, v]
    keep = [_bits(t).clone() for t in ins]
    if slabs is None:
        plan.run(out, x, v)
    else:
        for first, count in slabs:
            plan.run(out, x, v, first=first, count=count)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all()), "a guard beside the output was written"
    for t, k in zip(ins, keep):
        assert torch.equal(_bits(t), k), "an input was written"
    if written:
        assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    return out[..., 0]


def _normal(seed, shape, dtype):
    """standard-normal values rounded to `dtype` on the device, and the same values in float64 on the host"""
    v = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).to(dtype)
    return v.to(DEV), v.double().numpy()


def _worst(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max())


def _plan(t, R, L, K, n, ea, eb, o, Lo, corr):
    return mf.plan_fftconv_pair(DT[t], R, L, K, n, x_offset=ea, v_offset=eb, offset=o, out_length=Lo, correlate=corr)


# ---- 1. one length per class ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corr", [False, True], ids=["convolve", "correlate"])
@pytest.mark.parametrize("tn", list(PAIR_CLASSES), ids=_ids)
def test_length_classes(tn, corr):
    t, n = tn
    radices, tile, threads = PAIR_CLASSES[tn]
    L, K, o, Lo = single_shape(n)  # (L odd, K = n + 1 - L even: K > L exactly where n / 2 is odd)
    assert L % 2 == 1 and L != K and (K > L) == (n // 2 % 2 == 1)
    ea = K - 1 if corr else 0
    R = full_and_ragged(tile)
    plan = _plan(t, R, L, K, n, ea, 0, o, Lo, corr)
    name, geo = plan.kernel_name(1), plan.pass_geometry(1)
    text = f"{name} tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]}"
    assert name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "")) and name.endswith("_conv_pair_jit"), text
    assert _radices(name) == radices and geo[0] == tile and geo[1] == threads, (text, PAIR_CLASSES[tn])
    assert geo[2] == 3 and (tile == 1 or R % tile) and plan.kernel_name(0) == "none", text
    assert plan.num_launches == 1 and plan.scratch_bytes == 0, text
    esz = 4 if t == "f32" else 8
    assert plan.in_bytes == R * L * esz and plan.out_bytes == R * Lo * esz, text
    x, xh = _normal(n, (R, L, 1), DT[t])
    v, vh = _normal(n + 1, (R, K, 1), DT[t])
    got = _run(plan, x, v).cpu().numpy()
    err = _worst(got, ref_pair(xh[..., 0], vh[..., 0], n, ea, 0, o, Lo, corr))
    print(f"pair-lengths {t} n={n} corr={corr}: err {err:.3e} {text}")
    assert err <= TOL[t], (t, n, corr, err, text)


# ---- 2. impulses, index by index ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corr", [False, True], ids=["convolve", "correlate"])
@pytest.mark.parametrize("n,ea,eb,o,Lo", [(64, 0, 0, 0, 64), (64, 5, 3, 7, 33), (64, 27, 36, 1, 63), (64, 0, 0, 36, 1),
                                          (48, 0, 0, 0, 48), (48, 11, 20, 3, 37)])
def test_impulses(n, ea, eb, o, Lo, corr):
    """x = delta_s, v = delta_j: one 1 at index (ea + s + eb + j) mod n (correlation: ea + s - eb - j), or zeros where that index
    lies outside the window; n = 48 < L + K - 1 = 64 wraps"""
    L, K = 37, 28
    S, J = (0, L - 1, 17), (0, K - 1, 10)
    pairs = [(s, j) for s in S for j in J]
    xh, vh = np.zeros((len(pairs), L)), np.zeros((len(pairs), K))
    want = np.zeros((len(pairs), Lo))
    hits = 0
    for r, (s, j) in enumerate(pairs):
        xh[r, s] = vh[r, j] = 1.0
        p = (ea + s - eb - j) % n if corr else (ea + s + eb + j) % n
        if o <= p < o + Lo:
            want[r, p - o] = 1.0
            hits += 1
    assert np.array_equal(want, np.round(ref_pair(xh, vh, n, ea, eb, o, Lo, corr)))  # (the model's index)
    assert hits >= 1
    x, v = torch.from_numpy(xh).to(DEV).reshape(-1, L, 1), torch.from_numpy(vh).to(DEV).reshape(-1, K, 1)
    got = _run(_plan("f64", len(pairs), L, K, n, ea, eb, o, Lo, corr), x, v).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-13, (n, ea, eb, o, Lo, corr, np.abs(got - want).max())


# ---- 3. the modes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("L,K", [(37, 28), (28, 37)])
def test_modes(L, K, t):
    x, xh = _normal(L, (3, 2, L), DT[t])
    v, vh = _normal(K + 100, (3, 2, K), DT[t])
    n = mf.fftconv_length(L + K - 1, DT[t])
    for corr in (False, True):
        for mode in MODES:
            ea, eb, o, Lo = window_of(mode, L, K, corr)
            got = mf.fftconv_pair(x, v, mode=mode, correlate=corr)
            assert got.shape == (3, 2, Lo) and got.dtype == DT[t] and got.grad_fn is None
            err = _worst(got.cpu().numpy().reshape(6, Lo), ref_pair(xh, vh, n, ea, eb, o, Lo, corr).reshape(6, Lo))
            assert err <= TOL[t], (mode, corr, err)
    # a smaller n: the circular result, "causal" only
    got = mf.fftconv_pair(x, v, n=48, mode="causal")
    assert _worst(got.cpu().numpy().reshape(6, L), ref_pair(xh, vh, 48, 0, 0, 0, L, False).reshape(6, L)) <= TOL[t]


# ---- 4. rows do not see each other ---------------------------------------------------------------------------------------------------

def test_row_separation_and_autocorrelation():
    t, n = "f32", 192
    tile = PAIR_CLASSES[(t, n)][1]
    L, K, o, Lo = single_shape(n)
    R = full_and_ragged(tile)
    plan = _plan(t, R, L, K, n, 0, 0, o, Lo, False)
    x, _ = _normal(1, (R, L, 1), DT[t])
    v, _ = _normal(2, (R, K, 1), DT[t])
    base = _run(plan, x, v)
    for which, row in (("x", 5), ("v", tile + 7)):
        xs, vs = x.clone(), v.clone()
        (xs if which == "x" else vs)[row] = float("nan")
        got = _run(plan, xs, vs, written=False)
        assert bool(torch.isnan(got[row]).all()), which
        others = [r for r in range(R) if r != row]
        assert torch.equal(_bits(got[others]), _bits(base[others])), which
    # x is v: the autocorrelation of every row, from the same storage
    La = n // 2 - 1  # (odd; the 2 La - 1 lags fit the FFT length)
    auto = _plan(t, R, La, La, n, La - 1, 0, 0, 2 * La - 1, True)
    xa, xh = _normal(3, (R, La, 1), DT[t])
    got = _run(auto, xa, xa).cpu().numpy()
    ref = ref_pair(xh[..., 0], xh[..., 0], n, La - 1, 0, 0, 2 * La - 1, True)
    assert _worst(got, ref) <= TOL[t]
    assert np.abs(got[:, La - 1] - (xh[..., 0] ** 2).sum(-1)).max() <= 1e-4 * La  # (lag 0 is the energy)


# ---- 5. slabs and rounds ---------------------------------------------------------------------------------------------------------------

def test_slabs_are_bit_identical():
    t, n = "f64", 66
    tile = PAIR_CLASSES[(t, n)][1]
    L, K, o, Lo = single_shape(n)
    R = full_and_ragged(tile)
    plan = _plan(t, R, L, K, n, K - 1, 0, o, Lo, True)
    x, _ = _normal(4, (R, L, 1), DT[t])
    v, _ = _normal(5, (R, K, 1), DT[t])
    whole = _run(plan, x, v)
    a, b = tile // 2 + 1, tile + 3  # (slabs that start inside a tile of the whole-batch run)
    slabs = [(0, a), (a, b), (a + b, R - a - b)]
    assert all(c > 0 for _, c in slabs) and len({c for _, c in slabs}) == 3
    assert torch.equal(_bits(_run(plan, x, v, slabs=slabs)), _bits(whole))
    # a slab alone leaves the other rows NaN
    part = _run(plan, x, v, slabs=slabs[1:2], written=False)
    assert torch.equal(_bits(part[a:a + b]), _bits(whole[a:a + b]))
    assert bool(torch.isnan(part[:a]).all()) and bool(torch.isnan(part[a + b:]).all())


def test_every_workgroup_walks_three_tiles():
    t, n = "f32", 14
    L, K, o, Lo = single_shape(n)
    P = 37  # (distinct rows; no multiple of the tile, so a row meets every position of a tile)
    small = _plan(t, P, L, K, n, 0, 0, o, Lo, False)
    tile, threads, _, grid = small.pass_geometry(1, FAR)
    assert P % tile
    x, _ = _normal(6, (P, L, 1), DT[t])
    v, _ = _normal(7, (P, K, 1), DT[t])
    base = _run(small, x, v)
    R = 3 * grid * tile - tile // 2  # (the last tile ragged)
    big = _plan(t, R, L, K, n, 0, 0, o, Lo, False)
    assert big.pass_geometry(1) == (tile, threads, 3 * grid, grid)
    reps = -(-R // P)
    xb, vb = x.repeat(reps, 1, 1)[:R].contiguous(), v.repeat(reps, 1, 1)[:R].contiguous()
    got = _run(big, xb, vb)
    assert torch.equal(_bits(got), _bits(base.repeat(reps, 1)[:R]))


# ---- 6. the backward's plans are the forward's adjoints, on the device ---------------------------------------------------------------

@pytest.mark.parametrize("n,L,K", [(64, 37, 28), (64, 40, 40), (2058, 1029, 1030)])
def test_adjointness(n, L, K):
    rng = np.random.default_rng(n + L)
    R = 5
    for corr in (False, True):
        ea, eb = int(rng.integers(0, n - L + 1)), int(rng.integers(0, n - K + 1))
        o = int(rng.integers(0, n - 2)) | 1
        Lo = int(rng.integers(2, n - o + 1))
        x, _ = _normal(n + 1, (R, L, 1), torch.float64)
        v, _ = _normal(n + 2, (R, K, 1), torch.float64)
        gy, _ = _normal(n + 3, (R, Lo, 1), torch.float64)
        y = _run(_plan("f64", R, L, K, n, ea, eb, o, Lo, corr), x, v)
        lhs = float((gy[..., 0] * y).sum())
        scale = float(gy.norm() * y.norm())
        for spec, other, wrt in zip(adjoints_of(L, K, ea, eb, o, Lo, corr), (v, x), (x, v)):
            first, La, Lb, a_ea, a_eb, a_o, a_Lo, a_corr = spec
            a, b = (gy, other) if first == "gy" else (other, gy)
            g = _run(_plan("f64", R, La, Lb, n, a_ea, a_eb, a_o, a_Lo, a_corr), a, b)
            rhs = float((g * wrt[..., 0]).sum())
            assert abs(lhs - rhs) <= REL_L2_TOL_F64 * scale, (n, corr, spec, lhs, rhs)


# ---- 7. autograd --------------------------------------------------------------------------------------------------------------------------

def _torch_pair(x, v, n, ea, eb, o, Lo, corr):
    """the definition over torch.fft, differentiable by torch itself"""
    L, K = x.shape[-1], v.shape[-1]
    xe = torch.nn.functional.pad(x, (ea, n - ea - L))
    ve = torch.nn.functional.pad(v, (eb, n - eb - K))
    G = torch.fft.rfft(ve)
    return torch.fft.irfft(torch.fft.rfft(xe) * (G.conj() if corr else G), n)[..., o:o + Lo]


def _host_grads(xh, vh, wh, n, ea, eb, o, Lo, corr):
    x, v = (torch.from_numpy(a).clone().requires_grad_(True) for a in (xh, vh))
    (_torch_pair(x, v, n, ea, eb, o, Lo, corr) * torch.from_numpy(wh)).sum().backward()
    return x.grad.numpy(), v.grad.numpy()


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("L,K", [(37, 28), (28, 37), (16, 16)])
def test_autograd_against_torch(L, K, t):
    shape = (2, 3)
    n = mf.fftconv_length(L + K - 1, DT[t])
    x0, xh = _normal(L * 3, shape + (L,), DT[t])
    v0, vh = _normal(K * 5 + 1, shape + (K,), DT[t])
    for corr in (False, True):
        for mode in MODES:
            ea, eb, o, Lo = window_of(mode, L, K, corr)
            w, wh = _normal(Lo + 9, shape + (Lo,), DT[t])
            x, v = x0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
            y = mf.fftconv_pair(x, v, mode=mode, correlate=corr)
            assert y.grad_fn is not None
            with torch.no_grad():
                plain = mf.fftconv_pair(x, v, mode=mode, correlate=corr)
            assert plain.grad_fn is None and torch.equal(_bits(plain), _bits(y.detach()))  # (the same launch, bit for bit)
            (y * w).sum().backward()
            gx, gv = _host_grads(xh, vh, wh, n, ea, eb, o, Lo, corr)
            ex = _worst(x.grad.cpu().numpy().reshape(6, L), gx.reshape(6, L))
            ev = _worst(v.grad.cpu().numpy().reshape(6, K), gv.reshape(6, K))
            assert x.grad.dtype == DT[t] and ex <= TOL[t] and ev <= TOL[t], (mode, corr, ex, ev)


def test_autograd_circular_and_one_sided():
    L, K, n = 40, 40, 64
    x0, xh = _normal(1, (4, L), torch.float64)
    v0, vh = _normal(2, (4, K), torch.float64)
    w, wh = _normal(3, (4, L), torch.float64)
    for corr in (False, True):
        gx, gv = _host_grads(xh, vh, wh, n, 0, 0, 0, L, corr)
        x, v = x0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
        (mf.fftconv_pair(x, v, n=n, mode="causal", correlate=corr) * w).sum().backward()
        assert _worst(x.grad.cpu().numpy(), gx) <= REL_L2_TOL_F64 and _worst(v.grad.cpu().numpy(), gv) <= REL_L2_TOL_F64
        # only one of the two wants a gradient: the other comes back None, and the one that is computed has the same bits
        for only in ("x", "v"):
            a, b = x0.clone().requires_grad_(only == "x"), v0.clone().requires_grad_(only == "v")
            y = mf.fftconv_pair(a, b, n=n, mode="causal", correlate=corr)
            (y * w).sum().backward()
            assert (a.grad is None) == (only == "v") and (b.grad is None) == (only == "x")
            have, full = (a.grad, x.grad) if only == "x" else (b.grad, v.grad)
            assert torch.equal(_bits(have), _bits(full))
    # the incoming gradient of sum() is an expanded tensor: made contiguous
    x = x0.clone().requires_grad_(True)
    mf.fftconv_pair(x, v0, mode="valid", correlate=True).sum().backward()  # (L == K: one sample per row, the dot product)
    assert _worst(x.grad.cpu().numpy(), vh) <= REL_L2_TOL_F64
    # nothing requires grad: no grad_fn
    assert mf.fftconv_pair(x0, v0).grad_fn is None


def test_gradcheck():
    g = torch.Generator(device=DEV).manual_seed(21)
    mk = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float64).requires_grad_(True)
    x, v = mk(2, 8), mk(2, 5)
    for mode, corr in (("full", False), ("same", True), ("valid", False), ("causal", True)):
        fn = lambda x, v: mf.fftconv_pair(x, v, n=16, mode=mode, correlate=corr)
        assert torch.autograd.gradcheck(fn, (x, v), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
