"""Half-precision storage of fftconv on the device (``io_dtype`` = bfloat16 / float16: 16-bit rows in memory, float32 inside).
Widening a 16-bit float is exact and the arithmetic between the load and the store is the float32 kernel's, so almost every
check here is an identity on the bits: ``fftconv(x, k, ..., io_dtype=t) == fftconv(x.float(), k, ...).to(t)`` compared as
int16, on all three tiles (single block, overlap-save, partitioned), every gate combination, odd and 2-byte-aligned rows,
the ends of rows and block seams, the float16 range, slabs, three rounds of the persistent grid and untouched memory; the
filter gradient against the float32 kernel on the widened tensors, bit for bit; autograd bit for bit where the route has one
rounding, and within bounds counted from the roundings where it has more.  torch's ``.to`` is the model of the rounding
(test_fftconv_half_host.py holds it to the bit arithmetic)."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32
from test_fftconv_grad_host import reference_grads, worst_row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HALF = {"b16": torch.bfloat16, "h16": torch.float16}
TYPES = ["b16", "h16"]
# one rounding to storage is at most half an ulp: 2^-9 of a bfloat16 sample, 2^-12 of a float16 one
EPS = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}


def _i16(t):
    return t.contiguous().view(torch.int16)


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _rand(gen, shape, t, scale=1.0):
    """randn rounded to the storage type"""
    return (torch.randn(shape, generator=gen, device=DEV) * scale).to(t)


def _gates(gen, gates, xs, ys, t):
    a = _rand(gen, xs, t) if gates & 1 else None
    b = _rand(gen, ys, t) if gates & 2 else None
    return a, b


def _f(v):
    return None if v is None else v.float()


def _identity(x, k, t, a=None, b=None, skip=None, **kw):
    """the main identity; returns the half-storage result"""
    ref = mf.fftconv(x.float(), k, pregate=_f(a), postgate=_f(b), skip=skip, **kw)
    keep = [_i16(v).clone() for v in (x, a, b) if v is not None]
    got = mf.fftconv(x, k, pregate=a, postgate=b, skip=skip, io_dtype=t, **kw)
    torch.cuda.synchronize()
    assert ref.dtype == torch.float32 and got.dtype == t and got.shape == ref.shape
    bad = (_i16(got) != _i16(ref.to(t))).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} samples differ from ref.to({t}), the first at {bad[0].tolist()}"
    for v, w in zip([v for v in (x, a, b) if v is not None], keep):
        assert torch.equal(_i16(v), w)  # (no input is written)
    return got


def _out_len(mode, L, K):
    return mf.api._fftconv_window(mode, L, K)[1]


# ---- single block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("gates", [0, 1, 2, 3])
@pytest.mark.parametrize("variant", ["plain", "skip", "correlate"])
def test_single_block_identity(ts, gates, variant):
    t, (B, D, L, K) = HALF[ts], (2, 3, 37, 9)
    gen = _gen(100 + gates)
    x, k = _rand(gen, (B, D, L), t), torch.randn((D, K), generator=gen, device=DEV)
    a, b = _gates(gen, gates, (B, D, L), (B, D, L), t)
    skip = torch.randn(D, generator=gen, device=DEV) if variant == "skip" else None
    _identity(x, k, t, a, b, skip, n=64, correlate=variant == "correlate")


@pytest.mark.parametrize("n,L,K,B,D", [(8, 5, 3, 2, 3), (96, 50, 40, 2, 2), (2048, 1024, 1024, 2, 2), (16384, 8192, 8192, 2, 2)],
                         ids=lambda v: str(v))
def test_lengths_identity_bfloat16(n, L, K, B, D):
    gen = _gen(n)
    x, k = _rand(gen, (B, D, L), torch.bfloat16), torch.randn((D, K), generator=gen, device=DEV)
    _identity(x, k, torch.bfloat16, n=n)


def test_the_kernel_is_the_half_storage_twin():
    for ts, t in HALF.items():
        for kw, mid in ((dict(), "_conv"), (dict(taps=33), "_conv_ols"), (dict(taps=1000, partition=33), "_conv_pols")):
            L = 37 if not kw else 1000
            for gates in (0, 3):
                p = mf.plan_fftconv(torch.float32, 2, 3, L, 64, io_dtype=t, pregate=bool(gates & 1), postgate=bool(gates & 2), **kw)
                q = mf.plan_fftconv(torch.float32, 2, 3, L, 64, pregate=bool(gates & 1), postgate=bool(gates & 2), **kw)
                g = f"_g{gates}" if gates else ""
                assert p.kernel_name(1).endswith(f"{mid}{g}_{ts}_jit") and q.kernel_name(1).endswith(f"{mid}{g}_jit"), p.kernel_name(1)
                assert p.io_dtype == t and q.io_dtype is None and p.in_dtype == p.out_dtype == torch.float32
                assert p.filter_spectrum.dtype == torch.float32 and p.num_launches == 1 and p.scratch_bytes == 0
                # 2 bytes per element where the float32 plan counts 4
                assert (2 * p.in_bytes, 2 * p.out_bytes) == (q.in_bytes, q.out_bytes) == (6 * L * 4, 6 * L * 4)
        p, q = mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64, io_dtype=t), mf.plan_fftconv_grad(torch.float32, 2, 3, 37, 64)
        assert p.kernel_name(1).endswith(f"_wgrad_{ts}_jit") and q.kernel_name(1).endswith("_wgrad_jit")
        assert 2 * p.in_bytes == q.in_bytes and p.out_bytes == q.out_bytes and p.io_dtype == t  # (the result stays float32)
        p = mf.plan_fftconv_grad(torch.float32, 2, 3, 1000, 64, taps=33, io_dtype=t)
        assert p.kernel_name(1).endswith(f"_wgrad_ols_{ts}_jit")


# ---- alignment: odd L and odd Lo put every other row off a 4-byte boundary ---------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("L,K,mode", [(37, 9, "full"), (37, 9, "same"), (37, 4, "same"), (37, 10, "valid"), (37, 9, "valid"),
                                      (2, 9, "full"), (2, 2, "causal")], ids=lambda v: str(v))
def test_alignment_identity(ts, L, K, mode):
    t, (B, D) = HALF[ts], (3, 3)
    gen = _gen(L * 100 + K)
    Lo = _out_len(mode, L, K)
    x, k = _rand(gen, (B, D, L), t), torch.randn((D, K), generator=gen, device=DEV)
    a, b = _gates(gen, 3, (B, D, L), (B, D, Lo), t)
    _identity(x, k, t, n=64, mode=mode)
    _identity(x, k, t, a, b, n=64, mode=mode)


# ---- the ends of rows and the seams of blocks: an impulse through a one-tap filter comes back exactly -----------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("path", ["single", "ols", "part"])
def test_impulses_at_the_ends_and_across_a_seam(ts, path):
    t = HALF[ts]
    if path == "single":
        L, K, kw = 37, 1, dict(n=64)
        at = [0, 1, L - 2, L - 1]
    elif path == "ols":
        L, K, kw = 1000, 33, dict(block=64)  # S = 32
        at = [0, 1, 31, 32, 33, 63, 64, L - 2, L - 1]
    else:
        L, K, kw = 1000, 1000, dict(block=64, partition=33)  # S = 32
        at = [0, 1, 31, 32, 33, 63, 64, L - 2, L - 1]
    B, D = 2, 3
    k = torch.zeros((D, K), device=DEV)
    k[:, 0] = 1
    for s in at:
        x = torch.zeros((B, D, L), dtype=t, device=DEV)
        x[..., s] = torch.tensor([1.5, -0.75, 3.0], dtype=t, device=DEV).reshape(1, D)
        x[1, :, s] *= 2
        got = _identity(x, k, t, **kw)  # (the float32 kernel's bits on the same impulse, rounded)
        # The impulse comes back exactly where it stood.  Elsewhere an impulse off sample 0 leaves what the two float32
        # transforms leave of it (bins that are rounded twiddles do not cancel to the last bit: non-zero from s = 1 on, on
        # all three paths, in the float32 kernel too), far below the 16-bit ulp of the impulse but not zero: bounded by the
        # float32 budget of the kernel, REL_L2_TOL_F32 of the impulse.  At s = 0 every bin is the impulse itself and the
        # result is x, bit for bit.
        assert torch.equal(_i16(got[..., s]), _i16(x[..., s])), (path, s)
        rest = got.float().clone()
        rest[..., s] = 0
        assert rest.abs().max() <= REL_L2_TOL_F32 * 6.0, (path, s, float(rest.abs().max()))
        if s == 0:
            assert torch.equal(_i16(got + 0), _i16(x + 0)), path  # (+ 0: a -0.0 is 0)
    gen = _gen(7)
    x = _rand(gen, (B, D, L), t)
    x[..., [0, 1, L - 2, L - 1]] = torch.tensor([1.0, 2.0, -3.0, 4.0], dtype=t, device=DEV)
    got = _identity(x, k, t, **kw)  # (a full row with known ends: every sample within one rounding of itself)
    assert (got.float() - x.float()).abs().max() <= EPS[t] * x.float().abs().max() * 2


# ---- overlap-save and partitioned -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("gates", [0, 3])
@pytest.mark.parametrize("path,K,kw", [("ols", 33, dict(block=64)), ("ols", 30, dict(block=64)),
                                       ("part", 1000, dict(block=64, partition=33))], ids=["ols33", "ols30", "part"])
@pytest.mark.parametrize("variant", ["causal", "full", "correlate"])
def test_long_rows_identity(ts, gates, path, K, kw, variant):
    t, (B, D, T) = HALF[ts], (2, 3, 1000)
    gen = _gen(K + gates)
    mode = "full" if variant == "full" else "causal"
    Lo = _out_len(mode, T, K)
    x, k = _rand(gen, (B, D, T), t), torch.randn((D, K), generator=gen, device=DEV)
    a, b = _gates(gen, gates, (B, D, T), (B, D, Lo), t)
    skip = 0.5 if gates else None
    _identity(x, k, t, a, b, skip, mode=mode, correlate=variant == "correlate", **kw)


def test_partitioned_identity_at_the_largest_block():
    t, (B, D, T) = torch.bfloat16, (1, 2, 32768)
    gen = _gen(16384)
    x, k = _rand(gen, (B, D, T), t), torch.randn((D, T), generator=gen, device=DEV) / 64
    a, b = _gates(gen, 3, (B, D, T), (B, D, T), t)
    _identity(x, k, t, a, b, block=16384, partition=8193)


# ---- the float16 range ------------------------------------------------------------------------------------------------------
def test_float16_subnormals_are_kept():
    t, (B, D, L, K) = torch.float16, (2, 3, 37, 9)
    gen = _gen(14)
    x, k = _rand(gen, (B, D, L), t, 2.0 ** -14), torch.randn((D, K), generator=gen, device=DEV) / 4
    assert ((x != 0) & (x.float().abs() < 2.0 ** -14)).sum() > x.numel() // 4  # (subnormal inputs are read as they are)
    for kw in (dict(n=64), dict(block=64, mode="full")):
        got = _identity(x, k, t, **kw).float()
        sub = (got != 0) & (got.abs() < 2.0 ** -14)
        assert sub.sum() > got.numel() // 4, int(sub.sum())
    b = _rand(gen, (B, D, L), t, 2.0 ** -3)
    _identity(x * 8, k, t, None, b, n=64)  # (and a postgate that takes normal results down into the subnormals)


def test_float16_overflow_gives_infinity_where_torch_does():
    t, (B, D, L, K) = torch.float16, (2, 3, 37, 9)
    gen = _gen(65504)
    x, k = _rand(gen, (B, D, L), t, 100.0), torch.randn((D, K), generator=gen, device=DEV)
    x[1, 2] = (x[1, 2].float() * 300).clamp(-60000, 60000).to(t)
    got = _identity(x, k, t, n=64)
    assert torch.isinf(got[1, 2]).any() and torch.isfinite(got[0]).all()
    assert not torch.isnan(got).any()


# ---- slabs, the persistent grid, untouched memory ---------------------------------------------------------------------------
PATHS = [("single", dict(L=37, n=64), dict(offset=0, out_length=45)), ("ols", dict(L=333, n=64, taps=33), dict(out_length=365)),
         ("part", dict(L=333, n=64, taps=333, partition=33), dict(out_length=333))]


@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("path,kw,win", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("gates", [0, 3])
def test_slabs_and_untouched_memory(ts, path, kw, win, gates):
    """odd L and odd Lo: a slab that starts at an odd row starts 2 bytes off a 4-byte boundary.  out lies between guard
    rows; the union of the slabs is the whole-batch run, and a slab exec leaves every other row and the guards as they were"""
    t, (B, D) = HALF[ts], (3, 3)
    rows, L, Lo = B * D, kw["L"], win["out_length"]
    gen = _gen(rows + L + gates)
    plan = mf.plan_fftconv(torch.float32, B, D, L, kw["n"], taps=kw.get("taps"), partition=kw.get("partition"),
                           pregate=bool(gates & 1), postgate=bool(gates & 2), io_dtype=t, **win)
    assert plan.in_shape == (rows, L, 1) and plan.out_shape == (rows, Lo, 1) and L % 2 == 1 and Lo % 2 == 1
    plan.set_filter(torch.randn((D, min(kw.get("taps") or 9, 40)), generator=gen, device=DEV))
    x = _rand(gen, plan.in_shape, t)
    a, b = _gates(gen, gates, plan.in_shape, plan.out_shape, t)

    def run(out, **slab):
        if gates:
            plan.run(out, x, pregate=a, postgate=b, **slab)
        else:
            mf.fft(out, x, plan=plan, **slab)
        torch.cuda.synchronize()

    pattern = torch.arange((rows + 2) * Lo, device=DEV, dtype=torch.int32).mul(7919).remainder(30011).to(torch.int16)
    whole = pattern.clone().view(t).reshape(rows + 2, Lo, 1)
    run(whole[1:-1])
    assert torch.equal(_i16(whole[0]), pattern[:Lo].reshape(Lo, 1)) and torch.equal(_i16(whole[-1]), pattern[-Lo:].reshape(Lo, 1))
    union = pattern.clone().view(t).reshape(rows + 2, Lo, 1)
    for first, count in ((0, 1), (1, 3), (4, 0), (4, 1), (5, 4)):
        before = _i16(union).clone()
        run(union[1:-1], first=first, count=count)
        after = _i16(union)
        assert torch.equal(after[:1 + first], before[:1 + first]) and torch.equal(after[1 + first + count:], before[1 + first + count:])
        assert torch.equal(after[1 + first:1 + first + count], _i16(whole)[1 + first:1 + first + count]), (first, count)
    assert torch.equal(_i16(union), _i16(whole))


@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("kw", [dict(L=37, K=9), dict(L=7 * 32 - 5, K=33, taps=33)], ids=["single", "ols"])
def test_three_rounds_of_the_persistent_grid(ts, kw):
    t, D, n = HALF[ts], 3, 64
    L, K, taps = kw["L"], kw["K"], kw.get("taps")
    probe = mf.plan_fftconv(torch.float32, 2, D, L, n, taps=taps, io_dtype=t)
    tile, threads, _, G = probe.pass_geometry(1, 1 << 40)
    n_tiles = 2 * G + G // 2 + 3
    rows = -(-((n_tiles - 1) * tile + max(1, tile // 3)) // probe.blocks)
    rows += (-rows) % D
    gen = _gen(rows)
    k = torch.randn((D, K), generator=gen, device=DEV)
    hp = mf.plan_fftconv(torch.float32, rows // D, D, L, n, taps=taps, io_dtype=t)
    fp = mf.plan_fftconv(torch.float32, rows // D, D, L, n, taps=taps)
    geo = hp.pass_geometry(1)
    assert geo == fp.pass_geometry(1) and geo[2] >= 2 * geo[3] + 1, geo
    hp.set_filter(k)
    fp.set_filter(k)
    x = _rand(gen, hp.in_shape, t)
    got, want = torch.empty(hp.out_shape, dtype=t, device=DEV), torch.empty(fp.out_shape, device=DEV)
    mf.fft(got, x, plan=hp)
    mf.fft(want, x.float(), plan=fp)
    torch.cuda.synchronize()
    bad = (_i16(got) != _i16(want.to(t))).reshape(rows, -1).any(dim=1).nonzero().flatten().tolist()
    print(f"half fftconv rounds: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows}")
    assert not bad, f"signal rows {bad[:8]} differ"


# ---- what io_dtype=None does is what it did ---------------------------------------------------------------------------------
def test_float32_is_unchanged_and_float16_input_still_widens_to_float64():
    B, D, L, K, n = 2, 3, 37, 9, 64
    gen = _gen(32)
    x, k = torch.randn((B, D, L), generator=gen, device=DEV), torch.randn((D, K), generator=gen, device=DEV)
    got = mf.fftconv(x, k, n=n, io_dtype=None)
    plan = mf.plan_fftconv(torch.float32, B, D, L, n)
    assert not plan.kernel_name(1).endswith(("_b16_jit", "_h16_jit")) and plan.kernel_name(1).endswith("_conv_jit")
    plan.set_filter(k)
    want = torch.empty(plan.out_shape, device=DEV)
    mf.fft(want, x.reshape(plan.in_shape), plan=plan)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.equal(got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32))
    y = mf.fftconv(x.half(), k, n=n)
    assert y.dtype == torch.float64
    with pytest.raises(mf.MifftError):  # (a half-storage plan takes tensors of its io_dtype only)
        hp = mf.plan_fftconv(torch.float32, B, D, L, n, io_dtype=torch.bfloat16)
        mf.fft(torch.empty(hp.out_shape, device=DEV), x.reshape(hp.in_shape), plan=hp)
    # x of another dtype is converted: the same bits as from the converted tensor
    assert torch.equal(_i16(mf.fftconv(x, k, n=n, io_dtype=torch.bfloat16)), _i16(mf.fftconv(x.bfloat16(), k, n=n, io_dtype=torch.bfloat16)))


# ---- the filter gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("path,L,K,kw", [("single", 37, 28, dict(n=64)), ("correlate", 37, 28, dict(n=64, correlate=True)),
                                         ("ols", 1000, 33, dict(block=64)), ("part", 1000, 100, dict(block=64, partition=33))],
                         ids=["single", "correlate", "ols", "part"])
def test_filter_gradient_is_the_float32_kernel_s(ts, path, L, K, kw):
    t, (B, D) = HALF[ts], (4, 3)
    gen = _gen(L + K)
    x, gy = _rand(gen, (B, D, L), t), _rand(gen, (B, D, L), t)
    want = mf.fftconv_filter_grad(x.float(), gy.float(), K, **kw)
    got = mf.fftconv_filter_grad(x, gy, K, io_dtype=t, **kw)
    again = mf.fftconv_filter_grad(x, gy, K, io_dtype=t, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (D, K)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got.view(torch.int32), again.view(torch.int32))


# ---- autograd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("path,L,K,kw", [("single", 37, 9, dict(n=64)), ("ols", 1000, 33, dict(block=64))], ids=["single", "ols"])
def test_ungated_autograd_bit_for_bit(ts, path, L, K, kw):
    t, (B, D) = HALF[ts], (2, 3)
    gen = _gen(L)
    x, k = _rand(gen, (B, D, L), t).requires_grad_(True), torch.randn((D, K), generator=gen, device=DEV).requires_grad_(True)
    gy = _rand(gen, (B, D, L), t)
    y = mf.fftconv(x, k, io_dtype=t, **kw)
    assert y.dtype == t and y.grad_fn is not None
    y.backward(gy)
    assert x.grad.dtype == t and k.grad.dtype == torch.float32
    # gx: the float32 adjoint plan (the opposite correlate) on the widened gradient, rounded once
    rows = B * D
    adj = mf.plan_fftconv(torch.float32, B, D, L, 64, taps=None if path == "single" else K, correlate=True)
    adj.set_filter(k.detach())
    want = torch.empty(adj.out_shape, device=DEV)
    mf.fft(want, gy.float().reshape(rows, L, 1), plan=adj)
    torch.cuda.synchronize()
    assert torch.equal(_i16(x.grad), _i16(want.reshape(B, D, L).to(t)))
    gk = mf.fftconv_filter_grad(x.detach().float(), gy.float(), K, **kw)
    assert torch.equal(k.grad.view(torch.int32), gk.view(torch.int32))
    # only what is asked for is computed; a float32 gradient is converted to io_dtype on the way in
    x2, k2 = x.detach().clone(), k.detach().clone().requires_grad_(True)
    mf.fftconv(x2, k2, io_dtype=t, **kw).backward(gy.float().to(t))
    assert x2.grad is None and torch.equal(k2.grad.view(torch.int32), gk.view(torch.int32))
    x3 = x.detach().clone().requires_grad_(True)
    mf.fftconv(x3, k.detach(), io_dtype=t, **kw).backward(gy)
    assert torch.equal(_i16(x3.grad), _i16(x.grad))


@pytest.mark.parametrize("ts", TYPES)
@pytest.mark.parametrize("path,L,K,kw", [("single", 37, 9, dict(n=64)), ("ols", 300, 33, dict(block=64))], ids=["single", "ols"])
@pytest.mark.parametrize("mode", ["causal", "full"])
def test_gated_autograd_against_float64(ts, path, L, K, kw, mode):
    """All five gradients against torch CPU autograd of the float64 composition on the widened inputs, worst-row relative l2.
    The roundings to storage on the route built (each at most EPS = half an ulp per sample; the float32 error beside them
    is what REL_L2_TOL_F32 bounds):
      gk, skip: none -- u = a x and gv = b gy are float32 products of the widened tensors, the result is float32;
      gx = round(a * gu), gu = round(adjoint(b gy)) from the half-storage plan: two when the pregate's gradient is wanted too
           (one, fused into the store, when it is not) -- 2 EPS is the bound the contract gives gx, 2^-8 / 2^-11;
      ga = round(x * gu): two; gb = round(gy * v), v = round(conv(a x)): two -- within the three of the contract, whose
           bound is 2^-7 / 2^-10."""
    t, (B, D) = HALF[ts], (2, 3)
    o, Lo = mf.api._fftconv_window(mode, L, K)
    gen = _gen(L + K + len(mode))
    leaf = lambda shape, dt: _rand(gen, shape, dt).requires_grad_(True)
    x, a, b = leaf((B, D, L), t), leaf((B, D, L), t), leaf((B, D, Lo), t)
    k = torch.randn((D, K), generator=gen, device=DEV).requires_grad_(True)
    d = torch.randn(D, generator=gen, device=DEV).requires_grad_(True)
    gy = _rand(gen, (B, D, Lo), t)
    y = mf.fftconv(x, k, pregate=a, postgate=b, skip=d, mode=mode, io_dtype=t, **kw)
    y.backward(gy)
    assert (x.grad.dtype, a.grad.dtype, b.grad.dtype, k.grad.dtype, d.grad.dtype) == (t, t, t, torch.float32, torch.float32)
    wide = lambda v: v.detach().double().cpu().numpy()
    n_ref = 64 if path == "single" else 2048  # (a single FFT that holds the linear convolution of the long rows)
    yr, rx, rk, ra, rb, rd = reference_grads(wide(x), wide(k), wide(a), wide(b), wide(d), wide(gy), n_ref, o, Lo, False)
    one, gate = 2 * EPS[t], 4 * EPS[t]  # 2^-8 / 2^-11 and 2^-7 / 2^-10
    errs = {"y": worst_row(wide(y), yr), "gx": worst_row(wide(x.grad), rx), "gk": worst_row(wide(k.grad), rk),
            "ga": worst_row(wide(a.grad), ra), "gb": worst_row(wide(b.grad), rb),
            "gd": float(np.abs(wide(d.grad) - rd).max() / np.abs(rd).max())}
    print(f"half autograd {ts} {path} {mode}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert errs["y"] <= one and errs["gx"] <= one and errs["gk"] <= one and errs["gd"] <= one, errs
    assert errs["ga"] <= gate and errs["gb"] <= gate, errs
    # the filter gradient saw no rounding at all: the float32 plan on the float32 products, bit for bit
    gk = mf.fftconv_filter_grad(a.detach().float() * x.detach().float(), b.detach().float() * gy.float(), K, mode=mode, **kw)
    assert torch.equal(k.grad.view(torch.int32), gk.view(torch.int32))


# ---- accuracy as a user sees it ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", TYPES)
def test_accuracy_against_scipy(ts):
    """one rounding of the result to storage (at most EPS per sample) beside the float32 error of the kernel: within 2 EPS"""
    from scipy.signal import fftconvolve
    t, (B, D, L, K) = HALF[ts], (2, 3, 1024, 1024)
    gen = _gen(2048)
    x, k = _rand(gen, (B, D, L), t), torch.randn((D, K), generator=gen, device=DEV)
    y = mf.fftconv(x, k, n=2048, mode="full", io_dtype=t)
    ref = fftconvolve(x.double().cpu().numpy(), k.double().cpu().numpy()[None], axes=-1)
    err = worst_row(y.double().cpu().numpy(), ref)
    print(f"half fftconv {ts} n = 2048 against scipy: worst-row rel l2 {err:.3e}")
    assert err <= 2 * EPS[t] and REL_L2_TOL_F32 < EPS[t], err
