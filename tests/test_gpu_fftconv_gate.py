"""Gated fftconv on the device (plan_fftconv(pregate=, postgate=), ConvPlan.run, fftconv(pregate=, postgate=, skip=);
TileCfg::GATE): bit for bit against the ungated kernel on the products torch makes, for every gate combination, in every path
of the load and the store of both tiles; the fp64 model of test_fftconv_gate_host.py with skip terms; gate impulses index by
index around a block seam; slabs; three rounds of the persistent grid; the plan's reported facts; the refusals of the exec.
Every gate is a view into the middle of a larger buffer of NaNs: an element read outside the tensor and used shows in the
result.  x and the gates are compared bitwise before and after; outputs lie between canaries."""
import ctypes

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_fftconv_gate_host import gated_model
from test_fftconv_long_host import geometry

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 64  # canary elements on both sides of an output
CANARY = -7.25
PAD_A, PAD_B = 67, 129  # NaNs on both sides of a gate; odd, so that a gate is aligned to one element only


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _worst(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max())


class Gate:
    """standard-normal values of ``shape`` in the middle of a buffer that is NaN elsewhere; ``t`` is the view"""

    def __init__(self, gen, shape, dtype, pad, values=None):
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * pad,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.flat[pad:pad + numel].view(shape)
        self.t.copy_(torch.randn(shape, generator=gen, dtype=dtype, device=DEV) if values is None else values)
        self.keep = _bits(self.flat).clone()

    def unwritten(self):
        return torch.equal(_bits(self.flat), self.keep)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _canaried(shape, dtype):
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), CANARY, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def _canaries_intact(flat):
    return bool((flat[:GUARD] == CANARY).all()) and bool((flat[-GUARD:] == CANARY).all())


def _run(plan, x, a=None, b=None, first=None, count=None):
    """a gated exec into a canaried buffer"""
    flat, out = _canaried(plan.out_shape, plan.out_dtype)
    plan.run(out, x, pregate=a, postgate=b, first=first, count=count)
    torch.cuda.synchronize()
    assert _canaries_intact(flat), "a canary was written"
    return out


def _plain(plan, x):
    flat, out = _canaried(plan.out_shape, plan.out_dtype)
    mf.fft(out, x, plan=plan)
    torch.cuda.synchronize()
    assert _canaries_intact(flat), "a canary was written"
    return out


def _plans(dtype, B, D, L, n, gates, k, **kw):
    """the gated plan and the ungated one of the same shape, with the same filter"""
    g = mf.plan_fftconv(dtype, B, D, L, n, pregate=bool(gates & 1), postgate=bool(gates & 2), **kw)
    u = mf.plan_fftconv(dtype, B, D, L, n, **kw)
    for p in (g, u):
        p.set_filter(k)
    assert torch.equal(_bits(g.filter_spectrum), _bits(u.filter_spectrum))
    return g, u


def _bit_exact(dtype, B, D, L, n, K, gates, seed, **kw):
    gen = _gen(seed)
    k = torch.randn((D, K), generator=gen, dtype=dtype, device=DEV)
    gp, up = _plans(dtype, B, D, L, n, gates, k, **kw)
    x = torch.randn(gp.in_shape, generator=gen, dtype=dtype, device=DEV)
    a, b = Gate(gen, gp.in_shape, dtype, PAD_A), Gate(gen, gp.out_shape, dtype, PAD_B)
    keep = _bits(x).clone()
    got = _run(gp, x, a.t if gates & 1 else None, b.t if gates & 2 else None)
    want = _plain(up, x * a.t if gates & 1 else x)
    if gates & 2:
        want = want * b.t
    assert not bool(torch.isnan(got).any()), "a gate element outside its tensor was read and used"
    assert torch.equal(_bits(got), _bits(want)), f"gates {gates}: {int((_bits(got) != _bits(want)).sum())} samples differ"
    # gates of ones: the ungated result
    ones_a = Gate(gen, gp.in_shape, dtype, PAD_A, values=torch.ones(gp.in_shape, dtype=dtype, device=DEV))
    ones_b = Gate(gen, gp.out_shape, dtype, PAD_B, values=torch.ones(gp.out_shape, dtype=dtype, device=DEV))
    got1 = _run(gp, x, ones_a.t if gates & 1 else None, ones_b.t if gates & 2 else None)
    assert torch.equal(_bits(got1), _bits(_plain(up, x))), f"gates {gates}: ones as gates change the result"
    assert torch.equal(_bits(x), keep), "x was written"
    assert a.unwritten() and b.unwritten() and ones_a.unwritten() and ones_b.unwritten(), "a gate was written"
    return gp, up


# (n, L, K, o, Lo, D, B, dtype): odd L -- the single-element tail of the load; odd o -- the unaligned store and real-by-real
# postgate loads; L = Lo = n; a length whose passes are no powers of two; fp64; one large row of either type
SINGLE = [(16, 11, 5, 0, 11, 3, 2, "f32"), (64, 37, 20, 13, 37, 3, 2, "f32"), (96, 96, 9, 0, 96, 3, 2, "f32"),
          (1000, 777, 100, 0, 777, 3, 2, "f32"), (64, 37, 20, 13, 37, 3, 2, "f64"), (16384, 9001, 1000, 0, 9001, 2, 1, "f32"),
          (12288, 6001, 500, 0, 6001, 2, 1, "f64")]
# (n, T, K, D, B, dtype): S = 8 even; S = 12; s0 = -32 < 0 -- zeros in front of the row load no gate; S = 31 odd -- unaligned
# pair loads of x and gate alike; tiles straddle signal rows (D = 3, B = 2); fp64
OLS = [(16, 101, 9, 3, 2, "f32"), (16, 100, 5, 3, 2, "f32"), (64, 200, 33, 3, 2, "f32"), (64, 1000, 34, 3, 2, "f32"),
       (64, 200, 33, 3, 2, "f64")]


@pytest.mark.parametrize("gates", [1, 2, 3])
@pytest.mark.parametrize("n,L,K,o,Lo,D,B,t", SINGLE, ids=lambda v: str(v))
def test_single_block_equals_the_ungated_kernel_bit_for_bit(n, L, K, o, Lo, D, B, t, gates):
    gp, up = _bit_exact(DT[t], B, D, L, n, K, gates, 1000 * n + L + gates, offset=o, out_length=Lo)
    # the plan's facts
    name, plain = gp.kernel_name(1), up.kernel_name(1)
    assert name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "") + "r2c_") and name.endswith(f"_conv_g{gates}_jit"), name
    assert plain.endswith("_conv_jit") and plain == name.replace(f"_g{gates}", ""), (plain, name)
    assert gp.kernel_name(0) == "none" and gp.num_launches == 1 and gp.scratch_bytes == 0
    assert (gp.pregate, gp.postgate) == (bool(gates & 1), bool(gates & 2)) and (up.pregate, up.postgate) == (False, False)
    assert gp.in_bytes == up.in_bytes == B * D * L * gp.filter_spectrum.element_size()
    assert gp.out_bytes == up.out_bytes == B * D * Lo * gp.filter_spectrum.element_size()


@pytest.mark.parametrize("gates", [1, 2, 3])
@pytest.mark.parametrize("n,T,K,D,B,t", OLS, ids=lambda v: str(v))
def test_overlap_save_equals_the_ungated_kernel_bit_for_bit(n, T, K, D, B, t, gates):
    gp, up = _bit_exact(DT[t], B, D, T, n, K, gates, 1000 * n + T + gates, taps=K)
    assert (gp.step, gp.blocks) == (n - K + 1, -(-T // (n - K + 1))) == (up.step, up.blocks)
    name, plain = gp.kernel_name(1), up.kernel_name(1)
    assert name.endswith(f"_conv_ols_g{gates}_jit") and plain.endswith("_conv_ols_jit"), (name, plain)
    assert plain == name.replace(f"_g{gates}", "") and gp.num_launches == 1 and gp.scratch_bytes == 0


@pytest.mark.parametrize("gates", [1, 2, 3])
@pytest.mark.parametrize("kw", [dict(mode="causal"), dict(mode="full"), dict(mode="same"), dict(mode="valid"),
                                dict(correlate=True)], ids=lambda v: str(v))
def test_modes_through_fftconv_bit_for_bit(kw, gates):
    T, K, n, D, B = 333, 15, 16, 3, 2
    gen = _gen(7 + gates)
    x = torch.randn((B, D, T), generator=gen, device=DEV)
    k = torch.randn((D, K), generator=gen, device=DEV)
    plain = mf.fftconv(x, k, block=n, **kw)
    a, b = Gate(gen, x.shape, torch.float32, PAD_A), Gate(gen, plain.shape, torch.float32, PAD_B)
    got = mf.fftconv(x, k, block=n, pregate=a.t if gates & 1 else None, postgate=b.t if gates & 2 else None, **kw)
    want = mf.fftconv(x * a.t, k, block=n, **kw) if gates & 1 else plain
    if gates & 2:
        want = want * b.t
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (kw, gates)
    assert a.unwritten() and b.unwritten()


def _against_the_model(dtype, B, D, L, n, K, seed, o=0, Lo=None, taps=None):
    """both gates, skip as a float and as a (D,) tensor, convolution and correlation"""
    gen = _gen(seed)
    Lo = L if Lo is None else Lo
    k = torch.randn((D, K), generator=gen, dtype=dtype, device=DEV)
    x = torch.randn((B * D, L, 1), generator=gen, dtype=dtype, device=DEV)
    a, b = Gate(gen, (B * D, L, 1), dtype, PAD_A), Gate(gen, (B * D, Lo, 1), dtype, PAD_B)
    dvec = torch.randn((D,), generator=gen, dtype=dtype, device=DEV)
    worst = 0.0
    for correlate in (False, True):
        if taps is not None and correlate and o + Lo > L:
            continue
        plan = mf.plan_fftconv(dtype, B, D, L, n, offset=o, out_length=Lo, taps=taps, correlate=correlate, pregate=True,
                               postgate=True)
        ols = None if taps is None else geometry(n, K, o, Lo, correlate)
        for skip in (0.625, dvec):
            plan.set_filter(k)
            plan.add_skip(skip)
            got = _run(plan, x, a.t, b.t).cpu().numpy()[..., 0]
            ref = gated_model(x.cpu().numpy()[..., 0], k.cpu().numpy(), n, a=a.t.cpu().numpy(), b=b.t.cpu().numpy(),
                              skip=skip if isinstance(skip, float) else skip.cpu().numpy(), o=o, Lo=Lo, ols=ols,
                              correlate=correlate)
            err = _worst(got, ref)
            print(f"gated fftconv n={n} L={L} K={K} o={o} Lo={Lo} taps={taps} {dtype} correlate={correlate} "
                  f"skip={'float' if isinstance(skip, float) else 'tensor'} worst rel-L2 {err:.3e}")
            worst = max(worst, err)
    assert a.unwritten() and b.unwritten()
    return worst


@pytest.mark.parametrize("n,L,K,o,Lo,D,B,t", SINGLE, ids=lambda v: str(v))
def test_single_block_against_the_model(n, L, K, o, Lo, D, B, t):
    assert _against_the_model(DT[t], B, D, L, n, K, 31 * n + L, o=o, Lo=Lo) <= TOL[DT[t]]


@pytest.mark.parametrize("n,T,K,D,B,t", OLS, ids=lambda v: str(v))
def test_overlap_save_against_the_model(n, T, K, D, B, t):
    assert _against_the_model(DT[t], B, D, T, n, K, 37 * n + T, taps=K) <= TOL[DT[t]]


def test_skip_through_fftconv_against_the_model():
    T, K, n, D, B = 333, 15, 16, 3, 2
    gen = _gen(91)
    x = torch.randn((B, D, T), generator=gen, dtype=torch.float64, device=DEV)
    k = torch.randn((D, K), generator=gen, dtype=torch.float64, device=DEV)
    d = torch.randn((D,), generator=gen, dtype=torch.float64, device=DEV)
    for kw, block in ((dict(mode="causal"), n), (dict(correlate=True), n), (dict(mode="same"), None)):
        o, Lo = mf.api._fftconv_window(kw.get("mode", "causal"), T, K)
        a, b = Gate(gen, (B, D, T), torch.float64, PAD_A), Gate(gen, (B, D, Lo), torch.float64, PAD_B)
        for skip in (d, -1.5, None):
            got = mf.fftconv(x, k, block=block, pregate=a.t, postgate=b.t, skip=skip, **kw).cpu().numpy()
            nn = n if block else mf.fftconv_length(T + K - 1, torch.float64)
            ols = geometry(nn, K, o, Lo, bool(kw.get("correlate"))) if block else None
            ref = gated_model(x.cpu().numpy().reshape(B * D, T), k.cpu().numpy(), nn, a=a.t.cpu().numpy(), b=b.t.cpu().numpy(),
                              skip=None if skip is None else skip if isinstance(skip, float) else skip.cpu().numpy(), o=o,
                              Lo=Lo, ols=ols, correlate=bool(kw.get("correlate")))
            assert _worst(got.reshape(B * D, Lo), ref) <= REL_L2_TOL_F64, (kw, block, skip)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_gate_impulses_index_by_index(t):
    """x all ones, k a unit impulse at tap j0, the pregate a unit impulse at sample t0, the postgate all ones: the output is 1
    at t0 + j0 and 0 to tolerance elsewhere; t0 at both ends and around a block seam.  Then the postgate a unit impulse at
    sample u0 and x random: zero everywhere but at u0, where it is the ungated result bit for bit."""
    dtype = DT[t]
    n, T, K = 64, 200, 33
    S = n - K + 1
    gen = _gen(5)
    x1 = torch.ones((1, 1, T), dtype=dtype, device=DEV)
    for t0 in (0, S - 1, S, S + 1, T - 1):
        for j0 in (0, K - 1):
            k = torch.zeros((1, K), dtype=dtype, device=DEV)
            k[0, j0] = 1
            av = torch.zeros((1, 1, T), dtype=dtype, device=DEV)
            av[..., t0] = 1
            a = Gate(gen, (1, 1, T), dtype, PAD_A, values=av)
            b = Gate(gen, (1, 1, T + K - 1), dtype, PAD_B, values=torch.ones((1, 1, T + K - 1), dtype=dtype, device=DEV))
            y = mf.fftconv(x1, k, block=n, mode="full", pregate=a.t, postgate=b.t).cpu().numpy()[0, 0]
            want = np.zeros(T + K - 1)
            want[t0 + j0] = 1
            assert int(np.abs(y).argmax()) == t0 + j0, (t0, j0, int(np.abs(y).argmax()))
            assert np.linalg.norm(y - want) <= TOL[dtype], (t0, j0, np.linalg.norm(y - want))
    x = torch.randn((1, 1, T), generator=gen, dtype=dtype, device=DEV)
    k = torch.randn((1, K), generator=gen, dtype=dtype, device=DEV)
    plain = mf.fftconv(x, k, block=n, mode="full")
    Lo = T + K - 1
    for u0 in (0, S - 1, S, S + 1, Lo - 1):
        bv = torch.zeros((1, 1, Lo), dtype=dtype, device=DEV)
        bv[..., u0] = 1
        b = Gate(gen, (1, 1, Lo), dtype, PAD_B, values=bv)
        y = mf.fftconv(x, k, block=n, mode="full", postgate=b.t)
        assert torch.equal(_bits(y[..., u0]), _bits(plain[..., u0])), u0
        y[..., u0] = 0
        assert bool((y == 0).all()), u0


@pytest.mark.parametrize("kw", [dict(L=37, n=64, K=28), dict(L=333, n=64, K=28, taps=28)], ids=["single", "ols"])
def test_slabs_equal_the_whole_exec_bit_for_bit(kw):
    """run(first=, count=) over two uneven slabs: the library offsets x, out and both gates; the filter row follows first % D"""
    dtype, D, B = torch.float32, 3, 7
    L, n, K, taps = kw["L"], kw["n"], kw["K"], kw.get("taps")
    gen = _gen(41)
    k = torch.randn((D, K), generator=gen, device=DEV)
    plan = mf.plan_fftconv(dtype, B, D, L, n, taps=taps, pregate=True, postgate=True)
    plan.set_filter(k)
    x = torch.randn(plan.in_shape, generator=gen, device=DEV)
    a, b = Gate(gen, plan.in_shape, dtype, PAD_A), Gate(gen, plan.out_shape, dtype, PAD_B)
    whole = _run(plan, x, a.t, b.t)
    for first, count in ((0, 5), (5, 16), (20, 1)):
        part = _run(plan, x, a.t, b.t, first=first, count=count)
        assert torch.equal(_bits(part[first:first + count]), _bits(whole[first:first + count])), (first, count)
        assert bool((part[:first] == CANARY).all()) and bool((part[first + count:] == CANARY).all()), (first, count)
    # the same signals in a batch of another size: the same bits (rows 3 .. 8 start at a multiple of D)
    small = mf.plan_fftconv(dtype, 2, D, L, n, taps=taps, pregate=True, postgate=True)
    small.set_filter(k)
    part = _run(small, x[3:9].contiguous(), a.t[3:9].contiguous(), b.t[3:9].contiguous())
    assert torch.equal(_bits(part), _bits(whole[3:9]))
    assert a.unwritten() and b.unwritten()


def _three_rounds(dtype, D, L, n, K, taps):
    """the batch of tests/test_gpu_fftconv.py / test_gpu_fftconv_long.py: two full rounds of the persistent grid and a partial
    one with a ragged last tile, sized from Plan.pass_geometry"""
    probe = mf.plan_fftconv(dtype, 2, D, L, n, taps=taps, pregate=True, postgate=True)
    tile, threads, _, G = probe.pass_geometry(1, 1 << 40)
    F = probe.blocks
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    rows = -(-((n_tiles - 1) * tile + max(1, tile // 3)) // F)  # signal rows
    rows += (-rows) % D
    while (tile > 1 and (rows * F) % tile == 0) or -(-rows * F // tile) % G == 0:
        rows += D
    return rows // D, rows, (tile, threads)


@pytest.mark.parametrize("kw", [dict(L=37, n=64, K=28), dict(L=7 * 32 - 5, n=64, K=33, taps=33)], ids=["single", "ols"])
def test_three_rounds_of_the_persistent_grid(kw):
    dtype, D = torch.float32, 3
    L, n, K, taps = kw["L"], kw["n"], kw["K"], kw.get("taps")
    B, rows, tt = _three_rounds(dtype, D, L, n, K, taps)
    gen = _gen(51)
    k = torch.randn((D, K), generator=gen, device=DEV)
    gp, up = _plans(dtype, B, D, L, n, 3, k, taps=taps)
    geo = gp.pass_geometry(1)
    assert geo == up.pass_geometry(1), (geo, up.pass_geometry(1))
    assert geo[:2] == tt and geo[2] == -(-rows * gp.blocks // geo[0]) and geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0, geo
    if taps is not None and geo[0] > 1:
        assert geo[0] % gp.blocks != 0 and gp.blocks % geo[0] != 0, (geo, gp.blocks)  # (tiles straddle signal rows)
    x = torch.randn(gp.in_shape, generator=gen, device=DEV)
    a, b = Gate(gen, gp.in_shape, dtype, PAD_A), Gate(gen, gp.out_shape, dtype, PAD_B)
    got = _run(gp, x, a.t, b.t)
    want = _plain(up, x * a.t) * b.t
    bad = (_bits(got) != _bits(want)).reshape(rows, -1).any(dim=1).nonzero().flatten().tolist()
    print(f"gated fftconv rounds: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows} x {gp.blocks} blocks")
    assert not bad, f"signal rows {bad[:8]} differ from the ungated kernel"
    assert a.unwritten() and b.unwritten()


def test_the_exec_refuses_without_launching():
    dtype, B, D, L, n = torch.float32, 2, 3, 11, 16
    lib = _lib.lib()
    stream = torch.cuda.current_stream(0).cuda_stream
    plan = mf.plan_fftconv(dtype, B, D, L, n, pregate=True)
    plan.set_filter(torch.ones((D, 3), device=DEV))
    x = torch.randn(plan.in_shape, device=DEV)
    a = torch.randn(plan.in_shape, device=DEV)
    flat, out = _canaried(plan.out_shape, dtype)

    def block(magic=mf.GATED_ARGS_MAGIC, x=x.data_ptr(), pre=a.data_ptr(), post=None):
        return mf.GatedArgs(magic, x, pre, post)

    for args, status, word in ((block(pre=None), -12, "pregate is NULL"),                      # a missing gate
                               (block(post=a.data_ptr()), -15, "no postgate"),                # a gate the plan did not ask for
                               (block(pre=out.data_ptr()), -13, "pregate and out"),           # a gate that overlaps out
                               (block(pre=out.data_ptr() + 4 * (L * B * D - 1)), -13, "pregate and out"),
                               (block(x=None), -12, "x is NULL"),
                               (block(magic=0), -15, "mifft_gated_args")):
        rc = lib.mifft_exec_batch(plan._h, ctypes.addressof(args), out.data_ptr(), 0, B * D, stream)
        assert rc == status and word in lib.mifft_last_error().decode(), (rc, lib.mifft_last_error().decode())
    # the signal itself in the place of the block, as an ungated plan takes it
    rc = lib.mifft_exec(plan._h, x.data_ptr(), out.data_ptr(), stream)
    assert rc == -15 and "mifft_gated_args" in lib.mifft_last_error().decode(), (rc, lib.mifft_last_error().decode())
    rc = lib.mifft_exec_batch(plan._h, x.data_ptr(), out.data_ptr(), 0, B * D, stream)
    assert rc == -15 and "mifft_gated_args" in lib.mifft_last_error().decode()
    ms = ctypes.c_float()
    rc = lib.mifft_time_exec(plan._h, x.data_ptr(), out.data_ptr(), stream, 2, ctypes.byref(ms))
    assert rc == -15 and "mifft_gated_args" in lib.mifft_last_error().decode()
    with pytest.raises(mf.MifftError) as e:
        mf.fft(out, x, plan=plan)
    assert e.value.status == -15 and "run(" in str(e.value)
    # the Python layer says the same before it calls the library
    for kw, status in ((dict(), -12), (dict(pregate=a, postgate=a), -15), (dict(pregate=a[:-1]), -14),
                       (dict(pregate=a.double()), -14)):
        with pytest.raises(mf.MifftError) as e:
            plan.run(out, x, **kw)
        assert e.value.status == status, (kw, e.value)
    with pytest.raises(mf.MifftError) as e:  # run() belongs to gated plans
        mf.plan_fftconv(dtype, B, D, L, n).run(out, x)
    assert e.value.status == -15 and "fft(" in str(e.value)
    torch.cuda.synchronize()
    assert bool((flat == CANARY).all()), "a refused exec launched"
    # a gate may alias x; the block through mifft_exec and mifft_time_exec runs
    plan.run(out, x, pregate=x)
    want = out.clone()
    args = block(pre=x.data_ptr())
    flat2, out2 = _canaried(plan.out_shape, dtype)
    assert lib.mifft_exec(plan._h, ctypes.addressof(args), out2.data_ptr(), stream) == 0
    assert lib.mifft_time_exec(plan._h, ctypes.addressof(args), out2.data_ptr(), stream, 2, ctypes.byref(ms)) == 0 and ms.value > 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out2), _bits(want)) and _canaries_intact(flat2)
    ungated = mf.plan_fftconv(dtype, B, D, L, n)
    ungated.set_filter(torch.ones((D, 3), device=DEV))
    assert torch.equal(_bits(want), _bits(_plain(ungated, x * x)))
