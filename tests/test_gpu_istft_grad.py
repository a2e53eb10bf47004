"""Gradients of istft with respect to its frames: the fused adjoint (plan_istft_adjoint, the STFT tile with TileCfg::IADJ)
against torch.autograd over torch.istft in fp64 on the same rounded inputs (tests/istft_grad_reference.py)."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf

from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
import istft_grad_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = R.SMALL_SHAPES + [R.WALK, R.MID]
DTYPES = [torch.float32, torch.float64]
CASES = [(s, dt) for s in SHAPES for dt in DTYPES] + [(R.BIG, torch.float32)]
NP = {torch.float32: np.float32, torch.float64: np.float64}
CT = {torch.float32: torch.complex64, torch.float64: torch.complex128}
FAR = 1 << 40


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v).replace("torch.", "")


def _tol(dt):
    return REL_L2_TOL_F32 if dt == torch.float32 else REL_L2_TOL_F64


def _bits(t):
    t = torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _gain(shape):
    return float(shape[2]) ** 0.5 if shape[8] else 1.0


def _plan(shape, dt, batch=None):
    B, F, n, hop, centred, wname, wl, length, normalized = shape
    return mf.plan_istft_adjoint(dt, B if batch is None else batch, F, n, hop, window=R.table_of(wname, wl, n), center=centred,
                                 gain=_gain(shape), length=R.length_of(shape))


def _run(plan, gy, **kw):
    """the plan on a (batch, T) device tensor -> complex (batch, F, bins), from a NaN-prefilled output"""
    out = torch.full(plan.out_shape, float("nan"), dtype=plan.out_dtype, device=DEV)
    mf.fft(out, gy.reshape(plan.in_shape), plan=plan, **kw)
    torch.cuda.synchronize()
    return torch.view_as_complex(out)


def _istft_kw(shape):
    _, _, n, hop, centred, wname, wl, length, normalized = shape
    w = None if wname is None else torch.from_numpy(R.window_of(wname, wl))
    return dict(n_fft=n, hop_length=hop, win_length=wl, window=w, center=centred, normalized=normalized, length=length)


def _zero_frames(ref):
    """the frames (b, f) of a bins-major (B, bins, F) reference that are exact zeros"""
    return (ref == 0).all(axis=1)


def _check(got, ref, dt, what):
    """bins-major (B, bins, F): relative L2 per frame against the reference, exact zeros where it has them, and the imaginary
    parts of bins 0 and n / 2 exact zeros as integers"""
    gt = got.detach()
    g = gt.cpu().to(torch.complex128).numpy()
    assert g.shape == ref.shape and np.isfinite(g).all(), what
    zero = _zero_frames(ref)
    num = np.linalg.norm(g - ref, axis=1)
    den = np.linalg.norm(ref, axis=1)
    assert (num[zero] == 0).all(), (what, "a frame that sees no stored sample is not an exact zero")
    err = float((num[~zero] / den[~zero]).max())
    print(f"{what}: worst rel-L2 per frame {err:.3e}, {int(zero.sum())} zero frames")
    assert err <= _tol(dt), (what, err)
    im = _bits(gt.imag)
    N = ref.shape[1] - 1
    assert int(im[:, 0].abs().max()) == 0 and int(im[:, N].abs().max()) == 0, (what, "Im of bins 0 / n/2 is not +0")


@pytest.mark.parametrize("shape,dt", CASES, ids=_id)
def test_plan_and_backward_match_torch_autograd(shape, dt):
    X, gy, ref = R.reference(shape, NP[dt])
    B, F, n = shape[:3]
    gyd = torch.from_numpy(gy).to(dt).to(DEV)
    plan = _plan(shape, dt)
    assert plan.kernel_name(1).endswith("_stft_iadj_jit"), plan.kernel_name(1)
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    got = _run(plan, gyd).transpose(-1, -2)
    _check(got, ref, dt, f"plan {_id(shape)} {_id(dt)}")
    # ... and mf.istft(X).backward(gy): the same bits, in X's shape and dtype
    Xd = torch.from_numpy(X).to(CT[dt]).to(DEV).requires_grad_(True)
    y = mf.istft(Xd, **_istft_kw(shape))
    assert y.grad_fn is not None and y.shape == (B, R.length_of(shape))
    (g,) = torch.autograd.grad(y, Xd, gyd, retain_graph=True)
    assert g.stride(-2) == 1  # what the backward returns: the transposed view of the frames-major tensor, no transposing copy
    y.backward(gyd)
    assert Xd.grad.shape == Xd.shape and Xd.grad.dtype == Xd.dtype
    assert torch.equal(_bits(Xd.grad), _bits(got)) and torch.equal(_bits(g), _bits(got))


@pytest.mark.parametrize("shape", R.SMALL_SHAPES, ids=_id)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_nan_outside_the_range_and_one_entry_alone(shape, dt):
    """gy of one entry between guards of NaN, run alone: finite, and bit for bit the entry of the batched run -- the samples
    before 0 and at and beyond T are never read"""
    X, gy, ref = R.reference(shape, NP[dt])
    B, n, T = shape[0], shape[2], R.length_of(shape)
    whole = _run(_plan(shape, dt), torch.from_numpy(gy).to(dt).to(DEV))
    one = _plan(shape, dt, batch=1)
    for b in range(B):
        buf = torch.full((T + 2 * n,), float("nan"), dtype=dt, device=DEV)
        buf[n:n + T] = torch.from_numpy(gy[b]).to(dt)
        got = _run(one, buf[n:n + T])
        assert bool(torch.isfinite(torch.view_as_real(got)).all())
        assert torch.equal(_bits(got[0]), _bits(whole[b])), (shape, b)
    # the whole batch between guard rows of NaN
    rows = torch.full((B + 2, T), float("nan"), dtype=dt, device=DEV)
    rows[1:B + 1] = torch.from_numpy(gy).to(dt)
    assert torch.equal(_bits(_run(_plan(shape, dt), rows[1:B + 1])), _bits(whole))


@pytest.mark.parametrize("shape", [R.SMALL_SHAPES[0], R.SMALL_SHAPES[2], R.SMALL_SHAPES[5], R.SMALL_SHAPES[6]], ids=_id)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_impulses_bin_by_bin(shape, dt):
    _, F, n, hop, centred = shape[:5]
    T, c = R.length_of(shape), (n // 2 if centred else 0)
    spots = sorted({0, T - 1, hop, max(0, hop - c)} | ({n // 2} if centred else set()))  # ends, a hop boundary, the first sample after the trimmed ones
    plan = _plan(shape, dt, batch=len(spots))
    gy = torch.zeros((len(spots), T), dtype=dt, device=DEV)
    for i, t0 in enumerate(spots):
        gy[i, t0] = 1.0
    got = _run(plan, gy).cpu().to(torch.complex128).numpy()
    tol = 1e-5 if dt == torch.float32 else 1e-13
    for i, t0 in enumerate(spots):
        want = R.impulse_closed_form(shape, t0)
        scale = np.abs(want).max()
        assert scale > 0, (shape, t0)
        assert np.abs(got[i] - want).max() <= tol * scale, (shape, t0, np.abs(got[i] - want).max() / scale)
        covered = np.array([0 <= t0 + c - f * hop < n for f in range(F)])
        assert (got[i][~covered] == 0).all(), (shape, t0, "a frame that does not cover the impulse is not an exact zero")


@pytest.mark.parametrize("shape", R.SMALL_SHAPES + [R.MID], ids=_id)
def test_dot_product_identity_on_the_device(shape):
    X, gy, _ = R.reference(shape, np.float64, seed=2)
    Xd = torch.from_numpy(X).to(DEV)
    gyd = torch.from_numpy(gy).to(DEV)
    y = mf.istft(Xd, **_istft_kw(shape))
    gX = _run(_plan(shape, torch.float64), gyd).transpose(-1, -2)
    lhs = float((y * gyd).sum())
    rhs = float((Xd.real * gX.real + Xd.imag * gX.imag).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)


def test_gradcheck_complex128():
    torch.manual_seed(3)
    X = torch.randn(2, 9, 5, dtype=torch.complex128, device=DEV, requires_grad=True)
    w = torch.hann_window(16, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda Z: mf.istft(Z, 16, 4, window=w), (X,), nondet_tol=0)
    h = torch.hamming_window(16, dtype=torch.float64)  # (uncentred: a window that does not vanish at sample 0)
    assert torch.autograd.gradcheck(lambda Z: mf.istft(Z, 16, 4, window=h, center=False, normalized=True, length=27), (X,),
                                    nondet_tol=0)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bit_identity_across_batch_and_slabs(dt):
    shape = R.WALK
    B, F = shape[:2]
    X, gy, _ = R.reference(shape, NP[dt])
    gyd = torch.from_numpy(gy).to(dt).to(DEV)
    plan = _plan(shape, dt)
    whole = _run(plan, gyd)
    again = _run(plan, gyd)
    assert torch.equal(_bits(whole), _bits(again))
    alone = _run(_plan(shape, dt, batch=1), gyd[3:4])
    assert torch.equal(_bits(alone[0]), _bits(whole[3]))
    for first, count in ((0, 2), (2, 1), (3, 2)):
        part = _run(plan, gyd, first=first, count=count)
        assert torch.equal(_bits(part[first:first + count]), _bits(whole[first:first + count])), (first, count)
        rest = torch.view_as_real(torch.cat([part[:first], part[first + count:]]))
        assert bool(torch.isnan(rest).all()), "a slab wrote outside its entries"


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_three_rounds_of_the_persistent_grid(dt):
    """the batch sized from Plan.pass_geometry, as tests/test_gpu_persistent_rounds.py sizes its cases: two full rounds and a
    partial one with a ragged last tile; every frame against the fp64 model, entries from every round against the plan of
    one entry bit for bit"""
    shape = R.SMALL_SHAPES[1]  # 11 frames per entry, odd hop: tiles that wrap into the following entries
    _, F, n, hop = shape[:4]
    tile, threads, _, G = _plan(shape, dt, batch=4).pass_geometry(1, FAR)
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    B = -(-((n_tiles - 1) * tile + max(1, tile // 3)) // F)
    while (B * F) % tile == 0 or -(-(B * F) // tile) % G == 0:
        B += 1
    plan = _plan(shape, dt, batch=B)
    geo = plan.pass_geometry(1)
    assert geo[:2] == (tile, threads) and geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0 and (B * F) % tile != 0, geo
    T = R.length_of(shape)
    gy = np.random.default_rng(11).standard_normal((B, T)).astype(NP[dt])
    gyd = torch.from_numpy(gy).to(DEV)
    got = _run(plan, gyd)
    ref = R.adjoint_model(gy.astype(np.float64), shape)
    g = got.cpu().to(torch.complex128).numpy()
    err = float((np.linalg.norm(g - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max())
    print(f"rounds {_id(dt)}: tile {geo[0]} n_tiles {geo[2]} grid {geo[3]} entries {B}: worst rel-L2 per frame {err:.3e}")
    assert err <= _tol(dt), err
    one = _plan(shape, dt, batch=1)
    per_round = geo[3] * tile // F
    for b in (0, per_round // 2, per_round + 1, 2 * per_round + 3, B - 1):
        assert torch.equal(_bits(_run(one, gyd[b:b + 1])[0]), _bits(got[b])), b


@pytest.mark.parametrize("shape", [R.SMALL_SHAPES[0], R.SMALL_SHAPES[7]], ids=_id)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_the_plain_call_is_what_it_was(shape, dt):
    """without requires_grad and under no_grad: the bits of the inverse plan run directly, and no grad_fn; through
    _ISTFTFunction: the same bits"""
    B, F, n, hop, centred, wname, wl, length, normalized = shape
    X, _, _ = R.reference(shape, NP[dt])
    Xd = torch.from_numpy(X).to(CT[dt]).to(DEV)
    plan = mf.plan_istft(dt, B, F, n, hop, window=R.table_of(wname, wl, n), center=centred, normalized=normalized,
                         length=R.length_of(shape))
    out = torch.full(plan.out_shape, float("nan"), dtype=dt, device=DEV)
    mf.fft(out, torch.view_as_real(Xd.transpose(-1, -2).contiguous()), plan=plan)
    direct = out.reshape(B, -1)
    kw = _istft_kw(shape)
    y0 = mf.istft(Xd, **kw)
    assert y0.grad_fn is None and not y0.requires_grad and torch.equal(_bits(y0), _bits(direct))
    Xg = Xd.clone().requires_grad_(True)
    with torch.no_grad():
        y1 = mf.istft(Xg, **kw)
    assert y1.grad_fn is None and torch.equal(_bits(y1), _bits(direct))
    y2 = mf.istft(Xg, **kw)
    assert y2.grad_fn is not None and torch.equal(_bits(y2.detach()), _bits(direct))


def test_layouts_and_dtypes_of_the_gradient():
    shape = R.SMALL_SHAPES[0]
    X, gy, ref = R.reference(shape, np.float32)
    kw = _istft_kw(shape)
    gyd = torch.from_numpy(gy).float().to(DEV)
    grads = []
    # bins-major contiguous, and stft's transposed view of frames-major memory: the same gradient
    Xc = torch.from_numpy(X).to(torch.complex64).to(DEV)
    for Xin in (Xc.contiguous(), Xc.transpose(-1, -2).contiguous().transpose(-1, -2)):
        Xin = Xin.detach().requires_grad_(True)
        mf.istft(Xin, **kw).backward(gyd)
        assert Xin.grad.shape == Xin.shape and Xin.grad.dtype == torch.complex64
        grads.append(Xin.grad)
    assert torch.equal(_bits(grads[0]), _bits(grads[1]))
    # a leading batch of two dims, and a complex64 X with out_dtype float64: gX in X's shape and dtype, fp64 accuracy inside
    X4 = Xc.reshape(1, 3, *Xc.shape[1:]).detach().requires_grad_(True)
    y = mf.istft(X4, out_dtype=torch.float64, **kw)
    assert y.dtype == torch.float64 and y.shape == (1, 3, R.length_of(shape))
    y.backward(gyd.double().reshape(1, 3, -1))
    assert X4.grad.shape == X4.shape and X4.grad.dtype == torch.complex64
    g = X4.grad.reshape(Xc.shape).cpu().to(torch.complex128).numpy()
    err = float((np.linalg.norm(g - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())
    assert err <= 2e-7, err  # (one rounding of the fp64 result to complex64)
    # the window is kept by value: changing it in place between forward and backward changes nothing
    w = kw["window"].clone()
    Xa = Xc.detach().clone().requires_grad_(True)
    ya = mf.istft(Xa, **dict(kw, window=w))
    w.mul_(3.0)
    mf.clear_plan_cache()
    ya.backward(gyd)
    assert torch.equal(_bits(Xa.grad), _bits(grads[0]))


def test_refusal_is_raised_in_the_forward():
    X = torch.randn(2, 9, 5, dtype=torch.complex64, device=DEV)
    w = torch.tensor([0.0] * 8 + [1.0] * 8)
    with pytest.raises(mf.MifftError):  # (the forward refuses this window as well: the overlap-add condition)
        mf.istft(X.clone().requires_grad_(True), 16, 16, window=w, center=False)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_a_round_trip_that_trains(dt):
    torch.manual_seed(5)
    B, T, n, hop = 3, 200, 16, 4
    w = torch.hann_window(n, dtype=torch.float64)
    x = torch.randn(B, T, dtype=torch.float64).to(dt)
    gy = torch.randn(B, T, dtype=torch.float64).to(dt)
    xr = x.double().clone().requires_grad_(True)
    yr = torch.istft(torch.stft(xr, n, hop, window=w, return_complex=True), n, hop, window=w, length=T)
    yr.backward(gy.double())
    xd = x.to(DEV).requires_grad_(True)
    y = mf.istft(mf.stft(xd, n, hop, window=w), n, hop, window=w, length=T)
    y.backward(gy.to(DEV))
    got, ref = xd.grad.cpu().double().numpy(), xr.grad.numpy()
    err = float((np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())
    print(f"round trip {_id(dt)}: rel-L2 per entry {err:.3e}")
    assert xd.grad.dtype == dt and err <= _tol(dt), err
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) <= (1e-5 if dt == torch.float32 else 1e-12)
