"""Gradients of stft / spectrogram / mfcc with respect to the signal: the fused adjoint overlap-add (plan_stft_adjoint, the
ISTFT tile with TileCfg::ADJ) against torch.autograd over torch.stft in fp64 on the same rounded inputs."""
import functools
import zlib

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf

from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from istft_reference import rel_l2_blocks
from stft_grad_reference import SMALL_SHAPES, adjoint_model, frames_of, torch_stft, window_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WALK = (5, 460, 16, 3, "reflect", "hamming")       # several tiles per entry, the last one ragged (the runs: test_runs_of_tiles_with_a_carry)
MID = (2, 9000, 1024, 256, "reflect", "hann")
BIG = (1, 40000, 16384, 4096, "reflect", "hann")   # fp32 only: the twiddle table in global memory, 512 threads
SHAPES = SMALL_SHAPES + [WALK, MID]
DTYPES = [torch.float32, torch.float64]
CASES = [(s, dt) for s in SHAPES for dt in DTYPES] + [(BIG, torch.float32)]


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v).replace("torch.", "")


def _tol(dt):
    return REL_L2_TOL_F32 if dt == torch.float32 else REL_L2_TOL_F64


def _bits(t):
    t = torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _kw(centre):
    return dict(center=centre is not None, pad_mode=centre or "reflect")


@functools.lru_cache(maxsize=None)
def _reference(shape, dt, win_length=None, normalized=False):
    """inputs rounded to ``dt`` and the fp64 reference of torch.autograd over torch.stft on them (CPU): never modified"""
    B, T, n, hop, centre, win = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, win_length, normalized)).encode()))
    wl = n if win_length is None else win_length
    w_short = window_of(win, wl)
    w = np.zeros(n)
    left = (n - wl) // 2
    w[left:left + wl] = 1.0 if w_short is None else w_short
    x = torch.randn(B, T, generator=g, dtype=torch.float64).to(dt)
    F, bins = frames_of(T, n, hop, centre), n // 2 + 1
    ct = torch.complex64 if dt == torch.float32 else torch.complex128
    gX = torch.complex(torch.randn(B, bins, F, generator=g, dtype=torch.float64),
                       torch.randn(B, bins, F, generator=g, dtype=torch.float64)).to(ct)
    gP = torch.randn(B, bins, F, generator=g, dtype=torch.float64).to(dt)
    xr = x.double().clone().requires_grad_()
    X = torch_stft(xr, n, hop, centre, w, normalized)
    (gx_stft,) = torch.autograd.grad(X, xr, gX.to(torch.complex128), retain_graph=True)
    (gx_pow,) = torch.autograd.grad(X.abs().pow(2), xr, gP.double(), retain_graph=True)
    return dict(x=x, gX=gX, gP=gP, X=X.detach(), gx_stft=gx_stft.numpy(), gx_pow=gx_pow.numpy(),
                window=None if w_short is None else torch.from_numpy(w_short))


def _frame_err(got, ref):
    """relative L2 error per frame (bins-major (B, bins, F) tensors), the maximum"""
    d = torch.linalg.vector_norm((got.cpu().to(ref.dtype) - ref), dim=-2)
    return float((d / torch.linalg.vector_norm(ref, dim=-2)).max())


def _check_grad(got, ref, shape, dt, what):
    B, T, n, hop, centre, win = shape
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = rel_l2_blocks(got, ref, hop)
    print(f"{what} {shape} {dt}: rel_l2_blocks = {err:.3e}")
    assert err < _tol(dt), (what, shape, dt, err)
    c = n // 2 if centre else 0
    L = n + hop * (frames_of(T, n, hop, centre) - 1)
    if L - c < T:  # the samples no frame covers: an exact zero
        assert (got[:, L - c:] == 0).all() and (ref[:, L - c:] == 0).all()


def _run_case(shape, dt, win_length=None, normalized=False):
    B, T, n, hop, centre, win = shape
    r = _reference(shape, dt, win_length, normalized)
    x = r["x"].to(DEV)
    kw = dict(win_length=win_length, window=r["window"], normalized=normalized, **_kw(centre))
    # -- stft
    X0 = mf.stft(x, n, hop, **kw)
    assert X0.grad_fn is None and not X0.requires_grad
    xg = x.clone().requires_grad_()
    X = mf.stft(xg, n, hop, **kw)
    assert X.grad_fn is not None
    assert torch.equal(_bits(X.detach()), _bits(X0))
    assert _frame_err(X0, r["X"]) < _tol(dt)
    X.backward(r["gX"].to(DEV))
    assert xg.grad.dtype == dt and xg.grad.shape == x.shape
    _check_grad(xg.grad, r["gx_stft"], shape, dt, "stft")
    # -- spectrogram, power 2
    P0 = mf.spectrogram(x, n, hop, power=2, **kw)
    assert P0.grad_fn is None
    xg = x.clone().requires_grad_()
    P = mf.spectrogram(xg, n, hop, power=2, **kw)
    assert P.grad_fn is not None and torch.equal(_bits(P.detach()), _bits(P0))
    assert _frame_err(P0, r["X"].abs().pow(2)) < 4 * _tol(dt)  # |X|^2: twice the relative error of X, per component
    P.backward(r["gP"].to(DEV))
    _check_grad(xg.grad, r["gx_pow"], shape, dt, "spectrogram power 2")


FAR = 1 << 40   # a count at which no grid is clamped by the tile count


@functools.lru_cache(maxsize=None)
def _walk(dt, multiplier=None):
    """WALK's signal at the smallest batch from B = 5 on whose schedule (mf.istft_schedule on the adjoint plan) holds every kind
    of run: every workgroup walks three tiles or more (at B = 5 each walks one, which never reads the carry), a run starts
    inside an entry behind warm-up tiles, a run crosses into the next entry, the last tile of an entry is ragged.
    Returns (B, tiles per entry, runs)."""
    _, T, n, hop, centre, win = WALK
    w = window_of(win, n)
    probe = mf.plan_stft_adjoint(dt, 1, T, n, hop, window=w, center=centre, multiplier=multiplier)
    tile, _, _, cap = probe.pass_geometry(2, FAR)
    tpe = -(-probe.frames // tile)
    assert probe.frames % tile != 0, "a ragged last tile"
    B = max(WALK[0], -(-3 * cap // tpe) + 1)
    for _ in range(64):
        plan = mf.plan_stft_adjoint(dt, B, T, n, hop, window=w, center=centre, multiplier=multiplier)
        runs = mf.istft_schedule(plan)
        mid = any(r[0] % tpe and r[2] > 0 for r in runs)
        cross = any(r[0] // tpe != (r[0] + r[1] - 1) // tpe for r in runs)
        if min(r[1] for r in runs) >= 3 and mid and cross:
            print(f"walk {dt}: B = {B}, tile = {tile}, tiles per entry = {tpe}, grid = {len(runs)}, {plan.kernel_name(2)}")
            return B, tpe, tuple(runs)
        B += 1
    raise AssertionError("no batch size reaches every path")


@pytest.mark.parametrize("shape,dt", CASES, ids=_id)
def test_stft_and_power_spectrogram_backward(shape, dt):
    if shape == WALK:  # (enlarged until its schedule holds every kind of run: modes 1 and 2 through autograd there)
        shape = (_walk(dt)[0],) + WALK[1:]
    _run_case(shape, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_short_window_and_normalized(dt):
    _run_case(SMALL_SHAPES[0], dt, win_length=10)
    _run_case(SMALL_SHAPES[0], dt, normalized=True)


def test_fail_without_the_feature():
    assert hasattr(mf, "plan_stft_adjoint")
    x = torch.randn(2, 50, device=DEV).requires_grad_()
    assert mf.stft(x, 16, 4).grad_fn is not None
    assert mf.spectrogram(x, 16, 4).grad_fn is not None
    with torch.no_grad():
        assert mf.stft(x, 16, 4).grad_fn is None
    assert mf.stft(x.detach(), 16, 4).grad_fn is None
    lead = torch.randn(2, 3, 50, device=DEV, dtype=torch.float64).requires_grad_()   # leading dims fold into the batch
    mf.stft(lead, 16, 4).abs().sum().backward()
    assert lead.grad.shape == lead.shape and lead.grad.dtype == torch.float64


# ---- power 1, fb, log, post, mfcc: the chain down to the bins -------------------------------------------------------------------
CHAIN_SHAPES = [(3, 50, 16, 4, "reflect", "hann", 3, 2), (2, 600, 64, 16, "reflect", "hann", 10, 4)]  # .., bands, coefficients
CHAINS = ["power1", "fb", "fb_log", "fb_db", "fb_log_post", "mfcc"]
AMIN = 1e-10


def _chain_torch(x, shape, kind, w, fb, post):
    B, T, n, hop, centre, win, M, Q = shape
    X = torch_stft(x, n, hop, centre, w)
    if kind == "power1":
        return X.abs(), None
    v = (fb.to(x.dtype).T @ X.abs().pow(2))
    bands = v
    if kind in ("fb_log", "fb_log_post"):
        v = torch.log(torch.clamp(v, min=AMIN))
    if kind in ("fb_db", "mfcc"):
        v = 10.0 * torch.log10(torch.clamp(v, min=AMIN)) - 10.0 * np.log10(max(AMIN, 1.0))
    if kind in ("fb_log_post", "mfcc"):
        v = post.to(x.dtype).T @ v
    return v, bands


def _chain_mf(x, shape, kind, wt, fb, post):
    B, T, n, hop, centre, win, M, Q = shape
    kw = dict(window=wt, **_kw(centre))
    if kind == "power1":
        return mf.spectrogram(x, n, hop, power=1, **kw)
    if kind == "fb":
        return mf.spectrogram(x, n, hop, power=2, fb=fb, **kw)
    if kind == "fb_log":
        return mf.spectrogram(x, n, hop, power=2, fb=fb, log="log", amin=AMIN, **kw)
    if kind == "fb_db":
        return mf.spectrogram(x, n, hop, power=2, fb=fb, log="db", amin=AMIN, **kw)
    if kind == "fb_log_post":
        return mf.spectrogram(x, n, hop, power=2, fb=fb, log="log", amin=AMIN, post=post, **kw)
    return mf.mfcc(x, 16000, Q, n_fft=n, hop_length=hop, n_mels=M, log="db", amin=AMIN, **kw)


@functools.lru_cache(maxsize=None)
def _chain_reference(shape, kind, dt):
    B, T, n, hop, centre, win, M, Q = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, kind)).encode()))
    w = window_of(win, n)
    fb = mf.melscale_fbanks(n // 2 + 1, 0.0, 8000.0, M, 16000)
    post = mf.create_dct(Q, M, "ortho")
    x = torch.randn(B, T, generator=g, dtype=torch.float64).to(dt)
    xr = x.double().clone().requires_grad_()
    y, bands = _chain_torch(xr, shape, kind, w, fb, post)
    if bands is not None and "fb" != kind:  # amin lies below every band value: the clamp's tie never decides
        assert float(bands.detach().min()) > AMIN
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64).to(dt)
    (ref,) = torch.autograd.grad(y, xr, gy.double())
    xs = x.clone().requires_grad_()   # torch's own autograd in the same precision, on the CPU
    ys, _ = _chain_torch(xs, shape, kind, w, fb, post)
    (own,) = torch.autograd.grad(ys, xs, gy)
    return dict(x=x, gy=gy, ref=ref.numpy(), own=own.double().numpy(), y=y.detach(), fb=fb, post=post,
                window=None if w is None else torch.from_numpy(w))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("kind", CHAINS)
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=_id)
def test_chain_backward(shape, kind, dt):
    """Held to the larger of the conftest tolerance and 4 times the error of torch's own autograd in the same precision
    against the same fp64 reference: these gradients divide by |X| or by the band value, and their conditioning belongs to the
    input, not to the kernel."""
    hop = shape[3]
    r = _chain_reference(shape, kind, dt)
    x = r["x"].to(DEV)
    y0 = _chain_mf(x, shape, kind, r["window"], r["fb"], r["post"])
    assert y0.grad_fn is None
    xg = x.clone().requires_grad_()
    y = _chain_mf(xg, shape, kind, r["window"], r["fb"], r["post"])
    assert y.grad_fn is not None and y.shape == r["y"].shape and torch.equal(_bits(y.detach()), _bits(y0))
    y.backward(r["gy"].to(DEV))
    got = xg.grad.cpu().double().numpy()
    err, err_torch = rel_l2_blocks(got, r["ref"], hop), rel_l2_blocks(r["own"], r["ref"], hop)
    print(f"chain {kind} {shape} {dt}: rel_l2_blocks = {err:.3e}, torch's own autograd = {err_torch:.3e}")
    assert err < max(_tol(dt), 4 * err_torch), (kind, shape, dt, err, err_torch)


def test_gradcheck():
    torch.manual_seed(5)
    w = torch.hann_window(16, dtype=torch.float64)
    fb = mf.melscale_fbanks(9, 0.0, 8000.0, 3, 16000)
    x = torch.randn(2, 40, dtype=torch.float64, device=DEV, requires_grad=True)
    kw = dict(eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda t: torch.view_as_real(mf.stft(t, 16, 4, window=w)), (x,), **kw)
    assert torch.autograd.gradcheck(lambda t: mf.spectrogram(t, 16, 4, window=w, power=2, fb=fb, log="log"), (x,), **kw)


# ---- the plan: bits, memory discipline, facts and refusals ----------------------------------------------------------------------
def _plan_inputs(shape, dt, seed=3):
    B, T, n, hop, centre, win = shape
    g = torch.Generator().manual_seed(seed)
    F, bins = frames_of(T, n, hop, centre), n // 2 + 1
    X = torch.randn(B, F, bins, 2, generator=g, dtype=torch.float64).to(dt).to(DEV)
    m = torch.randn(B, F, bins, generator=g, dtype=torch.float64).to(dt).to(DEV)
    return X, m


def _guarded(shape, dt):
    """a NaN-prefilled tensor with a NaN guard behind it: (whole, view)"""
    numel = int(np.prod(shape))
    whole = torch.full((numel + 64,), float("nan"), dtype=dt, device=DEV)
    return whole, whole[:numel].view(shape)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SMALL_SHAPES + [WALK, MID], ids=_id)
def test_mode2_equals_mode1_on_the_product_and_memory_discipline(shape, dt):
    B, T, n, hop, centre, win = shape
    w = window_of(win, n)
    X, m = _plan_inputs(shape, dt)
    X_copy, m_copy = X.clone(), m.clone()
    p1 = mf.plan_stft_adjoint(dt, B, T, n, hop, window=w, center=centre)
    p2 = mf.plan_stft_adjoint(dt, B, T, n, hop, window=w, center=centre, multiplier=2)
    assert p1.frames == p2.frames == frames_of(T, n, hop, centre) and p1.multiplier is None and p2.multiplier == 2
    assert p1.edge_shape == ((B, 2, n // 2) if centre == "reflect" else None)
    prod = (2 * m)[..., None] * X   # a power of two times the rounded product: mode 1's input is mode 2's, doubled exactly
    res = []
    for plan, xin, mult in ((p1, prod, None), (p2, X, m)):
        ow, out = _guarded(plan.out_shape, dt)
        ew, edge = _guarded(plan.edge_shape, dt) if plan.edge_shape else (None, None)
        plan.run(out, xin, multiplier=mult, edge=edge)
        torch.cuda.synchronize()
        assert torch.isnan(ow[out.numel():]).all() and (ew is None or torch.isnan(ew[edge.numel():]).all())
        res.append((out.clone(), None if edge is None else edge.clone()))
    assert torch.equal(X, X_copy) and torch.equal(m, m_copy)
    (o1, e1), (o2, e2) = res
    c = n // 2 if centre else 0
    L = n + hop * (p1.frames - 1)
    cov = min(T, L - c)
    assert p1.covered == cov
    assert not torch.isnan(o2[:, :cov]).any() and torch.isnan(o2[:, cov:]).all()   # written exactly where a frame covers
    assert torch.equal(_bits(o1[:, :cov]), _bits(o2[:, :cov]))
    if e2 is not None:
        e = max(0, min(c, L - c - T))
        assert not torch.isnan(e2[:, 0]).any() and not torch.isnan(e2[:, 1, :e]).any() and torch.isnan(e2[:, 1, e:]).all()
        assert torch.equal(_bits(e1[:, 0]), _bits(e2[:, 0])) and torch.equal(_bits(e1[:, 1, :e]), _bits(e2[:, 1, :e]))
    # the launch against the fp64 model of the kernel, strips included
    Xc = torch.view_as_complex(X.cpu().double()).numpy()
    gx, out_m, edge_m = adjoint_model(Xc, m.cpu().double().numpy(), 2, w, n, hop, T, centre)
    tol = 10 * _tol(dt)  # (per sample against the largest one: the strips are too short for a block metric)
    scale = np.abs(gx).max()
    assert np.abs(o2[:, :cov, 0].cpu().double().numpy() - out_m[:, :cov]).max() < tol * scale
    if e2 is not None:
        assert np.abs(e2[:, 0].cpu().double().numpy() - edge_m[:, 0]).max() < tol * scale
    got = p2.apply(X, m)
    assert got.shape == (B, T) and rel_l2_blocks(got.cpu().double().numpy(), gx, hop) < _tol(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_entry_bits_do_not_depend_on_batch_slab_or_run(dt):
    B, T, n, hop, centre, win = WALK
    w = window_of(win, n)
    X, m = _plan_inputs(WALK, dt)
    for mult in (None, 2, 1):
        plan = mf.plan_stft_adjoint(dt, B, T, n, hop, window=w, center=centre, multiplier=mult)
        one = mf.plan_stft_adjoint(dt, 1, T, n, hop, window=w, center=centre, multiplier=mult)
        mm = None if mult is None else m
        full = plan.apply(X, mm)
        assert torch.equal(_bits(full), _bits(plan.apply(X, mm)))            # two runs
        alone = one.apply(X[3:4].contiguous(), None if mm is None else mm[3:4].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(full[3]))                  # B = 1 against entry 3 of B = 5
        out = torch.full(plan.out_shape, float("nan"), dtype=dt, device=DEV)
        edge = torch.full(plan.edge_shape, float("nan"), dtype=dt, device=DEV)
        ref_out, ref_edge = out.clone(), edge.clone()   # (NaN where the launch writes nothing, in all four)
        plan.run(ref_out, X, multiplier=mm, edge=ref_edge)
        plan.run(out, X, multiplier=mm, edge=edge, first=0, count=2)         # slabs
        assert torch.isnan(out[2:]).all() and torch.isnan(edge[2:]).all()
        plan.run(out, X, multiplier=mm, edge=edge, first=2, count=3)
        assert torch.equal(_bits(out), _bits(ref_out)) and torch.equal(_bits(edge), _bits(ref_edge))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("multiplier", [None, 2, 1], ids=["mode1", "mode2", "mode3"])
def test_runs_of_tiles_with_a_carry(multiplier, dt):
    """The plan itself at WALK's enlarged batch (_walk), in every mode: every sample against the fp64 model of the kernel (which
    tests/test_stft_grad_host.py holds against torch.autograd), and entries from the middle of the walk -- behind warm-up tiles,
    which load the factor too -- against the B = 1 plan bit for bit."""
    _, T, n, hop, centre, win = WALK
    w = window_of(win, n)
    B, tpe, runs = _walk(dt, multiplier)
    plan = mf.plan_stft_adjoint(dt, B, T, n, hop, window=w, center=centre, multiplier=multiplier)
    one = mf.plan_stft_adjoint(dt, 1, T, n, hop, window=w, center=centre, multiplier=multiplier)
    X, m = _plan_inputs((B,) + WALK[1:], dt, seed=11)
    mm = None if multiplier is None else m
    got = plan.apply(X, mm)
    mode = {None: 1, 2: 2, 1: 3}[multiplier]
    ref, _, _ = adjoint_model(torch.view_as_complex(X.cpu().double()).numpy(), m.cpu().double().numpy(), mode, w, n, hop, T, centre)
    err = rel_l2_blocks(got.cpu().double().numpy(), ref, hop)
    print(f"walk mode {mode} {dt}: rel_l2_blocks = {err:.3e}")
    assert err < _tol(dt)
    for b in sorted({0, 1, B // 2, B - 1} | {r[0] // tpe for r in runs[1:8]}):
        alone = one.apply(X[b:b + 1].contiguous(), None if mm is None else mm[b:b + 1].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(got[b])), b


def test_backward_survives_the_plan_cache():
    """the plan of the forward may have left the cache (closed) before the backward runs: the backward asks for it again"""
    torch.manual_seed(2)
    w = torch.hann_window(16, dtype=torch.float64)
    fb = mf.melscale_fbanks(9, 0.0, 8000.0, 3, 16000)
    x = torch.randn(2, 80, device=DEV, dtype=torch.float64)

    def grads(between):
        out = []
        for fn in (lambda t: torch.view_as_real(mf.stft(t, 16, 4, window=w)), lambda t: mf.spectrogram(t, 16, 4, window=w, power=1),
                   lambda t: mf.spectrogram(t, 16, 4, window=w, power=2, fb=fb, log="log")):
            xg = x.clone().requires_grad_()
            y = fn(xg)
            gy = torch.linspace(0.5, 1.5, y.numel(), device=DEV, dtype=y.dtype).reshape(y.shape)
            between()
            y.backward(gy)
            out.append(xg.grad.clone())
        return out

    def many_plans():  # more distinct plans than the cache holds
        z = torch.randn(1, 64, device=DEV)
        for k in range(40):
            mf.stft(z[:, :40 + k], 16, 4)

    base = grads(lambda: None)
    for between in (mf.clear_plan_cache, many_plans):
        for a, b in zip(base, grads(between)):
            assert torch.equal(_bits(a), _bits(b))


def test_window_and_matrices_are_taken_by_value():
    """a window or filterbank changed in place between forward and backward does not reach the backward"""
    torch.manual_seed(4)
    x = torch.randn(2, 80, device=DEV, dtype=torch.float64)
    res = []
    for spoil in (False, True):
        w = torch.hann_window(16, dtype=torch.float64)
        fb = mf.melscale_fbanks(9, 0.0, 8000.0, 3, 16000)
        xg = x.clone().requires_grad_()
        y = mf.spectrogram(xg, 16, 4, window=w, power=2, fb=fb, log="log")
        if spoil:
            w.mul_(3.0)
            fb.add_(1.0)
        y.backward(torch.linspace(0.5, 1.5, y.numel(), device=DEV, dtype=y.dtype).reshape(y.shape))
        res.append(xg.grad.clone())
    assert torch.equal(_bits(res[0]), _bits(res[1]))


def test_plan_facts_and_exec_refusals():
    B, T, n, hop = 3, 50, 16, 4
    w = window_of("hann", n)
    for mult, k in ((None, 1), (2, 2), (1, 3)):
        plan = mf.plan_stft_adjoint(torch.float32, B, T, n, hop, window=w, center="reflect", multiplier=mult)
        assert plan.kernel_name(2).endswith(f"_istft_adj{k}_jit"), plan.kernel_name(2)
        assert plan.kernel_name(0) == plan.kernel_name(1) == "none"
        assert plan.num_launches == 1 and plan.scratch_bytes == 0
        bins = n // 2 + 1
        assert plan.in_bytes == B * plan.frames * bins * 4 * (2 + (mult is not None))
        assert plan.out_bytes == B * (T + n) * 4
    p1 = mf.plan_stft_adjoint(torch.float32, B, T, n, hop, window=w, center="reflect")
    p2 = mf.plan_stft_adjoint(torch.float32, B, T, n, hop, window=w, center="constant", multiplier=2)
    assert p2.edge_shape is None and p2.out_bytes == B * T * 4
    X, m = _plan_inputs((B, T, n, hop, "reflect", "hann"), torch.float32)
    out = torch.empty(p1.out_shape, device=DEV)
    edge = torch.empty(p1.edge_shape, device=DEV)

    def status(fn):
        with pytest.raises(mf.MifftError) as e:
            fn()
        return e.value.status, str(e.value)

    assert status(lambda: p1.run(out, X))[0] == -12                                  # edge missing
    assert status(lambda: p1.run(out, X, multiplier=m, edge=edge))[0] == -15          # mult superfluous
    assert status(lambda: p2.run(out, X))[0] == -12                                  # mult missing
    assert status(lambda: p2.run(out, X, multiplier=m, edge=edge))[0] == -15          # edge superfluous
    big = torch.empty(X.numel() + out.numel(), device=DEV)
    alias_out = big[:out.numel()].view(p1.out_shape)
    alias_x = big[out.numel() - 2:out.numel() - 2 + X.numel()].view(X.shape)
    assert status(lambda: p1.run(alias_out, alias_x, edge=edge))[0] == -13            # x overlaps out
    st, why = status(lambda: mf.fft(out, X, plan=p1))
    assert st == -15 and "run" in why
    torch.cuda.synchronize()


def test_what_the_adjoint_cannot_do_raises_in_the_forward():
    x = torch.randn(2, 200, device=DEV)
    assert mf.stft(x, 16, 20, center=False).grad_fn is None                  # hop > n_fft: the forward alone works
    with pytest.raises(mf.MifftError) as e:
        mf.stft(x.clone().requires_grad_(), 16, 20, center=False)
    assert "requires_grad" in str(e.value)
    x64 = torch.randn(1, 30000, device=DEV, dtype=torch.float64)
    assert mf.stft(x64, 12288, 4096).grad_fn is None                          # fp64 frames beyond 10240
    with pytest.raises(mf.MifftError) as e:
        mf.spectrogram(x64.clone().requires_grad_(), 12288, 4096)
    assert "requires_grad" in str(e.value)
