"""Gradients of mdct and imdct: each is one launch of the other's fused plan (the fold and the unfold are transposes, the
DCT-IV is symmetric), held against torch.autograd over a dense fp64 cosine-matrix model on the CPU
(tests/istft_grad_reference.py: mdct_model, imdct_model)."""
import functools
import math

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf

from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
import istft_grad_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3
DTYPES = [torch.float32, torch.float64]
NS = [8, 16, 256]
CASES = [(n, T, win, norm) for n in NS for T in (2, n - 1, n, 3 * n + 5) for win in ("sine", "random") for norm in (None, "ortho")]


def _id(v):
    return str(v).replace("torch.", "")


def _tol(dt):
    return REL_L2_TOL_F32 if dt == torch.float32 else REL_L2_TOL_F64


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _window(n, win):
    if win == "sine":
        return None, mf.mdct_window(n).numpy()
    w = np.random.default_rng(n).uniform(0.2, 1.5, 2 * n)  # not symmetric
    return torch.from_numpy(w), w


def _block_err(got, ref, n):
    """relative L2 per block of n values along the last dim (the last block may be short), the maximum"""
    worst = 0.0
    for lo in range(0, ref.shape[-1], n):
        num = np.linalg.norm(got[..., lo:lo + n] - ref[..., lo:lo + n], axis=-1)
        den = np.linalg.norm(ref[..., lo:lo + n], axis=-1)
        worst = max(worst, float((num / den).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _mdct_reference(n, T, win, norm, dt):
    """x and gy rounded to ``dt``, and the fp64 gradient of <mdct_model(x), gy> by torch.autograd on the CPU: never modified"""
    g = torch.Generator().manual_seed(n * 1000 + T)
    F = mf.mdct_frames(T, n)
    x = torch.randn(B, T, generator=g, dtype=torch.float64).to(dt)
    gy = torch.randn(B, F, n, generator=g, dtype=torch.float64).to(dt)
    scale = math.sqrt(2.0 / n) if norm == "ortho" else 1.0
    xr = x.double().clone().requires_grad_(True)
    y = R.mdct_model(xr, n, _window(n, win)[1], scale)
    y.backward(gy.double())
    return x, gy, y.detach().numpy(), xr.grad.numpy()


@functools.lru_cache(maxsize=None)
def _imdct_reference(n, T, F, win, norm, dt):
    g = torch.Generator().manual_seed(n * 1000 + T + 7 * F)
    X = torch.randn(B, F, n, generator=g, dtype=torch.float64).to(dt)
    gy = torch.randn(B, T, generator=g, dtype=torch.float64).to(dt)
    gain = math.sqrt(2.0 / n) if norm == "ortho" else 2.0 / n
    Xr = X.double().clone().requires_grad_(True)
    y = R.imdct_model(Xr, n, _window(n, win)[1], gain, T)
    y.backward(gy.double())
    return X, gy, y.detach().numpy(), Xr.grad.numpy()


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("n,T,win,norm", CASES, ids=_id)
def test_mdct_gradient_matches_the_dense_model(n, T, win, norm, dt):
    x, gy, y_ref, gx_ref = _mdct_reference(n, T, win, norm, dt)
    w = _window(n, win)[0]
    xd = x.to(DEV).requires_grad_(True)
    y = mf.mdct(xd, n, window=w, norm=norm)
    assert y.grad_fn is not None and y.shape == gy.shape
    with torch.no_grad():
        plain = mf.mdct(xd, n, window=w, norm=norm)
    assert plain.grad_fn is None and torch.equal(_bits(plain), _bits(y.detach()))  # the forward is the same launch, bit for bit
    y.backward(gy.to(DEV))
    assert xd.grad.shape == xd.shape and xd.grad.dtype == dt
    err = _block_err(xd.grad.cpu().double().numpy(), gx_ref, n)
    print(f"mdct grad n {n} T {T} {win} {norm} {_id(dt)}: worst rel-L2 per block {err:.3e}")
    assert err <= _tol(dt), err


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("n,T,win,norm", CASES, ids=_id)
def test_imdct_gradient_matches_the_dense_model(n, T, win, norm, dt):
    F = mf.mdct_frames(T, n)
    X, gy, y_ref, gX_ref = _imdct_reference(n, T, F, win, norm, dt)
    w = _window(n, win)[0]
    Xd = X.to(DEV).requires_grad_(True)
    y = mf.imdct(Xd, window=w, norm=norm, length=T)
    assert y.grad_fn is not None and y.shape == gy.shape
    with torch.no_grad():
        plain = mf.imdct(Xd, window=w, norm=norm, length=T)
    assert plain.grad_fn is None and torch.equal(_bits(plain), _bits(y.detach()))
    y.backward(gy.to(DEV))
    assert Xd.grad.shape == Xd.shape and Xd.grad.dtype == dt
    got = Xd.grad.cpu().double().numpy()
    err = float((np.linalg.norm(got - gX_ref, axis=-1) / np.linalg.norm(gX_ref, axis=-1)).max())
    print(f"imdct grad n {n} T {T} {win} {norm} {_id(dt)}: worst rel-L2 per frame {err:.3e}")
    assert err <= _tol(dt), err


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("batch", [1, B], ids=lambda b: f"batch{b}")
@pytest.mark.parametrize("n", NS, ids=_id)
def test_imdct_gradient_with_a_cropped_length(n, batch, dt):
    """length cropped by more than one frame: the frames beyond mdct_frames(length, n) are exact zeros, the others the model's"""
    T = n + 3
    Fm, F = mf.mdct_frames(T, n), mf.mdct_frames(T, n) + 2
    X, gy, _, gX_ref = _imdct_reference(n, T, F, "random", None, dt)
    X, gy, gX_ref = X[:batch], gy[:batch], gX_ref[:batch]
    Xd = X.to(DEV).requires_grad_(True)
    mf.imdct(Xd, window=_window(n, "random")[0], length=T).backward(gy.to(DEV))
    got = Xd.grad.cpu().double().numpy()
    assert (gX_ref[:, Fm:] == 0).all() and (got[:, Fm:] == 0).all()
    err = float((np.linalg.norm(got[:, :Fm] - gX_ref[:, :Fm], axis=-1) / np.linalg.norm(gX_ref[:, :Fm], axis=-1)).max())
    assert err <= _tol(dt), err


@pytest.mark.parametrize("n,T", [(8, 29), (16, 53), (256, 773)], ids=_id)
def test_dot_product_identities_on_the_device(n, T):
    g = torch.Generator().manual_seed(n + T)
    w = _window(n, "random")[0]
    x = torch.randn(B, T, generator=g, dtype=torch.float64).to(DEV)
    F = mf.mdct_frames(T, n)
    Y = torch.randn(B, F, n, generator=g, dtype=torch.float64).to(DEV)
    xg = x.clone().requires_grad_(True)
    Xm = mf.mdct(xg, n, window=w)
    Xm.backward(Y)
    lhs, rhs = float((Xm.detach() * Y).sum()), float((x * xg.grad).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    Z = torch.randn(B, F + 1, n, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    gy = torch.randn(B, T, generator=g, dtype=torch.float64).to(DEV)
    y = mf.imdct(Z, window=w, length=T)
    y.backward(gy)
    lhs, rhs = float((y.detach() * gy).sum()), float((Z.detach() * Z.grad).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)


def test_gradcheck_fp64():
    torch.manual_seed(4)
    w = _window(8, "random")[0]
    x = torch.randn(2, 21, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: mf.mdct(t, 8, window=w), (x,), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda t: mf.mdct(t, 8, norm="ortho"), (x,), nondet_tol=0)
    X = torch.randn(2, 5, 8, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: mf.imdct(t, window=w), (X,), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda t: mf.imdct(t, norm="ortho", length=19), (X,), nondet_tol=0)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_the_plain_calls_keep_their_bits(dt):
    """without requires_grad: the bits of the plans run directly, and no grad_fn"""
    n, T = 16, 53
    F = mf.mdct_frames(T, n)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, T, generator=g, dtype=torch.float64).to(dt).to(DEV)
    out = torch.empty((B, F, n, 1), dtype=dt, device=DEV)
    mf.fft(out, x.reshape(B, T, 1), plan=mf.plan_mdct(dt, B, T, n))
    y = mf.mdct(x, n)
    assert y.grad_fn is None and torch.equal(_bits(y), _bits(out.reshape(B, F, n)))
    X = torch.randn(B, F, n, generator=g, dtype=torch.float64).to(dt).to(DEV)
    back = torch.empty((B, T, 1), dtype=dt, device=DEV)
    mf.fft(back, X.reshape(B, F, n, 1), plan=mf.plan_imdct(dt, B, F, n, length=T))
    z = mf.imdct(X, length=T)
    assert z.grad_fn is None and torch.equal(_bits(z), _bits(back.reshape(B, T)))


def test_imdct_of_one_sample_has_no_gradient():
    X = torch.randn(2, 3, 8, dtype=torch.float32, device=DEV)
    assert mf.imdct(X, length=1).shape == (2, 1)  # the forward alone works
    with torch.no_grad():
        assert mf.imdct(X.clone().requires_grad_(True), length=1).shape == (2, 1)
    with pytest.raises(mf.MifftError) as e:
        mf.imdct(X.clone().requires_grad_(True), length=1)
    assert e.value.status == -15 and "no_grad" in str(e.value)
