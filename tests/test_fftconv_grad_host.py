"""The filter gradient of fftconv without a device: an fp64 numpy model of the pair geometry of TileCfg::WGRAD (u-blocks,
g-blocks, the sum of conj(U) G over the slices of a channel's pairs) against the direct double sum; the model of the whole
backward of the gated op against torch CPU autograd of the composition; every refusal of the MIFFT_CONV_GRAD_TAG payload
that needs no device, and every host-side validation of plan_fftconv_grad, fftconv_filter_grad and the differentiable
fftconv.  The GPU tests (test_gpu_fftconv_grad.py) compare the kernel with the models defined here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from test_fftconv_long_host import geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STFT = 32
UNSUPPORTED = -15
TOO_LARGE = -9
TAG_LO, TAG_HI = 0x44524701, 0x7FF84D47
MAGIC = 0x314757544646494D


# ---- the model (fp64): the walk of the kernel's workgroups ------------------------------------------------------------------
def pair_slices(Q, P):
    """the P contiguous ascending ranges of Q pairs, lengths differing by one at most"""
    ln, rem = divmod(Q, P)
    out, q = [], 0
    for s in range(P):
        e = q + ln + (1 if s < rem else 0)
        out.append((q, e))
        q = e
    assert q == Q
    return out


def blocks_of(x, gy, n, c, S, s0, f, Lo):
    """u-block and g-block of block f of one row"""
    L = x.shape[0]
    i = np.arange(n)
    src = s0 + f * S + i
    ub = np.where((src >= 0) & (src < L), x[np.clip(src, 0, L - 1)], 0.0)
    t = f * S + i - c
    ok = (i >= c) & (i < c + S) & (t < Lo)
    gb = np.where(ok, gy[np.clip(t, 0, Lo - 1)], 0.0)
    return ub, gb, t[ok]


def wgrad_model(x, gy, n, D, c, S, s0, F, Lo, correlate=False, P=1, used=None):
    """A[p, d, k] of the kernel: x (R, L), gy (R, Lo) -> (P, D, n // 2 + 1) complex, unscaled.  ``used`` (R, Lo) counts how
    often every sample of gy enters a block."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    R = x.shape[0]
    assert R % D == 0 and gy.shape == (R, Lo)
    B = R // D
    A = np.zeros((P, D, n // 2 + 1), dtype=np.complex128)
    for d in range(D):
        for p, (q0, q1) in enumerate(pair_slices(B * F, P)):
            for q in range(q0, q1):
                b, f = divmod(q, F)
                r = b * D + d
                ub, gb, t = blocks_of(x[r], gy[r], n, c, S, s0, f, Lo)
                if used is not None:
                    used[r, t] += 1
                A[p, d] += np.conj(np.fft.rfft(ub)) * np.fft.rfft(gb)
    return np.conj(A) if correlate else A


def gk_of(A, n, K):
    return np.fft.irfft(A.sum(0), n, axis=-1)[:, :K]


def gk_direct(x, gy, D, K, o, correlate=False, n=None):
    """gk[d, j] = sum_r sum_t gy[r, t] x[r, o + t - j] (correlate: o + t + j); with n, indices modulo n (the circular forward)"""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    R, L = x.shape
    Lo = gy.shape[1]
    xe = np.zeros((R, n if n else L))
    xe[:, :L] = x
    gk = np.zeros((D, K))
    for r in range(R):
        for j in range(K):
            for t in range(Lo):
                s = o + t + j if correlate else o + t - j
                if n:
                    s %= n
                if 0 <= s < xe.shape[1]:
                    gk[r % D, j] += gy[r, t] * xe[r, s]
    return gk


def worst_row(got, ref):
    """the worst row's relative l2 (real or complex rows)"""
    wide = lambda v: np.asarray(v, dtype=np.complex128 if np.iscomplexobj(v) else np.float64)
    got, ref = wide(got), wide(ref)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max())


# (n, L, K, o, Lo, correlate): single blocks with o = 0 and o > 0, circular ones, a correlation
SINGLE = [(64, 37, 28, 0, 37, False), (64, 37, 28, 13, 37, False), (96, 50, 40, 0, 89, False), (16, 11, 5, 4, 7, False),
          (32, 30, 9, 0, 30, False), (32, 30, 9, 4, 28, False), (64, 37, 28, 0, 37, True), (32, 30, 9, 0, 30, True)]


@pytest.mark.parametrize("n,L,K,o,Lo,correlate", SINGLE, ids=lambda v: str(v))
@pytest.mark.parametrize("P", [1, 3])
def test_single_block_model_against_the_direct_sum(n, L, K, o, Lo, correlate, P):
    rng = np.random.default_rng(n * 1000 + L + o)
    D, B = 3, 2
    x, gy = rng.standard_normal((B * D, L)), rng.standard_normal((B * D, Lo))
    used = np.zeros((B * D, Lo), dtype=int)
    A = wgrad_model(x, gy, n, D, o, Lo, 0, 1, Lo, correlate, P=min(P, B), used=used)
    assert (used == 1).all()
    circular = n < L + K - 1
    want = gk_direct(x, gy, D, K, o, correlate, n=n if circular else None)
    assert worst_row(gk_of(A, n, K), want) <= 1e-12


# (n, T, K): odd S (n - K + 1), Lo no multiple of S
LONG = [(64, 300, 20), (16, 101, 8), (64, 333, 28), (96, 777, 40)]


@pytest.mark.parametrize("n,T,K", LONG, ids=lambda v: str(v))
@pytest.mark.parametrize("mode,correlate", [("causal", False), ("full", False), ("same", False), ("valid", False), ("causal", True)])
def test_overlap_save_model_against_the_direct_sum(n, T, K, mode, correlate):
    rng = np.random.default_rng(n + T + K)
    D, B = 2, 2
    o, Lo = mf.api._fftconv_window(mode, T, K)
    c, S, s0, F = geometry(n, K, o, Lo, correlate)
    assert (c, S, s0, F) == mf.api._fftconv_ols_geometry(n, K, o, Lo, correlate)
    assert S % 2 == 1 or n in (16,), S
    x, gy = rng.standard_normal((B * D, T)), rng.standard_normal((B * D, Lo))
    used = np.zeros((B * D, Lo), dtype=int)
    A = wgrad_model(x, gy, n, D, c, S, s0, F, Lo, correlate, P=3, used=used)
    assert (used == 1).all(), "every output sample enters exactly one block"
    assert worst_row(gk_of(A, n, K), gk_direct(x, gy, D, K, o, correlate)) <= 1e-12
    # the partition does not change the sum beyond rounding
    A1 = wgrad_model(x, gy, n, D, c, S, s0, F, Lo, correlate, P=1)
    assert np.abs(A.sum(0) - A1[0]).max() <= 1e-11 * np.abs(A1).max()


def test_pair_slices():
    for Q, P in ((10, 3), (3, 3), (7, 1), (4000, 256), (5, 4)):
        s = pair_slices(Q, P)
        lens = [b - a for a, b in s]
        assert sum(lens) == Q and max(lens) - min(lens) <= 1 and lens == sorted(lens, reverse=True)


# ---- the model of the whole backward against torch CPU autograd of the composition ------------------------------------------
def composition(x, k, a, b, d, n, o, Lo, correlate):
    """b * irfft(rfft(a x, n) (rfft(k, n) + d), n)[o : o + Lo] on CPU tensors (k (D, K) or (K,); d (D,), a float or None)"""
    u = x if a is None else a * x
    H = torch.fft.rfft(k, n=n)
    if d is not None:
        H = H + (d.reshape(-1, 1) if isinstance(d, torch.Tensor) and k.dim() == 2 else d)
    if correlate:
        H = H.conj()
    y = torch.fft.irfft(torch.fft.rfft(u, n=n) * H, n=n)[..., o:o + Lo]
    return y if b is None else b * y


def reference_grads(x, k, a, b, d, gy, n, o, Lo, correlate):
    """fp64 torch CPU autograd of the composition: gradients of x, k, a, b, d (None where the input is None or a float)"""
    t = lambda v: None if v is None else (torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True)
                                          if not isinstance(v, float) else v)
    xs, ks, as_, bs, ds = t(x), t(k), t(a), t(b), t(d)
    y = composition(xs, ks, as_, bs, ds, n, o, Lo, correlate)
    y.backward(torch.as_tensor(np.asarray(gy), dtype=torch.float64))
    g = lambda v: None if v is None or isinstance(v, float) else v.grad.numpy()
    return y.detach().numpy(), g(xs), g(ks), g(as_), g(bs), g(ds)


def backward_model(x, k, a, b, d, gy, n, o, Lo, correlate):
    """what the backward of the Function computes, in fp64 numpy, single block: x, a (B, D, L); b, gy (B, D, Lo); k (D, K)"""
    B, D, L = x.shape
    K = k.shape[1]
    u = x if a is None else a * x
    gv = gy if b is None else b * gy
    G = np.fft.rfft(k, n, axis=-1) + (0.0 if d is None else np.reshape(d, (-1, 1)))
    if correlate:
        G = np.conj(G)
    gvp = np.zeros((B, D, n))
    gvp[..., o:o + Lo] = gv
    gu = np.fft.irfft(np.fft.rfft(gvp, axis=-1) * np.conj(G), n, axis=-1)[..., :L]
    v = np.fft.irfft(np.fft.rfft(u, n, axis=-1) * G, n, axis=-1)[..., o:o + Lo]
    A = wgrad_model(u.reshape(B * D, L), gv.reshape(B * D, Lo), n, D, o, Lo, 0, 1, Lo, correlate)
    g = np.fft.irfft(A.sum(0), n, axis=-1)
    return (gu if a is None else a * gu), g[:, :K], (None if a is None else x * gu), (None if b is None else gy * v), g[:, 0]


@pytest.mark.parametrize("n,L,K,mode,correlate", [(96, 50, 40, "causal", False), (96, 50, 40, "full", False),
                                                  (96, 50, 40, "same", False), (128, 50, 40, "valid", False),
                                                  (96, 50, 40, "causal", True), (64, 50, 40, "causal", False)])
def test_backward_model_against_torch_autograd(n, L, K, mode, correlate):
    rng = np.random.default_rng(L + K + n)
    B, D = 3, 2
    o, Lo = mf.api._fftconv_window(mode, L, K)
    x, a = rng.standard_normal((B, D, L)), rng.standard_normal((B, D, L))
    b, gy = rng.standard_normal((B, D, Lo)), rng.standard_normal((B, D, Lo))
    k, d = rng.standard_normal((D, K)), rng.standard_normal(D)
    _, rx, rk, ra, rb, rd = reference_grads(x, k, a, b, d, gy, n, o, Lo, correlate)
    gx, gk, ga, gb, gd = backward_model(x, k, a, b, d, gy, n, o, Lo, correlate)
    for got, ref in ((gx, rx), (gk, rk), (ga, ra), (gb, rb)):
        assert worst_row(got, ref) <= 1e-12
    assert np.abs(gd - rd).max() <= 1e-12 * np.abs(rd).max()


# ---- the C ABI: what is refused before a device is looked for ---------------------------------------------------------------
def _create(L=37, n=64, *, batch=6, D=3, c=0, S=37, mode=0, F=1, s0=0, Lo=37, P=0, rsv=(0,) * 6, flags=STFT, radices=(),
            in_dtype=0, out_dtype=0, inverse=0, comps=1, device=0, len0=16, tag=(TAG_LO, TAG_HI)):
    """the default: a single block, rows of 37 samples at n = 64, o = 0, Lo = 37, the library's choice of P"""
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = [tag[0], tag[1], D, c, S, mode, F, s0 & 0xFFFFFFFF, Lo, P] + list(rsv) + list(radices)
    lens = (ctypes.c_int32 * 2)(len0, len(radices))
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(L, n), batch, comps, inverse,
                               (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


OLS = dict(L=1000, S=45, c=19, s0=-19, F=23, Lo=1000)  # (n = 64, K = 20)


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            (dict(S=0), -5, "S >= 1"),
            (dict(c=30, S=37, Lo=37), -5, "c + S <= n"),
            (dict(D=0), -5, "D >= 1"),
            (dict(D=4), -8, "multiple of D"),
            (dict(mode=2), -5, "mode word"),
            (dict(F=0), -5, "F >= 1"),
            (dict(Lo=0, S=1), -5, "F >= 1"),
            (dict(Lo=38), -5, "(F - 1) S < Lo <= F S"),
            (dict(OLS, Lo=1036), -5, "(F - 1) S < Lo <= F S"),
            (dict(OLS, Lo=990), -5, "(F - 1) S < Lo <= F S"),
            (dict(OLS, s0=-64), -5, "reads no sample"),
            (dict(OLS, s0=11), -5, "reads no sample"),
            (dict(OLS, L=(1 << 30) + 1), TOO_LARGE, "2 <= T"),
            (dict(P=3), -5, "partial sums"),           # 2 pairs per channel
            (dict(P=70000, batch=300000), -5, "partial sums"),
            (dict(rsv=(0, 0, 1, 0, 0, 0)), -5, "reserved word 12"),
            (dict(rsv=(5, 0, 0, 0, 0, 0)), -5, "reserved word 10"),
            (dict(n=63), UNSUPPORTED, "even length"),
            (dict(n=6, L=5, S=5, Lo=5), UNSUPPORTED, "even length"),
            (dict(n=32768, L=100, S=100, Lo=100), UNSUPPORTED, "even length"),
            (dict(n=16384, L=100, S=100, Lo=100, in_dtype=1, out_dtype=1), UNSUPPORTED, "FFT length"),
            (dict(n=74), UNSUPPORTED, "FFT length"),   # n / 2 = 37, a prime above 32
            (dict(inverse=1), UNSUPPORTED, "inverse must be 0"),
            (dict(comps=2), -3, "real rows"),
            (dict(in_dtype=0, out_dtype=1), -4, "float type"),
            (dict(flags=STFT | 0x8000), UNSUPPORTED, "MIFFT_CONV_GRAD_TAG"),
            (dict(flags=STFT | (16 << 16)), UNSUPPORTED, "hop"),
            (dict(flags=STFT | 2), UNSUPPORTED, "HALF_SPECTRUM"),
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw, rc, why)


def test_a_valid_request_gets_as_far_as_the_device():
    for kw in (dict(), dict(c=13), dict(mode=1), dict(D=1), dict(P=1), dict(P=2), dict(n=16, L=11, S=7, c=4, Lo=7),
               dict(n=16384, L=8192, S=8192, Lo=8192), dict(n=12288, L=6000, S=6000, Lo=6000, in_dtype=1, out_dtype=1),
               dict(radices=(2,)), OLS, dict(OLS, mode=1, c=0, s0=0), dict(OLS, Lo=993), dict(OLS, P=46),
               dict(L=100, S=37, Lo=37)):  # (one block of a longer row: the overlap-save geometry)
        rc, why = _create(device=-1, **kw)
        assert rc == -10 and "device" in why, (kw, rc, why)


def test_the_old_payloads_mean_what_they_meant():
    from test_fftconv_host import _create as create8
    rc, why = create8(mode=2)
    assert rc == -5 and "mode" in why, (rc, why)
    # the new tag in front of 8 or 12 words is no payload at all
    for len0 in (8, 12, 15, 17):
        rc, why = _create(len0=len0)
        assert rc != 0 and rc != -10, (len0, rc, why)


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_fftconv_grad_host import _create\n"
            "print(*_create(device=-1))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(str(UNSUPPORTED)) and "MIFFT_JIT=0" in r.stdout, r.stdout


def test_the_tag_and_the_argument_block_are_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    m = re.search(r"#define\s+MIFFT_CONV_GRAD_ARGS_MAGIC\s+0x([0-9A-Fa-f]+)ull\b", h)
    assert m and int(m.group(1), 16) == MAGIC == mf.CONV_GRAD_ARGS_MAGIC
    assert MAGIC.to_bytes(8, "little") == b"MIFFTWG1"
    lo = re.search(r"#define\s+MIFFT_CONV_GRAD_TAG_LO\s+0x([0-9A-Fa-f]+)u\b", h)
    hi = re.search(r"#define\s+MIFFT_CONV_GRAD_TAG_HI\s+0x([0-9A-Fa-f]+)u\b", h)
    assert (int(lo.group(1), 16), int(hi.group(1), 16)) == (TAG_LO, TAG_HI) == (mf.CONV_GRAD_TAG_LO, mf.CONV_GRAD_TAG_HI)
    assert (TAG_LO, TAG_HI) != (mf.CONV_TAG_LO, mf.CONV_TAG_HI)
    assert np.isnan(np.array([TAG_LO, TAG_HI], dtype=np.uint32).view(np.float64)[0])  # (no window value: a NaN)
    assert re.search(r"typedef struct mifft_conv_grad_args \{\s*uint64_t magic;[^}]*const void\* x;[^}]*const void\* gy;", h)
    assert [f[0] for f in mf.ConvGradArgs._fields_] == ["magic", "x", "gy"] and ctypes.sizeof(mf.ConvGradArgs) == 24


# ---- the Python entry points: every argument error comes before any device work ---------------------------------------------
def test_plan_fftconv_grad_validates_on_the_host():
    f32 = torch.float32
    for args, kw, status in (
            ((torch.int32, 2, 3, 40, 64), {}, -4),
            ((f32, 0, 3, 40, 64), {}, -8),
            ((f32, 2, 0, 40, 64), {}, -8),
            ((f32, 2, 3, 40, 74), {}, UNSUPPORTED),
            ((torch.float64, 2, 3, 40, 16384), {}, UNSUPPORTED),
            ((f32, 2, 3, 65, 64), {}, UNSUPPORTED),
            ((f32, 2, 3, 1, 64), {}, UNSUPPORTED),
            ((f32, 2, 3, 40, 64), dict(offset=30, out_length=40), -5),
            ((f32, 2, 3, 40, 64), dict(out_length=0), -5),
            ((f32, 2, 3, 40, 64), dict(taps=64), -2),
            ((f32, 2, 3, 40, 64), dict(taps=0), -2),
            ((f32, 2, 3, 1, 64), dict(taps=9), UNSUPPORTED),
            ((f32, 2, 3, 400, 64), dict(taps=9, offset=10, out_length=400), -5),
            ((f32, 2, 3, 400, 64), dict(taps=9, correlate=True, out_length=401), -5),
            ((f32, 2, 3, 40, 64), dict(partials=0), -5),
            ((f32, 2, 3, 40, 64), dict(partials=70000), -5),
    ):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv_grad(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
    for kw in (dict(), dict(taps=9), dict(partials=2), dict(correlate=True), dict(offset=4, out_length=50)):
        with pytest.raises(mf.MifftError) as e:  # (a valid request: as far as the device)
            mf.plan_fftconv_grad(f32, 2, 3, 40, 64, **kw)
        assert e.value.status == -10, kw


def test_fftconv_filter_grad_validates_on_the_host():
    x, gy = torch.zeros(2, 3, 40), torch.zeros(2, 3, 40)  # (host tensors: nothing reaches the library)
    for args, kw, exc in (
            ((x.to(torch.complex64), gy, 9), {}, mf.MifftError),
            ((x, gy, 9), dict(mode="circular"), ValueError),
            ((x, gy, 9), dict(mode="full", correlate=True), ValueError),
            ((x, gy[0], 9), {}, mf.MifftError),
            ((x, gy, 0), {}, mf.MifftError),
            ((torch.zeros(2, 3, 1), torch.zeros(2, 3, 1), 1), {}, mf.MifftError),
            ((x, gy, 9), dict(n=64, block=64), ValueError),
            ((x, gy, 9), dict(n=32), mf.MifftError),
            ((x, gy, 9), dict(n=74), mf.MifftError),
            ((x, gy, 70), dict(block=64), mf.MifftError),
            ((x, gy, 9), dict(mode="full"), ValueError),     # gy has 40 samples, the result 48
            ((x, torch.zeros(2, 3, 41), 9), {}, ValueError),
    ):
        with pytest.raises(exc):
            mf.fftconv_filter_grad(*args, **kw)
    with pytest.raises(mf.MifftError) as e:  # (a valid request gets as far as the device check)
        mf.fftconv_filter_grad(x, gy, 9)
    assert e.value.status == -10


def test_differentiable_fftconv_validates_as_before():
    x = torch.zeros(2, 3, 40, requires_grad=True)
    k = torch.zeros(3, 9, requires_grad=True)
    with pytest.raises(ValueError):
        mf.fftconv(x, k, mode="circular")
    with pytest.raises(ValueError):
        mf.fftconv(x, k, pregate=torch.zeros(2, 3, 41))
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(x, k, n=32)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:  # (host tensors: refused at the device check, before any autograd node exists)
        mf.fftconv(x, k)
    assert e.value.status == -10
    assert "autograd" in mf.fftconv.__doc__ and "Not differentiable" not in mf.fftconv.__doc__
