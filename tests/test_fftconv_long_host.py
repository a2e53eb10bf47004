"""Overlap-save fftconv (the 12-word MIFFT_CONV_TAG payload): an fp64 model of the payload's block loop against numpy.convolve
and scipy.signal.fftconvolve, the wrapper's block geometry, fftconv_block against a brute-force search of its rule, every
refusal that needs no device, and the wrappers' host validation."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT

STFT, REFLECT, ZEROS, POWER, ISTFT = 32, 64, 128, 0x8000, 0x4000
UNSUPPORTED = -15
TAG_LO, TAG_HI = 0x4F4E5601, 0x7FF84D43
MODES = ("causal", "full", "same", "valid")
SHAPES = [(100, 5, 16), (101, 9, 16), (333, 15, 16), (37, 28, 64), (1000, 33, 64), (50, 1, 8)]  # (T, K, n)


# ---- the model (fp64): the block loop of the payload ---------------------------------------------------------------------------
def ols_model(x, k, n, c, S, s0, F, Lo, correlate=False):
    """rows x (R, T) against filters k (D, K) or (K,), row r with filter r % D.  Block f: blk[i] = x[r][s0 + f S + i], zeros
    outside the row; y = irfft(rfft(blk) G[r % D], n); out[r][f S + j] = y[c + j] for j < S and f S + j < Lo."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    k = np.atleast_2d(np.asarray(k, dtype=np.float64))
    R, T = x.shape
    D = k.shape[0]
    assert S >= 1 and c + S <= n and F >= 1 and (F - 1) * S < Lo <= F * S
    G = np.fft.rfft(k, n, axis=-1)
    if correlate:
        G = np.conj(G)
    out = np.full((R, Lo), np.nan)
    for f in range(F):
        st = s0 + f * S
        assert -n < st < T, (f, st)  # (every block reads a sample of its row)
        blk = np.zeros((R, n))
        lo, hi = max(st, 0), min(st + n, T)
        blk[:, lo - st:hi - st] = x[:, lo:hi]
        y = np.fft.irfft(np.fft.rfft(blk, axis=-1) * G[np.arange(R) % D], n, axis=-1)
        w = min(S, Lo - f * S)
        out[:, f * S:f * S + w] = y[:, c:c + w]
    assert not np.isnan(out).any()  # (every sample written)
    return out


def geometry(n, K, offset, out_length, correlate=False):
    """(c, S, s0, F) of an overlap-save plan, written out on its own: S samples per block are free of wrap-around, from K - 1
    on (correlation: from 0 on)"""
    S = n - (K - 1)
    c = 0 if correlate else K - 1
    return c, S, offset - c, (out_length + S - 1) // S


@pytest.mark.parametrize("T,K,n", SHAPES)
def test_the_model_against_numpy_and_scipy(T, K, n):
    rng = np.random.default_rng(T * 100 + K)
    D, B = 3, 2
    x, k = rng.standard_normal((B * D, T)), rng.standard_normal((D, K))
    full = np.stack([np.convolve(x[r], k[r % D]) for r in range(B * D)])
    for mode in MODES:
        o, Lo = mf.api._fftconv_window(mode, T, K)
        c, S, s0, F = geometry(n, K, o, Lo)
        assert (c, S, s0, F) == mf.api._fftconv_ols_geometry(n, K, o, Lo, False), mode
        got = ols_model(x, k, n, c, S, s0, F, Lo)
        for r in range(B * D):
            want = full[r][:T] if mode == "causal" else scipy.signal.fftconvolve(x[r], k[r % D], mode=mode)
            assert got[r].shape == want.shape, (mode, got[r].shape, want.shape)
            assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max(), (mode, r)
    # correlation: y[t] = sum_j k[j] x[t + j], zeros beyond the row
    c, S, s0, F = geometry(n, K, 0, T, True)
    assert (c, S, s0, F) == mf.api._fftconv_ols_geometry(n, K, 0, T, True)
    got = ols_model(x, k, n, c, S, s0, F, T, correlate=True)
    xp = np.concatenate([x, np.zeros((B * D, K))], axis=1)
    for r in range(B * D):
        want = np.array([np.dot(k[r % D], xp[r, t:t + K]) for t in range(T)])
        assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max()


def test_a_window_inside_the_full_convolution():
    rng = np.random.default_rng(11)
    T, K, n = 333, 15, 16
    x, k = rng.standard_normal((1, T)), rng.standard_normal((1, K))
    full = np.convolve(x[0], k[0])
    for o, Lo in ((0, 1), (5, 7), (200, 147), (T + K - 2, 1), (1, T + K - 2)):
        c, S, s0, F = geometry(n, K, o, Lo)
        got = ols_model(x, k, n, c, S, s0, F, Lo)
        assert np.abs(got[0] - full[o:o + Lo]).max() <= 1e-12 * np.abs(full).max(), (o, Lo)


# ---- fftconv_block -------------------------------------------------------------------------------------------------------------
# time per block sample at every block length, hundredths of the cheapest: the sweep of profiles/r17_fftconv_long.txt
WEIGHT = {torch.float32: {256: 100, 512: 136, 1024: 148, 2048: 154, 4096: 133, 8192: 179, 16384: 166},
          torch.float64: {256: 100, 512: 109, 1024: 117, 2048: 133, 4096: 163, 8192: 200}}


def test_fftconv_block_against_its_rule():
    for dtype, top in ((torch.float32, 16384), (torch.float64, 8192)):
        for K in sorted(set(range(1, 300)) | set(range(1, top // 2 + 2, 61)) | {top // 2, top // 2 + 1, 129, 1025, 4097}):
            if K > top // 2 + 1:
                continue
            cands = [n for n in (256 << i for i in range(7)) if n <= top and n >= 2 * (K - 1)]
            cost = {n: Fraction(WEIGHT[dtype][n] * n, n - K + 1) for n in cands}  # (exact: ties are real ties)
            best = min(cands, key=lambda n: (cost[n], n))
            assert mf.fftconv_block(K, dtype) == best, (K, dtype)
            assert K <= best - 1
        for K in (top // 2 + 2, top, 100000):
            with pytest.raises(mf.MifftError) as e:
                mf.fftconv_block(K, dtype)
            assert e.value.status == UNSUPPORTED and "partitioned" in str(e.value), K
    assert mf.fftconv_block(8193) == 16384 and mf.fftconv_block(4097, torch.float64) == 8192
    assert mf.fftconv_block(1) == 256
    # the picks at the filter lengths of tools/fftconv_long_probe.py
    assert [mf.fftconv_block(K) for K in (33, 257, 1025, 4097)] == [256, 4096, 16384, 16384]
    assert [mf.fftconv_block(K, torch.float64) for K in (33, 1025)] == [256, 4096]
    with pytest.raises(mf.MifftError):
        mf.fftconv_block(0)
    with pytest.raises(mf.MifftError):
        mf.fftconv_block(5, torch.float16)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _create12(T=1000, n=64, *, batch=6, D=3, c=32, S=32, mode=0, addr=0x10000, F=32, s0=-32, Lo=1000, w11=0, flags=STFT,
              radices=(), in_dtype=0, out_dtype=0, inverse=0, comps=1, device=0):
    """T = 1000, K = 33 at n = 64, causal: c = 32, S = 32, s0 = -32, F = ceil(1000 / 32) = 32"""
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = [TAG_LO, TAG_HI, D, c, S, mode, addr & 0xFFFFFFFF, addr >> 32, F, s0 & 0xFFFFFFFF, Lo, w11]
    lens = (ctypes.c_int32 * 2)(12, len(radices))
    flat = flat + list(radices)
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(T, n), batch, comps, inverse,
                               (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            # what the 8-word form refuses and still applies
            (dict(n=6, c=2, S=4), UNSUPPORTED, "8 to 16384"),
            (dict(n=74), UNSUPPORTED, "packed"),
            (dict(n=63), UNSUPPORTED, "even"),
            (dict(n=16386), UNSUPPORTED, "16384"),
            (dict(n=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),
            (dict(D=0), -5, "D"),
            (dict(D=4), -8, "multiple of D"),
            (dict(batch=7), -8, "multiple of D"),
            (dict(addr=0), -5, "null"),
            (dict(addr=0x10004), -5, "aligned"),
            (dict(addr=0x10008, in_dtype=1, out_dtype=1), -5, "aligned"),
            (dict(mode=2), -5, "mode"),
            (dict(inverse=1), UNSUPPORTED, "inverse"),
            (dict(in_dtype=2), -4, "in_dtype"),
            (dict(in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(comps=2), -3, "in_components"),
            (dict(flags=STFT | 1), UNSUPPORTED, "MIFFT_FLAG_FAITHFUL_STAGES"),
            (dict(flags=STFT | 2), UNSUPPORTED, "MIFFT_FLAG_HALF_SPECTRUM"),
            (dict(flags=STFT | 4), UNSUPPORTED, "MIFFT_FLAG_DCT"),
            (dict(flags=STFT | 16), UNSUPPORTED, "MIFFT_FLAG_DCT_ND"),
            (dict(flags=STFT | 8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(flags=STFT | (1 << 8)), UNSUPPORTED, "MIFFT_FLAG_KEEP_DIM"),
            (dict(flags=STFT | REFLECT), UNSUPPORTED, "centre bit"),
            (dict(flags=STFT | ZEROS), UNSUPPORTED, "centre bit"),
            (dict(flags=STFT | (16 << 16)), UNSUPPORTED, "hop"),
            (dict(flags=STFT | POWER), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (dict(flags=STFT | ISTFT), UNSUPPORTED, "MIFFT_FLAG_ISTFT"),
            (dict(radices=(3,)), -5, "length"),
            # the block geometry
            (dict(S=0), -5, "S >= 1"),
            (dict(c=33, S=32), -5, "c + S <= n"),
            (dict(c=64, S=1), -5, "c + S <= n"),
            (dict(F=0), -5, "F >= 1"),
            (dict(Lo=0), -5, "Lo >= 1"),
            (dict(Lo=992), -5, "(F - 1) S < Lo"),       # (F - 1) S = 992: the last block would store nothing
            (dict(Lo=1025), -5, "Lo <= F S"),            # F S = 1024
            (dict(s0=-64), -5, "reads no sample"),       # block 0 lies wholly before the row
            (dict(s0=-100), -5, "reads no sample"),
            (dict(s0=8), -5, "reads no sample"),         # s0 + 31 * 32 = 1000 = T: the last block lies wholly behind it
            (dict(T=960), -5, "reads no sample"),
            (dict(w11=1), -5, "word 11"),
            (dict(T=(1 << 30) + 1), -9, "2^30"),
    ):
        rc, why = _create12(**kw)
        assert rc == status and word in why, (kw, rc, why)
    rc, why = _create12(T=1, F=1, Lo=1, s0=0)  # (a row of one sample: what every plan is told)
    assert rc == -2, (rc, why)


def test_the_eight_word_payload_means_what_it_meant():
    from test_fftconv_host import _create
    rc, why = _create(mode=2)
    assert rc == -5 and "mode" in why, (rc, why)
    rc, why = _create(L=65)
    assert rc == UNSUPPORTED and "L > n" in why, (rc, why)
    rc, why = _create(o=30, Lo=35)
    assert rc == -5 and "o + Lo" in why, (rc, why)
    assert len(_lib.EXPORTS) == 21  # (no new entry point)
    # the tag in front of any other number of words is still no convolution
    lib = _lib.lib()
    for len0 in (9, 11, 13):
        h = ctypes.c_void_p()
        flat = [TAG_LO, TAG_HI] + [1] * (len0 - 2)
        rc = lib.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(1000, 64), 3, 1, 0,
                                   (ctypes.c_uint32 * len0)(*flat), (ctypes.c_int32 * 2)(len0, 0), STFT | (16 << 16))
        assert rc == -5 and "bases_len[0]" in lib.mifft_last_error().decode(), len0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    for kw in (dict(), dict(mode=1, c=0, s0=0), dict(D=1), dict(D=6), dict(batch=0), dict(Lo=993), dict(Lo=1024, T=2000),
               dict(s0=-63, c=63, S=1, F=1000), dict(s0=7), dict(T=993),
               dict(T=37, c=27, S=37, s0=-27, F=1, Lo=37),                       # K near T: one partial block
               dict(T=37, c=27, S=37, s0=0, F=1, Lo=10),
               dict(n=16, T=100, c=4, S=12, s0=-4, F=9, Lo=100),
               dict(n=16384, T=70000, c=4096, S=12288, s0=-4096, F=6, Lo=70000),
               dict(n=12288, T=40000, c=2999, S=9289, s0=-2999, F=5, Lo=40000, in_dtype=1, out_dtype=1, addr=0x10010),
               dict(n=1000, T=5000, c=299, S=701, s0=-299, F=8, Lo=5000), dict(radices=(2,)), dict(addr=(1 << 40) + 8),
               dict(T=1 << 30, n=16384, c=4096, S=12288, s0=0, F=87382, Lo=87382 * 12288, batch=3)):
        rc, why = _create12(**kw)
        assert rc == -10, (kw, rc, why)


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_fftconv_long_host import _create12\n"
            "print(*_create12())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_plan_fftconv_taps_validates_before_device_work():
    f32 = torch.float32
    for args, kw, status in (((f32, 2, 3, 1000, 64), dict(taps=0), -2),
                             ((f32, 2, 3, 1000, 64), dict(taps=64), -2),                     # K <= n - 1
                             ((f32, 2, 3, 1, 64), dict(taps=33), UNSUPPORTED),
                             ((f32, 2, 3, (1 << 30) + 1, 64), dict(taps=33), UNSUPPORTED),
                             ((f32, 2, 3, 1000, 74), dict(taps=33), UNSUPPORTED),
                             ((torch.float64, 2, 3, 1000, 16384), dict(taps=33), UNSUPPORTED),
                             ((torch.float16, 2, 3, 1000, 64), dict(taps=33), -4),
                             ((f32, 0, 3, 1000, 64), dict(taps=33), -8),
                             ((f32, 2, 3, 1000, 64), dict(taps=33, offset=-1), -5),
                             ((f32, 2, 3, 1000, 64), dict(taps=33, out_length=0), -5),
                             ((f32, 2, 3, 1000, 64), dict(taps=33, offset=1, out_length=1032), -5),     # beyond L + K - 1
                             ((f32, 2, 3, 1000, 64), dict(taps=33, offset=1, correlate=True), -5),      # beyond L
                             ((f32, 2, 3, 1000, 64), dict(taps=33, out_length=1001, correlate=True), -5)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
    # taps=None is the single-block plan with its refusals
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv(f32, 2, 3, 1000, 64)
    assert e.value.status == UNSUPPORTED
    if not torch.cuda.is_available():
        for kw in (dict(taps=33), dict(taps=33, out_length=1032), dict(taps=63), dict(taps=1, correlate=True)):
            with pytest.raises(mf.MifftError) as e:
                mf.plan_fftconv(f32, 2, 3, 1000, 64, **kw)
            assert e.value.status == -10, kw


def test_fftconv_block_argument_validates_on_the_host():
    x, k = torch.zeros(2, 3, 600), torch.zeros(3, 33)  # (host tensors: nothing reaches the library)
    with pytest.raises(ValueError):
        mf.fftconv(x, k, n=1024, block=64)
    for kw, status in ((dict(block=32), -2),            # K <= block - 1
                       (dict(block=33), -2),
                       (dict(block=74), UNSUPPORTED),
                       (dict(block=63), UNSUPPORTED),
                       (dict(block=32768), UNSUPPORTED),
                       (dict(n=64), UNSUPPORTED)):      # an explicit n keeps its refusal of L > n
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv(x, k, **kw)
        assert e.value.status == status, (kw, e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(x.double(), k, block=16384)
    assert e.value.status == UNSUPPORTED
    long_x = torch.zeros(3, 20000)
    for args, kw in (((x, k), dict(block=64)), ((x, k), dict(block=64, mode="full")), ((x, k), dict(block=64, correlate=True)),
                     ((x, k), dict(block=1000)), ((long_x, k), {}), ((long_x, k), dict(mode="valid")),
                     ((long_x, torch.zeros(3, 8193)), {})):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.fftconv(*args, **kw)
        assert e.value.status == -10, kw
    with pytest.raises(mf.MifftError) as e:  # no block holds two such filters
        mf.fftconv(long_x, torch.zeros(3, 8194))
    assert e.value.status == UNSUPPORTED and "partitioned" in str(e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv_length(16385)
    assert e.value.status == UNSUPPORTED and "out of scope" not in str(e.value)
