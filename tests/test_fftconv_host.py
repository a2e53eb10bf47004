"""The fused FFT convolution (MIFFT_CONV_TAG in front of the payload of a MIFFT_FLAG_STFT plan): the fp64 reference against
numpy.convolve and scipy.signal.fftconvolve, fftconv_length against a brute-force search, the ABI constants, every refusal
that needs no device, and the wrappers' host validation."""
import ctypes
import os
import re
import struct
import subprocess
import sys

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


# ---- the reference (fp64) ------------------------------------------------------------------------------------------------------
def ref_fftconv(x, k, n, o=0, Lo=None, correlate=False):
    """rows x (R, L) against filters k (D, K) or (K,), row r with filter r % D:
    irfft(rfft(x[r], n) * G[r % D], n)[o : o + Lo], G = rfft(k, n) or its conjugate; Lo defaults to L"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    k = np.atleast_2d(np.asarray(k, dtype=np.float64))
    R, L = x.shape
    D = k.shape[0]
    Lo = L if Lo is None else Lo
    assert L <= n and k.shape[1] <= n and o + Lo <= n
    G = np.fft.rfft(k, n, axis=-1)
    if correlate:
        G = np.conj(G)
    y = np.fft.irfft(np.fft.rfft(x, n, axis=-1) * G[np.arange(R) % D], n, axis=-1)
    return y[:, o:o + Lo]


def window_of(mode, L, K):
    """(o, Lo) of a mode: the wrapper's own arithmetic, pinned against scipy below"""
    return mf.api._fftconv_window(mode, L, K)


@pytest.mark.parametrize("L,K", [(37, 28), (50, 40), (8, 5), (28, 37), (40, 40), (33, 1)])
def test_the_reference_against_numpy_and_scipy(L, K):
    rng = np.random.default_rng(L * 100 + K)
    D, B = 3, 2
    x, k = rng.standard_normal((B * D, L)), rng.standard_normal((D, K))
    n = mf.fftconv_length(L + K - 1)
    full = ref_fftconv(x, k, n, 0, L + K - 1)
    for r in range(B * D):
        want = np.convolve(x[r], k[r % D])
        assert np.abs(full[r] - want).max() <= 1e-12 * np.abs(want).max()
    for mode in MODES:
        o, Lo = window_of(mode, L, K)
        got = ref_fftconv(x, k, n, o, Lo)
        for r in range(B * D):
            if mode == "causal":
                want = np.convolve(x[r], k[r % D])[:L]
            else:
                want = scipy.signal.fftconvolve(x[r], k[r % D], mode=mode)
            assert got[r].shape == want.shape, (mode, got[r].shape, want.shape)
            assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max(), (mode, r)
    # correlation: y[t] = sum_j k[j] x[t + j], zeros beyond the row
    got = ref_fftconv(x, k, n, 0, L, correlate=True)
    xp = np.concatenate([x, np.zeros((B * D, K))], axis=1)
    for r in range(B * D):
        want = np.array([np.dot(k[r % D], xp[r, t:t + K]) for t in range(L)])
        assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max()


def test_the_circular_reference_wraps():
    rng = np.random.default_rng(3)
    x, k = rng.standard_normal((2, 16)), rng.standard_normal((1, 16))
    got = ref_fftconv(x, k, 16)
    for r in range(2):
        full = np.convolve(x[r], k[0])
        want = full[:16].copy()
        want[:15] += full[16:]
        assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full).max()


# ---- fftconv_length ------------------------------------------------------------------------------------------------------------
def _create(L=37, n=64, *, batch=6, D=3, o=0, Lo=37, mode=0, addr=0x10000, flags=STFT, radices=(), tag=(TAG_LO, TAG_HI),
            in_dtype=0, out_dtype=0, inverse=0, comps=1, len0=None, device=0):
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = list(tag) + [D, o, Lo, mode, addr & 0xFFFFFFFF, addr >> 32]
    lens = (ctypes.c_int32 * 2)(len(flat) if len0 is None else len0, len(radices))
    flat = flat + list(radices)
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(L, n), batch, comps, inverse,
                               (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


def _accepted(n, dt=0):
    """the library's host-side answer (device -1 is no device: nothing is compiled or uploaded even where one exists)"""
    rc, _ = _create(L=2, n=n, batch=1, D=1, Lo=1, in_dtype=dt, out_dtype=dt, device=-1)
    return rc == -10


def test_fftconv_length_is_minimal_and_accepted():
    sample = sorted(set(range(8, 140)) | set(range(16200, 16385)) | set(range(8, 16385, 97)) | {1024, 2049, 8191, 8193, 12289})
    for m in sample:
        n = mf.fftconv_length(m)
        assert n >= m and _accepted(n), (m, n)
        brute = next(c for c in range(m, 16385) if _accepted(c))
        assert n == brute, (m, n, brute)
    for m in (1, 5, 8):
        assert mf.fftconv_length(m) == 8
    for m in (16385, 20000):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv_length(m)
        assert e.value.status == UNSUPPORTED
    # float64 rows end at 12288 points and lack a few shorter lengths: the answer is the library's for that type
    for m in (430, 433, 5000, 12288):
        n = mf.fftconv_length(m, torch.float64)
        assert n == next(c for c in range(m, 16385) if _accepted(c, 1)), m
    assert mf.fftconv_length(433) == 434 and mf.fftconv_length(433, torch.float64) > 434
    with pytest.raises(mf.MifftError):
        mf.fftconv_length(12289, torch.float64)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_the_tag_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    lo = re.search(r"#define\s+MIFFT_CONV_TAG_LO\s+0x([0-9A-Fa-f]+)u\b", h)
    hi = re.search(r"#define\s+MIFFT_CONV_TAG_HI\s+0x([0-9A-Fa-f]+)u\b", h)
    assert lo and hi and int(lo.group(1), 16) == TAG_LO and int(hi.group(1), 16) == TAG_HI
    assert np.isnan(struct.unpack("<d", struct.pack("<II", TAG_LO, TAG_HI))[0])  # (no window value: those are finite)
    assert (TAG_LO, TAG_HI) not in ((mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI), (mf.MDCT_TAG_LO, mf.MDCT_TAG_HI))
    assert "MIFFT_CONV_TAG_LO" in open(os.path.join(ROOT, "include", "mifft.hpp")).read()
    assert (mf.CONV_TAG_LO, mf.CONV_TAG_HI) == (mf.api.CONV_TAG_LO, mf.api.CONV_TAG_HI) == (TAG_LO, TAG_HI)
    assert len(_lib.EXPORTS) == 21  # (no new entry point)


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            (dict(n=6, L=4, Lo=4), UNSUPPORTED, "8 to 16384"),               # below 8
            (dict(n=74), UNSUPPORTED, "packed"),                              # 74 / 2 = 37, a prime above 32
            (dict(n=63, L=37), UNSUPPORTED, "even"),                          # odd
            (dict(n=16386), UNSUPPORTED, "16384"),
            (dict(n=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288
            (dict(L=65), UNSUPPORTED, "L > n"),
            (dict(Lo=0), -5, "Lo"),
            (dict(o=30, Lo=35), -5, "o + Lo"),
            (dict(o=64, Lo=1), -5, "o + Lo"),
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
            (dict(radices=(3,)), -5, "length"),                               # the radices factor n
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw, rc, why)


def test_other_payloads_keep_their_meaning_and_refusals():
    # the tag anywhere but in front of exactly 8 words is no convolution: the STFT's own refusals, naming bases_len[0] or the hop
    rc, why = _create(L=1000, len0=8, tag=(TAG_LO, TAG_HI + 1), flags=STFT | (16 << 16))
    assert rc == -5 and "bases_len[0]" in why, why
    rc, why = _create(L=1000, tag=(TAG_LO, TAG_HI), len0=7, flags=STFT | (16 << 16))
    assert rc == -5 and "bases_len[0]" in why, why
    rc, why = _create(tag=(TAG_LO, TAG_HI), len0=7)  # (no hop: what a plain STFT plan without one has always been told)
    assert rc == UNSUPPORTED and "hop 0" in why, why
    # without MIFFT_FLAG_STFT the words are radices, and refused as such
    rc, why = _create(flags=0)
    assert rc != 0 and rc != -10, why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    for kw in (dict(), dict(L=64, Lo=64), dict(o=27, Lo=37), dict(o=63, Lo=1), dict(mode=1), dict(D=1), dict(D=6), dict(batch=0),
               dict(n=16, L=8, Lo=8), dict(n=16384, L=8192, Lo=8192), dict(n=12288, L=6000, Lo=6000, in_dtype=1, out_dtype=1, addr=0x10010),
               dict(n=1000, L=600, Lo=600), dict(radices=(2,)), dict(addr=(1 << 40) + 8)):
        rc, why = _create(**kw)
        assert rc == -10, (kw, rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_untagged_stft_payloads_are_what_they_were():
    lib = _lib.lib()
    n = 64
    words = [w for v in [0.5] * n for w in struct.unpack("<II", struct.pack("<d", v))]
    for flat, len0 in (([], 0), (words, 2 * n)):
        h = ctypes.c_void_p()
        rc = lib.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, (ctypes.c_int64 * 2)(1000, n), 3, 1, 0,
                                   (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * 2)(len0, 0), STFT | (16 << 16))
        assert rc == -10, lib.mifft_last_error().decode()


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_fftconv_host import _create\n"
            "print(*_create())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_modes_are_scipys_crops():
    for L, K in ((37, 28), (28, 37), (50, 40), (8, 8), (9, 1)):
        a, b = np.arange(L, dtype=np.float64) + 1, np.arange(K, dtype=np.float64) + 1
        full = np.convolve(a, b)
        for mode in ("full", "same", "valid"):
            o, Lo = window_of(mode, L, K)
            want = scipy.signal.fftconvolve(a, b, mode=mode)
            assert Lo == len(want) and np.abs(full[o:o + Lo] - want).max() < 1e-9, (L, K, mode)
        assert window_of("causal", L, K) == (0, L)


def test_wrappers_validate_on_the_host():
    x, k = torch.zeros(2, 3, 40), torch.zeros(3, 9)  # (host tensors: nothing reaches the library)
    with pytest.raises(ValueError):
        mf.fftconv(x, k, mode="circular")
    for mode in ("full", "same", "valid"):
        with pytest.raises(ValueError):
            mf.fftconv(x, k, mode=mode, correlate=True)
    for args, kw, status in (((x, torch.zeros(3, 65)), dict(n=64), -2),               # K > n
                             ((x, torch.zeros(4, 9)), {}, -2),                           # channels
                             ((x, torch.zeros(2, 3, 9)), {}, -1),
                             ((torch.zeros(40), k), {}, -1),
                             ((x.to(torch.complex64), k), {}, -3),
                             ((x, k), dict(n=74), UNSUPPORTED),                          # no accepted length
                             ((x, k), dict(n=32), UNSUPPORTED)):                         # L > n
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv(*args, **kw)
        assert e.value.status == status, (kw, e.value)
    for ok in (dict(), dict(mode="full"), dict(mode="same"), dict(mode="valid"), dict(correlate=True), dict(n=64)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.fftconv(x, k, **ok)
        assert e.value.status == -10, ok
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(torch.zeros(5, 40), torch.zeros(9))
    assert e.value.status == -10


def test_plan_fftconv_validates_before_device_work():
    for args, kw, status in (((torch.float16, 2, 3, 40, 64), {}, -4),
                             ((torch.float32, 2, 3, 40, 74), {}, UNSUPPORTED),
                             ((torch.float32, 2, 3, 40, 63), {}, UNSUPPORTED),
                             ((torch.float64, 2, 3, 40, 16384), {}, UNSUPPORTED),
                             ((torch.float64, 2, 3, 40, 434), {}, UNSUPPORTED),  # (one of the lengths only float64 lacks)
                             ((torch.float32, 2, 3, 65, 64), {}, UNSUPPORTED),
                             ((torch.float32, 0, 3, 40, 64), {}, -8),
                             ((torch.float32, 2, 0, 40, 64), {}, -8),
                             ((torch.float32, 2, 3, 40, 64), dict(out_length=0), -5),
                             ((torch.float32, 2, 3, 40, 64), dict(offset=30, out_length=35), -5),
                             ((torch.float32, 2, 3, 40, 64), dict(offset=-1), -5)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
    if not torch.cuda.is_available():
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv(torch.float32, 2, 3, 40, 64)
        assert e.value.status == -10


# ---- the payload encoder -------------------------------------------------------------------------------------------------------
GRAD_LO, GRAD_HI = 0x44524701, 0x7FF84D47
_ADDR = 0x7F0012345600  # (words 6 and 7: 0x12345600, 0x7F00)
_H = [0x12345600, 0x7F00]
# one request per payload form; T = 1000 samples, K = Q = 33 taps at n = 64: c = 32, S = 32, s0 = -32, F = 32, P = 31.
# The words are those the plan classes assembled for these arguments before the encoder existed, written out.
_PAYLOADS = (
    ("8 words", torch.float32, 40, dict(n=64, D=3, o=5, Lo=40, mode=1, address=_ADDR),
     [TAG_LO, TAG_HI, 3, 5, 40, 1] + _H),
    ("12 words", torch.float32, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-32, address=_ADDR),
     [TAG_LO, TAG_HI, 3, 32, 32, 0] + _H + [32, 4294967264, 1000, 0]),
    ("12 words, float64, 'same': s0 = -16", torch.float64, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-16, address=_ADDR),
     [TAG_LO, TAG_HI, 3, 32, 32, 0] + _H + [32, 4294967280, 1000, 0]),
    ("16 words, a single block", torch.float32, 40, dict(n=64, D=3, o=5, Lo=40, address=_ADDR, gates=3),
     [TAG_LO, TAG_HI, 3, 5, 40, 0] + _H + [0, 0, 0, 3, 0, 0, 0, 0]),
    ("16 words, overlap-save", torch.float32, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-32, address=_ADDR, gates=1),
     [TAG_LO, TAG_HI, 3, 32, 32, 0] + _H + [32, 4294967264, 1000, 1, 0, 0, 0, 0]),
    ("20 words", torch.float32, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-32, Q=33, P=31, address=_ADDR),
     [TAG_LO, TAG_HI, 3, 32, 32, 0] + _H + [32, 4294967264, 1000, 0, 0, 0, 0, 0, 33, 31, 0, 0]),
    ("20 words, gated", torch.float32, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-32, Q=33, P=31, address=_ADDR, gates=2),
     [TAG_LO, TAG_HI, 3, 32, 32, 0] + _H + [32, 4294967264, 1000, 2, 0, 0, 0, 0, 33, 31, 0, 0]),
    ("12 words, bfloat16 rows, correlation", torch.float32, 1000,
     dict(n=64, D=3, o=0, Lo=1000, S=32, F=32, s0=0, mode=1 | (8 << 8), address=_ADDR),
     [TAG_LO, TAG_HI, 3, 0, 32, 2049] + _H + [32, 0, 1000, 0]),
    ("gradient, a single block", torch.float32, 40, dict(n=64, D=3, o=5, Lo=40, grad=True),
     [GRAD_LO, GRAD_HI, 3, 5, 40, 0, 1, 0, 40, 0, 0, 0, 0, 0, 0, 0]),
    ("gradient, overlap-save, partials", torch.float32, 1000, dict(n=64, D=3, o=32, Lo=1000, S=32, F=32, s0=-32, grad=True, partials=7),
     [GRAD_LO, GRAD_HI, 3, 32, 32, 0, 32, 4294967264, 1000, 7, 0, 0, 0, 0, 0, 0]),
    ("gradient, float16 rows, correlation", torch.float32, 1000,
     dict(n=64, D=3, o=0, Lo=1000, S=32, F=32, s0=0, mode=1 | (7 << 8), grad=True),
     [GRAD_LO, GRAD_HI, 3, 0, 32, 1793, 32, 0, 1000, 0, 0, 0, 0, 0, 0, 0]),
)


@pytest.mark.parametrize("what,dtype,L,fields,words", _PAYLOADS, ids=[p[0] for p in _PAYLOADS])
def test_the_payload_words_of_every_form(what, dtype, L, fields, words):
    req = mf.api.ConvRequest(**fields)
    assert mf.api._conv_payload(req) == words
    # the library passes every check on them and stops for want of a device
    lib, h, code = _lib.lib(), ctypes.c_void_p(), mf.api._DTYPE_CODE[dtype]
    rc = lib.mifft_plan_create(ctypes.byref(h), -1, code, code, 2, (ctypes.c_int64 * 2)(L, req.n), 6, 1, 0,
                               (ctypes.c_uint32 * len(words))(*words), (ctypes.c_int32 * 2)(len(words), 0), STFT)
    assert rc == -10, lib.mifft_last_error().decode()


def test_the_requests_of_the_plan_arguments_and_what_fits_no_word():
    # the geometry of plan_fftconv's arguments lands in the fields the payloads above were written from
    assert (8, 7) == (mf.api._DTYPE_CODE[torch.bfloat16], mf.api._DTYPE_CODE[torch.float16])
    request = mf.api._fftconv_request
    assert request(64, 3, 5, 40, True, None, None, None) == mf.api.ConvRequest(64, 3, 5, 40, mode=1)
    assert request(64, 3, 0, 1000, False, 33, None, None) == mf.api.ConvRequest(64, 3, 32, 1000, S=32, F=32, s0=-32)
    assert request(64, 3, 16, 1000, False, 33, None, None) == mf.api.ConvRequest(64, 3, 32, 1000, S=32, F=32, s0=-16)
    assert request(64, 3, 0, 1000, False, 1000, 33, None) == mf.api.ConvRequest(64, 3, 32, 1000, S=32, F=32, s0=-32, Q=33, P=31)
    assert request(64, 3, 0, 1000, True, 33, None, torch.bfloat16) == mf.api.ConvRequest(64, 3, 0, 1000, S=32, F=32, mode=2049)
    for bad in (dict(D=1 << 32), dict(o=-1), dict(S=1 << 32, F=1), dict(S=32, s0=1 << 31), dict(S=32, s0=-(1 << 31) - 1), dict(gates=4),
                dict(S=32, Q=-1), dict(grad=True, partials=1 << 32)):
        with pytest.raises(mf.MifftError) as e:
            mf.api._conv_payload(mf.api.ConvRequest(**{**dict(n=64, D=3, o=0, Lo=40), **bad}))
        assert e.value.status == -5, bad
