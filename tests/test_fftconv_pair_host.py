"""The convolution / correlation of two signal batches (MIFFT_CONV_PAIR_TAG in front of the 16-word payload of a
MIFFT_FLAG_STFT plan): the fp64 model and the mode table against numpy (and scipy where it imports), the four adjoint formulas
by dot-product identities, the ABI constants, the payload words, every refusal that needs no device, and the wrappers' host
validation."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT

try:
    import scipy.signal as _sig
except Exception:  # (numpy alone then: the test is never skipped)
    _sig = None

STFT, REFLECT, ZEROS, POWER, ISTFT = 32, 64, 128, 0x8000, 0x4000
UNSUPPORTED = -15
TAG_LO, TAG_HI = 0x49415001, 0x7FF84D50
MODES = ("causal", "full", "same", "valid")
LENGTH_PAIRS = [(37, 28), (28, 37), (40, 40), (9, 6), (8, 5), (33, 1), (16, 16)]


# ---- the model (fp64), as the issue's appendix states it -----------------------------------------------------------------------
def ref_pair(x, v, n, ea, eb, o, Lo, corr):
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    L, K = x.shape[-1], v.shape[-1]
    assert ea + L <= n and eb + K <= n and o + Lo <= n
    xe = np.zeros(x.shape[:-1] + (n,))
    xe[..., ea:ea + L] = x
    ve = np.zeros(v.shape[:-1] + (n,))
    ve[..., eb:eb + K] = v
    A, B = np.fft.rfft(xe), np.fft.rfft(ve)
    return np.fft.irfft(A * (np.conj(B) if corr else B), n)[..., o:o + Lo]


def window_of(mode, L, K, corr):
    """(ea, eb, o, Lo) of a mode: the wrapper's own arithmetic, pinned against numpy / scipy below"""
    return mf.api._fftconv_pair_window(mode, L, K, corr)


def adjoints_of(L, K, ea, eb, o, Lo, corr):
    return mf.api._fftconv_pair_adjoints(L, K, ea, eb, o, Lo, corr)


@pytest.mark.parametrize("L,K", LENGTH_PAIRS)
def test_the_model_and_the_mode_table_against_numpy_and_scipy(L, K):
    rng = np.random.default_rng(L * 100 + K)
    x, v = rng.standard_normal((3, L)), rng.standard_normal((3, K))
    n = mf.fftconv_length(L + K - 1)
    for corr in (False, True):
        for r in range(3):
            full = np.correlate(x[r], v[r], "full") if corr else np.convolve(x[r], v[r])
            scale = np.abs(full).max()
            for mode in MODES:
                ea, eb, o, Lo = window_of(mode, L, K, corr)
                got = ref_pair(x[r], v[r], n, ea, eb, o, Lo, corr)
                if mode == "causal":  # (both rows at 0: the first L samples of the product; lags 0 .. L - 1 of a correlation)
                    assert (ea, eb, o, Lo) == (0, 0, 0, L)
                    xp = np.concatenate([x[r], np.zeros(K)])
                    want = np.array([np.dot(v[r], xp[t:t + K]) for t in range(L)]) if corr else full[:L]
                else:
                    crop = {"full": (0, L + K - 1), "same": ((K - 1) // 2, L), "valid": (min(L, K) - 1, abs(L - K) + 1)}[mode]
                    assert (o, Lo) == crop and (ea, eb) == ((K - 1 if corr else 0), 0)
                    want = full[crop[0]:crop[0] + crop[1]]
                    if _sig is not None:
                        direct = (_sig.correlate if corr else _sig.convolve)(x[r], v[r], mode=mode, method="direct")
                        assert direct.shape == want.shape and np.abs(direct - want).max() <= 1e-12 * scale, (mode, corr)
                assert got.shape == want.shape, (mode, corr, got.shape, want.shape)
                assert np.abs(got - want).max() <= 1e-12 * scale, (mode, corr, r)


def test_the_circular_model_wraps():
    rng = np.random.default_rng(3)
    x, v = rng.standard_normal(16), rng.standard_normal(9)
    full = np.convolve(x, v)
    want = full[:16].copy()
    want[:8] += full[16:]
    assert np.abs(ref_pair(x, v, 16, 0, 0, 0, 16, False) - want).max() <= 1e-12 * np.abs(full).max()


@pytest.mark.parametrize("n,L,K", [(16, 8, 5), (64, 37, 28), (64, 28, 37), (14, 9, 6), (64, 40, 40)])
def test_the_four_adjoints_by_dot_products(n, L, K):
    """<gy, pair(x, v)> = <gx, x> = <gv, v> with the gradients the formulas name, over random ea, eb, o, Lo -- n < L + K - 1
    (the circular case) included: (64, 40, 40) and (14, 9, 6)"""
    rng = np.random.default_rng(n * 1000 + L * 10 + K)
    worst = 0.0
    for trial in range(40):
        ea, eb = int(rng.integers(0, n - L + 1)), int(rng.integers(0, n - K + 1))
        o = int(rng.integers(0, n))
        Lo = int(rng.integers(1, n - o + 1))
        corr = bool(trial & 1)
        x, v, gy = rng.standard_normal((2, L)), rng.standard_normal((2, K)), rng.standard_normal((2, Lo))
        y = ref_pair(x, v, n, ea, eb, o, Lo, corr)
        lhs = float((gy * y).sum())
        for spec, other, wrt in zip(adjoints_of(L, K, ea, eb, o, Lo, corr), (v, x), (x, v)):
            first, La, Lb, a_ea, a_eb, a_o, a_Lo, a_corr = spec
            a, b = (gy, other) if first == "gy" else (other, gy)
            assert (a.shape[-1], b.shape[-1], a_Lo) == (La, Lb, wrt.shape[-1])
            g = ref_pair(a, b, n, a_ea, a_eb, a_o, a_Lo, a_corr)
            rhs = float((g * wrt).sum())
            worst = max(worst, abs(lhs - rhs) / max(1.0, abs(lhs)))
    assert worst <= 1e-12, worst
    # the formulas themselves, written out once
    assert adjoints_of(37, 28, 1, 2, 3, 4, False) == (("gy", 4, 28, 3, 2, 1, 37, True), ("gy", 4, 37, 3, 1, 2, 28, True))
    assert adjoints_of(37, 28, 1, 2, 3, 4, True) == (("gy", 4, 28, 3, 2, 1, 37, False), ("x", 37, 4, 1, 3, 2, 28, True))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _create(L=37, n=64, *, batch=6, K=28, ea=0, eb=0, o=0, Lo=37, mode=0, rest=(0,) * 8, flags=STFT, radices=(),
            tag=(TAG_LO, TAG_HI), in_dtype=0, out_dtype=0, inverse=0, comps=1, len0=None, device=0):
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = list(tag) + [K, ea, eb, o, Lo, mode] + list(rest)
    lens = (ctypes.c_int32 * 2)(len(flat) if len0 is None else len0, len(radices))
    flat = flat + list(radices)
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(L, n), batch, comps, inverse,
                               (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


def test_the_tag_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    lo = re.search(r"#define\s+MIFFT_CONV_PAIR_TAG_LO\s+0x([0-9A-Fa-f]+)u\b", h)
    hi = re.search(r"#define\s+MIFFT_CONV_PAIR_TAG_HI\s+0x([0-9A-Fa-f]+)u\b", h)
    magic = re.search(r"#define\s+MIFFT_CONV_PAIR_ARGS_MAGIC\s+0x([0-9A-Fa-f]+)ull\b", h)
    assert lo and hi and int(lo.group(1), 16) == TAG_LO and int(hi.group(1), 16) == TAG_HI
    assert np.isnan(struct.unpack("<d", struct.pack("<II", TAG_LO, TAG_HI))[0])  # (no window value: those are finite)
    others = ((mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI), (mf.MDCT_TAG_LO, mf.MDCT_TAG_HI), (mf.CONV_TAG_LO, mf.CONV_TAG_HI),
              (mf.CONV_GRAD_TAG_LO, mf.CONV_GRAD_TAG_HI), (mf.STFT_ADJ_TAG_LO, mf.STFT_ADJ_TAG_HI),
              (mf.ISTFT_ADJ_TAG_LO, mf.ISTFT_ADJ_TAG_HI))
    assert all(TAG_HI != t[1] and TAG_LO != t[0] for t in others)
    assert "MIFFT_CONV_PAIR_TAG_LO" in open(os.path.join(ROOT, "include", "mifft.hpp")).read()
    assert (mf.CONV_PAIR_TAG_LO, mf.CONV_PAIR_TAG_HI) == (mf.api.CONV_PAIR_TAG_LO, mf.api.CONV_PAIR_TAG_HI) == (TAG_LO, TAG_HI)
    assert magic and int(magic.group(1), 16) == mf.CONV_PAIR_ARGS_MAGIC == struct.unpack("<Q", b"MIFFTPA1")[0]
    assert ctypes.sizeof(mf.ConvPairArgs) == 8 + 2 * ctypes.sizeof(ctypes.c_void_p)
    assert len(_lib.EXPORTS) == 21  # (no new entry point)


_PAYLOADS = (
    (dict(n=64, K=28, ea=0, eb=0, o=0, Lo=64), [TAG_LO, TAG_HI, 28, 0, 0, 0, 64, 0] + [0] * 8),
    (dict(n=64, K=28, ea=27, eb=0, o=13, Lo=37, mode=1), [TAG_LO, TAG_HI, 28, 27, 0, 13, 37, 1] + [0] * 8),
    (dict(n=16384, K=8192, ea=3, eb=5, o=16383, Lo=1), [TAG_LO, TAG_HI, 8192, 3, 5, 16383, 1, 0] + [0] * 8),
)


@pytest.mark.parametrize("fields,words", _PAYLOADS, ids=["convolve", "correlate", "long"])
def test_the_payload_words(fields, words):
    req = mf.api.ConvPairRequest(**fields)
    assert mf.api._conv_pair_payload(req) == words and len(words) == 16
    assert mf.api._frame_payload(req) == (STFT, words, 1)
    lib, h = _lib.lib(), ctypes.c_void_p()
    rc = lib.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(37, req.n), 6, 1, 0,
                               (ctypes.c_uint32 * 16)(*words), (ctypes.c_int32 * 2)(16, 0), STFT)
    assert rc == -10, lib.mifft_last_error().decode()  # (every check passed: it stops for want of a device)
    for bad in (dict(K=1 << 32), dict(ea=-1), dict(o=1 << 32), dict(mode=-1)):
        with pytest.raises(mf.MifftError) as e:
            mf.api._conv_pair_payload(req._replace(**bad))
        assert e.value.status == -5, bad


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            (dict(n=6, L=4, K=2, Lo=4), UNSUPPORTED, "8 to 16384"),           # below 8
            (dict(n=74), UNSUPPORTED, "packed"),                              # 74 / 2 = 37, a prime above 32
            (dict(n=63), UNSUPPORTED, "even"),                                # odd
            (dict(n=16386), UNSUPPORTED, "16384"),
            (dict(n=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288
            (dict(L=65), -5, "ea + L"),
            (dict(ea=28), -5, "ea + L"),
            (dict(K=65), -5, "eb + K"),
            (dict(eb=37), -5, "eb + K"),
            (dict(K=0), -5, "K >= 1"),
            (dict(Lo=0), -5, "Lo >= 1"),
            (dict(o=30, Lo=35), -5, "o + Lo"),
            (dict(o=64, Lo=1), -5, "o + Lo"),
            (dict(mode=2), -5, "mode"),
            (dict(mode=1 | (8 << 8)), -5, "mode"),                            # no 16-bit storage
            (dict(mode=1 << 16), -5, "mode"),
            (dict(rest=(1,) + (0,) * 7), -5, "reserved word 8"),
            (dict(rest=(0,) * 7 + (5,)), -5, "reserved word 15"),
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


def test_a_valid_request_gets_as_far_as_the_device():
    """(device -1 is no device on any machine: nothing is compiled or uploaded even where one exists)"""
    for kw in (dict(), dict(L=64, Lo=64), dict(K=64, eb=0), dict(ea=27, eb=36), dict(o=27, Lo=37), dict(o=63, Lo=1), dict(mode=1),
               dict(batch=0), dict(batch=1), dict(K=1), dict(n=16, L=8, K=9, Lo=16), dict(n=16384, L=8192, K=8192, Lo=16383),
               dict(n=12288, L=6000, K=6289, Lo=12288, in_dtype=1, out_dtype=1), dict(n=1000, L=600, K=401, Lo=1000),
               dict(radices=(2,)), dict(radices=(4, 8))):
        rc, why = _create(device=-1, **kw)
        assert rc == -10, (kw, rc, why)


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_fftconv_pair_host import _create\n"
            "print(*_create(device=-1))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


def test_other_payloads_keep_their_meaning_and_refusals():
    lib = _lib.lib()

    def create(L, n, flat, len0, flags, batch=6):
        h = ctypes.c_void_p()
        rc = lib.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(L, n), batch, 1, 0,
                                   (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * 2)(len0, 0), flags)
        return rc, lib.mifft_last_error().decode()

    # the tag anywhere but in front of exactly 16 words, or with another upper half, is no two-signal plan: the STFT's own
    # refusals, naming bases_len[0] or the hop
    rc, why = _create(L=1000, tag=(TAG_LO, TAG_HI + 1), flags=STFT | (16 << 16), device=-1)
    assert rc == -5 and "bases_len[0]" in why, why
    rc, why = _create(L=1000, len0=15, flags=STFT | (16 << 16), device=-1)
    assert rc == -5 and "bases_len[0]" in why, why
    rc, why = _create(len0=15, device=-1)
    assert rc == UNSUPPORTED and "hop 0" in why, why
    # without MIFFT_FLAG_STFT the words are radices, and refused as such
    rc, why = _create(flags=0, device=-1)
    assert rc != 0 and rc != -10, why
    # the convolution, gated convolution and filter-gradient payloads of 8 and 16 words pass their own checks as ever
    conv = [mf.CONV_TAG_LO, mf.CONV_TAG_HI, 3, 5, 40, 1, 0x12345600, 0x7F00]
    assert create(40, 64, conv, 8, STFT)[0] == -10
    assert create(40, 64, conv[:5] + [0] + conv[6:] + [0, 0, 0, 3, 0, 0, 0, 0], 16, STFT)[0] == -10
    grad = [mf.CONV_GRAD_TAG_LO, mf.CONV_GRAD_TAG_HI, 3, 5, 40, 0, 1, 0, 40, 0, 0, 0, 0, 0, 0, 0]
    assert create(40, 64, grad, 16, STFT)[0] == -10
    rc, why = create(40, 64, conv[:5] + [2] + conv[6:], 8, STFT)
    assert rc == -5 and "mode" in why and "convolution payload" in why and "two-signal" not in why, why
    rc, why = create(40, 64, grad[:12] + [7, 0, 0, 0], 16, STFT)
    assert rc == -5 and "filter-gradient" in why, why
    # untagged STFT payloads: none, and a window of n values
    n = 64
    words = [w for v in [0.5] * n for w in struct.unpack("<II", struct.pack("<d", v))]
    for flat, len0 in (([], 0), (words, 2 * n)):
        assert create(1000, n, flat, len0, STFT | (16 << 16), batch=3)[0] == -10


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_wrappers_validate_on_the_host():
    x, v = torch.zeros(2, 3, 40), torch.zeros(2, 3, 9)  # (host tensors: nothing reaches the library)
    with pytest.raises(ValueError):
        mf.fftconv_pair(x, v, mode="circular")
    for args, kw, status, word in (
            ((x, torch.zeros(3, 9)), {}, -2, "fftconv"),                    # a shared filter: mismatched leading shapes
            ((x, torch.zeros(2, 4, 9)), {}, -2, "broadcast"),
            ((x, torch.zeros(1, 3, 9)), {}, -2, "broadcast"),
            ((x.to(torch.complex64), v), {}, -3, "real"),
            ((x, v.to(torch.complex64)), {}, -3, "real"),
            ((x, v), dict(n=40), -2, "causal"),                             # a smaller n with the default mode, "full"
            ((x, v), dict(n=40, mode="same"), -2, "causal"),
            ((x, v), dict(n=40, mode="valid"), -2, "causal"),
            ((x, v), dict(n=32, mode="causal"), -2, "max(L, K)"),
            ((x, v), dict(n=74), UNSUPPORTED, "FFT length"),
            ((torch.zeros(2, 9000), torch.zeros(2, 8000)), {}, UNSUPPORTED, "fftconv(block=)"),   # rows that are too long
            ((torch.zeros(2, 7000, dtype=torch.float64), torch.zeros(2, 6000, dtype=torch.float64)), {}, UNSUPPORTED,
             "fftconv(block=)"),
            ((torch.zeros(2, 1), torch.zeros(2, 5)), {}, -2, "at least 2")):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv_pair(*args, **kw)
        assert e.value.status == status and word in str(e.value), (kw, e.value)
    for ok in (dict(), dict(mode="same"), dict(mode="valid"), dict(mode="causal"), dict(correlate=True),
               dict(mode="same", correlate=True), dict(n=40, mode="causal"), dict(n=64)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.fftconv_pair(x, v, **ok)
        assert e.value.status == -10, ok


def test_plan_fftconv_pair_validates_before_device_work():
    for args, kw, status in (((torch.float16, 2, 40, 9, 64), {}, -4),
                             ((torch.float32, 2, 40, 9, 74), {}, UNSUPPORTED),
                             ((torch.float64, 2, 40, 9, 16384), {}, UNSUPPORTED),
                             ((torch.float32, 0, 40, 9, 64), {}, -8),
                             ((torch.float32, 2, 1, 9, 64), {}, -2),
                             ((torch.float32, 2, 40, 0, 64), {}, -2),
                             ((torch.float32, 2, 65, 9, 64), {}, -5),
                             ((torch.float32, 2, 40, 9, 64), dict(x_offset=25), -5),
                             ((torch.float32, 2, 40, 9, 64), dict(v_offset=56), -5),
                             ((torch.float32, 2, 40, 9, 64), dict(v_offset=-1), -5),
                             ((torch.float32, 2, 40, 9, 64), dict(out_length=0), -5),
                             ((torch.float32, 2, 40, 9, 64), dict(offset=30, out_length=35), -5)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv_pair(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
    if not torch.cuda.is_available():
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv_pair(torch.float32, 2, 40, 9, 64, x_offset=8, v_offset=55, offset=63, out_length=1, correlate=True)
        assert e.value.status == -10
