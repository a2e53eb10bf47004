"""The MDCT (MIFFT_MDCT_TAG in the window payload of a MIFFT_FLAG_STFT plan): the ABI constants, every refusal that needs no
device, the framing arithmetic and the fold / unfold tables against the direct sums, and the wrappers' host validation."""
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
from test_dct4_host import dct4_matrix

STFT, REFLECT, ZEROS, POWER = 32, 64, 128, 0x8000
UNSUPPORTED = -15
TAG_LO, TAG_HI = 0x43544401, 0x7FF84D44


# ---- references (fp64) ---------------------------------------------------------------------------------------------------------
def ref_mdct(x, n, window=None, norm=None):
    """the definition over zero-padded frames: x (B, T) -> (B, F, n); frame f covers the samples [(f - 1) n, (f + 1) n)"""
    x = np.asarray(x, dtype=np.float64)
    B, T = x.shape
    F = (T + n - 1) // n + 1
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n)) if window is None else np.asarray(window, dtype=np.float64)
    xp = np.zeros((B, (F + 1) * n))
    xp[:, n:n + T] = x
    j, k = np.arange(2 * n), np.arange(n)
    C = np.cos(np.pi / n * np.outer(j + 0.5 + n / 2, k + 0.5))
    frames = np.stack([xp[:, f * n:f * n + 2 * n] for f in range(F)], axis=1) * w
    X = frames @ C
    return X * np.sqrt(2.0 / n) if norm == "ortho" else X


def test_frames_and_window():
    for T, n, F in ((100, 8, 14), (96, 8, 13), (5, 8, 2), (4096, 256, 17), (5000, 1024, 6), (333, 30, 13)):
        assert mf.mdct_frames(T, n) == F == -(-T // n) + 1
    for bad in ((0, 8), (8, 0)):
        with pytest.raises(mf.MifftError):
            mf.mdct_frames(*bad)
    for n in (8, 30, 256):
        w = mf.mdct_window(n)
        assert w.dtype == torch.float64 and tuple(w.shape) == (2 * n,)
        assert np.abs(w.numpy() - np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n))).max() < 1e-15
        assert np.abs(w.numpy()[:n] ** 2 + w.numpy()[n:] ** 2 - 1).max() < 1e-15  # Princen-Bradley


@pytest.mark.parametrize("n", [4, 6, 16, 30, 200])
def test_fold_and_unfold_tables_against_the_direct_sums(n):
    """DCT-IV(fold(y)) / 2 is the MDCT of y, and unfold(DCT-IV(X) / 2) its transpose: with the sine window on both sides and
    the factor 2 / n the overlap-added frames reproduce the signal (TDAC)"""
    rng = np.random.default_rng(n)
    ia, sa, ib, sb = (t.numpy() for t in mf.api._mdct_fold_tables(n))
    y = rng.standard_normal((3, 2 * n))
    u = sa * y[:, ia] + sb * y[:, ib]
    j, k = np.arange(2 * n), np.arange(n)
    C = np.cos(np.pi / n * np.outer(j + 0.5 + n / 2, k + 0.5))
    assert np.abs(u @ dct4_matrix(n) / 2 - y @ C).max() < 1e-12 * n
    idx, sign = (t.numpy() for t in mf.api._mdct_unfold_tables(n))
    X = rng.standard_normal((3, n))
    v = X @ dct4_matrix(n) / 2
    assert np.abs(sign * v[:, idx] - X @ C.T).max() < 1e-12 * n
    T = 4 * n + 3
    x = rng.standard_normal((1, T))
    w = mf.mdct_window(n).numpy()
    Xf = ref_mdct(x, n)
    F = Xf.shape[1]
    yf = (2.0 / n) * w * (Xf @ C.T)
    acc = np.zeros((F + 1) * n)
    for f in range(F):
        acc[f * n:f * n + 2 * n] += yf[0, f]
    assert np.abs(acc[n:n + T] - x[0]).max() < 1e-12


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_the_tag_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    lo = re.search(r"#define\s+MIFFT_MDCT_TAG_LO\s+0x([0-9A-Fa-f]+)u\b", h)
    hi = re.search(r"#define\s+MIFFT_MDCT_TAG_HI\s+0x([0-9A-Fa-f]+)u\b", h)
    assert lo and hi and int(lo.group(1), 16) == TAG_LO and int(hi.group(1), 16) == TAG_HI
    assert np.isnan(struct.unpack("<d", struct.pack("<II", TAG_LO, TAG_HI))[0])
    assert (TAG_LO, TAG_HI) != (mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI)
    assert "MIFFT_MDCT_TAG_LO" in open(os.path.join(ROOT, "include", "mifft.hpp")).read()
    assert (mf.MDCT_TAG_LO, mf.MDCT_TAG_HI) == (mf.api.MDCT_TAG_LO, mf.api.MDCT_TAG_HI) == (TAG_LO, TAG_HI)
    assert len(_lib.EXPORTS) == 21  # (no new entry point)


def _words(values):
    return [w for v in values for w in struct.unpack("<II", struct.pack("<d", float(v)))]


def _create(T, M, *, hop=None, center=ZEROS, extra=0, scale=1.0, window=None, radices=(), tag=(TAG_LO, TAG_HI), in_dtype=0,
            out_dtype=0, inverse=0, comps=1, len0=None):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * 2)(T, 2 * M)
    flat = _words([0.5] * (2 * M) if window is None else window) + list(tag) + _words([scale])
    lens = (ctypes.c_int32 * 2)(len(flat) if len0 is None else len0, len(radices))
    flat = flat + list(radices)
    flags = STFT | center | ((M if hop is None else hop) << 16) | extra
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, 2, c_dims, 3, comps, inverse,
                             (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


def test_c_abi_refuses_before_looking_for_a_device():
    nan, inf = float("nan"), float("inf")
    for kw, status, word in (
            (dict(hop=8), UNSUPPORTED, "hop"),
            (dict(hop=32), UNSUPPORTED, "hop"),
            (dict(center=REFLECT), UNSUPPORTED, "MIFFT_FLAG_STFT_CENTER_REFLECT"),
            (dict(center=0), UNSUPPORTED, "centre bit"),
            (dict(extra=POWER), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (dict(extra=8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(inverse=1), UNSUPPORTED, "inverse"),
            (dict(M=6), UNSUPPORTED, "M = 6"),                        # below 8
            (dict(M=9), UNSUPPORTED, "M = 9"),                        # odd
            (dict(M=74), UNSUPPORTED, "packed"),                      # M / 2 = 37
            (dict(M=32768), UNSUPPORTED, "M = 32768"),
            (dict(M=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288 points (a 96-KiB tile)
            (dict(scale=inf), -5, "scale"),
            (dict(scale=nan), -5, "scale"),
            (dict(scale=0.0), -5, "scale"),
            (dict(window=[1.0] * 7 + [inf] + [1.0] * 24), -5, "window value 7"),
            (dict(window=[nan] + [1.0] * 31), -5, "window value 0"),
            (dict(in_dtype=2), -4, "in_dtype"),
            (dict(in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(comps=2), -3, "in_components"),
            (dict(radices=(3,)), -5, "length: 8"),                    # the radices factor M / 2
            # no tag behind the window, or another length: the STFT's own refusal, naming bases_len[0]
            (dict(tag=tuple(_words([nan]))), -5, "bases_len[0]"),
            (dict(tag=(mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI)), -5, "bases_len[0]"),
            (dict(len0=4 * 16 + 2), -5, "bases_len[0]"),
    ):
        kw = dict(kw)
        rc, why = _create(1000, kw.pop("M", 16), **kw)
        assert rc == status and word in why, (kw, rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    for T, M, kw in ((1000, 16, {}), (100, 8, {}), (5, 8, {}), (333, 30, {}), (40000, 8192, {}), (100000, 16384, {}),
                     (40000, 8192, dict(in_dtype=1, out_dtype=1)), (1000, 16, dict(radices=(2,))),
                     (1000, 16, dict(scale=-0.25)), (1000, 256, dict(radices=(16, 8)))):
        rc, why = _create(T, M, **kw)
        assert rc == -10, (T, M, kw, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_untagged_stft_payloads_are_what_they_were():
    L = _lib.lib()
    n = 64
    for flat, len0, want in (([], 0, -10), (_words([0.5] * n), 2 * n, -10)):
        h = ctypes.c_void_p()
        rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, (ctypes.c_int64 * 2)(1000, n), 3, 1, 0,
                                 (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * 2)(len0, 0), STFT | (16 << 16))
        assert rc == want, L.mifft_last_error().decode()


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_mdct_host import _create\n"
            "print(*_create(1000, 16))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_wrappers_validate_on_the_host():
    x = torch.zeros(3, 100)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(n=6), UNSUPPORTED), (dict(n=9), UNSUPPORTED), (dict(n=8, norm="forward"), UNSUPPORTED),
                       (dict(n=8, window=torch.ones(15)), -5), (dict(n=8, out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            mf.mdct(x, **kw)
        assert e.value.status == status, kw
    with pytest.raises(mf.MifftError) as e:
        mf.mdct(torch.zeros(3, 100, dtype=torch.complex64), 8)
    assert e.value.status == -3
    for ok in (dict(n=8), dict(n=8, norm="ortho"), dict(n=16, window=torch.ones(32)), dict(n=30, window=[0.5] * 60)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.mdct(x, **ok)
        assert e.value.status == -10, ok
    X = torch.zeros(3, 14, 8)
    for kw, status in ((dict(norm="forward"), UNSUPPORTED), (dict(window=torch.ones(15)), -5), (dict(length=0), -2),
                       (dict(length=14 * 8), -2)):
        with pytest.raises(mf.MifftError) as e:
            mf.imdct(X, **kw)
        assert e.value.status == status, kw
    for bad, status in ((torch.zeros(3, 14, 6), UNSUPPORTED), (torch.zeros(8), -1), (torch.zeros(1, 8), -2),
                        (torch.zeros(3, 14, 8, dtype=torch.complex64), -3)):
        with pytest.raises(mf.MifftError) as e:
            mf.imdct(bad)
        assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # valid: its DCT-IV fails only for want of a device tensor
        mf.imdct(X)
    assert e.value.status == -10


def test_plan_mdct_validates_before_device_work():
    for args, kw, status in (((torch.float16, 3, 100, 8), {}, -4), ((torch.float32, 3, 100, 6), {}, UNSUPPORTED),
                             ((torch.float32, 3, 100, 9), {}, UNSUPPORTED), ((torch.float32, 3, 1, 8), {}, -2),
                             ((torch.float32, 3, 100, 8), dict(norm="forward"), UNSUPPORTED),
                             ((torch.float32, 3, 100, 8), dict(window=torch.ones(8)), -5)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_mdct(*args, **kw)
        assert e.value.status == status, (args, kw)
    with pytest.raises(mf.MifftError) as e:  # the layouts of a Plan are checked against mdct_frames
        mf.Plan(torch.float32, torch.float32, (3, 100, 1), (3, 13, 8, 1), mdct=8)
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:  # the library's refusal: 74 / 2 = 37 is a prime above 32
        mf.Plan(torch.float32, torch.float32, (3, 100, 1), (3, 3, 74, 1), mdct=74)
    assert e.value.status == UNSUPPORTED and "packed" in str(e.value)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(norm="ortho"), dict(window=torch.hann_window(16, dtype=torch.float64))):
            with pytest.raises(mf.MifftError) as e:
                mf.plan_mdct(torch.float32, 3, 100, 8, **kw)
            assert e.value.status == -10, kw
