"""The fused inverse MDCT (MIFFT_MDCT_TAG in the window payload of a MIFFT_FLAG_ISTFT plan): the fp64 reference straight from
the definition, every refusal that needs no device, the untagged inverse STFT payloads, the wrappers' host validation and the
arithmetic of the schedule helper."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT
from test_dct4_host import ref_dct4
from test_mdct_host import ref_mdct

ISTFT, STFT, REFLECT, ZEROS = 0x4000, 32, 64, 128
UNSUPPORTED, BAD_DIM, BAD_COMPONENTS, BAD_DTYPE, BAD_BASES, NO_DEVICE = -15, -2, -3, -4, -5, -10
TAG_LO, TAG_HI = 0x43544401, 0x7FF84D44


# ---- references (fp64) ---------------------------------------------------------------------------------------------------------
def imdct_gain(n, norm):
    return np.sqrt(2.0 / n) if norm == "ortho" else 2.0 / n


def ref_imdct(X, n, w=None, norm=None, length=None):
    """the definition: X (B, F, n) -> (B, T).  y_f[j] = g w[j] sum_k X[f, k] cos(pi / n (j + 1/2 + n/2)(k + 1/2)), j < 2n, and
    out[q n + i] = y_q[n + i] + y_(q+1)[i]"""
    X = np.asarray(X, dtype=np.float64)
    B, F, M = X.shape
    assert M == n
    T = (F - 1) * n if length is None else length
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n)) if w is None else np.asarray(w, dtype=np.float64)
    j, k = np.arange(2 * n), np.arange(n)
    C = np.cos(np.pi / n * np.outer(j + 0.5 + n / 2, k + 0.5))  # (2n, n)
    y = imdct_gain(n, norm) * w * (X @ C.T)                      # (B, F, 2n)
    out = (y[:, :-1, n:] + y[:, 1:, :n]).reshape(B, (F - 1) * n)
    return out[:, :T]


def unfold_imdct(X, n, w=None, norm=None, length=None):
    """the arithmetic of the composition: v = DCT-IV(X) / 2 through ref_dct4, the index / sign table of
    _mdct_unfold_tables, the window and two shifted adds"""
    X = np.asarray(X, dtype=np.float64)
    B, F, _ = X.shape
    T = (F - 1) * n if length is None else length
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n)) if w is None else np.asarray(w, dtype=np.float64)
    idx, sign = (t.numpy() for t in mf.api._mdct_unfold_tables(n))
    v = ref_dct4(X) / 2
    y = imdct_gain(n, norm) * w * sign * v[..., idx]
    out = np.zeros((B, (F + 1) * n))
    out[:, :F * n] += y[..., :n].reshape(B, F * n)
    out[:, n:] += y[..., n:].reshape(B, F * n)
    return out[:, n:n + T]


def pb_window(n, seed):
    """a random window with w[j] ** 2 + w[j + n] ** 2 = 1 (Princen-Bradley) and the symmetry w[j] = w[2n - 1 - j] that time-domain
    aliasing cancellation needs"""
    th = np.random.default_rng(seed).uniform(0.1, np.pi / 2 - 0.1, n // 2)
    th = np.concatenate([th, np.pi / 2 - th[::-1]])  # theta[n-1-j] = pi/2 - theta[j]
    return np.concatenate([np.sin(th), np.cos(th)])


@pytest.mark.parametrize("norm", [None, "ortho"], ids=str)
@pytest.mark.parametrize("n", [8, 30, 64])
def test_the_reference_inverts_the_forward_reference(n, norm):
    rng = np.random.default_rng(n)
    for T in (5 * n, 5 * n + 3):
        x = rng.standard_normal((3, T))
        for w in (None, pb_window(n, n + 1)):
            if w is not None:
                assert np.abs(w[:n] ** 2 + w[n:] ** 2 - 1).max() < 1e-15 and np.abs(w - w[::-1]).max() < 1e-15
            X = ref_mdct(x, n, w, norm)
            assert np.abs(ref_imdct(X, n, w, norm, length=T) - x).max() < 1e-12
            full = ref_imdct(X, n, w, norm)
            assert full.shape == (3, (X.shape[1] - 1) * n) and np.abs(full[:, :T] - x).max() < 1e-12
            assert np.abs(full[:, T:]).max(initial=0.0) < 1e-12  # (the zeros the last frame saw beyond the signal)


@pytest.mark.parametrize("n", [8, 30, 64, 200])
def test_the_reference_equals_the_composition_arithmetic(n):
    rng = np.random.default_rng(n + 7)
    X = rng.uniform(-1, 1, (2, 6, n))
    w = rng.uniform(0.25, 1.0, 2 * n) * rng.choice([-1.0, 1.0], 2 * n)
    for norm in (None, "ortho"):
        for T in (None, 4 * n + 1, 2):
            a, b = ref_imdct(X, n, w, norm, T), unfold_imdct(X, n, w, norm, T)
            assert a.shape == b.shape and np.abs(a - b).max() < 1e-12 * n


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _words(values):
    return [w for v in values for w in struct.unpack("<II", struct.pack("<d", float(v)))]


def _create(T, F, M, *, hop=None, center=ZEROS, extra=0, gain=0.25, window=None, radices=(), tag=(TAG_LO, TAG_HI), in_dtype=0,
            out_dtype=0, inverse=1, comps=1, len0=None, pad=0):
    """an IMDCT request through mifft_plan_create; ``pad`` more window words in front of the tag (a tagged payload of another
    length), ``len0`` another bases_len[0]"""
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * 3)(T, F, 2 * M)
    flat = _words([0.5] * (2 * M) if window is None else window) + [0] * pad + list(tag) + _words([gain])
    lens = (ctypes.c_int32 * 3)(len(flat) if len0 is None else len0, 0, len(radices))
    flat = flat + list(radices)
    flags = ISTFT | center | ((M if hop is None else hop) << 16) | extra
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, 3, c_dims, 3, comps, inverse,
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
            (dict(center=0), UNSUPPORTED, "centre bit"),
            (dict(center=REFLECT), UNSUPPORTED, "MIFFT_FLAG_STFT_CENTER_REFLECT"),
            (dict(center=REFLECT | ZEROS), UNSUPPORTED, "MIFFT_FLAG_STFT_CENTER_REFLECT"),
            (dict(F=1), BAD_DIM, "dims[1]"),
            (dict(T=1), BAD_DIM, "size 1"),                             # (the rule that no dimension but F is of size 1)
            (dict(T=4 * 16 + 1), BAD_DIM, "dims[0]"),                   # T > (F - 1) M
            (dict(comps=2), BAD_COMPONENTS, "in_components"),
            (dict(in_dtype=2), BAD_DTYPE, "in_dtype"),
            (dict(in_dtype=0, out_dtype=1), BAD_DTYPE, "in_dtype"),
            (dict(M=6), UNSUPPORTED, "M = 6"),                          # below 8
            (dict(M=9), UNSUPPORTED, "M = 9"),                          # odd
            (dict(M=74), UNSUPPORTED, "packed"),                        # M / 2 = 37
            (dict(M=32768), UNSUPPORTED, "M = 32768"),
            (dict(M=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288 points (a 96-KiB tile)
            (dict(window=[1.0] * 7 + [inf] + [1.0] * 24), BAD_BASES, "window value 7"),
            (dict(window=[nan] + [1.0] * 31), BAD_BASES, "window value 0"),
            (dict(gain=inf), BAD_BASES, "gain"),
            (dict(gain=nan), BAD_BASES, "gain"),
            (dict(gain=0.0), BAD_BASES, "gain"),
            (dict(inverse=0), UNSUPPORTED, "inverse"),
            (dict(extra=STFT), UNSUPPORTED, "MIFFT_FLAG_ISTFT"),        # the two mode bits
            (dict(extra=1), UNSUPPORTED, "MIFFT_FLAG_FAITHFUL_STAGES"),
            (dict(extra=2), UNSUPPORTED, "MIFFT_FLAG_HALF_SPECTRUM"),
            (dict(extra=4), UNSUPPORTED, "MIFFT_FLAG_DCT"),
            (dict(extra=8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(radices=(3,)), BAD_BASES, "length: 8"),               # the radices factor M / 2
            # a tagged payload of another length; no tag, or the spectrogram's tag, in the slot: bases_len[0] is named
            (dict(pad=2), BAD_BASES, "bases_len[0]"),
            (dict(len0=4 * 16 + 1, comps=2), BAD_BASES, "bases_len[0]"),
            (dict(tag=tuple(_words([1.0])), comps=2), BAD_BASES, "bases_len[0]"),
            (dict(tag=(mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI), comps=2), BAD_BASES, "bases_len[0]"),
    ):
        kw = dict(kw)
        rc, why = _create(kw.pop("T", 50), kw.pop("F", 5), kw.pop("M", 16), **kw)
        assert rc == status and word in why, (kw, rc, why)
    assert len(_lib.EXPORTS) == 21  # (no new entry point)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    for T, F, M, kw in ((50, 5, 16, {}), (20, 4, 8, {}), (100, 5, 30, {}), (1000, 5, 256, {}), (4000, 5, 1024, {}),
                        (30000, 5, 8192, {}), (60000, 5, 16384, {}), (4000, 5, 1024, dict(in_dtype=1, out_dtype=1)),
                        (8, 2, 8, {}), (2, 2, 8, {}), (2, 7, 16, {}), (6 * 16, 7, 16, {}),
                        (50, 5, 16, dict(radices=(2,))), (1000, 5, 256, dict(radices=(16, 8))), (50, 5, 16, dict(gain=-0.25))):
        rc, why = _create(T, F, M, **kw)
        assert rc == NO_DEVICE, (T, F, M, kw, why)


def _istft_create(n, flat, len0, F=9, hop=16):
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 3, (ctypes.c_int64 * 3)(100, F, n), 3, 2, 1,
                             (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * 3)(len0, 0, 0), ISTFT | (hop << 16))
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


def test_untagged_istft_payloads_are_what_they_were():
    n = 64
    for flat in ([], _words([0.5] * n), _words([0.5] * n + [8.0])):
        rc, why = _istft_create(n, flat, len(flat))
        assert rc == (0 if torch.cuda.is_available() else NO_DEVICE), (len(flat), why)
    for len0 in (126, 129):
        rc, why = _istft_create(n, _words([0.5] * (n + 2)), len0)
        assert rc == BAD_BASES and "bases_len[0]" in why, (len0, why)


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_imdct_host import _create\n"
            "print(*_create(50, 5, 16))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_plan_imdct_validates_before_device_work():
    f32 = torch.float32
    for args, kw, status in (((torch.float16, 3, 5, 8), {}, BAD_DTYPE), ((f32, 3, 5, 6), {}, UNSUPPORTED),
                             ((f32, 3, 5, 9), {}, UNSUPPORTED), ((f32, 3, 1, 8), {}, BAD_DIM),
                             ((f32, 3, 5, 8), dict(length=1), BAD_DIM), ((f32, 3, 5, 8), dict(length=33), BAD_DIM),
                             ((f32, 3, 5, 8), dict(norm="forward"), UNSUPPORTED),
                             ((f32, 3, 5, 8), dict(window=torch.ones(8)), BAD_BASES)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_imdct(*args, **kw)
        assert e.value.status == status, (args, kw)
    with pytest.raises(mf.MifftError) as e:  # the layouts of a Plan are checked against the frames
        mf.Plan(f32, f32, (3, 5, 8, 1), (3, 33, 1), imdct=8)
    assert e.value.status == BAD_DIM
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(f32, f32, (3, 5, 16, 1), (3, 32, 1), imdct=8)
    assert e.value.status == BAD_DIM
    with pytest.raises(mf.MifftError) as e:  # the library's refusal: 74 / 2 = 37 is a prime above 32
        mf.Plan(f32, f32, (3, 5, 74, 1), (3, 100, 1), imdct=74)
    assert e.value.status == UNSUPPORTED and "packed" in str(e.value)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(norm="ortho"), dict(length=17), dict(window=torch.hann_window(16, dtype=torch.float64))):
            with pytest.raises(mf.MifftError) as e:
                mf.plan_imdct(f32, 3, 5, 8, **kw)
            assert e.value.status == NO_DEVICE, kw


def test_imdct_validates_on_the_host():
    X = torch.zeros(3, 14, 8)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(norm="forward"), UNSUPPORTED), (dict(window=torch.ones(15)), BAD_BASES), (dict(length=0), BAD_DIM),
                       (dict(length=13 * 8 + 1), BAD_DIM)):
        with pytest.raises(mf.MifftError) as e:
            mf.imdct(X, **kw)
        assert e.value.status == status, kw
    for ok in (dict(), dict(length=1), dict(length=2), dict(norm="ortho"), dict(window=[0.5] * 16)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.imdct(X, **ok)
        assert e.value.status == NO_DEVICE, ok


def test_the_schedule_arithmetic():
    S = mf.api._imdct_schedule
    # 3 entries of 10 frames in tiles of 4: tiles per entry 3 (4, 4, 2 frames), 9 tiles
    assert S(4, 9, 1, 10) == [(0, 9, 0)]
    assert S(4, 9, 2, 10) == [(0, 5, 0), (5, 4, 1)]                       # tile 5 is tile 2 of entry 1: one warm-up frame
    assert S(4, 9, 3, 10) == [(0, 3, 0), (3, 3, 0), (6, 3, 0)]            # every run starts an entry
    assert S(4, 9, 4, 10) == [(0, 3, 0), (3, 2, 0), (5, 2, 1), (7, 2, 1)]
    assert S(4, 9, 9, 10) == [(t, 1, 1 if t % 3 else 0) for t in range(9)]
    # one tile per entry (F <= TILE): no run ever starts inside an entry
    assert S(8, 5, 2, 8) == [(0, 3, 0), (3, 2, 0)]
    # TILE 1: every frame is a tile and hands its carry on
    assert S(1, 10, 3, 5) == [(0, 4, 0), (4, 3, 1), (7, 3, 1)]
    for tile, n_tiles, grid, F in ((4, 9, 4, 10), (1, 10, 3, 5), (7, 100, 13, 30)):
        runs = S(tile, n_tiles, grid, F)
        assert len(runs) == grid and runs[0][0] == 0 and sum(r[1] for r in runs) == n_tiles
        assert all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert max(r[1] for r in runs) - min(r[1] for r in runs) <= 1
