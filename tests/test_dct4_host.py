"""DCT-IV of real rows (MIFFT_DCT_TYPE4_TAG in the `bases` of a MIFFT_FLAG_DCT plan): the ABI constant, every refusal that needs
no device, and the fp64 numpy references the GPU tests compare against, themselves checked against the cosine sums here."""
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
from conftest import ROOT

DCT, ORTHO = 4, 8
UNSUPPORTED = -15
TAG = 0x44435434


# ---- references (fp64) ---------------------------------------------------------------------------------------------------------
def dct4_matrix(n):
    """C[j, k] = 2 cos(pi (2j+1)(2k+1) / 4n): scipy.fft.dct(x, 4) = x @ C (symmetric)"""
    j = np.arange(n)
    return 2.0 * np.cos(np.pi * np.outer(2 * j + 1, 2 * j + 1) / (4.0 * n))


def dct4_fft(x):
    """scipy.fft.dct(x, 4) of the rows of x by the n / 2-point complex route, for rows too long for the matrix:
    z_m = x[2m] + i x[n-1-2m], S = p . fft(p . z), p_m = e^(-i pi (8m+1) / 8n), X[2k] = 2 Re S_k, X[n-1-2k] = -2 Im S_k"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    p = np.exp(-1j * np.pi * (8 * np.arange(n // 2) + 1) / (8.0 * n))
    S = p * np.fft.fft(p * (x[..., 0::2] + 1j * x[..., ::-1][..., 0::2]), axis=-1)
    X = np.empty_like(x)
    X[..., 0::2] = 2 * S.real
    X[..., ::-1][..., 0::2] = -2 * S.imag
    return X


def ref_dct4(x, norm=None, inverse=False):
    """scipy.fft.dct / idct (type 4) of the rows of x in fp64: the cosine matrix up to 1080 points, the FFT route beyond"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    X = x @ dct4_matrix(n) if n <= 1080 else dct4_fft(x)
    if norm == "ortho":
        return X * np.sqrt(1.0 / (2 * n))
    return X / (2 * n) if inverse else X


def test_the_references_are_the_cosine_sum():
    rng = np.random.default_rng(4)
    for n in (8, 30, 64):
        x = rng.standard_normal((3, n))
        want = np.array([[2 * sum(x[r, j] * np.cos(np.pi * (2 * j + 1) * (2 * k + 1) / (4 * n)) for j in range(n))
                          for k in range(n)] for r in range(3)])
        assert np.abs(x @ dct4_matrix(n) - want).max() < 1e-12
        assert np.abs(dct4_fft(x) - want).max() < 1e-12
        assert np.abs(ref_dct4(ref_dct4(x), inverse=True) - x).max() < 1e-12          # idct(dct(x)) = x
        assert np.abs(ref_dct4(ref_dct4(x, "ortho"), "ortho") - x).max() < 1e-12        # ortho: an involution
    x = rng.standard_normal((2, 1000))
    assert np.abs(dct4_fft(x) - x @ dct4_matrix(1000)).max() < 1e-10


def test_the_reference_is_scipys_type_4():
    fft = pytest.importorskip("scipy.fft")
    x = np.random.default_rng(5).standard_normal((3, 30))
    for norm in (None, "ortho"):
        assert np.abs(ref_dct4(x, norm) - fft.dct(x, type=4, norm=norm)).max() < 1e-12
        assert np.abs(ref_dct4(x, norm, inverse=True) - fft.idct(x, type=4, norm=norm)).max() < 1e-12


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_the_tag_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    m = re.search(r"#define\s+MIFFT_DCT_TYPE4_TAG\s+0x([0-9A-Fa-f]+)u\b", h)
    assert m and int(m.group(1), 16) == TAG
    assert TAG > 16384  # no radix can equal it
    assert "MIFFT_DCT_TYPE4_TAG" in open(os.path.join(ROOT, "include", "mifft.hpp")).read()
    assert mf.DCT_TYPE4_TAG == mf.api.DCT_TYPE4_TAG == TAG


def test_export_list_is_unchanged():
    assert len(_lib.EXPORTS) == 21  # (the DCT-IV travels in `bases`: no new entry point, no new flag bit)


def _create(dims, *, bases=(TAG,), comps=1, inverse=False, in_dtype=0, out_dtype=0, flags=DCT, batch=3):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    flat = lens = None
    if bases is not None:
        flat = (ctypes.c_uint32 * max(len(bases), 1))(*bases)
        lens = (ctypes.c_int32 * len(dims))(len(bases), *([0] * (len(dims) - 1)))
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, len(dims), c_dims, batch, comps, int(inverse),
                             flat, lens, flags)
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


@pytest.mark.parametrize("inverse", [False, True])
def test_c_abi_refuses_before_looking_for_a_device(inverse):
    for kw, status, word in (
            (dict(dims=[64], comps=2), -3, "in_components"),
            (dict(dims=[64, 64]), UNSUPPORTED, "ndim"),
            (dict(dims=[31]), UNSUPPORTED, "odd"),
            (dict(dims=[6]), UNSUPPORTED, "8 points"),
            (dict(dims=[2 * 37 * 4]), UNSUPPORTED, "packed"),
            (dict(dims=[32768]), UNSUPPORTED, "16384"),
            (dict(dims=[16384], in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288 points (a 96-KiB tile)
            (dict(dims=[1024], flags=DCT | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (dict(dims=[1024], flags=DCT | 1), UNSUPPORTED, "FAITHFUL"),
            (dict(dims=[1024], flags=DCT | (1 << 8)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[1024], flags=ORTHO), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO without"),
            (dict(dims=[64], in_dtype=2), -4, "in_dtype"),                  # both directions read the plan's own float type
            (dict(dims=[64], in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(dims=[1024], bases=(TAG, 3)), -5, "512"),                 # the radices behind the tag factor n / 2
            (dict(dims=[1024], bases=(TAG, 2), flags=16), UNSUPPORTED, "MIFFT_FLAG_DCT_ND"),  # the N-D DCT has no type 4
    ):
        rc, why = _create(inverse=inverse, **kw)
        assert rc == status and word in why, (kw, rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
@pytest.mark.parametrize("inverse", [False, True])
def test_a_valid_request_gets_as_far_as_the_device(inverse):
    for n in (8, 30, 1024, 16384):
        for flags in (DCT, DCT | ORTHO):
            rc, why = _create([n], inverse=inverse, flags=flags)
            assert rc == -10, (n, why)
    rc, why = _create([8192], inverse=inverse, in_dtype=1, out_dtype=1)  # the longest fp64 power of two (the longest row: 12288)
    assert rc == -10, why
    rc, why = _create([1024], inverse=inverse, bases=(TAG, 16, 16, 2))  # the tag, then the radices of 512
    assert rc == -10, why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_an_untagged_plan_is_what_it_was():
    rc, why = _create([64], bases=None, in_dtype=2)  # DCT-II: the forward widens every in_dtype
    assert rc == -10, why
    rc, why = _create([64], bases=(2,), in_dtype=2)  # radices without the tag
    assert rc == -10, why
    rc, why = _create([64], bases=None, inverse=True, in_dtype=2)
    assert rc == -4 and "inverse" in why, why


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "for n in (1024, 30):\n"
            "    for inv in (0, 1):\n"
            "        h = ctypes.c_void_p(); d = (ctypes.c_int64 * 1)(n)\n"
            "        b = (ctypes.c_uint32 * 1)(%d); l = (ctypes.c_int32 * 1)(1)\n"
            "        rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 1, d, 4, 1, inv, b, l, 4)\n"
            "        print(n, rc, L.mifft_last_error().decode())\n" % (ROOT, TAG))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4
    for ln in lines:
        _, rc, why = ln.split(" ", 2)
        assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, ln


# ---- Python --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [mf.dct, mf.idct], ids=["dct", "idct"])
def test_the_row_wrappers_accept_type_4(fn):
    x = torch.zeros(3, 64)  # (a host tensor: nothing reaches the library)
    for ok in (dict(type=4), dict(type=4, norm="ortho"), dict(type=4, dim=-1), dict(type=4, out_dtype=torch.float64), dict(type=2)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            fn(x, **ok)
        assert e.value.status == -10, ok
    for kw, status in ((dict(type=1), UNSUPPORTED), (dict(type=3), UNSUPPORTED), (dict(type=5), UNSUPPORTED),
                       (dict(type=4, norm="forward"), UNSUPPORTED), (dict(type=4, dim=0), UNSUPPORTED),
                       (dict(type=4, out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            fn(x, **kw)
        assert e.value.status == status, kw
    for bad in (torch.zeros(3, 63), torch.zeros(3, 6)):
        with pytest.raises(mf.MifftError) as e:
            fn(bad, type=4)
        assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("fn", [mf.dctn, mf.idctn], ids=["dctn", "idctn"])
def test_the_nd_wrappers_still_refuse_it(fn):
    for t in (1, 3, 4):
        with pytest.raises(mf.MifftError) as e:
            fn(torch.zeros(3, 64, 64), type=t)
        assert e.value.status == UNSUPPORTED and "type" in str(e.value), t


def test_plan_fft_takes_dct_type():
    shape = (4, 64, 1)
    for make in (mf.Plan, mf.plan_fft):  # (plan_fft: before it creates a device context)
        with pytest.raises(mf.MifftError) as e:
            make(torch.float32, torch.float32, shape, shape, dct=True, dct_type=3)
        assert e.value.status == UNSUPPORTED and "dct_type" in str(e.value)
        with pytest.raises(mf.MifftError) as e:  # layouts are checked as for type 2
            make(torch.float32, torch.float32, shape, (4, 32, 1), dct=True, dct_type=4)
        assert e.value.status == -2
        if not torch.cuda.is_available():
            for kw in (dict(), dict(norm="ortho"), dict(inverse=True), dict(bases=[[16, 2]])):
                with pytest.raises(mf.MifftError) as e:
                    make(torch.float32, torch.float32, shape, shape, dct=True, dct_type=4, **kw)
                assert e.value.status == -10, kw
    with pytest.raises(mf.MifftError) as e:  # the DCT-IV reads its own float type: the library's refusal
        mf.Plan(torch.uint8, torch.float32, shape, shape, dct=True, dct_type=4)
    assert e.value.status == -4
    with pytest.raises(mf.MifftError) as e:  # radices that do not multiply to n / 2
        mf.Plan(torch.float32, torch.float32, shape, shape, dct=True, dct_type=4, bases=[[3]])
    assert e.value.status == -5
    with pytest.raises(mf.MifftError) as e:  # one list, as for every DCT plan
        mf.Plan(torch.float32, torch.float32, shape, shape, dct=True, dct_type=4, bases=[[16], [2]])
    assert e.value.status == -7
