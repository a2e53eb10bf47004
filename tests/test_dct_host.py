"""DCT-II / DCT-III of real rows (MIFFT_FLAG_DCT): the ABI constants and every refusal that needs no device -- the C library's
checks run before it looks for a HIP device, the Python checks before any device context is created."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT

DCT, ORTHO = 4, 8
UNSUPPORTED = -15


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_flags_are_declared():
    h = _header("mifft.h")
    assert re.search(r"#define\s+MIFFT_FLAG_DCT\s+4u\b", h)
    assert re.search(r"#define\s+MIFFT_FLAG_DCT_ORTHO\s+8u\b", h)
    hpp = _header("mifft.hpp")
    assert "MIFFT_FLAG_DCT_ORTHO" in hpp and re.search(r"MIFFT_FLAG_DCT\b", hpp)
    assert mf.FLAG_DCT == mf.api.FLAG_DCT == DCT
    assert mf.FLAG_DCT_ORTHO == mf.api.FLAG_DCT_ORTHO == ORTHO


def test_export_list_is_unchanged():
    assert len(_lib.EXPORTS) == 21  # (the DCT added none; mifft_plan_pass_geometry came later)
    assert _lib.lib().mifft_version() == 1


def _create(dims, *, comps=1, inverse=False, in_dtype=0, out_dtype=0, flags=DCT, batch=3):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, len(dims), c_dims, batch, comps, int(inverse),
                             None, None, flags)
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
            (dict(dims=[2 * 37 * 4]), UNSUPPORTED, "packed"),               # n / 2 has a prime factor above 32
            (dict(dims=[32768]), UNSUPPORTED, "16384"),                     # beyond the longest row
            (dict(dims=[16384], in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),  # fp64 rows end at 12288 points (a 96-KiB tile)
            (dict(dims=[1024], flags=DCT | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (dict(dims=[1024], flags=DCT | 1), UNSUPPORTED, "FAITHFUL"),
            (dict(dims=[1024], flags=DCT | (1 << 8)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[1024, 64], flags=DCT | (1 << 8)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[1024], flags=ORTHO), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO without"),
    ):
        rc, why = _create(inverse=inverse, **kw)
        assert rc == status and word in why, (kw, rc, why)


def test_c_abi_inverse_reads_its_own_float_type():
    rc, why = _create([64], inverse=True, in_dtype=2)  # uint8 coefficients
    assert rc == -4 and "in_dtype" in why, why
    rc, why = _create([64], inverse=True, in_dtype=0, out_dtype=1)
    assert rc == -4, why
    rc, why = _create([64], inverse=False, in_dtype=2)  # the forward widens every in_dtype
    assert rc in (0, -10), why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [1024, 30])
def test_a_valid_request_gets_as_far_as_the_device(n, inverse):
    for flags in (DCT, DCT | ORTHO):
        rc, why = _create([n], inverse=inverse, flags=flags)
        assert rc == -10, why
    rc, why = _create([8192], inverse=inverse, in_dtype=1, out_dtype=1)  # the longest fp64 power of two (the longest row: 12288)
    assert rc == -10, why
    rc, why = _create([16384], inverse=inverse)
    assert rc == -10, why


def test_without_runtime_specialisation_only_1024_points_are_routed():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process): 1024 points, fp32 and fp64, both directions and both
    size regimes of the forward, get past every check that needs no device; 1000 points are refused with the reason."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "for n, dt, batch in ((1024, 0, 4), (1024, 1, 4), (1024, 0, 1000000), (1000, 0, 4)):\n"
            "    for inv in (0, 1):\n"
            "        h = ctypes.c_void_p(); d = (ctypes.c_int64 * 1)(n)\n"
            "        rc = L.mifft_plan_create(ctypes.byref(h), 0, dt, dt, 1, d, batch, 1, inv, None, None, 4)\n"
            "        if rc == 0: L.mifft_plan_destroy(h)\n"
            "        print(n, rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8
    for ln in lines:
        n, rc, why = ln.split(" ", 2)
        if n == "1000":
            assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, ln
        else:  # planned on a GPU box, refused for want of a device here
            assert int(rc) in (0, -10), ln


@pytest.mark.parametrize("in_shape,out_shape,status", [
    ((4, 64, 1), (4, 64, 2), -3),        # a DCT writes reals
    ((4, 64, 2), (4, 64, 1), -3),        # ... and reads reals
    ((4, 64, 1), (4, 32, 1), -2),        # as many as it reads
    ((4, 64, 1), (5, 64, 1), -2),
    ((4, 8, 64, 1), (4, 8, 64, 1), -2),  # rows only: (batch, n, 1)
    ((4, 63, 1), (4, 63, 1), UNSUPPORTED),
    ((4, 6, 1), (4, 6, 1), UNSUPPORTED),
    ((4, 64, 1), (4, 64, 1), None),      # (valid: reaches the device)
])
@pytest.mark.parametrize("inverse", [False, True])
def test_python_layout_validation(in_shape, out_shape, status, inverse):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        with pytest.raises(mf.MifftError) as e:
            mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dct=True, norm="ortho")
        assert e.value.status == -10
        return
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dct=True)
    assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # the flag bit is the same request
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, flags=DCT)
    assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # plan_fft: before it creates a device context
        mf.plan_fft(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dct=True)
    assert e.value.status == status


def test_plan_norm_is_validated_before_device_work():
    for make in (mf.Plan, mf.plan_fft):
        with pytest.raises(mf.MifftError) as e:
            make(torch.float32, torch.float32, (4, 64, 1), (4, 64, 1), dct=True, norm="forward")
        assert e.value.status == UNSUPPORTED and "norm" in str(e.value)


def test_other_layout_checks_are_unchanged():
    with pytest.raises(mf.MifftError) as e:  # without dct=True a real output layout is still refused
        mf.Plan(torch.float32, torch.float32, (4, 64, 1), (4, 64, 1))
    assert e.value.status == -3


@pytest.mark.parametrize("fn", [mf.dct, mf.idct], ids=["dct", "idct"])
def test_wrappers_validate_on_the_host(fn):
    x = torch.zeros(3, 64)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(type=3), UNSUPPORTED), (dict(type=1), UNSUPPORTED), (dict(norm="forward"), UNSUPPORTED),
                       (dict(norm=1), UNSUPPORTED), (dict(dim=0), UNSUPPORTED), (dict(dim=2), -2),
                       (dict(out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            fn(x, **kw)
        assert e.value.status == status, kw
    for bad in (torch.zeros(3, 63), torch.zeros(3, 6), torch.zeros(9)):  # odd n, n below 8
        with pytest.raises(mf.MifftError) as e:
            fn(bad)
        assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:  # the innermost dim of size above 1 is dim 1 here
        fn(torch.zeros(3, 64, 1), dim=0)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        fn(torch.zeros(3, 64, dtype=torch.complex64))
    assert e.value.status == -3
    for ok in (dict(), dict(norm="ortho"), dict(norm="backward"), dict(dim=-1), dict(dim=1)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            fn(x, **ok)
        assert e.value.status == -10, ok
    with pytest.raises(mf.MifftError) as e:  # trailing dims of size 1 do not count
        fn(torch.zeros(3, 64, 1), dim=1)
    assert e.value.status == -10
