"""Half-spectrum real transforms (MIFFT_FLAG_HALF_SPECTRUM): the ABI constants and every refusal that needs no device --
the C library's checks run before it looks for a HIP device, the Python layout checks before any tensor is allocated."""
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

FLAG = 2
UNSUPPORTED = -15


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_flag_and_status_are_declared():
    h = _header("mifft.h")
    assert re.search(r"#define\s+MIFFT_FLAG_HALF_SPECTRUM\s+2u\b", h)
    assert re.search(r"MIFFT_ERR_UNSUPPORTED\s*=\s*-15\b", h)
    assert "MIFFT_FLAG_HALF_SPECTRUM" in _header("mifft.hpp")
    assert mf.api.FLAG_HALF_SPECTRUM == FLAG


def test_export_list_and_version_are_unchanged():
    assert len(_lib.EXPORTS) == 21 and "mifft_plan_create_slab" in _lib.EXPORTS  # (+ mifft_plan_pass_geometry)
    assert _lib.lib().mifft_version() == 1


def test_unsupported_status_string():
    L = _lib.lib()
    assert L.mifft_status_string(UNSUPPORTED) == b"unsupported request"
    assert L.mifft_status_string(-14) == b"buffer too small"


def _create(dims, *, comps, inverse, in_dtype=0, out_dtype=0, flags=FLAG, device=0):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    rc = L.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, len(dims), c_dims, 3, comps, int(inverse),
                             None, None, flags)
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, L.mifft_last_error().decode()


@pytest.mark.parametrize("inverse", [False, True])
def test_c_abi_refuses_before_looking_for_a_device(inverse):
    comps = 2 if inverse else 1
    rc, why = _create([64, 30 + 1], comps=comps, inverse=inverse)  # odd last dim
    assert rc == UNSUPPORTED and "odd" in why
    rc, why = _create([64, 32], comps=comps, inverse=inverse, flags=FLAG | 1)  # + MIFFT_FLAG_FAITHFUL_STAGES
    assert rc == UNSUPPORTED and "FAITHFUL" in why
    rc, why = _create([8192, 32], comps=comps, inverse=inverse)  # an outer dim beyond one column tile
    assert rc == UNSUPPORTED and "dimension 0" in why
    rc, why = _create([16, 2 * 37], comps=comps, inverse=inverse)  # n / 2 = 37: a prime above 32
    assert rc == UNSUPPORTED and "packed" in why
    rc, why = _create([4], comps=comps, inverse=inverse)  # below 8
    assert rc == UNSUPPORTED
    rc, why = _create([16, 32], comps=3 - comps, inverse=inverse)  # wrong component count for the direction
    assert rc == -3, why


def test_c_abi_inverse_reads_its_own_float_type():
    rc, why = _create([32], comps=2, inverse=True, in_dtype=2)  # uint8 half spectrum
    assert rc == -4, why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_half_spectrum_request_gets_as_far_as_the_device():
    rc, _ = _create([16, 480], comps=1, inverse=False)
    assert rc == -10
    rc, _ = _create([16, 480], comps=2, inverse=True)
    assert rc == -10


def test_without_runtime_specialisation_only_precompiled_lengths_are_routed():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process): the precompiled packed-row lengths get past every
    check that needs no device, a length without an instance (1000) is refused with the reason."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "for n, dt in ((1024, 0), (1920, 1), (1000, 0)):\n"
            "    for inv in (0, 1):\n"
            "        h = ctypes.c_void_p(); d = (ctypes.c_int64 * 1)(n)\n"
            "        rc = L.mifft_plan_create(ctypes.byref(h), 0, dt, dt, 1, d, 4, 1 + inv, inv, None, None, 2)\n"
            "        if rc == 0: L.mifft_plan_destroy(h)\n"
            "        print(n, rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for ln in r.stdout.strip().splitlines():
        n, rc, why = ln.split(" ", 2)
        if n == "1000":
            assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, ln
        else:  # planned on a GPU box, refused for want of a device here
            assert int(rc) in (0, -10), ln


def test_fp64_rows_end_at_12288_points():
    rc, why = _create([16384], comps=1, inverse=False, out_dtype=1, in_dtype=1)
    assert rc == UNSUPPORTED and "packed" in why
    rc, why = _create([16384], comps=1, inverse=False)  # fp32: the last supported length
    assert rc != UNSUPPORTED, why
    rc, why = _create([8192], comps=2, inverse=True, out_dtype=1, in_dtype=1)
    assert rc != UNSUPPORTED, why
    # the rule: the n / 2-point row tile fits 96 KiB of LDS -- 12288 points in fp64; the next smooth half is 12320 / 2
    for inverse in (False, True):
        rc, why = _create([12288], comps=2 if inverse else 1, inverse=inverse, out_dtype=1, in_dtype=1)
        assert rc != UNSUPPORTED, why
        rc, why = _create([12320], comps=2 if inverse else 1, inverse=inverse, out_dtype=1, in_dtype=1)
        assert rc == UNSUPPORTED and "packed" in why


def test_the_flag_bit_alone_selects_the_half_spectrum_layouts():
    with pytest.raises(mf.MifftError) as e:  # a full-spectrum layout is not a half-spectrum one
        mf.Plan(torch.float32, torch.float32, (4, 32, 1), (4, 32, 2), flags=FLAG)
    assert e.value.status == -2


@pytest.mark.parametrize("in_shape,out_shape,inverse,status", [
    ((4, 33, 1), (4, 17, 2), False, UNSUPPORTED),      # odd n
    ((4, 32, 1), (4, 16, 2), False, -2),               # h != n // 2 + 1
    ((4, 32, 1), (4, 32, 2), False, -2),               # the full spectrum is not a half-spectrum layout
    ((4, 32, 2), (4, 17, 2), False, -3),               # forward reads real input
    ((4, 32, 1), (4, 17, 1), False, -3),               # ... and writes complex output
    ((4, 17, 2), (4, 32, 1), True, None),              # (valid: reaches the device)
    ((4, 17, 1), (4, 32, 1), True, -3),                # inverse reads complex input
    ((4, 17, 2), (4, 32, 2), True, -3),                # ... and writes real output
    ((4, 16, 2), (4, 32, 1), True, -2),                # h mismatch
    ((4, 8, 17, 2), (4, 9, 32, 1), True, -2),          # outer dims differ
    ((4, 17, 2), (4, 33, 1), True, UNSUPPORTED),       # odd n
])
def test_python_layout_validation(in_shape, out_shape, inverse, status):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        with pytest.raises(mf.MifftError) as e:
            mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, half_spectrum=True)
        assert e.value.status == -10
        return
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, half_spectrum=True)
    assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # plan_fft: before it creates a device context
        mf.plan_fft(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, half_spectrum=True)
    assert e.value.status == status


def test_full_spectrum_layout_checks_are_unchanged():
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, (4, 32, 1), (4, 17, 2))
    assert e.value.status == -2


def test_irfftn_validates_before_device_work():
    X = torch.zeros(3, 17, dtype=torch.complex64)  # (a host tensor: nothing reaches the library)
    with pytest.raises(mf.MifftError) as e:
        mf.irfftn(X, n=33)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        mf.irfftn(X, n=30)
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:
        mf.irfftn(torch.zeros(3, 17, 3), n=32)  # interleaved input has 2 components
    assert e.value.status == -3
    with pytest.raises(mf.MifftError) as e:
        mf.rfftn(torch.zeros(3, 33), onesided=True)
    assert e.value.status == UNSUPPORTED
