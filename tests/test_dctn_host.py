"""N-D DCT (MIFFT_FLAG_DCT_ND): the ABI constant and every refusal that needs no device -- the C library's checks run before it
looks for a HIP device, the Python checks before any device context is created."""
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

DCT, ORTHO, DCT_ND = 4, 8, 16
UNSUPPORTED = -15


def KEEP(d):
    return 1 << (8 + d)


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_flag_is_declared():
    assert re.search(r"#define\s+MIFFT_FLAG_DCT_ND\s+16u\b", _header("mifft.h"))
    assert re.search(r"MIFFT_FLAG_DCT_ND\b.*16u", _header("mifft.hpp"))
    assert mf.FLAG_DCT_ND == mf.api.FLAG_DCT_ND == DCT_ND
    assert DCT_ND & (mf.api.FLAG_KEEP_MASK | DCT | ORTHO | mf.api.FLAG_HALF_SPECTRUM | mf.api.FLAG_FAITHFUL_STAGES) == 0


def test_export_list_is_unchanged():
    assert len(_lib.EXPORTS) == 21  # (the N-D DCT added none)
    assert _lib.lib().mifft_version() == 1


def _create(dims, *, comps=1, inverse=False, in_dtype=0, out_dtype=0, flags=DCT_ND, batch=3):
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
            (dict(dims=[64, 64], flags=DCT_ND | DCT), UNSUPPORTED, "MIFFT_FLAG_DCT together"),
            (dict(dims=[64, 64], flags=DCT_ND | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (dict(dims=[64, 64], flags=DCT_ND | 1), UNSUPPORTED, "FAITHFUL"),
            (dict(dims=[64, 64], comps=2), -3, "in_components"),
            (dict(dims=[8, 7]), UNSUPPORTED, "odd"),                                   # the last dim is a row: even
            (dict(dims=[8, 7], flags=DCT_ND | KEEP(1)), UNSUPPORTED, "odd stride"),     # 7 reals between the points of dim 0
            (dict(dims=[8, 3, 5], flags=DCT_ND | KEEP(1) | KEEP(2)), UNSUPPORTED, "odd stride"),
            (dict(dims=[8, 2], flags=DCT_ND | KEEP(1)), UNSUPPORTED, "stride of 2"),    # a single pair of columns
            (dict(dims=[8192, 64]), UNSUPPORTED, "4096"),                               # beyond one column tile
            (dict(dims=[2 * 37, 64]), UNSUPPORTED, "prime factor above 32"),
            (dict(dims=[64, 6]), UNSUPPORTED, "8 points"),                              # the limits of the row kernel
            (dict(dims=[64, 2 * 37 * 4]), UNSUPPORTED, "packed"),
            (dict(dims=[1024], flags=ORTHO), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO without"),
    ):
        rc, why = _create(inverse=inverse, **kw)
        assert rc == status and word in why, (kw, rc, why)


def test_c_abi_dtype_rules():
    rc, why = _create([64, 64], inverse=True, in_dtype=2)  # an inverse reads its own float type
    assert rc == -4 and "in_dtype" in why, why
    rc, why = _create([64, 64], inverse=True, in_dtype=0, out_dtype=1)
    assert rc == -4, why
    rc, why = _create([30, 38], flags=DCT_ND | KEEP(1), in_dtype=2)  # a forward whose first pass is a column pass
    assert rc == UNSUPPORTED and "in_dtype" in why, why
    rc, why = _create([30, 38], in_dtype=2)  # ... the row pass of a transformed last dim widens every in_dtype
    assert rc in (0, -10), why


def test_the_one_dimensional_flag_keeps_its_refusals():
    rc, why = _create([64, 64], flags=DCT)
    assert rc == UNSUPPORTED and "ndim" in why, why
    rc, why = _create([1024, 64], flags=DCT | KEEP(0))
    assert rc == UNSUPPORTED and "KEEP_DIM" in why, why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
@pytest.mark.parametrize("inverse", [False, True])
def test_a_valid_request_gets_as_far_as_the_device(inverse):
    for dims, flags in (([64, 64], DCT_ND), ([15, 64], DCT_ND), ([8, 6, 8], DCT_ND | KEEP(1)),
                        ([30, 38], DCT_ND | KEEP(1)),  # the first pass is a column pass
                        ([64, 64], DCT_ND | ORTHO), ([64], DCT_ND), ([2, 8], DCT_ND), ([3, 8], DCT_ND)):
        rc, why = _create(dims, inverse=inverse, flags=flags)
        assert rc == -10, (dims, flags, why)
    rc, why = _create([4096, 8, 16384], inverse=inverse, batch=1)  # the longest column and row
    assert rc == -10, why
    rc, why = _create([2048, 8, 8192], inverse=inverse, in_dtype=1, out_dtype=1, batch=1)  # ... and long fp64 ones
    assert rc == -10, why
    rc, why = _create([4096, 64], inverse=inverse, in_dtype=1, out_dtype=1)
    # (8 x 8 x 8 x 8: a four-pass fp64 tile holds at most 4096 elements, two columns of 4096 points are 8192, and the chooser
    #  does not retry with three passes -- as at 2058, 2080, .. where the tile would be 66 KB; test_column_classes_host.py)
    assert rc == UNSUPPORTED and "column configuration" in why, why


def test_without_runtime_specialisation_a_column_pass_is_refused():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process): any column pass is refused with the reason before the
    library looks for a device; a plan of rows only (1024 points, the precompiled instance) gets past every such check"""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "for dims, flags in (((64, 1024), 16), ((30, 38), 16 | 512), ((1024,), 16), ((64, 1024), 16 | 256)):\n"
            "    for inv in (0, 1):\n"
            "        h = ctypes.c_void_p(); d = (ctypes.c_int64 * len(dims))(*dims)\n"
            "        rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, len(dims), d, 4, 1, inv, None, None, flags)\n"
            "        if rc == 0: L.mifft_plan_destroy(h)\n"
            "        print(len(dims), flags, rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8
    for ln in lines:
        nd, flags, rc, why = ln.split(" ", 3)
        if (nd, flags) in (("1", "16"), ("2", "272")):  # rows only: planned on a GPU box, refused for want of a device here
            assert int(rc) in (0, -10), ln
        else:
            assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, ln


@pytest.mark.parametrize("in_shape,out_shape,status", [
    ((4, 8, 64, 1), (4, 8, 64, 2), -3),           # a DCT writes reals
    ((4, 8, 64, 2), (4, 8, 64, 1), -3),           # ... and reads reals
    ((4, 8, 64, 1), (4, 8, 32, 1), -2),           # as many as it reads
    ((4, 8, 64, 1), (4, 64, 1), -1),              # equal ranks
    ((4, 1), (4, 1), -1),                         # at least one dim
    ((4, 8, 1, 64, 1), (4, 8, 1, 64, 1), -2),     # no inner dimension of size 1
    ((2,) + (4,) * 7 + (1,), (2,) + (4,) * 7 + (1,), -1),  # at most 6 dims
    ((4, 8, 64, 1), (4, 8, 64, 1), None),         # (valid: reaches the device)
    ((4, 64, 1), (4, 64, 1), None),
])
@pytest.mark.parametrize("inverse", [False, True])
def test_python_layout_validation(in_shape, out_shape, status, inverse):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        with pytest.raises(mf.MifftError) as e:
            mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dctn=True, norm="ortho")
        assert e.value.status == -10
        return
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dctn=True)
    assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # the flag bit is the same request
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, flags=DCT_ND)
    assert e.value.status == status
    with pytest.raises(mf.MifftError) as e:  # plan_fft: before it creates a device context
        mf.plan_fft(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, dctn=True)
    assert e.value.status == status


def test_plan_norm_and_axes_are_validated_before_device_work():
    shape = (4, 8, 64, 1)
    for make in (mf.Plan, mf.plan_fft):
        with pytest.raises(mf.MifftError) as e:
            make(torch.float32, torch.float32, shape, shape, dctn=True, norm="forward")
        assert e.value.status == UNSUPPORTED and "norm" in str(e.value)
        with pytest.raises(mf.MifftError) as e:
            make(torch.float32, torch.float32, shape, shape, dctn=True, axes=(3,))
        assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:  # both DCT requests at once: the library refuses the pair
        mf.Plan(torch.float32, torch.float32, (4, 64, 1), (4, 64, 1), dctn=True, dct=True)
    assert e.value.status == UNSUPPORTED and "together" in str(e.value)
    with pytest.raises(mf.MifftError) as e:  # the library's own layout refusals come through a Plan too
        mf.Plan(torch.float32, torch.float32, (4, 8, 7, 1), (4, 8, 7, 1), dctn=True, axes=(1,))
    assert e.value.status == UNSUPPORTED and "odd stride" in str(e.value)


def test_dct_true_keeps_its_rows_only_layout():
    with pytest.raises(mf.MifftError) as e:  # rank 4 under dct=True is still -2
        mf.Plan(torch.float32, torch.float32, (4, 8, 64, 1), (4, 8, 64, 1), dct=True)
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:  # and dct() still refuses a dim that is not the innermost
        mf.dct(torch.zeros(4, 6, 64), dim=1)
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("fn", [mf.dctn, mf.idctn], ids=["dctn", "idctn"])
def test_wrappers_validate_on_the_host(fn):
    x = torch.zeros(3, 8, 64)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(type=3), UNSUPPORTED), (dict(type=1), UNSUPPORTED), (dict(norm="forward"), UNSUPPORTED),
                       (dict(norm=1), UNSUPPORTED), (dict(dim=3), -2), (dict(dim=(1, 1)), -2), (dict(dim=(1, -2)), -2),
                       (dict(out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            fn(x, **kw)
        assert e.value.status == status, kw
    with pytest.raises(mf.MifftError) as e:
        fn(torch.zeros(9))  # rank 1: no batch
    assert e.value.status == -1
    with pytest.raises(mf.MifftError) as e:
        fn(torch.zeros(3, 8, 64, dtype=torch.complex64))
    assert e.value.status == -3
    with pytest.raises(mf.MifftError) as e:
        fn(torch.zeros((2,) * 9), dim=(0, 2, 4, 6, 8))  # more dims than a plan takes
    assert e.value.status == -1
    for ok in (dict(), dict(norm="ortho"), dict(norm="backward"), dict(dim=(1, 2)), dict(dim=-1), dict(dim=(0, 2)), dict(dim=1)):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            fn(x, **ok)
        assert e.value.status == -10, ok
    # nothing to transform: a converted copy, with no device at all
    for dim in ((), ):
        y = fn(x, dim=dim, out_dtype=torch.float64)
        assert y.dtype == torch.float64 and y.shape == x.shape and y.data_ptr() != x.data_ptr()
    y = fn(torch.ones(3, 1, 1), dim=(1, 2))
    assert torch.equal(y, torch.ones(3, 1, 1))
