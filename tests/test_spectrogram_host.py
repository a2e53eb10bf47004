"""Spectrogram plans (MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_POWER): the ABI constant and every refusal that needs no device -- the C
library's checks run before it looks for a HIP device, the Python checks before any device context is created or any tensor
allocated."""
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
from hackathon_fft_amd import _lib, api
from conftest import ROOT

STFT, REFLECT, ZEROS, ISTFT, POWER = 32, 64, 128, 0x4000, 0x8000
UNSUPPORTED = -15
N, K = 64, 33


def HOP(h):
    return h << 16


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_flag_is_declared():
    assert re.search(r"#define\s+MIFFT_FLAG_STFT_POWER\s+0x8000u\b", _header("mifft.h"))
    assert re.search(r"MIFFT_FLAG_STFT_POWER\s*==\s*0x8000u", _header("mifft.hpp"))
    assert mf.FLAG_STFT_POWER == api.FLAG_STFT_POWER == POWER
    others = (mf.FLAG_STFT | mf.FLAG_STFT_CENTER_REFLECT | mf.FLAG_STFT_CENTER_ZEROS | api.FLAG_STFT_HOP_MASK | mf.FLAG_ISTFT |
              api.FLAG_KEEP_MASK | mf.FLAG_DCT | mf.FLAG_DCT_ND | mf.FLAG_DCT_ORTHO | api.FLAG_HALF_SPECTRUM |
              api.FLAG_FAITHFUL_STAGES)
    assert POWER & others == 0


def test_export_list_is_unchanged():
    assert len(_lib.EXPORTS) == 21  # (the request travels through mifft_plan_create[_slab])


def _words(values):
    return list(struct.unpack("<%dI" % (2 * len(values)), struct.pack("<%dd" % len(values), *values)))


def _bases(power=2.0, fb=None, window=None, n=N):
    """the first bases entry of a spectrogram plan: window, power, filterbank (K, M) row-major"""
    w = [1.0] * n if window is None else list(window)
    flat = _words(w) + _words([power])
    if fb is not None:
        flat += _words(list(np.asarray(fb, dtype=np.float64).reshape(-1)))
    return flat


def _create(dims, *, comps=1, inverse=False, in_dtype=0, out_dtype=0, flags=STFT | POWER | HOP(4), batch=3, flat=None, lens=None):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    c_flat = None if flat is None else (ctypes.c_uint32 * max(len(flat), 1))(*flat)
    c_len = None if lens is None else (ctypes.c_int32 * len(lens))(*lens)
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, len(dims), c_dims, batch, comps, int(inverse),
                             c_flat, c_len, flags)
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


def _with(flat, **kw):
    return dict(dims=[1000, N], flat=flat, lens=[len(flat), 0], **kw)


def test_c_abi_refuses_before_looking_for_a_device():
    ok = _bases()
    nan, inf = float("nan"), float("inf")
    fb5 = np.ones((K, 5))
    bad_fb = fb5.copy()
    bad_fb[7, 3] = inf
    for kw, status, word in (
            # the bit without its mode, or with the other mode
            (dict(dims=[1000, N], flags=POWER), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (dict(dims=[1000, N], flags=POWER | HOP(4)), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (_with(ok, flags=POWER | HOP(4)), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (dict(dims=[1000, 4, N], flags=ISTFT | POWER | HOP(16), inverse=True, comps=2), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            # the power has to be given
            (dict(dims=[1000, N]), -5, "bases_len[0]"),                                       # NULL bases
            (_with([0] * 128), -5, "bases_len[0]"),                                           # a window alone
            (_with([0] * 129), -5, "bases_len[0]"),
            (_with(ok + [0]), -5, "bases_len[0]"),                                            # 130 + 1
            (_with(ok + [0] * (2 * K * 2 + 2)), -5, "bases_len[0]"),                          # 130 + 2 * 33 * M + 2
            (_with(ok + [0] * (2 * K * 5 - 2)), -5, "bases_len[0]"),
            (dict(dims=[1000, N], flat=[0], lens=[0, 0]), -5, "bases_len[0]"),
            # 1 or 2, nothing else
            (_with(_bases(0.0)), -5, "power"),
            (_with(_bases(3.0)), -5, "power"),
            (_with(_bases(0.5)), -5, "power"),
            (_with(_bases(nan)), -5, "power"),
            (_with(_bases(-2.0)), -5, "power"),
            (_with(_bases(2.0, fb5, window=[1.0] * 63 + [nan])), -5, "not finite"),
            (_with(_bases(2.0, bad_fb)), -5, "not finite"),
            (_with(_bases(1.0, np.full((K, 1), nan))), -5, "not finite"),
            # every refusal of an STFT plan, with the bit set
            (dict(dims=[1000, 63], flat=ok, lens=[len(ok), 0]), UNSUPPORTED, "odd"),
            (dict(dims=[63, N], flat=ok, lens=[len(ok), 0]), UNSUPPORTED, "T < n"),
            (_with(ok, flags=STFT | POWER | HOP(4) | REFLECT | ZEROS), UNSUPPORTED, "both centre bits"),
            (_with(ok, comps=2), -3, "in_components"),
            (_with(ok, flags=STFT | POWER), UNSUPPORTED, "hop 0"),
            (_with(ok, flags=STFT | POWER | HOP(4) | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (_with(ok, inverse=True), UNSUPPORTED, "the inverse STFT is not routed"),
            (_with(ok, in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(dims=[32, N], flat=ok, lens=[len(ok), 0], flags=STFT | POWER | HOP(4) | REFLECT), UNSUPPORTED, "one reflection"),
            (dict(dims=[1000, N], flat=ok + [3], lens=[len(ok), 1]), -5, "multiply"),         # radices that do not make 64
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw.get("dims"), kw.get("flags"), kw.get("lens"), rc, why)


def test_more_bands_than_the_limit_are_refused():
    """n = 8: K = 5, so 2 M K words stay far below what an int32 bases_len holds"""
    assert re.search(r"#define\s+MIFFT_STFT_MAX_BANDS\s+32768\b", _header("mifft.h"))
    M = 32769
    flat = _words([1.0] * 8) + _words([2.0]) + [0] * (2 * 5 * M)
    rc, why = _create(dims=[1000, 8], flat=flat, lens=[len(flat), 0])
    assert rc == -9 and "MIFFT_STFT_MAX_BANDS" in why, (rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    rng = np.random.default_rng(3)
    dense = rng.standard_normal((K, 5))
    holed = dense.copy()
    holed[:, 2] = 0.0                                                                          # an all-zero column
    for kw in (_with(_bases(2.0)), _with(_bases(1.0)),                                         # M = 0
               _with(_bases(2.0, window=np.hanning(N))),
               _with(_bases(2.0, dense)), _with(_bases(1.0, dense)),                           # M = 5, dense and signed
               _with(_bases(2.0, holed)),
               _with(_bases(2.0, np.zeros((K, 1)))),
               _with(_bases(2.0, dense), flags=STFT | POWER | HOP(160) | REFLECT),
               dict(dims=[1000, N], flat=_bases(2.0, dense) + [8, 8], lens=[len(_bases(2.0, dense)), 2]),
               dict(dims=[40000, 16384], flat=_bases(2.0, np.ones((8193, 3)), n=16384),
                    lens=[len(_bases(2.0, np.ones((8193, 3)), n=16384)), 0]),
               dict(dims=[40000, 8192], in_dtype=1, out_dtype=1, flat=_bases(1.0, n=8192), lens=[2 * 8192 + 2, 0])):
        rc, why = _create(**kw)
        assert rc == -10, (kw.get("dims"), kw.get("lens"), rc, why)


def test_without_runtime_specialisation_a_spectrogram_plan_is_refused():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process), as for every STFT plan"""
    code = ("import ctypes, struct, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "h = ctypes.c_void_p(); d = (ctypes.c_int64 * 2)(4000, 1024)\n"
            "w = list(struct.unpack('<2050I', struct.pack('<1025d', *([1.0] * 1024 + [2.0]))))\n"
            "flat = (ctypes.c_uint32 * 2050)(*w); lens = (ctypes.c_int32 * 2)(2050, 0)\n"
            "rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, d, 4, 1, 0, flat, lens, 32 | 0x8000 | (256 << 16))\n"
            "print(rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, r.stdout


FB5 = np.ones((K, 5))


@pytest.mark.parametrize("in_shape,out_shape,kw,status", [
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=2), None),                 # (valid: reaches the device)
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=1.0), None),
    ((4, 1000, 1), (4, 251, 5, 1), dict(stft_hop=4, stft_center="reflect", stft_power=2, stft_fb=FB5), None),
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, stft_power=2), -3),                   # a complex-shaped out
    ((4, 1000, 1), (4, 235, 33, 3), dict(stft_hop=4, stft_power=2), -3),                   # a wrong last dim
    ((4, 1000, 1), (4, 235, 5, 2), dict(stft_hop=4, stft_power=2, stft_fb=FB5), -3),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4), -3),                                 # real-shaped, no power: as ever
    ((4, 1000, 1), (4, 235, 33), dict(stft_hop=4, stft_power=2), -1),
    ((4, 1000, 1), (4, 251, 33, 1), dict(stft_hop=4, stft_power=2), -2),                   # the uncentred count is 235
    ((4, 1000, 1), (5, 235, 33, 1), dict(stft_hop=4, stft_power=2), -2),
    ((4, 1000, 1), (4, 235, 6, 1), dict(stft_hop=4, stft_power=2, stft_fb=FB5), -2),       # 5 bands, not 6
    ((4, 1000, 1), (4, 235, 5, 1), dict(stft_hop=4, stft_power=2, stft_fb=FB5.T), -2),     # an (M, K) filterbank
    ((4, 1000, 1), (4, 235, 5, 1), dict(stft_hop=4, stft_power=2, stft_fb=np.ones(33)), -2),
    ((4, 1000, 1), (4, 235, 5, 1), dict(stft_hop=4, stft_power=2, stft_fb=FB5 * (1 + 1j)), -3),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=3), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=0), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=0.5), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power="2"), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 5, 2), dict(stft_hop=4, stft_fb=FB5), UNSUPPORTED),            # a filterbank without a power
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=2, stft_window=[1.0] * 63), -5),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4, stft_power=2, axes=(1,)), UNSUPPORTED),
    ((4, 32, 1), (4, 1, 33, 1), dict(stft_hop=4, stft_power=2), UNSUPPORTED),              # T < n
])
def test_python_layout_validation(in_shape, out_shape, kw, status):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        status = -10
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, **kw)
    assert e.value.status == status, str(e.value)


def test_plan_spectrogram_validates_before_device_work():
    fb = np.ones((K, 5))
    for args, kw, status in (
            ((torch.float32, 4, 1000, 63, 16), {}, UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 0), {}, UNSUPPORTED),
            ((torch.float32, 4, 32, 64, 16), {}, UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(center=True), UNSUPPORTED),
            ((torch.float16, 4, 1000, 64, 16), {}, -4),
            ((torch.float32, 4, 1000, 64, 16), dict(window=[1.0] * 65), -5),
            ((torch.float32, 4, 1000, 64, 16), dict(power=None), UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(power=3), UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(power=1.5), UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(fb=fb.T), -2),                         # librosa's orientation
            ((torch.float32, 4, 1000, 64, 16), dict(fb=np.ones((32, 5))), -2),
            ((torch.float32, 4, 1000, 64, 16), dict(fb=np.ones((K, 0))), -2),
            ((torch.float32, 4, 1000, 64, 16), dict(fb=np.ones((K, K)).T[:5]), -2),        # (5, 33) of a square one
    ):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_spectrogram(*args, **kw)
        assert e.value.status == status, (args, kw, str(e.value))
    if not torch.cuda.is_available():
        for kw in ({}, dict(power=1), dict(power=1.0), dict(center="reflect", fb=fb), dict(fb=torch.from_numpy(fb).float()),
                   dict(window=np.hanning(64), fb=[[1.0, -2.0]] * K), dict(power=2, fb=np.ones((K, K)))):
            with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device
                mf.plan_spectrogram(torch.float32, 4, 1000, 64, 16, **kw)
            assert e.value.status == -10, kw


def test_spectrogram_wrapper_validates_on_the_host():
    x = torch.zeros(3, 1000)  # (a host tensor: nothing reaches the library)
    fb = torch.ones(K, 5)
    for kw, status in ((dict(power=None), UNSUPPORTED), (dict(power=3), UNSUPPORTED), (dict(power=0), UNSUPPORTED),
                       (dict(onesided=False), UNSUPPORTED), (dict(pad_mode="replicate"), UNSUPPORTED),
                       (dict(pad_mode="circular"), UNSUPPORTED), (dict(win_length=65), -2),
                       (dict(window=torch.ones(63)), -5), (dict(hop_length=0), UNSUPPORTED),
                       (dict(out_dtype=torch.float16), -4),
                       (dict(fb=fb.T), -2), (dict(fb=torch.ones(K)), -2), (dict(fb=torch.ones(K + 1, 5)), -2)):
        with pytest.raises(mf.MifftError) as e:
            mf.spectrogram(x, 64, **kw)
        assert e.value.status == status, (kw, str(e.value))
    with pytest.raises(mf.MifftError) as e:
        mf.spectrogram(torch.zeros(3, 1000, dtype=torch.complex64), 64)
    assert e.value.status == -3
    with pytest.raises(mf.MifftError) as e:
        mf.spectrogram(x, 63)
    assert e.value.status == UNSUPPORTED
    for ok in (dict(), dict(power=1), dict(power=1.0, fb=fb), dict(fb=fb.numpy()), dict(normalized=True, win_length=32),
               dict(center=False, fb=fb.double()), dict(pad_mode="constant")):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.spectrogram(x, 64, **ok)
        assert e.value.status == -10, ok
    # the complex STFT wrapper is what it was
    with pytest.raises(mf.MifftError) as e:
        mf.stft(x, 64)
    assert e.value.status == -10
