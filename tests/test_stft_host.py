"""STFT plans (MIFFT_FLAG_STFT): the ABI constants and every refusal that needs no device -- the C library's checks run before
it looks for a HIP device, the Python checks before any device context is created or any tensor allocated."""
import ctypes
import math
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

STFT, REFLECT, ZEROS = 32, 64, 128
UNSUPPORTED = -15


def HOP(h):
    return h << 16


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_flags_are_declared():
    h = _header("mifft.h")
    assert re.search(r"#define\s+MIFFT_FLAG_STFT\s+32u\b", h)
    assert re.search(r"#define\s+MIFFT_FLAG_STFT_CENTER_REFLECT\s+64u\b", h)
    assert re.search(r"#define\s+MIFFT_FLAG_STFT_CENTER_ZEROS\s+128u\b", h)
    assert re.search(r"#define\s+MIFFT_FLAG_STFT_HOP\(h\)\s+\(\(uint32_t\)\(h\)\s*<<\s*16\)", h)
    assert re.search(r"#define\s+MIFFT_FLAG_STFT_HOP_MASK\s+0xFFFF0000u\b", h)
    hpp = _header("mifft.hpp")
    for name in ("MIFFT_FLAG_STFT", "MIFFT_FLAG_STFT_CENTER_REFLECT", "MIFFT_FLAG_STFT_CENTER_ZEROS", "MIFFT_FLAG_STFT_HOP",
                 "MIFFT_FLAG_STFT_HOP_MASK"):
        assert re.search(name + r"\b", hpp), name
    assert mf.FLAG_STFT == api.FLAG_STFT == STFT
    assert mf.FLAG_STFT_CENTER_REFLECT == api.FLAG_STFT_CENTER_REFLECT == REFLECT
    assert mf.FLAG_STFT_CENTER_ZEROS == api.FLAG_STFT_CENTER_ZEROS == ZEROS
    assert mf.FLAG_STFT_HOP(1) == 1 << 16 and mf.FLAG_STFT_HOP(65535) == api.FLAG_STFT_HOP_MASK == 0xFFFF0000
    for bad in (0, 65536, -1):
        with pytest.raises(mf.MifftError) as e:
            mf.FLAG_STFT_HOP(bad)
        assert e.value.status == UNSUPPORTED


def test_export_list_is_unchanged():
    assert len(_lib.EXPORTS) == 21  # (the request travels through mifft_plan_create[_slab])
    assert _lib.lib().mifft_version() == 1


def _create(dims, *, comps=1, inverse=False, in_dtype=0, out_dtype=0, flags=STFT | HOP(4), batch=3, flat=None, lens=None):
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


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            (dict(dims=[1000, 64], flags=HOP(4)), UNSUPPORTED, "without MIFFT_FLAG_STFT"),          # a hop field without the flag
            (dict(dims=[1000, 64], flags=STFT), UNSUPPORTED, "hop 0"),
            (dict(dims=[1000, 64], flags=REFLECT), UNSUPPORTED, "without MIFFT_FLAG_STFT"),          # a centre bit without it
            (dict(dims=[1000, 64], flags=ZEROS), UNSUPPORTED, "without MIFFT_FLAG_STFT"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | REFLECT | ZEROS), UNSUPPORTED, "both centre bits"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | 1), UNSUPPORTED, "FAITHFUL"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | 4), UNSUPPORTED, "MIFFT_FLAG_DCT"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | 16), UNSUPPORTED, "MIFFT_FLAG_DCT_ND"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | 8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | (1 << 8)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[1000, 64], flags=STFT | HOP(4) | (1 << 9)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[64]), UNSUPPORTED, "ndim"),
            (dict(dims=[8, 1000, 64]), UNSUPPORTED, "ndim"),
            (dict(dims=[1000, 64], inverse=True), UNSUPPORTED, "the inverse STFT is not routed"),
            (dict(dims=[1000, 63]), UNSUPPORTED, "odd"),
            (dict(dims=[1000, 6]), UNSUPPORTED, "8 points"),
            (dict(dims=[40000, 32768]), UNSUPPORTED, "16384"),
            (dict(dims=[40000, 16384], in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),      # fp64 rows end at 12288 points (a 96-KiB tile)
            (dict(dims=[1000, 2 * 37 * 4]), UNSUPPORTED, "prime factor above 32"),
            (dict(dims=[63, 64]), UNSUPPORTED, "T < n"),                                        # uncentred, shorter than a frame
            (dict(dims=[32, 64], flags=STFT | HOP(4) | REFLECT), UNSUPPORTED, "one reflection"),  # n / 2 = 32 > T - 1 = 31
            (dict(dims=[1000, 64], in_dtype=2), -4, "in_dtype"),                                # uint8 signals
            (dict(dims=[1000, 64], in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(dims=[1000, 64], comps=2), -3, "in_components"),
            (dict(dims=[1 << 31, 64]), -9, "2^31"),
            (dict(dims=[1000, 64], flat=[0] * 64, lens=[64, 0]), -5, "bases_len[0]"),           # neither 0 nor 2 n = 128 words
            (dict(dims=[1000, 64], flat=[0] * 129, lens=[129, 0]), -5, "bases_len[0]"),
            (dict(dims=[1000, 64], flat=[0, 0x7FF00000] + [0] * 126, lens=[128, 0]), -5, "not finite"),   # w[0] = inf
            (dict(dims=[1000, 64], flat=[0] * 126 + [1, 0x7FF80000], lens=[128, 0]), -5, "not finite"),   # w[63] = nan
            (dict(dims=[1000, 64], flat=[3], lens=[0, 1]), -5, "multiply"),                     # radices that do not make 64
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw, rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    one = list(struct.unpack("<2I", struct.pack("<d", 1.0)))
    for kw in (dict(dims=[1000, 64]),
               dict(dims=[64, 64]),                                              # T = n: one frame
               dict(dims=[33, 64], flags=STFT | HOP(4) | REFLECT),               # n / 2 = T - 1
               dict(dims=[2, 64], flags=STFT | HOP(65535) | ZEROS),              # zeros need no reach
               dict(dims=[480000, 400], flags=STFT | HOP(160) | REFLECT),
               dict(dims=[40000, 16384]),
               dict(dims=[40000, 8192], in_dtype=1, out_dtype=1),
               dict(dims=[1000, 64], flat=one * 64, lens=[128, 0]),              # a window, default radices
               dict(dims=[1000, 64], flat=one * 64 + [8, 8], lens=[128, 2]),     # a window and radices
               dict(dims=[1000, 64], flat=[2], lens=[0, 1]),                     # radices alone
               dict(dims=[1000, 64], flat=[0], lens=[0, 0])):                    # neither
        rc, why = _create(**kw)
        assert rc == -10, (kw, rc, why)


def test_without_runtime_specialisation_an_stft_plan_is_refused():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process): no precompiled STFT instances exist."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "h = ctypes.c_void_p(); d = (ctypes.c_int64 * 2)(4000, 1024)\n"
            "rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, d, 4, 1, 0, None, None, 32 | (256 << 16))\n"
            "print(rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, r.stdout


@pytest.mark.parametrize("in_shape,out_shape,kw,status", [
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4), None),                    # (valid: reaches the device)
    ((4, 1000, 1), (4, 251, 33, 2), dict(stft_hop=4, stft_center="reflect"), None),
    ((4, 1000, 1), (4, 251, 33, 2), dict(stft_hop=4), -2),                      # the uncentred count is 235
    ((4, 1000, 1), (5, 235, 33, 2), dict(stft_hop=4), -2),
    ((4, 1000, 2), (4, 235, 33, 2), dict(stft_hop=4), -3),
    ((4, 1000, 1), (4, 235, 33, 1), dict(stft_hop=4), -3),
    ((4, 1000, 1), (4, 235 * 33, 2), dict(stft_hop=4), -1),
    ((4, 1000, 1), (4, 249, 4, 2), dict(stft_hop=4), UNSUPPORTED),              # n = 6
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=70000), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, stft_center="edge"), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, stft_center=True), UNSUPPORTED),
    ((4, 32, 1), (4, 9, 33, 2), dict(stft_hop=4, stft_center="reflect"), UNSUPPORTED),   # n / 2 > T - 1
    ((4, 32, 1), (4, 1, 33, 2), dict(stft_hop=4), UNSUPPORTED),                 # T < n
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, stft_window=[1.0] * 63), -5),
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, axes=(1,)), UNSUPPORTED),
    ((4, 1000, 1), (4, 235, 33, 2), dict(stft_hop=4, bases=[[2], [2]]), -5),
])
def test_python_layout_validation(in_shape, out_shape, kw, status):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        status = -10
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, **kw)
    assert e.value.status == status, str(e.value)


def test_the_flag_bits_are_the_same_request():
    with pytest.raises(mf.MifftError) as e:  # the frame count of the flags' centring is checked on the host
        mf.Plan(torch.float32, torch.float32, (4, 1000, 1), (4, 235, 33, 2), flags=STFT | HOP(4) | REFLECT)
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:  # another mode beside it: the library refuses the pair, before any device
        mf.Plan(torch.float32, torch.float32, (4, 1000, 1), (4, 235, 33, 2), stft_hop=4, dct=True)
    assert e.value.status == UNSUPPORTED and "MIFFT_FLAG_DCT" in str(e.value)
    with pytest.raises(mf.MifftError) as e:  # without the STFT arguments these layouts are still refused
        mf.Plan(torch.float32, torch.float32, (4, 1000, 1), (4, 235, 33, 2))
    assert e.value.status == -1


def test_plan_stft_validates_before_device_work():
    for args, kw, status in (
            ((torch.float32, 4, 1000, 63, 16), {}, UNSUPPORTED),
            ((torch.float32, 4, 1000, 6, 2), {}, UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 0), {}, UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 65536), {}, UNSUPPORTED),
            ((torch.float32, 4, 32, 64, 16), {}, UNSUPPORTED),                       # T < n, uncentred
            ((torch.float32, 4, 32, 64, 16), dict(center="reflect"), UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(center="edge"), UNSUPPORTED),
            ((torch.float32, 4, 1000, 64, 16), dict(center=True), UNSUPPORTED),
            ((torch.float16, 4, 1000, 64, 16), {}, -4),
            ((torch.float32, 4, 1000, 64, 16), dict(window=[1.0] * 65), -5),          # wrong window length
            ((torch.float32, 4, 1000, 64, 16), dict(window=np.ones((2, 32))), -5),
            ((torch.float32, 4, 1000, 64, 16), dict(window=torch.hann_window(32)), -5),
    ):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_stft(*args, **kw)
        assert e.value.status == status, (args, kw, str(e.value))
    if not torch.cuda.is_available():
        for kw in ({}, dict(center="reflect"), dict(center="constant"), dict(window=torch.hann_window(64)),
                   dict(window=np.hanning(64)), dict(window=[0.5] * 64)):
            with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device
                mf.plan_stft(torch.float32, 4, 1000, 64, 16, **kw)
            assert e.value.status == -10, kw


def test_stft_wrapper_validates_on_the_host():
    x = torch.zeros(3, 1000)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(onesided=False), UNSUPPORTED), (dict(pad_mode="replicate"), UNSUPPORTED),
                       (dict(pad_mode="circular"), UNSUPPORTED), (dict(win_length=65), -2), (dict(win_length=0), -2),
                       (dict(window=torch.ones(63)), -5),                       # not win_length = n_fft values
                       (dict(win_length=32, window=torch.ones(64)), -5),        # not win_length values
                       (dict(hop_length=0), UNSUPPORTED), (dict(hop_length=1 << 16), UNSUPPORTED),
                       (dict(out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            mf.stft(x, 64, **kw)
        assert e.value.status == status, (kw, str(e.value))
    for n_fft in (63, 6):
        with pytest.raises(mf.MifftError) as e:
            mf.stft(x, n_fft)
        assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        mf.stft(torch.zeros(3, 1000, dtype=torch.complex64), 64)
    assert e.value.status == -3
    with pytest.raises(mf.MifftError) as e:  # reflect needs n_fft // 2 <= T - 1
        mf.stft(torch.zeros(3, 32), 64)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:  # uncentred, shorter than one frame
        mf.stft(torch.zeros(3, 32), 64, center=False)
    assert e.value.status == UNSUPPORTED
    for ok in (dict(), dict(hop_length=3), dict(win_length=32), dict(window=torch.hann_window(64)), dict(normalized=True),
               dict(center=False), dict(pad_mode="constant"), dict(win_length=20, window=torch.hann_window(20))):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.stft(x, 64, **ok)
        assert e.value.status == -10, ok


@pytest.mark.parametrize("T,n,hop,center", [
    (100, 16, 3, False), (100, 16, 3, True), (50, 16, 24, False), (64, 8, 1, True), (9, 16, 4, True), (16, 16, 16, False),
    (1000, 400, 160, True), (1000, 400, 160, False), (4000, 686, 100, False), (20000, 8192, 2048, False), (160, 16, 16, False),
    (480000, 400, 160, True), (220500, 1024, 256, True), (17, 16, 5, False),
])
def test_stft_frames_agrees_with_torch(T, n, hop, center):
    y = torch.stft(torch.zeros(T, dtype=torch.float64), n, hop_length=hop, center=center, return_complex=True,
                   window=torch.ones(n, dtype=torch.float64))
    assert mf.stft_frames(T, n, hop, center) == y.shape[-1]
    assert mf.stft_frames(T, n, hop, "reflect" if center else None) == y.shape[-1]


def test_window_words_round_trip_bit_for_bit():
    rng = np.random.default_rng(5)
    w = rng.standard_normal(257)
    w[:6] = [0.0, -0.0, 5e-324, 1.7976931348623157e308, math.pi, -1.0 / 3.0]  # signed zero, a subnormal, the largest
    words = api.window_words(w)
    assert len(words) == 2 * len(w) and all(0 <= v < 1 << 32 for v in words)
    assert words[2:4] == [0, 0x80000000]  # -0.0: low word first
    assert words[4:6] == [1, 0]           # the smallest subnormal
    back = np.array(api.words_window(words), dtype=np.float64)
    assert back.tobytes() == w.astype(np.float64).tobytes()
    for src in (torch.from_numpy(w), list(w)):
        assert api.window_words(src) == words
    # float32 values widen exactly
    w32 = torch.hann_window(64)
    assert np.array_equal(np.array(api.words_window(api.window_words(w32))), w32.double().numpy())
