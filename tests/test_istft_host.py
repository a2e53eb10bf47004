"""Inverse STFT plans (MIFFT_FLAG_ISTFT): the ABI constants, every refusal that needs no device -- the C library's checks run
before it looks for a HIP device, the Python checks before any device context is created -- the walk of the launch as host
arithmetic (istft_schedule), and the fp64 reference of tests/test_gpu_istft.py against torch.istft on the CPU."""
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

ISTFT, STFT, REFLECT, ZEROS = 0x4000, 32, 64, 128
UNSUPPORTED, BAD_DIM, BAD_COMPONENTS, BAD_DTYPE, BAD_BASES, TOO_LARGE, NO_DEVICE = -15, -2, -3, -4, -5, -9, -10


def HOP(h):
    return h << 16


def words(values):
    return [w for v in values for w in struct.unpack("<2I", struct.pack("<d", float(v)))]


def hann(n):  # periodic, as torch.hann_window
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def hamming(n):  # periodic, as torch.hamming_window
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / n)


def test_flag_is_declared():
    assert re.search(r"#define\s+MIFFT_FLAG_ISTFT\s+0x4000u\b", open(os.path.join(ROOT, "include", "mifft.h")).read())
    assert re.search(r"MIFFT_FLAG_ISTFT\b", open(os.path.join(ROOT, "include", "mifft.hpp")).read())
    assert mf.FLAG_ISTFT == api.FLAG_ISTFT == ISTFT
    assert ISTFT & (api.FLAG_KEEP_MASK | api.FLAG_STFT_HOP_MASK | STFT | REFLECT | ZEROS | 31) == 0
    assert len(_lib.EXPORTS) == 21  # (the request travels through mifft_plan_create[_slab])


def _create(dims, *, comps=2, inverse=True, in_dtype=0, out_dtype=0, flags=ISTFT | HOP(4), batch=3, flat=None, lens=None):
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


# dims = {T, F, n}: 10 frames of 64 every 4 cover L = 100 samples
OK = [100, 10, 64]


def test_c_abi_refuses_before_looking_for_a_device():
    inf = [0, 0x7FF00000]
    for kw, status, word in (
            (dict(dims=OK, flags=ISTFT | STFT | HOP(4)), UNSUPPORTED, "MIFFT_FLAG_STFT"),     # both mode bits
            (dict(dims=[1000, 64], flags=ISTFT | STFT | HOP(4), inverse=False, comps=1), UNSUPPORTED, "MIFFT_FLAG_STFT"),
            (dict(dims=OK, inverse=False), UNSUPPORTED, "inverse = 0"),
            (dict(dims=[100, 64]), UNSUPPORTED, "ndim"),
            (dict(dims=[100, 10, 64, 8]), UNSUPPORTED, "ndim"),
            (dict(dims=OK, flags=ISTFT), UNSUPPORTED, "hop 0"),
            (dict(dims=OK, flags=ISTFT | HOP(65)), UNSUPPORTED, "gaps"),                      # hop = n + 1
            (dict(dims=OK, flags=ISTFT | HOP(4) | REFLECT | ZEROS), UNSUPPORTED, "both centre bits"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | 1), UNSUPPORTED, "FAITHFUL"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | 2), UNSUPPORTED, "HALF_SPECTRUM"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | 4), UNSUPPORTED, "MIFFT_FLAG_DCT"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | 8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | 16), UNSUPPORTED, "MIFFT_FLAG_DCT_ND"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | (1 << 8)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=OK, flags=ISTFT | HOP(4) | (1 << 10)), UNSUPPORTED, "KEEP_DIM"),
            (dict(dims=[100, 10, 63]), UNSUPPORTED, "odd"),
            (dict(dims=[20, 10, 6], flags=ISTFT | HOP(2)), UNSUPPORTED, "8 points"),
            (dict(dims=[1000, 10, 2 * 37 * 4]), UNSUPPORTED, "prime factor above 32"),
            (dict(dims=[40000, 3, 32768]), UNSUPPORTED, "16384"),
            (dict(dims=[40000, 3, 16384], in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),
            (dict(dims=OK, comps=1), BAD_COMPONENTS, "in_components"),
            (dict(dims=OK, in_dtype=0, out_dtype=1), BAD_DTYPE, "in_dtype"),
            (dict(dims=OK, in_dtype=2), BAD_DTYPE, "in_dtype"),
            (dict(dims=[101, 10, 64]), BAD_DIM, "zero-padded"),                               # T = L + 1, uncentred
            (dict(dims=[69, 10, 64], flags=ISTFT | HOP(4) | REFLECT), BAD_DIM, "zero-padded"),  # T = L - c + 1, centred
            (dict(dims=[0, 10, 64]), BAD_DIM, ""),
            (dict(dims=[1, 10, 64]), BAD_DIM, "size 1"),                                      # (the rule of every plan)
            (dict(dims=[100, 0, 64]), BAD_DIM, ""),
            (dict(dims=[1 << 20, (1 << 26) // 64 + 1, 64], flags=ISTFT | HOP(64)), TOO_LARGE, "2^26"),   # L = 2^26 + 64
            (dict(dims=[1 << 20, 1 << 27, 64], flags=ISTFT | HOP(1)), TOO_LARGE, "2^26"),
            (dict(dims=OK, flat=[0] * 126, lens=[126, 0, 0]), BAD_BASES, "bases_len[0]"),     # 2 n - 2 words
            (dict(dims=OK, flat=[0] * 129, lens=[129, 0, 0]), BAD_BASES, "bases_len[0]"),
            (dict(dims=OK, flat=words(hamming(64)) + [8], lens=[128, 1, 0]), BAD_BASES, "bases_len[1]"),
            (dict(dims=OK, flat=words(hamming(64)) + inf, lens=[130, 0, 0]), BAD_BASES, "gain"),
            (dict(dims=OK, flat=inf + words(hamming(64))[2:], lens=[128, 0, 0]), BAD_BASES, "not finite"),
            (dict(dims=OK, flat=[3], lens=[0, 0, 1]), BAD_BASES, "multiply"),
            # flags that carry neither mode bit keep their wording
            (dict(dims=OK, flags=HOP(4)), UNSUPPORTED, "without MIFFT_FLAG_STFT"),
            (dict(dims=OK, flags=REFLECT), UNSUPPORTED, "without MIFFT_FLAG_STFT"),
            # ... and so does the forward bit with inverse = 1
            (dict(dims=[1000, 64], flags=STFT | HOP(4), comps=1), UNSUPPORTED, "the inverse STFT is not routed"),
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw, rc, why)


def test_windows_without_overlap_add_are_refused():
    """NOLA: a periodic Hann window starts at zero, so with hop == n and no centring output sample 0 (and every 16th) has a zero
    envelope; torch.istft raises for the same request."""
    n = 16
    w = hann(n)
    rc, why = _create(dims=[n * 5, 5, n], flags=ISTFT | HOP(n), flat=words(w), lens=[2 * n, 0, 0])
    assert rc == UNSUPPORTED and "overlap-add" in why, (rc, why)
    with pytest.raises(RuntimeError):
        torch.istft(torch.ones(n // 2 + 1, 5, dtype=torch.complex128), n, hop_length=n, window=torch.from_numpy(w), center=False)
    # hop 4, uncentred: only the very first sample is bare
    rc, why = _create(dims=[n + 4 * 4, 5, n], flags=ISTFT | HOP(4), flat=words(w), lens=[2 * n, 0, 0])
    assert rc == UNSUPPORTED and "overlap-add" in why and "sample 0" in why, (rc, why)
    if not torch.cuda.is_available():  # the same window centred: the bare samples are trimmed
        rc, why = _create(dims=[4 * 4, 5, n], flags=ISTFT | HOP(4) | REFLECT, flat=words(w), lens=[2 * n, 0, 0])
        assert rc == NO_DEVICE, (rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    one = words([1.0])
    for kw in (dict(dims=OK),
               dict(dims=[64, 1, 64]),                                               # one frame
               dict(dims=[2, 1, 64]),
               dict(dims=[640, 10, 64], flags=ISTFT | HOP(64)),                      # hop == n: no carry
               dict(dims=[68, 10, 64], flags=ISTFT | HOP(4) | REFLECT),              # T = L - c
               dict(dims=[68, 10, 64], flags=ISTFT | HOP(4) | ZEROS),
               dict(dims=[6400, 41, 400], flags=ISTFT | HOP(160) | REFLECT, flat=words(hann(400)), lens=[800, 0, 0]),
               dict(dims=[16384 * 2, 5, 16384], flags=ISTFT | HOP(4096)),
               dict(dims=[8192 * 2, 5, 8192], flags=ISTFT | HOP(2048), in_dtype=1, out_dtype=1),
               dict(dims=[1 << 26, (1 << 26) // 64, 64], flags=ISTFT | HOP(64), batch=1),   # L = 2^26
               dict(dims=OK, flat=one * 64, lens=[128, 0, 0]),                       # a window, default radices
               dict(dims=OK, flat=one * 64 + words([8.0]), lens=[130, 0, 0]),        # 2 n + 2 words: window and gain
               dict(dims=OK, flat=one * 64 + words([8.0]) + [8, 8], lens=[130, 0, 2]),
               dict(dims=OK, flat=[2], lens=[0, 0, 1]),                              # radices alone
               dict(dims=OK, flat=[0], lens=[0, 0, 0])):                             # neither
        rc, why = _create(**kw)
        assert rc == NO_DEVICE, (kw, rc, why)
    # MIFFT_FLAG_STFT is untouched
    rc, why = _create(dims=[1000, 64], flags=STFT | HOP(4), comps=1, inverse=False)
    assert rc == NO_DEVICE, (rc, why)


def test_without_runtime_specialisation_an_istft_plan_is_refused():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process): no precompiled instances exist."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "h = ctypes.c_void_p(); d = (ctypes.c_int64 * 3)(4000, 13, 1024)\n"
            "rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 3, d, 4, 2, 1, None, None, 0x4000 | (256 << 16))\n"
            "print(rc, L.mifft_last_error().decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, r.stdout


@pytest.mark.parametrize("F,n,hop,center", [
    (29, 16, 3, True), (29, 16, 3, False), (7, 16, 16, False), (1, 16, 4, False), (2, 64, 1, False), (9, 30, 7, True),
    (41, 400, 160, True), (33, 1024, 256, True), (5, 16384, 4096, True), (3001, 400, 160, True),
])
def test_istft_length_agrees_with_torch(F, n, hop, center):
    y = torch.istft(torch.zeros(n // 2 + 1, F, dtype=torch.complex64), n, hop_length=hop, center=center,
                    window=torch.ones(n))
    assert mf.istft_length(F, n, hop, center) == y.shape[-1]


@pytest.mark.parametrize("tile,tiles_per_entry,entries,grid,n,hop", [
    (64, 1, 5, 1, 16, 3), (64, 1, 5, 5, 16, 3), (8, 5, 7, 4, 1024, 256), (64, 5, 2, 3, 128, 1), (64, 5, 2, 10, 128, 1),
    (20, 3, 11, 8, 400, 160), (1, 5, 3, 4, 16384, 4096), (1, 5, 3, 15, 16384, 16384), (4, 9, 100, 256, 1024, 1),
])
def test_schedule_invariants(tile, tiles_per_entry, entries, grid, n, hop):
    frames = tiles_per_entry * tile - (tile // 2)   # a ragged last tile
    n_tiles = tiles_per_entry * entries
    runs = api._istft_schedule(tile, n_tiles, grid, frames, n, hop)
    assert len(runs) == grid
    pos = 0
    K = -(-n // hop)
    for first, length, warm in runs:
        assert first == pos and length >= 1
        pos += length
        g = first % tiles_per_entry
        assert warm == min(g, -(-(K - 1) // tile))
        if g == 0:
            assert warm == 0
        assert first - warm >= (first // tiles_per_entry) * tiles_per_entry  # the warm-up stays inside the entry
    assert pos == n_tiles
    lengths = [r[1] for r in runs]
    assert max(lengths) - min(lengths) <= 1 and lengths == sorted(lengths, reverse=True)
    if hop == n:
        assert all(r[2] == 0 for r in runs)


def test_schedule_is_for_istft_plans_only():
    class NotAPlan:
        istft = False
    with pytest.raises(mf.MifftError) as e:
        mf.istft_schedule(NotAPlan())
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("in_shape,out_shape,kw,status", [
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4), None),                       # (valid: reaches the device)
    ((4, 10, 33, 2), (4, 68, 1), dict(istft_hop=4, stft_center=True), None),
    ((4, 10, 33, 2), (4, 68, 1), dict(istft_hop=4, stft_center="constant"), None),
    ((4, 1, 33, 2), (4, 64, 1), dict(istft_hop=4), None),
    ((4, 10, 33, 2), (4, 100, 1), dict(flags=ISTFT | HOP(4)), None),              # the flag bits are the same request
    ((4, 10, 33, 2), (4, 101, 1), dict(istft_hop=4), -2),
    ((4, 10, 33, 2), (4, 69, 1), dict(istft_hop=4, stft_center=True), -2),
    ((4, 10, 33, 2), (4, 101, 1), dict(flags=ISTFT | HOP(4)), -2),
    ((4, 10, 33, 2), (4, 69, 1), dict(flags=ISTFT | HOP(4) | REFLECT), -2),
    ((4, 10, 33, 2), (5, 100, 1), dict(istft_hop=4), -2),
    ((4, 10, 33, 1), (4, 100, 1), dict(istft_hop=4), -3),
    ((4, 10, 33, 2), (4, 100, 2), dict(istft_hop=4), -3),
    ((4, 330, 2), (4, 100, 1), dict(istft_hop=4), -1),
    ((4, 10, 4, 2), (4, 20, 1), dict(istft_hop=2), UNSUPPORTED),                  # n = 6
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=65), UNSUPPORTED),               # hop > n
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=70000), UNSUPPORTED),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, stft_center="edge"), UNSUPPORTED),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, stft_window=[1.0] * 63), -5),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, axes=(1,)), UNSUPPORTED),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, bases=[[2], [], [2]]), -5),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, bases=[[2]]), -7),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, dct=True), UNSUPPORTED),      # another mode: the library refuses the pair
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, stft_hop=4), UNSUPPORTED),
    ((4, 10, 33, 2), (4, 100, 1), dict(istft_hop=4, istft_gain=float("inf")), -5),
    ((4, 5, 9, 2), (4, 80, 1), dict(istft_hop=16, stft_window=hann(16)), UNSUPPORTED),   # NOLA
])
def test_python_layout_validation(in_shape, out_shape, kw, status):
    if status is None:
        if torch.cuda.is_available():
            pytest.skip("valid layout: planned on the device by the GPU tests")
        status = NO_DEVICE
    with pytest.raises(mf.MifftError) as e:
        mf.Plan(torch.float32, torch.float32, in_shape, out_shape, **kw)
    assert e.value.status == status, str(e.value)


def test_plan_istft_validates_before_device_work():
    for args, kw, status in (
            ((torch.float32, 4, 10, 63, 16), {}, UNSUPPORTED),
            ((torch.float32, 4, 10, 6, 2), {}, UNSUPPORTED),
            ((torch.float32, 4, 10, 64, 0), {}, UNSUPPORTED),
            ((torch.float32, 4, 10, 64, 65), {}, UNSUPPORTED),
            ((torch.float32, 4, 10, 64, 65536), {}, UNSUPPORTED),
            ((torch.float32, 4, 0, 64, 16), {}, -2),
            ((torch.float32, 4, 10, 64, 16), dict(length=209), -2),                       # L = 208
            ((torch.float32, 4, 10, 64, 16), dict(length=177, center=True), -2),          # L - c = 176
            ((torch.float32, 4, 10, 64, 16), dict(length=0), -2),
            ((torch.float32, 4, 10, 64, 16), dict(center="edge"), UNSUPPORTED),
            ((torch.float16, 4, 10, 64, 16), {}, -4),
            ((torch.float32, 4, 10, 64, 16), dict(window=[1.0] * 65), -5),
            ((torch.float32, 4, 10, 64, 16), dict(window=torch.hann_window(32)), -5),
    ):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_istft(*args, **kw)
        assert e.value.status == status, (args, kw, str(e.value))


def test_istft_wrapper_validates_on_the_host():
    X = torch.zeros(3, 33, 10, dtype=torch.complex64)  # (a host tensor: nothing reaches the library)
    for kw, status in ((dict(onesided=False), UNSUPPORTED), (dict(return_complex=True), UNSUPPORTED),
                       (dict(win_length=65), -2), (dict(win_length=0), -2),
                       (dict(window=torch.ones(63)), -5), (dict(win_length=32, window=torch.ones(64)), -5),
                       (dict(hop_length=0), UNSUPPORTED), (dict(hop_length=65), UNSUPPORTED),
                       (dict(hop_length=1 << 16), UNSUPPORTED),
                       (dict(hop_length=16, length=177), UNSUPPORTED),                    # centred: 176 are covered
                       (dict(hop_length=16, length=209, center=False), UNSUPPORTED),
                       (dict(out_dtype=torch.float16), -4)):
        with pytest.raises(mf.MifftError) as e:
            mf.istft(X, 64, **kw)
        assert e.value.status == status, (kw, str(e.value))
    with pytest.raises(mf.MifftError) as e:
        mf.istft(torch.zeros(3, 32, 10, dtype=torch.complex64), 63)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        mf.istft(torch.zeros(3, 33, 10), 64)
    assert e.value.status == -3
    with pytest.raises(mf.MifftError) as e:
        mf.istft(torch.zeros(3, 32, 10, dtype=torch.complex64), 64)   # 32 bins are not n_fft // 2 + 1
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:
        mf.istft(torch.zeros(33, dtype=torch.complex64), 64)
    assert e.value.status == -1
    for ok in (dict(), dict(hop_length=3), dict(win_length=32), dict(window=torch.hann_window(64)), dict(normalized=True),
               dict(center=False), dict(length=100), dict(onesided=True), dict(win_length=20, window=torch.hann_window(20))):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.istft(X, 64, **ok)
        assert e.value.status == NO_DEVICE, ok


def test_reference_agrees_with_torch_istft():
    """the fp64 reference of the GPU tests (irfft, window, ascending overlap-add, envelope) against torch.istft on the CPU"""
    from istft_reference import SHAPES, istft_reference, spectrogram, window_of
    worst = 0.0
    for (B, F, n, hop, win, centred, length) in SHAPES:
        X = spectrogram(B, F, n, seed=n + hop)
        w = window_of(win, n)
        ref = istft_reference(X, n, hop, w, centred, length)
        got = torch.istft(torch.from_numpy(X).transpose(-1, -2), n, hop_length=hop, center=centred, length=length,
                          window=torch.ones(n, dtype=torch.float64) if w is None else torch.from_numpy(w)).numpy()
        assert got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print("reference against torch.istft: max relative difference", worst)
    assert worst <= 2e-15
