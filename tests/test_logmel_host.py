"""The log and post stages of a spectrogram plan (the tagged payload, MIFFT_STFT_EXT_TAG) and the host-side generators
melscale_fbanks / create_dct: the ABI constants, every refusal that needs no device, and the generators against their own
mathematical properties.  The C library's checks run before it looks for a HIP device, the Python checks before any device
context is created or any tensor allocated."""
import ctypes
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib, api
from conftest import ROOT
from test_spectrogram_host import HOP, K, N, POWER, REFLECT, STFT, UNSUPPORTED, _bases, _create, _header, _with, _words

TAG_LO, TAG_HI = 0x46465401, 0x7FF84D49
LOG10 = (0.0, 1e-10, math.log10(2.0), 0.0)  # add, amin, a, c


def tagged(power=2.0, fb=None, log=None, post=None, n=N, M=None, Q=None, lg=None, tag=(TAG_LO, TAG_HI), window=None):
    """the first bases entry of the extended payload: w | TAG | power | M | Q | log | add | amin | a | c | fb | post; M, Q and
    log follow the matrices unless given"""
    fb = None if fb is None else np.asarray(fb, dtype=np.float64)
    post = None if post is None else np.asarray(post, dtype=np.float64)
    M = (0 if fb is None else fb.shape[1]) if M is None else M
    Q = (0 if post is None else post.shape[1]) if Q is None else Q
    lg = (0.0 if log is None else 1.0) if lg is None else lg
    flat = _words([1.0] * n if window is None else list(window)) + list(tag)
    flat += _words([power, float(M), float(Q), float(lg)] + list(log or (0.0, 0.0, 0.0, 0.0)))
    for m in (fb, post):
        if m is not None:
            flat += _words(list(m.reshape(-1)))
    return flat


def test_the_tag_is_declared():
    assert re.search(r"#define\s+MIFFT_STFT_EXT_TAG_LO\s+0x46465401u\b", _header("mifft.h"))
    assert re.search(r"#define\s+MIFFT_STFT_EXT_TAG_HI\s+0x7FF84D49u\b", _header("mifft.h"))
    assert re.search(r"MIFFT_STFT_EXT_TAG_LO\s*==\s*0x46465401u", _header("mifft.hpp"))
    assert (mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI) == (api.STFT_EXT_TAG_LO, api.STFT_EXT_TAG_HI) == (TAG_LO, TAG_HI)
    tag = struct.unpack("<d", struct.pack("<II", TAG_LO, TAG_HI))[0]
    assert math.isnan(tag) and struct.pack("<d", tag) == struct.pack("<Q", 0x7FF84D4946465401)
    assert struct.pack("<d", float("nan")) == struct.pack("<Q", 0x7FF8000000000000)  # (the pinned untagged case is another NaN)
    assert len(_lib.EXPORTS) == 21
    assert "No log / dB stage" not in _header("mifft.h")


def test_an_untagged_payload_means_what_it_meant():
    """two of the cases test_spectrogram_host.py pins, as a canary beside the new branch"""
    ok = _bases()
    for kw, status, word in ((_with(ok + [0] * (2 * K * 5 - 2)), -5, "bases_len[0]"),
                             (_with(_bases(float("nan"))), -5, "power"),
                             (_with(_bases(3.0)), -5, "power")):
        rc, why = _create(**kw)
        assert rc == status and word in why, (rc, why)


FB5 = np.random.default_rng(1).uniform(0.1, 1.0, (K, 5))
POST = np.random.default_rng(2).standard_normal((5, 3))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_tagged_request_gets_as_far_as_the_device():
    big = tagged(2.0, np.ones((8193, 3)), LOG10, np.ones((3, 3)), n=16384)
    small = tagged(2.0, np.ones((5, 3)), LOG10, np.eye(3), n=8)
    for kw in (_with(tagged(2.0, None, LOG10)),                                              # log only, per bin
               _with(tagged(1.0, None, (1e-6, 1e-10, math.log(2.0), -3.0))),
               _with(tagged(2.0, FB5, LOG10)),
               _with(tagged(2.0, FB5, None, POST)),
               _with(tagged(2.0, FB5, LOG10, POST)),
               _with(tagged(2.0, FB5, LOG10, POST), flags=STFT | POWER | HOP(160) | REFLECT),
               _with(tagged(2.0)), _with(tagged(2.0, FB5)),                                  # log = 0, Q = 0: the old plans
               _with(tagged(2.0, FB5, (float("nan"),) * 4, POST, lg=0.0)),                   # log = 0: the four are not read
               dict(dims=[1000, N], flat=tagged(2.0, FB5, LOG10, POST) + [8, 8], lens=[len(tagged(2.0, FB5, LOG10, POST)), 2]),
               dict(dims=[40000, 16384], flat=big, lens=[len(big), 0]),
               dict(dims=[1000, 8], flat=small, lens=[len(small), 0]),                       # M = 3 = N - 1: the last .y slot
               dict(dims=[1000, 8], in_dtype=1, out_dtype=1, flat=small, lens=[len(small), 0]),
               _with(tagged(2.0, FB5, (0.0, 1e-50, 1.0, 0.0), POST), in_dtype=1, out_dtype=1)):  # normal in binary64
        rc, why = _create(**kw)
        assert rc == -10, (kw.get("dims"), kw.get("lens"), rc, why)


def test_the_tagged_payload_is_refused_before_looking_for_a_device():
    nan, inf = float("nan"), float("inf")
    ok = tagged(2.0, FB5, LOG10, POST)
    assert len(ok) == 2 * (N + 9 + K * 5 + 5 * 3)
    bad_post = POST.copy()
    bad_post[4, 1] = nan
    bad_fb = FB5.copy()
    bad_fb[3, 2] = inf

    def lg(add=0.0, amin=1e-10, a=1.0, c=0.0):
        return _with(tagged(2.0, FB5, (add, amin, a, c), POST))

    fb8 = np.ones((5, 4))
    m_is_n = tagged(2.0, fb8, LOG10, np.ones((4, 2)), n=8)
    too_many = tagged(2.0, np.ones((5, 3)), None, None, n=8, Q=32769)
    too_many_m = tagged(2.0, None, None, None, n=8, M=32769)
    for kw, status, word in (
            (_with(ok + [0, 0]), -5, "bases_len[0]"),
            (_with(ok[:-2]), -5, "bases_len[0]"),
            (_with(ok[:2 * N + 2]), -5, "bases_len[0]"),                                     # the tag and nothing behind it
            (_with(tagged(2.0, FB5, LOG10, POST, M=4)), -5, "bases_len[0]"),                 # a header that disagrees
            # one bit off the tag: an untagged payload with a NaN for its power, or of a length no M makes
            (_with(tagged(2.0, tag=(TAG_LO ^ 1, TAG_HI)) + [0] * (2 * K - 16)), -5, "power"),
            (_with(tagged(2.0, tag=(TAG_LO, TAG_HI ^ 0x10000)) + [0] * (2 * K - 16)), -5, "power"),
            (_with(tagged(2.0, FB5, LOG10, POST, tag=(TAG_LO ^ 1, TAG_HI))), -5, "bases_len[0]"),
            (_with(tagged(3.0, FB5, LOG10, POST)), -5, "power"),
            (_with(tagged(nan, FB5, LOG10, POST)), -5, "power"),
            (_with(tagged(2.0, FB5, LOG10, POST, lg=2.0)), -5, "header value log"),
            (_with(tagged(2.0, FB5, LOG10, POST, lg=0.5)), -5, "header value log"),
            (_with(tagged(2.0, FB5, LOG10, POST, M=2.5)), -5, "header value M"),
            (_with(tagged(2.0, FB5, LOG10, POST, M=-1.0)), -5, "header value M"),
            (_with(tagged(2.0, FB5, LOG10, POST, M=inf)), -5, "header value M"),
            (_with(tagged(2.0, FB5, LOG10, POST, Q=nan)), -5, "header value Q"),
            (_with(tagged(2.0, FB5, LOG10, POST, Q=1.5)), -5, "header value Q"),
            (lg(amin=0.0), -5, "amin"), (lg(amin=-1e-10), -5, "amin"), (lg(amin=1e-50), -5, "amin"), (lg(amin=inf), -5, "amin"),
            (lg(amin=nan), -5, "amin"),
            (lg(a=0.0), -5, "a of the log stage"), (lg(a=inf), -5, "a of the log stage"),
            (lg(add=-1e-6), -5, "add"), (lg(add=nan), -5, "add"), (lg(c=inf), -5, "c of the log stage"),
            (_with(tagged(2.0, FB5, LOG10, bad_post)), -5, "post weight (4, 1)"),
            (_with(tagged(2.0, bad_fb, LOG10, POST)), -5, "filterbank weight (3, 2)"),
            (_with(tagged(2.0, None, LOG10, window=[1.0] * 63 + [nan])), -5, "window"),
            (_with(tagged(2.0, None, LOG10, np.ones((0, 3)), Q=3)), UNSUPPORTED, "M = 0"),
            (dict(dims=[1000, 8], flat=m_is_n, lens=[len(m_is_n), 0]), UNSUPPORTED, "n / 2 - 1"),
            (dict(dims=[1000, 8], flat=too_many, lens=[len(too_many), 0]), -9, "Q = 32769"),
            (dict(dims=[1000, 8], flat=too_many_m, lens=[len(too_many_m), 0]), -9, "M = 32769"),
            # every refusal of an STFT plan still comes first
            (_with(ok, flags=STFT | POWER), UNSUPPORTED, "hop 0"),
            (_with(ok, comps=2), -3, "in_components"),
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw.get("lens"), rc, status, word, why)


def test_without_runtime_specialisation_a_tagged_plan_is_refused():
    """MIFFT_JIT=0 (fresh process: the switch is read once per process), as for every STFT plan"""
    flat = tagged(2.0, np.ones((513, 4)), LOG10, np.ones((4, 2)), n=1024)
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "w = %r\n"
            "h = ctypes.c_void_p(); d = (ctypes.c_int64 * 2)(4000, 1024)\n"
            "flat = (ctypes.c_uint32 * len(w))(*w); lens = (ctypes.c_int32 * 2)(len(w), 0)\n"
            "rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, d, 4, 1, 0, flat, lens, 32 | 0x8000 | (256 << 16))\n"
            "print(rc, L.mifft_last_error().decode())\n" % (ROOT, flat))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why, r.stdout


# ---- melscale_fbanks --------------------------------------------------------------------------------------------------------

def f_points(f_min, f_max, n_mels, scale):
    return api._mel_to_hz(np.linspace(float(api._mel(f_min, scale)), float(api._mel(f_max, scale)), n_mels + 2), scale)


def test_mel_scale_anchors():
    assert api._mel(700.0, "htk") == pytest.approx(2595.0 * math.log10(2.0), rel=1e-15)
    assert float(api._mel(1000.0, "slaney")) == 15.0
    assert float(api._mel(6400.0, "slaney")) == pytest.approx(42.0, rel=1e-15)
    assert float(api._mel(500.0, "slaney")) == 7.5
    f = np.array([0.0, 1.0, 200.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0, 22050.0])
    for scale in ("htk", "slaney"):
        assert np.allclose(api._mel_to_hz(api._mel(f, scale), scale), f, rtol=1e-13, atol=1e-11), scale


@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("n_freqs,n_mels", [(33, 6), (17, 5), (9, 3), (201, 40)])
def test_triangles_partition_unity_and_have_one_peak(n_freqs, n_mels, scale):
    rate = 16000
    fb = mf.melscale_fbanks(n_freqs, 0.0, 8000.0, n_mels, rate, mel_scale=scale)
    assert fb.dtype == torch.float64 and tuple(fb.shape) == (n_freqs, n_mels) and fb.is_contiguous()
    fb = fb.numpy()
    freqs = np.linspace(0.0, rate // 2, n_freqs)
    pts = f_points(0.0, 8000.0, n_mels, scale)
    assert (fb >= 0.0).all()
    inside = (freqs >= pts[1]) & (freqs <= pts[n_mels])
    assert inside.any()
    assert np.abs(fb[inside].sum(axis=1) - 1.0).max() <= 1e-12  # (neighbouring triangles: t and 1 - t)
    for m in range(n_mels):
        col = fb[:, m]
        nz = np.nonzero(col)[0]
        if nz.size == 0:  # (a triangle narrower than the bin spacing that holds no bin)
            assert not ((freqs > pts[m]) & (freqs < pts[m + 2])).any()
            continue
        assert (freqs[nz] > pts[m]).all() and (freqs[nz] < pts[m + 2]).all()
        assert nz[-1] - nz[0] + 1 == nz.size                       # one run
        peak = int(np.argmax(col))
        assert (np.diff(col[nz[0]:peak + 1]) >= 0).all() and (np.diff(col[peak:nz[-1] + 1]) <= 0).all()  # rises, then falls
        # The peak is the last bin at or below the centre f_pts[m+1] or the first one at or above it: no bin lies strictly
        # between the two.  (Not always the NEAREST bin: the falling side of a mel triangle is the wider one, so at
        # (33, 6) htk band 2, centre 1361.27 Hz, the bin at 1500 Hz holds 0.725 and the nearer one at 1250 Hz 0.697.)
        lo_f, hi_f = sorted((freqs[peak], pts[m + 1]))
        assert not ((freqs > lo_f) & (freqs < hi_f)).any()
        # and every weight is the scalar formula of its own bin
        for k in nz:
            up = (freqs[k] - pts[m]) / (pts[m + 1] - pts[m])
            down = (pts[m + 2] - freqs[k]) / (pts[m + 2] - pts[m + 1])
            assert col[k] == pytest.approx(min(up, down), rel=1e-13)
    slaney = mf.melscale_fbanks(n_freqs, 0.0, 8000.0, n_mels, rate, norm="slaney", mel_scale=scale).numpy()
    assert np.allclose(slaney, fb * (2.0 / (pts[2:] - pts[:-2]))[None, :], rtol=1e-15, atol=0.0)


def test_the_whisper_bank():
    """201 bins, 0 .. 8000 Hz, 80 bands at 16 kHz, slaney / slaney.  The three figures were computed on the CPU from the
    formulas in the docstring of melscale_fbanks; no library that has them (torchaudio, librosa) was at hand to confirm them."""
    fb = mf.melscale_fbanks(201, 0.0, 8000.0, 80, 16000, norm="slaney", mel_scale="slaney").numpy()
    assert (fb.max(axis=0) > 0).all()
    assert np.count_nonzero(fb) == 391
    assert fb[1, 0] == pytest.approx(0.024862593984176087, rel=1e-12)
    assert fb.max() == pytest.approx(0.02588068454527485, rel=1e-12)


def test_generator_arguments():
    for args, kw in (((201, 0.0, 8000.0, 80, 16000), dict(norm="ortho")), ((201, 0.0, 8000.0, 80, 16000), dict(mel_scale="mel")),
                     ((201, 8000.0, 100.0, 80, 16000), {}), ((201, 0.0, 8000.0, 0, 16000), {}), ((1, 0.0, 8000.0, 4, 16000), {})):
        with pytest.raises(mf.MifftError):
            mf.melscale_fbanks(*args, **kw)
    for args, kw in (((13, 40), dict(norm="backward")), ((0, 40), {}), ((13, 0), {})):
        with pytest.raises(mf.MifftError):
            mf.create_dct(*args, **kw)


@pytest.mark.parametrize("norm", [None, "ortho"])
@pytest.mark.parametrize("M,Q", [(3, 3), (40, 13), (80, 80)])
def test_create_dct_is_scipys_dct(M, Q, norm):
    D = mf.create_dct(Q, M, norm)
    assert D.dtype == torch.float64 and tuple(D.shape) == (M, Q)
    y = np.random.default_rng(M + Q).standard_normal((7, M))
    want = scipy.fft.dct(y, type=2, norm=norm)[..., :Q]
    assert np.abs(y @ D.numpy() - want).max() <= 1e-12


# ---- Python refusals --------------------------------------------------------------------------------------------------------

def test_the_python_layers_refuse_before_any_device():
    x = torch.zeros(3, 1000)  # (a host tensor: nothing reaches the library)
    fb = torch.ones(K, 5)
    for kw, status in ((dict(log="ln"), UNSUPPORTED), (dict(log=10), UNSUPPORTED), (dict(log=True), UNSUPPORTED),
                       (dict(log="log", ref=2.0), UNSUPPORTED), (dict(log="log10", ref=0.5), UNSUPPORTED),
                       (dict(ref=2.0), UNSUPPORTED),
                       (dict(log="db", amin=0.0), -5), (dict(log="db", ref=0.0), -5), (dict(log="log", eps=-1.0), -5),
                       (dict(fb=fb, post=torch.ones(4, 3)), -2), (dict(fb=fb, post=torch.ones(5)), -2),
                       (dict(fb=fb, post=torch.ones(5, 0)), -2),
                       (dict(post=torch.ones(5, 3)), UNSUPPORTED),
                       (dict(fb=fb, post=torch.ones(5, 3, dtype=torch.complex64)), -3)):
        with pytest.raises(mf.MifftError) as e:
            mf.spectrogram(x, 64, **kw)
        assert e.value.status == status, (kw, str(e.value))
        with pytest.raises(mf.MifftError) as e:
            mf.plan_spectrogram(torch.float32, 3, 1000, 64, 16, **kw)
        assert e.value.status == status, (kw, str(e.value))
    for ok in (dict(log="db"), dict(log="db", ref=2.0, power=1), dict(log="log", eps=1e-6, fb=fb), dict(log="log10", fb=fb.numpy()),
               dict(fb=fb, post=np.ones((5, 3))), dict(fb=fb, log="db", post=mf.create_dct(3, 5))):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.spectrogram(x, 64, **ok)
        assert e.value.status == -10, ok
    # the Plan keywords
    for kw, status in ((dict(stft_power=2, stft_log=(0.0, 1e-10, 1.0)), UNSUPPORTED),
                       (dict(stft_power=2, stft_log=(0.0, 0.0, 1.0, 0.0)), -5),
                       (dict(stft_log=LOG10), UNSUPPORTED),
                       (dict(stft_power=2, stft_post=np.ones((5, 3))), UNSUPPORTED)):
        with pytest.raises(mf.MifftError) as e:
            mf.Plan(torch.float32, torch.float32, (4, 1000, 1), (4, 235, 33, 1), stft_hop=4, **kw)
        assert e.value.status == status, (kw, str(e.value))
    with pytest.raises(mf.MifftError) as e:  # out follows Q
        mf.Plan(torch.float32, torch.float32, (4, 1000, 1), (4, 235, 5, 1), stft_hop=4, stft_power=2, stft_fb=np.ones((K, 5)),
                stft_post=np.ones((5, 3)))
    assert e.value.status == -2
    # mfcc
    for kw, status in ((dict(n_mels=200), UNSUPPORTED), (dict(n_mfcc=50, n_mels=40), -2), (dict(log="dB", n_mels=40), UNSUPPORTED),
                       (dict(dct_norm="forward", n_mels=40), UNSUPPORTED), (dict(mel_scale="bark", n_mels=40), UNSUPPORTED),
                       (dict(n_fft=401, n_mels=40), UNSUPPORTED)):
        with pytest.raises(mf.MifftError) as e:
            mf.mfcc(x, 16000, **kw)
        assert e.value.status == status, (kw, str(e.value))
    with pytest.raises(mf.MifftError) as e:
        mf.mfcc(x, 16000, 13, n_mels=40)
    assert e.value.status == -10


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_plan_spectrogram_builds_a_valid_tagged_payload():
    """the words the Python layer writes are a payload the library accepts (fp32 and fp64, every combination)"""
    fb = mf.melscale_fbanks(33, 0.0, 8000.0, 10, 16000)
    for dtype in (torch.float32, torch.float64):
        for kw in (dict(log="db"), dict(log="log", eps=1e-6), dict(log="log10", fb=fb), dict(fb=fb, post=mf.create_dct(4, 10)),
                   dict(fb=fb, log="db", ref=3.0, post=mf.create_dct(4, 10), window=np.hanning(64), center="reflect")):
            with pytest.raises(mf.MifftError) as e:
                mf.plan_spectrogram(dtype, 4, 1000, 64, 16, **kw)
            assert e.value.status == -10, (kw, str(e.value))
