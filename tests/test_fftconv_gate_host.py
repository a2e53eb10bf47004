"""Gated fftconv (the 16-word MIFFT_CONV_TAG payload; pregate, postgate, skip): an fp64 model of the gated operation against
numpy.convolve for the single-block and the overlap-save geometry, every refusal of the payload that needs no device, the
argument block of the exec as the header declares it, and the wrappers' host validation."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT
from test_fftconv_long_host import geometry

STFT, REFLECT, ZEROS, POWER, ISTFT = 32, 64, 128, 0x8000, 0x4000
UNSUPPORTED = -15
TAG_LO, TAG_HI = 0x4F4E5601, 0x7FF84D43
MAGIC = 0x314147544646494D  # "MIFFTGA1", little-endian


# ---- the model (fp64) ----------------------------------------------------------------------------------------------------------
def gated_model(x, k, n, *, a=None, b=None, skip=None, o=0, Lo=None, ols=None, correlate=False):
    """rows x (R, L) against filters k (D, K) or (K,), row r with filter r % D:
        xg = a * x;  G = rfft(k, n) + skip[r % D]  (conjugated: correlation);  y = b * irfft(rfft(blk) G, n)[window]
    ``ols`` None: one block, blk = xg zero-extended to n, the samples o .. o + Lo - 1.  ``ols`` = (c, S, s0, F): block f is
    blk[i] = xg[s0 + f S + i], zeros outside the row, and out[f S + j] = y[c + j] for j < S, f S + j < Lo."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    k = np.atleast_2d(np.asarray(k, dtype=np.float64))
    R, L = x.shape
    D = k.shape[0]
    Lo = L if Lo is None else Lo
    xg = x if a is None else np.asarray(a, dtype=np.float64).reshape(R, L) * x
    G = np.fft.rfft(k, n, axis=-1)
    if skip is not None:
        G = G + np.broadcast_to(np.asarray(skip, dtype=np.float64), (D,)).reshape(D, 1)
    if correlate:
        G = np.conj(G)
    G = G[np.arange(R) % D]
    if ols is None:
        assert L <= n and o + Lo <= n
        y = np.fft.irfft(np.fft.rfft(xg, n, axis=-1) * G, n, axis=-1)[:, o:o + Lo]
    else:
        c, S, s0, F = ols
        assert S >= 1 and c + S <= n and F >= 1 and (F - 1) * S < Lo <= F * S
        y = np.full((R, Lo), np.nan)
        for f in range(F):
            st = s0 + f * S
            blk = np.zeros((R, n))
            lo, hi = max(st, 0), min(st + n, L)
            blk[:, lo - st:hi - st] = xg[:, lo:hi]
            z = np.fft.irfft(np.fft.rfft(blk, axis=-1) * G, n, axis=-1)
            w = min(S, Lo - f * S)
            y[:, f * S:f * S + w] = z[:, c:c + w]
        assert not np.isnan(y).any()  # (every sample written once)
    return y if b is None else np.asarray(b, dtype=np.float64).reshape(R, Lo) * y


def direct(x, k, a, b, d, o, Lo, correlate=False):
    """b * (conv(a x, k) + d (a x)) sample by sample with numpy.convolve (correlation: sum_j k[j] xg[t + j])"""
    R, L = x.shape
    D, K = k.shape
    out = np.zeros((R, Lo))
    for r in range(R):
        xg = a[r] * x[r]
        if correlate:
            xp = np.concatenate([xg, np.zeros(K)])
            full = np.array([np.dot(k[r % D], xp[t:t + K]) for t in range(L)])
        else:
            full = np.convolve(xg, k[r % D])
        full = full.copy()
        full[:L] += d[r % D] * xg[:len(full[:L])]
        out[r] = b[r] * full[o:o + Lo]
    return out


@pytest.mark.parametrize("L,K,n", [(37, 28, 64), (11, 5, 16), (50, 1, 64), (101, 9, 16), (200, 33, 64), (333, 15, 16)])
@pytest.mark.parametrize("correlate", [False, True])
def test_the_model_against_numpy(L, K, n, correlate):
    rng = np.random.default_rng(L * 100 + K)
    D, B = 3, 2
    R = B * D
    x, k = rng.standard_normal((R, L)), rng.standard_normal((D, K))
    d = rng.standard_normal(D)
    single = L + K - 1 <= n
    for mode in (("causal",) if correlate else ("causal", "full", "same", "valid")):
        o, Lo = mf.api._fftconv_window(mode, L, K)
        a, b = rng.standard_normal((R, L)), rng.standard_normal((R, Lo))
        ols = None if single else geometry(n, K, o, Lo, correlate)
        for gates in (1, 2, 3):
            aa, bb = (a if gates & 1 else None), (b if gates & 2 else None)
            got = gated_model(x, k, n, a=aa, b=bb, skip=d, o=o, Lo=Lo, ols=ols, correlate=correlate)
            want = direct(x, k, a if gates & 1 else np.ones((R, L)), b if gates & 2 else np.ones((R, Lo)), d, o, Lo, correlate)
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (mode, gates)
        # a float skip is that value on every channel; no skip is zero
        got = gated_model(x, k, n, a=a, b=b, skip=0.75, o=o, Lo=Lo, ols=ols, correlate=correlate)
        assert np.abs(got - direct(x, k, a, b, np.full(D, 0.75), o, Lo, correlate)).max() <= 1e-11 * np.abs(got).max()
        got = gated_model(x, k, n, a=a, b=b, o=o, Lo=Lo, ols=ols, correlate=correlate)
        assert np.abs(got - direct(x, k, a, b, np.zeros(D), o, Lo, correlate)).max() <= 1e-11 * np.abs(got).max()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _create16(L=37, n=64, *, batch=6, D=3, w3=0, w4=37, mode=0, addr=0x10000, F=0, s0=0, Lo=0, gates=3, rsv=(0, 0, 0, 0),
              flags=STFT, radices=(), in_dtype=0, out_dtype=0, inverse=0, comps=1, device=0, len0=16):
    """the default: a single block (F = 0), rows of 37 samples at n = 64, o = 0, Lo = 37, both gates"""
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = [TAG_LO, TAG_HI, D, w3, w4, mode, addr & 0xFFFFFFFF, addr >> 32, F, s0 & 0xFFFFFFFF, Lo, gates] + list(rsv)
    flat = flat[:len0] + [1] * (len0 - len(flat))
    lens = (ctypes.c_int32 * 2)(len0, len(radices))
    flat = flat + list(radices)
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(L, n), batch, comps, inverse,
                               (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


# T = 1000, K = 33 at n = 64, causal: c = 32, S = 32, s0 = -32, F = 32 (the overlap-save form, F >= 1)
OLS = dict(L=1000, w3=32, w4=32, F=32, s0=-32, Lo=1000)


def test_c_abi_refuses_before_looking_for_a_device():
    for kw, status, word in (
            # the gated payload's own
            (dict(gates=0), -5, "gates word"),
            (dict(gates=4), -5, "gates word"),
            (dict(gates=7), -5, "gates word"),
            (dict(OLS, gates=0), -5, "gates word"),
            (dict(OLS, gates=4), -5, "gates word"),
            (dict(rsv=(1, 0, 0, 0)), -5, "reserved word 12"),
            (dict(rsv=(0, 0, 0, 9)), -5, "reserved word 15"),
            (dict(OLS, rsv=(0, 1, 0, 0)), -5, "reserved word 13"),
            (dict(s0=5), -5, "words 9 and 10"),
            (dict(Lo=37), -5, "words 9 and 10"),
            (dict(L=65), UNSUPPORTED, "L > n"),
            # what the 8-word form refuses, F = 0
            (dict(n=6, L=4, w4=4), UNSUPPORTED, "8 to 16384"),
            (dict(n=74), UNSUPPORTED, "packed"),
            (dict(n=63), UNSUPPORTED, "even"),
            (dict(n=16386), UNSUPPORTED, "16384"),
            (dict(n=16384, in_dtype=1, out_dtype=1), UNSUPPORTED, "packed"),
            (dict(w4=0), -5, "Lo"),
            (dict(w3=30, w4=35), -5, "o + Lo"),
            (dict(D=0), -5, "D"),
            (dict(D=4), -8, "multiple of D"),
            (dict(batch=7), -8, "multiple of D"),
            (dict(addr=0), -5, "null"),
            (dict(addr=0x10004), -5, "aligned"),
            (dict(addr=0x10008, in_dtype=1, out_dtype=1), -5, "aligned"),
            (dict(mode=2), -5, "mode"),
            (dict(inverse=1), UNSUPPORTED, "inverse"),
            (dict(in_dtype=2), -4, "in_dtype"),
            (dict(in_dtype=0, out_dtype=1), -4, "in_dtype"),
            (dict(comps=2), -3, "in_components"),
            (dict(flags=STFT | 1), UNSUPPORTED, "MIFFT_FLAG_FAITHFUL_STAGES"),
            (dict(flags=STFT | 2), UNSUPPORTED, "MIFFT_FLAG_HALF_SPECTRUM"),
            (dict(flags=STFT | 4), UNSUPPORTED, "MIFFT_FLAG_DCT"),
            (dict(flags=STFT | 16), UNSUPPORTED, "MIFFT_FLAG_DCT_ND"),
            (dict(flags=STFT | 8), UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO"),
            (dict(flags=STFT | (1 << 8)), UNSUPPORTED, "MIFFT_FLAG_KEEP_DIM"),
            (dict(flags=STFT | REFLECT), UNSUPPORTED, "centre bit"),
            (dict(flags=STFT | ZEROS), UNSUPPORTED, "centre bit"),
            (dict(flags=STFT | (16 << 16)), UNSUPPORTED, "hop"),
            (dict(flags=STFT | POWER), UNSUPPORTED, "MIFFT_FLAG_STFT_POWER"),
            (dict(flags=STFT | ISTFT), UNSUPPORTED, "MIFFT_FLAG_ISTFT"),
            (dict(radices=(3,)), -5, "length"),
            # what the 12-word form refuses, F >= 1
            (dict(OLS, w4=0), -5, "S >= 1"),
            (dict(OLS, w3=33), -5, "c + S <= n"),
            (dict(OLS, Lo=0), -5, "Lo >= 1"),
            (dict(OLS, Lo=992), -5, "(F - 1) S < Lo"),
            (dict(OLS, Lo=1025), -5, "Lo <= F S"),
            (dict(OLS, s0=-64), -5, "reads no sample"),
            (dict(OLS, s0=8), -5, "reads no sample"),
            (dict(OLS, L=960), -5, "reads no sample"),
            (dict(OLS, L=(1 << 30) + 1), -9, "2^30"),
            (dict(OLS, mode=2), -5, "mode"),
            (dict(OLS, D=4), -8, "multiple of D"),
            (dict(OLS, addr=0), -5, "null"),
            (dict(OLS, n=74), UNSUPPORTED, "packed"),
    ):
        rc, why = _create16(**kw)
        assert rc == status and word in why, (kw, rc, why)
    # the refusals name no device and none was looked for: the same answers for a device that cannot exist
    rc, why = _create16(gates=0, device=-1)
    assert rc == -5 and "gates word" in why, (rc, why)


def test_the_old_payloads_mean_what_they_meant():
    from test_fftconv_host import _create
    from test_fftconv_long_host import _create12
    rc, why = _create(mode=2)
    assert rc == -5 and "mode" in why, (rc, why)
    rc, why = _create12(mode=2)
    assert rc == -5 and "mode" in why, (rc, why)
    rc, why = _create12(w11=1)  # (word 11 is the gates word of the 16-word payload only)
    assert rc == -5 and "word 11" in why, (rc, why)
    rc, why = _create12(w11=3)
    assert rc == -5 and "word 11" in why, (rc, why)


def test_nearby_lengths_are_no_convolution_payloads():
    for len0 in (13, 14, 15, 17):
        rc, why = _create16(L=1000, len0=len0, flags=STFT | (16 << 16))
        assert rc == -5 and "bases_len[0]" in why, (len0, rc, why)
    rc, why = _create16(L=1000, flags=STFT | (16 << 16))  # (16 words: a convolution payload, which has no hop)
    assert rc == UNSUPPORTED and "hop" in why and "convolution" in why, (rc, why)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_a_valid_request_gets_as_far_as_the_device():
    for kw in (dict(), dict(gates=1), dict(gates=2), dict(L=64, w4=64), dict(w3=13, w4=37), dict(mode=1), dict(D=1), dict(batch=0),
               dict(n=16, L=11, w4=11), dict(n=16384, L=8192, w4=8192),
               dict(n=12288, L=6000, w4=6000, in_dtype=1, out_dtype=1, addr=0x10010), dict(radices=(2,)),
               OLS, dict(OLS, gates=1), dict(OLS, gates=2), dict(OLS, mode=1, w3=0, s0=0), dict(OLS, Lo=993),
               dict(n=16, L=100, w3=4, w4=12, s0=-4, F=9, Lo=100),
               dict(L=37, w3=27, w4=37, s0=-27, F=1, Lo=37),
               dict(n=16384, L=70000, w3=4096, w4=12288, s0=-4096, F=6, Lo=70000)):
        rc, why = _create16(**kw)
        assert rc == -10, (kw, rc, why)


def test_without_runtime_specialisation_the_plan_is_refused():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_fftconv_gate_host import _create16\n"
            "print(*_create16())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    rc, why = r.stdout.strip().split(" ", 1)
    assert int(rc) == UNSUPPORTED and "MIFFT_JIT=0" in why and "run time" in why, r.stdout


def test_the_argument_block_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    m = re.search(r"#define\s+MIFFT_GATED_ARGS_MAGIC\s+0x([0-9A-Fa-f]+)ull\b", h)
    assert m and int(m.group(1), 16) == MAGIC == mf.GATED_ARGS_MAGIC
    assert MAGIC.to_bytes(8, "little") == b"MIFFTGA1"
    body = re.search(r"typedef struct mifft_gated_args \{(.*?)\} mifft_gated_args;", re.sub(r"/\*.*?\*/", "", h, flags=re.S), re.S)
    assert body and [f.split()[-1].rstrip(";") for f in body.group(1).strip().splitlines()] == ["magic", "x", "pregate", "postgate"]
    assert [f[0] for f in mf.GatedArgs._fields_] == ["magic", "x", "pregate", "postgate"]
    assert ctypes.sizeof(mf.GatedArgs) == 8 + 3 * ctypes.sizeof(ctypes.c_void_p)
    assert "mifft_gated_args" in open(os.path.join(ROOT, "include", "mifft.hpp")).read()
    # the block travels through mifft_exec_batch: the exported functions are what they were
    assert "mifft_exec_batch" in _lib.EXPORTS and not [e for e in _lib.EXPORTS if "gate" in e]


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_fftconv_validates_its_gates_on_the_host():
    x, k = torch.zeros(2, 3, 40), torch.zeros(3, 9)  # (host tensors: nothing reaches the library)
    for kw in (dict(pregate=torch.zeros(2, 3, 41)), dict(pregate=torch.zeros(2, 3, 48), mode="full"),
               dict(postgate=torch.zeros(2, 3, 40), mode="full"),                # the result has 48 samples
               dict(postgate=torch.zeros(2, 3, 41)), dict(postgate=torch.zeros(6, 40)),
               dict(pregate=torch.zeros(3, 40)), dict(pregate=torch.zeros(1, 3, 40)),     # broadcastable: refused all the same
               dict(postgate=torch.zeros(2, 1, 40)), dict(pregate=torch.zeros(40)), dict(postgate=torch.zeros(2, 3, 1)),
               dict(skip=torch.zeros(4)), dict(skip=torch.zeros(1)), dict(skip=torch.zeros(3, 1)),
               dict(skip=torch.zeros(3, dtype=torch.complex64))):
        with pytest.raises(ValueError) as e:
            mf.fftconv(x, k, **kw)
        assert "broadcast" in str(e.value) or "skip" in str(e.value), (kw, e.value)
    with pytest.raises(ValueError) as e:
        mf.fftconv(x, k, pregate=torch.zeros(1, 3, 40))
    assert "cost what the fusion saves" in str(e.value)
    # a gate on another device than x's
    for kw in (dict(pregate=torch.zeros(2, 3, 40, device="meta")), dict(postgate=torch.zeros(2, 3, 40, device="meta"))):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv(x, k, **kw)
        assert e.value.status == -10 and "gate lives on meta" in str(e.value), (kw, e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(x, k, pregate=torch.zeros(2, 3, 40, dtype=torch.complex64))
    assert e.value.status == -3
    # valid: fails only for want of a device tensor
    for kw in (dict(pregate=torch.zeros(2, 3, 40)), dict(postgate=torch.zeros(2, 3, 40)), dict(skip=0.5), dict(skip=torch.zeros(3)),
               dict(pregate=torch.zeros(2, 3, 40), postgate=torch.zeros(2, 3, 48), skip=1, mode="full"),
               dict(pregate=torch.zeros(2, 3, 40), postgate=torch.zeros(2, 3, 40), block=16, correlate=True)):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv(x, k, **kw)
        assert e.value.status == -10 and "gate" not in str(e.value), (kw, e.value)  # (about x, or about there being no device)


def test_fft_refuses_a_gated_plan_and_points_to_run():
    plan = types.SimpleNamespace(conv_gates=3)  # (the one attribute fft looks at first: no device, no library call)
    with pytest.raises(mf.MifftError) as e:
        mf.fft(torch.zeros(1), torch.zeros(1), plan=plan)
    assert e.value.status == UNSUPPORTED and "run(" in str(e.value)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of a valid request")
def test_plan_fftconv_takes_the_gate_keywords():
    for kw in (dict(pregate=True), dict(postgate=True), dict(pregate=True, postgate=True, taps=9)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv(torch.float32, 2, 3, 40, 64, **kw)
        assert e.value.status == -10, kw
    with pytest.raises(mf.MifftError) as e:  # argument errors still come first
        mf.plan_fftconv(torch.float32, 2, 3, 65, 64, pregate=True)
    assert e.value.status == UNSUPPORTED
