"""The nine families of fused tile passes (csrc/kernels_jit.cpp), held to what they answer without a device: each one accepts
the smallest length it takes, refuses with the WHOLE message on every refusal branch of its configuration function that the
plan's earlier checks let through, and names its own reason when the runtime specialisation is switched off (MIFFT_JIT=0).

Every request comes in through the public plan function of its family with the no-device context (device = -1): an accepted
request ends in status -10, a refused one in -15 with its reason.  The expected texts are literals: what the library printed
before the families shared one table, so that the table is held to them.

Branches that cannot be reached from outside, because an earlier check answers first:
  * a packed row below 8 points or of odd length: every plan check but the half spectrum's names its own limit first;
  * a DCT column beyond 4096 points (dctn_check: "longer than one column tile") or of fewer than 2 (no dimension is of size 1);
  * the IMDCT carry that does not fit LDS: a packed tile is at most 96 KiB and the carry a quarter of a one-row tile, so every
    length a DCT-IV row plans has an IMDCT configuration;
  * a convolution length outside 8 .. 16384: conv_check names the limits of the packed rows itself.
plan_fftconv allocates the filter spectra on the device before it asks the library, and refuses an FFT length with a text of its
own before that; the convolution requests are therefore what its body makes after both -- Plan(conv=) of the same request,
with an address that nothing dereferences."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import hackathon_fft_amd as mf
from conftest import ROOT

ND = types.SimpleNamespace(device=-1)
ACCEPTED, UNSUPPORTED = -10, -15
F32, F64 = torch.float32, torch.float64

ROW_LIMITS = "packed real rows need an even length from 8 to 16384"
NO_PACKED = "n / 2 has no packed configuration (a prime factor above 32, or a tile beyond 96 KiB of LDS)"
NO_COLUMN = "no fused column configuration (a prime factor above 4093, or a tile beyond 160 KiB of LDS)"
BIG_PRIME_COLUMN = "a prime factor above 32 (the cooperative prime passes have no DCT load / store)"
JIT0_PACKED = "MIFFT_JIT=0 and no precompiled packed-row kernel for this length and element type"
JIT0_STFT = "MIFFT_JIT=0: the STFT kernels are compiled at run time only"
JIT0_CONV = "MIFFT_JIT=0: the convolution kernels are compiled at run time only"
JIT0_ISTFT = "MIFFT_JIT=0: the inverse STFT kernels are compiled at run time only"
JIT0_COLS = "MIFFT_JIT=0: the paired-column DCT tiles are compiled at run time only"
JIT0_DCT4 = "MIFFT_JIT=0: the DCT-IV kernels are compiled at run time only"  # (the IMDCT reports the DCT-IV's text, as it always has)


# ---- one request per family, through its public plan function ------------------------------------------------------------------
def half_rows(n, dt=F32, inverse=False):
    real, cplx = (2, n, 1), (2, n // 2 + 1, 2)
    return mf.plan_fft(dt, dt, cplx if inverse else real, real if inverse else cplx, half_spectrum=True, inverse=inverse, ctx=ND)


def dct_rows(n, dt=F32, **kw):
    return mf.plan_fft(dt, dt, (2, n, 1), (2, n, 1), dct=True, ctx=ND, **kw)


def dct4_rows(n, dt=F32):
    return dct_rows(n, dt, dct_type=4)


def dct_cols(c, dt=F32, **kw):
    """c-point columns beside an 8-point row"""
    return mf.plan_fft(dt, dt, (2, c, 8, 1), (2, c, 8, 1), dctn=True, ctx=ND, **kw)


def stft_rows(n, dt=F32):
    return mf.plan_stft(dt, 2, 4 * n, n, n // 4, ctx=ND)


def istft_rows(n, dt=F32):
    return mf.plan_istft(dt, 2, 5, n, n // 4, ctx=ND)


def mdct_rows(M, dt=F32):
    return mf.plan_mdct(dt, 2, 4 * M, M, ctx=ND)


def imdct_rows(M, dt=F32):
    return mf.plan_imdct(dt, 2, 5, M, ctx=ND)


def conv_rows(n, dt=F32):
    req = mf.api._fftconv_request(n, 2, 0, n // 2, False, None, None, None)
    return mf.Plan(dt, dt, (4, n // 2, 1), (4, n // 2, 1), device=-1, conv=req._replace(address=4096))


def answer(make, *args, **kw):
    try:
        make(*args, **kw)
    except mf.MifftError as e:
        return [e.status, str(e)]
    return [0, "a plan was made"]


def refusal(text):
    return [UNSUPPORTED, "mifft error %d: %s" % (UNSUPPORTED, text)]


def accepted(got):
    """the request passed every check that needs no device (the text counts the devices of the machine: not compared)"""
    return got[0] == ACCEPTED and "device -1" in got[1]


# family: (the request, the smallest length it takes, [(arguments, the whole refusal)])
FAMILIES = {
    "HalfRows": (half_rows, 8, [
        ((6,), "half spectrum of a last dimension of 6 points: " + ROW_LIMITS),  # (the one plan check without a limit of its own)
        ((32768,), "half spectrum of a last dimension of 32768 points: " + ROW_LIMITS),
        ((74,), "half spectrum of a last dimension of 74 points: " + NO_PACKED),
        ((16384, F64), "half spectrum of a last dimension of 16384 points: " + NO_PACKED)]),
    "DctRows": (dct_rows, 8, [
        ((32768,), "DCT of 32768 points: " + ROW_LIMITS),
        ((74,), "DCT of 74 points: " + NO_PACKED),
        ((16384, F64), "DCT of 16384 points: " + NO_PACKED)]),
    "StftRows": (stft_rows, 8, [
        ((32768,), "STFT with frames of 32768 points: " + ROW_LIMITS),
        ((74,), "STFT with frames of 74 points: " + NO_PACKED),
        ((16384, F64), "STFT with frames of 16384 points: " + NO_PACKED)]),
    "ConvRows": (conv_rows, 8, [
        ((74,), "convolution at an FFT length of 74: " + NO_PACKED),
        ((16384, F64), "convolution at an FFT length of 16384: " + NO_PACKED)]),
    "IstftRows": (istft_rows, 8, [
        ((32768,), "STFT with frames of 32768 points: " + ROW_LIMITS),
        ((74,), "STFT with frames of 74 points: " + NO_PACKED),
        ((16384, F64), "STFT with frames of 16384 points: " + NO_PACKED),
        # fp64 frames above 10240: tile (one row) and carry pass 160 KiB
        ((12288, F64), "STFT with frames of 12288 points: the tile and the overlap-add carry of 12288 reals do not fit the CU's LDS")]),
    "DctCols": (dct_cols, 2, [
        ((37,), "DCT column pass over dimension 0 (37 points): " + BIG_PRIME_COLUMN),
        ((4093,), "DCT column pass over dimension 0 (4093 points): " + NO_COLUMN),
        ((4096, F64), "DCT column pass over dimension 0 (4096 points): " + NO_COLUMN)]),
    "Dct4Rows": (dct4_rows, 8, [
        ((32768,), "DCT-IV of 32768 points: " + ROW_LIMITS),
        ((74,), "DCT-IV of 74 points: " + NO_PACKED),
        ((16384, F64), "DCT-IV of 16384 points: " + NO_PACKED)]),
    "MdctRows": (mdct_rows, 8, [
        ((32768,), "MDCT with M = 32768 coefficients per frame: " + ROW_LIMITS),
        ((74,), "MDCT with M = 74 coefficients per frame: " + NO_PACKED),
        ((16384, F64), "MDCT with M = 16384 coefficients per frame: " + NO_PACKED)]),
    "ImdctRows": (imdct_rows, 8, [
        ((32768,), "IMDCT with M = 32768 coefficients per frame: " + ROW_LIMITS),
        ((74,), "IMDCT with M = 74 coefficients per frame: " + NO_PACKED),
        ((16384, F64), "IMDCT with M = 16384 coefficients per frame: " + NO_PACKED)]),
}

# With MIFFT_JIT=0: the request (by name, for the child process), its arguments, and the whole refusal (None: accepted).  A
# column pass is asked alone (the row kept), or the row pass of the same plan would answer first; 1024 points are precompiled
# in both directions and element types of the two families a precompiled instance may serve, and for no sine transform.
JIT0 = {
    "HalfRows": ("half_rows", (8,), {}, refusal("half spectrum of a last dimension of 8 points: " + JIT0_PACKED)),
    "HalfRows-inverse": ("half_rows", (8,), dict(inverse=True), refusal("half spectrum of a last dimension of 8 points: " + JIT0_PACKED)),
    "HalfRows-precompiled": ("half_rows", (1024,), {}, None),
    "HalfRows-precompiled-f64-inverse": ("half_rows", (1024, F64), dict(inverse=True), None),
    "DctRows": ("dct_rows", (8,), {}, refusal("DCT of 8 points: " + JIT0_PACKED)),
    "DctRows-precompiled": ("dct_rows", (1024,), {}, None),
    "DctRows-precompiled-f64-inverse": ("dct_rows", (1024, F64), dict(inverse=True), None),
    "DctRows-sine": ("dct_rows", (1024,), dict(dst=True), refusal("DCT of 1024 points: " + JIT0_PACKED)),
    "StftRows": ("stft_rows", (8,), {}, refusal("STFT with frames of 8 points: " + JIT0_STFT)),
    "ConvRows": ("conv_rows", (8,), {}, refusal("convolution at an FFT length of 8: " + JIT0_CONV)),
    "IstftRows": ("istft_rows", (8,), {}, refusal("STFT with frames of 8 points: " + JIT0_ISTFT)),
    "DctCols": ("dct_cols", (2,), dict(axes=(1,)), refusal("DCT column pass over dimension 0 (2 points): " + JIT0_COLS)),
    "Dct4Rows": ("dct4_rows", (8,), {}, refusal("DCT-IV of 8 points: " + JIT0_DCT4)),
    "MdctRows": ("mdct_rows", (8,), {}, refusal("MDCT with M = 8 coefficients per frame: " + JIT0_DCT4)),
    "ImdctRows": ("imdct_rows", (8,), {}, refusal("IMDCT with M = 8 coefficients per frame: " + JIT0_DCT4)),
}


def jit0_answers():
    """every JIT0 request, answered in this process"""
    return {k: answer(globals()[name], *args, **kw) for k, (name, args, kw, _) in JIT0.items()}


@pytest.fixture(scope="module")
def without_jit():
    """the answers of one fresh process with MIFFT_JIT=0: the switch is read once per process"""
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_tile_families_host as t\n"
            "print(json.dumps(t.jit0_answers()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family(family, without_jit):
    make, smallest, refusals = FAMILIES[family]
    assert accepted(answer(make, smallest))
    for args, text in refusals:
        assert answer(make, *args) == refusal(text), args
    asked = [k for k in JIT0 if k.split("-")[0] == family]
    assert asked
    for k in asked:
        want = JIT0[k][3]
        assert accepted(without_jit[k]) if want is None else without_jit[k] == want, (k, without_jit[k])


def test_the_table_names_nine_families():
    assert list(FAMILIES) == ["HalfRows", "DctRows", "StftRows", "ConvRows", "IstftRows", "DctCols", "Dct4Rows", "MdctRows",
                              "ImdctRows"]
    assert {k.split("-")[0] for k in JIT0} == set(FAMILIES)
