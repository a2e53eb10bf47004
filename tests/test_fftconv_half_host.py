"""Half-precision storage of the fused convolution without a device: bits 8..15 of the mode word of every MIFFT_CONV_TAG form
(8, 12, 16 and 20 words) and of the MIFFT_CONV_GRAD_TAG form -- accepted with MIFFT_F16 (7) and MIFFT_BF16 (8), every other
value and every bit from 16 up refused with MIFFT_ERR_BAD_BASES, a storage type under an F64 plan with MIFFT_ERR_BAD_DTYPE --
the host-side validation of ``io_dtype`` in plan_fftconv, plan_fftconv_grad, fftconv and fftconv_filter_grad, and a numpy
model of the rounding of the kernel's store (to nearest even, on the bits) against torch's ``.to()``, on which the GPU tests
(test_gpu_fftconv_half.py) then rely.  A plan exists only on a device, so the byte counts of a half-storage plan
(mifft_plan_in_bytes / _out_bytes) are checked there."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from test_fftconv_gate_host import OLS as OLS16
from test_fftconv_gate_host import _create16
from test_fftconv_grad_host import OLS as OLSG
from test_fftconv_grad_host import _create as create_grad
from test_fftconv_host import _create as create8
from test_fftconv_long_host import _create12
from test_fftconv_part_host import _create20

F16, BF16 = 7, 8
NO_DEVICE, BAD_BASES, BAD_DTYPE = -10, -5, -4

# every payload form with arguments its own host tests accept (the defaults, and a second geometry where there is one)
FORMS = [("8 words", create8, dict()), ("8 words, o > 0", create8, dict(o=13, Lo=20)),
         ("12 words", _create12, dict()),
         ("16 words, single block", _create16, dict()), ("16 words, overlap-save", _create16, dict(OLS16, gates=1)),
         ("20 words", _create20, dict()), ("20 words, gated", _create20, dict(gates=3)),
         ("gradient", create_grad, dict()), ("gradient, overlap-save", create_grad, dict(OLSG))]
IDS = [f[0] for f in FORMS]


def test_the_codes_are_the_library_s():
    assert (mf.api._DTYPE_CODE[torch.float16], mf.api._DTYPE_CODE[torch.bfloat16]) == (F16, BF16)
    assert mf.api._io_mode_bits(None) == 0 and mf.api._io_mode_bits(torch.bfloat16) == BF16 << 8


@pytest.mark.parametrize("what,create,kw", FORMS, ids=IDS)
@pytest.mark.parametrize("io", [F16, BF16])
@pytest.mark.parametrize("correlate", [0, 1])
def test_a_storage_type_gets_as_far_as_the_device(what, create, kw, io, correlate):
    rc, why = create(device=-1, mode=(io << 8) | correlate, **kw)
    assert rc == NO_DEVICE and "device" in why, (what, rc, why)


@pytest.mark.parametrize("what,create,kw", FORMS, ids=IDS)
def test_storage_type_0_means_what_the_word_meant(what, create, kw):
    for mode in (0, 1):
        rc, why = create(device=-1, mode=mode, **kw)
        assert rc == NO_DEVICE and "device" in why, (what, mode, rc, why)


@pytest.mark.parametrize("what,create,kw", FORMS, ids=IDS)
def test_every_other_mode_word_is_refused(what, create, kw):
    bad = [2, 3, 4, 0x80] + [v << 8 for v in (1, 6, 9, 255)] + [(v << 8) | 1 for v in (1, 6, 9, 255)]
    bad += [1 << b for b in range(16, 32)] + [(BF16 << 8) | (1 << 16), (F16 << 8) | (1 << 31), (BF16 << 8) | 2]
    for mode in bad:
        rc, why = create(device=-1, mode=mode, **kw)
        assert rc == BAD_BASES and "mode" in why, (what, hex(mode), rc, why)


@pytest.mark.parametrize("what,create,kw", FORMS, ids=IDS)
@pytest.mark.parametrize("io", [F16, BF16])
def test_a_storage_type_under_a_float64_plan_is_a_dtype_error(what, create, kw, io):
    rc, why = create(device=-1, mode=io << 8, in_dtype=1, out_dtype=1, **kw)
    assert rc == BAD_DTYPE and "MIFFT_F32" in why, (what, rc, why)
    rc, why = create(device=-1, mode=0, in_dtype=1, out_dtype=1, **kw)  # (the float64 plan itself is what it was)
    assert rc == NO_DEVICE, (what, rc, why)


def test_acceptance_lists_of_the_existing_host_tests_still_plan():
    """a handful of each list, re-created here with storage type 0 and with both storage types"""
    cases = [(create8, dict(o=27, Lo=37)), (create8, dict(mode=1)), (create8, dict(n=16384, L=8192, Lo=8192)),
             (create8, dict(n=96, L=50, o=10, Lo=60)),
             (_create12, dict(Lo=993)), (_create12, dict(mode=1, c=0, s0=0)),
             (_create16, dict(gates=1)), (_create16, dict(gates=2)), (_create16, dict(OLS16)),
             (_create20, dict(gates=0)), (_create20, dict(mode=1, c=0, s0=0)),
             (create_grad, dict(c=13)), (create_grad, dict(P=2)), (create_grad, dict(OLSG, P=46)),
             (create_grad, dict(n=16384, L=8192, S=8192, Lo=8192))]
    for create, kw in cases:
        corr = kw.get("mode", 0)
        for io in (0, F16, BF16):
            rc, why = create(device=-1, **dict(kw, mode=corr | (io << 8)))
            assert rc == NO_DEVICE and "device" in why, (kw, io, rc, why)


# ---- Python: every refusal before any device work ---------------------------------------------------------------------------
def _status(fn, *a, **kw):
    with pytest.raises(mf.MifftError) as e:
        fn(*a, **kw)
    return e.value.status


@pytest.mark.parametrize("plan", [mf.plan_fftconv, mf.plan_fftconv_grad], ids=["plan_fftconv", "plan_fftconv_grad"])
def test_plan_io_dtype_is_checked_before_the_device(plan):
    for kw in (dict(), dict(taps=9), dict(taps=100, partition=9)):
        n, L = (64, 37) if not kw else (64, 1000)
        assert _status(plan, torch.float64, 2, 3, L, n, io_dtype=torch.bfloat16, **kw) == BAD_DTYPE
        assert _status(plan, torch.float64, 2, 3, L, n, io_dtype=torch.float16, **kw) == BAD_DTYPE
        assert _status(plan, torch.float32, 2, 3, L, n, io_dtype=torch.float32, **kw) == BAD_DTYPE
        assert _status(plan, torch.float32, 2, 3, L, n, io_dtype=torch.int16, **kw) == BAD_DTYPE
        assert _status(plan, torch.float32, 2, 3, L, n, io_dtype=torch.float64, **kw) == BAD_DTYPE
        assert _status(plan, torch.float16, 2, 3, L, n, **kw) == BAD_DTYPE       # (as ever)
        assert _status(plan, torch.bfloat16, 2, 3, L, n, **kw) == BAD_DTYPE
        assert _status(plan, torch.float16, 2, 3, L, n, io_dtype=torch.float16, **kw) == BAD_DTYPE
    # (the other argument checks still come first or after as they did: a bad n with a good io_dtype is the old refusal)
    assert _status(plan, torch.float32, 2, 3, 37, 74, io_dtype=torch.bfloat16) == -15
    assert _status(plan, torch.float32, 0, 3, 37, 64, io_dtype=torch.bfloat16) == -8


def test_fftconv_checks_its_arguments_and_then_the_device():
    x, k = torch.zeros(2, 3, 37), torch.zeros(3, 9)
    base = _status(mf.fftconv, x, k)  # (what a CPU tensor has always met)
    for t in (torch.bfloat16, torch.float16):
        assert _status(mf.fftconv, x, k, io_dtype=t) == base == NO_DEVICE
        assert _status(mf.fftconv, x.to(t), k, io_dtype=t) == NO_DEVICE
        assert _status(mf.fftconv_filter_grad, x, x, 9, io_dtype=t) == NO_DEVICE
    # the argument checks come first
    for bad in (torch.float32, torch.float64, torch.int16):
        assert _status(mf.fftconv, x, k, io_dtype=bad) == BAD_DTYPE
        assert _status(mf.fftconv_filter_grad, x, x, 9, io_dtype=bad) == BAD_DTYPE
    with pytest.raises(ValueError):
        mf.fftconv(x, k, io_dtype=torch.bfloat16, mode="sideways")
    with pytest.raises(ValueError):
        mf.fftconv(x, k, io_dtype=torch.bfloat16, pregate=torch.zeros(2, 3, 36))
    with pytest.raises(ValueError):
        mf.fftconv(x, k, io_dtype=torch.bfloat16, n=64, block=64)
    assert _status(mf.fftconv, x, torch.zeros(4, 9), io_dtype=torch.float16) == -2
    assert _status(mf.fftconv, x, k, io_dtype=torch.float16, n=74) == -15


def test_io_dtype_is_none_on_other_plans():
    assert mf.Plan.io_dtype is None and mf.api.ConvPlan.io_dtype is None and mf.api.ConvGradPlan.io_dtype is None


# ---- the rounding of the store: to nearest even on the bits -----------------------------------------------------------------
def bf16_bits(v):
    """float32 -> the bits of bfloat16, rounded to nearest even (the kernel's bf16_t::from_float): the half below the kept
    one plus the kept half's last bit carries into it; NaN -> 0x7fc0"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def _values():
    rng = np.random.default_rng(21)
    v = [rng.standard_normal(3000).astype(np.float32),
         (rng.standard_normal(1000) * 2.0 ** rng.integers(-30, 30, 1000)).astype(np.float32),
         (rng.standard_normal(1000) * 2.0 ** -14).astype(np.float32),    # float16 subnormals and their neighbours
         (rng.standard_normal(500) * 2.0 ** -24).astype(np.float32),     # around the smallest float16 subnormal
         (rng.standard_normal(500) * 65504.0).astype(np.float32)]        # some beyond the float16 range
    # ties of bfloat16 (the dropped half is exactly 0x8000) on even and odd kept halves, and their neighbours
    hi = rng.integers(0x0080, 0x7F7F, 600).astype(np.uint32)
    for low in (0x8000, 0x7FFF, 0x8001):
        v.append(((hi << 16) | low).view(np.float32))
        v.append(((hi << 16) | low | 0x80000000).astype(np.uint32).view(np.float32))
    # ties of float16: 11 significant bits kept, the 12th set and nothing below (normal range), and in the subnormal range
    m = rng.integers(0, 1 << 10, 400).astype(np.uint32)
    e = rng.integers(113, 142, 400).astype(np.uint32)
    v.append(((e << 23) | (m << 13) | 0x1000).view(np.float32))
    v.append((np.arange(0, 2048, dtype=np.float32) + 0.5) * np.float32(2.0 ** -24))
    fmax = np.finfo(np.float32).max
    v.append(np.array([0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e5, -1e5, fmax, -fmax, 3.3895e38,
                       np.inf, -np.inf, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14, 2.0 ** -126, 1e-45],
                      dtype=np.float32))
    return np.concatenate(v)


def test_the_numpy_model_of_the_rounding_is_torch_s():
    v = _values()
    assert v.size > 5000
    t = torch.from_numpy(v)
    got_b = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got_b, bf16_bits(v))
    with np.errstate(over="ignore"):
        want_h = v.astype(np.float16)  # (IEEE: to nearest even, overflow to infinity, subnormals kept)
    got_h = t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got_h, want_h.view(np.uint16))
    assert np.isinf(want_h).sum() > 4 and ((want_h != 0) & (np.abs(want_h) < 2.0 ** -14)).sum() > 1000
    # NaN stays NaN
    nan = torch.tensor([float("nan")])
    assert torch.isnan(nan.to(torch.bfloat16)).all() and bf16_bits(np.array([np.nan], dtype=np.float32))[0] == 0x7FC0
    # widening is exact: narrow(widen(h)) == h for every finite 16-bit pattern
    allbits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    for dt in (torch.bfloat16, torch.float16):
        h = allbits.view(dt)
        ok = torch.isfinite(h)
        assert torch.equal(h.float().to(dt).view(torch.int16)[ok], allbits[ok])
