"""Gates fused into the filter gradient of fftconv, without a device: word 11 of the MIFFT_CONV_GRAD_TAG payload as Python
writes it and as the library validates it (the payload checks run before a device is looked for), the argument block of the
gated exec as the header and ctypes declare it, the host-side refusals of plan_fftconv_grad / fftconv_filter_grad with gates,
and the slicing of the gates by the composed partitioned plan.  The GPU tests are in test_gpu_fftconv_grad_gate.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd.api import ConvRequest, _conv_payload, _fftconv_part_grad_operands, _fftconv_part_grad_slice
from test_fftconv_grad_host import OLS, TAG_HI, TAG_LO, _create

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC2 = 0x324757544646494D
BF16, F16 = 8, 7  # MIFFT_BF16, MIFFT_F16


# ---- the payload ------------------------------------------------------------------------------------------------------------
def test_payload_carries_the_gates_in_word_11():
    # a single block: n = 64, D = 3, o = 0, Lo = 37; today's words, written out
    assert _conv_payload(ConvRequest(64, 3, 0, 37, grad=True, gates=0)) == \
        [0x44524701, 0x7FF84D47, 3, 0, 37, 0, 1, 0, 37, 0, 0, 0, 0, 0, 0, 0]
    # overlap-save: n = 64, K = 20 on rows of 1000 (c = 19, S = 45, s0 = -19, F = 23), correlate off, bfloat16 rows, P = 4
    ols = ConvRequest(64, 3, 19, 1000, S=45, F=23, s0=-19, mode=BF16 << 8, grad=True, partials=4)
    assert _conv_payload(ols) == [0x44524701, 0x7FF84D47, 3, 19, 45, 0x800, 23, 0xFFFFFFED, 1000, 4, 0, 0, 0, 0, 0, 0]
    for g in (1, 2, 3):
        for r in (ConvRequest(64, 3, 0, 37, grad=True, gates=g), ols._replace(gates=g)):
            w, w0 = _conv_payload(r), _conv_payload(r._replace(gates=0))
            assert len(w) == 16 and w[11] == g and w[:11] == w0[:11] and w[12:] == [0, 0, 0, 0] == w0[12:]
    with pytest.raises(mf.MifftError) as e:
        _conv_payload(ConvRequest(64, 3, 0, 37, grad=True, gates=4))
    assert e.value.status == -5


def _rsv(word10=0, gates=0, word12=0):
    return (word10, gates, word12, 0, 0, 0)


def test_the_library_validates_word_11_before_it_looks_for_a_device():
    for g in (1, 2, 3):
        for kw in (dict(), OLS, dict(mode=BF16 << 8), dict(OLS, mode=(F16 << 8) | 1, c=0, s0=0), dict(P=2),
                   dict(n=16384, L=8192, S=8192, Lo=8192), dict(n=12288, L=6000, S=6000, Lo=6000, in_dtype=1, out_dtype=1)):
            rc, why = _create(device=-1, rsv=_rsv(gates=g), **kw)
            assert rc == -10 and "device" in why, (g, kw, rc, why)
    for g in (4, 7, 0x80000000):
        rc, why = _create(device=-1, rsv=_rsv(gates=g))
        assert rc == -5 and "gates" in why and "word 11" in why, (g, rc, why)
    # the reserved words around it keep their refusals, with gates and without
    for g in (0, 3):
        rc, why = _create(device=-1, rsv=_rsv(word10=5, gates=g))
        assert rc == -5 and "reserved word 10" in why, (rc, why)
        rc, why = _create(device=-1, rsv=_rsv(word12=1, gates=g))
        assert rc == -5 and "reserved word 12" in why, (rc, why)
        rc, why = _create(device=-1, rsv=(0, g, 0, 0, 0, 9))
        assert rc == -5 and "reserved word 15" in why, (rc, why)
    # a storage type wants an F32 plan, gated or not
    rc, why = _create(device=-1, rsv=_rsv(gates=3), mode=BF16 << 8, in_dtype=1, out_dtype=1)
    assert rc == -4, (rc, why)


def test_the_gated_argument_block_is_declared_and_mirrored():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    m = re.search(r"#define\s+MIFFT_CONV_GRAD_GATED_ARGS_MAGIC\s+0x([0-9A-Fa-f]+)ull\b", h)
    assert m and int(m.group(1), 16) == MAGIC2 == mf.CONV_GRAD_GATED_ARGS_MAGIC
    assert MAGIC2.to_bytes(8, "little") == b"MIFFTWG2"
    assert MAGIC2 not in (mf.CONV_GRAD_ARGS_MAGIC, mf.GATED_ARGS_MAGIC)
    assert re.search(r"typedef struct mifft_conv_grad_gated_args \{\s*uint64_t magic;[^}]*const void\* x;[^}]*const void\* gy;"
                     r"[^}]*const void\* pregate;[^}]*const void\* postgate;[^}]*\} mifft_conv_grad_gated_args;", h)
    assert [f[0] for f in mf.ConvGradGatedArgs._fields_] == ["magic", "x", "gy", "pregate", "postgate"]
    assert ctypes.sizeof(mf.ConvGradGatedArgs) == 8 + 4 * ctypes.sizeof(ctypes.c_void_p)
    # the ungated block is what it was
    assert [f[0] for f in mf.ConvGradArgs._fields_] == ["magic", "x", "gy"] and ctypes.sizeof(mf.ConvGradArgs) == 24
    assert (mf.CONV_GRAD_TAG_LO, mf.CONV_GRAD_TAG_HI) == (TAG_LO, TAG_HI)


# ---- Python: every argument error comes before any device work --------------------------------------------------------------
def test_plan_fftconv_grad_with_gates_validates_on_the_host():
    f32 = torch.float32
    for kw, status in ((dict(pregate=True, io_dtype=torch.int8), -4), (dict(postgate=True, io_dtype=torch.float32), -4),
                       (dict(pregate=True, partials=0), -5), (dict(pregate=True, postgate=True, taps=64), -2)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv_grad(f32, 2, 3, 40, 64, **kw)
        assert e.value.status == status, (kw, e.value)
    with pytest.raises(mf.MifftError) as e:  # (16-bit rows go with float32 arithmetic, gates or none)
        mf.plan_fftconv_grad(torch.float64, 2, 3, 40, 64, pregate=True, io_dtype=torch.bfloat16)
    assert e.value.status == -4
    for kw in (dict(pregate=True), dict(postgate=True), dict(pregate=True, postgate=True, taps=9),
               dict(pregate=True, postgate=True, io_dtype=torch.bfloat16), dict(postgate=True, io_dtype=torch.float16, taps=9),
               dict(pregate=True, postgate=True, taps=150, partition=9)):
        with pytest.raises(mf.MifftError) as e:  # (a valid request: as far as the device)
            mf.plan_fftconv_grad(f32, 2, 3, 40, 64, **kw)
        assert e.value.status == -10, kw


def test_fftconv_filter_grad_with_gates_validates_on_the_host():
    x, gy = torch.zeros(2, 3, 40), torch.zeros(2, 3, 40)  # (host tensors: nothing reaches the library)
    a, b = torch.ones(2, 3, 40), torch.ones(2, 3, 40)
    for kw, exc, status in (
            (dict(pregate=torch.ones(2, 3, 41)), ValueError, None),
            (dict(pregate=torch.ones(3, 40)), ValueError, None),       # (nothing is broadcast)
            (dict(pregate=torch.ones(1, 3, 40)), ValueError, None),
            (dict(postgate=torch.ones(2, 3, 39)), ValueError, None),
            (dict(pregate=a, postgate=torch.ones(2, 1, 40)), ValueError, None),
            (dict(pregate=a.to(torch.complex64)), mf.MifftError, -3),
            (dict(postgate=b.to(torch.complex128)), mf.MifftError, -3),
            (dict(pregate=a, postgate=b, io_dtype=torch.int8), mf.MifftError, -4),
            (dict(pregate=a, postgate=b, n=64, block=64), ValueError, None)):
        with pytest.raises(exc) as e:
            mf.fftconv_filter_grad(x, gy, 9, **kw)
        assert status is None or e.value.status == status, (kw, e.value)
    # "full": gy and the postgate have the result's 48 samples; a postgate of x's 40 is refused
    with pytest.raises(ValueError):
        mf.fftconv_filter_grad(x, torch.zeros(2, 3, 48), 9, mode="full", postgate=b)
    for kw in (dict(pregate=a), dict(postgate=b), dict(pregate=a, postgate=b, io_dtype=torch.bfloat16),
               dict(pregate=a, postgate=b, block=16, partition=5)):
        with pytest.raises(mf.MifftError) as e:  # (a valid request gets as far as the device check)
            mf.fftconv_filter_grad(x, gy, 9, **kw)
        assert e.value.status == -10, kw


# ---- the composed partitioned plan slices the gates as it slices x and gy ----------------------------------------------------
@pytest.mark.parametrize("L,Q,o,Lo,correlate,K", [(100, 9, 0, 100, False, 150), (100, 9, 0, 100, True, 150), (100, 9, 74, 100, False, 150),
                                                 (100, 9, 0, 249, False, 150), (40, 7, 12, 40, False, 30), (10, 9, 0, 10, True, 10)])
def test_partitions_slice_the_gates_as_x_and_gy(L, Q, o, Lo, correlate, K):
    rows = 4
    rng = np.random.default_rng(L + Q + o)
    x, a = (torch.from_numpy(rng.standard_normal((rows, L, 1))) for _ in range(2))
    gy, b = (torch.from_numpy(rng.standard_normal((rows, Lo, 1))) for _ in range(2))
    live = padded = 0
    for p in range(-(-K // Q)):
        sl = _fftconv_part_grad_slice(L, Q, o, Lo, correlate, p)
        if sl is None:
            continue
        live += 1
        u0, u1, g0, g1, _ = sl
        us, gs, pa, pb = _fftconv_part_grad_operands(sl, x, gy, a, b)
        w = max(u1 - u0, 2)
        padded += u1 - u0 < 2
        assert us.shape == pa.shape == (rows, w, 1) and gs.shape == pb.shape == (rows, g1 - g0, 1)
        assert all(t.is_contiguous() for t in (us, gs, pa, pb))
        assert torch.equal(us[:, :u1 - u0], x[:, u0:u1]) and torch.equal(pa[:, :u1 - u0], a[:, u0:u1])
        assert (us[:, u1 - u0:] == 0).all() and (pa[:, u1 - u0:] == 0).all()  # (the pregate is padded where x is)
        assert torch.equal(gs, gy[:, g0:g1]) and torch.equal(pb, b[:, g0:g1])
        # the operands of the gated sub-plan multiply to the operands the ungated sub-plan gets of the products
        ps, pg, none_a, none_b = _fftconv_part_grad_operands(sl, a * x, b * gy)
        assert none_a is None and none_b is None
        assert torch.equal(pa * us, ps) and torch.equal(pb * gs, pg)
    assert live >= 1
    if (L, Q, correlate) == (10, 9, True):
        assert padded == 1  # (partition 1 of a correlation reads the one sample u[9:10])
