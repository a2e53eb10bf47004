"""The STFT adjoint without a device: the fp64 numpy model of what the kernel computes (tests/stft_grad_reference.py) against
torch.autograd over torch.stft on the CPU, the dot-product identity, the tagged payload and its refusals through the C ABI
with device -1, and the layout of the exec's argument block."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib

from stft_grad_reference import SMALL_SHAPES, adjoint_model, frames_of, torch_stft, window_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISTFT, REFLECT, ZEROS = 0x4000, 64, 128
OK, NULL, BAD_DIM, NO_DEVICE, BAD_BASES, UNSUPPORTED, TOO_LARGE = 0, -11, -2, -10, -5, -15, -9
TAG = (mf.STFT_ADJ_TAG_LO, mf.STFT_ADJ_TAG_HI)
NAMES = "adjoint"


def _case(B, T, n, hop, centre, win, seed=0):
    torch.manual_seed(seed)
    w = window_of(win, n)
    x = torch.randn(B, T, dtype=torch.float64, requires_grad=True)
    X = torch_stft(x, n, hop, centre, w)
    return w, x, X


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_model_matches_torch_autograd(shape):
    B, T, n, hop, centre, win = shape
    w, x, X = _case(*shape)
    assert X.shape[-1] == frames_of(T, n, hop, centre)
    gX = torch.randn_like(X)
    (ref,) = torch.autograd.grad(X, x, gX, retain_graph=True)
    gx, out, edge = adjoint_model(gX.transpose(-1, -2).numpy(), None, 1, w, n, hop, T, centre)
    assert np.abs(gx - ref.numpy()).max() < 1e-12
    assert (edge is not None) == (centre == "reflect")
    Xf = X.detach().transpose(-1, -2).numpy()
    for mode, power in ((2, 2), (3, 1)):
        P = X.abs().pow(power)
        gP = torch.randn_like(P)
        (ref,) = torch.autograd.grad(P, x, gP, retain_graph=True)
        gx, _, _ = adjoint_model(Xf, gP.transpose(-1, -2).numpy(), mode, w, n, hop, T, centre)
        assert np.abs(gx - ref.numpy()).max() < 1e-12, (mode, shape)


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_dot_product_identity(shape):
    B, T, n, hop, centre, win = shape
    w, x, X = _case(*shape, seed=1)
    g = torch.randn_like(X)
    # <stft(x), g> with the real inner product Re sum conj(g) X, the pairing of torch's gradient convention
    lhs = float((X.detach().real * g.real + X.detach().imag * g.imag).sum())
    gx, _, _ = adjoint_model(g.transpose(-1, -2).numpy(), None, 1, w, n, hop, T, centre)
    rhs = float((x.detach().numpy() * gx).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_model_zero_magnitude_is_zero_gradient():
    """power 1 at |X| = 0: torch's abs backward gives 0, and so does the model's mode 3"""
    n, hop, T = 16, 4, 40
    X = np.zeros((1, frames_of(T, n, hop, None), n // 2 + 1), dtype=np.complex128)
    gx, _, _ = adjoint_model(X, np.ones(X.shape), 3, None, n, hop, T, None)
    assert np.all(gx == 0.0)


def _words(values):
    return [w for v in values for w in struct.unpack("<II", struct.pack("<d", float(v)))]


def _create(T=50, F=13, n=16, *, hop=4, center=REFLECT, extra=0, gain=1.0, mode=1, reserved=0, window=None, radices=(), tag=TAG,
            inverse=1, comps=2, dtype=0, len0=None, device=-1, tail=None):
    L = _lib.lib()
    h = ctypes.c_void_p()
    flat = _words([0.5] * n if window is None else window) + list(tag) + _words([gain]) + [mode, reserved]
    if tail is not None:
        flat = flat[:2 * n] + list(tail)
    lens = (ctypes.c_int32 * 3)(len(flat) if len0 is None else len0, 0, len(radices))
    flat = flat + list(radices)
    flags = ISTFT | center | (hop << 16) | extra
    rc = L.mifft_plan_create(ctypes.byref(h), device, dtype, dtype, 3, (ctypes.c_int64 * 3)(T, F, n), 3, comps, inverse,
                             (ctypes.c_uint32 * len(flat))(*flat), lens, flags)
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


def test_tagged_payload_is_accepted_up_to_the_device():
    for kw in (dict(), dict(mode=2), dict(mode=3), dict(center=ZEROS), dict(center=0, T=50, F=9), dict(dtype=1),
               dict(gain=0.125), dict(T=47, F=2, hop=16, center=0),      # T > L - c: lifted for the adjoint
               dict(T=9, F=3, hop=4)):                                   # n / 2 = T - 1
        rc, why = _create(**kw)
        assert rc == NO_DEVICE, (kw, rc, why)


@pytest.mark.parametrize("kw,status", [
    (dict(mode=0), BAD_BASES), (dict(mode=4), BAD_BASES), (dict(reserved=1), BAD_BASES),
    (dict(gain=0.0), BAD_BASES), (dict(gain=float("inf")), BAD_BASES), (dict(gain=float("nan")), BAD_BASES),
    (dict(hop=17, F=3), UNSUPPORTED), (dict(center=REFLECT | ZEROS), UNSUPPORTED), (dict(inverse=0), UNSUPPORTED),
    (dict(T=50, F=14), BAD_DIM),                       # the frames cover more than the padded signal
    (dict(T=8, F=3), BAD_DIM),                         # reflect with n / 2 > T - 1
    (dict(window=[0.5] * 15 + [float("nan")]), BAD_BASES),
    (dict(dtype=1, n=12288, T=40000, F=4, hop=12288 // 4 * 3, center=0), UNSUPPORTED),   # the fp64 carry limit
], ids=lambda v: None if isinstance(v, int) else ",".join(v))
def test_refusals_name_the_adjoint(kw, status):
    rc, why = _create(**kw)
    assert rc == status, (kw, rc, why)
    assert NAMES in why and "MIFFT_STFT_ADJ_TAG" in why, why


def _plain(n, flat, len0, T=100, F=9, hop=16):
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 3, (ctypes.c_int64 * 3)(T, F, n), 3, 2, 1,
                             (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * 3)(len0, 0, 0), ISTFT | (hop << 16))
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


def test_existing_istft_payload_lengths_answer_as_before():
    n = 16
    w = _words([1.0] * n)
    assert _plain(n, [], 0)[0] == NO_DEVICE
    assert _plain(n, w, 2 * n)[0] == NO_DEVICE
    assert _plain(n, w + _words([4.0]), 2 * n + 2)[0] == NO_DEVICE
    for bad in (2 * n + 1, 2 * n + 3, 2 * n + 5, 2 * n + 7):
        rc, why = _plain(n, w + [0] * 8, bad)
        assert rc == BAD_BASES and "bases_len[0] of an inverse STFT plan is 0" in why and NAMES not in why, (bad, rc, why)
    # 2 n + 6 words WITHOUT the tag: the length alone selects nothing
    rc, why = _plain(n, w + [0] * 6, 2 * n + 6)
    assert rc == BAD_BASES and "bases_len[0] of an inverse STFT plan is 0" in why and NAMES not in why
    # the untagged plan still refuses an output longer than the frames cover (the refusal the adjoint lifts)
    rc, why = _plain(n, w, 2 * n, T=200)
    assert rc == BAD_DIM and "a longer output is not zero-padded" in why


def test_args_block_matches_the_header():
    text = open(os.path.join(ROOT, "include", "mifft.h")).read()
    m = re.search(r"#define MIFFT_STFT_ADJ_ARGS_MAGIC (0x[0-9A-Fa-f]+)ull", text)
    assert m and int(m.group(1), 16) == mf.STFT_ADJ_ARGS_MAGIC
    assert struct.pack("<Q", mf.STFT_ADJ_ARGS_MAGIC) == b"MIFFTSA1"
    lo = re.search(r"#define MIFFT_STFT_ADJ_TAG_LO (0x[0-9A-Fa-f]+)u", text)
    hi = re.search(r"#define MIFFT_STFT_ADJ_TAG_HI (0x[0-9A-Fa-f]+)u", text)
    assert (int(lo.group(1), 16), int(hi.group(1), 16)) == TAG
    tag = struct.unpack("<d", struct.pack("<II", *TAG))[0]
    assert tag != tag  # a NaN: no window value, gain or scale can be mistaken for it
    body = re.search(r"typedef struct mifft_stft_adj_args \{(.*?)\} mifft_stft_adj_args;", text, re.S).group(1)
    fields = re.findall(r"(?:uint64_t|const void\*|void\*)\s+(\w+);", body)
    assert fields == ["magic", "x", "mult", "edge"] == [f[0] for f in mf.StftAdjArgs._fields_]
    assert ctypes.sizeof(mf.StftAdjArgs) == 32
    assert [getattr(mf.StftAdjArgs, f).offset for f in fields] == [0, 8, 16, 24]


def test_python_argument_errors_need_no_device():
    """the wrapper's own checks come before the device is asked for"""
    with pytest.raises(mf.MifftError) as e:
        mf.plan_stft_adjoint(torch.float32, 2, 50, 16, 4, multiplier=3)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        mf.plan_stft_adjoint(torch.float16, 2, 50, 16, 4)
    assert e.value.status == -4
    with pytest.raises(mf.MifftError) as e:
        mf.plan_stft_adjoint(torch.float32, 2, 50, 15, 4)
    assert e.value.status == UNSUPPORTED
