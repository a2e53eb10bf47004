"""The gradients of istft, mdct and imdct without a device: the fp64 numpy model of what the adjoint kernel computes
(tests/istft_grad_reference.py) against torch.autograd over torch.istft on the CPU, the payload of the new framed kind word by
word, every old kind's payload against tests/golden/framed_payloads.json, the MDCT / IMDCT transposition identities on a dense
cosine-matrix model, and the argument errors of plan_istft_adjoint, which the library raises before it looks for a device."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import istft_grad_reference as R  # noqa: E402
import test_framed_request_host as FR  # noqa: E402

NO_DEVICE = types.SimpleNamespace(device=-1)  # (the checks come first: an accepted request ends in status -10, no device)
IDS = lambda s: "x".join(str(v) for v in s)  # noqa: E731


@pytest.mark.parametrize("shape", R.SMALL_SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_matches_torch_autograd(shape, dtype):
    X, gy, gX = R.reference(shape, dtype)
    got = R.adjoint_model(gy, shape).transpose(0, 2, 1)
    assert got.shape == gX.shape
    assert np.abs(got - gX).max() < 1e-12
    N = shape[2] // 2
    assert (got[:, 0].imag == 0).all() and (got[:, N].imag == 0).all() and (gX[:, 0].imag == 0).all() and (gX[:, N].imag == 0).all()
    for f in R.ZERO_FRAMES.get(R.SMALL_SHAPES.index(shape), []):  # the frames that see no stored sample
        assert (gX[:, :, f] == 0).all() and (got[:, :, f] == 0).all(), f
    assert sorted(f for f in range(shape[1]) if (gX[:, :, f] == 0).all()) == R.ZERO_FRAMES.get(R.SMALL_SHAPES.index(shape), [])


@pytest.mark.parametrize("shape", R.SMALL_SHAPES, ids=IDS)
def test_model_dot_product_identity(shape):
    X, gy, _ = R.reference(shape, np.float64, seed=1)
    y = R.torch_istft(torch.from_numpy(X), shape).numpy()
    gX = R.adjoint_model(gy, shape).transpose(0, 2, 1)
    lhs, rhs = float((y * gy).sum()), float((X.real * gX.real + X.imag * gX.imag).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_impulse_closed_form_is_the_model():
    shape = R.SMALL_SHAPES[0]
    T = R.length_of(shape)
    for t0 in (0, T - 1, shape[3], 5):
        gy = np.zeros((1, T))
        gy[0, t0] = 1.0
        assert np.abs(R.adjoint_model(gy, shape)[0] - R.impulse_closed_form(shape, t0)).max() < 1e-14


# ---- the payload -------------------------------------------------------------------------------------------------------------------

def test_frame_payload_of_the_new_kind_word_by_word():
    n, hop, F = 16, 4, 13
    w = [(j + 1) / 16.0 for j in range(n)]
    r = api.FrameRequest("istft_adjoint", n, hop, center=True, window=w, gain=4.0, frames=F)
    bits, words, lead = api._frame_payload(r)
    assert (bits, lead) == (api.FLAG_STFT | hop << 16 | api.FLAG_STFT_CENTER_ZEROS, 1)
    assert len(words) == 2 * n + 6
    assert words[:2 * n] == api.window_words(w)
    assert words[2 * n:2 * n + 2] == [mf.ISTFT_ADJ_TAG_LO, mf.ISTFT_ADJ_TAG_HI] == [0x4A444901, 0x7FF84D4A]
    assert api.words_window(words[2 * n + 2:2 * n + 4]) == [4.0]
    assert words[2 * n + 4:] == [F, 0]
    # uncentred: no centre bit; no window: ones written out, the tag in the same place
    bits, words, _ = api._frame_payload(r._replace(center=False, window=None, gain=1.0))
    assert bits == api.FLAG_STFT | hop << 16
    assert words == api.window_words([1.0] * n) + [mf.ISTFT_ADJ_TAG_LO, mf.ISTFT_ADJ_TAG_HI] + api.window_words([1.0]) + [F, 0]
    assert api._frame_payload(r._replace(center="constant"))[0] == api.FLAG_STFT | hop << 16 | api.FLAG_STFT_CENTER_ZEROS
    with pytest.raises(mf.MifftError) as e:  # a window of another length than the frames
        api._frame_payload(r._replace(window=w[:-1]))
    assert e.value.status == -5
    with pytest.raises(mf.MifftError) as e:
        api._frame_payload(r._replace(center="reflect"))
    assert e.value.status == -15
    assert api.FrameRequest("stft", n, hop).frames == 0  # (the new field has a default: old constructions are unchanged)


def test_plan_istft_adjoint_reaches_the_library_as_its_payload_says(monkeypatch):
    n, hop, F, B = 16, 4, 13, 3
    w = [(j + 1) / 16.0 for j in range(n)]
    rec = FR.record(monkeypatch.setattr, lambda: mf.plan_istft_adjoint(torch.float64, B, F, n, hop, window=w, center=True, gain=4.0,
                                                                      length=40, ctx=FR.CTX))
    bits, words, lead = api._frame_payload(api.FrameRequest("istft_adjoint", n, hop, center=True, window=w, gain=4.0, frames=F))
    assert rec["flags"] == bits and rec["words"] == words and rec["lens"] == [len(words), 0]
    assert (rec["ndim"], rec["dims"], rec["batch"], rec["in_components"], rec["inverse"]) == (2, [40, n], B, 1, 0)


@pytest.mark.parametrize("name", sorted(FR.cases()))
def test_every_old_payload_is_unchanged(name, monkeypatch):
    call, _, _, computed = FR.cases()[name]
    assert FR.summary(FR.record(monkeypatch.setattr, call), computed) == FR.fixture()[name]


# ---- the MDCT pair: exact transposes of each other up to a scale -------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("T", [2, 7, 16, 29, 53])
def test_mdct_and_imdct_are_transposes_on_the_dense_model(n, T):
    rng = np.random.default_rng(n * 100 + T)
    w = rng.uniform(0.2, 1.5, 2 * n)   # not symmetric
    s, B = 0.37, 2
    x = rng.standard_normal((B, T))
    X = R.mdct_model(x, n, w, s)
    Fm = X.shape[1]
    assert Fm == mf.mdct_frames(T, n)
    Y = rng.standard_normal(X.shape)
    # <mdct(x), Y> == <x, imdct-with-gain-s(Y)>
    lhs, rhs = float((X * Y).sum()), float((x * R.imdct_model(Y, n, w, s, T)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # the converse, with more frames than the samples reach: <imdct(Z), gy> == <Z, mdct-with-scale-g(gy) zero-extended>
    F = Fm + 2
    Z = rng.standard_normal((B, F, n))
    gy = rng.standard_normal((B, T))
    gZ = np.zeros_like(Z)
    gZ[:, :Fm] = R.mdct_model(gy, n, w, s)
    lhs, rhs = float((R.imdct_model(Z, n, w, s, T) * gy).sum()), float((Z * gZ).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # and torch.autograd over the model agrees that the frames beyond mdct_frames(T, n) have a zero gradient
    Zt = torch.from_numpy(Z).requires_grad_(True)
    R.imdct_model(Zt, n, w, s, T).backward(torch.from_numpy(gy))
    assert np.abs(Zt.grad.numpy() - gZ).max() < 1e-12 and (Zt.grad.numpy()[:, Fm:] == 0).all()


# ---- argument errors, before any device work ---------------------------------------------------------------------------------------

def _status(**kw):
    args = dict(dtype=torch.float32, batch=2, frames=9, n_fft=16, hop_length=4, center=True, ctx=NO_DEVICE)
    args.update(kw)
    with pytest.raises(mf.MifftError) as e:
        mf.plan_istft_adjoint(args.pop("dtype"), args.pop("batch"), args.pop("frames"), args.pop("n_fft"), args.pop("hop_length"), **args)
    return e.value.status, str(e.value)


def test_plan_istft_adjoint_argument_errors():
    assert _status()[0] == -10                                   # accepted: only the device is missing
    assert _status(center=False, length=30)[0] == -10
    assert _status(window=np.hanning(17)[:16] + 0.1, gain=4.0)[0] == -10
    assert _status(dtype=torch.float16)[0] == -4
    assert _status(n_fft=15)[0] == -15
    assert _status(hop_length=17)[0] == -15                      # hop > n: gaps between the frames
    assert _status(hop_length=0)[0] == -15
    assert _status(length=49)[0] == -2                           # more than the frames cover (48)
    assert _status(frames=0)[0] == -2
    assert _status(center="reflect")[0] == -15
    assert _status(window=[1.0] * 15)[0] == -5
    assert _status(gain=0.0)[0] == -5
    assert _status(gain=float("nan"))[0] == -5
    st, msg = _status(window=[0.0] * 8 + [1.0] * 8, hop_length=16, frames=3)  # the envelope vanishes inside the stored range
    assert st == -15 and "overlap-add" in msg


def test_library_refusals_of_the_tagged_payload():
    """through Plan itself, so that the library's own checks answer (device -1: they run before the device is looked for)"""
    n, hop, F, B, T = 16, 4, 9, 2, 32

    def status(in_shape=(B, T, 1), out_shape=(B, F, n // 2 + 1, 2), **kw):
        args = dict(device=-1, stft_hop=hop, stft_center=True, istft_adjoint=F)
        args.update(kw)
        with pytest.raises(mf.MifftError) as e:
            mf.Plan(torch.float32, torch.float32, in_shape, out_shape, **args)
        return e.value.status, str(e.value)

    assert status()[0] == -10
    assert status(stft_power=2)[0] == -15
    assert status(istft_adjoint=F + 1)[0] == -2                  # out has F frames
    assert status(stft_center="reflect")[0] == -15
    st, msg = status(stft_window=[0.0] * n)
    assert st == -15 and "overlap-add" in msg
    st, msg = status(stft_window=[float("inf")] + [1.0] * (n - 1))
    assert st == -5 and "not finite" in msg
    # the raw ABI: the reflect bit, a reserved word, a frame count of zero, inverse = 1
    import ctypes
    from hackathon_fft_amd import _lib
    bits, words, _ = api._frame_payload(api.FrameRequest("istft_adjoint", n, hop, center=True, frames=F))

    def raw(flags=bits, words=words, inverse=0, dims=(T, n)):
        h = ctypes.c_void_p()
        flat = (ctypes.c_uint32 * len(words))(*words)
        lens = (ctypes.c_int32 * 2)(len(words), 0)
        return _lib.lib().mifft_plan_create_slab(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(*dims), B, 1, inverse, flat, lens,
                                                 flags, 0), _lib.lib().mifft_last_error().decode()

    code = raw()[0]
    assert code == -10, raw()
    st, msg = raw(flags=(bits & ~api.FLAG_STFT_CENTER_ZEROS) | api.FLAG_STFT_CENTER_REFLECT)
    assert st == -15 and "MIFFT_FLAG_STFT_CENTER_REFLECT" in msg
    assert raw(words=words[:-1] + [1])[0] == -5
    assert raw(words=words[:-2] + [0, 0])[0] == -2
    assert raw(inverse=1)[0] == -15
    st, msg = raw(dims=(49, n))
    assert st == -2 and "cover" in msg
