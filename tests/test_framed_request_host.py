"""The framed family's requests (STFT, spectrogram, inverse STFT, STFT adjoint, MDCT, IMDCT) between ``Plan(...)`` and the C
ABI, with no device: what ``mifft_plan_create_slab`` is handed for every branch of the encoder, pinned against
tests/golden/framed_payloads.json (recorded on the commit before ``FrameRequest`` existed: ``python
tests/test_framed_request_host.py`` rewrites it from the tree it runs in), ``_frame_payload`` called directly, and the cache
key of every wrapper that keeps its plans."""
import functools
import hashlib
import json
import math
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
import hackathon_fft_amd as mf  # noqa: E402
from hackathon_fft_amd import _lib, api  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "framed_payloads.json")
F32, F64 = torch.float32, torch.float64
N, HOP, T, B, M = 16, 4, 100, 3, 8          # the smallest shapes that take every branch of the encoder
BINS, FU, FC, FM = N // 2 + 1, 22, 26, 14   # frames: uncentred, centred, MDCT
CTX = types.SimpleNamespace(device=0)       # (plan_* read the device of their ctx and nothing else)
STFT, ISTFT, REFLECT, POWER = api.FLAG_STFT, api.FLAG_ISTFT, api.FLAG_STFT_CENTER_REFLECT, api.FLAG_STFT_POWER
# by-value tables of exactly representable values; the Hann window (a cosine: not every libm's bits) travels in the fixture
RAMP = [(j + 1) / 16.0 for j in range(N)]
FB = (np.arange(BINS * 3, dtype=np.float64).reshape(BINS, 3) - 5.0) / 32.0
POST = np.array([[1.0, 0.5], [-0.25, 2.0], [0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def hann():
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            return json.load(f)["hann16"]
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).tolist()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (the call, dict(FrameRequest fields) or None, the radices behind the payload, computed doubles {index: value}):
    ``computed`` are payload values that come out of a libm call (the default MDCT window, ln 2 ..): they are compared with
    the same call made here and left out of the digest"""
    H = hann()
    out = {}

    def add(name, call, req=None, radices=(), computed=None):
        assert name not in out
        out[name] = (call, req, list(radices), computed or {})

    sine = {j: float(v) for j, v in enumerate(mf.mdct_window(M).tolist())}
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        # ---- stft ------------------------------------------------------------------------------------------------------------
        for center, F in ((None, FU), ("reflect", FC), ("constant", FC)):
            for wname, w in (("none", None), ("hann", H)):
                add(f"stft-{tag}-{center}-{wname}",
                    lambda dt=dt, center=center, w=w: mf.plan_stft(dt, B, T, N, HOP, window=w, center=center, ctx=CTX),
                    dict(kind="stft", n=N, hop=HOP, center=center, window=w))
        add(f"stft-{tag}-bases", lambda dt=dt: mf.Plan(dt, dt, (B, T, 1), (B, FU, BINS, 2), stft_hop=HOP, bases=[[], [2]]),
            dict(kind="stft", n=N, hop=HOP), [2])
        # ---- spectrogram -----------------------------------------------------------------------------------------------------
        for name, kw, req in (("p1", dict(power=1), dict(power=1)), ("p2", dict(power=2), dict(power=2)),
                              ("p2-hann", dict(power=2, window=H), dict(power=2, window=H)),
                              ("fb", dict(power=2, fb=FB), dict(power=2, fb=FB)),
                              ("fb-post", dict(power=1, fb=FB, post=POST, window=H), dict(power=1, fb=FB, post=POST, window=H))):
            add(f"spec-{tag}-{name}", lambda dt=dt, kw=kw: mf.plan_spectrogram(dt, B, T, N, HOP, center="reflect", ctx=CTX, **kw),
                dict(kind="spec", n=N, hop=HOP, center="reflect", **req))
        for log, a in (("log", math.log(2.0)), ("log10", math.log10(2.0)), ("db", 10.0 * math.log10(2.0))):
            logv = (0.0, 1e-10, a, 0.0 if log != "db" else -10.0 * math.log10(1.0))
            add(f"spec-{tag}-fb-{log}", lambda dt=dt, log=log: mf.plan_spectrogram(dt, B, T, N, HOP, fb=FB, log=log, ctx=CTX),
                dict(kind="spec", n=N, hop=HOP, power=2, fb=FB, log=logv), computed={N + 1 + 6: a})
        add(f"spec-{tag}-log-post",
            lambda dt=dt: mf.plan_spectrogram(dt, B, T, N, HOP, fb=FB, log="log10", post=POST, window=H, ctx=CTX),
            dict(kind="spec", n=N, hop=HOP, power=2, fb=FB, log=(0.0, 1e-10, math.log10(2.0), 0.0), post=POST, window=H),
            computed={N + 1 + 6: math.log10(2.0)})
        add(f"spec-{tag}-log-exact",
            lambda dt=dt: mf.Plan(dt, dt, (B, T, 1), (B, FU, BINS, 1), stft_hop=HOP, stft_power=2, stft_log=(0.5, 2.0 ** -20, 0.25, 1.0)),
            dict(kind="spec", n=N, hop=HOP, power=2, log=(0.5, 2.0 ** -20, 0.25, 1.0)))
        # ---- istft -----------------------------------------------------------------------------------------------------------
        for name, kw, req in (("plain", {}, {}), ("window", dict(window=H), dict(window=H)),
                              ("gain", dict(normalized=True), dict(gain=4.0)),
                              ("window-gain", dict(window=H, normalized=True), dict(window=H, gain=4.0))):
            for center in (False, True, "constant"):
                add(f"istft-{tag}-{name}-{center}",
                    lambda dt=dt, kw=kw, center=center: mf.plan_istft(dt, B, FU, N, HOP, center=center, ctx=CTX, **kw),
                    dict(kind="istft", n=N, hop=HOP, center=center, **req))
        add(f"istft-{tag}-bases",
            lambda dt=dt: mf.Plan(dt, dt, (B, FU, BINS, 2), (B, T, 1), istft_hop=HOP, stft_window=H, bases=[[], [], [2]]),
            dict(kind="istft", n=N, hop=HOP, window=H), [2])
        # ---- the STFT adjoint ------------------------------------------------------------------------------------------------
        for mode, mult in ((1, None), (2, 2), (3, 1)):
            for center in (None, "reflect", "constant"):
                add(f"adjoint-{tag}-{mode}-{center}",
                    lambda dt=dt, mode=mode, mult=mult, center=center: mf.plan_stft_adjoint(dt, B, T, N, HOP, window=H if mode == 2 else None,
                                                                                  center=center, multiplier=mult, ctx=CTX),
                    dict(kind="adjoint", n=N, hop=HOP, center=center, window=H if mode == 2 else None, adjoint=mode))
        # ---- MDCT and IMDCT ------------------------------------------------------------------------------------------------
        for norm, scale, gain in ((None, 1.0, 0.25), ("ortho", 0.5, 0.5)):
            for wname, w in (("default", None), ("ramp", RAMP)):
                add(f"mdct-{tag}-{norm}-{wname}", lambda dt=dt, norm=norm, w=w: mf.plan_mdct(dt, B, T, M, window=w, norm=norm, ctx=CTX),
                    dict(kind="mdct", n=2 * M, hop=M, window=w, gain=scale), computed=sine if w is None else None)
                add(f"imdct-{tag}-{norm}-{wname}", lambda dt=dt, norm=norm, w=w: mf.plan_imdct(dt, B, FM, M, window=w, norm=norm, ctx=CTX),
                    dict(kind="imdct", n=2 * M, hop=M, window=w, gain=gain), computed=sine if w is None else None)
    # ---- requests that are flag bits alone ---------------------------------------------------------------------------------
    add("bits-stft", lambda: mf.Plan(F32, F32, (B, T, 1), (B, FC, BINS, 2), flags=STFT | api.FLAG_STFT_HOP(HOP) | REFLECT),
        dict(kind="stft", n=N, hop=HOP, center="reflect"))
    add("bits-istft", lambda: mf.Plan(F32, F32, (B, FU, BINS, 2), (B, T, 1), flags=ISTFT | api.FLAG_STFT_HOP(HOP), inverse=True),
        dict(kind="istft", n=N, hop=HOP))
    # ---- pairs that the library refuses: the recorded FLAGS are what matters --------------------------------------------
    add("pair-stft-dct", lambda: mf.Plan(F32, F32, (B, T, 1), (B, FU, BINS, 2), stft_hop=HOP, dct=True))
    add("pair-istft-stft", lambda: mf.Plan(F32, F32, (B, FU, BINS, 2), (B, T, 1), istft_hop=HOP, stft_hop=HOP))
    add("pair-istft-dct", lambda: mf.Plan(F32, F32, (B, FU, BINS, 2), (B, T, 1), istft_hop=HOP, dct=True))
    add("pair-mdct-half", lambda: mf.Plan(F32, F32, (B, T, 1), (B, FM, M, 1), mdct=M, half_spectrum=True))
    return out


def record(monkeypatch_setattr, call):
    """what ``call`` hands to mifft_plan_create_slab, the library's entry replaced by a recorder that makes no plan"""
    seen = []

    def create(h, device, in_code, out_code, ndim, dims, batch, comps, inverse, flat, lens, flags, whole_batch):
        lens_ = None if lens is None else list(lens)
        seen.append(dict(in_code=in_code, out_code=out_code, ndim=ndim, dims=list(dims[:ndim]), batch=batch, in_components=comps,
                         inverse=inverse, lens=lens_, flags=flags, whole_batch=whole_batch,
                         words=None if flat is None else list(flat[:max(sum(lens_), 0)])))
        return 0

    monkeypatch_setattr(_lib.lib(), "mifft_plan_create_slab", create)
    call()
    assert len(seen) == 1
    return seen[0]


def digest(words, computed):
    """SHA-256 of the flat words, the ``computed`` doubles zeroed (None: no bases at all)"""
    if words is None:
        return None
    words = list(words)
    for j in computed:
        words[2 * j:2 * j + 2] = [0, 0]
    return hashlib.sha256(np.asarray(words, dtype="<u4").tobytes()).hexdigest()


def summary(rec, computed):
    out = {k: v for k, v in rec.items() if k != "words"}
    out["n_words"] = None if rec["words"] is None else len(rec["words"])
    out["sha256"] = digest(rec["words"], computed)
    return out


def fixture():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_fixture_covers_the_case_list():
    assert sorted(fixture()) == sorted(cases())


@pytest.mark.parametrize("name", sorted(cases()))
def test_request_reaches_the_library_as_recorded(name, monkeypatch):
    call, req, radices, computed = cases()[name]
    rec = record(monkeypatch.setattr, call)
    assert summary(rec, computed) == fixture()[name]
    for j, v in computed.items():  # (bit for bit what the same libm call gives here)
        assert rec["words"][2 * j:2 * j + 2] == list(struct.unpack("<2I", struct.pack("<d", v))), (name, j)
    if req is None:
        return
    bits, words, lead = api._frame_payload(api.FrameRequest(**req))
    assert bits & rec["flags"] == bits and rec["flags"] & ~bits & ~api.FLAG_KEEP_MASK == 0, (name, hex(bits), hex(rec["flags"]))
    assert lead == rec["ndim"] - 1
    if rec["words"] is None:
        assert words == [] and not radices
    else:
        assert words + radices == rec["words"] and rec["lens"] == [len(words)] + [0] * (lead - 1) + [len(radices)]


def test_frame_payload_is_pure_and_names_its_layouts():
    """no device, no library: the five layouts by their lengths and tags"""
    w = [1.0] * N
    r = api.FrameRequest("stft", N, HOP)
    assert api._frame_payload(r) == (STFT | HOP << 16, [], 1)
    assert api._frame_payload(r._replace(window=w))[1] == api.window_words(w)
    spec = api._frame_payload(r._replace(kind="spec", power=2, fb=FB))[1]                      # w | power | fb
    assert len(spec) == 2 * (N + 1 + FB.size) and spec[:2 * N] == api.window_words(w) and api.words_window(spec[2 * N:2 * N + 2]) == [2.0]
    ext = api._frame_payload(r._replace(kind="spec", power=1, fb=FB, post=POST))[1]            # w | EXT_TAG | 8 values | fb | post
    assert ext[2 * N:2 * N + 2] == [api.STFT_EXT_TAG_LO, api.STFT_EXT_TAG_HI] and len(ext) == 2 * (N + 1 + 8 + FB.size + POST.size)
    assert api.words_window(ext[2 * N + 2:2 * N + 18]) == [1.0, 3.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    inv = r._replace(kind="istft")
    assert api._frame_payload(inv) == (ISTFT | HOP << 16, [], 2)
    assert api._frame_payload(inv._replace(gain=4.0))[1] == api.window_words(w + [4.0])         # w | gain
    adj = api._frame_payload(inv._replace(kind="adjoint", adjoint=3, center="reflect"))        # w | TAG | gain | mode, 0
    assert adj[0] == ISTFT | HOP << 16 | REFLECT
    assert adj[1] == api.window_words(w) + [api.STFT_ADJ_TAG_LO, api.STFT_ADJ_TAG_HI] + api.window_words([1.0]) + [3, 0]
    for kind, bit, lead in (("mdct", STFT, 1), ("imdct", ISTFT, 2)):                            # w | TAG | scale
        bits, words, ld = api._frame_payload(api.FrameRequest(kind, 2 * M, M, window=RAMP, gain=0.5))
        assert (bits, ld) == (bit | M << 16 | api.FLAG_STFT_CENTER_ZEROS, lead)
        assert words == api.window_words(RAMP) + [api.MDCT_TAG_LO, api.MDCT_TAG_HI] + api.window_words([0.5])
    with pytest.raises(mf.MifftError) as e:  # a window of another length than the frames
        api._frame_payload(r._replace(window=[1.0] * (N - 1)))
    assert e.value.status == -5
    conv = api.ConvRequest(64, 3, 0, 37)     # the conv kinds through the same door
    assert api._frame_payload(conv) == (STFT, api._conv_payload(conv), 1)


# ---- the wrappers' cache keys ----------------------------------------------------------------------------------------------------
class FakeTensor:
    """what the wrappers ask of their input before the plan is looked up"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True
        self.device = types.SimpleNamespace(index=0)

    def is_complex(self):
        return self.dtype.is_complex

    def dim(self):
        return len(self.shape)

    def reshape(self, shape):
        return FakeTensor(shape, self.dtype)

    def to(self, dtype):
        return FakeTensor(self.shape, dtype)

    def contiguous(self):
        return self

    def transpose(self, a, b):
        return self


class Stop(Exception):
    pass


def sha1(t):
    return hashlib.sha1(np.ascontiguousarray(np.asarray(t, dtype=np.float64)).tobytes()).digest()


def test_cache_keys_are_what_they_were(monkeypatch):
    """one call of each of the eight sites that keep plans, the plan builders replaced by a stub: the key under which the
    plan is kept is the tuple the site has always built (device 0, stream handle 0x5EED)"""
    keys = []

    def stub(*a, **k):
        raise Stop

    for name in ("Plan", "plan_fft", "plan_fftconv", "plan_fftconv_grad", "plan_stft_adjoint"):
        monkeypatch.setattr(api, name, stub)
    monkeypatch.setattr(api, "DeviceContext", lambda device=None, stream=None: types.SimpleNamespace(device=0 if device is None else device))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0x5EED))
    real_get = api._PLAN_CACHE.get
    monkeypatch.setattr(api, "_PLAN_CACHE", types.SimpleNamespace(get=lambda key: keys.append(key) or real_get(key)))
    S = 0x5EED
    H = torch.tensor(RAMP, dtype=F64)
    W2 = torch.tensor(RAMP, dtype=F64)
    x = FakeTensor((B, T), F32)

    def key_of(call):
        del keys[:]
        with pytest.raises(Stop):
            call()
        assert len(keys) == 1
        return keys[0]

    assert key_of(lambda: api._cached_plan(F32, F32, (B, N, 2), (B, N, 2), [[2]], False, False, 0)) == \
        (F32, F32, (B, N, 2), (B, N, 2), ((2,),), False, False, 0, S, False, 0, 0)
    assert key_of(lambda: api._cached_plan(F32, F32, (B, N, 1), (B, N, 1), None, True, False, 0, dct_flags=api.FLAG_DCT, dct_type=4,
                                           dst=True)) == \
        (F32, F32, (B, N, 1), (B, N, 1), None, True, False, 0, S, False, 0, api.FLAG_DCT, 4, "dst")
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    monkeypatch.setattr(torch, "view_as_real", lambda t: t)
    assert key_of(lambda: mf.mdct(x, M, window=W2, norm="ortho")) == ("mdct", F32, (B, T, 1), M, 0.5, sha1(RAMP), 0, S)
    assert key_of(lambda: mf.mdct(x, M)) == ("mdct", F32, (B, T, 1), M, 1.0, None, 0, S)
    assert key_of(lambda: mf.imdct(FakeTensor((B, FM, M), F64), window=W2, length=50)) == \
        ("imdct", F64, (B, FM, M, 1), 50, 0.25, sha1(RAMP), 0, S)
    assert key_of(lambda: mf.stft(x, N, HOP, window=H)) == ("stft", F32, (B, T, 1), N, HOP, "reflect", sha1(RAMP), 0, S)
    assert key_of(lambda: mf.stft(x, N, HOP, center=False)) == ("stft", F32, (B, T, 1), N, HOP, None, None, 0, S)
    assert key_of(lambda: mf.spectrogram(x, N, HOP, power=1, fb=FB)) == \
        ("stft", F32, (B, T, 1), N, HOP, "reflect", None, 0, S, 1, ((BINS, 3), sha1(FB)))
    logv = (0.0, 1e-10, math.log10(2.0), 0.0)
    assert key_of(lambda: mf.spectrogram(x, N, HOP, fb=FB, log="log10", post=POST)) == \
        ("stft", F32, (B, T, 1), N, HOP, "reflect", None, 0, S, 2, ((BINS, 3), sha1(FB)), logv, ((3, 2), sha1(POST)))
    assert key_of(lambda: mf.spectrogram(x, N, HOP, log="log10")) == \
        ("stft", F32, (B, T, 1), N, HOP, "reflect", None, 0, S, 2, None, logv, None)
    assert key_of(lambda: mf.istft(FakeTensor((B, BINS, FU), torch.complex64), N, HOP, window=H, center=False, normalized=True)) == \
        ("istft", F32, (B, FU, BINS, 2), N, HOP, False, T, 4.0, sha1(RAMP), 0, S)
    call = api._StftCall("stft", F64, B, T, N, HOP, True, "constant", H, None, None, None, None, 0)
    assert key_of(lambda: api._stft_adjoint_plan(call, 2)) == \
        ("stft_adjoint", F64, (B, T), N, HOP, "constant", sha1(RAMP), 2, 0, S)
    with api._PLAN_CACHE_LOCK:
        assert key_of(lambda: api._fftconv_fwd_plan(F32, 6, 3, T, 128, None, 0, T, False, 0, 3, None, torch.bfloat16)) == \
            ("fftconv", F32, 6, 3, T, 128, 0, T, False, 0, S, None, 3, None, torch.bfloat16)
        assert key_of(lambda: api._fftconv_grad_plan(F32, 6, 3, T, 128, 40, 0, T, True, 0, 8, None, 1)) == \
            ("fftconv_grad", F32, 6, 3, T, 128, 0, T, True, 0, S, 40, 8, None, 1)


if __name__ == "__main__":
    class _Patch:
        def __init__(self):
            self.undo = []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

    fixture = {"hann16": hann(), "cases": {}}
    for _name, (_call, _req, _radices, _computed) in sorted(cases().items()):
        _p = _Patch()
        fixture["cases"][_name] = summary(record(_p.setattr, _call), _computed)
        for _obj, _attr, _old in _p.undo:
            setattr(_obj, _attr, _old)
    with open(GOLDEN, "w") as _f:
        json.dump(fixture, _f, indent=1, sort_keys=True)
        _f.write("\n")
    print(f"{len(fixture['cases'])} cases -> {GOLDEN}")
