"""One plan per stream, and reuse: the rule every wrapper that keeps plans gets from the one cache helper (api._plan_cached).
Each wrapper is called twice on one stream and once on a second one: two plans of its kind are kept, not three and not one,
and the three results are the same bits."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import api

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HOP, T, B, M = 16, 4, 100, 3, 8


def _inputs():
    rng = np.random.default_rng(20)
    x = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)).to(DEV)
    w = torch.hann_window(N, periodic=True, dtype=torch.float64)
    fb = mf.melscale_fbanks(N // 2 + 1, 0.0, 8000.0, 5, 16000)
    X = torch.from_numpy((rng.standard_normal((B, N // 2 + 1, 22)) + 1j * rng.standard_normal((B, N // 2 + 1, 22))).astype(np.complex64)).to(DEV)
    X[:, 0].imag.zero_()
    X[:, -1].imag.zero_()
    C = torch.from_numpy(rng.standard_normal((B, 14, M)).astype(np.float32)).to(DEV)
    k = torch.from_numpy(rng.standard_normal(5).astype(np.float32)).to(DEV)
    return {"stft": lambda: mf.stft(x, N, HOP, window=w),
            "spectrogram": lambda: mf.spectrogram(x, N, HOP, window=w, fb=fb, log="db", post=mf.create_dct(3, 5)),
            "istft": lambda: mf.istft(X, N, HOP, window=w),
            "mdct": lambda: mf.mdct(x, M),
            "imdct": lambda: mf.imdct(C),
            "fftconv": lambda: mf.fftconv(x, k)}


# (the first word of the wrapper's cache keys; fftconv also keeps the rfftn plan that transforms its filter, under a key of
#  that family, so the plans are counted by their kind)
HEAD = {"stft": "stft", "spectrogram": "stft", "istft": "istft", "mdct": "mdct", "imdct": "imdct", "fftconv": "fftconv"}


@pytest.mark.parametrize("name", sorted(HEAD))
def test_one_plan_per_stream_and_reuse(name):
    call = _inputs()[name]
    mf.clear_plan_cache()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for st in (s1, s1, s2):
        with torch.cuda.stream(st):
            outs.append(call())
    torch.cuda.synchronize()
    kept = [key for key in api._PLAN_CACHE if key[0] == HEAD[name]]
    assert len(kept) == 2, kept
    assert len(kept[0]) == len(kept[1]) and sum(a != b for a, b in zip(*kept)) == 1  # (they differ in the stream alone)
    assert not torch.isnan(torch.view_as_real(outs[0]) if outs[0].is_complex() else outs[0]).any()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    mf.clear_plan_cache()
