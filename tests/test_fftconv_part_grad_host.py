"""The fused partitioned filter gradient without a device (FusedPartConvGradPlan, plan_fftconv_grad(fused=True)): the one
geometry function against brute force, an fp64 numpy model of its two stages -- every u-frame and every g-block transformed
once, then the lag-group sums over stored spectra -- against the direct double sum, the dead frames, the slab split, the
argument errors raised before any device work, the selector, and the staged MIFFT_CONV_GRAD_TAG payloads through the C ABI.
The GPU tests (test_gpu_fftconv_part_grad.py) use the direct sum defined here."""
import os
import re

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import api
from hackathon_fft_amd.api import ConvRequest, _conv_payload
from test_fftconv_grad_host import _create

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -15

NS = (8, 16, 20, 32)
SHAPES = ((37, 37, 37, 0), (50, 86, 37, 0), (50, 50, 37, 18), (50, 14, 37, 36), (33, 40, 70, 5), (9, 3, 29, 0))  # (L, Lo, K, o)
CASES = [(n, L, Lo, K, o, c) for n in NS for (L, Lo, K, o) in SHAPES for c in (False, True)]


def direct_gk(u, gv, D, K, o, correlate):
    """gk[d, j] = sum_b sum_t gv[b, d, t] u[b, d, o + t - j] (correlate: o + t + j), zeros outside the rows: the direct fp64
    double sum, tap by tap.  u (B D, L), gv (B D, Lo) -> (D, K)"""
    u, gv = np.asarray(u, dtype=np.float64), np.asarray(gv, dtype=np.float64)
    R, L = u.shape
    Lo = gv.shape[1]
    pad = K + Lo + abs(o)
    up = np.concatenate([np.zeros((R, pad)), u, np.zeros((R, pad))], axis=1)
    gk = np.zeros((D, K))
    for r in range(R):
        for j in range(K):
            s = pad + o + (j if correlate else -j)
            gk[r % D, j] += np.dot(gv[r], up[r, s:s + Lo])
    return gk


def brute_geometry(n, L, Lo, K, o, correlate):
    """what the table of the geometry says, sample by sample: for every tap j and sample t the lag group, the g-block, the
    u-frame they meet in, and the live frames"""
    H = n // 2
    Pg, Fg = -(-K // H), -(-Lo // H)
    frames = set()
    for p in range(Pg):
        for f in range(Fg):
            frames.add(f + p if correlate else f - p)
    start = lambda m: o + m * H - (0 if correlate else H)
    live = {m for m in frames if any(0 <= start(m) + i < L for i in range(n))}
    return H, Pg, Fg, frames, live, start


@pytest.mark.parametrize("n,L,Lo,K,o,correlate", CASES, ids=lambda v: str(v))
def test_the_geometry_function_against_brute_force(n, L, Lo, K, o, correlate):
    g = api._fftconv_fused_grad_geometry(n, L, Lo, K, o, correlate)
    H, Pg, Fg, frames, live, start = brute_geometry(n, L, Lo, K, o, correlate)
    assert (g.H, g.Pg, g.Fg, g.c) == (H, Pg, Fg, 0 if correlate else H)
    assert set(range(g.m_lo, g.m_hi + 1)) == frames
    assert all(g.frame_start(m) == start(m) for m in frames)
    # the dead frames are exactly the ones the function marks, and the live ones are one contiguous run
    assert {m for m in frames if g.live(m)} == live
    assert live == set(range(g.u_first, g.u_first + g.Fu))
    if g.Fu:
        assert g.u_start == start(g.u_first) and -n < g.u_start and g.u_start + (g.Fu - 1) * H < L
    # every pair (t, j) that meets a sample of u lies in the frame the table names, at the index the correlation needs
    for j in range(K):
        p, l = divmod(j, H)
        for t in range(Lo):
            f, i = divmod(t, H)
            s = o + t + j if correlate else o + t - j
            m = g.lag_frame(f, p)
            assert g.m_lo <= m <= g.m_hi
            at = s - g.frame_start(m)  # (where the sample sits in its frame)
            assert at == (i + l if correlate else H + i - l) and 0 <= at < n
            if 0 <= s < L:
                assert g.live(m)
    # the taps a pair of samples can reach
    j0, j1 = g.reachable
    can = {j for j in range(K) for t in range(Lo) if 0 <= (o + t + j if correlate else o + t - j) < L}
    assert can == set(range(j0, j1))


def two_stage_model(u, gv, D, n, K, o, correlate, slabs=None):
    """the fp64 model of the two stages: rfft of every live u-frame and of every g-block ONCE, the lag-group sums over the
    stored spectra in the kernel's order (slabs ascending, b ascending, f ascending), irfft, the first H lags of every group"""
    u, gv = np.asarray(u, dtype=np.float64), np.asarray(gv, dtype=np.float64)
    R, L = u.shape
    Lo, B = gv.shape[1], R // D
    g = api._fftconv_fused_grad_geometry(n, L, Lo, K, o, correlate)
    H = g.H
    transforms = 0
    U = np.zeros((R, max(g.Fu, 1), n // 2 + 1), dtype=np.complex128)
    G = np.zeros((R, g.Fg, n // 2 + 1), dtype=np.complex128)
    for r in range(R):
        for j in range(g.Fu):
            src = g.u_start + j * H + np.arange(n)
            U[r, j] = np.fft.rfft(np.where((src >= 0) & (src < L), u[r, np.clip(src, 0, L - 1)], 0.0))
            transforms += 1
        for f in range(g.Fg):
            blk = np.zeros(n)
            seg = gv[r, f * H:min(Lo, (f + 1) * H)]
            blk[g.c:g.c + len(seg)] = seg
            G[r, f] = np.fft.rfft(blk)
            transforms += 1
    parts = []
    for b0, b1 in (slabs or [(0, B)]):
        A = np.zeros((D, g.Pg, n // 2 + 1), dtype=np.complex128)
        for d in range(D):
            for b in range(b0, b1):
                r = b * D + d
                for f in range(g.Fg):
                    for p in range(g.Pg):
                        m = g.lag_frame(f, p)
                        if g.live(m):  # (a dead frame is zero and is not read)
                            A[d, p] += np.conj(U[r, m - g.u_first]) * G[r, f]
        parts.append(np.conj(A) if correlate else A)
    A = np.sum(parts, axis=0)
    gk = np.fft.irfft(A, n, axis=-1)[:, :, :H].reshape(D, g.Pg * H)[:, :K]
    return gk, transforms, U, G, g


@pytest.mark.parametrize("n,L,Lo,K,o,correlate", CASES, ids=lambda v: str(v))
def test_the_two_stage_model_equals_the_direct_double_sum(n, L, Lo, K, o, correlate):
    rng = np.random.default_rng(n * 1000 + L + Lo + K + o)
    D, B = 2, 3
    u, gv = rng.standard_normal((B * D, L)), rng.standard_normal((B * D, Lo))
    want = direct_gk(u, gv, D, K, o, correlate)
    got, transforms, _, _, g = two_stage_model(u, gv, D, n, K, o, correlate)
    assert transforms == B * D * (g.Fu + g.Fg)  # (every block once)
    scale = max(np.abs(want).max(), 1.0)
    assert np.abs(got - want).max() <= 1e-12 * scale, np.abs(got - want).max()
    # the same sums cut into slabs, one partial each
    sl = api._fftconv_fused_grad_slabs(B, 10, 10)
    assert sl == [(0, 1), (1, 2), (2, 3)]
    again, _, _, _, _ = two_stage_model(u, gv, D, n, K, o, correlate, slabs=sl)
    assert np.abs(again - want).max() <= 1e-12 * scale
    # taps that no pair of samples reaches are zero in the direct sum
    j0, j1 = g.reachable
    assert (want[:, :j0] == 0).all() and (want[:, j1:] == 0).all()


def test_the_transform_count_of_the_issue():
    # L = K = 65536 at n = 16384, causal: 8 live u-frames and 8 g-blocks per row, where the composed plan makes about 72
    g = api._fftconv_fused_grad_geometry(16384, 65536, 65536, 65536, 0, False)
    assert (g.H, g.Pg, g.Fg) == (8192, 8, 8) and g.Fu + g.Fg <= 9 + 8
    assert (g.m_lo, g.m_hi, g.u_first) == (-7, 7, 0)  # (the seven frames before the row are dead)
    assert g.reachable == (0, 65536)


def test_the_slab_split():
    for B in (1, 2, 5, 7, 64):
        for per in (1, 2, 3, 5, 64, 1000):
            entry = 1000
            sl = api._fftconv_fused_grad_slabs(B, entry, per * entry + 999)
            assert sl[0][0] == 0 and sl[-1][1] == B and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))  # (the batch once)
            sizes = [b1 - b0 for b0, b1 in sl]
            assert all(1 <= s <= per for s in sizes) and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            assert len(sl) == -(-B // per)  # (the fewest slabs under the limit)
    assert [len(api._fftconv_fused_grad_slabs(5, 100, lim)) for lim in (500, 499, 299, 200, 199, 100)] == [1, 2, 3, 3, 5, 5]
    # the default: half the Infinity Cache, and never a refusal
    m = re.search(r"kInfinityCacheBytes\s*=\s*256\.0 \* 1024\.0 \* 1024\.0", open(os.path.join(
        ROOT, "hackathon_fft_amd", "csrc", "mifft_config.h")).read())
    assert m and api._INFINITY_CACHE_BYTES == 256 << 20 and api._FUSED_GRAD_SCRATCH_DEFAULT == 128 << 20
    assert api._fftconv_fused_grad_slabs(4, 32 << 20, None) == [(0, 4)]
    assert api._fftconv_fused_grad_slabs(4, 48 << 20, None) == [(0, 2), (2, 4)]
    assert api._fftconv_fused_grad_slabs(3, 300 << 20, None) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(mf.MifftError) as e:
        api._fftconv_fused_grad_slabs(3, 1001, 1000)
    assert e.value.status == UNSUPPORTED and "composed" in str(e.value)
    g = api._fftconv_fused_grad_geometry(16384, 65536, 65536, 65536, 0, False)
    assert api._fftconv_fused_grad_entry_bytes(g, 256, torch.float32) == 256 * 16 * 8193 * 8


def test_argument_errors_come_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(api, "DeviceContext", no_device)
    F32 = torch.float32
    # more than 32 lag groups of n // 2 lags
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv_grad(F32, 1, 1, 300, 16, taps=8 * 32 + 1, partition=9, fused=True)
    assert e.value.status == UNSUPPORTED and "33 lag groups" in str(e.value) and "composed" in str(e.value)
    # fused without partition
    for kw in (dict(), dict(taps=5)):
        with pytest.raises(mf.MifftError) as e:
            mf.plan_fftconv_grad(F32, 1, 1, 12, 16, fused=True, **kw)
        assert e.value.status == -2 and "partition" in str(e.value)
    # one batch entry above a given limit; a limit without the fused plan; partials
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv_grad(F32, 5, 2, 100, 16, taps=40, partition=9, fused=True, scratch_bytes=100)
    assert e.value.status == UNSUPPORTED and "composed" in str(e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv_grad(F32, 5, 2, 100, 16, taps=40, partition=9, scratch_bytes=1 << 20)
    assert e.value.status == -2
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv_grad(F32, 5, 2, 100, 16, taps=40, partition=9, fused=True, partials=2)
    assert e.value.status == UNSUPPORTED
    # the shared checks of plan_fftconv_grad still come first
    with pytest.raises(mf.MifftError) as e:
        mf.plan_fftconv_grad(F32, 1, 1, 100, 74, taps=40, partition=9, fused=True)
    assert e.value.status == UNSUPPORTED and "FFT length" in str(e.value)
    x, gy = torch.zeros(1, 1, 100), torch.zeros(1, 1, 100)
    with pytest.raises(mf.MifftError) as e:  # (the single-block path has no partitions to fuse)
        mf.fftconv_filter_grad(x, gy, 5, fused=True)
    assert e.value.status == -2 and "partition" in str(e.value)


def test_the_selector_keeps_the_composed_plan_where_nothing_was_measured():
    sel = api._fftconv_grad_fused
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        for n in (16, 64, 96, 1000, 2048, 4096, 12288):
            if n not in api._FFTCONV_FUSED_GRAD.get(dt, {}):
                assert sel(None, dt, n, 10 * n, n // 2 + 1) is False, (dt, n)
    # the n = 16 / 64 of the existing tests keep their route
    assert sel(None, torch.float32, 16, 150, 9) is False and sel(None, torch.float64, 64, 100, 33) is False
    # the caller's word, and the context manager for the calls that have no keyword (the autograd backward)
    assert sel(True, torch.float32, 16, 150, 9) is True and sel(False, torch.float32, 16384, 1 << 17, 8193) is False
    with mf.fftconv_fused_filter_grad(True):
        assert sel(None, torch.float32, 16, 150, 9) is True and sel(False, torch.float32, 16, 150, 9) is False
        with mf.fftconv_fused_filter_grad(None):
            assert sel(None, torch.float32, 16, 150, 9) is False
        assert sel(None, torch.float32, 16, 150, 9) is True
    assert sel(None, torch.float32, 16, 150, 9) is False
    assert sel(None, torch.float32, 16, 150, None) is False  # (no partitioned path: nothing to fuse)
    # every measured key names a least lag-group count within the kernel's limit
    for dt, table in api._FFTCONV_FUSED_GRAD.items():
        for n, least in table.items():
            assert 1 <= least <= api._FUSED_GRAD_MAX_LAG_GROUPS and api._fftconv_ok(n)
            assert sel(None, dt, n, least * (n // 2), n // 2 + 1) is True
            assert sel(None, dt, n, 33 * (n // 2), n // 2 + 1) is False  # (beyond 32 lag groups: the composed plan)


# ---- the payloads ----------------------------------------------------------------------------------------------------------------
TAG = [0x44524701, 0x7FF84D47]


def test_payload_carries_the_stage_in_word_10():
    # stage 0 is what every payload has been
    assert _conv_payload(ConvRequest(64, 3, 0, 37, grad=True)) == TAG + [3, 0, 37, 0, 1, 0, 37, 0, 0, 0, 0, 0, 0, 0]
    g = api._fftconv_fused_grad_geometry(64, 200, 200, 100, 0, False)  # H = 32, Pg = 4, Fg = 7, live frames 0 .. 6
    assert (g.Pg, g.Fg, g.u_first, g.Fu, g.u_start) == (4, 7, 0, 7, -32)
    u = ConvRequest(64, 3, 0, g.Fu * g.H, S=g.H, F=g.Fu, s0=g.u_start, grad=True, gates=1, stage=1)
    assert _conv_payload(u) == TAG + [3, 0, 32, 0, 7, 0xFFFFFFE0, 224, 0, 1, 1, 0, 0, 0, 0]
    v = ConvRequest(64, 3, g.c, 200, S=g.H, F=g.Fg, s0=0, grad=True, gates=2, stage=2, mode=mf.api._io_mode_bits(torch.bfloat16))
    assert _conv_payload(v) == TAG + [3, 32, 32, 0x800, 7, 0, 200, 0, 2, 2, 0, 0, 0, 0]
    lag = ConvRequest(64, 3, g.Fu, g.Fg, S=g.Pg, F=g.Fg, s0=g.u_first, mode=1, grad=True, stage=3)
    assert _conv_payload(lag) == TAG + [3, 7, 4, 1, 7, 0, 7, 0, 3, 0, 0, 0, 0, 0]
    for bad in (ConvRequest(64, 3, 0, 37, grad=True, stage=4), ConvRequest(64, 3, 0, 37, stage=1)):
        with pytest.raises(mf.MifftError) as e:
            _conv_payload(bad)
        assert e.value.status == -5
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    for name, value in (("U", 1), ("G", 2), ("LAGS", 3)):
        assert re.search(rf"#define\s+MIFFT_CONV_GRAD_STAGE_{name}\s+{value}u\b", h), name


def _stage(stage, gates=0):
    return (stage, gates, 0, 0, 0, 0)


U_PLAN = dict(L=200, n=64, c=0, S=32, F=7, s0=-32, Lo=224)
G_PLAN = dict(L=200, n=64, c=32, S=32, F=7, s0=0, Lo=200)
LAG_PLAN = dict(L=7, n=64, c=7, S=4, F=7, s0=0, Lo=7)  # (words 3 .. 8: Fu | Pg | mode | Fg | m0 | Fg)


def test_the_library_accepts_the_staged_payloads_as_far_as_the_device():
    for kw in (dict(U_PLAN, rsv=_stage(1)), dict(U_PLAN, rsv=_stage(1, 1)), dict(U_PLAN, rsv=_stage(1), mode=0x800),
               dict(G_PLAN, rsv=_stage(2)), dict(G_PLAN, rsv=_stage(2, 2)), dict(G_PLAN, rsv=_stage(2, 2), mode=0x800 | 1, c=0),
               dict(LAG_PLAN, rsv=_stage(3)), dict(LAG_PLAN, rsv=_stage(3), mode=1), dict(LAG_PLAN, rsv=_stage(3), P=2),
               dict(LAG_PLAN, rsv=_stage(3), s0=-3), dict(LAG_PLAN, rsv=_stage(3), S=32), dict(LAG_PLAN, rsv=_stage(3), D=1),
               dict(LAG_PLAN, rsv=_stage(3), n=12288, in_dtype=1, out_dtype=1),
               dict(LAG_PLAN, rsv=_stage(3), L=2, c=1), dict(LAG_PLAN, rsv=_stage(3), L=2, c=2)):  # (dims[0] = max(Fu, 2))
        rc, why = _create(device=-1, **kw)
        assert rc == -10 and "device" in why, (kw, rc, why)


def test_the_library_refuses_what_the_stages_do_not_define():
    for kw, status, word in (
            (dict(U_PLAN, rsv=_stage(4)), -5, "reserved word 10"),
            (dict(U_PLAN, rsv=_stage(0x80000000)), -5, "reserved word 10"),
            (dict(U_PLAN, rsv=_stage(1, 2)), -5, "word 11"),       # stage 1 loads x alone: no postgate
            (dict(U_PLAN, rsv=_stage(1, 3)), -5, "word 11"),
            (dict(G_PLAN, rsv=_stage(2, 1)), -5, "word 11"),       # stage 2 loads gy alone: no pregate
            (dict(U_PLAN, rsv=(1, 0, 1, 0, 0, 0)), -5, "reserved word 12"),
            (dict(U_PLAN, rsv=_stage(1), s0=-64), -5, "reads no sample"),  # a dead first frame
            (dict(U_PLAN, rsv=_stage(1), F=9, Lo=288), -5, "reads no sample"),  # a dead last frame
            (dict(LAG_PLAN, rsv=_stage(3, 1)), -5, "reserved word 11"),  # the gates went into stage 1
            (dict(LAG_PLAN, rsv=(3, 0, 0, 0, 0, 1)), -5, "reserved word 15"),
            (dict(LAG_PLAN, rsv=_stage(3), S=0), -5, "Pg"),
            (dict(LAG_PLAN, rsv=_stage(3), S=33), UNSUPPORTED, "32"),
            (dict(LAG_PLAN, rsv=_stage(3), mode=0x800), -5, "mode word"),
            (dict(LAG_PLAN, rsv=_stage(3), mode=2), -5, "mode word"),
            (dict(LAG_PLAN, rsv=_stage(3), c=6), -5, "Fu"),           # word 3 against dims[0]
            (dict(LAG_PLAN, rsv=_stage(3), Lo=8), -5, "word 8"),      # Fg twice
            (dict(LAG_PLAN, rsv=_stage(3), F=0, Lo=0), -5, "F ="),
            (dict(LAG_PLAN, rsv=_stage(3), D=0), -5, "D ="),
            (dict(LAG_PLAN, rsv=_stage(3), D=4), -8, "multiple"),
            (dict(LAG_PLAN, rsv=_stage(3), P=3), -5, "partial sums"),   # 2 batch entries per channel
            (dict(LAG_PLAN, rsv=_stage(3), n=74), UNSUPPORTED, "FFT length"),
            (dict(LAG_PLAN, rsv=_stage(3), in_dtype=0, out_dtype=1), -4, "float type"),
    ):
        rc, why = _create(**kw)
        assert rc == status and word in why, (kw, rc, why)
