"""Partitioned fftconv on the host (plan_fftconv(taps=, partition=), fftconv(partition=), fftconv_partition; the 20-word
MIFFT_CONV_TAG payload): an fp64 model of uniformly partitioned overlap-save, written out on its own, against numpy / scipy in
every mode and for correlation; the plan's geometry against the model's arithmetic; the partition rule; every refusal of the
payload and of the Python arguments before a device is looked for.  The GPU tests import the model."""
import ctypes

import numpy as np
import pytest
import scipy.signal
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib

STFT = 1 << 5
UNSUPPORTED = -15
TAG_LO, TAG_HI = 0x4F4E5601, 0x7FF84D43
MODES = ("causal", "full", "same", "valid")
SHAPES = [(100, 40, 16, 5), (101, 101, 16, 9), (1000, 1000, 64, 33), (777, 300, 96, 40), (37, 90, 64, 28),
          (333, 200, 16, 15), (50, 7, 16, 9)]  # (T, K, n, Q); the last one has a single partition


# ---- the model (fp64): the loops of the payload ----------------------------------------------------------------------------------
def part_model(x, k, n, Q, c, S, s0, F, Lo, correlate=False, counts=None):
    """rows x (R, T) against filters k (D, K) or (K,), row r with filter r % D, cut into P = ceil(K / Q) partitions of Q taps
    with H_p = rfft(k[p Q : (p + 1) Q], n).  Output block f: Y = sum over p of rfft(blk_p) H_p, blk_p[i] = x[r][s0 + f S - p Q
    + i] (correlation: + p Q, and conj(H_p)), zeros outside the row; a pair (f, p) whose block holds no sample of the row is
    skipped; y = irfft(Y, n); out[r][f S + j] = y[c + j] for j < S and f S + j < Lo.  ``counts`` (R, Lo) ints, if given, counts
    the writes of every output sample; the number of (f, p) pairs transformed is returned beside the result."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    k = np.atleast_2d(np.asarray(k, dtype=np.float64))
    R, T = x.shape
    D, K = k.shape
    P = -(-K // Q)
    assert 1 <= Q <= n - 1 and 1 <= S <= n - Q + 1 and c + S <= n and F >= 1 and (F - 1) * S < Lo <= F * S
    kp = np.zeros((D, P * Q))
    kp[:, :K] = k
    H = np.fft.rfft(kp.reshape(D, P, Q), n, axis=-1)
    if correlate:
        H = np.conj(H)
    out = np.full((R, Lo), np.nan)
    pairs = 0
    for f in range(F):
        Y = np.zeros((R, n // 2 + 1), dtype=np.complex128)
        for p in range(P):
            st = s0 + f * S + (p * Q if correlate else -p * Q)
            if st <= -n or st >= T:
                continue  # (no sample of [0, T): neither loaded nor transformed)
            pairs += 1
            blk = np.zeros((R, n))
            lo, hi = max(st, 0), min(st + n, T)
            blk[:, lo - st:hi - st] = x[:, lo:hi]
            Y += np.fft.rfft(blk, axis=-1) * H[np.arange(R) % D, p]
        y = np.fft.irfft(Y, n, axis=-1)
        w = min(S, Lo - f * S)
        out[:, f * S:f * S + w] = y[:, c:c + w]
        if counts is not None:
            counts[:, f * S:f * S + w] += 1
    assert not np.isnan(out).any()  # (every sample written)
    return out, pairs


def part_geometry(n, Q, K, offset, out_length, correlate=False):
    """(c, S, s0, F, P) of a partitioned plan, written out on its own: the overlap-save geometry of a filter of Q taps"""
    S = n - (Q - 1)
    c = 0 if correlate else Q - 1
    return c, S, offset - c, (out_length + S - 1) // S, (K + Q - 1) // Q


def model(x2d, k, n, Q, offset, out_length, correlate=False):
    K = np.atleast_2d(k).shape[-1]
    c, S, s0, F, _ = part_geometry(n, Q, K, offset, out_length, correlate)
    return part_model(x2d, k, n, Q, c, S, s0, F, out_length, correlate)[0]


@pytest.mark.parametrize("T,K,n,Q", SHAPES)
def test_the_model_against_numpy_and_scipy(T, K, n, Q):
    rng = np.random.default_rng(T * 100 + K)
    D, B = 3, 2
    x, k = rng.standard_normal((B * D, T)), rng.standard_normal((D, K))
    full = np.stack([np.convolve(x[r], k[r % D]) for r in range(B * D)])
    for mode in MODES:
        o, Lo = mf.api._fftconv_window(mode, T, K)
        c, S, s0, F, P = part_geometry(n, Q, K, o, Lo)
        assert (c, S, s0, F, P) == mf.api._fftconv_part_geometry(n, Q, K, o, Lo, False), mode
        counts = np.zeros((B * D, Lo), dtype=np.int64)
        got, pairs = part_model(x, k, n, Q, c, S, s0, F, Lo, counts=counts)
        assert (counts == 1).all(), mode  # (every output sample is written exactly once)
        assert pairs <= F * P
        for r in range(B * D):
            want = full[r][:T] if mode == "causal" else scipy.signal.fftconvolve(x[r], k[r % D], mode=mode)
            assert got[r].shape == want.shape, (mode, got[r].shape, want.shape)
            assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max(), (mode, r)
    # correlation: y[t] = sum_j k[j] x[t + j], zeros beyond the row
    c, S, s0, F, P = part_geometry(n, Q, K, 0, T, True)
    assert (c, S, s0, F, P) == mf.api._fftconv_part_geometry(n, Q, K, 0, T, True)
    counts = np.zeros((B * D, T), dtype=np.int64)
    got, _ = part_model(x, k, n, Q, c, S, s0, F, T, correlate=True, counts=counts)
    assert (counts == 1).all()
    xp = np.concatenate([x, np.zeros((B * D, K))], axis=1)
    for r in range(B * D):
        want = np.array([np.dot(k[r % D], xp[r, t:t + K]) for t in range(T)])
        assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(full[r]).max()


def test_a_single_partition_is_the_overlap_save_block():
    from test_fftconv_long_host import geometry, ols_model
    rng = np.random.default_rng(5)
    T, K, n = 50, 7, 16
    x, k = rng.standard_normal((2, T)), rng.standard_normal((2, K))
    c, S, s0, F = geometry(n, K, 0, T)
    one, pairs = part_model(x, k, n, K, c, S, s0, F, T)
    assert pairs == F and np.array_equal(one, ols_model(x, k, n, c, S, s0, F, T))


def test_the_model_skips_about_half_the_pairs_of_a_causal_filter_as_long_as_the_row():
    # the transform counts of DESIGN.md 3.4q: L = K, n = 16384, Q = 8193, counted with the model's own skip rule
    n, Q = 16384, 8193
    for L, forward, inverse in ((32768, 10, 4), (65536, 36, 8), (131072, 136, 16)):
        c, S, s0, F, P = part_geometry(n, Q, L, 0, L)
        live = sum(1 for f in range(F) for p in range(P) if -n < s0 + f * S - p * Q < L)
        assert (live, F) == (forward, inverse), (L, live, F)


# ---- fftconv_partition -----------------------------------------------------------------------------------------------------------
def test_fftconv_partition_against_its_rule():
    for dtype, top in ((torch.float32, 16384), (torch.float64, 8192)):
        for K in (1, 2, 4097, 8193, 8194, 20000, 65536, 131072, 1 << 20):
            assert mf.fftconv_partition(K, dtype) == (top, top // 2 + 1), (K, dtype)
    assert mf.fftconv_partition(40000) == (16384, 8193)
    for K, dtype, status in ((0, torch.float32, -2), (-3, torch.float32, -2), (5, torch.float16, -4), (5, torch.complex64, -4),
                             ((1 << 30) + 1, torch.float32, UNSUPPORTED)):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv_partition(K, dtype)
        assert e.value.status == status, (K, dtype, e.value)
    assert "fftconv_partition" in mf.__all__


# ---- the C ABI: what is refused before a device is looked for --------------------------------------------------------------------
def _create20(T=1000, n=64, *, batch=6, D=3, c=32, S=32, mode=0, addr=0x10000, F=32, s0=-32, Lo=1000, gates=0, rsv=(0, 0, 0, 0),
              Q=33, P=31, w18=0, w19=0, flags=STFT, in_dtype=0, out_dtype=0, inverse=0, comps=1, device=-1):
    """the default: T = K = 1000 at n = 64 in partitions of Q = 33 taps, causal: c = 32, S = 32, s0 = -32, F = ceil(1000 / 32),
    P = ceil(1000 / 33)"""
    lib = _lib.lib()
    h = ctypes.c_void_p()
    flat = [TAG_LO, TAG_HI, D, c, S, mode, addr & 0xFFFFFFFF, addr >> 32, F, s0 & 0xFFFFFFFF, Lo, gates] + list(rsv) + [Q, P, w18, w19]
    assert len(flat) == 20
    rc = lib.mifft_plan_create(ctypes.byref(h), device, in_dtype, out_dtype, 2, (ctypes.c_int64 * 2)(T, n), batch, comps, inverse,
                               (ctypes.c_uint32 * 20)(*flat), (ctypes.c_int32 * 2)(20, 0), flags)
    why = lib.mifft_last_error().decode()
    if rc == 0:
        lib.mifft_plan_destroy(h)
    return rc, why


def test_a_valid_payload_passes_every_check():
    for kw in (dict(), dict(gates=1), dict(gates=2), dict(gates=3), dict(mode=1, c=0, s0=0), dict(D=1), dict(D=6), dict(batch=0),
               dict(Q=1, P=1000, S=64, c=0, F=16, s0=0), dict(Q=63, P=16, S=2, c=62, F=500, s0=-62),
               dict(S=16, F=63, s0=-32),                     # fewer samples stored than n - Q + 1 allows
               dict(P=1), dict(P=40),                        # P is the caller's: fewer or more partitions than the row needs
               dict(s0=-1000), dict(s0=5000, mode=1, c=0),  # a block without a live partition stores zeros: no refusal
               dict(Lo=993), dict(Lo=1024)):
        rc, why = _create20(**kw)
        assert rc == -10, (kw, rc, why)


def test_every_check_of_the_payload_refuses_with_a_message():
    big = (1 << 30) // 33 + 1
    for kw, status, word in ((dict(Q=0), -5, "Q = 0"), (dict(Q=64), -5, "Q = 64"), (dict(Q=100), -5, "Q = 100"),
                             (dict(S=0), -5, "S = 0"),
                             (dict(mode=1, c=0, s0=0, S=33, F=31), -5, "n - Q + 1"),  # S beyond what no wrap-around touches
                             (dict(c=33), -5, "c + S"),
                             (dict(P=0), -5, "P = 0"), (dict(P=big), -5, "2^30"),
                             (dict(D=0), -5, "D = 0"), (dict(batch=7), -8, "multiple"), (dict(mode=2), -5, "mode"),
                             (dict(addr=0), -5, "null"), (dict(addr=0x10004), -5, "aligned"),
                             (dict(F=0), -5, "F = 0"), (dict(Lo=0), -5, "Lo = 0"), (dict(Lo=992), -5, "Lo = 992"),
                             (dict(Lo=1025), -5, "Lo = 1025"), (dict(T=1), -2, "size 1"),
                             (dict(gates=4), -5, "gates"),
                             (dict(rsv=(1, 0, 0, 0)), -5, "reserved word 12"), (dict(rsv=(0, 0, 0, 7)), -5, "reserved word 15"),
                             (dict(gates=3, rsv=(0, 1, 0, 0)), -5, "reserved word 13"),
                             (dict(w18=1), -5, "reserved word 18"), (dict(w19=1), -5, "reserved word 19"),
                             (dict(n=63), UNSUPPORTED, "even"), (dict(inverse=1), UNSUPPORTED, "inverse"),
                             (dict(comps=2), -3, "real rows"), (dict(flags=STFT | (16 << 16)), UNSUPPORTED, "hop")):
        rc, why = _create20(**kw)
        assert rc == status and word in why, (kw, rc, why)


def test_the_other_payload_lengths_keep_their_meaning():
    lib = _lib.lib()
    assert len(_lib.EXPORTS) == 21  # (no new entry point)
    for len0 in (18, 19, 21):  # the tag in front of any other number of words is still no convolution
        h = ctypes.c_void_p()
        flat = [TAG_LO, TAG_HI] + [1] * (len0 - 2)
        rc = lib.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(1000, 64), 3, 1, 0,
                                   (ctypes.c_uint32 * len0)(*flat), (ctypes.c_int32 * 2)(len0, 0), STFT | (16 << 16))
        assert rc == -5 and "bases_len[0]" in lib.mifft_last_error().decode(), len0
    # the 16-word form still refuses its reserved words and F >= 1 blocks that read no sample
    for words, word in (([3, 32, 32, 0, 0x10000, 0, 32, -32 & 0xFFFFFFFF, 1000, 3, 0, 0, 1, 0], "reserved word 14"),
                        ([3, 32, 32, 0, 0x10000, 0, 32, 5000, 1000, 3, 0, 0, 0, 0], "reads no sample")):
        h = ctypes.c_void_p()
        flat = [TAG_LO, TAG_HI] + words
        rc = lib.mifft_plan_create(ctypes.byref(h), -1, 0, 0, 2, (ctypes.c_int64 * 2)(1000, 64), 6, 1, 0,
                                   (ctypes.c_uint32 * 16)(*flat), (ctypes.c_int32 * 2)(16, 0), STFT)
        assert rc == -5 and word in lib.mifft_last_error().decode(), (word, rc, lib.mifft_last_error().decode())


# ---- Python: argument errors on host tensors -------------------------------------------------------------------------------------
def test_fftconv_partition_argument_validates_on_the_host():
    x, k = torch.zeros(2, 3, 600), torch.zeros(3, 700)  # (host tensors: nothing reaches the library)
    with pytest.raises(ValueError):
        mf.fftconv(x, k, n=1024, partition=40)
    with pytest.raises(ValueError):
        mf.fftconv(x, k, partition="always")
    with pytest.raises(ValueError):
        mf.fftconv_filter_grad(x, torch.zeros(2, 3, 600), 700, n=1024, partition=40)
    for kw, status in ((dict(partition=64, block=64), -2),     # Q <= block - 1
                       (dict(partition=0, block=64), -2),
                       (dict(partition=16384), -2),            # (the default block is 16384 points)
                       (dict(partition=40, block=74), UNSUPPORTED),
                       (dict(partition=40, block=32768), UNSUPPORTED)):
        with pytest.raises(mf.MifftError) as e:
            mf.fftconv(x, k, **kw)
        assert e.value.status == status, (kw, e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(x.double(), k, partition=40, block=16384)  # float64 blocks end at 12288 points
    assert e.value.status == UNSUPPORTED
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(torch.zeros(2, 3, 600, dtype=torch.complex64), k, partition=40, block=64)
    assert e.value.status == -3
    long_x = torch.zeros(3, 20000)
    for args, kw in (((x, k), dict(partition=40, block=96)), ((x, k), dict(partition=33, block=64, mode="full")),
                     ((x, k), dict(partition=63, block=64, correlate=True)), ((x, k), dict(partition=8193)),
                     ((x, k), dict(partition="auto")), ((long_x, torch.zeros(3, 20000)), dict(partition="auto")),
                     ((long_x, torch.zeros(3, 20000)), dict(partition="auto", mode="valid")),
                     ((long_x.double(), torch.zeros(3, 5000).double()), dict(partition="auto")),
                     ((x, torch.zeros(3, 5)), dict(partition=9, block=16))):
        with pytest.raises(mf.MifftError) as e:  # valid: fails only for want of a device tensor
            mf.fftconv(*args, **kw)
        assert e.value.status == -10, (kw, e.value)
    # partition=None is today's refusal, with a hint that names the keyword
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(long_x, torch.zeros(3, 8194))
    assert e.value.status == UNSUPPORTED and "partitioned" in str(e.value) and "partition=" in str(e.value)
    # "auto" with block= keeps the refusals of the overlap-save path
    with pytest.raises(mf.MifftError) as e:
        mf.fftconv(x, k, partition="auto", block=64)
    assert e.value.status == -2


def test_plan_fftconv_partition_validates_before_any_device_work():
    f32 = torch.float32
    for args, kw, status in (((f32, 2, 3, 1000, 64), dict(partition=33), -2),                  # partition goes with taps
                             ((f32, 2, 3, 1000, 64), dict(taps=1000, partition=0), -2),
                             ((f32, 2, 3, 1000, 64), dict(taps=1000, partition=64), -2),
                             ((f32, 2, 3, 1000, 64), dict(taps=0, partition=33), -2),
                             ((f32, 2, 3, 1, 64), dict(taps=1000, partition=33), UNSUPPORTED),
                             ((f32, 2, 3, 1000, 74), dict(taps=1000, partition=33), UNSUPPORTED),
                             ((f32, 2, 3, 1000, 64), dict(taps=1000, partition=33, offset=-1), -5),
                             ((f32, 2, 3, 1000, 64), dict(taps=1000, partition=33, out_length=2000), -5),
                             ((f32, 2, 3, 1000, 64), dict(taps=1000, partition=33, out_length=1001, correlate=True), -5),
                             ((torch.float16, 2, 3, 1000, 64), dict(taps=1000, partition=33), -4),
                             ((f32, 0, 3, 1000, 64), dict(taps=1000, partition=33), -8)):
        for make in (mf.plan_fftconv, mf.plan_fftconv_grad):
            with pytest.raises(mf.MifftError) as e:
                make(*args, **kw)
            assert e.value.status == status, (make.__name__, args, kw, e.value)
    if not torch.cuda.is_available():
        for kw in (dict(taps=1000, partition=33), dict(taps=1000, partition=33, out_length=1999), dict(taps=5, partition=63),
                   dict(taps=100000, partition=1, correlate=True), dict(taps=1000, partition=33, pregate=True)):
            with pytest.raises(mf.MifftError) as e:
                mf.plan_fftconv(f32, 2, 3, 1000, 64, **kw)
            assert e.value.status == -10, kw


def test_the_slices_of_the_composed_filter_gradient():
    """taps p Q .. of the filter gradient from the overlap-save gradient of Q taps on slices of u and gy: the slices' own
    arithmetic against a direct sum, in fp64 on the host"""
    rng = np.random.default_rng(9)
    for T, K, Q, mode, correlate in ((100, 150, 9, "causal", False), (100, 150, 9, "full", False), (100, 150, 9, "same", False),
                                     (100, 150, 9, "valid", False), (333, 200, 33, "valid", False), (20, 30, 5, "causal", True),
                                     (100, 150, 9, "causal", True), (37, 90, 28, "same", False)):
        o, Lo = mf.api._fftconv_window(mode, T, K)
        u, gy = rng.standard_normal(T), rng.standard_normal(Lo)
        up = np.concatenate([np.zeros(K + Lo), u, np.zeros(K + Lo + o)])  # u[i] = up[i + K + Lo], zeros outside [0, T)
        z = K + Lo
        want = np.array([sum(gy[t] * up[z + (o + t + j if correlate else o + t - j)] for t in range(Lo)) for j in range(K)])
        got = np.zeros(K)
        for p in range(-(-K // Q)):
            sl = mf.api._fftconv_part_grad_slice(T, Q, o, Lo, correlate, p)
            if sl is None:
                continue
            u0, u1, g0, g1, off = sl
            assert 0 <= u0 < u1 <= T and 0 <= g0 < g1 <= Lo and off >= 0
            us, gs = u[u0:u1], gy[g0:g1]
            full = len(us) if correlate else len(us) + Q - 1
            assert off + len(gs) <= full  # (what plan_fftconv_grad(taps=Q) asks of its window)
            usp = np.concatenate([np.zeros(Q + len(gs)), us, np.zeros(Q + len(gs) + off)])
            zz = Q + len(gs)
            for j in range(min(Q, K - p * Q)):
                got[p * Q + j] = sum(gs[t] * usp[zz + (off + t + j if correlate else off + t - j)] for t in range(len(gs)))
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), (T, K, Q, mode, correlate)
