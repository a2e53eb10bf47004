"""The log and post stages of a spectrogram plan (TileCfg::LOG / TileCfg::POST, the tagged payload) on the GPU, and the
wrappers on top of them (spectrogram(log=, post=), mfcc).

Reference: numpy fp64 from the test's own input -- rfft of the framed, windowed signal (test_gpu_spectrogram.ref_stft),
abs(.) ** p, @ fb, the log formula, @ post.

Stage isolation adds no FFT tolerance: a plan WITH a stage is compared against the stage's formula evaluated in fp64 on the
output of the same plan WITHOUT it, which is bit for bit the stage's input.
  log:   y = fma(a, L, c), L = log2(max(v + add, amin)); a, c, add, amin and the sum v + add as rounded to T.  The device's L
         is within E ulp_T(L), the one fma rounds once: |y^ - y| <= |a| E ulp_T(L) + ulp_T(max(|a L|, |c|)).
  post:  z[q] = sum_m post[m, q] y[m], weights rounded to T, M fma from an exact zero: |z^ - z| <= u (M + 2) sum_m |post| |y|.
End to end: the per-frame budget e = REL_L2_TOL_F32 / REL_L2_TOL_F64 of the complex frame gives dv per frame
(test_gpu_spectrogram.ref_and_bound); then, per element, dy <= |a| log2(e) dv / (max(v + add, amin) - dv) (the mean value
theorem on log2; no statement where the denominator is not positive) and dz <= sum_m |post| dy + u (M + 2) sum_m |post| |y|.
No new constant."""
import ctypes
import math
import struct

import numpy as np
import pytest
import scipy.fft
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from test_gpu_spectrogram import (DEV, DT, FAR, NP, TOL, UNIT, _bits, _exec_guarded, _signals, hann, ref_and_bound, ref_stft)

pytestmark = pytest.mark.gpu

# The device logarithm's error in ulps of T: twice the largest error measured over the arguments of
# test_the_log_stage_alone on an MI355X against numpy fp64, rounded up to an integer, at least 1.
# Measured: 0.994 ulp in fp32 (__builtin_log2f), 0.618 ulp in fp64 (__ocml_log2_f64), over 216 .. 1305 arguments per case
# (the fp64 figure against numpy's long double; against numpy fp64 it reads 1.000).
E_ULP = 2
LN2 = math.log(2.0)
DB = (0.0, 1e-10, 10.0 * math.log10(2.0), 0.0)          # add, amin, a, c: 10 log10(max(v, 1e-10))
LOGE = (1e-6, 1e-10, LN2, 0.0)                           # ln(max(v + 1e-6, 1e-10))


def rounded(vals, dtype):
    return tuple(float(NP[dtype](v)) for v in vals)


def ulp(x, dtype):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(NP[dtype])).astype(np.float64)


def make_plan(dtype, B, T, n, hop, center, window, power, fb=None, logv=None, post=None):
    F = mf.stft_frames(T, n, hop, center is not None)
    W = post.shape[1] if post is not None else fb.shape[1] if fb is not None else n // 2 + 1
    plan = mf.Plan(dtype, dtype, (B, T, 1), (B, F, W, 1), stft_hop=hop, stft_center=center, stft_window=window,
                   stft_power=power, stft_fb=fb, stft_log=logv, stft_post=post)
    name = plan.kernel_name(1)
    assert f"_stft_p{power}" in name and ("_fb" in name) == (fb is not None), name
    assert ("_lg" in name) == (logv is not None) and ("_pm" in name) == (post is not None), name
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert plan.out_bytes == B * F * W * (4 if dtype == torch.float32 else 8)
    return plan


def run(xh, dtype, n, hop, center, window, power, fb=None, logv=None, post=None, first=None, count=None):
    """the plan's output (B, F, W) on the host, written into a NaN-prefilled tensor with a NaN guard behind it"""
    B, T = xh.shape
    plan = make_plan(dtype, B, T, n, hop, center, window, power, fb, logv, post)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1), first, count)
    plan.close()
    return got


def log_formula(v, logv, dtype):
    """(y, L) from values v of type T: the constants and the sum v + add as rounded to T.  Evaluated in numpy's long double
    (x87 extended, 64 significant bits) and returned as such, so that the reference's own rounding stays below the bound of
    an fp64 plan as well; everything after the subtraction from the device's value happens in fp64."""
    add, amin, a, c = rounded(logv, dtype)
    s = v.astype(NP[dtype]) + NP[dtype](add)  # (one IEEE addition in T, as on the device)
    L = np.log2(np.maximum(s, NP[dtype](amin)).astype(np.longdouble))
    return np.longdouble(a) * L + np.longdouble(c), L


def log_bound(L, logv, dtype):
    _, _, a, c = rounded(logv, dtype)
    return abs(a) * E_ULP * ulp(L, dtype) + ulp(np.maximum(np.abs(a * L), abs(c)), dtype)


def post_bound(y, post, dtype):
    M = post.shape[0]
    return UNIT[dtype] * (M + 2) * (np.abs(y) @ np.abs(post))


def through_post(dy, post):
    """sum_m |post[m, q]| dy[m]; a frame with a band whose dy is unbounded has no bound at all"""
    open_ = ~np.isfinite(dy).all(axis=-1)
    dz = np.where(np.isfinite(dy), dy, 0.0) @ np.abs(post)
    dz[open_] = np.inf
    return dz


def htk40():
    return mf.melscale_fbanks(201, 0.0, 8000.0, 40, 16000).numpy()


def uniform_fb(K, M, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (K, M))


# (n, dtype, B, T, hop, center, M, Q): white noise keeps every band far above amin
ISOLATION = [(16, "f32", 5, 100, 3, None, 0, 0), (16, "f64", 5, 100, 3, None, 0, 0),
             (16, "f32", 5, 100, 3, "reflect", 5, 3), (16, "f64", 5, 100, 3, "reflect", 5, 3),
             (400, "f32", 4, 1000, 160, "reflect", 40, 13), (10, "f32", 3, 80, 3, None, 3, 2)]


def _isolation_inputs(n, dt, B, T, hop, center, M, Q):
    dtype, K = DT[dt], n // 2 + 1
    xh = _signals(B, T, dtype, 700 + n + M)
    fb = None if M == 0 else htk40() if M == 40 else uniform_fb(K, M, 701)
    post = None if Q == 0 else mf.create_dct(Q, M).numpy() if M == 40 else np.random.default_rng(702).standard_normal((M, Q))
    return dtype, xh, fb, post


@pytest.mark.parametrize("logv", [DB, LOGE, (0.0, 1e-10, -2.5, 7.0)], ids=["db", "log_eps", "negative_a"])
@pytest.mark.parametrize("n,dt,B,T,hop,center,M,Q", ISOLATION)
def test_the_log_stage_alone(n, dt, B, T, hop, center, M, Q, logv):
    dtype, xh, fb, _ = _isolation_inputs(n, dt, B, T, hop, center, M, Q)
    w = hann(n)
    v = run(xh, dtype, n, hop, center, w, 2, fb).numpy()
    assert v.min() > 1e3 * logv[1], "the input never reaches amin here"
    # the logarithm by itself: a = 1, c = 0 makes the fma exact
    Ldev = run(xh, dtype, n, hop, center, w, 2, fb, (logv[0], logv[1], 1.0, 0.0)).numpy().astype(np.float64)
    _, L = log_formula(v, logv, dtype)
    e_meas = float((np.abs(Ldev - L).astype(np.float64) / ulp(L, dtype)).max())
    print(f"log2 n={n} {dt} M={M}: {v.size} arguments in [{v.min():.3e}, {v.max():.3e}], largest error {e_meas:.3f} ulp")
    assert e_meas <= 4.0, "a finding about the builtin, not a tolerance to raise"
    got = run(xh, dtype, n, hop, center, w, 2, fb, logv).numpy().astype(np.float64)
    y, L = log_formula(v, logv, dtype)
    err, bound = np.abs(got - y).astype(np.float64), log_bound(L.astype(np.float64), logv, dtype)
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"log stage n={n} {dt} M={M}: worst {i}: err {err[i]:.3e} bound {bound[i]:.3e}")
    assert (err <= bound).all(), (float(err[i]), float(bound[i]))


@pytest.mark.parametrize("logv", [None, DB], ids=["linear", "db"])
@pytest.mark.parametrize("n,dt,B,T,hop,center,M,Q", [c for c in ISOLATION if c[7]])
def test_the_post_stage_alone(n, dt, B, T, hop, center, M, Q, logv):
    dtype, xh, fb, post = _isolation_inputs(n, dt, B, T, hop, center, M, Q)
    w = hann(n)
    y = run(xh, dtype, n, hop, center, w, 2, fb, logv).numpy().astype(np.float64)
    got = run(xh, dtype, n, hop, center, w, 2, fb, logv, post).numpy().astype(np.float64)
    assert got.shape == y.shape[:2] + (Q,) and not np.isnan(got).any()
    err, bound = np.abs(got - y @ post), post_bound(y, post, dtype)
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"post stage n={n} {dt} M={M} Q={Q}: worst {i}: err {err[i]:.3e} bound {bound[i]:.3e}")
    assert (err <= bound).all(), (float(err[i]), float(bound[i]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("M", [0, 5])
def test_silence_is_exactly_minus_seven(M, dt):
    """v = 0 everywhere: fma(0.5, log2(2^-20), 3) = -7 with no rounding anywhere"""
    n, dtype = 16, DT[dt]
    xh = np.zeros((3, 100), dtype=NP[dtype])
    fb = None if M == 0 else uniform_fb(9, M, 710)
    got = run(xh, dtype, n, 3, "constant", hann(n), 2, fb, (0.0, 2.0 ** -20, 0.5, 3.0))
    assert torch.equal(got, torch.full_like(got, -7.0))
    if M:
        z = run(xh, dtype, n, 3, "constant", hann(n), 2, fb, (0.0, 2.0 ** -20, 0.5, 3.0), np.eye(M)[:, [M - 1, 0]])
        assert torch.equal(z, torch.full_like(z, -7.0))


@pytest.mark.parametrize("logv", [None, DB], ids=["linear", "db"])
@pytest.mark.parametrize("n,dt,M", [(16, "f32", 5), (16, "f64", 7), (400, "f32", 40), (10, "f32", 4)])
def test_identity_and_selection_post_are_exact(n, dt, M, logv):
    dtype, K = DT[dt], n // 2 + 1
    B, T, hop = (4, 1000, 160) if n == 400 else (5, 100, 3)
    xh = _signals(B, T, dtype, 720 + n)
    fb = htk40() if M == 40 else uniform_fb(K, M, 721)
    w = hann(n)
    y = run(xh, dtype, n, hop, "reflect", w, 2, fb, logv)
    assert not torch.isnan(y).any()
    assert torch.equal(run(xh, dtype, n, hop, "reflect", w, 2, fb, logv, np.eye(M)), y)
    cols = [M - 1, 0, 1]
    sel = np.zeros((M, 3))
    sel[cols, range(3)] = 1.0
    assert torch.equal(run(xh, dtype, n, hop, "reflect", w, 2, fb, logv, sel), y[..., cols].contiguous())


def _words(values):
    return list(struct.unpack("<%dI" % (2 * len(values)), struct.pack("<%dd" % len(values), *values)))


@pytest.mark.parametrize("M", [0, 5])
def test_a_tagged_payload_without_stages_is_the_old_plan(M):
    """log = 0 and Q = 0 behind the tag: the untagged plan's kernel, and its bits"""
    B, T, n, hop, K = 3, 100, 16, 3, 9
    F = mf.stft_frames(T, n, hop)
    fb = None if M == 0 else uniform_fb(K, M, 730)
    xh = _signals(B, T, torch.float32, 731)
    old_plan = make_plan(torch.float32, B, T, n, hop, None, hann(n), 2, fb)
    old_name = old_plan.kernel_name(1)
    old_plan.close()
    old = run(xh, torch.float32, n, hop, None, hann(n), 2, fb)
    flat = _words(list(hann(n))) + [mf.STFT_EXT_TAG_LO, mf.STFT_EXT_TAG_HI] + _words([2.0, float(M), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    if M:
        flat += _words(list(fb.reshape(-1)))
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.mifft_plan_create(ctypes.byref(h), 0, 0, 0, 2, (ctypes.c_int64 * 2)(T, n), B, 1, 0,
                             (ctypes.c_uint32 * len(flat))(*flat), (ctypes.c_int32 * 2)(len(flat), 0),
                             mf.FLAG_STFT | mf.FLAG_STFT_POWER | mf.FLAG_STFT_HOP(hop))
    assert rc == 0, L.mifft_last_error().decode()
    try:
        assert L.mifft_plan_kernel_name(h, 1).decode() == old_name
        W = M if M else K
        assert int(L.mifft_plan_out_bytes(h)) == B * F * W * 4
        x = torch.from_numpy(xh).to(DEV)
        out = torch.full((B, F, W), float("nan"), device=DEV)
        assert L.mifft_exec_batch(h, x.data_ptr(), out.data_ptr(), 0, B, torch.cuda.current_stream(0).cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.cpu()), _bits(old))
    finally:
        L.mifft_plan_destroy(h)


def end_to_end(xh, dtype, n, hop, center, power, fb, logv, post):
    """(reference, bound) per element of the whole pipeline"""
    add, amin, a, c = rounded(logv, dtype)
    v, dv = ref_and_bound(ref_stft(xh, n, hop, hann(n), center), power, fb, dtype)
    s = np.maximum(v + add, amin)
    den = s - dv[..., None]
    dy = np.where(den > 0, abs(a) / LN2 * dv[..., None] / np.where(den > 0, den, 1.0), np.inf)
    y = a * np.log2(s) + c
    if post is None:
        return y, dy
    return y @ post, through_post(dy, post) + post_bound(y, post, dtype)


def check_elements(got, ref, bound, what):
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    finite = np.isfinite(bound)
    assert finite.mean() >= 0.9, (what, "the bound says nothing about most elements")
    err = np.abs(got - ref)
    ratio = np.where(finite, err / np.where(finite, bound, 1.0), 0.0)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: worst {i}: err {err[i]:.3e} bound {bound[i]:.3e}; largest error anywhere {err.max():.3e}")
    assert (ratio <= 1.0).all(), (what, float(err[i]), float(bound[i]))


@pytest.mark.parametrize("kind", ["db", "log_eps"])
@pytest.mark.parametrize("n,dt,B,T,hop,M,Q", [(16, "f32", 5, 100, 3, 5, 3), (16, "f64", 5, 100, 3, 5, 3),
                                              (400, "f32", 4, 1000, 160, 40, 13)])
def test_end_to_end_against_fp64(n, dt, B, T, hop, M, Q, kind):
    dtype, K = DT[dt], n // 2 + 1
    logv = DB if kind == "db" else LOGE
    xh = _signals(B, T, dtype, 740 + n)
    fb = htk40() if M == 40 else uniform_fb(K, M, 741)
    post = mf.create_dct(Q, M).numpy()
    for pm in (None, post):
        got = run(xh, dtype, n, hop, "reflect", hann(n), 2, fb, logv, pm).numpy().astype(np.float64)
        ref, bound = end_to_end(xh, dtype, n, hop, "reflect", 2, fb, logv, pm)
        check_elements(got, ref, bound, f"end to end n={n} {dt} {kind} Q={0 if pm is None else Q}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_last_free_slot(dt):
    """n = 8: N = 4, M = 3 = N - 1 bands fill the .y of slots 1 .. 3"""
    dtype = DT[dt]
    xh = _signals(5, 60, dtype, 750)
    fb, post = uniform_fb(5, 3, 751), np.random.default_rng(752).standard_normal((3, 3))
    y = run(xh, dtype, 8, 2, None, hann(8) + 0.25, 2, fb, DB).numpy().astype(np.float64)
    got = run(xh, dtype, 8, 2, None, hann(8) + 0.25, 2, fb, DB, post).numpy().astype(np.float64)
    assert (np.abs(got - y @ post) <= post_bound(y, post, dtype)).all()
    with pytest.raises(mf.MifftError) as e:
        make_plan(dtype, 5, 60, 8, 2, None, None, 2, uniform_fb(5, 4, 753), DB, np.ones((4, 2)))
    assert e.value.status == -15 and "n / 2 - 1" in str(e.value)


@pytest.mark.parametrize("B,T,n,hop,center,dt", [(1, 40000, 16384, 4096, "reflect", "f32"), (1, 20000, 8192, 2048, None, "f64")])
def test_the_rows_that_fill_the_lds(B, T, n, hop, center, dt):
    """3 bands + log + post on the longest rows: the stages add no byte of LDS"""
    dtype, K = DT[dt], n // 2 + 1
    fb = np.zeros((K, 3))
    fb[0:10, 0] = 1.0
    fb[K // 2 - 50:K // 2 + 51, 1] = 1.0 - np.abs(np.arange(-50, 51)) / 51.0
    fb[K - 20:K, 2] = np.linspace(0.05, 1.0, 20)
    post = np.random.default_rng(760).standard_normal((3, 4))
    xh = _signals(B, T, dtype, 761)
    got = run(xh, dtype, n, hop, center, hann(n), 2, fb, DB, post).numpy().astype(np.float64)
    ref, bound = end_to_end(xh, dtype, n, hop, center, 2, fb, DB, post)
    check_elements(got, ref, bound, f"n={n} {dt} fb + log + post")
    y = run(xh, dtype, n, hop, center, hann(n), 2, fb, DB).numpy().astype(np.float64)
    assert (np.abs(got - y @ post) <= post_bound(y, post, dtype)).all()


def test_tiles_that_straddle_entries():
    """B = 3 of F = 29 frames in tiles of 64 rows: every entry equals the same signal run alone, bit for bit"""
    B, T, n, hop = 3, 100, 16, 3
    fb, post = uniform_fb(9, 5, 770), np.random.default_rng(771).standard_normal((5, 3))
    xh = _signals(B, T, torch.float32, 772)
    plan = make_plan(torch.float32, B, T, n, hop, None, hann(n), 2, fb, DB, post)
    tile = plan.pass_geometry(1)[0]
    plan.close()
    F = mf.stft_frames(T, n, hop)
    assert F % tile != 0 and (B * F) % tile != 0 and tile < B * F, (tile, F)
    whole = run(xh, torch.float32, n, hop, None, hann(n), 2, fb, DB, post)
    for b in range(B):
        alone = run(xh[b:b + 1], torch.float32, n, hop, None, hann(n), 2, fb, DB, post)
        assert torch.equal(_bits(whole[b:b + 1]), _bits(alone)), b
    ref, bound = end_to_end(xh, torch.float32, n, hop, None, 2, fb, DB, post)
    check_elements(whole.numpy().astype(np.float64), ref, bound, "tiles that straddle entries")


def test_persistent_rounds_rewrite_the_free_slots():
    """n = 1024, 5 bands + log + post, sized from pass_geometry(1) so that the grid walks two full rounds plus a partial one
    with a ragged last tile: the .y slots are rewritten by every tile; every frame is compared"""
    n, hop, T, K = 1024, 256, 4200, 513
    F = mf.stft_frames(T, n, hop, True)
    w = hann(n)
    fb = np.zeros((K, 5))
    for m, (lo, hi) in enumerate([(0, 4), (3, 40), (30, 200), (150, 513), (500, 513)]):
        fb[lo:hi, m] = np.random.default_rng(780 + m).uniform(0.1, 1.0, hi - lo)
    post = np.random.default_rng(785).standard_normal((5, 3))
    probe = make_plan(torch.float32, 1, T, n, hop, "reflect", w, 2, fb, DB, post)
    tile, threads, _, G = probe.pass_geometry(1, FAR)
    probe.close()

    def ok(B):
        rows = B * F
        n_tiles = -(-rows // tile)
        return n_tiles >= 2 * G + 1 and n_tiles % G != 0 and n_tiles % 8 != 0 and (tile == 1 or rows % tile != 0)

    B = -(-((2 * G + G // 2 + 3) * tile) // F)
    while not ok(B):
        B += 1
    plan = make_plan(torch.float32, B, T, n, hop, "reflect", w, 2, fb, DB, post)
    geo = plan.pass_geometry(1)
    text = f"{plan.kernel_name(1)}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {B * F}"
    print(text)
    assert (geo[0], geo[1]) == (tile, threads) and geo[2] == -(-B * F // tile) and geo[3] == G, text
    xh = _signals(B, T, torch.float32, 786)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1)).numpy().astype(np.float64)
    plan.close()
    for b0 in range(0, B, 256):
        ref, bound = end_to_end(xh[b0:b0 + 256], torch.float32, n, hop, "reflect", 2, fb, DB, post)
        check_elements(got[b0:b0 + 256], ref, bound, f"persistent rounds B={B} entries {b0}..")


def test_a_slab_exec_touches_its_own_entries_only():
    B, T, n, hop = 5, 100, 16, 3
    fb, post = uniform_fb(9, 5, 790), np.random.default_rng(791).standard_normal((5, 3))
    xh = _signals(B, T, torch.float32, 792)
    whole = run(xh, torch.float32, n, hop, None, hann(n), 2, fb, DB, post)
    xs = xh.copy()
    xs[[0, 1, 4]] = np.nan
    got = run(xs, torch.float32, n, hop, None, hann(n), 2, fb, DB, post, first=2, count=2)
    assert torch.isnan(got[[0, 1, 4]]).all()
    assert not torch.isnan(got[2:4]).any() and torch.equal(_bits(got[2:4]), _bits(whole[2:4]))


@pytest.mark.parametrize("logv", [None, DB], ids=["linear", "db"])
def test_a_nan_sample_stays_in_the_frames_that_cover_it(logv):
    """all Q outputs of exactly the covering frames are NaN (the max of the log stage keeps a NaN; the .y slots leak nothing
    between rows); every other frame is bit-identical to the run without it"""
    B, T, n, hop, at = 3, 100, 16, 3, 50
    w = hann(n) + 0.25
    fb, post = uniform_fb(9, 5, 800), np.random.default_rng(801).uniform(0.5, 1.5, (5, 3))
    xh = _signals(B, T, torch.float32, 802)
    clean = run(xh, torch.float32, n, hop, None, w, 2, fb, logv, post)
    xn = xh.copy()
    xn[1, at] = np.nan
    got = run(xn, torch.float32, n, hop, None, w, 2, fb, logv, post)
    F = clean.shape[1]
    covers = np.array([f * hop <= at < f * hop + n for f in range(F)])
    assert 0 < covers.sum() < F
    hit = torch.zeros(B, F, dtype=torch.bool)
    hit[1] = torch.from_numpy(covers)
    assert torch.isnan(got[hit]).all() and not torch.isnan(got[~hit]).any()
    assert torch.equal(_bits(got[~hit]), _bits(clean[~hit]))


def test_plan_spectrogram_maps_its_keywords():
    """log=, amin=, eps=, ref= of plan_spectrogram are the (add, amin, a, c) of the plan, bit for bit"""
    B, T, n, hop = 3, 100, 16, 3
    xh = _signals(B, T, torch.float32, 810)
    x = torch.from_numpy(xh).to(DEV).reshape(B, T, 1)
    fb = uniform_fb(9, 5, 811)
    for power in (1, 2):
        mult = 10.0 if power == 2 else 20.0
        for kw, logv in ((dict(log="log", eps=1e-6), (1e-6, 1e-10, LN2, 0.0)),
                         (dict(log="log10"), (0.0, 1e-10, math.log10(2.0), 0.0)),
                         (dict(log="db", amin=1e-5, ref=3.0), (0.0, 1e-5, mult * math.log10(2.0), -mult * math.log10(3.0))),
                         (dict(log="db", amin=2.0, ref=0.5), (0.0, 2.0, mult * math.log10(2.0), -mult * math.log10(2.0)))):
            plan = mf.plan_spectrogram(torch.float32, B, T, n, hop, window=hann(n), power=power, fb=fb, **kw)
            got = _exec_guarded(plan, x)
            plan.close()
            assert torch.equal(_bits(got), _bits(run(xh, torch.float32, n, hop, None, hann(n), power, fb, logv))), (power, kw)


@pytest.mark.parametrize("power", [1, 2])
def test_the_wrapper_in_decibels_against_torch_stft(power):
    n, K = 64, 33
    xc = torch.from_numpy(np.random.default_rng(820).standard_normal((2, 3, 500))).float()
    hw = torch.hann_window(n, dtype=torch.float64)
    fb = uniform_fb(K, 6, 821)
    X = torch.stft(xc.double().reshape(-1, 500), n, window=hw, return_complex=True).reshape(2, 3, K, -1)
    mult, ref, amin = (10.0 if power == 2 else 20.0), 2.5, 1e-10
    for bank in (None, fb):
        v = np.swapaxes(X.abs().pow(power).numpy(), -1, -2)
        if bank is not None:
            v = v @ bank
        want = mult * np.log10(np.maximum(v, amin)) - mult * math.log10(max(amin, ref))
        got = mf.spectrogram(xc.to(DEV), n, window=hw.to(DEV), power=power, fb=None if bank is None else torch.from_numpy(bank),
                             log="db", ref=ref)
        torch.cuda.synchronize()
        W = K if bank is None else 6
        assert tuple(got.shape) == (2, 3, W, X.shape[-1]) and got.dtype == torch.float32 and got.stride(-2) == 1
        _, dv = ref_and_bound(np.swapaxes(X.numpy(), -1, -2), power, bank, torch.float32)
        den = np.maximum(v, amin) - dv[..., None]
        bound = np.where(den > 0, mult / math.log(10.0) * dv[..., None] / np.where(den > 0, den, 1.0), np.inf)
        err = np.abs(np.swapaxes(got.cpu().numpy().astype(np.float64), -1, -2) - want)
        if bank is not None:
            assert np.isfinite(bound).all()
        print(f"db wrapper p={power} M={0 if bank is None else 6}: largest error {err[np.isfinite(bound)].max():.3e} dB")
        assert (err[np.isfinite(bound)] <= bound[np.isfinite(bound)]).all()


@pytest.mark.parametrize("shape", [(500,), (2, 3, 500)])
def test_mfcc_against_the_composition(shape):
    """torch.stft -> abs ** 2 -> @ melscale_fbanks -> 10 log10 -> scipy.fft.dct, in fp64.  8 bands from 1 kHz up: every band
    spans two bins or more, so that the frame budget dv stays below the band's value in (nearly) every frame -- where it
    does not, the propagated bound says nothing about the frame and nothing is asserted of it"""
    rate, n, n_mels, n_mfcc, f_min = 16000, 64, 8, 5, 1000.0
    xc = torch.from_numpy(np.random.default_rng(830).standard_normal(shape)).float()
    hw = torch.hann_window(n, dtype=torch.float64)
    got = mf.mfcc(xc.to(DEV), rate, n_mfcc, n_fft=n, window=hw.to(DEV), n_mels=n_mels, f_min=f_min)
    torch.cuda.synchronize()
    X = torch.stft(xc.double().reshape(-1, 500), n, window=hw, return_complex=True)
    X = np.swapaxes(X.reshape(tuple(shape[:-1]) + tuple(X.shape[-2:])).numpy(), -1, -2)
    fb = mf.melscale_fbanks(n // 2 + 1, f_min, rate / 2, n_mels, rate).numpy()
    assert tuple(got.shape) == tuple(shape[:-1]) + (n_mfcc, X.shape[-2]) and got.stride(-2) == 1 and got.dtype == torch.float32
    v, dv = ref_and_bound(X, 2, fb, torch.float32)
    y = 10.0 * np.log10(np.maximum(v, 1e-10))
    want = scipy.fft.dct(y, type=2, norm="ortho")[..., :n_mfcc]
    D = mf.create_dct(n_mfcc, n_mels).numpy()
    den = np.maximum(v, 1e-10) - dv[..., None]
    dy = np.where(den > 0, 10.0 / math.log(10.0) * dv[..., None] / np.where(den > 0, den, 1.0), np.inf)
    bound = through_post(dy, D) + post_bound(y, D, torch.float32)
    check_elements(np.swapaxes(got.cpu().numpy().astype(np.float64), -1, -2), want, bound + 1e-12 * np.abs(want),
                   f"mfcc {shape}")  # (1e-12: scipy's dct against the matrix, test_logmel_host.py)


def test_a_post_changed_in_place_never_meets_a_stale_plan():
    n, K = 64, 33
    xh = np.random.default_rng(840).standard_normal((2, 400))
    x = torch.from_numpy(xh).to(DEV)
    fb = torch.from_numpy(uniform_fb(K, 6, 841))
    post = torch.from_numpy(np.random.default_rng(842).standard_normal((6, 4))).to(DEV)
    z1 = mf.spectrogram(x, n, fb=fb, log="db", post=post)
    p1 = post.cpu().numpy().copy()
    post.mul_(torch.linspace(0.5, 2.0, 4, dtype=torch.float64, device=DEV))
    z2 = mf.spectrogram(x, n, fb=fb, log="db", post=post)
    y = mf.spectrogram(x, n, fb=fb, log="db")
    torch.cuda.synchronize()
    assert not torch.equal(z1, z2)
    yh = np.swapaxes(y.cpu().numpy(), -1, -2)
    for z, pm in ((z1, p1), (z2, post.cpu().numpy())):
        assert (np.abs(np.swapaxes(z.cpu().numpy(), -1, -2) - yh @ pm) <= post_bound(yh, pm, torch.float64)).all()
    # another log stage is another plan too
    assert not torch.equal(mf.spectrogram(x, n, fb=fb, log="log10"), y)
