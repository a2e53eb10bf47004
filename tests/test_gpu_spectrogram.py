"""Spectrogram plans (MIFFT_FLAG_STFT_POWER, TileCfg::SPEC / TileCfg::FB) on the GPU: plan_spectrogram through fft(), the
spectrogram wrapper against torch.stft(...).abs().pow(p) (@ fb).

Reference: fp64 numpy -- the frames of test_gpu_stft.py's reference, abs(np.fft.rfft(frames)) ** p, then @ fb in fp64.

Bounds.  No new numbers: the project's per-frame budget e = REL_L2_TOL_F32 / REL_L2_TOL_F64 on the complex frame,
||X^ - X||_2 <= e ||X||_2, pushed through the new arithmetic.  All norms are per frame and of the fp64 reference.
  magnitude:  ||y^ - |X|||_2 <= e ||X||_2                                   (| |a| - |b| | <= |a - b|)
  power:      ||y^ - |X|^2||_2 <= e ||X||_2 (2 ||X||_inf + e ||X||_2)       (| |a|^2 - |b|^2 | = | |a| - |b| | (|a| + |b|))
  filterbank: the same right-hand side times ||fb||_F (Cauchy-Schwarz per band, valid for signed weights), plus
              u (L + 2) ||fb||_F ||P||_2 for rounding the weights and the L-term sums; L the longest band, u = 2^-24 / 2^-53.
The bounds are loose by design: the exact-equality cases catch indexing mistakes, the bounds arithmetic ones.  Every exec
writes into a NaN-prefilled output with a NaN guard region behind it, and x must come back unchanged."""
import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
NP = {torch.float32: np.float32, torch.float64: np.float64}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 4096           # NaN elements behind every output
MAX_BYTES = 512 << 20  # per tensor
FAR = 1 << 40          # a count at which no grid is clamped by the tile count


def ref_stft(x, n, hop, window=None, center=None):
    """(B, T) -> (B, F, n // 2 + 1) complex128"""
    x = np.asarray(x, dtype=np.float64)
    if center == "reflect":
        x = np.pad(x, ((0, 0), (n // 2, n // 2)), mode="reflect")
    elif center == "constant":
        x = np.pad(x, ((0, 0), (n // 2, n // 2)))
    frames = sliding_window_view(x, n, axis=-1)[:, ::hop]
    if window is not None:
        frames = frames * np.asarray(window, dtype=np.float64)
    return np.fft.rfft(frames, axis=-1)


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)  # (torch.hann_window, periodic)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def longest_band(fb):
    """the longest span first non-zero row .. last non-zero row over the columns of a (K, M) matrix"""
    L = 0
    for m in range(fb.shape[1]):
        nz = np.nonzero(fb[:, m])[0]
        if nz.size:
            L = max(L, int(nz[-1] - nz[0] + 1))
    return L


def ref_and_bound(X, power, fb, dtype):
    """the fp64 reference (.., F, K or M) of the complex frames X (.., F, K), and the bound on ||got - ref||_2 of every frame"""
    e, u = TOL[dtype], UNIT[dtype]
    mag = np.abs(X)
    n2, ninf = np.linalg.norm(X, axis=-1), mag.max(axis=-1)
    P = mag ** power
    bound = e * n2 if power == 1 else e * n2 * (2 * ninf + e * n2)
    if fb is None:
        return P, bound
    fro = np.linalg.norm(fb)
    return P @ fb, bound * fro + u * (longest_band(fb) + 2) * fro * np.linalg.norm(P, axis=-1)


def check(got, ref, bound, what):
    """every frame within its bound; prints the largest error beside its bound"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    err = np.linalg.norm(got - ref, axis=-1)
    assert (bound > 0).all()
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{what}: worst frame {i}: err {err[i]:.3e} bound {bound[i]:.3e} (ratio {err[i] / bound[i]:.3e})")
    assert (err <= bound).all(), (what, float(err[i]), float(bound[i]))


def _exec_guarded(plan, x, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN; x must not change.
    Returns the output (B, F, K or M) on the host, in the plan's dtype."""
    numel = int(np.prod(plan.out_shape))
    assert numel * x.element_size() <= MAX_BYTES and x.numel() * x.element_size() <= MAX_BYTES, (plan.in_shape, plan.out_shape)
    flat = torch.full((numel + GUARD,), float("nan"), dtype=plan.out_dtype, device=DEV)
    out = flat[:numel].view(plan.out_shape)
    before = x.clone()
    if first is None:
        mf.fft(out, x, plan=plan)
    else:
        mf.fft(out, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.isnan(flat[numel:]).all(), "the guard region behind the output was written"
    assert torch.equal(_bits(x), _bits(before)), "x was written"
    return out.cpu()[..., 0]


def _assert_plan(plan, B, T, n, hop, center, power, M):
    F = mf.stft_frames(T, n, hop, center is not None)
    width = M if M else n // 2 + 1
    assert plan.in_shape == (B, T, 1) and plan.out_shape == (B, F, width, 1)
    name = plan.kernel_name(1)
    assert f"_stft_p{power}" in name and ("_fb" in name) == bool(M), name
    assert plan.kernel_name(0) == "none"
    assert plan.stages(0) == [] and int(np.prod(plan.stages(1))) == n
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    es = 4 if plan.out_dtype == torch.float32 else 8
    assert plan.in_bytes == B * T * es and plan.out_bytes == B * F * width * es
    return F


def _signals(B, T, dtype, seed):
    return np.random.default_rng(seed).standard_normal((B, T)).astype(NP[dtype])


def _run(xh, n, hop, center, window, dtype, power, fb=None):
    """plan_spectrogram + fft of the host signals xh (B, T): the output on the host (torch, the plan's dtype)"""
    B, T = xh.shape
    x = torch.from_numpy(xh).to(DEV).reshape(B, T, 1)
    plan = mf.plan_spectrogram(dtype, B, T, n, hop, window=window, center=center, power=power, fb=fb)
    _assert_plan(plan, B, T, n, hop, center, power, 0 if fb is None else fb.shape[1])
    got = _exec_guarded(plan, x)
    name, geo = plan.kernel_name(1), plan.pass_geometry(1)
    plan.close()
    return got, f"{name} geometry={geo}"


def _run_case(B, T, n, hop, center, window, dtype, power, fb=None, seed=0):
    xh = _signals(B, T, dtype, seed + T + n + hop)
    ref, bound = ref_and_bound(ref_stft(xh, n, hop, window, center), power, fb, dtype)
    got, text = _run(xh, n, hop, center, window, dtype, power, fb)
    check(got.numpy().astype(np.float64), ref, bound,
          f"spectrogram B={B} T={T} n={n} hop={hop} center={center} p={power} M={0 if fb is None else fb.shape[1]} {dtype} {text}")
    return got


def mel_fb(n_fft, bands, rate=16000.0):
    """a triangular mel-style filterbank (n_fft // 2 + 1, bands), HTK mel scale, unnormalised: at 80 bands over 201 bins some
    low bands are empty or a single bin"""
    K = n_fft // 2 + 1
    freqs = np.linspace(0.0, rate / 2, K)
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + rate / 2 / 700.0), bands + 2)
    pts = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    up = (freqs[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None, :]
    down = (pts[None, 2:] - freqs[:, None]) / (pts[2:] - pts[1:-1])[None, :]
    return np.maximum(0.0, np.minimum(up, down))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("power", [1, 2])
def test_rows_of_nine_reals_and_tiles_that_straddle_entries(power, dt):
    """case 1: F = 29 divides no tile; rows of 9 reals start at odd offsets; bins 0 and N come from one work item"""
    _run_case(5, 100, 16, 3, None, hann(16), DT[dt], power)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("center", ["reflect", "constant"])
def test_the_middle_bin_is_stored_once(center, dt):
    """case 2: N = 200, so 2 k = N occurs"""
    _run_case(4, 1000, 400, 160, center, hann(400), DT[dt], 2)


def test_an_odd_packed_length_has_no_middle_pair():
    """case 3: N = 343"""
    _run_case(3, 4000, 686, 100, None, hann(686), torch.float32, 1)


@pytest.mark.parametrize("B,T,n,hop,center,dt", [(1, 40000, 16384, 4096, "reflect", "f32"), (1, 20000, 8192, 2048, None, "f64")])
def test_the_longest_rows_with_a_filterbank(B, T, n, hop, center, dt):
    """case 4: the in-place LDS layout fits where the STFT tile fills the LDS; the last band ends at bin N"""
    K = n // 2 + 1
    fb = np.zeros((K, 3))
    fb[0:10, 0] = 1.0
    fb[K // 2 - 50:K // 2 + 51, 1] = 1.0 - np.abs(np.arange(-50, 51)) / 51.0
    fb[K - 20:K, 2] = np.linspace(0.05, 1.0, 20)
    _run_case(B, T, n, hop, center, hann(n), DT[dt], 2, fb)


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n,dt", [(16, "f32"), (16, "f64"), (400, "f32")])
def test_identity_and_selection_filterbanks_are_exact(n, dt, power):
    """case 5: an identity filterbank is the M = 0 plan bit for bit; four selected columns are those columns bit for bit"""
    dtype, K = DT[dt], n // 2 + 1
    B, T, hop = (5, 100, 3) if n == 16 else (4, 1000, 160)
    xh = _signals(B, T, dtype, 50 + n)
    w = hann(n)
    plain, _ = _run(xh, n, hop, "reflect", w, dtype, power)
    ident, _ = _run(xh, n, hop, "reflect", w, dtype, power, np.eye(K))
    assert not torch.isnan(plain).any()
    assert torch.equal(_bits(ident), _bits(plain))
    cols = [K - 1, 0, 1, K - 2]  # bins N, 0, 1, N - 1
    sel = np.zeros((K, 4))
    sel[cols, range(4)] = 1.0
    picked, _ = _run(xh, n, hop, "reflect", w, dtype, power, sel)
    assert torch.equal(_bits(picked), _bits(plain[..., cols].contiguous()))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("power", [1, 2])
def test_dense_signed_and_degenerate_columns(power, dt):
    """case 6: n = 64; a dense signed matrix of 7 bands; columns with interior zeros, no rows, bin 0 only, bin N only"""
    n, K = 64, 33
    rng = np.random.default_rng(6)
    _run_case(3, 500, n, 20, "reflect", hann(n), DT[dt], power, rng.standard_normal((K, 7)))
    fb = np.zeros((K, 5))
    fb[[2, 9], 0] = [0.75, -1.5]   # zero in its interior: the span 2 .. 9 is kept
    fb[0, 2] = 2.0                 # (column 1: no rows at all)
    fb[K - 1, 3] = -0.5
    fb[:, 4] = rng.standard_normal(K)
    got = _run_case(3, 500, n, 20, "reflect", hann(n), DT[dt], power, fb)
    assert (_bits(got[..., 1]) == 0).all(), "a band without rows stores an exact +0.0"


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_mel_filterbank(dt):
    """case 7: 80 triangular bands over 201 bins"""
    fb = mel_fb(400, 80)
    spans = [(np.nonzero(fb[:, m])[0].size) for m in range(80)]
    assert min(spans) <= 1 and max(spans) >= 8, spans  # (narrow at the bottom, wide at the top)
    _run_case(4, 1000, 400, 160, "reflect", hann(400), DT[dt], 2, fb)


def test_persistent_rounds():
    """case 8: n = 1024, hop = 256, centre reflect, fp32, 5 bands; sized from pass_geometry(1) so that the grid walks two
    full rounds plus a partial one with a ragged last tile; every frame is compared"""
    n, hop, T, K = 1024, 256, 4200, 513
    F = mf.stft_frames(T, n, hop, True)
    assert F == 17
    w = hann(n)
    fb = np.zeros((K, 5))
    for m, (lo, hi) in enumerate([(0, 4), (3, 40), (30, 200), (150, 513), (512, 513)]):
        fb[lo:hi, m] = np.random.default_rng(80 + m).uniform(0.1, 1.0, hi - lo)
    probe = mf.plan_spectrogram(torch.float32, 1, T, n, hop, window=w, center="reflect", power=2, fb=fb)
    tile, threads, _, G = probe.pass_geometry(1, FAR)
    probe.close()

    def ok(B):
        rows = B * F
        n_tiles = -(-rows // tile)
        return n_tiles >= 2 * G + 1 and n_tiles % G != 0 and n_tiles % 8 != 0 and (tile == 1 or rows % tile != 0)

    B = -(-((2 * G + G // 2 + 3) * tile) // F)
    while not ok(B):
        B += 1
    plan = mf.plan_spectrogram(torch.float32, B, T, n, hop, window=w, center="reflect", power=2, fb=fb)
    geo = plan.pass_geometry(1)
    text = f"{plan.kernel_name(1)}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {B * F}"
    print(text)
    assert (geo[0], geo[1]) == (tile, threads) and geo[2] == -(-B * F // tile) and geo[3] == G, text
    assert geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0 and geo[2] % 8 != 0 and (tile == 1 or (B * F) % tile != 0), text
    xh = _signals(B, T, torch.float32, 9)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1)).numpy().astype(np.float64)
    plan.close()
    for b0 in range(0, B, 256):  # (the reference in chunks: the frames of 256 entries are 36 MB of fp64)
        ref, bound = ref_and_bound(ref_stft(xh[b0:b0 + 256], n, hop, w, "reflect"), 2, fb, torch.float32)
        check(got[b0:b0 + 256], ref, bound, f"persistent rounds B={B} entries {b0}..")


def test_a_slab_exec_touches_its_own_entries_only():
    """case 9: first = 2, count = 2 of a batch of 5; the other entries are NaN in x and stay NaN in out; the slab equals the
    same entries of the whole-batch run bit for bit"""
    B, T, n, hop = 5, 100, 16, 3
    w = hann(n)
    fb = np.random.default_rng(90).standard_normal((n // 2 + 1, 3))
    xh = _signals(B, T, torch.float32, 10)
    whole, _ = _run(xh, n, hop, None, w, torch.float32, 2, fb)
    ref, bound = ref_and_bound(ref_stft(xh, n, hop, w, None), 2, fb, torch.float32)
    xs = xh.copy()
    xs[[0, 1, 4]] = np.nan
    plan = mf.plan_spectrogram(torch.float32, B, T, n, hop, window=w, power=2, fb=fb)
    got = _exec_guarded(plan, torch.from_numpy(xs).to(DEV).reshape(B, T, 1), first=2, count=2)
    plan.close()
    assert torch.isnan(got[[0, 1, 4]]).all()
    check(got[2:4].numpy().astype(np.float64), ref[2:4], bound[2:4], "slab 2..3 of 5")
    assert torch.equal(_bits(got[2:4]), _bits(whole[2:4]))


@pytest.mark.parametrize("bands", [0, 3])
def test_a_nan_sample_stays_in_the_frames_that_cover_it(bands):
    """case 10: one NaN in the middle of entry 1 of 3: exactly the frames that cover it are NaN, every other frame is finite
    and bit-identical to the run without it (the filterbank reuses the tile's LDS in place: nothing leaks between rows)"""
    B, T, n, hop, at = 3, 100, 16, 3, 50
    w = hann(n) + 0.25  # (no zero weight: every frame that holds the sample sees it)
    fb = None if not bands else np.random.default_rng(100).uniform(0.5, 1.5, (n // 2 + 1, bands))
    xh = _signals(B, T, torch.float32, 11)
    clean, _ = _run(xh, n, hop, None, w, torch.float32, 2, fb)
    xn = xh.copy()
    xn[1, at] = np.nan
    got, _ = _run(xn, n, hop, None, w, torch.float32, 2, fb)
    F = clean.shape[1]
    covers = np.array([f * hop <= at < f * hop + n for f in range(F)])
    assert 0 < covers.sum() < F
    hit = torch.zeros(B, F, dtype=torch.bool)
    hit[1] = torch.from_numpy(covers)
    assert torch.isnan(got[hit]).all(), "a frame that covers the NaN sample is not NaN in every value"
    assert not torch.isnan(got[~hit]).any(), "NaN outside the frames that cover the sample"
    assert torch.equal(_bits(got[~hit]), _bits(clean[~hit]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(500,), (2, 3, 500)])
def test_the_wrapper_against_torch_stft(shape, dt):
    """case 11"""
    dtype = DT[dt]
    n, K = 64, 33
    xc = torch.from_numpy(np.random.default_rng(11).standard_normal(shape)).to(dtype)
    x = xc.to(DEV)
    fb = torch.from_numpy(np.random.default_rng(12).uniform(-1.0, 1.0, (K, 6)))
    fb[:8, 0] = 0.0
    fb[20:, 0] = 0.0
    hw = torch.hann_window(n, dtype=torch.float64)
    for kw in (dict(window=hw),                                                                # the default hop, centred, reflect
               dict(win_length=48, window=torch.hann_window(48, dtype=torch.float64)),         # a shorter window
               dict(normalized=True, window=hw),
               dict(win_length=48, normalized=True, hop_length=7, center=False),
               dict(hop_length=24, pad_mode="constant", window=hw)):
        X = torch.stft(xc.double().reshape(-1, shape[-1]), n, return_complex=True, **kw)
        X = X.reshape(tuple(shape[:-1]) + tuple(X.shape[-2:]))
        for power in (1, 2.0):
            for bank in (None, fb):
                want = X.abs().pow(power)
                if bank is not None:
                    want = bank.T @ want
                ref, bound = ref_and_bound(np.swapaxes(X.numpy(), -1, -2), int(power),
                                           None if bank is None else bank.numpy(), dtype)
                assert np.allclose(ref, np.swapaxes(want.numpy(), -1, -2), rtol=1e-12, atol=1e-12)
                dkw = dict(kw)
                if dkw.get("window") is not None:
                    dkw["window"] = dkw["window"].to(DEV)
                got = mf.spectrogram(x, n, power=power, fb=None if bank is None else bank.to(DEV), **dkw)
                torch.cuda.synchronize()
                width = K if bank is None else bank.shape[1]
                assert tuple(got.shape) == tuple(want.shape) and got.shape[-2] == width
                assert got.dtype == dtype and not got.is_complex()
                assert got.stride(-2) == 1 and got.stride(-1) == width  # a transposed view of the frames-major tensor
                check(np.swapaxes(got.cpu().numpy().astype(np.float64), -1, -2), ref, bound,
                      f"wrapper {shape} {dtype} p={power} M={0 if bank is None else width} {sorted(kw)}")


def test_a_filterbank_changed_in_place_never_meets_a_stale_plan():
    """case 11, the cache key: the digest of the filterbank's values"""
    n, K = 64, 33
    xh = np.random.default_rng(13).standard_normal((2, 400))
    x = torch.from_numpy(xh).to(DEV)
    fb = torch.from_numpy(np.random.default_rng(14).uniform(0.0, 1.0, (K, 4))).to(DEV)
    y1 = mf.spectrogram(x, n, fb=fb)
    fb1 = fb.cpu().numpy().copy()
    fb.mul_(torch.linspace(0.5, 2.0, 4, dtype=torch.float64, device=DEV))
    y2 = mf.spectrogram(x, n, fb=fb)
    torch.cuda.synchronize()
    assert not torch.equal(y1, y2)
    X = ref_stft(xh, n, n // 4, None, "reflect")
    for y, bank, what in ((y1, fb1, "before"), (y2, fb.cpu().numpy(), "after")):
        ref, bound = ref_and_bound(X, 2, bank, torch.float64)
        check(np.swapaxes(y.cpu().numpy(), -1, -2), ref, bound, f"filterbank {what} the change")


def test_plan_facts():
    """case 12"""
    B, T, n, hop, K = 3, 1000, 64, 16, 33
    fb = np.ones((K, 5))
    for dtype in (torch.float32, torch.float64):
        for power in (1, 2):
            for bank in (None, fb):
                plan = mf.plan_spectrogram(dtype, B, T, n, hop, power=power, fb=bank)
                F = _assert_plan(plan, B, T, n, hop, None, power, 0 if bank is None else 5)
                assert plan.pass_geometry(1)[2] == -(-B * F // plan.pass_geometry(1)[0])
                plan.close()
        plain = mf.plan_stft(dtype, B, T, n, hop)
        name = plain.kernel_name(1)
        assert "_stft" in name and "_stft_p" not in name and "_fb" not in name, name
        assert plain.out_bytes == B * mf.stft_frames(T, n, hop) * K * 2 * (4 if dtype == torch.float32 else 8)
        plain.close()
    by_flag = mf.Plan(torch.float32, torch.float32, (B, T, 1), (B, mf.stft_frames(T, n, hop), 5, 1), stft_hop=hop,
                      stft_power=2, stft_fb=fb)
    assert by_flag.flags & mf.FLAG_STFT_POWER and "_stft_p2_fb" in by_flag.kernel_name(1)
    by_flag.close()
