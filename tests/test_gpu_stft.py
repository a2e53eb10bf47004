"""STFT plans (MIFFT_FLAG_STFT, TileCfg::STFT) on the GPU: plan_stft through fft(), the stft wrapper against torch.stft.

Reference: fp64 numpy -- np.pad (reflect / zeros / nothing), sliding_window_view(x, n)[:, ::hop] times the window, np.fft.rfft
(equal to torch.stft on the CPU to 2e-14).  The error is the relative L2 PER FRAME, its maximum over frames and batch, held to
conftest's REL_L2_TOL_F32 / REL_L2_TOL_F64: normalised over a whole entry, one misaddressed frame would hide among the others.
Every exec writes into a NaN-prefilled output with a NaN guard region behind it, and x must come back unchanged."""
import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
TWIN_TOL = {torch.float32: 2e-6, torch.float64: 1e-12}  # two kernels with the same arithmetic (test_gpu_persistent_rounds.py)
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


def frame_err(got, ref):
    """max over batch and frames of ||got - ref||_2 / ||ref||_2 of one frame's bins"""
    num = np.linalg.norm(got - ref, axis=-1)
    den = np.linalg.norm(ref, axis=-1)
    assert (den > 0).all()
    return float((num / den).max())


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)  # (torch.hann_window, periodic)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_guarded(plan, x, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN; x must not change.
    Returns the output as complex128 (B, F, n // 2 + 1) on the host."""
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
    o = out.cpu().numpy().astype(np.float64)
    return o[..., 0] + 1j * o[..., 1]


def _assert_plan(plan, B, T, n, hop, center):
    F = mf.stft_frames(T, n, hop, center is not None)
    assert plan.in_shape == (B, T, 1) and plan.out_shape == (B, F, n // 2 + 1, 2)
    assert "_stft" in plan.kernel_name(1), plan.kernel_name(1)
    assert plan.kernel_name(0) == "none"
    assert plan.stages(0) == [] and int(np.prod(plan.stages(1))) == n
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    es = 4 if plan.out_dtype == torch.float32 else 8
    assert plan.in_bytes == B * T * es and plan.out_bytes == B * F * (n // 2 + 1) * 2 * es
    return F


def _run_case(B, T, n, hop, center, window, dtype, seed=0, poison=None):
    """plan_stft + fft on random signals against the reference; poison(x_host): NaN into samples no frame may read"""
    rng = np.random.default_rng(seed + T + n + hop)
    xh = rng.standard_normal((B, T)).astype(NP[dtype])
    ref = ref_stft(xh, n, hop, window, center)
    if poison is not None:
        poison(xh)
    x = torch.from_numpy(xh).to(DEV).reshape(B, T, 1)
    plan = mf.plan_stft(dtype, B, T, n, hop, window=window, center=center)
    F = _assert_plan(plan, B, T, n, hop, center)
    assert ref.shape == (B, F, n // 2 + 1)
    got = _exec_guarded(plan, x)
    assert not np.isnan(got).any()
    err = frame_err(got, ref)
    print(f"stft B={B} T={T} n={n} hop={hop} center={center} {dtype} {plan.kernel_name(1)} "
          f"geometry={plan.pass_geometry(1)} frame_err={err:.3e}")
    assert err < TOL[dtype]
    plan.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_odd_hop_and_tiles_that_straddle_entries(dt):
    """case 1: pair loads aligned to one element; F = 29 is no multiple of any tile"""
    _run_case(5, 100, 16, 3, None, hann(16), DT[dt])


def test_a_hop_above_the_frame_length_leaves_gaps_that_are_never_read():
    """case 2: the samples between the frames and past the last frame are NaN in x"""
    def poison(xh):
        xh[:, 16:24] = np.nan
        xh[:, 40:] = np.nan
    assert mf.stft_frames(50, 16, 24) == 2
    _run_case(2, 50, 16, 24, None, None, torch.float32, poison=poison)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_shortest_frames_hop_one_zeros(dt):
    """case 3: n = 8, hop = 1, F = 65, zeros beyond both ends"""
    _run_case(2, 64, 8, 1, "constant", hann(8), DT[dt])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_every_frame_reflects_at_both_ends(dt):
    """case 4: T at its minimum n / 2 + 1"""
    _run_case(3, 9, 16, 4, "reflect", hann(16), DT[dt])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("center", ["reflect", "constant"])
def test_interior_and_boundary_rows_share_a_tile(center, dt):
    """case 5: N = 200"""
    _run_case(4, 1000, 400, 160, center, hann(400), DT[dt])


def test_an_odd_packed_length():
    """case 6: N = 343"""
    _run_case(3, 4000, 686, 100, None, hann(686), torch.float32)


@pytest.mark.parametrize("B,T,n,hop,center,dt", [(1, 20000, 8192, 2048, None, "f64"), (1, 40000, 16384, 4096, "reflect", "f32")])
def test_the_longest_rows(B, T, n, hop, center, dt):
    """case 7"""
    _run_case(B, T, n, hop, center, hann(n), DT[dt])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_disjoint_rectangular_frames_equal_the_half_spectrum_rows(dt):
    """case 8: n = hop = 16, T = 160, no window, uncentred: the rows of rfftn(onesided=True)"""
    dtype = DT[dt]
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((3, 160)).astype(NP[dtype])).to(DEV)
    plan = mf.plan_stft(dtype, 3, 160, 16, 16)
    _assert_plan(plan, 3, 160, 16, 16, None)
    got = _exec_guarded(plan, x.reshape(3, 160, 1)).reshape(30, 9)
    twin = mf.rfftn(x.reshape(-1, 16), onesided=True)
    torch.cuda.synchronize()
    twin = twin.cpu().numpy().astype(np.complex128)
    err = frame_err(got, twin)
    print(f"stft against rfftn rows {dtype}: {err:.3e}")
    assert err < TWIN_TOL[dtype]
    plan.close()


def test_persistent_rounds():
    """case 9: n = 1024, hop = 256, centre reflect, fp32, sized from pass_geometry(1) so that the grid walks two full rounds
    plus a partial one with a ragged last tile; every frame is compared"""
    n, hop, T = 1024, 256, 4200
    F = mf.stft_frames(T, n, hop, True)
    assert F == 17
    w = hann(n)
    probe = mf.plan_stft(torch.float32, 1, T, n, hop, window=w, center="reflect")
    tile, threads, _, G = probe.pass_geometry(1, FAR)
    probe.close()

    def ok(B):
        rows = B * F
        n_tiles = -(-rows // tile)
        return n_tiles >= 2 * G + 1 and n_tiles % G != 0 and n_tiles % 8 != 0 and (tile == 1 or rows % tile != 0)

    B = -(-((2 * G + G // 2 + 3) * tile) // F)
    while not ok(B):
        B += 1
    plan = mf.plan_stft(torch.float32, B, T, n, hop, window=w, center="reflect")
    geo = plan.pass_geometry(1)
    text = f"{plan.kernel_name(1)}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {B * F}"
    print(text)
    assert (geo[0], geo[1]) == (tile, threads) and geo[2] == -(-B * F // tile) and geo[3] == G, text
    assert geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0 and geo[2] % 8 != 0 and (tile == 1 or (B * F) % tile != 0), text
    xh = np.random.default_rng(9).standard_normal((B, T)).astype(np.float32)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    assert not np.isnan(got).any()
    err = 0.0
    for b0 in range(0, B, 256):  # (the reference in chunks: the frames of 256 entries are 36 MB of fp64)
        err = max(err, frame_err(got[b0:b0 + 256], ref_stft(xh[b0:b0 + 256], n, hop, w, "reflect")))
    print(f"stft persistent rounds B={B}: frame_err={err:.3e}")
    assert err < TOL[torch.float32]
    plan.close()


@pytest.mark.parametrize("center", [None, "reflect"])
def test_a_slab_exec_touches_its_own_entries_only(center):
    """case 10: first = 2, count = 2 of a batch of 5; the other entries are NaN in x and stay NaN in out"""
    B, T, n, hop = 5, 100, 16, 3
    w = hann(n)
    xh = np.random.default_rng(10).standard_normal((B, T)).astype(np.float32)
    ref = ref_stft(xh, n, hop, w, center)
    xh[[0, 1, 4]] = np.nan
    plan = mf.plan_stft(torch.float32, B, T, n, hop, window=w, center=center)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1), first=2, count=2)
    assert np.isnan(got[[0, 1, 4]].real).all() and np.isnan(got[[0, 1, 4]].imag).all()
    assert not np.isnan(got[2:4]).any()
    assert frame_err(got[2:4], ref[2:4]) < TOL[torch.float32]
    plan.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(500,), (2, 3, 500)])
def test_the_wrapper_against_torch_stft(shape, dt):
    """case 11"""
    dtype = DT[dt]
    n = 64
    xc = torch.from_numpy(np.random.default_rng(11).standard_normal(shape)).to(dtype)
    x = xc.to(DEV)
    wc = torch.hann_window(48, dtype=torch.float64)
    for kw in (dict(window=torch.hann_window(n, dtype=torch.float64)),          # the default hop, centred, reflect
               dict(win_length=48, window=wc),                                  # a shorter window, zero-padded centred
               dict(win_length=48),                                             # ... and a rectangular one
               dict(normalized=True, window=torch.hann_window(n, dtype=torch.float64)),
               dict(window=None),
               dict(hop_length=7, center=False, window=torch.hann_window(n, dtype=torch.float64)),
               dict(hop_length=24, pad_mode="constant", window=torch.hann_window(n, dtype=torch.float64))):
        # (torch.stft takes (T,) or (B, T) only: the leading dims folded, as the wrapper folds them, and unfolded again)
        ref = torch.stft(xc.double().reshape(-1, shape[-1]), n, return_complex=True, **kw)
        ref = ref.reshape(tuple(shape[:-1]) + tuple(ref.shape[-2:])).numpy()
        dkw = dict(kw)
        if dkw.get("window") is not None:
            dkw["window"] = dkw["window"].to(DEV)
        got = mf.stft(x, n, **dkw)
        torch.cuda.synchronize()
        assert tuple(got.shape) == ref.shape and got.shape[-2] == n // 2 + 1
        assert got.dtype == (torch.complex64 if dtype == torch.float32 else torch.complex128)
        assert got.stride(-2) == 1 and got.stride(-1) == n // 2 + 1  # a transposed view of the frames-major tensor
        g = got.cpu().numpy().astype(np.complex128)
        err = frame_err(np.swapaxes(g, -1, -2), np.swapaxes(ref, -1, -2))
        assert err < TOL[dtype], (kw, err)


def test_a_window_changed_in_place_never_meets_a_stale_plan():
    """case 12"""
    n = 64
    xh = np.random.default_rng(12).standard_normal((2, 400))
    x = torch.from_numpy(xh).to(DEV)
    w = torch.hann_window(n, dtype=torch.float64, device=DEV)
    y1 = mf.stft(x, n, window=w)
    w.mul_(torch.linspace(0.5, 2.0, n, dtype=torch.float64, device=DEV))
    y2 = mf.stft(x, n, window=w)
    torch.cuda.synchronize()
    wn = w.cpu().numpy()
    ref2 = ref_stft(xh, n, n // 4, wn, "reflect")
    ref1 = ref_stft(xh, n, n // 4, hann(n), "reflect")
    assert frame_err(np.swapaxes(y1.cpu().numpy(), -1, -2), ref1) < TOL[torch.float64]
    assert frame_err(np.swapaxes(y2.cpu().numpy(), -1, -2), ref2) < TOL[torch.float64]
