"""Inverse STFT plans (MIFFT_FLAG_ISTFT, TileCfg::ISTFT) on the GPU: plan_istft through fft(), the istft wrapper against
torch.istft.

Reference: fp64 numpy (tests/istft_reference.py: irfft, window, ascending overlap-add, division by the overlap-added squared
window; equal to torch.istft on the CPU to 2e-15, tests/test_istft_host.py).  Inputs are random complex spectrograms -- not
outputs of stft -- whose DC and Nyquist bins have imaginary parts.  The error is the relative L2 over blocks of max(hop, 16)
consecutive samples, its maximum over blocks and batch, held to conftest's REL_L2_TOL_F32 / REL_L2_TOL_F64: a block of one sample
(hop = 1) would measure the cancellation among up to 128 terms (4e-4 in an fp32 proxy on the CPU; 4e-7 at most with 16), and one
misplaced frame among 128 still shows as 1e-1.  Every exec writes into a NaN-prefilled output with a NaN guard region behind it,
and X must come back unchanged."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from istft_reference import FP32_ONLY, SHAPES, istft_length, istft_reference, rel_l2_blocks, spectrogram, window_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
CNP = {torch.float32: np.complex64, torch.float64: np.complex128}
CT = {torch.float32: torch.complex64, torch.float64: torch.complex128}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 4096           # NaN elements behind every output
MAX_BYTES = 512 << 20  # per tensor
FAR = 1 << 40          # a count at which no grid is clamped by the tile count


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _device_spectrogram(B, F, n, dtype, seed):
    """random spectrogram rounded to the plan's type: (host complex128 of the rounded values, device (B, F, n/2+1, 2))"""
    Xh = spectrogram(B, F, n, seed).astype(CNP[dtype])
    X = torch.view_as_real(torch.from_numpy(Xh)).to(DEV).contiguous()
    assert X.numel() * X.element_size() <= MAX_BYTES
    return Xh.astype(np.complex128), X


def _exec_guarded(plan, X, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN; X must not change.
    Returns the output tensor (batch, T, 1), still on the device."""
    numel = int(np.prod(plan.out_shape))
    assert numel * X.element_size() <= MAX_BYTES
    flat = torch.full((numel + GUARD,), float("nan"), dtype=plan.out_dtype, device=DEV)
    out = flat[:numel].view(plan.out_shape)
    before = X.clone()
    if first is None:
        mf.fft(out, X, plan=plan)
    else:
        mf.fft(out, X, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.isnan(flat[numel:]).all(), "the guard region behind the output was written"
    assert torch.equal(_bits(X), _bits(before)), "X was written"
    return out


def _assert_plan(plan, B, F, n, T):
    assert plan.in_shape == (B, F, n // 2 + 1, 2) and plan.out_shape == (B, T, 1) and plan.ndim == 3
    name = plan.kernel_name(2)
    assert name.startswith(f"rows{n}_") and "_c2r_" in name and name.endswith("_istft_jit"), name
    assert ("_f64_" in name) == (plan.out_dtype == torch.float64)
    assert plan.kernel_name(0) == "none" and plan.kernel_name(1) == "none"
    assert plan.stages(0) == [] and plan.stages(1) == [] and int(np.prod(plan.stages(2))) == n
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    es = 4 if plan.out_dtype == torch.float32 else 8
    assert plan.in_bytes == B * F * (n // 2 + 1) * 2 * es and plan.out_bytes == B * T * es
    for dim in (0, 1):
        with pytest.raises(mf.MifftError):
            plan.pass_geometry(dim)
    tile, threads, n_tiles, grid = plan.pass_geometry(2)
    assert n_tiles == B * -(-F // tile) and 1 <= grid <= n_tiles


def _summary(runs):
    lens = [r[1] for r in runs]
    return f"{len(runs)} runs of {min(lens)}..{max(lens)} tiles, warm-up up to {max(r[2] for r in runs)}"


def _run_case(B, F, n, hop, win, centred, length, dtype):
    T = istft_length(F, n, hop, centred) if length is None else length
    w = window_of(win, n)
    Xh, X = _device_spectrogram(B, F, n, dtype, seed=F + n + hop)
    ref = istft_reference(Xh, n, hop, w, centred, length)
    plan = mf.plan_istft(dtype, B, F, n, hop, window=w, center=centred, length=length)
    _assert_plan(plan, B, F, n, T)
    got = _exec_guarded(plan, X).cpu().numpy().reshape(B, T)
    assert not np.isnan(got).any()
    err = rel_l2_blocks(got, ref, hop)
    print(f"istft B={B} F={F} n={n} hop={hop} {win} centred={centred} T={T} {dtype} {plan.kernel_name(2)} "
          f"geometry={plan.pass_geometry(2)} {_summary(mf.istft_schedule(plan))} block_err={err:.3e}")
    assert err < TOL[dtype]
    plan.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES) - FP32_ONLY))
def test_shapes(case, dt):
    _run_case(*SHAPES[case], DT[dt])


@pytest.mark.parametrize("case", range(len(SHAPES) - FP32_ONLY, len(SHAPES)))
def test_one_frame_per_tile_and_the_table_in_global_memory(case):
    """n = 16384 and n = 16000 (radices up to 10 in four passes): one row per tile; tile and carry leave no room for the twiddle
    table in LDS, and such a configuration runs 512 threads, not the plain rows' 1024 (which spill with the table in global
    memory); fp32 only"""
    n = SHAPES[case][2]
    plan = mf.plan_istft(torch.float32, 1, SHAPES[case][1], n, SHAPES[case][3], window=window_of(SHAPES[case][4], n), center=True)
    assert plan.pass_geometry(2)[:2] == (1, 512), plan.pass_geometry(2)
    plan.close()
    _run_case(*SHAPES[case], torch.float32)


def test_gain_stays_out_of_the_envelope():
    B, F, n, hop = 3, 11, 64, 16
    w = window_of("hann", n)
    Xh, X = _device_spectrogram(B, F, n, torch.float64, seed=3)
    plan = mf.plan_istft(torch.float64, B, F, n, hop, window=w, center=True, normalized=True)
    got = _exec_guarded(plan, X).cpu().numpy().reshape(B, -1)
    ref = istft_reference(Xh, n, hop, w, True, gain=float(n) ** 0.5)
    assert rel_l2_blocks(got, ref, hop) < REL_L2_TOL_F64
    plan.close()


def _sized_for_runs(dtype, F, n, hop, win, centred):
    """a batch at which every workgroup of the full grid owns at least three tiles, and whose schedule holds every path"""
    w = window_of(win, n)
    probe = mf.plan_istft(dtype, 1, F, n, hop, window=w, center=centred)
    tile, _, _, cap = probe.pass_geometry(2, FAR)
    probe.close()
    tpe = -(-F // tile)
    assert F % tile != 0, "the last tile of an entry must be ragged"
    want_warm = -(-(-(-n // hop) - 1) // tile)
    assert want_warm < tpe
    B = -(-3 * cap // tpe) + 1
    for _ in range(64):
        plan = mf.plan_istft(dtype, B, F, n, hop, window=w, center=centred)
        runs = mf.istft_schedule(plan)
        mid = any(r[0] % tpe for r in runs)
        cross = any(r[0] // tpe != (r[0] + r[1] - 1) // tpe for r in runs)
        if min(r[1] for r in runs) >= 3 and mid and cross and any(r[2] == want_warm for r in runs):
            return plan, B, runs, tile, tpe
        plan.close()
        B += 1
    raise AssertionError("no batch size reaches every path")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("F,n,hop,win,centred", [(150, 16, 3, "hamming", False), (33, 1024, 256, "hann", True),
                                                 (300, 128, 1, "hamming", False)])
def test_runs_of_tiles_with_a_carry(F, n, hop, win, centred, dt):
    """every workgroup walks three tiles or more: runs that start inside an entry (warm-up tiles), runs that cross into the next
    entry (the carry is reset), ragged last tiles; every output sample is compared"""
    dtype = DT[dt]
    plan, B, runs, tile, tpe = _sized_for_runs(dtype, F, n, hop, win, centred)
    assert len(runs) == plan.pass_geometry(2)[3] and sum(r[1] for r in runs) == B * tpe
    assert min(r[1] for r in runs) >= 3
    assert any(r[0] % tpe for r in runs), "no run starts inside an entry"
    assert any(r[0] // tpe != (r[0] + r[1] - 1) // tpe for r in runs), "no run crosses an entry boundary"
    assert F % tile != 0
    K = -(-n // hop)
    want_warm = -(-(K - 1) // tile)
    assert max(r[2] for r in runs) == want_warm >= 1, "no run needs the full warm-up"
    if n == 128 and dtype == torch.float32:
        assert want_warm == 2 and any(r[2] == 2 for r in runs), "two warm-up tiles (K - 1 = 127 frames, 64 per tile)"
    T = istft_length(F, n, hop, centred)
    Xh, X = _device_spectrogram(B, F, n, dtype, seed=n)
    ref = istft_reference(Xh, n, hop, window_of(win, n), centred)
    got = _exec_guarded(plan, X).cpu().numpy().reshape(B, T)
    assert not np.isnan(got).any()
    err = rel_l2_blocks(got, ref, hop)
    print(f"istft runs B={B} F={F} n={n} hop={hop} {dtype} {plan.kernel_name(2)} geometry={plan.pass_geometry(2)} "
          f"{_summary(runs)} block_err={err:.3e}")
    assert err < TOL[dtype]
    plan.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("F,n,hop,win,centred", [(150, 16, 3, "hamming", False), (33, 1024, 256, "hann", True)])
def test_an_entry_is_bit_identical_whatever_the_partition(F, n, hop, win, centred, dt):
    """every sample is summed in ascending frame order from an exact zero: another batch (the runs fall differently),
    first / count slabs and a whole_batch slab plan give the same bits"""
    dtype = DT[dt]
    w = window_of(win, n)
    probe = mf.plan_istft(dtype, 1, F, n, hop, window=w, center=centred)
    tile, _, _, cap = probe.pass_geometry(2, FAR)
    probe.close()
    # 1.3 tiles per workgroup of the full grid: runs of one and two tiles; a third of it: fewer tiles than workgroups
    B = -(-13 * cap // (10 * -(-F // tile))) + 1
    B2 = B // 3
    _, X = _device_spectrogram(B, F, n, dtype, seed=7)
    plan = mf.plan_istft(dtype, B, F, n, hop, window=w, center=centred)
    plan2 = mf.plan_istft(dtype, B2, F, n, hop, window=w, center=centred)
    r1, r2 = mf.istft_schedule(plan), mf.istft_schedule(plan2)
    tpe = -(-F // plan.pass_geometry(2)[0])
    assert [r[0] % tpe for r in r1[:len(r2)]] != [r[0] % tpe for r in r2], "the two batches are walked alike"
    whole = _exec_guarded(plan, X)
    assert not torch.isnan(whole).any()
    other = _exec_guarded(plan2, X[:B2].contiguous())
    assert torch.equal(_bits(other), _bits(whole[:B2])), "the smaller batch against the first entries of the larger"
    # first / count slabs of the same plan: unequal pieces, so their runs fall differently again
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device=DEV)
    out = flat[:numel].view(plan.out_shape)
    for first, count in ((0, B // 5), (B // 5, 1), (B // 5 + 1, B // 2), (B // 5 + 1 + B // 2, B - B // 5 - 1 - B // 2)):
        mf.fft(out, X, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.isnan(flat[numel:]).all()
    assert torch.equal(_bits(out), _bits(whole)), "first / count slabs"
    # a slab plan of a larger batch
    slab = mf.plan_istft(dtype, B2, F, n, hop, window=w, center=centred, whole_batch=B)
    got = _exec_guarded(slab, X[B - B2:].contiguous())
    assert torch.equal(_bits(got), _bits(whole[B - B2:])), "whole_batch slab plan"
    for p in (plan, plan2, slab):
        p.close()


def _torch_ref(Xc, n, **kw):
    """torch.istft on the CPU in float64; leading dims folded (torch takes 2-D or 3-D input)"""
    X = Xc.detach().cpu().to(torch.complex128)
    lead = X.shape[:-2]
    w = kw.pop("window", None)
    if w is not None:
        w = w.detach().cpu().double()
    y = torch.istft(X.reshape((-1,) + X.shape[-2:]), n, window=w, **kw)
    return y.reshape(lead + y.shape[-1:]).numpy()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_wrapper_against_torch(dt):
    dtype = DT[dt]
    n, F = 64, 23
    rng = np.random.default_rng(11)
    Xh = (rng.standard_normal((2, 3, n // 2 + 1, F)) + 1j * rng.standard_normal((2, 3, n // 2 + 1, F))).astype(CNP[dtype])
    X = torch.from_numpy(Xh).to(DEV)  # bins-major, torch's layout in memory: the copying path
    assert not X.transpose(-1, -2).is_contiguous()
    hann64 = torch.hann_window(64, dtype=torch.float64)
    for kw in (dict(hop_length=16, window=hann64),
               dict(window=hann64),                                                   # hop defaults to n // 4
               dict(hop_length=16, win_length=40, window=torch.hann_window(40, dtype=torch.float64)),
               dict(hop_length=16, window=hann64, normalized=True),
               dict(hop_length=16, window=torch.hamming_window(64, dtype=torch.float64), center=False),
               dict(hop_length=16, window=hann64, length=300),
               dict(hop_length=64, center=False),                                     # rectangular, no overlap
               dict(hop_length=5, window=hann64, onesided=True)):
        got = mf.istft(X, n, **kw)
        ref = _torch_ref(X, n, **dict(kw))
        assert got.dtype == dtype and tuple(got.shape) == ref.shape, (kw, got.shape, ref.shape)
        err = rel_l2_blocks(got.cpu().numpy().reshape(6, -1), ref.reshape(6, -1), kw.get("hop_length", 16))
        print(f"istft wrapper {dt} {sorted(k for k in kw if k != 'window')} block_err={err:.3e}")
        assert err < TOL[dtype], kw
    # a 2-D X, and one that lies frames-major already
    got = mf.istft(X[0, 0], n, hop_length=16, window=hann64)
    assert tuple(got.shape) == (istft_length(F, n, 16, True),)
    Xt = X.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert torch.equal(_bits(mf.istft(Xt, n, hop_length=16, window=hann64)), _bits(mf.istft(X, n, hop_length=16, window=hann64)))
    # torch refuses the same window without overlap-add
    with pytest.raises(mf.MifftError) as e:
        mf.istft(X, n, hop_length=64, window=hann64, center=False)
    assert e.value.status == -15 and "overlap-add" in str(e.value)
    mf.clear_plan_cache()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_round_trip_without_a_copy(dt):
    dtype = DT[dt]
    B, T, n, hop = 6, 4000, 400, 160
    w = torch.hann_window(n, dtype=torch.float64)
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((B, T))).to(dtype).to(DEV)
    S = mf.stft(x, n, hop_length=hop, window=w)
    assert S.transpose(-1, -2).is_contiguous()
    y = mf.istft(S, n, hop_length=hop, window=w, length=T)   # (plan and kernel exist from here on)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = mf.istft(S, n, hop_length=hop, window=w, length=T)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    s_bytes = S.numel() * S.element_size()
    assert grown < s_bytes, f"istft allocated {grown} bytes: a copy of X ({s_bytes}) beside the output ({y.numel() * y.element_size()})"
    err = rel_l2_blocks(y.cpu().numpy(), x.cpu().numpy().astype(np.float64), hop)
    print(f"round trip {dt}: block_err={err:.3e}")
    assert tuple(y.shape) == (B, T) and err < TOL[dtype]
    mf.clear_plan_cache()


def test_a_changed_window_does_not_meet_a_stale_plan():
    n, F, hop = 64, 12, 16
    Xh = spectrogram(2, F, n, seed=5)
    X = torch.from_numpy(Xh).to(DEV).transpose(-1, -2)  # (2, n/2+1, F), frames-major underneath
    w = torch.hann_window(n, dtype=torch.float64)
    a = mf.istft(X, n, hop_length=hop, window=w)
    w[10:50] *= 0.5                                       # in place: same object, same shape
    b = mf.istft(X, n, hop_length=hop, window=w)
    c = mf.istft(X, n, hop_length=hop, window=w, normalized=True)
    for got, gain, win in ((a, 1.0, torch.hann_window(n, dtype=torch.float64)), (b, 1.0, w), (c, 8.0, w)):
        ref = istft_reference(Xh, n, hop, win.numpy(), True, gain=gain)
        assert rel_l2_blocks(got.cpu().numpy(), ref, hop) < REL_L2_TOL_F64
    mf.clear_plan_cache()
