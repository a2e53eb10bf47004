"""The fused inverse MDCT on the MI355X (MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan, TileCfg::IMDCT): the one-launch kernel against
the definition in fp64 (test_imdct_host.ref_imdct), its runs, carries and warm-up frames as mf.istft_schedule restates them,
bit identity over batches and slabs, containment, the round trip through mf.mdct, and mf.imdct against the plan and against the
composition it replaced.  Everything is sized from plan.pass_geometry(2) and the schedule, never from a hard-coded tile.

Error measure: the max over the blocks of n output samples of ||got - ref|| / ||ref||, held to conftest's REL_L2_TOL_F32 /
REL_L2_TOL_F64.  A last block that the plan stores only in part (T no multiple of n) is measured against the reference's norm over
the WHOLE block, scaled by sqrt(stored / n): the rounding error of a sample is relative to the size of the two frames it is summed
from, not to the sample itself, so one or two stored samples that happen to be small say nothing about the kernel.  For whole
blocks this is the plain ratio."""
import functools

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_imdct_host import imdct_gain, ref_imdct, unfold_imdct

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]
GUARD = 4096  # NaN elements behind every output
FAR = 1 << 20


def _ref(X, n, w, norm):
    """all (F - 1) n samples: the definition (the cosine matrix) up to 1080 coefficients; beyond, ref_dct4 and the numpy unfold,
    which test_imdct_host.py checks against the definition"""
    return ref_imdct(X, n, w, norm) if n <= 1080 else unfold_imdct(X, n, w, norm)


def _block_err(got, ref_full, n):
    """got (B, T) against the first T samples of ref_full (B, (F - 1) n): see the module docstring"""
    got = np.asarray(got, dtype=np.float64)
    B, T = got.shape
    nb = -(-T // n)
    den = np.linalg.norm(ref_full[:, :nb * n].reshape(B, nb, n), axis=2)
    d = np.zeros((B, nb * n))
    d[:, :T] = got - ref_full[:, :T]
    num = np.linalg.norm(d.reshape(B, nb, n), axis=2)
    stored = np.minimum(n, T - n * np.arange(nb))
    assert den.min() > 0
    return float((num / (den * np.sqrt(stored / n))).max())


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_guarded(plan, X, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN; X must not change.
    Returns the output (B, T) on the device."""
    numel = int(np.prod(plan.out_shape))
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
    return out[..., 0]


def _window(kind, n, seed=0):
    """"sine": the default; else uniform in [0.25, 1] with random signs -- no block of the reference near zero, no symmetry"""
    if kind == "sine":
        return None
    rng = np.random.default_rng(1000 + n + seed)
    return rng.uniform(0.25, 1.0, 2 * n) * rng.choice([-1.0, 1.0], 2 * n)


def _coeffs(B, F, n, dtype, seed=0):
    return np.random.default_rng(B * 7919 + F * 31 + n + seed).uniform(-1.0, 1.0, (B, F, n)).astype(NP[dtype])


@functools.lru_cache(maxsize=None)
def _tile(n, dtype):
    probe = mf.plan_imdct(dtype, 1, 2, n)
    tile = probe.pass_geometry(2)[0]
    probe.close()
    return tile


def _lengths(F, n):
    return sorted({(F - 1) * n, (F - 2) * n + 1, 2} - {0, 1})


# ---- values -------------------------------------------------------------------------------------------------------------------
SIZES = [(8, torch.float32), (30, torch.float32), (256, torch.float32), (1024, torch.float32), (8192, torch.float32),
         (8, torch.float64), (1024, torch.float64)]


@pytest.mark.parametrize("window", ["sine", "random"])
@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("n,dtype", SIZES, ids=lambda v: str(v))
def test_matches_the_definition(n, dtype, norm, window):
    """one block per entry; a carry inside an entry (F = TILE + 1), a ragged last tile, entry boundaries inside a run
    (B = 5, F = 2 TILE + 3); with TILE = 1 (n = 8192) F = 5 hands a carry on at every tile.  Every length: all blocks, a last
    block of one sample, and T = 2"""
    tile = _tile(n, dtype)
    w = _window(window, n)
    shapes = [(3, 2)] + [(B, F) for F in sorted({tile, tile + 1, 2 * tile + 3}) if F >= 2 for B in (1, 5)]
    if tile == 1:
        assert (5, 5) in shapes
    worst = 0.0
    for B, F in shapes:
        Xh = _coeffs(B, F, n, dtype)
        ref = _ref(Xh, n, w, norm)
        X = torch.from_numpy(Xh).to(DEV).reshape(B, F, n, 1)
        for T in _lengths(F, n):
            plan = mf.plan_imdct(dtype, B, F, n, length=T, window=w, norm=norm)
            assert plan.in_shape == (B, F, n, 1) and plan.out_shape == (B, T, 1)
            geo = plan.pass_geometry(2)
            assert geo[0] == tile and geo[2] == B * -(-F // tile), geo
            got = _exec_guarded(plan, X).cpu().numpy()
            assert np.isfinite(got).all(), (B, F, T)
            err = _block_err(got, ref, n)
            worst = max(worst, err)
            assert err <= TOL[dtype], (n, dtype, B, F, T, err, plan.kernel_name(2), geo)
            plan.close()
    print(f"imdct n={n} {dtype} norm={norm} window={window} tile={tile}: worst block rel L2 {worst:.3e} over {shapes}")


def test_the_plan_reports_one_launch_and_its_kernel():
    n, B, F = 256, 3, 7
    plan = mf.plan_imdct(torch.float32, B, F, n)
    name = plan.kernel_name(2)
    assert name.startswith("rows256_dct4_") and name.endswith("_imdct_jit"), name
    assert plan.kernel_name(0) == "none" and plan.kernel_name(1) == "none"
    assert plan.stages(0) == [] and plan.stages(1) == [] and int(np.prod(plan.stages(2))) == n // 2
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert plan.in_bytes == B * F * n * 4 and plan.out_bytes == B * (F - 1) * n * 4
    tile, threads, n_tiles, grid = plan.pass_geometry(2)
    assert n_tiles == B * -(-F // tile) and 1 <= grid <= n_tiles and threads % 64 == 0
    assert plan.pass_geometry(2, 2)[2] == 2 * -(-F // tile)
    plan.close()
    p64 = mf.plan_imdct(torch.float64, 2, 3, 1024)
    assert p64.kernel_name(2).startswith("rows1024_f64_dct4_") and p64.kernel_name(2).endswith("_imdct_jit")
    p64.close()


def test_the_largest_length_that_plans():
    n, B, F = 16384, 2, 3
    w = _window("random", n)
    Xh = _coeffs(B, F, n, torch.float32)
    plan = mf.plan_imdct(torch.float32, B, F, n, window=w)
    assert plan.kernel_name(2).startswith("rows16384_dct4_") and plan.kernel_name(2).endswith("_imdct_jit")
    got = _exec_guarded(plan, torch.from_numpy(Xh).to(DEV).reshape(B, F, n, 1)).cpu().numpy()
    assert np.isfinite(got).all()
    err = _block_err(got, _ref(Xh, n, w, None), n)
    print(f"imdct n=16384: block rel L2 {err:.3e} {plan.kernel_name(2)} geometry={plan.pass_geometry(2)}")
    assert err <= REL_L2_TOL_F32
    plan.close()
    with pytest.raises(mf.MifftError) as e:  # fp64 rows end at 12288 points (a 96-KiB tile)
        mf.plan_imdct(torch.float64, B, F, n)
    assert e.value.status == -15


# ---- runs ---------------------------------------------------------------------------------------------------------------------
def test_runs_warm_up_frames_and_entry_boundaries():
    """n = 8: more than three tiles per workgroup, two tiles per entry (the second ragged), so that runs of three and four tiles
    start at an entry and inside one alternately and every run crosses an entry boundary"""
    n = 8
    tile = _tile(n, torch.float32)
    F = tile + 3
    probe = mf.plan_imdct(torch.float32, 1, F, n)
    G = probe.pass_geometry(2, FAR)[3]
    probe.close()
    B = (3 * G + G // 2 + 3) // 2 + 1
    while (2 * B) % G == 0:
        B += 1
    w = _window("random", n)
    plan = mf.plan_imdct(torch.float32, B, F, n, window=w)
    t, threads, n_tiles, grid = plan.pass_geometry(2)
    assert (t, n_tiles, grid) == (tile, 2 * B, G) and n_tiles > 3 * grid, (t, n_tiles, grid)
    runs = mf.istft_schedule(plan)
    assert len(runs) == grid and sum(r[1] for r in runs) == n_tiles
    tpe = -(-F // tile)
    assert tpe == 2 and F % tile != 0                                             # a ragged last tile in every entry
    assert min(r[1] for r in runs) >= 3                                           # runs of three or more tiles
    assert any(r[0] % tpe != 0 and r[2] == 1 for r in runs)                       # a run starting inside an entry: a warm-up frame
    assert any(r[0] % tpe == 0 and r[2] == 0 for r in runs[1:])                   # ... and one starting at an entry
    assert all((r[0] + r[1] - 1) // tpe > r[0] // tpe for r in runs)              # every run crosses an entry boundary
    assert B * F * n * 4 < 32 << 20
    Xh = _coeffs(B, F, n, torch.float32)
    got = _exec_guarded(plan, torch.from_numpy(Xh).to(DEV).reshape(B, F, n, 1)).cpu().numpy()
    assert np.isfinite(got).all()
    err = _block_err(got, ref_imdct(Xh, n, w, None), n)
    print(f"imdct runs: B={B} F={F} tile={tile} n_tiles={n_tiles} grid={grid} runs of {min(r[1] for r in runs)}.."
          f"{max(r[1] for r in runs)} tiles, {sum(r[2] for r in runs)} warm-up frames: block rel L2 {err:.3e}")
    assert err <= REL_L2_TOL_F32
    plan.close()


# ---- bit identity and containment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 256])
def test_an_entry_is_bit_identical_for_any_batch_and_slab(n):
    """first = 2, count = 2 of a batch of 5; the same entries of the whole batch; a plan of the slab's own batch.  The other
    entries of X hold NaN during the slab exec and their outputs stay NaN"""
    tile = _tile(n, torch.float32)
    B, F = 5, 2 * tile + 3
    T = (F - 2) * n + 1
    w = _window("random", n, 1)
    Xh = _coeffs(B, F, n, torch.float32, 1)
    ref = _ref(Xh, n, w, "ortho")
    plan = mf.plan_imdct(torch.float32, B, F, n, length=T, window=w, norm="ortho")
    whole = _exec_guarded(plan, torch.from_numpy(Xh).to(DEV).reshape(B, F, n, 1))
    assert _block_err(whole.cpu().numpy(), ref, n) <= REL_L2_TOL_F32
    Xn = Xh.copy()
    Xn[[0, 1, 4]] = np.nan
    slab = _exec_guarded(plan, torch.from_numpy(Xn).to(DEV).reshape(B, F, n, 1), first=2, count=2)
    assert torch.isnan(slab[[0, 1, 4]]).all()
    assert torch.isfinite(slab[2:4]).all()
    assert torch.equal(_bits(slab[2:4].contiguous()), _bits(whole[2:4].contiguous()))
    assert _block_err(slab[2:4].cpu().numpy(), ref[2:4], n) <= REL_L2_TOL_F32
    small = mf.plan_imdct(torch.float32, 2, F, n, length=T, window=w, norm="ortho")
    alone = _exec_guarded(small, torch.from_numpy(np.ascontiguousarray(Xh[2:4])).to(DEV).reshape(2, F, n, 1))
    assert torch.equal(_bits(alone.contiguous()), _bits(whole[2:4].contiguous()))
    # ... and as the slab of a larger whole batch, whose grid is sized for all of it
    part = mf.plan_imdct(torch.float32, 2, F, n, length=T, window=w, norm="ortho", whole_batch=4096)
    other = _exec_guarded(part, torch.from_numpy(np.ascontiguousarray(Xh[2:4])).to(DEV).reshape(2, F, n, 1))
    assert torch.equal(_bits(other.contiguous()), _bits(whole[2:4].contiguous()))
    for p in (plan, small, part):
        p.close()


# ---- round trip ----------------------------------------------------------------------------------------------------------------
def _rel_rows(got, ref):
    g = np.asarray(got, dtype=np.float64).reshape(-1, got.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [30, 256, 1024])
def test_imdct_of_mdct_reproduces_the_signal(n, dtype, norm):
    """the sine window on both sides (TDAC), T no multiple of n, a leading shape (2, 3, T); tolerances as test_gpu_mdct.py"""
    T = 5 * n + 7
    x = torch.randn((2, 3, T), dtype=dtype, device=DEV)
    X = mf.mdct(x, n, norm=norm)
    F = mf.mdct_frames(T, n)
    assert X.shape == (2, 3, F, n)
    y = mf.imdct(X, norm=norm, length=T)
    assert y.shape == x.shape and y.dtype == dtype and y.is_contiguous()
    xn = x.cpu().numpy().reshape(-1, T)
    assert _rel_rows(y.cpu().numpy().reshape(-1, T), xn) <= TOL[dtype]
    full = mf.imdct(X, norm=norm)  # length defaults to (F - 1) n: the signal, then the zeros the last frames saw
    L = (F - 1) * n
    padded = np.zeros((xn.shape[0], L))
    padded[:, :T] = xn
    assert full.shape == (2, 3, L) and _rel_rows(full.cpu().numpy().reshape(-1, L), padded) <= TOL[dtype]


# ---- mf.imdct -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [8, 1024])
def test_imdct_runs_the_plan_and_agrees_with_the_composition(n, dtype):
    tile = _tile(n, dtype)
    B, F = 3, tile + 2
    T = (F - 2) * n + 5
    w = _window("random", n, 2)
    Xh = _coeffs(B, F, n, dtype, 2)
    X = torch.from_numpy(Xh).to(DEV)
    for norm in NORMS:
        got = mf.imdct(X, window=w, norm=norm, length=T)
        assert got.shape == (B, T) and got.dtype == dtype
        plan = mf.plan_imdct(dtype, B, F, n, length=T, window=w, norm=norm)
        assert plan.num_launches == 1 and plan.scratch_bytes == 0 and plan.kernel_name(2).endswith("_imdct_jit")
        out = _exec_guarded(plan, X.reshape(B, F, n, 1))
        assert torch.equal(_bits(got.contiguous()), _bits(out.contiguous()))
        ref = _ref(Xh, n, w, norm)
        assert _block_err(got.cpu().numpy(), ref, n) <= TOL[dtype]
        wt = torch.from_numpy(w)
        composed = mf.api._imdct_composed(X, wt, norm == "ortho", T)
        assert composed.shape == got.shape and _block_err(composed.cpu().numpy(), ref, n) <= TOL[dtype]
        # length 1 is what the fused plan refuses: the composition serves it
        one = mf.imdct(X, window=w, norm=norm, length=1)
        assert one.shape == (B, 1)
        assert np.abs(one.cpu().numpy().astype(np.float64) - ref[:, :1]).max() <= TOL[dtype] * np.linalg.norm(ref[:, :n], axis=1).max()
        plan.close()


def test_a_window_changed_in_place_never_meets_a_stale_plan():
    n = 8
    X = torch.randn(2, 9, n, device=DEV)
    w = mf.mdct_window(n).clone()
    a = mf.imdct(X, window=w)
    w.mul_(2.0)
    b = mf.imdct(X, window=w)
    assert _rel_rows(b.cpu().numpy(), 2 * a.cpu().numpy().astype(np.float64)) <= REL_L2_TOL_F32
    assert torch.equal(mf.imdct(X), mf.imdct(X, window=mf.mdct_window(n)))
    assert imdct_gain(n, None) == 2.0 / n
